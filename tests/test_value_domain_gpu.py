"""GPU (MI355X): signed, wide-range and non-finite data through every kernel family, through the C ABI -- the table of
tests/value_domain.py (test_value_domain_host.py checks the table and runs it through the CPU replays).

Per case: aai_last_kernel() names the family the case was built for; seven finite images (normal, offset, sign-mixed log-normal, x1e30,
x1e-30, checker, negative constant) against the oracle under the magnitude-scaled bound |got - oracle(src)| <= TOL max(oracle(|src|),
1e-3 max|src|), exact zeros where oracle(|src|) is 0; then NaN, +Inf and -Inf on combs of source pixels (of gradient pixels, for the
adjoints): non-finite exactly on the oracle's support, and outside it the bits of the run with those pixels at 0.  Host entries for
plain fp32 images; the device entries on the current stream for batches, row bands, typed and interleaved images and every adjoint.
Every mask and value expected here is the oracle's (value_domain.py).  Nothing here reads outside the repository."""
import collections

import numpy as np
import pytest

import value_domain as vd

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _upload(a, pad):
    """an [H, row] host image -> a device tensor with `pad` elements of row padding; (tensor, row stride)"""
    import torch
    H, row = a.shape[0], int(np.prod(a.shape[1:]))
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16}[a.dtype]
    t = torch.zeros((H, row + pad), dtype=tdt, device="cuda")
    flat = np.ascontiguousarray(a).reshape(H, row)
    t[:, :row] = torch.from_numpy(flat.view(np.int16) if a.dtype == np.uint16 else flat).cuda()
    return t, row + pad


def _group(c):
    w = c.name.split()
    return "k1 empty at %g" % c.ang if c.name.startswith("k1 empty") and c.via == "host" else ("k1 other" if w[0] == "k1" else w[0])


def _forward_run(gpu, po, c):
    """run(src) -> dst through the entry the case names; every call asserts the kernel family"""
    import torch
    from area_average_interpolation_amd import _lib as L
    rq = vd.fwd_request(gpu, c)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    dW, dH, C = lay.dst_width, lay.dst_height, c.C
    code = {"f32": L.DTYPE_F32, "u8": L.DTYPE_U8, "u16": L.DTYPE_U16}[c.T]
    bands = None
    if c.band:
        band = vd.band_of(po, c, lay)
        bands = [band, (0, band[0]) if band[0] else (band[1], dH)]

    def named():
        assert c.kernel in gpu.last_kernel(), (c.name, gpu.last_kernel())

    def run(src):
        if c.via == "host":
            gpu.debug_cell_min_waves(0 if c.cell else -1)
            try:
                rc, msg, dst, _, _ = gpu.resample_host(src, c.sr, c.dr, c.iso, c.ang, mode=c.mode, policy=c.policy)
            finally:
                gpu.debug_cell_min_waves(-1)
            assert rc == 0 and dst.shape == (dH, dW), (c.name, msg)
            named()
            return dst
        extra = L.POLICY_PREFER_CELL if c.cell else 0
        rqd = gpu.make_request(c.W, c.H, c.sr, c.dr, c.iso, c.ang, mode=c.mode, policy=c.policy | extra)
        t, stride = _upload(src, pad=5)
        dpad = 3
        if bands:
            out = np.empty((dH, dW), np.float32)
            for (r0, r1) in bands:
                a, b = gpu.band_source_rows(rqd, r0, r1)
                d = torch.full((r1 - r0, dW + dpad), SENTINEL, dtype=torch.float32, device="cuda")
                gpu.resample_band_device(rqd, r0, r1, t.data_ptr() + 4 * a * stride, stride, d.data_ptr(), dW + dpad, _stream())
                torch.cuda.synchronize()
                named()
                h = d.cpu().numpy()
                assert (h[:, dW:] == SENTINEL).all(), c.name
                out[r0:r1] = h[:, :dW]
            return out
        batch = 2 if (C == 1 and c.T == "f32") else 1
        if batch == 2:
            t = torch.stack([t, t]).contiguous()
        d = torch.full((batch, dH, dW * C + dpad), SENTINEL, dtype=torch.float32, device="cuda")
        if C == 1:
            gpu.resample_device(rqd, t.data_ptr(), stride, d.data_ptr(), dW + dpad, _stream(), batch=batch, src_image_stride=c.H * stride,
                                dst_image_stride=dH * (dW + dpad), src_dtype=code)
        else:
            gpu.resample_interleaved_device(rqd, C, t.data_ptr(), stride, d.data_ptr(), dW * C + dpad, _stream(), batch=1, src_dtype=code)
        torch.cuda.synchronize()
        named()
        h = d.cpu().numpy()
        assert (h[:, :, dW * C:] == SENTINEL).all(), (c.name, "the padding of the dst rows was written")
        assert all(np.array_equal(h[0].view(np.int32), h[b].view(np.int32)) for b in range(batch)), c.name
        return h[0, :, :dW * C].reshape((dH, dW) if C == 1 else (dH, dW, C)).copy()
    return run


@pytest.fixture(scope="module")
def fwd(gpu, hostemu, knife_golden):
    groups = collections.OrderedDict()
    for c in vd.forward_cases(gpu, hostemu, knife_golden[1]):
        groups.setdefault(_group(c), []).append(c)
    return groups


FORWARD_GROUPS = ["k1 empty at 0", "k1 empty at 90", "k1 empty at 180", "k1 empty at 270", "k1 other", "quad", "cell", "wide", "f64", "fix-up",
                  "bilinear", "bicubic"]


def test_the_forward_groups_are_the_table(fwd):
    assert sorted(fwd) == sorted(FORWARD_GROUPS)


@pytest.mark.parametrize("group", FORWARD_GROUPS)
def test_forward_families(gpu, po, fwd, group):
    import re
    worst, runs, cover, excused = 0.0, 0, 0, 0
    for c in fwd[group]:
        run = _forward_run(gpu, po, c)
        err = vd.check_forward_finite(po, gpu, c, run)
        worst = max(worst, err)
        line = "%-40s %-32s scaled err %.2e" % (c.name, gpu.last_kernel(), err)
        if c.T == "f32" and not vd.not_local(c):
            r, n, x = vd.check_forward_locality(po, gpu, c, run)
            runs, cover, excused = runs + r, cover + n, excused + x
            line += "  %d poisoned runs, %d support pixels" % (r, n)
        if c.name.startswith("fix-up"):
            m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(vd.fwd_request(gpu, c)))
            assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, (c.name, gpu.plan_shape(vd.fwd_request(gpu, c)))
            line += "  " + m.group(0)
        print(line)
    print("%s: worst magnitude-scaled error %.2e, %d poisoned runs, %d support pixels, %d excused" % (group, worst, runs, cover, excused))
    assert excused == 0


NOT_LOCAL_CASES = vd.NOT_LOCAL_CASES


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.xfail(strict=True, raises=AssertionError, reason=r)) for n, r in NOT_LOCAL_CASES])
def test_locality_of_the_families_left_as_they_are(gpu, po, fwd, name):
    """the locality check of the cases value_domain.NOT_LOCAL_CASES names, one item each: expected to fail its assertion, and to say so
    the day it does not"""
    (c,) = [c for g in fwd.values() for c in g if c.name == name]
    run = _forward_run(gpu, po, c)
    run(vd.image("normal", c.H, c.W))                      # (kernel name, return code and shape are asserted outside the expected failure)
    try:
        vd.check_forward_locality(po, gpu, c, run)
    except AssertionError as e:
        if "non-finite where the oracle has no weight" not in str(e):
            raise RuntimeError("failed, but not on a leak: %s" % (e,))           # (not the expected failure)
        raise


def test_dense_form_of_the_fixup_pass(gpu):
    """AAI_MAX_LISTED_PIXELS=10 in a fresh child process (the hook is read once): value_domain.dense_child -- the two fix-up cases with the
    whole image in the strict double-precision pass, finite data and locality against the oracle"""
    import os
    import subprocess
    import sys
    gpu.shutdown()
    env = dict(os.environ, AAI_MAX_LISTED_PIXELS="10")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "value_domain.py")], capture_output=True, text=True,
                       env=env, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "dense ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    assert sum(1 for l in p.stdout.splitlines() if l.startswith("dense fix-up") and "strict" in l) == len(vd.KNIFE_FIXUP)


def _adjoint_run(gpu, c):
    """run(gdst) -> gsrc through the device entry of the case's family, on the current stream"""
    import torch
    rq = vd.adj_request(gpu, c)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    dW, dH, C = lay.dst_width, lay.dst_height, c.C

    def run(g):
        gt, gstride = _upload(np.ascontiguousarray(g, dtype=np.float32), pad=3)
        out = torch.full((c.H, c.W * C + 5), SENTINEL, dtype=torch.float32, device="cuda")
        args = (gt.data_ptr(), gstride, out.data_ptr(), c.W * C + 5, _stream())
        if c.family == "sample":
            if C == 1:
                gpu.adjoint_sample_device(rq, *args)
            else:
                gpu.adjoint_sample_interleaved_device(rq, C, *args)
        elif C == 1:
            gpu.adjoint_device(rq, *args, planned={"general": False, "planned": True, "any": "any"}[c.family])
        else:
            gpu.adjoint_interleaved_device(rq, C, *args, planned={"general": False, "any": "any", "separable": "separable"}[c.family])
        torch.cuda.synchronize()
        assert c.kernel in gpu.last_kernel(), (c.name, gpu.last_kernel())
        h = out.cpu().numpy()
        assert (h[:, c.W * C:] == SENTINEL).all(), (c.name, "the padding of the gradient's rows was written")
        return h[:, :c.W * C].reshape((c.H, c.W) if C == 1 else (c.H, c.W, C)).copy()
    return run


ADJ = vd.adjoint_cases()
ADJ_GROUPS = list(collections.OrderedDict((a.family, None) for a in ADJ))


@pytest.mark.parametrize("family", ADJ_GROUPS)
def test_adjoint_families(gpu, po, family):
    worst = 0.0
    for c in ADJ:
        if c.family != family:
            continue
        run = _adjoint_run(gpu, c)
        err = vd.check_adjoint_finite(po, gpu, c, run)
        runs, cover, unread = vd.check_adjoint_locality(po, gpu, c, run)
        worst = max(worst, err)
        print("%-36s %-44s scaled err %.2e  %d poisoned runs, %d support pixels, %d poisoned dst pixels nothing reads"
              % (c.name, gpu.last_kernel(), err, runs, cover, unread))
    print("adjoint %s: worst magnitude-scaled error %.2e, 0 excused" % (family, worst))
