"""The planned adjoint at general rotations on the MI355X: aai_adjoint_rotated_batch_device_f32 / aai_adjoint_rotated_f32 /
aai_adjoint_rotated_prepare and torch_ops.resample(..., planned_backward="any").

The bar everywhere: the int32 view of gsrc equals that of adjoint_device(planned=False) -- the general adjoint -- on the same gradient.
No tolerance is involved, except where one case is ALSO held against the oracle's matrix (test_adjoint_host.assert_adjoint_matches) so
that the file does not rest on the general adjoint alone.  Images have a few thousand pixels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from guard_layout import GuardedLayout, to_device
from test_adjoint_host import EIGHT, adjoint_gold, assert_adjoint_matches
from test_adjoint_rotated_host import KNIFE_STRIDE

pytestmark = pytest.mark.gpu

PLAIN_KERNEL = "aai_adjoint_plain_gather_kernel"
GATHER_KERNEL = "aai_adjoint_gather_kernel"
AXIS_KERNEL = "aai_axis_adjoint_kernel"


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    yield aai
    torch.cuda.synchronize()
    aai.shutdown()                 # the plans of this module (and their tables) do not outlive it


def _run(gpu, rq, g, planned="any"):
    """the device entry on a host gradient image, gsrc prefilled with -1; (gsrc on the host, aai_last_kernel())"""
    import torch
    gd = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
    gs = torch.full((rq.src_height, rq.src_width), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), gd.shape[1], gs.data_ptr(), rq.src_width, torch.cuda.current_stream().cuda_stream, batch=1, planned=planned)
    torch.cuda.synchronize()
    return gs.cpu().numpy(), gpu.last_kernel()


def _gradient(gpu, rq, seed=3):
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    return np.random.default_rng(seed).random((lay.dst_height, lay.dst_width)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_as_general(gpu, rq, what, seed=3):
    """the new entry and the general entry on one gradient: equal bits; returns (gsrc, kernel of the new entry)"""
    g = _gradient(gpu, rq, seed)
    got, kernel = _run(gpu, rq, g)
    ref, kref = _run(gpu, rq, g, planned=False)
    assert GATHER_KERNEL in kref, kref
    diff = int((_bits(got) != _bits(ref)).sum())
    assert diff == 0, (what, kernel, "%d of %d source pixels differ from the general adjoint" % (diff, got.size), gpu.plan_shape(rq))
    assert (got >= 0).all(), what                               # every pixel written (weights and gradients are non-negative)
    return got, kernel


def _knife(gpu, rq):
    m = re.search(r"rot_adjoint=(\w+)(?: knife=(\d+))?$", gpu.plan_shape(rq))
    assert m, gpu.plan_shape(rq)
    return m.group(1), int(m.group(2)) if m.group(2) else None


MODES = lambda gpu: ((gpu.MODE_AREA, gpu.POLICY_REFERENCE), (gpu.MODE_AREA, gpu.POLICY_EXACT), (gpu.MODE_FAST, gpu.POLICY_REFERENCE))
GENERAL_EIGHT = [c for c in EIGHT if c[4] % 90 != 0]


# 1.  basic geometries
@pytest.mark.parametrize("case", range(len(GENERAL_EIGHT)))
def test_rotated_adjoint_has_the_general_adjoints_bits(gpu, po, case):
    W, H, sr, dr, ang, off = GENERAL_EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mode, policy in MODES(gpu):
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
        got, kernel = _same_as_general(gpu, rq, "case %d mode %d policy %d" % (case, mode, policy))
        print("case %d mode %d policy %d: %s, %s" % (case, mode, policy, kernel, gpu.plan_shape(rq)))
        state, knife = _knife(gpu, rq)
        if case == 2:                    # 45 degrees on a 1:2 lattice is grid-aligned: whatever serves it (the bits are the general's)
            assert kernel.startswith(PLAIN_KERNEL) or GATHER_KERNEL in kernel
            continue
        assert kernel.startswith(PLAIN_KERNEL), (kernel, gpu.plan_shape(rq))
        assert state == "sums" and "rot_adjoint=sums" in gpu.plan_shape(rq) and knife is not None
        assert kernel.endswith("+listed") == (knife > 0)
    # the host-buffer entry gives the device entry's bits
    rq = gpu.make_request(W, H, sr, dr, iso, ang)
    g = _gradient(gpu, rq)
    rc, msg, gsrc = gpu.adjoint_host(g, (H, W), sr, dr, iso, ang, planned="any")
    assert rc == 0, msg
    assert np.array_equal(_bits(gsrc), _bits(_run(gpu, rq, g)[0]))
    if case == 0:                        # ... and one case against the oracle's matrix
        for mode, policy in MODES(gpu):
            g, gold = adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, mode, policy)
            got, kernel = _run(gpu, gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy), g)
            assert kernel.startswith(PLAIN_KERNEL)
            assert_adjoint_matches(got, gold, "rotated entry against the oracle, mode %d policy %d" % (mode, policy))


def test_rotated_adjoint_on_the_92_by_68_geometry(gpu):
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(92, 68, 3.0, 1.0, (45.5, 33.5), 17.5, mode=mode)
        got, kernel = _same_as_general(gpu, rq, "92 x 68 mode %d" % mode)
        assert kernel.startswith(PLAIN_KERNEL) and "rot_adjoint=sums" in gpu.plan_shape(rq), (kernel, gpu.plan_shape(rq))


# 2.  tile edges and replication
@pytest.mark.parametrize("side", [15, 16, 17, 33])
def test_rotated_adjoint_at_tile_edges(gpu, side):
    """source sides on both sides of the 16 x 16 workgroup and of two of them; the dst sizes (3:2 and 1:1 at 17.5 and 30 degrees: 14 to
    46 pixels a side) leave partial 16 x 16 tiles of the one-off sums kernel and partial 64 x 4 tiles of the element-wise pass"""
    plain = 0
    for (W, H) in ((side, side), (side, 21), (19, side)):
        for sr, dr, ang in ((3, 2, 17.5), (1, 1, 30.0)):
            for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
                rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2), ang, mode=mode)
                lay = gpu.query(rq)[2]
                assert lay.dst_width % 16 or lay.dst_height % 16
                _, kernel = _same_as_general(gpu, rq, "tile edges %dx%d %g:%g %g mode %d" % (W, H, sr, dr, ang, mode))
                plain += kernel.startswith(PLAIN_KERNEL)
    assert plain >= 10


@pytest.mark.parametrize("ang", [17.5, 107.5, 197.5, 287.5])
def test_rotated_adjoint_of_replicated_sources_in_every_quadrant(gpu, ang):
    """x2 and x3 up-sampling (scale > 1): adjoint_virtual_pixel's four branches"""
    for (W, H, dr) in ((29, 23, 2), (19, 17, 3)):
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(W, H, 1, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            assert gpu.query(rq)[2].scale > 1 and gpu.query(rq)[2].quadrant == int(ang // 90)
            _, kernel = _same_as_general(gpu, rq, "x%d at %g mode %d" % (dr, ang, mode))
            assert kernel.startswith(PLAIN_KERNEL), kernel


def test_rotated_adjoint_with_the_isocenter_outside_and_at_40_to_1(gpu):
    for (W, H, sr, dr, iso, ang) in ((60, 50, 3, 1, (-90.0, 70.0), 17.5), (50, 60, 1, 2, (115.0, -45.0), 215.0), (200, 130, 40, 1, (99.5, 64.5), 17.5)):
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
            _, kernel = _same_as_general(gpu, rq, "%dx%d %g:%g iso %r mode %d" % (W, H, sr, dr, iso, mode))
            assert kernel.startswith(PLAIN_KERNEL), kernel


# 3.  knife fixtures
def test_rotated_adjoint_on_knife_edge_geometries(gpu, knife_golden):
    """the stride tests/test_adjoint_rotated_host.py fixed on the CPU; which path served a geometry is the plan's choice and is counted"""
    manifest = knife_golden[1]
    ran = plain = listed = general = 0
    for i in range(0, len(manifest), KNIFE_STRIDE):             # a fixed stride by index, never a choice by outcome
        c = manifest[i]
        if c["W"] * c["H"] > 1300:
            continue
        ran += 1
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode)
            _, kernel = _same_as_general(gpu, rq, "knife %d mode %d" % (i, mode))
            state, knife = _knife(gpu, rq)
            if kernel.startswith(PLAIN_KERNEL):
                assert state == "sums" and kernel.endswith("+listed") == (knife > 0), (kernel, gpu.plan_shape(rq))
                plain, listed = plain + 1, listed + kernel.endswith("+listed")
            else:
                assert GATHER_KERNEL in kernel and state == "general", (kernel, gpu.plan_shape(rq))
                general += 1
    print("%d geometries, %d calls: %d served by %s (%d of them with the listed pass), %d by the general adjoint" % (ran, 2 * ran, plain, PLAIN_KERNEL, listed, general))
    assert ran >= 20 and listed >= 3 and plain - listed >= 1 and plain + general == 2 * ran


# 4.  fall-backs
def test_rotated_adjoint_near_the_axes_and_on_a_grid_aligned_lattice(gpu):
    """whatever serves them, the bits are the general adjoint's"""
    for (W, H, sr, dr, ang) in ((40, 30, 3, 1, 0.01), (40, 30, 3, 1, 89.99), (32, 32, 2, 1, 45.0), (16, 12, 1, 2, 45.0)):
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            _, kernel = _same_as_general(gpu, rq, "%dx%d %g mode %d" % (W, H, ang, mode))
            state, _ = _knife(gpu, rq)
            print("%dx%d at %g mode %d: %s, %s" % (W, H, ang, mode, kernel, gpu.plan_shape(rq)))
            assert (kernel.startswith(PLAIN_KERNEL) and state == "sums") or (GATHER_KERNEL in kernel and state == "general")


def test_rotated_adjoint_at_reduced_angle_0_is_the_planned_adjoint(gpu):
    for (W, H, sr, dr, ang) in ((24, 24, 4, 1, 0.0), (40, 30, 2.5, 1, 90.0), (20, 16, 2, 1, 180.0)):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
        g = _gradient(gpu, rq)
        got, kernel = _run(gpu, rq, g)
        ref, kref = _run(gpu, rq, g, planned=True)
        assert kernel.startswith(AXIS_KERNEL) and kernel == kref, (kernel, kref)
        assert np.array_equal(_bits(got), _bits(ref))
        assert "adjoint=tables" in gpu.plan_shape(rq) and "rot_adjoint=none" in gpu.plan_shape(rq)


LIMIT_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch            # (before the library: one HIP runtime per process)
import area_average_interpolation_amd as aai
import test_adjoint_rotated_gpu as m
aai.set_device(0)
c = %r
for mode in (aai.MODE_AREA,):
    rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode)
    aai.adjoint_rotated_prepare(rq)
    state, knife = m._knife(aai, rq)
    assert state == "general" and knife > 3, aai.plan_shape(rq)
    got, kernel = m._same_as_general(aai, rq, "limit 3")
    assert m.GATHER_KERNEL in kernel, kernel
print("limit ok")
"""


def test_rotated_adjoint_beyond_the_listed_limit_is_the_general_adjoint(gpu, knife_golden):
    """AAI_MAX_LISTED_PIXELS=3 (the library reads it once -- hence a child process): a geometry whose K holds 13 pixels, served with the
    listed pass in this process, takes the general path whole there and reports rot_adjoint=general"""
    c = knife_golden[1][24]
    rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"])
    _, kernel = _same_as_general(gpu, rq, "knife 24")
    assert kernel == PLAIN_KERNEL + "<area>+listed" and _knife(gpu, rq)[1] > 3, (kernel, gpu.plan_shape(rq))
    env = dict(os.environ, AAI_MAX_LISTED_PIXELS="3")
    p = subprocess.run([sys.executable, "-c", LIMIT_CHILD % (ROOT, os.path.join(ROOT, "tests"), dict(c))], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "limit ok" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])


# 5.  determinism and batches.  One geometry whose K is empty and one whose K is not (knife fixture 24, see the host test)
CLEAN = (92, 68, 3.0, 1.0, (45.5, 33.5), 17.5)


def _clean_and_knife(gpu, knife_golden):
    c = knife_golden[1][24]
    return [CLEAN, (c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"])]


def test_rotated_adjoint_is_deterministic_and_batches_match_single_images(gpu, knife_golden):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    seen = set()
    for geo, mode in zip(_clean_and_knife(gpu, knife_golden) + [CLEAN], (gpu.MODE_AREA, gpu.MODE_AREA, gpu.MODE_FAST)):
        rq = gpu.make_request(*geo, mode=mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        B = 5
        dstride, sstride = dW + 3, W + 5
        dimg, simg = dstride * dH + 17, sstride * H + 11              # image strides greater than H x stride
        gen = torch.Generator(device="cuda").manual_seed(21)
        gd = torch.rand(B * dimg, dtype=torch.float32, device="cuda", generator=gen)      # distinct gdst per image
        outs = []
        for planned in ("any", "any", False):
            gs = torch.full((B * simg,), -7.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_device(rq, gd.data_ptr(), dstride, gs.data_ptr(), sstride, st, batch=B, dst_image_stride=dimg, src_image_stride=simg, planned=planned)
            torch.cuda.synchronize()
            if planned:
                kernel = gpu.last_kernel()
            outs.append(gs)
        assert kernel.startswith(PLAIN_KERNEL), kernel
        seen.add(kernel.endswith("+listed"))
        assert torch.equal(outs[0], outs[1])                           # two runs give equal results
        assert torch.equal(outs[0], outs[2])                           # ... and the general adjoint's batch, padding included
        gs = outs[0]
        touched = torch.zeros(B * simg, dtype=torch.bool, device="cuda")
        for b in range(B):
            one_g = gd[b * dimg:b * dimg + dstride * dH].view(dH, dstride)[:, :dW].contiguous()
            one = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_device(rq, one_g.data_ptr(), dW, one.data_ptr(), W, st, planned="any")
            torch.cuda.synchronize()
            assert torch.equal(gs[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W], one), (geo, mode, b)
            touched[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W] = True
        assert bool((gs[~touched] == -7.0).all())          # padding and gaps untouched
        assert bool((gs[touched] >= 0.0).all())            # every pixel written
    assert seen == {False, True}


def test_rotated_adjoint_batch_of_two_scratch_chunks(gpu):
    """the fp64 scratch is cut at 1 GiB as in enqueue_adjoint (test_adjoint_batch_of_several_scratch_chunks reaches that with 96 large
    images; here the images are small -- 40 x 30, x2 up-sampled to some 7,600 dst pixels -- and the batch is long): the whole batch equals
    the general adjoint's, and the images on both sides of the cut equal their single-image calls"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    W, H = 40, 30
    rq = gpu.make_request(W, H, 1.0, 2.0, ((W - 1) / 2, (H - 1) / 2), 17.5)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    per_image = dW * dH * 8
    chunk = (1 << 30) // per_image
    batch = chunk + 37
    assert 1 < chunk < 65535 and per_image * batch > (1 << 30) and batch * dW * dH * 4 < (1 << 30)
    gen = torch.Generator(device="cuda").manual_seed(9)
    gd = torch.rand((batch, dH, dW), dtype=torch.float32, device="cuda", generator=gen)
    outs = []
    for planned in ("any", False):
        gs = torch.full((batch, H, W), -7.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, gd.data_ptr(), dW, gs.data_ptr(), W, st, batch=batch, dst_image_stride=dW * dH, src_image_stride=W * H, planned=planned)
        torch.cuda.synchronize()
        if planned:
            assert gpu.last_kernel().startswith(PLAIN_KERNEL), gpu.last_kernel()
        outs.append(gs)
    assert torch.equal(outs[0], outs[1]) and bool((outs[0] >= 0).all())
    for b in (0, chunk - 1, chunk, chunk + 1, batch - 1):
        one = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, gd[b].data_ptr(), dW, one.data_ptr(), W, st, planned="any")
        torch.cuda.synchronize()
        assert torch.equal(outs[0][b], one), b
    del gd, outs
    torch.cuda.empty_cache()


def test_rotated_adjoint_past_grid_z(gpu):
    """the sums path is cut by grid.z where the images are tiny: 65,540 images of 12 x 10 (2:1, 17.5 degrees; 7 x 7 dst pixels, 392 bytes of
    scratch each, so the 1 GiB rule does not cut first).  The images on both sides of the cut equal their single-image calls and the
    general adjoint's, bit for bit."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    W, H = 12, 10
    rq = gpu.make_request(W, H, 2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 17.5)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    batch, cut = 65540, 65535
    assert batch > cut and (1 << 30) // (dW * dH * 8) > batch
    gen = torch.Generator(device="cuda").manual_seed(9)
    gd = torch.rand((batch, dH, dW), dtype=torch.float32, device="cuda", generator=gen)
    outs = []
    for planned in ("any", False):
        gs = torch.full((batch, H, W), -7.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, gd.data_ptr(), dW, gs.data_ptr(), W, st, batch=batch, dst_image_stride=dW * dH, src_image_stride=W * H, planned=planned)
        torch.cuda.synchronize()
        if planned:
            assert gpu.last_kernel().startswith(PLAIN_KERNEL), gpu.last_kernel()
        outs.append(gs)
    assert bool((outs[0] >= 0).all())
    for b in (0, cut - 1, cut, cut + 1, batch - 1):
        one = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, gd[b].data_ptr(), dW, one.data_ptr(), W, st, planned="any")
        torch.cuda.synchronize()
        assert torch.equal(outs[0][b], one) and torch.equal(outs[1][b], one), b


# 6.  guard bands
def test_rotated_adjoint_stays_inside_its_buffers(gpu, knife_golden):
    """gdst is the guarded SOURCE (NaN around it), gsrc the guarded destination (sentinel everywhere), the three layouts of
    tests/test_gpu_memory_contract.py: every pixel of gsrc inside the image finite and equal, bit for bit, to the tight call; nothing
    else written"""
    import torch
    from test_gpu_memory_contract import LAYOUTS, _pad
    st = torch.cuda.current_stream().cuda_stream
    B = 2
    seen = set()
    for i, (geo, mode) in enumerate(zip(_clean_and_knife(gpu, knife_golden) + [CLEAN], (gpu.MODE_AREA, gpu.MODE_AREA, gpu.MODE_FAST))):
        rq = gpu.make_request(*geo, mode=mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        g = np.random.default_rng(5 + i).random((B, dH, dW, 1)).astype(np.float32)
        tg = to_device(g)
        ts = torch.full((B, H, W), float("nan"), dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, tg.data_ptr(), dW, ts.data_ptr(), W, st, batch=B, dst_image_stride=dW * dH, src_image_stride=W * H, planned="any")
        torch.cuda.synchronize()
        kernel = gpu.last_kernel()
        assert kernel.startswith(PLAIN_KERNEL), kernel
        seen.add(kernel.endswith("+listed"))
        tight = ts.cpu().numpy().reshape(B, H, W, 1)
        assert np.isfinite(tight).all()
        for sp, so, sg, dp, do, dg in LAYOUTS:
            gl = GuardedLayout((B, dH, dW, 1), "f32", dW + _pad(dW, dp), dH * (dW + _pad(dW, dp)) + dg, do)
            sl = GuardedLayout((B, H, W, 1), "f32", W + _pad(W, sp), H * (W + _pad(W, sp)) + sg, so)
            gdev, sdev = to_device(gl.make_src(g, "nan")), to_device(sl.make_dst())
            gpu.adjoint_device(rq, gl.ptr(gdev), gl.stride, sl.ptr(sdev), sl.stride, st, batch=B, dst_image_stride=gl.image_stride,
                               src_image_stride=sl.image_stride, planned="any")
            torch.cuda.synchronize()
            what = (gpu.last_kernel(), geo, mode, "gdst stride %d image stride %d base %+d, gsrc stride %d image stride %d base %+d"
                    % (gl.stride, gl.image_stride, gl.base_offset, sl.stride, sl.image_stride, sl.base_offset))
            assert gpu.last_kernel() == kernel, what
            out, first, count = sl.check_dst(sdev)
            assert count == 0, ("%d guard elements of gsrc were written, first: %s" % (count, sl.describe(first)), what)
            assert sl.sentinels_left(out) == 0, what
            bad = ~np.isfinite(out)
            assert not bad.any(), ("%d non-finite gsrc pixels, first at %s" % (int(bad.sum()), np.argwhere(bad)[0].tolist()), what)
            assert np.array_equal(out.view(np.int32), tight.view(np.int32)), what
    assert seen == {False, True}


# 7.  torch operator
def test_torch_operator_with_planned_backward_any(gpu):
    import torch
    from area_average_interpolation_amd import torch_ops
    st = lambda: torch.cuda.current_stream().cuda_stream
    W, H, sr, dr, ang = 84, 60, 3, 1, 17.5                               # a geometry no other test of this module prepares
    iso = ((W - 1) / 2, (H - 1) / 2)
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        B = 3
        gen = torch.Generator(device="cuda").manual_seed(5)
        x = torch.rand((B, H, W), dtype=torch.float32, device="cuda", generator=gen)
        g = torch.rand((B, dH, dW), dtype=torch.float32, device="cuda", generator=gen)
        kw = dict(batch=B, dst_image_stride=dW * dH, src_image_stride=W * H)
        # no gradient wanted: no tables are built, whatever the keyword says
        torch_ops.resample(x, sr, dr, iso, ang, mode=mode, planned_backward="any")
        assert "rot_adjoint=none" in gpu.plan_shape(rq)
        # the default keyword, then True: the existing adjoint, and no tables are built
        grads = []
        for planned in (False, True):
            xd = x.clone().requires_grad_(True)
            yd, _ = torch_ops.resample(xd, sr, dr, iso, ang, mode=mode, planned_backward=planned)
            (yd * g).sum().backward()
            assert "rot_adjoint=none" in gpu.plan_shape(rq)
            grads.append(xd.grad)
        # "any": the forward builds the tables, the backward is the new entry
        xp = x.clone().requires_grad_(True)
        yp, _ = torch_ops.resample(xp, sr, dr, iso, ang, mode=mode, planned_backward="any")
        assert "rot_adjoint=sums" in gpu.plan_shape(rq) and torch.equal(yp.detach(), yd.detach())
        (yp * g).sum().backward()
        # (aai_last_kernel() is per thread and autograd runs the backward on a thread of its own: the kernel is named by the direct call)
        direct = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, g.data_ptr(), dW, direct.data_ptr(), W, st(), planned="any", **kw)
        torch.cuda.synchronize()
        assert gpu.last_kernel().startswith(PLAIN_KERNEL)
        assert torch.equal(xp.grad, direct) and torch.equal(xp.grad, grads[0]) and torch.equal(xp.grad, grads[1])
    # at an axis geometry "any" behaves exactly as True
    args = (2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 180.0)
    rq = gpu.make_request(W, H, *args)
    x = torch.rand((H, W), dtype=torch.float32, device="cuda")
    grads = []
    for planned in ("any", True):
        xx = x.clone().requires_grad_(True)
        y, _ = torch_ops.resample(xx, *args, planned_backward=planned)
        assert "adjoint=tables" in gpu.plan_shape(rq).split()
        y.sum().backward()
        grads.append(xx.grad)
    assert torch.equal(grads[0], grads[1])
    with pytest.raises(ValueError):
        torch_ops.resample(x, *args, planned_backward="sums")


def test_torch_operator_refuses_to_build_rotated_tables_inside_a_capture(gpu, monkeypatch):
    """with the current stream reported as capturing, a rotated geometry that has a plan but no sums raises instead of building them
    (which would synchronise); once they exist the call goes through"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 70, 54
    args = (3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 30.0)                  # a geometry no other test of this module prepares
    rq = gpu.make_request(W, H, *args)
    x = torch.rand((H, W), dtype=torch.float32, device="cuda", requires_grad=True)
    eager, _ = torch_ops.resample(x, *args)                              # the forward's plan, no tables
    assert "rot_adjoint=none" in gpu.plan_shape(rq)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        torch_ops.resample(x, *args, planned_backward="any")
    assert "rot_adjoint=none" in gpu.plan_shape(rq)
    torch_ops.resample(x, *args)                                         # the default keyword needs no tables
    torch_ops.resample(x, *args, planned_backward=True)                  # ... nor does True at a general rotation
    torch_ops.resample(x.detach(), *args, planned_backward="any")        # ... nor a call that wants no gradient
    monkeypatch.undo()
    torch_ops.resample(x, *args, planned_backward="any")                 # builds the tables outside a capture
    assert "rot_adjoint=sums" in gpu.plan_shape(rq)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    again, _ = torch_ops.resample(x, *args, planned_backward="any")
    torch.cuda.synchronize()
    assert torch.equal(again.detach(), eager.detach())


def test_torch_operator_takes_the_planar_route_for_channels_last_input(gpu):
    """(B, 3, H, W) channels_last with planned_backward="any" at a general rotation: the planar route, so x.grad has the planar
    operator's bits plane by plane (and is not channels_last), and the tables are built"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 44, 36
    args = (2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 17.5)
    rq = gpu.make_request(W, H, *args)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand((2, 3, H, W), dtype=torch.float32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    xa = x.clone(memory_format=torch.channels_last).requires_grad_(True)
    ya, _ = torch_ops.resample(xa, *args, planned_backward="any")
    assert "rot_adjoint=sums" in gpu.plan_shape(rq)
    assert ya.is_contiguous()                                            # planar: the interleaved route returns a channels_last y
    g = torch.rand(ya.shape, dtype=torch.float32, device="cuda", generator=gen)
    (ya * g).sum().backward()
    xp = x.contiguous().view(6, H, W).clone().requires_grad_(True)
    yp, _ = torch_ops.resample(xp, *args)
    (yp * g.view(6, *g.shape[2:])).sum().backward()
    assert torch.equal(ya.detach().view(6, *g.shape[2:]), yp.detach())
    assert torch.equal(xa.grad.contiguous().view(6, H, W), xp.grad)
    # the default keyword keeps the interleaved route for the same tensor
    yi, _ = torch_ops.resample(x, *args)
    assert yi.is_contiguous(memory_format=torch.channels_last) and not yi.is_contiguous()


# 8.  prepare
def test_rotated_prepare_takes_the_cost_up_front_and_shutdown_frees_the_tables(gpu):
    W, H = 66, 58
    rq = gpu.make_request(W, H, 3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 62.5)     # a geometry no other test of this module prepares
    assert gpu.plan_shape(rq) == ""
    gpu.adjoint_rotated_prepare(rq)
    shape = gpu.plan_shape(rq)
    assert "rot_adjoint=sums" in shape and re.search(r" knife=\d+$", shape), shape
    build_ms = re.search(r"build_ms=([0-9.]+)", shape).group(1)
    g = _gradient(gpu, rq)
    got, kernel = _run(gpu, rq, g)
    assert kernel.startswith(PLAIN_KERNEL) and gpu.plan_shape(rq) == shape and build_ms in gpu.plan_shape(rq)      # the call only enqueued
    # the existing prepare entry still builds no plan at a general rotation, and the general entry needs none
    gpu.shutdown()
    assert gpu.plan_shape(rq) == ""
    gpu.adjoint_prepare(rq)
    ref, kref = _run(gpu, rq, g, planned=False)
    assert gpu.plan_shape(rq) == "" and GATHER_KERNEL in kref
    # after aai_shutdown a call rebuilds the plan and its tables
    again, kernel = _run(gpu, rq, g)
    assert kernel.startswith(PLAIN_KERNEL) and "rot_adjoint=sums" in gpu.plan_shape(rq)
    assert np.array_equal(_bits(again), _bits(got)) and np.array_equal(_bits(again), _bits(ref))
