"""GPU (MI355X): every template instantiation the rotated-lattice launchers can choose, run at the footprints that just fit and
just enter its window (the case table of tests/rot_variants.py; test_rot_variants_host.py checks the table itself on the CPU).

aai_last_kernel() names the family that ran, the variant probe (tests/emulation, the launchers' own header functions) names the
instantiation inside it; every case is compared with the CPU oracle: 1e-5 relative with the project's floor of 1e-3 x the value
scale, exact zeros exact.  The typed instantiations of the two comparison samplers are at the end.  Nothing here reads /root/reference.
"""
import re

import numpy as np
import pytest

import rot_variants as rv
from conftest import TOL

pytestmark = pytest.mark.gpu

FAMILY_ORDER = ("aai_quad_kernel", "aai_quad_fast_kernel", "aai_quad_multi_kernel", "aai_cell_kernel", "aai_cell_multi_kernel",
                "aai_wide_kernel", "aai_wide_fast_kernel")
ITEMS = [(f, T) for f in FAMILY_ORDER for T in rv.TYPES]

NOT_DISPATCHED = rv.NOT_DISPATCHED


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


def _family_of(kernel_name):
    name = kernel_name.split("<")[0].split("+")[0]
    return "fp64" if name in ("aai_rotated_kernel", "aai_rotated_runs_kernel") else name


def _to_device(arrays, pad):
    """[B] host images of one shape -> one device tensor with `pad` elements of row padding; returns (tensor, row stride, image stride)"""
    import torch
    a0 = arrays[0]
    H, row = a0.shape[0], int(np.prod(a0.shape[1:]))
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16}[a0.dtype]
    t = torch.zeros((len(arrays), H, row + pad), dtype=tdt, device="cuda")
    for b, a in enumerate(arrays):
        flat = np.ascontiguousarray(a).reshape(H, row)
        t[b, :, :row] = torch.from_numpy(flat.view(np.int16) if a.dtype == np.uint16 else flat).cuda()
    return t, row + pad, H * (row + pad)


def _launch(gpu, rq, srcs, C, T, device):
    """host entry (one image) or batch device entry (padded strides); returns the [B] outputs, [dH, dW] or [dH, dW, C]"""
    import torch
    from area_average_interpolation_amd import _lib as L
    code = rv.TYPES[T][2]
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    dW, dH = lay.dst_width, lay.dst_height
    if not device:
        assert len(srcs) == 1
        src = srcs[0]
        args = (src, rq.src_res_x, rq.dst_res_x, (rq.src_iso_x, rq.src_iso_y), rq.rotation_deg)
        if C == 1:
            rc, msg, dst, _, _ = gpu.resample_host(*args, mode=rq.mode, policy=rq.policy)
        else:
            rc, msg, dst, _ = gpu.resample_interleaved_host(*args, mode=rq.mode, policy=rq.policy)
        assert rc == 0, msg
        return [dst]
    SENTINEL = -7.0
    t, stride, image = _to_device(srcs, pad=5)
    dpad = 3
    out = torch.full((len(srcs), dH, dW * C + dpad), SENTINEL, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if C == 1:
        gpu.resample_device(rq, t.data_ptr(), stride, out.data_ptr(), dW + dpad, st, batch=len(srcs), src_image_stride=image,
                            dst_image_stride=dH * (dW + dpad), src_dtype=code)
    else:
        gpu.resample_interleaved_device(rq, C, t.data_ptr(), stride, out.data_ptr(), dW * C + dpad, st, batch=len(srcs), src_image_stride=image,
                                        dst_image_stride=dH * (dW * C + dpad), src_dtype=code)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, :, dW * C:] == SENTINEL).all()                 # the padding of the dst rows is nobody's to write
    return [host[b, :, :dW * C].reshape((dH, dW) if C == 1 else (dH, dW, C)) for b in range(len(srcs))]


@pytest.mark.parametrize("family,T", ITEMS, ids=["%s-%s" % it for it in ITEMS])
def test_every_dispatched_instantiation_against_oracle(gpu, hostemu, po, family, T):
    """All cases of one (family, source type): area cases of the cell families carry AAI_POLICY_PREFER_CELL (the table's policy),
    C > 1 goes through the interleaved entries, every other item through the batch device entry with padded strides and two images.
    Per case: the oracle's bar, exact zeros, a plan that is not dense and leaves at most 5 % of the pixels to the double-precision
    pass.  Then coverage: a case whose aai_last_kernel() family is its candidate's covers the candidate (the probe, which the host
    module holds to the table, names the instantiation); every C = 1 candidate must be covered, a C > 1 candidate is covered or
    listed in NOT_DISPATCHED with the rule that keeps it away and the family that ran instead."""
    cands, cases, probe = rv.table(hostemu)
    device = ITEMS.index((family, T)) % 2 == 1
    hi = rv.TYPES[T][3]
    mine = [case for case in cases if case.cand.family == family and case.cand.T == T]
    assert mine
    gpu.shutdown()                                                   # (no plans of earlier items: plan_shape below finds this case's)
    covered, ran = set(), {}
    worst = 0.0
    try:
        for case in mine:
            C = case.cand.C
            rq = gpu.make_request(case.W, case.H, case.ratio, 1.0, case.iso, case.angle, mode=case.mode, policy=case.policy)
            srcs = [rv.case_source(case)] + ([rv.case_source(case, flip=True)] if device else [])
            outs = _launch(gpu, rq, srcs, C, T, device)
            kernel = gpu.last_kernel()
            for src, dst in zip(srcs, outs):
                gold = rv.case_gold(po, case, src)
                assert dst.dtype == np.float32 and dst.shape == gold.shape, (rv.case_id(case), dst.shape, gold.shape)
                err = float((np.abs(dst - gold) / np.maximum(np.abs(gold), 1e-3 * hi)).max())
                worst = max(worst, err)
                print("%-70s %-40s rel err %.2e" % (rv.case_id(case), kernel, err))
                assert err <= TOL, (rv.case_id(case), kernel, err)
                assert np.array_equal(gold == 0, dst == 0), (rv.case_id(case), kernel)
            m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq, channels=C))
            assert m, (rv.case_id(case), gpu.plan_shape(rq, channels=C))
            assert int(m.group(2)) == 0 and int(m.group(1)) <= 0.05 * case.dW * case.dH, (rv.case_id(case), m.group(0), case.dW * case.dH)
            ran.setdefault(case.cand, set()).add(_family_of(kernel))
            if _family_of(kernel) == family:
                covered.add(case.cand)
    finally:
        gpu.shutdown()
    for cand in sorted(c for c in cands if c.family == family and c.T == T):
        entry = NOT_DISPATCHED.get((cand.family, cand.T, cand.C, cand.win))
        if cand.C == 1:
            assert entry is None and cand in covered, (cand, ran[cand])          # nothing below 4 GiB keeps a family away from a plain image
        elif entry is None:
            assert cand in covered and cands[cand][2], (cand, ran[cand])
        else:
            assert cand not in covered, ("stale NOT_DISPATCHED entry: the family ran", cand, entry)
            assert ran[cand] == {entry[1]} and not cands[cand][2], (cand, ran[cand], entry)
    # (and no entry of the table names a candidate the grid does not hold)
    for key in NOT_DISPATCHED:
        if key[0] == family and key[1] == T:
            assert any((c.family, c.T, c.C, c.win) == key for c in cands), ("NOT_DISPATCHED entry without a candidate", key)
    print("%s %s: %d cases, %d candidates covered, worst rel err %.2e" % (family, T, len(mine), len(covered), worst))


# ---- the comparison samplers on 8- / 16-bit sources (aai_sample_kernel<mode, u8 / u16>) --------------------------------------------
SAMPLER_GEOMETRIES = [(41, 33, 1.0, 1.0, 0.0), (37, 29, 1.0, 2.0, 300.0), (67, 53, 3.0, 1.0, 17.5), (23, 19, 1.0, 4.0, 45.0)]      # W, H, src res, dst res, angle


@pytest.mark.parametrize("T", ["u8", "u16"])
@pytest.mark.parametrize("mode", [3, 4], ids=["bilinear", "bicubic"])
def test_typed_samplers_against_cpu_restatement(gpu, po, mode, T):
    """Bilinear and bicubic on typed sources, planar and RGB, through the host entries and the batch device entries (padded strides,
    two images), against the oracle's restatement at 2e-5 x the value scale -- the bound of
    test_comparison_samplers_against_cpu_restatement (fp32 taps against fp64; cubic weights reach 1.125)."""
    npdt, _, _, hi = rv.TYPES[T]
    rng = np.random.default_rng(31 + mode)
    for (W, H, sr, dr, ang) in SAMPLER_GEOMETRIES:
        iso = ((W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.375)
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
        for C in (1, 3):
            shape = (H, W) if C == 1 else (H, W, C)
            srcs = [rng.integers(0, int(hi), size=shape).astype(npdt) for _ in range(2)]
            golds = []
            for src in srcs:
                planes = [src] if C == 1 else [src[:, :, c] for c in range(C)]
                g = [po.oracle_run(mode, np.ascontiguousarray(p, dtype=np.float64), sr, dr, iso, ang).dst for p in planes]
                golds.append(g[0] if C == 1 else np.stack(g, axis=2))
            outs = _launch(gpu, rq, srcs[:1], C, T, device=False) + _launch(gpu, rq, srcs, C, T, device=True)
            assert ("bilinear" if mode == 3 else "bicubic") in gpu.last_kernel(), gpu.last_kernel()
            for dst, gold in zip(outs, [golds[0]] + golds):
                assert dst.shape == gold.shape, (W, H, sr, dr, ang, C, dst.shape, gold.shape)
                err = float(np.abs(dst - gold).max()) / hi
                print("sampler mode %d %s C%d %gx%g %g:%g at %g: %.2e of the value scale" % (mode, T, C, W, H, sr, dr, ang, err))
                assert err <= 2e-5, (mode, T, C, W, H, sr, dr, ang, err)
