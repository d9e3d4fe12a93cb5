"""GPU (MI355X): every kernel, launch shape and strip path of the axis-aligned family K1 the launcher can choose (the case table of
tests/axis_variants.py; test_axis_variants_host.py checks the table itself on the CPU).

aai_last_kernel() names the kernel that ran, the variant probe (tests/emulation: the launcher's own axis_launch_shape on the plan's
own tables) names the branch, pipeline and store shape inside it; every case is compared with the CPU oracle: 1e-5 relative with the
project's floor of 1e-3 x the value scale, exact zeros exact.  Two bit identities the project promises are held against the new
paths: a 90 / 270 degree tile-kernel image equals the same image computed in row bands (which take the strip kernel's vertical_pass
where the image takes issue_rows / finish_rows), and channel c of an interleaved call equals the single-channel call on plane c.
The tile pipeline for windows of five to eight source rows, branch B and the multi-iteration register loops had no test before this
module: their cases run first between guard margins (tests/guard_layout.py), so that an overrun lands in memory the test owns.
"""
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import axis_variants as av
from conftest import TOL
from guard_layout import GuardedLayout, to_device

pytestmark = pytest.mark.gpu

KERNEL_ORDER = ("aai_axis_kernel", "aai_axis_tile_kernel", "aai_axis_wide_kernel")
ITEMS = [(k, T) for k in KERNEL_ORDER for T in av.TYPES]
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


def _request(gpu, p):
    return gpu.make_request(p.W, p.H, p.ratio, 1.0, av.iso_of(p.W, p.H, p.off), p.angle, mode=p.mode)


def _call(gpu, rq, C, T, batch, sptr, sstride, simage, dptr, dstride, dimage):
    """the typed batch device entry, or the interleaved one for C > 1"""
    import torch
    code = av.TYPES[T][2]
    if C == 1:
        gpu.resample_device(rq, sptr, sstride, dptr, dstride, _stream(), batch=batch, src_image_stride=simage, dst_image_stride=dimage, src_dtype=code)
    else:
        gpu.resample_interleaved_device(rq, C, sptr, sstride, dptr, dstride, _stream(), batch=batch, src_image_stride=simage,
                                        dst_image_stride=dimage, src_dtype=code)
    torch.cuda.synchronize()
    return gpu.last_kernel()


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


def _padded(gpu, rq, srcs, C, T, dW, dH):
    """two images, padded source and destination strides, a sentinel in the destination's padding; returns (outputs, kernel)"""
    import torch
    t, stride, image = _to_device(srcs, pad=5)
    dpad = 3
    out = torch.full((len(srcs), dH, dW * C + dpad), SENTINEL, dtype=torch.float32, device="cuda")
    kernel = _call(gpu, rq, C, T, len(srcs), t.data_ptr(), stride, image, out.data_ptr(), dW * C + dpad, dH * (dW * C + dpad))
    host = out.cpu().numpy()
    assert (host[:, :, dW * C:] == SENTINEL).all(), "the padding of the dst rows was written"
    return [host[b, :, :dW * C].reshape((dH, dW) if C == 1 else (dH, dW, C)) for b in range(len(srcs))], kernel


def _guarded(gpu, rq, srcs, C, T, dW, dH):
    """the same call with both buffers between guard margins: poison around the source, a sentinel pattern around the destination"""
    B = len(srcs)
    p_h, p_w = srcs[0].shape[0], srcs[0].shape[1]
    sl = GuardedLayout((B, p_h, p_w, C), T, p_w * C + 5, p_h * (p_w * C + 5) + 7, 1)
    dl = GuardedLayout((B, dH, dW, C), "f32", dW * C + 3, dH * (dW * C + 3) + 6, 2)
    values = np.stack([np.asarray(s).reshape(p_h, p_w, C) for s in srcs])
    sdev, ddev = to_device(sl.make_src(values, "nan" if T == "f32" else "ones")), to_device(dl.make_dst())
    kernel = _call(gpu, rq, C, T, B, sl.ptr(sdev), sl.stride, sl.image_stride, dl.ptr(ddev), dl.stride, dl.image_stride)
    out, first, count = dl.check_dst(ddev)
    assert count == 0, ("%d guard elements of the destination were written, first: %s" % (count, dl.describe(first)), kernel)
    assert dl.sentinels_left(out) == 0 and np.isfinite(out).all(), ("pixels never written, or poison read", kernel)
    return [out[b].reshape((dH, dW) if C == 1 else (dH, dW, C)) for b in range(B)], kernel


def _needs_guard(cands):
    """candidates no test ran before this module: the tile pipeline for windows of five to eight source rows"""
    return any(c.kernel == "aai_axis_tile_kernel" and c.sub == "NR8" for c in cands)


@pytest.mark.parametrize("kernel,T", ITEMS, ids=["%s-%s" % it for it in ITEMS])
def test_every_launch_shape_and_strip_path_against_oracle(gpu, hostemu, po, kernel, T):
    """All small cases of one (kernel, source type), each distinct geometry once: the typed batch device entry (C > 1: the interleaved
    one) with two images, the second the first flipped, padded strides and a sentinel in the dst padding.  Per geometry:
    aai_last_kernel() is the probe's kernel, the oracle's bar, exact zeros, a plan that is not dense and leaves at most 5 % of the
    pixels to the fix-up pass; 90 / 270 degree tile-kernel images (fp32: the band entry takes fp32 sources) equal their row bands bit
    for bit; channels equal planes bit for bit.  Then coverage: every candidate of (kernel, T) that has a small case was hosted by a
    launch whose aai_last_kernel() matched."""
    import torch
    cands, big, tall, cases, probe = av.table(hostemu)
    hi = av.TYPES[T][3]
    mine = [case for case in cases if case.cand.kernel == kernel and case.cand.T == T]
    assert mine
    points = {}
    for case in mine:
        points.setdefault(case.point, case)
    gpu.shutdown()                                                   # (no plans of earlier items: plan_shape below finds this case's)
    covered = set()
    worst, t0 = 0.0, time.time()
    try:
        for p, case in points.items():
            C = p.C
            v = av.probe_point(probe, p)
            hosts = av.hosted(v, T, C, p.W)
            rq = _request(gpu, p)
            rc, msg, lay = gpu.query(rq)
            assert rc == 0 and (lay.dst_width, lay.dst_height) == (case.dW, case.dH), (av.case_id(case), msg)
            dW, dH = case.dW, case.dH
            srcs = [av.case_source(case), av.case_source(case, flip=True)]
            guarded = _guarded(gpu, rq, srcs, C, T, dW, dH) if _needs_guard(hosts) else None
            outs, ran = _padded(gpu, rq, srcs, C, T, dW, dH)
            assert ran.split("+")[0] == av.KERNELS[v.kernel] == kernel, (av.case_id(case), ran, v)
            if guarded:
                assert guarded[1] == ran and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(guarded[0], outs)), (av.case_id(case), guarded[1], ran)
            for src, dst in zip(srcs, outs):
                gold = av.case_gold(po, case, src)
                assert dst.dtype == np.float32 and dst.shape == gold.shape, (av.case_id(case), dst.shape, gold.shape)
                err = float((np.abs(dst - gold) / np.maximum(np.abs(gold), 1e-3 * hi)).max())
                worst = max(worst, err)
                print("%-110s %-24s rel err %.2e" % (av.case_id(case), ran, err))
                assert err <= TOL, (av.case_id(case), ran, err)
                assert np.array_equal(gold == 0, dst == 0), (av.case_id(case), ran)
            m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq, channels=C))
            assert m, (av.case_id(case), gpu.plan_shape(rq, channels=C))
            assert int(m.group(2)) == 0 and int(m.group(1)) <= 0.05 * dW * dH, (av.case_id(case), m.group(0), dW * dH)
            if kernel == "aai_axis_tile_kernel" and T == "f32":
                # the image in dst row bands of at most 64 rows: at most 64 outputs per strip, the strip kernel's branch A
                t, stride, _ = _to_device(srcs[:1], pad=5)
                for (r0, r1) in av.bands_of(dH):
                    vb = av.probe_point(probe, p._replace(batch=1), (r0, r1))
                    assert av.KERNELS[vb.kernel] == "aai_axis_kernel" and vb.branches == 1, (av.case_id(case), r0, r1, vb)
                    a, b = gpu.band_source_rows(rq, r0, r1)
                    band = torch.full((r1 - r0, dW + 3), SENTINEL, dtype=torch.float32, device="cuda")
                    gpu.resample_band_device(rq, r0, r1, t.data_ptr() + 4 * a * stride, stride, band.data_ptr(), dW + 3, _stream())
                    torch.cuda.synchronize()
                    assert gpu.last_kernel().split("+")[0] == "aai_axis_kernel", (av.case_id(case), gpu.last_kernel())
                    got = band.cpu().numpy()
                    assert (got[:, dW:] == SENTINEL).all()
                    diff = got[:, :dW].view(np.int32) != outs[0][r0:r1].view(np.int32)
                    assert not diff.any(), ("%d pixels of band [%d, %d) differ in bits from the whole image, first at %s"
                                            % (int(diff.sum()), r0, r1, np.argwhere(diff)[0].tolist()), av.case_id(case))
            if C > 1 and kernel != "aai_axis_wide_kernel":
                for c in range(C):
                    plane, pk = _padded(gpu, rq, [np.ascontiguousarray(srcs[0][:, :, c])], 1, T, dW, dH)
                    if "aai_axis_wide_kernel" in pk:
                        continue
                    diff = plane[0].view(np.int32) != np.ascontiguousarray(outs[0][:, :, c]).view(np.int32)
                    assert not diff.any(), ("channel %d: %d pixels differ in bits from the single-channel call (%s), first at %s"
                                            % (c, int(diff.sum()), pk, np.argwhere(diff)[0].tolist()), av.case_id(case))
            covered |= hosts
    finally:
        gpu.shutdown()
    want = sorted(c for c in cands if c.kernel == kernel and c.T == T and cands[c])
    for cand in want:
        assert cand in covered, cand
        print("covered: %s" % av.cand_id(cand))
    print("%s %s: %d geometries, %d candidates covered, worst rel err %.2e, %.1f s" % (kernel, T, len(points), len(want), worst, time.time() - t0))


def _device_source(gpu, W, H, T, seed, margin):
    """a synthetic [H, W] image of type T on the device, inside an allocation with `margin` poisoned elements on either side
    (NaN for fp32, all-ones for the integer types); returns (allocation, view, host copy as float32)"""
    import torch
    f = torch.empty((H, W), dtype=torch.float32, device="cuda")
    gpu.synth_device(f.data_ptr(), W, H, W, seed)
    torch.cuda.synchronize()
    if T == "f32":
        whole = torch.full((2 * margin + H * W,), float("nan"), dtype=torch.float32, device="cuda")
        view = whole[margin:margin + H * W].view(H, W)
        view.copy_(f + 0.25)
        host = view.cpu().numpy()
    else:
        hi = av.TYPES[T][3]
        q = (f * (hi - 2) + 1).to(torch.int32)                       # 1 .. hi - 1
        tdt = torch.uint8 if T == "u8" else torch.int16
        whole = torch.full((2 * margin + H * W,), -1, dtype=torch.int32, device="cuda").to(tdt)
        view = whole[margin:margin + H * W].view(H, W)
        view.copy_(q.to(tdt))
        host = q.cpu().numpy().astype(np.float32)
        del q
    del f
    return whole, view, host


def _device_dst(n, margin):
    import torch
    whole = torch.full((2 * margin + n,), SENTINEL, dtype=torch.float32, device="cuda")
    return whole, whole[margin:margin + n]


def _margins_intact(whole, margin):
    return bool((whole[:margin] == SENTINEL).all().item() and (whole[-margin:] == SENTINEL).all().item())


def test_large_cases_reach_branch_b_the_register_loops_and_the_typed_escalation(gpu, hostemu, po):
    """axis_variants.BIG: what no small request reaches.  a: u8 100 x 1,048,601 at 270 and 100 x 1,048,602 at 90 degrees -- branch B,
    forward and reverse 16-byte stores, eight iterations of its loop, and a last chunk of one / two output rows for its scalar tail;
    e: u8 200 x 1,048,601 at 270 -- branch B with four outputs per lane; b: fp32 40 x 1,100,000 at 90 and 270 -- branch A, four
    iterations; c / d: 16 images u8 / u16 1024 x 4096 at 4:1 -- 8 / 4 output rows per workgroup.  The source is made on the device;
    the destination, and for a, e and b the source, lie between margins of sentinel / poison (an overrun of a few rows lands in the
    margin); dst row bands against the oracle's rows, ALL columns (the scalar tail is the last one or two): rows 0..1, 63..64 and
    98..99 of the 100-row outputs (lanes 63 | 64 and the tail), 0..1, 127..128, 191..192 and 198..199 of e, 0..1, 19..20 and 38..39 of b,
    four bands of four rows per image of c / d.  A row of a million columns takes the oracle three to seven seconds, so the bands of
    a, e and b have two rows each, and the bands of a case run in threads.  Every output is freed before the next."""
    import torch
    cands, big, tall, cases, probe = av.table(hostemu)
    covered = set()
    gpu.shutdown()
    try:
        for name, p in av.BIG.items():
            t0 = time.time()
            v = av.probe_point(probe, p)
            rq = _request(gpu, p)
            rc, msg, lay = gpu.query(rq)
            assert rc == 0, msg
            dW, dH = lay.dst_width, lay.dst_height
            assert (dW, dH) == (v.dW, v.dH)
            hi = av.TYPES[p.T][3]
            omode = po.MODE_EXACT if p.mode == av.MODE_AREA else po.MODE_FAST
            margin = 64 * max(p.W, dW) + 4096
            images, hosts = [], []
            if p.batch == 1:
                swhole, sview, host = _device_source(gpu, p.W, p.H, p.T, 3, margin)
                hosts.append(host)
                sptr, simage = sview.data_ptr(), p.W * p.H
            else:
                # (one allocation for the batch: the images follow each other, the margins lie around all of them)
                parts = [_device_source(gpu, p.W, p.H, p.T, 1 + b, 0) for b in range(p.batch)]
                swhole = torch.cat([q[1].reshape(-1) for q in parts])
                hosts = [q[2] for q in parts]
                del parts
                sptr, simage = swhole.data_ptr(), p.W * p.H
            dwhole, dview = _device_dst(p.batch * dW * dH, margin)
            ran = _call(gpu, rq, 1, p.T, p.batch, sptr, p.W, simage, dview.data_ptr(), dW, dW * dH)
            assert ran.split("+")[0] == av.KERNELS[v.kernel], (name, ran, v)
            assert _margins_intact(dwhole, margin), (name, "the margins around the destination were written")
            m = re.search(r"rows=(\d+) nt=(\d+).*flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq))
            assert m and int(m.group(1)) == 0 and int(m.group(4)) == 0 and int(m.group(3)) <= 0.05 * dW * dH, (name, gpu.plan_shape(rq))     # rows=0: no measured shape
            out = dview.view(p.batch, dH, dW)
            if dH == 100:
                bands = [(0, 2), (63, 65), (98, 100)]
            elif dH == 200:
                bands = [(0, 2), (127, 129), (191, 193), (198, 200)]         # outputs k0 + lane + 64 q: q = 1 | 2, 2 | 3 and the tail
            elif dH == 40:
                bands = [(0, 2), (19, 21), (38, 40)]
            else:
                bands = [(0, 4), (dH // 3, dH // 3 + 4), (2 * dH // 3 + 1, 2 * dH // 3 + 5), (dH - 4, dH)]
            worst, t1 = 0.0, time.time()
            jobs = [(b, r0, r1) for b in range(p.batch) for (r0, r1) in bands]
            with ThreadPoolExecutor(4) as pool:                          # (the oracle keeps no state between calls; ctypes releases the GIL)
                golds = list(pool.map(lambda j: po.oracle_rows(omode, hosts[j[0]], p.ratio, 1.0, av.iso_of(p.W, p.H, p.off), p.angle, j[1], j[2], dW), jobs))
            t_oracle = time.time() - t1
            for (b, r0, r1), gold in zip(jobs, golds):
                got = out[b, r0:r1].cpu().numpy()
                err = float((np.abs(got - gold) / np.maximum(np.abs(gold), 1e-3 * hi)).max())
                worst = max(worst, err)
                assert err <= TOL, (name, ran, b, r0, err)
                assert np.array_equal(gold == 0, got == 0), (name, ran, b, r0)
            covered |= av.hosted(v, p.T, p.C, p.W)
            print("large case %-5s %-16s rows %2d  %d x %d x %d -> %d x %d: worst rel err %.2e, oracle %.1f s, %.1f s in all"
                  % (name, ran, v.rows, p.batch, p.W, p.H, dW, dH, worst, t_oracle, time.time() - t0))
            del out, dview, dwhole, swhole, hosts
            torch.cuda.empty_cache()
    finally:
        gpu.shutdown()
    for cand in sorted(big):
        assert cand in covered, cand
        print("covered: %s" % av.cand_id(cand))
    # branch B in both store directions, A and B with more than one iteration of their loops -- through these cases and no others
    only = {c for c in big if not cands.get(c)}
    assert {(c.sub, c.dir_b, c.rows_class, c.shape) for c in only} == {
        ("A", 1, "n", "8"), ("A", -1, "n", "8"), ("B", 1, "n", "4"), ("B", -1, "n", "4"), ("B", 1, "n", "1"), ("B", -1, "n", "1"),
        ("B", 0, "nq2", ""), ("B", 0, "nq4", "")}, only
