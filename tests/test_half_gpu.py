"""The half-precision path on the MI355X (include/aai_half.h): the direct kernel against its CPU replay bit for bit, against the oracle
and against the forwarding arithmetic; the memory contract with guarded, 2-byte-aligned, padded buffers; non-finite data; the
forwarding route's bits; stream order of both routes.

Why "at most 1 % of elements differ" between the two routes: their fp32 sums agree to about 1e-6 relative, so they straddle a
rounding boundary of relative width 2^-11 with probability of about 2e-3 per element; 1 % is five times that.  A difference is then
one unit in the last place, never more.  The forwarding route against narrow(fp32 entry(widen)) is at 0 %: equal bits."""
import numpy as np
import pytest

import half_cases as hc
import stream_order as so
from guard_layout import GuardedLayout, to_device, to_numpy
from test_half_host import TAIL_CASES, replay_case

pytestmark = pytest.mark.gpu

SENTINEL16 = 0x7fa5           # a NaN in both element types that no arithmetic here produces
NAN16 = {hc.F16: 0x7e00, hc.BF16: 0x7fc0}
INF16 = {hc.F16: 0x7c00, hc.BF16: 0x7f80}


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return aai


def tdtype(ht):
    import torch
    return torch.float16 if ht == hc.F16 else torch.bfloat16


def upload(bits, ht):
    """raw 16-bit elements -> a device tensor of the element type"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()).cuda().view(tdtype(ht))


def download(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def run_half(gpu, rq, ht, src_bits):
    """one image through resample_half_device -> raw output bits"""
    import torch
    lay = gpu.query(rq)[2]
    x = upload(src_bits, ht)
    y = torch.full((lay.dst_height, lay.dst_width), float("nan"), dtype=tdtype(ht), device="cuda")
    gpu.resample_half_device(rq, x.data_ptr(), rq.src_width, y.data_ptr(), lay.dst_width, ht, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return download(y)


def run_forwarded_with_torch(gpu, rq, ht, src_bits):
    """narrow(resample_device(widen(src))), widening and narrowing done by torch -> raw output bits"""
    import torch
    lay = gpu.query(rq)[2]
    x32 = upload(src_bits, ht).float().contiguous()
    y32 = torch.full((lay.dst_height, lay.dst_width), float("nan"), dtype=torch.float32, device="cuda")
    gpu.resample_device(rq, x32.data_ptr(), rq.src_width, y32.data_ptr(), lay.dst_width, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return download(y32.to(tdtype(ht)))


# ---- the direct route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht, tname", hc.TYPES, ids=[t[1] for t in hc.TYPES])
@pytest.mark.parametrize("mode_name", hc.MODES)
@pytest.mark.parametrize("case", sorted(hc.CASES))
def test_direct_kernel_has_the_replays_bits(gpu, po, case, mode_name, ht, tname):
    rq, src, want, pre, gold = replay_case(gpu, po, case, mode_name, ht)
    got = run_half(gpu, rq, ht, src)
    assert gpu.last_kernel() == "aai_axis_half_kernel<%s>" % tname, gpu.last_kernel()
    assert "flagged=0 dense=0" in gpu.plan_shape(rq), gpu.plan_shape(rq)
    assert got.shape == want.shape
    differ = got != want
    assert not differ.any(), (case, mode_name, tname, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    excess = hc.rounded_excess(hc.widen(got, ht), gold, ht)
    # against the forwarding arithmetic: at most one unit in the last place, in at most 1 % of the elements
    fwd = run_forwarded_with_torch(gpu, rq, ht, src)
    ulps = hc.ulp_distance(got, fwd)
    share = float((ulps != 0).mean())
    print("direct %s %s %s: %.3e over the rounded-value bound; %d of %d elements (%.3f %%) differ from the forwarding arithmetic, by at most %d ulp"
          % (case, mode_name, tname, excess, int((ulps != 0).sum()), ulps.size, 100 * share, int(ulps.max())))
    assert excess <= 0, (case, mode_name, tname, excess)
    assert int(ulps.max()) <= 1, (case, mode_name, tname, int(ulps.max()))
    assert share <= 0.01, (case, mode_name, tname, share)


@pytest.mark.parametrize("ht, tname", hc.TYPES, ids=[t[1] for t in hc.TYPES])
@pytest.mark.parametrize("case", ["b", "c", "e"] + TAIL_CASES)
def test_direct_kernel_memory_contract(gpu, po, case, ht, tname):
    """batch 3, odd padded row strides on both sides, gaps between the images, a base address one element past a 256-byte boundary
    (2-byte aligned and nothing more).  Source padding holds NaN: a read of it would reach the output.  dst padding holds a sentinel.
    The tail cases (test_half_host.TAIL_CASES) end the one strip's store in a quad of lanes with 1, 2 or 3 live outputs."""
    import torch
    B = 3
    W, H = (hc.CASES[case] if isinstance(case, str) else case)[:2]
    for mode_name in hc.MODES:
        rq = hc.request(gpu, case, mode_name)
        if not isinstance(case, str):
            axis, wide, transposed, strips, most, shared, rowspan, direct = hc.facts(rq)
            assert direct == 1 and strips == 1 and most == W // 4 <= 64, (case, mode_name, strips, most)
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        sstride = W + 3 + (W % 2)                        # odd
        dstride = dW + 5 + (dW % 2)                      # odd
        assert sstride % 2 == 1 and dstride % 2 == 1
        sl = GuardedLayout((B, H, W, 1), "u16", stride=sstride, image_stride=H * sstride + 11, base_offset=1)
        dl = GuardedLayout((B, dH, dW, 1), "u16", stride=dstride, image_stride=dH * dstride + 7, base_offset=1)
        images = [hc.source_bits(W, H, ht, seed=20 + b) for b in range(B)]
        sbuf = sl.make_src(np.stack(images)[..., None], "zeros")
        sbuf[~sl.entitled] = NAN16[ht]
        dbuf = np.full(dl.total, SENTINEL16, np.uint16)
        ds, dd = to_device(sbuf), to_device(dbuf)
        assert sl.ptr(ds) % 4 == 2 and dl.ptr(dd) % 4 == 2
        gpu.resample_half_device(rq, sl.ptr(ds), sstride, dl.ptr(dd), dstride, ht, stream=torch.cuda.current_stream().cuda_stream, batch=B,
                                 src_image_stride=sl.image_stride, dst_image_stride=dl.image_stride)
        torch.cuda.synchronize()
        assert gpu.last_kernel().startswith("aai_axis_half_kernel")
        after = to_numpy(dd, np.uint16)
        changed = np.flatnonzero((after != SENTINEL16) & ~dl.entitled)
        assert changed.size == 0, (case, mode_name, tname, [dl.describe(int(o) - dl.lead) for o in changed[:4]])
        assert np.array_equal(to_numpy(ds, np.uint16), sbuf)
        out = after[dl.index].reshape(B, dH, dW)
        assert not (out == SENTINEL16).any(), (case, mode_name, tname, "entitled elements not written")
        for b in range(B):
            single = run_half(gpu, rq, ht, images[b])
            assert np.array_equal(out[b], single), (case, mode_name, tname, b)
            assert np.array_equal(single, hc.replay(gpu, rq, ht, images[b])[0]), (case, mode_name, tname, b)


@pytest.mark.parametrize("ht, tname", hc.TYPES, ids=[t[1] for t in hc.TYPES])
def test_direct_kernel_non_finite_pixels_reach_their_footprint_only(gpu, po, ht, tname):
    W, H, sr, dr, iso, ang = hc.CASES["a"]
    spots = ((10, 9, INF16[ht]), (40, 30, NAN16[ht]))
    for mode_name in hc.MODES:
        rq, src, clean, pre, gold = replay_case(gpu, po, "a", mode_name, ht)
        dirty = src.copy()
        impulse = np.zeros((H, W))
        for x, y, bits in spots:
            dirty[y, x] = bits
            impulse[y, x] = 1.0
        touched = po.oracle_run(hc.oracle_mode(po, mode_name), impulse, sr, dr, iso, ang).dst != 0
        assert 1 <= int(touched.sum()) <= 8
        got = run_half(gpu, rq, ht, dirty)
        assert gpu.last_kernel().startswith("aai_axis_half_kernel")
        assert np.array_equal(~np.isfinite(hc.widen(got, ht)), touched), (mode_name, tname)
        assert np.array_equal(got[~touched], clean[~touched]), (mode_name, tname)


def test_direct_kernel_zeroes_dst_pixels_off_the_image(gpu, po):
    """an isocenter far off the centre leaves dst rows and columns without a source pixel: +0 there, whatever the source holds (NaN
    everywhere here), as the fp32 entry writes it"""
    rq = gpu.make_request(64, 48, 4, 1, (-7.0, 60.0), 0.0)
    assert hc.facts(rq)[7] == 1
    for ht, tname in hc.TYPES:
        src = np.full((48, 64), NAN16[ht], np.uint16)
        got = run_half(gpu, rq, ht, src)
        assert gpu.last_kernel().startswith("aai_axis_half_kernel")
        want = hc.replay(gpu, rq, ht, src)[0]
        assert np.array_equal(got, want)
        assert (got == 0).any() and np.isnan(hc.widen(got[got != 0], ht)).all()
        fwd = run_forwarded_with_torch(gpu, rq, ht, src)
        assert np.array_equal(got == 0, fwd == 0)


# ---- the forwarding route ----------------------------------------------------------------------------------------------------
ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)
FORWARDED = [("rotated area", ROT, "area"), ("rotated fast", ROT, "fast"), ("case b at 90 degrees", hc.CASES["b"][:5] + (90.0,), "area"),
             ("bilinear", (96, 80, 2, 1, (47.5, 39.5), 30.0), "bilinear")]


def _request(gpu, geom, mode_name):
    W, H, sr, dr, iso, ang = geom
    mode = {"area": gpu.MODE_AREA, "fast": gpu.MODE_FAST, "bilinear": gpu.MODE_BILINEAR}[mode_name]
    return gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)


@pytest.mark.parametrize("ht, tname", hc.TYPES, ids=[t[1] for t in hc.TYPES])
@pytest.mark.parametrize("name, geom, mode_name", FORWARDED, ids=[f[0] for f in FORWARDED])
def test_forwarding_route_has_the_fp32_entrys_bits(gpu, name, geom, mode_name, ht, tname):
    rq = _request(gpu, geom, mode_name)
    src = hc.source_bits(geom[0], geom[1], ht, seed=31)
    got = run_half(gpu, rq, ht, src)
    kernel = gpu.last_kernel()
    assert kernel.endswith("+widened") and not kernel.startswith("aai_axis_half_kernel"), kernel
    want = run_forwarded_with_torch(gpu, rq, ht, src)
    assert gpu.last_kernel() + "+widened" == kernel
    assert np.array_equal(got, want), (name, tname, int((got != want).sum()))
    assert np.isfinite(hc.widen(got, ht)).all()


@pytest.mark.parametrize("ht, tname", hc.TYPES, ids=[t[1] for t in hc.TYPES])
def test_forwarding_route_on_a_plan_with_listed_pixels(gpu, po, axis_knife_golden, ht, tname):
    """the first reference-generated axis-aligned knife geometry whose plan lists pixels (area mode): the half entry forwards, has the fp32
    entry's bits and stays within the rounded-value bound of the array the UNMODIFIED reference recorded (the source is the recorded
    call's source rounded to the element type)"""
    import re
    z, manifest = axis_knife_golden
    for i, c in enumerate(manifest):
        rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=gpu.MODE_AREA)
        gpu.prepare(rq)
        m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq))
        if int(m.group(1)) > 0 and int(m.group(2)) == 0:
            break
    else:
        pytest.fail("no axis-aligned knife geometry lists pixels")
    assert i == 0, i
    src = hc.narrow(np.asarray(po.synth_image(c["W"], c["H"], c["seed"]), np.float32), ht)
    got = run_half(gpu, rq, ht, src)
    kernel = gpu.last_kernel()
    assert kernel.endswith("+widened"), kernel
    assert np.array_equal(got, run_forwarded_with_torch(gpu, rq, ht, src))
    gold = z["a%03d_exact" % i]
    excess = hc.rounded_excess(hc.widen(got, ht), gold, ht)
    print("knife geometry %d %s: %.3e over the rounded-value bound of the recorded array" % (i, tname, excess))
    assert excess <= 0, (tname, excess)


def test_forwarding_route_batch_with_padded_strides(gpu):
    import torch
    B, ht = 2, hc.BF16
    W, H = ROT[:2]
    rq = _request(gpu, ROT, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    sl = GuardedLayout((B, H, W, 1), "u16", stride=W + 3, image_stride=H * (W + 3) + 11, base_offset=1)
    dl = GuardedLayout((B, dH, dW, 1), "u16", stride=dW + 5 + (dW % 2), image_stride=dH * (dW + 5 + (dW % 2)) + 7, base_offset=1)
    images = [hc.source_bits(W, H, ht, seed=40 + b) for b in range(B)]
    sbuf = sl.make_src(np.stack(images)[..., None], "zeros")
    sbuf[~sl.entitled] = NAN16[ht]
    ds, dd = to_device(sbuf), to_device(np.full(dl.total, SENTINEL16, np.uint16))
    gpu.resample_half_device(rq, sl.ptr(ds), sl.stride, dl.ptr(dd), dl.stride, ht, stream=torch.cuda.current_stream().cuda_stream, batch=B,
                             src_image_stride=sl.image_stride, dst_image_stride=dl.image_stride)
    torch.cuda.synchronize()
    assert gpu.last_kernel().endswith("+widened")
    after = to_numpy(dd, np.uint16)
    assert not ((after != SENTINEL16) & ~dl.entitled).any()
    out = after[dl.index].reshape(B, dH, dW)
    for b in range(B):
        assert np.array_equal(out[b], run_forwarded_with_torch(gpu, rq, ht, images[b])), b


# ---- stream order ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(gpu):
    """one scenario per route: the call between a delayed producer and a consumer on the caller's stream, no host wait (stream_order.py)"""
    import torch
    h = so.Harness(gpu)
    for name, geom, mode_name, ht, route in (("direct", hc.CASES["a"], "area", hc.F16, "aai_axis_half_kernel"), ("forwarding", ROT, "area", hc.BF16, "+widened")):
        W, H = geom[:2]
        rq = _request(gpu, geom, mode_name)
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        assert (W * H) % 2 == 0
        inp = torch.empty((H, W), dtype=tdtype(ht), device="cuda")
        out = torch.empty((dW * dH + (dW * dH) % 2,), dtype=tdtype(ht), device="cuda")      # (an even count: the harness compares 32-bit words)
        sc = so.Scenario(name, inp, out, so.rand_frames(torch, (H, W), 50),
                         lambda handle, rq=rq, inp=inp, out=out, W=W, dW=dW, ht=ht: gpu.resample_half_device(rq, inp.data_ptr(), W, out.data_ptr(), dW, ht, handle))
        sc.rq, sc.lay = rq, lay
        gpu.prepare(rq)
        h.add(sc)
        sc.kernel = gpu.last_kernel()
        assert route in sc.kernel, (name, sc.kernel)
    h.calibrate()
    return h


@pytest.mark.parametrize("name", ["direct", "forwarding"])
def test_half_entry_keeps_stream_order(harness, name):
    import torch
    sc = harness.scenario(name)
    for caller in (so.Caller("torch's current stream", torch.cuda.current_stream()), so.Caller("a fresh stream", torch.cuda.Stream())):
        harness.frame_loop(sc, caller)
