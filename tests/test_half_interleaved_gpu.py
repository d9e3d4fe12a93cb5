"""The half-precision interleaved path on the MI355X (include/aai_half_interleaved.h): the direct kernel with channels against its CPU
replay bit for bit, against the oracle per channel and against the forwarding arithmetic; the forwarding route's bits; one channel
against aai_resample_half_batch_device; signed and non-finite data channel by channel; the memory contract with guarded, 2-byte-aligned,
padded buffers; address arithmetic at a wide pitch; stream order of both routes.

The forwarding arithmetic is always computed here as narrow(aai_resample_interleaved_device(widen(src))), widening and narrowing done
by torch.  The two routes' fp32 sums differ in the order of a few operations, so their rounded elements differ by at most one unit in
the last place (include/aai_half_interleaved.h); the forwarding route against that arithmetic has equal bits."""
import re

import numpy as np
import pytest

import half_cases as hc
import half_interleaved_cases as hi
import stream_order as so
import wide_pitch as wp
from conftest import TOL
from guard_layout import GuardedLayout, to_device, to_numpy

pytestmark = pytest.mark.gpu

SENTINEL16 = 0x7fa5           # a NaN in both element types that no arithmetic here produces
NAN16 = {hc.F16: 0x7e00, hc.BF16: 0x7fc0}
INF16 = {hc.F16: 0x7c00, hc.BF16: 0x7f80}
ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    aai.set_device(0)
    return aai


def tdtype(ht):
    import torch
    return torch.float16 if ht == hc.F16 else torch.bfloat16


def upload(bits, ht):
    """raw 16-bit elements -> a device tensor of the element type, same shape"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()).cuda().view(tdtype(ht))


def download(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_hi(gpu, rq, ht, src):
    """one [H, W, C] image of raw bits through resample_half_interleaved_device -> [dH, dW, C] raw bits"""
    import torch
    H, W, C = src.shape
    lay = gpu.query(rq)[2]
    x = upload(src, ht)
    y = upload(np.full((lay.dst_height, lay.dst_width, C), SENTINEL16, np.uint16), ht)
    gpu.resample_half_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), lay.dst_width * C, ht, stream=stream())
    torch.cuda.synchronize()
    return download(y)


def run_f32(gpu, rq, ht, src):
    """the widened image through aai_resample_interleaved_device -> fp32 [dH, dW, C] (a device tensor)"""
    import torch
    H, W, C = src.shape
    lay = gpu.query(rq)[2]
    x32 = upload(src, ht).float().contiguous()
    y32 = torch.full((lay.dst_height, lay.dst_width, C), float("nan"), dtype=torch.float32, device="cuda")
    gpu.resample_interleaved_device(rq, C, x32.data_ptr(), W * C, y32.data_ptr(), lay.dst_width * C, stream())
    torch.cuda.synchronize()
    return y32


def run_forwarded_with_torch(gpu, rq, ht, src):
    """narrow(aai_resample_interleaved_device(widen(src))) -> raw bits"""
    return download(run_f32(gpu, rq, ht, src).to(tdtype(ht)))


def _request(gpu, geom, mode_name):
    W, H, sr, dr, iso, ang = geom
    mode = {"area": gpu.MODE_AREA, "fast": gpu.MODE_FAST, "bilinear": gpu.MODE_BILINEAR, "bicubic": gpu.MODE_BICUBIC}[mode_name]
    return gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)


# ---- the direct route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("mode_name", hi.MODES)
@pytest.mark.parametrize("geom, channels", hi.CASES, ids=hi.CASE_IDS)
def test_direct_kernel_has_the_replays_bits(gpu, po, geom, channels, mode_name, ht, tname):
    """every case x type x mode: the kernel's output IS the replay's; it is within one rounding of the oracle per channel (the contract
    users see); and it is at most one unit in the last place from the forwarding arithmetic"""
    rq, src, want, pre, gold = hi.case(gpu, po, geom, channels, mode_name, ht)
    got = run_hi(gpu, rq, ht, src)
    kernel = gpu.last_kernel()
    assert "flagged=0 dense=0" in gpu.plan_shape(rq, channels), gpu.plan_shape(rq, channels)
    assert got.shape == want.shape
    fwd = run_forwarded_with_torch(gpu, rq, ht, src)
    assert not gpu.last_kernel().startswith("aai_axis_half_kernel")
    assert kernel == "aai_axis_half_kernel<%s>" % tname, kernel
    differ = got != want
    assert not differ.any(), (geom, channels, mode_name, tname, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    excess = max(hc.rounded_excess(hc.widen(got[:, :, c], ht), gold[:, :, c], ht) for c in range(channels))
    ulps = hc.ulp_distance(got, fwd)
    print("direct %s x%d %s %s: %.3e over the rounded-value bound; %d of %d elements differ from the forwarding arithmetic, by at most %d ulp"
          % (geom, channels, mode_name, tname, excess, int((ulps != 0).sum()), ulps.size, int(ulps.max())))
    assert excess <= 0, (geom, channels, mode_name, tname, excess)
    assert int(ulps.max()) <= 1, (geom, channels, mode_name, tname, int(ulps.max()))


def test_a_row_of_three_elements_forwards(gpu):
    geom, channels = hi.FORWARDS
    for ht, tname in hi.TYPES:
        rq = hi.request(gpu, geom, "area")
        src = hi.source_bits(geom, channels, ht)
        got = run_hi(gpu, rq, ht, src)
        kernel = gpu.last_kernel()
        assert kernel.endswith("+widened"), kernel
        assert np.array_equal(got, run_forwarded_with_torch(gpu, rq, ht, src))


# ---- the forwarding route ----------------------------------------------------------------------------------------------------
FORWARDED = [("rotated area", ROT, "area"), ("rotated fast", ROT, "fast"), ("case b at 90 degrees", hi.GEOMETRIES["b"][:5] + (90.0,), "area"),
             ("bicubic", (96, 80, 1, 2, (47.5, 39.5), 30.0), "bicubic")]


@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("channels", [2, 3, 4])
@pytest.mark.parametrize("name, geom, mode_name", FORWARDED, ids=[f[0] for f in FORWARDED])
def test_forwarding_route_has_the_interleaved_fp32_entrys_bits(gpu, name, geom, mode_name, channels, ht, tname):
    rq = _request(gpu, geom, mode_name)
    src = hi.source_bits(geom, channels, ht, seed=31)
    got = run_hi(gpu, rq, ht, src)
    kernel = gpu.last_kernel()
    assert kernel.endswith("+widened") and not kernel.startswith("aai_axis_half_kernel"), kernel
    want = run_forwarded_with_torch(gpu, rq, ht, src)
    assert gpu.last_kernel() + "+widened" == kernel
    assert np.array_equal(got, want), (name, channels, tname, int((got != want).sum()))
    assert np.isfinite(hc.widen(got, ht)).all()


@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
def test_forwarding_route_on_a_plan_with_listed_pixels(gpu, po, axis_knife_golden, ht, tname):
    """the first reference-generated axis-aligned knife geometry whose 3-channel plan lists pixels (area mode): the entry forwards and has
    the narrowed fp32 interleaved entry's bits, listed pixels included"""
    z, manifest = axis_knife_golden
    C = 3
    for i, c in enumerate(manifest):
        rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=gpu.MODE_AREA)
        gpu.prepare(rq, C)
        m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq, C))
        if int(m.group(1)) > 0 and int(m.group(2)) == 0:
            break
    else:
        pytest.fail("no axis-aligned knife geometry lists pixels")
    src = hi.source_bits((c["W"], c["H"]), C, ht, seed=c["seed"])
    got = run_hi(gpu, rq, ht, src)
    assert gpu.last_kernel().endswith("+widened"), gpu.last_kernel()
    assert np.array_equal(got, run_forwarded_with_torch(gpu, rq, ht, src))


# ---- one channel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("name, geom", [("direct", hi.GEOMETRIES["b"]), ("forwarding", ROT)])
def test_one_channel_is_the_single_channel_entry(gpu, name, geom, ht, tname):
    import torch
    W, H = geom[:2]
    rq = _request(gpu, geom, "area")
    lay = gpu.query(rq)[2]
    src = hc.source_bits(W, H, ht, seed=13)
    got = run_hi(gpu, rq, ht, src[:, :, None])[:, :, 0]
    kernel = gpu.last_kernel()
    x = upload(src, ht)
    y = upload(np.full((lay.dst_height, lay.dst_width), SENTINEL16, np.uint16), ht)
    gpu.resample_half_device(rq, x.data_ptr(), W, y.data_ptr(), lay.dst_width, ht, stream=stream())
    torch.cuda.synchronize()
    assert gpu.last_kernel() == kernel and (kernel == "aai_axis_half_kernel<%s>" % tname if name == "direct" else kernel.endswith("+widened")), kernel
    assert np.array_equal(got, download(y))


# ---- the value domain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("angle", [0.0, 180.0])
def test_signed_and_non_finite_values_stay_in_their_channel(gpu, po, angle, ht, tname):
    """case a with 3 channels of signed values, then with +Inf, -Inf and NaN planted in channel 1: the clean run has the replay's bits and
    is within the bound of the oracle; the dirty run is non-finite exactly in the planted pixels' footprints IN CHANNEL 1 and has the
    clean run's bits everywhere else, channels 0 and 2 whole"""
    W, H, sr, dr, iso, _ = hi.GEOMETRIES["a"]
    C = 3
    neg = 0x8000
    spots = ((10, 9, INF16[ht]), (40, 30, NAN16[ht]), (50, 12, INF16[ht] | neg))
    rng = np.random.default_rng(17)
    src = hc.narrow((2.0 * rng.random((H, W, C)) - 1.0).astype(np.float32), ht)
    assert (hc.widen(src, ht) < 0).any() and (hc.widen(src, ht) > 0).any()
    for mode_name in hi.MODES:
        rq = hi.request(gpu, "a", mode_name, angle=angle)
        assert hi.facts(rq, C)[7] == 1
        clean = run_hi(gpu, rq, ht, src)
        kernel = gpu.last_kernel()
        assert kernel == "aai_axis_half_kernel<%s>" % tname, kernel
        assert np.array_equal(clean, hi.replay(gpu, rq, ht, src)[0])
        # signed data cancels, so the project's bar is taken relative to the magnitude of what is summed (the oracle on |src|: the
        # forward-error bound of a weighted sum), plus one rounding of the value itself
        where = hi.GEOMETRIES["a"][:5] + (angle,)
        gold, mag = hi.oracle(po, where, mode_name, src, ht), hi.oracle(po, where, mode_name, src & 0x7fff, ht)
        err = np.abs(hc.widen(clean, ht).astype(np.float64) - gold)
        assert (err <= hc.UNIT[ht] * np.abs(gold) * (1 + TOL) + TOL * np.maximum(mag, 1e-3)).all(), (mode_name, tname, float(err.max()))
        dirty = src.copy()
        impulse = np.zeros((H, W))
        for x, y, bits in spots:
            dirty[y, x, 1] = bits
            impulse[y, x] = 1.0
        touched = po.oracle_run(hc.oracle_mode(po, mode_name), impulse, sr, dr, iso, angle).dst != 0
        assert 3 <= int(touched.sum()) <= 12
        got = run_hi(gpu, rq, ht, dirty)
        assert gpu.last_kernel() == kernel
        for c in (0, 2):
            assert np.array_equal(got[:, :, c], clean[:, :, c]), (mode_name, tname, c, "a non-finite value of channel 1 reached channel %d" % c)
        assert np.array_equal(~np.isfinite(hc.widen(got[:, :, 1], ht)), touched), (mode_name, tname)
        assert np.array_equal(got[:, :, 1][~touched], clean[:, :, 1][~touched]), (mode_name, tname)


def test_overflow_past_the_largest_fp16_value_is_infinity(gpu):
    """bicubic (the forwarding route) on a checkerboard of +-65504 overshoots: where the fp32 result rounds beyond the largest finite
    fp16 value (|v| >= 65520) the element is +-Inf, and it is finite everywhere else"""
    geom, C, ht = (96, 80, 1, 2, (47.5, 39.5), 30.0), 3, hc.F16
    W, H = geom[:2]
    y, x = np.mgrid[0:H, 0:W]
    plane = np.where((x + y) & 1, 65504.0, -65504.0).astype(np.float32)
    src = hc.narrow(np.repeat(plane[:, :, None], C, axis=2), ht)
    rq = _request(gpu, geom, "bicubic")
    got = run_hi(gpu, rq, ht, src)
    assert gpu.last_kernel().endswith("+widened")
    f32 = run_f32(gpu, rq, ht, src).cpu().numpy()
    over = np.abs(f32) >= 65520.0
    assert over.any() and not over.all()
    wide = hc.widen(got, ht)
    assert np.array_equal(np.isinf(wide), over) and np.array_equal(np.sign(wide[over]), np.sign(f32[over])) and not np.isnan(wide).any()


# ---- the memory contract -------------------------------------------------------------------------------------------------------
def guarded_batch(gpu, rq, geometry, channels, ht, what):
    """Batch 3 through the device entry; base addresses ONE element past a 256-byte boundary (2-byte aligned and nothing more); odd padded
    row strides on both sides (row strides larger than the row); image strides larger than the image.  Source padding is pre-filled
    with NaN: a read of it would reach the output, and it is checked unchanged.  Destination: every element starts as a sentinel, and
    none outside the entitled elements may change.  -> (the kernel's name, the [3, dH, dW, C] output, the three source images)"""
    import torch
    B = 3
    W, H = geometry[:2]
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    sstride = W * channels + 3 + (W * channels) % 2                  # odd
    dstride = dW * channels + 5 + (dW * channels) % 2                # odd
    assert sstride % 2 == 1 and dstride % 2 == 1
    sl = GuardedLayout((B, H, W, channels), "u16", stride=sstride, image_stride=H * sstride + 11, base_offset=1)
    dl = GuardedLayout((B, dH, dW, channels), "u16", stride=dstride, image_stride=dH * dstride + 7, base_offset=1)
    images = [hi.source_bits(geometry, channels, ht, seed=20 + b) for b in range(B)]
    sbuf = sl.make_src(np.stack(images), "zeros")
    sbuf[~sl.entitled] = NAN16[ht]
    dbuf = np.full(dl.total, SENTINEL16, np.uint16)
    ds, dd = to_device(sbuf), to_device(dbuf)
    assert sl.ptr(ds) % 4 == 2 and dl.ptr(dd) % 4 == 2
    gpu.resample_half_interleaved_device(rq, channels, sl.ptr(ds), sstride, dl.ptr(dd), dstride, ht, stream=stream(), batch=B,
                                         src_image_stride=sl.image_stride, dst_image_stride=dl.image_stride)
    torch.cuda.synchronize()
    kernel = gpu.last_kernel()
    after = to_numpy(dd, np.uint16)
    changed = np.flatnonzero((after != SENTINEL16) & ~dl.entitled)
    assert changed.size == 0, (what, [dl.describe(int(o) - dl.lead) for o in changed[:4]])
    assert np.array_equal(to_numpy(ds, np.uint16), sbuf)
    out = after[dl.index].reshape(B, dH, dW, channels)
    assert not (out == SENTINEL16).any(), (what, "entitled elements not written")
    return kernel, out, images


@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("mode_name", hi.MODES)
@pytest.mark.parametrize("geom, channels", hi.CASES, ids=hi.CASE_IDS)
def test_direct_kernel_batch_of_three_in_padded_buffers(gpu, geom, channels, mode_name, ht, tname):
    """every case x mode x type as guarded_batch runs it: the direct kernel, pad elements and gaps untouched, and every image of the batch
    with the replay's bits -- packed (0 degrees) and scattered (180 degrees) stores, at most 64 and more outputs per strip, rows of
    4 and of 777 elements, 13-row windows"""
    rq = hi.request(gpu, geom, mode_name)
    what = (geom, channels, mode_name, tname)
    kernel, out, images = guarded_batch(gpu, rq, hi.GEOMETRIES[geom], channels, ht, what)
    assert kernel == "aai_axis_half_kernel<%s>" % tname, kernel
    for b, image in enumerate(images):
        assert np.array_equal(out[b], hi.replay(gpu, rq, ht, image)[0]), what + (b,)


@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("name, geom", [("rotated", ROT), ("case b at 90 degrees", hi.GEOMETRIES["b"][:5] + (90.0,))])
def test_forwarding_route_batch_of_three_in_padded_buffers(gpu, name, geom, ht, tname):
    C = 3
    rq = _request(gpu, geom, "area")
    kernel, out, images = guarded_batch(gpu, rq, geom, C, ht, (name, tname))
    assert kernel.endswith("+widened"), kernel
    for b, image in enumerate(images):
        assert np.array_equal(out[b], run_forwarded_with_torch(gpu, rq, ht, image)), (name, tname, b)


# ---- address arithmetic at a wide pitch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, angle", [("direct", 180.0), ("forwarding", 17.5)])
def test_rows_beyond_2_31_elements(gpu, name, angle):
    """one small bf16 RGB image in source and destination views whose last rows start beyond 2^31 elements (the method of
    tests/wide_pitch.py: a strided view into an arena that is never filled whole; about 4.3 GiB each): the tight call's bits, the
    elements behind every dst row untouched"""
    import torch
    geom, C, ht = (120, 41, 2, 1, (59.5, 20.0), angle), 3, hc.BF16
    W, H = geom[:2]
    rq = _request(gpu, geom, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    src = hi.source_bits(geom, C, ht, seed=5)
    tight = run_hi(gpu, rq, ht, src)
    kernel = gpu.last_kernel()
    if name == "direct":
        assert kernel == "aai_axis_half_kernel<bf16>" and np.array_equal(tight, hi.replay(gpu, rq, ht, src)[0])
    else:
        assert kernel.endswith("+widened") and np.array_equal(tight, run_forwarded_with_torch(gpu, rq, ht, src))
    spitch, dpitch = -(-(1 << 31) // (H - 1)) + 5, -(-(1 << 31) // (dH - 1)) + 5
    spitch, dpitch = spitch | 1, dpitch | 1                                            # odd: rows alternate between 4-byte phases
    assert (H - 1) * spitch >= 1 << 31 and (dH - 1) * dpitch >= 1 << 31
    sa = wp.Arena(wp.extent_bytes(H, W * C, spitch, 2))
    da = wp.Arena(wp.extent_bytes(dH, dW * C, dpitch, 2))
    try:
        sptr = wp.place_source(sa, src, "u16", spitch)
        drows, dguard = da.view("u16", dH, dW * C, dpitch)
        drows.fill_(0x7fa5)
        dguard.fill_(0x7fa5)
        gpu.resample_half_interleaved_device(rq, C, sptr, spitch, drows.data_ptr(), dpitch, ht, stream=stream())
        torch.cuda.synchronize()
        assert gpu.last_kernel() == kernel
        assert np.array_equal(drows.cpu().numpy().view(np.uint16).reshape(dH, dW, C), tight)
        assert bool((dguard == 0x7fa5).all())
    finally:
        sa.free()
        da.free()


# ---- stream order ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(gpu):
    """one scenario per route: the call between a delayed producer and a consumer on the caller's stream, no host wait (stream_order.py)"""
    import torch
    h = so.Harness(gpu)
    C = 3
    for name, geom, ht, route in (("direct", hi.GEOMETRIES["d"], hc.F16, "aai_axis_half_kernel"), ("forwarding", ROT, hc.BF16, "+widened")):
        W, H = geom[:2]
        rq = _request(gpu, geom, "area")
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        n = dW * dH * C
        inp = torch.empty((H, W, C), dtype=tdtype(ht), device="cuda")
        out = torch.empty((n + n % 2,), dtype=tdtype(ht), device="cuda")      # (an even count: the harness compares 32-bit words)
        sc = so.Scenario(name, inp, out, so.rand_frames(torch, (H, W, C), 50),
                         lambda handle, rq=rq, inp=inp, out=out, W=W, dW=dW, ht=ht: gpu.resample_half_interleaved_device(rq, C, inp.data_ptr(), W * C, out.data_ptr(),
                                                                                                                         dW * C, ht, handle))
        sc.rq, sc.lay = rq, lay
        gpu.prepare(rq, C)
        h.add(sc)
        sc.kernel = gpu.last_kernel()
        assert route in sc.kernel, (name, sc.kernel)
    h.calibrate()
    return h


@pytest.mark.parametrize("name", ["direct", "forwarding"])
def test_half_interleaved_entry_keeps_stream_order(harness, name):
    import torch
    sc = harness.scenario(name)
    for caller in (so.Caller("torch's current stream", torch.cuda.current_stream()), so.Caller("a fresh stream", torch.cuda.Stream())):
        harness.frame_loop(sc, caller)
