"""The integer path on the MI355X (include/aai_int.h): the direct kernel against its CPU replay bit for bit, against the oracle and against
the forwarding arithmetic; the forwarding route's bits; the memory contract with guarded, element-aligned, padded buffers; address
arithmetic at a wide pitch; stream order of both routes; a batch beyond one launch's grid.z.

The forwarding arithmetic is always computed here as quantize(aai_resample_interleaved_device(src)) with the conversion in numpy
(int_cases.quantize: np.clip(np.rint(x), 0, max))."""
import re

import numpy as np
import pytest

import int_cases as ic
import stream_order as so
import wide_pitch as wp
from guard_layout import GuardedLayout, poisons, to_device, to_numpy

pytestmark = pytest.mark.gpu

KERNEL = {ic.U8: "aai_axis_int_kernel<u8>", ic.U16: "aai_axis_int_kernel<u16>"}
GNAME = {ic.U8: "u8", ic.U16: "u16"}
PATTERN = 0xA5           # every byte of a destination before the call


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    aai.set_device(0)
    return aai


def upload(a):
    """a host array as raw bytes on the device (a torch uint8 tensor)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_int(gpu, rq, dt, src):
    """one [H, W, C] image through resample_int_device -> [dH, dW, C]"""
    import torch
    H, W, C = src.shape
    lay = gpu.query(rq)[2]
    x = upload(src)
    y = upload(np.full((lay.dst_height, lay.dst_width, C), PATTERN, ic.NP[dt]))
    gpu.resample_int_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), lay.dst_width * C, dt, stream=stream())
    torch.cuda.synchronize()
    return y.cpu().numpy().view(ic.NP[dt]).reshape(lay.dst_height, lay.dst_width, C)


def run_f32(gpu, rq, dt, src):
    """the same image through aai_resample_interleaved_device -> fp32 [dH, dW, C]"""
    import torch
    H, W, C = src.shape
    lay = gpu.query(rq)[2]
    x = upload(src)
    y = torch.full((lay.dst_height, lay.dst_width, C), float("nan"), dtype=torch.float32, device="cuda")
    gpu.resample_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), lay.dst_width * C, stream(), src_dtype=dt)
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ---- the direct route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt, tname", ic.TYPES, ids=[t[1] for t in ic.TYPES])
@pytest.mark.parametrize("mode_name", ic.MODES)
@pytest.mark.parametrize("geom, channels", ic.CASES, ids=ic.CASE_IDS)
def test_direct_kernel_has_the_replays_bits(gpu, po, geom, channels, mode_name, dt, tname):
    """every case x type x mode, on the random, the constant and the checkerboard source: the kernel's output IS the replay's; it is
    within one conversion of the oracle per channel (the contract users see); and it is at most one count from the forwarding arithmetic"""
    for kind in ic.SOURCES:
        rq, src, want, pre, gold = ic.case(gpu, po, geom, channels, mode_name, dt, kind)
        got = run_int(gpu, rq, dt, src)
        kernel = gpu.last_kernel()
        assert "flagged=0 dense=0" in gpu.plan_shape(rq, channels), gpu.plan_shape(rq, channels)
        assert got.shape == want.shape
        over = ic.excess(got, gold)
        f32 = run_f32(gpu, rq, dt, src)
        assert not gpu.last_kernel().startswith("aai_axis_int_kernel")
        if ic.direct(rq, channels, dt):
            assert kernel == KERNEL[dt], kernel
            differ = got != want
            assert not differ.any(), (geom, channels, mode_name, tname, kind, int(differ.sum()), np.argwhere(differ)[:4].tolist())
        else:
            # the class the measurement sends to the forwarding route (u8, at most 64 outputs per strip): the quantized fp32 entry's bits,
            # at most one count from the replay
            assert kernel == gpu.last_kernel() + "+quantized", kernel
            assert np.array_equal(got, ic.quantize(f32, dt)), (geom, channels, mode_name, tname, kind)
            assert int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()) <= 1, (geom, channels, mode_name, tname, kind)
        apart = np.abs(got.astype(np.int64) - ic.quantize(f32, dt).astype(np.int64))
        print("direct %s x%d %s %s %s: %.3e over the bound; %d of %d elements differ from the forwarding arithmetic, by at most %d"
              % (geom, channels, mode_name, tname, kind, over, int((apart != 0).sum()), apart.size, int(apart.max())))
        assert over <= 0, (geom, channels, mode_name, tname, kind, over)
        assert int(apart.max()) <= 1, (geom, channels, mode_name, tname, kind, int(apart.max()))


# ---- the forwarding route ----------------------------------------------------------------------------------------------------
ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)
FORWARDED = [("rotated area", ROT, "area", "random"), ("rotated fast", ROT, "fast", "random"),
             ("case b at 90 degrees", ic.GEOMETRIES["b"][:5] + (90.0,), "area", "random"),
             ("bicubic on the checkerboard", (96, 80, 1, 2, (47.5, 39.5), 30.0), "bicubic", "checker")]


def _request(gpu, geom, mode_name):
    W, H, sr, dr, iso, ang = geom
    mode = {"area": gpu.MODE_AREA, "fast": gpu.MODE_FAST, "bilinear": gpu.MODE_BILINEAR, "bicubic": gpu.MODE_BICUBIC}[mode_name]
    return gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)


@pytest.mark.parametrize("dt, tname", ic.TYPES, ids=[t[1] for t in ic.TYPES])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name, geom, mode_name, kind", FORWARDED, ids=[f[0] for f in FORWARDED])
def test_forwarding_route_is_the_quantized_fp32_entry(gpu, name, geom, mode_name, kind, channels, dt, tname):
    rq = _request(gpu, geom, mode_name)
    src = ic.source(geom, channels, dt, kind, seed=31)
    got = run_int(gpu, rq, dt, src)
    kernel = gpu.last_kernel()
    assert kernel.endswith("+quantized") and not kernel.startswith("aai_axis_int_kernel"), kernel
    f32 = run_f32(gpu, rq, dt, src)
    assert gpu.last_kernel() + "+quantized" == kernel
    want = ic.quantize(f32, dt)
    assert np.array_equal(got, want), (name, channels, tname, int((got != want).sum()))
    if mode_name == "bicubic":
        # the sampler overshoots on the checkerboard: both ends saturate, exactly where the fp32 output leaves the range
        low, high = f32 < 0, f32 > ic.MAXV[dt]
        assert low.any() and high.any(), (float(f32.min()), float(f32.max()))
        assert (got[low] == 0).all() and (got[high] == ic.MAXV[dt]).all()


@pytest.mark.parametrize("dt, tname", ic.TYPES, ids=[t[1] for t in ic.TYPES])
def test_forwarding_route_on_a_plan_with_listed_pixels(gpu, po, axis_knife_golden, dt, tname):
    """the first reference-generated axis-aligned knife geometry whose plan lists pixels (area mode): the integer entry forwards and has
    the quantized fp32 entry's bits, listed pixels included"""
    z, manifest = axis_knife_golden
    for i, c in enumerate(manifest):
        rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=gpu.MODE_AREA)
        gpu.prepare(rq)
        m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq))
        if int(m.group(1)) > 0 and int(m.group(2)) == 0:
            break
    else:
        pytest.fail("no axis-aligned knife geometry lists pixels")
    src = ic.source((c["W"], c["H"]), 1, dt, "random", seed=c["seed"])
    got = run_int(gpu, rq, dt, src)
    assert gpu.last_kernel().endswith("+quantized"), gpu.last_kernel()
    assert np.array_equal(got, ic.quantize(run_f32(gpu, rq, dt, src), dt))


def test_forwarding_route_batch_with_padded_strides(gpu):
    import torch
    B, C, dt = 3, 3, ic.U8
    W, H = ROT[:2]
    rq = _request(gpu, ROT, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    sl = GuardedLayout((B, H, W, C), "u8", stride=W * C + 5, image_stride=H * (W * C + 5) + 11, base_offset=1)
    dl = GuardedLayout((B, dH, dW, C), "u8", stride=dW * C + 7, image_stride=dH * (dW * C + 7) + 3, base_offset=3)
    images = [ic.source(ROT, C, dt, "random", seed=40 + b) for b in range(B)]
    sbuf = sl.make_src(np.stack(images), "ones")
    ds, dd = to_device(sbuf), to_device(np.full(dl.total, PATTERN, np.uint8))
    gpu.resample_int_device(rq, C, sl.ptr(ds), sl.stride, dl.ptr(dd), dl.stride, dt, stream=stream(), batch=B,
                            src_image_stride=sl.image_stride, dst_image_stride=dl.image_stride)
    torch.cuda.synchronize()
    assert gpu.last_kernel().endswith("+quantized")
    after = to_numpy(dd, np.uint8)
    assert not ((after != PATTERN) & ~dl.entitled).any()
    out = after[dl.index].reshape(B, dH, dW, C)
    for b in range(B):
        assert np.array_equal(out[b], ic.quantize(run_f32(gpu, rq, dt, images[b]), dt)), b


# ---- the memory contract -------------------------------------------------------------------------------------------------------
CONTRACT = [("b", ic.GEOMETRIES["b"], "direct"), ("c", ic.GEOMETRIES["c"], "direct"), ("e", ic.GEOMETRIES["e"], "direct"), ("rotated", ROT, "forwarding")]


@pytest.mark.parametrize("dt, tname", ic.TYPES, ids=[t[1] for t in ic.TYPES])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name, geom, route", CONTRACT, ids=[c[0] for c in CONTRACT])
def test_memory_contract(gpu, name, geom, route, channels, dt, tname):
    """batch 2; base addresses 1, 2 and 3 elements past a 256-byte boundary (odd u8 pointers); padded row strides that are no multiple
    of 4; gaps between the images.  Source: everything the call is not entitled to holds poison, once all zeros and once all ones -- the
    outputs must agree bit for bit.  Destination: every byte starts as a pattern, and no byte outside the entitled elements may change
    (an entitled element may legitimately equal the pattern, so only the guard regions are compared)."""
    import torch
    B = 2
    W, H = geom[:2]
    tn = GNAME[dt]
    rq = _request(gpu, geom, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    images = np.stack([ic.source(geom, channels, dt, "random", seed=20 + b) for b in range(B)])
    singles = [run_int(gpu, rq, dt, images[b]) for b in range(B)]
    for base in (1, 2, 3):
        sstride = W * channels + 1 + base
        sstride += 1 if sstride % 4 == 0 else 0
        dstride = dW * channels + 4 + base
        dstride += 1 if dstride % 4 == 0 else 0
        assert sstride % 4 and dstride % 4
        sl = GuardedLayout((B, H, W, channels), tn, stride=sstride, image_stride=H * sstride + 7, base_offset=base)
        dl = GuardedLayout((B, dH, dW, channels), tn, stride=dstride, image_stride=dH * dstride + 5, base_offset=4 - base)
        outs = []
        for poison in poisons(tn):
            sbuf = sl.make_src(images, poison)
            dbuf = np.full(dl.total * ic.NP[dt]().itemsize, PATTERN, np.uint8)
            ds, dd = to_device(sbuf), to_device(dbuf)
            assert sl.ptr(ds) % 256 == base * sbuf.itemsize
            gpu.resample_int_device(rq, channels, sl.ptr(ds), sstride, dl.ptr(dd), dstride, dt, stream=stream(), batch=B,
                                    src_image_stride=sl.image_stride, dst_image_stride=dl.image_stride)
            torch.cuda.synchronize()
            kernel = gpu.last_kernel()
            assert (kernel == KERNEL[dt]) if route == "direct" and ic.direct(rq, channels, dt) else kernel.endswith("+quantized"), kernel
            after = to_numpy(dd, np.uint8)
            guard = np.repeat(~dl.entitled, ic.NP[dt]().itemsize)
            changed = np.flatnonzero((after != PATTERN) & guard)
            assert changed.size == 0, (name, channels, tname, base, poison, [dl.describe(int(o) // ic.NP[dt]().itemsize - dl.lead) for o in changed[:4]])
            assert np.array_equal(to_numpy(ds, ic.NP[dt]), sbuf)
            outs.append(after.view(ic.NP[dt])[dl.index].reshape(B, dH, dW, channels))
        assert np.array_equal(outs[0], outs[1]), (name, channels, tname, base, "the output depends on the padding")
        for b in range(B):
            assert np.array_equal(outs[0][b], singles[b]), (name, channels, tname, base, b)


# ---- address arithmetic at a wide pitch ------------------------------------------------------------------------------------------
def test_direct_kernel_addresses_rows_beyond_2_31_elements(gpu, po):
    """one small u8 RGB image in source and destination views whose last rows start beyond 2^31 elements (the method of
    tests/wide_pitch.py: a strided view into an arena that is never filled whole; about 2.2 GiB each): the tight call's bits"""
    import torch
    geom, C, dt = (300, 300, 2, 1, (149.5, 149.5), 180.0), 3, ic.U8
    W, H = geom[:2]
    rq = _request(gpu, geom, "area")
    assert ic.facts(rq, C)[7] == 1
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    src = ic.source(geom, C, dt, "random", seed=5)
    tight = run_int(gpu, rq, dt, src)
    assert gpu.last_kernel() == KERNEL[dt] and np.array_equal(tight, ic.replay(gpu, rq, dt, src)[0])
    spitch, dpitch = -(-(1 << 31) // (H - 1)) + 5, -(-(1 << 31) // (dH - 1)) + 5        # odd: no row starts on a power of two
    assert (H - 1) * spitch >= 1 << 31 and (dH - 1) * dpitch >= 1 << 31
    sa = wp.Arena(wp.extent_bytes(H, W * C, spitch, 1))
    da = wp.Arena(wp.extent_bytes(dH, dW * C, dpitch, 1))
    try:
        sptr = wp.place_source(sa, src, "u8", spitch)
        drows, dguard = da.view("u8", dH, dW * C, dpitch)
        drows.fill_(PATTERN)
        dguard.fill_(PATTERN)
        gpu.resample_int_device(rq, C, sptr, spitch, drows.data_ptr(), dpitch, dt, stream=stream())
        torch.cuda.synchronize()
        assert gpu.last_kernel() == KERNEL[dt]
        assert np.array_equal(drows.cpu().numpy().reshape(dH, dW, C), tight)
        assert bool((dguard == PATTERN).all())
    finally:
        sa.free()
        da.free()


# ---- stream order ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(gpu):
    """one scenario per route: the call between a delayed producer and a consumer on the caller's stream, no host wait (stream_order.py).
    u8 RGB; the output buffer is held as 32-bit words, which is what the harness compares and fills."""
    import torch
    h = so.Harness(gpu)
    C = 3
    for name, geom, route in (("direct", ic.GEOMETRIES["d"], "aai_axis_int_kernel<u8>"), ("forwarding", ROT, "+quantized")):
        W, H = geom[:2]
        rq = _request(gpu, geom, "area")
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        inp = torch.empty((H, W, C), dtype=torch.uint8, device="cuda")
        out = torch.empty(((dW * dH * C + 3) // 4,), dtype=torch.int32, device="cuda")
        sc = so.Scenario(name, inp, out, so.rand_frames(torch, (H, W, C), 60, torch.uint8),
                         lambda handle, rq=rq, inp=inp, out=out, W=W, dW=dW: gpu.resample_int_device(rq, C, inp.data_ptr(), W * C, out.data_ptr(), dW * C, ic.U8, handle),
                         poison=255)
        sc.rq, sc.lay = rq, lay
        gpu.prepare(rq, C)
        h.add(sc)
        sc.kernel = gpu.last_kernel()
        assert route in sc.kernel, (name, sc.kernel)
    h.calibrate()
    return h


@pytest.mark.parametrize("name", ["direct", "forwarding"])
def test_int_entry_keeps_stream_order(harness, name):
    import torch
    sc = harness.scenario(name)
    for caller in (so.Caller("torch's current stream", torch.cuda.current_stream()), so.Caller("a fresh stream", torch.cuda.Stream())):
        harness.frame_loop(sc, caller)


# ---- a batch beyond one launch's grid.z -------------------------------------------------------------------------------------------
def test_direct_route_batch_beyond_one_launch(gpu):
    """65535 + 3 images of 5 x 7 u16 pixels (4.6 MB): the engine splits the batch into two launches; every image has the single call's bits"""
    import torch
    geom, dt = ic.GEOMETRIES["h"], ic.U16
    W, H = geom[:2]
    B = 65535 + 3
    rq = _request(gpu, geom, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    src = np.random.default_rng(9).integers(0, 65536, size=(B, H, W, 1)).astype(np.uint16)
    x = upload(src)
    y = upload(np.full((B, dH, dW, 1), PATTERN, np.uint16))
    gpu.resample_int_device(rq, 1, x.data_ptr(), W, y.data_ptr(), dW, dt, stream=stream(), batch=B, src_image_stride=H * W, dst_image_stride=dH * dW)
    torch.cuda.synchronize()
    assert gpu.last_kernel() == KERNEL[dt]
    got = y.cpu().numpy().view(np.uint16).reshape(B, dH, dW, 1)
    for b in (0, 1, 65534, 65535, 65536, B - 1):
        assert np.array_equal(got[b], ic.replay(gpu, rq, dt, src[b])[0]), b
    # every image at once: the images are independent, so a permutation of the batch permutes the results
    perm = np.random.default_rng(10).permutation(B)
    x2 = upload(src[perm])
    y2 = upload(np.full((B, dH, dW, 1), PATTERN, np.uint16))
    gpu.resample_int_device(rq, 1, x2.data_ptr(), W, y2.data_ptr(), dW, dt, stream=stream(), batch=B, src_image_stride=H * W, dst_image_stride=dH * dW)
    torch.cuda.synchronize()
    assert np.array_equal(y2.cpu().numpy().view(np.uint16).reshape(B, dH, dW, 1), got[perm])
