"""Resample-and-convert on the MI355X (include/ext/aai_convert.h): the direct kernel against its CPU replay bit for bit over the case table;
the forwarding route against the conversion of the fp32 entry's downloaded output; the memory contract with guarded, element-aligned,
padded buffers (planes included); stream order of both routes; batches, one of them beyond a launch's grid.z; the host entry."""
import re

import numpy as np
import pytest

import convert_cases as cc
import int_cases as ic
import stream_order as so
from guard_layout import GuardedLayout, poisons, to_device, to_numpy

pytestmark = pytest.mark.gpu

PATTERN = 0xA5           # every byte of a destination before the call
OUT_BYTES = {cc.F32: 4, cc.F16: 2, cc.BF16: 2}


def kernel_name(st, ot):
    return "aai_axis_convert_kernel<%s,%s>" % (cc.SRC_NAME[st], cc.OUT_NAME[ot])


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


def _request(gpu, geom, mode_name):
    W, H, sr, dr, iso, ang = geom
    mode = {"area": gpu.MODE_AREA, "fast": gpu.MODE_FAST, "bilinear": gpu.MODE_BILINEAR, "bicubic": gpu.MODE_BICUBIC}[mode_name]
    return gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)


def run_convert(gpu, rq, st, src, scale, offset, ot, lay):
    """one [H, W, C] image through resample_convert_device, dense -> [dH, dW, C] or [C, dH, dW] of the output type's raw elements"""
    import torch
    H, W, C = src.shape
    l = gpu.query(rq)[2]
    dH, dW = l.dst_height, l.dst_width
    x = upload(src)
    y = upload(np.full(cc.out_shape(dH, dW, C, lay), PATTERN, np.uint8).repeat(OUT_BYTES[ot]))
    cv = gpu.make_convert(C, ot, lay == cc.PLANAR, scale[:C], offset[:C])
    gpu.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW if lay == cc.PLANAR else dW * C, st, cv, stream=stream(),
                                dst_plane_stride=dW * dH)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(cc.OUT_NP[ot]).reshape(cc.out_shape(dH, dW, C, lay))


def run_f32(gpu, rq, st, src):
    """the same image through aai_resample_interleaved_device -> fp32 [dH, dW, C]"""
    import torch
    H, W, C = src.shape
    l = gpu.query(rq)[2]
    x = upload(src)
    y = torch.full((l.dst_height, l.dst_width, C), float("nan"), dtype=torch.float32, device="cuda")
    gpu.resample_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), l.dst_width * C, stream(), src_dtype=st)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_route(gpu, rq, st, src, scale, offset, ot, lay, direct, tag):
    """one call: on the direct route the replay's bits under the kernel's name; on the forwarding route the conversion of the fp32 entry's
    output under that entry's kernel name + "+converted" """
    got = run_convert(gpu, rq, st, src, scale, offset, ot, lay)
    kernel = gpu.last_kernel()
    if direct:
        assert kernel == kernel_name(st, ot), (tag, kernel)
        want = cc.replay(gpu, rq, st, src, scale, offset, ot, lay)[0]
    else:
        f32 = run_f32(gpu, rq, st, src)
        assert kernel == gpu.last_kernel() + "+converted" and not kernel.startswith("aai_axis_convert_kernel"), (tag, kernel, gpu.last_kernel())
        want = cc.apply(f32, scale, offset, ot, lay)
    differ = got.view(np.uint8) != want.view(np.uint8)
    assert got.shape == want.shape and not differ.any(), (tag, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    return got


# ---- the direct route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom, channels, st, ot, lay", cc.CASES, ids=cc.CASE_IDS)
def test_direct_kernel_has_the_replays_bits(gpu, geom, channels, st, ot, lay):
    """every case x mode x conversion on the random and the constant source: the kernel's output IS the replay's (which
    tests/test_convert_host.py holds to the oracle).  A class that the measurement sends to forwarding is checked as forwarding."""
    for mode_name in cc.MODES:
        rq = ic.request(gpu, geom, mode_name)
        for kind in ("random", "constant"):
            src = ic.source(geom, channels, st, kind)
            for conv in cc.CONVERSIONS:
                scale, offset = cc.conversion(conv, st)
                check_route(gpu, rq, st, src, scale, offset, ot, lay, cc.direct(rq, channels, st, ot, lay), (geom, channels, mode_name, kind, conv))
        assert "flagged=0 dense=0" in gpu.plan_shape(rq, channels), gpu.plan_shape(rq, channels)


@pytest.mark.parametrize("name", sorted(cc.OFF_IMAGE))
def test_outputs_off_the_image_are_the_rounded_offset(gpu, name):
    geom, C = cc.OFF_IMAGE[name], 3
    rq = ic.request(gpu, geom, "fast")
    for st in (ic.U8, ic.U16):
        src = ic.source(geom, C, st, "random", seed=3)
        blank = run_f32(gpu, rq, st, ic.source(geom, C, st, "constant")) == 0
        assert blank.any()
        scale, offset = cc.conversion("edge", st)
        for ot, _ in cc.OUT_TYPES:
            for lay in (cc.INTERLEAVED, cc.PLANAR):
                got = cc.to_hwc(check_route(gpu, rq, st, src, scale, offset, ot, lay, cc.direct(rq, C, st, ot, lay), (name, st, ot, lay)), lay)
                want = np.broadcast_to(cc.narrow(offset[:C], ot), got.shape)
                assert np.array_equal(got[blank], want[blank]), (name, st, ot, lay)


# ---- the forwarding route ----------------------------------------------------------------------------------------------------
ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)
P = (1, 9, 1, 1, (0, 4), 0.0)          # with 3 channels: a row of 3 elements, fewer than the strip form loads
FORWARDED = [("rotated area", ROT, "area", "random", (1, 3)), ("case b at 90 degrees", ic.GEOMETRIES["b"][:5] + (90.0,), "area", "random", (1, 3)),
             ("bicubic on the checkerboard", (96, 80, 1, 2, (47.5, 39.5), 30.0), "bicubic", "checker", (1, 3)), ("a row of 3 elements", P, "area", "random", (3,))]
FORMS = [(cc.F16, cc.PLANAR), (cc.F32, cc.INTERLEAVED), (cc.BF16, cc.INTERLEAVED), (cc.F32, cc.PLANAR)]


@pytest.mark.parametrize("st, sname", ic.TYPES, ids=[t[1] for t in ic.TYPES])
@pytest.mark.parametrize("name, geom, mode_name, kind, channel_counts", FORWARDED, ids=[f[0] for f in FORWARDED])
def test_forwarding_route_is_the_converted_fp32_entry(gpu, name, geom, mode_name, kind, channel_counts, st, sname):
    rq = _request(gpu, geom, mode_name)
    for channels in channel_counts:
        src = ic.source(geom, channels, st, kind, seed=31)
        for ot, lay in FORMS:
            for conv in ("normalise", "edge"):
                scale, offset = cc.conversion(conv, st)
                check_route(gpu, rq, st, src, scale, offset, ot, lay, False, (name, channels, sname, ot, lay, conv))


@pytest.mark.parametrize("st, sname", ic.TYPES, ids=[t[1] for t in ic.TYPES])
def test_forwarding_route_on_a_plan_with_listed_pixels(gpu, axis_knife_golden, st, sname):
    """the first reference-generated axis-aligned knife geometry whose plan lists pixels (area mode), the one tests/test_int_gpu.py uses"""
    z, manifest = axis_knife_golden
    for c in manifest:
        rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=gpu.MODE_AREA)
        gpu.prepare(rq)
        m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq))
        if int(m.group(1)) > 0 and int(m.group(2)) == 0:
            break
    else:
        pytest.fail("no axis-aligned knife geometry lists pixels")
    src = ic.source((c["W"], c["H"]), 1, st, "random", seed=c["seed"])
    scale, offset = cc.conversion("normalise", st)
    for ot, lay in FORMS[:2]:
        check_route(gpu, rq, st, src, scale, offset, ot, lay, False, ("listed", sname, ot, lay))


# ---- the memory contract -------------------------------------------------------------------------------------------------------
class GuardedPlanes:
    """a planar destination [B, C, dH, dW] inside one allocation between two guard margins, in the manner of guard_layout.GuardedLayout:
    element (b, c, y, x) at lead + b image_stride + c plane_stride + y stride + x"""

    def __init__(self, B, C, dH, dW, stride, plane_stride, image_stride, base_offset, itemsize):
        assert stride >= dW and plane_stride >= dH * stride and image_stride >= C * plane_stride
        self.stride, self.plane_stride, self.image_stride = stride, plane_stride, image_stride
        margin = 8 * stride + 1024
        per = 256 // itemsize
        self.lead = -(-margin // per) * per + base_offset
        span = (B - 1) * image_stride + (C - 1) * plane_stride + (dH - 1) * stride + dW
        self.total = self.lead + span + margin
        b, c, y, x = np.meshgrid(np.arange(B), np.arange(C), np.arange(dH), np.arange(dW), indexing="ij")
        self.index = (self.lead + b * image_stride + c * plane_stride + y * stride + x).astype(np.int64)
        self.entitled = np.zeros(self.total, bool)
        self.entitled[self.index.reshape(-1)] = True
        assert int(self.entitled.sum()) == B * C * dH * dW


CONTRACT = [("b", ic.GEOMETRIES["b"], "direct"), ("c", ic.GEOMETRIES["c"], "direct"), ("e", ic.GEOMETRIES["e"], "direct"), ("rotated", ROT, "forwarding"),
            ("b at 90 degrees", ic.GEOMETRIES["b"][:5] + (90.0,), "forwarding")]


@pytest.mark.parametrize("st, sname", ic.TYPES, ids=[t[1] for t in ic.TYPES])
@pytest.mark.parametrize("ot, lay", [(cc.F16, cc.PLANAR), (cc.F32, cc.INTERLEAVED), (cc.F32, cc.PLANAR), (cc.F16, cc.INTERLEAVED)], ids=["f16-nchw", "f32-nhwc", "f32-nchw", "f16-nhwc"])
@pytest.mark.parametrize("name, geom, route", CONTRACT, ids=[c[0] for c in CONTRACT])
def test_memory_contract(gpu, name, geom, route, ot, lay, st, sname):
    """batch 2, three channels; base addresses one element past a 256-byte boundary; padded row strides that are no multiple of 4; a plane
    stride larger than a plane; gaps between the images.  Source: everything the call is not entitled to holds poison, once all zeros
    and once all ones -- the outputs must agree bit for bit.  Destination: every byte starts as a pattern, no byte outside the
    entitled elements may change, and the entitled elements hold the tight call's bits (so every one of them was written)."""
    import torch
    B, C = 2, 3
    W, H = geom[:2]
    tn = cc.SRC_NAME[st]
    rq = _request(gpu, geom, "area")
    l = gpu.query(rq)[2]
    dW, dH = l.dst_width, l.dst_height
    scale, offset = cc.conversion("normalise", st)
    images = np.stack([ic.source(geom, C, st, "random", seed=20 + b) for b in range(B)])
    direct = route == "direct" and cc.direct(rq, C, st, ot, lay)
    singles = [check_route(gpu, rq, st, images[b], scale, offset, ot, lay, direct, (name, b)) for b in range(B)]
    osz = OUT_BYTES[ot]
    sstride = W * C + 3
    sstride += 1 if sstride % 4 == 0 else 0
    sl = GuardedLayout((B, H, W, C), tn, stride=sstride, image_stride=H * sstride + 7, base_offset=1)
    if lay == cc.PLANAR:
        dstride = dW + 5 + (1 if (dW + 5) % 4 == 0 else 0)
        dl = GuardedPlanes(B, C, dH, dW, dstride, dH * dstride + 9, C * (dH * dstride + 9) + 11, 1, osz)
    else:
        dstride = dW * C + 5 + (1 if (dW * C + 5) % 4 == 0 else 0)
        dl = GuardedLayout((B, dH, dW, C), "f32" if ot == cc.F32 else "u16", stride=dstride, image_stride=dH * dstride + 5, base_offset=1)
        dl.plane_stride = 0
    assert sstride % 4 and dstride % 4
    cv = gpu.make_convert(C, ot, lay == cc.PLANAR, scale[:C], offset[:C])
    outs = []
    for poison in poisons(tn):
        sbuf = sl.make_src(images, poison)
        ds, dd = to_device(sbuf), to_device(np.full(dl.total * osz, PATTERN, np.uint8))
        dptr = dd.data_ptr() + dl.lead * osz
        assert sl.ptr(ds) % 256 == sbuf.itemsize and dptr % 256 == osz
        gpu.resample_convert_device(rq, C, sl.ptr(ds), sstride, dptr, dstride, st, cv, stream=stream(), batch=B, src_image_stride=sl.image_stride,
                                    dst_image_stride=dl.image_stride, dst_plane_stride=dl.plane_stride)
        torch.cuda.synchronize()
        kernel = gpu.last_kernel()
        assert (kernel == kernel_name(st, ot)) if direct else kernel.endswith("+converted"), kernel
        after = to_numpy(dd, np.uint8)
        guard = np.repeat(~dl.entitled, osz)
        changed = np.flatnonzero((after != PATTERN) & guard)
        assert changed.size == 0, (name, sname, poison, (changed[:4] // osz - dl.lead).tolist())
        assert np.array_equal(to_numpy(ds, ic.NP[st]), sbuf)
        outs.append(after.view(cc.OUT_NP[ot])[dl.index].reshape((B, C, dH, dW) if lay == cc.PLANAR else (B, dH, dW, C)))
    assert same(outs[0], outs[1]), (name, sname, "the output depends on the padding")
    for b in range(B):
        assert same(np.ascontiguousarray(outs[0][b]), singles[b]), (name, sname, b)


# ---- stream order ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(gpu):
    """one scenario per route: the call between a delayed producer and a consumer on the caller's stream, no host wait (stream_order.py).
    u8 RGB in; direct: fp16 planar out, forwarding: fp32 interleaved out; the output buffer is held as 32-bit words."""
    import torch
    h = so.Harness(gpu)
    C = 3
    scale, offset = cc.conversion("normalise", ic.U8)
    for name, geom, route, ot, lay in (("direct", ic.GEOMETRIES["d"], "aai_axis_convert_kernel<u8,f16>", cc.F16, cc.PLANAR),
                                       ("forwarding", ROT, "+converted", cc.F32, cc.INTERLEAVED)):
        W, H = geom[:2]
        rq = _request(gpu, geom, "area")
        l = gpu.query(rq)[2]
        dW, dH = l.dst_width, l.dst_height
        cv = gpu.make_convert(C, ot, lay == cc.PLANAR, scale[:C], offset[:C])
        inp = torch.empty((H, W, C), dtype=torch.uint8, device="cuda")
        out = torch.empty(((dW * dH * C * OUT_BYTES[ot] + 3) // 4,), dtype=torch.int32, device="cuda")
        sc = so.Scenario(name, inp, out, so.rand_frames(torch, (H, W, C), 60, torch.uint8),
                         lambda handle, rq=rq, inp=inp, out=out, W=W, dW=dW, dH=dH, cv=cv, lay=lay: gpu.resample_convert_device(
                             rq, C, inp.data_ptr(), W * C, out.data_ptr(), dW if lay == cc.PLANAR else dW * C, ic.U8, cv, handle, dst_plane_stride=dW * dH),
                         poison=255)
        sc.rq, sc.lay = rq, l
        gpu.prepare(rq, C)
        h.add(sc)
        sc.kernel = gpu.last_kernel()
        assert route in sc.kernel, (name, sc.kernel)
    h.calibrate()
    return h


@pytest.mark.parametrize("name", ["direct", "forwarding"])
def test_convert_entry_keeps_stream_order(harness, name):
    import torch
    sc = harness.scenario(name)
    for caller in (so.Caller("torch's current stream", torch.cuda.current_stream()), so.Caller("a fresh stream", torch.cuda.Stream())):
        harness.frame_loop(sc, caller)


# ---- batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, geom, direct", [("direct", ic.GEOMETRIES["l"], True), ("forwarding", ROT, False)])
def test_a_batch_equals_singles(gpu, name, geom, direct):
    import torch
    B, C, st, ot = 3, 3, ic.U16, cc.BF16
    W, H = geom[:2]
    rq = _request(gpu, geom, "area")
    l = gpu.query(rq)[2]
    dW, dH = l.dst_width, l.dst_height
    scale, offset = cc.conversion("edge", st)
    images = np.stack([ic.source(geom, C, st, "random", seed=40 + b) for b in range(B)])
    for lay in (cc.INTERLEAVED, cc.PLANAR):
        cv = gpu.make_convert(C, ot, lay == cc.PLANAR, scale[:C], offset[:C])
        x = upload(images)
        y = upload(np.full((B, dH * dW * C), PATTERN, np.uint8).repeat(2))
        gpu.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW if lay == cc.PLANAR else dW * C, st, cv, stream=stream(), batch=B,
                                    src_image_stride=H * W * C, dst_image_stride=dH * dW * C, dst_plane_stride=dH * dW)
        torch.cuda.synchronize()
        assert (gpu.last_kernel() == kernel_name(st, ot)) if direct and cc.direct(rq, C, st, ot, lay) else gpu.last_kernel().endswith("+converted")
        got = y.cpu().numpy().view(np.uint16).reshape((B,) + cc.out_shape(dH, dW, C, lay))
        for b in range(B):
            assert same(np.ascontiguousarray(got[b]), run_convert(gpu, rq, st, images[b], scale, offset, ot, lay)), (name, lay, b)


def test_direct_route_batch_beyond_one_launch(gpu):
    """65535 + 3 images of 2 x 6 pixels of two u16 channels -- rows of exactly 4 elements -- into fp16 planar (3.1 MB in, 3.1 MB out): the
    engine splits the batch into two launches; the images on both sides of the split have the single call's bits"""
    import torch
    geom, C, st, ot, lay = ic.GEOMETRIES["n"], 2, ic.U16, cc.F16, cc.PLANAR
    W, H = geom[:2]
    B = 65535 + 3
    rq = _request(gpu, geom, "area")
    assert cc.facts(rq, C)[7] == 1 and W * C == 4
    l = gpu.query(rq)[2]
    dW, dH = l.dst_width, l.dst_height
    scale, offset = cc.conversion("normalise", st)
    cv = gpu.make_convert(C, ot, True, scale[:C], offset[:C])
    src = np.random.default_rng(9).integers(0, 65536, size=(B, H, W, C)).astype(np.uint16)
    x = upload(src)
    y = upload(np.full((B, C, dH, dW), PATTERN, np.uint8).repeat(2))
    gpu.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW, st, cv, stream=stream(), batch=B, src_image_stride=H * W * C,
                                dst_image_stride=C * dH * dW, dst_plane_stride=dH * dW)
    torch.cuda.synchronize()
    assert cc.direct(rq, C, st, ot, lay) and gpu.last_kernel() == kernel_name(st, ot), gpu.last_kernel()
    got = y.cpu().numpy().view(np.uint16).reshape(B, C, dH, dW)
    for b in (0, 1, 65534, 65535, 65536, B - 1):
        assert same(got[b], cc.replay(gpu, rq, st, src[b], scale, offset, ot, lay)[0]), b
    # every image at once: the images are independent, so a permutation of the batch permutes the results
    perm = np.random.default_rng(10).permutation(B)
    x2 = upload(src[perm])
    y2 = upload(np.full((B, C, dH, dW), PATTERN, np.uint8).repeat(2))
    gpu.resample_convert_device(rq, C, x2.data_ptr(), W * C, y2.data_ptr(), dW, st, cv, stream=stream(), batch=B, src_image_stride=H * W * C,
                                dst_image_stride=C * dH * dW, dst_plane_stride=dH * dW)
    torch.cuda.synchronize()
    assert np.array_equal(y2.cpu().numpy().view(np.uint16).reshape(B, C, dH, dW), got[perm])


# ---- the host entry, the empty batch, the late argument errors ---------------------------------------------------------------------
@pytest.mark.parametrize("name, geom", [("direct", ic.GEOMETRIES["e"]), ("forwarding", ROT)])
def test_host_entry_has_the_device_entrys_bits(gpu, name, geom):
    W, H, sr, dr, iso, ang = geom
    rq = _request(gpu, geom, "area")
    for st, ot, planar in ((ic.U8, cc.F16, True), (ic.U16, cc.F32, False), (ic.U8, cc.BF16, False), (ic.U16, cc.F32, True)):
        src = ic.source(geom, 3, st, "random", seed=11)
        scale, offset = cc.conversion("normalise", st)
        rc, msg, dst, dst_iso, l = gpu.resample_convert_host(src, sr, dr, iso, ang, out_type=ot, planar=planar, scale=scale[:3], offset=offset[:3])
        assert rc == 0, msg
        host_kernel = gpu.last_kernel()
        want = run_convert(gpu, rq, st, src, scale, offset, ot, cc.PLANAR if planar else cc.INTERLEAVED)
        assert host_kernel == gpu.last_kernel() and same(np.ascontiguousarray(dst).view(cc.OUT_NP[ot]), want), (name, st, ot, planar)
        assert (l.dst_width, l.dst_height) == ((want.shape[2], want.shape[1]) if planar else (want.shape[1], want.shape[0]))
    # a 2-D image is one channel
    rc, msg, dst, _, _ = gpu.resample_convert_host(ic.source(geom, 1, ic.U8, "random")[:, :, 0], sr, dr, iso, ang, out_type=cc.F16, scale=2.0, offset=-1.0)
    assert rc == 0 and dst.ndim == 2 and dst.dtype == np.float16


def test_an_empty_batch_touches_nothing_and_late_errors_are_reported(gpu):
    import torch
    geom, C, st = ic.GEOMETRIES["b"], 3, ic.U8
    W, H = geom[:2]
    rq = _request(gpu, geom, "area")
    l = gpu.query(rq)[2]
    dW, dH = l.dst_width, l.dst_height
    x = upload(ic.source(geom, C, st, "random"))
    y = upload(np.full((C, dH, dW), PATTERN, np.uint8).repeat(2))
    cv = gpu.make_convert(C, cc.F16, True)
    before = gpu.last_kernel()
    gpu.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW, st, cv, stream=stream(), batch=0, dst_plane_stride=dW * dH)
    gpu.resample_convert_device(rq, C, 0, 1, 0, 1, st, cv, stream=stream(), batch=0)      # (not even the pointers and strides are looked at)
    torch.cuda.synchronize()
    assert gpu.last_kernel() == before and bool((y == PATTERN).all())
    # behind the device check: the strides, the planar ones among them
    for kw, text in ((dict(src_stride=W * C - 1), "Source stride smaller than the image width."), (dict(dst_stride=dW - 1), "Destination stride smaller than the output width."),
                     (dict(dst_plane_stride=dW * dH - 1), "Destination plane stride smaller than one plane.")):
        a = dict(src_stride=W * C, dst_stride=dW, dst_plane_stride=dW * dH)
        a.update(kw)
        with pytest.raises(gpu.AaiError) as e:
            gpu.resample_convert_device(rq, C, x.data_ptr(), a["src_stride"], y.data_ptr(), a["dst_stride"], st, cv, stream=stream(), dst_plane_stride=a["dst_plane_stride"])
        assert text in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert bool((y == PATTERN).all())
    # an interleaved destination row is dW x C elements: dW alone is too short there
    with pytest.raises(gpu.AaiError):
        gpu.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW, st, gpu.make_convert(C, cc.F16, False), stream=stream())
