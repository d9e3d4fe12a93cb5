"""resample(x, ..., integer=True, out_dtype=...) on the MI355X: dtype, memory format, no grad, no copy, and the C entry's values."""
import numpy as np
import pytest

import convert_cases as cc
import int_cases as ic

pytestmark = pytest.mark.gpu

DIRECT = ic.GEOMETRIES["e"]                       # 180 degrees, 140 outputs per strip
FORWARDED = (96, 80, 3, 1, (47.5, 39.5), 17.5)


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    aai.set_device(0)
    return aai


def _torch_dtype(torch, ot):
    return {cc.F32: torch.float32, cc.F16: torch.float16, cc.BF16: torch.bfloat16}[ot]


def _bits(t):
    """a tensor's elements in its logical (B, C, H, W) order as raw integers"""
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _c_entry(gpu, geom, images, st, scale, offset, ot):
    """[B, H, W, C] -> the C entry's planar output per image as raw integers [B, C, dH, dW] (interleaved and planar hold the same elements:
    tests/test_convert_gpu.py)"""
    import torch
    B, H, W, C = images.shape
    rq = ic.request(gpu, geom, "area")
    l = gpu.query(rq)[2]
    dH, dW = l.dst_height, l.dst_width
    x = torch.from_numpy(images.reshape(-1).view(np.uint8).copy()).cuda()
    y = torch.zeros((B, C, dH, dW), dtype=_torch_dtype(torch, ot), device="cuda")
    cv = gpu.make_convert(C, ot, True, scale[:C], offset[:C])
    gpu.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW, st, cv, stream=torch.cuda.current_stream().cuda_stream, batch=B,
                                src_image_stride=H * W * C, dst_image_stride=C * dH * dW, dst_plane_stride=dH * dW)
    torch.cuda.synchronize()
    return _bits(y), gpu.last_kernel()


@pytest.mark.parametrize("route, geom", [("direct", DIRECT), ("forwarding", FORWARDED)])
@pytest.mark.parametrize("ot, oname", cc.OUT_TYPES, ids=[t[1] for t in cc.OUT_TYPES])
def test_operator_writes_the_c_entrys_values_in_place(gpu, route, geom, ot, oname):
    import torch
    B, C, st = 2, 3, ic.U8
    W, H, sr, dr, iso, ang = geom
    images = np.stack([ic.source(geom, C, st, "random", seed=50 + b) for b in range(B)])
    scale, offset = cc.conversion("normalise", st)
    want, kernel = _c_entry(gpu, geom, images, st, scale, offset, ot)
    assert ("aai_axis_convert_kernel" in kernel) == (route == "direct" and cc.direct(ic.request(gpu, geom, "area"), C, st, ot, cc.PLANAR)), kernel
    nhwc = torch.from_numpy(images).cuda()                                   # [B, H, W, C] storage
    sources = {"channels_last": nhwc.permute(0, 3, 1, 2), "contiguous": nhwc.permute(0, 3, 1, 2).contiguous()}
    assert sources["channels_last"].is_contiguous(memory_format=torch.channels_last) and not sources["channels_last"].is_contiguous()
    for sname, x in sources.items():
        for fmt in (torch.contiguous_format, torch.channels_last):
            before = x.clone()
            ptr = x.data_ptr()
            y, yiso = gpu.resample(x, sr, dr, iso, ang, integer=True, out_dtype=_torch_dtype(torch, ot), scale=[float(v) for v in scale[:C]],
                                   offset=[float(v) for v in offset[:C]], out_memory_format=fmt)
            torch.cuda.synchronize()
            tag = (route, oname, sname, fmt)
            assert y.dtype == _torch_dtype(torch, ot) and tuple(y.shape) == want.shape and not y.requires_grad and y.grad_fn is None, tag
            assert y.is_contiguous(memory_format=fmt), tag
            assert x.data_ptr() == ptr and torch.equal(x, before), tag
            assert np.array_equal(_bits(y), want), tag
            # the tensor returned IS the buffer the library wrote: its storage starts at its first element and holds exactly the output
            assert y.storage_offset() == 0 and y.untyped_storage().nbytes() == y.numel() * y.element_size(), tag
            assert y.untyped_storage().data_ptr() == y.data_ptr(), tag
    # single-channel forms: (H, W) and (B, H, W), a scalar scale and offset
    one = torch.from_numpy(np.ascontiguousarray(images[:, :, :, 0])).cuda()
    y3, _ = gpu.resample(one, sr, dr, iso, ang, integer=True, out_dtype=_torch_dtype(torch, ot), scale=float(scale[0]), offset=float(offset[0]))
    y2, _ = gpu.resample(one[1], sr, dr, iso, ang, integer=True, out_dtype=_torch_dtype(torch, ot), scale=float(scale[0]), offset=float(offset[0]))
    torch.cuda.synchronize()
    assert tuple(y3.shape) == (B,) + want.shape[2:] and np.array_equal(_bits(y3), want[:, 0]) and np.array_equal(_bits(y2), want[1, 0])


def test_operator_refusals_and_defaults(gpu):
    import torch
    geom = DIRECT
    W, H, sr, dr, iso, ang = geom
    x = torch.from_numpy(ic.source(geom, 3, ic.U8, "random")[None]).cuda().permute(0, 3, 1, 2)
    # the defaults: scale 1, offset 0 -- in float32 the sums themselves, which the integer operator rounds to its elements
    y, _ = gpu.resample(x, sr, dr, iso, ang, integer=True, out_dtype=torch.float32)
    q, _ = gpu.resample(x, sr, dr, iso, ang, integer=True)
    torch.cuda.synchronize()
    assert q.dtype == torch.uint8 and y.dtype == torch.float32 and y.is_contiguous()
    assert int((torch.round(y).clamp(0, 255).to(torch.int32) - q.to(torch.int32)).abs().max()) <= 1
    with pytest.raises(ValueError):
        gpu.resample(x, sr, dr, iso, ang, out_dtype=torch.float16)
    for extra in (dict(half=True), dict(f64=True), dict(planned_backward=True), dict(sampler_backward=True)):
        with pytest.raises(ValueError):
            gpu.resample(x, sr, dr, iso, ang, integer=True, out_dtype=torch.float16, **extra)
    with pytest.raises(RuntimeError, match="finite"):
        gpu.resample(x, sr, dr, iso, ang, integer=True, out_dtype=torch.float16, scale=(1.0, float("inf"), 1.0))
    # an empty batch returns an empty tensor of the output's shape without a launch
    before = gpu.last_kernel()
    e, _ = gpu.resample(x[:0], sr, dr, iso, ang, integer=True, out_dtype=torch.bfloat16, out_memory_format=torch.channels_last)
    assert tuple(e.shape) == (0, 3) + tuple(y.shape[2:]) and e.dtype == torch.bfloat16 and gpu.last_kernel() == before
