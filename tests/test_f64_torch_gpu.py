"""torch_ops.resample(..., f64=True) on the MI355X: the reference-precision operator on float64 tensors.  Its forward and its gradient
are the device entries' bits (aai_resample_batch_device_f64 / aai_adjoint_batch_device_f64); it takes every shape and layout the fp32
operator takes; its forward and adjoint are autograd Functions that are each other's backward, so torch.autograd.gradcheck AND
gradgradcheck pass with torch's defaults -- which the fp32 operator cannot be asked, gradcheck needs float64; and it refuses what it
does not do."""
import pytest

from test_f64_host import wide_range

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


def _geo(W, H, sr=3.0, dr=1.0, ang=17.5):
    return sr, dr, ((W - 1) / 2, (H - 1) / 2), ang


def _entries(gpu, x, gy, geo, mode):
    """(W x, W^T gy) through the device entries on contiguous (B, H, W) / (B, dH, dW) float64 tensors"""
    import torch
    B, H, W = x.shape
    rq = gpu.make_request(W, H, *geo, mode=mode)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    y = torch.full((B, dH, dW), -1.0, dtype=torch.float64, device="cuda")
    gx = torch.full((B, H, W), -1.0, dtype=torch.float64, device="cuda")
    gpu.resample_device_f64(rq, x.data_ptr(), W, y.data_ptr(), dW, st, batch=B, src_image_stride=W * H, dst_image_stride=dW * dH)
    gpu.adjoint_device_f64(rq, gy.data_ptr(), dW, gx.data_ptr(), W, st, batch=B, dst_image_stride=dW * dH, src_image_stride=W * H)
    torch.cuda.synchronize()
    return y, gx


def _same(torch, a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


@pytest.mark.parametrize("mode_name", ["area", "fast"])
def test_forward_and_gradient_are_the_device_entries_bits_in_every_shape(gpu, mode_name):
    import torch
    from area_average_interpolation_amd.torch_ops import resample
    mode = gpu.MODE_FAST if mode_name == "fast" else gpu.MODE_AREA
    B, C, H, W = 2, 3, 29, 37
    geo = _geo(W, H)
    base = torch.from_numpy(wide_range((B, C, H, W), 71)).cuda()
    planes = base.view(B * C, H, W)
    lay = gpu.query(gpu.make_request(W, H, *geo, mode=mode))[2]
    gy = torch.from_numpy(wide_range((B * C, lay.dst_height, lay.dst_width), 72)).cuda()
    y_ref, gx_ref = _entries(gpu, planes, gy, geo, mode)
    wide = torch.from_numpy(wide_range((B, C, H, 2 * W), 73)).cuda()
    wide[..., ::2] = base
    cases = {
        "(H, W)": (base[0, 0].clone(), y_ref[0], gy[0], gx_ref[0]),
        "(B, H, W)": (planes.clone(), y_ref, gy, gx_ref),
        "(B, C, H, W)": (base.clone(), y_ref.view(B, C, *y_ref.shape[1:]), gy.view(B, C, *gy.shape[1:]), gx_ref.view(B, C, H, W)),
        "channels_last": (base.clone().contiguous(memory_format=torch.channels_last), y_ref.view(B, C, *y_ref.shape[1:]), gy.view(B, C, *gy.shape[1:]),
                          gx_ref.view(B, C, H, W)),
        "non-contiguous": (wide[..., ::2], y_ref.view(B, C, *y_ref.shape[1:]), gy.view(B, C, *gy.shape[1:]), gx_ref.view(B, C, H, W)),
    }
    assert not cases["non-contiguous"][0].is_contiguous() and not cases["channels_last"][0].is_contiguous()
    for name, (x, y_want, g, gx_want) in cases.items():
        x = x.detach().requires_grad_(True)
        y, iso = resample(x, *geo, mode=mode, f64=True)
        assert y.dtype == torch.float64 and iso == (lay.dst_iso_x, lay.dst_iso_y), name
        assert "aai_f64_forward_kernel" in gpu.last_kernel(), name
        assert _same(torch, y, y_want), name
        y.backward(g)                  # (autograd's thread: aai_last_kernel() is per thread, the bits below say which kernel ran)
        assert x.grad.dtype == torch.float64 and _same(torch, x.grad, gx_want), name
        # the options of the fp32 operator's backward are not consulted
        y2, _ = resample(x.detach(), *geo, mode, 0, "any", sampler_backward=True, f64=True)
        assert _same(torch, y2, y_want), name


def test_gradients_accumulate_and_a_side_stream_works(gpu):
    import torch
    from area_average_interpolation_amd.torch_ops import resample
    H, W = 29, 37
    geo = _geo(W, H)
    x = torch.from_numpy(wide_range((2, H, W), 81)).cuda().requires_grad_(True)
    lay = gpu.query(gpu.make_request(W, H, *geo))[2]
    g1, g2 = [torch.from_numpy(wide_range((2, lay.dst_height, lay.dst_width), s)).cuda() for s in (82, 83)]
    _, gx1 = _entries(gpu, x.detach(), g1, geo, gpu.MODE_AREA)
    y_ref, gx2 = _entries(gpu, x.detach(), g2, geo, gpu.MODE_AREA)
    resample(x, *geo, f64=True)[0].backward(g1)
    resample(x, *geo, f64=True)[0].backward(g2)
    assert _same(torch, x.grad, gx1 + gx2)
    # a side stream: producer, operator, backward and consumer on it, ordered by the stream alone
    side = torch.cuda.Stream()
    x2 = x.detach().clone().requires_grad_(True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y, _ = resample(x2, *geo, f64=True)
        y.backward(g2)
        y_copy, g_copy = y.detach().clone(), x2.grad.clone()
    side.synchronize()
    assert _same(torch, y_copy, y_ref) and _same(torch, g_copy, gx2)


@pytest.mark.parametrize("mode_name", ["area", "fast"])
@pytest.mark.parametrize("geometry", [(12, 10, 2.0, 1.0, 30.0), (8, 6, 1.0, 2.0, 117.5)], ids=["12x10 2:1 at 30", "8x6 1:2 at 117.5"])
def test_gradcheck_and_gradgradcheck_pass_with_torch_defaults(gpu, geometry, mode_name):
    import torch
    from area_average_interpolation_amd.torch_ops import resample
    W, H, sr, dr, ang = geometry
    mode = gpu.MODE_FAST if mode_name == "fast" else gpu.MODE_AREA
    geo = _geo(W, H, sr, dr, ang)
    x = torch.randn((H, W), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)).requires_grad_(True)
    fn = lambda t: resample(t, *geo, mode=mode, f64=True)[0]
    assert torch.autograd.gradcheck(fn, (x,))
    assert torch.autograd.gradgradcheck(fn, (x,))
    xb = torch.randn((2, H, W), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(10)).requires_grad_(True)
    assert torch.autograd.gradcheck(fn, (xb,))


def test_refusals_and_empty_batches(gpu):
    import torch
    from area_average_interpolation_amd.torch_ops import resample
    geo = _geo(16, 12)
    x64 = torch.zeros((12, 16), dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError):
        resample(x64.float(), *geo, f64=True)                  # float32 with f64=True
    with pytest.raises(TypeError):
        resample(x64, *geo)                                    # float64 without f64=True: as before
    with pytest.raises(TypeError):
        resample([[0.0]], *geo, f64=True)                       # not a tensor
    for mode in (gpu.MODE_BILINEAR, gpu.MODE_BICUBIC):
        with pytest.raises(ValueError):
            resample(x64, *geo, mode=mode, f64=True)           # up front, without requires_grad
    with pytest.raises(ValueError):
        resample(x64.cpu(), *geo, f64=True)
    with pytest.raises(ValueError):
        resample(x64.view(1, 1, 1, 12, 16), *geo, f64=True)
    with pytest.raises(gpu.AaiError):
        resample(x64, (1.0, 2.0), 1.0, (0, 0), 0.0, f64=True)
    lay = gpu.query(gpu.make_request(16, 12, *geo))[2]
    before = gpu.last_kernel()
    for shape in ((0, 12, 16), (0, 3, 12, 16), (2, 0, 12, 16)):
        x = torch.zeros(shape, dtype=torch.float64, device="cuda", requires_grad=True)
        y, iso = resample(x, *geo, f64=True)
        assert y.dtype == torch.float64 and tuple(y.shape) == shape[:-2] + (lay.dst_height, lay.dst_width) and y.numel() == 0
        assert iso == (lay.dst_iso_x, lay.dst_iso_y)
    assert gpu.last_kernel() == before                          # no launch
