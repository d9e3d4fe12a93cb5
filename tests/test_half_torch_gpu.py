"""resample(..., half=True) on the MI355X: float16 / bfloat16 tensors of every rank with the bits of resample_half_device, the backward as
the fp32 adjoint of the widened gradient rounded once, and what the operator refuses."""
import numpy as np
import pytest

import half_cases as hc

pytestmark = pytest.mark.gpu

ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return aai


def dtypes():
    import torch
    return ((torch.float16, hc.F16), (torch.bfloat16, hc.BF16))


def device_entry(gpu, x3, geom, mode):
    """resample_half_device on a contiguous (B, H, W) half tensor"""
    import torch
    W, H, sr, dr, iso, ang = geom
    rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
    lay = gpu.query(rq)[2]
    B = x3.shape[0]
    y = torch.full((B, lay.dst_height, lay.dst_width), float("nan"), dtype=x3.dtype, device="cuda")
    gpu.resample_half_device(rq, x3.data_ptr(), W, y.data_ptr(), lay.dst_width, dict(dtypes())[x3.dtype], stream=torch.cuda.current_stream().cuda_stream,
                             batch=B, src_image_stride=H * W, dst_image_stride=lay.dst_height * lay.dst_width)
    torch.cuda.synchronize()
    return y


def same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))


@pytest.mark.parametrize("geom", [hc.CASES["a"], ROT], ids=["direct", "forwarding"])
def test_values_and_shapes(gpu, geom):
    import torch
    W, H, sr, dr, iso, ang = geom
    gen = torch.Generator(device="cuda").manual_seed(7)
    for dtype, ht in dtypes():
        x4 = (torch.rand((2, 3, H, W), device="cuda", generator=gen) + 0.25).to(dtype)
        want = device_entry(gpu, x4.view(6, H, W), geom, gpu.MODE_AREA)
        dH, dW = want.shape[1:]
        y4, iso_out = gpu.resample(x4, sr, dr, iso, ang, half=True)
        assert y4.dtype == dtype and y4.shape == (2, 3, dH, dW) and y4.is_contiguous() and same_bits(y4, want.view(2, 3, dH, dW))
        assert iso_out == tuple(gpu.query(gpu.make_request(W, H, sr, dr, iso, ang))[2].__getattribute__(k) for k in ("dst_iso_x", "dst_iso_y"))
        y3, _ = gpu.resample(x4[0], sr, dr, iso, ang, half=True)
        assert y3.dtype == dtype and same_bits(y3, want[:3])
        y2, _ = gpu.resample(x4[1, 2], sr, dr, iso, ang, half=True)
        assert y2.dtype == dtype and y2.shape == (dH, dW) and same_bits(y2, want[5])
        # channels_last storage: made contiguous, the planar route's bits
        ycl, _ = gpu.resample(x4.contiguous(memory_format=torch.channels_last), sr, dr, iso, ang, half=True)
        assert ycl.is_contiguous() and same_bits(ycl, y4)
        yf, _ = gpu.resample(x4, sr, dr, iso, ang, gpu.MODE_FAST, half=True)
        assert same_bits(yf, device_entry(gpu, x4.view(6, H, W), geom, gpu.MODE_FAST).view(2, 3, dH, dW))


@pytest.mark.parametrize("planned", [False, True, "any"], ids=["general", "planned", "any"])
@pytest.mark.parametrize("geom", [hc.CASES["a"], ROT], ids=["direct", "forwarding"])
def test_gradient_is_the_fp32_adjoint_rounded_once(gpu, geom, planned):
    import torch
    W, H, sr, dr, iso, ang = geom
    rq = gpu.make_request(W, H, sr, dr, iso, ang)
    gen = torch.Generator(device="cuda").manual_seed(11)
    for dtype, ht in dtypes():
        x = (torch.rand((2, H, W), device="cuda", generator=gen) + 0.25).to(dtype).requires_grad_(True)
        y, _ = gpu.resample(x, sr, dr, iso, ang, half=True, planned_backward=planned)
        gy = (torch.rand(y.shape, device="cuda", generator=gen) - 0.5).to(dtype)
        y.backward(gy)
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        g32 = gy.float().contiguous()
        want = torch.full((2, H, W), float("nan"), dtype=torch.float32, device="cuda")
        dH, dW = y.shape[1:]
        gpu.adjoint_device(rq, g32.data_ptr(), dW, want.data_ptr(), W, stream=torch.cuda.current_stream().cuda_stream, batch=2,
                           dst_image_stride=dH * dW, src_image_stride=H * W, planned=planned)
        torch.cuda.synchronize()
        assert same_bits(x.grad, want.to(dtype)), (dtype, planned)
        # ... which is the gradient of the fp32 operator on the widened tensors, rounded
        x32 = x.detach().float().requires_grad_(True)
        y32, _ = gpu.resample(x32, sr, dr, iso, ang, planned_backward=planned)
        y32.backward(g32)
        assert same_bits(x.grad, x32.grad.to(dtype))
        with pytest.raises(RuntimeError):      # differentiable once
            x2 = x.detach().clone().requires_grad_(True)
            y2, _ = gpu.resample(x2, sr, dr, iso, ang, half=True)
            (gx,) = torch.autograd.grad(y2, x2, gy, create_graph=True)
            gx.sum().backward()


def test_sampler_backward(gpu):
    import torch
    W, H = 96, 80
    x = (torch.rand((1, H, W), device="cuda") + 0.25).to(torch.bfloat16).requires_grad_(True)
    with pytest.raises(ValueError):
        gpu.resample(x, 2, 1, (47.5, 39.5), 30.0, gpu.MODE_BILINEAR, half=True)
    y, _ = gpu.resample(x, 2, 1, (47.5, 39.5), 30.0, gpu.MODE_BILINEAR, half=True, sampler_backward=True)
    assert gpu.last_kernel().endswith("+widened")
    gy = torch.ones_like(y)
    y.backward(gy)
    x32 = x.detach().float().requires_grad_(True)
    y32, _ = gpu.resample(x32, 2, 1, (47.5, 39.5), 30.0, gpu.MODE_BILINEAR, sampler_backward=True)
    y32.backward(gy.float())
    assert same_bits(y, y32.to(torch.bfloat16)) and same_bits(x.grad, x32.grad.to(torch.bfloat16))


def test_refusals_and_edge_cases(gpu):
    import torch
    W, H, sr, dr, iso, ang = hc.CASES["a"]
    for dtype, ht in dtypes():
        xh = torch.ones((H, W), dtype=dtype, device="cuda")
        with pytest.raises(TypeError):
            gpu.resample(xh, sr, dr, iso, ang)                      # half=False: nothing changes
        with pytest.raises(ValueError):
            gpu.resample(xh.cpu(), sr, dr, iso, ang, half=True)
        empty, _ = gpu.resample(torch.empty((0, H, W), dtype=dtype, device="cuda"), sr, dr, iso, ang, half=True)
        assert empty.dtype == dtype and empty.shape == (0, 12, 16)
        empty4, _ = gpu.resample(torch.empty((2, 0, H, W), dtype=dtype, device="cuda"), sr, dr, iso, ang, half=True)
        assert empty4.dtype == dtype and empty4.shape == (2, 0, 12, 16)
    with pytest.raises(TypeError):
        gpu.resample(torch.ones((H, W), dtype=torch.float32, device="cuda"), sr, dr, iso, ang, half=True)
    with pytest.raises(TypeError):
        gpu.resample(torch.ones((H, W), dtype=torch.float64, device="cuda"), sr, dr, iso, ang, half=True)
    with pytest.raises(ValueError):
        gpu.resample(torch.ones((W,), dtype=torch.float16, device="cuda"), sr, dr, iso, ang, half=True)


def test_unprepared_geometry_inside_a_capture_raises(gpu, monkeypatch):
    """with the current stream reported as capturing, a geometry without a plan raises instead of building one (which would
    synchronise); prepared outside the capture, the direct route is recorded into a graph and replays"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 52, 44                                       # a geometry no other test prepares
    args = (2, 1, (25.5, 21.5), 0.0)
    rq = gpu.make_request(W, H, *args)
    x = (torch.rand((H, W), device="cuda") + 0.25).to(torch.float16)
    assert gpu.plan_shape(rq) == ""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        torch_ops.resample(x, *args, half=True)
    assert gpu.plan_shape(rq) == ""
    monkeypatch.undo()
    eager, _ = torch_ops.resample(x, *args, half=True)
    assert gpu.last_kernel().startswith("aai_axis_half_kernel") and gpu.plan_shape(rq) != ""
    torch.cuda.synchronize()
    lay = gpu.query(rq)[2]
    out = torch.zeros((lay.dst_height, lay.dst_width), dtype=torch.float16, device="cuda")
    graph, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=cs):
        gpu.resample_half_device(rq, x.data_ptr(), W, out.data_ptr(), lay.dst_width, gpu.HALF_F16, torch.cuda.current_stream().cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager)
