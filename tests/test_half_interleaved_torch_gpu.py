"""resample(..., half="channels_last") on the MI355X: a channels_last float16 / bfloat16 (B, C, H, W) tensor with 2 <= C <= 4 is read in
place by aai_resample_half_interleaved_device and comes back channels_last with that entry's bits; every other input takes exactly the
half=True path; the backward is the fp32 operator's backward for a channels_last tensor on the widened gradient, rounded once."""
import numpy as np
import pytest

import half_cases as hc

pytestmark = pytest.mark.gpu

ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)
CL = "channels_last"


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return aai


def dtypes():
    import torch
    return ((torch.float16, hc.F16), (torch.bfloat16, hc.BF16))


def same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))


def is_channels_last(t):
    import torch
    return t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def c_entry(gpu, x_nhwc, geom, mode):
    """aai_resample_half_interleaved_device on a dense (B, H, W, C) half tensor -> (B, dH, dW, C)"""
    import torch
    W, H, sr, dr, iso, ang = geom
    B, _, _, C = x_nhwc.shape
    rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
    lay = gpu.query(rq)[2]
    dH, dW = lay.dst_height, lay.dst_width
    y = torch.full((B, dH, dW, C), float("nan"), dtype=x_nhwc.dtype, device="cuda")
    gpu.resample_half_interleaved_device(rq, C, x_nhwc.data_ptr(), W * C, y.data_ptr(), dW * C, dict(dtypes())[x_nhwc.dtype],
                                         stream=torch.cuda.current_stream().cuda_stream, batch=B, src_image_stride=H * W * C, dst_image_stride=dH * dW * C)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("geom", [hc.CASES["a"], hc.CASES["e"], ROT], ids=["direct", "direct at 180", "forwarding"])
def test_channels_last_tensor_is_read_in_place(gpu, geom):
    import torch
    W, H, sr, dr, iso, ang = geom
    gen = torch.Generator(device="cuda").manual_seed(7)
    for dtype, ht in dtypes():
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            x = (torch.rand((2, 3, H, W), device="cuda", generator=gen) + 0.25).to(dtype).contiguous(memory_format=torch.channels_last)
            assert is_channels_last(x)
            want = c_entry(gpu, x.permute(0, 2, 3, 1), geom, mode)            # (the permuted view IS the dense NHWC storage)
            assert x.permute(0, 2, 3, 1).is_contiguous()
            y, iso_out = gpu.resample(x, sr, dr, iso, ang, mode, half=CL)
            kernel = gpu.last_kernel()
            assert y.dtype == dtype and y.shape == (2, 3) + tuple(want.shape[1:3]) and is_channels_last(y)
            assert same_bits(y.permute(0, 2, 3, 1), want), (dtype, mode)
            lay = gpu.query(gpu.make_request(W, H, sr, dr, iso, ang, mode=mode))[2]
            assert iso_out == (lay.dst_iso_x, lay.dst_iso_y)
            # the half=True detour on the same tensor copies, comes back contiguous and is within one unit of these bits, not equal by
            # contract (test_the_entry_reads_the_tensors_own_storage holds the zero-copy claim on poisoned storage)
            planar, _ = gpu.resample(x, sr, dr, iso, ang, mode, half=True)
            assert planar.is_contiguous() and not is_channels_last(planar)
            ulps = hc.ulp_distance(planar.view(torch.int16).cpu().numpy().view(np.uint16), y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16))
            assert int(ulps.max()) <= 1
            if ang != 17.5:
                assert kernel == "aai_axis_half_kernel<%s>" % ("f16" if ht == hc.F16 else "bf16"), kernel
            else:
                assert kernel.endswith("+widened"), kernel


def test_the_entry_reads_the_tensors_own_storage(gpu):
    """the storage of x is poisoned except where x itself lives: x is a channels_last VIEW into a larger NHWC buffer of NaN (one image of
    padding before and behind); the result is finite and has the C entry's bits on exactly that storage"""
    import torch
    W, H, sr, dr, iso, ang = hc.CASES["b"]
    for dtype, ht in dtypes():
        buf = torch.full((4, H, W, 3), float("nan"), dtype=dtype, device="cuda")
        buf[1:3] = (torch.rand((2, H, W, 3), device="cuda") + 0.25).to(dtype)
        x = buf[1:3].permute(0, 3, 1, 2)
        assert is_channels_last(x) and x.data_ptr() == buf[1].data_ptr()
        y, _ = gpu.resample(x, sr, dr, iso, ang, half=CL)
        assert is_channels_last(y) and bool(torch.isfinite(y.float()).all())
        assert same_bits(y.permute(0, 2, 3, 1), c_entry(gpu, buf[1:3], hc.CASES["b"], gpu.MODE_AREA))


@pytest.mark.parametrize("geom", [hc.CASES["a"], ROT], ids=["direct", "forwarding"])
def test_every_other_input_takes_the_half_true_path(gpu, geom):
    import torch
    W, H, sr, dr, iso, ang = geom
    gen = torch.Generator(device="cuda").manual_seed(9)
    for dtype, ht in dtypes():
        inputs = {
            "C = 1, channels_last": (torch.rand((2, 1, H, W), device="cuda", generator=gen) + 0.25).to(dtype).contiguous(memory_format=torch.channels_last),
            "C = 5, channels_last": (torch.rand((1, 5, H, W), device="cuda", generator=gen) + 0.25).to(dtype).contiguous(memory_format=torch.channels_last),
            "C = 3, contiguous": (torch.rand((2, 3, H, W), device="cuda", generator=gen) + 0.25).to(dtype),
            "3-D": (torch.rand((2, H, W), device="cuda", generator=gen) + 0.25).to(dtype),
            "2-D": (torch.rand((H, W), device="cuda", generator=gen) + 0.25).to(dtype),
        }
        for name, x in inputs.items():
            y, _ = gpu.resample(x, sr, dr, iso, ang, half=CL)
            want, _ = gpu.resample(x, sr, dr, iso, ang, half=True)
            assert same_bits(y, want) and y.stride() == want.stride() and y.is_contiguous(), (name, dtype)
    empty, _ = gpu.resample(torch.empty((0, 3, H, W), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last), sr, dr, iso, ang, half=CL)
    assert empty.shape[:2] == (0, 3) and empty.dtype == torch.float16
    with pytest.raises(TypeError):
        gpu.resample(torch.ones((2, 3, H, W), dtype=torch.float32, device="cuda").contiguous(memory_format=torch.channels_last), sr, dr, iso, ang, half=CL)
    # a string that is not "channels_last" is refused, not read as half=True
    xcl = torch.ones((2, 3, H, W), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
    for bad in ("channel_last", "Channels_Last", "true", ""):
        with pytest.raises(ValueError, match="half must be"):
            gpu.resample(xcl, sr, dr, iso, ang, half=bad)


BACKWARD = [("general", hc.CASES["a"], False), ("general, rotated", ROT, False), ("interleaved, rotated", ROT, "interleaved"),
            ("interleaved, separable", hc.CASES["a"], "interleaved"), ("channels_last, separable", hc.CASES["a"], CL), ("channels_last, rotated", ROT, CL),
            ("planned, separable", hc.CASES["a"], True), ("any, rotated", ROT, "any")]


@pytest.mark.parametrize("name, geom, planned", BACKWARD, ids=[b[0] for b in BACKWARD])
def test_gradient_is_the_fp32_channels_last_gradient_rounded_once(gpu, name, geom, planned):
    """x.grad is channels_last in x's dtype and equals round(the gradient of the fp32 operator on the widened channels_last x under the
    widened gy and the same planned_backward): "interleaved" and "channels_last" keep their meaning, they do not collapse to "any" """
    import torch
    W, H, sr, dr, iso, ang = geom
    gen = torch.Generator(device="cuda").manual_seed(11)
    for dtype, ht in dtypes():
        x = (torch.rand((2, 3, H, W), device="cuda", generator=gen) + 0.25).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y, _ = gpu.resample(x, sr, dr, iso, ang, half=CL, planned_backward=planned)
        assert is_channels_last(y)
        gy = (torch.rand(y.shape, device="cuda", generator=gen) - 0.5).to(dtype).contiguous(memory_format=torch.channels_last)
        y.backward(gy)
        assert x.grad.dtype == dtype and x.grad.shape == x.shape and is_channels_last(x.grad)
        x32 = x.detach().float().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        assert is_channels_last(x32)
        y32, _ = gpu.resample(x32, sr, dr, iso, ang, planned_backward=planned)
        y32.backward(gy.float())
        assert same_bits(x.grad, x32.grad.to(dtype)), (name, dtype)
        with pytest.raises(RuntimeError):      # differentiable once
            x2 = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
            y2, _ = gpu.resample(x2, sr, dr, iso, ang, half=CL)
            (gx,) = torch.autograd.grad(y2, x2, gy, create_graph=True)
            gx.sum().backward()


def test_sampler_backward(gpu):
    import torch
    W, H = 96, 80
    args = (2, 1, (47.5, 39.5), 30.0, gpu.MODE_BILINEAR)
    x = (torch.rand((2, 3, H, W), device="cuda") + 0.25).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with pytest.raises(ValueError):
        gpu.resample(x, *args, half=CL)
    y, _ = gpu.resample(x, *args, half=CL, sampler_backward=True)
    assert gpu.last_kernel().endswith("+widened") and is_channels_last(y)
    gy = (torch.rand(y.shape, device="cuda") - 0.5).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y.backward(gy)
    x32 = x.detach().float().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y32, _ = gpu.resample(x32, *args, sampler_backward=True)
    y32.backward(gy.float())
    assert is_channels_last(x.grad) and x.grad.dtype == torch.bfloat16
    assert same_bits(y, y32.to(torch.bfloat16)) and same_bits(x.grad, x32.grad.to(torch.bfloat16))
