"""resample(..., half=..., half_backward=True) on the MI355X: the backward stays in the tensor's dtype (aai_adjoint_half_device on gy, its output
is x.grad), has the bits of the widening backward under planned_backward="any" / "channels_last", allocates no fp32 image, and refuses
what the operator documents."""
import pytest

import half_cases as hc

pytestmark = pytest.mark.gpu

ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)
DIRECT = [hc.CASES["a"], hc.CASES["a"][:5] + (90.0,), hc.CASES["e"]]


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return aai


def dtypes():
    import torch
    return ((torch.float16, "f16"), (torch.bfloat16, "bf16"))


def same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))


def watch_backward_kernel(gpu, leaf):
    """-> a list that receives aai.last_kernel() as the thread that ran the backward sees it (the text is per thread, and autograd runs the
    backward of a CUDA tensor on a thread of its own): a hook on the leaf runs there, right after the operator's backward"""
    seen = []
    leaf.register_hook(lambda grad: seen.append(gpu.last_kernel()))
    return seen


def _pair(gpu, x, geom, gen, **reference):
    """(x.grad with half_backward=True, the kernel after that backward, x.grad of the same call with `reference` instead, y of both equal?)"""
    import torch
    W, H, sr, dr, iso, ang = geom
    half = reference.pop("half")
    a = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    ya, _ = gpu.resample(a, sr, dr, iso, ang, half=half, half_backward=True)
    gy = (torch.rand(ya.shape, device="cuda", generator=gen) - 0.5).to(x.dtype)
    seen = watch_backward_kernel(gpu, a)
    ya.backward(gy)
    (kernel,) = seen
    b = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    yb, _ = gpu.resample(b, sr, dr, iso, ang, half=half, **reference)
    yb.backward(gy)
    torch.cuda.synchronize()
    assert same_bits(ya, yb) and ya.stride() == yb.stride()
    return a.grad, kernel, b.grad


@pytest.mark.parametrize("geom", DIRECT + [ROT], ids=["a", "a at 90", "e", "rotated"])
def test_planar_tensors_of_every_rank(gpu, geom):
    import torch
    W, H = geom[:2]
    gen = torch.Generator(device="cuda").manual_seed(11)
    for dtype, tname in dtypes():
        for shape in ((H, W), (2, H, W), (2, 3, H, W)):
            x = (torch.rand(shape, device="cuda", generator=gen) + 0.25).to(dtype)
            got, kernel, want = _pair(gpu, x, geom, gen, half=True, planned_backward="any")
            assert got.dtype == dtype and got.shape == x.shape and got.is_contiguous()
            assert same_bits(got, want), (tname, shape)
            assert kernel.endswith("+widened") if geom is ROT else kernel == "aai_axis_adjoint_half_kernel<%s,1>" % tname, kernel
        # a channels_last tensor under half=True is made contiguous: the planar route, B * C single-channel images
        x = (torch.rand((2, 3, H, W), device="cuda", generator=gen) + 0.25).to(dtype).contiguous(memory_format=torch.channels_last)
        got, kernel, want = _pair(gpu, x, geom, gen, half=True, planned_backward="any")
        assert same_bits(got, want) and ("<%s,1>" % tname in kernel or geom is ROT), kernel


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("geom", DIRECT + [ROT], ids=["a", "a at 90", "e", "rotated"])
def test_channels_last_tensors_go_as_interleaved_images(gpu, geom, C):
    import torch
    W, H = geom[:2]
    gen = torch.Generator(device="cuda").manual_seed(13)
    for dtype, tname in dtypes():
        x = (torch.rand((2, C, H, W), device="cuda", generator=gen) + 0.25).to(dtype).contiguous(memory_format=torch.channels_last)
        got, kernel, want = _pair(gpu, x, geom, gen, half="channels_last", planned_backward="channels_last")
        assert got.dtype == dtype and got.shape == x.shape
        assert got.is_contiguous(memory_format=torch.channels_last) and not got.is_contiguous()
        assert same_bits(got, want) and got.stride() == want.stride(), (tname, C)
        if geom is ROT:
            assert kernel.endswith("+widened"), kernel
        else:
            assert kernel == "aai_axis_adjoint_half_kernel<%s,%d>" % (tname, C), kernel
        # a contiguous tensor under half="channels_last" is exactly half=True: planar
        xc = x.contiguous()
        got, kernel, want = _pair(gpu, xc, geom, gen, half="channels_last", planned_backward="any")
        assert got.is_contiguous() and same_bits(got, want) and ("<%s,1>" % tname in kernel or geom is ROT), kernel


def test_backward_allocates_the_half_gradient_and_nothing_else(gpu):
    """Peak allocated memory around the backward at a direct geometry grows by no more than gx itself (4 MiB: 2048 x 1024 fp16) plus
    2 MiB -- the granularity of the caching allocator's large blocks (requests are rounded up to 512 bytes, and a cached block is handed
    out whole when what would be left of it is under 1 MiB), taken twice.  The three-step route allocates gy.float() (2 MiB), an fp32 gx
    (8 MiB) and the half gx (4 MiB) -- a peak of 12 MiB against 4 MiB when this was written: it is run beside for comparison and must
    NOT fit."""
    import torch
    W, H, sr, dr, iso, ang = 2048, 1024, 2, 1, (1023.5, 511.5), 180.0
    gx_bytes, allowance = W * H * 2, 2 << 20
    x = (torch.rand((H, W), device="cuda") + 0.25).to(torch.float16)
    growth = {}
    for name, kwargs in (("half_backward", dict(half_backward=True)), ("three steps", dict(planned_backward="any"))):
        a = x.detach().clone().requires_grad_(True)
        y, _ = gpu.resample(a, sr, dr, iso, ang, half=True, **kwargs)
        gy = torch.ones_like(y)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        seen = watch_backward_kernel(gpu, a)
        (gx,) = torch.autograd.grad(y, a, gy)
        torch.cuda.synchronize()
        growth[name] = torch.cuda.max_memory_allocated() - before
        assert gx.dtype == torch.float16
        if name == "half_backward":
            assert seen == ["aai_axis_adjoint_half_kernel<f16,1>"], seen
        del gx, y, a
    print("peak growth during backward: %s" % {k: "%.2f MiB" % (v / 2 ** 20) for k, v in growth.items()})
    assert growth["half_backward"] <= gx_bytes + allowance, growth
    assert growth["three steps"] > gx_bytes + allowance, growth


def test_refusals(gpu):
    import torch
    W, H, sr, dr, iso, ang = hc.CASES["a"]
    x = (torch.rand((H, W), device="cuda") + 0.25).to(torch.float16).requires_grad_(True)
    with pytest.raises(ValueError, match="half=True"):
        gpu.resample(x, sr, dr, iso, ang, half_backward=True)
    for planned in (True, "any", "channels_last"):
        with pytest.raises(ValueError, match="planned_backward"):
            gpu.resample(x, sr, dr, iso, ang, half=True, half_backward=True, planned_backward=planned)
    for mode in (gpu.MODE_BILINEAR, gpu.MODE_BICUBIC):
        with pytest.raises(ValueError, match="area and fast"):
            gpu.resample(x, sr, dr, iso, ang, mode, half=True, half_backward=True, sampler_backward=True)
    with pytest.raises(TypeError):
        gpu.resample(x.detach().float().requires_grad_(True), sr, dr, iso, ang, half=True, half_backward=True)
    with pytest.raises(RuntimeError):      # differentiable once
        y, _ = gpu.resample(x, sr, dr, iso, ang, half=True, half_backward=True)
        (gx,) = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)
        gx.sum().backward()
    # nothing existing changes: the default is off, and an empty batch returns without a launch
    empty, _ = gpu.resample(torch.empty((0, H, W), dtype=torch.float16, device="cuda"), sr, dr, iso, ang, half=True, half_backward=True)
    assert empty.shape == (0, 12, 16)


def test_unprepared_geometry_inside_a_capture_raises(gpu, monkeypatch):
    """with the current stream reported as capturing, a geometry whose single-channel plan has no adjoint tables raises in the forward
    instead of building them (which would synchronise); nothing is built"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 54, 46                                       # a geometry no other test prepares
    args = (2, 1, (26.5, 22.5), 90.0)
    rq = gpu.make_request(W, H, *args)
    x = (torch.rand((H, W), device="cuda") + 0.25).to(torch.bfloat16).requires_grad_(True)
    assert gpu.plan_shape(rq) == ""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        torch_ops.resample(x, *args, half=True, half_backward=True)
    assert gpu.plan_shape(rq) == ""
    gpu.prepare(rq)                                      # the forward's plan alone is not enough: the adjoint tables are missing
    assert "adjoint=none" in gpu.plan_shape(rq)
    with pytest.raises(RuntimeError, match="adjoint tables"):
        torch_ops.resample(x, *args, half=True, half_backward=True)
    assert "adjoint=none" in gpu.plan_shape(rq)
    monkeypatch.undo()
    y, _ = torch_ops.resample(x, *args, half=True, half_backward=True)
    assert "adjoint=tables" in gpu.plan_shape(rq)
    seen = watch_backward_kernel(gpu, x)
    y.backward(torch.ones_like(y))
    assert seen == ["aai_axis_adjoint_half_kernel<bf16,1>"] and x.grad.dtype == torch.bfloat16, seen
