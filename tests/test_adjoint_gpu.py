"""The adjoint (transposed) resampling on the MI355X: gsrc = W^T gdst against the oracle's matrix (small and knife-edge
geometries), the adjoint identity <W x, y> = <x, W^T y> against the shipped forward at size, determinism, batches with padded
strides, and the differentiable torch operator."""
import numpy as np
import pytest

from conftest import TOL
from test_adjoint_host import EIGHT, adjoint_gold, assert_adjoint_matches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


def _adjoint(gpu, rq, g):
    """aai_adjoint_batch_device_f32 on a host gradient image; gsrc prefilled with -1"""
    import torch
    gd = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
    gs = torch.full((rq.src_height, rq.src_width), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), gd.shape[1], gs.data_ptr(), rq.src_width, torch.cuda.current_stream().cuda_stream, batch=1)
    torch.cuda.synchronize()
    assert "aai_adjoint_gather_kernel" in gpu.last_kernel()
    return gs.cpu().numpy()


def _check_case(gpu, po, W, H, sr, dr, iso, ang, mode, policy, what):
    g, gold = adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, mode, policy)
    got = _adjoint(gpu, gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy), g)
    assert_adjoint_matches(got, gold, what)


@pytest.mark.parametrize("case", range(len(EIGHT)))
def test_adjoint_matches_the_oracle_matrix(gpu, po, case):
    W, H, sr, dr, ang, off = EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mode, policy in ((gpu.MODE_AREA, gpu.POLICY_REFERENCE), (gpu.MODE_AREA, gpu.POLICY_EXACT), (gpu.MODE_FAST, gpu.POLICY_REFERENCE)):
        _check_case(gpu, po, W, H, sr, dr, iso, ang, mode, policy, "case %d mode %d policy %d" % (case, mode, policy))
    # the host-buffer entry gives the device entry's bits
    g, _ = adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, gpu.MODE_AREA)
    rc, msg, gsrc = gpu.adjoint_host(g, (H, W), sr, dr, iso, ang)
    assert rc == 0, msg
    assert np.array_equal(gsrc, _adjoint(gpu, gpu.make_request(W, H, sr, dr, iso, ang), g))


def _golden_sweep(gpu, po, manifest, stride, tag):
    ran = 0
    for i in range(0, len(manifest), stride):             # a fixed stride by index, never a choice by outcome
        c = manifest[i]
        if c["W"] * c["H"] > 1300:
            continue
        ran += 1
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            _check_case(gpu, po, c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode, gpu.POLICY_REFERENCE,
                        "%s %d mode %d" % (tag, i, mode))
    return ran


def test_adjoint_on_the_reference_generated_small_geometries(gpu, po, small_golden):
    assert _golden_sweep(gpu, po, small_golden[1], 3, "small") >= 40


def test_adjoint_on_knife_edge_geometries(gpu, po, knife_golden):
    assert _golden_sweep(gpu, po, knife_golden[1], 4, "knife") >= 45


def test_adjoint_on_axis_knife_edge_geometries(gpu, po, axis_knife_golden):
    assert _golden_sweep(gpu, po, axis_knife_golden[1], 12, "axis knife") >= 45


# (name, W, H, srcRes, dstRes, angle): config 3, the 8:1 wide footprint, x2 up-sampling, theta = 0 and theta = 90
AT_SIZE = [("cfg3", 8192, 8192, 8192.0, 2731.0, 17.5), ("wide8", 8192, 8192, 8.0, 1.0, 17.5), ("up2", 2048, 2048, 1.0, 2.0, 30.0),
           ("axis4", 4096, 4096, 4.0, 1.0, 0.0), ("quarter2.5", 4096, 4096, 2.5, 1.0, 90.0)]


def _at_size(gpu, name, mode):
    """(rq, lay, x, y, W x, W^T y) on the device: x = synthetic seed 1, y = synthetic seed 2 at the dst size"""
    import torch
    _, W, H, sr, dr, ang = [c for c in AT_SIZE if c[0] == name][0]
    rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((H, W), dtype=torch.float32, device="cuda")
    y = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    gpu.synth_device(x.data_ptr(), W, H, W, 1, st)
    gpu.synth_device(y.data_ptr(), dW, dH, dW, 2, st)
    wx = torch.full((dH, dW), -1.0, dtype=torch.float32, device="cuda")
    wty = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
    gpu.resample_device(rq, x.data_ptr(), W, wx.data_ptr(), dW, st)
    gpu.adjoint_device(rq, y.data_ptr(), dW, wty.data_ptr(), W, st)
    torch.cuda.synchronize()
    return rq, lay, x, y, wx, wty


@pytest.mark.parametrize("name", [c[0] for c in AT_SIZE])
def test_adjoint_identity_against_the_shipped_forward(gpu, name):
    """<W x, y> = <x, W^T y>.  The forward is allowed TOL max(|v|, 1e-3) per pixel and the adjoint the bar of the matrix tests, so
    |lhs - rhs| <= TOL (sum_d max(|W x|_d, 1e-3) |y_d| + sum_s |x_s| max(|W^T y|_s, 1e-3 max|W^T y|)): no new number."""
    import torch
    lines = []
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq, lay, x, y, wx, wty = _at_size(gpu, name, mode)
        xd, yd, wxd, wtyd = x.double(), y.double(), wx.double(), wty.double()
        lhs, rhs = float((wxd * yd).sum()), float((xd * wtyd).sum())
        bound = TOL * (float((wxd.abs().clamp_min(1e-3) * yd.abs()).sum()) +
                       float((xd.abs() * wtyd.abs().clamp_min(1e-3 * float(wtyd.abs().max()))).sum()))
        lines.append("%-10s mode %d  %dx%d -> %dx%d  lhs %.9e  rhs %.9e  |lhs-rhs|/lhs %.3e  (allowed %.3e)" % (
            name, mode, rq.src_width, rq.src_height, lay.dst_width, lay.dst_height, lhs, rhs, abs(lhs - rhs) / abs(lhs), bound / abs(lhs)))
        print(lines[-1])
        assert float(wty.min()) >= 0.0           # the -1 prefill is gone everywhere (weights and y are non-negative)
        assert lhs > 0 and abs(lhs - rhs) <= bound, lines[-1]


def test_adjoint_is_deterministic_and_batches_match_single_images(gpu):
    import torch
    rq, lay, x, y, wx, wty = _at_size(gpu, "cfg3", gpu.MODE_AREA)
    _, _, _, _, _, again = _at_size(gpu, "cfg3", gpu.MODE_AREA)
    assert torch.equal(wty, again)
    del x, wx, again
    # a batch of 3 with padded strides and gaps between the images
    W, H, sr, dr, ang = 640, 480, 3.0, 1.0, 17.5
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        st = torch.cuda.current_stream().cuda_stream
        dstride, sstride = dW + 3, W + 5
        dimg, simg = dstride * dH + 17, sstride * H + 11
        gd = torch.zeros(3 * dimg, dtype=torch.float32, device="cuda")
        for b in range(3):
            gpu.synth_device(gd.data_ptr() + 4 * b * dimg, dW, dH, dstride, 10 + b, st)
        gs = torch.full((3 * simg,), -7.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, gd.data_ptr(), dstride, gs.data_ptr(), sstride, st, batch=3, dst_image_stride=dimg, src_image_stride=simg)
        torch.cuda.synchronize()
        touched = torch.zeros(3 * simg, dtype=torch.bool, device="cuda")
        for b in range(3):
            one_g = gd[b * dimg:b * dimg + dstride * dH].view(dH, dstride)[:, :dW].contiguous()
            one = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_device(rq, one_g.data_ptr(), dW, one.data_ptr(), W, st)
            torch.cuda.synchronize()
            assert torch.equal(gs[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W], one), (mode, b)
            touched[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W] = True
        assert bool((gs[~touched] == -7.0).all())          # padding and gaps untouched
        assert bool((gs[touched] >= 0.0).all())


def test_adjoint_scratch_pool_survives_shutdown(gpu):
    """aai_shutdown destroys the adjoint's memory pool; the next call creates it again and gives the same bits"""
    import torch
    W, H = 200, 160
    rq = gpu.make_request(W, H, 3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 17.5)
    lay = gpu.query(rq)[2]
    g = torch.rand((lay.dst_height, lay.dst_width), dtype=torch.float32, device="cuda")
    outs = []
    for _ in range(3):
        out = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, g.data_ptr(), lay.dst_width, out.data_ptr(), W, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(out)
        gpu.shutdown()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and float(outs[0].min()) >= 0.0


def test_torch_operator_forward_backward_and_streams(gpu):
    import torch
    from area_average_interpolation_amd import torch_ops
    assert gpu.resample is not None
    for (W, H, sr, dr, ang, mode) in ((24, 20, 3, 1, 17.5, gpu.MODE_AREA), (16, 12, 1, 2, 45, gpu.MODE_FAST), (160, 120, 2.5, 1, 90, gpu.MODE_AREA)):
        iso = ((W - 1) / 2, (H - 1) / 2)
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        B = 3
        gen = torch.Generator(device="cuda").manual_seed(5)
        x = torch.rand((B, H, W), dtype=torch.float32, device="cuda", generator=gen).requires_grad_(True)
        g = torch.rand((B, dH, dW), dtype=torch.float32, device="cuda", generator=gen)
        y, iso_out = torch_ops.resample(x, sr, dr, iso, ang, mode=mode)
        ref = torch.empty((B, dH, dW), dtype=torch.float32, device="cuda")
        gpu.resample_device(rq, x.data_ptr(), W, ref.data_ptr(), dW, torch.cuda.current_stream().cuda_stream, batch=B,
                            src_image_stride=W * H, dst_image_stride=dW * dH)
        assert torch.equal(y.detach(), ref) and tuple(iso_out) == (lay.dst_iso_x, lay.dst_iso_y)
        (y * g).sum().backward()
        gref = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, g.data_ptr(), dW, gref.data_ptr(), W, torch.cuda.current_stream().cuda_stream, batch=B,
                           dst_image_stride=dW * dH, src_image_stride=W * H)
        assert torch.equal(x.grad, gref)
        y2, _ = gpu.resample(x, sr, dr, iso, ang, mode=mode)             # the package-level export
        (y2 * g).sum().backward()
        assert torch.equal(x.grad, gref + gref)                          # gradients accumulate
        # (H, W) input, non-contiguous: made contiguous
        xt = x.detach()[0].t().contiguous().t()
        assert not xt.is_contiguous()
        y1, _ = torch_ops.resample(xt, sr, dr, iso, ang, mode=mode)
        assert y1.shape == (dH, dW) and torch.equal(y1, ref[0])
        # a side stream: correct after synchronising only that stream
        side = torch.cuda.Stream()
        xs = x.detach().clone().requires_grad_(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ys, _ = torch_ops.resample(xs, sr, dr, iso, ang, mode=mode)
            (ys * g).sum().backward()
        side.synchronize()
        assert torch.equal(ys.detach(), ref) and torch.equal(xs.grad, gref)
    # once differentiable: a double backward raises instead of treating the adjoint as a constant
    xx = torch.rand((12, 16), dtype=torch.float32, device="cuda", requires_grad=True)
    yy, _ = torch_ops.resample(xx, 2, 1, (7.5, 5.5), 30.0)
    (gx,) = torch.autograd.grad(yy.sum(), xx, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    # the comparison paths have no adjoint: refused up front when a gradient is wanted, fine without
    with pytest.raises(ValueError):
        torch_ops.resample(xx, 2, 1, (7.5, 5.5), 30.0, mode=gpu.MODE_BILINEAR)
    yb, _ = torch_ops.resample(xx.detach(), 2, 1, (7.5, 5.5), 30.0, mode=gpu.MODE_BILINEAR)
    assert yb.shape == yy.shape and not yb.requires_grad
    with pytest.raises(TypeError):
        torch_ops.resample(torch.zeros((8, 8), dtype=torch.float64, device="cuda"), 2, 1, (3.5, 3.5), 0.0)
    with pytest.raises(ValueError):
        torch_ops.resample(torch.zeros((8, 8), dtype=torch.float32), 2, 1, (3.5, 3.5), 0.0)
    with pytest.raises(ValueError):
        torch_ops.resample(torch.zeros((8,), dtype=torch.float32, device="cuda"), 2, 1, (3.5, 3.5), 0.0)
    with pytest.raises(gpu.AaiError):
        torch_ops.resample(torch.zeros((8, 8), dtype=torch.float32, device="cuda"), (1, 2), 1, (3.5, 3.5), 0.0)


def test_torch_operator_refuses_an_unprepared_geometry_inside_a_capture(gpu, monkeypatch):
    """the guard itself: with the current stream reported as capturing, a geometry without a plan raises instead of building one
    (which would synchronise); a prepared geometry goes through"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 96, 80
    x = torch.rand((H, W), dtype=torch.float32, device="cuda")
    args = (3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 21.25)                 # a geometry no other test of this module prepares
    assert gpu.plan_shape(gpu.make_request(W, H, *args)) == ""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        torch_ops.resample(x, *args)
    assert gpu.plan_shape(gpu.make_request(W, H, *args)) == ""
    monkeypatch.undo()
    eager, _ = torch_ops.resample(x, *args)                              # prepares the plan outside a capture
    assert gpu.plan_shape(gpu.make_request(W, H, *args)) != ""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    again, _ = torch_ops.resample(x, *args)
    torch.cuda.synchronize()
    assert torch.equal(again, eager)
