"""The interleaved-channel adjoint on the MI355X (aai_adjoint_interleaved_device_f32, csrc/aai_adjoint_multi.hip) and the torch operator's
(B, C, H, W) input.

The oracle's matrix on the eight geometries of DESIGN.md section 9; everything else bit for bit against the shipped single-channel entry
(aai_adjoint_batch_device_f32, which tests/test_adjoint_gpu.py pins to the oracle and which this change does not touch): partial tiles
on both sides, padded strides and gaps in guarded buffers, the reference-generated knife-edge geometries, a batch whose C-fold scratch
goes through in two chunks; and the two routes of the torch operator."""
import numpy as np
import pytest

from conftest import TOL, rel_err
from guard_layout import GuardedLayout, to_device, to_numpy
from test_adjoint_interleaved_host import EIGHT, VARIANTS, assert_oracle_bar, interleaved_gold

pytestmark = pytest.mark.gpu

MULTI_GATHER = "aai_adjoint_gather_multi_kernel"


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _mode_name(gpu, mode):
    return "fast" if mode == gpu.MODE_FAST else "area"


def _interleaved(gpu, rq, g):
    """aai_adjoint_interleaved_device_f32 on a dense gradient image [dH, dW, C] (numpy or device tensor); gsrc [H, W, C] on the device,
    prefilled with -1"""
    import torch
    gd = g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
    assert gd.is_contiguous()
    dH, dW, C = gd.shape
    gs = torch.full((rq.src_height, rq.src_width, C), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), rq.src_width * C, _stream(), batch=1)
    torch.cuda.synchronize()
    assert gpu.last_kernel() == "%s<%s, %d>" % (MULTI_GATHER, _mode_name(gpu, rq.mode), C), gpu.last_kernel()
    return gs


def _single(gpu, rq, plane):
    """the shipped single-channel entry on one dense plane [dH, dW] (device tensor); gsrc [H, W] on the device"""
    import torch
    gd = plane.contiguous()
    gs = torch.full((rq.src_height, rq.src_width), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), gd.shape[1], gs.data_ptr(), rq.src_width, _stream(), batch=1)
    torch.cuda.synchronize()
    assert "aai_adjoint_gather_kernel" in gpu.last_kernel()
    return gs


def _same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", range(len(EIGHT)))
def test_interleaved_adjoint_matches_the_oracle_matrix(gpu, po, case):
    for variant in VARIANTS:
        rq, g, gold = interleaved_gold(po, gpu, case, variant, 3)
        got = _interleaved(gpu, rq, g).cpu().numpy()
        assert_oracle_bar(got, gold, "interleaved C=3 case %d %s policy %d" % ((case,) + variant))
    # the host-buffer entry gives the device entry's bits
    W, H, sr, dr, ang, off = EIGHT[case]
    rq, g, _ = interleaved_gold(po, gpu, case, VARIANTS[0], 3)
    rc, msg, gsrc = gpu.adjoint_interleaved_host(g, (H, W, 3), sr, dr, ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1]), ang)
    assert rc == 0, msg
    assert np.array_equal(gsrc.view(np.int32), _interleaved(gpu, rq, g).cpu().numpy().view(np.int32))


# (W, H, srcRes, dstRes, angle): the last 16 x 16 tiles are partial; the last one is grid-aligned, so nearly every boundary pair is a knife edge
PARTIAL_TILES = [(37, 29, 3.0, 1.0, 17.5), (33, 18, 1.0, 2.0, 30.0), (40, 24, 2.5, 1.0, 90.0), (32, 32, 4.0, 1.0, 0.0)]


@pytest.mark.parametrize("channels", (2, 3, 4))
@pytest.mark.parametrize("geo", PARTIAL_TILES, ids=["%dx%d-%g-%g-%g" % g for g in PARTIAL_TILES])
def test_channels_have_the_single_channel_entrys_bits_in_guarded_buffers(gpu, geo, channels):
    """batch 3, row strides of width x C + 5, a gap between the images, poison in guards, padding and gaps: every channel bit for bit the
    single-channel call on that plane, nothing but the entitled elements touched on either buffer, the same bits on a second call"""
    import torch
    W, H, sr, dr, ang = geo
    B, C = 3, channels
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
        rc, msg, lay = gpu.query(rq)
        assert rc == 0, msg
        dW, dH = lay.dst_width, lay.dst_height
        gl = GuardedLayout((B, dH, dW, C), stride=dW * C + 5, image_stride=(dW * C + 5) * dH + 37, base_offset=12)
        sl = GuardedLayout((B, H, W, C), stride=W * C + 5, image_stride=(W * C + 5) * H + 29, base_offset=4)
        values = np.random.default_rng(3 * W + C).random((B, dH, dW, C)).astype(np.float32)
        ghost = gl.make_src(values, "nan")
        gdev = to_device(ghost)
        results = []
        for _ in range(2):
            sdev = to_device(sl.make_dst())
            gpu.adjoint_interleaved_device(rq, C, gl.ptr(gdev), gl.stride, sl.ptr(sdev), sl.stride, _stream(), batch=B,
                                           dst_image_stride=gl.image_stride, src_image_stride=sl.image_stride)
            torch.cuda.synchronize()
            what = (gpu.last_kernel(), geo, mode, C)
            assert gpu.last_kernel() == "%s<%s, %d>" % (MULTI_GATHER, _mode_name(gpu, mode), C), what
            out, first, count = sl.check_dst(sdev)
            assert count == 0, ("%d guard elements of gsrc were written, first: %s" % (count, sl.describe(first)), what)
            assert GuardedLayout.sentinels_left(out) == 0, what
            assert not np.isnan(out).any(), ("padding or a gap of gdst was read", what)
            # gdst is an input: guards, padding, gaps and values as uploaded
            assert np.array_equal(to_numpy(gdev, np.int32), ghost.view(np.int32)), what
            results.append(out)
        assert np.array_equal(results[0].view(np.int32), results[1].view(np.int32)), what
        planes = torch.from_numpy(values).cuda()
        nonzero = 0
        for b in range(B):
            for c in range(C):
                one = _single(gpu, rq, planes[b, :, :, c]).cpu().numpy()
                assert np.array_equal(results[0][b, :, :, c].view(np.int32), one.view(np.int32)), (what, b, c)
                nonzero += int((one != 0).sum())
        assert nonzero > 0, what


def _knife_sweep(gpu, manifest, stride, tag):
    """C = 2 on every `stride`-th geometry (by index, never by outcome), both modes; returns (cases run, cases with a non-zero gradient in
    every channel)"""
    import torch
    ran = full = 0
    gen = torch.Generator(device="cuda").manual_seed(17)
    for i in range(0, len(manifest), stride):
        c = manifest[i]
        ran += 1
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode)
            rc, msg, lay = gpu.query(rq)
            assert rc == 0, msg
            g = torch.rand((lay.dst_height, lay.dst_width, 2), dtype=torch.float32, device="cuda", generator=gen)
            got = _interleaved(gpu, rq, g)
            live = True
            for ch in range(2):
                one = _single(gpu, rq, g[:, :, ch])
                assert _same_bits(got[:, :, ch], one), ("%s %d mode %d channel %d" % (tag, i, mode, ch))
                live = live and bool((one != 0).any())
            full += 1 if live and mode == gpu.MODE_AREA else 0
    return ran, full


def test_knife_edge_geometries_have_the_single_channel_bits(gpu, knife_golden, axis_knife_golden):
    ran, full = _knife_sweep(gpu, knife_golden[1], 8, "knife")
    assert ran == len(range(0, len(knife_golden[1]), 8)) and ran >= 20 and full >= 1
    ran, full = _knife_sweep(gpu, axis_knife_golden[1], 24, "axis knife")
    assert ran == len(range(0, len(axis_knife_golden[1]), 24)) and ran >= 20 and full >= 1


def test_scratch_chunking_with_four_channels(gpu):
    """fast mode, C = 4, 512^2 up-sampled x2: the batch is the smallest whose 4-channel scratch takes two chunks of the engine's 1 GiB bound,
    plus one image so that the second chunk has a first and a last one.  The same batch of single-channel images would fit in one chunk."""
    import torch
    W, H, C = 512, 512, 4
    rq = gpu.make_request(W, H, 1.0, 2.0, ((W - 1) / 2, (H - 1) / 2), 0.0, mode=gpu.MODE_FAST)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    assert (dW, dH) == (1024, 1024)
    per_image = dW * dH * C * 8
    chunk = (1 << 30) // per_image
    batch = chunk + 2
    assert 1 < chunk and per_image * (chunk + 1) > (1 << 30) and (per_image // C) * batch <= (1 << 30)
    gen = torch.Generator(device="cuda").manual_seed(23)
    gd = torch.rand((batch, dH, dW, C), dtype=torch.float32, device="cuda", generator=gen)
    gs = torch.full((batch, H, W, C), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, _stream(), batch=batch,
                                   dst_image_stride=dH * dW * C, src_image_stride=H * W * C)
    torch.cuda.synchronize()
    assert gpu.last_kernel() == MULTI_GATHER + "<fast, 4>"
    assert float(gs.min()) >= 0.0                                # the -1 prefill is gone in every image of both chunks
    for b in (0, chunk - 1, chunk, batch - 1):
        one = _interleaved(gpu, rq, gd[b])
        assert _same_bits(gs[b], one) and bool((one != 0).any()), b


def _planes_reference(gpu, torch_ops, x, g, args, **kw):
    """(y, x.grad) of the existing 3-D operator on the B * C planes of a contiguous (B, C, H, W) tensor"""
    B, C, H, W = x.shape
    xp = x.detach().contiguous().view(B * C, H, W).clone().requires_grad_(True)
    yp, iso = torch_ops.resample(xp, *args, **kw)
    (yp * g.contiguous().view(B * C, g.shape[2], g.shape[3])).sum().backward()
    return yp.detach().view(B, C, g.shape[2], g.shape[3]), xp.grad.view(B, C, H, W), iso


def _case_tensors(gpu, W, H, sr, dr, ang, B=2, C=3, seed=5):
    import torch
    iso = ((W - 1) / 2, (H - 1) / 2)
    lay = gpu.query(gpu.make_request(W, H, sr, dr, iso, ang))[2]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((B, C, H, W), dtype=torch.float32, device="cuda", generator=gen)
    g = torch.rand((B, C, lay.dst_height, lay.dst_width), dtype=torch.float32, device="cuda", generator=gen)
    return x, g, (sr, dr, iso, ang), lay


def test_torch_operator_planar_route(gpu):
    import torch
    from area_average_interpolation_amd import torch_ops
    for (W, H, sr, dr, ang, kw) in ((37, 29, 3.0, 1.0, 17.5, {}), (37, 29, 3.0, 1.0, 17.5, {"mode": gpu.MODE_FAST}),
                                    (40, 24, 2.5, 1.0, 90.0, {"planned_backward": True})):
        x, g, args, lay = _case_tensors(gpu, W, H, sr, dr, ang)
        yref, gref, iso_ref = _planes_reference(gpu, torch_ops, x, g, args, **kw)
        xr = x.clone().requires_grad_(True)
        y, iso = torch_ops.resample(xr, *args, **kw)
        assert y.shape == (2, 3, lay.dst_height, lay.dst_width) and y.is_contiguous() and tuple(iso) == tuple(iso_ref)
        (y * g).sum().backward()
        assert _same_bits(y.detach(), yref) and _same_bits(xr.grad, gref), (W, H, ang, kw)
        if kw.get("planned_backward"):
            rq = gpu.make_request(W, H, sr, dr, args[2], ang)
            assert "adjoint=tables" in gpu.plan_shape(rq)          # the planned backward really was asked for
    y2, _ = gpu.resample(x, *args)                                  # the package-level export takes 4-D input too
    assert y2.shape == y.shape


def test_torch_operator_interleaved_route(gpu):
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H, sr, dr, ang = 37, 29, 3.0, 1.0, 17.5
    x, g, args, lay = _case_tensors(gpu, W, H, sr, dr, ang)
    dW, dH = lay.dst_width, lay.dst_height
    rq = gpu.make_request(W, H, sr, dr, args[2], ang)
    yref, gref, _ = _planes_reference(gpu, torch_ops, x, g, args)
    xl = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert xl.is_contiguous(memory_format=torch.channels_last) and not xl.is_contiguous()
    y, iso = torch_ops.resample(xl, *args)
    assert y.shape == (2, 3, dH, dW) and y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
    assert tuple(iso) == (lay.dst_iso_x, lay.dst_iso_y)
    assert gpu.plan_shape(rq, 3) != ""
    err = rel_err(y.detach().cpu().numpy(), yref.cpu().numpy())          # (floor 1e-3, the forward's bar)
    print("interleaved forward against the planar forward: max rel err %.3e" % float(err.max()))
    assert float(err.max()) <= TOL
    (y * g).sum().backward()
    assert xl.grad.shape == xl.shape and xl.grad.is_contiguous(memory_format=torch.channels_last) and not xl.grad.is_contiguous()
    # bit for bit the single-channel adjoint of the planes of gy (= g)
    for b in range(2):
        for c in range(3):
            assert _same_bits(xl.grad[b, c], _single(gpu, rq, g[b, c])), (b, c)
    # (aai_last_kernel() is per thread and autograd runs the backward on a thread of its own: the kernel is named by the direct call
    # below, whose bits the gradient must equal)
    gl = g.contiguous(memory_format=torch.channels_last)
    direct = torch.empty_like(xl.grad)
    gpu.adjoint_interleaved_device(rq, 3, gl.data_ptr(), dW * 3, direct.data_ptr(), W * 3, _stream(), batch=2,
                                   dst_image_stride=dH * dW * 3, src_image_stride=H * W * 3)
    torch.cuda.synchronize()
    assert gpu.last_kernel() == MULTI_GATHER + "<area, 3>"
    assert _same_bits(xl.grad.permute(0, 2, 3, 1), direct.permute(0, 2, 3, 1))
    # a gy that is not channels_last is made so
    xl2 = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y2, _ = torch_ops.resample(xl2, *args)
    y2.backward(g.contiguous())
    assert _same_bits(xl2.grad, xl.grad) and _same_bits(y2.detach(), y.detach())
    # channels_last with C = 5 and C = 1: the planar route's bits
    for C in (5, 1):
        xc, gc, _, _ = _case_tensors(gpu, W, H, sr, dr, ang, C=C, seed=9)
        yref_c, gref_c, _ = _planes_reference(gpu, torch_ops, xc, gc, args)
        xcl = xc.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        yc, _ = torch_ops.resample(xcl, *args)
        (yc * gc).sum().backward()
        assert yc.shape == yref_c.shape and _same_bits(yc.detach(), yref_c) and _same_bits(xcl.grad, gref_c), C
    # channels_last, C = 3, planned_backward at 90 degrees: the planar route, hence the planned single-channel adjoint's bits
    xq, gq, args_q, _ = _case_tensors(gpu, 40, 24, 2.5, 1.0, 90.0)
    yref_q, gref_q, _ = _planes_reference(gpu, torch_ops, xq, gq, args_q, planned_backward=True)
    xql = xq.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yq, _ = torch_ops.resample(xql, *args_q, planned_backward=True)
    (yq * gq).sum().backward()
    assert _same_bits(yq.detach(), yref_q) and _same_bits(xql.grad, gref_q)
    # B = 0 and C = 0: empty tensors of the output's shape
    for shape in ((0, 3, H, W), (2, 0, H, W)):
        for fmt in (torch.contiguous_format, torch.channels_last):
            ye, _ = torch_ops.resample(torch.empty(shape, dtype=torch.float32, device="cuda").contiguous(memory_format=fmt), *args)
            assert ye.shape == (shape[0], shape[1], dH, dW) and ye.dtype == torch.float32 and ye.is_cuda
    # a side stream: correct after synchronising only that stream
    side = torch.cuda.Stream()
    xs = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ys, _ = torch_ops.resample(xs, *args)
        (ys * g).sum().backward()
    side.synchronize()
    assert _same_bits(ys.detach(), y.detach()) and _same_bits(xs.grad, xl.grad)
    # the comparison paths have no adjoint, in either layout
    with pytest.raises(ValueError):
        torch_ops.resample(xs, *args, mode=gpu.MODE_BILINEAR)
    yb, _ = torch_ops.resample(xs.detach(), *args, mode=gpu.MODE_BILINEAR)
    assert yb.shape == y.shape and not yb.requires_grad
    with pytest.raises(ValueError):
        torch_ops.resample(torch.zeros((1, 1, 2, 8, 8), dtype=torch.float32, device="cuda"), 2, 1, (3.5, 3.5), 0.0)
