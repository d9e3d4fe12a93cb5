"""The adjoint (transposed) resampling on the MI355X: gsrc = W^T gdst.

Small geometries against the oracle's matrix built column by column (eight hand-picked ones, strides through the golden and knife-edge
fixtures).  Everything larger per source pixel against columns of the same matrix taken from comb images (tests/adjoint_columns.py: the
oracle on a source that is 1 at isolated pixels is a set of columns of W; a second run with labels assigns each dst pixel to its source
pixel and proves the spacing): every tile edge and residue modulo 16 of mid-size images whose last workgroups are partial, in every
quadrant, mode, policy and up- / down-sampling regime; at size (8192^2 and the other AT_SIZE geometries) the corners, the border ring,
the interior and both sides of workgroup boundaries far from the origin; the launch limits the code provides for (sources and
outputs taller than one grid, batches of several scratch chunks and of more than 65,535 images, gradient images past 4 GiB); and the
torch operator's gradient by its definition.  The adjoint identity <W x, y> = <x, W^T y> against the shipped forward stays as one
scalar per run beside them, with determinism, batches with padded strides, and the operator's plumbing."""
import numpy as np
import pytest

from conftest import TOL
from adjoint_columns import comb_cases, comb_gold_pixels, comb_pitch, edge_phases
from grid_carry_cases import rows_pixels as _rows_pixels
from test_adjoint_host import EIGHT, adjoint_gold, assert_adjoint_matches, oracle_matrix

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


# ---- per source pixel against comb gold (tests/adjoint_columns.py) ----

def _omode(gpu, po, mode):
    return po.MODE_FAST if mode == gpu.MODE_FAST else po.MODE_EXACT


def _adjoint_tensor(gpu, rq, lay, gd):
    """one adjoint call on a dense device gradient image; gsrc (device) prefilled with -1"""
    import torch
    assert gd.shape == (lay.dst_height, lay.dst_width) and gd.is_contiguous()
    gs = torch.full((rq.src_height, rq.src_width), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), lay.dst_width, gs.data_ptr(), rq.src_width, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return gs


def _at(t, xs, ys):
    """elements (ys[k], xs[k]) of a 2-D device tensor, on the host"""
    import torch
    return t[torch.as_tensor(np.asarray(ys, np.int64), device=t.device), torch.as_tensor(np.asarray(xs, np.int64), device=t.device)].cpu().numpy()


def _check_listed(gpu, po, rq, lay, gd, gs, sx, sy, what, image=None):
    """the listed source pixels of one adjoint result against the pixel-list comb; returns the number compared"""
    gold, evaluated = comb_gold_pixels(po, _omode(gpu, po, rq.mode), rq, lay, lambda dx, dy: _at(gd, dx, dy), sx, sy, image=image)
    assert 4 * int((gold != 0).sum()) >= len(sx), (what, int((gold != 0).sum()), len(sx))     # the sample is not all in unread corners
    assert_adjoint_matches(_at(gs, sx, sy), gold, "%s (%d source pixels, %d oracle dst pixels)" % (what, len(sx), evaluated))
    return len(sx)


# (name, W, H, srcRes, dstRes, angle, isocenter offset, mode, policy): no size is a multiple of 16, so the last workgroup row and column
# are partial.  Quadrants 0-3, both policies and fast mode, 16:1 ... 1:3 (scale 1, 2, 3 and 5), multiples of 90 degrees, a near-axis angle.
TILE_EDGE = [
    ("3:1 q0", 300, 221, 3, 1, 17.5, (0, 0), "area", 0), ("3:1 q0 exact", 300, 221, 3, 1, 17.5, (0, 0), "area", 1), ("3:1 q0 fast", 300, 221, 3, 1, 17.5, (0, 0), "fast", 0),
    ("1:1 q0 scale 2", 203, 187, 1, 1, 30.0, (0.3, -0.2), "area", 0), ("1:2 q1 scale 3", 101, 93, 1, 2, 117.5, (0, 0), "area", 0),
    ("1:3 q2 scale 5", 90, 83, 1, 3, 200.25, (-3, 4), "fast", 0), ("1:2 q3 scale 3 exact", 85, 99, 1, 2, 305.0, (0, 0), "area", 1),
    ("1:2 q0 scale 3 fast", 93, 101, 1, 2, 45.0, (0, 0), "fast", 0),
    ("4:1 0", 250, 230, 4, 1, 0.0, (0, 0), "area", 0), ("2.5:1 90", 210, 190, 2.5, 1, 90.0, (0, 0), "area", 0), ("2:1 180 fast", 150, 170, 2, 1, 180.0, (0.5, 0.5), "fast", 0),
    ("1:1 270 scale 2", 130, 110, 1, 1, 270.0, (0, 0), "area", 0), ("3:1 near axis", 290, 310, 3, 1, 1e-7, (0, 0), "area", 0),
    ("8:1 q2", 250, 270, 8, 1, 200.25, (-3, 4), "area", 0), ("16:1 q0 fast", 410, 430, 16, 1, 17.5, (0, 0), "fast", 0), ("16:1 q1", 430, 410, 16, 1, 107.5, (0, 0), "area", 0),
    ("1.7:1 q3", 190, 230, 1.7, 1, 290.0, (0, 0), "area", 0),
]


@pytest.mark.parametrize("case", TILE_EDGE, ids=[c[0] for c in TILE_EDGE])
def test_adjoint_at_every_tile_edge(gpu, po, case):
    """3a.  Full oracle combs of odd pitch over images at least 16 pitches a side: each phase walks through every residue of sx and of
    sy modulo 16, and the phases put columns 0, 15, 16, 17, W-2, W-1 and the same rows among the pixels (asserted)."""
    name, W, H, sr, dr, ang, off, mode, policy = case
    assert W % 16 and H % 16
    mode = gpu.MODE_FAST if mode == "fast" else gpu.MODE_AREA
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    pitch = comb_pitch(lay, ang)
    assert pitch % 2 == 1 and min(W, H) >= 16 * pitch
    g = np.random.default_rng(11).random((lay.dst_height, lay.dst_width)).astype(np.float32)
    sx, sy, gold = comb_cases(po, _omode(gpu, po, mode), W, H, sr, dr, iso, ang, policy, g, edge_phases(W, H, pitch), pitch)
    for c, n, v in ((sx, W, "column"), (sy, H, "row")):
        assert set(np.unique(c % 16)) == set(range(16)), v
        assert set((0, 15, 16, 17, n - 2, n - 1)) <= set(c.tolist()), v
    assert sx.size >= 2 * (W // pitch) * (H // pitch) and 4 * int((gold != 0).sum()) >= sx.size
    got = _adjoint(gpu, rq, g)
    assert_adjoint_matches(got[sy, sx], gold, "tile edges %s (%d source pixels)" % (name, sx.size))


# 3b.  Source pixels compared per AT_SIZE geometry and mode: 64 in the corners (the 4 x 4 block of each), 192 of the border ring, 384 of the
# interior, 192 at workgroup boundaries far from the origin = 832 (826 where two draws coincide).  Measured oracle time per configuration
# (aai_oracle_pixels, comb + labels, candidate search included, one CPU core): 3:1, 4,881 dst pixels, 0.9 s (~90 us per pixel and run);
# 8:1, 2,365 dst pixels, 0.7 s (~150 us); x2 up-sampling, 57,107 dst pixels, 3.4 s (~30 us).
N_RING, N_INTERIOR, N_BOUNDARY_K = 192, 384, 12


def _at_size_pixels(W, H, seed):
    """drawn by seed and index before anything is computed"""
    rng = np.random.default_rng(seed)
    px = []
    for cx in (0, W - 4):
        for cy in (0, H - 4):
            px += [(cx + i, cy + j) for j in range(4) for i in range(4)]
    side, t = rng.integers(0, 4, N_RING), rng.random(N_RING)
    for s, u in zip(side, t):
        a, b = 1 + int(u * (W - 2)), 1 + int(u * (H - 2))
        px.append(((a, 0), (a, H - 1), (0, b), (W - 1, b))[s])
    px += [(int(x), int(y)) for x, y in zip(rng.integers(4, W - 4, N_INTERIOR), rng.integers(4, H - 4, N_INTERIOR))]
    # both sides of workgroup boundaries far from the origin: sx or sy in {16k-1, 16k}, k in the upper half of the image, and the four
    # pixels where two boundaries cross -- 16 pixels per k
    for i in range(N_BOUNDARY_K):
        kx, ky = W // 16 - 1 - int(rng.integers(0, W // 32)), H // 16 - 1 - int(rng.integers(0, H // 32))
        ox, oy = int(rng.integers(4, W - 4)), int(rng.integers(4, H - 4))
        px += [(16 * kx - 1, oy), (16 * kx, oy), (ox, 16 * ky - 1), (ox, 16 * ky)]
        px += [(16 * kx - 1 + i2, 16 * ky - 1 + j2) for j2 in range(2) for i2 in range(2)]
        px += [(16 * kx - 1 + i2, 5 + i) for i2 in range(2)] + [(7 + i, 16 * ky - 1 + j2) for j2 in range(2)]
        px += [(16 * kx - 1 + i2, H - 1) for i2 in range(2)] + [(W - 1, 16 * ky - 1 + j2) for j2 in range(2)]
    px = list(dict.fromkeys(px))                                 # duplicates (by coordinates, not by outcome) dropped, order kept
    return np.array([p[0] for p in px]), np.array([p[1] for p in px])


@pytest.mark.parametrize("name", [c[0] for c in AT_SIZE])
def test_adjoint_per_pixel_at_size(gpu, po, name):
    import torch
    _, W, H, sr, dr, ang = [c for c in AT_SIZE if c[0] == name][0]
    image = np.zeros((H, W), np.float32)
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
        rc, msg, lay = gpu.query(rq)
        assert rc == 0, msg
        gd = torch.empty((lay.dst_height, lay.dst_width), dtype=torch.float32, device="cuda")
        gpu.synth_device(gd.data_ptr(), lay.dst_width, lay.dst_height, lay.dst_width, 2, torch.cuda.current_stream().cuda_stream)
        gs = _adjoint_tensor(gpu, rq, lay, gd)
        sx, sy = _at_size_pixels(W, H, 2024)
        assert 800 <= sx.size <= 64 + N_RING + N_INTERIOR + 16 * N_BOUNDARY_K and (sx >= W - 16).any() and (sy >= H - 16).any()
        assert _check_listed(gpu, po, rq, lay, gd, gs, sx, sy, "at size %s mode %d" % (name, mode), image=image) == sx.size
        assert not image.any()
        del gd, gs
    torch.cuda.empty_cache()


def test_adjoint_taller_than_one_grid(gpu, po):
    """3c.  More than 65,535 x 16 source rows (the gather goes band by band: launch_adjoint's second loop) and more than that many dst
    rows (the normaliser's loop: a narrow image up-sampled x2).  Source rows on both sides of the band boundary, the first and the last
    rows; for the tall dst the source rows that the dst rows around 65,535 x 16 feed."""
    import torch
    edge = 65535 * 16
    for (W, H, sr, dr, ang, rows_of) in ((40, 1_100_000, 1.0, 1.0, 0.05, lambda H, dH: [0, 1, edge - 17, edge - 16, edge - 2, edge - 1, edge, edge + 1, edge + 15, edge + 16, H - 2, H - 1]),
                                         (24, 560_000, 1.0, 2.0, 0.05, lambda H, dH: [0, 1] + list(range(int(edge * H / dH) - 8, int(edge * H / dH) + 9)) + [H - 2, H - 1])):
        image = np.zeros((H, W), np.float32)
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            rc, msg, lay = gpu.query(rq)
            assert rc == 0, msg
            assert (H if dr == 1.0 else lay.dst_height) > edge + 16, (H, lay.dst_height)
            gd = torch.empty((lay.dst_height, lay.dst_width), dtype=torch.float32, device="cuda")
            gpu.synth_device(gd.data_ptr(), lay.dst_width, lay.dst_height, lay.dst_width, 4, torch.cuda.current_stream().cuda_stream)
            gs = _adjoint_tensor(gpu, rq, lay, gd)
            sx, sy = _rows_pixels(W, rows_of(H, lay.dst_height), 5)
            assert sx.size >= 60
            _check_listed(gpu, po, rq, lay, gd, gs, sx, sy, "tall %dx%d -> %dx%d mode %d" % (W, H, lay.dst_width, lay.dst_height, mode), image=image)
            assert float(gs.min()) >= 0.0                        # the -1 prefill is gone in every band
            del gd, gs
        torch.cuda.empty_cache()


def _batch_against_singles(gpu, rq, lay, batch, check, pad):
    """a batch with padded strides and gaps (pad = (dst columns, dst gap, src columns, src gap)); the images listed in `check` bit for bit
    against single-image calls, padding untouched.  Returns (gd of the last checked image, its gsrc, both dense on the device)."""
    import torch
    W, H, dW, dH = rq.src_width, rq.src_height, lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    dstride, sstride = dW + pad[0], W + pad[2]
    dimg, simg = dstride * dH + pad[1], sstride * H + pad[3]
    gen = torch.Generator(device="cuda").manual_seed(9)
    gd = torch.rand(batch * dimg, dtype=torch.float32, device="cuda", generator=gen)
    gs = torch.full((batch * simg,), -7.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), dstride, gs.data_ptr(), sstride, st, batch=batch, dst_image_stride=dimg, src_image_stride=simg)
    torch.cuda.synchronize()
    # padding and gaps untouched, every image pixel written (weights and gradients are non-negative)
    view = gs.view(batch, simg)
    rows = view[:, :sstride * H].view(batch, H, sstride)
    assert bool((rows[:, :, W:] == -7.0).all()) and bool((view[:, sstride * H:] == -7.0).all())
    assert bool((rows[:, :, :W] >= 0.0).all())
    one_g = one = None
    for b in check:
        one_g = gd[b * dimg:b * dimg + dstride * dH].view(dH, dstride)[:, :dW].contiguous()
        one = _adjoint_tensor(gpu, rq, lay, one_g)
        assert torch.equal(rows[b, :, :W], one), b
    return one_g, one


def test_adjoint_batch_of_several_scratch_chunks(gpu, po):
    """3c.  96 images of 1000 x 1000 at 1:1: 12.6 MB of fp64 scratch each, 1.2 GB for the batch, so enqueue_adjoint cuts it into chunks of
    85 + 11 and reuses the scratch.  EVERY image equals its single-image call; the first image of the second chunk against comb gold."""
    import torch
    W, H = 1000, 1000
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, 1.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 17.5, mode=mode)
        lay = gpu.query(rq)[2]
        per_image = lay.dst_width * lay.dst_height * 8
        chunk = (1 << 30) // per_image
        batch = 96
        assert 1 < chunk < batch and per_image * batch > (1 << 30)
        check = list(range(batch))
        check.remove(chunk)
        one_g, one = _batch_against_singles(gpu, rq, lay, batch, check + [chunk], (3, 17, 5, 11))
        sx, sy = _at_size_pixels(W, H, 77)
        _check_listed(gpu, po, rq, lay, one_g, one, sx[::4], sy[::4], "chunked batch image %d mode %d" % (chunk, mode))
        del one_g, one
        torch.cuda.empty_cache()


def test_adjoint_batch_of_more_than_65535_images(gpu, po):
    """3c.  65,600 images of 12 x 10 (grid.z carries 65,535): images 0, 65534, 65535, 65536 and the last equal their single-image calls; the
    last one checked against the oracle's matrix at every pixel."""
    W, H, sr, dr, ang = 12, 10, 2.0, 1.0, 17.5
    iso = ((W - 1) / 2, (H - 1) / 2)
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
        lay = gpu.query(rq)[2]
        batch = 65600
        one_g, one = _batch_against_singles(gpu, rq, lay, batch, [0, 65534, 65535, 65536, batch - 1], (1, 3, 2, 5))
        M = oracle_matrix(po, _omode(gpu, po, mode), W, H, sr, dr, iso, ang)
        gold = (M.T @ one_g.cpu().numpy().astype(np.float64).ravel()).reshape(H, W)
        assert_adjoint_matches(one.cpu().numpy(), gold, "batch of %d, last image, mode %d (%d source pixels)" % (batch, mode, W * H))


def _band_pixels(W, H, seed, per_band=48):
    """the 4 x 4 corner blocks and seeded pixels in the top 64 rows, 64 rows around the middle and the last 64 rows"""
    rng = np.random.default_rng(seed)
    px = []
    for cx in (0, W - 4):
        for cy in (0, H - 4):
            px += [(cx + i, cy + j) for j in range(4) for i in range(4)]
    for r0 in (0, H // 2 - 32, H - 64):
        px += [(int(x), r0 + int(y)) for x, y in zip(rng.integers(0, W, per_band), rng.integers(0, 64, per_band))]
    px = list(dict.fromkeys(px))
    return np.array([p[0] for p in px]), np.array([p[1] for p in px])


@pytest.mark.parametrize("shape", [(33000, 33000, 3.0, 1.0, 17.5), (12400, 12400, 1.0, 3.0, 17.5)], ids=["gsrc 4.36 GB", "gdst 8.7 GB"])
def test_adjoint_gradient_images_past_4_gib(gpu, po, shape):
    """3c.  A 33,000^2 source at 3:1 (gsrc: 4.36 GB, byte offsets past 32 bits) and a 12,400^2 source up-sampled x3 (gdst: 46,662^2 =
    2.18 G elements, 8.7 GB, past 32-bit ELEMENT offsets; 17.4 GB of fp64 scratch).  Corners and source rows near the top, the middle and
    the end."""
    import torch
    W, H, sr, dr, ang = shape
    image = np.zeros((H, W), np.float32)
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
        rc, msg, lay = gpu.query(rq)
        assert rc == 0, msg
        assert max(W * H, lay.dst_width * lay.dst_height) * 4 > (1 << 32)
        if dr > sr:
            assert lay.dst_width * lay.dst_height > (1 << 31)
        gd = torch.empty((lay.dst_height, lay.dst_width), dtype=torch.float32, device="cuda")
        gpu.synth_device(gd.data_ptr(), lay.dst_width, lay.dst_height, lay.dst_width, 6, torch.cuda.current_stream().cuda_stream)
        gs = _adjoint_tensor(gpu, rq, lay, gd)
        sx, sy = _band_pixels(W, H, 31)
        assert sx.size >= 200
        _check_listed(gpu, po, rq, lay, gd, gs, sx, sy, "past 4 GiB %dx%d -> %dx%d mode %d" % (W, H, lay.dst_width, lay.dst_height, mode), image=image)
        del gd, gs
        torch.cuda.empty_cache()


def test_torch_operator_gradient_is_the_adjoint_by_definition(gpu, po):
    """3d.  d/dx sum(resample(x) * g) = W^T g against comb gold directly: autograd -> adjoint -> kernel, end to end"""
    import torch
    from area_average_interpolation_amd import torch_ops
    total = 0
    for (W, H, sr, dr, ang, mode) in ((203, 187, 3.0, 1.0, 17.5, gpu.MODE_AREA), (101, 93, 1.0, 2.0, 117.5, gpu.MODE_FAST)):
        iso = ((W - 1) / 2, (H - 1) / 2)
        lay = gpu.query(gpu.make_request(W, H, sr, dr, iso, ang, mode=mode))[2]
        pitch = comb_pitch(lay, ang)
        gen = torch.Generator(device="cuda").manual_seed(3)
        x = torch.rand((2, H, W), dtype=torch.float32, device="cuda", generator=gen).requires_grad_(True)
        g = torch.rand((2, lay.dst_height, lay.dst_width), dtype=torch.float32, device="cuda", generator=gen)
        y, _ = torch_ops.resample(x, sr, dr, iso, ang, mode=mode)
        (gx,) = torch.autograd.grad((y * g).sum(), x)
        for b in range(2):
            sx, sy, gold = comb_cases(po, _omode(gpu, po, mode), W, H, sr, dr, iso, ang, 0, g[b].cpu().numpy(), edge_phases(W, H, pitch)[:3], pitch)
            assert 4 * int((gold != 0).sum()) >= sx.size
            assert_adjoint_matches(gx[b].cpu().numpy()[sy, sx], gold, "autograd %dx%d mode %d image %d (%d source pixels)" % (W, H, mode, b, sx.size))
            total += sx.size
    assert total >= 2000
