"""Every launcher of csrc/ past what one grid carries, on the MI355X: images taller than 65535 row blocks (a second launch, a doubled row
block, a second grid stride) and batches past grid.z or past the 1 GiB scratch rule, for the kernel families that had no such test --
the transposed separable adjoint (fp32, interleaved, half), the planned adjoint at general rotations, the narrow-element direct kernel,
the converters of the forwarding routes, the wide kernel, the zero pass, and the batch loops of the narrow routes.  The geometries and
what each crosses are grid_carry_cases.GEOMETRIES; tests/test_grid_carry_host.py holds them to the planner and to the sources' constants.

No tolerance of its own: the oracle's bars are those of the family's existing tests (assert_adjoint_matches, conftest.TOL with rel_err,
half_cases.rounded_excess, int_cases.excess), the fp32 adjoint against the f64 entry is test_f64_gpu.py's 1e-6 max|ref|, and everything a
header promises bit for bit is compared bit for bit.  Every output starts as a sentinel (NaN bits; 0xA5 bytes for integers) and every
entitled element must have been written; aai_last_kernel() must name the kernel the test is about.

"Boundary rows" are grid_carry_cases.boundary_rows: 33 rows on both sides of the first carried row, and the first and last two rows."""
import numpy as np
import pytest

import adjoint_half_cases as ac
import axis_variants as av
import grid_carry_cases as gc
import half_cases as hc
import half_interleaved_cases as hic
import int_cases as ic
from adjoint_columns import comb_gold_pixels
from conftest import TOL, rel_err
from test_adjoint_gpu import _check_listed

pytestmark = pytest.mark.gpu

SENTINEL16 = 0x7fa5           # a NaN in both 16-bit float types that no arithmetic here produces
PATTERN = 0xA5                # every byte of an integer destination before the call
TNAME = dict((t, n) for t, n in hc.TYPES)


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    aai.set_device(0)
    return aai


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def to_dev(a):
    """a host array as raw bytes on the device (a torch uint8 tensor): keeps NaN payloads and 16-bit patterns as they are"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def to_host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def nan32(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def rand32(shape, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(shape, dtype=torch.float32, device="cuda", generator=gen)


def widened(raw, ht):
    """raw 16-bit elements (host, uint16) -> an fp32 device tensor of the same shape, widened exactly"""
    import torch
    return torch.from_numpy(hc.widen(raw, ht)).cuda()


def dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ---- 4. the transposed separable adjoint, tall ------------------------------------------------------------------------------------
def adjoint_half(gpu, rq, ht, g):
    """[dH, dW, C] raw bits through adjoint_half_device, gsrc prefilled with a sentinel -> ([H, W, C] raw bits, the kernel's name)"""
    import torch
    dH, dW, C = g.shape
    H, W = rq.src_height, rq.src_width
    gd, gs = to_dev(g), to_dev(np.full((H, W, C), SENTINEL16, np.uint16))
    gpu.adjoint_half_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, ht, stream=stream())
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    return to_host(gs, np.uint16, (H, W, C)), kernel


def adjoint_half_reference(gpu, rq, ht, g):
    """narrow(aai_adjoint_planned_interleaved_device_f32(widen(g))), narrowed on the host by the library's rounding helper"""
    import torch
    dH, dW, C = g.shape
    H, W = rq.src_height, rq.src_width
    g32 = widened(g, ht)
    s32 = nan32(H, W, C)
    gpu.adjoint_interleaved_device(rq, C, g32.data_ptr(), dW * C, s32.data_ptr(), W * C, stream(), planned="separable")
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    return hc.narrow(s32.cpu().numpy(), ht), kernel


def planned_single(gpu, rq, lay, gd):
    """adjoint_device(planned=True) on a dense [dH, dW] device gradient -> (gsrc prefilled with NaN, the kernel's name)"""
    import torch
    assert gd.shape == (lay.dst_height, lay.dst_width) and gd.is_contiguous()
    gs = nan32(rq.src_height, rq.src_width)
    gpu.adjoint_device(rq, gd.data_ptr(), lay.dst_width, gs.data_ptr(), rq.src_width, stream(), planned=True)
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    return gs, kernel


TALL_ADJOINT = [(name, route) for name in ("A0", "A180", "A90", "A11") for route in ("f32", "f32 x3", "half")] + [("A270", "f32"), ("A270", "half"), ("A0", "half, area replay")]


@pytest.mark.parametrize("name, route", TALL_ADJOINT, ids=["%s %s" % t for t in TALL_ADJOINT])
def test_separable_adjoint_taller_than_one_grid(gpu, po, name, route):
    """More than 65535 x 32 source rows: the second launch of launch_axis_adjoint (fp32, planned=True), launch_axis_adjoint_multi (C = 3,
    planned="separable") and launch_axis_adjoint_half_as (f16 with C = 1, bf16 with C = 4; A270: f16 alone).
    fp32: the boundary source rows against columns of the oracle's matrix, and EVERY element against the f64 entry (whose own carry
    test_image_taller_than_one_grid_carries holds to the oracle).  C = 3: channel c has the single-channel call's bits on plane c.
    half: the bits of narrow(fp32 entry(widen(g))) in both modes and, in fast mode, of the kernel's CPU replay, whole image.  The replay
    runs the planner's model check on the CPU: 1 to 2 s per call in fast mode; in area mode about 7 s for the five-column geometries and
    42 s for A11, so area mode has the replay's bits on A0 alone (f16, C = 1), in a case of its own."""
    import torch
    geo = gc.GEOMETRIES[name]
    W, H = geo.W, geo.H
    assert H > gc.EDGE_AXIS_ADJOINT + 33
    rq = gc.request(gpu, name, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    if route == "f32":
        gd = rand32((dH, dW), 4)
        gs, kernel = planned_single(gpu, rq, lay, gd)
        assert kernel == "aai_axis_adjoint_kernel", (kernel, gpu.plan_shape(rq))
        assert not bool(torch.isnan(gs).any())                                   # every row block of both launches wrote its rows
        sx, sy = gc.rows_pixels(W, gc.boundary_rows(gc.EDGE_AXIS_ADJOINT, H), 5)
        assert _check_listed(gpu, po, rq, lay, gd, gs, sx, sy, "tall separable %s" % name) == sx.size
        ref = torch.full((H, W), float("nan"), dtype=torch.float64, device="cuda")
        gd64 = gd.double()
        gpu.adjoint_device_f64(rq, gd64.data_ptr(), dW, ref.data_ptr(), W, stream())
        torch.cuda.synchronize()
        worst = float((ref - gs.double()).abs().max())
        print("%s: fp32 against f64, worst %.3e of max|ref| %.3e" % (name, worst, float(gs.abs().max())))
        assert worst <= 1e-6 * float(gs.abs().max()), (name, worst)
    elif route == "f32 x3":
        C = 3
        gd = rand32((dH, dW, C), 6)
        gs = nan32(H, W, C)
        gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, stream(), planned="separable")
        kernel = gpu.last_kernel()
        torch.cuda.synchronize()
        assert kernel == "aai_axis_adjoint_multi_kernel<%d>" % C, kernel
        assert not bool(torch.isnan(gs).any())
        for c in range(C):
            one, k1 = planned_single(gpu, rq, lay, gd[:, :, c].contiguous())
            assert k1 == "aai_axis_adjoint_kernel" and same_bits(gs[:, :, c], one), (name, c)
    elif route == "half, area replay":
        ht, C = hc.F16, 1
        g = ac.gradient_bits(lay, C, ht)
        got, kernel = adjoint_half(gpu, rq, ht, g)
        assert kernel == "aai_axis_adjoint_half_kernel<%s,%d>" % (TNAME[ht], C), kernel
        rep = ac.replay(rq, ht, g)
        differ = got != rep
        assert not differ.any(), (name, "area replay", int(differ.sum()), np.argwhere(differ)[:4].tolist())
    else:
        for mode in ("fast", "area"):
            rqm = gc.request(gpu, name, mode)
            for ht, C in ((hc.F16, 1), (hc.BF16, 4))[:1 if name == "A270" else 2]:
                if mode == "fast":
                    assert ac.serves_direct(gpu, rqm, C), (name, C)              # (not the class the engine forwards by measurement)
                g = ac.gradient_bits(lay, C, ht)
                got, kernel = adjoint_half(gpu, rqm, ht, g)
                assert kernel == "aai_axis_adjoint_half_kernel<%s,%d>" % (TNAME[ht], C), (name, mode, kernel)
                assert not (got == SENTINEL16).any()
                want, ref_kernel = adjoint_half_reference(gpu, rqm, ht, g)
                assert ref_kernel == ("aai_axis_adjoint_kernel" if C == 1 else "aai_axis_adjoint_multi_kernel<%d>" % C), ref_kernel
                differ = got != want
                assert not differ.any(), (name, mode, TNAME[ht], C, int(differ.sum()), np.argwhere(differ)[:4].tolist())
                if mode == "fast":
                    rep = ac.replay(rqm, ht, g)
                    differ = got != rep
                    assert not differ.any(), (name, "replay", TNAME[ht], C, int(differ.sum()), np.argwhere(differ)[:4].tolist())


# ---- 5. the planned adjoint at a general rotation, tall -----------------------------------------------------------------------------
def fed_source_rows(edge, H, dH):
    """the source rows that the dst rows around `edge` feed (the method of test_adjoint_taller_than_one_grid), with the first and last two"""
    c = int(edge * H / dH)
    return [r for r in sorted(set([0, 1, H - 2, H - 1]) | set(range(c - 17, c + 18))) if 0 <= r < H]


@pytest.mark.parametrize("name", ["R", "Rup"])
def test_planned_rotated_adjoint_taller_than_one_grid(gpu, po, name):
    """0.003 degrees: a canvas of 79 columns (at the 0.05 degrees of the older tall tests it is 939 columns wide), and the plan is served
    by the plain kernels (aai_adjoint_plain_gather_kernel, on R behind "+listed": 183 knife pairs; from 0.01 degrees on the plan falls
    back to the general kernels).  R: 1,048,700 source and dst rows -- launch_adjoint_sums (the call comes first on a fresh plan), the
    scale pass in five launches of 65535 blocks of 4 rows, the gather in two of 65535 tiles of 16.  Rup: 524,400 source rows up-sampled
    to 1,048,800, only the dst-side loops carry.  The same through launch_adjoint_plain_multi and launch_adjoint_multi with C = 2.
    planned="any" has the general adjoint's bits at EVERY element and channel c those of plane c (the headers' promise); the source rows
    on both sides of every carry against columns of the oracle's matrix."""
    import torch
    geo = gc.GEOMETRIES[name]
    W, H = geo.W, geo.H
    rq = gc.request(gpu, name, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    assert dH > gc.EDGE_PLAIN + 33 and (H > gc.EDGE_PLAIN + 33) == (name == "R")
    gpu.shutdown()                                                               # no cached plan: the sums are computed by this call
    assert gpu.plan_shape(rq) == ""
    gd = rand32((dH, dW), 4)
    runs = {}
    for planned in ("any", False, "any"):
        gs = nan32(H, W)
        gpu.adjoint_device(rq, gd.data_ptr(), dW, gs.data_ptr(), W, stream(), planned=planned)
        kernel = gpu.last_kernel()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(gs).any()), (name, planned)
        if planned == "any":
            assert kernel.startswith("aai_adjoint_plain_gather_kernel<area>") and "rot_adjoint=sums" in gpu.plan_shape(rq), (kernel, gpu.plan_shape(rq))
            assert "any" not in runs or same_bits(runs["any"], gs)                # the call that computed the sums and the one that found them
        else:
            assert kernel == "aai_adjoint_gather_kernel<area>", kernel
        runs[planned] = gs
    assert same_bits(runs["any"], runs[False]), name
    rows = set()
    for edge in (gc.GRID_Y * gc.SCALE_ROWS, gc.EDGE_PLAIN):
        rows |= set(fed_source_rows(edge, H, dH))
    if name == "R":
        rows |= set(gc.boundary_rows(gc.EDGE_PLAIN, H))                          # the gather's second launch
    sx, sy = gc.rows_pixels(W, sorted(rows), 5)
    assert sx.size >= 250                                                         # (two carries' worth of rows, at least four columns each)
    assert _check_listed(gpu, po, rq, lay, gd, runs["any"], sx, sy, "tall planned rotated %s" % name) == sx.size
    C = 2
    gdc = torch.stack([gd, rand32((dH, dW), 8)], dim=2).contiguous()
    single = [runs[False]]
    g1, plane1 = nan32(H, W), gdc[:, :, 1].contiguous()
    gpu.adjoint_device(rq, plane1.data_ptr(), dW, g1.data_ptr(), W, stream())
    torch.cuda.synchronize()
    single.append(g1)
    for planned, want in (("any", "aai_adjoint_plain_gather_multi_kernel<area, 2>"), (False, "aai_adjoint_gather_multi_kernel<area, 2>")):
        gsc = nan32(H, W, C)
        gpu.adjoint_interleaved_device(rq, C, gdc.data_ptr(), dW * C, gsc.data_ptr(), W * C, stream(), planned=planned)
        kernel = gpu.last_kernel()
        torch.cuda.synchronize()
        assert kernel.startswith(want), (planned, kernel)
        for c in range(C):
            assert same_bits(gsc[:, :, c], single[c]), (name, planned, c)
    torch.cuda.empty_cache()


# ---- 6. the narrow direct kernel with doubled rows ----------------------------------------------------------------------------------
def half_forward(gpu, rq, lay, ht, src):
    """[H, W, C] raw bits through resample_half_interleaved_device (C = 1: resample_half_device), dst prefilled with a sentinel"""
    import torch
    H, W, C = src.shape
    dW, dH = lay.dst_width, lay.dst_height
    x, y = to_dev(src), to_dev(np.full((dH, dW, C), SENTINEL16, np.uint16))
    if C == 1:
        gpu.resample_half_device(rq, x.data_ptr(), W, y.data_ptr(), dW, ht, stream=stream())
    else:
        gpu.resample_half_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C, ht, stream=stream())
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    out = to_host(y, np.uint16, (dH, dW, C))
    assert not (out == SENTINEL16).any(), "entitled elements not written"
    return out, kernel


def int_forward(gpu, rq, lay, dt, src):
    """[H, W, C] through resample_int_device, every byte of dst prefilled with PATTERN -> (dst, kernel, a second run prefilled with the
    complement: an element that neither run wrote differs between the two)"""
    import torch
    H, W, C = src.shape
    dW, dH = lay.dst_width, lay.dst_height
    x = to_dev(src)
    outs = []
    for fill in (PATTERN, PATTERN ^ 0xff):
        y = to_dev(np.full((dH, dW, C), fill, np.uint8).repeat(ic.NP[dt]().itemsize, axis=2))
        gpu.resample_int_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C, dt, stream=stream())
        kernel = gpu.last_kernel()
        torch.cuda.synchronize()
        outs.append(to_host(y, ic.NP[dt], (dH, dW, C)))
    assert np.array_equal(outs[0], outs[1]), "an entitled element kept the destination's bytes"
    return outs[0], kernel


def f32_forward(gpu, rq, lay, src32):
    """an fp32 device image [H, W] or [H, W, C] through the fp32 entry, dst prefilled with NaN"""
    import torch
    C = src32.shape[2] if src32.dim() == 3 else 1
    W = rq.src_width
    dW, dH = lay.dst_width, lay.dst_height
    y = nan32(*((dH, dW) + ((C,) if src32.dim() == 3 else ())))
    if src32.dim() == 3:
        gpu.resample_interleaved_device(rq, C, src32.data_ptr(), W * C, y.data_ptr(), dW * C, stream())
    else:
        gpu.resample_device(rq, src32.data_ptr(), W, y.data_ptr(), dW, stream())
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y).any()), "entitled elements not written"
    return y, kernel


def oracle_channels(po, omode, src32, geo, rows, dW):
    """the oracle at dst rows `rows` per channel of a float32 [H, W, C] host image -> [len(rows), dW, C]"""
    return np.stack([gc.oracle_at_rows(po, omode, np.ascontiguousarray(src32[:, :, c]), geo, rows, dW) for c in range(src32.shape[2])], axis=2)


# (geometry, element type, channels, rows doubled): N2 / N2r have 2-byte elements, N8 / N8c one byte.  N8 with three channels has 198
# elements in its strip, the class of 32 rows per workgroup: that case checks a direct launch of 16,388 row blocks in ONE grid, nothing
# doubled.  N8c (22 columns: 66 elements per strip) is the three-channel case whose rows ARE doubled.
DOUBLED = [("N2", "f16", 1, True), ("N2", "bf16", 1, True), ("N2", "u16", 1, True), ("N2r", "f16", 3, True), ("N2r", "u16", 3, True),
           ("N8", "u8", 1, True), ("N8", "u8", 3, False), ("N8c", "u8", 3, True)]


@pytest.mark.parametrize("name, tname, C, doubled", DOUBLED, ids=["%s %s x%d" % d[:3] for d in DOUBLED])
def test_narrow_direct_kernel_with_doubled_rows(gpu, po, hostemu, name, tname, C, doubled):
    """More output rows than 65535 row blocks of the launch shape's own size: axis_launch_shape doubles `rows` until one grid carries
    them (asserted through the variant probe against the same geometry at a tenth of the height).  The kernel's CPU replay, whole
    image, bit for bit; the boundary dst rows against the oracle by the bar of the type's own tests."""
    geo = gc.GEOMETRIES[name]
    rq = gc.request(gpu, name, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    rows = gc.forward_rows(dH)
    elem = 1 if tname == "u8" else 2
    probe = av.Prober(hostemu)
    shape = lambda H: probe(geo.W, H, geo.ratio, geo.angle, av.MODE_AREA, ((geo.W - 1) / 2.0, (H - 1) / 2.0), C, elem, 1)
    tall, short = shape(geo.H), shape(geo.H // 10)
    assert (tall.rows > short.rows) == doubled and tall.grid_y <= gc.GRID_Y and (tall.nB > gc.GRID_Y * short.rows) == doubled, (tall.rows, short.rows, tall.grid_y)
    if tname in ("f16", "bf16"):
        ht = hc.F16 if tname == "f16" else hc.BF16
        src = hic.source_bits((geo.W, geo.H), C, ht)
        got, kernel = half_forward(gpu, rq, lay, ht, src)
        assert kernel == "aai_axis_half_kernel<%s>" % tname, kernel
        want = (hc.replay(gpu, rq, ht, src[:, :, 0])[0][:, :, None] if C == 1 else hic.replay(gpu, rq, ht, src)[0])
        gold = oracle_channels(po, po.MODE_EXACT, hc.widen(src, ht), geo, rows, dW)
        over = hc.rounded_excess(hc.widen(got[rows], ht), gold, ht)
    else:
        dt = ic.U8 if tname == "u8" else ic.U16
        src = ic.source((geo.W, geo.H), C, dt, "random")
        assert ic.direct(rq, C, dt), ic.facts(rq, C)
        got, kernel = int_forward(gpu, rq, lay, dt, src)
        assert kernel == "aai_axis_int_kernel<%s>" % tname, kernel
        want = ic.replay(gpu, rq, dt, src)[0]
        gold = oracle_channels(po, po.MODE_EXACT, src.astype(np.float32), geo, rows, dW)
        over = ic.excess(got[rows], gold)
    differ = got != want
    assert not differ.any(), (name, tname, C, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    print("%s %s x%d: rows %d (a tenth of the height: %d), gridY %d; %.3e over the bound at %d boundary rows" % (name, tname, C, tall.rows, short.rows, tall.grid_y, over, len(rows)))
    assert over <= 0, (name, tname, C, over)


# ---- 7. the converters and the wide kernel, tall ------------------------------------------------------------------------------------
def test_wide_kernel_taller_than_one_launch(gpu, po):
    """Wd: 262,210 dst rows of two pixels, more than one launch of 65535 blocks of 4 rows carries (aai_axis.hip: kb0)"""
    geo = gc.GEOMETRIES["Wd"]
    for mode in hc.MODES:
        rq = gc.request(gpu, "Wd", mode)
        lay = gpu.query(rq)[2]
        src = po.synth_image(geo.W, geo.H, 3).astype(np.float32)
        y, kernel = f32_forward(gpu, rq, lay, dev32(src))
        assert kernel == "aai_axis_wide_kernel", kernel
        rows = gc.forward_rows(lay.dst_height)
        assert len(rows) >= 70
        got = y.cpu().numpy()[rows]
        gold = gc.oracle_at_rows(po, hc.oracle_mode(po, mode), src, geo, rows, lay.dst_width)
        err = float(rel_err(got, gold).max())
        print("Wd %s: max rel err %.3e at %d boundary rows" % (mode, err, len(rows)))
        assert err <= TOL and np.array_equal(got == 0, gold == 0), (mode, err)


FORWARDING = [("Wd", "bf16", 1), ("Wd", "u8", 1), ("Wd", "u8", 3), ("T", "bf16", 1)]


@pytest.mark.parametrize("name, tname, C", FORWARDING, ids=["%s %s x%d" % f for f in FORWARDING])
def test_forwarding_converters_taller_than_one_grid_stride(gpu, po, name, tname, C):
    """More than 65535 x 4 rows on a forwarding route: aai_narrow_widen_kernel and aai_narrow_store_kernel go round their grid-stride loop
    a second time.
    Wd: 524,420 source and 262,210 dst rows behind the wide kernel.  With three channels of u8 a row has 9 elements, so the store's
    one-by-one tail runs in the second stride too, behind aai_axis_kernel.  (A half image of three channels takes the direct kernel
    there; the half converters' tails are test_half_adjoint_forwarding_converters_taller_than_one_grid_stride's.)
    T: 262,300 rows on both sides of the rotated cell kernel.
    The bits of narrow(fp32 entry(widen(x))) / quantize(fp32 entry(x)) computed here, whole image; the boundary dst rows against the
    oracle by the bar of the type's own tests."""
    import torch
    geo = gc.GEOMETRIES[name]
    rq = gc.request(gpu, name, "area")
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    assert geo.H > gc.EDGE_ROWS4 + 33 and dH > gc.EDGE_ROWS4 + 33
    rows = gc.forward_rows(dH)
    if tname in ("f16", "bf16"):
        ht = hc.F16 if tname == "f16" else hc.BF16
        src = hic.source_bits((geo.W, geo.H), C, ht)
        got, kernel = half_forward(gpu, rq, lay, ht, src)
        x32 = widened(src if C > 1 else src[:, :, 0], ht)
        y32, fkernel = f32_forward(gpu, rq, lay, x32)
        assert kernel == fkernel + "+widened", (kernel, fkernel)
        want = hc.narrow(y32.cpu().numpy(), ht).reshape(dH, dW, C)
        gold = oracle_channels(po, po.MODE_EXACT, hc.widen(src, ht), geo, rows, dW)
        over = hc.rounded_excess(hc.widen(got[rows], ht), gold, ht)
    else:
        dt = ic.U8
        src = ic.source((geo.W, geo.H), C, dt, "random")
        got, kernel = int_forward(gpu, rq, lay, dt, src)
        y32 = nan32(dH, dW, C)
        x = to_dev(src)
        gpu.resample_interleaved_device(rq, C, x.data_ptr(), geo.W * C, y32.data_ptr(), dW * C, stream(), src_dtype=dt)
        fkernel = gpu.last_kernel()
        torch.cuda.synchronize()
        assert kernel == fkernel + "+quantized", (kernel, fkernel)
        want = ic.quantize(y32.cpu().numpy(), dt)
        gold = oracle_channels(po, po.MODE_EXACT, src.astype(np.float32), geo, rows, dW)
        over = ic.excess(got[rows], gold)
    assert fkernel == {("Wd", 1): "aai_axis_wide_kernel", ("Wd", 3): "aai_axis_kernel", ("T", 1): "aai_cell_kernel<area>"}[name, C], fkernel
    differ = got != want
    assert not differ.any(), (name, tname, C, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    print("%s %s x%d (%s): %.3e over the bound at %d boundary rows" % (name, tname, C, kernel, over, len(rows)))
    assert over <= 0, (name, tname, C, over)


@pytest.mark.parametrize("ht, tname", hc.TYPES, ids=[t[1] for t in hc.TYPES])
def test_half_adjoint_forwarding_converters_taller_than_one_grid_stride(gpu, po, ht, tname):
    """adjoint_half_device on Wd (a wide plan forwards): gdst of 262,210 rows widened, gsrc of 524,420 rows stored, rows of 2 and 3 elements
    (6 and 9 with three channels) -- the converters' tail branch, over two strides.  The bits of narrow(fp32 entry(widen(g))); the source
    rows on both sides of the second stride against columns of the oracle's matrix, one rounding on top of the bar."""
    geo = gc.GEOMETRIES["Wd"]
    rq = gc.request(gpu, "Wd", "area")
    lay = gpu.query(rq)[2]
    for C in (1, 3):
        g = ac.gradient_bits(lay, C, ht, seed=31)
        got, kernel = adjoint_half(gpu, rq, ht, g)
        assert not (got == SENTINEL16).any()
        want, ref_kernel = adjoint_half_reference(gpu, rq, ht, g)
        assert kernel == ref_kernel + "+widened" and "aai_adjoint_gather" in kernel, (kernel, ref_kernel)
        differ = got != want
        assert not differ.any(), (tname, C, int(differ.sum()), np.argwhere(differ)[:4].tolist())
        if C == 1:
            sx, sy = gc.rows_pixels(geo.W, gc.boundary_rows(gc.EDGE_ROWS4, geo.H), 5)
            g32 = hc.widen(g[:, :, 0], ht)
            gold, evaluated = comb_gold_pixels(po, po.MODE_EXACT, rq, lay, lambda dx, dy: g32[dy, dx], sx, sy)
            over = hc.rounded_excess(hc.widen(got[sy, sx, 0], ht), gold, ht)
            print("Wd half adjoint %s: %.3e over the bound at %d source pixels (%d oracle dst pixels)" % (tname, over, sx.size, evaluated))
            assert 4 * int((gold != 0).sum()) >= sx.size and over <= 0, (tname, over)
            assert np.all(got[sy, sx, 0][gold == 0] == 0)


# ---- 8. the zero pass at height -------------------------------------------------------------------------------------------------------
def test_zero_pass_taller_than_one_grid_stride(gpu, po):
    """Z: 7 x 524,420 at 2:1 with the isocenter half a pixel right of the centre -- the canvas is one column wider than the image's
    footprint, the lane table's last entry is empty, and aai_axis_zero_kernel writes that dst column over 262,210 rows: its grid
    carries 65535 blocks of 4 rows, the rest is its grid-stride loop.
    K1 itself stores the empty entry as (its neighbour's window) x weights of 0, which is already +0 for a finite source, so the pass
    shows only on a source that is not finite: with NaN in the upper half of the source and +Inf in the lower, K1 leaves NaN in the
    empty column of every row, and only the zero pass makes it +0.  That run: +0 bits in the empty column of EVERY row, every other
    element non-finite.  The finite run: every element written, the boundary rows against the oracle."""
    import torch
    geo = gc.GEOMETRIES["Z"]
    for mode in hc.MODES:
        rq = gc.request(gpu, "Z", mode)
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        assert dH > gc.EDGE_ROWS4 + 33
        src = 0.25 + po.synth_image(geo.W, geo.H, 5).astype(np.float32)            # no zero in the source: a zero in dst is an empty window
        y, kernel = f32_forward(gpu, rq, lay, dev32(src))
        assert kernel == "aai_axis_kernel", kernel
        assert bool((bits(y[:, dW - 1]) == 0).all()), "the empty column is not +0 in every row"
        assert bool((y[:, :dW - 1] > 0).all())
        rows = gc.forward_rows(dH)
        got = y.cpu().numpy()[rows]
        gold = gc.oracle_at_rows(po, hc.oracle_mode(po, mode), src, geo, rows, dW)
        err = float(rel_err(got, gold).max())
        print("Z %s: max rel err %.3e at %d boundary rows" % (mode, err, len(rows)))
        assert not gold[:, dW - 1].any() and err <= TOL and np.array_equal(got == 0, gold == 0), (mode, err)
        # the source that shows the pass (dst prefilled with a finite value, so that a row nobody wrote shows as well)
        bad = torch.full((geo.H, geo.W), float("nan"), dtype=torch.float32, device="cuda")
        bad[geo.H // 2:] = float("inf")
        y = torch.full((dH, dW), -7.0, dtype=torch.float32, device="cuda")
        gpu.resample_device(rq, bad.data_ptr(), geo.W, y.data_ptr(), dW, stream())
        assert gpu.last_kernel() == "aai_axis_kernel", gpu.last_kernel()
        torch.cuda.synchronize()
        wrong = torch.nonzero(bits(y[:, dW - 1]) != 0).flatten()
        assert wrong.numel() == 0, ("%d rows of the empty column are not +0, first %s" % (wrong.numel(), wrong[:4].tolist()), mode)
        assert not bool(torch.isfinite(y[:, :dW - 1]).any()), mode


# ---- 9. batches through the forwarding routes and the half adjoint -----------------------------------------------------------------
H_CASE = hc.CASES["h"]                     # 5 x 7 at 2:1: the narrowest image the strip form serves
GOLDEN_IMAGES = (0, 1, 65534, 65535, 65536)


class Route:
    """one narrow-element entry on dense batches: elements of `np_dtype`, C channels; run(x, y, batch) enqueues on device byte tensors"""

    def __init__(self, gpu, name, rq, C, adjoint):
        self.gpu, self.name, self.rq, self.C, self.adjoint = gpu, name, rq, C, adjoint
        lay = gpu.query(rq)[2]
        src_shape, dst_shape = (rq.src_height, rq.src_width, C), (lay.dst_height, lay.dst_width, C)
        self.in_shape, self.out_shape = (dst_shape, src_shape) if adjoint else (src_shape, dst_shape)      # the adjoint reads gdst, writes gsrc
        self.lay = lay

    def inputs(self, batch, seed):
        raise NotImplementedError

    def call(self, x_ptr, in_stride, in_image, y_ptr, out_stride, out_image, batch):
        raise NotImplementedError

    def dense(self, x, y, batch):
        import torch
        n_in, n_out = int(np.prod(self.in_shape)), int(np.prod(self.out_shape))
        self.call(x.data_ptr(), self.in_shape[1] * self.C, n_in, y.data_ptr(), self.out_shape[1] * self.C, n_out, batch)
        kernel = self.gpu.last_kernel()
        torch.cuda.synchronize()
        return kernel


class HalfRoute(Route):
    np_dtype, fill, ht = np.uint16, SENTINEL16, hc.BF16

    def inputs(self, batch, seed):
        rng = np.random.default_rng(seed)
        return hc.narrow((0.25 + rng.random((batch,) + self.in_shape, dtype=np.float32)), self.ht)

    def call(self, x_ptr, in_stride, in_image, y_ptr, out_stride, out_image, batch):
        if self.adjoint:
            self.gpu.adjoint_half_device(self.rq, self.C, x_ptr, in_stride, y_ptr, out_stride, self.ht, stream=stream(), batch=batch,
                                         dst_image_stride=in_image, src_image_stride=out_image)
        else:
            assert self.C == 1
            self.gpu.resample_half_device(self.rq, x_ptr, in_stride, y_ptr, out_stride, self.ht, stream=stream(), batch=batch,
                                          src_image_stride=in_image, dst_image_stride=out_image)

    def gold(self, x_bits):
        """narrow(fp32 entry(widen(x))) of one image, computed here"""
        import torch
        x32 = widened(x_bits, self.ht)
        y32 = nan32(*self.out_shape)
        H, W, dH, dW, C = self.rq.src_height, self.rq.src_width, self.lay.dst_height, self.lay.dst_width, self.C
        if self.adjoint:
            self.gpu.adjoint_interleaved_device(self.rq, C, x32.data_ptr(), dW * C, y32.data_ptr(), W * C, stream(), planned="separable")
        else:
            self.gpu.resample_device(self.rq, x32.data_ptr(), W, y32.data_ptr(), dW, stream())
        torch.cuda.synchronize()
        return hc.narrow(y32.cpu().numpy(), self.ht)


class IntRoute(Route):
    np_dtype, fill, dt = np.uint8, PATTERN, ic.U8

    def inputs(self, batch, seed):
        return np.random.default_rng(seed).integers(0, 256, size=(batch,) + self.in_shape).astype(np.uint8)

    def call(self, x_ptr, in_stride, in_image, y_ptr, out_stride, out_image, batch):
        self.gpu.resample_int_device(self.rq, self.C, x_ptr, in_stride, y_ptr, out_stride, self.dt, stream=stream(), batch=batch,
                                     src_image_stride=in_image, dst_image_stride=out_image)

    def gold(self, x):
        """quantize(fp32 entry(x)) of one image, computed here"""
        import torch
        H, W, dH, dW, C = self.rq.src_height, self.rq.src_width, self.lay.dst_height, self.lay.dst_width, self.C
        xd = to_dev(x)
        y32 = nan32(*self.out_shape)
        self.gpu.resample_interleaved_device(self.rq, C, xd.data_ptr(), W * C, y32.data_ptr(), dW * C, stream(), src_dtype=self.dt)
        torch.cuda.synchronize()
        return ic.quantize(y32.cpu().numpy(), self.dt)


def route_of(gpu, name, geom, small):
    """(the route on this geometry, what aai_last_kernel() must say).  small (geometry h): the half forward forwards at 90 degrees and the
    u8 forward at 0 degrees (at most 64 outputs per strip); otherwise both run at 17.5 degrees.  The half adjoint forwards at 17.5."""
    W, H, sr, dr, iso = geom[:5]
    rq = lambda a: gpu.make_request(W, H, sr, dr, iso, a, mode=gpu.MODE_AREA)
    if name == "half adjoint, direct":
        return HalfRoute(gpu, name, rq(0.0), 1, True), "aai_axis_adjoint_half_kernel<bf16,1>"
    if name == "half adjoint, forwarding":
        return HalfRoute(gpu, name, rq(17.5), 1, True), "+widened"
    if name == "half forward, forwarding":
        return HalfRoute(gpu, name, rq(90.0 if small else 17.5), 1, False), "+widened"
    assert name == "u8 forward, forwarding", name
    return IntRoute(gpu, name, rq(0.0 if small else 17.5), 1, False), "+quantized"


ROUTES = ["half adjoint, direct", "half adjoint, forwarding", "half forward, forwarding", "u8 forward, forwarding"]


def run_batch(route, x_host, batch):
    x = to_dev(x_host)
    y = to_dev(np.full((batch,) + route.out_shape, route.fill, route.np_dtype))
    kernel = route.dense(x, y, batch)
    return to_host(y, route.np_dtype, (batch,) + route.out_shape), kernel


@pytest.mark.parametrize("name", ROUTES)
def test_narrow_routes_batch_beyond_grid_z(gpu, name):
    """65,538 images of 5 x 7: grid.z carries 65,535, so the direct half adjoint goes in two launches (aai_engine.cpp, enqueue_adjoint_half) and
    the forwarding routes in two chunks of widen / fp32 entry / store.  Images 0, 1, 65534, 65535, 65536 and the last equal their single
    calls bit for bit, and a permuted batch permutes the results: every image of both launches is the right one."""
    B = gc.GRID_Y + 3
    route, kernel_part = route_of(gpu, name, H_CASE, True)
    assert gc.chunk_images(B, gc.round256(4 * int(np.prod(route.in_shape))) + gc.round256(4 * int(np.prod(route.out_shape)))) == gc.GRID_Y
    x = route.inputs(B, 9)
    got, kernel = run_batch(route, x, B)
    assert (kernel == kernel_part) if not kernel_part.startswith("+") else (kernel.endswith(kernel_part) and "half_kernel" not in kernel and "int_kernel" not in kernel), kernel
    if route.fill == SENTINEL16:
        assert not (got == SENTINEL16).any()
    for b in GOLDEN_IMAGES + (B - 1,):
        one, k1 = run_batch(route, x[b:b + 1], 1)
        assert k1 == kernel and np.array_equal(got[b], one[0]), (name, b)
    perm = np.random.default_rng(10).permutation(B)
    got2, _ = run_batch(route, x[perm], B)
    assert np.array_equal(got2, got[perm]), name


CHUNKED = ["half forward, forwarding", "u8 forward, forwarding", "half adjoint, forwarding"]
BIG = (1024, 1024, 1, 1, (511.5, 511.5))         # at 17.5 degrees: megabytes of fp32 scratch per image in flight


@pytest.mark.parametrize("name", CHUNKED)
def test_narrow_forwarding_routes_batch_of_two_scratch_chunks(gpu, name):
    """1024 x 1024 at 17.5 degrees: the fp32 scratch of one image in flight (the widened input and the fp32 output, each rounded up to
    256 bytes; the integer route widens nothing) allows fewer images per chunk than the batch has, by chunk_images' arithmetic restated
    in grid_carry_cases.chunk_images: 1 < chunk < batch = chunk + 3.  EVERY image equals its single call; the images on both sides of
    the cut equal narrow(fp32 entry(widen(x))) / quantize(fp32 entry(x)) computed here.  The half forward runs in guarded buffers:
    padded odd row strides, gaps between the images, bases one element past a 256-byte boundary, NaN in the source padding and a
    sentinel everywhere in dst -- a chunk pointer off by an image lands in padding."""
    import torch
    route, kernel_part = route_of(gpu, name, BIG, False)
    n_in, n_out = int(np.prod(route.in_shape)), int(np.prod(route.out_shape))
    per_image = (gc.round256(4 * n_in) if isinstance(route, HalfRoute) else 0) + gc.round256(4 * n_out)
    batch = (1 << 30) // per_image + 3
    chunk = gc.chunk_images(batch, per_image)
    assert 1 < chunk < batch and chunk == batch - 3, (chunk, batch)
    esz = np.dtype(route.np_dtype).itemsize
    guarded = name == "half forward, forwarding"
    # layouts: dense, or padded rows and gaps inside margins of 1024 elements
    def layout(shape):
        rows, row = shape[0], shape[1] * shape[2]
        if not guarded:
            return row, rows * row, 0, batch * rows * row
        stride = (row + 5) | 1
        image = rows * stride + 37
        lead = 1024 + 128 + 1                                                   # one element past a 256-byte boundary
        return stride, image, lead, lead + batch * image + 1024

    (istride, iimage, ilead, itotal), (ostride, oimage, olead, ototal) = layout(route.in_shape), layout(route.out_shape)
    tdt = torch.int16 if esz == 2 else torch.uint8
    fill_in = 0x7fc0 if esz == 2 else 0                                          # (bf16 NaN in the padding a call must not read)
    xbuf = torch.full((itotal,), fill_in, dtype=tdt, device="cuda")
    ybuf = torch.full((ototal,), route.fill, dtype=tdt, device="cuda")

    def view(buf, lead, image, stride, shape):
        rows, row = shape[0], shape[1] * shape[2]
        return buf[lead:lead + batch * image].view(batch, image)[:, :rows * stride].view(batch, rows, stride)[:, :, :row]

    xin, yout = view(xbuf, ilead, iimage, istride, route.in_shape), view(ybuf, olead, oimage, ostride, route.out_shape)
    gen = torch.Generator(device="cuda").manual_seed(12)
    if esz == 2:
        vals = (0.25 + torch.rand(xin.shape, dtype=torch.float32, device="cuda", generator=gen)).bfloat16().view(torch.int16)
    else:
        vals = torch.randint(0, 256, xin.shape, dtype=torch.uint8, device="cuda", generator=gen)
    xin.copy_(vals)
    del vals
    if guarded:
        assert (xbuf.data_ptr() + ilead * esz) % 256 == esz and (ybuf.data_ptr() + olead * esz) % 256 == esz
    route.call(xbuf.data_ptr() + ilead * esz, istride, iimage, ybuf.data_ptr() + olead * esz, ostride, oimage, batch)
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    assert kernel.endswith(kernel_part), kernel
    got = yout.clone()
    if esz == 2:
        assert not bool((got == SENTINEL16).any()), "entitled elements not written"
    # every image against its single call (dense buffers)
    one = torch.empty(route.out_shape, dtype=tdt, device="cuda").view(-1)
    for b in range(batch):
        xi = xin[b].contiguous()
        one.fill_(PATTERN if esz == 1 else SENTINEL16)
        route.call(xi.data_ptr(), route.in_shape[1] * route.C, n_in, one.data_ptr(), route.out_shape[1] * route.C, n_out, 1)
        torch.cuda.synchronize()
        assert bool(torch.equal(got[b].reshape(-1), one)), (name, b, chunk)
    for b in (chunk - 1, chunk, batch - 1):
        x_host = xin[b].contiguous().cpu().numpy().view(route.np_dtype).reshape(route.in_shape)
        want = route.gold(x_host)
        assert np.array_equal(got[b].cpu().numpy().view(route.np_dtype).reshape(route.out_shape), want), (name, b)
    if guarded:
        # nothing outside the entitled elements was written: with those put back to the sentinel the whole allocation is the sentinel
        yout.fill_(SENTINEL16)
        assert bool((ybuf == SENTINEL16).all()), "dst padding, a gap or a margin was written"
    del xbuf, ybuf, got
    torch.cuda.empty_cache()
