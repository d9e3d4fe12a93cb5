"""The reference-precision path on the MI355X (include/aai_f64.h): forward dst = W src and adjoint gsrc = W^T gdst on double images.

Parity with the two bars of tests/test_f64_host.py -- F64_TOL against the oracle on wide-range data, F64_GOLDEN_TOL against the arrays the
UNMODIFIED reference recorded -- both below what one fp32 rounding costs, so no wrapper around the fp32 entries passes.  Then the
element-wise transpose (one batched forward and one batched adjoint call on unit impulses), the host entries, batches with padded
strides and gaps, more images than grid.z carries, more tile rows than grid.y carries, non-finite source pixels, the stream-order
contract without a host wait, and a stream capture of both calls on a geometry nothing has seen before."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_err
from adjoint_columns import comb_cases, comb_pitch
from test_adjoint_host import EIGHT, corner_phases
from test_f64_host import (F64_GOLDEN_TOL, F64_TOL, SINGLES, THREE, check_adjoint_wide, check_forward_wide, eight_case, f64_measure, forward_gold,
                           golden_sweep, modes_of, transpose_check, wide_range)

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


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


def _forward(gpu, rq, src):
    """aai_resample_batch_device_f64 on a host image; dst prefilled with -1, and every element must have been written (no image used
    here holds a result of exactly -1)"""
    import torch
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    s = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float64)).cuda()
    d = torch.full((lay.dst_height, lay.dst_width), -1.0, dtype=torch.float64, device="cuda")
    gpu.resample_device_f64(rq, s.data_ptr(), rq.src_width, d.data_ptr(), lay.dst_width, _stream(), batch=1)
    torch.cuda.synchronize()
    assert "aai_f64_forward_kernel" in gpu.last_kernel()
    out = d.cpu().numpy()
    assert not (out == -1.0).any(), "dst elements were not written"
    return out


def _adjoint(gpu, rq, g):
    """aai_adjoint_batch_device_f64 on a host gradient image; gsrc prefilled with -1"""
    import torch
    gd = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float64)).cuda()
    gs = torch.full((rq.src_height, rq.src_width), -1.0, dtype=torch.float64, device="cuda")
    gpu.adjoint_device_f64(rq, gd.data_ptr(), gd.shape[1], gs.data_ptr(), rq.src_width, _stream(), batch=1)
    torch.cuda.synchronize()
    assert "aai_f64_adjoint_gather_kernel" in gpu.last_kernel()
    out = gs.cpu().numpy()
    assert not (out == -1.0).any(), "gsrc elements were not written"
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("case", range(len(EIGHT)))
def test_forward_and_adjoint_match_the_oracle(gpu, po, case):
    """EIGHT x {area, area with POLICY_EXACT, fast} on wide-range data; the host entries give the device entries' bits"""
    fwd, adj = (lambda rq, s: _forward(gpu, rq, s)), (lambda rq, g: _adjoint(gpu, rq, g))
    for name, policy in THREE:
        rq, geom = eight_case(gpu, case, name, policy)
        omode = modes_of(gpu, po, name)[1]
        check_forward_wide(po, fwd, rq, geom, omode, policy, "case %d %s policy %d" % (case, name, policy))
        check_adjoint_wide(po, gpu, adj, rq, geom, omode, policy, "case %d %s policy %d" % (case, name, policy))
        W, H, sr, dr, iso, ang = geom
        src = wide_range((H, W), 21)
        rc, msg, dst, diso, lay = gpu.resample_exact_host(src, sr, dr, iso, ang, mode=rq.mode, policy=policy)
        assert rc == 0 and dst.dtype == np.float64, msg
        assert "aai_f64_forward_kernel" in gpu.last_kernel()
        qlay = gpu.query(rq)[2]
        assert (diso, lay.dst_width, lay.dst_height, lay.kernel) == ((qlay.dst_iso_x, qlay.dst_iso_y), qlay.dst_width, qlay.dst_height, qlay.kernel)
        assert np.array_equal(_bits(dst), _bits(_forward(gpu, rq, src))), (case, name, policy)
        g = wide_range(dst.shape, 22)
        rc, msg, gsrc = gpu.adjoint_exact_host(g, (H, W), sr, dr, iso, ang, mode=rq.mode, policy=policy)
        assert rc == 0 and gsrc.dtype == np.float64, msg
        assert np.array_equal(_bits(gsrc), _bits(_adjoint(gpu, rq, g))), (case, name, policy)
    # the class with exact=True is the host entry
    W, H, sr, dr, ang, off = EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    src = wide_range((H, W), 23)
    cls = gpu.AreaAverageInterpolation(exact=True)
    for method, mode in ((cls.areaAverageInterpolation, gpu.MODE_AREA), (cls.fastAreaAverageInterpolation, gpu.MODE_FAST)):
        status, dst, diso = method(src, sr, dr, iso, ang)
        assert status == (True, "") and dst.dtype == np.float64
        assert np.array_equal(_bits(dst), _bits(_forward(gpu, gpu.make_request(W, H, sr, dr, iso, ang, mode=mode), src)))
    status, dst, diso = cls.bilinearInterpolation(src.astype(np.float32), sr, dr, iso, ang)
    assert status == (True, "") and dst.dtype == np.float32             # the sampler methods are unchanged


def test_forward_on_the_small_geometries_against_the_recorded_arrays(gpu, po, small_golden):
    """all 140 reference-generated geometries, both modes, against the UNMODIFIED reference's float64 outputs on its [0, 1) source"""
    z, manifest = small_golden
    worst = 0.0
    for i, c in enumerate(manifest):
        src = np.asarray(po.synth_image(c["W"], c["H"], c["seed"]), np.float64)
        for name, tag in (("area", "exact"), ("fast", "fast")):
            rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=modes_of(gpu, po, name)[0])
            got, gold = _forward(gpu, rq, src), z["c%03d_%s" % (i, tag)]
            assert got.shape == gold.shape, (i, tag)
            err = float(rel_err(got, gold).max())
            worst = max(worst, err)
            assert err <= F64_GOLDEN_TOL, (i, tag, err)
            assert np.array_equal(gold == 0, got == 0), (i, tag)
    print("small_cases against the recorded arrays: worst %.3e" % worst)


def _manifest(name):
    z = np.load(os.path.join(GOLDEN, name))
    return json.loads(bytes(z["manifest"]).decode())


# the knife-edge sweeps in blocks of four visited geometries (the adjoint's gold is the oracle's matrix, W H oracle runs per geometry):
# (file, stride, first visit of the block)
KNIFE_BLOCK = 4
KNIFE_SWEEPS = [(f, s, k) for f, s in (("knife_cases.npz", 4), ("axis_knife_cases.npz", 12))
                for k in range(0, len(range(0, len(_manifest(f)), s)), KNIFE_BLOCK)]


@pytest.mark.parametrize("sweep", KNIFE_SWEEPS, ids=lambda s: "%s-%d" % (s[0].split("_cases")[0], s[2]))
def test_forward_and_adjoint_on_knife_edge_geometries(gpu, po, sweep):
    """knife_cases at stride 4 and axis_knife_cases at stride 12 by index, both modes, wide-range data"""
    name, stride, first = sweep
    manifest = _manifest(name)
    visits = list(range(0, len(manifest), stride))
    assert len(visits) >= 45
    ran, ran_adj, _, _ = golden_sweep(gpu, po, manifest, visits[first:first + KNIFE_BLOCK], name, lambda rq, s: _forward(gpu, rq, s),
                                      lambda rq, g: _adjoint(gpu, rq, g))
    assert ran == len(visits[first:first + KNIFE_BLOCK])


@pytest.mark.parametrize("case", SINGLES, ids=lambda c: c[0])
def test_forward_and_adjoint_at_larger_sizes(gpu, po, case):
    """more than one workgroup, partial last workgroups, 40:1 footprints, near-axis angles, an isocenter far outside the image: the
    forward against the oracle, the adjoint per source pixel against columns of the oracle's matrix taken from comb images
    (tests/adjoint_columns.py), both on wide-range data"""
    name, W, H, sr, dr, ang, off = case
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mname in ("area", "fast"):
        mode, omode = modes_of(gpu, po, mname)
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
        check_forward_wide(po, lambda rq, s: _forward(gpu, rq, s), rq, (W, H, sr, dr, iso, ang), omode, 0, "%s %s" % (name, mname))
        lay = gpu.query(rq)[2]
        g = wide_range((lay.dst_height, lay.dst_width), 11)
        pitch = comb_pitch(lay, ang)
        phases = corner_phases(W, H, pitch, 2)
        sx, sy, gold = comb_cases(po, omode, W, H, sr, dr, iso, ang, 0, g, phases, pitch)
        _, _, scale = comb_cases(po, omode, W, H, sr, dr, iso, ang, 0, np.abs(g), phases, pitch)
        assert (sx == 0).any() and (sy == 0).any() and (sx == W - 1).any() and (sy == H - 1).any()
        worst = f64_measure(_adjoint(gpu, rq, g)[sy, sx], gold, scale, "%s %s adjoint" % (name, mname))
        print("%s %s: adjoint worst %.3e over %d source pixels" % (name, mname, worst, sx.size))
        assert worst <= F64_TOL, (name, mname, worst)


@pytest.mark.parametrize("case", range(len(EIGHT)))
def test_forward_and_adjoint_are_transposes_element_by_element(gpu, case):
    """A from ONE batched forward call on the W H impulse images, B from ONE batched adjoint call on the dW dH impulses"""
    import torch

    def fcols(rq, lay):
        W, H, n = rq.src_width, rq.src_height, lay.dst_width * lay.dst_height
        src = torch.eye(W * H, dtype=torch.float64, device="cuda").view(W * H, H, W).contiguous()
        dst = torch.full((W * H, lay.dst_height, lay.dst_width), -1.0, dtype=torch.float64, device="cuda")
        gpu.resample_device_f64(rq, src.data_ptr(), W, dst.data_ptr(), lay.dst_width, _stream(), batch=W * H, src_image_stride=W * H, dst_image_stride=n)
        torch.cuda.synchronize()
        return dst.view(W * H, n).t().cpu().numpy()

    def acols(rq, lay):
        W, H, n = rq.src_width, rq.src_height, lay.dst_width * lay.dst_height
        g = torch.eye(n, dtype=torch.float64, device="cuda").view(n, lay.dst_height, lay.dst_width).contiguous()
        gs = torch.full((n, H, W), -1.0, dtype=torch.float64, device="cuda")
        gpu.adjoint_device_f64(rq, g.data_ptr(), lay.dst_width, gs.data_ptr(), W, _stream(), batch=n, dst_image_stride=n, src_image_stride=W * H)
        torch.cuda.synchronize()
        return gs.view(n, W * H).t().cpu().numpy()
    for name in ("area", "fast"):
        transpose_check(gpu, fcols, acols, case, name, "transpose case %d %s" % (case, name))


def _padded(torch, images, stride, image_stride, fill):
    """B dense [h, w] images laid out with a row stride and an image stride, everything else `fill`; returns (flat tensor, mask of the
    entitled elements)"""
    B, h, w = images.shape
    flat = torch.full((B * image_stride,), fill, dtype=torch.float64, device="cuda")
    mask = torch.zeros(B * image_stride, dtype=torch.bool, device="cuda")
    for b in range(B):
        flat[b * image_stride:b * image_stride + stride * h].view(h, stride)[:, :w] = images[b]
        mask[b * image_stride:b * image_stride + stride * h].view(h, stride)[:, :w] = True
    return flat, mask


@pytest.mark.parametrize("mode_name", ["area", "fast"])
def test_padded_batch_of_three(gpu, mode_name):
    """B = 3 with padded strides and gaps between the images: NaN in the input's padding and gaps is never read, the sentinel in the
    output's padding and gaps keeps its bits, each image has its single-image bits, and a second run is bit-identical"""
    import torch
    W, H, sr, dr, ang = 37, 29, 3.0, 1.0, 17.5
    rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=gpu.MODE_FAST if mode_name == "fast" else gpu.MODE_AREA)
    lay = gpu.query(rq)[2]
    dW, dH, B = lay.dst_width, lay.dst_height, 3
    sstride, dstride = W + 5, dW + 3
    simg, dimg = sstride * H + 11, dstride * dH + 17
    src = wide_range((B, H, W), 31)
    g = wide_range((B, dH, dW), 32)
    single_f = [_forward(gpu, rq, src[b]) for b in range(B)]
    single_a = [_adjoint(gpu, rq, g[b]) for b in range(B)]
    sent_bits = int(np.float64(SENTINEL).view(np.int64))
    for what, data, single, in_stride, in_img, out_stride, out_img, (oh, ow) in (
            ("forward", src, single_f, sstride, simg, dstride, dimg, (dH, dW)), ("adjoint", g, single_a, dstride, dimg, sstride, simg, (H, W))):
        inp, _ = _padded(torch, torch.from_numpy(data).cuda(), in_stride, in_img, float("nan"))
        runs = []
        for _ in range(2):
            out = torch.full((B * out_img,), SENTINEL, dtype=torch.float64, device="cuda")
            if what == "forward":
                gpu.resample_device_f64(rq, inp.data_ptr(), in_stride, out.data_ptr(), out_stride, _stream(), batch=B, src_image_stride=in_img,
                                        dst_image_stride=out_img)
            else:
                gpu.adjoint_device_f64(rq, inp.data_ptr(), in_stride, out.data_ptr(), out_stride, _stream(), batch=B, dst_image_stride=in_img,
                                       src_image_stride=out_img)
            torch.cuda.synchronize()
            runs.append(out)
        _, mask = _padded(torch, torch.zeros((B, oh, ow), dtype=torch.float64, device="cuda"), out_stride, out_img, 0.0)
        out = runs[0]
        assert torch.equal(out.view(torch.int64), runs[1].view(torch.int64)), what
        assert bool((out[~mask].view(torch.int64) == sent_bits).all()), (what, "padding or gap overwritten")
        assert not bool(out[mask].isnan().any()), (what, "padding was read")
        for b in range(B):
            got = out[b * out_img:b * out_img + out_stride * oh].view(oh, out_stride)[:, :ow].cpu().numpy()
            assert np.array_equal(_bits(got), _bits(single[b])), (what, b)


def test_batch_of_more_images_than_one_grid_carries(gpu):
    """65,537 images of 6 x 5 at 2:1 and 30 degrees: the first, the last and image 65,535 (the first of the second launch) have their
    single-image bits, forward and adjoint"""
    import torch
    W, H, B = 6, 5, 65537
    rq = gpu.make_request(W, H, 2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 30.0)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    gen = torch.Generator(device="cuda").manual_seed(5)
    src = torch.randn((B, H, W), dtype=torch.float64, device="cuda", generator=gen)
    dst = torch.full((B, dH, dW), -1.0, dtype=torch.float64, device="cuda")
    gpu.resample_device_f64(rq, src.data_ptr(), W, dst.data_ptr(), dW, _stream(), batch=B, src_image_stride=W * H, dst_image_stride=dW * dH)
    g = torch.randn((B, dH, dW), dtype=torch.float64, device="cuda", generator=gen)
    gs = torch.full((B, H, W), -1.0, dtype=torch.float64, device="cuda")
    gpu.adjoint_device_f64(rq, g.data_ptr(), dW, gs.data_ptr(), W, _stream(), batch=B, dst_image_stride=dW * dH, src_image_stride=W * H)
    torch.cuda.synchronize()
    for b in (0, 65535, B - 1):
        assert np.array_equal(_bits(dst[b].cpu().numpy()), _bits(_forward(gpu, rq, src[b].cpu().numpy()))), b
        assert np.array_equal(_bits(gs[b].cpu().numpy()), _bits(_adjoint(gpu, rq, g[b].cpu().numpy()))), b
    assert not bool((dst == -1.0).any()) and not bool((gs == -1.0).any())


def test_image_taller_than_one_grid_carries(gpu, po):
    """source 3 x 1,048,700 at 1:1 and 0 degrees: 65,544 tile rows, the second launch starts at dst row 1,048,560.  Rows on both sides of
    it, the first and the last rows against the oracle; the adjoint's rows there against the fp32 adjoint (its own second launch)"""
    import torch
    W, H = 3, 1048700
    iso = ((W - 1) / 2, (H - 1) / 2)
    src32 = np.random.default_rng(3).standard_normal((H, W)).astype(np.float32)
    rows = np.array([0, 1, 15, 16, 1048543, 1048544, 1048558, 1048559, 1048560, 1048561, 1048575, 1048576, H - 2, H - 1])
    ys, xs = [a.ravel().astype(np.int32) for a in np.meshgrid(rows, np.arange(W), indexing="ij")]
    for mname in ("area", "fast"):
        mode, omode = modes_of(gpu, po, mname)
        rq = gpu.make_request(W, H, 1.0, 1.0, iso, 0.0, mode=mode)
        lay = gpu.query(rq)[2]
        assert (lay.dst_width, lay.dst_height) == (W, H) and (H + 15) // 16 > 65535
        got = _forward(gpu, rq, src32.astype(np.float64))
        gold = po.oracle_pixels(omode, src32, 1.0, 1.0, iso, 0.0, xs, ys)
        scale = po.oracle_pixels(omode, np.abs(src32), 1.0, 1.0, iso, 0.0, xs, ys)
        worst = f64_measure(got[ys, xs], gold, scale, "tall %s" % mname)
        print("tall %s: forward worst %.3e" % (mname, worst))
        assert worst <= F64_TOL and (scale != 0).all(), (mname, worst)
        # the adjoint: every row written (both launches of both passes), and the fp32 adjoint's values to fp32 precision
        g = torch.from_numpy(src32).cuda()
        gs32 = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, g.data_ptr(), W, gs32.data_ptr(), W, _stream(), batch=1)
        torch.cuda.synchronize()
        gs = _adjoint(gpu, rq, src32.astype(np.float64))
        ref = gs32.cpu().numpy().astype(np.float64)
        assert np.abs(gs - ref).max() <= 1e-6 * np.abs(ref).max(), mname


@pytest.mark.parametrize("geometry", [(96, 80, 3.0, 1.0, 17.5), (96, 80, 4.0, 1.0, 0.0)], ids=["3:1 at 17.5", "4:1 at 0"])
def test_non_finite_source_pixels_stay_local(gpu, po, geometry):
    """one NaN, one +Inf and one -Inf source pixel: the output is non-finite exactly where the oracle has weight on one of them, and
    every other pixel stays within F64_TOL"""
    W, H, sr, dr, ang = geometry
    iso = ((W - 1) / 2, (H - 1) / 2)
    src = wide_range((H, W), 41)
    poisoned = [((H // 3, W // 3), np.nan), ((H // 2, 2 * W // 3), np.inf), ((3 * H // 4, W // 5), -np.inf)]
    mark, clean, bad = np.zeros((H, W)), src.copy(), src.copy()
    for (y, x), v in poisoned:
        mark[y, x], clean[y, x], bad[y, x] = 1.0, 0.0, v
    for mname in ("area", "fast"):
        mode, omode = modes_of(gpu, po, mname)
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
        support = po.oracle_run(omode, mark, sr, dr, iso, ang).dst != 0
        assert support.any() and not support.all()
        got = _forward(gpu, rq, bad)
        assert np.array_equal(~np.isfinite(got), support), (mname, int((~np.isfinite(got) ^ support).sum()))
        gold, scale = forward_gold(po, omode, clean, sr, dr, iso, ang)
        keep = ~support
        worst = f64_measure(np.where(keep, got, 0.0), np.where(keep, gold, 0.0), np.where(keep, scale, 0.0), "non-finite %s" % mname)
        print("non-finite %s %s: worst %.3e outside a support of %d pixels" % (geometry, mname, worst, int(support.sum())))
        assert worst <= F64_TOL, (mname, worst)


@pytest.fixture(scope="module")
def delay(gpu):
    """a long-running producer made of ordinary torch work: in-place passes over 64 MiB, several milliseconds in all -- far longer
    than the calls below and than the host needs to enqueue a frame"""
    import torch
    buf = torch.zeros(16 << 20, dtype=torch.float32, device="cuda")

    def run():
        for _ in range(160):
            buf.add_(1.0)
    return run


@pytest.mark.parametrize("which", ["forward", "adjoint"])
@pytest.mark.parametrize("null_stream", [False, True], ids=["created stream", "NULL stream"])
def test_stream_order_without_a_host_wait(gpu, delay, which, null_stream):
    """producer (behind a long delay) -> the call -> consumer -> the input overwritten, all enqueued on one stream without a host wait:
    the consumer's copy has the bits of the synchronous call"""
    import torch
    W, H = 160, 120
    rq = gpu.make_request(W, H, 3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 17.5)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    ishape, oshape = ((H, W), (dH, dW)) if which == "forward" else ((dH, dW), (H, W))
    frames = [torch.from_numpy(wide_range(ishape, 50 + f)).cuda() for f in range(2)]
    inp = torch.empty(ishape, dtype=torch.float64, device="cuda")
    out = torch.empty(oshape, dtype=torch.float64, device="cuda")

    def call(handle):
        if which == "forward":
            gpu.resample_device_f64(rq, inp.data_ptr(), W, out.data_ptr(), dW, handle)
        else:
            gpu.adjoint_device_f64(rq, inp.data_ptr(), dW, out.data_ptr(), W, handle)
    refs = []
    for f in range(2):
        inp.copy_(frames[f])
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        call(_stream())
        torch.cuda.synchronize()
        refs.append(out.clone())
    assert not torch.equal(refs[0], refs[1])
    stream = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    handle = 0 if null_stream else stream.cuda_stream
    got = [torch.empty_like(out) for _ in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for f in range(2):
            inp.fill_(float("nan"))                    # stale reads are loud
            out.fill_(SENTINEL)
            delay()
            inp.copy_(frames[f])                       # the producer, still behind the delay when the call is enqueued
            call(handle)
            got[f].copy_(out)                          # the consumer, enqueued behind the call without a host wait
            for _ in range(4):
                inp.fill_(float("nan"))                # the input's buffer is reused at once
    stream.synchronize()
    for f in range(2):
        assert torch.equal(got[f].view(torch.int64), refs[f].view(torch.int64)), (which, f, int(got[f].isnan().sum()), int((got[f] == SENTINEL).sum()))


def test_capture_of_both_calls_on_a_geometry_never_seen_before(gpu):
    """torch.cuda.graph over forward + adjoint on a geometry no other test uses and nothing has been called with: there is no plan to
    build, so the capture records launches (and the adjoint's stream-ordered scratch) and nothing else; replayed on new input it gives
    the eager bits.  (One adjoint call of ANOTHER geometry comes first: the device's scratch pool is created by the first adjoint call of
    a process, which is host work.)"""
    import torch
    other = gpu.make_request(8, 8, 1.0, 1.0, (3.5, 3.5), 10.0)
    _adjoint(gpu, other, np.ones((gpu.query(other)[2].dst_height, gpu.query(other)[2].dst_width)))
    W, H = 53, 47
    rq = gpu.make_request(W, H, 2.75, 1.0, ((W - 1) / 2 + 0.125, (H - 1) / 2 - 0.375), 23.25)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    x = torch.from_numpy(wide_range((H, W), 61)).cuda()
    y = torch.full((dH, dW), SENTINEL, dtype=torch.float64, device="cuda")
    gx = torch.full((H, W), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    graph, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=cs):
        h = torch.cuda.current_stream().cuda_stream
        gpu.resample_device_f64(rq, x.data_ptr(), W, y.data_ptr(), dW, h)
        gpu.adjoint_device_f64(rq, y.data_ptr(), dW, gx.data_ptr(), W, h)          # W^T W x
    torch.cuda.synchronize()
    for seed in (62, 63):
        new = wide_range((H, W), seed)
        x.copy_(torch.from_numpy(new).cuda())
        y.fill_(SENTINEL)
        gx.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager_y = _forward(gpu, rq, new)
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(eager_y)), seed
        assert np.array_equal(_bits(gx.cpu().numpy()), _bits(_adjoint(gpu, rq, eager_y))), seed
