"""The half-precision adjoint on the MI355X (include/aai_adjoint_half.h): both routes against narrow(aai_adjoint_planned_interleaved_device_f32(
widen(g))) computed on the GPU in the same test, bit for bit; the direct kernel against its CPU replay; non-finite gradients; batches; the
memory contract with guarded, 2-byte-aligned, padded buffers; address arithmetic at a wide pitch; stream order; a captured graph.

The reference arithmetic is always computed here around the fp32 entry: torch widens (exactly), and the fp32 result is narrowed on the
host by the library's rounding helper (half_cases.narrow), which keeps a NaN's sign as the contract's narrowing does.  No tolerance
anywhere in this file: the header promises equal bits on every route."""
import numpy as np
import pytest

import adjoint_half_cases as ac
import half_cases as hc
import stream_order as so
import wide_pitch as wp
from guard_layout import GuardedLayout, to_device, to_numpy

pytestmark = pytest.mark.gpu

SENTINEL16 = 0x7fa5           # a NaN in both element types that no arithmetic here produces
NAN16 = {hc.F16: 0x7e00, hc.BF16: 0x7fc0}
ROT = (96, 80, 3, 1, (47.5, 39.5), 17.5)               # ROT of tests/test_half_torch_gpu.py
WIDE = (3, 50, 2, 1, (1.0, 24.5), 0.0)                 # aai_query: AAI_KERNEL_AXIS_WIDE
IDS = [t[1] for t in ac.TYPES]


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    aai.set_device(0)
    return aai


def tdtype(ht):
    import torch
    return torch.float16 if ht == hc.F16 else torch.bfloat16


def upload(bits, ht):
    """raw 16-bit elements -> a device tensor of the element type, same shape"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()).cuda().view(tdtype(ht))


def download(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_half(gpu, rq, ht, g):
    """one [dH, dW, C] gradient of raw bits through adjoint_half_device -> ([H, W, C] raw bits, the kernel's name)"""
    import torch
    dH, dW, C = g.shape
    H, W = rq.src_height, rq.src_width
    gd = upload(g, ht)
    gs = upload(np.full((H, W, C), SENTINEL16, np.uint16), ht)
    gpu.adjoint_half_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, ht, stream=stream())
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    return download(gs), kernel


def run_reference(gpu, rq, ht, g):
    """narrow(aai_adjoint_planned_interleaved_device_f32(widen(g))) -> ([H, W, C] raw bits, the fp32 route's name)"""
    import torch
    dH, dW, C = g.shape
    H, W = rq.src_height, rq.src_width
    g32 = upload(g, ht).float().contiguous()
    s32 = torch.full((H, W, C), float("nan"), dtype=torch.float32, device="cuda")
    gpu.adjoint_interleaved_device(rq, C, g32.data_ptr(), dW * C, s32.data_ptr(), W * C, stream=stream(), planned="separable")
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    # (narrowed on the host by the library's own rounding helper: it keeps a NaN's sign, as the contract's narrowing does; torch's
    # conversion does not)
    return hc.narrow(s32.cpu().numpy(), ht), kernel


def kernel_name(tname, C):
    return "aai_axis_adjoint_half_kernel<%s,%d>" % (tname, C)


def _request(gpu, geom, mode_name="area"):
    W, H, sr, dr, iso, ang = geom
    return gpu.make_request(W, H, sr, dr, iso, ang, mode=hc.mode_of(gpu, mode_name))


# ---- the direct route --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ac.KEYS, ids=ac.key_id)
def test_direct_kernel_has_the_fp32_entrys_narrowed_bits_and_the_replays(gpu, key):
    """every case x {own angle, + 90, + 270} x type x C in {1, 3, 4} (C = 2 on case d) in every mode whose plan the CPU-side planner gives
    adjoint tables and no lists; the non-finite variant at C = 3"""
    ran = direct = 0
    for mode in ac.MODES:
        rq = ac.request(gpu, key, mode)
        if not ac.is_direct(rq):
            continue
        lay = gpu.query(rq)[2]
        for ht, tname in ac.TYPES:
            for C in (1, 3, 4) + ((2,) if key[0] == "d" else ()):
                for nonfinite in ((False, True) if C == 3 else (False,)):
                    what = "%s %s %s C=%d nonfinite=%d" % (ac.key_id(key), mode, tname, C, nonfinite)
                    g = ac.gradient_bits(lay, C, ht, nonfinite=nonfinite)
                    got, kernel = run_half(gpu, rq, ht, g)
                    want, ref_kernel = run_reference(gpu, rq, ht, g)
                    if ac.serves_direct(gpu, rq, C):
                        assert kernel == kernel_name(tname, C), (what, kernel, gpu.plan_shape(rq, 1))
                        direct += 1
                    else:      # the class that forwards by measurement: the same bits, the replay's included
                        assert C == 1 and kernel == ref_kernel + "+widened", (what, kernel)
                    assert ref_kernel == ("aai_axis_adjoint_kernel" if C == 1 else "aai_axis_adjoint_multi_kernel<%d>" % C), (what, ref_kernel)
                    differ = got != want
                    assert not differ.any(), (what, int(differ.sum()), np.argwhere(differ)[:4].tolist())
                    rep = ac.replay(rq, ht, g)
                    assert np.array_equal(got, rep), (what, "replay", int((got != rep).sum()))
                    if nonfinite:
                        v = hc.widen(got, ht)
                        assert np.isnan(v[:, :, 0]).any() and not np.isnan(v[:, :, C - 1]).any(), what
                    ran += 1
    assert ran and direct >= ran * 2 // 3, "no mode of this case takes the direct route"


# ---- the forwarding route ------------------------------------------------------------------------------------------------------
def listed_keys(gpu):
    """the shared cases whose plan has correction lists (the CPU-side planner's answer; area mode)"""
    return [k for k in ac.KEYS if ac.facts(ac.request(gpu, k, "area"))[1][1] > 0 and ac.facts(ac.request(gpu, k, "area"))[1][2] > 0]


@pytest.mark.parametrize("ht, tname", ac.TYPES, ids=IDS)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", ["rotated area", "rotated fast", "wide", "listed", "listed transposed"])
def test_forwarding_route_has_the_fp32_entrys_narrowed_bits(gpu, name, C, ht, tname):
    if name.startswith("rotated"):
        rq = _request(gpu, ROT, name.split()[1])
    elif name == "wide":
        rq = _request(gpu, WIDE)
        assert gpu.query(rq)[2].kernel == gpu._lib.KERNEL_AXIS_WIDE
    else:
        keys = [k for k in listed_keys(gpu) if (k[1] != 0.0) == (name == "listed transposed")]
        assert keys, "no shared case with correction lists"
        rq = ac.request(gpu, keys[0], "area")
    lay = gpu.query(rq)[2]
    for nonfinite in (False, True):
        g = ac.gradient_bits(lay, C, ht, seed=31, nonfinite=nonfinite)
        got, kernel = run_half(gpu, rq, ht, g)
        want, ref_kernel = run_reference(gpu, rq, ht, g)
        assert kernel == ref_kernel + "+widened" and "aai_axis_adjoint_half_kernel" not in kernel, (name, kernel, ref_kernel)
        if name.startswith("listed"):
            assert "+listed" in kernel, kernel
        assert np.array_equal(got, want), (name, C, tname, nonfinite, int((got != want).sum()))
        assert nonfinite or np.isfinite(hc.widen(got, ht)).all()


# ---- batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht, tname", ac.TYPES, ids=IDS)
@pytest.mark.parametrize("name", ["direct", "forwarding"])
def test_image_b_of_a_batch_has_the_single_calls_bits_and_an_empty_batch_touches_nothing(gpu, name, ht, tname):
    import torch
    C, B = 3, 3
    rq = ac.request(gpu, ("e", 90.0), "area") if name == "direct" else _request(gpu, ROT)
    lay = gpu.query(rq)[2]
    H, W, dH, dW = rq.src_height, rq.src_width, lay.dst_height, lay.dst_width
    gs_np = [ac.gradient_bits(lay, C, ht, seed=40 + b) for b in range(B)]
    singles = [run_half(gpu, rq, ht, g) for g in gs_np]
    gd = upload(np.stack(gs_np), ht)
    gs = upload(np.full((B, H, W, C), SENTINEL16, np.uint16), ht)
    gpu.adjoint_half_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, ht, stream=stream(), batch=B, dst_image_stride=dH * dW * C,
                            src_image_stride=H * W * C)
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    out = download(gs)
    assert kernel == singles[0][1] and (kernel == kernel_name(tname, C) if name == "direct" else kernel.endswith("+widened")), kernel
    for b in range(B):
        assert np.array_equal(out[b], singles[b][0]), (name, tname, b)
    # batch = 0: AAI_OK, nothing read, nothing written
    gs = upload(np.full((B, H, W, C), SENTINEL16, np.uint16), ht)
    gpu.adjoint_half_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, ht, stream=stream(), batch=0, dst_image_stride=dH * dW * C,
                            src_image_stride=H * W * C)
    torch.cuda.synchronize()
    assert (download(gs) == SENTINEL16).all()


# ---- the memory contract -----------------------------------------------------------------------------------------------------------
def guarded_batch(gpu, rq, channels, ht, what):
    """Batch 3 through the device entry; both base addresses ONE element past a 256-byte boundary (2-byte aligned and nothing more); odd
    padded row strides on both sides; image strides larger than the image.  The padding of gdst is pre-filled with NaN: a read of it would
    reach gsrc, and it is checked unchanged.  gsrc: every element starts as a sentinel, every entitled element must be written (zeros
    included) and none outside them may change.  -> (the kernel's name, the [3, H, W, C] output, the three gradients)"""
    import torch
    B = 3
    lay = gpu.query(rq)[2]
    H, W, dH, dW = rq.src_height, rq.src_width, lay.dst_height, lay.dst_width
    sstride = W * channels + 3 + (W * channels) % 2                  # odd
    dstride = dW * channels + 5 + (dW * channels) % 2                # odd
    assert sstride % 2 == 1 and dstride % 2 == 1
    dl = GuardedLayout((B, dH, dW, channels), "u16", stride=dstride, image_stride=dH * dstride + 7, base_offset=1)      # gdst: read
    sl = GuardedLayout((B, H, W, channels), "u16", stride=sstride, image_stride=H * sstride + 11, base_offset=1)        # gsrc: written
    grads = [ac.gradient_bits(lay, channels, ht, seed=20 + b) for b in range(B)]
    dbuf = dl.make_src(np.stack(grads), "zeros")
    dbuf[~dl.entitled] = NAN16[ht]
    sbuf = np.full(sl.total, SENTINEL16, np.uint16)
    dd, ds = to_device(dbuf), to_device(sbuf)
    assert dl.ptr(dd) % 4 == 2 and sl.ptr(ds) % 4 == 2
    gpu.adjoint_half_device(rq, channels, dl.ptr(dd), dstride, sl.ptr(ds), sstride, ht, stream=stream(), batch=B, dst_image_stride=dl.image_stride,
                            src_image_stride=sl.image_stride)
    kernel = gpu.last_kernel()
    torch.cuda.synchronize()
    after = to_numpy(ds, np.uint16)
    changed = np.flatnonzero((after != SENTINEL16) & ~sl.entitled)
    assert changed.size == 0, (what, [sl.describe(int(o) - sl.lead) for o in changed[:4]])
    assert np.array_equal(to_numpy(dd, np.uint16), dbuf)
    out = after[sl.index].reshape(B, H, W, channels)
    assert not (out == SENTINEL16).any(), (what, "entitled elements not written")
    return kernel, out, grads


# (d + 90: W * C odd for C = 1 and 3 -- 67 and 201 elements in a source row; h: 5 and 15; c + 270: five workgroups in x, flipped and transposed)
GUARDED_DIRECT = [(("d", 90.0), 1), (("d", 90.0), 3), (("h", 0.0), 3), (("c", 270.0), 4), (("e", 0.0), 2), (("a", 270.0), 1)]


@pytest.mark.parametrize("ht, tname", ac.TYPES, ids=IDS)
@pytest.mark.parametrize("key, C", GUARDED_DIRECT, ids=["%s x%d" % (ac.key_id(k), c) for k, c in GUARDED_DIRECT])
def test_direct_kernel_batch_of_three_in_padded_buffers(gpu, key, C, ht, tname):
    rq = ac.request(gpu, key, "fast")
    assert ac.is_direct(rq)
    what = (ac.key_id(key), C, tname)
    kernel, out, grads = guarded_batch(gpu, rq, C, ht, what)
    assert kernel == kernel_name(tname, C), kernel
    zeros = 0
    for b, g in enumerate(grads):
        rep = ac.replay(rq, ht, g)
        assert np.array_equal(out[b], rep), what + (b,)
        zeros += int((rep == 0).sum())
    print("%s: %d elements of gsrc that no dst pixel reads, written as +0" % (what, zeros))


@pytest.mark.parametrize("ht, tname", ac.TYPES, ids=IDS)
@pytest.mark.parametrize("name, C", [("rotated", 3), ("listed", 1)])
def test_forwarding_route_batch_of_three_in_padded_buffers(gpu, name, C, ht, tname):
    """rotated: 96 x 3 = 288 elements per row; listed: case b (area mode), 259 elements per row -- an odd row length"""
    rq = _request(gpu, ROT) if name == "rotated" else ac.request(gpu, [k for k in listed_keys(gpu) if k[0] == "b"][0], "area")
    assert name == "rotated" or (rq.src_width * C) % 2 == 1
    kernel, out, grads = guarded_batch(gpu, rq, C, ht, (name, tname))
    assert kernel.endswith("+widened"), kernel
    for b, g in enumerate(grads):
        assert np.array_equal(out[b], run_reference(gpu, rq, ht, g)[0]), (name, tname, b)


# ---- address arithmetic at a wide pitch ----------------------------------------------------------------------------------------------
def test_gsrc_rows_beyond_2_31_elements(gpu):
    """A 5 x 40 bf16 RGB source gradient whose view has a row pitch that puts its last rows beyond 2^31 elements (the method of
    tests/wide_pitch.py: a strided view into an arena that is never filled whole, about 4.3 GiB; only the entitled elements and the guard
    behind each row are initialised): the dense call's bits, the elements behind every row untouched.  gdst is dense."""
    import torch
    geom, C, ht = (5, 40, 2, 1, (2.0, 19.5), 90.0), 3, hc.BF16
    W, H = geom[:2]
    rq = _request(gpu, geom, "fast")
    assert ac.is_direct(rq)
    lay = gpu.query(rq)[2]
    dW = lay.dst_width
    g = ac.gradient_bits(lay, C, ht, seed=5)
    tight, kernel = run_half(gpu, rq, ht, g)
    assert kernel == kernel_name("bf16", C) and np.array_equal(tight, ac.replay(rq, ht, g))
    pitch = (-(-(1 << 31) // (H - 1)) + 5) | 1                                       # odd: rows alternate between 4-byte phases
    assert (H - 1) * pitch >= 1 << 31
    arena = wp.Arena(wp.extent_bytes(H, W * C, pitch, 2))
    try:
        rows, guard = arena.view("u16", H, W * C, pitch)
        rows.fill_(0x7fa5)
        guard.fill_(0x7fa5)
        gd = upload(g, ht)
        gpu.adjoint_half_device(rq, C, gd.data_ptr(), dW * C, rows.data_ptr(), pitch, ht, stream=stream())
        assert gpu.last_kernel() == kernel
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy().view(np.uint16).reshape(H, W, C), tight)
        assert bool((guard == 0x7fa5).all())
    finally:
        arena.free()


# ---- stream order --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(gpu):
    """one scenario per route: the call between a delayed producer and a consumer on the caller's stream, no host wait (stream_order.py)"""
    import torch
    h = so.Harness(gpu)
    C = 3
    for name, rq, ht, route in (("direct", ac.request(gpu, ("d", 90.0), "area"), hc.F16, "aai_axis_adjoint_half_kernel"),
                                ("forwarding", _request(gpu, ROT), hc.BF16, "+widened")):
        lay = gpu.query(rq)[2]
        H, W, dH, dW = rq.src_height, rq.src_width, lay.dst_height, lay.dst_width
        n = W * H * C
        inp = torch.empty((dH, dW, C), dtype=tdtype(ht), device="cuda")
        out = torch.empty((n + n % 2,), dtype=tdtype(ht), device="cuda")      # (an even count: the harness compares 32-bit words)
        sc = so.Scenario(name, inp, out, so.rand_frames(torch, (dH, dW, C), 50),
                         lambda handle, rq=rq, inp=inp, out=out, W=W, dW=dW, ht=ht: gpu.adjoint_half_device(rq, C, inp.data_ptr(), dW * C, out.data_ptr(),
                                                                                                            W * C, ht, handle))
        sc.rq, sc.lay = rq, lay
        gpu.adjoint_rotated_prepare(rq)
        h.add(sc)
        sc.kernel = gpu.last_kernel()
        assert route in sc.kernel, (name, sc.kernel)
    h.calibrate()
    return h


@pytest.mark.parametrize("name", ["direct", "forwarding"])
def test_adjoint_half_entry_keeps_stream_order(harness, name):
    import torch
    sc = harness.scenario(name)
    for caller in (so.Caller("torch's current stream", torch.cuda.current_stream()), so.Caller("a fresh stream", torch.cuda.Stream())):
        harness.frame_loop(sc, caller)


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht, tname", ac.TYPES, ids=IDS)
def test_a_prepared_direct_call_replays_from_a_graph_to_the_eager_bits(gpu, ht, tname):
    """one kernel, a linear graph; the plan and its adjoint tables are prepared beforehand (an unprepared call is not attempted)"""
    import torch
    C = 4
    rq = ac.request(gpu, ("l", 270.0), "area")
    assert ac.is_direct(rq)
    lay = gpu.query(rq)[2]
    H, W, dH, dW = rq.src_height, rq.src_width, lay.dst_height, lay.dst_width
    gpu.adjoint_rotated_prepare(rq)
    assert "adjoint=tables" in gpu.plan_shape(rq, 1), gpu.plan_shape(rq, 1)
    g = ac.gradient_bits(lay, C, ht, seed=77)
    eager, kernel = run_half(gpu, rq, ht, g)
    assert kernel == kernel_name(tname, C)
    gd = upload(np.zeros_like(g), ht)
    gs = upload(np.full((H, W, C), SENTINEL16, np.uint16), ht)
    torch.cuda.synchronize()
    graph, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=cs):
        gpu.adjoint_half_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, ht, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (download(gs) == SENTINEL16).all()                  # recorded, not run
    gd.copy_(upload(g, ht))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(download(gs), eager)
