"""GPU (MI355X): every device entry keeps its stream-order contract with NO host synchronisation around it.

include/aai.h promises that the device entries only enqueue work on the caller's stream.  The library does not stay on that stream --
the double-precision fix-up pass of a rotated request runs beside the production kernel on a pool-owned side stream (fork / join
events), the adjoint takes stream-ordered scratch from a pool shared by every stream, plans are built on a private stream -- so the
contract rests on a handful of event calls that every other GPU test cannot see: they all drain the device around the call.

Here a producer is still running when the call is enqueued, a consumer and the next frame's overwrite of the source are enqueued
right behind it, and only the caller's own stream is synchronised at the end (tests/stream_order.py: the frame loop).  The producer
is held back by a delay of ordinary torch work calibrated to at least 10 x the slowest library call of the module, and a canary
proves first that unordered work really overtakes that delay on this machine.  Results must equal the synchronous call's bit for bit.

Checked once against three deliberately broken builds (not committed): without the side stream's wait for the fork, without the
caller's wait for the join, and with the adjoint wrapper ignoring its stream; each turns the rows that cover it red."""
import pytest

import stream_order as so
from stream_order import FRAMES, SENTINEL, same_bits

pytestmark = pytest.mark.gpu

QUAD = (300, 260, 3.0, 1.0, 30.0, 1)                       # the knife geometry of the flagged-pixel test: aai_quad_kernel, flagged > 0

# name -> how to build it (see _build).  Rows with flagged=True have the double-precision pass beside the production kernel.
FORWARD = [
    "quad area", "cell area (hint)", "cell area 1500x1100", "quad fast", "wide", "K1 fix-up list", "K1 plain", "K1 tile", "K1 wide fallback",
    "double-precision runs", "bicubic sampler", "u8 interleaved C=3", "batch of 3, padded strides", "row band [16, 48)",
]
LIFE_CYCLE = ["quad area", "cell area (hint)", "quad fast", "wide", "K1 fix-up list"]
ADJOINT = ["adjoint general area", "adjoint general fast", "adjoint planned axis", "adjoint planned rotated, listed",
           "adjoint interleaved C=3", "adjoint planned interleaved C=3"]
# name -> (W, H, srcRes, dstRes, angle), planned_backward, channels (None: a (B, H, W) tensor)
TORCH = {"general": ((160, 120, 3.0, 1.0, 17.5), False, None), "planned": ((160, 120, 2.5, 1.0, 90.0), True, None),
         "any": ((128, 96, 3.0, 1.0, 30.0), "any", None), "channels_last": ((128, 96, 3.0, 1.0, 30.0), False, 3)}


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    yield aai
    torch.cuda.synchronize()
    aai.debug_skip_fixup(False)
    aai.debug_cell_min_waves(-1)
    aai.shutdown()


class TorchCase:
    """torch_ops.resample() forward and backward() on a leaf tensor that a delayed producer fills"""

    def __init__(self, h, name):
        import torch
        from area_average_interpolation_amd import torch_ops
        self.torch, self.op, self.name = torch, torch_ops.resample, name
        (W, H, sr, dr, ang), self.planned, C = TORCH[name]
        rq, lay = so.request(h.gpu, W, H, sr, dr, ang, h.gpu.MODE_AREA)
        self.args = (sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
        shape, gshape = ((2, H, W), (2, lay.dst_height, lay.dst_width)) if C is None else ((2, C, H, W), (2, C, lay.dst_height, lay.dst_width))
        fmt = torch.contiguous_format if C is None else torch.channels_last
        self.xs = [x.contiguous(memory_format=fmt) for x in so.rand_frames(torch, shape, 41)]
        self.gs = so.rand_frames(torch, gshape, 43)
        self.x = torch.empty(shape, dtype=torch.float32, device="cuda").contiguous(memory_format=fmt).requires_grad_(True)
        self.ref = []
        for f in range(FRAMES):                            # the synchronous way
            torch.cuda.synchronize()
            y, gx = self.step(f)
            torch.cuda.synchronize()
            self.ref.append((y.clone(), gx.clone()))
            self.x.grad = None
        self.got = [(torch.empty_like(y), torch.empty_like(gx)) for (y, gx) in self.ref]
        assert not same_bits(torch, self.ref[0][1], self.ref[1][1])
        if C is not None:                                  # the zero-copy interleaved route was taken
            assert self.ref[0][0].is_contiguous(memory_format=torch.channels_last) and not self.ref[0][0].is_contiguous()

        def once():
            self.step(0)
            self.x.grad = None
        h.time_call("torch resample+backward " + name, once)

    def step(self, f):
        with self.torch.no_grad():
            self.x.copy_(self.xs[f])
        y, _ = self.op(self.x, *self.args, planned_backward=self.planned)
        (y * self.gs[f]).sum().backward()
        return y.detach(), self.x.grad

    def loop(self, h, caller):
        torch = self.torch
        torch.cuda.synchronize()
        with torch.cuda.stream(caller.stream):
            for f in range(FRAMES):
                with torch.no_grad():
                    self.x.fill_(float("nan"))
                h.delay(caller.stream)
                y, gx = self.step(f)
                self.got[f][0].copy_(y)
                self.got[f][1].copy_(gx)
                self.x.grad = None
                del y, gx
                with torch.no_grad():
                    self.x.fill_(float("nan"))
        caller.stream.synchronize()
        for f in range(FRAMES):
            for k, what in enumerate(("output", "x.grad")):
                got, ref = self.got[f][k], self.ref[f][k]
                assert same_bits(torch, got, ref), "torch resample (%s) from %s, frame %d: %s differs from the synchronous run in %d of %d elements, %d of them NaN" % (
                    self.name, caller.name, f, what, int((got != ref).sum()), got.numel(), int(got.isnan().sum()))


def _build(h, name):
    gpu = h.gpu
    A, F = gpu.MODE_AREA, gpu.MODE_FAST
    if name == "quad area":
        return so.forward(h, name, QUAD, "aai_quad_kernel", 11, flagged=True)
    if name == "quad area (second caller)":                # the same request on buffers of its own: the other caller, and what occupies the side streams
        return so.forward(h, name, QUAD, "aai_quad_kernel", 11, flagged=True, timed=False)
    if name == "cell area (hint)":
        return so.forward(h, name, QUAD, "aai_cell_kernel", 12, flagged=True, prefer_cell=True)
    if name == "cell area 1500x1100":
        return so.forward(h, name, (1500, 1100, 1.0, 1.0, 30.0, A), "aai_cell_kernel", 13, flagged=True)
    if name == "quad fast":
        # (fast mode lists a pixel only where a source pixel's centre lies ON an edge of the dst square: with the isocenter between
        # lattice points, as at even sizes, none does; the third geometry has odd sizes and 296 such pixels)
        for geo in ((600, 600, 2.0, 1.0, 45.0, F), (512, 512, 1.0, 2.0, 45.0, F), (301, 261, 3.0, 1.0, 30.0, F)):
            rq, _ = so.request(gpu, *geo)
            gpu.prepare(rq)
            if so.plan_counts(gpu, rq)[0] > 0:
                break
        return so.forward(h, name, geo, "aai_quad_fast_kernel", 14, flagged=True)
    if name == "wide":                                     # the smallest wide-footprint case that lists pixels, else the flagged-pixel test's
        geo = so.first_runs_case(h, "aai_wide_kernel", flagged=True) or (2048, 2048, 8.0, 1.0, 17.5, A)
        return so.forward(h, name, geo, "aai_wide_kernel", 15, flagged=True)
    if name == "K1 fix-up list":                           # the separable kernel with its listed pixels behind it, in-stream
        return so.forward(h, name, (40, 9, 3.0, 1.0, 0.0, A), "aai_axis", 16, flagged=True)
    if name == "K1 plain":
        return so.forward(h, name, (517, 40, 4.0, 1.0, 0.0, A), "aai_axis_kernel", 17)
    if name == "K1 tile":
        return so.forward(h, name, (300, 33, 3.0, 1.0, 90.0, A), "aai_axis_tile_kernel", 18)
    if name == "K1 wide fallback":
        return so.forward(h, name, (3, 50, 2.0, 1.0, 0.0, A), "aai_axis_wide_kernel", 19)
    if name == "double-precision runs":                    # a footprint beyond 32 x 32 source pixels
        geo = so.first_runs_case(h, "aai_rotated_runs_kernel", flagged=False)
        assert geo is not None, "no RUNS_CASES geometry takes aai_rotated_runs_kernel"
        return so.forward(h, name, geo, "aai_rotated_runs_kernel", 20)
    if name == "bicubic sampler":
        return so.forward(h, name, (80, 60, 1.0, 2.0, 300.0, gpu.MODE_BICUBIC), "aai_sample_kernel", 21)
    if name == "u8 interleaved C=3":
        return so.interleaved_u8(h, name, (128, 96, 3.0, 1.0, 30.0, A), 3, 22)
    if name == "batch of 3, padded strides":
        return so.padded_batch(h, name, QUAD, 23)
    if name == "row band [16, 48)":
        return so.row_band(h, name, (640, 480, 3.0, 1.0, 30.0, A), (16, 48), 24)
    if name == "adjoint general area":
        return so.adjoint(h, name, (160, 120, 3.0, 1.0, 17.5, A), 31, kernel="aai_adjoint_gather_kernel")
    if name == "adjoint general fast":
        return so.adjoint(h, name, (16, 12, 1.0, 2.0, 45.0, F), 32, kernel="aai_adjoint_gather_kernel")
    if name == "adjoint planned axis":
        return so.adjoint(h, name, (160, 120, 2.5, 1.0, 90.0, A), 33, planned=True, kernel="aai_axis_adjoint_kernel")
    if name == "adjoint planned rotated, listed":          # the knife geometry: the plan's knife list is not empty, its listed pass runs
        return so.adjoint(h, name, QUAD, 34, planned="any", kernel="aai_adjoint_plain_gather_kernel", listed=True)
    if name == "adjoint interleaved C=3":
        return so.adjoint(h, name, (160, 120, 3.0, 1.0, 17.5, A), 35, channels=3, kernel="aai_adjoint_gather_multi_kernel")
    if name == "adjoint planned interleaved C=3":
        return so.adjoint(h, name, (128, 96, 3.0, 1.0, 30.0, A), 36, planned="any", channels=3, kernel="aai_adjoint_plain_gather_multi_kernel")
    raise KeyError(name)


@pytest.fixture(scope="module")
def harness(gpu):
    """Builds every scenario of the module (buffers, seeded frames, synchronous references, event-timed calls), then sizes the delay by
    the slowest of them and runs the canary: once, before any ordering test."""
    h = so.Harness(gpu)
    h.torch_cases = {}
    for name in FORWARD + ["quad area (second caller)"] + ADJOINT + list(TORCH):
        try:                                               # a scenario that cannot be built fails its own tests, not the module
            if name in TORCH:
                h.torch_cases[name] = TorchCase(h, name)
            else:
                _build(h, name)
        except Exception as e:
            h.broken[name] = e
    h.slowest_ms = h.calibrate()
    h.run_canary()
    h.write_profile()
    print(h.report)
    return h


def test_the_delay_dwarfs_every_call_and_unordered_work_overtakes_it(harness):
    h = harness
    assert h.delay_ms >= so.MARGIN * h.slowest_ms, h.report
    assert not h.broken, (h.broken, h.report)
    assert h.canary is not None, "harness cannot discriminate: none of %d unordered streams overtook the delay\n%s" % (len(h.canary_tries), h.report)
    assert len(h.callers()) == 5 and h.callers()[0].handle == 0


def _beside(sc):
    """does this row's fix-up pass run on a side stream of the pool?  (K1's list follows in-stream)"""
    return sc.flagged > 0 and "axis" not in sc.kernel


@pytest.mark.parametrize("name", FORWARD)
def test_forward_entries_in_a_frame_loop(harness, name):
    """Every caller stream runs the frame loop; rows whose pass runs beside the production kernel run it a second time with the pool's
    side streams occupied by another caller, so that the pass finishes long after the production kernel and only the join holds the
    consumer (and the next frame's overwrite of the source) back."""
    h = harness
    h.require_canary()
    sc = h.scenario(name)
    for caller in h.callers():
        h.frame_loop(sc, caller)
        if _beside(sc):
            h.frame_loop(sc, caller, blocker=h.scenario("quad area (second caller)"))
        if sc.valid is not None:                           # the padding between rows and images keeps the caller's bytes
            assert all(bool((g[~sc.valid] == SENTINEL).all()) for g in sc.got), (name, caller.name)


@pytest.mark.parametrize("name", LIFE_CYCLE)
def test_side_stream_life_cycle_inside_a_frame_loop(harness, name):
    """After aai_shutdown (plans, the pool's side streams and its launch count are gone): frame 0 builds the plan mid-stream and has
    the pass in-stream, frame 1 creates the side streams, frames 2 and 3 run beside on rotating slots."""
    h = harness
    h.require_canary()
    sc = h.scenario(name)
    for caller in (h.callers()[0], h.callers()[3]):
        h.torch.cuda.synchronize()
        h.gpu.shutdown()
        assert h.plan_info(sc) == ""
        h.frame_loop(sc, caller)
        assert h.plan_info(sc) != ""


def _two_streams(h, first, second, order, scales):
    """frames of two scenarios on two streams, enqueued in `order` (a sequence of 0 / 1: whose next frame), each with its own delay"""
    h.torch.cuda.synchronize()
    pair, nxt = (first, second), [0, 0]
    for who in order:
        sc, caller = pair[who]
        h.enqueue_frame(sc, caller, nxt[who], scales[who])
        nxt[who] += 1
    assert nxt == [FRAMES, FRAMES]
    for sc, caller in pair:
        caller.stream.synchronize()
    for sc, caller in pair:
        h.check(sc, "%s from %s beside %s" % (sc.name, caller.name, pair[1 - pair.index((sc, caller))][0].name))


ALTERNATING, FIRST_THEN_SECOND = [0, 1] * FRAMES, [0] * FRAMES + [1] * FRAMES


def test_two_callers_share_the_plan_and_the_side_streams(harness):
    """Two streams run the quad-area loop at once on the same request: one plan, the pool's four event slots, staggered delays.
    Alternating enqueues; then one caller's four calls take all four slots while its stream is still busy and the other caller's
    faster frames queue their passes behind them, both ways round."""
    h = harness
    h.require_canary()
    a, b = h.callers()[2], so.Caller("the canary's unordered stream", h.canary[1])
    one, two = h.scenario("quad area"), h.scenario("quad area (second caller)")
    _two_streams(h, (one, a), (two, b), ALTERNATING, (1.0, 1.5))
    _two_streams(h, (one, a), (two, b), FIRST_THEN_SECOND, (2.0, 1.0))
    _two_streams(h, (two, b), (one, a), FIRST_THEN_SECOND, (2.0, 1.0))


def test_multi_device_entry_with_a_delayed_producer_per_shard(harness):
    """aai_resample_batch_multi_device_f32: two shards of device 0 on two streams, each shard's source written by its own delayed
    producer, each stream synchronised alone"""
    h = harness
    h.require_canary()
    gpu, torch = h.gpu, h.torch
    rq, lay = h.scenario("quad area").rq, h.scenario("quad area").lay
    W, H, dW, dH = rq.src_width, rq.src_height, lay.dst_width, lay.dst_height
    frames = so.rand_frames(torch, (2, H, W), 25)
    inp = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    out = torch.empty((2, dH, dW), dtype=torch.float32, device="cuda")
    got = [torch.empty_like(out) for _ in range(FRAMES)]

    def call(h1, h2):
        gpu.resample_multi_device(rq, [(0, 1, inp[0].data_ptr(), out[0].data_ptr(), h1), (0, 1, inp[1].data_ptr(), out[1].data_ptr(), h2)], W, W * H, dW, dW * dH)

    ref = []
    for f in range(FRAMES):
        inp.copy_(frames[f])
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        call(0, 0)
        torch.cuda.synchronize()
        ref.append(out.clone())
    c = h.callers()
    for pair in ((c[0], c[2]), (c[2], c[3]), (c[4], c[1])):
        torch.cuda.synchronize()
        for f in range(FRAMES):
            for k, caller in enumerate(pair):
                with torch.cuda.stream(caller.stream):
                    inp[k].fill_(float("nan"))
                    out[k].fill_(SENTINEL)
                    h.delay(caller.stream, 1.0 + 0.5 * k)
                    inp[k].copy_(frames[f][k])
            call(pair[0].handle, pair[1].handle)
            for k, caller in enumerate(pair):
                with torch.cuda.stream(caller.stream):
                    got[f][k].copy_(out[k])
                    inp[k].fill_(float("nan"))
        for caller in pair:
            caller.stream.synchronize()
        for f in range(FRAMES):
            for k in range(2):
                g = got[f][k]
                assert same_bits(torch, g, ref[f][k]), "shard %d on %s, frame %d: %d of %d pixels differ, %d NaN, %d sentinel" % (
                    k, pair[k].name, f, int((g != ref[f][k]).sum()), g.numel(), int(g.isnan().sum()), int((g == SENTINEL).sum()))


@pytest.mark.parametrize("name", ADJOINT)
def test_adjoint_entries_in_a_frame_loop(harness, name):
    """gdst from a delayed producer, gsrc read by a consumer behind the call, gdst overwritten right after"""
    h = harness
    h.require_canary()
    for caller in h.callers():
        h.frame_loop(h.scenario(name), caller)


def test_adjoint_scratch_pool_across_two_streams(harness):
    """Two streams alternate general-adjoint calls of two sizes with staggered delays: scratch freed in one stream's order is handed
    out again while the other stream's kernels are in flight, and every result keeps the synchronous call's bits."""
    h = harness
    h.require_canary()
    a, b = h.callers()[2], so.Caller("the canary's unordered stream", h.canary[1])
    big, small = h.scenario("adjoint general area"), h.scenario("adjoint general fast")
    _two_streams(h, (big, a), (small, b), ALTERNATING, (1.0, 1.5))
    _two_streams(h, (small, a), (big, b), ALTERNATING, (1.5, 1.0))
    _two_streams(h, (big, h.callers()[0]), (small, b), FIRST_THEN_SECOND, (2.0, 1.0))


@pytest.mark.parametrize("name", list(TORCH))
def test_torch_operator_between_asynchronous_torch_kernels(harness, name):
    """resample() and backward() under torch.cuda.stream(s): the input comes from a delayed producer, output and x.grad are consumed
    in stream order, the stream is synchronised only at the end"""
    h = harness
    h.require_canary()
    for caller in h.callers():
        h.scenario(name).loop(h, caller)


@pytest.mark.parametrize("name", ["quad area", "K1 fix-up list"])
def test_captured_call_replays_on_new_data(harness, name):
    """A linear graph of one resample_device call, captured after aai_prepare and after the side streams exist (the pass then follows
    in-stream), replayed on three frames without a host wait: the capture recorded launches, not results or stale state."""
    h = harness
    h.require_canary()
    gpu, torch = h.gpu, h.torch
    sc = h.scenario(name)
    gpu.prepare(sc.rq)
    one = h.scenario("quad area")
    for _ in range(2):                                     # (the pool creates its side streams at the second launch that has a pass beside it)
        h.call(one, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    graph, cs = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=cs):
        h.call(sc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(cs):
        for f in range(3):
            sc.inp.fill_(sc.poison)
            sc.out.fill_(SENTINEL)
            h.delay(cs)
            sc.inp.copy_(sc.frames[f])
            graph.replay()
            sc.got[f].copy_(sc.out)
            sc.inp.fill_(sc.poison)
        sc.got[3].copy_(sc.ref[3])                         # (three frames: the fourth slot is not part of this test)
    cs.synchronize()
    h.check(sc, "%s replayed from a captured graph" % name)
    del graph
