"""Harness of tests/test_gpu_stream_order.py: a calibrated delay made of ordinary torch work, the canary that proves unordered work
overtakes it on this machine, the scenarios (one library call each, on buffers of their own, with reference results computed the
synchronous way) and the frame loop that runs a scenario from a caller's stream without a host wait.

A scenario's call reads `inp` and writes `out`, both allocated once; the frame loop reuses them for every frame, as a real frame loop
would, and poisons them around the call so that a read or write the library orders wrongly shows up as NaN, as the sentinel or as
another frame's data.  Nothing here synchronises inside a loop; reference results are computed with a device-wide synchronise on both
sides of the call."""
import math
import os
import re

from conftest import ROOT, RUNS_CASES

FRAMES = 4
SENTINEL = -7.0
DELAY_BYTES = 256 << 20            # the tensor the delay passes over
MARGIN = 10                        # delay >= MARGIN x the slowest library call of the module
MIN_DELAY_MS = 5.0                 # ... and long against the host's time to enqueue one frame (a dozen launches, ~0.1 ms)
PROFILE = os.path.join(ROOT, "profiles", "stream_order.txt")


class Caller:
    """a stream the way a caller holds it: the torch object (to enqueue torch work on and to synchronise) and the handle the library gets"""

    def __init__(self, name, stream, handle=None):
        self.name, self.stream = name, stream
        self.handle = stream.cuda_stream if handle is None else handle


class Scenario:
    """One call under test.  call(handle) enqueues it on the stream `handle`, reading self.inp and writing self.out."""

    def __init__(self, name, inp, out, frames, enqueue, poison=float("nan"), prefer_cell=False, maskable=False, kernel="", info=""):
        self.name, self.inp, self.out, self.frames, self._enqueue = name, inp, out, frames, enqueue
        self.poison, self.prefer_cell, self.maskable, self.kernel, self.info = poison, prefer_cell, maskable, kernel, info
        self.ref = None            # FRAMES results of the synchronous way, never written again
        self.got = None
        self.valid = None          # bool mask of the elements of `out` the call writes (None: all of them)
        self.flagged = 0
        self.ms = 0.0


class Harness:
    def __init__(self, gpu):
        import torch
        self.torch, self.gpu = torch, gpu
        self.buf = torch.zeros(DELAY_BYTES // 4, dtype=torch.float32, device="cuda")
        self.pass_ms = self.delay_ms = 0.0
        self.passes = 0
        self.call_ms = {}
        self.scenarios = {}
        self.torch_cases = {}
        self.broken = {}           # name -> the exception that kept a scenario from being built
        self.canary = None         # (stream A, stream B that overtook A's delay)
        self.canary_tries = []
        self._callers = None
        self.report = ""

    # ---- the delay ---------------------------------------------------------------------------------------------------
    def delay(self, stream, scale=1.0):
        """`scale` x the calibrated delay as ordinary torch work on `stream` (callers on several streams share the tensor: nobody
        reads its values)"""
        with self.torch.cuda.stream(stream):
            for _ in range(int(math.ceil(self.passes * scale))):
                self.buf.add_(1.0)

    def _events_ms(self, fn, repeats=1):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(repeats):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / repeats

    def time_call(self, name, fn):
        """event-measured duration of one library call on the current stream, after warm-up: the slowest of three"""
        fn()
        fn()
        self.call_ms[name] = max(self._events_ms(fn) for _ in range(3))
        return self.call_ms[name]

    def calibrate(self):
        self.passes = 8
        self.delay(self.torch.cuda.current_stream())                                 # warm-up
        self.pass_ms = self._events_ms(lambda: self.buf.add_(1.0), repeats=50)
        slowest = max(self.call_ms.values())
        want = max(MARGIN * slowest, MIN_DELAY_MS)
        self.passes = int(math.ceil(1.25 * want / self.pass_ms))                     # (25 % above the bar: passes do not all take the mean)
        self.delay_ms = self._events_ms(lambda: self.delay(self.torch.cuda.current_stream()))
        lines = ["stream-order harness calibration (tests/test_gpu_stream_order.py), event-measured on %s" % self.torch.cuda.get_device_name(0),
                 "library calls, slowest of three after warm-up [ms]:"]
        lines += ["  %-28s %8.4f" % (k, v) for k, v in sorted(self.call_ms.items(), key=lambda kv: -kv[1])]
        lines += ["delay: %d in-place passes over %d MiB, %.4f ms per pass, %.3f ms measured = %.1f x the slowest call (%.4f ms); bar %d x"
                  % (self.passes, DELAY_BYTES >> 20, self.pass_ms, self.delay_ms, self.delay_ms / slowest, slowest, MARGIN)]
        self.report = "\n".join(lines)
        return slowest

    def write_profile(self):
        try:
            with open(PROFILE, "w") as f:
                f.write(self.report + "\n")
        except OSError:                # a read-only checkout: the figures are still in the first assertion's message
            pass

    # ---- the canary --------------------------------------------------------------------------------------------------
    def run_canary(self):
        """On stream A: delay, then buf <- new.  On an unrelated stream B, with no wait: snap <- buf.  B overtakes A when snap holds
        the OLD contents.  Streams can share a hardware queue, so up to 8 fresh B streams are tried; the first that overtakes is kept."""
        torch = self.torch
        old = torch.full((1 << 18,), 1.0, dtype=torch.float32, device="cuda")
        new = torch.full((1 << 18,), 2.0, dtype=torch.float32, device="cuda")
        buf, snap = torch.empty_like(old), torch.empty_like(old)
        a = torch.cuda.Stream()
        for k in range(8):
            b = torch.cuda.Stream()
            buf.copy_(old)
            snap.fill_(0.0)
            torch.cuda.synchronize()
            self.delay(a)
            with torch.cuda.stream(a):
                buf.copy_(new)
            with torch.cuda.stream(b):
                snap.copy_(buf)
            a.synchronize()
            b.synchronize()
            overtook = bool(torch.equal(snap, old))
            self.canary_tries.append(overtook)
            assert overtook or bool(torch.equal(snap, new)), "the canary's copy is neither the old nor the new contents"
            if overtook:
                self.canary = (a, b)
                break
        self.report += "\ncanary: unordered stream overtook the delay on try %s of %d" % (
            self.canary_tries.index(True) + 1 if self.canary else "-", len(self.canary_tries))

    def require_canary(self):
        assert self.canary is not None, "harness cannot discriminate: no unordered stream overtook the delay\n" + self.report

    def callers(self):
        """the legacy default stream by its handle 0, torch's current stream, three fresh streams (the canary's A among them)"""
        torch = self.torch
        if self._callers is None:
            self._callers = [Caller("legacy default stream", torch.cuda.default_stream(), 0), Caller("torch's current stream", torch.cuda.current_stream()),
                             Caller("fresh stream 1", self.canary[0]), Caller("fresh stream 2", torch.cuda.Stream()), Caller("fresh stream 3", torch.cuda.Stream())]
        return self._callers

    # ---- scenarios ---------------------------------------------------------------------------------------------------
    def call(self, sc, handle):
        if sc.prefer_cell:
            self.gpu.debug_cell_min_waves(0)
        try:
            sc._enqueue(handle)
        finally:
            if sc.prefer_cell:
                self.gpu.debug_cell_min_waves(-1)

    def plan_info(self, sc):
        """aai_plan_info of the scenario's request as the library sees it (with the scenario's hint bits)"""
        if sc.prefer_cell:
            self.gpu.debug_cell_min_waves(0)
        try:
            return self.gpu.plan_shape(sc.rq)
        finally:
            if sc.prefer_cell:
                self.gpu.debug_cell_min_waves(-1)

    def scenario(self, name):
        if name in self.broken:
            raise self.broken[name]
        return self.torch_cases[name] if name in self.torch_cases else self.scenarios[name]

    def reference(self, sc):
        """ref[f] the synchronous way, through the same entry, with a device sync on both sides of the call"""
        torch = self.torch
        sc.ref, sc.got = [], [torch.empty_like(sc.out) for _ in range(FRAMES)]
        for f in range(FRAMES):
            sc.inp.copy_(sc.frames[f])
            sc.out.fill_(SENTINEL)
            torch.cuda.synchronize()
            self.call(sc, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            sc.ref.append(sc.out.clone())
        assert not same_bits(torch, sc.ref[0], sc.ref[1]), (sc.name, "two frames of distinct data give the same result")
        return sc

    def add(self, sc, timed=True):
        self.reference(sc)
        if timed:
            sc.inp.copy_(sc.frames[0])
            sc.ms = self.time_call(sc.name, lambda: self.call(sc, self.torch.cuda.current_stream().cuda_stream))
        self.scenarios[sc.name] = sc
        return sc

    def flagged_mask(self, sc):
        """the elements of `out` the plan leaves to the double-precision pass: those that keep the sentinel with that pass switched off"""
        torch = self.torch
        torch.cuda.synchronize()
        self.gpu.debug_skip_fixup(True)
        try:
            sc.inp.copy_(sc.frames[0])
            sc.out.fill_(SENTINEL)
            torch.cuda.synchronize()
            self.call(sc, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            self.gpu.debug_skip_fixup(False)
        return (sc.out == SENTINEL) & (sc.ref[0] != SENTINEL)

    # ---- the frame loop ----------------------------------------------------------------------------------------------
    def enqueue_frame(self, sc, caller, f, scale=1.0):
        """one frame on the caller's stream, no host synchronisation: poison, delayed producer, the call, consumer, buffer reuse"""
        with self.torch.cuda.stream(caller.stream):
            sc.inp.fill_(sc.poison)                    # stale reads are loud
            sc.out.fill_(SENTINEL)
            self.delay(caller.stream, scale)
            sc.inp.copy_(sc.frames[f])                 # the producer, still behind the delay when the call is enqueued
            self.call(sc, caller.handle)
            sc.got[f].copy_(sc.out)                    # the consumer, enqueued behind the call without a host wait
            sc.inp.fill_(sc.poison)                    # the next frame reuses the buffer

    def occupy_side_streams(self, blocker, stream, frames=FRAMES):
        """A second caller whose stream is busy for longer than the whole frame loop, then makes one call per side-stream slot of the
        library's pool: every fix-up pass the loop forks now queues behind a pass that waits for THIS stream, so it finishes long
        after its production kernel -- a consumer the library does not hold back until the pass has joined reads the sentinel."""
        self.delay(stream, frames + 2)
        with self.torch.cuda.stream(stream):
            blocker.inp.copy_(blocker.frames[0])
            for _ in range(4):
                self.call(blocker, stream.cuda_stream)

    def frame_loop(self, sc, caller, blocker=None):
        torch = self.torch
        torch.cuda.synchronize()
        if blocker is not None:
            self.occupy_side_streams(blocker, self.canary[1])
        for f in range(FRAMES):
            self.enqueue_frame(sc, caller, f)
        caller.stream.synchronize()                    # this stream only, never the device
        self.check(sc, "%s from %s%s" % (sc.name, caller.name, ", side streams occupied" if blocker is not None else ""))
        if blocker is not None:
            self.canary[1].synchronize()

    def check(self, sc, what):
        """every got[f] equals ref[f] bit for bit; the message says what the differing elements hold"""
        torch = self.torch
        bad = [f for f in range(FRAMES) if not same_bits(torch, sc.got[f], sc.ref[f])]
        if not bad:
            return
        mask = self.flagged_mask(sc) if sc.maskable else None
        lines = []
        for f in bad:
            got, ref = sc.got[f].reshape(-1), sc.ref[f].reshape(-1)
            diff = got.view(torch.int32) != ref.view(torch.int32)
            lines.append("frame %d: %d of %d elements differ; %d of them NaN, %d the sentinel, %s in the plan's flagged set%s" % (
                f, int(diff.sum()), diff.numel(), int((diff & got.isnan()).sum()), int((diff & (got == SENTINEL)).sum()),
                "n/a" if mask is None else int((diff & mask.reshape(-1)).sum()), "" if mask is None else " of %d" % int(mask.sum())))
        raise AssertionError("%s: not the bits of the synchronous call [%s %s]\n%s" % (what, sc.kernel, sc.info, "\n".join(lines)))


def same_bits(torch, a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ---- building the scenarios ----------------------------------------------------------------------------------------------
def request(gpu, W, H, sr, dr, ang, mode, off=(0.0, 0.0), policy=0):
    """isocenter at the image centre (+ off): the symmetric geometries have knife-edge pixels at 30 / 45 degrees"""
    rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1]), ang, mode=mode, policy=policy)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    return rq, lay


def rand_frames(torch, shape, seed, dtype=None):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == torch.uint8:
        return [torch.randint(0, 200, shape, dtype=torch.uint8, device="cuda", generator=gen) for _ in range(FRAMES)]
    return [torch.rand(shape, dtype=torch.float32, device="cuda", generator=gen) + 0.25 for _ in range(FRAMES)]


def plan_counts(gpu, rq, channels=1):
    m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq, channels))
    assert m, gpu.plan_shape(rq, channels)
    return int(m.group(1)), int(m.group(2))


def forward(h, name, geo, kernel, seed, flagged=False, prefer_cell=False, policy=0, timed=True):
    """resample_device on one (H, W) image.  geo = (W, H, srcRes, dstRes, angle, mode[, iso offset]); `kernel` must be in
    aai_last_kernel(); flagged: the plan must list pixels for the double-precision pass and must not be dense."""
    gpu, torch = h.gpu, h.torch
    W, H, sr, dr, ang, mode = geo[:6]
    rq, lay = request(gpu, W, H, sr, dr, ang, mode, geo[6] if len(geo) > 6 else (0.0, 0.0), policy)
    dW, dH = lay.dst_width, lay.dst_height
    inp = torch.empty((H, W), dtype=torch.float32, device="cuda")
    out = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    sc = Scenario(name, inp, out, rand_frames(torch, (H, W), seed),
                  lambda handle: gpu.resample_device(rq, inp.data_ptr(), W, out.data_ptr(), dW, handle), prefer_cell=prefer_cell, maskable=True)
    sc.rq, sc.lay = rq, lay
    if prefer_cell:
        gpu.debug_cell_min_waves(0)
    try:
        gpu.prepare(rq)
        sc.info = gpu.plan_shape(rq)
        sc.flagged, dense = plan_counts(gpu, rq)
    finally:
        gpu.debug_cell_min_waves(-1)
    h.add(sc, timed)
    sc.kernel = gpu.last_kernel()
    assert kernel in sc.kernel, (name, kernel, sc.kernel, sc.info)
    if flagged:
        assert sc.flagged > 0 and dense == 0, (name, sc.info)
    return sc


def first_runs_case(h, want, flagged):
    """the first RUNS_CASES geometry whose area request is served by the kernel `want` (and, if asked, lists pixels without being dense)"""
    gpu, torch = h.gpu, h.torch
    for (W, H, sr, dr, ang, off) in RUNS_CASES:
        rq, lay = request(gpu, W, H, sr, dr, ang, gpu.MODE_AREA, off)
        gpu.prepare(rq)
        n, dense = plan_counts(gpu, rq)
        if flagged and (n == 0 or dense):
            continue
        src = torch.rand((H, W), dtype=torch.float32, device="cuda")
        dst = torch.empty((lay.dst_height, lay.dst_width), dtype=torch.float32, device="cuda")
        gpu.resample_device(rq, src.data_ptr(), W, dst.data_ptr(), lay.dst_width, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        if want in gpu.last_kernel():
            return (W, H, sr, dr, ang, gpu.MODE_AREA, off)
    return None


def interleaved_u8(h, name, geo, channels, seed):
    gpu, torch = h.gpu, h.torch
    W, H, sr, dr, ang, mode = geo
    rq, lay = request(gpu, W, H, sr, dr, ang, mode)
    dW, dH, C = lay.dst_width, lay.dst_height, channels
    inp = torch.empty((H, W, C), dtype=torch.uint8, device="cuda")
    out = torch.empty((dH, dW, C), dtype=torch.float32, device="cuda")
    sc = Scenario(name, inp, out, rand_frames(torch, (H, W, C), seed, torch.uint8),
                  lambda handle: gpu.resample_interleaved_device(rq, C, inp.data_ptr(), W * C, out.data_ptr(), dW * C, handle, src_dtype=gpu.DTYPE_U8),
                  poison=255, maskable=True)
    gpu.prepare(rq, C)
    sc.info = gpu.plan_shape(rq, C)
    sc.flagged = plan_counts(gpu, rq, C)[0]
    h.add(sc)
    sc.kernel = gpu.last_kernel()
    return sc


def padded_batch(h, name, geo, seed, batch=3):
    """a batch with row and image padding on both sides: the padding of `out` keeps the sentinel"""
    gpu, torch = h.gpu, h.torch
    W, H, sr, dr, ang, mode = geo
    rq, lay = request(gpu, W, H, sr, dr, ang, mode)
    dW, dH = lay.dst_width, lay.dst_height
    sstride, dstride = W + 5, dW + 3
    simg, dimg = sstride * H + 11, dstride * dH + 17
    inp = torch.empty(batch * simg, dtype=torch.float32, device="cuda")
    out = torch.empty(batch * dimg, dtype=torch.float32, device="cuda")
    sc = Scenario(name, inp, out, rand_frames(torch, (batch * simg,), seed),
                  lambda handle: gpu.resample_device(rq, inp.data_ptr(), sstride, out.data_ptr(), dstride, handle, batch=batch,
                                                     src_image_stride=simg, dst_image_stride=dimg), maskable=True)
    gpu.prepare(rq)
    sc.info = gpu.plan_shape(rq)
    sc.flagged = plan_counts(gpu, rq)[0]
    h.add(sc)
    sc.kernel = gpu.last_kernel()
    sc.valid = torch.zeros(batch * dimg, dtype=torch.bool, device="cuda")
    for b in range(batch):
        sc.valid[b * dimg:b * dimg + dstride * dH].view(dH, dstride)[:, :dW] = True
    for ref in sc.ref:
        assert bool((ref[~sc.valid] == SENTINEL).all()) and bool((ref[sc.valid] >= 0.0).all()), name
    return sc


def row_band(h, name, geo, rows, seed):
    """dst rows [rows[0], rows[1]) from a buffer that holds only their source footprint; the reference is checked against the rows of
    the synchronous full-image call"""
    gpu, torch = h.gpu, h.torch
    W, H, sr, dr, ang, mode = geo
    rq, lay = request(gpu, W, H, sr, dr, ang, mode)
    dW, dH = lay.dst_width, lay.dst_height
    r0, r1 = rows
    a, b = gpu.band_source_rows(rq, r0, r1)
    assert 0 <= a < b <= H
    full = rand_frames(torch, (H, W), seed)
    inp = torch.empty((b - a, W), dtype=torch.float32, device="cuda")
    out = torch.empty((r1 - r0, dW), dtype=torch.float32, device="cuda")
    sc = Scenario(name, inp, out, [x[a:b].contiguous() for x in full],
                  lambda handle: gpu.resample_band_device(rq, r0, r1, inp.data_ptr(), W, out.data_ptr(), dW, handle), maskable=True)
    gpu.prepare(rq)
    sc.info = gpu.plan_shape(rq)
    sc.flagged = plan_counts(gpu, rq)[0]
    h.add(sc)
    sc.kernel = gpu.last_kernel()
    whole = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    for f in range(FRAMES):
        gpu.resample_device(rq, full[f].data_ptr(), W, whole.data_ptr(), dW, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert same_bits(torch, sc.ref[f], whole[r0:r1]), (name, f)
    return sc


def adjoint(h, name, geo, seed, planned=False, channels=1, kernel="", listed=False):
    """the adjoint entries: inp = gdst [dH, dW(, C)], out = gsrc [H, W(, C)]"""
    gpu, torch = h.gpu, h.torch
    W, H, sr, dr, ang, mode = geo
    rq, lay = request(gpu, W, H, sr, dr, ang, mode)
    dW, dH, C = lay.dst_width, lay.dst_height, channels
    tail = (C,) if C > 1 else ()
    inp = torch.empty((dH, dW) + tail, dtype=torch.float32, device="cuda")
    out = torch.empty((H, W) + tail, dtype=torch.float32, device="cuda")
    if C > 1:
        enqueue = lambda handle: gpu.adjoint_interleaved_device(rq, C, inp.data_ptr(), dW * C, out.data_ptr(), W * C, handle, planned=planned)
    else:
        enqueue = lambda handle: gpu.adjoint_device(rq, inp.data_ptr(), dW, out.data_ptr(), W, handle, planned=planned)
    sc = Scenario(name, inp, out, rand_frames(torch, (dH, dW) + tail, seed), enqueue)
    if planned == "any":
        gpu.adjoint_rotated_prepare(rq)
    elif planned:
        gpu.adjoint_prepare(rq)
    sc.info = gpu.plan_shape(rq)
    h.add(sc)
    sc.kernel = gpu.last_kernel()
    assert kernel in sc.kernel and (not listed or sc.kernel.endswith("+listed")), (name, kernel, sc.kernel, sc.info)
    for ref in sc.ref:
        assert bool((ref >= 0.0).all()), name              # every element written: weights and gradients are non-negative
    return sc
