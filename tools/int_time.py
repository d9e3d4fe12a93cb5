#!/usr/bin/env python3
"""Time the integer path (include/aai_int.h) next to what a caller had to do without it and next to the library's own forwarding route.

One fresh child process per row (a row = a geometry, an element type and a channel count; area mode, one image), the legs taking turns:
  (a)  aai_resample_int_batch_device: the integer entry (the direct kernel on every row here)
  (b)  what a user does today: aai_resample_interleaved_device into a preallocated fp32 tensor, then torch round().clamp_(0, max).to(dtype)
  (c)  the library's forwarding route for the same request, from its two stages: (c1) aai_resample_interleaved_device into fp32 -- the
       launches enqueue() makes -- plus (c2) the stream-ordered scratch and the conversion kernel (aai_narrow_store_kernel).  No request
       reaches the forwarding route at a direct-route geometry, so (c2) is measured on the BILINEAR request of the same geometry,
       which forwards and has the same output size: (c2) = integer entry (bilinear) - aai_resample_interleaved_device (bilinear), medians.
3 warm-up launches of each leg, then N (default 24) timed launches of each between device events; per leg the median and the
10th..90th percentile.  A row KEEPS the direct route where (a) is faster than (c) beyond the recorded spread: p90(a) < (c) built from
the favourable ends, p10(c1) + p10(int bilinear) - p90(fp32 bilinear).

usage: python tools/int_time.py [--launches N] [--out FILE]      (the table also goes to stdout; profiles/int_time.txt)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle)
GEOMETRIES = [("4:1", 8192, 8192, 4.0, 1.0, 0.0), ("4:1@180", 8192, 8192, 4.0, 1.0, 180.0), ("1:1", 4096, 4096, 1.0, 1.0, 0.0), ("1:2", 2048, 2048, 1.0, 2.0, 0.0)]
TYPES = ("u8", "u16")
CHANNELS = (1, 3)


def child(name, tname, C, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    dt, top, bits = (aai.DTYPE_U8, 255, torch.uint8) if tname == "u8" else (aai.DTYPE_U16, 65535, torch.int16)
    out_dtype = torch.uint8
    if tname == "u16":
        # (a torch without a 16-bit unsigned conversion on the device: the user's pass then ends in int32, which only favours (b))
        try:
            out_dtype = torch.uint16
            torch.zeros(4, device="cuda").to(out_dtype)
        except (AttributeError, RuntimeError, TypeError):
            out_dtype = torch.int32
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = aai.make_request(W, H, sr, dr, iso, ang)
    rqs = aai.make_request(W, H, sr, dr, iso, ang, mode=aai.MODE_BILINEAR)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(0, 256, (H, W * C * (1 if tname == "u8" else 2)), dtype=torch.uint8, device="cuda", generator=gen).view(bits)      # every bit pattern: the full range
    ya, ys = torch.empty((dH, dW * C), dtype=bits, device="cuda"), torch.empty((dH, dW * C), dtype=bits, device="cuda")
    y32, y32s = torch.empty((dH, dW * C), dtype=torch.float32, device="cuda"), torch.empty((dH, dW * C), dtype=torch.float32, device="cuda")
    aai.prepare(rq, C)
    aai.prepare(rqs, C)
    kernel = {}

    def leg_a():
        aai.resample_int_device(rq, C, x.data_ptr(), W * C, ya.data_ptr(), dW * C, dt, st)
        kernel["a"] = aai.last_kernel()

    def fp32(r, dst):
        aai.resample_interleaved_device(r, C, x.data_ptr(), W * C, dst.data_ptr(), dW * C, st, src_dtype=dt)

    def leg_b():
        fp32(rq, y32)
        kernel["b"] = y32.round().clamp_(0, top).to(out_dtype)

    def leg_is():
        aai.resample_int_device(rqs, C, x.data_ptr(), W * C, ys.data_ptr(), dW * C, dt, st)
        kernel["is"] = aai.last_kernel()

    runs = {"a": leg_a, "b": leg_b, "c1": lambda: fp32(rq, y32), "is": leg_is, "fs": lambda: fp32(rqs, y32s)}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(launches):
        for key, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[key].append(a.elapsed_time(b) * 1e3)
    t = {k: np.array(v) for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in t.items()}
    lo = {k: float(np.percentile(v, 10)) for k, v in t.items()}
    hi = {k: float(np.percentile(v, 90)) for k, v in t.items()}
    cell = lambda k: "%7.1f us (%.1f..%.1f)" % (med[k], lo[k], hi[k])
    c2 = med["is"] - med["fs"]
    c = med["c1"] + c2
    c_low = lo["c1"] + lo["is"] - hi["fs"]
    keep = hi["a"] < c_low
    assert kernel["is"].endswith("+quantized"), kernel["is"]
    print("%-8s %-3s x%d %5dx%-5d -> %5dx%-5d  (a) int entry %s  (b) fp32 entry + torch round/clamp/to %s  (c1) fp32 entry %s  int entry, bilinear %s  fp32 entry, bilinear %s  "
          "(c2) %6.1f us  (c) = c1 + c2 %7.1f us (at best %.1f)  (a)/(c) %5.2f  (a)/(b) %5.2f  %s  [%s]" % (
              name, tname, C, W, H, dW, dH, cell("a"), cell("b"), cell("c1"), cell("is"), cell("fs"), c2, c, c_low, med["a"] / c, med["a"] / med["b"],
              "KEEP direct" if keep else "NOT faster beyond the spread", kernel["a"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 timed launches")
    if args.child:
        child(args.child[0], args.child[1], int(args.child[2]), args.launches)
        return 0
    lines = ["# median (10th..90th percentile) of %d launches each, device events, the legs taking turns, one process per row, area mode, one image" % args.launches]
    print(lines[0], flush=True)
    for g in GEOMETRIES:
        for tname in TYPES:
            for C in CHANNELS:
                # a fresh process per row, under its own time limit; a row that fails ends the run
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", g[0], tname, str(C)],
                                   capture_output=True, text=True, timeout=180)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    return r.returncode or 1
                line = [ln for ln in r.stdout.splitlines() if ln.startswith(g[0])][-1]
                print(line, flush=True)
                lines.append(line)
                if args.out:                   # (rewritten row by row: a run that is cut short keeps what it measured)
                    with open(args.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
