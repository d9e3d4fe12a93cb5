#!/usr/bin/env python3
"""Time the half-precision path (include/aai_half.h) next to the fp32 entry and next to what a caller had to do without it.

Three legs taking turns in one fresh child process per row (a row = a geometry and an element type, area mode):
  (a) aai_resample_batch_device_f32 on an fp32 copy of the images (the caller who holds fp32 anyway)
  (b) aai_resample_half_batch_device on the half images
  (c) widen + (a) + narrow written with torch into preallocated tensors (x32.copy_(x16); the fp32 entry; y16.copy_(y32)): the caller
      who holds half images and has only the fp32 entry
3 warm-up launches of each, then N (default 24) timed launches of each between device events; reported per leg: median and
10th..90th percentile; then the ratios of the medians (b)/(c) -- the rule: below 1 on every row the direct route serves -- and
(b)/(a), which is recorded and not gated; then the kernel aai_last_kernel() names for (b).

usage: python tools/half_time.py [--launches N] [--out FILE]      (the table also goes to stdout; profiles/half_time.txt)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle, batch)
GEOMETRIES = [("4:1", 8192, 8192, 4.0, 1.0, 0.0, 4), ("4:1@180", 8192, 8192, 4.0, 1.0, 180.0, 4), ("2:1", 8192, 8192, 2.0, 1.0, 0.0, 1),
              ("1:1", 4096, 4096, 1.0, 1.0, 0.0, 1), ("1:2", 2048, 2048, 1.0, 2.0, 0.0, 1), ("4:1@90", 8192, 8192, 4.0, 1.0, 90.0, 1),
              ("cfg3", 8192, 8192, 8192.0, 2731.0, 17.5, 1)]
TYPES = ("f16", "bf16")


def child(name, tname, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang, B = [g for g in GEOMETRIES if g[0] == name][0]
    dtype, ht = (torch.float16, aai.HALF_F16) if tname == "f16" else (torch.bfloat16, aai.HALF_BF16)
    rq = aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    x32 = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    for b in range(B):
        aai.synth_device(x32[b].data_ptr(), W, H, W, 1 + b, st)
    x16 = x32.to(dtype)
    x32.copy_(x16)                         # (a) and (c) see the values (b) sees
    scratch32 = torch.empty_like(x32)
    y32, ya = torch.empty((B, dH, dW), dtype=torch.float32, device="cuda"), torch.empty((B, dH, dW), dtype=torch.float32, device="cuda")
    yb, yc = torch.empty((B, dH, dW), dtype=dtype, device="cuda"), torch.empty((B, dH, dW), dtype=dtype, device="cuda")
    aai.prepare(rq)
    kernel = {}

    def fp32(src, dst):
        aai.resample_device(rq, src.data_ptr(), W, dst.data_ptr(), dW, st, batch=B, src_image_stride=W * H, dst_image_stride=dW * dH)

    def leg_b():
        aai.resample_half_device(rq, x16.data_ptr(), W, yb.data_ptr(), dW, ht, st, batch=B, src_image_stride=W * H, dst_image_stride=dW * dH)
        kernel["b"] = aai.last_kernel()

    def leg_c():
        scratch32.copy_(x16)
        fp32(scratch32, y32)
        yc.copy_(y32)

    runs = {"a": lambda: fp32(x32, ya), "b": leg_b, "c": leg_c}
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
            times[key].append(a.elapsed_time(b))
    t = {k: np.array(v) for k, v in times.items()}
    cell = lambda v: "%8.3f ms (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))
    differ = float((yb.view(torch.int16) != yc.view(torch.int16)).float().mean())
    print("%-8s %-4s %dx %5dx%-5d -> %5dx%-5d  (a) fp32 entry %s  (b) half entry %s  (c) torch widen + fp32 + narrow %s  (b)/(c) %5.2f  (b)/(a) %5.2f  "
          "(b) differs from (c) in %.4f %% of elements  [%s]" % (
              name, tname, B, W, H, dW, dH, cell(t["a"]), cell(t["b"]), cell(t["c"]), np.median(t["b"]) / np.median(t["c"]),
              np.median(t["b"]) / np.median(t["a"]), 100 * differ, kernel["b"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 timed launches")
    if args.child:
        child(args.child[0], args.child[1], args.launches)
        return 0
    lines = ["# median (10th..90th percentile) of %d launches each, device events, the three legs taking turns, one process per row, area mode" % args.launches]
    print(lines[0], flush=True)
    for g in GEOMETRIES:
        for tname in TYPES:
            # a fresh process per row, under its own time limit; a row that fails ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", g[0], tname],
                               capture_output=True, text=True, timeout=240)
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
