#!/usr/bin/env python3
"""Time the reference-precision path (include/aai_f64.h) next to the fp32-I/O code that does the same double-precision pair
evaluations, on the geometries of the adjoint identity test (tools/adjoint_time.py: GEOMETRIES), both modes.

Four legs taking turns in one fresh child process per row:
  (a) the fp32-I/O forward under AAI_POLICY_DOUBLE_PRECISION (aai_resample_device_f32; at multiples of 90 degrees the separable kernel)
  (b) aai_resample_batch_device_f64, the f64 forward
  (c) aai_adjoint_batch_device_f32, the general adjoint (fp64 arithmetic, fp32 images)
  (d) aai_adjoint_batch_device_f64, the f64 adjoint
3 warm-up launches of each, then N (default 24) timed launches of each between device events; reported per leg: median and
10th..90th percentile; then the ratios of the medians (b)/(a) and (d)/(c), and the largest deviation of (b) from (a) and of (d) from
(c) relative to max(|f64|, 1e-3 max|f64|) -- the fp32 legs' rounding, a plausibility check of the legs, not a parity test.

usage: python tools/f64_time.py [--launches N] [--out FILE]      (the table also goes to stdout; profiles/f64_time.txt)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle): tools/adjoint_time.py GEOMETRIES = tests/test_adjoint_gpu.py AT_SIZE
GEOMETRIES = [("cfg3", 8192, 8192, 8192.0, 2731.0, 17.5), ("wide8", 8192, 8192, 8.0, 1.0, 17.5), ("up2", 2048, 2048, 1.0, 2.0, 30.0),
              ("axis4", 4096, 4096, 4.0, 1.0, 0.0), ("quarter2.5", 4096, 4096, 2.5, 1.0, 90.0)]


def child(name, mode, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    fwd32 = aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=aai.POLICY_REFERENCE | aai.POLICY_DOUBLE_PRECISION)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((H, W), dtype=torch.float32, device="cuda")
    y = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    aai.synth_device(x.data_ptr(), W, H, W, 1, st)
    aai.synth_device(y.data_ptr(), dW, dH, dW, 2, st)
    x64, y64 = x.double(), y.double()
    wx, wty = torch.empty_like(y), torch.empty_like(x)
    wx64, wty64 = torch.empty_like(y64), torch.empty_like(x64)
    aai.prepare(fwd32)
    kernels = {}

    def leg(key, fn):
        def run():
            fn()
            kernels[key] = aai.last_kernel().split("(")[0].strip()
        return run

    runs = {"a": leg("a", lambda: aai.resample_device(fwd32, x.data_ptr(), W, wx.data_ptr(), dW, st)),
            "b": leg("b", lambda: aai.resample_device_f64(rq, x64.data_ptr(), W, wx64.data_ptr(), dW, st)),
            "c": leg("c", lambda: aai.adjoint_device(rq, y.data_ptr(), dW, wty.data_ptr(), W, st)),
            "d": leg("d", lambda: aai.adjoint_device_f64(rq, y64.data_ptr(), dW, wty64.data_ptr(), W, st))}
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

    def dev(lo, hi):
        floor = 1e-3 * float(hi.abs().max())
        return float(((lo.double() - hi).abs() / hi.abs().clamp_min(max(floor, 1e-300))).max())
    print("%-10s %-4s %5dx%-5d -> %5dx%-5d  (a) forward fp32 I/O %s  (b) forward f64 %s  (b)/(a) %6.2f  (c) adjoint fp32 I/O %s  (d) adjoint f64 %s  "
          "(d)/(c) %5.2f  dev (a):(b) %.1e (c):(d) %.1e  [%s; %s; %s; %s]" % (
              name, "area" if mode == aai.MODE_AREA else "fast", W, H, dW, dH, cell(t["a"]), cell(t["b"]), np.median(t["b"]) / np.median(t["a"]),
              cell(t["c"]), cell(t["d"]), np.median(t["d"]) / np.median(t["c"]), dev(wx, wx64), dev(wty, wty64),
              kernels["a"], kernels["b"], kernels["c"], kernels["d"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 timed launches")
    if args.child:
        child(args.child[0], int(args.child[1]), args.launches)
        return 0
    lines = ["# median (10th..90th percentile) of %d launches each, device events, the four legs taking turns, one process per row" % args.launches]
    print(lines[0], flush=True)
    for g in GEOMETRIES:
        for mode in (1, 2):
            # a fresh process per row, under its own time limit; a row that fails ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", g[0], str(mode)],
                               capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode or 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith(g[0])][-1]
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
