#!/usr/bin/env python3
"""Time resample-and-convert (include/ext/aai_convert.h) next to the library's own forwarding route and next to what a caller had to do
without it.

One fresh child process per geometry (4096^2 -> 4096^2, 2048^2 and 1024^2, at 0 and 180 degrees; area mode, one image); in it one row per
source type (u8, u16) x channel count (1, 3, 4) x output type (f16, bf16, f32) x layout (interleaved; planar with channels), the legs of
a row taking turns:
  (a)  aai_resample_convert_device: the entry as shipped (the kernel it ran is named at the end of the row)
  (b)  what a caller does today: aai_resample_interleaved_device into a preallocated fp32 NHWC tensor, then torch mul / add per channel,
       permute().contiguous() for planar, .to(out dtype)
  (c)  the library's forwarding route for the same request, from its two stages: (c1) aai_resample_interleaved_device into dense fp32 --
       the launches enqueue() makes -- plus (c2) the stream-ordered scratch and aai_convert_store_kernel.  No request reaches the
       forwarding route at a direct-route geometry, so (c2) is measured on the BILINEAR request of the same geometry, which forwards and
       has the same output: (c2) = convert entry (bilinear) - aai_resample_interleaved_device (bilinear), medians.
3 warm-up launches of each leg, then N (default 24) timed launches of each between device events; per leg the median and the 10th..90th
percentile.  A row is FASTER where (a) beats (c) beyond the recorded spread: p90(a) < (c) built from the favourable ends, p10(c1) +
p10(convert bilinear) - p90(fp32 bilinear).  The verdict is per CLASS -- source type x output type x layout x "at most 64 / more than 64
outputs per strip" x rotation: a class keeps the direct route only if every row of it is faster in every run (axis_convert_can_serve,
csrc/aai_axis_convert.hip).  The verdict column only means something for rows whose (a) ran aai_axis_convert_kernel.

usage: python tools/convert_time.py [--launches N] [--runs R] [--out FILE]      (the table also goes to stdout; profiles/convert_time.txt)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle, most outputs per strip is above 64)
GEOMETRIES = [("1:1", 4096, 4096, 1.0, 1.0, 0.0, True), ("1:1@180", 4096, 4096, 1.0, 1.0, 180.0, True), ("2:1", 4096, 4096, 2.0, 1.0, 0.0, True),
              ("2:1@180", 4096, 4096, 2.0, 1.0, 180.0, True), ("4:1", 4096, 4096, 4.0, 1.0, 0.0, False), ("4:1@180", 4096, 4096, 4.0, 1.0, 180.0, False)]
TYPES = ("u8", "u16")
CHANNELS = (1, 3, 4)
OUTS = ("f16", "bf16", "f32")
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)


def child(name, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang, _ = [g for g in GEOMETRIES if g[0] == name][0]
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = aai.make_request(W, H, sr, dr, iso, ang)
    rqs = aai.make_request(W, H, sr, dr, iso, ang, mode=aai.MODE_BILINEAR)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    for tname in TYPES:
        dt, top, esz = (aai.DTYPE_U8, 255.0, 1) if tname == "u8" else (aai.DTYPE_U16, 65535.0, 2)
        for C in CHANNELS:
            x = torch.randint(0, 256, (H, W * C * esz), dtype=torch.uint8, device="cuda", generator=gen)      # every bit pattern: the full range
            y32, y32s = torch.empty((dH, dW, C), dtype=torch.float32, device="cuda"), torch.empty((dH, dW, C), dtype=torch.float32, device="cuda")
            scale = [1.0 / (top * s) for s in STD[:C]]
            offset = [-m / s for m, s in zip(MEAN[:C], STD[:C])]
            tscale, toffset = torch.tensor(scale, device="cuda"), torch.tensor(offset, device="cuda")
            aai.prepare(rq, C)
            aai.prepare(rqs, C)
            for oname in OUTS:
                ot, tdt = {"f16": (aai.HALF_F16, torch.float16), "bf16": (aai.HALF_BF16, torch.bfloat16), "f32": (aai.DTYPE_F32, torch.float32)}[oname]
                for planar in ((False, True) if C > 1 else (False,)):
                    cv = aai.make_convert(C, ot, planar, scale, offset)
                    ya, ys = torch.empty(dH * dW * C, dtype=tdt, device="cuda"), torch.empty(dH * dW * C, dtype=tdt, device="cuda")
                    dstride = dW if planar else dW * C
                    kernel = {}

                    def convert(r, dst, key):
                        aai.resample_convert_device(r, C, x.data_ptr(), W * C, dst.data_ptr(), dstride, dt, cv, st, dst_plane_stride=dW * dH)
                        kernel[key] = aai.last_kernel()

                    def fp32(r, dst):
                        aai.resample_interleaved_device(r, C, x.data_ptr(), W * C, dst.data_ptr(), dW * C, st, src_dtype=dt)

                    def leg_b():
                        fp32(rq, y32)
                        v = y32.mul(tscale).add_(toffset)
                        if planar:
                            v = v.permute(2, 0, 1).contiguous()
                        kernel["b"] = v.to(tdt)

                    runs = {"a": lambda: convert(rq, ya, "a"), "b": leg_b, "c1": lambda: fp32(rq, y32), "is": lambda: convert(rqs, ys, "is"), "fs": lambda: fp32(rqs, y32s)}
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
                    faster = hi["a"] < c_low
                    assert kernel["is"].endswith("+converted"), kernel["is"]
                    print("ROW %-8s %-3s x%d %-4s %-4s %5dx%-5d -> %5dx%-5d  (a) convert entry %s  (b) fp32 entry + torch mul/add%s/to %s  (c1) fp32 entry %s  "
                          "convert entry, bilinear %s  fp32 entry, bilinear %s  (c2) %6.1f us  (c) = c1 + c2 %7.1f us (at best %.1f)  (a)/(c) %5.2f  (a)/(b) %5.2f  %s  [%s]" % (
                              name, tname, C, oname, "nchw" if planar else "nhwc", W, H, dW, dH, cell("a"), "/permute" if planar else "", cell("b"), cell("c1"), cell("is"),
                              cell("fs"), c2, c, c_low, med["a"] / c, med["a"] / med["b"], "FASTER" if faster else "NOT faster beyond the spread", kernel["a"]), flush=True)
                    del ya, ys
            del x, y32, y32s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 timed launches")
    if args.child:
        child(args.child, args.launches)
        return 0
    lines = ["# median (10th..90th percentile) of %d launches each, device events, the legs taking turns, one process per geometry, area mode, one image" % args.launches]
    print(lines[0], flush=True)
    verdict = {}      # class -> [every row of run r faster, ...], worst and best (a)/(c)
    for run in range(1, args.runs + 1):
        lines.append("# run %d" % run)
        print(lines[-1], flush=True)
        for g in GEOMETRIES:
            # a fresh process per geometry, under its own time limit; a geometry that fails ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", g[0]], capture_output=True, text=True, timeout=420)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode or 1
            for ln in r.stdout.splitlines():
                if not ln.startswith("ROW "):
                    continue
                ln = ln[4:]
                print(ln, flush=True)
                lines.append(ln)
                f = ln.split()
                key = (f[1], f[3], f[4], "more than 64 per strip" if g[6] else "at most 64 per strip", "180 degrees" if g[5] else "0 degrees")
                ratio = float(ln.split("(a)/(c)")[1].split()[0])
                v = verdict.setdefault(key, {"runs": [True] * args.runs, "lo": ratio, "hi": ratio})
                v["runs"][run - 1] &= "NOT faster" not in ln
                v["lo"], v["hi"] = min(v["lo"], ratio), max(v["hi"], ratio)
            if args.out:                   # (rewritten geometry by geometry: a run that is cut short keeps what it measured)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    lines.append("# classes: source, output, layout, outputs per strip, rotation: (a)/(c) over the rows of both runs; faster beyond the spread in every row of run 1, 2, ...")
    for key in sorted(verdict):
        v = verdict[key]
        lines.append("CLASS %-3s %-4s %-4s %-22s %-11s  (a)/(c) %.2f..%.2f  %s  %s" % (key + (v["lo"], v["hi"], " ".join("yes" if r else "no" for r in v["runs"]),
                                                                                  "KEEP direct" if all(v["runs"]) else "FORWARD")))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
