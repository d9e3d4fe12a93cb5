#!/usr/bin/env python3
"""Time the half-precision interleaved path (include/aai_half_interleaved.h) next to the two detours a caller of the torch operator
had without it, and next to the library's own forwarding route.

One fresh child process per geometry; in it one row per channel count and element type (area mode, one channels_last image of
4096 x 4096 pixels), the legs of a row taking turns:
  (a)  aai_resample_half_interleaved_device on the NHWC storage (what resample(x, half="channels_last") runs)
  (p)  the planar detour: resample(x, half=True) on the channels_last tensor -- an NHWC -> NCHW copy, C single-channel images,
       a planar result
  (f)  the fp32 detour: x.float() -> resample() on the fp32 channels_last tensor (aai_resample_interleaved_device) -> .to(dtype)
  (c)  the library's forwarding route for the same request, from its stages: (c1) aai_resample_interleaved_device on an fp32 copy
       into fp32 -- the launches enqueue() makes -- plus (c2) the stream-ordered scratch, the widening and the narrowing kernel.  No
       request reaches the forwarding route at a direct-route geometry, so (c2) is measured on the BILINEAR request of the same
       geometry, which forwards and has the same source and output size: (c2) = half interleaved entry (bilinear) - fp32 interleaved
       entry (bilinear), medians.
3 warm-up launches of each leg, then N (default 24) timed launches of each between device events; per leg the median and the
10th..90th percentile.  A row KEEPS the direct route where (a) is faster than (c) beyond the recorded spread: p90(a) < (c) built
from the favourable ends, p10(c1) + p10(half bilinear) - p90(fp32 bilinear).  (The rows that decide the rule of
aai::axis_narrow_can_serve are taken with every class on the direct kernel; the name in brackets says what (a) ran.)

usage: python tools/half_interleaved_time.py [--launches N] [--out FILE] [--only NAME,...]
       (the table also goes to stdout; profiles/half_interleaved_time.txt)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle): 4096^2 -> 4096^2, 2048^2, 1024^2, forwards and backwards
GEOMETRIES = [("1:1", 4096, 4096, 1.0, 1.0, 0.0), ("1:1@180", 4096, 4096, 1.0, 1.0, 180.0), ("2:1", 4096, 4096, 2.0, 1.0, 0.0),
              ("2:1@180", 4096, 4096, 2.0, 1.0, 180.0), ("4:1", 4096, 4096, 4.0, 1.0, 0.0), ("4:1@180", 4096, 4096, 4.0, 1.0, 180.0)]
TYPES = ("f16", "bf16")
CHANNELS = (3, 4)


def row(name, tname, C, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    dtype, ht = (torch.float16, aai.HALF_F16) if tname == "f16" else (torch.bfloat16, aai.HALF_BF16)
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = aai.make_request(W, H, sr, dr, iso, ang)
    rqs = aai.make_request(W, H, sr, dr, iso, ang, mode=aai.MODE_BILINEAR)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.rand((1, C, H, W), device="cuda", generator=gen) + 0.25).to(dtype).contiguous(memory_format=torch.channels_last)
    x32 = x.float()
    assert x32.is_contiguous(memory_format=torch.channels_last) and not x32.is_contiguous()
    ya, ys = torch.empty((dH, dW * C), dtype=dtype, device="cuda"), torch.empty((dH, dW * C), dtype=dtype, device="cuda")
    y32, y32s = torch.empty((dH, dW * C), dtype=torch.float32, device="cuda"), torch.empty((dH, dW * C), dtype=torch.float32, device="cuda")
    aai.prepare(rq, C)
    aai.prepare(rqs, C)
    aai.prepare(rq, 1)
    kernel, keep = {}, {}

    def half_entry(r, dst, key):
        aai.resample_half_interleaved_device(r, C, x.data_ptr(), W * C, dst.data_ptr(), dW * C, ht, st)
        kernel[key] = aai.last_kernel()

    def fp32_entry(r, dst):
        aai.resample_interleaved_device(r, C, x32.data_ptr(), W * C, dst.data_ptr(), dW * C, st)

    def leg_p():
        keep["p"] = aai.resample(x, sr, dr, iso, ang, half=True)[0]

    def leg_f():
        keep["f"] = aai.resample(x.float(), sr, dr, iso, ang)[0].to(dtype)

    runs = {"a": lambda: half_entry(rq, ya, "a"), "p": leg_p, "f": leg_f, "c1": lambda: fp32_entry(rq, y32), "hs": lambda: half_entry(rqs, ys, "hs"),
            "fs": lambda: fp32_entry(rqs, y32s)}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    assert keep["f"].is_contiguous(memory_format=torch.channels_last) and keep["p"].is_contiguous()
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
    c2 = med["hs"] - med["fs"]
    c = med["c1"] + c2
    c_low = lo["c1"] + lo["hs"] - hi["fs"]
    assert kernel["hs"].endswith("+widened"), kernel["hs"]
    # (a) against the detours' results: the same image up to one unit in the last place
    got = ya.view(dH, dW, C).permute(2, 0, 1)
    apart = max(int((got.view(torch.int16).int() - keep[k][0].view(torch.int16).int()).abs().max()) for k in ("p", "f"))
    print("%-8s %-4s x%d %5dx%-5d -> %5dx%-5d  (a) half interleaved entry %s  (p) planar detour, half=True %s  (f) fp32 detour, float / resample / to %s  "
          "(c1) fp32 interleaved entry %s  half entry, bilinear %s  fp32 entry, bilinear %s  (c2) %6.1f us  (c) = c1 + c2 %7.1f us (at best %.1f)  "
          "(a)/(c) %5.2f  (a)/(p) %5.2f  (a)/(f) %5.2f  %s  at most %d ulp from the detours  [%s]" % (
              name, tname, C, W, H, dW, dH, cell("a"), cell("p"), cell("f"), cell("c1"), cell("hs"), cell("fs"), c2, c, c_low, med["a"] / c,
              med["a"] / med["p"], med["a"] / med["f"], "KEEP direct" if hi["a"] < c_low else "NOT faster beyond the spread", apart, kernel["a"]), flush=True)


def child(name, launches):
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    for tname in TYPES:
        for C in CHANNELS:
            row(name, tname, C, launches)
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated geometry names (default: all)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 timed launches")
    if args.child:
        child(args.child, args.launches)
        return 0
    names = [g[0] for g in GEOMETRIES]
    if args.only:
        names = [n for n in names if n in args.only.split(",")]
    lines = ["# median (10th..90th percentile) of %d launches each, device events, the legs taking turns, one process per geometry, area mode, one image" % args.launches]
    print(lines[0], flush=True)
    for name in names:
        # a fresh process per geometry, under its own time limit; a geometry that fails ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", name], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return r.returncode or 1
        for line in [ln for ln in r.stdout.splitlines() if ln.startswith(name + " ")]:
            print(line, flush=True)
            lines.append(line)
        if args.out:                   # (rewritten geometry by geometry: a run that is cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
