#!/usr/bin/env python3
"""Time the half-precision adjoint (include/aai_adjoint_half.h) next to the forwarding route it replaces at multiples of 90 degrees,
next to what the torch operator did before it, and next to the forward.

One fresh child process per geometry row; in it one line per mode (area, fast), element type (f16, bf16) and channel count (1, 3, 4),
one image, the legs of a line taking turns:
  (a)  aai_adjoint_half_device on the half gradient (what resample(..., half_backward=True) runs): the direct kernel
  (b)  the forwarding route for the same request, from its stages on buffers allocated beforehand: widen the half gradient into a dense
       fp32 image, the fp32 entry (aai_adjoint_rotated_batch_device_f32 for C = 1, aai_adjoint_planned_interleaved_device_f32 for C > 1),
       narrow the dense fp32 result.  No request reaches the library's forwarding route at a direct-route geometry and the library has no
       switch to force it, so the two conversions are torch's element-wise copy kernels (fp32.copy_(half), half.copy_(fp32)): the same
       bytes moved by one bandwidth-bound pass each, without the route's stream-ordered scratch allocation.  (b) is therefore a lower
       estimate of the forwarding route.
  (c)  what the torch operator's backward did: gy.float() (a fresh fp32 tensor), adjoint_device(planned="any") /
       adjoint_interleaved_device(planned="separable") into a fresh fp32 tensor, .to(dtype)
  (d)  the forward on the same tensors for scale: aai_resample_half_interleaved_device (its direct kernel at 0 / 180 degrees, its
       forwarding route at 90 / 270)
3 warm-up launches of each leg, then N (default 24) timed launches of each between device events; per leg the median and the
10th..90th percentile.  A CLASS of requests (geometry row = quadrant pair x up- / down-sampling, x channel count) keeps the direct route
only if (a)'s median is below (b)'s in every line of the class, in both runs; the verdict lines at the end of a run say so.

usage: python tools/adjoint_half_time.py [--launches N] [--runs R] [--out FILE] [--only NAME,...]
       (the table also goes to stdout; profiles/adjoint_half_time.txt holds two runs)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle)
GEOMETRIES = [("4:1@0", 4096, 4096, 4.0, 1.0, 0.0), ("2.5:1@90", 4096, 4096, 2.5, 1.0, 90.0), ("2:1@180", 4096, 4096, 2.0, 1.0, 180.0),
              ("x2@270", 2048, 2048, 1.0, 2.0, 270.0)]
MODES = ("area", "fast")
TYPES = ("f16", "bf16")
CHANNELS = (1, 3, 4)


def line(name, mode_name, tname, C, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    dtype, ht = (torch.float16, aai.HALF_F16) if tname == "f16" else (torch.bfloat16, aai.HALF_BF16)
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=aai.MODE_FAST if mode_name == "fast" else aai.MODE_AREA)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    gy = (torch.rand((dH, dW, C), device="cuda", generator=gen) - 0.5).to(dtype)
    x = (torch.rand((H, W, C), device="cuda", generator=gen) + 0.25).to(dtype)
    gx_a, gx_b = torch.empty((H, W, C), dtype=dtype, device="cuda"), torch.empty((H, W, C), dtype=dtype, device="cuda")
    gy32, gx32 = torch.empty((dH, dW, C), dtype=torch.float32, device="cuda"), torch.empty((H, W, C), dtype=torch.float32, device="cuda")
    y = torch.empty((dH, dW, C), dtype=dtype, device="cuda")
    aai.prepare(rq, C)
    aai.adjoint_rotated_prepare(rq)
    kernel, keep = {}, {}

    def fp32_entry(g32, out32):
        if C == 1:
            aai.adjoint_device(rq, g32.data_ptr(), dW, out32.data_ptr(), W, stream=st, planned="any")
        else:
            aai.adjoint_interleaved_device(rq, C, g32.data_ptr(), dW * C, out32.data_ptr(), W * C, stream=st, planned="separable")

    def leg_a():
        aai.adjoint_half_device(rq, C, gy.data_ptr(), dW * C, gx_a.data_ptr(), W * C, ht, stream=st)
        kernel["a"] = aai.last_kernel()

    def leg_b():
        gy32.copy_(gy)
        fp32_entry(gy32, gx32)
        kernel["b"] = aai.last_kernel()
        gx_b.copy_(gx32)

    def leg_c():
        g32 = gy.float()
        out32 = torch.empty((H, W, C), dtype=torch.float32, device="cuda")
        fp32_entry(g32, out32)
        keep["c"] = out32.to(dtype)

    def leg_d():
        aai.resample_half_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C, ht, st)
        kernel["d"] = aai.last_kernel()

    runs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
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
    cell = lambda k: "%7.1f us (%.1f..%.1f)" % (med[k], float(np.percentile(t[k], 10)), float(np.percentile(t[k], 90)))
    same = bool(torch.equal(gx_a.view(torch.int16), gx_b.view(torch.int16)) and torch.equal(gx_a.view(torch.int16), keep["c"].view(torch.int16)))
    print("%-9s %-4s %-4s x%d %5dx%-5d <- %5dx%-5d  (a) half adjoint entry %s  (b) forwarding from its stages %s  (c) float / fp32 adjoint / to %s  "
          "(d) half forward %s  (a)/(b) %5.2f  (a)/(c) %5.2f  (a)/(d) %5.2f  %s  bits %s  [%s | %s | %s]" % (
              name, mode_name, tname, C, W, H, dW, dH, cell("a"), cell("b"), cell("c"), cell("d"), med["a"] / med["b"], med["a"] / med["c"],
              med["a"] / med["d"], "a<b" if med["a"] < med["b"] else "a>=b", "equal" if same else "DIFFER", kernel["a"], kernel["b"], kernel["d"]), flush=True)


def child(name, launches):
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    for mode_name in MODES:
        for tname in TYPES:
            for C in CHANNELS:
                line(name, mode_name, tname, C, launches)
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--runs", type=int, default=2)
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
    lines = ["# median (10th..90th percentile) of %d launches each, device events, the legs taking turns, one process per geometry row, one image" % args.launches]
    print(lines[0], flush=True)
    for run in range(1, args.runs + 1):
        lines.append("# run %d" % run)
        print(lines[-1], flush=True)
        verdict = {}
        for name in names:
            # a fresh process per geometry row, under its own time limit; a row that fails ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", name], capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode or 1
            for ln in [ln for ln in r.stdout.splitlines() if ln.startswith(name + " ")]:
                print(ln, flush=True)
                lines.append(ln)
                C = ln.split()[3]
                verdict[name, C] = verdict.get((name, C), True) and " a<b " in ln and "bits equal" in ln
            if args.out:                   # (rewritten row by row: a run that is cut short keeps what it measured)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
        for (name, C), keep in sorted(verdict.items()):
            lines.append("# run %d class %s %s: %s" % (run, name, C, "(a) below (b) in every line" if keep else "(a) NOT below (b) in every line"))
            print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
