#!/usr/bin/env python3
"""Time the samplers' adjoint (aai_adjoint_sample_batch_device_f32, bilinear and bicubic) next to what it is planned against, on four
geometries.  A fresh child process per row (geometry x mode), each under its own time limit; in it 3 warm-up launches of every leg,
then N (default 24) timed launches of each between device events, the legs taking turns; reported: median and 10th..90th percentile.

  (a) the forward sampler (aai_resample_batch_device_f32 in the row's mode)
  (b) the new adjoint
  (c) bilinear rows only: the backward of torch's grid_sample (bilinear, border padding, fp32) on the same grid -- an atomic scatter,
      not deterministic; the grid is the forward's own sample points, read off by resampling two coordinate ramps
  (d) aai_adjoint_batch_device_f32 in AREA mode on the same geometry: the scale people already plan with

Beside the times: the candidates the gather visits per source pixel and how many of them carry weight, counted by the CPU replay
(tests/emulation/adjoint_sample_emulation.cpp, built with g++ on first use) on a 192 x 192 image of the same resolutions and angle.

usage: python tools/adjoint_sample_time.py [--launches N] [--out FILE]      (the table also goes to stdout)"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle)
GEOMETRIES = [("cfg3", 8192, 8192, 8192.0, 3426.0, 17.5), ("axis4", 4096, 4096, 4.0, 1.0, 0.0), ("up2", 2048, 2048, 1.0, 2.0, 30.0),
              ("up4x45", 4096, 4096, 1.0, 4.0, 45.0)]
MODE_NAME = {3: "bilinear", 4: "bicubic"}
COUNT_SIZE = 192


def candidate_counts(aai, sr, dr, ang, mode):
    """(candidates visited, candidates with weight) per source pixel on a COUNT_SIZE^2 image of the same geometry, by the CPU replay"""
    import numpy as np
    from area_average_interpolation_amd import _lib as L
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libaai_adjsampleemu.so")
    src = os.path.join(ROOT, "tests", "emulation", "adjoint_sample_emulation.cpp")
    deps = [src] + [os.path.join(ROOT, "area_average_interpolation_amd", "csrc", f) for f in ("aai_adjoint_sample_math.hpp", "aai_sample_math.hpp", "aai_plan.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    LL = ctypes.POINTER(ctypes.c_longlong)
    lib.aai_emu_adjoint_sample.restype = ctypes.c_int
    lib.aai_emu_adjoint_sample.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, LL, LL]
    n = COUNT_SIZE
    rq = aai.make_request(n, n, sr, dr, ((n - 1) / 2, (n - 1) / 2), ang, mode=mode)
    lay = aai.query(rq)[2]
    g = np.zeros((lay.dst_height, lay.dst_width), np.float32)
    out = np.zeros((n, n), np.float32)
    visited, weighted = ctypes.c_longlong(0), ctypes.c_longlong(0)
    assert lib.aai_emu_adjoint_sample(ctypes.byref(rq), 1, g.ctypes.data, out.ctypes.data, ctypes.byref(visited), ctypes.byref(weighted)) == 0
    return visited.value / (n * n), weighted.value / (n * n)


def child(name, mode, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    area = aai.make_request(W, H, sr, dr, iso, ang, mode=aai.MODE_AREA)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((H, W), dtype=torch.float32, device="cuda")
    y = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    aai.synth_device(x.data_ptr(), W, H, W, 1, st)
    aai.synth_device(y.data_ptr(), dW, dH, dW, 2, st)
    wx = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    wty = torch.empty((H, W), dtype=torch.float32, device="cuda")
    wty_area = torch.empty((H, W), dtype=torch.float32, device="cuda")
    aai.prepare(rq)
    kernels = {}

    def run_fwd():
        aai.resample_device(rq, x.data_ptr(), W, wx.data_ptr(), dW, st)
        kernels["fwd"] = aai.last_kernel()

    def run_adj():
        aai.adjoint_sample_device(rq, y.data_ptr(), dW, wty.data_ptr(), W, st)
        kernels["adj"] = aai.last_kernel()

    def run_area():
        aai.adjoint_device(area, y.data_ptr(), dW, wty_area.data_ptr(), W, st)
        kernels["area"] = aai.last_kernel()

    runs = {"fwd": run_fwd, "adj": run_adj, "area": run_area}
    if mode == aai.MODE_BILINEAR:
        # the forward's own sample points: the bilinear forward of the two coordinate ramps (exact up to fp32 rounding; points outside
        # the extent come out as 0, which only moves where that leg scatters to)
        ramp = torch.arange(W, dtype=torch.float32, device="cuda").expand(H, W).contiguous()
        sx = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
        aai.resample_device(rq, ramp.data_ptr(), W, sx.data_ptr(), dW, st)
        ramp = torch.arange(H, dtype=torch.float32, device="cuda")[:, None].expand(H, W).contiguous()
        sy = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
        aai.resample_device(rq, ramp.data_ptr(), W, sy.data_ptr(), dW, st)
        grid = torch.stack(((2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1), dim=-1)[None]
        del ramp, sx, sy
        xg = x.clone()[None, None].requires_grad_(True)
        yg = torch.nn.functional.grid_sample(xg, grid, mode="bilinear", padding_mode="border", align_corners=False)
        gy = y[None, None]

        def run_grid():
            xg.grad = None
            yg.backward(gy, retain_graph=True)
        runs["grid"] = run_grid
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
    cell = lambda v: "%9.3f ms (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))
    visited, weighted = candidate_counts(aai, sr, dr, ang, mode)
    print("%-7s %-8s %5dx%-5d -> %5dx%-5d  (a) forward %s  (b) adjoint %s  (c) grid_sample backward %s  (d) area adjoint %s  (b)/(a) %6.2f  "
          "(b)/(d) %5.2f  candidates per source pixel %7.2f, with weight %7.2f (%.1f x)  [%s; %s; %s]" % (
              name, MODE_NAME[mode], W, H, dW, dH, cell(t["fwd"]), cell(t["adj"]), cell(t["grid"]) if "grid" in t else "%28s" % "-", cell(t["area"]),
              np.median(t["adj"]) / np.median(t["fwd"]), np.median(t["adj"]) / np.median(t["area"]), visited, weighted, visited / max(weighted, 1e-30),
              kernels["fwd"], kernels["adj"], kernels["area"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 timed launches")
    if args.child:
        child(args.child[0], int(args.child[1]), args.launches)
        return 0
    lines = ["# median (10th..90th percentile) of %d launches each, device events, the legs taking turns, one process per row; candidates: CPU "
             "replay on a %d x %d image of the same resolutions and angle" % (args.launches, COUNT_SIZE, COUNT_SIZE)]
    print(lines[0], flush=True)
    for g in GEOMETRIES:
        for mode in (3, 4):
            # a fresh process per row, under its own time limit; a row that fails ends the run
            r = subprocess.run(["timeout", "-k", "10", "200", sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", g[0], str(mode)],
                               capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode or 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith(g[0])][-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:                   # (kept up to date row by row)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
