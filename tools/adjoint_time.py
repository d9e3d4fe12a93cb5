#!/usr/bin/env python3
"""Time the adjoint (aai_adjoint_batch_device_f32) next to the forward under AAI_POLICY_DOUBLE_PRECISION -- the shipped code that
does the same double-precision pair evaluations once per pair -- on the geometries of the adjoint identity test, both modes.
A fresh child process per geometry; in it 3 warm-up launches of each, then N (default 24) timed launches of each between
device events, forward and adjoint alternating; reported: median, 10th..90th percentile, and the ratio of the medians.

--planned: the rotations by multiples of 90 degrees instead (PLANNED_GEOMETRIES), three launches taking turns -- the forward (the
separable kernel), the general adjoint and the planned adjoint (aai_adjoint_planned_batch_device_f32, after aai_adjoint_prepare) --
with the largest deviation of the planned from the general result relative to max(|general|, 1e-3 max|general|) at the end of each row.

--channels: the interleaved adjoint (aai_adjoint_interleaved_device_f32) on INTERLEAVED_ROWS with C = 3 and C = 4, two legs taking
turns -- one interleaved call, and C calls of the unchanged single-channel entry on planes split beforehand (the split is not timed) --
with the ratio of the medians (interleaved / planar) and whether the two results have the same bits at the end of each row.

--rotated: the planned adjoint at general rotations (aai_adjoint_rotated_batch_device_f32, after aai_adjoint_rotated_prepare) against the
unchanged general entry on ROTATED_GEOMETRIES -- the general-angle rows of the first table -- both modes, the two legs taking turns;
with the ratio of the medians (general / rotated), whether the new entry's 90th percentile lies below the general's 10th, and whether
the two results have the same bits at the end of each row.  (profiles/adjoint_rotated_time.txt)

--rotated --channels: the interleaved planned adjoint at general rotations (aai_adjoint_rotated_interleaved_device_f32, after
aai_adjoint_rotated_prepare) on ROTATED_INTERLEAVED_ROWS with C = 3 and C = 4, three legs taking turns -- (a) the new entry, (b)
aai_adjoint_interleaved_device_f32, the general interleaved adjoint, (c) C calls of aai_adjoint_rotated_batch_device_f32 on planes split
beforehand (the split is not timed) -- with the ratios of the medians (b)/(a) and (c)/(a), whether (a)'s 90th percentile lies below
(b)'s 10th, and whether (a) and (b) have the same bits at the end of each row.  (profiles/adjoint_rotated_interleaved_time.txt)

--planned --channels: the interleaved planned adjoint at multiples of 90 degrees (aai_adjoint_planned_interleaved_device_f32, after
aai_adjoint_rotated_prepare) on PLANNED_GEOMETRIES, both modes, C = 3 and C = 4, the legs taking turns in one process -- (a)
aai_adjoint_interleaved_device_f32, the general interleaved adjoint, (b) C calls of aai_adjoint_planned_batch_device_f32 on planes split
beforehand (the split is not timed), (c) the new entry, and (d) the torch operator's BACKWARD alone on a (1, C, H, W) channels_last input
with a channels_last gy: the planar route (planned_backward=True, its permutes included) against planned_backward="channels_last" --
with (a)/(c), (c)/(b), whether (c)'s 90th percentile lies below (a)'s 10th, whether (c) and (b) have the same bits, and the two torch
medians at the end of each row; the header lines state the three conditions and the rows that miss them.
(profiles/adjoint_axis_interleaved_time.txt)

usage: python tools/adjoint_time.py [--planned | --channels | --rotated | --rotated --channels | --planned --channels] [--launches N] [--out FILE]      (the table also goes to stdout)"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, W, H, srcRes, dstRes, angle)
GEOMETRIES = [("cfg3", 8192, 8192, 8192.0, 2731.0, 17.5), ("wide8", 8192, 8192, 8.0, 1.0, 17.5), ("up2", 2048, 2048, 1.0, 2.0, 30.0),
              ("axis4", 4096, 4096, 4.0, 1.0, 0.0), ("quarter2.5", 4096, 4096, 2.5, 1.0, 90.0)]
# the planned adjoint's rows: the two axis rows above, a flipped quadrant and a transposed up-sampling
PLANNED_GEOMETRIES = [GEOMETRIES[3], GEOMETRIES[4], ("half180", 4096, 4096, 2.0, 1.0, 180.0), ("up2x270", 2048, 2048, 1.0, 2.0, 270.0)]
# the planned adjoint at general rotations: the general-angle rows
ROTATED_GEOMETRIES = GEOMETRIES[:3]
# the interleaved adjoint's rows: (geometry name, mode)
INTERLEAVED_ROWS = [("cfg3", 1), ("cfg3", 2), ("up2", 1)]
# the interleaved planned adjoint's rows: (geometry name, mode)
ROTATED_INTERLEAVED_ROWS = [("cfg3", 1), ("cfg3", 2), ("wide8", 1), ("up2", 1)]


def child_rotated_channels(name, mode, channels, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    C = channels
    rq = aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(2)
    gd = torch.rand((dH, dW, C), dtype=torch.float32, device="cuda", generator=gen)
    planes = gd.permute(2, 0, 1).contiguous()                       # split beforehand: not part of any leg
    new = torch.empty((H, W, C), dtype=torch.float32, device="cuda")
    general = torch.empty_like(new)
    ps = torch.empty((C, H, W), dtype=torch.float32, device="cuda")
    aai.adjoint_rotated_prepare(rq)                                 # serves every channel count
    kernels = {}

    def run_new():
        aai.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, new.data_ptr(), W * C, st, planned="any")
        kernels["new"] = aai.last_kernel()

    def run_general():
        aai.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, general.data_ptr(), W * C, st)
        kernels["general"] = aai.last_kernel()

    def run_planar():
        for c in range(C):
            aai.adjoint_device(rq, planes[c].data_ptr(), dW, ps[c].data_ptr(), W, st, planned="any")
        kernels["planar"] = aai.last_kernel()

    runs = {"new": run_new, "general": run_general, "planar": run_planar}
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
    same = torch.equal(new.view(torch.int32), general.view(torch.int32))
    same_planar = torch.equal(new.permute(2, 0, 1).contiguous().view(torch.int32), ps.view(torch.int32))
    t = {k: np.array(v) for k, v in times.items()}
    cell = lambda v: "%8.3f ms (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))
    clear = np.percentile(t["new"], 90) < np.percentile(t["general"], 10)
    print("%-10s %-4s C=%d %5dx%-5d -> %5dx%-5d  (a) new entry %s  (b) general interleaved %s  (c) %d planned single-channel calls %s  "
          "(b)/(a) %5.2f  (c)/(a) %5.2f  p90(a) < p10(b) %s  bits (a)=(b) %s (a)=(c) %s  [%s; %s; %s]" % (
              name, "area" if mode == aai.MODE_AREA else "fast", C, W, H, dW, dH, cell(t["new"]), cell(t["general"]), C, cell(t["planar"]),
              np.median(t["general"]) / np.median(t["new"]), np.median(t["planar"]) / np.median(t["new"]), "yes" if clear else "NO",
              "same" if same else "DIFFERENT", "same" if same_planar else "DIFFERENT", kernels["new"], kernels["planar"],
              " ".join(tok for tok in aai.plan_shape(rq).split() if tok.split("=")[0] in ("rot_adjoint", "knife"))), flush=True)


def child_planned_channels(name, mode, channels, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    from area_average_interpolation_amd import torch_ops
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in PLANNED_GEOMETRIES if g[0] == name][0]
    C = channels
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(2)
    gd = torch.rand((dH, dW, C), dtype=torch.float32, device="cuda", generator=gen)
    planes = gd.permute(2, 0, 1).contiguous()                       # split beforehand: not part of any leg
    new = torch.empty((H, W, C), dtype=torch.float32, device="cuda")
    general = torch.empty_like(new)
    ps = torch.empty((C, H, W), dtype=torch.float32, device="cuda")
    aai.adjoint_rotated_prepare(rq)                                 # the single-channel plan and its axis tables: every channel count
    kernels = {}

    def run_general():
        aai.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, general.data_ptr(), W * C, st)
        kernels["general"] = aai.last_kernel()

    def run_planar():
        for c in range(C):
            aai.adjoint_device(rq, planes[c].data_ptr(), dW, ps[c].data_ptr(), W, st, planned=True)
        kernels["planar"] = aai.last_kernel()

    def run_new():
        aai.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, new.data_ptr(), W * C, st, planned="separable")
        kernels["new"] = aai.last_kernel()

    # (d) the torch operator's backward alone: one forward per route, its graph kept
    x = torch.rand((1, C, H, W), dtype=torch.float32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    gy = gd.unsqueeze(0).permute(0, 3, 1, 2)                        # (1, C, dH, dW), dense in channels_last
    routes = {}
    for key, planned in (("torch planar", True), ("torch cl", "channels_last")):
        xr = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y, _ = torch_ops.resample(xr, sr, dr, iso, ang, mode=mode, planned_backward=planned)
        routes[key] = (xr, y)

    def backward(key):
        xr, y = routes[key]
        xr.grad = None
        y.backward(gy, retain_graph=True)

    runs = {"general": run_general, "planar": run_planar, "new": run_new,
            "torch planar": lambda: backward("torch planar"), "torch cl": lambda: backward("torch cl")}
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
    same_planar = torch.equal(new.permute(2, 0, 1).contiguous().view(torch.int32), ps.view(torch.int32))
    gp, gc = routes["torch planar"][0].grad, routes["torch cl"][0].grad
    same_torch = torch.equal(gp.contiguous().view(torch.int32), gc.contiguous().view(torch.int32)) and gc.is_contiguous(memory_format=torch.channels_last)
    gdd = general.double()
    dev = float(((new.double() - gdd).abs() / gdd.abs().clamp_min(1e-3 * float(gdd.abs().max()))).max())
    t = {k: np.array(v) for k, v in times.items()}
    cell = lambda v: "%8.3f ms (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))
    clear = np.percentile(t["new"], 90) < np.percentile(t["general"], 10)
    row = "%s %s C=%d" % (name, "area" if mode == aai.MODE_AREA else "fast", C)
    print("%-10s %-4s C=%d %5dx%-5d -> %5dx%-5d  (a) general interleaved %s  (b) %d planned single-channel calls %s  (c) new entry %s  "
          "(a)/(c) %6.1f  (c)/(b) %5.2f  p90(c) < p10(a) %s  bits (c)=(b) %s  deviation from (a) %.2e  (d) torch backward: planar route %s  "
          "channels_last route %s  planar/channels_last %5.2f  grads %s  [%s; %s]" % (
              name, "area" if mode == aai.MODE_AREA else "fast", C, W, H, dW, dH, cell(t["general"]), C, cell(t["planar"]), cell(t["new"]),
              np.median(t["general"]) / np.median(t["new"]), np.median(t["new"]) / np.median(t["planar"]), "yes" if clear else "NO",
              "same" if same_planar else "DIFFERENT", dev, cell(t["torch planar"]), cell(t["torch cl"]),
              np.median(t["torch planar"]) / np.median(t["torch cl"]), "same" if same_torch else "DIFFERENT", kernels["new"],
              " ".join(tok for tok in aai.plan_shape(rq).split() if tok.split("=")[0] in ("flagged", "dense", "adjoint"))), flush=True)
    # for the parent's header lines: row | (c) clear of (a) | (c)/(b) | torch channels_last median below planar's | the two torch medians
    print("@ %s | %d | %.3f | %d | %.3f %.3f" % (row, clear, np.median(t["new"]) / np.median(t["planar"]),
                                               np.median(t["torch cl"]) < np.median(t["torch planar"]), np.median(t["torch planar"]), np.median(t["torch cl"])), flush=True)


def planned_channels_table(launches, out):
    """the parent of child_planned_channels: the rows, then the header lines that state the three conditions with the rows that miss them"""
    rows, facts = [], []
    for g in PLANNED_GEOMETRIES:
        for mode in (1, 2):
            for channels in (3, 4):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--planned", "--channels", "--launches", str(launches),
                                    "--child", g[0], str(mode), str(channels)], capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    return r.returncode or 1
                line = [ln for ln in r.stdout.splitlines() if ln.startswith(g[0])][-1]
                print(line, flush=True)
                rows.append(line)
                f = [x.strip() for x in [ln for ln in r.stdout.splitlines() if ln.startswith("@ ")][-1][2:].split("|")]
                facts.append((f[0], int(f[1]), float(f[2]), int(f[3]), f[4]))
    unclear = [f[0] for f in facts if not f[1]]
    slower = ["%s (%.2f)" % (f[0], f[2]) for f in facts if f[2] > 1.0]
    torch_slower = ["%s (planar, channels_last medians in ms: %s)" % (f[0], f[4]) for f in facts if not f[3]]
    ratios = [f[2] for f in facts]
    head = ["# median (10th..90th percentile) of %d launches each, device events, the legs taking turns, one process per row: (a) "
            "aai_adjoint_interleaved_device_f32, (b) C calls of aai_adjoint_planned_batch_device_f32 on pre-split planes, (c) "
            "aai_adjoint_planned_interleaved_device_f32, (d) the torch backward alone, planar route (planned_backward=True, permutes included) "
            "and planned_backward=\"channels_last\"" % launches,
            "# condition 1, (c) against (a): (c)'s 90th percentile below (a)'s 10th in every row -- %s" % (
                "holds in all %d rows" % len(facts) if not unclear else "MISSED in: " + "; ".join(unclear)),
            "# condition 2, (c) against (b): (c)/(b) between %.2f and %.2f over the rows -- %s" % (
                min(ratios), max(ratios), "(c) is slower than (b) in no row" if not slower else "(c) is SLOWER than (b) in: " + "; ".join(slower)),
            "# condition 3, (d): the channels_last route's median below the planar route's -- %s" % (
                "holds in all %d rows: no row class keeps the planar route" % len(facts) if not torch_slower else "MISSED in: " + "; ".join(torch_slower))]
    for ln in head:
        print(ln, flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(head + rows) + "\n")
    return 0


def child_channels(name, mode, channels, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    C = channels
    rq = aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(2)
    gd = torch.rand((dH, dW, C), dtype=torch.float32, device="cuda", generator=gen)
    planes = gd.permute(2, 0, 1).contiguous()                       # split beforehand: not part of either leg
    gs = torch.empty((H, W, C), dtype=torch.float32, device="cuda")
    ps = torch.empty((C, H, W), dtype=torch.float32, device="cuda")
    kernels = {}

    def run_interleaved():
        aai.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, st)
        kernels["interleaved"] = aai.last_kernel()

    def run_planar():
        for c in range(C):
            aai.adjoint_device(rq, planes[c].data_ptr(), dW, ps[c].data_ptr(), W, st)
        kernels["planar"] = aai.last_kernel()

    runs = {"interleaved": run_interleaved, "planar": run_planar}
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
    same = torch.equal(gs.permute(2, 0, 1).contiguous().view(torch.int32), ps.view(torch.int32))
    t = {k: np.array(v) for k, v in times.items()}
    cell = lambda v: "%8.3f ms (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))
    print("%-10s %-4s C=%d %5dx%-5d -> %5dx%-5d  interleaved %s  %d planar calls %s  interleaved/planar %5.2f  bits %s  [%s; %s]" % (
        name, "area" if mode == aai.MODE_AREA else "fast", C, W, H, dW, dH, cell(t["interleaved"]), C, cell(t["planar"]),
        np.median(t["interleaved"]) / np.median(t["planar"]), "same" if same else "DIFFERENT", kernels["interleaved"], kernels["planar"]), flush=True)


def child_planned(name, mode, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in PLANNED_GEOMETRIES if g[0] == name][0]
    rq = aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((H, W), dtype=torch.float32, device="cuda")
    y = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    aai.synth_device(x.data_ptr(), W, H, W, 1, st)
    aai.synth_device(y.data_ptr(), dW, dH, dW, 2, st)
    wx, general, planned = torch.empty_like(y), torch.empty_like(x), torch.empty_like(x)
    aai.adjoint_prepare(rq)
    runs = {"fwd": lambda: aai.resample_device(rq, x.data_ptr(), W, wx.data_ptr(), dW, st),
            "general": lambda: aai.adjoint_device(rq, y.data_ptr(), dW, general.data_ptr(), W, st),
            "planned": lambda: aai.adjoint_device(rq, y.data_ptr(), dW, planned.data_ptr(), W, st, planned=True)}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    kernel = aai.last_kernel()
    times = {k: [] for k in runs}
    for _ in range(launches):
        for key, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[key].append(a.elapsed_time(b))
    gd = general.double()
    dev = float(((planned.double() - gd).abs() / gd.abs().clamp_min(1e-3 * float(gd.abs().max()))).max())
    t = {k: np.array(v) for k, v in times.items()}
    cell = lambda v: "%8.3f ms (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))
    print("%-10s %-4s %5dx%-5d -> %5dx%-5d  forward %s  general adjoint %s  planned adjoint %s  general/planned %6.1f  planned/forward %5.2f  deviation %.2e  [%s; %s]" % (
        name, "area" if mode == aai.MODE_AREA else "fast", W, H, dW, dH, cell(t["fwd"]), cell(t["general"]), cell(t["planned"]),
        np.median(t["general"]) / np.median(t["planned"]), np.median(t["planned"]) / np.median(t["fwd"]), dev, kernel,
        " ".join(tok for tok in aai.plan_shape(rq).split() if tok.split("=")[0] in ("flagged", "dense", "adjoint"))), flush=True)


def child_rotated(name, mode, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in ROTATED_GEOMETRIES if g[0] == name][0]
    rq = aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
    lay = aai.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    aai.synth_device(y.data_ptr(), dW, dH, dW, 2, st)
    general = torch.empty((H, W), dtype=torch.float32, device="cuda")
    rotated = torch.empty_like(general)
    aai.adjoint_rotated_prepare(rq)
    kernels = {}

    def run_general():
        aai.adjoint_device(rq, y.data_ptr(), dW, general.data_ptr(), W, st)
        kernels["general"] = aai.last_kernel()

    def run_rotated():
        aai.adjoint_device(rq, y.data_ptr(), dW, rotated.data_ptr(), W, st, planned="any")
        kernels["rotated"] = aai.last_kernel()

    runs = {"general": run_general, "rotated": run_rotated}
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
    same = torch.equal(general.view(torch.int32), rotated.view(torch.int32))
    t = {k: np.array(v) for k, v in times.items()}
    cell = lambda v: "%8.3f ms (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))
    clear = np.percentile(t["rotated"], 90) < np.percentile(t["general"], 10)
    print("%-10s %-4s %5dx%-5d -> %5dx%-5d  general adjoint %s  rotated entry %s  general/rotated %5.2f  p90 < p10 %s  bits %s  [%s; %s]" % (
        name, "area" if mode == aai.MODE_AREA else "fast", W, H, dW, dH, cell(t["general"]), cell(t["rotated"]),
        np.median(t["general"]) / np.median(t["rotated"]), "yes" if clear else "NO", "same" if same else "DIFFERENT", kernels["rotated"],
        " ".join(tok for tok in aai.plan_shape(rq).split() if tok.split("=")[0] in ("rot_adjoint", "knife"))), flush=True)


def child(name, mode, launches):
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    aai.set_device(0)
    _, W, H, sr, dr, ang = [g for g in GEOMETRIES if g[0] == name][0]
    iso = ((W - 1) / 2, (H - 1) / 2)
    adj = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    fwd = aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=aai.POLICY_REFERENCE | aai.POLICY_DOUBLE_PRECISION)
    lay = aai.query(adj)[2]
    dW, dH = lay.dst_width, lay.dst_height
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((H, W), dtype=torch.float32, device="cuda")
    y = torch.empty((dH, dW), dtype=torch.float32, device="cuda")
    aai.synth_device(x.data_ptr(), W, H, W, 1, st)
    aai.synth_device(y.data_ptr(), dW, dH, dW, 2, st)
    wx, wty = torch.empty_like(y), torch.empty_like(x)
    aai.prepare(fwd)

    def run_fwd():
        aai.resample_device(fwd, x.data_ptr(), W, wx.data_ptr(), dW, st)

    def run_adj():
        aai.adjoint_device(adj, y.data_ptr(), dW, wty.data_ptr(), W, st)

    for _ in range(3):
        run_fwd()
        run_adj()
    torch.cuda.synchronize()
    fwd_kernel = ""
    times = {"fwd": [], "adj": []}
    for _ in range(launches):
        for key, fn in (("fwd", run_fwd), ("adj", run_adj)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[key].append(a.elapsed_time(b))
            if key == "fwd":
                fwd_kernel = aai.last_kernel()
    f, a = np.array(times["fwd"]), np.array(times["adj"])
    print("%-10s %-4s %5dx%-5d -> %5dx%-5d  forward fp64 %8.3f ms (%.3f..%.3f)  adjoint %8.3f ms (%.3f..%.3f)  ratio %5.2f  [%s]" % (
        name, "area" if mode == aai.MODE_AREA else "fast", W, H, dW, dH,
        np.median(f), np.percentile(f, 10), np.percentile(f, 90), np.median(a), np.percentile(a, 10), np.percentile(a, 90),
        np.median(a) / np.median(f), fwd_kernel.split("(")[0].strip()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--planned", action="store_true")
    ap.add_argument("--channels", action="store_true")
    ap.add_argument("--rotated", action="store_true")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("at least 20 timed launches")
    both = args.rotated and args.channels                      # the interleaved planned adjoint's table
    axis_channels = args.planned and args.channels and not args.rotated      # ... and its table at multiples of 90 degrees
    if args.planned + args.channels + args.rotated > 1 and not (both and not args.planned) and not axis_channels:
        ap.error("--planned, --channels and --rotated are separate tables (--rotated --channels is a fourth, --planned --channels a fifth)")
    if axis_channels and not args.child:
        return planned_channels_table(args.launches, args.out)
    if args.child:
        if axis_channels:
            child_planned_channels(args.child[0], int(args.child[1]), int(args.child[2]), args.launches)
        elif both:
            child_rotated_channels(args.child[0], int(args.child[1]), int(args.child[2]), args.launches)
        elif args.channels:
            child_channels(args.child[0], int(args.child[1]), int(args.child[2]), args.launches)
        elif args.rotated:
            child_rotated(args.child[0], int(args.child[1]), args.launches)
        else:
            (child_planned if args.planned else child)(args.child[0], int(args.child[1]), args.launches)
        return 0
    if args.channels:
        lines = ["# median (10th..90th percentile) of %d launches each, device events, %s taking turns, one process per row" % (
            args.launches, "(a) aai_adjoint_rotated_interleaved_device_f32, (b) aai_adjoint_interleaved_device_f32 and (c) C calls of "
            "aai_adjoint_rotated_batch_device_f32 on pre-split planes" if both else
            "the interleaved call and the C single-channel calls on pre-split planes")]
        print(lines[0], flush=True)
        for name, mode in (ROTATED_INTERLEAVED_ROWS if both else INTERLEAVED_ROWS):
            for channels in (3, 4):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--channels"] + (["--rotated"] if both else []) +
                                   ["--launches", str(args.launches), "--child", name, str(mode), str(channels)],
                                   capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    return r.returncode or 1
                line = [ln for ln in r.stdout.splitlines() if ln.startswith(name)][-1]
                print(line, flush=True)
                lines.append(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return 0
    leg = ["--planned"] if args.planned else (["--rotated"] if args.rotated else [])
    lines = ["# median (10th..90th percentile) of %d launches each, device events, %s, one process per row"
             % (args.launches, "forward, general adjoint and planned adjoint taking turns" if args.planned else
                ("general adjoint and aai_adjoint_rotated_batch_device_f32 taking turns" if args.rotated else "forward and adjoint alternating"))]
    print(lines[0], flush=True)
    for g in (PLANNED_GEOMETRIES if args.planned else (ROTATED_GEOMETRIES if args.rotated else GEOMETRIES)):
        for mode in (1, 2):
            # a fresh process per row, under its own time limit; a row that fails ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", g[0], str(mode)] + leg,
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
