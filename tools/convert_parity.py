#!/usr/bin/env python3
"""How far apart the two routes of resample-and-convert (include/ext/aai_convert.h) are, over the case table of tests/convert_cases.py.

For every case, mode and conversion, on the random source: (1) the direct kernel's output through aai_resample_convert_device (cases
whose class forwards are skipped and counted), (2) the forwarding route's arithmetic, round(fmaf(aai_resample_interleaved_device(src),
scale, offset)), with the conversion on the CPU (tests/emulation/convert_emulation.cpp: aai_emu_convert_apply, which
tests/test_convert_gpu.py holds the forwarding route to bit for bit).  Reported per conversion and output type: the largest difference
in units of the output type's last place (non-finite elements must agree exactly), and the largest |ds| |scale| with ds the difference
of the two routes' fp32 sums (the replay's sums, which are the kernel's, against the fp32 entry's output).

usage: python tools/convert_parity.py [--out FILE]      (profiles/convert_parity.txt)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ulps(a, b, ot, cc, np):
    """distance in units of the last place between two arrays of one output type (finite elements); non-finite ones must be equal"""
    if ot == cc.F32:
        ka, kb = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
        sign = np.int64(1) << 31
    else:
        ka, kb = a.view(np.int16).astype(np.int64), b.view(np.int16).astype(np.int64)
        sign = np.int64(1) << 15
    ka, kb = np.where(ka < 0, -(ka + sign), ka), np.where(kb < 0, -(kb + sign), kb)
    fa, fb = np.isfinite(cc.as_float(a, ot)), np.isfinite(cc.as_float(b, ot))
    assert np.array_equal(fa, fb) and np.array_equal(a[~fa], b[~fb]), "the routes disagree on a non-finite element"
    return int(np.abs(ka - kb)[fa].max()) if fa.any() else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import area_average_interpolation_amd as aai
    import convert_cases as cc
    import int_cases as ic
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    aai.set_device(0)
    st_handle = torch.cuda.current_stream().cuda_stream

    def upload(a):
        return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()

    worst, worst_ds, skipped, ran = {}, {}, 0, 0
    for g, C, st, ot, lay in cc.CASES:
        for mode_name in cc.MODES:
            rq = ic.request(aai, g, mode_name)
            src = ic.source(g, C, st, "random")
            H, W = src.shape[:2]
            l = aai.query(rq)[2]
            dH, dW = l.dst_height, l.dst_width
            x = upload(src)
            y32 = torch.empty((dH, dW, C), dtype=torch.float32, device="cuda")
            aai.resample_interleaved_device(rq, C, x.data_ptr(), W * C, y32.data_ptr(), dW * C, st_handle, src_dtype=st)
            torch.cuda.synchronize()
            f32 = y32.cpu().numpy()
            for conv in cc.CONVERSIONS:
                scale, offset = cc.conversion(conv, st)
                y = upload(np.zeros(dH * dW * C * (4 if ot == cc.F32 else 2), np.uint8))
                cv = aai.make_convert(C, ot, lay == cc.PLANAR, scale[:C], offset[:C])
                aai.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW if lay == cc.PLANAR else dW * C, st, cv, stream=st_handle, dst_plane_stride=dW * dH)
                torch.cuda.synchronize()
                if not aai.last_kernel().startswith("aai_axis_convert_kernel"):
                    skipped += 1
                    continue
                got = y.cpu().numpy().view(cc.OUT_NP[ot]).reshape(cc.out_shape(dH, dW, C, lay))
                fwd = cc.apply(f32, scale, offset, ot, lay)
                pre = cc.replay(aai, rq, st, src, scale, offset, ot, lay)[1]
                key = (conv, cc.OUT_NAME[ot])
                worst[key] = max(worst.get(key, 0), ulps(got, fwd, ot, cc, np))
                ds = float((np.abs(pre.astype(np.float64) - f32.astype(np.float64)) * np.abs(scale[:C].astype(np.float64))).max())
                worst_ds[key] = max(worst_ds.get(key, 0.0), ds)
                ran += 1
    lines = ["# direct route against the forwarding route's arithmetic over the case table of tests/convert_cases.py, random sources, both modes: %d comparisons, %d skipped (their class forwards)" % (ran, skipped),
             "# conversion  output  largest difference [units of the output's last place]  largest |ds| |scale|"]
    for key in sorted(worst):
        lines.append("%-10s %-5s %6d  %.3e" % (key[0], key[1], worst[key], worst_ds[key]))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
