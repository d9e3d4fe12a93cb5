"""Which instantiations of the knife-edge fix-up pass a request log reaches (needs the GPU: the plans say what is flagged).

    python tools/knife_variants_report.py --log before.jsonl [--log after.jsonl ...]

The logs come from tools/request_log.py.  For every distinct area / fast request of a log that a rotated-lattice kernel served, the
request's plan is built (aai_prepare) and aai_plan_info read: `flagged > 0` means the call ran the listed form
aai_fixup_group_kernel<MODE, T, MULTI> for its source type and channel count, `dense=1` the strict form of aai_rotated_kernel.
Printed per log: the calls per instantiation, split by entry (host, device, band), and the production kernels that ran beside a
non-empty list per (source type, plain / interleaved).  Calls made from child processes are not in a log (the dense form of the
tests runs in one).
"""
import argparse
import collections
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TYPE = {0: "f32", 1: "u8", 2: "u16"}
MODE = {1: "area", 2: "fast"}
DIAG_NO_FIXUP = 0x400


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", action="append", required=True)
    args = ap.parse_args()
    import torch            # noqa: F401  (before the library: one HIP runtime per process)
    import area_average_interpolation_amd as aai
    from area_average_interpolation_amd import _lib as L
    aai.set_device(0)
    no_fixup = getattr(L, "POLICY_DIAG_NO_FIXUP", DIAG_NO_FIXUP)
    fields = [f for f, _ in L.Request._fields_]
    plans = {}
    for path in args.log:
        calls = collections.Counter()
        beside = collections.defaultdict(set)
        total = 0
        for line in open(path):
            rec = json.loads(line)
            if rec["rc"] != 0 or rec["mode"] not in MODE or "axis" in rec["kernel"] or not rec["kernel"]:
                continue
            total += 1
            key = tuple(rec[f] for f in fields) + (rec["channels"],)
            if key not in plans:
                rq = L.Request(*[rec[f] for f in fields])
                rq.policy &= ~no_fixup
                aai.shutdown()
                aai.prepare(rq, rec["channels"])
                m = re.search(r"flagged=(\d+) dense=(\d+)", aai.plan_shape(rq, channels=rec["channels"]))
                plans[key] = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
            flagged, dense = plans[key]
            if not flagged and not dense:
                continue
            if rec["policy"] & no_fixup:
                continue                                         # (the fix-up was switched off for this call)
            entry = "band" if "band" in rec["entry"] else ("host" if rec["entry"] in ("aai_resample_f32", "aai_resample_f64", "aai_resample_host", "aai_resample_batch_host", "aai_resample_interleaved_host") else "device")
            inst = ("dense" if dense else "listed", MODE[rec["mode"]], TYPE[rec["dtype"]], "interleaved" if rec["channels"] > 1 else "plain")
            calls[inst + (entry,)] += 1
            if not dense:
                beside[(rec["kernel"].split("<")[0], TYPE[rec["dtype"]], inst[3])].add(rec["channels"])
        print("== %s: %d distinct area / fast calls on rotated lattices ==" % (os.path.basename(path), total))
        reached = sorted({k[:4] for k in calls})
        print("fix-up instantiations reached: %d of 12 listed, %d of 12 dense" % (sum(1 for k in reached if k[0] == "listed"), sum(1 for k in reached if k[0] == "dense")))
        for inst in reached:
            print("    %-7s %-5s %-4s %-12s %s" % (inst + (", ".join("%s %d" % (e, calls[inst + (e,)]) for e in ("host", "device", "band") if calls[inst + (e,)]),)))
        print("production kernels beside a non-empty list (kernel, source type, form: channel counts):")
        for k in sorted(beside):
            print("    %-26s %-4s %-12s C = %s" % (k + (sorted(beside[k]),)))


if __name__ == "__main__":
    main()
