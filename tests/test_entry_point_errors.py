"""CPU: which (return code, aai_last_error()) every compute entry point of include/*.h reports for a faulty call.

Every argument error is reported before the device is touched, so none of this needs a GPU.  Each entry point is called
with a valid call, with every single fault it can be given, and with every pair of faults (which pins the ORDER of its
checks: a request with two faults reports the one checked first).  The expected values are a recording, not a
specification: tests/golden/entry_point_errors.json (the entries of include/aai.h) and entry_point_errors_typed.json (those
of the eleven extension headers) hold what the library answered when the tables were made
(`python tests/test_entry_point_errors.py --record` rewrites them from the library in the tree), and a change of the
host code that is meant to keep behaviour must reproduce them.  Device pointers are fake non-null integers: nothing
dereferences them before the device check, and a probe whose recorded answer is "no device" is not run where there is one.
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "entry_point_errors.json")
TYPED_TABLE = os.path.join(HERE, "golden", "entry_point_errors_typed.json")

FAKE_SRC, FAKE_DST = 0x10000, 0x20000
BIG = 4096          # a row stride no smaller than any row of the base request, in elements (4 channels included)


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _ptrs(*v):
    return (ctypes.c_void_p * len(v))(*v)


_TEXT = ctypes.create_string_buffer(512)
_ROW0, _ROW1 = ctypes.c_int32(), ctypes.c_int32()

# the base request: 64 x 48 pixels, 1:1, rotated by 17.5 degrees (so that the band entries apply their multiple-of-16 rule)
BASE = dict(mode=1, policy=0, src_width=64, src_height=48, src_res_x=1.0, src_res_y=1.0, dst_res_x=1.0, dst_res_y=1.0,
            src_iso_x=31.5, src_iso_y=23.5, rotation_deg=17.5)

# entry point -> its arguments in ABI order with the values of a valid call ("req" stands for the request pointer)
_HOST = [("src", FAKE_SRC), ("src_stride", BIG), ("dst", FAKE_DST), ("dst_stride", BIG), ("layout", None)]
ENTRIES = {
    "aai_resample_f32": [("req", 1)] + _HOST,
    "aai_resample_f64": [("req", 1)] + _HOST,
    "aai_resample_host": [("req", 1), ("src", FAKE_SRC), ("src_dtype", 0), ("src_stride", BIG), ("dst", FAKE_DST), ("dst_stride", BIG), ("layout", None)],
    "aai_resample_interleaved_host": [("req", 1), ("channels", 3), ("src", FAKE_SRC), ("src_dtype", 0), ("src_stride", BIG), ("dst", FAKE_DST),
                                      ("dst_stride", BIG), ("layout", None)],
    "aai_resample_batch_host": [("req", 1), ("batch", 2), ("src", FAKE_SRC), ("src_dtype", 0), ("src_stride", BIG), ("src_image_stride", BIG * BIG),
                                ("dst", FAKE_DST), ("dst_stride", BIG), ("dst_image_stride", BIG * BIG), ("layout", None)],
    "aai_resample_device_f32": [("req", 1), ("src", FAKE_SRC), ("src_stride", BIG), ("dst", FAKE_DST), ("dst_stride", BIG), ("stream", None)],
    "aai_resample_batch_device_f32": [("req", 1), ("batch", 2), ("src", FAKE_SRC), ("src_stride", BIG), ("src_image_stride", BIG * BIG),
                                      ("dst", FAKE_DST), ("dst_stride", BIG), ("dst_image_stride", BIG * BIG), ("stream", None)],
    "aai_resample_batch_device": [("req", 1), ("batch", 2), ("src", FAKE_SRC), ("src_dtype", 0), ("src_stride", BIG), ("src_image_stride", BIG * BIG),
                                  ("dst", FAKE_DST), ("dst_stride", BIG), ("dst_image_stride", BIG * BIG), ("stream", None)],
    "aai_resample_batch_multi_device_f32": [("req", 1), ("n_shards", 1), ("devices", _i32(0)), ("counts", _i32(1)), ("shard_src", _ptrs(FAKE_SRC)),
                                            ("src_stride", BIG), ("src_image_stride", BIG * BIG), ("shard_dst", _ptrs(FAKE_DST)), ("dst_stride", BIG),
                                            ("dst_image_stride", BIG * BIG), ("streams", None)],
    "aai_resample_interleaved_device": [("req", 1), ("batch", 2), ("channels", 3), ("src", FAKE_SRC), ("src_dtype", 0), ("src_stride", BIG),
                                        ("src_image_stride", BIG * BIG), ("dst", FAKE_DST), ("dst_stride", BIG), ("dst_image_stride", BIG * BIG),
                                        ("stream", None)],
    "aai_band_source_rows": [("req", 1), ("dst_row0", 16), ("dst_row1", 32), ("out_row0", ctypes.pointer(_ROW0)), ("out_row1", ctypes.pointer(_ROW1))],
    "aai_resample_band_device_f32": [("req", 1), ("dst_row0", 16), ("dst_row1", 32), ("src", FAKE_SRC), ("src_stride", BIG), ("dst", FAKE_DST),
                                     ("dst_stride", BIG), ("stream", None)],
    "aai_prepare": [("req", 1), ("channels", 1)],
    "aai_plan_info": [("req", 1), ("channels", 1), ("text", _TEXT), ("capacity", 512)],
    # (the adjoint names its arguments the other way round: gdst is read, gsrc written; the fault names follow the image they belong to)
    "aai_adjoint_batch_device_f32": [("req", 1), ("batch", 2), ("dst", FAKE_DST), ("dst_stride", BIG), ("dst_image_stride", BIG * BIG),
                                     ("src", FAKE_SRC), ("src_stride", BIG), ("src_image_stride", BIG * BIG), ("stream", None)],
    "aai_adjoint_f32": [("req", 1), ("dst", FAKE_DST), ("dst_stride", BIG), ("src", FAKE_SRC), ("src_stride", BIG), ("layout", None)],
    "aai_synth_device_f32": [("dst", FAKE_DST), ("width", 64), ("height", 48), ("stride", 64), ("seed", 1), ("stream", None)],
    "aai_synth_rows_device_f32": [("dst", FAKE_DST), ("width", 64), ("height", 48), ("row0", 8), ("row1", 16), ("stride", 64), ("seed", 1), ("stream", None)],
}

# fault -> the arguments ("rq.<field>": a field of the request) it replaces.  A fault applies to an entry point that has every
# argument it names; two faults pair up when they replace different things.
FAULTS = {
    "null_request": {"req": 0},
    "bad_mode": {"rq.mode": 9},
    "bad_policy": {"rq.policy": 2},
    "res_mismatch": {"rq.src_res_y": 2.0},                                   # the reference's four validation errors ...
    "res_nonpositive": {"rq.dst_res_x": 0.0, "rq.dst_res_y": 0.0},
    "no_rows": {"rq.src_height": 0},
    "no_columns": {"rq.src_width": 0},
    "nonfinite": {"rq.rotation_deg": float("nan")},                          # ... and the library's own
    "nonfinite_iso": {"rq.src_iso_x": float("inf")},
    "too_large": {"rq.src_res_x": 1e-6, "rq.src_res_y": 1e-6},
    "mode_bilinear": {"rq.mode": 3},                                          # (a fault for the adjoint only; valid elsewhere)
    "policy_no_fixup": {"rq.policy": 0x400},                                  # (likewise)
    "bad_dtype": {"src_dtype": 7},
    "channels_zero": {"channels": 0},
    "channels_five": {"channels": 5},
    "negative_batch": {"batch": -1},
    "zero_batch": {"batch": 0},                                               # (no fault: which checks still run for an empty batch)
    "null_src": {"src": None},
    "null_dst": {"dst": None},
    "short_src_stride": {"src_stride": 1},
    "short_dst_stride": {"dst_stride": 1},
    # a row of more than INT32_MAX / 2 elements once the channels are counted (2^29 pixels of 4 channels, halved by the resampling)
    "row_too_long": {"rq.src_width": 1 << 29, "rq.src_height": 1, "rq.dst_res_x": 0.5, "rq.dst_res_y": 0.5, "rq.rotation_deg": 0.0, "channels": 4},
    "band_reversed": {"dst_row0": 32, "dst_row1": 16},
    "band_beyond": {"dst_row1": 1 << 20},
    "band_negative": {"dst_row0": -16},
    "band_not_16": {"dst_row0": 8},
    "null_out_row0": {"out_row0": None},
    "null_out_row1": {"out_row1": None},
    "null_text": {"text": None},
    "zero_capacity": {"capacity": 0},
    "negative_shards": {"n_shards": -1},
    "zero_shards": {"n_shards": 0},
    "null_devices": {"devices": None},
    "null_counts": {"counts": None},
    "negative_count": {"counts": _i32(-1)},
    "null_shard_array": {"shard_src": None},
    "null_shard_src": {"shard_src": _ptrs(None)},
    "null_shard_dst": {"shard_dst": _ptrs(None)},
    "negative_width": {"width": -1},
    "negative_height": {"height": -1},
    "short_stride": {"stride": 1},
    "rows_reversed": {"row0": 16, "row1": 8},
    "rows_beyond": {"row1": 49},
    "negative_row0": {"row0": -1},
}

# The entries of the extension headers, recorded in TYPED_TABLE.  They take the faults above and a few of their own (TYPED_FAULTS),
# which the entries of include/aai.h are not probed with: their table was recorded without them.
_BATCH = [("src", FAKE_SRC), ("src_stride", BIG), ("src_image_stride", BIG * BIG), ("dst", FAKE_DST), ("dst_stride", BIG), ("dst_image_stride", BIG * BIG),
          ("stream", None)]
_ADJ_BATCH = [("dst", FAKE_DST), ("dst_stride", BIG), ("dst_image_stride", BIG * BIG), ("src", FAKE_SRC), ("src_stride", BIG), ("src_image_stride", BIG * BIG),
              ("stream", None)]
_ADJ_HOST = [("dst", FAKE_DST), ("dst_stride", BIG), ("src", FAKE_SRC), ("src_stride", BIG), ("layout", None)]
_RQ, _RQ_B, _RQ_BC, _RQ_C = [("req", 1)], [("req", 1), ("batch", 2)], [("req", 1), ("batch", 2), ("channels", 3)], [("req", 1), ("channels", 3)]
TYPED_ENTRIES = {
    # include/aai_f64.h
    "aai_resample_batch_device_f64": _RQ_B + _BATCH,
    "aai_resample_exact_f64": _RQ + _HOST,
    "aai_adjoint_batch_device_f64": _RQ_B + _ADJ_BATCH,
    "aai_adjoint_f64": _RQ + _ADJ_HOST,
    # include/aai_half.h, aai_half_interleaved.h, aai_int.h
    "aai_resample_half_batch_device": _RQ_B + [("half_dtype", 1)] + _BATCH,
    "aai_resample_half_host": _RQ + [("half_dtype", 2)] + _HOST,
    "aai_resample_half_interleaved_device": _RQ_BC + [("half_dtype", 1)] + _BATCH,
    "aai_resample_half_interleaved_host": _RQ_C + [("half_dtype", 2)] + _HOST,
    "aai_resample_int_batch_device": _RQ_BC + [("dtype", 1)] + _BATCH,
    "aai_resample_int_host": _RQ_C + [("dtype", 2)] + _HOST,
    # include/aai_adjoint_half.h
    "aai_adjoint_half_device": _RQ_BC + [("half_dtype", 1)] + _ADJ_BATCH,
    "aai_adjoint_half_host": _RQ_C + [("half_dtype", 2)] + _ADJ_HOST,
    # include/aai_adjoint_planned.h, aai_adjoint_rotated.h
    "aai_adjoint_prepare": _RQ,
    "aai_adjoint_planned_batch_device_f32": _RQ_B + _ADJ_BATCH,
    "aai_adjoint_planned_f32": _RQ + _ADJ_HOST,
    "aai_adjoint_rotated_prepare": _RQ,
    "aai_adjoint_rotated_batch_device_f32": _RQ_B + _ADJ_BATCH,
    "aai_adjoint_rotated_f32": _RQ + _ADJ_HOST,
    # include/aai_adjoint_interleaved.h, aai_adjoint_rotated_interleaved.h, aai_adjoint_planned_interleaved.h
    "aai_adjoint_interleaved_device_f32": _RQ_BC + _ADJ_BATCH,
    "aai_adjoint_interleaved_f32": _RQ_C + _ADJ_HOST,
    "aai_adjoint_rotated_interleaved_device_f32": _RQ_BC + _ADJ_BATCH,
    "aai_adjoint_rotated_interleaved_f32": _RQ_C + _ADJ_HOST,
    "aai_adjoint_planned_interleaved_device_f32": _RQ_BC + _ADJ_BATCH,
    "aai_adjoint_planned_interleaved_f32": _RQ_C + _ADJ_HOST,
    # include/aai_adjoint_sample.h
    "aai_adjoint_sample_batch_device_f32": _RQ_B + _ADJ_BATCH,
    "aai_adjoint_sample_f32": _RQ + _ADJ_HOST,
    "aai_adjoint_sample_interleaved_device_f32": _RQ_BC + _ADJ_BATCH,
    "aai_adjoint_sample_interleaved_f32": _RQ_C + _ADJ_HOST,
}
# (the samplers' adjoint takes the bilinear and bicubic modes only: its valid call is the base request in bilinear mode)
REQUEST = {e: {"mode": 3} for e in TYPED_ENTRIES if e.startswith("aai_adjoint_sample_")}
TYPED_FAULTS = dict(FAULTS, **{
    "bad_half_dtype": {"half_dtype": 7},
    "bad_int_dtype": {"dtype": 7},
    "f32_int_dtype": {"dtype": 0},                                            # (an element type of the fp32 entries, none of the integer ones)
    "mode_area": {"rq.mode": 1},                                              # (faults for the samplers' adjoint only; valid elsewhere)
    "mode_fast": {"rq.mode": 2},
    "mode_bicubic": {"rq.mode": 4},                                           # (a fault for the area adjoint and the f64 forward)
})


def _args(entry):
    return ENTRIES[entry] if entry in ENTRIES else TYPED_ENTRIES[entry]


def _faults(entry):
    return FAULTS if entry in ENTRIES else TYPED_FAULTS


# TYPED_TABLE holds its 6,046 probes packed, one entry point per line, and names everything it packs:
#   "faults"   the fault names that the numbers below stand for
#   "answers"  the distinct [return code, text] pairs that the numbers below stand for
#   entry  ->  "singles": the faults that apply to it, "valid": the answer without a fault, "single": the answer per single fault, and
#              "pairs": row i holds the answers of the pairs (singles[i], singles[i + 1 + j]), null where the two are not paired
def pack(tables):
    """{entry: {probe: [rc, text]}} -> the packed form"""
    names, answers = list(TYPED_FAULTS), []

    def number(answer):
        if answer not in answers:
            answers.append(answer)
        return answers.index(answer)

    entries = {}
    for entry, t in tables.items():
        s = [f for f in names if f in t]
        entries[entry] = {"singles": [names.index(f) for f in s], "valid": number(t["valid"]), "single": [number(t[f]) for f in s],
                          "pairs": [[number(t[a + "+" + b]) if a + "+" + b in t else None for b in s[i + 1:]] for i, a in enumerate(s)]}
    return {"faults": names, "answers": answers, "entries": entries}


def unpack(packed):
    """the packed form -> {entry: {probe: [rc, text]}}"""
    names, answers, tables = packed["faults"], packed["answers"], {}
    for entry, e in packed["entries"].items():
        s = [names[i] for i in e["singles"]]
        t = {"valid": answers[e["valid"]]}
        t.update({f: answers[k] for f, k in zip(s, e["single"])})
        for i, row in enumerate(e["pairs"]):
            t.update({s[i] + "+" + s[i + 1 + j]: answers[k] for j, k in enumerate(row) if k is not None})
        tables[entry] = t
    return tables


def load_table(entry):
    """{entry: {probe: [rc, text]}} of the golden file that holds `entry`"""
    return json.load(open(TABLE)) if entry in ENTRIES else unpack(json.load(open(TYPED_TABLE)))


def _applies(fault, entry):
    names = [n for n, _ in _args(entry)]
    return all((k.startswith("rq.") and "req" in names) or k in names for k in _faults(entry)[fault])


def probes(entry):
    """the fault combinations of an entry point: (), every single fault, every pair that replaces different things"""
    faults = _faults(entry)
    singles = [f for f in faults if _applies(f, entry)]
    out = [()] + [(f,) for f in singles]
    for a, b in itertools.combinations(singles, 2):
        ka, kb = set(faults[a]), set(faults[b])
        if ka & kb:
            continue
        if ("req" in ka and any(k.startswith("rq.") for k in kb)) or ("req" in kb and any(k.startswith("rq.") for k in ka)):
            continue      # a null request has no fields
        out.append((a, b))
    return out


def call(lib, L, entry, faults):
    """-> [return code, aai_last_error()] of one probe"""
    fields, args = dict(BASE, **REQUEST.get(entry, {})), dict(_args(entry))
    for f in faults:
        for k, v in _faults(entry)[f].items():
            if k.startswith("rq."):
                fields[k[3:]] = v
            else:
                args[k] = v
    rq = L.Request(**fields)
    if "req" in args:
        args["req"] = ctypes.byref(rq) if args["req"] else None
    # start from an empty error text: a successful query clears it
    lay = L.Layout()
    assert lib.aai_query(ctypes.byref(L.Request(**BASE)), ctypes.byref(lay)) == L.OK and lib.aai_last_error() == b""
    rc = getattr(lib, entry)(*[args[n] for n, _ in _args(entry)])
    return [rc, lib.aai_last_error().decode()]


def record(lib, L, entries):
    return {entry: {"+".join(p) or "valid": call(lib, L, entry, p) for p in probes(entry)} for entry in entries}


def test_every_compute_entry_point_is_probed():
    import re
    import glob
    headers = sorted(glob.glob(os.path.join(os.path.dirname(HERE), "include", "*.h")))
    assert len(headers) == 12, headers
    declared = set()
    for header in headers:
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        declared |= set(re.findall(r"\b(aai_[a-z0-9_]+)\s*\(", text))
    # what is left out computes nothing: queries, device management, the error texts, page-locked allocation
    left_out = {"aai_query", "aai_last_error", "aai_last_kernel", "aai_error_string", "aai_version", "aai_device_count", "aai_set_device",
                "aai_device_synchronize", "aai_host_alloc", "aai_host_free", "aai_shutdown"}
    assert not set(ENTRIES) & set(TYPED_ENTRIES)
    assert declared - left_out == set(ENTRIES) | set(TYPED_ENTRIES)
    for entry in list(ENTRIES) + list(TYPED_ENTRIES):
        table = load_table(entry)
        assert sorted(table[entry]) == sorted("+".join(p) or "valid" for p in probes(entry)), entry
        assert len(table[entry]) > 10 and any("+" in k for k in table[entry]), entry


@pytest.mark.parametrize("entry", sorted(ENTRIES) + sorted(TYPED_ENTRIES))
def test_entry_point_reports_the_recorded_error(aai, entry):
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    table = load_table(entry)[entry]
    have_gpu = aai.device_count() > 0
    wrong = []
    for p in probes(entry):
        key = "+".join(p) or "valid"
        want = table[key]
        if want[0] == L.ERR_NO_DEVICE:
            assert "no CPU fallback" in want[1], key
            if have_gpu:
                continue      # with a device this call would go on to compute, on pointers that point nowhere
        got = call(lib, L, entry, p)
        if got != want:
            wrong.append((key, got, want))
    assert not wrong, wrong[:10]
    # a valid call ends at the device check -- but for aai_band_source_rows, which is host arithmetic and succeeds
    assert table["valid"][0] == (L.OK if entry == "aai_band_source_rows" else L.ERR_NO_DEVICE)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_entry_point_errors.py --record")
    sys.path.insert(0, os.path.dirname(HERE))
    import area_average_interpolation_amd as _aai
    from area_average_interpolation_amd import _lib as _L
    if _aai.device_count() > 0:
        sys.exit("record the table on a machine without a GPU: every probe must stop at the device check at the latest")
    with open(TABLE, "w") as f:
        json.dump(record(_L.load(), _L, ENTRIES), f, indent=0, sort_keys=True)
        f.write("\n")
    packed = pack(record(_L.load(), _L, sorted(TYPED_ENTRIES)))
    with open(TYPED_TABLE, "w") as f:      # (one line per entry point)
        f.write('{"faults": %s,\n"answers": %s,\n"entries": {\n%s\n}}\n' % (json.dumps(packed["faults"]), json.dumps(packed["answers"]), ",\n".join(
            "%s: %s" % (json.dumps(e), json.dumps(v, separators=(",", ":"))) for e, v in packed["entries"].items())))
    print("wrote", TABLE, TYPED_TABLE)
