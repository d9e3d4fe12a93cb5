"""Resample-and-convert (include/ext/aai_convert.h: u8 / u16 images of 1..4 interleaved channels in, a scaled fp32 / fp16 / bf16 image out,
interleaved or planar), checks that need no GPU: ABI and header text, argument errors call by call -- the shared ones against the
interleaved fp32 entries' recorded answers, the new ones against tests/golden/entry_point_errors_convert.json --, what the case table
reaches, and the serial CPU replay of aai_axis_convert_kernel (tests/emulation/convert_emulation.cpp over narrow_replay.hpp) against
the oracle.

The bar of the replay (convert_cases.excess): |got - e| <= |scale| TOL max(|s|, 1e-3) + u |e| (1 + TOL), e = s scale + offset in float64 on
the oracle's sums s -- |scale| times the bar the integer and half tests hold the sums to, plus ONE rounding of the output type."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import convert_cases as cc
import half_cases as hc
import int_cases as ic
import test_entry_point_errors as T
from conftest import BUILD, GOLDEN, ROOT, TOL, rel_err

ENTRIES = ("aai_resample_convert_device", "aai_resample_convert_host")
INT_TYPE_MESSAGE = "Unknown integer element type."
CONVERT_TABLE = os.path.join(GOLDEN, "entry_point_errors_convert.json")

# the two entries' arguments in ABI order with the values of a valid call, in the manner of test_entry_point_errors.ENTRIES ("cv": a
# valid conversion, interleaved fp16)
DEVICE_ARGS = [("req", 1), ("batch", 2), ("channels", 3), ("src_dtype", 1), ("src", T.FAKE_SRC), ("src_stride", T.BIG), ("src_image_stride", T.BIG * T.BIG),
               ("cv", "valid"), ("dst", T.FAKE_DST), ("dst_stride", T.BIG), ("dst_plane_stride", T.BIG * T.BIG), ("dst_image_stride", 4 * T.BIG * T.BIG), ("stream", None)]
HOST_ARGS = [("req", 1), ("channels", 3), ("src_dtype", 2), ("src", T.FAKE_SRC), ("src_stride", T.BIG), ("cv", "valid"), ("dst", T.FAKE_DST), ("dst_stride", T.BIG),
             ("dst_plane_stride", T.BIG * T.BIG), ("layout", None)]
NAN, INF = float("nan"), float("inf")
# the new arguments' faults: "cv.<field>" replaces a field of the conversion
NEW_FAULTS = {
    "null_cv": {"cv": None},
    "bad_out_type": {"cv.out_type": 3},
    "negative_out_type": {"cv.out_type": -1},
    "bad_out_layout": {"cv.out_layout": 2},
    "nonfinite_scale": {"cv.scale": (1.0, NAN, 1.0, 1.0)},
    "nonfinite_offset": {"cv.offset": (0.0, 0.0, -INF, 0.0)},
    "nonfinite_beyond_channels": {"cv.scale": (1.0, 1.0, 1.0, NAN), "cv.offset": (0.0, 0.0, 0.0, INF)},      # (no fault with 3 channels)
    "planar": {"cv.out_layout": 1},                                                                            # (no fault)
    "planar_short_dst_stride": {"cv.out_layout": 1, "dst_stride": 1},
    "planar_short_plane_stride": {"cv.out_layout": 1, "dst_plane_stride": 1},
}


def _call(lib, L, fn, arglist, faults):
    """test_entry_point_errors.call for an entry of this file: the faults of that file's table and NEW_FAULTS"""
    fields, args = dict(T.BASE), dict(arglist)
    cv = dict(out_type=1, out_layout=0, scale=(1.0, 0.5, 2.0, 1.0), offset=(0.0, -1.0, 3.0, 0.0))
    for f in faults:
        for k, v in (f if isinstance(f, dict) else NEW_FAULTS[f] if f in NEW_FAULTS else T.FAULTS[f]).items():
            if k.startswith("rq."):
                fields[k[3:]] = v
            elif k.startswith("cv."):
                cv[k[3:]] = v
            else:
                args[k] = v
    rq = L.Request(**fields)
    args["req"] = ctypes.byref(rq) if args["req"] else None
    conv = L.Convert(cv["out_type"], cv["out_layout"], (ctypes.c_float * 4)(*cv["scale"]), (ctypes.c_float * 4)(*cv["offset"]))
    args["cv"] = ctypes.byref(conv) if args["cv"] else None
    lay = L.Layout()
    assert lib.aai_query(ctypes.byref(L.Request(**T.BASE)), ctypes.byref(lay)) == L.OK and lib.aai_last_error() == b""
    rc = fn(*[args[n] for n, _ in arglist])
    return [rc, lib.aai_last_error().decode()]


def test_abi_declares_exports_and_binds_the_convert_entries(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ext", "aai_convert.h")).read()
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.CONVERT_SYMBOLS and name not in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == L.CONVERT_SYMBOLS[name][1]
        # no header directly in include/ declares them: that list is closed (tests/test_entry_point_errors.py)
        for h in os.listdir(os.path.join(ROOT, "include")):
            if h.endswith(".h"):
                assert name not in open(os.path.join(ROOT, "include", h)).read(), (name, h)
    assert (L.DTYPE_F32, L.HALF_F16, L.HALF_BF16) == (0, 1, 2) == (cc.F32, cc.F16, cc.BF16)
    assert (L.LAYOUT_INTERLEAVED, L.LAYOUT_PLANAR) == (0, 1) == (cc.INTERLEAVED, cc.PLANAR)
    assert "AAI_LAYOUT_INTERLEAVED = 0, AAI_LAYOUT_PLANAR = 1" in header and ctypes.sizeof(L.Convert) == 40
    assert '#include "../aai.h"' in header and lib.aai_version() == 2
    for name in ("resample_convert_device", "resample_convert_host", "make_convert"):
        assert hasattr(aai, name) and name in aai.__all__
    for word in ("ties to even", "+-Inf", "canonical quiet NaN", "fp32 is not rounded", "ONE fused operation", "ONE rounding", "s = +0", "Channels never mix",
                 "+converted", "aai_axis_convert_kernel<u8|u16,f32|f16|bf16>", "row bands", "multi-device", "adjoint", "stream capture", "90 / 270 degrees",
                 "listed pixels", "plane", "aligned to one element", "batch == 0 returns AAI_OK", "c * dst_plane_stride + y * dst_stride + x",
                 "y * dst_stride + x * channels + c", "profiles/convert_parity.txt", INT_TYPE_MESSAGE):
        assert word in header, word
    # every new message the header states is one the table pins, and the other way round
    table = json.load(open(CONVERT_TABLE))
    stated = set(re.findall(r'AAI_ERR_[A-Z_]+\s+"([^"]+)"', header))
    pinned = {v[1] for e in table.values() for v in e.values() if v[0] not in (L.OK, L.ERR_NO_DEVICE)}
    new = {"Null conversion.", "Unknown output element type.", "Unknown output layout.", "Conversion scale and offset must be finite.",
           "Destination plane stride smaller than one plane."}
    assert new <= stated and new <= pinned, (new - stated, new - pinned)


def test_build_lists_the_unit_and_the_library_exports_the_entries(aai):
    mk = open(os.path.join(ROOT, "area_average_interpolation_amd", "csrc", "Makefile")).read()
    for var in ("NOCONTRACT", "REPORT_UNITS"):
        line = re.search(r"^%s := (.*)$" % var, mk, flags=re.M).group(1).split()
        assert "aai_axis_convert" in line and "aai_axis_narrow" in line, var
    hdrs = re.search(r"^HDRS  := (.*)$", mk, flags=re.M).group(1)
    assert "include/ext/aai_convert.h" in hdrs and "aai_axis_narrow_parts.hpp" in hdrs
    assert "$(OBJ)/aai_axis_convert.o" in mk
    so = os.path.join(ROOT, "area_average_interpolation_amd", "libaai_hip.so")
    r = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}
    assert set(ENTRIES) <= exported


@pytest.mark.parametrize("entry, typed, arglist", [("aai_resample_convert_device", "aai_resample_interleaved_device", DEVICE_ARGS),
                                                   ("aai_resample_convert_host", "aai_resample_interleaved_host", HOST_ARGS)])
def test_shared_argument_errors_are_those_of_the_interleaved_entries(aai, entry, typed, arglist):
    """Every single fault and every pair of faults of the fault table of tests/test_entry_point_errors.py: the new entry answers what the
    interleaved fp32 entry of the same shape answered when tests/golden/entry_point_errors.json was recorded -- the parent's recorded
    behaviour, not a recording of the code under test -- with the integer entries' message for the element type.  The one difference: an
    empty batch returns AAI_OK before the device check.  All of it before AAI_ERR_NO_DEVICE, with pointers that point nowhere."""
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    table = json.load(open(T.TABLE))
    have_gpu = aai.device_count() > 0
    fn = getattr(lib, entry)
    wrong, refused = [], 0
    for p in T.probes(typed):
        key = "+".join(p) or "valid"
        want = list(table[typed][key])
        if want[1] == "Unknown source element type.":
            want[1] = INT_TYPE_MESSAGE
        if want[0] == L.ERR_NO_DEVICE:
            if "zero_batch" in p and "batch" in dict(arglist):
                want = [L.OK, ""]
            elif have_gpu:
                continue      # with a device this call would go on to compute, on pointers that point nowhere
        else:
            refused += 1
        got = _call(lib, L, fn, arglist, p)
        if got != want:
            wrong.append((key, got, want))
    assert not wrong, wrong[:10]
    assert refused > 100
    # the element type: u8 and u16 only -- fp32 (0) is refused like every unknown value, where aai_int.h checks it
    for value in (0, 3, -1, 7):
        assert _call(lib, L, fn, arglist, ({"src_dtype": value},)) == [L.ERR_BAD_ARGUMENT, INT_TYPE_MESSAGE], value
    assert _call(lib, L, fn, arglist, ("channels_five", "bad_dtype"))[1] == "Channels must be 1..4."
    assert _call(lib, L, fn, arglist, ("bad_dtype", "res_mismatch"))[1] == INT_TYPE_MESSAGE


@pytest.mark.parametrize("entry, arglist", [("aai_resample_convert_device", DEVICE_ARGS), ("aai_resample_convert_host", HOST_ARGS)])
def test_new_argument_errors_are_the_ones_the_header_states(aai, entry, arglist):
    """tests/golden/entry_point_errors_convert.json: the faults of the new arguments, alone and in the pairs that pin their order -- behind
    every shared check, cv == NULL, out_type, out_layout, the non-finite rejection, the planar strides -- with the header's strings"""
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    table = json.load(open(CONVERT_TABLE))[entry]
    have_gpu = aai.device_count() > 0
    fn = getattr(lib, entry)
    wrong = []
    for key, want in table.items():
        if want[0] == L.ERR_NO_DEVICE and have_gpu:
            continue
        got = _call(lib, L, fn, arglist, tuple(key.split("+")) if key != "valid" else ())
        if got != list(want):
            wrong.append((key, got, want))
    assert not wrong, wrong
    assert len(table) >= 20 and sum(1 for v in table.values() if v[0] == L.ERR_NONFINITE) >= 2


def test_api_wrappers_report_the_same(aai):
    from area_average_interpolation_amd import _lib as L
    rq = aai.make_request(24, 20, 3, 1, (11.5, 9.5), 0.0)
    cv = aai.make_convert(3, L.HALF_F16, planar=True, scale=(1, 2, 3), offset=0.5)
    assert (cv.out_type, cv.out_layout, list(cv.scale), list(cv.offset)) == (1, 1, [1, 2, 3, 0], [0.5, 0.5, 0.5, 0])
    with pytest.raises(aai.AaiError) as e:
        aai.resample_convert_device(rq, 3, 8, 72, 8, 24, L.DTYPE_F32, cv)
    assert INT_TYPE_MESSAGE in str(e.value)
    with pytest.raises(aai.AaiError) as e:
        aai.resample_convert_device(rq, 3, 8, 72, 8, 24, L.DTYPE_U8, None)
    assert "Null conversion." in str(e.value)
    aai.resample_convert_device(rq, 3, 8, 72, 8, 24, L.DTYPE_U8, cv, batch=0)      # returns before the device
    with pytest.raises(ValueError):
        aai.make_convert(3, scale=(1, 2))
    with pytest.raises(ValueError):
        aai.make_convert(5)
    rc, msg, dst, iso, lay = aai.resample_convert_host(np.zeros((4, 4, 3), np.uint8), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and dst is None and msg == "Assumed X & Y resolution are same."
    rc, msg, dst, iso, lay = aai.resample_convert_host(np.zeros((8, 8, 3), np.uint8), 2, 1, (3.5, 3.5), 0, scale=(1, float("nan"), 1))
    assert rc == L.ERR_NONFINITE and dst is None and msg == "Conversion scale and offset must be finite."
    with pytest.raises(TypeError):
        aai.resample_convert_host(np.zeros((4, 4), np.float32), 1, 1, (0, 0), 0)
    with pytest.raises(ValueError):
        aai.resample_convert_host(np.zeros((4, 4), np.uint8), 1, 1, (0, 0), 0, out_type=7)
    if aai.device_count() == 0:
        rc, msg, dst, iso, lay = aai.resample_convert_host(np.zeros((8, 8, 3), np.uint8), 2, 1, (3.5, 3.5), 0, planar=True, out_type=L.HALF_BF16)
        assert rc == L.ERR_NO_DEVICE and dst is None


# ---- what the case table reaches ---------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_branch(aai):
    """from the emulation's facts, so that a pruned table cannot silently lose a branch: each channel count, both source types, all three
    output types, both layouts, both rotations, at most 64 and more than 64 outputs per strip, a row length that is no multiple of 4, a
    partial workgroup, rows of exactly 4 elements -- and, for the store forms, every combination of (channels or not, layout, direction,
    one or four outputs per lane) that exists"""
    seen = {k: set() for k in ("C", "src", "out", "layout", "flip", "small", "ragged", "partial", "four", "form", "src_out_layout", "direct", "forwarded")}
    for g, c, st, ot, lay in cc.CASES:
        W = ic.GEOMETRIES[g][0]
        for mode_name in cc.MODES:
            f = cc.facts(ic.request(aai, g, mode_name), c)
            assert (f[0], f[1], f[2], f[7]) == (1, 0, 0, 1), (g, c, mode_name, f)      # every case is a direct-route case
            assert f[8] == f[9] == (ic.GEOMETRIES[g][5] == 180.0)
        seen["C"].add(c); seen["src"].add(st); seen["out"].add(ot); seen["layout"].add(lay); seen["flip"].add(f[8]); seen["small"].add(f[4] <= 64)
        seen["ragged"].add((W * c) % 4 != 0)
        seen["partial"].add(f[3] > 4 and f[3] % 4 != 0)
        seen["four"].add(W * c == 4)
        if cc.direct(ic.request(aai, g, "area"), c, st, ot, lay):      # (the store forms: over the cases that the measured rule leaves on the direct route)
            seen["form"].add((c > 1, lay if c > 1 else cc.INTERLEAVED, f[8], f[4] <= 64))
            seen["direct"].add((st, ot))
        else:
            seen["forwarded"].add(st)
        seen["src_out_layout"].add((st, ot, lay))
    assert seen["C"] == {1, 2, 3, 4} and seen["src"] == {ic.U8, ic.U16} and seen["out"] == {cc.F32, cc.F16, cc.BF16}
    assert seen["layout"] == {cc.INTERLEAVED, cc.PLANAR} and seen["flip"] == {0, 1} and seen["small"] == {True, False}
    assert True in seen["ragged"] and True in seen["partial"] and True in seen["four"]
    assert seen["form"] == {(ch, lay, flip, small) for ch in (False, True) for lay in ((cc.INTERLEAVED, cc.PLANAR) if ch else (cc.INTERLEAVED,))
                            for flip in (0, 1) for small in (True, False)}, seen["form"]
    assert len(seen["src_out_layout"]) == 12 and len(seen["direct"]) == 6 and seen["forwarded"] == {ic.U8, ic.U16}
    assert len(set(cc.CASES)) == len(cc.CASES) == 4 * len(cc.PAIRS)
    assert {g for g, _ in cc.PAIRS} == set("abcdeglmnoh")


def test_conversions_are_the_three_sets():
    for st in (ic.U8, ic.U16):
        s, o = cc.conversion("identity", st)
        assert s.dtype == o.dtype == np.float32 and list(s) == [1] * 4 and list(o) == [0] * 4
        s, o = cc.conversion("normalise", st)
        assert np.allclose(s * ic.MAXV[st] * np.float32(cc.STD), 1, rtol=1e-6) and np.allclose(o * np.float32(cc.STD), -np.float32(cc.MEAN), rtol=1e-6)
        s, o = cc.conversion("edge", st)
        assert s[0] == np.float32(-1.0 / ic.MAXV[st]) and list(s[1:]) == [300, 1, -2] and list(o) == [0.5, 0, -7.25, np.float32(1e-3)]
    # u8 at scale 300 overflows fp16: 255 x 300 = 76500 rounds to +Inf, and the narrowing says so
    assert list(cc.narrow(np.float32([76500.0, 65519.0, 65520.0, -65520.0, np.nan]), cc.F16)) == [0x7c00, 0x7bff, 0x7c00, 0xfc00, 0x7e00]


# ---- the replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom, channels, st, ot, lay", cc.CASES, ids=cc.CASE_IDS)
def test_cpu_replay_matches_the_oracle(aai, po, geom, channels, st, ot, lay):
    for mode_name in cc.MODES:
        for kind in cc.SOURCES:
            rq, src, _, pre_int, gold = cc.case(aai, po, geom, channels, mode_name, st, kind)
            for conv in cc.CONVERSIONS:
                scale, offset = cc.conversion(conv, st)
                out, pre = cc.replay(aai, rq, st, src, scale, offset, ot, lay)
                tag = (geom, channels, cc.SRC_NAME[st], cc.OUT_NAME[ot], cc.LAYOUT_NAME[lay], mode_name, kind, conv)
                # the sums have the bits of the integer direct kernel's value before its quantisation
                assert np.array_equal(pre.view(np.uint32), pre_int.view(np.uint32)), tag
                assert float(rel_err(pre, gold).max()) <= TOL, tag
                hwc = cc.to_hwc(out, lay)
                assert hwc.shape == gold.shape
                over = cc.excess(cc.as_float(hwc, ot), gold, scale, offset, ot)
                print("replay %s: %.3e over the bound" % ("-".join(str(t) for t in tag), over))
                assert over <= 0, (tag, over)
                if conv == "identity":
                    # fp32: the sums bit for bit; half types: the library's one narrowing of them
                    want = pre if ot == cc.F32 else hc.narrow(pre, hc.F16 if ot == cc.F16 else hc.BF16)
                    assert np.array_equal(hwc.view(np.uint32 if ot == cc.F32 else np.uint16), want.view(np.uint32 if ot == cc.F32 else np.uint16)), tag
                # the layouts hold the same elements
                if lay == cc.PLANAR:
                    other = cc.replay(aai, rq, st, src, scale, offset, ot, cc.INTERLEAVED)[0]
                    assert np.array_equal(hwc, other), tag
                # an output pixel without weight is the rounded offset, exactly (the constant source: the oracle's 0 is "no weight")
                if kind == "constant":
                    off = gold == 0
                    assert np.array_equal(pre[off], np.zeros(int(off.sum()), np.float32))
                    want = np.broadcast_to(cc.narrow(offset[:channels], ot), hwc.shape)
                    assert np.array_equal(hwc[off], want[off]), tag
                if conv == "edge" and ot == cc.F16 and st == ic.U8 and channels >= 2 and kind == "constant":
                    # 255 x 300 overflows fp16: +Inf wherever the pixel has its full weight
                    assert (hwc[:, :, 1][gold[:, :, 1] >= 255.0 * (1 - TOL)] == 0x7c00).all(), tag


@pytest.mark.parametrize("name", sorted(cc.OFF_IMAGE))
def test_outputs_off_the_image_are_the_rounded_offset(aai, po, name):
    """none of the table's geometries has a dst row or column without weight (asserted: the check in the test above is vacuous there), so
    three fast-mode geometries that have one: those outputs are round(offset[c]) exactly, in every output type and both layouts, with at
    most 64 and with more than 64 outputs per strip, and the rest keeps the oracle's bar"""
    assert not any((cc.case(aai, po, g, c, m, st, "constant")[4] == 0).any() for g, c, st, _, _ in cc.CASES[::4] for m in cc.MODES)
    geom, C = cc.OFF_IMAGE[name], 3
    rq = ic.request(aai, geom, "fast")
    assert cc.facts(rq, C)[7] == 1
    for st in (ic.U8, ic.U16):
        src = ic.source(geom, C, st, "constant")
        gold = ic.oracle(po, geom, "fast", src)
        off = gold == 0
        assert off.any() and (off.all(axis=(1, 2)).any() or off.all(axis=(0, 2)).any()), name
        for conv in ("normalise", "edge"):
            scale, offset = cc.conversion(conv, st)
            for ot, _ in cc.OUT_TYPES:
                for lay in (cc.INTERLEAVED, cc.PLANAR):
                    out, pre = cc.replay(aai, rq, st, src, scale, offset, ot, lay)
                    hwc = cc.to_hwc(out, lay)
                    want = np.broadcast_to(cc.narrow(offset[:C], ot), hwc.shape)
                    assert np.array_equal(hwc[off], want[off]) and not pre[off].any(), (name, st, conv, ot, lay)
                    assert cc.excess(cc.as_float(hwc, ot), gold, scale, offset, ot) <= 0, (name, st, conv, ot, lay)


def test_replay_program_runs_clean_under_the_sanitizers(aai):
    """tests/cpp/convert_sanitize.cpp: the replay over the case table on exactly-sized heap buffers in a stand-alone program built with
    -fsanitize=address,undefined (nothing is loaded into python, nothing is preloaded)"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "convert_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "convert_sanitize.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    args = cc.sanitize_args(aai)
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert len(r.stdout.splitlines()) == len(args) == 2 * len(cc.CASES) and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the torch operator's argument checks (no device needed) -------------------------------------------------------------------------
def test_torch_operator_refuses_what_it_cannot_serve(aai):
    import torch
    x = torch.zeros((2, 3, 8, 8), dtype=torch.uint8)
    geometry = (2, 1, (3.5, 3.5), 0.0)
    with pytest.raises(ValueError, match="needs integer=True"):
        aai.resample(x, *geometry, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="needs integer=True"):
        aai.resample(x.float(), *geometry, out_dtype=torch.float32)
    for extra in (dict(half=True), dict(f64=True), dict(planned_backward=True), dict(sampler_backward=True), dict(half="channels_last", half_backward=True)):
        with pytest.raises(ValueError, match="has no gradient"):
            aai.resample(x, *geometry, integer=True, out_dtype=torch.float16, **extra)
    for bad in (torch.float64, torch.uint8, "float16"):
        with pytest.raises(ValueError, match="takes torch.float32, torch.float16 or torch.bfloat16"):
            aai.resample(x, *geometry, integer=True, out_dtype=bad)
    with pytest.raises(ValueError, match="out_memory_format"):
        aai.resample(x, *geometry, integer=True, out_dtype=torch.float16, out_memory_format=torch.preserve_format)
    with pytest.raises(ValueError, match="shape \\(B, C, H, W\\)"):
        aai.resample(x[0], *geometry, integer=True, out_dtype=torch.float16, out_memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="one value per channel"):
        aai.resample(x, *geometry, integer=True, out_dtype=torch.float16, scale=(1.0, 2.0))
    with pytest.raises(ValueError, match="at most 4 channels"):
        aai.resample(torch.zeros((1, 5, 8, 8), dtype=torch.uint8), *geometry, integer=True, out_dtype=torch.float16)
    with pytest.raises(TypeError, match="uint8 or uint16"):
        aai.resample(x.float(), *geometry, integer=True, out_dtype=torch.float16)
    # scale, offset and the output's memory format belong to out_dtype; without it integer=True is the integer operator, which has none
    for extra in (dict(scale=2.0), dict(offset=(0.0, 1.0, 2.0)), dict(out_memory_format=torch.channels_last)):
        with pytest.raises(ValueError, match="belong to out_dtype"):
            aai.resample(x, *geometry, integer=True, **extra)
    with pytest.raises(ValueError, match="on a GPU"):
        aai.resample(x, *geometry, integer=True, out_dtype=torch.bfloat16, scale=(1.0, 2.0, 3.0), offset=0.5, out_memory_format=torch.channels_last)
