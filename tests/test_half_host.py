"""The half-precision path (include/aai_half.h: fp16 / bf16 images in, the same type out), checks that need no GPU: ABI, argument errors
call by call against the fp32 entries' recorded answers, the portable rounding helpers against numpy and torch over the fp32 bit
patterns that matter, and the serial CPU replay of the direct kernel (tests/emulation/half_emulation.cpp over narrow_replay.hpp,
csrc/aai_half_math.hpp and the planner's tables) against the oracle on the direct-route geometries.

The two bars of the replay:
  before the rounding   the fp32 value against the oracle on the widened source: conftest.TOL relative, with the suite's floor of 1e-3
  after it              |got - gold| <= u |gold| (1 + TOL) + TOL max(|gold|, 1e-3), u = 2^-11 (fp16) or 2^-8 (bf16): ONE rounding to
                        the element type on top of the project's bar"""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest

import half_cases as hc
import test_entry_point_errors as T
from conftest import ROOT, TOL, rel_err

ENTRIES = ("aai_resample_half_batch_device", "aai_resample_half_host")
HALF_TYPE_MESSAGE = "Unknown half-precision element type."

# the two entries' arguments in ABI order with the values of a valid call, in the manner of test_entry_point_errors.ENTRIES
DEVICE_ARGS = [("req", 1), ("batch", 2), ("half_dtype", 1), ("src", T.FAKE_SRC), ("src_stride", T.BIG), ("src_image_stride", T.BIG * T.BIG),
               ("dst", T.FAKE_DST), ("dst_stride", T.BIG), ("dst_image_stride", T.BIG * T.BIG), ("stream", None)]
HOST_ARGS = [("req", 1), ("half_dtype", 2), ("src", T.FAKE_SRC), ("src_stride", T.BIG), ("dst", T.FAKE_DST), ("dst_stride", T.BIG), ("layout", None)]


def test_abi_declares_exports_and_binds_the_half_entries(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aai_half.h")).read()
    base = open(os.path.join(ROOT, "include", "aai.h")).read()
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        # (_lib.SYMBOLS is the table of include/aai.h alone, which tests/test_host_logic.py compares with that header: an extension
        # header's entries have a table of their own, like F64_SYMBOLS)
        assert name in L.HALF_SYMBOLS and name not in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == L.HALF_SYMBOLS[name][1]
        assert name not in base
    assert re.search(r"AAI_HALF_F16\s*=\s*1\s*,\s*AAI_HALF_BF16\s*=\s*2", header)
    assert (L.HALF_F16, L.HALF_BF16) == (1, 2) == (aai.HALF_F16, aai.HALF_BF16) == (hc.F16, hc.BF16)
    assert '#include "aai.h"' in header and lib.aai_version() == 2 and "#define AAI_VERSION_MINOR 2" in base
    for name in ("resample_half_device", "resample_half_host", "HALF_F16", "HALF_BF16"):
        assert hasattr(aai, name) and name in aai.__all__
    for word in ("interleaved channels", "row bands", "multi-device", "adjoint", "listed-pixel", "transposed quadrants", "stream capture"):
        assert word in header, word


def _call(lib, L, fn, arglist, faults):
    """test_entry_point_errors.call for an entry of this file: the element type takes the place of src_dtype"""
    fields, args = dict(T.BASE), dict(arglist)
    for f in faults:
        for k, v in T.FAULTS[f].items():
            if k.startswith("rq."):
                fields[k[3:]] = v
            else:
                args["half_dtype" if k == "src_dtype" else k] = v
    rq = L.Request(**fields)
    args["req"] = ctypes.byref(rq) if args["req"] else None
    lay = L.Layout()
    assert lib.aai_query(ctypes.byref(L.Request(**T.BASE)), ctypes.byref(lay)) == L.OK and lib.aai_last_error() == b""
    rc = fn(*[args[n] for n, _ in arglist])
    return [rc, lib.aai_last_error().decode()]


@pytest.mark.parametrize("entry, typed, arglist", [("aai_resample_half_batch_device", "aai_resample_batch_device", DEVICE_ARGS),
                                                   ("aai_resample_half_host", "aai_resample_host", HOST_ARGS)])
def test_argument_errors_are_those_of_the_fp32_entries(aai, entry, typed, arglist):
    """Every single fault and every pair of faults of the fault table of tests/test_entry_point_errors.py: the half entry answers what the
    typed fp32 entry of the same shape answered when tests/golden/entry_point_errors.json was recorded (aai_resample_batch_device, which
    is aai_resample_batch_device_f32 plus the check of its element type; aai_resample_host) -- the same code and message in the same
    order, the bad element type with its own message in src_dtype's place -- and, fault for fault, what aai_resample_batch_device_f32
    answers in this process.  The one difference: an empty batch returns AAI_OK before the device check.  All of it before
    AAI_ERR_NO_DEVICE, with pointers that point nowhere."""
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
            want[1] = HALF_TYPE_MESSAGE
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
        # ... and the fp32 entry itself, here and now, wherever the probe exists for it and stops before the device
        f32 = "aai_resample_batch_device_f32"
        if "batch" in dict(arglist) and all(T._applies(f, f32) for f in p) and want[0] not in (L.OK, L.ERR_NO_DEVICE):
            live = T.call(lib, L, f32, p)
            if live != got:
                wrong.append((key, got, "f32 now", live))
    assert not wrong, wrong[:10]
    assert refused > 100
    # the element type: checked behind the request and before everything else, like src_dtype
    bad = dict(arglist, half_dtype=0)
    rq = L.Request(**T.BASE)
    bad["req"] = ctypes.byref(rq)
    for value in (0, 3, -1, 7):
        bad["half_dtype"] = value
        assert fn(*[bad[n] for n, _ in arglist]) == L.ERR_BAD_ARGUMENT and aai.last_error() == HALF_TYPE_MESSAGE, value
    assert _call(lib, L, fn, arglist, ("null_request", "bad_dtype"))[1] == "Null request."
    assert _call(lib, L, fn, arglist, ("bad_policy", "bad_dtype"))[1] == "Unknown weight policy."
    assert _call(lib, L, fn, arglist, ("bad_dtype", "res_mismatch"))[1] == HALF_TYPE_MESSAGE
    assert _call(lib, L, fn, arglist, ("bad_dtype", "null_src"))[1] == HALF_TYPE_MESSAGE


def test_api_wrappers_report_the_same(aai):
    from area_average_interpolation_amd import _lib as L
    with pytest.raises(aai.AaiError) as e:
        aai.resample_half_device(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 0.0), 8, 24, 8, 8, 9)
    assert HALF_TYPE_MESSAGE in str(e.value)
    aai.resample_half_device(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 0.0), 8, 24, 8, 8, aai.HALF_BF16, batch=0)      # returns before the device
    rc, msg, dst, iso, lay = aai.resample_half_host(np.zeros((4, 4), np.float16), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and dst is None and msg == "Assumed X & Y resolution are same."
    rc, msg, dst, iso, lay = aai.resample_half_host(np.zeros((0, 0), np.uint16), 1, 1, (0, 0), 0)
    assert rc == L.ERR_NO_ROWS and dst is None
    with pytest.raises(TypeError):
        aai.resample_half_host(np.zeros((4, 4), np.float32), 1, 1, (0, 0), 0)
    if aai.device_count() == 0:
        rc, msg, dst, iso, lay = aai.resample_half_host(np.zeros((8, 8), np.float16), 2, 1, (3.5, 3.5), 0)
        assert rc == L.ERR_NO_DEVICE and dst is None


# ---- the rounding helpers ----------------------------------------------------------------------------------------------------
LOW_BITS = (0x00, 0x7f, 0x80, 0x81, 0xff)


def _same_or_nan(got_bits, want_bits, nan_mask_bits, what):
    """equal bits wherever the expected value is no NaN; a NaN wherever it is (exp_mask all ones, mantissa not 0)"""
    exp, man = nan_mask_bits
    want_nan = ((want_bits & exp) == exp) & ((want_bits & man) != 0)
    got_nan = ((got_bits & exp) == exp) & ((got_bits & man) != 0)
    assert np.array_equal(got_nan, want_nan), what
    assert np.array_equal(got_bits[~want_nan], want_bits[~want_nan]), what


def test_fp16_rounding_against_numpy():
    """every fp32 bit pattern whose low 8 mantissa bits are 0x00, 0x7f, 0x80, 0x81 or 0xff (5 x 2^24 values): the 13 bits that fp16 drops
    are then everything below, at and above the halfway point in every exponent, both signs"""
    hi = np.arange(1 << 24, dtype=np.uint32) << 8
    for low in LOW_BITS:
        f = (hi | np.uint32(low)).view(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            want = f.astype(np.float16).view(np.uint16)
        _same_or_nan(hc.narrow(f, hc.F16), want, (0x7c00, 0x03ff), hex(low))


def test_bf16_rounding_against_torch():
    torch = pytest.importorskip("torch")
    hi = np.arange(1 << 24, dtype=np.uint32) << 8
    for low in LOW_BITS:
        f = (hi | np.uint32(low)).view(np.float32)
        want = torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        _same_or_nan(hc.narrow(f, hc.BF16), want, (0x7f80, 0x007f), hex(low))


def test_rounding_ties_subnormals_overflow_and_non_finite_values():
    f32 = lambda bits: np.asarray(bits, np.uint32).view(np.float32)
    # every tie: the midpoint of two neighbouring values of the type is an fp32 number (11 / 8 significant bits + 1) and goes to the even one
    b = np.arange(0, 0x7bff, dtype=np.uint16)
    mid = ((hc.widen(b, hc.F16).astype(np.float64) + hc.widen(b + 1, hc.F16).astype(np.float64)) / 2).astype(np.float32)
    even = np.where(b & 1, b + 1, b).astype(np.uint16)
    assert np.array_equal(hc.narrow(mid, hc.F16), even) and np.array_equal(hc.narrow(-mid, hc.F16), even | 0x8000)
    assert np.array_equal(hc.narrow(np.nextafter(mid, np.float32(np.inf)), hc.F16), b + 1)
    assert np.array_equal(hc.narrow(np.nextafter(mid, np.float32(-np.inf)), hc.F16), b)
    b = np.arange(0, 0x7f7f, dtype=np.uint16)
    mid = ((hc.widen(b, hc.BF16).astype(np.float64) + hc.widen(b + 1, hc.BF16).astype(np.float64)) / 2).astype(np.float32)
    even = np.where(b & 1, b + 1, b).astype(np.uint16)
    assert np.array_equal(hc.narrow(mid, hc.BF16), even) and np.array_equal(hc.narrow(-mid, hc.BF16), even | 0x8000)
    assert np.array_equal(hc.narrow(np.nextafter(mid, np.float32(np.inf)), hc.BF16), b + 1)
    assert np.array_equal(hc.narrow(np.nextafter(mid[1:], np.float32(-np.inf)), hc.BF16), b[1:])
    # every value of the type survives the round trip (subnormals and both zeros among them), and widening is numpy's
    for ht, last in ((hc.F16, 0x7c00), (hc.BF16, 0x7f80)):
        b = np.concatenate([np.arange(0, last + 1), np.arange(0x8000, 0x8000 + last + 1)]).astype(np.uint16)
        assert np.array_equal(hc.narrow(hc.widen(b, ht), ht), b), ht
        mine = np.empty(b.shape, np.float32)
        (hc.emu().aai_emu_f16_to_f32 if ht == hc.F16 else hc.emu().aai_emu_bf16_to_f32)(b.ctypes.data, mine.ctypes.data, b.size)
        assert np.array_equal(mine.view(np.uint32), hc.widen(b, ht).view(np.uint32)), ht
    # the overflow threshold: 65520 = the midpoint of 65504 and 2^16 goes to Inf, the number below it to 65504
    assert list(hc.narrow(np.float32([65520.0, -65520.0, np.nextafter(np.float32(65520.0), np.float32(0)), 65504.0, 1e30, -1e30]), hc.F16)) == \
        [0x7c00, 0xfc00, 0x7bff, 0x7bff, 0x7c00, 0xfc00]
    assert list(hc.narrow(f32([0x7f7f8000, 0xff7f8000, 0x7f7f7fff, 0x7f7fffff]), hc.BF16)) == [0x7f80, 0xff80, 0x7f7f, 0x7f80]
    # the smallest subnormal and the tie below it
    assert list(hc.narrow(np.float32([2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -26, 1.5 * 2.0 ** -24]), hc.F16)) == \
        [1, 0, 1, 0, 2]
    # Inf stays Inf, NaN stays NaN with its sign, whatever its payload
    for ht, inf, man in ((hc.F16, 0x7c00, 0x03ff), (hc.BF16, 0x7f80, 0x007f)):
        assert list(hc.narrow(np.float32([np.inf, -np.inf]), ht)) == [inf, inf | 0x8000]
        nan = hc.narrow(f32([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff]), ht)
        assert np.all((nan & inf) == inf) and np.all((nan & man) != 0)
        assert list(nan >> 15) == [0, 1, 0, 1, 0]
        wide = hc.widen(nan, ht)
        assert np.isnan(wide).all()


# ---- the replay ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def replay_case(aai, po, case, mode_name, ht):
    """-> (request, source bits, replay bits, replay fp32 values before the rounding, the oracle on the widened source); computed once"""
    W, H, sr, dr, iso, ang = hc.CASES[case] if isinstance(case, str) else case
    rq = hc.request(aai, case, mode_name)
    src = hc.source_bits(W, H, ht)
    out, pre = hc.replay(aai, rq, ht, src)
    gold = po.oracle_run(hc.oracle_mode(po, mode_name), hc.widen(src, ht).astype(np.float64), sr, dr, iso, ang).dst
    for a in (src, out, pre, gold):
        a.setflags(write=False)
    return rq, src, out, pre, gold


# The tails of the store of a strip of at most 64 outputs, where neighbouring lanes exchange their elements and the first of them stores
# them: W x 8 images at 4:1, grid-aligned, at 0 and 180 degrees -> ONE strip of W / 4 = 5, 6, 7 outputs, so that the last quad of lanes
# holds 1, 2, 3 live outputs (and the last pair 1, 2, 1), and 2 output rows.  Geometries as in hc.CASES, kept out of it: the integer
# tests iterate that table too.
TAIL_CASES = [pytest.param((W, 8, 4, 1, ((W - 1) / 2, 3.5), ang), id="tail%d@%d" % (W // 4, ang)) for W in (20, 24, 28) for ang in (0.0, 180.0)]


@pytest.mark.parametrize("case", TAIL_CASES)
def test_tail_cases_reach_the_small_strip_store(aai, case):
    """the direct route, one strip of 5, 6 or 7 outputs, two output rows -- asserted so that a tail case cannot silently move to the
    other horizontal form or to the forwarding route"""
    W = case[0]
    for mode_name in hc.MODES:
        rq = hc.request(aai, case, mode_name)
        axis, wide, transposed, strips, most, shared, rowspan, direct = hc.facts(rq)
        assert (axis, wide, transposed, direct) == (1, 0, 0, 1), (case, mode_name)
        assert strips == 1 and most == W // 4 <= 64 and most % 4 in (1, 2, 3), (case, mode_name, strips, most)
        lay = aai.query(rq)[2]
        assert (lay.dst_width, lay.dst_height) == (W // 4, 2), (case, mode_name)


# what the table of the issue says a case reaches: (strips, most outputs in a strip, most source rows of a window); None = not pinned
REACHES = {"b": (2, None, None), "c": (5, None, None), "d": (None, 67, None), "e": (None, 140, None), "g": (None, None, 13), "l": (None, 221, None)}


@pytest.mark.parametrize("case", sorted(hc.CASES))
def test_direct_route_cases_stay_on_the_direct_route(aai, hostemu, case):
    """every case takes the separable path, lists no pixel in either mode and is not wide -- asserted here so that a change of the
    planner cannot silently move a case to the forwarding route -- and reaches what it is there for"""
    W, H, sr, dr, iso, ang = hc.CASES[case]
    for mode_name in hc.MODES:
        rq = hc.request(aai, case, mode_name)
        axis, wide, transposed, strips, most, shared, rowspan, direct = hc.facts(rq)
        assert (axis, wide, transposed, direct) == (1, 0, 0, 1), (case, mode_name)
        out, took_axis = hostemu.resample(rq, np.random.default_rng(3).random((H, W), dtype=np.float32))
        assert took_axis and hostemu.aai_emu_axis_fixups() == 0, (case, mode_name)
        rc, (n_strips, most_outputs, is_wide, max_rows) = hostemu.strip_stats(rq)
        assert rc == 0 and is_wide == 0 and (n_strips, most_outputs, max_rows) == (strips, most, rowspan)
        assert 1 <= most <= 256
        want = REACHES.get(case, (None, None, None))
        if mode_name == "area":
            for got, w in zip((strips, most, rowspan), want):
                assert w is None or got == w, (case, (strips, most, rowspan), want)
    if case == "b":
        assert W % 4 and hc.facts(hc.request(aai, case, "area"))[5] == 1      # output rows share source rows
    if case == "h":
        assert W == 5


@pytest.mark.parametrize("ht, tname", hc.TYPES, ids=[t[1] for t in hc.TYPES])
@pytest.mark.parametrize("mode_name", hc.MODES)
@pytest.mark.parametrize("case", sorted(hc.CASES) + TAIL_CASES)
def test_cpu_replay_matches_the_oracle(aai, po, case, mode_name, ht, tname):
    rq, src, out, pre, gold = replay_case(aai, po, case, mode_name, ht)
    assert pre.shape == gold.shape and not np.isnan(pre).any()
    # the source really is in the element type, in [0.25, 1.25]
    wide = hc.widen(src, ht)
    assert wide.min() >= 0.25 and wide.max() <= 1.25 and np.array_equal(hc.narrow(wide, ht), src)
    before = float(rel_err(pre, gold).max())
    after = hc.rounded_excess(hc.widen(out, ht), gold, ht)
    print("replay %s %s %s: before the rounding %.3e (bar %.0e), after it %.3e over the bound" % (case, mode_name, tname, before, TOL, after))
    assert before <= TOL, (case, mode_name, tname, before)
    assert after <= 0, (case, mode_name, tname, after)
    # one rounding: the stored element is the rounded fp32 value, and dst pixels off the image are +0
    assert np.array_equal(out, hc.narrow(pre, ht))
    assert np.array_equal(gold == 0, out == 0)
