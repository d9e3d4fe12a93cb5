"""The half-precision interleaved path (include/aai_half_interleaved.h: fp16 / bf16 images of 1..4 interleaved channels in, the same type
out), checks that need no GPU: ABI, argument errors call by call against the interleaved fp32 entries' recorded answers, which route
a request takes, and the serial CPU replay of the kernel with channels (tests/emulation/half_interleaved_emulation.cpp over
narrow_replay.hpp and the planner's tables) against the oracle per channel and against the single-channel replay of each plane.

The bars of the replay are the single-channel path's (tests/test_half_host.py): conftest.TOL before the rounding,
half_cases.rounded_excess <= 0 after it."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import half_cases as hc
import half_interleaved_cases as hi
import test_entry_point_errors as T
from conftest import ROOT, TOL, rel_err

ENTRIES = ("aai_resample_half_interleaved_device", "aai_resample_half_interleaved_host")
HALF_TYPE_MESSAGE = "Unknown half-precision element type."

# the two entries' arguments in ABI order with the values of a valid call, in the manner of test_entry_point_errors.ENTRIES
DEVICE_ARGS = [("req", 1), ("batch", 2), ("channels", 3), ("half_dtype", 1), ("src", T.FAKE_SRC), ("src_stride", T.BIG), ("src_image_stride", T.BIG * T.BIG),
               ("dst", T.FAKE_DST), ("dst_stride", T.BIG), ("dst_image_stride", T.BIG * T.BIG), ("stream", None)]
HOST_ARGS = [("req", 1), ("channels", 3), ("half_dtype", 2), ("src", T.FAKE_SRC), ("src_stride", T.BIG), ("dst", T.FAKE_DST), ("dst_stride", T.BIG),
             ("layout", None)]


def test_abi_declares_exports_and_binds_the_half_interleaved_entries(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aai_half_interleaved.h")).read()
    base = open(os.path.join(ROOT, "include", "aai.h")).read()
    half = open(os.path.join(ROOT, "include", "aai_half.h")).read()
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.HALF_INTERLEAVED_SYMBOLS and name not in L.SYMBOLS and name not in L.HALF_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == L.HALF_INTERLEAVED_SYMBOLS[name][1]
        assert name not in base and name not in half
    assert '#include "aai_half.h"' in header and lib.aai_version() == 2 and "#define AAI_VERSION_MINOR 2" in base
    for name in ("resample_half_interleaved_device", "resample_half_interleaved_host"):
        assert hasattr(aai, name) and name in aai.__all__
    for word in ("ties to even", "+widened", "aai_axis_half_kernel<f16>", "aai_axis_half_kernel<bf16>", "NOT PROVIDED", "row bands", "multi-device",
                 "half adjoint", "listed-pixel", "transposed quadrants", "stream capture", "2 bytes", "one unit in the last place",
                 "aai_resample_interleaved_device", "half_interleaved_time.txt"):
        assert word in header, word


def _call(lib, L, fn, arglist, faults):
    """test_entry_point_errors.call for an entry of this file: `half_dtype` takes the place of src_dtype"""
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


@pytest.mark.parametrize("entry, typed, arglist", [("aai_resample_half_interleaved_device", "aai_resample_interleaved_device", DEVICE_ARGS),
                                                   ("aai_resample_half_interleaved_host", "aai_resample_interleaved_host", HOST_ARGS)])
def test_argument_errors_are_those_of_the_interleaved_entries(aai, entry, typed, arglist):
    """Every single fault and every pair of faults of the fault table of tests/test_entry_point_errors.py: the entry answers what the
    interleaved fp32 entry of the same shape answered when tests/golden/entry_point_errors.json was recorded -- the same code and message
    in the same order, the bad element type with its own message in src_dtype's place -- and, fault for fault, what that entry answers in
    this process.  The one difference: an empty batch returns AAI_OK before the device check.  All of it before AAI_ERR_NO_DEVICE, with
    pointers that point nowhere."""
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
        # ... and the interleaved entry itself, here and now, wherever the probe stops before the device
        if want[0] not in (L.OK, L.ERR_NO_DEVICE):
            live = T.call(lib, L, typed, p)
            if live[1] == "Unknown source element type.":
                live[1] = HALF_TYPE_MESSAGE
            if live != got:
                wrong.append((key, got, "interleaved now", live))
    assert not wrong, wrong[:10]
    assert refused > 100
    # the element type: fp16 (1) and bf16 (2) only
    bad = dict(arglist)
    rq = L.Request(**T.BASE)
    bad["req"] = ctypes.byref(rq)
    for value in (0, 3, -1, 7):
        bad["half_dtype"] = value
        assert fn(*[bad[n] for n, _ in arglist]) == L.ERR_BAD_ARGUMENT and aai.last_error() == HALF_TYPE_MESSAGE, value
    # the channel count: 1..4, reported before the element type
    for value in (0, 5):
        bad["channels"], bad["half_dtype"] = value, 1
        assert fn(*[bad[n] for n, _ in arglist]) == L.ERR_BAD_ARGUMENT and aai.last_error() == "Channels must be 1..4.", value
    assert _call(lib, L, fn, arglist, ("null_request", "bad_dtype"))[1] == "Null request."
    assert _call(lib, L, fn, arglist, ("bad_policy", "bad_dtype"))[1] == "Unknown weight policy."
    assert _call(lib, L, fn, arglist, ("channels_five", "bad_dtype"))[1] == "Channels must be 1..4."
    assert _call(lib, L, fn, arglist, ("channels_zero", "bad_dtype"))[1] == "Channels must be 1..4."
    assert _call(lib, L, fn, arglist, ("bad_dtype", "res_mismatch"))[1] == HALF_TYPE_MESSAGE
    assert _call(lib, L, fn, arglist, ("bad_dtype", "null_src"))[1] == HALF_TYPE_MESSAGE


def test_api_wrappers_report_the_same(aai):
    from area_average_interpolation_amd import _lib as L
    rq = aai.make_request(24, 20, 3, 1, (11.5, 9.5), 0.0)
    with pytest.raises(aai.AaiError) as e:
        aai.resample_half_interleaved_device(rq, 3, 8, 72, 8, 24, 0)
    assert HALF_TYPE_MESSAGE in str(e.value)
    with pytest.raises(aai.AaiError) as e:
        aai.resample_half_interleaved_device(rq, 5, 8, 120, 8, 40, L.HALF_F16)
    assert "Channels must be 1..4." in str(e.value)
    aai.resample_half_interleaved_device(rq, 3, 8, 72, 8, 24, L.HALF_BF16, batch=0)      # returns before the device
    rc, msg, dst, iso, lay = aai.resample_half_interleaved_host(np.zeros((4, 4, 3), np.float16), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and dst is None and msg == "Assumed X & Y resolution are same."
    rc, msg, dst, iso, lay = aai.resample_half_interleaved_host(np.zeros((0, 0), np.uint16), 1, 1, (0, 0), 0)
    assert rc == L.ERR_NO_ROWS and dst is None
    with pytest.raises(TypeError):
        aai.resample_half_interleaved_host(np.zeros((4, 4, 3), np.float32), 1, 1, (0, 0), 0)
    if aai.device_count() == 0:
        rc, msg, dst, iso, lay = aai.resample_half_interleaved_host(np.zeros((8, 8, 3), np.float16), 2, 1, (3.5, 3.5), 0)
        assert rc == L.ERR_NO_DEVICE and dst is None


def test_an_unknown_half_string_is_refused_by_the_torch_operator(aai):
    """half="channel_last" must not silently mean half=True (a copy and a planar result): ValueError, before the tensor is looked at"""
    import torch
    x = torch.ones((2, 3, 8, 8), dtype=torch.float16)
    for bad in ("channel_last", "Channels_Last", "true", ""):
        with pytest.raises(ValueError, match="half must be"):
            aai.resample(x, 2, 1, (3.5, 3.5), 0.0, half=bad)
    with pytest.raises(ValueError, match="on a GPU"):      # the two accepted spellings get as far as the device check
        aai.resample(x, 2, 1, (3.5, 3.5), 0.0, half="channels_last")


# ---- which route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom, channels", hi.CASES, ids=hi.CASE_IDS)
def test_direct_route_cases_are_served(aai, hostemu, geom, channels):
    """every case takes the separable path, lists no pixel in either mode, is not wide, holds at most 256 outputs per strip with its
    channel count and at least 4 elements in a row -- asserted here so that a change of the planner cannot silently move a case to the
    forwarding route -- and reaches what half_interleaved_cases says it is there for"""
    W, H = hi.GEOMETRIES[geom][:2]
    back = hi.GEOMETRIES[geom][5] == 180.0
    for mode_name in hi.MODES:
        rq = hi.request(aai, geom, mode_name)
        axis, wide, transposed, strips, most, shared, rowspan, direct = hi.facts(rq, channels)
        assert (axis, wide, transposed, direct) == (1, 0, 0, 1), (geom, channels, mode_name)
        assert 1 <= most <= 256 and W * channels >= 4
        out, took_axis = hostemu.resample(rq, np.random.default_rng(3).random((H, W), dtype=np.float32))
        assert took_axis and hostemu.aai_emu_axis_fixups() == 0, (geom, mode_name)
        if mode_name == "area":
            if geom == "a":
                assert strips == 1 and most <= 64 and not back
            if geom in ("b", "m"):
                assert strips >= 2 and back == (geom == "m") and (shared == 1 or geom == "m")
            if geom == "c":
                assert strips > 8 and strips % 4 and most <= 64 and back      # more than two workgroups of strips, the last partial
            if geom == "d":
                assert strips == 1 and 65 <= most <= 256 and not back
            if geom in ("e", "l"):
                assert 65 <= most <= 256 and back
            if geom == "g":
                assert rowspan == 13
    if (geom, channels) in (("b", 3), ("m", 3)):
        assert W * channels == 777 and (W * channels) % 4
    if geom == "n":
        assert W * channels == 4


def test_strip_forms_and_store_shapes_are_all_reached(aai):
    """one output per lane (<= 64 per strip) and four per lane (> 64), each packed forwards (0 degrees) and element by element (180
    degrees with channels); every channel count 2, 3, 4 in both strip forms"""
    seen, per_channel = set(), set()
    for geom, channels in hi.CASES:
        most = hi.facts(hi.request(aai, geom, "area"), channels)[4]
        back = hi.GEOMETRIES[geom][5] == 180.0
        seen.add((most <= 64, back))
        per_channel.add((channels, most <= 64))
    assert seen == {(s, b) for s in (True, False) for b in (True, False)}, seen
    assert per_channel == {(c, s) for c in (2, 3, 4) for s in (True, False)}, per_channel


def test_a_row_of_three_elements_is_not_served(aai):
    geom, channels = hi.FORWARDS
    W = hi.GEOMETRIES[geom][0]
    assert W * channels == 3
    for mode_name in hi.MODES:
        rq = hi.request(aai, geom, mode_name)
        f = hi.facts(rq, channels)
        assert f[0] == 1 and f[7] == 0, f
        src = hi.source_bits(geom, channels, hi.F16)
        out = np.zeros((rq.src_height, W, channels), np.uint16)
        assert hi.emu().aai_emu_half_interleaved_replay(ctypes.byref(rq), channels, hi.F16, src.ctypes.data, out.ctypes.data, None) == -1
    # ... and one more channel makes it the narrowest served image
    assert hi.facts(hi.request(aai, geom, "area"), 4)[7] == 1


FORWARDED = [("rotated", (96, 80, 3, 1, (47.5, 39.5), 17.5), "area"), ("case b at 90 degrees", hi.GEOMETRIES["b"][:5] + (90.0,), "area"),
             ("bicubic", hi.GEOMETRIES["a"], "bicubic"), ("a wide-kernel ratio", (900, 300, 300, 1, (449.5, 149.5), 0.0), "area")]


@pytest.mark.parametrize("name, geom, mode_name", FORWARDED, ids=[f[0] for f in FORWARDED])
def test_forwarded_examples_do_not_take_the_direct_route(aai, name, geom, mode_name):
    W, H, sr, dr, iso, ang = geom
    mode = {"area": aai.MODE_AREA, "bicubic": aai.MODE_BICUBIC}[mode_name]
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    for channels in (2, 3, 4):
        f = hi.facts(rq, channels)
        assert f[7] == 0, (name, channels, f)


# ---- the replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("mode_name", hi.MODES)
@pytest.mark.parametrize("geom, channels", hi.CASES, ids=hi.CASE_IDS)
def test_cpu_replay_matches_the_oracle_per_channel(aai, po, geom, channels, mode_name, ht, tname):
    rq, src, out, pre, gold = hi.case(aai, po, geom, channels, mode_name, ht)
    assert out.shape == gold.shape == pre.shape and out.shape[2] == channels and not np.isnan(pre).any()
    wide = hc.widen(src, ht)
    assert wide.min() >= 0.25 and wide.max() <= 1.25 and np.array_equal(hc.narrow(wide, ht), src)
    for c in range(channels):
        before = float(rel_err(pre[:, :, c], gold[:, :, c]).max())
        after = hc.rounded_excess(hc.widen(out[:, :, c], ht), gold[:, :, c], ht)
        print("replay %s x%d channel %d %s %s: before the rounding %.3e (bar %.0e), after it %.3e over the bound" % (geom, channels, c, mode_name, tname, before, TOL, after))
        assert before <= TOL, (geom, channels, c, mode_name, tname, before)
        assert after <= 0, (geom, channels, c, mode_name, tname, after)
    # one rounding: the stored element is the rounded fp32 value, and dst pixels off the image are +0
    assert np.array_equal(out, hc.narrow(pre, ht))
    assert np.array_equal(gold == 0, out == 0)


@pytest.mark.parametrize("ht, tname", hi.TYPES, ids=[t[1] for t in hi.TYPES])
@pytest.mark.parametrize("mode_name", hi.MODES)
@pytest.mark.parametrize("geom, channels", hi.CASES, ids=hi.CASE_IDS)
def test_channels_are_the_single_channel_replay_of_each_plane(aai, po, geom, channels, mode_name, ht, tname):
    """The channels are independent: channel c of the replay with C channels against the SINGLE-channel replay (half_cases.replay, the one
    the single-channel kernel is held to) of de-interleaved plane c.  The two walk different strips -- 256 elements are 256 / C pixels --
    but every output sums the same taps with the same weights in the same order, so this asserts BIT EQUALITY, before and after the
    rounding: it holds on every case and type here.  (Case n is skipped for this comparison only: a plane of 2 pixels is narrower than
    the single-channel strip form serves.)"""
    rq, src, out, pre, gold = hi.case(aai, po, geom, channels, mode_name, ht)
    if rq.src_width < 4:
        assert geom == "n"
        return
    for c in range(channels):
        alone, alone_pre = hc.replay(aai, rq, ht, np.ascontiguousarray(src[:, :, c]))
        assert int(hc.ulp_distance(alone, out[:, :, c]).max()) <= 1, (geom, channels, c)
        assert np.array_equal(alone_pre, pre[:, :, c]) and np.array_equal(alone, out[:, :, c]), (geom, channels, c, mode_name, tname)
