"""The interleaved planned adjoint at multiples of 90 degrees (include/aai_adjoint_planned_interleaved.h:
aai_adjoint_planned_interleaved_device_f32 / aai_adjoint_planned_interleaved_f32), checks that need no GPU: the ABI, argument errors call
by call against the existing interleaved entries, the python wrappers, and a serial CPU replay of the path
(tests/emulation/axis_adjoint_multi_emulation.cpp: the single-channel plan's tables, their inversion and lists, the kernel's
lane-per-element order with fused multiply-adds, the listed overwrite by adjoint_normalised_multi / adjoint_gather_multi) whose every
channel must equal, BIT FOR BIT, the single-channel replay (axis_adjoint_emulation.cpp) on that plane -- no tolerance anywhere in this
file."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import BUILD, GOLDEN, ROOT
from test_adjoint_planned_host import axisemu                               # noqa: F401  (the single-channel replay's fixture)
from test_adjoint_planned_gpu import MATRIX                                 # (the geometries only: nothing there runs at import)

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")
ENTRIES = ("aai_adjoint_planned_interleaved_device_f32", "aai_adjoint_planned_interleaved_f32")
CHANNELS = (2, 3, 4)


def test_header_declares_library_exports_and_lib_binds_the_entries(aai):
    from area_average_interpolation_amd import _lib as L
    from area_average_interpolation_amd import api
    header = open(os.path.join(ROOT, "include", "aai_adjoint_planned_interleaved.h")).read()
    assert '#include "aai.h"' in header
    assert "aai_adjoint_rotated_prepare" in header                   # no prepare entry of its own: said where the entries are declared
    lib = L.load()
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    rq, ly = ctypes.POINTER(L.Request), ctypes.POINTER(L.Layout)
    args = {ENTRIES[0]: [rq, i32, i32, p, i64, i64, p, i64, i64, p], ENTRIES[1]: [rq, i32, p, i64, p, i64, ly]}
    existing = dict(zip(ENTRIES, ("aai_adjoint_interleaved_device_f32", "aai_adjoint_interleaved_f32")))
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.PLANNED_INTERLEAVED_ADJOINT_SYMBOLS and name not in L.SYMBOLS
        assert L.PLANNED_INTERLEAVED_ADJOINT_SYMBOLS[name][0] is ctypes.c_int and list(L.PLANNED_INTERLEAVED_ADJOINT_SYMBOLS[name][1]) == args[name]
        # the argument list of the existing interleaved entry
        assert list(L.PLANNED_INTERLEAVED_ADJOINT_SYMBOLS[name][1]) == list(L.INTERLEAVED_ADJOINT_SYMBOLS[existing[name]][1]), name
    assert len(L.PLANNED_INTERLEAVED_ADJOINT_SYMBOLS) == 2
    assert not re.search(r"\bint\s+aai_adjoint_planned_interleaved\w*prepare\b", header)
    assert not hasattr(lib, "aai_adjoint_planned_interleaved_prepare")
    assert lib.aai_version() == 2                                    # additions in a header of their own: the version stays 0.2
    main = open(os.path.join(ROOT, "include", "aai.h")).read()
    for name in ENTRIES:
        assert name not in main
    # the python surface: the keyword exists, defaults to the existing behaviour
    for fn in (aai.adjoint_interleaved_device, aai.adjoint_interleaved_host):
        assert inspect.signature(fn).parameters["planned"].default is False
    assert api._ADJOINT_ENTRY[True, "separable"] == ENTRIES
    src = open(os.path.join(ROOT, "area_average_interpolation_amd", "torch_ops.py")).read()
    assert re.search(r"def resample\([^)]*planned_backward=False\)", src) and '"channels_last"' in src


def _calls(lib):
    """(existing entry, new entry) pairs with one signature: device, host"""
    def dev(fn):
        return lambda rq, channels=3, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20: fn(
            None if rq is None else ctypes.byref(rq), batch, channels, gdst, dst_stride, 0, gsrc, src_stride, 0, None)

    def host(fn):
        return lambda rq, channels=3, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20: fn(
            None if rq is None else ctypes.byref(rq), channels, gdst, dst_stride, gsrc, src_stride, None)
    return [(dev(lib.aai_adjoint_interleaved_device_f32), dev(lib.aai_adjoint_planned_interleaved_device_f32)),
            (host(lib.aai_adjoint_interleaved_f32), host(lib.aai_adjoint_planned_interleaved_f32))]


def test_new_entries_refuse_what_the_existing_interleaved_entries_refuse(aai):
    """the probe set of test_adjoint_rotated_interleaved_host.py; dummy (never dereferenced) pointers: every call below returns before the
    device is touched, with the existing entry's code and message"""
    from area_average_interpolation_amd import _lib as L
    lib = L.load()

    def same(pair, *a, **k):
        rc0 = pair[0](*a, **k)
        msg0 = aai.last_error()
        rc1 = pair[1](*a, **k)
        assert rc1 == rc0 and aai.last_error() == msg0, (a, k, rc0, rc1, msg0, aai.last_error())
        return rc0, msg0

    probes = json.load(open(os.path.join(GOLDEN, "error_paths.json")))
    rejected = 0
    for p in probes:
        if p["kind"] == "args":
            rq = aai.make_request(4, 4, p["src_res"], p["dst_res"], (0, 0), 0, mode=p["mode"])
        else:
            rq = aai.make_request(0 if p["rows"] else 4, p["rows"], 1, 1, (0, 0), 0, mode=p["mode"])
        rc, msg, _ = aai.query(rq)
        if rc == L.OK:
            continue
        rejected += 1
        for pair in _calls(lib):
            assert same(pair, rq) == (rc, msg), p
    assert rejected >= 4
    W, H, C = 24, 20, 3
    # a rotated and an axis-aligned request: validation does not depend on which path would serve them
    for ang in (17.5, 0.0):
        mk = lambda **k: aai.make_request(W, H, 3, 1, (11.5, 9.5), ang, **k)
        ok = mk()
        lay = aai.query(ok)[2]
        for pair in _calls(lib):
            for channels in (0, 5):
                rc, msg = same(pair, ok, channels=channels)
                assert rc == L.ERR_BAD_ARGUMENT and "Channels" in msg
            for mode, name in ((L.MODE_BILINEAR, "BILINEAR"), (L.MODE_BICUBIC, "BICUBIC")):
                rc, msg = same(pair, mk(mode=mode))
                assert rc == L.ERR_BAD_ARGUMENT and name in msg
            rc, msg = same(pair, mk(policy=L.POLICY_DIAG_NO_FIXUP))
            assert rc == L.ERR_BAD_ARGUMENT and "DIAG_NO_FIXUP" in msg
            rc, msg = same(pair, mk(policy=0x800))                          # an unknown policy bit
            assert rc == L.ERR_BAD_ARGUMENT and msg == "Unknown weight policy."
            rc, msg = same(pair, ok, src_stride=W * C - 1)
            assert rc == L.ERR_BAD_ARGUMENT and "Source stride" in msg
            rc, msg = same(pair, ok, src_stride=W)                          # a stride that would do for one channel
            assert rc == L.ERR_BAD_ARGUMENT and "Source stride" in msg
            rc, msg = same(pair, ok, dst_stride=lay.dst_width * C - 1)
            assert rc == L.ERR_BAD_ARGUMENT and "Destination stride" in msg
            assert same(pair, ok, gdst=None)[0] == L.ERR_BAD_ARGUMENT and same(pair, ok, gsrc=None)[0] == L.ERR_BAD_ARGUMENT
            assert same(pair, None)[0] == L.ERR_BAD_ARGUMENT
            # two faults: the earlier check speaks (channels before the mode, the mode before the pointers)
            assert "Channels" in same(pair, mk(mode=L.MODE_BICUBIC), channels=5)[1]
            assert "BICUBIC" in same(pair, mk(mode=L.MODE_BICUBIC), gdst=None)[1]
        device = _calls(lib)[0]
        rc, msg = same(device, ok, batch=-1)
        assert rc == L.ERR_BAD_ARGUMENT and "batch" in msg
        for channels in (1, 2, 3, 4):
            assert same(device, ok, channels=channels, batch=0)[0] == L.OK  # returns before the device is touched
        hints = mk(policy=L.POLICY_DOUBLE_PRECISION | L.POLICY_PREFER_CELL | L.POLICY_EXACT)
        assert same(device, hints, batch=0)[0] == L.OK
    # a row of width x channels elements beyond what the interleaved entries accept
    wide = aai.make_request(400_000_000, 2, 1, 1, (0, 0), 0)
    rc, msg = same(_calls(lib)[0], wide, channels=4, batch=0, dst_stride=1 << 40, src_stride=1 << 40)
    assert rc != L.OK


def test_api_wrappers_take_separable_on_the_interleaved_wrappers_only(aai):
    from area_average_interpolation_amd import _lib as L
    from area_average_interpolation_amd import api
    W, H, C = 24, 20, 3
    for ang in (0.0, 17.5):
        ok = aai.make_request(W, H, 3, 1, (11.5, 9.5), ang)
        lay = aai.query(ok)[2]
        g = np.zeros((lay.dst_height, lay.dst_width, C), np.float32)
        for bad in (True, "sums", "planned", 1, None):
            with pytest.raises(ValueError):
                aai.adjoint_interleaved_device(ok, C, 8, 1 << 20, 8, 1 << 20, planned=bad)
            with pytest.raises(ValueError):
                aai.adjoint_interleaved_host(g, (H, W), 3, 1, (11.5, 9.5), ang, planned=bad)
        # "separable" reaches the new entries: their argument errors come back as the existing wrappers report them
        with pytest.raises(aai.AaiError) as info:
            aai.adjoint_interleaved_device(ok, 5, 8, 1 << 20, 8, 1 << 20, planned="separable")
        assert info.value.code == L.ERR_BAD_ARGUMENT and "Channels" in info.value.message
        with pytest.raises(aai.AaiError):
            aai.adjoint_interleaved_device(aai.make_request(W, H, 3, 1, (11.5, 9.5), ang, mode=L.MODE_BICUBIC), C, 8, 1 << 20, 8, 1 << 20, planned="separable")
        aai.adjoint_interleaved_device(ok, C, 8, 1 << 20, 8, 1 << 20, batch=0, planned="separable")       # batch 0: OK without a device
        rc, msg, out = aai.adjoint_interleaved_host(np.zeros((4, 4, 3), np.float32), (4, 4), (1, 2), 1, (0, 0), ang, planned="separable")
        assert rc == L.ERR_RESOLUTION_MISMATCH and out is None and msg == "Assumed X & Y resolution are same."
        rc, msg, out = aai.adjoint_interleaved_host(np.zeros((lay.dst_height, lay.dst_width, 5), np.float32), (H, W), 3, 1, (11.5, 9.5), ang, planned="separable")
        assert rc == L.ERR_BAD_ARGUMENT and out is None and "Channels" in msg
    assert api._planned_interleaved_kind("separable") == "separable" and api._planned_interleaved_kind("any") == "any"
    assert api._planned_interleaved_kind(False) == "general"
    # the single-channel wrappers still take no string but "any"
    with pytest.raises(ValueError):
        api._planned_kind("separable")
    with pytest.raises(ValueError):
        aai.adjoint_device(aai.make_request(W, H, 3, 1, (11.5, 9.5), 0.0), 8, 1 << 20, 8, 1 << 20, batch=0, planned="separable")
    from area_average_interpolation_amd import torch_ops
    assert torch_ops._normalise_planned("channels_last") == "channels_last" and torch_ops._normalise_planned("interleaved") == "interleaved"
    with pytest.raises(ValueError):
        torch_ops._normalise_planned("sums")
    with pytest.raises(ValueError):
        torch_ops._normalise_planned("separable")                   # the wrappers' word, not the operator's


def test_new_sources_have_no_inline_assembly_and_no_environment_reads():
    for f in (os.path.join(CSRC, "aai_axis_adjoint_multi.hip"), os.path.join(ROOT, "tests", "emulation", "axis_adjoint_multi_emulation.cpp")):
        text = open(f).read().lower()
        for w in ("asm", "getenv", "atomic", "__shared__"):
            assert w not in text.replace("no atomics", ""), (f, w)


def test_the_new_unit_is_built_and_reported():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(OBJ)/aai_axis_adjoint_multi.o" in mk and "aai_adjoint_planned_interleaved.h" in mk
    assert re.search(r"^REPORT_UNITS :=.*\baai_axis_adjoint_multi\b", mk, re.M)
    # contraction as in the single-channel unit (the fused multiply-adds are spelled out): not among the units compiled without it
    assert not re.search(r"^NOCONTRACT :=.*\baai_axis_adjoint_multi\b", mk, re.M)


@pytest.fixture(scope="module")
def axismultiemu(aai):
    """tests/emulation/axis_adjoint_multi_emulation.cpp compiled with g++, no contraction, like axis_adjoint_emulation.cpp:
    run(rq, gdst [dH, dW, C]) -> (status, gsrc [H, W, C], (flagged dst pixels, listed source pixels, listed dst pixels))"""
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_axisadjmultiemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", "axis_adjoint_multi_emulation.cpp")] + [os.path.join(CSRC, f) for f in
            ("aai_adjoint_math.hpp", "aai_axis_verify.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_axis_adjoint_multi.restype = ctypes.c_int
    lib.aai_emu_axis_adjoint_multi.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]

    def run(rq, gdst):
        gdst = np.ascontiguousarray(gdst, dtype=np.float32)
        out = np.full((rq.src_height, rq.src_width, gdst.shape[2]), -1.0, np.float32)
        counts = (ctypes.c_int * 3)()
        rc = lib.aai_emu_axis_adjoint_multi(ctypes.byref(rq), gdst.shape[2], gdst.ctypes.data, out.ctypes.data, counts)
        return rc, out, tuple(counts)
    return run


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


LISTED = {}          # (case, channels) -> mode / policy pairs whose replay ran the listed pass


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("case", range(len(MATRIX)))
def test_replay_channels_have_the_single_channel_replays_bits(aai, axismultiemu, axisemu, case, channels):
    assert len(MATRIX) == 12
    W, H, sr, dr, ang, off, absolute = MATRIX[case]
    iso = off if absolute else ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    listed = 0
    for mode, policy in ((aai.MODE_AREA, aai.POLICY_REFERENCE), (aai.MODE_AREA, aai.POLICY_EXACT), (aai.MODE_FAST, aai.POLICY_REFERENCE)):
        rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
        rc, msg, lay = aai.query(rq)
        assert rc == 0, msg
        what = "case %d mode %d policy %d C=%d" % (case, mode, policy, channels)
        # a different random gradient per channel: a mix-up of channels cannot pass
        g = np.stack([np.random.default_rng(11 + 17 * c).random((lay.dst_height, lay.dst_width)).astype(np.float32) for c in range(channels)], axis=2)
        rc, got, counts = axismultiemu(rq, g)
        assert rc == 0, (what, rc)
        nonzero = 0
        for c in range(channels):
            rc1, one, counts1 = axisemu(rq, g[:, :, c])
            assert rc1 == 0 and counts1 == counts, (what, c, counts1, counts)      # the same plan: ranges and lists know no channels
            assert np.array_equal(_bits(got[:, :, c]), _bits(one)), (what, "channel %d" % c, int((_bits(got[:, :, c]) != _bits(one)).sum()))
            nonzero += int((one != 0).sum())
        assert nonzero and not np.array_equal(got[:, :, 0], got[:, :, 1]), what
        assert (got >= 0).all(), what                                               # the -1 prefill is gone: every element written
        listed += counts[1] > 0 and counts[2] > 0
    LISTED[case, channels] = listed


@pytest.mark.parametrize("channels", CHANNELS)
def test_the_replayed_geometries_cover_the_listed_pass(channels):
    """(after the test above) at least three geometries whose replay ran the listed pass, at least one that never did"""
    mine = {case: n for (case, c), n in LISTED.items() if c == channels}
    assert len(mine) == len(MATRIX), "the replay test did not run for every geometry"
    assert sum(1 for n in mine.values() if n) >= 3 and sum(1 for n in mine.values() if not n) >= 1, mine


def test_replay_refuses_what_the_planned_path_does_not_serve(aai, axismultiemu):
    from area_average_interpolation_amd import _lib as L
    z = np.zeros((1, 1, 3), np.float32)
    assert axismultiemu(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5), z)[0] == -1                  # a general rotation
    for (W, H, sr, dr, ang) in ((3, 50, 2, 1, 0.0), (2, 30, 1, 1, 90.0), (900, 300, 300, 1, 0.0)):     # AAI_KERNEL_AXIS_WIDE
        rq = aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
        assert aai.query(rq)[2].kernel == L.KERNEL_AXIS_WIDE
        assert axismultiemu(rq, z)[0] == -1, (W, H)
