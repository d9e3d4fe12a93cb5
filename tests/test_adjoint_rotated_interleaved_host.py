"""The interleaved planned adjoint at general rotations (include/aai_adjoint_rotated_interleaved.h:
aai_adjoint_rotated_interleaved_device_f32 / aai_adjoint_rotated_interleaved_f32), checks that need no GPU: the ABI, argument errors call
by call against the existing interleaved entries, the python wrappers, and a serial CPU replay of the path
(tests/emulation/adjoint_plain_multi_emulation.cpp: S and K as the single-channel plan holds them, the source list, the element-wise
pass 1 per row element, adjoint_plain_gather_multi, the listed overwrite by adjoint_gather_multi) whose every channel must equal, BIT FOR
BIT, the single-channel plain replay (adjoint_plain_emulation.cpp) on that plane AND the general multi replay
(adjoint_multi_emulation.cpp) -- no tolerance anywhere in this file."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import BUILD, GOLDEN, ROOT
from test_adjoint_host import EIGHT
from test_adjoint_interleaved_host import multiemu                          # noqa: F401  (the general multi replay's fixture)
from test_adjoint_rotated_host import KNIFE_STRIDE, adjemu, plainemu         # noqa: F401  (the single-channel replays' fixtures)

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")
ENTRIES = ("aai_adjoint_rotated_interleaved_device_f32", "aai_adjoint_rotated_interleaved_f32")
GENERAL_EIGHT = [c for c in EIGHT if c[4] % 90 != 0]
CHANNELS = (2, 3, 4)


def test_header_declares_library_exports_and_lib_binds_the_entries(aai):
    from area_average_interpolation_amd import _lib as L
    from area_average_interpolation_amd import api
    header = open(os.path.join(ROOT, "include", "aai_adjoint_rotated_interleaved.h")).read()
    assert '#include "aai.h"' in header
    assert "aai_adjoint_rotated_prepare" in header                   # no prepare entry of its own: said where the entries are declared
    assert "aai_adjoint_rotated_interleaved" in open(os.path.join(ROOT, "include", "aai_adjoint_rotated.h")).read()      # ... and there
    lib = L.load()
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    rq, ly = ctypes.POINTER(L.Request), ctypes.POINTER(L.Layout)
    args = {ENTRIES[0]: [rq, i32, i32, p, i64, i64, p, i64, i64, p], ENTRIES[1]: [rq, i32, p, i64, p, i64, ly]}
    existing = dict(zip(ENTRIES, ("aai_adjoint_interleaved_device_f32", "aai_adjoint_interleaved_f32")))
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.ROTATED_INTERLEAVED_ADJOINT_SYMBOLS and name not in L.SYMBOLS
        assert L.ROTATED_INTERLEAVED_ADJOINT_SYMBOLS[name][0] is ctypes.c_int and list(L.ROTATED_INTERLEAVED_ADJOINT_SYMBOLS[name][1]) == args[name]
        # the argument list of the existing interleaved entry
        assert list(L.ROTATED_INTERLEAVED_ADJOINT_SYMBOLS[name][1]) == list(L.INTERLEAVED_ADJOINT_SYMBOLS[existing[name]][1]), name
    assert not re.search(r"\bint\s+aai_adjoint_rotated_interleaved_prepare\b", header)
    assert lib.aai_version() == 2                                    # additions in a header of their own: the version stays 0.2
    main = open(os.path.join(ROOT, "include", "aai.h")).read()
    for name in ENTRIES:
        assert name not in main
    # the python surface: the keyword exists, defaults to the existing behaviour
    for fn in (aai.adjoint_interleaved_device, aai.adjoint_interleaved_host):
        assert inspect.signature(fn).parameters["planned"].default is False
    assert api._planned_interleaved_kind(False) == "general" and api._planned_interleaved_kind("any") == "any"
    src = open(os.path.join(ROOT, "area_average_interpolation_amd", "torch_ops.py")).read()
    assert re.search(r"def resample\([^)]*planned_backward=False\)", src) and '"interleaved"' in src


def _calls(lib):
    """(existing entry, new entry) pairs with one signature: device, host"""
    def dev(fn):
        return lambda rq, channels=3, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20: fn(
            None if rq is None else ctypes.byref(rq), batch, channels, gdst, dst_stride, 0, gsrc, src_stride, 0, None)

    def host(fn):
        return lambda rq, channels=3, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20: fn(
            None if rq is None else ctypes.byref(rq), channels, gdst, dst_stride, gsrc, src_stride, None)
    return [(dev(lib.aai_adjoint_interleaved_device_f32), dev(lib.aai_adjoint_rotated_interleaved_device_f32)),
            (host(lib.aai_adjoint_interleaved_f32), host(lib.aai_adjoint_rotated_interleaved_f32))]


def test_new_entries_refuse_what_the_existing_interleaved_entries_refuse(aai):
    """dummy (never dereferenced) pointers: every call below returns before the device is touched, with the existing entry's code and
    message"""
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


def test_api_wrappers_take_false_or_any_and_nothing_else(aai):
    from area_average_interpolation_amd import _lib as L
    W, H, C = 24, 20, 3
    ok = aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5)
    lay = aai.query(ok)[2]
    g = np.zeros((lay.dst_height, lay.dst_width, C), np.float32)
    for bad in (True, "sums", "planned", 1, None):
        with pytest.raises(ValueError):
            aai.adjoint_interleaved_device(ok, C, 8, 1 << 20, 8, 1 << 20, planned=bad)
        with pytest.raises(ValueError):
            aai.adjoint_interleaved_host(g, (H, W), 3, 1, (11.5, 9.5), 17.5, planned=bad)
    # "any" reaches the new entries: their argument errors come back as the existing wrappers report them
    with pytest.raises(aai.AaiError) as info:
        aai.adjoint_interleaved_device(ok, 5, 8, 1 << 20, 8, 1 << 20, planned="any")
    assert info.value.code == L.ERR_BAD_ARGUMENT and "Channels" in info.value.message
    with pytest.raises(aai.AaiError):
        aai.adjoint_interleaved_device(aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BICUBIC), C, 8, 1 << 20, 8, 1 << 20, planned="any")
    aai.adjoint_interleaved_device(ok, C, 8, 1 << 20, 8, 1 << 20, batch=0, planned="any")       # batch 0: OK without a device
    rc, msg, out = aai.adjoint_interleaved_host(np.zeros((4, 4, 3), np.float32), (4, 4), (1, 2), 1, (0, 0), 17.5, planned="any")
    assert rc == L.ERR_RESOLUTION_MISMATCH and out is None and msg == "Assumed X & Y resolution are same."
    rc, msg, out = aai.adjoint_interleaved_host(np.zeros((lay.dst_height, lay.dst_width, 5), np.float32), (H, W), 3, 1, (11.5, 9.5), 17.5, planned="any")
    assert rc == L.ERR_BAD_ARGUMENT and out is None and "Channels" in msg
    from area_average_interpolation_amd import torch_ops
    assert torch_ops._normalise_planned("interleaved") == "interleaved" and torch_ops._normalise_planned("any") == "any"
    with pytest.raises(ValueError):
        torch_ops._normalise_planned("sums")


def test_new_sources_have_no_inline_assembly_and_no_environment_reads():
    for f in (os.path.join(CSRC, "aai_adjoint_plain_multi.hip"), os.path.join(CSRC, "aai_adjoint_plain.hpp"),
              os.path.join(ROOT, "tests", "emulation", "adjoint_plain_multi_emulation.cpp")):
        text = open(f).read().lower()
        for w in ("asm", "getenv"):
            assert w not in text, (f, w)


@pytest.fixture(scope="module")
def plainmultiemu(aai):
    """tests/emulation/adjoint_plain_multi_emulation.cpp compiled with g++, no contraction, like the other replays:
    run(rq, gdst [dH, dW, C]) -> (status, gsrc [H, W, C], (pixels of K, listed source pixels, 1 if the general adjoint served it))"""
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_adjplainmultiemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", "adjoint_plain_multi_emulation.cpp")] + [os.path.join(CSRC, f) for f in
            ("aai_adjoint_plain.hpp", "aai_adjoint_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_adjoint_plain_multi.restype = ctypes.c_int
    lib.aai_emu_adjoint_plain_multi.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint,
                                                ctypes.POINTER(ctypes.c_long)]

    def run(rq, gdst, max_listed=1 << 24):
        gdst = np.ascontiguousarray(gdst, dtype=np.float32)
        out = np.full((rq.src_height, rq.src_width, gdst.shape[2]), -1.0, np.float32)
        counts = (ctypes.c_long * 3)()
        rc = lib.aai_emu_adjoint_plain_multi(ctypes.byref(rq), gdst.shape[2], gdst.ctypes.data, out.ctypes.data, max_listed, counts)
        return rc, out, tuple(counts)
    return run


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(aai, emus, rq, channels, what):
    """the three replays on one gradient whose channels are drawn independently: every channel of the new replay equals the
    single-channel plain replay on that plane and the general multi replay; returns the plan's counts"""
    plainmultiemu, plainemu, multiemu = emus
    rc, msg, lay = aai.query(rq)
    assert rc == 0, msg
    g = np.stack([np.random.default_rng(7 + 13 * c).random((lay.dst_height, lay.dst_width)).astype(np.float32) for c in range(channels)], axis=2)
    rc, got, counts = plainmultiemu(rq, g)
    assert rc == 0, (what, rc)
    knife, listed, general = counts
    assert listed <= got.shape[0] * got.shape[1] // 2 and (knife > 0 or listed == 0), (what, counts)
    ref = multiemu(rq, g)
    assert np.array_equal(_bits(got), _bits(ref)), (what, "general multi replay", int((_bits(got) != _bits(ref)).sum()))
    nonzero = 0
    for c in range(channels):
        rc1, one, counts1 = plainemu(rq, g[:, :, c])
        assert rc1 == 0 and counts1[:3] == counts, (what, c, counts1, counts)         # the same plan: S, K and the list know no channels
        assert np.array_equal(_bits(got[:, :, c]), _bits(one)), (what, "single-channel plain replay, channel %d" % c)
        nonzero += int((one != 0).sum())
    if channels > 1 and nonzero:
        assert not np.array_equal(got[:, :, 0], got[:, :, 1]), what                  # independent channels: a mix-up cannot pass
    assert (got >= 0).all(), what                                                     # the -1 prefill is gone
    return counts


def _modes(aai):
    return (aai.MODE_AREA, aai.MODE_FAST)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("case", range(len(GENERAL_EIGHT)))
def test_replay_channels_have_both_replays_bits(aai, plainmultiemu, plainemu, multiemu, case, channels):
    assert [c[4] for c in GENERAL_EIGHT] == [17.5, 30, 45, 200.25, 117.5]
    W, H, sr, dr, ang, off = GENERAL_EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mode, policy in ((aai.MODE_AREA, aai.POLICY_REFERENCE), (aai.MODE_AREA, aai.POLICY_EXACT), (aai.MODE_FAST, aai.POLICY_REFERENCE)):
        rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
        _same_bits(aai, (plainmultiemu, plainemu, multiemu), rq, channels, "case %d mode %d policy %d C=%d" % (case, mode, policy, channels))


@pytest.mark.parametrize("channels", CHANNELS)
def test_replay_on_the_92_by_68_geometry(aai, plainmultiemu, plainemu, multiemu, channels):
    for mode in _modes(aai):
        rq = aai.make_request(92, 68, 3.0, 1.0, (45.5, 33.5), 17.5, mode=mode)
        counts = _same_bits(aai, (plainmultiemu, plainemu, multiemu), rq, channels, "92 x 68 mode %d C=%d" % (mode, channels))
        assert counts[2] == 0


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("ang", [17.5, 107.5, 197.5, 287.5])
def test_replay_of_replicated_sources_in_every_quadrant(aai, plainmultiemu, plainemu, multiemu, ang, channels):
    """x2 and x3 up-sampling (scale > 1): adjoint_virtual_pixel's four branches"""
    for (W, H, dr) in ((29, 23, 2), (19, 17, 3)):
        for mode in _modes(aai):
            rq = aai.make_request(W, H, 1, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            lay = aai.query(rq)[2]
            assert lay.scale > 1 and lay.quadrant == int(ang // 90)
            counts = _same_bits(aai, (plainmultiemu, plainemu, multiemu), rq, channels, "x%d at %g mode %d C=%d" % (dr, ang, mode, channels))
            assert counts[2] == 0


@pytest.mark.parametrize("channels", CHANNELS)
def test_replay_on_knife_edge_geometries(aai, plainmultiemu, plainemu, multiemu, knife_golden, channels):
    """the reference-generated knife fixtures at KNIFE_STRIDE, both modes: plans with a listed pass and plans without are among them,
    and that is asserted -- the test cannot pass with the listed pass unexercised"""
    manifest = knife_golden[1]
    listed = empty = general = ran = 0
    for i in range(0, len(manifest), KNIFE_STRIDE):             # a fixed stride by index, never a choice by outcome
        c = manifest[i]
        if c["W"] * c["H"] > 1300:
            continue
        ran += 1
        for mode in _modes(aai):
            rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode)
            knife, nsrc, gen = _same_bits(aai, (plainmultiemu, plainemu, multiemu), rq, channels, "knife %d mode %d C=%d" % (i, mode, channels))
            listed, empty, general = listed + (nsrc > 0 and not gen), empty + (nsrc == 0 and not gen), general + gen
    print("C=%d, %d geometries: %d plans with a non-empty source list, %d with an empty one, %d that keep the general adjoint" % (channels, ran, listed, empty, general))
    assert ran >= 20 and listed >= 3 and empty >= 1


def test_replay_refuses_a_reduced_angle_of_0(aai, plainmultiemu):
    """those geometries are the general interleaved adjoint's (the entry forwards them)"""
    assert plainmultiemu(aai.make_request(24, 24, 4, 1, (11.5, 11.5), 90.0), np.zeros((6, 6, 3), np.float32))[0] == -1
