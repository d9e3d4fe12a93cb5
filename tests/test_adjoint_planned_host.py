"""The planned adjoint (aai_adjoint_prepare / aai_adjoint_planned_batch_device_f32 / aai_adjoint_planned_f32), checks that need no
GPU: the ABI, argument errors in the order and with the texts of the existing adjoint entries, the python wrappers, and a serial CPU
replay of the planned path at rotations by multiples of 90 degrees (tests/emulation/axis_adjoint_emulation.cpp: the product's
tables, their inversion, the correction lists and the general adjoint's per-pixel bodies) against the oracle's matrix."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import BUILD, GOLDEN, ROOT
from test_adjoint_host import adjoint_gold, assert_adjoint_matches

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

# (W, H, srcRes, dstRes, angle, isocenter offset from the image centre): the geometries of tests/test_adjoint_planned_gpu.py, test 1
PLANNED_EIGHT = [(24, 24, 4, 1, 0, (0, 0)), (20, 16, 2, 1, 180, (0, 0)), (40, 30, 2.5, 1, 90, (0, 0)), (40, 30, 2.5, 1, 270, (0, 0)),
                 (21, 17, 3, 2, 0, (0.3, -0.2)), (20, 24, 1, 1, 90, (0, 0)), (16, 12, 1, 2, 0, (0, 0)), (16, 12, 1, 3, 270, (0, 0))]


def test_abi_declares_exports_and_binds_the_planned_adjoint(aai):
    from area_average_interpolation_amd import _lib as L
    base = open(os.path.join(ROOT, "include", "aai.h")).read()
    header = open(os.path.join(ROOT, "include", "aai_adjoint_planned.h")).read()        # the extension header that declares the three entries
    assert '#include "aai.h"' in header
    lib = L.load()
    rq, i32, i64, p, ly = ctypes.POINTER(L.Request), ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(L.Layout)
    protos = {"aai_adjoint_prepare": [rq],
              "aai_adjoint_planned_batch_device_f32": [rq, i32, p, i64, i64, p, i64, i64, p],
              "aai_adjoint_planned_f32": [rq, p, i64, p, i64, ly]}
    for name, args in protos.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.PLANNED_SYMBOLS and hasattr(lib, name)
        assert L.PLANNED_SYMBOLS[name][0] is ctypes.c_int and list(L.PLANNED_SYMBOLS[name][1]) == args, name
    # the header's version and the library's agree (the number itself is pinned by tests/test_adjoint_host.py)
    major = int(re.search(r"#define AAI_VERSION_MAJOR (\d+)", base).group(1))
    minor = int(re.search(r"#define AAI_VERSION_MINOR (\d+)", base).group(1))
    assert lib.aai_version() == major * 1000 + minor
    # the python surface
    assert "planned" in inspect.signature(aai.adjoint_device).parameters and "planned" in inspect.signature(aai.adjoint_host).parameters
    assert inspect.signature(aai.adjoint_device).parameters["planned"].default is False
    assert callable(aai.adjoint_prepare)
    src = open(os.path.join(ROOT, "area_average_interpolation_amd", "torch_ops.py")).read()
    assert re.search(r"def resample\([^)]*planned_backward=False\)", src)


def _calls(lib):
    """(existing entry, planned entry) pairs with one signature: device, host"""
    def dev(fn):
        return lambda rq, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20: fn(
            None if rq is None else ctypes.byref(rq), batch, gdst, dst_stride, 0, gsrc, src_stride, 0, None)

    def host(fn):
        return lambda rq, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20: fn(
            None if rq is None else ctypes.byref(rq), gdst, dst_stride, gsrc, src_stride, None)
    return [(dev(lib.aai_adjoint_batch_device_f32), dev(lib.aai_adjoint_planned_batch_device_f32)),
            (host(lib.aai_adjoint_f32), host(lib.aai_adjoint_planned_f32))]


def test_planned_entries_refuse_what_the_existing_entries_refuse(aai):
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
        assert lib.aai_adjoint_prepare(ctypes.byref(rq)) == rc and aai.last_error() == msg, p
    assert rejected >= 4
    # an axis-aligned and a rotated request: validation does not depend on which path would serve them
    for ang in (0.0, 17.5):
        mk = lambda **k: aai.make_request(24, 20, 3, 1, (11.5, 9.5), ang, **k)
        ok = mk()
        lay = aai.query(ok)[2]
        for pair in _calls(lib):
            for mode, name in ((L.MODE_BILINEAR, "BILINEAR"), (L.MODE_BICUBIC, "BICUBIC")):
                rc, msg = same(pair, mk(mode=mode))
                assert rc == L.ERR_BAD_ARGUMENT and name in msg
            rc, msg = same(pair, mk(policy=L.POLICY_DIAG_NO_FIXUP))
            assert rc == L.ERR_BAD_ARGUMENT and "DIAG_NO_FIXUP" in msg
            assert same(pair, mk(policy=0x800))[0] == L.ERR_BAD_ARGUMENT
            rc, msg = same(pair, ok, src_stride=23)
            assert rc == L.ERR_BAD_ARGUMENT and "Source stride" in msg
            rc, msg = same(pair, ok, dst_stride=lay.dst_width - 1)
            assert rc == L.ERR_BAD_ARGUMENT and "Destination stride" in msg
            assert same(pair, ok, gdst=None)[0] == L.ERR_BAD_ARGUMENT and same(pair, ok, gsrc=None)[0] == L.ERR_BAD_ARGUMENT
            assert same(pair, None)[0] == L.ERR_BAD_ARGUMENT
            # two faults: the earlier check speaks (mode before pointers, request before batch)
            assert "BICUBIC" in same(pair, mk(mode=L.MODE_BICUBIC), gdst=None)[1]
        device = _calls(lib)[0]
        rc, msg = same(device, ok, batch=-1)
        assert rc == L.ERR_BAD_ARGUMENT and "batch" in msg
        assert same(device, mk(policy=0x800), batch=-1)[1] == "Unknown weight policy."
        assert same(device, ok, batch=0)[0] == L.OK                      # returns before the device
        hints = mk(policy=L.POLICY_DOUBLE_PRECISION | L.POLICY_PREFER_CELL | L.POLICY_EXACT)
        assert same(device, hints, batch=0)[0] == L.OK
        # aai_adjoint_prepare: the request's checks
        for bad, word in ((mk(mode=L.MODE_BILINEAR), "BILINEAR"), (mk(policy=L.POLICY_DIAG_NO_FIXUP), "DIAG_NO_FIXUP"), (mk(policy=0x800), "policy")):
            assert lib.aai_adjoint_prepare(ctypes.byref(bad)) == L.ERR_BAD_ARGUMENT and word in aai.last_error()
        assert lib.aai_adjoint_prepare(None) == L.ERR_BAD_ARGUMENT
    # api wrappers raise / report the same
    with pytest.raises(aai.AaiError):
        aai.adjoint_device(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 0.0, mode=L.MODE_BICUBIC), 8, 8, 8, 24, planned=True)
    with pytest.raises(aai.AaiError):
        aai.adjoint_prepare(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 0.0, mode=L.MODE_BICUBIC))
    rc, msg, g = aai.adjoint_host(np.zeros((4, 4), np.float32), (4, 4), (1, 2), 1, (0, 0), 0, planned=True)
    assert rc == L.ERR_RESOLUTION_MISMATCH and g is None and msg == "Assumed X & Y resolution are same."


def test_new_sources_keep_the_shared_machine_word_rules():
    """no inline assembly and no environment reads in the new kernel file and the replay (the instruction-name rules are those of
    tests/test_adjoint_host.py, which lists the files it covers)"""
    for f in (os.path.join(CSRC, "aai_axis_adjoint.hip"), os.path.join(ROOT, "tests", "emulation", "axis_adjoint_emulation.cpp")):
        text = open(f).read().lower()
        for w in ("asm", "getenv"):
            assert w not in text, (f, w)


@pytest.fixture(scope="module")
def axisemu(aai):
    """tests/emulation/axis_adjoint_emulation.cpp compiled with g++, no contraction"""
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_axisadjemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", "axis_adjoint_emulation.cpp")] + [os.path.join(CSRC, f) for f in
            ("aai_adjoint_math.hpp", "aai_axis_verify.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_axis_adjoint.restype = ctypes.c_int
    lib.aai_emu_axis_adjoint.argtypes = [ctypes.POINTER(L.Request), ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]

    def run(rq, gdst):
        gdst = np.ascontiguousarray(gdst, dtype=np.float32)
        out = np.full((rq.src_height, rq.src_width), -1.0, np.float32)
        counts = (ctypes.c_int * 3)()
        rc = lib.aai_emu_axis_adjoint(ctypes.byref(rq), gdst.ctypes.data, out.ctypes.data, counts)
        return rc, out, tuple(counts)
    return run


@pytest.mark.parametrize("case", range(len(PLANNED_EIGHT)))
def test_cpu_replay_of_the_planned_path_matches_the_oracle_matrix(aai, po, axisemu, case):
    W, H, sr, dr, ang, off = PLANNED_EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mode, policy in ((aai.MODE_AREA, aai.POLICY_REFERENCE), (aai.MODE_AREA, aai.POLICY_EXACT), (aai.MODE_FAST, aai.POLICY_REFERENCE)):
        g, gold = adjoint_gold(po, aai, W, H, sr, dr, iso, ang, mode, policy)
        rc, got, counts = axisemu(aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy), g)
        assert rc == 0, (case, mode, policy, rc)
        print("case %d mode %d policy %d: flagged %d, listed source pixels %d, listed dst pixels %d" % ((case, mode, policy) + counts))
        assert_adjoint_matches(got, gold, "planned replay case %d mode %d policy %d" % (case, mode, policy))


def test_cpu_replay_refuses_what_the_planned_path_does_not_serve(aai, axisemu):
    rc, _, _ = axisemu(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5), np.zeros((1, 1), np.float32))
    assert rc == -1
