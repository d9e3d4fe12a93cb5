"""The adjoint of the bilinear / bicubic samplers (include/aai_adjoint_sample.h), checks that need no GPU: ABI, argument errors before
any device call, and a serial CPU replay of the kernel's per-pixel body (tests/emulation/adjoint_sample_emulation.cpp over
csrc/aai_adjoint_sample_math.hpp) against the oracle's matrix (oracle modes 3 / 4 on unit impulses), against columns of it taken from
comb images at mid sizes, and against a brute-force loop over all dst pixels for the superset property of the candidate walk."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import BUILD, GOLDEN, ROOT
from adjoint_sample_cases import (COMB_CASES, MATRIX_CASES, MODE_NAME, MODES, assert_sample_adjoint_matches, comb_gold, matrix_gold)

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

# new entry -> the general-adjoint entry whose argument list it takes
COUNTERPART = {"aai_adjoint_sample_batch_device_f32": "aai_adjoint_batch_device_f32", "aai_adjoint_sample_f32": "aai_adjoint_f32",
               "aai_adjoint_sample_interleaved_device_f32": "aai_adjoint_interleaved_device_f32",
               "aai_adjoint_sample_interleaved_f32": "aai_adjoint_interleaved_f32"}


def test_abi_declares_exports_and_binds_the_sampler_adjoint(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aai_adjoint_sample.h")).read()
    main = open(os.path.join(ROOT, "include", "aai.h")).read()
    lib = L.load()
    assert set(L.SAMPLE_ADJOINT_SYMBOLS) == set(COUNTERPART)
    known = dict(L.SYMBOLS)
    known.update(L.INTERLEAVED_ADJOINT_SYMBOLS)
    for name, other in COUNTERPART.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert not re.search(r"\b%s\b" % name, main), name
        assert hasattr(lib, name) and name not in L.SYMBOLS
        res, args = L.SAMPLE_ADJOINT_SYMBOLS[name]
        assert (res, args) == known[other], name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert lib.aai_version() == 2 and "#define AAI_VERSION_MINOR 2" in main
    for name in ("adjoint_sample_device", "adjoint_sample_host", "adjoint_sample_interleaved_device", "adjoint_sample_interleaved_host"):
        assert callable(getattr(aai, name)) and name in aai.__all__


def _calls(lib):
    """the four entries as f(rq, batch=, channels=, gdst=, dst_stride=, gsrc=, src_stride=) on dummy, never dereferenced pointers"""
    ref = lambda rq: None if rq is None else ctypes.byref(rq)

    def device(rq, batch=1, channels=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
        return lib.aai_adjoint_sample_batch_device_f32(ref(rq), batch, gdst, dst_stride, 0, gsrc, src_stride, 0, None)

    def host(rq, batch=1, channels=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
        return lib.aai_adjoint_sample_f32(ref(rq), gdst, dst_stride, gsrc, src_stride, None)

    def device_il(rq, batch=1, channels=3, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
        return lib.aai_adjoint_sample_interleaved_device_f32(ref(rq), batch, channels, gdst, dst_stride, 0, gsrc, src_stride, 0, None)

    def host_il(rq, batch=1, channels=3, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
        return lib.aai_adjoint_sample_interleaved_f32(ref(rq), channels, gdst, dst_stride, gsrc, src_stride, None)
    return device, host, device_il, host_il


def test_argument_errors_come_before_any_device_call(aai):
    """dummy (never dereferenced) pointers: every call below must return before the device is touched"""
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    device, host, device_il, host_il = calls = _calls(lib)
    probes = json.load(open(os.path.join(GOLDEN, "error_paths.json")))
    rejected = 0
    for p in probes:
        for mode in MODES:
            if p["kind"] == "args":
                rq = aai.make_request(4, 4, p["src_res"], p["dst_res"], (0, 0), 0, mode=mode)
            else:
                rq = aai.make_request(0 if p["rows"] else 4, p["rows"], 1, 1, (0, 0), 0, mode=mode)
            rc, msg, _ = aai.query(rq)
            if rc == L.OK:
                continue
            rejected += 1
            for call in calls:
                assert call(rq) == rc and aai.last_error() == msg, (p, call.__name__)
    assert rejected >= 8
    for mode in MODES:
        ok = aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=mode)
        rc, _, lay = aai.query(ok)
        assert rc == L.OK
        for call in calls:
            C = 3 if call in (device_il, host_il) else 1
            # area / fast: the general adjoint's job, and the message says which entry that is
            for other in (L.MODE_AREA, L.MODE_FAST):
                assert call(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=other)) == L.ERR_BAD_ARGUMENT
                assert "aai_adjoint_batch_device_f32" in aai.last_error()
            assert call(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=mode, policy=0x800)) == L.ERR_BAD_ARGUMENT      # unknown policy bit
            assert aai.last_error() == "Unknown weight policy."
            assert call(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=mode, policy=2)) == L.ERR_BAD_ARGUMENT          # unknown rule
            assert call(ok, src_stride=24 * C - 1) == L.ERR_BAD_ARGUMENT and "Source stride" in aai.last_error()
            assert call(ok, dst_stride=lay.dst_width * C - 1) == L.ERR_BAD_ARGUMENT and "Destination stride" in aai.last_error()
            assert call(ok, gdst=None) == L.ERR_BAD_ARGUMENT and "Null image pointer" in aai.last_error()
            assert call(ok, gsrc=None) == L.ERR_BAD_ARGUMENT and "Null image pointer" in aai.last_error()
            assert call(None) == L.ERR_BAD_ARGUMENT
        for call in (device_il, host_il):
            for C in (0, 5):
                assert call(ok, channels=C) == L.ERR_BAD_ARGUMENT and aai.last_error() == "Channels must be 1..4."
        for call in (device, device_il):
            assert call(ok, batch=-1) == L.ERR_BAD_ARGUMENT and "batch" in aai.last_error()
            assert call(ok, batch=0) == L.OK
            # the policy's bits are validated like aai_query validates them and otherwise ignored: with batch 0 the call returns before the device
            hints = L.POLICY_DOUBLE_PRECISION | L.POLICY_PREFER_CELL | L.POLICY_DIAG_NO_FIXUP | L.POLICY_EXACT
            assert call(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=mode, policy=hints), batch=0) == L.OK
    # the existing entries keep refusing the samplers
    rq = aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BILINEAR)
    assert lib.aai_adjoint_batch_device_f32(ctypes.byref(rq), 1, 8, 1 << 20, 0, 8, 1 << 20, 0, None) == L.ERR_BAD_ARGUMENT
    assert aai.last_error() == "No adjoint for AAI_MODE_BILINEAR: the area and fast modes only."
    # api wrappers raise / report the same
    with pytest.raises(aai.AaiError):
        aai.adjoint_sample_device(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_AREA), 8, 8, 8, 24)
    with pytest.raises(aai.AaiError):
        aai.adjoint_sample_interleaved_device(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BICUBIC), 5, 8, 8, 8, 24)
    rc, msg, g = aai.adjoint_sample_host(np.zeros((4, 4), np.float32), (4, 4), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and g is None and msg == "Assumed X & Y resolution are same."
    with pytest.raises(ValueError):
        aai.adjoint_device(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BILINEAR), 8, 8, 8, 24, planned="sample")      # planned= is not overloaded


@pytest.fixture(scope="module")
def sampleemu(aai):
    """tests/emulation/adjoint_sample_emulation.cpp compiled with g++, no contraction: the kernel's body, one source pixel after the other"""
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_adjsampleemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", "adjoint_sample_emulation.cpp")] + [os.path.join(CSRC, f) for f in
            ("aai_adjoint_sample_math.hpp", "aai_sample_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    RQ = ctypes.POINTER(L.Request)
    LL = ctypes.POINTER(ctypes.c_longlong)
    lib.aai_emu_adjoint_sample.restype = ctypes.c_int
    lib.aai_emu_adjoint_sample.argtypes = [RQ, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, LL, LL]
    lib.aai_emu_adjoint_sample_superset.restype = ctypes.c_int
    lib.aai_emu_adjoint_sample_superset.argtypes = [RQ, LL, LL]
    lib.aai_emu_adjoint_sample_matrix.restype = ctypes.c_int
    lib.aai_emu_adjoint_sample_matrix.argtypes = [RQ, ctypes.c_void_p]

    class Emu:
        @staticmethod
        def run(rq, gdst):
            """(gsrc with gdst's channel layout, candidates visited)"""
            gdst = np.ascontiguousarray(gdst, dtype=np.float32)
            C = gdst.shape[2] if gdst.ndim == 3 else 1
            out = np.full((rq.src_height, rq.src_width) + gdst.shape[2:], -1.0, np.float32)
            n = ctypes.c_longlong(0)
            assert lib.aai_emu_adjoint_sample(ctypes.byref(rq), C, gdst.ctypes.data, out.ctypes.data, ctypes.byref(n), None) == 0
            return out, n.value

        @staticmethod
        def superset(rq):
            """(pairs with weight that the walk misses, pairs with weight)"""
            missed, pairs = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
            assert lib.aai_emu_adjoint_sample_superset(ctypes.byref(rq), ctypes.byref(missed), ctypes.byref(pairs)) == 0
            return missed.value, pairs.value

        @staticmethod
        def matrix(rq, rows):
            M = np.zeros((rows, rq.src_width * rq.src_height))
            assert lib.aai_emu_adjoint_sample_matrix(ctypes.byref(rq), M.ctypes.data) == 0
            return M
    return Emu


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAME[m] for m in MODES])
@pytest.mark.parametrize("case", range(len(MATRIX_CASES)))
def test_cpu_replay_matches_the_oracle_matrix(aai, po, sampleemu, case, mode):
    rq, g, gold, M = matrix_gold(po, aai, case, mode)
    got, visited = sampleemu.run(rq, g)
    assert_sample_adjoint_matches(got, gold, "replay case %d %s" % (case, MODE_NAME[mode]))
    # the rules of the header reproduce the oracle's matrix entry by entry (sums of at most 16 weights of magnitude <= 1)
    Mr = sampleemu.matrix(rq, M.shape[0])
    print("matrix: max |replay - oracle| %.3e" % float(np.abs(Mr - M).max()))
    assert float(np.abs(Mr - M).max()) <= 1e-14
    # the candidate walk is a superset of the pairs that carry weight
    missed, pairs = sampleemu.superset(rq)
    print("candidates visited %d, pairs with weight %d (%.2f x)" % (visited, pairs, visited / max(pairs, 1)))
    assert missed == 0 and pairs > 0 and visited >= pairs


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAME[m] for m in MODES])
def test_cpu_replay_interleaved_channels_get_the_single_channel_bits(aai, po, sampleemu, mode):
    rq, g, gold, _ = matrix_gold(po, aai, 0, mode)
    planes = [g, (g * np.float32(-0.5)).astype(np.float32), np.roll(g, 3, axis=1), np.flipud(g)]
    for C in (2, 3, 4):
        got, _ = sampleemu.run(rq, np.stack(planes[:C], axis=2))
        for c in range(C):
            assert np.array_equal(got[:, :, c], sampleemu.run(rq, planes[c])[0]), (C, c)


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAME[m] for m in MODES])
@pytest.mark.parametrize("case", range(len(COMB_CASES)))
def test_cpu_replay_matches_comb_gold(aai, po, sampleemu, case, mode):
    """per-pixel gold at sizes the matrix cannot reach: columns of the oracle's matrix from comb images of pitch 7"""
    rq, g, sx, sy, gold = comb_gold(po, aai, case, mode)
    got, visited = sampleemu.run(rq, g)
    print("candidates visited per source pixel: %.2f" % (visited / (rq.src_width * rq.src_height)))
    assert_sample_adjoint_matches(got[sy, sx], gold, "replay comb %r %s (%d source pixels)" % (COMB_CASES[case], MODE_NAME[mode], sx.size))


def test_clean_tree_cross_compiles_for_gfx950(tmp_path):
    """the library builds from nothing but its sources (another output and object directory; the tree's own build is untouched)"""
    out = tmp_path / "libaai_hip.so"
    r = subprocess.run(["make", "-j8", "-C", CSRC, "OUT=%s" % out, "OBJ=%s" % (tmp_path / "build_adjoint_sample")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(out))
    for name in COUNTERPART:
        assert hasattr(lib, name), name
    nm = subprocess.run(["strings", str(out)], capture_output=True, text=True).stdout
    assert "aai_adjoint_sample_kernel" in nm
