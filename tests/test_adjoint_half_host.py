"""The half-precision adjoint (include/aai_adjoint_half.h: aai_adjoint_half_device / aai_adjoint_half_host), checks that need no GPU: the
ABI, argument errors probe by probe against the fp32 entries whose validation the header promises
(aai_adjoint_planned_interleaved_device_f32 / _f32, answering live in the same process), the python surface, and a serial CPU replay of
the direct kernel (tests/emulation/adjoint_half_emulation.cpp over csrc/aai_axis_adjoint_half_math.hpp, the function the kernel calls)
that must equal, BIT FOR BIT, narrow(fp32 replay(widen(g))) with the fp32 replay of tests/emulation/axis_adjoint_emulation.cpp."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import adjoint_half_cases as ac
import half_cases as hc
import test_entry_point_errors as E
from conftest import ROOT
from test_adjoint_host import oracle_matrix
from test_adjoint_planned_host import PLANNED_EIGHT, axisemu                 # noqa: F401  (the fp32 replay's fixture)

CSRC = ac.CSRC
NEW = ("aai_adjoint_half_device", "aai_adjoint_half_host")
REF = ("aai_adjoint_planned_interleaved_device_f32", "aai_adjoint_planned_interleaved_f32")
HALF_MESSAGE = "Unknown half-precision element type."


def test_header_declares_library_exports_and_lib_binds_the_entries(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aai_adjoint_half.h")).read()
    assert '#include "aai_half.h"' in header
    lib = L.load()
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    rq, ly = ctypes.POINTER(L.Request), ctypes.POINTER(L.Layout)
    args = {NEW[0]: [rq, i32, i32, i32, p, i64, i64, p, i64, i64, p], NEW[1]: [rq, i32, i32, p, i64, p, i64, ly]}
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.ADJOINT_HALF_SYMBOLS and name not in L.SYMBOLS
        assert L.ADJOINT_HALF_SYMBOLS[name][0] is ctypes.c_int and list(L.ADJOINT_HALF_SYMBOLS[name][1]) == args[name]
    assert len(L.ADJOINT_HALF_SYMBOLS) == 2
    assert lib.aai_version() == 2                                    # additions in a header of their own: the version stays 0.2
    main = open(os.path.join(ROOT, "include", "aai.h")).read()
    assert "#define AAI_VERSION_MINOR 2" in main
    for name in NEW:
        assert name not in main
    # the headers that listed "a half adjoint in the C ABI" under NOT PROVIDED keep their text
    for h in ("aai_half.h", "aai_half_interleaved.h"):
        assert "a half adjoint in the C ABI" in re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", h)).read()), h
    for word in ("VALUES", "VALIDATION", "PLAN", "direct", "forwarding", "NOT PROVIDED", "aai_adjoint_rotated_prepare", "NOT TESTED"):
        assert word in header, word
    # the python surface
    import area_average_interpolation_amd as pkg
    assert "adjoint_half_device" in pkg.__all__ and "adjoint_half_host" in pkg.__all__
    assert list(inspect.signature(aai.adjoint_half_device).parameters) == ["request", "channels", "gdst_ptr", "dst_stride", "gsrc_ptr", "src_stride",
                                                                           "half_dtype", "stream", "batch", "dst_image_stride", "src_image_stride"]
    assert list(inspect.signature(aai.adjoint_half_host).parameters) == ["gdst_bits", "src_shape", "src_resolution", "dst_resolution", "src_isocenter",
                                                                         "rotation_angle", "mode", "policy", "half_dtype"]
    src = open(os.path.join(ROOT, "area_average_interpolation_amd", "torch_ops.py")).read()
    m = re.search(r"def resample\(([^)]*)\)", src)
    assert m and "half_backward=False" in m.group(1).split("*positional,")[1]          # keyword-only, off by default


# ---- argument errors: the faults of tests/test_entry_point_errors.py, singly and in pairs, against the fp32 entries' live answers --------
_DEV = [("req", 1), ("batch", 2), ("channels", 3), ("dst", E.FAKE_DST), ("dst_stride", E.BIG), ("dst_image_stride", E.BIG * E.BIG),
        ("src", E.FAKE_SRC), ("src_stride", E.BIG), ("src_image_stride", E.BIG * E.BIG), ("stream", None)]
_HOST = [("req", 1), ("channels", 3), ("dst", E.FAKE_DST), ("dst_stride", E.BIG), ("src", E.FAKE_SRC), ("src_stride", E.BIG), ("layout", None)]
# checks that speak before the element type: the request's own (check_request) and the channel count
BEFORE_HALF = {"null_request", "bad_mode", "bad_policy", "channels_zero", "channels_five"}


def _probes(arglist):
    """E.probes for an argument list that is not in E.ENTRIES: (), every single fault, every pair that replaces different things"""
    names = [n for n, _ in arglist]
    singles = [f for f in E.FAULTS if all((k.startswith("rq.") and "req" in names) or k in names for k in E.FAULTS[f])]
    out = [()] + [(f,) for f in singles]
    for a, b in itertools.combinations(singles, 2):
        ka, kb = set(E.FAULTS[a]), set(E.FAULTS[b])
        if ka & kb:
            continue
        if ("req" in ka and any(k.startswith("rq.") for k in kb)) or ("req" in kb and any(k.startswith("rq.") for k in ka)):
            continue
        out.append((a, b))
    return out


def _call(lib, L, entry, arglist, faults, half_dtype=None):
    """-> (return code, aai_last_error()) of one probe; half_dtype: the new entries' extra argument, directly behind the channels"""
    fields, args = dict(E.BASE), dict(arglist)
    for f in faults:
        for k, v in E.FAULTS[f].items():
            if k.startswith("rq."):
                fields[k[3:]] = v
            else:
                args[k] = v
    rq = L.Request(**fields)
    args["req"] = ctypes.byref(rq) if args["req"] else None
    lay = L.Layout()
    assert lib.aai_query(ctypes.byref(L.Request(**E.BASE)), ctypes.byref(lay)) == L.OK and lib.aai_last_error() == b""
    values = []
    for n, _ in arglist:
        values.append(args[n])
        if n == "channels" and half_dtype is not None:
            values.append(half_dtype)
    rc = getattr(lib, entry)(*values)
    return rc, lib.aai_last_error().decode()


@pytest.mark.parametrize("which", (0, 1), ids=("device", "host"))
def test_entries_answer_every_fault_and_pair_like_the_fp32_entries(aai, which):
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    arglist = (_DEV, _HOST)[which]
    have_gpu = aai.device_count() > 0
    probes = _probes(arglist)
    assert len(probes) > 100 and any(len(p) == 2 for p in probes)
    wrong, seen = [], set()
    for p in probes:
        reaches_device = not (set(p) - {"zero_batch"}) and not (which == 0 and "zero_batch" in p)
        if have_gpu and reaches_device:
            continue      # with a device this call would go on to compute, on pointers that point nowhere
        want = _call(lib, L, REF[which], arglist, p)
        for ht in (hc.F16, hc.BF16):
            got = _call(lib, L, NEW[which], arglist, p, half_dtype=ht)
            if got != want:
                wrong.append((p, ht, got, want))
        if reaches_device:
            assert want[0] == L.ERR_NO_DEVICE, (p, want)
        elif "zero_batch" in p and len(p) == 1:
            assert want == (L.OK, ""), want                           # an empty batch: AAI_OK before the device is touched
        else:
            assert want[0] not in (L.OK, L.ERR_NO_DEVICE), (p, want)  # everything is refused before the device check
        seen.add(want[1])
        # the bad element type on top: checked behind `channels` and before everything else -- the batch, the geometry, the mode, the pointers
        for bad in (0, 3, 7, -1):
            got = _call(lib, L, NEW[which], arglist, p, half_dtype=bad)
            expect = want if set(p) & BEFORE_HALF else (L.ERR_BAD_ARGUMENT, HALF_MESSAGE)
            if got != expect:
                wrong.append((p, bad, got, expect))
    assert not wrong, wrong[:10]
    assert len(seen) >= 12, seen                                       # the probes reach the checks, not one early exit


def test_api_wrappers_report_what_the_entries_report(aai):
    from area_average_interpolation_amd import _lib as L
    W, H, C = 24, 20, 3
    for ang in (0.0, 17.5):
        ok = aai.make_request(W, H, 3, 1, (11.5, 9.5), ang)
        lay = aai.query(ok)[2]
        with pytest.raises(aai.AaiError) as info:
            aai.adjoint_half_device(ok, 5, 8, 1 << 20, 8, 1 << 20, hc.F16)
        assert info.value.code == L.ERR_BAD_ARGUMENT and "Channels" in info.value.message
        with pytest.raises(aai.AaiError) as info:
            aai.adjoint_half_device(ok, C, 8, 1 << 20, 8, 1 << 20, 9)
        assert info.value.message == HALF_MESSAGE
        with pytest.raises(aai.AaiError):
            aai.adjoint_half_device(aai.make_request(W, H, 3, 1, (11.5, 9.5), ang, mode=L.MODE_BICUBIC), C, 8, 1 << 20, 8, 1 << 20, hc.BF16)
        aai.adjoint_half_device(ok, C, 8, 1 << 20, 8, 1 << 20, hc.BF16, batch=0)        # batch 0: OK without a device
        g = np.zeros((lay.dst_height, lay.dst_width, C), np.uint16)
        with pytest.raises(ValueError):
            aai.adjoint_half_host(g, (H, W), 3, 1, (11.5, 9.5), ang)                     # uint16 bits do not name their type
        with pytest.raises(TypeError):
            aai.adjoint_half_host(g.astype(np.float32), (H, W), 3, 1, (11.5, 9.5), ang, half_dtype=hc.F16)
        with pytest.raises(ValueError):
            aai.adjoint_half_host(g[1:], (H, W), 3, 1, (11.5, 9.5), ang, half_dtype=hc.F16)
        rc, msg, out = aai.adjoint_half_host(np.zeros((4, 4, 3), np.uint16), (4, 4), (1, 2), 1, (0, 0), ang, half_dtype=hc.F16)
        assert rc == L.ERR_RESOLUTION_MISMATCH and out is None and msg == "Assumed X & Y resolution are same."
        rc, msg, out = aai.adjoint_half_host(np.zeros((lay.dst_height, lay.dst_width, 5), np.uint16), (H, W), 3, 1, (11.5, 9.5), ang, half_dtype=hc.BF16)
        assert rc == L.ERR_BAD_ARGUMENT and out is None and "Channels" in msg


def test_torch_operator_refuses_half_backward_without_its_conditions():
    torch = pytest.importorskip("torch")
    from area_average_interpolation_amd import _lib as L
    from area_average_interpolation_amd import torch_ops
    x = torch.zeros((8, 8), dtype=torch.float16)
    geo = (2, 1, (3.5, 3.5), 0.0)
    for kwargs, word in ((dict(half_backward=True), "half=True"), (dict(half=True, half_backward=True, planned_backward="any"), "planned_backward"),
                         (dict(half=True, half_backward=True, planned_backward=True), "planned_backward"),
                         (dict(half="channels_last", half_backward=True, mode=L.MODE_BILINEAR), "area and fast"),
                         (dict(half=True, half_backward=True, mode=L.MODE_BICUBIC, sampler_backward=True), "area and fast"),
                         (dict(integer=True, half_backward=True), "half=True")):
        with pytest.raises(ValueError) as info:
            torch_ops.resample(x, *geo, **kwargs)
        assert word in str(info.value), (kwargs, str(info.value))
    with pytest.raises(TypeError):
        torch_ops.resample(x.float(), *geo, half=True, half_backward=True)               # a float32 tensor is not the half operator's


def test_new_sources_keep_the_shared_machine_word_rules():
    for f in (os.path.join(CSRC, "aai_axis_adjoint_narrow.hip"), os.path.join(CSRC, "aai_axis_adjoint_half_math.hpp"),
              os.path.join(ROOT, "tests", "emulation", "adjoint_half_emulation.cpp")):
        text = open(f).read().lower()
        for w in ("asm", "getenv", "atomic", "__shared__"):
            assert w not in text.replace("no atomics", ""), (f, w)


def test_the_new_unit_is_built_without_contraction_and_reported():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(OBJ)/aai_axis_adjoint_narrow.o" in mk and "aai_adjoint_half.h" in mk and "aai_axis_adjoint_half_math.hpp" in mk
    assert re.search(r"^REPORT_UNITS :=.*\baai_axis_adjoint_narrow\b", mk, re.M)
    assert re.search(r"^NOCONTRACT :=.*\baai_axis_adjoint_narrow\b", mk, re.M)           # compiled the way aai_axis_narrow is
    # the fp32 twins are untouched by name: still built, still outside NOCONTRACT
    assert not re.search(r"^NOCONTRACT :=.*\baai_axis_adjoint(_multi)?\b(?!_)", mk, re.M)


# ---- the replay ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_both_routes_and_every_transposed_quadrant(aai):
    direct = [(k, m) for k in ac.KEYS for m in ac.MODES if ac.is_direct(ac.request(aai, k, m))]
    forward = [(k, m) for k in ac.KEYS for m in ac.MODES if not ac.is_direct(ac.request(aai, k, m))]
    print("direct:", [ac.key_id(k) + "/" + m for k, m in direct])
    print("forwarding:", [ac.key_id(k) + "/" + m for k, m in forward])
    # every case reaches the direct kernel in some mode at its own angle and in a transposed quadrant
    for case in ac.CASES:
        for extra in ac.EXTRA_ANGLES:
            assert any(k == (case, extra) for k, _ in direct), (case, extra)
    assert forward, "no case with correction lists: the forwarding list of the GPU test would be empty"
    assert ac.facts(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5))[0] == -1          # a general rotation is never the direct kernel's


@pytest.mark.parametrize("key", ac.KEYS, ids=ac.key_id)
def test_replay_has_the_bits_of_the_narrowed_fp32_replay(aai, axisemu, key):
    """every case x quadrant x type, C = 1 and 3, both modes where the direct route serves them: narrow(fp32 replay(widen(g))) per plane"""
    ran = 0
    for mode in ac.MODES:
        rq = ac.request(aai, key, mode)
        if not ac.is_direct(rq):
            continue
        lay = aai.query(rq)[2]
        for ht, tname in ac.TYPES:
            for C in (1, 3):
                for nonfinite in ((False, True) if C == 3 else (False,)):
                    g = ac.gradient_bits(lay, C, ht, nonfinite=nonfinite)
                    got = ac.replay(rq, ht, g)
                    what = "%s %s %s C=%d nonfinite=%d" % (ac.key_id(key), mode, tname, C, nonfinite)
                    for c in range(C):
                        rc, ref32, counts = axisemu(rq, ac.widen(g[:, :, c], ht))
                        assert rc == 0 and not (counts[1] and counts[2]), (what, rc, counts)
                        want = ac.narrow(ref32, ht)
                        assert np.array_equal(got[:, :, c], want), (what, "channel %d" % c, int((got[:, :, c] != want).sum()))
                    if nonfinite:
                        v = ac.widen(got, ht)
                        assert np.isnan(v[:, :, 0]).any() and not np.isnan(v[:, :, C - 1]).any(), what      # channels never mix
                    else:
                        assert np.isfinite(ac.widen(got, ht)).all() and (got != 0xffff).all(), what
                        assert C == 1 or not np.array_equal(got[:, :, 0], got[:, :, 1]), what
                    ran += 1
    assert ran, "no mode of this case takes the direct route"


def test_replay_is_clean_under_asan_and_ubsan_in_a_program_of_its_own():
    """tests/cpp/adjoint_half_sanitize.cpp: the replay on exactly-sized heap buffers in a stand-alone program built with
    -fsanitize=address,undefined (nothing is loaded into python, nothing is preloaded)"""
    import subprocess
    from conftest import BUILD
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "adjoint_half_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "adjoint_half_sanitize.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert len(r.stdout.splitlines()) >= 100 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


SMALL = [(W, H, sr, dr, ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1]), ang) for (W, H, sr, dr, ang, off) in PLANNED_EIGHT] + [hc.CASES["h"]]
_matrices = {}
ORACLE_RAN = {}


@pytest.mark.parametrize("geo", range(len(SMALL)))
def test_replay_stays_within_one_rounding_of_the_oracles_transpose(aai, po, geo):
    """The float64 W^T g of the oracle's matrix (tests/test_adjoint_host.py: one oracle run per source pixel, so only small images can
    afford it -- the geometries of tests/test_adjoint_planned_host.py and case h) against the replay: half_cases.rounded_excess <= 0,
    one rounding to the element type on top of the project's bar."""
    W, H, sr, dr, iso, ang = SMALL[geo]
    ran = 0
    for mode in ac.MODES:
        rq = aai.make_request(W, H, sr, dr, iso, ang, mode=hc.mode_of(aai, mode))
        if not ac.is_direct(rq):
            continue
        lay = aai.query(rq)[2]
        M = _matrices.setdefault((geo, mode), oracle_matrix(po, hc.oracle_mode(po, mode), W, H, sr, dr, iso, ang))
        for ht, tname in ac.TYPES:
            g = ac.gradient_bits(lay, 3, ht)
            got = ac.widen(ac.replay(rq, ht, g), ht)
            for c in range(3):
                gold = (M.T @ ac.widen(g[:, :, c], ht).astype(np.float64).ravel()).reshape(H, W)
                excess = hc.rounded_excess(got[:, :, c], gold, ht)
                print("geometry %d %s %s channel %d: excess %.3e" % (geo, mode, tname, c, excess))
                assert excess <= 0, (geo, mode, tname, c, excess)
                assert np.all(got[:, :, c][gold == 0] == 0.0)
            ran += 1
    ORACLE_RAN[geo] = ran      # (0: this geometry's plan has correction lists in both modes -- the forwarding route serves it, not the replayed kernel)


def test_the_oracle_comparison_ran_on_most_small_geometries():
    """(after the test above)"""
    assert len(ORACLE_RAN) == len(SMALL), "the oracle test did not run for every geometry"
    assert sum(1 for n in ORACLE_RAN.values() if n) >= 6, ORACLE_RAN
