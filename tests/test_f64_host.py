"""The reference-precision path (include/aai_f64.h: forward and adjoint on double images), checks that need no GPU: ABI, argument
errors before any device call, a clean cross-compile, and a serial CPU replay of the three kernels' per-pixel bodies
(tests/emulation/f64_emulation.cpp over csrc/aai_f64_math.hpp and csrc/aai_adjoint_math.hpp) against the oracle, against the outputs the
UNMODIFIED reference recorded, and -- forward against adjoint -- element by element as a matrix and its transpose.

The two bars, both far below the 5.9e-8 that ONE fp32 rounding of a value costs (so nothing built on the fp32 entries passes) and at
least 28 x above what the replay measures on the shapes they apply to (DESIGN.md section 9 quotes the measured distances):
  F64_TOL         against the oracle on wide-range data, |got - gold| / (the oracle on |src|): the error relative to the
                  magnitude-weighted average under the footprint, which is what summation in double can promise when the terms span
                  twelve decades and cancel
  F64_GOLDEN_TOL  against the reference-recorded float64 outputs on their own [0, 1) / dose sources, with the suite's floor"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import BUILD, GOLDEN, ROOT, rel_err
from test_adjoint_host import EIGHT, oracle_matrix

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

F64_TOL = 1e-8
F64_GOLDEN_TOL = 1e-11
ENTRIES = ("aai_resample_batch_device_f64", "aai_resample_exact_f64", "aai_adjoint_batch_device_f64", "aai_adjoint_f64")
# (mode, policy) by name: the three of every EIGHT sweep
THREE = (("area", 0), ("area", 1), ("fast", 0))
# the single geometries of the issue: (name, W, H, srcRes, dstRes, angle, isocenter offset from the image centre)
SINGLES = [("3:1", 300, 220, 3, 1, 17.5, (0, 0)), ("1:3 q1", 90, 70, 1, 3, 117.5, (0, 0)), ("40:1", 420, 380, 40, 1, 17.5, (0, 0)),
           ("near 0", 180, 150, 3, 1, 1e-7, (0, 0)), ("near 90", 180, 150, 3, 1, 89.9999999, (0, 0)),
           ("iso outside", 150, 130, 3, 1, 17.5, (-240.0, 170.0))]


def wide_range(shape, seed=7):
    """signed values over twelve decades: N(0, 1) x 10^U(-6, 6)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, shape)


def f64_measure(got, gold, scale, what):
    """worst |got - gold| / scale, scale = the oracle on |src| (forward) or |W|^T |g| (adjoint); where scale is 0 got must be exactly 0"""
    got, gold, scale = np.asarray(got, np.float64), np.asarray(gold, np.float64), np.asarray(scale, np.float64)
    assert got.shape == gold.shape == scale.shape, (what, got.shape, gold.shape)
    dead = scale == 0
    assert np.all(got[dead] == 0.0), what
    live = ~dead
    if not live.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        err = np.abs(got[live] - gold[live]) / scale[live]
    assert not np.isnan(err).any(), what
    return float(err.max())


def modes_of(aai, po, name):
    return (aai.MODE_FAST, po.MODE_FAST) if name == "fast" else (aai.MODE_AREA, po.MODE_EXACT)


def forward_gold(po, omode, src, sr, dr, iso, ang, policy=0):
    """(the oracle on src, the oracle on |src|)"""
    return (po.oracle_run(omode, src, sr, dr, iso, ang, policy=policy).dst, po.oracle_run(omode, np.abs(src), sr, dr, iso, ang, policy=policy).dst)


def test_abi_declares_exports_and_binds_the_f64_entries(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aai_f64.h")).read()
    base = open(os.path.join(ROOT, "include", "aai.h")).read()
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.F64_SYMBOLS and name not in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == L.F64_SYMBOLS[name][1]
        assert name not in base
    assert lib.aai_version() == 2
    assert "#define AAI_VERSION_MINOR 2" in base
    for name in ("resample_device_f64", "adjoint_device_f64", "resample_exact_host", "adjoint_exact_host"):
        assert callable(getattr(aai, name)) and name in aai.__all__


def _fwd_device(lib, rq, batch=1, a=8, dst_stride=1 << 20, b=8, src_stride=1 << 20):
    return lib.aai_resample_batch_device_f64(None if rq is None else ctypes.byref(rq), batch, b, src_stride, 0, a, dst_stride, 0, None)


def _fwd_host(lib, rq, a=8, dst_stride=1 << 20, b=8, src_stride=1 << 20):
    return lib.aai_resample_exact_f64(None if rq is None else ctypes.byref(rq), b, src_stride, a, dst_stride, None)


def _adj_device(lib, rq, batch=1, a=8, dst_stride=1 << 20, b=8, src_stride=1 << 20):
    return lib.aai_adjoint_batch_device_f64(None if rq is None else ctypes.byref(rq), batch, a, dst_stride, 0, b, src_stride, 0, None)


def _adj_host(lib, rq, a=8, dst_stride=1 << 20, b=8, src_stride=1 << 20):
    return lib.aai_adjoint_f64(None if rq is None else ctypes.byref(rq), a, dst_stride, b, src_stride, None)


def _f32_device(lib, rq, batch=1, a=8, dst_stride=1 << 20, b=8, src_stride=1 << 20):
    return lib.aai_adjoint_batch_device_f32(None if rq is None else ctypes.byref(rq), batch, a, dst_stride, 0, b, src_stride, 0, None)


def test_argument_errors_come_before_any_device_call(aai):
    """dummy (never dereferenced) pointers: every call below must return before the device is touched.  a = the dst-side image (dst /
    gdst), b = the source-side image (src / gsrc); every refusal is also compared with aai_adjoint_batch_device_f32's code, and its
    message where the message does not name the entry"""
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    probes = json.load(open(os.path.join(GOLDEN, "error_paths.json")))
    calls = (_fwd_device, _fwd_host, _adj_device, _adj_host)
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
        for call in calls:
            assert call(lib, rq) == rc and aai.last_error() == msg, (p, call.__name__)
    assert rejected >= 4
    ok = aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5)
    rc, _, lay = aai.query(ok)
    assert rc == L.OK

    def same_as_f32(call, rq, **kw):
        """the f64 entry's (code, message) and the f32 adjoint's on the same arguments"""
        got = (call(lib, rq, **kw), aai.last_error())
        return got, (_f32_device(lib, rq, **kw), aai.last_error())

    for call in calls:
        for mode, name in ((L.MODE_BILINEAR, "BILINEAR"), (L.MODE_BICUBIC, "BICUBIC")):
            assert call(lib, aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=mode)) == L.ERR_BAD_ARGUMENT
            assert name in aai.last_error()
        assert call(lib, aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, policy=L.POLICY_DIAG_NO_FIXUP)) == L.ERR_BAD_ARGUMENT
        assert "DIAG_NO_FIXUP" in aai.last_error()
        for rq, kw in ((aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, policy=0x800), {}),      # no new policy bit
                       (ok, {"src_stride": 23}), (ok, {"dst_stride": lay.dst_width - 1}), (ok, {"a": None}), (ok, {"b": None}), (None, {})):
            got, f32 = same_as_f32(call, rq, **kw)
            assert got == f32 and got[0] == L.ERR_BAD_ARGUMENT, (call.__name__, kw, got, f32)
        assert call(lib, ok, src_stride=23) == L.ERR_BAD_ARGUMENT and "Source stride" in aai.last_error()
        assert call(lib, ok, dst_stride=lay.dst_width - 1) == L.ERR_BAD_ARGUMENT and "Destination stride" in aai.last_error()
    for call in (_fwd_device, _adj_device):
        got, f32 = same_as_f32(call, ok, batch=-1)
        assert got == f32 and got[0] == L.ERR_BAD_ARGUMENT and "batch" in got[1]
        # a negative batch is reported before a bad geometry and after a bad request, as the f32 adjoint reports it
        bad = aai.make_request(4, 4, (1, 2), 1, (0, 0), 0)
        got, f32 = same_as_f32(call, bad, batch=-1)
        assert got == f32
        assert call(lib, ok, batch=0) == L.OK
        # the two accepted hints and the rule bit pass validation: with batch 0 the call returns before the device
        assert call(lib, aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, policy=L.POLICY_DOUBLE_PRECISION | L.POLICY_PREFER_CELL | L.POLICY_EXACT),
                    batch=0) == L.OK
    # api wrappers raise / report the same
    with pytest.raises(aai.AaiError):
        aai.resample_device_f64(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BICUBIC), 8, 24, 8, 8)
    with pytest.raises(aai.AaiError):
        aai.adjoint_device_f64(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BILINEAR), 8, 8, 8, 24)
    rc, msg, dst, iso, out_lay = aai.resample_exact_host(np.zeros((4, 4)), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and dst is None and msg == "Assumed X & Y resolution are same."
    rc, msg, g = aai.adjoint_exact_host(np.zeros((4, 4)), (4, 4), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and g is None and msg == "Assumed X & Y resolution are same."
    rc, msg, dst, iso, out_lay = aai.resample_exact_host(np.zeros((0, 0)), 1, 1, (0, 0), 0)
    assert rc == L.ERR_NO_ROWS and dst is None
    # the class: exact=True reports the reference's errors the reference's way
    status, dst, iso = aai.AreaAverageInterpolation(exact=True).areaAverageInterpolation(np.zeros((4, 4)), (1, 2), 1, (0, 0), 0)
    assert status == (False, "Assumed X & Y resolution are same.") and dst is None and iso is None
    assert aai.AreaAverageInterpolation().exact is False and aai.AreaAverageInterpolation(0, True).exact is True


def test_clean_tree_cross_compiles_for_gfx950(tmp_path):
    """the library builds from nothing but its sources (another output and object directory; the tree's own build is untouched)"""
    out = tmp_path / "libaai_hip.so"
    r = subprocess.run(["make", "-j8", "-C", CSRC, "OUT=%s" % out, "OBJ=%s" % (tmp_path / "build_f64")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(out))
    for name in ENTRIES:
        assert hasattr(lib, name), name
    nm = subprocess.run(["strings", str(out)], capture_output=True, text=True).stdout
    for kernel in ("aai_f64_forward_kernel", "aai_f64_adjoint_norm_kernel", "aai_f64_adjoint_gather_kernel"):
        assert kernel in nm, kernel


@pytest.fixture(scope="module")
def f64emu(aai):
    """tests/emulation/f64_emulation.cpp compiled with g++, no contraction: the three kernels' bodies, one pixel after the other"""
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_f64emu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", "f64_emulation.cpp")] + [os.path.join(CSRC, f) for f in
            ("aai_f64_math.hpp", "aai_adjoint_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    for fn in (lib.aai_emu_f64_forward, lib.aai_emu_f64_adjoint):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(L.Request), ctypes.c_void_p, ctypes.c_void_p]

    class Emu:
        @staticmethod
        def forward(rq, src):
            src = np.ascontiguousarray(src, dtype=np.float64)
            assert src.shape == (rq.src_height, rq.src_width)
            rc, msg, lay = aai.query(rq)
            assert rc == 0, msg
            out = np.full((lay.dst_height, lay.dst_width), -1.0, np.float64)
            assert lib.aai_emu_f64_forward(ctypes.byref(rq), src.ctypes.data, out.ctypes.data) == 0
            return out

        @staticmethod
        def adjoint(rq, gdst):
            gdst = np.ascontiguousarray(gdst, dtype=np.float64)
            out = np.full((rq.src_height, rq.src_width), -1.0, np.float64)
            assert lib.aai_emu_f64_adjoint(ctypes.byref(rq), gdst.ctypes.data, out.ctypes.data) == 0
            return out
    return Emu


def eight_case(aai, case, mode_name, policy):
    W, H, sr, dr, ang, off = EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    mode = aai.MODE_FAST if mode_name == "fast" else aai.MODE_AREA
    return aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy), (W, H, sr, dr, iso, ang)


def check_forward_wide(po, run, rq, geom, omode, policy, what, seed=7):
    """run(rq, src) against the oracle on wide-range data; returns the worst distance"""
    W, H, sr, dr, iso, ang = geom
    src = wide_range((H, W), seed)
    gold, scale = forward_gold(po, omode, src, sr, dr, iso, ang, policy)
    worst = f64_measure(run(rq, src), gold, scale, what)
    print("%s: forward worst %.3e" % (what, worst))
    assert worst <= F64_TOL, (what, worst)
    return worst


def check_adjoint_wide(po, aai, run, rq, geom, omode, policy, what, seed=11):
    """run(rq, g) against (the oracle's matrix)^T g with wide-range g; returns the worst distance"""
    W, H, sr, dr, iso, ang = geom
    M = oracle_matrix(po, omode, W, H, sr, dr, iso, ang, policy)
    lay = aai.query(rq)[2]
    assert M.shape == (lay.dst_width * lay.dst_height, W * H)
    g = wide_range((lay.dst_height, lay.dst_width), seed)
    gold, scale = (M.T @ g.ravel()).reshape(H, W), (np.abs(M).T @ np.abs(g).ravel()).reshape(H, W)
    worst = f64_measure(run(rq, g), gold, scale, what)
    print("%s: adjoint worst %.3e" % (what, worst))
    assert worst <= F64_TOL, (what, worst)
    return worst


@pytest.mark.parametrize("case", range(len(EIGHT)))
def test_cpu_replay_matches_the_oracle(aai, po, f64emu, case):
    """forward against the oracle, adjoint against the oracle's matrix, EIGHT x {area, area with POLICY_EXACT, fast}, wide-range data"""
    for name, policy in THREE:
        rq, geom = eight_case(aai, case, name, policy)
        omode = modes_of(aai, po, name)[1]
        check_forward_wide(po, f64emu.forward, rq, geom, omode, policy, "replay case %d %s policy %d" % (case, name, policy))
        check_adjoint_wide(po, aai, f64emu.adjoint, rq, geom, omode, policy, "replay case %d %s policy %d" % (case, name, policy))


def test_cpu_replay_forward_on_the_small_geometries(aai, po, f64emu, small_golden):
    """all 140 reference-generated geometries, both modes: against the arrays the UNMODIFIED reference recorded on its [0, 1) source
    (F64_GOLDEN_TOL, the suite's floor of 1e-3, exact zeros exact) and against the oracle on wide-range data (F64_TOL)"""
    z, manifest = small_golden
    worst_gold = worst_wide = 0.0
    for i, c in enumerate(manifest):
        src = np.asarray(po.synth_image(c["W"], c["H"], c["seed"]), np.float64)
        geom = (c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"])
        for name, tag in (("area", "exact"), ("fast", "fast")):
            mode, omode = modes_of(aai, po, name)
            rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode)
            got, gold = f64emu.forward(rq, src), z["c%03d_%s" % (i, tag)]
            assert got.shape == gold.shape, (i, tag)
            err = float(rel_err(got, gold).max())
            worst_gold = max(worst_gold, err)
            assert err <= F64_GOLDEN_TOL, (i, tag, err)
            assert np.array_equal(gold == 0, got == 0), (i, tag)
            worst_wide = max(worst_wide, check_forward_wide(po, f64emu.forward, rq, geom, omode, 0, "replay small %d %s" % (i, tag)))
    print("replay small_cases: worst against the recorded arrays %.3e, against the oracle on wide-range data %.3e" % (worst_gold, worst_wide))


def golden_sweep(aai, po, manifest, indices, tag, forward, adjoint):
    """the geometries `indices` of a knife-edge manifest (a fixed stride by index, never a choice by outcome), both modes: the forward
    at every one, the adjoint (None: not run) where the oracle's matrix is affordable (<= 1300 source pixels); returns (geometries
    visited, with the adjoint, worst forward, worst adjoint)"""
    ran = ran_adj = 0
    wf = wa = 0.0
    for i in indices:
        c = manifest[i]
        geom = (c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"])
        ran += 1
        small = adjoint is not None and c["W"] * c["H"] <= 1300
        ran_adj += small
        for name in ("area", "fast"):
            mode, omode = modes_of(aai, po, name)
            rq = aai.make_request(*geom[:2], *geom[2:], mode=mode)
            wf = max(wf, check_forward_wide(po, forward, rq, geom, omode, 0, "%s %d %s" % (tag, i, name)))
            if small:
                wa = max(wa, check_adjoint_wide(po, aai, adjoint, rq, geom, omode, 0, "%s %d %s" % (tag, i, name)))
    print("%s: %d geometries (%d with the adjoint), worst forward %.3e, worst adjoint %.3e" % (tag, ran, ran_adj, wf, wa))
    return ran, ran_adj, wf, wa


def test_cpu_replay_on_knife_edge_geometries(aai, po, f64emu, knife_golden, axis_knife_golden):
    """the forward at strides 4 / 12 through the reference-generated knife-edge geometries (the GPU suite adds the adjoint, whose gold is
    the oracle's matrix: W H oracle runs per geometry)"""
    assert golden_sweep(aai, po, knife_golden[1], range(0, len(knife_golden[1]), 4), "replay knife", f64emu.forward, None)[0] >= 45
    assert golden_sweep(aai, po, axis_knife_golden[1], range(0, len(axis_knife_golden[1]), 12), "replay axis knife", f64emu.forward, None)[0] >= 45


def test_cpu_replay_on_the_reference_default_call(aai, po, f64emu, refdefault_golden):
    """the reference's own example call on a 911 x 911 dose-like image (values over four decades) against the UNMODIFIED reference's
    output: F64_GOLDEN_TOL with the suite's floor for this image (1e-6), exact zeros exact"""
    z, meta = refdefault_golden
    src = np.asarray(po.dose_image(meta["W"], meta["H"], meta["seed"]), np.float64)
    for name, tag in (("area", "exact"), ("fast", "fast")):
        rq = aai.make_request(meta["W"], meta["H"], meta["src_res"], meta["dst_res"], meta["iso"], meta["angle"], mode=modes_of(aai, po, name)[0])
        got, gold = f64emu.forward(rq, src), z[tag]
        assert got.shape == gold.shape
        err = float(rel_err(got, gold, floor=1e-6).max())
        print("replay refdefault %s: %.3e" % (tag, err))
        assert err <= F64_GOLDEN_TOL, (tag, err)
        assert np.array_equal(got == 0, gold == 0), tag


@pytest.mark.parametrize("case", SINGLES + [("1500 x 1200", 1500, 1200, 3, 1, 17.5, (0, 0))], ids=lambda c: c[0])
def test_cpu_replay_forward_at_larger_sizes(aai, po, f64emu, case):
    name, W, H, sr, dr, ang, off = case
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mname in ("area", "fast"):
        mode, omode = modes_of(aai, po, mname)
        check_forward_wide(po, f64emu.forward, aai.make_request(W, H, sr, dr, iso, ang, mode=mode), (W, H, sr, dr, iso, ang), omode, 0,
                           "replay %s %s" % (name, mname))


def transpose_check(aai, forward_columns, adjoint_columns, case, mode_name, what):
    """A = the forward's matrix (dW dH x W H) from unit impulses, B = the adjoint's (W H x dW dH): the same zero pattern, and
    |A - B^T| <= (scale^2 + 2) eps A element by element.  Why a bound of that size: every term is positive, so relative errors carry
    over.  A[d, s] adds the up to scale^2 weights of s's virtual pixels (the products with 1 are exact) and divides by the sum; B[s, d]
    rounds 1 / sum, then each product w n, and adds in the same order: scale^2 roundings on one side, scale^2 + 2 on the other, each
    at most eps / 2 and partly shared."""
    rq, geom = eight_case(aai, case, mode_name, 0)
    lay = aai.query(rq)[2]
    A, B = forward_columns(rq, lay), adjoint_columns(rq, lay)
    assert A.shape == (lay.dst_width * lay.dst_height, geom[0] * geom[1]) and B.shape == A.shape[::-1]
    assert np.array_equal(A != 0, B.T != 0), what
    assert (A >= 0).all() and A.any(), what
    bound = (lay.scale ** 2 + 2) * 2.0 ** -52 * A
    excess = np.abs(A - B.T) - bound
    live = A != 0
    print("%s: worst |A - B^T| / A = %.2f eps (bound %d eps)" % (what, float((np.abs(A - B.T)[live] / A[live]).max() / 2.0 ** -52), lay.scale ** 2 + 2))
    assert (excess <= 0).all(), (what, float(excess.max()))


@pytest.mark.parametrize("case", range(len(EIGHT)))
def test_cpu_replay_forward_and_adjoint_are_transposes_element_by_element(aai, f64emu, case):
    def fcols(rq, lay):
        W, H = rq.src_width, rq.src_height
        cols = []
        for s in range(W * H):
            e = np.zeros(W * H)
            e[s] = 1.0
            cols.append(f64emu.forward(rq, e.reshape(H, W)).ravel())
        return np.stack(cols, axis=1)

    def acols(rq, lay):
        n = lay.dst_width * lay.dst_height
        cols = []
        for d in range(n):
            e = np.zeros(n)
            e[d] = 1.0
            cols.append(f64emu.adjoint(rq, e.reshape(lay.dst_height, lay.dst_width)).ravel())
        return np.stack(cols, axis=1)
    for name in ("area", "fast"):
        transpose_check(aai, fcols, acols, case, name, "replay transpose case %d %s" % (case, name))
