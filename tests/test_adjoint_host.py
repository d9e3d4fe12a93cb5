"""The adjoint (transposed) resampling, checks that need no GPU: ABI, argument errors before any device call, the package's
lazy torch import, the source-word rules of the new files, and a serial CPU replay of the kernels' per-pixel bodies
(tests/emulation/adjoint_emulation.cpp over csrc/aai_adjoint_math.hpp) against the oracle's matrix, and, at sizes the matrix cannot
reach, against columns of it taken from comb images (tests/adjoint_columns.py)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import BUILD, GOLDEN, ROOT, TOL, rel_err

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

# the eight hand-picked geometries of DESIGN.md section 9 ("how it is checked"): (W, H, srcRes, dstRes, angle, isocenter offset from the image centre)
EIGHT = [(24, 20, 3, 1, 17.5, (0, 0)), (20, 24, 1, 1, 30, (0.3, -0.2)), (16, 12, 1, 2, 45, (0, 0)), (24, 24, 4, 1, 0, (0, 0)),
         (20, 16, 2.5, 1, 90, (0, 0)), (18, 22, 1.7, 1, 200.25, (-3, 4)), (12, 10, 1, 3, 117.5, (0, 0)), (24, 20, 2, 1, 180, (0.5, 0.5))]


def oracle_matrix(po, omode, W, H, sr, dr, iso, ang, policy=0):
    """W of dst = W src, column by column from the oracle on unit impulses (float64)"""
    cols = []
    for s in range(W * H):
        e = np.zeros(W * H)
        e[s] = 1.0
        cols.append(po.oracle_run(omode, e.reshape(H, W), sr, dr, iso, ang, policy=policy).dst.ravel())
    return np.stack(cols, axis=1)


def adjoint_gold(po, aai, W, H, sr, dr, iso, ang, mode, policy=0, seed=7):
    """(gdst fp32 [dH, dW], W^T gdst in float64 [H, W])"""
    M = oracle_matrix(po, po.MODE_FAST if mode == aai.MODE_FAST else po.MODE_EXACT, W, H, sr, dr, iso, ang, policy)
    rc, msg, lay = aai.query(aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy))
    assert rc == 0 and M.shape == (lay.dst_width * lay.dst_height, W * H), msg
    g = np.random.default_rng(seed).random(M.shape[0]).astype(np.float32)
    return g.reshape(lay.dst_height, lay.dst_width), (M.T @ g.astype(np.float64)).reshape(H, W)


def assert_adjoint_matches(got, gold, what):
    """the bar of DESIGN.md section 9: every source pixel within TOL of gold relative to max(|gold|, 1e-3 max|gold|); exact zeros stay exact"""
    floor = 1e-3 * float(np.abs(gold).max())
    err = rel_err(got, gold, floor=floor if floor > 0 else 1e-300)
    print("%s: max rel err %.3e, %d unread source pixels" % (what, float(err.max()), int((gold == 0).sum())))
    assert float(err.max()) <= TOL, (what, float(err.max()))
    assert np.all(np.asarray(got)[gold == 0] == 0.0), what


def test_abi_declares_exports_and_binds_the_adjoint(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aai.h")).read()
    lib = L.load()
    for name in ("aai_adjoint_batch_device_f32", "aai_adjoint_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.aai_version() == 2
    assert "#define AAI_VERSION_MINOR 2" in header


def _device_call(lib, rq, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
    return lib.aai_adjoint_batch_device_f32(None if rq is None else ctypes.byref(rq), batch, gdst, dst_stride, 0, gsrc, src_stride, 0, None)


def _host_call(lib, rq, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
    return lib.aai_adjoint_f32(None if rq is None else ctypes.byref(rq), gdst, dst_stride, gsrc, src_stride, None)


def test_argument_errors_come_before_any_device_call(aai):
    """dummy (never dereferenced) pointers: every call below must return before the device is touched"""
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
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
        for call in (_device_call, _host_call):
            assert call(lib, rq) == rc and aai.last_error() == msg, (p, call.__name__)
    assert rejected >= 4
    ok = aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5)
    rc, _, lay = aai.query(ok)
    assert rc == L.OK
    for call in (_device_call, _host_call):
        for mode, name in ((L.MODE_BILINEAR, "BILINEAR"), (L.MODE_BICUBIC, "BICUBIC")):
            assert call(lib, aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=mode)) == L.ERR_BAD_ARGUMENT
            assert name in aai.last_error()
        assert call(lib, aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, policy=L.POLICY_DIAG_NO_FIXUP)) == L.ERR_BAD_ARGUMENT
        assert call(lib, aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, policy=0x800)) == L.ERR_BAD_ARGUMENT      # no new policy bit
        assert call(lib, ok, src_stride=23) == L.ERR_BAD_ARGUMENT and "Source stride" in aai.last_error()
        assert call(lib, ok, dst_stride=lay.dst_width - 1) == L.ERR_BAD_ARGUMENT and "Destination stride" in aai.last_error()
        assert call(lib, ok, gdst=None) == L.ERR_BAD_ARGUMENT and call(lib, ok, gsrc=None) == L.ERR_BAD_ARGUMENT
        assert call(lib, None) == L.ERR_BAD_ARGUMENT
    assert _device_call(lib, ok, batch=-1) == L.ERR_BAD_ARGUMENT and "batch" in aai.last_error()
    assert _device_call(lib, ok, batch=0) == L.OK
    # the two accepted hints pass validation: with batch 0 the call returns before the device
    assert _device_call(lib, aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, policy=L.POLICY_DOUBLE_PRECISION | L.POLICY_PREFER_CELL | L.POLICY_EXACT), batch=0) == L.OK
    # api wrappers raise / report the same
    with pytest.raises(aai.AaiError):
        aai.adjoint_device(aai.make_request(24, 20, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BICUBIC), 8, 8, 8, 24)
    rc, msg, g = aai.adjoint_host(np.zeros((4, 4), np.float32), (4, 4), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and g is None and msg == "Assumed X & Y resolution are same."


def test_package_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import area_average_interpolation_amd as a; "
            "assert callable(a.resample) and callable(a.adjoint_device); print('torch' in sys.modules)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "False"


def test_new_sources_keep_the_shared_machine_word_rules():
    """no scalar-store / scalar-atomic / cache-writeback instruction names, no inline assembly, no environment reads, not even
    in comments (the words are assembled here so that this file does not hold them either)"""
    words = ["s_" + w for w in ("store_dword", "buffer_store", "scratch_store", "atomic_", "buffer_atomic", "dcache_wb", "dcache_discard")]
    words += ["asm", "getenv"]
    files = [os.path.join(CSRC, "aai_adjoint.hip"), os.path.join(CSRC, "aai_adjoint_math.hpp"),
             os.path.join(ROOT, "area_average_interpolation_amd", "torch_ops.py"), os.path.join(ROOT, "tests", "emulation", "adjoint_emulation.cpp"),
             os.path.join(ROOT, "tools", "adjoint_time.py")]
    for f in files:
        text = open(f).read().lower()
        for w in words:
            assert w.lower() not in text, (f, w)


def test_clean_tree_cross_compiles_for_gfx950(tmp_path):
    """the library builds from nothing but its sources (another output and object directory; the tree's own build is untouched)"""
    out = tmp_path / "libaai_hip.so"
    r = subprocess.run(["make", "-j8", "-C", CSRC, "OUT=%s" % out, "OBJ=%s" % (tmp_path / "build_adjoint")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(out))
    assert hasattr(lib, "aai_adjoint_batch_device_f32") and hasattr(lib, "aai_adjoint_f32")
    nm = subprocess.run(["strings", str(out)], capture_output=True, text=True).stdout
    assert "aai_adjoint_gather_kernel" in nm and "aai_adjoint_norm_kernel" in nm


@pytest.fixture(scope="module")
def adjemu(aai):
    """tests/emulation/adjoint_emulation.cpp compiled with g++, no contraction: the kernels' bodies, one pixel after the other"""
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_adjemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", "adjoint_emulation.cpp")] + [os.path.join(CSRC, f) for f in
            ("aai_adjoint_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_adjoint.restype = ctypes.c_int
    lib.aai_emu_adjoint.argtypes = [ctypes.POINTER(L.Request), ctypes.c_void_p, ctypes.c_void_p]

    def run(rq, gdst):
        gdst = np.ascontiguousarray(gdst, dtype=np.float32)
        out = np.full((rq.src_height, rq.src_width), -1.0, np.float32)
        assert lib.aai_emu_adjoint(ctypes.byref(rq), gdst.ctypes.data, out.ctypes.data) == 0
        return out
    return run


@pytest.mark.parametrize("case", range(len(EIGHT)))
def test_cpu_replay_matches_the_oracle_matrix(aai, po, adjemu, case):
    W, H, sr, dr, ang, off = EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mode, policy in ((aai.MODE_AREA, aai.POLICY_REFERENCE), (aai.MODE_AREA, aai.POLICY_EXACT), (aai.MODE_FAST, aai.POLICY_REFERENCE)):
        g, gold = adjoint_gold(po, aai, W, H, sr, dr, iso, ang, mode, policy)
        got = adjemu(aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy), g)
        assert_adjoint_matches(got, gold, "replay case %d mode %d policy %d" % (case, mode, policy))


def test_cpu_replay_on_knife_edge_geometries(aai, po, adjemu, knife_golden, axis_knife_golden):
    """a sample of the reference-generated knife-edge geometries (the GPU suite runs the full strides of DESIGN.md section 9)"""
    for (z, manifest), stride in ((knife_golden, 16), (axis_knife_golden, 48)):
        ran = 0
        for i in range(0, len(manifest), stride):
            c = manifest[i]
            if c["W"] * c["H"] > 1300:
                continue
            ran += 1
            for mode in (aai.MODE_AREA, aai.MODE_FAST):
                g, gold = adjoint_gold(po, aai, c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode)
                got = adjemu(aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode), g)
                assert_adjoint_matches(got, gold, "replay knife %d mode %d" % (i, mode))
        assert ran >= 12


# ---- per-pixel gold at sizes the matrix cannot reach: comb images (tests/adjoint_columns.py) ----
# (name, W, H, srcRes, dstRes, angle, isocenter offset from the image centre, mode, policy, number of phases)
COMB_CASES = [
    ("3:1 area", 300, 220, 3, 1, 17.5, (0, 0), "area", 0, 4), ("3:1 fast", 300, 220, 3, 1, 17.5, (0, 0), "fast", 0, 4),
    ("1:3 q1", 90, 70, 1, 3, 117.5, (0, 0), "area", 0, 4), ("4:1 axis", 256, 256, 4, 1, 0.0, (0, 0), "area", 0, 4),
    ("8:1 q2", 200, 260, 8, 1, 200.25, (0, 0), "area", 0, 4), ("2:1 45", 128, 128, 2, 1, 45.0, (0, 0), "area", 0, 4),
    # near-axis pair
    ("near 0", 180, 150, 3, 1, 1e-7, (0, 0), "area", 0, 4), ("near 90", 180, 150, 3, 1, 89.9999999, (0, 0), "area", 0, 4),
    # scale >= 3 up-sampling in each quadrant (adjoint_virtual_pixel's four branches), both modes between them
    ("1:2 q0", 70, 54, 1, 2, 30.0, (0, 0), "area", 0, 4), ("1:2 q1", 54, 70, 1, 2, 107.5, (0.3, -0.2), "fast", 0, 4),
    ("1:3 q2", 60, 44, 1, 3, 200.25, (0, 0), "fast", 0, 4), ("1:2 q3", 58, 66, 1, 2, 305.0, (0, 0), "area", 0, 4),
    ("40:1", 420, 380, 40, 1, 17.5, (0, 0), "area", 0, 4), ("40:1 fast", 420, 380, 40, 1, 17.5, (0, 0), "fast", 0, 2),
    ("iso outside", 150, 130, 3, 1, 17.5, (-240.0, 170.0), "area", 0, 4), ("iso outside q2 up", 50, 60, 1, 2, 215.0, (90.0, -75.0), "area", 0, 4),
    ("exact policy", 300, 220, 3, 1, 17.5, (0, 0), "area", 1, 4), ("exact policy 1:1", 140, 120, 1, 1, 30.0, (0.3, -0.2), "area", 1, 4),
    ("1500 x 1200", 1500, 1200, 3, 1, 17.5, (0, 0), "area", 0, 2), ("1600 x 1300 fast", 1600, 1300, 3, 1, 107.5, (0, 0), "fast", 0, 2),
]


def corner_phases(W, H, pitch, count):
    """phases by index: column 0 / row 0, the last column / last row, then column 0 with the last row and the last column with row 0"""
    a, b = (W - 1) % pitch, (H - 1) % pitch
    out = []
    for ph in ((0, 0), (a, b), (0, b), (a, 0), (pitch // 2, pitch // 2), (1, pitch - 1)):
        if ph not in out:
            out.append(ph)
    return out[:count]


def comb_case_gold(po, aai, case, seed=7):
    """(rq, gdst fp32, sx, sy, gold) of a COMB_CASES entry"""
    from adjoint_columns import comb_cases, comb_pitch
    name, W, H, sr, dr, ang, off, mode, policy, phases = case
    mode = aai.MODE_FAST if mode == "fast" else aai.MODE_AREA
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
    rc, msg, lay = aai.query(rq)
    assert rc == 0, msg
    g = np.random.default_rng(seed).random((lay.dst_height, lay.dst_width)).astype(np.float32)
    pitch = comb_pitch(lay, ang)
    phs = corner_phases(W, H, pitch, phases)
    assert len(phs) == phases and phs[0] == (0, 0) and phs[1] == ((W - 1) % pitch, (H - 1) % pitch)
    sx, sy, gold = comb_cases(po, po.MODE_FAST if mode == aai.MODE_FAST else po.MODE_EXACT, W, H, sr, dr, iso, ang, policy, g, phs, pitch)
    # row 0, column 0, the last row and the last column are among the pixels, and the samples are not all in unread corners
    assert (sx == 0).any() and (sy == 0).any() and (sx == W - 1).any() and (sy == H - 1).any()
    assert sx.size >= phases * (W // pitch) * (H // pitch) and 4 * int((gold != 0).sum()) >= sx.size
    return rq, g, sx, sy, gold


@pytest.mark.parametrize("case", COMB_CASES, ids=[c[0] for c in COMB_CASES])
def test_cpu_replay_matches_comb_gold(aai, po, adjemu, case):
    """the replay of the kernels' per-pixel bodies against columns of the oracle's matrix taken from comb images: images up to
    1600 x 1300, coordinates up to 1600, footprints up to 40:1, every quadrant of a replicated (scale >= 3) source"""
    rq, g, sx, sy, gold = comb_case_gold(po, aai, case)
    got = adjemu(rq, g)
    assert_adjoint_matches(got[sy, sx], gold, "replay comb %s (%d source pixels)" % (case[0], sx.size))


def test_pixel_list_comb_equals_the_full_comb(aai, po, adjemu):
    """the pixel-list form of the comb (oracle_pixels on candidates from conftest.sample_points: what the GPU suite uses at size) gives
    the full form's gold, adjacent pixels and every quadrant included"""
    from adjoint_columns import comb_gold_pixels
    for case in (COMB_CASES[0], COMB_CASES[1], COMB_CASES[4], COMB_CASES[8], COMB_CASES[9], COMB_CASES[10], COMB_CASES[11], COMB_CASES[14]):
        rq, g, sx, sy, gold = comb_case_gold(po, aai, case[:9] + (2,))
        lay = aai.query(rq)[2]
        pick = np.arange(0, sx.size, max(1, sx.size // 150))
        omode = po.MODE_FAST if rq.mode == aai.MODE_FAST else po.MODE_EXACT
        listed, n = comb_gold_pixels(po, omode, rq, lay, lambda dx, dy: g[dy, dx], sx[pick], sy[pick])
        assert n > 0 and np.array_equal(listed, gold[pick]), case[0]
        # a 4 x 4 block of adjacent pixels in a corner and one in the middle: split over comb images, same bar as the full comb
        W, H = rq.src_width, rq.src_height
        bx, by = [a.ravel() for a in np.meshgrid(np.arange(4), np.arange(4))]
        bx, by = np.concatenate([W - 4 + bx, W // 2 + bx]), np.concatenate([H - 4 + by, H // 2 + by])
        block, _ = comb_gold_pixels(po, omode, rq, lay, lambda dx, dy: g[dy, dx], bx, by)
        assert_adjoint_matches(adjemu(rq, g)[by, bx], block, "replay pixel-list comb %s" % case[0])
