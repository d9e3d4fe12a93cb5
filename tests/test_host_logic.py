"""CPU: the host side of the product -- ABI surface, validation/geometry (aai_query), the separable-table
planner, and a serial replay of the kernels' arithmetic (tests/emulation) against the golden vectors."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, KNIFE_EDGE, KNIFE_EDGE_CASES, ROOT, RUNS_CASES, TOL, load_full, rel_err


# ---- ABI surface ---------------------------------------------------------------------------------------
def _header_functions():
    text = open(os.path.join(ROOT, "include", "aai.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(aai_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_every_declared_symbol(aai):
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    declared = _header_functions()
    assert len(declared) >= 13
    assert sorted(L.SYMBOLS) == declared, "ctypes table and include/aai.h drifted apart"
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (aai_[a-z0-9_]+)", nm))
    for name in declared:
        assert name in exported, name
        assert getattr(lib, name) is not None
    assert lib.aai_version() >= 1


def test_struct_layouts_match_header(aai):
    from area_average_interpolation_amd import _lib as L
    assert ctypes.sizeof(L.Request) == 16 + 7 * 8
    assert ctypes.sizeof(L.Layout) == 8 + 16 + 8 + 16 + 8


def test_package_never_touches_the_oracle():
    """The product path must not import, link or run anything under oracle/ (no CPU fallback)."""
    pkg = os.path.join(ROOT, "area_average_interpolation_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                for needle in ("pyoracle", "aai_oracle", "liboracle", "libaai_ref", "import oracle", "from oracle"):
                    assert needle not in text, (f, needle)
    from area_average_interpolation_amd import _lib as L
    ldd = subprocess.run(["ldd", L.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in ldd and "aai_ref" not in ldd


def test_compute_entry_points_fail_loudly_without_a_gpu(aai):
    if aai.device_count() > 0:
        pytest.skip("a GPU is present")
    from area_average_interpolation_amd import _lib as L
    rc, msg, dst, iso, lay = aai.resample_host(np.ones((4, 4), np.float32), 1, 1, (0, 0), 0)
    assert rc == L.ERR_NO_DEVICE and dst is None and "no CPU fallback" in msg
    with pytest.raises(aai.AaiError):
        aai.AreaAverageInterpolation().areaAverageInterpolation(np.ones((4, 4)), 1, 1, (0, 0), 0)
    rc, msg, dst, lay = aai.resample_batch_host(np.ones((2, 4, 4), np.uint8), 1, 1, (0, 0), 0)
    assert rc == L.ERR_NO_DEVICE and dst is None and "no CPU fallback" in msg
    with pytest.raises(aai.AaiError):
        aai.PinnedArray((4, 4), np.float32)
    rc, msg, dst, lay = aai.resample_interleaved_host(np.ones((4, 4, 3), np.float32), 1, 1, (0, 0), 0)
    assert rc == L.ERR_NO_DEVICE and dst is None and "no CPU fallback" in msg


# ---- validation and geometry -----------------------------------------------------------------------------
def test_error_codes_and_messages_match_reference(aai):
    from area_average_interpolation_amd import _lib as L
    probes = json.load(open(os.path.join(GOLDEN, "error_paths.json")))
    expect_code = {"Assumed X & Y resolution are same.": L.ERR_RESOLUTION_MISMATCH,
                   "0 or negative resolution is not acceptable.": L.ERR_RESOLUTION_NONPOSITIVE,
                   "There is no data in src array.": L.ERR_NO_ROWS,
                   "There is no data in the second dimension of src array.": L.ERR_NO_COLUMNS}
    for p in probes:
        if p["kind"] == "args":
            rq = aai.make_request(4, 4, p["src_res"], p["dst_res"], (0, 0), 0, mode=p["mode"])
        else:
            rq = aai.make_request(0 if p["rows"] else 4, p["rows"], 1, 1, (0, 0), 0, mode=p["mode"])
        rc, msg, lay = aai.query(rq)
        assert (rc == L.OK) == p["ok"]
        if not p["ok"]:
            assert msg == p["msg"] and rc == expect_code[p["msg"]] and lay is None
            assert L.load().aai_error_string(rc).decode() == p["msg"]
    # the reference method wrapper reports them as {false, message} without raising -- and before touching the GPU
    ok_msg, dst, iso = aai.AreaAverageInterpolation().areaAverageInterpolation(np.ones((4, 4)), (1, 2), 1, (0, 0), 0)
    assert ok_msg == (False, "Assumed X & Y resolution are same.") and dst is None and iso is None
    ok_msg, dst, iso = aai.AreaAverageInterpolation().fastAreaAverageInterpolation(np.ones((0, 0)), 1, 1, (0, 0), 0)
    assert ok_msg == (False, "There is no data in src array.")


def test_nonfinite_and_oversize_arguments_are_rejected(aai):
    from area_average_interpolation_amd import _lib as L
    for bad in (float("nan"), float("inf")):
        assert aai.query(aai.make_request(4, 4, 1, 1, (0, 0), bad))[0] == L.ERR_NONFINITE
        assert aai.query(aai.make_request(4, 4, 1, 1, (bad, 0), 0))[0] == L.ERR_NONFINITE
    # NaN resolutions slip through the reference's comparisons (Source.cpp:112-122); we reject
    assert aai.query(aai.make_request(4, 4, float("nan"), 1, (0, 0), 0))[0] in (L.ERR_NONFINITE, L.ERR_RESOLUTION_MISMATCH)
    assert aai.query(aai.make_request(1 << 20, 1 << 20, 1, 1e6, (0, 0), 0))[0] == L.ERR_TOO_LARGE
    assert aai.query(aai.make_request(4, 4, 1, 1, (0, 0), 0, mode=9))[0] == L.ERR_BAD_ARGUMENT
    # the weight policy proper is 0 or 1; the OR-able request bits are the three include/aai.h declares, nothing else
    for ok in (0, 1, L.POLICY_DOUBLE_PRECISION, 1 | L.POLICY_PREFER_CELL, L.POLICY_DIAG_NO_FIXUP | L.POLICY_PREFER_CELL | L.POLICY_DOUBLE_PRECISION):
        assert aai.query(aai.make_request(4, 4, 1, 1, (0, 0), 0, policy=ok))[0] == L.OK, ok
    for bad in (2, 0x80, 0x800, 0x1000 | 1, -1):
        assert aai.query(aai.make_request(4, 4, 1, 1, (0, 0), 0, policy=bad))[0] == L.ERR_BAD_ARGUMENT, bad


def test_the_library_has_no_process_wide_debug_switches(aai):
    """Round 3 shipped three exported globals that steered the library for every caller of the process (aai_debug_skip_fixup -- which
    switched the correctness pass off --, aai_debug_cell_min_waves, aai_debug_axis_tune) and eleven launch-heuristic getenv switches.
    They are per-request policy bits now (include/aai.h) or gone: the launch heuristics are fixed in the source."""
    import ctypes
    from area_average_interpolation_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("aai_debug_skip_fixup", "aai_debug_cell_min_waves", "aai_debug_axis_tune", "aai_debug_plan_shape"):
        assert not hasattr(lib, name), name
    blob = open(L.LIB_PATH, "rb").read()
    for env in (b"AAI_CELL_ROWS", b"AAI_CELL_TAIL", b"AAI_CELL\0", b"AAI_WIDE\0", b"AAI_FAST_ROWS", b"AAI_ROT_TUNE", b"AAI_AXIS_TUNE", b"AAI_AXIS_CLASS_VERIFY",
                b"AAI_FAST_LDS", b"AAI_XCD_ROWS", b"AAI_CELL_WAVE"):
        assert env not in blob, env
    for env in (b"AAI_AXIS_AUTOTUNE", b"AAI_MAX_LISTED_PIXELS", b"AAI_TRACE_PLAN"):      # the three include/aai.h documents
        assert env in blob, env


def test_query_matches_reference_layout_on_golden_cases(aai, small_golden):
    z, manifest = small_golden
    for i, c in enumerate(manifest):
        rc, msg, lay = aai.query(aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"]))
        assert rc == 0, msg
        assert [lay.dst_height, lay.dst_width] == c["shape"], i
        assert [lay.dst_iso_x, lay.dst_iso_y] == c["dst_iso"], i


def test_query_baseline_configs(aai):
    from area_average_interpolation_amd import _lib as L
    # SURVEY.md section 8(a) row A4 / Appendix C
    expect = {"cfg1": (256, 256, 127, 127, L.KERNEL_AXIS), "cfg2": (2048, 2048, 1023, 1023, L.KERNEL_AXIS),
              "cfg3": (3426, 3426, 1712, 1712, L.KERNEL_ROTATED), "cfg4": (1024, 1024, 511, 511, L.KERNEL_AXIS),
              "cfg5s": (2896, 2896, 1448, 1447, L.KERNEL_ROTATED)}
    for name, (w, h, ix, iy, kern) in expect.items():
        _, meta = load_full(name)
        rc, _, lay = aai.query(aai.make_request(meta["W"], meta["H"], meta["src_res"], meta["dst_res"], meta["iso"], meta["angle"]))
        assert rc == 0 and (lay.dst_width, lay.dst_height, lay.dst_iso_x, lay.dst_iso_y, lay.kernel) == (w, h, ix, iy, kern)
    rc, _, lay = aai.query(aai.make_request(4096, 4096, 1, 4, (2047.5, 2047.5), 45))       # cfg5 full
    assert (lay.dst_width, lay.dst_height, lay.scale, lay.side) == (23170, 23170, 6, 1.5)
    rc, _, lay = aai.query(aai.make_request(8192, 8192, 4, 1, (4095.5, 4095.5), 270, mode=L.MODE_FAST))
    assert lay.kernel == L.KERNEL_AXIS and lay.quadrant == 3
    rc, _, lay = aai.query(aai.make_request(8192, 8192, 4, 1, (4095.5, 4095.5), 17.5, mode=L.MODE_BICUBIC))
    assert lay.kernel == L.KERNEL_SAMPLE


# ---- planner: separable tables and strips ------------------------------------------------------------------
def test_strips_cover_baseline_geometry(aai, hostemu):
    # cfg2: 8192 -> 2048, windows start 2 columns into a float4 (isocenter-anchored grid):
    # 64 outputs x 4 columns must still fit one 256-column strip
    rc, (n, most, wide, span) = hostemu.strip_stats(aai.make_request(8192, 8192, 4, 1, (4095.5, 4095.5), 0))
    assert rc == 0 and (n, most, wide, span) == (32, 64, 0, 4)
    rc, (n, most, wide, span) = hostemu.strip_stats(aai.make_request(4096, 4096, 4, 1, (2047.5, 2047.5), 180))
    assert rc == 0 and (n, most, wide) == (16, 64, 0)
    # non-integer ratio, up-sampling, extreme down-sampling
    for (w, h, sr, dr) in ((1000, 700, 8192, 2731), (300, 200, 1, 4), (5000, 1200, 1000, 1), (257, 3, 1, 1)):
        for ang in (0, 90, 180, 270):
            rc, (n, most, wide, span) = hostemu.strip_stats(aai.make_request(w, h, sr, dr, ((w - 1) / 2, (h - 1) / 2), ang))
            assert rc == 0 and n >= 1, (w, h, sr, dr, ang, rc)
    rc, (_, _, wide, _) = hostemu.strip_stats(aai.make_request(5000, 1200, 1000, 1, (2499.5, 599.5), 0))
    assert wide == 1


# ---- serial replay of the device arithmetic vs the reference's golden vectors -------------------------------
def test_host_emulation_matches_small_golden(aai, hostemu, po, small_golden):
    z, manifest = small_golden
    checked = 0
    for i, c in enumerate(manifest):
        src = po.synth_image(c["W"], c["H"], c["seed"])
        for mode, tag in ((1, "exact"), (2, "fast")):
            rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=mode)
            out, axis = hostemu.resample(rq, src)
            gold = z["c%03d_%s" % (i, tag)]
            assert out.shape == gold.shape
            bad = int((rel_err(out, gold) > TOL).sum())
            allowed = KNIFE_EDGE.get((i, tag), 0)
            assert bad <= allowed, (i, tag, c, bad)
            if allowed == 0:
                assert np.array_equal(gold == 0, out == 0), (i, tag)      # exact zeros stay exact
            checked += 1
    assert checked == 2 * len(manifest)


def test_host_emulation_cfg1_full(aai, hostemu, po):
    z, meta = load_full("cfg1")
    src = po.synth_image(meta["W"], meta["H"], 1)
    for mode, tag in ((1, "exact"), (2, "fast")):
        rq = aai.make_request(meta["W"], meta["H"], meta["src_res"], meta["dst_res"], meta["iso"], meta["angle"], mode=mode)
        out, axis = hostemu.resample(rq, src)
        m = meta[tag]
        assert axis and out.shape == tuple(m["shape"])
        assert rel_err(out[::m["step"], ::m["step"]], z[tag + "_grid"]).max() <= TOL
        assert rel_err(out[m["rows"], :], z[tag + "_rows"]).max() <= TOL
        assert abs(float(out.astype(np.float64).sum()) - float(m["sum"])) <= 1e-6 * float(m["sum"])


def test_host_emulation_quadrants_agree_with_oracle(aai, hostemu, po):
    """Pre-rotation by 90/180/270 (Source.cpp:163-168) is an index map in the planner: check all four
    quadrants, scale > 1 and off-centre isocenters against the oracle."""
    rng = np.random.default_rng(3)
    for k in range(24):
        W, H = int(rng.integers(5, 70)), int(rng.integers(5, 70))
        sr, dr = [(2, 1), (3, 1), (7, 3), (1, 1), (1, 2), (5, 4)][k % 6]
        ang = [0, 90, 180, 270][k % 4] + (360 if k % 5 == 0 else 0)
        iso = (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
        src = rng.random((H, W)).astype(np.float32)
        for mode in (1, 2):
            gold = po.oracle_run(mode, src.astype(np.float64), sr, dr, iso, ang).dst
            out, axis = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=mode), src)
            assert axis and out.shape == gold.shape
            assert rel_err(out, gold).max() <= TOL, (k, mode, W, H, sr, dr, ang, iso)


def test_rows_as_runs_path_matches_oracle(aai, hostemu, po):
    """Large footprints walk each source row as boundary / interior / boundary runs (csrc/aai_rot_math.hpp: row_runs,
    aai_rotated_runs_kernel): same answers as the oracle, exact zeros exact, both policies, all quadrants, including
    knife-edge angles (flagged pixels still go through the strict replay)."""
    rng = np.random.default_rng(77)
    for k, (W, H, sr, dr, ang, off) in enumerate(RUNS_CASES):
        iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
        src = rng.random((H, W)).astype(np.float32)
        for policy in (0, 1):
            rq = aai.make_request(W, H, sr, dr, iso, ang, policy=policy)
            assert hostemu.aai_emu_uses_runs(rq) == 1, (k, "geometry does not take the runs path")
            gold = po.oracle_run(1, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
            out, axis = hostemu.resample(rq, src)
            assert not axis and out.shape == gold.shape
            assert rel_err(out, gold).max() <= TOL, (k, policy, W, H, sr, ang)
            assert np.array_equal(gold == 0, out == 0), (k, policy)
            assert hostemu.aai_emu_missed_knife_pairs() == 0, (k, policy)
    # small footprints, up-sampling and the fast mode keep the per-position loop
    assert hostemu.aai_emu_uses_runs(aai.make_request(64, 64, 3.0, 1.0, (31.5, 31.5), 17.5)) == 0
    assert hostemu.aai_emu_uses_runs(aai.make_request(64, 64, 4.0, 1.0, (31.5, 31.5), 17.5)) == 0      # interior 2.75 < kRunsMinInterior
    assert hostemu.aai_emu_uses_runs(aai.make_request(64, 64, 1.0, 4.0, (31.5, 31.5), 45.0)) == 0
    assert hostemu.aai_emu_uses_runs(aai.make_request(64, 64, 8.0, 1.0, (31.5, 31.5), 17.5, mode=2)) == 0


def test_single_cut_closed_form_equals_general_clip(aai, hostemu):
    """The closed form used for pairs cut by ONE edge line (csrc/aai_rot_math.hpp: single_cut_area, incl.
    the reference-policy substitution) must agree with the general scan-line clip + slab detection."""
    rng = np.random.default_rng(21)
    for k in range(30):
        W, H = int(rng.integers(6, 60)), int(rng.integers(6, 60))
        sr, dr = float(rng.uniform(1.0, 6.0)), float(rng.uniform(0.6, 2.0))
        ang = float(rng.uniform(0.001, 89.999)) + 90 * int(rng.integers(0, 4))
        if k % 7 == 0:
            ang = [1e-6, 89.999999, 44.9999, 45.0001, 0.5, 17.5, 33.3][k // 7 % 7]
        src = rng.random((H, W)).astype(np.float32)
        for policy in (0, 1):
            rq = aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, policy=policy)
            hostemu.aai_emu_force_general(0)
            fast, axis = hostemu.resample(rq, src)
            hostemu.aai_emu_force_general(1)
            slow, _ = hostemu.resample(rq, src)
            hostemu.aai_emu_force_general(0)
            assert not axis
            assert np.abs(fast.astype(np.float64) - slow).max() <= 2e-6, (k, policy, ang, sr, dr)


def _structured_geometries(rng, n_iso=3):
    """Geometries full of exact coincidences: rational / special angles, integer and sqrt(2) ratios,
    isocenters on pixel centres and half-pixels."""
    import math
    angs = [30, 45, 60, math.degrees(math.atan(0.5)), math.degrees(math.atan(0.75)), 15, 22.5, 135, 210, 330, 315]
    ratios = [(2, 1), (3, 1), (4, 1), (1, 1), (1, 2), (3, 2), (2.8284271247461903, 1), (1.4142135623730951, 1)]
    for ang in angs:
        for (sr, dr) in ratios:
            for kind in range(n_iso):
                W, H = int(rng.integers(16, 36)), int(rng.integers(16, 36))
                if dr / sr > 1:
                    W, H = W // 3 + 4, H // 3 + 4
                iso = [((W - 1) / 2, (H - 1) / 2), (0.0, 0.0), (float(rng.integers(0, W)), float(rng.integers(0, H)) + 0.5)][kind]
                yield W, H, float(sr), float(dr), iso, float(ang)


def test_knife_edge_geometries_match_oracle_exactly_in_class(aai, hostemu, po, small_golden):
    """Structured geometries where dst edges run through pixel corners and dst vertices sit on pixel sides:
    the fast path flags those pairs and the strict replay (csrc/aai_strict.hpp) must then agree with the
    reference restatement on EVERY pixel -- no allowance."""
    z, manifest = small_golden
    # the golden knife-edge cases need the strict pass: without it they differ, with it they do not
    for (i, tag) in KNIFE_EDGE_CASES:
        c = manifest[i]
        src = po.synth_image(c["W"], c["H"], c["seed"])
        rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=1 if tag == "exact" else 2)
        gold = z["c%03d_%s" % (i, tag)]
        hostemu.aai_emu_set_strict(0)
        loose, _ = hostemu.resample(rq, src)
        hostemu.aai_emu_set_strict(1)
        strict, _ = hostemu.resample(rq, src)
        pairs, pixels = hostemu.knife_stats()
        assert pairs > 0 and pixels > 0
        assert (rel_err(loose, gold) > TOL).sum() > 0, (i, tag)          # the production pass alone is off here
        assert (rel_err(strict, gold) > TOL).sum() == 0, (i, tag)
    rng = np.random.default_rng(4)
    runs = knife = 0
    for (W, H, sr, dr, iso, ang) in _structured_geometries(rng):
        src = rng.random((H, W)).astype(np.float32)
        for mode, omode in ((1, po.MODE_EXACT), (2, po.MODE_FAST)):
            gold = po.oracle_run(omode, src.astype(np.float64), sr, dr, iso, ang).dst
            out, axis = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=mode), src)
            knife += hostemu.knife_stats()[0]
            # the per-pixel knife test of the production pass must cover every pair-level knife edge
            assert hostemu.aai_emu_missed_knife_pairs() == 0, (W, H, sr, dr, iso, ang, mode)
            assert out.shape == gold.shape
            assert (rel_err(out, gold) > TOL).sum() == 0, (W, H, sr, dr, iso, ang, mode)
            assert np.array_equal(gold == 0, out == 0), (W, H, sr, dr, iso, ang, mode)
            runs += 1
    assert runs > 400 and knife > 50000          # the sweep really is made of knife edges


def conftest_synth(c):
    from oracle import pyoracle
    return pyoracle.synth_image(c["W"], c["H"], c["seed"])


def test_knife_edge_replay_matches_reference_goldens(aai, hostemu, po, knife_golden):
    """The same class of geometries against fixtures produced by the UNMODIFIED reference (tests/golden/knife_cases.npz),
    so that the strict replay (csrc/aai_strict.hpp) is not only compared with the oracle it shares its origin with:
    production pass + knife-edge fix-up, with and without the fp32 quad formulation for the unflagged pixels; every
    pixel within the bar, exact zeros exact."""
    z, manifest = knife_golden
    knife = 0
    for quad in (0, 1):
        hostemu.aai_emu_use_quad(quad)
        try:
            for i, c in enumerate(manifest):
                src = po.synth_image(c["W"], c["H"], c["seed"])
                for mode, tag in ((1, "exact"), (2, "fast")):
                    rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=mode)
                    out, axis = hostemu.resample(rq, src)
                    gold = z["k%03d_%s" % (i, tag)]
                    knife += hostemu.knife_stats()[0]
                    assert out.shape == gold.shape
                    assert (rel_err(out, gold) > TOL).sum() == 0, (quad, i, tag, c)
                    assert np.array_equal(gold == 0, out == 0), (quad, i, tag, c)
        finally:
            hostemu.aai_emu_use_quad(0)
    assert knife > 50000


def test_axis_aligned_knife_geometries_take_the_model_scan(aai, hostemu, axis_knife_golden):
    """K1 is built on overlap = (x overlap) * (y overlap).  The reference's classifier departs from that where a dst
    vertex sits on the midpoint of a pixel side (it returns the whole pixel), which changes the normalisation of the
    dst pixel, where a dst pixel only grazes the lattice, and -- fast mode -- where a pixel centre lies exactly on a dst
    edge or vertex: the plan's scan (csrc/aai_axis_verify.hpp) finds those dst pixels and the fix-up pass recomputes them.
    CPU replay of both against outputs of the unmodified reference (tests/golden/axis_knife_cases.npz) -- every case
    within the bar with the scan, a known set of them outside it without."""
    z, manifest = axis_knife_golden
    fixed = {1: 0, 2: 0}
    broken = {1: 0, 2: 0}
    for i, c in enumerate(manifest):
        src = conftest_synth(c)
        for mode, tag in ((1, "exact"), (2, "fast")):
            rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=mode)
            gold = z["a%03d_%s" % (i, tag)]
            out, axis = hostemu.resample(rq, src)
            n = hostemu.aai_emu_axis_fixups()
            assert axis and out.shape == gold.shape
            assert rel_err(out, gold).max() <= 1e-6 and np.array_equal(gold == 0, out == 0), (i, tag, c, float(rel_err(out, gold).max()))
            if n:
                fixed[mode] += 1
                hostemu.aai_emu_skip_axis_fixup(1)
                try:
                    raw, _ = hostemu.resample(rq, src)
                finally:
                    hostemu.aai_emu_skip_axis_fixup(0)
                broken[mode] += int(rel_err(raw, gold).max() > TOL)
    assert min(fixed.values()) >= 20 and min(broken.values()) >= 20, (fixed, broken)
    # policy EXACT differs from REFERENCE in the corner-triangle rule of a slanted edge only: the same scan at multiples of 90 degrees
    c = manifest[0]
    a, _ = hostemu.resample(aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=1, policy=1), conftest_synth(c))
    assert hostemu.aai_emu_axis_fixups() > 0 and rel_err(a, z["a000_exact"]).max() <= 1e-6


def test_axis_class_verification_equals_the_per_pixel_scan(aai, hostemu, axis_knife_golden):
    """Plans of axis-aligned requests whose arithmetic is exact check K1's separable model on the host, one representative
    per (column class, row class) -- csrc/aai_plan.cpp: axis_verify_by_class -- instead of scanning every dst pixel on the
    device (6.6 ms at config 2).  On all 576 reference-generated axis knife geometries x both modes, and on the BASELINE
    shapes, the flagged set must equal the per-pixel scan's exactly; geometries with inexact arithmetic must decline."""
    import ctypes
    z, manifest = axis_knife_golden
    qualified = flagged = 0
    for i, c in enumerate(manifest):
        for mode in (1, 2):
            rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=mode)
            a, b = ctypes.c_long(), ctypes.c_long()
            bad = hostemu.aai_emu_axis_class_verify(ctypes.byref(rq), ctypes.byref(a), ctypes.byref(b))
            assert bad in (0, -1), (i, c, mode, bad, a.value, b.value)
            if bad == 0:
                qualified += 1
                flagged += a.value
                assert a.value == b.value
    # (only dyadic ratios / isocenters qualify -- 2 : 1 of the nine ratios there; the geometries that need the fix-up pass are
    # the 3 : 1, 5 : 1 ... ones, whose coordinates round and which therefore keep the per-pixel device scan)
    assert qualified >= 96, (qualified, flagged)
    # a sweep of dyadic geometries (the side must be a power of two for 1 / side to be exact): isocenters on eighth pixels, odd
    # and even sizes, every quadrant, both modes
    swept = 0
    for (W, H) in ((12, 7), (9, 8)):
        for (sr, dr) in ((1, 1), (2, 1), (4, 1), (8, 1), (4, 2), (8, 4)):
            for fx in (0, 0.125, 0.5, 0.75):
                for ang in (0.0, 90.0, 180.0, 270.0):
                    for mode in (1, 2):
                        rq = aai.make_request(W, H, float(sr), float(dr), (W // 2 + fx, H // 2 + 0.25), ang, mode=mode)
                        a, b = ctypes.c_long(), ctypes.c_long()
                        bad = hostemu.aai_emu_axis_class_verify(ctypes.byref(rq), ctypes.byref(a), ctypes.byref(b))
                        assert bad == 0 and a.value == b.value, (W, H, sr, dr, fx, ang, mode, bad, a.value, b.value)
                        swept += 1
    assert swept == 384
    for (W, H, sr, dr, iso, ang, mode) in ((512, 512, 2.0, 1.0, (255.5, 255.5), 0.0, 1), (1024, 768, 4.0, 1.0, (511.5, 383.5), 90.0, 1),
                                           (1024, 768, 4.0, 1.0, (511.5, 383.5), 180.0, 2), (300, 200, 4.0, 2.0, (100.25, 50.0), 270.0, 1)):
        rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
        a, b = ctypes.c_long(), ctypes.c_long()
        assert hostemu.aai_emu_axis_class_verify(ctypes.byref(rq), ctypes.byref(a), ctypes.byref(b)) == 0 and a.value == b.value
    # 8192 : 2731 is not a dyadic ratio: the device scan keeps such plans
    rq = aai.make_request(600, 400, 8192.0, 2731.0, (299.5, 199.5), 0.0, mode=1)
    a, b = ctypes.c_long(), ctypes.c_long()
    assert hostemu.aai_emu_axis_class_verify(ctypes.byref(rq), ctypes.byref(a), ctypes.byref(b)) == -1


def test_structured_sweeps_of_the_replay_against_the_oracle(aai, hostemu):
    """tools/replay_sweep.py, bounded: randomised structured geometries (integer / rational ratios, isocenters on centres,
    corners, half and quarter pixels) at multiples of 90 degrees and at atan(p/q) / 15-degree / hair-breadth rotations, both
    modes, both policies -- the K1 tables with their model scan and the fp32 quad formulation with its scans, each followed by
    the strict fix-up, against the CPU oracle.  (Round 2 ran 22 k + 40 k cases of these; they found the three classes of
    axis-aligned geometries the model scan now covers.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("replay_sweep", os.path.join(ROOT, "tools", "replay_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    problems = []
    n, bad, worst, fixups = mod.sweep("axis", 2500, 101, hostemu, report=lambda *a: problems.append(a))
    assert n > 2000 and bad == 0 and fixups >= 20, (n, bad, fixups, problems[:3])
    n, bad, worst, fixups = mod.sweep("rotated", 2500, 102, hostemu, report=lambda *a: problems.append(a))
    assert n > 2000 and bad == 0 and worst <= 0.7 * TOL, (n, bad, worst, problems[:3])
    # the same angles at ratios 6:1 ... 20:1: the wide-footprint formulation (a window in parts) and its scan
    n, bad, worst, fixups = mod.sweep("wide", 600, 103, hostemu, report=lambda *a: problems.append(a))
    assert n > 500 and bad == 0 and worst <= 0.5 * TOL, (n, bad, worst, problems[:3])


def test_baseline_geometries_raise_no_knife_flags(aai, hostemu, po):
    """BASELINE configs 3 and 5 (at reduced size) never enter the strict path (zero end-point hits)."""
    for (W, sr, dr, ang) in ((768, 8192.0, 2731.0, 17.5), (96, 1.0, 4.0, 45.0)):
        src = po.synth_image(W, W, 1)
        for mode in (1, 2):
            out, axis = hostemu.resample(aai.make_request(W, W, sr, dr, ((W - 1) / 2, (W - 1) / 2), ang, mode=mode), src)
            assert not axis and hostemu.knife_stats() == (0, 0), (W, ang, mode, hostemu.knife_stats())


def test_planner_invariants_fuzzed(aai, hostemu):
    """Fuzz the axis-aligned planner (hypothesis): table sizes, window ranges, weights summing to one, strips that
    partition the lane axis with at most 256 outputs and contain their windows, and band slices that re-create the
    full tables (csrc/aai_plan.cpp)."""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=300, deadline=None)
    @given(W=st.integers(1, 3000), H=st.integers(1, 400), sr=st.floats(0.2, 50.0), dr=st.floats(0.2, 5.0),
           quadrant=st.integers(0, 3), mode=st.sampled_from([1, 2]),
           fx=st.floats(-0.2, 1.2), fy=st.floats(-0.2, 1.2))
    def check(W, H, sr, dr, quadrant, mode, fx, fy):
        if dr / sr > 4 or (W * dr / sr) * (H * dr / sr) > 4e6:
            return
        rq = aai.make_request(W, H, sr, dr, (fx * (W - 1), fy * (H - 1)), 90.0 * quadrant, mode=mode)
        rc, msg, lay = aai.query(rq)
        if rc != 0 or lay.dst_width == 0 or lay.dst_height == 0:
            return
        assert hostemu.aai_emu_axis_invariants(ctypes.byref(rq)) == 0, (W, H, sr, dr, quadrant, mode, fx, fy)

    check()
    # wide footprints with interleaved channels: the windows of neighbouring pixels' channels interleave, and a parked
    # empty entry sits below its successors -- the case where "the last window bounds the strip" used to be assumed
    # (about 86:1 RGB: a channel entry's window ended 257 elements past the strip origin)
    for (W, H, sr, dr, iso) in ((3000, 90, 86.0, 1.0, (1499.5, 44.5)), (3000, 90, 85.4, 1.0, (1400.0, 40.0)), (2600, 100, 86.3, 1.0, (2599.0, 0.0)),
                                (4000, 64, 64.0, 1.0, (1999.5, 31.5)), (3000, 90, 83.0, 1.0, (-5.0, 44.5)), (2000, 70, 50.0, 1.0, (999.5, 34.5))):
        for quadrant in range(4):
            for mode in (1, 2):
                rq = aai.make_request(W, H, sr, dr, iso, 90.0 * quadrant, mode=mode)
                rc, msg, lay = aai.query(rq)
                if rc != 0:
                    continue
                assert hostemu.aai_emu_axis_invariants(ctypes.byref(rq)) == 0, (W, H, sr, dr, iso, quadrant, mode)


def test_line_runs_never_contradict_the_pair_classifier(aai, hostemu):
    """The rows-as-runs kernel skips classify_pair for a line's interior pixels (area 1) and never visits pixels
    outside the touched interval: check, over fuzzed geometries (hypothesis) and the structured knife-edge angles, that
    classify_pair would indeed have said INSIDE / OUTSIDE for every such pixel, along rows and along columns
    (csrc/aai_rot_math.hpp: line_runs)."""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=120, deadline=None)
    @given(W=st.integers(8, 90), H=st.integers(8, 90), ratio=st.floats(1.2, 24.0), ang=st.floats(-360.0, 720.0),
           fx=st.floats(-0.1, 1.1), fy=st.floats(-0.1, 1.1), policy=st.sampled_from([0, 1]))
    def check(W, H, ratio, ang, fx, fy, policy):
        rq = aai.make_request(W, H, ratio, 1.0, (fx * (W - 1), fy * (H - 1)), ang, policy=policy)
        bad = hostemu.aai_emu_check_line_runs(ctypes.byref(rq))
        assert bad <= 0, (W, H, ratio, ang, fx, fy, bad)          # -1: axis-aligned, nothing to check

    check()
    for ang in (30.0, 45.0, 60.0, 26.565051177077990, 36.869897645844020, 1e-6, 89.999999, 135.0, 210.0, 300.0):
        for ratio in (2.0, 4.0, 5.0, 8.0, 2.0 * 2 ** 0.5, 12.0):
            for iso in ((31.5, 31.5), (32.0, 32.0), (31.75, 30.25)):
                rq = aai.make_request(64, 64, ratio, 1.0, iso, ang)
                assert hostemu.aai_emu_check_line_runs(ctypes.byref(rq)) == 0, (ang, ratio, iso)


def test_interleaved_channel_tables_replay_equals_planar(aai, hostemu):
    """Interleaved channels through the axis-aligned planner (csrc/aai_plan.cpp: build_axis_tables with channels): the
    lane table over (pixel, channel) pairs, its strips and the output addressing of enqueue() are replayed on the CPU and
    must give, for every channel, exactly what the single-channel replay gives -- all quadrants, ratios on both sides of
    4:1, up-sampling, odd widths, narrow images (per-pixel fallback), both modes."""
    rng = np.random.default_rng(51)
    cases = [(517, 40, 4, 1), (300, 33, 3, 1), (301, 21, 2, 1), (259, 17, 1, 1), (70, 50, 1, 2), (40, 30, 1, 4), (1030, 9, 8, 1),
             (263, 31, 8192, 2731), (3000, 800, 700, 1), (3, 50, 2, 1), (1, 7, 1, 1), (90, 90, 5, 2)]
    for k, (W, H, sr, dr) in enumerate(cases):
        for ang in (0.0, 90.0, 180.0, 270.0):
            C = 2 + (k + int(ang) // 90) % 3
            mode = 1 + k % 2
            iso = (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
            rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
            rc, msg, lay = aai.query(rq)
            assert rc == 0, msg
            src = rng.random((H, W, C)).astype(np.float32)
            dst = np.full((lay.dst_height, lay.dst_width, C), -1.0, np.float32)
            rc = hostemu.aai_emu_resample_channels(ctypes.byref(rq), C, src.ctypes.data, dst.ctypes.data)
            assert rc == 0, (k, W, H, sr, dr, ang, C, rc)
            for c in range(C):
                planar, axis = hostemu.resample(rq, np.ascontiguousarray(src[:, :, c]))
                assert axis
                if W * C >= 4 > W:          # strip replay vs per-pixel fallback: same weights, another summation order
                    assert np.abs(dst[:, :, c] - planar).max() <= 1e-6
                else:
                    assert np.array_equal(dst[:, :, c], planar), (k, W, H, sr, dr, ang, C, c)


# ---- the fp32 quad formulation of the rotated area kernel (csrc/aai_rot_quad.hpp) ----------------------------------
QUAD_GEOMETRIES = [  # W, H, srcRes, dstRes, angle, isocenter
    (64, 64, 3.0, 1.0, 17.5, (31.5, 31.5)), (64, 64, 8192.0, 2731.0, 17.5, (31.5, 31.5)), (32, 32, 1.0, 4.0, 45.0, (15.5, 15.5)),
    (40, 30, 2.0, 1.0, 33.3, (10.25, 3.5)), (40, 30, 1.7, 1.0, 117.0, (10.25, 3.5)), (40, 30, 4.0, 1.0, 10.0, (10.25, 3.5)),
    (40, 30, 4.0, 1.0, 80.5, (10.25, 3.5)), (40, 30, 1.0, 1.0, 200.0, (0.0, 0.0)), (33, 47, 1.0, 2.0, 300.0, (40.0, -2.0)),
    (50, 50, 2.5, 1.0, 61.0, (24.5, 24.5)), (48, 48, 1.0, 1.3, 27.0, (3.0, 44.0)),
]


def test_quad_formulas_equal_the_strict_replay_pair_by_pair(aai, hostemu):
    """Every (dst pixel, source pixel) pair of a set of geometries: the quad formulation's area (single-line term,
    segment-crossing sign tests, vertex pixels), evaluated in double precision, against the older closed forms and
    against the operation-by-operation replay of the reference's classifier (Source.cpp:986-1431) -- both policies."""
    rng = np.random.default_rng(23)
    cases = list(QUAD_GEOMETRIES)
    for k in range(30):
        W, H = int(rng.integers(8, 60)), int(rng.integers(8, 60))
        cases.append((W, H, float(rng.uniform(0.5, 4.2)), float(rng.uniform(0.5, 2.0)), float(rng.uniform(-400, 400)),
                      (float(rng.uniform(-3, W + 3)), float(rng.uniform(-3, H + 3)))))
    served = pairs = 0
    for (W, H, sr, dr, ang, iso) in cases:
        for policy in (0, 1):
            n, vs_old, vs_strict = hostemu.quad_pair_check(aai.make_request(W, H, sr, dr, iso, ang, mode=1, policy=policy))
            if n < 0:
                continue            # window wider than the masks, or too close to an axis: served by the double-precision kernel
            served += 1
            pairs += n
            assert vs_old <= 1e-11 and vs_strict <= 1e-11, (W, H, sr, dr, ang, iso, policy, vs_old, vs_strict)
    assert served >= 60 and pairs > 500000


def test_quad_fp32_replay_matches_small_golden(aai, hostemu, po, small_golden):
    """The GPU's production arrangement replayed on the CPU: fp32 quad formulation for every dst pixel its scan does
    not flag, the double-precision path (with the strict replay at knife edges) for the rest -- against the
    unmodified reference's golden outputs, no pixel excepted."""
    z, manifest = small_golden
    hostemu.aai_emu_use_quad(1)
    try:
        quad = flagged = 0
        for i, c in enumerate(manifest):
            src = po.synth_image(c["W"], c["H"], c["seed"])
            for mode, tag in ((1, "exact"), (2, "fast")):       # fast mode: centres in the square, same frame (quad_fast_pixel)
                rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=mode)
                out, axis = hostemu.resample(rq, src)
                gold = z["c%03d_%s" % (i, tag)]
                q, u = hostemu.quad_stats()
                quad += q
                flagged += u
                assert rel_err(out, gold).max() <= 0.3 * TOL, (i, c, tag, float(rel_err(out, gold).max()))
                assert np.array_equal(gold == 0, out == 0), (i, tag)
        assert quad > 50000 and flagged < 0.08 * quad, (quad, flagged)      # small images: many border pixels
    finally:
        hostemu.aai_emu_use_quad(0)


def test_cell_fp32_replay_matches_reference_goldens(aai, hostemu, po, small_golden, knife_golden):
    """The cell formulation (csrc/aai_rot_cell.hpp: every (dst, src) pair evaluated once, by the cell of the dst grid whose
    zone holds the source pixel's centre, and shared between the up to four dst pixels it feeds) replayed on the CPU in the
    kernel's arrangement -- fp32 cells where the cell scan flags nothing, the double-precision path (strict replay at knife
    edges) elsewhere -- against the unmodified reference's outputs: all 140 small cases and the 189 knife-edge geometries,
    no pixel excepted."""
    hostemu.aai_emu_use_cell(1)
    try:
        for z, manifest in (small_golden, knife_golden):
            cell = flagged = 0
            for i, c in enumerate(manifest):
                src = po.synth_image(c["W"], c["H"], c["seed"])
                rq = aai.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], c["iso"], c["angle"], mode=1)
                out, axis = hostemu.resample(rq, src)
                key = "c%03d_exact" % i
                gold = z[key] if key in z.files else z["k%03d_exact" % i]
                q, u = hostemu.quad_stats()
                cell += q
                flagged += u
                assert rel_err(out, gold).max() <= 0.3 * TOL, (i, c, float(rel_err(out, gold).max()))
                assert np.array_equal(gold == 0, out == 0), i
            assert cell > 20000 and flagged < 0.2 * cell, (cell, flagged)
    finally:
        hostemu.aai_emu_use_cell(0)


def test_fp32_replays_on_the_reference_default_call(aai, hostemu, po, refdefault_golden):
    """The reference's own example (150 -> 25.4 dpi about (455, 455), 1.5 degrees: 5.9 : 1 within two degrees of an axis, so
    hiPrec, 7 x 7 / 8 x 8 windows) on a dose-like image whose values span four decades next to each other: relative error
    against the unmodified reference's output with an absolute floor of 1e-6 (values run from 0.03 to 250) -- the fp32
    formulations' "value far below its neighbours" caveat (include/aai.h) is exactly what this image probes."""
    z, meta = refdefault_golden
    src = po.dose_image(meta["W"], meta["H"], meta["seed"])
    for hook, modes in ((hostemu.aai_emu_use_cell, ((1, "exact"),)), (hostemu.aai_emu_use_quad, ((1, "exact"), (2, "fast")))):
        hook(1)
        try:
            for mode, tag in modes:
                rq = aai.make_request(meta["W"], meta["H"], meta["src_res"], meta["dst_res"], meta["iso"], meta["angle"], mode=mode)
                out, axis = hostemu.resample(rq, src)
                q, u = hostemu.quad_stats()
                gold = z[tag]
                assert not axis and q > 0.8 * out.size - meta[tag]["zeros"], (tag, q, u)
                assert rel_err(out, gold, floor=1e-6).max() <= TOL, (tag, float(rel_err(out, gold, floor=1e-6).max()))
                assert np.array_equal(gold == 0, out == 0)
        finally:
            hook(0)


def test_band_source_rows_hold_every_window_the_cell_kernel_fetches(aai, hostemu):
    """Row bands hand the kernels a buffer with only the source rows aai_band_source_rows reports.  The cell
    kernel evaluates one more cell row and column than the band has dst rows and columns, and fetches whole lattice windows
    around zone centres: every pixel of those windows must lie inside the reported rows (a GPU fuzz run of round 3 faulted
    on exactly that).  All quadrants, up- and down-sampling, bands at the top, in the middle and at the bottom."""
    import ctypes
    rng = np.random.default_rng(8)
    checked = 0
    for k in range(160):
        W, H = int(rng.integers(20, 140)), int(rng.integers(20, 140))
        sr = float(rng.uniform(0.5, 5.0))
        dr = float(rng.uniform(0.5, 2.5))
        ang = float(rng.uniform(1.0, 89.0)) + 90.0 * (k % 4)
        iso = (float(rng.uniform(-3, W + 3)), float(rng.uniform(-3, H + 3)))
        rq = aai.make_request(W, H, sr, dr, iso, ang, mode=1)
        rc, msg, lay = aai.query(rq)
        if rc != 0 or lay.dst_height < 32:
            continue
        for _ in range(3):
            r0 = 16 * int(rng.integers(0, lay.dst_height // 16))
            r1 = int(rng.integers(r0 + 1, lay.dst_height + 1))
            out = hostemu.aai_emu_cell_band_cover(ctypes.byref(rq), r0, r1)
            assert out in (0, -1), (W, H, sr, dr, ang, iso, r0, r1, out)
            checked += out == 0
    assert checked > 150, checked


def test_band_source_rows_hold_every_window_the_wide_kernel_fetches(aai, hostemu):
    """The same for aai_wide_kernel: its parts overhang the footprint's window by up to parts - 1 positions, and every fetched
    position (clamped to the lattice, not to the band) must lie inside the rows aai_band_source_rows reports."""
    import ctypes
    rng = np.random.default_rng(9)
    checked = 0
    for k in range(120):
        W, H = int(rng.integers(300, 700)), int(rng.integers(300, 700))
        sr = float(rng.uniform(5.6, 22.0))
        ang = float(rng.uniform(0.5, 89.5)) + 90.0 * (k % 4)
        iso = (float(rng.uniform(-3, W + 3)), float(rng.uniform(-3, H + 3)))
        rq = aai.make_request(W, H, sr, float(rng.uniform(0.9, 1.1)), iso, ang, mode=1)
        rc, msg, lay = aai.query(rq)
        if rc != 0 or lay.dst_height < 32:
            continue
        for _ in range(3):
            r0 = 16 * int(rng.integers(0, lay.dst_height // 16))
            r1 = int(rng.integers(r0 + 1, lay.dst_height + 1))
            out = hostemu.aai_emu_wide_band_cover(ctypes.byref(rq), r0, r1)
            assert out in (0, -1), (W, H, sr, ang, iso, r0, r1, out)
            checked += out == 0
    assert checked > 150, checked


def test_band_source_rows_hold_what_every_kernel_family_fetches(aai, hostemu):
    """ONE cover check for every kernel family that takes a band buffer (the fault class of round 3's band over-read, not its
    instance): for random bands of random geometries -- four quadrants, replication 1 / 2 / 6 and more, ratios from x6 up-sampling to
    24:1 -- the emulation replays what each family's kernel fetches for the band's dst rows (the window kernels through the product's
    own pixel functions with a recording source, the double-precision kernels through rot_window, the samplers' tap rows) and every
    fetched element must lie in the source rows aai_band_source_rows reports, whose margin is derived from the per-family reach
    constants of the math headers (rot_window_reach, quad_window_reach, quad_fast_window_reach, cell_window_reach)."""
    import ctypes
    rng = np.random.default_rng(31)
    names = {0: "double precision", 1: "quad / wide, area", 2: "quad / wide, fast", 3: "cell", 4: "bilinear", 5: "bicubic"}
    served = {k: 0 for k in names}
    fetched = ctypes.c_long(0)
    ratios = [1 / 6.0, 0.25, 0.5, 0.77, 1.0, 1.5, 2.0, 2731.0 / 8192, 3.0, 4.0, 5.9, 8.0, 12.0, 24.0]
    bands = 0
    for k in range(150):
        ratio = ratios[k % len(ratios)] if k % 3 else float(rng.uniform(0.17, 24.0))      # source pixels per dst pixel
        dst_side = int(rng.integers(40, 110))
        W = max(8, int(dst_side * ratio * rng.uniform(0.7, 1.4))); H = max(8, int(dst_side * ratio * rng.uniform(0.7, 1.4)))
        ang = float(rng.uniform(0.3, 89.7)) + 90.0 * (k % 4)
        if k % 11 == 0:
            ang = 90.0 * (k % 4) + float(rng.choice([0.004, 0.05, 89.95, 45.0, 30.0]))
        iso = (float(rng.uniform(-3, W + 3)), float(rng.uniform(-3, H + 3)))
        rq = aai.make_request(W, H, ratio, 1.0, iso, ang, mode=1)
        rc, msg, lay = aai.query(rq)
        if rc != 0 or lay.dst_height < 17:
            continue
        for _ in range(3):
            r0 = 16 * int(rng.integers(0, lay.dst_height // 16))
            r1 = int(rng.integers(r0 + 1, lay.dst_height + 1))
            bands += 1
            for family in names:
                out = hostemu.aai_emu_band_cover(ctypes.byref(rq), r0, r1, family, ctypes.byref(fetched))
                assert out in (0, -1), (names[family], W, H, ratio, ang, iso, r0, r1, out, lay.scale)
                served[family] += 1 if (out == 0 and fetched.value > 0) else 0
    assert bands >= 400 and all(n > 100 for n in served.values()), (bands, served)


def test_staged_tile_boxes_hold_every_window_of_their_tile(aai, hostemu):
    """An LDS-staged fast-mode kernel (measured, not shipped: profiles/r04_fast_lds.txt) stages the box of each 16 x 16 dst tile
    (fast_tile_box, aai_rot_quad.hpp) and its lanes read their windows from it: every lattice position of every window (quad_fast_pixel's own arithmetic, through a recording source) must
    lie inside its tile's box, and no box may exceed the side the LDS pitch is sized for.  All quadrants, ratios 1:1 ... 5:1."""
    import ctypes
    rng = np.random.default_rng(17)
    seen = ctypes.c_long(0)
    served = 0
    for k in range(160):
        ratio = float(rng.uniform(0.75, 5.4))
        W, H = int(rng.integers(60, 260)), int(rng.integers(60, 260))
        ang = float(rng.uniform(0.3, 89.7)) + 90.0 * (k % 4)
        if k % 13 == 0:
            ang = 90.0 * (k % 4) + float(rng.choice([0.01, 45.0, 30.0, 89.99]))
        iso = (float(rng.uniform(-3, W + 3)), float(rng.uniform(-3, H + 3)))
        rq = aai.make_request(W, H, ratio, 1.0, iso, ang, mode=2)
        rc, msg, lay = aai.query(rq)
        if rc != 0:
            continue
        out = hostemu.aai_emu_fast_tile_cover(ctypes.byref(rq), ctypes.byref(seen))
        assert out in (0, -1), (W, H, ratio, ang, iso, out)
        served += 1 if (out == 0 and seen.value > 0) else 0
    assert served > 100, served


def test_live_tile_spans_hold_every_nonzero_pixel(aai, hostemu, po):
    """The per-pixel kernels on a rotated canvas skip the tiles outside each tile row's live span (csrc/aai_plan.cpp:
    rotated_live_spans) and store zeros there: every pixel the oracle gives a non-zero value must lie inside the span of its tile
    row -- all four modes, all quadrants, up- and down-sampling, isocenters that push the image off the canvas's centre."""
    import ctypes
    rng = np.random.default_rng(10)
    tables = dead_tiles = 0
    for k in range(140):
        W, H = int(rng.integers(40, 260)), int(rng.integers(40, 260))
        sr, dr = float(rng.uniform(0.5, 6.0)), float(rng.uniform(0.5, 2.0))
        if dr / sr > 2.2:
            dr = sr * 2.2
        ang = float(rng.uniform(0.5, 89.5)) + 90.0 * (k % 4)
        iso = ((W - 1) / 2, (H - 1) / 2) if k % 3 else (float(rng.uniform(-3, W + 3)), float(rng.uniform(-3, H + 3)))
        mode = 1 + k % 4
        rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
        rc, msg, lay = aai.query(rq)
        if rc != 0 or lay.dst_height < 16:
            continue
        buf = (ctypes.c_int * (2 * ((lay.dst_height + 15) // 16)))()
        n = hostemu.aai_emu_live_spans(ctypes.byref(rq), buf, len(buf))
        assert n in (0, len(buf)), n
        if n == 0:
            continue
        tables += 1
        src = rng.random((H, W)) + 0.5              # strictly positive: a pixel that gets anything is non-zero
        gold = po.oracle_run({1: po.MODE_EXACT, 2: po.MODE_FAST, 3: 3, 4: 4}[mode], src, sr, dr, iso, ang).dst
        tilesX = (lay.dst_width + 15) // 16
        for t in range(n // 2):
            first, last = buf[2 * t], buf[2 * t + 1]
            rows = gold[16 * t:16 * t + 16]
            cols = np.nonzero(rows.any(axis=0))[0]
            if cols.size:
                assert first <= cols[0] // 16 and cols[-1] // 16 <= last, (W, H, sr, dr, ang, iso, mode, t, first, last, int(cols[0]), int(cols[-1]))
            dead_tiles += tilesX if first > last else first + (tilesX - 1 - last)
    assert tables > 60 and dead_tiles > 1000, (tables, dead_tiles)
    # config 3 and config 5: about a third and a half of the canvas
    for (W, sr, dr, ang, want) in ((8192, 8192.0, 2731.0, 17.5, 0.25), (4096, 1.0, 4.0, 45.0, 0.45)):
        rq = aai.make_request(W, W, sr, dr, ((W - 1) / 2, (W - 1) / 2), ang, mode=2)
        rc, msg, lay = aai.query(rq)
        buf = (ctypes.c_int * (2 * ((lay.dst_height + 15) // 16)))()
        n = hostemu.aai_emu_live_spans(ctypes.byref(rq), buf, len(buf))
        tilesX = (lay.dst_width + 15) // 16
        dead = sum(tilesX if buf[2 * t] > buf[2 * t + 1] else buf[2 * t] + (tilesX - 1 - buf[2 * t + 1]) for t in range(n // 2))
        assert n == len(buf) and dead > want * tilesX * (n // 2), (W, ang, dead, tilesX * (n // 2))


def test_cell_live_row_interval_is_a_superset(aai, hostemu):
    """The cell kernel skips the cell rows outside cell_live_rows' interval for its 64 columns without computing anything
    (the empty corners of a rotated canvas): no cell outside the interval may contribute.  Random geometries, all quadrants,
    isocenters inside and outside the image, up- and down-sampling."""
    import ctypes
    rng = np.random.default_rng(9)
    checked = 0
    for k in range(120):
        W, H = int(rng.integers(8, 150)), int(rng.integers(8, 150))
        sr, dr = float(rng.uniform(0.5, 5.0)), float(rng.uniform(0.5, 2.5))
        ang = float(rng.uniform(0.5, 89.5)) + 90.0 * (k % 4)
        iso = (float(rng.uniform(-W, 2 * W)), float(rng.uniform(-H, 2 * H))) if k % 3 else ((W - 1) / 2, (H - 1) / 2)
        rq = aai.make_request(W, H, sr, dr, iso, ang, mode=1)
        rc, msg, lay = aai.query(rq)
        if rc != 0:
            continue
        bad = hostemu.aai_emu_cell_live_rows_check(ctypes.byref(rq))
        assert bad in (0, -1), (W, H, sr, dr, iso, ang, bad)
        checked += bad == 0
    assert checked > 90, checked


def test_cell_fp32_replay_against_oracle_at_larger_sizes(aai, hostemu, po):
    """... and against the oracle at sizes where border pixels no longer dominate: BASELINE config 3's and 5's geometries,
    all quadrants, both policies, near-axis rotations (hiPrec); few pixels left to the double-precision pass."""
    hostemu.aai_emu_use_cell(1)
    try:
        for (W, sr, dr, ang, policy) in ((768, 8192.0, 2731.0, 17.5, 0), (512, 3.0, 1.0, 33.0, 0), (128, 1.0, 4.0, 45.0, 0),
                                         (256, 1.0, 1.0, 61.0, 0), (200, 1.0, 2.0, 117.5, 1), (384, 2.0, 1.0, 215.0, 0),
                                         (512, 4.0, 1.0, 0.5, 0), (400, 2.0, 1.0, 89.5, 0), (300, 1.0, 1.0, 179.9, 0),
                                         (200, 1.0, 2.0, 0.2, 0), (384, 2.5, 1.0, 357.0, 1)):
            src = po.synth_image(W, W, 2)
            iso = ((W - 1) / 2, (W - 1) / 2)
            out, axis = hostemu.resample(aai.make_request(W, W, sr, dr, iso, ang, mode=1, policy=policy), src)
            q, u = hostemu.quad_stats()
            gold = po.oracle_run(po.MODE_EXACT, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
            assert not axis and q > 0 and u < 0.02 * q, (W, sr, dr, ang, q, u)
            assert rel_err(out, gold).max() <= 0.5 * TOL, (W, sr, dr, ang, float(rel_err(out, gold).max()))
            assert np.array_equal(gold == 0, out == 0)
    finally:
        hostemu.aai_emu_use_cell(0)


def test_quad_fp32_replay_against_oracle_at_larger_sizes(aai, hostemu, po):
    """BASELINE config 3's ratio and angle, config 5's (x4 up-sampling at 45 degrees: replicated virtual pixels) and a few
    others at sizes where border pixels no longer dominate: error well inside the bar and few pixels left to the
    double-precision pass."""
    hostemu.aai_emu_use_quad(1)
    try:
        for (W, sr, dr, ang, policy) in ((768, 8192.0, 2731.0, 17.5, 0), (512, 3.0, 1.0, 33.0, 0), (128, 1.0, 4.0, 45.0, 0),
                                         (256, 1.0, 1.0, 61.0, 0), (200, 1.0, 2.0, 117.5, 1), (384, 2.0, 1.0, 215.0, 0),
                                         # close to an axis: the reference's corner-triangle rule is steep in t (slope 1 / (2 sin)),
                                         # so the left/right edge's t comes from double precision (QuadConsts::hiPrec)
                                         (512, 4.0, 1.0, 0.5, 0), (400, 2.0, 1.0, 89.5, 0), (400, 3.0, 1.0, 0.01, 0), (300, 1.0, 1.0, 179.9, 0),
                                         (200, 1.0, 2.0, 0.2, 0), (384, 2.5, 1.0, 357.0, 1)):
            src = po.synth_image(W, W, 2)
            iso = ((W - 1) / 2, (W - 1) / 2)
            out, axis = hostemu.resample(aai.make_request(W, W, sr, dr, iso, ang, mode=1, policy=policy), src)
            q, u = hostemu.quad_stats()
            gold = po.oracle_run(po.MODE_EXACT, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
            assert not axis and q > 0 and u < 0.01 * q, (W, sr, dr, ang, q, u)
            assert rel_err(out, gold).max() <= 0.5 * TOL, (W, sr, dr, ang, float(rel_err(out, gold).max()))
            assert np.array_equal(gold == 0, out == 0)
            # fast mode in the same frame: a mean of pixel values, fp32 rounding only
            out, axis = hostemu.resample(aai.make_request(W, W, sr, dr, iso, ang, mode=2, policy=policy), src)
            q, u = hostemu.quad_stats()
            gold = po.oracle_run(po.MODE_FAST, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
            assert not axis and q > 0 and u < 0.01 * q, (W, sr, dr, ang, q, u)        # (with replication too, since round 3)
            assert rel_err(out, gold).max() <= 0.1 * TOL, (W, sr, dr, ang, float(rel_err(out, gold).max()))
            assert np.array_equal(gold == 0, out == 0)
    finally:
        hostemu.aai_emu_use_quad(0)


def test_wide_fp32_replay_against_oracle(aai, hostemu, po):
    """Footprints wider than one 8 x 8 window (ratios above ~5.5 : 1 at an angle): the fp32 formulation over a window split
    into 2 x 2 or 4 x 4 parts (csrc/aai_rotated_wide.hip), replayed on the CPU in the kernel's arithmetic and summation order."""
    hostemu.aai_emu_use_quad(1)
    try:
        for (W, H, sr, dr, ang, policy, iso) in ((512, 512, 8.0, 1.0, 17.5, 0, None), (600, 480, 6.0, 1.0, 45.0, 0, None), (640, 512, 11.0, 1.0, 33.0, 1, None),
                                                (800, 700, 16.0, 1.0, 61.0, 0, None), (768, 768, 21.0, 1.0, 45.0, 0, None), (700, 900, 14.3, 1.7, 200.5, 0, (311.2, 420.9)),
                                                # close to an axis: hiPrec
                                                (640, 640, 9.0, 1.0, 0.7, 0, None), (640, 640, 12.0, 1.0, 89.2, 1, None), (900, 500, 28.0, 1.0, 2.0, 0, None)):
            src = po.synth_image(W, H, 3)
            iso = iso or ((W - 1) / 2, (H - 1) / 2)
            out, axis = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=1, policy=policy), src)
            q, u = hostemu.quad_stats()
            gold = po.oracle_run(po.MODE_EXACT, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
            assert not axis and q > 0 and u < 0.02 * q + 2, (W, sr, dr, ang, q, u)
            assert rel_err(out, gold).max() <= 0.3 * TOL, (W, sr, dr, ang, float(rel_err(out, gold).max()))
            assert np.array_equal(gold == 0, out == 0)
            # fast mode over the same footprints (aai_wide_fast_kernel): a mean of pixel values, fp32 rounding only
            out, axis = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=2, policy=policy), src)
            q, u = hostemu.quad_stats()
            gold = po.oracle_run(po.MODE_FAST, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
            assert not axis and q > 0 and u < 0.02 * q + 2, (W, sr, dr, ang, q, u)
            assert rel_err(out, gold).max() <= 0.1 * TOL, (W, sr, dr, ang, float(rel_err(out, gold).max()))
            assert np.array_equal(gold == 0, out == 0)
        # 8-bit noise, where a dst value can lie far below its neighbours
        for (W, H, sr, dr, ang, policy) in ((400, 400, 8.0, 1.0, 17.5, 0), (500, 400, 13.0, 1.0, 45.0, 0), (400, 400, 7.0, 1.0, 1.0, 0)):
            iso = ((W - 1) / 2, (H - 1) / 2)
            for seed in range(2):
                src = np.random.default_rng(seed).integers(0, 256, size=(H, W)).astype(np.float32)
                gold = po.oracle_run(po.MODE_EXACT, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
                out, _ = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=1, policy=policy), src)
                assert hostemu.quad_stats()[0] > 0
                assert rel_err(out, gold, floor=0.256).max() <= 2e-6, (W, sr, ang, float(rel_err(out, gold, floor=0.256).max()))
    finally:
        hostemu.aai_emu_use_quad(0)
    # the geometry rule: one window up to 8 x 8, 2 x 2 parts up to 16 x 16, 4 x 4 up to 32 x 32, beyond that the double-precision kernels
    def plan_of(sr, ang):
        return aai.make_request(2048, 2048, sr, 1.0, (1023.5, 1023.5), ang, mode=1)
    assert hostemu.aai_emu_wide_parts(ctypes.byref(plan_of(5.0, 17.5))) == 0
    assert hostemu.aai_emu_wide_parts(ctypes.byref(plan_of(8.0, 17.5))) == 2
    assert hostemu.aai_emu_wide_parts(ctypes.byref(plan_of(16.0, 45.0))) == 4
    assert hostemu.aai_emu_wide_parts(ctypes.byref(plan_of(40.0, 45.0))) == 0
    assert hostemu.aai_emu_wide_parts(ctypes.byref(plan_of(8.0, 0.0))) == 0          # axis-aligned: K1
    # fast mode: the window of centres is two positions narrower
    def fast_plan_of(sr, ang):
        return aai.make_request(2048, 2048, sr, 1.0, (1023.5, 1023.5), ang, mode=2)
    assert hostemu.aai_emu_wide_parts(ctypes.byref(fast_plan_of(5.9, 1.5))) == 0      # the reference's default call: one window (aai_quad_fast_kernel)
    assert hostemu.aai_emu_wide_parts(ctypes.byref(fast_plan_of(8.0, 17.5))) == 2
    assert hostemu.aai_emu_wide_parts(ctypes.byref(fast_plan_of(20.0, 30.0))) == 4


def test_double_precision_policy_keeps_requests_off_the_fp32_formulation(aai, hostemu, po):
    """AAI_POLICY_DOUBLE_PRECISION (include/aai.h): the plan never marks such a request for the fp32 quad kernels, and the
    double-precision replay is exact to fp32 rounding even where the fp32 formulation has its worst tail (slight up-sampling
    within a degree of an axis: dst values far below their neighbours)."""
    W, H, sr, dr, ang, iso = 203, 367, 2.6611805249461478, 2.9963661425245225, 90.69816691569076, (101.0, 183.0)
    src = np.random.default_rng(5).random((H, W)).astype(np.float32)
    hostemu.aai_emu_use_quad(1)
    try:
        for mode, omode in ((1, po.MODE_EXACT), (2, po.MODE_FAST)):
            gold = po.oracle_run(omode, src.astype(np.float64), sr, dr, iso, ang, policy=1).dst
            out, _ = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=1), src)
            assert hostemu.quad_stats()[0] > 0 and rel_err(out, gold).max() <= TOL
            out, _ = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=1 | aai.POLICY_DOUBLE_PRECISION), src)
            assert hostemu.quad_stats()[0] == 0 and rel_err(out, gold).max() <= 1e-7
    finally:
        hostemu.aai_emu_use_quad(0)
    # the flag is part of the policy word: anything else in it is rejected
    bad = aai.make_request(W, H, sr, dr, iso, ang, mode=1, policy=2 | aai.POLICY_DOUBLE_PRECISION)
    rc, msg, lay = aai.query(bad)
    assert rc == 6 and "policy" in msg        # AAI_ERR_BAD_ARGUMENT


def test_quad_accuracy_where_dst_values_are_far_below_their_neighbours(aai, hostemu, po):
    """The two situations the GPU fuzz of round 2 found close to (or past) the bar in plain fp32 -- rotations within ~1.6
    degrees of an axis, and up-sampling, both on noise that puts tiny values beside large ones -- now run under hiPrec
    (edge parameters and vertex positions from double precision; profiles/r02_fuzz_parity.txt).  CPU replay of the kernels'
    arithmetic against the oracle on 8-bit noise: 7e-6 ... 1.2e-5 before, at most 2.5e-6 now."""
    cases = [  # W, H, srcRes, dstRes, angle, isocenter, policy
        (217, 168, 1.0119315959847874, 1.854544895549838, 360.50747310428073, None, 0),
        (113, 72, 0.922939311056676, 1.219781765637425, 179.59630264794134, None, 1),
        (95, 126, 0.48711324967955455, 0.9586407503613487, -359.9196040876093, None, 1),
        (140, 231, 1.0, 2.0, 297.258112637219, (60.64185182247049, 197.4686723371354), 0),
        (119, 58, 0.8158969581426692, 1.7949733079138723, 287.5, (59.0, 28.5), 0),
        (128, 128, 1.0, 4.0, 45.0, None, 0),
    ]
    for hook in (hostemu.aai_emu_use_quad, hostemu.aai_emu_use_cell):            # both fp32 formulations
        hook(1)
        try:
            for (W, H, sr, dr, ang, iso, policy) in cases:
                iso = iso or ((W - 1) / 2, (H - 1) / 2)
                worst = 0.0
                for seed in range(6):
                    src = np.random.default_rng(seed).integers(0, 256, size=(H, W)).astype(np.float32)      # 8-bit noise: a 1 beside a 255
                    gold = po.oracle_run(po.MODE_EXACT, src.astype(np.float64), sr, dr, iso, ang, policy=policy).dst
                    out, _ = hostemu.resample(aai.make_request(W, H, sr, dr, iso, ang, mode=1, policy=policy), src)
                    assert hostemu.quad_stats()[0] > 0
                    worst = max(worst, float(rel_err(out, gold, floor=0.256).max()))
                assert worst <= 4e-6, (W, H, sr, dr, ang, worst)
        finally:
            hook(0)


def test_quad_serves_the_baseline_rotated_configs(aai, hostemu):
    """configs 3 and 5 take the quad kernel, and so do rotations close to an axis (with the left/right edge's t in double
    precision); wide footprints and angles within ~0.006 degrees of an axis stay on the double-precision kernels"""
    def pairs(W, sr, dr, ang):
        return hostemu.quad_pair_check(aai.make_request(W, W, sr, dr, ((W - 1) / 2, (W - 1) / 2), ang, mode=1))[0]
    assert pairs(48, 8192.0, 2731.0, 17.5) > 0 and pairs(24, 1.0, 4.0, 45.0) > 0
    assert pairs(48, 4.0, 1.0, 0.5) > 0 and pairs(48, 2.0, 1.0, 89.5) > 0      # hiPrec
    assert pairs(48, 3.0, 1.0, 0.004) < 0 and pairs(48, 3.0, 1.0, 90 - 1e-7) < 0
    assert pairs(64, 8.0, 1.0, 17.5) < 0                                        # window wider than 8 x 8


def test_empty_output_and_shape_errors(aai):
    """An output extent that rounds to 0 is reported (the reference crashes there: its edge-line tables index
    dstSize - 1, Source.cpp:243-305 -- measured with oracle/_ref); non-2-D inputs are a ValueError, not "no data"."""
    from area_average_interpolation_amd import _lib as L
    for (W, H, sr, dr, ang) in ((1, 1, 4, 1, 0.0), (3, 1, 4, 1, 0.0), (1, 5, 4, 1, 0.0), (2, 2, 8, 1, 30.0)):
        rc, msg, lay = aai.query(aai.make_request(W, H, sr, dr, (0.0, 0.0), ang))
        assert rc == L.ERR_EMPTY_OUTPUT and "empty" in msg and lay is None, (W, H, rc, msg)
    rc, msg, lay = aai.query(aai.make_request(1, 3, 2, 1, (5.0, 5.0), 0.0))
    assert rc == 0 and (lay.dst_width, lay.dst_height) == (1, 2)
    with pytest.raises(ValueError):
        aai.resample_host(np.zeros((4, 4, 3), np.float32), 2, 1, (1.5, 1.5), 0.0)
    rc, msg, dst, iso, lay = aai.resample_host(np.zeros((0,), np.float32), 2, 1, (0, 0), 0.0)
    assert rc == L.ERR_NO_ROWS and msg == "There is no data in src array."


def test_replicated_window_indices_stay_on_the_image_for_any_window_origin(hostemu):
    """The replicated (up-sampling) border path of the window kernels turns lattice positions into source indices with a floating-point
    division.  The cell kernel evaluates cells whose window lies wholly beside the lattice (it has no branch around them): the indices
    must equal clamp(position) // scale for ANY origin -- an earlier form was exact only for windows that met the lattice and produced
    index n (one past the image) for origins beyond it, which the GPU answered with a memory access fault."""
    for n, scale in ((50, 2), (33, 3), (1024, 4), (17, 6), (4096, 6), (5, 7), (100000, 2), (3, 16)):
        mN = n * scale
        for lo, hi in ((-700, 700), (mN - 700, mN + 700)):
            assert hostemu.aai_emu_replicated_indices(n, scale, lo, hi) == 0, (n, scale, lo, hi)
