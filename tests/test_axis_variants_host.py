"""CPU (no GPU): the case table of tests/axis_variants.py -- one small geometry per (kernel, source type, launch shape, strip branch or
tile pipeline, store shape) the launcher of the axis-aligned family can choose, and five large ones (seven launches) -- is what it claims to be, and the
CPU replay of K1 answers every small geometry like the oracle does.  test_axis_variants_gpu.py runs the same table on the MI355X."""
import ctypes

import numpy as np
import pytest

import axis_variants as av
from conftest import TOL, rel_err


@pytest.fixture(scope="module")
def tab(hostemu):
    return av.table(hostemu)


def test_each_case_selects_the_candidate_it_was_built_for(tab):
    """(a) the probe, asked about the case as it will be launched (its size, isocenter, quadrant, mode, type, channels and the
    two images of the GPU module), reports the case's candidate and the kernel aai_last_kernel() will be compared with."""
    cands, big, tall, cases, probe = tab
    for case in cases:
        p = case.point
        assert p.batch == av.BATCH
        v = av.probe_point(probe, p)
        assert case.cand in av.hosted(v, p.T, p.C, p.W), (av.case_id(case), v)
        assert av.KERNELS[v.kernel] == case.cand.kernel and (v.dW, v.dH) == (case.dW, case.dH), (av.case_id(case), v)
        assert p.W * p.H <= 80000 or case.cand.sub == "footprint", av.case_id(case)       # small: about 300 x 230 at the most
        assert case.dW * case.dH <= 100000, av.case_id(case)
    # the large cases: what the table says they are there for
    v = {name: av.probe_point(probe, p) for name, p in av.BIG.items()}
    for name, sign, outputs, nq in (("a270", 1, 100, 2), ("a90", -1, 100, 2), ("e270", 1, 200, 4)):
        # (b_stores 0b11: the 16-byte stores and the scalar tail; b_nq: one bit, the strip's outputs per lane)
        assert (av.KERNELS[v[name].kernel], v[name].branches, v[name].rows, v[name].b_iters, v[name].b_stores, v[name].sign_b) == \
               ("aai_axis_kernel", 1 << 1, 32, 8, 0b11, sign), v[name]
        assert (v[name].max_outputs, v[name].max_row_span, v[name].b_nq) == (outputs, 2, 1 << (nq - 1)), v[name]
    for name, sign in (("b90", -1), ("b270", 1)):
        assert (av.KERNELS[v[name].kernel], v[name].branches, v[name].rows, v[name].a_iters, v[name].a_stores & 1, v[name].sign_b) == \
               ("aai_axis_kernel", 1 << 0, 32, 4, 1, sign), v[name]
    assert (v["c"].rows, v["d"].rows) == (8, 4) and v["c"].kernel == v["d"].kernel == 1, (v["c"], v["d"])
    # ... and one image of the same requests is not enough to start the escalation of 8- / 16-bit sources
    for name in ("c", "d"):
        assert av.probe_point(probe, av.BIG[name]._replace(batch=1)).rows == 1


def test_case_table_covers_the_candidate_set_exactly(tab):
    """(b) a fresh scan of the grid (axis_variants.GRID) gives the table's candidates, and every candidate has one small case or, where
    no small request reaches it, a large one.  (c) what must be among them."""
    cands, big, tall, cases, probe = tab
    fresh, fresh_big, _ = av.scan_grid(probe)
    assert set(fresh) == set(cands) and fresh_big == big
    small = {case.cand for case in cases}
    assert len(small) == len(cases)
    every = set(cands) | set(big)
    assert small | set(big) == every and small == {c for c in cands if cands[c]}
    print("%d candidates, %d small cases on %d distinct geometries, %d large launches" % (len(every), len(cases), len({c.point for c in cases}), len(av.BIG)))
    has = lambda **kw: any(all(getattr(c, k) == x for k, x in kw.items()) for c in every)
    # both tile pipelines, each for all three source types and both kinds of load; every nCols class of each
    for T in av.TYPES:
        for nr in ("NR4", "NR8"):
            for shape in av.NCOLS:
                assert has(kernel="aai_axis_tile_kernel", T=T, sub=nr, shape=shape), (T, nr, shape)
            for d in (1, -1):
                assert has(kernel="aai_axis_tile_kernel", T=T, sub=nr, dir_b=d), (T, nr, d)
        for nt in (0, 1):
            assert has(kernel="aai_axis_tile_kernel", T=T, sub="NR4", nt=nt), (T, nt)
        # (the issue behind this module asked for both pipelines at both kinds of load; the scan shows one of the four does not exist:
        # windows of five to eight source rows are never disjoint: a ratio between 3 and 4 whose windows are, is lattice-aligned and
        # has windows of at most four rows.  NR8 with nontemporal loads is not a launch.)
        assert has(kernel="aai_axis_tile_kernel", T=T, sub="NR8", nt=0) and not has(kernel="aai_axis_tile_kernel", T=T, sub="NR8", nt=1), T
        # branches A..E (B: below), both kinds of load, every store shape of A in both directions
        for b in "ACDE":
            for nt in (0, 1):
                assert has(kernel="aai_axis_kernel", T=T, sub=b, nt=nt, multi=0), (T, b, nt)
        for b in "CDE":
            assert has(kernel="aai_axis_kernel", T=T, sub=b, multi=1), (T, b)
        for shape in av.A_STORES:
            for d in (1, -1):
                assert has(kernel="aai_axis_kernel", T=T, sub="A", shape=shape, dir_b=d, rows_class="1"), (T, shape, d)
        for kind in ("narrow", "footprint"):
            assert has(kernel="aai_axis_wide_kernel", T=T, sub=kind), (T, kind)
    # branch B, and a second iteration of either register loop: through the large cases only, in both store directions
    b_cands = {c for c in every if c.sub == "B"}
    assert b_cands and all(not cands.get(c) and big.get(c) for c in b_cands), b_cands
    # (both store shapes of B in both directions; two and four outputs per lane -- three: not among the cases, see axis_variants.BIG)
    assert {(c.dir_b, c.shape, c.rows_class) for c in b_cands} == {(1, "4", "n"), (-1, "4", "n"), (1, "1", "n"), (-1, "1", "n"),
                                                                    (0, "", "nq2"), (0, "", "nq4")}, b_cands
    loops = {c for c in every if c.rows_class == "n"}          # ("nq.." of the tile kernel and of branch B is no rows class)
    assert {(c.sub, c.dir_b) for c in loops} == {("A", 1), ("A", -1), ("B", 1), ("B", -1)} and all(c in big for c in loops), loops
    # among the small cases: every right-edge shift, a last workgroup with fewer than four strips and a full one, every nq of the tile kernel
    seen = [av.probe_point(probe, case.point) for case in cases]
    for s in (0, 1, 2, 3):
        for kernel in (1, 2):
            assert any(v.kernel == kernel and v.shifts >> s & 1 for v in seen), (kernel, s)
    assert any(v.kernel == 1 and v.last_wg_short for v in seen) and any(v.kernel == 1 and not v.last_wg_short for v in seen)
    assert any(v.kernel == 1 and v.grid_x > 1 for v in seen) and all(v.grid_y > 1 for v in seen if v.kernel == 2)
    nq = 0
    for v in seen:
        nq |= v.tile_nq
    assert nq == 0b1111, bin(nq)


def test_no_tile_window_is_taller_than_its_pipeline(tab):
    """(d) tile_columns falls back to the plain path for a window of NR source rows or more.  No grid point, no case and no band of a
    case has one: with equal x and y resolutions the launch rules never choose the tile kernel at a ratio that has such windows."""
    cands, big, tall, cases, probe = tab
    assert not tall, tall[:5]
    for case in cases:
        assert not av.probe_point(probe, case.point).tile_tall
        if case.cand.kernel == "aai_axis_tile_kernel":
            for band in av.bands_of(case.dH):
                assert not av.probe_point(probe, case.point, band).tile_tall


def test_bands_of_the_tile_cases_take_the_strip_kernel(tab):
    """What the GPU module's band check relies on: a band of at most 64 dst rows of a 90 / 270 degree tile-kernel case has at most 64
    outputs per strip and takes branch A of the strip kernel (vertical_pass), where the whole image takes finish_rows."""
    cands, big, tall, cases, probe = tab
    n = 0
    for case in cases:
        if case.cand.kernel != "aai_axis_tile_kernel":
            continue
        for band in av.bands_of(case.dH):
            v = av.probe_point(probe, case.point._replace(batch=1), band)
            assert av.KERNELS[v.kernel] == "aai_axis_kernel" and v.branches == 1 and v.max_outputs <= 64, (av.case_id(case), band, v)
            n += 1
    assert n


def test_every_small_case_is_sensitive_to_one_source_element(tab):
    """(e) derived, not measured: smallest non-zero lane weight x smallest non-zero row weight >= 1e-3, so one dropped, doubled or
    misplaced source element (noise in [0.25, 1.25)) moves a pixel by at least 1e-3 x 0.25 / 1.25 = 2e-4 relative, twenty times the
    bar.  The one exception is the wide kernel's footprint of more than 256 x 256 taps (axis_variants.eligible)."""
    cands, big, tall, cases, probe = tab
    for case in cases:
        v = av.probe_point(probe, case.point)
        if case.cand.kernel == "aai_axis_wide_kernel" and case.cand.sub == "footprint":
            assert v.min_lane_w < 1.0 / 256
            continue
        assert v.min_lane_w * v.min_row_w >= av.MIN_WEIGHT, (av.case_id(case), v.min_lane_w, v.min_row_w)
    for name, p in av.BIG.items():
        v = av.probe_point(probe, p)
        assert v.min_lane_w * v.min_row_w >= 0.0625, (name, v)


def test_cpu_replay_of_every_small_case_matches_the_oracle(tab, aai, hostemu, po):
    """(f) the CPU replay of K1 (aai_emu_resample, aai_emu_resample_channels) on every small case's geometry against the oracle:
    within conftest.TOL, exact zeros exact.  (g) the fix-up pass behind K1 recomputes at most 5 % of the dst pixels -- otherwise K1's
    own arithmetic was not what got tested.  The replay is fp32 arithmetic, so cases that differ only in source type share one run."""
    cands, big, tall, cases, probe = tab
    done = {}
    worst, most = 0.0, 0.0
    for case in cases:
        p = case.point
        key = p._replace(T="", batch=0)
        if key in done:
            continue
        done[key] = case
        shape = (p.H, p.W) if p.C == 1 else (p.H, p.W, p.C)
        src = np.random.default_rng(7 + len(done)).random(shape, dtype=np.float32) + np.float32(0.25)
        iso = av.iso_of(p.W, p.H, p.off)
        omode = po.MODE_EXACT if p.mode == av.MODE_AREA else po.MODE_FAST
        planes = [src] if p.C == 1 else [src[:, :, c] for c in range(p.C)]
        gold = [po.oracle_run(omode, np.ascontiguousarray(q, dtype=np.float64), p.ratio, 1.0, iso, p.angle).dst for q in planes]
        gold = gold[0] if p.C == 1 else np.stack(gold, axis=2)
        rq = aai.make_request(p.W, p.H, p.ratio, 1.0, iso, p.angle, mode=p.mode)
        plane_out, axis = hostemu.resample(rq, planes[0])
        fixups = hostemu.aai_emu_axis_fixups()
        assert axis, av.case_id(case)
        if p.C == 1:
            out = plane_out
        else:
            out = np.empty((case.dH, case.dW, p.C), np.float32)
            assert hostemu.aai_emu_resample_channels(ctypes.byref(rq), p.C, src.ctypes.data, out.ctypes.data) == 0, av.case_id(case)
        assert out.shape == gold.shape == ((case.dH, case.dW) if p.C == 1 else (case.dH, case.dW, p.C)), av.case_id(case)
        assert fixups <= 0.05 * case.dW * case.dH, (av.case_id(case), fixups)
        most = max(most, fixups / float(case.dW * case.dH))
        err = float(rel_err(out, gold).max())
        worst = max(worst, err)
        assert err <= TOL, (av.case_id(case), err)
        assert np.array_equal(gold == 0, out == 0), av.case_id(case)
    print("distinct geometries replayed: %d, worst rel err %.2e, largest share of fix-up pixels %.2f %%" % (len(done), worst, 100 * most))
