"""CPU (no GPU): the case table of tests/rot_variants.py -- two geometries per template instantiation the rotated-lattice launchers
can choose, each next to the boundary of its window -- is what it claims to be, and the CPU replay of the fp32 formulations
(tests/emulation) answers every one of its geometries like the oracle does.  test_rot_variants_gpu.py runs the same table on the MI355X."""
import numpy as np
import pytest

import rot_variants as rv
from conftest import TOL, rel_err


@pytest.fixture(scope="module")
def tab(hostemu):
    return rv.table(hostemu)


def test_each_case_selects_the_variant_it_was_built_for(tab):
    """(a) the probe, asked about the case as it will be launched (its canvas, isocenter, quadrant, policy bits, type and channels),
    reports the case's candidate; the case has the canvas and the isocenter the table promises."""
    cands, cases, probe = tab
    assert len(cases) == 2 * len(cands)
    for k, case in enumerate(cases):
        c = case.cand
        found = rv.hosted(probe, case.ratio, case.angle, case.mode, c.T, c.C, W=case.W, H=case.H, iso=case.iso)
        assert found.get(c) == (case.policy, case.dispatched), (rv.case_id(case), found)
        v = probe(case.ratio, case.angle, case.mode, case.policy, c.C, rv.TYPES[c.T][1], W=case.W, H=case.H, iso=case.iso)
        assert (rv.FAMILIES[v.family] == c.family) == case.dispatched, (rv.case_id(case), v)
        lo, hi = rv.TEMPLATE_WIN[c.family]
        assert lo <= c.win <= hi, rv.case_id(case)              # an instantiation the source compiles
        # two 16 x 16 tiles per axis, one cell strip (63 / 31 columns) and one 64-column row wave crossed; about 70 x 40
        assert 66 <= case.dW <= 100 and 34 <= case.dH <= 100 and (case.dW, case.dH) == (v.dW, v.dH), (rv.case_id(case), case.dW, case.dH)
        assert int(case.angle // 90) == k % 4                   # the quadrants round-robin
        for iso in case.iso:
            assert 0.1 < (2.0 * iso) % 1.0 < 0.9                # off the lattice and off its half points
    # every candidate has one case 0.001 inside each end of its region; nearly all of those ends are window thresholds
    kinds = [case.boundary for case in cases]
    assert kinds.count("window") >= 0.95 * len(cases), {k: kinds.count(k) for k in set(kinds)}


def test_case_table_covers_the_candidate_set_exactly(tab):
    """(d) the candidates are those of a scan of the whole grid (rot_variants.GRID), and the cases' candidates are exactly those:
    each twice (enter, leave)."""
    cands, cases, probe = tab
    fresh = rv.scan_grid(probe)
    assert set(fresh) == set(cands)
    per = {}
    for case in cases:
        per.setdefault(case.cand, []).append(case.which)
    assert set(per) == set(cands) and all(sorted(w) == ["enter", "leave"] for w in per.values())
    # plain fp32 requests: the 70-odd (family, WIN, SCALED / WR, HP, PARTS) combinations, every family among them
    plain = {c for c in cands if c.T == "f32" and c.C == 1}
    assert {c.family for c in plain} == {"aai_quad_kernel", "aai_quad_fast_kernel", "aai_cell_kernel", "aai_wide_kernel", "aai_wide_fast_kernel"}
    assert 70 <= len(plain) <= 90, len(plain)
    # only interleaved candidates can be kept from their family; NOT_DISPATCHED lists exactly those, each with the family the
    # probe says serves the request instead
    kept = {c for c in cands if not cands[c][2]}
    assert all(c.C > 1 for c in kept)
    assert {(c.family, c.T, c.C, c.win) for c in kept} == set(rv.NOT_DISPATCHED)
    assert not any((c.family, c.T, c.C, c.win) in rv.NOT_DISPATCHED for c in cands if cands[c][2])
    for case in cases:
        if not case.dispatched:
            c = case.cand
            v = probe(case.ratio, case.angle, case.mode, case.policy, c.C, rv.TYPES[c.T][1], W=case.W, H=case.H, iso=case.iso)
            assert rv.FAMILIES[v.family] == rv.NOT_DISPATCHED[(c.family, c.T, c.C, c.win)][1], (rv.case_id(case), v)
    # plain images: the three source types have the same candidates
    assert {c._replace(T="") for c in cands if c.C == 1 and c.T == "u8"} == {c._replace(T="") for c in cands if c.C == 1 and c.T == "f32"}
    assert {c._replace(T="") for c in cands if c.C == 1 and c.T == "u16"} == {c._replace(T="") for c in cands if c.C == 1 and c.T == "f32"}


def test_cpu_replay_of_every_case_matches_the_oracle(tab, aai, hostemu, po):
    """(b) every case's geometry through the CPU replay of its formulation (cell families: aai_emu_use_cell, the others:
    aai_emu_use_quad, which replays the quad, fast and wide kernels) against the oracle: within conftest.TOL, exact zeros exact.
    (c) and the double-precision pass gets at most 5 % of the dst pixels -- otherwise the fp32 window was not what got tested.
    The replay is fp32 arithmetic on one plane, so cases that differ only in source type or channel count share one run."""
    cands, cases, probe = tab
    done = {}
    worst = 0.0
    for case in cases:
        cell = case.cand.family.startswith("aai_cell")
        key = (cell, case.mode, case.W, case.H, case.ratio, case.iso, case.angle)
        if key in done:
            continue
        done[key] = case
        src = np.random.default_rng(7 + len(done)).random((case.H, case.W), dtype=np.float32) + np.float32(0.25)
        gold = po.oracle_run(po.MODE_EXACT if case.mode == rv.MODE_AREA else po.MODE_FAST, src.astype(np.float64), case.ratio, 1.0, case.iso, case.angle).dst
        rq = aai.make_request(case.W, case.H, case.ratio, 1.0, case.iso, case.angle, mode=case.mode)
        hook = hostemu.aai_emu_use_cell if cell else hostemu.aai_emu_use_quad
        hook(1)
        try:
            out, axis = hostemu.resample(rq, src)
        finally:
            hook(0)
        fp32, fp64 = hostemu.quad_stats()
        assert not axis and out.shape == gold.shape == (case.dH, case.dW), rv.case_id(case)
        assert fp32 > 0 and fp64 <= 0.05 * out.size, (rv.case_id(case), fp32, fp64, out.size)
        err = float(rel_err(out, gold).max())
        worst = max(worst, err)
        assert err <= TOL, (rv.case_id(case), err)
        assert np.array_equal(gold == 0, out == 0), rv.case_id(case)
    print("distinct geometries replayed: %d, worst rel err %.2e" % (len(done), worst))
