"""CPU (no GPU): the table of tests/value_domain.py -- signed, wide-range and non-finite data through every kernel family -- checked
against the oracle alone, and run through the CPU replays of the kernels (tests/emulation: K1, the fp32 quad / fast / wide and cell
formulations, the double-precision arithmetic, every adjoint family).  test_value_domain_gpu.py runs the same table on the MI355X.
The samplers have no forward replay; their cases are checked on the device only."""
import ctypes

import numpy as np
import pytest

import value_domain as vd


@pytest.fixture(scope="module")
def fwd(aai, hostemu, knife_golden):
    return vd.forward_cases(aai, hostemu, knife_golden[1])


def _replay(aai, hostemu, c):
    """run(src) -> dst through the replay the case names"""
    rq = vd.fwd_request(aai, c)
    rc, msg, lay = aai.query(rq)
    assert rc == 0, msg

    def plane(src):
        hook = {"quad": hostemu.aai_emu_use_quad, "cell": hostemu.aai_emu_use_cell}.get(c.replay)
        if hook:
            hook(1)
        try:
            out, axis = hostemu.resample(rq, src)
        finally:
            if hook:
                hook(0)
        assert axis == (c.replay == "axis"), c.name
        return out

    def run(src):
        src = np.ascontiguousarray(src, dtype=np.float32)
        if c.C == 1:
            return plane(src)
        if c.replay == "axis":
            out = np.full((lay.dst_height, lay.dst_width, c.C), -1.0, np.float32)
            assert hostemu.aai_emu_resample_channels(ctypes.byref(rq), c.C, src.ctypes.data, out.ctypes.data) == 0, c.name
            return out
        return np.stack([plane(np.ascontiguousarray(src[:, :, k])) for k in range(c.C)], axis=2)      # (the replay is one plane's arithmetic)
    return run


def test_the_table_is_what_it_claims_to_be(aai, po, fwd):
    """oracle only: every locality case has a non-empty support, every "empty border" case an all-zero oracle row / column, and the
    checker image at an even integer ratio averages to exactly 0 under a magnitude of exactly 1: a kernel that passes there sums."""
    borders = {}
    for c in fwd:
        lay, pitch, phases = vd.fwd_phases(aai, c)
        assert c.W <= 128 and c.H <= 128 or c.name.startswith("k1 branch"), c.name      # (the strip-branch shapes are the axis table's)
        masks = vd.comb_masks(c.W, c.H, pitch, phases)
        assert any((vd.oracle_forward(po, c, m.astype(np.float64)) != 0).any() for m in masks), c.name
        if c.border:
            assert vd.empty_border(vd.oracle_forward(po, c, np.ones((c.H, c.W))), c.border) is not None, c.name
            if c.kernel.startswith("aai_axis") and c.C == 1 and c.T == "f32" and c.via == "host":
                borders.setdefault((c.ang, c.border), c)
    assert set(borders) == {(a, k) for a in (0.0, 90.0, 180.0, 270.0) for k in ("row", "col")}
    c = vd._fwd("checker 4:1", "aai_axis_kernel", 32, 24, 4, 1, 0.0, replay="axis")
    chk = vd.image("checker", c.H, c.W).astype(np.float64)
    gold, mag = vd.oracle_forward(po, c, chk), vd.oracle_forward(po, c, np.abs(chk))
    assert gold.shape == (6, 8) and np.all(gold[1:-1, 1:-1] == 0) and np.all(mag[1:-1, 1:-1] == 1)
    for a in vd.adjoint_cases():
        M = vd.adjoint_matrix(po, a)
        rc, msg, lay = aai.query(vd.adj_request(aai, a))
        unread = 0
        for m in vd.dst_combs(lay.dst_width, lay.dst_height):
            unread += int((~(M[m.ravel()] != 0).any(1)).sum())
        assert (M != 0).any() and ("empty" not in a.name or unread > 0), (a.name, unread)


def test_replays_on_finite_signed_data(aai, po, hostemu, fwd):
    worst = {}
    for c in fwd:
        if c.replay is None:
            continue
        err = vd.check_forward_finite(po, aai, c, _replay(aai, hostemu, c))
        worst[c.replay] = max(worst.get(c.replay, 0.0), err)
    for k, v in sorted(worst.items()):
        print("replay %-5s worst magnitude-scaled error %.2e" % (k, v))


@pytest.mark.parametrize("family", ["axis", "quad", "cell", "f64"])
def test_replays_keep_non_finite_values_local(aai, po, hostemu, fwd, family):
    runs = cover = 0
    for c in fwd:
        if c.T != "f32" or c.replay != family or vd.not_local(c):
            continue
        r, n, excused = vd.check_forward_locality(po, aai, c, _replay(aai, hostemu, c))
        assert excused == 0
        runs, cover = runs + r, cover + n
    assert runs > 0
    print("replay %s: %d poisoned runs, %d support pixels, 0 excused" % (family, runs, cover))


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.xfail(strict=True, raises=AssertionError, reason=r)) for n, r in vd.NOT_LOCAL_CASES])
def test_replays_of_the_cases_left_as_they_are(aai, po, hostemu, fwd, name):
    """one item per case of value_domain.NOT_LOCAL_CASES: expected to fail on a leak, and on nothing else"""
    (c,) = [c for c in fwd if c.name == name]
    run = _replay(aai, hostemu, c)
    run(vd.image("normal", c.H, c.W))
    try:
        vd.check_forward_locality(po, aai, c, run)
    except AssertionError as e:
        if "non-finite where the oracle has no weight" not in str(e):
            raise RuntimeError("failed, but not on a leak: %s" % (e,))           # (not the expected failure)
        raise


ADJ = vd.adjoint_cases()


@pytest.mark.parametrize("case", ADJ, ids=[a.name for a in ADJ])
def test_adjoint_replays(aai, po, case):
    run = vd.adjoint_replay(aai, case)
    worst = vd.check_adjoint_finite(po, aai, case, run)
    runs, cover, unread = vd.check_adjoint_locality(po, aai, case, run)
    print("adjoint replay %s: worst magnitude-scaled error %.2e; %d poisoned runs, %d support pixels, %d poisoned dst pixels no source pixel reads"
          % (case.name, worst, runs, cover, unread))
