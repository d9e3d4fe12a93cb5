"""The CPU side of tests/test_grid_carry_gpu.py (no GPU): the limits that file crosses are the sources' own constants; every geometry of
grid_carry_cases.GEOMETRIES crosses the limit it is there for, by the planner's own facts, so that a later change of a constant or of a
launch rule cannot quietly turn a GPU test into a one-launch test; axis_launch_shape (csrc/aai_plan.hpp) covers its rows with a grid of
at most 65535 blocks over a sweep of heights; and the three CPU replays, whose bits are the GPU tests' gold, stay within their own host
tests' bars of the oracle at these heights, at the rows the GPU tests sample."""
import os

import numpy as np
import pytest

import adjoint_half_cases as ac
import axis_variants as av
import grid_carry_cases as gc
import half_cases as hc
import int_cases as ic
from adjoint_columns import comb_gold_pixels
from conftest import TOL, rel_err


@pytest.fixture(scope="module")
def probe(hostemu):
    return av.Prober(hostemu)


def _probe(probe, geo, channels, elem_bytes, height=None):
    H = geo.H if height is None else height
    return probe(geo.W, H, geo.ratio, geo.angle, av.MODE_AREA, ((geo.W - 1) / 2.0 + geo.off[0], (H - 1) / 2.0 + geo.off[1]), channels, elem_bytes, 1)


def test_the_limits_are_the_sources_constants():
    assert gc.csrc_constant("aai_axis_adjoint.hip", "kAxisAdjRows") == gc.AXIS_ADJOINT_ROWS
    assert gc.csrc_constant("aai_adjoint_plain.hip", "kPlainTile") == gc.PLAIN_TILE
    assert gc.csrc_constant("aai_adjoint_multi.hip", "kAdjMultiTile") == gc.PLAIN_TILE
    assert gc.csrc_constant("aai_adjoint_plain.hip", "kScaleRows") == gc.SCALE_ROWS
    assert gc.csrc_constant("aai_engine.hpp", "kMaxGridZ") == gc.GRID_Y
    assert (gc.EDGE_AXIS_ADJOINT, gc.EDGE_PLAIN, gc.EDGE_ROWS4) == (2097120, 1048560, 262140)
    # the converters' grid and the wide kernel's launches: blocks of 4 rows, 65535 of them (the text of the sources)
    narrow = open(os.path.join(gc.CSRC, "aai_axis_narrow.hip")).read()
    assert "std::min((H + 3) / 4, 65535)" in narrow and "y += (int)gridDim.y * 4" in narrow
    assert "kb0 += 65535 * 4" in open(os.path.join(gc.CSRC, "aai_axis.hip")).read()
    assert "kb += gridDim.y * 4" in open(os.path.join(gc.CSRC, "aai_util.hip")).read()


@pytest.mark.parametrize("name", list(gc.GEOMETRIES))
def test_every_geometry_crosses_the_limit_it_is_there_for(aai, hostemu, probe, name):
    geo = gc.GEOMETRIES[name]
    rq = gc.request(aai, name)
    rc, msg, lay = aai.query(rq)
    assert rc == 0, msg
    axis, wide, transposed, strips, most, shared, rowspan, direct = hc.facts(rq)
    rows = geo.H if geo.side == "src" else lay.dst_height
    assert rows > geo.edge + 33, (name, rows, geo.edge)
    if name.startswith("A"):
        assert axis and not wide and geo.H > gc.EDGE_AXIS_ADJOINT and transposed == (geo.angle in (90.0, 270.0))
        assert ((geo.H + gc.AXIS_ADJOINT_ROWS - 1) // gc.AXIS_ADJOINT_ROWS) > gc.GRID_Y        # a second launch of the adjoint launchers
        if name in ("A0", "A180"):
            assert (rowspan, direct, shared) == (2, 1, 0)
        if name in ("A90", "A270", "A11"):
            assert shared
        if name == "A180":
            v = _probe(probe, geo, 1, 4)
            assert (v.sign_a, v.sign_b) == (-1, -1)                       # outBase = (nA - 1) outStrideA + (nB - 1) outStrideB
    elif name == "Wd":
        assert axis and wide and lay.dst_height > gc.EDGE_ROWS4 and lay.kernel == aai._lib.KERNEL_AXIS_WIDE
        assert av.KERNELS[_probe(probe, geo, 1, 4).kernel] == "aai_axis_wide_kernel"
        # ... and with three channels a row of 9 elements: the strip kernel, behind converters whose tail branch runs (9 % 4 = 1)
        assert av.KERNELS[_probe(probe, geo, 3, 4).kernel] == "aai_axis_kernel" and (geo.W * 3) % 4 == 1
    elif name in ("N2", "N2r", "N8", "N8c"):
        elem, channels = {"N2": (2, (1,)), "N2r": (2, (3,)), "N8": (1, (1,)), "N8c": (1, (3,))}[name]
        assert axis and not wide and not transposed and direct
        for C in channels:
            tall, short = _probe(probe, geo, C, elem), _probe(probe, geo, C, elem, height=geo.H // 10)
            assert av.KERNELS[tall.kernel] == "aai_axis_kernel"
            assert tall.nB > gc.GRID_Y * short.rows and tall.rows > short.rows and 1 <= tall.grid_y <= gc.GRID_Y, (name, C, tall.rows, short.rows, tall.grid_y)
            if elem == 1:
                f = ic.facts(rq, C)
                assert f[4] > 64 and ic.direct(rq, C, ic.U8), (name, C, f)       # more than 64 outputs in a strip: u8 stays direct
    elif name in ("R", "Rup", "T"):
        assert not axis and lay.dst_width in ((79,) if name != "T" else (86,)), (name, lay.dst_width)
        if name == "R":
            assert geo.H > gc.EDGE_PLAIN and lay.dst_height > gc.EDGE_PLAIN
        if name == "Rup":
            assert geo.H < gc.EDGE_PLAIN < lay.dst_height                     # only the dst-side loops carry
            assert lay.dst_height > gc.GRID_Y * gc.SCALE_ROWS * 4             # the scale pass: several launches of 65535 blocks of 4 rows
        if name == "T":
            assert geo.H > gc.EDGE_ROWS4 and lay.dst_height > gc.EDGE_ROWS4   # widen (source rows) and store (dst rows) both stride
    elif name == "Z":
        assert axis and not wide and not transposed and lay.dst_height > gc.EDGE_ROWS4
        # an empty entry at the end of the lane table: at a height the emulation affords, the kernels' CPU replay (whose zero pass is
        # the engine's: AxisTables::emptyLane) and the oracle both give a last dst column of exact zeros from an all-ones source
        small = gc.request(aai, name, height=24)
        out, is_axis = hostemu.resample(small, np.ones((24, geo.W), np.float32))
        assert is_axis and out.shape[1] == lay.dst_width
        assert not out[:, -1].any() and out[:, :-1].all()
    else:
        pytest.fail("no assertion for geometry %s" % name)


@pytest.mark.parametrize("channels, W, ratio, outputs", gc.SWEEP_STRIPS, ids=["C%d W%d %g:1" % s[:3] for s in gc.SWEEP_STRIPS])
def test_axis_launch_shape_covers_its_rows_with_one_grid(probe, channels, W, ratio, outputs):
    """axis_launch_shape through the probe: 1 <= gridY <= 65535, rows * gridY >= nB, rows * (gridY - 1) < nB, for nB on both sides of
    65535 r (r = 1 ... 64) and at 2,097,190 and 8,400,000, element sizes 1, 2 and 4, and strips of every class of maxOutputsPerStrip
    that exists (a strip ends at 256 outputs: the up-sampling cases land in the class 129..256)"""
    rows_seen = {elem: set() for elem in gc.SWEEP_ELEM}
    for nb in gc.SWEEP_NB:
        H = nb if ratio == 1.0 else (nb + 1) // 2
        for elem in gc.SWEEP_ELEM:
            v = probe(W, H, ratio, 0.0, av.MODE_AREA, ((W - 1) / 2.0, (H - 1) / 2.0), channels, elem, 1)
            what = (W, H, ratio, channels, elem, v.rows, v.grid_y, v.nB, v.max_outputs)
            assert av.KERNELS[v.kernel] == "aai_axis_kernel" and outputs[0] <= v.max_outputs <= outputs[1], what
            assert v.nB == (nb if ratio == 1.0 else 2 * H), what
            assert 1 <= v.grid_y <= gc.GRID_Y, what
            assert v.rows * v.grid_y >= v.nB and v.rows * (v.grid_y - 1) < v.nB, what
            rows_seen[elem].add(v.rows)
    # the loop under test did run: the tallest launches of every element size have more rows per workgroup than the shortest
    for elem in gc.SWEEP_ELEM:
        assert len(rows_seen[elem]) > 1, (elem, rows_seen[elem])


# ---- the CPU replays at height: the gold of the GPU tests' bit comparisons ---------------------------------------------------------
FORWARD_REPLAYS = ["N2", "A0"]


@pytest.mark.parametrize("name", FORWARD_REPLAYS)
def test_half_replay_stays_within_its_bar_at_height(aai, po, name):
    """half_cases.replay (bits and the fp32 values before the rounding) against the oracle on the widened source: the two bars of
    tests/test_half_host.py, at the rows tests/test_grid_carry_gpu.py samples"""
    geo = gc.GEOMETRIES[name]
    for mode in hc.MODES:
        rq = gc.request(aai, name, mode)
        lay = aai.query(rq)[2]
        rows = gc.forward_rows(lay.dst_height)
        for ht, tname in hc.TYPES:
            src = hc.source_bits(geo.W, geo.H, ht)
            out, pre = hc.replay(aai, rq, ht, src)
            assert not np.isnan(pre).any()                                   # every element written
            gold = gc.oracle_at_rows(po, hc.oracle_mode(po, mode), hc.widen(src, ht), geo, rows, lay.dst_width)
            before = float(rel_err(pre[rows], gold).max())
            after = hc.rounded_excess(hc.widen(out[rows], ht), gold, ht)
            print("half replay %s %s %s, %d rows: before the rounding %.3e, after it %.3e over the bound" % (name, mode, tname, len(rows), before, after))
            assert before <= TOL and after <= 0, (name, mode, tname, before, after)


@pytest.mark.parametrize("name", FORWARD_REPLAYS)
def test_int_replay_stays_within_its_bar_at_height(aai, po, name):
    """int_cases.replay against the oracle per channel: the two bars of tests/test_int_host.py at the sampled rows"""
    geo = gc.GEOMETRIES[name]
    rq = gc.request(aai, name)
    lay = aai.query(rq)[2]
    rows = gc.forward_rows(lay.dst_height)
    for dt, tname in ic.TYPES:
        src = ic.source((geo.W, geo.H), 1, dt, "random")
        out, pre = ic.replay(aai, rq, dt, src)
        assert not np.isnan(pre).any()
        gold = gc.oracle_at_rows(po, po.MODE_EXACT, src[:, :, 0].astype(np.float32), geo, rows, lay.dst_width)
        before = float(rel_err(pre[rows, :, 0], gold).max())
        after = ic.excess(out[rows, :, 0], gold)
        print("int replay %s %s, %d rows: before the conversion %.3e, after it %.3e over the bound" % (name, tname, len(rows), before, after))
        assert before <= TOL and after <= 0, (name, tname, before, after)


@pytest.mark.parametrize("name", FORWARD_REPLAYS)
def test_adjoint_half_replay_stays_within_one_rounding_at_height(aai, po, name):
    """adjoint_half_cases.replay at the boundary source rows against columns of the oracle's matrix (adjoint_columns.comb_gold_pixels on
    the widened gradient): half_cases.rounded_excess <= 0 and exact zeros, the bar of tests/test_adjoint_half_host.py.  Both modes, f16
    and bf16 in fast mode and f16 in area mode: the replay runs the planner's model check on the CPU, which in area mode takes about 3 s
    (N2) and 7 s (A0) per call at these heights, and 0.2 to 2 s in fast mode."""
    geo = gc.GEOMETRIES[name]
    edge = gc.EDGE_AXIS_ADJOINT if geo.H > gc.EDGE_AXIS_ADJOINT else gc.EDGE_ROWS4
    sx, sy = gc.rows_pixels(geo.W, gc.boundary_rows(edge, geo.H), 5)
    for mode, ht, tname in [("fast",) + t for t in ac.TYPES] + [("area",) + ac.TYPES[0]]:
        rq = gc.request(aai, name, mode)
        lay = aai.query(rq)[2]
        g = ac.gradient_bits(lay, 1, ht)
        got = hc.widen(ac.replay(rq, ht, g), ht)[:, :, 0]
        g32 = hc.widen(g[:, :, 0], ht)
        gold, evaluated = comb_gold_pixels(po, hc.oracle_mode(po, mode), rq, lay, lambda dx, dy: g32[dy, dx], sx, sy)
        assert 4 * int((gold != 0).sum()) >= sx.size
        excess = hc.rounded_excess(got[sy, sx], gold, ht)
        print("adjoint replay %s %s %s, %d source pixels, %d oracle dst pixels: excess %.3e" % (name, mode, tname, sx.size, evaluated, excess))
        assert excess <= 0, (name, mode, tname, excess)
        assert np.all(got[sy, sx][gold == 0] == 0.0)
