"""CPU: the wide-pitch case table (tests/wide_pitch.py) is what it claims to be, and the oracle it is judged by would notice one
misaddressed source row.  test_wide_pitch_gpu.py runs the table on the device.

The CPU replays of the quad, wide and cell kernels (tests/emulation: emu_quad_pixel, emu_wide_pixel, emu_cells) are NOT run at a pitch
here: they address the source through virt_offset with a 64-bit stride and restate the kernels' per-pair arithmetic, not their 32-bit
lane offsets (QuadSrc::issue: the 24-bit multiplies, the anchor row, the rebased wave), so at any pitch they compute what they compute
on the tight image and would hold nothing this table is about.  What the CPU can hold of the address regimes is the probe: the
launchers' own predicates (csrc/aai_rot_serve.hpp) and make_quad_map, asked for every case below.
"""
import math

import numpy as np
import pytest

import rot_variants as rv
import wide_pitch as wp


@pytest.fixture(scope="module")
def tab(hostemu):
    return wp.table(hostemu)


def _all_cases(tab):
    probe, fwd, bnd = tab
    return fwd + [c for (_, a, b) in bnd for c in (a, b)]


def test_pitched_probe_agrees_with_the_tight_probe_and_with_the_stated_thresholds(tab):
    """At the image's own row stride the pitched probe names the family aai_emu_rot_variant names (two statements of the precedence,
    held together here and both against aai_last_kernel() on the GPU), reports regime T's fields, and its span / pitch fields flip where
    the header comments say: H x pitch x element size = 2^32, pitch x element size = 2^23."""
    probe, fwd, bnd = tab
    for g in wp.GEOMS + wp.BOUND_GEOMS:
        for T in g.types:
            for H in set(g.heights):
                v = probe(g, H, T, wp.row_elems(g))
                t = probe.tight(g.src_res / g.dst_res, g.angle, g.mode, g.policy, g.C, wp.TYPES[T][1], W=g.W, H=H, iso=wp.iso_of(g, H)) if g.mode in (1, 2) else None
                if t is not None:
                    assert v[:len(rv.FIELDS)] == tuple(t), (g.name, T, H, v, t)
                assert (v.spans_4gib, v.anchorRows, v.rebaseWaves) == (0, 0, 0), (g.name, T, H, v)
                assert v.mul24Ok == 1 and v.fastOk == int(g.C == 1 and T == "f32" and v.scale == 1), (g.name, T, H, v)
    g, T = wp.BY_NAME["quad/17.5"], "u16"
    H = 560
    p4 = -(-(1 << 32) // (H * 2))
    assert (probe(g, H, T, p4 - 1).spans_4gib, probe(g, H, T, p4).spans_4gib) == (0, 1)
    assert (probe(g, H, T, (1 << 22) - 1).mul24Ok, probe(g, H, T, 1 << 22).mul24Ok) == (1, 0)


def test_table_covers_every_family_and_regime_its_grid_can_produce(tab):
    """Every (family, regime) pair the probe produces over the grid -- every geometry x type x pitch class x height -- has a case;
    every (family, type) pair that can span 4 GiB meets G or GP; u8 and u16 meet E31 in every family that takes them; every X case
    names both the family that refuses and the family that takes over, and they differ."""
    probe, fwd, bnd = tab
    have = {(c.family, c.regime) for c in fwd}
    grid = wp.grid(probe)
    assert len(grid) > 300
    want = {(fam, reg) for (g, T, cls, H, pitch, fam, reg, e) in grid}
    assert want <= have, sorted(want - have)
    assert {r for (_, r) in have} >= {"P", "G", "GP", "T+"}
    # (family, type): above 4 GiB at least once
    above = {(c.family, c.T) for c in fwd if c.regime in ("G", "GP")}
    reach = {(fam, T) for (g, T, cls, H, pitch, fam, reg, e) in grid if reg in ("G", "GP")}
    assert reach <= above, sorted(reach - above)
    for T in ("u8", "u16"):
        fams = {fam for (g, Tg, cls, H, pitch, fam, reg, e) in grid if Tg == T and e}
        assert fams <= {c.family for c in fwd if c.T == T and c.e31}, T
    assert any(c.T == "f32" and c.e31 and c.family.startswith("aai_axis") for c in fwd)
    assert any(c.T == "f32" and c.e31 and c.family in ("aai_quad_kernel", "aai_cell_kernel") for c in fwd)
    assert any(c.T == "u8" and c.e31 and c.regime == "T+" for c in fwd)            # 2^31 elements below every 4 GiB switch
    # per family and regime: every quadrant parity the grid has it at (quadrants 1 / 3: the pitch is the stride of virtual X)
    for key in have:
        par = {int(c.geom.angle // 90) % 2 for c in fwd if (c.family, c.regime) == key}
        assert par == {int(g.angle // 90) % 2 for (g, T, cls, H, pitch, fam, reg, e) in grid if (fam, reg) == key}, (key, par)
    for fam in {f for (f, _) in have} - {"aai_axis_tile_kernel"}:              # (the tile kernel IS K1's transposed form)
        assert {int(c.geom.angle // 90) % 2 for c in fwd if c.family == fam} == {0, 1}, fam
    xs = [c for c in _all_cases(tab) if c.x]
    assert xs
    for c in xs:
        assert c.family and c.control and c.family != c.control, c
    # the takeovers the header comments promise: the cell kernel hands pitches of 8 MiB and more to the next fp32 family, interleaved
    # images above 4 GiB go to the double-precision kernels
    assert {(c.control, c.family) for c in xs} >= {("aai_cell_kernel", "aai_quad_kernel"), ("aai_quad_multi_kernel", "fp64"), ("aai_cell_multi_kernel", "fp64")}


def test_boundary_pairs_sit_within_one_element_of_their_bound(tab):
    """The two cases of a pair are one element of pitch apart and differ in the probed field the pair names; the pairs cover the 4 GiB
    threshold, the 8 MiB pitch, cell_can_serve's span bound at a two-row wave with rebased waves on its inner side, and
    quad_can_address's anchor bound for a quad and for a wide geometry with anchor rows on its inner side."""
    probe, fwd, bnd = tab
    names = set()
    for b, inside, at in bnd:
        assert at.pitch - inside.pitch == 1 and (inside.geom, inside.T, inside.H) == (at.geom, at.T, at.H) == (b.geom, b.T, b.H)
        f = wp._field(probe, b.geom, b.H, b.T, b.field)
        assert f(inside.pitch) != f(at.pitch), (b, inside.pitch)
        assert f(inside.pitch) == f(b.lo), b
        vi, va = probe(b.geom, b.H, b.T, inside.pitch), probe(b.geom, b.H, b.T, at.pitch)
        esz = wp.TYPES[b.T][1]
        if b.name == "4GiB":
            assert (vi.spans_4gib, va.spans_4gib) == (0, 1) and b.H * at.pitch * esz >= 1 << 32 > b.H * inside.pitch * esz
        elif b.name == "8MiB":
            assert (vi.mul24Ok, va.mul24Ok) == (1, 0) and at.pitch * esz == 1 << 23
        elif b.name == "cell-span":
            assert vi.spans_4gib and vi.rebaseWaves == 1 and vi.cell_wave_rows == 2 and inside.family == "aai_cell_kernel" and at.x, (vi, at)
            assert at.pitch * esz < 1 << 23                         # (the span bound, not the pitch bound, refuses)
            assert vi.dH >= 34                                      # (a wave walks more than 32 cell rows)
        elif b.name == "anchor":
            assert vi.spans_4gib and vi.anchorRows > 0 and inside.family in ("aai_quad_kernel", "aai_wide_kernel") and at.family == "fp64", (vi, at)
            assert b.H > 2 * vi.anchorRows                          # (the image is taller than the rows a wave may span)
        names.add((b.name, inside.family))
    assert {n for (n, _) in names} == {"4GiB", "8MiB", "cell-span", "anchor"}
    assert ("anchor", "aai_quad_kernel") in names and ("anchor", "aai_wide_kernel") in names


def test_every_case_fits_the_arena(tab, hostemu):
    probe, fwd, bnd = tab
    for c in _all_cases(tab):
        g = c.geom
        assert wp.row_elems(g) <= wp.MAX_ROW and c.H <= wp.MAX_H, c
        assert c.pitch >= wp.row_elems(g) + wp.GUARD
        assert wp.extent_bytes(c.H, wp.row_elems(g), c.pitch, wp.TYPES[c.T][1]) <= wp.ARENA_CAP, wp.case_id(c)
    s, d = wp.source_arena_bytes(hostemu), wp.dst_arena_bytes(hostemu)
    assert s <= wp.ARENA_CAP and d <= wp.ARENA_CAP
    # the GPU module holds one arena at a time where both would pass the joint cap (its Arenas class frees the other)
    assert max(s, d) <= wp.ARENA_CAP_BOTH
    for name, T, cls in wp.DST_CASES:
        g = wp.geom_by_name(name)
        dH, dW, drow = wp.dst_size(probe, g, g.heights[0])
        pitch = wp.dst_pitch_for(cls, dH)
        assert dH * pitch * 4 >= 1 << 32 and (cls != "E31" or dH * pitch >= 1 << 31), (name, dH, pitch)
    assert {"k1/90", "k1-empty/0", "k1-fixup/0", "bilinear/17.5", "bicubic/300", "knife-quad/30"} <= {n for (n, _, _) in wp.DST_CASES}
    assert sum(1 for (_, _, cls) in wp.DST_CASES if cls == "E31") >= 2
    for name, T in wp.BATCH_CASES:
        assert wp.batch_apart(T, "src") >= ((1 << 32) if T == "u8" else (1 << 31))


BASES = []
for _geom in wp.GEOMS + wp.BOUND_GEOMS:
    if _geom.name.split("/")[0] not in BASES:
        BASES.append(_geom.name.split("/")[0])


@pytest.mark.parametrize("base", BASES)
def test_oracle_notices_two_swapped_source_rows(tab, po, base):
    """Derived sensitivity, on the oracle alone: for every (geometry, type, height) a forward case uses, the source with two adjacent
    rows swapped moves at least one pixel of the oracle's output by 100 x the bar -- so a kernel that reads one row from the wrong
    address cannot pass.  The pair of rows: the first of ceil(ratio) + 1 consecutive pairs from the middle of the image that does
    (rows that fall into one dst pixel with full weight change nothing: area averages do not see their order)."""
    keys = []
    for c in _all_cases(tab):
        k = (c.geom, c.T, c.H)
        if c.geom.name.split("/")[0] == base and k not in keys:
            keys.append(k)
    assert keys
    for g, T, H in keys:
        src = wp.source(g, T, H)
        gold = wp.gold(po, g, H, src)
        bound = wp.bar(g, T)[1]
        best = 0.0
        for k in range(int(math.ceil(g.src_res / g.dst_res)) + 1):
            r = H // 2 + k
            swapped = src.copy()
            swapped[[r, r + 1]] = swapped[[r + 1, r]]
            moved = float(wp.scaled_error(g, T, wp.gold(po, g, H, swapped).astype(np.float32), gold).max())
            best = max(best, moved)
            if moved >= 100 * bound:
                break
        assert best >= 100 * bound, (g.name, T, H, best, bound)
