"""CPU: the wide-pitch table of the typed entries (tests/wide_pitch_typed.py) is what it claims to be -- what it reaches is derived from
the probes' facts, every pitch is in its class, every view fits the arena --, the CPU replays of its new tall geometries stay within
the typed host tests' own bounds against the oracle, and a replay notices two swapped rows of its input.  test_wide_pitch_typed_gpu.py
then runs the table on the device with bit comparisons only.
"""
import math

import numpy as np
import pytest

import adjoint_columns as acol
import convert_cases as cc
import half_cases as hc
import half_interleaved_cases as hic
import int_cases as ic
import wide_pitch as wp
import wide_pitch_typed as wt

FORWARD_ENTRIES = ("half", "half-il", "int", "convert")
NARROW = ("half", "half-il", "int")


@pytest.fixture(scope="module")
def rows(aai):
    return wt.rows(aai)


def _configs(rows, direct=None, entries=wt.ENTRIES):
    """the distinct configurations of the table's rows, in table order"""
    out = []
    for r in rows:
        if r.config.entry in entries and (direct is None or r.direct == direct) and r.config not in out:
            out.append(r.config)
    return out


# ---- what the table reaches ---------------------------------------------------------------------------------------------------------
def test_table_reaches_every_form_of_the_direct_kernels(aai, rows):
    """From the probes' facts (convert_cases.facts: strips, outputs per strip, shared rows, the two flips), in the manner of
    test_convert_host.test_case_table_reaches_every_branch: a pruned table cannot silently lose a form."""
    seen = {k: set() for k in ("half", "channels", "narrow-mode", "narrow-shared", "narrow-up", "convert-form", "convert-small", "convert-mode", "convert-shared",
                               "convert-up", "convert-types", "adjoint")}
    for c in _configs(rows, direct=True):
        f = wt.route_facts(aai, c)
        lay = aai.query(wt.request(aai, c))[2]
        W, H = wt.geometry(c)[:2]
        if c.entry == "adjoint":
            assert f[0] == 1 and lay.quadrant == int(c.angle // 90), (c, f)
            seen["adjoint"].add((lay.quadrant, c.C))
            continue
        # a direct row of a forward entry: the strip form, not transposed, at most 256 outputs per strip, both flips together
        assert (f[0], f[1], f[2], f[7]) == (1, 0, 0, 1) and f[4] <= 256 and f[8] == f[9], (c, f)
        small, flip, shared, up = f[4] <= 64, f[8], f[5], lay.dst_height > H
        if c.entry in NARROW:
            if c.C == 1 and c.entry != "int":
                seen["half"].add((small, flip))                  # the pair store (at most 64), four per lane; forwards and backwards
            if c.C > 1:
                seen["channels"].add((c.C, small, flip))         # the quad store / four per lane; packed (0 degrees), scattered (180)
            seen["narrow-mode"].add(c.mode); seen["narrow-shared"].add(shared); seen["narrow-up"].add(up)
        else:
            seen["convert-form"].add((c.C > 1, wt.planar(c), flip)); seen["convert-small"].add(small); seen["convert-mode"].add(c.mode)
            seen["convert-shared"].add(shared); seen["convert-up"].add(up)
            seen["convert-types"].add((c.T, c.out, c.layout))
    both = {(s, f) for s in (True, False) for f in (0, 1)}
    assert seen["half"] == both, seen["half"]
    assert {(s, f) for (C, s, f) in seen["channels"]} == both and {C for (C, _, _) in seen["channels"]} >= {3, 4}, seen["channels"]
    for C in (3, 4):
        assert {f for (Cc, _, f) in seen["channels"] if Cc == C} == {0, 1}, (C, seen["channels"])
    for k in ("narrow", "convert"):
        assert seen[k + "-mode"] == {"area", "fast"} and seen[k + "-shared"] == {0, 1} and seen[k + "-up"] == {True, False}, (k, seen)
    assert seen["convert-small"] == {True, False}
    assert seen["convert-form"] == {(False, False, 0), (False, False, 1), (True, False, 0), (True, False, 1), (True, True, 0), (True, True, 1)}, seen["convert-form"]
    # every (source type, output type, layout) has a direct row: each output type in each layout, both source types in each layout
    assert seen["convert-types"] == {(s, o, l) for s in ("u8", "u16") for o in ("f32", "f16", "bf16") for l in ("nhwc", "nchw")}, seen["convert-types"]
    assert seen["adjoint"] == {(q, C) for q in range(4) for C in (1, 3)}, seen["adjoint"]
    # the integer entry's direct rows have both element types
    assert {c.T for c in _configs(rows, direct=True, entries=("int",))} == {"u8", "u16"}
    assert {c.T for c in _configs(rows, direct=True, entries=("half", "half-il"))} == {"f16", "bf16"}


def test_table_reaches_every_forwarding_class(aai, rows):
    """per forward entry: a transposed plan (90 degrees: the strip form refuses it), a general rotation, for the integer and convert
    entries a sampler mode and a class that the strip form serves and the measured table forwards; the half adjoint's one forwarding
    class -- a single channel, up-sampling, 90 degrees"""
    for entry in FORWARD_ENTRIES:
        kinds = set()
        for c in _configs(rows, direct=False, entries=(entry,)):
            f = wt.route_facts(aai, c)
            if c.mode == "bilinear":
                kinds.add("sampler")
            elif not f[0]:
                kinds.add("rotation")
            elif f[2]:
                kinds.add("transposed")
            elif f[7]:
                kinds.add("measured")
                assert f[4] <= 64 or entry == "convert", (c, f)
        want = {"transposed", "rotation"} | ({"sampler", "measured"} if entry in ("int", "convert") else set())
        assert kinds >= want, (entry, kinds)
    assert any(c.T == "u8" and wt.route_facts(aai, c)[4] <= 64 and wt.route_facts(aai, c)[7] for c in _configs(rows, direct=False, entries=("int",)))
    fwd = _configs(rows, direct=False, entries=("adjoint",))
    assert fwd
    for c in fwd:
        lay = aai.query(wt.request(aai, c))[2]
        W, H = wt.geometry(c)[:2]
        assert c.C == 1 and lay.quadrant in (1, 3) and lay.dst_width * lay.dst_height > W * H, c


def test_every_kernel_meets_every_side_it_touches(rows):
    """(kernel family, side) pairs: the direct kernels on the side read and the side written (the convert kernel on a plane row too), the
    converters of the forwarding routes on the side they touch -- with a batch row each"""
    have = {}
    for r in rows:
        c = r.config
        read = r.side.endswith("src")
        if r.direct:
            fam = {"half": "narrow", "half-il": "narrow", "int": "narrow", "convert": "convert", "adjoint": "adjoint"}[c.entry]
        elif read:
            fam = "widen" if c.entry in ("half", "half-il", "adjoint") else "fp32-entry"
        else:
            fam = "convert-store" if c.entry == "convert" else "narrow-store"
        have.setdefault(fam, set()).add((r.side, r.cls))
    for fam in ("narrow", "convert", "adjoint"):
        assert have[fam] >= {("src", "G"), ("src", "GP"), ("dst", "G"), ("batch-src", "E31"), ("batch-dst", "E31")}, (fam, have[fam])
    assert ("src", "E31") in have["narrow"] and ("src", "E31") in have["convert"] and ("src", "E31") in have["fp32-entry"]
    assert have["widen"] >= {("src", "G"), ("src", "GP"), ("batch-src", "E31")}, have["widen"]
    assert have["fp32-entry"] >= {("src", "G"), ("src", "GP"), ("batch-src", "E31")}, have["fp32-entry"]
    assert have["narrow-store"] >= {("dst", "G"), ("batch-dst", "E31")} and have["convert-store"] >= {("dst", "G"), ("batch-dst", "E31")}, have
    assert ("plane", "E31") in have["convert"] and ("plane", "E31") in have["convert-store"]
    assert ("dst", "E31") in have["convert"] and ("dst", "E31") in have["convert-store"]            # fp32 out: 2^31 elements
    # the engine's advances to a second round of launches: each direct kernel's on both sides, the forwarding routes' on both sides
    for fam in ("narrow", "convert", "adjoint", "widen", "narrow-store", "convert-store"):
        assert have[fam] & {("grid-src", "E31"), ("grid-dst", "E31")}, (fam, have[fam])
    for fam in ("narrow", "convert", "adjoint"):
        assert have[fam] >= {("grid-src", "E31"), ("grid-dst", "E31")}, (fam, have[fam])
    # every entry has each side on both routes
    for entry in wt.ENTRIES:
        for direct in (True, False):
            sides = {(r.side, r.cls) for r in rows if r.config.entry == entry and r.direct == direct}
            # (GP asks for 4 GiB at 8 MiB a row, 512 rows: the gdst of the half adjoint's forwarding class -- transposed -- has 200)
            assert sides >= {("src", "G"), ("dst", "G")} | (set() if (entry, direct) == ("adjoint", False) else {("src", "GP")}), (entry, direct, sides)
    assert len({wt.row_id(r) for r in rows}) == len(rows)


# ---- pitch classes and the arena --------------------------------------------------------------------------------------------------------
def test_every_pitch_is_in_its_class_and_every_view_fits_the_arena(aai, rows):
    for r in rows:
        im = wt.images(aai, r.config)
        p = wt.placement(im, r)
        esz = wt.ESZ[p.T]
        what = wt.row_id(r)
        # at most 640 x 1100 elements (the images of a transposed quadrant lie on their side)
        assert min(p.row, p.rows) <= wp.MAX_ROW and max(p.row, p.rows) <= wp.MAX_H and p.pitch >= p.row + wp.GUARD, (what, p)
        assert wt.extent_bytes(p) <= wp.ARENA_CAP, (what, wt.extent_bytes(p))
        if r.side in ("src", "dst"):
            assert p.pitch == r.pitch and p.images == 1
            last = (p.planes * p.rows - 1) * p.pitch            # where the last row starts, in elements
            beyond = wt.rows_beyond(r, p)
            assert 2 <= beyond < p.planes * p.rows, (what, beyond)
            if r.cls == "G":
                assert last * esz >= 1 << 32 and (esz != 2 or last >= 1 << 31), (what, last)
                if r.side == "src" and r.config.entry != "adjoint":
                    assert p.pitch * esz < 1 << 23, (what, p.pitch)          # below the pitch at which the forwarded fp32 entry changes form
            elif r.cls == "GP":
                assert p.pitch * esz >= 1 << 23 and last * esz >= 1 << 32, (what, p.pitch)
            else:
                assert r.cls == "E31" and last >= 1 << 31, (what, last)
                assert (p.T, r.side) in (("u8", "src"), ("f32", "dst")), what
                if p.T == "u8":
                    assert wt.extent_bytes(p) < 1 << 32, (what, last)        # 2^31 elements below 4 GiB
        elif r.side == "plane":
            assert p.planes > 1 and p.pitch == p.row + wp.GUARD and p.plane >= 1 << 31 and p.plane >= p.rows * p.pitch, (what, p)
            assert (p.planes, esz) in ((2, 4), (3, 2)), (what, p)
        elif r.side.startswith("grid"):
            # the engine's second round of launches starts at image 65535 (what grid.z carries): beyond 2^31 elements
            assert p.images == wt.GRID_IMAGES > 65535 and p.pitch == p.row + wp.GUARD and 65535 * p.image >= 1 << 31, (what, p)
            assert p.image >= p.planes * p.plane and p.image % 2 == 1
        else:
            assert p.images == 2 and p.pitch == p.row + wp.GUARD and p.image >= 1 << 31, (what, p)
            assert p.image >= (1 << 32 if (p.T == "u8" and r.side == "batch-src") else 1 << 31)
            assert p.image >= p.planes * p.plane
    s, d = wt.arena_bytes(aai, "src"), wt.arena_bytes(aai, "dst")
    assert 0 < s <= wp.ARENA_CAP and 0 < d <= wp.ARENA_CAP and s + d <= wp.ARENA_CAP_BOTH, (s, d)


# ---- the new geometries against the oracle -----------------------------------------------------------------------------------------------
def _adjoint_excess(aai, po, c, got_bits):
    """The half-adjoint host test's bound (half_cases.rounded_excess against the oracle's W^T g), at the source pixels of comb images
    (tests/adjoint_columns.py: the oracle's own columns at sizes where its matrix is out of reach), first and last channel."""
    W, H, sr, dr, iso, ang = wt.geometry(c)
    rq = wt.request(aai, c)
    lay = aai.query(rq)[2]
    ht = wt.HT[c.T]
    g = hc.widen(wt.read_image(aai, c).reshape(lay.dst_height, lay.dst_width, c.C), ht).astype(np.float64)
    got = hc.widen(got_bits.reshape(H, W, c.C), ht)
    pitch = acol.comb_pitch(lay, ang)
    worst = -np.inf
    for ch in sorted({0, c.C - 1}):
        sx, sy, gold = acol.comb_cases(po, hc.oracle_mode(po, c.mode), W, H, sr, dr, iso, ang, 0, g[:, :, ch], acol.edge_phases(W, H, pitch), pitch)
        assert sx.size >= W * H // (pitch * pitch)
        worst = max(worst, hc.rounded_excess(got[sy, sx, ch], gold, ht))
        assert np.all(got[sy, sx, ch][gold == 0] == 0.0)
    return worst


@pytest.mark.parametrize("entry", wt.ENTRIES)
def test_replays_of_the_tall_geometries_stay_within_their_entrys_bound(aai, po, rows, entry):
    """every configuration with a direct row: the replay the GPU module compares bits with, against the oracle per channel, within the
    bound of the entry's own host test -- hc.rounded_excess (half, half adjoint), ic.excess, cc.excess"""
    configs = _configs(rows, direct=True, entries=(entry,))
    assert configs
    for c in configs:
        g = wt.geometry(c)
        W, H = g[:2]
        img = wt.read_image(aai, c)
        out = wt.replay(aai, c, img)
        if entry == "adjoint":
            over = _adjoint_excess(aai, po, c, out)
        else:
            src = img.reshape(H, W, c.C)
            if entry in ("half", "half-il"):
                gold = hic.oracle(po, g, c.mode, src, wt.HT[c.T])
                over = hc.rounded_excess(hc.widen(out.reshape(gold.shape), wt.HT[c.T]), gold, wt.HT[c.T])
                assert (out != 0xffff).all()
            else:
                gold = ic.oracle(po, g, c.mode, src)
                if entry == "int":
                    over = ic.excess(out.reshape(gold.shape), gold)
                else:
                    scale, offset = wt.conversion(c)
                    ot, lay = wt.OT[c.out], wt.LAY[c.layout]
                    hwc = cc.to_hwc(out.reshape(cc.out_shape(gold.shape[0], gold.shape[1], c.C, lay)), lay)
                    over = cc.excess(cc.as_float(hwc, ot), gold, scale, offset, ot)
        print("%-48s %.3e over its bound" % (wt.config_id(c), over))
        assert over <= 0, (wt.config_id(c), over)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", wt.ENTRIES)
def test_replay_notices_two_swapped_rows(aai, rows, entry):
    """the first configuration of the entry with a direct row: the image read with two adjacent rows swapped changes the replay's bits, so
    the GPU module's bit comparison notices a row read from the wrong address.  The pair: the first of ceil(ratio) + 1 consecutive
    pairs from the middle of the image that does (rows that fall into one window with the same weight change a sum's order only)."""
    c = _configs(rows, direct=True, entries=(entry,))[0]
    img = wt.read_image(aai, c)
    want = wt.replay(aai, c, img)
    s = wt.SHAPES[c.shape]
    for k in range(int(math.ceil(max(s.src_res / s.dst_res, 1.0))) + 1):
        r = img.shape[0] // 2 + k
        swapped = img.copy()
        swapped[[r, r + 1]] = swapped[[r + 1, r]]
        changed = int((wt.replay(aai, c, swapped) != want).sum())
        if changed:
            break
    print("%s: rows %d / %d swapped: %d elements change" % (wt.config_id(c), r, r + 1, changed))
    assert changed >= min(img.shape[1], want.shape[1]) // 2, (wt.config_id(c), changed)
