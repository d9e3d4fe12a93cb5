"""Signed, wide-range and non-finite data through every kernel family: images, the two checks and the case table shared by
test_value_domain_host.py (CPU replays of the kernels, tests/emulation) and test_value_domain_gpu.py (the C ABI on the MI355X).

Every expected value and mask comes from the CPU oracle (oracle/aai_oracle.c), from test_adjoint_host.oracle_matrix, or, for the
samplers' tap windows, from conftest.sample_points -- never from the library, its replay or a device run.

Finite data.  A result is linear in the data, out = sum w_i v_i, so a kernel whose weights are right to a relative eps is off by at most
eps sum w_i |v_i|.  Hence, per pixel,

    |got - oracle(src)| <= TOL max(oracle(|src|), 1e-3 max|src|)

with conftest.TOL and the project's floor for typed sources; on non-negative data this is rel_err <= TOL as the suite asserts it
elsewhere.  Where oracle(|src|) == 0 (a dst pixel off the image) got == 0 is required (compared with ==: 0 x negative is -0.0).  For
the adjoints gold = W^T g and the magnitude is |W|^T |g| (the bicubic W has negative lobes); the floor is 1e-3 of the largest
magnitude, the adjoint tests' own convention (a column of W does not add up to 1, so max|g| is not the value scale there).
Magnitudes up to 1e30: beyond that the fp32 sums of value x area over a window can overflow.

Non-finite data.  A NaN / +Inf / -Inf at a source pixel (a dst pixel of the gradient, for the adjoints) reaches exactly the outputs that
have a non-zero weight on it: with `support` = oracle(0/1 image of the poisoned pixels) != 0 the test requires
~isfinite(got) == support, and outside the support the bits of the run with the poisoned pixels set to 0.  The poisoned pixels are
combs (pitch: adjoint_columns.comb_pitch, phases: adjoint_columns.edge_phases -- image corners, the 15 / 16 / 17 tile edges, the last
two rows and columns), one comb and one value per run.  Samplers: a tap of weight 0 still belongs to the tap window
(fmaf(v10 - v00, 0, v00)), so non-finite is required where oracle(comb) != 0, allowed where the clamped 2 x 2 / 4 x 4 tap window around
floor(sample point) holds a poisoned pixel, and forbidden everywhere else.

EXCUSED: a grazing pair the oracle weighs below 1e-6 of the pixel's weight sum and a kernel drops may be excused, by case name, with
a count (at most 1 per 1000 pixels of the support) and a reason.  It is empty: no such pixel has turned up.
"""
import collections
import ctypes
import functools
import os
import subprocess

import numpy as np

import adjoint_columns as ac
from conftest import BUILD, ROOT, TOL, sample_points

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")
MODE_AREA, MODE_FAST, MODE_BILINEAR, MODE_BICUBIC = 1, 2, 3, 4

IMAGES = ("normal", "offset", "lognormal", "big", "small", "checker", "negconst")
POISONS = (float("nan"), float("inf"), float("-inf"))
EXCUSED = {}                  # case name -> (count, reason)
# Cases whose kernel is known to break the locality contract and was left as it is, because no fix fitted the speed margin: their
# locality items are expected failures (strict, one item per case), their finite-data items stay live.  (case name, reason)
_WIDE = ("aai_wide_kernel<area> keeps w x v for zero-area pairs of a part: a select costs 1.2 % at 8:1 (0.1371 vs 0.1355 ms), "
         "a select behind a vote 3.6 % (0.1404 vs 0.1355 ms), measured against the parent build on one MI355X")
NOT_LOCAL_CASES = (("wide area 96x80 5.5:1 at 200", _WIDE), ("wide area 120x90 8:1 at 33.3", _WIDE))


def not_local(c):
    return any(c.name == n for n, _ in NOT_LOCAL_CASES)


def image(name, H, W, index=0, C=1):
    """image `name` of IMAGES for an (H, W[, C]) source, fixed by seed and index; float32"""
    shape = (H, W) if C == 1 else (H, W, C)
    rng = np.random.default_rng(4242 + 31 * IMAGES.index(name) + index)
    n = rng.standard_normal(shape)
    if name == "normal":
        a = n
    elif name == "offset":
        a = 1000.0 + n
    elif name == "lognormal":
        a = np.exp(3.0 * n) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    elif name == "big":
        a = n * 1e30
    elif name == "small":
        a = n * 1e-30
    elif name == "checker":
        yy, xx = np.indices((H, W))
        a = np.where((yy + xx) & 1, -1.0, 1.0)
        a = a if C == 1 else np.repeat(a[:, :, None], C, axis=2)
    else:
        a = np.full(shape, -0.7310586)
    return np.ascontiguousarray(a, dtype=np.float32)


def int_image(T, H, W, index=0, C=1):
    """8- / 16-bit noise over the whole range of the type, 0 and the largest value included"""
    hi = 256 if T == "u8" else 65536
    a = np.random.default_rng(977 + index).integers(0, hi, size=(H, W) if C == 1 else (H, W, C))
    a.flat[0], a.flat[-1] = 0, hi - 1
    return a.astype(np.uint8 if T == "u8" else np.uint16)


def scaled_error(got, gold, mag, floor, what):
    """the finite-data check: exact zeros where the magnitude is 0, |got - gold| <= TOL max(mag, floor); returns the worst
    |got - gold| / max(mag, floor), which the caller prints"""
    got, gold, mag = np.asarray(got, np.float64), np.asarray(gold, np.float64), np.asarray(mag, np.float64)
    assert got.shape == gold.shape == mag.shape, (what, got.shape, gold.shape)
    assert np.isfinite(got).all(), (what, "non-finite output from finite data")
    off = mag == 0
    assert np.all(got[off] == 0), (what, "%d pixels the oracle leaves at 0 are not 0" % int((got[off] != 0).sum()))
    assert floor > 0, what
    err = np.abs(got - gold) / np.maximum(mag, floor)
    worst = float(err.max())
    assert worst <= TOL, (what, worst, np.unravel_index(int(err.argmax()), err.shape))
    return worst


def locality(got_bad, got_zero, support, allowed, what, name):
    """the non-finite check.  support: where non-finite is required; allowed: where it is tolerated (== support except for the samplers)"""
    broken = ~np.isfinite(got_bad)
    leaks = broken & ~allowed
    missed = support & ~broken
    assert not leaks.any(), (what, "%d outputs are non-finite where the oracle has no weight on a poisoned pixel, first %s"
                             % (int(leaks.sum()), np.argwhere(leaks)[0].tolist()))
    budget = EXCUSED.get(name, (0, ""))[0]
    assert budget <= support.sum() // 1000
    assert int(missed.sum()) <= budget, (what, "%d outputs stayed finite inside the oracle's support, first %s"
                                         % (int(missed.sum()), np.argwhere(missed)[0].tolist()))
    same = ~allowed
    assert np.array_equal(got_bad[same], got_zero[same]), (what, "outputs outside the support differ from the run with the poisoned pixels at 0")
    return int(missed.sum())


def comb_masks(W, H, pitch, phases):
    """boolean [H, W] masks, one per phase"""
    out = []
    for (ox, oy) in phases:
        m = np.zeros((H, W), bool)
        m[oy::pitch, ox::pitch] = True
        out.append(m)
    return out


def tap_window_hit(rq, lay, mask, mode):
    """[dH, dW]: does the clamped tap window of the dst pixel (2 x 2 bilinear, 4 x 4 bicubic, around floor(sample point)) hold a pixel of
    `mask`?  The sample points are conftest.sample_points'."""
    sx, sy = sample_points(rq, lay, list(range(lay.dst_height)), "cpu")
    fx, fy = np.floor(sx.numpy()).astype(np.int64), np.floor(sy.numpy()).astype(np.int64)
    H, W = mask.shape
    lo, hi = (0, 1) if mode == MODE_BILINEAR else (-1, 2)
    hit = np.zeros(fx.shape, bool)
    for j in range(lo, hi + 1):
        for i in range(lo, hi + 1):
            hit |= mask[np.clip(fy + j, 0, H - 1), np.clip(fx + i, 0, W - 1)]
    return hit


# ---- forward cases ----------------------------------------------------------------------------------------------------------------
# kernel: what aai_last_kernel() must name (a substring); replay: which CPU replay of tests/emulation runs the case ("axis" K1, "quad" the
# fp32 quad / fast / wide formulation, "cell", "f64" the double-precision kernels' arithmetic, None: the samplers have no replay);
# cell: the request carries AAI_POLICY_PREFER_CELL (debug_cell_min_waves(0)); border: the oracle's output has an all-zero border "row" /
# "col"; phases: "edge" (adjoint_columns.edge_phases) or "all" (every phase of the pitch: the empty-border cases, so that whatever
# source position a table parks an empty entry on is poisoned in some run; the three values then take turns over the combs); via: "host" entry or the "device" entries (batch of two,
# interleaved, typed, band); band: the device band entry on the half of the dst rows that holds the empty border row.
Fwd = collections.namedtuple("Fwd", "name kernel W H sr dr ang iso mode policy C T cell replay border phases via band")


def _fwd(name, kernel, W, H, sr, dr, ang, iso=None, mode=MODE_AREA, policy=0, C=1, T="f32", cell=False, replay="quad", border=None,
         phases="edge", via="host", band=False):
    iso = ((W - 1) / 2.0, (H - 1) / 2.0) if iso is None else iso
    return Fwd(name, kernel, W, H, float(sr), float(dr), float(ang), iso, mode, policy, C, T, cell, replay, border, phases, via, band)


# Axis-aligned requests whose canvas overhangs the image by a whole dst row or column (found with the oracle on an all-ones image over
# random isocenters; test_value_domain_host.py re-checks every one): angle -> (row case, column case).  The first two are the issue's.
BORDERS = {
    0.0: ((48, 50, 4.0, (18.00705583183881, 15.836908327848215)), (15, 16, 2.0, (5.924464005972803, 6.690854843538962)),
          (17, 15, 2.0, (7.902140466326401, 5.967663754556569))),
    90.0: ((13, 18, 2.0, (3.840879499544567, 7.8795681862766855)), (15, 37, 2.0, (11.874843083855108, 22.390053803268035)),
           (14, 13, 2.0, (3.8297826262211903, 3.908245866204088))),
    180.0: ((12, 15, 2.0, (4.148381134281411, 9.69773848176986)), (15, 13, 2.0, (5.872060585568743, 6.942146700367012))),
    270.0: ((13, 21, 2.0, (8.121215869969564, 7.518497528122669)), (21, 13, 2.0, (11.770655227805786, 8.838483884951536))),
}
BORDER_KIND = {0.0: ("row", "col", "row"), 90.0: ("row", "col", "col"), 180.0: ("row", "col"), 270.0: ("row", "col")}
# a source narrower than four elements (the wide kernel) whose canvas overhangs it: found the same way
NARROW_BORDER = (3, 13, 2.0, 0.0, (1.631432173674119, 5.71551704031469))

# the fix-up pass behind the fp32 kernels: cases of tests/golden/knife_cases.npz by index, two of conftest.KNIFE_EDGE_CASES.  Listed form:
# in the table.  Dense form (the whole image in the double-precision pass): reached through AAI_MAX_LISTED_PIXELS only, which the library
# reads once per process -- dense_child below, started by test_value_domain_gpu.py, runs the same two cases there.
KNIFE_FIXUP = (48, 73)


def forward_cases(aai, hostemu=None, knife_manifest=None):
    """the forward table; the K1 strip-branch cases come from tests/axis_variants.py's table when `hostemu` is given"""
    D = aai.POLICY_DOUBLE_PRECISION
    cs = []
    # ---- K1
    for ang, geos in BORDERS.items():
        for (W, H, sr, iso), kind in zip(geos, BORDER_KIND[ang]):
            for mode in (MODE_AREA, MODE_FAST):
                cs.append(_fwd("k1 empty %s %dx%d at %g mode %d" % (kind, W, H, ang, mode), "aai_axis", W, H, sr, 1, ang, iso, mode,
                               replay="axis", border=kind, phases="all"))
    W, H, sr, iso = BORDERS[0.0][2]
    cs.append(_fwd("k1 empty row C=3", "aai_axis_kernel", W, H, sr, 1, 0.0, iso, C=3, replay="axis", border="row", phases="all", via="device"))
    cs.append(_fwd("k1 empty row band", "aai_axis_kernel", W, H, sr, 1, 0.0, iso, replay="axis", border="row", phases="all", via="device", band=True))
    cs.append(_fwd("k1 empty row batch", "aai_axis_kernel", W, H, sr, 1, 0.0, iso, replay="axis", border="row", phases="all", via="device"))
    W, H, sr, iso = BORDERS[90.0][2]
    cs.append(_fwd("k1 empty col C=3 at 90", "aai_axis_kernel", W, H, sr, 1, 90.0, iso, C=3, replay="axis", border="col", phases="all", via="device"))
    for T in ("u8", "u16"):
        for mode in (MODE_AREA, MODE_FAST):
            cs.append(_fwd("k1 %s mode %d" % (T, mode), "aai_axis_kernel", 17, 15, 2.0, 1, 0.0, BORDERS[0.0][2][3], mode, T=T, replay="axis",
                           border="row", via="device"))
    cs.append(_fwd("k1 tile 70x50 1:2 at 90", "aai_axis_tile_kernel", 70, 50, 1, 2, 90.0, replay="axis"))
    cs.append(_fwd("k1 wide 3x50 2:1", "aai_axis_wide_kernel", 3, 50, 2, 1, 0.0, replay="axis"))
    W, H, sr, ang, iso = NARROW_BORDER
    cs.append(_fwd("k1 wide narrow empty row", "aai_axis_wide_kernel", W, H, sr, 1, ang, iso, replay="axis", border="row", phases="all"))
    if hostemu is not None:
        import axis_variants as av
        cands, big, tall, cases, probe = av.table(hostemu)
        seen = set()
        for case in cases:
            c, p = case.cand, case.point
            if c.kernel == "aai_axis_kernel" and c.T == "f32" and not c.multi and c.sub in av.BRANCHES and c.sub not in seen:
                seen.add(c.sub)
                cs.append(_fwd("k1 branch %s %dx%d %g:1 at %g" % (c.sub, p.W, p.H, p.ratio, p.angle), "aai_axis_kernel", p.W, p.H, p.ratio, 1,
                               p.angle, av.iso_of(p.W, p.H, p.off), p.mode, replay="axis"))
        # (branch B and a second turn of A's loop need a million output rows: axis_variants.BIG; no small case reaches them)
        assert seen >= set("ACDE"), seen
    # ---- rotated, fp32
    cs.append(_fwd("quad area 90x70 3:1 at 17.5", "aai_quad_kernel", 90, 70, 3, 1, 17.5))
    cs.append(_fwd("quad fast 90x70 3:1 at 17.5", "aai_quad_fast_kernel", 90, 70, 3, 1, 17.5, mode=MODE_FAST))
    cs.append(_fwd("quad area 40x30 x3 at 45", "aai_quad_kernel", 40, 30, 1, 3, 45.0))
    cs.append(_fwd("quad area 64x48 1:1 at 200 batch", "aai_quad_kernel", 64, 48, 1, 1, 200.0, iso=(30.2, 25.7), via="device"))
    cs.append(_fwd("quad multi C=2", "aai_quad_multi_kernel", 90, 70, 3, 1, 17.5, C=2, via="device"))
    cs.append(_fwd("quad multi C=4 x3 at 45", "aai_quad_multi_kernel", 40, 30, 1, 3, 45.0, C=4, via="device"))
    cs.append(_fwd("cell 90x70 3:1 at 17.5", "aai_cell_kernel", 90, 70, 3, 1, 17.5, cell=True, replay="cell"))
    cs.append(_fwd("cell 40x30 x3 at 45", "aai_cell_kernel", 40, 30, 1, 3, 45.0, cell=True, replay="cell"))
    cs.append(_fwd("cell multi C=3 x2 at 30", "aai_cell_multi_kernel", 128, 96, 1, 2, 30.0, C=3, cell=True, replay="cell", via="device"))
    cs.append(_fwd("wide area 96x80 5.5:1 at 200", "aai_wide_kernel", 96, 80, 5.5, 1, 200.0))
    cs.append(_fwd("wide area 120x90 8:1 at 33.3", "aai_wide_kernel", 120, 90, 8, 1, 33.3))
    cs.append(_fwd("wide fast 96x80 5.5:1 at 200", "fast_kernel", 96, 80, 5.5, 1, 200.0, mode=MODE_FAST))
    cs.append(_fwd("wide fast 120x90 8:1 at 33.3", "aai_wide_fast_kernel", 120, 90, 8, 1, 33.3, mode=MODE_FAST))
    # ---- rotated, double precision
    cs.append(_fwd("f64 runs 64x64 40:1 at 17.5", "aai_rotated_runs_kernel", 64, 64, 40, 1, 17.5, replay="f64"))
    cs.append(_fwd("f64 area 90x70 3:1 at 17.5", "aai_rotated_kernel<area>", 90, 70, 3, 1, 17.5, policy=D, replay="f64"))
    cs.append(_fwd("f64 fast 90x70 3:1 at 17.5", "aai_rotated_kernel<fast>", 90, 70, 3, 1, 17.5, mode=MODE_FAST, policy=D, replay="f64"))
    cs.append(_fwd("f64 near axis 37x29 2.5:1", "aai_rotated_kernel<area>", 37, 29, 2.5, 1, 89.9999999, policy=D, replay="f64"))
    cs.append(_fwd("f64 wide 96x80 5.5:1 at 200", "aai_rotated_runs_kernel", 96, 80, 5.5, 1, 200.0, policy=D, replay="f64"))
    cs.append(_fwd("f64 wide 120x90 8:1 at 33.3", "aai_rotated_runs_kernel", 120, 90, 8, 1, 33.3, policy=D, replay="f64"))
    if knife_manifest is not None:
        for idx in KNIFE_FIXUP:
            c = knife_manifest[idx]
            # every phase of the comb: each source pixel is poisoned in some run, so every pair of a flagged pixel is, touching ones included
            cs.append(_fwd("fix-up knife %d" % idx, "aai_quad_kernel", c["W"], c["H"], c["src_res"], c["dst_res"], c["angle"], tuple(c["iso"]),
                           replay="quad", phases="all"))
    # ---- samplers: planar takes the vector-load path in the interior and the general path at clamped edges, C = 3 the general path
    for mode, nm in ((MODE_BILINEAR, "bilinear"), (MODE_BICUBIC, "bicubic")):
        for (W, H, sr, dr, ang) in ((80, 60, 1, 2, 300.0), (64, 64, 2, 1, 17.5)):
            for C in (1, 3):
                cs.append(_fwd("%s %dx%d C=%d at %g" % (nm, W, H, C, ang), "aai_sample_kernel<%s>" % nm, W, H, sr, dr, ang, mode=mode, C=C,
                               replay=None, via="device" if C > 1 else "host"))
    assert len({c.name for c in cs}) == len(cs)
    return cs


def fwd_request(aai, c):
    return aai.make_request(c.W, c.H, c.sr, c.dr, c.iso, c.ang, mode=c.mode, policy=c.policy)


def oracle_forward(po, c, plane):
    """the oracle on one [H, W] plane (float32 values widened to float64)"""
    omode = {MODE_AREA: po.MODE_EXACT, MODE_FAST: po.MODE_FAST, MODE_BILINEAR: 3, MODE_BICUBIC: 4}[c.mode]
    return po.oracle_run(omode, np.ascontiguousarray(plane, dtype=np.float64), c.sr, c.dr, c.iso, c.ang).dst


def per_plane(fn, a):
    return fn(a) if a.ndim == 2 else np.stack([fn(a[:, :, k]) for k in range(a.shape[2])], axis=2)


def fwd_phases(aai, c):
    rc, msg, lay = aai.query(fwd_request(aai, c))
    assert rc == 0, msg
    pitch = ac.comb_pitch(lay, c.ang)
    if c.mode == MODE_BICUBIC:
        pitch = max(pitch, 7)            # (farther apart than the 4 x 4 window of an up-sampled pixel)
    if c.phases == "all":
        return lay, pitch, [(ox, oy) for oy in range(min(pitch, c.H)) for ox in range(min(pitch, c.W))]
    return lay, pitch, [(ox, oy) for (ox, oy) in ac.edge_phases(c.W, c.H, pitch) if ox < c.W and oy < c.H]


def empty_border(gold_ones, kind):
    """which border row / column of the oracle's all-ones output is all zero: (axis, index) or None"""
    if kind == "row":
        for r in (0, gold_ones.shape[0] - 1):
            if not gold_ones[r].any():
                return 0, r
    if kind == "col":
        for k in (0, gold_ones.shape[1] - 1):
            if not gold_ones[:, k].any():
                return 1, k
    return None


def band_of(po, c, lay):
    """the half of the dst rows that holds the case's empty border row"""
    _, r = empty_border(oracle_forward(po, c, np.ones((c.H, c.W))), "row")
    half = lay.dst_height // 2
    return (0, half) if r < half else (half, lay.dst_height)


def check_forward_finite(po, aai, c, run, images=IMAGES):
    """run(src) -> dst of the case's shape.  Returns the worst scaled error over the images."""
    worst = 0.0
    for k, nm in enumerate(images):
        src = int_image(c.T, c.H, c.W, k, c.C) if c.T != "f32" else image(nm, c.H, c.W, k, c.C)
        got = run(src)
        wide = src.astype(np.float64)
        gold = per_plane(lambda p: oracle_forward(po, c, p), wide)
        if c.mode == MODE_BICUBIC:
            # the cubic's weights are signed, so oracle(|src|) is not sum |w_i| |v_i| (its lobes cancel there too).  A tap window is
            # 4 x 4 source pixels, clamped taps fold onto one edge pixel: of a comb of pitch 5 a dst pixel sees at most one pixel, so
            # the absolute values of the 25 combs' outputs add up to sum |w_i| |v_i| exactly -- from the oracle alone
            mag = per_plane(lambda p: sum(np.abs(oracle_forward(po, c, np.where(m, np.abs(p), 0.0))) for m in
                                          comb_masks(c.W, c.H, 5, [(i, j) for j in range(5) for i in range(5)])), wide)
        else:
            mag = per_plane(lambda p: oracle_forward(po, c, np.abs(p)), wide)
        worst = max(worst, scaled_error(got, gold, mag, 1e-3 * float(np.abs(wide).max()), "%s / %s" % (c.name, nm)))
        if c.T != "f32":
            break
    return worst


def check_forward_locality(po, aai, c, run, poisons=POISONS):
    """Returns (runs, pixels in the supports, excused misses)."""
    lay, pitch, phases = fwd_phases(aai, c)
    rq = fwd_request(aai, c)
    base = image("normal", c.H, c.W, 99, c.C) + np.float32(0.5)
    runs = cover = excused = 0
    masks = comb_masks(c.W, c.H, pitch, phases)
    if c.phases == "all":
        assert np.logical_or.reduce(masks).all(), (c.name, "a source pixel is in no comb")
    for n, m in enumerate(masks):
        support = oracle_forward(po, c, m.astype(np.float64)) != 0
        if not support.any() and c.phases == "all":
            continue                     # (a comb of an "all phases" case that no dst pixel sees)
        allowed = support if c.mode in (MODE_AREA, MODE_FAST) else support | tap_window_hit(rq, lay, m, c.mode)
        zeroed = base.copy()
        zeroed[m] = 0.0
        got_zero = run(zeroed)
        for bad in (poisons if c.phases != "all" else (poisons[n % len(poisons)],)):
            poisoned = base.copy()
            poisoned[m] = bad
            got = run(poisoned)
            sup, alw = (support, allowed) if c.C == 1 else (np.repeat(support[:, :, None], c.C, 2), np.repeat(allowed[:, :, None], c.C, 2))
            excused += locality(got, got_zero, sup, alw, "%s / phase %s / %r" % (c.name, phases[n], bad), c.name)
            runs += 1
            cover += int(support.sum())
    assert runs > 0 and cover > 0, c.name
    return runs, cover, excused


# ---- adjoint cases ------------------------------------------------------------------------------------------------------------------
# family: "general" | "planned" | "any" | "separable" (interleaved planned) | "sample"; kernel: a substring of aai_last_kernel() or None
Adj = collections.namedtuple("Adj", "name family kernel W H sr dr ang iso mode C")


def _adj(name, family, kernel, W, H, sr, dr, ang, iso=None, mode=MODE_AREA, C=1):
    iso = ((W - 1) / 2.0, (H - 1) / 2.0) if iso is None else iso
    return Adj(name, family, kernel, W, H, float(sr), float(dr), float(ang), iso, mode, C)


def adjoint_cases():
    cs = [_adj("general area", "general", "aai_adjoint_gather_kernel<area>", 24, 20, 3, 1, 17.5),
          _adj("general fast", "general", "aai_adjoint_gather_kernel<fast>", 24, 20, 3, 1, 17.5, mode=MODE_FAST),
          _adj("general C=3", "general", "aai_adjoint", 24, 20, 3, 1, 17.5, C=3),
          _adj("planned any at 17.5", "any", "aai_adjoint_plain_gather_kernel<area>", 24, 20, 3, 1, 17.5),
          _adj("planned any C=3 at 17.5", "any", "aai_adjoint_plain", 24, 20, 3, 1, 17.5, C=3),
          _adj("separable C=3 at 17.5", "separable", "aai_adjoint_plain", 24, 20, 3, 1, 17.5, C=3)]
    for ang in (0.0, 270.0):
        for (W, H, sr, iso), kind in zip(BORDERS[ang][-2:], ("row", "col")):
            cs.append(_adj("planned at %g empty %s %dx%d" % (ang, kind, W, H), "planned", "aai_axis_adjoint_kernel", W, H, sr, 1, ang, iso))
    W, H, sr, iso = BORDERS[90.0][2]
    cs.append(_adj("separable C=3 at 90 empty col", "separable", "aai_axis_adjoint_multi_kernel", W, H, sr, 1, 90.0, iso, C=3))
    for mode, nm in ((MODE_BILINEAR, "bilinear"), (MODE_BICUBIC, "bicubic")):
        for C in (1, 3):
            cs.append(_adj("sample %s C=%d" % (nm, C), "sample", "aai_adjoint_sample_kernel", 24, 20, 3, 1, 17.5, mode=mode, C=C))
            cs.append(_adj("sample %s C=%d x2 at 45" % (nm, C), "sample", "aai_adjoint_sample_kernel", 16, 12, 1, 2, 45.0, mode=mode, C=C))
    assert len({c.name for c in cs}) == len(cs)
    return cs


@functools.lru_cache(maxsize=None)
def _matrix(W, H, sr, dr, ang, iso, mode):
    from oracle import pyoracle as po
    from test_adjoint_host import oracle_matrix
    omode = {MODE_AREA: po.MODE_EXACT, MODE_FAST: po.MODE_FAST, MODE_BILINEAR: 3, MODE_BICUBIC: 4}[mode]
    M = oracle_matrix(po, omode, W, H, sr, dr, iso, ang)
    M.setflags(write=False)
    return M


def adjoint_matrix(po, c):
    """the oracle's W ([dH dW, H W], float64) of the case's geometry: built once per session per geometry, read-only"""
    return _matrix(c.W, c.H, c.sr, c.dr, c.ang, c.iso, c.mode)


def adj_request(aai, c):
    return aai.make_request(c.W, c.H, c.sr, c.dr, c.iso, c.ang, mode=c.mode)


def dst_combs(dW, dH, pitch=5):
    """poisoned dst pixels: combs through (0, 0), through the last row and column, and one inside"""
    phases = []
    for ph in ((0, 0), ((dW - 1) % pitch, (dH - 1) % pitch), (2 % pitch, 3 % pitch)):
        if ph not in phases and ph[0] < dW and ph[1] < dH:
            phases.append(ph)
    return comb_masks(dW, dH, pitch, phases)


def check_adjoint_finite(po, aai, c, run, images=IMAGES):
    """run(gdst [dH, dW] or [dH, dW, C]) -> gsrc [H, W(, C)]"""
    M = adjoint_matrix(po, c)
    rc, msg, lay = aai.query(adj_request(aai, c))
    assert rc == 0 and M.shape == (lay.dst_width * lay.dst_height, c.W * c.H), msg
    worst = 0.0
    for k, nm in enumerate(images):
        g = image(nm, lay.dst_height, lay.dst_width, 50 + k, c.C)
        got = run(g)
        wide = g.astype(np.float64)
        gold = per_plane(lambda p: (M.T @ p.ravel()).reshape(c.H, c.W), wide)
        mag = per_plane(lambda p: (np.abs(M).T @ np.abs(p).ravel()).reshape(c.H, c.W), wide)
        worst = max(worst, scaled_error(got, gold, mag, 1e-3 * float(mag.max()), "%s / %s" % (c.name, nm)))
    return worst


def check_adjoint_locality(po, aai, c, run, poisons=POISONS):
    """poison in gdst, support in gsrc: support = (W[poisoned d, :] != 0).any(0).  Returns (runs, pixels in the supports, poisoned dst
    pixels whose row of W is all zero)."""
    M = adjoint_matrix(po, c)
    rq = adj_request(aai, c)
    rc, msg, lay = aai.query(rq)
    assert rc == 0, msg
    dW, dH = lay.dst_width, lay.dst_height
    base = image("normal", dH, dW, 98, c.C) + np.float32(0.5)
    runs = cover = unread = 0
    for m in dst_combs(dW, dH):
        rows = M[m.ravel()]
        support = (rows != 0).any(0).reshape(c.H, c.W)
        unread += int((~(rows != 0).any(1)).sum())
        allowed = support
        if c.mode in (MODE_BILINEAR, MODE_BICUBIC):
            # the source pixels inside the tap window of a poisoned dst pixel
            sx, sy = sample_points(rq, lay, list(range(dH)), "cpu")
            fx, fy = np.floor(sx.numpy()).astype(np.int64)[m], np.floor(sy.numpy()).astype(np.int64)[m]
            lo, hi = (0, 1) if c.mode == MODE_BILINEAR else (-1, 2)
            allowed = support.copy()
            for j in range(lo, hi + 1):
                for i in range(lo, hi + 1):
                    allowed[np.clip(fy + j, 0, c.H - 1), np.clip(fx + i, 0, c.W - 1)] = True
        zeroed = base.copy()
        zeroed[m] = 0.0
        got_zero = run(zeroed)
        for bad in poisons:
            poisoned = base.copy()
            poisoned[m] = bad
            got = run(poisoned)
            sup, alw = (support, allowed) if c.C == 1 else (np.repeat(support[:, :, None], c.C, 2), np.repeat(allowed[:, :, None], c.C, 2))
            locality(got, got_zero, sup, alw, "%s / %r" % (c.name, bad), c.name)
            runs += 1
            cover += int(support.sum())
    assert cover > 0, c.name
    return runs, cover, unread


# ---- CPU replays of the adjoint kernels (tests/emulation) -----------------------------------------------------------------------------
_EMU = {"general": ("adjoint_emulation.cpp", "aai_emu_adjoint"), "general_multi": ("adjoint_multi_emulation.cpp", "aai_emu_adjoint_multi"),
        "planned": ("axis_adjoint_emulation.cpp", "aai_emu_axis_adjoint"), "separable_axis": ("axis_adjoint_multi_emulation.cpp", "aai_emu_axis_adjoint_multi"),
        "any": ("adjoint_plain_emulation.cpp", "aai_emu_adjoint_plain"), "any_multi": ("adjoint_plain_multi_emulation.cpp", "aai_emu_adjoint_plain_multi"),
        "sample": ("adjoint_sample_emulation.cpp", "aai_emu_adjoint_sample")}


@functools.lru_cache(maxsize=None)
def _emu_lib(source):
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_vd_%s.so" % source[:-4])
    src = os.path.join(ROOT, "tests", "emulation", source)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".cpp"))]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return ctypes.CDLL(so)


def adjoint_replay(aai, c):
    """run(gdst) -> gsrc through the CPU replay of the kernels that serve the case's family at its geometry"""
    axis = c.ang % 90.0 == 0.0
    key = {"general": "general" if c.C == 1 else "general_multi", "planned": "planned",
           "any": "any" if c.C == 1 else "any_multi", "separable": "separable_axis" if axis else "any_multi", "sample": "sample"}[c.family]
    source, symbol = _EMU[key]
    fn = getattr(_emu_lib(source), symbol)
    fn.restype = ctypes.c_int
    fn.argtypes = None
    rq = adj_request(aai, c)
    P = ctypes.c_void_p

    def run(g):
        g = np.ascontiguousarray(g, dtype=np.float32)
        out = np.full((c.H, c.W) if c.C == 1 else (c.H, c.W, c.C), -1.0, np.float32)
        gp, op = P(g.ctypes.data), P(out.ctypes.data)
        if key == "general":
            rc = fn(ctypes.byref(rq), gp, op)
        elif key == "general_multi":
            rc = fn(ctypes.byref(rq), ctypes.c_int(c.C), gp, op)
        elif key == "planned":
            rc = fn(ctypes.byref(rq), gp, op, (ctypes.c_int * 3)())
        elif key == "separable_axis":
            rc = fn(ctypes.byref(rq), ctypes.c_int(c.C), gp, op, (ctypes.c_int * 3)())
        elif key == "any":
            rc = fn(ctypes.byref(rq), gp, op, ctypes.c_uint(1 << 24), (ctypes.c_long * 4)())
        elif key == "any_multi":
            rc = fn(ctypes.byref(rq), ctypes.c_int(c.C), gp, op, ctypes.c_uint(1 << 24), (ctypes.c_long * 3)())
        else:
            v, w = ctypes.c_longlong(), ctypes.c_longlong()
            rc = fn(ctypes.byref(rq), ctypes.c_int(c.C), gp, op, ctypes.byref(v), ctypes.byref(w))
        assert rc == 0, (c.name, key, rc)
        return out
    return run



# ---- the dense form of the fix-up pass ------------------------------------------------------------------------------------------------
def dense_child():
    """Runs in a process of its own with AAI_MAX_LISTED_PIXELS=10 (test_value_domain_gpu.py starts it): the plans of the two fix-up cases
    keep no list, and the strict form of aai_rotated_kernel computes the whole image -- finite data and locality, as in the table."""
    import json
    import re
    import torch            # noqa: F401  (before the library: one HIP runtime per process)
    import area_average_interpolation_amd as aai
    from oracle import pyoracle as po
    assert os.environ.get("AAI_MAX_LISTED_PIXELS") == "10"
    aai.set_device(0)
    z = np.load(os.path.join(ROOT, "tests", "golden", "knife_cases.npz"))
    manifest = json.loads(bytes(z["manifest"]).decode())
    for c in forward_cases(aai, None, manifest):
        if not c.name.startswith("fix-up"):
            continue

        def run(src, c=c):
            rc, msg, dst, _, _ = aai.resample_host(src, c.sr, c.dr, c.iso, c.ang, mode=c.mode, policy=c.policy)
            assert rc == 0 and "strict" in aai.last_kernel(), (c.name, msg, aai.last_kernel())
            return dst
        err = check_forward_finite(po, aai, c, run)
        runs, cover, excused = check_forward_locality(po, aai, c, run)
        m = re.search(r"flagged=(\d+) dense=(\d+)", aai.plan_shape(fwd_request(aai, c)))
        assert m and int(m.group(2)) == 1 and excused == 0, (c.name, aai.plan_shape(fwd_request(aai, c)))
        print("dense %s %s scaled err %.2e  %d poisoned runs, %d support pixels" % (c.name, aai.last_kernel(), err, runs, cover))
    print("dense ok")


if __name__ == "__main__":
    dense_child()
