"""Which template instantiation of the rotated-lattice fp32 kernels serves a request, and a table of test cases that reaches every
one the dispatcher can choose (helper of test_rot_variants_host.py / test_rot_variants_gpu.py; needs no GPU).

The launchers (csrc/aai_rotated_quad.hip, aai_rotated_cell.hip, aai_rotated_wide.hip) pick one instantiation per call:

    aai_quad_kernel                 <T, WIN 2..8, SCALED, HP>
    aai_quad_fast_kernel / _rows    <T, WIN 2..8, SCALED>            (the row-shaped wave is a kernel of its own)
    aai_quad_multi_kernel           <T, WIN 3..8, SCALED, WORDS>     (HP is a run-time branch there; the table keeps it apart)
    aai_cell_kernel                 <T, WIN 2..8, SCALED, HP, WR>
    aai_cell_multi_kernel           <T, WIN 2..6, SCALED, HP, WORDS>
    aai_wide_kernel                 <T, WIN 5..8, HP, PARTS>
    aai_wide_fast_kernel            <T, WIN 5..8, PARTS>

What they key on comes from the variant probe aai_emu_rot_variant (tests/emulation/host_emulation.cpp), which asks the header
functions the launchers ask.  No rule of the dispatch is restated here: this file only names the fields, walks a grid and bisects.

CANDIDATES: the set of (family, T, C, WIN, SCALED, HP, X) the probe reports over GRID below, X = WR (cell), PARTS (wide),
WORDS (interleaved), row-shaped wave (fast), 0 (quad).  For C > 1 a candidate whose family an LDS admission rule keeps away is kept
with dispatched = False (the GPU module lists those in NOT_DISPATCHED).

CASES: two geometries per candidate, found by bisecting the probe along the ratio axis at a fixed angle: `leave` sits with
hb = h (c + s) 0.001 source pixel BELOW the boundary at which the candidate's region ends towards larger footprints (where the
footprint just fits the window: a window one column too small would drop an outer column there, at least 1e-3 / side of a pixel's
weight, a hundred times the 1e-5 bar for every side these kernels serve), `enter` 0.001 ABOVE the boundary at which it begins.
The angle is one of the candidate's grid angles at which that boundary is a window threshold (the window's full extent changes
across it); where a candidate has none -- its region ends at another rule first: the smallest dst pixel the reference's
pre-expansion allows, a change of the precision variant or of the wave's shape -- the case sits 0.001 inside that boundary
instead and says so (Case.boundary).
"""
import collections
import ctypes
import math

import numpy as np

# ---- the probe ------------------------------------------------------------------------------------------------------------------
FIELDS = ("family", "scale", "quad", "cell", "wide", "win", "win_full", "parts", "hiprec", "cell_win", "cell_hiprec",
          "cell_wave_rows", "words", "fast_row_shaped", "quad_multi_fits", "cell_multi_fits", "dW", "dH")      # enum RotVariantField
Variant = collections.namedtuple("Variant", FIELDS)
FAMILIES = {1: "aai_quad_kernel", 2: "aai_quad_fast_kernel", 3: "aai_quad_multi_kernel", 4: "aai_cell_kernel",
            5: "aai_cell_multi_kernel", 6: "aai_wide_kernel", 7: "aai_wide_fast_kernel", 8: "fp64"}          # enum RotVariantFamily
# the WIN range each family is instantiated for (the kernel table above): every candidate must lie inside
TEMPLATE_WIN = {"aai_quad_kernel": (2, 8), "aai_quad_fast_kernel": (2, 8), "aai_quad_multi_kernel": (3, 8), "aai_cell_kernel": (2, 8),
                "aai_cell_multi_kernel": (2, 6), "aai_wide_kernel": (5, 8), "aai_wide_fast_kernel": (5, 8)}
MODE_AREA, MODE_FAST = 1, 2
PREFER_CELL = 0x200          # AAI_POLICY_PREFER_CELL
TYPES = {"f32": (np.float32, 4, 0, 1.0), "u8": (np.uint8, 1, 1, 256.0), "u16": (np.uint16, 2, 2, 65536.0)}     # numpy type, bytes, AAI_DTYPE_*, value scale
CHANNELS = (1, 2, 3, 4)


def bind(lib):
    """lib: the CDLL of tests/emulation/host_emulation.cpp (conftest's hostemu fixture)"""
    from area_average_interpolation_amd import _lib as L
    lib.aai_emu_rot_variant.restype = ctypes.c_int
    lib.aai_emu_rot_variant.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


class Prober:
    def __init__(self, lib):
        from area_average_interpolation_amd import _lib as L
        self.lib = bind(lib)
        self.out = (ctypes.c_int * len(FIELDS))()
        self.rq = L.Request(1, 0, 64, 64, 1.0, 1.0, 1.0, 1.0, 31.7, 32.2, 0.0)
        self.calls = 0

    def __call__(self, ratio, angle, mode, policy, C, esz, W=64, H=64, iso=(31.7, 32.2), dst_res=1.0):
        rq = self.rq
        rq.mode, rq.policy, rq.src_width, rq.src_height = mode, policy, W, H
        rq.src_res_x = rq.src_res_y = ratio
        rq.dst_res_x = rq.dst_res_y = dst_res
        rq.src_iso_x, rq.src_iso_y, rq.rotation_deg = iso[0], iso[1], angle
        rc = self.lib.aai_emu_rot_variant(ctypes.byref(rq), C, esz, self.out)
        assert rc == 0, (rc, ratio, angle, W, H)
        self.calls += 1
        return Variant(*self.out)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
# ratio = source pixels per dst pixel side (src_res / dst_res), 0.25 (x4 up-sampling) ... 40; reduced angle in degrees, the last
# degree at each end in six steps
# (+ sqrt 2 / k: the largest dst pixel pre-expansion by k + 1 allows; at sqrt 2 and 45 degrees it is the only place where a replicated
# source meets the widest windows replication can have, a sliver 1e-5 of hb wide that the knife-edge goldens sit in)
RATIOS = sorted(np.concatenate([np.arange(0.25, 3.0, 0.05), np.arange(3.0, 12.0, 0.25), np.arange(12.0, 40.0 + 1e-9, 1.0)]).round(6).tolist() +
                [math.sqrt(2.0) / k for k in (1, 2, 3, 4)])
_HALF = [0.01, 0.03, 0.1, 0.3, 0.6, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0] + [float(a) for a in range(8, 45, 2)]
ANGLES = _HALF + [45.0] + [90.0 - a for a in reversed(_HALF)]
GRID = "ratio %g..%g (%d values) x reduced angle %g..%g degrees (%d values) x {area, fast} x {f32, u8, u16} x C in {1, 2, 3, 4}" % (
    RATIOS[0], RATIOS[-1], len(RATIOS), ANGLES[0], ANGLES[-1], len(ANGLES))

# (family, T, C, WIN, SCALED, HP, X)
Candidate = collections.namedtuple("Candidate", "family T C win scaled hp x")


def hosted(probe, ratio, angle, mode, T, C, **where):
    """The candidates a geometry hosts for (mode, T, C): {candidate: (policy that selects it, dispatched)}.  Area mode is probed
    twice: small outputs take the quad family by default and the cell family with AAI_POLICY_PREFER_CELL."""
    esz = TYPES[T][1]
    found = {}
    for policy in ((0, PREFER_CELL) if mode == MODE_AREA else (0,)):
        v = probe(ratio, angle, mode, policy, C, esz, **where)
        fam = FAMILIES.get(v.family)
        scaled = int(v.scale > 1)
        if fam in ("aai_quad_kernel",):
            found.setdefault(Candidate(fam, T, C, v.win, scaled, v.hiprec, 0), (policy, True))
        elif fam == "aai_quad_fast_kernel":
            found.setdefault(Candidate(fam, T, C, v.win, scaled, 0, v.fast_row_shaped), (policy, True))
        elif fam == "aai_quad_multi_kernel":
            found.setdefault(Candidate(fam, T, C, v.win, scaled, v.hiprec, v.words), (policy, True))
        elif fam == "aai_cell_kernel":
            found.setdefault(Candidate(fam, T, C, v.cell_win, scaled, v.cell_hiprec, v.cell_wave_rows), (policy, True))
        elif fam == "aai_cell_multi_kernel":
            found.setdefault(Candidate(fam, T, C, v.cell_win, scaled, v.cell_hiprec, v.words), (policy, True))
        elif fam in ("aai_wide_kernel", "aai_wide_fast_kernel"):
            found.setdefault(Candidate(fam, T, C, v.win, 0, v.hiprec if fam == "aai_wide_kernel" else 0, v.parts), (policy, True))
        # interleaved windows an LDS admission rule keeps away from a family that is instantiated for them
        if C > 1 and mode == MODE_AREA:
            if policy == PREFER_CELL and v.cell and not v.cell_multi_fits and TEMPLATE_WIN["aai_cell_multi_kernel"][0] <= v.cell_win <= TEMPLATE_WIN["aai_cell_multi_kernel"][1]:
                found.setdefault(Candidate("aai_cell_multi_kernel", T, C, v.cell_win, scaled, v.cell_hiprec, v.words), (policy, False))
            if policy == 0 and v.quad and not v.quad_multi_fits:
                found.setdefault(Candidate("aai_quad_multi_kernel", T, C, v.win, scaled, v.hiprec, v.words), (policy, False))
    return found


def window_extent(v, family):
    return v.cell_win if family.startswith("aai_cell") else v.win_full


def scan_grid(probe, types=tuple(TYPES), channels=CHANNELS):
    """candidate -> (policy, dispatched, [(ratio, angle), ...]) over the whole grid"""
    cands = {}
    for T in types:
        for C in channels:
            for mode in (MODE_AREA, MODE_FAST):
                for ratio in RATIOS:
                    for angle in ANGLES:
                        for cand, (policy, dispatched) in hosted(probe, ratio, angle, mode, T, C).items():
                            e = cands.setdefault(cand, (mode, policy, dispatched, []))
                            assert e[:3] == (mode, policy, dispatched), (cand, e[:3], mode, policy, dispatched)
                            e[3].append((ratio, angle))
    return cands


# ---- cases ------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "index cand dispatched mode policy which boundary W H ratio iso angle dW dH")
HB_STEP = 1e-3               # source pixels of hb = h (c + s) between a case and its boundary
ISO_OFFSETS = ((0.3137, -0.2113), (-0.4181, 0.1319), (0.1873, 0.4337))      # isocenter - image centre: off the lattice, no symmetry


def _hb_per_ratio(v, angle):
    t = math.radians(angle)
    return 0.5 * v.scale * (math.cos(t) + math.sin(t))          # hb = h (c + s), h = side / 2, side = ratio x scale


def _boundary(probe, cand, mode, ratio0, angle, up):
    """Bisect the probe along the ratio axis from a grid point that hosts `cand`: returns (ratio just inside, ratio just outside),
    outside None where the candidate reaches the end of the grid."""
    T, C = cand.T, cand.C
    i = RATIOS.index(ratio0)
    inside = ratio0
    outside = None
    while True:
        i += 1 if up else -1
        if i < 0 or i >= len(RATIOS):
            return inside, None
        if cand in hosted(probe, RATIOS[i], angle, mode, T, C):
            inside = RATIOS[i]
        else:
            outside = RATIOS[i]
            break
    for _ in range(60):
        mid = 0.5 * (inside + outside)
        if mid == inside or mid == outside or abs(outside - inside) < 1e-12:
            break
        if cand in hosted(probe, mid, angle, mode, T, C):
            inside = mid
        else:
            outside = mid
    return inside, outside


def canvas(ratio, scale, angle):
    """The smallest source (W, H) whose dst canvas holds two 16 x 16 tiles per axis, crosses a cell strip (63 or 31 columns) and a
    64-column row wave -- at least 66 x 34 dst pixels, about 70 x 40 -- with all four canvas borders inside the output by construction
    (the output IS the bounding box of the rotated source).  angle: the full rotation; odd quadrants swap the source's axes."""
    quadrant = int(angle // 90) % 4
    t = math.radians(angle - 90 * quadrant)
    c, s = math.cos(t), math.sin(t)
    side = ratio * scale
    A, B = 70.0 * side, 40.0 * side                   # virtual pixels the canvas should span
    low = max(4.0 * scale, 2.0 * side + 2.0 * scale)  # never a source narrower than a footprint
    det = c * c - s * s
    mW = (A * c - B * s) / det if abs(det) > 1e-9 else -1.0
    mH = (B * c - A * s) / det if abs(det) > 1e-9 else -1.0
    if mW < low or mH < low:
        # no rectangle has that bounding box at this angle (towards 45 degrees it turns square): one axis at its minimum, the other
        # as long as both extents ask
        if s <= c:
            mH = low
            mW = max((A - mH * s) / c, (B - mH * c) / s if s > 1e-9 else 0.0)
        else:
            mW = low
            mH = max((A - mW * c) / s, (B - mW * s) / c if c > 1e-9 else 0.0)
    vW, vH = int(math.ceil(mW / scale)), int(math.ceil(mH / scale))
    return (vH, vW) if quadrant & 1 else (vW, vH)


def build_cases(probe, cands):
    """Two cases per candidate; deterministic (the order of `cands` sorted)."""
    cases = []
    for cand in sorted(cands):
        mode, policy, dispatched, points = cands[cand]
        angles = sorted({a for (_, a) in points})
        # from the middle of the candidate's angles outwards: clear of the region's angular borders
        mid = angles[len(angles) // 2]
        angles.sort(key=lambda a: (abs(a - mid), a))
        for which, up in (("enter", False), ("leave", True)):
            chosen = None
            for angle in angles:
                ratios = {r for (r, a) in points if a == angle}
                # every stretch of consecutive grid ratios that hosts the candidate at this angle (replication makes several): its
                # end in the direction asked
                ends = [r for r in sorted(ratios, reverse=up)
                        if not (0 <= RATIOS.index(r) + (1 if up else -1) < len(RATIOS)) or RATIOS[RATIOS.index(r) + (1 if up else -1)] not in ratios]
                for start in ends:
                    inside, outside = _boundary(probe, cand, mode, start, angle, up)
                    esz = TYPES[cand.T][1]
                    vin = probe(inside, angle, mode, policy, cand.C, esz)
                    kind = "grid end"
                    if outside is not None:
                        vout = probe(outside, angle, mode, policy, cand.C, esz)
                        kind = "window" if window_extent(vout, cand.family) != window_extent(vin, cand.family) else "other rule"
                    if chosen is None or (kind == "window" and chosen[0] != "window"):
                        chosen = (kind, angle, inside, outside, vin, start)
                    if kind == "window":
                        break
                if chosen[0] == "window":
                    break
            kind, angle, inside, outside, vin, start = chosen
            step = HB_STEP / _hb_per_ratio(vin, angle)
            other = _boundary(probe, cand, mode, start, angle, not up)[0]      # where the same stretch of ratios ends the other way
            ratio = inside - step if up else inside + step
            if (up and ratio < other) or (not up and ratio > other):
                ratio = 0.5 * (inside + other)                       # a region narrower than two steps: its middle
            if outside is None:
                ratio = inside                                       # the end of the grid itself
            index = len(cases)
            full = angle + 90.0 * (index % 4)                        # the quadrants round-robin
            W, H = canvas(ratio, vin.scale, full)
            ox, oy = ISO_OFFSETS[(index // 4) % len(ISO_OFFSETS)]
            iso = ((W - 1) / 2.0 + ox, (H - 1) / 2.0 + oy)
            v = probe(ratio, full, mode, policy, cand.C, TYPES[cand.T][1], W=W, H=H, iso=iso)
            cases.append(Case(index, cand, dispatched, mode, policy, which, kind, W, H, ratio, iso, full, v.dW, v.dH))
    return cases


_TABLE = {}


def table(lib):
    """(candidates, cases) -- built once per process"""
    if "t" not in _TABLE:
        probe = Prober(lib)
        cands = scan_grid(probe)
        _TABLE["t"] = (cands, build_cases(probe, cands), probe)
    return _TABLE["t"]


# Interleaved candidates an LDS admission rule keeps from their family: (family, T, C, WIN) -> (rule, what runs instead).  Every
# SCALED / HP variant of the entry is meant.  An entry whose family DID run is stale and fails the test, like a missing one.
# Instead of the cell family the quad family would be next, but its window is one position wider and fails its own rule wherever
# the cell rule fails, so both end on the double-precision kernels (aai_rotated_kernel / aai_rotated_runs_kernel <area, channels>).
_CELL_RULE = "aai_rot_cell.hpp:cell_multi_fits_lds (asked by aai_rotated_cell.hip:cell_can_serve): WIN * WIN * WORDS > 64 KiB of LDS"
_QUAD_RULE = "aai_rot_quad.hpp:quad_multi_fits_lds (asked by aai_rotated_quad.hip:quad_can_address): WIN * WIN * WORDS > 80 KiB of LDS"
NOT_DISPATCHED = {}
for _T, _C, _wins in (("f32", 2, (6,)), ("f32", 3, (5, 6)), ("f32", 4, (5, 6)), ("u16", 3, (6,)), ("u16", 4, (6,))):
    for _w in _wins:
        NOT_DISPATCHED[("aai_cell_multi_kernel", _T, _C, _w)] = (_CELL_RULE, "fp64")
for _T, _C, _wins in (("f32", 2, (7, 8)), ("f32", 3, (6, 7, 8)), ("f32", 4, (5, 6, 7, 8)), ("u16", 3, (7, 8)), ("u16", 4, (7, 8))):
    for _w in _wins:
        NOT_DISPATCHED[("aai_quad_multi_kernel", _T, _C, _w)] = (_QUAD_RULE, "fp64")


# ---- data and reference of a case -----------------------------------------------------------------------------------------------
def case_source(case, flip=False):
    """the case's source image: [H, W] or [H, W, C] of its type; noise well away from zero (exact zeros are the canvas corners')"""
    npdt, _, _, hi = TYPES[case.cand.T]
    rng = np.random.default_rng(1000 + case.index)
    shape = (case.H, case.W) if case.cand.C == 1 else (case.H, case.W, case.cand.C)
    src = (rng.random(shape, dtype=np.float32) + np.float32(0.25)) if npdt == np.float32 else rng.integers(1, int(hi), size=shape).astype(npdt)
    return np.ascontiguousarray(src[::-1]) if flip else src


def case_gold(po, case, src):
    """the oracle on the case's source, per channel: [dH, dW] or [dH, dW, C] float64"""
    omode = po.MODE_EXACT if case.mode == MODE_AREA else po.MODE_FAST
    run = lambda plane: po.oracle_run(omode, np.ascontiguousarray(plane, dtype=np.float64), case.ratio, 1.0, case.iso, case.angle).dst
    if src.ndim == 2:
        return run(src)
    return np.stack([run(src[:, :, c]) for c in range(src.shape[2])], axis=2)


def case_id(case):
    c = case.cand
    return "%s<%s,C%d,WIN%d,S%d,HP%d,X%d>/%s" % (c.family, c.T, c.C, c.win, c.scaled, c.hp, c.x, case.which)
