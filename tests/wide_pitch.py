"""Small images in WIDE-PITCH buffers: the case table that takes every kernel family through the regimes of its hand-written offset
arithmetic (helper of test_wide_pitch_host.py / test_wide_pitch_gpu.py; needs no GPU to import).

Every switch of that arithmetic reads the source view's row stride, never the image width: QuadMap::mul24Ok / fastOk (make_quad_map:
pitch below 8 MiB), spans_4gib (H x pitch x element size: anchor rows of the quad and wide kernels, rebased waves of the cell kernel,
the samplers' vector-tap path, lastLoad4 / lastLoad8, interleaved images to the fp64 kernels), and the bounds of cell_can_serve /
quad_can_address that keep one wave's rows inside 32 bits.  So a narrow, tall image (W C <= 640, H <= 1100) placed at a row stride of
megabytes takes the paths of a 4 ... 8 GiB image, costs a few seconds, and the oracle judges every pixel of it.

REGIMES of a source view, classified by the probe aai_emu_rot_variant_pitched (tests/emulation/host_emulation.cpp: the launchers' own
predicates of csrc/aai_rot_serve.hpp and make_quad_map) -- nothing of the dispatch is restated here:
    T    tight (the control every wide case is compared with)
    T+   a wide pitch below both switches: u8 at 2^31 elements, and the inner side of the boundary pairs of the two thresholds
    P    pitch >= 8 MiB (mul24Ok = 0), span below 4 GiB
    G    span >= 4 GiB (spans_4gib), pitch below 8 MiB
    GP   span >= 4 GiB and pitch >= 8 MiB
    E31  a flag beside the regime: H x pitch >= 2^31 ELEMENTS (fp32 about 8.6 GB; u16 whenever it spans 4 GiB; u8 from 2 GiB, i.e.
         below every 4 GiB switch)
    X    the family of the tight control does not serve the view (its own bound refuses): the case names the family that takes over

BOUNDARY PAIRS: two cases one element of pitch apart, found by bisecting the probe along the pitch, either side of the 4 GiB threshold,
of pitch x element size = 2^23, of cell_can_serve's span bound (at a geometry with a two-row wave) and of quad_can_address's anchor
bound (a quad geometry and a wide one).  The last pitch a family still serves is where a wrong bound gives wrong pixels.

NOT REACHABLE, by the rules the probe asks: aai_cell_kernel in GP (cell_can_serve: a pitch below 2^23 bytes above 4 GiB -- the X cases
show aai_quad_kernel taking over), aai_quad_multi_kernel / aai_cell_multi_kernel in G and GP (spans_4gib sends interleaved images to
the double-precision kernels -- X cases too).  LEFT OUT: K1's per-pixel kernel at a footprint wider than a strip (280 : 1): no swap of
two source rows moves its output by 100 x the bar, so the oracle could not tell a misaddressed row there; the same kernel runs in
every regime on rows shorter than four elements (k1-wide).

ARENA: one device byte buffer for sources and one for destinations per test module (torch.empty: never filled whole), at most
ARENA_CAP bytes each and ARENA_CAP_BOTH together; an [H, W C] image is a strided view into it, the 64 elements behind every source row
poisoned (NaN / all ones), the rows of a destination and 64 elements of their padding pre-filled with the sentinel.
"""
import collections
import ctypes

import numpy as np

import rot_variants as rv

GiB = 1 << 30
ARENA_CAP = int(8.75 * GiB)
ARENA_CAP_BOTH = int(13.5 * GiB)
GUARD = 64                   # poisoned / sentinel elements behind a row
SENTINEL = -7.0
MAX_ROW, MAX_H = 640, 1100

TYPES = rv.TYPES             # name -> (numpy type, bytes, AAI_DTYPE_*, value scale)
MODE_AREA, MODE_FAST, MODE_BILINEAR, MODE_BICUBIC = 1, 2, 3, 4
DOUBLE_PRECISION, PREFER_CELL = 0x100, 0x200

# ---- the probe ------------------------------------------------------------------------------------------------------------------
PFIELDS = rv.FIELDS + ("spans_4gib", "mul24Ok", "fastOk", "anchorRows", "rebaseWaves", "form")         # + enum RotPitchedField
View = collections.namedtuple("View", PFIELDS)
FAMILIES = dict(rv.FAMILIES)
FAMILIES[0] = None           # K1 and the samplers: named by the axis probe / by the mode


class Prober:
    def __init__(self, lib):
        from area_average_interpolation_amd import _lib as L
        import axis_variants as av
        lib.aai_emu_rot_variant_pitched.restype = ctypes.c_int
        lib.aai_emu_rot_variant_pitched.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)]
        self.lib = lib
        self.out = (ctypes.c_int * len(PFIELDS))()
        self.tight = rv.Prober(lib)
        self.axis = av.Prober(lib)
        self.axis_names = av.KERNELS
        self.L = L

    def request(self, g, H):
        iso = iso_of(g, H)
        return self.L.Request(g.mode, g.policy, g.W, H, g.src_res, g.src_res, g.dst_res, g.dst_res, iso[0], iso[1], g.angle)

    def __call__(self, g, H, T, pitch):
        """the probed View of geometry g at source height H, type T, row stride `pitch` elements"""
        rq = self.request(g, H)
        rc = self.lib.aai_emu_rot_variant_pitched(ctypes.byref(rq), g.C, TYPES[T][1], int(pitch), self.out)
        assert rc == 0, (rc, g, H, T, pitch)
        return View(*self.out)

    def family(self, g, H, T, pitch):
        """the name aai_last_kernel() must start with"""
        v = self(g, H, T, pitch)
        if v.family:
            return FAMILIES[v.family]
        if g.mode == MODE_BILINEAR:
            return "aai_sample_kernel<bilinear>"
        if g.mode == MODE_BICUBIC:
            return "aai_sample_kernel<bicubic>"
        a = self.axis(g.W, H, g.src_res / g.dst_res, g.angle, g.mode, iso_of(g, H), g.C, TYPES[T][1], 1)
        return self.axis_names[a.kernel]


def regime(v, tight):
    """T / P / G / GP of a probed view (`tight`: the stride is the image's row)"""
    if tight:
        return "T"
    return ("GP" if not v.mul24Ok else "G") if v.spans_4gib else ("P" if not v.mul24Ok else "T+")


def e31(H, pitch):
    return H * pitch >= 1 << 31


def extent_bytes(H, row, pitch, esz, guard=GUARD):
    """bytes of arena a view takes, the guard behind its last row included"""
    return ((H - 1) * pitch + row + guard) * esz


# ---- geometries -----------------------------------------------------------------------------------------------------------------
# One geometry per kernel family and quadrant parity: `angle` in quadrant 0 / 2 (the pitch is the stride of virtual Y) or 1 / 3 (of
# virtual X).  W in source pixels; the height comes from the pitch class (H supplies the span).  knife: the isocentre sits on the
# lattice and the plan must report flagged > 0 dense=0 (the fix-up pass then reads the wide-pitch source).
Geom = collections.namedtuple("Geom", "name mode policy src_res dst_res angle W C iso_off types knife heights iso_y")
OFF = (0.3137, -0.2113)
ALL = ("f32", "u8", "u16")
SHORT, TALL, TOP = 300, 560, MAX_H          # P needs H x 8 MiB < 4 GiB; G needs H x pitch >= 4 GiB at a pitch below 8 MiB; fp32 E31 needs both at 2^31 elements


def _g(name, mode, policy, src_res, dst_res, angles, W, C=1, types=ALL, knife=False, heights=(SHORT, TALL), iso_off=OFF, iso_y=None):
    """iso_off: isocentre - image centre; iso_y: the isocentre's row instead, whatever the height"""
    return [Geom("%s/%g" % (name, a), mode, policy, float(src_res), float(dst_res), float(a), W, C, (0.0, 0.0) if knife else iso_off, types, knife, heights, iso_y) for a in angles]


GEOMS = (
    # K1: the strip kernel at 0 / 180 degrees, its transposed forms (branch A, the tile kernel) at 90 / 270, the per-pixel kernel of rows shorter than four elements
    _g("k1", MODE_AREA, 0, 2, 1, (180.0, 90.0), 300, heights=(SHORT, TALL, TOP)) +
    _g("k1-r4", MODE_AREA, 0, 4, 1, (0.0, 270.0), 520) +
    _g("k1-fast", MODE_FAST, 0, 3, 1, (0.0, 90.0), 200) +
    _g("k1-wide", MODE_AREA, 0, 2, 1, (0.0, 90.0), 3) +
    _g("k1-rgb", MODE_AREA, 0, 2, 1, (0.0, 270.0), 100, C=3) +
    # ... and K1 with a fix-up list behind it (3 : 1 about a pixel centre of row 7: the classifier departs from the separable model in
    # two dst rows -- in quadrant 1 two dst columns)
    _g("k1-fixup", MODE_AREA, 0, 3, 1, (0.0, 90.0), 120, knife=True, iso_y=7.0) +
    # the cell kernel: 32 x 2 waves (side >= 2.35), 64 x 1 waves, replicated sources (x2 up-sampling)
    _g("cell-32x2", MODE_AREA, PREFER_CELL, 3, 1, (17.5, 107.5), 200, heights=(SHORT, TALL, TOP)) +
    _g("cell-64x1", MODE_AREA, PREFER_CELL, 2, 1, (210.0, 300.0), 160) +
    _g("cell-scaled", MODE_AREA, PREFER_CELL, 1, 2, (30.0, 120.0), 40, heights=(SHORT, 530)) +
    # the quad kernels: area; fast with the 16 x 4 wave and with the row-shaped wave
    _g("quad", MODE_AREA, 0, 3, 1, (17.5, 287.5), 200, heights=(SHORT, TALL, TOP)) +
    _g("quad-scaled", MODE_AREA, 0, 1, 2, (200.0, 120.0), 40, heights=(SHORT, 530)) +
    _g("fast-16x4", MODE_FAST, 0, 3, 1, (197.5, 107.5), 200) +
    _g("fast-rows", MODE_FAST, 0, 1.5, 1, (30.0, 120.0), 100) +
    # wide footprints
    _g("wide", MODE_AREA, 0, 8, 1, (17.5, 107.5), 400) +
    _g("wide-fast", MODE_FAST, 0, 8, 1, (197.5, 287.5), 400) +
    # the double-precision kernels: area, fast, rows as runs
    _g("fp64-area", MODE_AREA, DOUBLE_PRECISION, 3, 1, (17.5, 107.5), 120, types=("f32", "u16")) +
    _g("fp64-fast", MODE_FAST, DOUBLE_PRECISION, 3, 1, (200.0, 290.0), 120, types=("f32", "u8")) +
    _g("fp64-runs", MODE_AREA, DOUBLE_PRECISION, 8, 1, (17.5, 107.5), 300, types=("f32", "u8")) +
    # interleaved RGB: the multi kernels below 4 GiB, the double-precision kernels they fall to above
    _g("quad-rgb", MODE_AREA, 0, 3, 1, (17.5, 107.5), 100, C=3) +
    _g("cell-rgb", MODE_AREA, PREFER_CELL, 2, 1, (30.0, 120.0), 100, C=3) +
    # the comparison samplers: the vector-tap path below 4 GiB, the general path above
    _g("bilinear", MODE_BILINEAR, 0, 2, 1, (17.5, 107.5), 200) +
    _g("bicubic", MODE_BICUBIC, 0, 1, 2, (200.0, 300.0), 60, heights=(SHORT, 530)) +
    _g("bilinear-rgb", MODE_BILINEAR, 0, 2, 1, (0.0, 90.0), 100, C=3) +
    # one knife-edge geometry per fp32 formulation: the isocentre on the lattice
    _g("knife-cell", MODE_AREA, PREFER_CELL, 1, 1, (30.0, 120.0), 81, knife=True, heights=(SHORT - 1, TALL + 1), types=("f32",)) +
    _g("knife-quad", MODE_AREA, 0, 3, 1, (30.0, 300.0), 201, knife=True, heights=(SHORT - 1, TALL + 1), types=("f32",)) +
    _g("knife-fast", MODE_FAST, 0, 2, 1, (30.0, 120.0), 201, knife=True, heights=(SHORT - 1, TALL + 1), types=("f32",))
)
GEOMS = tuple(GEOMS)
BY_NAME = {g.name: g for g in GEOMS}


def pitch_for(cls, H, row, esz):
    """The row stride (elements) of a pitch class for an image of H rows of `row` elements: the smallest pitch of the class plus an
    odd number of elements, so that no row starts on a power of two.  cls: "P" / "GP" (just past 8 MiB), "G" (just past 4 GiB of
    span), "E31" (just past 2^31 elements)."""
    if cls in ("P", "GP"):
        return -(-(1 << 23) // esz) + 37
    if cls == "G":
        return -(-(1 << 32) // (H * esz)) + 129
    if cls == "E31":
        return -(-(1 << 31) // H) + 5
    raise ValueError(cls)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# family: what serves the view (the name aai_last_kernel() must report); control: the family of the tight control; regime and e31 as
# probed; x: the two differ, `family` is the one that takes over; bound: the boundary pair's name and side ("" for the regime cases)
Case = collections.namedtuple("Case", "index kind geom T H pitch cls regime e31 family control x bound")


def case_id(c):
    return "%s-%s-H%d-%s%s%s%s" % (c.geom.name, c.T, c.H, c.regime, "+E31" if c.e31 else "", "-X" if c.x else "", ("-" + c.bound) if c.bound else "")


def row_elems(g):
    return g.W * g.C


def _mk(probe, index, kind, g, T, H, pitch, cls, bound=""):
    esz = TYPES[T][1]
    row = row_elems(g)
    tight = pitch == row
    v = probe(g, H, T, pitch)
    fam = probe.family(g, H, T, pitch)
    ctl = probe.family(g, H, T, row)
    return Case(index, kind, g, T, H, int(pitch), cls, regime(v, tight), e31(H, pitch), fam, ctl, fam != ctl, bound)


def classes_of(g):
    """(pitch class, height) pairs of a geometry's grid"""
    out = [("P", g.heights[0]), ("G", g.heights[1]), ("GP", g.heights[1]), ("E31", g.heights[1])]
    if len(g.heights) > 2:
        out.append(("E31", g.heights[2]))
    return out


def grid(probe):
    """every (geometry, type, pitch class, height) of the table's grid with what the probe says of it: [(g, T, cls, H, pitch, family, regime, e31)]"""
    out = []
    for g in GEOMS:
        for T in g.types:
            esz = TYPES[T][1]
            for cls, H in classes_of(g):
                pitch = pitch_for(cls, H, row_elems(g), esz)
                if extent_bytes(H, row_elems(g), pitch, esz) > ARENA_CAP:
                    continue
                v = probe(g, H, T, pitch)
                out.append((g, T, cls, H, pitch, probe.family(g, H, T, pitch), regime(v, False), e31(H, pitch)))
    return out


def forward_cases(probe):
    """Each (geometry, pitch class) once, the types rotating with the geometry's index so that the two quadrant parities of a family
    meet different types in the same class; u8 always takes E31 (2 ... 4 GiB: below every 4 GiB switch), fp32 where the geometry has a
    third height; and the tight controls (regime T) of every (geometry, type, height) a wide case uses."""
    cases = []
    for gi, g in enumerate(GEOMS):
        row = row_elems(g)
        for ci, (cls, H) in enumerate(classes_of(g)):
            if cls == "E31":
                Ts = [T for T in (("u8",) if H != MAX_H else ("f32",)) if T in g.types]
            else:
                Ts = [g.types[(gi + ci) % len(g.types)]]
                if cls == "G" and len(g.types) == 3:
                    Ts.append(g.types[(gi + ci + 2) % 3])         # (with GP's type the third: both parities together see all three above 4 GiB)
            for T in Ts:
                esz = TYPES[T][1]
                pitch = pitch_for(cls, H, row, esz)
                if extent_bytes(H, row, pitch, esz) > ARENA_CAP:
                    continue
                cases.append(_mk(probe, len(cases), "forward", g, T, H, pitch, cls))
    return cases


# ---- boundary pairs ---------------------------------------------------------------------------------------------------------------
# (name, geometry, type, H, probed field, pitch range to bisect): the two cases are the last pitch with the field's first value and
# the first pitch with another.  The ranges start where the view already spans what the bound needs.
def _field(probe, g, H, T, field):
    if field == "family":
        return lambda p: probe.family(g, H, T, p)
    return lambda p: getattr(probe(g, H, T, p), field)


def bisect_pitch(f, lo, hi):
    """smallest pitch in (lo, hi] at which f differs from f(lo); None if f(hi) == f(lo)"""
    a = f(lo)
    if f(hi) == a:
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(mid) == a:
            lo = mid
        else:
            hi = mid
    return hi


Bound = collections.namedtuple("Bound", "name geom T H field lo hi")


def bounds():
    M8 = 1 << 23
    B = []
    # the 4 GiB threshold itself: spans_4gib flips (anchor rows, rebased waves, the samplers' general path, interleaved -> fp64)
    for name, T in (("quad/17.5", "f32"), ("cell-32x2/107.5", "u16"), ("wide/17.5", "u8"), ("fast-16x4/107.5", "f32"), ("cell-scaled/30", "u8"),
                    ("bilinear/17.5", "f32"), ("bicubic/300", "f32"), ("quad-rgb/107.5", "f32"), ("fp64-area/17.5", "f32"), ("k1/90", "f32")):
        g = BY_NAME[name]
        esz = TYPES[T][1]
        B.append(Bound("4GiB", g, T, g.heights[1], "spans_4gib", row_elems(g), M8 // esz - 1))
    # pitch x element size = 2^23: mul24Ok (and fastOk) flip -- below 4 GiB (short image) and above (tall image)
    for name, T, hsel in (("quad/287.5", "f32", 0), ("fast-16x4/197.5", "f32", 0), ("cell-scaled/120", "u16", 0), ("quad-scaled/200", "u8", 0),
                          ("wide/107.5", "f32", 1), ("quad/17.5", "u16", 1), ("fast-rows/30", "f32", 0), ("cell-32x2/17.5", "f32", 0)):
        g = BY_NAME[name]
        esz = TYPES[T][1]
        B.append(Bound("8MiB", g, T, g.heights[hsel], "mul24Ok", M8 // esz - 4096, M8 // esz + 4096))
    # cell_can_serve's span bound at a geometry with the tallest wave (two cell rows per step) whose span x pitch reaches 2^32 below a
    # pitch of 8 MiB: side 5.2 at 8 degrees
    B.append(Bound("cell-span", CELL_SPAN, "f32", 600, "family", -(-(1 << 32) // (600 * 4)) + 1, M8 // 4 - 1))
    B.append(Bound("cell-span", CELL_SPAN_ODD, "u8", 600, "family", -(-(1 << 32) // 600) + 1, M8 - 1))
    # quad_can_address's anchor bound, (2 anchorRows + win + 2) x pitch = 2^32, for a quad geometry and a wide one: short images whose
    # few rows lie tens of MiB apart
    B.append(Bound("anchor", QUAD_ANCHOR, "f32", 130, "family", -(-(1 << 32) // (130 * 4)) + 1, (1 << 32) // (100 * 4)))
    B.append(Bound("anchor", QUAD_ANCHOR_ODD, "u16", 130, "family", -(-(1 << 32) // (130 * 2)) + 1, (1 << 32) // (100 * 2)))
    B.append(Bound("anchor", WIDE_ANCHOR, "f32", 320, "family", -(-(1 << 32) // (320 * 4)) + 1, (1 << 32) // (200 * 4)))
    return B


CELL_SPAN, CELL_SPAN_ODD = _g("cell-span", MODE_AREA, PREFER_CELL, 5.2, 1, (8.0, 98.0), 400, heights=(SHORT, 600))
QUAD_ANCHOR, QUAD_ANCHOR_ODD = _g("quad-anchor", MODE_AREA, 0, 3, 1, (17.5, 107.5), 400, heights=(130, 130))
WIDE_ANCHOR, = _g("wide-anchor", MODE_AREA, 0, 8, 1, (17.5,), 600, heights=(320, 320))
BOUND_GEOMS = (CELL_SPAN, CELL_SPAN_ODD, QUAD_ANCHOR, QUAD_ANCHOR_ODD, WIDE_ANCHOR)


def boundary_cases(probe, first_index):
    """[(bound, inside case, at case)]; the pitch of `at` is the first at which the probed field changes"""
    out = []
    idx = first_index
    for b in bounds():
        at = bisect_pitch(_field(probe, b.geom, b.H, b.T, b.field), b.lo, b.hi)
        assert at is not None, ("the probed field does not change over the range", b)
        tag = "%s:%s" % (b.name, b.field)
        inside = _mk(probe, idx, "forward", b.geom, b.T, b.H, at - 1, "bound", tag + "-inside")
        edge = _mk(probe, idx + 1, "forward", b.geom, b.T, b.H, at, "bound", tag + "-at")
        idx += 2
        out.append((b, inside, edge))
    return out


# ---- destinations of 4 GiB and more, and of 2^31 elements; batches whose images lie 2^31 elements apart ------------------------------
# (geometry, type, dst class "G" / "E31"): the source is tight; dst pitch = the class's pitch for dH rows of fp32
DST_CASES = (("k1/180", "f32", "G"), ("k1/90", "u8", "G"), ("k1/90", "f32", "E31"), ("k1-r4/270", "u16", "G"), ("k1-wide/0", "f32", "G"), ("k1-fixup/0", "f32", "G"),
             ("k1-empty/0", "f32", "G"),
             ("cell-32x2/17.5", "f32", "G"), ("cell-64x1/300", "u8", "G"), ("cell-scaled/30", "u16", "G"), ("quad/287.5", "f32", "G"), ("quad/17.5", "u16", "E31"),
             ("fast-16x4/107.5", "f32", "G"), ("fast-rows/30", "f32", "G"), ("wide/17.5", "u8", "G"), ("wide-fast/287.5", "f32", "G"),
             ("fp64-area/17.5", "f32", "G"), ("fp64-runs/107.5", "u8", "G"), ("quad-rgb/17.5", "f32", "G"), ("cell-rgb/120", "u8", "G"),
             ("bilinear/17.5", "f32", "G"), ("bicubic/300", "f32", "G"), ("bilinear-rgb/90", "u8", "G"), ("knife-quad/30", "f32", "G"))
# a K1 geometry whose canvas overhangs the image by a whole dst row (value_domain.BORDERS: launch_axis_zero writes that row)
K1_EMPTY, = _g("k1-empty", MODE_AREA, 0, 4, 1, (0.0,), 48, iso_off=(18.00705583183881 - 23.5, 0.0), iso_y=15.836908327848215, types=("f32",), heights=(50, 50))
BATCH_CASES = (("k1/180", "f32"), ("cell-32x2/17.5", "u8"), ("quad/287.5", "u16"), ("fp64-area/107.5", "f32"), ("bicubic/300", "f32"))


def geom_by_name(name):
    if name in BY_NAME:
        return BY_NAME[name]
    for g in BOUND_GEOMS + (K1_EMPTY,):
        if g.name == name:
            return g
    raise KeyError(name)


def dst_pitch_for(cls, dH):
    return pitch_for("G" if cls == "G" else "E31", dH, 0, 4)


def batch_apart(T, side):
    """elements between the two images of a batch case: 2^31 and a little (u8 sources: 2^32)"""
    return ((1 << 32) if T == "u8" and side == "src" else (1 << 31)) + 4099


def source_arena_bytes(lib):
    """what the source arena must hold: the largest view of the table and the batch cases' second image"""
    probe, fwd, bnd = table(lib)
    need = [extent_bytes(c.H, row_elems(c.geom), c.pitch, TYPES[c.T][1]) for c in fwd + [c for (_, a, b) in bnd for c in (a, b)]]
    for name, T in BATCH_CASES:
        g = geom_by_name(name)
        need.append((batch_apart(T, "src") + extent_bytes(g.heights[0], row_elems(g), row_elems(g) + GUARD, 1)) * TYPES[T][1])
    return max(need)


def dst_size(probe, g, H):
    v = probe(g, H, g.types[0], row_elems(g))
    return v.dH, v.dW, v.dW * g.C


def dst_arena_bytes(lib):
    probe, _, _ = table(lib)
    need = []
    for name, T, cls in DST_CASES:
        g = geom_by_name(name)
        dH, dW, drow = dst_size(probe, g, g.heights[0])
        need.append(extent_bytes(dH, drow, dst_pitch_for(cls, dH), 4))
    for name, T in BATCH_CASES:
        g = geom_by_name(name)
        dH, dW, drow = dst_size(probe, g, g.heights[0])
        need.append((batch_apart(T, "dst") + extent_bytes(dH, drow, drow + GUARD, 1)) * 4)
    return max(need)


_TABLE = {}


def table(lib):
    """(probe, forward cases, boundary triples) -- built once per process"""
    if "t" not in _TABLE:
        probe = Prober(lib)
        fwd = forward_cases(probe)
        _TABLE["t"] = (probe, fwd, boundary_cases(probe, len(fwd)))
    return _TABLE["t"]


# ---- data and reference ---------------------------------------------------------------------------------------------------------
def source(g, T, H, seed=0):
    """[H, W] or [H, W, C] of type T: noise in [0.25, 1.25) x the type's value scale (rot_variants.case_source)"""
    npdt, _, _, hi = TYPES[T]
    rng = np.random.default_rng(7000 + 131 * GEOMS_INDEX.get(g.name, 999) + H + seed)
    shape = (H, g.W) if g.C == 1 else (H, g.W, g.C)
    if npdt == np.float32:
        return rng.random(shape, dtype=np.float32) + np.float32(0.25)
    return rng.integers(1, int(hi), size=shape).astype(npdt)


GEOMS_INDEX = {g.name: i for i, g in enumerate(GEOMS + BOUND_GEOMS + (K1_EMPTY,))}


def iso_of(g, H):
    return ((g.W - 1) / 2.0 + g.iso_off[0], (H - 1) / 2.0 + g.iso_off[1] if g.iso_y is None else g.iso_y)


def gold(po, g, H, src):
    """the oracle on a source, per channel: float64 [dH, dW] or [dH, dW, C]"""
    omode = {MODE_AREA: po.MODE_EXACT, MODE_FAST: po.MODE_FAST}.get(g.mode, g.mode)
    run = lambda plane: po.oracle_run(omode, np.ascontiguousarray(plane, dtype=np.float64), g.src_res, g.dst_res, iso_of(g, H), g.angle).dst
    if src.ndim == 2:
        return run(src)
    return np.stack([run(src[:, :, c]) for c in range(src.shape[2])], axis=2)


def bar(g, T):
    """(relative?, bound): conftest.TOL relative with the floor of 1e-3 x the value scale for the area / fast modes; the samplers keep the
    absolute 2e-5 x the value scale of test_comparison_samplers_against_cpu_restatement"""
    return (False, 2e-5) if g.mode in (MODE_BILINEAR, MODE_BICUBIC) else (True, 1e-5)


def scaled_error(g, T, got, want):
    """per-pixel error in units of the bar's reference: relative (floor 1e-3 x value scale) or absolute / value scale"""
    hi = TYPES[T][3]
    got = np.asarray(got, dtype=np.float64)
    if bar(g, T)[0]:
        return np.abs(got - want) / np.maximum(np.abs(want), 1e-3 * hi)
    return np.abs(got - want) / hi


# ---- the arena and the placement of images in it (GPU modules only: torch is imported here, not above) ----------------------------------
def _torch_type(T):
    import torch
    return {"f32": torch.float32, "u8": torch.uint8, "u16": torch.int16, "f64": torch.float64}[T]


ESZ = {"f32": 4, "u8": 1, "u16": 2, "f64": 8}


class Arena:
    """One device byte buffer, never filled whole; views are handed out from its first byte (one image at a time)."""

    def __init__(self, nbytes):
        import torch
        assert nbytes <= ARENA_CAP, nbytes
        self.nbytes = (nbytes + 15) // 16 * 16
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def view(self, T, H, row, pitch, offset=0, guard=GUARD):
        """([H, row] image view, [H, guard] view of the elements behind every row) at row stride `pitch` elements, `offset` elements in"""
        import torch
        assert pitch >= row + guard and (offset + (H - 1) * pitch + row + guard) * ESZ[T] <= self.nbytes, (T, H, row, pitch, offset, self.nbytes)
        typed = self.buf.view(_torch_type(T))
        return torch.as_strided(typed, (H, row), (pitch, 1), offset), torch.as_strided(typed, (H, guard), (pitch, 1), offset + row)

    def free(self):
        import torch
        self.buf = None
        torch.cuda.empty_cache()


def to_device(img, T):
    """a host image [H, W] / [H, W, C] of type T as a device tensor [H, W C] (16-bit pixels travel as int16 bits)"""
    import torch
    flat = np.array(img).reshape(img.shape[0], -1)              # (a copy: the shared sources are read-only)
    return torch.from_numpy(flat.view(np.int16) if T == "u16" else flat).cuda()


def place_source(arena, img, T, pitch, offset=0):
    """the image at row stride `pitch` in the arena, the GUARD elements behind every row poisoned (NaN / all ones); returns its address"""
    H, row = img.shape[0], int(np.prod(img.shape[1:]))
    rows, guard = arena.view(T, H, row, pitch, offset)
    rows.copy_(to_device(img, T))
    guard.fill_(float("nan") if T in ("f32", "f64") else (255 if T == "u8" else -1))
    return rows.data_ptr()


def place_dst(arena, dH, drow, pitch, offset=0, T="f32"):
    """sentinel-filled dst rows (+ GUARD elements of padding) at row stride `pitch`; returns (address, rows view, padding view)"""
    rows, guard = arena.view(T, dH, drow, pitch, offset)
    rows.fill_(SENTINEL)
    guard.fill_(SENTINEL)
    return rows.data_ptr(), rows, guard


def tight_dst(dH, drow, batch=1):
    """a dst of its own with GUARD elements of sentinel padding per row: (tensor [B, dH, drow + GUARD], row stride, image stride)"""
    import torch
    t = torch.full((batch, dH, drow + GUARD), SENTINEL, dtype=torch.float32, device="cuda")
    return t, drow + GUARD, dH * (drow + GUARD)


def make_request(g, H, extra_policy=0):
    from area_average_interpolation_amd import _lib as L
    iso = iso_of(g, H)
    return L.Request(g.mode, g.policy | extra_policy, g.W, H, g.src_res, g.src_res, g.dst_res, g.dst_res, iso[0], iso[1], g.angle)


def resample(g, T, H, src_ptr, src_pitch, dst_ptr, dst_pitch, batch=1, src_image=0, dst_image=0, extra_policy=0):
    """aai_resample_batch_device (plain images) / aai_resample_interleaved_device on raw addresses, on torch's current stream; synchronises"""
    import torch
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    rq = make_request(g, H, extra_policy)
    st = torch.cuda.current_stream().cuda_stream
    if g.C == 1:
        rc = lib.aai_resample_batch_device(ctypes.byref(rq), batch, src_ptr, TYPES[T][2], src_pitch, src_image, dst_ptr, dst_pitch, dst_image, st)
    else:
        rc = lib.aai_resample_interleaved_device(ctypes.byref(rq), batch, g.C, src_ptr, TYPES[T][2], src_pitch, src_image, dst_ptr, dst_pitch, dst_image, st)
    try:
        if rc == L.ERR_HIP:
            raise RuntimeError(lib.aai_last_error().decode())
        torch.cuda.synchronize()
    except RuntimeError as e:
        # a device error: nothing more may be started on this GPU by this process
        import pytest
        pytest.exit("device error in %s %s H=%d src pitch %d dst pitch %d (%s): %s" % (g.name, T, H, src_pitch, dst_pitch, lib.aai_last_kernel().decode(), e), returncode=3)
    assert rc == 0, (rc, lib.aai_last_error().decode(), g.name, T, H, src_pitch, dst_pitch)
    return lib.aai_last_kernel().decode()


def family_of(kernel_name):
    """aai_last_kernel() -> the table's family names"""
    if kernel_name.startswith("aai_sample_kernel"):
        return kernel_name
    name = kernel_name.split("<")[0].split("+")[0]
    return "fp64" if name in ("aai_rotated_kernel", "aai_rotated_runs_kernel") else name


# families whose wide-pitch result must equal the tight control's bit for bit: their per-pixel arithmetic does not depend on the view
# (K1's tables, the samplers' taps, the double-precision kernels).  The fp32 window kernels sum a window in the order its loads arrive
# in, which the view's regime changes: they are held to the bar, and the largest difference from the control is printed.
def bit_exact_family(family):
    return family.startswith("aai_axis") or family.startswith("aai_sample") or family == "fp64"
