"""Which kernel, launch shape and strip path of the axis-aligned family K1 (csrc/aai_axis.hip) serves a request, and a table of test
cases that reaches every one of them (helper of test_axis_variants_host.py / test_axis_variants_gpu.py; needs no GPU).

launch_axis_typed launches what axis_launch_shape (csrc/aai_plan.hpp) says:

    aai_axis_kernel        <NT, T, CH>    five branches per strip (A..E in the order of the source), `rows` output rows per workgroup
    aai_axis_tile_kernel   <NT, T>        two pipelines: tile_columns<.., NR 4, depth 8> and <.., NR 8, depth 4>
    aai_axis_wide_kernel   <T>

aai_last_kernel() names the kernel only.  The variant probe aai_emu_axis_variant (tests/emulation/host_emulation.cpp) builds the
request's tables as the plan does, asks axis_launch_shape, and walks the strips, workgroups, waves and lanes of the launch: which
branches the strips take, how often the kb0 loops of branches A and B run, which of their store shapes occur, the tile kernel's
pipeline, its nq values and nCols classes, the right-edge shifts.  No launch rule is restated here: this file names the probe's
fields, walks a grid and picks cases.

CANDIDATES: the set of (kernel, T, C > 1, nt, strip branch | tile NR | wide kind, rows class, direction of outStrideB, store shape |
nCols class) the probe reports over GRID.  The rows class (one or several iterations of the kb0 loop) and the store shape exist for
branches A and B, the direction for A, B and the tile kernel; the tile kernel and branch B have further candidates of their own, one
per nq = outputs per lane (1..4, B: 2..4) their strips have, in the place of the rows class.  The wide kernel has two candidates per type: a source row of fewer
than four elements, and a footprint wider than a strip.

CASES: per candidate the grid point with the fewest source pixels (to within a row of eight columns; ties go round the tied points
by the candidate's index, so that widths, isocenters and heights all occur) among the points whose smallest lane weight times
smallest row weight is at least MIN_WEIGHT -- then one dropped, doubled or misplaced source element moves a pixel by at least
1e-3 x 0.25 / 1.25 = 2e-4 relative, twenty times the 1e-5 bar (case_source: noise in [0.25, 1.25)).  BIG: five large cases (seven
launches), for what no small request reaches -- branch B and a second iteration of A's loop need more than 1,048,560 output rows at
90 / 270 degrees, the rows-per-workgroup escalation of 8- / 16-bit sources needs 2048 workgroups.  The scan classifies them through the probe like every
grid point; their weights are about a half.  (The wide kernel's wide-footprint candidate cannot meet MIN_WEIGHT, see eligible: its
case shows the 1e-5 bar and not more -- one dropped tap of 280 x 280 moves a pixel by about 1e-5; test_gpu_parity.py and
test_gpu_memory_contract.py run that kernel at other footprints.)

NOT covered: the five launch shapes tune_axis_plan (csrc/aai_engine.cpp) measures on the device for large fp32 streaming requests
(rows 1 / 2 / 4, nt 0 / 1).  Which one such a request runs with depends on the device it runs on and nothing forces one; the probe
asks for the built-in shape (tuneRows = 0), which every request below 64 MiB of source has.  test_axis_kernel_at_size
(test_gpu_parity.py) covers "whatever this device measured".
"""
import collections
import ctypes
import math
import struct

import numpy as np

# ---- the probe ------------------------------------------------------------------------------------------------------------------
FIELDS = ("kernel", "nt", "rows", "tile_nr", "n_strips", "nA", "nB", "max_outputs", "max_row_span", "rows_shared", "transposed",
          "sign_a", "sign_b", "out_chan", "branches", "a_iters", "a_stores", "b_iters", "b_stores", "tile_nq", "tile_ncols", "tile_tall",
          "shifts", "last_wg_short", "min_lane_w", "min_row_w", "dW", "dH", "grid_x", "grid_y", "b_nq")            # enum AxisVariantField
Variant = collections.namedtuple("Variant", FIELDS)
KERNELS = {1: "aai_axis_kernel", 2: "aai_axis_tile_kernel", 3: "aai_axis_wide_kernel"}                     # enum AxisKernelKind
BRANCHES = "ABCDE"                                                                                          # enum AxisStripBranch
A_STORES = ("8", "4", "2", "1")          # bits of a_stores: dst columns per store of branch A
B_STORES = ("4", "1")                    # bits of b_stores
NCOLS = ("16", "depth..15", "1..depth-1", "0")        # bits of tile_ncols: a wave's output rows against its pipeline's depth
MODE_AREA, MODE_FAST = 1, 2
TYPES = {"f32": (np.float32, 4, 0, 1.0), "u8": (np.uint8, 1, 1, 256.0), "u16": (np.uint16, 2, 2, 65536.0)}     # numpy type, bytes, AAI_DTYPE_*, value scale
CHANNELS = (1, 2, 3, 4)
MIN_WEIGHT = 1e-3
ISO_OFFSET = (0.3137, -0.2113)           # isocenter - image centre of the "off" cases: consecutive output rows share source rows


def bind(lib):
    """lib: the CDLL of tests/emulation/host_emulation.cpp (conftest's hostemu fixture)"""
    from area_average_interpolation_amd import _lib as L
    lib.aai_emu_axis_variant.restype = ctypes.c_int
    lib.aai_emu_axis_variant.argtypes = [ctypes.POINTER(L.Request)] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    lib.aai_emu_axis_fixups.restype = ctypes.c_long
    lib.aai_emu_axis_fixups.argtypes = []
    return lib


def _as_float(bits):
    return struct.unpack("f", struct.pack("i", bits))[0]


class Prober:
    def __init__(self, lib):
        from area_average_interpolation_amd import _lib as L
        self.lib = bind(lib)
        self.out = (ctypes.c_int * len(FIELDS))()
        self.rq = L.Request(1, 0, 64, 64, 1.0, 1.0, 1.0, 1.0, 31.5, 31.5, 0.0)
        self.calls = 0

    def __call__(self, W, H, ratio, angle, mode, iso, C, esz, batch, band=(-1, -1)):
        rq = self.rq
        rq.mode, rq.policy, rq.src_width, rq.src_height = mode, 0, W, H
        rq.src_res_x = rq.src_res_y = ratio
        rq.dst_res_x = rq.dst_res_y = 1.0
        rq.src_iso_x, rq.src_iso_y, rq.rotation_deg = iso[0], iso[1], angle
        rc = self.lib.aai_emu_axis_variant(ctypes.byref(rq), C, esz, batch, band[0], band[1], self.out)
        assert rc == 0, (rc, W, H, ratio, angle, band)
        self.calls += 1
        v = Variant(*self.out)
        return v._replace(min_lane_w=_as_float(v.min_lane_w), min_row_w=_as_float(v.min_row_w))


# (kernel, T, C > 1, nt, branch "A".."E" | tile NR 4 / 8 | wide kind, rows class "" / "1" / "n" | an nq of the tile kernel "nq3", direction of outStrideB 0 / +1 / -1, store shape | nCols class | "")
Candidate = collections.namedtuple("Candidate", "kernel T multi nt sub rows_class dir_b shape")


def _bits(mask, names):
    return [n for i, n in enumerate(names) if mask >> i & 1]


def hosted(v, T, C, W):
    """the candidates one launch (a probe result) hosts"""
    kernel = KERNELS.get(v.kernel)
    multi = int(C > 1)
    found = set()
    if kernel == "aai_axis_wide_kernel":
        found.add(Candidate(kernel, T, multi, 0, "narrow" if W * C < 4 else "footprint", "", 0, ""))
    elif kernel == "aai_axis_tile_kernel":
        for shape in _bits(v.tile_ncols, NCOLS):
            found.add(Candidate(kernel, T, multi, v.nt, "NR%d" % v.tile_nr, "", v.sign_b, shape))
        for nq in _bits(v.tile_nq, "1234"):
            found.add(Candidate(kernel, T, multi, v.nt, "NR%d" % v.tile_nr, "nq" + nq, 0, ""))
    elif kernel == "aai_axis_kernel":
        for b in _bits(v.branches, BRANCHES):
            if b == "A":
                for shape in _bits(v.a_stores, A_STORES):
                    found.add(Candidate(kernel, T, multi, v.nt, b, "1" if v.a_iters == 1 else "n", v.sign_b, shape))
            elif b == "B":
                for shape in _bits(v.b_stores, B_STORES):
                    found.add(Candidate(kernel, T, multi, v.nt, b, "1" if v.b_iters == 1 else "n", v.sign_b, shape))
                for nq in _bits(v.b_nq, "1234"):
                    found.add(Candidate(kernel, T, multi, v.nt, b, "nq" + nq, 0, ""))
            else:
                found.add(Candidate(kernel, T, multi, v.nt, b, "", 0, ""))
    return found


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
# ratio = source pixels per dst pixel side: x4 up-sampling ... 12:1, crossing 1, 2, 3, 4 and 8 from both sides (the kernels change
# path where a strip's outputs cross 64, 128 and 256 and where the windows' row counts cross 2, 3, 4 and 8)
RATIOS = (0.25, 0.5, 0.75, 0.9, 0.95, 1.0, 1.05, 10.0 / 9.0, 1.5, 1.9, 1.95, 2.0, 2.05, 2.1, 2.5, 2.9, 2.95, 3.0, 3.05, 3.1, 3.5, 3.7, 3.9,
          3.95, 4.0, 4.05, 4.1, 5.0, 6.0, 7.0, 7.9, 7.95, 8.0, 8.05, 8.1, 10.0, 12.0)
QUADRANTS = (0, 1, 2, 3)
WIDTHS = (300, 301, 302, 303)            # two strips and a right edge at every residue of W x C mod 4 (C = 2: the even ones)
NARROW = (50, 51, 52, 53)                # at most 64 outputs per strip below 4:1 too (90 / 270 degrees, one channel)
# output rows asked for (the source's height follows): every residue mod 16 -- the tile kernel's waves take 16, its workgroups 64, the
# strip kernel's register paths 8, 4 or 2 -- and always a second workgroup of the tile kernel
NB_TRANSPOSED = tuple(range(65, 81))
NB_OTHER = (66, 69)
BATCH = 2                                # what the GPU module launches: the image and its flip
OTHER_BATCHES = (1, 4096)                # one image; more than enough workgroups for the 8- / 16-bit escalation (isocenter at the centre, first width)
# the wide kernel: a source row of fewer than four elements; a footprint wider than a strip (280 source columns per dst pixel)
WIDE_POINTS = ((3, 40, 1.0), (2, 40, 1.0), (1, 40, 1.0), (600, 300, 280.0))
GRID = "ratio %g..%g (%d values) x 0 / 90 / 180 / 270 degrees x {area, fast} x {f32, u8, u16} x C in 1..4 x isocenter {centre, centre + %r} x W in %r (+ %r transposed) x %d heights, batch %d (+ %r)" % (
    RATIOS[0], RATIOS[-1], len(RATIOS), ISO_OFFSET, WIDTHS, NARROW, len(NB_TRANSPOSED), BATCH, OTHER_BATCHES)

Point = collections.namedtuple("Point", "W H ratio angle mode off C T batch")


def iso_of(W, H, off):
    return ((W - 1) / 2.0 + (ISO_OFFSET[0] if off else 0.0), (H - 1) / 2.0 + (ISO_OFFSET[1] if off else 0.0))


def grid_points(types=tuple(TYPES), channels=CHANNELS):
    for T in types:
        for C in channels:
            for mode in (MODE_AREA, MODE_FAST):
                for q in QUADRANTS:
                    plain_transposed = C == 1 and q & 1
                    for ratio in RATIOS:
                        for W in WIDTHS + (NARROW if plain_transposed else ()):
                            for nB in (NB_TRANSPOSED if plain_transposed else NB_OTHER):
                                H = max(2, int(math.ceil(nB * ratio)))
                                for off in (0, 1):
                                    yield Point(W, H, ratio, 90.0 * q, mode, off, C, T, BATCH)
                                    if not off and W == WIDTHS[0] and nB == NB_OTHER[0]:
                                        for batch in OTHER_BATCHES:
                                            yield Point(W, H, ratio, 90.0 * q, mode, off, C, T, batch)
                    for (W, H, ratio) in WIDE_POINTS:
                        yield Point(W, H, ratio, 90.0 * q, mode, 0, C, T, BATCH)


# The large cases (five, seven launches: a and b at both transposed angles): name -> grid point.
#   a  branch B, forward and reverse stores, rows 4 -> 32 = eight iterations of its loop.  The sources are one and two rows taller than
#      1,048,600, so that the last workgroup ends on a chunk of one / two output rows: B's scalar tail beside its 16-byte stores
#   e  branch B with 200 outputs per strip: four outputs per lane (nq = 4; a has two), so its third and fourth horizontal pass run.
#      nq = 3 (129..192 outputs per strip) takes the same passes but for the fourth and is not among the cases
#   b  branch A, rows 8 -> 32, four iterations of its loop
#   c / d  the escalation of 8- / 16-bit sources to 8 / 4 rows per workgroup
BIG = collections.OrderedDict([
    ("a270", Point(100, 1048601, 1.0, 270.0, MODE_AREA, 0, 1, "u8", 1)), ("a90", Point(100, 1048602, 1.0, 90.0, MODE_AREA, 0, 1, "u8", 1)),
    ("e270", Point(200, 1048601, 1.0, 270.0, MODE_AREA, 0, 1, "u8", 1)),
    ("b90", Point(40, 1100000, 1.0, 90.0, MODE_AREA, 0, 1, "f32", 1)), ("b270", Point(40, 1100000, 1.0, 270.0, MODE_AREA, 0, 1, "f32", 1)),
    ("c", Point(1024, 4096, 4.0, 0.0, MODE_AREA, 0, 1, "u8", 16)), ("d", Point(1024, 4096, 4.0, 0.0, MODE_AREA, 0, 1, "u16", 16)),
])


def _cost(p):
    return (p.W // 8) * p.H


def probe_point(probe, p, band=(-1, -1)):
    return probe(p.W, p.H, p.ratio, p.angle, p.mode, iso_of(p.W, p.H, p.off), p.C, TYPES[p.T][1], p.batch, band)


def eligible(v):
    """a point a small case may sit on: derived sensitivity (module text), and nothing a tile pipeline was not built for"""
    if KERNELS.get(v.kernel) == "aai_axis_wide_kernel" and v.max_outputs <= 4 and v.min_lane_w < 1.0 / 256:
        # a footprint wider than a strip has more than 256 x 256 taps: no weight of it reaches MIN_WEIGHT, whatever the geometry.  The
        # one condition the table waives; that candidate's case checks the bar and not more.
        return True
    return v.min_lane_w * v.min_row_w >= MIN_WEIGHT and not v.tile_tall


def scan_grid(probe, types=tuple(TYPES), channels=CHANNELS):
    """(candidate -> [its cheapest eligible points at batch BATCH], candidate -> [names of the big cases that host it], any `tall` window seen)"""
    cands, big, tall = {}, {}, []
    for p in grid_points(types, channels):
        v = probe_point(probe, p)
        if v.tile_tall:
            tall.append(p)
        for cand in hosted(v, p.T, p.C, p.W):
            if (p.W, p.H, p.ratio) in WIDE_POINTS and cand.kernel != "aai_axis_wide_kernel":
                continue                 # (a source row of exactly four elements: nothing to learn about the strip kernel from it)
            pts = cands.setdefault(cand, [])
            if p.batch == BATCH and eligible(v):
                # (kept: the cheapest points only, all that tie)
                if pts and _cost(p) < _cost(pts[0]):
                    del pts[:]
                if not pts or _cost(p) == _cost(pts[0]):
                    pts.append(p)
    for name, p in BIG.items():
        if p.T in types and p.C in channels:
            v = probe_point(probe, p)
            if v.tile_tall:
                tall.append(p)
            for cand in hosted(v, p.T, p.C, p.W):
                big.setdefault(cand, []).append(name)
    return cands, big, tall


# ---- cases ------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "index cand point dW dH")


def build_cases(probe, cands, big):
    """one small case per candidate some eligible grid point hosts; a candidate without one must be hosted by a big case"""
    cases = []
    for k, cand in enumerate(sorted(cands)):
        pts = cands[cand]
        if not pts:
            assert cand in big, ("no grid point with weights of at least %g hosts this candidate" % MIN_WEIGHT, cand)
            continue
        tied = sorted(pts)
        p = tied[k % len(tied)]
        v = probe_point(probe, p)
        cases.append(Case(len(cases), cand, p, v.dW, v.dH))
    return cases


_TABLE = {}


def table(lib):
    """(candidates, big, tall, cases, probe) -- built once per process"""
    if "t" not in _TABLE:
        probe = Prober(lib)
        cands, big, tall = scan_grid(probe)
        _TABLE["t"] = (cands, big, tall, build_cases(probe, cands, big), probe)
    return _TABLE["t"]


def bands_of(dH, rows=64):
    """dst row bands of at most `rows` rows"""
    return [(r0, min(r0 + rows, dH)) for r0 in range(0, dH, rows)]


# ---- data and reference of a case -----------------------------------------------------------------------------------------------
def case_source(case, flip=False):
    """the case's source image: [H, W] or [H, W, C] of its type; noise well away from zero (exact zeros are the canvas borders')"""
    p = case.point
    npdt, _, _, hi = TYPES[p.T]
    rng = np.random.default_rng(1000 + case.index)
    shape = (p.H, p.W) if p.C == 1 else (p.H, p.W, p.C)
    src = (rng.random(shape, dtype=np.float32) + np.float32(0.25)) if npdt == np.float32 else rng.integers(1, int(hi), size=shape).astype(npdt)
    return np.ascontiguousarray(src[::-1]) if flip else src


def case_gold(po, case, src):
    """the oracle on the case's source, per channel: [dH, dW] or [dH, dW, C] float64"""
    p = case.point
    omode = po.MODE_EXACT if p.mode == MODE_AREA else po.MODE_FAST
    run = lambda plane: po.oracle_run(omode, np.ascontiguousarray(plane, dtype=np.float64), p.ratio, 1.0, iso_of(p.W, p.H, p.off), p.angle).dst
    if src.ndim == 2:
        return run(src)
    return np.stack([run(src[:, :, c]) for c in range(src.shape[2])], axis=2)


def cand_id(c):
    return "%s<%s,C%s,nt%d,%s,rows:%s,dir%+d,%s>" % (c.kernel, c.T, ">1" if c.multi else "1", c.nt, c.sub, c.rows_class or "-", c.dir_b, c.shape or "-")


def case_id(case):
    p = case.point
    return "%s %dx%dx%d %g:1 at %g mode %d iso %s" % (cand_id(case.cand), p.W, p.H, p.C, p.ratio, p.angle, p.mode, "off" if p.off else "centre")
