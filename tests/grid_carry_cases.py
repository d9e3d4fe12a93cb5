"""Shared by tests/test_grid_carry_host.py and tests/test_grid_carry_gpu.py: the geometries at which a launcher of csrc/ has to go
beyond ONE grid -- a second launch over row blocks (`for (b0 = 0; ...; b0 += 65535)`), a `while (blocksY > 65535) rows *= 2`, a
grid-stride loop over rows, a batch cut at kMaxGridZ or by the 1 GiB scratch rule of chunk_images() -- the limits themselves as read from
the constants of csrc/, and the row samples around a limit.  Needs neither torch nor a GPU.

A geometry is (W, H, source pixels per dst pixel side, angle, isocenter offset from the image centre); every one is tall and narrow, so
that the limit is crossed with tens of megabytes.  `edge` is the first row (source or dst, see `side`) that the second launch, the
second stride or the doubled row block takes."""
import collections
import os
import re

import numpy as np

import half_cases as hc
from conftest import ROOT

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

GRID_Y = 65535                         # blocks one grid dimension y / z carries


def csrc_constant(filename, name):
    """the integer value of `constexpr int <name> = <value>` in a file of csrc/ (several declarations on one line allowed)"""
    text = open(os.path.join(CSRC, filename)).read()
    m = re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*%s\s*=\s*(\d+)" % re.escape(name), text)
    assert m, (filename, name)
    return int(m.group(1))


# rows per block of the launchers that carry, as the sources state them (test_grid_carry_host.py holds them to csrc/)
AXIS_ADJOINT_ROWS = 32                 # kAxisAdjRows (aai_axis_adjoint.hip; the multi and the half launcher use the same constant)
PLAIN_TILE = 16                        # kPlainTile (aai_adjoint_plain.hip), kAdjMultiTile (aai_adjoint_multi.hip)
SCALE_ROWS = 4                         # kScaleRows: the element-wise pass of the planned adjoint at general rotations
CONVERT_ROWS = 4                       # convert_grid (aai_axis_narrow.hip), aai_axis_wide_kernel's launches, aai_axis_zero_kernel

EDGE_AXIS_ADJOINT = GRID_Y * AXIS_ADJOINT_ROWS       # 2,097,120 source rows
EDGE_PLAIN = GRID_Y * PLAIN_TILE                     # 1,048,560 dst or source rows
EDGE_ROWS4 = GRID_Y * CONVERT_ROWS                   # 262,140 rows

Geometry = collections.namedtuple("Geometry", "W H ratio angle off side edge what")

# side: which image's rows cross `edge` ("src" or "dst").
GEOMETRIES = collections.OrderedDict([
    ("A0", Geometry(5, 2097190, 2.0, 0.0, (0.0, 0.0), "src", EDGE_AXIS_ADJOINT, "separable, the direct narrow kernel serves")),
    ("A180", Geometry(5, 2097190, 2.0, 180.0, (0.0, 0.0), "src", EDGE_AXIS_ADJOINT, "A0 flipped: outBase holds (nB - 1) * outStrideB")),
    ("A90", Geometry(5, 2097190, 2.0, 90.0, (0.0, 0.0), "src", EDGE_AXIS_ADJOINT, "transposed, rows shared: a tall source, a wide gdst")),
    ("A270", Geometry(5, 2097190, 2.0, 270.0, (0.0, 0.0), "src", EDGE_AXIS_ADJOINT, "A90 flipped")),
    ("A11", Geometry(6, 2097190, 1.0, 0.0, (0.0, 0.0), "src", EDGE_AXIS_ADJOINT, "1:1, rows shared")),
    ("Wd", Geometry(3, 524420, 2.0, 0.0, (0.0, 0.0), "dst", EDGE_ROWS4, "wide: a source row of fewer than four elements")),
    ("N2", Geometry(8, 524420, 2.0, 0.0, (0.0, 0.0), "dst", EDGE_ROWS4, "direct narrow kernel, nB > 4 x 65535: rows doubled for 2-byte elements")),
    ("N2r", Geometry(8, 524420, 2.0, 180.0, (0.0, 0.0), "dst", EDGE_ROWS4, "N2 at 180 degrees: with channels the scattered store")),
    ("N8", Geometry(66, 524400, 1.0, 180.0, (0.0, 0.0), "dst", EDGE_ROWS4, "66 outputs per strip: u8 stays direct, rows doubled for 1-byte elements")),
    ("N8c", Geometry(22, 524400, 1.0, 180.0, (0.0, 0.0), "dst", EDGE_ROWS4, "N8 for three channels: 66 elements per strip (N8 itself has 198 there, 32 rows per workgroup, no doubling)")),
    ("R", Geometry(24, 1048700, 1.0, 0.003, (0.0, 0.0), "src", EDGE_PLAIN, "general rotation, canvas 79 x 1,048,700: source and dst rows carry")),
    ("Rup", Geometry(12, 524400, 0.5, 0.003, (0.0, 0.0), "dst", EDGE_PLAIN, "x2 up-sampling, canvas 79 x 1,048,800: only the dst side carries")),
    ("T", Geometry(40, 262300, 1.0, 0.01, (0.0, 0.0), "dst", EDGE_ROWS4, "general rotation on a forwarding route: widen and store carry")),
    ("Z", Geometry(7, 524420, 2.0, 0.0, (0.5, 0.0), "dst", EDGE_ROWS4, "the lane table's last entry is empty: aai_axis_zero_kernel over 262,210 rows")),
])


def iso_of(geo):
    return ((geo.W - 1) / 2.0 + geo.off[0], (geo.H - 1) / 2.0 + geo.off[1])


def args_of(geo):
    """(srcRes, dstRes, isocenter, angle) as the oracle and make_request take them"""
    return geo.ratio, 1.0, iso_of(geo), geo.angle


def request(aai, name, mode_name="area", height=None):
    """the request of a named geometry (or of a Geometry); height: the same geometry at another height, isocenter at its centre"""
    geo = GEOMETRIES[name] if isinstance(name, str) else name
    if height is not None:
        geo = geo._replace(H=int(height))
    return aai.make_request(geo.W, geo.H, geo.ratio, 1.0, iso_of(geo), geo.angle, mode=hc.mode_of(aai, mode_name))


def boundary_rows(edge, n):
    """rows edge - 33 ... edge + 33 around the first carried row, and rows 0, 1, n - 2, n - 1; those inside [0, n), ascending"""
    rows = set(range(edge - 33, edge + 34)) | {0, 1, n - 2, n - 1}
    return sorted(r for r in rows if 0 <= r < n)


def row_runs(rows):
    """[(r0, r1)): the maximal runs of consecutive rows of an ascending list"""
    runs = []
    for r in rows:
        if runs and runs[-1][1] == r:
            runs[-1][1] = r + 1
        else:
            runs.append([r, r + 1])
    return [tuple(r) for r in runs]


def oracle_at_rows(po, omode, src_f32, geo, rows, dst_width):
    """the oracle's dst rows `rows` (ascending) of a float32 [H, W] source -> float64 [len(rows), dst_width]"""
    sr, dr, iso, ang = args_of(geo)
    return np.concatenate([po.oracle_rows(omode, src_f32, sr, dr, iso, ang, r0, r1, dst_width) for r0, r1 in row_runs(rows)], axis=0)


def rows_pixels(W, rows, seed):
    """every listed row at columns 0, 15, 16, W-1 and two seeded ones"""
    rng = np.random.default_rng(seed)
    px = []
    for r in rows:
        cols = [0, 15, 16, W - 1] + [int(c) for c in rng.integers(1, W - 1, 2)]
        px += [(c, r) for c in dict.fromkeys(c for c in cols if 0 <= c < W)]
    return np.array([p[0] for p in px]), np.array([p[1] for p in px])


def forward_rows(dH):
    """the dst rows the forward tests sample: the boundary rows of every limit below the image's height"""
    rows = set()
    for edge in (EDGE_ROWS4, EDGE_PLAIN):
        if edge + 33 < dH:
            rows |= set(boundary_rows(edge, dH))
    return sorted(rows)


def chunk_images(batch, image_bytes):
    """chunk_images() of csrc/aai_engine.hpp restated: what grid.z carries, cut so that the scratch stays within 1 GiB; at least one"""
    chunk = max(0, min(batch, GRID_Y))
    if image_bytes:
        chunk = min(chunk, (1 << 30) // image_bytes)
    return max(1, chunk)


def round256(nbytes):
    return (nbytes + 255) & ~255


# ---- axis_launch_shape over a sweep (the probe takes a request: nB is produced by the image height) --------------------------------
SWEEP_NB = sorted({GRID_Y * r + d for r in (1, 2, 4, 8, 16, 32, 64) for d in (-1, 0, 1)} | {2097190, 8400000})
SWEEP_ELEM = (1, 2, 4)
# (channels, W, source pixels per dst pixel side, the class of maxOutputsPerStrip it must land in: outputs are counted in elements,
# pixels x channels).  build_axis_strips (csrc/aai_plan.cpp) ends a strip at 256 outputs, so a class above 256 does not exist: the
# up-sampling rows (nB = 2 H; an odd nB of the sweep is produced as nB + 1) land in 129..256 and are asserted to.
SWEEP_STRIPS = ((1, 50, 1.0, (1, 64)), (1, 100, 1.0, (65, 128)), (1, 200, 1.0, (129, 256)), (1, 200, 0.5, (129, 256)),
                (3, 20, 1.0, (1, 64)), (3, 40, 1.0, (65, 128)), (3, 70, 1.0, (129, 256)), (3, 100, 0.5, (129, 256)))
