"""The typed entries in WIDE-PITCH buffers: the case table that takes the half, integer, convert and half-adjoint entries -- whose kernels
read and write the caller's pitched images in element types other than fp32 -- through the offset products of their hand-written
address arithmetic (helper of test_wide_pitch_typed_host.py / test_wide_pitch_typed_gpu.py; needs no GPU to import).  The method, the
arena and the pitch classes are tests/wide_pitch.py's: a narrow, tall image placed at a row stride of megabytes.

    entry (api.py)                     direct kernel                    forwarding stages that touch the caller's image
    resample_half_device               aai_axis_narrow_kernel           aai_narrow_widen_kernel, aai_narrow_store_kernel   (+widened)
    resample_half_interleaved_device   aai_axis_narrow_kernel           the same
    resample_int_device                aai_axis_narrow_kernel           the fp32 entry reads it, aai_narrow_store_kernel    (+quantized)
    resample_convert_device            aai_axis_convert_kernel          the fp32 entry reads it, aai_convert_store_kernel   (+converted)
    adjoint_half_device                aai_axis_adjoint_half_kernel     widen, the fp32 adjoint, narrow store               (+widened)

The products a row is there for: row x rowStride (vertical_pass, the stores' kb x outStrideB / kb x rowStep, the converters' y x
rowStride), blockIdx.z x imageStride, c x planeStride, and the engine's b0 x imageStride x elem advances -- each beyond 2^31 elements or
2^32 bytes.  They are written in int64_t; a 32-bit product at these sizes addresses another row of the same allocation, silently.

A ROW of the table = a configuration (entry, element type, output type and layout, channels, shape, angle, mode) x a side x a class:
    src        the image the entry READS is wide (the source; gdst for the adjoint)
    dst        the image the entry WRITES is wide
    plane      planar convert only: tight rows, the plane stride just past 2^31 elements
    batch-src  a batch of two, tight rows + GUARD, the second image wide_pitch.batch_apart elements behind the first, on the side read
    batch-dst  ... on the side written
    grid-src   a batch of 65537 tiny images 32771 elements apart on the side read: the engine's second round of launches starts beyond
               2^31 elements
    grid-dst   ... on the side written
    G          the last rows START beyond 2^32 bytes (on the src side of the forward entries, whose images have 530 rows and more: at a
               pitch below 8 MiB).  For 2-byte elements that is 2^31 elements, for u8 2^32
    GP         pitch >= 2^23 bytes (the forwarded fp32 entry changes form there); the rows from 512 on start beyond 2^32 bytes
    E31        the last rows start beyond 2^31 ELEMENTS -- a signed 32-bit element offset wraps, an unsigned one does not: u8 sources
               (below 4 GiB) and, on the dst side, the fp32 output of convert (8.6 GB: fp32 reaches 2^32 bytes at 2^30 elements)
The pitches are wide_pitch.pitch_for's, asked for the rows that must lie below the threshold (pitch_of): a product row x stride that
lost its 64 bits addresses another element from those rows on.
The ROUTE of a configuration is asked of the predicates the typed suites already have (int_cases.direct, convert_cases.direct,
half_cases.facts, half_interleaved_cases.facts, adjoint_half_cases.serves_direct): nothing of the dispatch is restated here.  A row
records the name aai_last_kernel() must report -- the direct kernel's, or the suffix of the forwarding route.

SHAPES (rows of at most 640 elements, 560 source rows; the up-sampling shape 530, so that no image has more than 1100 rows).  The
isocentre sits off the lattice by wide_pitch.OFF -- no edge of a dst pixel runs through a source pixel's corner, the plan lists no
pixel --; the shapes named ...y keep the x component only: with y on the lattice no two output rows share a source row, which is what
selects the kernels' nontemporal loads (an offset in y always shares the boundary row).
"""
import collections

import numpy as np

import adjoint_half_cases as ac
import convert_cases as cc
import half_cases as hc
import half_interleaved_cases as hic
import int_cases as ic
import wide_pitch as wp

HT = {"f16": hc.F16, "bf16": hc.BF16}
DT = {"u8": ic.U8, "u16": ic.U16}
OT = {"f32": cc.F32, "f16": cc.F16, "bf16": cc.BF16}
LAY = {"nhwc": cc.INTERLEAVED, "nchw": cc.PLANAR}
ESZ = {"u8": 1, "u16": 2, "f16": 2, "bf16": 2, "f32": 4}
NP = {"u8": np.uint8, "u16": np.uint16, "f16": np.uint16, "bf16": np.uint16, "f32": np.float32}      # (fp16 / bf16 as raw 16-bit elements)
SUFFIX = {"half": "+widened", "half-il": "+widened", "int": "+quantized", "convert": "+converted", "adjoint": "+widened"}
ENTRIES = ("half", "half-il", "int", "convert", "adjoint")
PATTERN = 0xA5                # every byte of an image that is written, and of the GUARD elements behind its rows, before the call

# ---- shapes -------------------------------------------------------------------------------------------------------------------------
# row: elements of a source row (the image is row // channels pixels wide)
Shape = collections.namedtuple("Shape", "name row H src_res dst_res iso_off")
OFF_X = (wp.OFF[0], 0.0)
UP_H = 530
SHAPES = {s.name: s for s in (
    Shape("r4", 520, wp.TALL, 4.0, 1.0, wp.OFF),          # 4 : 1: at most 64 outputs per strip; the boundary row is shared: cached loads
    Shape("r4y", 520, wp.TALL, 4.0, 1.0, OFF_X),          # ... windows of 4 rows that share nothing: nontemporal loads
    Shape("r2", 300, wp.TALL, 2.0, 1.0, wp.OFF),          # 2 : 1: 65..256 outputs per strip, two strips
    Shape("r2y", 300, wp.TALL, 2.0, 1.0, OFF_X),
    Shape("up", 100, UP_H, 1.0, 2.0, wp.OFF),             # 1 : 2 up-sampling: one strip of about 200 outputs, 1060 output rows
    Shape("up2", 100, 280, 1.0, 2.0, wp.OFF),             # ... with 560 output rows: the half adjoint's gdst at 8 MiB a row stays below 5 GB
    Shape("tiny", 8, 6, 2.0, 1.0, wp.OFF),                # for the batches beyond one launch's grid.z
    Shape("rot", 240, wp.TALL, 3.0, 1.0, wp.OFF),         # for the general rotation
    Shape("smp", 200, wp.TALL, 2.0, 1.0, wp.OFF),         # for the sampler mode
)}

# ---- configurations -------------------------------------------------------------------------------------------------------------------
# T: the element type of the image read (and written, but for convert); out / layout: convert only
Config = collections.namedtuple("Config", "entry T out layout C shape angle mode")


def _h(T, shape, angle, mode="area"):
    return Config("half", T, None, None, 1, shape, float(angle), mode)


def _hi(T, C, shape, angle, mode="area"):
    return Config("half-il", T, None, None, C, shape, float(angle), mode)


def _i(T, C, shape, angle, mode="area"):
    return Config("int", T, None, None, C, shape, float(angle), mode)


def _c(T, out, layout, C, shape, angle, mode="area"):
    return Config("convert", T, out, layout, C, shape, float(angle), mode)


def _a(T, C, shape, angle, mode="area"):
    return Config("adjoint", T, None, None, C, shape, float(angle), mode)


S_D = (("src", "G"), ("dst", "G"))
S_P_D = (("src", "G"), ("src", "GP"), ("dst", "G"))
# (configuration, its (side, class) pairs); u8 configurations get ("src", "E31") on top (rows())
CONFIGS = (
    # resample_half_device: one channel -- the pair store at 4 : 1, packed forwards (0 degrees) and backwards (180)
    (_h("f16", "r4", 0), S_D), (_h("bf16", "r4y", 180, "fast"), S_P_D), (_h("bf16", "r2", 0, "fast"), S_D), (_h("f16", "r2y", 180), S_D),
    (_h("f16", "up", 180), S_D), (_h("bf16", "up", 0), (("src", "GP"),)),
    # ... forwarding: transposed, a general rotation
    (_h("f16", "r2", 90), S_P_D), (_h("bf16", "rot", 17.5), S_D),
    # resample_half_interleaved_device: the quad store, packed at 0 degrees and scattered at 180
    (_hi("f16", 3, "r4", 0), S_D), (_hi("bf16", 4, "r4y", 180, "fast"), S_D), (_hi("bf16", 3, "r2", 180), S_P_D), (_hi("f16", 4, "r2y", 0, "fast"), S_D),
    (_hi("f16", 2, "up", 0), S_D), (_hi("bf16", 3, "up", 180), (("dst", "G"),)),
    (_hi("bf16", 3, "r2", 90), S_D), (_hi("f16", 3, "rot", 17.5), S_P_D),
    # resample_int_device (u8 at 4 : 1 forwards by measurement)
    (_i("u16", 1, "r4", 0), S_D), (_i("u16", 3, "r4y", 180, "fast"), S_P_D), (_i("u8", 1, "r2", 180), S_P_D), (_i("u8", 3, "r2y", 0, "fast"), S_D),
    (_i("u8", 4, "up", 180), S_D), (_i("u16", 4, "r2", 0), S_D), (_i("u16", 1, "up", 0), (("src", "GP"), ("dst", "G"))),
    (_i("u8", 1, "r4", 0), S_P_D), (_i("u8", 3, "r4y", 180, "fast"), S_D), (_i("u16", 1, "r2", 90), S_D), (_i("u8", 3, "rot", 17.5), S_P_D),
    (_i("u16", 1, "rot", 17.5), (("src", "G"),)), (_i("u8", 1, "smp", 17.5, "bilinear"), S_P_D),
    # resample_convert_device: every (source type, layout) on the direct kernel, every output type once per layout
    (_c("u8", "f32", "nhwc", 3, "r4", 0), S_D), (_c("u8", "f32", "nchw", 3, "r2", 180), S_P_D), (_c("u8", "f16", "nhwc", 1, "r2", 0), S_D),
    (_c("u8", "f16", "nchw", 4, "r2y", 0, "fast"), S_D), (_c("u8", "bf16", "nhwc", 3, "r2", 180), S_D), (_c("u8", "bf16", "nchw", 3, "r4", 0), S_D),
    (_c("u16", "f32", "nhwc", 1, "r4", 180), S_P_D + (("dst", "E31"),)), (_c("u16", "f16", "nhwc", 4, "up", 180), S_D), (_c("u16", "bf16", "nhwc", 1, "r4y", 0, "fast"), S_D),
    (_c("u16", "f32", "nchw", 2, "r4y", 180), S_D + (("plane", "E31"),)), (_c("u16", "f16", "nchw", 3, "up", 0), S_D), (_c("u16", "bf16", "nchw", 3, "r2y", 180, "fast"), S_D),
    # ... forwarding: two classes the measured table forwards, transposed, a general rotation, a sampler
    (_c("u8", "f32", "nhwc", 3, "r2", 0), S_D), (_c("u8", "f16", "nchw", 3, "r4", 180), S_D), (_c("u16", "f16", "nhwc", 3, "r2", 90), S_D),
    (_c("u8", "bf16", "nchw", 3, "rot", 17.5), S_P_D + (("plane", "E31"),)), (_c("u16", "f32", "nhwc", 1, "rot", 17.5), S_D + (("dst", "E31"),)),
    (_c("u8", "f32", "nchw", 3, "smp", 17.5, "bilinear"), S_P_D),
    # adjoint_half_device: all four quadrants with 1 and 3 channels (outStrideA = +- the dst stride in the transposed ones)
    (_a("f16", 1, "r2", 0), S_D), (_a("bf16", 3, "r2", 90), S_D), (_a("bf16", 1, "r4", 180, "fast"), S_D), (_a("f16", 3, "r4y", 270), S_D),
    (_a("f16", 1, "r2y", 90, "fast"), S_D), (_a("bf16", 3, "up2", 0), S_P_D), (_a("bf16", 1, "r4", 270), S_D), (_a("f16", 3, "r2", 180), S_D),
    # ... the one class that forwards: a single channel, up-sampling, 90 degrees (its gdst has 200 rows: no GP row, which needs 512)
    (_a("f16", 1, "up", 90), S_D),
)
# (configuration, sides): a batch of two on the side read and / or written -- one direct row per kernel, one forwarding row per converter
BATCHES = (
    (_hi("bf16", 3, "r2", 180), ("batch-src", "batch-dst")),                 # aai_axis_narrow_kernel
    (_i("u8", 3, "r2y", 0, "fast"), ("batch-src",)),                          # ... a u8 source 2^32 elements apart
    (_c("u16", "f32", "nhwc", 1, "r4", 180), ("batch-src", "batch-dst")),    # aai_axis_convert_kernel
    (_c("u16", "bf16", "nchw", 3, "r2y", 180, "fast"), ("batch-dst",)),      # ... planar
    (_a("bf16", 3, "r2", 90), ("batch-src", "batch-dst")),                   # aai_axis_adjoint_half_kernel
    (_h("f16", "r2", 90), ("batch-src", "batch-dst")),                       # aai_narrow_widen_kernel / aai_narrow_store_kernel
    (_i("u8", 3, "rot", 17.5), ("batch-src", "batch-dst")),                  # the fp32 entry / aai_narrow_store_kernel
    (_c("u16", "f32", "nhwc", 1, "rot", 17.5), ("batch-dst",)),              # aai_convert_store_kernel
    (_a("f16", 1, "up", 90), ("batch-src", "batch-dst")),                    # widen / narrow store around the fp32 adjoint
)


# (configuration, sides): a batch of GRID_IMAGES tiny images GRID_APART elements apart, which the engine splits into two rounds of launches
# (65535 images: what grid.z carries) -- the second round starts at b0 x imageStride x elem = 65535 x GRID_APART elements, beyond 2^31, in
# enqueue_narrow, enqueue_convert, enqueue_adjoint_half and, on the forwarding routes, NarrowSide::image and the convert store's advance
GRID_IMAGES = 65535 + 2
GRID_APART = 32771
GRIDS = (
    (_hi("bf16", 2, "tiny", 180), ("grid-src", "grid-dst")),                  # enqueue_narrow, direct
    (_c("u16", "f16", "nchw", 2, "tiny", 0), ("grid-src", "grid-dst")),       # enqueue_convert, direct
    (_a("f16", 1, "tiny", 90), ("grid-src", "grid-dst")),                     # enqueue_adjoint_half, direct
    (_h("f16", "tiny", 90), ("grid-src", "grid-dst")),                        # NarrowSide::image, read and written
    (_c("u8", "f32", "nhwc", 1, "tiny", 90), ("grid-dst",)),                  # enqueue_convert's store, fp32 out: 8.6 GB
)


def config_id(c):
    return "%s-%s%s-x%d-%s/%g-%s" % (c.entry, c.T, ("-%s-%s" % (c.out, c.layout)) if c.out else "", c.C, c.shape, c.angle, c.mode)


# ---- what a configuration is ------------------------------------------------------------------------------------------------------------
def geometry(c):
    """(W, H, src resolution, dst resolution, isocentre, angle): the tuples of half_cases.CASES"""
    s = SHAPES[c.shape]
    W = s.row // c.C
    return (W, s.H, s.src_res, s.dst_res, ((W - 1) / 2.0 + s.iso_off[0], (s.H - 1) / 2.0 + s.iso_off[1]), c.angle)


def request(aai, c):
    W, H, sr, dr, iso, ang = geometry(c)
    mode = {"area": aai.MODE_AREA, "fast": aai.MODE_FAST, "bilinear": aai.MODE_BILINEAR}[c.mode]
    return aai.make_request(W, H, sr, dr, iso, ang, mode=mode)


def planar(c):
    return c.layout == "nchw"


def conversion(c):
    """(scale[4], offset[4]) of a convert configuration: the usual normalisation"""
    return cc.conversion("normalise", DT[c.T])


def route_facts(aai, c):
    """the facts of the probe that answers for c's entry, as convert_cases.facts lists them (the integer probe's eight, then the two flips)"""
    return cc.facts(request(aai, c), c.C)


def is_direct(aai, c):
    """the route, from the predicate of c's entry"""
    rq = request(aai, c)
    if c.entry == "half":
        return bool(hc.facts(rq)[7])
    if c.entry == "half-il":
        return bool(hic.facts(rq, c.C)[7])
    if c.entry == "int":
        return ic.direct(rq, c.C, DT[c.T])
    if c.entry == "convert":
        return cc.direct(rq, c.C, DT[c.T], OT[c.out], LAY[c.layout])
    assert c.entry == "adjoint", c.entry
    return ac.serves_direct(aai, rq, c.C)


def direct_name(c):
    """what aai_last_kernel() reports for the direct kernel of c's entry and types"""
    if c.entry in ("half", "half-il"):
        return "aai_axis_half_kernel<%s>" % c.T
    if c.entry == "int":
        return "aai_axis_int_kernel<%s>" % c.T
    if c.entry == "convert":
        return "aai_axis_convert_kernel<%s,%s>" % (c.T, c.out)
    return "aai_axis_adjoint_half_kernel<%s,%d>" % (c.T, c.C)


def name_matches(row_kernel, reported):
    """a row's recorded name against aai_last_kernel(): the direct kernel's name itself, or the forwarding route's suffix behind the name of
    an fp32 kernel"""
    if row_kernel.startswith("+"):
        return reported.endswith(row_kernel) and not reported.startswith(("aai_axis_half_kernel", "aai_axis_int_kernel", "aai_axis_convert_kernel",
                                                                            "aai_axis_adjoint_half_kernel"))
    return reported == row_kernel


# the image read and the image written, in elements: rows x row length; the image written of a planar configuration is `planes` planes
Images = collections.namedtuple("Images", "rT rH rrow wT wH wrow planes")


def images(aai, c):
    W, H = geometry(c)[:2]
    lay = aai.query(request(aai, c))[2]
    dW, dH = lay.dst_width, lay.dst_height
    if c.entry == "adjoint":
        return Images(c.T, dH, dW * c.C, c.T, H, W * c.C, 1)
    if planar(c):
        return Images(c.T, H, W * c.C, c.out, dH, dW, c.C)
    return Images(c.T, H, W * c.C, c.out or c.T, dH, dW * c.C, 1)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
# pitch: the row stride (elements) of the wide image, 0 for plane and batch rows (tight rows + GUARD); apart: the plane stride of a
# plane row, the image stride of a batch row (elements)
Row = collections.namedtuple("Row", "index config side cls direct kernel pitch apart")


def row_id(r):
    return "%s-%s-%s" % (config_id(r.config), r.side, r.cls)


def wide_image(im, side):
    """(element type, rows, row length) of the image on `side`; a planar image written counts as planes x rows rows"""
    return (im.rT, im.rH, im.rrow) if side.endswith("src") else (im.wT, im.wH * im.planes, im.wrow)


def rows_below(cls, rows, esz):
    """How many rows of an image of `rows` rows must START below the threshold of a pitch class, so that the rows behind them start
    beyond it: all but an eighth (a sixteenth for fp32 at 2^31 elements, 8.6 GB: the arena's cap), and, of images of 530 rows and more,
    520 -- 4 GiB over fewer rows is a pitch of 8 MiB and more."""
    b = rows - max(rows // (16 if (cls, esz) == ("E31", 4) else 8), 2)
    return max(b, 520) if rows > 522 else b


def pitch_of(cls, rows, row, esz):
    """wide_pitch.pitch_for, asked for the rows that must lie below the class's threshold (rows_below), not for the image's height: with
    the height itself the LAST row would start one pitch short of 2^32 bytes / 2^31 elements and no offset product would pass them.
    GP's pitch does not depend on the height: rows from 512 on start beyond 2^32 bytes."""
    return wp.pitch_for(cls, rows if cls == "GP" else rows_below(cls, rows, esz), row, esz)


def rows_beyond(r, p):
    """how many row starts of Placement p (of a src / dst row r) lie at or beyond the threshold of r's class: 2^32 bytes (G, GP),
    2^31 elements (E31)"""
    limit = (1 << 31) if r.cls == "E31" else -(-(1 << 32) // ESZ[p.T])
    return sum(1 for y in range(p.planes * p.rows) if y * p.pitch >= limit)


PLANE_APART = (1 << 31) + 4099      # the plane stride of a plane row: just past 2^31 elements, odd


# Where the images of a row lie in their arena, in elements of type T from the arena's first byte: image b, plane p, row y starts at
# b image + p plane + y pitch; every row is `row` elements with GUARD elements behind it.  `images`: 2 for a batch row.
Placement = collections.namedtuple("Placement", "T rows row pitch planes plane images image")


def placement(im, r):
    """the Placement of the image of row r that lies in an arena: the image read (src, batch-src) or the image written"""
    read = r.side.endswith("src")
    T, rows_, row = (im.rT, im.rH, im.rrow) if read else (im.wT, im.wH, im.wrow)
    planes = 1 if read else im.planes
    pitch = r.pitch if r.side in ("src", "dst") else row + wp.GUARD
    plane = r.apart if r.side == "plane" else rows_ * pitch
    images_ = 2 if r.side.startswith("batch") else (GRID_IMAGES if r.side.startswith("grid") else 1)
    return Placement(T, rows_, row, pitch, planes, plane, images_, r.apart if images_ > 1 else 0)


def tight_placement(im, read, images_=1):
    """the same image(s) on buffers of their own: rows of `row` + GUARD elements, planes and images back to back"""
    T, rows_, row = (im.rT, im.rH, im.rrow) if read else (im.wT, im.wH, im.wrow)
    planes = 1 if read else im.planes
    pitch = row + wp.GUARD
    return Placement(T, rows_, row, pitch, planes, rows_ * pitch, images_, planes * rows_ * pitch)


def extent_bytes(p):
    """bytes of arena a Placement takes, the guard behind its last row included"""
    return ((p.images - 1) * p.image + (p.planes - 1) * p.plane + (p.rows - 1) * p.pitch + p.row + wp.GUARD) * ESZ[p.T]


_ROWS = {}


def rows(aai):
    """the table, built once per process"""
    if "rows" in _ROWS:
        return _ROWS["rows"]
    out = []

    def add(c, side, cls, pitch=0, apart=0):
        direct = is_direct(aai, c)
        out.append(Row(len(out), c, side, cls, direct, direct_name(c) if direct else SUFFIX[c.entry], int(pitch), int(apart)))

    for c, pairs in CONFIGS:
        im = images(aai, c)
        for side, cls in pairs + ((("src", "E31"),) if c.T == "u8" else ()):
            if side == "plane":
                add(c, side, cls, apart=PLANE_APART)
            else:
                T, vH, vrow = wide_image(im, side)
                add(c, side, cls, pitch=pitch_of(cls, vH, vrow, ESZ[T]))
    for c, sides in BATCHES:
        im = images(aai, c)
        for side in sides:
            T = wide_image(im, side)[0]
            # (wide_pitch.batch_apart knows u8 sources: 2^32 elements there, 2^31 everywhere else)
            add(c, side, "E31", apart=wp.batch_apart("u8" if T == "u8" else "u16", "src" if side == "batch-src" else "dst"))
    for c, sides in GRIDS:
        for side in sides:
            add(c, side, "E31", apart=GRID_APART)
    _ROWS["rows"] = out
    return out


def arena_bytes(aai, which):
    """what the arena of the images read ("src") / written ("dst") must hold"""
    need = [0]
    for r in rows(aai):
        if (r.side.endswith("src")) == (which == "src"):
            need.append(extent_bytes(placement(images(aai, r.config), r)))
    return max(need)


# ---- data and replays -------------------------------------------------------------------------------------------------------------------
_DATA = {}


def gradient_bits(lay, channels, ht, seed):
    """[dH, dW, C] raw 16-bit elements: uniform in [0.25, 1.25) rounded to the type, a different stream per channel (a mix-up of channels
    cannot pass) -- the value range of the forward entries' sources.  Not adjoint_half_cases.gradient_bits: its signed gradients cancel,
    and on images of this size some of the sums land in fp16's subnormal range (below 2^-14), where one rounding is
    2^-25 absolute; half_cases.rounded_excess models a rounding as u |gold|, which holds for normal numbers only."""
    g = np.stack([np.random.default_rng(seed + 17 * c).random((lay.dst_height, lay.dst_width), dtype=np.float32) + np.float32(0.25) for c in range(channels)], axis=2)
    return hc.narrow(g, ht)


def read_image(aai, c, seed=0):
    """the image c's entry reads, [rows, row length] of raw elements (read-only, computed once)"""
    key = (c, seed)
    if key not in _DATA:
        g = geometry(c)
        W, H = g[:2]
        if c.entry == "half":
            a = hc.source_bits(W, H, HT[c.T], seed=5 + seed)
        elif c.entry == "half-il":
            a = hic.source_bits(g, c.C, HT[c.T], seed=5 + seed)
        elif c.entry in ("int", "convert"):
            a = ic.source(g, c.C, DT[c.T], "random", seed=7 + seed)
        else:
            a = gradient_bits(aai.query(request(aai, c))[2], c.C, HT[c.T], 3 + seed)
        a = np.ascontiguousarray(a).reshape(a.shape[0], -1)
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def read_images(aai, c, n):
    """n small images for a grid row, [n, rows, row length] of raw elements: the value ranges of read_image, one stream"""
    key = (c, "grid", n)
    if key not in _DATA:
        im = images(aai, c)
        rng = np.random.default_rng(11)
        if c.T in HT:
            a = hc.narrow(rng.random((n, im.rH, im.rrow), dtype=np.float32) + np.float32(0.25), HT[c.T])
        else:
            a = rng.integers(0, ic.MAXV[DT[c.T]] + 1, size=(n, im.rH, im.rrow)).astype(NP[c.T])
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def replay(aai, c, img):
    """the CPU replay of c's direct kernel on the dense image `img` ([rows, row length]): the image written, [planes x rows, row length]"""
    rq = request(aai, c)
    W, H = geometry(c)[:2]
    if c.entry == "half":
        out = hc.replay(aai, rq, HT[c.T], img.reshape(H, W))[0]
    elif c.entry == "half-il":
        out = hic.replay(aai, rq, HT[c.T], img.reshape(H, W, c.C))[0]
    elif c.entry == "int":
        out = ic.replay(aai, rq, DT[c.T], img.reshape(H, W, c.C))[0]
    elif c.entry == "convert":
        scale, offset = conversion(c)
        out = cc.replay(aai, rq, DT[c.T], img.reshape(H, W, c.C), scale, offset, OT[c.out], LAY[c.layout])[0]
    else:
        out = ac.replay(rq, HT[c.T], img.reshape(img.shape[0], -1, c.C))
    im = images(aai, c)
    return np.ascontiguousarray(out).reshape(im.planes * im.wH, im.wrow)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
