"""Shared by the tests of resample-and-convert (include/ext/aai_convert.h): the case table (geometry x channels x source type x output
type x layout, pruned), the three conversions, the CPU replay of the kernel (tests/emulation/convert_emulation.cpp), and the bound of
the converted value against the oracle."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import half_cases as hc
import int_cases as ic
from conftest import BUILD, ROOT, TOL

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

F32, F16, BF16 = 0, 1, 2               # AAI_DTYPE_F32 / AAI_HALF_F16 / AAI_HALF_BF16
OUT_TYPES = ((F32, "f32"), (F16, "f16"), (BF16, "bf16"))
OUT_NAME = dict(OUT_TYPES)
OUT_NP = {F32: np.float32, F16: np.uint16, BF16: np.uint16}        # fp16 / bf16 as raw 16-bit elements
UNIT = {F32: 2.0 ** -24, F16: hc.UNIT[hc.F16], BF16: hc.UNIT[hc.BF16]}      # unit roundoff of one round-to-nearest
INTERLEAVED, PLANAR = 0, 1
LAYOUT_NAME = {INTERLEAVED: "nhwc", PLANAR: "nchw"}
SRC_NAME = dict(ic.TYPES)
MODES = ic.MODES
SOURCES = ic.SOURCES

# (geometry of int_cases.GEOMETRIES, channels): a one strip of at most 64 outputs; b ragged width, two strips, shared rows; c a full and a
# partial workgroup at 180 degrees; d 67 outputs per strip; e 140 per strip at 180 degrees; g 13-row windows; l 221 per strip, non-integer
# ratio, 180 degrees; m 777 elements backwards; n / o rows of exactly 4 elements; h the narrowest image
PAIRS = [("a", 1), ("a", 3), ("b", 2), ("b", 3), ("c", 1), ("c", 4), ("d", 1), ("d", 3), ("e", 2), ("e", 3), ("g", 3), ("l", 1), ("l", 3), ("m", 3),
         ("n", 2), ("o", 1), ("h", 1), ("h", 3)]
# ... x (source type, output type, layout), pruned: pair i takes every third of the twelve combinations from the i-th on -- four each, both
# layouts and both source types among them; tests/test_convert_host.py asserts what the whole table reaches
_COMBOS = [(st, ot, lay) for st in (ic.U8, ic.U16) for ot in (F32, F16, BF16) for lay in (INTERLEAVED, PLANAR)]
CASES = [(g, c) + _COMBOS[(i + 3 * k) % 12] for i, (g, c) in enumerate(PAIRS) for k in range(4)]
CASE_IDS = ["%s%d-%s-%s-%s" % (g, c, SRC_NAME[st], OUT_NAME[ot], LAYOUT_NAME[lay]) for g, c, st, ot, lay in CASES]

# fast-mode geometries whose canvas overhangs the image: a dst column (the lane axis) or a dst row without weight; three channels
OFF_IMAGE = {"a column at 0 degrees": (37, 12, 1.7, 1, (38.7, 6.3), 0.0), "a row at 180 degrees": (17, 26, 3, 1, (6.4, 14.6), 180.0),
             "a column at 180 degrees": (36, 13, 3.3, 2, (-2.7, 9.25), 180.0)}

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
CONVERSIONS = ("identity", "normalise", "edge")


def conversion(name, st):
    """-> (scale[4], offset[4]) as float32: identity; the usual normalisation of an image of the source type's range; a set with
    cancellation (channel 0), fp16 overflow for u8 at scale 300 (channel 1), a shift (channel 2) and a negative scale (channels 0, 3)"""
    maxv = float(ic.MAXV[st])
    if name == "identity":
        return np.ones(4, np.float32), np.zeros(4, np.float32)
    if name == "normalise":
        return (np.float32([1.0 / (maxv * s) for s in STD]), np.float32([-m / s for m, s in zip(MEAN, STD)]))
    assert name == "edge", name
    return np.float32([-1.0 / maxv, 300.0, 1.0, -2.0]), np.float32([0.5, 0.0, -7.25, 1e-3])


_emu = None


def emu():
    """tests/emulation/convert_emulation.cpp (over narrow_replay.hpp) compiled with g++, no contraction"""
    global _emu
    if _emu is not None:
        return _emu
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_convertemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", f) for f in ("convert_emulation.cpp", "narrow_replay.hpp")] + [os.path.join(CSRC, f) for f in
            ("aai_int_math.hpp", "aai_half_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_convert_facts.restype = ctypes.c_int
    lib.aai_emu_convert_facts.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.aai_emu_convert_replay.restype = ctypes.c_int
    lib.aai_emu_convert_replay.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.aai_emu_convert_apply.restype = ctypes.c_int
    lib.aai_emu_convert_apply.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p]
    _emu = lib
    return lib


def facts(rq, channels):
    """(axis-aligned area / fast, wide, transposed, strips, most outputs in a strip, rows shared, most source rows of a window, direct kernel
    serves, the lane axis runs backwards, the row axis runs backwards)"""
    v = (ctypes.c_int * 10)()
    assert emu().aai_emu_convert_facts(ctypes.byref(rq), channels, v) == 0
    return tuple(v)


# the classes that profiles/convert_time.txt sends to the forwarding route although the strip form applies (csrc/aai_axis_convert.hip:
# kConvertForwards): (source, output, layout) -> the (at most 64 outputs per strip, 180 degrees) pairs that forward
FORWARDS = {
    (ic.U8, F32, INTERLEAVED): {(False, False), (False, True), (True, True)}, (ic.U8, F32, PLANAR): {(True, False), (True, True)},
    (ic.U8, F16, INTERLEAVED): {(False, True), (True, False), (True, True)}, (ic.U8, F16, PLANAR): {(True, False), (True, True)},
    (ic.U8, BF16, INTERLEAVED): {(True, False), (True, True)}, (ic.U8, BF16, PLANAR): {(True, True)},
    (ic.U16, F32, INTERLEAVED): {(False, True)}, (ic.U16, F16, INTERLEAVED): {(False, False)}, (ic.U16, BF16, INTERLEAVED): {(False, False)},
}


def direct(rq, channels, st, ot, lay):
    """whether the request takes the direct route: the strip form serves it (facts) and its class is not one of those that
    profiles/convert_time.txt sends to the forwarding route (a planar image of one channel counts as interleaved: it runs as one)"""
    f = facts(rq, channels)
    return bool(f[7]) and (f[4] <= 64, bool(f[8])) not in FORWARDS.get((st, ot, lay if channels > 1 else INTERLEAVED), ())


def out_shape(dH, dW, C, lay):
    return (C, dH, dW) if lay == PLANAR else (dH, dW, C)


def replay(aai, rq, st, src, scale, offset, ot, lay):
    """src [H, W, C] -> (the converted image of the kernel's CPU replay: [dH, dW, C] or [C, dH, dW] of OUT_NP[ot]; its fp32 sums s [dH, dW, C])"""
    src = np.ascontiguousarray(src, dtype=ic.NP[st])
    H, W, C = src.shape
    assert (H, W) == (rq.src_height, rq.src_width)
    l = aai.query(rq)[2]
    out = np.full(out_shape(l.dst_height, l.dst_width, C, lay), 0xA5, OUT_NP[ot])
    pre = np.full((l.dst_height, l.dst_width, C), np.nan, np.float32)
    scale, offset = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(offset, np.float32)
    assert emu().aai_emu_convert_replay(ctypes.byref(rq), C, src.itemsize, src.ctypes.data, scale.ctypes.data, offset.ctypes.data, ot, lay, out.ctypes.data,
                                        pre.ctypes.data) == 0
    return out, pre


def apply(img, scale, offset, ot, lay):
    """fp32 [dH, dW, C] -> round(fmaf(img, scale[c], offset[c])) in the output type and layout: the forwarding route's conversion on the CPU"""
    img = np.ascontiguousarray(img, dtype=np.float32)
    dH, dW, C = img.shape
    out = np.empty(out_shape(dH, dW, C, lay), OUT_NP[ot])
    scale, offset = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(offset, np.float32)
    assert emu().aai_emu_convert_apply(img.ctypes.data, dW, dH, C, scale.ctypes.data, offset.ctypes.data, ot, lay, out.ctypes.data) == 0
    return out


def as_float(out, ot):
    """the converted image as float64 values (fp16 / bf16 widened exactly)"""
    if ot == F32:
        return np.asarray(out, np.float32).astype(np.float64)
    return hc.widen(out, hc.F16 if ot == F16 else hc.BF16).astype(np.float64)


def to_hwc(out, lay):
    """[C, dH, dW] or [dH, dW, C] -> [dH, dW, C]"""
    return np.transpose(out, (1, 2, 0)) if lay == PLANAR else out


def narrow(values, ot):
    """fp32 array -> elements of the output type (the library's own narrowings for fp16 / bf16; fp32 unchanged)"""
    v = np.ascontiguousarray(values, np.float32)
    return v if ot == F32 else hc.narrow(v, hc.F16 if ot == F16 else hc.BF16)


@functools.lru_cache(maxsize=None)
def case(aai, po, geom, channels, mode_name, st, kind):
    """int_cases.case: (request, source, -, the replay's fp32 sums, the oracle per channel), computed once and shared with the integer tests"""
    return ic.case(aai, po, geom, channels, mode_name, st, kind)


F16_MAX_ROUNDS_TO_INF = 65520.0


def excess(got, gold_s, scale, offset, ot):
    """got [dH, dW, C] float64 (widened), gold_s the oracle's sums [dH, dW, C]: the worst of |got - e| - bound over the elements, e = gold_s
    scale[c] + offset[c] in float64 and
        bound = |scale[c]| TOL max(|gold_s|, 1e-3)      |scale| times the bar test_int_host.py / test_half_host.py hold the sums to
              + u |e| (1 + TOL)                          one rounding of the output type (u: its unit roundoff; fp32: 2^-24)
    <= 0 passes.  An fp16 element that is +-Inf passes where e, moved by the first term, reaches what rounds to Inf (65520)."""
    C = gold_s.shape[2]
    sc, of = np.asarray(scale, np.float64)[:C], np.asarray(offset, np.float64)[:C]
    e = gold_s * sc + of
    first = np.abs(sc) * TOL * np.maximum(np.abs(gold_s), 1e-3)
    bound = first + UNIT[ot] * np.abs(e) * (1 + TOL)
    inf = np.isinf(got)
    with np.errstate(invalid="ignore"):
        over = np.where(inf, np.where((np.sign(got) == np.sign(e)) & (np.abs(e) + first >= F16_MAX_ROUNDS_TO_INF), -1.0, np.inf), np.abs(got - e) - bound)
    assert not np.isnan(over).any()
    return float(over.max())


def sanitize_args(aai):
    """one argument of tests/cpp/convert_sanitize.cpp per case and mode"""
    args = []
    for g, c, st, ot, lay in CASES:
        W, H, sr, dr, iso, ang = ic.GEOMETRIES[g]
        for mode_name in MODES:
            args.append("%d,%d,%r,%r,%r,%r,%r,%d,%d,%d,%d,%d" % (W, H, float(sr), float(dr), float(iso[0]), float(iso[1]), float(ang), hc.mode_of(aai, mode_name), c,
                                                             ic.NP[st]().itemsize, ot, lay))
    return args
