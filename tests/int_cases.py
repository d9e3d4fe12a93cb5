"""Shared by the tests of the integer path (include/aai_int.h): the direct-route cases (geometry x channel count), the sources, the CPU
replay of the kernel (tests/emulation/int_emulation.cpp), the conversion in numpy and the bound of one conversion on top of the project's bar."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import half_cases as hc
from conftest import BUILD, ROOT, TOL

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

U8, U16 = 1, 2                         # AAI_DTYPE_U8 / AAI_DTYPE_U16
TYPES = ((U8, "u8"), (U16, "u16"))
NP = {U8: np.uint8, U16: np.uint16}
MAXV = {U8: 255, U16: 65535}
MODES = hc.MODES
SOURCES = ("random", "constant", "checker")

# the nine direct-route geometries of the half-precision path (strip count, ragged widths, shared rows, 67 / 140 / 221 outputs per strip,
# x3 pre-expansion, 13-row windows, the narrowest image, 180 degrees) and three of this path's own
GEOMETRIES = dict(hc.CASES)
GEOMETRIES["m"] = (259, 37, 3.3, 1, (100.25, 17.5), 180.0)      # with 3 channels: a row of 777 elements, not a multiple of 4, backwards
GEOMETRIES["n"] = (2, 6, 1, 1, (0.5, 2.5), 0.0)                 # with 2 channels: a row of exactly 4 elements
GEOMETRIES["o"] = (4, 5, 1, 1, (1.5, 2.0), 180.0)               # one channel: a row of exactly 4 elements, backwards

# (geometry, channels): every half-path geometry with 1 and 3 channels, b / c / e with 2 and 4 as well
CASES = [(g, c) for g in sorted(hc.CASES) for c in (1, 3)] + [(g, c) for g in "bce" for c in (2, 4)] + [("m", 3), ("n", 2), ("o", 1)]
CASE_IDS = ["%s%d" % gc for gc in CASES]


def request(aai, geom, mode_name, angle=None):
    return hc.request(aai, GEOMETRIES[geom] if isinstance(geom, str) else geom, mode_name, angle=angle)


def source(geom, channels, dt, kind, seed=7):
    """[H, W, C] image of the element type: uniform random over the full range, the type's maximum everywhere, or a checkerboard of 0 and
    the maximum (per pixel, all channels alike)"""
    W, H = (GEOMETRIES[geom] if isinstance(geom, str) else geom)[:2]
    if kind == "random":
        return np.random.default_rng(seed).integers(0, MAXV[dt] + 1, size=(H, W, channels)).astype(NP[dt])
    if kind == "constant":
        return np.full((H, W, channels), MAXV[dt], NP[dt])
    assert kind == "checker", kind
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((x + y) & 1) * MAXV[dt]).astype(NP[dt])[:, :, None], channels, axis=2)


def quantize(values, dt):
    """the contract's conversion in numpy: round to nearest, ties to even, saturate; NaN -> 0"""
    v = np.asarray(values, np.float32)
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.clip(np.rint(v), 0, MAXV[dt]), nan=0.0).astype(NP[dt])


_emu = None


def emu():
    """tests/emulation/int_emulation.cpp (over narrow_replay.hpp) compiled with g++, no contraction"""
    global _emu
    if _emu is not None:
        return _emu
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_intemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", f) for f in ("int_emulation.cpp", "narrow_replay.hpp")] + [os.path.join(CSRC, f) for f in
            ("aai_int_math.hpp", "aai_half_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_int_facts.restype = ctypes.c_int
    lib.aai_emu_int_facts.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.aai_emu_int_replay.restype = ctypes.c_int
    lib.aai_emu_int_replay.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for fn in (lib.aai_emu_int_quantize_u8, lib.aai_emu_int_quantize_u16):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    _emu = lib
    return lib


def lib_quantize(values, dt):
    """fp32 array -> elements, the library's own int_quantize (csrc/aai_int_math.hpp)"""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty(v.shape, NP[dt])
    (emu().aai_emu_int_quantize_u8 if dt == U8 else emu().aai_emu_int_quantize_u16)(v.ctypes.data, out.ctypes.data, v.size)
    return out


def facts(rq, channels):
    """(axis-aligned area / fast, wide, transposed, strips, most outputs in a strip, rows shared, most source rows of a window, direct kernel serves)"""
    v = (ctypes.c_int * 8)()
    assert emu().aai_emu_int_facts(ctypes.byref(rq), channels, v) == 0
    return tuple(v)


def direct(rq, channels, dt):
    """whether the request takes the direct route: the strip form serves it (facts) and it is not of the class that
    profiles/int_time.txt sends to the forwarding route -- 8-bit elements with at most 64 outputs in every strip"""
    f = facts(rq, channels)
    return bool(f[7]) and (f[4] > 64 or dt == U16)


def replay(aai, rq, dt, src):
    """src [H, W, C] -> (the [dH, dW, C] output of the kernel's CPU replay, its fp32 values before the conversion)"""
    src = np.ascontiguousarray(src, dtype=NP[dt])
    H, W, C = src.shape
    assert (H, W) == (rq.src_height, rq.src_width)
    lay = aai.query(rq)[2]
    out = np.full((lay.dst_height, lay.dst_width, C), 0xA5, NP[dt])
    pre = np.full((lay.dst_height, lay.dst_width, C), np.nan, np.float32)
    assert emu().aai_emu_int_replay(ctypes.byref(rq), C, src.itemsize, src.ctypes.data, out.ctypes.data, pre.ctypes.data) == 0
    return out, pre


def oracle(po, geom, mode_name, src):
    """the oracle per channel on the integer values -> [dH, dW, C] float64"""
    W, H, sr, dr, iso, ang = GEOMETRIES[geom] if isinstance(geom, str) else geom
    return np.stack([po.oracle_run(hc.oracle_mode(po, mode_name), src[:, :, c].astype(np.float64), sr, dr, iso, ang).dst for c in range(src.shape[2])], axis=2)


@functools.lru_cache(maxsize=None)
def case(aai, po, geom, channels, mode_name, dt, kind):
    """-> (request, source, replay output, replay fp32 values before the conversion, the oracle per channel); computed once, read-only"""
    rq = request(aai, geom, mode_name)
    src = source(geom, channels, dt, kind)
    out, pre = replay(aai, rq, dt, src)
    gold = oracle(po, geom, mode_name, src)
    for a in (src, out, pre, gold):
        a.setflags(write=False)
    return rq, src, out, pre, gold


def excess(got, gold):
    """|q - gold| - (0.5 + TOL max(|gold|, 1e-3)), worst element: one conversion on top of the project's bar.  <= 0 passes.  (gold lies
    within the range of the type up to TOL -- area weights are non-negative and sum to 1 -- so the saturation adds nothing.)"""
    got, gold = np.asarray(got, np.float64), np.asarray(gold, np.float64)
    assert got.shape == gold.shape, (got.shape, gold.shape)
    return float((np.abs(got - gold) - (0.5 + TOL * np.maximum(np.abs(gold), 1e-3))).max())
