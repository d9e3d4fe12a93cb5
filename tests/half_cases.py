"""Shared by the tests of the half-precision path (include/aai_half.h): the direct-route geometries, the CPU replay of the kernel
(tests/emulation/half_emulation.cpp), bit-level conversions that need neither torch nor a GPU, and the rounded-value bound."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import BUILD, ROOT, TOL

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")

F16, BF16 = 1, 2                       # AAI_HALF_F16 / AAI_HALF_BF16
UNIT = {F16: 2.0 ** -11, BF16: 2.0 ** -8}      # unit roundoff of one round-to-nearest
TYPES = ((F16, "f16"), (BF16, "bf16"))
MODES = ("area", "fast")

# the direct-route geometries: name -> (W, H, src resolution, dst resolution, isocenter, angle)
CASES = {
    "a": (64, 48, 4, 1, (31.5, 23.5), 0.0),            # grid-aligned
    "b": (259, 37, 3.3, 1, (100.25, 17.5), 0.0),       # two strips, width not a multiple of 4, output rows share source rows
    "c": (1030, 21, 4, 1, (514.5, 10.5), 180.0),       # five strips = one full and one partial workgroup, flipped
    "d": (67, 45, 1, 1, (33, 22), 0.0),                # 67 outputs in a strip
    "e": (70, 50, 1, 2, (34.5, 24.5), 180.0),          # x2, 140 outputs per strip
    "f": (37, 29, 1, 3, (18, 14), 0.0),                # x3 integer pre-expansion
    "g": (300, 200, 12, 1, (149.5, 99.5), 0.0),        # 13 source rows per output row
    "h": (5, 7, 2, 1, (2, 3), 0.0),                    # narrowest image the strip form serves
    "l": (130, 90, 1, 1.7, (64.2, 44.9), 180.0),       # 221 outputs per strip
}


def mode_of(aai, name):
    return aai.MODE_FAST if name == "fast" else aai.MODE_AREA


def oracle_mode(po, name):
    return po.MODE_FAST if name == "fast" else po.MODE_EXACT


def request(aai, case, mode_name, angle=None, policy=0):
    W, H, sr, dr, iso, ang = CASES[case] if isinstance(case, str) else case
    return aai.make_request(W, H, sr, dr, iso, ang if angle is None else angle, mode=mode_of(aai, mode_name), policy=policy)


_emu = None


def emu():
    """tests/emulation/half_emulation.cpp (over narrow_replay.hpp) compiled with g++, no contraction"""
    global _emu
    if _emu is not None:
        return _emu
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_halfemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", f) for f in ("half_emulation.cpp", "narrow_replay.hpp")] + [os.path.join(CSRC, f) for f in
            ("aai_half_math.hpp", "aai_int_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_half_facts.restype = ctypes.c_int
    lib.aai_emu_half_facts.argtypes = [ctypes.POINTER(L.Request), ctypes.POINTER(ctypes.c_int)]
    lib.aai_emu_half_replay.restype = ctypes.c_int
    lib.aai_emu_half_replay.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for fn in (lib.aai_emu_f32_to_f16, lib.aai_emu_f32_to_bf16, lib.aai_emu_f16_to_f32, lib.aai_emu_bf16_to_f32):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    _emu = lib
    return lib


def narrow(values, ht):
    """fp32 array -> raw 16-bit elements (uint16), the library's own rounding helper"""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty(v.shape, np.uint16)
    (emu().aai_emu_f32_to_f16 if ht == F16 else emu().aai_emu_f32_to_bf16)(v.ctypes.data, out.ctypes.data, v.size)
    return out


def widen(bits, ht):
    """raw 16-bit elements -> fp32, exactly (numpy's own conversions, not the library's)"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    if ht == F16:
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def facts(rq):
    """(axis-aligned, wide, transposed, strips, most outputs in a strip, rows shared, most source rows of a window, direct kernel serves)"""
    v = (ctypes.c_int * 8)()
    assert emu().aai_emu_half_facts(ctypes.byref(rq), v) == 0
    return tuple(v)


def replay(aai, rq, ht, src_bits):
    """-> (raw 16-bit output of the kernel's CPU replay, its fp32 values before the rounding)"""
    src_bits = np.ascontiguousarray(src_bits, dtype=np.uint16)
    assert src_bits.shape == (rq.src_height, rq.src_width)
    lay = aai.query(rq)[2]
    out = np.full((lay.dst_height, lay.dst_width), 0xffff, np.uint16)
    pre = np.full((lay.dst_height, lay.dst_width), np.nan, np.float32)
    assert emu().aai_emu_half_replay(ctypes.byref(rq), ht, src_bits.ctypes.data, out.ctypes.data, pre.ctypes.data) == 0
    return out, pre


def source_bits(W, H, ht, seed=5):
    """uniform in [0.25, 1.25), rounded to the element type"""
    rng = np.random.default_rng(seed)
    return narrow((0.25 + rng.random((H, W))).astype(np.float32), ht)


def rounded_excess(got, gold, ht):
    """|got - gold| - (u |gold| (1 + TOL) + TOL max(|gold|, 1e-3)), worst element: one rounding to the element type on top of the
    project's bar.  <= 0 passes."""
    got, gold = np.asarray(got, np.float64), np.asarray(gold, np.float64)
    assert got.shape == gold.shape
    bound = UNIT[ht] * np.abs(gold) * (1 + TOL) + TOL * np.maximum(np.abs(gold), 1e-3)
    return float((np.abs(got - gold) - bound).max())


def ulp_distance(a_bits, b_bits):
    """distance in units of the last place between two arrays of raw 16-bit elements of one type (finite values)"""
    def key(b):
        b = np.asarray(b, np.uint16).astype(np.int32)
        return np.where(b & 0x8000, -(b & 0x7fff), b)
    return np.abs(key(a_bits) - key(b_bits))
