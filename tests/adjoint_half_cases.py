"""Shared by the tests of the half-precision adjoint (include/aai_adjoint_half.h): the geometries -- half_cases.CASES, each at its own
angle and at that angle + 90 and + 270 degrees, so that every case also runs in a transposed quadrant --, the gradients, the CPU replay
of the direct kernel (tests/emulation/adjoint_half_emulation.cpp over csrc/aai_axis_adjoint_half_math.hpp) and the planner's facts that
decide a geometry's route.  Needs neither torch nor a GPU.

What the shapes exercise (kernel: 256 elements of a source row per workgroup, 32 source rows per row block):
  b, c            more than 256 columns: two or more workgroups in x
  a, d, e, g, l   more than 32 source rows: two or more row blocks (the register-held horizontal sums start afresh per block)
  e, f, l         up-sampling and integer pre-expansion
  h               5 x 7: one partial workgroup, one partial row block"""
import ctypes
import os
import subprocess

import numpy as np

import half_cases as hc
from conftest import BUILD, ROOT
from half_cases import BF16, CASES, F16, MODES, TYPES, mode_of, narrow, widen      # noqa: F401  (re-exported)

CSRC = hc.CSRC
EXTRA_ANGLES = (0.0, 90.0, 270.0)
KEYS = [(case, extra) for case in CASES for extra in EXTRA_ANGLES]


def key_id(key):
    return "%s+%d" % (key[0], int(key[1]))


def request(aai, key, mode_name, policy=0):
    case, extra = key
    W, H, sr, dr, iso, ang = CASES[case]
    return aai.make_request(W, H, sr, dr, iso, (ang + extra) % 360.0, mode=mode_of(aai, mode_name), policy=policy)


_emu = None


def emu():
    """tests/emulation/adjoint_half_emulation.cpp compiled with g++, no contraction"""
    global _emu
    if _emu is not None:
        return _emu
    from area_average_interpolation_amd import _lib as L
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libaai_adjhalfemu.so")
    srcs = [os.path.join(ROOT, "tests", "emulation", "adjoint_half_emulation.cpp")] + [os.path.join(CSRC, f) for f in
            ("aai_axis_adjoint_half_math.hpp", "aai_half_math.hpp", "aai_axis_verify.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.aai_emu_adjoint_half_facts.restype = ctypes.c_int
    lib.aai_emu_adjoint_half_facts.argtypes = [ctypes.POINTER(L.Request), ctypes.POINTER(ctypes.c_int)]
    lib.aai_emu_adjoint_half.restype = ctypes.c_int
    lib.aai_emu_adjoint_half.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    _emu = lib
    return lib


_facts = {}


def facts(rq):
    """(0: the planner gives this request adjoint tables and no correction lists, so the direct route serves it; -1: it does not,
    (flagged dst pixels, listed source pixels, listed dst pixels)) -- the product's planner, model check and list builder on the CPU"""
    k = tuple(getattr(rq, f) for f, _ in rq._fields_)
    if k not in _facts:
        counts = (ctypes.c_int * 3)()
        rc = emu().aai_emu_adjoint_half_facts(ctypes.byref(rq), counts)
        _facts[k] = (rc, tuple(counts))
    return _facts[k]


def is_direct(rq):
    rc, _ = facts(rq)
    assert rc in (0, -1), rc
    return rc == 0


def serves_direct(aai, rq, channels):
    """is_direct, and the request is not of the one class the engine forwards by measurement (profiles/adjoint_half_time.txt): a single
    channel, up-sampled (more dst than source pixels), at 90 / 270 degrees.  Such a request has the direct kernel's bits all the same:
    both routes have the bits of narrow(fp32 entry(widen(g)))."""
    lay = aai.query(rq)[2]
    loses = channels == 1 and lay.quadrant in (1, 3) and lay.dst_width * lay.dst_height > rq.src_width * rq.src_height
    return is_direct(rq) and not loses


def replay(rq, ht, gbits):
    """raw 16-bit gdst [dH, dW, C] -> the raw 16-bit gsrc [H, W, C] of the kernel's CPU replay (prefilled 0xffff: every element is written)"""
    gbits = np.ascontiguousarray(gbits, dtype=np.uint16)
    assert gbits.ndim == 3
    out = np.full((rq.src_height, rq.src_width, gbits.shape[2]), 0xffff, np.uint16)
    rc = emu().aai_emu_adjoint_half(ctypes.byref(rq), ht, gbits.shape[2], gbits.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


def gradient_bits(lay, channels, ht, seed=3, nonfinite=False):
    """[dH, dW, C] raw 16-bit elements: uniform in [-0.5, 0.5) rounded to the type, a different stream per channel (a mix-up of channels
    cannot pass).  nonfinite: NaN, +Inf and -Inf planted in channel 0 (the last channel stays finite: channels never mix) and, for fp16,
    a block of +-60000 whose sums pass 65504 in every channel."""
    dH, dW = lay.dst_height, lay.dst_width
    g = np.stack([np.random.default_rng(seed + 17 * c).random((dH, dW), dtype=np.float32) - np.float32(0.5) for c in range(channels)], axis=2)
    bits = narrow(g, ht)
    if nonfinite:
        v = widen(bits, ht)
        ys, xs = max(dH // 2, 1), max(dW // 2, 1)
        if ht == F16:
            v[:ys, :xs, :] = np.where(np.arange(xs)[None, :, None] % 5 == 4, -60000.0, 60000.0)       # sums of neighbours pass 65504
        bits = narrow(v, ht)
        nan, pinf, ninf = (0x7e00, 0x7c00, 0xfc00) if ht == F16 else (0x7fc0, 0x7f80, 0xff80)
        flat = bits[:, :, 0].reshape(-1)
        n = flat.size
        for i, b in ((n // 7, nan), (n // 3, pinf), (n - 1 - n // 5, ninf)):
            flat[i] = b
        bits[:, :, 0] = flat.reshape(dH, dW)
    return bits
