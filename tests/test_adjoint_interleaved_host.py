"""The interleaved-channel adjoint (include/aai_adjoint_interleaved.h), checks that need no GPU: declarations and bindings, argument
errors before any device call, a serial CPU replay of the channel-generic per-pixel bodies (tests/emulation/adjoint_multi_emulation.cpp
over csrc/aai_adjoint_math.hpp) against the oracle's matrix and, bit for bit, against the single-channel replay, and the argument checks
of the torch operator's 4-D input."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import BUILD, GOLDEN, ROOT, TOL, rel_err

CSRC = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")
ENTRIES = ("aai_adjoint_interleaved_device_f32", "aai_adjoint_interleaved_f32")

# the eight hand-picked geometries of DESIGN.md section 9 ("how it is checked"), restated: (W, H, srcRes, dstRes, angle, isocenter
# offset from the image centre)
EIGHT = [(24, 20, 3, 1, 17.5, (0, 0)), (20, 24, 1, 1, 30, (0.3, -0.2)), (16, 12, 1, 2, 45, (0, 0)), (24, 24, 4, 1, 0, (0, 0)),
         (20, 16, 2.5, 1, 90, (0, 0)), (18, 22, 1.7, 1, 200.25, (-3, 4)), (12, 10, 1, 3, 117.5, (0, 0)), (24, 20, 2, 1, 180, (0.5, 0.5))]
# (mode, policy) by name: area under both policies, and fast
VARIANTS = (("area", 0), ("area", 1), ("fast", 0))
# (channels, index into EIGHT): three channels everywhere; two and four channels on two geometries each, chosen by what they are -- a
# replicated source (scale 2 and 5: the gather's virtual-pixel loop) for C = 2, a down-sampling at an angle and the grid-aligned 4:1 at
# 0 degrees, where nearly every boundary pair is a knife edge, for C = 4
REPLAY_CASES = [(3, i) for i in range(len(EIGHT))] + [(2, 1), (2, 6), (4, 0), (4, 3)]


def case_request(aai, case, variant):
    W, H, sr, dr, ang, off = EIGHT[case]
    mode, policy = variant
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    return aai.make_request(W, H, sr, dr, iso, ang, mode=aai.MODE_FAST if mode == "fast" else aai.MODE_AREA, policy=policy)


@functools.lru_cache(maxsize=None)
def _matrix(case, variant):
    """W of dst = W src for EIGHT[case], column by column from the oracle on unit impulses (float64); computed once per session"""
    from oracle import pyoracle as po
    W, H, sr, dr, ang, off = EIGHT[case]
    mode, policy = variant
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    cols = []
    for s in range(W * H):
        e = np.zeros(W * H)
        e[s] = 1.0
        cols.append(po.oracle_run(po.MODE_FAST if mode == "fast" else po.MODE_EXACT, e.reshape(H, W), sr, dr, iso, ang, policy=policy).dst.ravel())
    M = np.stack(cols, axis=1)
    M.setflags(write=False)
    return M


def interleaved_gold(po, aai, case, variant, channels, seed=7):
    """(rq, gdst fp32 [dH, dW, C] with an independent random image per channel, W^T gdst per channel in float64 [H, W, C])"""
    assert po.have_oracle()
    rq = case_request(aai, case, variant)
    rc, msg, lay = aai.query(rq)
    M = _matrix(case, variant)
    assert rc == 0 and M.shape == (lay.dst_width * lay.dst_height, rq.src_width * rq.src_height), msg
    g = np.stack([np.random.default_rng(seed + 13 * c).random(M.shape[0]).astype(np.float32) for c in range(channels)], axis=1)
    gold = np.stack([(M.T @ g[:, c].astype(np.float64)) for c in range(channels)], axis=1)
    return rq, g.reshape(lay.dst_height, lay.dst_width, channels), gold.reshape(rq.src_height, rq.src_width, channels)


def assert_oracle_bar(got, gold, what):
    """the bar of DESIGN.md section 9, per channel: every source pixel within TOL of gold relative to max(|gold|, 1e-3 max|gold|); exact
    zeros where the oracle's column is zero"""
    assert got.shape == gold.shape, (what, got.shape, gold.shape)
    for c in range(gold.shape[2]):
        floor = 1e-3 * float(np.abs(gold[:, :, c]).max())
        err = rel_err(got[:, :, c], gold[:, :, c], floor=floor if floor > 0 else 1e-300)
        print("%s channel %d: max rel err %.3e, %d unread source pixels" % (what, c, float(err.max()), int((gold[:, :, c] == 0).sum())))
        assert float(err.max()) <= TOL, (what, c, float(err.max()))
        assert np.all(got[:, :, c][gold[:, :, c] == 0] == 0.0), (what, c)


def test_header_declares_library_exports_and_lib_binds_the_entries(aai):
    from area_average_interpolation_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "aai_adjoint_interleaved.h")).read()
    lib = L.load()
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    rq, ly = ctypes.POINTER(L.Request), ctypes.POINTER(L.Layout)
    args = {ENTRIES[0]: [rq, i32, i32, p, i64, i64, p, i64, i64, p], ENTRIES[1]: [rq, i32, p, i64, p, i64, ly]}
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.INTERLEAVED_ADJOINT_SYMBOLS and name not in L.SYMBOLS
        assert L.INTERLEAVED_ADJOINT_SYMBOLS[name][0] is ctypes.c_int and list(L.INTERLEAVED_ADJOINT_SYMBOLS[name][1]) == args[name], name
        assert getattr(lib, name).argtypes is not None
    assert callable(aai.adjoint_interleaved_device) and callable(aai.adjoint_interleaved_host)
    assert lib.aai_version() == 2
    # include/aai.h is what it was: additions live in headers of their own
    main = open(os.path.join(ROOT, "include", "aai.h"), "rb").read()
    for name in ENTRIES:
        assert name.encode() not in main
    try:
        r = subprocess.run(["git", "-C", ROOT, "show", "HEAD:include/aai.h"], capture_output=True)
    except OSError:
        r = None
    if r is not None and r.returncode == 0:
        assert r.stdout == main


def _device_call(lib, rq, channels=3, batch=1, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
    return lib.aai_adjoint_interleaved_device_f32(None if rq is None else ctypes.byref(rq), batch, channels, gdst, dst_stride, 0, gsrc, src_stride, 0, None)


def _host_call(lib, rq, channels=3, gdst=8, dst_stride=1 << 20, gsrc=8, src_stride=1 << 20):
    return lib.aai_adjoint_interleaved_f32(None if rq is None else ctypes.byref(rq), channels, gdst, dst_stride, gsrc, src_stride, None)


def test_argument_errors_come_before_any_device_call(aai):
    """dummy (never dereferenced) pointers: every call below must return before the device is touched"""
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    probes = json.load(open(os.path.join(GOLDEN, "error_paths.json")))
    rejected = 0
    for p in probes:
        if p["kind"] == "args":
            rq = aai.make_request(4, 4, p["src_res"], p["dst_res"], (0, 0), 0, mode=p["mode"])
        else:
            rq = aai.make_request(0 if p["rows"] else 4, p["rows"], 1, 1, (0, 0), 0, mode=p["mode"])
        rc, msg, _ = aai.query(rq)
        if rc == L.OK:
            continue
        rejected += 1
        for call in (_device_call, _host_call):
            assert call(lib, rq) == rc and aai.last_error() == msg, (p, call.__name__)
    assert rejected >= 4
    W, H, C = 24, 20, 3
    ok = aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5)
    rc, _, lay = aai.query(ok)
    assert rc == L.OK
    # the forward's interleaved entry reports a bad channel count with this message
    assert lib.aai_resample_interleaved_device(ctypes.byref(ok), 1, 0, 8, L.DTYPE_F32, 1 << 20, 0, 8, 1 << 20, 0, None) == L.ERR_BAD_ARGUMENT
    channels_message = aai.last_error()
    for call in (_device_call, _host_call):
        for channels in (0, 5, -1):
            assert call(lib, ok, channels=channels) == L.ERR_BAD_ARGUMENT and aai.last_error() == channels_message, (call.__name__, channels)
        for mode, name in ((L.MODE_BILINEAR, "BILINEAR"), (L.MODE_BICUBIC, "BICUBIC")):
            assert call(lib, aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5, mode=mode)) == L.ERR_BAD_ARGUMENT
            assert name in aai.last_error()
        assert call(lib, aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5, policy=L.POLICY_DIAG_NO_FIXUP)) == L.ERR_BAD_ARGUMENT
        assert call(lib, aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5, policy=0x800)) == L.ERR_BAD_ARGUMENT      # no new policy bit
        assert call(lib, ok, src_stride=W * C - 1) == L.ERR_BAD_ARGUMENT and "Source stride" in aai.last_error()
        assert call(lib, ok, dst_stride=lay.dst_width * C - 1) == L.ERR_BAD_ARGUMENT and "Destination stride" in aai.last_error()
        # a stride that would do for one channel does not do for three
        assert call(lib, ok, src_stride=W) == L.ERR_BAD_ARGUMENT and "Source stride" in aai.last_error()
        assert call(lib, ok, gdst=None) == L.ERR_BAD_ARGUMENT and call(lib, ok, gsrc=None) == L.ERR_BAD_ARGUMENT
        assert call(lib, None) == L.ERR_BAD_ARGUMENT
    assert _device_call(lib, ok, batch=-1) == L.ERR_BAD_ARGUMENT and "batch" in aai.last_error()
    for channels in (1, 2, 3, 4):
        assert _device_call(lib, ok, channels=channels, batch=0) == L.OK
    # the two accepted hints pass validation: with batch 0 the call returns before the device
    assert _device_call(lib, aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5, policy=L.POLICY_DOUBLE_PRECISION | L.POLICY_PREFER_CELL | L.POLICY_EXACT), batch=0) == L.OK
    # a row of width x channels elements beyond what the forward's interleaved entry accepts: its code
    wide = aai.make_request(400_000_000, 2, 1, 1, (0, 0), 0)
    rc_fwd = lib.aai_resample_interleaved_device(ctypes.byref(wide), 0, 4, 8, L.DTYPE_F32, 1 << 40, 0, 8, 1 << 40, 0, None)
    assert rc_fwd != L.OK
    message = aai.last_error()
    assert _device_call(lib, wide, channels=4, batch=0, dst_stride=1 << 40, src_stride=1 << 40) == rc_fwd and aai.last_error() == message
    # api wrappers raise / report the same
    with pytest.raises(aai.AaiError):
        aai.adjoint_interleaved_device(aai.make_request(W, H, 3, 1, (11.5, 9.5), 17.5, mode=L.MODE_BICUBIC), 3, 8, 8 * C, 8, W * C)
    with pytest.raises(aai.AaiError) as info:
        aai.adjoint_interleaved_device(ok, 5, 8, 1 << 20, 8, 1 << 20)
    assert info.value.code == L.ERR_BAD_ARGUMENT and info.value.message == channels_message
    rc, msg, g = aai.adjoint_interleaved_host(np.zeros((4, 4, 3), np.float32), (4, 4), (1, 2), 1, (0, 0), 0)
    assert rc == L.ERR_RESOLUTION_MISMATCH and g is None and msg == "Assumed X & Y resolution are same."
    rc, msg, g = aai.adjoint_interleaved_host(np.zeros((lay.dst_height, lay.dst_width, 5), np.float32), (H, W), 3, 1, (11.5, 9.5), 17.5)
    assert rc == L.ERR_BAD_ARGUMENT and g is None and msg == channels_message
    with pytest.raises(ValueError):
        aai.adjoint_interleaved_host(np.zeros((lay.dst_height, lay.dst_width), np.float32), (H, W), 3, 1, (11.5, 9.5), 17.5)


def _build(source, so, deps):
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "emulation", source)] + [os.path.join(CSRC, f) for f in deps]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return ctypes.CDLL(so)


EMU_DEPS = ("aai_adjoint_math.hpp", "aai_plan.cpp", "aai_plan.hpp", "aai_rot_math.hpp", "aai_strict.hpp")


@pytest.fixture(scope="module")
def multiemu(aai):
    """tests/emulation/adjoint_multi_emulation.cpp compiled with g++, no contraction: run(rq, gdst [dH, dW, C]) -> gsrc [H, W, C]"""
    from area_average_interpolation_amd import _lib as L
    lib = _build("adjoint_multi_emulation.cpp", os.path.join(BUILD, "libaai_adjmultiemu.so"), EMU_DEPS)
    lib.aai_emu_adjoint_multi.restype = ctypes.c_int
    lib.aai_emu_adjoint_multi.argtypes = [ctypes.POINTER(L.Request), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    def run(rq, gdst):
        gdst = np.ascontiguousarray(gdst, dtype=np.float32)
        out = np.full((rq.src_height, rq.src_width, gdst.shape[2]), -1.0, np.float32)
        assert lib.aai_emu_adjoint_multi(ctypes.byref(rq), gdst.shape[2], gdst.ctypes.data, out.ctypes.data) == 0
        return out
    return run


@pytest.fixture(scope="module")
def singleemu(aai):
    """the existing single-channel replay (tests/emulation/adjoint_emulation.cpp), built and loaded as tests/test_adjoint_host.py does"""
    from area_average_interpolation_amd import _lib as L
    lib = _build("adjoint_emulation.cpp", os.path.join(BUILD, "libaai_adjemu.so"), EMU_DEPS)
    lib.aai_emu_adjoint.restype = ctypes.c_int
    lib.aai_emu_adjoint.argtypes = [ctypes.POINTER(L.Request), ctypes.c_void_p, ctypes.c_void_p]

    def run(rq, gdst):
        gdst = np.ascontiguousarray(gdst, dtype=np.float32)
        out = np.full((rq.src_height, rq.src_width), -1.0, np.float32)
        assert lib.aai_emu_adjoint(ctypes.byref(rq), gdst.ctypes.data, out.ctypes.data) == 0
        return out
    return run


@pytest.mark.parametrize("channels,case", REPLAY_CASES, ids=["C%d-case%d" % cc for cc in REPLAY_CASES])
def test_cpu_replay_matches_the_oracle_matrix(aai, po, multiemu, channels, case):
    for variant in VARIANTS:
        rq, g, gold = interleaved_gold(po, aai, case, variant, channels)
        assert_oracle_bar(multiemu(rq, g), gold, "multi replay C=%d case %d %s policy %d" % ((channels, case) + variant))


@pytest.mark.parametrize("channels,case", REPLAY_CASES, ids=["C%d-case%d" % cc for cc in REPLAY_CASES])
def test_cpu_replay_channels_have_the_single_channel_replays_bits(aai, multiemu, singleemu, channels, case):
    for variant in VARIANTS:
        rq = case_request(aai, case, variant)
        lay = aai.query(rq)[2]
        g = np.random.default_rng(100 + case).random((lay.dst_height, lay.dst_width, channels)).astype(np.float32)
        got = multiemu(rq, g)
        nonzero = 0
        for c in range(channels):
            one = singleemu(rq, g[:, :, c])
            assert np.array_equal(got[:, :, c].view(np.int32), one.view(np.int32)), (channels, case, variant, c)
            nonzero += int((one != 0).sum())
        assert nonzero > 0 and float(got.min()) >= 0.0          # not an empty comparison, and the -1 prefill is gone


def test_torch_operator_argument_checks():
    """the 4-D input's checks that need no device: ranks beyond (B, C, H, W) and CPU tensors are refused up front"""
    import torch
    from area_average_interpolation_amd import torch_ops
    with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
        torch_ops.resample(torch.zeros((1, 2, 3, 8, 8), dtype=torch.float32), 2, 1, (3.5, 3.5), 0.0)
    with pytest.raises(ValueError, match="GPU"):
        torch_ops.resample(torch.zeros((2, 3, 8, 8), dtype=torch.float32), 2, 1, (3.5, 3.5), 0.0)
    with pytest.raises(ValueError, match="GPU"):
        torch_ops.resample(torch.zeros((2, 3, 8, 8), dtype=torch.float32).contiguous(memory_format=torch.channels_last), 2, 1, (3.5, 3.5), 0.0)
