"""GPU (MI355X): the kernels touch only the memory a call entitles them to (include/aai.h).

Every buffer of every case lies INSIDE one larger allocation (tests/guard_layout.py): row padding, gaps between batch images, rows
outside a band's footprint and wide margins on both sides hold poison in a source (a quiet NaN; all-zero and all-ones for 8- / 16-bit
pixels) and a sentinel bit pattern in a destination.  A read of poison shows as a non-finite output pixel or as output bits that depend
on the poison; a write outside the output shows as a changed guard element.  Nothing here can fault: an overrun lands in guard.

What every case asserts: every output pixel finite, within conftest.TOL of the oracle on the entitled view (the samplers: the 2e-5
absolute bound of test_comparison_samplers_against_cpu_restatement), exact zeros exact; bits identical to the same call on a tight,
aligned, contiguous copy whenever aai.last_kernel() names the same kernel for both; for 8- / 16-bit pixels bits identical under both
poisons; no guard element of the destination changed; no sentinel left in the output.  tests/test_guard_layout.py shows, without a
GPU, that each of these assertions can fail.

Coverage is asserted by kernel name at the end of the module (test_every_kernel_family_ran).  A case that fails puts its kernel on a
list, and later cases that expect that kernel fail at once without launching it: nothing is retried.

aai_axis_kernel has five branches and aai_last_kernel() does not tell them apart; the geometries below reach them by the launch
rules of aai_axis.hip (a strip = 256 source elements; nOut = outputs per strip; rows = output rows per workgroup):
  one output per lane            0 / 180 degrees, ratio >= 4                                (517 x 40 at 4:1, 1030 x 9 at 8:1)
  four outputs per lane          0 degrees, ratios 1..4 (also x2 of a narrow image)         (303 x 33 at 3:1, 301 x 21 at 2:1, 259 x 17 at 1:1)
  walking lanes                  up-sampling with nOut > 256; 180 degrees at ratios 1..4    (150 x 20 at 1:2; the cases above at 180)
  transposed, 8-column stores    90 / 270 degrees, nOut <= 64.  rows = 8 needs windows of at most two source rows, i.e. a NARROW
                                 image at ratio 1: 50 / 51 / 53 x nB with nB = 16 (8 + 8), 12 (8 + 4), 10 (8 + 2), 11 (8 + scalar);
                                 at 4:1 rows = 4 (the 4-store tail alone), at 8:1 rows = 2 (the 2-store tail alone)
  transposed, 4-column stores    not reached here: it needs 65..256 outputs per strip (a ratio below 4) in a launch the LDS-tile kernel
                                 does not take.  launch_axis_typed gives the tile kernel every such launch whose windows are at most 8
                                 source rows tall -- with equal x and y resolutions (aai_query refuses others) a ratio below 4 never has
                                 taller ones -- UNLESS the tile kernel's grid cannot carry it: more than 1,048,560 output columns at
                                 90 / 270 degrees (65,535 groups of 16).  A 100 x 1,048,600 source at 1:1 and 270 degrees lands in this
                                 branch; tests/test_axis_variants_gpu.py runs it.  The geometries below land in aai_axis_tile_kernel.
"""
import ctypes
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, RUNS_CASES, TOL, rel_err
from guard_layout import DTYPES, GuardedLayout, poisons, to_device

pytestmark = pytest.mark.gpu

SEEN = set()        # every aai.last_kernel() a guarded call reported
FAILED = set()      # kernels (name before "<") of failed cases: not launched again
FLOOR = {"f32": 1e-3, "u8": 1e-3 * 256, "u16": 1e-3 * 65536}
CODE = {"f32": 0, "u8": 1, "u16": 2}
T0 = time.time()

REQUIRED = [
    "aai_axis_kernel", "aai_axis_tile_kernel", "aai_axis_wide_kernel", "aai_axis_kernel+fixup", "aai_rotated_kernel<area, strict>",
    "aai_quad_kernel<area>", "aai_quad_fast_kernel", "aai_quad_multi_kernel<area, channels>",
    "aai_cell_kernel<area>", "aai_cell_multi_kernel<area, channels>", "aai_cell_kernel<area> unprompted",
    "aai_wide_kernel<area>", "aai_wide_fast_kernel",
    "aai_rotated_runs_kernel<area>", "aai_rotated_runs_kernel<area, channels>",
    "aai_rotated_kernel<area>", "aai_rotated_kernel<fast>", "aai_rotated_kernel<area, channels>", "aai_rotated_kernel<fast, channels>",
    "aai_quad_kernel<area> beside fix-up",
    "aai_sample_kernel<bilinear>", "aai_sample_kernel<bicubic>", "aai_sample_kernel<bilinear> band", "aai_sample_kernel<bicubic> band",
    "aai_adjoint_gather_kernel<area>", "aai_adjoint_gather_kernel<fast>",
]

# (source padding p of stride W*C + p, source base offset, source image gap, dst padding, dst base offset, dst image gap): paddings
# from {1, 3, 5}, base offsets 1..3 elements, gaps that are not multiples of 4
LAYOUTS = [(1, 1, 5, 3, 2, 7), (3, 3, 6, 5, 1, 3), (5, 2, 7, 1, 3, 6)]


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


def _pad(row, p):
    """a padding from {1, 3, 5}, `p` first, that makes the stride odd -- or, for odd rows, at least no multiple of 4"""
    cands = [p] + [q for q in (1, 3, 5) if q != p]
    for q in cands:
        if (row + q) % 2:
            return q
    return [q for q in cands if (row + q) % 4][0]


def _offset(dtype, off):
    return off if dtype != "u16" or off % 2 else off + 1 if off < 3 else 1       # 16-bit pixels: 1 and 3 elements


def _values(rng, dtype, shape):
    if dtype == "f32":
        return rng.random(shape).astype(np.float32)
    return rng.integers(0, np.iinfo(DTYPES[dtype]).max + 1, size=shape).astype(DTYPES[dtype])


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _launch(gpu, entry, rq, B, C, dtype, sptr, sstride, simg, dptr, dstride, dimg):
    """the C entry that carries the case: the typed batch entry, or the interleaved one"""
    from area_average_interpolation_amd import _lib as L
    import torch
    lib = L.load()
    if entry == "typed":
        assert C == 1
        rc = lib.aai_resample_batch_device(ctypes.byref(rq), B, sptr, CODE[dtype], sstride, simg, dptr, dstride, dimg, _stream())
    else:
        rc = lib.aai_resample_interleaved_device(ctypes.byref(rq), B, C, sptr, CODE[dtype], sstride, simg, dptr, dstride, dimg, _stream())
    assert rc == 0, gpu.last_error()
    torch.cuda.synchronize()
    return gpu.last_kernel()


def _gate(expect):
    if expect and expect.split("<")[0] in FAILED:
        pytest.fail("not launched: an earlier case of %s failed" % expect.split("<")[0])


def _judge(out, gold, tight, same_kernel, dtype, sampler, msg):
    """the value assertions of one guarded run"""
    bad = ~np.isfinite(out)
    assert not bad.any(), ("%d non-finite output pixels (a poisoned source element was read), first at [image, y, x, channel] %s"
                           % (int(bad.sum()), np.argwhere(bad)[0].tolist()), msg)
    if sampler:
        err = np.abs(out.astype(np.float64) - gold)
        assert err.max() <= 2e-5, (float(err.max()), msg)
    else:
        err = rel_err(out, gold, floor=FLOOR[dtype])
        assert err.max() <= TOL, (float(err.max()), np.argwhere(err > TOL)[0].tolist(), msg)
        assert np.array_equal(gold == 0, out == 0), ("exact zeros", msg)
    if same_kernel:
        diff = out.view(np.int32) != tight.view(np.int32)
        assert not diff.any(), ("%d pixels differ in bits from the tight call, first at %s" % (int(diff.sum()), np.argwhere(diff)[0].tolist()), msg)


def _check_guards(dl, ddev, msg):
    out, first, count = dl.check_dst(ddev)
    assert count == 0, ("%d guard elements of the destination were written, first: %s" % (count, dl.describe(first)), msg)
    left = dl.sentinels_left(out)
    assert left == 0, ("%d output pixels were never written" % left, msg)
    return out


def guarded_forward(gpu, po, W, H, sr, dr, ang, mode=1, policy=0, dtype="f32", C=1, B=3, entry=None, layouts=(0, 1), iso=None,
                    expect=None, tag=None, values=None):
    """One geometry through a batch entry: a tight call, then every guarded layout under every poison.  Returns the kernel name."""
    import torch
    entry = entry or ("interleaved" if C > 1 else "typed")
    _gate(expect)
    iso = ((W - 1) / 2, (H - 1) / 2) if iso is None else iso
    rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    dW, dH = lay.dst_width, lay.dst_height
    rng = np.random.default_rng(1000 * W + H + int(ang))
    if values is None:
        values = _values(rng, dtype, (B, H, W, C))
    sampler = mode in (3, 4)
    omode = {1: po.MODE_EXACT, 2: po.MODE_FAST, 3: 3, 4: 4}[mode]
    gold = np.empty((B, dH, dW, C), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            g = po.oracle_run(omode, values[b, :, :, c].astype(np.float64), sr, dr, iso, ang, policy=policy & 1)
            assert g.dst.shape == (dH, dW)
            gold[b, :, :, c] = g.dst
    tsrc = to_device(values)
    tdst = torch.full((B, dH, dW, C), float("nan"), dtype=torch.float32, device="cuda")
    k_tight = _launch(gpu, entry, rq, B, C, dtype, tsrc.data_ptr(), W * C, H * W * C, tdst.data_ptr(), dW * C, dH * dW * C)
    # (a geometry that takes another kernel than this file expects is a mistake of the file, not a finding about that kernel)
    assert not expect or expect in k_tight, ("expected %s, ran %s" % (expect, k_tight), (W, H, sr, dr, ang, mode, policy, dtype, C))
    _gate(k_tight)
    kernel = k_tight
    try:
        SEEN.add(k_tight)
        tight = tdst.cpu().numpy()
        info = gpu.plan_shape(rq, C)
        _judge(tight, gold, tight, False, dtype, sampler, ("tight call", k_tight, info, (W, H, sr, dr, ang, mode, policy, dtype, C)))
        for li in layouts:
            sp, so, sg, dp, do, dg = LAYOUTS[li] if isinstance(li, int) else li
            sstride = W * C + _pad(W * C, sp)
            dstride = dW * C + _pad(dW * C, dp)
            sl = GuardedLayout((B, H, W, C), dtype, sstride, H * sstride + sg, _offset(dtype, so))
            dl = GuardedLayout((B, dH, dW, C), "f32", dstride, dH * dstride + dg, do)
            outs = []
            for poison in poisons(dtype):
                sdev, ddev = to_device(sl.make_src(values, poison)), to_device(dl.make_dst())
                k = _launch(gpu, entry, rq, B, C, dtype, sl.ptr(sdev), sl.stride, sl.image_stride, dl.ptr(ddev), dl.stride, dl.image_stride)
                kernel = k
                SEEN.add(k)
                what = ("kernels: guarded %s, tight %s" % (k, k_tight), info, (W, H, sr, dr, ang, mode, policy, dtype, C, B),
                        "src stride %d image stride %d base %+d, dst stride %d image stride %d base %+d, poison %s"
                        % (sl.stride, sl.image_stride, sl.base_offset, dl.stride, dl.image_stride, dl.base_offset, poison))
                out = _check_guards(dl, ddev, what)
                _judge(out, gold, tight, k == k_tight, dtype, sampler, what)
                outs.append(out)
                del sdev, ddev
            if len(outs) == 2:
                diff = outs[0].view(np.int32) != outs[1].view(np.int32)
                assert not diff.any(), ("%d output pixels depend on the poison around the image, first at %s" % (int(diff.sum()), np.argwhere(diff)[0].tolist()), what)
    except AssertionError:
        FAILED.add(kernel.split("<")[0])
        raise
    if tag:
        SEEN.add(tag)
    return k_tight


def guarded_bands(gpu, po, W, H, sr, dr, ang, mode=1, policy=0, layouts=(0, 2), expect=None, tag=None):
    """aai_resample_band_device_f32: three bands per image (starts at multiples of 16), each from a buffer that holds ONLY its source
    footprint [src_row0, src_row1) between guards: the rows before and after it are poison."""
    import torch
    from area_average_interpolation_amd.distributed import shard_rows
    _gate(expect)
    iso = ((W - 1) / 2, (H - 1) / 2)
    rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    dW, dH = lay.dst_width, lay.dst_height
    rng = np.random.default_rng(77 + W + H)
    image = rng.random((H, W)).astype(np.float32)
    sampler = mode in (3, 4)
    omode = {1: po.MODE_EXACT, 2: po.MODE_FAST, 3: 3, 4: 4}[mode]
    gold = po.oracle_run(omode, image.astype(np.float64), sr, dr, iso, ang, policy=policy & 1).dst
    assert gold.shape == (dH, dW)
    kernel = expect or "?"
    bands = 0
    try:
        for rank in range(3):
            r0, r1 = shard_rows(dH, rank, 3)
            if r0 >= r1:
                continue
            bands += 1
            assert r0 % 16 == 0
            a, b = gpu.band_source_rows(rq, r0, r1)
            assert 0 <= a < b <= H
            values = image[a:b]
            tsrc = to_device(values)
            tdst = torch.full((r1 - r0, dW), float("nan"), dtype=torch.float32, device="cuda")
            gpu.resample_band_device(rq, r0, r1, tsrc.data_ptr(), W, tdst.data_ptr(), dW, _stream())
            torch.cuda.synchronize()
            k_tight = kernel = gpu.last_kernel()
            SEEN.add(k_tight)
            if expect and expect not in k_tight:
                pytest.fail("expected %s, ran %s: %r" % (expect, k_tight, (W, H, sr, dr, ang, mode, policy)))      # (the file's mistake, no finding)
            tight = tdst.cpu().numpy().reshape(1, r1 - r0, dW, 1)
            g = gold[r0:r1].reshape(1, r1 - r0, dW, 1)
            _judge(tight, g, tight, False, "f32", sampler, ("tight band", k_tight, (W, H, sr, dr, ang, mode, policy), (r0, r1, a, b)))
            for li in layouts:
                sp, so, sg, dp, do, dg = LAYOUTS[li]
                sl = GuardedLayout((1, b - a, W, 1), "f32", W + _pad(W, sp), None, so)
                dl = GuardedLayout((1, r1 - r0, dW, 1), "f32", dW + _pad(dW, dp), None, do)
                sdev, ddev = to_device(sl.make_src(values, "nan")), to_device(dl.make_dst())
                gpu.resample_band_device(rq, r0, r1, sl.ptr(sdev), sl.stride, dl.ptr(ddev), dl.stride, _stream())
                torch.cuda.synchronize()
                k = kernel = gpu.last_kernel()
                SEEN.add(k)
                what = ("kernels: guarded %s, tight %s" % (k, k_tight), (W, H, sr, dr, ang, mode, policy),
                        "dst rows [%d, %d) from source rows [%d, %d); src stride %d base %+d, dst stride %d base %+d"
                        % (r0, r1, a, b, sl.stride, sl.base_offset, dl.stride, dl.base_offset))
                out = _check_guards(dl, ddev, what)
                _judge(out, g, tight, k == k_tight, "f32", sampler, what)
        assert bands == 3, (bands, dH)
    except AssertionError:
        FAILED.add(kernel.split("<")[0])
        raise
    if tag:
        SEEN.add(tag)
    return kernel


# ---- K1: the axis-aligned kernels ----------------------------------------------------------------------------------------------------
AXIS_CASES = [  # W, H, srcRes, dstRes: see the module text for the branch each one takes in which quadrant
    (517, 40, 4, 1), (1030, 9, 8, 1), (303, 33, 3, 1), (301, 21, 2, 1), (259, 17, 1, 1), (150, 20, 1, 2), (70, 50, 1, 2), (40, 30, 1, 4),
    (263, 31, 8192, 2731), (1500, 20, 10, 9), (5, 700, 3, 1), (4, 4, 2, 1),
    (50, 16, 1, 1), (53, 12, 1, 1), (51, 10, 1, 1), (50, 11, 1, 1), (126, 23, 2, 1),
]


@pytest.mark.parametrize("ang", [0.0, 90.0, 180.0, 270.0])
def test_axis_kernels_stay_inside_their_buffers(gpu, po, ang):
    """Every reachable branch of aai_axis_kernel and both NT variants of aai_axis_tile_kernel (integer ratios with the isocenter at the
    centre: disjoint windows, nontemporal loads; 8192:2731 and 10:9: shared rows, cached loads), widths with W % 4 in 1..3 (the last
    lane of a row loads colc = W - 4 instead of its own column), in every quadrant: outBase and negative outStride* at 90 / 180 / 270.
    The tile kernel's last cooperative workgroup has trailing waves without output rows wherever ceil(nB / 16) % 4 != 0: all of its
    cases here (nB = the dst width at 90 / 270 degrees, 10 to 20)."""
    seen = set()
    for i, (W, H, sr, dr) in enumerate(AXIS_CASES):
        dtype = ("f32", "u8", "u16")[i % 3] if i % 4 == 3 else "f32"
        k = guarded_forward(gpu, po, W, H, float(sr), float(dr), ang, mode=1 + i % 2, dtype=dtype, layouts=(i % 3, (i + 1) % 3), expect="aai_axis")
        seen.add(k)
    # plain fp32 in both modes already ran; typed pixels and interleaved channels through the same branches
    for (W, H, sr, dr, dtype, C) in ((517, 40, 4, 1, "u8", 1), (303, 33, 3, 1, "u16", 1), (259, 17, 1, 1, "u8", 1), (150, 20, 1, 2, "u16", 1),
                                     (173, 24, 4, 1, "f32", 3), (101, 19, 2, 1, "u8", 2), (67, 13, 1, 1, "u16", 4), (50, 12, 1, 2, "f32", 3)):
        seen.add(guarded_forward(gpu, po, W, H, float(sr), float(dr), ang, dtype=dtype, C=C, layouts=(2, 0), expect="aai_axis"))
    assert "aai_axis_kernel" in seen, seen
    if ang in (90.0, 270.0):
        assert "aai_axis_tile_kernel" in seen, seen


def test_axis_wide_kernel_stays_inside_its_buffers(gpu, po):
    """aai_axis_wide_kernel: images narrower than one 4-column vector, and a footprint wider than a strip"""
    for (W, H, sr, dr) in ((3, 50, 2, 1), (2, 300, 1, 1), (1, 1, 1, 1), (3000, 800, 700, 1)):
        for ang in (0.0, 90.0, 180.0, 270.0):
            for dtype in (("f32", "u8") if W == 3 else ("f32",)):
                guarded_forward(gpu, po, W, H, float(sr), float(dr), ang, dtype=dtype, B=3 if W < 4 else 2, expect="aai_axis_wide_kernel")
    guarded_forward(gpu, po, 3, 50, 2.0, 1.0, 0.0, C=1, entry="interleaved", expect="aai_axis_wide_kernel")


def test_axis_kernel_with_a_fixup_list(gpu, po, axis_knife_golden):
    """K1 followed by the double-precision pass over the pixels its plan lists (aai_axis_verify.hpp): geometries of
    tests/golden/axis_knife_cases.npz, the first three (by a fixed stride through the manifest) whose plan has flagged > 0"""
    _, manifest = axis_knife_golden
    ran = 0
    for i in range(0, len(manifest), 7):
        c = manifest[i]
        rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=1)
        gpu.prepare(rq)
        m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq))
        assert m, gpu.plan_shape(rq)
        if int(m.group(1)) == 0 or int(m.group(2)) != 0:
            continue
        k = guarded_forward(gpu, po, c["W"], c["H"], c["src_res"], c["dst_res"], c["angle"], iso=tuple(c["iso"]), layouts=(ran % 3, (ran + 2) % 3),
                            expect="aai_axis")
        ran += 1
        if ran == 3:
            break
    assert ran == 3, ran
    SEEN.add("aai_axis_kernel+fixup")


def test_axis_bands_stay_inside_their_footprint(gpu, po):
    for (W, H, sr, dr, ang, mode) in ((261, 200, 4, 1, 0.0, 1), (257, 190, 4, 1, 180.0, 2), (210, 303, 3, 1, 90.0, 1), (180, 211, 1, 1, 270.0, 1),
                                      (131, 97, 2, 1, 0.0, 1), (150, 30, 1, 2, 90.0, 2)):
        guarded_bands(gpu, po, W, H, float(sr), float(dr), ang, mode=mode, expect="aai_axis")


def test_axis_kernel_at_size(gpu, po):
    """4096^2 -> 1024^2 at 0 degrees: the smallest size K1's launch-shape measurement accepts, so the launch shape in force is
    whatever this device measured (the message carries aai_plan_info)."""
    guarded_forward(gpu, po, 4096, 4096, 4.0, 1.0, 0.0, B=1, layouts=((1, 1, 0, 3, 1, 0),), expect="aai_axis_kernel")


DENSE_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import torch            # (before the library: one HIP runtime per process)
import area_average_interpolation_amd as aai
from oracle import pyoracle as po
import test_gpu_memory_contract as m
aai.set_device(0)
for (W, H, sr, dr, ang, mode) in ((96, 80, 2.0, 1.0, 45.0, 1), (96, 80, 2.0, 1.0, 30.0, 1), (40, 9, 3.0, 1.0, 0.0, 1)):
    k = m.guarded_forward(aai, po, W, H, sr, dr, ang, mode=mode, layouts=(0, 1, 2), expect="strict")
    assert "dense=1" in aai.plan_shape(aai.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)), k
m.guarded_forward(aai, po, 40, 9, 3.0, 1.0, 0.0, C=2, layouts=(1, 2))
print("dense ok", sorted(m.SEEN))
"""


def test_dense_strict_form_stays_inside_its_buffers(gpu):
    """The double-precision pass as the only kernel of a request (`dense` plans): reached by lowering AAI_MAX_LISTED_PIXELS, which the
    library reads once -- hence a child process, whose own assertions count toward the coverage set."""
    _gate("aai_rotated_kernel")
    env = dict(os.environ, AAI_MAX_LISTED_PIXELS="10")
    p = subprocess.run([sys.executable, "-c", DENSE_CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "dense ok" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])
    assert "aai_rotated_kernel<area, strict>" in p.stdout, p.stdout[-2000:]
    SEEN.add("aai_rotated_kernel<area, strict>")


# ---- the rotated lattice --------------------------------------------------------------------------------------------------------------
def test_quad_kernels_stay_inside_their_buffers(gpu, po):
    for i, (W, H, sr, dr, ang) in enumerate(((90, 70, 3, 1, 17.5), (131, 97, 3, 1, 107.5), (64, 48, 1, 3, 200.0), (203, 167, 2.66, 2.99, 290.7))):
        for dtype in (("f32", "u8", "u16") if i == 0 else ("f32",)):
            guarded_forward(gpu, po, W, H, float(sr), float(dr), ang, mode=1, dtype=dtype, layouts=(i % 3, (i + 1) % 3), expect="aai_quad_kernel<area>")
            guarded_forward(gpu, po, W, H, float(sr), float(dr), ang, mode=2, dtype=dtype, layouts=((i + 1) % 3, (i + 2) % 3), expect="aai_quad_fast_kernel")
    for (W, H, sr, dr, ang, C, dtype) in ((128, 96, 3, 1, 17.5, 3, "f32"), (64, 64, 2, 1, 45.0, 2, "u8"), (64, 48, 1, 3, 30.0, 4, "u16")):
        guarded_forward(gpu, po, W, H, float(sr), float(dr), ang, C=C, dtype=dtype, expect="aai_quad_multi_kernel")


def test_cell_kernels_stay_inside_their_buffers(gpu, po):
    from area_average_interpolation_amd import _lib as L
    prefer = L.POLICY_PREFER_CELL
    for i, (W, H, sr, dr, ang, dtype) in enumerate(((140, 100, 2.2, 1.0, 17.5, "f32"), (120, 90, 2.0, 1.0, 290.0, "u16"), (96, 128, 1.0, 3.0, 45.0, "f32"),
                                                    (150, 130, 1.5, 1.0, 333.0, "u8"), (139, 101, 3.0, 1.0, 107.5, "f32"))):
        guarded_forward(gpu, po, W, H, sr, dr, ang, policy=prefer, dtype=dtype, layouts=(i % 3, (i + 2) % 3), expect="aai_cell_kernel<area>")
    for i, (W, H, sr, dr, ang, C, dtype) in enumerate(((101, 90, 2.0, 1.0, 107.5, 3, "f32"), (96, 80, 2.39, 1.0, 30.0, 3, "u8"), (70, 50, 1.0, 2.0, 200.0, 2, "u16"),
                                                       (90, 71, 2.2, 1.0, 17.5, 4, "f32"))):
        guarded_forward(gpu, po, W, H, sr, dr, ang, policy=prefer, C=C, dtype=dtype, layouts=(i % 3, (i + 1) % 3), expect="aai_cell_multi_kernel")
    # a size that takes the cell kernel without the hint (outputs from ~720 x 720 pixels)
    guarded_forward(gpu, po, 801, 800, 1.0, 1.0, 10.0, B=1, layouts=(0,), expect="aai_cell_kernel<area>", tag="aai_cell_kernel<area> unprompted")


def test_wide_and_runs_kernels_stay_inside_their_buffers(gpu, po):
    """the geometries of conftest.RUNS_CASES: aai_wide_kernel / aai_wide_fast_kernel up to 32 x 32 source pixels per window, the
    rows-as-runs kernel beyond that; plain and interleaved"""
    for k, (W, H, sr, dr, ang, off) in enumerate(RUNS_CASES):
        iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
        dtype = ("f32", "u8", "u16")[k % 3]
        guarded_forward(gpu, po, W, H, sr, dr, ang, mode=1, dtype=dtype, B=2, iso=iso, layouts=(k % 3, (k + 1) % 3))
        if k % 3 == 0:
            guarded_forward(gpu, po, W, H, sr, dr, ang, mode=2, dtype=dtype, B=2, iso=iso, layouts=((k + 2) % 3,))
    guarded_forward(gpu, po, 64, 64, 40.0, 1.0, 17.5, expect="aai_rotated_runs_kernel<area>")
    guarded_forward(gpu, po, 65, 63, 40.0, 1.0, 117.5, C=2, expect="aai_rotated_runs_kernel<area, channels>")
    guarded_forward(gpu, po, 120, 90, 8.0, 1.0, 33.3, C=3, dtype="u8")


def test_double_precision_kernels_stay_inside_their_buffers(gpu, po):
    dp = gpu.POLICY_DOUBLE_PRECISION
    for i, (W, H, sr, dr, ang) in enumerate(((90, 70, 3.0, 1.0, 17.5), (63, 49, 1.0, 2.0, 200.0), (131, 97, 2.5, 1.0, 290.0))):
        dtype = ("f32", "u8", "u16")[i]
        guarded_forward(gpu, po, W, H, sr, dr, ang, mode=1, policy=dp, dtype=dtype, layouts=(i, (i + 1) % 3), expect="aai_rotated_kernel<area>")
        guarded_forward(gpu, po, W, H, sr, dr, ang, mode=2, policy=dp, dtype=dtype, layouts=(i, (i + 2) % 3), expect="aai_rotated_kernel<fast>")
        guarded_forward(gpu, po, W, H, sr, dr, ang, mode=1, policy=dp, dtype=dtype, C=2 + i, layouts=(i,), expect="aai_rotated_kernel<area, channels>")
        guarded_forward(gpu, po, W, H, sr, dr, ang, mode=2, policy=dp, dtype=dtype, C=2 + i, layouts=((i + 1) % 3,), expect="aai_rotated_kernel<fast, channels>")


def test_fixup_beside_the_production_kernel_stays_inside_its_buffers(gpu, po):
    """A knife-edge geometry whose flagged pixels go to the double-precision pass BESIDE a production kernel that skips them (a side
    stream, from the second such launch of the process on): the case runs twice, so that its second pass is certainly beside."""
    W, H, sr, dr, ang = 300, 260, 3.0, 1.0, 30.0
    rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
    for again in range(2):
        guarded_forward(gpu, po, W, H, sr, dr, ang, B=2, layouts=(again, 2), expect="aai_quad_kernel<area>")
        m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq))
        assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, gpu.plan_shape(rq)
    SEEN.add("aai_quad_kernel<area> beside fix-up")


def test_rotated_bands_stay_inside_their_footprint(gpu, po):
    guarded_bands(gpu, po, 160, 120, 3.0, 1.0, 17.5, mode=1, expect="aai_quad_kernel")
    guarded_bands(gpu, po, 160, 120, 3.0, 1.0, 200.0, mode=2, expect="aai_quad_fast_kernel")
    guarded_bands(gpu, po, 141, 120, 2.5, 1.0, 107.5, mode=1, policy=0x200)         # AAI_POLICY_PREFER_CELL
    guarded_bands(gpu, po, 60, 50, 1.0, 3.0, 45.0, mode=1, expect="aai_quad_kernel")
    guarded_bands(gpu, po, 500, 400, 6.0, 1.0, 107.5, mode=1)
    guarded_bands(gpu, po, 400, 500, 8.0, 1.0, 300.0, mode=2)
    guarded_bands(gpu, po, 160, 120, 3.0, 1.0, 17.5, mode=1, policy=gpu.POLICY_DOUBLE_PRECISION, expect="aai_rotated_kernel<area>")


# ---- the samplers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 4])
def test_samplers_stay_inside_their_buffers(gpu, po, mode):
    """aai_sample_kernel shifts each dst row's columns left to the 256-byte boundary below its address and runs one more column of
    workgroups: dst base offsets of 0, 1 and 63 elements with padded strides give shift = 0, 1, 63 in row 0 and every other
    residue in the rows below; dst widths 63, 64, 65 and 129 put the row end on, before and after a wave boundary.  At 1:1 and 0
    degrees the waves that hold a first or last tap column take the clamped path, the others (129 wide: columns 1..63) the vector
    path; rotated and up-sampled cases have both in every row.  Planar and interleaved."""
    name = "aai_sample_kernel<%s>" % ("bilinear" if mode == 3 else "bicubic")
    shifts = [(1, 1, 5, 3, 0, 7), (3, 2, 6, 1, 1, 3), (5, 3, 7, 5, 63, 6)]
    for W in (63, 64, 65, 129):
        guarded_forward(gpu, po, W, 21, 1.0, 1.0, 0.0, mode=mode, layouts=shifts, expect=name)
    for (W, H, sr, dr, ang) in ((80, 60, 1.0, 2.0, 300.0), (129, 70, 1.0, 1.0, 90.0), (90, 77, 3.0, 1.0, 17.5), (40, 30, 1.0, 4.0, 45.0)):
        guarded_forward(gpu, po, W, H, sr, dr, ang, mode=mode, layouts=shifts, expect=name)
    for (W, H, sr, dr, ang, C) in ((80, 60, 2.0, 1.0, 17.5, 3), (65, 40, 1.0, 2.0, 200.0, 2), (63, 21, 1.0, 1.0, 0.0, 4)):
        guarded_forward(gpu, po, W, H, sr, dr, ang, mode=mode, C=C, layouts=shifts[1:], expect=name)
    guarded_bands(gpu, po, 129, 100, 1.0, 1.0, 0.0, mode=mode, expect=name)
    guarded_bands(gpu, po, 150, 100, 1.0, 2.0, 30.0, mode=mode, expect=name, tag=name + " band")


# ---- the adjoint ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_adjoint_stays_inside_its_buffers(gpu, mode):
    """aai_adjoint_batch_device_f32: gdst is the guarded SOURCE (NaN around it), gsrc the guarded destination (sentinel everywhere): every
    pixel of gsrc inside the image finite and equal, bit for bit, to the tight call; nothing else written."""
    import torch
    name = "aai_adjoint_gather_kernel<%s>" % ("area" if mode == 1 else "fast")
    _gate(name)
    B = 3
    try:
        for i, (W, H, sr, dr, ang) in enumerate(((90, 70, 3.0, 1.0, 17.5), (61, 47, 1.0, 2.0, 200.0), (129, 65, 4.0, 1.0, 0.0), (66, 131, 2.0, 1.0, 270.0),
                                                 (120, 90, 8.0, 1.0, 33.3))):
            rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            rc, msg, lay = gpu.query(rq)
            assert rc == 0, msg
            dW, dH = lay.dst_width, lay.dst_height
            g = np.random.default_rng(5 + i).random((B, dH, dW, 1)).astype(np.float32)
            tg = to_device(g)
            ts = torch.full((B, H, W), float("nan"), dtype=torch.float32, device="cuda")
            gpu.adjoint_device(rq, tg.data_ptr(), dW, ts.data_ptr(), W, _stream(), batch=B, dst_image_stride=dW * dH, src_image_stride=W * H)
            torch.cuda.synchronize()
            assert name in gpu.last_kernel(), gpu.last_kernel()
            tight = ts.cpu().numpy().reshape(B, H, W, 1)
            assert np.isfinite(tight).all()
            for li in (i % 3, (i + 1) % 3):
                sp, so, sg, dp, do, dg = LAYOUTS[li]
                gl = GuardedLayout((B, dH, dW, 1), "f32", dW + _pad(dW, dp), dH * (dW + _pad(dW, dp)) + dg, do)
                sl = GuardedLayout((B, H, W, 1), "f32", W + _pad(W, sp), H * (W + _pad(W, sp)) + sg, so)
                gdev, sdev = to_device(gl.make_src(g, "nan")), to_device(sl.make_dst())
                gpu.adjoint_device(rq, gl.ptr(gdev), gl.stride, sl.ptr(sdev), sl.stride, _stream(), batch=B, dst_image_stride=gl.image_stride,
                                   src_image_stride=sl.image_stride)
                torch.cuda.synchronize()
                SEEN.add(gpu.last_kernel())
                what = (gpu.last_kernel(), (W, H, sr, dr, ang, mode), "gdst stride %d image stride %d base %+d, gsrc stride %d image stride %d base %+d"
                        % (gl.stride, gl.image_stride, gl.base_offset, sl.stride, sl.image_stride, sl.base_offset))
                out = _check_guards(sl, sdev, what)
                bad = ~np.isfinite(out)
                assert not bad.any(), ("%d non-finite gsrc pixels, first at %s" % (int(bad.sum()), np.argwhere(bad)[0].tolist()), what)
                assert np.array_equal(out.view(np.int32), tight.view(np.int32)), what
    except AssertionError:
        FAILED.add(name.split("<")[0])
        raise


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_family_ran():
    """(last in the module) every family of the list ran guarded -- by aai.last_kernel(), with its <...> variant where variants differ --
    and none of them failed a case"""
    print("guarded kernels:", sorted(SEEN))
    print("module wall time so far: %.1f s" % (time.time() - T0))
    missing = [k for k in REQUIRED if k not in SEEN]
    assert not missing, (missing, sorted(SEEN))
    assert not FAILED, sorted(FAILED)
