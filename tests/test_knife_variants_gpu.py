"""GPU (MI355X): the knife-edge handoff -- the plan flags dst pixels, the fp32 production kernel skips exactly those, the
double-precision fix-up pass (csrc/aai_rotated_strict.hip) writes them -- for typed, interleaved, batched and banded requests on
rotated lattices: the case table of tests/knife_variants.py (test_knife_variants_host.py checks the table itself on the CPU).

Gold: the committed outputs of the unmodified reference for plain fp32 images (and for the channel of an interleaved fp32 image that
carries the golden's image), the fp64 oracle for everything else.  Bar: conftest.TOL relative with the floor of 1e-3 x the value
scale, no pixel excepted, exact zeros exact.  Every case asserts `flagged > 0 dense=0` from aai_plan_info.  Nothing here reads the
reference tree.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import knife_variants as kv
from conftest import ROOT, TOL

pytestmark = pytest.mark.gpu

ITEM_IDS = [kv.item_id(it) for it in kv.ITEMS]


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


@pytest.fixture(scope="module")
def golds(po):
    """(geometry, mode, T, C, batch image) -> (source, oracle gold): computed once, shared by the tests, never written to"""
    store = {}

    def get(geom, mode, T, C, b):
        key = (geom.origin, geom.index, mode, T, C, b)
        if key not in store:
            src = kv.source(po, geom, T, C, b)
            gold = kv.oracle_gold(po, mode, geom, src)
            src.setflags(write=False)
            gold.setflags(write=False)
            store[key] = (src, gold)
        return store[key]
    return get


def _family_of(kernel_name):
    name = kernel_name.split("<")[0].split("+")[0]
    return "fp64" if name in ("aai_rotated_kernel", "aai_rotated_runs_kernel") else name


def _fp32_formulation(kernel_name):
    return any(t in kernel_name for t in ("aai_quad", "aai_cell", "aai_wide"))


@pytest.mark.parametrize("item", kv.ITEMS, ids=ITEM_IDS)
def test_listed_form_through_every_entry(gpu, hostemu, po, golds, item):
    """Every case of one (mode, T, C): three different images through the host entry one by one and through the device entry as one
    batch with padded source and dst strides (C = 1: the batch entry, C > 1: the interleaved entry); the dst padding keeps its sentinel.
    Per case: `flagged > 0 dense=0`, the production kernel the table expects, every image at the bar against its gold, batch image b
    bit-identical to the single call on image b, and every interleaved channel bit-identical to the planar call on that plane
    whenever both take an fp32 formulation or both a double-precision kernel (else: the same areas to ~1e-7, bound 2e-6)."""
    mode, T, C = item
    hi = kv.TYPES[T][3]
    z, _ = kv.manifest()
    mine = [c for c in kv.table(hostemu) if c.item == item]
    assert len(mine) >= 3
    worst = 0.0
    try:
        for case in mine:
            g, what = case.geom, kv.case_id(case)
            gpu.shutdown()                                               # (plan_flags below finds this case's plan, no earlier one)
            rq = kv.make_request(gpu, g, mode, case.policy)
            pairs = [golds(g, mode, T, C, b) for b in range(3)]
            srcs = [p[0] for p in pairs]
            assert not np.array_equal(srcs[0], srcs[1]) and not np.array_equal(srcs[0], srcs[2]) and not np.array_equal(srcs[1], srcs[2])
            singles = [kv.run_host(gpu, g, mode, case.policy, s) for s in srcs]
            kernel = gpu.last_kernel()
            flagged, dense = kv.plan_flags(gpu, rq, C)
            print("%-60s %-44s flagged=%d dense=%d" % (what, kernel, flagged, dense))
            assert flagged > 0 and dense == 0, (what, flagged, dense)
            assert _family_of(kernel) == case.kernel, (what, kernel, case.kernel)
            for b in range(3):
                worst = max(worst, kv.check_against(singles[b], pairs[b][1], hi, TOL, (what, "host", b)))
            if T == "f32" and g.origin == "manifest":
                ch = kv.GOLDEN_CHANNEL[C]
                kv.check_against(singles[0] if C == 1 else singles[0][:, :, ch], kv.reference_golden(z, mode, g), 1.0, TOL, (what, "reference golden"))
            outs = kv.run_device(gpu, rq, srcs, T, C)
            assert gpu.last_kernel() == kernel, (what, gpu.last_kernel(), kernel)
            for b in range(3):
                got = outs[b, :, :, 0] if C == 1 else outs[b]
                assert np.array_equal(got, singles[b]), (what, "batch image %d differs from the single call" % b)
            if C > 1:
                for c in range(C):
                    planar = kv.run_host(gpu, g, mode, case.policy, np.ascontiguousarray(srcs[0][:, :, c]))
                    if _fp32_formulation(gpu.last_kernel()) == _fp32_formulation(kernel):
                        assert np.array_equal(singles[0][:, :, c], planar), (what, c, kernel, gpu.last_kernel())
                    else:
                        assert float(kv.rel_err_scaled(singles[0][:, :, c], planar, hi).max()) <= 2e-6, (what, c, kernel, gpu.last_kernel())
                        assert np.array_equal(singles[0][:, :, c] == 0, planar == 0), (what, c)
    finally:
        gpu.shutdown()
    print("%s: %d cases, worst rel err %.2e" % (kv.item_id(item), len(mine), worst))


# ---- the handoff ------------------------------------------------------------------------------------------------------------------
HANDOFF_ITEMS = [("area", "f32", 3), ("area", "u8", 1), ("area", "u8", 2), ("area", "u16", 1), ("area", "u16", 4), ("fast", "u8", 1), ("fast", "u16", 1)]


@pytest.mark.parametrize("item", HANDOFF_ITEMS, ids=[kv.item_id(it) for it in HANDOFF_ITEMS])
def test_typed_and_interleaved_kernels_leave_exactly_the_flagged_pixels_alone(gpu, hostemu, po, golds, item):
    """The method of test_production_kernels_leave_exactly_the_flagged_pixels_alone (test_gpu_parity.py) at the table's small
    geometries, for the forms it does not reach: with the fix-up switched off (aai_debug_skip_fixup) a sentinel-filled dst keeps the
    sentinel in exactly `flagged` pixels of EACH image of a batch of two -- in all C elements of those pixels and in no other element
    -- and the normal call differs from that run in exactly those elements.  Every case of the item whose production kernel skips."""
    mode, T, C = item
    mine = [c for c in kv.table(hostemu) if c.item == item and kv.kernel_key(c) in kv.SKIPPING]
    assert mine
    ran = set()
    try:
        for case in mine:
            g, what = case.geom, kv.case_id(case)
            gpu.shutdown()
            rq = kv.make_request(gpu, g, mode, case.policy)
            srcs = [golds(g, mode, T, C, b)[0] for b in range(2)]
            full = kv.run_device(gpu, rq, srcs, T, C)
            kernel = gpu.last_kernel()
            assert _family_of(kernel) == case.kernel, (what, kernel)
            flagged, dense = kv.plan_flags(gpu, rq, C)
            assert flagged > 0 and dense == 0, (what, flagged, dense)
            assert not (full == kv.SENTINEL).any(), what
            gpu.debug_skip_fixup(True)
            holes = kv.run_device(gpu, kv.make_request(gpu, g, mode, case.policy), srcs, T, C)
            gpu.debug_skip_fixup(False)
            left = holes == kv.SENTINEL                                    # [B, dH, dW, C]
            for b in range(2):
                pixels = left[b].all(axis=2)
                assert int(pixels.sum()) == flagged, (what, b, int(pixels.sum()), flagged)
                assert np.array_equal(left[b].any(axis=2), pixels), (what, b, "a flagged pixel kept only some of its channels")
            assert np.array_equal(left[0], left[1]), what                  # (the flags are the geometry's, not the image's)
            assert np.array_equal(holes[~left], full[~left]), what
            ran.add(kv.kernel_key(case))
            print("%-60s %-44s flagged=%d" % (what, kernel, flagged))
    finally:
        gpu.debug_skip_fixup(False)
        gpu.shutdown()
    expect = {("area", 1): {"aai_quad_kernel", "aai_cell_kernel", "aai_wide_kernel"}, ("area", 2): {"aai_quad_multi_kernel", "aai_cell_multi_kernel"},
              ("fast", 1): {"aai_quad_fast_kernel", "aai_quad_fast_kernel/rows", "aai_wide_fast_kernel"}}[(mode, min(C, 2))]
    assert expect <= ran, (item, ran)


# ---- row bands --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", kv.ITEMS, ids=ITEM_IDS)
def test_row_bands_of_flagged_geometries_equal_the_full_image(gpu, hostemu, po, item):
    """Every geometry (and policy) of the item through aai_resample_band_device_f32, for each aligned cut r0 = 16, 32, ... the entry
    accepts: rows [0, r0) and [r0, dH) from buffers that hold only the band's source footprint, into sentinel-filled buffers -- bit-
    identical to the same rows of the full call, no sentinel left.  The band entry takes plain fp32 images only, so an item's source
    type and channel count enter through the image alone (its last plane, quantised, as floats): the band filter of the listed form
    (`dy >= r.dyBase`, `dy < r.dyEnd`, `dy - r.dyBase`) is reached for T = float, MULTI = false.  Where the flagged pixels are comes
    from a run with the fix-up off; per item at least one band starts below a flagged pixel (the filter drops it), one starts above one
    at a row other than 0 (rebasing) -- and the band before it ends above that one --, and one output takes two cuts."""
    mode, T, C = item
    hi = kv.TYPES[T][3]
    mine = [c for c in kv.table(hostemu) if c.item == item]
    above = below = cuts = two_cuts = 0
    try:
        for case in mine:
            g, what = case.geom, kv.case_id(case)
            gpu.shutdown()
            img = kv.quantise(kv.planes(kv.base_image(po, g), C)[C - 1], T).astype(np.float32)
            rq = kv.make_request(gpu, g, mode, case.policy)
            full = kv.run_device(gpu, rq, [img], "f32", 1)[0, :, :, 0]
            kernel = gpu.last_kernel()
            kv.check_against(full, kv.oracle_gold(po, mode, g, img), hi, TOL, what)
            flagged, dense = kv.plan_flags(gpu, rq, 1)
            assert flagged > 0 and dense == 0, (what, flagged, dense)
            assert not (full == kv.SENTINEL).any(), what
            gpu.debug_skip_fixup(True)
            holes = kv.run_device(gpu, kv.make_request(gpu, g, mode, case.policy), [img], "f32", 1)[0, :, :, 0]
            gpu.debug_skip_fixup(False)
            rows = np.flatnonzero((holes == kv.SENTINEL).any(axis=1))
            assert int((holes == kv.SENTINEL).sum()) == flagged and len(rows), (what, kernel)     # (plain fp32 requests here all take a skipping kernel)
            dH, dW = full.shape
            for r0 in range(16, dH, 16):
                for (b0, b1) in ((0, r0), (r0, dH)):
                    band = kv.run_band(gpu, rq, img, b0, b1, dW)
                    assert not (band == kv.SENTINEL).any(), (what, b0, b1)
                    assert np.array_equal(band, full[b0:b1]), (what, b0, b1, kernel, gpu.last_kernel())
                cuts += 1
                above += int((rows < r0).any())          # [r0, dH) starts below a flagged pixel: the filter drops it
                below += int((rows >= r0).any())         # [r0, dH) holds one, rebased to its row r0; [0, r0) ends above it
            two_cuts += int(dH > 32)
    finally:
        gpu.debug_skip_fixup(False)
        gpu.shutdown()
    print("%s: %d cuts; with a flagged pixel above the cut %d, below it %d" % (kv.item_id(item), cuts, above, below))
    assert cuts >= 3 and two_cuts > 0 and above > 0 and below > 0, (item, cuts, two_cuts, above, below)


# ---- the dense form ---------------------------------------------------------------------------------------------------------------
def test_dense_form_of_every_instantiation(gpu, po):
    """AAI_MAX_LISTED_PIXELS=10 in a fresh child process (the hook is read once): knife_variants.dense_child -- rotated geometries for
    both modes x three source types x C in {1, 3}, single, padded batch of two and (plain fp32) one band, against the oracle at the
    bar; aai_last_kernel() names the strict form and aai_plan_info says dense=1."""
    gpu.shutdown()
    env = dict(os.environ, AAI_MAX_LISTED_PIXELS="10")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "knife_variants.py")], capture_output=True, text=True, env=env, timeout=600)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "dense ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("dense ") and l != "dense ok"]
    assert len(lines) == 2 * len(kv.DENSE_ITEMS) == 24, lines
    for (mode, T, C) in kv.DENSE_ITEMS:
        assert sum(1 for l in lines if l.split()[1] == kv.item_id((mode, T, C)) and "aai_rotated_kernel<%s, strict>" % mode in l) == 2, ((mode, T, C), lines)
