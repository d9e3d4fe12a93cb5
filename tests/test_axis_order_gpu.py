"""GPU (MI355X): K1's banded workgroup order (axis_block_order, csrc/aai_plan.hpp; test_axis_order_host.py checks the map itself).

The strip kernel's streaming class -- plain fp32, nontemporal loads, windows that share no source row, quadrants 0 and 2 -- takes its
(strip block, row block) from the map instead of blockIdx (the transposed quadrants lost time under it and keep launch order).  A wrong map drops or doubles a row block, so every case runs between guard margins
(tests/guard_layout.py): the destination starts as NaN sentinels and none may remain inside it (doubled blocks write equal values, so
the dropped one shows), no element around it may change, and the result is held against the CPU oracle at the suite's bar (1e-5
relative, conftest.rel_err) with the same zero pattern.  Plain fp32, both modes.

Each case first asks the variant probe (aai_emu_axis_variant: the launcher's own axis_launch_shape on the plan's own tables) for the
grid, the load policy and the row sharing and asserts the values the case was chosen for, so that a later change of the tables cannot
hollow the test.  The shapes are the smallest at which the order can go wrong (W x H source, ratio, angle -> gridX x gridY):

  1   600 x 44   4:1   0          1 x 11   one full group of 8 row blocks and a remainder of 3
  2  2300 x 28   4:1   0          3 x 7    a short last workgroup along x; remainder only
  3  2300 x 100  4:1 180          3 x 25   both flips
  4  8200 x 68   4:1   0          9 x 17   gridX neither 8 nor a power of two; batch 3 (blockIdx.z), padded row and image strides
  5  2100 x 64   8:1  90 / 270    3 x 4    transposed branch A, two output rows per workgroup: exempt by measurement, launch order,
  5t 2100 x 200  8:1  90 / 270    3 x 13   parity only (5t added: a grid with a full group of 8 row blocks, should the exemption ever go)
  6  dst rows [5, 25) of case 3   3 x 20   band-restricted tables (resample_band_device)
  6t dst rows [5, 29) of 2300 x 120 at 180 degrees   3 x 24   (case 3 has 25 dst rows, so the band [5, 29) runs on the taller twin)
  7  2300 x 90   8192:2731  0     3 x 15   area mode: output rows share source rows -- the exempt class (cached loads, launch order),
                                           parity only; fast mode's windows share nothing there and run banded (3 x 8, four rows)
"""
import collections

import numpy as np
import pytest

import axis_variants as av
from conftest import TOL, rel_err
from guard_layout import GuardedLayout, to_device

pytestmark = pytest.mark.gpu

AREA, FAST = 1, 2
# expect: mode -> (gridX, gridY, nt, rows shared, transposed)
Case = collections.namedtuple("Case", "name W H ratio angle batch padded band expect")


def _both(gx, gy, transposed=0):
    return {AREA: (gx, gy, 1, 0, transposed), FAST: (gx, gy, 1, 0, transposed)}


CASES = [
    Case("1-one-group-and-remainder", 600, 44, 4.0, 0.0, 1, False, None, _both(1, 11)),
    Case("2-remainder-only-short-last-workgroup", 2300, 28, 4.0, 0.0, 1, False, None, _both(3, 7)),
    Case("3-both-flips", 2300, 100, 4.0, 180.0, 1, False, None, _both(3, 25)),
    Case("4-gridx9-batch3-padded", 8200, 68, 4.0, 0.0, 3, True, None, _both(9, 17)),
    Case("5-transposed-90", 2100, 64, 8.0, 90.0, 1, False, None, _both(3, 4, 1)),
    Case("5-transposed-270", 2100, 64, 8.0, 270.0, 1, False, None, _both(3, 4, 1)),
    Case("5t-transposed-90-tall", 2100, 200, 8.0, 90.0, 1, False, None, _both(3, 13, 1)),
    Case("5t-transposed-270-tall", 2100, 200, 8.0, 270.0, 1, False, None, _both(3, 13, 1)),
    Case("6-band-5-25-of-case-3", 2300, 100, 4.0, 180.0, 1, False, (5, 25), _both(3, 20)),
    Case("6t-band-5-29", 2300, 120, 4.0, 180.0, 1, False, (5, 29), _both(3, 24)),
    Case("7-shared-rows-exempt", 2300, 90, 8192.0 / 2731.0, 0.0, 1, False, None, {AREA: (3, 15, 0, 1, 0), FAST: (3, 8, 1, 0, 0)}),
]


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    aai.set_device(0)
    return aai


@pytest.fixture(scope="module")
def probe(hostemu):
    return av.Prober(hostemu)


@pytest.fixture(scope="module")
def golds(po):
    """oracle outputs, computed once per (geometry, mode, image) and shared by the whole image and its bands"""
    memo = {}

    def gold(c, mode, b):
        key = (c.W, c.H, c.ratio, c.angle, mode, b)
        if key not in memo:
            src = po.synth_image(c.W, c.H, 11 + b)
            iso = ((c.W - 1) / 2.0, (c.H - 1) / 2.0)
            memo[key] = (src, po.oracle_run(po.MODE_EXACT if mode == AREA else po.MODE_FAST, src.astype(np.float64), c.ratio, 1.0, iso, c.angle).dst)
        return memo[key]

    return gold


@pytest.mark.parametrize("mode", (AREA, FAST), ids=("area", "fast"))
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_banded_order_against_oracle_between_guards(gpu, probe, golds, c, mode):
    import torch
    iso = ((c.W - 1) / 2.0, (c.H - 1) / 2.0)
    v = probe(c.W, c.H, c.ratio, c.angle, mode, iso, 1, 4, c.batch, c.band or (-1, -1))
    assert av.KERNELS[v.kernel] == "aai_axis_kernel", v
    assert (v.grid_x, v.grid_y, v.nt, v.rows_shared, v.transposed) == c.expect[mode], (c.name, v)
    if c.name.startswith("5"):
        assert v.branches == 1 and v.rows > 1, v                            # branch A alone, several output rows per workgroup
    banded = bool(v.nt and not v.rows_shared and not v.transposed)          # what AxisShape::banded says for a plain fp32 image
    rq = gpu.make_request(c.W, c.H, c.ratio, 1.0, iso, c.angle, mode=mode)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0 and (lay.dst_width, lay.dst_height) == (v.dW, v.dH), msg
    dW, dH = v.dW, v.dH
    stream = torch.cuda.current_stream().cuda_stream
    pairs = [golds(c, mode, b) for b in range(c.batch)]
    gpu.shutdown()                                                          # (no plan of an earlier case: plan_shape below is this one's)
    try:
        if c.band is None:
            sl = GuardedLayout((c.batch, c.H, c.W, 1), "f32", c.W + 5 if c.padded else None, c.H * (c.W + 5) + 7 if c.padded else None, 1)
            dl = GuardedLayout((c.batch, dH, dW, 1), "f32", dW + 3 if c.padded else None, dH * (dW + 3) + 6 if c.padded else None, 2)
            sdev = to_device(sl.make_src(np.stack([s for s, _ in pairs]), "nan"))
            ddev = to_device(dl.make_dst())
            gpu.resample_device(rq, sl.ptr(sdev), sl.stride, dl.ptr(ddev), dl.stride, stream, batch=c.batch,
                                src_image_stride=sl.image_stride, dst_image_stride=dl.image_stride)
            torch.cuda.synchronize()
            rows = (0, dH)
            assert ("order=banded" if banded else "order=launch") in gpu.plan_shape(rq).split(), gpu.plan_shape(rq)
        else:
            r0, r1 = c.band
            a, b = gpu.band_source_rows(rq, r0, r1)
            sl = GuardedLayout((1, b - a, c.W, 1), "f32", None, None, 1)
            dl = GuardedLayout((1, r1 - r0, dW, 1), "f32", None, None, 2)
            sdev = to_device(sl.make_src(pairs[0][0][a:b][None], "nan"))
            ddev = to_device(dl.make_dst())
            gpu.resample_band_device(rq, r0, r1, sl.ptr(sdev), sl.stride, dl.ptr(ddev), dl.stride, stream)
            torch.cuda.synchronize()
            rows = (r0, r1)
        assert gpu.last_kernel().split("+")[0] == "aai_axis_kernel", gpu.last_kernel()
        out, first, count = dl.check_dst(ddev)
        assert count == 0, "%d elements around the destination were written, first: %s" % (count, dl.describe(first))
        assert dl.sentinels_left(out) == 0, "%d dst pixels were never written (a dropped row block)" % dl.sentinels_left(out)
        assert np.isfinite(out).all(), "poison from outside the source reached the output"
        for i, (_, gold) in enumerate(pairs):
            got, want = out[i, :, :, 0], gold[rows[0]:rows[1]]
            assert got.shape == want.shape, (got.shape, want.shape)
            err = float(rel_err(got, want).max())
            print("%-40s mode %d image %d grid %d x %d %s  rel err %.2e" % (c.name, mode, i, v.grid_x, v.grid_y, "banded" if banded else "launch", err))
            assert err <= TOL, (c.name, mode, i, err)
            assert np.array_equal(got == 0, want == 0), (c.name, mode, i)
    finally:
        gpu.shutdown()
