"""CPU (no GPU): the case table of tests/knife_variants.py -- knife-edge geometries for every (mode, source type, channel count) the
double-precision fix-up pass is instantiated for -- is what it claims to be: every geometry is flagged in the CPU replay
(tests/emulation), none is dense, every item has its three ratio classes in two quadrants, every kernel that skips flagged pixels has
a case.  test_knife_variants_gpu.py runs the same table on the MI355X."""
import numpy as np
import pytest

import knife_variants as kv
import rot_variants as rv
from conftest import TOL, rel_err

K_MAX_LISTED = 1 << 24          # csrc/aai_engine.cpp kMaxListedPixels: a plan with more flagged pixels keeps no list (the dense form)


@pytest.fixture(scope="module")
def tab(hostemu):
    return kv.table(hostemu)


@pytest.fixture(scope="module")
def replayed(tab, aai, hostemu, po):
    """(origin, index, mode) -> (flagged pixels the replay reports, dst shape, worst error against the gold): each distinct geometry once,
    through the fp32 quad formulation (which replays the quad, fast and wide kernels) with the strict pass for the flagged pixels"""
    z, _ = kv.manifest()
    out = {}
    for case in tab:
        g, mode = case.geom, case.item[0]
        key = (g.origin, g.index, mode)
        if key in out:
            continue
        src = kv.base_image(po, g)
        rq = aai.make_request(g.W, g.H, g.src_res, g.dst_res, g.iso, g.angle, mode=kv.MODES[mode])
        hostemu.aai_emu_use_quad(1)
        try:
            dst, axis = hostemu.resample(rq, src)
        finally:
            hostemu.aai_emu_use_quad(0)
        pairs, pixels = hostemu.knife_stats()
        gold = kv.reference_golden(z, mode, g) if g.origin == "manifest" else kv.oracle_gold(po, mode, g, src)
        assert not axis and dst.shape == gold.shape, key
        assert np.array_equal(gold == 0, dst == 0), key
        out[key] = (pixels, dst.shape, float(rel_err(dst, gold).max()))
    return out


def test_every_case_is_flagged_in_the_replay_and_none_is_dense(tab, replayed):
    """The replay's flagged pixels with a knife pair are a subset of the pixels the plan's scan flags (pixel_on_knife_edge), so a
    positive count here is a positive `flagged` on the GPU; and the count is far below the list limit, let alone the pixel count."""
    assert len(replayed) >= 20
    for key, (pixels, shape, err) in replayed.items():
        assert pixels > 0, key
        assert pixels <= shape[0] * shape[1] < K_MAX_LISTED, (key, pixels, shape)
        assert err <= TOL, (key, err)                      # (and the replay, fix-up included, holds the bar on it)
        if key[0] == "manifest":
            assert max(shape) <= 44 and pixels > 10, (key, shape, pixels)      # small; and dense once the list limit is 10 (the dense cases)


def test_every_item_has_its_three_geometries(tab):
    _, m = kv.manifest()
    assert len(kv.ITEMS) == 24 and len(set(kv.ITEMS)) == 24
    for item in kv.ITEMS:
        mine = [c for c in tab if c.item == item]
        geoms = list(dict.fromkeys(c.geom for c in mine))
        assert geoms == kv.item_geometries(m, item)
        small = [g for g in geoms if g.origin == "manifest" and g.ratio_class != "large window"]
        assert len(small) == 3 and len({g.index for g in small}) == 3, item
        assert [g.ratio_class for g in small] == ["down", "one", "up"], item
        down, one, up = small
        assert down.src_res > down.dst_res and one.src_res == one.dst_res and up.src_res < up.dst_res, item
        assert len({kv.quadrant(g) for g in small}) >= 2, (item, [g.angle for g in small])
        assert all(max(g.W, g.H) <= 40 for g in small), item
        # one output tall enough for two aligned band cuts (rows 16 and 32)
        z, _ = kv.manifest()
        assert max(kv.reference_golden(z, item[0], g).shape[0] for g in small) > 32, item
        # the cell family gets every small geometry of an area item, a plain item one wide footprint
        extra = ["wide"] if item[2] == 1 else (["large window"] if item[0] == "area" else [])
        assert [g.ratio_class for g in geoms[3:]] == extra, item
        assert sum(1 for c in mine if c.policy == rv.PREFER_CELL) == (len([g for g in geoms if g.origin == "manifest"]) if item[0] == "area" else 0), item
    for mode, pool in kv.DENSE_POOL.items():
        down, up = (m[i] for i in pool)
        assert down["src_res"] > down["dst_res"] and up["src_res"] < up["dst_res"], (mode, pool)
        assert down["angle"] % 90 != 0 and up["angle"] % 90 != 0


def test_every_skipping_kernel_has_a_case(tab):
    """Every kernel that leaves flagged pixels to the fix-up appears beside a flagged geometry: plain fp32, and with a typed source and
    interleaved channels where it has such a form; the fp64 kernels too (the fix-up then runs behind them).  The kernels recorded
    are the probe's -- a few fixed points are restated here so that a probe that answered nonsense would not go unnoticed."""
    seen = {}
    for c in tab:
        seen.setdefault(kv.kernel_key(c), set()).add((c.item[1], c.item[2]))
    assert set(kv.SKIPPING) <= set(seen), set(kv.SKIPPING) - set(seen)
    assert any(C > 1 for (_, C) in seen["fp64"]) and {c.item[0] for c in tab if c.kernel == "fp64"} == {"area", "fast"}
    for k in kv.SKIPPING:
        forms = seen[k]
        if k in kv.INTERLEAVED_FORM:
            assert all(C > 1 for (_, C) in forms) and {"f32", "u8", "u16"} <= {T for (T, _) in forms}, (k, forms)
            assert {2, 3, 4} <= {C for (_, C) in forms}, (k, forms)
        else:
            assert forms == {("f32", 1), ("u8", 1), ("u16", 1)}, (k, forms)
    for c in tab:
        mode, T, C = c.item
        if c.geom.origin == "runs_cases":
            assert c.kernel == ("aai_wide_kernel" if mode == "area" else "aai_wide_fast_kernel"), kv.case_id(c)
        elif mode == "fast":
            assert c.kernel == ("aai_quad_fast_kernel" if C == 1 else "fp64"), kv.case_id(c)      # no interleaved fp32 fast kernel
            assert c.rows == (C == 1 and c.geom.ratio_class != "down"), kv.case_id(c)
        elif C == 1:
            assert c.kernel == ("aai_cell_kernel" if c.policy else "aai_quad_kernel"), kv.case_id(c)
        else:
            assert c.kernel in (("aai_cell_multi_kernel", "fp64") if c.policy else ("aai_quad_multi_kernel", "fp64")), kv.case_id(c)
