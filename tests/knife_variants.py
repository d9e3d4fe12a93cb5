"""Knife-edge requests in every form the double-precision fix-up pass is instantiated for (helper of test_knife_variants_host.py /
test_knife_variants_gpu.py; needs no GPU).

The pass (csrc/aai_rotated_strict.hip) writes the dst pixels the plan's scan flagged and the fp32 production kernels skipped:

    listed form   aai_fixup_group_kernel<MODE, T, MULTI>           2 modes x {f32, u8, u16} x {plain, interleaved}
    dense form    aai_rotated_kernel<MODE, strict, T, MULTI>       the same twelve, when the plan keeps no list

ITEMS: one item per (mode, T, C), C = 1..4 -- 24 items, two per listed instantiation of MULTI = false, six per MULTI = true.

CASES: per item three geometries of tests/golden/knife_cases.npz (outputs of the unmodified reference; origin "manifest") for which
the CPU replay (tests/emulation, hostemu.knife_stats()) reports flagged pixels: one down-sampling, one 1 : 1, one up-sampling (a
replicated source: virt_offset with scale > 1), reduced angles in two quadrants at least, one of them with more than 32 dst rows
(two aligned band cuts).  The manifest has enough of them in fast mode too (a 1 : 1 geometry only once), so no structured geometry
of this file's own making is needed; the choice is written down by manifest index in POOL and the host module replays it.
Area items run every geometry a second time with AAI_POLICY_PREFER_CELL (the cell family), C = 1 items add the wide-footprint
geometry of conftest.RUNS_CASES that lists pixels in their mode (origin "runs_cases": no reference golden, the oracle is the gold),
interleaved area items a fourth manifest geometry whose window fp32 pixels of three and four channels cannot stage (LARGE_WINDOW).

Each case records the production kernel expected beside the fix-up: what the variant probe of tests/rot_variants.py -- the launchers'
own header functions -- answers for the request.  SKIPPING names the kernels that leave flagged pixels to the fix-up (the ones that
test `skipMasks`: csrc/aai_rotated_quad.hip, aai_rotated_cell.hip, aai_rotated_wide.hip); the fp64 kernels write every pixel and the
fix-up overwrites the flagged ones behind them.
"""
import collections
import json
import os

import numpy as np

import rot_variants as rv
from conftest import GOLDEN, RUNS_CASES

MODES = {"area": rv.MODE_AREA, "fast": rv.MODE_FAST}
TYPES = rv.TYPES                                   # name -> (numpy type, bytes, AAI_DTYPE_*, value scale)
ITEMS = [(mode, T, C) for mode in MODES for T in TYPES for C in rv.CHANNELS]

# indices into the manifest of knife_cases.npz, by ratio class; item k of a mode (k = 4 x type + C - 1) takes one of each, the pools
# turned against each other so that every item meets two quadrants.  Chosen from the replay's report (test_knife_variants_host.py
# checks each): down 2 : 1 at 30 / 135 / 315 / 135 degrees (fast: 30 / 210 / 135 at 2 sqrt 2 : 1 / atan 1/2), 1 : 1 at 30 / 60 / 210 / 30
# (fast: the manifest's only one, 60 degrees), up 1 : 2 at 30 / 135 / 315 / 315 (fast: 210 degrees, two isocenters).
POOL = {
    "area": {"down": (0, 126, 168, 127), "one": (156, 10, 11, 51), "up": (138, 180, 182, 14)},
    "fast": {"down": (1, 148, 141, 65), "one": (53,), "up": (159, 161)},
}
# interleaved area items add the manifest's 2 sqrt 2 : 1 geometry at 135 degrees: its window is too large to stage for fp32 pixels of three
# and four channels, which take the double-precision kernel there (aai_rotated_kernel<area, channels>, the fix-up behind it)
LARGE_WINDOW = 141
# the wide-footprint geometries: index into RUNS_CASES
WIDE = {"area": 8, "fast": 9}

# every kernel that tests the plan's lane masks and returns on a flagged pixel; aai_quad_fast_kernel has two of them (the 16 x 4
# wave and the row-shaped wave aai_quad_fast_rows_kernel, which aai_last_kernel() reports under one name: Case.rows tells them apart)
SKIPPING = ("aai_quad_kernel", "aai_quad_fast_kernel", "aai_quad_fast_kernel/rows", "aai_quad_multi_kernel", "aai_cell_kernel",
            "aai_cell_multi_kernel", "aai_wide_kernel", "aai_wide_fast_kernel")
# which of them have a form for typed sources / interleaved channels (wide: plain images only)
TYPED_FORM = SKIPPING
INTERLEAVED_FORM = ("aai_quad_multi_kernel", "aai_cell_multi_kernel")

Geometry = collections.namedtuple("Geometry", "origin index W H src_res dst_res iso angle seed ratio_class")
Case = collections.namedtuple("Case", "item geom policy kernel rows")


def manifest():
    z = np.load(os.path.join(GOLDEN, "knife_cases.npz"))
    return z, json.loads(bytes(z["manifest"]).decode())


def _manifest_geometry(m, i, ratio_class):
    c = m[i]
    return Geometry("manifest", i, c["W"], c["H"], float(c["src_res"]), float(c["dst_res"]), tuple(c["iso"]), float(c["angle"]), c["seed"], ratio_class)


def _wide_geometry(k):
    W, H, sr, dr, ang, off = RUNS_CASES[k]
    return Geometry("runs_cases", k, W, H, float(sr), float(dr), ((W - 1) / 2.0 + off[0], (H - 1) / 2.0 + off[1]), float(ang), 5, "wide")


def item_geometries(m, item):
    mode, T, C = item
    k = list(TYPES).index(T) * 4 + C - 1
    pool = POOL[mode]
    geoms = [_manifest_geometry(m, pool[cls][k % len(pool[cls])], cls) for cls in ("down", "one", "up")]
    if C == 1:
        geoms.append(_wide_geometry(WIDE[mode]))
    elif mode == "area":
        geoms.append(_manifest_geometry(m, LARGE_WINDOW, "large window"))
    return geoms


def quadrant(geom):
    return int((geom.angle % 360.0) // 90)


def expected_kernel(probe, item, geom, policy):
    """(family, row-shaped fast wave) the probe names for the request"""
    mode, T, C = item
    v = probe(geom.src_res, geom.angle, MODES[mode], policy, C, TYPES[T][1], W=geom.W, H=geom.H, iso=geom.iso, dst_res=geom.dst_res)
    fam = rv.FAMILIES[v.family]
    return fam, bool(fam == "aai_quad_fast_kernel" and v.fast_row_shaped)


_TABLE = {}


def table(lib):
    """[Case] in item order -- built once per process.  lib: conftest's hostemu"""
    if "t" not in _TABLE:
        probe = rv.Prober(lib)
        _, m = manifest()
        cases = []
        for item in ITEMS:
            for geom in item_geometries(m, item):
                policies = (0, rv.PREFER_CELL) if item[0] == "area" and geom.origin == "manifest" else (0,)
                for policy in policies:
                    fam, rows = expected_kernel(probe, item, geom, policy)
                    cases.append(Case(item, geom, policy, fam, rows))
        _TABLE["t"] = cases
    return _TABLE["t"]


def kernel_key(case):
    return case.kernel + ("/rows" if case.rows else "")


def case_id(case):
    g = case.geom
    return "%s-%s-C%d/%s%d(%s %g:%g at %g)%s" % (case.item + (g.origin[0], g.index, g.ratio_class, g.src_res, g.dst_res, g.angle, "+cell" if case.policy else ""))


def item_id(item):
    return "%s-%s-C%d" % item


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def base_image(po, geom):
    """the image the reference golden was made from (float32, values in [0, 1))"""
    return po.synth_image(geom.W, geom.H, geom.seed)


def quantise(img, T):
    """a float image in [0, 1] as source type T (f32: itself)"""
    npdt, _, _, hi = TYPES[T]
    return img.astype(np.float32) if T == "f32" else np.floor(img.astype(np.float64) * (hi - 1.0)).astype(npdt)


def planes(img, C, b=0):
    """C different planes of batch image b, all derived from `img`; plane GOLDEN_CHANNEL[C] of image 0 is img itself.  Returns float
    images in [0, 1] -- quantise() makes the source type of them."""
    one = np.float32(1.0)
    variants = [img[::-1], img, one - img, img[:, ::-1]]
    if C == 1:
        variants = [img]
    if b == 1:
        variants = [np.roll(v[::-1], 3, axis=1) for v in variants]
    elif b == 2:
        variants = [one - np.roll(v, 5, axis=0) for v in variants]
    return [np.ascontiguousarray(v, dtype=np.float32) for v in variants[:C]]


GOLDEN_CHANNEL = {1: 0, 2: 1, 3: 1, 4: 1}


def source(po, geom, T, C, b=0):
    """batch image b of a case in its source type: [H, W] (C = 1) or [H, W, C]"""
    ps = [quantise(p, T) for p in planes(base_image(po, geom), C, b)]
    return ps[0] if C == 1 else np.ascontiguousarray(np.stack(ps, axis=2))


def oracle_gold(po, mode, geom, src):
    """the fp64 oracle on `src` (as source(...) returns it), per plane: [dH, dW] or [dH, dW, C] float64"""
    omode = po.MODE_EXACT if mode == "area" else po.MODE_FAST
    run = lambda plane: po.oracle_run(omode, np.ascontiguousarray(plane, dtype=np.float64), geom.src_res, geom.dst_res, geom.iso, geom.angle).dst
    if src.ndim == 2:
        return run(src)
    return np.stack([run(src[:, :, c]) for c in range(src.shape[2])], axis=2)


def reference_golden(z, mode, geom):
    """the unmodified reference's output for the geometry's own fp32 image (manifest geometries only)"""
    assert geom.origin == "manifest"
    return z["k%03d_%s" % (geom.index, "exact" if mode == "area" else "fast")]


def rel_err_scaled(got, gold, hi):
    """conftest.rel_err with the project's floor of 1e-3 x the value scale"""
    got, gold = np.asarray(got, dtype=np.float64), np.asarray(gold, dtype=np.float64)
    return np.abs(got - gold) / np.maximum(np.abs(gold), 1e-3 * hi)


# ---- the dense form: a child process (AAI_MAX_LISTED_PIXELS is read once) ---------------------------------------------------------
DENSE_ITEMS = [(mode, T, C) for mode in MODES for T in TYPES for C in (1, 3)]
DENSE_POOL = {"area": (0, 182), "fast": (148, 159)}        # manifest indices: one down-sampling, one up-sampling; quadrants 0 / 3 and 2


# ---- launching (GPU; torch is imported late so that the host module needs none) ---------------------------------------------------
SENTINEL = -7.0              # no output is negative: the sources are not


def make_request(aai, g, mode, policy=0):
    return aai.make_request(g.W, g.H, g.src_res, g.dst_res, g.iso, g.angle, mode=MODES[mode], policy=policy)


def run_host(aai, geom, mode, policy, src):
    """the host entry for one image ([H, W]: aai_resample_host, [H, W, C]: aai_resample_interleaved_host)"""
    args = (src, geom.src_res, geom.dst_res, geom.iso, geom.angle)
    if src.ndim == 2:
        rc, msg, dst, _, _ = aai.resample_host(*args, mode=MODES[mode], policy=policy)
    else:
        rc, msg, dst, _ = aai.resample_interleaved_host(*args, mode=MODES[mode], policy=policy)
    assert rc == 0, msg
    return dst


def to_device(arrays, pad=5, extra_rows=1):
    """[B] host images of one shape -> one device tensor with `pad` elements of row padding and `extra_rows` rows between the images;
    returns (tensor, row stride, image stride) in elements"""
    import torch
    a0 = arrays[0]
    H, row = a0.shape[0], int(np.prod(a0.shape[1:]))
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16}[a0.dtype]
    t = torch.zeros((len(arrays), H + extra_rows, row + pad), dtype=tdt, device="cuda")
    for b, a in enumerate(arrays):
        flat = np.array(a).reshape(H, row)                             # (a copy: the shared sources are read-only)
        t[b, :H, :row] = torch.from_numpy(flat.view(np.int16) if a.dtype == np.uint16 else flat).cuda()
    return t, row + pad, (H + extra_rows) * (row + pad)


def run_device(aai, rq, srcs, T, C, dpad=3, extra_rows=1):
    """the batch device entry (C = 1) or the interleaved device entry (C > 1) on [B] images with padded source and dst strides, the
    dst pre-filled with SENTINEL; asserts that the dst padding keeps it; returns [B, dH, dW, C] float32 (C = 1 included)"""
    import torch
    rc, msg, lay = aai.query(rq)
    assert rc == 0, msg
    dW, dH = lay.dst_width, lay.dst_height
    t, stride, image = to_device(srcs)
    B = len(srcs)
    out = torch.full((B, dH + extra_rows, dW * C + dpad), SENTINEL, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dimage = (dH + extra_rows) * (dW * C + dpad)
    if C == 1:
        aai.resample_device(rq, t.data_ptr(), stride, out.data_ptr(), dW + dpad, st, batch=B, src_image_stride=image, dst_image_stride=dimage,
                            src_dtype=TYPES[T][2])
    else:
        aai.resample_interleaved_device(rq, C, t.data_ptr(), stride, out.data_ptr(), dW * C + dpad, st, batch=B, src_image_stride=image,
                                        dst_image_stride=dimage, src_dtype=TYPES[T][2])
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, :, dW * C:] == SENTINEL).all() and (host[:, dH:, :] == SENTINEL).all()        # the padding is nobody's to write
    return host[:, :dH, :dW * C].reshape(B, dH, dW, C)


def run_band(aai, rq, src, b0, b1, dW):
    """dst rows [b0, b1) of one plain fp32 image through aai_resample_band_device_f32 from a buffer that holds only the band's source
    footprint, into a SENTINEL-filled buffer"""
    import torch
    a, b = aai.band_source_rows(rq, b0, b1)
    assert 0 <= a < b <= src.shape[0]
    band_src = torch.from_numpy(np.ascontiguousarray(src[a:b])).cuda()
    band_dst = torch.full((b1 - b0, dW), SENTINEL, dtype=torch.float32, device="cuda")
    aai.resample_band_device(rq, b0, b1, band_src.data_ptr(), src.shape[1], band_dst.data_ptr(), dW, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return band_dst.cpu().numpy()


def plan_flags(aai, rq, C):
    """(flagged, dense) of the request's cached plan (aai_plan_info)"""
    import re
    text = aai.plan_shape(rq, channels=C)
    m = re.search(r"flagged=(\d+) dense=(\d+)", text)
    assert m, text
    return int(m.group(1)), int(m.group(2))


def check_against(got, gold, hi, tol, what):
    """the bar: `tol` relative with the floor of 1e-3 x the value scale, no pixel excepted, exact zeros exact; returns the worst error"""
    assert got.dtype == np.float32 and got.shape == gold.shape, (what, got.shape, gold.shape)
    err = float(rel_err_scaled(got, gold, hi).max())
    assert err <= tol, (what, err)
    assert np.array_equal(gold == 0, got == 0), what
    return err


def dense_child():
    """Runs in a process of its own with AAI_MAX_LISTED_PIXELS=10 (test_knife_variants_gpu.py starts it): every plan with more than ten
    flagged pixels keeps no list, and the strict form of aai_rotated_kernel computes the whole image.  All twelve instantiations, each
    as a single image (host entry), as a padded batch of two (device entry) and -- plain fp32 images, the only kind the band entry
    takes -- as one band that starts at row 16; every run against the oracle at the bar of the listed form."""
    import torch            # (before the library: one HIP runtime per process)
    import area_average_interpolation_amd as aai
    from oracle import pyoracle as po
    from conftest import TOL
    assert os.environ.get("AAI_MAX_LISTED_PIXELS") == "10"
    aai.set_device(0)
    z, m = manifest()
    for item in DENSE_ITEMS:
        mode, T, C = item
        hi = TYPES[T][3]
        for i in DENSE_POOL[mode]:
            g = _manifest_geometry(m, i, "dense")
            what = (item, i)
            rq = make_request(aai, g, mode)
            srcs = [source(po, g, T, C, b) for b in range(2)]
            golds = [oracle_gold(po, mode, g, s) for s in srcs]
            single = run_host(aai, g, mode, 0, srcs[0])
            name = aai.last_kernel()
            assert "strict" in name and ("fast" in name) == (mode == "fast"), (what, name)
            flagged, dense = plan_flags(aai, rq, C)
            assert dense == 1 and flagged == 0, (what, flagged, dense)                # (a dense plan keeps no list and counts none)
            check_against(single, golds[0], hi, TOL, what + ("single",))
            if T == "f32":
                ch = GOLDEN_CHANNEL[C]
                check_against(single if C == 1 else single[:, :, ch], reference_golden(z, mode, g), 1.0, TOL, what + ("reference golden",))
            outs = run_device(aai, rq, srcs, T, C)
            assert "strict" in aai.last_kernel(), (what, aai.last_kernel())
            for b in range(2):
                got = outs[b, :, :, 0] if C == 1 else outs[b]
                check_against(got, golds[b], hi, TOL, what + ("batch", b))
            assert np.array_equal(outs[0, :, :, 0] if C == 1 else outs[0], single), what
            if T == "f32" and C == 1:
                dH, dW = single.shape
                assert dH > 16, what
                band = run_band(aai, rq, srcs[0], 16, dH, dW)
                assert "strict" in aai.last_kernel(), (what, aai.last_kernel())
                assert not (band == SENTINEL).any() and np.array_equal(band, single[16:]), what
                check_against(band, golds[0][16:], hi, TOL, what + ("band",))
            print("dense %s k%03d %s" % (item_id(item), i, name))
    print("dense ok")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dense_child()
