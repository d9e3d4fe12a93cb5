"""GPU (MI355X): every kernel family at the row pitches where its hand-written offset arithmetic changes regime -- small images in
wide-pitch views of one device arena (the case table of tests/wide_pitch.py; test_wide_pitch_host.py checks the table itself and the
oracle's sensitivity to one misaddressed row on the CPU).

Per forward case: the oracle's bar (conftest.TOL relative with the floor of 1e-3 x the value scale; the samplers 2e-5 x the value
scale absolute), no pixel excepted, exact zeros exact, no NaN (the 64 elements behind every source row are NaN / all ones), the dst
padding keeps its sentinel, aai_last_kernel() is the family the probe names, and the result equals the tight control's bit for bit
where the family's arithmetic does not depend on the view (K1, the samplers, the double-precision kernels, every pixel of the fix-up
pass); for the fp32 window kernels the largest difference from the control is printed.  The module ends with the coverage assertion:
every (family, regime) pair of the table ran under the kernel name it expected.  Nothing here reads the reference tree.
"""
import re

import numpy as np
import pytest

import wide_pitch as wp
from conftest import TOL

pytestmark = pytest.mark.gpu

DIAG_NO_FIXUP = 0x400
RAN = {}                     # (family, regime, X?) -> ids of the cases that ran under that kernel name
WORST = {}                   # family -> worst scaled error (in units of its bar's reference)


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


class Arenas:
    """the source arena and the destination arena, each allocated at the size its cases need when first asked for; asking for one frees
    the other where both together would pass wp.ARENA_CAP_BOTH"""

    def __init__(self, src_bytes, dst_bytes):
        self.want = {"src": src_bytes, "dst": dst_bytes}
        self.have = {"src": None, "dst": None}

    def get(self, which):
        other = "dst" if which == "src" else "src"
        if self.have[which] is None:
            if self.have[other] is not None and self.have[other].nbytes + self.want[which] > wp.ARENA_CAP_BOTH:
                self.have[other].free()
                self.have[other] = None
            self.have[which] = wp.Arena(self.want[which])
        return self.have[which]

    def free(self):
        for k, a in self.have.items():
            if a is not None:
                a.free()
                self.have[k] = None


@pytest.fixture(scope="module")
def ctx(gpu, hostemu, po):
    probe, fwd, bnd = wp.table(hostemu)
    c = type("Ctx", (), {})()
    c.gpu, c.po, c.probe, c.fwd, c.bnd = gpu, po, probe, fwd, bnd
    c.arenas = Arenas(wp.source_arena_bytes(hostemu), wp.dst_arena_bytes(hostemu))
    c.golds, c.controls = {}, {}
    yield c
    c.arenas.free()
    gpu.shutdown()


def _gold(ctx, g, T, H, seed=0):
    """(source, oracle gold) of (geometry, type, height): computed once, shared, never written to"""
    key = (g.name, T, H, seed)
    if key not in ctx.golds:
        src = wp.source(g, T, H, seed)
        gold = wp.gold(ctx.po, g, H, src)
        src.setflags(write=False)
        gold.setflags(write=False)
        ctx.golds[key] = (src, gold)
    return ctx.golds[key]


def _shape(g, gold):
    dH, dW = gold.shape[0], gold.shape[1]
    return dH, dW, dW * g.C


def _holes(ctx, g, T, H, src_ptr, src_pitch, shape, got, family, flagged):
    """The dst pixels the fix-up pass wrote: with the pass switched off (AAI_POLICY_DIAG_NO_FIXUP) the fp32 kernels of the rotated
    lattice leave exactly the plan's `flagged` pixels to the sentinel.  K1 writes every pixel itself and the pass overwrites the listed
    ones, mostly with the same float: no mask there (None) -- K1's cases are bit-identical to their control in EVERY pixel."""
    dH, dW, drow = shape
    t, dp, _ = wp.tight_dst(dH, drow)
    wp.resample(g, T, H, src_ptr, src_pitch, t.data_ptr(), dp, extra_policy=DIAG_NO_FIXUP)
    without = t[0, :, :drow].cpu().numpy().reshape(gold_shape(g, dH, dW))
    if family.startswith("aai_axis"):
        return None
    holes = without == wp.SENTINEL
    assert int(holes.sum()) == flagged * g.C, (g.name, T, H, int(holes.sum()), flagged)
    return holes


def gold_shape(g, dH, dW):
    return (dH, dW) if g.C == 1 else (dH, dW, g.C)


def _flagged(ctx, g, H):
    m = re.search(r"flagged=(\d+) dense=(\d+)", ctx.gpu.plan_shape(wp.make_request(g, H), channels=g.C))
    assert m, (g.name, H)
    return int(m.group(1)), int(m.group(2))


def _check(case_name, g, T, got, gold, kernel, family):
    """the bar, exact zeros, no NaN, the family; returns the worst scaled error"""
    assert got.dtype == np.float32 and got.shape == gold.shape, (case_name, got.shape, gold.shape)
    assert not np.isnan(got).any(), (case_name, kernel, int(np.isnan(got).sum()))
    err = float(wp.scaled_error(g, T, got, gold).max())
    bound = TOL if wp.bar(g, T)[0] else wp.bar(g, T)[1]
    print("%-62s %-40s err %.2e (bar %.0e)" % (case_name, kernel, err, bound))
    assert wp.family_of(kernel) == family, (case_name, kernel, family)
    assert err <= bound, (case_name, kernel, err)
    assert np.array_equal(gold == 0, got == 0), (case_name, kernel)
    WORST[family] = max(WORST.get(family, 0.0), err / bound)
    return err


def _control(ctx, g, T, H):
    """the same call on tight buffers (regime T): (result, family, holes or None); held to the bar like every case"""
    import torch
    key = (g.name, T, H)
    if key not in ctx.controls:
        src, gold = _gold(ctx, g, T, H)
        shape = _shape(g, gold)
        ctx.gpu.shutdown()
        s = wp.to_device(src, T)
        t, dp, _ = wp.tight_dst(shape[0], shape[2])
        kernel = wp.resample(g, T, H, s.data_ptr(), wp.row_elems(g), t.data_ptr(), dp)
        host = t[0].cpu().numpy()
        assert (host[:, shape[2]:] == wp.SENTINEL).all(), (g.name, T, H, "control: dst padding written")
        got = host[:, :shape[2]].reshape(gold.shape)
        family = ctx.probe.family(g, H, T, wp.row_elems(g))
        _check("%s-%s-H%d-T" % (g.name, T, H), g, T, got, gold, kernel, family)
        holes = None
        if g.knife:
            flagged, dense = _flagged(ctx, g, H)
            assert flagged > 0 and dense == 0, (g.name, T, H, flagged, dense)
            holes = _holes(ctx, g, T, H, s.data_ptr(), wp.row_elems(g), shape, got, family, flagged)
        RAN.setdefault((family, "T", False), set()).add(key)
        ctx.controls[key] = (got, family, holes)
    return ctx.controls[key]


def _forward(ctx, case):
    g, T, H = case.geom, case.T, case.H
    name = wp.case_id(case)
    src, gold = _gold(ctx, g, T, H)
    shape = _shape(g, gold)
    ctl, ctl_family, ctl_holes = _control(ctx, g, T, H)
    assert ctl_family == case.control, (name, ctl_family, case.control)
    arena = ctx.arenas.get("src")
    ptr = wp.place_source(arena, src, T, case.pitch)
    ctx.gpu.shutdown()                                             # (the plan of THIS view: its form follows the pitch)
    t, dp, _ = wp.tight_dst(shape[0], shape[2])
    kernel = wp.resample(g, T, H, ptr, case.pitch, t.data_ptr(), dp)
    host = t[0].cpu().numpy()
    assert (host[:, shape[2]:] == wp.SENTINEL).all(), (name, kernel, "dst padding written")
    got = host[:, :shape[2]].reshape(gold.shape)
    _check(name, g, T, got, gold, kernel, case.family)
    differ = float(np.abs(got.astype(np.float64) - ctl).max()) / wp.TYPES[T][3]
    if wp.bit_exact_family(case.family) and case.family == ctl_family:
        assert np.array_equal(got, ctl), (name, kernel, "differs from the tight control", differ)
    else:
        print("%-62s largest difference from the tight control: %.2e of the value scale" % (name, differ))
    if g.knife:
        flagged, dense = _flagged(ctx, g, H)
        assert flagged > 0 and dense == 0, (name, flagged, dense)
        holes = _holes(ctx, g, T, H, ptr, case.pitch, shape, got, case.family, flagged)
        # every pixel the fix-up pass wrote here AND in the control: the same double-precision arithmetic, the same bits
        if holes is not None and ctl_holes is not None:
            both = holes & ctl_holes
            assert both.any() and np.array_equal(got[both], ctl[both]), (name, kernel, int(both.sum()))
            if case.family == ctl_family:
                assert np.array_equal(holes, ctl_holes), (name, "the same family flags other pixels at this pitch")
        else:
            assert wp.bit_exact_family(case.family) and case.family == ctl_family, (name, case.family, ctl_family)
    RAN.setdefault((case.family, case.regime, case.x), set()).add(name)


def _base(g):
    return g.name.split("/")[0]


BASES = []
for _geom in wp.GEOMS + wp.BOUND_GEOMS:
    if _base(_geom) not in BASES:
        BASES.append(_base(_geom))


@pytest.mark.parametrize("base", BASES)
def test_forward_at_every_regime_of_the_source_pitch(ctx, base):
    """All forward cases (source view wide) and boundary pairs of one geometry family, both quadrant parities."""
    mine = [c for c in ctx.fwd if _base(c.geom) == base] + [c for (_, a, b) in ctx.bnd for c in (a, b) if _base(c.geom) == base]
    assert mine
    for case in mine:
        _forward(ctx, case)
    print("%s: %d cases" % (base, len(mine)))


# ---- destinations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,cls", wp.DST_CASES, ids=["%s-%s-dst%s" % c for c in wp.DST_CASES])
def test_destination_views_of_4_gib_and_of_2_31_elements(ctx, name, T, cls):
    """The tight source into a dst view whose rows lie so far apart that it spans 4 GiB (G) or 2^31 elements (E31): bit-identical to
    the control (the same kernel, the same source view: only the store addresses differ), padding untouched."""
    g = wp.geom_by_name(name)
    H = g.heights[0]
    src, gold = _gold(ctx, g, T, H)
    dH, dW, drow = _shape(g, gold)
    ctl, family, ctl_holes = _control(ctx, g, T, H)
    pitch = wp.dst_pitch_for(cls, dH)
    assert dH * pitch * 4 >= 1 << 32 and (cls != "E31" or dH * pitch >= 1 << 31)
    arena = ctx.arenas.get("dst")
    dptr, rows, guard = wp.place_dst(arena, dH, drow, pitch)
    s = wp.to_device(src, T)
    ctx.gpu.shutdown()
    kernel = wp.resample(g, T, H, s.data_ptr(), wp.row_elems(g), dptr, pitch)
    got = rows.cpu().numpy().reshape(gold.shape)
    what = "%s-%s-H%d-dst%s" % (name, T, H, cls)
    assert bool((guard == wp.SENTINEL).all().item()), (what, kernel, "dst padding written")
    _check(what, g, T, got, gold, kernel, family)
    assert np.array_equal(got, ctl), (what, kernel, "differs from the tight control")
    if g.knife:
        assert ctl_holes is None or ctl_holes.any()                    # (the fix-up pass wrote into the wide dst view)
    if g.name.startswith("k1-empty"):
        assert (gold == 0).all(axis=1).any()                           # (a whole dst row off the image: launch_axis_zero's)
    RAN.setdefault((family, "dst" + cls, False), set()).add(what)


# ---- batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", wp.BATCH_CASES, ids=["%s-%s" % c for c in wp.BATCH_CASES])
@pytest.mark.parametrize("side", ["src", "dst"])
def test_batches_whose_images_lie_2_31_elements_apart(ctx, side, name, T):
    """A batch of two with tight rows, the second image 2^31 elements and more behind the first (u8 sources: 2^32), on the source side
    and, separately, on the dst side: both images at the bar and bit-identical to single calls on tight buffers."""
    import torch
    g = wp.geom_by_name(name)
    H = g.heights[0]
    pairs = [_gold(ctx, g, T, H, seed) for seed in (0, 1)]
    dH, dW, drow = _shape(g, pairs[0][1])
    row = wp.row_elems(g)
    apart = wp.batch_apart(T, side)
    ctx.gpu.shutdown()
    family = ctx.probe.family(g, H, T, row)
    singles = []
    for src, gold in pairs:
        s = wp.to_device(src, T)
        t, dp, _ = wp.tight_dst(dH, drow)
        wp.resample(g, T, H, s.data_ptr(), row, t.data_ptr(), dp)
        singles.append(t[0, :, :drow].cpu().numpy().reshape(gold.shape))
    if side == "src":
        arena = ctx.arenas.get("src")
        for b, (src, _) in enumerate(pairs):
            ptr = wp.place_source(arena, src, T, row + wp.GUARD, offset=b * apart)
            base = ptr if b == 0 else base
        t, dp, di = wp.tight_dst(dH, drow, batch=2)
        kernel = wp.resample(g, T, H, base, row + wp.GUARD, t.data_ptr(), dp, batch=2, src_image=apart, dst_image=di)
        outs = [t[b, :, :drow].cpu().numpy() for b in range(2)]
        assert bool((t[:, :, drow:] == wp.SENTINEL).all().item())
    else:
        arena = ctx.arenas.get("dst")
        views = [wp.place_dst(arena, dH, drow, drow + wp.GUARD, offset=b * apart) for b in range(2)]
        s = torch.stack([wp.to_device(src, T) for src, _ in pairs])
        kernel = wp.resample(g, T, H, s.data_ptr(), row, views[0][0], drow + wp.GUARD, batch=2, src_image=H * row, dst_image=apart)
        outs = [v[1].cpu().numpy() for v in views]
        assert all(bool((v[2] == wp.SENTINEL).all().item()) for v in views)
    for b in range(2):
        what = "%s-%s-batch-%s-image%d" % (name, T, side, b)
        got = outs[b].reshape(pairs[b][1].shape)
        _check(what, g, T, got, pairs[b][1], kernel, family)
        assert np.array_equal(got, singles[b]), (what, kernel, "differs from the single call")
    RAN.setdefault((family, "batch-" + side, False), set()).add(name)


# ---- the adjoints and the reference-precision path -----------------------------------------------------------------------------------
# (id, api function, its extra keywords, element type, mode, src : dst, angle, W, C): one geometry each
ADJOINTS = [
    ("general", "adjoint_device", dict(planned=False), "f32", 1, 3.0, 17.5, 100, 1),
    ("general-rgb", "adjoint_interleaved_device", dict(planned=False), "f32", 1, 3.0, 107.5, 40, 3),
    ("general-fast", "adjoint_device", dict(planned=False), "f32", 2, 3.0, 197.5, 100, 1),
    ("planned-0", "adjoint_device", dict(planned=True), "f32", 1, 2.0, 0.0, 100, 1),
    ("planned-90", "adjoint_device", dict(planned=True), "f32", 1, 2.0, 90.0, 100, 1),
    ("planned-0-channels-last", "adjoint_interleaved_device", dict(planned="separable"), "f32", 1, 2.0, 0.0, 40, 3),
    ("planned-90-channels-last", "adjoint_interleaved_device", dict(planned="separable"), "f32", 1, 2.0, 90.0, 40, 3),
    ("rotated-plain", "adjoint_device", dict(planned="any"), "f32", 1, 3.0, 17.5, 100, 1),
    ("rotated-plain-rgb", "adjoint_interleaved_device", dict(planned="any"), "f32", 1, 3.0, 287.5, 40, 3),
    ("sample-bilinear", "adjoint_sample_device", {}, "f32", 3, 2.0, 17.5, 100, 1),
    ("sample-bicubic", "adjoint_sample_device", {}, "f32", 4, 2.0, 107.5, 100, 1),
    ("sample-bilinear-rgb", "adjoint_sample_interleaved_device", {}, "f32", 3, 2.0, 17.5, 40, 3),
    ("f64-adjoint", "adjoint_device_f64", {}, "f64", 1, 3.0, 17.5, 100, 1),
    ("f64-adjoint-fast", "adjoint_device_f64", {}, "f64", 2, 3.0, 107.5, 100, 1),
    ("f64-forward", "resample_device_f64", {}, "f64", 1, 3.0, 17.5, 100, 1),
    ("f64-forward-90", "resample_device_f64", {}, "f64", 2, 3.0, 107.5, 100, 1),
]
ADJ_H = 560


@pytest.mark.parametrize("entry", ADJOINTS, ids=[e[0] for e in ADJOINTS])
def test_adjoints_and_f64_entries_on_wide_views(ctx, entry):
    """Every adjoint entry and the two double-precision entries, the source-side image wide (4 GiB of span below a pitch of 8 MiB, and
    above it) and, separately, the dst-side image wide: bit-identical to the same entry on tight buffers (the adjoint modules and
    test_f64_gpu.py hold those to the oracle).  What is read has NaN behind every row, what is written the sentinel, which it keeps.
    Doubles span 4 GiB at 2^29 elements."""
    import torch
    name, fn_name, kw, T, mode, ratio, angle, W, C = entry
    gpu = ctx.gpu
    fn = getattr(gpu, fn_name)
    forward = fn_name.startswith("resample")
    H, esz = ADJ_H, wp.ESZ[T]
    tdt = torch.float64 if T == "f64" else torch.float32
    rq = gpu.make_request(W, H, ratio, 1.0, ((W - 1) / 2.0 + wp.OFF[0], (H - 1) / 2.0 + wp.OFF[1]), angle, mode=mode)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    dH, drow, srow = lay.dst_height, lay.dst_width * C, W * C
    rng = np.random.default_rng(99)
    # the image the entry READS (the forward: the source; an adjoint: gdst) and the shape of the one it WRITES
    rH, rrow, wH, wrow = (H, srow, dH, drow) if forward else (dH, drow, H, srow)
    data = torch.from_numpy(rng.random((rH, rrow)) + 0.25).to(tdt).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def call(read_ptr, read_pitch, write_ptr, write_pitch):
        gpu.shutdown()
        args = (rq,) + ((C,) if "interleaved" in fn_name else ()) + (read_ptr, read_pitch, write_ptr, write_pitch, st)
        try:
            fn(*args, batch=1, **kw)
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit("device error in %s: %s" % (name, e), returncode=3)
        return gpu.last_kernel()

    tight = torch.full((wH, wrow + wp.GUARD), wp.SENTINEL, dtype=tdt, device="cuda")
    kernel = call(data.data_ptr(), rrow, tight.data_ptr(), wrow + wp.GUARD)
    assert bool((tight[:, wrow:] == wp.SENTINEL).all().item()) and not bool(torch.isnan(tight).any().item()), (name, kernel)
    want = tight[:, :wrow].cpu().numpy()
    assert np.abs(want).max() > 0
    # (side, pitch class): the source-side image is the one written by an adjoint and read by the forward
    for side, cls in (("src", "G"), ("src", "GP"), ("dst", "G")):
        wide_is_read = (side == "src") == forward
        vH, vrow = (rH, rrow) if wide_is_read else (wH, wrow)
        pitch = wp.pitch_for(cls, vH, vrow, esz)
        assert vH * pitch * esz >= 1 << 32
        if cls == "GP" and vH * pitch * esz > wp.ARENA_CAP:
            continue
        arena = ctx.arenas.get(side)
        rows, guard = arena.view(T, vH, vrow, pitch)
        if wide_is_read:
            rows.copy_(data)
            guard.fill_(float("nan"))
            out = torch.full((wH, wrow + wp.GUARD), wp.SENTINEL, dtype=tdt, device="cuda")
            k = call(rows.data_ptr(), pitch, out.data_ptr(), wrow + wp.GUARD)
            got, pad = out[:, :wrow].cpu().numpy(), out[:, wrow:]
        else:
            rows.fill_(wp.SENTINEL)
            guard.fill_(wp.SENTINEL)
            k = call(data.data_ptr(), rrow, rows.data_ptr(), pitch)
            got, pad = rows.cpu().numpy(), guard
        what = "%s-%s-wide-%s" % (name, side, cls)
        print("%-44s %-44s pitch %d" % (what, k, pitch))
        assert k == kernel, (what, k, kernel)
        assert bool((pad == wp.SENTINEL).all().item()), (what, k, "padding written")
        assert np.array_equal(got, want), (what, k, float(np.nanmax(np.abs(got - want))), int(np.isnan(got).sum()))
        RAN.setdefault((name, side + "-" + cls, False), set()).add(what)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_family_ran_in_every_regime_of_the_table(ctx):
    """(Last in the module.)  Every (family, regime) pair the table holds ran, under the kernel name the probe expected -- _check
    asserted the name case by case; this is the bookkeeping that no pair was left out -- and every X case documents a takeover."""
    want = {}
    for c in ctx.fwd + [c for (_, a, b) in ctx.bnd for c in (a, b)]:
        want.setdefault((c.family, c.regime, c.x), set()).add(wp.case_id(c))
    missing = {k: sorted(v) for k, v in want.items() if RAN.get(k, set()) != v}
    assert not missing, missing
    for (family, regime, x) in sorted(want, key=str):
        print("%-28s %-3s %s %3d cases" % (family, regime, "X" if x else " ", len(want[(family, regime, x)])))
    for family in sorted(WORST):
        print("worst scaled error %-28s %.3f of its bar" % (family, WORST[family]))
