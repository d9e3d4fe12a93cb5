"""GPU (MI355X): the half, integer, convert and half-adjoint entries on wide-pitch views of one device arena -- the case table of
tests/wide_pitch_typed.py, whose reach, pitch classes and replays test_wide_pitch_typed_host.py checks on the CPU (the replays against
the oracle: this module needs bit comparisons only).

Per row: the TIGHT CONTROL -- the same call on buffers of their own with GUARD elements of padding per row, computed once per
configuration and shared: aai_last_kernel() is the row's name, the padding keeps its fill, on direct rows the plan reports flagged=0
dense=0 and the result has the CPU replay's bits -- and the WIDE CALL: the image on the wide side is a strided view into the arena, the
GUARD elements behind every row read are all ones (NaN for fp16 / bf16), every row written and the GUARD elements behind it start as a
byte pattern, the plan is dropped before the call.  Asserted: the kernel's name, every padding element behind a written row keeps the
pattern, and the image written equals the tight control bit for bit.  One exception to the last: a u8 / u16 forwarding row with a
wide source, whose inner fp32 entry reads the wide view itself -- at a general rotation with an fp32 window kernel whose bits follow
the view's regime (wide_pitch.bit_exact_family).  There the expected image is the route's contract computed on the same wide view,
int_cases.lib_quantize / convert_cases.apply of the fp32 entry's output, and the tight control is still compared wherever the inner
kernel's family is bit-exact and the same on both views (90 degrees, the samplers).  Batch rows: both images equal single tight calls.
Grid rows (65537 tiny images, which the engine serves in two rounds of launches): the batch equals the same batch on tight buffers,
whose images on both sides of the split equal single tight calls.  The module ends with the coverage assertion.  Nothing here reads the reference tree.
"""
import numpy as np
import pytest

import convert_cases as cc
import int_cases as ic
import wide_pitch as wp
import wide_pitch_typed as wt
from test_wide_pitch_gpu import Arenas

pytestmark = pytest.mark.gpu

POISON = 0xFF                # every byte of the GUARD elements behind a row that is read
RAN = {}                     # row index -> the kernel name the row ran under


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
def ctx(gpu):
    c = type("Ctx", (), {})()
    c.gpu, c.rows = gpu, wt.rows(gpu)
    c.arenas = Arenas(wt.arena_bytes(gpu, "src"), wt.arena_bytes(gpu, "dst"))
    c.controls = {}
    yield c
    c.arenas.free()
    gpu.shutdown()


# ---- images in byte buffers ---------------------------------------------------------------------------------------------------------
def _views(buf, p):
    """every image and plane of a wide_pitch_typed.Placement in the device byte buffer `buf`: ([images, planes, rows, row bytes] view,
    [images, planes, rows, GUARD bytes] view of the elements behind every row)"""
    import torch
    esz = wt.ESZ[p.T]
    assert wt.extent_bytes(p) <= buf.numel(), (p, buf.numel())
    strides = (p.image * esz, p.plane * esz, p.pitch * esz, 1)
    return (torch.as_strided(buf, (p.images, p.planes, p.rows, p.row * esz), strides, 0),
            torch.as_strided(buf, (p.images, p.planes, p.rows, wp.GUARD * esz), strides, p.row * esz))


def _buffer(p, fill):
    import torch
    return torch.full((wt.extent_bytes(p),), fill, dtype=torch.uint8, device="cuda")


def _put(buf, p, imgs):
    """the images read ([images, rows, row] of raw elements), the GUARD elements behind every row poisoned"""
    import torch
    imgs = np.array(imgs)                                           # (a copy: the shared images are read-only)
    assert imgs.shape == (p.images, p.rows, p.row) and p.planes == 1, (imgs.shape, p)
    rows, guard = _views(buf, p)
    rows.copy_(torch.from_numpy(imgs.view(np.uint8).reshape(p.images, 1, p.rows, -1)).cuda())
    guard.fill_(POISON)


def _prefill(buf, p):
    for v in _views(buf, p):
        v.fill_(wt.PATTERN)


def _fetch(buf, p, what):
    """the images written, [images, planes x rows, row] of raw elements; every padding element behind their rows must hold the pattern"""
    rows, guard = _views(buf, p)
    clean = (guard == wt.PATTERN).flatten(1).all(dim=1).cpu().numpy()
    assert clean.all(), (what, "padding written behind a row of image(s)", np.flatnonzero(~clean)[:4].tolist())
    return np.ascontiguousarray(rows.cpu().numpy()).view(wt.NP[p.T]).reshape(p.images, p.planes * p.rows, p.row)


# ---- the call -------------------------------------------------------------------------------------------------------------------------
def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _guarded(what, fn):
    """fn(), then a synchronisation; a device error ends the session: nothing more may be started on this GPU by this process"""
    import torch
    from area_average_interpolation_amd import _lib as L
    from area_average_interpolation_amd.api import AaiError
    try:
        fn()
        torch.cuda.synchronize()
    except RuntimeError as e:
        if isinstance(e, AaiError) and e.code != L.ERR_HIP:
            raise
        pytest.exit("device error in %s: %s" % (what, e), returncode=3)


def _call(gpu, c, rd, rptr, wr, wptr, what):
    """c's entry on the image(s) read at rptr (Placement rd) and written at wptr (Placement wr), the plan built for this call; returns
    aai_last_kernel()"""
    assert rd.images == wr.images
    rq = wt.request(gpu, c)
    kw = dict(stream=_stream(), batch=rd.images)
    fwd = dict(src_image_stride=rd.image, dst_image_stride=wr.image)
    gpu.shutdown()                                                  # (the plan of THIS view: its form follows the pitch)
    if c.entry == "half":
        fn = lambda: gpu.resample_half_device(rq, rptr, rd.pitch, wptr, wr.pitch, wt.HT[c.T], **fwd, **kw)
    elif c.entry == "half-il":
        fn = lambda: gpu.resample_half_interleaved_device(rq, c.C, rptr, rd.pitch, wptr, wr.pitch, wt.HT[c.T], **fwd, **kw)
    elif c.entry == "int":
        fn = lambda: gpu.resample_int_device(rq, c.C, rptr, rd.pitch, wptr, wr.pitch, wt.DT[c.T], **fwd, **kw)
    elif c.entry == "convert":
        scale, offset = wt.conversion(c)
        cv = gpu.make_convert(c.C, wt.OT[c.out], wt.planar(c), scale[:c.C], offset[:c.C])
        fn = lambda: gpu.resample_convert_device(rq, c.C, rptr, rd.pitch, wptr, wr.pitch, wt.DT[c.T], cv, dst_plane_stride=wr.plane if wt.planar(c) else 0, **fwd, **kw)
    else:
        fn = lambda: gpu.adjoint_half_device(rq, c.C, rptr, rd.pitch, wptr, wr.pitch, wt.HT[c.T], dst_image_stride=rd.image, src_image_stride=wr.image, **kw)
    _guarded(what, fn)
    return gpu.last_kernel()


def _tight(ctx, c, imgs, what):
    """c's entry on tight buffers of their own -- rows + GUARD elements, images back to back -- for the images read `imgs` [n, rows, row]:
    (the images written [n, planes x rows, row], the kernel's name)"""
    gpu = ctx.gpu
    im = wt.images(gpu, c)
    rd, wr = wt.tight_placement(im, True, len(imgs)), wt.tight_placement(im, False, len(imgs))
    rbuf, wbuf = _buffer(rd, POISON), _buffer(wr, wt.PATTERN)
    _put(rbuf, rd, imgs)
    kernel = _call(gpu, c, rd, rbuf.data_ptr(), wr, wbuf.data_ptr(), what)
    direct = wt.is_direct(gpu, c)
    assert wt.name_matches(wt.direct_name(c) if direct else wt.SUFFIX[c.entry], kernel), (what, kernel)
    return _fetch(wbuf, wr, what), kernel


def _control(ctx, c, seed=0):
    """(the image written, the kernel's name) of c's entry on tight buffers: computed once, shared, never written to"""
    key = (c, seed)
    if key not in ctx.controls:
        gpu = ctx.gpu
        what = "%s-tight%s" % (wt.config_id(c), "-seed%d" % seed if seed else "")
        img = wt.read_image(gpu, c, seed)
        (got,), kernel = _tight(ctx, c, img[None], what)
        if wt.is_direct(gpu, c):
            # (the half adjoint runs on the forward's single-channel plan)
            shape = gpu.plan_shape(wt.request(gpu, c), 1 if c.entry == "adjoint" else c.C)
            assert "flagged=0 dense=0" in shape, (what, shape)
            want = wt.replay(gpu, c, img)
            assert wt.same_bits(got, want), (what, kernel, "differs from the CPU replay", int((got != want).sum()))
        got.setflags(write=False)
        ctx.controls[key] = (got, kernel)
    return ctx.controls[key]


def _contract(ctx, c, rd, rptr, inner, what):
    """The forwarding route's documented contract on the view the row reads: the fp32 entry on that view (the kernel must be the one the
    route ran), then the conversion on the CPU -- int_cases.lib_quantize / convert_cases.apply.  One image per image of the batch."""
    import torch
    gpu = ctx.gpu
    rq = wt.request(gpu, c)
    lay = gpu.query(rq)[2]
    dH, dW = lay.dst_height, lay.dst_width
    y = torch.full((rd.images, dH, dW, c.C), float("nan"), dtype=torch.float32, device="cuda")
    gpu.shutdown()
    _guarded(what + " (fp32 entry)", lambda: gpu.resample_interleaved_device(rq, c.C, rptr, rd.pitch, y.data_ptr(), dW * c.C, _stream(), batch=rd.images,
                                                                             src_image_stride=rd.image, dst_image_stride=dH * dW * c.C, src_dtype=wt.DT[c.T]))
    assert gpu.last_kernel() == inner, (what, gpu.last_kernel(), inner)
    f32 = y.cpu().numpy()
    im = wt.images(gpu, c)
    outs = []
    for b in range(rd.images):
        if c.entry == "int":
            out = ic.lib_quantize(f32[b], wt.DT[c.T])
        else:
            scale, offset = wt.conversion(c)
            out = cc.apply(f32[b], scale, offset, wt.OT[c.out], wt.LAY[c.layout])
        outs.append(np.ascontiguousarray(out).reshape(im.planes * im.wH, im.wrow))
    return np.stack(outs)


def _differing(got, want):
    """(images that differ, elements that differ) of two [images, rows, row] arrays"""
    d = got != want
    return np.flatnonzero(d.any(axis=(1, 2)))[:4].tolist(), int(d.sum())


def _run(ctx, r):
    gpu, c = ctx.gpu, r.config
    what = wt.row_id(r)
    im = wt.images(gpu, c)
    p = wt.placement(im, r)
    if r.side.startswith("grid"):
        # a batch beyond one round of launches: the control is the same batch on tight buffers, and the images on both sides of the
        # split -- the last two are the second round's -- equal single tight calls (direct rows: the CPU replay too)
        imgs = wt.read_images(gpu, c, p.images)
        key = (c, "grid")
        if key not in ctx.controls:
            outs, k = _tight(ctx, c, imgs, what + "-tight")
            for b in (0, 65534, 65535, p.images - 1):
                (one,), k1 = _tight(ctx, c, imgs[b:b + 1], what + "-tight-single")
                assert k1 == k and wt.same_bits(outs[b], one), (what, b, "the tight batch differs from the single call")
                if r.direct:
                    assert wt.same_bits(one, wt.replay(gpu, c, imgs[b])), (what, b, "differs from the CPU replay")
            ctx.controls[key] = (outs, k)
        want, names = ctx.controls[key][0], [ctx.controls[key][1]]
    else:
        seeds = (0, 1) if r.side.startswith("batch") else (0,)
        controls = [_control(ctx, c, s) for s in seeds]
        want, names = np.stack([got for (got, _) in controls]), [k for (_, k) in controls]
        imgs = np.stack([wt.read_image(gpu, c, s) for s in seeds])
    assert p.images == len(imgs)
    read_wide = r.side.endswith("src")
    if read_wide:
        rd, wr = p, wt.tight_placement(im, False, p.images)
        rbuf, wbuf = ctx.arenas.get("src").buf, _buffer(wr, wt.PATTERN)
    else:
        rd, wr = wt.tight_placement(im, True, p.images), p
        rbuf, wbuf = _buffer(rd, POISON), ctx.arenas.get("dst").buf
        _prefill(wbuf, wr)
    _put(rbuf, rd, imgs)
    assert wt.extent_bytes(rd) <= rbuf.numel() and wt.extent_bytes(wr) <= wbuf.numel(), (what, rd, wr)      # (what the call is entitled to lies inside the buffers)
    kernel = _call(gpu, c, rd, rbuf.data_ptr(), wr, wbuf.data_ptr(), what)
    assert wt.name_matches(r.kernel, kernel), (what, kernel, r.kernel)
    outs = _fetch(wbuf, wr, what)
    suffix = wt.SUFFIX[c.entry]
    if not r.direct and c.entry in ("int", "convert") and read_wide:
        # the inner fp32 entry read the wide view itself
        inner = kernel[:-len(suffix)]
        family = wp.family_of(inner)
        contract = _contract(ctx, c, rd, rbuf.data_ptr(), inner, what)
        assert wt.same_bits(outs, contract), (what, kernel, "differs from the converted fp32 entry", _differing(outs, contract))
        exact = wp.bit_exact_family(family) and all(wp.family_of(k[:-len(suffix)]) == family for k in names)
        note = "the tight control's bits too" if exact else "its family's bits follow the view: the contract on the wide view only"
    else:
        assert all(k == kernel for k in names), (what, kernel, names)
        exact, note = True, ""
    if exact:
        assert wt.same_bits(outs, want), (what, kernel, "differs from the tight control", _differing(outs, want))
    print("%-64s %-44s pitch %9d apart %11d %s" % (what, kernel, p.pitch, r.apart, note))
    RAN[r.index] = kernel


# ---- the rows, grouped by entry and side ----------------------------------------------------------------------------------------------
SIDES = ("src", "dst", "plane", "batch-src", "batch-dst", "grid-src", "grid-dst")
_HAVE = {(c.entry, side) for c, pairs in wt.CONFIGS for side, _ in pairs} | {(c.entry, side) for c, sides in wt.BATCHES + wt.GRIDS for side in sides}
GROUPS = [(e, s) for e in wt.ENTRIES for s in SIDES if (e, s) in _HAVE]


@pytest.mark.parametrize("entry,side", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_typed_entries_on_wide_views(ctx, entry, side):
    """All rows of one entry with the image on one side wide (see the module's text)."""
    mine = [r for r in ctx.rows if r.config.entry == entry and r.side == side]
    assert mine, (entry, side)
    for r in mine:
        _run(ctx, r)
    print("%s %s: %d rows" % (entry, side, len(mine)))


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_row_of_the_table_ran_under_its_expected_name(ctx):
    """(Last in the module.)  Every row ran, under the kernel name it records -- _run asserted the name row by row; this is the
    bookkeeping that no row was left out -- and the count per (entry, route, side, class)."""
    missing = [wt.row_id(r) for r in ctx.rows if r.index not in RAN or not wt.name_matches(r.kernel, RAN[r.index])]
    assert not missing, missing
    count = {}
    for r in ctx.rows:
        k = (r.config.entry, "direct" if r.direct else "forwarding", r.side, r.cls)
        count[k] = count.get(k, 0) + 1
    for k in sorted(count):
        print("%-8s %-10s %-9s %-3s %3d rows" % (k + (count[k],)))
    assert all(count.values()) and sum(count.values()) == len(ctx.rows)
