"""The guard-band harness (tests/guard_layout.py) must be able to fail -- no GPU needed.

A CPU stand-in for a device call -- the oracle on the entitled view of a guarded source, written into the entitled view of a guarded
destination -- passes the harness in every source type, channel count and base offset; four deliberately wrong variants of it, each
breaking one promise of include/aai.h the way a kernel plausibly would, are each reported, at the element they touched.  This is the
evidence that the assertions of tests/test_gpu_memory_contract.py are not vacuous."""
import numpy as np
import pytest

from guard_layout import ALIGN, DTYPES, SENTINEL_BITS, GuardedLayout, poisons

W, H, SR, DR = 22, 14, 2.0, 1.0
ISO = ((W - 1) / 2, (H - 1) / 2)


def _values(rng, dtype, shape):
    if dtype == "f32":
        return (rng.random(shape) + 0.25).astype(np.float32)
    return rng.integers(1, np.iinfo(DTYPES[dtype]).max, size=shape).astype(DTYPES[dtype])


def _oracle(po, img, ang):
    return po.oracle_run(po.MODE_EXACT, img.astype(np.float64), SR, DR, ISO, ang).dst.astype(np.float32)


def stand_in(po, ang, sl, src_buf, dl, dst_buf, band=None, wrong=None):
    """What a device call does, on the host: reads the entitled source elements only, writes the entitled dst elements only.
    band = (dst_row0, dst_row1, src_row0, src_row1): the source buffer holds rows [src_row0, src_row1) only.
    wrong: None, or the promise to break -- "row_end", "band_end", "next_image", "dst_overrun"."""
    src = sl.gather(src_buf)
    B, rows, _, C = sl.shape
    res = np.empty(dl.shape, dtype=np.float32)
    for b in range(B):
        for c in range(C):
            img = src[b, :, :, c]
            if band is not None:
                full = np.zeros((H, W), dtype=img.dtype)
                full[band[2]:band[3]] = img
                img = full
            out = _oracle(po, img, ang)
            res[b, :, :, c] = out if band is None else out[band[0]:band[1]]
    flat = np.asarray(src_buf).astype(np.float32)
    weight = np.float32(0.0 if sl.dtype == "f32" else 1.0)        # (0 x an integer poison is 0: only a weighted read of it shows)
    with np.errstate(invalid="ignore"):
        if wrong == "row_end":         # one vector load too far at the end of the last row of every image, weight 0
            for b in range(B):
                res[b, -1] += weight * flat[sl.lead + b * sl.image_stride + (rows - 1) * sl.stride + sl.row]
        elif wrong == "band_end":      # the row after the band's footprint
            res[:, -1] += weight * flat[sl.lead + rows * sl.stride]
        elif wrong == "next_image":    # image b looks at the first element of image b + 1
            for b in range(B):
                res[b, 0, 0, 0] += weight * flat[sl.lead + (b + 1) * sl.image_stride]
    dst = np.asarray(dst_buf).view(np.float32)
    dst[dl.index.reshape(-1)] = res.reshape(-1)
    if wrong == "dst_overrun":         # one element past the end of dst row 2, and one whole vector before dst row 0
        dst[dl.lead + 2 * dl.stride + dl.row] = 1.0
        dst[dl.lead - 4:dl.lead] = 2.0


def _layouts(dtype, B, C, rows, drows, dW, off, pad=3, gap=5):
    sl = GuardedLayout((B, rows, W, C), dtype, stride=W * C + pad, image_stride=rows * (W * C + pad) + gap, base_offset=off)
    dl = GuardedLayout((B, drows, dW, C), "f32", stride=dW * C + pad + 2, image_stride=drows * (dW * C + pad + 2) + gap + 2,
                       base_offset=(off + 1) % 4)
    return sl, dl


def _run(po, ang, sl, dl, band=None, wrong=None):
    def run(src_buf):
        dst_buf = dl.make_dst()
        stand_in(po, ang, sl, src_buf, dl, dst_buf, band, wrong)
        return dst_buf
    return run


def test_layout_geometry():
    for dtype in DTYPES:
        for off in range(4):
            lay = GuardedLayout((3, 5, 7, 3), dtype, stride=7 * 3 + 5, image_stride=5 * 26 + 3, base_offset=off)
            per = ALIGN // lay.np_dtype.itemsize
            assert (lay.lead - off) % per == 0 and lay.byte_offset() % ALIGN == off * lay.np_dtype.itemsize
            assert lay.margin == 8 * lay.stride + 1024 and lay.lead >= lay.margin and lay.total - lay.lead - lay.span >= lay.margin
            assert lay.region(0)[0] == "entitled" and lay.region(20) == ("entitled", 0, 0, 20) and lay.region(21) == ("pad", 0, 0, 21)
            assert lay.region(5 * 26) == ("gap", 0, 5, 0) and lay.region(5 * 26 + 3) == ("entitled", 1, 0, 0)
            assert lay.region(-1)[0] == "before" and lay.region(lay.span)[0] == "after" and lay.region(lay.span - 1)[0] == "entitled"
            masks = [lay.region_mask((name,)) for name in ("before", "pad", "gap", "after")]
            assert all(m.any() for m in masks) and int(sum(m.sum() for m in masks)) + int(lay.entitled.sum()) == lay.total
            for name, m in zip(("before", "pad", "gap", "after"), masks):
                k = int(np.flatnonzero(m)[len(np.flatnonzero(m)) // 2])
                assert lay.region(k - lay.lead)[0] == name
    with pytest.raises(AssertionError):
        GuardedLayout((1, 4, 8, 1), "f32", stride=7)
    with pytest.raises(AssertionError):
        GuardedLayout((2, 4, 8, 1), "f32", stride=9, image_stride=35)
    dst = GuardedLayout((1, 2, 3, 1), "f32").make_dst()
    assert np.isnan(dst).all() and (dst.view(np.int32) == SENTINEL_BITS).all()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_correct_stand_in_passes(po, dtype):
    rng = np.random.default_rng(7)
    for C in (1, 2, 3, 4):
        for off in range(4):
            ang = (0.0, 90.0, 180.0, 270.0)[off]
            dH, dW = _oracle(po, np.zeros((H, W)), ang).shape
            sl, dl = _layouts(dtype, 2, C, H, dH, dW, off)
            values = _values(rng, dtype, sl.shape)
            run = _run(po, ang, sl, dl)
            outs = []
            for poison in poisons(dtype):
                out, first, count = dl.check_dst(run(sl.make_src(values, poison)))
                assert count == 0 and first is None
                assert np.isfinite(out).all() and dl.sentinels_left(out) == 0
                outs.append(out)
            assert all(np.array_equal(o, outs[0]) for o in outs)
            for b in range(2):
                for c in range(C):
                    assert np.array_equal(outs[0][b, :, :, c], _oracle(po, values[b, :, :, c], ang))
            assert sl.locate_reads(lambda buf: dl.check_dst(run(buf))[0], values, poisons(dtype)[-1]) == []


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_a_read_past_the_last_row_end_is_reported(po, dtype):
    rng = np.random.default_rng(8)
    dH, dW = _oracle(po, np.zeros((H, W)), 0.0).shape
    for off in (0, 3):
        sl, dl = _layouts(dtype, 2, 2, H, dH, dW, off)
        values = _values(rng, dtype, sl.shape)
        run = _run(po, 0.0, sl, dl, wrong="row_end")
        outs = [dl.check_dst(run(sl.make_src(values, p)))[0] for p in poisons(dtype)]
        if dtype == "f32":
            bad = ~np.isfinite(outs[0])
        else:
            bad = outs[0] != outs[1]
        # the last dst row of every image, and nothing else
        assert bad[:, -1].all() and not bad[:, :-1].any()
        where = sl.locate_reads(lambda buf: dl.check_dst(run(buf))[0], values, poisons(dtype)[-1])
        assert where == [b * sl.image_stride + (H - 1) * sl.stride + sl.row for b in range(2)]
        # (row padding in image 0; behind the last row of the last image the trailing margin begins)
        assert [sl.region(o) for o in where] == [("pad", 0, H - 1, sl.row), ("after", 1, H - 1, sl.row)]
    # tight rows: the same read is the first element of the next row for every row but the very last, which reads the trailing margin
    sl = GuardedLayout((1, H, W, 1), dtype, base_offset=1)
    dl = GuardedLayout((1, dH, dW, 1), "f32")
    values = _values(rng, dtype, sl.shape)
    run = _run(po, 0.0, sl, dl, wrong="row_end")
    where = sl.locate_reads(lambda buf: dl.check_dst(run(buf))[0], values, poisons(dtype)[-1])
    assert where == [sl.span] and sl.region(where[0]) == ("after", 0, H, 0)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_a_read_of_the_row_after_a_band_footprint_is_reported(po, aai, dtype):
    rng = np.random.default_rng(9)
    ang = 0.0
    rq = aai.make_request(W, H, SR, DR, ISO, ang)
    dH, dW = _oracle(po, np.zeros((H, W)), ang).shape
    r0, r1 = 2, 5
    a, b = aai.band_source_rows(rq, r0, r1)
    assert 0 <= a < b < H                      # (a band in the middle: there IS a row after its footprint in the image)
    sl, dl = _layouts(dtype, 1, 1, b - a, r1 - r0, dW, 2)
    image = _values(rng, dtype, (1, H, W, 1))
    values = image[:, a:b]
    band = (r0, r1, a, b)
    # the correct stand-in computes the band from its footprint alone, whatever lies around it
    gold = _oracle(po, image[0, :, :, 0], ang)[r0:r1]
    for poison in poisons(dtype):
        out, first, count = dl.check_dst(_run(po, ang, sl, dl, band)(sl.make_src(values, poison)))
        assert count == 0 and np.array_equal(out[0, :, :, 0], gold)
    run = _run(po, ang, sl, dl, band, wrong="band_end")
    outs = [dl.check_dst(run(sl.make_src(values, p)))[0] for p in poisons(dtype)]
    bad = ~np.isfinite(outs[0]) if dtype == "f32" else outs[0] != outs[1]
    assert bad[:, -1].all() and not bad[:, :-1].any()
    where = sl.locate_reads(lambda buf: dl.check_dst(run(buf))[0], values, poisons(dtype)[-1])
    assert where == [(b - a) * sl.stride] and sl.region(where[0]) == ("after", 0, b - a, 0)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_a_read_of_the_next_batch_image_is_reported(po, dtype):
    rng = np.random.default_rng(10)
    dH, dW = _oracle(po, np.zeros((H, W)), 0.0).shape
    B = 3
    sl, dl = _layouts(dtype, B, 1, H, dH, dW, 1)
    values = _values(rng, dtype, sl.shape)
    run = _run(po, 0.0, sl, dl, wrong="next_image")
    outs = [dl.check_dst(run(sl.make_src(values, p)))[0] for p in poisons(dtype)]
    bad = ~np.isfinite(outs[0]) if dtype == "f32" else outs[0] != outs[1]
    # images 0 and 1 read live pixels of their neighbours (for 8- / 16-bit pixels that shows against the oracle only); the last image
    # of the batch reads where image B would start: poison
    assert np.argwhere(bad).tolist() == [[B - 1, 0, 0, 0]]
    where = sl.locate_reads(lambda buf: dl.check_dst(run(buf))[0], values, poisons(dtype)[-1])
    assert where == [B * sl.image_stride] and sl.region(where[0])[:2] == ("after", B - 1)
    if dtype != "f32":
        assert not np.array_equal(outs[0][0, :, :, 0], _oracle(po, values[0, :, :, 0], 0.0))


def test_writes_outside_the_output_are_reported(po):
    rng = np.random.default_rng(11)
    dH, dW = _oracle(po, np.zeros((H, W)), 0.0).shape
    for off in range(4):
        sl, dl = _layouts("f32", 2, 3, H, dH, dW, off)
        values = _values(rng, "f32", sl.shape)
        buf = _run(po, 0.0, sl, dl, wrong="dst_overrun")(sl.make_src(values, "nan"))
        out, first, count = dl.check_dst(buf)
        assert (first, count) == (-4, 5)
        assert dl.changed_guards(buf).tolist() == [-4, -3, -2, -1, 2 * dl.stride + dl.row]
        assert dl.region(first)[0] == "before" and dl.region(2 * dl.stride + dl.row) == ("pad", 0, 2, dl.row)
        assert "pad (image 0, row 2" in dl.describe(2 * dl.stride + dl.row)
        # (the output itself is still right: only the guards tell)
        assert np.isfinite(out).all() and dl.sentinels_left(out) == 0
    # an output pixel that is never written keeps the sentinel
    dst = dl.make_dst()
    stand_in(po, 0.0, sl, sl.make_src(values, "nan"), dl, dst)
    dst.view(np.int32)[dl.index[1, 3, 4]] = SENTINEL_BITS
    out, first, count = dl.check_dst(dst)
    assert count == 0 and dl.sentinels_left(out) == 1 and not np.isfinite(out[1, 3].reshape(-1)[4])
