"""The interleaved planned adjoint at general rotations on the MI355X: aai_adjoint_rotated_interleaved_device_f32 /
aai_adjoint_rotated_interleaved_f32 (api.adjoint_interleaved_device / _host with planned="any") and
torch_ops.resample(..., planned_backward="interleaved").

The bar everywhere: the int32 view of gsrc equals that of adjoint_interleaved_device(planned=False) -- the general interleaved adjoint --
on the same buffers.  No tolerance is involved, except where one case is ALSO held against the oracle's matrix
(test_adjoint_host.assert_adjoint_matches) so that the file does not rest on the general adjoint alone.  Images have a few thousand
pixels, the scratch-chunking batch aside."""
import re

import numpy as np
import pytest

from guard_layout import GuardedLayout, to_device
from test_adjoint_host import EIGHT, adjoint_gold, assert_adjoint_matches
from test_adjoint_rotated_host import KNIFE_STRIDE

pytestmark = pytest.mark.gpu

PLAIN_MULTI = "aai_adjoint_plain_gather_multi_kernel"
MULTI_GATHER = "aai_adjoint_gather_multi_kernel"
PLAIN_SINGLE = "aai_adjoint_plain_gather_kernel"
AXIS_KERNEL = "aai_axis_adjoint_kernel"


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    yield aai
    torch.cuda.synchronize()
    aai.shutdown()                 # the plans of this module (and their tables) do not outlive it


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _mode_name(gpu, mode):
    return "fast" if mode == gpu.MODE_FAST else "area"


def _run(gpu, rq, g, planned="any"):
    """the device entry on a dense host gradient image [dH, dW, C], gsrc prefilled with -1; (gsrc [H, W, C] on the host, aai_last_kernel())"""
    import torch
    gd = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
    dH, dW, C = gd.shape
    gs = torch.full((rq.src_height, rq.src_width, C), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), rq.src_width * C, _stream(), batch=1, planned=planned)
    torch.cuda.synchronize()
    return gs.cpu().numpy(), gpu.last_kernel()


def _gradient(gpu, rq, channels, seed=3):
    """[dH, dW, C], every channel drawn on its own: a channel mix-up cannot pass"""
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    return np.stack([np.random.default_rng(seed + 13 * c).random((lay.dst_height, lay.dst_width)).astype(np.float32) for c in range(channels)], axis=2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_as_general(gpu, rq, channels, what, seed=3):
    """the new entry and the general interleaved entry on one gradient: equal bits; returns (gsrc, kernel of the new entry)"""
    g = _gradient(gpu, rq, channels, seed)
    got, kernel = _run(gpu, rq, g)
    ref, kref = _run(gpu, rq, g, planned=False)
    assert kref == "%s<%s, %d>" % (MULTI_GATHER, _mode_name(gpu, rq.mode), channels), kref
    diff = int((_bits(got) != _bits(ref)).sum())
    assert diff == 0, (what, kernel, "%d of %d elements differ from the general interleaved adjoint" % (diff, got.size), gpu.plan_shape(rq))
    assert (got >= 0).all(), what                               # every element written (weights and gradients are non-negative)
    return got, kernel


def _plain_name(gpu, rq, channels):
    return "%s<%s, %d>" % (PLAIN_MULTI, _mode_name(gpu, rq.mode), channels)


def _knife(gpu, rq):
    """(rot_adjoint state, count of K) of the channels = 1 plan -- the plan the new entry uses"""
    m = re.search(r"rot_adjoint=(\w+)(?: knife=(\d+))?$", gpu.plan_shape(rq, 1))
    assert m, gpu.plan_shape(rq, 1)
    return m.group(1), int(m.group(2)) if m.group(2) else None


MODES = lambda gpu: ((gpu.MODE_AREA, gpu.POLICY_REFERENCE), (gpu.MODE_AREA, gpu.POLICY_EXACT), (gpu.MODE_FAST, gpu.POLICY_REFERENCE))
GENERAL_EIGHT = [c for c in EIGHT if c[4] % 90 != 0]


# 1.  basic geometries
@pytest.mark.parametrize("channels", (2, 3, 4))
@pytest.mark.parametrize("case", range(len(GENERAL_EIGHT)))
def test_new_entry_has_the_general_interleaved_adjoints_bits(gpu, po, case, channels):
    W, H, sr, dr, ang, off = GENERAL_EIGHT[case]
    iso = ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    for mode, policy in MODES(gpu):
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
        got, kernel = _same_as_general(gpu, rq, channels, "case %d mode %d policy %d C=%d" % (case, mode, policy, channels))
        print("case %d mode %d policy %d C=%d: %s, %s" % (case, mode, policy, channels, kernel, gpu.plan_shape(rq, 1)))
        state, knife = _knife(gpu, rq)
        if case == 2:                    # 45 degrees on a 1:2 lattice is grid-aligned: whatever serves it (the bits are the general's)
            assert kernel.startswith(PLAIN_MULTI) or kernel.startswith(MULTI_GATHER), kernel
            continue
        assert kernel.startswith(_plain_name(gpu, rq, channels)), (kernel, gpu.plan_shape(rq, 1))
        assert state == "sums" and "rot_adjoint=sums" in gpu.plan_shape(rq, 1) and knife is not None
        assert kernel.endswith("+listed") == (knife > 0), (kernel, knife)
    # the host-buffer entry gives the device entry's bits
    rq = gpu.make_request(W, H, sr, dr, iso, ang)
    g = _gradient(gpu, rq, channels)
    rc, msg, gsrc = gpu.adjoint_interleaved_host(g, (H, W, channels), sr, dr, iso, ang, planned="any")
    assert rc == 0, msg
    assert np.array_equal(_bits(gsrc), _bits(_run(gpu, rq, g)[0]))
    if case == 0 and channels == 3:      # ... and one case against the oracle's matrix
        for mode, policy in MODES(gpu):
            pairs = [adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, mode, policy, seed=7 + 5 * c) for c in range(channels)]
            g = np.stack([p[0] for p in pairs], axis=2)
            got, kernel = _run(gpu, gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy), g)
            assert kernel.startswith(PLAIN_MULTI), kernel
            for c in range(channels):
                assert_adjoint_matches(got[:, :, c], pairs[c][1], "new entry against the oracle, mode %d policy %d channel %d" % (mode, policy, c))


# 2.  tile edges and replication
@pytest.mark.parametrize("side,channels", [(15, 3), (16, 3), (17, 3), (33, 3), (17, 2), (17, 4)])
def test_new_entry_at_tile_edges(gpu, side, channels):
    """source sides on both sides of the 16 x 16 workgroup and of two of them; the rows of dW * C elements (14 to 46 pixels) leave partial
    waves of the element-wise pass, and with side 17 no row length is a multiple of 64 (with C = 3 and rows of more than 64 elements a
    pixel's three elements straddle the wave boundary)"""
    plain = 0
    for (W, H) in ((side, side), (side, 21), (19, side)):
        for sr, dr, ang in ((3, 2, 17.5), (1, 1, 30.0)):
            for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
                rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2), ang, mode=mode)
                lay = gpu.query(rq)[2]
                assert lay.dst_width % 16 or lay.dst_height % 16
                if side == 17:
                    assert (lay.dst_width * channels) % 64 != 0, (lay.dst_width, channels)
                _, kernel = _same_as_general(gpu, rq, channels, "tile edges %dx%d %g:%g %g mode %d C=%d" % (W, H, sr, dr, ang, mode, channels))
                plain += kernel.startswith(PLAIN_MULTI)
    assert plain >= 10


@pytest.mark.parametrize("ang", [17.5, 107.5, 197.5, 287.5])
def test_new_entry_on_replicated_sources_in_every_quadrant(gpu, ang):
    """x2 and x3 up-sampling (scale > 1): adjoint_virtual_pixel's four branches"""
    for (W, H, dr) in ((29, 23, 2), (19, 17, 3)):
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(W, H, 1, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            assert gpu.query(rq)[2].scale > 1 and gpu.query(rq)[2].quadrant == int(ang // 90)
            _, kernel = _same_as_general(gpu, rq, 3, "x%d at %g mode %d" % (dr, ang, mode))
            assert kernel.startswith(_plain_name(gpu, rq, 3)), kernel


# 3.  knife fixtures
def test_new_entry_on_knife_edge_geometries(gpu, knife_golden):
    """the stride tests/test_adjoint_rotated_host.py fixed on the CPU; which path served a geometry is the plan's choice and is counted"""
    manifest = knife_golden[1]
    ran = plain = listed = general = 0
    for i in range(0, len(manifest), KNIFE_STRIDE):             # a fixed stride by index, never a choice by outcome
        c = manifest[i]
        if c["W"] * c["H"] > 1300:
            continue
        ran += 1
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode)
            _, kernel = _same_as_general(gpu, rq, 3, "knife %d mode %d" % (i, mode))
            state, knife = _knife(gpu, rq)
            if kernel.startswith(PLAIN_MULTI):
                assert state == "sums" and kernel.endswith("+listed") == (knife > 0), (kernel, gpu.plan_shape(rq, 1))
                plain, listed = plain + 1, listed + kernel.endswith("+listed")
            else:
                assert kernel.startswith(MULTI_GATHER) and state == "general", (kernel, gpu.plan_shape(rq, 1))
                general += 1
    print("%d geometries, %d calls: %d served by %s (%d of them with the listed pass), %d by the general interleaved adjoint"
          % (ran, 2 * ran, plain, PLAIN_MULTI, listed, general))
    assert ran >= 20 and listed >= 3 and plain - listed >= 1 and plain + general == 2 * ran


# 4.  fall-backs
def test_new_entry_near_the_axes_and_on_grid_aligned_lattices(gpu):
    """whatever serves them, the bits are the general interleaved adjoint's"""
    for (W, H, sr, dr, ang) in ((40, 30, 3, 1, 0.01), (40, 30, 3, 1, 89.99), (32, 32, 2, 1, 45.0), (16, 12, 1, 2, 45.0)):
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            _, kernel = _same_as_general(gpu, rq, 3, "%dx%d %g mode %d" % (W, H, ang, mode))
            state, _ = _knife(gpu, rq)
            print("%dx%d at %g mode %d: %s, %s" % (W, H, ang, mode, kernel, gpu.plan_shape(rq, 1)))
            assert (kernel.startswith(PLAIN_MULTI) and state == "sums") or (kernel.startswith(MULTI_GATHER) and state == "general")


def test_new_entry_at_reduced_angle_0_is_the_general_interleaved_adjoint(gpu):
    """there is no interleaved transposed separable kernel: the general multi gather serves these, under its own name"""
    for (W, H, sr, dr, ang) in ((24, 24, 4, 1, 0.0), (40, 30, 2.5, 1, 90.0), (20, 16, 2, 1, 180.0)):
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
            _, kernel = _same_as_general(gpu, rq, 3, "%dx%d %g mode %d" % (W, H, ang, mode))
            assert kernel == "%s<%s, 3>" % (MULTI_GATHER, _mode_name(gpu, mode)), kernel


def test_new_entry_with_one_channel_is_the_single_channel_rotated_entry(gpu):
    import torch
    for (W, H, sr, dr, ang, expect) in ((36, 28, 3, 1, 17.5, PLAIN_SINGLE), (24, 24, 4, 1, 0.0, AXIS_KERNEL)):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
        g = _gradient(gpu, rq, 1)
        got, kernel = _run(gpu, rq, g)
        gd = torch.from_numpy(np.ascontiguousarray(g[:, :, 0])).cuda()
        gs = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, gd.data_ptr(), gd.shape[1], gs.data_ptr(), W, _stream(), batch=1, planned="any")
        torch.cuda.synchronize()
        assert gpu.last_kernel() == kernel and kernel.startswith(expect), (kernel, gpu.last_kernel())
        assert np.array_equal(_bits(got[:, :, 0]), _bits(gs.cpu().numpy()))


# 5.  determinism and batches.  One geometry whose K is empty and one whose K is not (knife fixture 24, see the host tests)
CLEAN = (92, 68, 3.0, 1.0, (45.5, 33.5), 17.5)


def _clean_and_knife(knife_golden):
    c = knife_golden[1][24]
    return [CLEAN, (c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"])]


def test_new_entry_is_deterministic_and_batches_match_single_images(gpu, knife_golden):
    import torch
    seen = set()
    C = 3
    for geo, mode in zip(_clean_and_knife(knife_golden) + [CLEAN], (gpu.MODE_AREA, gpu.MODE_AREA, gpu.MODE_FAST)):
        rq = gpu.make_request(*geo, mode=mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        B = 5
        dstride, sstride = dW * C + 3, W * C + 5
        dimg, simg = dstride * dH + 17, sstride * H + 11              # image strides greater than H x stride
        gen = torch.Generator(device="cuda").manual_seed(21)
        gd = torch.rand(B * dimg, dtype=torch.float32, device="cuda", generator=gen)      # distinct gdst per image
        outs = []
        for planned in ("any", "any", False):
            gs = torch.full((B * simg,), -7.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dstride, gs.data_ptr(), sstride, _stream(), batch=B, dst_image_stride=dimg,
                                           src_image_stride=simg, planned=planned)
            torch.cuda.synchronize()
            if planned:
                kernel = gpu.last_kernel()
            outs.append(gs)
        assert kernel.startswith(_plain_name(gpu, rq, C)), kernel
        seen.add(kernel.endswith("+listed"))
        assert torch.equal(outs[0], outs[1])                           # two runs give equal results
        assert torch.equal(outs[0], outs[2])                           # ... and the general interleaved adjoint's batch, padding included
        gs = outs[0]
        touched = torch.zeros(B * simg, dtype=torch.bool, device="cuda")
        for b in range(B):
            one_g = gd[b * dimg:b * dimg + dstride * dH].view(dH, dstride)[:, :dW * C].contiguous()
            one = torch.full((H, W * C), -1.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_interleaved_device(rq, C, one_g.data_ptr(), dW * C, one.data_ptr(), W * C, _stream(), planned="any")
            torch.cuda.synchronize()
            assert torch.equal(gs[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W * C], one), (geo, mode, b)
            touched[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W * C] = True
        assert bool((gs[~touched] == -7.0).all())          # padding and gaps untouched
        assert bool((gs[touched] >= 0.0).all())            # every element written
    assert seen == {False, True}


def test_new_entry_batch_of_two_scratch_chunks_with_four_channels(gpu):
    """fast mode, C = 4, 256^2 up-sampled x2 at 17.5 degrees: the batch is the smallest whose 4-channel scratch takes two chunks of the
    engine's 1 GiB bound, plus one image so that the second chunk has a first and a last one.  The same batch of single-channel scratch
    would fit in one chunk.  The images on both sides of the cut equal their single-image calls."""
    import torch
    W, H, C = 256, 256, 4
    rq = gpu.make_request(W, H, 1.0, 2.0, ((W - 1) / 2, (H - 1) / 2), 17.5, mode=gpu.MODE_FAST)
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    per_image = dW * dH * C * 8
    chunk = (1 << 30) // per_image
    batch = chunk + 2
    assert 1 < chunk < 65535 and per_image * (chunk + 1) > (1 << 30) and (per_image // C) * batch <= (1 << 30)
    # gdst + gsrc + one chunk of scratch
    assert batch * dW * dH * C * 4 + batch * W * H * C * 4 + chunk * per_image < 1.9e9
    gen = torch.Generator(device="cuda").manual_seed(23)
    gd = torch.rand((batch, dH, dW, C), dtype=torch.float32, device="cuda", generator=gen)
    gs = torch.full((batch, H, W, C), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, _stream(), batch=batch,
                                   dst_image_stride=dH * dW * C, src_image_stride=H * W * C, planned="any")
    torch.cuda.synchronize()
    kernel = gpu.last_kernel()
    assert kernel.startswith(_plain_name(gpu, rq, C)), (kernel, gpu.plan_shape(rq, 1))
    assert float(gs.min()) >= 0.0                                # the -1 prefill is gone in every image of both chunks
    for b in (0, chunk - 1, chunk, chunk + 1, batch - 1):
        for planned in ("any", False):
            one = torch.full((H, W, C), -1.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_interleaved_device(rq, C, gd[b].data_ptr(), dW * C, one.data_ptr(), W * C, _stream(), planned=planned)
            torch.cuda.synchronize()
            assert torch.equal(gs[b].view(torch.int32), one.view(torch.int32)) and bool((one != 0).any()), (b, planned)
    del gd, gs
    torch.cuda.empty_cache()


# 6.  guard bands
def test_new_entry_stays_inside_its_buffers(gpu, knife_golden):
    """gdst is the guarded SOURCE (NaN around it), gsrc the guarded destination (sentinel everywhere), the three layouts of
    tests/test_gpu_memory_contract.py with rows of width x C elements: every element of gsrc inside the image finite and equal, bit for
    bit, to the tight call; nothing else written"""
    import torch
    from test_gpu_memory_contract import LAYOUTS, _pad
    B, C = 2, 3
    seen = set()
    for i, (geo, mode) in enumerate(zip(_clean_and_knife(knife_golden) + [CLEAN], (gpu.MODE_AREA, gpu.MODE_AREA, gpu.MODE_FAST))):
        rq = gpu.make_request(*geo, mode=mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        g = np.random.default_rng(5 + i).random((B, dH, dW, C)).astype(np.float32)
        tg = to_device(g)
        ts = torch.full((B, H, W, C), float("nan"), dtype=torch.float32, device="cuda")
        gpu.adjoint_interleaved_device(rq, C, tg.data_ptr(), dW * C, ts.data_ptr(), W * C, _stream(), batch=B, dst_image_stride=dW * dH * C,
                                       src_image_stride=W * H * C, planned="any")
        torch.cuda.synchronize()
        kernel = gpu.last_kernel()
        assert kernel.startswith(_plain_name(gpu, rq, C)), kernel
        seen.add(kernel.endswith("+listed"))
        tight = ts.cpu().numpy()
        assert np.isfinite(tight).all()
        for sp, so, sg, dp, do, dg in LAYOUTS:
            gstride, sstride = dW * C + _pad(dW * C, dp), W * C + _pad(W * C, sp)
            gl = GuardedLayout((B, dH, dW, C), "f32", gstride, dH * gstride + dg, do)
            sl = GuardedLayout((B, H, W, C), "f32", sstride, H * sstride + sg, so)
            gdev, sdev = to_device(gl.make_src(g, "nan")), to_device(sl.make_dst())
            gpu.adjoint_interleaved_device(rq, C, gl.ptr(gdev), gl.stride, sl.ptr(sdev), sl.stride, _stream(), batch=B,
                                           dst_image_stride=gl.image_stride, src_image_stride=sl.image_stride, planned="any")
            torch.cuda.synchronize()
            what = (gpu.last_kernel(), geo, mode, "gdst stride %d image stride %d base %+d, gsrc stride %d image stride %d base %+d"
                    % (gl.stride, gl.image_stride, gl.base_offset, sl.stride, sl.image_stride, sl.base_offset))
            assert gpu.last_kernel() == kernel, what
            out, first, count = sl.check_dst(sdev)
            assert count == 0, ("%d guard elements of gsrc were written, first: %s" % (count, sl.describe(first)), what)
            assert sl.sentinels_left(out) == 0, what
            bad = ~np.isfinite(out)
            assert not bad.any(), ("%d non-finite gsrc elements, first at %s" % (int(bad.sum()), np.argwhere(bad)[0].tolist()), what)
            assert np.array_equal(out.view(np.int32), tight.view(np.int32)), what
    assert seen == {False, True}


# 7.  torch operator
def _is_channels_last(t):
    import torch
    return t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def test_torch_operator_with_planned_backward_interleaved(gpu):
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H, sr, dr, ang = 50, 38, 3, 1, 22.5                               # a geometry no other test of this module prepares
    iso = ((W - 1) / 2, (H - 1) / 2)
    args = (sr, dr, iso, ang)
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, *args, mode=mode)
        gen = torch.Generator(device="cuda").manual_seed(5)
        x = torch.rand((2, 3, H, W), dtype=torch.float32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
        assert _is_channels_last(x)
        # no gradient wanted: no tables are built, whatever the keyword says
        y0, _ = torch_ops.resample(x, *args, mode=mode, planned_backward="interleaved")
        assert _is_channels_last(y0) and "rot_adjoint=sums" not in gpu.plan_shape(rq, 1)
        g = torch.rand(y0.shape, dtype=torch.float32, device="cuda", generator=gen)
        # the default keyword on the same tensor: the interleaved route with the general interleaved backward, and no tables
        xd = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        yd, _ = torch_ops.resample(xd, *args, mode=mode)
        (yd * g).sum().backward()
        assert _is_channels_last(yd) and _is_channels_last(xd.grad) and "rot_adjoint=sums" not in gpu.plan_shape(rq, 1)
        assert torch.equal(y0, yd.detach())
        # "interleaved": the forward builds the tables (on the channels = 1 plan), the backward is the new entry
        xi = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        yi, _ = torch_ops.resample(xi, *args, mode=mode, planned_backward="interleaved")
        assert "rot_adjoint=sums" in gpu.plan_shape(rq, 1)
        (yi * g).sum().backward()
        assert _is_channels_last(yi) and _is_channels_last(xi.grad)
        assert torch.equal(yi.detach(), yd.detach())
        assert torch.equal(xi.grad, xd.grad) and bool((xi.grad != 0).any())
        # (aai_last_kernel() is per thread and autograd runs the backward on a thread of its own: the kernel is named by the direct call)
        dH, dW = yi.shape[2], yi.shape[3]
        gl = g.contiguous(memory_format=torch.channels_last)
        direct = torch.empty((2, 3, H, W), dtype=torch.float32, device="cuda", memory_format=torch.channels_last)
        gpu.adjoint_interleaved_device(rq, 3, gl.data_ptr(), dW * 3, direct.data_ptr(), W * 3, _stream(), batch=2, dst_image_stride=dH * dW * 3,
                                       src_image_stride=H * W * 3, planned="any")
        torch.cuda.synchronize()
        assert gpu.last_kernel().startswith(_plain_name(gpu, rq, 3)), gpu.last_kernel()
        assert torch.equal(xi.grad, direct)
        # "any": the planar route -- its grad has, plane by plane, the same bits
        xa = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        ya, _ = torch_ops.resample(xa, *args, mode=mode, planned_backward="any")
        (ya * g).sum().backward()
        assert ya.is_contiguous() and xa.grad.shape == xi.grad.shape
        for b in range(2):
            for c in range(3):
                assert torch.equal(xi.grad[b, c], xa.grad[b, c]), (mode, b, c)


def test_torch_operator_interleaved_is_any_for_every_other_input(gpu):
    """a default-format tensor, a 3-D tensor and an axis geometry: the same outputs, gradients and formats as "any"; other strings raise"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 46, 34
    gen = torch.Generator(device="cuda").manual_seed(7)
    general = (3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 40.0)
    axis = (2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 180.0)
    from area_average_interpolation_amd import _lib as L
    assert gpu.query(gpu.make_request(W, H, *axis))[2].kernel == L.KERNEL_AXIS
    x4 = torch.rand((2, 3, H, W), dtype=torch.float32, device="cuda", generator=gen)
    cases = [("default format", x4, general), ("3-D", x4[0].clone(), general),
             ("channels_last at an axis geometry", x4.contiguous(memory_format=torch.channels_last), axis),
             ("channels_last with 5 channels", torch.rand((1, 5, H, W), dtype=torch.float32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last), general)]
    for what, x, args in cases:
        res = []
        for planned in ("interleaved", "any"):
            xx = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            y, iso = torch_ops.resample(xx, *args, planned_backward=planned)
            y.sum().backward()
            res.append((y.detach(), xx.grad, iso))
        (yi, gi, isoi), (ya, ga, isoa) = res
        assert isoi == isoa and torch.equal(yi, ya) and torch.equal(gi, ga), what
        assert yi.stride() == ya.stride() and gi.stride() == ga.stride(), what
        assert yi.is_contiguous(), what                                  # the planar route in every one of these cases
    with pytest.raises(ValueError):
        torch_ops.resample(x4, *general, planned_backward="sums")
    with pytest.raises(ValueError):
        torch_ops.resample(x4.contiguous(memory_format=torch.channels_last), *general, planned_backward="sums")


def test_torch_operator_refuses_to_build_the_tables_inside_a_capture(gpu, monkeypatch):
    """with the current stream reported as capturing, a rotated geometry that has its C-channel plan but no sums raises instead of
    building them (which would synchronise); once they exist the call goes through"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 54, 42
    args = (3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 30.0)                  # a geometry no other test of this module prepares
    rq = gpu.make_request(W, H, *args)
    x = torch.rand((2, 3, H, W), dtype=torch.float32, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    eager, _ = torch_ops.resample(x, *args)                              # the forward's plan for 3 channels, no tables
    assert gpu.plan_shape(rq, 3) != "" and "rot_adjoint=sums" not in gpu.plan_shape(rq, 1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        torch_ops.resample(x, *args, planned_backward="interleaved")
    assert "rot_adjoint=sums" not in gpu.plan_shape(rq, 1)
    torch_ops.resample(x, *args)                                         # the default keyword needs no tables
    torch_ops.resample(x.detach(), *args, planned_backward="interleaved")        # ... nor a call that wants no gradient
    monkeypatch.undo()
    torch_ops.resample(x, *args, planned_backward="interleaved")         # builds the tables outside a capture
    assert "rot_adjoint=sums" in gpu.plan_shape(rq, 1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    again, _ = torch_ops.resample(x, *args, planned_backward="interleaved")
    torch.cuda.synchronize()
    assert _is_channels_last(again) and torch.equal(again.detach(), eager.detach())
