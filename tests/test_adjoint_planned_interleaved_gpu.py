"""The interleaved planned adjoint at multiples of 90 degrees on the MI355X: aai_adjoint_planned_interleaved_device_f32 /
aai_adjoint_planned_interleaved_f32 (api.adjoint_interleaved_device / _host with planned="separable") and
torch_ops.resample(..., planned_backward="channels_last").

The bar everywhere: channel c of the new entry's gsrc has the int32 view of what adjoint_device(planned=True) --
aai_adjoint_planned_batch_device_f32, which tests/test_adjoint_planned_gpu.py holds to the oracle -- gives the de-interleaved plane c.
No tolerance is involved, except where one channel count is ALSO held against the oracle's matrix
(test_adjoint_host.assert_adjoint_matches) so that the file does not rest on the single-channel entry alone.  Where the new entry hands
a request on (general rotations, wide and dense plans, one channel) the bar is the bits and the kernel name of the entry it hands it to."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_order as so
from conftest import ROOT
from guard_layout import GuardedLayout, to_device
from test_adjoint_host import adjoint_gold, assert_adjoint_matches
from test_adjoint_planned_gpu import BOUNDARY_GEOMETRIES, CLEAN, GRID_Z, KNIFE, KNIFE_X2, MATRIX, MODES, _request

pytestmark = pytest.mark.gpu

MULTI_AXIS = "aai_axis_adjoint_multi_kernel"
AXIS_KERNEL = "aai_axis_adjoint_kernel"
MULTI_GATHER = "aai_adjoint_gather_multi_kernel"
PLAIN_MULTI = "aai_adjoint_plain_gather_multi_kernel"


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _run(gpu, rq, g, planned="separable"):
    """an interleaved device entry on a dense host gradient image [dH, dW, C], gsrc prefilled with -1; (gsrc [H, W, C], aai_last_kernel())"""
    import torch
    gd = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
    dH, dW, C = gd.shape
    gs = torch.full((rq.src_height, rq.src_width, C), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), rq.src_width * C, _stream(), batch=1, planned=planned)
    torch.cuda.synchronize()
    return gs.cpu().numpy(), gpu.last_kernel()


def _single(gpu, rq, plane, planned=True):
    """a single-channel device entry on one de-interleaved plane [dH, dW], gsrc prefilled with -1; (gsrc [H, W], aai_last_kernel())"""
    import torch
    gd = torch.from_numpy(np.ascontiguousarray(plane, dtype=np.float32)).cuda()
    gs = torch.full((rq.src_height, rq.src_width), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), gd.shape[1], gs.data_ptr(), rq.src_width, _stream(), batch=1, planned=planned)
    torch.cuda.synchronize()
    return gs.cpu().numpy(), gpu.last_kernel()


def _gradient(gpu, rq, channels, seed=3):
    """[dH, dW, C], every channel drawn on its own: a channel mix-up cannot pass"""
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    return np.stack([np.random.default_rng(seed + 13 * c).random((lay.dst_height, lay.dst_width)).astype(np.float32) for c in range(channels)], axis=2)


def _planes_match(gpu, rq, g, what, separable=True):
    """the new entry on g and the single-channel planned entry on every plane of g: equal bits per plane.  separable: the new kernel
    must have served the call, with "+listed" exactly when the single-channel call has it.  Returns (gsrc, kernel, single-channel kernel)"""
    C = g.shape[2]
    got, kernel = _run(gpu, rq, g)
    ksingle = None
    for c in range(C):
        one, k = _single(gpu, rq, g[:, :, c])
        assert ksingle in (None, k), (what, ksingle, k)
        ksingle = k
        diff = int((_bits(got[:, :, c]) != _bits(one)).sum())
        assert diff == 0, (what, kernel, k, "channel %d: %d of %d elements differ from the single-channel planned entry" % (c, diff, one.size), gpu.plan_shape(rq, 1))
    assert (got >= 0).all(), what                               # every element written (weights and gradients are non-negative)
    if C > 1 and (got != 0).any():
        assert not np.array_equal(got[:, :, 0], got[:, :, 1]), what
    if separable:
        assert kernel.startswith("%s<%d>" % (MULTI_AXIS, C)) and ksingle.startswith(AXIS_KERNEL), (what, kernel, ksingle, gpu.plan_shape(rq, 1))
        assert kernel in ("%s<%d>" % (MULTI_AXIS, C), "%s<%d>+listed" % (MULTI_AXIS, C)), kernel
        assert kernel.endswith("+listed") == ksingle.endswith("+listed"), (what, kernel, ksingle)
    return got, kernel, ksingle


# 1.  the matrix of tests/test_adjoint_planned_gpu.py
SEEN = {}            # (case, channels) -> (calls with "+listed", calls without)


@pytest.mark.parametrize("channels", (2, 3, 4))
@pytest.mark.parametrize("case", range(len(MATRIX)))
def test_new_entry_has_the_single_channel_planned_entrys_bits(gpu, po, case, channels):
    assert len(MATRIX) == 12
    W, H, sr, dr, ang, off, absolute = MATRIX[case]
    iso = off if absolute else ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    listed = clean = 0
    for mode, policy in MODES(gpu):
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
        what = "case %d mode %d policy %d C=%d" % (case, mode, policy, channels)
        _, kernel, _ = _planes_match(gpu, rq, _gradient(gpu, rq, channels), what)
        print("%s: %s, %s" % (what, kernel, gpu.plan_shape(rq, 1)))
        assert "adjoint=tables" in gpu.plan_shape(rq, 1)
        listed, clean = listed + kernel.endswith("+listed"), clean + (not kernel.endswith("+listed"))
        if channels == 3 and mode == gpu.MODE_AREA and policy == gpu.POLICY_REFERENCE:       # ... and against the oracle's matrix
            pairs = [adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, mode, policy, seed=7 + 5 * c) for c in range(channels)]
            got, k = _run(gpu, rq, np.stack([p[0] for p in pairs], axis=2))
            assert k.startswith(MULTI_AXIS), k
            for c in range(channels):
                assert_adjoint_matches(got[:, :, c], pairs[c][1], "new entry against the oracle, %s channel %d" % (what, c))
    # the host-buffer entry gives the device entry's bits
    rq = gpu.make_request(W, H, sr, dr, iso, ang)
    g = _gradient(gpu, rq, channels, seed=5)
    rc, msg, gsrc = gpu.adjoint_interleaved_host(g, (H, W, channels), sr, dr, iso, ang, planned="separable")
    assert rc == 0, msg
    assert gpu.last_kernel().startswith(MULTI_AXIS)
    assert np.array_equal(_bits(gsrc), _bits(_run(gpu, rq, g)[0]))
    SEEN[case, channels] = (listed, clean)


@pytest.mark.parametrize("channels", (2, 3, 4))
def test_the_matrix_geometries_cover_both_kinds_of_plan(channels):
    """(after test 1) at least one geometry that never ran the correction pass, at least three that did"""
    mine = {case: v for (case, c), v in SEEN.items() if c == channels}
    assert len(mine) == len(MATRIX), "test 1 did not run for every geometry"
    assert sum(1 for l, c in mine.values() if c and not l) >= 1
    assert sum(1 for l, c in mine.values() if l) >= 3, mine


# 2.  lane and workgroup boundaries in ELEMENTS: one lane per element of a source row of W * C floats, 64 lanes a wave, 256 elements a
# workgroup.  W * C on both sides of 64, 256 and 512; for C = 3 a pixel straddles a wave (21 * 3 = 63, 22 * 3 = 66) and a workgroup
# (85 * 3 = 255, 86 * 3 = 258; 171 * 3 = 513).  A workgroup walks 32 source rows: 33 has a second, partial row block.
ELEMENT_WIDTHS = [(21, 3, 33), (22, 3, 33), (32, 2, 33), (16, 4, 33), (85, 3, 17), (86, 3, 17), (128, 2, 13), (129, 2, 13), (64, 4, 13), (65, 4, 11),
                  (171, 3, 9)]


@pytest.mark.parametrize("geometry", BOUNDARY_GEOMETRIES, ids=[b[0] for b in BOUNDARY_GEOMETRIES])
@pytest.mark.parametrize("size", ELEMENT_WIDTHS, ids=["%dx%dx%d" % (w, h, c) for w, c, h in ELEMENT_WIDTHS])
def test_new_entry_at_lane_and_workgroup_boundaries_in_elements(gpu, size, geometry):
    (W, C, H), (name, sr, dr, ang) = size, geometry
    assert min(abs(W * C - b) for b in (64, 256, 512)) <= 4
    rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
    _planes_match(gpu, rq, _gradient(gpu, rq, C, seed=13), "boundaries %s %dx%d C=%d" % (name, W, H, C))


# 3.  quadrants and integer pre-expansion
@pytest.mark.parametrize("geo", [(40, 30, 2.5, 1, 0.0, None), (40, 30, 2.5, 1, 90.0, None), (40, 30, 2.5, 1, 180.0, None), (40, 30, 2.5, 1, 270.0, None),
                                 (16, 12, 1, 3, 270.0, None), (27, 27, 4, 3, 270.0, (13.3, 12.8))],
                         ids=["2.5:1 0", "2.5:1 90", "2.5:1 180", "2.5:1 270", "1:3 270", "4:3 270 off-centre"])
def test_new_entry_in_every_quadrant_and_with_pre_expansion(gpu, geo):
    W, H, sr, dr, ang, iso = geo
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, sr, dr, iso or ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)
        lay = gpu.query(rq)[2]
        assert lay.quadrant == int(ang // 90)
        _planes_match(gpu, rq, _gradient(gpu, rq, 3, seed=17), "%s mode %d" % (geo, mode))


# 4.
def test_new_entry_on_axis_knife_edge_geometries(gpu, axis_knife_golden):
    """the stride and the filter of test_planned_adjoint_on_axis_knife_edge_geometries, C = 3: per plane the single-channel planned
    entry's bits whichever kernel served the call (wide and dense plans keep the general kernels: counted, not prescribed)"""
    manifest = axis_knife_golden[1]
    ran = axis = listed = 0
    for i in range(0, len(manifest), 12):             # a fixed stride by index, never a choice by outcome
        c = manifest[i]
        if c["W"] * c["H"] > 1300:
            continue
        ran += 1
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            rq = gpu.make_request(c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"], mode=mode)
            _, kernel, ksingle = _planes_match(gpu, rq, _gradient(gpu, rq, 3, seed=19), "axis knife %d mode %d" % (i, mode), separable=False)
            assert kernel.startswith(MULTI_AXIS) == ksingle.startswith(AXIS_KERNEL), (i, mode, kernel, ksingle)
            assert kernel.startswith(MULTI_AXIS) or kernel.startswith(MULTI_GATHER), kernel
            if kernel.startswith(MULTI_AXIS):
                assert kernel.endswith("+listed") == ksingle.endswith("+listed"), (i, mode, kernel, ksingle)
            axis, listed = axis + kernel.startswith(MULTI_AXIS), listed + (kernel.startswith(MULTI_AXIS) and kernel.endswith("+listed"))
    print("%d geometries, %d calls served by %s, %d of them with the correction pass" % (ran, axis, MULTI_AXIS, listed))
    assert ran >= 45 and axis >= ran and listed >= 3


# 5.  what the new entry hands on carries the bits and the names of the entry it is handed to
def _same_as(gpu, rq, g, planned, what):
    a, ka = _run(gpu, rq, g)
    b, kb = _run(gpu, rq, g, planned=planned)
    assert ka == kb and np.array_equal(_bits(a), _bits(b)), (what, ka, kb)
    return ka


def test_new_entry_hands_on_with_the_existing_entries_bits_and_names(gpu):
    from area_average_interpolation_amd import _lib as L
    # a general rotation: aai_adjoint_rotated_interleaved_device_f32
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(92, 68, 3.0, 1.0, (45.5, 33.5), 17.5, mode=mode)
        for C in (2, 3, 4):
            k = _same_as(gpu, rq, _gradient(gpu, rq, C), "any", "general rotation mode %d C=%d" % (mode, C))
            assert k.startswith(PLAIN_MULTI), k
    # AAI_KERNEL_AXIS_WIDE: aai_adjoint_interleaved_device_f32
    for (W, H, sr, dr, ang) in ((3, 50, 2, 1, 0.0), (2, 30, 1, 1, 90.0), (900, 300, 300, 1, 0.0)):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
        assert gpu.query(rq)[2].kernel == L.KERNEL_AXIS_WIDE
        k = _same_as(gpu, rq, _gradient(gpu, rq, 3), False, "wide %dx%d" % (W, H))
        assert k == MULTI_GATHER + "<area, 3>", k
        assert "adjoint=none" in gpu.plan_shape(rq, 1)
    # one channel: aai_adjoint_rotated_batch_device_f32, at an axis geometry and at a general rotation
    for (W, H, sr, dr, ang, expect) in ((24, 24, 4, 1, 0.0, AXIS_KERNEL), (36, 28, 3, 1, 17.5, "aai_adjoint_plain_gather_kernel")):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
        g = _gradient(gpu, rq, 1)
        got, kernel = _run(gpu, rq, g)
        one, k = _single(gpu, rq, g[:, :, 0], planned="any")
        assert kernel == k and kernel.startswith(expect), (kernel, k)
        assert np.array_equal(_bits(got[:, :, 0]), _bits(one))


DENSE_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch            # (before the library: one HIP runtime per process)
import area_average_interpolation_amd as aai
import test_adjoint_planned_interleaved_gpu as m
aai.set_device(0)
for (W, H, sr, dr, iso, ang, mode) in ((24, 13, 3.0, 1.0, (12.5, 4.0), 180.0, 1), (27, 27, 6.0, 1.0, (13.0, 13.0), 90.0, 2)):
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    aai.adjoint_rotated_prepare(rq)
    assert "dense=1" in aai.plan_shape(rq) and "adjoint=none" in aai.plan_shape(rq), aai.plan_shape(rq)
    k = m._same_as(aai, rq, m._gradient(aai, rq, 3), False, (W, H))
    assert k.startswith(m.MULTI_GATHER), k
print("dense ok")
"""


def test_new_entry_on_a_dense_plan_is_the_general_interleaved_adjoint(gpu):
    """`dense` plans (reached by lowering AAI_MAX_LISTED_PIXELS, which the library reads once -- hence a child process), as in
    test_planned_adjoint_of_a_dense_plan_is_the_general_adjoint"""
    env = dict(os.environ, AAI_MAX_LISTED_PIXELS="3")
    p = subprocess.run([sys.executable, "-c", DENSE_CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "dense ok" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])


# 6.
def test_new_entry_is_deterministic_and_batches_match_single_images(gpu):
    import torch
    seen = set()
    C = 3
    for geo, ang, mode in ((CLEAN, 0.0, gpu.MODE_AREA), (KNIFE, 180.0, gpu.MODE_AREA), (CLEAN, 270.0, gpu.MODE_FAST)):
        rq = _request(gpu, geo, ang, mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        B = 5
        dstride, sstride = dW * C + 3, W * C + 5
        dimg, simg = dstride * dH + 17, sstride * H + 11              # image strides greater than H x stride
        gen = torch.Generator(device="cuda").manual_seed(21)
        gd = torch.rand(B * dimg, dtype=torch.float32, device="cuda", generator=gen)      # distinct gdst per image
        outs = []
        for _ in range(2):
            gs = torch.full((B * simg,), -7.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dstride, gs.data_ptr(), sstride, _stream(), batch=B, dst_image_stride=dimg,
                                           src_image_stride=simg, planned="separable")
            torch.cuda.synchronize()
            outs.append(gs)
        kernel = gpu.last_kernel()
        assert kernel.startswith("%s<%d>" % (MULTI_AXIS, C)), kernel
        seen.add(kernel.endswith("+listed"))
        assert torch.equal(outs[0], outs[1])                           # two runs give equal results
        gs = outs[0]
        touched = torch.zeros(B * simg, dtype=torch.bool, device="cuda")
        for b in range(B):
            one_g = gd[b * dimg:b * dimg + dstride * dH].view(dH, dstride)[:, :dW * C].contiguous()
            one = torch.full((H, W * C), -1.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_interleaved_device(rq, C, one_g.data_ptr(), dW * C, one.data_ptr(), W * C, _stream(), planned="separable")
            torch.cuda.synchronize()
            assert gpu.last_kernel() == kernel
            assert torch.equal(gs[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W * C], one), (geo, ang, mode, b)
            touched[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W * C] = True
        assert bool((gs[~touched] == -7.0).all())          # padding and gaps keep the prefill
        assert bool((gs[touched] >= 0.0).all())            # every element written
    assert seen == {False, True}


# 7.
def _batch_against_single_images(gpu, rq, C, batch, images, seed=9):
    """one call over `batch` dense images (gsrc prefilled with -7) and, for `images`, their single-image calls: bit for bit"""
    import torch
    W, H = rq.src_width, rq.src_height
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    gen = torch.Generator(device="cuda").manual_seed(seed)
    gd = torch.rand((batch, dH, dW, C), dtype=torch.float32, device="cuda", generator=gen)
    gs = torch.full((batch, H, W, C), -7.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_interleaved_device(rq, C, gd.data_ptr(), dW * C, gs.data_ptr(), W * C, _stream(), batch=batch, dst_image_stride=dW * dH * C,
                                   src_image_stride=W * H * C, planned="separable")
    torch.cuda.synchronize()
    kernel = gpu.last_kernel()
    for b in images:
        one = torch.full((H, W, C), -1.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_interleaved_device(rq, C, gd[b].data_ptr(), dW * C, one.data_ptr(), W * C, _stream(), planned="separable")
        torch.cuda.synchronize()
        assert gpu.last_kernel() == kernel and torch.equal(gs[b], one) and bool((one != 0).any()), (b, kernel, gpu.last_kernel())
    return gs, kernel


def test_new_entry_with_a_list_across_a_scratch_chunk_cut(gpu):
    """KNIFE_X2 at 180 degrees with C = 4: 88 x 44 x 4 doubles = 123,904 bytes of scratch per image in flight, so the 1 GiB rule cuts the
    batch at 2^30 // 123,904 = 8,665 images, 1 < chunk < 65535.  Three images past the cut: the images on both sides of it equal their
    single-image calls."""
    import torch
    C = 4
    rq = _request(gpu, KNIFE_X2, 180.0, gpu.MODE_AREA)
    lay = gpu.query(rq)[2]
    per_image = lay.dst_width * lay.dst_height * C * 8
    chunk = (1 << 30) // per_image
    assert per_image == 123904 and chunk == 8665 and 1 < chunk < GRID_Z
    batch = chunk + 3
    gs, kernel = _batch_against_single_images(gpu, rq, C, batch, (0, chunk - 1, chunk, chunk + 1, batch - 1))
    assert kernel == "%s<%d>+listed" % (MULTI_AXIS, C), (kernel, gpu.plan_shape(rq, 1))
    assert float(gs.min()) >= 0.0                  # every element of every image written
    del gs
    torch.cuda.empty_cache()


def test_new_entry_without_scratch_past_grid_z(gpu):
    """the path WITHOUT a list allocates nothing and is cut by grid.z alone: 65,540 images of 24 x 24 (4:1, 0 degrees), C = 2"""
    import torch
    C = 2
    rq = gpu.make_request(24, 24, 4, 1, (11.5, 11.5), 0.0)
    batch = 65540
    assert batch > GRID_Z
    gs, kernel = _batch_against_single_images(gpu, rq, C, batch, (0, GRID_Z - 1, GRID_Z, GRID_Z + 1, batch - 1))
    assert kernel == "%s<%d>" % (MULTI_AXIS, C), (kernel, gpu.plan_shape(rq, 1))
    assert float(gs.min()) >= 0.0
    del gs
    torch.cuda.empty_cache()


# 8.
@pytest.mark.parametrize("ang", [0.0, 90.0, 180.0, 270.0])
def test_new_entry_stays_inside_its_buffers(gpu, ang):
    """gdst is the guarded SOURCE (NaN around it), gsrc the guarded destination (sentinel everywhere), the three layouts of
    tests/test_gpu_memory_contract.py with rows of width x C elements: every element of gsrc inside the image finite and equal, bit for
    bit, to the tight call; nothing else written"""
    import torch
    from test_gpu_memory_contract import LAYOUTS, _pad
    B, C = 2, 3
    seen = set()
    for i, (geo, mode) in enumerate(((CLEAN, gpu.MODE_AREA), (KNIFE, gpu.MODE_AREA), (CLEAN, gpu.MODE_FAST))):
        rq = _request(gpu, geo, ang, mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        g = np.random.default_rng(5 + i).random((B, dH, dW, C)).astype(np.float32)
        tg = to_device(g)
        ts = torch.full((B, H, W, C), float("nan"), dtype=torch.float32, device="cuda")
        gpu.adjoint_interleaved_device(rq, C, tg.data_ptr(), dW * C, ts.data_ptr(), W * C, _stream(), batch=B, dst_image_stride=dW * dH * C,
                                       src_image_stride=W * H * C, planned="separable")
        torch.cuda.synchronize()
        kernel = gpu.last_kernel()
        assert kernel.startswith("%s<%d>" % (MULTI_AXIS, C)), kernel
        seen.add(kernel.endswith("+listed"))
        tight = ts.cpu().numpy()
        assert np.isfinite(tight).all()
        for sp, so_, sg, dp, do, dg in LAYOUTS:
            gstride, sstride = dW * C + _pad(dW * C, dp), W * C + _pad(W * C, sp)
            gl = GuardedLayout((B, dH, dW, C), "f32", gstride, dH * gstride + dg, do)
            sl = GuardedLayout((B, H, W, C), "f32", sstride, H * sstride + sg, so_)
            gdev, sdev = to_device(gl.make_src(g, "nan")), to_device(sl.make_dst())
            gpu.adjoint_interleaved_device(rq, C, gl.ptr(gdev), gl.stride, sl.ptr(sdev), sl.stride, _stream(), batch=B,
                                           dst_image_stride=gl.image_stride, src_image_stride=sl.image_stride, planned="separable")
            torch.cuda.synchronize()
            what = (gpu.last_kernel(), geo, ang, mode, "gdst stride %d image stride %d base %+d, gsrc stride %d image stride %d base %+d"
                    % (gl.stride, gl.image_stride, gl.base_offset, sl.stride, sl.image_stride, sl.base_offset))
            assert gpu.last_kernel() == kernel, what
            out, first, count = sl.check_dst(sdev)
            assert count == 0, ("%d guard elements of gsrc were written, first: %s" % (count, sl.describe(first)), what)
            assert sl.sentinels_left(out) == 0, what
            bad = ~np.isfinite(out)
            assert not bad.any(), ("%d non-finite gsrc elements, first at %s" % (int(bad.sum()), np.argwhere(bad)[0].tolist()), what)
            assert np.array_equal(out.view(np.int32), tight.view(np.int32)), what
    assert seen == {False, True}


# 9.  the stream-order contract, through tests/stream_order.py as tests/test_gpu_stream_order.py runs its adjoint scenarios
STREAM_ORDER = {"adjoint separable interleaved C=3": ((160, 120, 2.5, 1.0, 90.0, 1), False),
                "adjoint separable interleaved C=3, listed": ((27, 27, 4.0, 3.0, 270.0, 1), True)}


@pytest.fixture(scope="module")
def harness(gpu):
    """the two scenarios (buffers, seeded frames, synchronous references, event-timed calls), then the delay sized by the slower of
    them and the canary; the calibration is not written to profiles/"""
    h = so.Harness(gpu)
    for i, (name, (geo, listed)) in enumerate(STREAM_ORDER.items()):
        try:
            so.adjoint(h, name, geo, 51 + i, planned="separable", channels=3, kernel=MULTI_AXIS, listed=listed)
        except Exception as e:                             # a scenario that cannot be built fails its own test
            h.broken[name] = e
    if h.call_ms:
        h.calibrate()
        h.run_canary()
        print(h.report)
    return h


@pytest.mark.parametrize("name", list(STREAM_ORDER))
def test_new_entry_in_a_frame_loop(harness, name):
    """gdst from a delayed producer, gsrc read by a consumer behind the call, gdst overwritten right after"""
    h = harness
    sc = h.scenario(name)
    assert sc.kernel.endswith("+listed") == STREAM_ORDER[name][1], (sc.kernel, sc.info)
    h.require_canary()
    assert h.delay_ms >= so.MARGIN * max(h.call_ms.values()), h.report
    for caller in h.callers():
        h.frame_loop(sc, caller)


# 10.  torch operator
def _is_channels_last(t):
    import torch
    return t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


@pytest.mark.parametrize("geo", [(46, 34, 2.0, 1.0, 180.0), (40, 30, 2.5, 1.0, 90.0)], ids=["2:1 180", "2.5:1 90"])
def test_torch_operator_with_planned_backward_channels_last(gpu, geo):
    import torch
    from area_average_interpolation_amd import _lib as L
    from area_average_interpolation_amd import torch_ops
    W, H, sr, dr, ang = geo
    iso = ((W - 1) / 2, (H - 1) / 2)
    args = (sr, dr, iso, ang)
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(W, H, *args, mode=mode)
        assert gpu.query(rq)[2].kernel == L.KERNEL_AXIS
        gen = torch.Generator(device="cuda").manual_seed(5)
        x = torch.rand((2, 3, H, W), dtype=torch.float32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
        assert _is_channels_last(x)
        # the default keyword: the interleaved route, the general interleaved backward
        xd = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        yd, _ = torch_ops.resample(xd, *args, mode=mode)
        assert _is_channels_last(yd)
        g = torch.rand(yd.shape, dtype=torch.float32, device="cuda", generator=gen)
        # "channels_last": the interleaved route too, and the backward is the new entry
        xc = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        yc, _ = torch_ops.resample(xc, *args, mode=mode, planned_backward="channels_last")
        assert "adjoint=tables" in gpu.plan_shape(rq, 1)
        (yc * g).sum().backward()
        assert _is_channels_last(yc) and _is_channels_last(xc.grad)
        assert torch.equal(yc.detach(), yd.detach())
        # True: the planar route -- its gradient has, plane by plane, the same bits; its forward is within the library's tolerance
        xp = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        yp, _ = torch_ops.resample(xp, *args, mode=mode, planned_backward=True)
        (yp * g).sum().backward()
        assert yp.is_contiguous() and xp.grad.shape == xc.grad.shape
        for b in range(2):
            for c in range(3):
                assert torch.equal(xc.grad[b, c].contiguous().view(torch.int32), xp.grad[b, c].contiguous().view(torch.int32)), (mode, b, c)
                assert bool((xc.grad[b, c] != 0).any())
        assert float((yc.detach() - yp.detach()).abs().max()) <= 1e-5 * float(yp.detach().abs().max())
        # (aai_last_kernel() is per thread and autograd runs the backward on a thread of its own: the kernel is named by the direct call)
        dH, dW = yc.shape[2], yc.shape[3]
        gl = g.contiguous(memory_format=torch.channels_last)
        direct = torch.empty((2, 3, H, W), dtype=torch.float32, device="cuda", memory_format=torch.channels_last)
        gpu.adjoint_interleaved_device(rq, 3, gl.data_ptr(), dW * 3, direct.data_ptr(), W * 3, _stream(), batch=2, dst_image_stride=dH * dW * 3,
                                       src_image_stride=H * W * 3, planned="separable")
        torch.cuda.synchronize()
        assert gpu.last_kernel().startswith(MULTI_AXIS + "<3>"), gpu.last_kernel()
        assert torch.equal(xc.grad, direct)
        # "interleaved" at this geometry is still the planar route
        yi, _ = torch_ops.resample(x, *args, mode=mode, planned_backward="interleaved")
        assert yi.is_contiguous() and torch.equal(yi, yp.detach())


def test_torch_operator_channels_last_is_interleaved_for_every_other_input(gpu):
    """a channels_last tensor at a general rotation, a default-format tensor, a 3-D tensor and five channels (the last three at an axis
    geometry too): the same outputs, gradients and strides as "interleaved" """
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 46, 34
    gen = torch.Generator(device="cuda").manual_seed(7)
    general = (3.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 40.0)
    axis = (2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 180.0)
    x4 = torch.rand((2, 3, H, W), dtype=torch.float32, device="cuda", generator=gen)
    x5 = torch.rand((1, 5, H, W), dtype=torch.float32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    cases = [("channels_last at a general rotation", x4.contiguous(memory_format=torch.channels_last), general)]
    for where, args in (("general rotation", general), ("axis geometry", axis)):
        cases += [("default format, " + where, x4, args), ("3-D, " + where, x4[0].clone(), args), ("channels_last with 5 channels, " + where, x5, args)]
    for what, x, args in cases:
        res = []
        for planned in ("channels_last", "interleaved"):
            xx = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            y, iso = torch_ops.resample(xx, *args, planned_backward=planned)
            y.sum().backward()
            res.append((y.detach(), xx.grad, iso))
        (yc, gc, isoc), (yi, gi, isoi) = res
        assert isoc == isoi and torch.equal(yc, yi) and torch.equal(gc, gi), what
        assert yc.stride() == yi.stride() and gc.stride() == gi.stride(), what
    with pytest.raises(ValueError):
        torch_ops.resample(x4, *general, planned_backward="separable")


def test_torch_operator_refuses_to_build_the_tables_inside_a_capture(gpu, monkeypatch):
    """with the current stream reported as capturing, an axis geometry that has its C-channel plan but no tables on the single-channel
    plan raises instead of building them (which would synchronise); after adjoint_rotated_prepare the call goes through"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 104, 88
    args = (2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 90.0)                  # a geometry no other test prepares
    rq = gpu.make_request(W, H, *args)
    x = torch.rand((2, 3, H, W), dtype=torch.float32, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    eager, _ = torch_ops.resample(x, *args)                              # the forward's plan for 3 channels; no single-channel plan
    assert gpu.plan_shape(rq, 3) != "" and "adjoint=tables" not in gpu.plan_shape(rq, 1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        torch_ops.resample(x, *args, planned_backward="channels_last")
    assert "adjoint=tables" not in gpu.plan_shape(rq, 1)
    torch_ops.resample(x, *args)                                         # the default keyword needs no tables
    torch_ops.resample(x.detach(), *args, planned_backward="channels_last")      # ... nor a call that wants no gradient
    monkeypatch.undo()
    gpu.adjoint_rotated_prepare(rq)
    assert "adjoint=tables" in gpu.plan_shape(rq, 1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    again, _ = torch_ops.resample(x, *args, planned_backward="channels_last")
    again.sum().backward()
    torch.cuda.synchronize()
    assert _is_channels_last(again) and torch.equal(again.detach(), eager.detach())
    assert _is_channels_last(x.grad) and bool((x.grad != 0).any())


# 11.
def test_the_rotated_interleaved_entry_at_reduced_angle_0_is_untouched(gpu):
    rq = gpu.make_request(24, 24, 4, 1, (11.5, 11.5), 0.0)
    assert _run(gpu, rq, _gradient(gpu, rq, 3), planned="any")[1] == MULTI_GATHER + "<area, 3>"
