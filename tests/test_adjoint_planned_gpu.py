"""The planned adjoint on the MI355X: aai_adjoint_planned_batch_device_f32 / aai_adjoint_planned_f32 / aai_adjoint_prepare and
torch_ops.resample(..., planned_backward=True).

At rotations by multiples of 90 degrees the transposed separable kernel (aai_axis_adjoint_kernel) serves the call, with the listed
passes of the general adjoint behind it where the plan has flagged pixels ("+listed"); everything else is the existing adjoint, bit
for bit.  Gold is the oracle's matrix built column by column (small geometries) or columns of it from comb images
(tests/adjoint_columns.py); the bar is that of tests/test_adjoint_host.py: conftest.TOL relative with a floor of 1e-3 max|gold|, and
exact zeros where the oracle's column is zero."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from adjoint_columns import comb_cases, comb_pitch
from guard_layout import GuardedLayout, to_device
from test_adjoint_host import adjoint_gold, assert_adjoint_matches

pytestmark = pytest.mark.gpu

AXIS_KERNEL = "aai_axis_adjoint_kernel"
GATHER_KERNEL = "aai_adjoint_gather_kernel"


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from area_average_interpolation_amd import _lib as L
    L.load()                       # raises if libaai_hip.so is missing: no silent fallback
    assert aai.device_count() >= 1
    aai.set_device(0)
    return aai


def _flagged(gpu, rq):
    m = re.search(r"flagged=(\d+) dense=(\d+)", gpu.plan_shape(rq))
    assert m, gpu.plan_shape(rq)
    return int(m.group(1)), int(m.group(2))


def _planned(gpu, rq, g, planned=True):
    """the device entry on a host gradient image, gsrc prefilled with -1; (gsrc on the host, aai_last_kernel())"""
    import torch
    gd = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
    gs = torch.full((rq.src_height, rq.src_width), -1.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), gd.shape[1], gs.data_ptr(), rq.src_width, torch.cuda.current_stream().cuda_stream, batch=1, planned=planned)
    torch.cuda.synchronize()
    return gs.cpu().numpy(), gpu.last_kernel()


def _omode(gpu, po, mode):
    return po.MODE_FAST if mode == gpu.MODE_FAST else po.MODE_EXACT


MODES = lambda gpu: ((gpu.MODE_AREA, gpu.POLICY_REFERENCE), (gpu.MODE_AREA, gpu.POLICY_EXACT), (gpu.MODE_FAST, gpu.POLICY_REFERENCE))

# 1.  (W, H, srcRes, dstRes, angle, isocenter: offset from the image centre, or absolute when the last field is True).  The first
# eight are the issue's set; none of them has a flagged pixel in any mode (every plan of theirs says flagged=0), so NONE WAS REPLACED and
# four geometries of tests/golden/axis_knife_cases.npz were ADDED whose plans do list pixels (in area or in fast mode): dst edges through
# pixel centres beside edges along pixel boundaries, at 180, 270, 90 and 0 degrees, one with integer pre-expansion (4:3).
MATRIX = [(24, 24, 4, 1, 0, (0, 0), False), (20, 16, 2, 1, 180, (0, 0), False), (40, 30, 2.5, 1, 90, (0, 0), False), (40, 30, 2.5, 1, 270, (0, 0), False),
          (21, 17, 3, 2, 0, (0.3, -0.2), False), (20, 24, 1, 1, 90, (0, 0), False), (16, 12, 1, 2, 0, (0, 0), False), (16, 12, 1, 3, 270, (0, 0), False),
          (24, 13, 3, 1, 180, (12.5, 4.0), True), (27, 27, 4, 3, 270, (13.0, 13.0), True), (27, 27, 6, 1, 90, (13.0, 13.0), True),
          (60, 7, 3, 2, 0, (20.25, 1.75), True)]
LISTED = {}          # case -> (modes with flagged > 0 and "+listed", modes with flagged = 0), filled by test 1


@pytest.mark.parametrize("case", range(len(MATRIX)))
def test_planned_adjoint_matches_the_oracle_matrix(gpu, po, case):
    W, H, sr, dr, ang, off, absolute = MATRIX[case]
    iso = off if absolute else ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])
    listed = clean = 0
    for mode, policy in MODES(gpu):
        g, gold = adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, mode, policy)
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode, policy=policy)
        got, kernel = _planned(gpu, rq, g)
        flagged, dense = _flagged(gpu, rq)
        print("case %d mode %d policy %d: %s, flagged=%d dense=%d, %s" % (case, mode, policy, kernel, flagged, dense, gpu.plan_shape(rq)))
        assert kernel.startswith(AXIS_KERNEL) and dense == 0, (kernel, gpu.plan_shape(rq))
        assert "adjoint=tables" in gpu.plan_shape(rq)
        assert kernel.endswith("+listed") or flagged == 0, (kernel, flagged)       # (a plan without flagged pixels may still list grazed rows)
        listed, clean = listed + (flagged > 0), clean + (flagged == 0)
        assert_adjoint_matches(got, gold, "planned case %d mode %d policy %d" % (case, mode, policy))
        # the general adjoint on the same gradient: a few 1e-7 apart (include/aai.h), far inside the bar
        ref, kref = _planned(gpu, rq, g, planned=False)
        assert GATHER_KERNEL in kref
        assert_adjoint_matches(got, ref.astype(np.float64), "planned against general, case %d mode %d policy %d" % (case, mode, policy))
    # the host-buffer entry gives the device entry's bits
    g, _ = adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, gpu.MODE_AREA)
    rc, msg, gsrc = gpu.adjoint_host(g, (H, W), sr, dr, iso, ang, planned=True)
    assert rc == 0, msg
    assert np.array_equal(gsrc, _planned(gpu, gpu.make_request(W, H, sr, dr, iso, ang), g)[0])
    LISTED[case] = (listed, clean)


def test_the_matrix_geometries_cover_both_kinds_of_plan():
    """(after test 1) at least one geometry without flagged pixels, at least three whose planned call ran the correction pass"""
    assert len(LISTED) == len(MATRIX), "test 1 did not run for every geometry"
    assert sum(1 for l, c in LISTED.values() if c and not l) >= 1
    assert sum(1 for l, c in LISTED.values() if l) >= 3, LISTED


# 2.  lane, vector and strip boundaries.  One lane per source column, 64 lanes a wave, 256 columns a workgroup: widths on both sides of
# 64, 256 and 512; the heights fall from 33 to 9 as the widths grow (a workgroup walks 32 source rows: 33 has a second, partial one).
WIDTHS = [(63, 33), (64, 31), (65, 29), (255, 17), (256, 13), (257, 11), (513, 9)]
BOUNDARY_GEOMETRIES = [("2:1 0", 2, 1, 0.0), ("3:1 0", 3, 1, 0.0), ("2:1 90", 2, 1, 90.0), ("3:1 90", 3, 1, 90.0), ("x2 0", 1, 2, 0.0)]


@pytest.mark.parametrize("geometry", BOUNDARY_GEOMETRIES, ids=[b[0] for b in BOUNDARY_GEOMETRIES])
@pytest.mark.parametrize("size", WIDTHS, ids=["%dx%d" % s for s in WIDTHS])
def test_planned_adjoint_at_lane_vector_and_strip_boundaries(gpu, po, size, geometry):
    """Combs of EVERY x phase (one phase per residue of x modulo the pitch, so every source column is among the pixels: every residue
    modulo 4 and modulo 64, the first and last two columns, both sides of every 256-column boundary -- asserted), their y phases
    chosen so that rows 0, 1, H-2 and H-1 are among the rows."""
    (W, H), (name, sr, dr, ang) = size, geometry
    iso = ((W - 1) / 2, (H - 1) / 2)
    mode = gpu.MODE_AREA
    rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
    rc, msg, lay = gpu.query(rq)
    assert rc == 0, msg
    pitch = comb_pitch(lay, ang)
    ys = [0, 1, (H - 2) % pitch, (H - 1) % pitch]
    phases = [(ox, ys[ox % 4] if ox < 4 else (ox * 3) % pitch) for ox in range(pitch)]
    assert pitch >= 4 and len(set(phases)) == pitch
    g = np.random.default_rng(13).random((lay.dst_height, lay.dst_width)).astype(np.float32)
    sx, sy, gold = comb_cases(po, _omode(gpu, po, mode), W, H, sr, dr, iso, ang, 0, g, phases, pitch)
    assert set(sx.tolist()) == set(range(W))
    assert set(np.unique(sx % 4)) == set(range(4)) and set(np.unique(sx % 64)) == set(range(min(W, 64)))
    for b in range(256, W, 256):
        assert b - 1 in sx and b in sx
    assert set((0, 1, H - 2, H - 1)) <= set(sy.tolist())
    assert 4 * int((gold != 0).sum()) >= sx.size
    got, kernel = _planned(gpu, rq, g)
    assert kernel.startswith(AXIS_KERNEL), kernel
    assert_adjoint_matches(got[sy, sx], gold, "boundaries %s %dx%d (%d source pixels, %s)" % (name, W, H, sx.size, kernel))


# 3.
def test_planned_adjoint_on_axis_knife_edge_geometries(gpu, po, axis_knife_golden):
    """the stride and the minimum count of test_adjoint_on_axis_knife_edge_geometries, through the planned entry; which kernel served a
    geometry is the library's choice (wide and dense plans keep the general kernels) and is counted, not prescribed"""
    manifest = axis_knife_golden[1]
    ran = axis = listed = 0
    for i in range(0, len(manifest), 12):             # a fixed stride by index, never a choice by outcome
        c = manifest[i]
        if c["W"] * c["H"] > 1300:
            continue
        ran += 1
        for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
            W, H, sr, dr, iso, ang = c["W"], c["H"], c["src_res"], c["dst_res"], tuple(c["iso"]), c["angle"]
            g, gold = adjoint_gold(po, gpu, W, H, sr, dr, iso, ang, mode, gpu.POLICY_REFERENCE)
            got, kernel = _planned(gpu, gpu.make_request(W, H, sr, dr, iso, ang, mode=mode), g)
            assert kernel.startswith(AXIS_KERNEL) or GATHER_KERNEL in kernel, kernel
            axis, listed = axis + kernel.startswith(AXIS_KERNEL), listed + kernel.endswith("+listed")
            assert_adjoint_matches(got, gold, "planned axis knife %d mode %d (%s)" % (i, mode, kernel))
    print("%d geometries, %d calls served by %s, %d of them with the correction pass" % (ran, axis, AXIS_KERNEL, listed))
    assert ran >= 45 and axis >= ran and listed >= 3


# 4.
def _both(gpu, rq, seed=3):
    lay = gpu.query(rq)[2]
    g = np.random.default_rng(seed).random((lay.dst_height, lay.dst_width)).astype(np.float32)
    a, ka = _planned(gpu, rq, g)
    b, kb = _planned(gpu, rq, g, planned=False)
    return a, ka, b, kb


def test_planned_adjoint_falls_back_to_the_general_kernels(gpu):
    from area_average_interpolation_amd import _lib as L
    # a general rotation
    for mode in (gpu.MODE_AREA, gpu.MODE_FAST):
        rq = gpu.make_request(92, 68, 3.0, 1.0, (45.5, 33.5), 17.5, mode=mode)
        gpu.adjoint_prepare(rq)                                        # a validated no-op: no plan is built
        assert gpu.plan_shape(rq) == ""
        a, ka, b, kb = _both(gpu, rq)
        assert GATHER_KERNEL in ka and ka == kb and np.array_equal(a.view(np.int32), b.view(np.int32))
    # images narrower than one 4-column vector, and a footprint wider than a strip: AAI_KERNEL_AXIS_WIDE
    for (W, H, sr, dr, ang) in ((3, 50, 2, 1, 0.0), (2, 30, 1, 1, 90.0), (900, 300, 300, 1, 0.0)):
        rq = gpu.make_request(W, H, sr, dr, ((W - 1) / 2, (H - 1) / 2), ang)
        assert gpu.query(rq)[2].kernel == L.KERNEL_AXIS_WIDE
        gpu.adjoint_prepare(rq)
        assert "adjoint=none" in gpu.plan_shape(rq)
        a, ka, b, kb = _both(gpu, rq)
        assert GATHER_KERNEL in ka and ka == kb and np.array_equal(a.view(np.int32), b.view(np.int32)), (W, H)


DENSE_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch            # (before the library: one HIP runtime per process)
import area_average_interpolation_amd as aai
import test_adjoint_planned_gpu as m
aai.set_device(0)
for (W, H, sr, dr, iso, ang, mode) in ((24, 13, 3.0, 1.0, (12.5, 4.0), 180.0, 1), (27, 27, 6.0, 1.0, (13.0, 13.0), 90.0, 2)):
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    aai.adjoint_prepare(rq)
    assert "dense=1" in aai.plan_shape(rq) and "adjoint=none" in aai.plan_shape(rq), aai.plan_shape(rq)
    a, ka, b, kb = m._both(aai, rq)
    assert m.GATHER_KERNEL in ka and ka == kb and np.array_equal(a.view(np.int32), b.view(np.int32)), (ka, kb)
print("dense ok")
"""


def test_planned_adjoint_of_a_dense_plan_is_the_general_adjoint(gpu):
    """`dense` plans (reached by lowering AAI_MAX_LISTED_PIXELS, which the library reads once -- hence a child process): two of test 1's
    geometries with flagged > 3 take the general path whole"""
    env = dict(os.environ, AAI_MAX_LISTED_PIXELS="3")
    p = subprocess.run([sys.executable, "-c", DENSE_CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "dense ok" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])


# 5. / 6.  one geometry whose plan has no flagged pixel and one whose plan has some, per quadrant
CLEAN = (129, 65, 4.0, 1.0, None)                  # isocenter at the image centre
KNIFE = (132, 67, 3.0, 1.0, (12.5, 4.0))           # x edges through pixel centres, y edges along pixel boundaries (the 24 x 13 one of test 1, larger)


def _request(gpu, geo, ang, mode):
    W, H, sr, dr, iso = geo
    return gpu.make_request(W, H, sr, dr, iso if iso else ((W - 1) / 2, (H - 1) / 2), ang, mode=mode)


def test_planned_adjoint_is_deterministic_and_batches_match_single_images(gpu):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    seen = set()
    for geo, ang, mode in ((CLEAN, 0.0, gpu.MODE_AREA), (KNIFE, 180.0, gpu.MODE_AREA), (CLEAN, 270.0, gpu.MODE_FAST)):
        rq = _request(gpu, geo, ang, mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        B = 5
        dstride, sstride = dW + 3, W + 5
        dimg, simg = dstride * dH + 17, sstride * H + 11              # image strides greater than H x stride
        gen = torch.Generator(device="cuda").manual_seed(21)
        gd = torch.rand(B * dimg, dtype=torch.float32, device="cuda", generator=gen)      # distinct gdst per image
        outs = []
        for _ in range(2):
            gs = torch.full((B * simg,), -7.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_device(rq, gd.data_ptr(), dstride, gs.data_ptr(), sstride, st, batch=B, dst_image_stride=dimg, src_image_stride=simg, planned=True)
            torch.cuda.synchronize()
            outs.append(gs)
        kernel = gpu.last_kernel()
        flagged, _ = _flagged(gpu, rq)
        assert kernel.startswith(AXIS_KERNEL) and (kernel.endswith("+listed") or flagged == 0), (kernel, flagged)
        seen.add(flagged > 0)
        assert torch.equal(outs[0], outs[1])
        gs = outs[0]
        touched = torch.zeros(B * simg, dtype=torch.bool, device="cuda")
        for b in range(B):
            one_g = gd[b * dimg:b * dimg + dstride * dH].view(dH, dstride)[:, :dW].contiguous()
            one = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
            gpu.adjoint_device(rq, one_g.data_ptr(), dW, one.data_ptr(), W, st, planned=True)
            torch.cuda.synchronize()
            assert torch.equal(gs[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W], one), (geo, ang, mode, b)
            touched[b * simg:b * simg + sstride * H].view(H, sstride)[:, :W] = True
        assert bool((gs[~touched] == -7.0).all())          # padding and gaps untouched
        assert bool((gs[touched] >= 0.0).all())            # every pixel written (weights and gradients are non-negative)
    assert seen == {False, True}


def _batch_against_single_images(gpu, rq, batch, images, planned=True, seed=9):
    """one planned call over `batch` dense images (gsrc prefilled with -7) and, for `images`, their single-image calls: bit for bit;
    (gsrc of the batch, aai_last_kernel() of the batch call, gdst)"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    W, H = rq.src_width, rq.src_height
    lay = gpu.query(rq)[2]
    dW, dH = lay.dst_width, lay.dst_height
    gen = torch.Generator(device="cuda").manual_seed(seed)
    gd = torch.rand((batch, dH, dW), dtype=torch.float32, device="cuda", generator=gen)
    gs = torch.full((batch, H, W), -7.0, dtype=torch.float32, device="cuda")
    gpu.adjoint_device(rq, gd.data_ptr(), dW, gs.data_ptr(), W, st, batch=batch, dst_image_stride=dW * dH, src_image_stride=W * H, planned=planned)
    torch.cuda.synchronize()
    kernel = gpu.last_kernel()
    for b in images:
        one = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, gd[b].data_ptr(), dW, one.data_ptr(), W, st, planned=planned)
        torch.cuda.synchronize()
        assert gpu.last_kernel() == kernel and torch.equal(gs[b], one), (b, kernel, gpu.last_kernel())
    return gs, kernel, gd


GRID_Z = 65535                                     # images one launch takes: grid.z carries the batch
KNIFE_X2 = (264, 133, 3.0, 1.0, (12.5, 4.0))       # KNIFE at twice the size: the same edges through pixel centres, 88 x 44 dst pixels


@pytest.mark.parametrize("geo", [KNIFE, KNIFE_X2], ids=["knife-grid.z-cut", "knife-x2-1GiB-cut"])
def test_planned_adjoint_with_a_list_across_a_scratch_chunk_cut(gpu, geo):
    """The planned path WITH a correction list takes fp64 scratch of dW x dH x 8 bytes per image in flight and goes through in chunks of
    min(batch, 65535, 2^30 // per_image) images.  KNIFE_X2 (30,976 bytes per image) is cut by the 1 GiB rule, 1 < chunk < 65535, as in
    test_rotated_adjoint_batch_of_two_scratch_chunks; KNIFE itself (44 x 22 dst pixels, 7,744 bytes per image: 2^30 // 7744 = 138,654)
    is cut by grid.z first.  Three images past the cut: the images on both sides of it equal their single-image calls bit for bit."""
    import torch
    rq = _request(gpu, geo, 180.0, gpu.MODE_AREA)
    lay = gpu.query(rq)[2]
    per_image = lay.dst_width * lay.dst_height * 8
    chunk = (1 << 30) // per_image
    if geo is KNIFE_X2:
        assert 1 < chunk < GRID_Z
    else:
        assert chunk > GRID_Z
        chunk = GRID_Z
    batch = chunk + 3
    gs, kernel, gd = _batch_against_single_images(gpu, rq, batch, (0, chunk - 1, chunk, chunk + 1, batch - 1))
    print("%s: %d bytes of scratch per image, chunk %d, batch %d, %.2f GB of gdst, %s" % (geo[:2], per_image, chunk, batch, gd.numel() * 4 / 1e9, gpu.plan_shape(rq)))
    assert _flagged(gpu, rq)[0] > 0 and kernel == AXIS_KERNEL + "+listed", (kernel, gpu.plan_shape(rq))
    assert bool((gs >= 0.0).all())                 # every pixel of every image written (weights and gradients are non-negative)
    del gs, gd
    torch.cuda.empty_cache()


def test_planned_adjoint_without_scratch_past_grid_z(gpu):
    """the planned path WITHOUT a list allocates nothing and is cut by grid.z alone: 65,540 images of 24 x 24 (4:1, 0 degrees; the first
    geometry of MATRIX whose call reports no "+listed")"""
    import torch
    for W, H, sr, dr, ang, off, absolute in MATRIX:
        rq = gpu.make_request(W, H, sr, dr, off if absolute else ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1]), ang)
        lay = gpu.query(rq)[2]
        if _planned(gpu, rq, np.ones((lay.dst_height, lay.dst_width), np.float32))[1] == AXIS_KERNEL:
            break
    else:
        pytest.fail("no geometry of MATRIX is served without the correction pass")
    batch = 65540
    # tiny images: if this path took scratch, the 1 GiB rule would not cut before grid.z either
    assert batch > GRID_Z and (1 << 30) // (lay.dst_width * lay.dst_height * 8) > batch
    gs, kernel, gd = _batch_against_single_images(gpu, rq, batch, (0, GRID_Z - 1, GRID_Z, GRID_Z + 1, batch - 1))
    assert kernel == AXIS_KERNEL, (kernel, gpu.plan_shape(rq))
    assert bool((gs >= 0.0).all())
    del gs, gd
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ang", [0.0, 90.0, 180.0, 270.0])
def test_planned_adjoint_stays_inside_its_buffers(gpu, ang):
    """gdst is the guarded SOURCE (NaN around it), gsrc the guarded destination (sentinel everywhere), the three layouts of
    tests/test_gpu_memory_contract.py: every pixel of gsrc inside the image finite and equal, bit for bit, to the tight call; nothing
    else written"""
    import torch
    from test_gpu_memory_contract import LAYOUTS, _pad
    st = torch.cuda.current_stream().cuda_stream
    B = 2
    seen = set()
    for i, (geo, mode) in enumerate(((CLEAN, gpu.MODE_AREA), (KNIFE, gpu.MODE_AREA), (CLEAN, gpu.MODE_FAST))):
        rq = _request(gpu, geo, ang, mode)
        W, H = rq.src_width, rq.src_height
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        g = np.random.default_rng(5 + i).random((B, dH, dW, 1)).astype(np.float32)
        tg = to_device(g)
        ts = torch.full((B, H, W), float("nan"), dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, tg.data_ptr(), dW, ts.data_ptr(), W, st, batch=B, dst_image_stride=dW * dH, src_image_stride=W * H, planned=True)
        torch.cuda.synchronize()
        kernel = gpu.last_kernel()
        flagged, _ = _flagged(gpu, rq)
        assert kernel.startswith(AXIS_KERNEL) and (kernel.endswith("+listed") or flagged == 0), (kernel, flagged)
        seen.add(flagged > 0)
        tight = ts.cpu().numpy().reshape(B, H, W, 1)
        assert np.isfinite(tight).all()
        for sp, so, sg, dp, do, dg in LAYOUTS:
            gl = GuardedLayout((B, dH, dW, 1), "f32", dW + _pad(dW, dp), dH * (dW + _pad(dW, dp)) + dg, do)
            sl = GuardedLayout((B, H, W, 1), "f32", W + _pad(W, sp), H * (W + _pad(W, sp)) + sg, so)
            gdev, sdev = to_device(gl.make_src(g, "nan")), to_device(sl.make_dst())
            gpu.adjoint_device(rq, gl.ptr(gdev), gl.stride, sl.ptr(sdev), sl.stride, st, batch=B, dst_image_stride=gl.image_stride,
                               src_image_stride=sl.image_stride, planned=True)
            torch.cuda.synchronize()
            what = (gpu.last_kernel(), geo, ang, mode, "gdst stride %d image stride %d base %+d, gsrc stride %d image stride %d base %+d"
                    % (gl.stride, gl.image_stride, gl.base_offset, sl.stride, sl.image_stride, sl.base_offset))
            assert gpu.last_kernel() == kernel, what
            out, first, count = sl.check_dst(sdev)
            assert count == 0, ("%d guard elements of gsrc were written, first: %s" % (count, sl.describe(first)), what)
            assert sl.sentinels_left(out) == 0, what
            bad = ~np.isfinite(out)
            assert not bad.any(), ("%d non-finite gsrc pixels, first at %s" % (int(bad.sum()), np.argwhere(bad)[0].tolist()), what)
            assert np.array_equal(out.view(np.int32), tight.view(np.int32)), what
    assert seen == {False, True}


# 7.
def test_torch_operator_with_a_planned_backward(gpu):
    import torch
    from area_average_interpolation_amd import torch_ops
    st = lambda: torch.cuda.current_stream().cuda_stream
    results = []
    for (W, H, sr, dr, ang, mode) in ((160, 120, 4, 1, 0.0, gpu.MODE_AREA), (160, 120, 2.5, 1, 90.0, gpu.MODE_AREA)):
        iso = ((W - 1) / 2, (H - 1) / 2)
        rq = gpu.make_request(W, H, sr, dr, iso, ang, mode=mode)
        lay = gpu.query(rq)[2]
        dW, dH = lay.dst_width, lay.dst_height
        B = 3
        gen = torch.Generator(device="cuda").manual_seed(5)
        x = torch.rand((B, H, W), dtype=torch.float32, device="cuda", generator=gen)
        g = torch.rand((B, dH, dW), dtype=torch.float32, device="cuda", generator=gen)
        kw = dict(batch=B, dst_image_stride=dW * dH, src_image_stride=W * H)
        # the default keyword first: the existing adjoint, and no adjoint tables are built
        xd = x.clone().requires_grad_(True)
        yd, _ = torch_ops.resample(xd, sr, dr, iso, ang, mode=mode)
        (yd * g).sum().backward()
        assert "adjoint=none" in gpu.plan_shape(rq)
        # (aai_last_kernel() is per thread and autograd runs the backward on a thread of its own: the kernels are named by the direct
        # calls below, whose bits the gradients must equal)
        gref = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, g.data_ptr(), dW, gref.data_ptr(), W, st(), **kw)
        assert GATHER_KERNEL in gpu.last_kernel()
        assert torch.equal(xd.grad, gref)
        # planned: the forward builds the tables, the backward is the planned entry
        xp = x.clone().requires_grad_(True)
        yp, _ = torch_ops.resample(xp, sr, dr, iso, ang, mode=mode, planned_backward=True)
        assert "adjoint=tables" in gpu.plan_shape(rq) and torch.equal(yp.detach(), yd.detach())
        (yp * g).sum().backward()
        pref = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
        gpu.adjoint_device(rq, g.data_ptr(), dW, pref.data_ptr(), W, st(), planned=True, **kw)
        assert gpu.last_kernel().startswith(AXIS_KERNEL)
        assert torch.equal(xp.grad, pref)
        results.append((x, g, gref, pref, (sr, dr, iso, ang, mode)))
    # both again in one process, after both plans (and their tables) exist
    for x, g, gref, pref, (sr, dr, iso, ang, mode) in results:
        for planned, want in ((False, gref), (True, pref)):
            xx = x.clone().requires_grad_(True)
            y, _ = torch_ops.resample(xx, sr, dr, iso, ang, mode=mode, planned_backward=planned)
            (y * g).sum().backward()
            assert torch.equal(xx.grad, want), (ang, planned)
        assert float((gref - pref).abs().max()) <= 1e-5 * float(gref.abs().max())
    # no gradient wanted: no tables are built, whatever the keyword says
    W, H = 96, 80
    rq = gpu.make_request(W, H, 2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 180.0)
    torch_ops.resample(torch.rand((H, W), dtype=torch.float32, device="cuda"), 2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 180.0, planned_backward=True)
    assert "adjoint=none" in gpu.plan_shape(rq)


def test_torch_operator_refuses_to_build_adjoint_tables_inside_a_capture(gpu, monkeypatch):
    """with the current stream reported as capturing, an axis geometry that has a plan but no adjoint tables raises instead of building
    them (which would synchronise); once they exist the call goes through"""
    import torch
    from area_average_interpolation_amd import torch_ops
    W, H = 100, 84
    args = (2.0, 1.0, ((W - 1) / 2, (H - 1) / 2), 270.0)                 # a geometry no other test of this module prepares
    rq = gpu.make_request(W, H, *args)
    x = torch.rand((H, W), dtype=torch.float32, device="cuda", requires_grad=True)
    assert gpu.plan_shape(rq) == ""
    eager, _ = torch_ops.resample(x, *args)                              # the forward's plan, no tables
    assert "adjoint=none" in gpu.plan_shape(rq)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        torch_ops.resample(x, *args, planned_backward=True)
    assert "adjoint=none" in gpu.plan_shape(rq)
    torch_ops.resample(x, *args)                                         # the default keyword needs no tables
    torch_ops.resample(x.detach(), *args, planned_backward=True)         # ... and neither does a call that wants no gradient
    monkeypatch.undo()
    torch_ops.resample(x, *args, planned_backward=True)                  # builds the tables outside a capture
    assert "adjoint=tables" in gpu.plan_shape(rq)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    again, _ = torch_ops.resample(x, *args, planned_backward=True)
    torch.cuda.synchronize()
    assert torch.equal(again.detach(), eager.detach())
