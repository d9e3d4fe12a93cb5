"""Columns of the oracle's matrix from comb images: per-pixel gold for the adjoint (gsrc = W^T gdst) at sizes where building W
column by column (test_adjoint_host.oracle_matrix: one oracle run per source pixel) is out of reach.

A source image that is 1 at isolated pixels s_k and 0 elsewhere, the s_k farther apart than any dst pixel's window, gives
oracle(comb)[d] = W[d, s_k] for the one s_k that d sees, so

    gold[s_k] = sum over the dst pixels d that see s_k of oracle(comb)[d] * (double)gdst[d]

is the adjoint at s_k from the oracle alone.  A second run with the value k + 1 at s_k assigns every dst pixel to its source
pixel (label = oracle(labels)[d] / oracle(comb)[d]) without any geometry restated here, and proves the spacing: two comb pixels in
one window give a weighted mean of their labels, which the integer check refuses.  Nothing here is chosen by outcome: pixels,
phases and samples are fixed by index and seed before anything is computed, and a failed label check fails the test."""
import math

import numpy as np

from conftest import sample_points

LABEL_EPS = 1e-6


def comb_pitch(lay, ang):
    """a comb pitch (source pixels, odd) from the geometry: the dst pixel's extent along the source axes, side (|cos| + |sin|) virtual
    pixels = that / scale source pixels, plus a margin of 3.  Odd, so that one phase walks through every residue modulo 16.  The
    label check of comb_gold, not this formula, is what guarantees that the pitch was wide enough."""
    th = math.radians(ang % 90.0)
    p = int(math.ceil(lay.side / lay.scale * (abs(math.cos(th)) + abs(math.sin(th))))) + 3
    return p | 1


def edge_phases(W, H, pitch, extra=0):
    """phases (ox, oy) whose combs hold columns 0, 15, 16, 17, W-2, W-1 and rows 0, 15, 16, 17, H-2, H-1 (paired by index), plus `extra`
    diagonal ones; duplicates dropped, order kept"""
    cols, rows = [0, 15, 16, 17, W - 2, W - 1], [0, 15, 16, 17, H - 2, H - 1]
    out = []
    for c, r in list(zip(cols, rows)) + [(3 + 5 * i, 7 + 3 * i) for i in range(extra)]:
        ph = (c % pitch, r % pitch)
        if ph not in out:
            out.append(ph)
    return out


def _labels_to_gold(c, l, g, K, what):
    """c = oracle(comb), l = oracle(labels), g = gdst as float64, all flat over the same dst pixels: (label of every dst pixel, 0 = sees
    no comb pixel; gold per comb pixel)"""
    seen = c != 0.0
    assert not np.any(l[~seen] != 0.0), "%s: a dst pixel has a label and no weight" % what
    lab = l[seen] / c[seen]
    k = np.rint(lab)
    bad = (np.abs(lab - k) > LABEL_EPS) | (k < 1) | (k > K)
    assert not bad.any(), "%s: %d dst pixels see more than one comb pixel (labels %s): the comb is too dense" % (what, int(bad.sum()), lab[bad][:4])
    label = np.zeros(c.shape, np.int64)
    label[seen] = k.astype(np.int64)
    gold = np.bincount(label[seen] - 1, weights=c[seen] * g[seen], minlength=K)
    return label, gold


def comb_gold(po, omode, W, H, sr, dr, iso, ang, policy, gdst, phase, pitch):
    """Full oracle runs (float64 images).  phase = (ox, oy): the comb is 1 at (ox + i pitch, oy + j pitch).  Returns (sx, sy, gold):
    the comb's source pixels and W^T gdst at them in float64."""
    ox, oy = phase
    assert 0 <= ox < pitch and 0 <= oy < pitch
    xs, ys = np.arange(ox, W, pitch), np.arange(oy, H, pitch)
    sy, sx = [a.ravel() for a in np.meshgrid(ys, xs, indexing="ij")]
    K = sx.size
    assert K > 0
    comb, labels = np.zeros((H, W)), np.zeros((H, W))
    comb[sy, sx] = 1.0
    labels[sy, sx] = np.arange(1, K + 1)
    c = po.oracle_run(omode, comb, sr, dr, iso, ang, policy=policy).dst
    l = po.oracle_run(omode, labels, sr, dr, iso, ang, policy=policy).dst
    assert c.shape == np.shape(gdst), (c.shape, np.shape(gdst))
    _, gold = _labels_to_gold(c.ravel(), l.ravel(), np.asarray(gdst, np.float64).ravel(), K, "comb phase %s pitch %d" % (phase, pitch))
    return sx, sy, gold


def comb_cases(po, omode, W, H, sr, dr, iso, ang, policy, gdst, phases, pitch):
    """comb_gold over several phases, concatenated"""
    parts = [comb_gold(po, omode, W, H, sr, dr, iso, ang, policy, gdst, ph, pitch) for ph in phases]
    return [np.concatenate([p[i] for p in parts]) for i in range(3)]


def candidate_radius(lay):
    """source pixels: the dst footprint's half-diagonal plus two source pixels"""
    return lay.side / lay.scale * math.sqrt(0.5) + 2.0


def split_into_combs(sx, sy, radius):
    """Greedy, by index: pixel i goes into the first comb image in which it is farther than 2 radius (+ 1) from every member.  Returns
    a list of index arrays."""
    groups = []
    for i in range(len(sx)):
        for grp in groups:
            m = np.asarray(grp)
            if np.all(np.hypot(sx[m] - sx[i], sy[m] - sy[i]) > 2.0 * radius + 1.0):
                grp.append(i)
                break
        else:
            groups.append([i])
    return [np.asarray(grp) for grp in groups]


def _candidates(rq, lay, sx, sy, radius):
    """dst pixels whose centre (conftest.sample_points) lies within `radius` source pixels of (sx[k], sy[k]): (k, dx, dy, distance),
    flat.  The dst rows to evaluate are located through the affine map that sample_points itself defines (its values at three dst
    pixels), with two rows of margin; the distances that select are sample_points' own."""
    px, py = sample_points(rq, lay, [0, 1], "cpu")
    px, py = px.numpy(), py.numpy()
    o = np.array([px[0, 0], py[0, 0]])
    A = np.array([[px[0, 1] - px[0, 0], px[1, 0] - px[0, 0]], [py[0, 1] - py[0, 0], py[1, 0] - py[0, 0]]])     # source = o + A (dx, dy)
    Ai = np.linalg.inv(A)
    rd = radius * float(np.abs(Ai).sum(axis=1).max()) + 2.0                       # reach in dst pixels along either dst axis
    ks, dxs, dys, dist = [], [], [], []
    for k in range(len(sx)):
        f = Ai @ (np.array([sx[k], sy[k]], np.float64) - o)
        r0, r1 = max(int(math.floor(f[1] - rd)), 0), min(int(math.ceil(f[1] + rd)), lay.dst_height - 1)
        c0, c1 = max(int(math.floor(f[0] - rd)), 0), min(int(math.ceil(f[0] + rd)), lay.dst_width - 1)
        if r0 > r1 or c0 > c1:
            continue
        qx, qy = sample_points(rq, lay, list(range(r0, r1 + 1)), "cpu")
        d = np.hypot(qx.numpy()[:, c0:c1 + 1] - sx[k], qy.numpy()[:, c0:c1 + 1] - sy[k])
        jj, ii = np.nonzero(d <= radius)
        ks.append(np.full(jj.size, k)), dxs.append(ii + c0), dys.append(jj + r0), dist.append(d[jj, ii])
    cat = lambda v, t: np.concatenate(v).astype(t) if v else np.zeros(0, t)
    return cat(ks, np.int64), cat(dxs, np.int32), cat(dys, np.int32), cat(dist, np.float64)


def comb_gold_pixels(po, omode, rq, lay, gdst_at, sx, sy, image=None):
    """The pixel-list form, for images too large for a full oracle run.  (sx[k], sy[k]): the source pixels to evaluate (any order,
    adjacent ones allowed: they are split over several comb images).  gdst_at(dx, dy) -> the fp32 gradient image at those dst pixels.
    `image`: an all-zero fp32 [H, W] array to reuse (it is all zero again on return).  Returns (gold float64 per pixel, number of dst
    pixels the oracle evaluated)."""
    sx, sy = np.asarray(sx, np.int64), np.asarray(sy, np.int64)
    W, H = rq.src_width, rq.src_height
    assert sx.shape == sy.shape and sx.ndim == 1 and np.all((sx >= 0) & (sx < W) & (sy >= 0) & (sy < H))
    assert len(set(zip(sx.tolist(), sy.tolist()))) == sx.size, "a source pixel is listed twice"
    sr, dr, iso, ang, policy = rq.src_res_x, rq.dst_res_x, (rq.src_iso_x, rq.src_iso_y), rq.rotation_deg, rq.policy & 1
    radius = candidate_radius(lay)
    if image is None:
        image = np.zeros((H, W), np.float32)
    gold = np.zeros(sx.size)
    evaluated = 0
    for grp in split_into_combs(sx, sy, radius):
        gx, gy = sx[grp], sy[grp]
        if grp.size > 1:                                                       # pairwise farther apart than twice the radius
            dd = np.hypot(gx[:, None] - gx[None, :], gy[:, None] - gy[None, :]) + np.eye(grp.size) * 1e30
            assert dd.min() > 2.0 * radius
        k, dx, dy, dist = _candidates(rq, lay, gx, gy, radius)
        evaluated += k.size
        if k.size == 0:
            continue
        image[gy, gx] = 1.0
        c = po.oracle_pixels(omode, image, sr, dr, iso, ang, dx, dy, policy=policy)
        image[gy, gx] = np.arange(1, grp.size + 1, dtype=np.float32)
        l = po.oracle_pixels(omode, image, sr, dr, iso, ang, dx, dy, policy=policy)
        image[gy, gx] = 0.0
        label, g = _labels_to_gold(c, l, np.asarray(gdst_at(dx, dy), np.float64), grp.size, "pixel-list comb")
        assert np.all((label == 0) | (label == k + 1)), "a candidate dst pixel sees another comb pixel than its own"
        # the candidates are a superset: the outermost source pixel of the disc holds no weight, so nothing beyond it can
        assert not np.any(c[dist > radius - 1.0] != 0.0), "weight in the outer ring of the candidate disc: the disc is too small"
        gold[grp] = g
    return gold, evaluated
