"""Cases, gold and the bar of the samplers' adjoint (gsrc = W^T gdst, bilinear / bicubic), shared by tests/test_adjoint_sample_host.py and
tests/test_adjoint_sample_gpu.py.  Gold comes from the oracle alone: its matrix on unit impulses (modes 3 / 4) at small sizes, columns
of it from comb images (tests/adjoint_columns.py) at mid sizes.  Every gold is computed once per session and never modified."""
import functools

import numpy as np

from conftest import TOL, rel_err
from test_adjoint_host import EIGHT, oracle_matrix

OMODE = {3: 3, 4: 4}          # library mode -> oracle mode (AAI_ORACLE_MODE_BILINEAR / _BICUBIC)
MODES = (3, 4)                # MODE_BILINEAR, MODE_BICUBIC
MODE_NAME = {3: "bilinear", 4: "bicubic"}

# (W, H, srcRes, dstRes, angle, isocentre offset from the image centre): single rows / columns / pixels, every tap clamped; a 90
# degree map (a strip coefficient of 0); a long thin image just off an axis
DEGENERATE = [(1, 6, 1, 1, 0, (0, 0)), (5, 1, 1, 2, 30, (0, 0)), (1, 1, 1, 3, 45, (0, 0)), (2, 2, 1, 4, 72, (.25, -.25)),
              (7, 3, 3, 1, 303, (0, 0)), (9, 8, 1, 1, 90, (0, 0)), (33, 5, 1.3, 1, 359, (1, 0))]
MATRIX_CASES = list(EIGHT) + DEGENERATE

# (W, H, srcRes, dstRes, angle), isocentre at the image centre; comb pitch 7
COMB_CASES = [(150, 130, 2.5, 1, 17.5), (70, 50, 1, 2, 30), (130, 150, 3, 1, 270)]
COMB_PITCH = 7


def iso_of(W, H, off=(0, 0)):
    return ((W - 1) / 2 + off[0], (H - 1) / 2 + off[1])


def comb_phases(W, H):
    out = []
    for ph in ((0, 0), (1, 1), (2, 2), (3, 3), (6, 6), ((W - 1) % COMB_PITCH, (H - 1) % COMB_PITCH)):
        if ph not in out:
            out.append(ph)
    return out


def assert_sample_adjoint_matches(got, gold, what):
    """the bar of DESIGN.md section 9: every source pixel within TOL of gold relative to max(|gold|, 1e-3 max|gold|).  No exact-zero
    clause: the oracle's own matrix holds weights below 1e-12 where a fraction that should be 0 comes out as 1e-16."""
    gold = np.asarray(gold, np.float64)
    floor = 1e-3 * float(np.abs(gold).max())
    err = rel_err(got, gold, floor=floor if floor > 0 else 1e-300)
    print("%s: max rel err %.3e" % (what, float(err.max())))
    assert np.all(np.isfinite(np.asarray(got, np.float64))), what
    assert float(err.max()) <= TOL, (what, float(err.max()))


@functools.lru_cache(maxsize=None)
def _matrix_gold(case, mode):
    from oracle import pyoracle as po
    import area_average_interpolation_amd as aai
    W, H, sr, dr, ang, off = MATRIX_CASES[case]
    iso = iso_of(W, H, off)
    M = oracle_matrix(po, OMODE[mode], W, H, sr, dr, iso, ang)
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    rc, msg, lay = aai.query(rq)
    assert rc == 0 and M.shape == (lay.dst_width * lay.dst_height, W * H), msg
    # gradients of either sign: the cubic's lobes and the gradient's sign both cancel
    g = (np.random.default_rng(7 + case).random(M.shape[0]) - 0.25).astype(np.float32)
    gold = (M.T @ g.astype(np.float64)).reshape(H, W)
    g = g.reshape(lay.dst_height, lay.dst_width)
    g.setflags(write=False), gold.setflags(write=False), M.setflags(write=False)
    return rq, g, gold, M


def matrix_gold(po, aai, case, mode):
    """(request, gdst fp32 [dH, dW], W^T gdst float64 [H, W], W) of MATRIX_CASES[case]; po / aai: the session fixtures (built by now)"""
    return _matrix_gold(case, mode)


@functools.lru_cache(maxsize=None)
def _comb_gold(case, mode):
    from oracle import pyoracle as po
    import area_average_interpolation_amd as aai
    from adjoint_columns import comb_cases
    W, H, sr, dr, ang = COMB_CASES[case]
    iso = iso_of(W, H)
    rq = aai.make_request(W, H, sr, dr, iso, ang, mode=mode)
    rc, msg, lay = aai.query(rq)
    assert rc == 0, msg
    g = (np.random.default_rng(11 + case).random((lay.dst_height, lay.dst_width)) - 0.25).astype(np.float32)
    sx, sy, gold = comb_cases(po, OMODE[mode], W, H, sr, dr, iso, ang, 0, g, comb_phases(W, H), COMB_PITCH)
    assert (sx == 0).any() and (sy == 0).any() and (sx == W - 1).any() and (sy == H - 1).any()
    for a in (g, sx, sy, gold):
        a.setflags(write=False)
    return rq, g, sx, sy, gold


def comb_gold(po, aai, case, mode):
    """(request, gdst fp32, sx, sy, gold at (sx, sy)) of COMB_CASES[case]"""
    return _comb_gold(case, mode)
