// aai_adjoint_sample_math.hpp -- the adjoint (transposed) bilinear / bicubic sampler, per source pixel: gsrc = W^T gdst.
//
// The samplers are linear, dst = W src: row d of W holds the tap weights of dst pixel d at its sample point (sample_point() of
// aai_sample_math.hpp, the forward's own): 2 x 2 taps (1 - tx, tx) x (1 - ty, ty), or 4 x 4 Keys taps (a = -0.5, first tap at -1); a
// tap index is clamped into the image, taps that clamp onto one source pixel add up; a dst pixel whose point lies outside the guarded
// extent is a zero row.  The body below is the gather for one SOURCE pixel (X, Y): shared between aai_adjoint_sample.hip and the CPU
// replay of the test-suite (tests/emulation/adjoint_sample_emulation.cpp), compiled without contraction in both.
//
// Candidates.  A dst pixel can only hold a tap on (X, Y) if its sample point lies in the square (X - R, X + R) x (Y - R, Y + R),
// R = 1 (bilinear) or 2 (bicubic) -- edge pixels included: the extent guard keeps every live sample point within 1/2 pixel of an
// edge pixel's centre.  The host inverts the 2 x 2 part of the affine map once (make_adjoint_sample_launch); the lane maps the square
// back into the dst lattice, walks the dy range of that parallelogram and, per row, the dx interval the two strip conditions
// |sx - X| <= R and |sy - Y| <= R allow, padded by one pixel at each end and clipped to the image.  A strip whose dx coefficient is
// (as good as) 0 -- rotations by multiples of 90 degrees -- is a condition on dy alone and is tested, not divided by.  This set is a
// SUPERSET; membership and weight are decided per candidate by the forward's sample_point(): ix, iy and `outside` are the forward's.
//
// Precision.  Fractions, weights, products and the sum are double precision, the result takes ONE fp32 rounding.  fp32 weights are not
// enough: the bicubic lobes cancel, sum |w g| reaches 80 x the result's magnitude, and 80 x 2^-24 x a few operations is the whole
// 1e-5 bar.  Fixed summation order (dy ascending, then dx ascending), no atomics: deterministic, image b of a batch and channel c of
// an interleaved image get the bits of the single-image, single-channel call.
#pragma once

#include "aai_sample_math.hpp"

namespace aai {

struct AdjSampleLaunch {
    RotLaunch r;                // the forward's launch block: sample_point(r, dx, dy)
    double iyx, iyy;            // row of the inverse 2 x 2 map that gives dy: dy = iyx (sx - sCx) + iyy (sy - sCy)
    int flatX, flatY;           // sAx (sAy) is as good as 0: the strip |sx - X| <= R (|sy - Y| <= R) is a condition on dy alone
};

// |coefficient| x dW below this (pixels): the strip does not depend on dx
#define AAI_ADJ_SAMPLE_FLAT 1e-7
// ... and is then tested with this slack
#define AAI_ADJ_SAMPLE_SLACK 1e-6

inline AdjSampleLaunch make_adjoint_sample_launch(const RotLaunch &r)
{
    AdjSampleLaunch a{};
    a.r = r;
    // [sx; sy] = [sAx sBx; sAy sBy] [dx; dy] + [sCx; sCy]: a similarity, its determinant is +-(side / scale)^2 != 0
    const double det = r.sAx * r.sBy - r.sBx * r.sAy;
    a.iyx = -r.sAy / det;
    a.iyy = r.sAx / det;
    a.flatX = fabs(r.sAx) * (double)r.dW < AAI_ADJ_SAMPLE_FLAT ? 1 : 0;
    a.flatY = fabs(r.sAy) * (double)r.dW < AAI_ADJ_SAMPLE_FLAT ? 1 : 0;
    return a;
}

// Keys cubic convolution weights, a = -0.5, in double precision (the expression of the oracle)
AAI_HD void keys_f64(double t, double w[4])
{
    const double a = -0.5, t2 = t * t, t3 = t2 * t;
    w[0] = a * (t3 - 2 * t2 + t);
    w[1] = (a + 2) * t3 - (a + 3) * t2 + 1;
    w[2] = -(a + 2) * t3 + (2 * a + 3) * t2 - a * t;
    w[3] = a * (t2 - t3);
}

// the fractions of sample_point()'s point before their fp32 rounding: the same fused expression, so floor() agrees with ix, iy
AAI_HD void sample_fractions_f64(const RotLaunch &r, int dx, int dy, double &tx, double &ty)
{
    const double ddx = (double)dx, ddy = (double)dy;
    const double sx = fma(ddx, r.sAx, fma(ddy, r.sBx, r.sCx)), sy = fma(ddx, r.sAy, fma(ddy, r.sBy, r.sCy));
    tx = sx - floor(sx); ty = sy - floor(sy);
}

// the weight of dst pixel (dx, dy) on source pixel (X, Y): entry (d, s) of W.  0 for a dst pixel outside the extent.
template <int MODE>
AAI_HD double adjoint_sample_weight(const RotLaunch &r, int dx, int dy, int X, int Y)
{
    constexpr int N = MODE == AAI_MODE_BILINEAR ? 2 : 4, FIRST = MODE == AAI_MODE_BILINEAR ? 0 : -1;
    const SamplePoint p = sample_point(r, dx, dy);
    if (p.outside) return 0.0;
    double tx, ty;
    sample_fractions_f64(r, dx, dy, tx, ty);
    double wx[4], wy[4];
    if (MODE == AAI_MODE_BILINEAR) { wx[0] = 1.0 - tx; wx[1] = tx; wy[0] = 1.0 - ty; wy[1] = ty; wx[2] = wx[3] = wy[2] = wy[3] = 0.0; }
    else { keys_f64(tx, wx); keys_f64(ty, wy); }
    double wX = 0.0, wY = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int cx = p.ix + FIRST + i, cy = p.iy + FIRST + i;
        if ((cx < 0 ? 0 : (cx > r.W - 1 ? r.W - 1 : cx)) == X) wX += wx[i];
        if ((cy < 0 ? 0 : (cy > r.H - 1 ? r.H - 1 : cy)) == Y) wY += wy[i];
    }
    return wX * wY;
}

// a double that may be far outside int's range -> an int in [lo, hi]
AAI_HD int adjoint_sample_clip(double v, int lo, int hi)
{
    return v < (double)lo ? lo : (v > (double)hi ? hi : (int)v);
}

// The dx interval [x0, x1] of dst row dy that one strip allows: |A dx + t| <= R with t = B dy + C - centre.  false: no dx at all.
// (flat: the strip does not depend on dx)
AAI_HD bool adjoint_sample_strip(double A, double t, bool flat, double R, double &lo, double &hi)
{
    if (flat) return fabs(t) <= R + AAI_ADJ_SAMPLE_SLACK;
    const double u = (-R - t) / A, v = (R - t) / A;
    lo = fmax(lo, fmin(u, v));
    hi = fmin(hi, fmax(u, v));
    return true;
}

struct AdjSampleNoVisit { AAI_HD void operator()(int, int) const {} };

// gsrc of source pixel (X, Y), C interleaved channels: acc[c] = sum over the candidates d of W[d][(X, Y)] * gdst[d][c].
// gdst: element (dx, dy, c) at dy * rowStride + dx * C + c.  visit(dx, dy) is called for every candidate (the CPU replay counts them
// and proves the superset property with it; the kernel passes AdjSampleNoVisit).
template <int MODE, int C, typename Visit>
AAI_HD void adjoint_sample_gather(const AdjSampleLaunch &a, int X, int Y, const float *gdst, int64_t rowStride, double (&acc)[C], Visit visit)
{
    const RotLaunch &r = a.r;
    const double R = MODE == AAI_MODE_BILINEAR ? 1.0 : 2.0;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    // the dy range of the square's image in the dst lattice: its centre, and the half height of the parallelogram
    const double cdy = a.iyx * ((double)X - r.sCx) + a.iyy * ((double)Y - r.sCy);
    const double half = R * (fabs(a.iyx) + fabs(a.iyy));
    const int dy0 = adjoint_sample_clip(floor(cdy - half) - 1.0, 0, r.dH - 1), dy1 = adjoint_sample_clip(ceil(cdy + half) + 1.0, 0, r.dH - 1);
    for (int dy = dy0; dy <= dy1; ++dy) {
        const double ddy = (double)dy;
        double lo = 0.0, hi = (double)(r.dW - 1);
        if (!adjoint_sample_strip(r.sAx, ddy * r.sBx + r.sCx - (double)X, a.flatX != 0, R, lo, hi)) continue;
        if (!adjoint_sample_strip(r.sAy, ddy * r.sBy + r.sCy - (double)Y, a.flatY != 0, R, lo, hi)) continue;
        if (!(lo <= hi + 2.0)) continue;             // (the padding below cannot make the interval non-empty)
        const int x0 = adjoint_sample_clip(floor(lo) - 1.0, 0, r.dW - 1), x1 = adjoint_sample_clip(ceil(hi) + 1.0, 0, r.dW - 1);
        const float *row = gdst + (int64_t)dy * rowStride;
        for (int dx = x0; dx <= x1; ++dx) {
            visit(dx, dy);
            const double w = adjoint_sample_weight<MODE>(r, dx, dy, X, Y);
            if (w == 0.0) continue;
            const float *g = row + (int64_t)dx * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += w * (double)g[c];
        }
    }
}

}  // namespace aai
