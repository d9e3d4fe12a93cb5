// aai_adjoint_math.hpp -- per-pixel bodies of the adjoint (transposed) resampling, gsrc = W^T gdst, shared between the HIP
// kernels (aai_adjoint.hip, aai_adjoint_multi.hip) and the serial CPU replays of the test-suite (tests/emulation/adjoint_emulation.cpp,
// adjoint_multi_emulation.cpp).  aai_adjoint_plain.hpp builds the planned adjoint at general rotations on the *_report forms below.
//
// W is the matrix aai_resample_device_f32 applies: W[d, s] = weight(d, s) / (sum over s' of weight(d, s')), where weight is
// the overlap area of dst pixel d with virtual source pixel s (area mode) or the membership of s's centre in d's closed
// square (fast mode), both exactly as the double-precision fix-up pass of the forward evaluates them (aai_rotated_kernel<...,
// STRICT = true>: classify_pair, the closed forms, the strict replay of the reference's classifier at knife edges).  The
// transpose is computed as a gather in two passes so that every element is written once, in a fixed order, without atomics:
//
//   1. adjoint_normalised: one dst pixel.  n[d] = gdst[d] / sum of weights (0 where the forward writes 0).
//   2. adjoint_gather:     one SOURCE pixel.  gsrc[s] = sum over its scale^2 virtual pixels, over the dst pixels d whose
//                          window (rot_window) holds the virtual pixel, of weight(d, s) n[d].
// adjoint_normalised_multi / adjoint_gather_multi are the same two passes for C interleaved channels (aai_adjoint_multi.hip,
// tests/emulation/adjoint_multi_emulation.cpp): the weights do not depend on the channel, so they are computed once per pair.
//
// Both evaluate a pair from the same operands as the forward -- (px, py) from pixel_centre(r, dx, dy), ex = X - px -- and the
// translation units that include this header are compiled without contraction, so a pair gets the same weight whichever
// pass, and whichever direction, asks.  The gather tests a candidate against the forward's own window, so the set of pairs
// is the forward's set too.
//
// Reduced angle 0 (rotations by multiples of 90 degrees) runs through this code too, although make_rot_launch says the area
// kernels only run with s > 0: there r.s == 0, so im1, m2, rs, rLs and r2cs are infinite.  This is RELIED ON, as the fix-up pass
// behind the separable kernel and aai_axis_verify.hpp already rely on it: single_cut_area only takes its trapezoid branch (lo = 0,
// hi = 1), ray_integral's fmax / fmin drop the NaN of 0 x infinity, which only arises with a vertex on a pixel boundary line, and
// exactly those pairs are reported edgy and overruled by the strict replay.  tests/test_adjoint_*.py cover 0 / 90 / 180 degrees
// and the axis-knife geometries; an edit of those helpers has to keep them green.
#pragma once

#include "aai_rot_math.hpp"
#include "aai_strict.hpp"

namespace aai {

// weight of the pair (dst pixel (dx, dy) centred at (px, py), virtual pixel (X, Y)) -- the per-pair code of the forward's
// fix-up pass.  sv4 / haveVertices: the reference's vertices of the dst pixel, fetched on the first knife edge.
// knife: set (never cleared) when the pair reported a knife edge -- edgy / edgy2, i.e. when the strict replay decided its weight.  A pair
// that leaves it alone got the weight of the plain closed forms (adjoint_plain_pair_weight in aai_adjoint_plain.hpp), bit for bit.
template <int MODE>
AAI_HD double adjoint_pair_weight_report(const RotLaunch &r, int dx, int dy, double px, double py, int X, int Y, SVec sv4[4], bool &haveVertices, bool &knife)
{
    const double ex = X - px, ey = Y - py;
    if (MODE == AAI_MODE_FAST) {
        // closed-square membership of the pixel centre with the reference's parameter slack
        const double lim = r.h + DBL_EPSILON * r.side;
        const double a = fabs(ex * r.c - ey * r.s), b = fabs(ex * r.s + ey * r.c);
        bool in = a <= lim && b <= lim;
        const bool edgy = (fabs(a - r.h) < AAI_KNIFE_GUARD && b <= r.h + AAI_KNIFE_GUARD) || (fabs(b - r.h) < AAI_KNIFE_GUARD && a <= r.h + AAI_KNIFE_GUARD);
        if (edgy) {                      // a centre on an edge: the reference's ray cast decides
            knife = true;
            if (!haveVertices) { strict_vertices(r, dx, dy, sv4); haveVertices = true; }
            SVec pc; pc.x = X; pc.y = Y;
            in = strict_centre_inside(pc, sv4);
        }
        return in ? 1.0 : 0.0;
    }
    const double a = ex * r.c - ey * r.s, b = ex * r.s + ey * r.c;
    double d = 0.0, w = 0.0;
    bool edgy = false, edgy2 = false;
    const int cls = classify_pair<true>(r, a, b, d, edgy);
    if (cls != PAIR_OUTSIDE) {
        if (cls == PAIR_INSIDE) w = 1.0;
        else if (cls == PAIR_GENERAL) w = wedge_pair_area<true>(r, px - (X - 0.5), py - (Y - 0.5), a < 0.0, b < 0.0, r.policy, edgy2);
        else w = single_cut_area<true>(r, d, cls == PAIR_CUT_LR, r.policy, edgy2);
        if (edgy || edgy2) {
            knife = true;
            if (!haveVertices) { strict_vertices(r, dx, dy, sv4); haveVertices = true; }
            w = strict_pair_area(sv4, X, Y, r.policy);
        }
    }
    return w;
}

template <int MODE>
AAI_HD double adjoint_pair_weight(const RotLaunch &r, int dx, int dy, double px, double py, int X, int Y, SVec sv4[4], bool &haveVertices)
{
    bool knife = false;
    return adjoint_pair_weight_report<MODE>(r, dx, dy, px, py, X, Y, sv4, haveVertices, knife);
}

// the sum of the weights of dst pixel (dx, dy) over its window, row by row: pass 1's denominator, the same for every channel
// (knife: whether any pair of the window reported a knife edge -- the per-plan table of the rotated planned adjoint lists these pixels)
template <int MODE>
AAI_HD double adjoint_weight_sum_report(const RotLaunch &r, int dx, int dy, bool &knife)
{
    double px, py;
    pixel_centre(r, dx, dy, px, py);
    int x0, x1, y0, y1;
    rot_window(r, px, py, x0, x1, y0, y1);
    SVec sv4[4];
    bool haveVertices = false;
    double sum = 0.0;
    for (int Y = y0; Y <= y1; ++Y)
        for (int X = x0; X <= x1; ++X) sum += adjoint_pair_weight_report<MODE>(r, dx, dy, px, py, X, Y, sv4, haveVertices, knife);
    return sum;
}
template <int MODE>
AAI_HD double adjoint_weight_sum(const RotLaunch &r, int dx, int dy)
{
    bool knife = false;
    return adjoint_weight_sum_report<MODE>(r, dx, dy, knife);
}

// whether the forward divides by this sum (it writes 0 otherwise: Source.cpp:577 / 905)
template <int MODE>
AAI_HD bool adjoint_sum_counts(double sum) { return MODE == AAI_MODE_FAST ? sum > 0.0 : DBL_EPSILON < fabs(sum); }

// pass 1: gd / (sum of the weights of dst pixel (dx, dy)), 0 where the forward writes 0 (Source.cpp:577 / 905)
template <int MODE>
AAI_HD double adjoint_normalised(const RotLaunch &r, int dx, int dy, double gd)
{
    const double sum = adjoint_weight_sum<MODE>(r, dx, dy);
    const bool any = adjoint_sum_counts<MODE>(sum);
    return any ? gd / sum : 0.0;
}

// pass 1 for C interleaved channels: the sum once, then a DIVISION per channel (not a multiplication by the reciprocal), so that
// channel c gets the bits adjoint_normalised gives plane c
template <int MODE, int C>
AAI_HD void adjoint_normalised_multi(const RotLaunch &r, int dx, int dy, const double (&gd)[C], double (&out)[C])
{
    const double sum = adjoint_weight_sum<MODE>(r, dx, dy);
    const bool any = adjoint_sum_counts<MODE>(sum);
    for (int c = 0; c < C; ++c) out[c] = any ? gd[c] / sum : 0.0;
}

// How far (in dst pixels, along either dst axis) the centre of a dst pixel can lie from a virtual pixel whose weight is not 0:
// the pixel's centre is within h + k of the square's centre along both dst axes (classify_pair; fast mode: within h), the
// knife guard and the rounding of the inverse map (~1e-11 on coordinates up to 2^31) are covered by 1e-6.
AAI_HD double adjoint_reach(const RotLaunch &r) { return (r.h + r.k + 1e-6) / r.side; }

// virtual pixel (X, Y) of the lattice that replicates source pixel (sx, sy) at sub-position (jx, jy), 0 <= j < scale:
// the inverse of virt_offset's quadrant mapping
AAI_HD void adjoint_virtual_pixel(const RotLaunch &r, int sx, int sy, int jx, int jy, int &X, int &Y)
{
    const int vx = sx * r.scale + jx, vy = sy * r.scale + jy;
    switch (r.quadrant) {
    default:
    case 0: X = vx;            Y = vy;            break;
    case 1: X = r.mW - 1 - vy; Y = vx;            break;
    case 2: X = r.mW - 1 - vx; Y = r.mH - 1 - vy; break;
    case 3: X = vy;            Y = r.mH - 1 - vx; break;
    }
}

// the dst pixels [dxa, dxb] x [dya, dyb] whose window can hold virtual pixel (X, Y) (false: none); R = adjoint_reach(r), rL = 1 / side.
// (Shared with the host, which lists the dst pixels a listed gather reads: aai_plan.cpp, build_adjoint_lists.)
AAI_HD bool adjoint_candidates(const RotLaunch &r, int X, int Y, double R, double rL, int &dxa, int &dxb, int &dya, int &dyb)
{
    // (X, Y) in the dst lattice: the inverse of pixel_centre, px = cXa dx + cXb dy + cX0 with (cXa, cXb) = side (cs, sn),
    // py = cYa dx + cYb dy + cY0 with (cYa, cYb) = side (-sn, cs)
    const double u = X - r.cX0, v = Y - r.cY0;
    const double fx = (u * r.cs - v * r.sn) * rL, fy = (u * r.sn + v * r.cs) * rL;
    // clamp in double before converting
    const double xa = fmax(ceil(fx - R), 0.0), xb = fmin(floor(fx + R), (double)(r.dW - 1));
    const double ya = fmax(ceil(fy - R), 0.0), yb = fmin(floor(fy + R), (double)(r.dH - 1));
    if (!(xa <= xb) || !(ya <= yb)) return false;
    dxa = (int)xa; dxb = (int)xb; dya = (int)ya; dyb = (int)yb;
    return true;
}

// pass 2: the gradient of source pixel (sx, sy); n = pass 1's image of this batch entry, dW elements per row
template <int MODE>
AAI_HD double adjoint_gather(const RotLaunch &r, int sx, int sy, const double *n)
{
    const double R = adjoint_reach(r), rL = 1.0 / r.side;
    double acc = 0.0;
    for (int jy = 0; jy < r.scale; ++jy)
        for (int jx = 0; jx < r.scale; ++jx) {
            int X, Y;
            adjoint_virtual_pixel(r, sx, sy, jx, jy, X, Y);
            int dxa, dxb, dya, dyb;
            if (!adjoint_candidates(r, X, Y, R, rL, dxa, dxb, dya, dyb)) continue;
            for (int dy = dya; dy <= dyb; ++dy)
                for (int dx = dxa; dx <= dxb; ++dx) {
                    double px, py;
                    pixel_centre(r, dx, dy, px, py);
                    int x0, x1, y0, y1;
                    rot_window(r, px, py, x0, x1, y0, y1);
                    if (X < x0 || X > x1 || Y < y0 || Y > y1) continue;          // the forward does not visit this pair
                    SVec sv4[4];
                    bool haveVertices = false;
                    const double w = adjoint_pair_weight<MODE>(r, dx, dy, px, py, X, Y, sv4, haveVertices);
                    if (w != 0.0) acc += w * n[(int64_t)dy * r.dW + dx];
                }
        }
    return acc;
}

// pass 2 for C interleaved channels: adjoint_gather's enumeration, window test and weight, once per pair; n = pass 1's image of
// this batch entry with the channels innermost ([dH][dW][C]), so that channel c sums the terms of plane c in plane c's order
template <int MODE, int C>
AAI_HD void adjoint_gather_multi(const RotLaunch &r, int sx, int sy, const double *n, double (&acc)[C])
{
    const double R = adjoint_reach(r), rL = 1.0 / r.side;
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int jy = 0; jy < r.scale; ++jy)
        for (int jx = 0; jx < r.scale; ++jx) {
            int X, Y;
            adjoint_virtual_pixel(r, sx, sy, jx, jy, X, Y);
            int dxa, dxb, dya, dyb;
            if (!adjoint_candidates(r, X, Y, R, rL, dxa, dxb, dya, dyb)) continue;
            for (int dy = dya; dy <= dyb; ++dy)
                for (int dx = dxa; dx <= dxb; ++dx) {
                    double px, py;
                    pixel_centre(r, dx, dy, px, py);
                    int x0, x1, y0, y1;
                    rot_window(r, px, py, x0, x1, y0, y1);
                    if (X < x0 || X > x1 || Y < y0 || Y > y1) continue;          // the forward does not visit this pair
                    SVec sv4[4];
                    bool haveVertices = false;
                    const double w = adjoint_pair_weight<MODE>(r, dx, dy, px, py, X, Y, sv4, haveVertices);
                    if (w != 0.0) {
                        const double *nd = n + ((int64_t)dy * r.dW + dx) * C;
                        for (int c = 0; c < C; ++c) acc[c] += w * nd[c];
                    }
                }
        }
}

}  // namespace aai
