// aai_adjoint_plain.hpp -- per-pixel bodies of the planned adjoint at general rotations (aai_adjoint_rotated_*), shared between the HIP
// kernels (aai_adjoint_plain.hip) and the serial CPU replay of the test-suite (tests/emulation/adjoint_plain_emulation.cpp).
//
// The general adjoint (aai_adjoint_math.hpp) pays the knife-edge variant of the per-pair code for every pair, twice: once in the
// normaliser and once in the gather.  Here the forward's own split is applied to it, per plan:
//
//   S[d]  the sum of the weights of dst pixel d, from adjoint_weight_sum_report -- the general normaliser's own function, so S has its
//         bits -- computed once per geometry; pass 1 becomes adjoint_scaled, one division per element.
//   K     the dst pixels with at least one pair that reported a knife edge inside adjoint_pair_weight_report (edgy / edgy2: the pairs
//         whose weight the strict replay decided), listed once per geometry by the same one-off kernel.
//   plain adjoint_plain_gather: adjoint_gather's enumeration, window test and summation order with the per-pair weight from the plain
//         closed forms -- classify_pair<false>, single_cut_area<false>, wedge_pair_area<false>, the plain membership test of the fast
//         mode: no side lists, no strict replay, no knife tests.
//
// Why the bits are the general adjoint's: classify_pair<false> returns the class and the d of classify_pair<true>, the <false> closed
// forms return the area of their <true> forms (KNIFE only adds the edgy reports), and without contraction the fast mode's plain test is
// adjoint_pair_weight's own `in`.  So a pair that reports no edge gets, from the plain forms, bit for bit the weight the general adjoint
// uses; every pair of a dst pixel outside K is such a pair; and a source pixel that no window of a K pixel holds sums only such pairs
// (the gather skips a pair whose window does not hold the virtual pixel), in the general gather's order, times the general pass 1's n.
// The source pixels inside the windows of K pixels (build_adjoint_lists) are recomputed behind the plain gather by the general gather
// itself (aai_adjoint_gather_listed_kernel), which overwrites them.  The translation units that include this header are compiled
// without contraction, like those of aai_adjoint_math.hpp.
#pragma once

#include "aai_adjoint_math.hpp"

namespace aai {

// pass 1 from the plan's sums: the general pass 1's value (adjoint_normalised) given its own sum -- a DIVISION, not a multiplication
// by a reciprocal, so that n has its bits
template <int MODE>
AAI_HD double adjoint_scaled(double sum, double gd)
{
    return adjoint_sum_counts<MODE>(sum) ? gd / sum : 0.0;
}

// weight of the pair (dst pixel centred at (px, py), virtual pixel (X, Y)) from the plain closed forms: what adjoint_pair_weight
// returns for every pair that reports no knife edge
template <int MODE>
AAI_HD double adjoint_plain_pair_weight(const RotLaunch &r, double px, double py, int X, int Y)
{
    const double ex = X - px, ey = Y - py;
    if (MODE == AAI_MODE_FAST) {
        const double lim = r.h + DBL_EPSILON * r.side;
        const double a = fabs(ex * r.c - ey * r.s), b = fabs(ex * r.s + ey * r.c);
        return a <= lim && b <= lim ? 1.0 : 0.0;
    }
    const double a = ex * r.c - ey * r.s, b = ex * r.s + ey * r.c;
    double d = 0.0;
    bool unused = false;
    const int cls = classify_pair<false>(r, a, b, d, unused);
    if (cls == PAIR_OUTSIDE) return 0.0;
    if (cls == PAIR_INSIDE) return 1.0;
    if (cls == PAIR_GENERAL) return wedge_pair_area<false>(r, px - (X - 0.5), py - (Y - 0.5), a < 0.0, b < 0.0, r.policy, unused);
    return single_cut_area<false>(r, d, cls == PAIR_CUT_LR, r.policy, unused);
}

// pass 2: adjoint_gather with the plain per-pair weight -- the same virtual pixels, candidates, window test and order of additions
template <int MODE>
AAI_HD double adjoint_plain_gather(const RotLaunch &r, int sx, int sy, const double *n)
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
                    const double w = adjoint_plain_pair_weight<MODE>(r, px, py, X, Y);
                    if (w != 0.0) acc += w * n[(int64_t)dy * r.dW + dx];
                }
        }
    return acc;
}

// The same two passes for C interleaved channels (aai_adjoint_plain_multi.hip, tests/emulation/adjoint_plain_multi_emulation.cpp): S, K
// and the plain weight of a pair do not depend on the channel, so a pair is enumerated, window-tested and integrated ONCE and each
// channel then costs a load and a multiply-add -- channel c gets the operands adjoint_plain_gather gives plane c, in its order.
// pass 1 per channel is adjoint_scaled<MODE>(S[d], gd[c]) itself: a division per channel.
// pass 2: n has the channels innermost, [dH][dW][C], as in aai_adjoint_multi.hip
template <int MODE, int C>
AAI_HD void adjoint_plain_gather_multi(const RotLaunch &r, int sx, int sy, const double *n, double (&acc)[C])
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
                    const double w = adjoint_plain_pair_weight<MODE>(r, px, py, X, Y);
                    if (w != 0.0) {
                        const double *nd = n + ((int64_t)dy * r.dW + dx) * C;
                        for (int c = 0; c < C; ++c) acc[c] += w * nd[c];
                    }
                }
        }
}

}  // namespace aai
