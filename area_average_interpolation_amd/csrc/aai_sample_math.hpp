// aai_sample_math.hpp -- the sample point and the cubic weights of the bilinear / bicubic samplers (K4/K5), shared between the forward
// (aai_sample_kernel in aai_rotated.hip), the samplers' adjoint (aai_adjoint_sample_math.hpp) and the CPU replay of the test-suite:
// ONE definition of ix, iy and `outside` (AAI_HD: __host__ __device__ under hipcc, plain inline under g++).
#pragma once

#include "aai_rot_math.hpp"

namespace aai {

AAI_HD void keys(float t, float w[4])
{
    // Every multiply-add spelled out: the planar fast path and the general path (typed sources, interleaved channels) must
    // round these weights alike, whatever the compiler would fuse in either place.
    // In factored form: every weight is a product of terms that fp32 holds to a relative 1e-7, so a weight near its zero (t close to
    // 0 or 1) keeps its RELATIVE accuracy.  The expanded polynomials cancel there (absolute error 1e-7 on a weight of 1e-5), which
    // shows as soon as the tap behind such a weight is orders of magnitude larger than its neighbours (tests/value_domain.py).
    const float a = -0.5f, u = 1.f - t;
    w[0] = (a * t) * (u * u);                                             // a (t^3 - 2 t^2 + t) = a t (1 - t)^2
    w[1] = u * fmaf(-1.5f * t, t, 1.f + t);                               // (a + 2) t^3 - (a + 3) t^2 + 1 = (1 - t) (1 + t - 1.5 t^2)
    w[2] = t * fmaf(-1.5f * u, u, 1.f + u);                               // the same in 1 - t
    w[3] = (a * u) * (t * t);                                             // a (t^2 - t^3) = a t^2 (1 - t)
}

// one sample point: integer tap origin, fractions, and whether it lies outside the image extent
struct SamplePoint { int ix, iy; float tx, ty; bool outside; };

// the sample point of dst pixel (dx, dy) in continuous original-image coordinates: affine in (dx, dy), coefficients from
// the host (the same expression for every caller, so that row bands reproduce the full image bit for bit)
AAI_HD SamplePoint sample_point(const RotLaunch &r, int dx, int dy)
{
    const double ddx = (double)dx, ddy = (double)dy;
    const double sx = fma(ddx, r.sAx, fma(ddy, r.sBx, r.sCx)), sy = fma(ddx, r.sAy, fma(ddy, r.sBy, r.sCy));
    // (a guard of 1e-9 pixels on the extent: points exactly on its edge are inside however the map was rounded)
    const double guard = 1e-9;
    SamplePoint p;
    p.outside = sx < -0.5 - guard || sx > r.W - 0.5 + guard || sy < -0.5 - guard || sy > r.H - 0.5 + guard;
    const double fx = floor(sx), fy = floor(sy);
    p.ix = p.outside ? 0 : (int)fx; p.iy = p.outside ? 0 : (int)fy;
    p.tx = (float)(sx - fx); p.ty = (float)(sy - fy);
    return p;
}

}  // namespace aai
