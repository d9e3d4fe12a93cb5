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
    const float a = -0.5f, t2 = t * t, t3 = t2 * t;
    w[0] = a * (fmaf(-2.f, t2, t3) + t);                                  // a (t^3 - 2 t^2 + t)
    w[1] = fmaf(a + 2.f, t3, fmaf(-(a + 3.f), t2, 1.f));                  // (a + 2) t^3 - (a + 3) t^2 + 1
    w[2] = fmaf(-(a + 2.f), t3, fmaf(2.f * a + 3.f, t2, -(a * t)));       // -(a + 2) t^3 + (2 a + 3) t^2 - a t
    w[3] = a * (t2 - t3);                                                 // a (t^2 - t^3)
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
