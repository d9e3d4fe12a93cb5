// aai_axis_adjoint_half_math.hpp -- the per-lane arithmetic of the half-precision transposed separable kernel
// (aai_axis_adjoint_narrow.hip; include/aai_adjoint_half.h), shared with the serial CPU replay of the test-suite
// (tests/emulation/adjoint_half_emulation.cpp).
//
// One lane owns element e = sx * C + c of a source row and walks the source rows [sy0, sy1) downwards.  It executes, operation for
// operation, what aai_axis_adjoint_multi_kernel<C> (for C = 1: aai_axis_adjoint_kernel) executes for that element on the widened
// gradient: the same table weights, the same fused multiply-adds in the same order (ka ascending inside kb ascending), the horizontal
// sums of the last two kb held in registers.  The two differences are at the ends: every gdst element is widened exactly on load
// (half_widen), and the finished sum is narrowed once on store (half_narrow: to nearest, ties to even; overflow gives +-Inf, NaN the
// type's quiet NaN).  An element no dst pixel reads sums nothing and stores +0.  Hence
//     gsrc = narrow(fp32 kernel(widen(gdst)))     bit for bit,
// by construction.  Every fused multiply-add is spelt out (half_fma) and the unit is compiled without contraction.
#pragma once

#include "aai_half_math.hpp"
#include "aai_plan.hpp"

namespace aai {

// half_widen / half_narrow (aai_half_math.hpp) as this path spells them: the header's integer forms on the host, and on the device the
// hardware conversions aai_axis_narrow.hip already uses for the same bits (fp16: v_cvt_f32_f16, exact, and v_cvt_f16_f32 -- to nearest
// even, overflow to Inf, subnormals kept -- with the header's canonical NaN; bf16: the header's own shift and integer rounding)
template <int HT> AAI_HD float adjoint_half_widen(uint16_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (HT == HALF_F16) return (float)__builtin_bit_cast(_Float16, h);
#endif
    return half_widen<HT>(h);
}
template <int HT> AAI_HD uint16_t adjoint_half_narrow(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (HT == HALF_F16) return f != f ? (uint16_t)(((__float_as_uint(f) >> 16) & 0x8000u) | 0x7e00u) : __builtin_bit_cast(uint16_t, (_Float16)f);
#endif
    return half_narrow<HT>(f);
}

// the weight of source index s within the window of an entry (s0 <= s <= s1): the rule of AxisEntry, s0 == s1 included
AAI_HD float adjoint_half_weight(const AxisEntry &en, int s) { return s == en.s0 ? en.wFirst : (s == en.s1 ? en.wLast : en.wMid); }

// t(kb, sx) of one channel: g = the gdst element of (ka = 0, kb) of that channel; ka ascending
template <int HT>
AAI_HD float adjoint_half_horizontal(const AxisEntry *laneTab, AxisRange c, int sx, const uint16_t *g, int64_t outStrideA)
{
    float t = 0.f;
    for (int ka = c.k0; ka <= c.k1; ++ka)
        t = half_fma(adjoint_half_weight(laneTab[ka], sx), adjoint_half_widen<HT>(g[(int64_t)ka * outStrideA]), t);
    return t;
}

// The lane of element e = sx * C + ch: gd = gdst of this image + outBase + ch, gs = gsrc of this image + e; rows [sy0, sy1).
// Writes gs[sy * srcRowStride] for every row of the range, zeros included, and nothing else.
template <int HT>
AAI_HD void adjoint_half_lane(const AxisEntry *laneTab, const AxisEntry *rowTab, AxisRange c, const AxisRange *rowRange, int sx, int sy0, int sy1,
                              const uint16_t *gd, int64_t outStrideA, int64_t outStrideB, uint16_t *gs, int64_t srcRowStride)
{
    int kOld = -1, kNew = -1;         // the two most recent kb whose horizontal sums are held
    float tOld = 0.f, tNew = 0.f;
    for (int sy = sy0; sy < sy1; ++sy) {
        const AxisRange rr = rowRange[sy];
        float acc = 0.f;
        for (int kb = rr.k0; kb <= rr.k1; ++kb) {
            float t;
            if (kb == kNew) t = tNew;
            else if (kb == kOld) t = tOld;
            else {
                t = adjoint_half_horizontal<HT>(laneTab, c, sx, gd + (int64_t)kb * outStrideB, outStrideA);
                kOld = kNew; tOld = tNew; kNew = kb; tNew = t;
            }
            acc = half_fma(adjoint_half_weight(rowTab[kb], sy), t, acc);
        }
        gs[(int64_t)sy * srcRowStride] = adjoint_half_narrow<HT>(acc);      // (an empty range: no dst pixel reads this element, +0 is written)
    }
}

}  // namespace aai
