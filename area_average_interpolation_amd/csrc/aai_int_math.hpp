// aai_int_math.hpp -- the arithmetic of the integer path (aai_axis_narrow.hip; include/aai_int.h), shared with the serial CPU replay of the
// test-suite (tests/emulation/int_emulation.cpp): the vertical sum and the single-channel horizontal pass are aai_half_math.hpp's,
// unchanged; this header adds the horizontal pass over interleaved channels (taps `step` elements apart) and the single conversion of
// an fp32 sum to an 8- or 16-bit unsigned element.
//
// The contract (include/aai_int.h): every source element is used as its integer value (exact in fp32: at most 16 bits), the forward's
// own fp32 weights (the K1 tables of aai_plan.cpp) are applied, sums are fp32, and the result is converted ONCE: rounded to the nearest
// integer, ties to even, then saturated to the range of the type.  Every fused multiply-add is spelt out (half_fma) and the unit is
// compiled without contraction (Makefile: NOCONTRACT), so that aai_axis_narrow_kernel and the replay execute the same IEEE operations in
// the same order and agree bit for bit.
#pragma once

#include "aai_half_math.hpp"

namespace aai {

template <typename T> struct IntRange;
template <> struct IntRange<unsigned char> { static constexpr float max = 255.f; };
template <> struct IntRange<unsigned short> { static constexpr float max = 65535.f; };

// ---- the conversion: ONE rounding, to nearest, ties to even, then saturation ------------------------------------------------------
// NaN, -Inf and everything at or below 0.5 give 0; +Inf and everything at or above the maximum give the maximum.  Between them the
// value lies in (0, 65535): rintf under the default rounding mode (the device's v_rndne_f32) rounds it to the nearest integer, ties
// to even, and the integer converts exactly.
template <typename T> AAI_HD T int_quantize(float s)
{
    if (!(s > 0.f)) return (T)0;                                  // NaN, -Inf, negatives, both zeros
    if (s >= IntRange<T>::max) return (T)IntRange<T>::max;        // +Inf and what saturates
    return (T)(unsigned)__builtin_rintf(s);
}

// ---- one output element over interleaved channels ---------------------------------------------------------------------------------
// half_horizontal with the taps `step` elements apart: taps line[off], line[off + step] ... line[off + span * step] (span = taps - 1),
//   wF * first                                        span == 0
//   fma(wL, last, fma(wM, mid, wF * first))           otherwise, mid = the taps strictly between, summed in ascending order from 0
AAI_HD float int_horizontal_stepped(const float *line, int off, int span, int step, float wF, float wM, float wL)
{
    float s = wF * line[off];
    if (span > 0) {
        float mid = 0.f;
        for (int i = 1; i < span; ++i) mid += line[off + i * step];
        s = half_fma(wL, line[off + span * step], half_fma(wM, mid, s));
    }
    return s;
}

}  // namespace aai
