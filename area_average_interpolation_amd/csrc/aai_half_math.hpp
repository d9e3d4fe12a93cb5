// aai_half_math.hpp -- the arithmetic of the half-precision path (aai_axis_narrow.hip; include/aai_half.h), shared with the serial CPU replay
// of the test-suite (tests/emulation/half_emulation.cpp): widening of fp16 / bf16 elements, the vertical sum, the horizontal pass and
// the single rounding to the element type.
//
// The contract (include/aai_half.h): every source element is widened exactly to fp32, the forward's own fp32 weights (the K1 tables of
// aai_plan.cpp) are applied, sums are fp32, and the result is rounded ONCE to the element type, round-to-nearest-even.  Every fused
// multiply-add is spelt out (half_fma, like qfma of aai_rot_quad.hpp) and the unit is compiled without contraction (Makefile:
// NOCONTRACT), so that aai_axis_narrow_kernel and the replay execute the same IEEE operations in the same order and agree bit for bit.
//
// The conversions are plain integer C++: they do not depend on a compiler's or a device's half types.  The kernels may use a hardware
// conversion where it gives the same bits (fp16 -> fp32 is exact in hardware too: v_cvt_f32_f16 with fp16 denormals preserved, the
// default; the shift that widens bf16 IS the hardware's way).
#pragma once

#include "aai_rot_math.hpp"

namespace aai {

enum HalfType { HALF_F16 = 1, HALF_BF16 = 2 };      // AAI_HALF_F16 / AAI_HALF_BF16 of include/aai_half.h

AAI_HD uint32_t half_f32_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof u);
    return u;
#endif
}
AAI_HD float half_bits_f32(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
#endif
}

// ---- widening: exact -------------------------------------------------------------------------------------------------------
AAI_HD float bf16_to_f32(uint16_t h) { return half_bits_f32((uint32_t)h << 16); }

AAI_HD float f16_to_f32(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t exp = (h >> 10) & 31u;
    uint32_t man = h & 0x3ffu;
    if (exp == 31u) return half_bits_f32(sign | 0x7f800000u | (man << 13));      // Inf, NaN (payload kept)
    if (exp != 0u) return half_bits_f32(sign | ((exp + 112u) << 23) | (man << 13));
    if (man == 0u) return half_bits_f32(sign);
    // subnormal: man * 2^-24, normalised
    int e = 113;
    while (!(man & 0x400u)) { man <<= 1; --e; }
    return half_bits_f32(sign | ((uint32_t)e << 23) | ((man & 0x3ffu) << 13));
}

// ---- narrowing: ONE rounding, to nearest, ties to even -----------------------------------------------------------------------
// NaN stays NaN (the canonical quiet NaN of the type, sign kept); what rounds beyond the largest finite value is +-Inf.
AAI_HD uint16_t f32_to_bf16(float f)
{
    const uint32_t u = half_f32_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)(((u >> 16) & 0x8000u) | 0x7fc0u);
    // (a carry out of the mantissa moves into the exponent, and from the largest exponent into Inf: both are the right answer)
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

AAI_HD uint16_t f32_to_f16(float f)
{
    const uint32_t u = half_f32_bits(f);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                            // NaN
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                            // >= 65536 (and Inf): Inf
    if (a >= 0x38800000u) {
        // normal range of fp16 (>= 2^-14): rebias, round off 13 bits; 65520 and above carry into Inf
        const uint32_t r = a - 0x38000000u;
        return (uint16_t)(sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13));
    }
    if (a < 0x33000000u) return (uint16_t)sign;      // below 2^-25, half of the smallest subnormal: 0
    // subnormal result: the 24-bit significand shifted right by 14..24 places, a carry into 0x400 is the smallest normal number;
    // 2^-25 itself is a tie between 0 and 2^-24 and goes to the even one, 0
    const uint32_t e = a >> 23;                      // 102 .. 112
    const uint32_t m = (a & 0x7fffffu) | 0x800000u;
    const uint32_t shift = 126u - e;                 // 14 .. 24
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
    return (uint16_t)(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
}

template <int HT> AAI_HD float half_widen(uint16_t h) { return HT == HALF_F16 ? f16_to_f32(h) : bf16_to_f32(h); }
template <int HT> AAI_HD uint16_t half_narrow(float f) { return HT == HALF_F16 ? f32_to_f16(f) : f32_to_bf16(f); }

// ---- one output element -----------------------------------------------------------------------------------------------------
AAI_HD float half_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// the three distinct weights of a table entry (AxisEntry: s0, s1, wFirst, wMid, wLast) at source index y
AAI_HD float half_row_weight(int s0, int s1, float wF, float wM, float wL, int y) { return y == s0 ? wF : (y == s1 ? wL : wM); }

// an entry without weight: a dst row / column off the image.  Its elements are +0 whatever the source holds.
AAI_HD bool half_entry_empty(float wF, float wM, float wL) { return wF == 0.f && wM == 0.f && wL == 0.f; }

// One step of the vertical sum, source rows in ascending order from acc = 0: acc' = w(y) * v + acc, fused.
AAI_HD float half_vertical_step(float acc, float w, float v) { return half_fma(w, v, acc); }

// The horizontal pass over a line of vertical sums: taps line[off] ... line[off + span] (span = s1 - s0),
//   wF * first                                        span == 0
//   fma(wL, last, fma(wM, mid, wF * first))           otherwise, mid = the taps strictly between, summed in ascending order from 0
AAI_HD float half_horizontal(const float *line, int off, int span, float wF, float wM, float wL)
{
    float s = wF * line[off];
    if (span > 0) {
        float mid = 0.f;
        for (int i = 1; i < span; ++i) mid += line[off + i];
        s = half_fma(wL, line[off + span], half_fma(wM, mid, s));
    }
    return s;
}

}  // namespace aai
