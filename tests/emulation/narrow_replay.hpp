// TEST INFRASTRUCTURE ONLY -- the serial CPU replay of the narrow-element kernel (csrc/aai_axis_narrow.hip: aai_axis_narrow_kernel), shared
// by half_emulation.cpp (fp16 / bf16, one channel) and int_emulation.cpp (u8 / u16, 1..4 interleaved channels).
//
// It reuses the PRODUCT's host planner (csrc/aai_plan.cpp: the K1 tables and strips the kernel reads, interleaved channels included) and
// the PRODUCT's arithmetic (csrc/aai_int_math.hpp over csrc/aai_half_math.hpp) and walks the kernel's work decomposition one strip, one
// output row and one output after the other: the vertical sums of the strip's elements into a line, then every output of the strip from
// the line.  Same IEEE operations in the same order as the kernel, hence its bits.  The including file has included aai_plan.cpp.
#pragma once

#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_int_math.hpp"

// src: H rows of W * channels elements (dense); dst: dH rows of dW * channels elements; pre (may be NULL): the fp32 values before the
// conversion.  to_float / from_float: the element type's two conversions (aai_half_math.hpp, aai_int_math.hpp); an output without
// weight -- a dst row or column off the image -- is from_float(+0), all bits 0 in every type.
template <typename T, typename ToFloat, typename FromFloat>
static void narrow_replay(const aai::Geometry &g, const aai::AxisTables &t, int channels, const T *src, T *dst, float *pre, ToFloat to_float, FromFloat from_float)
{
    using namespace aai;
    const int rowElems = g.W * channels;
    const AxisOutMap m = axis_out_map(t, channels, (int64_t)g.dW * channels);
    std::vector<float> line(STRIP_COLS);
    for (const AxisStrip &st : t.strips)
        for (int kb = 0; kb < t.nB; ++kb) {
            const AxisEntry &e = t.row[kb];
            const bool emptyRow = half_entry_empty(e.wFirst, e.wMid, e.wLast);
            if (!emptyRow)
                for (int x = st.x0; x < st.x0 + STRIP_COLS && x < rowElems; ++x) {
                    float acc = 0.f;
                    for (int y = e.s0; y <= e.s1; ++y)
                        acc = half_vertical_step(acc, half_row_weight(e.s0, e.s1, e.wFirst, e.wMid, e.wLast, y), to_float(src[(size_t)y * rowElems + x]));
                    line[x - st.x0] = acc;
                }
            for (int k = st.k0; k < st.k1; ++k) {
                const AxisEntry &c = t.lane[k];
                float v = 0.f;
                if (!emptyRow && !half_entry_empty(c.wFirst, c.wMid, c.wLast))
                    v = channels > 1 ? int_horizontal_stepped(line.data(), c.s0 - st.x0, (c.s1 - c.s0) / channels, channels, c.wFirst, c.wMid, c.wLast)
                                     : half_horizontal(line.data(), c.s0 - st.x0, c.s1 - c.s0, c.wFirst, c.wMid, c.wLast);
                const int64_t o = m.outBase + (int64_t)(k / m.outChan) * m.outStrideA + k % m.outChan + (int64_t)kb * m.outStrideB;
                dst[o] = from_float(v);
                if (pre) pre[o] = v;
            }
        }
}
