// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the half-precision kernel (csrc/aai_half.hip: aai_axis_half_kernel).
//
// Built by tests/half_cases.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_halfemu.so.  It reuses the PRODUCT's
// host planner (csrc/aai_plan.cpp: the K1 tables and strips the kernel reads) and the PRODUCT's arithmetic (csrc/aai_half_math.hpp) and
// walks the kernel's work decomposition one strip, one output row and one output after the other: the vertical sums of the strip's
// columns into a line, then every output of the strip from the line.  Same IEEE operations in the same order as the kernel, hence its
// bits.  It is not part of the package, is never loaded by it, and is not a fallback for anything.
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_half_math.hpp"

using namespace aai;

template <int HT>
static void replay(const Geometry &g, const AxisTables &t, const uint16_t *src, uint16_t *dst, float *pre)
{
    const AxisOutMap m = axis_out_map(t, 1, g.dW);
    std::vector<float> line(STRIP_COLS);
    for (const AxisStrip &st : t.strips)
        for (int kb = 0; kb < t.nB; ++kb) {
            const AxisEntry &e = t.row[kb];
            const bool emptyRow = half_entry_empty(e.wFirst, e.wMid, e.wLast);
            if (!emptyRow)
                for (int x = st.x0; x < st.x0 + STRIP_COLS && x < g.W; ++x) {
                    float acc = 0.f;
                    for (int y = e.s0; y <= e.s1; ++y)
                        acc = half_vertical_step(acc, half_row_weight(e.s0, e.s1, e.wFirst, e.wMid, e.wLast, y), half_widen<HT>(src[(size_t)y * g.W + x]));
                    line[x - st.x0] = acc;
                }
            for (int k = st.k0; k < st.k1; ++k) {
                const AxisEntry &c = t.lane[k];
                float v = 0.f;
                if (!emptyRow && !half_entry_empty(c.wFirst, c.wMid, c.wLast)) v = half_horizontal(line.data(), c.s0 - st.x0, c.s1 - c.s0, c.wFirst, c.wMid, c.wLast);
                const int64_t o = m.outBase + (int64_t)k * m.outStrideA + (int64_t)kb * m.outStrideB;
                dst[o] = half_narrow<HT>(v);
                if (pre) pre[o] = v;
            }
        }
}

// facts[0..7] = axis-aligned, wide, transposed, strips, most outputs in a strip, rows share source rows, most source rows of a window,
// the direct kernel's static predicate (the part of aai::axis_half_can_serve the tables decide)
extern "C" int aai_emu_half_facts(const aai_request *rq, int *facts)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    for (int i = 0; i < 8; ++i) facts[i] = 0;
    facts[0] = g.axisAligned && (rq->mode == AAI_MODE_AREA || rq->mode == AAI_MODE_FAST) ? 1 : 0;
    if (!facts[0]) return AAI_OK;
    AxisTables t;
    build_axis_tables(g, rq->mode, t);
    facts[1] = t.wide; facts[2] = t.transposed; facts[3] = (int)t.strips.size(); facts[4] = t.maxOutputsPerStrip;
    facts[5] = t.rowsShared; facts[6] = t.maxRowSpan;
    facts[7] = !t.wide && !t.transposed && g.W >= 4 && t.maxOutputsPerStrip <= 256;
    return AAI_OK;
}

// src: W x H raw 16-bit elements (dense); dst: dW x dH raw elements; pre (may be NULL): the fp32 values before the rounding.
// Returns the library's status code of the geometry, or -1 where the direct kernel does not serve the request.
extern "C" int aai_emu_half_replay(const aai_request *rq, int halfType, const uint16_t *src, uint16_t *dst, float *pre)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (!g.axisAligned || (rq->mode != AAI_MODE_AREA && rq->mode != AAI_MODE_FAST)) return -1;
    AxisTables t;
    build_axis_tables(g, rq->mode, t);
    if (t.wide || t.transposed || g.W < 4) return -1;
    if (halfType == HALF_F16) replay<HALF_F16>(g, t, src, dst, pre);
    else if (halfType == HALF_BF16) replay<HALF_BF16>(g, t, src, dst, pre);
    else return -1;
    return AAI_OK;
}

// the rounding helpers over arrays
extern "C" void aai_emu_f32_to_f16(const float *in, uint16_t *out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = f32_to_f16(in[i]); }
extern "C" void aai_emu_f32_to_bf16(const float *in, uint16_t *out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = f32_to_bf16(in[i]); }
extern "C" void aai_emu_f16_to_f32(const uint16_t *in, float *out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = f16_to_f32(in[i]); }
extern "C" void aai_emu_bf16_to_f32(const uint16_t *in, float *out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = bf16_to_f32(in[i]); }
