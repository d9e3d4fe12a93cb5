// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the narrow-element kernel on fp16 / bf16 images (csrc/aai_axis_narrow.hip:
// aai_axis_narrow_kernel, reported as aai_axis_half_kernel).
//
// Built by tests/half_cases.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_halfemu.so.  The replay itself is
// narrow_replay.hpp's, with one channel and the conversions of csrc/aai_half_math.hpp.  It is not part of the package, is never loaded
// by it, and is not a fallback for anything.
#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "narrow_replay.hpp"

using namespace aai;

template <int HT>
static void replay(const Geometry &g, const AxisTables &t, const uint16_t *src, uint16_t *dst, float *pre)
{
    narrow_replay(g, t, 1, src, dst, pre, [](uint16_t h) { return half_widen<HT>(h); }, [](float v) { return half_narrow<HT>(v); });
}

// facts[0..7] = axis-aligned, wide, transposed, strips, most outputs in a strip, rows share source rows, most source rows of a window,
// the direct kernel's static predicate (the part of aai::axis_narrow_can_serve the tables decide)
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
