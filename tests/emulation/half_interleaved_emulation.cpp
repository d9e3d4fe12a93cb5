// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the narrow-element kernel on fp16 / bf16 images of 1..4 interleaved channels
// (csrc/aai_axis_narrow.hip: aai_axis_narrow_kernel, reported as aai_axis_half_kernel; include/aai_half_interleaved.h).
//
// Built by tests/half_interleaved_cases.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_halfilemu.so.  The replay
// itself is narrow_replay.hpp's, with the channel count of the request and the conversions of csrc/aai_half_math.hpp.  It is not part
// of the package, is never loaded by it, and is not a fallback for anything.
#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "narrow_replay.hpp"

using namespace aai;

// the part of aai::axis_narrow_can_serve (with the mode) that the tables decide, for a half image of `channels` channels
static bool direct_serves(const aai_request &rq, const Geometry &g, const AxisTables &t, int channels)
{
    return g.axisAligned && (rq.mode == AAI_MODE_AREA || rq.mode == AAI_MODE_FAST) && !t.wide && !t.transposed && g.W * channels >= 4 &&
           t.maxOutputsPerStrip <= 256;
}

template <int HT>
static void replay(const Geometry &g, const AxisTables &t, int channels, const uint16_t *src, uint16_t *dst, float *pre)
{
    narrow_replay(g, t, channels, src, dst, pre, [](uint16_t h) { return half_widen<HT>(h); }, [](float v) { return half_narrow<HT>(v); });
}

// facts[0..7] = axis-aligned area / fast request, wide, transposed, strips, most outputs in a strip, rows share source rows, most source
// rows of a window, the direct kernel's static predicate
extern "C" int aai_emu_half_interleaved_facts(const aai_request *rq, int channels, int *facts)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    for (int i = 0; i < 8; ++i) facts[i] = 0;
    facts[0] = g.axisAligned && (rq->mode == AAI_MODE_AREA || rq->mode == AAI_MODE_FAST) ? 1 : 0;
    if (!facts[0]) return AAI_OK;
    AxisTables t;
    build_axis_tables(g, rq->mode, t, channels);
    facts[1] = t.wide; facts[2] = t.transposed; facts[3] = (int)t.strips.size(); facts[4] = t.maxOutputsPerStrip;
    facts[5] = t.rowsShared; facts[6] = t.maxRowSpan;
    facts[7] = direct_serves(*rq, g, t, channels);
    return AAI_OK;
}

// src: H rows of W * channels raw 16-bit elements (dense); dst: dH rows of dW * channels elements; pre (may be NULL): the fp32 values
// before the rounding.  Returns the library's status code of the geometry, or -1 where the direct kernel does not serve the request.
extern "C" int aai_emu_half_interleaved_replay(const aai_request *rq, int channels, int halfType, const uint16_t *src, uint16_t *dst, float *pre)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (!g.axisAligned || (rq->mode != AAI_MODE_AREA && rq->mode != AAI_MODE_FAST) || channels < 1 || channels > 4) return -1;
    AxisTables t;
    build_axis_tables(g, rq->mode, t, channels);
    if (!direct_serves(*rq, g, t, channels)) return -1;
    if (halfType == HALF_F16) replay<HALF_F16>(g, t, channels, src, dst, pre);
    else if (halfType == HALF_BF16) replay<HALF_BF16>(g, t, channels, src, dst, pre);
    else return -1;
    return AAI_OK;
}
