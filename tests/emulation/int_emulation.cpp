// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the narrow-element kernel on u8 / u16 images (csrc/aai_axis_narrow.hip:
// aai_axis_narrow_kernel, reported as aai_axis_int_kernel).
//
// Built by tests/int_cases.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_intemu.so.  The replay itself is
// narrow_replay.hpp's, with the integer value of an element and the conversion of csrc/aai_int_math.hpp.  It is not part of the
// package, is never loaded by it, and is not a fallback for anything.
#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "narrow_replay.hpp"

using namespace aai;

// the part of aai::axis_narrow_can_serve (with the mode) that the tables decide
static bool direct_serves(const aai_request &rq, const Geometry &g, const AxisTables &t, int channels)
{
    return g.axisAligned && (rq.mode == AAI_MODE_AREA || rq.mode == AAI_MODE_FAST) && !t.wide && !t.transposed && g.W * channels >= 4 &&
           t.maxOutputsPerStrip <= 256;
}

template <typename T>
static void replay(const Geometry &g, const AxisTables &t, int channels, const T *src, T *dst, float *pre)
{
    narrow_replay(g, t, channels, src, dst, pre, [](T e) { return (float)e; }, [](float v) { return int_quantize<T>(v); });
}

// facts[0..7] = axis-aligned area / fast request, wide, transposed, strips, most outputs in a strip, rows share source rows, most source
// rows of a window, the direct kernel's static predicate
extern "C" int aai_emu_int_facts(const aai_request *rq, int channels, int *facts)
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

// src: H rows of W * channels elements (dense), elemBytes 1 or 2; dst: dH rows of dW * channels elements; pre (may be NULL): the fp32
// values before the conversion.  Returns the library's status code of the geometry, or -1 where the direct kernel does not serve.
extern "C" int aai_emu_int_replay(const aai_request *rq, int channels, int elemBytes, const void *src, void *dst, float *pre)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (!g.axisAligned || (rq->mode != AAI_MODE_AREA && rq->mode != AAI_MODE_FAST) || channels < 1 || channels > 4) return -1;
    AxisTables t;
    build_axis_tables(g, rq->mode, t, channels);
    if (!direct_serves(*rq, g, t, channels)) return -1;
    if (elemBytes == 1) replay<unsigned char>(g, t, channels, static_cast<const unsigned char *>(src), static_cast<unsigned char *>(dst), pre);
    else if (elemBytes == 2) replay<unsigned short>(g, t, channels, static_cast<const unsigned short *>(src), static_cast<unsigned short *>(dst), pre);
    else return -1;
    return AAI_OK;
}

// the conversion over arrays
extern "C" void aai_emu_int_quantize_u8(const float *in, unsigned char *out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = int_quantize<unsigned char>(in[i]); }
extern "C" void aai_emu_int_quantize_u16(const float *in, unsigned short *out, size_t n) { for (size_t i = 0; i < n; ++i) out[i] = int_quantize<unsigned short>(in[i]); }
