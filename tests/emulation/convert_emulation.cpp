// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the resample-and-convert kernel (csrc/aai_axis_convert.hip: aai_axis_convert_kernel;
// include/ext/aai_convert.h) and of the forwarding route's last stage (aai_convert_store_kernel).
//
// Built by tests/convert_cases.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_convertemu.so.  The sums s are
// narrow_replay.hpp's `pre`, unchanged: the product's planner and the arithmetic of csrc/aai_int_math.hpp in the kernel's order.  On top:
// v = std::fmaf(s, scale[c], offset[c]), the narrowings of csrc/aai_half_math.hpp, and the planar mapping.  It is not part of the
// package, is never loaded by it, and is not a fallback for anything.
#include <cmath>
#include <cstring>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "narrow_replay.hpp"

using namespace aai;

enum { OUT_F32 = 0, OUT_F16 = 1, OUT_BF16 = 2 };      // AAI_DTYPE_F32 / AAI_HALF_F16 / AAI_HALF_BF16

// the part of aai::axis_convert_can_serve (with the mode) that the tables decide
static bool direct_serves(const aai_request &rq, const Geometry &g, const AxisTables &t, int channels)
{
    return g.axisAligned && (rq.mode == AAI_MODE_AREA || rq.mode == AAI_MODE_FAST) && !t.wide && !t.transposed && g.W * channels >= 4 &&
           t.maxOutputsPerStrip <= 256;
}

// fp32 interleaved [dH][dW][C] -> round(fmaf(s, scale[c], offset[c])) in outType, interleaved [dH][dW][C] or planar [C][dH][dW], dense
static int apply(const float *img, int dW, int dH, int channels, const float *scale, const float *offset, int outType, int planar, void *dst)
{
    if (outType < OUT_F32 || outType > OUT_BF16 || channels < 1 || channels > 4) return -1;
    for (int y = 0; y < dH; ++y)
        for (int x = 0; x < dW; ++x)
            for (int c = 0; c < channels; ++c) {
                const size_t i = ((size_t)y * dW + x) * channels + c;
                const size_t o = planar ? ((size_t)c * dH + y) * dW + x : i;
                const float v = std::fmaf(img[i], scale[c], offset[c]);
                if (outType == OUT_F32) static_cast<float *>(dst)[o] = v;
                else static_cast<uint16_t *>(dst)[o] = outType == OUT_F16 ? half_narrow<HALF_F16>(v) : half_narrow<HALF_BF16>(v);
            }
    return 0;
}

template <typename T>
static void sums(const Geometry &g, const AxisTables &t, int channels, const T *src, float *pre)
{
    std::vector<T> unused((size_t)g.dW * g.dH * channels);
    narrow_replay(g, t, channels, src, unused.data(), pre, [](T e) { return (float)e; }, [](float) { return (T)0; });
}

// facts[0..7] = axis-aligned area / fast request, wide, transposed, strips, most outputs in a strip, rows share source rows, most source
// rows of a window, the direct kernel's static predicate; facts[8..9] = the lane axis / the row axis runs backwards (180 degrees)
extern "C" int aai_emu_convert_facts(const aai_request *rq, int channels, int *facts)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    for (int i = 0; i < 10; ++i) facts[i] = 0;
    facts[0] = g.axisAligned && (rq->mode == AAI_MODE_AREA || rq->mode == AAI_MODE_FAST) ? 1 : 0;
    if (!facts[0]) return AAI_OK;
    AxisTables t;
    build_axis_tables(g, rq->mode, t, channels);
    facts[1] = t.wide; facts[2] = t.transposed; facts[3] = (int)t.strips.size(); facts[4] = t.maxOutputsPerStrip;
    facts[5] = t.rowsShared; facts[6] = t.maxRowSpan;
    facts[7] = direct_serves(*rq, g, t, channels);
    facts[8] = t.flipA; facts[9] = t.flipB;
    return AAI_OK;
}

// src: H rows of W * channels elements (dense), elemBytes 1 or 2; dst: the converted image, dense, interleaved or planar; pre (may be
// NULL): the fp32 sums s, interleaved [dH][dW][C].  Returns the library's status code of the geometry, or -1 where the direct kernel
// does not serve.
extern "C" int aai_emu_convert_replay(const aai_request *rq, int channels, int elemBytes, const void *src, const float *scale, const float *offset, int outType,
                                      int planar, void *dst, float *pre)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (!g.axisAligned || (rq->mode != AAI_MODE_AREA && rq->mode != AAI_MODE_FAST) || channels < 1 || channels > 4) return -1;
    AxisTables t;
    build_axis_tables(g, rq->mode, t, channels);
    if (!direct_serves(*rq, g, t, channels)) return -1;
    std::vector<float> s((size_t)g.dW * g.dH * channels);
    if (elemBytes == 1) sums<unsigned char>(g, t, channels, static_cast<const unsigned char *>(src), s.data());
    else if (elemBytes == 2) sums<unsigned short>(g, t, channels, static_cast<const unsigned short *>(src), s.data());
    else return -1;
    if (pre) std::memcpy(pre, s.data(), s.size() * sizeof(float));
    return apply(s.data(), g.dW, g.dH, channels, scale, offset, outType, planar, dst);
}

// the conversion alone, for the forwarding route: img = the fp32 interleaved output of aai_resample_interleaved_device, dense
extern "C" int aai_emu_convert_apply(const float *img, int dW, int dH, int channels, const float *scale, const float *offset, int outType, int planar, void *dst)
{
    return apply(img, dW, dH, channels, scale, offset, outType, planar, dst);
}
