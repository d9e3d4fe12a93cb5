// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the integer kernel (csrc/aai_int.hip: aai_axis_int_kernel).
//
// Built by tests/int_cases.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_intemu.so.  It reuses the PRODUCT's
// host planner (csrc/aai_plan.cpp: the K1 tables and strips the kernel reads, interleaved channels included) and the PRODUCT's
// arithmetic (csrc/aai_int_math.hpp over csrc/aai_half_math.hpp) and walks the kernel's work decomposition one strip, one output row and
// one output after the other: the vertical sums of the strip's elements into a line, then every output of the strip from the line.
// Same IEEE operations in the same order as the kernel, hence its bits.  It is not part of the package, is never loaded by it, and is
// not a fallback for anything.
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_int_math.hpp"

using namespace aai;

// the part of aai::axis_int_can_serve (with the mode) that the tables decide
static bool direct_serves(const aai_request &rq, const Geometry &g, const AxisTables &t, int channels)
{
    return g.axisAligned && (rq.mode == AAI_MODE_AREA || rq.mode == AAI_MODE_FAST) && !t.wide && !t.transposed && g.W * channels >= 4 &&
           t.maxOutputsPerStrip <= 256;
}

template <typename T>
static void replay(const Geometry &g, const AxisTables &t, int channels, const T *src, T *dst, float *pre)
{
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
                        acc = half_vertical_step(acc, half_row_weight(e.s0, e.s1, e.wFirst, e.wMid, e.wLast, y), (float)src[(size_t)y * rowElems + x]);
                    line[x - st.x0] = acc;
                }
            for (int k = st.k0; k < st.k1; ++k) {
                const AxisEntry &c = t.lane[k];
                float v = 0.f;
                bool live = false;
                if (!emptyRow && !half_entry_empty(c.wFirst, c.wMid, c.wLast)) {
                    live = true;
                    v = channels > 1 ? int_horizontal_stepped(line.data(), c.s0 - st.x0, (c.s1 - c.s0) / channels, channels, c.wFirst, c.wMid, c.wLast)
                                     : half_horizontal(line.data(), c.s0 - st.x0, c.s1 - c.s0, c.wFirst, c.wMid, c.wLast);
                }
                const int64_t o = m.outBase + (int64_t)(k / m.outChan) * m.outStrideA + k % m.outChan + (int64_t)kb * m.outStrideB;
                dst[o] = live ? int_quantize<T>(v) : (T)0;
                if (pre) pre[o] = v;
            }
        }
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
