// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the interleaved planned adjoint at rotations by multiples of 90 degrees
// (csrc/aai_axis_adjoint_multi.hip and the listed passes of csrc/aai_adjoint_plain_multi.hip behind it: launch_adjoint_listed_multi).
//
// Built by tests/test_adjoint_planned_interleaved_host.py with plain g++ (no HIP, no contraction) into
// tests/_build/libaai_axisadjmultiemu.so, like axis_adjoint_emulation.cpp, whose single-channel replay it is compared with bit for
// bit.  It reuses the PRODUCT's host planner (csrc/aai_plan.cpp: the SINGLE-channel tables, their inversion, the correction lists),
// the PRODUCT's model check (csrc/aai_axis_verify.hpp) and the PRODUCT's per-pixel bodies of the general multi-channel adjoint
// (csrc/aai_adjoint_math.hpp: adjoint_normalised_multi, adjoint_gather_multi), and walks a source row in the kernel's order: one
// "lane" per ELEMENT e = sx * C + c, the pixel e / C picking ranges and weights, the channel an address offset, fused multiply-adds,
// ka ascending inside kb ascending.  It is not part of the package, is never loaded by it, and is not a fallback for anything.
#include <cmath>
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_adjoint_math.hpp"
#include "../../area_average_interpolation_amd/csrc/aai_axis_verify.hpp"

using namespace aai;

static float entry_weight(const AxisEntry &e, int s) { return s == e.s0 ? e.wFirst : (s == e.s1 ? e.wLast : e.wMid); }

// launch_adjoint_listed_multi: n is [dH][dW][C]
template <int MODE, int C>
static void listed(const RotLaunch &r, const std::vector<std::pair<int, int>> &srcList, const std::vector<std::pair<int, int>> &dstList,
                   const float *gdst, float *gsrc)
{
    std::vector<double> n((size_t)r.dW * r.dH * C, std::nan(""));    // (an element outside dstList that is read shows as NaN)
    for (const auto &d : dstList) {
        const size_t at = ((size_t)d.second * r.dW + d.first) * C;
        double gd[C], out[C];
        for (int c = 0; c < C; ++c) gd[c] = (double)gdst[at + c];
        adjoint_normalised_multi<MODE, C>(r, d.first, d.second, gd, out);
        for (int c = 0; c < C; ++c) n[at + c] = out[c];
    }
    for (const auto &s : srcList) {
        double acc[C];
        adjoint_gather_multi<MODE, C>(r, s.first, s.second, n.data(), acc);
        for (int c = 0; c < C; ++c) gsrc[((size_t)s.second * r.W + s.first) * C + c] = (float)acc[c];
    }
}

template <int C>
static void replay(const aai_request &rq, const Geometry &g, const AxisTables &t, const std::vector<AxisRange> &cols, const std::vector<AxisRange> &rows,
                   const RotLaunch &r, const std::vector<std::pair<int, int>> &srcList, const std::vector<std::pair<int, int>> &dstList,
                   const float *gdst, float *gsrc)
{
    // (ka, kb) -> the first element of a dst pixel: the engine's mapping (enqueue_adjoint) with a dense dst of dW * C elements a row
    const int64_t dstStride = (int64_t)g.dW * C;
    const int64_t sa = t.transposed ? dstStride : C, sb = t.transposed ? C : dstStride;
    const int64_t strideA = t.flipA ? -sa : sa, strideB = t.flipB ? -sb : sb;
    const int64_t base = (t.flipA ? (int64_t)(t.nA - 1) * sa : 0) + (t.flipB ? (int64_t)(t.nB - 1) * sb : 0);
    const int rowLen = g.W * C;
    for (int sy = 0; sy < g.H; ++sy)
        for (int e = 0; e < rowLen; ++e) {
            const int sx = e / C, ch = e - sx * C;
            float acc = 0.f;
            for (int kb = rows[sy].k0; kb <= rows[sy].k1; ++kb) {
                float tsum = 0.f;
                for (int ka = cols[sx].k0; ka <= cols[sx].k1; ++ka)
                    tsum = std::fmaf(entry_weight(t.lane[ka], sx), gdst[base + ch + ka * strideA + kb * strideB], tsum);
                acc = std::fmaf(entry_weight(t.row[kb], sy), tsum, acc);
            }
            gsrc[(size_t)sy * rowLen + e] = acc;
        }
    if (srcList.empty() || dstList.empty()) return;                  // (the engine's `listed`)
    if (rq.mode == AAI_MODE_FAST) listed<AAI_MODE_FAST, C>(r, srcList, dstList, gdst, gsrc);
    else listed<AAI_MODE_AREA, C>(r, srcList, dstList, gdst, gsrc);
}

// gdst: dH x dW x channels (dense), gsrc: H x W x channels (dense), channels in 2..4.  counts[0..2] = flagged dst pixels, listed source
// pixels, listed dst pixels.  Returns the library's status code of the geometry, -1 where the planned path does not serve the request
// (not axis-aligned, wide, tables the inversion refuses, a correction list over more than half of the image), -2 for a channel count
// outside 2..4.
extern "C" int aai_emu_axis_adjoint_multi(const aai_request *rq, int channels, const float *gdst, float *gsrc, int *counts)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (channels < 2 || channels > 4) return -2;
    if (!g.axisAligned || (rq->mode != AAI_MODE_AREA && rq->mode != AAI_MODE_FAST)) return -1;
    AxisTables t;
    build_axis_tables(g, rq->mode, t);                               // the SINGLE-channel tables
    std::vector<AxisRange> cols, rows;
    if (t.wide || !build_axis_adjoint_ranges(t, g.W, g.H, cols, rows)) return -1;
    const RotLaunch r = make_rot_launch(g, rq->mode, rq->policy);
    std::vector<std::pair<int, int>> flagged, srcList, dstList;
    for (int dy = 0; dy < g.dH; ++dy)
        for (int dx = 0; dx < g.dW; ++dx)
            if (rq->mode == AAI_MODE_FAST ? axis_pixel_differs_fast(r, dx, dy) : axis_pixel_differs(r, dx, dy)) flagged.emplace_back(dx, dy);
    std::vector<int> grazedCols, grazedRows;
    axis_grazed_indices(t.lane, grazedCols);
    axis_grazed_indices(t.row, grazedRows);
    if (!build_adjoint_lists(r, flagged, grazedCols, grazedRows, (size_t)g.W * g.H / 2, srcList, dstList)) return -1;
    counts[0] = (int)flagged.size(); counts[1] = (int)srcList.size(); counts[2] = (int)dstList.size();
    switch (channels) {
    case 2: replay<2>(*rq, g, t, cols, rows, r, srcList, dstList, gdst, gsrc); break;
    case 3: replay<3>(*rq, g, t, cols, rows, r, srcList, dstList, gdst, gsrc); break;
    default: replay<4>(*rq, g, t, cols, rows, r, srcList, dstList, gdst, gsrc); break;
    }
    return AAI_OK;
}
