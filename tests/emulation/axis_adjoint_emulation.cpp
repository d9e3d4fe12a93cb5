// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the planned adjoint at rotations by multiples of 90 degrees
// (csrc/aai_axis_adjoint.hip and the listed passes of csrc/aai_adjoint.hip behind it).
//
// Built by tests/test_adjoint_planned_host.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_axisadjemu.so.  It
// reuses the PRODUCT's host planner (csrc/aai_plan.cpp: the forward's tables, their inversion, the correction lists), the PRODUCT's
// model check (csrc/aai_axis_verify.hpp, evaluated for every dst pixel: what the plan's scan lists) and the PRODUCT's per-pixel
// bodies of the general adjoint (csrc/aai_adjoint_math.hpp), and sums in the kernel's order with the kernel's fused multiply-adds.
// It is not part of the package, is never loaded by it, and is not a fallback for anything.
#include <cmath>
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_adjoint_math.hpp"
#include "../../area_average_interpolation_amd/csrc/aai_axis_verify.hpp"

using namespace aai;

static float entry_weight(const AxisEntry &e, int s) { return s == e.s0 ? e.wFirst : (s == e.s1 ? e.wLast : e.wMid); }

template <int MODE>
static void listed(const RotLaunch &r, const std::vector<std::pair<int, int>> &srcList, const std::vector<std::pair<int, int>> &dstList,
                   const float *gdst, float *gsrc)
{
    std::vector<double> n((size_t)r.dW * r.dH, std::nan(""));        // (an element outside dstList that is read shows as NaN)
    for (const auto &d : dstList)
        n[(size_t)d.second * r.dW + d.first] = adjoint_normalised<MODE>(r, d.first, d.second, (double)gdst[(size_t)d.second * r.dW + d.first]);
    for (const auto &s : srcList) gsrc[(size_t)s.second * r.W + s.first] = (float)adjoint_gather<MODE>(r, s.first, s.second, n.data());
}

// gdst: dW x dH (dense), gsrc: W x H (dense).  counts[0..2] = flagged dst pixels, listed source pixels, listed dst pixels.
// Returns the library's status code of the geometry, -1 where the planned path does not serve the request (not axis-aligned, wide,
// tables the inversion refuses, a correction list over more than half of the image).
extern "C" int aai_emu_axis_adjoint(const aai_request *rq, const float *gdst, float *gsrc, int *counts)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (!g.axisAligned || (rq->mode != AAI_MODE_AREA && rq->mode != AAI_MODE_FAST)) return -1;
    AxisTables t;
    build_axis_tables(g, rq->mode, t);
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
    // (ka, kb) -> element of gdst: make_axis_launch of csrc/aai_engine.cpp with a dense dst
    const int64_t sa = t.transposed ? g.dW : 1, sb = t.transposed ? 1 : g.dW;
    const int64_t strideA = t.flipA ? -sa : sa, strideB = t.flipB ? -sb : sb;
    const int64_t base = (t.flipA ? (int64_t)(t.nA - 1) * sa : 0) + (t.flipB ? (int64_t)(t.nB - 1) * sb : 0);
    for (int sy = 0; sy < g.H; ++sy)
        for (int sx = 0; sx < g.W; ++sx) {
            float acc = 0.f;
            for (int kb = rows[sy].k0; kb <= rows[sy].k1; ++kb) {
                float tsum = 0.f;
                for (int ka = cols[sx].k0; ka <= cols[sx].k1; ++ka)
                    tsum = std::fmaf(entry_weight(t.lane[ka], sx), gdst[base + ka * strideA + kb * strideB], tsum);
                acc = std::fmaf(entry_weight(t.row[kb], sy), tsum, acc);
            }
            gsrc[(size_t)sy * g.W + sx] = acc;
        }
    if (rq->mode == AAI_MODE_FAST) listed<AAI_MODE_FAST>(r, srcList, dstList, gdst, gsrc);
    else listed<AAI_MODE_AREA>(r, srcList, dstList, gdst, gsrc);
    return AAI_OK;
}
