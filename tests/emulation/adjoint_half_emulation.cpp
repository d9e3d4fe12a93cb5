// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the half-precision transposed separable kernel
// (csrc/aai_axis_adjoint_narrow.hip: aai_axis_adjoint_half_kernel<HT, C>, the direct route of include/aai_adjoint_half.h).
//
// Built by tests/adjoint_half_cases.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_adjhalfemu.so.  It reuses the
// PRODUCT's host planner (csrc/aai_plan.cpp: the forward's tables and their inversion, build_axis_adjoint_ranges), the PRODUCT's model
// check and list builder (what decides whether a plan has correction lists, and with them whether the direct route serves it) and
// the PRODUCT's per-lane arithmetic (csrc/aai_axis_adjoint_half_math.hpp: adjoint_half_lane, the function the kernel calls), and walks
// the kernel's grid serially: row blocks of 32 source rows, one lane per element of a source row.
// It is not part of the package, is never loaded by it, and is not a fallback for anything.
#include <cstdint>
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_axis_verify.hpp"
#include "../../area_average_interpolation_amd/csrc/aai_axis_adjoint_half_math.hpp"

using namespace aai;

namespace {

constexpr int kRows = 32;      // kAxisAdjHalfRows of the kernel: source rows per workgroup

struct Facts {
    Geometry g;
    AxisTables t;
    std::vector<AxisRange> cols, rows;
    int flagged = 0, srcListed = 0, dstListed = 0;
};

// 0: the direct route serves the request; -1: it does not (not axis-aligned, a sampler, wide, tables the inversion refuses, a plan with
// correction lists or with lists over most of the image); > 0: the library's status code of the geometry
int plan_facts(const aai_request &rq, Facts &f)
{
    std::string msg;
    const int rc = make_geometry(rq, f.g, msg);
    if (rc != AAI_OK) return rc;
    const Geometry &g = f.g;
    if (!g.axisAligned || (rq.mode != AAI_MODE_AREA && rq.mode != AAI_MODE_FAST)) return -1;
    build_axis_tables(g, rq.mode, f.t);
    if (f.t.wide || !build_axis_adjoint_ranges(f.t, g.W, g.H, f.cols, f.rows)) return -1;
    const RotLaunch r = make_rot_launch(g, rq.mode, rq.policy);
    std::vector<std::pair<int, int>> flagged, srcList, dstList;
    for (int dy = 0; dy < g.dH; ++dy)
        for (int dx = 0; dx < g.dW; ++dx)
            if (rq.mode == AAI_MODE_FAST ? axis_pixel_differs_fast(r, dx, dy) : axis_pixel_differs(r, dx, dy)) flagged.emplace_back(dx, dy);
    std::vector<int> grazedCols, grazedRows;
    axis_grazed_indices(f.t.lane, grazedCols);
    axis_grazed_indices(f.t.row, grazedRows);
    if (!flagged.empty() || !grazedCols.empty() || !grazedRows.empty())
        if (!build_adjoint_lists(r, flagged, grazedCols, grazedRows, (size_t)g.W * g.H / 2, srcList, dstList)) return -1;
    f.flagged = (int)flagged.size(); f.srcListed = (int)srcList.size(); f.dstListed = (int)dstList.size();
    return f.srcListed != 0 && f.dstListed != 0 ? -1 : 0;
}

template <int HT>
void replay(const Facts &f, int C, const uint16_t *gdst, uint16_t *gsrc)
{
    const Geometry &g = f.g;
    const AxisTables &t = f.t;
    // (ka, kb) -> the first element of a dst PIXEL: make_axis_adjoint_launch of csrc/aai_engine.cpp with a dense dst
    const int64_t dstStride = (int64_t)g.dW * C, srcStride = (int64_t)g.W * C;
    const int64_t sa = t.transposed ? dstStride : C, sb = t.transposed ? C : dstStride;
    const int64_t strideA = t.flipA ? -sa : sa, strideB = t.flipB ? -sb : sb;
    const int64_t base = (t.flipA ? (int64_t)(t.nA - 1) * sa : 0) + (t.flipB ? (int64_t)(t.nB - 1) * sb : 0);
    for (int sy0 = 0; sy0 < g.H; sy0 += kRows) {
        const int sy1 = sy0 + kRows < g.H ? sy0 + kRows : g.H;
        for (int e = 0; e < g.W * C; ++e) {
            const int sx = e / C, ch = e - sx * C;
            adjoint_half_lane<HT>(t.lane.data(), t.row.data(), f.cols[sx], f.rows.data(), sx, sy0, sy1, gdst + base + ch, strideA, strideB, gsrc + e, srcStride);
        }
    }
}

}  // namespace

// counts[0..2] = flagged dst pixels, listed source pixels, listed dst pixels of the plan.  0: the direct route serves the request.
extern "C" int aai_emu_adjoint_half_facts(const aai_request *rq, int *counts)
{
    Facts f;
    const int rc = plan_facts(*rq, f);
    counts[0] = f.flagged; counts[1] = f.srcListed; counts[2] = f.dstListed;
    return rc;
}

// gdst: dH x dW x C raw 16-bit elements (dense), gsrc: H x W x C (dense).  ht: AAI_HALF_F16 (1) / AAI_HALF_BF16 (2).
extern "C" int aai_emu_adjoint_half(const aai_request *rq, int ht, int channels, const uint16_t *gdst, uint16_t *gsrc)
{
    Facts f;
    const int rc = plan_facts(*rq, f);
    if (rc != 0) return rc;
    if (channels < 1 || channels > 4 || (ht != HALF_F16 && ht != HALF_BF16)) return -2;
    if (ht == HALF_F16) replay<HALF_F16>(f, channels, gdst, gsrc);
    else replay<HALF_BF16>(f, channels, gdst, gsrc);
    return 0;
}
