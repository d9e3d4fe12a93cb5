// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the planned adjoint at general rotations (aai_adjoint_rotated_*: csrc/aai_engine.cpp
// build_rot_adjoint_tables / enqueue_adjoint, the ROTATED family; csrc/aai_adjoint_plain.hip).
//
// Built by tests/test_adjoint_rotated_host.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_adjplainemu.so.  It
// reuses the PRODUCT's host planner (csrc/aai_plan.cpp: build_adjoint_lists) and the PRODUCT's per-pixel bodies
// (csrc/aai_adjoint_math.hpp, csrc/aai_adjoint_plain.hpp) and runs the plan's tables and the call's passes one pixel after the other:
// S and K, the source list, the element-wise pass 1, the plain gather, the listed overwrite -- and the general adjoint whole where the
// engine would keep it.  It also checks the set K against its definition by a direct loop over all pairs.  Not part of the package,
// never loaded by it, not a fallback for anything.
#include <utility>
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_adjoint_plain.hpp"

using namespace aai;

// does the pair report a knife edge?  Written out from the definition: the reports of classify_pair<true> and of the <true> closed
// forms in area mode, the guard test of the centre's membership in fast mode
template <int MODE>
static bool pair_reports_knife(const RotLaunch &r, double px, double py, int X, int Y)
{
    const double ex = X - px, ey = Y - py;
    if (MODE == AAI_MODE_FAST) {
        const double a = fabs(ex * r.c - ey * r.s), b = fabs(ex * r.s + ey * r.c);
        return (fabs(a - r.h) < AAI_KNIFE_GUARD && b <= r.h + AAI_KNIFE_GUARD) || (fabs(b - r.h) < AAI_KNIFE_GUARD && a <= r.h + AAI_KNIFE_GUARD);
    }
    const double a = ex * r.c - ey * r.s, b = ex * r.s + ey * r.c;
    double d = 0.0;
    bool edgy = false, edgy2 = false;
    const int cls = classify_pair<true>(r, a, b, d, edgy);
    if (cls == PAIR_OUTSIDE) return false;
    if (cls == PAIR_GENERAL) (void)wedge_pair_area<true>(r, px - (X - 0.5), py - (Y - 0.5), a < 0.0, b < 0.0, r.policy, edgy2);
    else if (cls != PAIR_INSIDE) (void)single_cut_area<true>(r, d, cls == PAIR_CUT_LR, r.policy, edgy2);
    return edgy || edgy2;
}

// counts: [0] pixels of K, [1] listed source pixels, [2] 1 when the general adjoint served the geometry, [3] dst pixels whose membership
// of K differs from the definition
template <int MODE>
static void run(const RotLaunch &r, const float *gdst, float *gsrc, unsigned maxListed, long *counts)
{
    const size_t N = (size_t)r.dW * r.dH;
    std::vector<double> S(N), n(N);
    std::vector<std::pair<int, int>> K, srcList, dstList;
    long wrong = 0;
    for (int dy = 0; dy < r.dH; ++dy)
        for (int dx = 0; dx < r.dW; ++dx) {
            bool knife = false;
            S[(size_t)dy * r.dW + dx] = adjoint_weight_sum_report<MODE>(r, dx, dy, knife);
            if (knife) K.emplace_back(dx, dy);
            double px, py;
            pixel_centre(r, dx, dy, px, py);
            int x0, x1, y0, y1;
            rot_window(r, px, py, x0, x1, y0, y1);
            bool byDefinition = false;
            for (int Y = y0; Y <= y1; ++Y)
                for (int X = x0; X <= x1; ++X) byDefinition = pair_reports_knife<MODE>(r, px, py, X, Y) || byDefinition;
            wrong += byDefinition != knife;
        }
    bool general = K.size() > (size_t)maxListed;
    if (!general && !build_adjoint_lists(r, K, std::vector<int>(), std::vector<int>(), (size_t)r.W * r.H / 2, srcList, dstList)) general = true;
    counts[0] = (long)K.size(); counts[1] = general ? 0 : (long)srcList.size(); counts[2] = general ? 1 : 0; counts[3] = wrong;
    if (general) {
        for (int dy = 0; dy < r.dH; ++dy)
            for (int dx = 0; dx < r.dW; ++dx) n[(size_t)dy * r.dW + dx] = adjoint_normalised<MODE>(r, dx, dy, (double)gdst[(size_t)dy * r.dW + dx]);
        for (int sy = 0; sy < r.H; ++sy)
            for (int sx = 0; sx < r.W; ++sx) gsrc[(size_t)sy * r.W + sx] = (float)adjoint_gather<MODE>(r, sx, sy, n.data());
        return;
    }
    for (size_t i = 0; i < N; ++i) n[i] = adjoint_scaled<MODE>(S[i], (double)gdst[i]);
    for (int sy = 0; sy < r.H; ++sy)
        for (int sx = 0; sx < r.W; ++sx) gsrc[(size_t)sy * r.W + sx] = (float)adjoint_plain_gather<MODE>(r, sx, sy, n.data());
    for (const auto &s : srcList) gsrc[(size_t)s.second * r.W + s.first] = (float)adjoint_gather<MODE>(r, s.first, s.second, n.data());
}

// gdst: dW x dH (dense), gsrc: W x H (dense), counts: 4 longs (see run).  Returns the library's status code of the geometry, or -1 for
// a reduced angle of 0 (the planned path serves those with the transposed separable kernel: axis_adjoint_emulation.cpp).
extern "C" int aai_emu_adjoint_plain(const aai_request *rq, const float *gdst, float *gsrc, unsigned maxListed, long *counts)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (g.axisAligned) return -1;
    const RotLaunch r = make_rot_launch(g, rq->mode, rq->policy);
    if (rq->mode == AAI_MODE_FAST) run<AAI_MODE_FAST>(r, gdst, gsrc, maxListed, counts);
    else run<AAI_MODE_AREA>(r, gdst, gsrc, maxListed, counts);
    return AAI_OK;
}
