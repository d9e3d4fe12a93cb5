// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the interleaved planned adjoint at general rotations
// (aai_adjoint_rotated_interleaved_*: csrc/aai_engine.cpp enqueue_adjoint, the ROTATED family with 2..4 channels; csrc/aai_adjoint_plain_multi.hip).
//
// Built by tests/test_adjoint_rotated_interleaved_host.py with plain g++ (no HIP, no contraction) into
// tests/_build/libaai_adjplainmultiemu.so.  Like adjoint_plain_emulation.cpp it reuses the PRODUCT's host planner (csrc/aai_plan.cpp:
// build_adjoint_lists) and the PRODUCT's per-pixel bodies (csrc/aai_adjoint_math.hpp, csrc/aai_adjoint_plain.hpp) and runs the plan's
// tables and the call's passes one pixel after the other: S and K (single-channel, as the plan holds them), the source list, the
// element-wise pass 1 per row element, adjoint_plain_gather_multi, the listed overwrite by adjoint_gather_multi -- and the general
// interleaved adjoint whole where the engine would keep it.  Scratch layout of the kernels: [dH][dW][C] doubles.  Not part of the
// package, never loaded by it, not a fallback for anything.
#include <utility>
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_adjoint_plain.hpp"

using namespace aai;

// counts: [0] pixels of K, [1] listed source pixels, [2] 1 when the general interleaved adjoint served the geometry
template <int MODE, int C>
static void run(const RotLaunch &r, const float *gdst, float *gsrc, unsigned maxListed, long *counts)
{
    const size_t N = (size_t)r.dW * r.dH;
    std::vector<double> S(N), n(N * C);
    std::vector<std::pair<int, int>> K, srcList, dstList;
    for (int dy = 0; dy < r.dH; ++dy)
        for (int dx = 0; dx < r.dW; ++dx) {
            bool knife = false;
            S[(size_t)dy * r.dW + dx] = adjoint_weight_sum_report<MODE>(r, dx, dy, knife);
            if (knife) K.emplace_back(dx, dy);
        }
    bool general = K.size() > (size_t)maxListed;
    if (!general && !build_adjoint_lists(r, K, std::vector<int>(), std::vector<int>(), (size_t)r.W * r.H / 2, srcList, dstList)) general = true;
    counts[0] = (long)K.size(); counts[1] = general ? 0 : (long)srcList.size(); counts[2] = general ? 1 : 0;
    if (general) {
        for (int dy = 0; dy < r.dH; ++dy)
            for (int dx = 0; dx < r.dW; ++dx) {
                const size_t at = ((size_t)dy * r.dW + dx) * C;
                double gd[C], out[C];
                for (int c = 0; c < C; ++c) gd[c] = (double)gdst[at + c];
                adjoint_normalised_multi<MODE, C>(r, dx, dy, gd, out);
                for (int c = 0; c < C; ++c) n[at + c] = out[c];
            }
    } else {
        // one step per row ELEMENT, S indexed by e / C, as aai_adjoint_scale_multi_kernel does
        const size_t rowLen = (size_t)r.dW * C;
        for (int dy = 0; dy < r.dH; ++dy)
            for (size_t e = 0; e < rowLen; ++e) n[(size_t)dy * rowLen + e] = adjoint_scaled<MODE>(S[(size_t)dy * r.dW + e / C], (double)gdst[(size_t)dy * rowLen + e]);
    }
    for (int sy = 0; sy < r.H; ++sy)
        for (int sx = 0; sx < r.W; ++sx) {
            double acc[C];
            if (general) adjoint_gather_multi<MODE, C>(r, sx, sy, n.data(), acc);
            else adjoint_plain_gather_multi<MODE, C>(r, sx, sy, n.data(), acc);
            for (int c = 0; c < C; ++c) gsrc[((size_t)sy * r.W + sx) * C + c] = (float)acc[c];
        }
    for (const auto &s : srcList) {
        double acc[C];
        adjoint_gather_multi<MODE, C>(r, s.first, s.second, n.data(), acc);
        for (int c = 0; c < C; ++c) gsrc[((size_t)s.second * r.W + s.first) * C + c] = (float)acc[c];
    }
}

template <int MODE>
static int run_channels(const RotLaunch &r, int channels, const float *gdst, float *gsrc, unsigned maxListed, long *counts)
{
    switch (channels) {
    case 2: run<MODE, 2>(r, gdst, gsrc, maxListed, counts); return AAI_OK;
    case 3: run<MODE, 3>(r, gdst, gsrc, maxListed, counts); return AAI_OK;
    case 4: run<MODE, 4>(r, gdst, gsrc, maxListed, counts); return AAI_OK;
    default: return AAI_ERR_BAD_ARGUMENT;
    }
}

// gdst: dH x dW x channels (dense, channels innermost), gsrc: H x W x channels, counts: 3 longs (see run).  Returns the library's status
// code of the geometry, or -1 for a reduced angle of 0 (the entry forwards those to the general interleaved adjoint:
// adjoint_multi_emulation.cpp).
extern "C" int aai_emu_adjoint_plain_multi(const aai_request *rq, int channels, const float *gdst, float *gsrc, unsigned maxListed, long *counts)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    if (g.axisAligned) return -1;
    const RotLaunch r = make_rot_launch(g, rq->mode, rq->policy);
    return rq->mode == AAI_MODE_FAST ? run_channels<AAI_MODE_FAST>(r, channels, gdst, gsrc, maxListed, counts)
                                     : run_channels<AAI_MODE_AREA>(r, channels, gdst, gsrc, maxListed, counts);
}
