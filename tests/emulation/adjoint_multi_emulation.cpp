// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the interleaved adjoint kernels (csrc/aai_adjoint_multi.hip).
//
// Built by tests/test_adjoint_interleaved_host.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_adjmultiemu.so.
// Like adjoint_emulation.cpp it reuses the PRODUCT's host planner (csrc/aai_plan.cpp) and the PRODUCT's per-pixel bodies
// (csrc/aai_adjoint_math.hpp: adjoint_normalised_multi, adjoint_gather_multi) and runs the two passes one pixel after the other, with
// the kernels' scratch layout ([dH][dW][C] doubles).  It is not part of the package, is never loaded by it, and is not a fallback.
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_adjoint_math.hpp"

using namespace aai;

template <int MODE, int C>
static void run(const RotLaunch &r, const float *gdst, float *gsrc)
{
    std::vector<double> n((size_t)r.dW * r.dH * C);
    for (int dy = 0; dy < r.dH; ++dy)
        for (int dx = 0; dx < r.dW; ++dx) {
            const size_t at = ((size_t)dy * r.dW + dx) * C;
            double gd[C], out[C];
            for (int c = 0; c < C; ++c) gd[c] = (double)gdst[at + c];
            adjoint_normalised_multi<MODE, C>(r, dx, dy, gd, out);
            for (int c = 0; c < C; ++c) n[at + c] = out[c];
        }
    for (int sy = 0; sy < r.H; ++sy)
        for (int sx = 0; sx < r.W; ++sx) {
            double acc[C];
            adjoint_gather_multi<MODE, C>(r, sx, sy, n.data(), acc);
            for (int c = 0; c < C; ++c) gsrc[((size_t)sy * r.W + sx) * C + c] = (float)acc[c];
        }
}

template <int MODE>
static int run_channels(const RotLaunch &r, int channels, const float *gdst, float *gsrc)
{
    switch (channels) {
    case 2: run<MODE, 2>(r, gdst, gsrc); return AAI_OK;
    case 3: run<MODE, 3>(r, gdst, gsrc); return AAI_OK;
    case 4: run<MODE, 4>(r, gdst, gsrc); return AAI_OK;
    default: return AAI_ERR_BAD_ARGUMENT;
    }
}

// gdst: dH x dW x channels (dense, channels innermost), gsrc: H x W x channels.  Returns the library's status code of the geometry.
extern "C" int aai_emu_adjoint_multi(const aai_request *rq, int channels, const float *gdst, float *gsrc)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    const RotLaunch r = make_rot_launch(g, rq->mode, rq->policy);
    return rq->mode == AAI_MODE_FAST ? run_channels<AAI_MODE_FAST>(r, channels, gdst, gsrc) : run_channels<AAI_MODE_AREA>(r, channels, gdst, gsrc);
}
