// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the adjoint kernels (csrc/aai_adjoint.hip).
//
// Built by tests/test_adjoint_host.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_adjemu.so.  It reuses the
// PRODUCT's host planner (csrc/aai_plan.cpp) and the PRODUCT's per-pixel bodies (csrc/aai_adjoint_math.hpp) and runs the two
// passes one pixel after the other, so that the CPU test-suite can compare gsrc = W^T gdst with the oracle's matrix in a
// container without a GPU.  It is not part of the package, is never loaded by it, and is not a fallback for anything.
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_adjoint_math.hpp"

using namespace aai;

template <int MODE>
static void run(const RotLaunch &r, const float *gdst, float *gsrc)
{
    std::vector<double> n((size_t)r.dW * r.dH);
    for (int dy = 0; dy < r.dH; ++dy)
        for (int dx = 0; dx < r.dW; ++dx) n[(size_t)dy * r.dW + dx] = adjoint_normalised<MODE>(r, dx, dy, (double)gdst[(size_t)dy * r.dW + dx]);
    for (int sy = 0; sy < r.H; ++sy)
        for (int sx = 0; sx < r.W; ++sx) gsrc[(size_t)sy * r.W + sx] = (float)adjoint_gather<MODE>(r, sx, sy, n.data());
}

// gdst: dW x dH (dense), gsrc: W x H (dense).  Returns the library's status code of the geometry.
extern "C" int aai_emu_adjoint(const aai_request *rq, const float *gdst, float *gsrc)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    const RotLaunch r = make_rot_launch(g, rq->mode, rq->policy);
    if (rq->mode == AAI_MODE_FAST) run<AAI_MODE_FAST>(r, gdst, gsrc);
    else run<AAI_MODE_AREA>(r, gdst, gsrc);
    return AAI_OK;
}
