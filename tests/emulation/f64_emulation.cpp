// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the reference-precision kernels (csrc/aai_f64.hip).
//
// Built by tests/test_f64_host.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_f64emu.so.  It reuses the
// PRODUCT's host planner (csrc/aai_plan.cpp) and the PRODUCT's per-pixel bodies (csrc/aai_f64_math.hpp, csrc/aai_adjoint_math.hpp) and
// runs the three kernels one pixel after the other on dense double images, so that the CPU test-suite can compare dst = W src and
// gsrc = W^T gdst with the oracle and with the reference's recorded outputs in a container without a GPU.  It is not part of the
// package, is never loaded by it, and is not a fallback for anything.
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_f64_math.hpp"

using namespace aai;

template <int MODE>
static void forward(const RotLaunch &r, const double *src, double *dst)
{
    for (int dy = 0; dy < r.dH; ++dy)
        for (int dx = 0; dx < r.dW; ++dx) dst[(size_t)dy * r.dW + dx] = f64_forward<MODE>(r, dx, dy, src, r.W);
}

template <int MODE>
static void adjoint(const RotLaunch &r, const double *gdst, double *gsrc)
{
    std::vector<double> n((size_t)r.dW * r.dH);
    for (int dy = 0; dy < r.dH; ++dy)
        for (int dx = 0; dx < r.dW; ++dx) n[(size_t)dy * r.dW + dx] = adjoint_normalised<MODE>(r, dx, dy, gdst[(size_t)dy * r.dW + dx]);
    for (int sy = 0; sy < r.H; ++sy)
        for (int sx = 0; sx < r.W; ++sx) gsrc[(size_t)sy * r.W + sx] = adjoint_gather<MODE>(r, sx, sy, n.data());
}

static int launch_of(const aai_request *rq, RotLaunch &r)
{
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    r = make_rot_launch(g, rq->mode, rq->policy);
    return AAI_OK;
}

// src: W x H (dense), dst: dW x dH (dense).  Returns the library's status code of the geometry.
extern "C" int aai_emu_f64_forward(const aai_request *rq, const double *src, double *dst)
{
    RotLaunch r;
    const int rc = launch_of(rq, r);
    if (rc != AAI_OK) return rc;
    if (rq->mode == AAI_MODE_FAST) forward<AAI_MODE_FAST>(r, src, dst);
    else forward<AAI_MODE_AREA>(r, src, dst);
    return AAI_OK;
}

// gdst: dW x dH (dense), gsrc: W x H (dense)
extern "C" int aai_emu_f64_adjoint(const aai_request *rq, const double *gdst, double *gsrc)
{
    RotLaunch r;
    const int rc = launch_of(rq, r);
    if (rc != AAI_OK) return rc;
    if (rq->mode == AAI_MODE_FAST) adjoint<AAI_MODE_FAST>(r, gdst, gsrc);
    else adjoint<AAI_MODE_AREA>(r, gdst, gsrc);
    return AAI_OK;
}
