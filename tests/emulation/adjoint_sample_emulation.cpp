// TEST INFRASTRUCTURE ONLY -- serial CPU replay of the samplers' adjoint kernel (csrc/aai_adjoint_sample.hip).
//
// Built by tests/test_adjoint_sample_host.py with plain g++ (no HIP, no contraction) into tests/_build/libaai_adjsampleemu.so.  It reuses
// the PRODUCT's host planner (csrc/aai_plan.cpp) and the PRODUCT's per-pixel body (csrc/aai_adjoint_sample_math.hpp) and runs it one
// source pixel after the other, so that the CPU test-suite can compare gsrc = W^T gdst with the oracle's matrix in a container without
// a GPU, count the candidates the walk visits, and prove that the walk is a superset.  It is not part of the package, is never loaded
// by it, and is not a fallback for anything.
#include <vector>

#include "../../area_average_interpolation_amd/csrc/aai_plan.cpp"
#include "../../area_average_interpolation_amd/csrc/aai_adjoint_sample_math.hpp"

using namespace aai;

namespace {

// counts the candidates of one source pixel's walk and, among them, the pairs that carry weight
template <int MODE>
struct Count {
    const RotLaunch *r;
    int X, Y;
    long long *n, *weighted;
    void operator()(int dx, int dy) const
    {
        ++*n;
        if (adjoint_sample_weight<MODE>(*r, dx, dy, X, Y) != 0.0) ++*weighted;
    }
};

struct Mark {
    unsigned char *seen;      // dW x dH
    int dW;
    void operator()(int dx, int dy) const { seen[(size_t)dy * dW + dx] = 1; }
};

template <int MODE, int C>
void run(const AdjSampleLaunch &a, const float *gdst, float *gsrc, long long *visited, long long *weighted)
{
    const RotLaunch &r = a.r;
    long long n = 0, m = 0;
    for (int Y = 0; Y < r.H; ++Y)
        for (int X = 0; X < r.W; ++X) {
            double acc[C];
            adjoint_sample_gather<MODE, C>(a, X, Y, gdst, (int64_t)r.dW * C, acc, Count<MODE>{&r, X, Y, &n, &m});
            for (int c = 0; c < C; ++c) gsrc[((size_t)Y * r.W + X) * C + c] = (float)acc[c];
        }
    if (visited) *visited = n;
    if (weighted) *weighted = m;
}

template <int MODE>
void run_mode(const AdjSampleLaunch &a, int channels, const float *gdst, float *gsrc, long long *visited, long long *weighted)
{
    switch (channels) {
    case 1: run<MODE, 1>(a, gdst, gsrc, visited, weighted); break;
    case 2: run<MODE, 2>(a, gdst, gsrc, visited, weighted); break;
    case 3: run<MODE, 3>(a, gdst, gsrc, visited, weighted); break;
    default: run<MODE, 4>(a, gdst, gsrc, visited, weighted); break;
    }
}

// every (dst, src) pair with a nonzero weight by the brute-force loop over ALL dst pixels must be among the candidates of the source
// pixel's walk; counts the pairs with weight and returns the number the walk misses
template <int MODE>
long long superset(const AdjSampleLaunch &a, long long *pairs)
{
    const RotLaunch &r = a.r;
    std::vector<unsigned char> seen((size_t)r.dW * r.dH);
    std::vector<float> zeros((size_t)r.dW * r.dH, 0.f);
    long long missed = 0, withWeight = 0;
    for (int Y = 0; Y < r.H; ++Y)
        for (int X = 0; X < r.W; ++X) {
            std::fill(seen.begin(), seen.end(), 0);
            double acc[1];
            adjoint_sample_gather<MODE, 1>(a, X, Y, zeros.data(), (int64_t)r.dW, acc, Mark{seen.data(), r.dW});
            for (int dy = 0; dy < r.dH; ++dy)
                for (int dx = 0; dx < r.dW; ++dx)
                    if (adjoint_sample_weight<MODE>(r, dx, dy, X, Y) != 0.0) {
                        ++withWeight;
                        if (!seen[(size_t)dy * r.dW + dx]) ++missed;
                    }
        }
    if (pairs) *pairs = withWeight;
    return missed;
}

int launch_of(const aai_request *rq, AdjSampleLaunch &a)
{
    if (rq->mode != AAI_MODE_BILINEAR && rq->mode != AAI_MODE_BICUBIC) return AAI_ERR_BAD_ARGUMENT;
    Geometry g;
    std::string msg;
    const int rc = make_geometry(*rq, g, msg);
    if (rc != AAI_OK) return rc;
    a = make_adjoint_sample_launch(make_rot_launch(g, rq->mode, rq->policy));
    return AAI_OK;
}

}  // namespace

// gdst: dW x dH x channels (dense), gsrc: W x H x channels (dense); *visited, *weighted (either may be NULL): candidates the walks
// visited in all, and how many of them carry weight.  Returns the library's status code of the geometry.
extern "C" int aai_emu_adjoint_sample(const aai_request *rq, int channels, const float *gdst, float *gsrc, long long *visited, long long *weighted)
{
    AdjSampleLaunch a;
    const int rc = launch_of(rq, a);
    if (rc != AAI_OK) return rc;
    if (channels < 1 || channels > 4) return AAI_ERR_BAD_ARGUMENT;
    if (rq->mode == AAI_MODE_BILINEAR) run_mode<AAI_MODE_BILINEAR>(a, channels, gdst, gsrc, visited, weighted);
    else run_mode<AAI_MODE_BICUBIC>(a, channels, gdst, gsrc, visited, weighted);
    return AAI_OK;
}

// *missed: pairs with a nonzero weight that the candidate walk does not visit (must be 0); *pairs: pairs with a nonzero weight
extern "C" int aai_emu_adjoint_sample_superset(const aai_request *rq, long long *missed, long long *pairs)
{
    AdjSampleLaunch a;
    const int rc = launch_of(rq, a);
    if (rc != AAI_OK) return rc;
    *missed = rq->mode == AAI_MODE_BILINEAR ? superset<AAI_MODE_BILINEAR>(a, pairs) : superset<AAI_MODE_BICUBIC>(a, pairs);
    return AAI_OK;
}

// the dense matrix W (dW * dH rows, W * H columns, row-major) by the brute-force loop: what the replay's weights are, pair by pair
extern "C" int aai_emu_adjoint_sample_matrix(const aai_request *rq, double *M)
{
    AdjSampleLaunch a;
    const int rc = launch_of(rq, a);
    if (rc != AAI_OK) return rc;
    const RotLaunch &r = a.r;
    for (int dy = 0; dy < r.dH; ++dy)
        for (int dx = 0; dx < r.dW; ++dx)
            for (int Y = 0; Y < r.H; ++Y)
                for (int X = 0; X < r.W; ++X)
                    M[((size_t)dy * r.dW + dx) * ((size_t)r.W * r.H) + (size_t)Y * r.W + X] =
                        rq->mode == AAI_MODE_BILINEAR ? adjoint_sample_weight<AAI_MODE_BILINEAR>(r, dx, dy, X, Y) : adjoint_sample_weight<AAI_MODE_BICUBIC>(r, dx, dy, X, Y);
    return AAI_OK;
}
