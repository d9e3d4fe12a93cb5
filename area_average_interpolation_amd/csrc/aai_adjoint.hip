// aai_adjoint.hip -- the adjoint (transposed) resampling of the area and fast modes: gsrc = W^T gdst.
//
// Compiled with -ffp-contract=off like aai_rotated_strict.hip (see the Makefile): the weights are the ones the forward's
// double-precision fix-up pass computes, knife edges included, and they only come out the same if every product and sum
// rounds the same.  The per-pixel bodies live in aai_adjoint_math.hpp (shared with the CPU replay of the test-suite).
//
// Two kernels, both a gather, no atomics, every element written exactly once (zeros included) -- so the result is
// deterministic, and image b of a batch gets the bits a single-image call gives it:
//   aai_adjoint_norm_kernel    one lane per dst pixel, the 16 x 16 tiling of aai_rotated_kernel: n[d] = gdst[d] / sum of weights
//   aai_adjoint_gather_kernel  one lane per SOURCE pixel, 16 x 16 source pixels per workgroup (a wave covers 16 x 4, its candidate
//                              dst pixels overlap in L1): sum over the pixel's scale^2 virtual pixels and the dst pixels they feed
// n is fp64: the result then carries ONE fp32 rounding (~6e-8 relative); its loads are the gather's only memory traffic beside
// one store per lane, and the kernel sits on the fp64 issue rate either way.
// One code path for every angle: a reduced angle of 0 (where the separable kernel serves the forward) runs through the same
// per-pair code -- correct, and deliberately not fast.
#include "aai_kernels.hpp"
#include "aai_adjoint_math.hpp"

namespace aai {

constexpr int kAdjTile = 16;      // workgroup = 16 x 16 pixels (dst pixels in pass 1, source pixels in pass 2)

template <int MODE>
__global__ __launch_bounds__(kAdjTile *kAdjTile) void aai_adjoint_norm_kernel(RotLaunch r, const float *__restrict__ gdst, ImageView dv,
                                                                              double *__restrict__ n, int tileRow0)
{
    const int dx = blockIdx.x * kAdjTile + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kAdjTile + threadIdx.y;
    if (dx >= r.dW || dy >= r.dH) return;
    const float gd = gdst[(int64_t)blockIdx.z * dv.imageStride + (int64_t)dy * dv.rowStride + dx];
    n[((int64_t)blockIdx.z * r.dH + dy) * r.dW + dx] = adjoint_normalised<MODE>(r, dx, dy, (double)gd);
}

template <int MODE>
__global__ __launch_bounds__(kAdjTile *kAdjTile) void aai_adjoint_gather_kernel(RotLaunch r, const double *__restrict__ n, float *__restrict__ gsrc,
                                                                                ImageView sv, int tileRow0)
{
    const int sx = blockIdx.x * kAdjTile + threadIdx.x;
    const int sy = (tileRow0 + blockIdx.y) * kAdjTile + threadIdx.y;
    if (sx >= r.W || sy >= r.H) return;
    const double g = adjoint_gather<MODE>(r, sx, sy, n + (int64_t)blockIdx.z * r.dH * r.dW);
    gsrc[(int64_t)blockIdx.z * sv.imageStride + (int64_t)sy * sv.rowStride + sx] = (float)g;
}

// The one-off kernel behind the planned adjoint at general rotations (aai_adjoint_plain.hip, aai_adjoint_plain.hpp): pass 1's sum of
// every dst pixel, kept per plan, a byte that says whether a pair of its window reported a knife edge, and the count of such pixels.
template <int MODE>
__global__ __launch_bounds__(kAdjTile *kAdjTile) void aai_adjoint_sums_kernel(RotLaunch r, double *__restrict__ S, unsigned char *__restrict__ knife,
                                                                                  unsigned *__restrict__ count, int tileRow0)
{
    const int dx = blockIdx.x * kAdjTile + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kAdjTile + threadIdx.y;
    if (dx >= r.dW || dy >= r.dH) return;
    bool k = false;
    const double sum = adjoint_weight_sum_report<MODE>(r, dx, dy, k);
    const int64_t i = (int64_t)dy * r.dW + dx;
    S[i] = sum;
    knife[i] = k ? 1 : 0;
    if (k) atomicAdd(count, 1u);
}

// The two passes over lists of pixels: the per-pixel bodies of the whole-image kernels above, one lane per list entry (x, y).
constexpr int kAdjListBlock = 256;

template <int MODE>
__global__ __launch_bounds__(kAdjListBlock) void aai_adjoint_norm_listed_kernel(RotLaunch r, const float *__restrict__ gdst, ImageView dv,
                                                                                double *__restrict__ n, const uint2 *__restrict__ list, unsigned count)
{
    const unsigned i = blockIdx.x * kAdjListBlock + threadIdx.x;
    if (i >= count) return;
    const int dx = (int)list[i].x, dy = (int)list[i].y;
    const float gd = gdst[(int64_t)blockIdx.z * dv.imageStride + (int64_t)dy * dv.rowStride + dx];
    n[((int64_t)blockIdx.z * r.dH + dy) * r.dW + dx] = adjoint_normalised<MODE>(r, dx, dy, (double)gd);
}

template <int MODE>
__global__ __launch_bounds__(kAdjListBlock) void aai_adjoint_gather_listed_kernel(RotLaunch r, const double *__restrict__ n, float *__restrict__ gsrc,
                                                                                 ImageView sv, const uint2 *__restrict__ list, unsigned count)
{
    const unsigned i = blockIdx.x * kAdjListBlock + threadIdx.x;
    if (i >= count) return;
    const int sx = (int)list[i].x, sy = (int)list[i].y;
    const double g = adjoint_gather<MODE>(r, sx, sy, n + (int64_t)blockIdx.z * r.dH * r.dW);
    gsrc[(int64_t)blockIdx.z * sv.imageStride + (int64_t)sy * sv.rowStride + sx] = (float)g;
}

hipError_t launch_adjoint_listed(const RotLaunch &r, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                 const uint2 *dstList, unsigned nDst, const uint2 *srcList, unsigned nSrc, hipStream_t stream)
{
    if (batch <= 0 || !nDst || !nSrc) return hipSuccess;
    const dim3 block(kAdjListBlock, 1, 1), gridD((nDst + kAdjListBlock - 1) / kAdjListBlock, 1, batch), gridS((nSrc + kAdjListBlock - 1) / kAdjListBlock, 1, batch);
    if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_norm_listed_kernel<AAI_MODE_FAST>, gridD, block, 0, stream, r, gdst, dv, n, dstList, nDst);
    else hipLaunchKernelGGL(aai_adjoint_norm_listed_kernel<AAI_MODE_AREA>, gridD, block, 0, stream, r, gdst, dv, n, dstList, nDst);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_gather_listed_kernel<AAI_MODE_FAST>, gridS, block, 0, stream, r, n, gsrc, sv, srcList, nSrc);
    else hipLaunchKernelGGL(aai_adjoint_gather_listed_kernel<AAI_MODE_AREA>, gridS, block, 0, stream, r, n, gsrc, sv, srcList, nSrc);
    return hipGetLastError();
}

// S: dH x dW doubles, knife: dH x dW bytes, count: one zeroed word.  Only enqueues.
hipError_t launch_adjoint_sums(const RotLaunch &r, double *S, unsigned char *knife, unsigned *count, hipStream_t stream)
{
    if (r.dW <= 0 || r.dH <= 0) return hipSuccess;
    const dim3 block(kAdjTile, kAdjTile, 1);
    const int tileRows = (r.dH + kAdjTile - 1) / kAdjTile;
    for (int t0 = 0; t0 < tileRows; t0 += 65535) {            // grid.y carries at most 65535 tiles
        const dim3 grid((r.dW + kAdjTile - 1) / kAdjTile, tileRows - t0 < 65535 ? tileRows - t0 : 65535, 1);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_sums_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r, S, knife, count, t0);
        else hipLaunchKernelGGL(aai_adjoint_sums_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r, S, knife, count, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the listed gather alone: n is complete already (the planned adjoint at general rotations, whose pass 1 is element-wise)
hipError_t launch_adjoint_gather_listed(const RotLaunch &r, int batch, const double *n, float *gsrc, ImageView sv, const uint2 *srcList, unsigned nSrc,
                                        hipStream_t stream)
{
    if (batch <= 0 || !nSrc) return hipSuccess;
    const dim3 block(kAdjListBlock, 1, 1), gridS((nSrc + kAdjListBlock - 1) / kAdjListBlock, 1, batch);
    if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_gather_listed_kernel<AAI_MODE_FAST>, gridS, block, 0, stream, r, n, gsrc, sv, srcList, nSrc);
    else hipLaunchKernelGGL(aai_adjoint_gather_listed_kernel<AAI_MODE_AREA>, gridS, block, 0, stream, r, n, gsrc, sv, srcList, nSrc);
    return hipGetLastError();
}

// `batch` images (at most 65535: grid.z); n holds batch x dH x dW doubles.  Only enqueues.
hipError_t launch_adjoint(const RotLaunch &r, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                          hipStream_t stream, const char **kernelName)
{
    if (kernelName) *kernelName = r.mode == AAI_MODE_FAST ? "aai_adjoint_gather_kernel<fast>" : "aai_adjoint_gather_kernel<area>";
    if (batch <= 0 || r.dW <= 0 || r.dH <= 0 || r.W <= 0 || r.H <= 0) return hipSuccess;
    const dim3 block(kAdjTile, kAdjTile, 1);
    const int dstTileRows = (r.dH + kAdjTile - 1) / kAdjTile, srcTileRows = (r.H + kAdjTile - 1) / kAdjTile;
    for (int t0 = 0; t0 < dstTileRows; t0 += 65535) {         // grid.y carries at most 65535 tiles
        const dim3 grid((r.dW + kAdjTile - 1) / kAdjTile, dstTileRows - t0 < 65535 ? dstTileRows - t0 : 65535, batch);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_norm_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r, gdst, dv, n, t0);
        else hipLaunchKernelGGL(aai_adjoint_norm_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r, gdst, dv, n, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (int t0 = 0; t0 < srcTileRows; t0 += 65535) {
        const dim3 grid((r.W + kAdjTile - 1) / kAdjTile, srcTileRows - t0 < 65535 ? srcTileRows - t0 : 65535, batch);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_gather_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r, n, gsrc, sv, t0);
        else hipLaunchKernelGGL(aai_adjoint_gather_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r, n, gsrc, sv, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace aai
