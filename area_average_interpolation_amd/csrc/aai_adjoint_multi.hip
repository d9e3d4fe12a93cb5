// aai_adjoint_multi.hip -- the adjoint (transposed) resampling of images with 2..4 interleaved channels: gsrc = W^T gdst per channel.
//
// Compiled with -ffp-contract=off like aai_adjoint.hip (see the Makefile), and from the same per-pixel code (aai_adjoint_math.hpp:
// adjoint_normalised_multi, adjoint_gather_multi): the weight of a (dst, src) pair does not depend on the channel, so a pair is
// classified, integrated and -- at a knife edge -- replayed ONCE, and each channel then costs a load and a multiply-add (pass 2) or
// a load and a division (pass 1).  Channel c of the result has the bits aai_adjoint.hip gives plane c alone: the same operands
// in the same order, only shared.
//
// The two kernels are the two of aai_adjoint.hip with C elements per lane -- the 16 x 16 tiling, tileRow0 for images of more than
// 65,535 tile rows, the batch in grid.z; no LDS, no atomics, every element of gsrc written exactly once (zeros included):
//   aai_adjoint_norm_multi_kernel<MODE, C>    one lane per dst pixel: n[d][c] = gdst[d][c] / sum of weights
//   aai_adjoint_gather_multi_kernel<MODE, C>  one lane per SOURCE pixel: gsrc[s][c] = sum of weight(d, s) n[d][c]
// n is fp64 with the channels innermost, [dH][dW][C]: a lane's C loads per pair are contiguous.  The C floats of a pixel are loaded
// and stored one by one: a row stride is any number of elements, so nothing wider than 4 bytes is aligned.
#include "aai_kernels.hpp"
#include "aai_adjoint_math.hpp"

namespace aai {

constexpr int kAdjMultiTile = 16;      // workgroup = 16 x 16 pixels (dst pixels in pass 1, source pixels in pass 2)

template <int MODE, int C>
__global__ __launch_bounds__(kAdjMultiTile *kAdjMultiTile) void aai_adjoint_norm_multi_kernel(RotLaunch r, const float *__restrict__ gdst, ImageView dv,
                                                                                             double *__restrict__ n, int tileRow0)
{
    const int dx = blockIdx.x * kAdjMultiTile + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kAdjMultiTile + threadIdx.y;
    if (dx >= r.dW || dy >= r.dH) return;
    const float *g = gdst + (int64_t)blockIdx.z * dv.imageStride + (int64_t)dy * dv.rowStride + (int64_t)dx * C;
    double gd[C], out[C];
#pragma unroll
    for (int c = 0; c < C; ++c) gd[c] = (double)g[c];
    adjoint_normalised_multi<MODE, C>(r, dx, dy, gd, out);
    double *nd = n + (((int64_t)blockIdx.z * r.dH + dy) * r.dW + dx) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) nd[c] = out[c];
}

template <int MODE, int C>
__global__ __launch_bounds__(kAdjMultiTile *kAdjMultiTile) void aai_adjoint_gather_multi_kernel(RotLaunch r, const double *__restrict__ n, float *__restrict__ gsrc,
                                                                                               ImageView sv, int tileRow0)
{
    const int sx = blockIdx.x * kAdjMultiTile + threadIdx.x;
    const int sy = (tileRow0 + blockIdx.y) * kAdjMultiTile + threadIdx.y;
    if (sx >= r.W || sy >= r.H) return;
    double acc[C];
    adjoint_gather_multi<MODE, C>(r, sx, sy, n + (int64_t)blockIdx.z * r.dH * r.dW * C, acc);
    float *g = gsrc + (int64_t)blockIdx.z * sv.imageStride + (int64_t)sy * sv.rowStride + (int64_t)sx * C;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = (float)acc[c];
}

template <int MODE, int C>
static hipError_t launch_adjoint_multi_as(const RotLaunch &r, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                          hipStream_t stream)
{
    const dim3 block(kAdjMultiTile, kAdjMultiTile, 1);
    const int dstTileRows = (r.dH + kAdjMultiTile - 1) / kAdjMultiTile, srcTileRows = (r.H + kAdjMultiTile - 1) / kAdjMultiTile;
    for (int t0 = 0; t0 < dstTileRows; t0 += 65535) {         // grid.y carries at most 65535 tiles
        const dim3 grid((r.dW + kAdjMultiTile - 1) / kAdjMultiTile, dstTileRows - t0 < 65535 ? dstTileRows - t0 : 65535, batch);
        hipLaunchKernelGGL((aai_adjoint_norm_multi_kernel<MODE, C>), grid, block, 0, stream, r, gdst, dv, n, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (int t0 = 0; t0 < srcTileRows; t0 += 65535) {
        const dim3 grid((r.W + kAdjMultiTile - 1) / kAdjMultiTile, srcTileRows - t0 < 65535 ? srcTileRows - t0 : 65535, batch);
        hipLaunchKernelGGL((aai_adjoint_gather_multi_kernel<MODE, C>), grid, block, 0, stream, r, n, gsrc, sv, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int MODE>
static hipError_t launch_adjoint_multi_mode(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, double *n, float *gsrc,
                                            ImageView sv, hipStream_t stream)
{
    switch (channels) {
    case 2: return launch_adjoint_multi_as<MODE, 2>(r, batch, gdst, dv, n, gsrc, sv, stream);
    case 3: return launch_adjoint_multi_as<MODE, 3>(r, batch, gdst, dv, n, gsrc, sv, stream);
    case 4: return launch_adjoint_multi_as<MODE, 4>(r, batch, gdst, dv, n, gsrc, sv, stream);
    default: return hipErrorInvalidValue;      // (1 channel is launch_adjoint's; the engine never asks for another count)
    }
}

// `channels` in 2..4; `batch` images (at most 65535: grid.z); n holds batch x dH x dW x channels doubles.  Only enqueues.
hipError_t launch_adjoint_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                hipStream_t stream, const char **kernelName)
{
    static const char *const names[2][3] = {
        {"aai_adjoint_gather_multi_kernel<area, 2>", "aai_adjoint_gather_multi_kernel<area, 3>", "aai_adjoint_gather_multi_kernel<area, 4>"},
        {"aai_adjoint_gather_multi_kernel<fast, 2>", "aai_adjoint_gather_multi_kernel<fast, 3>", "aai_adjoint_gather_multi_kernel<fast, 4>"}};
    if (channels < 2 || channels > 4) return hipErrorInvalidValue;
    if (kernelName) *kernelName = names[r.mode == AAI_MODE_FAST ? 1 : 0][channels - 2];
    if (batch <= 0 || r.dW <= 0 || r.dH <= 0 || r.W <= 0 || r.H <= 0) return hipSuccess;
    return r.mode == AAI_MODE_FAST ? launch_adjoint_multi_mode<AAI_MODE_FAST>(r, channels, batch, gdst, dv, n, gsrc, sv, stream)
                                   : launch_adjoint_multi_mode<AAI_MODE_AREA>(r, channels, batch, gdst, dv, n, gsrc, sv, stream);
}

}  // namespace aai
