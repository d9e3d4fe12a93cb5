// aai_adjoint_plain_multi.hip -- the planned adjoint at general rotations for images with 2..4 interleaved channels
// (aai_adjoint_rotated_interleaved_*): gsrc = W^T gdst per channel from the plan's sums and the plain closed forms.  It combines the two
// halves that existed apart: aai_adjoint_multi.hip shares a pair's weight over the channels, aai_adjoint_plain.hip takes the
// knife-edge code off the common path.  The per-pixel bodies live in aai_adjoint_plain.hpp (adjoint_scaled,
// adjoint_plain_gather_multi) and aai_adjoint_math.hpp (adjoint_gather_multi), shared with the CPU replay of the test-suite
// (tests/emulation/adjoint_plain_multi_emulation.cpp); the plan's tables -- S and the listed source pixels -- do not depend on the
// channel count and are the single-channel path's own.
//
// Compiled with -ffp-contract=off like aai_adjoint_plain.hip and aai_adjoint_multi.hip (see the Makefile): channel c must get the bits
// those units give plane c.
//
// Per call, every element of gsrc written exactly once by the plain gather (zeros included), no LDS, no atomics -- deterministic, image
// b of a batch gets the bits of a single-image call:
//   aai_adjoint_scale_multi_kernel<MODE, C>          one lane per row ELEMENT: n[d][c] = gdst[d][c] / S[d] (0 where the forward writes
//                                                    0).  A wave covers 64 consecutive floats of a row of dW * C floats and S is
//                                                    indexed by e / C, so loads and stores are coalesced for C = 3 too
//   aai_adjoint_plain_gather_multi_kernel<MODE, C>   one lane per SOURCE pixel, the 16 x 16 tiling and indexing of
//                                                    aai_adjoint_plain_gather_kernel, C fp64 accumulators
//   aai_adjoint_gather_listed_multi_kernel<MODE, C>  one lane per listed source pixel: the general per-pair code
//                                                    (adjoint_gather_multi), OVERWRITING the C floats of that pixel -- the
//                                                    multi-channel twin of aai_adjoint_gather_listed_kernel
//   aai_adjoint_norm_listed_multi_kernel<MODE, C>    one lane per listed DST pixel: the general normaliser (adjoint_normalised_multi)
//                                                    into the C doubles of that pixel of n -- the multi-channel twin of
//                                                    aai_adjoint_norm_listed_kernel.  Not part of the path above: with the listed
//                                                    gather it is the correction pass behind the interleaved transposed separable
//                                                    kernel (launch_adjoint_listed_multi; aai_axis_adjoint_multi.hip), which has no
//                                                    sums to scale by and so normalises the listed dst pixels itself
// n is fp64 with the channels innermost, [dH][dW][C], the layout of aai_adjoint_multi.hip.  The C floats of a pixel of gdst / gsrc are
// accessed one by one: a row stride is any number of elements, so nothing wider than 4 bytes is aligned.
// The group of C doubles of a pixel of n is read in the source as C plain 8-byte loads -- the form that shipped.  The scratch is the
// library's own and its pool allocation is aligned, so 16-byte loads are legal for C = 2 and C = 4, and a hand-written 16-byte form
// was not needed: the ISA of this unit shows that the compiler merges the C loads of a pair itself (one global_load_dwordx4 for
// C = 2, dwordx4 + dwordx2 for C = 3, two dwordx4 for C = 4, in the plain and in the listed gather).  No spills and no private memory
// in the scale and plain gather kernels (`make report`; DESIGN.md section 9 has the table of every instantiation).
#include "aai_kernels.hpp"
#include "aai_adjoint_plain.hpp"

namespace aai {

constexpr int kPlainMultiTile = 16;                           // workgroup = 16 x 16 source pixels, as in aai_adjoint_plain.hip
constexpr int kScaleMultiCols = 64, kScaleMultiRows = 4;      // the element-wise pass: a wave covers 64 consecutive ELEMENTS of a row
constexpr int kListedMultiBlock = 256;

template <int MODE, int C>
__global__ __launch_bounds__(kScaleMultiCols *kScaleMultiRows) void aai_adjoint_scale_multi_kernel(int dW, int dH, const double *__restrict__ S,
                                                                                                  const float *__restrict__ gdst, ImageView dv,
                                                                                                  double *__restrict__ n, int tileRow0)
{
    const int rowLen = dW * C;                                // (at most INT32_MAX / 2: the entries check the row length)
    const int e = blockIdx.x * kScaleMultiCols + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kScaleMultiRows + threadIdx.y;
    if (e >= rowLen || dy >= dH) return;
    const float gd = gdst[(int64_t)blockIdx.z * dv.imageStride + (int64_t)dy * dv.rowStride + e];
    n[((int64_t)blockIdx.z * dH + dy) * rowLen + e] = adjoint_scaled<MODE>(S[(int64_t)dy * dW + e / C], (double)gd);
}

template <int MODE, int C>
__global__ __launch_bounds__(kPlainMultiTile *kPlainMultiTile) void aai_adjoint_plain_gather_multi_kernel(RotLaunch r, const double *__restrict__ n,
                                                                                                         float *__restrict__ gsrc, ImageView sv, int tileRow0)
{
    const int sx = blockIdx.x * kPlainMultiTile + threadIdx.x;
    const int sy = (tileRow0 + blockIdx.y) * kPlainMultiTile + threadIdx.y;
    if (sx >= r.W || sy >= r.H) return;
    double acc[C];
    adjoint_plain_gather_multi<MODE, C>(r, sx, sy, n + (int64_t)blockIdx.z * r.dH * r.dW * C, acc);
    float *g = gsrc + (int64_t)blockIdx.z * sv.imageStride + (int64_t)sy * sv.rowStride + (int64_t)sx * C;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = (float)acc[c];
}

template <int MODE, int C>
__global__ __launch_bounds__(kListedMultiBlock) void aai_adjoint_gather_listed_multi_kernel(RotLaunch r, const double *__restrict__ n, float *__restrict__ gsrc,
                                                                                           ImageView sv, const uint2 *__restrict__ list, unsigned count)
{
    const unsigned i = blockIdx.x * kListedMultiBlock + threadIdx.x;
    if (i >= count) return;
    const int sx = (int)list[i].x, sy = (int)list[i].y;
    double acc[C];
    adjoint_gather_multi<MODE, C>(r, sx, sy, n + (int64_t)blockIdx.z * r.dH * r.dW * C, acc);
    float *g = gsrc + (int64_t)blockIdx.z * sv.imageStride + (int64_t)sy * sv.rowStride + (int64_t)sx * C;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = (float)acc[c];
}

template <int MODE, int C>
__global__ __launch_bounds__(kListedMultiBlock) void aai_adjoint_norm_listed_multi_kernel(RotLaunch r, const float *__restrict__ gdst, ImageView dv,
                                                                                         double *__restrict__ n, const uint2 *__restrict__ list, unsigned count)
{
    const unsigned i = blockIdx.x * kListedMultiBlock + threadIdx.x;
    if (i >= count) return;
    const int dx = (int)list[i].x, dy = (int)list[i].y;
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
static hipError_t launch_adjoint_listed_multi_as(const RotLaunch &r, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                                 const uint2 *dstList, unsigned nDst, const uint2 *srcList, unsigned nSrc, hipStream_t stream)
{
    const dim3 block(kListedMultiBlock, 1, 1), gridD((nDst + kListedMultiBlock - 1) / kListedMultiBlock, 1, batch), gridS((nSrc + kListedMultiBlock - 1) / kListedMultiBlock, 1, batch);
    hipLaunchKernelGGL((aai_adjoint_norm_listed_multi_kernel<MODE, C>), gridD, block, 0, stream, r, gdst, dv, n, dstList, nDst);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((aai_adjoint_gather_listed_multi_kernel<MODE, C>), gridS, block, 0, stream, r, n, gsrc, sv, srcList, nSrc);
    return hipGetLastError();
}

template <int MODE>
static hipError_t launch_adjoint_listed_multi_mode(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, double *n, float *gsrc,
                                                   ImageView sv, const uint2 *dstList, unsigned nDst, const uint2 *srcList, unsigned nSrc, hipStream_t stream)
{
    switch (channels) {
    case 2: return launch_adjoint_listed_multi_as<MODE, 2>(r, batch, gdst, dv, n, gsrc, sv, dstList, nDst, srcList, nSrc, stream);
    case 3: return launch_adjoint_listed_multi_as<MODE, 3>(r, batch, gdst, dv, n, gsrc, sv, dstList, nDst, srcList, nSrc, stream);
    case 4: return launch_adjoint_listed_multi_as<MODE, 4>(r, batch, gdst, dv, n, gsrc, sv, dstList, nDst, srcList, nSrc, stream);
    default: return hipErrorInvalidValue;
    }
}

// The two passes of the general multi-channel adjoint over LISTS of pixels (the correction pass behind launch_axis_adjoint_multi): pass 1
// over the nDst dst pixels of dstList into n (the other elements of n are neither written nor read), pass 2 over the nSrc source pixels
// of srcList, whose C floats of gsrc it OVERWRITES.  `channels` in 2..4; n holds batch x dH x dW x channels doubles; `batch` <= 65535.
hipError_t launch_adjoint_listed_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                       const uint2 *dstList, unsigned nDst, const uint2 *srcList, unsigned nSrc, hipStream_t stream)
{
    if (channels < 2 || channels > 4) return hipErrorInvalidValue;
    if (batch <= 0 || !nDst || !nSrc) return hipSuccess;
    return r.mode == AAI_MODE_FAST ? launch_adjoint_listed_multi_mode<AAI_MODE_FAST>(r, channels, batch, gdst, dv, n, gsrc, sv, dstList, nDst, srcList, nSrc, stream)
                                   : launch_adjoint_listed_multi_mode<AAI_MODE_AREA>(r, channels, batch, gdst, dv, n, gsrc, sv, dstList, nDst, srcList, nSrc, stream);
}

template <int MODE, int C>
static hipError_t launch_adjoint_plain_multi_as(const RotLaunch &r, int batch, const float *gdst, ImageView dv, const double *S, double *n, float *gsrc,
                                                ImageView sv, const uint2 *srcList, unsigned nSrc, hipStream_t stream)
{
    const int dstTileRows = (r.dH + kScaleMultiRows - 1) / kScaleMultiRows, srcTileRows = (r.H + kPlainMultiTile - 1) / kPlainMultiTile;
    const int64_t rowLen = (int64_t)r.dW * C;
    for (int t0 = 0; t0 < dstTileRows; t0 += 65535) {         // grid.y carries at most 65535 tiles
        const dim3 block(kScaleMultiCols, kScaleMultiRows, 1);
        const dim3 grid((unsigned)((rowLen + kScaleMultiCols - 1) / kScaleMultiCols), dstTileRows - t0 < 65535 ? dstTileRows - t0 : 65535, batch);
        hipLaunchKernelGGL((aai_adjoint_scale_multi_kernel<MODE, C>), grid, block, 0, stream, r.dW, r.dH, S, gdst, dv, n, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (int t0 = 0; t0 < srcTileRows; t0 += 65535) {
        const dim3 block(kPlainMultiTile, kPlainMultiTile, 1);
        const dim3 grid((r.W + kPlainMultiTile - 1) / kPlainMultiTile, srcTileRows - t0 < 65535 ? srcTileRows - t0 : 65535, batch);
        hipLaunchKernelGGL((aai_adjoint_plain_gather_multi_kernel<MODE, C>), grid, block, 0, stream, r, n, gsrc, sv, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!nSrc) return hipSuccess;
    const dim3 block(kListedMultiBlock, 1, 1), gridS((nSrc + kListedMultiBlock - 1) / kListedMultiBlock, 1, batch);
    hipLaunchKernelGGL((aai_adjoint_gather_listed_multi_kernel<MODE, C>), gridS, block, 0, stream, r, n, gsrc, sv, srcList, nSrc);
    return hipGetLastError();
}

template <int MODE>
static hipError_t launch_adjoint_plain_multi_mode(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, const double *S, double *n,
                                                  float *gsrc, ImageView sv, const uint2 *srcList, unsigned nSrc, hipStream_t stream)
{
    switch (channels) {
    case 2: return launch_adjoint_plain_multi_as<MODE, 2>(r, batch, gdst, dv, S, n, gsrc, sv, srcList, nSrc, stream);
    case 3: return launch_adjoint_plain_multi_as<MODE, 3>(r, batch, gdst, dv, S, n, gsrc, sv, srcList, nSrc, stream);
    case 4: return launch_adjoint_plain_multi_as<MODE, 4>(r, batch, gdst, dv, S, n, gsrc, sv, srcList, nSrc, stream);
    default: return hipErrorInvalidValue;      // (1 channel is launch_adjoint_plain's; the engine never asks for another count)
    }
}

// `channels` in 2..4; `batch` images (at most 65535: grid.z); S: the plan's sums; n holds batch x dH x dW x channels doubles; srcList /
// nSrc: the plan's listed source pixels (nSrc == 0: no listed pass).  Only enqueues.
hipError_t launch_adjoint_plain_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, const double *S, double *n, float *gsrc,
                                      ImageView sv, const uint2 *srcList, unsigned nSrc, hipStream_t stream, const char **kernelName)
{
    static const char *const names[2][3] = {
        {"aai_adjoint_plain_gather_multi_kernel<area, 2>", "aai_adjoint_plain_gather_multi_kernel<area, 3>", "aai_adjoint_plain_gather_multi_kernel<area, 4>"},
        {"aai_adjoint_plain_gather_multi_kernel<fast, 2>", "aai_adjoint_plain_gather_multi_kernel<fast, 3>", "aai_adjoint_plain_gather_multi_kernel<fast, 4>"}};
    if (channels < 2 || channels > 4) return hipErrorInvalidValue;
    if (kernelName) *kernelName = names[r.mode == AAI_MODE_FAST ? 1 : 0][channels - 2];
    if (batch <= 0 || r.dW <= 0 || r.dH <= 0 || r.W <= 0 || r.H <= 0) return hipSuccess;
    return r.mode == AAI_MODE_FAST ? launch_adjoint_plain_multi_mode<AAI_MODE_FAST>(r, channels, batch, gdst, dv, S, n, gsrc, sv, srcList, nSrc, stream)
                                   : launch_adjoint_plain_multi_mode<AAI_MODE_AREA>(r, channels, batch, gdst, dv, S, n, gsrc, sv, srcList, nSrc, stream);
}

}  // namespace aai
