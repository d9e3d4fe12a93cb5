// aai_f64.hip -- the reference-precision path of the area and fast modes: forward dst = W src and adjoint gsrc = W^T gdst on DOUBLE
// images, end to end (the reference's own element type).  No value is rounded to fp32 anywhere.
//
// Compiled with -ffp-contract=off like aai_adjoint.hip (see the Makefile): the weights are the ones of aai_adjoint_math.hpp, and the
// CPU replay of the test-suite (tests/emulation/f64_emulation.cpp) executes the same IEEE operations.
//
// Three kernels, each a gather without atomics, LDS or staging, every element written exactly once (zeros included) -- so the result
// is deterministic, and image b of a batch gets the bits a single-image call gives it:
//   aai_f64_forward_kernel         one lane per dst pixel, the 16 x 16 tiling of aai_adjoint_norm_kernel: f64_forward (aai_f64_math.hpp)
//   aai_f64_adjoint_norm_kernel    one lane per dst pixel: n[d] = gdst[d] / sum of weights (adjoint_normalised)
//   aai_f64_adjoint_gather_kernel  one lane per SOURCE pixel, 16 x 16 source pixels per workgroup: adjoint_gather, stored as it is
// The kernels sit on the fp64 issue rate; the 8-byte gathers of neighbouring lanes overlap and mostly hit L1 (staging the window
// through LDS was measured for the double-precision forward and lost: aai_rotated_kernel.hpp).
// One code path for every angle: rotations by multiples of 90 degrees run through the same per-pair code -- correct, and deliberately
// not fast.
#include "aai_kernels.hpp"
#include "aai_f64_math.hpp"

namespace aai {

constexpr int kF64Tile = 16;      // workgroup = 16 x 16 pixels (dst pixels in the forward and pass 1, source pixels in the gather)

template <int MODE>
__global__ __launch_bounds__(kF64Tile *kF64Tile) void aai_f64_forward_kernel(RotLaunch r, const double *__restrict__ src, ImageView sv,
                                                                             double *__restrict__ dst, ImageView dv, int tileRow0)
{
    const int dx = blockIdx.x * kF64Tile + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kF64Tile + threadIdx.y;
    if (dx >= r.dW || dy >= r.dH) return;
    const double v = f64_forward<MODE>(r, dx, dy, src + (int64_t)blockIdx.z * sv.imageStride, sv.rowStride);
    dst[(int64_t)blockIdx.z * dv.imageStride + (int64_t)dy * dv.rowStride + dx] = v;
}

template <int MODE>
__global__ __launch_bounds__(kF64Tile *kF64Tile) void aai_f64_adjoint_norm_kernel(RotLaunch r, const double *__restrict__ gdst, ImageView dv,
                                                                                  double *__restrict__ n, int tileRow0)
{
    const int dx = blockIdx.x * kF64Tile + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kF64Tile + threadIdx.y;
    if (dx >= r.dW || dy >= r.dH) return;
    const double gd = gdst[(int64_t)blockIdx.z * dv.imageStride + (int64_t)dy * dv.rowStride + dx];
    n[((int64_t)blockIdx.z * r.dH + dy) * r.dW + dx] = adjoint_normalised<MODE>(r, dx, dy, gd);
}

template <int MODE>
__global__ __launch_bounds__(kF64Tile *kF64Tile) void aai_f64_adjoint_gather_kernel(RotLaunch r, const double *__restrict__ n, double *__restrict__ gsrc,
                                                                                    ImageView sv, int tileRow0)
{
    const int sx = blockIdx.x * kF64Tile + threadIdx.x;
    const int sy = (tileRow0 + blockIdx.y) * kF64Tile + threadIdx.y;
    if (sx >= r.W || sy >= r.H) return;
    const double g = adjoint_gather<MODE>(r, sx, sy, n + (int64_t)blockIdx.z * r.dH * r.dW);
    gsrc[(int64_t)blockIdx.z * sv.imageStride + (int64_t)sy * sv.rowStride + sx] = g;
}

// `batch` images (at most 65535: grid.z).  Only enqueues.
hipError_t launch_f64_forward(const RotLaunch &r, int batch, const double *src, ImageView sv, double *dst, ImageView dv, hipStream_t stream,
                              const char **kernelName)
{
    if (kernelName) *kernelName = r.mode == AAI_MODE_FAST ? "aai_f64_forward_kernel<fast>" : "aai_f64_forward_kernel<area>";
    if (batch <= 0 || r.dW <= 0 || r.dH <= 0) return hipSuccess;
    const dim3 block(kF64Tile, kF64Tile, 1);
    const int tileRows = (r.dH + kF64Tile - 1) / kF64Tile;
    for (int t0 = 0; t0 < tileRows; t0 += 65535) {            // grid.y carries at most 65535 tiles
        const dim3 grid((r.dW + kF64Tile - 1) / kF64Tile, tileRows - t0 < 65535 ? tileRows - t0 : 65535, batch);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_f64_forward_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r, src, sv, dst, dv, t0);
        else hipLaunchKernelGGL(aai_f64_forward_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r, src, sv, dst, dv, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// `batch` images (at most 65535: grid.z); n holds batch x dH x dW doubles.  Only enqueues.
hipError_t launch_f64_adjoint(const RotLaunch &r, int batch, const double *gdst, ImageView dv, double *n, double *gsrc, ImageView sv,
                              hipStream_t stream, const char **kernelName)
{
    if (kernelName) *kernelName = r.mode == AAI_MODE_FAST ? "aai_f64_adjoint_gather_kernel<fast>" : "aai_f64_adjoint_gather_kernel<area>";
    if (batch <= 0 || r.dW <= 0 || r.dH <= 0 || r.W <= 0 || r.H <= 0) return hipSuccess;
    const dim3 block(kF64Tile, kF64Tile, 1);
    const int dstTileRows = (r.dH + kF64Tile - 1) / kF64Tile, srcTileRows = (r.H + kF64Tile - 1) / kF64Tile;
    for (int t0 = 0; t0 < dstTileRows; t0 += 65535) {         // grid.y carries at most 65535 tiles
        const dim3 grid((r.dW + kF64Tile - 1) / kF64Tile, dstTileRows - t0 < 65535 ? dstTileRows - t0 : 65535, batch);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_f64_adjoint_norm_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r, gdst, dv, n, t0);
        else hipLaunchKernelGGL(aai_f64_adjoint_norm_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r, gdst, dv, n, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (int t0 = 0; t0 < srcTileRows; t0 += 65535) {
        const dim3 grid((r.W + kF64Tile - 1) / kF64Tile, srcTileRows - t0 < 65535 ? srcTileRows - t0 : 65535, batch);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_f64_adjoint_gather_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r, n, gsrc, sv, t0);
        else hipLaunchKernelGGL(aai_f64_adjoint_gather_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r, n, gsrc, sv, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace aai
