// aai_adjoint_plain.hip -- the planned adjoint at general rotations (aai_adjoint_rotated_*): gsrc = W^T gdst from per-plan sums and
// the plain closed forms.  The per-pixel bodies and the argument why the result has the bits of aai_adjoint.hip's kernels live in
// aai_adjoint_plain.hpp (shared with the CPU replay of the test-suite).
//
// Compiled with -ffp-contract=off like aai_adjoint.hip (see the Makefile): a pair's weight must round as it does there.
//
// Once per geometry (the plan's tables, aai_engine.cpp: build_rot_adjoint_tables), behind aai_adjoint_sums_kernel -- which is the general
// normaliser with its strict replay and therefore lives in aai_adjoint.hip; no kernel of THIS unit has side lists or private memory:
//   aai_adjoint_knife_list_kernel  the flagged pixels as a list of (dx, dy), through a cursor, at most `capacity` entries
// Per call, both writing every element once (zeros included), no atomics -- deterministic, image b of a batch gets the bits of a
// single-image call:
//   aai_adjoint_scale_kernel         one lane per dst pixel: n[d] = gdst[d] / S[d] (0 where the forward writes 0): element-wise
//   aai_adjoint_plain_gather_kernel  one lane per SOURCE pixel, the tiling and indexing of aai_adjoint_gather_kernel
// and behind them, where the plan lists source pixels, aai_adjoint_gather_listed_kernel of aai_adjoint.hip.
#include "aai_kernels.hpp"
#include "aai_adjoint_plain.hpp"

namespace aai {

constexpr int kPlainTile = 16;                           // workgroup = 16 x 16 pixels, as in aai_adjoint.hip
constexpr int kScaleCols = 64, kScaleRows = 4;           // the element-wise pass: a wave covers 64 consecutive pixels of a row

__global__ __launch_bounds__(kPlainTile *kPlainTile) void aai_adjoint_knife_list_kernel(const unsigned char *__restrict__ knife, int dW, int dH,
                                                                                        uint2 *__restrict__ list, unsigned *__restrict__ cursor,
                                                                                        unsigned capacity, int tileRow0)
{
    const int dx = blockIdx.x * kPlainTile + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kPlainTile + threadIdx.y;
    if (dx >= dW || dy >= dH) return;
    if (!knife[(int64_t)dy * dW + dx]) return;
    const unsigned at = atomicAdd(cursor, 1u);
    if (at < capacity) list[at] = make_uint2((unsigned)dx, (unsigned)dy);
}

template <int MODE>
__global__ __launch_bounds__(kScaleCols *kScaleRows) void aai_adjoint_scale_kernel(int dW, int dH, const double *__restrict__ S, const float *__restrict__ gdst,
                                                                                  ImageView dv, double *__restrict__ n, int tileRow0)
{
    const int dx = blockIdx.x * kScaleCols + threadIdx.x;
    const int dy = (tileRow0 + blockIdx.y) * kScaleRows + threadIdx.y;
    if (dx >= dW || dy >= dH) return;
    const int64_t i = (int64_t)dy * dW + dx;
    const float gd = gdst[(int64_t)blockIdx.z * dv.imageStride + (int64_t)dy * dv.rowStride + dx];
    n[(int64_t)blockIdx.z * dH * dW + i] = adjoint_scaled<MODE>(S[i], (double)gd);
}

template <int MODE>
__global__ __launch_bounds__(kPlainTile *kPlainTile) void aai_adjoint_plain_gather_kernel(RotLaunch r, const double *__restrict__ n, float *__restrict__ gsrc,
                                                                                          ImageView sv, int tileRow0)
{
    const int sx = blockIdx.x * kPlainTile + threadIdx.x;
    const int sy = (tileRow0 + blockIdx.y) * kPlainTile + threadIdx.y;
    if (sx >= r.W || sy >= r.H) return;
    const double g = adjoint_plain_gather<MODE>(r, sx, sy, n + (int64_t)blockIdx.z * r.dH * r.dW);
    gsrc[(int64_t)blockIdx.z * sv.imageStride + (int64_t)sy * sv.rowStride + sx] = (float)g;
}

// list: room for `capacity` entries, cursor: one zeroed word.  Only enqueues.
hipError_t launch_adjoint_knife_list(const RotLaunch &r, const unsigned char *knife, uint2 *list, unsigned *cursor, unsigned capacity, hipStream_t stream)
{
    if (r.dW <= 0 || r.dH <= 0 || !capacity) return hipSuccess;
    const dim3 block(kPlainTile, kPlainTile, 1);
    const int tileRows = (r.dH + kPlainTile - 1) / kPlainTile;
    for (int t0 = 0; t0 < tileRows; t0 += 65535) {
        const dim3 grid((r.dW + kPlainTile - 1) / kPlainTile, tileRows - t0 < 65535 ? tileRows - t0 : 65535, 1);
        hipLaunchKernelGGL(aai_adjoint_knife_list_kernel, grid, block, 0, stream, knife, r.dW, r.dH, list, cursor, capacity, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// `batch` images (at most 65535: grid.z); S: the plan's sums; n holds batch x dH x dW doubles.  Only enqueues.
hipError_t launch_adjoint_plain(const RotLaunch &r, int batch, const float *gdst, ImageView dv, const double *S, double *n, float *gsrc, ImageView sv,
                                hipStream_t stream, const char **kernelName)
{
    if (kernelName) *kernelName = r.mode == AAI_MODE_FAST ? "aai_adjoint_plain_gather_kernel<fast>" : "aai_adjoint_plain_gather_kernel<area>";
    if (batch <= 0 || r.dW <= 0 || r.dH <= 0 || r.W <= 0 || r.H <= 0) return hipSuccess;
    const int dstTileRows = (r.dH + kScaleRows - 1) / kScaleRows, srcTileRows = (r.H + kPlainTile - 1) / kPlainTile;
    for (int t0 = 0; t0 < dstTileRows; t0 += 65535) {
        const dim3 block(kScaleCols, kScaleRows, 1);
        const dim3 grid((r.dW + kScaleCols - 1) / kScaleCols, dstTileRows - t0 < 65535 ? dstTileRows - t0 : 65535, batch);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_scale_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r.dW, r.dH, S, gdst, dv, n, t0);
        else hipLaunchKernelGGL(aai_adjoint_scale_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r.dW, r.dH, S, gdst, dv, n, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (int t0 = 0; t0 < srcTileRows; t0 += 65535) {
        const dim3 block(kPlainTile, kPlainTile, 1);
        const dim3 grid((r.W + kPlainTile - 1) / kPlainTile, srcTileRows - t0 < 65535 ? srcTileRows - t0 : 65535, batch);
        if (r.mode == AAI_MODE_FAST) hipLaunchKernelGGL(aai_adjoint_plain_gather_kernel<AAI_MODE_FAST>, grid, block, 0, stream, r, n, gsrc, sv, t0);
        else hipLaunchKernelGGL(aai_adjoint_plain_gather_kernel<AAI_MODE_AREA>, grid, block, 0, stream, r, n, gsrc, sv, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace aai
