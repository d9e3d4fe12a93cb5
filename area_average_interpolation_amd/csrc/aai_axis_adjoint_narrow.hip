// aai_axis_adjoint_narrow.hip -- the transpose of the separable axis-aligned kernel on HALF-PRECISION gradients
// (include/aai_adjoint_half.h): gsrc = narrow(W^T widen(gdst)) at rotations by multiples of 90 degrees, fp16 / bf16 images of raw 16-bit
// elements with 1..4 interleaved channels in and out, no fp32 image anywhere.
//
// The structure is that of aai_axis_adjoint_multi_kernel<C> (aai_axis_adjoint_multi.hip; for C = 1 of aai_axis_adjoint_kernel, which has
// the derivation): the tables of the forward's SINGLE-channel plan and their inverse ranges, one lane per ELEMENT e = sx * C + c of a
// source row, a workgroup of 256 elements walks 32 source rows downwards and holds the horizontal sums of the last two kb in registers.
// The per-lane arithmetic is adjoint_half_lane (aai_axis_adjoint_half_math.hpp, shared with the CPU replay of the tests): the fp32
// kernel's weights and fused multiply-adds in its order, every gdst element widened exactly on load, the finished sum rounded ONCE on
// store.  The output therefore has the bits of narrow(fp32 kernel(widen(gdst))) by construction.
// elem(ka, kb, c) = outBase + ka outStrideA + kb outStrideB + c with PIXEL strides: all four quadrants, flips and the dst stride are in
// that mapping, which the engine computes.  No LDS, no atomics, int64 addressing, every element of gsrc written exactly once (zeros
// included) by a 2-byte store: base pointers and strides need 2-byte alignment and nothing more.  Image b of a batch (grid z) gets the
// bits of a single-image call.
#include "aai_kernels.hpp"
#include "aai_axis_adjoint_half_math.hpp"

namespace aai {

constexpr int kAxisAdjHalfElems = 256;    // source-row elements per workgroup (4 waves)
constexpr int kAxisAdjHalfRows = 32;      // source rows per workgroup: kAxisAdjRows of aai_axis_adjoint.hip

template <int HT, int C>
__global__ __launch_bounds__(kAxisAdjHalfElems) void aai_axis_adjoint_half_kernel(AxisAdjointLaunch a, const uint16_t *__restrict__ gdst, ImageView dv,
                                                                                 uint16_t *__restrict__ gsrc, ImageView sv, int rowBlock0)
{
    const int e = blockIdx.x * kAxisAdjHalfElems + threadIdx.x;      // (a.srcW * C <= INT32_MAX / 2: the entries check the row length)
    if (e >= a.srcW * C) return;
    const int sx = e / C, ch = e - sx * C;
    const int sy0 = (rowBlock0 + (int)blockIdx.y) * kAxisAdjHalfRows;
    const int sy1 = sy0 + kAxisAdjHalfRows < a.srcH ? sy0 + kAxisAdjHalfRows : a.srcH;
    const uint16_t *gd = gdst + (int64_t)blockIdx.z * dv.imageStride + a.outBase + ch;
    uint16_t *gs = gsrc + (int64_t)blockIdx.z * sv.imageStride + e;
    adjoint_half_lane<HT>(a.laneTab, a.rowTab, a.colRange[sx], a.rowRange, sx, sy0, sy1, gd, a.outStrideA, a.outStrideB, gs, sv.rowStride);
}

template <int HT, int C>
static hipError_t launch_axis_adjoint_half_as(const AxisAdjointLaunch &a, int batch, const uint16_t *gdst, ImageView dv, uint16_t *gsrc, ImageView sv,
                                              hipStream_t stream)
{
    const int rowBlocks = (a.srcH + kAxisAdjHalfRows - 1) / kAxisAdjHalfRows;
    const int64_t rowLen = (int64_t)a.srcW * C;
    for (int b0 = 0; b0 < rowBlocks; b0 += 65535) {            // grid.y carries at most 65535 row blocks
        const dim3 grid((unsigned)((rowLen + kAxisAdjHalfElems - 1) / kAxisAdjHalfElems), rowBlocks - b0 < 65535 ? rowBlocks - b0 : 65535, batch);
        hipLaunchKernelGGL((aai_axis_adjoint_half_kernel<HT, C>), grid, dim3(kAxisAdjHalfElems, 1, 1), 0, stream, a, gdst, dv, gsrc, sv, b0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int HT>
static hipError_t launch_axis_adjoint_half_of(const AxisAdjointLaunch &a, int channels, int batch, const uint16_t *gdst, ImageView dv, uint16_t *gsrc,
                                              ImageView sv, hipStream_t stream)
{
    switch (channels) {
    case 1: return launch_axis_adjoint_half_as<HT, 1>(a, batch, gdst, dv, gsrc, sv, stream);
    case 2: return launch_axis_adjoint_half_as<HT, 2>(a, batch, gdst, dv, gsrc, sv, stream);
    case 3: return launch_axis_adjoint_half_as<HT, 3>(a, batch, gdst, dv, gsrc, sv, stream);
    default: return launch_axis_adjoint_half_as<HT, 4>(a, batch, gdst, dv, gsrc, sv, stream);
    }
}

// `type`: NARROW_F16 / NARROW_BF16; `channels` in 1..4; a.srcW / a.srcH in PIXELS, a.outBase / outStrideA / outStrideB the mapping of PIXELS
// onto elements of gdst; `batch` images (at most 65535: grid.z).  Only enqueues.
hipError_t launch_axis_adjoint_half(const AxisAdjointLaunch &a, int type, int channels, int batch, const void *gdst, ImageView dv, void *gsrc, ImageView sv,
                                    hipStream_t stream, const char **kernelName)
{
    static const char *const names[2][4] = {
        {"aai_axis_adjoint_half_kernel<f16,1>", "aai_axis_adjoint_half_kernel<f16,2>", "aai_axis_adjoint_half_kernel<f16,3>", "aai_axis_adjoint_half_kernel<f16,4>"},
        {"aai_axis_adjoint_half_kernel<bf16,1>", "aai_axis_adjoint_half_kernel<bf16,2>", "aai_axis_adjoint_half_kernel<bf16,3>", "aai_axis_adjoint_half_kernel<bf16,4>"}};
    if (!narrow_is_half(type) || channels < 1 || channels > 4) return hipErrorInvalidValue;      // (the engine never asks for anything else)
    if (kernelName) *kernelName = names[type == NARROW_F16 ? 0 : 1][channels - 1];
    if (batch <= 0 || a.srcW <= 0 || a.srcH <= 0) return hipSuccess;
    const uint16_t *gd = static_cast<const uint16_t *>(gdst);
    uint16_t *gs = static_cast<uint16_t *>(gsrc);
    return type == NARROW_F16 ? launch_axis_adjoint_half_of<HALF_F16>(a, channels, batch, gd, dv, gs, sv, stream)
                              : launch_axis_adjoint_half_of<HALF_BF16>(a, channels, batch, gd, dv, gs, sv, stream);
}

}  // namespace aai
