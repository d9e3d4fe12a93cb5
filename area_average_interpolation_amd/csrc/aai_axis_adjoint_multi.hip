// aai_axis_adjoint_multi.hip -- the transpose of the separable axis-aligned kernel for images with 2..4 interleaved channels
// (aai_adjoint_planned_interleaved_*): gsrc = W^T gdst per channel at rotations by multiples of 90 degrees, from the tables of the
// forward's SINGLE-channel plan -- laneTab, rowTab and their inverse ranges know pixels, not channels, so every channel count shares
// them and nothing is added to a plan.
//
// The structure is that of aai_axis_adjoint_kernel (aai_axis_adjoint.hip, which has the derivation): a workgroup of 256 lanes walks
// kAxisAdjMultiRows source rows downwards and holds the horizontal sums of the last two kb in registers.  Here a lane owns one
// ELEMENT e = sx * C + c of the source row instead of one column:
//   - the pixel sx = e / C (C is a template constant: a multiply and a shift) indexes colRange and the weight test, the channel
//     c = e % C is an offset into gdst and nothing else;
//   - a wave loads and stores 64 consecutive floats of a row for C = 3 too.  Strides are any number of elements, so nothing wider
//     than 4 bytes is aligned (aai_adjoint_scale_multi_kernel made the same choice for the same reason);
//   - lane e executes, operation for operation, what aai_axis_adjoint_kernel executes for column sx of plane c: the same weights,
//     the same fmaf in the same order (ka ascending inside kb ascending).  Channel c therefore has the bits the single-channel
//     kernel gives plane c, by construction.  The C lanes of a pixel compute the same weights C times; a lane-per-pixel form that
//     shares them is a different kernel (profiles/adjoint_axis_interleaved_time.txt has the figures to judge it by).
// elem(ka, kb, c) = outBase + ka outStrideA + kb outStrideB + c with PIXEL strides (the engine computes them: a dst pixel is C elements
// wide).  No LDS, no atomics, every element of gsrc written exactly once (zeros included): deterministic, image b of a batch
// (grid z) gets the bits of a single-image call.
#include "aai_kernels.hpp"

namespace aai {

constexpr int kAxisAdjMultiElems = 256;    // source-row elements per workgroup (4 waves)
constexpr int kAxisAdjMultiRows = 32;      // source rows per workgroup: kAxisAdjRows of aai_axis_adjoint.hip

// the weight of source index s within the window of an entry (s0 <= s <= s1): the rule of AxisEntry, s0 == s1 included
__device__ __forceinline__ float axis_entry_weight_multi(int s0, int s1, float wFirst, float wMid, float wLast, int s)
{
    return s == s0 ? wFirst : (s == s1 ? wLast : wMid);
}

template <int C>
__global__ __launch_bounds__(kAxisAdjMultiElems) void aai_axis_adjoint_multi_kernel(AxisAdjointLaunch a, const float *__restrict__ gdst, ImageView dv,
                                                                                   float *__restrict__ gsrc, ImageView sv, int rowBlock0)
{
    const int e = blockIdx.x * kAxisAdjMultiElems + threadIdx.x;      // (a.srcW * C <= INT32_MAX / 2: the entries check the row length)
    if (e >= a.srcW * C) return;
    const int sx = e / C, ch = e - sx * C;
    const int sy0 = (rowBlock0 + (int)blockIdx.y) * kAxisAdjMultiRows;
    const int sy1 = sy0 + kAxisAdjMultiRows < a.srcH ? sy0 + kAxisAdjMultiRows : a.srcH;
    const float *gd = gdst + (int64_t)blockIdx.z * dv.imageStride + a.outBase + ch;
    float *gs = gsrc + (int64_t)blockIdx.z * sv.imageStride + e;
    const AxisRange c = a.colRange[sx];

    // t(kb, sx) of this lane's channel for one kb: ka ascending
    auto horizontal = [&](int kb) -> float {
        const float *g = gd + (int64_t)kb * a.outStrideB;
        float t = 0.f;
        for (int ka = c.k0; ka <= c.k1; ++ka) {
            const AxisEntry en = a.laneTab[ka];
            t = fmaf(axis_entry_weight_multi(en.s0, en.s1, en.wFirst, en.wMid, en.wLast, sx), g[(int64_t)ka * a.outStrideA], t);
        }
        return t;
    };

    int kOld = -1, kNew = -1;         // the two most recent kb whose horizontal sums are held
    float tOld = 0.f, tNew = 0.f;
    for (int sy = sy0; sy < sy1; ++sy) {
        const AxisRange rr = a.rowRange[sy];
        float acc = 0.f;
        for (int kb = rr.k0; kb <= rr.k1; ++kb) {
            const AxisEntry en = a.rowTab[kb];
            float t;
            if (kb == kNew) t = tNew;
            else if (kb == kOld) t = tOld;
            else {
                t = horizontal(kb);
                kOld = kNew; tOld = tNew; kNew = kb; tNew = t;
            }
            acc = fmaf(axis_entry_weight_multi(en.s0, en.s1, en.wFirst, en.wMid, en.wLast, sy), t, acc);
        }
        gs[(int64_t)sy * sv.rowStride] = acc;      // (an empty range: no dst pixel reads this source pixel, 0 is written)
    }
}

template <int C>
static hipError_t launch_axis_adjoint_multi_as(const AxisAdjointLaunch &a, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv,
                                               hipStream_t stream)
{
    const int rowBlocks = (a.srcH + kAxisAdjMultiRows - 1) / kAxisAdjMultiRows;
    const int64_t rowLen = (int64_t)a.srcW * C;
    for (int b0 = 0; b0 < rowBlocks; b0 += 65535) {            // grid.y carries at most 65535 row blocks
        const dim3 grid((unsigned)((rowLen + kAxisAdjMultiElems - 1) / kAxisAdjMultiElems), rowBlocks - b0 < 65535 ? rowBlocks - b0 : 65535, batch);
        hipLaunchKernelGGL(aai_axis_adjoint_multi_kernel<C>, grid, dim3(kAxisAdjMultiElems, 1, 1), 0, stream, a, gdst, dv, gsrc, sv, b0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// `channels` in 2..4; a.srcW / a.srcH in PIXELS, a.outBase / outStrideA / outStrideB the mapping of PIXELS onto elements of gdst; `batch`
// images (at most 65535: grid.z).  Only enqueues.
hipError_t launch_axis_adjoint_multi(const AxisAdjointLaunch &a, int channels, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv,
                                     hipStream_t stream, const char **kernelName)
{
    static const char *const names[3] = {"aai_axis_adjoint_multi_kernel<2>", "aai_axis_adjoint_multi_kernel<3>", "aai_axis_adjoint_multi_kernel<4>"};
    if (channels < 2 || channels > 4) return hipErrorInvalidValue;      // (1 channel is launch_axis_adjoint's; the engine never asks for another count)
    if (kernelName) *kernelName = names[channels - 2];
    if (batch <= 0 || a.srcW <= 0 || a.srcH <= 0) return hipSuccess;
    switch (channels) {
    case 2: return launch_axis_adjoint_multi_as<2>(a, batch, gdst, dv, gsrc, sv, stream);
    case 3: return launch_axis_adjoint_multi_as<3>(a, batch, gdst, dv, gsrc, sv, stream);
    default: return launch_axis_adjoint_multi_as<4>(a, batch, gdst, dv, gsrc, sv, stream);
    }
}

}  // namespace aai
