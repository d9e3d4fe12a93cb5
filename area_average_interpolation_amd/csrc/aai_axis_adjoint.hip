// aai_axis_adjoint.hip -- the transpose of the separable axis-aligned kernel K1 (aai_axis.hip): gsrc = W^T gdst at rotations by
// multiples of 90 degrees, from the forward plan's own tables.
//
// With the forward's tables dst pixel (ka, kb) = sum over sy in the row window of kb and sx in the lane window of ka of
// wrow(kb, sy) wlane(ka, sx) src[sy][sx].  Windows are monotone in the output index, so the outputs whose window holds a source
// index are one range [k0, k1] (AxisRange, inverted and checked on the host: build_axis_adjoint_ranges), and
//
//     gsrc[sy][sx] = sum over kb in R(sy) of wrow(kb, sy) * t(kb, sx),   t(kb, sx) = sum over ka in C(sx) of wlane(ka, sx) gdst[elem(ka, kb)]
//
// elem(ka, kb) = outBase + ka outStrideA + kb outStrideB is the forward's own mapping (make_axis_launch): quadrants, flips and the dst
// stride are in it, and the integer pre-expansion is in the tables.  No geometry is computed here.
//
// One lane per source column, a workgroup of 256 columns walks kAxisAdjRows source rows downwards.  Consecutive source rows share
// their kb range (4 rows per kb at 4:1), so the horizontal sums t(kb, .) of the last two kb stay in registers and are computed once
// per workgroup and kb; the row table and the row ranges are uniform over the workgroup (scalar loads).  A wave stores 256
// contiguous bytes per source row and reads gdst through the caches (at most a quarter of gsrc when down-sampling).  No LDS, no
// atomics, every element of gsrc written exactly once by one lane in a fixed summation order (ka ascending inside kb ascending), fp32
// fused multiply-adds: deterministic, and image b of a batch (grid z) gets the bits of a single-image call.  A cached t is the
// value the lane would compute again, so the grouping of rows into workgroups does not show in the bits.
#include "aai_kernels.hpp"

namespace aai {

constexpr int kAxisAdjCols = 256;     // source columns per workgroup (4 waves)
constexpr int kAxisAdjRows = 32;      // source rows per workgroup

// the weight of source index s within the window of entry e (s0 <= s <= s1): the rule of AxisEntry, s0 == s1 included
__device__ __forceinline__ float axis_entry_weight(int s0, int s1, float wFirst, float wMid, float wLast, int s)
{
    return s == s0 ? wFirst : (s == s1 ? wLast : wMid);
}

__global__ __launch_bounds__(kAxisAdjCols) void aai_axis_adjoint_kernel(AxisAdjointLaunch a, const float *__restrict__ gdst, ImageView dv,
                                                                        float *__restrict__ gsrc, ImageView sv, int rowBlock0)
{
    const int sx = blockIdx.x * kAxisAdjCols + threadIdx.x;
    if (sx >= a.srcW) return;
    const int sy0 = (rowBlock0 + (int)blockIdx.y) * kAxisAdjRows;
    const int sy1 = sy0 + kAxisAdjRows < a.srcH ? sy0 + kAxisAdjRows : a.srcH;
    const float *gd = gdst + (int64_t)blockIdx.z * dv.imageStride + a.outBase;
    float *gs = gsrc + (int64_t)blockIdx.z * sv.imageStride + sx;
    const AxisRange c = a.colRange[sx];

    // t(kb, sx) for one kb: ka ascending
    auto horizontal = [&](int kb) -> float {
        const float *g = gd + (int64_t)kb * a.outStrideB;
        float t = 0.f;
        for (int ka = c.k0; ka <= c.k1; ++ka) {
            const AxisEntry e = a.laneTab[ka];
            t = fmaf(axis_entry_weight(e.s0, e.s1, e.wFirst, e.wMid, e.wLast, sx), g[(int64_t)ka * a.outStrideA], t);
        }
        return t;
    };

    int kOld = -1, kNew = -1;         // the two most recent kb whose horizontal sums are held
    float tOld = 0.f, tNew = 0.f;
    for (int sy = sy0; sy < sy1; ++sy) {
        const AxisRange rr = a.rowRange[sy];
        float acc = 0.f;
        for (int kb = rr.k0; kb <= rr.k1; ++kb) {
            const AxisEntry e = a.rowTab[kb];
            float t;
            if (kb == kNew) t = tNew;
            else if (kb == kOld) t = tOld;
            else {
                t = horizontal(kb);
                kOld = kNew; tOld = tNew; kNew = kb; tNew = t;
            }
            acc = fmaf(axis_entry_weight(e.s0, e.s1, e.wFirst, e.wMid, e.wLast, sy), t, acc);
        }
        gs[(int64_t)sy * sv.rowStride] = acc;      // (an empty range: no dst pixel reads this source pixel, 0 is written)
    }
}

// `batch` images (at most 65535: grid.z).  Only enqueues.
hipError_t launch_axis_adjoint(const AxisAdjointLaunch &a, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv,
                               hipStream_t stream, const char **kernelName)
{
    if (kernelName) *kernelName = "aai_axis_adjoint_kernel";
    if (batch <= 0 || a.srcW <= 0 || a.srcH <= 0) return hipSuccess;
    const int rowBlocks = (a.srcH + kAxisAdjRows - 1) / kAxisAdjRows;
    for (int b0 = 0; b0 < rowBlocks; b0 += 65535) {            // grid.y carries at most 65535 row blocks
        const dim3 grid((a.srcW + kAxisAdjCols - 1) / kAxisAdjCols, rowBlocks - b0 < 65535 ? rowBlocks - b0 : 65535, batch);
        hipLaunchKernelGGL(aai_axis_adjoint_kernel, grid, dim3(kAxisAdjCols, 1, 1), 0, stream, a, gdst, dv, gsrc, sv, b0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace aai
