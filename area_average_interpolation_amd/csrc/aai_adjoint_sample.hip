// aai_adjoint_sample.hip -- the adjoint (transposed) resampling of the bilinear / bicubic samplers: gsrc = W^T gdst.
//
// Compiled with -ffp-contract=off (see the Makefile): the per-pixel body lives in aai_adjoint_sample_math.hpp and is shared with the CPU
// replay of the test-suite, and channel c of an interleaved call must get the bits of the single-channel call on plane c.
//
// One kernel, a gather, no atomics, every element of gsrc written exactly once (zeros included): deterministic, and image b of a batch
// gets the bits a single-image call gives it.  One lane per SOURCE pixel; a wave covers 64 consecutive X of one source row, so that a
// wave's stores are whole lines, and the four waves of a workgroup take four consecutive rows: their candidate dst pixels overlap in L1.
// Templated on the mode and the channel count 1..4: a candidate's weight is computed once and serves every channel.
// No scratch, no plan, no side stream: one launch per 65535 x 4 source rows on the caller's stream.
#include "aai_kernels.hpp"
#include "aai_adjoint_sample_math.hpp"

namespace aai {

namespace {

constexpr int kAdjSampleCols = 64, kAdjSampleRows = 4;      // workgroup = 64 x 4 source pixels, one wave per row
constexpr int kMaxGridY = 65535;

template <int MODE, int C>
__global__ __launch_bounds__(kAdjSampleCols *kAdjSampleRows) void aai_adjoint_sample_kernel(AdjSampleLaunch a, const float *__restrict__ gdst, ImageView dv,
                                                                                           float *__restrict__ gsrc, ImageView sv, int tileRow0)
{
    const int X = blockIdx.x * kAdjSampleCols + threadIdx.x;
    const int Y = (tileRow0 + blockIdx.y) * kAdjSampleRows + threadIdx.y;
    if (X >= a.r.W || Y >= a.r.H) return;
    double acc[C];
    adjoint_sample_gather<MODE, C>(a, X, Y, gdst + (int64_t)blockIdx.z * dv.imageStride, dv.rowStride, acc, AdjSampleNoVisit());
    float *out = gsrc + (int64_t)blockIdx.z * sv.imageStride + (int64_t)Y * sv.rowStride + (int64_t)X * C;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = (float)acc[c];
}

template <int MODE, int C>
hipError_t launch_typed(const AdjSampleLaunch &a, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv, hipStream_t stream)
{
    const dim3 block(kAdjSampleCols, kAdjSampleRows, 1);
    const int tileRows = (a.r.H + kAdjSampleRows - 1) / kAdjSampleRows;
    for (int t0 = 0; t0 < tileRows; t0 += kMaxGridY) {          // grid.y carries at most 65535 tile rows
        const dim3 grid((a.r.W + kAdjSampleCols - 1) / kAdjSampleCols, std::min(tileRows - t0, kMaxGridY), batch);
        hipLaunchKernelGGL((aai_adjoint_sample_kernel<MODE, C>), grid, block, 0, stream, a, gdst, dv, gsrc, sv, t0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int MODE>
hipError_t launch_mode(const AdjSampleLaunch &a, int channels, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv, hipStream_t stream)
{
    switch (channels) {
    case 1: return launch_typed<MODE, 1>(a, batch, gdst, dv, gsrc, sv, stream);
    case 2: return launch_typed<MODE, 2>(a, batch, gdst, dv, gsrc, sv, stream);
    case 3: return launch_typed<MODE, 3>(a, batch, gdst, dv, gsrc, sv, stream);
    case 4: return launch_typed<MODE, 4>(a, batch, gdst, dv, gsrc, sv, stream);
    default: return hipErrorInvalidValue;
    }
}

const char *kernel_name(int mode, int channels)
{
    static const char *const names[2][4] = {
        {"aai_adjoint_sample_kernel<bilinear>", "aai_adjoint_sample_kernel<bilinear, 2 channels>", "aai_adjoint_sample_kernel<bilinear, 3 channels>",
         "aai_adjoint_sample_kernel<bilinear, 4 channels>"},
        {"aai_adjoint_sample_kernel<bicubic>", "aai_adjoint_sample_kernel<bicubic, 2 channels>", "aai_adjoint_sample_kernel<bicubic, 3 channels>",
         "aai_adjoint_sample_kernel<bicubic, 4 channels>"}};
    return names[mode == AAI_MODE_BICUBIC ? 1 : 0][channels >= 1 && channels <= 4 ? channels - 1 : 0];
}

}  // namespace

// `batch` images (at most 65535: grid.z) of `channels` = 1..4 interleaved channels.  Only enqueues.
hipError_t launch_adjoint_sample_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv,
                                       hipStream_t stream, const char **kernelName)
{
    if (kernelName) *kernelName = kernel_name(r.mode, channels);
    if (r.mode != AAI_MODE_BILINEAR && r.mode != AAI_MODE_BICUBIC) return hipErrorInvalidValue;
    if (batch <= 0 || r.dW <= 0 || r.dH <= 0 || r.W <= 0 || r.H <= 0) return hipSuccess;
    const AdjSampleLaunch a = make_adjoint_sample_launch(r);
    return r.mode == AAI_MODE_BILINEAR ? launch_mode<AAI_MODE_BILINEAR>(a, channels, batch, gdst, dv, gsrc, sv, stream)
                                       : launch_mode<AAI_MODE_BICUBIC>(a, channels, batch, gdst, dv, gsrc, sv, stream);
}

hipError_t launch_adjoint_sample(const RotLaunch &r, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv, hipStream_t stream,
                                 const char **kernelName)
{
    return launch_adjoint_sample_multi(r, 1, batch, gdst, dv, gsrc, sv, stream, kernelName);
}

}  // namespace aai
