// aai_engine.hpp -- host-side engine behind the C ABI (aai_engine.cpp): error state, request checks, plan cache, dispatch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "aai_kernels.hpp"

namespace aai {
namespace engine {

// per-thread texts behind aai_last_error() / aai_last_kernel()
extern thread_local std::string g_lastError;
extern thread_local std::string g_lastKernel;
int fail(int code, const std::string &msg);                 // records msg, returns code
int hip_fail(hipError_t e, const char *what);               // AAI_ERR_NO_DEVICE for a missing / unusable device, else AAI_ERR_HIP

#define AAI_HIP(call)                                                     \
    do {                                                                  \
        hipError_t e__ = (call);                                          \
        if (e__ != hipSuccess) return ::aai::engine::hip_fail(e__, #call); \
    } while (0)

struct Plan {
    aai_request key{};
    int band0 = -1, band1 = -1;      // dst row band this plan serves (-1: the whole image)
    int channels = 1;                // interleaved channels the K1 tables were built for
    int form = 0;                    // rotated area / fast requests: the fp32 formulation whose scan flagged the pixels (aai::RotForm)
    int srcRow0 = 0, srcRow1 = 0;     // source rows the band reads; the source pointer addresses row srcRow0
    int device = -1;
    aai::Geometry g;
    int kernel = 0;
    // K1
    aai::AxisTables tabs;
    aai::AxisEntry *dLane = nullptr, *dRow = nullptr;
    aai::AxisStrip *dStrips = nullptr;
    int tuneRows = 0, tuneNt = 0;                     // K1 launch shape for this device (0 rows = built-in default)
    int tuneSource = 0;                               // 0 = built-in default, 1 = measured for this plan, 2 = taken from the per-class cache
    // K2/K3: the dst pixels flagged by the one-off scans (knife edges of the reference's classifier; decisions the fp32
    // kernels leave to double precision) as a list of (dx, dy) the fix-up pass runs over; `dense` when there are
    // so many that the whole image takes that pass instead
    void *dList = nullptr;
    unsigned flaggedPixels = 0;
    bool dense = false;
    // fp32 rotated kernels: the lane masks of the flagged pixels (they skip them; the fix-up pass runs beside them on a side stream of
    // the device's pool)
    void *dScan = nullptr;           // ONE allocation: lane masks | tile flags | the scans' counter
    unsigned long long *dMasks = nullptr;      // (into dScan)
    unsigned *dTileFlags = nullptr;  // (into dScan) one bit per 16 x 16 tile with a flagged pixel (aai::launch_tile_flags), tileFlagWords words per tile row
    int tileFlagWords = 0;
    int *dLive = nullptr;            // per-pixel kernels on a rotated canvas: live tile span per tile row (aai::rotated_live_spans), or none
    // the transposed K1 (aai_adjoint_planned_*): built by the first planned adjoint of the plan or by aai_adjoint_prepare, under `build`.
    // adjState: 0 = not asked for yet, 1 = tables on the device, 2 = this plan keeps the general adjoint (wide or dense plan, a
    // table the inversion's check refuses, a correction list that would cover most of the image)
    int adjState = 0;
    aai::AxisRange *dColRange = nullptr, *dRowRange = nullptr;
    void *dAdjSrcList = nullptr, *dAdjDstList = nullptr;      // uint2 (x, y): the source pixels the general adjoint recomputes, the dst pixels it reads
    unsigned adjSrcCount = 0, adjDstCount = 0;
    // the planned adjoint at general rotations (aai_adjoint_rotated_*; rotated area / fast plans): built by its first call of the plan or by
    // aai_adjoint_rotated_prepare, under `build`.  rotAdjState: 0 = not asked for yet, 1 = sums on the device, 2 = this plan keeps the
    // general adjoint (too many knife pixels, a source list over more than half of the image, sums beyond 1 GiB).  The source pixels the
    // general gather recomputes are dAdjSrcList / adjSrcCount above (an axis plan never holds these tables, a rotated plan never those).
    int rotAdjState = 0;
    double *dAdjSums = nullptr;      // fp64 [dH][dW]: 8 bytes per dst pixel
    long long adjKnife = -1;         // dst pixels with a knife-edge pair (-1: not counted)
    double buildMs = 0.0;            // wall clock of build_plan (tables, scans, launch-shape measurement)
    // Built once, by whoever gets here first, under `build` -- NOT under the cache's lock: other requests, other devices
    // and other threads are not held up by this plan's scans or launch-shape measurement.  `launch` serialises the launches of a
    // plan between caller threads.
    std::mutex build, launch;
    bool built = false;
    int buildRc = AAI_OK;
    std::string buildError;
    ~Plan()
    {
        if (dScan) (void)hipFree(dScan);
        if (dLive) (void)hipFree(dLive);
        if (dList) (void)hipFree(dList);
        if (dLane) (void)hipFree(dLane);
        if (dRow) (void)hipFree(dRow);
        if (dStrips) (void)hipFree(dStrips);
        if (dColRange) (void)hipFree(dColRange);
        if (dRowRange) (void)hipFree(dRowRange);
        if (dAdjSrcList) (void)hipFree(dAdjSrcList);
        if (dAdjDstList) (void)hipFree(dAdjDstList);
        if (dAdjSums) (void)hipFree(dAdjSums);
    }
};
typedef std::shared_ptr<Plan> PlanRef;

// Streams and events the engine needs beside the callers' own, ONE set per device and process, created on first need: creating a
// stream costs 2.7 ... 5 ms of host time on this platform (a hardware queue each; profiles/r04_plan_time.txt), which at one private
// stream and four side streams per PLAN was 16 of the 19 ms a first rotated call took.
//   build   aai_prepare's stream (the resampling entry points build a missing plan on the CALLER's stream instead)
//   side[]  the fix-up pass beside a production kernel that skips the plan's listed pixels: dealt round-robin per launch, each with
//           its fork / join events, so that the passes of callers on different streams run beside each other.  Created by the SECOND
//           launch that wants them: a process that makes one call (the reference's user, Source.cpp:1565) runs its pass behind the
//           production kernel (~10 us) and never pays the ~11 ms.
// `m` guards creation and the slot rotation and is held while a launch with a pass beside it is being enqueued (fork ... join).
struct DevicePool {
    static constexpr int kSideSlots = 4;
    std::mutex m;
    hipStream_t build = nullptr;
    hipStream_t side[kSideSlots] = {};
    hipEvent_t fork[kSideSlots] = {}, join[kSideSlots] = {};
    bool sideReady = false, sideFailed = false;
    unsigned besideLaunches = 0, nextSide = 0;
    // the adjoint's scratch (for_each_adjoint_chunk behind enqueue_adjoint): a memory pool of the library's own, created on the first adjoint call of the device.
    // It keeps what it has been given (release threshold: everything), so that after the first call of a size an allocation is
    // stream-ordered bookkeeping and never a trip to the driver -- the device's default pool hands its memory back at every
    // synchronisation.  aai_shutdown destroys it.
    hipMemPool_t scratch = nullptr;
};
DevicePool &device_pool(int device);      // (heap, never destroyed; aai_shutdown releases the streams while the runtime is alive)

// The cache (most recently used first) lives on the heap and is never destroyed: a static destructor would call into HIP
// after the runtime's own teardown.  aai_shutdown() empties it while the runtime is alive.
extern std::mutex g_planMutex;          // guards the cache's structure only; never held across device work
std::list<PlanRef> &plan_cache();
void drop_plans();

bool same_request(const aai_request &a, const aai_request &b);
int check_request(const aai_request *rq);
int axis_band_margin(const aai_request &rq);                 // extra source rows either side of a K1 row band (fix-up pass)
int pick_kernel(const aai_request &rq, const Geometry &g);
int resolved_kernel(const aai_request &rq, const Geometry &g);      // pick_kernel, with AXIS -> AXIS_WIDE where the tables say so
void fill_layout(const Geometry &g, int kernel, aai_layout *out);
int require_device();

// Finds the plan for (request, current device) or inserts a fresh one, then builds it if nobody has (blocking: table
// uploads, the one-off scans, K1's launch-shape measurement -- on `stream` when the caller has one to give (onCallerStream; a
// stream that is being captured into a graph is not used), else on the device pool's build stream).
// form: aai::RotForm of a rotated request's launch (rot_form below); ignored by the other kernels
int acquire_plan(const aai_request &rq, const Geometry &g, int band0, int band1, int channels, int form, PlanRef *out, bool onCallerStream = false, hipStream_t stream = nullptr);
// "kernel=K rows=R nt=N swap=0 tune=T order=banded|launch flagged=F dense=D form=M build_ms=B adjoint=tables|none rot_adjoint=none|sums|general[ knife=N]" of the
// cached whole-image plan ("" when there is none); new tokens are appended at the end
std::string plan_description(const aai_request &rq, int channels);
// which fp32 formulation serves a launch of this request: the cell formulation takes plain images below 4 GiB in area mode
int rot_form(const aai_request &rq, const Geometry &g, int channels, int srcType, int64_t srcStride);

// Enqueues one batched launch (plus the fix-up pass where the plan has one) on `stream`.  g: the request's geometry (make_geometry,
// which the caller ran to validate the request).  Strides in elements.
int enqueue(const aai_request &rq, const Geometry &g, int batch, const void *dSrc, int srcType, int64_t srcStride, int64_t srcImageStride,
            float *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream, int band0 = -1, int band1 = -1,
            int channels = 1);

// grid.z carries the batch of a launch
constexpr int kMaxGridZ = 65535;

// How many images of a batch the adjoint takes per round of launches: all that grid.z carries, cut so that their fp64 scratch of
// imageBytes each stays within 1 GiB (imageBytes == 0: the launches need no scratch); at least one.
inline int chunk_images(int batch, size_t imageBytes)
{
    size_t chunk = (size_t)std::max(0, std::min(batch, kMaxGridZ));
    if (imageBytes) chunk = std::min(chunk, ((size_t)1 << 30) / imageBytes);
    return (int)std::max<size_t>(1, chunk);
}

// The adjoint of an area / fast request, every entry's (aai_adjoint_*; the caller has checked the arguments): gsrc = W^T gdst for
// `batch` images of `channels` = 1..4 interleaved channels, element (x, y, c) of image b at b * imageStride + y * stride + x * channels
// + c, strides in elements.  `family` is what the entry asks for; which launches serve the call:
//
//   asked for   request / plan                                      served by
//   GENERAL     any                                                 GENERAL
//   PLANNED     not axis-aligned (or channels != 1)                 GENERAL
//               axis plan that is wide or dense, tables the         GENERAL
//               inversion refuses, lists over most of the image
//               (adjState 2)
//               axis plan with its adjoint tables (adjState 1)      PLANNED
//   ROTATED     reduced angle 0, one channel                        as PLANNED above
//               reduced angle 0, 2..4 channels                      GENERAL (the interleaved transposed separable kernel is SEPARABLE's)
//               plan that keeps the general adjoint (rotAdjState 2) GENERAL
//               plan with its sums (rotAdjState 1)                  ROTATED
//   SEPARABLE   one channel, or not axis-aligned                    as ROTATED above, line for line
//               axis-aligned, 2..4 channels: the single-channel     GENERAL
//               plan is wide or dense, ... (adjState 2)
//               the single-channel plan has its adjoint tables      SEPARABLE
//               (adjState 1)
//
//   GENERAL  no plan, nothing blocks: pass 1 and the gather of aai_adjoint.hip (one channel) or aai_adjoint_multi.hip (2..4; a pair's
//            weight computed once, channel c with the bits of plane c alone), fp64.
//   PLANNED  the forward's plan (the forward's key, built like aai_prepare builds it when missing) with its adjoint tables, then
//            aai_axis_adjoint_kernel (fp32, no scratch) and, where the plan has lists, the listed passes of the general adjoint behind
//            it: "aai_axis_adjoint_kernel+listed".
//   ROTATED  the forward's SINGLE-channel plan (same key; built like aai_prepare(req, 1) builds it) with its sums and source list, which
//            every channel count shares, then the element-wise pass 1 and the plain gather (aai_adjoint_plain.hip, or
//            aai_adjoint_plain_multi.hip with `channels` accumulators) and, where the plan lists source pixels, the general gather over
//            them: "<plain name>+listed".  The general adjoint's bits.
//
//   SEPARABLE  the forward's SINGLE-channel plan with the adjoint tables of PLANNED (the same tables: inverse ranges and lists know pixels,
//            not channels), then aai_axis_adjoint_multi_kernel<C> (aai_axis_adjoint_multi.hip: one lane per row element, fp32, no scratch)
//            and, where the plan has lists, the listed passes of the general multi-channel adjoint behind it
//            (launch_adjoint_listed_multi): "aai_axis_adjoint_multi_kernel<C>+listed".  Channel c has PLANNED's bits of plane c.
//
//   SAMPLE   (ADJOINT_SAMPLE: the entries of include/aai_adjoint_sample.h, bilinear / bicubic requests only -- the one family that takes
//            them, and it takes no other mode.)  No plan, no scratch, nothing blocks: aai_adjoint_sample_kernel (aai_adjoint_sample.hip), one
//            gather per source pixel in double precision, `channels` accumulators.  Never rerouted.
//
// A plan's tables are built on first need, under its `build` lock: that blocks; afterwards a call only enqueues.  The launches of
// PLANNED, SEPARABLE and ROTATED hold the plan's `launch` lock; GENERAL takes none.  Scratch: dW x dH x channels doubles per image in flight
// (PLANNED and SEPARABLE: only where there are lists, else none), stream-ordered from the device pool's memory pool (hipMallocFromPoolAsync /
// hipFreeAsync on `stream`), the batch in chunks of chunk_images().
// dGdst == NULL: prepare only -- build what the family needs and return (aai_adjoint_prepare, aai_adjoint_rotated_prepare).
enum AdjointFamily { ADJOINT_GENERAL, ADJOINT_PLANNED, ADJOINT_ROTATED, ADJOINT_SEPARABLE, ADJOINT_SAMPLE };
int enqueue_adjoint(AdjointFamily family, const aai_request &rq, const Geometry &g, int batch, int channels, const float *dGdst, int64_t dstStride,
                    int64_t dstImageStride, float *dGsrc, int64_t srcStride, int64_t srcImageStride, hipStream_t stream);

// The reference-precision path (include/aai_f64.h; the caller has checked the arguments): double images, single-channel, area / fast
// modes.  No plan, no lock, nothing blocks: the launches of aai_f64.hip on `stream`, the batch split at kMaxGridZ (forward) or in chunks
// of chunk_images() with the adjoint's stream-ordered scratch (for_each_adjoint_chunk).  Strides in elements.
int enqueue_f64_forward(const aai_request &rq, const Geometry &g, int batch, const double *dSrc, int64_t srcStride, int64_t srcImageStride, double *dDst,
                        int64_t dstStride, int64_t dstImageStride, hipStream_t stream);
int enqueue_f64_adjoint(const aai_request &rq, const Geometry &g, int batch, const double *dGdst, int64_t dstStride, int64_t dstImageStride, double *dGsrc,
                        int64_t srcStride, int64_t srcImageStride, hipStream_t stream);

// The narrow-element paths (the caller has checked the arguments, strides included): the element type in, the same type out, every mode.
//   enqueue_half   include/aai_half.h (channels = 1) and include/aai_half_interleaved.h: fp16 / bf16 images of raw 16-bit elements
//                  (halfType = AAI_HALF_F16 / AAI_HALF_BF16) of `channels` interleaved channels
//   enqueue_int    include/aai_int.h: u8 / u16 images (srcType = SRC_U8 / SRC_U16) of `channels` interleaved channels
// Both are one body (enqueue_narrow, aai_engine.cpp).  The plan is the forward's own under the key (request, channels) -- the one the
// forwarding route's enqueue() takes (for a half image: of a packed fp32 source), built on the caller's stream by the first call, which
// blocks; aai_prepare(req, channels) builds the same plan.  Two routes, chosen by static facts of the plan:
//   DIRECT      kernel AXIS, not dense, no listed pixel, the lane axis along dst x (aai::axis_narrow_can_serve); integer images also: area
//               or fast mode, u16 or more than 64 outputs in some strip.  aai_axis_narrow_kernel reads the image and writes the image, no
//               scratch, the batch split at kMaxGridZ.  aai_last_kernel(): "aai_axis_half_kernel<f16|bf16>", "aai_axis_int_kernel<u8|u16>".
//   FORWARDING  everything else: (half: widen into fp32 scratch,) enqueue() -- the code behind aai_resample_batch_device_f32, which reads
//               u8 / u16 itself -- into dense fp32 output scratch, one conversion into the caller's buffer.  Scratch = (half: a dense fp32
//               source and) a dense fp32 output per image in flight, stream-ordered from the device's pool (for_each_adjoint_chunk's), the
//               batch in chunks of chunk_images().  aai_last_kernel(): "<fp32 name>+widened" (half), "<fp32 name>+quantized" (integer).
int enqueue_half(const aai_request &rq, const Geometry &g, int batch, int channels, int halfType, const void *dSrc, int64_t srcStride, int64_t srcImageStride,
                 void *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream);
int enqueue_int(const aai_request &rq, const Geometry &g, int batch, int channels, int srcType, const void *dSrc, int64_t srcStride, int64_t srcImageStride,
                void *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream);

// Resample and convert (include/ext/aai_convert.h; the caller has checked the arguments, strides included): u8 / u16 images (srcType =
// SRC_U8 / SRC_U16) of `channels` interleaved channels in, round(fma(s, scale[c], offset[c])) out in cv's type and layout (dstStride,
// cv.planeStride and dstImageStride in elements of the output type), every mode.  enqueue_narrow's plan and two routes:
//   DIRECT      kernel AXIS, not dense, no listed pixel, area or fast mode, aai::axis_convert_can_serve: aai_axis_convert_kernel reads the
//               integer image and writes the converted image, no scratch, the batch split at kMaxGridZ.  aai_last_kernel():
//               "aai_axis_convert_kernel<u8|u16,f32|f16|bf16>".
//   FORWARDING  everything else: enqueue() into dense fp32 output scratch (through_fp32_scratch_into's pool and chunks),
//               aai_convert_store_kernel into the caller's buffer.  aai_last_kernel(): "<fp32 name>+converted".
int enqueue_convert(const aai_request &rq, const Geometry &g, int batch, int channels, int srcType, const void *dSrc, int64_t srcStride, int64_t srcImageStride,
                    const aai::ConvertParams &cv, void *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream);

// The half-precision adjoint (include/aai_adjoint_half.h; the caller has checked the arguments): gsrc = narrow(W^T widen(gdst)) for `batch`
// fp16 / bf16 images (halfType = AAI_HALF_F16 / AAI_HALF_BF16) of raw 16-bit elements with `channels` = 1..4 interleaved channels, area /
// fast modes, strides in elements.  On both routes the bits of narrow(enqueue_adjoint(ADJOINT_SEPARABLE, widen(gdst))).  The plan is
// SEPARABLE's: the forward's single-channel plan with its adjoint tables, built on first need (that blocks; aai_adjoint_rotated_prepare
// builds the same).  Two routes, chosen by static facts of the plan:
//   DIRECT      pick_kernel() says AXIS (rotations by 0 / 90 / 180 / 270 degrees), the plan holds its adjoint tables (adjState 1) and has
//               no lists for a correction pass -- but for the one class that measured no faster than forwarding, a single channel
//               up-sampled (more dst than source pixels) at 90 / 270 degrees (profiles/adjoint_half_time.txt) --: one launch of aai_axis_adjoint_half_kernel<HT, C> on the caller's images, no scratch, no
//               lock, the batch split at kMaxGridZ.  aai_last_kernel(): "aai_axis_adjoint_half_kernel<f16|bf16,C>".
//   FORWARDING  everything else (general rotations, wide or dense plans, refused inversions, plans with lists): gdst widened into dense
//               fp32 scratch, enqueue_adjoint(ADJOINT_SEPARABLE) into a dense fp32 gsrc, one rounding into the caller's buffer.  Scratch =
//               a dense fp32 gdst and gsrc per image in flight (beside enqueue_adjoint's own), stream-ordered from the device's pool, the
//               batch in chunks of chunk_images().  aai_last_kernel(): "<the fp32 route's name>+widened".
int enqueue_adjoint_half(const aai_request &rq, const Geometry &g, int batch, int channels, int halfType, const void *dGdst, int64_t dstStride,
                         int64_t dstImageStride, void *dGsrc, int64_t srcStride, int64_t srcImageStride, hipStream_t stream);

}  // namespace engine

}  // namespace aai
