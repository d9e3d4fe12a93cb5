/* aai_half_interleaved.h -- extension of the C ABI (include/aai.h, libaai_hip.so): half-precision images with interleaved channels.
 * aai_half.h reads and writes single-channel fp16 / bf16 images; the entries below read fp16 or bf16 images of 1..4 INTERLEAVED
 * channels and write the same element type and layout, so that a caller who holds RGB(A) half-precision data -- a channels-last
 * activation under mixed precision is exactly this layout -- neither de-interleaves nor widens it first.
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares), the
 * interface version stays 0.2 and aai_half.h keeps its text, so these entries have a header of their own, like aai_int.h. */
#ifndef AAI_HALF_INTERLEAVED_H
#define AAI_HALF_INTERLEAVED_H

#include "aai_half.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dst = resample(src) on fp16 / bf16 images of interleaved channels ----------------------------------------------------------
 * IMAGES: `half_dtype` is AAI_HALF_F16 or AAI_HALF_BF16 (aai_half.h); source and output both hold that type with `channels` (1..4)
 * interleaved; element (x, y, c) of image b at b * image_stride + y * stride + x * channels + c, strides in elements: the layout of
 * aai_resample_interleaved_device.  All four modes.
 * VALUES (the contract): aai_half.h's, per channel -- every source element is widened exactly to fp32, the forward's own fp32 weights
 * are applied, sums are fp32, and the result is rounded ONCE to `half_dtype`, to nearest, ties to even.  What rounds beyond the
 * largest finite fp16 value is +-Inf; NaN stays NaN (the type's quiet NaN).  Channels never mix: a non-finite element of one channel
 * reaches outputs of that channel only.
 * VALIDATION: exactly as aai_resample_interleaved_device (the host entry: aai_resample_interleaved_host) validates, in its order, with
 * its codes and messages; `half_dtype` is checked where that entry checks its src_dtype (AAI_ERR_BAD_ARGUMENT, "Unknown
 * half-precision element type.").  batch == 0 returns AAI_OK without touching the device.
 * PLAN: the forward's own, under the key (req, channels): aai_prepare(req, channels) prepares these calls too, aai_plan_info(req,
 * channels) describes the plan, unchanged.  The first call of a geometry on a device builds the plan and synchronises, like the fp32
 * entry; later calls only enqueue.  Calls keep the stream-order contract of aai.h.
 * MEMORY: the memory contract of aai.h -- only entitled elements are read or written, row and image padding is neither read nor
 * written.  A base pointer and a stride are assumed aligned to 2 bytes (one element) and nothing more.
 *
 * TWO ROUTES, chosen per request by static facts of its plan:
 *   direct      the static facts of aai_half.h's direct route -- aai_query reports AAI_KERNEL_AXIS, the plan is not `dense` and lists no
 *               pixel, the rotation is 0 or 180 degrees, the mode is area or fast -- and the strip form applies (not
 *               AAI_KERNEL_AXIS_WIDE, at most 256 outputs per strip, at least 4 ELEMENTS in a source row: width x channels >= 4).
 *               ONE streaming kernel reads the half image and writes the half image: four consecutive elements as one 8-byte store at
 *               0 degrees, element by element at 180 degrees (pixels run backwards there, the channels of a pixel forwards).  No
 *               scratch, no fp32 image anywhere.  aai_last_kernel() names "aai_axis_half_kernel<f16>" / "aai_axis_half_kernel<bf16>"
 *               for every channel count.  Which classes of such requests keep this route is measured, profiles/half_interleaved_time.txt.
 *   forwarding  everything else -- general rotations, 90 / 270 degrees, AAI_KERNEL_AXIS_WIDE, plans with listed pixels or `dense`, the
 *               samplers, rows of fewer than 4 elements: widen width x channels elements per row into dense fp32 scratch, run the code
 *               behind aai_resample_interleaved_device on it (AAI_DTYPE_F32, `channels`), narrow into the caller's buffer.  The bits are
 *               exactly narrow(aai_resample_interleaved_device(widen(src))).  Scratch and its pool as in aai_half.h.
 *               aai_last_kernel() names the fp32 kernel with "+widened" appended.
 *               NOT TESTED: whether this route can be recorded into a stream capture (the pool's allocations, like the adjoint's).
 * The two routes agree to one unit in the last place of `half_dtype`: their fp32 sums differ in the order of a few operations.
 * channels == 1 gives the bits, the route and the kernel name of aai_resample_half_batch_device / aai_resample_half_host.
 *
 * NOT PROVIDED: row bands, the multi-device entry, a half adjoint in the C ABI (the torch operator widens the gradient and runs the
 * fp32 interleaved adjoint), the listed-pixel correction behind the direct kernel (such plans forward), a direct kernel for the
 * transposed quadrants (90 / 270 degrees forward), stream capture of the forwarding route (untested). */
int aai_resample_half_interleaved_device(const aai_request *req, int32_t batch, int32_t channels, int32_t half_dtype,
                                         const void *d_src, int64_t src_stride, int64_t src_image_stride,
                                         void *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream);
/* host buffers: upload src, run, download dst; `layout` may be NULL.  The device entry's bits. */
int aai_resample_half_interleaved_host(const aai_request *req, int32_t channels, int32_t half_dtype, const void *src, int64_t src_stride,
                                       void *dst, int64_t dst_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_HALF_INTERLEAVED_H */
