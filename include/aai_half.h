/* aai_half.h -- extension of the C ABI (include/aai.h, libaai_hip.so): half-precision images.  The entries of aai.h read fp32, 8-bit
 * and 16-bit integer sources and always write fp32; the entries below read fp16 or bf16 images and write the SAME element type, so
 * that a caller who holds half-precision data (an activation under mixed precision, an fp16 image stack) neither widens it first nor
 * narrows the result afterwards.
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares) and the
 * interface version stays 0.2, so these entries have a header of their own, like aai_f64.h. */
#ifndef AAI_HALF_H
#define AAI_HALF_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AAI_HALF_F16 = 1, AAI_HALF_BF16 = 2 };   /* IEEE binary16 / bfloat16, as raw 16-bit elements */

/* ---- dst = resample(src) on fp16 / bf16 images ------------------------------------------------------------------------------
 * IMAGES: source and output both hold `half_dtype` elements; single-channel; strides in elements; image b at b * image_stride: the
 * layout of aai_resample_batch_device_f32.  All four modes.
 * VALUES (the contract): every source element is widened exactly to fp32, the forward's own fp32 weights are applied, sums are fp32,
 * and the result is rounded ONCE to `half_dtype`, to nearest, ties to even.  What rounds beyond the largest finite fp16 value is
 * +-Inf; NaN stays NaN (the type's quiet NaN).  The precision policy bits of the request mean what they mean for
 * aai_resample_batch_device_f32.
 * VALIDATION: exactly as aai_resample_batch_device_f32 validates, in its order, with its codes and messages, before any device call
 * where that entry reports before any device call; the element type is checked where aai_resample_batch_device checks its
 * src_dtype (AAI_ERR_BAD_ARGUMENT, "Unknown half-precision element type.").  batch == 0 returns AAI_OK without touching the device.
 * PLAN: the forward's own, under the forward's single-channel key: aai_prepare(req, 1) prepares these calls too, aai_plan_info(req, 1)
 * describes the plan, unchanged.  The first call of a geometry on a device builds the plan and synchronises, like the fp32 entry;
 * later calls only enqueue.  Calls keep the stream-order contract of aai.h.
 * MEMORY: the memory contract of aai.h -- only entitled elements are read or written, row and image padding is neither read nor
 * written.  A base pointer and a stride are assumed aligned to 2 bytes (one element) and nothing more.
 *
 * TWO ROUTES, chosen per request by static facts of its plan:
 *   direct      aai_query reports AAI_KERNEL_AXIS, the plan is not `dense` and lists no pixel (aai_plan_info: flagged=0 dense=0), the
 *               rotation is 0 or 180 degrees (the lane axis of the separable kernel runs along dst x) and the mode is area or fast:
 *               ONE streaming kernel reads the half image and writes the half image.  No scratch, no fp32 image anywhere.
 *               aai_last_kernel() names "aai_axis_half_kernel<f16>" / "aai_axis_half_kernel<bf16>".
 *   forwarding  everything else -- general rotations, 90 / 270 degrees, AAI_KERNEL_AXIS_WIDE, plans with listed pixels or `dense`, the
 *               samplers: widen into fp32 scratch, run the code behind aai_resample_batch_device_f32, narrow into the caller's
 *               buffer.  The bits are exactly narrow(fp32 entry(widen(src))).  Scratch: an fp32 source copy and an fp32 output per
 *               image in flight, stream-ordered from the library's pool like the adjoint's (at most about 1 GiB per round of launches,
 *               larger batches in chunks; the pool is created, on the host, by the first such call of a process on a device).
 *               aai_last_kernel() names the fp32 kernel with "+widened" appended.
 *               NOT TESTED: whether this route can be recorded into a stream capture (the pool's allocations, like the adjoint's).
 * The two routes agree to one unit in the last place of `half_dtype`: their fp32 sums differ in the order of a few operations.
 *
 * NOT PROVIDED: interleaved channels (by these two entries: aai_half_interleaved.h has them), row bands, the multi-device entry, a
 * half adjoint in the C ABI (the torch operator widens the gradient and runs the fp32 adjoint), the listed-pixel correction behind the
 * direct kernel (such plans forward), a direct kernel for the transposed quadrants (90 / 270 degrees forward). */
int aai_resample_half_batch_device(const aai_request *req, int32_t batch, int32_t half_dtype,
                                   const void *d_src, int64_t src_stride, int64_t src_image_stride,
                                   void *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream);
/* host buffers: upload src, run, download dst; `layout` may be NULL.  The device entry's bits. */
int aai_resample_half_host(const aai_request *req, int32_t half_dtype, const void *src, int64_t src_stride,
                           void *dst, int64_t dst_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_HALF_H */
