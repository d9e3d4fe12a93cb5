/* aai_int.h -- extension of the C ABI (include/aai.h, libaai_hip.so): integer images in, the same type out.  The entries of aai.h read
 * 8-bit and 16-bit unsigned sources (AAI_DTYPE_U8, AAI_DTYPE_U16; 1..4 interleaved channels) and always write fp32; the entries below
 * write the SAME element type, so that a caller who resamples an RGB scan or a 16-bit detector frame neither holds an fp32 image four
 * (or two) times the size of the result nor rounds and clamps it in a pass of their own.
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares) and the
 * interface version stays 0.2, so these entries have a header of their own, like aai_f64.h and aai_half.h. */
#ifndef AAI_INT_H
#define AAI_INT_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dst = quantize(resample(src)) on u8 / u16 images ---------------------------------------------------------------------------
 * IMAGES: `dtype` is AAI_DTYPE_U8 or AAI_DTYPE_U16 (AAI_DTYPE_F32 and anything else: AAI_ERR_BAD_ARGUMENT, "Unknown integer element
 * type."); source and output both hold that type with `channels` (1..4) interleaved; element (x, y, c) of image b at b * image_stride
 * + y * stride + x * channels + c, strides in elements: the layout of aai_resample_interleaved_device.  All four modes.
 * VALUES (the contract): every source element is used as its integer value, exactly; the forward's own fp32 weights are applied, sums
 * are fp32, and the result s is converted ONCE: rounded to the nearest integer, ties to even, then saturated to [0, 255] / [0, 65535].
 * The bicubic sampler overshoots, so the saturation is reachable.  NaN and -Inf give 0, +Inf gives the maximum (integer sources
 * produce no such sum; the conversion kernel of the forwarding route is defined for them all the same).
 * VALIDATION: exactly as aai_resample_interleaved_device validates, in its order, with its codes and messages; `dtype` is checked
 * where that entry checks its src_dtype.  batch == 0 returns AAI_OK without touching the device.
 * PLAN: the forward's own, under the key (req, channels): aai_prepare(req, channels) prepares these calls too, aai_plan_info(req,
 * channels) describes the plan, unchanged.  The first call of a geometry on a device builds the plan and synchronises, like the fp32
 * entry; later calls only enqueue.  Calls keep the stream-order contract of aai.h.
 * MEMORY: the memory contract of aai.h -- only entitled elements are read or written, row and image padding is neither read nor
 * written.  A base pointer and a stride are assumed aligned to one element and nothing more: for u8 that is 1 byte.
 *
 * TWO ROUTES, chosen per request by static facts of its plan:
 *   direct      aai_query reports AAI_KERNEL_AXIS, the plan is not `dense` and lists no pixel (aai_plan_info: flagged=0 dense=0), the
 *               rotation is 0 or 180 degrees (the lane axis of the separable kernel runs along dst x), the mode is area or fast, and
 *               the strip form applies (not AAI_KERNEL_AXIS_WIDE, at most 256 outputs per strip, at least 4 elements in a source row).
 *               Measured exception (profiles/int_time.txt): AAI_DTYPE_U8 requests whose strips all hold at most 64 outputs (ratios
 *               of about 4 and more) forward -- the direct kernel was not faster there beyond the spread of the measurement.
 *               ONE streaming kernel reads the integer image and writes the integer image.  No scratch, no fp32 image anywhere.
 *               aai_last_kernel() names "aai_axis_int_kernel<u8>" / "aai_axis_int_kernel<u16>".
 *   forwarding  everything else -- general rotations, 90 / 270 degrees, AAI_KERNEL_AXIS_WIDE, plans with listed pixels or `dense`, the
 *               samplers: the code behind aai_resample_interleaved_device reads the integer image itself (no widening pass) and writes
 *               dense fp32 output scratch, one conversion kernel writes the caller's buffer.  The bits are exactly
 *               quantize(aai_resample_interleaved_device(src)).  Scratch: an fp32 output per image in flight, stream-ordered from the
 *               library's pool like the adjoint's (at most about 1 GiB per round of launches, larger batches in chunks; the pool is
 *               created, on the host, by the first such call of a process on a device).
 *               aai_last_kernel() names the fp32 kernel with "+quantized" appended.
 *               NOT TESTED: whether this route can be recorded into a stream capture (the pool's allocations, like the adjoint's).
 * The two routes agree within one count: their fp32 sums differ in the order of a few operations.
 *
 * NOT PROVIDED: row bands, the multi-device entry, a pipelined host batch, an adjoint (integers carry no gradient), a direct kernel
 * for the transposed quadrants (90 / 270 degrees forward). */
int aai_resample_int_batch_device(const aai_request *req, int32_t batch, int32_t channels, int32_t dtype,
                                  const void *d_src, int64_t src_stride, int64_t src_image_stride,
                                  void *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream);
/* host buffers: upload src, run, download dst; `layout` may be NULL.  The device entry's bits. */
int aai_resample_int_host(const aai_request *req, int32_t channels, int32_t dtype, const void *src, int64_t src_stride,
                          void *dst, int64_t dst_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_INT_H */
