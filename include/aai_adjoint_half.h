/* aai_adjoint_half.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the adjoint on half-precision gradients.
 * aai_half.h and aai_half_interleaved.h read and write fp16 / bf16 images in the forward; the entries below are their transpose:
 * gsrc = W(req)^T gdst on fp16 or bf16 gradient images of 1..4 interleaved channels, the same element type and layout out, so that a
 * mixed-precision backward neither widens its gradient into an fp32 copy first nor rounds an fp32 result afterwards.
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares), the
 * interface version stays 0.2 and aai_half.h / aai_half_interleaved.h keep their text, so these entries have a header of their own. */
#ifndef AAI_ADJOINT_HALF_H
#define AAI_ADJOINT_HALF_H

#include "aai_half.h"
#include "aai_adjoint_planned_interleaved.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- gsrc = W^T gdst on fp16 / bf16 images of interleaved channels --------------------------------------------------------------
 * IMAGES: `half_dtype` is AAI_HALF_F16 or AAI_HALF_BF16 (aai_half.h); gdst (dst_width x dst_height) and gsrc (src_width x src_height)
 * both hold that type as raw 16-bit elements with `channels` (1..4) interleaved; element (x, y, c) of image b at b * image_stride +
 * y * stride + x * channels + c, strides in elements: the layout of aai_adjoint_planned_interleaved_device_f32.  Area and fast modes.
 * Every element of gsrc is written, zeros included.
 * VALUES (the contract): on every route and at every geometry the result is, bit for bit,
 *     narrow(aai_adjoint_planned_interleaved_device_f32(widen(gdst)))
 * -- for channels == 1 that is aai_adjoint_rotated_batch_device_f32 --: ONE exact widening of every gdst element to fp32, the fp32
 * entry's arithmetic, and ONE rounding of every gsrc element to `half_dtype`, to nearest, ties to even.  What rounds beyond the largest
 * finite value of the type is +-Inf; NaN stays NaN (the type's quiet NaN).  Channels never mix: a non-finite element of one channel
 * reaches gradients of that channel only.  A source element that no dst pixel reads gets +0.
 * This is stronger than the forward's "one unit in the last place between routes", and it holds by construction: the direct kernel
 * executes the fp32 kernel's operations (the same table weights, the same fused multiply-adds, ka ascending inside kb ascending)
 * between its widening load and its rounding store.
 * VALIDATION: exactly as aai_adjoint_planned_interleaved_device_f32 (the host entry: aai_adjoint_planned_interleaved_f32) validates,
 * in its order, with its codes and messages -- bilinear / bicubic requests and AAI_POLICY_DIAG_NO_FIXUP are refused as there.
 * `half_dtype` is checked directly behind `channels` (AAI_ERR_BAD_ARGUMENT, "Unknown half-precision element type.").  batch == 0 returns
 * AAI_OK before the device is touched.
 * PLAN: the SINGLE-channel forward plan of the request with its axis adjoint tables, which know pixels and not channels -- there is no
 * new per-plan memory.  aai_adjoint_rotated_prepare(req) prepares these calls.  Without a prepare, the first call of a geometry on a
 * device builds the tables and synchronises; later calls only enqueue.  Calls keep the stream-order contract of aai.h.
 * MEMORY: the memory contract of aai.h -- only entitled elements are read or written, row and image padding is neither read nor
 * written.  Base pointers and strides are assumed aligned to 2 bytes (one element) and nothing more.
 *
 * TWO ROUTES, chosen per request by static facts of its plan:
 *   direct      aai_query reports AAI_KERNEL_AXIS (the rotation is 0, 90, 180 or 270 degrees and the plan is not AAI_KERNEL_AXIS_WIDE),
 *               the mode is area or fast, the plan holds its adjoint tables and has no correction lists, and the request is not of the
 *               one class that measured no faster than forwarding (below).  ONE launch of
 *               aai_axis_adjoint_half_kernel<HT, C> reads the half gradient and writes the half gradient: one lane per element of a
 *               source row, 2-byte stores, no LDS, no atomics, no scratch, no fp32 image anywhere.  All four quadrants: the transposed
 *               kernel takes them through its output strides, so 90 / 270 degrees -- which the forward's direct route lacks -- are
 *               served here.  aai_last_kernel() names "aai_axis_adjoint_half_kernel<f16,C>" / "aai_axis_adjoint_half_kernel<bf16,C>".
 *   forwarding  everything else -- general rotations, AAI_KERNEL_AXIS_WIDE, dense plans, tables the inversion refuses, plans with
 *               correction lists: widen gdst into dense fp32 scratch, run the code behind aai_adjoint_planned_interleaved_device_f32 on
 *               it, narrow its dense fp32 result into the caller's gsrc.  Scratch: a dense fp32 gdst and a dense fp32 gsrc per image in
 *               flight beside whatever the fp32 route takes itself, stream-ordered from the library's pool on the caller's stream, large
 *               batches in chunks.  aai_last_kernel() names the fp32 route with "+widened" appended.
 *               NOT TESTED: whether this route can be recorded into a stream capture (the pool's allocations, like the fp32 adjoint's).
 * WHICH CLASSES KEEP THE DIRECT ROUTE is measured, not assumed (tools/adjoint_half_time.py -> profiles/adjoint_half_time.txt; a class of
 * requests -- quadrant pair x up- / down-sampling x channel count -- keeps the direct route only if its median is below the forwarding
 * route's in both runs; a class that loses forwards):
 *   MI355X, one image, medians of 24 launches, two runs that agree to a few per cent; (a) the direct entry, (b) the forwarding route
 *   from its stages on scratch allocated beforehand (a lower estimate of it), (d) the half forward; area mode, fp16 (fast mode and
 *   bf16 lie within a few per cent of these, 2.5:1 fast mode 15-25 % lower):
 *     4096^2 <- 1024^2, 4:1, 0 deg      C=1  31 us (b) 46  (d) 14    C=3  73 (b) 113 (d) 33    C=4  90 (b) 175 (d) 36
 *     4096^2 <- 1638^2, 2.5:1, 90 deg   C=1  45 us (b) 61  (d) 60    C=3  99 (b) 142 (d) 157   C=4 122 (b) 195 (d) 200
 *     4096^2 <- 2048^2, 2:1, 180 deg    C=1  33 us (b) 50  (d) 26    C=3  93 (b) 135 (d) 72    C=4 115 (b) 197 (d) 69
 *     2048^2 <- 4096^2, x2, 270 deg     C=1 187 us (b) 184 (d) 73    C=3 298 (b) 328 (d) 354   C=4 187 (b) 310 (d) 372
 *   The direct route is 0.52-0.74 of the forwarding route when down-sampling and 0.60 (C = 4) / 0.91 (C = 3) of it at x2 up-sampling
 *   at 270 degrees.  ONE CLASS LOSES in both runs and therefore FORWARDS: a single channel, up-sampled (more dst than source pixels),
 *   at 90 / 270 degrees -- there the kernel is bound by its strided gdst loads, which cost a 2-byte element what they cost a 4-byte
 *   one (187 against 184 us; the fp32 kernel's known weak spot, 2.6 x the forward).  aai_last_kernel() then names
 *   "aai_axis_adjoint_kernel+widened".  The backward as a whole still costs 2.1-2.5 x the half forward at 4:1 and 1.3-1.7 x at 2:1.
 *
 * NOT PROVIDED: bilinear / bicubic (refused like the fp32 entry: their adjoint is aai_adjoint_sample.h's), integer types (they carry
 * no gradient), the listed correction behind the direct kernel (such plans forward), row bands. */
int aai_adjoint_half_device(const aai_request *req, int32_t batch, int32_t channels, int32_t half_dtype,
                            const void *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                            void *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL.  The device entry's bits. */
int aai_adjoint_half_host(const aai_request *req, int32_t channels, int32_t half_dtype,
                          const void *gdst, int64_t dst_stride, void *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_ADJOINT_HALF_H */
