/* aai_adjoint_planned_interleaved.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the planned adjoint at rotations by
 * multiples of 90 degrees for images with interleaved channels -- the transposed separable kernel on NHWC / RGB(A) storage.
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares) and the
 * interface version stays 0.2, so these entries have a header of their own, like aai_adjoint_planned.h, aai_adjoint_interleaved.h,
 * aai_adjoint_rotated.h and aai_adjoint_rotated_interleaved.h.  They validate exactly like aai_adjoint_interleaved_device_f32 /
 * aai_adjoint_interleaved_f32 (tests/test_adjoint_planned_interleaved_host.py compares them call by call). */
#ifndef AAI_ADJOINT_PLANNED_INTERLEAVED_H
#define AAI_ADJOINT_PLANNED_INTERLEAVED_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the interleaved planned adjoint: gsrc = W^T gdst for 1..4 interleaved channels, planned at EVERY geometry ------------------
 * Layout, contract and validation of aai_adjoint_interleaved_device_f32 / aai_adjoint_interleaved_f32 (aai_adjoint_interleaved.h):
 * element (x, y, c) of image b at b * image_stride + y * stride + x * channels + c, strides in elements; the same checks in the same
 * order with the same codes and messages -- the request, channels outside 1..4 "Channels must be 1..4.", bilinear / bicubic and
 * AAI_POLICY_DIAG_NO_FIXUP refused, AAI_POLICY_DOUBLE_PRECISION and AAI_POLICY_PREFER_CELL accepted and ignored, batch < 0, the row
 * length, null pointers, the strides; batch == 0 returns AAI_OK before the device is touched.  Every element of d_gsrc is written
 * (zeros included); nothing outside the entitled elements is read or written.  The stream-order contract of aai.h covers the device
 * entry: after the plan's tables exist it only enqueues on `stream`.
 *
 * WHICH PATH SERVES A CALL, and with whose bits:
 *   - Rotation by a multiple of 90 degrees (aai_query: AAI_KERNEL_AXIS), channels 2..4, area or fast mode: the forward's
 *     SINGLE-channel plan with the adjoint tables aai_adjoint_planned.h describes -- the inverse ranges per source column and row and
 *     the correction lists.  They know pixels, not channels: they are shared with single-channel calls, there is no second copy and no
 *     new per-plan memory, and aai_plan_info(req, 1, ...) reports adjoint=tables as it does for them.  Per call:
 *       aai_axis_adjoint_multi_kernel<C>                 one lane per ELEMENT e = x * C + c of a source row, 256 elements per
 *                                                        workgroup walking 32 source rows; the pixel e / C picks ranges and weights, the
 *                                                        channel is an address offset.  fp32 fused multiply-adds in the single-channel
 *                                                        kernel's order, no scratch, 4-byte coalesced loads and stores for C = 3 too;
 *       aai_adjoint_norm_listed_multi_kernel<MODE, C>,   where the plan lists pixels: the general multi-channel adjoint over the listed
 *       aai_adjoint_gather_listed_multi_kernel<MODE, C>  dst pixels and source pixels, which it overwrites.
 *     aai_last_kernel() names "aai_axis_adjoint_multi_kernel<C>", with "+listed" appended when the correction pass ran.
 *     BITS: channel c has, everywhere, the bits aai_adjoint_planned_batch_device_f32 gives plane c (listed pixels therefore carry the
 *     general adjoint's bits): lane e executes, operation for operation, what the single-channel kernel executes for plane c.
 *   - The same request where the single-channel plan keeps the general adjoint (adjoint=none after preparing: a wide plan --
 *     AAI_KERNEL_AXIS_WIDE --, a dense plan, tables the inversion refuses, a correction list over more than half of the image): the code
 *     behind aai_adjoint_interleaved_device_f32, its kernel names and bits.
 *   - Every other rotation (the rotated area / fast kernels' geometries): exactly what aai_adjoint_rotated_interleaved_device_f32 does
 *     (aai_adjoint_rotated_interleaved.h), its kernel names and bits.
 *   - channels == 1: exactly aai_adjoint_rotated_batch_device_f32 (aai_adjoint_rotated.h), its kernel names and bits.
 * NOTE that aai_adjoint_rotated_interleaved_device_f32 is unchanged: at a multiple of 90 degrees with 2..4 channels it still runs the
 * general interleaved gather.  These entries are the ones that ask for the interleaved transposed separable kernel.
 *
 * PREPARING: there is no new prepare entry.  aai_adjoint_rotated_prepare(req) (aai_adjoint_rotated.h) already builds everything this
 * path needs -- at a multiple of 90 degrees the single-channel plan plus its axis adjoint tables (what aai_adjoint_prepare builds), at
 * every other rotation the sums -- and after it these entries only enqueue.  Without it the first call of a geometry on a device builds
 * the tables and SYNCHRONISES.  That first call builds the single-channel forward plan even if the caller only ever prepared for C
 * channels (aai_prepare(req, C)): the tables live on the single-channel plan.
 *
 * Scratch: none where the plan has no lists; dst_width x dst_height x channels doubles per image in flight where it has, stream-ordered
 * from the library's retained pool; batches whose scratch would exceed about 1 GiB go through in chunks, sized exactly as
 * aai_adjoint_interleaved_device_f32 sizes them.
 * Determinism: no atomics, no shared memory, a fixed summation order: the same bits on every call, image b of a batch gets the bits
 * of a single-image call.
 * Resources: DESIGN.md section 9 (registers and occupancy of the three instantiations; no private memory).
 * MEASURED on an MI355X, the legs taking turns in the same process (`tools/adjoint_time.py --planned --channels`,
 * profiles/adjoint_axis_interleaved_time.txt, one run; DESIGN.md section 9 quotes it), median of 24 launches, 4096 x 4096 sources unless
 * said, C = 3 / C = 4: aai_adjoint_interleaved_device_f32 / new entry 92 / 73 at grid-aligned 4:1 (area; 7.05 -> 0.076 ms for C = 3) and
 * 5.1 / 4.3 (fast); 15.6 / 13.3 and 5.0 / 4.2 at 2.5:1, 90 degrees; 83 / 74 and 4.8 / 4.2 at 2:1, 180 degrees; 12.5 / 15.9 and 3.2 / 4.0 at
 * x2 up-sampling of 2048 x 2048, 270 degrees.  In every row the new entry's 90th percentile lies below the general entry's 10th.  New entry
 * / C calls of aai_adjoint_planned_batch_device_f32 on planes split beforehand: 0.73 to 0.92 when down-sampling, 0.33 to 0.54 in the
 * up-sampling rows; slower in no row; identical bits in every row.  The torch operator's backward alone on a channels_last input,
 * planned_backward=True (the planar route, its permutes included) / planned_backward="channels_last": 1.5 to 2.0 when down-sampling, 2.8 to
 * 4.5 in the up-sampling rows; the new route's median is the lower one in every row, so no geometry keeps the planar route.
 * The interface version (aai.h: AAI_VERSION_MINOR) stays at 2: these are additions in a header of their own. */
int aai_adjoint_planned_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                               const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                               float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL */
int aai_adjoint_planned_interleaved_f32(const aai_request *req, int32_t channels,
                                        const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_ADJOINT_PLANNED_INTERLEAVED_H */
