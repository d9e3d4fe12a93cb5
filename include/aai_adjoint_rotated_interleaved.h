/* aai_adjoint_rotated_interleaved.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the planned adjoint at general
 * rotations for images with interleaved channels.
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares) and the
 * interface version stays 0.2, so these entries have a header of their own, like aai_adjoint_interleaved.h and aai_adjoint_rotated.h,
 * whose two halves they combine.  They validate exactly like aai_adjoint_interleaved_device_f32 / aai_adjoint_interleaved_f32
 * (tests/test_adjoint_rotated_interleaved_host.py compares them call by call). */
#ifndef AAI_ADJOINT_ROTATED_INTERLEAVED_H
#define AAI_ADJOINT_ROTATED_INTERLEAVED_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the interleaved planned adjoint: gsrc = W^T gdst for 1..4 interleaved channels from the plan's cached sums -----------------
 * Layout, contract and validation of aai_adjoint_interleaved_device_f32 / aai_adjoint_interleaved_f32 (aai_adjoint_interleaved.h):
 * element (x, y, c) of image b at b * image_stride + y * stride + x * channels + c, strides in elements; the same checks in the same
 * order with the same codes and messages -- the request, channels outside 1..4 "Channels must be 1..4.", bilinear / bicubic and
 * AAI_POLICY_DIAG_NO_FIXUP refused, AAI_POLICY_DOUBLE_PRECISION and AAI_POLICY_PREFER_CELL accepted and ignored, batch < 0, the row
 * length, null pointers, the strides; batch == 0 returns AAI_OK before the device is touched.  Every element of d_gsrc is written
 * (zeros included); nothing outside the entitled elements is read or written.
 *
 * BITS: channel c of the result has, bit for bit, the value aai_adjoint_interleaved_device_f32 gives channel c, the value
 * aai_adjoint_rotated_batch_device_f32 gives plane c and the value aai_adjoint_batch_device_f32 gives plane c:
 *   - n[d][c] = gdst[d][c] / S[d], a division per channel, with S from the general normaliser's own function;
 *   - a pair that reports no knife edge gets the general weight from the plain closed forms;
 *   - a source pixel outside every window of a knife-edge dst pixel sums only such pairs, in the general order;
 *   - the listed source pixels are recomputed by the general multi-channel gather itself, which overwrites them.
 *
 * ONE entry for every rotation and channel count:
 *   - channels == 1: the code behind aai_adjoint_rotated_batch_device_f32 (aai_adjoint_rotated.h), its kernels and bits.
 *   - Reduced angle 0 (rotations by multiples of 90 degrees), channels 2..4: forwarded to the code behind
 *     aai_adjoint_interleaved_device_f32, the GENERAL interleaved adjoint, with its bits (aai_last_kernel() names
 *     aai_adjoint_gather_multi_kernel).  The interleaved transposed separable kernel (aai_axis_adjoint_multi_kernel<C>) is NOT reached
 *     through these entries, whose routing and bits are pinned: aai_adjoint_planned_interleaved_device_f32
 *     (aai_adjoint_planned_interleaved.h) is the entry that asks for it, and is this entry everywhere else.  NOTE that the
 *     single-channel entry differs there: it forwards to the fp32 transposed separable kernel (aai_axis_adjoint_kernel).
 *   - Every other rotation, area or fast mode, channels 2..4: the plan aai_adjoint_rotated_batch_device_f32 uses -- the forward's
 *     SINGLE-channel plan, same key -- with the tables aai_adjoint_rotated.h describes: S (8 bytes per dst pixel) and the list of
 *     source pixels inside the windows of knife-edge dst pixels.  Neither depends on the channel count: they are shared with
 *     single-channel calls, there is no second copy and no new per-plan memory, and aai_plan_info(req, 1, ...) reports
 *     rot_adjoint=none|sums|general as it does for them.  Per call (per chunk of a large batch):
 *       aai_adjoint_scale_multi_kernel<MODE, C>          element-wise pass 1, one lane per row element;
 *       aai_adjoint_plain_gather_multi_kernel<MODE, C>   one lane per source pixel: a pair is enumerated, window-tested and
 *                                                        integrated once from the plain closed forms, each channel adds a load and
 *                                                        a multiply-add;
 *       aai_adjoint_gather_listed_multi_kernel<MODE, C>  where the plan lists source pixels: the general per-pair code over them.
 *     aai_last_kernel() names "aai_adjoint_plain_gather_multi_kernel<area|fast, C>", with "+listed" appended when that pass ran.
 *   - Plans that keep the general adjoint (rot_adjoint=general, see aai_adjoint_rotated.h): forwarded to the code behind
 *     aai_adjoint_interleaved_device_f32, identical bits.
 *
 * PREPARING: there is no new prepare entry.  aai_adjoint_rotated_prepare(req) (aai_adjoint_rotated.h) builds everything this path
 * needs; after it these entries only enqueue.  Without it the first call of a geometry on a device builds the tables and SYNCHRONISES.
 * That first call builds the single-channel forward plan even if the caller only ever prepared for C channels (aai_prepare(req, C)):
 * the tables live on the single-channel plan.
 *
 * Scratch: dst_width x dst_height x channels doubles per image in flight, stream-ordered from the library's retained pool; batches
 * whose scratch would exceed about 1 GiB go through in chunks, sized exactly as aai_adjoint_interleaved_device_f32 sizes them.
 * Determinism: no atomics, no shared memory, a fixed summation order: the same bits on every call, image b of a batch gets the bits
 * of a single-image call.
 * Resources: DESIGN.md section 9 (registers and occupancy of every instantiation).
 * MEASURED on an MI355X, three legs taking turns in the same process (`tools/adjoint_time.py --rotated --channels`,
 * profiles/adjoint_rotated_interleaved_time.txt, one run; DESIGN.md section 9 quotes it), median of 24 launches, C = 3 / C = 4:
 * aai_adjoint_interleaved_device_f32 / new entry 3.6 / 3.4 at 8192 x 8192 -> 3426 x 3426 at 17.5 degrees (area; 7.64 -> 2.14 ms for C = 3)
 * and 2.1 / 1.9 (fast); 3.2 / 3.0 at 8:1 (area); 4.2 / 3.9 at x2 up-sampling of 2048 x 2048 at 30 degrees (area).  C calls of
 * aai_adjoint_rotated_batch_device_f32 on planes split beforehand / new entry: 2.5 to 3.5 over the same rows.  Identical bits in every
 * row; in every row the new entry's 90th percentile lies below the general entry's 10th, so no row is routed back.
 * The interface version (aai.h: AAI_VERSION_MINOR) stays at 2: these are additions in a header of their own. */
int aai_adjoint_rotated_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                               const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                               float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL */
int aai_adjoint_rotated_interleaved_f32(const aai_request *req, int32_t channels,
                                        const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_ADJOINT_ROTATED_INTERLEAVED_H */
