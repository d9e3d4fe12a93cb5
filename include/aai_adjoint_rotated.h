/* aai_adjoint_rotated.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the planned adjoint at every rotation.
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares) and the
 * interface version stays 0.2, so these entries have a header of their own, like aai_adjoint_planned.h.  They validate exactly like
 * aai_adjoint_batch_device_f32 / aai_adjoint_f32 (tests/test_adjoint_rotated_host.py compares them call by call). */
#ifndef AAI_ADJOINT_ROTATED_H
#define AAI_ADJOINT_ROTATED_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the planned adjoint at general rotations: cached sums, plain closed forms ---------------------------------------------
 * Same contract as aai_adjoint_batch_device_f32 / aai_adjoint_f32 of aai.h -- the same validation in the same order with the same
 * messages, bilinear / bicubic and AAI_POLICY_DIAG_NO_FIXUP refused, AAI_POLICY_DOUBLE_PRECISION and AAI_POLICY_PREFER_CELL accepted
 * and ignored, every element of gsrc written (zeros included), nothing outside the entitled elements read or written, batch == 0
 * returns before the device is touched.  ONE entry for every rotation:
 *   - Reduced angle 0 (rotations by multiples of 90 degrees): forwarded to the code behind aai_adjoint_planned_batch_device_f32
 *     (aai_adjoint_planned.h: the transposed separable kernel, fp32, aai_last_kernel() names "aai_axis_adjoint_kernel").
 *   - Every other rotation, area or fast mode: gsrc has the BITS of aai_adjoint_batch_device_f32, from a cheaper formulation.  The
 *     general adjoint evaluates the knife-edge variant of the per-pair code for every pair, in its normaliser and again in its
 *     gather.  Here the request's plan (the forward's own: the plan aai_prepare(req, 1) builds, same key) gains two tables, built by
 *     a one-off kernel with one lane per dst pixel:
 *       S  the sum of the weights of every dst pixel, fp64 [dH][dW], from the general normaliser's own function.  Pass 1 becomes
 *          element-wise, n[d] = gdst[d] / S[d] (aai_adjoint_scale_kernel);
 *       K  the dst pixels with a pair whose weight the strict replay of the reference's classifier decided (a knife edge), and from
 *          them the list of the source pixels inside their windows.
 *     aai_adjoint_plain_gather_kernel then sums, per source pixel and in the general gather's order, weights from the plain closed
 *     forms -- which give a pair that reports no knife edge bit for bit the weight the general adjoint uses -- and the listed source
 *     pixels are recomputed behind it by the general gather itself (aai_adjoint_gather_listed_kernel, which overwrites them).
 *     aai_last_kernel() names "aai_adjoint_plain_gather_kernel<area>" / "<fast>", with "+listed" appended when that pass ran.
 *     MEMORY: 8 bytes per dst pixel per plan on the device (S), plus 8 bytes per listed source pixel; freed with the plan (the cache
 *     keeps 32 plans per device) and by aai_shutdown.  Per call: the fp64 scratch of aai_adjoint_batch_device_f32, chunked alike.
 *     The first call of a geometry on a device builds the tables and SYNCHRONISES; aai_adjoint_rotated_prepare (= aai_prepare plus
 *     the tables) takes that cost up front, later calls only enqueue.  aai_plan_info appends rot_adjoint=none|sums|general, then
 *     knife=<count of K> once the scan has run.
 *   - These plans keep the general adjoint (rot_adjoint=general; the call is forwarded to the code behind
 *     aai_adjoint_batch_device_f32, identical bits, aai_last_kernel() names the gather kernel): more K pixels than
 *     AAI_MAX_LISTED_PIXELS, a source list over more than half of the source image (grid-aligned lattices, e.g. 45 degrees at 2.83:1), an S of
 *     more than 1 GiB.
 * The existing entries keep their behaviour: aai_adjoint_batch_device_f32 needs no plan and never synchronises, and at a general
 * rotation aai_adjoint_planned_* and aai_adjoint_prepare still build no plan.
 * MEASURED on an MI355X against aai_adjoint_batch_device_f32 taking turns in the same process (profiles/adjoint_rotated_time.txt, one run;
 * DESIGN.md section 9 quotes it), general / new, median of 24 launches: 8192 x 8192 -> 3426 x 3426 at 17.5 degrees 3.7 (area: 7.54 -> 2.04
 * ms) and 2.2 (fast); 8:1 at 17.5 degrees 3.3 and 2.1; x2 up-sampling at 30 degrees 5.0 and 2.5; identical bits in every row.
 * aai_adjoint_rotated_prepare also prepares the interleaved entries of aai_adjoint_rotated_interleaved.h: they use this plan and these
 * tables for every channel count and have no prepare entry of their own. */
int aai_adjoint_rotated_prepare(const aai_request *req);
int aai_adjoint_rotated_batch_device_f32(const aai_request *req, int32_t batch,
                                         const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                         float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL */
int aai_adjoint_rotated_f32(const aai_request *req, const float *gdst, int64_t dst_stride,
                            float *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_ADJOINT_ROTATED_H */
