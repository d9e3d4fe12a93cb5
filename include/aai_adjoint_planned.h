/* aai_adjoint_planned.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the planned adjoint.
 *
 * aai.h holds the resampling entries and the general adjoint; this header adds the adjoint that uses the forward's cached plan.  It
 * is a header of its own because aai.h is a closed list: every compute entry it declares has its argument errors recorded, entry by
 * entry, in tests/golden/entry_point_errors.json.  The entries below validate exactly like aai_adjoint_batch_device_f32 /
 * aai_adjoint_f32 (tests/test_adjoint_planned_host.py compares them call by call). */
#ifndef AAI_ADJOINT_PLANNED_H
#define AAI_ADJOINT_PLANNED_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the planned adjoint: the transposed separable kernel at rotations by multiples of 90 degrees -----------------------
 * Same contract as aai_adjoint_batch_device_f32 / aai_adjoint_f32 of aai.h -- the same validation in the same order with the same
 * messages, bilinear / bicubic and AAI_POLICY_DIAG_NO_FIXUP refused, AAI_POLICY_DOUBLE_PRECISION and AAI_POLICY_PREFER_CELL accepted
 * and ignored, every element of gsrc written (zeros included), nothing outside the entitled elements read or written, batch == 0
 * returns before the device is touched -- with one difference: these calls apply the transpose of the matrix the FORWARD KERNELS
 * apply, and they use the request's cached plan.
 *   - Axis-aligned requests (aai_query reports AAI_KERNEL_AXIS; single channel; the plan is not `dense`): the forward at these
 *     rotations is the separable streaming kernel, dst(ka, kb) = sum of wrow(kb, sy) wlane(ka, sx) src[sy][sx] over two windows
 *     from the plan's fp32 tables.  aai_axis_adjoint_kernel is its transpose from the SAME tables: one lane per source column,
 *     gsrc[sy][sx] = sum over the outputs kb whose row window holds sy of wrow(kb, sy) x (sum over the outputs ka whose lane
 *     window holds sx of wlane(ka, sx) gdst(ka, kb)); quadrants, flips, the dst stride and the integer pre-expansion are the
 *     tables' and the forward's output mapping, the kernel computes no geometry.  gsrc is written once and gdst read once or a
 *     few times from cache.
 *     Precision: fp32 weights (the forward's normalised table entries) and fp32 fused multiply-add sums, a result within a few
 *     1e-7 relative of the general adjoint -- inside the project's 1e-5 bar; a fixed summation order (ka ascending inside kb
 *     ascending), no atomics: deterministic, and image b of a batch gets the bits of a single-image call.
 *     Flagged pixels: where the plan lists dst pixels whose weights are NOT the product of the two tables (aai_plan_info:
 *     flagged=; the forward recomputes them in its double-precision fix-up pass), the source pixels inside their windows are
 *     recomputed behind the separable kernel by the general adjoint's own per-pixel code, over lists built with the tables
 *     (one lane per listed dst pixel, then one per listed source pixel, which OVERWRITES gsrc there; fp64 scratch of the dst
 *     size from the adjoint's pool, only when the lists are not empty).  Listed source pixels carry the bits of
 *     aai_adjoint_batch_device_f32, all others the separable kernel's.  aai_last_kernel() names "aai_axis_adjoint_kernel",
 *     with "+listed" appended when that correction pass ran.
 *   - The plan is the forward's own, looked up with the forward's key: a request shares ONE plan between aai_resample_* and
 *     these calls; a missing plan is built exactly as aai_prepare builds it.  It gains adjoint tables -- per source column and
 *     per source row the range of outputs that read it (two int32 each), and the two lists above -- built on the host from the
 *     forward's tables by the first planned call of a geometry on a device.  That call therefore SYNCHRONISES, like the forward's
 *     first call; aai_adjoint_prepare (= aai_prepare plus the adjoint tables) takes the cost up front, later calls only enqueue.
 *     aai_plan_info reports adjoint=tables once they exist, adjoint=none otherwise; aai_shutdown frees them with the plan.
 *   - Everything else -- general rotations, AAI_KERNEL_AXIS_WIDE, `dense` plans, a table whose inversion fails its consistency
 *     check, a correction list over more than half of the source image -- is forwarded to the code behind
 *     aai_adjoint_batch_device_f32: identical bits, aai_last_kernel() names the gather kernel, aai_adjoint_prepare is a validated
 *     no-op (it still builds the forward's plan of an axis-aligned request).
 *   - Why both exist: aai_adjoint_batch_device_f32 is unchanged -- one double-precision code path for every rotation, no plan, no
 *     synchronisation, the transpose of the reference's weights to one fp32 rounding.  The planned entries trade that for speed
 *     where the forward is the separable kernel (MEASURED: profiles/adjoint_axis_time.txt).  A caller that needs bit-identical
 *     gradients across library versions or rotations keeps the former; a training loop through an axis-aligned down-sampling
 *     wants the latter (torch: resample(..., planned_backward=True)).
 * The interface version (aai.h: AAI_VERSION_MINOR) stays at 2: these are additions in a header of their own, and every entry of
 * aai.h keeps its behaviour. */
int aai_adjoint_prepare(const aai_request *req);
int aai_adjoint_planned_batch_device_f32(const aai_request *req, int32_t batch,
                                         const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                         float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL */
int aai_adjoint_planned_f32(const aai_request *req, const float *gdst, int64_t dst_stride,
                            float *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_ADJOINT_PLANNED_H */
