/* aai_f64.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the reference-precision path.  Forward and adjoint of the area
 * and fast modes on DOUBLE images from end to end, the reference's own element type (IMG = vector<vector<double>>).
 *
 * aai.h is a closed list (tests/golden/entry_point_errors.json pins the argument errors of every compute entry it declares) and the
 * interface version stays 0.2, so these entries have a header of their own, like aai_adjoint_planned.h.  aai_resample_f64 of aai.h
 * keeps its behaviour: it rounds its source to fp32 on the device and widens an fp32 result, and AAI_POLICY_DOUBLE_PRECISION computes
 * in fp64 between fp32 loads and stores -- neither gets below the ~6e-8 of one fp32 rounding.  The entries below never round a value
 * to fp32: they are within ~1e-12 of the reference on the reference's own recorded outputs (DESIGN.md section 9 quotes the measured
 * distances), which is what validating against Source.cpp, data that spans decades, torch.autograd.gradcheck and iterative solvers
 * on W / W^T need. */
#ifndef AAI_F64_H
#define AAI_F64_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dst = W src and gsrc = W^T gdst on doubles ----------------------------------------------------------------------------
 * W is the matrix of aai_adjoint_batch_device_f32: a (dst, src) pair's weight is the overlap area (area mode) or the membership of
 * the source pixel's centre (fast mode), in double precision with the strict replay of the reference's classifier at knife edges,
 * divided by the dst pixel's sum of weights; a dst pixel whose sum does not count is 0.  The forward and both passes of the adjoint
 * evaluate a pair with the same code from the same operands, so the adjoint is the transpose of the forward to a few ulps per
 * element.  One code path for every rotation, multiples of 90 degrees included (correct there, not fast).
 *
 * VALIDATION: exactly as aai_adjoint_batch_device_f32 validates, in the same order with the same messages, before any device call:
 * the request, batch < 0, the geometry, the mode (AAI_MODE_BILINEAR / AAI_MODE_BICUBIC: AAI_ERR_BAD_ARGUMENT, the message names the
 * mode), AAI_POLICY_DIAG_NO_FIXUP (refused), null pointers, strides.  The rule bits of the policy (AAI_POLICY_REFERENCE /
 * AAI_POLICY_EXACT) are honoured; AAI_POLICY_DOUBLE_PRECISION and AAI_POLICY_PREFER_CELL are accepted and ignored.  batch == 0
 * returns AAI_OK without touching the device.
 * NO PLAN: nothing is built, scanned or prepared and no call synchronises, the first included.  The device entries only enqueue on
 * `stream`, keep the stream-order contract of aai.h, and can be captured into a graph as they stand.  The adjoint takes its scratch
 * (one double per dst pixel per image in flight, at most 1 GiB per round of launches) from the library's stream-ordered pool, like
 * aai_adjoint_batch_device_f32 (the pool itself is created, on the host, by the first adjoint call of a process on a device).
 * IMAGES: single-channel; strides in elements (doubles); image b at b * image_stride.  Every element of the output is written, zeros
 * included; nothing outside the entitled elements is read or written; a source pixel is read only where its weight is not 0, so a
 * non-finite source pixel reaches exactly the dst pixels that carry weight on it.  A batch of any size (split at 65,535 images).
 * aai_last_kernel() names "aai_f64_forward_kernel<area>" / "<fast>" and "aai_f64_adjoint_gather_kernel<area>" / "<fast>".
 * NOT PROVIDED: interleaved channels, row bands, the multi-device entry, a separable kernel for multiples of 90 degrees.  Offsets
 * are 64-bit throughout.  EXERCISED: views that span 4 GiB and more (2^29 doubles) through a wide row pitch, on the source side and on
 * the dst side, forward and adjoint (tests/test_wide_pitch_gpu.py).  NOT EXERCISED: a dense double image of 4 GiB. */
int aai_resample_batch_device_f64(const aai_request *req, int32_t batch,
                                  const double *d_src, int64_t src_stride, int64_t src_image_stride,
                                  double *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream);
/* host buffers: upload src, run, download dst; `layout` may be NULL.  The device entry's bits. */
int aai_resample_exact_f64(const aai_request *req, const double *src, int64_t src_stride,
                           double *dst, int64_t dst_stride, aai_layout *layout);
int aai_adjoint_batch_device_f64(const aai_request *req, int32_t batch,
                                 const double *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                 double *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL.  The device entry's bits. */
int aai_adjoint_f64(const aai_request *req, const double *gdst, int64_t dst_stride,
                    double *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_F64_H */
