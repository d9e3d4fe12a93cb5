/* aai_adjoint_sample.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the adjoint of the bilinear / bicubic samplers.
 *
 * aai.h holds the adjoint of the area and fast modes (aai_adjoint_batch_device_f32, aai_adjoint_f32), the other extension headers its
 * planned and interleaved forms; all of them refuse AAI_MODE_BILINEAR and AAI_MODE_BICUBIC, and keep doing so.  This header adds the
 * gradient side of those two modes.  It is a header of its own because aai.h is a closed list: every compute entry it declares has
 * its argument errors recorded, entry by entry, in tests/golden/entry_point_errors.json. */
#ifndef AAI_ADJOINT_SAMPLE_H
#define AAI_ADJOINT_SAMPLE_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the samplers' adjoint: gsrc = W^T gdst for AAI_MODE_BILINEAR and AAI_MODE_BICUBIC, fp32 in, fp32 out -------------------
 * The samplers are linear, dst = W src.  Row d of W holds the tap weights of dst pixel d at its sample point -- the dst pixel centre
 * mapped through the request's affine map, quadrant pre-rotation included, exactly as the forward computes it:
 *   bilinear   2 x 2 taps, weights (1 - tx, tx) x (1 - ty, ty)
 *   bicubic    4 x 4 taps, Keys weights with a = -0.5, first tap at offset -1
 * A tap index is clamped into the image and taps that clamp onto the same source pixel add up; a dst pixel whose point lies outside
 * the image extent (guarded by 1e-9 pixels) is a zero row.
 *
 * Arguments: those of aai_adjoint_batch_device_f32 / aai_adjoint_f32 (single channel) and of aai_adjoint_interleaved_device_f32 /
 * aai_adjoint_interleaved_f32 (1..4 interleaved channels: element (x, y, c) of image b at b * image_stride + y * stride + x * channels
 * + c).  Strides in elements.  d_gdst holds `batch` gradient images of the output's size (aai_query), d_gsrc receives `batch` images of
 * src_width x src_height pixels; every element of them is written, zeros included: the caller never clears gsrc.
 *
 * Precision: the integer tap origin and the inside / outside decision are the forward's own (one shared definition); the fractions,
 * the weights, every product and the sum are DOUBLE precision, and the result takes one fp32 rounding.  fp32 weights would not do:
 * the lobes of the cubic cancel, sum |w g| reaches 80 times the magnitude of the result, and the library's 1e-5 bar would be spent
 * on weight rounding alone.  (The forward samples with fp32 weights: W here is the matrix of the sampler in exact arithmetic, within
 * ~1e-7 of what the forward applies.)
 *
 * Validation, before the device is touched: the request as aai_query checks it, with its codes and messages (the policy's rule and
 * bits are validated and otherwise ignored, as the forward's samplers ignore them); AAI_MODE_AREA and AAI_MODE_FAST fail with
 * AAI_ERR_BAD_ARGUMENT and a message that names aai_adjoint_batch_device_f32, whose job they are; batch < 0; null pointers;
 * "Source stride ..." / "Destination stride ..."; for the interleaved entries channels outside 1..4 ("Channels must be 1..4.", right
 * after the request's mode and policy bits) and a row of more than INT32_MAX / 2 elements (AAI_ERR_TOO_LARGE).  batch == 0 returns
 * AAI_OK without touching the device.
 *
 * Memory: only the elements named above are read (d_gdst) or written (d_gsrc).  No scratch, no plan, no side stream: the device entry
 * is one launch per 65535 images and 262140 source rows on `stream`, only enqueues, never synchronises, and can be captured into a
 * graph.
 *
 * Determinism: one gather kernel, one lane per source pixel, no atomics, a fixed summation order (dst rows ascending, then columns):
 * the same bits on every call; image b of a batch gets the bits of a single-image call, channel c the bits of the single-channel call
 * on plane c.
 *
 * aai_last_kernel() afterwards: "aai_adjoint_sample_kernel<bilinear>" or "...<bicubic>", with ", C channels" for C = 2..4.
 * Cost and resources: DESIGN.md section 9.  The interface version (aai.h: AAI_VERSION_MINOR) stays at 2: these are additions in a
 * header of their own. */
int aai_adjoint_sample_batch_device_f32(const aai_request *req, int32_t batch,
                                        const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                        float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL */
int aai_adjoint_sample_f32(const aai_request *req, const float *gdst, int64_t dst_stride,
                           float *gsrc, int64_t src_stride, aai_layout *layout);
int aai_adjoint_sample_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                              const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                              float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
int aai_adjoint_sample_interleaved_f32(const aai_request *req, int32_t channels,
                                       const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_ADJOINT_SAMPLE_H */
