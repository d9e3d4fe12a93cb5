/* aai_adjoint_interleaved.h -- extension of the C ABI (include/aai.h, libaai_hip.so): the adjoint of images with interleaved channels.
 *
 * aai.h holds the resampling entries (aai_resample_interleaved_device / _host among them) and the single-channel adjoint; this header
 * adds the gradient side of the interleaved entries.  It is a header of its own because aai.h is a closed list: every compute entry it
 * declares has its argument errors recorded, entry by entry, in tests/golden/entry_point_errors.json. */
#ifndef AAI_ADJOINT_INTERLEAVED_H
#define AAI_ADJOINT_INTERLEAVED_H

#include "aai.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the interleaved adjoint: gsrc = W^T gdst for 1..4 interleaved channels, fp32 in, fp32 out ----------------------------
 * W is the matrix of aai_resample_interleaved_device with this request (area and fast modes; the same W for every channel).
 * Element (x, y, c) of image b sits at b * image_stride + y * stride + x * channels + c; strides in elements, dst_stride >=
 * dst_width * channels, src_stride >= src_width * channels.  d_gdst holds `batch` gradient images of the output's size (aai_query),
 * d_gsrc receives `batch` images of src_width x src_height pixels; every element of them is written, zeros included.
 *
 * Semantics: channel c of the result is, BIT FOR BIT, what aai_adjoint_batch_device_f32 returns for plane c alone -- the weights of the
 * forward's double-precision fix-up pass, knife edges included, an fp64 sum in the same fixed order, one fp32 rounding.  The weight of
 * a (dst, src) pair does not depend on the channel, so these entries compute it once per pair for all channels
 * (aai_adjoint_norm_multi_kernel<MODE, C>, aai_adjoint_gather_multi_kernel<MODE, C>; aai_last_kernel() names the gather with its mode
 * and channel count); channels == 1 runs the code behind aai_adjoint_batch_device_f32 itself.
 *
 * Validation, before the device is touched: everything aai_adjoint_batch_device_f32 checks, with its codes and messages (the
 * request, bilinear / bicubic and AAI_POLICY_DIAG_NO_FIXUP refused, AAI_POLICY_DOUBLE_PRECISION and AAI_POLICY_PREFER_CELL accepted and
 * ignored, batch < 0, null pointers, "Source stride ..." / "Destination stride ..."); channels outside 1..4 fails with
 * AAI_ERR_BAD_ARGUMENT "Channels must be 1..4." right after the request's mode and policy bits, like the forward's interleaved
 * entries; a row of more than INT32_MAX / 2 elements (width * channels) fails with AAI_ERR_TOO_LARGE as it does there.  batch == 0
 * returns AAI_OK without touching the device.
 *
 * Memory: only the elements named above are read (d_gdst) or written (d_gsrc): the padding between rows and between images and
 * everything outside the buffers is neither read nor written.  Scratch: dst_width x dst_height x channels doubles per image in
 * flight, stream-ordered from the library's retained pool (the single-channel adjoint's); batches whose scratch would exceed about
 * 1 GiB go through in chunks.  The device entry only enqueues on `stream` and never synchronises; no plan is built or used.
 *
 * Determinism: two gather kernels, no atomics, no shared memory, a fixed summation order: the same bits on every call, and image b of
 * a batch gets the bits of a single-image call.
 *
 * Cost: the single-channel kernels sit on the fp64 issue rate of the per-pair code, which these kernels run once instead of
 * `channels` times; each extra channel adds a load and a multiply-add per pair (a load and a division in pass 1).  Register use and
 * occupancy are the single-channel kernels' (gfx950: area 2 waves per SIMD, fast 4 / 3).  NOT MEASURED yet: the
 * ratio of one interleaved call to `channels` single-channel calls on pre-split planes is what `tools/adjoint_time.py --channels`
 * reports; until its table exists, "cheaper than `channels` calls" is design reasoning, not a number.
 * The interface version (aai.h: AAI_VERSION_MINOR) stays at 2: these are additions in a header of their own. */
int aai_adjoint_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                       const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                       float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream);
/* host buffers: upload gdst, run, download gsrc; `layout` may be NULL */
int aai_adjoint_interleaved_f32(const aai_request *req, int32_t channels,
                                const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_ADJOINT_INTERLEAVED_H */
