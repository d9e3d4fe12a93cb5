/* aai_convert.h -- extension of the C ABI (include/aai.h, libaai_hip.so): integer images in, a SCALED FLOATING image out.  The entries
 * of aai.h read 8-bit and 16-bit unsigned sources and write fp32 interleaved; aai_int.h writes the same integer type.  What a caller
 * with integer pixels mostly wants next is a floating tensor, scaled and shifted per channel, often planar, often half precision:
 * the entries below resample and convert in one call, so that no fp32 image four times the size of the result is written, scaled,
 * permuted and narrowed in passes of the caller's own.
 *
 * aai.h and the extension headers beside it are a closed list (tests/test_entry_point_errors.py pins the argument errors of every
 * compute entry they declare); this header lives in include/ext/ and its entries' argument errors are pinned by
 * tests/test_convert_host.py.  The interface version stays 0.2. */
#ifndef AAI_CONVERT_H
#define AAI_CONVERT_H

#include "../aai.h"
#include "../aai_half.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AAI_LAYOUT_INTERLEAVED = 0, AAI_LAYOUT_PLANAR = 1 };

/* The conversion of one call: a plain struct, read on the host during the call and copied into the launch block.  It holds no device
 * pointer and adds nothing to the memory contract. */
typedef struct aai_convert {
    int32_t out_type;     /* AAI_DTYPE_F32 (0), AAI_HALF_F16 (1) or AAI_HALF_BF16 (2): the values do not collide */
    int32_t out_layout;   /* AAI_LAYOUT_INTERLEAVED: element (x, y, c) at y * dst_stride + x * channels + c, dst_plane_stride ignored;
                             AAI_LAYOUT_PLANAR: element (x, y, c) at c * dst_plane_stride + y * dst_stride + x */
    float scale[4];       /* per channel; entries at index >= channels are ignored */
    float offset[4];
} aai_convert;

/* ---- dst = round(fma(resample(src), scale, offset)) on u8 / u16 images -------------------------------------------------------------
 * IMAGES: `src_dtype` is AAI_DTYPE_U8 or AAI_DTYPE_U16; the source holds `channels` (1..4) interleaved channels in the layout of
 * aai_resample_interleaved_device: element (x, y, c) of image b at b * src_image_stride + y * src_stride + x * channels + c.  The
 * output holds cv->out_type in cv->out_layout, image b at b * dst_image_stride.  Strides in elements of the respective type.  All four modes.
 * VALUES (the contract): every source element is taken as its integer value, exactly; the forward's own fp32 weights are applied and
 * the sums s are fp32; then v = fmaf(s, scale[c], offset[c]) in fp32, ONE fused operation; then ONE rounding of v to out_type by the
 * rules of aai_half.h: to nearest, ties to even; what rounds beyond the largest finite fp16 value is +-Inf; NaN becomes the type's
 * canonical quiet NaN; fp32 is not rounded.  An output pixel without weight (a dst row or column off the image) has s = +0, hence the
 * value offset[c], rounded: the canvas is the normalised zero, as if the caller had normalised a zero-padded fp32 result.  Channels never mix.
 * VALIDATION: exactly as aai_resample_interleaved_device (the host entry: aai_resample_interleaved_host) validates, in its order, with
 * its codes and messages; `src_dtype` is checked where aai_int.h checks `dtype` (AAI_DTYPE_F32 and unknown values: AAI_ERR_BAD_ARGUMENT,
 * "Unknown integer element type.").  Then, in this order:
 *   cv == NULL                                          AAI_ERR_BAD_ARGUMENT  "Null conversion."
 *   unknown out_type                                    AAI_ERR_BAD_ARGUMENT  "Unknown output element type."
 *   unknown out_layout                                  AAI_ERR_BAD_ARGUMENT  "Unknown output layout."
 *   a scale or offset among the first `channels`        AAI_ERR_NONFINITE     "Conversion scale and offset must be finite."
 *   that is NaN or +-Inf
 *   planar: dst_stride < dst_width                      AAI_ERR_BAD_ARGUMENT  "Destination stride smaller than the output width."
 *   planar: dst_plane_stride < (dst_height - 1)         AAI_ERR_BAD_ARGUMENT  "Destination plane stride smaller than one plane."
 *           * dst_stride + dst_width
 * The strides -- the two planar checks with them -- are reported where the entry the call is modelled on reports its strides: by the
 * host entry in front of the conversion's checks, by the device entry behind the device check.  Everything else is reported before
 * the device is touched.  batch == 0 returns AAI_OK without touching the device.
 * PLAN: the forward's own, under the key (req, channels): aai_prepare(req, channels) prepares these calls too, aai_plan_info(req,
 * channels) describes the plan, unchanged.  STREAM ORDER: the stream-order contract of aai.h.  MEMORY: the memory contract of aai.h --
 * only entitled elements are read or written; row, plane and image padding is never touched.  Base pointers and strides are assumed
 * aligned to one element of their type and nothing more.
 *
 * TWO ROUTES, chosen per request by static facts of its plan, as in aai_int.h:
 *   direct      aai_query reports AAI_KERNEL_AXIS, the plan is not `dense` and lists no pixel, the rotation is 0 or 180 degrees, the
 *               mode is area or fast, and the strip form applies (not AAI_KERNEL_AXIS_WIDE, at most 256 outputs per strip, at least 4
 *               elements in a source row).  ONE kernel reads the integer image and writes the converted image in its final type and
 *               layout.  No scratch, no fp32 image anywhere.  aai_last_kernel() names "aai_axis_convert_kernel<u8|u16,f32|f16|bf16>".
 *               Which classes keep this route is measured (profiles/convert_time.txt; DESIGN.md, "Resample and convert").
 *   forwarding  everything else -- general rotations, 90 / 270 degrees, AAI_KERNEL_AXIS_WIDE, plans with listed pixels or `dense`, the
 *               samplers, rows of fewer than 4 elements: the code behind aai_resample_interleaved_device reads the integer image into
 *               dense fp32 scratch (stream-ordered from the library's pool, larger batches in chunks, like aai_int.h), one conversion
 *               kernel writes the caller's buffer.  The bits are exactly round(fmaf(aai_resample_interleaved_device(src)[c], scale[c],
 *               offset[c])).  aai_last_kernel() names the fp32 kernel with "+converted" appended.
 * Route agreement, as observed (profiles/convert_parity.txt, the tests' case table): the two routes' sums s differ in the order of a few
 * fp32 operations, by at most 2 units of fp32's last place; the outputs then differ by at most |ds| |scale[c]| before the one rounding to
 * out_type -- at most 2 units of the last place of fp16 / bf16, and of fp32 where the fma does not cancel (where offset[c] is close to
 * -s scale[c] the same absolute difference is many units of the small result).
 *
 * NOT PROVIDED: row bands, the multi-device entry, a pipelined host batch, an adjoint, a direct kernel at 90 / 270 degrees or behind
 * listed pixels.  NOT TESTED: stream capture of the forwarding route (the pool's allocations, like aai_int.h). */
int aai_resample_convert_device(const aai_request *req, int32_t batch, int32_t channels, int32_t src_dtype,
                                const void *d_src, int64_t src_stride, int64_t src_image_stride,
                                const aai_convert *cv,
                                void *d_dst, int64_t dst_stride, int64_t dst_plane_stride, int64_t dst_image_stride, void *stream);
/* host buffers: upload src, run, download dst (one image; a planar dst plane by plane); `layout` may be NULL.  The device entry's bits. */
int aai_resample_convert_host(const aai_request *req, int32_t channels, int32_t src_dtype, const void *src, int64_t src_stride,
                              const aai_convert *cv, void *dst, int64_t dst_stride, int64_t dst_plane_stride, aai_layout *layout);

#ifdef __cplusplus
}
#endif
#endif /* AAI_CONVERT_H */
