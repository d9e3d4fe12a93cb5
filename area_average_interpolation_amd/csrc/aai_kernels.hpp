// aai_kernels.hpp -- launcher declarations shared between the host engine (aai_engine.cpp, aai_capi.cpp) and the HIP
// translation units.  Every launcher only enqueues work on `stream`.
#pragma once

#include <hip/hip_runtime.h>

#include "aai_plan.hpp"
#include "aai_rot_math.hpp"
#include "aai_rot_serve.hpp"

#include <cstdlib>

namespace aai {

// ImageView, SrcType, src_elem_size, spans_4gib and the *_can_* predicates of the rotated families: aai_rot_serve.hpp (no HIP type in it)

// ---- K1: axis-aligned separable kernel ----------------------------------------------------------------
struct AxisLaunch {
    const AxisEntry *laneTab;   // device, nA entries (ascending source x)
    const AxisEntry *rowTab;    // device, nB entries (ascending source y)
    const AxisStrip *strips;    // device, nStrips entries
    int nA, nB, nStrips;
    int srcW, srcH;
    int64_t outBase, outStrideA, outStrideB;   // dst element = outBase + ka*outStrideA + kb*outStrideB
    int wide;
    int maxRowSpan;             // largest number of source rows any output row needs
    int rowsShared;             // consecutive output rows share a source row
    int maxOutputsPerStrip;
    // interleaved channels (1 = none): lane entries are (pixel, channel) pairs over the source row's ELEMENTS; the taps of
    // one entry are tapStep elements apart; dst element = outBase + (ka / outChan)*outStrideA + ka % outChan + kb*outStrideB
    // (outChan = 1 when the lane order is already the dst element order: not transposed, not flipped)
    int tapStep, outChan;
    int transposed;             // the lane axis runs along dst y (quadrants 1 and 3)
    // launch shape measured by the plan for this (geometry, device): output rows per workgroup (0 = built-in default),
    // nontemporal source loads (see aai_axis_kernel)
    int tuneRows, tuneNt;
};
hipError_t launch_axis(const AxisLaunch &a, const void *src, int srcType, ImageView sv, float *dst, ImageView dv,
                       int batch, hipStream_t stream, const char **kernelName);
// 0 into the dst pixels of output indices [ka0, ka1) x [kb0, kb1): the rows and columns of empty table entries, behind launch_axis
hipError_t launch_axis_zero(const AxisLaunch &a, int ka0, int ka1, int kb0, int kb1, float *dst, ImageView dv, int batch, hipStream_t stream);

// ---- K2/K3/K4/K5: per-output-pixel kernels on the rotated lattice --------------------------------------
// Flagged dst pixels (geometry only), found once per plan: one 64-bit lane mask per wave of the 16x16-pixel tiling.
// launch_knife_scan marks the pixels with a knife edge of the reference's classifier, launch_quad_scan adds the
// pixels whose decisions the fp32 quad kernel must not take; both count the pixels they newly flag in counter[0].
// launch_flag_list turns the masks into the list of (dx, dy) the double-precision fix-up pass runs over.
struct RotFlags {
    const void *list = nullptr;        // device array of uint2 (dx, dy), `count` entries
    unsigned count = 0;
    bool dense = false;                // so many that the whole image takes the double-precision pass instead
    // With the lane masks kept, the quad kernel leaves the flagged pixels alone, so the fix-up pass no longer has to
    // FOLLOW it: it runs beside it on the plan's side stream (fork / join through two events), where its few,
    // latency-bound waves cost nothing instead of ~40 us behind the production pass.
    const unsigned long long *masks = nullptr;
    const unsigned *tileFlags = nullptr;   // one bit per 16 x 16 tile that holds a flagged pixel (launch_tile_flags), tileFlagWords words per tile row
    int tileFlagWords = 0;
    const int *live = nullptr;         // per 16-row tile row of the canvas: first and last 16-column tile that can hold a non-zero pixel (rotated_live_spans)
    int form = 0;                      // which fp32 formulation's scan produced the flags: ROT_FORM_QUAD or ROT_FORM_CELL (it serves the launch)
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
enum RotForm { ROT_FORM_QUAD = 0, ROT_FORM_CELL = 1 };
size_t rotated_flag_words(const RotLaunch &r);      // waves of the tiling = 64-bit words of the mask array
hipError_t launch_knife_scan(const RotLaunch &r, unsigned long long *laneMasks, unsigned *counter, hipStream_t stream);
// the double-precision fix-up pass over a list of dst pixels (defined in aai_rotated_strict.hip);
// pixelList == NULL: the whole image (grid as for the production pass, at most 65535 tile rows)
void launch_rotated_fixup(const RotLaunch &r, int batch, const void *src, int srcType, ImageView sv, float *dst, ImageView dv,
                          const uint2 *pixelList, unsigned nList, hipStream_t stream);
// axis-aligned geometries (K1): dst pixels whose weights the separable model gets wrong (aai_axis_verify.hpp), same layout
hipError_t launch_axis_verify(const RotLaunch &r, unsigned long long *laneMasks, unsigned *counter, hipStream_t stream);
hipError_t launch_quad_scan(const RotLaunch &r, unsigned long long *laneMasks, unsigned *counter, hipStream_t stream);
// one bit per 16 x 16 tile whose lane masks are not all zero: out[tileRow * rowWords + (tileX >> 5)] bit (tileX & 31); out zeroed by the caller
inline unsigned tile_flag_row_words(unsigned tilesX) { return (tilesX + 31u) / 32u + 1u; }
hipError_t launch_tile_flags(const unsigned long long *laneMasks, unsigned tilesX, unsigned tilesY, unsigned *out, hipStream_t stream);
hipError_t launch_flag_list(const unsigned long long *laneMasks, size_t waves, unsigned tilesX, void *list, unsigned *cursor, unsigned capacity,
                            hipStream_t stream);
hipError_t launch_rotated(const RotLaunch &r, const QuadMap &m, const void *src, int srcType, ImageView sv, float *dst, ImageView dv,
                          int batch, const RotFlags &flags, hipStream_t stream, const char **kernelName);
hipError_t launch_quad(const RotLaunch &r, const QuadMap &m, const void *src, int srcType, ImageView sv, float *dst, ImageView dv,
                       int batch, const unsigned long long *skipMasks, hipStream_t stream, const int *live = nullptr);

// wide footprints (aai_rotated_wide.hip): the quad formulation over a window split into parts, one lane per part
// (wide_can_serve, cell_can_serve: aai_rot_serve.hpp)
hipError_t launch_wide_scan(const RotLaunch &r, unsigned long long *laneMasks, unsigned *counter, hipStream_t stream);
hipError_t launch_wide(const RotLaunch &r, const QuadMap &m, const void *src, int srcType, ImageView sv, float *dst, ImageView dv,
                       int batch, const unsigned long long *skipMasks, hipStream_t stream);

// the cell formulation (aai_rotated_cell.hip): one lane per cell of the dst grid, every (dst, src) pair evaluated once
hipError_t launch_cell_scan(const RotLaunch &r, unsigned long long *laneMasks, unsigned *counter, hipStream_t stream);
hipError_t launch_cell(const RotLaunch &r, const QuadMap &m, const void *src, int srcType, ImageView sv, float *dst, ImageView dv,
                       int batch, const unsigned long long *skipMasks, hipStream_t stream);

// ---- the adjoint of the area / fast modes (aai_adjoint.hip): gsrc = W^T gdst, double precision, every angle ------------
// `batch` <= 65535 images; n = scratch of batch x dH x dW doubles (pass 1 writes it, pass 2 gathers from it)
hipError_t launch_adjoint(const RotLaunch &r, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                          hipStream_t stream, const char **kernelName);

// the same two passes for `channels` = 2..4 interleaved channels (aai_adjoint_multi.hip): a pair's weight is computed once for all
// channels, channel c gets the bits launch_adjoint gives plane c.  gdst / gsrc: element (x, y, c) at y * rowStride + x * channels + c;
// n = scratch of batch x dH x dW x channels doubles, channels innermost.  `batch` <= 65535.
hipError_t launch_adjoint_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                hipStream_t stream, const char **kernelName);

// the same two passes over LISTS of pixels (the correction pass behind the transposed separable kernel): pass 1 over the nDst dst
// pixels of dstList into n (the other elements of n are neither written nor read), pass 2 over the nSrc source pixels of srcList,
// whose gsrc it OVERWRITES.  The lists hold every dst pixel pass 2 reads (build_adjoint_lists).  `batch` <= 65535.
hipError_t launch_adjoint_listed(const RotLaunch &r, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                 const uint2 *dstList, unsigned nDst, const uint2 *srcList, unsigned nSrc, hipStream_t stream);
// pass 2 of the above alone, over an n that is complete already (behind launch_adjoint_plain)
hipError_t launch_adjoint_gather_listed(const RotLaunch &r, int batch, const double *n, float *gsrc, ImageView sv, const uint2 *srcList, unsigned nSrc,
                                        hipStream_t stream);

// ---- the adjoint at general rotations from per-plan sums (aai_adjoint_plain.hip, the one-off sums kernel in aai_adjoint.hip; bodies and the bit-equality argument in
// aai_adjoint_plain.hpp).  Once per geometry: S[d] = the general normaliser's sum (dH x dW doubles), knife[d] = whether a pair of d's
// window reported a knife edge (dH x dW bytes), *count += the number of such pixels; then the flagged pixels as a list through *cursor
// (both words zeroed by the caller; entries beyond `capacity` are dropped).  Only enqueue.
hipError_t launch_adjoint_sums(const RotLaunch &r, double *S, unsigned char *knife, unsigned *count, hipStream_t stream);
hipError_t launch_adjoint_knife_list(const RotLaunch &r, const unsigned char *knife, uint2 *list, unsigned *cursor, unsigned capacity, hipStream_t stream);
// per call: n[b][d] = gdst[b][d] / S[d] (element-wise), then the plain gather over every source pixel, which writes all of gsrc.
// `batch` <= 65535; n holds batch x dH x dW doubles.  Only enqueues.
hipError_t launch_adjoint_plain(const RotLaunch &r, int batch, const float *gdst, ImageView dv, const double *S, double *n, float *gsrc, ImageView sv,
                                hipStream_t stream, const char **kernelName);
// the same for `channels` = 2..4 interleaved channels (aai_adjoint_plain_multi.hip): the element-wise pass 1 over rows of dW x channels
// elements, the plain gather with `channels` accumulators, and -- where nSrc != 0 -- the general multi-channel gather over the plan's
// listed source pixels, which overwrites them.  Channel c gets the bits launch_adjoint_plain (+ launch_adjoint_gather_listed) gives
// plane c.  n holds batch x dH x dW x channels doubles, channels innermost.  `batch` <= 65535.  Only enqueues.
hipError_t launch_adjoint_plain_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, const double *S, double *n, float *gsrc,
                                      ImageView sv, const uint2 *srcList, unsigned nSrc, hipStream_t stream, const char **kernelName);

// ---- the transpose of K1 (aai_axis_adjoint.hip): the adjoint at rotations by multiples of 90 degrees, fp32, from the forward's tables
struct AxisAdjointLaunch {
    const AxisEntry *laneTab;   // the forward plan's tables (device)
    const AxisEntry *rowTab;
    const AxisRange *colRange;  // device, srcW entries: the lane-axis outputs that read source column sx
    const AxisRange *rowRange;  // device, srcH entries: the row-axis outputs that read source row sy
    int srcW, srcH;
    int64_t outBase, outStrideA, outStrideB;   // gdst element of (ka, kb) = outBase + ka*outStrideA + kb*outStrideB (the forward's mapping)
};
hipError_t launch_axis_adjoint(const AxisAdjointLaunch &a, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv,
                               hipStream_t stream, const char **kernelName);

// the same for `channels` = 2..4 interleaved channels (aai_axis_adjoint_multi.hip): one lane per ELEMENT of a source row.  a.srcW / a.srcH
// in pixels and a.outBase / outStrideA / outStrideB the mapping of PIXELS onto elements of gdst (a dst pixel is `channels` elements wide);
// the tables are the single-channel plan's.  Channel c gets the bits launch_axis_adjoint gives plane c.  `batch` <= 65535.
hipError_t launch_axis_adjoint_multi(const AxisAdjointLaunch &a, int channels, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv,
                                     hipStream_t stream, const char **kernelName);
// ... and its correction pass (aai_adjoint_plain_multi.hip): launch_adjoint_listed for `channels` = 2..4, the same lists (they know no
// channels); n holds batch x dH x dW x channels doubles, channels innermost.  Channel c gets the bits launch_adjoint_listed gives plane c.
hipError_t launch_adjoint_listed_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, double *n, float *gsrc, ImageView sv,
                                       const uint2 *dstList, unsigned nDst, const uint2 *srcList, unsigned nSrc, hipStream_t stream);

// ---- the adjoint of the bilinear / bicubic samplers (aai_adjoint_sample.hip; body in aai_adjoint_sample_math.hpp): gsrc = W^T gdst, one
// deterministic gather per source pixel in double precision, every element of gsrc written.  No scratch.  `batch` <= 65535.  Only enqueue.
hipError_t launch_adjoint_sample(const RotLaunch &r, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv, hipStream_t stream,
                                 const char **kernelName);
// the same for `channels` interleaved channels (element (x, y, c) at y * rowStride + x * channels + c): a candidate's weight is computed
// once, channel c gets the bits launch_adjoint_sample gives plane c
hipError_t launch_adjoint_sample_multi(const RotLaunch &r, int channels, int batch, const float *gdst, ImageView dv, float *gsrc, ImageView sv,
                                       hipStream_t stream, const char **kernelName);

// ---- utilities -----------------------------------------------------------------------------------------
hipError_t launch_synth(float *dst, int W, int H, int64_t stride, uint64_t seed, hipStream_t stream);
hipError_t launch_synth_rows(float *dst, int W, int H, int row0, int row1, int64_t stride, uint64_t seed, hipStream_t stream);
hipError_t launch_f64_to_f32(const double *src, float *dst, size_t n, hipStream_t stream);
hipError_t launch_f32_to_f64(const float *src, double *dst, size_t n, hipStream_t stream);

// ---- the reference-precision path (aai_f64.hip): DOUBLE images end to end, area / fast modes, every angle, no plan ------
// forward dst = W src with the weights of aai_adjoint_math.hpp (aai_f64_math.hpp); every dst element written.  `batch` <= 65535.
hipError_t launch_f64_forward(const RotLaunch &r, int batch, const double *src, ImageView sv, double *dst, ImageView dv, hipStream_t stream,
                              const char **kernelName);
// adjoint gsrc = W^T gdst: launch_adjoint's two passes without its final fp32 rounding; n = scratch of batch x dH x dW doubles.
// `batch` <= 65535.
hipError_t launch_f64_adjoint(const RotLaunch &r, int batch, const double *gdst, ImageView dv, double *n, double *gsrc, ImageView sv,
                              hipStream_t stream, const char **kernelName);

// ---- the narrow-element paths (aai_axis_narrow.hip; bodies in aai_half_math.hpp and aai_int_math.hpp): the element type in and out ----
// The element types of include/aai_half.h and include/aai_half_interleaved.h (fp16 / bf16, images of raw 16-bit elements) and
// include/aai_int.h (u8 / u16), each with 1..4 interleaved channels.  The public values AAI_HALF_* and AAI_DTYPE_U* collide, so the engine maps them onto this one.  Strides in elements.
enum NarrowType { NARROW_U8 = 0, NARROW_U16 = 1, NARROW_F16 = 2, NARROW_BF16 = 3 };
constexpr bool narrow_known(int type) { return type >= NARROW_U8 && type <= NARROW_BF16; }
constexpr bool narrow_is_half(int type) { return type == NARROW_F16 || type == NARROW_BF16; }
constexpr size_t narrow_elem_size(int type) { return type == NARROW_U8 ? 1 : 2; }
// The direct kernel over K1's tables: whether it serves a launch block (static facts of the plan: not wide, the lane axis along dst x,
// at most 256 outputs per strip, at least four elements in a source row; 8-bit elements only with more than 64 outputs in some strip:
// the measured rule of profiles/int_time.txt; the half types with channels in every class: profiles/half_interleaved_time.txt) ...
bool axis_narrow_can_serve(const AxisLaunch &a, int type);
// ... and its launch (hipErrorInvalidValue where it does not).  No scratch.  `batch` <= 65535.  *kernelName: what aai_last_kernel()
// reports, "aai_axis_half_kernel<f16|bf16>" or "aai_axis_int_kernel<u8|u16>".
hipError_t launch_axis_narrow(const AxisLaunch &a, int type, const void *src, ImageView sv, void *dst, ImageView dv, int batch, hipStream_t stream,
                              const char **kernelName);
// pitched half images -> dense fp32 images (W x H elements each, image b at b * W * H); the half types only (enqueue() reads u8 / u16
// itself).  `batch` <= 65535.
hipError_t launch_narrow_widen(int type, const void *src, ImageView sv, float *dst, int W, int H, int batch, hipStream_t stream);
// dense fp32 images (W x H elements each -- W = pixels x channels --, image b at b * W * H) -> pitched element images, the one conversion
// of the type: half_narrow or int_quantize.  `batch` <= 65535.
hipError_t launch_narrow_store(int type, const float *src, void *dst, ImageView dv, int W, int H, int batch, hipStream_t stream);

// ---- resample and convert (aai_axis_convert.hip; include/ext/aai_convert.h): u8 / u16 in, scaled fp32 / fp16 / bf16 out ----
// out = round(fma(s, scale[c], offset[c])) in `outType` (CONVERT_F32: not rounded), interleaved (element (x, y, c) at y * rowStride +
// x * channels + c of dv) or planar (c * planeStride + y * rowStride + x).  Strides in elements of the output type.
enum ConvertOut { CONVERT_F32 = 0, CONVERT_F16 = 1, CONVERT_BF16 = 2 };      // AAI_DTYPE_F32 / AAI_HALF_F16 / AAI_HALF_BF16
struct ConvertParams {
    int outType;      // ConvertOut
    int planar;
    int64_t planeStride;
    float scale[4], offset[4];
};
constexpr bool convert_out_known(int outType) { return outType >= CONVERT_F32 && outType <= CONVERT_BF16; }
constexpr size_t convert_out_size(int outType) { return outType == CONVERT_F32 ? 4 : 2; }
// The direct kernel over K1's tables: whether it serves a launch block (the static facts of axis_narrow_can_serve for an integer
// source type `srcType`: NARROW_U8 / NARROW_U16, and the measured rule of profiles/convert_time.txt) ...
bool axis_convert_can_serve(const AxisLaunch &a, int srcType, int outType, int planar);
// ... and its launch (hipErrorInvalidValue where it does not).  a: make_axis_launch's block for `channels` and the dst row stride (its
// flips and tables are read; the dst mapping is the convert kernel's own).  No scratch.  `batch` <= 65535.  *kernelName:
// "aai_axis_convert_kernel<u8|u16,f32|f16|bf16>".
hipError_t launch_axis_convert(const AxisLaunch &a, int srcType, const ConvertParams &cv, const void *src, ImageView sv, void *dst, ImageView dv, int batch,
                               hipStream_t stream, const char **kernelName);
// dense fp32 interleaved images (H rows of W pixels x channels elements, image b at b * W * channels * H) -> pitched converted images:
// the forwarding route's last stage.  `batch` <= 65535.
hipError_t launch_convert_store(const ConvertParams &cv, int channels, const float *src, void *dst, ImageView dv, int W, int H, int batch, hipStream_t stream);

// ---- the half-precision transposed separable kernel (aai_axis_adjoint_narrow.hip; body in aai_axis_adjoint_half_math.hpp) ----
// launch_axis_adjoint_multi's launch block (a.srcW / a.srcH in pixels, the mapping of PIXELS onto elements of gdst, the single-channel
// plan's tables) for `channels` = 1..4 on fp16 / bf16 images (`type`: NARROW_F16 / NARROW_BF16) of raw 16-bit elements: the bits of
// narrow(launch_axis_adjoint[_multi](widen(gdst))).  No scratch.  `batch` <= 65535.  *kernelName: "aai_axis_adjoint_half_kernel<f16|bf16,C>".
hipError_t launch_axis_adjoint_half(const AxisAdjointLaunch &a, int type, int channels, int batch, const void *gdst, ImageView dv, void *gsrc, ImageView sv,
                                    hipStream_t stream, const char **kernelName);

}  // namespace aai
