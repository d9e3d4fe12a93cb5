// aai_axis_narrow.hip -- the narrow-element paths: images whose elements are narrower than fp32 in, the same element type out.
//   include/aai_half.h   fp16 / bf16, single-channel  (include/aai_half_interleaved.h: 1..4 interleaved channels)
//   include/aai_int.h    u8 / u16, 1..4 interleaved channels
//
//   aai_axis_narrow_kernel<E>   the DIRECT route: K1's streaming form (aai_axis.hip) over the forward plan's cached tables -- strips, lane
//                               and row entries, the (ka, kb) -> dst element map -- for lane axes that run along dst x (rotations by 0 and
//                               180 degrees).  It computes no geometry.  A narrow element cuts the source bytes of a kernel that is bound
//                               by the source read, and the output goes out in the element type: no fp32 image exists anywhere.
//   aai_narrow_widen_kernel<E>  } the FORWARDING route of every other request (aai_engine.cpp: enqueue_narrow): pitched element image ->
//   aai_narrow_store_kernel<E>  } dense fp32 scratch (half types only: enqueue() reads u8 / u16 itself), the fp32 entry's own launches,
//                                 dense fp32 scratch -> pitched element image.
//
// Work decomposition of the direct kernel = K1's, because the plan's strips are built for it: wave64, one wave per strip of 256 source
// ELEMENTS (a row of W x channels of them), four waves (adjacent strips) per workgroup, four elements per lane = ONE 4-byte (u8) or
// 8-byte (2-byte elements) load per lane and source row, the vertical pass in registers with up to four source rows in flight, the row
// of vertical sums parked in a per-wave LDS line and re-indexed by OUTPUT element for the horizontal pass, whose taps are `tapStep`
// elements apart (CH; the single-channel form is compiled without the step).  Waves never synchronise with each other: no workgroup barrier.
// Two forms of the horizontal pass, chosen per strip (wave-uniform) like K1's branches C and D:
//   * up to 64 outputs in the strip (ratios of 4 and more): one output per lane; neighbouring lanes exchange their elements through
//     DPP and the first of them stores them (the type's SmallStore: the four lanes of a quad, or -- half types, one channel -- a pair);
//   * 65 .. 256 outputs (ratios below 4, 1:1, up-sampling -- a strip never holds more than 256, build_axis_strips): four consecutive
//     outputs per lane.
// Stores: where the lane order is the dst element order -- 0 degrees with any channel count (forwards), 180 degrees with one channel
// (backwards) -- four consecutive elements go out as ONE 4-byte (u8) or 8-byte (2-byte elements) store; the tail of a strip, and 180
// degrees with channels (pixels run backwards, the channels of a pixel forwards), element by element.  Every store covers only elements
// its lane computed: nothing is read back, so a dword shared with another wave's strip or with the row padding is never rewritten.
//
// What an element type decides (Elem<E>), and nothing else:
//   u8     v_cvt_f32_ubyte<i> in; round to nearest even, saturate (int_quantize) out; 4-byte packs; channels; quad store
//   u16    shift / mask and convert in; int_quantize out; 8-byte packs; channels; quad store
//   f16    v_cvt_f32_f16 in (exact); v_cvt_f16_f32 with the canonical NaN of aai_half_math.hpp out; u16's packs; channels; pair store
//          with one channel, quad store with more
//   bf16   shift / mask in (the bits ARE the fp32's upper half); f32_to_bf16 out; u16's packs; channels; pair / quad store like f16
// (The pair store is measured, profiles/narrow_time.txt: with the quad store the half 4:1 rows took about 0.5-1 us more of 107-117 us.
// It pairs lanes that are adjacent in memory forwards and backwards, which holds for one channel only: at 180 degrees the pixels of an
// interleaved row run backwards and the channels of a pixel forwards, so with channels the half types take the quad store, whose
// scattered form places every element by itself.)
//
// The arithmetic of an element is aai_half_math.hpp's and aai_int_math.hpp's, operation for operation, and this unit is compiled
// without contraction: the CPU replays of the tests (tests/emulation/narrow_replay.hpp behind half_emulation.cpp and int_emulation.cpp)
// give this kernel's bits.
//
// Memory: loads start no later than element srcW - 4 (park()'s shift rule of K1) and cover source rows of the window only; stores cover
// output elements only; nothing assumes more than element alignment of a base pointer or a stride.
#include "aai_axis_narrow_parts.hpp"

namespace aai {

namespace {

template <int E, bool NT, bool CH, bool PK>
__global__ __launch_bounds__(kWaves * 64) void aai_axis_narrow_kernel(AxisLaunch a, const AxisEntry *__restrict__ laneTab,
                                                                       const AxisEntry *__restrict__ rowTab, const AxisStrip *__restrict__ strips,
                                                                       const typename Elem<E>::T *__restrict__ src, ImageView sv,
                                                                       typename Elem<E>::T *__restrict__ dst, ImageView dv, int rowsPerBlock)
{
    typedef typename Elem<E>::T T;
    __shared__ __attribute__((aligned(16))) float lds[kWaves][64 * VEC + 8];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = (int)blockIdx.x * kWaves + wave;
    if (strip >= a.nStrips) return;   // waves are independent: no barrier is skipped by leaving early

    typedef int i4s __attribute__((ext_vector_type(4)));
    const i4s stq = reinterpret_cast<const i4s *>(strips)[strip];
    const int k0 = stq.x, k1 = stq.y, x0 = stq.z;
    const T *img = src + (int64_t)blockIdx.z * sv.imageStride;
    T *out = dst + (int64_t)blockIdx.z * dv.imageStride + a.outBase;
    float *line = lds[wave];
    const int col = x0 + VEC * lane;
    const int colc = min(col, a.srcW - VEC);        // srcW >= VEC (the route's predicate)
    const int shift = col - colc;

    const int rowStart = (int)blockIdx.y * rowsPerBlock;
    const int rowEnd = min(rowStart + rowsPerBlock, a.nB);
    const int nOut = k1 - k0;
    const int step = CH ? a.tapStep : 1;
    const bool fwd = a.outStrideA == 1;              // PK: the lane order is the dst element order (fwd) or its reverse (one channel at 180 degrees)

    if (nOut <= 64) {
        const bool live = lane < nOut;
        const Win c = lane_win<CH>(laneTab, live ? k0 + lane : k0, step);
        const typename Elem<E>::template SmallStore<CH, PK> st(a, k0, k1, lane, fwd);
        for (int kb = rowStart; kb < rowEnd; ++kb) {
            const Win e = load_win(rowTab, kb);
            unsigned v = 0u;
            if (!half_entry_empty(e.wF, e.wM, e.wL)) {      // (wave-uniform) a dst row off the image reads nothing
                const Cols s = vertical_pass<E, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, s);
                __builtin_amdgcn_wave_barrier();
                v = element<E, CH>(line, c, x0, step);
            }
            st.store(out + (int64_t)kb * a.outStrideB, v);
        }
    } else {
        const int kq = k0 + 4 * lane;
        const int n = min(max(k1 - kq, 0), 4);                   // how many of this lane's four outputs exist
        const Win c0 = lane_win<CH>(laneTab, n > 0 ? kq : k0, step), c1 = lane_win<CH>(laneTab, n > 1 ? kq + 1 : k0, step);
        const Win c2 = lane_win<CH>(laneTab, n > 2 ? kq + 2 : k0, step), c3 = lane_win<CH>(laneTab, n > 3 ? kq + 3 : k0, step);
        const Scatter sc = PK ? Scatter{} : make_scatter(a, kq);
        for (int kb = rowStart; kb < rowEnd; ++kb) {
            const Win e = load_win(rowTab, kb);
            unsigned v0 = 0u, v1 = 0u, v2 = 0u, v3 = 0u;
            if (!half_entry_empty(e.wF, e.wM, e.wL)) {
                const Cols s = vertical_pass<E, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, s);
                __builtin_amdgcn_wave_barrier();
                v0 = element<E, CH>(line, c0, x0, step);
                v1 = element<E, CH>(line, c1, x0, step);
                v2 = element<E, CH>(line, c2, x0, step);
                v3 = element<E, CH>(line, c3, x0, step);
            }
            store_outputs<T, PK>(out + (int64_t)kb * a.outStrideB, sc, fwd, kq, n, v0, v1, v2, v3);
        }
    }
}

// ---- the forwarding route's conversions: lane = four consecutive elements of a row (W elements: pixels x channels), one 4- / 8-byte
// access on the element side and one 16-byte access on the fp32 side (element-aligned both: rows of any width and pitch); the last
// elements of a row one by one.  Padding is not touched.
template <int E>
__global__ __launch_bounds__(256) void aai_narrow_widen_kernel(const typename Elem<E>::T *__restrict__ src, ImageView sv, float *__restrict__ dst, int W, int H)
{
    typedef typename Elem<E>::T T;
    const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    if (x >= W) return;
    const T *img = src + (int64_t)blockIdx.z * sv.imageStride;
    float *o = dst + (int64_t)blockIdx.z * ((int64_t)W * H);
    for (int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); y < H; y += (int)gridDim.y * 4) {
        const T *p = img + (int64_t)y * sv.rowStride + x;
        float *q = o + (int64_t)y * W + x;
        if (x + 4 <= W) {
            Pack<T> r;
            r.template load<false>(p);
            const f4 v = {Elem<E>::to_float(r, 0), Elem<E>::to_float(r, 1), Elem<E>::to_float(r, 2), Elem<E>::to_float(r, 3)};
            *reinterpret_cast<f4u *>(q) = v;
        } else {
            for (int i = 0; x + i < W; ++i) q[i] = Elem<E>::widen(p[i]);
        }
    }
}

template <int E>
__global__ __launch_bounds__(256) void aai_narrow_store_kernel(const float *__restrict__ src, typename Elem<E>::T *__restrict__ dst, ImageView dv, int W, int H)
{
    typedef typename Elem<E>::T T;
    const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    if (x >= W) return;
    const float *img = src + (int64_t)blockIdx.z * ((int64_t)W * H);
    T *o = dst + (int64_t)blockIdx.z * dv.imageStride;
    for (int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); y < H; y += (int)gridDim.y * 4) {
        const float *p = img + (int64_t)y * W + x;
        T *q = o + (int64_t)y * dv.rowStride + x;
        if (x + 4 <= W) {
            const f4 v = *reinterpret_cast<const f4u *>(p);
            Pack<T>::store(q, Elem<E>::from_float(v.x), Elem<E>::from_float(v.y), Elem<E>::from_float(v.z), Elem<E>::from_float(v.w));
        } else {
            for (int i = 0; x + i < W; ++i) q[i] = (T)Elem<E>::from_float(p[i]);
        }
    }
}

dim3 convert_grid(int W, int H, int batch)
{
    return dim3((unsigned)((W + 255) / 256), (unsigned)std::min((H + 3) / 4, 65535), (unsigned)batch);
}

template <int E>
hipError_t launch_axis_typed(const AxisLaunch &a, const AxisShape &shape, const void *src, ImageView sv, void *dst, ImageView dv, hipStream_t stream)
{
    typedef typename Elem<E>::T T;
    const T *s = static_cast<const T *>(src);
    T *d = static_cast<T *>(dst);
    const dim3 grid(shape.gridX, shape.gridY, shape.gridZ), block(kWaves * 64);
    const int rows = shape.rows;
#define AAI_NARROW_LAUNCH(NT, CH, PK) hipLaunchKernelGGL((aai_axis_narrow_kernel<E, NT, CH, PK>), grid, block, 0, stream, a, a.laneTab, a.rowTab, a.strips, s, sv, d, dv, rows)
    const bool pk = a.outStrideA == 1 || a.outStrideA == -1;
    if (a.tapStep > 1) {
        // (with channels the packed form is 0 degrees, the scattered one 180 degrees)
        if (pk) { if (shape.nt) AAI_NARROW_LAUNCH(true, true, true); else AAI_NARROW_LAUNCH(false, true, true); }
        else { if (shape.nt) AAI_NARROW_LAUNCH(true, true, false); else AAI_NARROW_LAUNCH(false, true, false); }
        return hipGetLastError();
    }
    if (!pk) return hipErrorInvalidValue;      // (one channel: outStrideA is +-1)
    if (shape.nt) AAI_NARROW_LAUNCH(true, false, true); else AAI_NARROW_LAUNCH(false, false, true);
#undef AAI_NARROW_LAUNCH
    return hipGetLastError();
}

const char *const kNames[4] = {Elem<NARROW_U8>::kName, Elem<NARROW_U16>::kName, Elem<NARROW_F16>::kName, Elem<NARROW_BF16>::kName};

}  // namespace

bool axis_narrow_can_serve(const AxisLaunch &a, int type)
{
    if (!narrow_known(type) || a.wide || a.transposed || a.srcW < VEC || a.maxOutputsPerStrip > 256) return false;
    if (narrow_is_half(type) && a.tapStep <= 1) return a.outStrideA == 1 || a.outStrideA == -1;      // single-channel
    // Half types with channels: u16's rule, every class kept.  Measured (profiles/half_interleaved_time.txt: 4096^2 -> 4096^2, 2048^2 and
    // 1024^2 at 0 and 180 degrees, 3 and 4 channels, fp16 and bf16, two runs): the kernel is 0.29-0.58 of the forwarding route's time with
    // more than 64 outputs in some strip and 0.31-0.36 with at most 64, faster beyond the spread in all 24 rows of both runs (the same
    // row's medians differ by at most 10 % from run to run).
    if (narrow_is_half(type)) return true;
    // Measured (profiles/int_time.txt): with more than 64 outputs in some strip (ratios below 4, 1:1, up-sampling) the kernel is 0.54-0.83 of
    // the forwarding route's time for both integer types and every channel count, and with 16-bit elements also at 4:1 (0.72-0.83); with
    // 8-bit elements and at most 64 outputs per strip it is not faster beyond the run's spread (0.80-0.98), so that class forwards.
    return a.maxOutputsPerStrip > 64 || type == NARROW_U16;
}

hipError_t launch_axis_narrow(const AxisLaunch &a, int type, const void *src, ImageView sv, void *dst, ImageView dv, int batch, hipStream_t stream,
                              const char **kernelName)
{
    if (!narrow_known(type)) return hipErrorInvalidValue;
    if (kernelName) *kernelName = kNames[type];
    if (!axis_narrow_can_serve(a, type)) return hipErrorInvalidValue;
    // K1's launch rules for a 1- / 2-byte source (axis_launch_shape): nontemporal loads unless output rows share source rows, output rows
    // per workgroup by the rows of a window and the element size.  The plan's measured shape (tuneRows) is fp32's and is not used.
    const AxisShapeFacts facts{a.nA, a.nB, a.nStrips, 0, a.maxRowSpan, a.rowsShared, a.maxOutputsPerStrip, 0, a.tapStep, a.outStrideB, 0, 0,
                               (int)narrow_elem_size(type), batch};
    const AxisShape shape = axis_launch_shape(facts);
    if (shape.kernel == AXIS_RUN_NOTHING) return hipSuccess;
    if (shape.kernel != AXIS_RUN_STRIP) return hipErrorInvalidValue;
    switch (type) {
    case NARROW_U8: return launch_axis_typed<NARROW_U8>(a, shape, src, sv, dst, dv, stream);
    case NARROW_U16: return launch_axis_typed<NARROW_U16>(a, shape, src, sv, dst, dv, stream);
    case NARROW_F16: return launch_axis_typed<NARROW_F16>(a, shape, src, sv, dst, dv, stream);
    default: return launch_axis_typed<NARROW_BF16>(a, shape, src, sv, dst, dv, stream);
    }
}

hipError_t launch_narrow_widen(int type, const void *src, ImageView sv, float *dst, int W, int H, int batch, hipStream_t stream)
{
    if (W <= 0 || H <= 0 || batch <= 0) return hipSuccess;
    if (!narrow_is_half(type)) return hipErrorInvalidValue;
    const unsigned short *s = static_cast<const unsigned short *>(src);
    if (type == NARROW_F16) hipLaunchKernelGGL((aai_narrow_widen_kernel<NARROW_F16>), convert_grid(W, H, batch), dim3(256), 0, stream, s, sv, dst, W, H);
    else hipLaunchKernelGGL((aai_narrow_widen_kernel<NARROW_BF16>), convert_grid(W, H, batch), dim3(256), 0, stream, s, sv, dst, W, H);
    return hipGetLastError();
}

hipError_t launch_narrow_store(int type, const float *src, void *dst, ImageView dv, int W, int H, int batch, hipStream_t stream)
{
    if (W <= 0 || H <= 0 || batch <= 0) return hipSuccess;
    if (!narrow_known(type)) return hipErrorInvalidValue;
    const dim3 grid = convert_grid(W, H, batch), block(256);
    unsigned short *d = static_cast<unsigned short *>(dst);
    switch (type) {
    case NARROW_U8: hipLaunchKernelGGL((aai_narrow_store_kernel<NARROW_U8>), grid, block, 0, stream, src, static_cast<unsigned char *>(dst), dv, W, H); break;
    case NARROW_U16: hipLaunchKernelGGL((aai_narrow_store_kernel<NARROW_U16>), grid, block, 0, stream, src, d, dv, W, H); break;
    case NARROW_F16: hipLaunchKernelGGL((aai_narrow_store_kernel<NARROW_F16>), grid, block, 0, stream, src, d, dv, W, H); break;
    default: hipLaunchKernelGGL((aai_narrow_store_kernel<NARROW_BF16>), grid, block, 0, stream, src, d, dv, W, H); break;
    }
    return hipGetLastError();
}

}  // namespace aai
