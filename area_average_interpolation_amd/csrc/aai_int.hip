// aai_int.hip -- the integer path (include/aai_int.h): 8- / 16-bit unsigned images of 1..4 interleaved channels in, the same type out.
//
//   aai_axis_int_kernel<T>     the DIRECT route: K1's streaming form (aai_axis.hip) over the forward plan's cached tables -- strips, lane
//                              and row entries, the (ka, kb) -> dst element map -- for lane axes that run along dst x (rotations by 0 and
//                              180 degrees).  It computes no geometry.  The output goes out in the element type: no fp32 image exists.
//   aai_int_quantize_kernel<T> the FORWARDING route of every other request (aai_engine.cpp: enqueue_int): enqueue() reads the integer
//                              image itself and writes dense fp32 scratch; this kernel converts the scratch into the caller's buffer.
//
// Work decomposition of the direct kernel = K1's, because the plan's strips are built for it: wave64, one wave per strip of 256 source
// ELEMENTS (a row of W x channels of them), four waves (adjacent strips) per workgroup, four elements per lane = ONE 4-byte (u8) or
// 8-byte (u16) load per lane and source row, the vertical pass in registers with up to four source rows in flight, the row of vertical
// sums parked in a per-wave LDS line and re-indexed by OUTPUT element for the horizontal pass, whose taps are `tapStep` elements apart
// (CH; the single-channel form is compiled without the step).  Waves never synchronise with each other: no workgroup barrier.
// Two forms of the horizontal pass, chosen per strip (wave-uniform) like K1's branches C and D:
//   * up to 64 outputs in the strip: one output per lane; the four lanes of a quad exchange their elements through DPP and the quad's
//     first lane stores them;
//   * 65 .. 256 outputs (a strip never holds more, build_axis_strips): four consecutive outputs per lane.
// Stores: where the lane order is the dst element order -- 0 degrees with any channel count (forwards), 180 degrees with one channel
// (backwards) -- four consecutive elements go out as ONE 4-byte (u8) or 8-byte (u16) store; the tail of a strip, and 180 degrees with
// channels (pixels run backwards, the channels of a pixel forwards), element by element.  Every store covers only elements its lane
// computed: nothing is read back, so a dword shared with another wave's strip or with the row padding is never rewritten.
//
// The arithmetic of an element is aai_int_math.hpp's (and aai_half_math.hpp's), operation for operation, and this unit is compiled
// without contraction: the CPU replay of the tests (tests/emulation/int_emulation.cpp) gives this kernel's bits.
//
// Memory: loads start no later than element srcW - 4 (park()'s shift rule of K1) and cover source rows of the window only; stores cover
// output elements only; nothing assumes more than element alignment of a base pointer or a stride.
#include "aai_kernels.hpp"
#include "aai_int_math.hpp"

#include <algorithm>

namespace aai {

namespace {

constexpr int kWaves = kAxisWaves;
constexpr int VEC = 4;         // source elements per lane and load

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));             // dword-aligned 16-byte access
typedef float f4 __attribute__((ext_vector_type(4)));

// VEC consecutive elements of one row, as loaded and as stored (the element-aligned vector types of Raw<T>, aai_axis.hip)
template <typename T> struct Pack;

template <> struct Pack<unsigned char> {
    typedef unsigned int word __attribute__((aligned(1)));
    unsigned w;
    template <bool NT> __device__ __forceinline__ void load(const unsigned char *p)
    {
        const word *v = reinterpret_cast<const word *>(p);
        w = NT ? __builtin_nontemporal_load(v) : *v;
    }
    __device__ __forceinline__ float get(int i) const { return (float)((w >> (8 * i)) & 255u); }     // v_cvt_f32_ubyte<i>
    // elements e0 .. e3 at p[0] .. p[3]
    static __device__ __forceinline__ void store(unsigned char *p, unsigned e0, unsigned e1, unsigned e2, unsigned e3)
    {
        *reinterpret_cast<word *>(p) = e0 | (e1 << 8) | (e2 << 16) | (e3 << 24);
    }
};

template <> struct Pack<unsigned short> {
    typedef unsigned int word2 __attribute__((ext_vector_type(2), aligned(2)));
    unsigned w0, w1;
    template <bool NT> __device__ __forceinline__ void load(const unsigned short *p)
    {
        const word2 *v = reinterpret_cast<const word2 *>(p);
        const word2 x = NT ? __builtin_nontemporal_load(v) : *v;
        w0 = x.x; w1 = x.y;
    }
    __device__ __forceinline__ float get(int i) const { return (float)(((i < 2 ? w0 : w1) >> (16 * (i & 1))) & 65535u); }
    static __device__ __forceinline__ void store(unsigned short *p, unsigned e0, unsigned e1, unsigned e2, unsigned e3)
    {
        word2 r;
        r.x = e0 | (e1 << 16); r.y = e2 | (e3 << 16);
        *reinterpret_cast<word2 *>(p) = r;
    }
};

// a table entry in registers; `span` = number of taps - 1 (of a lane entry: (s1 - s0) / tapStep, worked out once per strip)
struct Win { int s0, s1; float wF, wM, wL; };

__device__ __forceinline__ Win load_win(const AxisEntry *__restrict__ tab, int k)
{
    typedef int i4 __attribute__((ext_vector_type(4)));
    const i4 q = reinterpret_cast<const i4 *>(tab)[2 * k];
    const float wl = reinterpret_cast<const float *>(tab)[8 * k + 4];
    Win w;
    w.s0 = q.x; w.s1 = q.y; w.wF = __int_as_float(q.z); w.wM = __int_as_float(q.w); w.wL = wl;
    return w;
}

struct Cols { float v[VEC]; };

// Vertical pass of one output row: acc = fma(w(y), src[y][col], acc) over the window's rows in ascending order (half_vertical_step).
// Up to four source rows are issued together; the window is wave-uniform, so rows past it are neither loaded nor added.
template <typename T, bool NT>
__device__ __forceinline__ Cols vertical_pass(const T *__restrict__ img, int64_t rowStride, int colc, const Win e)
{
    Cols acc;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc.v[i] = 0.f;
    for (int y = e.s0; y <= e.s1; y += 4) {
        Pack<T> r0, r1, r2, r3;
        const T *p = img + (int64_t)y * rowStride + colc;
        const bool h1 = y + 1 <= e.s1, h2 = y + 2 <= e.s1, h3 = y + 3 <= e.s1;
        r0.template load<NT>(p);
        r1 = r0; r2 = r0; r3 = r0;
        if (h1) r1.template load<NT>(p + rowStride);
        if (h2) r2.template load<NT>(p + 2 * rowStride);
        if (h3) r3.template load<NT>(p + 3 * rowStride);
        const float w0 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y), w1 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y + 1);
        const float w2 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y + 2), w3 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y + 3);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w0, r0.get(i));
        if (h1) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w1, r1.get(i));
        }
        if (h2) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w2, r2.get(i));
        }
        if (h3) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w3, r3.get(i));
        }
    }
    return acc;
}

// K1's park(): the lane's VEC vertical sums into the wave's LDS line (position = element - strip origin).  Near the right image edge a
// lane loaded the last in-range vector instead of its own (colc = min(col, srcW - VEC), shift = col - colc) and writes only the
// elements at or right of its own first one.
__device__ __forceinline__ void park(float *line, int lane, int shift, const Cols &c)
{
    if (shift == 0) {
        const f4 v = {c.v[0], c.v[1], c.v[2], c.v[3]};
        *reinterpret_cast<f4 *>(line + VEC * lane) = v;
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (i >= shift) line[VEC * lane + i - shift] = c.v[i];
    }
}

// one output element from the parked line, converted: 0 for an entry without weight (a dst column off the image).  c.s1 holds the
// entry's span (taps - 1), not its last element.
template <typename T, bool CH>
__device__ __forceinline__ unsigned element(const float *line, const Win c, int x0, int step)
{
    if (half_entry_empty(c.wF, c.wM, c.wL)) return 0u;
    const float s = CH ? int_horizontal_stepped(line, c.s0 - x0, c.s1, step, c.wF, c.wM, c.wL) : half_horizontal(line, c.s0 - x0, c.s1, c.wF, c.wM, c.wL);
    return (unsigned)int_quantize<T>(s);
}

template <bool CH> __device__ __forceinline__ Win lane_win(const AxisEntry *__restrict__ laneTab, int k, int step)
{
    Win c = load_win(laneTab, k);
    c.s1 = CH ? (c.s1 - c.s0) / step : c.s1 - c.s0;
    return c;
}

// The up to four consecutive outputs kq .. kq + n - 1 of one lane into dst row `row` (= out + kb * outStrideB).
//   PK (the lane order is the dst element order, forwards or backwards): all four as one store, fewer one by one
//   else (180 degrees with channels): element (ka / outChan) * outStrideA + ka % outChan each, worked out once per strip (Scatter)
struct Scatter { int o[4]; };       // element offsets within a dst row: below 2^30 (check_row_length)

__device__ __forceinline__ Scatter make_scatter(const AxisLaunch &a, int kq)
{
    Scatter s;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int ka = kq + i; s.o[i] = (ka / a.outChan) * (int)a.outStrideA + ka % a.outChan; }
    return s;
}

template <typename T, bool PK>
__device__ __forceinline__ void store_outputs(T *row, const Scatter &sc, bool fwd, int kq, int n, unsigned e0, unsigned e1, unsigned e2, unsigned e3)
{
    if (n <= 0) return;
    if (PK) {
        T *o = row + (fwd ? (int64_t)kq : -(int64_t)kq);
        if (n == 4) {
            if (fwd) Pack<T>::store(o, e0, e1, e2, e3);
            else Pack<T>::store(o - 3, e3, e2, e1, e0);
        } else {
            const int64_t sA = fwd ? 1 : -1;
            o[0] = (T)e0;
            if (n > 1) o[sA] = (T)e1;
            if (n > 2) o[2 * sA] = (T)e2;
        }
    } else {
        row[sc.o[0]] = (T)e0;
        if (n > 1) row[sc.o[1]] = (T)e1;
        if (n > 2) row[sc.o[2]] = (T)e2;
        if (n > 3) row[sc.o[3]] = (T)e3;
    }
}

template <typename T, bool NT, bool CH, bool PK>
__global__ __launch_bounds__(kWaves * 64) void aai_axis_int_kernel(AxisLaunch a, const AxisEntry *__restrict__ laneTab,
                                                                    const AxisEntry *__restrict__ rowTab, const AxisStrip *__restrict__ strips,
                                                                    const T *__restrict__ src, ImageView sv, T *__restrict__ dst, ImageView dv, int rowsPerBlock)
{
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
        // the quad's first lane stores the quad's elements: n of them exist
        const int kq = k0 + (lane & ~3);
        const int n = (lane & 3) == 0 ? min(max(k1 - kq, 0), 4) : 0;
        const Scatter sc = PK ? Scatter{} : make_scatter(a, kq);
        for (int kb = rowStart; kb < rowEnd; ++kb) {
            const Win e = load_win(rowTab, kb);
            unsigned v = 0u;
            if (!half_entry_empty(e.wF, e.wM, e.wL)) {      // (wave-uniform) a dst row off the image reads nothing
                const Cols s = vertical_pass<T, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, s);
                __builtin_amdgcn_wave_barrier();
                v = element<T, CH>(line, c, x0, step);
            }
            // quad_perm broadcasts of the quad's lanes 1, 2 and 3 (the first lane's own element is v)
            const unsigned v1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xF, 0xF, false);
            const unsigned v2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xF, 0xF, false);
            const unsigned v3 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xF, 0xF, false);
            store_outputs<T, PK>(out + (int64_t)kb * a.outStrideB, sc, fwd, kq, n, v, v1, v2, v3);
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
                const Cols s = vertical_pass<T, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, s);
                __builtin_amdgcn_wave_barrier();
                v0 = element<T, CH>(line, c0, x0, step);
                v1 = element<T, CH>(line, c1, x0, step);
                v2 = element<T, CH>(line, c2, x0, step);
                v3 = element<T, CH>(line, c3, x0, step);
            }
            store_outputs<T, PK>(out + (int64_t)kb * a.outStrideB, sc, fwd, kq, n, v0, v1, v2, v3);
        }
    }
}

// ---- the forwarding route's conversion: lane = four consecutive elements of a row (W elements: pixels x channels), one 16-byte read on
// the fp32 side and one 4- / 8-byte store on the integer side (element-aligned both: rows of any width and pitch); the last elements of
// a row one by one.  Padding is not touched.
template <typename T>
__global__ __launch_bounds__(256) void aai_int_quantize_kernel(const float *__restrict__ src, T *__restrict__ dst, ImageView dv, int W, int H)
{
    const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    if (x >= W) return;
    const float *img = src + (int64_t)blockIdx.z * ((int64_t)W * H);
    T *o = dst + (int64_t)blockIdx.z * dv.imageStride;
    for (int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); y < H; y += (int)gridDim.y * 4) {
        const float *p = img + (int64_t)y * W + x;
        T *q = o + (int64_t)y * dv.rowStride + x;
        if (x + 4 <= W) {
            const f4 v = *reinterpret_cast<const f4u *>(p);
            Pack<T>::store(q, int_quantize<T>(v.x), int_quantize<T>(v.y), int_quantize<T>(v.z), int_quantize<T>(v.w));
        } else {
            for (int i = 0; x + i < W; ++i) q[i] = int_quantize<T>(p[i]);
        }
    }
}

template <typename T>
hipError_t launch_axis_int_typed(const AxisLaunch &a, const AxisShape &shape, const T *s, ImageView sv, T *d, ImageView dv, hipStream_t stream)
{
    const dim3 grid(shape.gridX, shape.gridY, shape.gridZ), block(kWaves * 64);
    const int rows = shape.rows;
#define AAI_INT_LAUNCH(NT, CH, PK) hipLaunchKernelGGL((aai_axis_int_kernel<T, NT, CH, PK>), grid, block, 0, stream, a, a.laneTab, a.rowTab, a.strips, s, sv, d, dv, rows)
    const bool pk = a.outStrideA == 1 || a.outStrideA == -1;
    if (a.tapStep > 1) {
        // (with channels the packed form is 0 degrees, the scattered one 180 degrees)
        if (pk) { if (shape.nt) AAI_INT_LAUNCH(true, true, true); else AAI_INT_LAUNCH(false, true, true); }
        else { if (shape.nt) AAI_INT_LAUNCH(true, true, false); else AAI_INT_LAUNCH(false, true, false); }
    } else {
        if (!pk) return hipErrorInvalidValue;      // (one channel: outStrideA is +-1)
        if (shape.nt) AAI_INT_LAUNCH(true, false, true); else AAI_INT_LAUNCH(false, false, true);
    }
#undef AAI_INT_LAUNCH
    return hipGetLastError();
}

}  // namespace

// Measured (profiles/int_time.txt): with more than 64 outputs in some strip (ratios below 4, 1:1, up-sampling) the kernel is 0.54-0.83 of
// the forwarding route's time for both types and every channel count, and with 16-bit elements also at 4:1 (0.72-0.83); with 8-bit
// elements and at most 64 outputs per strip it is not faster beyond the run's spread (0.80-0.98), so that class forwards.
bool axis_int_can_serve(const AxisLaunch &a, int srcType)
{
    return !a.wide && !a.transposed && a.srcW >= VEC && a.maxOutputsPerStrip <= 256 && (a.maxOutputsPerStrip > 64 || srcType == SRC_U16);
}

hipError_t launch_axis_int(const AxisLaunch &a, int srcType, const void *src, ImageView sv, void *dst, ImageView dv, int batch, hipStream_t stream,
                           const char **kernelName)
{
    if (srcType != SRC_U8 && srcType != SRC_U16) return hipErrorInvalidValue;
    if (kernelName) *kernelName = srcType == SRC_U8 ? "aai_axis_int_kernel<u8>" : "aai_axis_int_kernel<u16>";
    if (!axis_int_can_serve(a, srcType)) return hipErrorInvalidValue;
    // K1's launch rules for a 1- / 2-byte source (axis_launch_shape): nontemporal loads unless output rows share source rows, output rows
    // per workgroup by the rows of a window and the element size.  The plan's measured shape (tuneRows) is fp32's and is not used.
    const AxisShapeFacts facts{a.nA, a.nB, a.nStrips, 0, a.maxRowSpan, a.rowsShared, a.maxOutputsPerStrip, 0, a.tapStep, a.outStrideB, 0, 0,
                               srcType == SRC_U8 ? 1 : 2, batch};
    const AxisShape shape = axis_launch_shape(facts);
    if (shape.kernel == AXIS_RUN_NOTHING) return hipSuccess;
    if (shape.kernel != AXIS_RUN_STRIP) return hipErrorInvalidValue;
    if (srcType == SRC_U8) return launch_axis_int_typed(a, shape, static_cast<const unsigned char *>(src), sv, static_cast<unsigned char *>(dst), dv, stream);
    return launch_axis_int_typed(a, shape, static_cast<const unsigned short *>(src), sv, static_cast<unsigned short *>(dst), dv, stream);
}

hipError_t launch_int_quantize(int srcType, const float *src, void *dst, ImageView dv, int W, int H, int batch, hipStream_t stream)
{
    if (W <= 0 || H <= 0 || batch <= 0) return hipSuccess;
    if (srcType != SRC_U8 && srcType != SRC_U16) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)std::min((H + 3) / 4, 65535), (unsigned)batch);
    if (srcType == SRC_U8) hipLaunchKernelGGL((aai_int_quantize_kernel<unsigned char>), grid, dim3(256), 0, stream, src, static_cast<unsigned char *>(dst), dv, W, H);
    else hipLaunchKernelGGL((aai_int_quantize_kernel<unsigned short>), grid, dim3(256), 0, stream, src, static_cast<unsigned short *>(dst), dv, W, H);
    return hipGetLastError();
}

}  // namespace aai
