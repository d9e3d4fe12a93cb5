// aai_half.hip -- the half-precision path (include/aai_half.h): fp16 / bf16 images in, the same element type out.
//
//   aai_axis_half_kernel<T>   the DIRECT route: K1's streaming form (aai_axis.hip) over the forward plan's cached tables -- strips, lane and
//                             row entries, the (ka, kb) -> dst element map -- for lane axes that run along dst x (rotations by 0 and 180
//                             degrees).  It computes no geometry.  A 2-byte element halves the source bytes of a kernel that is bound by
//                             the source read, and the output goes out in the element type: no fp32 image exists anywhere.
//   aai_half_widen_kernel<T>  } the FORWARDING route of every other request (aai_engine.cpp: enqueue_half): pitched half image -> dense
//   aai_half_narrow_kernel<T> } fp32 scratch, the fp32 entry's own launches, dense fp32 scratch -> pitched half image.
//
// Work decomposition of the direct kernel = K1's, because the plan's strips are built for it: wave64, one wave per strip of 256 source
// columns, four waves (adjacent strips) per workgroup, four columns per lane = ONE 8-byte load per lane and source row, the vertical pass
// in registers with up to four source rows in flight, the row of vertical sums parked in a per-wave LDS line and re-indexed by OUTPUT
// pixel for the horizontal pass.  Waves never synchronise with each other: no s_barrier.
// Two forms of the horizontal pass, chosen per strip (wave-uniform) like K1's branches C and D:
//   * up to 64 outputs in the strip (ratios of 4 and more): one output per lane; lane pairs exchange their 16 bits through DPP and the
//     even lane stores both (4 bytes);
//   * 65 .. 256 outputs (ratios below 4, 1:1, up-sampling -- a strip never holds more than 256, build_axis_strips): four consecutive
//     outputs per lane, one 8-byte store per lane and output row.
// With dst x running against the lanes (180 degrees) the same elements are stored from the other end.
//
// The arithmetic of an element is aai_half_math.hpp's, operation for operation, and this unit is compiled without contraction: the CPU
// replay of the tests (tests/emulation/half_emulation.cpp) gives this kernel's bits.
//
// Memory: loads start no later than column srcW - 4 (park()'s shift rule of K1) and cover source rows of the window only; stores cover
// output elements only; nothing assumes more than 2-byte alignment of a base pointer or a stride.
#include "aai_kernels.hpp"
#include "aai_half_math.hpp"

#include <algorithm>

namespace aai {

namespace {

constexpr int kWaves = kAxisWaves;
constexpr int VEC = 4;         // source columns per lane and load

typedef unsigned int u2h __attribute__((ext_vector_type(2), aligned(2)));      // four 2-byte elements, element-aligned
typedef unsigned int u1h __attribute__((aligned(2)));                          // two 2-byte elements, element-aligned
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));             // dword-aligned 16-byte access
typedef float f4 __attribute__((ext_vector_type(4)));

// widening on the device: the bits of half_widen<HT> (aai_half_math.hpp).  fp16 through v_cvt_f32_f16, which is exact.
template <int HT> __device__ __forceinline__ float widen_dev(unsigned bits16)
{
    if (HT == HALF_BF16) return __uint_as_float(bits16 << 16);
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
}
// ... and narrowing, the bits of half_narrow<HT>: fp16 through v_cvt_f16_f32 (round to nearest even, overflow to Inf, subnormals kept),
// with the header's canonical NaN; bf16 in the header's integer form
template <int HT> __device__ __forceinline__ unsigned narrow_dev(float f)
{
    if (HT == HALF_BF16) return f32_to_bf16(f);
    const unsigned h = __builtin_bit_cast(unsigned short, (_Float16)f);
    return f != f ? (((__float_as_uint(f) >> 16) & 0x8000u) | 0x7e00u) : h;
}

// VEC consecutive source columns of one row, as loaded
struct RawH {
    unsigned w0, w1;
    template <bool NT> __device__ __forceinline__ void load(const uint16_t *p)
    {
        const u2h *v = reinterpret_cast<const u2h *>(p);
        const u2h x = NT ? __builtin_nontemporal_load(v) : *v;
        w0 = x.x; w1 = x.y;
    }
    template <int HT> __device__ __forceinline__ float get(int i) const
    {
        const unsigned w = i < 2 ? w0 : w1;
        if (HT == HALF_BF16) return __uint_as_float((i & 1) ? (w & 0xffff0000u) : (w << 16));
        return widen_dev<HT>((i & 1) ? (w >> 16) : (w & 0xffffu));
    }
};

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
template <int HT, bool NT>
__device__ __forceinline__ Cols vertical_pass(const uint16_t *__restrict__ img, int64_t rowStride, int colc, const Win e)
{
    Cols acc;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc.v[i] = 0.f;
    for (int y = e.s0; y <= e.s1; y += 4) {
        RawH r0, r1, r2, r3;
        const uint16_t *p = img + (int64_t)y * rowStride + colc;
        const bool h1 = y + 1 <= e.s1, h2 = y + 2 <= e.s1, h3 = y + 3 <= e.s1;
        r0.template load<NT>(p);
        r1 = r0; r2 = r0; r3 = r0;
        if (h1) r1.template load<NT>(p + rowStride);
        if (h2) r2.template load<NT>(p + 2 * rowStride);
        if (h3) r3.template load<NT>(p + 3 * rowStride);
        const float w0 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y), w1 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y + 1);
        const float w2 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y + 2), w3 = half_row_weight(e.s0, e.s1, e.wF, e.wM, e.wL, y + 3);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w0, r0.template get<HT>(i));
        if (h1) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w1, r1.template get<HT>(i));
        }
        if (h2) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w2, r2.template get<HT>(i));
        }
        if (h3) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w3, r3.template get<HT>(i));
        }
    }
    return acc;
}

// K1's park(): the lane's VEC vertical sums into the wave's LDS line (position = column - strip origin).  Near the right image edge a
// lane loaded the last in-range vector instead of its own (colc = min(col, W - VEC), shift = col - colc) and writes only the columns
// at or right of its own first one.
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

// one output element from the parked line: +0 for an entry without weight (a dst column off the image), whatever the line holds
__device__ __forceinline__ float horizontal(const float *line, const Win c, int x0)
{
    if (half_entry_empty(c.wF, c.wM, c.wL)) return 0.f;
    return half_horizontal(line, c.s0 - x0, c.s1 - c.s0, c.wF, c.wM, c.wL);
}

template <int HT, bool NT>
__global__ __launch_bounds__(kWaves * 64) void aai_axis_half_kernel(AxisLaunch a, const AxisEntry *__restrict__ laneTab,
                                                                     const AxisEntry *__restrict__ rowTab, const AxisStrip *__restrict__ strips,
                                                                     const uint16_t *__restrict__ src, ImageView sv,
                                                                     uint16_t *__restrict__ dst, ImageView dv, int rowsPerBlock)
{
    __shared__ __attribute__((aligned(16))) float lds[kWaves][64 * VEC + 8];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = (int)blockIdx.x * kWaves + wave;
    if (strip >= a.nStrips) return;   // waves are independent: no barrier is skipped by leaving early

    typedef int i4s __attribute__((ext_vector_type(4)));
    const i4s stq = reinterpret_cast<const i4s *>(strips)[strip];
    const int k0 = stq.x, k1 = stq.y, x0 = stq.z;
    const uint16_t *img = src + (int64_t)blockIdx.z * sv.imageStride;
    uint16_t *out = dst + (int64_t)blockIdx.z * dv.imageStride + a.outBase;
    float *line = lds[wave];
    const int col = x0 + VEC * lane;
    const int colc = min(col, a.srcW - VEC);        // srcW >= VEC (the route's predicate)
    const int shift = col - colc;

    const int rowStart = (int)blockIdx.y * rowsPerBlock;
    const int rowEnd = min(rowStart + rowsPerBlock, a.nB);
    const int nOut = k1 - k0;
    const bool fwd = a.outStrideA == 1;              // else -1: dst x runs against the lanes

    if (nOut <= 64) {
        const bool live = lane < nOut;
        const Win c = load_win(laneTab, live ? k0 + lane : k0);
        const bool pairHead = live && !(lane & 1), paired = lane + 1 < nOut;
        // element of this lane: out[(k0 + lane) * (+-1)]; the pair (lane, lane + 1) is adjacent in memory either way
        uint16_t *o = out + (fwd ? (int64_t)(k0 + lane) : -(int64_t)(k0 + lane) - (paired ? 1 : 0));
        for (int kb = rowStart; kb < rowEnd; ++kb) {
            const Win e = load_win(rowTab, kb);
            unsigned bits = 0u;      // +0 in both types
            if (!half_entry_empty(e.wF, e.wM, e.wL)) {      // (wave-uniform) a dst row off the image reads nothing
                const Cols v = vertical_pass<HT, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, v);
                __builtin_amdgcn_wave_barrier();
                bits = narrow_dev<HT>(horizontal(line, c, x0));
            }
            const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)bits, 0xB1, 0xF, 0xF, false);      // quad_perm [1, 0, 3, 2]: the pair's other lane
            if (pairHead) {
                uint16_t *p = o + (int64_t)kb * a.outStrideB;
                if (paired) *reinterpret_cast<u1h *>(p) = fwd ? (bits | (other << 16)) : (other | (bits << 16));
                else *p = (uint16_t)bits;
            }
        }
    } else {
        const int kq = k0 + 4 * lane;
        const int nq = min(max(k1 - kq, 0), 4);                   // how many of this lane's four outputs exist
        const Win c0 = load_win(laneTab, nq > 0 ? kq : k0), c1 = load_win(laneTab, nq > 1 ? kq + 1 : k0);
        const Win c2 = load_win(laneTab, nq > 2 ? kq + 2 : k0), c3 = load_win(laneTab, nq > 3 ? kq + 3 : k0);
        for (int kb = rowStart; kb < rowEnd; ++kb) {
            const Win e = load_win(rowTab, kb);
            unsigned b0 = 0u, b1 = 0u, b2 = 0u, b3 = 0u;
            if (!half_entry_empty(e.wF, e.wM, e.wL)) {
                const Cols v = vertical_pass<HT, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, v);
                __builtin_amdgcn_wave_barrier();
                b0 = narrow_dev<HT>(horizontal(line, c0, x0));
                b1 = narrow_dev<HT>(horizontal(line, c1, x0));
                b2 = narrow_dev<HT>(horizontal(line, c2, x0));
                b3 = narrow_dev<HT>(horizontal(line, c3, x0));
            }
            uint16_t *o = out + (fwd ? (int64_t)kq : -(int64_t)kq) + (int64_t)kb * a.outStrideB;      // this lane's first output
            if (nq == 4) {
                u2h r;
                if (fwd) { r.x = b0 | (b1 << 16); r.y = b2 | (b3 << 16); *reinterpret_cast<u2h *>(o) = r; }
                else { r.x = b3 | (b2 << 16); r.y = b1 | (b0 << 16); *reinterpret_cast<u2h *>(o - 3) = r; }
            } else {
                const int64_t sA = fwd ? 1 : -1;
                if (nq > 0) o[0] = (uint16_t)b0;
                if (nq > 1) o[sA] = (uint16_t)b1;
                if (nq > 2) o[2 * sA] = (uint16_t)b2;
            }
        }
    }
}

// ---- the forwarding route's conversions: lane = four consecutive elements of a row, one 8-byte access on the half side and one 16-byte
// access on the fp32 side (element-aligned both: rows of any width and pitch); the last elements of a row one by one.  Padding is not touched.
template <int HT>
__global__ __launch_bounds__(256) void aai_half_widen_kernel(const uint16_t *__restrict__ src, ImageView sv, float *__restrict__ dst, int W, int H)
{
    const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    if (x >= W) return;
    const uint16_t *img = src + (int64_t)blockIdx.z * sv.imageStride;
    float *o = dst + (int64_t)blockIdx.z * ((int64_t)W * H);
    for (int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); y < H; y += (int)gridDim.y * 4) {
        const uint16_t *p = img + (int64_t)y * sv.rowStride + x;
        float *q = o + (int64_t)y * W + x;
        if (x + 4 <= W) {
            RawH r;
            r.template load<false>(p);
            const f4 v = {r.template get<HT>(0), r.template get<HT>(1), r.template get<HT>(2), r.template get<HT>(3)};
            *reinterpret_cast<f4u *>(q) = v;
        } else {
            for (int i = 0; x + i < W; ++i) q[i] = widen_dev<HT>(p[i]);
        }
    }
}

template <int HT>
__global__ __launch_bounds__(256) void aai_half_narrow_kernel(const float *__restrict__ src, uint16_t *__restrict__ dst, ImageView dv, int W, int H)
{
    const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    if (x >= W) return;
    const float *img = src + (int64_t)blockIdx.z * ((int64_t)W * H);
    uint16_t *o = dst + (int64_t)blockIdx.z * dv.imageStride;
    for (int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); y < H; y += (int)gridDim.y * 4) {
        const float *p = img + (int64_t)y * W + x;
        uint16_t *q = o + (int64_t)y * dv.rowStride + x;
        if (x + 4 <= W) {
            const f4 v = *reinterpret_cast<const f4u *>(p);
            u2h r;
            r.x = narrow_dev<HT>(v.x) | (narrow_dev<HT>(v.y) << 16);
            r.y = narrow_dev<HT>(v.z) | (narrow_dev<HT>(v.w) << 16);
            *reinterpret_cast<u2h *>(q) = r;
        } else {
            for (int i = 0; x + i < W; ++i) q[i] = (uint16_t)narrow_dev<HT>(p[i]);
        }
    }
}

dim3 convert_grid(int W, int H, int batch)
{
    return dim3((unsigned)((W + 255) / 256), (unsigned)std::min((H + 3) / 4, 65535), (unsigned)batch);
}

}  // namespace

bool axis_half_can_serve(const AxisLaunch &a)
{
    return !a.wide && !a.transposed && a.tapStep <= 1 && a.srcW >= VEC && (a.outStrideA == 1 || a.outStrideA == -1) && a.maxOutputsPerStrip <= 256;
}

hipError_t launch_axis_half(const AxisLaunch &a, int halfType, const void *src, ImageView sv, void *dst, ImageView dv, int batch, hipStream_t stream,
                            const char **kernelName)
{
    if (kernelName) *kernelName = halfType == HALF_F16 ? "aai_axis_half_kernel<f16>" : "aai_axis_half_kernel<bf16>";
    if (!axis_half_can_serve(a)) return hipErrorInvalidValue;
    // K1's launch rules for a 2-byte source (axis_launch_shape): nontemporal loads unless output rows share source rows, output rows per
    // workgroup by the rows of a window.  The plan's measured shape (tuneRows) is fp32's and is not used.
    const AxisShapeFacts facts{a.nA, a.nB, a.nStrips, 0, a.maxRowSpan, a.rowsShared, a.maxOutputsPerStrip, 0, 1, a.outStrideB, 0, 0, 2, batch};
    const AxisShape shape = axis_launch_shape(facts);
    if (shape.kernel == AXIS_RUN_NOTHING) return hipSuccess;
    if (shape.kernel != AXIS_RUN_STRIP) return hipErrorInvalidValue;
    const dim3 grid(shape.gridX, shape.gridY, shape.gridZ), block(kWaves * 64);
    const uint16_t *s = static_cast<const uint16_t *>(src);
    uint16_t *d = static_cast<uint16_t *>(dst);
    const int rows = shape.rows;
    if (halfType == HALF_F16) {
        if (shape.nt) hipLaunchKernelGGL((aai_axis_half_kernel<HALF_F16, true>), grid, block, 0, stream, a, a.laneTab, a.rowTab, a.strips, s, sv, d, dv, rows);
        else hipLaunchKernelGGL((aai_axis_half_kernel<HALF_F16, false>), grid, block, 0, stream, a, a.laneTab, a.rowTab, a.strips, s, sv, d, dv, rows);
    } else {
        if (shape.nt) hipLaunchKernelGGL((aai_axis_half_kernel<HALF_BF16, true>), grid, block, 0, stream, a, a.laneTab, a.rowTab, a.strips, s, sv, d, dv, rows);
        else hipLaunchKernelGGL((aai_axis_half_kernel<HALF_BF16, false>), grid, block, 0, stream, a, a.laneTab, a.rowTab, a.strips, s, sv, d, dv, rows);
    }
    return hipGetLastError();
}

hipError_t launch_half_widen(int halfType, const void *src, ImageView sv, float *dst, int W, int H, int batch, hipStream_t stream)
{
    if (W <= 0 || H <= 0 || batch <= 0) return hipSuccess;
    const uint16_t *s = static_cast<const uint16_t *>(src);
    if (halfType == HALF_F16) hipLaunchKernelGGL((aai_half_widen_kernel<HALF_F16>), convert_grid(W, H, batch), dim3(256), 0, stream, s, sv, dst, W, H);
    else hipLaunchKernelGGL((aai_half_widen_kernel<HALF_BF16>), convert_grid(W, H, batch), dim3(256), 0, stream, s, sv, dst, W, H);
    return hipGetLastError();
}

hipError_t launch_half_narrow(int halfType, const float *src, void *dst, ImageView dv, int W, int H, int batch, hipStream_t stream)
{
    if (W <= 0 || H <= 0 || batch <= 0) return hipSuccess;
    uint16_t *d = static_cast<uint16_t *>(dst);
    if (halfType == HALF_F16) hipLaunchKernelGGL((aai_half_narrow_kernel<HALF_F16>), convert_grid(W, H, batch), dim3(256), 0, stream, src, d, dv, W, H);
    else hipLaunchKernelGGL((aai_half_narrow_kernel<HALF_BF16>), convert_grid(W, H, batch), dim3(256), 0, stream, src, d, dv, W, H);
    return hipGetLastError();
}

}  // namespace aai
