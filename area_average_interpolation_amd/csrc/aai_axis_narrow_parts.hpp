// aai_axis_narrow_parts.hpp -- the pieces of the narrow-element strip kernel that more than one unit compiles: aai_axis_narrow.hip (the
// element type in, the same type out) and aai_axis_convert.hip (u8 / u16 in, scaled fp32 / fp16 / bf16 out; include/ext/aai_convert.h).
//   Pack                      VEC consecutive elements of one row, as loaded and as stored
//   Elem<E>                   the element policy: conversions in and out, the store of a strip of at most 64 outputs, the kernel's name
//   Win, load_win, lane_win   a table entry in registers
//   vertical_pass, park       the vertical sums of a lane's VEC columns, parked in the wave's LDS line
//   element                   one output element from the parked line, converted
//   Scatter, store_outputs, QuadStore, PairStore      the narrow kernel's stores
// Everything here has internal linkage: each unit compiles its own copy, with its own flags (both without contraction).
#pragma once

#include "aai_kernels.hpp"
#include "aai_int_math.hpp"

#include <algorithm>
#include <type_traits>

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
    static __device__ __forceinline__ void store(unsigned short *p, unsigned e0, unsigned e1, unsigned e2, unsigned e3)
    {
        word2 r;
        r.x = e0 | (e1 << 16); r.y = e2 | (e3 << 16);
        *reinterpret_cast<word2 *>(p) = r;
    }
};

template <typename T, bool PK> struct QuadStore;
struct PairStore;

// The element policy: storage type, element i of a pack as a float, a float as an element (in the low bits), the store of a strip of
// at most 64 outputs as a function of the kernel's form (CH, PK), the name aai_last_kernel() reports.
template <int E> struct Elem;

template <> struct Elem<NARROW_U8> {
    typedef unsigned char T;
    static constexpr const char *kName = "aai_axis_int_kernel<u8>";
    template <bool CH, bool PK> using SmallStore = QuadStore<T, PK>;
    static __device__ __forceinline__ float to_float(const Pack<T> &p, int i) { return (float)((p.w >> (8 * i)) & 255u); }     // v_cvt_f32_ubyte<i>
    static __device__ __forceinline__ unsigned from_float(float f) { return (unsigned)int_quantize<T>(f); }
};

template <> struct Elem<NARROW_U16> {
    typedef unsigned short T;
    static constexpr const char *kName = "aai_axis_int_kernel<u16>";
    template <bool CH, bool PK> using SmallStore = QuadStore<T, PK>;
    static __device__ __forceinline__ float to_float(const Pack<T> &p, int i) { return (float)(((i < 2 ? p.w0 : p.w1) >> (16 * (i & 1))) & 65535u); }
    static __device__ __forceinline__ unsigned from_float(float f) { return (unsigned)int_quantize<T>(f); }
};

// fp16: the bits of half_widen / half_narrow<HALF_F16> (aai_half_math.hpp) through v_cvt_f32_f16, which is exact, and v_cvt_f16_f32
// (round to nearest even, overflow to Inf, subnormals kept) with the header's canonical NaN
template <> struct Elem<NARROW_F16> {
    typedef unsigned short T;
    static constexpr const char *kName = "aai_axis_half_kernel<f16>";
    template <bool CH, bool PK> using SmallStore = std::conditional_t<CH, QuadStore<T, PK>, PairStore>;
    static __device__ __forceinline__ float widen(unsigned bits16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16); }
    static __device__ __forceinline__ float to_float(const Pack<T> &p, int i)
    {
        const unsigned w = i < 2 ? p.w0 : p.w1;
        return widen((i & 1) ? (w >> 16) : (w & 0xffffu));
    }
    static __device__ __forceinline__ unsigned from_float(float f)
    {
        const unsigned h = __builtin_bit_cast(unsigned short, (_Float16)f);
        return f != f ? (((__float_as_uint(f) >> 16) & 0x8000u) | 0x7e00u) : h;
    }
};

// bf16: the bits of half_widen / half_narrow<HALF_BF16>, the narrowing in the header's integer form
template <> struct Elem<NARROW_BF16> {
    typedef unsigned short T;
    static constexpr const char *kName = "aai_axis_half_kernel<bf16>";
    template <bool CH, bool PK> using SmallStore = std::conditional_t<CH, QuadStore<T, PK>, PairStore>;
    static __device__ __forceinline__ float widen(unsigned bits16) { return __uint_as_float(bits16 << 16); }
    static __device__ __forceinline__ float to_float(const Pack<T> &p, int i)
    {
        const unsigned w = i < 2 ? p.w0 : p.w1;
        return __uint_as_float((i & 1) ? (w & 0xffff0000u) : (w << 16));
    }
    static __device__ __forceinline__ unsigned from_float(float f) { return f32_to_bf16(f); }
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
template <int E, bool NT>
__device__ __forceinline__ Cols vertical_pass(const typename Elem<E>::T *__restrict__ img, int64_t rowStride, int colc, const Win e)
{
    typedef typename Elem<E>::T T;
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
        for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w0, Elem<E>::to_float(r0, i));
        if (h1) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w1, Elem<E>::to_float(r1, i));
        }
        if (h2) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w2, Elem<E>::to_float(r2, i));
        }
        if (h3) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = half_vertical_step(acc.v[i], w3, Elem<E>::to_float(r3, i));
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

// one output element from the parked line, converted: +0 (all bits 0 in every type) for an entry without weight (a dst column off the
// image), whatever the line holds.  c.s1 holds the entry's span (taps - 1), not its last element.
template <int E, bool CH>
__device__ __forceinline__ unsigned element(const float *line, const Win c, int x0, int step)
{
    if (half_entry_empty(c.wF, c.wM, c.wL)) return 0u;
    const float s = CH ? int_horizontal_stepped(line, c.s0 - x0, c.s1, step, c.wF, c.wM, c.wL) : half_horizontal(line, c.s0 - x0, c.s1, c.wF, c.wM, c.wL);
    return Elem<E>::from_float(s);
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

// The store of a strip of at most 64 outputs, one output per lane (lane = ka - k0): set up once per strip, then one call per output row
// with the lane's element; every lane of the wave calls it (the exchange is a DPP move).
//   QuadStore: the quad's first lane stores the quad's elements, n of which exist, like a lane of the other form stores its four
template <typename T, bool PK> struct QuadStore {
    int kq, n;
    bool fwd;
    Scatter sc;
    __device__ __forceinline__ QuadStore(const AxisLaunch &a, int k0, int k1, int lane, bool fwd_) : fwd(fwd_)
    {
        kq = k0 + (lane & ~3);
        n = (lane & 3) == 0 ? min(max(k1 - kq, 0), 4) : 0;
        sc = PK ? Scatter{} : make_scatter(a, kq);
    }
    __device__ __forceinline__ void store(T *row, unsigned v) const
    {
        // quad_perm broadcasts of the quad's lanes 1, 2 and 3 (the first lane's own element is v)
        const unsigned v1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xF, 0xF, false);
        const unsigned v2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xF, 0xF, false);
        const unsigned v3 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xF, 0xF, false);
        store_outputs<T, PK>(row, sc, fwd, kq, n, v, v1, v2, v3);
    }
};

//   PairStore (2-byte elements, one channel): lane pairs exchange their 16 bits and the even lane stores both (4 bytes); the pair
//   (lane, lane + 1) is adjacent in memory forwards and backwards
struct PairStore {
    typedef unsigned int word __attribute__((aligned(2)));      // two 2-byte elements, element-aligned
    int64_t o;              // the pair's first element in memory, relative to the dst row
    bool head, paired, fwd;
    __device__ __forceinline__ PairStore(const AxisLaunch &, int k0, int k1, int lane, bool fwd_) : fwd(fwd_)
    {
        head = k0 + lane < k1 && !(lane & 1);
        paired = k0 + lane + 1 < k1;
        o = fwd ? (int64_t)(k0 + lane) : -(int64_t)(k0 + lane) - (paired ? 1 : 0);
    }
    __device__ __forceinline__ void store(unsigned short *row, unsigned v) const
    {
        const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);      // quad_perm [1, 0, 3, 2]: the pair's other lane
        if (head) {
            if (paired) *reinterpret_cast<word *>(row + o) = fwd ? (v | (other << 16)) : (other | (v << 16));
            else row[o] = (unsigned short)v;
        }
    }
};

}  // namespace

}  // namespace aai
