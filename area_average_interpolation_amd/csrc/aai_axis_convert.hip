// aai_axis_convert.hip -- resample and convert (include/ext/aai_convert.h): u8 / u16 images of 1..4 interleaved channels in, a scaled
// fp32 / fp16 / bf16 image out, interleaved or planar.
//
//   aai_axis_convert_kernel<E, O>   the DIRECT route: the narrow-element strip kernel's work decomposition (aai_axis_narrow.hip, whose
//                                   pieces it shares through aai_axis_narrow_parts.hpp) over the forward plan's cached tables, for lane
//                                   axes that run along dst x (rotations by 0 and 180 degrees).  wave64, one wave per strip, four waves
//                                   per workgroup, one 4-byte (u8) or 8-byte (u16) load per lane and source row, the vertical pass in
//                                   registers with up to four rows in flight, the vertical sums parked in a per-wave LDS line, the
//                                   horizontal pass indexed by output element, no workgroup barrier.  The sum s of an output has the
//                                   bits of the integer kernel's value before its quantisation; the epilogue is ONE fma with the
//                                   channel's scale and offset and ONE rounding to the output type.  No fp32 image exists anywhere.
//   aai_convert_store_kernel<O, P>  the FORWARDING route's last stage (aai_engine.cpp: enqueue_convert): dense fp32 interleaved scratch ->
//                                   the caller's pitched image, the same fma and rounding.
//
// Which lane computes which output.  A strip holds whole pixels (build_axis_strips advances by `channels`), nOut = pixels x channels
// outputs, and the horizontal pass reads the LDS line by an arbitrary index, so the assignment is free; it changes no output's bits.
//   interleaved   virtual output q = lane-axis index ka - k0: pixel-major, the order of the dst elements at 0 degrees
//   planar        CHANNEL-MAJOR within the strip: q = c * pixels + pixel.  Consecutive q are consecutive pixels of one plane, so every
//                 plane gets coalesced, packable stores -- forwards at 0 degrees, backwards at 180 -- like a single-channel image.
//                 (A planar image of one channel IS an interleaved one and runs as such.)
// Up to 64 outputs in the strip: output q = lane; more (at most 256): outputs 4 lane .. 4 lane + 3.  Four consecutive q that exist and
// are contiguous in memory -- interleaved: at 0 degrees, and at 180 degrees with one channel; planar: within one plane -- go out as
// ONE 16-byte (fp32) or 8-byte (fp16 / bf16) element-aligned store, by the lane that holds them or by the first lane of a quad after a
// DPP exchange; everything else (180 degrees with interleaved channels, quads that cross a plane, strip tails) element by element.
// Every store covers only elements its lanes computed: nothing is read back, padding is never touched.
//
// LDS: the channel-major horizontal reads of a wave start `tapStep` elements apart for consecutive lanes of one plane, like the
// interleaved kernel's reads of one channel; the line is the narrow kernel's, 264 floats per wave.
//
// The arithmetic up to s is aai_half_math.hpp's and aai_int_math.hpp's, operation for operation; this unit is compiled without
// contraction and spells out its fmas: the CPU replay of the tests (tests/emulation/convert_emulation.cpp over narrow_replay.hpp) gives
// this kernel's bits.
#include "aai_axis_narrow_parts.hpp"

namespace aai {

namespace {

// The output policy: storage type, a float as an element (the bits, in the low half for 2-byte types), one element and four consecutive
// elements stored (element-aligned).
template <int O> struct Out;

template <> struct Out<CONVERT_F32> {
    typedef float T;
    static __device__ __forceinline__ unsigned bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ void store1(T *p, unsigned e) { *p = __uint_as_float(e); }
    static __device__ __forceinline__ void store4(T *p, unsigned e0, unsigned e1, unsigned e2, unsigned e3)
    {
        const f4 v = {__uint_as_float(e0), __uint_as_float(e1), __uint_as_float(e2), __uint_as_float(e3)};
        *reinterpret_cast<f4u *>(p) = v;
    }
};

template <> struct Out<CONVERT_F16> {
    typedef unsigned short T;
    static __device__ __forceinline__ unsigned bits(float v) { return Elem<NARROW_F16>::from_float(v); }
    static __device__ __forceinline__ void store1(T *p, unsigned e) { *p = (T)e; }
    static __device__ __forceinline__ void store4(T *p, unsigned e0, unsigned e1, unsigned e2, unsigned e3) { Pack<T>::store(p, e0, e1, e2, e3); }
};

template <> struct Out<CONVERT_BF16> {
    typedef unsigned short T;
    static __device__ __forceinline__ unsigned bits(float v) { return Elem<NARROW_BF16>::from_float(v); }
    static __device__ __forceinline__ void store1(T *p, unsigned e) { *p = (T)e; }
    static __device__ __forceinline__ void store4(T *p, unsigned e0, unsigned e1, unsigned e2, unsigned e3) { Pack<T>::store(p, e0, e1, e2, e3); }
};

// the conversion and the dst mapping of a launch (scalar registers): dst row of output row kb at rowBase + kb * rowStep; within it pixel
// x of channel c at x * chan + c (interleaved) or c * planeStride + x (planar), x = pixel or nPix - 1 - pixel (flipA: 180 degrees)
struct ConvertLaunch {
    float scale[4], offset[4];
    int chan, nPix, flipA;
    int64_t rowBase, rowStep, planeStride;
};

// v / chan for the wave-uniform chan = 1..4
__device__ __forceinline__ int div_chan(int v, int chan) { return chan == 1 ? v : (chan == 2 ? v >> 1 : (chan == 3 ? v / 3 : v >> 2)); }

__device__ __forceinline__ float pick(const float (&s)[4], int c) { return c == 0 ? s[0] : (c == 1 ? s[1] : (c == 2 ? s[2] : s[3])); }

// one output of a lane: its lane-axis index, its channel's conversion, its element offset within a dst row
template <bool PLANAR> struct Place {
    typedef std::conditional_t<PLANAR, int64_t, int> Off;
    int ka, c;
    Off o;
    float sc, of;
};

// output q (in the order above) of the strip [k0, k0 + pixels x chan); pp / c: its pixel within the strip and its channel
template <bool CH, bool PLANAR>
__device__ __forceinline__ Place<PLANAR> place(const ConvertLaunch &cl, int k0, int pp, int c)
{
    Place<PLANAR> p;
    const int pixel = (CH ? div_chan(k0, cl.chan) : k0) + pp;
    const int x = cl.flipA ? cl.nPix - 1 - pixel : pixel;
    p.ka = CH ? k0 + pp * cl.chan + c : k0 + pp;
    p.c = c;
    if (PLANAR) p.o = (typename Place<PLANAR>::Off)((int64_t)c * cl.planeStride + x);
    else p.o = (typename Place<PLANAR>::Off)(CH ? x * cl.chan + c : x);
    p.sc = pick(cl.scale, c);
    p.of = pick(cl.offset, c);
    return p;
}

// (pixel within the strip, channel) of output q, and of the one after it
template <bool CH, bool PLANAR> __device__ __forceinline__ void split(const ConvertLaunch &cl, int q, int pixels, int &pp, int &c)
{
    if (!CH) { pp = q; c = 0; }
    else if (PLANAR) { c = (int)((unsigned)q / (unsigned)pixels); pp = q - c * pixels; }
    else { pp = div_chan(q, cl.chan); c = q - pp * cl.chan; }
}
template <bool CH, bool PLANAR> __device__ __forceinline__ void advance(const ConvertLaunch &cl, int pixels, int &pp, int &c)
{
    if (!CH) ++pp;
    else if (PLANAR) { if (++pp == pixels) { pp = 0; ++c; } }
    else { if (++c == cl.chan) { c = 0; ++pp; } }
}

// the fp32 sum of one output from the parked line: +0 for an entry without weight (a dst column off the image), whatever the line
// holds.  c.s1 holds the entry's span (taps - 1), not its last element (lane_win).
template <bool CH> __device__ __forceinline__ float strip_sum(const float *line, const Win c, int x0, int step)
{
    if (half_entry_empty(c.wF, c.wM, c.wL)) return 0.f;
    return CH ? int_horizontal_stepped(line, c.s0 - x0, c.s1, step, c.wF, c.wM, c.wL) : half_horizontal(line, c.s0 - x0, c.s1, c.wF, c.wM, c.wL);
}

// E: NARROW_U8 / NARROW_U16 (the source).  O: ConvertOut.  NT: nontemporal source loads.  CH: interleaved channels in the source (taps
// tapStep apart).  PLANAR: planar output (with CH only).  PK (interleaved output): the order of q is the dst element order, forwards or
// backwards -- 0 degrees, or one channel; planar kernels are compiled with PK = true and find out per group of four.
template <int E, int O, bool NT, bool CH, bool PLANAR, bool PK>
__global__ __launch_bounds__(kWaves * 64) void aai_axis_convert_kernel(AxisLaunch a, ConvertLaunch cl, const AxisEntry *__restrict__ laneTab,
                                                                        const AxisEntry *__restrict__ rowTab, const AxisStrip *__restrict__ strips,
                                                                        const typename Elem<E>::T *__restrict__ src, ImageView sv,
                                                                        typename Out<O>::T *__restrict__ dst, ImageView dv, int rowsPerBlock)
{
    typedef typename Elem<E>::T T;
    typedef typename Out<O>::T D;
    __shared__ __attribute__((aligned(16))) float lds[kWaves][64 * VEC + 8];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = (int)blockIdx.x * kWaves + wave;
    if (strip >= a.nStrips) return;   // waves are independent: no barrier is skipped by leaving early

    typedef int i4s __attribute__((ext_vector_type(4)));
    const i4s stq = reinterpret_cast<const i4s *>(strips)[strip];
    const int k0 = stq.x, k1 = stq.y, x0 = stq.z;
    const T *img = src + (int64_t)blockIdx.z * sv.imageStride;
    D *out = dst + (int64_t)blockIdx.z * dv.imageStride + cl.rowBase;
    float *line = lds[wave];
    const int col = x0 + VEC * lane;
    const int colc = min(col, a.srcW - VEC);        // srcW >= VEC (the route's predicate)
    const int shift = col - colc;

    const int rowStart = (int)blockIdx.y * rowsPerBlock;
    const int rowEnd = min(rowStart + rowsPerBlock, a.nB);
    const int nOut = k1 - k0;
    const int pixels = CH ? div_chan(nOut, cl.chan) : nOut;      // of the strip
    const int step = CH ? a.tapStep : 1;
    const bool fwd = !cl.flipA;

    if (nOut <= 64) {
        const bool live = lane < nOut;
        int pp, c;
        split<CH, PLANAR>(cl, live ? lane : 0, pixels, pp, c);
        const Place<PLANAR> p = place<CH, PLANAR>(cl, k0, pp, c);
        const Win w = lane_win<CH>(laneTab, p.ka, step);
        // the quad (lane & ~3 .. + 3) goes out as one store of its first lane where all four outputs exist and are contiguous
        const int cFirst = __builtin_amdgcn_update_dpp(0, p.c, 0x00, 0xF, 0xF, false), cLast = __builtin_amdgcn_update_dpp(0, p.c, 0xFF, 0xF, 0xF, false);
        const bool packed = (lane | 3) < nOut && (PLANAR ? cFirst == cLast : PK);
        const bool head = (lane & 3) == 0;
        for (int kb = rowStart; kb < rowEnd; ++kb) {
            const Win e = load_win(rowTab, kb);
            float s = 0.f;
            if (!half_entry_empty(e.wF, e.wM, e.wL)) {      // (wave-uniform) a dst row off the image reads nothing
                const Cols vs = vertical_pass<E, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, vs);
                __builtin_amdgcn_wave_barrier();
                s = strip_sum<CH>(line, w, x0, step);
            }
            const unsigned v = Out<O>::bits(half_fma(s, p.sc, p.of));
            // quad_perm broadcasts of the quad's lanes 1, 2 and 3 (the first lane's own element is v)
            const unsigned v1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xF, 0xF, false);
            const unsigned v2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xF, 0xF, false);
            const unsigned v3 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xF, 0xF, false);
            D *o = out + (int64_t)kb * cl.rowStep + p.o;
            if (packed) {
                if (head) {
                    if (fwd) Out<O>::store4(o, v, v1, v2, v3);
                    else Out<O>::store4(o - 3, v3, v2, v1, v);
                }
            } else if (live) Out<O>::store1(o, v);
        }
    } else {
        const int q0 = 4 * lane;
        const int n = min(max(nOut - q0, 0), 4);                   // how many of this lane's four outputs exist
        int pp, c;
        split<CH, PLANAR>(cl, n > 0 ? q0 : 0, pixels, pp, c);
        const Place<PLANAR> p0 = place<CH, PLANAR>(cl, k0, pp, c);
        if (n > 1) advance<CH, PLANAR>(cl, pixels, pp, c);
        const Place<PLANAR> p1 = place<CH, PLANAR>(cl, k0, pp, c);
        if (n > 2) advance<CH, PLANAR>(cl, pixels, pp, c);
        const Place<PLANAR> p2 = place<CH, PLANAR>(cl, k0, pp, c);
        if (n > 3) advance<CH, PLANAR>(cl, pixels, pp, c);
        const Place<PLANAR> p3 = place<CH, PLANAR>(cl, k0, pp, c);
        const Win c0 = lane_win<CH>(laneTab, p0.ka, step), c1 = lane_win<CH>(laneTab, p1.ka, step);
        const Win c2 = lane_win<CH>(laneTab, p2.ka, step), c3 = lane_win<CH>(laneTab, p3.ka, step);
        const bool packed = n == 4 && (PLANAR ? p0.c == p3.c : PK);
        for (int kb = rowStart; kb < rowEnd; ++kb) {
            const Win e = load_win(rowTab, kb);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            if (!half_entry_empty(e.wF, e.wM, e.wL)) {
                const Cols vs = vertical_pass<E, NT>(img, sv.rowStride, colc, e);
                __builtin_amdgcn_wave_barrier();
                park(line, lane, shift, vs);
                __builtin_amdgcn_wave_barrier();
                s0 = strip_sum<CH>(line, c0, x0, step);
                s1 = strip_sum<CH>(line, c1, x0, step);
                s2 = strip_sum<CH>(line, c2, x0, step);
                s3 = strip_sum<CH>(line, c3, x0, step);
            }
            const unsigned v0 = Out<O>::bits(half_fma(s0, p0.sc, p0.of)), v1 = Out<O>::bits(half_fma(s1, p1.sc, p1.of));
            const unsigned v2 = Out<O>::bits(half_fma(s2, p2.sc, p2.of)), v3 = Out<O>::bits(half_fma(s3, p3.sc, p3.of));
            D *row = out + (int64_t)kb * cl.rowStep;
            if (packed) {
                if (fwd) Out<O>::store4(row + p0.o, v0, v1, v2, v3);
                else Out<O>::store4(row + p3.o, v3, v2, v1, v0);
            } else {
                if (n > 0) Out<O>::store1(row + p0.o, v0);
                if (n > 1) Out<O>::store1(row + p1.o, v1);
                if (n > 2) Out<O>::store1(row + p2.o, v2);
                if (n > 3) Out<O>::store1(row + p3.o, v3);
            }
        }
    }
}

// ---- the forwarding route's last stage: dense fp32 interleaved scratch -> the caller's pitched image.  Interleaved output: a lane takes
// four consecutive ELEMENTS of a row (one 16-byte load, one 16- / 8-byte store, element-aligned both), the last elements of a row one
// by one.  Planar output (2..4 channels): a lane takes four consecutive PIXELS, and per plane their four elements, `chan` apart in the
// scratch (the lane reads its 4 x chan contiguous floats over the planes), as one store; the last pixels of a row one by one.  Padding is not touched.
struct ConvertStore {
    float scale[4], offset[4];
    int chan;
    int64_t planeStride;
};

template <int O, bool PLANAR>
__global__ __launch_bounds__(256) void aai_convert_store_kernel(const float *__restrict__ src, typename Out<O>::T *__restrict__ dst, ImageView dv, ConvertStore cs,
                                                                 int W, int H)
{
    typedef typename Out<O>::T D;
    // W: elements of a row (interleaved) or pixels of a row (planar)
    const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
    if (x >= W) return;
    const int64_t rowElems = PLANAR ? (int64_t)W * cs.chan : (int64_t)W;
    const float *img = src + (int64_t)blockIdx.z * (rowElems * H);
    D *o = dst + (int64_t)blockIdx.z * dv.imageStride;
    for (int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); y < H; y += (int)gridDim.y * 4) {
        D *q = o + (int64_t)y * dv.rowStride + x;
        if (PLANAR) {
            const float *p = img + (int64_t)y * rowElems + (int64_t)x * cs.chan;
            for (int c = 0; c < cs.chan; ++c) {
                const float sc = pick(cs.scale, c), of = pick(cs.offset, c);
                D *qc = q + (int64_t)c * cs.planeStride;
                if (x + 4 <= W)
                    Out<O>::store4(qc, Out<O>::bits(half_fma(p[c], sc, of)), Out<O>::bits(half_fma(p[cs.chan + c], sc, of)),
                                   Out<O>::bits(half_fma(p[2 * cs.chan + c], sc, of)), Out<O>::bits(half_fma(p[3 * cs.chan + c], sc, of)));
                else
                    for (int i = 0; x + i < W; ++i) Out<O>::store1(qc + i, Out<O>::bits(half_fma(p[i * cs.chan + c], sc, of)));
            }
        } else {
            const float *p = img + (int64_t)y * rowElems + x;
            int c = x - div_chan(x, cs.chan) * cs.chan;      // channel of element x
            if (x + 4 <= W) {
                const f4 v = *reinterpret_cast<const f4u *>(p);
                const int ca = c;
                const int cb = ca + 1 == cs.chan ? 0 : ca + 1, cc = cb + 1 == cs.chan ? 0 : cb + 1, cd = cc + 1 == cs.chan ? 0 : cc + 1;
                Out<O>::store4(q, Out<O>::bits(half_fma(v.x, pick(cs.scale, ca), pick(cs.offset, ca))), Out<O>::bits(half_fma(v.y, pick(cs.scale, cb), pick(cs.offset, cb))),
                               Out<O>::bits(half_fma(v.z, pick(cs.scale, cc), pick(cs.offset, cc))), Out<O>::bits(half_fma(v.w, pick(cs.scale, cd), pick(cs.offset, cd))));
            } else {
                for (int i = 0; x + i < W; ++i) {
                    Out<O>::store1(q + i, Out<O>::bits(half_fma(p[i], pick(cs.scale, c), pick(cs.offset, c))));
                    c = c + 1 == cs.chan ? 0 : c + 1;
                }
            }
        }
    }
}

template <int E, int O>
hipError_t launch_convert_typed(const AxisLaunch &a, const ConvertLaunch &cl, bool planar, const AxisShape &shape, const void *src, ImageView sv, void *dst,
                                ImageView dv, hipStream_t stream)
{
    typedef typename Elem<E>::T T;
    typedef typename Out<O>::T D;
    const T *s = static_cast<const T *>(src);
    D *d = static_cast<D *>(dst);
    const dim3 grid(shape.gridX, shape.gridY, shape.gridZ), block(kWaves * 64);
    const int rows = shape.rows;
#define AAI_CONVERT_LAUNCH(NT, CH, PLANAR, PK) \
    hipLaunchKernelGGL((aai_axis_convert_kernel<E, O, NT, CH, PLANAR, PK>), grid, block, 0, stream, a, cl, a.laneTab, a.rowTab, a.strips, s, sv, d, dv, rows)
    if (cl.chan > 1) {
        if (planar) { if (shape.nt) AAI_CONVERT_LAUNCH(true, true, true, true); else AAI_CONVERT_LAUNCH(false, true, true, true); }
        // (interleaved channels: the packed form is 0 degrees, the element-by-element one 180 degrees)
        else if (!cl.flipA) { if (shape.nt) AAI_CONVERT_LAUNCH(true, true, false, true); else AAI_CONVERT_LAUNCH(false, true, false, true); }
        else { if (shape.nt) AAI_CONVERT_LAUNCH(true, true, false, false); else AAI_CONVERT_LAUNCH(false, true, false, false); }
        return hipGetLastError();
    }
    if (shape.nt) AAI_CONVERT_LAUNCH(true, false, false, true); else AAI_CONVERT_LAUNCH(false, false, false, true);
#undef AAI_CONVERT_LAUNCH
    return hipGetLastError();
}

// convert_grid's rules (aai_axis_narrow.hip): 256 row elements per block of four rows, grid.y capped (the kernel strides over the rest), the
// batch in grid.z (chunks of at most kMaxGridZ: aai_engine.cpp)
dim3 convert_store_grid(int W, int H, int batch)
{
    return dim3((unsigned)((W + 255) / 256), (unsigned)std::min((H + 3) / 4, 65535), (unsigned)batch);
}

template <int O>
hipError_t launch_store_typed(const ConvertStore &cs, bool planar, const float *src, void *dst, ImageView dv, int W, int H, int batch, hipStream_t stream)
{
    typedef typename Out<O>::T D;
    D *d = static_cast<D *>(dst);
    if (planar) hipLaunchKernelGGL((aai_convert_store_kernel<O, true>), convert_store_grid(W, H, batch), dim3(256), 0, stream, src, d, dv, cs, W, H);
    else hipLaunchKernelGGL((aai_convert_store_kernel<O, false>), convert_store_grid(W * cs.chan, H, batch), dim3(256), 0, stream, src, d, dv, cs, W * cs.chan, H);
    return hipGetLastError();
}

const char *const kConvertNames[2][3] = {{"aai_axis_convert_kernel<u8,f32>", "aai_axis_convert_kernel<u8,f16>", "aai_axis_convert_kernel<u8,bf16>"},
                                         {"aai_axis_convert_kernel<u16,f32>", "aai_axis_convert_kernel<u16,f16>", "aai_axis_convert_kernel<u16,bf16>"}};

// The classes that forward although the strip form applies: [source u8, u16][output f32, f16, bf16][layout interleaved, planar], one bit
// per (outputs per strip, rotation): 1 = more than 64 at 0 degrees, 2 = more than 64 at 180, 4 = at most 64 at 0, 8 = at most 64 at 180.
// Measured (profiles/convert_time.txt: 4096^2 -> 4096^2, 2048^2 and 1024^2 at 0 and 180 degrees, 1, 3 and 4 channels, two runs): the
// project's standing rule keeps a class only where the kernel is faster than the forwarding route's stages beyond the recorded spread in
// EVERY row of BOTH runs.  By the medians the kernel is faster in every row, 0.25-0.97 of the forwarding route's time: 0.25-0.95 with
// 16-bit sources or more than 64 outputs per strip, and 0.59-0.97 with 8-bit sources at at most 64 outputs per strip, the class that
// aai_int.h forwards too.  The classes below missed the rule in one of the two runs, most of them
// through the spread of the baseline's bilinear legs in a single-channel row, not through their medians.
constexpr unsigned char kConvertForwards[2][3][2] = {{{1 | 2 | 8, 4 | 8}, {2 | 4 | 8, 4 | 8}, {4 | 8, 8}}, {{2, 0}, {1, 0}, {1, 0}}};

}  // namespace

bool axis_convert_can_serve(const AxisLaunch &a, int srcType, int outType, int planar)
{
    if ((srcType != NARROW_U8 && srcType != NARROW_U16) || !convert_out_known(outType)) return false;
    if (a.wide || a.transposed || a.srcW < VEC || a.maxOutputsPerStrip > 256) return false;
    const int layout = planar && a.tapStep > 1 ? 1 : 0;      // (a planar image of one channel is an interleaved one)
    const unsigned bit = (a.maxOutputsPerStrip <= 64 ? 4u : 1u) << (a.outStrideA < 0 ? 1 : 0);
    return !(kConvertForwards[srcType == NARROW_U8 ? 0 : 1][outType][layout] & bit);
}

hipError_t launch_axis_convert(const AxisLaunch &a, int srcType, const ConvertParams &cv, const void *src, ImageView sv, void *dst, ImageView dv, int batch,
                               hipStream_t stream, const char **kernelName)
{
    if ((srcType != NARROW_U8 && srcType != NARROW_U16) || !convert_out_known(cv.outType)) return hipErrorInvalidValue;
    if (kernelName) *kernelName = kConvertNames[srcType == NARROW_U8 ? 0 : 1][cv.outType];
    if (!axis_convert_can_serve(a, srcType, cv.outType, cv.planar)) return hipErrorInvalidValue;
    // the narrow kernel's launch rules (launch_axis_narrow): K1's for a 1- / 2-byte source
    const AxisShapeFacts facts{a.nA, a.nB, a.nStrips, 0, a.maxRowSpan, a.rowsShared, a.maxOutputsPerStrip, 0, a.tapStep, a.outStrideB, 0, 0,
                               (int)narrow_elem_size(srcType), batch};
    const AxisShape shape = axis_launch_shape(facts);
    if (shape.kernel == AXIS_RUN_NOTHING) return hipSuccess;
    if (shape.kernel != AXIS_RUN_STRIP) return hipErrorInvalidValue;
    ConvertLaunch cl{};
    for (int i = 0; i < 4; ++i) { cl.scale[i] = cv.scale[i]; cl.offset[i] = cv.offset[i]; }
    cl.chan = a.tapStep > 1 ? a.tapStep : 1;
    cl.nPix = a.nA / cl.chan;
    // (not transposed: the lane axis is dst x, the row axis dst y; a negative stride of make_axis_launch's map is a flip)
    cl.flipA = a.outStrideA < 0 ? 1 : 0;
    const bool flipB = a.outStrideB < 0;
    cl.rowStep = flipB ? -dv.rowStride : dv.rowStride;
    cl.rowBase = flipB ? (int64_t)(a.nB - 1) * dv.rowStride : 0;
    const bool planar = cv.planar && cl.chan > 1;      // (a planar image of one channel is an interleaved one)
    cl.planeStride = planar ? cv.planeStride : 0;
#define AAI_CONVERT_OUT(E) \
    (cv.outType == CONVERT_F32 ? launch_convert_typed<E, CONVERT_F32>(a, cl, planar, shape, src, sv, dst, dv, stream) \
     : cv.outType == CONVERT_F16 ? launch_convert_typed<E, CONVERT_F16>(a, cl, planar, shape, src, sv, dst, dv, stream) \
                                 : launch_convert_typed<E, CONVERT_BF16>(a, cl, planar, shape, src, sv, dst, dv, stream))
    return srcType == NARROW_U8 ? AAI_CONVERT_OUT(NARROW_U8) : AAI_CONVERT_OUT(NARROW_U16);
#undef AAI_CONVERT_OUT
}

hipError_t launch_convert_store(const ConvertParams &cv, int channels, const float *src, void *dst, ImageView dv, int W, int H, int batch, hipStream_t stream)
{
    if (W <= 0 || H <= 0 || batch <= 0) return hipSuccess;
    if (!convert_out_known(cv.outType) || channels < 1 || channels > 4) return hipErrorInvalidValue;
    ConvertStore cs{};
    for (int i = 0; i < 4; ++i) { cs.scale[i] = cv.scale[i]; cs.offset[i] = cv.offset[i]; }
    cs.chan = channels;
    const bool planar = cv.planar && channels > 1;
    cs.planeStride = planar ? cv.planeStride : 0;
    switch (cv.outType) {
    case CONVERT_F32: return launch_store_typed<CONVERT_F32>(cs, planar, src, dst, dv, W, H, batch, stream);
    case CONVERT_F16: return launch_store_typed<CONVERT_F16>(cs, planar, src, dst, dv, W, H, batch, stream);
    default: return launch_store_typed<CONVERT_BF16>(cs, planar, src, dst, dv, W, H, batch, stream);
    }
}

}  // namespace aai
