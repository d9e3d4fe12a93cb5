// aai_rot_serve.hpp -- which fp32 family of the rotated lattice can serve a launch, as a function of the SOURCE VIEW: the predicates
// rot_family (aai_rotated.hip) and rot_form (aai_engine.cpp) ask, and the per-wave address regimes the launchers derive from the same
// view (anchor rows, rebased waves).  Host code without a HIP type in it: the launchers and the variant probe of the test-suite
// (tests/emulation, compiled by the host compiler alone) include this one header, so each rule is stated once.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "aai_rot_cell.hpp"

namespace aai {

// Image addressing shared by every kernel: element (x,y) of image b is base[b*imageStride + y*rowStride + x].
// Source element types (AAI_DTYPE_* in include/aai.h).  Outputs are always fp32.
enum SrcType { SRC_F32 = 0, SRC_U8 = 1, SRC_U16 = 2 };

struct ImageView {
    int64_t rowStride;
    int64_t imageStride;
};

// Small facts the launchers and their *_can_* predicates share, each stated once (host code; no kernel calls these).
// bytes per element of a source type
constexpr size_t src_elem_size(int srcType) { return srcType == SRC_U8 ? 1 : srcType == SRC_U16 ? 2 : 4; }
// (slot_words -- LDS words per window slot of interleaved channels -- lives in aai_rot_quad.hpp, where the CPU replay can ask it too)

// the source image spans 4 GiB and more: unsigned 32-bit byte offsets from its first element no longer reach every pixel
inline bool spans_4gib(const RotLaunch &r, int srcType, ImageView sv)
{
    return (int64_t)r.H * sv.rowStride * (int64_t)src_elem_size(srcType) >= ((int64_t)1 << 32);
}

// ---- the quad and wide formulations (aai_rotated_quad.hip, aai_rotated_wide.hip) ---------------------------------------------------
// the widest window of source pixels a dst pixel's footprint can touch, per axis
inline int quad_window(const RotLaunch &r) { return (int)floor(2.0 * (r.h * (r.c + r.s) - 0.5 + 1e-5)) + 3; }

// How many source rows apart two lanes of one wave (a 16 x 4 dst tile) can read: their centres differ by at most
// 15.6 dst pixel sides, each reaches half a window further, plus slack for rounding and clamping.
inline int quad_anchor_rows(const RotLaunch &r)
{
    return (int)ceil(15.6 * 2.0 * r.h / r.scale) + quad_window(r) + 4;
}

inline bool quad_can_address(const RotLaunch &r, int srcType, ImageView sv)
{
    // lanes address their pixels with unsigned 32-bit byte offsets from the image's first element -- or, for plain images
    // of 4 GiB and more, from an anchor row of their wave (quad_anchor_rows)
    const int win = quad_window(r);
    if (spans_4gib(r, srcType, sv)) {
        if (r.chan > 1) return false;
        if ((int64_t)(2 * quad_anchor_rows(r) + win + 2) * sv.rowStride * (int64_t)src_elem_size(srcType) >= ((int64_t)1 << 32)) return false;
    }
    if (r.chan > 1) {
        // interleaved channels: the staged window (win^2 slots of `words` LDS words per lane) must leave room for two
        // workgroups per CU
        if (!quad_multi_fits_lds(win, slot_words(src_elem_size(srcType), r.chan))) return false;
    }
    return true;
}

// wide footprints: the quad formulation over a window split into parts, one lane per part.  r.chan set; RotLaunch::wide, plain images
inline bool wide_can_serve(const RotLaunch &r, int srcType, ImageView sv)
{
    if (!r.wide || (r.mode != AAI_MODE_AREA && r.mode != AAI_MODE_FAST) || r.chan != 1 || r.scale != 1 || (r.dyBase & 15) != 0) return false;
    // (tilesX * 16 blocks along grid.x)
    if ((int64_t)((r.dW + 15) / 16) * 16 > 2147483647ll) return false;
    return quad_can_address(r, srcType, sv);
}

// ---- the cell formulation (aai_rotated_cell.hip).  r.chan set; area mode --------------------------------------------------------------
inline bool cell_can_serve(const RotLaunch &r, int srcType, ImageView sv)
{
    // plain images below 4 GiB (lanes address their pixels with unsigned 32-bit byte offsets from the image's first element)
    if (!r.cell || r.mode != AAI_MODE_AREA) return false;
    // Small outputs stay on the quad kernel: a cell wave lives for rows + 1 cell rows, and an image of fewer than ~1000 such
    // waves (about 720 x 720 dst pixels) cannot fill the chip with them -- the reference's own example call (158 x 158 dst
    // pixels at 5.9 : 1) takes 71 us on 60 cell waves and 36 us on 390 one-shot quad waves.
    // (AAI_POLICY_PREFER_CELL asks for the cell kernel all the same)
    if (!r.preferCell && (int64_t)((r.dW + 62) / 63) * ((r.dH + 7) / 8) < 1024) return false;      // (in waves of 63 columns x 8 rows, whatever the wave's shape)
    const int64_t esz = (int64_t)src_elem_size(srcType);
    if (r.chan > 1) {
        // interleaved channels (aai_cell_multi_kernel, 64 x 1 wave): windows whose slots fit 64 KiB of LDS, below 4 GiB
        if (r.chan > kQuadMaxChan) return false;
        // Where it wins (tools/interleaved_bench.py, profiles/r04_interleaved.txt): replicated sources of any type (x2 up-sampling of RGB
        // fp32 at 30 degrees: 1.48 ms against the quad kernel's 2.78) and fp32 pixels (config 3's geometry, RGB: 0.72 against 0.77);
        // 8- / 16-bit pixels without replication stay on aai_quad_multi_kernel (RGB 8-bit: 0.49 ms there, 0.68 here -- one lane's window
        // of packed words is unpacked for four dst pixels' sums, and four channels' sums cross lanes and rows)
        if (esz != 4 && r.scale <= 1 && !r.preferCell) return false;
        const CellConsts<float> z = make_cell_consts<float>(r.side, r.c, r.s);
        if (!cell_multi_fits_lds(z.win, slot_words((size_t)esz, r.chan))) return false;
        return !spans_4gib(r, srcType, sv);
    }
    if (!spans_4gib(r, srcType, sv)) return true;
    // 4 GiB and more: every wave rebases its offsets on its own first source row (aai_cell_kernel, QuadMap::rebaseWaves); the rows one
    // wave can touch -- 64 cell columns and up to 33 cell rows of `side` lattice points each, plus its windows -- must span less than
    // 4 GiB, and the 24-bit multiplies of the window addresses need a pitch below 8 MiB
    const int64_t span = (int64_t)((97.0 * r.side + 24.0) / (r.scale > 0 ? r.scale : 1)) + 2;
    return sv.rowStride * esz < ((int64_t)1 << 23) && span * sv.rowStride * esz < ((int64_t)1 << 32);
}

// ---- what the launchers write into their copy of the QuadMap for a view (launch_quad, launch_wide, launch_cell) ----------------------
// plain images of 4 GiB and more under the quad and wide kernels: lane offsets are relative to an anchor row per wave (QuadSrc::issue)
inline int quad_map_anchor_rows(const RotLaunch &r, int srcType, ImageView sv) { return spans_4gib(r, srcType, sv) ? quad_anchor_rows(r) : 0; }
// ... and under the cell kernel every wave rebases its offsets on its own first source row (interleaved images never get there)
inline int cell_map_rebase_waves(const RotLaunch &r, int srcType, ImageView sv) { return r.chan <= 1 && spans_4gib(r, srcType, sv) ? 1 : 0; }

}  // namespace aai
