// aai_plan.hpp -- host-side geometry ("plan") for one resampling request, and the argument blocks the
// device kernels consume.  Host code is plain C++17 (no HIP types) so that validation and layout
// queries work on machines without a GPU.
//
// Geometry follows SURVEY.md Appendix A, i.e. Source.cpp:112-305 of the reference, evaluated in double
// precision.  Nothing the reference materialises per pixel (modSrc, dstPos, the edge-line tables) is
// stored: they are affine in the pixel indices and are recomputed on the fly.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/aai.h"
#include "aai_rot_math.hpp"

namespace aai {

// ---- geometry --------------------------------------------------------------------------------------
struct Geometry {
    int W = 0, H = 0;            // input image
    int scale = 1;               // Source.cpp:139
    int quadrant = 0;            // Source.cpp:140-146
    double angle = 0;            // reduced angle, degrees, [0,90)
    double sn = 0, cs = 1;       // Source.cpp:147-148
    int mW = 0, mH = 0;          // virtual (scaled, pre-rotated) source size, Source.cpp:150-156
    double isoX = 0, isoY = 0;   // isocenter on the virtual lattice, Source.cpp:173-174
    double ratio = 1, side = 1;  // expansionRatio, dstSideLength, Source.cpp:177-178
    int dW = 0, dH = 0;          // Source.cpp:179-180
    double dIsoX = 0, dIsoY = 0; // Source.cpp:185-186
    double fracX = 0, fracY = 0; // Source.cpp:183-184
    double offX = 0, offY = 0;   // Source.cpp:187-200
    bool lt45 = true;            // Source.cpp:230
    double tsn = 0, tcs = 1, ttn = 0;   // Source.cpp:229-240 (ttn snapped to 0 below DBL_EPSILON)
    bool axisAligned = true;     // ttn == 0 with lt45: dst pixel edges parallel to the source axes
};

// Validates like Source.cpp:112-132 (+ finiteness and size limits) and fills g.  Returns AAI_OK or an
// AAI_ERR_* code with the message in `msg`.
int make_geometry(const aai_request &rq, Geometry &g, std::string &msg);

// Centre of dst pixel (dx,dy) on the virtual lattice, Source.cpp:212-219.
inline void dst_centre(const Geometry &g, double dx, double dy, double &px, double &py)
{
    const double u = (dx + g.fracX) * g.side - g.isoX + g.offX;
    const double v = (dy + g.fracY) * g.side - g.isoY + g.offY;
    px = u * g.cs + v * g.sn + g.isoX;
    py = -u * g.sn + v * g.cs + g.isoY;
}

// Interior width (virtual pixels, L - cos - sin) from which the area kernel walks rows as runs.
constexpr double kRunsMinInterior = 3.25;

// Fills the uniform block of the per-output-pixel kernels (K2-K5) from the geometry.
RotLaunch make_rot_launch(const Geometry &g, int mode, int policy);

// Virtual pixel (X, Y) -> element of the source image for the quad kernel (Source.cpp:164-167: the pre-rotation only
// flips / swaps axes, and (m - 1 - X) div scale = m / scale - 1 - X div scale because m is a multiple of scale):
//   element = base + uX * strideX + uY * strideY,  uX = flipX ? nX - 1 - X div scale : X div scale  (uY alike)
// with non-negative strides, so that a lane addresses its pixels with unsigned 32-bit byte offsets from one uniform
// base.  rowStride in elements; srcRow0 = the source row the image pointer addresses (row bands).
struct QuadMap {
    int64_t base;                // elements; negative for a band (base = -srcRow0 * rowStride)
    int64_t strideX, strideY;    // elements per step of uX / uY: 1 or rowStride
    int nX, nY;                  // source pixels along virtual X / Y (mW / scale, mH / scale)
    int flipX, flipY;
    int scale;
    float invScale;
    double invScaleD;
    // interleaved 8- / 16-bit pixels are fetched with one 4- / 8-byte load each, which may reach past the pixel: loads start
    // no later than lastLoad4 / lastLoad8 (byte offsets of the last 4 / 8 bytes of the image) and shift the rest away
    uint32_t lastLoad4, lastLoad8;
    int anchorRows;              // set by the launcher for plain images of 4 GiB and more: offsets are relative to an anchor row per wave (QuadSrc::issue)    // set by the launcher when the kernel skips the pixels the plan's scans flagged: one bit per 16 x 16 dst tile, set where the tile holds
    // a flagged pixel (tileFlagWords 32-bit words per tile row, one more than the tiles need: a wave reads two words at once), so that
    // a wave of the cell kernel asks for the per-pixel masks only where there is something to find; NULL = no summary
    const unsigned *tileFlags;
    int tileFlagWords;
    // Plain fp32 images without replication, a window wholly inside the lattice (QuadSrc::issue's common case): the byte offset of
    // the first element of the window's first line IN MEMORY ORDER is fastC0 + X fastSX + Y fastSY - (WIN - 1) fastRev4 (mod 2^32,
    // (X, Y) = virtual pixel of window position (0, 0)), its lines follow fastLine bytes apart.  fastOk: the fields are valid (lattice
    // below 2^23 pixels a side, so that a 24-bit multiply serves the contiguous axis).
    // (last in the struct: kernels that never read them do not pull them into scalar registers with their neighbours)
    uint32_t fastC0, fastSX, fastSY, fastLine, fastRev4;
    int fastAlongX, fastOk;      // fastAlongX: the contiguous axis is virtual X (quadrants 0 / 2)
    // every index x byte-stride product of the map fits a 24-bit multiply (v_mul_i32_i24, full rate, where the 32-bit multiply runs at a
    // quarter): fewer than 2^23 source pixels a side and a row pitch below 8 MiB.  fastOk implies it.
    int mul24Ok;
    // set by the cell kernel's launcher for plain images of 4 GiB and more: every wave moves its base pointer to the first source row its
    // cells can touch and takes that row's byte offset (mod 2^32) off its 32-bit lane offsets (QuadSrc::rebase, aai_rotated_cell.hip)
    int rebaseWaves;
};
QuadMap make_quad_map(const Geometry &g, int64_t rowStride, int srcRow0, int channels = 1, int elementBytes = 4);      // channels: elements per pixel (interleaved)

// ---- K1: separable axis-aligned tables ---------------------------------------------------------------
// One entry per output index along one axis: the source window [s0,s1] along the matching SOURCE axis
// (original-image indices, ascending) and the three distinct weights a box footprint can produce.
// Weights are already divided by the window's total weight, so the kernel never normalises.
struct alignas(16) AxisEntry {
    int32_t s0, s1;      // inclusive source index range; s0 > s1 never happens (empty => weights 0)
    float wFirst;        // weight of s0
    float wMid;          // weight of every index strictly between s0 and s1
    float wLast;         // weight of s1 (unused when s0 == s1)
    int32_t pad[3];
};
static_assert(sizeof(AxisEntry) == 32, "AxisEntry layout");

// A wave strip: output indices [k0,k1) along the lane axis whose windows all lie in [x0, x0+STRIP_COLS).
struct alignas(16) AxisStrip { int32_t k0, k1, x0, pad; };

// Output indices [k0, k1) along one axis whose entries are all empty (weights 0: dst pixels off the image)
struct AxisRun { int32_t k0, k1; };

constexpr int STRIP_COLS = 256;   // 64 lanes x float4

struct AxisTables {
    std::vector<AxisEntry> lane;     // along source x (the coalesced, lane-mapped axis): nA entries
    std::vector<AxisEntry> row;      // along source y: nB entries
    std::vector<AxisStrip> strips;   // partition of the lane axis
    int nA = 0, nB = 0;
    // output element for (ka,kb) = base + ka*strideA + kb*strideB   (in elements of one dst image, with
    // the dst row stride folded in by the launcher)
    bool transposed = false;         // lane axis runs along dst y (quadrants 1 and 3)
    bool flipA = false, flipB = false;
    bool wide = false;               // some window is wider than a strip -> per-pixel fallback kernel
    int maxRowSpan = 0;              // largest s1-s0+1 over the row table
    bool rowsShared = false;         // consecutive output rows read a common source row (windows not pixel-aligned)
    int maxOutputsPerStrip = 0;
    int channels = 1;                // interleaved channels: the lane table has nA = pixels * channels entries, taps `channels` apart
    // Maximal runs of empty entries (as a rule the first and the last few of a table, when the canvas overhangs the image).  K1 multiplies
    // the parked window of such an entry by its weights of 0, which is 0 for finite data only: the launcher stores 0 into these rows and
    // columns behind K1 (launch_axis_zero), so that a NaN or Inf at the parked position stays where it is.
    std::vector<AxisRun> emptyLane, emptyRow;
};
void axis_empty_runs(const std::vector<AxisEntry> &tab, std::vector<AxisRun> &runs);

// mode: AAI_MODE_AREA (overlap lengths) or AAI_MODE_FAST (centre counts).  Only for g.axisAligned.
void build_axis_tables(const Geometry &g, int mode, AxisTables &t, int channels = 1);
void restrict_axis_tables_to_band(const Geometry &g, AxisTables &t, int row0, int row1, int &srcRow0, int &srcRow1, int extraRows = 0);

// (ka, kb) -> dst element of K1: outBase + (ka / outChan) * outStrideA + ka % outChan + kb * outStrideB.  The lane axis is dst x unless
// the quadrant transposes; flips run an axis backwards.  With interleaved channels a dst pixel is `channels` elements
// wide and lane entry ka = pixel * channels + channel.  dstStride: elements of a dst row.
struct AxisOutMap {
    int64_t outBase, outStrideA, outStrideB;
    int tapStep, outChan;
};
inline AxisOutMap axis_out_map(const AxisTables &t, int channels, int64_t dstStride)
{
    AxisOutMap m{};
    const int nApix = t.nA / channels;
    const int64_t sa = t.transposed ? dstStride : channels, sb = t.transposed ? channels : dstStride;
    m.outStrideA = t.flipA ? -sa : sa;
    m.outStrideB = t.flipB ? -sb : sb;
    m.outBase = (t.flipA ? (int64_t)(nApix - 1) * sa : 0) + (t.flipB ? (int64_t)(t.nB - 1) * sb : 0);
    m.tapStep = channels; m.outChan = channels;
    if (channels > 1 && !t.transposed && !t.flipA) { m.outStrideA = 1; m.outChan = 1; }     // lane order = dst element order
    return m;
}

// ---- K1: the launch shape (aai_axis.hip: launch_axis_typed launches what axis_launch_shape says) ---------------------------------
// Stated here, without HIP types, so that the variant probe of the tests (tests/emulation: aai_emu_axis_variant, tests/axis_variants.py)
// asks the function the launcher asks.
constexpr int kAxisWaves = 4;          // waves (= strips of the strip kernel) per workgroup
constexpr int kAxisTileCols = 16;      // output rows (= dst columns) a wave of the tile kernel gathers

enum AxisKernelKind { AXIS_RUN_NOTHING = 0, AXIS_RUN_STRIP = 1, AXIS_RUN_TILE = 2, AXIS_RUN_WIDE = 3 };      // aai_axis_kernel, aai_axis_tile_kernel, aai_axis_wide_kernel

// what the choice reads: fields of AxisLaunch (aai_kernels.hpp) of the same names, the source's element size and the batch
struct AxisShapeFacts {
    int nA, nB, nStrips;
    int wide, maxRowSpan, rowsShared, maxOutputsPerStrip;
    int transposed, tapStep;
    int64_t outStrideB;
    int tuneRows, tuneNt;
    int elemBytes;               // 4, 2 or 1
    int batch;
};

struct AxisShape {
    int kernel;                  // AxisKernelKind
    int nt;                      // nontemporal source loads (strip and tile kernels)
    int rows;                    // output rows per workgroup (strip kernel; the tile kernel's workgroups take kAxisWaves * kAxisTileCols)
    int tileNR;                  // tile kernel: source rows per pipeline window (axis_tile_window_rows)
    unsigned gridX, gridY, gridZ;      // strip and tile kernels (the wide kernel: gridX and gridZ; its rows go in launches of 65535 * 4)
    int banded;                  // strip kernel: workgroups take their (strip block, row block) from axis_block_order
};

// The banded workgroup order of the strip kernel's streaming class.  Workgroups are dealt round-robin over the 8 XCDs, each with an L2
// of its own, and every 4 KiB piece a strip reads shares its first 128-byte line with the strip to its left.  In launch order the
// strip blocks of one row block are CONSECUTIVE workgroups and so sit behind eight different L2s (at gridX == 8, XCD j reads column
// block j of every row and nothing else): every shared line is fetched twice.  Here the linear index b = blockIdx.y * gridX +
// blockIdx.x of a workgroup within its image is re-read: of every group of 8 gridX consecutive workgroups, those with equal b % 8
// take ONE whole row block, strip block by strip block (xcd_tile's arithmetic, aai_quad_src.hpp, with a band of one row block), so
// that the eight XCDs advance in step over eight consecutive row blocks.  The row blocks past the last whole group of 8 keep launch
// order: the grid stays exactly axis_launch_shape's, the map is a bijection of [0, gridX gridY) for every grid, and nothing depends
// on where a workgroup really runs -- a different placement costs the shared lines again, never a result.
AAI_HD void axis_block_order(unsigned b, unsigned gridX, unsigned gridY, int *bx, int *by)
{
    const unsigned group = 8u * gridX, banded = (gridY >> 3) * group;      // workgroups of the whole groups of 8 row blocks
    if (b >= banded) {
        *bx = (int)(b % gridX);
        *by = (int)(b / gridX);
        return;
    }
    const unsigned super = b / group, within = b - super * group;
    *bx = (int)(within >> 3);
    *by = (int)(super * 8u + (within & 7u));
}

// The tile kernel's pipeline: windows of at most four source rows (ratios up to 3) run eight output rows in flight, windows of up to
// eight rows (ratios up to 4, where a strip still holds more than 64 outputs) four.  Asked by aai_axis_tile_kernel itself.
AAI_HD constexpr int axis_tile_window_rows(int maxRowSpan) { return maxRowSpan <= 4 ? 4 : 8; }

// Which of its five branches aai_axis_kernel takes for a strip of nOut outputs, in the order of the source.  This RESTATES the five
// conditions of the if / else chain in aai_axis_kernel (aai_axis.hip) for the tests' variant probe; the kernel keeps its own text,
// because routing it through this function changes the code the compiler emits for it.  Change both together.
//   A  transposed quadrants, one output per lane, eight dst columns in registers      B  transposed, up to four outputs per lane, four columns
//   C  one output per lane      D  four consecutive outputs per lane (dst x along the lanes)      E  lanes walk the outputs
enum AxisStripBranch { AXIS_BRANCH_A = 0, AXIS_BRANCH_B = 1, AXIS_BRANCH_C = 2, AXIS_BRANCH_D = 3, AXIS_BRANCH_E = 4 };
AAI_HD constexpr int axis_strip_branch(bool interleaved, int nOut, int64_t outStrideA, int64_t outStrideB)
{
    return (!interleaved && nOut <= 64 && (outStrideB == 1 || outStrideB == -1))    ? AXIS_BRANCH_A
           : (!interleaved && nOut <= 256 && (outStrideB == 1 || outStrideB == -1)) ? AXIS_BRANCH_B
           : nOut <= 64                                                             ? AXIS_BRANCH_C
           : (nOut <= 256 && outStrideA == 1)                                       ? AXIS_BRANCH_D
                                                                                    : AXIS_BRANCH_E;
}

// Launch shape (see the comment at aai_axis_kernel for the measurements behind the defaults).
// Defaults from the sweeps in profiles/r01_axis_tune_*.txt (8192^2 sources):
//   * windows that share source rows between output rows (grid not pixel-aligned) want cached loads and
//     two rows per workgroup (5.8 vs 5.2 TB/s at 4:1); disjoint windows want nontemporal loads;
//   * >= 4 source rows per output row: one output row per workgroup (6.8 TB/s at 4:1; 5.3 at 8 rows);
//   * 2-3 source rows: four (5.0-5.2 TB/s vs 3.7-4.6 at one or two);
//   * ratios below 2 (129..256 outputs per strip, write-heavy): 32 rows per workgroup (4.2 TB/s at 1:1
//     vs 2.5 at four and 1.4 at one); the up-sampling path (more than 256 outputs per strip) prefers 4;
//   * 8- and 16-bit sources move 4x / 2x fewer bytes and are bound by per-wave latency, not by HBM: eight / four
//     rows per workgroup (8192^2 u8 -> 2048^2: 28 us at one row, 21 at eight; profiles/r01_typed_sources.txt).
inline AxisShape axis_launch_shape(const AxisShapeFacts &a)
{
    AxisShape s{};
    if (a.nA <= 0 || a.nB <= 0 || a.batch <= 0) return s;
    s.gridZ = (unsigned)a.batch;
    if (a.wide) {
        s.kernel = AXIS_RUN_WIDE;
        s.gridX = (unsigned)((a.nA + 63) / 64);
        return s;
    }
    int nt = a.rowsShared ? 0 : 1;
    int rows = a.maxRowSpan >= 4 ? (a.rowsShared ? 2 : 1) : 4;
    if (a.elemBytes < 4) {
        // ... as long as that leaves a few workgroups per CU
        const int want = a.elemBytes == 1 ? 8 : 4;
        const int64_t stripBlocks = (int64_t)((a.nStrips + kAxisWaves - 1) / kAxisWaves) * a.batch;
        while (rows < want && stripBlocks * ((a.nB + 2 * rows - 1) / (2 * rows)) >= 2048) rows *= 2;
    }
    if (a.transposed) {
        // transposed quadrants: 2, 4 or 8 dst columns per lane and store; about 16 source rows per workgroup is the
        // sweet spot between DRAM page locality and store width (8192^2 at 90 degrees: 4:1 5.9 TB/s at 4 rows vs 5.2 at
        // 8; 8:1 6.0 at 2 vs 4.8 at 8; profiles/r01_axis_transposed.txt)
        rows = a.maxRowSpan >= 8 ? 2 : (a.maxRowSpan >= 3 ? 4 : 8);
        if (a.maxOutputsPerStrip > 64) rows = a.maxRowSpan >= 2 ? 4 : 16;     // the four-column path (ratios below 4)
    }
    if (!a.transposed && a.maxOutputsPerStrip > 128 && a.maxOutputsPerStrip <= 256) rows = 32;      // ratios below 2: write-heavy
    // the plan's measured choice for this (geometry, device) -- fp32 sources only (aai_engine.cpp: tune_axis_plan)
    if (a.elemBytes == 4 && a.tuneRows > 0) { rows = a.tuneRows; nt = a.tuneNt; }
    s.nt = nt;
    // the banded order (axis_block_order): plain fp32 sources whose windows share no source row, streamed with nontemporal loads.
    // Plans with shared rows keep launch order on purpose: vertically adjacent workgroups there read a common source row, and at
    // gridX == 8 launch order already puts them on one XCD.  The transposed quadrants keep launch order too: consecutive row blocks
    // there write neighbouring dst COLUMNS, i.e. the same dst lines, and launch order keeps those behind one L2 -- banded, 8192^2 at 90
    // degrees went from 53.8 to 60.5 us at 4:1 (270 degrees: 53.1 to 60.7) and from 47.6 to 54.2 us at 8:1, where 0 / 180 degrees gain
    // (48.9 to 46.6, 47.7 to 46.6; 16:1 46.3 to 44.5; profiles/axis_order.txt).  (Set for the strip kernel only, below.)
    const int banded = nt && !a.rowsShared && !a.transposed && a.elemBytes == 4 && a.tapStep <= 1;
    // The LDS-tile kernel (measured, profiles/r01_axis_transposed.txt: wins below 2:1 -- 1:1 1.8 -> 2.3 TB/s, x4 up-sampling 1.2 -> 1.6 --
    // and loses 5-14 % to the four-column register path between 2:1 and 4:1)
    // ... and, since its output rows run in a software pipeline and its waves store together, down to 64 outputs per strip (ratios up
    // to 4) wherever no output row needs more than the pipeline's eight source rows: 3:1 at 270 degrees 300 -> 242 us per 4 images,
    // 2.5:1 351 -> 271, 2:1 285 -> 275 (profiles/r03_axis_tile.txt)
    const bool tileable = a.transposed && a.tapStep <= 1 && (a.outStrideB == 1 || a.outStrideB == -1) && a.maxOutputsPerStrip <= 256;
    const bool tile = tileable && (a.maxOutputsPerStrip > 128 || (a.maxOutputsPerStrip > 64 && a.maxRowSpan <= 8));
    if (tile && (a.nB + kAxisTileCols - 1) / kAxisTileCols <= 65535) {
        // transposed quadrants at ratios below 4: LDS tile, stores along dst x (see aai_axis_tile_kernel); one strip per workgroup
        s.kernel = AXIS_RUN_TILE;
        s.rows = kAxisWaves * kAxisTileCols;
        s.tileNR = axis_tile_window_rows(a.maxRowSpan);
        s.gridX = (unsigned)a.nStrips;
        s.gridY = (unsigned)((a.nB + kAxisWaves * kAxisTileCols - 1) / (kAxisWaves * kAxisTileCols));
        return s;
    }
    int blocksY = (a.nB + rows - 1) / rows;
    while (blocksY > 65535) { rows *= 2; blocksY = (a.nB + rows - 1) / rows; }
    s.kernel = AXIS_RUN_STRIP;
    s.rows = rows;
    s.gridX = (unsigned)((a.nStrips + kAxisWaves - 1) / kAxisWaves);
    s.gridY = (unsigned)blocksY;
    s.banded = banded;
    return s;
}

// ---- the transpose of K1 (aai_axis_adjoint.hip) ------------------------------------------------------------
// Output indices [k0, k1] (inclusive) along one axis whose window holds a given source index; k0 > k1: no dst pixel reads it.
struct AxisRange { int32_t k0, k1; };
static_assert(sizeof(AxisRange) == 8, "AxisRange layout");

// Inverts the two tables of a whole-image, single-channel plan: one range per source column (from t.lane) and per source row
// (from t.row).  Windows are monotone in the output index, so the outputs that read a source index are consecutive; this is
// CHECKED entry by entry (every k of a range is a non-empty entry whose window holds the index, every window lies in the
// image), and false is returned where it does not hold -- the caller then keeps the general adjoint.
bool build_axis_adjoint_ranges(const AxisTables &t, int W, int H, std::vector<AxisRange> &cols, std::vector<AxisRange> &rows);

// Source indices along one axis that some window of the table only GRAZES: its first or last weight is below 1e-9 of the dst pixel's
// total, a rounding residue of an edge that should lie on the pixel boundary.  Whether such a residue counts is a decision of the
// reference's classifier, taken pair by pair (the forward's tolerance does not see 1e-16; the adjoint's exact zeros do), so the
// source pixels of these rows and columns are left to the general adjoint (build_adjoint_lists).
void axis_grazed_indices(const std::vector<AxisEntry> &tab, std::vector<int> &grazed);

// The pixels the general adjoint recomputes behind the transposed separable kernel.  srcList = every source pixel inside the window
// (rot_window) of a flagged dst pixel (dx, dy) of the plan, and every pixel of the grazed source rows and columns; dstList = every
// dst pixel the general gather visits for a pixel of srcList (adjoint_gather's own candidate box, one more pixel on every side).
// Both deduplicated, (x, y) pairs in row-major order.  False when srcList would exceed maxSource pixels (the lists are then empty).
bool build_adjoint_lists(const RotLaunch &r, const std::vector<std::pair<int, int>> &flagged, const std::vector<int> &grazedCols,
                         const std::vector<int> &grazedRows, size_t maxSource,
                         std::vector<std::pair<int, int>> &srcList, std::vector<std::pair<int, int>> &dstList);

// K1's separable model checked on the host, one representative per (column class, row class), where the geometry's
// arithmetic is exact (aai_plan.cpp); false = does not qualify, run the device scan.  flagged: (dx, dy) of the dst pixels
// the fix-up pass must recompute; dense: more than maxListed of them.
bool axis_verify_by_class(const RotLaunch &r, std::vector<std::pair<int, int>> &flagged, bool &dense, unsigned maxListed);

// Source rows [srcRow0, srcRow1) that dst rows [row0,row1) of a rotated-lattice request can touch (conservative).
void rotated_band_source_rows(const Geometry &g, int row0, int row1, bool sampler, int &srcRow0, int &srcRow1);
// Live span of every 16-row tile row of the dst canvas, in 16-column tiles: spans[2 t] ... spans[2 t + 1] (first > last: none).
// Tiles outside it hold only pixels that are 0 in every mode (rot_live_cols); empty when the geometry has no dead tiles to speak of.
void rotated_live_spans(const RotLaunch &r, bool sampler, std::vector<int> &spans);

}  // namespace aai
