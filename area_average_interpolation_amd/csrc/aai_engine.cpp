// aai_engine.cpp -- the host-side engine behind the C ABI: per-thread error state, request checks, the plan cache
// (K1 tables and launch-shape measurement, the one-off scans of a geometry and their fix-up lists) and the dispatch of a
// request onto the kernels.  aai_capi.cpp holds the extern "C" entry points and the host-buffer paths built on this.
//
// There is deliberately no CPU implementation here: without a HIP device every compute entry point fails with
// AAI_ERR_NO_DEVICE.  The CPU oracle under oracle/ is test infrastructure and is never linked or loaded.
#include "aai_engine.hpp"
#include "../../include/aai_half.h"

#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <map>
#include <tuple>
#include <cstdlib>
#include <cstring>
#include <algorithm>

namespace aai {
namespace engine {

thread_local std::string g_lastError;
thread_local std::string g_lastKernel;

int fail(int code, const std::string &msg)
{
    g_lastError = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    // a missing / unusable device is reported as such so callers can tell it from a kernel fault
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver || e == hipErrorNotInitialized)
        return fail(AAI_ERR_NO_DEVICE, m);
    return fail(AAI_ERR_HIP, m);
}

// ---- plan cache ------------------------------------------------------------------------------------
std::mutex g_planMutex;
std::list<PlanRef> &plan_cache()
{
    static std::list<PlanRef> *cache = new std::list<PlanRef>();      // never destroyed: no HIP calls from static destructors
    return *cache;
}
static std::mutex g_poolMutex;
static std::map<int, DevicePool *> &pools()
{
    static std::map<int, DevicePool *> *m = new std::map<int, DevicePool *>();
    return *m;
}
DevicePool &device_pool(int device)
{
    std::lock_guard<std::mutex> lock(g_poolMutex);
    DevicePool *&p = pools()[device];
    if (!p) p = new DevicePool();
    return *p;
}
// the pool's build stream, created on first use (callers hold no lock)
static hipError_t pool_build_stream(DevicePool &pool, hipStream_t *out)
{
    std::lock_guard<std::mutex> lock(pool.m);
    if (!pool.build) {
        const hipError_t e = hipStreamCreateWithFlags(&pool.build, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
    }
    *out = pool.build;
    return hipSuccess;
}
// the side streams and their events; under pool.m.  A failure leaves the pool without them (passes then run in-stream).
static void pool_create_sides(DevicePool &pool)
{
    hipError_t e = hipSuccess;
    for (int k = 0; k < DevicePool::kSideSlots && e == hipSuccess; ++k) {
        // (Default priority.  Created with the highest priority -- so that the pass's few hundred short workgroups would go first
        // -- the mere existence of such streams cost EVERY kernel of the process a third to a half of its rate: config 3 162 ->
        // 270 us, its fast mode 98 -> 217 us, 8:1 171 -> 329 us: profiles/r04_fixup_beside.txt.)
        e = hipStreamCreateWithFlags(&pool.side[k], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&pool.fork[k], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&pool.join[k], hipEventDisableTiming);
    }
    if (e == hipSuccess) pool.sideReady = true;
    else { (void)hipGetLastError(); pool.sideFailed = true; }
}

void drop_plans()
{
    std::list<PlanRef> gone;
    {
        std::lock_guard<std::mutex> lock(g_planMutex);
        gone.swap(plan_cache());
    }
    gone.clear();                     // frees device memory of every plan nobody is launching from
    // ... and the pools' streams and events (created again on the next need)
    std::lock_guard<std::mutex> lock(g_poolMutex);
    int current = -1;
    (void)hipGetDevice(&current);
    for (auto &kv : pools()) {
        DevicePool &pool = *kv.second;
        std::lock_guard<std::mutex> plock(pool.m);
        if (hipSetDevice(kv.first) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (pool.build) { (void)hipStreamSynchronize(pool.build); (void)hipStreamDestroy(pool.build); pool.build = nullptr; }
        for (int k = 0; k < DevicePool::kSideSlots; ++k) {
            if (pool.side[k]) { (void)hipStreamSynchronize(pool.side[k]); (void)hipStreamDestroy(pool.side[k]); pool.side[k] = nullptr; }
            if (pool.fork[k]) { (void)hipEventDestroy(pool.fork[k]); pool.fork[k] = nullptr; }
            if (pool.join[k]) { (void)hipEventDestroy(pool.join[k]); pool.join[k] = nullptr; }
        }
        pool.sideReady = false; pool.sideFailed = false; pool.besideLaunches = 0;
        if (pool.scratch) { (void)hipMemPoolDestroy(pool.scratch); pool.scratch = nullptr; }      // (its memory goes once the frees in flight have run)
    }
    if (current >= 0) (void)hipSetDevice(current);
}
constexpr size_t kMaxPlans = 32;       // per device
constexpr unsigned kMaxListedPixels = 1u << 24;      // beyond 16 M flagged pixels the whole image takes the double-precision pass

// (AAI_MAX_LISTED_PIXELS: test hook, lowers the threshold so that small geometries exercise the dense form; documented in include/aai.h)
static unsigned max_listed_pixels()
{
    static const unsigned maxListed = [] { const char *v = getenv("AAI_MAX_LISTED_PIXELS"); return v ? (unsigned)strtoul(v, nullptr, 10) : kMaxListedPixels; }();
    return maxListed;
}

bool same_request(const aai_request &a, const aai_request &b)
{
    // (AAI_POLICY_DIAG_NO_FIXUP is a property of a launch, not of the plan: with and without it a request shares one plan)
    return a.mode == b.mode && (a.policy & ~AAI_POLICY_DIAG_NO_FIXUP) == (b.policy & ~AAI_POLICY_DIAG_NO_FIXUP) && a.src_width == b.src_width && a.src_height == b.src_height &&
           a.src_res_x == b.src_res_x && a.src_res_y == b.src_res_y && a.dst_res_x == b.dst_res_x &&
           a.dst_res_y == b.dst_res_y && a.src_iso_x == b.src_iso_x && a.src_iso_y == b.src_iso_y &&
           a.rotation_deg == b.rotation_deg;
}

int check_request(const aai_request *rq)
{
    if (!rq) return fail(AAI_ERR_BAD_ARGUMENT, "Null request.");
    if (rq->mode < AAI_MODE_AREA || rq->mode > AAI_MODE_BICUBIC) return fail(AAI_ERR_BAD_ARGUMENT, "Unknown interpolation mode.");
    const int rule = rq->policy & AAI_POLICY_RULE_MASK;
    const int known = AAI_POLICY_RULE_MASK | AAI_POLICY_DOUBLE_PRECISION | AAI_POLICY_PREFER_CELL | AAI_POLICY_DIAG_NO_FIXUP;
    if ((rule != AAI_POLICY_REFERENCE && rule != AAI_POLICY_EXACT) || (rq->policy & ~known)) return fail(AAI_ERR_BAD_ARGUMENT, "Unknown weight policy.");
    return AAI_OK;
}

// K1 row bands keep one more source row on either side where the fix-up pass behind K1 may run (get_plan: verifyAxis):
// its window includes rows that only touch the dst pixel
int axis_band_margin(const aai_request &rq)
{
    return rq.mode == AAI_MODE_AREA || rq.mode == AAI_MODE_FAST ? 1 : 0;
}

int pick_kernel(const aai_request &rq, const aai::Geometry &g)
{
    if (rq.mode == AAI_MODE_BILINEAR || rq.mode == AAI_MODE_BICUBIC) return AAI_KERNEL_SAMPLE;
    if (g.axisAligned) return AAI_KERNEL_AXIS;
    return rq.mode == AAI_MODE_FAST ? AAI_KERNEL_FAST : AAI_KERNEL_ROTATED;
}

int resolved_kernel(const aai_request &rq, const aai::Geometry &g)
{
    int kernel = pick_kernel(rq, g);
    if (kernel == AAI_KERNEL_AXIS) {
        aai::AxisTables t;
        aai::build_axis_tables(g, rq.mode, t);
        if (t.wide) kernel = AAI_KERNEL_AXIS_WIDE;
    }
    return kernel;
}

void fill_layout(const aai::Geometry &g, int kernel, aai_layout *out)
{
    aai_layout l{};
    l.dst_width = g.dW; l.dst_height = g.dH;
    l.dst_iso_x = g.dIsoX; l.dst_iso_y = g.dIsoY;
    l.scale = g.scale; l.quadrant = g.quadrant;
    l.reduced_angle_deg = g.angle; l.side = g.side;
    l.kernel = kernel;
    *out = l;
}

// the argument block of K1 for a plan and a dst row stride (elements)
static aai::AxisLaunch make_axis_launch(const Plan &p, int channels, int64_t dstStride)
{
    const aai::AxisTables &t = p.tabs;
    const aai::Geometry &g = p.g;
    aai::AxisLaunch a{};
    a.laneTab = p.dLane; a.rowTab = p.dRow; a.strips = p.dStrips;
    a.nA = t.nA; a.nB = t.nB; a.nStrips = (int)t.strips.size();
    a.srcW = g.W * channels; a.srcH = g.H;      // elements of a source row
    a.wide = t.wide ? 1 : 0;
    a.maxRowSpan = t.maxRowSpan;
    a.rowsShared = t.rowsShared ? 1 : 0;
    a.maxOutputsPerStrip = t.maxOutputsPerStrip;
    // (ka, kb) -> dst element: axis_out_map (aai_plan.hpp)
    const aai::AxisOutMap m = aai::axis_out_map(t, channels, dstStride);
    a.outStrideA = m.outStrideA; a.outStrideB = m.outStrideB; a.outBase = m.outBase;
    a.transposed = t.transposed ? 1 : 0;
    a.tapStep = m.tapStep; a.outChan = m.outChan;
    a.tuneRows = p.tuneRows; a.tuneNt = p.tuneNt;
    return a;
}

// K1 is HBM-bound and its best launch shape moves with the box by a few per cent (the same binary measured 5.8 to 6.9
// TB/s across boxes of one pool: profiles/r01_axis_tune_sweep2.txt, profiles/r02_axis_autotune.txt), so the first plan of
// a CLASS of large streaming geometries on a device times the shapes that ever win -- output rows per workgroup,
// nontemporal or cached loads -- on scratch images larger than the Infinity Cache and keeps the fastest; later plans of
// the class (same device, same rows per footprint, same row sharing, same width class) take the result from a cache.
// Bounds: plain fp32 images, footprints of >= 4 source rows, un-transposed quadrants, whole image; scratch of at most
// ~1.25 GiB of source copies plus their outputs (images too large for that take the class's cached shape or the built-in
// one); a private stream; about 13 ms (profiles/axis_order.txt).  AAI_AXIS_AUTOTUNE=0 disables it.  (Documented in include/aai.h at aai_prepare.)
struct TuneKey {
    int device, rowSpan, rowsShared, widthClass;
    bool operator<(const TuneKey &o) const
    {
        return std::tie(device, rowSpan, rowsShared, widthClass) < std::tie(o.device, o.rowSpan, o.rowsShared, o.widthClass);
    }
};
struct TuneShape { int rows, nt; };
static std::mutex g_tuneMutex;
static std::map<TuneKey, TuneShape> &tune_cache()
{
    static std::map<TuneKey, TuneShape> *m = new std::map<TuneKey, TuneShape>();
    return *m;
}

static void tune_axis_plan(Plan &p, int channels, int band0, hipStream_t stream)
{
    static const bool enabled = [] { const char *e = getenv("AAI_AXIS_AUTOTUNE"); return !(e && atoi(e) == 0); }();
    const aai::AxisTables &t = p.tabs;
    const aai::Geometry &g = p.g;
    const size_t srcBytes = sizeof(float) * (size_t)g.W * g.H, dstBytes = sizeof(float) * (size_t)g.dW * g.dH;
    if (!enabled || channels != 1 || band0 >= 0 || t.wide || t.transposed || t.maxRowSpan < 4 || t.maxOutputsPerStrip > 64 ||
        srcBytes < ((size_t)64 << 20) || !dstBytes)
        return;
    int widthClass = 0;
    while ((g.W >> widthClass) > 1) ++widthClass;
    const TuneKey key{p.device, std::min(t.maxRowSpan, 64), t.rowsShared ? 1 : 0, widthClass};
    {
        std::lock_guard<std::mutex> lock(g_tuneMutex);
        auto it = tune_cache().find(key);
        if (it != tune_cache().end()) {
            p.tuneRows = it->second.rows; p.tuneNt = it->second.nt; p.tuneSource = 2;
            return;
        }
    }
    constexpr size_t kScratchCap = (size_t)5 << 28;           // 1.25 GiB of source copies
    if (2 * srcBytes > kScratchCap) return;                   // too large to measure within the cap: built-in shape
    // at least two images and at least 512 MiB of source per launch: twice the 256 MiB Infinity Cache, so every launch streams
    // from HBM (1 GiB, as bench.py uses, measured the same shapes; half the scratch halves the cost of this measurement)
    const int images = (int)std::min<size_t>(8, std::max<size_t>(2, std::min((((size_t)1 << 29) + srcBytes - 1) / srcBytes, kScratchCap / srcBytes)));
    float *src = nullptr, *dst = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = hipMalloc((void **)&src, srcBytes * images) == hipSuccess && hipMalloc((void **)&dst, dstBytes * images) == hipSuccess &&
              hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    for (int b = 0; b < images && ok; ++b)         // realistic data: the memory system's speed depends on what it moves
        ok = aai::launch_synth(src + (size_t)b * g.W * g.H, g.W, g.H, g.W, (uint64_t)b + 1, stream) == hipSuccess;
    struct Shape { int rows, nt; float ms; };
    Shape shapes[] = {{1, 1, 0.f}, {2, 1, 0.f}, {1, 0, 0.f}, {2, 0, 0.f}, {4, 1, 0.f}};
    const aai::ImageView sv{g.W, (int64_t)g.W * g.H}, dv{g.dW, (int64_t)g.dW * g.dH};
    static const bool trace = [] { const char *v = getenv("AAI_TRACE_PLAN"); return v && atoi(v) != 0; }();
    // one timed turn of a shape: `launches` launches between two events
    auto turn = [&](const Shape &sh, int launches, float &ms) {
        p.tuneRows = sh.rows; p.tuneNt = sh.nt;
        const aai::AxisLaunch a = make_axis_launch(p, 1, g.dW);
        ms = 0.f;
        bool good = hipEventRecord(e0, stream) == hipSuccess;
        for (int i = 0; i < launches && good; ++i) good = aai::launch_axis(a, src, aai::SRC_F32, sv, dst, dv, images, stream, nullptr) == hipSuccess;
        return good && hipEventRecord(e1, stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    };
    // the shapes take turns, two rounds after a warm-up round, two launches per turn; each keeps its faster turn.  This only RANKS
    // them: two turns right after allocation are too thin to decide between shapes a few per cent apart
    for (int round = 0; round < 3 && ok; ++round)
        for (Shape &sh : shapes) {
            float ms = 0.f;
            ok = ok && turn(sh, 2, ms);
            if (ok && round > 0 && (sh.ms == 0.f || ms < sh.ms)) sh.ms = ms;       // round 0 warms up
            if (ok && trace) fprintf(stderr, "[aai tune] round %d rows=%d nt=%d  %.4f ms per launch\n", round, sh.rows, sh.nt, ms / 2);
        }
    // The decision is a duel of the two fastest: kDuelTurns alternating turns of kDuelLaunches launches each, medians compared.  The
    // shapes that ever win lie 4 to 8 % apart and the turns of one shape lie within 1 to 4 % of their median (profiles/axis_order.txt), so
    // the medians of 12 turns settle a difference of 2 % in every process.  The earlier of the two in the list (the built-in shape
    // comes first) is kept unless the other's median is lower by more than 1 %.
    constexpr int kDuelTurns = 12, kDuelLaunches = 4;
    const Shape *first = nullptr, *second = nullptr;
    if (ok) {
        for (const Shape &sh : shapes)
            if (!first || sh.ms < first->ms) { second = first; first = &sh; }
            else if (!second || sh.ms < second->ms) second = &sh;
        if (second < first) std::swap(first, second);                       // list order: `first` is the incumbent
        float t[2][kDuelTurns];
        for (int i = 0; i < kDuelTurns && ok; ++i)
            for (int s = 0; s < 2 && ok; ++s) ok = turn(s ? *second : *first, kDuelLaunches, t[s][i]);
        if (ok) {
            for (int s = 0; s < 2; ++s) std::sort(t[s], t[s] + kDuelTurns);
            const float m0 = 0.5f * (t[0][kDuelTurns / 2 - 1] + t[0][kDuelTurns / 2]), m1 = 0.5f * (t[1][kDuelTurns / 2 - 1] + t[1][kDuelTurns / 2]);
            if (trace)
                for (int s = 0; s < 2; ++s) {
                    const Shape &sh = s ? *second : *first;
                    fprintf(stderr, "[aai tune] duel rows=%d nt=%d  median %.4f ms per launch, turns", sh.rows, sh.nt, (s ? m1 : m0) / kDuelLaunches);
                    for (int i = 0; i < kDuelTurns; ++i) fprintf(stderr, " %.4f", t[s][i] / kDuelLaunches);
                    fprintf(stderr, "\n");
                }
            if (m1 < m0 * 0.99f) first = second;
            if (trace) fprintf(stderr, "[aai tune] chosen rows=%d nt=%d\n", first->rows, first->nt);
        }
    }
    p.tuneRows = 0; p.tuneNt = 0;
    if (ok) {
        p.tuneRows = first->rows; p.tuneNt = first->nt; p.tuneSource = 1;
        std::lock_guard<std::mutex> lock(g_tuneMutex);
        tune_cache()[key] = TuneShape{first->rows, first->nt};
    }
    (void)hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (src) (void)hipFree(src);
    if (dst) (void)hipFree(dst);
}

// Everything a fresh plan needs from the device; the caller holds p.build, not the cache's lock.
static int build_plan(Plan &p, hipStream_t bs)
{
    const aai_request &rq = p.key;
    const aai::Geometry &g = p.g;
    const int band0 = p.band0, band1 = p.band1, channels = p.channels, form = p.form;
    // AAI_TRACE_PLAN=1: stage timings of every plan build on stderr (tools/plan_time.py)
    static const bool trace = [] { const char *v = getenv("AAI_TRACE_PLAN"); return v && atoi(v) != 0; }();
    auto tick = std::chrono::steady_clock::now();
    auto stage = [&](const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[aai plan] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
    };
    // (bs: the caller's stream, or the device pool's build stream -- no stream is created or destroyed here; whatever was
    // enqueued is complete when this returns, also on failure)
    std::vector<int> spans;                                          // (declared before the guard: alive until the stream is synchronised)
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); } } guard{bs};
    if (p.kernel == AAI_KERNEL_AXIS) {
        aai::build_axis_tables(g, rq.mode, p.tabs, channels);
        if (band0 >= 0) aai::restrict_axis_tables_to_band(g, p.tabs, band0, band1, p.srcRow0, p.srcRow1, axis_band_margin(rq));
        if (p.tabs.wide) p.kernel = AAI_KERNEL_AXIS_WIDE;
        auto upload = [&](const void *h, size_t bytes, void **d) -> hipError_t {
            if (!bytes) { *d = nullptr; return hipSuccess; }
            hipError_t e = hipMalloc(d, bytes);
            if (e != hipSuccess) return e;
            return hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, bs);      // (p.tabs outlives the copy: synchronised below)
        };
        hipError_t e = upload(p.tabs.lane.data(), p.tabs.lane.size() * sizeof(aai::AxisEntry), (void **)&p.dLane);
        if (e == hipSuccess) e = upload(p.tabs.row.data(), p.tabs.row.size() * sizeof(aai::AxisEntry), (void **)&p.dRow);
        if (e == hipSuccess) e = upload(p.tabs.strips.data(), p.tabs.strips.size() * sizeof(aai::AxisStrip), (void **)&p.dStrips);
        if (e == hipSuccess) e = hipStreamSynchronize(bs);
        if (e != hipSuccess) return hip_fail(e, "uploading axis tables");
        stage("axis tables");
        if (p.kernel == AAI_KERNEL_AXIS) tune_axis_plan(p, channels, band0, bs);
        stage("launch-shape measurement");
    }
    if (p.kernel == AAI_KERNEL_ROTATED || p.kernel == AAI_KERNEL_FAST || p.kernel == AAI_KERNEL_SAMPLE) {
        // the corners of a rotated canvas hold nothing: which tiles of each tile row can (the whole image's table; bands index it by row)
        aai::rotated_live_spans(aai::make_rot_launch(g, rq.mode, rq.policy), p.kernel == AAI_KERNEL_SAMPLE, spans);
        if (!spans.empty()) {
            // (no synchronisation of its own: `spans` lives until the stream has been synchronised at the end of the build)
            hipError_t e = hipMalloc((void **)&p.dLive, spans.size() * sizeof(int));
            if (e == hipSuccess) e = hipMemcpyAsync(p.dLive, spans.data(), spans.size() * sizeof(int), hipMemcpyHostToDevice, bs);
            if (e != hipSuccess) return hip_fail(e, "uploading the live tile spans");
        }
        stage("live tile spans");
    }
    const bool axisKernel = p.kernel == AAI_KERNEL_AXIS || p.kernel == AAI_KERNEL_AXIS_WIDE;
    // K1's separable model against the reference's classifier (aai_axis_verify.hpp).  Both policies: they differ in the
    // corner-triangle rule of a slanted left/right edge only, which does not exist at multiples of 90 degrees.
    const bool verifyAxis = axisKernel && axis_band_margin(rq) != 0;
    if (p.kernel == AAI_KERNEL_ROTATED || p.kernel == AAI_KERNEL_FAST || verifyAxis) {
        const aai::RotLaunch r = aai::make_rot_launch(g, rq.mode, rq.policy);
        const unsigned maxListed = max_listed_pixels();
        std::vector<std::pair<int, int>> hostPixels;
        bool hostDense = false;
        if (verifyAxis && aai::axis_verify_by_class(r, hostPixels, hostDense, maxListed)) {
            std::vector<uint2> hostList(hostPixels.size());
            for (size_t i = 0; i < hostPixels.size(); ++i) hostList[i] = make_uint2((unsigned)hostPixels[i].first, (unsigned)hostPixels[i].second);
            // exact arithmetic: one representative per (column class, row class) checked on the host
            p.dense = hostDense;
            p.flaggedPixels = (unsigned)hostList.size();
            if (!hostList.empty()) {
                hipError_t e = hipMalloc(&p.dList, hostList.size() * sizeof(uint2));
                if (e == hipSuccess) e = hipMemcpyAsync(p.dList, hostList.data(), hostList.size() * sizeof(uint2), hipMemcpyHostToDevice, bs);
                if (e == hipSuccess) e = hipStreamSynchronize(bs);
                if (e != hipSuccess) return hip_fail(e, "axis model scan");
            }
            stage("axis model check (host)");
            return AAI_OK;
        }
        // one-off scans of this geometry (rotated: aai_knife_scan_kernel, and the scan of the fp32 formulation that serves
        // it; axis-aligned: aai_axis_verify_kernel); keeps the list of flagged pixels only if there are any
        const size_t waves = aai::rotated_flag_words(r);
        unsigned count = 0;
        hipError_t e = hipSuccess;
        if (waves) {
            // ONE allocation: lane masks | tile flags (one bit per 16 x 16 tile) | the scans' counter / the list's cursor
            const unsigned tilesX = (unsigned)((g.dW + 15) / 16), tilesY = (unsigned)((g.dH + 15) / 16);
            const int tileFlagWords = (int)aai::tile_flag_row_words(tilesX);
            const size_t maskBytes = waves * sizeof(unsigned long long);
            const size_t tileBytes = ((size_t)tilesY * (size_t)tileFlagWords * sizeof(unsigned) + 15) & ~(size_t)15;
            char *block = nullptr;
            e = hipMalloc((void **)&block, maskBytes + tileBytes + 16);
            unsigned long long *dMasks = reinterpret_cast<unsigned long long *>(block);
            unsigned *dTiles = reinterpret_cast<unsigned *>(block + maskBytes), *dCount = reinterpret_cast<unsigned *>(block + maskBytes + tileBytes);
            // (the scans write every lane-mask word they own; tile flags and the counter start at zero)
            if (e == hipSuccess) e = hipMemsetAsync(dTiles, 0, tileBytes + 16, bs);
            if (e == hipSuccess) e = verifyAxis ? aai::launch_axis_verify(r, dMasks, dCount, bs) : aai::launch_knife_scan(r, dMasks, dCount, bs);
            if (e == hipSuccess && r.quad) e = form == aai::ROT_FORM_CELL ? aai::launch_cell_scan(r, dMasks, dCount, bs) : aai::launch_quad_scan(r, dMasks, dCount, bs);
            if (e == hipSuccess && r.wide && !verifyAxis) e = aai::launch_wide_scan(r, dMasks, dCount, bs);
            if (e == hipSuccess) e = hipMemcpyAsync(&count, dCount, sizeof(unsigned), hipMemcpyDeviceToHost, bs);
            if (e == hipSuccess) e = hipStreamSynchronize(bs);
            stage("scans");
            if (e == hipSuccess && count > maxListed) { p.dense = true; count = 0; }
            if (e == hipSuccess && count) {
                e = hipMalloc(&p.dList, (size_t)count * 2 * sizeof(unsigned));
                if (e == hipSuccess) e = hipMemsetAsync(dCount, 0, sizeof(unsigned), bs);
                if (e == hipSuccess) e = aai::launch_flag_list(dMasks, waves, tilesX, p.dList, dCount, count, bs);
                if (e == hipSuccess && (r.quad || r.wide)) {
                    // keep the masks: the fp32 kernel skips the flagged pixels (the fix-up pass runs beside it) and asks for the
                    // per-pixel masks only in tiles that hold a flagged pixel
                    p.dScan = block; p.dMasks = dMasks; p.dTileFlags = dTiles; p.tileFlagWords = tileFlagWords;
                    block = nullptr;
                    e = aai::launch_tile_flags(p.dMasks, tilesX, tilesY, p.dTileFlags, bs);
                }
                if (e == hipSuccess) e = hipStreamSynchronize(bs);
            }
            if (block) (void)hipFree(block);
            stage("flag list + tile flags");
        }
        if (e != hipSuccess) return hip_fail(e, verifyAxis ? "axis model scan" : "knife-edge scan");
        p.flaggedPixels = count;
    }
    return AAI_OK;
}

int rot_form(const aai_request &rq, const aai::Geometry &g, int channels, int srcType, int64_t srcStride)
{
    if (pick_kernel(rq, g) != AAI_KERNEL_ROTATED) return aai::ROT_FORM_QUAD;
    aai::RotLaunch r = aai::make_rot_launch(g, rq.mode, rq.policy);
    r.chan = channels;
    return aai::cell_can_serve(r, srcType, aai::ImageView{srcStride, 0}) ? aai::ROT_FORM_CELL : aai::ROT_FORM_QUAD;
}

int acquire_plan(const aai_request &rq, const aai::Geometry &g, int band0, int band1, int channels, int form, PlanRef *out, bool onCallerStream, hipStream_t stream)
{
    int dev = -1;
    AAI_HIP(hipGetDevice(&dev));
    const int kernel = pick_kernel(rq, g);
    if (kernel != AAI_KERNEL_ROTATED) form = aai::ROT_FORM_QUAD;
    if (kernel != AAI_KERNEL_AXIS && (band0 >= 0 || channels != 1)) {
        // Only K1's tables depend on the row band.  The per-pixel kernels take the band as launch parameters and their
        // one-off scans cover the whole image, so every band and every channel count of a rotated request shares one plan.
        band0 = band1 = -1; channels = 1;
    }
    PlanRef p;
    {
        std::lock_guard<std::mutex> lock(g_planMutex);
        std::list<PlanRef> &plans = plan_cache();
        for (auto it = plans.begin(); it != plans.end(); ++it) {
            const Plan &q = **it;
            if (q.device == dev && q.band0 == band0 && q.band1 == band1 && q.channels == channels && q.form == form && same_request(q.key, rq)) {
                plans.splice(plans.begin(), plans, it);
                p = plans.front();
                break;
            }
        }
        if (!p) {
            p = std::make_shared<Plan>();
            p->key = rq; p->band0 = band0; p->band1 = band1; p->channels = channels; p->form = form; p->device = dev; p->g = g; p->kernel = kernel;
            p->srcRow0 = 0; p->srcRow1 = g.H;
            plans.push_front(p);
            // the cache is sized per device: the least recently used plans of THIS device go first (a plan somebody is still
            // launching from lives on until its last reference is dropped)
            size_t mine = 0;
            for (const PlanRef &q : plans) mine += q->device == dev ? 1 : 0;
            for (auto it = plans.end(); mine > kMaxPlans && it != plans.begin();) {
                --it;
                if ((*it)->device == dev && *it != p) { it = plans.erase(it); --mine; }
            }
        }
    }
    {
        std::lock_guard<std::mutex> lock(p->build);
        if (!p->built) {
            const auto t0 = std::chrono::steady_clock::now();
            // where the build's kernels and copies go: the caller's stream when there is one to use (the resampling entry points;
            // not while it is being captured into a graph: the build synchronises), else the device pool's build stream
            hipStream_t bs = stream;
            bool own = onCallerStream;
            if (own) {
                hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
                if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
                if (cap != hipStreamCaptureStatusNone) own = false;
            }
            if (!own) {
                const hipError_t e = pool_build_stream(device_pool(dev), &bs);
                if (e != hipSuccess) { p->buildRc = hip_fail(e, "creating the build stream"); p->buildError = g_lastError; }
            }
            if (p->buildRc == AAI_OK) p->buildRc = build_plan(*p, bs);
            p->buildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            p->buildError = p->buildRc == AAI_OK ? std::string() : g_lastError;
            p->built = true;
        }
    }
    if (p->buildRc != AAI_OK) {
        std::lock_guard<std::mutex> lock(g_planMutex);
        plan_cache().remove(p);               // a later call tries again
        return fail(p->buildRc, p->buildError);
    }
    *out = p;
    return AAI_OK;
}

std::string plan_description(const aai_request &rq, int channels)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return std::string();
    std::lock_guard<std::mutex> lock(g_planMutex);
    for (const PlanRef &q : plan_cache()) {
        const Plan &p = *q;
        const bool rotated = p.kernel != AAI_KERNEL_AXIS && p.kernel != AAI_KERNEL_AXIS_WIDE;
        if (p.device == dev && p.band0 < 0 && (rotated || p.channels == channels) && p.built && same_request(p.key, rq)) {
            char buf[320];
            // (swap=0: the grid-order field stays in the format that bench.py, the tests and the recorded profiles read; new tokens go at the end)
            // order: the workgroup order K1 runs a plain fp32 image of this plan in (AxisShape::banded, aai_plan.hpp)
            bool banded = false;
            if (p.kernel == AAI_KERNEL_AXIS && p.channels == 1) {
                const aai::AxisLaunch a = make_axis_launch(p, 1, p.g.dW);
                banded = aai::axis_launch_shape(aai::AxisShapeFacts{a.nA, a.nB, a.nStrips, a.wide, a.maxRowSpan, a.rowsShared, a.maxOutputsPerStrip, a.transposed, a.tapStep,
                                                                    a.outStrideB, a.tuneRows, a.tuneNt, 4, 1}).banded != 0;
            }
            int len = snprintf(buf, sizeof buf, "kernel=%d rows=%d nt=%d swap=0 tune=%s order=%s flagged=%u dense=%d form=%s build_ms=%.3f adjoint=%s rot_adjoint=%s", p.kernel, p.tuneRows, p.tuneNt,
                     p.tuneSource == 1 ? "measured" : (p.tuneSource == 2 ? "cached" : "default"), banded ? "banded" : "launch", p.flaggedPixels, p.dense ? 1 : 0,
                     p.kernel == AAI_KERNEL_ROTATED ? (p.form == aai::ROT_FORM_CELL ? "cell" : "quad") : "-", p.buildMs, p.adjState == 1 ? "tables" : "none",
                     p.rotAdjState == 1 ? "sums" : (p.rotAdjState == 2 ? "general" : "none"));
            if (p.adjKnife >= 0 && len > 0 && len < (int)sizeof buf) snprintf(buf + len, sizeof buf - (size_t)len, " knife=%lld", p.adjKnife);
            return std::string(buf);
        }
    }
    return std::string();
}

// element offset into a typed source buffer
static const void *src_at(const void *base, int srcType, int64_t elements)
{
    return static_cast<const char *>(base) + elements * (int64_t)aai::src_elem_size(srcType);
}

int enqueue(const aai_request &rq, const aai::Geometry &g, int batch, const void *dSrc, int srcType, int64_t srcStride, int64_t srcImageStride,
            float *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream, int band0, int band1, int channels)
{
    PlanRef p;
    const int rc = acquire_plan(rq, g, band0, band1, channels, rot_form(rq, g, channels, srcType, srcStride), &p, /*onCallerStream*/ true, stream);
    if (rc != AAI_OK) return rc;
    // launches only enqueue; the plan's side stream and fork / join events are shared by its callers, hence the plan's lock
    std::lock_guard<std::mutex> lock(p->launch);
    // strides are in elements; an interleaved pixel takes `channels` of them
    if (srcStride < (int64_t)g.W * channels) return fail(AAI_ERR_BAD_ARGUMENT, "Source stride smaller than the image width.");
    if (dstStride < (int64_t)g.dW * channels) return fail(AAI_ERR_BAD_ARGUMENT, "Destination stride smaller than the output width.");
    if (g.dW == 0 || g.dH == 0 || batch == 0) return AAI_OK;

    aai::ImageView sv{srcStride, srcImageStride}, dv{dstStride, dstImageStride};
    const char *name = "";
    hipError_t e;
    const bool axisKernel = p->kernel == AAI_KERNEL_AXIS || p->kernel == AAI_KERNEL_AXIS_WIDE;
    // per-pixel launch description: the rotated kernels, and the fix-up pass behind K1
    aai::RotLaunch r = aai::make_rot_launch(g, rq.mode, rq.policy);
    if (band0 >= 0) {
        int srcRow0 = p->srcRow0, srcRow1 = p->srcRow1;
        if (!axisKernel) aai::rotated_band_source_rows(g, band0, band1, p->kernel == AAI_KERNEL_SAMPLE, srcRow0, srcRow1);
        r.dyBase = band0; r.dyEnd = band1; r.srcRow0 = srcRow0; r.srcRow1 = srcRow1;
    }
    r.chan = channels;
    if (axisKernel && !p->dense) {
        const aai::AxisLaunch a = make_axis_launch(*p, channels, dstStride);
        e = hipSuccess;
        for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridZ) {      // grid.z carries the batch
            const void *s0 = src_at(dSrc, srcType, (int64_t)b0 * srcImageStride);
            float *d0 = dDst + (int64_t)b0 * dstImageStride;
            const int nb = std::min(batch - b0, kMaxGridZ);
            e = aai::launch_axis(a, s0, srcType, sv, d0, dv, nb, stream, &name);
            // dst rows and columns off the image: 0 whatever the source holds (K1 multiplies a parked window by weights of 0).
            // Integer sources have no value whose product with 0 is not 0.
            if (srcType == aai::SRC_F32) {
                for (size_t i = 0; i < p->tabs.emptyRow.size() && e == hipSuccess; ++i)
                    e = aai::launch_axis_zero(a, 0, a.nA, p->tabs.emptyRow[i].k0, p->tabs.emptyRow[i].k1, d0, dv, nb, stream);
                for (size_t i = 0; i < p->tabs.emptyLane.size() && e == hipSuccess; ++i)
                    e = aai::launch_axis_zero(a, p->tabs.emptyLane[i].k0, p->tabs.emptyLane[i].k1, 0, a.nB, d0, dv, nb, stream);
            }
            // dst pixels where the reference's classifier departs from the separable model (aai_axis_verify.hpp)
            if (e == hipSuccess && p->flaggedPixels) {
                aai::launch_rotated_fixup(r, nb, s0, srcType, sv, d0, dv, static_cast<const uint2 *>(p->dList), p->flaggedPixels, stream);
                e = hipGetLastError();
            }
        }
    } else {
        // (an axis-aligned geometry lands here when the separable model fails for most of its pixels: `dense`)
        const aai::QuadMap qm = aai::make_quad_map(g, srcStride, r.srcRow0, channels, aai::src_elem_size(srcType));
        aai::RotFlags flags;
        flags.list = p->dList; flags.count = p->flaggedPixels; flags.dense = p->dense;
        flags.masks = p->dMasks; flags.tileFlags = p->dTileFlags; flags.tileFlagWords = p->tileFlagWords; flags.live = p->dLive; flags.form = p->form;
        // A production kernel that skips the plan's listed pixels has the fix-up pass BESIDE it on a side stream of the device's
        // pool (fork / join events; the pool's lock is held while the launch is enqueued).  The pool's side streams are created by
        // the second such launch of the process: until then -- for the one call the reference's user makes -- the pass runs behind
        // the production kernel on the caller's stream, which then computes the listed pixels too and has them overwritten.
        DevicePool &pool = device_pool(p->device);
        std::unique_lock<std::mutex> poolLock(pool.m, std::defer_lock);
        if (p->flaggedPixels && p->dMasks && !p->dense) {
            poolLock.lock();
            if (!pool.sideReady && !pool.sideFailed && ++pool.besideLaunches >= 2) pool_create_sides(pool);
            if (pool.sideReady) {
                const unsigned slot = pool.nextSide++ % DevicePool::kSideSlots;
                flags.side = pool.side[slot]; flags.fork = pool.fork[slot]; flags.join = pool.join[slot];
            } else poolLock.unlock();
        }
        e = hipSuccess;
        for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridZ)
            e = aai::launch_rotated(r, qm, src_at(dSrc, srcType, (int64_t)b0 * srcImageStride), srcType, sv, dDst + (int64_t)b0 * dstImageStride, dv,
                                    std::min(batch - b0, kMaxGridZ), flags, stream, &name);
    }
    g_lastKernel = name;
    if (e != hipSuccess) return hip_fail(e, name);
    return AAI_OK;
}

// the adjoint's scratch pool of a device, created on first need
static int adjoint_scratch_pool(int device, hipMemPool_t *out)
{
    DevicePool &pool = device_pool(device);
    std::lock_guard<std::mutex> lock(pool.m);
    if (!pool.scratch) {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = device;
        AAI_HIP(hipMemPoolCreate(&pool.scratch, &props));
        uint64_t keep = UINT64_MAX;
        const hipError_t ea = hipMemPoolSetAttribute(pool.scratch, hipMemPoolAttrReleaseThreshold, &keep);
        if (ea != hipSuccess) { (void)hipMemPoolDestroy(pool.scratch); pool.scratch = nullptr; return hip_fail(ea, "hipMemPoolSetAttribute"); }
    }
    *out = pool.scratch;
    return AAI_OK;
}

// The scratch and the chunk loop of every adjoint family: fp64 scratch of imageBytes per image in flight from the device's pool
// (stream-ordered: hipMallocFromPoolAsync / hipFreeAsync on `stream`; imageBytes == 0: none, n == nullptr), the batch in chunks of
// chunk_images(), and launch(nb, gd, gs, n) -> hipError_t for the nb images of a chunk at gd / gs.  A launch error is reported under
// `name`, which the launchers may set; the scratch is freed whatever the launches returned.  aai_last_kernel(): name, "+listed" appended.
// T: the images' element type (float: every fp32 family; double: the reference-precision adjoint, enqueue_f64_adjoint), deduced.
template <typename T, typename Launch>
static int for_each_adjoint_chunk(int batch, const T *dGdst, int64_t dstImageStride, T *dGsrc, int64_t srcImageStride, size_t imageBytes,
                                  int device, hipStream_t stream, const char *&name, bool listed, Launch launch)
{
    const int chunk = chunk_images(batch, imageBytes);
    double *n = nullptr;
    if (imageBytes) {
        hipMemPool_t scratch = nullptr;
        const int rc = adjoint_scratch_pool(device, &scratch);
        if (rc != AAI_OK) return rc;
        AAI_HIP(hipMallocFromPoolAsync((void **)&n, imageBytes * (size_t)chunk, scratch, stream));
    }
    hipError_t e = hipSuccess;
    for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += chunk)
        e = launch(std::min(batch - b0, chunk), dGdst + (int64_t)b0 * dstImageStride, dGsrc + (int64_t)b0 * srcImageStride, n);
    const hipError_t ef = n ? hipFreeAsync(n, stream) : hipSuccess;
    g_lastKernel = listed ? std::string(name) + "+listed" : std::string(name);
    if (e != hipSuccess) return hip_fail(e, name);
    if (ef != hipSuccess) return hip_fail(ef, "hipFreeAsync");
    return AAI_OK;
}

// The adjoint tables of an axis plan (Plan::adjState): the inverse ranges of its two tables and, where it has flagged pixels, the
// lists of the correction pass.  Under p.build; blocks (uploads on the device pool's build stream, the flagged list read back).
static int build_adjoint_tables(Plan &p)
{
    if (p.adjState) return AAI_OK;
    if (p.kernel != AAI_KERNEL_AXIS || p.dense || p.channels != 1 || p.band0 >= 0) { p.adjState = 2; return AAI_OK; }
    const aai::Geometry &g = p.g;
    std::vector<aai::AxisRange> cols, rows;
    if (!aai::build_axis_adjoint_ranges(p.tabs, g.W, g.H, cols, rows)) { p.adjState = 2; return AAI_OK; }
    hipStream_t bs = nullptr;
    AAI_HIP(pool_build_stream(device_pool(p.device), &bs));
    std::vector<std::pair<int, int>> srcList, dstList, flagged;
    std::vector<int> grazedCols, grazedRows;
    aai::axis_grazed_indices(p.tabs.lane, grazedCols);
    aai::axis_grazed_indices(p.tabs.row, grazedRows);
    if (p.flaggedPixels) {
        std::vector<uint2> flaggedDev(p.flaggedPixels);
        AAI_HIP(hipMemcpyAsync(flaggedDev.data(), p.dList, flaggedDev.size() * sizeof(uint2), hipMemcpyDeviceToHost, bs));
        AAI_HIP(hipStreamSynchronize(bs));
        flagged.resize(flaggedDev.size());
        for (size_t i = 0; i < flaggedDev.size(); ++i) flagged[i] = std::make_pair((int)flaggedDev[i].x, (int)flaggedDev[i].y);
    }
    if (!flagged.empty() || !grazedCols.empty() || !grazedRows.empty()) {
        // (a correction pass over more than half of the source image is the general adjoint with a detour)
        const aai::RotLaunch r = aai::make_rot_launch(g, p.key.mode, p.key.policy);
        if (!aai::build_adjoint_lists(r, flagged, grazedCols, grazedRows, (size_t)g.W * g.H / 2, srcList, dstList)) { p.adjState = 2; return AAI_OK; }
    }
    std::vector<uint2> src2(srcList.size()), dst2(dstList.size());
    for (size_t i = 0; i < srcList.size(); ++i) src2[i] = make_uint2((unsigned)srcList[i].first, (unsigned)srcList[i].second);
    for (size_t i = 0; i < dstList.size(); ++i) dst2[i] = make_uint2((unsigned)dstList[i].first, (unsigned)dstList[i].second);
    auto upload = [&](const void *h, size_t bytes, void **d) -> hipError_t {
        if (!bytes) { *d = nullptr; return hipSuccess; }
        hipError_t e = hipMalloc(d, bytes);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, bs);      // (the host vectors outlive the copy: synchronised below)
    };
    hipError_t e = upload(cols.data(), cols.size() * sizeof(aai::AxisRange), (void **)&p.dColRange);
    if (e == hipSuccess) e = upload(rows.data(), rows.size() * sizeof(aai::AxisRange), (void **)&p.dRowRange);
    if (e == hipSuccess) e = upload(src2.data(), src2.size() * sizeof(uint2), &p.dAdjSrcList);
    if (e == hipSuccess) e = upload(dst2.data(), dst2.size() * sizeof(uint2), &p.dAdjDstList);
    const hipError_t es = hipStreamSynchronize(bs);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        for (void **d : {(void **)&p.dColRange, (void **)&p.dRowRange, &p.dAdjSrcList, &p.dAdjDstList})
            if (*d) { (void)hipFree(*d); *d = nullptr; }
        return hip_fail(e, "uploading the adjoint tables");             // (adjState stays 0: a later call tries again)
    }
    p.adjSrcCount = (unsigned)src2.size(); p.adjDstCount = (unsigned)dst2.size();
    p.adjState = 1;
    return AAI_OK;
}

// The tables of the planned adjoint at general rotations (Plan::rotAdjState): the sums of every dst pixel, the dst pixels with a knife-edge
// pair and, from those, the source pixels the general gather recomputes.  Under p.build; blocks (the one-off kernels on the device
// pool's build stream, the knife list read back, the source list uploaded).
static int build_rot_adjoint_tables(Plan &p)
{
    if (p.rotAdjState) return AAI_OK;
    const aai::Geometry &g = p.g;
    const size_t pixels = (size_t)g.dW * (size_t)g.dH;
    if ((p.kernel != AAI_KERNEL_ROTATED && p.kernel != AAI_KERNEL_FAST) || p.channels != 1 || p.band0 >= 0 || !pixels ||
        pixels * sizeof(double) > ((size_t)1 << 30)) {
        p.rotAdjState = 2;
        return AAI_OK;
    }
    const aai::RotLaunch r = aai::make_rot_launch(g, p.key.mode, p.key.policy);
    hipStream_t bs = nullptr;
    AAI_HIP(pool_build_stream(device_pool(p.device), &bs));
    // ONE scratch allocation: a byte per dst pixel | the count of flagged pixels | the list's cursor
    const size_t flagBytes = (pixels + 15) & ~(size_t)15;
    double *dSums = nullptr;
    char *block = nullptr;
    void *dKnife = nullptr, *dSrc = nullptr;
    std::vector<uint2> knife, src2;                                  // (declared before the first copy: alive until the stream is synchronised)
    unsigned count = 0;
    bool general = false;
    hipError_t e = hipMalloc((void **)&dSums, pixels * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&block, flagBytes + 16);
    unsigned *dCount = reinterpret_cast<unsigned *>(block + flagBytes), *dCursor = dCount + 1;
    if (e == hipSuccess) e = hipMemsetAsync(dCount, 0, 16, bs);
    if (e == hipSuccess) e = aai::launch_adjoint_sums(r, dSums, reinterpret_cast<unsigned char *>(block), dCount, bs);
    if (e == hipSuccess) e = hipMemcpyAsync(&count, dCount, sizeof(unsigned), hipMemcpyDeviceToHost, bs);
    if (e == hipSuccess) e = hipStreamSynchronize(bs);
    if (e == hipSuccess && count > max_listed_pixels()) general = true;
    if (e == hipSuccess && count && !general) {
        knife.resize(count);
        e = hipMalloc(&dKnife, (size_t)count * sizeof(uint2));
        if (e == hipSuccess) e = aai::launch_adjoint_knife_list(r, reinterpret_cast<const unsigned char *>(block), static_cast<uint2 *>(dKnife), dCursor, count, bs);
        if (e == hipSuccess) e = hipMemcpyAsync(knife.data(), dKnife, (size_t)count * sizeof(uint2), hipMemcpyDeviceToHost, bs);
        if (e == hipSuccess) e = hipStreamSynchronize(bs);
        if (e == hipSuccess) {
            std::vector<std::pair<int, int>> flagged(knife.size()), srcList, dstList;
            for (size_t i = 0; i < knife.size(); ++i) flagged[i] = std::make_pair((int)knife[i].x, (int)knife[i].y);
            // (a correction pass over more than half of the source image is the general adjoint with a detour; n is complete here, so
            // the list of dst pixels is not needed)
            if (!aai::build_adjoint_lists(r, flagged, std::vector<int>(), std::vector<int>(), (size_t)g.W * g.H / 2, srcList, dstList)) general = true;
            else {
                src2.resize(srcList.size());
                for (size_t i = 0; i < srcList.size(); ++i) src2[i] = make_uint2((unsigned)srcList[i].first, (unsigned)srcList[i].second);
                if (!src2.empty()) {
                    e = hipMalloc(&dSrc, src2.size() * sizeof(uint2));
                    if (e == hipSuccess) e = hipMemcpyAsync(dSrc, src2.data(), src2.size() * sizeof(uint2), hipMemcpyHostToDevice, bs);
                }
            }
        }
    }
    const hipError_t es = hipStreamSynchronize(bs);
    if (e == hipSuccess) e = es;
    if (block) (void)hipFree(block);
    if (dKnife) (void)hipFree(dKnife);
    if (e != hipSuccess || general) {
        if (dSums) (void)hipFree(dSums);
        if (dSrc) (void)hipFree(dSrc);
        if (e != hipSuccess) return hip_fail(e, "building the rotated adjoint tables");      // (rotAdjState stays 0: a later call tries again)
        p.adjKnife = (long long)count;
        p.rotAdjState = 2;
        return AAI_OK;
    }
    p.dAdjSums = dSums;
    p.dAdjSrcList = dSrc; p.adjSrcCount = (unsigned)src2.size();
    p.adjKnife = (long long)count;
    p.rotAdjState = 1;
    return AAI_OK;
}

// the forward's single-channel plan (the forward's key: a packed fp32 image, the whole image) with its rotated-adjoint tables, which
// do not depend on the channel count: every channel count shares them
static int acquire_rot_adjoint_plan(const aai_request &rq, const Geometry &g, bool prepareOnly, hipStream_t stream, PlanRef *out)
{
    const int rc = acquire_plan(rq, g, -1, -1, 1, rot_form(rq, g, 1, aai::SRC_F32, g.W), out, /*onCallerStream*/ !prepareOnly, stream);
    if (rc != AAI_OK) return rc;
    std::lock_guard<std::mutex> lock((*out)->build);
    return build_rot_adjoint_tables(**out);
}

// the argument block of the transposed separable kernels for a single-channel plan with its adjoint tables, a channel count and a dst row
// stride (elements): the forward's mapping (make_axis_launch) of (ka, kb) onto the first element of a dst PIXEL of `channels` elements
static aai::AxisAdjointLaunch make_axis_adjoint_launch(const Plan &p, int channels, int64_t dstStride)
{
    const aai::AxisTables &t = p.tabs;
    const int64_t sa = t.transposed ? dstStride : channels, sb = t.transposed ? channels : dstStride;
    aai::AxisAdjointLaunch a{};
    a.laneTab = p.dLane; a.rowTab = p.dRow; a.colRange = p.dColRange; a.rowRange = p.dRowRange;
    a.srcW = p.g.W; a.srcH = p.g.H;
    a.outStrideA = t.flipA ? -sa : sa;
    a.outStrideB = t.flipB ? -sb : sb;
    a.outBase = (t.flipA ? (int64_t)(t.nA - 1) * sa : 0) + (t.flipB ? (int64_t)(t.nB - 1) * sb : 0);
    return a;
}

int enqueue_adjoint(AdjointFamily family, const aai_request &rq, const Geometry &g, int batch, int channels, const float *dGdst, int64_t dstStride,
                    int64_t dstImageStride, float *dGsrc, int64_t srcStride, int64_t srcImageStride, hipStream_t stream)
{
    const bool prepareOnly = dGdst == nullptr;
    // ---- the routing table (aai_engine.hpp): what the entry asked for -> the family whose launches serve the call
    const int kernel = pick_kernel(rq, g);
    // (SAMPLE -- the samplers' adjoint -- is never rerouted: none of the tests below names it)
    // (SEPARABLE is the one entry that asks for the interleaved transposed separable kernel; everywhere else it is ROTATED, line for line)
    if (family == ADJOINT_SEPARABLE && (channels == 1 || kernel != AAI_KERNEL_AXIS)) family = ADJOINT_ROTATED;
    if (family == ADJOINT_ROTATED && kernel != AAI_KERNEL_ROTATED && kernel != AAI_KERNEL_FAST)      // reduced angle 0
        family = channels == 1 ? ADJOINT_PLANNED : ADJOINT_GENERAL;
    if (family == ADJOINT_PLANNED && (kernel != AAI_KERNEL_AXIS || channels != 1)) family = ADJOINT_GENERAL;
    PlanRef p;
    if (family == ADJOINT_PLANNED || family == ADJOINT_SEPARABLE) {
        // the forward's plan under the forward's key (a packed fp32 image, one channel, the whole image): its adjoint tables know pixels,
        // not channels, and serve every channel count
        const int rc = acquire_plan(rq, g, -1, -1, 1, aai::ROT_FORM_QUAD, &p, /*onCallerStream*/ !prepareOnly, stream);
        if (rc != AAI_OK) return rc;
        std::lock_guard<std::mutex> lock(p->build);
        const int rt = build_adjoint_tables(*p);
        if (rt != AAI_OK) return rt;
        if (p->adjState != 1) family = ADJOINT_GENERAL;          // a wide or dense plan, tables the inversion refuses
    } else if (family == ADJOINT_ROTATED) {
        const int rc = acquire_rot_adjoint_plan(rq, g, prepareOnly, stream, &p);
        if (rc != AAI_OK) return rc;
        if (p->rotAdjState != 1) family = ADJOINT_GENERAL;       // rotAdjState 2
    }
    if (prepareOnly) return AAI_OK;

    // ---- the launches.  A plan's launches are serialised between caller threads; the general family has no plan.
    int device = 0;
    std::unique_lock<std::mutex> lock;
    if (family == ADJOINT_GENERAL || family == ADJOINT_SAMPLE) AAI_HIP(hipGetDevice(&device));
    else { device = p->device; lock = std::unique_lock<std::mutex>(p->launch); }
    const aai::ImageView dv{dstStride, dstImageStride}, sv{srcStride, srcImageStride};
    // scratch: one fp64 image of the dst size times the channels per image in flight
    size_t imageBytes = (size_t)g.dW * (size_t)g.dH * (size_t)channels * sizeof(double);
    const char *name = "";
    bool listed = false;                 // the plan has lists for a pass of the general kernels behind its own
    aai::AxisAdjointLaunch a{};
    if (family == ADJOINT_PLANNED || family == ADJOINT_SEPARABLE) {
        // (ka, kb) -> the first element of a dst PIXEL: the forward's mapping (make_axis_launch) with a pixel of `channels` elements.  Not
        // make_axis_launch(*p, channels, ...): that divides the plan's nA by the channel count, and this plan's nA is in pixels already.
        a = make_axis_adjoint_launch(*p, channels, dstStride);
        name = "aai_axis_adjoint_kernel";            // (SEPARABLE: its launcher names the instantiation)
        listed = p->adjSrcCount != 0 && p->adjDstCount != 0;
        if (!listed) imageBytes = 0;     // the transposed separable kernels need no scratch, only the correction pass does
    } else if (family == ADJOINT_ROTATED) listed = p->adjSrcCount != 0;
    else if (family == ADJOINT_SAMPLE) imageBytes = 0;      // one gather, no scratch
    // (AAI_POLICY_DOUBLE_PRECISION / AAI_POLICY_PREFER_CELL choose between forward kernels; the adjoint has one, in double precision)
    const aai::RotLaunch r = (family != ADJOINT_PLANNED && family != ADJOINT_SEPARABLE) || listed ? aai::make_rot_launch(g, rq.mode, rq.policy) : aai::RotLaunch{};
    const uint2 *srcList = p ? static_cast<const uint2 *>(p->dAdjSrcList) : nullptr, *dstList = p ? static_cast<const uint2 *>(p->dAdjDstList) : nullptr;
    auto launch = [&](int nb, const float *gd, float *gs, double *n) -> hipError_t {
        hipError_t e = hipSuccess;
        switch (family) {
        case ADJOINT_GENERAL:
            return channels == 1 ? aai::launch_adjoint(r, nb, gd, dv, n, gs, sv, stream, &name)
                                 : aai::launch_adjoint_multi(r, channels, nb, gd, dv, n, gs, sv, stream, &name);
        case ADJOINT_PLANNED:
            e = aai::launch_axis_adjoint(a, nb, gd, dv, gs, sv, stream, nullptr);
            if (e == hipSuccess && listed) e = aai::launch_adjoint_listed(r, nb, gd, dv, n, gs, sv, dstList, p->adjDstCount, srcList, p->adjSrcCount, stream);
            return e;
        case ADJOINT_SEPARABLE:
            e = aai::launch_axis_adjoint_multi(a, channels, nb, gd, dv, gs, sv, stream, &name);
            if (e == hipSuccess && listed)
                e = aai::launch_adjoint_listed_multi(r, channels, nb, gd, dv, n, gs, sv, dstList, p->adjDstCount, srcList, p->adjSrcCount, stream);
            return e;
        case ADJOINT_SAMPLE:
            return channels == 1 ? aai::launch_adjoint_sample(r, nb, gd, dv, gs, sv, stream, &name)
                                 : aai::launch_adjoint_sample_multi(r, channels, nb, gd, dv, gs, sv, stream, &name);
        case ADJOINT_ROTATED:
            if (channels != 1) return aai::launch_adjoint_plain_multi(r, channels, nb, gd, dv, p->dAdjSums, n, gs, sv, srcList, p->adjSrcCount, stream, &name);
            e = aai::launch_adjoint_plain(r, nb, gd, dv, p->dAdjSums, n, gs, sv, stream, &name);
            if (e == hipSuccess && listed) e = aai::launch_adjoint_gather_listed(r, nb, n, gs, sv, srcList, p->adjSrcCount, stream);
            return e;
        }
        return e;
    };
    return for_each_adjoint_chunk(batch, dGdst, dstImageStride, dGsrc, srcImageStride, imageBytes, device, stream, name, listed, launch);
}

// ---- the reference-precision path (include/aai_f64.h, aai_f64.hip): no plan, no lock, nothing blocks
int enqueue_f64_forward(const aai_request &rq, const Geometry &g, int batch, const double *dSrc, int64_t srcStride, int64_t srcImageStride, double *dDst,
                        int64_t dstStride, int64_t dstImageStride, hipStream_t stream)
{
    const aai::RotLaunch r = aai::make_rot_launch(g, rq.mode, rq.policy);
    const aai::ImageView sv{srcStride, srcImageStride}, dv{dstStride, dstImageStride};
    const char *name = "";
    hipError_t e = hipSuccess;
    for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridZ)
        e = aai::launch_f64_forward(r, std::min(batch - b0, kMaxGridZ), dSrc + (int64_t)b0 * srcImageStride, sv, dDst + (int64_t)b0 * dstImageStride, dv,
                                    stream, &name);
    g_lastKernel = name;
    if (e != hipSuccess) return hip_fail(e, name);
    return AAI_OK;
}

int enqueue_f64_adjoint(const aai_request &rq, const Geometry &g, int batch, const double *dGdst, int64_t dstStride, int64_t dstImageStride, double *dGsrc,
                        int64_t srcStride, int64_t srcImageStride, hipStream_t stream)
{
    int device = 0;
    AAI_HIP(hipGetDevice(&device));
    const aai::RotLaunch r = aai::make_rot_launch(g, rq.mode, rq.policy);
    const aai::ImageView dv{dstStride, dstImageStride}, sv{srcStride, srcImageStride};
    const size_t imageBytes = (size_t)g.dW * (size_t)g.dH * sizeof(double);      // pass 1's image, per image in flight
    const char *name = "";
    auto launch = [&](int nb, const double *gd, double *gs, double *n) -> hipError_t { return aai::launch_f64_adjoint(r, nb, gd, dv, n, gs, sv, stream, &name); };
    return for_each_adjoint_chunk(batch, dGdst, dstImageStride, dGsrc, srcImageStride, imageBytes, device, stream, name, false, launch);
}

// ---- forwarding a narrow-element call through dense fp32 scratch: the second route of enqueue_narrow and enqueue_adjoint_half
// One side of it: the caller's images of raw `type` elements (view: strides in elements) and the shape of their dense fp32 twins.
struct NarrowSide {
    const void *p;
    aai::ImageView view;
    int64_t row;      // elements per dense row
    int rows;
    size_t count() const { return (size_t)row * (size_t)rows; }
    const char *image(int type, int b) const { return static_cast<const char *>(p) + (int64_t)b * view.imageStride * (int64_t)aai::narrow_elem_size(type); }
};
// Per chunk of chunk_images(): (widen: `in` widened into scratch,) inner(nb, in32, out32) -> int, the fp32 entry's launches on dense
// images (image b of the chunk at b * in.count() / b * out.count(); !widen: in32 is the caller's own image, which that entry reads),
// and one conversion of out32 into `out`.  The scratch is stream-ordered from `device`'s pool: all of a chunk's widened inputs, each
// rounded up to 256 bytes, then all its outputs.  aai_last_kernel(): what inner() left there, `suffix` appended.  A failed inner()
// keeps its error text, whatever the free says; a failed launch is reported under its kernel's name.
// `store(nb, out32, b0) -> hipError_t` is that conversion for the nb images from image b0 on, reported as `storeName` when it fails.
template <typename Inner, typename Store>
static int through_fp32_scratch_into(int type, bool widen, const NarrowSide &in, const NarrowSide &out, int batch, int device, const char *suffix,
                                     hipStream_t stream, const char *storeName, Inner inner, Store store)
{
    const size_t inBytes = widen ? (in.count() * sizeof(float) + 255) & ~(size_t)255 : 0, outBytes = (out.count() * sizeof(float) + 255) & ~(size_t)255;
    const int chunk = chunk_images(batch, inBytes + outBytes);
    hipMemPool_t pool = nullptr;
    const int rp = adjoint_scratch_pool(device, &pool);
    if (rp != AAI_OK) return rp;
    char *scratch = nullptr;
    AAI_HIP(hipMallocFromPoolAsync((void **)&scratch, (inBytes + outBytes) * (size_t)chunk, pool, stream));
    float *in32 = reinterpret_cast<float *>(scratch), *out32 = reinterpret_cast<float *>(scratch + inBytes * (size_t)chunk);
    const char *what = storeName;
    hipError_t e = hipSuccess;
    int rl = AAI_OK;
    for (int b0 = 0; b0 < batch && e == hipSuccess && rl == AAI_OK; b0 += chunk) {
        const int nb = std::min(batch - b0, chunk);
        if (widen) {
            what = "aai_half_widen_kernel";
            if (in.count()) e = aai::launch_narrow_widen(type, in.image(type, b0), in.view, in32, (int)in.row, in.rows, nb, stream);
            if (e != hipSuccess) break;
        }
        rl = inner(nb, widen ? (const void *)in32 : (const void *)in.image(type, b0), out32);
        if (rl != AAI_OK) break;
        what = storeName;
        e = store(nb, out32, b0);
    }
    const std::string lastError = g_lastError;      // (of a failed inner(): hipFreeAsync below must not replace it)
    const hipError_t ef = hipFreeAsync(scratch, stream);
    if (rl != AAI_OK) return fail(rl, lastError);
    g_lastKernel += suffix;
    if (e != hipSuccess) return hip_fail(e, what);
    if (ef != hipSuccess) return hip_fail(ef, "hipFreeAsync");
    return AAI_OK;
}

// ... with the element type's own conversion into `out`: half_narrow or int_quantize
template <typename Inner>
static int through_fp32_scratch(int type, bool widen, const NarrowSide &in, const NarrowSide &out, int batch, int device, const char *suffix,
                                hipStream_t stream, Inner inner)
{
    return through_fp32_scratch_into(type, widen, in, out, batch, device, suffix, stream, aai::narrow_is_half(type) ? "aai_half_narrow_kernel" : "aai_int_quantize_kernel",
                                     inner, [&](int nb, const float *out32, int b0) {
                                         return aai::launch_narrow_store(type, out32, const_cast<char *>(out.image(type, b0)), out.view, (int)out.row, out.rows, nb, stream);
                                     });
}

// ---- the narrow-element paths (include/aai_half.h, include/aai_half_interleaved.h, include/aai_int.h; aai_axis_narrow.hip)
// `type`: aai::NarrowType.  `srcType` is what enqueue() reads on the forwarding route and what keys the plan: the caller's u8 / u16
// image itself, or the dense fp32 scratch a half image is widened into.
static int enqueue_narrow(const aai_request &rq, const Geometry &g, int batch, int channels, int type, const void *dSrc, int64_t srcStride,
                          int64_t srcImageStride, void *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream)
{
    if (g.dW == 0 || g.dH == 0 || batch == 0) return AAI_OK;
    const bool half = aai::narrow_is_half(type);
    const int srcType = half ? aai::SRC_F32 : type == aai::NARROW_U8 ? aai::SRC_U8 : aai::SRC_U16;
    const int64_t rowSrc = (int64_t)g.W * channels, rowDst = (int64_t)g.dW * channels;
    const size_t nSrc = (size_t)rowSrc * (size_t)g.H, nDst = (size_t)rowDst * (size_t)g.dH;
    const int64_t inStride = half ? rowSrc : srcStride, inImageStride = half ? (int64_t)nSrc : srcImageStride;      // of enqueue()'s source
    // the forward's plan under (request, channels): the one the forwarding route's enqueue() takes, and aai_prepare(req, channels) builds
    PlanRef p;
    const int rc = acquire_plan(rq, g, -1, -1, channels, rot_form(rq, g, channels, srcType, inStride), &p, /*onCallerStream*/ true, stream);
    if (rc != AAI_OK) return rc;
    const int64_t elem = (int64_t)aai::narrow_elem_size(type);
    const char *src = static_cast<const char *>(dSrc);
    char *dst = static_cast<char *>(dDst);
    const aai::ImageView sv{srcStride, srcImageStride}, dv{dstStride, dstImageStride};
    hipError_t e = hipSuccess;
    if (p->kernel == AAI_KERNEL_AXIS && !p->dense && p->flaggedPixels == 0 && (half || rq.mode == AAI_MODE_AREA || rq.mode == AAI_MODE_FAST)) {
        // (the tables and the launch block are read-only here: no side stream, no event, hence no lock)
        const aai::AxisLaunch a = make_axis_launch(*p, channels, dstStride);
        if (aai::axis_narrow_can_serve(a, type)) {
            const char *name = "";
            for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridZ)
                e = aai::launch_axis_narrow(a, type, src + (int64_t)b0 * srcImageStride * elem, sv, dst + (int64_t)b0 * dstImageStride * elem, dv,
                                            std::min(batch - b0, kMaxGridZ), stream, &name);
            g_lastKernel = name;
            if (e != hipSuccess) return hip_fail(e, name);
            return AAI_OK;
        }
    }
    // forwarding: (half: widen,) the fp32 entry's launches into dense fp32 scratch, one conversion -- the bits of
    // narrow(fp32 entry(widen(src))) and of quantize(fp32 entry(src))
    const NarrowSide in{dSrc, sv, rowSrc, g.H}, out{dDst, dv, rowDst, g.dH};
    return through_fp32_scratch(type, half, in, out, batch, p->device, half ? "+widened" : "+quantized", stream, [&](int nb, const void *in32, float *out32) {
        return enqueue(rq, g, nb, in32, srcType, inStride, inImageStride, out32, rowDst, (int64_t)nDst, stream, -1, -1, channels);
    });
}

// ---- the half-precision adjoint (include/aai_adjoint_half.h; aai_axis_adjoint_narrow.hip): routes in aai_engine.hpp
int enqueue_adjoint_half(const aai_request &rq, const Geometry &g, int batch, int channels, int halfType, const void *dGdst, int64_t dstStride,
                         int64_t dstImageStride, void *dGsrc, int64_t srcStride, int64_t srcImageStride, hipStream_t stream)
{
    const int type = halfType == AAI_HALF_F16 ? aai::NARROW_F16 : aai::NARROW_BF16;
    const char *gd = static_cast<const char *>(dGdst);
    char *gs = static_cast<char *>(dGsrc);
    const int64_t elem = (int64_t)aai::narrow_elem_size(type);
    const aai::ImageView dv{dstStride, dstImageStride}, sv{srcStride, srcImageStride};
    if (pick_kernel(rq, g) == AAI_KERNEL_AXIS) {
        // the forward's single-channel plan with the adjoint tables of PLANNED / SEPARABLE: what enqueue_adjoint acquires for them, and
        // what aai_adjoint_rotated_prepare builds
        PlanRef p;
        const int rc = acquire_plan(rq, g, -1, -1, 1, aai::ROT_FORM_QUAD, &p, /*onCallerStream*/ true, stream);
        if (rc != AAI_OK) return rc;
        {
            std::lock_guard<std::mutex> lock(p->build);
            const int rt = build_adjoint_tables(*p);
            if (rt != AAI_OK) return rt;
        }
        // DIRECT: the tables are there, the plan has no lists for a correction pass, and the request is of a class whose direct launch
        // was measured faster than the forwarding route's stages (profiles/adjoint_half_time.txt: every class but one -- a single
        // channel, up-sampling, at 90 / 270 degrees, where the kernel is bound by its strided 2-byte gdst loads and gains nothing over the
        // fp32 kernel: 187 against 184 us for 2048^2 <- 4096^2).  Tables and launch block are read-only here: no scratch, no side stream,
        // no event, hence no lock.
        const bool loses = channels == 1 && p->tabs.transposed && (int64_t)g.dW * g.dH > (int64_t)g.W * g.H;
        if (p->adjState == 1 && !(p->adjSrcCount != 0 && p->adjDstCount != 0) && !loses) {
            const aai::AxisAdjointLaunch a = make_axis_adjoint_launch(*p, channels, dstStride);
            const char *name = "";
            hipError_t e = hipSuccess;
            for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridZ)      // grid.z carries the batch
                e = aai::launch_axis_adjoint_half(a, type, channels, std::min(batch - b0, kMaxGridZ), gd + (int64_t)b0 * dstImageStride * elem, dv,
                                                  gs + (int64_t)b0 * srcImageStride * elem, sv, stream, &name);
            g_lastKernel = name;
            if (e != hipSuccess) return hip_fail(e, name);
            return AAI_OK;
        }
    }
    // FORWARDING: widen gdst into dense fp32 scratch, the code behind aai_adjoint_planned_interleaved_device_f32 into a dense fp32 gsrc,
    // one rounding into the caller's buffer -- the bits of narrow(fp32 entry(widen(gdst))).  (An empty gdst is not widened: nothing to launch.)
    const NarrowSide in{dGdst, dv, (int64_t)g.dW * channels, g.dH}, out{dGsrc, sv, (int64_t)g.W * channels, g.H};
    int device = 0;
    AAI_HIP(hipGetDevice(&device));
    return through_fp32_scratch(type, true, in, out, batch, device, "+widened", stream, [&](int nb, const void *gd32, float *gs32) {
        return enqueue_adjoint(ADJOINT_SEPARABLE, rq, g, nb, channels, static_cast<const float *>(gd32), in.row, (int64_t)in.count(), gs32, out.row,
                               (int64_t)out.count(), stream);
    });
}

int enqueue_half(const aai_request &rq, const Geometry &g, int batch, int channels, int halfType, const void *dSrc, int64_t srcStride, int64_t srcImageStride,
                 void *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream)
{
    const int type = halfType == AAI_HALF_F16 ? aai::NARROW_F16 : aai::NARROW_BF16;
    return enqueue_narrow(rq, g, batch, channels, type, dSrc, srcStride, srcImageStride, dDst, dstStride, dstImageStride, stream);
}

int enqueue_int(const aai_request &rq, const Geometry &g, int batch, int channels, int srcType, const void *dSrc, int64_t srcStride, int64_t srcImageStride,
                void *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream)
{
    const int type = srcType == aai::SRC_U8 ? aai::NARROW_U8 : aai::NARROW_U16;
    return enqueue_narrow(rq, g, batch, channels, type, dSrc, srcStride, srcImageStride, dDst, dstStride, dstImageStride, stream);
}

// ---- resample and convert (include/ext/aai_convert.h; aai_axis_convert.hip): routes in aai_engine.hpp
int enqueue_convert(const aai_request &rq, const Geometry &g, int batch, int channels, int srcType, const void *dSrc, int64_t srcStride, int64_t srcImageStride,
                    const aai::ConvertParams &cv, void *dDst, int64_t dstStride, int64_t dstImageStride, hipStream_t stream)
{
    if (g.dW == 0 || g.dH == 0 || batch == 0) return AAI_OK;
    const int type = srcType == aai::SRC_U8 ? aai::NARROW_U8 : aai::NARROW_U16;
    const int64_t rowDst = (int64_t)g.dW * channels;
    const size_t nDst = (size_t)rowDst * (size_t)g.dH;
    // the forward's plan under (request, channels), as enqueue_narrow acquires it for an integer image
    PlanRef p;
    const int rc = acquire_plan(rq, g, -1, -1, channels, rot_form(rq, g, channels, srcType, srcStride), &p, /*onCallerStream*/ true, stream);
    if (rc != AAI_OK) return rc;
    const int64_t elem = (int64_t)aai::narrow_elem_size(type), outElem = (int64_t)aai::convert_out_size(cv.outType);
    const char *src = static_cast<const char *>(dSrc);
    char *dst = static_cast<char *>(dDst);
    const aai::ImageView sv{srcStride, srcImageStride}, dv{dstStride, dstImageStride};
    hipError_t e = hipSuccess;
    if (p->kernel == AAI_KERNEL_AXIS && !p->dense && p->flaggedPixels == 0 && (rq.mode == AAI_MODE_AREA || rq.mode == AAI_MODE_FAST)) {
        // (the tables and the launch block are read-only here: no side stream, no event, hence no lock)
        const aai::AxisLaunch a = make_axis_launch(*p, channels, dstStride);
        if (aai::axis_convert_can_serve(a, type, cv.outType, cv.planar)) {
            const char *name = "";
            for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridZ)
                e = aai::launch_axis_convert(a, type, cv, src + (int64_t)b0 * srcImageStride * elem, sv, dst + (int64_t)b0 * dstImageStride * outElem, dv,
                                             std::min(batch - b0, kMaxGridZ), stream, &name);
            g_lastKernel = name;
            if (e != hipSuccess) return hip_fail(e, name);
            return AAI_OK;
        }
    }
    // forwarding: the fp32 entry's launches into dense fp32 scratch (enqueue() reads u8 / u16 itself), one conversion -- the bits of
    // round(fma(fp32 entry(src), scale, offset))
    const NarrowSide in{dSrc, sv, (int64_t)g.W * channels, g.H}, out{dDst, dv, rowDst, g.dH};
    return through_fp32_scratch_into(type, false, in, out, batch, p->device, "+converted", stream, "aai_convert_store_kernel",
                                     [&](int nb, const void *in32, float *out32) {
                                         return enqueue(rq, g, nb, in32, srcType, srcStride, srcImageStride, out32, rowDst, (int64_t)nDst, stream, -1, -1, channels);
                                     },
                                     [&](int nb, const float *out32, int b0) {
                                         return aai::launch_convert_store(cv, channels, out32, dst + (int64_t)b0 * dstImageStride * outElem, dv, g.dW, g.dH, nb, stream);
                                     });
}

int require_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(AAI_ERR_NO_DEVICE, "No HIP device available: libaai_hip has no CPU fallback.");
    }
    return AAI_OK;
}


}  // namespace engine
}  // namespace aai
