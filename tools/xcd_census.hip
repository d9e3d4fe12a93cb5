// xcd_census.hip -- which XCD does workgroup b of a launch run on?  K1's banded workgroup order (axis_block_order, aai_plan.hpp) assumes
// the dispatcher deals the workgroups of a launch round-robin over the 8 XCDs; this program looks.  It launches a trivial kernel on the
// grids of BASELINE config 2 -- (8, 1024, 4) and (8, 2048, 4) workgroups of 256 threads: rows = 2 and rows = 1 -- and every workgroup
// records the XCC_ID hardware register and the wall clock.  For 20 back-to-back launches per grid it prints the XCD of workgroup 0,
// whether placement was strictly round-robin (XCD of b = XCD of 0 + b, mod 8), and the table label (b % 8) -> XCD; then the same after
// a preceding dummy launch of k = 1..7 workgroups, which shows whether a launch starts where the one before it stopped.
// Run it in several fresh processes: the question is whether the first XCD is the same within a process and differs between them.
// build + run:  hipcc --offload-arch=gfx950 -O3 -o xcd_census tools/xcd_census.hip && ./xcd_census
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

struct Rec { unsigned long long clock; unsigned xcd, pad; };

__global__ __launch_bounds__(256) void k_census(Rec *rec, unsigned n)
{
    if (threadIdx.x != 0) return;
    const unsigned b = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (b >= n) return;
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(id));
    Rec r;
    r.clock = wall_clock64(); r.xcd = id; r.pad = 0;
    rec[b] = r;                                  // (an ordinary vector store)
}
__global__ __launch_bounds__(256) void k_dummy(unsigned *sink) { if (sink && threadIdx.x == 1024) *sink = 0; }

static void report(const char *what, const std::vector<Rec> &r)
{
    const unsigned n = (unsigned)r.size(), first = r[0].xcd;
    unsigned rr = 0, table[8][8] = {};
    unsigned long long lo = ~0ull, hi = 0;
    for (unsigned b = 0; b < n; ++b) {
        rr += r[b].xcd == ((first + b) & 7u);
        ++table[b & 7u][r[b].xcd & 7u];
        lo = r[b].clock < lo ? r[b].clock : lo; hi = r[b].clock > hi ? r[b].clock : hi;
    }
    printf("%-28s first=%u  round-robin=%s (%.4f of %u)  label->xcd", what, first, rr == n ? "strict" : "no", (double)rr / n, n);
    for (int l = 0; l < 8; ++l) {
        int best = 0;
        for (int x = 1; x < 8; ++x) if (table[l][x] > table[l][best]) best = x;
        printf(" %d:%d(%.3f)", l, best, (double)table[l][best] / (n / 8));
    }
    printf("  span %.1f us\n", (double)(hi - lo) / 100.0);       // the wall clock ticks at 100 MHz
}

int main()
{
    const dim3 grids[2] = {dim3(8, 1024, 4), dim3(8, 2048, 4)};
    const unsigned nMax = 8 * 2048 * 4;
    Rec *dev = nullptr;
    CHECK(hipMalloc((void **)&dev, sizeof(Rec) * nMax));
    std::vector<Rec> host;
    char what[64];
    for (const dim3 &g : grids) {
        const unsigned n = g.x * g.y * g.z;
        host.resize(n);
        for (int i = 0; i < 20; ++i) {                           // back to back: nothing between the launches but the copy
            hipLaunchKernelGGL(k_census, g, dim3(256), 0, 0, dev, n);
            CHECK(hipGetLastError());
            CHECK(hipMemcpy(host.data(), dev, sizeof(Rec) * n, hipMemcpyDeviceToHost));
            snprintf(what, sizeof what, "grid (%u,%u,%u) launch %2d", g.x, g.y, g.z, i);
            report(what, host);
        }
        for (unsigned k = 1; k <= 7; ++k) {
            hipLaunchKernelGGL(k_dummy, dim3(k), dim3(256), 0, 0, (unsigned *)nullptr);
            hipLaunchKernelGGL(k_census, g, dim3(256), 0, 0, dev, n);
            CHECK(hipGetLastError());
            CHECK(hipMemcpy(host.data(), dev, sizeof(Rec) * n, hipMemcpyDeviceToHost));
            snprintf(what, sizeof what, "grid (%u,%u,%u) after k=%u", g.x, g.y, g.z, k);
            report(what, host);
        }
    }
    CHECK(hipFree(dev));
    return 0;
}
