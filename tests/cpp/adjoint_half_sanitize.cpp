// TEST INFRASTRUCTURE ONLY -- a stand-alone host program around the CPU replay of the half-precision transposed separable kernel
// (tests/emulation/adjoint_half_emulation.cpp: the product's planner and csrc/aai_axis_adjoint_half_math.hpp, the function the kernel
// calls), built by tests/test_adjoint_half_host.py with -fsanitize=address,undefined.  gdst and gsrc are heap buffers of exactly the
// entitled size, so a read or write of the per-lane arithmetic outside them -- in any quadrant, with flips, at odd row lengths -- stops
// the program.  Prints one line per geometry; exit status 0 when every replay ran.
#include <cstdio>
#include <cstdlib>

#include "../emulation/adjoint_half_emulation.cpp"

namespace {

struct Geo { int W, H; double sr, dr, isoX, isoY, ang; };
// cases a, c, e, f, h, l of tests/half_cases.py
const Geo kGeos[] = {{64, 48, 4, 1, 31.5, 23.5, 0}, {1030, 21, 4, 1, 514.5, 10.5, 180}, {70, 50, 1, 2, 34.5, 24.5, 180}, {37, 29, 1, 3, 18, 14, 0},
                     {5, 7, 2, 1, 2, 3, 0},          {130, 90, 1, 1.7, 64.2, 44.9, 180}};

}  // namespace

int main()
{
    int ran = 0;
    for (const Geo &k : kGeos)
        for (double extra : {0.0, 90.0, 270.0})
            for (int mode : {AAI_MODE_AREA, AAI_MODE_FAST}) {
                aai_request rq{};
                rq.mode = mode; rq.policy = 0; rq.src_width = k.W; rq.src_height = k.H;
                rq.src_res_x = rq.src_res_y = k.sr; rq.dst_res_x = rq.dst_res_y = k.dr;
                rq.src_iso_x = k.isoX; rq.src_iso_y = k.isoY;
                rq.rotation_deg = k.ang + extra >= 360.0 ? k.ang + extra - 360.0 : k.ang + extra;
                Facts f;
                const int rc = plan_facts(rq, f);
                if (rc > 0) { fprintf(stderr, "geometry refused: %d\n", rc); return 2; }
                if (rc != 0) continue;      // a plan with correction lists: not the replayed kernel's
                for (int ht : {(int)HALF_F16, (int)HALF_BF16})
                    for (int C : {1, 3, 4}) {
                        const size_t nDst = (size_t)f.g.dW * f.g.dH * C, nSrc = (size_t)f.g.W * f.g.H * C;
                        uint16_t *gdst = static_cast<uint16_t *>(malloc(nDst * sizeof(uint16_t)));
                        uint16_t *gsrc = static_cast<uint16_t *>(malloc(nSrc * sizeof(uint16_t)));
                        if (!gdst || !gsrc) return 3;
                        // every finite bit pattern shape in turn: normal, subnormal and zero of either sign
                        for (size_t i = 0; i < nDst; ++i) gdst[i] = (uint16_t)((i * 2654435761u) >> 7) & 0xbbffu;
                        if (aai_emu_adjoint_half(&rq, ht, C, gdst, gsrc) != 0) return 4;
                        unsigned sum = 0;
                        for (size_t i = 0; i < nSrc; ++i) sum = sum * 31u + gsrc[i];
                        printf("%dx%d %g:%g at %g mode %d type %d C=%d: checksum %08x\n", k.W, k.H, k.sr, k.dr, rq.rotation_deg, mode, ht, C, sum);
                        free(gdst);
                        free(gsrc);
                        ++ran;
                    }
            }
    return ran >= 100 ? 0 : 5;
}
