// TEST INFRASTRUCTURE ONLY -- a stand-alone host program around the CPU replay of the resample-and-convert kernel
// (tests/emulation/convert_emulation.cpp: the product's planner, csrc/aai_int_math.hpp and csrc/aai_half_math.hpp), built by
// tests/test_convert_host.py with -fsanitize=address,undefined.  Source and destination are heap buffers of exactly the entitled size, so
// a read or write of the replay outside them -- at 180 degrees, at odd row lengths, in the planar mapping -- stops the program.
// One argument per case of tests/convert_cases.py: W,H,src_res,dst_res,iso_x,iso_y,angle,mode,channels,elem_bytes,out_type,planar.
// Prints one line per case; exit status 0 when every replay ran.
#include <cstdio>
#include <cstdlib>

#include "../emulation/convert_emulation.cpp"

int main(int argc, char **argv)
{
    int ran = 0;
    for (int i = 1; i < argc; ++i) {
        int W, H, mode, C, eb, ot, planar;
        double sr, dr, ix, iy, ang;
        if (sscanf(argv[i], "%d,%d,%lf,%lf,%lf,%lf,%lf,%d,%d,%d,%d,%d", &W, &H, &sr, &dr, &ix, &iy, &ang, &mode, &C, &eb, &ot, &planar) != 12) return 2;
        aai_request rq{};
        rq.mode = mode; rq.policy = 0; rq.src_width = W; rq.src_height = H;
        rq.src_res_x = rq.src_res_y = sr; rq.dst_res_x = rq.dst_res_y = dr;
        rq.src_iso_x = ix; rq.src_iso_y = iy; rq.rotation_deg = ang;
        Geometry g;
        std::string msg;
        if (make_geometry(rq, g, msg) != AAI_OK) { fprintf(stderr, "geometry refused: %s\n", msg.c_str()); return 3; }
        const size_t nSrc = (size_t)W * H * C, nDst = (size_t)g.dW * g.dH * C, osz = ot == OUT_F32 ? 4 : 2;
        unsigned char *src = static_cast<unsigned char *>(malloc(nSrc * eb));
        unsigned char *dst = static_cast<unsigned char *>(malloc(nDst * osz));
        float *pre = static_cast<float *>(malloc(nDst * sizeof(float)));
        if (!src || !dst || !pre) return 4;
        for (size_t k = 0; k < nSrc * eb; ++k) src[k] = (unsigned char)((k * 2654435761u) >> 11);
        const float scale[4] = {-1.f / 255.f, 300.f, 1.f, -2.f}, offset[4] = {0.5f, 0.f, -7.25f, 1e-3f};
        if (aai_emu_convert_replay(&rq, C, eb, src, scale, offset, ot, planar, dst, pre) != 0) { fprintf(stderr, "case %s: no direct replay\n", argv[i]); return 5; }
        unsigned sum = 0;
        for (size_t k = 0; k < nDst * osz; ++k) sum = sum * 31u + dst[k];
        printf("%s: checksum %08x\n", argv[i], sum);
        free(src);
        free(dst);
        free(pre);
        ++ran;
    }
    return ran == argc - 1 && ran > 0 ? 0 : 6;
}
