// aai_f64_math.hpp -- the per-pixel body of the reference-precision forward (aai_f64.hip), shared with the serial CPU replay of the
// test-suite (tests/emulation/f64_emulation.cpp).  The f64 adjoint needs no body of its own: it is adjoint_normalised and adjoint_gather
// of aai_adjoint_math.hpp, read and stored as doubles.
//
// dst = W src on double images, with W exactly as aai_adjoint_math.hpp states it: a pair's weight is adjoint_pair_weight<MODE> -- the
// closed forms of the forward's double-precision fix-up pass with the strict replay of the reference's classifier at knife edges --
// from the same operands ((px, py) from pixel_centre, ex = X - px), over the window of rot_window, rows outer and columns inner.  The
// sum of the weights is accumulated in adjoint_weight_sum's order, so a (dst, src) pair has the same weight bits, and a dst pixel the
// same denominator bits, in the forward, in pass 1 of the adjoint and in its gather: the three kernels apply one matrix and its
// transpose.  No plan: every angle runs through this code, reduced angle 0 included (aai_adjoint_math.hpp says why that is sound).
//
// Value domain (include/aai.h): a source pixel is read only where its weight is not 0, so a non-finite source pixel reaches exactly
// the dst pixels that carry weight on it.
#pragma once

#include "aai_adjoint_math.hpp"

namespace aai {

// dst pixel (dx, dy) of one image; img addresses source element (0, 0), rowStride in elements
template <int MODE>
AAI_HD double f64_forward(const RotLaunch &r, int dx, int dy, const double *img, int64_t rowStride)
{
    double px, py;
    pixel_centre(r, dx, dy, px, py);
    int x0, x1, y0, y1;
    rot_window(r, px, py, x0, x1, y0, y1);
    SVec sv4[4];
    bool haveVertices = false;
    double sum = 0.0, acc = 0.0;
    for (int Y = y0; Y <= y1; ++Y)
        for (int X = x0; X <= x1; ++X) {
            const double w = adjoint_pair_weight<MODE>(r, dx, dy, px, py, X, Y, sv4, haveVertices);
            sum += w;
            if (w != 0.0) acc += w * img[virt_offset(r, X, Y, rowStride)];
        }
    return adjoint_sum_counts<MODE>(sum) ? acc / sum : 0.0;      // the forward writes 0 otherwise (Source.cpp:577 / 905)
}

}  // namespace aai
