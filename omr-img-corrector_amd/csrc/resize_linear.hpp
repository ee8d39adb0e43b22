// resize_linear.hpp -- the coefficient expressions of OpenCV's bilinear resize (resize.cpp, resizeGeneric_ with
// HResizeLinear<uchar,int,short,2048>), shared by the per-call kernel (stages.hip) and the batch kernel
// (projection_front.hip).  Device code; the files that include it are built -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace omr {

// One axis of one destination index d: the first source index s0, the two 11-bit taps c0 / c1 (double products, float
// fractions, saturate_cast<short>(c * 2048) with round-half-even) and, on the horizontal axis (ssize > 0), whether the
// column copies S[s0] * 2048 ("dx >= xmax": sx is monotone in dx, so that is just sx + 1 >= ssize).  area_mode: the
// coefficients INTER_AREA takes when an axis enlarges (quirk B7).
__device__ __forceinline__ void linear_coef(int d, double scale, double inv_scale, int ssize, bool area_mode, int &s0,
                                            int &c0, int &c1, bool &edge)
{
    float f;
    int sx;
    if (!area_mode) {
        f = (float)(((double)d + 0.5) * scale - 0.5);
        sx = (int)floorf(f);
        f -= (float)sx;
    } else {
        sx = (int)floor((double)d * scale);
        f = (float)((double)(d + 1) - (double)(sx + 1) * inv_scale);
        f = f <= 0.f ? 0.f : f - floorf(f);
    }
    s0 = sx;
    edge = false;
    if (ssize > 0) {  // horizontal axis only: the vertical axis keeps sy and clips the ROWS instead
        if (sx < 0) f = 0.f, sx = 0;
        if (sx + 1 >= ssize) {
            edge = true;
            if (sx >= ssize - 1) f = 0.f, sx = ssize - 1;
        }
        s0 = sx;
    }
    c0 = max(-32768, min(32767, (int)rintf((1.f - f) * 2048.f)));
    c1 = max(-32768, min(32767, (int)rintf(f * 2048.f)));
}

}  // namespace omr
