// bgr.hpp -- colour (BGR) scans into the sweep's bit images: the gray conversion and the threshold fused into the
// bit-packing loads, so no gray image is ever written (the colour batch entry points).
//
// gray = cvtColor(COLOR_RGB2GRAY) applied to BGR memory order, as projection.rs:29-32 does (quirk B8):
// byte 0 takes the R weight and byte 2 the B weight, (b0 * 9798 + b1 * 19235 + b2 * 3735 + 2^14) >> 15 -- the arithmetic of
// rgb2gray3_x4_kernel (stages.hip) and oracle.rgb2gray.  A pixel is black iff gray <= black_max, i.e. iff the weighted
// sum is below (black_max + 1) << 15: no shift per pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace omr {

__device__ __forceinline__ uint32_t bgr_gray(uint32_t b0, uint32_t b1, uint32_t b2)
{
    return (b0 * 9798u + b1 * 19235u + b2 * 3735u + 16384u) >> 15;
}

__device__ __forceinline__ uint32_t bgr_black(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t lim)
{
    return b0 * 9798u + b1 * 19235u + b2 * 3735u + 16384u < lim ? 1u : 0u;
}

// 32 BGR pixels at p (96 bytes) -> one word, bit i = pixel i is black.  n = pixels that exist (1..32); lim = (black_max + 1)
// << 15.  p 16-byte aligned and n = 32: six 16-byte loads; otherwise byte loads of the n pixels only.
__device__ __forceinline__ uint32_t bgr_pack32(const uint8_t *__restrict__ p, int n, uint32_t lim)
{
    uint32_t w = 0;
    if (n == 32 && (((uintptr_t)p) & 15u) == 0) {
        uint32_t d[24];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const uint4 q = *(const uint4 *)(p + 16 * k);
            d[4 * k] = q.x, d[4 * k + 1] = q.y, d[4 * k + 2] = q.z, d[4 * k + 3] = q.w;
        }
        // pixel i = bytes 3 i .. 3 i + 2 of the 96: four pixels per three dwords
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const uint32_t a = d[3 * g], b = d[3 * g + 1], c = d[3 * g + 2];
            w |= bgr_black(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u, lim) << (4 * g);
            w |= bgr_black(a >> 24, b & 255u, (b >> 8) & 255u, lim) << (4 * g + 1);
            w |= bgr_black((b >> 16) & 255u, b >> 24, c & 255u, lim) << (4 * g + 2);
            w |= bgr_black((c >> 8) & 255u, (c >> 16) & 255u, c >> 24, lim) << (4 * g + 3);
        }
    } else {
        for (int i = 0; i < n; i++) w |= bgr_black(p[3 * i], p[3 * i + 1], p[3 * i + 2], lim) << i;
    }
    return w;
}

}  // namespace omr
