// warp_fixed.hpp -- the fixed-point arithmetic of OpenCV 4.6.0 warpAffine (imgwarp.cpp, WarpAffineInvoker + remapNearest /
// remapBilinear) that every warp kernel shares: warp_affine.hip (rotate_mat) evaluates the tables in place, deskew.hip
// (the batch's final warp) reads them precomputed and uses sat_u8, sat16 and the gray global tap only.  Device code; the files that
// include it are built -ffp-contract=off, and the f64 expressions keep OpenCV's operation order.
// The tile boxes and the staged bilinear blends stay written out in their kernels, on these expressions: routed through
// shared functions, the compiler merged tap bytes into 16-bit LDS reads at odd addresses and lost a 24-bit multiply
// (warp_lds_kernel<1, true>: 25 -> 31 us on an A4 sheet; profiles/r09_one_warp_path.md).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace omr {

__device__ __forceinline__ uint8_t sat_u8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
__device__ __forceinline__ int sat16(int v) { return max(-32768, min(32767, v)); }  // saturate_cast<short>

// The dst -> src matrix, passed to a kernel by value.
struct WarpM {
    double m[6];
};

// Source coordinates of destination pixel (x, y) with AB_BITS = 10 fraction bits: a row term that carries the round
// delta rd (512 for NEAREST, 16 otherwise) plus a column term -- OpenCV's X0 / Y0 and adelta / bdelta tables.
__device__ __forceinline__ int warp_row_x(const double *M, int y, int rd) { return (int)rint((M[1] * (double)y + M[2]) * 1024.0) + rd; }
__device__ __forceinline__ int warp_row_y(const double *M, int y, int rd) { return (int)rint((M[4] * (double)y + M[5]) * 1024.0) + rd; }
__device__ __forceinline__ int warp_col_x(const double *M, int x) { return (int)rint(M[0] * (double)x * 1024.0); }
__device__ __forceinline__ int warp_col_y(const double *M, int x) { return (int)rint(M[3] * (double)x * 1024.0); }

// One channel of the sample at fixed-point (Xf, Yf) straight from global memory, BORDER_CONSTANT: src points at the
// channel's byte of pixel (0, 0), pixels are cn bytes apart.
template <bool LINEAR>
__device__ __forceinline__ int warp_tap_global(const uint8_t *__restrict__ src, int64_t sstep, int srows, int scols, int cn,
                                               int Xf, int Yf, int border)
{
    if (!LINEAR) {
        const int X = sat16(Xf >> 10), Y = sat16(Yf >> 10);
        return ((unsigned)X < (unsigned)scols && (unsigned)Y < (unsigned)srows) ? src[(int64_t)Y * sstep + (int64_t)X * cn] : border;
    }
    const int X = Xf >> 5, Y = Yf >> 5;
    const int sx = sat16(X >> 5), sy = sat16(Y >> 5);
    if (sx >= scols || sx + 1 < 0 || sy >= srows || sy + 1 < 0) return border;
    const bool in_x0 = sx >= 0 && sx < scols, in_x1 = sx + 1 >= 0 && sx + 1 < scols;
    const bool in_y0 = sy >= 0 && sy < srows, in_y1 = sy + 1 >= 0 && sy + 1 < srows;
    const int v0 = in_x0 && in_y0 ? src[(int64_t)sy * sstep + (int64_t)sx * cn] : border;
    const int v1 = in_x1 && in_y0 ? src[(int64_t)sy * sstep + (int64_t)(sx + 1) * cn] : border;
    const int v2 = in_x0 && in_y1 ? src[(int64_t)(sy + 1) * sstep + (int64_t)sx * cn] : border;
    const int v3 = in_x1 && in_y1 ? src[(int64_t)(sy + 1) * sstep + (int64_t)(sx + 1) * cn] : border;
    // INTER_LINEAR's 15-bit weights (initInterTab2D: exact products of the 5-bit fractions) and FixedPtCast<int, uchar, 15>
    const int fx = X & 31, fy = Y & 31;
    const int w0 = (32 - fy) * (32 - fx) * 32, w1 = (32 - fy) * fx * 32, w2 = fy * (32 - fx) * 32, w3 = fy * fx * 32;
    return sat_u8((v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3 + (1 << 14)) >> 15);
}

}  // namespace omr
