// warp_affine.hip -- warpAffine of rotate_mat (transfer.rs:459-523) and of the final deskew of a single sheet
// (omr.rs:408-445, core/src/main.rs:72-81), for one image or for a batch of same-shape images with a matrix and a
// canvas each (image index = blockIdx.z): one dispatch rule, two kernels.  OpenCV 4.6.0 imgwarp.cpp: WarpAffineInvoker's
// fixed-point coordinates (AB_BITS = 10, round delta 512 for NEAREST and 16 otherwise, saturate_cast<short>), then
// remapNearest / remapBilinear / remapBicubic / remapLanczos4 with FixedPtCast<int, uchar, 15> (warp_fixed.hpp).
//
// Both kernels give a workgroup a 64 x 16 destination tile, bound the tile's source box by its four corner samples and
// copy the box to LDS with row-contiguous dword loads, so a tap is an LDS byte read with no bounds test instead of a byte
// gather through L1 along a slanted line (about 45 cache lines per wave).  A tile whose box does not fit (strong
// magnification) takes its taps from global memory.
//   warp_lds_kernel<CN, LINEAR>      1 / 3 channels, NEAREST / LINEAR, BORDER_CONSTANT: 16 KB of LDS, 4 pixels per lane
//   warp_taps_kernel<CN, K, BORDER>  everything else: K x K taps per pixel (K = 1 NEAREST, 2 LINEAR, 4 CUBIC, 8
//                                    LANCZOS4), 1..4 channels, every border mode, the border map applied while staging
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "kernels.hpp"
#include "warp_fixed.hpp"

namespace omr {

#define WL_TW 64
#define WL_TH 16
#define WL_LDS 16384

// One image per call (B.per == NULL: the matrix and the canvas are the kernel's arguments) or a batch of same-shape
// images with a matrix and a canvas each: image blockIdx.z reads its record, moves src / dst to its own image and
// slot, and leaves at once when the tile lies outside its canvas (the grid covers the largest one).  Everything here
// is uniform over the workgroup; from here on both cases run the same code.
#define WARP_PICK_IMAGE(tx0_, ty0_)                                                  \
    if (B.per) {                                                                     \
        const WarpImg &I = B.per[blockIdx.z];                                        \
        for (int i = 0; i < 6; i++) M[i] = I.minv[i];                                \
        drows = I.rows, dcols = I.cols;                                              \
        if ((tx0_) >= dcols || (ty0_) >= drows) return;                              \
        src += (int64_t)blockIdx.z * B.sstride, dst += (int64_t)blockIdx.z * B.dstride; \
    } else {                                                                         \
        for (int i = 0; i < 6; i++) M[i] = W.m[i];                                   \
    }

// The box has one pixel of slack for the rounding of the fixed-point tables and one more for the bilinear taps; pixels
// outside the image are staged as the border value.
template <int CN, bool LINEAR>
__global__ __launch_bounds__(256) void warp_lds_kernel(const uint8_t *__restrict__ src, int64_t sstep, int srows,
                                                       int scols, uint8_t *__restrict__ dst, int64_t dstep, int drows,
                                                       int dcols, const WarpM W, uint32_t border_rgba,
                                                       const WarpBatch B)
{
    __shared__ __attribute__((aligned(16))) uint8_t box[WL_LDS];
    const int rd = LINEAR ? 16 : 512;
    const int tx0 = blockIdx.x * WL_TW, ty0 = blockIdx.y * WL_TH;
    double M[6];
    WARP_PICK_IMAGE(tx0, ty0);
    const int tx1 = min(dcols, tx0 + WL_TW) - 1, ty1 = min(drows, ty0 + WL_TH) - 1;
    // fixed-point source coordinates (OpenCV's tables) of the tile's corner samples: wave-uniform.  X0(y) and
    // adelta(x) are both monotone, so the four corners bound every sample of the tile.  (The two kernels write the box
    // out, each with its own slack, on the shared coordinate expressions: behind a shared box function the compiler no
    // longer proved the tap index 24-bit here -- v_mad_u64_u32 for v_mad_i32_i24 -- profiles/r09_one_warp_path.md)
    auto FX = [&](int x, int y) { return warp_row_x(M, y, rd) + warp_col_x(M, x); };
    auto FY = [&](int x, int y) { return warp_row_y(M, y, rd) + warp_col_y(M, x); };
    const int cx[4] = {FX(tx0, ty0) >> 10, FX(tx1, ty0) >> 10, FX(tx0, ty1) >> 10, FX(tx1, ty1) >> 10};
    const int cy[4] = {FY(tx0, ty0) >> 10, FY(tx1, ty0) >> 10, FY(tx0, ty1) >> 10, FY(tx1, ty1) >> 10};
    const int bx0 = min(min(cx[0], cx[1]), min(cx[2], cx[3])) - 1;
    const int bx1 = max(max(cx[0], cx[1]), max(cx[2], cx[3])) + 1 + (LINEAR ? 1 : 0);
    const int by0 = min(min(cy[0], cy[1]), min(cy[2], cy[3])) - 1;
    const int by1 = max(max(cy[0], cy[1]), max(cy[2], cy[3])) + 1 + (LINEAR ? 1 : 0);
    // the box in BYTES of a source row, widened to whole dwords of the row
    const int bb0 = (bx0 * CN) & ~3, bb1 = ((bx1 + 1) * CN + 3) & ~3;  // [bb0, bb1)
    const int bwb = bb1 - bb0, bh = by1 - by0 + 1;
    const bool staged = bwb > 0 && bh > 0 && (int64_t)bwb * bh <= WL_LDS && bx0 > -30000 && bx1 < 30000 &&
                        by0 > -30000 && by1 < 30000;
    const int rowb = scols * CN;  // bytes of a source row that hold pixels
    if (staged) {
        const int bq = bwb >> 2;
        const bool aligned = ((sstep | (int64_t)(uintptr_t)src) & 3) == 0;
        for (int i = threadIdx.x; i < bq * bh; i += 256) {
            const int ly = i / bq, lq = i - ly * bq;
            const int gy = by0 + ly, gb = bb0 + lq * 4;
            uint32_t v;
            if (aligned && (unsigned)gy < (unsigned)srows && gb >= 0 && gb + 4 <= rowb) {
                v = *(const uint32_t *)(src + (int64_t)gy * sstep + gb);
            } else {
                v = 0;
                for (int j = 0; j < 4; j++) {
                    const int b = gb + j;  // byte b of row gy: pixel b / CN, channel b % CN (floor semantics for b < 0)
                    const int ch = ((b % CN) + CN) % CN;
                    uint32_t px = (border_rgba >> (8 * ch)) & 255u;
                    if ((unsigned)gy < (unsigned)srows && b >= 0 && b < rowb) px = src[(int64_t)gy * sstep + b];
                    v |= px << (8 * j);
                }
            }
            *(uint32_t *)&box[ly * bwb + lq * 4] = v;
        }
    }
    __syncthreads();
    const int lx = (threadIdx.x & 15) * 4, ly = threadIdx.x >> 4;
    const int x0 = tx0 + lx, y = ty0 + ly;
    if (x0 >= dcols || y >= drows) return;
    const int X0 = warp_row_x(M, y, rd), Y0 = warp_row_y(M, y, rd);
    uint8_t o[4 * CN];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = x0 + j;
        const int Xf = X0 + warp_col_x(M, x), Yf = Y0 + warp_col_y(M, x);
        if (!staged) {
#pragma unroll
            for (int c = 0; c < CN; c++)
                o[j * CN + c] = (uint8_t)warp_tap_global<LINEAR>(src + c, sstep, srows, scols, CN, Xf, Yf, (border_rgba >> (8 * c)) & 255);
        } else if (!LINEAR) {
            const uint8_t *B = &box[((Yf >> 10) - by0) * bwb + (Xf >> 10) * CN - bb0];
#pragma unroll
            for (int c = 0; c < CN; c++) o[j * CN + c] = B[c];
        } else {
            const int X = Xf >> 5, Y = Yf >> 5;
            const uint8_t *B = &box[((Y >> 5) - by0) * bwb + (X >> 5) * CN - bb0];
            const int fx = X & 31, fy = Y & 31;
            const int w0 = (32 - fy) * (32 - fx) * 32, w1 = (32 - fy) * fx * 32, w2 = fy * (32 - fx) * 32, w3 = fy * fx * 32;
#pragma unroll
            for (int c = 0; c < CN; c++)
                o[j * CN + c] = sat_u8((B[c] * w0 + B[CN + c] * w1 + B[bwb + c] * w2 + B[bwb + CN + c] * w3 + (1 << 14)) >> 15);
        }
    }
    uint8_t *D = dst + (int64_t)y * dstep + (int64_t)x0 * CN;
    if (x0 + 4 <= dcols && ((uintptr_t)D & 3) == 0) {  // packed CONTAIN canvases have odd widths: rows start anywhere
#pragma unroll
        for (int q = 0; q < CN; q++)
            ((uint32_t *)D)[q] = (uint32_t)o[4 * q] | ((uint32_t)o[4 * q + 1] << 8) | ((uint32_t)o[4 * q + 2] << 16) |
                                 ((uint32_t)o[4 * q + 3] << 24);
    } else {
        for (int j = 0; j < 4 * CN && x0 * CN + j < dcols * CN; j++) D[j] = o[j];
    }
}

// ---- K x K taps under every border mode.  The box is the corner samples' widened by the window (K/2 - 1 texels before,
// K/2 after) and staged with the border map applied, so the inner loop is K x K integer multiply-adds from LDS.
// BORDER_CONSTANT stages the border value at outside taps: remapBicubic's cv*ONE + sum (S - cv) w equals sum S w with cv
// at the outside taps, since the fixed-point weights sum to 32768.  A tile whose box does not fit gathers its taps from
// global memory with the same map.
#define WT_TW 64
#define WT_TH 16
#define WT_LDS 32768

// borderInterpolate (OpenCV 4.6.0) of coordinate p on an axis of length len; -1 for BORDER_CONSTANT outside.
// BORDER_TRANSPARENT (5) maps as REFLECT_101: remap's borderType1.  REFLECT / REFLECT_101 are the library's loop in
// closed form (each pass of the loop folds by one reflection, so p lands where p mod 2 len, or 2 len - 2, puts it);
// WRAP is the floor modulus.
template <int BORDER>
__device__ __forceinline__ int wt_border_map(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (BORDER == 0) return -1;
    if (BORDER == 1) return p < 0 ? 0 : len - 1;
    if (BORDER == 3) {
        const int m = p % len;
        return m < 0 ? m + len : m;
    }
    if (len == 1) return 0;
    constexpr int d = BORDER == 2 ? 0 : 1;
    const int per = 2 * len - 2 * d;
    int m = p % per;
    if (m < 0) m += per;
    return m < len ? m : per - 1 + d - m;
}

template <int CN, int K, int BORDER>
__global__ __launch_bounds__(256) void warp_taps_kernel(const uint8_t *__restrict__ src, int64_t sstep, int srows,
                                                        int scols, uint8_t *__restrict__ dst, int64_t dstep, int drows,
                                                        int dcols, const WarpM W, uint32_t border_rgba,
                                                        const int16_t *__restrict__ wtab, const WarpBatch B)
{
    constexpr int O = K == 1 ? 0 : K / 2 - 1;  // first tap = sx - O
    __shared__ __attribute__((aligned(16))) uint8_t box[WT_LDS];
    const int rd = K == 1 ? 512 : 16;
    const int tx0 = blockIdx.x * WT_TW, ty0 = blockIdx.y * WT_TH;
    double M[6];
    WARP_PICK_IMAGE(tx0, ty0);
    const int tx1 = min(dcols, tx0 + WT_TW) - 1, ty1 = min(drows, ty0 + WT_TH) - 1;
    // the corner samples, as in warp_lds_kernel; saturate_cast<short>(X >> 5 >> 5) == sat16(Xf >> 10) for every K
    auto FX = [&](int x, int y) { return warp_row_x(M, y, rd) + warp_col_x(M, x); };
    auto FY = [&](int x, int y) { return warp_row_y(M, y, rd) + warp_col_y(M, x); };
    const int cx[4] = {sat16(FX(tx0, ty0) >> 10), sat16(FX(tx1, ty0) >> 10), sat16(FX(tx0, ty1) >> 10), sat16(FX(tx1, ty1) >> 10)};
    const int cy[4] = {sat16(FY(tx0, ty0) >> 10), sat16(FY(tx1, ty0) >> 10), sat16(FY(tx0, ty1) >> 10), sat16(FY(tx1, ty1) >> 10)};
    const int bx0 = min(min(cx[0], cx[1]), min(cx[2], cx[3])) - O;
    const int bx1 = max(max(cx[0], cx[1]), max(cx[2], cx[3])) - O + K - 1;
    const int by0 = min(min(cy[0], cy[1]), min(cy[2], cy[3])) - O;
    const int by1 = max(max(cy[0], cy[1]), max(cy[2], cy[3])) - O + K - 1;
    const int bb0 = (bx0 * CN) & ~3, bb1 = ((bx1 + 1) * CN + 3) & ~3;  // box bytes [bb0, bb1) of a row, whole dwords
    const int bwb = bb1 - bb0, bh = by1 - by0 + 1;
    const bool staged = (int64_t)bwb * bh <= WT_LDS && bx0 > -30000 && bx1 < 30000 && by0 > -30000 && by1 < 30000;
    const int rowb = scols * CN;
    if (staged) {
        const int bq = bwb >> 2;
        const bool aligned = ((sstep | (int64_t)(uintptr_t)src) & 3) == 0;
        for (int i = threadIdx.x; i < bq * bh; i += 256) {
            const int ly = i / bq, lq = i - ly * bq;
            const int gy = by0 + ly, gb = bb0 + lq * 4;
            uint32_t v;
            if (aligned && (unsigned)gy < (unsigned)srows && gb >= 0 && gb + 4 <= rowb) {
                v = *(const uint32_t *)(src + (int64_t)gy * sstep + gb);
            } else {
                const int my = wt_border_map<BORDER>(gy, srows);
                v = 0;
                for (int j = 0; j < 4; j++) {
                    const int b = gb + j;
                    const int p = b >= 0 ? b / CN : -((-b + CN - 1) / CN);  // pixel (floor), channel b - p CN
                    const int ch = b - p * CN;
                    const int mx = wt_border_map<BORDER>(p, scols);
                    const uint32_t px = (my < 0 || mx < 0) ? (border_rgba >> (8 * ch)) & 255u
                                                           : src[(int64_t)my * sstep + (int64_t)mx * CN + ch];
                    v |= px << (8 * j);
                }
            }
            *(uint32_t *)&box[ly * bwb + lq * 4] = v;
        }
    }
    __syncthreads();
    const int lx = (threadIdx.x & 15) * 4, ly = threadIdx.x >> 4;
    const int x0 = tx0 + lx, y = ty0 + ly;
    if (x0 >= dcols || y >= drows) return;
    const int X0 = warp_row_x(M, y, rd), Y0 = warp_row_y(M, y, rd);
    // Lanczos4 (64 taps) stores each pixel as soon as it is done: four pixels in flight need 256 VGPRs at 3 and 4
    // channels (one wave per SIMD); one at a time needs about half that
    constexpr bool DIRECT = K == 8;
    uint8_t *D = dst + (int64_t)y * dstep + (int64_t)x0 * CN;
    uint8_t o[4 * CN];
    unsigned keepm = 0;
#pragma unroll DIRECT ? 1 : 4
    for (int j = 0; j < 4; j++) {
        const int x = min(x0 + j, dcols - 1);  // a column past the canvas is computed as the last one, never stored
        const int Xf = X0 + warp_col_x(M, x), Yf = Y0 + warp_col_y(M, x);
        const int sx = sat16(Xf >> 10), sy = sat16(Yf >> 10);
        const int fx = (Xf >> 5) & 31, fy = (Yf >> 5) & 31;
        bool keep = x0 + j < dcols;
        if (BORDER == 5) {
            // remapBilinear skips every pixel off its interior (w - 1); remapNearest / Bicubic / Lanczos4 those whose
            // centre tap is outside
            if (K == 2)
                keep = keep && (unsigned)sx < (unsigned)(scols - 1) && (unsigned)sy < (unsigned)(srows - 1);
            else
                keep = keep && (unsigned)sx < (unsigned)scols && (unsigned)sy < (unsigned)srows;
        }
        keepm |= (unsigned)keep << j;
        // fixed-point weights, tap row * K + col; the table's int16 pairs stay packed in dwords until used
        int w2[4] = {0, 0, 0, 0};
        uint32_t wpk[K >= 4 ? K * K / 2 : 1] = {0};
        if constexpr (K == 2) {  // initInterTab2D(INTER_LINEAR): exact products, no sum fix
            w2[0] = (32 - fy) * (32 - fx) * 32;
            w2[1] = (32 - fy) * fx * 32;
            w2[2] = fy * (32 - fx) * 32;
            w2[3] = fy * fx * 32;
        } else if constexpr (K >= 4) {  // the host's initInterTab2D table (oics_rotate.cpp), one entry per (fy, fx)
            const uint4 *wp = (const uint4 *)(wtab + (fy * 32 + fx) * K * K);
#pragma unroll
            for (int q = 0; q < K * K / 8; q++) {
                const uint4 t = wp[q];
                wpk[4 * q] = t.x;
                wpk[4 * q + 1] = t.y;
                wpk[4 * q + 2] = t.z;
                wpk[4 * q + 3] = t.w;
            }
        }
        auto wk = [&](int i) -> int {
            if constexpr (K == 1) return 1 << 15;
            else if constexpr (K == 2) return w2[i];
            else return (int)(int16_t)(uint16_t)(wpk[i >> 1] >> (16 * (i & 1)));
        };
        int sum[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) sum[c] = 0;
        if (staged) {
            const uint8_t *B = &box[(sy - O - by0) * bwb + (sx - O) * CN - bb0];
#pragma unroll
            for (int r = 0; r < K; r++)
#pragma unroll
                for (int t = 0; t < K; t++)
#pragma unroll
                    for (int c = 0; c < CN; c++) sum[c] += (int)B[r * bwb + t * CN + c] * wk(r * K + t);
        } else {
            // the slow path keeps its loops rolled (an unrolled 64-tap gather holds every load in flight) and so reads
            // the weights by computed index: LINEAR's from (fx, fy), the tables' from memory
#pragma unroll 1
            for (int r = 0; r < K; r++) {
                const int my = wt_border_map<BORDER>(sy - O + r, srows);
#pragma unroll 1
                for (int t = 0; t < K; t++) {
                    const int mx = wt_border_map<BORDER>(sx - O + t, scols);
                    int w;
                    if constexpr (K == 1) w = 1 << 15;
                    else if constexpr (K == 2) w = (r ? fy : 32 - fy) * (t ? fx : 32 - fx) * 32;
                    else w = wtab[(fy * 32 + fx) * K * K + r * K + t];
#pragma unroll
                    for (int c = 0; c < CN; c++) {
                        const int v = (my < 0 || mx < 0) ? (int)((border_rgba >> (8 * c)) & 255u)
                                                         : (int)src[(int64_t)my * sstep + (int64_t)mx * CN + c];
                        sum[c] += v * w;
                    }
                }
            }
        }
        if constexpr (DIRECT) {
            if (keep)
#pragma unroll
                for (int c = 0; c < CN; c++) D[j * CN + c] = sat_u8((sum[c] + (1 << 14)) >> 15);
        } else {
#pragma unroll
            for (int c = 0; c < CN; c++) o[j * CN + c] = sat_u8((sum[c] + (1 << 14)) >> 15);
        }
    }
    if constexpr (DIRECT) return;
    if (BORDER != 5 && x0 + 4 <= dcols && ((uintptr_t)D & 3) == 0) {
#pragma unroll
        for (int q = 0; q < CN; q++)
            ((uint32_t *)D)[q] = (uint32_t)o[4 * q] | ((uint32_t)o[4 * q + 1] << 8) | ((uint32_t)o[4 * q + 2] << 16) |
                                 ((uint32_t)o[4 * q + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (keepm >> j & 1)
#pragma unroll
                for (int c = 0; c < CN; c++) D[j * CN + c] = o[j * CN + c];
    }
}

template <int CN, int K>
static void launch_taps_border(dim3 grid, hipStream_t s, int border_mode, const uint8_t *d_src, int64_t sstep,
                               int srows, int scols, uint8_t *d_dst, int64_t dstep, int drows, int dcols,
                               const WarpM &W, uint32_t border_rgba, const int16_t *d_wtab, const WarpBatch &B)
{
#define WT_LAUNCH(B_)                                                                                                  \
    hipLaunchKernelGGL((warp_taps_kernel<CN, K, B_>), grid, dim3(256), 0, s, d_src, sstep, srows, scols, d_dst, dstep, \
                       drows, dcols, W, border_rgba, d_wtab, B)
    switch (border_mode) {
    case 0: WT_LAUNCH(0); break;
    case 1: WT_LAUNCH(1); break;
    case 2: WT_LAUNCH(2); break;
    case 3: WT_LAUNCH(3); break;
    case 4: WT_LAUNCH(4); break;
    default: WT_LAUNCH(5); break;
    }
#undef WT_LAUNCH
}

template <int CN>
static void launch_taps_k(int K, dim3 grid, hipStream_t s, int border_mode, const uint8_t *d_src, int64_t sstep,
                          int srows, int scols, uint8_t *d_dst, int64_t dstep, int drows, int dcols, const WarpM &W,
                          uint32_t border_rgba, const int16_t *d_wtab, const WarpBatch &B)
{
    if (K == 1) launch_taps_border<CN, 1>(grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
    else if (K == 2) launch_taps_border<CN, 2>(grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
    else if (K == 4) launch_taps_border<CN, 4>(grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
    else launch_taps_border<CN, 8>(grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
}

// the one dispatch rule: channels, interpolation and border mode.  The grid covers drows x dcols: the canvas of the one
// image, or the largest canvas of a batch (grid.z images, their records at B.per)
static hipError_t launch_warp(const uint8_t *d_src, int64_t sstep, int srows, int scols, int cn, uint8_t *d_dst,
                              int64_t dstep, int drows, int dcols, const WarpM &W, const WarpBatch &B, int nz, int interp,
                              int border_mode, uint32_t border_rgba, const int16_t *d_wtab, hipStream_t s)
{
    if (cn < 1 || cn > 4 || border_mode < 0 || border_mode > 5 || nz < 1 || nz > 65535) return hipErrorInvalidValue;
    const int K = interp == 0 ? 1 : interp == 1 ? 2 : interp == 2 ? 4 : interp == 4 ? 8 : 0;
    if (!K || (K >= 4 && !d_wtab)) return hipErrorInvalidValue;
    static_assert(WL_TW == WT_TW && WL_TH == WT_TH, "one grid for both kernels");
    dim3 grid((dcols + WT_TW - 1) / WT_TW, (drows + WT_TH - 1) / WT_TH, nz);
    if ((cn == 1 || cn == 3) && K <= 2 && border_mode == 0) {
#define WL_LAUNCH(CN_, LIN_)                                                                                           \
    hipLaunchKernelGGL((warp_lds_kernel<CN_, LIN_>), grid, dim3(256), 0, s, d_src, sstep, srows, scols, d_dst, dstep, \
                       drows, dcols, W, border_rgba, B)
        if (cn == 1 && K == 1) WL_LAUNCH(1, false);
        else if (cn == 1) WL_LAUNCH(1, true);
        else if (K == 1) WL_LAUNCH(3, false);
        else WL_LAUNCH(3, true);
#undef WL_LAUNCH
    } else if (cn == 1) launch_taps_k<1>(K, grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
    else if (cn == 2) launch_taps_k<2>(K, grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
    else if (cn == 3) launch_taps_k<3>(K, grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
    else launch_taps_k<4>(K, grid, s, border_mode, d_src, sstep, srows, scols, d_dst, dstep, drows, dcols, W, border_rgba, d_wtab, B);
    return hipGetLastError();
}

hipError_t launch_warp_affine(const uint8_t *d_src, int64_t sstep, int srows, int scols, int cn, uint8_t *d_dst,
                              int64_t dstep, int drows, int dcols, const double Minv[6], int interp, int border_mode,
                              uint32_t border_rgba, const int16_t *d_wtab, hipStream_t s)
{
    WarpM W;
    for (int i = 0; i < 6; i++) W.m[i] = Minv[i];
    return launch_warp(d_src, sstep, srows, scols, cn, d_dst, dstep, drows, dcols, W, WarpBatch{nullptr, 0, 0}, 1, interp,
                       border_mode, border_rgba, d_wtab, s);
}

hipError_t launch_warp_affine_batch(const uint8_t *d_src, int64_t sstride, int64_t sstep, int srows, int scols, int cn,
                                    uint8_t *d_dst, int64_t dstride, int64_t dstep, int max_drows, int max_dcols,
                                    const WarpImg *d_per, int n, int interp, int border_mode, uint32_t border_rgba,
                                    const int16_t *d_wtab, hipStream_t s)
{
    if (!d_per) return hipErrorInvalidValue;
    return launch_warp(d_src, sstep, srows, scols, cn, d_dst, dstep, max_drows, max_dcols, WarpM{}, WarpBatch{d_per, sstride, dstride},
                       n, interp, border_mode, border_rgba, d_wtab, s);
}

}  // namespace omr
