// stages.hip -- the per-image stage kernels either side of the sweep: the front end
// of omr.rs:87-139 (gray, erode x3) and threshold; the INTER_AREA shrink and every other resize are resize.hip, the
// final deskew warp is warp_affine.hip.  All are HBM-bound byte work: the tuned forms move 4 or 16 pixels per lane
// (dword loads / stores), stage reuse through LDS and keep OpenCV 4.6.0's integer arithmetic bit for bit.  One
// launcher per stage picks the tuned kernel where layout and alignment allow and otherwise the generic form (one
// thread per destination byte) that sits next to it.
#include <hip/hip_runtime.h>

#include "bgr.hpp"
#include "kernels.hpp"

namespace omr {

// ------------------------------------------------------------------------------------------
// cvtColor(COLOR_RGB2GRAY), 3 channels, 4 pixels per lane: three dword loads, one dword store.
__global__ __launch_bounds__(256) void rgb2gray3_x4_kernel(const uint8_t *__restrict__ src, int64_t sstep, int rows,
                                                           int cols, uint8_t *__restrict__ dst, int64_t dstep)
{
    const int q = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int x = q * 4;
    if (x >= cols) return;
    const uint8_t *S = src + (int64_t)y * sstep + (int64_t)x * 3;
    uint8_t *D = dst + (int64_t)y * dstep + x;
    if (x + 4 <= cols) {
        const uint32_t a = *(const uint32_t *)(S), b = *(const uint32_t *)(S + 4), c = *(const uint32_t *)(S + 8);
        // bytes: a = p0.c0 p0.c1 p0.c2 p1.c0 | b = p1.c1 p1.c2 p2.c0 p2.c1 | c = p2.c2 p3.c0 p3.c1 p3.c2
        const uint32_t g0 = ((a & 255) * 9798 + ((a >> 8) & 255) * 19235 + ((a >> 16) & 255) * 3735 + (1 << 14)) >> 15;
        const uint32_t g1 = ((a >> 24) * 9798 + (b & 255) * 19235 + ((b >> 8) & 255) * 3735 + (1 << 14)) >> 15;
        const uint32_t g2 = (((b >> 16) & 255) * 9798 + (b >> 24) * 19235 + (c & 255) * 3735 + (1 << 14)) >> 15;
        const uint32_t g3 = (((c >> 8) & 255) * 9798 + ((c >> 16) & 255) * 19235 + (c >> 24) * 3735 + (1 << 14)) >> 15;
        *(uint32_t *)D = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    } else {
        for (int j = 0; x + j < cols; j++)
            D[j] = (uint8_t)bgr_gray(S[3 * j], S[3 * j + 1], S[3 * j + 2]);
    }
}

// transfer.rs:283-290 / omr.rs:88-92: cvtColor(COLOR_RGB2GRAY) 8U,
// (c0*9798 + c1*19235 + c2*3735 + 16384) >> 15 in memory order (quirk B8 kept).
__global__ __launch_bounds__(256) void rgb2gray_kernel(const uint8_t *__restrict__ src, int64_t sstep, int rows,
                                                       int cols, int cn, uint8_t *__restrict__ dst, int64_t dstep)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < cols) {
        const uint8_t *S = src + (int64_t)y * sstep + (int64_t)x * cn;
        dst[(int64_t)y * dstep + x] = (uint8_t)bgr_gray(S[0], S[1], S[2]);
    }
}

hipError_t launch_rgb2gray(const uint8_t *d_src, int64_t sstep, int rows, int cols, int cn, uint8_t *d_dst,
                           int64_t dstep, hipStream_t s)
{
    if (cn == 3 && (sstep & 3) == 0 && (dstep & 3) == 0 && ((uintptr_t)d_src & 3) == 0 && ((uintptr_t)d_dst & 3) == 0) {
        hipLaunchKernelGGL(rgb2gray3_x4_kernel, dim3((cols + 1023) / 1024, rows), dim3(256), 0, s, d_src, sstep, rows,
                           cols, d_dst, dstep);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(rgb2gray_kernel, dim3((cols + 255) / 256, rows), dim3(256), 0, s, d_src, sstep, rows, cols, cn,
                       d_dst, dstep);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// The same conversion for a batch (omr_rgb_to_gray_batch_device): n scans of one shape, 3 or 4 channels, in one launch,
// grid (tile, scan).  Any base address and any row pitch on either side: a lane owns the four destination pixels of one
// ALIGNED destination dword of a row -- group g of a row starts at pixel 4 g - (row address & 3) -- and reads the CN + 1
// aligned source dwords that cover their 4 CN bytes whatever the source's alignment, all of them issued before the first
// is used (4 or 5 dwords in flight per lane, consecutive lanes on consecutive groups: a wave reads one contiguous piece of a
// row), then shifts them into place with v_alignbyte_b32.  A covering dword that does not lie wholly inside the row's
// cols x CN bytes -- only the first and the last groups of a row can have one -- is put together from the bytes that do,
// and a group that is not wholly inside the row is done pixel by pixel: nothing outside a row is read or written.
#define GB_GROUPS 64  // groups (destination dwords) across a tile: one wave per row of a tile
#define GB_ROWS 16    // rows of a tile: four per lane

// the aligned dword at byte `off` of a row of `len` bytes, of which only the bytes inside the row are read
__device__ __forceinline__ uint32_t gb_load_inside(const uint8_t *__restrict__ row, int off, int len)
{
    if (off >= 0 && off + 4 <= len) return *(const uint32_t *)(row + off);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (off + k >= 0 && off + k < len) v |= (uint32_t)row[off + k] << (8 * k);
    return v;
}

template <int CN>
__global__ __launch_bounds__(256) void rgb2gray_batch_kernel(const uint8_t *__restrict__ src, int64_t sstride, int64_t sstep,
                                                             int rows, int cols, uint8_t *__restrict__ dst, int64_t dstride,
                                                             int64_t dstep, int tiles_x)
{
    constexpr int ND = CN + 1;  // aligned dwords that cover 4 CN bytes at any alignment
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int g = tx * GB_GROUPS + (int)(threadIdx.x & (GB_GROUPS - 1));
    const int r0 = ty * GB_ROWS + (int)(threadIdx.x / GB_GROUPS);
    const uint8_t *S0 = src + (int64_t)blockIdx.y * sstride;
    uint8_t *D0 = dst + (int64_t)blockIdx.y * dstride;
#pragma unroll
    for (int k = 0; k < GB_ROWS / 4; k++) {
        const int y = r0 + 4 * k;
        if (y >= rows) break;
        const uint8_t *srow = S0 + (int64_t)y * sstep;
        uint8_t *drow = D0 + (int64_t)y * dstep;
        const int x0 = 4 * g - (int)((uintptr_t)drow & 3u);
        if (x0 >= cols) continue;
        if (x0 >= 0 && x0 + 4 <= cols) {
            const int len = cols * CN;  // (cols < 32767: no overflow)
            const uint32_t sh = ((uint32_t)(uintptr_t)srow + (uint32_t)(x0 * CN)) & 3u;
            const int a0 = x0 * CN - (int)sh;  // the first covering dword, as a byte offset in the row: -3 at the least
            uint32_t w[ND];
            if (a0 >= 0 && a0 + 4 * ND <= len) {
#pragma unroll
                for (int j = 0; j < ND; j++) w[j] = *(const uint32_t *)(srow + a0 + 4 * j);
            } else {
#pragma unroll
                for (int j = 0; j < ND; j++) w[j] = gb_load_inside(srow, a0 + 4 * j, len);
            }
            uint32_t b[CN];  // the group's 4 CN bytes, in order
#pragma unroll
            for (int j = 0; j < CN; j++) b[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
            uint32_t g0, g1, g2, g3;
            if (CN == 3) {  // p0.c0 p0.c1 p0.c2 p1.c0 | p1.c1 p1.c2 p2.c0 p2.c1 | p2.c2 p3.c0 p3.c1 p3.c2
                g0 = bgr_gray(b[0] & 255u, (b[0] >> 8) & 255u, (b[0] >> 16) & 255u);
                g1 = bgr_gray(b[0] >> 24, b[1] & 255u, (b[1] >> 8) & 255u);
                g2 = bgr_gray((b[1] >> 16) & 255u, b[1] >> 24, b[2] & 255u);
                g3 = bgr_gray((b[2] >> 8) & 255u, (b[2] >> 16) & 255u, b[2] >> 24);
            } else {
                g0 = bgr_gray(b[0] & 255u, (b[0] >> 8) & 255u, (b[0] >> 16) & 255u);
                g1 = bgr_gray(b[1] & 255u, (b[1] >> 8) & 255u, (b[1] >> 16) & 255u);
                g2 = bgr_gray(b[2] & 255u, (b[2] >> 8) & 255u, (b[2] >> 16) & 255u);
                g3 = bgr_gray(b[CN - 1] & 255u, (b[CN - 1] >> 8) & 255u, (b[CN - 1] >> 16) & 255u);
            }
            *(uint32_t *)(drow + x0) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
        } else {  // the row begins or ends inside this group
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x = x0 + j;
                if (x >= 0 && x < cols) {
                    const uint8_t *P = srow + (int64_t)x * CN;
                    drow[x] = (uint8_t)bgr_gray(P[0], P[1], P[2]);
                }
            }
        }
    }
}

hipError_t launch_rgb2gray_batch(const uint8_t *d_src, int64_t sstride, int64_t sstep, int rows, int cols, int cn, int n,
                                 uint8_t *d_dst, int64_t dstride, int64_t dstep, hipStream_t s)
{
    // a row's first group may start up to 3 pixels before the row: (cols + 3) pixels in groups of 4
    const int tiles_x = ((cols + 6) / 4 + GB_GROUPS - 1) / GB_GROUPS, tiles_y = (rows + GB_ROWS - 1) / GB_ROWS;
    for (int i0 = 0; i0 < n; i0 += 65535) {  // (one launch for any batch a grid's y takes)
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(n - i0 < 65535 ? n - i0 : 65535));
        const uint8_t *S = d_src + (int64_t)i0 * sstride;
        uint8_t *D = d_dst + (int64_t)i0 * dstride;
        if (cn == 3)
            hipLaunchKernelGGL(rgb2gray_batch_kernel<3>, grid, dim3(256), 0, s, S, sstride, sstep, rows, cols, D, dstride, dstep, tiles_x);
        else
            hipLaunchKernelGGL(rgb2gray_batch_kernel<4>, grid, dim3(256), 0, s, S, sstride, sstep, rows, cols, D, dstride, dstep, tiles_x);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------
// erode(3x3 cross, iterations = 3, border = +inf), the three passes fused in LDS: a 64 x 16 output
// tile with a halo of 3; positions outside the image stay +inf (255) in every pass, exactly as
// three separate cv::erode calls would treat them.
#define ER_TW 64
#define ER_TH 16
#define ER_W (ER_TW + 6)
#define ER_H (ER_TH + 6)

__global__ __launch_bounds__(256) void erode3x_cross_kernel(const uint8_t *__restrict__ src, int64_t sstep, int rows,
                                                            int cols, uint8_t *__restrict__ dst, int64_t dstep)
{
    __shared__ uint8_t t0[ER_H][ER_W + 2], t1[ER_H][ER_W + 2];
    const int x0 = blockIdx.x * ER_TW - 3, y0 = blockIdx.y * ER_TH - 3;
    for (int i = threadIdx.x; i < ER_W * ER_H; i += 256) {
        const int ly = i / ER_W, lx = i - ly * ER_W;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool in = (unsigned)gx < (unsigned)cols && (unsigned)gy < (unsigned)rows;
        t0[ly][lx] = in ? src[(int64_t)gy * sstep + gx] : 255;
    }
    __syncthreads();
    // pass p shrinks the valid region by one on every side
    for (int pass = 1; pass <= 3; pass++) {
        uint8_t(*a)[ER_W + 2] = (pass & 1) ? t0 : t1;
        uint8_t(*b)[ER_W + 2] = (pass & 1) ? t1 : t0;
        const int w = ER_W - 2 * pass, h = ER_H - 2 * pass;
        for (int i = threadIdx.x; i < w * h; i += 256) {
            const int ly = pass + i / w, lx = pass + i % w;
            const int gx = x0 + lx, gy = y0 + ly;
            int m = 255;
            if ((unsigned)gx < (unsigned)cols && (unsigned)gy < (unsigned)rows)
                m = min(min((int)a[ly][lx], min((int)a[ly - 1][lx], (int)a[ly + 1][lx])),
                        min((int)a[ly][lx - 1], (int)a[ly][lx + 1]));
            b[ly][lx] = (uint8_t)m;
        }
        __syncthreads();
    }
    // after three passes the result sits in t1 (passes 1 and 3 write t1)
    for (int i = threadIdx.x; i < ER_TW * ER_TH; i += 256) {
        const int ly = i / ER_TW, lx = i - ly * ER_TW;
        const int gx = x0 + 3 + lx, gy = y0 + 3 + ly;
        if (gx < cols && gy < rows) dst[(int64_t)gy * dstep + gx] = t1[ly + 3][lx + 3];
    }
}

// The same filter at 4 pixels per lane.  Three passes of the 5-point minimum with a +inf border are one
// minimum over the L1 ball of radius 3 (in-image points only):
//     out(y, x) = min over dy in [-3, 3] of  h_{3 - |dy|}(y + dy, x),   h_r(y, x) = min over |dx| <= r of in(y, x + dx).
// Tile = 256 x 64 output pixels; its source rows (+3 halo rows, +1 halo dword either side, 255 outside the
// image) go to LDS with every load in flight at once.  A lane then owns one dword column (4 pixels) of a
// 16-row strip and walks down its 22 source rows: the eight byte pairs (p_d, p_{d+2}), d = -3..4, come out of
// the three dwords around the column with v_perm_b32 as zero-extended u16 pairs, so every minimum handles
// two pixels (v_pk_min_u16): 12 for h_1..h_3 of the even and the odd pixels, 12 for the seven running
// column minima that a source row feeds (row t closes output row t - 3).
#define E4_TW 64  // dword columns per tile
#define E4_SH 16  // output rows per strip
#define E4_NS 4   // strips per tile
#define E4_LW (E4_TW + 2)
#define E4_LH (E4_SH * E4_NS + 6)

__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__global__ __launch_bounds__(256) void erode3x_cross_x4_kernel(const uint8_t *__restrict__ src, int64_t sstep, int rows,
                                                               int cols, uint8_t *__restrict__ dst, int64_t dstep)
{
    __shared__ uint32_t tile[E4_LH][E4_LW + 1];
    const int qx0 = blockIdx.x * E4_TW - 1;          // first dword column of the tile (halo)
    const int y0 = blockIdx.y * (E4_SH * E4_NS) - 3;  // first source row of the tile (halo)
    for (int i = threadIdx.x; i < E4_LH * E4_LW; i += 256) {
        const int ly = i / E4_LW, lq = i - ly * E4_LW;
        const int gy = y0 + ly, gx = (qx0 + lq) * 4;
        uint32_t v = 0xffffffffu;
        if ((unsigned)gy < (unsigned)rows && gx >= 0 && gx < cols) {
            const uint8_t *S = src + (int64_t)gy * sstep + gx;
            if (gx + 4 <= cols) {
                v = *(const uint32_t *)S;
            } else {  // the row ends inside this dword: pixels past the end stay +inf
                for (int j = 0; gx + j < cols; j++) v = (v & ~(255u << (8 * j))) | ((uint32_t)S[j] << (8 * j));
            }
        }
        tile[ly][lq] = v;
    }
    __syncthreads();
    const int lq = threadIdx.x & (E4_TW - 1), strip = threadIdx.x / E4_TW;
    const int gx = (qx0 + 1 + lq) * 4;
    const int oy0 = blockIdx.y * (E4_SH * E4_NS) + strip * E4_SH;
    if (gx >= cols || oy0 >= rows) return;
    uint32_t aE[6], aO[6];  // running minima of output rows t - 2 .. t + 3 (t = source row being read)
#pragma unroll
    for (int i = 0; i < 6; i++) aE[i] = aO[i] = 0x00ff00ffu;
#pragma unroll
    for (int t = 0; t < E4_SH + 6; t++) {  // source row oy0 - 3 + t
        const uint32_t *T = &tile[strip * E4_SH + t][lq];
        const uint32_t L = T[0], C = T[1], R = T[2];
        const uint32_t Pm3 = __builtin_amdgcn_perm(L, L, 0x0c030c01u), Pm2 = __builtin_amdgcn_perm(C, L, 0x0c040c02u);
        const uint32_t Pm1 = __builtin_amdgcn_perm(C, L, 0x0c050c03u), P0 = C & 0x00ff00ffu;
        const uint32_t P1 = __builtin_amdgcn_perm(C, C, 0x0c030c01u), P2 = __builtin_amdgcn_perm(R, C, 0x0c040c02u);
        const uint32_t P3 = __builtin_amdgcn_perm(R, C, 0x0c050c03u), P4 = R & 0x00ff00ffu;
        const uint32_t h1E = pk_min(pk_min(Pm1, P0), P1), h1O = pk_min(pk_min(P0, P1), P2);
        const uint32_t h2E = pk_min(pk_min(h1E, Pm2), P2), h2O = pk_min(pk_min(h1O, Pm1), P3);
        const uint32_t h3E = pk_min(pk_min(h2E, Pm3), P3), h3O = pk_min(pk_min(h2O, Pm2), P4);
        // source row t feeds output rows t-3 (h0, closes it), t-2 (h1), t-1 (h2), t (h3), t+1 (h2), t+2 (h1), t+3 (h0)
        const uint32_t oE = pk_min(aE[0], P0), oO = pk_min(aO[0], P1);
        aE[0] = pk_min(aE[1], h1E), aO[0] = pk_min(aO[1], h1O);
        aE[1] = pk_min(aE[2], h2E), aO[1] = pk_min(aO[2], h2O);
        aE[2] = pk_min(aE[3], h3E), aO[2] = pk_min(aO[3], h3O);
        aE[3] = pk_min(aE[4], h2E), aO[3] = pk_min(aO[4], h2O);
        aE[4] = pk_min(aE[5], h1E), aO[4] = pk_min(aO[5], h1O);
        aE[5] = P0, aO[5] = P1;
        if (t >= 6) {
            const int oy = oy0 + t - 6;
            if (oy < rows) {
                const uint32_t out = oE | (oO << 8);
                uint8_t *D = dst + (int64_t)oy * dstep + gx;
                if (gx + 4 <= cols && (((uintptr_t)D) & 3) == 0) {
                    *(uint32_t *)D = out;
                } else {
                    for (int j = 0; gx + j < cols && j < 4; j++) D[j] = (uint8_t)(out >> (8 * j));
                }
            }
        }
    }
}

hipError_t launch_erode3x_cross(const uint8_t *d_src, int64_t sstep, int rows, int cols, uint8_t *d_dst, int64_t dstep,
                                hipStream_t s)
{
    if ((sstep & 3) == 0 && ((uintptr_t)d_src & 3) == 0) {
        hipLaunchKernelGGL(erode3x_cross_x4_kernel,
                           dim3((cols + 4 * E4_TW - 1) / (4 * E4_TW), (rows + E4_SH * E4_NS - 1) / (E4_SH * E4_NS)), dim3(256),
                           0, s, d_src, sstep, rows, cols, d_dst, dstep);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(erode3x_cross_kernel, dim3((cols + ER_TW - 1) / ER_TW, (rows + ER_TH - 1) / ER_TH), dim3(256), 0,
                       s, d_src, sstep, rows, cols, d_dst, dstep);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// transfer.rs:294-301 / omr.rs:129-139: threshold(127, 255, THRESH_BINARY), one pixel per lane
__global__ __launch_bounds__(256) void threshold_kernel(const uint8_t *__restrict__ src, int64_t sstep, int rows,
                                                        int cols, uint8_t *__restrict__ dst, int64_t dstep,
                                                        int thresh, int maxval)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < cols) dst[(int64_t)y * dstep + x] = (int)src[(int64_t)y * sstep + x] > thresh ? (uint8_t)maxval : 0;
}

// the same, 16 pixels per lane
__global__ __launch_bounds__(256) void threshold_x16_kernel(const uint8_t *__restrict__ src, int64_t sstep, int rows,
                                                            int cols, uint8_t *__restrict__ dst, int64_t dstep,
                                                            int thresh, int maxval)
{
    const int q = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int x = q * 16;
    if (x >= cols) return;
    const uint8_t *S = src + (int64_t)y * sstep + x;
    uint8_t *D = dst + (int64_t)y * dstep + x;
    if (x + 16 <= cols) {
        const uint4 v = *(const uint4 *)S;
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t r = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) r |= ((int)((in[k] >> (8 * j)) & 255) > thresh ? (uint32_t)maxval : 0u) << (8 * j);
            o[k] = r;
        }
        *(uint4 *)D = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        for (int j = 0; x + j < cols; j++) D[j] = (int)S[j] > thresh ? (uint8_t)maxval : 0;
    }
}

hipError_t launch_threshold(const uint8_t *d_src, int64_t sstep, int rows, int cols, uint8_t *d_dst, int64_t dstep,
                            int thresh, int maxval, hipStream_t s)
{
    if ((sstep & 15) == 0 && (dstep & 15) == 0 && ((uintptr_t)d_src & 15) == 0 && ((uintptr_t)d_dst & 15) == 0) {
        hipLaunchKernelGGL(threshold_x16_kernel, dim3((cols + 4095) / 4096, rows), dim3(256), 0, s, d_src, sstep, rows,
                           cols, d_dst, dstep, thresh, maxval);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(threshold_kernel, dim3((cols + 255) / 256, rows), dim3(256), 0, s, d_src, sstep, rows, cols,
                       d_dst, dstep, thresh, maxval);
    return hipGetLastError();
}

}  // namespace omr
