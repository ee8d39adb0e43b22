// correct_front.hip -- the front end of correct_default (omr.rs:87-126) for a batch of same-shape sheets, one launch
// per stage:
//
//   front_kernel      gray (cvtColor(COLOR_RGB2GRAY) on BGR bytes, quirk B8, bgr.hpp's arithmetic) + erode(3x3 cross,
//                     iterations = 3) + -- when the shrink is an integer factor -- INTER_AREA's resizeAreaFast_, fused:
//                     every sheet is read once and only its projection-size image is written.  Other resizes: the
//                     eroded gray sheets are written and resize.hip takes over, one launch per chunk.
//
// Arithmetic is the per-call stage kernels' (stages.hip, resize.hip) operation for operation, so the images are the
// per-call path's bit for bit.
#include <hip/hip_runtime.h>

#include "bgr.hpp"
#include "kernels.hpp"
#include "warp_fixed.hpp"

namespace omr {

__device__ __forceinline__ uint32_t cb_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// One workgroup = one tile of one sheet (blockIdx.z).  The tile is EW x EH eroded pixels (EW <= 256: one column per lane);
// its gray values with a halo of 3 (255 outside the sheet: the erosion's +inf border) are staged in LDS as bytes.  Three
// passes of the 5-point minimum are one minimum over the L1 ball of radius 3 (erode3x_cross_x4_kernel): a lane walks down
// its column, forms h_1..h_3 (horizontal minima of radius r) of every source row and keeps the seven running column minima
// in registers; source row t closes eroded row t - 6 of the tile.
//   area (kx, ky >= 1): a lane adds its column's eroded values over ky rows; after the barrier a lane per output pixel adds
//                       kx of those column sums and rounds as resizeAreaFast_ (resize_area_int_colsum_kernel).  The tile is
//                       TWo x THo output pixels, EW = TWo kx, EH = THo ky.
//   eroded (kx = 0):    the eroded rows go straight to `dst` (full size).
__global__ __launch_bounds__(256) void front_kernel(const uint8_t *__restrict__ src, int64_t scan_stride, int64_t sstep, int cn,
                                                    int rows, int cols, uint8_t *__restrict__ dst, int64_t out_stride,
                                                    int64_t dstep, int kx, int ky, int TWo, int THo, int EW, int EH)
{
    extern __shared__ uint32_t cb_lds[];
    const int GW = EW + 6, GH = EH + 6;
    uint8_t *gt = (uint8_t *)cb_lds;                      // [GH][GW] gray with halo
    uint32_t *colsum = cb_lds + ((GW * GH + 3) >> 2);     // [THo][EW] (area mode)
    const uint8_t *S = src + (int64_t)blockIdx.z * scan_stride;
    const int ex0 = blockIdx.x * EW, ey0 = blockIdx.y * EH;  // first eroded pixel of the tile (sheet coordinates)
    for (int i = threadIdx.x; i < GW * GH; i += 256) {
        const int ly = i / GW, lx = i - ly * GW;
        const int gy = ey0 - 3 + ly, gx = ex0 - 3 + lx;
        uint32_t v = 255;
        if ((unsigned)gy < (unsigned)rows && (unsigned)gx < (unsigned)cols) {
            const uint8_t *P = S + (int64_t)gy * sstep + (int64_t)gx * cn;
            v = cn == 1 ? (uint32_t)P[0] : bgr_gray(P[0], P[1], P[2]);
        }
        gt[i] = (uint8_t)v;
    }
    __syncthreads();
    const int c = threadIdx.x;
    const bool area = kx > 0;
    if (c < EW) {
        uint32_t a[6];
#pragma unroll
        for (int i = 0; i < 6; i++) a[i] = 255;
        uint32_t acc = 0;
        const int gx = ex0 + c;
        uint8_t *D = dst + (int64_t)blockIdx.z * out_stride;
        for (int t = 0; t < GH; t++) {
            const uint8_t *T = gt + t * GW + c;  // T[3] = the column's own pixel
            const uint32_t pm3 = T[0], pm2 = T[1], pm1 = T[2], p0 = T[3], p1 = T[4], p2 = T[5], p3 = T[6];
            const uint32_t h1 = cb_min(cb_min(pm1, p0), p1);
            const uint32_t h2 = cb_min(cb_min(h1, pm2), p2);
            const uint32_t h3 = cb_min(cb_min(h2, pm3), p3);
            const uint32_t o = cb_min(a[0], p0);
            a[0] = cb_min(a[1], h1);
            a[1] = cb_min(a[2], h2);
            a[2] = cb_min(a[3], h3);
            a[3] = cb_min(a[4], h2);
            a[4] = cb_min(a[5], h1);
            a[5] = p0;
            if (t >= 6) {
                const int e = t - 6;  // eroded row of the tile
                if (area) {
                    acc += o;
                    if ((e + 1) % ky == 0) {
                        colsum[(e / ky) * EW + c] = acc;
                        acc = 0;
                    }
                } else {
                    const int gy = ey0 + e;
                    if (gy < rows && gx < cols) D[(int64_t)gy * dstep + gx] = (uint8_t)o;
                }
            }
        }
    }
    if (!area) return;
    __syncthreads();
    const int dr = rows / ky, dc = cols / kx;
    uint8_t *D = dst + (int64_t)blockIdx.z * out_stride;
    for (int i = threadIdx.x; i < TWo * THo; i += 256) {
        const int ly = i / TWo, lx = i - ly * TWo;
        const int oy = blockIdx.y * THo + ly, ox = blockIdx.x * TWo + lx;
        if (oy >= dr || ox >= dc) continue;
        int sum = 0;
        for (int j = 0; j < kx; j++) sum += (int)colsum[ly * EW + lx * kx + j];
        uint8_t out;
        if (kx == 2 && ky == 2) out = (uint8_t)((sum + 2) >> 2);
        else out = sat_u8((int)rintf((float)sum * (1.f / (float)(kx * ky))));
        D[(int64_t)oy * dstep + ox] = out;
    }
}

// Tile shape of front_kernel for integer factors kx, ky (kx = 0: full-size eroded output) and its LDS bytes.
void front_tile(int kx, int ky, int *TWo, int *THo, int *EW, int *EH)
{
    if (kx <= 0) {
        *TWo = *THo = 0;
        *EW = 256;
        *EH = 64;
        return;
    }
    *TWo = 256 / kx;
    *THo = 64 / ky < 1 ? 1 : (64 / ky > 16 ? 16 : 64 / ky);
    *EW = *TWo * kx;
    *EH = *THo * ky;
}

size_t front_lds_bytes(int kx, int ky)
{
    int TWo, THo, EW, EH;
    front_tile(kx, ky, &TWo, &THo, &EW, &EH);
    const size_t gray = (((size_t)(EW + 6) * (EH + 6) + 3) >> 2) * 4;
    return gray + (kx > 0 ? sizeof(uint32_t) * (size_t)THo * EW : 0);
}

hipError_t launch_front(const uint8_t *d_src, int64_t scan_stride, int64_t sstep, int cn, int rows, int cols, int n,
                        uint8_t *d_dst, int64_t out_stride, int64_t dstep, int kx, int ky, hipStream_t s)
{
    if ((cn != 1 && cn != 3) || n <= 0 || (kx > 0 && (kx > 64 || ky <= 0 || ky > 64))) return hipErrorInvalidValue;
    int TWo, THo, EW, EH;
    front_tile(kx, ky, &TWo, &THo, &EW, &EH);
    const size_t lds = front_lds_bytes(kx, ky);
    dim3 grid;
    if (kx > 0) grid = dim3((cols / kx + TWo - 1) / TWo, (rows / ky + THo - 1) / THo, n);
    else grid = dim3((cols + EW - 1) / EW, (rows + EH - 1) / EH, n);
    hipLaunchKernelGGL(front_kernel, grid, dim3(256), lds, s, d_src, scan_stride, sstep, cn, rows, cols, d_dst, out_stride, dstep,
                       kx, ky, TWo, THo, EW, EH);
    return hipGetLastError();
}

}  // namespace omr
