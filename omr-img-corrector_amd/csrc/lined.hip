// lined.hip -- the line picture of the Hough and FFT detectors (hough.rs:44-63, fft.rs:173-213) for one edge map or a
// batch: cvtColor(GRAY2BGR) of the edge map with every HoughLinesP segment drawn on by
// imgproc::line(.., Scalar(186, 88, 255), 1, LINE_AA, 0), in list order.  OpenCV 4.6.0 drawing.cpp, LineAA(), restated
// for 8-bit BGR, thickness 1, shift 0 (tests/lined_ref.py holds the statement-by-statement form and this closed form):
//
//   LineAA walks E + 1 steps along the major axis.  Step k (scount = k, ecount = E - k) sits at the major coordinate
//   m0 + k and the minor 16.16 value v = v0 + k * step; it blends the three pixels (v >> 16) - 1 .. + 1 of the minor axis
//   with a = (ep_corr * FilterTable[..] >> 8) & 0xff, FilterTable indexed by dist = (v >> 11) & 31, and ep_corr taken
//   from ep_table[min(k, 2) * 3 + min(E - k, 2)].  All of it is a function of k alone: a step can be taken from any
//   starting point, so a segment clipped to a tile paints exactly what the un-clipped walk paints there.  The steps
//   of one segment touch disjoint pixels; LINE_AA blends into what is there, so SEGMENTS must keep their order.
//
//   lined_prepare_kernel  a thread per segment: (x0, y0, x1, y1) -> LinedSeg (the swap, the truncating division of the
//                         step, SlopeCorrTable); an end point outside the picture raises the flag the host refuses on
//   lined_draw_kernel     a workgroup per 128 x 128 pixels of a picture, a wavefront per 64 x 64 tile of them, the tile
//                         in LDS as BGR bytes (GRAY2BGR fused into the fill).  The workgroup passes over the picture's
//                         segments 256 at a time, keeps those that reach its pixels -- the exact test: the major range
//                         clipped to the workgroup, the minor values at the two clipped ends +- 1 -- in an LDS list in
//                         segment order (ballot + prefix: no atomics), and whenever the list fills or the segments end
//                         every wave walks the list in order, lane = step.  Then the tile leaves as aligned dwords.
//
// LDS rows are 49 dwords apart (48 of pixels): lanes that step along x are 3 bytes apart, lanes that step along y 49
// dwords, an odd count, so neither collides on the 32 banks of a byte or dword access.  A wave owns its tile: a
// wave's LDS operations complete in order, so the walk needs no barrier; the fences keep the compiler from moving one
// segment's accesses across the next one's.
//
// Dword stores need the picture's base and pitch to be multiples of 4; any other layout, and a row's last partial
// dword, go byte by byte.  Nothing is written past 3 * cols: the caller's pitch padding stays as it was.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace omr {
namespace {

constexpr int LT = 64;              // tile side = lanes of a wavefront
constexpr int LT_DWORDS = 48;       // a tile row of BGR bytes
constexpr int LT_PITCH = 49;        // LDS row pitch in dwords
constexpr int LS = 2 * LT;          // side of a workgroup's 2 x 2 tiles
constexpr int LCAP = 1024;          // entries of the segment list; drained when fewer than 256 are free

// drawing.cpp: SlopeCorrTable
__device__ const uint8_t kSlopeCorr[32] = {181, 181, 181, 182, 182, 183, 184, 185, 187, 188, 190, 192, 194, 196, 198, 201,
                                           203, 206, 209, 211, 214, 218, 221, 224, 227, 231, 235, 238, 242, 246, 250, 254};
// drawing.cpp: FilterTable
__device__ const uint8_t kFilter[64] = {168, 177, 185, 194, 202, 210, 218, 224, 231, 236, 241, 246, 249, 252, 254, 254,
                                        254, 254, 252, 249, 246, 241, 236, 231, 224, 218, 210, 202, 194, 185, 177, 168,
                                        158, 149, 140, 131, 122, 114, 105, 99,  91,  85,  79,  72,  67,  61,  56,  51,
                                        46,  42,  38,  34,  30,  27,  24,  21,  18,  16,  14,  12,  10,  8,   7,   6};

__global__ __launch_bounds__(256) void lined_prepare_kernel(const int32_t *lines, int64_t count, int rows, int cols,
                                                            LinedSeg *segs, int32_t *bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    int x0 = lines[4 * i], y0 = lines[4 * i + 1], x1 = lines[4 * i + 2], y1 = lines[4 * i + 3];
    LinedSeg sg{};
    if ((unsigned)x0 >= (unsigned)cols || (unsigned)x1 >= (unsigned)cols || (unsigned)y0 >= (unsigned)rows ||
        (unsigned)y1 >= (unsigned)rows) {
        atomicOr(bad, 1);
        sg.e = -1;  // no step
        segs[i] = sg;
        return;
    }
    const int ax = abs(x1 - x0), ay = abs(y1 - y0);
    const bool xm = ax > ay;
    // the major axis runs upwards: LineAA swaps the end points when it does not
    if (xm ? x1 < x0 : y1 < y0) {
        int t = x0;
        x0 = x1, x1 = t;
        t = y0, y0 = y1, y1 = t;
    }
    const int dn = xm ? y1 - y0 : x1 - x0, am = xm ? ax : ay;
    // x_step / y_step = (d << XY_SHIFT) / (a | 1) on 16.16 values: C's division truncates towards zero
    const int64_t step = ((int64_t)dn * (1ll << 32)) / ((((int64_t)am) << 16) | 1);
    int slope = (int)(step >> 11) & 0x3f;
    slope ^= step < 0 ? 0x3f : 0;
    slope = (slope & 0x20) ? 0x100 : kSlopeCorr[slope];
    sg.m0 = xm ? x0 : y0;
    sg.e = am + 1;  // pt2 += XY_ONE: the walk runs one pixel past the end point
    sg.step = (int32_t)step;
    sg.slope_x = slope | (xm ? 1 << 16 : 0);
    sg.v0 = ((int64_t)(xm ? y0 : x0) << 16) + (1 << 15);
    segs[i] = sg;
}

// does a step of `sg` paint into the square of `side` pixels at (X0, Y0)?
__device__ __forceinline__ bool reaches(const LinedSeg &sg, int X0, int Y0, int side)
{
    const bool xm = sg.slope_x >> 16;
    const int M0 = xm ? X0 : Y0, N0 = xm ? Y0 : X0;
    const int klo = max(0, M0 - sg.m0), khi = min(sg.e, M0 + side - 1 - sg.m0);
    if (klo > khi) return false;
    // the minor value is linear in k: its extremes over [klo, khi] are at the ends; a step paints +-1 around it
    const int64_t va = sg.v0 + (int64_t)klo * sg.step, vb = sg.v0 + (int64_t)khi * sg.step;
    const int lo = (int)(min(va, vb) >> 16) - 1, hi = (int)(max(va, vb) >> 16) + 1;
    return hi >= N0 && lo < N0 + side;
}

// ICV_PUT_POINT: the blend runs twice per channel
__device__ __forceinline__ void put_point(uint8_t *q, uint32_t bgr, int a)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int col = (bgr >> (8 * c)) & 0xff;
        int v = q[c];
        v += ((col - v) * a + 127) >> 8;
        v += ((col - v) * a + 127) >> 8;
        q[c] = (uint8_t)v;
    }
}

__global__ __launch_bounds__(256) void lined_draw_kernel(LinedImg p, const LinedSeg *segs, const int32_t *off)
{
    __shared__ uint32_t tiles[4][LT * LT_PITCH];
    __shared__ int32_t list[LCAP];
    __shared__ int32_t wtot[4];
    __shared__ uint8_t filt[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int X0 = blockIdx.x * LS, Y0 = blockIdx.y * LS;
    const int sx = X0 + (wave & 1) * LT, sy = Y0 + (wave >> 1) * LT;
    const int rows = p.rows, cols = p.cols;
    const bool live = sx < cols && sy < rows;  // a wave whose tile lies outside the picture only helps with the list
    const uint8_t *S = p.src + (int64_t)blockIdx.z * p.sstride;
    uint8_t *D = p.dst + (int64_t)blockIdx.z * p.dstride;
    uint32_t *tile = tiles[wave];
    uint8_t *tile_b = reinterpret_cast<uint8_t *>(tile);

    if (tid < 64) filt[tid] = kFilter[tid];
    if (live)  // GRAY2BGR: byte b of the row's dword d belongs to pixel (4 d + b) / 3
        for (int idx = lane; idx < LT * LT_DWORDS; idx += 64) {
            const int r = idx / LT_DWORDS, d = idx - r * LT_DWORDS, y = sy + r;
            uint32_t w = 0;
            if (y < rows) {
                const uint8_t *srow = S + (int64_t)y * p.sstep;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int x = sx + (4 * d + b) / 3;
                    if (x < cols) w |= (uint32_t)srow[x] << (8 * b);
                }
            }
            tile[r * LT_PITCH + d] = w;
        }
    __syncthreads();

    const int s0 = off[blockIdx.z], s1 = off[blockIdx.z + 1];
    int count = 0;  // list entries, the same in every thread
    for (int base = s0; base < s1; base += 256) {
        const int i = base + tid;
        const bool hit = i < s1 && reaches(segs[i], X0, Y0, LS);
        const unsigned long long votes = __ballot(hit);
        if (lane == 0) wtot[wave] = __popcll(votes);
        __syncthreads();
        int before = count, total = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wave) before += wtot[w];
            total += wtot[w];
        }
        if (hit) list[before + __popcll(votes & ((1ull << lane) - 1))] = i;
        count += total;
        __syncthreads();
        if (count <= LCAP - 256 && base + 256 < s1) continue;
        // every wave walks the list in order on its own tile
        if (live)
            for (int e = 0; e < count; e++) {
                const LinedSeg sg = segs[__builtin_amdgcn_readfirstlane(list[e])];
                const bool xm = sg.slope_x >> 16;
                const int slope = sg.slope_x & 0xffff;
                const int N0 = xm ? sy : sx;
                const int m = (xm ? sx : sy) + lane, k = m - sg.m0;
                if (k >= 0 && k <= sg.e && m < (xm ? cols : rows)) {
                    const int64_t v = sg.v0 + (int64_t)k * sg.step;
                    const int n = (int)(v >> 16) - 1, dist = (int)(v >> 11) & 31;
                    // ep_table for end points without a fraction (shift 0), row min(scount, 2), column min(ecount, 2):
                    // {0, 4, 124; 4, 132, 252; 4, 132, 256} * slope >> 8
                    const int r = min(k, 2), c = min(sg.e - k, 2);
                    const int mult = c == 0 ? (r == 0 ? 0 : 4) : c == 1 ? (r == 0 ? 4 : 132) : (r == 0 ? 124 : r == 1 ? 252 : 256);
                    const int ep = (mult * slope >> 8) & 0x1ff;
                    const int nend = min(N0 + LT, xm ? rows : cols);
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const int f = filt[j == 0 ? dist + 32 : j == 1 ? dist : 63 - dist];
                        const int a = (ep * f >> 8) & 0xff, nn = n + j;
                        if (nn >= N0 && nn < nend) {
                            const int px = xm ? lane : nn - N0, py = xm ? nn - N0 : lane;
                            put_point(tile_b + py * (LT_PITCH * 4) + px * 3, p.bgr, a);
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        count = 0;
        __syncthreads();  // the list is free again
    }

    if (!live) return;
    const bool ddw = (((uintptr_t)D | (uintptr_t)p.dstep) & 3) == 0;
    const int row_bytes = 3 * cols;
    for (int idx = lane; idx < LT * LT_DWORDS; idx += 64) {
        const int r = idx / LT_DWORDS, d = idx - r * LT_DWORDS, y = sy + r;
        const int bo = 3 * sx + 4 * d;  // 3 * sx is a multiple of 192
        if (y >= rows || bo >= row_bytes) continue;
        const uint32_t w = tile[r * LT_PITCH + d];
        uint8_t *drow = D + (int64_t)y * p.dstep;
        if (ddw && bo + 4 <= row_bytes) {
            *reinterpret_cast<uint32_t *>(drow + bo) = w;
        } else {
            for (int b = 0; b < 4; b++)
                if (bo + b < row_bytes) drow[bo + b] = (uint8_t)(w >> (8 * b));
        }
    }
}

}  // namespace

hipError_t launch_lined_prepare(const int32_t *d_lines, int64_t count, int rows, int cols, LinedSeg *d_segs, int32_t *d_bad,
                                hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    if (count > (int64_t)0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lined_prepare_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, d_lines, count, rows, cols,
                       d_segs, d_bad);
    return hipGetLastError();
}

hipError_t launch_lined_draw(const LinedImg &p, const LinedSeg *d_segs, const int32_t *d_off, hipStream_t s)
{
    if (p.n < 1 || p.n > 65535 || p.rows < 1 || p.cols < 1) return hipErrorInvalidValue;
    const dim3 grid((p.cols + LS - 1) / LS, (p.rows + LS - 1) / LS, p.n);
    hipLaunchKernelGGL(lined_draw_kernel, grid, dim3(256), 0, s, p, d_segs, d_off);
    return hipGetLastError();
}

}  // namespace omr
