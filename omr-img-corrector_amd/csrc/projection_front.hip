// projection_front.hip -- scale_self (transfer.rs:66-91), the first stage of get_angle_with_projections
// (projection.rs:24-27), for a batch of same-shape scans of 1 or 3 interleaved 8-bit channels: one launch per stage,
// the image index in blockIdx.z.
//
//   pf_area_tile_kernel<true>    INTER_AREA, integer factors: resizeAreaFast_ (resize_area_int_kernel's arithmetic)
//   pf_area_tile_kernel<false>   INTER_AREA, any other shrink: resizeArea_<uchar,float> with the context's tap tables
//                                (resize_area_general_kernel's float operations in its order)
//   pf_area_direct_kernel        both, one thread per destination byte straight from memory: only when the source
//                                segment of a single destination pixel does not fit the LDS budget
//   pf_linear_kernel             INTER_LINEAR (scale > 1): resize_linear_kernel with the image index added
//
// The per-call kernels give a thread one destination byte, so neighbouring lanes read the source cn / scale bytes
// apart; on a colour A4 scan that gather is the whole cost.  The tile kernel turns it round: a workgroup owns a tile of
// destination columns, reads the source rows under it as contiguous, aligned dword segments into LDS (a few rows at a
// time), applies the horizontal taps of a source row once per lane from LDS and keeps the vertical accumulation in
// registers, walking down the tile.  Every scan byte is read from memory once (a tile's first source row may be shared
// with the tile above).  The order of the float operations per destination byte is the per-call kernel's, so the
// images are its images bit for bit; the file is built with the same -ffp-contract=off.
// When the scan pointer, scan_stride_bytes or step_bytes is not a multiple of 4 the segments are staged byte by byte:
// same result, slower.
#include <hip/hip_runtime.h>

#include "projection_front.hpp"
#include "resize_linear.hpp"
#include "warp_fixed.hpp"

namespace omr {

#define PF_THREADS 256
#define PF_LDS_DWORDS 4096  // 16 KB of staged source rows per workgroup
#define PF_TILE_ROWS 16     // destination rows per workgroup
#define PF_MAX_CHUNK 16     // source rows staged at once
#define PF_REG_TAPS 8       // horizontal weights a lane keeps in registers (the rest come from the table)

// floor(i / d) for i * d < 2^32, d >= 2, with m = ceil(2^32 / d)
__device__ __forceinline__ uint32_t pf_div(uint32_t i, uint32_t m) { return __umulhi(i, m); }

template <bool INT>
__global__ __launch_bounds__(PF_THREADS) void pf_area_tile_kernel(PfArea p, int twp, int th, int segd, int chunk, int aligned)
{
    extern __shared__ uint32_t pf_lds[];  // [chunk][segd]: source rows r0 .. r0 + nr - 1, bytes `base` .. of each
    const int cn = p.cn;
    const int p0 = blockIdx.x * twp, p1 = min(p0 + twp, p.dcols);    // destination pixels of the tile
    const int dy0 = blockIdx.y * th, dy1 = min(dy0 + th, p.drows);  // destination rows of the tile
    const uint8_t *S = p.src + (int64_t)blockIdx.z * p.scan_stride;
    const int row_bytes = p.scols * cn;
    // source bytes [seg_lo, seg_hi) of a row and source rows [r, r_end) under the tile; j walks the vertical taps
    int seg_lo, seg_hi, j, r, r_end;
    if (INT) {
        seg_lo = p0 * p.kx * cn, seg_hi = p1 * p.kx * cn;
        j = dy0 * p.ky, r = j, r_end = dy1 * p.ky;
    } else {
        seg_lo = p.xtab[p.xofs[p0]].si, seg_hi = p.xtab[p.xofs[p1] - 1].si + cn;
        j = p.yofs[dy0], r = p.ytab[j].si, r_end = p.ytab[p.yofs[dy1] - 1].si + 1;
    }
    const int base = aligned ? (seg_lo & ~3) : seg_lo;
    const int nd = (seg_hi - base + 3) >> 2;  // dwords of a staged row (<= segd)
    const uint32_t nd_m = nd > 1 ? (uint32_t)(((1ull << 32) + (uint32_t)nd - 1) / (uint32_t)nd) : 0;

    // the lane's destination byte and its horizontal taps
    const int t = threadIdx.x;
    const int lp = cn == 3 ? t / 3 : t, c = t - lp * cn;
    const bool active = lp < p1 - p0;
    int x0 = 0, nt = 0, off = 0;
    float a[PF_REG_TAPS];
#pragma unroll
    for (int k = 0; k < PF_REG_TAPS; k++) a[k] = 0.f;
    if (active) {
        if (INT) {
            nt = p.kx;
            off = (p0 + lp) * p.kx * cn + c - base;
        } else {
            x0 = p.xofs[p0 + lp];
            nt = p.xofs[p0 + lp + 1] - x0;
            off = p.xtab[x0].si + c - base;  // a destination pixel's taps are consecutive source pixels
#pragma unroll
            for (int k = 0; k < PF_REG_TAPS; k++)
                if (k < nt) a[k] = p.xtab[x0 + k].alpha;
        }
    }
    int dy = dy0;
    int jend = INT ? (dy0 + 1) * p.ky : p.yofs[dy0 + 1];
    float sum = 0.f;
    int isum = 0;
    bool first = true;
    uint8_t *D = p.dst + (int64_t)blockIdx.z * p.out_stride + (int64_t)p0 * cn + t;

    for (; r < r_end; r += chunk) {
        const int nr = min(chunk, r_end - r);
        const uint8_t *G = S + (int64_t)r * p.sstep + base;
        for (int i = t; i < nr * nd; i += PF_THREADS) {
            const int ly = nd > 1 ? (int)pf_div((uint32_t)i, nd_m) : i, q = i - ly * nd;
            const uint8_t *P = G + (int64_t)ly * p.sstep + q * 4;
            uint32_t v;
            if (aligned && base + q * 4 + 4 <= row_bytes) {
                v = *(const uint32_t *)P;
            } else {  // byte-wise staging, and the dword that would cross the end of the row
                v = 0;
                for (int b = 0; b < 4; b++)
                    if (base + q * 4 + b < seg_hi) v |= (uint32_t)P[b] << (8 * b);
            }
            pf_lds[ly * segd + q] = v;
        }
        __syncthreads();
        if (active) {
            const int rlim = r + nr;
            while (dy < dy1) {
                if (j == jend) {  // the destination row is complete
                    uint8_t out;
                    if (INT) {
                        if (p.kx == 2 && p.ky == 2) out = (uint8_t)((isum + 2) >> 2);
                        else out = sat_u8((int)rintf((float)isum * (1.f / (float)(p.kx * p.ky))));
                    } else {
                        out = sat_u8((int)rintf(sum));
                    }
                    D[(int64_t)dy * p.dstep] = out;
                    dy++;
                    if (dy < dy1) jend = INT ? (dy + 1) * p.ky : p.yofs[dy + 1];
                    sum = 0.f, isum = 0, first = true;
                    continue;
                }
                const int si = INT ? j : p.ytab[j].si;
                if (si >= rlim) break;  // in the next chunk
                const uint8_t *row = (const uint8_t *)(pf_lds + (si - r) * segd) + off;
                if (INT) {
                    for (int k = 0; k < nt; k++) isum += row[k * cn];
                } else {
                    const float beta = p.ytab[j].alpha;
                    float buf = 0.f;
#pragma unroll
                    for (int k = 0; k < PF_REG_TAPS; k++)
                        if (k < nt) buf += (float)row[k * cn] * a[k];
                    for (int k = PF_REG_TAPS; k < nt; k++) buf += (float)row[k * cn] * p.xtab[x0 + k].alpha;
                    if (first) {
                        sum = beta * buf;  // ResizeArea_Invoker assigns on the first tap of a destination row
                        first = false;
                    } else {
                        sum += beta * buf;
                    }
                }
                j++;
            }
        }
        __syncthreads();
    }
}

// One thread per destination byte, no staging: resize_area_int_kernel's full-block branch (integer factors always
// divide both sizes here) and resize_area_general_kernel with the image index added.
template <bool INT>
__global__ __launch_bounds__(PF_THREADS) void pf_area_direct_kernel(PfArea p)
{
    const int dxb = blockIdx.x * PF_THREADS + threadIdx.x, dy = blockIdx.y;
    if (dxb >= p.dcols * p.cn) return;
    const int dx = dxb / p.cn, c = dxb - dx * p.cn;
    const uint8_t *Sz = p.src + (int64_t)blockIdx.z * p.scan_stride;
    uint8_t out;
    if (INT) {
        const uint8_t *S = Sz + (int64_t)dy * p.ky * p.sstep + (int64_t)dx * p.kx * p.cn + c;
        int sum = 0;
        for (int sy = 0; sy < p.ky; sy++)
            for (int sx = 0; sx < p.kx; sx++) sum += S[(int64_t)sy * p.sstep + sx * p.cn];
        if (p.kx == 2 && p.ky == 2) out = (uint8_t)((sum + 2) >> 2);
        else out = sat_u8((int)rintf((float)sum * (1.f / (float)(p.kx * p.ky))));
    } else {
        float sum = 0.f;
        bool first = true;
        for (int j = p.yofs[dy]; j < p.yofs[dy + 1]; j++) {
            const float beta = p.ytab[j].alpha;
            const uint8_t *S = Sz + (int64_t)p.ytab[j].si * p.sstep + c;
            float buf = 0.f;
            for (int k = p.xofs[dx]; k < p.xofs[dx + 1]; k++) buf += (float)S[p.xtab[k].si] * p.xtab[k].alpha;
            if (first) {
                sum = beta * buf;
                first = false;
            } else {
                sum += beta * buf;
            }
        }
        out = sat_u8((int)rintf(sum));
    }
    p.dst[(int64_t)blockIdx.z * p.out_stride + (int64_t)dy * p.dstep + dxb] = out;
}

// Bytes [lo, hi) of a source row under the tile of destination pixels [p0, p1)
static void pf_segment(int cn, int kx, const std::vector<AreaTap> *xtab, const std::vector<int32_t> *xofs, int p0, int p1,
                       int *lo, int *hi)
{
    if (kx > 0) {
        *lo = p0 * kx * cn, *hi = p1 * kx * cn;
    } else {
        *lo = (*xtab)[(size_t)(*xofs)[(size_t)p0]].si;
        *hi = (*xtab)[(size_t)(*xofs)[(size_t)p1] - 1].si + cn;
    }
}

PfTiling pf_area_tiling(int cn, int dcols, int kx, const std::vector<AreaTap> *xtab, const std::vector<int32_t> *xofs,
                        const std::vector<AreaTap> *ytab)
{
    PfTiling t;
    if (kx <= 0) {
        // what the tile kernel relies on, by construction of area_tab: every destination index has a tap, a pixel's
        // horizontal taps are consecutive source pixels, and the vertical taps never step back
        for (int dx = 0; dx < dcols; dx++) {
            const int k0 = (*xofs)[(size_t)dx], k1 = (*xofs)[(size_t)dx + 1];
            if (k1 <= k0) return t;
            for (int k = k0 + 1; k < k1; k++)
                if ((*xtab)[(size_t)k].si != (*xtab)[(size_t)k - 1].si + cn) return t;
        }
        if (ytab->empty()) return t;
        for (size_t j = 1; j < ytab->size(); j++)
            if ((*ytab)[j].si < (*ytab)[j - 1].si) return t;
    }
    for (int twp = std::min(PF_THREADS / cn, dcols); twp >= 1; twp = twp > 1 ? (twp + 1) / 2 : 0) {
        int segd = 0;
        for (int p0 = 0; p0 < dcols; p0 += twp) {
            int lo, hi;
            pf_segment(cn, kx, xtab, xofs, p0, std::min(p0 + twp, dcols), &lo, &hi);
            segd = std::max(segd, (hi - (lo & ~3) + 3) >> 2);
        }
        if (segd > PF_LDS_DWORDS) continue;
        t.tiled = true;
        t.twp = twp;
        t.th = PF_TILE_ROWS;
        t.segd = segd;
        t.chunk = std::max(1, std::min(PF_MAX_CHUNK, PF_LDS_DWORDS / segd));
        return t;
    }
    return t;
}

hipError_t launch_pf_area(const PfArea &p, const PfTiling &t, int n, hipStream_t s)
{
    if ((p.cn != 1 && p.cn != 3) || n <= 0 || n > 65535) return hipErrorInvalidValue;
    const bool integer = p.kx > 0;
    if (!t.tiled) {
        const dim3 grid((p.dcols * p.cn + PF_THREADS - 1) / PF_THREADS, p.drows, n);
        if (integer) hipLaunchKernelGGL(pf_area_direct_kernel<true>, grid, dim3(PF_THREADS), 0, s, p);
        else hipLaunchKernelGGL(pf_area_direct_kernel<false>, grid, dim3(PF_THREADS), 0, s, p);
        return hipGetLastError();
    }
    const int aligned = ((((uintptr_t)p.src) | (uintptr_t)p.scan_stride | (uintptr_t)p.sstep) & 3) == 0;
    const dim3 grid((p.dcols + t.twp - 1) / t.twp, (p.drows + t.th - 1) / t.th, n);
    const size_t lds = sizeof(uint32_t) * (size_t)t.chunk * t.segd;
    if (integer)
        hipLaunchKernelGGL(pf_area_tile_kernel<true>, grid, dim3(PF_THREADS), lds, s, p, t.twp, t.th, t.segd, t.chunk, aligned);
    else
        hipLaunchKernelGGL(pf_area_tile_kernel<false>, grid, dim3(PF_THREADS), lds, s, p, t.twp, t.th, t.segd, t.chunk, aligned);
    return hipGetLastError();
}

// resize_linear_kernel (stages.hip) over a batch: the source is the smaller image, so its rows stay in cache and a
// thread per destination byte is the right shape.
__global__ __launch_bounds__(PF_THREADS) void pf_linear_kernel(const uint8_t *__restrict__ src, int64_t scan_stride, int64_t sstep,
                                                               int srows, int scols, int cn, uint8_t *__restrict__ dst,
                                                               int64_t out_stride, int64_t dstep, int drows, int dcols,
                                                               double scale_x, double inv_scale_x, double scale_y,
                                                               double inv_scale_y, int area_mode)
{
    const int dxb = blockIdx.x * PF_THREADS + threadIdx.x, dy = blockIdx.y;
    if (dxb >= dcols * cn) return;
    const int dx = dxb / cn, c = dxb - dx * cn;
    int sx, a0, a1, sy, b0, b1;
    bool edge, unused;
    linear_coef(dx, scale_x, inv_scale_x, scols, area_mode != 0, sx, a0, a1, edge);
    linear_coef(dy, scale_y, inv_scale_y, 0, area_mode != 0, sy, b0, b1, unused);
    const int sy0 = max(0, min(srows - 1, sy)), sy1 = max(0, min(srows - 1, sy + 1));
    const uint8_t *Sz = src + (int64_t)blockIdx.z * scan_stride;
    const uint8_t *S0 = Sz + (int64_t)sy0 * sstep + (int64_t)sx * cn + c;
    const uint8_t *S1 = Sz + (int64_t)sy1 * sstep + (int64_t)sx * cn + c;
    int h0, h1;
    if (!edge) {
        h0 = (int)S0[0] * a0 + (int)S0[cn] * a1;
        h1 = (int)S1[0] * a0 + (int)S1[cn] * a1;
    } else {
        h0 = (int)S0[0] * 2048;
        h1 = (int)S1[0] * 2048;
    }
    dst[(int64_t)blockIdx.z * out_stride + (int64_t)dy * dstep + dxb] =
        (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

hipError_t launch_pf_linear(const uint8_t *d_src, int64_t scan_stride, int64_t sstep, int srows, int scols, int cn, int n,
                            uint8_t *d_dst, int64_t out_stride, int64_t dstep, int drows, int dcols, bool area_mode,
                            hipStream_t s)
{
    if (n <= 0 || n > 65535 || drows > 65535) return hipErrorInvalidValue;
    const double inv_scale_x = (double)dcols / scols, inv_scale_y = (double)drows / srows;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    hipLaunchKernelGGL(pf_linear_kernel, dim3((dcols * cn + PF_THREADS - 1) / PF_THREADS, drows, n), dim3(PF_THREADS), 0, s, d_src,
                       scan_stride, sstep, srows, scols, cn, d_dst, out_stride, dstep, drows, dcols, scale_x, inv_scale_x,
                       scale_y, inv_scale_y, area_mode ? 1 : 0);
    return hipGetLastError();
}

}  // namespace omr
