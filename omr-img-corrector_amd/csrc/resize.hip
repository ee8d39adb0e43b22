// resize.hip -- OpenCV 4.6.0 resize() on the device (transfer.rs:66-91 scale_self, :128-145 resize_self, omr.rs:114-126)
// for n same-shape images of 8-bit interleaved channels, one launch, the image index in blockIdx.z.  The per-call
// entry points (resize_ptr, oics_host.cpp) are a batch of one; the correct_default batch and
// the projection batch (section 4.12) hand in their chunk.  One set of kernels, so the three callers' images are the
// same bytes by construction:
//
//   resize_linear_kernel            INTER_LINEAR and INTER_AREA's bilinear emulation when an axis enlarges (quirk B7)
//   resize_area_direct_kernel<INT>  INTER_AREA, one thread per destination byte straight from memory: resizeAreaFast_
//                                   (integer factors) / resizeArea_<uchar,float> with the tap tables (any other shrink)
//   pf_area_tile_kernel<INT>        the same two through LDS tiles, for images whose gather is the whole cost
//   resize_area_int_colsum_kernel, resize_area_int_c1_kernel
//                                   resizeAreaFast_ for gray images and one factor k on both axes
//
// launch_resize picks by resize()'s dispatch and by what the caller asks for; it tunes nothing by itself.
// The file is built -ffp-contract=off: the coefficient and tap arithmetic rounds like OpenCV's scalar code.
//
// The direct kernels give a thread one destination byte, so neighbouring lanes read the source cn / scale bytes
// apart; on a colour A4 scan that gather is the whole cost.  The tile kernel turns it round: a workgroup owns a tile of
// destination columns, reads the source rows under it as contiguous, aligned dword segments into LDS (a few rows at a
// time), applies the horizontal taps of a source row once per lane from LDS and keeps the vertical accumulation in
// registers, walking down the tile.  Every source byte is read from memory once (a tile's first source row may be shared
// with the tile above).  The order of the float operations per destination byte is the direct kernel's, so the
// images are its images bit for bit.
// When the source pointer, scan_stride or sstep is not a multiple of 4 the segments are staged byte by byte:
// same result, slower.
#include <hip/hip_runtime.h>

#include "resize.hpp"
#include "warp_fixed.hpp"

namespace omr {

#define PF_THREADS 256
#define PF_LDS_DWORDS 4096  // 16 KB of staged source rows per workgroup
#define PF_TILE_ROWS 16     // destination rows per workgroup
#define PF_MAX_CHUNK 16     // source rows staged at once
#define PF_REG_TAPS 8       // horizontal weights a lane keeps in registers (the rest come from the table)

// ------------------------------------------------------------------------------------------
// The coefficient expressions of OpenCV's bilinear resize (resize.cpp, resizeGeneric_ with
// HResizeLinear<uchar,int,short,2048>).  One axis of one destination index d: the first source index s0, the two 11-bit
// taps c0 / c1 (double products, float fractions, saturate_cast<short>(c * 2048) with round-half-even) and, on the
// horizontal axis (ssize > 0), whether the column copies S[s0] * 2048 ("dx >= xmax": sx is monotone in dx, so that is
// just sx + 1 >= ssize).  area_mode: the coefficients INTER_AREA takes when an axis enlarges (quirk B7).
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

// resize(INTER_LINEAR) and INTER_AREA's bilinear emulation when an axis enlarges (OpenCV resizeGeneric_ with
// HResizeLinear<uchar,int,short,2048> / VResizeLinear<uchar,int,short,FixedPtCast<22>>): scale_self with
// scale > 1 (transfer.rs:66-91) and path 2's unclamped scale (omr.rs:60-82,114-126, quirk B7).  Every thread
// rebuilds its two coefficient pairs: 11-bit horizontal taps on the two source rows, then
// (((b0*(h0>>4))>>16) + ((b1*(h1>>4))>>16) + 2) >> 2.  The source is the smaller image, so its rows stay in cache and
// a thread per destination byte is the right shape.
__global__ __launch_bounds__(256) void resize_linear_kernel(ResizeImgs p, double scale_x, double inv_scale_x, double scale_y,
                                                            double inv_scale_y, int area_mode)
{
    const int cn = p.cn;
    const int dxb = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y;
    if (dxb >= p.dcols * cn) return;
    const int dx = dxb / cn, c = dxb - dx * cn;
    int sx, a0, a1, sy, b0, b1;
    bool edge, unused;
    linear_coef(dx, scale_x, inv_scale_x, p.scols, area_mode != 0, sx, a0, a1, edge);
    linear_coef(dy, scale_y, inv_scale_y, 0, area_mode != 0, sy, b0, b1, unused);
    const int sy0 = max(0, min(p.srows - 1, sy)), sy1 = max(0, min(p.srows - 1, sy + 1));
    const uint8_t *Sz = p.src + (int64_t)blockIdx.z * p.scan_stride;
    const uint8_t *S0 = Sz + (int64_t)sy0 * p.sstep + (int64_t)sx * cn + c;
    const uint8_t *S1 = Sz + (int64_t)sy1 * p.sstep + (int64_t)sx * cn + c;
    int h0, h1;
    if (!edge) {
        h0 = (int)S0[0] * a0 + (int)S0[cn] * a1;
        h1 = (int)S1[0] * a0 + (int)S1[cn] * a1;
    } else {
        h0 = (int)S0[0] * 2048;
        h1 = (int)S1[0] * 2048;
    }
    p.dst[(int64_t)blockIdx.z * p.out_stride + (int64_t)dy * p.dstep + dxb] =
        (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

// ------------------------------------------------------------------------------------------
// resize INTER_AREA, one thread per destination byte (dxb runs over dcols * cn).
//   INT   integer factors (OpenCV resizeAreaFast_): the kx x ky block mean.  The factors divide both sizes (launch_resize
//         refuses anything else), so every block is a full one.
//   else  general shrink (OpenCV resizeArea_<uchar,float>): the same float accumulation order as ResizeArea_Invoker:
//         for each source row tap (ascending) the row sum buf = sum_k S*alpha_k (ascending k), then sum (+)= beta*buf.
template <bool INT>
__global__ __launch_bounds__(256) void resize_area_direct_kernel(ResizeImgs p)
{
    const int cn = p.cn;
    const int dxb = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y;
    if (dxb >= p.dcols * cn) return;
    const uint8_t *src = p.src + (int64_t)blockIdx.z * p.scan_stride;
    uint8_t out;
    if (INT) {
        const int kx = p.kx, ky = p.ky;
        const int sy0 = dy * ky;
        const int sx0 = kx * (dxb / cn) * cn + dxb % cn;
        int sum = 0;
        for (int sy = 0; sy < ky; sy++)
            for (int sx = 0; sx < kx; sx++) sum += src[(int64_t)(sy0 + sy) * p.sstep + sx0 + sx * cn];
        if (kx == 2 && ky == 2) out = (uint8_t)((sum + 2) >> 2);
        else out = sat_u8((int)rintf((float)sum * (1.f / (float)(kx * ky))));
    } else {
        const AreaTap *__restrict__ xtab = p.t.xtab, *__restrict__ ytab = p.t.ytab;
        const int32_t *__restrict__ xofs = p.t.xofs, *__restrict__ yofs = p.t.yofs;
        const int dx = dxb / cn, c = dxb % cn;
        float sum = 0.f;
        bool first = true;
        for (int j = yofs[dy]; j < yofs[dy + 1]; j++) {
            const float beta = ytab[j].alpha;
            const uint8_t *S = src + (int64_t)ytab[j].si * p.sstep + c;
            float buf = 0.f;
            for (int k = xofs[dx]; k < xofs[dx + 1]; k++) buf += (float)S[xtab[k].si] * xtab[k].alpha;
            if (first) {
                sum = beta * buf;  // ResizeArea_Invoker assigns on the first tap of a destination row
                first = false;
            } else {
                sum += beta * buf;
            }
        }
        out = sat_u8((int)rintf(sum));
    }
    p.dst[(int64_t)blockIdx.z * p.out_stride + (int64_t)dy * p.dstep + dxb] = out;
}

// ------------------------------------------------------------------------------------------
// floor(i / d) for i * d < 2^32, d >= 2, with m = ceil(2^32 / d)
__device__ __forceinline__ uint32_t pf_div(uint32_t i, uint32_t m) { return __umulhi(i, m); }

template <bool INT>
__global__ __launch_bounds__(PF_THREADS) void pf_area_tile_kernel(ResizeImgs p, int twp, int th, int segd, int chunk, int aligned)
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
        seg_lo = p.t.xtab[p.t.xofs[p0]].si, seg_hi = p.t.xtab[p.t.xofs[p1] - 1].si + cn;
        j = p.t.yofs[dy0], r = p.t.ytab[j].si, r_end = p.t.ytab[p.t.yofs[dy1] - 1].si + 1;
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
            x0 = p.t.xofs[p0 + lp];
            nt = p.t.xofs[p0 + lp + 1] - x0;
            off = p.t.xtab[x0].si + c - base;  // a destination pixel's taps are consecutive source pixels
#pragma unroll
            for (int k = 0; k < PF_REG_TAPS; k++)
                if (k < nt) a[k] = p.t.xtab[x0 + k].alpha;
        }
    }
    int dy = dy0;
    int jend = INT ? (dy0 + 1) * p.ky : p.t.yofs[dy0 + 1];
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
                    if (dy < dy1) jend = INT ? (dy + 1) * p.ky : p.t.yofs[dy + 1];
                    sum = 0.f, isum = 0, first = true;
                    continue;
                }
                const int si = INT ? j : p.t.ytab[j].si;
                if (si >= rlim) break;  // in the next chunk
                const uint8_t *row = (const uint8_t *)(pf_lds + (si - r) * segd) + off;
                if (INT) {
                    for (int k = 0; k < nt; k++) isum += row[k * cn];
                } else {
                    const float beta = p.t.ytab[j].alpha;
                    float buf = 0.f;
#pragma unroll
                    for (int k = 0; k < PF_REG_TAPS; k++)
                        if (k < nt) buf += (float)row[k * cn] * a[k];
                    for (int k = PF_REG_TAPS; k < nt; k++) buf += (float)row[k * cn] * p.t.xtab[x0 + k].alpha;
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

// ------------------------------------------------------------------------------------------
// resize INTER_AREA, integer factor k (OpenCV resizeAreaFast_), 1 channel: coalesced row loads, k*k sum per output
// pixel from LDS.
#define RA_OW 64
#define RA_OH 4
#define RA_MAXK 8

__global__ __launch_bounds__(256) void resize_area_int_c1_kernel(const uint8_t *__restrict__ src, int64_t scan_stride,
                                                                 int64_t sstep, uint8_t *__restrict__ dst, int64_t out_stride,
                                                                 int64_t dstep, int drows, int dcols, int k)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[RA_OH * RA_MAXK][RA_OW * RA_MAXK + 4];
    const int ox0 = blockIdx.x * RA_OW, oy0 = blockIdx.y * RA_OH;
    const int iw = min(RA_OW, dcols - ox0) * k, ih = min(RA_OH, drows - oy0) * k;
    const uint8_t *S = src + (int64_t)blockIdx.z * scan_stride + (int64_t)oy0 * k * sstep + (int64_t)ox0 * k;
    if ((((uintptr_t)S | (uintptr_t)sstep) & 3) == 0) {  // dword loads: a quarter of the load instructions
        const int iw4 = iw >> 2;
        for (int i = threadIdx.x; i < iw4 * ih; i += 256) {
            const int ly = i / iw4, lq = i - ly * iw4;
            *(uint32_t *)&tile[ly][lq * 4] = *(const uint32_t *)(S + (int64_t)ly * sstep + lq * 4);
        }
        for (int i = threadIdx.x; i < (iw & 3) * ih; i += 256) {  // last, partial block of a row
            const int ly = i / (iw & 3), lx = (iw & ~3) + i % (iw & 3);
            tile[ly][lx] = S[(int64_t)ly * sstep + lx];
        }
    } else {
        for (int i = threadIdx.x; i < iw * ih; i += 256) {
            const int ly = i / iw, lx = i - ly * iw;
            tile[ly][lx] = S[(int64_t)ly * sstep + lx];
        }
    }
    __syncthreads();
    const int lx = threadIdx.x & (RA_OW - 1), ly = threadIdx.x / RA_OW;
    const int ox = ox0 + lx, oy = oy0 + ly;
    if (ox < dcols && oy < drows) {
        int sum = 0;
        for (int yy = 0; yy < k; yy++)
            for (int xx = 0; xx < k; xx++) sum += tile[ly * k + yy][lx * k + xx];
        uint8_t out;
        if (k == 2) out = (uint8_t)((sum + 2) >> 2);
        else out = sat_u8((int)rintf((float)sum * (1.f / (float)(k * k))));
        dst[(int64_t)blockIdx.z * out_stride + (int64_t)oy * dstep + ox] = out;
    }
}

// The same reduction with the column sums taken first: a lane adds the k source rows of one dword column
// straight from global memory (k coalesced dword loads in flight, 4 pixels each, byte pairs widened to
// u16 with two masks and added with v_pk_add_u16), parks four u16 column sums in LDS, and after the
// barrier a lane per output pixel adds k neighbouring column sums -- 2k LDS accesses per output pixel
// instead of k*k byte reads, and no staging of the raw tile.
#define RB_OW 64
#define RB_OH 4
#define RB_MAXK 16

__global__ __launch_bounds__(256) void resize_area_int_colsum_kernel(const uint8_t *__restrict__ src, int64_t scan_stride,
                                                                     int64_t sstep, uint8_t *__restrict__ dst,
                                                                     int64_t out_stride, int64_t dstep, int drows, int dcols,
                                                                     int k)
{
    __shared__ uint16_t colsum[RB_OH][RB_OW * RB_MAXK + 8];
    const int ox0 = blockIdx.x * RB_OW, oy0 = blockIdx.y * RB_OH;
    const int ow = min(RB_OW, dcols - ox0), oh = min(RB_OH, drows - oy0);
    const int iw = ow * k, nq = (iw + 3) >> 2;  // source pixels / dword columns of the tile (iw may end inside a dword)
    // 4-byte aligned: ox0 * k is a multiple of 64
    const uint8_t *S = src + (int64_t)blockIdx.z * scan_stride + (int64_t)oy0 * k * sstep + (int64_t)ox0 * k;
    for (int i = threadIdx.x; i < nq * oh; i += 256) {
        const int ly = i / nq, q = i - ly * nq;
        const uint8_t *P = S + (int64_t)ly * k * sstep + q * 4;
        uint32_t e = 0, o = 0;  // (px0, px2) and (px1, px3) as u16 pairs
        for (int yy = 0; yy < k; yy++) {
            const uint32_t v = *(const uint32_t *)(P + (int64_t)yy * sstep);  // may read past iw inside the row pitch: unused
            e += v & 0x00ff00ffu;
            o += (v >> 8) & 0x00ff00ffu;
        }
        uint16_t *C = &colsum[ly][q * 4];
        C[0] = (uint16_t)e;
        C[1] = (uint16_t)o;
        C[2] = (uint16_t)(e >> 16);
        C[3] = (uint16_t)(o >> 16);
    }
    __syncthreads();
    const int lx = threadIdx.x & (RB_OW - 1), ly = threadIdx.x / RB_OW;
    if (lx < ow && ly < oh) {
        int sum = 0;
        for (int xx = 0; xx < k; xx++) sum += colsum[ly][lx * k + xx];
        uint8_t out;
        if (k == 2) out = (uint8_t)((sum + 2) >> 2);
        else out = sat_u8((int)rintf((float)sum * (1.f / (float)(k * k))));
        dst[(int64_t)blockIdx.z * out_stride + (int64_t)(oy0 + ly) * dstep + ox0 + lx] = out;
    }
}

// ------------------------------------------------------------------------------------------
template <bool INT>
static void launch_area(const ResizeImgs &p, int n, hipStream_t s, const PfTiling *tiling)
{
    if (!tiling || !tiling->tiled) {
        hipLaunchKernelGGL(resize_area_direct_kernel<INT>, dim3((p.dcols * p.cn + 255) / 256, p.drows, n), dim3(256), 0, s, p);
        return;
    }
    const PfTiling &t = *tiling;
    const int aligned = ((((uintptr_t)p.src) | (uintptr_t)p.scan_stride | (uintptr_t)p.sstep) & 3) == 0;
    const dim3 grid((p.dcols + t.twp - 1) / t.twp, (p.drows + t.th - 1) / t.th, n);
    const size_t lds = sizeof(uint32_t) * (size_t)t.chunk * t.segd;
    hipLaunchKernelGGL(pf_area_tile_kernel<INT>, grid, dim3(PF_THREADS), lds, s, p, t.twp, t.th, t.segd, t.chunk, aligned);
}

hipError_t launch_resize(const ResizeDispatch &d, const ResizeImgs &im, int n, hipStream_t s, const AreaTaps &taps,
                         const PfTiling *tiling)
{
    if (n <= 0 || n > 65535 || im.drows > 65535 || im.cn < 1) return hipErrorInvalidValue;
    if (tiling && im.cn != 1 && im.cn != 3) return hipErrorInvalidValue;
    ResizeImgs p = im;
    p.kx = p.ky = 0;
    p.t = AreaTaps();
    switch (d.kind) {
    case ResizeDispatch::COPY: return hipErrorInvalidValue;
    case ResizeDispatch::LINEAR: {
        const double inv_scale_x = (double)p.dcols / p.scols, inv_scale_y = (double)p.drows / p.srows;
        const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
        hipLaunchKernelGGL(resize_linear_kernel, dim3((p.dcols * p.cn + 255) / 256, p.drows, n), dim3(256), 0, s, p, scale_x,
                           inv_scale_x, scale_y, inv_scale_y, d.area_mode ? 1 : 0);
        break;
    }
    case ResizeDispatch::AREA_INT: {
        // resize()'s test for integer factors (host_image.hpp) holds only for exact multiples at every size
        // check_image_shape admits, so the kernels carry no partial-block arithmetic
        if (d.kx < 1 || d.ky < 1 || p.dcols * d.kx != p.scols || p.drows * d.ky != p.srows) return hipErrorInvalidValue;
        p.kx = d.kx, p.ky = d.ky;
        const int k = d.kx;
        const bool gray_k = !tiling && p.cn == 1 && d.kx == d.ky && k >= 2;
        // the dword loads of the last column may run up to 3 bytes past the last source pixel of a row: the row pitch
        // must cover them (always true for a pitch that is a multiple of 4)
        if (gray_k && k <= RB_MAXK && ((((uintptr_t)p.src) | (uintptr_t)p.scan_stride | (uintptr_t)p.sstep) & 3) == 0) {
            hipLaunchKernelGGL(resize_area_int_colsum_kernel, dim3((p.dcols + RB_OW - 1) / RB_OW, (p.drows + RB_OH - 1) / RB_OH, n),
                               dim3(256), 0, s, p.src, p.scan_stride, p.sstep, p.dst, p.out_stride, p.dstep, p.drows, p.dcols, k);
        } else if (gray_k && k <= RA_MAXK) {
            hipLaunchKernelGGL(resize_area_int_c1_kernel, dim3((p.dcols + RA_OW - 1) / RA_OW, (p.drows + RA_OH - 1) / RA_OH, n),
                               dim3(256), 0, s, p.src, p.scan_stride, p.sstep, p.dst, p.out_stride, p.dstep, p.drows, p.dcols, k);
        } else {
            launch_area<true>(p, n, s, tiling);
        }
        break;
    }
    case ResizeDispatch::AREA_GENERAL:
        if (!taps.xtab || !taps.xofs || !taps.ytab || !taps.yofs) return hipErrorInvalidValue;
        p.t = taps;
        launch_area<false>(p, n, s, tiling);
        break;
    }
    return hipGetLastError();
}

}  // namespace omr
