// jpeg.hip -- baseline-sequential JPEG encoding of a batch of device-resident images, byte for
// byte what libjpeg writes after jpeg_set_defaults + jpeg_set_quality(q, TRUE); restated stage by stage in
// tests/jpeg_ref.py.
//
//   jpeg_block_kernel    a workgroup per 128 x 64 pixel tile: source rows -> LDS (aligned dword loads, byte-wise for odd
//                        bases and pitches), rgb_ycc_convert + edge replication + h2v2_downsample into component planes
//                        in LDS, then a thread per 8 x 8 block: jfdctint.c in int32, jcdctmgr.c's rounding division,
//                        zig-zag i16 coefficients and the bit length of the block's AC codes
//   jpeg_dc_kernel       a thread per block in scan order: the DC difference (dummy blocks of jccoefct.c resolved to the
//                        real block whose DC they repeat), the block's bit length, a scan inside the 256-block segment
//   jpeg_seg_scan_kernel a wave per image: exclusive scan of its segments' sums (used for bits and for 0xFF counts)
//   jpeg_bits_kernel     a thread per block: its code bits at its offset in the image's cleared bit buffer -- whole
//                        dwords stored, the two boundary dwords through atomicOr
//   jpeg_ff_kernel       a thread per 16 bytes: 0xFF bytes counted (the stream's last byte padded with 1-bits first)
//   jpeg_stream_kernel   the same bytes scattered behind the header with a 0x00 after every 0xFF, then EOI
//   jpeg_header_kernel   the call's header in front of every stream, SOF0's size patched per image
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "jpeg.hpp"

namespace omr {
namespace {

constexpr int TW = JPEG_TILE_W, TH = JPEG_TILE_H;

// jpeg_natural_order: ZZ[k] = natural index of the k-th coefficient in zig-zag order
__device__ constexpr int ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint.c over d[0], d[S], .. d[7 * S]
template <int S, bool FIRST>
__device__ __forceinline__ void fdct_pass(int *d)
{
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * 4;
        d[4 * S] = (t10 - t11) * 4;
    } else {
        d[0] = descale(t10 + t11, 2);
        d[4 * S] = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * S] = descale(z1 + t13 * 6270, N);
    d[6 * S] = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    d[7 * S] = descale(a4 + z1 + z3, N);
    d[5 * S] = descale(a5 + z2 + z4, N);
    d[3 * S] = descale(a6 + z2 + z3, N);
    d[S] = descale(a7 + z1 + z4, N);
}

__device__ __forceinline__ int nbits_of(int v) { return 32 - __clz(v < 0 ? -v : v); }  // v != 0, or 0 for 0

// tables of one launch in LDS
struct LdsTables {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};
__device__ __forceinline__ void load_tables(LdsTables *t, const JpegTables *g)
{
    for (int i = threadIdx.x; i < 24; i += blockDim.x) (&t->dc[0][0])[i] = (&g->dc[0][0])[i];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) (&t->ac[0][0])[i] = (&g->ac[0][0])[i];
}

// exclusive scan of one value per thread over a 256-thread workgroup; *total = the sum.  `sh`: 4 dwords of LDS.
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t *sh, uint32_t *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // sh may still be read from the call before
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < w) base += sh[k];
        tot += sh[k];
    }
    *total = tot;
    return base + inc - v;
}

template <int CN>
__global__ __launch_bounds__(256) void jpeg_block_kernel(JpegPass p)
{
    const JpegImg im = p.imgs[blockIdx.z];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int ext_w = im.mw * (CN == 3 ? 16 : 8), ext_h = im.mh * (CN == 3 ? 16 : 8);
    if (x0 >= ext_w || y0 >= ext_h) return;  // also every tile of a 0 x 0 image
    constexpr int ROWB = TW * CN, ROWDW = ROWB / 4;
    __shared__ uint32_t raw[TH * ROWDW];
    __shared__ uint8_t yp[CN == 3 ? TH * TW : 4];
    __shared__ uint8_t cp[CN == 3 ? 2 * (TH / 2) * (TW / 2) : 4];
    __shared__ uint16_t qdiv[2][64];
    __shared__ uint32_t acl[2][256];
    const int tid = threadIdx.x;
    if (tid < 128) (&qdiv[0][0])[tid] = (&p.tab->div[0][0])[tid];
    for (int i = tid; i < 512; i += 256) (&acl[0][0])[i] = (&p.tab->ac[0][0])[i];

    // ---- the tile's real pixels -> raw, rows ROWB bytes apart
    const int vr = min(TH, im.rows - y0), vb = min(TW, im.cols - x0) * CN, vdw = (vb + 3) >> 2;
    const uint8_t *base = p.src + im.src_off + (int64_t)y0 * p.step + (int64_t)x0 * CN;
    const bool aligned = ((((uintptr_t)(p.src + im.src_off)) | (uintptr_t)p.step) & 3) == 0;  // x0 * CN is a multiple of 4
    for (int it = tid; it < vr * vdw; it += 256) {
        const int r = it / vdw, d = it - r * vdw;
        const uint8_t *q = base + (int64_t)r * p.step + 4 * d;
        uint32_t v;
        if (aligned && 4 * d + 4 <= vb) {
            v = *reinterpret_cast<const uint32_t *>(q);
        } else {
            v = 0;
            for (int k = 0; k < 4 && 4 * d + k < vb; k++) v |= (uint32_t)q[k] << (8 * k);
        }
        raw[r * ROWDW + d] = v;
    }
    __syncthreads();
    const uint8_t *rawb = reinterpret_cast<const uint8_t *>(raw);
    const int lx_max = min(TW, im.cols - x0) - 1, ly_max = vr - 1;  // clamping to these replicates the image's edges

    if (CN == 3) {
        // ---- a thread per 2 x 2 pixels: four Y samples, one Cb and one Cr
        const int crows = (im.rows + 1) >> 1;
        for (int qd = tid; qd < (TW / 2) * (TH / 2); qd += 256) {
            const int qx = qd & (TW / 2 - 1), qy = qd / (TW / 2);
            const int lx0 = min(2 * qx, lx_max), lx1 = min(2 * qx + 1, lx_max);
            const int ly0 = min(2 * qy, ly_max), ly1 = min(2 * qy + 1, ly_max);
            // chroma: below the image the last *down-sampled* row repeats (expand_bottom_edge runs behind the down-sampler)
            const int cy = min(y0 / 2 + qy, crows - 1);
            const int cl0 = min(2 * cy, im.rows - 1) - y0, cl1 = min(2 * cy + 1, im.rows - 1) - y0;
            int scb = 0, scr = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int lx = (k & 1) ? lx1 : lx0;
                {
                    const uint8_t *px = rawb + ((k & 2) ? ly1 : ly0) * ROWB + lx * 3;
                    const int b = px[0], g = px[1], r = px[2];
                    yp[(2 * qy + (k >> 1)) * TW + 2 * qx + (k & 1)] = (uint8_t)((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
                }
                const uint8_t *px = rawb + ((k & 2) ? cl1 : cl0) * ROWB + lx * 3;
                const int b = px[0], g = px[1], r = px[2];
                scb += (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
                scr += (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
            }
            const int bias = 1 + (qx & 1);  // 1, 2, 1, 2, .. along a row; x0 / 2 is even
            cp[qy * (TW / 2) + qx] = (uint8_t)((scb + bias) >> 2);
            cp[(TH / 2) * (TW / 2) + qy * (TW / 2) + qx] = (uint8_t)((scr + bias) >> 2);
        }
    }
    __syncthreads();

    // ---- a thread per 8 x 8 block
    int comp, lbx, lby;       // component 0..2, block position inside the tile (in that component's blocks)
    uint32_t blk;             // its index in scan order
    bool real = true;
    if (CN == 3) {
        if (tid >= 192) return;
        if (tid < 128) {
            comp = 0, lbx = tid & 15, lby = tid >> 4;
            const int bx = x0 / 8 + lbx, by = y0 / 8 + lby, mx = bx >> 1, my = by >> 1;
            if (mx >= im.mw || my >= im.mh) return;
            real = bx < im.bw && by < im.bh;
            blk = (uint32_t)(my * im.mw + mx) * 6 + (uint32_t)((by & 1) * 2 + (bx & 1));
        } else {
            comp = 1 + ((tid - 128) >> 5);
            lbx = (tid - 128) & 7, lby = ((tid - 128) >> 3) & 3;
            const int mx = x0 / 16 + lbx, my = y0 / 16 + lby;
            if (mx >= im.mw || my >= im.mh) return;
            blk = (uint32_t)(my * im.mw + mx) * 6 + 3 + (uint32_t)comp;
        }
    } else {
        if (tid >= 128) return;
        comp = 0, lbx = tid & 15, lby = tid >> 4;
        const int bx = x0 / 8 + lbx, by = y0 / 8 + lby;
        if (bx >= im.bw || by >= im.bh) return;
        blk = (uint32_t)(by * im.bw + bx);
    }
    blk += im.blk0;
    const int tq = comp ? 1 : 0;
    uint4 *dst = reinterpret_cast<uint4 *>(p.coef + (size_t)blk * 64);
    const uint32_t eob = acl[tq][0] & 255;
    if (!real) {  // a dummy block: no AC; its DC is looked up by the DC pass
#pragma unroll
        for (int k = 0; k < 8; k++) dst[k] = make_uint4(0, 0, 0, 0);
        p.aclen[blk] = (uint16_t)eob;
        return;
    }
    int d[64];
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            int v;
            if (CN == 3) {
                v = comp == 0 ? yp[(lby * 8 + i) * TW + lbx * 8 + j]
                              : cp[(comp - 1) * (TH / 2) * (TW / 2) + (lby * 8 + i) * (TW / 2) + lbx * 8 + j];
            } else {
                v = rawb[min(lby * 8 + i, ly_max) * ROWB + min(lbx * 8 + j, lx_max)];
            }
            d[i * 8 + j] = v - 128;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) fdct_pass<1, true>(d + 8 * i);
#pragma unroll
    for (int j = 0; j < 8; j++) fdct_pass<8, false>(d + j);
    // jcdctmgr.c: divisor = 8 x table entry, half of it added to the magnitude, truncating division
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int dv = qdiv[tq][k], v = d[k], a = v < 0 ? -v : v;
        const int q = (a + (dv >> 1)) / dv;
        d[k] = v < 0 ? -q : q;
    }
    uint32_t bits = 0;
    int run = 0;
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int v = d[ZZ[k]];
        if (k & 1)
            w[k >> 1] |= (uint32_t)(v & 0xffff) << 16;
        else
            w[k >> 1] = (uint32_t)(v & 0xffff);
        if (k == 0) continue;
        if (v == 0) {
            run++;
        } else {
            const int nb = nbits_of(v);
            bits += (uint32_t)(run >> 4) * (acl[tq][0xF0] & 255) + (acl[tq][((run & 15) << 4) | nb] & 255) + (uint32_t)nb;
            run = 0;
        }
    }
    if (run) bits += eob;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    p.aclen[blk] = (uint16_t)bits;
}

// DC of Y block k of MCU (mx, my), dummy blocks resolved (jccoefct.c: a dummy right of the image repeats the block before
// it in its row of the MCU; both blocks of a dummy row below the image repeat the last block of the row above)
__device__ __forceinline__ int y_dc(const JpegImg &im, const int16_t *coef, int m, int k)
{
    const int my = m / im.mw, mx = m - my * im.mw;
    const bool right = 2 * mx + 1 < im.bw, low = 2 * my + 1 < im.bh;
    if (k >= 2 && !low) k = 1;
    if ((k & 1) && !right) k -= 1;
    return coef[((size_t)im.blk0 + (size_t)m * 6 + k) * 64];
}

template <int CN>
__global__ __launch_bounds__(256) void jpeg_dc_kernel(JpegPass p)
{
    const JpegImg im = p.imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    __shared__ uint32_t sh[4];
    __shared__ uint32_t dcl[2][12];
    if (threadIdx.x < 24) (&dcl[0][0])[threadIdx.x] = (&p.tab->dc[0][0])[threadIdx.x];
    __syncthreads();
    const uint32_t b = blockIdx.x * JPEG_CHUNK + threadIdx.x;
    uint32_t len = 0;
    if (b < im.nblk) {
        int cur, pred;
        int tq = 0;
        if (CN == 3) {
            const int m = (int)(b / 6), k = (int)(b - (uint32_t)m * 6);
            if (k < 4) {
                cur = y_dc(im, p.coef, m, k);
                pred = k > 0 ? y_dc(im, p.coef, m, k - 1) : (m > 0 ? y_dc(im, p.coef, m - 1, 3) : 0);
            } else {
                tq = 1;
                cur = p.coef[((size_t)im.blk0 + b) * 64];
                pred = m > 0 ? p.coef[((size_t)im.blk0 + b - 6) * 64] : 0;
            }
        } else {
            cur = p.coef[((size_t)im.blk0 + b) * 64];
            pred = b > 0 ? p.coef[((size_t)im.blk0 + b - 1) * 64] : 0;
        }
        const int diff = cur - pred, nb = diff ? nbits_of(diff) : 0;
        p.dcdiff[im.blk0 + b] = (int16_t)diff;
        len = (dcl[tq][nb] & 255) + (uint32_t)nb + p.aclen[im.blk0 + b];
    }
    uint32_t total;
    const uint32_t ex = block_scan_256(len, sh, &total);
    if (b < im.nblk) p.local[im.blk0 + b] = ex;
    if (threadIdx.x == 0) p.chunk_sum[im.chunk0 + blockIdx.x] = total;
}

// a wave per image: exclusive scan of sums[first .. first + count) into offs, the total into totals[image]
__global__ __launch_bounds__(64) void jpeg_seg_scan_kernel(const JpegImg *imgs, int bytes_stage, const uint32_t *sums, uint32_t *offs,
                                                          uint32_t *totals)
{
    const JpegImg im = imgs[blockIdx.x];
    const uint32_t first = bytes_stage ? im.bchunk0 : im.chunk0, count = bytes_stage ? im.nbchunk : im.nchunk;
    const int lane = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < count; c0 += 64) {
        const uint32_t c = c0 + lane, v = c < count ? sums[first + c] : 0;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (c < count) offs[first + c] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) totals[blockIdx.x] = carry;
}

// the code bits of one block into the image's bit buffer: bit 31 of a dword is the earliest
struct BitWriter {
    uint32_t *w;
    uint64_t acc;
    int n;
    bool first;
    __device__ __forceinline__ void put(uint32_t code, int len)
    {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            const uint32_t word = (uint32_t)(acc >> n);
            acc &= (1ull << n) - 1;
            if (first)
                atomicOr(w, word);  // shared with the blocks before
            else
                *w = word;          // all 32 bits are this block's
            first = false;
            w++;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (n > 0) atomicOr(w, (uint32_t)(acc << (32 - n)));  // shared with the blocks behind
    }
};

__global__ __launch_bounds__(256) void jpeg_bits_kernel(JpegPass p)
{
    const JpegImg im = p.imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    __shared__ LdsTables t;
    load_tables(&t, p.tab);
    __syncthreads();
    const uint32_t b = blockIdx.x * JPEG_CHUNK + threadIdx.x;
    if (b >= im.nblk) return;
    const uint32_t blk = im.blk0 + b;
    int tq = 0;
    if (p.cn == 3) tq = (b % 6) >= 4;
    const uint32_t off = p.chunk_off[im.chunk0 + blockIdx.x] + p.local[blk];
    BitWriter bw{p.bitbuf + im.bit_word + (off >> 5), 0, (int)(off & 31), true};
    const int diff = p.dcdiff[blk];
    {
        const int nb = diff ? nbits_of(diff) : 0;
        const uint32_t e = t.dc[tq][nb];
        bw.put(e >> 8, (int)(e & 255));
        if (nb) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
    }
    const uint4 *src = reinterpret_cast<const uint4 *>(p.coef + (size_t)blk * 64);
    int run = 0;
    for (int q = 0; q < 8; q++) {
        const uint4 v4 = src[q];
        const uint32_t ws[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (q == 0 && j == 0) continue;
            const int v = (int)(int16_t)(ws[j >> 1] >> ((j & 1) * 16));
            if (v == 0) {
                run++;
                continue;
            }
            while (run > 15) {
                const uint32_t z = t.ac[tq][0xF0];
                bw.put(z >> 8, (int)(z & 255));
                run -= 16;
            }
            const int nb = nbits_of(v);
            const uint32_t e = t.ac[tq][(run << 4) | nb];
            // code and value bits together: at most 16 + 10 bits
            bw.put(((e >> 8) << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1)), (int)(e & 255) + nb);
            run = 0;
        }
    }
    if (run) {
        const uint32_t e = t.ac[tq][0];
        bw.put(e >> 8, (int)(e & 255));
    }
    bw.flush();
}

// dword `w` of an image's bit buffer as the stream holds it: the last byte padded with 1-bits (jchuff.c flush_bits)
__device__ __forceinline__ uint32_t stream_word(const JpegImg &im, const uint32_t *buf, uint32_t w)
{
    uint32_t v = buf[w];
    const uint32_t last = (im.nbytes - 1) >> 2;
    if (w == last && (im.bits & 7)) {
        const uint32_t p0 = im.bits - 32 * w, p1 = 8 * im.nbytes - 32 * w;  // bit positions, 0 = the dword's top bit; p0 < p1 <= 32
        const uint32_t hi = 0xffffffffu >> p0, lo = p1 == 32 ? 0u : (0xffffffffu >> p1);
        v |= hi & ~lo;
    }
    return v;
}

// 0xFF bytes among bytes [16 t, 16 t + 16) of the image's stream (t = the thread's position in the image)
__device__ __forceinline__ uint32_t count_ff(const JpegImg &im, const uint32_t *buf, uint32_t t)
{
    uint32_t c = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t w = 4 * t + k;
        if (4 * w >= im.nbytes) break;
        const uint32_t v = stream_word(im, buf, w);
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * w + j < im.nbytes && ((v >> (24 - 8 * j)) & 255) == 255) c++;
    }
    return c;
}

__global__ __launch_bounds__(256) void jpeg_ff_kernel(JpegPass p)
{
    const JpegImg im = p.imgs[blockIdx.y];
    if (blockIdx.x >= im.nbchunk) return;
    __shared__ uint32_t sh[4];
    const uint32_t c = count_ff(im, p.bitbuf + im.bit_word, blockIdx.x * 256 + threadIdx.x);
    uint32_t total;
    (void)block_scan_256(c, sh, &total);
    if (threadIdx.x == 0) p.ff_sum[im.bchunk0 + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_stream_kernel(JpegPass p)
{
    const JpegImg im = p.imgs[blockIdx.y];
    if (blockIdx.x >= im.nbchunk) return;
    __shared__ uint32_t sh[4];
    const uint32_t *buf = p.bitbuf + im.bit_word;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    uint32_t total;
    const uint32_t ex = block_scan_256(count_ff(im, buf, t), sh, &total);
    uint8_t *dst = p.out + im.out_off + p.header_len + 16 * (size_t)t + p.ff_off[im.bchunk0 + blockIdx.x] + ex;
    for (int k = 0; k < 4; k++) {
        const uint32_t w = 4 * t + k;
        if (4 * w >= im.nbytes) break;
        const uint32_t v = stream_word(im, buf, w);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (4 * w + j >= im.nbytes) break;
            const uint8_t byte = (uint8_t)(v >> (24 - 8 * j));
            *dst++ = byte;
            if (byte == 255) *dst++ = 0;
            if (4 * w + j == im.nbytes - 1) dst[0] = 0xFF, dst[1] = 0xD9;  // EOI
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_header_kernel(JpegPass p)
{
    const JpegImg im = p.imgs[blockIdx.x];
    if (im.nblk == 0) return;
    uint8_t *dst = p.out + im.out_off;
    for (int i = threadIdx.x; i < p.header_len; i += 256) {
        uint8_t v = p.header[i];
        const int k = i - p.sof_off;  // rows, cols: 16 bits each, big-endian
        if (k == 0) v = (uint8_t)(im.rows >> 8);
        if (k == 1) v = (uint8_t)im.rows;
        if (k == 2) v = (uint8_t)(im.cols >> 8);
        if (k == 3) v = (uint8_t)im.cols;
        dst[i] = v;
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

}  // namespace

int jpeg_launch_blocks(const JpegPass &p, int max_tiles_x, int max_tiles_y, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles_x, (unsigned)max_tiles_y, (unsigned)p.n);
    if (p.cn == 3)
        jpeg_block_kernel<3><<<grid, 256, 0, s>>>(p);
    else
        jpeg_block_kernel<1><<<grid, 256, 0, s>>>(p);
    return launched("jpeg_block_kernel");
}

int jpeg_launch_lengths(const JpegPass &p, int max_chunks, hipStream_t s)
{
    const dim3 grid((unsigned)max_chunks, (unsigned)p.n);
    if (p.cn == 3)
        jpeg_dc_kernel<3><<<grid, 256, 0, s>>>(p);
    else
        jpeg_dc_kernel<1><<<grid, 256, 0, s>>>(p);
    if (int rc = launched("jpeg_dc_kernel")) return rc;
    jpeg_seg_scan_kernel<<<(unsigned)p.n, 64, 0, s>>>(p.imgs, 0, p.chunk_sum, p.chunk_off, p.img_bits);
    return launched("jpeg_seg_scan_kernel");
}

int jpeg_launch_bits(const JpegPass &p, int max_chunks, int max_bchunks, hipStream_t s)
{
    jpeg_bits_kernel<<<dim3((unsigned)max_chunks, (unsigned)p.n), 256, 0, s>>>(p);
    if (int rc = launched("jpeg_bits_kernel")) return rc;
    jpeg_ff_kernel<<<dim3((unsigned)max_bchunks, (unsigned)p.n), 256, 0, s>>>(p);
    if (int rc = launched("jpeg_ff_kernel")) return rc;
    jpeg_seg_scan_kernel<<<(unsigned)p.n, 64, 0, s>>>(p.imgs, 1, p.ff_sum, p.ff_off, p.img_ff);
    return launched("jpeg_seg_scan_kernel");
}

int jpeg_launch_streams(const JpegPass &p, int max_bchunks, hipStream_t s)
{
    jpeg_header_kernel<<<(unsigned)p.n, 256, 0, s>>>(p);
    if (int rc = launched("jpeg_header_kernel")) return rc;
    jpeg_stream_kernel<<<dim3((unsigned)max_bchunks, (unsigned)p.n), 256, 0, s>>>(p);
    return launched("jpeg_stream_kernel");
}

}  // namespace omr
