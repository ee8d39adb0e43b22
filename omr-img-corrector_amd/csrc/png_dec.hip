// png_dec.hip -- PNG decoding on the device: what imread returns, byte for byte.  The stages:
//
//   inflate    pdec_inflate_kernel   RFC 1950 / 1951, one wave per image, in phases: all lanes refill an input window in
//                                    LDS; the wave decodes a batch of symbols into LDS records (a wave-uniform dependent
//                                    chain, tables in LDS); all lanes write the records' literals and carry out their copies
//   Adler-32   pdec_adler_kernel     the two sums per 64 KB of inflated bytes; pdec_verdict_kernel compares with the trailer
//   samples    pdec_unfilter_kernel  the five filters as a skewed sweep (lane k walks row r0 + k one filter unit behind
//                                    lane k - 1; the row above arrives by a shuffle) and imread's conversion into the slot
//
// No wave waits for another one: a workgroup is one wave, and its barriers stand in wave-uniform control flow.
// Where the bounds sit.  The inflate kernel reads its input only through the window, whose words past the image's input are
// zero, and gives up once the bits consumed pass the input's; it records a literal or a match only when the bytes produced
// plus its length stay within raw_len and a match's distance within the bytes produced, so the copy phase indexes
// [0, raw_len) alone.  Every loop ends with the input's bits, the records of a batch or the length of a copy.  The Adler and
// unfilter kernels index by the header's geometry alone; a palette index is compared with PLTE's length before the look-up.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "png_adler.hpp"
#include "png_dec.hpp"

namespace omr {
namespace {

constexpr int kFast = 10;  // bits of the first-level table
constexpr int kHeaderWords = 160;  // a dynamic block's header: 17 + 19 x 3 + 316 x 14 bits at most

struct Huff {
    uint16_t look[1 << kFast];  // the next kFast bits -> length << 9 | symbol; 0: a longer code, or none
    uint16_t sorted[320];       // symbols in canonical order
    uint16_t first[16];         // [len] the first code of that length
    uint16_t count[16];
    uint16_t off[16];           // [len] index into sorted of that length's first code
};

struct Bits {
    uint64_t bb;
    int bc;
    uint32_t wp;  // the next word of the window
};

__device__ const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ inline void refill(Bits &b, const uint32_t *win)
{
    if (b.bc <= 32) {
        b.bb |= (uint64_t)win[min(b.wp, (uint32_t)PDEC_WIN_WORDS - 1)] << b.bc;
        b.wp++, b.bc += 32;
    }
}

__device__ inline uint32_t take(Bits &b, const uint32_t *win, int n)  // n <= 16
{
    refill(b, win);
    const uint32_t v = (uint32_t)b.bb & ((1u << n) - 1);
    b.bb >>= n, b.bc -= n;
    return v;
}

// the next symbol, -1 for bits that are no code of the set
__device__ inline int decode(Bits &b, const uint32_t *win, const Huff &h)
{
    refill(b, win);
    const uint32_t e = h.look[(uint32_t)b.bb & ((1u << kFast) - 1)];
    int len = (int)(e >> 9);
    if (len) {
        b.bb >>= len, b.bc -= len;
        return (int)(e & 511);
    }
    const uint32_t rev = __brev((uint32_t)b.bb) >> 17;  // the next 15 bits, first bit on top
    for (len = kFast + 1; len <= 15; len++) {
        const int d = (int)(rev >> (15 - len)) - (int)h.first[len];
        if (d >= 0 && d < (int)h.count[len]) {
            const int sym = h.sorted[h.off[len] + d];
            b.bb >>= len, b.bc -= len;
            return sym;
        }
    }
    return -1;
}

// The tables of the n code lengths at lens, by zlib's rules (inftrees.c): no over-subscribed set; an incomplete one only
// where its longest code is 1 bit and the set is not the code-length alphabet's; a set without any code decodes nothing.
// Called by the whole wave in uniform control flow.  Returns false for a refused set.
__device__ bool build(Huff &h, const uint8_t *lens, int n, bool codes, uint32_t *verdict)
{
    const int lane = threadIdx.x;
    __syncthreads();
    if (lane >= 1 && lane <= 15) {
        int c = 0;
        for (int s = 0; s < n; s++) c += lens[s] == lane;
        h.count[lane] = (uint16_t)c;
    }
    for (int i = lane; i < (1 << kFast); i += 64) h.look[i] = 0;
    __syncthreads();
    if (lane == 0) {
        int left = 1, code = 0, k = 0, longest = 0;
        bool ok = true;
        for (int len = 1; len <= 15; len++) {
            const int c = h.count[len];
            left = left * 2 - c;
            if (left < 0) ok = false, left = 0;
            code <<= 1;
            h.first[len] = (uint16_t)code, h.off[len] = (uint16_t)k;
            code += c, k += c;
            if (c) longest = len;
        }
        if (left > 0 && longest != 0 && (codes || longest != 1)) ok = false;
        *verdict = ok;
    }
    __syncthreads();
    const bool ok = *verdict != 0;
    if (ok && lane >= 1 && lane <= 15) {
        int c = 0;
        const int first = h.first[lane], off = h.off[lane];
        for (int s = 0; s < n; s++) {
            if (lens[s] != lane) continue;
            h.sorted[off + c] = (uint16_t)s;
            if (lane <= kFast) {
                const uint32_t r = __brev((uint32_t)(first + c)) >> (32 - lane);
                for (uint32_t f = 0; f < (1u << (kFast - lane)); f++) h.look[r | f << lane] = (uint16_t)(lane << 9 | s);
            }
            c++;
        }
    }
    __syncthreads();
    return ok;
}

__global__ __launch_bounds__(64) void pdec_inflate_kernel(PdecPass p)
{
    const PdecImg *im = p.imgs + blockIdx.x;
    if (im->skip) return;
    __shared__ uint32_t win[PDEC_WIN_WORDS];
    __shared__ Huff hl, hd;
    __shared__ uint8_t lens[320];
    __shared__ uint32_t lpos[PDEC_RECORDS], mpos[PDEC_RECORDS], mld[PDEC_RECORDS];
    __shared__ uint8_t lbyte[PDEC_RECORDS];
    __shared__ uint32_t verdict;
    const int lane = threadIdx.x;
    const uint8_t *src = p.src + im->src_off;
    uint8_t *raw = p.raw + im->raw_off;
    const uint32_t src_len = im->src_len, raw_len = im->raw_len;
    PdecDyn *dyn = p.dyn + blockIdx.x;
    if (src_len < 6) {  // the zlib header and the trailer alone
        if (lane == 0) dyn->err = PDEC_ERR_INPUT;
        return;
    }
    const uint32_t limit = (src_len - 4) * 8;  // the deflate data ends before the trailer
    uint32_t bp = 16, out = 0, err = 0;
    bool in_block = false, last = false, done = false;
    bool fixed_tables = false;  // hl / hd hold the fixed code: a further fixed block builds nothing
    bool reload = true;         // the window is loaded again once half of it is used, and behind a stored block
    uint32_t wbase = 0;
    Bits b{0, 0, 0};
    while (!done && !err) {
        // ---- the window: words from the one that holds bit bp on; zero past the input
        if (reload) wbase = bp >> 5;
        __syncthreads();
        for (int i = lane; reload && i < PDEC_WIN_WORDS; i += 64) {
            const uint64_t at = ((uint64_t)wbase + (uint32_t)i) * 4;
            uint32_t w = 0;
            if (at + 4 <= src_len) {
                w = *reinterpret_cast<const uint32_t *>(src + at);
            } else {
                for (int k = 0; k < 4; k++)
                    if (at + k < src_len) w |= (uint32_t)src[at + k] << (8 * k);
            }
            win[i] = w;
        }
        __syncthreads();
        if (reload) {
            b = Bits{0, 0, 0};
            (void)take(b, win, (int)(bp & 15));
            if (bp & 16) (void)take(b, win, 16);
        }
        // ---- a batch of symbols -> records
        int nl = 0, nm = 0;
        bool stored = false;
        uint32_t stored_len = 0;
        while (!err) {
            if (!in_block) {
                if (last) {
                    done = true;
                    break;
                }
                if (b.wp > (uint32_t)(PDEC_WIN_WORDS - kHeaderWords)) break;
                last = take(b, win, 1) != 0;
                const uint32_t type = take(b, win, 2);
                if (type == 0) {
                    (void)take(b, win, b.bc & 7);  // to the byte
                    stored_len = take(b, win, 16);
                    const uint32_t nlen = take(b, win, 16);
                    if (stored_len != (~nlen & 0xffffu)) err = PDEC_ERR_CODE;
                    stored = true;
                    break;
                } else if (type == 1) {
                    if (!fixed_tables) {
                        __syncthreads();
                        for (int s = lane; s < 320; s += 64) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
                        if (!build(hl, lens, 288, false, &verdict) || !build(hd, lens + 288, 32, false, &verdict)) err = PDEC_ERR_CODE;
                        fixed_tables = true;
                    }
                } else if (type == 2) {
                    fixed_tables = false;
                    const int nlen = (int)take(b, win, 5) + 257, ndist = (int)take(b, win, 5) + 1, ncode = (int)take(b, win, 4) + 4;
                    if (nlen > 286 || ndist > 30) err = PDEC_ERR_CODE;
                    __syncthreads();
                    for (int s = lane; s < 320; s += 64) lens[s] = 0;
                    __syncthreads();
                    for (int i = 0; i < ncode; i++) {
                        const uint32_t v = take(b, win, 3);
                        if (lane == 0) lens[kClOrder[i]] = (uint8_t)v;
                    }
                    if (!err && !build(hd, lens, 19, true, &verdict)) err = PDEC_ERR_CODE;
                    __syncthreads();
                    for (int s = lane; s < 320; s += 64) lens[s] = 0;
                    __syncthreads();
                    // the lengths of both sets in one run: a repeat may cross from the first into the second
                    const int total = nlen + ndist;
                    int prev = 0;
                    for (int i = 0; i < total && !err;) {
                        const int sym = decode(b, win, hd);
                        int rep = 1, val = sym;
                        if (sym < 0) {
                            err = PDEC_ERR_CODE;
                        } else if (sym == 16) {
                            if (i == 0) err = PDEC_ERR_CODE;
                            rep = 3 + (int)take(b, win, 2), val = prev;
                        } else if (sym == 17) {
                            rep = 3 + (int)take(b, win, 3), val = 0;
                        } else if (sym == 18) {
                            rep = 11 + (int)take(b, win, 7), val = 0;
                        }
                        if (i + rep > total) err = PDEC_ERR_CODE;
                        if (err) break;
                        if (lane == 0)
                            for (int k = 0; k < rep; k++) lens[i + k] = (uint8_t)val;
                        i += rep, prev = val;
                    }
                    __syncthreads();
                    if (!err && lens[256] == 0) err = PDEC_ERR_CODE;  // no end-of-block code
                    if (!err && (!build(hl, lens, nlen, false, &verdict) || !build(hd, lens + nlen, ndist, false, &verdict)))
                        err = PDEC_ERR_CODE;
                } else {
                    err = PDEC_ERR_CODE;
                }
                if (!err && (wbase + b.wp) * 32 - (uint32_t)b.bc > limit) err = PDEC_ERR_INPUT;
                in_block = true;
                continue;
            }
            if (nl >= PDEC_RECORDS || nm >= PDEC_RECORDS || b.wp >= (uint32_t)(PDEC_WIN_WORDS - 4)) break;
            const int sym = decode(b, win, hl);
            if (sym < 0 || sym > 285) {
                err = PDEC_ERR_CODE;
            } else if (sym < 256) {
                if (out >= raw_len) {
                    err = PDEC_ERR_SIZE;
                } else {
                    if (lane == 0) lpos[nl] = out, lbyte[nl] = (uint8_t)sym;
                    nl++, out++;
                }
            } else if (sym == 256) {
                in_block = false;
            } else {
                const uint32_t len = kLenBase[sym - 257] + take(b, win, kLenExtra[sym - 257]);
                const int ds = decode(b, win, hd);
                if (ds < 0 || ds > 29) {
                    err = PDEC_ERR_CODE;
                } else {
                    const uint32_t dist = kDistBase[ds] + take(b, win, kDistExtra[ds]);
                    if (dist > out) {
                        err = PDEC_ERR_DISTANCE;
                    } else if (len > raw_len - out) {
                        err = PDEC_ERR_SIZE;
                    } else {
                        if (lane == 0) mpos[nm] = out, mld[nm] = len | dist << 16;
                        nm++, out += len;
                    }
                }
            }
            if (!err && (wbase + b.wp) * 32 - (uint32_t)b.bc > limit) err = PDEC_ERR_INPUT;
        }
        bp = (wbase + b.wp) * 32 - (uint32_t)b.bc;
        reload = stored || b.wp >= (uint32_t)PDEC_WIN_WORDS / 2;
        // ---- the records: literals first (nothing depends on their order), then the copies in stream order; a barrier
        // stands before a copy whose source reaches into a copy made since the last one
        __syncthreads();
        for (int i = lane; i < nl; i += 64) raw[lpos[i]] = lbyte[i];
        __syncthreads();
        uint32_t open = 0xffffffffu;  // where the first copy since the last barrier begins
        for (int j = 0; j < nm; j++) {
            const uint32_t pos = mpos[j], len = mld[j] & 0xffffu, dist = mld[j] >> 16;
            const uint32_t from = pos - dist;
            if (from + min(len, dist) > open) {
                __syncthreads();
                open = 0xffffffffu;
            }
            for (uint32_t k = lane; k < len; k += 64) raw[pos + k] = raw[from + (dist >= len ? k : k % dist)];
            open = min(open, pos);
        }
        __syncthreads();
        if (stored && !err) {
            const uint32_t at = bp >> 3;  // a whole byte: the block's header ended on one
            if (at + stored_len > src_len - 4) {
                err = PDEC_ERR_INPUT;
            } else if (stored_len > raw_len - out) {
                err = PDEC_ERR_SIZE;
            } else {
                for (uint32_t k = lane; k < stored_len; k += 64) raw[out + k] = src[at + k];
                out += stored_len, bp += stored_len * 8;
            }
        }
    }
    if (!err && out != raw_len) err = PDEC_ERR_SIZE;
    if (lane == 0) {
        uint32_t want = 0;
        if (!err) {
            const uint32_t at = (bp + 7) >> 3;
            if (at + 4 > src_len) err = PDEC_ERR_INPUT;
            else want = (uint32_t)src[at] << 24 | (uint32_t)src[at + 1] << 16 | (uint32_t)src[at + 2] << 8 | src[at + 3];
        }
        dyn->err = err, dyn->out_len = out, dyn->adler_want = want;
    }
}

// Adler-32: the sums per PDEC_ADLER_CHUNK bytes are png_adler.hpp's, shared with the encoder
static_assert(PDEC_ADLER_CHUNK == PNG_ADLER_CHUNK, "the host sizes the grid by PDEC_ADLER_CHUNK");
__global__ __launch_bounds__(256) void pdec_adler_kernel(PdecPass p)
{
    const PdecImg *im = p.imgs + blockIdx.y;
    PdecDyn *dyn = p.dyn + blockIdx.y;
    if (im->skip || dyn->err) return;
    adler_chunk_sums(p.raw + im->raw_off, im->raw_len, blockIdx.x, &dyn->a_sum, &dyn->b_sum);
}

__global__ void pdec_verdict_kernel(PdecPass p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n || p.imgs[i].skip || p.dyn[i].err) return;
    if (adler_finish(p.imgs[i].raw_len, p.dyn[i].a_sum, p.dyn[i].b_sum) != p.dyn[i].adler_want) p.dyn[i].err = PDEC_ERR_ADLER;
}

__device__ inline int paeth(int a, int b, int c)
{
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// One filter unit's pixels into the slot: imread's conversion (grfmt_png.cpp's libpng transforms)
template <int BPP>
__device__ inline void emit(const PdecImg *im, const uint8_t (&v)[BPP], int x, uint8_t *row, int cn, const uint8_t *pal, uint32_t *bad)
{
    const int ct = im->color_type, depth = im->depth;
    if (BPP == 1) {
        const int per = 8 / depth, mask = (1 << depth) - 1;
        const int scale = depth == 1 ? 255 : depth == 2 ? 85 : depth == 4 ? 17 : 1;
        for (int j = 0; j < per; j++) {
            const size_t px = (size_t)x * per + j;
            if (px >= (size_t)im->cols) break;
            const int s = (v[0] >> (8 - depth * (j + 1))) & mask;
            if (ct == 3) {
                if (s >= im->npal) {
                    *bad = 1;
                    continue;
                }
                row[3 * px] = pal[3 * s + 2], row[3 * px + 1] = pal[3 * s + 1], row[3 * px + 2] = pal[3 * s];
            } else {
                for (int k = 0; k < cn; k++) row[cn * px + k] = (uint8_t)(s * scale);
            }
        }
    } else if (BPP == 2) {  // gray + alpha
        for (int k = 0; k < cn; k++) row[(size_t)cn * x + k] = v[0];
    } else {  // RGB, RGBA
        row[(size_t)3 * x] = v[2], row[(size_t)3 * x + 1] = v[1], row[(size_t)3 * x + 2] = v[0];
    }
}

// A band of 64 rows per pass: lane k walks row r0 + k, at step t the unit t - k.  The unit above is what lane k - 1 made one
// step earlier, the one above left what it made two steps earlier; lane 0 reads them from the band before, whose last row
// went back into the raw bytes unfiltered.  U steps share one set of loads.
template <int BPP>
__device__ void unfilter_image(const PdecPass &p, const PdecImg *im, PdecDyn *dyn, const uint8_t *pal)
{
    constexpr int U = 8;
    const int lane = threadIdx.x;
    uint8_t *raw = p.raw + im->raw_off;
    const int rows = im->rows, units = im->row_bytes / BPP, pitch = 1 + im->row_bytes, cn = p.channels;
    uint32_t bad_filter = 0, bad_index = 0;
    for (int r0 = 0; r0 < rows; r0 += 64) {
        const int r = r0 + lane;
        const bool live = r < rows;
        uint8_t *line = raw + (size_t)(live ? r : 0) * pitch;
        const uint8_t *above = raw + (size_t)(r0 > 0 ? r0 - 1 : 0) * pitch + 1;
        uint8_t *dst = p.out + im->out_off + (size_t)(live ? r : 0) * p.step;
        int ft = live ? line[0] : 0;
        if (ft > 4) bad_filter = 1, ft = 0;
        const int nlive = min(64, rows - r0);
        const int steps = units + nlive - 1;
        int res[BPP], up[BPP];
        for (int k = 0; k < BPP; k++) res[k] = up[k] = 0;
        for (int t0 = 0; t0 < steps; t0 += U) {
            uint8_t cur[U][BPP], top[U][BPP];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int x = t0 + u - lane;
                const bool in = live && x >= 0 && x < units;
#pragma unroll
                for (int k = 0; k < BPP; k++) {
                    cur[u][k] = in ? line[1 + (size_t)x * BPP + k] : 0;
                    top[u][k] = (in && lane == 0 && r0 > 0) ? above[(size_t)x * BPP + k] : 0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int x = t0 + u - lane;
                const bool in = live && x >= 0 && x < units;
                uint8_t v[BPP];
#pragma unroll
                for (int k = 0; k < BPP; k++) {
                    const int c = up[k], a = res[k];
                    const int fromlane = __shfl_up(res[k], 1);
                    const int b = lane == 0 ? top[u][k] : fromlane;
                    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
                    up[k] = in ? b : 0;
                    res[k] = in ? (cur[u][k] + pred) & 255 : 0;
                    v[k] = (uint8_t)res[k];
                }
                if (in) {
                    emit<BPP>(im, v, x, dst, cn, pal, &bad_index);
                    if (lane == nlive - 1 && r0 + 64 < rows)
                        for (int k = 0; k < BPP; k++) line[1 + (size_t)x * BPP + k] = v[k];
                }
            }
        }
        __syncthreads();  // the band's last row stands before the next band reads it
    }
    if (bad_filter) atomicOr(&dyn->err, (uint32_t)PDEC_ERR_FILTER);
    if (bad_index) atomicOr(&dyn->err, (uint32_t)PDEC_ERR_PALETTE);
}

__global__ __launch_bounds__(64) void pdec_unfilter_kernel(PdecPass p)
{
    const PdecImg *im = p.imgs + blockIdx.x;
    PdecDyn *dyn = p.dyn + blockIdx.x;
    __shared__ uint8_t pal[768];
    if (im->skip || dyn->err) return;
    for (int i = threadIdx.x; i < 768; i += 64) pal[i] = im->pal[i];
    __syncthreads();
    switch (im->bpp) {
    case 1: unfilter_image<1>(p, im, dyn, pal); break;
    case 2: unfilter_image<2>(p, im, dyn, pal); break;
    case 3: unfilter_image<3>(p, im, dyn, pal); break;
    default: unfilter_image<4>(p, im, dyn, pal); break;
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

}  // namespace

int pdec_launch_inflate(const PdecPass &p, hipStream_t s)
{
    pdec_inflate_kernel<<<(unsigned)p.n, 64, 0, s>>>(p);
    return launched("pdec_inflate_kernel");
}

int pdec_launch_adler(const PdecPass &p, int max_chunks, hipStream_t s)
{
    pdec_adler_kernel<<<dim3((unsigned)max_chunks, (unsigned)p.n), 256, 0, s>>>(p);
    if (int rc = launched("pdec_adler_kernel")) return rc;
    pdec_verdict_kernel<<<(unsigned)(p.n + 63) / 64, 64, 0, s>>>(p);
    return launched("pdec_verdict_kernel");
}

int pdec_launch_unfilter(const PdecPass &p, hipStream_t s)
{
    pdec_unfilter_kernel<<<(unsigned)p.n, 64, 0, s>>>(p);
    return launched("pdec_unfilter_kernel");
}

}  // namespace omr
