// png_enc.hip -- PNG encoding on the device: a batch of device-resident gray / BGR / BGRA images
// -> one PNG stream each, lossless and deterministic.  Wave64 kernels for gfx950, a launch per stage, no workgroup waits
// on another:
//   filter     penc_filter_kernel   a workgroup per row: the five filters' sums of absolute values in parallel, the smallest
//                                   wins (ties: the lowest type), its bytes go to the raw buffer with BGR -> RGB in the loads
//   Adler-32   penc_adler_kernel    png_adler.hpp's sums, shared with the decoder
//   matches    penc_match_kernel    a thread per raw byte: the longest run against distance 1, the pixel's bytes and the
//                                   row above, from equality bits in LDS; the best length, ties to the shortest distance
//   parse      penc_parse_kernel    a lane per piece of PENC_PIECE bytes walks greedily: a match of >= 3 cut at the
//                                   piece's end, or a literal; tokens replace the match entries in place
//   blocks     penc_block_kernel    a wave per block of PENC_BLOCK_PIECES pieces: histograms, length-limited canonical
//                                   codes, the code-length code, the sizes as dynamic / fixed / stored, the smallest kept
//              penc_scan_kernel     a workgroup per image: the blocks' byte offsets, the length of the deflate data
//   bits       penc_bits_kernel     a lane per piece packs its codes LSB first into the block's region of the bit buffer
//   streams    penc_copy_kernel     a workgroup per block: its bytes to the stream, and their CRC
//              penc_wrap_kernel     signature, IHDR, IDAT's frame, zlib header, Adler-32, the combined CRC-32, IEND
// Every block but an image's last is followed by an empty stored block, so every block starts on a byte boundary (pigz's
// form) and offsets are sums of byte counts.  Nothing depends on the order in which atomics land: the atomics are integer
// additions (histograms, Adler-32) and ORs into cleared dwords.
#include <hip/hip_runtime.h>

#include "crc32_combine.hpp"
#include "engine.hpp"
#include "png_adler.hpp"
#include "png_enc.hpp"

namespace omr {
namespace {

constexpr uint32_t kTokMatch = 0x8000;  // a token / match entry: kTokMatch | candidate << 8 | length - 3; else a literal byte
constexpr uint32_t kLimit15 = 2584;     // a Huffman tree over weights that sum to less than Fibonacci(18) is at most 15 deep
constexpr uint32_t kLimit7 = 55;        // ... less than Fibonacci(10): at most 7 deep

__device__ inline int paeth(int a, int b, int c)
{
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

__device__ inline uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- filter.  LDS: 5 x 4 dwords + 1.
// Byte loads throughout: any base and any pitch; neighbouring lanes read neighbouring bytes.
// Bounds: r < rows, x < row_bytes, so every source byte read lies in rows r - 1 (r > 0 only) and r of the image, and the
// row written is raw[r * (1 + row_bytes) .. + row_bytes] inside raw_len.
__global__ __launch_bounds__(256) void penc_filter_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= im.rows) return;
    const int bpp = p.cn, rb = im.row_bytes;
    const uint8_t *cur = p.src + im.src_off + (int64_t)r * p.step;
    const uint8_t *up = cur - p.step;  // read for r > 0 only
    __shared__ uint32_t part[5][4];
    __shared__ int chosen;
    uint32_t s[5] = {0, 0, 0, 0, 0};
    auto filtered = [&](int x, int f[5]) {
        const int ch = x % bpp;
        const int sx = x - ch + (bpp >= 3 && ch < 3 ? 2 - ch : ch);  // BGR(A) in memory, RGB(A) in the file
        const int v = cur[sx];
        const int a = x >= bpp ? cur[sx - bpp] : 0;
        const int b = r > 0 ? up[sx] : 0;
        const int c = r > 0 && x >= bpp ? up[sx - bpp] : 0;
        f[0] = v, f[1] = (v - a) & 255, f[2] = (v - b) & 255, f[3] = (v - ((a + b) >> 1)) & 255, f[4] = (v - paeth(a, b, c)) & 255;
    };
    for (int x = threadIdx.x; x < rb; x += 256) {
        int f[5];
        filtered(x, f);
        for (int k = 0; k < 5; k++) s[k] += f[k] < 128 ? f[k] : 256 - f[k];  // at most 2^22 bytes of 128: no overflow
    }
    for (int k = 0; k < 5; k++) {
        const uint32_t t = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        uint32_t best_sum = 0;
        for (int k = 0; k < 5; k++) {
            const uint32_t t = part[k][0] + part[k][1] + part[k][2] + part[k][3];
            if (k == 0 || t < best_sum) best = k, best_sum = t;  // ties: the lowest type
        }
        chosen = best;
    }
    __syncthreads();
    const int type = chosen;
    uint8_t *dst = p.raw + im.raw_off + (int64_t)r * (rb + 1);
    if (threadIdx.x == 0) dst[0] = (uint8_t)type;
    for (int x = threadIdx.x; x < rb; x += 256) {
        int f[5];
        filtered(x, f);
        dst[1 + x] = (uint8_t)f[type];
    }
}

__global__ __launch_bounds__(256) void penc_adler_kernel(PencPass p)
{
    const PencImg *im = p.imgs + blockIdx.y;
    PencDyn *dyn = p.dyn + blockIdx.y;
    adler_chunk_sums(p.raw + im->raw_off, im->raw_len, blockIdx.x, &dyn->a_sum, &dyn->b_sum);
}

// ---- matches.  LDS: 12 x 8 bytes.  A workgroup takes 256 positions; per candidate distance d it sets bit q - P0 where
// raw[q] == raw[q - d] for the 768 positions from its first on (q < raw_len and q >= d, else 0), and a position's run is
// the distance to the next zero bit: at most 255 + 258 < 768 bits ahead.
// Bounds: every raw byte read has an index q or q - d with d <= q < raw_len; the entry written is mt[p], p < raw_len.
__global__ __launch_bounds__(256) void penc_match_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.y];
    const uint32_t n = im.raw_len;
    const uint64_t P0 = (uint64_t)blockIdx.x * 256;
    if (P0 >= n) return;
    const uint8_t *raw = p.raw + im.raw_off;
    __shared__ unsigned long long mask[12];
    const uint32_t dist[3] = {1u, (uint32_t)p.cn, (uint32_t)im.row_bytes + 1u};
    const int tid = threadIdx.x;
    int best = 0, best_c = 0;
    for (int c = 0; c < 3; c++) {
        const uint32_t d = dist[c];
        if ((c == 1 && d == 1) || d > (uint32_t)PENC_MAX_DISTANCE) continue;  // uniform
        for (int j = 0; j < 3; j++) {
            const uint64_t q = P0 + (uint64_t)(tid + 256 * j);
            const bool e = q < n && q >= d && raw[q] == raw[q - d];
            const unsigned long long m = __ballot(e);
            if ((tid & 63) == 0) mask[j * 4 + (tid >> 6)] = m;
        }
        __syncthreads();
        int w = tid >> 6;
        const int b = tid & 63;
        int len;
        unsigned long long inv = ~mask[w] >> b;  // zeros come in at the top: "no zero bit seen"
        if (inv) {
            len = __ffsll((long long)inv) - 1;
        } else {
            len = 64 - b;
            for (w++; w < 12 && len < 258; w++) {
                inv = ~mask[w];
                if (inv) {
                    len += __ffsll((long long)inv) - 1;
                    break;
                }
                len += 64;
            }
        }
        len = min(len, 258);
        if (len > best) best = len, best_c = c;  // on equal length the shorter distance stays
        __syncthreads();
    }
    const uint64_t pos = P0 + tid;
    if (pos < n) p.mt[im.raw_off + (int64_t)pos] = best >= 3 ? (uint16_t)(kTokMatch | best_c << 8 | (best - 3)) : (uint16_t)0;
}

// ---- parse.  A lane per piece; the only sequential loop of the encoder, at most PENC_PIECE steps (pos grows every step).
// Tokens overwrite the match entries of the piece: token number t is written at start + t with t <= pos - start, an entry
// this lane has already read.
// Bounds: pos < end <= raw_len for every raw byte and entry read; start + cnt <= pos < end for every token written.
__global__ __launch_bounds__(64) void penc_parse_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.y];
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= im.npiece) return;
    const uint32_t start = k * PENC_PIECE, end = min(start + (uint32_t)PENC_PIECE, im.raw_len);
    const uint8_t *raw = p.raw + im.raw_off;
    uint16_t *t = p.mt + im.raw_off;
    uint32_t pos = start, cnt = 0;
    while (pos < end) {
        const uint32_t e = t[pos];
        uint32_t tok = raw[pos], adv = 1;
        if (e & kTokMatch) {
            const uint32_t len = min((e & 255) + 3, end - pos);
            if (len >= 3) tok = kTokMatch | (e & 0x300) | (len - 3), adv = len;
        }
        t[start + cnt] = (uint16_t)tok;
        cnt++, pos += adv;
    }
    p.piece_cnt[im.blk0 * PENC_BLOCK_PIECES + k] = (uint16_t)cnt;
}

// ---- symbols
__device__ inline void length_symbol(uint32_t l, uint32_t *sym, uint32_t *ebits, uint32_t *eval)  // l = length - 3
{
    if (l == 255) {
        *sym = 28, *ebits = 0, *eval = 0;
    } else if (l < 8) {
        *sym = l, *ebits = 0, *eval = 0;
    } else {
        const uint32_t nb = 31 - __clz(l);
        *sym = 4 * (nb - 1) + ((l >> (nb - 2)) & 3), *ebits = nb - 2, *eval = l & ((1u << (nb - 2)) - 1);
    }
}
__device__ inline void distance_symbol(uint32_t d, uint32_t *sym, uint32_t *ebits, uint32_t *eval)  // 1 .. 32768
{
    if (d <= 4) {
        *sym = d - 1, *ebits = 0, *eval = 0;
    } else {
        const uint32_t nb = 31 - __clz(d - 1);
        *sym = 2 * nb + (((d - 1) >> (nb - 1)) & 1), *ebits = nb - 1, *eval = (d - 1) & ((1u << (nb - 1)) - 1);
    }
}
__device__ inline uint32_t length_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }  // sym 257 ..
__device__ inline uint32_t distance_extra(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
__device__ inline uint32_t fixed_length(uint32_t sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
__device__ inline uint32_t fixed_code(uint32_t sym)
{
    return sym < 144 ? 0x30 + sym : sym < 256 ? 0x190 + (sym - 144) : sym < 280 ? sym - 256 : 0xC0 + (sym - 280);
}
__device__ inline uint32_t packed_code(uint32_t code, uint32_t len) { return len ? (__brev(code) >> (32 - len)) | len << 16 : 0; }

// Code lengths of a Huffman code over freq[0 .. n), by the whole wave.  Rules, restated in tests/png_enc_ref.py:
//   - fewer than two symbols in use: the lowest-numbered unused ones join with weight 1 (zlib's build_tree pads likewise),
//     so the set is complete with at least two codes;
//   - weights are max(1, freq >> s) for the smallest s with a sum below `limit`.  A Huffman tree of depth d weighs at
//     least Fibonacci(d + 2), so the sum bounds the depth: 15 bits below 2584, 7 bits below 55.  The loop over s is
//     bounded by construction: freq < 2^16, so at s = 16 every weight is 1 and the sum is at most n < limit;
//   - the two nodes of the smallest (weight, index) merge; leaves have their symbol as index, merge number m gets n + m.
// key / par hold 2 n entries.  Leaves the wave behind a barrier.
__device__ void build_lengths(const uint32_t *freq, int n, uint32_t limit, uint8_t *len, uint32_t *key, uint16_t *par)
{
    const int lane = threadIdx.x;
    uint32_t used = 0;
    for (int i = lane; i < n; i += 64) used += freq[i] != 0;
    used = wave_sum(used);
    int pad0 = -1, pad1 = -1;
    if (used < 2)
        for (int i = 0, need = 2 - (int)used; i < 3 && need; i++)
            if (freq[i] == 0) (pad0 < 0 ? pad0 : pad1) = i, need--;
    auto weight = [&](int i) -> uint32_t { return freq[i] ? freq[i] : (i == pad0 || i == pad1) ? 1u : 0u; };
    int s = 0;
    for (; s < 16; s++) {
        uint32_t t = 0;
        for (int i = lane; i < n; i += 64) {
            const uint32_t w = weight(i);
            t += w ? max(1u, w >> s) : 0u;
        }
        if (wave_sum(t) < limit) break;
    }
    uint32_t alive = 0;
    for (int i = lane; i < n; i += 64) {
        const uint32_t w = weight(i);
        key[i] = w ? max(1u, w >> s) << 10 | (uint32_t)i : 0xffffffffu;
        alive += w != 0;
    }
    alive = wave_sum(alive);
    __syncthreads();
    int nodes = n;
    for (uint32_t m = 0; m + 1 < alive; m++, nodes++) {  // alive <= n merges
        uint32_t m1 = 0xffffffffu, m2 = 0xffffffffu;
        for (int i = lane; i < nodes; i += 64) {
            const uint32_t k = key[i];
            if (k < m1) m2 = m1, m1 = k;
            else if (k < m2) m2 = k;
        }
        for (int o = 32; o; o >>= 1) {
            const uint32_t o1 = __shfl_xor(m1, o), o2 = __shfl_xor(m2, o);
            if (o1 < m1) m2 = min(m1, o2), m1 = o1;
            else m2 = min(m2, o1);
        }
        if (lane == 0) {
            par[m1 & 1023] = par[m2 & 1023] = (uint16_t)nodes;
            key[m1 & 1023] = key[m2 & 1023] = 0xffffffffu;
            key[nodes] = ((m1 >> 10) + (m2 >> 10)) << 10 | (uint32_t)nodes;
        }
        __syncthreads();
    }
    const int root = nodes - 1;
    for (int i = lane; i < n; i += 64) {
        int d = 0;
        if (weight(i))
            for (int j = i; d < 15 && j != root; d++) j = par[j];
        len[i] = (uint8_t)d;
    }
    __syncthreads();
}

// canonical codes of len[0 .. n) (one lane): bit-reversed code | length << 16
__device__ void assign_codes(const uint8_t *len, int n, uint32_t *out)
{
    uint32_t count[16], next[16];
    for (int k = 0; k < 16; k++) count[k] = 0;
    for (int i = 0; i < n; i++) count[len[i]]++;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int k = 1; k < 16; k++) code = (code + count[k - 1]) << 1, next[k] = code;
    for (int i = 0; i < n; i++) out[i] = len[i] ? packed_code(next[len[i]]++, len[i]) : 0;
}

struct LdsBits {
    uint32_t *w;
    uint32_t n = 0;
    __device__ void put(uint32_t v, uint32_t bits)
    {
        if (!bits) return;
        const uint32_t at = n >> 5, sh = n & 31;
        w[at] |= v << sh;
        if (sh + bits > 32) w[at + 1] |= v >> (32 - sh);
        n += bits;
    }
};

// ---- blocks.  One wave per block.  LDS: freq 316 x 4, key 572 x 4, par 572 x 2, lengths 316 + 19, code-length
// frequencies and codes 2 x 19 x 4, run-length entries 316 x 2, the sequence 316, codes 316 x 4, header 144 x 4:
// about 8.3 KB.  Every barrier is in control flow that is uniform over the wave (b, stored_only and the loop counts are).
// Bounds: piece k < pieces of the block, token t < piece_cnt <= bytes of the piece, so every entry read lies in the
// block's raw range; codes / hdr / blk / piece_bit are indexed by the block's and the pieces' numbers in the launch.
__global__ __launch_bounds__(64) void penc_block_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= im.nblk) return;
    const int lane = threadIdx.x;
    const int64_t gb = im.blk0 + b;
    const uint32_t raw0 = b * PENC_BLOCK, rawn = min((uint32_t)PENC_BLOCK, im.raw_len - raw0);
    const uint32_t np = (rawn + PENC_PIECE - 1) / PENC_PIECE;
    const bool last = b + 1 == im.nblk;
    const uint32_t stored_bytes = PENC_STORED_HEAD + rawn;
    if (p.stored_only) {
        if (lane == 0) p.blk[gb] = PencBlk{PENC_STORED, 0, 0, stored_bytes, 0, 0};
        return;
    }
    __shared__ uint32_t fl[286], fd[30], fc[19], key[572], codes[PENC_CODES], ccode[19], hdr[PENC_HDR_WORDS];
    __shared__ uint16_t par[572], rle[PENC_CODES];
    __shared__ uint8_t lenL[286], lenD[30], lenC[19], seq[PENC_CODES];
    __shared__ uint32_t sh_hdr_bits, sh_nrle;
    uint32_t dsym[3], debits[3], deval[3];
    distance_symbol(1, &dsym[0], &debits[0], &deval[0]);
    distance_symbol((uint32_t)p.cn, &dsym[1], &debits[1], &deval[1]);
    distance_symbol(min((uint32_t)im.row_bytes + 1u, (uint32_t)PENC_MAX_DISTANCE), &dsym[2], &debits[2], &deval[2]);
    for (int i = lane; i < 286; i += 64) fl[i] = 0;
    if (lane < 30) fd[lane] = 0;
    if (lane < 19) fc[lane] = 0;
    for (int i = lane; i < PENC_HDR_WORDS; i += 64) hdr[i] = 0;
    __syncthreads();
    const uint16_t *tok = p.mt + im.raw_off + raw0;
    const int64_t gp = gb * PENC_BLOCK_PIECES;
    for (uint32_t k = 0; k < np; k++) {
        const uint32_t cnt = p.piece_cnt[gp + k];
        for (uint32_t t = lane; t < cnt; t += 64) {
            const uint32_t e = tok[k * PENC_PIECE + t];
            if (e & kTokMatch) {
                uint32_t ls, lb, lv;
                length_symbol(e & 255, &ls, &lb, &lv);
                atomicAdd(&fl[257 + ls], 1u);
                atomicAdd(&fd[dsym[(e >> 8) & 3]], 1u);
            } else {
                atomicAdd(&fl[e], 1u);
            }
        }
    }
    if (lane == 0) atomicAdd(&fl[256], 1u);
    __syncthreads();
    build_lengths(fl, 286, kLimit15, lenL, key, par);
    build_lengths(fd, 30, kLimit15, lenD, key, par);
    if (lane == 0) {
        int hlit = 286, hdist = 30;
        while (hlit > 257 && lenL[hlit - 1] == 0) hlit--;
        while (hdist > 1 && lenD[hdist - 1] == 0) hdist--;
        int ns = 0;
        for (int i = 0; i < hlit; i++) seq[ns++] = lenL[i];
        for (int i = 0; i < hdist; i++) seq[ns++] = lenD[i];
        // the lengths of both sets as one sequence, run-length coded: entries of symbol | extra value << 5
        int nr = 0;
        for (int i = 0; i < ns;) {
            const int v = seq[i];
            int j = i;
            while (j < ns && seq[j] == v) j++;
            int run = j - i;
            if (v == 0) {
                while (run >= 11) {
                    const int k = min(run, 138);
                    rle[nr++] = (uint16_t)(18 | (k - 11) << 5), run -= k;
                }
                if (run >= 3) rle[nr++] = (uint16_t)(17 | (run - 3) << 5), run = 0;
            } else {
                rle[nr++] = (uint16_t)v, run--;
                while (run >= 3) {
                    const int k = min(run, 6);
                    rle[nr++] = (uint16_t)(16 | (k - 3) << 5), run -= k;
                }
            }
            for (; run > 0; run--) rle[nr++] = (uint16_t)v;
            i = j;
        }
        for (int i = 0; i < nr; i++) fc[rle[i] & 31]++;
        sh_nrle = (uint32_t)nr;
        sh_hdr_bits = (uint32_t)(hlit << 16 | hdist);
    }
    __syncthreads();
    build_lengths(fc, 19, kLimit7, lenC, key, par);
    if (lane == 0) {
        const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const int hlit = (int)(sh_hdr_bits >> 16), hdist = (int)(sh_hdr_bits & 0xffff);
        assign_codes(lenC, 19, ccode);
        assign_codes(lenL, 286, codes);
        assign_codes(lenD, 30, codes + 286);
        int hclen = 19;
        while (hclen > 4 && lenC[order[hclen - 1]] == 0) hclen--;
        LdsBits w{hdr};
        w.put((last ? 1u : 0u) | 2u << 1, 3);
        w.put((uint32_t)(hlit - 257), 5), w.put((uint32_t)(hdist - 1), 5), w.put((uint32_t)(hclen - 4), 4);
        for (int i = 0; i < hclen; i++) w.put(lenC[order[i]], 3);
        const int nr = (int)sh_nrle;
        for (int i = 0; i < nr; i++) {
            const uint32_t sym = rle[i] & 31, extra = rle[i] >> 5;
            w.put(ccode[sym] & 0xffff, ccode[sym] >> 16);
            w.put(extra, sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        sh_hdr_bits = w.n;
    }
    __syncthreads();
    // the three sizes
    uint32_t dyn_body = 0, fix_body = 0;
    for (int i = lane; i < 286; i += 64) {
        const uint32_t x = i >= 257 ? length_extra((uint32_t)i) : 0;
        dyn_body += fl[i] * (lenL[i] + x), fix_body += fl[i] * (fixed_length((uint32_t)i) + x);
    }
    if (lane < 30) dyn_body += fd[lane] * (lenD[lane] + distance_extra((uint32_t)lane)), fix_body += fd[lane] * (5 + distance_extra((uint32_t)lane));
    const uint32_t dyn_bits = sh_hdr_bits + wave_sum(dyn_body), fix_bits = 3 + wave_sum(fix_body);
    auto bytes_of = [&](uint32_t bits) { return last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4; };
    uint32_t type = PENC_STORED, nbytes = stored_bytes, bits = 0, hdr_bits = 0;
    if (bytes_of(fix_bits) < nbytes) type = PENC_FIXED, nbytes = bytes_of(fix_bits), bits = fix_bits, hdr_bits = 3;
    if (bytes_of(dyn_bits) < nbytes) type = PENC_DYNAMIC, nbytes = bytes_of(dyn_bits), bits = dyn_bits, hdr_bits = sh_hdr_bits;
    if (lane == 0) p.blk[gb] = PencBlk{type, hdr_bits, bits, nbytes, 0, 0};
    if (type == PENC_STORED) return;  // uniform
    __syncthreads();
    if (type == PENC_FIXED) {
        for (int i = lane; i < 286; i += 64) codes[i] = packed_code(fixed_code((uint32_t)i), fixed_length((uint32_t)i));
        if (lane < 30) codes[286 + lane] = packed_code((uint32_t)lane, 5);
        if (lane == 0) hdr[0] = (last ? 1u : 0u) | 1u << 1;
        __syncthreads();
    }
    for (int i = lane; i < PENC_CODES; i += 64) p.codes[gb * PENC_CODES + i] = codes[i];
    for (uint32_t i = lane; i < (hdr_bits + 31) / 32; i += 64) p.hdr[gb * PENC_HDR_WORDS + i] = hdr[i];
    // where every piece's codes start, behind the header
    uint32_t run = 0;
    for (uint32_t k = 0; k < np; k++) {
        const uint32_t cnt = p.piece_cnt[gp + k];
        uint32_t sum = 0;
        for (uint32_t t = lane; t < cnt; t += 64) {
            const uint32_t e = tok[k * PENC_PIECE + t];
            if (e & kTokMatch) {
                uint32_t ls, lb, lv;
                length_symbol(e & 255, &ls, &lb, &lv);
                const uint32_t c = (e >> 8) & 3;
                sum += (codes[257 + ls] >> 16) + lb + (codes[286 + dsym[c]] >> 16) + debits[c];
            } else {
                sum += codes[e] >> 16;
            }
        }
        if (lane == 0) p.piece_bit[gp + k] = run;
        run += wave_sum(sum);
    }
}

// ---- placement.  A workgroup per image walks its blocks 256 at a time with a running sum.  LDS: 256 x 4.
__global__ __launch_bounds__(256) void penc_scan_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.x];
    __shared__ uint32_t sc[256];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < im.nblk; base += 256) {  // uniform
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < im.nblk ? p.blk[im.blk0 + i].nbytes : 0;
        sc[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t add = (int)threadIdx.x >= d ? sc[threadIdx.x - d] : 0;
            __syncthreads();
            sc[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < im.nblk) p.blk[im.blk0 + i].byte_off = carry + sc[threadIdx.x] - v;
        carry += sc[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.dyn[blockIdx.x].deflate_len = carry;
}

// A lane's bits into the cleared bit buffer, LSB first.  The lane owns the bit range it writes; the dwords that lie
// wholly inside it are stored, the first and the last one, which a neighbour may share, are ORed in atomically -- the
// result does not depend on who comes first.
struct BitPut {
    uint32_t *w;
    unsigned long long acc = 0;
    uint32_t nb;
    bool first = true;
    __device__ BitPut(uint32_t *base, uint32_t bitpos) : w(base + (bitpos >> 5)), nb(bitpos & 31) {}
    __device__ void put(uint32_t v, uint32_t bits)  // bits <= 32, v below 2^bits
    {
        acc |= (unsigned long long)v << nb;
        nb += bits;
        if (nb >= 32) {
            if (first) atomicOr(w, (uint32_t)acc), first = false;
            else *w = (uint32_t)acc;
            w++, acc >>= 32, nb -= 32;
        }
    }
    __device__ void finish()
    {
        if (nb) atomicOr(w, (uint32_t)acc);
    }
};

// ---- bit writer.  A wave per block: lane k < pieces writes piece k's codes, lane PENC_BLOCK_PIECES the header, the next
// one the end-of-block code and, behind every block but the last, the empty stored block (000, padding, 00 00 FF FF).
// Bounds: every bit written lies below 8 x nbytes of the block, nbytes <= 5 + PENC_BLOCK < PENC_ZBLOCK: inside the
// block's region of zbuf.
__global__ __launch_bounds__(64) void penc_bits_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= im.nblk) return;
    const int64_t gb = im.blk0 + b;
    const PencBlk blk = p.blk[gb];
    if (blk.type == PENC_STORED) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t raw0 = b * PENC_BLOCK, rawn = min((uint32_t)PENC_BLOCK, im.raw_len - raw0);
    const uint32_t np = (rawn + PENC_PIECE - 1) / PENC_PIECE;
    uint32_t *z = p.zbuf + gb * (PENC_ZBLOCK / 4);
    const uint32_t *codes = p.codes + gb * PENC_CODES;
    if (lane < np) {
        uint32_t dsym[3], debits[3], deval[3];
        distance_symbol(1, &dsym[0], &debits[0], &deval[0]);
        distance_symbol((uint32_t)p.cn, &dsym[1], &debits[1], &deval[1]);
        distance_symbol(min((uint32_t)im.row_bytes + 1u, (uint32_t)PENC_MAX_DISTANCE), &dsym[2], &debits[2], &deval[2]);
        const int64_t gp = gb * PENC_BLOCK_PIECES + lane;
        const uint16_t *tok = p.mt + im.raw_off + raw0 + lane * PENC_PIECE;
        const uint32_t cnt = p.piece_cnt[gp];
        BitPut w(z, blk.hdr_bits + p.piece_bit[gp]);
        for (uint32_t t = 0; t < cnt; t++) {
            const uint32_t e = tok[t];
            if (e & kTokMatch) {
                uint32_t ls, lb, lv;
                length_symbol(e & 255, &ls, &lb, &lv);
                const uint32_t c = (e >> 8) & 3, lc = codes[257 + ls], dc = codes[286 + dsym[c]];
                w.put((lc & 0xffff) | lv << (lc >> 16), (lc >> 16) + lb);             // <= 15 + 5 bits
                w.put((dc & 0xffff) | deval[c] << (dc >> 16), (dc >> 16) + debits[c]);  // <= 15 + 13 bits
            } else {
                w.put(codes[e] & 0xffff, codes[e] >> 16);
            }
        }
        w.finish();
    } else if (lane == PENC_BLOCK_PIECES) {
        const uint32_t *h = p.hdr + gb * PENC_HDR_WORDS;
        BitPut w(z, 0);
        for (uint32_t i = 0; i < blk.hdr_bits / 32; i++) w.put(h[i], 32);
        if (blk.hdr_bits & 31) w.put(h[blk.hdr_bits / 32] & ((1u << (blk.hdr_bits & 31)) - 1), blk.hdr_bits & 31);
        w.finish();
    } else if (lane == PENC_BLOCK_PIECES + 1) {
        const uint32_t eob = codes[256];
        BitPut w(z, blk.bits - (eob >> 16));
        w.put(eob & 0xffff, eob >> 16);
        if (b + 1 != im.nblk) {
            w.put(0, 3 + ((0u - (blk.bits + 3)) & 7));
            w.put(0, 16);
            w.put(0xffff, 16);
        }
        w.finish();
    }
}

// ---- streams.  A workgroup per block copies its bytes (a stored block's from the raw buffer) and computes their CRC: a
// register per thread over a contiguous part, shifted by what lies behind it in the block.  LDS: 256 x 4 x 2.
// Bounds: i < nbytes; the destination byte is PENC_BEFORE + byte_off + i < PENC_BEFORE + deflate_len of the image's stream.
__global__ __launch_bounds__(256) void penc_copy_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= im.nblk) return;
    const int64_t gb = im.blk0 + b;
    const PencBlk blk = p.blk[gb];
    const uint32_t raw0 = b * PENC_BLOCK, rawn = min((uint32_t)PENC_BLOCK, im.raw_len - raw0);
    const uint8_t *raw = p.raw + im.raw_off + raw0;
    const uint8_t *z = (const uint8_t *)(p.zbuf + gb * (PENC_ZBLOCK / 4));
    const bool stored = blk.type == PENC_STORED, last = b + 1 == im.nblk;
    auto get = [&](uint32_t i) -> uint32_t {
        if (!stored) return z[i];
        if (i >= PENC_STORED_HEAD) return raw[i - PENC_STORED_HEAD];
        return i == 0 ? (last ? 1u : 0u) : i == 1 ? rawn & 255 : i == 2 ? rawn >> 8 : i == 3 ? ~rawn & 255 : (~rawn >> 8) & 255;
    };
    uint8_t *dst = p.out + im.out_off + PENC_BEFORE + blk.byte_off;
    for (uint32_t i = threadIdx.x; i < blk.nbytes; i += 256) dst[i] = (uint8_t)get(i);
    __shared__ uint32_t tab[256], part[256];
    {
        uint32_t c = threadIdx.x;
        for (int k = 0; k < 8; k++) c = c & 1 ? CRC_POLY ^ (c >> 1) : c >> 1;
        tab[threadIdx.x] = c;
    }
    __syncthreads();
    const uint32_t per = (blk.nbytes + 255) / 256;
    const uint32_t lo = min(threadIdx.x * per, blk.nbytes), hi = min(lo + per, blk.nbytes);
    uint32_t c = 0;
    for (uint32_t i = lo; i < hi; i++) c = tab[(c ^ get(i)) & 255] ^ (c >> 8);
    if (lo < hi && hi < blk.nbytes) c = crc_shift(c, blk.nbytes - hi);
    part[threadIdx.x] = c;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] ^= part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.blk[gb].crc = part[0];
}

// A workgroup per image: the blocks' CRCs shifted to the end of IDAT's data and XORed together, then everything around the
// deflate data.  LDS: 256 x 4.
// Bounds: the stream is PENC_BEFORE + deflate_len + PENC_AFTER bytes, the length the host placed it with.
__global__ __launch_bounds__(256) void penc_wrap_kernel(PencPass p)
{
    const PencImg im = p.imgs[blockIdx.x];
    if (im.rows == 0) return;
    const PencDyn dyn = p.dyn[blockIdx.x];
    const uint32_t dl = dyn.deflate_len;
    __shared__ uint32_t part[256];
    uint32_t acc = 0;
    for (uint32_t i = threadIdx.x; i < im.nblk; i += 256) {
        const PencBlk blk = p.blk[im.blk0 + i];
        acc ^= crc_shift(blk.crc, (uint64_t)(dl - blk.byte_off - blk.nbytes) + 4);
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] ^= part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    uint8_t *o = p.out + im.out_off;
    auto be32 = [](uint8_t *q, uint32_t v) { q[0] = (uint8_t)(v >> 24), q[1] = (uint8_t)(v >> 16), q[2] = (uint8_t)(v >> 8), q[3] = (uint8_t)v; };
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int k = 0; k < 8; k++) o[k] = sig[k];
    be32(o + 8, 13);
    o[12] = 'I', o[13] = 'H', o[14] = 'D', o[15] = 'R';
    be32(o + 16, (uint32_t)im.cols), be32(o + 20, (uint32_t)im.rows);
    o[24] = 8, o[25] = (uint8_t)(p.cn == 1 ? 0 : p.cn == 3 ? 2 : 6), o[26] = 0, o[27] = 0, o[28] = 0;
    uint32_t c = 0xffffffffu;
    for (int k = 12; k < 29; k++) c = crc_byte(c, o[k]);
    be32(o + 29, ~c);
    be32(o + 33, 2 + dl + 4);
    o[37] = 'I', o[38] = 'D', o[39] = 'A', o[40] = 'T';
    o[41] = 0x78, o[42] = 0x01;  // deflate with a 32 K window, no dictionary, "fastest"
    c = 0xffffffffu;
    for (int k = 37; k < 43; k++) c = crc_byte(c, o[k]);
    uint8_t *t = o + PENC_BEFORE + dl;
    be32(t, adler_finish(im.raw_len, dyn.a_sum, dyn.b_sum));
    uint32_t tail = 0;
    for (int k = 0; k < 4; k++) tail = crc_byte(tail, t[k]);
    c = crc_shift(c, (uint64_t)dl + 4) ^ part[0] ^ tail;
    be32(t + 4, ~c);
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int k = 0; k < 12; k++) t[8 + k] = iend[k];
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

unsigned up_div(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

int penc_launch_filter(const PencPass &p, int max_rows, hipStream_t s)
{
    penc_filter_kernel<<<dim3((unsigned)max_rows, (unsigned)p.n), 256, 0, s>>>(p);
    return launched("penc_filter_kernel");
}

int penc_launch_adler(const PencPass &p, int64_t max_raw, hipStream_t s)
{
    penc_adler_kernel<<<dim3(up_div(max_raw, PNG_ADLER_CHUNK), (unsigned)p.n), 256, 0, s>>>(p);
    return launched("penc_adler_kernel");
}

int penc_launch_parse(const PencPass &p, int64_t max_raw, int max_pieces, hipStream_t s)
{
    penc_match_kernel<<<dim3(up_div(max_raw, 256), (unsigned)p.n), 256, 0, s>>>(p);
    if (int rc = launched("penc_match_kernel")) return rc;
    penc_parse_kernel<<<dim3(up_div(max_pieces, 64), (unsigned)p.n), 64, 0, s>>>(p);
    return launched("penc_parse_kernel");
}

int penc_launch_blocks(const PencPass &p, int max_blocks, hipStream_t s)
{
    penc_block_kernel<<<dim3((unsigned)max_blocks, (unsigned)p.n), 64, 0, s>>>(p);
    if (int rc = launched("penc_block_kernel")) return rc;
    penc_scan_kernel<<<(unsigned)p.n, 256, 0, s>>>(p);
    return launched("penc_scan_kernel");
}

int penc_launch_bits(const PencPass &p, int max_blocks, hipStream_t s)
{
    penc_bits_kernel<<<dim3((unsigned)max_blocks, (unsigned)p.n), 64, 0, s>>>(p);
    return launched("penc_bits_kernel");
}

int penc_launch_streams(const PencPass &p, int max_blocks, hipStream_t s)
{
    penc_copy_kernel<<<dim3((unsigned)max_blocks, (unsigned)p.n), 256, 0, s>>>(p);
    if (int rc = launched("penc_copy_kernel")) return rc;
    penc_wrap_kernel<<<(unsigned)p.n, 256, 0, s>>>(p);
    return launched("penc_wrap_kernel");
}

}  // namespace omr
