// tiff_dec8.hip -- 8-bit gray and RGB TIFF on the device: the LZW decoder, one wave per strip,
// 64 codes a round; and the finishing kernel that turns raw rows (uploaded, or decoded by tdec_packbits / tdec_lzw into
// the workspace) into the output slots: horizontal differencing undone, Photometric 0 inverted, RGB turned to BGR.
//
// Bounds.  Everything a kernel loops over is fixed on the host: a strip's byte length, its rows, the row's bytes.  A round
// of tdec_lzw consumes at least 9 bits of the strip's bit length or ends the strip; no code is read that ends behind the
// strip's last bit.  Output bytes go to base + t with t below the strip's remaining room, so inside its rows x pitch of the
// workspace.  A byte's source is a literal, or a position of the strip's output below the round's first byte (an older
// entry, the previous code), found by walking at most 64 steps down the codes of the round: a code names entries made by
// codes in front of it only (tlzw_check), so every step goes to a lower lane.  Table reads are of entries 258 .. 256 + ci,
// all written since the last Clear; table writes are of entries <= 4095 (tlzw_check).
#include <hip/hip_runtime.h>

#include "../../include/omrdeskew.h"
#include "engine.hpp"
#include "tiff_dec.hpp"
#include "tiff_lzw.hpp"

namespace omr {
namespace {

constexpr int LZW_WIN = 1024;  // a strip's input window in LDS; a round reads at most 64 x 12 bits and two bytes
constexpr int LZW_LIT = -2, LZW_OLD = -3;  // a code's kind; >= -1: the lane whose output, with one more byte, is its entry
constexpr uint32_t LZW_VALUE = 0x80000000u;  // a first byte known by value, not by position

struct LzwBytes {
    const uint8_t *in;   // the strip in global memory
    const uint8_t *win;  // its window in LDS: bytes wbase .. wbase + LZW_WIN
    uint32_t len, wbase;
    __device__ uint32_t operator()(uint32_t i) const
    {
        if (i >= len) return 0;
        const uint32_t o = i - wbase;
        return o < (uint32_t)LZW_WIN ? win[o] : in[i];
    }
};

// ---- LZW: one wave per strip.  A round: every lane cuts one code from the bit stream (a code's place depends on its index
// since the last Clear alone); a ballot finds the first Clear, EOI or refused code; the lengths of the codes in front of
// it are resolved (a code that names an entry made in this round is one byte longer than the code in front of that
// entry's maker) and scanned into output positions; every lane adds its entry; then the wave copies the round's bytes,
// a byte a lane, each from its source below the round's first byte.  What stays serial: the rounds of a strip, and inside
// a round the walk down a chain of codes that name each other's entries (a constant page: up to 64 steps).
__global__ void __launch_bounds__(64) tdec_lzw(const uint8_t *__restrict__ src, const TdecStrip *__restrict__ strips, TdecDyn *dyn,
                                               uint8_t *raw)
{
    __shared__ uint32_t tab_pos[TLZW_ENTRIES];
    __shared__ uint16_t tab_len[TLZW_ENTRIES];
    __shared__ uint32_t win[LZW_WIN / 4];
    __shared__ uint32_t r_off[64], r_len[64], r_src[64], r_first[64];
    __shared__ int32_t r_dep[64];
    const TdecStrip st = strips[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const uint8_t *in = src + st.src_off;  // src_off is a multiple of 16
    const uint32_t len = st.src_len, bitlen = len * 8;  // len < 2^28
    const uint32_t total = (uint32_t)st.rows * (uint32_t)st.pitch;
    uint8_t *out = raw + st.dst_off;
    uint32_t pos = 0, ci = 0, base = 0, prev_pos = 0, prev_len = 0, err = 0, wbase = 0;
    bool started = false;
    for (;;) {  // a round a turn: at least 9 bits of bitlen, or the last
        if (!started || (pos >> 3) - wbase + 104 > (uint32_t)LZW_WIN) {  // the window follows the reader
            __syncthreads();
            wbase = (pos >> 3) & ~3u;
            for (int i = lane; i < LZW_WIN / 4; i += 64) {
                const uint32_t at = wbase + 4 * (uint32_t)i;
                uint32_t w = 0;
                if (at < len && at + 4 <= len) w = *(const uint32_t *)(in + at);
                else
                    for (uint32_t k = 0; k < 4 && at + k < len; k++) w |= (uint32_t)in[at + k] << (8 * k);
                win[i] = w;
            }
            __syncthreads();
        }
        const LzwBytes byte{in, (const uint8_t *)win, len, wbase};
        if (!started) {  // a strip begins with Clear
            const uint32_t c = tlzw_code(byte, 0, 9, bitlen);
            if (c != TLZW_CLEAR) {
                err = c == TLZW_MISSING ? TLZW_ERR_INPUT : TLZW_ERR_CODE;
                break;
            }
            pos = 9, started = true;
            continue;
        }
        const uint32_t i = ci + (uint32_t)lane;
        const uint32_t w = tlzw_width(i);
        const uint32_t c = tlzw_code(byte, pos + tlzw_bits_before(i) - tlzw_bits_before(ci), w, bitlen);
        const bool stop = c == TLZW_CLEAR || c == TLZW_EOI || c == TLZW_MISSING;
        const uint64_t sm = __ballot(stop);
        const int S = sm ? __builtin_ctzll(sm) : 64;
        const uint32_t bad = stop ? 0u : tlzw_check(c, i);
        const uint64_t bm = __ballot(bad != 0 && lane < S);
        const int E = bm ? __builtin_ctzll(bm) : 64;
        const int n = S < E ? S : E;  // the codes of this round: lanes 0 .. n - 1, each of them valid
        const bool active = lane < n;
        // kind, length, first byte
        int dep = LZW_LIT;
        uint32_t ln = active ? 1u : 0u, first = LZW_VALUE | (c & 0xffu), from = c & 0xffu;
        bool resolved = true;
        if (active && c >= TLZW_FIRST) {
            if (c <= 256 + ci) {  // an entry of an earlier round
                dep = LZW_OLD, ln = tab_len[c], first = from = tab_pos[c];
            } else {  // the entry of lane c - 257 - ci, which is this lane's own in the KwKwK form
                dep = (int)(c - 257 - ci) - 1;  // -1 .. lane - 1
                if (dep < 0) ln = prev_len + 1, first = prev_pos;
                else resolved = false;
            }
        }
        for (int it = 0; it < 64 && __ballot(!resolved); it++) {  // every turn resolves the lowest lane left
            const int d = dep > 0 ? dep : 0;
            const uint32_t ol = __shfl(ln, d, 64), of = __shfl(first, d, 64);
            const int ok = __shfl((int)resolved, d, 64);
            if (!resolved && ok) ln = ol + 1, first = of, resolved = true;
        }
        uint32_t incl = ln;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        const uint32_t excl = incl - ln, T = __shfl(incl, 63, 64);
        const uint32_t room = total - base;  // > 0
        const bool complete = T >= room;
        if (!complete) {
            if (E < S) {
                err = __shfl(bad, E, 64);
                break;
            }
            if (S < 64 && __shfl(c, S, 64) != TLZW_CLEAR) {  // EOI, or no room for a code, before the rows are full
                err = TLZW_ERR_INPUT;
                break;
            }
        }
        // the code in front: its place in the output and its length
        const uint32_t before_pos = __shfl_up(base + excl, 1, 64), before_len = __shfl_up(ln, 1, 64);
        const uint32_t bp = lane == 0 ? prev_pos : before_pos, bl = lane == 0 ? prev_len : before_len;
        const uint32_t dep_excl = __shfl(excl, dep > 0 ? dep : 0, 64);
        if (dep >= 0) from = base + dep_excl;
        else if (dep == -1) from = prev_pos;
        if (active && i >= 1) tab_pos[257 + i] = bp, tab_len[257 + i] = (uint16_t)(bl + 1);  // 257 + i <= 4095: tlzw_check
        r_off[lane] = active ? excl : 0xffffffffu, r_len[lane] = ln, r_src[lane] = from, r_first[lane] = first, r_dep[lane] = dep;
        __syncthreads();
        const uint32_t Tc = complete ? room : T;
        for (uint32_t t = (uint32_t)lane; t < Tc; t += 64) {
            int m = 0;
            for (int s = 32; s; s >>= 1)
                if (r_off[m + s] <= t) m += s;  // r_off[0] = 0; lanes that hold no code say 0xffffffff
            uint32_t k = t - r_off[m], at = 0, v = 0;
            bool by_value = false;
            for (int hop = 0; hop < 65; hop++) {  // every turn ends or goes to a lower lane
                const int d = r_dep[m];
                if (d == LZW_LIT) {
                    v = r_src[m], by_value = true;
                    break;
                }
                if (d == LZW_OLD) {
                    at = r_src[m] + k;
                    break;
                }
                if (k + 1 == r_len[m]) {  // the entry's last byte: the first byte of the code behind lane d
                    const uint32_t f = r_first[d + 1];
                    if (f & LZW_VALUE) v = f & 0xffu, by_value = true;
                    else at = f;
                    break;
                }
                if (d < 0) {
                    at = prev_pos + k;
                    break;
                }
                m = d;
            }
            if (!by_value) v = at < base ? out[at] : 0u;  // at < base by construction; the test keeps the read behind the round
            out[base + t] = (uint8_t)v;
        }
        if (complete) break;
        if (n > 0) prev_pos = base + __shfl(excl, n - 1, 64), prev_len = __shfl(ln, n - 1, 64);
        base += T;
        pos += tlzw_bits_before(ci + (uint32_t)n) - tlzw_bits_before(ci);
        ci += (uint32_t)n;
        if (S < 64) pos += __shfl(w, S, 64), ci = 0;  // a Clear
        __threadfence();  // the next round reads this one's bytes from other lanes
        __syncthreads();
    }
    if (lane == 0 && err) atomicOr(&dyn[st.img].err, err);
}

// per-byte a + b modulo 256
__device__ inline uint32_t add8(uint32_t a, uint32_t b) { return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u); }

constexpr int F8_PX = 4;              // pixels a thread and turn
constexpr int F8_CHUNK = 256 * F8_PX;  // pixels a block and turn

// ---- raw rows -> the output slots.  A block a row, F8_CHUNK pixels a turn: a thread loads F8_PX pixels (a pixel's samples
// packed in a word), Predictor 2 is a running sum modulo 256 per sample (in the thread, then a scan over the wave and the
// block's four waves, then the carry of the turns before), the converted bytes go through LDS, and the block stores them
// as aligned dwords along the row and bytes at the ragged ends, whatever the slot's base address and pitch.
__global__ void __launch_bounds__(256) tdec_finish8(TdecPass p)
{
    __shared__ uint32_t stage[F8_CHUNK * 3 / 4];
    __shared__ uint32_t wsum[4];
    const int i = (int)blockIdx.y, r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const TdecImg im = p.imgs[i];
    if (im.depth != 8 || r >= im.rows || p.dyn[i].err) return;
    const uint8_t *in = (im.from_src ? p.src : p.raw) + im.bits_off + (int64_t)r * im.pitch;
    uint8_t *o = p.out + im.out_off + (int64_t)r * p.step;
    const int spp = im.samples == 3 ? 3 : 1, cn = spp == 3 ? 3 : (p.channels == 3 ? 3 : 1);
    const bool pred = im.predictor == 2;
    const uint32_t inv = im.invert ? 0xffffffu : 0u;
    uint8_t *sb = (uint8_t *)stage;
    uint32_t carry = 0;
    for (int x0 = 0; x0 < im.cols; x0 += F8_CHUNK) {
        const int npx = min(F8_CHUNK, im.cols - x0);
        uint32_t v[F8_PX];
        for (int q = 0; q < F8_PX; q++) {
            const int x = F8_PX * tid + q;
            v[q] = 0;
            if (x < npx) {
                const uint8_t *s = in + (int64_t)(x0 + x) * spp;
                v[q] = spp == 3 ? (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 : (uint32_t)s[0];
            }
        }
        if (pred) {
            for (int q = 1; q < F8_PX; q++) v[q] = add8(v[q], v[q - 1]);
            uint32_t incl = v[F8_PX - 1];
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t u = __shfl_up(incl, d, 64);
                if ((tid & 63) >= d) incl = add8(incl, u);
            }
            if ((tid & 63) == 63) wsum[tid >> 6] = incl;
            uint32_t before = __shfl_up(incl, 1, 64);
            if ((tid & 63) == 0) before = 0;
            __syncthreads();
            uint32_t all = carry;
            for (int k = 0; k < 4; k++) {
                if (k == (tid >> 6)) before = add8(before, all);
                all = add8(all, wsum[k]);
            }
            carry = all;
            for (int q = 0; q < F8_PX; q++) v[q] = add8(v[q], before);
        }
        for (int q = 0; q < F8_PX; q++) {
            const int x = F8_PX * tid + q;
            if (x >= npx) continue;
            const uint32_t s = v[q] ^ inv;
            if (spp == 3) sb[3 * x] = (uint8_t)(s >> 16), sb[3 * x + 1] = (uint8_t)(s >> 8), sb[3 * x + 2] = (uint8_t)s;  // BGR
            else if (cn == 3) sb[3 * x] = sb[3 * x + 1] = sb[3 * x + 2] = (uint8_t)s;
            else sb[x] = (uint8_t)s;
        }
        __syncthreads();
        uint8_t *dst = o + (int64_t)x0 * cn;
        const uint32_t nb = (uint32_t)npx * (uint32_t)cn;
        const uint32_t lead = min(nb, (uint32_t)(-(uintptr_t)dst & 3));
        const uint32_t nd = (nb - lead) >> 2;
        for (uint32_t t = (uint32_t)tid; t < nd; t += 256) {
            const uint32_t j = lead + 4 * t;
            *(uint32_t *)(dst + j) = (uint32_t)sb[j] | (uint32_t)sb[j + 1] << 8 | (uint32_t)sb[j + 2] << 16 | (uint32_t)sb[j + 3] << 24;
        }
        if ((uint32_t)tid < lead) dst[tid] = sb[tid];
        const uint32_t tail = lead + 4 * nd + (uint32_t)tid;
        if (tail < nb) dst[tail] = sb[tail];
        __syncthreads();
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

}  // namespace

int tdec_launch_lzw(const TdecPass &p, const TdecStrip *d_strips, int nstrips, hipStream_t s)
{
    if (nstrips <= 0) return OMR_OK;
    tdec_lzw<<<(unsigned)nstrips, 64, 0, s>>>(p.src, d_strips, p.dyn, p.raw);
    return launched("tdec_lzw");
}

int tdec_launch_finish8(const TdecPass &p, int max_rows, hipStream_t s)
{
    if (p.n <= 0 || max_rows <= 0) return OMR_OK;
    tdec_finish8<<<dim3((unsigned)max_rows, (unsigned)p.n), 256, 0, s>>>(p);
    return launched("tdec_finish8");
}

}  // namespace omr
