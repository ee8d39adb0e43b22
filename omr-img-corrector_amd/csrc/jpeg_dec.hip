// jpeg_dec.hip -- baseline JPEG decoding on the device: what libjpeg returns with its defaults
// (JDCT_ISLOW, fancy up-sampling), byte for byte.  int32 VALU throughout.  The stages:
//
//   un-stuffing   jdec_count_kernel    per 4096-byte segment: bytes that stay, RSTn markers, the first end of scan
//                 jdec_chunk_scan      per image: exclusive sums of the segments, the scan's end
//                 jdec_compact_kernel  the bit buffer (0xFF 0x00 -> 0xFF, markers dropped), every interval's first byte
//                 jdec_ival_scan       per image: every interval's first subsequence
//   Huffman       jdec_sync_kernel     one round of the self-synchronising decode: where each lane stands at its end
//                 jdec_sub_scan        per image: blocks finished and DC differences summed before each subsequence
//                 jdec_write_kernel    the decode from the known states: coefficients and DC values
//   samples       jdec_idct_kernel     de-quantisation and jidctint.c, one thread per block, into component planes
//                 jdec_color_kernel    h2v1 / h2v2 fancy up-sampling, ycc_rgb_convert, the slot's pixels
//
// Where the bounds sit.  A lane of the Huffman kernels reads bits through peek(), whose index is clamped to the words its
// workgroup staged, and it stops at min(its subsequence's end, its interval's end); a code that would run past the
// interval's end is not taken.  It writes block b of its interval only while b is below the interval's block count, which
// the header fixes.  The un-stuffing kernels write position k of an image's bit buffer only for k below its stuffed length,
// interval starts only below the header's interval count.  The sample kernels index by the header's geometry alone.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "jpeg_dec.hpp"

namespace omr {
namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kSubBytes = JDEC_SUB_BITS / 8;
constexpr int kSpanWords = JDEC_LANES * kSubBytes / 4 + 8;  // a workgroup's subsequences, the word before and the peek behind

// exclusive sum over the workgroup's 256 threads; *total = the sum
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t a = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += a;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[255];
    __syncthreads();
    return incl - v;
}

// The 16 bytes at i0 of an image's entropy data, below `lim`: bit j of *keep: byte i0 + j is data; of *rst: it is the 0xFF
// of an RSTn marker.  *first_end: the first 0xFF that ends the scan (before a marker that is neither RSTn nor a fill byte;
// the last byte of the data counts as standing before EOI), kNone without one.  Of *fill: fill 0xFFs stand before this
// 0xFF 0x00.  libjpeg's C decoder skips them and keeps the data 0xFF, libjpeg-turbo's takes a marker there and returns
// another picture; no encoder writes this, and the image is refused (jdec_count_kernel) rather than decoded either way.
__device__ inline void classify(const uint8_t *src, uint32_t len, uint32_t i0, uint32_t lim, uint32_t *keep, uint32_t *rst,
                                uint32_t *first_end, uint32_t *fill = nullptr)
{
    uint32_t k = 0, r = 0, f = 0, e = kNone;
    if (i0 < len) {
        uint32_t prev = i0 > 0 ? src[i0 - 1] : 0, cur = src[i0];
        for (int j = 0; j < 16; j++) {
            const uint32_t i = i0 + j;
            if (i >= len) break;
            const uint32_t nx = i + 1 < len ? src[i + 1] : 0xD9;
            const bool ff = cur == 0xFF, is_rst = ff && nx >= 0xD0 && nx <= 0xD7;
            if (ff && nx != 0 && nx != 0xFF && !is_rst && e == kNone) e = i;
            if (i < lim) {
                if (!(ff && nx != 0) && prev != 0xFF) k |= 1u << j;
                if (ff && prev == 0xFF && nx == 0) f |= 1u << j;
                if (is_rst) r |= 1u << j;
            }
            prev = cur, cur = nx;
        }
    }
    *keep = k, *rst = r, *first_end = e;
    if (fill) *fill = f;
}

__global__ __launch_bounds__(256) void jdec_count_kernel(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    __shared__ uint32_t s_end, s_keep, s_rst;
    if (threadIdx.x == 0) s_end = kNone, s_keep = 0, s_rst = 0;
    __syncthreads();
    const uint8_t *src = p.src + im.src_off;
    const uint32_t i0 = blockIdx.x * JDEC_BYTE_CHUNK + threadIdx.x * 16;
    uint32_t keep, rst, e, fill;
    classify(src, im.src_len, i0, kNone, &keep, &rst, &e, &fill);
    if (e != kNone) atomicMin(&s_end, e);
    __syncthreads();
    const uint32_t end = s_end;
    if (end != kNone && end < i0 + 16) {  // only what lies before the end counts
        const uint32_t m = end <= i0 ? 0 : (1u << (end - i0)) - 1;
        keep &= m, rst &= m, fill &= m;
    }
    if (fill) atomicOr(&s_rst, 0x80000000u);  // bit 31 of the segment's marker count: jdec_chunk_scan knows the scan's end
    if (keep) atomicAdd(&s_keep, (uint32_t)__popc(keep));
    if (rst) atomicAdd(&s_rst, (uint32_t)__popc(rst));
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c = im.chunk0 + blockIdx.x;
        p.chunk_keep[c] = s_keep, p.chunk_rst[c] = s_rst, p.chunk_end[c] = end;
    }
}

__global__ __launch_bounds__(256) void jdec_chunk_scan(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.x];
    if (im.nchunk == 0) return;
    __shared__ uint32_t lds[256];
    __shared__ uint32_t s_first;
    uint32_t carry_k = 0, carry_r = 0, end_pos = im.src_len;
    bool dead = false;
    for (uint32_t c0 = 0; c0 < im.nchunk; c0 += 256) {
        const uint32_t c = c0 + threadIdx.x;
        const bool in = c < im.nchunk;
        if (threadIdx.x == 0) s_first = kNone;
        __syncthreads();
        uint32_t k = in ? p.chunk_keep[im.chunk0 + c] : 0, r = in ? p.chunk_rst[im.chunk0 + c] : 0;
        const uint32_t e = in ? p.chunk_end[im.chunk0 + c] : kNone;
        if (e != kNone) atomicMin(&s_first, c);
        __syncthreads();
        const uint32_t first = s_first;
        if (dead || c > first) k = r = 0;
        if (r >> 31) p.dyn[blockIdx.x].err = 1;  // fill bytes before a stuffed 0xFF inside the scan (classify)
        r &= 0x7fffffffu;
        uint32_t tk, tr;
        const uint32_t ek = block_excl_scan(k, lds, &tk), er = block_excl_scan(r, lds, &tr);
        if (in) p.chunk_off[im.chunk0 + c] = carry_k + ek, p.chunk_rst_off[im.chunk0 + c] = carry_r + er;
        carry_k += tk, carry_r += tr;
        if (!dead && first != kNone) {
            end_pos = p.chunk_end[im.chunk0 + first];
            dead = true;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        JdecDyn &d = p.dyn[blockIdx.x];
        d.end_pos = end_pos, d.nbytes = carry_k;
        if (carry_r + 1 != im.nival) d.err = 1;  // not the intervals DRI and the MCU count predict
        p.ival_start[im.ival0] = 0;
        p.ival_start[im.ival0 + im.nival] = carry_k;
    }
}

__global__ __launch_bounds__(256) void jdec_compact_kernel(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    const JdecDyn d = p.dyn[blockIdx.y];
    __shared__ uint32_t lds[256];
    __shared__ uint32_t s_err;  // one reading for the workgroup: other workgroups of this launch may set the flag
    if (threadIdx.x == 0) s_err = d.err;
    __syncthreads();
    if (s_err) return;
    const uint8_t *src = p.src + im.src_off;
    const uint32_t i0 = blockIdx.x * JDEC_BYTE_CHUNK + threadIdx.x * 16;
    uint32_t keep, rst, e;
    classify(src, im.src_len, i0, d.end_pos, &keep, &rst, &e);
    uint32_t tk, tr;
    uint32_t pos = block_excl_scan((uint32_t)__popc(keep), lds, &tk) + p.chunk_off[im.chunk0 + blockIdx.x];
    uint32_t k = block_excl_scan((uint32_t)__popc(rst), lds, &tr) + p.chunk_rst_off[im.chunk0 + blockIdx.x];
    if (!(keep | rst)) return;
    uint8_t *dst = p.bitbuf + im.bit_off;
    for (int j = 0; j < 16; j++) {
        if (keep >> j & 1) {
            if (pos < im.src_len) dst[pos] = src[i0 + j];
            pos++;
        }
        if (rst >> j & 1) {
            k++;  // the interval this marker opens
            if (src[i0 + j + 1] != 0xD0 + ((k - 1) & 7)) p.dyn[blockIdx.y].err = 1;
            if (k < im.nival) p.ival_start[im.ival0 + k] = pos;
        }
    }
}

__global__ __launch_bounds__(256) void jdec_ival_scan(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.x];
    if (im.nchunk == 0 || p.dyn[blockIdx.x].err) return;
    __shared__ uint32_t lds[256];
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < im.nival; k0 += 256) {
        const uint32_t k = k0 + threadIdx.x;
        uint32_t ns = 0;
        if (k < im.nival) {
            const uint32_t bytes = p.ival_start[im.ival0 + k + 1] - p.ival_start[im.ival0 + k];
            ns = bytes > 0 ? (bytes + kSubBytes - 1) / kSubBytes : 1;
        }
        uint32_t total;
        const uint32_t ex = block_excl_scan(ns, lds, &total);
        if (k < im.nival) p.ival_sub0[im.ival0 + k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        p.ival_sub0[im.ival0 + im.nival] = carry;
        p.dyn[blockIdx.x].nsub = carry;
        if (carry > im.sub_cap) p.dyn[blockIdx.x].err = 1;  // cannot happen: sub_cap bounds the sum
    }
}

// ---- the Huffman lanes

struct Lane {
    uint32_t p;  // bit of the image's bit buffer where the next code starts
    int slot;    // block within the MCU
    int zz;      // zig-zag index the next code is for; 0: the DC code
};

__device__ inline uint64_t pack(const Lane &l) { return (uint64_t)l.p << 32 | (uint32_t)(l.zz << 8 | l.slot); }
__device__ inline Lane unpack(uint64_t v) { return Lane{(uint32_t)(v >> 32), (int)(v & 255), (int)(v >> 8 & 255)}; }

// what a lane of subsequence j needs to know about its place
struct Place {
    uint32_t k;        // its interval
    uint32_t first;    // the interval's first subsequence
    uint32_t start;    // the subsequence's first bit
    uint32_t lim;      // where the lane stops: the subsequence's end or the interval's
    uint32_t iend;     // the interval's last bit + 1
    bool last;         // the interval's last subsequence
};

__device__ inline Place place_of(const JdecPass &p, const JdecImg &im, uint32_t j)
{
    const uint32_t *sub0 = p.ival_sub0 + im.ival0;
    uint32_t lo = 0, hi = im.nival;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sub0[mid] <= j) lo = mid;
        else hi = mid;
    }
    Place q;
    q.k = lo, q.first = sub0[lo];
    q.iend = p.ival_start[im.ival0 + lo + 1] * 8;
    q.start = p.ival_start[im.ival0 + lo] * 8 + (j - q.first) * JDEC_SUB_BITS;
    q.lim = min(q.start + JDEC_SUB_BITS, q.iend);
    q.last = j + 1 == sub0[lo + 1];
    return q;
}

struct Span {
    const uint32_t *w;
    uint32_t wbase;  // word of the bit buffer that w[0] holds
    uint32_t nw;
};

// the next 32 bits at bit p
__device__ inline uint32_t peek(const Span &s, uint32_t p)
{
    uint32_t i = (p >> 5) - s.wbase;
    i = i > s.nw - 2 ? s.nw - 2 : i;  // (unsigned: a p before the span lands here too)
    const uint32_t hi = __builtin_bswap32(s.w[i]), lo = __builtin_bswap32(s.w[i + 1]), sh = p & 31;
    return sh ? hi << sh | lo >> (32 - sh) : hi;
}

// Stages the bit buffer from the first lane's subsequence to the last's into LDS.  Every thread calls it.
__device__ inline Span stage_span(const JdecPass &p, const JdecImg &im, uint32_t nsub, uint32_t *w, uint32_t *s_range)
{
    const uint32_t j0 = blockIdx.x * JDEC_LANES, j1 = min(j0 + JDEC_LANES, nsub) - 1;
    if (threadIdx.x == 0) s_range[0] = place_of(p, im, j0).start >> 5;
    if (threadIdx.x == 64) s_range[1] = (place_of(p, im, j1).lim + 31) >> 5;
    __syncthreads();
    Span s;
    s.w = w, s.wbase = s_range[0] > 0 ? s_range[0] - 1 : 0;
    s.nw = min(s_range[1] - s.wbase + 3, (uint32_t)kSpanWords);
    const uint32_t cap = (uint32_t)((((uint64_t)im.src_len + JDEC_PAD + 15) & ~(uint64_t)15) >> 2);  // words of the image's own
    const uint32_t *g = reinterpret_cast<const uint32_t *>(p.bitbuf + im.bit_off);
    for (uint32_t i = threadIdx.x; i < s.nw; i += JDEC_LANES) w[i] = s.wbase + i < cap ? g[s.wbase + i] : 0;
    __syncthreads();
    return s;
}

__device__ inline int extend(uint32_t v, int n) { return n == 0 || v >> (n - 1) ? (int)v : (int)v - (1 << n) + 1; }

// One lane from state l to q.lim.  cnt[0]: blocks finished, cnt[1 + c]: DC differences of component c summed.
// WRITE: block b0 + cnt[0] of the interval's nb blocks at coef, DC values from dcb[c].
template <bool WRITE>
__device__ inline bool run_lane(const JdecHuff *tabs, const Span &s, int ny, int bpm, const Place &q, Lane &l, uint32_t cnt[4],
                                int16_t *coef, uint32_t b0, uint32_t nb, const uint32_t dcb[3])
{
    bool bad = false;
    while (l.p < q.lim) {
        // the interval's blocks are done: what is left is its padding, which is not read as codes (libjpeg discards it at
        // the marker; 0-bits or mixed bits there would otherwise decode as the start of a block that does not exist)
        if (WRITE && b0 + cnt[0] >= nb) break;
        const int c =l.slot < ny ? 0 : l.slot - ny + 1;
        const JdecHuff &t = tabs[l.zz == 0 ? c : 3 + c];
        const uint32_t w = peek(s, l.p);
        int len, sym;
        bool ok = true;
        const uint32_t e = t.look[w >> 23];
        if (e) {
            len = (int)(e >> 8), sym = (int)(e & 255);
        } else {
            len = 10;
            while (len <= 16 && (int)(w >> (32 - len)) > t.maxcode[len]) len++;
            if (len <= 16) {
                sym = t.vals[((int)(w >> (32 - len)) + t.valoff[len]) & 255];
            } else {
                len = 16, sym = 0, ok = false;  // no such code: the rule for it only has to be the same in every pass
            }
        }
        const int n = sym & 15;
        const uint32_t vbits = n ? (w << len) >> (32 - n) : 0;
        uint32_t p2 = l.p + (uint32_t)len;
        int slot2 = l.slot, zz2;
        bool done = false;
        int kind = 2, idx = 0, v = 0;
        if (l.zz == 0) {
            p2 += (uint32_t)n, zz2 = 1, kind = 0, v = extend(vbits, n);
        } else if (n == 0) {
            zz2 = (sym >> 4) == 15 ? l.zz + 16 : 64;
            done = zz2 > 63;
        } else {
            const int k = l.zz + (sym >> 4);
            p2 += (uint32_t)n, zz2 = k + 1, done = k >= 63;
            if (k <= 63) kind = 1, idx = k, v = extend(vbits, n);
            else ok = false;
        }
        if (p2 > q.iend || p2 < l.p) {  // the code runs past the interval (its padding, or a cut stream): the lane stops
            l.p = q.iend;               // there; the blocks counted and the state at the end tell which it was
            break;
        }
        bad |= !ok;
        if (kind == 0) cnt[1 + c] += (uint32_t)v;
        if (WRITE) {
            const uint32_t b = b0 + cnt[0];
            if (b < nb) {
                if (kind == 0) coef[(size_t)b * 64] = (int16_t)(dcb[c] + cnt[1 + c]);
                else if (kind == 1) coef[(size_t)b * 64 + idx] = (int16_t)v;
            }
        }
        if (done) slot2 = l.slot + 1 == bpm ? 0 : l.slot + 1, zz2 = 0, cnt[0]++;
        l.p = p2, l.slot = slot2, l.zz = zz2;
    }
    return bad;
}

__device__ inline void load_tables(const JdecPass &p, uint32_t *lds_tab)
{
    const uint32_t *g = reinterpret_cast<const uint32_t *>(p.tabs + blockIdx.y);
    for (uint32_t i = threadIdx.x; i < 6 * sizeof(JdecHuff) / 4; i += JDEC_LANES) lds_tab[i] = g[i];
}

// Round 0: every lane decodes its subsequence from its first bit as if an MCU began there (true of an interval's first).
// Round r > 0: lane j starts again from state[j - 1] where that changed in round r - 1.  The rounds end when one changes
// nothing; then state[j] is what a sequential decoder has when it crosses the end of subsequence j, whatever the order in
// which the lanes ran: state[j] was computed from the state[j - 1] that stands, or lane j - 1 flagged its change.
__global__ __launch_bounds__(JDEC_LANES) void jdec_sync_kernel(JdecPass p, int round)
{
    const JdecImg im = p.imgs[blockIdx.y];
    const JdecDyn d = p.dyn[blockIdx.y];
    if (im.nchunk == 0 || d.err || blockIdx.x * JDEC_LANES >= d.nsub) return;
    __shared__ uint32_t s_w[kSpanWords];
    __shared__ uint32_t s_tab[6 * sizeof(JdecHuff) / 4];
    __shared__ uint32_t s_range[2];
    const uint32_t j = blockIdx.x * JDEC_LANES + threadIdx.x;
    const bool in = j < d.nsub;
    uint8_t *chg_now = p.chg + (size_t)(round & 1) * p.sub_total + im.sub0;
    const uint8_t *chg_prev = p.chg + (size_t)((round & 1) ^ 1) * p.sub_total + im.sub0;
    Place q{};
    bool work = false;
    if (in) {
        q = place_of(p, im, j);
        work = round == 0 || (j != q.first && chg_prev[j - 1]);
    }
    if (!__syncthreads_or(work)) {
        if (in) chg_now[j] = 0;
        return;
    }
    load_tables(p, s_tab);
    const Span s = stage_span(p, im, d.nsub, s_w, s_range);
    if (!in) return;
    if (!work) {
        chg_now[j] = 0;
        return;
    }
    Lane l{q.start, 0, 0};
    // state[j - 1] may be rewritten by another workgroup of this launch: a stale value is covered by the invariant above,
    // a torn one is not, hence single-copy-atomic 64-bit accesses
    if (round > 0) l = unpack(__atomic_load_n(&p.state[im.sub0 + j - 1], __ATOMIC_RELAXED));
    uint32_t cnt[4] = {0, 0, 0, 0};
    const int ny = im.ncomp == 3 ? im.hs * im.vs : 1;
    run_lane<false>(reinterpret_cast<const JdecHuff *>(s_tab), s, ny, im.bpm, q, l, cnt, nullptr, 0, 0, nullptr);
    const uint64_t st = pack(l);
    const bool changed = round == 0 || st != p.state[im.sub0 + j];
    // the counts belong to the entry state: a lane that found its way back to the same exit state still counted anew
    reinterpret_cast<uint4 *>(p.sub_cnt)[im.sub0 + j] = make_uint4(cnt[0], cnt[1], cnt[2], cnt[3]);
    if (changed) {
        __atomic_store_n(&p.state[im.sub0 + j], st, __ATOMIC_RELAXED);
        if (round > 0) atomicAdd(p.changed, 1u);
    }
    chg_now[j] = changed;
}

__global__ __launch_bounds__(256) void jdec_sub_scan(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.x];
    const JdecDyn d = p.dyn[blockIdx.x];
    if (im.nchunk == 0 || d.err) return;
    __shared__ uint32_t lds[256];
    uint32_t carry[4] = {0, 0, 0, 0};
    const uint4 *cnt = reinterpret_cast<const uint4 *>(p.sub_cnt) + im.sub0;
    uint4 *ex = reinterpret_cast<uint4 *>(p.sub_ex) + im.sub0;
    for (uint32_t j0 = 0; j0 < d.nsub; j0 += 256) {
        const uint32_t j = j0 + threadIdx.x;
        const uint4 v = j < d.nsub ? cnt[j] : make_uint4(0, 0, 0, 0);
        uint32_t t0, t1, t2, t3;
        const uint32_t e0 = block_excl_scan(v.x, lds, &t0), e1 = block_excl_scan(v.y, lds, &t1);
        const uint32_t e2 = block_excl_scan(v.z, lds, &t2), e3 = block_excl_scan(v.w, lds, &t3);
        if (j < d.nsub) ex[j] = make_uint4(carry[0] + e0, carry[1] + e1, carry[2] + e2, carry[3] + e3);
        carry[0] += t0, carry[1] += t1, carry[2] += t2, carry[3] += t3;
    }
}

__global__ __launch_bounds__(JDEC_LANES) void jdec_write_kernel(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.y];
    const JdecDyn d = p.dyn[blockIdx.y];
    if (im.nchunk == 0 || blockIdx.x * JDEC_LANES >= d.nsub) return;
    __shared__ uint32_t s_w[kSpanWords];
    __shared__ uint32_t s_tab[6 * sizeof(JdecHuff) / 4];
    __shared__ uint32_t s_range[2];
    __shared__ uint32_t s_err;  // one reading for the workgroup: other workgroups of this launch may set the flag
    if (threadIdx.x == 0) s_err = d.err;
    __syncthreads();
    if (s_err) return;
    const uint32_t j = blockIdx.x * JDEC_LANES + threadIdx.x;
    load_tables(p, s_tab);
    const Span s = stage_span(p, im, d.nsub, s_w, s_range);
    if (j >= d.nsub) return;
    const Place q = place_of(p, im, j);
    Lane l{q.start, 0, 0};
    if (j != q.first) l = unpack(p.state[im.sub0 + j - 1]);
    const uint4 *ex = reinterpret_cast<const uint4 *>(p.sub_ex) + im.sub0;
    const uint4 a = ex[j], f = ex[q.first];
    const uint32_t dcb[3] = {a.y - f.y, a.z - f.z, a.w - f.w};
    const uint32_t b0 = a.x - f.x;
    const uint32_t mcus = im.ri ? min((uint32_t)im.ri, im.nmcu - q.k * (uint32_t)im.ri) : im.nmcu;
    const uint32_t nb = mcus * (uint32_t)im.bpm;
    int16_t *coef = p.coef + ((size_t)im.blk0 + (size_t)q.k * (uint32_t)im.ri * (uint32_t)im.bpm) * 64;
    uint32_t cnt[4] = {0, 0, 0, 0};
    const int ny = im.ncomp == 3 ? im.hs * im.vs : 1;
    bool bad = run_lane<true>(reinterpret_cast<const JdecHuff *>(s_tab), s, ny, im.bpm, q, l, cnt, coef, b0, nb, dcb);
    // the interval must end between two MCUs with all its blocks and no more: behind the last block less than a byte of
    // padding, whatever its bits
    if (q.last && (b0 + cnt[0] != nb || l.slot != 0 || l.zz != 0 || q.iend - l.p >= 8)) bad = true;
    if (bad) p.dyn[blockIdx.y].err = 1;
}

// ---- samples

// jpeg_natural_order
__device__ constexpr int kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// one pass of jidctint.c over d[0], d[stride], ..: CONST_BITS 13.  The arithmetic is unsigned (two's complement wraps
// to the same bits wherever int does not overflow, and a damaged stream's coefficients may make it overflow); only the
// final shifts are signed.
template <int SHIFT>
__device__ inline void idct8(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7)
{
    typedef uint32_t U;
    const U a0 = (U)d0, a2 = (U)d2, a4 = (U)d4, a6 = (U)d6;
    U z1 = (a2 + a6) * 4433u;
    const U t2 = z1 - a6 * 15137u, t3 = z1 + a2 * 6270u;
    const U t0 = (a0 + a4) << 13, t1 = (a0 - a4) << 13;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    U u0 = (U)d7, u1 = (U)d5, u2 = (U)d3, u3 = (U)d1;
    z1 = u0 + u3;
    U z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3;
    const U z5 = (z3 + z4) * 9633u;
    u0 *= 2446u, u1 *= 16819u, u2 *= 25172u, u3 *= 12299u;
    z1 *= (U)-7373, z2 *= (U)-20995, z3 = z3 * (U)-16069 + z5, z4 = z4 * (U)-3196 + z5;
    u0 += z1 + z3, u1 += z2 + z4, u2 += z2 + z3, u3 += z1 + z4;
    constexpr U R = 1u << (SHIFT - 1);
    d0 = (int)(t10 + u3 + R) >> SHIFT, d7 = (int)(t10 - u3 + R) >> SHIFT;
    d1 = (int)(t11 + u2 + R) >> SHIFT, d6 = (int)(t11 - u2 + R) >> SHIFT;
    d2 = (int)(t12 + u1 + R) >> SHIFT, d5 = (int)(t12 - u1 + R) >> SHIFT;
    d3 = (int)(t13 + u0 + R) >> SHIFT, d4 = (int)(t13 - u0 + R) >> SHIFT;
}

// One thread per block: coefficient x table entry, columns then rows, + 128, saturated (libjpeg's C code masks into its
// range-limit table there; the two agree on what an encoder writes).
__global__ __launch_bounds__(128) void jdec_idct_kernel(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.y];
    const uint32_t b = blockIdx.x * 128 + threadIdx.x;
    if (im.nchunk == 0 || b >= im.nblk || p.dyn[blockIdx.y].err) return;
    const int ny = im.ncomp == 3 ? im.hs * im.vs : 1;
    const uint32_t m = b / (uint32_t)im.bpm;
    const int slot = (int)(b - m * (uint32_t)im.bpm);
    const int c = slot < ny ? 0 : slot - ny + 1;
    if (c > 0 && p.channels == 1) return;
    const int mx = (int)(m % (uint32_t)im.mw), my = (int)(m / (uint32_t)im.mw);
    int bx = mx, by = my, pitch = im.cpitch;
    if (c == 0) {
        const int hs = im.ncomp == 3 ? im.hs : 1, vs = im.ncomp == 3 ? im.vs : 1;
        bx = mx * hs + slot % hs, by = my * vs + slot / hs, pitch = im.ypitch;
    }
    const uint4 *src = reinterpret_cast<const uint4 *>(p.coef + ((size_t)im.blk0 + b) * 64);
    const uint16_t *qt = p.tabs[blockIdx.y].quant[c];
    int v[64];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint4 x = src[i];
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int cf = (int16_t)(w[k >> 1] >> (16 * (k & 1)));
            v[kNatural[i * 8 + k]] = cf * (int)qt[i * 8 + k];
        }
    }
#pragma unroll
    for (int x = 0; x < 8; x++) idct8<11>(v[x], v[8 + x], v[16 + x], v[24 + x], v[32 + x], v[40 + x], v[48 + x], v[56 + x]);
    uint8_t *dst = p.planes + im.plane_off[c] + (size_t)(by * 8) * pitch + bx * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {
        idct8<18>(v[8 * y], v[8 * y + 1], v[8 * y + 2], v[8 * y + 3], v[8 * y + 4], v[8 * y + 5], v[8 * y + 6], v[8 * y + 7]);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 4; x++) {
            lo |= (uint32_t)min(max(v[8 * y + x] + 128, 0), 255) << (8 * x);
            hi |= (uint32_t)min(max(v[8 * y + 4 + x] + 128, 0), 255) << (8 * x);
        }
        *reinterpret_cast<uint2 *>(dst + (size_t)y * pitch) = make_uint2(lo, hi);
    }
}

// the chroma sample of pixel (x, y): jdsample.c's h2v1_fancy_upsample / h2v2_fancy_upsample over the cw x ch real samples
// (plain doubling when cw <= 2, jinit_upsampler's rule), or the sample itself at 4:4:4
__device__ inline int chroma_at(const uint8_t *pl, int pitch, int hs, int vs, int cw, int ch, int x, int y)
{
    if (hs == 1) return pl[(size_t)y * pitch + x];
    const int ci = x >> 1;
    if (vs == 1) {
        const uint8_t *r = pl + (size_t)y * pitch;
        const int t = r[ci];
        if (cw <= 2) return t;
        if (x & 1) return ci == cw - 1 ? t : (3 * t + r[ci + 1] + 2) >> 2;
        return ci == 0 ? t : (3 * t + r[ci - 1] + 1) >> 2;
    }
    const int cj = y >> 1;
    const uint8_t *near = pl + (size_t)cj * pitch;
    if (cw <= 2) return near[ci];
    const int fj = (y & 1) ? min(cj + 1, ch - 1) : max(cj - 1, 0);  // beyond the first / last real row: the row itself
    const uint8_t *far = pl + (size_t)fj * pitch;
    const int t = 3 * near[ci] + far[ci];
    if (x & 1) return ci == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[ci + 1] + far[ci + 1] + 7) >> 4;
    return ci == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[ci - 1] + far[ci - 1] + 8) >> 4;
}

// One thread per four pixels of a row.  Only the image's own rows x cols pixels of the slot are written.
__global__ __launch_bounds__(256) void jdec_color_kernel(JdecPass p)
{
    const JdecImg im = p.imgs[blockIdx.z];
    const int x0 = (int)(blockIdx.x * 64 + threadIdx.x) * 4, y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (im.nchunk == 0 || y >= im.rows || x0 >= im.cols || p.dyn[blockIdx.z].err) return;
    const int cn = p.channels, nx = min(4, im.cols - x0);
    const uint8_t *yp = p.planes + im.plane_off[0] + (size_t)y * im.ypitch;
    uint8_t px[12];
    if (cn == 3 && im.ncomp == 3) {
        const int cw = (im.cols + im.hs - 1) / im.hs, ch = (im.rows + im.vs - 1) / im.vs;
        const uint8_t *cbp = p.planes + im.plane_off[1], *crp = p.planes + im.plane_off[2];
        for (int i = 0; i < nx; i++) {
            const int yy = yp[x0 + i];
            const int cb = chroma_at(cbp, im.cpitch, im.hs, im.vs, cw, ch, x0 + i, y) - 128;
            const int cr = chroma_at(crp, im.cpitch, im.hs, im.vs, cw, ch, x0 + i, y) - 128;
            const int r = yy + ((91881 * cr + 32768) >> 16);
            const int g = yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
            const int b = yy + ((116130 * cb + 32768) >> 16);
            px[3 * i] = (uint8_t)min(max(b, 0), 255), px[3 * i + 1] = (uint8_t)min(max(g, 0), 255);
            px[3 * i + 2] = (uint8_t)min(max(r, 0), 255);
        }
    } else {
        for (int i = 0; i < nx; i++)
            for (int k = 0; k < cn; k++) px[cn * i + k] = yp[x0 + i];
    }
    uint8_t *dst = p.out + im.out_off + (size_t)y * p.step + (size_t)x0 * cn;
    const int nbytes = nx * cn;
    if (nx == 4 && ((uintptr_t)dst & 3) == 0) {
        for (int k = 0; k < cn; k++)
            reinterpret_cast<uint32_t *>(dst)[k] =
                px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
    } else {
        for (int k = 0; k < nbytes; k++) dst[k] = px[k];
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

}  // namespace

int jdec_launch_unstuff(const JdecPass &p, int max_chunks, hipStream_t s)
{
    const dim3 grid((unsigned)max_chunks, (unsigned)p.n);
    jdec_count_kernel<<<grid, 256, 0, s>>>(p);
    if (int rc = launched("jdec_count_kernel")) return rc;
    jdec_chunk_scan<<<(unsigned)p.n, 256, 0, s>>>(p);
    if (int rc = launched("jdec_chunk_scan")) return rc;
    jdec_compact_kernel<<<grid, 256, 0, s>>>(p);
    if (int rc = launched("jdec_compact_kernel")) return rc;
    jdec_ival_scan<<<(unsigned)p.n, 256, 0, s>>>(p);
    return launched("jdec_ival_scan");
}

int jdec_launch_sync(const JdecPass &p, int round, int max_groups, hipStream_t s)
{
    jdec_sync_kernel<<<dim3((unsigned)max_groups, (unsigned)p.n), JDEC_LANES, 0, s>>>(p, round);
    return launched("jdec_sync_kernel");
}

int jdec_launch_finish(const JdecPass &p, int max_groups, uint32_t max_blocks, int max_rows, int max_cols, hipStream_t s,
                       hipEvent_t *marks)
{
    jdec_sub_scan<<<(unsigned)p.n, 256, 0, s>>>(p);
    if (int rc = launched("jdec_sub_scan")) return rc;
    jdec_write_kernel<<<dim3((unsigned)max_groups, (unsigned)p.n), JDEC_LANES, 0, s>>>(p);
    if (int rc = launched("jdec_write_kernel")) return rc;
    if (marks) OMR_HIP(hipEventRecord(marks[0], s));
    jdec_idct_kernel<<<dim3((max_blocks + 127) / 128, (unsigned)p.n), 128, 0, s>>>(p);
    if (int rc = launched("jdec_idct_kernel")) return rc;
    if (marks) OMR_HIP(hipEventRecord(marks[1], s));
    const dim3 grid((unsigned)(max_cols + 255) / 256, (unsigned)(max_rows + 3) / 4, (unsigned)p.n);
    jdec_color_kernel<<<grid, dim3(64, 4), 0, s>>>(p);
    return launched("jdec_color_kernel");
}

}  // namespace omr
