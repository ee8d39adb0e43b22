// tiff_enc.hip -- CCITT Group 4 (T.6) TIFF encoding on the device: a batch of device-resident gray
// or BGR images -> one bilevel TIFF file each, its strips byte for byte what libtiff writes for the thresholded picture.
// Wave64 kernels for gfx950, a launch per stage, no workgroup waits on another and no atomics:
//   pack    tenc_pack_kernel       a thread per eight pixels: threshold (BGR: bgr.hpp's gray), one byte of the packed rows
//   rows    tenc_rows_kernel       a lane per row codes it against the row above (the first of a strip: a white line) into
//                                  the row's own segment of the workspace, and leaves the code's bit length
//   place   tenc_rowscan_kernel    a wave per strip: the rows' bit offsets in the strip, the strip's bytes
//           tenc_stripscan_kernel  a wave per image: the strips' offsets (even), the length of the data
//   merge   tenc_head_kernel       header, IFD, resolutions, StripOffsets and StripByteCounts, in bytes
//           tenc_merge_kernel      a thread per two bytes of the strips gathers them from the rows' segments and the EOFB
// The merge gathers (every output byte is computed by one thread from the rows that cover it), so nothing is cleared
// beforehand and nothing is written at or behind a file's end.
#include <hip/hip_runtime.h>

#include "bgr.hpp"
#include "engine.hpp"
#include "row_bytes.hpp"
#include "tiff_enc.hpp"

namespace omr {
namespace {

// ---- pack.
// Packed row y of an image (y = 0: a line of zeros, the white line above a strip; y >= 1: image row y - 1) is pack_w dwords;
// thread idx writes its byte idx % (4 pack_w).  Bounds: y <= rows, so the source row y - 1 < rows; pixels x0 .. x0 + npx - 1
// < cols; the byte written has an index below (rows + 1) x 4 pack_w, the image's share of the workspace.
__global__ __launch_bounds__(256) void tenc_pack_kernel(TencPass p)
{
    const TencImg &im = p.imgs[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cbw = 4 * im.pack_w;
    if (idx >= ((int64_t)im.rows + 1) * cbw) return;
    const int y = (int)(idx / cbw), j = (int)(idx % cbw);
    const int x0 = 8 * j;
    const int npx = y == 0 ? 0 : min(max(im.cols - x0, 0), 8);
    uint32_t bits = 0;
    if (npx > 0) {
        const uint8_t *row = p.src + im.src_off + (int64_t)(y - 1) * p.step;
        if (p.cn == 1) {
            uint32_t v[2];
            load_segment<2>(row, im.cols, x0, npx, v);
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (i < npx && byte_of<2>(v, i) <= p.lim) bits |= 0x80u >> i;
        } else {
            uint32_t v[6];
            load_segment<6>(row, im.cols * 3, x0 * 3, npx * 3, v);
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (i < npx && bgr_black(byte_of<6>(v, 3 * i), byte_of<6>(v, 3 * i + 1), byte_of<6>(v, 3 * i + 2), p.lim)) bits |= 0x80u >> i;
        }
    }
    // the row's first pixel is the most significant bit of its first dword
    uint8_t *dst = (uint8_t *)(p.pack + im.pack_off + (int64_t)y * im.pack_w);
    dst[j ^ 3] = (uint8_t)bits;
}

// ---- rows.
__device__ __forceinline__ uint32_t pixel(const uint32_t *row, int x) { return (row[x >> 5] >> (31 - (x & 31))) & 1u; }

// the first position >= s whose pixel differs from c, or n.  nw = ceil(n / 32) dwords are read at most; the bits of the last
// dword behind n are zeros.
__device__ __forceinline__ int find_other(const uint32_t *row, int s, uint32_t c, int n, int nw)
{
    if (s >= n) return n;
    const uint32_t flip = c ? ~0u : 0u;
    int w = s >> 5;
    uint32_t x = (row[w] ^ flip) & (~0u >> (s & 31));
    while (!x && ++w < nw) x = row[w] ^ flip;
    if (!x) return n;
    return min(32 * w + __clz(x), n);
}

// a row's code: bits collected in a register, whole dwords to the segment (never at or behind seg_w - 1: the last dword of
// a segment belongs to the merge's look-ahead)
struct BitOut {
    uint32_t *seg;
    int limit;
    int at = 0;
    uint64_t acc = 0;
    int nb = 0;
    uint32_t total = 0;
    __device__ __forceinline__ void put(uint32_t code, int len)
    {
        acc = (acc << len) | code, nb += len, total += (uint32_t)len;
        if (nb >= 32) {
            if (at < limit) seg[at] = (uint32_t)(acc >> (nb - 32));
            at++, nb -= 32;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (nb && at < limit) seg[at] = (uint32_t)(acc << (32 - nb));
    }
};

// the codes of one run: 2560s while it is 2624 or more, one make-up code, one terminating code
__device__ __forceinline__ void put_span(BitOut &o, const uint32_t *tab, int k, int steps)
{
    for (int i = 0; i < steps && k >= 2624; i++) {
        o.put(tab[63 + 40] & 0xffffu, (int)(tab[63 + 40] >> 16));
        k -= 2560;
    }
    if (k >= 64) {
        const uint32_t m = tab[63 + (k >> 6)];
        o.put(m & 0xffffu, (int)(m >> 16));
        k &= 63;
    }
    o.put(tab[k] & 0xffffu, (int)(tab[k] >> 16));
}

// A lane per row.  The rule is libtiff's Fax3Encode2DRow (restated in tests/tiff_enc_ref.py); b1 and b2 are remembered while
// they stay what a fresh search would give: b1 = B(a0, c) -- the end of the reference's first run of colour c that reaches
// a0 or begins behind it -- is the same for every a0' in [a0, b1) of the same colour, and b2 depends on b1 alone.
// Bounds: row < rows; bp and rp are packed rows 1 + row and (1 + row - 1 or 0) of the image, pack_w dwords each; every
// search reads dwords below ceil(cols / 32); the segment written is row's own, seg_w dwords, BitOut keeps inside it.
__global__ __launch_bounds__(256) void tenc_rows_kernel(TencPass p)
{
    const TencImg &im = p.imgs[blockIdx.y];
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= im.rows) return;
    const int n = im.cols, nw = (n + 31) >> 5;
    const uint32_t *base = p.pack + im.pack_off;
    const uint32_t *bp = base + (int64_t)(row + 1) * im.pack_w;
    const uint32_t *rp = row % im.rps == 0 ? base : bp - im.pack_w;
    const uint32_t *white = p.codes, *black = p.codes + TENC_CODES;
    BitOut o;
    o.seg = p.code + im.code_off + (int64_t)row * im.seg_w, o.limit = im.seg_w - 1;
    int a0 = 0;
    int a1 = pixel(bp, 0) ? 0 : find_other(bp, 0, 0, n, nw);
    int b1 = pixel(rp, 0) ? 0 : find_other(rp, 0, 0, n, nw);
    int lo0 = n, hi0 = 0, lo1 = n, hi1 = 0;  // b1 = hi<c> for a0 in [lo<c>, hi<c>)
    int b2_of = -1, b2 = 0;
    for (int step = 0; step < p.row_steps; step++) {
        if (b1 != b2_of) b2_of = b1, b2 = b1 < n ? find_other(rp, b1, pixel(rp, b1), n, nw) : n;
        if (b2 >= a1) {
            const int d = b1 - a1;
            if (d < -3 || d > 3) {  // horizontal
                const int a2 = a1 < n ? find_other(bp, a1, pixel(bp, a1), n, nw) : n;
                o.put(1, 3);
                const bool white_first = a0 + a1 == 0 || pixel(bp, a0) == 0;
                put_span(o, white_first ? white : black, a1 - a0, p.span_steps);
                put_span(o, white_first ? black : white, a2 - a1, p.span_steps);
                a0 = a2;
            } else {  // vertical: a1 - b1 = -d
                const int ad = d < 0 ? -d : d;
                o.put(d == 0 ? 1u : d < 0 ? 3u : 2u, ad == 0 ? 1 : ad == 1 ? 3 : ad + 4);
                a0 = a1;
            }
        } else {  // pass
            o.put(1, 4);
            a0 = b2;
        }
        if (a0 >= n) break;
        const uint32_t c = pixel(bp, a0);
        a1 = find_other(bp, a0, c, n, nw);
        const int lo = c ? lo1 : lo0, hi = c ? hi1 : hi0;
        if (a0 >= lo && a0 < hi) {
            b1 = hi;
        } else {
            b1 = find_other(rp, a0, 1u - c, n, nw);
            b1 = find_other(rp, b1, c, n, nw);
            if (c) lo1 = a0, hi1 = b1;
            else lo0 = a0, hi0 = b1;
        }
    }
    o.flush();
    p.len[im.row0 + row] = o.total;
}

// ---- place.
// exclusive sums through a wave, every lane active; *total: the sum of all
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t *total)
{
    const int lane = threadIdx.x & 63;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    *total = __shfl(x, 63);
    return x - v;
}

// A wave per strip; lane l takes rows [l x chunk, (l + 1) x chunk) of it, chunk = ceil(max rows of a strip / 64).
// Bounds: k < ns; r < rows of the strip, so row0 + k x rps + r is a row of the image.
__global__ __launch_bounds__(256) void tenc_rowscan_kernel(TencPass p, int chunk)
{
    const TencImg &im = p.imgs[blockIdx.y];
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= im.ns) return;  // the whole wave
    const int R = min(im.rps, im.rows - k * im.rps);
    const int64_t first = im.row0 + (int64_t)k * im.rps;
    const int r0 = min(lane * chunk, R), r1 = min(r0 + chunk, R);
    uint32_t sum = 0;
    for (int r = r0; r < r1; r++) sum += p.len[first + r];
    uint32_t total;
    uint32_t at = wave_exclusive(sum, &total);
    for (int r = r0; r < r1; r++) {
        p.off[first + r] = at;
        at += p.len[first + r];
    }
    if (lane == 0) p.sbytes[im.strip0 + k] = (total + TENC_EOFB_BITS + 7) >> 3;
}

// A wave per image; every strip starts at an even offset.
__global__ __launch_bounds__(64) void tenc_stripscan_kernel(TencPass p, int chunk)
{
    const TencImg &im = p.imgs[blockIdx.x];
    const int lane = threadIdx.x;
    const int k0 = min(lane * chunk, im.ns), k1 = min(k0 + chunk, im.ns);
    uint32_t sum = 0;
    for (int k = k0; k < k1; k++) sum += (p.sbytes[im.strip0 + k] + 1) & ~1u;
    uint32_t total;
    uint32_t at = wave_exclusive(sum, &total);
    for (int k = k0; k < k1; k++) {
        p.soff[im.strip0 + k] = at;
        at += (p.sbytes[im.strip0 + k] + 1) & ~1u;
    }
    if (lane == 0) {
        TencDyn d;
        d.data_len = im.ns ? total - (p.sbytes[im.strip0 + im.ns - 1] & 1u) : 0, d.pad = 0;  // nothing behind the last strip
        p.dyn[blockIdx.x] = d;
    }
}

// ---- merge.
__device__ __forceinline__ void put_le32(uint8_t *d, uint32_t v)
{
    d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8), d[2] = (uint8_t)(v >> 16), d[3] = (uint8_t)(v >> 24);
}

// A workgroup per image.  Bounds: b < head_len <= data_at; the arrays' values stand at off_pos + 4 k and cnt_pos + 4 k,
// k < ns, inside the entry (ns = 1) or between the IFD and data_at, so everything lies in front of the first strip.
__global__ __launch_bounds__(256) void tenc_head_kernel(TencPass p, int strip_iters)
{
    const TencImg &im = p.imgs[blockIdx.x];
    if (im.rows == 0) return;
    uint8_t *out = p.out + im.out_off;
    for (int b = threadIdx.x; b < im.head_len; b += 256) {
        const bool value = im.ns == 1 && ((b >= im.off_pos && b < im.off_pos + 4) || (b >= im.cnt_pos && b < im.cnt_pos + 4));
        if (!value) out[b] = im.head[b];
    }
    for (int it = 0; it < strip_iters; it++) {
        const int k = it * 256 + threadIdx.x;
        if (k >= im.ns) break;
        put_le32(out + im.off_pos + 4 * (int64_t)k, (uint32_t)im.data_at + p.soff[im.strip0 + k]);
        put_le32(out + im.cnt_pos + 4 * (int64_t)k, p.sbytes[im.strip0 + k]);
    }
}

// A thread per two bytes of an image's strip data (strips start at even offsets, so both belong to one strip, the second
// possibly its pad byte): which strip, which row holds the first bit, then up to 16 rows' bits and the EOFB's two ones.
// Bounds: B < data_len; k < ns; r < R rows of strip k; a segment is read at dwords j and j + 1 with j + 1 < seg_w; the bytes
// written are data_at + B and, where it lies in front of the file's end, data_at + B + 1.
__global__ __launch_bounds__(256) void tenc_merge_kernel(TencPass p)
{
    const TencImg &im = p.imgs[blockIdx.y];
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (im.rows == 0 || 2 * u >= (int64_t)p.dyn[blockIdx.y].data_len) return;
    const uint32_t B = (uint32_t)(2 * u);
    const uint32_t *soff = p.soff + im.strip0;
    int k = 0, khi = im.ns - 1;
    for (int it = 0; it < p.lg_strips && k < khi; it++) {
        const int mid = (k + khi + 1) >> 1;
        if (soff[mid] <= B) k = mid;
        else khi = mid - 1;
    }
    const uint32_t b = B - soff[k], nbytes = p.sbytes[im.strip0 + k];
    const int R = min(im.rps, im.rows - k * im.rps);
    const uint32_t *off = p.off + im.row0 + (int64_t)k * im.rps, *len = p.len + im.row0 + (int64_t)k * im.rps;
    const uint32_t *seg0 = p.code + im.code_off + (int64_t)k * im.rps * im.seg_w;
    const uint32_t T = off[R - 1] + len[R - 1];  // the rows' bits; the EOFB follows
    const uint32_t P = 8 * b;
    uint32_t val = 0;
    if (P < T) {
        int r = 0, rhi = R - 1;
        for (int it = 0; it < p.lg_rows && r < rhi; it++) {
            const int mid = (r + rhi + 1) >> 1;
            if (off[mid] <= P) r = mid;
            else rhi = mid - 1;
        }
        int filled = 0;
        for (int it = 0; it < 16 && filled < 16 && r < R; it++, r++) {
            const uint32_t L = len[r], o = P + filled - off[r];
            if (o >= L) continue;  // (an empty row: no code is empty, so never)
            const int take = min(16 - filled, (int)(L - o));
            const uint32_t j = o >> 5;
            uint32_t bits = 0;
            if (j + 1 < (uint32_t)im.seg_w) {
                const uint32_t *seg = seg0 + (int64_t)r * im.seg_w;
                const uint64_t x = ((uint64_t)seg[j] << 32) | seg[j + 1];
                bits = (uint32_t)(x >> (64 - (o & 31) - take)) & ((1u << take) - 1);
            }
            val |= bits << (16 - filled - take);
            filled += take;
        }
    }
    const uint32_t e1 = T + 11, e2 = T + 23;  // 000000000001 twice
    if (e1 >= P && e1 < P + 16) val |= 0x8000u >> (e1 - P);
    if (e2 >= P && e2 < P + 16) val |= 0x8000u >> (e2 - P);
    uint8_t *dst = p.out + im.out_off + im.data_at + B;
    const bool second = b + 1 < nbytes || k + 1 < im.ns;  // the strip's next byte, or the pad in front of the next strip
    if (second && (((uintptr_t)dst) & 1) == 0) {
        *(uint16_t *)dst = (uint16_t)((val >> 8) | (val << 8));
    } else {
        dst[0] = (uint8_t)(val >> 8);
        if (second) dst[1] = (uint8_t)val;
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

unsigned up_div(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

int tenc_launch_pack(const TencPass &p, int64_t max_pack_bytes, hipStream_t s)
{
    tenc_pack_kernel<<<dim3(up_div(max_pack_bytes, 256), (unsigned)p.n), 256, 0, s>>>(p);
    return launched("tenc_pack_kernel");
}

int tenc_launch_rows(const TencPass &p, int max_rows, hipStream_t s)
{
    tenc_rows_kernel<<<dim3(up_div(max_rows, 256), (unsigned)p.n), 256, 0, s>>>(p);
    return launched("tenc_rows_kernel");
}

int tenc_launch_place(const TencPass &p, int max_strips, int max_rps, hipStream_t s)
{
    tenc_rowscan_kernel<<<dim3(up_div(max_strips, 4), (unsigned)p.n), 256, 0, s>>>(p, (max_rps + 63) / 64);
    if (int rc = launched("tenc_rowscan_kernel")) return rc;
    return tenc_launch_stripscan(p, max_strips, s);
}

int tenc_launch_stripscan(const TencPass &p, int max_strips, hipStream_t s)
{
    tenc_stripscan_kernel<<<(unsigned)p.n, 64, 0, s>>>(p, (max_strips + 63) / 64);
    return launched("tenc_stripscan_kernel");
}

int tenc_launch_head(const TencPass &p, int max_strips, hipStream_t s)
{
    tenc_head_kernel<<<(unsigned)p.n, 256, 0, s>>>(p, (max_strips + 255) / 256);
    return launched("tenc_head_kernel");
}

int tenc_launch_merge(const TencPass &p, int64_t max_data_len, int max_strips, hipStream_t s)
{
    if (int rc = tenc_launch_head(p, max_strips, s)) return rc;
    if (max_data_len <= 0) return OMR_OK;
    tenc_merge_kernel<<<dim3(up_div((max_data_len + 1) / 2, 256), (unsigned)p.n), 256, 0, s>>>(p);
    return launched("tenc_merge_kernel");
}

}  // namespace omr
