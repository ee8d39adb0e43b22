// tiff_dec.hip -- bilevel TIFF on the device: the T.6 (CCITT Group 4) decoder, one wave per strip;
// PackBits, one lane per strip; and the unpack kernel that turns packed rows into bytes of 0 / 255 in the output slots.
//
// Bounds.  Everything a kernel loops over is fixed on the host: a strip's byte length, its rows, the image's cols.  The
// T.6 code reader consumes at least one bit per code and takes none that begins behind the strip's bit length; a line's
// change positions are strictly increasing and below cols, so a line holds at most cols of them (cols <=
// TDEC_T6_MAX_COLS, checked by the parser); the PackBits loop consumes at least one input byte a turn.  Writes go to the workspace rows of the strip
// (rows x pitch from dst_off) and, in the unpack kernel, to cols x channels bytes of rows `step` apart in the slot.
#include <hip/hip_runtime.h>

#include "../../include/omrdeskew.h"
#include "engine.hpp"
#include "tiff_dec.hpp"

namespace omr {
namespace {

__device__ inline uint32_t rev8(uint32_t b) { return __brev(b) >> 24; }

// ---- PackBits: one lane per strip.  The runs are byte-sized and a bilevel page is tens of kilobytes.
__global__ void __launch_bounds__(64) tdec_packbits(const uint8_t *__restrict__ src, const TdecStrip *__restrict__ strips, int nstrips,
                                                    TdecDyn *dyn, uint8_t *__restrict__ raw)
{
    const int k = (int)(blockIdx.x * 64 + threadIdx.x);
    if (k >= nstrips) return;
    const TdecStrip st = strips[k];
    const uint8_t *in = src + st.src_off;
    uint8_t *out = raw + st.dst_off;
    const uint32_t total = (uint32_t)st.rows * (uint32_t)st.pitch, len = st.src_len;
    const bool lsb = st.lsb != 0;
    uint32_t p = 0, o = 0, err = 0;
    while (o < total) {
        if (p >= len) {
            err = TDEC_ERR_INPUT;
            break;
        }
        uint32_t b = in[p++];
        if (lsb) b = rev8(b);
        if (b == 128) continue;
        if (b < 128) {  // b + 1 literal bytes
            const uint32_t cnt = b + 1;
            if (cnt > len - p) {
                err = TDEC_ERR_INPUT;
                break;
            }
            if (cnt > total - o) {
                err = TDEC_ERR_RUN;
                break;
            }
            for (uint32_t i = 0; i < cnt; i++) {
                const uint32_t v = in[p + i];
                out[o + i] = (uint8_t)(lsb ? rev8(v) : v);
            }
            p += cnt, o += cnt;
        } else {  // the next byte 257 - b times
            const uint32_t cnt = 257 - b;
            if (p >= len) {
                err = TDEC_ERR_INPUT;
                break;
            }
            if (cnt > total - o) {
                err = TDEC_ERR_RUN;
                break;
            }
            uint32_t v = in[p++];
            if (lsb) v = rev8(v);
            for (uint32_t i = 0; i < cnt; i++) out[o + i] = (uint8_t)v;
            o += cnt;
        }
    }
    if (err) atomicOr(&dyn[st.img].err, err);
}

// ---- T.6: one wave per strip.  Lane 0 reads the code stream and keeps a0 / b1 / b2 against the reference line's change
// positions; both lines' positions are in LDS.  The wave then turns the finished line's positions into packed words, a
// word a lane, and stores them.
struct T6Reader {
    const uint8_t *in;      // the strip in global memory
    const uint8_t *win;     // its window in LDS: bytes wbase .. wbase + TDEC_WIN_BYTES
    uint32_t len, wbase, pos;  // pos: bits consumed
    bool lsb;
    __device__ uint32_t byte(uint32_t i) const
    {
        if (i >= len) return 0;
        const uint32_t o = i - wbase;
        const uint32_t b = o < (uint32_t)TDEC_WIN_BYTES ? win[o] : in[i];
        return lsb ? rev8(b) : b;
    }
    // the next 13 bits, zeros behind the strip's end
    __device__ uint32_t peek() const
    {
        const uint32_t i = pos >> 3;
        const uint32_t v = byte(i) << 16 | byte(i + 1) << 8 | byte(i + 2);
        return (v >> (11 - (pos & 7))) & 0x1fffu;
    }
    // false: the code begins behind the strip's end.  One that begins inside it and ends behind it was matched with zeros
    // for the missing bits, as libtiff reads it: a writer may drop a last byte that held only a code's trailing zeros
    // (three at the most; no code is all zeros, so the next one finds nothing).
    __device__ bool skip(uint32_t bits)
    {
        if (pos >= len * 8) return false;
        pos += bits;
        return true;
    }
};

// one run of `colour`: make-up codes and a terminating code.  The sum stays <= limit; returns an error or 0.
__device__ uint32_t t6_run(T6Reader &rd, const uint16_t *__restrict__ lut, int colour, int limit, int *run)
{
    int total = 0;
    for (;;) {  // a code a turn, each at least two bits of a strip of rd.len bytes
        const uint32_t e = lut[(colour << TDEC_LUT_BITS) + rd.peek()];
        if (!e) return TDEC_ERR_CODE;
        if (!rd.skip(e >> 12)) return TDEC_ERR_INPUT;
        const int r = (int)(e & 0xfff);
        total += r;
        if (total > limit) return TDEC_ERR_RUN;
        if (r < 64) break;
    }
    *run = total;
    return 0;
}

// One row.  R: the reference line's nr change positions and TDEC_T6_PAD sentinels of `cols`; C receives the row's.
// A change with an even index is white -> black.  Returns an error or 0, *nc_out = the positions written.
__device__ uint32_t t6_row(T6Reader &rd, const uint16_t *__restrict__ lut, const uint16_t *R, int nr, uint16_t *C, int cols, int *nc_out)
{
    int a0 = -1, colour = 0, ri = 0, nc = 0;
    while (a0 < cols) {  // every turn moves a0 to the right or ends the row with an error
        while (ri < nr && (int)R[ri] <= a0) ri += 2;  // b1: right of a0, a change to the other colour
        const int b1 = R[ri], b2 = R[ri + 1];
        const uint32_t b = rd.peek();
        int v;  // a vertical code's a1 - b1
        if (b & 0x1000) {
            if (!rd.skip(1)) return TDEC_ERR_INPUT;
            v = 0;
        } else if ((b >> 10) == 3) {
            if (!rd.skip(3)) return TDEC_ERR_INPUT;
            v = 1;
        } else if ((b >> 10) == 2) {
            if (!rd.skip(3)) return TDEC_ERR_INPUT;
            v = -1;
        } else if ((b >> 10) == 1) {  // horizontal: a0a1 in the current colour, a1a2 in the other
            if (!rd.skip(3)) return TDEC_ERR_INPUT;
            const int s = a0 < 0 ? 0 : a0;
            int r1 = 0, r2 = 0;
            uint32_t e = t6_run(rd, lut, colour, cols - s, &r1);
            if (e) return e;
            const int a1 = s + r1;
            if ((e = t6_run(rd, lut, colour ^ 1, cols - a1, &r2))) return e;
            const int a2 = a1 + r2;
            if (a1 <= a0 || (a2 <= a1 && a1 < cols)) return TDEC_ERR_RUN;  // a run of 0 that is not the row's first or last
            if (a1 < cols) C[nc++] = (uint16_t)a1;
            if (a2 < cols) C[nc++] = (uint16_t)a2;
            a0 = a2;
            continue;
        } else if ((b >> 9) == 1) {  // pass
            if (!rd.skip(4)) return TDEC_ERR_INPUT;
            a0 = b2;
            ri += 2;
            continue;
        } else if ((b >> 7) == 3) {
            if (!rd.skip(6)) return TDEC_ERR_INPUT;
            v = 2;
        } else if ((b >> 7) == 2) {
            if (!rd.skip(6)) return TDEC_ERR_INPUT;
            v = -2;
        } else if ((b >> 6) == 3) {
            if (!rd.skip(7)) return TDEC_ERR_INPUT;
            v = 3;
        } else if ((b >> 6) == 2) {
            if (!rd.skip(7)) return TDEC_ERR_INPUT;
            v = -3;
        } else {
            return rd.pos + 7 > rd.len * 8 ? TDEC_ERR_INPUT : TDEC_ERR_CODE;  // an extension code, EOFB before the last row, zeros
        }
        const int a1 = b1 + v;
        if (a1 <= a0 || a1 > cols) return TDEC_ERR_RUN;
        if (a1 < cols) C[nc++] = (uint16_t)a1;
        a0 = a1, colour ^= 1;
        ri = ri > 0 ? ri - 1 : ri + 1;  // the change before the old b1 may lie right of the new a0 (vertical left); none further back can
    }
    *nc_out = nc;
    return 0;
}

__global__ void __launch_bounds__(64) tdec_t6(const uint8_t *__restrict__ src, const TdecStrip *__restrict__ strips,
                                              const uint16_t *__restrict__ lut, TdecDyn *dyn, uint8_t *__restrict__ raw)
{
    __shared__ uint16_t line[2][TDEC_T6_MAX_COLS + TDEC_T6_PAD];
    __shared__ uint32_t win[TDEC_WIN_BYTES / 4];
    __shared__ uint32_t s_nc, s_err, s_pos;
    const TdecStrip st = strips[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const int cols = st.cols;
    if (cols < 1 || cols > TDEC_T6_MAX_COLS) return;  // the parser's rule, kept where the buffers are
    const uint8_t *in = src + st.src_off;  // src_off is a multiple of 16
    const uint32_t len = st.src_len;
    if (lane < TDEC_T6_PAD) line[0][lane] = (uint16_t)cols;  // the imaginary white line above the strip
    if (lane == 0) s_pos = 0, s_err = 0, s_nc = 0;
    uint32_t wbase = 0;
    int cur = 1, nr = 0;
    const int words = (cols + 31) >> 5;
    for (int row = 0; row < st.rows; row++) {
        __syncthreads();
        const uint32_t pos = s_pos;
        if (row == 0 || (pos >> 3) - wbase > (uint32_t)TDEC_WIN_BYTES / 2) {  // the window follows the reader, a row at a time
            wbase = (pos >> 3) & ~3u;
            for (int i = lane; i < TDEC_WIN_BYTES / 4; i += 64) {
                const uint32_t at = wbase + 4 * (uint32_t)i;
                uint32_t w = 0;
                if (at + 4 <= len) w = *(const uint32_t *)(in + at);
                else
                    for (uint32_t k = 0; k < 4 && at + k < len; k++) w |= (uint32_t)in[at + k] << (8 * k);
                win[i] = w;
            }
            __syncthreads();
        }
        uint16_t *C = line[cur];
        const uint16_t *R = line[cur ^ 1];
        if (lane == 0) {
            T6Reader rd{in, (const uint8_t *)win, len, wbase, pos, st.lsb != 0};
            int nc = 0;
            const uint32_t e = t6_row(rd, lut, R, nr, C, cols, &nc);
            for (int k = 0; k < TDEC_T6_PAD; k++) C[nc + k] = (uint16_t)cols;
            s_nc = (uint32_t)nc, s_pos = rd.pos, s_err = e;
        }
        __syncthreads();
        if (s_err) break;
        const int nc = (int)s_nc;
        // the row as packed words, first pixel in a byte's top bit; a set bit is a pixel of a black run
        uint32_t *dst = (uint32_t *)(raw + st.dst_off + (int64_t)row * st.pitch);  // dst_off: a multiple of 16, pitch: of 4
        for (int w = lane; w < words; w += 64) {
            const int x0 = 32 * w;
            int lo = 0, hi = nc;
            while (lo < hi) {  // the changes at or left of x0
                const int mid = (lo + hi) >> 1;
                if ((int)C[mid] <= x0) lo = mid + 1;
                else hi = mid;
            }
            uint32_t bits = 0;
            int x = x0, j = lo;
            while (x < x0 + 32) {  // at most 32 turns: the positions strictly increase
                const int next = j < nc ? min((int)C[j], x0 + 32) : x0 + 32;
                if (j & 1) {
                    const int a = x - x0, e = next - x0;
                    bits |= (0xffffffffu >> a) & (e == 32 ? 0xffffffffu : ~(0xffffffffu >> e));
                }
                x = next, j++;
            }
            dst[w] = __builtin_bswap32(bits);
        }
        nr = nc, cur ^= 1;
    }
    if (lane == 0 && s_err) atomicOr(&dyn[st.img].err, s_err);
}

// ---- packed rows -> bytes of 0 / 255, `channels` of them a pixel.  A block a row: aligned dwords along the row, bytes at
// its ragged ends, whatever the slot's base address and pitch.
__global__ void __launch_bounds__(256) tdec_unpack(TdecPass p)
{
    const int i = (int)blockIdx.y, r = (int)blockIdx.x;
    const TdecImg im = p.imgs[i];
    if (im.depth != 1 || r >= im.rows || p.dyn[i].err) return;  // depth 8: tdec_finish8's (tiff_dec8.hip)
    const uint8_t *bits = (im.from_src ? p.src : p.raw) + im.bits_off + (int64_t)r * im.pitch;
    uint8_t *o = p.out + im.out_off + (int64_t)r * p.step;
    const int cn = p.channels;
    const uint32_t n = (uint32_t)im.cols * (uint32_t)cn;
    const bool lsb = im.lsb != 0;
    const uint32_t inv = im.invert ? 1u : 0u;
    auto px = [&](uint32_t j) -> uint32_t {
        const uint32_t x = cn == 3 ? j / 3 : j;
        const uint32_t b = bits[x >> 3];
        const uint32_t bit = (b >> (lsb ? (x & 7) : 7 - (x & 7))) & 1u;
        return (bit ^ inv) ? 255u : 0u;
    };
    const uint32_t lead = min(n, (uint32_t)(-(uintptr_t)o & 3));
    const uint32_t nd = (n - lead) >> 2;
    for (uint32_t t = threadIdx.x; t < nd; t += 256) {
        const uint32_t j = lead + 4 * t;
        *(uint32_t *)(o + j) = px(j) | px(j + 1) << 8 | px(j + 2) << 16 | px(j + 3) << 24;
    }
    if (threadIdx.x < lead) o[threadIdx.x] = (uint8_t)px(threadIdx.x);
    const uint32_t tail = lead + 4 * nd + threadIdx.x;
    if (tail < n) o[tail] = (uint8_t)px(tail);
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

}  // namespace

int tdec_launch_packbits(const TdecPass &p, const TdecStrip *d_strips, int nstrips, hipStream_t s)
{
    if (nstrips <= 0) return OMR_OK;
    tdec_packbits<<<(unsigned)((nstrips + 63) / 64), 64, 0, s>>>(p.src, d_strips, nstrips, p.dyn, p.raw);
    return launched("tdec_packbits");
}

int tdec_launch_t6(const TdecPass &p, const TdecStrip *d_strips, int nstrips, hipStream_t s)
{
    if (nstrips <= 0) return OMR_OK;
    tdec_t6<<<(unsigned)nstrips, 64, 0, s>>>(p.src, d_strips, p.lut, p.dyn, p.raw);
    return launched("tdec_t6");
}

int tdec_launch_unpack(const TdecPass &p, int max_rows, hipStream_t s)
{
    if (p.n <= 0 || max_rows <= 0) return OMR_OK;
    tdec_unpack<<<dim3((unsigned)max_rows, (unsigned)p.n), 256, 0, s>>>(p);
    return launched("tdec_unpack");
}

}  // namespace omr
