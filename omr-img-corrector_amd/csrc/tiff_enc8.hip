// tiff_enc8.hip -- 8-bit gray and RGB TIFF encoding on the device, uncompressed and LZW: a batch of
// device-resident gray or BGR images -> one TIFF file each that decodes to the image exactly.  The LZW stream obeys
// tiff_lzw.hpp / tiff_lzw_enc.hpp and is restated in tests/tiff8_enc_ref.py, byte for byte.
// Wave64 kernels for gfx950, a launch per stage, no workgroup waits on another and no global atomics:
//   stage   tenc8_stage_kernel     a thread per four pixels of a row: BGR -> RGB, Predictor 2's differences, into the
//                                  strip's contiguous raw bytes (Compression 1: where they stand in the file)
//   LZW     tenc8_lzw_kernel       a wave per strip, the dictionary a hash table in LDS: lane 0 finds up to 64 codes, the
//                                  64 lanes place them (a code's bit position is closed-form in its index since Clear)
//           tenc8_rawlens_kernel   Compression 1 instead: the strips' lengths
//   place   tenc_stripscan_kernel  (tiff_enc.hip) the strips' offsets, the length of the data
//   merge   tenc_head_kernel       (tiff_enc.hip) header, IFD, StripOffsets and StripByteCounts
//           tenc8_copy_kernel      the coded segments to their places in the file, a zero behind an odd strip
// Nothing is written at or behind a file's end.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "row_bytes.hpp"
#include "tiff_enc8.hpp"
#include "tiff_lzw_enc.hpp"

namespace omr {
namespace {

__device__ __forceinline__ int strip_rows(const TencImg &im, int k) { return min(im.rps, im.rows - k * im.rps); }

// ---- stage.
// Pixels x0 .. x0 + npx - 1 of row y and, for the predictor, the pixel on their left.  Bounds: y < rows and x0 + npx <= cols,
// so load_segment reads inside the row; the bytes written are (y % rps) x cols x CN + x0 x CN .. + npx x CN - 1 of strip
// y / rps, below the strip's rows x cols x CN raw bytes, and the pad is the byte behind them.
template <int CN>
__device__ __forceinline__ void stage_unit(const uint8_t *row, int cols, int x0, int npx, bool pred, uint8_t *dst)
{
    constexpr int NW = CN == 1 ? 2 : 4;
    const int xs = x0 > 0 ? x0 - 1 : 0, sh = x0 - xs;
    uint32_t v[NW];
    load_segment<NW>(row, cols * CN, xs * CN, (x0 + npx - xs) * CN, v);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i >= npx) break;
#pragma unroll
        for (int c = 0; c < CN; c++) {
            const int sc = CN == 3 ? 2 - c : 0;  // B G R in memory, R G B in the file
            uint32_t cur = byte_of<NW>(v, (i + sh) * CN + sc);
            if (pred && x0 + i > 0) cur = (cur - byte_of<NW>(v, (i + sh - 1) * CN + sc)) & 255u;
            dst[(x0 + i) * CN + c] = (uint8_t)cur;
        }
    }
}

__global__ __launch_bounds__(256) void tenc8_stage_kernel(Tenc8Pass p)
{
    const TencImg &im = p.t.imgs[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int upr = (im.cols + 3) >> 2;
    if (idx >= (int64_t)im.rows * upr) return;
    const int y = (int)(idx / upr), x0 = 4 * (int)(idx % upr), npx = min(4, im.cols - x0);
    const int k = y / im.rps, ry = y - k * im.rps, cn = p.t.cn;
    const int64_t rowb = (int64_t)im.cols * cn;
    uint8_t *strip;
    if (p.raw_to_file) strip = p.t.out + im.out_off + im.data_at + (int64_t)k * ((im.rps * rowb + 1) & ~(int64_t)1);
    else strip = (uint8_t *)(p.stage + im.pack_off + (int64_t)k * im.pack_w);
    const uint8_t *row = p.t.src + im.src_off + (int64_t)y * p.t.step;
    uint8_t *dst = strip + ry * rowb;
    if (cn == 1) stage_unit<1>(row, im.cols, x0, npx, p.predictor == 2, dst);
    else stage_unit<3>(row, im.cols, x0, npx, p.predictor == 2, dst);
    // the zero between an odd strip and the next one
    if (p.raw_to_file && x0 + npx == im.cols && ry + 1 == strip_rows(im, k) && k + 1 < im.ns && ((strip_rows(im, k) * rowb) & 1)) dst[rowb] = 0;
}

// Compression 1: a strip's bytes are its rows'.  Bounds: k < ns.
__global__ __launch_bounds__(256) void tenc8_rawlens_kernel(Tenc8Pass p)
{
    const TencImg &im = p.t.imgs[blockIdx.y];
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= im.ns) return;
    p.t.sbytes[im.strip0 + k] = (uint32_t)strip_rows(im, k) * (uint32_t)im.cols * (uint32_t)p.t.cn;
}

// ---- LZW.
constexpr int CHUNK_DW = 256;  // dwords of input in LDS at a time

// A wave per strip.  Lane 0 walks the input and finds the codes, at most 64 a round; a round ends early behind a Clear, so
// that the codes of a round have consecutive indices i0 .. i0 + n - 1 since the last Clear and code j of the round begins
// tlzw_bits_before(i0 + j) - tlzw_bits_before(i0) bits behind the round's first.  The lanes OR their codes into the round's
// dwords in LDS (bit 31 first); whole dwords go out byte-swapped, the open one starts the next round.
// LDS: 24 KB of table and 1.4 KB besides, six workgroups a CU.
// Bounds: the table is indexed through tlzwe_find (below TLZWE_SLOTS); inb at (pos - c0) >> 2 with c0 <= pos < c0 + 4 CHUNK_DW;
// the input is read in dwords below pack_w, the strip's room in the staging buffer; a round takes at most 31 + 64 x 12 bits,
// 25 dwords of obuf; the segment is written below seg_w, which holds tlzwe_strip_bound of the strip.  The rounds are
// counted: every round takes a byte, sends a code or loads a chunk, so `rounds` is never reached.
__global__ __launch_bounds__(64) void tenc8_lzw_kernel(Tenc8Pass p)
{
    __shared__ uint32_t tab[TLZWE_SLOTS];
    __shared__ uint32_t inb[CHUNK_DW], codes[64], obuf[32], st[8];
    const TencImg &im = p.t.imgs[blockIdx.y];
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= im.ns) return;  // the whole wave
    const uint32_t total = (uint32_t)strip_rows(im, k) * (uint32_t)im.cols * (uint32_t)p.t.cn;
    const uint32_t *in = p.stage + im.pack_off + (int64_t)k * im.pack_w;
    uint32_t *out = p.code + im.code_off + (int64_t)k * im.seg_w;
    const uint32_t in_dw = (uint32_t)im.pack_w, out_dw = (uint32_t)im.seg_w;
    for (uint32_t h = lane; h < TLZWE_SLOTS; h += 64) tab[h] = TLZWE_EMPTY;
    if (lane < 32) obuf[lane] = lane == 0 ? TLZW_CLEAR << 23 : 0;  // a strip begins with Clear, 9 bits
    uint32_t bits = 9;                      // of the strip so far
    uint32_t pos = 0, c0 = 0, c1 = 0;       // input taken; the chunk in LDS is [c0, c1)
    uint32_t ent = TLZWE_NONE, idx = 0;     // the match so far; the index of the next code
    uint32_t fin = 0;                       // 1: EOI is still to come (behind a Clear), 2: sent
    const uint32_t rounds = 2 * total + total / (4 * CHUNK_DW) + 8;
    for (uint32_t round = 0; round < rounds && fin != 2; round++) {
        if (pos == c1 && pos < total) {  // the next chunk, from a dword boundary
            c0 = pos & ~3u, c1 = min(total, c0 + 4 * CHUNK_DW);
            __syncthreads();
            for (int j = lane; j < CHUNK_DW; j += 64) {
                const uint32_t d = (c0 >> 2) + (uint32_t)j;
                inb[j] = d < in_dw ? in[d] : 0u;
            }
        }
        __syncthreads();
        const uint32_t i0 = idx;
        if (lane == 0) {
            uint32_t n = 0, clr = 0;
            auto send = [&](uint32_t code) {
                codes[n++] = code;
                if (++idx == TLZWE_CLEAR_AT) codes[n++] = TLZW_CLEAR, idx = 0, clr = 1;
            };
            if (fin == 1) {
                codes[n++] = TLZW_EOI, fin = 2;
            } else {
                while (n <= 61 && pos < c1 && !clr) {
                    const uint32_t o = pos - c0, b = (inb[o >> 2] >> (8 * (o & 3))) & 255u;
                    pos++;
                    if (ent == TLZWE_NONE) {
                        ent = b;
                        continue;
                    }
                    const uint32_t key = ent << 8 | b;
                    uint32_t slot = 0;
                    const uint32_t c = tlzwe_find(tab, key, &slot);
                    if (c != TLZWE_EMPTY) {
                        ent = c;
                        continue;
                    }
                    tab[slot] = key << 12 | (TLZW_FIRST + idx);
                    send(ent);
                    ent = b;
                }
                if (pos == total && n <= 61 && !clr) {  // the last match, then EOI: at once, or behind the Clear
                    send(ent);
                    if (clr) fin = 1;
                    else codes[n++] = TLZW_EOI, fin = 2;
                }
            }
            st[0] = n, st[1] = pos, st[2] = ent, st[3] = idx, st[4] = fin, st[5] = clr;
        }
        __syncthreads();
        const uint32_t n = st[0], clr = st[5];
        pos = st[1], ent = st[2], idx = st[3], fin = st[4];
        const uint32_t base = tlzw_bits_before(i0), r0 = bits & 31u;
        if ((uint32_t)lane < n) {
            const uint32_t i = i0 + (uint32_t)lane, w = tlzw_width(i), q = r0 + tlzw_bits_before(i) - base;
            const uint32_t d = q >> 5, sft = q & 31u, c = codes[lane];
            if (sft + w <= 32) {
                atomicOr(&obuf[d], c << (32 - sft - w));
            } else {
                atomicOr(&obuf[d], c >> (sft + w - 32));
                atomicOr(&obuf[d + 1], c << (64 - sft - w));
            }
        }
        __syncthreads();
        const uint32_t rbits = tlzw_bits_before(i0 + n) - base, full = (r0 + rbits) >> 5, dw0 = bits >> 5;
        if ((uint32_t)lane < full && dw0 + (uint32_t)lane < out_dw) out[dw0 + lane] = __builtin_bswap32(obuf[lane]);
        const uint32_t open = obuf[full];
        __syncthreads();
        if (lane < 32) obuf[lane] = lane == 0 ? open : 0;
        bits += rbits;
        if (clr)
            for (uint32_t h = lane; h < TLZWE_SLOTS; h += 64) tab[h] = TLZWE_EMPTY;
    }
    __syncthreads();
    if (lane == 0) {
        if ((bits & 31u) && (bits >> 5) < out_dw) out[bits >> 5] = __builtin_bswap32(obuf[0]);
        p.t.sbytes[im.strip0 + k] = (bits + 7) >> 3;
    }
}

// ---- the strips into the file.
// A workgroup per piece of TENC8_PIECE bytes of a strip, a thread per aligned dword of the file: whole dwords where all four
// bytes are the strip's, bytes at its ends, a zero behind an odd strip that another follows.
// Bounds: k < ns; byte j of the strip is read below nbytes <= 4 seg_w; what is written is file bytes data_at + soff[k] + j
// for j < nbytes, and j = nbytes where the next strip begins at soff[k] + nbytes + 1.
__global__ __launch_bounds__(256) void tenc8_copy_kernel(Tenc8Pass p, int pieces)
{
    const TencImg &im = p.t.imgs[blockIdx.y];
    const int k = blockIdx.x / pieces, piece = blockIdx.x % pieces;
    if (im.rows == 0 || k >= im.ns) return;
    const uint32_t nbytes = p.t.sbytes[im.strip0 + k];
    const uint32_t npad = nbytes + ((nbytes & 1u) && k + 1 < im.ns ? 1u : 0u);
    const uint32_t *seg = p.code + im.code_off + (int64_t)k * im.seg_w;
    const uint8_t *segb = (const uint8_t *)seg;
    uint8_t *dst = p.t.out + im.out_off + im.data_at + p.t.soff[im.strip0 + k];
    const uint32_t m = (uint32_t)((uintptr_t)dst & 3u);
    // slot t of the file's dwords holds the strip's bytes 4 t - m .. 4 t - m + 3
    const uint32_t t0 = (uint32_t)piece * (TENC8_PIECE / 4);
    for (uint32_t t = t0 + threadIdx.x; t < t0 + TENC8_PIECE / 4; t += 256) {
        const int64_t j0 = 4 * (int64_t)t - m;
        if (j0 >= (int64_t)npad) break;
        if (j0 >= 0 && j0 + 4 <= (int64_t)nbytes) {
            const uint32_t q = (uint32_t)j0 >> 2;
            const uint32_t v = m == 0 ? seg[q] : (seg[q] >> (8 * (4 - m))) | (seg[q + 1] << (8 * m));
            *(uint32_t *)(dst + j0) = v;
        } else {
            for (int b = 0; b < 4; b++) {
                const int64_t j = j0 + b;
                if (j >= 0 && j < (int64_t)npad) dst[j] = j < (int64_t)nbytes ? segb[j] : (uint8_t)0;
            }
        }
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? OMR_OK : fail_gpu(what, e);
}

unsigned up_div(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

int tenc8_launch_stage(const Tenc8Pass &p, int64_t max_units, hipStream_t s)
{
    tenc8_stage_kernel<<<dim3(up_div(max_units, 256), (unsigned)p.t.n), 256, 0, s>>>(p);
    return launched("tenc8_stage_kernel");
}

int tenc8_launch_lzw(const Tenc8Pass &p, int max_strips, hipStream_t s)
{
    tenc8_lzw_kernel<<<dim3((unsigned)max_strips, (unsigned)p.t.n), 64, 0, s>>>(p);
    return launched("tenc8_lzw_kernel");
}

int tenc8_launch_rawlens(const Tenc8Pass &p, int max_strips, hipStream_t s)
{
    tenc8_rawlens_kernel<<<dim3(up_div(max_strips, 256), (unsigned)p.t.n), 256, 0, s>>>(p);
    return launched("tenc8_rawlens_kernel");
}

int tenc8_launch_copy(const Tenc8Pass &p, int max_strips, int64_t max_seg_bytes, hipStream_t s)
{
    const int pieces = (int)up_div(max_seg_bytes + 4, TENC8_PIECE);
    tenc8_copy_kernel<<<dim3((unsigned)max_strips * (unsigned)pieces, (unsigned)p.t.n), 256, 0, s>>>(p, pieces);
    return launched("tenc8_copy_kernel");
}

}  // namespace omr
