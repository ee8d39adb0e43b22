// orient.hip -- the eight EXIF orientation transforms (OpenCV's ExifTransform, Pillow's exif_transpose) on a batch of
// device-resident images of 1 or 3 byte channels, each by its own code and of its own size: one launch, grid (tile, image).
//
//   code  1 copy   2 flip left-right   3 turn by 180   4 flip top-bottom
//         5 transpose   6 transpose + flip left-right (90 clockwise)   7 transpose + flip both   8 transpose + flip top-bottom
//
// A workgroup moves one square tile of pixels (128 a side for 1 channel, 64 for 3) through LDS.  Both sides of the move run
// along rows of global memory: the tile's segment of a row is visited as the aligned dwords that cover it, consecutive
// lanes taking consecutive dwords -- a dword that lies inside the segment moves as a dword, the ragged ones at either end
// byte by byte, so no byte outside the segment is read or written (a 3-channel row's length and pitch are in general no
// multiple of 4, so the ends differ from row to row).  The LDS image of a source row keeps the row's alignment -- its
// first byte stands (address & 3) bytes into the LDS row -- which makes the load dword to dword.  The store gathers its
// four bytes from LDS one by one: along an LDS row (forwards or backwards) for codes 1..4, down a column for 5..8.
//
// LDS layout: row r at r * P + 4 * (r >> 5) bytes, P = 4 * Q with Q = 33 (1 channel) or 49 (3 channels) dwords.  Byte
// reads bank by (address / 4) % 32 within each half wave.  Down a column of a 1-channel tile consecutive lanes are 4 rows
// apart: r * Q alone would give 4 * (lane % 8) -- a 4-way conflict -- and the (r >> 5) dword that every 32 rows add
// separates the four; in a 3-channel tile consecutive lanes are 4 / 3 rows apart and Q odd makes any 32 consecutive rows
// distinct, which leaves a 2-way conflict on the eleven rows a half wave reaches beyond 32.  Rows shifted by differing
// (address & 3) can add one more where a column crosses a dword.  Codes 1..4 read consecutive dwords: no conflict.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "orient.hpp"

namespace omr {
namespace {

constexpr int ORIENT_THREADS = 256;

template <int CN>
struct Geom {
    static constexpr int TS = CN == 1 ? 128 : 64;  // pixels a side
    static constexpr int ND = (TS * CN + 6) / 4;   // aligned dwords that cover a row segment at any alignment
    static constexpr int P = 4 * ND;               // LDS row pitch in bytes
    static constexpr int BYTES = TS * P + 16;      // with the dwords the rows' (r >> 5) adds
    static_assert(ND % 2 == 1, "an odd pitch in dwords keeps 32 consecutive rows on 32 banks");
};

template <int CN>
__device__ __forceinline__ int lrow(int r)
{
    return r * Geom<CN>::P + 4 * (r >> 5);
}

template <int CN>
__global__ __launch_bounds__(ORIENT_THREADS) void orient_kernel(const uint8_t *__restrict__ src, int64_t sstep,
                                                                uint8_t *__restrict__ dst, int64_t dstep,
                                                                const OrientImg *__restrict__ recs)
{
    using G = Geom<CN>;
    constexpr int TS = G::TS, ND = G::ND;
    __shared__ uint32_t tile32[G::BYTES / 4];
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile32);

    const OrientImg im = recs[blockIdx.y];
    const int tiles_y = (im.rows + TS - 1) / TS;
    const int t = (int)blockIdx.x;
    if (t >= im.tiles_x * tiles_y) return;  // the grid is as wide as the batch's largest image
    const int ty = t / im.tiles_x, tx = t - ty * im.tiles_x;
    const int r0 = ty * TS, c0 = tx * TS;
    const int h = min(TS, im.rows - r0), w = min(TS, im.cols - c0);
    const bool T = orient_transposes(im.code), FR = orient_flips_rows(im.code), FC = orient_flips_cols(im.code);

    // ---- the tile's source rows -> LDS
    const uint8_t *s0 = src + im.src_off + (int64_t)r0 * sstep + (int64_t)c0 * CN;
    const uint32_t s0_lo = (uint32_t)(uintptr_t)s0 & 3u, sstep_lo = (uint32_t)sstep & 3u;
    const int L = w * CN;
    for (int e = (int)threadIdx.x; e < h * ND; e += ORIENT_THREADS) {
        const int i = e / ND, d = e - i * ND;
        const uint8_t *row = s0 + (int64_t)i * sstep;
        const int b0 = 4 * d - (int)((s0_lo + (uint32_t)i * sstep_lo) & 3u);  // the dword's first byte, counted in the segment
        if (b0 >= 0 && b0 + 4 <= L) {
            tile32[(lrow<CN>(i) >> 2) + d] = *reinterpret_cast<const uint32_t *>(row + b0);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (b0 + k >= 0 && b0 + k < L) tile[lrow<CN>(i) + 4 * d + k] = row[b0 + k];
        }
    }
    __syncthreads();

    // ---- LDS -> the tile's destination rows
    const int dh = T ? w : h, dw = T ? h : w;
    const int rr = FR ? im.rows - (r0 + h) : r0, cc = FC ? im.cols - (c0 + w) : c0;  // where the tile's rows / columns land
    uint8_t *d0 = dst + im.dst_off + (int64_t)(T ? cc : rr) * dstep + (int64_t)(T ? rr : cc) * CN;
    const uint32_t d0_lo = (uint32_t)(uintptr_t)d0 & 3u, dstep_lo = (uint32_t)dstep & 3u;
    const int Ld = dw * CN;
    for (int e = (int)threadIdx.x; e < dh * ND; e += ORIENT_THREADS) {
        const int i = e / ND, d = e - i * ND;
        uint8_t *row = d0 + (int64_t)i * dstep;
        const int b0 = 4 * d - (int)((d0_lo + (uint32_t)i * dstep_lo) & 3u);
        if (b0 >= Ld || b0 + 4 <= 0) continue;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int b = b0 + k;
            if (b < 0 || b >= Ld) continue;
            const int px = b / CN, ch = b - px * CN;
            // destination pixel (i, px) of the tile comes from source pixel (sr, sc) of the tile
            const int sr = T ? (FR ? h - 1 - px : px) : (FR ? h - 1 - i : i);
            const int sc = T ? (FC ? w - 1 - i : i) : (FC ? w - 1 - px : px);
            const int sh = (int)((s0_lo + (uint32_t)sr * sstep_lo) & 3u);
            v |= (uint32_t)tile[lrow<CN>(sr) + sh + sc * CN + ch] << (8 * k);
        }
        if (b0 >= 0 && b0 + 4 <= Ld) {
            *reinterpret_cast<uint32_t *>(row + b0) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (b0 + k >= 0 && b0 + k < Ld) row[b0 + k] = (uint8_t)(v >> (8 * k));
        }
    }
}

}  // namespace

void orient_plan(OrientImg *recs, int n, int cn, int *max_tiles)
{
    const int ts = cn == 1 ? Geom<1>::TS : Geom<3>::TS;
    int m = 1;
    for (int i = 0; i < n; i++) {
        recs[i].tiles_x = (recs[i].cols + ts - 1) / ts;
        m = std::max(m, recs[i].tiles_x * ((recs[i].rows + ts - 1) / ts));
    }
    *max_tiles = m;
}

hipError_t orient_launch(const uint8_t *d_src, int64_t sstep, uint8_t *d_dst, int64_t dstep, int cn, const OrientImg *d_recs,
                         int n, int max_tiles, hipStream_t s)
{
    const dim3 grid((unsigned)max_tiles, (unsigned)n);
    if (cn == 1) orient_kernel<1><<<grid, ORIENT_THREADS, 0, s>>>(d_src, sstep, d_dst, dstep, d_recs);
    else orient_kernel<3><<<grid, ORIENT_THREADS, 0, s>>>(d_src, sstep, d_dst, dstep, d_recs);
    return hipGetLastError();
}

}  // namespace omr
