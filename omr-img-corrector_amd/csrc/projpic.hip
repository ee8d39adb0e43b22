// projpic.hip -- the two projection pictures of a sheet (transfer.rs:337-376, :409-455) for one image or a batch: one
// set of kernels, the scan index on a grid axis.  The input is 8-bit, one channel, ANY values; the reference's loops
// reduce to closed forms (tests/projpic_ref.py holds both and compares them):
//
//   horizontal, row r:   k0 = index of the first pixel == 255 (cols when there is none), K = pixels != 255 (K >= k0);
//                        columns [0, k0) keep the source bytes, [k0, K) are 0, [K, cols) are 255
//   vertical, column c:  n = pixels <= 127; rows [0, rows - n) are 255, rows [rows - n, rows) are 0
//
//   projpic_rows_kernel        a wavefront per row: the row is read ONCE, four pixels a lane and step, and every dword
//                              is parked in LDS at the slot its lane comes back to; K and k0 are reduced across the
//                              wave, then the lane writes its dwords of the picture row -- constants beyond k0, the
//                              parked source bytes before it.  No lane reads another lane's slot, so no barrier.
//   projpic_col_counts_kernel  tiles of 256 columns x 256 rows: a lane counts four columns of every fourth row in one
//                              packed register, the four waves meet in LDS, one atomicAdd per column and tile on
//                              uint32 counters in global memory (integer sums: the order does not matter)
//   projpic_col_bars_kernel    the same tiles: a lane takes its four counts and writes its dwords of the bars
//
// Dword loads and stores need the image's base and row pitch to be multiples of 4; any other layout takes byte
// accesses with identical results.  A row's last, partial dword is always read and written byte by byte: nothing is
// read or written past `cols`, so the caller's pitch padding stays as it was.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace omr {
namespace {

constexpr int PP_TILE = 256;  // columns (bytes) and rows of a column tile

__device__ __forceinline__ bool dwords_ok(const void *base, int64_t step)
{
    return (((uintptr_t)base | (uintptr_t)step) & 3) == 0;
}

// the four pixels of a row from column c on; columns at or past `cols` read as 255 (white: neither predicate counts them)
__device__ __forceinline__ uint32_t load4(const uint8_t *row, int c, int cols, bool dw)
{
    if (dw && c + 4 <= cols) return *reinterpret_cast<const uint32_t *>(row + c);
    uint32_t w = 0xffffffffu;
    for (int j = 0; j < 4; j++)
        if (c + j < cols) w = (w & ~(0xffu << (8 * j))) | ((uint32_t)row[c + j] << (8 * j));
    return w;
}

__device__ __forceinline__ void store4(uint8_t *row, int c, int cols, bool dw, uint32_t w)
{
    if (dw && c + 4 <= cols) {
        *reinterpret_cast<uint32_t *>(row + c) = w;
        return;
    }
    for (int j = 0; j < 4; j++)
        if (c + j < cols) row[c + j] = (uint8_t)(w >> (8 * j));
}

// 0x80 in every byte of w that is 255, exactly (no carry crosses a byte)
__device__ __forceinline__ uint32_t bytes_255(uint32_t w)
{
    const uint32_t x = ~w;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// the low `k` bytes of a dword set (k is clamped to 0..4)
__device__ __forceinline__ uint32_t low_bytes(int k)
{
    return k <= 0 ? 0u : k >= 4 ? 0xffffffffu : (1u << (8 * k)) - 1u;
}

__global__ __launch_bounds__(256) void projpic_rows_kernel(ProjPicImg p, int lds_dwords)
{
    extern __shared__ uint32_t parked[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= p.rows) return;  // whole waves leave; the kernel has no barrier
    const uint8_t *S = p.src + (int64_t)blockIdx.y * p.sstride;
    uint8_t *D = p.hdst + (int64_t)blockIdx.y * p.hstride;
    const bool sdw = dwords_ok(S, p.sstep), ddw = dwords_ok(D, p.hstep);
    S += (int64_t)r * p.sstep;
    D += (int64_t)r * p.hstep;
    uint32_t *slot = parked + wave * lds_dwords;
    const int cols = p.cols, nd = (cols + 3) >> 2;

    int K = 0, k0 = cols;
    auto take = [&](int q, uint32_t w) {
        slot[q] = w;
        const uint32_t e = bytes_255(w);
        K += 4 - __popc(e);
        // a lane's q only grow: its first hit is its smallest; a padded byte of the last dword lies at or past cols
        if (e && k0 == cols) k0 = min(cols, 4 * q + ((__ffs((int)e) - 1) >> 3));
    };
    int q = lane;
    if (sdw)  // four loads in flight a lane: none of these dwords is the row's last one
        for (; q + 192 < nd - 1; q += 256) {
            uint32_t w[4];
            for (int i = 0; i < 4; i++) w[i] = *reinterpret_cast<const uint32_t *>(S + 4 * (q + 64 * i));
            for (int i = 0; i < 4; i++) take(q + 64 * i, w[i]);
        }
    for (; q < nd; q += 64) take(q, load4(S, 4 * q, cols, sdw));
    for (int d = 32; d; d >>= 1) {
        K += __shfl_xor(K, d, 64);
        k0 = min(k0, __shfl_xor(k0, d, 64));
    }
    for (q = lane; q < nd; q += 64) {
        const int c = 4 * q;
        // bytes before k0: the source's; before K: 0; the rest: 255 (k0 <= K)
        const uint32_t w = (slot[q] & low_bytes(k0 - c)) | ~low_bytes(K - c);
        store4(D, c, cols, ddw, w);
    }
}

__global__ __launch_bounds__(256) void projpic_col_counts_kernel(ProjPicImg p, uint32_t *counts)
{
    __shared__ uint32_t part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *S = p.src + (int64_t)blockIdx.z * p.sstride;
    const bool sdw = dwords_ok(S, p.sstep);
    const int c = blockIdx.x * PP_TILE + 4 * lane;
    const int r0 = blockIdx.y * PP_TILE, r1 = min(r0 + PP_TILE, p.rows);
    uint32_t acc = 0;  // four byte counters: at most 64 rows a lane
    if (sdw && c + 4 <= p.cols) {
#pragma unroll 8
        for (int r = r0 + wave; r < r1; r += 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(S + (int64_t)r * p.sstep + c);
            acc += (~w >> 7) & 0x01010101u;  // <= 127: the top bit is clear
        }
    } else if (c < p.cols) {
        for (int r = r0 + wave; r < r1; r += 4) acc += (~load4(S + (int64_t)r * p.sstep, c, p.cols, sdw) >> 7) & 0x01010101u;
    }
    part[wave][lane] = acc;
    __syncthreads();
    const int b = threadIdx.x, col = blockIdx.x * PP_TILE + b;  // one column a thread
    if (col < p.cols) {
        uint32_t n = 0;
        for (int w = 0; w < 4; w++) n += (part[w][b >> 2] >> (8 * (b & 3))) & 0xffu;
        if (n) atomicAdd(counts + (int64_t)blockIdx.z * p.cols + col, n);
    }
}

__global__ __launch_bounds__(256) void projpic_col_bars_kernel(ProjPicImg p, const uint32_t *counts)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t *D = p.vdst + (int64_t)blockIdx.z * p.vstride;
    const bool ddw = dwords_ok(D, p.vstep);
    const int c = blockIdx.x * PP_TILE + 4 * lane;
    if (c >= p.cols) return;
    const int r0 = blockIdx.y * PP_TILE, r1 = min(r0 + PP_TILE, p.rows);
    int top[4];  // first black row of the lane's four columns
    for (int j = 0; j < 4; j++) top[j] = c + j < p.cols ? p.rows - (int)counts[(int64_t)blockIdx.z * p.cols + c + j] : p.rows;
    for (int r = r0 + wave; r < r1; r += 4) {
        uint32_t w = 0;
        for (int j = 0; j < 4; j++) w |= (r >= top[j] ? 0u : 0xffu) << (8 * j);
        store4(D + (int64_t)r * p.vstep, c, p.cols, ddw, w);
    }
}

dim3 col_grid(const ProjPicImg &p)
{
    return dim3((p.cols + PP_TILE - 1) / PP_TILE, (p.rows + PP_TILE - 1) / PP_TILE, p.n);
}

}  // namespace

hipError_t launch_projpic_rows(const ProjPicImg &p, hipStream_t s)
{
    if (p.n < 1 || p.n > 65535 || p.cols < 1 || p.cols >= 32767) return hipErrorInvalidValue;
    // a wave parks its row in LDS: four rows a workgroup while they fit 48 KB, one for the longest (32 766 pixels: 32 KB)
    const int lds_dwords = (p.cols + 3) >> 2;
    int waves = 4;
    while (waves > 1 && (size_t)waves * lds_dwords * sizeof(uint32_t) > 48 * 1024) waves >>= 1;
    const dim3 grid((p.rows + waves - 1) / waves, p.n);
    hipLaunchKernelGGL(projpic_rows_kernel, grid, dim3(64 * waves), (size_t)waves * lds_dwords * sizeof(uint32_t), s, p,
                       lds_dwords);
    return hipGetLastError();
}

hipError_t launch_projpic_col_counts(const ProjPicImg &p, uint32_t *d_counts, hipStream_t s)
{
    if (p.n < 1 || p.n > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(projpic_col_counts_kernel, col_grid(p), dim3(256), 0, s, p, d_counts);
    return hipGetLastError();
}

hipError_t launch_projpic_col_bars(const ProjPicImg &p, const uint32_t *d_counts, hipStream_t s)
{
    if (p.n < 1 || p.n > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(projpic_col_bars_kernel, col_grid(p), dim3(256), 0, s, p, d_counts);
    return hipGetLastError();
}

}  // namespace omr
