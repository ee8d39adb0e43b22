// row_bytes.hpp -- reading a piece of an image row on the device at any base address and pitch: aligned dword loads
// where the dword lies inside the row, byte loads of the row's own bytes at its two ends.  Shared by the TIFF encoders'
// first kernels (tiff_enc.hip, tiff_enc8.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace omr {

// Bytes [sb, sb + nbytes) of a row (row .. row + row_len) -> v[k] = bytes 4 k .. 4 k + 3 of them, little-endian.  Aligned
// dword loads where the dword lies inside the ROW (neighbouring threads' bytes included), byte loads of the row's own bytes
// where it straddles an end: nothing outside the row is read, at any base address and pitch.
template <int NW>
__device__ __forceinline__ void load_segment(const uint8_t *row, int row_len, int sb, int nbytes, uint32_t (&v)[NW])
{
    const uintptr_t r0 = (uintptr_t)row, r1 = r0 + (uintptr_t)row_len, p = r0 + (uintptr_t)sb;
    const uint32_t a = (uint32_t)(p & 3);
    const uintptr_t q = p - a;
    uint32_t w[NW + 1];
#pragma unroll
    for (int k = 0; k <= NW; k++) {
        const uintptr_t d = q + 4 * (uintptr_t)k;
        uint32_t x = 0;
        if (d < p + (uintptr_t)nbytes) {
            if (d >= r0 && d + 4 <= r1) {
                x = *(const uint32_t *)d;
            } else {
                for (int b = 0; b < 4; b++)
                    if (d + b >= r0 && d + b < r1) x |= (uint32_t)*(const uint8_t *)(d + b) << (8 * b);
            }
        }
        w[k] = x;
    }
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = a ? (w[k] >> (8 * a)) | (w[k + 1] << (32 - 8 * a)) : w[k];
}

template <int NW>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&v)[NW], int b)
{
    return (v[b >> 2] >> (8 * (b & 3))) & 255u;
}

}  // namespace omr
