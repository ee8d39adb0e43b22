// png_adler.hpp -- Adler-32 of bytes in device memory, the part the PNG decoder (png_dec.hip) and the PNG encoder
// (png_enc.hip) share.  Device code only.
//
// Adler-32 = (1 + sum b_i) mod 65521 | (n + sum (n - i) b_i) mod 65521 << 16.  A workgroup of 256 threads takes
// PNG_ADLER_CHUNK bytes, every thread 256 of them, and adds its part of the two sums (each below 65521 x 256) to the
// image's; integer additions, so the result does not depend on the order in which they land.  adler_finish folds them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace omr {

constexpr int PNG_ADLER_CHUNK = 65536;  // bytes per workgroup

// called by all 256 threads of workgroup `chunk` of an image (uniform control flow: it holds barriers); q = the image's
// n bytes; *a_sum and *b_sum were zero before the launch
__device__ inline void adler_chunk_sums(const uint8_t *data, uint32_t n, uint32_t chunk, unsigned long long *a_sum,
                                        unsigned long long *b_sum)
{
    const uint64_t at = (uint64_t)chunk * PNG_ADLER_CHUNK + (uint64_t)threadIdx.x * 256;
    __shared__ unsigned long long sa[256], sb[256];
    unsigned long long a = 0, b = 0;
    if (at < n) {
        const uint8_t *q = data + at;
        const uint32_t m = (uint32_t)min((uint64_t)256, (uint64_t)n - at);
        uint32_t s1 = 0, s2 = 0;
        for (uint32_t j = 0; j < m; j++) s1 += q[j], s2 += (m - j) * q[j];
        const uint64_t rest = (uint64_t)n - at - m;  // bytes behind this thread's
        a = s1;
        b = (s2 + (rest % 65521u) * s1) % 65521u;
    }
    sa[threadIdx.x] = a, sb[threadIdx.x] = b;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) sa[threadIdx.x] += sa[threadIdx.x + d], sb[threadIdx.x] += sb[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && (uint64_t)chunk * PNG_ADLER_CHUNK < n) {
        atomicAdd(a_sum, sa[0] % 65521u);
        atomicAdd(b_sum, sb[0] % 65521u);
    }
}

__device__ inline uint32_t adler_finish(uint32_t n, unsigned long long a_sum, unsigned long long b_sum)
{
    const uint32_t a = (uint32_t)((1 + a_sum) % 65521u);
    const uint32_t b = (uint32_t)((n % 65521u + b_sum) % 65521u);
    return b << 16 | a;
}

}  // namespace omr
