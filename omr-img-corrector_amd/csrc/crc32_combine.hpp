// crc32_combine.hpp -- the arithmetic that lets CRC-32 (ISO 3309, PNG's) be computed in pieces: plain C++ for the host and
// for device code alike (png_enc.hip; tests/test_png_encode_abi.py compiles it into a host program and compares with zlib).
//
// A CRC register is a polynomial over GF(2) modulo P = 0xEDB88320 (reflected: bit 31 is x^0).  crc_raw(M) below is the
// register after the bytes M from register 0, without the pre- and post-conditioning; it is linear:
//     crc_raw(A || B) = crc_shift(crc_raw(A), |B|) ^ crc_raw(B),
// where crc_shift(c, n) = c * x^(8 n) mod P is what n zero bytes do to a register.  The CRC-32 of a message M is
//     ~(crc_shift(0xffffffff, |M|) ^ crc_raw(M)).
// This is zlib's crc32_combine (multmodp, x2nmodp) without its tables.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OMR_CRC_HD __host__ __device__ inline
#else
#define OMR_CRC_HD inline
#endif

namespace omr {

constexpr uint32_t CRC_POLY = 0xEDB88320u;

// one byte into a register, bit by bit (the encoder's few header bytes; bulk data goes through a table)
OMR_CRC_HD uint32_t crc_byte(uint32_t c, uint8_t b)
{
    c ^= b;
    for (int k = 0; k < 8; k++) c = c & 1 ? CRC_POLY ^ (c >> 1) : c >> 1;
    return c;
}

// a * b mod P: a carry-less multiply of 32 steps
OMR_CRC_HD uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) {
        if (a >> k & 1) p ^= b;
        b = b & 1 ? CRC_POLY ^ (b >> 1) : b >> 1;
    }
    return p;
}

// x^(8 n) mod P by square-and-multiply over the bits of n: at most 64 rounds
OMR_CRC_HD uint32_t crc_x8n(uint64_t n)
{
    uint32_t r = 0x80000000u;  // x^0
    uint32_t b = 0x00800000u;  // x^8
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mulmod(r, b);
        b = crc_mulmod(b, b);
    }
    return r;
}

// the register c after n more zero bytes
OMR_CRC_HD uint32_t crc_shift(uint32_t c, uint64_t n) { return crc_mulmod(c, crc_x8n(n)); }

}  // namespace omr
