// tiff_lzw.hpp -- the serial logic of the TIFF 6.0 LZW decoder for the device and the host alike:
// where a code stands in the bit stream, how it is read, which codes are refused, and what a table entry is.  tdec_lzw
// (tiff_dec8.hip) applies these to 64 codes at a time; tlzw_decode_serial below applies them to one code at a time and is
// what tests/fuzz/tiff8_fuzz.cpp drives under the host sanitizers.
//
// The stream: codes most significant bit first, Clear 256, EOI 257, the first free entry 258.  Since the last Clear the
// code with index 0 is a literal and adds nothing; the code with index i >= 1 adds entry 257 + i.  The width of the code
// with index i is therefore fixed by i alone: 9 bits while the next free entry is below 511, 10 below 1023, 11 below 2047,
// else 12 (the early change), which is i < 254, i < 766, i < 1790.
//
// A table entry is a substring of the strip's own output: the entry that code i adds is the output of code i - 1 and the
// first byte of code i, and those bytes lie next to each other.  So an entry is (position, length), never a byte chain.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TLZW_FN __host__ __device__ inline
#else
#define TLZW_FN inline
#endif

namespace omr {

constexpr uint32_t TLZW_CLEAR = 256, TLZW_EOI = 257, TLZW_FIRST = 258, TLZW_ENTRIES = 4096;
constexpr uint32_t TLZW_MISSING = 0xffffffffu;  // the code would end behind the strip's last bit
// the values of TdecErr
constexpr uint32_t TLZW_ERR_INPUT = 1, TLZW_ERR_CODE = 2, TLZW_ERR_TABLE = 4;

// the bits of the codes with index 0 .. i - 1 since a Clear
TLZW_FN uint32_t tlzw_bits_before(uint32_t i)
{
    return 9 * i + (i > 254 ? i - 254 : 0) + (i > 766 ? i - 766 : 0) + (i > 1790 ? i - 1790 : 0);
}

TLZW_FN uint32_t tlzw_width(uint32_t i) { return 9 + (i >= 254) + (i >= 766) + (i >= 1790); }

// The `width` bits from bit `bitpos` of a strip of `bitlen` bits, or TLZW_MISSING for a code that does not fit: libtiff
// takes such a strip as ended.  byte(k) gives the strip's byte k, and 0 behind its end.
template <class Bytes>
TLZW_FN uint32_t tlzw_code(const Bytes &byte, uint32_t bitpos, uint32_t width, uint32_t bitlen)
{
    if (bitpos > bitlen || width > bitlen - bitpos) return TLZW_MISSING;
    const uint32_t k = bitpos >> 3;
    const uint32_t v = byte(k) << 16 | byte(k + 1) << 8 | byte(k + 2);
    return (v >> (24 - (bitpos & 7) - width)) & ((1u << width) - 1);
}

// A code other than Clear and EOI with index i since the last Clear: 0, or why the strip is refused.  A code may name
// the entry it is about to add (257 + i, the KwKwK form) and nothing above; so index 0 is a literal.  Entry 4095 is the
// last one.
TLZW_FN uint32_t tlzw_check(uint32_t code, uint32_t i)
{
    if (code > 257 + i) return TLZW_ERR_CODE;
    if (i >= 1 && 257 + i >= TLZW_ENTRIES) return TLZW_ERR_TABLE;
    return 0;
}

// One strip, a code at a time: `total` bytes into out, or an error.  tab_pos / tab_len: TLZW_ENTRIES each.  What ends a
// strip well: its rows are full (whatever follows is not read).  What is refused: a strip that does not begin with
// Clear, tlzw_check's cases, and input that ends (EOI, or no room for a code) before the rows are full.
TLZW_FN uint32_t tlzw_decode_serial(const uint8_t *in, uint32_t len, uint8_t *out, uint32_t total, uint32_t *tab_pos, uint16_t *tab_len)
{
    auto byte = [&](uint32_t k) -> uint32_t { return k < len ? in[k] : 0u; };
    const uint32_t bitlen = len * 8;
    uint32_t pos = 0, o = 0, i = 0, prev_pos = 0, prev_len = 0;
    uint32_t c = tlzw_code(byte, 0, 9, bitlen);
    if (c != TLZW_CLEAR) return c == TLZW_MISSING ? TLZW_ERR_INPUT : TLZW_ERR_CODE;
    pos = 9;
    while (o < total) {  // a code a turn, at least 9 bits of bitlen each
        const uint32_t w = tlzw_width(i);
        c = tlzw_code(byte, pos, w, bitlen);
        if (c == TLZW_MISSING || c == TLZW_EOI) return TLZW_ERR_INPUT;
        pos += w;
        if (c == TLZW_CLEAR) {
            i = 0;
            continue;
        }
        if (const uint32_t e = tlzw_check(c, i)) return e;
        uint32_t src = 0, n = 1;
        if (c >= TLZW_FIRST) {
            if (c == 257 + i) src = prev_pos, n = prev_len + 1;  // KwKwK: the copy below reads its own first byte last
            else src = tab_pos[c], n = tab_len[c];
        }
        if (i >= 1) tab_pos[257 + i] = prev_pos, tab_len[257 + i] = (uint16_t)(prev_len + 1);
        prev_pos = o, prev_len = n;
        const uint32_t m = n < total - o ? n : total - o;
        if (c < 256) out[o] = (uint8_t)c;
        else
            for (uint32_t k = 0; k < m; k++) out[o + k] = out[src + k];  // src + k < o + k: behind the write position
        o += m;
        i++;
    }
    return 0;
}

}  // namespace omr
