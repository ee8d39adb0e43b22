// tiff_lzw_enc.hpp -- the serial logic of the TIFF 6.0 LZW encoder for the device and the host
// alike: when Clear is sent, what the dictionary is, and how many bytes a strip can take.  tenc8_lzw_kernel (tiff_enc8.hip)
// applies these with one lane finding the codes and 64 lanes placing them; tlzw_encode_serial below writes a code at a
// time and is what tests/fuzz/tiff8_enc_fuzz.cpp drives under the host sanitizers, against tlzw_decode_serial.
//
// The stream is the one tiff_lzw.hpp reads: Clear first (9 bits), then the codes of the longest dictionary matches, each
// with the width of its index since the last Clear (tlzw_width), then EOI with the width of the index it stands at, then
// zeros to a byte.  The code with index i adds entry 258 + i (its string and the byte that follows).  Clear is sent when
// the table is full and only then: as libtiff's writer does, once entry 4093 is made, which is after the code with index
// 3835.  So Clear is the code with index TLZWE_CLEAR_AT = 3836 (12 bits), the code behind it has index 0 again, and a
// reader, which adds entry 257 + i at the code with index i, never adds one above 4092.  A strip's last code counts like
// any other: if it has index 3835, Clear follows it and EOI takes 9 bits.
//
// The dictionary is an open-addressed table of TLZWE_SLOTS dwords, key (prefix code << 8 | byte) << 12 | code, probed
// linearly.  At most 3836 entries live in 6144 slots.  Which slot an entry takes never shows in the stream.
#pragma once
#include <stdint.h>

#include "tiff_lzw.hpp"

namespace omr {

constexpr uint32_t TLZWE_CLEAR_AT = 3836;
constexpr uint32_t TLZWE_SLOTS = 6144;
constexpr uint32_t TLZWE_EMPTY = 0xffffffffu;
constexpr uint32_t TLZWE_NONE = 0xffffffffu;  // no prefix yet: a strip's first byte

// 20 bits of key -> a slot
TLZW_FN uint32_t tlzwe_slot(uint32_t key) { return (((key * 0x9E3779B1u) >> 16) * TLZWE_SLOTS) >> 16; }

// The code of `key`, or TLZWE_EMPTY with *slot the free slot where it belongs.  tab[h] for h < TLZWE_SLOTS only; the walk
// ends at a free slot, of which there are always 2308 or more.
template <class Tab>
TLZW_FN uint32_t tlzwe_find(const Tab &tab, uint32_t key, uint32_t *slot)
{
    uint32_t h = tlzwe_slot(key);
    for (uint32_t k = 0; k < TLZWE_SLOTS; k++) {
        const uint32_t e = tab[h];
        if (e == TLZWE_EMPTY) break;
        if ((e >> 12) == key) return e & 4095u;
        h = h + 1 == TLZWE_SLOTS ? 0 : h + 1;
    }
    *slot = h;
    return TLZWE_EMPTY;
}

// Bytes of a strip of n >= 1 raw bytes at most.  Every code but Clear and EOI takes at least one byte of input, so there
// are at most n of them; Clear stands in front and then once behind every 3836 of those, so at most 1 + n / 3836 times;
// EOI once.  No code is wider than 12 bits; the last byte is filled up.
TLZW_FN int64_t tlzwe_strip_bound(int64_t n) { return (12 * (n + n / TLZWE_CLEAR_AT + 2) + 7) / 8; }

// One strip, a code at a time: n >= 1 bytes of `in` -> the strip's bytes in out, at most cap.  Returns their number, or
// TLZW_MISSING where cap does not hold them (nothing is written behind cap).  tab: TLZWE_SLOTS dwords of workspace.
TLZW_FN uint32_t tlzw_encode_serial(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *tab)
{
    uint64_t acc = 0;
    uint32_t nb = 0, len = 0;
    bool fits = true;
    auto put = [&](uint32_t code, uint32_t width) {
        acc = (acc << width) | code, nb += width;
        while (nb >= 8) {
            if (len < cap) out[len] = (uint8_t)(acc >> (nb - 8));
            else fits = false;
            len++, nb -= 8;
        }
    };
    auto wipe = [&]() {
        for (uint32_t h = 0; h < TLZWE_SLOTS; h++) tab[h] = TLZWE_EMPTY;
    };
    wipe();
    put(TLZW_CLEAR, 9);
    uint32_t ent = TLZWE_NONE, i = 0;
    // the code with index i, then Clear where the table is full
    auto send = [&](uint32_t code) {
        put(code, tlzw_width(i));
        if (++i == TLZWE_CLEAR_AT) put(TLZW_CLEAR, tlzw_width(i)), i = 0, wipe();
    };
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t b = in[k];
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
        tab[slot] = key << 12 | (TLZW_FIRST + i);
        send(ent);
        ent = b;
    }
    if (ent != TLZWE_NONE) send(ent);
    put(TLZW_EOI, tlzw_width(i));
    if (nb) put(0, 8 - nb);
    return fits ? len : TLZW_MISSING;
}

}  // namespace omr
