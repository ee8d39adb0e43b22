// tiff8_enc_fuzz.cpp -- a stand-alone program that drives the serial logic of the LZW encoder (csrc/tiff_lzw_enc.hpp: the
// hash table, the Clear rule, the widths, EOI and the pad, as tenc8_lzw_kernel applies them) under the host sanitizers and
// checks the round trip through the decoder's serial logic (tlzw_decode_serial, csrc/tiff_lzw.hpp) on random and structured
// strips, and the strip bound on every one.  CPU only.
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ -I omr-img-corrector_amd/csrc tests/fuzz/tiff8_enc_fuzz.cpp -o tiff8_enc_fuzz && ./tiff8_enc_fuzz
// Every buffer handed over is an exact-size heap block, so one byte read or written past its end is reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tiff_lzw_enc.hpp"

static long strips, clears, bytes_in, bytes_out;

static uint32_t rnd_state = 12345;
static uint32_t rnd()
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

// the Clears behind the first, read back with the decoder's own bit reader
static long count_clears(const uint8_t *s, uint32_t len)
{
    auto byte = [&](uint32_t k) -> uint32_t { return k < len ? s[k] : 0u; };
    uint32_t pos = 9, i = 0;
    long n = 0;
    for (;;) {
        const uint32_t c = omr::tlzw_code(byte, pos, omr::tlzw_width(i), len * 8);
        if (c == omr::TLZW_MISSING || c == omr::TLZW_EOI) return n;
        pos += omr::tlzw_width(i);
        if (c == omr::TLZW_CLEAR) {
            if (i != omr::TLZWE_CLEAR_AT) printf("a Clear at index %u\n", i), exit(1);
            n++, i = 0;
        } else {
            i++;
        }
    }
}

static void one(const std::vector<uint8_t> &data)
{
    const uint32_t n = (uint32_t)data.size();
    const uint32_t cap = (uint32_t)omr::tlzwe_strip_bound(n);
    uint8_t *in = (uint8_t *)malloc(n);
    memcpy(in, data.data(), n);
    uint8_t *enc = (uint8_t *)malloc(cap);
    uint32_t *tab = (uint32_t *)malloc(sizeof(uint32_t) * omr::TLZWE_SLOTS);
    const uint32_t len = omr::tlzw_encode_serial(in, n, enc, cap, tab);
    if (len == omr::TLZW_MISSING || len > cap) printf("%u bytes: the strip passes its bound %u\n", n, cap), exit(1);
    // a buffer one byte short is refused and never overrun
    if (len > 0) {
        uint8_t *tight = (uint8_t *)malloc(len - 1 ? len - 1 : 1);
        if (omr::tlzw_encode_serial(in, n, tight, len - 1, tab) != omr::TLZW_MISSING) printf("%u bytes: a short buffer accepted\n", n), exit(1);
        free(tight);
    }
    // the round trip, from an exact-size copy
    uint8_t *strip = (uint8_t *)malloc(len);
    memcpy(strip, enc, len);
    uint8_t *out = (uint8_t *)malloc(n);
    uint32_t *tp = (uint32_t *)malloc(sizeof(uint32_t) * omr::TLZW_ENTRIES);
    uint16_t *tl = (uint16_t *)malloc(sizeof(uint16_t) * omr::TLZW_ENTRIES);
    const uint32_t e = omr::tlzw_decode_serial(strip, len, out, n, tp, tl);
    if (e || memcmp(out, in, n)) printf("%u bytes: the round trip fails (error %u)\n", n, e), exit(1);
    clears += count_clears(strip, len);
    strips++, bytes_in += n, bytes_out += len;
    free(in), free(enc), free(tab), free(strip), free(out), free(tp), free(tl);
}

int main()
{
    std::vector<uint8_t> d;
    // every short length, noise and constant
    for (uint32_t n = 1; n <= 600; n++) {
        d.assign(n, 0);
        for (auto &b : d) b = (uint8_t)rnd();
        one(d);
        d.assign(n, 200);
        one(d);
    }
    // noise of a few alphabets around the width switches and the full table
    for (uint32_t alphabet : {2u, 3u, 16u, 256u})
        for (uint32_t n : {253u, 254u, 255u, 765u, 766u, 767u, 1789u, 1790u, 1791u, 3835u, 3836u, 3837u, 3838u, 3839u, 4096u, 8192u, 16384u, 40000u}) {
            d.assign(n, 0);
            for (auto &b : d) b = (uint8_t)(rnd() % alphabet);
            one(d);
        }
    // strips that end around a Clear: 16 KB of noise fills the table four times; cut at every length near the first fills
    d.assign(16384, 0);
    for (auto &b : d) b = (uint8_t)rnd();
    for (uint32_t n = 5500; n < 5900; n++) one(std::vector<uint8_t>(d.begin(), d.begin() + n));
    // periods, ramps and their differences, long runs with rare changes (KwKwK chains, long entries)
    for (uint32_t period : {1u, 2u, 3u, 7u, 255u, 256u, 257u}) {
        d.assign(20000, 0);
        for (size_t k = 0; k < d.size(); k++) d[k] = (uint8_t)(k % period);
        one(d);
    }
    d.assign(30000, 255);
    for (int k = 0; k < 40; k++) d[rnd() % d.size()] = (uint8_t)rnd();
    one(d);
    // random lengths and mixtures
    for (int t = 0; t < 300; t++) {
        const uint32_t n = 1 + rnd() % 12000, alphabet = 1 + rnd() % 256, run = 1 + rnd() % 40;
        d.assign(n, 0);
        uint8_t cur = 0;
        for (uint32_t k = 0; k < n; k++) {
            if (rnd() % run == 0) cur = (uint8_t)(rnd() % alphabet);
            d[k] = cur;
        }
        one(d);
    }
    printf("tiff8_enc_fuzz: %ld strips, %ld bytes in, %ld out, %ld Clears at index %u, all round trips exact\n", strips, bytes_in, bytes_out,
           clears, omr::TLZWE_CLEAR_AT);
    if (clears < 10) printf("too few full tables\n"), exit(1);
    return 0;
}
