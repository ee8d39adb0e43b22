// oics_tiff_dec.cpp -- host side of the TIFF decoder (bilevel: tiff_dec.hip; 8-bit gray and RGB:
// tiff_dec8.hip, section 4.27): the walk over the
// first IFD with what it refuses, the run-length code tables of ITU-T T.4 and the lookup table the T.6 kernel reads, the
// launches of a group and the entry points omr_tiff_info / omr_tiff_decode*.  The host visits the header and the tags
// only; everything inside the strips is the device's.  Every offset read from the file is checked against the stream's
// length before it is followed.
//
// With TDEC_PARSER_ONLY defined the file holds the parser and the tables alone and needs no HIP: the stand-alone program
// tests/fuzz/tiff_parse_fuzz.cpp includes it that way.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#ifndef TDEC_PARSER_ONLY
#include "codec_host.hpp"
#include "host_threads.hpp"
#endif
#include "tiff_dec.hpp"
#ifdef TDEC_PARSER_ONLY
namespace omr {
int fail(int code, const char *fmt, ...);  // the including program's
}
#endif

using namespace omr;

namespace {

// ---- ITU-T T.4, Tables 2 and 3: {code, bits}, the code's first bit in the value's top used bit
struct Code {
    uint16_t code;
    uint8_t bits;
};

const Code kWhiteTerm[64] = {
    {0b00110101, 8}, {0b000111, 6},   {0b0111, 4},     {0b1000, 4},     {0b1011, 4},     {0b1100, 4},     {0b1110, 4},     {0b1111, 4},
    {0b10011, 5},    {0b10100, 5},    {0b00111, 5},    {0b01000, 5},    {0b001000, 6},   {0b000011, 6},   {0b110100, 6},   {0b110101, 6},
    {0b101010, 6},   {0b101011, 6},   {0b0100111, 7},  {0b0001100, 7},  {0b0001000, 7},  {0b0010111, 7},  {0b0000011, 7},  {0b0000100, 7},
    {0b0101000, 7},  {0b0101011, 7},  {0b0010011, 7},  {0b0100100, 7},  {0b0011000, 7},  {0b00000010, 8}, {0b00000011, 8}, {0b00011010, 8},
    {0b00011011, 8}, {0b00010010, 8}, {0b00010011, 8}, {0b00010100, 8}, {0b00010101, 8}, {0b00010110, 8}, {0b00010111, 8}, {0b00101000, 8},
    {0b00101001, 8}, {0b00101010, 8}, {0b00101011, 8}, {0b00101100, 8}, {0b00101101, 8}, {0b00000100, 8}, {0b00000101, 8}, {0b00001010, 8},
    {0b00001011, 8}, {0b01010010, 8}, {0b01010011, 8}, {0b01010100, 8}, {0b01010101, 8}, {0b00100100, 8}, {0b00100101, 8}, {0b01011000, 8},
    {0b01011001, 8}, {0b01011010, 8}, {0b01011011, 8}, {0b01001010, 8}, {0b01001011, 8}, {0b00110010, 8}, {0b00110011, 8}, {0b00110100, 8},
};
const Code kWhiteMake[27] = {  // 64, 128 .. 1728
    {0b11011, 5},     {0b10010, 5},     {0b010111, 6},    {0b0110111, 7},   {0b00110110, 8},  {0b00110111, 8},  {0b01100100, 8},
    {0b01100101, 8},  {0b01101000, 8},  {0b01100111, 8},  {0b011001100, 9}, {0b011001101, 9}, {0b011010010, 9}, {0b011010011, 9},
    {0b011010100, 9}, {0b011010101, 9}, {0b011010110, 9}, {0b011010111, 9}, {0b011011000, 9}, {0b011011001, 9}, {0b011011010, 9},
    {0b011011011, 9}, {0b010011000, 9}, {0b010011001, 9}, {0b010011010, 9}, {0b011000, 6},    {0b010011011, 9},
};
const Code kBlackTerm[64] = {
    {0b0000110111, 10},   {0b010, 3},           {0b11, 2},            {0b10, 2},            {0b011, 3},           {0b0011, 4},
    {0b0010, 4},          {0b00011, 5},         {0b000101, 6},        {0b000100, 6},        {0b0000100, 7},       {0b0000101, 7},
    {0b0000111, 7},       {0b00000100, 8},      {0b00000111, 8},      {0b000011000, 9},     {0b0000010111, 10},   {0b0000011000, 10},
    {0b0000001000, 10},   {0b00001100111, 11},  {0b00001101000, 11},  {0b00001101100, 11},  {0b00000110111, 11},  {0b00000101000, 11},
    {0b00000010111, 11},  {0b00000011000, 11},  {0b000011001010, 12}, {0b000011001011, 12}, {0b000011001100, 12}, {0b000011001101, 12},
    {0b000001101000, 12}, {0b000001101001, 12}, {0b000001101010, 12}, {0b000001101011, 12}, {0b000011010010, 12}, {0b000011010011, 12},
    {0b000011010100, 12}, {0b000011010101, 12}, {0b000011010110, 12}, {0b000011010111, 12}, {0b000001101100, 12}, {0b000001101101, 12},
    {0b000011011010, 12}, {0b000011011011, 12}, {0b000001010100, 12}, {0b000001010101, 12}, {0b000001010110, 12}, {0b000001010111, 12},
    {0b000001100100, 12}, {0b000001100101, 12}, {0b000001010010, 12}, {0b000001010011, 12}, {0b000000100100, 12}, {0b000000110111, 12},
    {0b000000111000, 12}, {0b000000100111, 12}, {0b000000101000, 12}, {0b000001011000, 12}, {0b000001011001, 12}, {0b000000101011, 12},
    {0b000000101100, 12}, {0b000001011010, 12}, {0b000001100110, 12}, {0b000001100111, 12},
};
const Code kBlackMake[27] = {  // 64, 128 .. 1728
    {0b0000001111, 10},    {0b000011001000, 12},  {0b000011001001, 12},  {0b000001011011, 12},  {0b000000110011, 12},
    {0b000000110100, 12},  {0b000000110101, 12},  {0b0000001101100, 13}, {0b0000001101101, 13}, {0b0000001001010, 13},
    {0b0000001001011, 13}, {0b0000001001100, 13}, {0b0000001001101, 13}, {0b0000001110010, 13}, {0b0000001110011, 13},
    {0b0000001110100, 13}, {0b0000001110101, 13}, {0b0000001110110, 13}, {0b0000001110111, 13}, {0b0000001010010, 13},
    {0b0000001010011, 13}, {0b0000001010100, 13}, {0b0000001010101, 13}, {0b0000001011010, 13}, {0b0000001011011, 13},
    {0b0000001100100, 13}, {0b0000001100101, 13},
};
const Code kExtMake[13] = {  // 1792, 1856 .. 2560, either colour
    {0b00000001000, 11},  {0b00000001100, 11},  {0b00000001101, 11},  {0b000000010010, 12}, {0b000000010011, 12},
    {0b000000010100, 12}, {0b000000010101, 12}, {0b000000010110, 12}, {0b000000010111, 12}, {0b000000011100, 12},
    {0b000000011101, 12}, {0b000000011110, 12}, {0b000000011111, 12},
};

uint32_t rd16(const uint8_t *p, bool be) { return be ? (uint32_t)p[0] << 8 | p[1] : (uint32_t)p[1] << 8 | p[0]; }
uint32_t rd32(const uint8_t *p, bool be)
{
    return be ? (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]
              : (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0];
}

int64_t row_bytes_of(const TdecHeader &h) { return h.bits_per_sample == 8 ? (int64_t)h.cols * h.samples : ((int64_t)h.cols + 7) / 8; }

}  // namespace

void omr::tdec_code_tables(int black, int32_t *run, int32_t *code, int32_t *bits)
{
    const Code *term = black ? kBlackTerm : kWhiteTerm, *make = black ? kBlackMake : kWhiteMake;
    int k = 0;
    for (int i = 0; i < 64; i++, k++) run[k] = i, code[k] = term[i].code, bits[k] = term[i].bits;
    for (int i = 0; i < 27; i++, k++) run[k] = 64 * (i + 1), code[k] = make[i].code, bits[k] = make[i].bits;
    for (int i = 0; i < 13; i++, k++) run[k] = 1792 + 64 * i, code[k] = kExtMake[i].code, bits[k] = kExtMake[i].bits;
}

bool omr::tdec_is_tiff(const uint8_t *s, int64_t len)
{
    return len >= 4 && ((s[0] == 'I' && s[1] == 'I' && s[2] == 42 && s[3] == 0) || (s[0] == 'M' && s[1] == 'M' && s[2] == 0 && s[3] == 42));
}

int omr::tdec_parse(const uint8_t *s, int64_t len, TdecHeader *h)
{
    *h = TdecHeader();
    if (len < 4 || !((s[0] == 'I' && s[1] == 'I') || (s[0] == 'M' && s[1] == 'M')))
        return fail(OMR_ERR_BADARG, "not a TIFF stream: no byte-order mark");
    const bool be = s[0] == 'M';
    const uint32_t magic = rd16(s + 2, be);
    if (magic == 43) return fail(OMR_ERR_NOTIMPL, "BigTIFF is not implemented");
    if (magic != 42) return fail(OMR_ERR_BADARG, "not a TIFF stream: version %u", magic);
    if (len < 8) return fail(OMR_ERR_BADARG, "the stream is too short for a TIFF header");
    const int64_t ifd = rd32(s + 4, be);
    if (ifd < 8 || ifd + 2 > len) return fail(OMR_ERR_BADARG, "the first IFD (byte %lld) lies outside the stream", (long long)ifd);
    const int64_t entries = rd16(s + ifd, be);
    if (entries == 0 || ifd + 2 + 12 * entries > len) return fail(OMR_ERR_BADARG, "the first IFD's %lld entries run past the end", (long long)entries);

    bool have_cols = false, have_rows = false, tiles = false, extra = false;
    int64_t bps = 1, bps_count = 1, spp = 1, planar = 1, t6opt = 0, rps = 0xffffffffll, predictor = 1;
    // StripOffsets / StripByteCounts: where the values stand, their type and count
    int64_t arr_at[2] = {-1, -1}, arr_n[2] = {0, 0};
    int arr_size[2] = {0, 0};
    for (int64_t e = 0; e < entries; e++) {
        const uint8_t *p = s + ifd + 2 + 12 * e;
        const uint32_t tag = rd16(p, be), type = rd16(p + 2, be);
        const int64_t count = rd32(p + 4, be);
        if (tag >= 322 && tag <= 325) {  // TileWidth, TileLength, TileOffsets, TileByteCounts
            tiles = true;
            continue;
        }
        if (tag == 338) {  // ExtraSamples
            extra = true;
            continue;
        }
        const bool known = tag == 256 || tag == 257 || tag == 258 || tag == 259 || tag == 262 || tag == 266 || tag == 273 ||
                           tag == 274 || tag == 277 || tag == 278 || tag == 279 || tag == 284 || tag == 293 || tag == 317;
        if (!known) continue;
        const int size = type == 3 ? 2 : type == 4 ? 4 : type == 1 ? 1 : 0;
        if (size == 0 || (size == 1 && tag != 258)) return fail(OMR_ERR_BADARG, "tag %u has type %u (SHORT or LONG expected)", tag, type);
        if (count < 1) return fail(OMR_ERR_BADARG, "tag %u has no value", tag);
        int64_t at = ifd + 2 + 12 * e + 8;  // inline
        if (count * size > 4) {
            at = rd32(p + 8, be);
            if (at < 8 || at > len || count * size > len - at)
                return fail(OMR_ERR_BADARG, "the values of tag %u (byte %lld, %lld of them) lie outside the stream", tag, (long long)at, (long long)count);
        }
        const int64_t v = size == 2 ? rd16(s + at, be) : size == 4 ? rd32(s + at, be) : s[at];
        if (tag == 273 || tag == 279) {
            const int k = tag == 279;
            arr_at[k] = at, arr_n[k] = count, arr_size[k] = size;
            continue;
        }
        if (tag == 258 || tag == 277) {  // one value per sample
            if (tag == 258) bps = v, bps_count = count;
            else spp = v;
            if (tag == 258 && count == 3) {  // the three must agree
                for (int k = 1; k < 3; k++)
                    if ((size == 2 ? (int64_t)rd16(s + at + 2 * k, be) : size == 4 ? (int64_t)rd32(s + at + 4 * k, be) : (int64_t)s[at + k]) != v) bps = -1;
            } else if (tag == 258 && count != 1) {
                bps = -1;
            }
            continue;
        }
        if (count != 1) return fail(OMR_ERR_BADARG, "tag %u has %lld values", tag, (long long)count);
        switch (tag) {
        case 256: h->cols = (int32_t)std::min<int64_t>(v, 0x7fffffff), have_cols = true; break;
        case 257: h->rows = (int32_t)std::min<int64_t>(v, 0x7fffffff), have_rows = true; break;
        case 259: h->compression = (int32_t)v; break;
        case 262: h->photometric = (int32_t)v; break;
        case 266: h->fill_order = (int32_t)v; break;
        case 274: h->orient = (int32_t)v; break;
        case 278: rps = v; break;
        case 284: planar = v; break;
        case 293: t6opt = v; break;
        case 317: predictor = v; break;
        }
    }
    if (tiles) return fail(OMR_ERR_NOTIMPL, "tiled TIFF is not implemented");
    if (extra) return fail(OMR_ERR_NOTIMPL, "ExtraSamples (alpha or other extra samples) are not implemented");
    if (bps != 1 && bps != 8) return fail(OMR_ERR_NOTIMPL, "BitsPerSample other than 1 and 8 (the same for every sample) is not implemented");
    if (planar != 1 && spp > 1) return fail(OMR_ERR_NOTIMPL, "PlanarConfiguration 2 with %lld samples is not implemented", (long long)spp);
    if (spp != 1 && spp != 3) return fail(OMR_ERR_NOTIMPL, "SamplesPerPixel %lld is not implemented (1 and 3 are)", (long long)spp);
    if (spp == 3 && (bps != 8 || bps_count != 3)) return fail(OMR_ERR_NOTIMPL, "three samples are implemented with BitsPerSample 8,8,8 alone");
    if (spp == 1 && bps_count != 1) return fail(OMR_ERR_NOTIMPL, "%lld values of BitsPerSample for one sample", (long long)bps_count);
    if (h->compression != TDEC_COMP_NONE && h->compression != TDEC_COMP_PACKBITS && h->compression != TDEC_COMP_T6 && h->compression != TDEC_COMP_LZW)
        return fail(OMR_ERR_NOTIMPL, "Compression %d is not implemented (1, 4, 5 and 32773 are)", h->compression);
    if (h->compression == TDEC_COMP_T6 && bps != 1) return fail(OMR_ERR_NOTIMPL, "Compression 4 (T.6) is implemented at 1 bit alone");
    if (h->compression == TDEC_COMP_LZW && bps != 8) return fail(OMR_ERR_NOTIMPL, "Compression 5 (LZW) is implemented at 8 bits alone");
    if (spp == 3 ? h->photometric != 2 : (h->photometric != 0 && h->photometric != 1))
        return fail(OMR_ERR_NOTIMPL, "Photometric %d with %lld samples is not implemented (0 and 1 with one sample, 2 with three; -1: the tag is missing)",
                    h->photometric, (long long)spp);
    if (h->fill_order != 1 && h->fill_order != 2) return fail(OMR_ERR_BADARG, "FillOrder %d (1 or 2)", h->fill_order);
    if (h->fill_order == 2 && bps == 8) return fail(OMR_ERR_NOTIMPL, "FillOrder 2 at 8 bits is not implemented");
    // libtiff knows the tag with LZW and Deflate alone and reads a raw or PackBits file that carries it as if it did not
    if (h->compression == TDEC_COMP_LZW && predictor != 1 && predictor != 2)
        return fail(OMR_ERR_NOTIMPL, "Predictor %lld is not implemented (1 and 2 are)", (long long)predictor);
    h->bits_per_sample = (int32_t)bps, h->samples = (int32_t)spp;
    h->predictor = h->compression == TDEC_COMP_LZW ? (int32_t)predictor : 1;
    if (h->compression == TDEC_COMP_T6 && (t6opt & 2)) return fail(OMR_ERR_NOTIMPL, "T6Options bit 1 (uncompressed mode) is not implemented");
    if (h->compression == TDEC_COMP_T6 && t6opt) return fail(OMR_ERR_BADARG, "T6Options %lld (0 expected)", (long long)t6opt);
    if (h->orient != 1)
        return fail(OMR_ERR_NOTIMPL, "Orientation %d is not implemented (what imread does with it is not established)", h->orient);
    if (!have_cols || !have_rows || h->cols < 1 || h->rows < 1) return fail(OMR_ERR_BADARG, "ImageWidth / ImageLength missing or 0");
    // OpenCV's imread fails above these; they also keep every count of the kernels inside 32 bits
    if (h->cols > TDEC_MAX_SIDE || h->rows > TDEC_MAX_SIDE || (int64_t)h->rows * h->cols > TDEC_MAX_PIXELS)
        return fail(OMR_ERR_ASSERT, "%d x %d is above imread's limits (2^20 a side, 2^30 pixels): not supported", h->rows, h->cols);
    if (h->compression == TDEC_COMP_T6 && h->cols > TDEC_T6_MAX_COLS)
        return fail(OMR_ERR_NOTIMPL, "a T.6 image of %d columns is not implemented (%d at the most)", h->cols, TDEC_T6_MAX_COLS);
    if (rps < 1) return fail(OMR_ERR_BADARG, "RowsPerStrip 0");
    h->rows_per_strip = (int32_t)std::min<int64_t>(rps, h->rows);
    const int64_t nstrips = ((int64_t)h->rows + h->rows_per_strip - 1) / h->rows_per_strip;
    if (arr_at[0] < 0) return fail(OMR_ERR_BADARG, "StripOffsets missing");
    // StripByteCounts may be missing (old writers): a strip then runs to the next strip offset above its own, the last
    // one in the file to the stream's end, as libtiff estimates it.  A present tag is taken at its word.
    const bool have_counts = arr_at[1] >= 0;
    if (arr_n[0] != nstrips || (have_counts && arr_n[1] != nstrips))
        return fail(OMR_ERR_BADARG, "%lld strip offsets and %lld byte counts for %lld strips of %d rows", (long long)arr_n[0],
                    (long long)arr_n[1], (long long)nstrips, h->rows_per_strip);
    auto offset_of = [&](int64_t k) -> int64_t { return arr_size[0] == 2 ? rd16(s + arr_at[0] + 2 * k, be) : rd32(s + arr_at[0] + 4 * k, be); };
    std::vector<int64_t> sorted;
    if (!have_counts) {
        sorted.resize((size_t)nstrips);
        for (int64_t k = 0; k < nstrips; k++) sorted[(size_t)k] = offset_of(k);
        std::sort(sorted.begin(), sorted.end());
    }
    h->strips.resize((size_t)nstrips);
    for (int64_t k = 0; k < nstrips; k++) {
        const int64_t off = offset_of(k);
        int64_t cnt;
        if (have_counts) {
            cnt = arr_size[1] == 2 ? rd16(s + arr_at[1] + 2 * k, be) : rd32(s + arr_at[1] + 4 * k, be);
        } else {
            const auto next = std::upper_bound(sorted.begin(), sorted.end(), off);
            cnt = (next == sorted.end() ? len : *next) - off;  // < 1 or past the end where off is: refused below
        }
        if (cnt < 1 || off < 8 || off > len || cnt > len - off)
            return fail(OMR_ERR_BADARG, "strip %lld (byte %lld, %lld bytes) lies outside the stream", (long long)k, (long long)off, (long long)cnt);
        if (cnt >= ((int64_t)1 << 28)) return fail(OMR_ERR_ASSERT, "a strip of 2^28 bytes or more: not supported");
        const int64_t srows = std::min<int64_t>(h->rows_per_strip, h->rows - k * h->rows_per_strip);
        if (h->compression == TDEC_COMP_LZW) {
            // libtiff takes a strip that begins 00 with the low bit of the next byte set for the old LZW, least significant bit first
            if (cnt >= 2 && s[off] == 0 && (s[off + 1] & 1)) return fail(OMR_ERR_NOTIMPL, "strip %lld is old-style LZW: not implemented", (long long)k);
            if (srows * row_bytes_of(*h) >= ((int64_t)1 << 31))
                return fail(OMR_ERR_ASSERT, "an LZW strip of 2^31 bytes of rows or more: not supported");
        }
        if (h->compression == TDEC_COMP_NONE && cnt < srows * row_bytes_of(*h))
            return fail(OMR_ERR_BADARG, "strip %lld holds %lld bytes, its %lld rows need %lld", (long long)k, (long long)cnt, (long long)srows,
                        (long long)(srows * row_bytes_of(*h)));
        h->strips[(size_t)k] = TdecPiece{off, (uint32_t)cnt};
    }
    return OMR_OK;
}

#ifndef TDEC_PARSER_ONLY

namespace {

constexpr int64_t kGroupRaw = (int64_t)1 << 30;    // packed rows of one group of launches
constexpr int64_t kGroupBytes = (int64_t)1 << 30;  // strips of one group
constexpr int kGroupImages = 4096;                 // the unpack kernel's grid takes 65535

constexpr size_t kLutBytes = sizeof(uint16_t) * 2 * ((size_t)1 << TDEC_LUT_BITS);

// the next 13 bits -> length << 12 | run for every code of both colours (white first), 0 where no code begins
const std::vector<uint16_t> &lut()
{
    static const std::vector<uint16_t> t = [] {
        std::vector<uint16_t> v((size_t)2 << TDEC_LUT_BITS, 0);
        int32_t run[TDEC_CODES], code[TDEC_CODES], bits[TDEC_CODES];
        for (int c = 0; c < 2; c++) {
            tdec_code_tables(c, run, code, bits);
            for (int k = 0; k < TDEC_CODES; k++) {
                const int rest = TDEC_LUT_BITS - bits[k];
                for (int f = 0; f < (1 << rest); f++)
                    v[((size_t)c << TDEC_LUT_BITS) + ((size_t)code[k] << rest) + (size_t)f] = (uint16_t)(bits[k] << 12 | run[k]);
            }
        }
        return v;
    }();
    return t;
}

int64_t raw_bytes_of(const TdecHeader &h)
{
    if (h.compression == TDEC_COMP_NONE) return 0;
    const int64_t pitch = h.compression == TDEC_COMP_T6 ? (((int64_t)h.cols + 31) / 32) * 4 : row_bytes_of(h);
    return pitch * h.rows;
}

int64_t src_bytes_of(const TdecHeader &h)
{
    int64_t b = 0;
    for (const TdecPiece &pc : h.strips) b += (int64_t)up16(pc.len);
    return b;
}

// one group: images idx[0 .. g)
int decode_group(const uint8_t *const *streams, const TdecHeader *hdr, const int *idx, int g, int channels, uint8_t *d_out,
                 int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s)
{
    // the host objects that asynchronous copies read or write stand before the drain
    std::vector<TdecImg> im((size_t)g);
    std::vector<TdecDyn> dyn((size_t)g);
    std::vector<TdecStrip> strips[3];  // PackBits, T.6, LZW
    std::vector<uint8_t> host;
    DrainOnExit drain{s};
    StageTimer<TDEC_STAGES> ev;
    if (int r = ev.begin(tdec_stats().on)) return r;
    // the uploaded bytes: the lookup table, then every strip at a multiple of 16 (a Compression 1 image: its rows in a row)
    size_t src_bytes = up16(kLutBytes), raw_bytes = 0;
    int max_rows[2] = {0, 0};  // of the bilevel images, of the 8-bit ones
    std::vector<size_t> first((size_t)g);  // an image's first strip in the uploaded bytes
    for (int j = 0; j < g; j++) {
        const TdecHeader &h = hdr[idx[j]];
        TdecImg &m = im[(size_t)j];
        memset(&m, 0, sizeof m);
        const int32_t rb = (int32_t)row_bytes_of(h);
        m.out_off = (int64_t)idx[j] * out_stride;
        m.rows = h.rows, m.cols = h.cols, m.invert = h.photometric == 0;
        m.depth = h.bits_per_sample, m.samples = h.samples, m.predictor = h.predictor;
        max_rows[h.bits_per_sample == 8] = std::max(max_rows[h.bits_per_sample == 8], h.rows);
        first[(size_t)j] = src_bytes;
        if (h.compression == TDEC_COMP_NONE) {
            m.bits_off = (int64_t)src_bytes, m.pitch = rb, m.from_src = 1, m.lsb = h.fill_order == 2;  // 8 bits: FillOrder 1 (the parser)
            src_bytes += up16((size_t)rb * (size_t)h.rows);
            continue;
        }
        const bool t6 = h.compression == TDEC_COMP_T6;
        m.bits_off = (int64_t)raw_bytes, m.pitch = t6 ? ((h.cols + 31) / 32) * 4 : rb;
        for (size_t k = 0; k < h.strips.size(); k++) {
            const int32_t row0 = (int32_t)k * h.rows_per_strip;
            TdecStrip st;
            memset(&st, 0, sizeof st);
            st.src_off = (int64_t)src_bytes, st.src_len = h.strips[k].len;
            st.dst_off = m.bits_off + (int64_t)row0 * m.pitch;
            st.img = j, st.rows = std::min(h.rows_per_strip, h.rows - row0), st.cols = h.cols, st.pitch = m.pitch;
            st.lsb = h.fill_order == 2;
            strips[t6 ? 1 : h.compression == TDEC_COMP_LZW ? 2 : 0].push_back(st);
            src_bytes += up16(st.src_len);
        }
        raw_bytes += up16((size_t)m.pitch * (size_t)h.rows);
    }
    host.assign(src_bytes, 0);
    memcpy(host.data(), lut().data(), kLutBytes);
    int r = on_threads(g, [&](hipStream_t, int lo, int hi) -> int {
        for (int j = lo; j < hi; j++) {
            const uint8_t *st = streams[idx[j]];
            const TdecHeader &h = hdr[idx[j]];
            uint8_t *to = host.data() + first[(size_t)j];
            const size_t rb = (size_t)row_bytes_of(h);
            for (size_t k = 0; k < h.strips.size(); k++) {
                if (h.compression == TDEC_COMP_NONE) {  // the strip's rows; bytes behind them are not the image's
                    const size_t srows = (size_t)std::min<int64_t>(h.rows_per_strip, h.rows - (int64_t)k * h.rows_per_strip);
                    memcpy(to, st + h.strips[k].off, srows * rb), to += srows * rb;
                } else {
                    memcpy(to, st + h.strips[k].off, h.strips[k].len), to += up16(h.strips[k].len);
                }
            }
        }
        return OMR_OK;
    });
    if (r) return r;
    const size_t np = strips[0].size(), nt = strips[1].size(), nl = strips[2].size();
    std::vector<TdecStrip> all(strips[0]);
    all.insert(all.end(), strips[1].begin(), strips[1].end());
    all.insert(all.end(), strips[2].begin(), strips[2].end());
    DevBuf d_src, d_im, d_dyn, d_strips, raw;
    OMR_HIP(d_src.alloc(src_bytes));
    OMR_HIP(d_im.alloc(sizeof(TdecImg) * (size_t)g));
    OMR_HIP(d_dyn.alloc(sizeof(TdecDyn) * (size_t)g));
    OMR_HIP(d_strips.alloc(sizeof(TdecStrip) * std::max<size_t>(all.size(), 1)));
    OMR_HIP(raw.alloc(std::max<size_t>(raw_bytes, 16)));
    TdecPass p;
    memset(&p, 0, sizeof p);
    p.src = d_src.as<uint8_t>(), p.imgs = d_im.as<TdecImg>(), p.dyn = d_dyn.as<TdecDyn>(), p.raw = raw.as<uint8_t>();
    p.lut = d_src.as<uint16_t>();
    p.n = g, p.channels = channels, p.out = d_out, p.step = step;
    if ((r = ev.mark(0, s))) return r;
    OMR_HIP(hipMemcpyAsync(d_src.p, host.data(), src_bytes, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(TdecImg) * (size_t)g, hipMemcpyHostToDevice, s));
    if (!all.empty()) OMR_HIP(hipMemcpyAsync(d_strips.p, all.data(), sizeof(TdecStrip) * all.size(), hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemsetAsync(d_dyn.p, 0, sizeof(TdecDyn) * (size_t)g, s));
    if ((r = ev.mark(1, s)) || (r = tdec_launch_packbits(p, d_strips.as<TdecStrip>(), (int)np, s)) || (r = ev.mark(2, s)) ||
        (r = tdec_launch_t6(p, d_strips.as<TdecStrip>() + np, (int)nt, s)) || (r = ev.mark(3, s)) ||
        (r = tdec_launch_lzw(p, d_strips.as<TdecStrip>() + np + nt, (int)nl, s)) || (r = ev.mark(4, s)) || (r = tdec_launch_unpack(p, max_rows[0], s)) ||
        (r = ev.mark(5, s)) || (r = tdec_launch_finish8(p, max_rows[1], s)) || (r = ev.mark(6, s)))
        return r;
    OMR_HIP(hipMemcpyAsync(dyn.data(), d_dyn.p, sizeof(TdecDyn) * (size_t)g, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    if ((r = ev.finish(tdec_stats()))) return r;
    for (int j = 0; j < g; j++)
        if (dyn[(size_t)j].err) rc[idx[j]] = OMR_ERR_ASSERT;
    return OMR_OK;
}

}  // namespace

TdecStats &omr::tdec_stats() { return thread_stats<TdecStats>(); }

int omr::tdec_check_channels(const TdecHeader &h, int channels)
{
    if (channels == 1 && h.samples == 3)
        return fail(OMR_ERR_NOTIMPL, "a gray image from an RGB stream is not implemented (the gray weights of imread's TIFF reader are not established)");
    return OMR_OK;
}

int omr::tiff_decode_device(const uint8_t *const *streams, const int64_t *, const TdecHeader *hdr, const int32_t *skip, int n,
                            int channels, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s)
{
    tdec_stats().begin_call();
    DrainOnExit drain{s};
    return for_each_group(
        n, skip, kGroupImages, kGroupRaw, kGroupBytes,
        [&](int i) {
            const int64_t by = hdr[i].compression == TDEC_COMP_NONE ? row_bytes_of(hdr[i]) * hdr[i].rows : src_bytes_of(hdr[i]);
            return GroupCost{raw_bytes_of(hdr[i]), by, true};
        },
        [&](const int *idx, int g) { return decode_group(streams, hdr, idx, g, channels, d_out, out_stride, step, rc, s); });
}

extern "C" {

int omr_tiff_info(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *compression, int32_t *photometric,
                  int32_t *fill_order, int32_t *strips)
{
    clear_error();
    if (!stream || len < 0) return fail(OMR_ERR_BADARG, "null stream");
    TdecHeader h;
    const int rc = tdec_parse(stream, len, &h);
    if (rows) *rows = h.rows;
    if (cols) *cols = h.cols;
    if (compression) *compression = h.compression;
    if (photometric) *photometric = h.photometric;
    if (fill_order) *fill_order = h.fill_order;
    if (strips) *strips = (int32_t)h.strips.size();
    return rc;
}

int omr_tiff_info_ex(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *compression, int32_t *photometric,
                     int32_t *fill_order, int32_t *strips, int32_t *bits_per_sample, int32_t *samples_per_pixel, int32_t *predictor)
{
    clear_error();
    if (!stream || len < 0) return fail(OMR_ERR_BADARG, "null stream");
    TdecHeader h;
    const int rc = tdec_parse(stream, len, &h);
    if (rows) *rows = h.rows;
    if (cols) *cols = h.cols;
    if (compression) *compression = h.compression;
    if (photometric) *photometric = h.photometric;
    if (fill_order) *fill_order = h.fill_order;
    if (strips) *strips = (int32_t)h.strips.size();
    if (bits_per_sample) *bits_per_sample = h.bits_per_sample;
    if (samples_per_pixel) *samples_per_pixel = h.samples;
    if (predictor) *predictor = h.predictor;
    return rc;
}

int omr_tiff_code_tables(int32_t black, int32_t *run, int32_t *code, int32_t *bits)
{
    clear_error();
    if (!run || !code || !bits) return fail(OMR_ERR_BADARG, "null argument");
    if (black != 0 && black != 1) return fail(OMR_ERR_BADARG, "black is 0 or 1, got %d", black);
    tdec_code_tables(black, run, code, bits);
    return OMR_OK;
}

int omr_tiff_decode_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels, uint8_t *d_out,
                                 int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols, int32_t *out_size,
                                 int32_t *rc)
{
    std::vector<TdecHeader> hdr;
    return decode_batch_entry(
        BatchDecodeArgs{streams, len, n, channels, d_out, out_stride_bytes, step_bytes, rows, cols, out_size, rc},
        "stream %d is %d x %d, the slot %d x %d", no_extra_check, [&](size_t cnt) { hdr.reserve(cnt); },
        [&](int i) {
            hdr.emplace_back();
            int r = tdec_parse(streams[i], len[i], &hdr.back());
            if (r == OMR_OK) r = tdec_check_channels(hdr.back(), channels);
            return ParsedSize{r, hdr.back().rows, hdr.back().cols};
        },
        [&](const int32_t *skip, hipStream_t s) {
            return tiff_decode_device(streams, len, hdr.data(), skip, n, channels, d_out, out_stride_bytes, step_bytes, rc, s);
        });
}

int omr_tiff_decode_stats(int32_t enable, int32_t *groups, double *stage_ms)
{
    clear_error();
    TdecStats &st = tdec_stats();
    if (groups) *groups = st.groups;
    const int four[4] = {0, 1, 2, 4};  // upload, PackBits, T.6, unpack: the stages this call has always reported
    if (stage_ms)
        for (int k = 0; k < 4; k++) stage_ms[k] = st.ms[four[k]];
    st.on = enable != 0;
    return OMR_OK;
}

int omr_tiff_decode_stats_ex(int32_t enable, int32_t *groups, double *stage_ms, int32_t capacity, int32_t *stages)
{
    clear_error();
    if (capacity < 0 || (capacity > 0 && !stage_ms)) return fail(OMR_ERR_BADARG, "capacity %d with %s stage_ms", capacity, stage_ms ? "a" : "a null");
    tdec_stats().report(enable, groups, stage_ms, std::min<int>(capacity, TDEC_STAGES));
    if (stages) *stages = TDEC_STAGES;
    return OMR_OK;
}

int omr_tiff_decode(const uint8_t *stream, int64_t len, int32_t channels, omr_image_owned *dst)
{
    TdecHeader h;
    const int32_t skip = 0;
    return decode_one_entry(
        stream, len, channels, dst,
        "the image data is damaged (an invalid code, a run past the row's or the strip's end, a full LZW table, or input that ends early)",
        no_extra_check,
        [&] {
            int r = tdec_parse(stream, len, &h);
            if (r == OMR_OK) r = tdec_check_channels(h, channels);
            return ParsedSize{r, h.rows, h.cols};
        },
        [&](uint8_t *d_out, int64_t stride, int64_t step, int32_t *rc, hipStream_t s) {
            return tiff_decode_device(&stream, &len, &h, &skip, 1, channels, d_out, stride, step, rc, s);
        });
}

}  // extern "C"

#endif  // TDEC_PARSER_ONLY
