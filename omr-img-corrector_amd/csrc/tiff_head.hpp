// tiff_head.hpp -- the first bytes of a little-endian classic TIFF file with one IFD, as both TIFF encoders write them
// (oics_tiff_enc.cpp, oics_tiff_enc8.cpp; DESIGN.md sections 4.26 and 4.29): "II" 42, the IFD at 8 with its tags in ascending
// order, the next-IFD pointer 0, then the two resolutions (dpi > 0) and BitsPerSample's three values and two zeros (three
// samples).  Behind them, for more than one strip, stand StripOffsets' and StripByteCounts' arrays (LONG), then the strips,
// each at an even offset; the arrays' values are the device's to write.  Plain C++: nothing of HIP.
#pragma once
#include <stdint.h>
#include <string.h>

#pragma GCC visibility push(hidden)  // the library's own: not in the dynamic symbol table
namespace omr {

inline void le16(uint8_t *d, uint32_t v) { d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8); }
inline void le32(uint8_t *d, uint32_t v) { le16(d, v), le16(d + 2, v >> 16); }
inline int strips_of(int rows, int rps) { return (rows + rps - 1) / rps; }
inline int64_t even_offset(int64_t v) { return (v + 1) & ~(int64_t)1; }  // a strip ends, the next begins at an even offset

struct TiffHeadDesc {
    int rows, cols;
    int rps, ns;          // rows of a strip, strips
    int bits, samples;    // BitsPerSample (of every sample), SamplesPerPixel: 1 or 3
    int compression, photometric;
    int predictor;        // 2: the Predictor tag is written
    bool t6_options;      // T6Options (0) is written
    int dpi;              // > 0: XResolution, YResolution (dpi / 1) and ResolutionUnit (inch) are written
};

struct TiffHead {
    int head_len;          // bytes written
    int off_pos, cnt_pos;  // where StripOffsets' and StripByteCounts' values stand in the file
    int data_at;           // the file offset of the first strip
};

// tags of the IFD, and bytes of the head: what a writer holds its buffer to at compile time
constexpr int tiff_head_tags(bool res, bool rgb, bool t6_options, bool predictor2)
{
    return 9 + (res ? 3 : 0) + (rgb ? 1 : 0) + (t6_options ? 1 : 0) + (predictor2 ? 1 : 0);
}
constexpr int tiff_head_len(bool res, bool rgb, bool t6_options, bool predictor2)
{
    return 8 + 2 + 12 * tiff_head_tags(res, rgb, t6_options, predictor2) + 4 + (res ? 16 : 0) + (rgb ? 8 : 0);
}

// Writes the head into h[0 .. head_len), head_len = tiff_head_len of the description: the caller's buffer holds that much.
inline TiffHead tiff_head(const TiffHeadDesc &d, uint8_t *h)
{
    const bool res = d.dpi > 0, rgb = d.samples == 3;
    const int nt = tiff_head_tags(res, rgb, d.t6_options, d.predictor == 2);
    const int ifd_end = 8 + 2 + 12 * nt + 4;
    const int res_at = ifd_end, bps_at = res_at + (res ? 16 : 0), arrays_at = bps_at + (rgb ? 8 : 0);
    memset(h, 0, (size_t)arrays_at);
    h[0] = h[1] = 'I', le16(h + 2, 42), le32(h + 4, 8);
    le16(h + 8, (uint32_t)nt);
    uint8_t *e = h + 10;
    auto entry = [&](int tag, int type, uint32_t count, uint32_t value) {
        le16(e, (uint32_t)tag), le16(e + 2, (uint32_t)type), le32(e + 4, count);
        if (type == 3 && count == 1) le16(e + 8, value);
        else le32(e + 8, value);
        e += 12;
        return (int)(e - 4 - h);  // where the value stands
    };
    const uint32_t ns = (uint32_t)d.ns;
    entry(256, 4, 1, (uint32_t)d.cols);
    entry(257, 4, 1, (uint32_t)d.rows);
    if (rgb) entry(258, 3, 3, (uint32_t)bps_at);
    else entry(258, 3, 1, (uint32_t)d.bits);
    entry(259, 3, 1, (uint32_t)d.compression);
    entry(262, 3, 1, (uint32_t)d.photometric);
    const int off_in = entry(273, 4, ns, ns > 1 ? (uint32_t)arrays_at : 0);
    entry(277, 3, 1, (uint32_t)d.samples);
    entry(278, 4, 1, (uint32_t)d.rps);
    const int cnt_in = entry(279, 4, ns, ns > 1 ? (uint32_t)(arrays_at + 4 * ns) : 0);
    if (res) entry(282, 5, 1, (uint32_t)res_at), entry(283, 5, 1, (uint32_t)res_at + 8);
    if (rgb) entry(284, 3, 1, 1);
    if (d.t6_options) entry(293, 4, 1, 0);
    if (res) entry(296, 3, 1, 2);
    if (d.predictor == 2) entry(317, 3, 1, 2);
    if (res) le32(h + res_at, (uint32_t)d.dpi), le32(h + res_at + 4, 1), le32(h + res_at + 8, (uint32_t)d.dpi), le32(h + res_at + 12, 1);
    if (rgb) le16(h + bps_at, (uint32_t)d.bits), le16(h + bps_at + 2, (uint32_t)d.bits), le16(h + bps_at + 4, (uint32_t)d.bits);
    TiffHead r;
    r.head_len = arrays_at;
    r.off_pos = ns > 1 ? arrays_at : off_in;
    r.cnt_pos = ns > 1 ? arrays_at + 4 * (int)ns : cnt_in;
    r.data_at = arrays_at + (ns > 1 ? 8 * (int)ns : 0);
    return r;
}

}  // namespace omr
#pragma GCC visibility pop
