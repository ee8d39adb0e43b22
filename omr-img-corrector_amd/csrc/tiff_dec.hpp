// tiff_dec.hpp -- the TIFF decoder's device side (tiff_dec.hip: bilevel; tiff_dec8.hip: 8-bit gray
// and RGB, section 4.27) as oics_tiff_dec.cpp sees it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "codec_stats.hpp"

namespace omr {

constexpr int TDEC_MAX_SIDE = 1 << 20;  // rows and cols tdec_parse takes: imread's own limits
constexpr int64_t TDEC_MAX_PIXELS = (int64_t)1 << 30;
constexpr int TDEC_T6_MAX_COLS = 12288;  // a T.6 row's change positions, two lines of them, live in LDS as 16-bit values
constexpr int TDEC_T6_PAD = 8;           // sentinels behind a line's changes
constexpr int TDEC_WIN_BYTES = 8192;     // a strip's input window in LDS
constexpr int TDEC_LUT_BITS = 13;        // the longest run-length code
constexpr int TDEC_CODES = 104;          // per colour: 64 terminating, 27 make-up and 13 extended make-up codes

constexpr int TDEC_COMP_NONE = 1, TDEC_COMP_T6 = 4, TDEC_COMP_LZW = 5, TDEC_COMP_PACKBITS = 32773;

// One image of a launch, filled on the host from its header.
struct TdecImg {
    int64_t bits_off;  // its packed rows: in the uploaded bytes (Compression 1) or in the workspace (the other two)
    int64_t out_off;   // its slot in the output
    int32_t rows, cols;
    int32_t pitch;     // bytes from one packed row to the next
    int32_t from_src;  // != 0: bits_off counts in the uploaded bytes
    int32_t lsb;       // != 0: the packed rows' first pixel is bit 0 of a byte (FillOrder 2 without a decoder in front)
    int32_t invert;    // != 0: a set bit is black (Photometric 0); at depth 8: every sample is inverted
    int32_t depth;     // 1: tdec_unpack's image; 8: tdec_finish8's, its rows `samples` bytes a pixel
    int32_t samples;   // 1 or 3
    int32_t predictor; // 2: a row's samples are differences to the pixel on the left
};

// One strip of a launch of the PackBits, the T.6 or the LZW kernel.
struct TdecStrip {
    int64_t src_off;   // its bytes in the uploaded bytes
    int64_t dst_off;   // its first row in the workspace
    uint32_t src_len;
    int32_t img;       // whose it is: the index of dyn
    int32_t rows, cols;
    int32_t pitch;     // of the workspace rows
    int32_t lsb;       // FillOrder 2: every byte is read bit-reversed
};

struct TdecDyn {
    uint32_t err;  // != 0: damaged data (OMR_ERR_ASSERT); the unpack kernel skips the image
};

enum TdecErr : uint32_t {
    TDEC_ERR_INPUT = 1,  // input that ends before the strip's rows do
    TDEC_ERR_CODE = 2,   // an invalid code or an extension code
    TDEC_ERR_RUN = 4,    // a run past the row's end (T.6), past the strip's rows (PackBits) or one that does not advance
};

struct TdecPass {
    const uint8_t *src;
    const TdecImg *imgs;
    TdecDyn *dyn;  // [n], cleared
    uint8_t *raw;  // the workspace: packed rows
    const uint16_t *lut;  // [2][1 << TDEC_LUT_BITS]: the next 13 bits -> length << 12 | run, 0 for no code; white first
    int n;
    int channels;  // of the output: 1 or 3
    uint8_t *out;
    int64_t step;
};

int tdec_launch_packbits(const TdecPass &p, const TdecStrip *d_strips, int nstrips, hipStream_t s);
int tdec_launch_t6(const TdecPass &p, const TdecStrip *d_strips, int nstrips, hipStream_t s);
int tdec_launch_lzw(const TdecPass &p, const TdecStrip *d_strips, int nstrips, hipStream_t s);
// max_rows: the tallest image's of the kernel's depth
int tdec_launch_unpack(const TdecPass &p, int max_rows, hipStream_t s);
int tdec_launch_finish8(const TdecPass &p, int max_rows, hipStream_t s);

// ---- host side (oics_tiff_dec.cpp)
struct TdecPiece {
    int64_t off;  // of a strip's bytes
    uint32_t len;
};
// What the first IFD says.  tdec_parse returns 0, OMR_ERR_NOTIMPL, OMR_ERR_BADARG or OMR_ERR_ASSERT (a size above imread's
// limits, a strip of 2^28 bytes or more) with the thread's error text set; the fields are filled as far as the tags were
// readable.
struct TdecHeader {
    int32_t rows = 0, cols = 0;
    int32_t compression = 1, photometric = -1, fill_order = 1, orient = 1;
    int32_t rows_per_strip = 0;
    int32_t bits_per_sample = 1, samples = 1, predictor = 1;
    std::vector<TdecPiece> strips;
};
bool tdec_is_tiff(const uint8_t *stream, int64_t len);
int tdec_parse(const uint8_t *stream, int64_t len, TdecHeader *h);
// OMR_ERR_NOTIMPL for a gray image asked of an RGB stream (the PNG decoder's rule, pdec_check_channels), else 0
int tdec_check_channels(const TdecHeader &h, int channels);
// the run-length codes of ITU-T T.4 (Tables 2 and 3) for one colour, TDEC_CODES entries each
void tdec_code_tables(int black, int32_t *run, int32_t *code, int32_t *bits);
// n parsed streams (hdr[i]; skip[i] != 0: not decoded) into slots d_out + i * out_stride of `channels` channels, rows
// `step` apart; every image fits its slot (checked by the caller).  rc[i] = OMR_ERR_ASSERT for damaged data.  Synchronises
// `s`; its workspace comes from the calling thread's pool scope.
int tiff_decode_device(const uint8_t *const *streams, const int64_t *len, const TdecHeader *hdr, const int32_t *skip, int n,
                       int channels, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s);

constexpr int TDEC_STAGES = 6;  // upload, PackBits, T.6, LZW, unpack, finish8
struct TdecStats : CodecStats<TDEC_STAGES> {};
TdecStats &tdec_stats();

}  // namespace omr
