// png_dec.hpp -- the PNG decoder's device side (png_dec.hip) as oics_png_dec.cpp sees it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "codec_stats.hpp"

namespace omr {

constexpr int PDEC_WIN_WORDS = 1024;    // an image's input window in LDS, 32-bit words
constexpr int PDEC_RECORDS = 512;       // literal records and match records of one decode batch
constexpr int PDEC_MAX_SIDE = 1 << 20;        // rows and cols pdec_parse takes: imread's own limits
constexpr int64_t PDEC_MAX_PIXELS = (int64_t)1 << 30;
constexpr int PDEC_ADLER_CHUNK = 65536; // inflated bytes per workgroup of the Adler-32 kernel

// One image of a launch, filled on the host from its header.
struct PdecImg {
    int64_t src_off;    // its zlib stream (the IDAT payloads in a row) in the uploaded bytes, a multiple of 16
    int64_t raw_off;    // its inflated bytes: rows x (1 + row_bytes), a multiple of 16
    int64_t out_off;    // its slot in the output
    uint32_t src_len;
    uint32_t raw_len;
    int32_t rows, cols;
    int32_t color_type, depth;
    int32_t bpp;        // bytes the filters step by: max(1, samples per pixel x depth / 8)
    int32_t row_bytes;  // without the filter byte
    int32_t npal;       // palette entries
    int32_t skip;       // != 0: refused on the host behind the header (a chunk's CRC); no kernel touches it
    uint8_t pal[768];   // R G B per entry
};

// what the device learns about an image
struct PdecDyn {
    uint32_t err;          // != 0: damaged data (OMR_ERR_ASSERT); later kernels skip the image
    uint32_t out_len;      // bytes inflated
    uint32_t adler_want;   // the stream's trailer
    uint32_t pad;
    unsigned long long a_sum, b_sum;  // Adler-32's two sums, before the final modulo
};

enum PdecErr : uint32_t {
    PDEC_ERR_INPUT = 1,     // input running out
    PDEC_ERR_CODE = 2,      // an invalid code, code set or block type
    PDEC_ERR_DISTANCE = 4,  // a distance beyond the bytes produced so far
    PDEC_ERR_SIZE = 8,      // inflated data longer or shorter than the image needs
    PDEC_ERR_ADLER = 16,
    PDEC_ERR_FILTER = 32,   // a filter byte above 4
    PDEC_ERR_PALETTE = 64,  // a palette index beyond PLTE
};

struct PdecPass {
    const uint8_t *src;
    const PdecImg *imgs;
    PdecDyn *dyn;  // [n], cleared
    uint8_t *raw;
    int n;
    int channels;  // of the output: 1 or 3
    uint8_t *out;
    int64_t step;
};

int pdec_launch_inflate(const PdecPass &p, hipStream_t s);
// max_chunks: the largest image's PDEC_ADLER_CHUNK pieces
int pdec_launch_adler(const PdecPass &p, int max_chunks, hipStream_t s);
int pdec_launch_unfilter(const PdecPass &p, hipStream_t s);

// ---- host side (oics_png_dec.cpp)
// What a stream's chunks say.  pdec_parse returns 0, OMR_ERR_NOTIMPL, OMR_ERR_BADARG or OMR_ERR_ASSERT (no IEND, a size
// above imread's limits, raw data of 2^32 bytes or more) with the thread's error text set; the IHDR fields are filled whenever IHDR was readable.
struct PdecPiece {
    int64_t off;  // of an IDAT chunk's payload
    uint32_t len;
};
struct PdecHeader {
    int32_t rows = 0, cols = 0, color_type = 0, depth = 0;
    int32_t npal = 0;
    int32_t orient = 1;  // the eXIf chunk's orientation (1: none); anything else is refused
    uint8_t pal[768];
    std::vector<PdecPiece> idat;
    std::vector<PdecPiece> critical;  // every critical chunk from its type field on: type + payload, the CRC behind
    int64_t idat_bytes = 0;
};
bool pdec_is_png(const uint8_t *stream, int64_t len);
int pdec_parse(const uint8_t *stream, int64_t len, PdecHeader *h);
// OMR_ERR_NOTIMPL for a colour or paletted stream asked for as gray
int pdec_check_channels(const PdecHeader &h, int channels);
// n parsed streams (hdr[i]; skip[i] != 0: not decoded) into slots d_out + i * out_stride of `channels` channels, rows
// `step` apart; every image fits its slot and passes pdec_check_channels (checked by the caller).  rc[i] = OMR_ERR_ASSERT
// for damaged data.  Synchronises `s`; its workspace comes from the calling thread's pool scope.
int png_decode_device(const uint8_t *const *streams, const int64_t *len, const PdecHeader *hdr, const int32_t *skip, int n,
                      int channels, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s);
// the EXIF orientation of a TIFF block ("II*\0" / "MM\0*" first), or 1 (oics_jpeg_dec.cpp)
int exif_orientation_tiff(const uint8_t *tiff, int64_t n);

constexpr int PDEC_STAGES = 4;  // upload, inflate, Adler-32, unfilter and convert
struct PdecStats : CodecStats<PDEC_STAGES> {};
PdecStats &pdec_stats();

}  // namespace omr
