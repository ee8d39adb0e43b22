// png_enc.hpp -- the PNG encoder's device side (png_enc.hip) as oics_png_enc.cpp sees it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "codec_stats.hpp"
#include "jpeg.hpp"  // JpegSink: where a group's streams go (the protocol is the JPEG encoder's: place, then done)

namespace omr {

constexpr int PENC_PIECE = 512;          // raw bytes one lane parses; a match is cut at a piece's end
constexpr int PENC_BLOCK_PIECES = 32;    // pieces of a deflate block
constexpr int PENC_BLOCK = PENC_PIECE * PENC_BLOCK_PIECES;  // 16384 raw bytes (<= 65535: a stored block always holds them)
constexpr int PENC_STORED_HEAD = 5;      // a stored block's header byte, LEN and NLEN
constexpr int PENC_ZBLOCK = PENC_BLOCK + 8;  // a block's region in the bit buffer: its bytes (<= 5 + PENC_BLOCK), dword aligned
constexpr int PENC_CODES = 286 + 30;     // code table of a block: literal / length symbols, then distance symbols
constexpr int PENC_HDR_WORDS = 144;      // a dynamic block's header: <= 17 + 19 x 3 + 316 x 14 = 4498 bits
constexpr int PENC_MAX_DISTANCE = 32768;
constexpr int PENC_BEFORE = 8 + 25 + 8 + 2;  // signature, IHDR, IDAT's length and type, the zlib header
constexpr int PENC_AFTER = 4 + 4 + 12;       // Adler-32, IDAT's CRC, IEND
constexpr int PENC_MAX_SIDE = 1 << 20;       // imread's own limits, as the decoder's
constexpr int64_t PENC_MAX_PIXELS = (int64_t)1 << 30;
// offsets inside one image (raw bytes, tokens, bits of a block, bytes of the deflate stream) are 32-bit; PNG's chunk
// length is below 2^31
constexpr int64_t PENC_MAX_IDAT = ((int64_t)1 << 31) - 1;

// One image of a launch, filled on the host.
struct PencImg {
    int64_t src_off;   // of the image's first byte from the batch's base
    int64_t raw_off;   // its filtered bytes: rows x (1 + row_bytes), a multiple of 16; its match / token entries likewise
    int64_t out_off;   // of its stream from the output's base
    int64_t blk0;      // its first block among the launch's
    uint32_t raw_len;
    uint32_t nblk;     // ceil(raw_len / PENC_BLOCK)
    uint32_t npiece;   // ceil(raw_len / PENC_PIECE)
    int32_t rows, cols;
    int32_t row_bytes; // cols x channels
};

// what the device learns about an image
struct PencDyn {
    unsigned long long a_sum, b_sum;  // Adler-32's two sums (png_adler.hpp)
    uint32_t deflate_len;             // bytes of its deflate blocks
    uint32_t pad;
};

enum PencType : uint32_t { PENC_STORED = 0, PENC_FIXED = 1, PENC_DYNAMIC = 2 };

struct PencBlk {
    uint32_t type;
    uint32_t hdr_bits;   // BFINAL, BTYPE and a dynamic block's code sets
    uint32_t bits;       // header, tokens and the end-of-block code
    uint32_t nbytes;     // in the stream, the empty stored block behind it included
    uint32_t byte_off;   // in the image's deflate data
    uint32_t crc;        // crc_raw of its bytes (crc32_combine.hpp)
};

struct PencPass {
    const uint8_t *src;
    int64_t step;
    const PencImg *imgs;
    PencDyn *dyn;        // [n], cleared
    int n;
    int cn;
    int stored_only;     // compression 0
    uint8_t *raw;
    uint16_t *mt;        // [raw bytes]: per position the best match, then (in place) per piece its tokens
    uint16_t *piece_cnt; // [pieces] tokens
    uint32_t *piece_bit; // [pieces] bit offset of its tokens behind the block's header
    PencBlk *blk;        // [blocks]
    uint32_t *codes;     // [blocks][PENC_CODES] bit-reversed code | length << 16
    uint32_t *hdr;       // [blocks][PENC_HDR_WORDS]
    uint32_t *zbuf;      // [blocks][PENC_ZBLOCK / 4], cleared
    uint8_t *out;
};

// max_*: the largest image's rows, pieces, blocks
int penc_launch_filter(const PencPass &p, int max_rows, hipStream_t s);
int penc_launch_adler(const PencPass &p, int64_t max_raw, hipStream_t s);
int penc_launch_parse(const PencPass &p, int64_t max_raw, int max_pieces, hipStream_t s);   // matches, then tokens
int penc_launch_blocks(const PencPass &p, int max_blocks, hipStream_t s);                   // code sets, sizes, per-image scan
int penc_launch_bits(const PencPass &p, int max_blocks, hipStream_t s);
int penc_launch_streams(const PencPass &p, int max_blocks, hipStream_t s);                  // copy with CRC-32, then the wrap

// ---- host side (oics_png_enc.cpp)
// rows x (1 + cols x cn), the blocks of that, and the bound of a stream's length
int64_t penc_raw_bytes(int rows, int cols, int cn);
int64_t penc_bound(int rows, int cols, int cn);
// OMR_ERR_ASSERT for 2 channels, an empty image, a size above imread's limits or one whose IDAT chunk could exceed
// 2^31 - 1 bytes; host arithmetic, called by every entry point on its slot shape before any device work
int penc_check_shape(int rows, int cols, int cn);
// n images at d_imgs + i * img_stride, rows `step` apart, image i sizes[2 i] x sizes[2 i + 1] (0 x 0: skipped).  Pointers,
// pitches and channels already checked.  compression is clamped to 0 .. 9.  Synchronises `s`; its workspace comes from
// the calling thread's pool scope.
int png_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n,
                      int compression, JpegSink &sink, hipStream_t s);

constexpr int PENC_STAGES = 6;  // filter, Adler-32, matches and parse, code sets and placement, bit writer, copy + CRC-32 + wrap
struct PencStats : CodecStats<PENC_STAGES> {};
PencStats &penc_stats();

}  // namespace omr
