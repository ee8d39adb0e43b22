// jpeg.hpp -- the baseline JPEG encoder's device side (jpeg.hip) as oics_jpeg.cpp sees it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace omr {

constexpr int JPEG_TILE_W = 128, JPEG_TILE_H = 64;  // pixels a workgroup of the block kernel converts: 8 x 4 MCUs (BGR) or 16 x 8 blocks (gray)
constexpr int JPEG_CHUNK = 256;                     // blocks per workgroup of the DC / bit-writer kernels (one scan segment)
constexpr int JPEG_BYTE_CHUNK = 4096;               // unstuffed bytes per workgroup of the stuffing kernels
constexpr int JPEG_MAX_HEADER = 623;                // SOI .. SOS of a 3-component stream

// One image of a launch.  Filled on the host; the fields below `nchunk` after the block lengths have been summed.
struct JpegImg {
    int64_t src_off;   // of the image's first byte from the batch's base
    int64_t out_off;   // of its stream from the output's base
    int64_t bit_word;  // first dword of its bit buffer
    int32_t rows, cols;
    int32_t bw, bh;    // real Y blocks per row / column
    int32_t mw, mh;    // MCUs per row / column (gray: bw, bh)
    uint32_t blk0, nblk;      // its blocks in the launch's coefficient array, scan order
    uint32_t chunk0, nchunk;  // its JPEG_CHUNK segments
    uint32_t bits;            // code bits of the scan (< 2^32: the entry point refuses larger images)
    uint32_t nbytes;          // ceil(bits / 8)
    uint32_t bchunk0, nbchunk;  // its JPEG_BYTE_CHUNK segments
    uint32_t pad_;
};

// what the kernels look up: divisors (table entry x 8, natural order), code tables as (code << 8 | length)
struct JpegTables {
    uint16_t div[2][64];
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

struct JpegPass {
    const uint8_t *src;
    int64_t step;
    const JpegImg *imgs;
    int n;
    int cn;
    const JpegTables *tab;
    int16_t *coef;       // [blocks][64] zig-zag
    uint16_t *aclen;     // [blocks] bits of the AC codes
    int16_t *dcdiff;     // [blocks]
    uint32_t *local;     // [blocks] bit offset inside the block's segment
    uint32_t *chunk_sum, *chunk_off;  // [segments]
    uint32_t *img_bits;  // [n]
    uint32_t *bitbuf;
    uint32_t *ff_sum, *ff_off;  // [byte segments]
    uint32_t *img_ff;    // [n]
    const uint8_t *header;  // device copy, header_len bytes, the SOF0 size at sof_off
    int header_len, sof_off;
    uint8_t *out;
};

// max_tiles_x / y: the largest image's tiles; max_chunks / max_bchunks: the largest image's segments
int jpeg_launch_blocks(const JpegPass &p, int max_tiles_x, int max_tiles_y, hipStream_t s);
int jpeg_launch_lengths(const JpegPass &p, int max_chunks, hipStream_t s);   // DC pass, segment sums, per-image scan
int jpeg_launch_bits(const JpegPass &p, int max_chunks, int max_bchunks, hipStream_t s);  // bit writer, 0xFF counts, per-image scan
int jpeg_launch_streams(const JpegPass &p, int max_bchunks, hipStream_t s);  // header, stuffed bytes, EOI


// ---- host side (oics_jpeg.cpp)
// Where the streams of a group of images go.  The encoder knows every stream's length before it writes one, so a caller
// without slots of the worst-case size (omr_jpeg_bound) can allocate what the streams need.
struct JpegSink {
    virtual ~JpegSink() {}
    // images [i0, i0 + cnt) have streams of len[0 .. cnt) bytes (0: no stream): *d_out and off[0 .. cnt) say where they go
    virtual int place(int i0, int cnt, const int64_t *len, uint8_t **d_out, int64_t *off) = 0;
    // they are written, and the encoder's stream has drained
    virtual int done(int i0, int cnt, const int64_t *len) = 0;
};
// The kernels keep bit offsets inside one image in 32 bits: OMR_ERR_ASSERT for a rows x cols x cn image whose scan could
// exceed 2^32 bits (every block at its longest code).  Host arithmetic; an entry point calls it on its slot shape before
// any device work.
int jpeg_check_scan_bits(int rows, int cols, int cn);
// n images at d_imgs + i * img_stride, rows `step` apart, image i sizes[2 i] x sizes[2 i + 1] (0 x 0: skipped).  Pointers,
// pitches and channels already checked; every size is held to jpeg_check_scan_bits here, before the first device call.
// Synchronises `s`; its workspace comes from the calling thread's pool scope.
int jpeg_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n,
                       int quality, JpegSink &sink, hipStream_t s);

}  // namespace omr
