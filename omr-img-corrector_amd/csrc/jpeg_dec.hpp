// jpeg_dec.hpp -- the baseline JPEG decoder's device side (jpeg_dec.hip) as oics_jpeg_dec.cpp sees it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "codec_stats.hpp"

namespace omr {

// Bits of a subsequence (one lane of the Huffman kernels) and subsequences per workgroup.  -DOMR_JDEC_SUB_BITS /
// -DOMR_JDEC_LANES build the library with other values for a measurement (tools/bench_jpeg_decode.py --sweep); a
// workgroup stages LANES x SUB_BITS / 8 bytes of the bit buffer in LDS, so 2048 bits go with 128 lanes.  1024 is the
// measured choice (profiles/r18_jpeg_decode.md): 512 gains 7 % on the dataset's sheets and loses 12 % at A4 quality 100,
// 2048 gains 6 % there and loses 14 % on the dataset's sheets.
#ifndef OMR_JDEC_SUB_BITS
#define OMR_JDEC_SUB_BITS 1024
#endif
#ifndef OMR_JDEC_LANES
#define OMR_JDEC_LANES 256
#endif
constexpr int JDEC_SUB_BITS = OMR_JDEC_SUB_BITS;
constexpr int JDEC_LANES = OMR_JDEC_LANES;
static_assert(JDEC_SUB_BITS % 32 == 0 && JDEC_SUB_BITS >= 32, "a subsequence is whole words");
static_assert(JDEC_LANES == 128 || JDEC_LANES == 256, "the span staging reads place_of from threads 0 and 64");
constexpr int JDEC_BYTE_CHUNK = 4096;   // stuffed bytes per workgroup of the un-stuffing kernels
constexpr int JDEC_PAD = 64;            // bytes kept free behind an image's bit buffer (the kernels peek 8 bytes ahead)

// one DHT table as the kernels look it up
struct JdecHuff {
    uint16_t look[512];   // the next 9 bits -> length << 8 | symbol; 0: a longer code, or none
    int32_t maxcode[17];  // [len] the largest code of that length, -1: none
    int32_t valoff[17];   // [len] index into vals of that length's first code, minus that code
    uint8_t vals[256];
};

// per image: the tables of component 0 .. 2 (a gray stream fills [0])
struct JdecTables {
    JdecHuff dc[3], ac[3];
    uint16_t quant[3][64];  // zig-zag order, as DQT has them
};

// One image of a launch, filled on the host from its header.
struct JdecImg {
    int64_t src_off;       // its entropy data (everything behind SOS) in the uploaded bytes
    int64_t bit_off;       // its un-stuffed bytes in the bit buffer (multiple of 16; src_len + JDEC_PAD bytes are its own)
    int64_t out_off;       // its slot in the output
    int64_t plane_off[3];  // its component planes, whole MCUs large
    uint32_t src_len;
    int32_t rows, cols;
    int32_t ncomp, hs, vs;    // components; Y's sampling factors (chroma: 1 x 1)
    int32_t mw, mh, bpm, ri;  // MCUs per row / column, blocks per MCU, restart interval in MCUs (0: none)
    uint32_t nmcu, nblk;      // of the scan, dummy blocks included
    uint32_t blk0;            // its blocks in the coefficient array
    uint32_t nival, ival0;    // intervals the header predicts; its nival + 1 entries of ival_start / ival_sub0
    uint32_t sub0, sub_cap;   // its subsequences: ceil(src_len * 8 / JDEC_SUB_BITS) + nival bounds their number
    uint32_t chunk0, nchunk;  // its JDEC_BYTE_CHUNK segments
    int32_t ypitch, cpitch;   // pitch of the Y / chroma planes
};

// what the device learns about an image
struct JdecDyn {
    uint32_t end_pos;  // where the scan ends in its entropy data
    uint32_t nbytes;   // un-stuffed bytes
    uint32_t nsub;     // subsequences
    uint32_t err;      // != 0: the entropy data is not a scan of this header (OMR_ERR_ASSERT); later kernels skip the image
};

struct JdecPass {
    const uint8_t *src;
    const JdecImg *imgs;
    const JdecTables *tabs;  // [n]
    JdecDyn *dyn;            // [n], cleared
    int n;
    int channels;            // of the output: 1 or 3
    uint32_t *chunk_keep, *chunk_rst, *chunk_end;  // [segments] counts, and the first end-of-scan inside (or ~0)
    uint32_t *chunk_off, *chunk_rst_off;           // [segments] exclusive sums over the image
    uint8_t *bitbuf;
    uint32_t *ival_start;   // bytes
    uint32_t *ival_sub0;    // first subsequence (counted from the image's first)
    uint64_t *state;        // [subsequences] where its lane stands at its end: bit << 32 | zig-zag index << 8 | slot
    uint32_t *sub_cnt;      // [subsequences][4] blocks finished, DC differences summed per component
    uint32_t *sub_ex;       // [subsequences][4] their exclusive sums over the image
    uint8_t *chg;           // [2][total subsequences] "changed in that round"
    uint32_t sub_total;
    uint32_t *changed;      // [1] lanes whose state changed in the round
    int16_t *coef;          // [blocks][64] zig-zag, DC values in [0]; cleared
    uint8_t *planes;
    uint8_t *out;
    int64_t step;
};

// max_chunks: the largest image's byte segments
int jdec_launch_unstuff(const JdecPass &p, int max_chunks, hipStream_t s);
// one round of the self-synchronising decode (round 0: every lane from its own first bit); max_groups: the largest
// image's sub_cap in workgroups of JDEC_LANES
int jdec_launch_sync(const JdecPass &p, int round, int max_groups, hipStream_t s);
// the sums per subsequence, the coefficients, the inverse DCT, up-sampling and colour
// marks: null, or two events recorded behind the coefficient kernel and behind the inverse DCT
int jdec_launch_finish(const JdecPass &p, int max_groups, uint32_t max_blocks, int max_rows, int max_cols, hipStream_t s,
                       hipEvent_t *marks);

// ---- host side (oics_jpeg_dec.cpp)
// What a stream's header says.  jdec_parse returns 0, OMR_ERR_NOTIMPL, OMR_ERR_BADARG (or OMR_ERR_ASSERT for entropy data
// of 2^32 bits or more) with the thread's error text set; rows / cols are filled whenever SOF was readable.  orient: the
// EXIF orientation the last APP1 segment that carries one gives (1: none).  With refuse_orientation, a value other than 1
// is OMR_ERR_NOTIMPL -- the contract of omr_jpeg_info / omr_jpeg_decode*; the imread layer (orient.hpp) passes false and
// turns the image.
struct JdecHeader {
    int32_t rows = 0, cols = 0, ncomp = 0, hs = 0, vs = 0, ri = 0;
    int32_t orient = 1;
    int64_t data = 0;  // offset of the entropy data
    JdecTables tab;
};
int jdec_parse(const uint8_t *stream, int64_t len, JdecHeader *h, bool refuse_orientation = true);
// n parsed streams (hdr[i]; skip[i] != 0: not decoded) into slots d_out + i * out_stride of `channels` channels, rows
// `step` apart; every image fits its slot (checked by the caller).  rc[i] = OMR_ERR_ASSERT where the entropy data is not a
// scan of its header.  Synchronises `s`; its workspace comes from the calling thread's pool scope.
int jpeg_decode_device(const uint8_t *const *streams, const int64_t *len, const JdecHeader *hdr, const int32_t *skip, int n,
                       int channels, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s);


// What omr_jpeg_decode_stats reports: kept per thread, filled by jpeg_decode_device while `on`.
constexpr int JDEC_STAGES = 6;  // upload and clearing, un-stuffing, synchronisation rounds, coefficients, inverse DCT, colour
struct JdecStats : CodecStats<JDEC_STAGES> {
    int32_t rounds = 0;  // the most any group took
    void begin_call() { CodecStats::begin_call(), rounds = 0; }
};
JdecStats &jdec_stats();

}  // namespace omr
