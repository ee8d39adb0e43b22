// tiff_enc8.hpp -- the 8-bit gray and RGB TIFF encoder's device side (tiff_enc8.hip) as oics_tiff_enc8.cpp sees it
// (DESIGN.md section 4.29).  An image of a launch is the Group 4 writer's TencImg (tiff_enc.hpp), whose placement and head
// steps write this file's offsets and first bytes too; four of its fields mean something else here, see Tenc8Pass.
//
// rows_per_strip = 0 is libtiff's default here (the most rows whose raw strip is at most 8192 bytes, at least one), not
// the Group 4 writer's one strip a page: a strip's LZW dictionary is a serial chain and the strips are this encoder's
// parallelism, so one strip a page would leave a page to one wave.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "codec_stats.hpp"
#include "tiff_enc.hpp"

namespace omr {

constexpr int TENC8_HEAD_MAX = tiff_head_len(true, true, false, true);  // header, the IFD with every tag, the two resolutions, BitsPerSample's three: 206
static_assert(TENC8_HEAD_MAX <= TENC_HEAD_CAP, "TencImg::head holds the 8-bit writer's head");
constexpr int TENC8_DEFAULT_STRIP = 8192;  // libtiff's STRIP_SIZE_DEFAULT
constexpr int TENC8_NONE = 1, TENC8_LZW = 5;  // Compression
constexpr int TENC8_PIECE = 16384;      // bytes of a strip that one workgroup of the last step copies

// TencImg here: pack_off = the image's staged strips in the workspace, in dwords; pack_w = dwords from one staged strip to
// the next (a strip's raw bytes, rounded up); code_off = its strips' coded segments, in dwords; seg_w = dwords from one
// segment to the next (tlzwe_strip_bound of a full strip, rounded up).  row0 is unused.
struct Tenc8Pass {
    TencPass t;          // src, step, imgs, dyn, n, cn, sbytes, soff, out: what tenc_launch_stripscan / _head read
    int predictor;       // 1 or 2
    int raw_to_file;     // Compression 1: the stage kernel writes the strips where they stand in the file
    uint32_t *stage;     // the staged strips (LZW)
    uint32_t *code;      // the strips' coded segments, bytes in stream order
};

// max_*: the largest image's
int tenc8_launch_stage(const Tenc8Pass &p, int64_t max_units, hipStream_t s);  // canvas rows -> raw strips (RGB order, predictor)
int tenc8_launch_lzw(const Tenc8Pass &p, int max_strips, hipStream_t s);       // raw strips -> coded segments, sbytes[]
int tenc8_launch_rawlens(const Tenc8Pass &p, int max_strips, hipStream_t s);   // Compression 1: sbytes[]
int tenc8_launch_copy(const Tenc8Pass &p, int max_strips, int64_t max_seg_bytes, hipStream_t s);  // segments -> the file, pads

// ---- host side (oics_tiff_enc8.cpp)
// the rows of a strip: rows_per_strip clamped to rows, 0 -> the default above
int tenc8_rps(int rows, int cols, int cn, int rows_per_strip);
// the bound of the file's length (rps: 1 .. rows)
int64_t tenc8_bound(int rows, int cols, int cn, int compression, int rps);
// OMR_ERR_ASSERT for an empty image, a size above imread's limits, a strip that could pass 2^31 - 1 bits or a file that could
// pass 2^32 - 1 bytes.  *rps: the rows of a strip
int tenc8_check_shape(int rows, int cols, int cn, int compression, int rows_per_strip, int *rps);
// OMR_ERR_BADARG for channels other than 1 or 3, a compression other than 1 or 5, a predictor other than 1 or 2, predictor 2
// without LZW, a negative rows_per_strip or dpi
int tenc8_check_params(int cn, int compression, int predictor, int rows_per_strip, int dpi);
// n images at d_imgs + i * img_stride, rows `step` apart, image i sizes[2 i] x sizes[2 i + 1] (0 x 0: skipped).  Pointers,
// pitches, parameters and every image's shape already checked.  Synchronises `s`; its workspace comes from the calling
// thread's pool scope.
int tiff8_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n, int compression,
                        int predictor, int rows_per_strip, int dpi, JpegSink &sink, hipStream_t s);

constexpr int TENC8_STAGES = 4;  // staging, LZW (raw: the strips' lengths), placement, head + strips into the file
struct Tenc8Stats : CodecStats<TENC8_STAGES> {};
Tenc8Stats &tenc8_stats();

}  // namespace omr
