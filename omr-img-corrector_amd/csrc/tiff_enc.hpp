// tiff_enc.hpp -- the Group 4 TIFF encoder's device side (tiff_enc.hip) as oics_tiff_enc.cpp sees it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "codec_stats.hpp"
#include "jpeg.hpp"  // JpegSink: where a group's streams go (the protocol is the JPEG encoder's: place, then done)
#include "tiff_head.hpp"

namespace omr {

constexpr int TENC_MAX_SIDE = 1 << 20;  // imread's own limits, as the decoder's
constexpr int64_t TENC_MAX_PIXELS = (int64_t)1 << 30;
constexpr int TENC_CODES = 104;         // per colour, in tdec_code_tables' order: entry r for a run r < 64, 63 + m / 64 for a make-up run m
constexpr int TENC_EOFB_BITS = 24;
constexpr int TENC_HEAD_MAX = tiff_head_len(true, false, true, false);  // header, the IFD with every tag, the two resolutions: 186
constexpr int TENC_HEAD_CAP = 208;      // room of TencImg::head: the 8-bit writer's head too (TENC8_HEAD_MAX, tiff_enc8.hpp)
constexpr int64_t TENC_MAX_STRIP_BITS = ((int64_t)1 << 31) - 1;  // bit offsets inside a strip are 32 bits wide
constexpr int64_t TENC_MAX_FILE = ((int64_t)1 << 32) - 1;        // classic TIFF's offsets

// One image of a launch, filled on the host.  Rows and strips of a launch are numbered through all its images.
struct TencImg {
    int64_t src_off;   // of the image's first byte from the batch's base
    int64_t out_off;   // of its stream from the output's base
    int64_t pack_off;  // its packed rows in the workspace, in dwords
    int64_t code_off;  // its rows' code segments in the workspace, in dwords
    int64_t row0;      // its first row among the launch's (len[], off[])
    int64_t strip0;    // its first strip among the launch's (sbytes[], soff[])
    int32_t rows, cols;
    int32_t rps;       // rows of a strip (1 .. rows)
    int32_t ns;        // strips
    int32_t pack_w;    // dwords of a packed row: ceil(cols / 32) and one of zeros
    int32_t seg_w;     // dwords of a row's code segment: its bound and one the merge may read behind it
    int32_t head_len;  // bytes of head[]
    int32_t off_pos, cnt_pos;  // where StripOffsets' and StripByteCounts' values stand in the file
    int32_t data_at;   // the file offset of the first strip
    uint8_t head[TENC_HEAD_CAP];  // header, IFD and resolutions as the file begins, the two strip arrays' values left out
};

// the file's head (tiff_head.hpp) into m.head, and where it says the strip arrays and the first strip stand.  Only the
// head's own bytes are written: m is a zeroed TencImg (both encoders memset theirs), so that the rest of m.head, which the
// table's upload carries along, is zeros and not stale bytes
static_assert(TENC_HEAD_MAX <= TENC_HEAD_CAP, "TencImg::head holds the Group 4 writer's head");
inline void tenc_set_head(TencImg &m, const TiffHeadDesc &d)
{
    const TiffHead h = tiff_head(d, m.head);
    m.head_len = h.head_len, m.off_pos = h.off_pos, m.cnt_pos = h.cnt_pos, m.data_at = h.data_at;
}

// what the device learns about an image
struct TencDyn {
    uint32_t data_len;  // bytes from the first strip to the file's end
    uint32_t pad;
};

struct TencPass {
    const uint8_t *src;
    int64_t step;
    const TencImg *imgs;
    TencDyn *dyn;          // [n]
    int n;
    int cn;
    uint32_t lim;          // gray: threshold; BGR: (threshold + 1) << 15, bgr.hpp's limit
    const uint32_t *codes; // [2][TENC_CODES]: code | bits << 16, white first
    uint32_t *pack;        // packed rows: pixel x of a row is bit 31 - x % 32 of dword x / 32, 1 = black
    uint32_t *code;        // the rows' code segments, first bit = bit 31 of a dword
    uint32_t *len;         // [rows] bits of a row's code
    uint32_t *off;         // [rows] its bit offset in its strip
    uint32_t *sbytes;      // [strips] bytes of a strip
    uint32_t *soff;        // [strips] its offset from the first strip's
    uint8_t *out;
    int span_steps;        // loop bounds fixed on the host: 2560 codes of one run,
    int row_steps;         // steps of a row (2 * max cols + 2),
    int lg_rows, lg_strips;  // halvings of the searches over a strip's rows and an image's strips
};

// max_*: the largest image's
int tenc_launch_pack(const TencPass &p, int64_t max_pack_bytes, hipStream_t s);
int tenc_launch_rows(const TencPass &p, int max_rows, hipStream_t s);
int tenc_launch_place(const TencPass &p, int max_strips, int max_rps, hipStream_t s);  // row offsets, then strip offsets and lengths
int tenc_launch_merge(const TencPass &p, int64_t max_data_len, int max_strips, hipStream_t s);  // head and strip arrays, then the strips' bits
// the halves of place and merge that know nothing of Group 4, for the 8-bit writer (tiff_enc8.hpp) as well: sbytes[] ->
// soff[] and dyn[] (imgs, dyn, n, sbytes, soff of p are read); head[], soff[] and sbytes[] -> the file's first data_at bytes
int tenc_launch_stripscan(const TencPass &p, int max_strips, hipStream_t s);
int tenc_launch_head(const TencPass &p, int max_strips, hipStream_t s);

// ---- host side (oics_tiff_enc.cpp)
// bits of one row's code at most, and the bound of the file's length (rps: 1 .. rows)
int64_t tenc_row_bits(int cols);
int64_t tenc_bound(int rows, int cols, int rps);
// OMR_ERR_ASSERT for an empty image, a size above imread's limits, a strip that could pass 2^31 - 1 bits or a file that could
// pass 2^32 - 1 bytes; OMR_ERR_BADARG for a negative rows_per_strip.  *rps: the rows of a strip (0 -> rows, clamped to rows)
int tenc_check_shape(int rows, int cols, int rows_per_strip, int *rps);
// OMR_ERR_BADARG for channels other than 1 or 3, a threshold outside 0 .. 254, a negative rows_per_strip or dpi
int tenc_check_params(int cn, int threshold, int rows_per_strip, int dpi);
// n images at d_imgs + i * img_stride, rows `step` apart, image i sizes[2 i] x sizes[2 i + 1] (0 x 0: skipped).  Pointers,
// pitches, parameters and every image's shape already checked.  Synchronises `s`; its workspace comes from the calling
// thread's pool scope.
int tiff_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n, int threshold,
                       int rows_per_strip, int dpi, JpegSink &sink, hipStream_t s);

constexpr int TENC_STAGES = 4;  // threshold and pack, row coder, placement, head + bit merge
struct TencStats : CodecStats<TENC_STAGES> {};
TencStats &tenc_stats();

}  // namespace omr
