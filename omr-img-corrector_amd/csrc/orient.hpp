// orient.hpp -- the eight EXIF orientation transforms on device-resident images (orient.hip) and the imread layer that
// applies them (oics_imread.cpp); DESIGN.md section 4.23.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "jpeg_dec.hpp"
#include "png_dec.hpp"
#include "tiff_dec.hpp"

namespace omr {

// One image of a launch.  rows x cols is the SOURCE image; codes 5..8 write cols x rows.
struct OrientImg {
    int64_t src_off, dst_off;  // bytes from the launch's source / destination base to the image's first pixel
    int32_t rows, cols;
    int32_t code;     // 1..8
    int32_t tiles_x;  // tiles per tile row of the source (filled by orient_plan)
};

// what a code does, as three switches: the result has the source's columns as rows; source rows / columns run backwards
__host__ __device__ inline bool orient_transposes(int code) { return code >= 5; }
__host__ __device__ inline bool orient_flips_rows(int code) { return code == 3 || code == 4 || code == 6 || code == 7; }
__host__ __device__ inline bool orient_flips_cols(int code) { return code == 2 || code == 3 || code == 7 || code == 8; }

// orient_plan fills tiles_x of n host records and gives the tile count of the largest image (the grid's width); the
// caller uploads the records.  orient_launch: the n images (n <= 65535) of `cn` (1 or 3) byte channels, source rows `sstep`
// and destination rows `dstep` bytes apart, in one launch on `s`.  Every image and its turned form lie inside their
// buffers (checked by the caller).
void orient_plan(OrientImg *recs, int n, int cn, int *max_tiles);
hipError_t orient_launch(const uint8_t *d_src, int64_t sstep, uint8_t *d_dst, int64_t dstep, int cn, const OrientImg *d_recs,
                         int n, int max_tiles, hipStream_t s);

// ---- host side (oics_imread.cpp)
// the records' upload and the launches for any n (arguments already checked; tiles_x is filled in); synchronises `s`
int orient_device(const uint8_t *d_src, int64_t sstep, uint8_t *d_dst, int64_t dstep, int cn, std::vector<OrientImg> *recs,
                  hipStream_t s);

// What imread does with a parsed JPEG's EXIF orientation: 0 = decode as stored (code 1, or `ignore`), 1 = decode and turn
// (2..8), OMR_ERR_NOTIMPL for a value outside 1..8.
int imread_turn_of(const JdecHeader &h, bool ignore);

// A stream's kind, by its first bytes: PNG's eight signature bytes, "II*\0" / "MM\0*" for a TIFF, else a JPEG.  The values
// are those of OMR_IMREAD_KIND_*.
enum ImreadKind : uint8_t { IMREAD_JPEG = 0, IMREAD_PNG = 1, IMREAD_TIFF = 2 };
// the parsed headers of a run of streams: member i's header stands in the array of kind[i], the other two entries are unused
struct ImreadHeaders {
    const JdecHeader *jpeg;
    const PdecHeader *png;
    const TdecHeader *tiff;
    const uint8_t *kind;
};
// What the header step of every imread entry point and of the streams flows finds for one stream.
struct ImreadParsed {
    int kind = IMREAD_JPEG;
    int rc = 0;
    int rows = 0, cols = 0;  // as imread returns it: after the turn
    int components = 0, orient = 1;
};
// The header of its kind is filled in; rc by its decoder's rules, with a JPEG's orientation 2..8 accepted (and the size
// turned) unless `ignore`, a value outside 1..8 refused.  channels: 1 or 3 adds the PNG decoder's rule for that output
// (pdec_check_channels), 0 leaves it out.
ImreadParsed imread_parse(const uint8_t *stream, int64_t len, int channels, bool ignore, JdecHeader *jpeg, PdecHeader *png, TdecHeader *tiff);

#pragma GCC visibility push(hidden)  // the library's own: not in the dynamic symbol table
// The owner of a run's parsed headers: the three parallel header vectors and the kind bytes behind an ImreadHeaders.
struct ImreadRun {
    std::vector<JdecHeader> jpeg;
    std::vector<PdecHeader> png;
    std::vector<TdecHeader> tiff;
    std::vector<uint8_t> kind;
    void reserve(size_t n) { jpeg.reserve(n), png.reserve(n), tiff.reserve(n), kind.reserve(n); }
    // imread_parse of one more stream, as the run's last member; a caller that does not accept it drops it again
    ImreadParsed append(const uint8_t *stream, int64_t len, int channels, bool ignore);
    void drop_last() { jpeg.pop_back(), png.pop_back(), tiff.pop_back(), kind.pop_back(); }
    ImreadHeaders view() const { return ImreadHeaders{jpeg.data(), png.data(), tiff.data(), kind.data()}; }
};

// One chunk of a streams flow's bucket, reused from chunk to chunk: what imread_decode_device takes for members
// idx[j0 .. j0 + z) of the run `src` (with the run's streams and their lengths), and their codes.
struct ImreadChunk {
    std::vector<const uint8_t *> zs;
    std::vector<int64_t> zlen;
    ImreadRun hd;
    std::vector<int32_t> zrc;
    void gather(const ImreadHeaders &src, const uint8_t *const *streams, const int64_t *len, const std::vector<int> &idx, int j0, int z);
};
#pragma GCC visibility pop

// The decode of one run of parsed streams into the slots d_out + i * out_stride (rows `step` apart): PNG and TIFF members
// and JPEG members that need no turn (orient == 1, or `ignore`) go straight into their slots through their decoders; JPEG
// members with an orientation 2..8 are decoded into a scratch buffer of the run and turned into their slots by one launch
// of orient.hip -- no scratch and no launch when the run has none.  skip (may be null): members left alone.  Every
// member's turned image fits its slot (checked by the caller).  rc[i] as the decoders'.  Synchronises `s`.
int imread_decode_device(const uint8_t *const *streams, const int64_t *len, const ImreadHeaders &hd, const int32_t *skip, int n,
                         int channels, bool ignore, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s);

}  // namespace omr
