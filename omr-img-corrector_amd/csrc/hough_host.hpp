// hough_host.hpp -- the host-side stages of the Hough-line path (oics_hough.cpp), shared with the FFT path
// (oics_fft.cpp) and correct_default's batches (correct_batch.cpp).  One chain serves every entry point, per call (n = 1
// on an uploaded image) and per batch:  Canny -> segments (BatchSegments) -> vote -> line pictures.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/omrdeskew.h"
#include "engine.hpp"
#include "hough_select.hpp"  // line_angles, select_omr_rs, select_fft_rs: the pure host rules

namespace omr {
namespace hh {

struct HoughParams {
    double low = 50.0, high = 150.0;  // hough.rs:27, omr.rs:239
    double rho = 1.0, theta = kPi / 180.0;
    int threshold = 0;
    double min_line_length = 0, max_line_gap = 0;
};
inline HoughParams hough_params(double min_line_length, double max_line_gap)
{
    HoughParams hp;
    hp.min_line_length = min_line_length, hp.max_line_gap = max_line_gap;
    return hp;
}

// a host image into a fresh packed device buffer
int upload(const omr_image *im, DevBuf *buf, hipStream_t s);
// Canny on n device-resident scans of one shape -> d_map holds the edges (0 / 255), packed;
// d_rowcnt (n x rows) receives the edge pixels per row (what segments_from_edges starts from)
int canny_device(const uint8_t *d_src, int64_t scan_stride, int64_t step, int rows, int cols, int cn, int n, double low_t,
                 double high_t, uint8_t *d_map, int *d_flag, hipStream_t s, int32_t *d_rowcnt);

// fn(lo, hi) over [0, count) in contiguous pieces on a few host threads (the caller's alone for a small count)
template <class Fn>
void host_fan_out(size_t count, size_t min_piece, Fn fn)
{
    // at most 16 threads, as on_threads (host_threads.hpp)
    const size_t want = std::min<size_t>(std::min(std::thread::hardware_concurrency(), 16u), count / std::max<size_t>(min_piece, 1));
    if (want < 2) return fn((size_t)0, count);
    const size_t piece = (count + want - 1) / want;
    std::vector<std::thread> pool;
    for (size_t lo = 0; lo < count; lo += piece) pool.emplace_back(fn, lo, std::min(count, lo + piece));
    for (auto &th : pool) th.join();
}

// the argument rules the device batch forms of the detectors share, before any device work: have_outputs = the caller's
// host arrays are all there; the picture's layout is looked at only when d_lined is given
int hough_batch_check(const void *d_scans, int n, int64_t stride, int rows, int cols, int cn, int64_t step, bool have_outputs,
                      const void *d_lined, int64_t lstride, int64_t lstep);

// HoughLinesP's output, the only form it has: the segments of n scans of one shape packed in scan order -- scan i owns
// segments off[i] .. off[i + 1] -- on the device (d_off; d_packed: null when there is no segment at all) and on the host
// (off, lines: four ints a segment).  edges: the edge maps as Canny left them (packed n x rows x cols), copied before
// HoughLinesP erased the points it used; filled only when asked for
struct BatchSegments {
    DevBuf edges, d_off, d_packed;
    std::vector<int32_t> off, lines;
    int scans() const { return (int)off.size() - 1; }
    size_t total() const { return (size_t)off.back(); }
    int count(int i) const { return off[(size_t)i + 1] - off[(size_t)i]; }
    int max_count() const
    {
        int m = 0;
        for (int i = 0; i < scans(); i++) m = std::max(m, count(i));
        return m;
    }
};
// The segment stage.  segments_from_edges: HoughLinesP on n packed device edge images (consumed; d_rowcnt as Canny or
// launch_edges_rowcount filled it) -> slots -> offsets -> packed list, two downloads.  batch_segments_device: Canny,
// the kept edges, then that.  A scan whose segments exceed its slot fails the call with OMR_ERR_NOMEM.
// Arguments already checked.  Both synchronise `s` on success.  The caller holds a PoolScope on `s` (a LeasedStream
// carries one) or drains `s` itself before it lets go of `seg`: the stage's own buffers go back on every return, and it
// is the block cache's drain of their stream that keeps an error return from freeing what queued work still uses.
int segments_from_edges(uint8_t *d_edges, int32_t *d_rowcnt, int n, int rows, int cols, const HoughParams &hp, hipStream_t s,
                        BatchSegments *seg);
int batch_segments_device(const uint8_t *d_scans, int n, int64_t stride, int64_t step, int rows, int cols, int cn,
                          const HoughParams &hp, bool keep_edges, hipStream_t s, BatchSegments *seg);

// The vote stage of omr.rs (:257-284): the f32 angles of the whole packed list (host threads, libm) and per angle the
// f64 count of its scan's angles within 0.1, one launch indexed by seg.d_off.  Synchronises `s`.  (hough.rs's vote is
// vote_select_kernel alone, fft.rs's is select_fft_rs.)
int omr_rs_votes(const BatchSegments &seg, hipStream_t s, std::vector<float> *ang, std::vector<int32_t> *cnt);
// omr.rs:231-302 for n device-resident scans of one shape: segments, votes, select_omr_rs per scan; a scan without a
// segment reports 0.0 and OMR_STATUS_NOT_A_RESULT.  status, n_lines and the candidate outputs -- scan 0's -- may be null.
// Arguments already checked.  Synchronises `s`
int edges_detection_device(const uint8_t *d_scans, int n, int64_t stride, int64_t step, int rows, int cols, int cn,
                           const HoughParams &hp, double *angles, int32_t *status, int32_t *n_lines, hipStream_t s,
                           double *candidates = nullptr, int32_t cand_cap = 0, int32_t *cand_len = nullptr);
// the per-call form: one packed scan, and no segment is the reference's panic (quirk B11), OMR_ERR_ASSERT; the outputs
// are written on success only
int edges_detection_one(const uint8_t *d_src, int rows, int cols, int cn, const HoughParams &hp, hipStream_t s, double *angle,
                        int32_t *status, double *candidates, int32_t cand_cap, int32_t *cand_len);

// the detectors' line pictures (lined.hip) of n packed edge maps: GRAY2BGR with picture i's device segments
// d_lines[off[i] .. off[i + 1]) drawn on in list order; arguments already checked, a null d_lines only with no segment.
// Synchronises `s`
extern const uint8_t kLinedBgr[3];
int lined_device(const uint8_t *d_edges, int n, int64_t estride, int64_t estep, int rows, int cols, const int32_t *d_lines,
                 const int32_t *off, const uint8_t bgr[3], uint8_t *d_out, int64_t ostride, int64_t ostep, hipStream_t s);
// a packed device picture (rows x cols x 3) as a fresh host image, one staged copy; synchronises `s`
int picture_to_host(const uint8_t *d_pic, int rows, int cols, hipStream_t s, omr_image_owned *picture);
// the pictures of a chunk's scans -> lined[members[j0 + j]], from several threads; skip[j] != 0 leaves scan j without one
// (skip may be null)
int download_pictures(const uint8_t *d_pics, int m, int rows, int cols, const std::vector<int> &members, int j0,
                      const int32_t *skip, omr_image_owned *lined);

}  // namespace hh
}  // namespace omr
