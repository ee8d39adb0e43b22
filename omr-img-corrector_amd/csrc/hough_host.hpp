// hough_host.hpp -- host-side building blocks of the Hough-line path (oics_hough.cpp), shared with
// the FFT path (oics_fft.cpp), which ends in the same Canny -> HoughLinesP -> vote chain.
#pragma once
#include <stdint.h>

#include <math.h>

#include <algorithm>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/omrdeskew.h"
#include "engine.hpp"

namespace omr {
namespace hh {

constexpr double kPi = 3.14159265358979323846;

struct HoughParams {
    double low = 50.0, high = 150.0;  // hough.rs:27, omr.rs:239
    double rho = 1.0, theta = kPi / 180.0;
    int threshold = 0;
    double min_line_length = 0, max_line_gap = 0;
};

// a host image into a fresh packed device buffer
int upload(const omr_image *im, DevBuf *buf, hipStream_t s);
// Canny on n device-resident scans of one shape -> d_map holds the edges (0 / 255), packed;
// d_rowcnt (n x rows) receives the edge pixels per row (what ppht_device starts from)
int canny_device(const uint8_t *d_src, int64_t scan_stride, int64_t step, int rows, int cols, int cn, int n, double low_t,
                 double high_t, uint8_t *d_map, int *d_flag, hipStream_t s, int32_t *d_rowcnt);
// HoughLinesP on n device-resident edge images (packed)
int ppht_device(uint8_t *d_edges, int32_t *d_rowcnt, int rows, int cols, int n, const HoughParams &hp, hipStream_t s,
                std::vector<std::vector<int32_t>> *lines_out);
// keep_edges (may be null): receives a copy of the edge maps, which HoughLinesP consumes
int edges_lines_device(const uint8_t *d_src, int64_t scan_stride, int64_t step, int rows, int cols, int cn, int n,
                       const HoughParams &hp, hipStream_t s, std::vector<std::vector<int32_t>> *lines,
                       DevBuf *keep_edges = nullptr);
// the detectors' line picture (lined.hip): GRAY2BGR of a packed device edge map with `n_lines` host segments
// (x0, y0, x1, y1) drawn on in list order, as a fresh host image; synchronises `s`
extern const uint8_t kLinedBgr[3];
int lined_to_host(const uint8_t *d_edges, int rows, int cols, const int32_t *lines, int n_lines, const uint8_t bgr[3],
                  hipStream_t s, omr_image_owned *picture);
void line_angles(const std::vector<int32_t> &l, std::vector<float> *ang);
int vote_counts(const std::vector<float> &ang, bool as_f64, hipStream_t s, std::vector<int32_t> *counts);
int select_omr_rs(const std::vector<float> &ang, const std::vector<int32_t> &cnt, double *angle, int32_t *status,
                  double *candidates, int32_t cand_cap, int32_t *cand_len);

// fft.rs:197-247 on n segments (x1, y1, x2, y2): f64 angles (libm atan2) folded into [-45, 45]; the inner loop re-reads
// line i (quirk B10, fft.rs:231), so line i collects n - 1 votes iff its raw angle is within 0.1 of its folded angle,
// else none.  No segment, or no line with a vote: 0.0.  The one statement of the rule, for the per-call and batch forms
inline void select_fft_rs(const int32_t *l, int n, double *angle_out)
{
    double average_angle = 0.0;
    int max_votes = 0;
    for (int i = 0; i < n; i++) {
        const double x1 = l[4 * i], y1 = l[4 * i + 1], x2 = l[4 * i + 2], y2 = l[4 * i + 3];
        const double raw = (atan2(y2 - y1, x2 - x1) * 180.0) / kPi;
        const double angle = raw < -45.0 ? raw + 90.0 : (raw > 45.0 ? raw - 90.0 : raw);
        int votes = 0;
        for (int j = 0; j < n; j++) {
            if (i == j) continue;
            if (fabs(raw - angle) < 0.1) votes++;
        }
        if (votes > max_votes) {
            max_votes = votes;
            average_angle = angle;
        }
        if (max_votes == n - 1 && n > 1) break;  // nothing can beat n - 1 with a strict '>'
    }
    *angle_out = average_angle;
}

// ---- the batch forms' shared stages (oics_hough.cpp)

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

// What the segment stage of a batch leaves: Canny and HoughLinesP of n scans of one shape, the segments packed in scan
// order -- scan i owns segments off[i] .. off[i + 1] -- on the device (d_packed: null when the batch has no segment at
// all) and on the host (lines, four ints a segment).  edges: the edge maps as Canny left them (packed n x rows x cols),
// copied before HoughLinesP erased the points it used; filled only when asked for
struct BatchSegments {
    DevBuf edges, d_off, d_packed;
    std::vector<int32_t> off, lines;
    size_t total() const { return (size_t)off.back(); }
    int count(int i) const { return off[(size_t)i + 1] - off[(size_t)i]; }
};
// arguments already checked.  Synchronises `s` on success.  The caller holds a PoolScope on `s` (or drains `s` itself
// before it lets go of `seg`): the stage's own buffers go back on every return, and it is the block cache's drain of
// their stream that keeps an error return from freeing what queued work still uses.
int batch_segments_device(const uint8_t *d_scans, int n, int64_t stride, int64_t step, int rows, int cols, int cn,
                          const HoughParams &hp, bool keep_edges, hipStream_t s, BatchSegments *seg);
// the line pictures of n packed edge maps (lined.hip); arguments already checked, a null d_lines only with no segment.
// Synchronises `s`
int lined_device(const uint8_t *d_edges, int n, int64_t estride, int64_t estep, int rows, int cols, const int32_t *d_lines,
                 const int32_t *off, const uint8_t bgr[3], uint8_t *d_out, int64_t ostride, int64_t ostep, hipStream_t s);
// the body of omr_edges_detection_batch_device (omr.rs:231-302 per scan); arguments already checked.  Synchronises `s`
int edges_detection_device(const uint8_t *d_scans, int n, int64_t stride, int64_t step, int rows, int cols, int cn,
                           const HoughParams &hp, double *angles, int32_t *status, int32_t *n_lines, hipStream_t s);
// pictures (packed, `pic` bytes each, rows x cols x 3) of a chunk's scans -> fresh host images lined[members[j0 + j]], from
// several threads, one staged copy each; skip[j] != 0 leaves scan j without one (skip may be null)
int download_pictures(const uint8_t *d_pics, int m, int rows, int cols, const std::vector<int> &members, int j0,
                      const int32_t *skip, omr_image_owned *lined);

}  // namespace hh
}  // namespace omr
