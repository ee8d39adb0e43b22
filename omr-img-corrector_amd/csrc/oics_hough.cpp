// oics_hough.cpp -- host side of the Hough-line deskew path and of
// correct_default, exported through the C ABI with the reference's names and argument meaning:
//
//   oics::hough::get_angle_with_hough            packages/lib/src/hough.rs:17-100
//   oics::omr::get_result_from_edges_detection   packages/lib/src/omr.rs:231-302
//   oics::omr::correct_default                   packages/lib/src/omr.rs:339-448 (minus imread / imwrite)
//   imgproc::canny / imgproc::hough_lines_p      call sites hough.rs:27-43, omr.rs:236-253
//
// One chain of stages (hough_host.hpp) serves every entry point; a per-call form is
// the batch form with n = 1 on an uploaded image.  The image work (Canny, point list, progressive
// probabilistic Hough, the O(n^2) votes) runs on the GPU (hough.hip).  The host builds the 180-entry
// trigonometric / walk tables (double cos / sin -> float, exactly hough.cpp's expressions), turns the
// segments into angles with libm (hough_select.hpp) and applies omr.rs's selection rule.  No CPU
// fallback: without a HIP device every entry point returns -217.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "../../include/omrdeskew.h"
#include "detector_deskew.hpp"
#include "engine.hpp"
#include "hough.hpp"
#include "hough_host.hpp"
#include "host_threads.hpp"

using namespace omr;
using namespace omr::hh;

namespace omr {
namespace hh {

// omr_hough_set_scans_in_flight(): 0 = the default (launch_ppht: one workgroup per scan)
std::atomic<int> g_scans_in_flight{0};

const uint8_t kLinedBgr[3] = {186, 88, 255};  // Scalar(186, 88, 255, 0): hough.rs:59, fft.rs:209

inline int cv_round(double v) { return (int)lrint(v); }
inline int cv_round(float v) { return (int)lrintf(v); }

// Canny on n device-resident scans of one shape -> d_map holds the edges (0 / 255), packed.
int canny_device(const uint8_t *d_src, int64_t scan_stride, int64_t step, int rows, int cols, int cn, int n, double low_t,
                 double high_t, uint8_t *d_map, int *d_flag, hipStream_t s, int32_t *d_rowcnt)
{
    if (low_t > high_t) std::swap(low_t, high_t);
    const int low = (int)floor(low_t), high = (int)floor(high_t);
    OMR_HIP(launch_canny_nms(d_src, scan_stride, step, rows, cols, cn, n, low, high, d_map, s));
    for (int pass = 0; pass < 100000; pass++) {
        int flag = 0;
        OMR_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), s));
        OMR_HIP(launch_canny_hysteresis(d_map, rows, cols, n, d_flag, s));
        OMR_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
        OMR_HIP(hipStreamSynchronize(s));
        if (!flag) break;
    }
    OMR_HIP(launch_edges_rowcount(d_map, rows, cols, n, 1, d_rowcnt, s));
    return OMR_OK;
}

// A HoughLinesP launch on n scans and what it owns on the device until the caller has read the result: n slots of `cap`
// segments in `lines`, the segments found per scan in `nlines`
struct PphtRun {
    DevBuf rowoff, total, scanoff, nz, order, d_ttab, d_walk, d_rowbase, accum, lines, nlines, tiled, queue;
    int cap = 0;
};

// enqueues HoughLinesP on n device-resident edge images (d_edges: packed, kept; d_rowcnt filled)
static int ppht_launch(uint8_t *d_edges, int32_t *d_rowcnt, int rows, int cols, int n, const HoughParams &hp, hipStream_t s,
                       PphtRun *run)
{
    const float rho = (float)hp.rho, theta = (float)hp.theta, irho = 1.0f / rho;
    if (!(rho > 0) || !(theta > 0)) return fail(OMR_ERR_BADARG, "rho and theta must be positive");
    const int numangle = cv_round(3.1415926535897932384626433832795 / theta);
    if (numangle <= 0 || numangle > OMR_PPHT_MAX_ANGLES)
        return fail(OMR_ERR_NOTIMPL, "HoughLinesP: %d accumulator angles (theta too small; the reference uses pi/180)",
                    numangle);
    std::vector<float> ttab((size_t)numangle * 2);
    std::vector<PphtWalk> walk((size_t)numangle);
    for (int k = 0; k < numangle; k++) {
        ttab[2 * k] = (float)(cos((double)k * theta) * irho);
        ttab[2 * k + 1] = (float)(sin((double)k * theta) * irho);
        const float a = -ttab[2 * k + 1], b = ttab[2 * k];
        PphtWalk w{};
        if (fabsf(a) > fabsf(b)) {
            w.xflag = 1;
            w.dx0 = a > 0 ? 1 : -1;
            w.dy0 = cv_round(b * (float)(1 << 16) / fabsf(a));
        } else {
            w.xflag = 0;
            w.dy0 = b > 0 ? 1 : -1;
            w.dx0 = cv_round(a * (float)(1 << 16) / fabsf(b));
        }
        walk[k] = w;
    }
    // OpenCV's accumulator has (cols + rows) * 2 + 1 bins per angle; a pixel of a cols x rows image only reaches
    // rho = cvRound(x cos + y sin) in [lo_k, hi_k], so row k keeps just that range (+-2 for the float rounding)
    std::vector<int32_t> row_base((size_t)numangle);
    int64_t accum_stride = 0;
    for (int k = 0; k < numangle; k++) {
        const double c = ttab[2 * k], sn = ttab[2 * k + 1];
        const double lo = (cols - 1) * std::min(c, 0.0) + (rows - 1) * std::min(sn, 0.0);
        const double hi = (cols - 1) * std::max(c, 0.0) + (rows - 1) * std::max(sn, 0.0);
        const int64_t rmin = (int64_t)floor(lo) - 2, rmax = (int64_t)ceil(hi) + 2;
        row_base[k] = (int32_t)(accum_stride - rmin);
        accum_stride += rmax - rmin + 1;
    }
    accum_stride += 64;  // scratch bins of the lanes that hold no angle
    accum_stride += accum_stride & 1;
    const bool acc_u16 = rows + cols <= OMR_PPHT_U16_MAX_EXTENT;  // hough.hip: a bin's count is bounded by the diagonal
    const size_t bin_bytes = acc_u16 ? sizeof(uint16_t) : sizeof(int32_t);
    DevBuf &rowoff = run->rowoff, &total = run->total, &scanoff = run->scanoff, &nz = run->nz, &order = run->order;
    DevBuf &d_ttab = run->d_ttab, &d_walk = run->d_walk, &d_rowbase = run->d_rowbase, &accum = run->accum;
    DevBuf &lines = run->lines, &nlines = run->nlines, &tiled = run->tiled, &queue = run->queue;
    OMR_HIP(rowoff.alloc(sizeof(int32_t) * (size_t)n * rows));
    OMR_HIP(total.alloc(sizeof(int32_t) * (size_t)n));
    OMR_HIP(launch_edges_rowscan(d_rowcnt, rows, n, rowoff.as<int32_t>(), total.as<int32_t>(), s));
    std::vector<int32_t> counts((size_t)n);
    OMR_HIP(hipMemcpyAsync(counts.data(), total.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    std::vector<int64_t> off((size_t)n);
    int64_t sum = 0;
    int maxc = 0;
    for (int i = 0; i < n; i++) {
        off[i] = sum;
        sum += counts[i];
        maxc = std::max(maxc, counts[i]);
    }
    const int cap = std::max(1, std::min(maxc, 1 << 16));
    OMR_HIP(scanoff.alloc(sizeof(int64_t) * (size_t)n));
    OMR_HIP(nz.alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(sum, 1)));
    OMR_HIP(order.alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(sum, 1)));
    OMR_HIP(hipMemcpyAsync(scanoff.p, off.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
    OMR_HIP(tiled.alloc((size_t)n * (size_t)ppht_mask_bytes(rows, cols)));
    OMR_HIP(hipMemsetAsync(tiled.p, 0, tiled.bytes, s));
    OMR_HIP(launch_edges_compact(d_edges, rows, cols, n, rowoff.as<int32_t>(), scanoff.as<int64_t>(), nz.as<uint32_t>(),
                                 tiled.as<uint8_t>(), s));
    OMR_HIP(d_ttab.alloc(sizeof(float) * ttab.size()));
    OMR_HIP(d_walk.alloc(sizeof(PphtWalk) * walk.size()));
    OMR_HIP(hipMemcpyAsync(d_ttab.p, ttab.data(), sizeof(float) * ttab.size(), hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemcpyAsync(d_walk.p, walk.data(), sizeof(PphtWalk) * walk.size(), hipMemcpyHostToDevice, s));
    OMR_HIP(d_rowbase.alloc(sizeof(int32_t) * row_base.size()));
    OMR_HIP(hipMemcpyAsync(d_rowbase.p, row_base.data(), sizeof(int32_t) * row_base.size(), hipMemcpyHostToDevice, s));
    OMR_HIP(accum.alloc(bin_bytes * (size_t)n * (size_t)accum_stride));
    OMR_HIP(hipMemsetAsync(accum.p, acc_u16 ? 0x80 : 0, accum.bytes, s));
    OMR_HIP(lines.alloc(sizeof(int32_t) * 4 * (size_t)n * cap));
    OMR_HIP(nlines.alloc(sizeof(int32_t) * (size_t)n));
    PphtArgs a{};
    a.mask = tiled.as<uint8_t>();
    a.width = cols;
    a.height = rows;
    a.nz = nz.as<uint32_t>();
    a.order = order.as<uint32_t>();
    a.scan_off = scanoff.as<int64_t>();
    a.count = total.as<int32_t>();
    a.accum = accum.p;
    a.accum_stride = accum_stride;
    a.acc_u16 = acc_u16 ? 1 : 0;
    a.row_base = d_rowbase.as<int32_t>();
    a.numangle = numangle;
    a.ttab = d_ttab.as<float>();
    a.walk = d_walk.as<PphtWalk>();
    a.threshold = hp.threshold;
    a.line_length = cv_round(hp.min_line_length);
    a.line_gap = cv_round(hp.max_line_gap);
    a.lines = lines.as<int32_t>();
    a.cap = cap;
    a.n_lines = nlines.as<int32_t>();
    OMR_HIP(queue.alloc(sizeof(int32_t)));
    OMR_HIP(hipMemsetAsync(queue.p, 0, sizeof(int32_t), s));
    a.n_scans = n;
    a.queue = queue.as<int32_t>();
    OMR_HIP(launch_ppht(a, g_scans_in_flight.load(std::memory_order_relaxed), s));
    run->cap = cap;
    return OMR_OK;
}

// HoughLinesP -> packed segment list (hough_host.hpp).  d_over and the PPHT run are released on every return without a
// wait of their own: the caller's PoolScope makes that a drain of `s`
int segments_from_edges(uint8_t *d_edges, int32_t *d_rowcnt, int n, int rows, int cols, const HoughParams &hp, hipStream_t s,
                        BatchSegments *seg)
{
    PphtRun run;
    int rc = ppht_launch(d_edges, d_rowcnt, rows, cols, n, hp, s, &run);
    if (rc) return rc;
    // slots -> offsets (one small download) -> packed list (one download)
    DevBuf d_over;
    DevBuf &d_off = seg->d_off, &d_packed = seg->d_packed;
    std::vector<int32_t> &off = seg->off;
    off.assign((size_t)n + 1, 0);
    seg->lines.clear();
    int32_t over[2] = {0, 0};
    OMR_HIP(d_off.alloc(sizeof(int32_t) * off.size()));
    OMR_HIP(d_over.alloc(sizeof(over)));
    OMR_HIP(hipMemsetAsync(d_over.p, 0, sizeof(over), s));
    OMR_HIP(launch_ppht_offsets(run.nlines.as<int32_t>(), n, run.cap, d_off.as<int32_t>(), d_over.as<int32_t>(), s));
    OMR_HIP(hipMemcpyAsync(off.data(), d_off.p, sizeof(int32_t) * off.size(), hipMemcpyDeviceToHost, s));
    OMR_HIP(hipMemcpyAsync(over, d_over.p, sizeof(over), hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    if (over[0]) return fail(OMR_ERR_NOMEM, "HoughLinesP: %d segments exceed the buffer of %d", over[0], run.cap);
    if (over[1]) return fail(OMR_ERR_NOMEM, "HoughLinesP: the batch's segments exceed a list of 2^31 - 1");
    const size_t total = seg->total();
    if (total > 0) {
        seg->lines.resize(total * 4);
        OMR_HIP(d_packed.alloc(sizeof(int32_t) * 4 * total));
        OMR_HIP(launch_ppht_pack(run.lines.as<int32_t>(), run.cap, d_off.as<int32_t>(), n, seg->max_count(), d_packed.as<int32_t>(), s));
        OMR_HIP(hipMemcpyAsync(seg->lines.data(), d_packed.p, sizeof(int32_t) * 4 * total, hipMemcpyDeviceToHost, s));
        OMR_HIP(hipStreamSynchronize(s));
    }
    return OMR_OK;
}

// upload a host image into a packed device buffer
int upload(const omr_image *im, DevBuf *buf, hipStream_t s)
{
    const size_t row = (size_t)im->cols * im->channels;
    OMR_HIP(buf->alloc(row * (size_t)im->rows));
    return upload_rows(buf->p, row, im->data, (size_t)im->step_bytes, row, (size_t)im->rows, s);
}

// ---- the line picture (lined.hip): every argument rule of the omr_lined_picture* entry points, before any device work
static int lined_check(const void *d_edges, int n, int64_t estride, int64_t estep, int rows, int cols, const void *d_lines,
                       const int32_t *off, const uint8_t *bgr, const void *d_out, int64_t ostride, int64_t ostep, bool batch)
{
    clear_error();
    if (!d_edges || !d_out || !off || !bgr) return fail(OMR_ERR_BADARG, "null pointer");
    if (n <= 0) return fail(OMR_ERR_BADARG, "empty batch");
    int rc = check_image_shape(rows, cols);
    if (rc) return rc;
    if (estep < cols || ostep < 3 * (int64_t)cols) return fail(OMR_ERR_BADARG, "step too small");
    if (batch) {
        if (estride < 0) return fail(OMR_ERR_BADARG, "negative edge-map stride");
        if (ostride < rows * ostep) return fail(OMR_ERR_BADARG, "picture stride smaller than a picture");
    }
    if (off[0] < 0) return fail(OMR_ERR_BADARG, "negative segment count or offset");
    for (int i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return fail(OMR_ERR_BADARG, "line_offsets must not decrease (picture %d)", i);
    if (off[n] > off[0] && !d_lines) return fail(OMR_ERR_BADARG, "null segment list");
    if (d_edges == d_out) return fail(OMR_ERR_BADARG, "the picture cannot be made in place");
    return OMR_OK;
}

// arguments already checked.  Synchronises `s`: the end-point verdict is read before anything is drawn, and the segment
// records go back to the block cache on return
int lined_device(const uint8_t *d_edges, int n, int64_t estride, int64_t estep, int rows, int cols, const int32_t *d_lines,
                 const int32_t *off, const uint8_t bgr[3], uint8_t *d_out, int64_t ostride, int64_t ostep, hipStream_t s)
{
    PoolScope scope(s);
    const int64_t total = (int64_t)off[n] - off[0];
    std::vector<int32_t> rel((size_t)n + 1);
    for (int i = 0; i <= n; i++) rel[i] = off[i] - off[0];
    DevBuf segs, doff, bad;
    OMR_HIP(segs.alloc(sizeof(LinedSeg) * (size_t)std::max<int64_t>(total, 1)));
    OMR_HIP(doff.alloc(sizeof(int32_t) * rel.size()));
    OMR_HIP(hipMemcpyAsync(doff.p, rel.data(), sizeof(int32_t) * rel.size(), hipMemcpyHostToDevice, s));
    if (total > 0) {
        int32_t verdict = 0;
        OMR_HIP(bad.alloc(sizeof(int32_t)));
        OMR_HIP(hipMemsetAsync(bad.p, 0, sizeof(int32_t), s));
        OMR_HIP(launch_lined_prepare(d_lines + 4 * (int64_t)off[0], total, rows, cols, segs.as<LinedSeg>(), bad.as<int32_t>(), s));
        OMR_HIP(hipMemcpyAsync(&verdict, bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        OMR_HIP(hipStreamSynchronize(s));
        if (verdict) return fail(OMR_ERR_BADARG, "a segment's end point lies outside the %d x %d picture", cols, rows);
    }
    for (int i0 = 0; i0 < n; i0 += 65535) {
        LinedImg p{};
        p.n = std::min(n - i0, 65535);
        p.rows = rows, p.cols = cols;
        p.src = d_edges + i0 * estride, p.sstride = estride, p.sstep = estep;
        p.dst = d_out + i0 * ostride, p.dstride = ostride, p.dstep = ostep;
        p.bgr = (uint32_t)bgr[0] | (uint32_t)bgr[1] << 8 | (uint32_t)bgr[2] << 16;
        OMR_HIP(launch_lined_draw(p, segs.as<LinedSeg>(), doff.as<int32_t>() + i0, s));
    }
    OMR_HIP(hipStreamSynchronize(s));
    return OMR_OK;
}

// a packed device picture as a fresh host image
int picture_to_host(const uint8_t *d_pic, int rows, int cols, hipStream_t s, omr_image_owned *picture)
{
    const size_t row = (size_t)cols * 3;
    uint8_t *data = (uint8_t *)malloc(row * rows);
    if (!data) return fail(OMR_ERR_NOMEM, "out of host memory");
    *picture = omr_image_owned{data, rows, cols, 3, (int64_t)row};
    int rc = staged_d2h(data, d_pic, row * rows, s);
    if (rc) omr_image_free(picture);
    return rc;
}

// ---- get_angle_with_hough for a batch: the segments stay on the device (hough.hip: offsets, pack, vote-and-select)

// every argument rule of omr_hough_angles_batch_device (and of the FFT detectors' batch forms), before any device work
int hough_batch_check(const void *d_scans, int n, int64_t stride, int rows, int cols, int cn, int64_t step, bool have_outputs,
                      const void *d_lined, int64_t lstride, int64_t lstep)
{
    clear_error();
    if (!d_scans || !have_outputs) return fail(OMR_ERR_BADARG, "null pointer");
    if (n <= 0) return fail(OMR_ERR_BADARG, "empty batch");
    int rc = check_image_shape(rows, cols);
    if (rc || (rc = cn_canny(cn))) return rc;
    if (step < (int64_t)cols * cn) return fail(OMR_ERR_BADARG, "step_bytes too small");
    if (stride < 0) return fail(OMR_ERR_BADARG, "negative scan stride");
    if (d_lined) {
        if (lstep < 3 * (int64_t)cols) return fail(OMR_ERR_BADARG, "step too small");
        if (lstride < rows * lstep) return fail(OMR_ERR_BADARG, "picture stride smaller than a picture");
        if (d_lined == d_scans) return fail(OMR_ERR_BADARG, "the picture cannot be made in place");
    }
    return OMR_OK;
}

// Canny -> the kept edges -> the segment stage (hough_host.hpp).  map, flag and rowcnt are released as that stage's buffers
int batch_segments_device(const uint8_t *d_scans, int n, int64_t stride, int64_t step, int rows, int cols, int cn,
                          const HoughParams &hp, bool keep_edges, hipStream_t s, BatchSegments *seg)
{
    const size_t img = (size_t)rows * cols;
    DevBuf map, flag, rowcnt;
    OMR_HIP(map.alloc((size_t)n * img));
    OMR_HIP(flag.alloc(sizeof(int)));
    OMR_HIP(rowcnt.alloc(sizeof(int32_t) * (size_t)n * rows));
    int rc = canny_device(d_scans, stride, step, rows, cols, cn, n, hp.low, hp.high, map.as<uint8_t>(), flag.as<int>(), s,
                          rowcnt.as<int32_t>());
    if (rc) return rc;
    if (keep_edges) {  // the pictures' background: HoughLinesP erases the points it has used from its input
        OMR_HIP(seg->edges.alloc(map.bytes));
        OMR_HIP(hipMemcpyAsync(seg->edges.p, map.p, (size_t)n * img, hipMemcpyDeviceToDevice, s));
    }
    return segments_from_edges(map.as<uint8_t>(), rowcnt.as<int32_t>(), n, rows, cols, hp, s, seg);
}

// the f32 angles of the whole packed list: on the host (libm atan2f / fmodf, as the reference: the device's are not the
// host's bit for bit), then uploaded for the vote.  Enqueues only; nothing to do without a segment
static int segment_angles(const BatchSegments &seg, hipStream_t s, std::vector<float> *ang, DevBuf *d_ang)
{
    const size_t total = seg.total();
    ang->resize(total);
    if (total == 0) return OMR_OK;
    host_fan_out(total, 4096, [&](size_t lo, size_t hi) { line_angles(seg.lines.data() + 4 * lo, hi - lo, ang->data() + lo); });
    OMR_HIP(d_ang->alloc(sizeof(float) * total));
    OMR_HIP(hipMemcpyAsync(d_ang->p, ang->data(), sizeof(float) * total, hipMemcpyHostToDevice, s));
    return OMR_OK;
}

// arguments already checked.  Synchronises `s`.
static int hough_angles_device(const uint8_t *d_scans, int n, int64_t stride, int64_t step, int rows, int cols, int cn,
                               const HoughParams &hp, double *angles, int32_t *rc_out, int32_t *n_lines, uint8_t *d_lined,
                               int64_t lstride, int64_t lstep, hipStream_t s)
{
    PoolScope scope(s);
    const size_t img = (size_t)rows * cols;
    BatchSegments seg;
    int rc = batch_segments_device(d_scans, n, stride, step, rows, cols, cn, hp, d_lined != nullptr, s, &seg);
    if (rc) return rc;
    const std::vector<int32_t> &off = seg.off;
    const DevBuf &edges = seg.edges, &d_off = seg.d_off, &d_packed = seg.d_packed;
    std::vector<int32_t> win((size_t)n, -1);
    std::vector<float> ang;
    DevBuf d_ang, d_win;
    if ((rc = segment_angles(seg, s, &ang, &d_ang))) return rc;
    if (seg.total() > 0) {  // hough.rs:70-92 is vote_select_kernel alone
        OMR_HIP(d_win.alloc(sizeof(int32_t) * (size_t)n));
        OMR_HIP(launch_vote_select(d_ang.as<float>(), d_off.as<int32_t>(), n, d_win.as<int32_t>(), s));
        OMR_HIP(hipMemcpyAsync(win.data(), d_win.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        OMR_HIP(hipStreamSynchronize(s));
    }
    for (int i = 0; i < n; i++) {
        const int32_t o = off[(size_t)i], m = off[(size_t)i + 1] - o;
        if (n_lines) n_lines[i] = m;
        if (m == 0) {  // the per-call form's error: the reference panics on angles[0], hough.rs:74
            angles[i] = 0.0;
            rc_out[i] = OMR_ERR_ASSERT;
            continue;
        }
        if (win[(size_t)i] < 0 || win[(size_t)i] >= m) return fail(OMR_ERR_GPU, "vote_select_kernel: scan %d has no winner", i);
        angles[i] = (double)ang[(size_t)o + (size_t)win[(size_t)i]];
        rc_out[i] = OMR_OK;
    }
    if (!d_lined) return OMR_OK;
    // pictures for the runs of scans that have segments: the slot of a scan without one is not written
    for (int i0 = 0; i0 < n;) {
        if (off[(size_t)i0 + 1] == off[(size_t)i0]) {
            i0++;
            continue;
        }
        int i1 = i0 + 1;
        while (i1 < n && off[(size_t)i1 + 1] > off[(size_t)i1]) i1++;
        if ((rc = lined_device(edges.as<uint8_t>() + (size_t)i0 * img, i1 - i0, (int64_t)img, cols, rows, cols,
                               d_packed.as<int32_t>(), off.data() + i0, kLinedBgr, d_lined + (int64_t)i0 * lstride, lstride,
                               lstep, s)))
            return rc;
        i0 = i1;
    }
    return OMR_OK;
}

// omr.rs's vote stage (hough_host.hpp)
int omr_rs_votes(const BatchSegments &seg, hipStream_t s, std::vector<float> *ang, std::vector<int32_t> *cnt)
{
    const size_t total = seg.total();
    DevBuf d_ang, d_cnt;
    int rc = segment_angles(seg, s, ang, &d_ang);
    if (rc) return rc;
    cnt->resize(total);
    if (total == 0) return OMR_OK;
    OMR_HIP(d_cnt.alloc(sizeof(int32_t) * total));
    OMR_HIP(launch_angle_votes_batch(d_ang.as<float>(), seg.d_off.as<int32_t>(), seg.scans(), seg.max_count(), d_cnt.as<int32_t>(), s));
    OMR_HIP(hipMemcpyAsync(cnt->data(), d_cnt.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    return OMR_OK;
}

// omr.rs:231-302 per scan (hough_host.hpp)
int edges_detection_device(const uint8_t *d_scans, int n, int64_t stride, int64_t step, int rows, int cols, int cn,
                           const HoughParams &hp, double *angles, int32_t *status, int32_t *n_lines, hipStream_t s,
                           double *candidates, int32_t cand_cap, int32_t *cand_len)
{
    PoolScope scope(s);
    BatchSegments seg;
    std::vector<float> ang;
    std::vector<int32_t> cnt;
    int rc = batch_segments_device(d_scans, n, stride, step, rows, cols, cn, hp, false, s, &seg);
    if (rc || (rc = omr_rs_votes(seg, s, &ang, &cnt))) return rc;
    for (int i = 0; i < n; i++) {  // no segment: the reference would panic (quirk B11), select_omr_rs says "not a result"
        const size_t o = (size_t)seg.off[(size_t)i];
        if (n_lines) n_lines[i] = seg.count(i);
        select_omr_rs(ang.data() + o, cnt.data() + o, seg.count(i), &angles[i], status ? &status[i] : nullptr,
                      i == 0 ? candidates : nullptr, cand_cap, i == 0 ? cand_len : nullptr);
    }
    return OMR_OK;
}

int edges_detection_one(const uint8_t *d_src, int rows, int cols, int cn, const HoughParams &hp, hipStream_t s, double *angle,
                        int32_t *status, double *candidates, int32_t cand_cap, int32_t *cand_len)
{
    double a = 0;
    int32_t st = 0, nl = 0, nc = 0;
    std::vector<double> cand((size_t)std::max(cand_cap, 0));
    int rc = edges_detection_device(d_src, 1, 0, (int64_t)cols * cn, rows, cols, cn, hp, &a, &st, &nl, s, cand.data(), cand_cap, &nc);
    if (rc) return rc;
    if (nl == 0) return fail(OMR_ERR_ASSERT, "no line segment found (the reference panics on angles[0], omr.rs:272)");
    *angle = a;
    if (status) *status = st;
    if (cand_len) *cand_len = nc;
    if (candidates) std::copy_n(cand.begin(), std::min(nc, std::max(cand_cap, 0)), candidates);
    return OMR_OK;
}

// pictures -> fresh host images, from several threads, one staged copy each (hough_host.hpp)
int download_pictures(const uint8_t *d_pics, int m, int rows, int cols, const std::vector<int> &members, int j0,
                      const int32_t *skip, omr_image_owned *lined)
{
    const size_t pic = (size_t)cols * 3 * rows;
    return on_threads(m, [&](hipStream_t s, int lo, int hi) -> int {
        for (int j = lo; j < hi; j++) {
            if (skip && skip[j] != OMR_OK) continue;
            if (int rc1 = picture_to_host(d_pics + (size_t)j * pic, rows, cols, s, &lined[members[(size_t)(j0 + j)]])) return rc1;
        }
        return OMR_OK;
    });
}

}  // namespace hh
}  // namespace omr

extern "C" {

int32_t omr_hough_set_scans_in_flight(int32_t scans)
{
    return (int32_t)omr::hh::g_scans_in_flight.exchange(scans < 0 ? 0 : scans);
}

int omr_canny(const omr_image *src, double low_thresh, double high_thresh, omr_image_owned *edges)
{
    clear_error();
    int rc = check_image(src, cn_canny);
    if (rc) return rc;
    if (!edges) return fail(OMR_ERR_BADARG, "null output");
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    DevBuf in, map, flag, rowcnt;
    if ((rc = upload(src, &in, st.s))) return rc;
    OMR_HIP(map.alloc((size_t)src->rows * src->cols));
    OMR_HIP(flag.alloc(sizeof(int)));
    OMR_HIP(rowcnt.alloc(sizeof(int32_t) * (size_t)src->rows));
    if ((rc = canny_device(in.as<uint8_t>(), 0, (int64_t)src->cols * src->channels, src->rows, src->cols, src->channels, 1,
                           low_thresh, high_thresh, map.as<uint8_t>(), flag.as<int>(), st.s, rowcnt.as<int32_t>())))
        return rc;
    edges->rows = src->rows;
    edges->cols = src->cols;
    edges->channels = 1;
    edges->step_bytes = src->cols;
    edges->data = (uint8_t *)malloc((size_t)src->rows * src->cols);
    if (!edges->data) return fail(OMR_ERR_NOMEM, "out of host memory");
    rc = staged_d2h(edges->data, map.p, (size_t)src->rows * src->cols, st.s);
    if (rc) omr_image_free(edges);
    return rc;
}

int omr_hough_lines_p(const omr_image *edges, double rho, double theta, int32_t threshold, double min_line_length,
                      double max_line_gap, int32_t *lines, int32_t cap, int32_t *n_lines)
{
    clear_error();
    int rc = check_image(edges, cn_canny);
    if (rc) return rc;
    if (edges->channels != 1) return fail(OMR_ERR_ASSERT, "HoughLinesP takes an 8-bit single-channel image");
    if (!n_lines || (cap > 0 && !lines)) return fail(OMR_ERR_BADARG, "null output");
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    DevBuf img, rowcnt;
    if ((rc = upload(edges, &img, st.s))) return rc;
    OMR_HIP(rowcnt.alloc(sizeof(int32_t) * (size_t)edges->rows));
    OMR_HIP(launch_edges_rowcount(img.as<uint8_t>(), edges->rows, edges->cols, 1, 0, rowcnt.as<int32_t>(), st.s));
    HoughParams hp = hough_params(min_line_length, max_line_gap);
    hp.rho = rho;
    hp.theta = theta;
    hp.threshold = threshold;
    BatchSegments seg;  // the segment stage's edges half, n = 1
    if ((rc = segments_from_edges(img.as<uint8_t>(), rowcnt.as<int32_t>(), 1, edges->rows, edges->cols, hp, st.s, &seg))) return rc;
    const int n = seg.count(0);
    *n_lines = n;
    if (lines && cap > 0 && n > 0) memcpy(lines, seg.lines.data(), sizeof(int32_t) * 4 * (size_t)std::min(n, (int)cap));
    return OMR_OK;
}

// get_angle_with_hough; `lined` (may be null) receives the picture the reference writes (hough.rs:44-63, :91-96)
static int angle_with_hough(const omr_image *gray, double min_line_length, double max_line_gap, double *angle_out,
                            omr_image_owned *lined)
{
    clear_error();
    if (lined) memset(lined, 0, sizeof(*lined));
    int rc = check_image(gray, cn_canny);
    if (rc) return rc;
    if (!angle_out) return fail(OMR_ERR_BADARG, "null output");
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    const int rows = gray->rows, cols = gray->cols;
    const int64_t pic = (int64_t)cols * 3 * rows;
    DevBuf in, d_pic;
    if ((rc = upload(gray, &in, st.s))) return rc;
    if (lined) OMR_HIP(d_pic.alloc((size_t)pic));
    double angle = 0.0;
    int32_t code = OMR_OK;
    if ((rc = hough_angles_device(in.as<uint8_t>(), 1, 0, (int64_t)cols * gray->channels, rows, cols, gray->channels,
                                  hough_params(min_line_length, max_line_gap), &angle, &code, nullptr, d_pic.as<uint8_t>(), pic,
                                  (int64_t)cols * 3, st.s)))
        return rc;
    if (code)  // the reference panics before its imwrite: no picture
        return fail(code, "no line segment found (the reference panics on angles[0], hough.rs:74)");
    *angle_out = angle;
    return lined ? picture_to_host(d_pic.as<uint8_t>(), rows, cols, st.s, lined) : OMR_OK;
}

int omr_get_angle_with_hough(const omr_image *gray, double min_line_length, double max_line_gap, double *angle_out)
{
    return angle_with_hough(gray, min_line_length, max_line_gap, angle_out, nullptr);
}

int omr_get_angle_with_hough_ex(const omr_image *gray, double min_line_length, double max_line_gap, double *angle_out,
                                omr_image_owned *lined)
{
    return angle_with_hough(gray, min_line_length, max_line_gap, angle_out, lined);
}

int omr_hough_angles_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows, int32_t cols,
                                  int32_t channels, int64_t step_bytes, double min_line_length, double max_line_gap,
                                  double *angles, int32_t *rc, int32_t *n_lines, uint8_t *d_lined, int64_t lined_stride_bytes,
                                  int64_t lined_step, void *stream)
{
    int err = hough_batch_check(d_scans, n, scan_stride_bytes, rows, cols, channels, step_bytes, angles && rc, d_lined,
                                lined_stride_bytes, lined_step);
    if (err || (err = have_device())) return err;
    return hough_angles_device(d_scans, n, scan_stride_bytes, step_bytes, rows, cols, channels,
                               hough_params(min_line_length, max_line_gap), angles, rc, n_lines, d_lined, lined_stride_bytes,
                               lined_step, (hipStream_t)stream);
}

// the Hough leg of the reference's benchmark on device-resident scans: gray, this file's batch detector, rotate_mat of the
// originals (detector_deskew.cpp)
int omr_hough_deskew_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows, int32_t cols,
                                  int32_t channels, int64_t step_bytes, double min_line_length, double max_line_gap, int32_t flags,
                                  int32_t border_mode, const uint8_t border_value[4], int32_t clip, uint8_t *d_out,
                                  int64_t out_stride_bytes, int64_t out_step_bytes, int32_t *out_size, double *angles, int32_t *rc,
                                  int32_t *n_lines, void *stream)
{
    Detector d;
    d.min_line_length = min_line_length, d.max_line_gap = max_line_gap;
    return detector_deskew_device(d, d_scans, n, scan_stride_bytes, rows, cols, channels, step_bytes, flags, border_mode, border_value,
                                  clip, d_out, out_stride_bytes, out_step_bytes, out_size, angles, rc, n_lines, (hipStream_t)stream);
}

int omr_hough_vote_select_device(const float *d_angles, const int32_t *d_offsets, int32_t n, int32_t *d_winner, void *stream)
{
    clear_error();
    if (!d_angles || !d_offsets || !d_winner) return fail(OMR_ERR_BADARG, "null pointer");
    if (n <= 0) return fail(OMR_ERR_BADARG, "empty batch");
    int rc = have_device();
    if (rc) return rc;
    OMR_HIP(launch_vote_select(d_angles, d_offsets, n, d_winner, (hipStream_t)stream));
    return OMR_OK;
}

// one bucket of omr_get_angles_with_hough_batch: `members` index same-shape images of `grays`; at most HB_SCANS go to the
// device at a time (an A4 gray scan holds about 60 MB there with its edge maps, accumulator and picture).  Uploads and
// picture downloads run on several host threads (host_threads.hpp), as in the other host batches
static int hough_host_bucket(const omr_image *grays, const std::vector<int> &members, const HoughParams &hp, double *angles,
                             int32_t *rcs, omr_image_owned *lined)
{
    constexpr int HB_SCANS = 64;
    const omr_image &first = grays[members[0]];
    const int rows = first.rows, cols = first.cols, cn = first.channels;
    const int64_t row = (int64_t)cols * cn, img = row * rows, pic = (int64_t)cols * 3 * rows;
    LeasedStream st;
    int rc = st.create();
    if (rc) return rc;
    const int total = (int)members.size(), zmax = std::min(HB_SCANS, total);
    DevBuf in, pics;
    OMR_HIP(in.alloc((size_t)img * zmax));
    if (lined) OMR_HIP(pics.alloc((size_t)pic * zmax));
    std::vector<double> a((size_t)zmax);
    std::vector<int32_t> r((size_t)zmax);
    for (int j0 = 0; j0 < total; j0 += zmax) {
        const int m = std::min(zmax, total - j0);
        if ((rc = upload_chunk(grays, members, j0, m, rows, row, in.as<uint8_t>(), img))) return rc;
        if ((rc = hough_angles_device(in.as<uint8_t>(), m, img, row, rows, cols, cn, hp, a.data(), r.data(), nullptr,
                                      lined ? pics.as<uint8_t>() : nullptr, pic, (int64_t)cols * 3, st.s)))
            return rc;
        for (int j = 0; j < m; j++) {
            angles[members[(size_t)(j0 + j)]] = a[(size_t)j];
            rcs[members[(size_t)(j0 + j)]] = r[(size_t)j];
        }
        if (!lined) continue;
        rc = download_pictures(pics.as<uint8_t>(), m, rows, cols, members, j0, r.data(), lined);
        if (rc) return rc;
    }
    return OMR_OK;
}

int omr_get_angles_with_hough_batch(const omr_image *grays, int32_t n, double min_line_length, double max_line_gap,
                                    double *angles, int32_t *rc, omr_image_owned *lined)
{
    clear_error();
    if (!grays || n < 1 || !angles || !rc) return fail(OMR_ERR_BADARG, "bad batch arguments");
    if (lined) memset(lined, 0, sizeof(*lined) * (size_t)n);
    ShapeBuckets b;
    // omr_get_angle_with_hough's checks, for every image before any device work
    int err = bucket_by_shape(grays, n, [](const omr_image &im) { return check_image(&im, cn_canny); }, &b);
    if (err || (err = have_device())) return err;
    const HoughParams hp = hough_params(min_line_length, max_line_gap);
    // angles and codes go to the caller's arrays only when the whole call has succeeded
    std::vector<double> ang((size_t)n);
    std::vector<int32_t> rcs((size_t)n);
    for (size_t k = 0; k < b.shapes.size() && err == OMR_OK; k++)
        err = hough_host_bucket(grays, b.members[k], hp, ang.data(), rcs.data(), lined);
    if (err) {
        if (lined)
            for (int i = 0; i < n; i++) omr_image_free(&lined[i]);
        return err;
    }
    memcpy(angles, ang.data(), sizeof(double) * (size_t)n);
    memcpy(rc, rcs.data(), sizeof(int32_t) * (size_t)n);
    return OMR_OK;
}

int omr_lined_picture_batch_device(const uint8_t *d_edges, int32_t n, int64_t edge_stride_bytes, int64_t edge_step,
                                   int32_t rows, int32_t cols, const int32_t *d_lines, const int32_t *line_offsets,
                                   const uint8_t bgr[3], uint8_t *d_out, int64_t out_stride_bytes, int64_t out_step,
                                   void *stream)
{
    int rc = lined_check(d_edges, n, edge_stride_bytes, edge_step, rows, cols, d_lines, line_offsets, bgr, d_out,
                         out_stride_bytes, out_step, true);
    if (rc || (rc = have_device())) return rc;
    return lined_device(d_edges, n, edge_stride_bytes, edge_step, rows, cols, d_lines, line_offsets, bgr, d_out,
                        out_stride_bytes, out_step, (hipStream_t)stream);
}

int omr_lined_picture_device(const uint8_t *d_edges, int64_t edge_step, int32_t rows, int32_t cols, const int32_t *d_lines,
                             int32_t n_lines, const uint8_t bgr[3], uint8_t *d_out, int64_t out_step, void *stream)
{
    const int32_t off[2] = {0, n_lines};
    int rc = lined_check(d_edges, 1, 0, edge_step, rows, cols, d_lines, off, bgr, d_out, 0, out_step, false);
    if (rc || (rc = have_device())) return rc;
    return lined_device(d_edges, 1, 0, edge_step, rows, cols, d_lines, off, bgr, d_out, 0, out_step, (hipStream_t)stream);
}

int omr_lined_picture(const omr_image *edges, const int32_t *lines, int32_t n_lines, const uint8_t bgr[3],
                      omr_image_owned *picture)
{
    clear_error();
    int rc = check_image(edges, cn_one);
    if (rc) return rc;
    if (!picture || !bgr) return fail(OMR_ERR_BADARG, "null pointer");
    if (n_lines < 0 || (n_lines > 0 && !lines)) return fail(OMR_ERR_BADARG, "negative segment count or null segment list");
    for (int64_t i = 0; i < 4 * (int64_t)n_lines; i++)
        if (lines[i] < 0 || lines[i] >= ((i & 1) ? edges->rows : edges->cols))
            return fail(OMR_ERR_BADARG, "end point of segment %lld lies outside the %d x %d picture", (long long)(i / 4),
                        edges->cols, edges->rows);
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    const int32_t off[2] = {0, n_lines};
    DevBuf in, d_lines, d_pic;
    if ((rc = upload(edges, &in, st.s))) return rc;
    if (n_lines > 0) {
        OMR_HIP(d_lines.alloc(sizeof(int32_t) * 4 * (size_t)n_lines));
        OMR_HIP(hipMemcpyAsync(d_lines.p, lines, sizeof(int32_t) * 4 * (size_t)n_lines, hipMemcpyHostToDevice, st.s));
    }
    OMR_HIP(d_pic.alloc((size_t)edges->cols * 3 * edges->rows));
    if ((rc = lined_device(in.as<uint8_t>(), 1, 0, edges->cols, edges->rows, edges->cols, d_lines.as<int32_t>(), off, bgr,
                           d_pic.as<uint8_t>(), 0, (int64_t)edges->cols * 3, st.s)))
        return rc;
    return picture_to_host(d_pic.as<uint8_t>(), edges->rows, edges->cols, st.s, picture);
}

int omr_get_result_from_edges_detection(const omr_image *src, double edges_min_line_length, double edges_max_line_gap,
                                        double *angle, int32_t *status, double *candidates, int32_t cand_cap,
                                        int32_t *cand_len)
{
    clear_error();
    int rc = check_image(src, cn_canny);
    if (rc) return rc;
    if (!angle) return fail(OMR_ERR_BADARG, "null output");
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    DevBuf in;
    if ((rc = upload(src, &in, st.s))) return rc;
    return edges_detection_one(in.as<uint8_t>(), src->rows, src->cols, src->channels,
                               hough_params(edges_min_line_length, edges_max_line_gap), st.s, angle, status, candidates, cand_cap,
                               cand_len);
}

int omr_edges_detection_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows,
                                     int32_t cols, int32_t channels, int64_t step_bytes, double min_line_length,
                                     double max_line_gap, double *angles, int32_t *status, int32_t *n_lines, void *stream)
{
    int rc = hough_batch_check(d_scans, n, scan_stride_bytes, rows, cols, channels, step_bytes, angles != nullptr, nullptr, 0, 0);
    if (rc || (rc = have_device())) return rc;
    return edges_detection_device(d_scans, n, scan_stride_bytes, step_bytes, rows, cols, channels,
                                  hough_params(min_line_length, max_line_gap), angles, status, n_lines, (hipStream_t)stream);
}

// omr.rs:351-399
void omr_correct_default_decision(double proj_angle, int32_t proj_status, const double *proj_candidates, int32_t n_cand,
                                  double edges_angle, double *rotate_angle, int32_t *need_check)
{
    if (proj_status == OMR_STATUS_BELIEVED) {
        *rotate_angle = proj_angle;
        *need_check = 0;
    } else if (proj_status == OMR_STATUS_NEED_CHECK) {
        const bool far = fabs(proj_angle - edges_angle) >= 0.1;
        *rotate_angle = far ? edges_angle : proj_angle;
        *need_check = far ? 1 : 0;
    } else {
        int bi = -1;
        for (int i = 0; i < n_cand; i++)  // min_by keeps the first minimum
            if (bi < 0 || fabs(proj_candidates[i] - edges_angle) < fabs(proj_candidates[bi] - edges_angle)) bi = i;
        if (bi >= 0 && fabs(proj_candidates[bi] - edges_angle) < 0.05) {
            *rotate_angle = proj_candidates[bi];
            *need_check = 0;
        } else {
            *rotate_angle = edges_angle;
            *need_check = 1;
        }
    }
}

int omr_correct_default(const omr_image *src, uint16_t projection_max_angle, double projection_angle_step,
                        int32_t projection_max_width, int32_t projection_max_height, double hough_min_line_length,
                        double hough_max_line_gap, double *rotate_angle, int32_t *need_check, omr_image_owned *rotated)
{
    clear_error();
    if (!rotate_angle || !need_check) return fail(OMR_ERR_BADARG, "null output");
    int rc = check_image(src, cn_canny);
    if (rc) return rc;
    double pa = 0;
    int32_t pst = 0, pn = 0;
    int32_t n_half = 0;
    const int n_cand = omr_candidate_count(projection_max_angle, projection_angle_step, &n_half);  // candidates <= sweep angles
    if (n_cand <= 0) return fail(OMR_ERR_BADARG, "empty candidate range");
    std::vector<double> pc((size_t)n_cand + 1);
    if (src->channels == 2) return fail(OMR_ERR_ASSERT, "RGB2GRAY needs 3 or 4 channels");
    if ((rc = have_device())) return rc;
    // the sheet goes to the device once; projection, the Hough fallback and the final warp all read that copy
    LeasedStream st;
    if ((rc = st.create())) return rc;
    DevBuf in;
    if ((rc = upload(src, &in, st.s))) return rc;
    const uint8_t *d_src = in.as<uint8_t>();
    rc = omr::result_from_projection_device(d_src, src->rows, src->cols, src->channels, projection_max_angle,
                                            projection_angle_step, projection_max_width, projection_max_height, st.s, &pa,
                                            &pst, pc.data(), (int32_t)pc.size(), &pn);
    if (rc) return rc;
    if (pst == OMR_STATUS_BELIEVED) {
        *rotate_angle = pa;
        *need_check = 0;
    } else {  // omr.rs:361-402
        double ea = 0;
        if ((rc = edges_detection_one(d_src, src->rows, src->cols, src->channels, hough_params(hough_min_line_length, hough_max_line_gap),
                                      st.s, &ea, nullptr, nullptr, 0, nullptr)))
            return rc;
        omr_correct_default_decision(pa, pst, pc.data(), std::min<int32_t>(pn, (int32_t)pc.size()), ea, rotate_angle,
                                     need_check);
    }
    if (rotated) {  // omr.rs:404-445: CONTAIN canvas, nearest neighbour, white border, scale 1
        const uint8_t white[4] = {255, 255, 255, 0};
        rc = omr::rotate_device_to_host(d_src, src->rows, src->cols, src->channels, *rotate_angle, 1.0, OMR_INTER_NEAREST, white,
                                        OMR_CLIP_CONTAIN, st.s, rotated);
    }
    return rc;
}

}  // extern "C"

#ifdef OMR_RUNS_DEBUG
extern "C" int omr_debug_ppht_stamps(unsigned long long *out12, int reset)
{
    OMR_HIP(omr::debug_ppht_stamps(out12, reset != 0));
    return OMR_OK;
}
#endif
