// correct_batch.cpp -- correct_default (omr.rs:339-448) for batches of sheets on the device:
//
//   front end   one launch per stage over the batch: gray + erode x3 (+ integer INTER_AREA shrink) fused
//               (correct_front.hip); every other resize() path on the eroded sheets, a launch per chunk (resize.hip) --
//               fractional shrinks with the context's resizeArea_ tap tables, enlargement (quirk B7) bilinear
//   sweep       the context's omr_batch_ctx at the resize scale (quirk B4), black_max 127 (omr.rs:129-139); the scores
//               go to the host, where omr_select_projection_result decides every sheet (omr.rs:147-221)
//   Hough       only the sheets that are not Believed: one batched Canny + HoughLinesP pass on a gather of their
//               colour sheets with its omr.rs vote (edges_detection_device), then the omr.rs:351-399 decision per sheet
//   warp        the batch colour warp (deskew.hip) with a per-call candidate set made of the decided angles: NEAREST,
//               white border, CONTAIN, scale 1.  The Believed sheets' warp runs on a stream of its own while the Hough
//               pass runs.
//
// Every per-sheet result is omr_correct_default's for the same sheet, bit for bit.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/omrdeskew.h"
#include "encode_any.hpp"
#include "engine.hpp"
#include "flow_frame.hpp"
#include "hough_host.hpp"
#include "host_threads.hpp"
#include "jpeg_dec.hpp"
#include "orient.hpp"
#include "png_dec.hpp"
#include "stream_sink.hpp"

using namespace omr;
using namespace omr::hh;

namespace {

// the front-end modes (include/omrdeskew.h, OMR_CORRECT_FRONT_*)
enum FrontMode {
    FRONT_AREA_FUSED = OMR_CORRECT_FRONT_AREA_FUSED,  // integer factors <= 64: gray + erode + resizeAreaFast_ in one kernel
    FRONT_AREA_INT = OMR_CORRECT_FRONT_AREA_INT,      // integer factors > 64: eroded sheets, then resizeAreaFast_
    FRONT_AREA_GENERAL = OMR_CORRECT_FRONT_AREA_GENERAL,  // fractional shrink: eroded sheets, then resizeArea_ (tap tables)
    FRONT_LINEAR = OMR_CORRECT_FRONT_LINEAR,  // an axis enlarges (quirk B7): eroded sheets, then the bilinear kernel
};
const int kChunk = 256;  // sheets per front-end / warp launch when a full-size intermediate is needed

// the decided angles of one warp phase as a candidate set of the batch warp
struct WarpSet {
    DeskewTables tab;
    DevBuf best, tiles;
    std::vector<double> angles;  // the distinct ones
    std::vector<int32_t> h_best;
};

// Largest CONTAIN canvas over every angle: ceil(rows |sin| + cols |cos|) <= ceil(sqrt(rows^2 + cols^2)) on both axes,
// and floor(sqrt) + 1 bounds that with room for the rounding of the f64 expression.  Cols rounded up to 4 (the warp's
// tables).
void canvas_of(int rows, int cols, int *R, int *C)
{
    const int64_t d2 = (int64_t)rows * rows + (int64_t)cols * cols;
    int64_t r = (int64_t)sqrt((double)d2);
    while (r * r > d2) r--;
    while ((r + 1) * (r + 1) <= d2) r++;
    *R = (int)(r + 1);
    *C = (int)((r + 1 + 3) & ~3);
}

}  // namespace

struct omr_correct_batch {
    int device = 0, rows = 0, cols = 0, cn = 0, max_scans = 0;
    uint16_t max_angle = 0;
    double step = 0, hough_min = 0, hough_gap = 0;
    int N = 0, A = 0;
    double scale = 1;
    int dr = 0, dc = 0;  // projection-size image
    ResizeDispatch rd{ResizeDispatch::COPY, false, 1, 1};  // resize()'s path from rows x cols to dr x dc
    int mode = FRONT_AREA_FUSED;                           // the same as omr_correct_batch_info reports it
    int64_t small_step = 0, small_stride = 0, er_stride = 0;
    int DR = 0, DC = 0;  // largest canvas
    omr_batch_ctx *sweep = nullptr;
    hipStream_t s = nullptr, sw = nullptr;  // front end / sweep hand-off / Hough, and the warp
    DevBuf small, eroded, best, vsd, hsd, gather;
    AreaTables area;  // FRONT_AREA_GENERAL
    double *h_vsd = nullptr, *h_hsd = nullptr;  // pinned
    WarpSet warp[2];                            // [0] Believed sheets, [1] the rest
    std::mutex mu;
    ~omr_correct_batch()
    {
        if (s) (void)hipStreamSynchronize(s);
        if (sw) (void)hipStreamSynchronize(sw);
        if (sweep) omr_batch_destroy(sweep);
        if (h_vsd) (void)hipHostFree(h_vsd);
        if (h_hsd) (void)hipHostFree(h_hsd);
        if (s) (void)hipStreamDestroy(s);
        if (sw) (void)hipStreamDestroy(sw);
    }
};

namespace {

// resize()'s dispatch for INTER_AREA from rows x cols to dr x dc, and the front-end mode it means
void front_mode(omr_correct_batch *cb)
{
    const ResizeDispatch d = cb->rd = resize_dispatch(cb->rows, cb->cols, cb->dr, cb->dc, OMR_INTER_AREA);
    switch (d.kind) {
    case ResizeDispatch::COPY:  // resizeAreaFast_ with factor 1 is the identity
    case ResizeDispatch::AREA_INT:
        cb->mode = d.kx <= 64 && d.ky <= 64 ? FRONT_AREA_FUSED : FRONT_AREA_INT;
        break;
    case ResizeDispatch::LINEAR: cb->mode = FRONT_LINEAR; break;
    case ResizeDispatch::AREA_GENERAL: cb->mode = FRONT_AREA_GENERAL; break;
    }
}

int upload_vec(DevBuf *b, const void *p, size_t bytes, hipStream_t s)
{
    int rc = grow(b, bytes);
    if (rc) return rc;
    OMR_HIP(hipMemcpyAsync(b->p, p, bytes, hipMemcpyHostToDevice, s));
    return OMR_OK;
}

// Rotate the listed sheets (ascending) by angle[i] on stream s: the distinct angles become the candidate set of the batch
// warp, sheet i's entry best[i].  Sizes go to out_size (host, may be NULL).
int warp_phase(omr_correct_batch *cb, WarpSet &w, const std::vector<int> &sheets, const double *angle, const uint8_t *d_scans,
               int64_t scan_stride, int64_t step, uint8_t *d_out, int64_t out_stride, int64_t out_step, int32_t *out_size,
               hipStream_t s)
{
    if (sheets.empty()) return OMR_OK;
    std::map<uint64_t, int> index;  // angle bits -> candidate
    w.angles.clear();
    w.h_best.assign((size_t)cb->max_scans, 0);
    for (int i : sheets) {
        uint64_t bits;
        memcpy(&bits, &angle[i], sizeof bits);
        auto it = index.find(bits);
        if (it == index.end()) {
            it = index.emplace(bits, (int)index.size()).first;
            w.angles.push_back(angle[i]);
        }
        w.h_best[(size_t)i] = it->second;
    }
    DeskewTables &t = w.tab;
    int rc = t.plan(cb->rows, cb->cols, w.angles.data(), (int)w.angles.size());
    if (rc) return rc;
    if (t.rows > cb->DR || t.cols > cb->DC)
        return fail(OMR_ERR_ASSERT, "canvas %d x %d exceeds the context's %d x %d", t.rows, t.cols, cb->DR, cb->DC);
    if (out_size)
        for (int i : sheets) memcpy(&out_size[2 * (size_t)i], &t.h_size[2 * (size_t)w.h_best[(size_t)i]], 2 * sizeof(int32_t));
    t.rows = cb->DR, t.cols = cb->DC;  // tables and tiles of the context's canvas whatever the angles: the buffers grow once
    if ((rc = upload_vec(&w.best, w.h_best.data(), sizeof(int32_t) * w.h_best.size(), s))) return rc;
    if ((rc = t.upload(s))) return rc;
    DeskewPass p = t.pass();
    p.scan_stride = scan_stride;
    p.sstep = step;
    p.srows = cb->rows;
    p.scols = cb->cols;
    p.out_stride = out_stride;
    p.dstep = out_step;
    p.border = cb->cn == 1 ? 255 : 0xffffff;  // omr.rs:438: Scalar(255, 255, 255, 0)
    p.cn = cb->cn;
    if ((rc = grow(&w.tiles, deskew_tile_bytes(p, kChunk)))) return rc;
    // one launch per run of consecutive sheets (at most kChunk of them)
    for (size_t j = 0; j < sheets.size();) {
        size_t e = j + 1;
        while (e < sheets.size() && sheets[e] == sheets[e - 1] + 1 && (int)(e - j) < kChunk) e++;
        const int i0 = sheets[j];
        p.src = d_scans + (size_t)i0 * scan_stride;
        p.dst = d_out + (size_t)i0 * out_stride;
        p.best = w.best.as<int32_t>() + i0;
        OMR_HIP(launch_deskew_warp(p, (int)(e - j), OMR_INTER_NEAREST, w.tiles.p, s));
        j = e;
    }
    return OMR_OK;
}

// the front end of n sheets -> cb->small (projection-size images)
int front_end(omr_correct_batch *cb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n)
{
    hipStream_t s = cb->s;
    if (cb->mode == FRONT_AREA_FUSED) {
        OMR_HIP(launch_front(d_scans, scan_stride, step, cb->cn, cb->rows, cb->cols, n, cb->small.as<uint8_t>(), cb->small_stride,
                             cb->small_step, cb->rd.kx, cb->rd.ky, s));
        return OMR_OK;
    }
    for (int i0 = 0; i0 < n; i0 += kChunk) {
        const int z = std::min(kChunk, n - i0);
        int rc = grow(&cb->eroded, (size_t)z * cb->er_stride);
        if (rc) return rc;
        uint8_t *er = cb->eroded.as<uint8_t>();
        uint8_t *sm = cb->small.as<uint8_t>() + (size_t)i0 * cb->small_stride;
        OMR_HIP(launch_front(d_scans + (size_t)i0 * scan_stride, scan_stride, step, cb->cn, cb->rows, cb->cols, z, er, cb->er_stride,
                             cb->cols, 0, 0, s));
        ResizeImgs im{};
        im.src = er, im.scan_stride = cb->er_stride, im.sstep = cb->cols;
        im.dst = sm, im.out_stride = cb->small_stride, im.dstep = cb->small_step;
        im.cn = 1, im.srows = cb->rows, im.scols = cb->cols, im.drows = cb->dr, im.dcols = cb->dc;
        OMR_HIP(launch_resize(cb->rd, im, z, s, cb->area.taps()));
    }
    return OMR_OK;
}

int run_locked(omr_correct_batch *cb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n, double *rotate_angle,
               int32_t *need_check, int32_t *scan_rc, uint8_t *d_out, int64_t out_stride, int64_t out_step, int32_t *out_size)
{
    const int A = cb->A;
    int rc;
    // 1. front end -> projection-size images
    if ((rc = front_end(cb, d_scans, scan_stride, step, n))) return rc;
    OMR_HIP(hipStreamSynchronize(cb->s));  // the sweep runs on the batch context's own streams
    // 2. sweep at the resize scale, scores to the host, omr.rs:147-221 per sheet
    if ((rc = omr_batch_run_device(cb->sweep, cb->small.as<uint8_t>(), cb->small_stride, cb->small_step, n, 127,
                                   cb->best.as<int32_t>(), cb->vsd.as<double>(), cb->hsd.as<double>())))
        return rc;
    if ((rc = omr_batch_sync(cb->sweep))) return rc;
    OMR_HIP(hipMemcpyAsync(cb->h_vsd, cb->vsd.p, sizeof(double) * (size_t)n * A, hipMemcpyDeviceToHost, cb->s));
    OMR_HIP(hipMemcpyAsync(cb->h_hsd, cb->hsd.p, sizeof(double) * (size_t)n * A, hipMemcpyDeviceToHost, cb->s));
    OMR_HIP(hipStreamSynchronize(cb->s));
    std::vector<double> pa((size_t)n), pc((size_t)n * (A + 1));
    std::vector<int32_t> pst((size_t)n), pn((size_t)n);
    std::vector<int> believed, rest;
    for (int i = 0; i < n; i++) {
        if ((rc = omr_select_projection_result(cb->h_vsd + (size_t)i * A, cb->h_hsd + (size_t)i * A, A, cb->N, cb->step, &pa[i],
                                               &pst[i], &pc[(size_t)i * (A + 1)], A + 1, &pn[i])))
            return rc;
        scan_rc[i] = OMR_OK;
        if (pst[i] == OMR_STATUS_BELIEVED) {
            rotate_angle[i] = pa[i];
            need_check[i] = 0;
            believed.push_back(i);
        } else {
            rest.push_back(i);
        }
        if (out_size) out_size[2 * (size_t)i] = out_size[2 * (size_t)i + 1] = 0;
    }
    // 3. the Believed sheets' warp, on its own stream, beside the Hough pass
    if (d_out && (rc = warp_phase(cb, cb->warp[0], believed, rotate_angle, d_scans, scan_stride, step, d_out, out_stride, out_step,
                                  out_size, cb->sw)))
        return rc;
    // 4. Hough on a gather of the other sheets (packed, at most kChunk at a time), omr.rs:351-399 per sheet
    if (!rest.empty()) {
        const int64_t row = (int64_t)cb->cols * cb->cn, gstride = row * cb->rows;
        const HoughParams hp = hough_params(cb->hough_min, cb->hough_gap);
        std::vector<int> decided;
        for (size_t j0 = 0; j0 < rest.size(); j0 += kChunk) {
            const int m = (int)std::min(rest.size() - j0, (size_t)kChunk);
            if ((rc = grow(&cb->gather, (size_t)m * gstride))) return rc;
            for (int j = 0; j < m; j++)
                OMR_HIP(hipMemcpy2DAsync(cb->gather.as<uint8_t>() + (size_t)j * gstride, (size_t)row,
                                         d_scans + (size_t)rest[j0 + j] * scan_stride, (size_t)step, (size_t)row, (size_t)cb->rows,
                                         hipMemcpyDeviceToDevice, cb->s));
            std::vector<double> ea((size_t)m);
            std::vector<int32_t> nl((size_t)m), sheet_rc((size_t)m, OMR_OK);
            uint8_t *g = cb->gather.as<uint8_t>();
            // the pass's own buffers come from the block cache: edges_detection_device holds a PoolScope on cb->s
            rc = edges_detection_device(g, m, gstride, row, cb->rows, cb->cols, cb->cn, hp, ea.data(), nullptr, nl.data(), cb->s);
            if (rc == OMR_ERR_NOMEM)  // a sheet with more segments than the buffer holds: the per-call function fails on that
                for (int j = 0; j < m; j++) {  // sheet alone, so the chunk is redone sheet by sheet, the same stages with n = 1
                    rc = edges_detection_device(g + (size_t)j * gstride, 1, gstride, row, cb->rows, cb->cols, cb->cn, hp, &ea[(size_t)j],
                                                nullptr, &nl[(size_t)j], cb->s);
                    if (rc == OMR_ERR_NOMEM) sheet_rc[(size_t)j] = rc, rc = OMR_OK;
                    if (rc) return rc;
                }
            if (rc) return rc;
            for (int j = 0; j < m; j++) {
                const int i = rest[j0 + j];
                if (sheet_rc[(size_t)j] == OMR_OK && nl[(size_t)j] == 0) sheet_rc[(size_t)j] = OMR_ERR_ASSERT;  // no segment: -215 (quirk B11)
                if (sheet_rc[(size_t)j] != OMR_OK) {
                    scan_rc[i] = sheet_rc[(size_t)j];
                    rotate_angle[i] = 0.0;
                    need_check[i] = 0;
                    continue;
                }
                omr_correct_default_decision(pa[i], pst[i], &pc[(size_t)i * (A + 1)], std::min<int32_t>(pn[i], A + 1), ea[(size_t)j],
                                             &rotate_angle[i], &need_check[i]);
                decided.push_back(i);
            }
        }
        clear_error();
        // 5. their warp, behind the Believed sheets' on the warp stream
        if (d_out && (rc = warp_phase(cb, cb->warp[1], decided, rotate_angle, d_scans, scan_stride, step, d_out, out_stride,
                                      out_step, out_size, cb->sw)))
            return rc;
    }
    OMR_HIP(hipStreamSynchronize(cb->sw));
    return OMR_OK;
}

// the sheet arguments of omr_correct_batch_run_device / _front_device
int check_sheets(omr_correct_batch *cb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n)
{
    if (!cb || !d_scans) return fail(OMR_ERR_BADARG, "null argument");
    if (n < 1 || n > cb->max_scans) return fail(OMR_ERR_BADARG, "n = %d outside 1..max_scans (%d)", n, cb->max_scans);
    if (step < (int64_t)cb->cols * cb->cn) return fail(OMR_ERR_BADARG, "step_bytes < cols x channels");
    if (scan_stride < (int64_t)cb->rows * step) return fail(OMR_ERR_BADARG, "scan_stride_bytes < rows x step_bytes");
    return OMR_OK;
}

}  // namespace

namespace {

// ---- contexts kept per (device, shape, parameters) -------------------------------------------------------------------
struct CtxKey {
    int device, rows, cols, cn;
    uint16_t max_angle;
    double step;
    int32_t max_w, max_h;
    double hmin, hgap;
    bool operator==(const CtxKey &o) const
    {
        return device == o.device && rows == o.rows && cols == o.cols && cn == o.cn && max_angle == o.max_angle &&
               step == o.step && max_w == o.max_w && max_h == o.max_h && hmin == o.hmin && hgap == o.hgap;
    }
};
ContextCache<CtxKey, omr_correct_batch> g_ctx(4);

// a context of kAnglesChunk sheets for this key: from the cache, or made and cached
int cached_context(const CtxKey &k, std::shared_ptr<omr_correct_batch> *out)
{
    return g_ctx.get(k, [&](std::shared_ptr<omr_correct_batch> *sp) -> int {
        omr_correct_batch *raw = nullptr;
        int rc = omr_correct_batch_create(k.rows, k.cols, k.cn, k.max_angle, k.step, k.max_w, k.max_h, k.hmin, k.hgap, k.device,
                                          kAnglesChunk, &raw);
        if (rc == OMR_OK) sp->reset(raw, omr_correct_batch_destroy);
        return rc;
    }, out);
}

// ---- the batch forms: the frame's walk (flow_frame.hpp) with this flow's few answers -------------------------------------
struct Correct {
    uint16_t max_angle;
    double step;
    int32_t max_w, max_h;
    double hmin, hgap;
};

Flow correct_flow(const Correct &a)
{
    Flow f;
    f.writes_early = true;
    f.extra_refused = 0;  // need_check of a sheet with a code
    f.accept = f.accept_parsed = [](const omr_image &im) { return check_image(&im, cn_correct_batch); };
    f.canvas = [](int rows, int cols, int *R, int *C) {
        canvas_of(rows, cols, R, C);
        return (int)OMR_OK;
    };
    f.open = [a](int rows, int cols, int cn, bool, FlowBucket *b) -> int {
        int dev = 0;
        OMR_HIP(hipGetDevice(&dev));
        std::shared_ptr<omr_correct_batch> cb;
        int rc = cached_context(CtxKey{dev, rows, cols, cn, a.max_angle, a.step, a.max_w, a.max_h, a.hmin, a.hgap}, &cb);
        if (rc == OMR_ERR_ASSERT) {  // the projection size truncates to 0 x n: the per-call function fails on each of these sheets
            clear_error();
            b->how = FlowBucket::ALL_CODE, b->code = rc;
            return OMR_OK;
        }
        if (rc) return rc;
        b->chunk = kAnglesChunk, b->canvas_rows = cb->DR, b->canvas_cols = cb->DC, b->out_step = (int64_t)cb->DC * cn;
        b->ctx = cb;
        return OMR_OK;
    };
    f.run = [](const FlowBucket &b, const FlowSlots &s, double *ang, int32_t *chk, int32_t *src, int32_t *size) -> int {
        return omr_correct_batch_run_device(static_cast<omr_correct_batch *>(b.ctx.get()), s.din, s.in_stride, s.row, s.z, ang, chk, src, s.dout,
                                            s.out_stride, s.out_step, size);
    };
    return f;
}

// omr_correct_default_batch and its JPEG and PNG forms: `rotated` (may be null) receives the canvases, or `out` / `out_len`
// (null for the plain form) their streams
int correct_default_host(const omr_image *srcs, int32_t n, const Correct &a, double *rotate_angle, int32_t *need_check,
                         int32_t *scan_rc, omr_image_owned *rotated, uint8_t **out, int64_t *out_len, const OutFormat &fmt)
{
    if (!srcs || n < 1 || !rotate_angle || !need_check || !scan_rc) return fail(OMR_ERR_BADARG, "bad batch arguments");
    FlowSink sink;
    if (out) sink.kind = FlowSink::STREAMS, sink.fmt = fmt;
    else if (rotated) sink.kind = FlowSink::CANVASES;
    FlowOut to;
    to.angle = rotate_angle, to.extra = need_check, to.code = scan_rc, to.rotated = rotated, to.out = out, to.out_len = out_len;
    return flow_host_call(correct_flow(a), sink, srcs, n, to);
}

// omr_correct_default_batch_streams and its PNG form: `out` receives the streams of either kind
int correct_default_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, const Correct &a, const OutFormat &fmt,
                            double *rotate_angle, int32_t *need_check, int32_t *scan_rc, uint8_t **out, int64_t *out_len)
{
    clear_error();
    if (!streams || !len || n < 1 || !rotate_angle || !need_check || !scan_rc || !out || !out_len)
        return fail(OMR_ERR_BADARG, "bad batch arguments");
    if (int r = flow_check_streams(streams, len, n)) return r;
    FlowSink sink;
    sink.kind = FlowSink::STREAMS, sink.fmt = fmt;
    FlowOut to;
    to.angle = rotate_angle, to.extra = need_check, to.code = scan_rc, to.out = out, to.out_len = out_len;
    // this flow's own header policy: a PNG, or a JPEG as omr_jpeg_decode takes it -- an EXIF orientation other than 1 is
    // refused, and so is a TIFF (no JPEG).  A sheet the decoder refuses keeps its code and leaves the batch here
    const auto parse = [](ImreadRun &run, const uint8_t *stream, int64_t l) {
        run.jpeg.emplace_back(), run.png.emplace_back(), run.tiff.emplace_back();
        const bool png = pdec_is_png(stream, l);
        run.kind.push_back(png ? IMREAD_PNG : IMREAD_JPEG);
        ImreadParsed ps;
        ps.rc = png ? pdec_parse(stream, l, &run.png.back()) : jdec_parse(stream, l, &run.jpeg.back());
        ps.rows = png ? run.png.back().rows : run.jpeg.back().rows, ps.cols = png ? run.png.back().cols : run.jpeg.back().cols;
        return ps;
    };
    return flow_streams_call(correct_flow(a), sink, streams, len, n, 3, parse, to);
}

}  // namespace

extern "C" {

int omr_correct_batch_canvas(int32_t rows, int32_t cols, int32_t *max_rows, int32_t *max_cols)
{
    clear_error();
    if (!max_rows || !max_cols || rows <= 0 || cols <= 0) return fail(OMR_ERR_BADARG, "bad arguments");
    int R, C;
    canvas_of(rows, cols, &R, &C);
    *max_rows = R;
    *max_cols = C;
    return OMR_OK;
}

int omr_correct_batch_create(int32_t rows, int32_t cols, int32_t channels, uint16_t projection_max_angle,
                             double projection_angle_step, int32_t projection_max_width, int32_t projection_max_height,
                             double hough_min_line_length, double hough_max_line_gap, int32_t device, int32_t max_scans,
                             omr_correct_batch **out)
{
    clear_error();
    if (!out) return fail(OMR_ERR_BADARG, "null out");
    *out = nullptr;
    if (max_scans < 1 || max_scans > 65535) return fail(OMR_ERR_BADARG, "max_scans must be in 1..65535");
    if (device < 0) return fail(OMR_ERR_BADARG, "negative device");
    int rc = check_image_shape(rows, cols);
    if (rc || (rc = cn_correct_batch(channels))) return rc;
    int N = 0;
    const int A = candidate_count(projection_max_angle, projection_angle_step, &N);
    if (A <= 0) return fail(OMR_ERR_BADARG, "empty candidate range");
    // omr.rs:60-82, :114-126
    const double scale = shrink_scale(cols, rows, projection_max_width, projection_max_height);
    const int dc = (int)((double)cols * scale), dr = (int)((double)rows * scale);
    if (dr <= 0 || dc <= 0) return fail(OMR_ERR_ASSERT, "resize to an empty size");
    if ((rc = select_device(device))) return rc;
    NoPoolScope owned;
    std::unique_ptr<omr_correct_batch> cb(new omr_correct_batch);
    cb->device = device, cb->rows = rows, cb->cols = cols, cb->cn = channels, cb->max_scans = max_scans;
    cb->max_angle = projection_max_angle, cb->step = projection_angle_step;
    cb->hough_min = hough_min_line_length, cb->hough_gap = hough_max_line_gap;
    cb->N = N, cb->A = A, cb->scale = scale, cb->dr = dr, cb->dc = dc;
    front_mode(cb.get());
    canvas_of(rows, cols, &cb->DR, &cb->DC);
    cb->small_step = (dc + 3) & ~3;
    cb->small_stride = ((int64_t)dr * cb->small_step + 255) & ~(int64_t)255;
    OMR_HIP(hipStreamCreateWithFlags(&cb->s, hipStreamNonBlocking));
    OMR_HIP(hipStreamCreateWithFlags(&cb->sw, hipStreamNonBlocking));
    OMR_HIP(cb->small.alloc((size_t)max_scans * cb->small_stride));
    OMR_HIP(cb->best.alloc(sizeof(int32_t) * (size_t)max_scans));
    OMR_HIP(cb->vsd.alloc(sizeof(double) * (size_t)max_scans * A));
    OMR_HIP(cb->hsd.alloc(sizeof(double) * (size_t)max_scans * A));
    OMR_HIP(hipHostMalloc((void **)&cb->h_vsd, sizeof(double) * (size_t)max_scans * A, hipHostMallocDefault));
    OMR_HIP(hipHostMalloc((void **)&cb->h_hsd, sizeof(double) * (size_t)max_scans * A, hipHostMallocDefault));
    if (cb->mode != FRONT_AREA_FUSED) cb->er_stride = ((int64_t)rows * cols + 255) & ~(int64_t)255;  // buffer: front_end
    // resizeArea_'s tap tables, once per context
    if (cb->mode == FRONT_AREA_GENERAL && (rc = cb->area.build(cols, dc, rows, dr, 1, nullptr))) return rc;
    if ((rc = omr_batch_create(dr, dc, projection_max_angle, projection_angle_step, scale, device, 1, &cb->sweep))) return rc;
    if ((rc = omr_batch_set_group(cb->sweep, std::min(max_scans, 64)))) return rc;
    *out = cb.release();
    return OMR_OK;
}

void omr_correct_batch_destroy(omr_correct_batch *cb) { delete cb; }

int omr_correct_batch_run_device(omr_correct_batch *cb, const uint8_t *d_scans, int64_t scan_stride_bytes, int64_t step_bytes,
                                 int32_t n, double *rotate_angle, int32_t *need_check, int32_t *scan_rc, uint8_t *d_out,
                                 int64_t out_stride_bytes, int64_t out_step_bytes, int32_t *out_size)
{
    clear_error();
    if (!rotate_angle || !need_check || !scan_rc) return fail(OMR_ERR_BADARG, "null argument");
    int rc = check_sheets(cb, d_scans, scan_stride_bytes, step_bytes, n);
    if (rc) return rc;
    if (d_out && (out_step_bytes < (int64_t)cb->DC * cb->cn || out_stride_bytes < (int64_t)cb->DR * out_step_bytes))
        return fail(OMR_ERR_BADARG, "every output slot must hold %d x %d x %d channels (omr_correct_batch_canvas)", cb->DR, cb->DC,
                    cb->cn);
    std::lock_guard<std::mutex> lk(cb->mu);
    OMR_HIP(hipSetDevice(cb->device));
    rc = run_locked(cb, d_scans, scan_stride_bytes, step_bytes, n, rotate_angle, need_check, scan_rc, d_out, out_stride_bytes,
                    out_step_bytes, out_size);
    if (rc) {  // nothing of this call may still run when the next one starts
        (void)hipStreamSynchronize(cb->s);
        (void)hipStreamSynchronize(cb->sw);
        (void)omr_batch_sync(cb->sweep);
    }
    return rc;
}

int omr_correct_batch_info(omr_correct_batch *cb, int32_t *proj_rows, int32_t *proj_cols, int32_t *front_mode, int32_t *kx,
                           int32_t *ky)
{
    clear_error();
    if (!cb) return fail(OMR_ERR_BADARG, "null context");
    if (proj_rows) *proj_rows = cb->dr;
    if (proj_cols) *proj_cols = cb->dc;
    if (front_mode) *front_mode = cb->mode;
    if (kx) *kx = cb->rd.kx;  // 0 unless the factors are integers
    if (ky) *ky = cb->rd.ky;
    return OMR_OK;
}

int omr_correct_batch_front_device(omr_correct_batch *cb, const uint8_t *d_scans, int64_t scan_stride_bytes, int64_t step_bytes,
                                   int32_t n, uint8_t *d_small, int64_t small_stride_bytes, int64_t small_step_bytes)
{
    clear_error();
    int rc = check_sheets(cb, d_scans, scan_stride_bytes, step_bytes, n);
    if (rc) return rc;
    if (!d_small) return fail(OMR_ERR_BADARG, "null argument");
    if (small_step_bytes < cb->dc || small_stride_bytes < (int64_t)cb->dr * small_step_bytes)
        return fail(OMR_ERR_BADARG, "every output slot must hold %d x %d bytes", cb->dr, cb->dc);
    std::lock_guard<std::mutex> lk(cb->mu);
    OMR_HIP(hipSetDevice(cb->device));
    rc = front_end(cb, d_scans, scan_stride_bytes, step_bytes, n);
    for (int i = 0; rc == OMR_OK && i < n; i++)
        if (hipMemcpy2DAsync(d_small + (size_t)i * small_stride_bytes, (size_t)small_step_bytes,
                             cb->small.as<uint8_t>() + (size_t)i * cb->small_stride, (size_t)cb->small_step, (size_t)cb->dc,
                             (size_t)cb->dr, hipMemcpyDeviceToDevice, cb->s) != hipSuccess)
            rc = fail(OMR_ERR_GPU, "hipMemcpy2DAsync failed");
    if (hipStreamSynchronize(cb->s) != hipSuccess && rc == OMR_OK) rc = fail(OMR_ERR_GPU, "hipStreamSynchronize failed");
    return rc;
}

int omr_correct_default_batch(const omr_image *srcs, int32_t n, uint16_t projection_max_angle, double projection_angle_step,
                              int32_t projection_max_width, int32_t projection_max_height, double hough_min_line_length,
                              double hough_max_line_gap, double *rotate_angle, int32_t *need_check, int32_t *scan_rc,
                              omr_image_owned *rotated)
{
    clear_error();
    return correct_default_host(srcs, n, Correct{projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                                                hough_min_line_length, hough_max_line_gap},
                                rotate_angle, need_check, scan_rc, rotated, nullptr, nullptr, OutFormat{OUT_JPEG, 0});
}

int omr_correct_default_batch_jpeg(const omr_image *srcs, int32_t n, uint16_t projection_max_angle, double projection_angle_step,
                                   int32_t projection_max_width, int32_t projection_max_height, double hough_min_line_length,
                                   double hough_max_line_gap, int32_t quality, double *rotate_angle, int32_t *need_check,
                                   int32_t *scan_rc, uint8_t **jpeg, int64_t *jpeg_len)
{
    clear_error();
    if (!jpeg || !jpeg_len) return fail(OMR_ERR_BADARG, "bad batch arguments");
    return correct_default_host(srcs, n, Correct{projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                                                hough_min_line_length, hough_max_line_gap},
                                rotate_angle, need_check, scan_rc, nullptr, jpeg, jpeg_len, OutFormat{OUT_JPEG, quality});
}

int omr_correct_default_batch_png(const omr_image *srcs, int32_t n, uint16_t projection_max_angle, double projection_angle_step,
                                  int32_t projection_max_width, int32_t projection_max_height, double hough_min_line_length,
                                  double hough_max_line_gap, int32_t compression, double *rotate_angle, int32_t *need_check,
                                  int32_t *scan_rc, uint8_t **png, int64_t *png_len)
{
    clear_error();
    if (!png || !png_len) return fail(OMR_ERR_BADARG, "bad batch arguments");
    return correct_default_host(srcs, n, Correct{projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                                                hough_min_line_length, hough_max_line_gap},
                                rotate_angle, need_check, scan_rc, nullptr, png, png_len, OutFormat{OUT_PNG, compression});
}

int omr_correct_default_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, uint16_t projection_max_angle,
                                      double projection_angle_step, int32_t projection_max_width, int32_t projection_max_height,
                                      double hough_min_line_length, double hough_max_line_gap, int32_t quality,
                                      double *rotate_angle, int32_t *need_check, int32_t *scan_rc, uint8_t **jpeg,
                                      int64_t *jpeg_len)
{
    return correct_default_streams(streams, len, n,
                                   Correct{projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                                           hough_min_line_length, hough_max_line_gap},
                                   OutFormat{OUT_JPEG, quality}, rotate_angle, need_check, scan_rc, jpeg, jpeg_len);
}

int omr_correct_default_batch_streams_png(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                          uint16_t projection_max_angle, double projection_angle_step,
                                          int32_t projection_max_width, int32_t projection_max_height,
                                          double hough_min_line_length, double hough_max_line_gap, int32_t compression,
                                          double *rotate_angle, int32_t *need_check, int32_t *scan_rc, uint8_t **png,
                                          int64_t *png_len)
{
    return correct_default_streams(streams, len, n,
                                   Correct{projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                                           hough_min_line_length, hough_max_line_gap},
                                   OutFormat{OUT_PNG, compression}, rotate_angle, need_check, scan_rc, png, png_len);
}

}  // extern "C"
