// projection_batch.cpp -- get_angle_with_projections (projection.rs:17-194) with its resize_scale for batches of scans
// (DESIGN.md section 4.12):
//
//   front end   scale_self on the colour scans (transfer.rs:66-91), one launch over the batch (resize.hip),
//               into the context's working buffer.  The dispatch is resize()'s (resize_dispatch, host_image.hpp); the tap
//               tables of a fractional shrink are built when the context is created and stay on the device.
//   sweep       the context's omr_batch_ctx for the working shape: gray (quirk B8) and threshold(127) fused into its
//               bit-packing loads, arg-max on the device.
//   deskew      (omr_projection_batch_deskew_device) the batch warp (deskew.hip) of the FULL-SIZE
//               scans by the sweep's winners, read on the device: the context keeps a second candidate set, planned
//               for rows x cols instead of the working shape.
//   streams     (omr_deskew_with_projections_batch_streams) the same from file contents to file
//               contents: JPEG / PNG streams decoded on the device straight into the scan slots, the canvases encoded
//               there, only streams on the link.
//
// Scan i's angle is omr_get_angle_with_projections' for the same scan, as f64 bits; its canvas is omr_rotate's for that
// angle, byte for byte.
#include <math.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <vector>

#include "../../include/omrdeskew.h"
#include "encode_any.hpp"
#include "engine.hpp"
#include "flow_frame.hpp"
#include "host_threads.hpp"
#include "hough_host.hpp"
#include "jpeg_dec.hpp"
#include "orient.hpp"
#include "png_dec.hpp"
#include "stream_sink.hpp"

using namespace omr;
using namespace omr::hh;

namespace {

const int kWarpChunk = 64;  // scans per launch of the deskew warp: bounds the tile records (2.4 MB per A4 colour scan's canvas)

// scale_self's size and resize()'s dispatch for it, on the host (COPY: the working images are the scans)
struct Working {
    int wr = 0, wc = 0;
    ResizeDispatch d{ResizeDispatch::COPY, false, 1, 1};
    int front_mode() const  // as omr_projection_batch_working_size and _info report it
    {
        switch (d.kind) {
        case ResizeDispatch::LINEAR: return OMR_PROJECTION_FRONT_LINEAR;
        case ResizeDispatch::AREA_INT: return OMR_PROJECTION_FRONT_AREA_INT;
        case ResizeDispatch::AREA_GENERAL: return OMR_PROJECTION_FRONT_AREA_GENERAL;
        default: return OMR_PROJECTION_FRONT_NONE;
        }
    }
};

int working_size(int rows, int cols, double scale, Working *w)
{
    int rc = check_image_shape(rows, cols);
    if (rc) return rc;
    if (!isfinite(scale) || scale <= 0.0) return fail(OMR_ERR_BADARG, "resize_scale must be finite and positive");
    if (scale == 1.0) {  // projection.rs:24: no scale_self
        w->wr = rows, w->wc = cols;
        return OMR_OK;
    }
    const double fc = (double)cols * scale, fr = (double)rows * scale;
    if (fc >= 32767.0 || fr >= 32767.0) return fail(OMR_ERR_ASSERT, "working image dimension >= SHRT_MAX");
    const int dc = (int)fc, dr = (int)fr;  // transfer.rs:70-71 `as i32`
    if (dr <= 0 || dc <= 0) return fail(OMR_ERR_ASSERT, "resize to an empty size");
    w->wr = dr, w->wc = dc;
    w->d = resize_dispatch(rows, cols, dr, dc, scale > 1.0 ? OMR_INTER_LINEAR : OMR_INTER_AREA);
    return OMR_OK;
}

}  // namespace

struct omr_projection_batch {
    int device = 0, rows = 0, cols = 0, cn = 0, max_scans = 0;
    double step = 0;
    int N = 0, A = 0;
    Working w;
    PfTiling tiling;
    int64_t wstep = 0, wstride = 0;  // the working buffer's row pitch and image stride
    omr_batch_ctx *sweep = nullptr;
    hipStream_t s = nullptr;  // front end and result copies
    DevBuf work, best, vsd, hsd;
    AreaTables area;  // AREA_GENERAL
    std::vector<int32_t> h_best;
    // the deskew: the candidates' CONTAIN canvases and warp tables at rows x cols, planned at create (host arithmetic),
    // on the device from the first deskew call on; tile records and canvas sizes per run
    DeskewTables dk;
    DevBuf dk_tiles, dk_size;
    std::vector<int32_t> h_size;
    std::mutex mu;
    ~omr_projection_batch()
    {
        if (s) (void)hipStreamSynchronize(s);
        if (sweep) omr_batch_destroy(sweep);
        if (s) (void)hipStreamDestroy(s);
    }
};

namespace {

int check_scans(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n)
{
    if (!pb || !d_scans) return fail(OMR_ERR_BADARG, "null argument");
    if (n < 1 || n > pb->max_scans) return fail(OMR_ERR_BADARG, "n = %d outside 1..max_scans (%d)", n, pb->max_scans);
    if (step < (int64_t)pb->cols * pb->cn) return fail(OMR_ERR_BADARG, "step_bytes < cols x channels");
    if (scan_stride < 0) return fail(OMR_ERR_BADARG, "negative scan_stride_bytes");
    return OMR_OK;
}

// scale_self of n scans -> pb->work, on pb->s (nothing to do, and nothing written, when the dispatch is COPY)
int front_end(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n)
{
    const Working &w = pb->w;
    if (w.d.kind == ResizeDispatch::COPY) return OMR_OK;
    ResizeImgs im{};
    im.src = d_scans, im.scan_stride = scan_stride, im.sstep = step;
    im.dst = pb->work.as<uint8_t>(), im.out_stride = pb->wstride, im.dstep = pb->wstep;
    im.cn = pb->cn, im.srows = pb->rows, im.scols = pb->cols, im.drows = w.wr, im.dcols = w.wc;
    // INTER_AREA goes through the tile kernel: on a colour scan the per-byte gather is the whole cost
    const bool area = w.d.kind != ResizeDispatch::LINEAR;
    OMR_HIP(launch_resize(w.d, im, n, pb->s, pb->area.taps(), area ? &pb->tiling : nullptr));
    return OMR_OK;
}

// front end, sweep and arg-max of n scans: the winners are in pb->best (and the scores in pb->vsd / hsd) when it returns
int sweep_locked(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n, bool scores)
{
    const size_t A = (size_t)pb->A;
    int rc;
    if (scores) {
        if ((rc = grow(&pb->vsd, sizeof(double) * (size_t)n * A))) return rc;
        if ((rc = grow(&pb->hsd, sizeof(double) * (size_t)n * A))) return rc;
    }
    if ((rc = front_end(pb, d_scans, scan_stride, step, n))) return rc;
    const bool resized = pb->w.d.kind != ResizeDispatch::COPY;
    if (resized) OMR_HIP(hipStreamSynchronize(pb->s));  // the sweep runs on the batch context's own streams
    // projection.rs:29-32: RGB2GRAY and threshold(127) are fused into the sweep's loads
    if ((rc = omr_batch_run_device_cn(pb->sweep, resized ? pb->work.as<uint8_t>() : d_scans, resized ? pb->wstride : scan_stride,
                                      resized ? pb->wstep : step, pb->cn, n, 127, pb->best.as<int32_t>(),
                                      scores ? pb->vsd.as<double>() : nullptr, scores ? pb->hsd.as<double>() : nullptr)))
        return rc;
    return omr_batch_sync(pb->sweep);
}

// the winners to the host (after whatever else the call queued on pb->s), and the angles they mean
int winners_to_host(omr_projection_batch *pb, int n, double *angle, int32_t *best_idx)
{
    OMR_HIP(hipMemcpyAsync(pb->h_best.data(), pb->best.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, pb->s));
    OMR_HIP(hipStreamSynchronize(pb->s));
    for (int i = 0; i < n; i++) {
        const int idx = pb->h_best[(size_t)i];
        angle[i] = ((double)idx - (double)pb->N) * pb->step;  // projection.rs:189-190
        if (best_idx) best_idx[i] = idx;
    }
    return OMR_OK;
}

int run_locked(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n, double *angle,
               int32_t *best_idx, double *v_sd, double *h_sd)
{
    const size_t A = (size_t)pb->A;
    int rc;
    if ((rc = sweep_locked(pb, d_scans, scan_stride, step, n, v_sd || h_sd))) return rc;
    if (v_sd) OMR_HIP(hipMemcpyAsync(v_sd, pb->vsd.p, sizeof(double) * (size_t)n * A, hipMemcpyDeviceToHost, pb->s));
    if (h_sd) OMR_HIP(hipMemcpyAsync(h_sd, pb->hsd.p, sizeof(double) * (size_t)n * A, hipMemcpyDeviceToHost, pb->s));
    return winners_to_host(pb, n, angle, best_idx);
}

// the border's bytes as DeskewPass::border takes them (3 channels: channel c = byte c)
int packed_border(int cn, const uint8_t bv[4])
{
    return cn == 1 ? (int)bv[0] : (int)((uint32_t)bv[0] | ((uint32_t)bv[1] << 8) | ((uint32_t)bv[2] << 16));
}

// sweep, then the warp of the full-size scans by pb->best on pb->s; winners and canvas sizes come down once, at the end
int deskew_locked(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n, int interp,
                  const uint8_t border_value[4], uint8_t *d_out, int64_t out_stride, int64_t out_step, int32_t *out_size,
                  double *angle, int32_t *best_idx)
{
    int rc;
    if (!pb->dk.on_device && (rc = pb->dk.upload(nullptr))) return rc;  // once per context
    if ((rc = sweep_locked(pb, d_scans, scan_stride, step, n, false))) return rc;
    DeskewPass p = pb->dk.pass();
    p.scan_stride = scan_stride, p.sstep = step, p.srows = pb->rows, p.scols = pb->cols;
    p.out_stride = out_stride, p.dstep = out_step;
    p.border = packed_border(pb->cn, border_value);
    p.cn = pb->cn;
    if ((rc = grow(&pb->dk_tiles, deskew_tile_bytes(p, std::min(pb->max_scans, kWarpChunk))))) return rc;
    for (int i0 = 0; i0 < n; i0 += kWarpChunk) {  // the launches of a stream run one after the other: one set of records
        p.src = d_scans + (size_t)i0 * scan_stride;
        p.dst = d_out + (size_t)i0 * out_stride;
        p.best = pb->best.as<int32_t>() + i0;
        p.out_size = pb->dk_size.as<int32_t>() + 2 * (size_t)i0;
        OMR_HIP(launch_deskew_warp(p, std::min(kWarpChunk, n - i0), interp, pb->dk_tiles.p, pb->s));
    }
    OMR_HIP(hipMemcpyAsync(pb->h_size.data(), pb->dk_size.p, 2 * sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, pb->s));
    if ((rc = winners_to_host(pb, n, angle, best_idx))) return rc;
    memcpy(out_size, pb->h_size.data(), 2 * sizeof(int32_t) * (size_t)n);
    return OMR_OK;
}

// ---- contexts kept per (device, shape, parameters) -------------------------------------------------------------------
struct CtxKey {
    int device, rows, cols, cn;
    uint16_t max_angle;
    double step, scale;
    bool operator==(const CtxKey &o) const
    {
        return device == o.device && rows == o.rows && cols == o.cols && cn == o.cn && max_angle == o.max_angle &&
               step == o.step && scale == o.scale;
    }
};
ContextCache<CtxKey, omr_projection_batch> g_ctx(4);

int cached_context(const CtxKey &k, std::shared_ptr<omr_projection_batch> *out)
{
    return g_ctx.get(k, [&](std::shared_ptr<omr_projection_batch> *sp) -> int {
        omr_projection_batch *raw = nullptr;
        int rc = omr_projection_batch_create(k.rows, k.cols, k.cn, k.max_angle, k.step, k.scale, k.device, kAnglesChunk, &raw);
        if (rc == OMR_OK) sp->reset(raw, omr_projection_batch_destroy);
        return rc;
    }, out);
}

// ---- the batch forms: the frame's walk (flow_frame.hpp) with this flow's few answers -------------------------------------
struct Sweep {
    uint16_t max_angle;
    double step, scale;
    int N;
    int interp;
    const uint8_t *border;
    int cn = 0;                  // the streams forms: the channels every sheet is decoded to,
    OutFormat fmt{OUT_JPEG, 0};  // and what writes the canvases
};

// a code of the per-call chain that belongs to its sheet (any other ends the call)
bool sheet_code(int rc) { return rc == OMR_ERR_ASSERT || rc == OMR_ERR_BADARG || rc == OMR_ERR_NOTIMPL; }

// the per-call function, image by image: the buckets a batch context does not take
int host_per_call(const Sweep &a, const omr_image *srcs, const std::vector<int> &idx, const FlowOut &r)
{
    for (int i : idx) {
        int rc = omr_get_angle_with_projections(&srcs[i], a.max_angle, a.step, a.scale, 1, &r.angle[i]);
        if (rc) return rc;
        r.extra[i] = (int32_t)llround(r.angle[i] / a.step) + a.N;
        if (r.rotated && (rc = omr_rotate(&srcs[i], r.angle[i], 1.0, a.interp, a.border, OMR_CLIP_CONTAIN, &r.rotated[i]))) return rc;
    }
    return OMR_OK;
}

// the per-call chain from file contents, sheet by sheet; a sheet's own code stays with the sheet
int streams_per_call(const Sweep &a, const FlowIn &in, const std::vector<int> &idx, const FlowOut &r)
{
    for (int k : idx) {
        omr_image_owned img{nullptr, 0, 0, 0, 0}, rot{nullptr, 0, 0, 0, 0};
        uint8_t *bytes = nullptr;
        int64_t cap = 0, used = 0;
        int rc = omr_imread(in.streams[k], in.len[k], a.cn, 0, &img);
        const omr_image view{img.data, img.rows, img.cols, img.channels, img.step_bytes};
        if (!rc) rc = omr_get_angle_with_projections(&view, a.max_angle, a.step, a.scale, 1, &r.angle[k]);
        if (!rc && r.out) {
            rc = omr_rotate(&view, r.angle[k], 1.0, a.interp, a.border, OMR_CLIP_CONTAIN, &rot);
            if (!rc) rc = a.fmt.bound(rot.rows, rot.cols, rot.channels, &cap);
            if (!rc && !(bytes = (uint8_t *)malloc((size_t)cap))) rc = fail(OMR_ERR_NOMEM, "out of host memory");
            const omr_image canvas{rot.data, rot.rows, rot.cols, rot.channels, rot.step_bytes};
            if (!rc) rc = a.fmt.encode_host(&canvas, bytes, cap, &used);
        }
        omr_image_free(&img);
        omr_image_free(&rot);
        if (rc) {
            free(bytes);
            if (!sheet_code(rc)) return rc;
            r.code[k] = rc, r.angle[k] = 0.0, r.extra[k] = -1;
            continue;
        }
        r.extra[k] = (int32_t)llround(r.angle[k] / a.step) + a.N;
        if (r.out) {
            uint8_t *fit = (uint8_t *)realloc(bytes, (size_t)std::max<int64_t>(used, 1));  // the bound is several times the stream
            r.out[k] = fit ? fit : bytes, r.out_len[k] = used;
        }
    }
    clear_error();
    return OMR_OK;
}

Flow projection_flow(const Sweep &a)
{
    Flow f;
    f.extra_refused = -1;  // best_idx of a sheet with a code
    // omr_get_angle_with_projections' checks
    f.accept = [a](const omr_image &im) -> int {
        Working w;
        int rc = check_image(&im, cn_gray_source);
        return rc ? rc : working_size(im.rows, im.cols, a.scale, &w);
    };
    f.canvas = [a](int rows, int cols, int *R, int *C) -> int {
        const int A = candidate_count(a.max_angle, a.step, nullptr);
        std::vector<double> cand((size_t)A);
        for (int i = 0; i < A; i++) cand[(size_t)i] = (double)(i - a.N) * a.step;
        DeskewTables dk;
        if (dk.plan(rows, cols, cand.data(), A)) clear_error(), *R = 0;  // (a shape without a canvas goes sheet by sheet)
        else *R = dk.rows, *C = dk.cols;
        return OMR_OK;
    };
    f.open = [a](int rows, int cols, int cn, bool canvases, FlowBucket *b) -> int {
        b->how = FlowBucket::PER_SHEET;
        if (cn == 4) return OMR_OK;
        int dev = 0;
        OMR_HIP(hipGetDevice(&dev));
        std::shared_ptr<omr_projection_batch> pb;
        int rc = cached_context(CtxKey{dev, rows, cols, cn, a.max_angle, a.step, a.scale}, &pb);
        if (rc == OMR_ERR_NOTIMPL || rc == OMR_ERR_BADARG || rc == OMR_ERR_ASSERT) {  // a sweep the batch context cannot plan
            clear_error();
            return OMR_OK;
        }
        if (rc) return rc;
        if (canvases && !pb->dk.count()) return OMR_OK;  // a canvas the warp's tables cannot hold
        b->how = FlowBucket::RUN, b->chunk = canvases ? kDeskewChunk : kAnglesChunk;
        b->canvas_rows = pb->dk.rows, b->canvas_cols = pb->dk.cols, b->out_step = (int64_t)pb->dk.cols * cn;
        b->ctx = pb;
        return OMR_OK;
    };
    f.run = [a](const FlowBucket &b, const FlowSlots &s, double *ang, int32_t *best, int32_t *, int32_t *size) -> int {
        omr_projection_batch *pb = static_cast<omr_projection_batch *>(b.ctx.get());
        return s.dout ? omr_projection_batch_deskew_device(pb, s.din, s.in_stride, s.row, s.z, a.interp, a.border, s.dout, s.out_stride,
                                                           s.out_step, size, ang, best)
                      : omr_projection_batch_run_device(pb, s.din, s.in_stride, s.row, s.z, ang, best, nullptr, nullptr);
    };
    f.per_sheet = [a](const FlowIn &in, const std::vector<int> &idx, const FlowOut &r) -> int {
        return in.streams ? streams_per_call(a, in, idx, r) : host_per_call(a, in.imgs, idx, r);
    };
    return f;
}

// both host forms
int host_form(const omr_image *srcs, int n, uint16_t max_angle, double step, double scale, double *angles, int32_t *best_idx,
              omr_image_owned *rotated, int interp, const uint8_t *border)
{
    int N = 0;
    if (candidate_count(max_angle, step, &N) <= 0)
        return fail(OMR_ERR_BADARG, "empty candidate range (the reference indexes [0] and panics)");
    FlowSink sink;
    if (rotated) sink.kind = FlowSink::CANVASES;
    FlowOut to;
    to.angle = angles, to.extra = best_idx, to.rotated = rotated;
    return flow_host_call(projection_flow(Sweep{max_angle, step, scale, N, interp, border}), sink, srcs, n, to);
}

// omr_deskew_with_projections_batch_streams and its PNG and TIFF forms: `out` receives the streams
// of any kind
int deskew_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels, uint16_t max_angle, double step,
                   double scale, int32_t interp, const uint8_t *border, const OutFormat &fmt, double *angles, int32_t *best_idx,
                   int32_t *scan_rc, uint8_t **out, int64_t *out_len)
{
    clear_error();
    if (int r = fmt.check_params(channels == 1 ? 1 : 3)) return r;  // a bad channel count has its own refusal below
    if (!streams || !len || n < 1 || !angles || !scan_rc) return fail(OMR_ERR_BADARG, "bad batch arguments");
    if (!out != !out_len) return fail(OMR_ERR_BADARG, "the streams and their lengths are returned together, or neither");
    if (out && !border) return fail(OMR_ERR_BADARG, "null border_value");
    if (channels != 1 && channels != 3) return fail(OMR_ERR_BADARG, "channels must be 1 or 3, got %d", channels);
    if (int r = flow_check_streams(streams, len, n)) return r;
    int N = 0;
    if (candidate_count(max_angle, step, &N) <= 0)
        return fail(OMR_ERR_BADARG, "empty candidate range (the reference indexes [0] and panics)");
    if (!isfinite(scale) || scale <= 0.0) return fail(OMR_ERR_BADARG, "resize_scale must be finite and positive");
    if (interp != OMR_INTER_NEAREST && interp != OMR_INTER_LINEAR)
        return fail(OMR_ERR_NOTIMPL, "interpolation flag %d is not implemented", interp);
    FlowSink sink;
    if (out) sink.kind = FlowSink::STREAMS, sink.fmt = fmt;
    FlowOut to;
    to.angle = angles, to.extra = best_idx, to.code = scan_rc, to.out = out, to.out_len = out_len;
    // a sheet its decoder refuses, or for which the per-call function would fail, keeps its code (imread turns a JPEG by its
    // EXIF orientation: the scan's shape is the turned one)
    const auto parse = [channels, scale](ImreadRun &run, const uint8_t *stream, int64_t l) {
        ImreadParsed ps = run.append(stream, l, channels, false);
        Working w;
        if (!ps.rc) ps.rc = working_size(ps.rows, ps.cols, scale, &w);
        return ps;
    };
    return flow_streams_call(projection_flow(Sweep{max_angle, step, scale, N, interp, border, channels, fmt}), sink, streams, len, n,
                             channels, parse, to);
}

}  // namespace

extern "C" {

int omr_projection_batch_working_size(int32_t rows, int32_t cols, double resize_scale, int32_t *wrows, int32_t *wcols,
                                      int32_t *front_mode)
{
    clear_error();
    if (!wrows || !wcols || !front_mode) return fail(OMR_ERR_BADARG, "null output");
    Working w;
    int rc = working_size(rows, cols, resize_scale, &w);
    if (rc) return rc;
    *wrows = w.wr, *wcols = w.wc, *front_mode = w.front_mode();
    return OMR_OK;
}

int omr_projection_batch_create(int32_t rows, int32_t cols, int32_t channels, uint16_t max_angle, double step,
                                double resize_scale, int32_t device, int32_t max_scans, omr_projection_batch **out)
{
    clear_error();
    if (!out) return fail(OMR_ERR_BADARG, "null out");
    *out = nullptr;
    if (max_scans < 1 || max_scans > 65535) return fail(OMR_ERR_BADARG, "max_scans must be in 1..65535");
    if (device < 0) return fail(OMR_ERR_BADARG, "negative device");
    int rc = check_image_shape(rows, cols);
    if (rc || (rc = cn_projection_batch(channels))) return rc;
    int N = 0;
    const int A = candidate_count(max_angle, step, &N);
    if (A <= 0) return fail(OMR_ERR_BADARG, "empty candidate range");
    Working w;
    if ((rc = working_size(rows, cols, resize_scale, &w))) return rc;
    if ((rc = select_device(device))) return rc;
    NoPoolScope owned;
    std::unique_ptr<omr_projection_batch> pb(new omr_projection_batch);
    pb->device = device, pb->rows = rows, pb->cols = cols, pb->cn = channels, pb->max_scans = max_scans;
    pb->step = step, pb->N = N, pb->A = A, pb->w = w;
    pb->h_best.assign((size_t)max_scans, 0);
    pb->h_size.assign(2 * (size_t)max_scans, 0);
    {  // the deskew's candidate set, at the full shape: host arithmetic, so that the canvas query needs no device.  A shape
       // whose canvases leave the image limit keeps its sweep; the deskew entry points then refuse
        std::vector<double> angles((size_t)A);
        for (int i = 0; i < A; i++) angles[(size_t)i] = (double)(i - N) * step;
        if (pb->dk.plan(rows, cols, angles.data(), A)) clear_error();
    }
    OMR_HIP(hipStreamCreateWithFlags(&pb->s, hipStreamNonBlocking));
    OMR_HIP(pb->best.alloc(sizeof(int32_t) * (size_t)max_scans));
    OMR_HIP(pb->dk_size.alloc(2 * sizeof(int32_t) * (size_t)max_scans));
    if (w.d.kind != ResizeDispatch::COPY) {
        pb->wstep = ((int64_t)w.wc * channels + 3) & ~(int64_t)3;
        pb->wstride = ((int64_t)w.wr * pb->wstep + 255) & ~(int64_t)255;
        OMR_HIP(pb->work.alloc((size_t)max_scans * pb->wstride));
    }
    if (w.d.kind == ResizeDispatch::AREA_GENERAL) {  // resizeArea_'s tap tables, once per context
        if ((rc = pb->area.build(cols, w.wc, rows, w.wr, channels, nullptr))) return rc;
        pb->tiling = pf_area_tiling(channels, w.wc, 0, &pb->area.h_xt, &pb->area.h_xo, &pb->area.h_yt);
    } else if (w.d.kind == ResizeDispatch::AREA_INT) {
        pb->tiling = pf_area_tiling(channels, w.wc, w.d.kx, nullptr, nullptr, nullptr);
    }
    // the sweep of the working shape at unit scale (projection.rs:47-65), whatever kernels the context picks for it
    if ((rc = omr_batch_create(w.wr, w.wc, max_angle, step, 1.0, device, 1, &pb->sweep))) return rc;
    if ((rc = omr_batch_set_group(pb->sweep, std::min(max_scans, 64)))) return rc;
    *out = pb.release();
    return OMR_OK;
}

void omr_projection_batch_destroy(omr_projection_batch *pb) { delete pb; }

int omr_projection_batch_info(omr_projection_batch *pb, int32_t *wrows, int32_t *wcols, int32_t *front_mode, int32_t *candidates)
{
    clear_error();
    if (!pb) return fail(OMR_ERR_BADARG, "null context");
    if (wrows) *wrows = pb->w.wr;
    if (wcols) *wcols = pb->w.wc;
    if (front_mode) *front_mode = pb->w.front_mode();
    if (candidates) *candidates = pb->A;
    return OMR_OK;
}

int omr_projection_batch_front_device(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                      int64_t step_bytes, int32_t n, uint8_t *d_small, int64_t small_stride_bytes,
                                      int64_t small_step_bytes)
{
    clear_error();
    int rc = check_scans(pb, d_scans, scan_stride_bytes, step_bytes, n);
    if (rc) return rc;
    if (!d_small) return fail(OMR_ERR_BADARG, "null argument");
    const int64_t wrow = (int64_t)pb->w.wc * pb->cn;
    if (small_step_bytes < wrow || small_stride_bytes < (int64_t)pb->w.wr * small_step_bytes)
        return fail(OMR_ERR_BADARG, "every output slot must hold %d x %d x %d bytes", pb->w.wr, pb->w.wc, pb->cn);
    std::lock_guard<std::mutex> lk(pb->mu);
    OMR_HIP(hipSetDevice(pb->device));
    rc = front_end(pb, d_scans, scan_stride_bytes, step_bytes, n);
    const bool resized = pb->w.d.kind != ResizeDispatch::COPY;  // NONE: the working images are the scans
    for (int i = 0; rc == OMR_OK && i < n; i++) {
        const uint8_t *from = resized ? pb->work.as<uint8_t>() + (size_t)i * pb->wstride : d_scans + (size_t)i * scan_stride_bytes;
        if (hipMemcpy2DAsync(d_small + (size_t)i * small_stride_bytes, (size_t)small_step_bytes, from,
                             (size_t)(resized ? pb->wstep : step_bytes), (size_t)wrow, (size_t)pb->w.wr, hipMemcpyDeviceToDevice,
                             pb->s) != hipSuccess)
            rc = fail(OMR_ERR_GPU, "hipMemcpy2DAsync failed");
    }
    if (hipStreamSynchronize(pb->s) != hipSuccess && rc == OMR_OK) rc = fail(OMR_ERR_GPU, "hipStreamSynchronize failed");
    return rc;
}

int omr_projection_batch_run_device(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                    int64_t step_bytes, int32_t n, double *angle, int32_t *best_idx, double *v_sd, double *h_sd)
{
    clear_error();
    int rc = check_scans(pb, d_scans, scan_stride_bytes, step_bytes, n);
    if (rc) return rc;
    if (!angle) return fail(OMR_ERR_BADARG, "null argument");
    std::lock_guard<std::mutex> lk(pb->mu);
    OMR_HIP(hipSetDevice(pb->device));
    rc = run_locked(pb, d_scans, scan_stride_bytes, step_bytes, n, angle, best_idx, v_sd, h_sd);
    if (rc) {  // nothing of this call may still run when the next one starts
        (void)hipStreamSynchronize(pb->s);
        (void)omr_batch_sync(pb->sweep);
    }
    return rc;
}

int omr_projection_batch_deskew_canvas(omr_projection_batch *pb, int32_t *max_rows, int32_t *max_cols)
{
    clear_error();
    if (!pb || !max_rows || !max_cols) return fail(OMR_ERR_BADARG, "null argument");
    if (!pb->dk.count()) return fail(OMR_ERR_ASSERT, "a candidate's canvas leaves the image limit");
    *max_rows = pb->dk.rows, *max_cols = pb->dk.cols;
    return OMR_OK;
}

int omr_projection_batch_deskew_device(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                       int64_t step_bytes, int32_t n, int32_t interp, const uint8_t border_value[4],
                                       uint8_t *d_out, int64_t out_stride_bytes, int64_t out_step_bytes, int32_t *out_size,
                                       double *angle, int32_t *best_idx)
{
    clear_error();
    int rc = check_scans(pb, d_scans, scan_stride_bytes, step_bytes, n);
    if (rc) return rc;
    if (!border_value || !d_out || !out_size || !angle) return fail(OMR_ERR_BADARG, "null argument");
    if (interp != OMR_INTER_NEAREST && interp != OMR_INTER_LINEAR)
        return fail(OMR_ERR_NOTIMPL, "interpolation flag %d is not implemented", interp);
    if (!pb->dk.count()) return fail(OMR_ERR_ASSERT, "a candidate's canvas leaves the image limit");
    // (by division: rows x pitch of an absurd pitch would leave 64 bits)
    if (out_step_bytes < (int64_t)pb->dk.cols * pb->cn || out_stride_bytes / pb->dk.rows < out_step_bytes)
        return fail(OMR_ERR_BADARG, "every output slot must hold the largest canvas, %d x %d x %d channels (omr_projection_batch_deskew_canvas)",
                    pb->dk.rows, pb->dk.cols, pb->cn);
    std::lock_guard<std::mutex> lk(pb->mu);
    OMR_HIP(hipSetDevice(pb->device));
    rc = deskew_locked(pb, d_scans, scan_stride_bytes, step_bytes, n, interp, border_value, d_out, out_stride_bytes, out_step_bytes,
                       out_size, angle, best_idx);
    if (rc) {  // nothing of this call may still run when the next one starts
        (void)hipStreamSynchronize(pb->s);
        (void)omr_batch_sync(pb->sweep);
    }
    return rc;
}

int omr_get_angles_with_projections_batch(const omr_image *srcs, int32_t n, uint16_t max_angle, double step, double resize_scale,
                                          double *angles, int32_t *best_idx)
{
    clear_error();
    if (!srcs || n < 1 || !angles) return fail(OMR_ERR_BADARG, "bad batch arguments");
    return host_form(srcs, n, max_angle, step, resize_scale, angles, best_idx, nullptr, OMR_INTER_NEAREST, nullptr);
}

int omr_deskew_with_projections_batch(const omr_image *srcs, int32_t n, uint16_t max_angle, double step, double resize_scale,
                                      int32_t interp, const uint8_t border_value[4], double *angles, int32_t *best_idx,
                                      omr_image_owned *rotated)
{
    clear_error();
    if (!srcs || n < 1 || !border_value || !angles || !rotated) return fail(OMR_ERR_BADARG, "bad batch arguments");
    if (interp != OMR_INTER_NEAREST && interp != OMR_INTER_LINEAR)
        return fail(OMR_ERR_NOTIMPL, "interpolation flag %d is not implemented", interp);
    return host_form(srcs, n, max_angle, step, resize_scale, angles, best_idx, rotated, interp, border_value);
}

int omr_deskew_with_projections_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                              uint16_t max_angle, double step, double resize_scale, int32_t interp,
                                              const uint8_t border_value[4], int32_t quality, double *angles,
                                              int32_t *best_idx, int32_t *scan_rc, uint8_t **jpeg, int64_t *jpeg_len)
{
    return deskew_streams(streams, len, n, channels, max_angle, step, resize_scale, interp, border_value, OutFormat{OUT_JPEG, quality},
                          angles, best_idx, scan_rc, jpeg, jpeg_len);
}

int omr_deskew_with_projections_batch_streams_png(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                                  int32_t channels, uint16_t max_angle, double step, double resize_scale,
                                                  int32_t interp, const uint8_t border_value[4], int32_t compression,
                                                  double *angles, int32_t *best_idx, int32_t *scan_rc, uint8_t **png,
                                                  int64_t *png_len)
{
    return deskew_streams(streams, len, n, channels, max_angle, step, resize_scale, interp, border_value, OutFormat{OUT_PNG, compression},
                          angles, best_idx, scan_rc, png, png_len);
}

int omr_deskew_with_projections_batch_streams_tiff(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                                   int32_t channels, uint16_t max_angle, double step, double resize_scale,
                                                   int32_t interp, const uint8_t border_value[4], int32_t threshold,
                                                   int32_t rows_per_strip, int32_t dpi, double *angles, int32_t *best_idx,
                                                   int32_t *scan_rc, uint8_t **tiff, int64_t *tiff_len)
{
    return deskew_streams(streams, len, n, channels, max_angle, step, resize_scale, interp, border_value,
                          OutFormat{OUT_TIFF, threshold, 1, rows_per_strip, dpi}, angles, best_idx, scan_rc, tiff, tiff_len);
}

int omr_deskew_with_projections_batch_streams_tiff8(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                                    int32_t channels, uint16_t max_angle, double step, double resize_scale,
                                                    int32_t interp, const uint8_t border_value[4], int32_t compression,
                                                    int32_t predictor, int32_t rows_per_strip, int32_t dpi, double *angles,
                                                    int32_t *best_idx, int32_t *scan_rc, uint8_t **tiff, int64_t *tiff_len)
{
    return deskew_streams(streams, len, n, channels, max_angle, step, resize_scale, interp, border_value,
                          OutFormat{OUT_TIFF8, compression, predictor, rows_per_strip, dpi}, angles, best_idx, scan_rc, tiff, tiff_len);
}

}  // extern "C"
