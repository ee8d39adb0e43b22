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
#include "host_threads.hpp"
#include "hough_host.hpp"
#include "jpeg_dec.hpp"
#include "orient.hpp"
#include "png_dec.hpp"
#include "stream_sink.hpp"

using namespace omr;
using namespace omr::hh;

namespace {

const int kChunk = 256;     // scans per run of the host form's contexts
const int kDeskewChunk = 32;  // ... when the deskewed canvases come back with the angles
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

// ---- the host-image form: contexts kept per (device, shape, parameters) ----------------------------------------------
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
        int rc = omr_projection_batch_create(k.rows, k.cols, k.cn, k.max_angle, k.step, k.scale, k.device, kChunk, &raw);
        if (rc == OMR_OK) sp->reset(raw, omr_projection_batch_destroy);
        return rc;
    }, out);
}

struct HostArgs {
    const omr_image *srcs;
    uint16_t max_angle;
    double step, scale;
    int N;
    double *angles;
    int32_t *best_idx;
    int device;
    // omr_deskew_with_projections_batch: the deskewed images as well (null: the angles alone)
    omr_image_owned *rotated = nullptr;
    int interp = OMR_INTER_NEAREST;
    const uint8_t *border = nullptr;
};

// the per-call function, image by image: the buckets a batch context does not take
int bucket_per_call(const HostArgs &a, const std::vector<int> &idx)
{
    for (int i : idx) {
        int rc = omr_get_angle_with_projections(&a.srcs[i], a.max_angle, a.step, a.scale, 1, &a.angles[i]);
        if (rc) return rc;
        if (a.best_idx) a.best_idx[i] = (int32_t)llround(a.angles[i] / a.step) + a.N;
        if (a.rotated && (rc = omr_rotate(&a.srcs[i], a.angles[i], 1.0, a.interp, a.border, OMR_CLIP_CONTAIN, &a.rotated[i]))) return rc;
    }
    return OMR_OK;
}

int host_bucket(const HostArgs &a, int rows, int cols, int cn, const std::vector<int> &idx)
{
    if (cn == 4) return bucket_per_call(a, idx);
    std::shared_ptr<omr_projection_batch> pbp;
    int rc = cached_context(CtxKey{a.device, rows, cols, cn, a.max_angle, a.step, a.scale}, &pbp);
    if (rc == OMR_ERR_NOTIMPL || rc == OMR_ERR_BADARG || rc == OMR_ERR_ASSERT) {  // a sweep the batch context cannot plan
        clear_error();
        return bucket_per_call(a, idx);
    }
    if (rc) return rc;
    omr_projection_batch *pb = pbp.get();
    if (a.rotated && !pb->dk.count()) return bucket_per_call(a, idx);  // a canvas the warp's tables cannot hold
    // with canvases a run carries 32 scans: scan and slot of an A4 colour sheet are 26 + 54 MB on the device
    const int m = (int)idx.size(), zmax = std::min(m, a.rotated ? kDeskewChunk : kChunk);
    const int64_t row = (int64_t)cols * cn, in_stride = (row * rows + 255) & ~(int64_t)255;
    const int64_t out_step = (int64_t)pb->dk.cols * cn, out_stride = out_step * pb->dk.rows;
    LeasedStream st;  // the batch's device buffers come from the block cache and return to it when the call ends
    if ((rc = st.create())) return rc;
    DevBuf din, dout;
    OMR_HIP(din.alloc((size_t)zmax * in_stride));
    if (a.rotated) OMR_HIP(dout.alloc((size_t)zmax * out_stride));
    std::vector<double> ang((size_t)zmax);
    std::vector<int32_t> best((size_t)zmax), size(2 * (size_t)zmax);
    for (int j0 = 0; j0 < m; j0 += zmax) {
        const int z = std::min(zmax, m - j0);
        // host memory -> device, from several threads
        if ((rc = upload_chunk(a.srcs, idx, j0, z, rows, row, din.as<uint8_t>(), in_stride))) return rc;
        rc = a.rotated ? omr_projection_batch_deskew_device(pb, din.as<uint8_t>(), in_stride, row, z, a.interp, a.border, dout.as<uint8_t>(),
                                                            out_stride, out_step, size.data(), ang.data(), best.data())
                       : omr_projection_batch_run_device(pb, din.as<uint8_t>(), in_stride, row, z, ang.data(), best.data(), nullptr, nullptr);
        if (rc) return rc;
        for (int j = 0; j < z; j++) {
            const int i = idx[(size_t)(j0 + j)];
            a.angles[i] = ang[(size_t)j];
            if (a.best_idx) a.best_idx[i] = best[(size_t)j];
        }
        // canvases -> fresh host images, from several threads
        if (a.rotated && (rc = download_canvases(dout.as<uint8_t>(), out_stride, out_step, cn, size.data(), nullptr, idx, j0, z, a.rotated)))
            return rc;
    }
    return OMR_OK;
}

// both host forms: every image checked as the per-call function checks it, then bucket by bucket; the caller's arrays
// are written only when the whole call has succeeded
int host_form(const omr_image *srcs, int n, uint16_t max_angle, double step, double scale, double *angles, int32_t *best_idx,
              omr_image_owned *rotated, int interp, const uint8_t *border)
{
    int N = 0;
    if (candidate_count(max_angle, step, &N) <= 0)
        return fail(OMR_ERR_BADARG, "empty candidate range (the reference indexes [0] and panics)");
    ShapeBuckets b;
    // omr_get_angle_with_projections' checks, for every image before any device work
    int rc = bucket_by_shape(srcs, n, [&](const omr_image &im) -> int {
        Working w;
        int rc = check_image(&im, cn_gray_source);
        return rc ? rc : working_size(im.rows, im.cols, scale, &w);
    }, &b);
    if (rc || (rc = have_device())) return rc;
    int dev = 0;
    OMR_HIP(hipGetDevice(&dev));
    std::vector<double> ang((size_t)n);
    std::vector<int32_t> best((size_t)n);
    std::vector<omr_image_owned> rot(rotated ? (size_t)n : 0, omr_image_owned{nullptr, 0, 0, 0, 0});
    HostArgs a{srcs, max_angle, step, scale, N, ang.data(), best.data(), dev};
    a.rotated = rotated ? rot.data() : nullptr, a.interp = interp, a.border = border;
    for (size_t k = 0; k < b.shapes.size() && rc == OMR_OK; k++)
        rc = host_bucket(a, b.shapes[k].rows, b.shapes[k].cols, b.shapes[k].cn, b.members[k]);
    if (rc) {
        for (auto &o : rot) omr_image_free(&o);
        return rc;
    }
    memcpy(angles, ang.data(), sizeof(double) * (size_t)n);
    if (best_idx) memcpy(best_idx, best.data(), sizeof(int32_t) * (size_t)n);
    if (rotated) memcpy(rotated, rot.data(), sizeof(omr_image_owned) * (size_t)n);
    return OMR_OK;
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

}  // extern "C"

namespace {

// ---- the streams form: file contents in, file contents out --------------------------------------
// Everything is indexed by the accepted sheets (those whose header parsed and whose working size exists), in call order.
struct StreamArgs {
    const uint8_t *const *streams;
    const int64_t *len;
    ImreadHeaders hd;  // sheet k's header stands in the array of its kind, hd.kind[k]
    int cn;
    uint16_t max_angle;
    double step, scale;
    int N;
    int interp;
    const uint8_t *border;
    OutFormat fmt;  // what writes the canvases
    double *angles;
    int32_t *best_idx, *scan_rc;
    uint8_t **out;  // null (with out_len): the angles alone
    int64_t *out_len;
    int device;
};

// a code of the per-call chain that belongs to its sheet (any other ends the call)
bool sheet_code(int rc) { return rc == OMR_ERR_ASSERT || rc == OMR_ERR_BADARG || rc == OMR_ERR_NOTIMPL; }

// the per-call chain, sheet by sheet: the buckets a batch context does not take
int streams_per_call(const StreamArgs &a, const std::vector<int> &idx)
{
    for (int k : idx) {
        omr_image_owned img{nullptr, 0, 0, 0, 0}, rot{nullptr, 0, 0, 0, 0};
        uint8_t *bytes = nullptr;
        int64_t cap = 0, used = 0;
        int rc = omr_imread(a.streams[k], a.len[k], a.cn, 0, &img);
        const omr_image view{img.data, img.rows, img.cols, img.channels, img.step_bytes};
        if (!rc) rc = omr_get_angle_with_projections(&view, a.max_angle, a.step, a.scale, 1, &a.angles[k]);
        if (!rc && a.out) {
            rc = omr_rotate(&view, a.angles[k], 1.0, a.interp, a.border, OMR_CLIP_CONTAIN, &rot);
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
            a.scan_rc[k] = rc, a.angles[k] = 0.0, a.best_idx[k] = -1;
            continue;
        }
        a.best_idx[k] = (int32_t)llround(a.angles[k] / a.step) + a.N;
        if (a.out) {
            uint8_t *fit = (uint8_t *)realloc(bytes, (size_t)std::max<int64_t>(used, 1));  // the bound is several times the stream
            a.out[k] = fit ? fit : bytes, a.out_len[k] = used;
        }
    }
    clear_error();
    return OMR_OK;
}

int streams_bucket(const StreamArgs &a, int rows, int cols, const std::vector<int> &idx)
{
    const int cn = a.cn;
    std::shared_ptr<omr_projection_batch> pbp;
    int rc = cached_context(CtxKey{a.device, rows, cols, cn, a.max_angle, a.step, a.scale}, &pbp);
    if (rc == OMR_ERR_NOTIMPL || rc == OMR_ERR_BADARG || rc == OMR_ERR_ASSERT) {  // a sweep the batch context cannot plan
        clear_error();
        return streams_per_call(a, idx);
    }
    if (rc) return rc;
    omr_projection_batch *pb = pbp.get();
    if (a.out && !pb->dk.count()) return streams_per_call(a, idx);  // a canvas the warp's tables cannot hold
    const int m = (int)idx.size(), zmax = std::min(m, a.out ? kDeskewChunk : kChunk);
    const int64_t row = (int64_t)cols * cn, in_stride = (row * rows + 255) & ~(int64_t)255;
    const int64_t out_step = (int64_t)pb->dk.cols * cn, out_stride = out_step * pb->dk.rows;
    LeasedStream st;  // the batch's device buffers come from the block cache and return to it when the call ends
    if ((rc = st.create())) return rc;
    DevBuf din, dout;
    OMR_HIP(din.alloc((size_t)zmax * in_stride));
    if (a.out) OMR_HIP(dout.alloc((size_t)zmax * out_stride));
    std::vector<double> ang((size_t)zmax);
    std::vector<int32_t> best((size_t)zmax), size(2 * (size_t)zmax);
    ImreadChunk ck;
    for (int j0 = 0; j0 < m; j0 += zmax) {
        const int z = std::min(zmax, m - j0);
        // the chunk's streams -> the scan slots, decoded on the device; a bucket may hold both kinds: each decoder fills
        // its own members' slots and skips the other's
        // (JPEG members that imread turns -- the bucket's shape is their turned one -- go through a scratch buffer of the
        // chunk, which one launch turns into their slots)
        ck.gather(a.hd, a.streams, a.len, idx, j0, z);
        if ((rc = imread_decode_device(ck.zs.data(), ck.zlen.data(), ck.hd.view(), nullptr, z, cn, false, din.as<uint8_t>(), in_stride, row, ck.zrc.data(), st.s)))
            return rc;
        rc = a.out ? omr_projection_batch_deskew_device(pb, din.as<uint8_t>(), in_stride, row, z, a.interp, a.border, dout.as<uint8_t>(),
                                                        out_stride, out_step, size.data(), ang.data(), best.data())
                   : omr_projection_batch_run_device(pb, din.as<uint8_t>(), in_stride, row, z, ang.data(), best.data(), nullptr, nullptr);
        if (rc) return rc;
        for (int j = 0; j < z; j++) {
            const int k = idx[(size_t)(j0 + j)];
            if (ck.zrc[(size_t)j]) {  // damaged image data: the slot's content means nothing; its code and no output
                a.scan_rc[k] = ck.zrc[(size_t)j], a.angles[k] = 0.0, a.best_idx[k] = -1;
                size[2 * (size_t)j] = size[2 * (size_t)j + 1] = 0;
            } else {
                a.angles[k] = ang[(size_t)j], a.best_idx[k] = best[(size_t)j];
            }
        }
        if (!a.out) continue;
        // the canvases stay on the device: encoded there, only the streams come down
        StreamSink sink(a.out, a.out_len, idx, j0);
        if ((rc = a.fmt.encode_device(dout.as<uint8_t>(), out_stride, out_step, cn, size.data(), z, sink, st.s))) return rc;
    }
    return OMR_OK;
}

// omr_deskew_with_projections_batch_streams and its PNG and TIFF forms: `out` receives the streams of any kind
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
    for (int i = 0; i < n; i++)
        if (!streams[i] || len[i] < 0) return fail(OMR_ERR_BADARG, "streams[%d] is null or has a negative length", i);
    int N = 0;
    if (candidate_count(max_angle, step, &N) <= 0)
        return fail(OMR_ERR_BADARG, "empty candidate range (the reference indexes [0] and panics)");
    if (!isfinite(scale) || scale <= 0.0) return fail(OMR_ERR_BADARG, "resize_scale must be finite and positive");
    if (interp != OMR_INTER_NEAREST && interp != OMR_INTER_LINEAR)
        return fail(OMR_ERR_NOTIMPL, "interpolation flag %d is not implemented", interp);
    // the headers, on the host: a sheet its decoder refuses, or for which the per-call function would fail, keeps its
    // code and leaves the batch here
    std::vector<int32_t> code((size_t)n, OMR_OK);
    ImreadRun run;
    std::vector<int> at;
    std::vector<omr_image> views;
    std::vector<const uint8_t *> zs;
    std::vector<int64_t> zlen;
    run.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        // imread turns a JPEG by its EXIF orientation: the scan's shape is the turned one
        const ImreadParsed ps = run.append(streams[i], len[i], channels, false);
        int rc = ps.rc;
        const int rows = ps.rows, cols = ps.cols;
        Working w;
        if (!rc) rc = working_size(rows, cols, scale, &w);
        if ((code[(size_t)i] = rc)) {
            run.drop_last();
            continue;
        }
        at.push_back(i), zs.push_back(streams[i]), zlen.push_back(len[i]);
        views.push_back(omr_image{streams[i], rows, cols, channels, (int64_t)cols * channels});
    }
    clear_error();
    const int g = (int)at.size();
    std::vector<double> ang((size_t)g, 0.0);
    std::vector<int32_t> best((size_t)g, -1), src((size_t)g, OMR_OK);
    std::vector<uint8_t *> bytes((size_t)g, nullptr);
    std::vector<int64_t> bytes_len((size_t)g, 0);
    int rc = OMR_OK;
    if (g) {
        ShapeBuckets b;
        if ((rc = bucket_by_shape(views.data(), g, [](const omr_image &) { return (int)OMR_OK; }, &b))) return rc;
        if (out) {  // the encoders' offsets inside an image are 32-bit: a shape whose canvas slot could exceed them refuses the
                    // call, before any device work (a shape without a canvas goes sheet by sheet)
            const int A = candidate_count(max_angle, step, nullptr);
            std::vector<double> cand((size_t)A);
            for (int i = 0; i < A; i++) cand[(size_t)i] = (double)(i - N) * step;
            for (const ImageShape &sh : b.shapes) {
                DeskewTables dk;
                if (dk.plan(sh.rows, sh.cols, cand.data(), A)) {
                    clear_error();
                    continue;
                }
                if ((rc = fmt.check_canvas(dk.rows, dk.cols, sh.cn))) return rc;
            }
        }
        if ((rc = have_device())) return rc;
        int dev = 0;
        OMR_HIP(hipGetDevice(&dev));
        StreamArgs a{zs.data(), zlen.data(), run.view(), channels, max_angle, step, scale, N, interp,
                     border, fmt, ang.data(), best.data(), src.data(), out ? bytes.data() : nullptr,
                     out ? bytes_len.data() : nullptr, dev};
        for (size_t k = 0; k < b.shapes.size() && rc == OMR_OK; k++) rc = streams_bucket(a, b.shapes[k].rows, b.shapes[k].cols, b.members[k]);
        if (rc) {
            for (uint8_t *p : bytes) free(p);
            return rc;
        }
    }
    // every sheet is decided: the caller's arrays are written only now
    for (int i = 0; i < n; i++) {
        angles[i] = 0.0, scan_rc[i] = code[(size_t)i];
        if (best_idx) best_idx[i] = -1;
        if (out) out[i] = nullptr, out_len[i] = 0;
    }
    for (int k = 0; k < g; k++) {
        const int i = at[(size_t)k];
        angles[i] = ang[(size_t)k], scan_rc[i] = src[(size_t)k];
        if (best_idx) best_idx[i] = best[(size_t)k];
        if (out) out[i] = bytes[(size_t)k], out_len[i] = bytes_len[(size_t)k];
    }
    return OMR_OK;
}

}  // namespace

extern "C" {

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
