// projection_batch.cpp -- get_angle_with_projections (projection.rs:17-194) with its resize_scale for batches of scans
// (DESIGN.md section 4.12):
//
//   front end   scale_self on the colour scans (transfer.rs:66-91), one launch over the batch (projection_front.hip),
//               into the context's working buffer.  The dispatch is resize_ptr's (oics_host.cpp); the tap tables of a
//               fractional shrink are built by area_tab when the context is created and stay on the device.
//   sweep       the context's omr_batch_ctx for the working shape: gray (quirk B8) and threshold(127) fused into its
//               bit-packing loads, arg-max on the device.
//
// Scan i's angle is omr_get_angle_with_projections' for the same scan, as f64 bits.
#include <float.h>
#include <math.h>
#include <string.h>

#include <list>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/omrdeskew.h"
#include "engine.hpp"
#include "host_threads.hpp"
#include "hough_host.hpp"
#include "projection_front.hpp"

using namespace omr;
using namespace omr::hh;

namespace {

const int kChunk = 256;  // scans per run of the host form's contexts

// scale_self's size and resize_ptr's dispatch for it, on the host
struct Working {
    int wr = 0, wc = 0, mode = OMR_PROJECTION_FRONT_NONE, kx = 0, ky = 0;
    bool area_mode = false;  // LINEAR only: INTER_AREA's bilinear emulation (never reached by scale_self)
};

int check_shape(int rows, int cols)
{
    if (rows <= 0 || cols <= 0) return fail(OMR_ERR_ASSERT, "empty image");
    if (rows >= 32767 || cols >= 32767) return fail(OMR_ERR_ASSERT, "image dimension >= SHRT_MAX");
    return OMR_OK;
}

int working_size(int rows, int cols, double scale, Working *w)
{
    int rc = check_shape(rows, cols);
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
    if (dr == rows && dc == cols) return OMR_OK;  // resize() copies
    int interp = scale > 1.0 ? OMR_INTER_LINEAR : OMR_INTER_AREA;
    const double inv_scale_x = (double)dc / cols, inv_scale_y = (double)dr / rows;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    const int iscale_x = (int)lrint(scale_x), iscale_y = (int)lrint(scale_y);
    const bool fast = fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON;
    if (interp == OMR_INTER_LINEAR && fast && iscale_x == 2 && iscale_y == 2) interp = OMR_INTER_AREA;
    if (!(interp == OMR_INTER_AREA && scale_x >= 1 && scale_y >= 1)) {
        w->mode = OMR_PROJECTION_FRONT_LINEAR;
        w->area_mode = interp == OMR_INTER_AREA;
    } else if (fast) {
        w->mode = OMR_PROJECTION_FRONT_AREA_INT;
        w->kx = iscale_x, w->ky = iscale_y;
    } else {
        w->mode = OMR_PROJECTION_FRONT_AREA_GENERAL;
    }
    return OMR_OK;
}

int check_channels(int cn)
{
    if (cn == 4) return fail(OMR_ERR_NOTIMPL, "4-channel batches are not implemented (1 or 3 channels)");
    if (cn != 1 && cn != 3) return fail(OMR_ERR_ASSERT, "RGB2GRAY needs 3 or 4 channels, got %d", cn);
    return OMR_OK;
}

int grow(DevBuf *b, size_t bytes)
{
    if (b->bytes >= bytes) return OMR_OK;
    NoPoolScope owned;
    b->release();
    OMR_HIP(b->alloc(bytes));
    return OMR_OK;
}

int upload_table(DevBuf *b, const void *p, size_t bytes)
{
    OMR_HIP(b->alloc(bytes));
    OMR_HIP(hipMemcpy(b->p, p, bytes, hipMemcpyHostToDevice));
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
    DevBuf work, best, vsd, hsd, xt, xo, yt, yo;
    std::vector<int32_t> h_best;
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

// scale_self of n scans -> pb->work, on pb->s (nothing to do, and nothing written, in mode NONE)
int front_end(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n)
{
    const Working &w = pb->w;
    if (w.mode == OMR_PROJECTION_FRONT_NONE) return OMR_OK;
    if (w.mode == OMR_PROJECTION_FRONT_LINEAR) {
        OMR_HIP(launch_pf_linear(d_scans, scan_stride, step, pb->rows, pb->cols, pb->cn, n, pb->work.as<uint8_t>(), pb->wstride,
                                 pb->wstep, w.wr, w.wc, w.area_mode, pb->s));
        return OMR_OK;
    }
    PfArea p{};
    p.src = d_scans, p.scan_stride = scan_stride, p.sstep = step;
    p.dst = pb->work.as<uint8_t>(), p.out_stride = pb->wstride, p.dstep = pb->wstep;
    p.cn = pb->cn, p.scols = pb->cols, p.drows = w.wr, p.dcols = w.wc, p.kx = w.kx, p.ky = w.ky;
    p.xtab = pb->xt.as<AreaTap>(), p.xofs = pb->xo.as<int32_t>(), p.ytab = pb->yt.as<AreaTap>(), p.yofs = pb->yo.as<int32_t>();
    OMR_HIP(launch_pf_area(p, pb->tiling, n, pb->s));
    return OMR_OK;
}

int run_locked(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride, int64_t step, int n, double *angle,
               int32_t *best_idx, double *v_sd, double *h_sd)
{
    const size_t A = (size_t)pb->A;
    const bool scores = v_sd || h_sd;
    int rc;
    if (scores) {
        if ((rc = grow(&pb->vsd, sizeof(double) * (size_t)n * A))) return rc;
        if ((rc = grow(&pb->hsd, sizeof(double) * (size_t)n * A))) return rc;
    }
    if ((rc = front_end(pb, d_scans, scan_stride, step, n))) return rc;
    const bool resized = pb->w.mode != OMR_PROJECTION_FRONT_NONE;
    if (resized) OMR_HIP(hipStreamSynchronize(pb->s));  // the sweep runs on the batch context's own streams
    // projection.rs:29-32: RGB2GRAY and threshold(127) are fused into the sweep's loads
    if ((rc = omr_batch_run_device_cn(pb->sweep, resized ? pb->work.as<uint8_t>() : d_scans, resized ? pb->wstride : scan_stride,
                                      resized ? pb->wstep : step, pb->cn, n, 127, pb->best.as<int32_t>(),
                                      scores ? pb->vsd.as<double>() : nullptr, scores ? pb->hsd.as<double>() : nullptr)))
        return rc;
    if ((rc = omr_batch_sync(pb->sweep))) return rc;
    OMR_HIP(hipMemcpyAsync(pb->h_best.data(), pb->best.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, pb->s));
    if (v_sd) OMR_HIP(hipMemcpyAsync(v_sd, pb->vsd.p, sizeof(double) * (size_t)n * A, hipMemcpyDeviceToHost, pb->s));
    if (h_sd) OMR_HIP(hipMemcpyAsync(h_sd, pb->hsd.p, sizeof(double) * (size_t)n * A, hipMemcpyDeviceToHost, pb->s));
    OMR_HIP(hipStreamSynchronize(pb->s));
    for (int i = 0; i < n; i++) {
        const int idx = pb->h_best[(size_t)i];
        angle[i] = ((double)idx - (double)pb->N) * pb->step;  // projection.rs:189-190
        if (best_idx) best_idx[i] = idx;
    }
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
std::mutex g_ctx_mu;
std::list<std::pair<CtxKey, std::shared_ptr<omr_projection_batch>>> g_ctx;  // most recent first, at most kCachedContexts
const size_t kCachedContexts = 4;

int cached_context(const CtxKey &k, std::shared_ptr<omr_projection_batch> *out)
{
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        for (auto it = g_ctx.begin(); it != g_ctx.end(); ++it)
            if (it->first == k) {
                *out = it->second;
                g_ctx.splice(g_ctx.begin(), g_ctx, it);
                return OMR_OK;
            }
    }
    omr_projection_batch *raw = nullptr;
    int rc = omr_projection_batch_create(k.rows, k.cols, k.cn, k.max_angle, k.step, k.scale, k.device, kChunk, &raw);
    if (rc) return rc;
    std::shared_ptr<omr_projection_batch> sp(raw, omr_projection_batch_destroy);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    g_ctx.emplace_front(k, sp);
    while (g_ctx.size() > kCachedContexts) g_ctx.pop_back();
    *out = sp;
    return OMR_OK;
}

struct HostArgs {
    const omr_image *srcs;
    uint16_t max_angle;
    double step, scale;
    int N;
    double *angles;
    int32_t *best_idx;
    int device;
};

// the per-call function, image by image: the buckets a batch context does not take
int bucket_per_call(const HostArgs &a, const std::vector<int> &idx)
{
    for (int i : idx) {
        int rc = omr_get_angle_with_projections(&a.srcs[i], a.max_angle, a.step, a.scale, 1, &a.angles[i]);
        if (rc) return rc;
        if (a.best_idx) a.best_idx[i] = (int32_t)llround(a.angles[i] / a.step) + a.N;
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
    const int m = (int)idx.size(), zmax = std::min(m, kChunk);
    const int64_t row = (int64_t)cols * cn, in_stride = (row * rows + 255) & ~(int64_t)255;
    HStream st;  // the batch's device buffer comes from the block cache and returns to it when the call ends
    if ((rc = st.create())) return rc;
    DevBuf din;
    OMR_HIP(din.alloc((size_t)zmax * in_stride));
    std::vector<double> ang((size_t)zmax);
    std::vector<int32_t> best((size_t)zmax);
    for (int j0 = 0; j0 < m; j0 += zmax) {
        const int z = std::min(zmax, m - j0);
        rc = on_threads(z, [&](hipStream_t s, int lo, int hi) -> int {  // host memory -> device, from several threads
            for (int j = lo; j < hi; j++) {
                const omr_image &im = a.srcs[idx[(size_t)(j0 + j)]];
                uint8_t *d = din.as<uint8_t>() + (size_t)j * in_stride;
                if (im.step_bytes == row)
                    OMR_HIP(hipMemcpyAsync(d, im.data, (size_t)row * rows, hipMemcpyHostToDevice, s));
                else
                    OMR_HIP(hipMemcpy2DAsync(d, (size_t)row, im.data, (size_t)im.step_bytes, (size_t)row, (size_t)rows,
                                             hipMemcpyHostToDevice, s));
            }
            OMR_HIP(hipStreamSynchronize(s));
            return OMR_OK;
        });
        if (rc) return rc;
        if ((rc = omr_projection_batch_run_device(pb, din.as<uint8_t>(), in_stride, row, z, ang.data(), best.data(), nullptr, nullptr)))
            return rc;
        for (int j = 0; j < z; j++) {
            const int i = idx[(size_t)(j0 + j)];
            a.angles[i] = ang[(size_t)j];
            if (a.best_idx) a.best_idx[i] = best[(size_t)j];
        }
    }
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
    *wrows = w.wr, *wcols = w.wc, *front_mode = w.mode;
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
    int rc = check_shape(rows, cols);
    if (rc) return rc;
    if ((rc = check_channels(channels))) return rc;
    int N = 0;
    const int A = candidate_count(max_angle, step, &N);
    if (A <= 0) return fail(OMR_ERR_BADARG, "empty candidate range");
    Working w;
    if ((rc = working_size(rows, cols, resize_scale, &w))) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(OMR_ERR_GPU, "no usable HIP device (there is no CPU fallback)");
    if (device >= ndev) return fail(OMR_ERR_BADARG, "device %d of %d", device, ndev);
    OMR_HIP(hipSetDevice(device));
    NoPoolScope owned;
    std::unique_ptr<omr_projection_batch> pb(new omr_projection_batch);
    pb->device = device, pb->rows = rows, pb->cols = cols, pb->cn = channels, pb->max_scans = max_scans;
    pb->step = step, pb->N = N, pb->A = A, pb->w = w;
    pb->h_best.assign((size_t)max_scans, 0);
    OMR_HIP(hipStreamCreateWithFlags(&pb->s, hipStreamNonBlocking));
    OMR_HIP(pb->best.alloc(sizeof(int32_t) * (size_t)max_scans));
    if (w.mode != OMR_PROJECTION_FRONT_NONE) {
        pb->wstep = ((int64_t)w.wc * channels + 3) & ~(int64_t)3;
        pb->wstride = ((int64_t)w.wr * pb->wstep + 255) & ~(int64_t)255;
        OMR_HIP(pb->work.alloc((size_t)max_scans * pb->wstride));
    }
    if (w.mode == OMR_PROJECTION_FRONT_AREA_GENERAL) {  // resizeArea_'s tap tables, once per context
        std::vector<AreaTap> xt, yt;
        std::vector<int32_t> xo, yo;
        area_tab(cols, w.wc, channels, 1. / ((double)w.wc / cols), &xt, &xo);
        area_tab(rows, w.wr, 1, 1. / ((double)w.wr / rows), &yt, &yo);
        pb->tiling = pf_area_tiling(channels, w.wc, 0, &xt, &xo, &yt);
        if ((rc = upload_table(&pb->xt, xt.data(), sizeof(AreaTap) * xt.size()))) return rc;
        if ((rc = upload_table(&pb->xo, xo.data(), sizeof(int32_t) * xo.size()))) return rc;
        if ((rc = upload_table(&pb->yt, yt.data(), sizeof(AreaTap) * yt.size()))) return rc;
        if ((rc = upload_table(&pb->yo, yo.data(), sizeof(int32_t) * yo.size()))) return rc;
    } else if (w.mode == OMR_PROJECTION_FRONT_AREA_INT) {
        pb->tiling = pf_area_tiling(channels, w.wc, w.kx, nullptr, nullptr, nullptr);
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
    if (front_mode) *front_mode = pb->w.mode;
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
    const bool resized = pb->w.mode != OMR_PROJECTION_FRONT_NONE;  // NONE: the working images are the scans
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

int omr_get_angles_with_projections_batch(const omr_image *srcs, int32_t n, uint16_t max_angle, double step, double resize_scale,
                                          double *angles, int32_t *best_idx)
{
    clear_error();
    if (!srcs || n < 1 || !angles) return fail(OMR_ERR_BADARG, "bad batch arguments");
    int N = 0;
    if (candidate_count(max_angle, step, &N) <= 0)
        return fail(OMR_ERR_BADARG, "empty candidate range (the reference indexes [0] and panics)");
    std::vector<std::tuple<int, int, int>> shapes;  // in order of first appearance
    std::vector<std::vector<int>> members;
    for (int i = 0; i < n; i++) {  // omr_get_angle_with_projections' checks, for every image before any device work
        const omr_image &im = srcs[i];
        if (!im.data) return fail(OMR_ERR_BADARG, "null image %d", i);
        int rc = check_shape(im.rows, im.cols);
        if (rc) return rc;
        if (im.channels < 1 || im.channels > 4) return fail(OMR_ERR_ASSERT, "unsupported channel count %d", im.channels);
        if (im.channels == 2) return fail(OMR_ERR_ASSERT, "RGB2GRAY needs 3 or 4 channels");
        if (im.step_bytes < (int64_t)im.cols * im.channels) return fail(OMR_ERR_BADARG, "step_bytes too small");
        Working w;
        if ((rc = working_size(im.rows, im.cols, resize_scale, &w))) return rc;
        const std::tuple<int, int, int> sh(im.rows, im.cols, im.channels);
        size_t k = 0;
        while (k < shapes.size() && shapes[k] != sh) k++;
        if (k == shapes.size()) {
            shapes.push_back(sh);
            members.emplace_back();
        }
        members[k].push_back(i);
    }
    int rc = have_device();
    if (rc) return rc;
    int dev = 0;
    OMR_HIP(hipGetDevice(&dev));
    // results go to the caller's arrays only when the whole call has succeeded
    std::vector<double> ang((size_t)n);
    std::vector<int32_t> best((size_t)n);
    const HostArgs a{srcs, max_angle, step, resize_scale, N, ang.data(), best.data(), dev};
    for (size_t k = 0; k < shapes.size() && rc == OMR_OK; k++)
        rc = host_bucket(a, std::get<0>(shapes[k]), std::get<1>(shapes[k]), std::get<2>(shapes[k]), members[k]);
    if (rc) return rc;
    memcpy(angles, ang.data(), sizeof(double) * (size_t)n);
    if (best_idx) memcpy(best_idx, best.data(), sizeof(int32_t) * (size_t)n);
    return OMR_OK;
}

}  // extern "C"
