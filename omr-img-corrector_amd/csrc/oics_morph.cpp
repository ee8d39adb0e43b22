// oics_morph.cpp -- TransformableMatrix::erode / dilate (transfer.rs:206-277) behind the C ABI: the structuring
// element of OpenCV 4.6.0's getStructuringElement as row spans, the argument checks (all of them before any
// device work) and the choice of kernels (morph.hip):
//   - no iterations, or a 1 x 1 element: a copy;
//   - a full rectangle: the iterations fold into ONE element (size k + (it - 1)(k - 1), anchor it * anchor: with
//     the neutral border that pass gives the bytes of the iterated form), its reach is clamped to the image (cells
//     that no pixel can reach take no part), and what is left runs as a chain of separable launches of at most
//     31 x 31 each -- reaches add up along a chain for the same reason the iterations fold;
//   - other elements up to 31 x 31: the LDS span kernel, as many passes per launch as its halo allows;
//   - larger ones: the global-memory span kernel, one pass per launch.
// Several launches alternate between the destination and one scratch image, so that the last one writes the
// destination; the source is never written.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/omrdeskew.h"
#include "engine.hpp"

namespace omr {
namespace {

// getStructuringElement (OpenCV 4.6.0 morph.dispatch.cpp): row i of the element is the run [j1, j2)
int check_element(int shape, int kw, int kh, int *ax, int *ay)
{
    if (shape != OMR_MORPH_RECT && shape != OMR_MORPH_CROSS && shape != OMR_MORPH_ELLIPSE)
        return fail(OMR_ERR_ASSERT, "unknown structuring element shape %d", shape);
    if (kw < 1 || kh < 1) return fail(OMR_ERR_ASSERT, "structuring element size %dx%d", kw, kh);
    if (*ax == -1) *ax = kw / 2;  // normalizeAnchor
    if (*ay == -1) *ay = kh / 2;
    if (*ax < 0 || *ax >= kw || *ay < 0 || *ay >= kh)
        return fail(OMR_ERR_ASSERT, "anchor (%d, %d) outside the %dx%d element", *ax, *ay, kw, kh);
    return OMR_OK;
}

int element_spans(int shape, int kw, int kh, int *ax, int *ay, std::vector<int32_t> *spans)
{
    int rc = check_element(shape, kw, kh, ax, ay);
    if (rc) return rc;
    if (kw == 1 && kh == 1) shape = OMR_MORPH_RECT;
    int r = 0, c = 0;
    double inv_r2 = 0;
    if (shape == OMR_MORPH_ELLIPSE) {
        r = kh / 2;
        c = kw / 2;
        inv_r2 = r ? 1. / ((double)r * r) : 0;
    }
    try {
        spans->assign((size_t)2 * kh, 0);
    } catch (const std::bad_alloc &) {
        return fail(OMR_ERR_NOMEM, "out of host memory for %d element rows", kh);
    }
    for (int i = 0; i < kh; i++) {
        int j1 = 0, j2 = 0;
        if (shape == OMR_MORPH_RECT || (shape == OMR_MORPH_CROSS && i == *ay)) {
            j2 = kw;
        } else if (shape == OMR_MORPH_CROSS) {
            j1 = *ax, j2 = j1 + 1;
        } else {
            const int dy = i - r;
            if (abs(dy) <= r) {
                const int dx = (int)lrint(c * sqrt(((double)r * r - (double)dy * dy) * inv_r2));  // cvRound
                j1 = std::max(c - dx, 0);
                j2 = std::min(c + dx + 1, kw);
            }
        }
        (*spans)[2 * i] = j1;
        (*spans)[2 * i + 1] = j2 - j1;
    }
    return OMR_OK;
}

int check_morph(const void *s, const void *d, int64_t sstep, int64_t dstep, int rows, int cols, int cn, int op, int it)
{
    if (!s || !d) return fail(OMR_ERR_BADARG, "null pointer");
    if (rows <= 0 || cols <= 0 || rows >= 32767 || cols >= 32767 || cn < 1 || cn > 4)
        return fail(OMR_ERR_ASSERT, "bad image shape");
    if (sstep < (int64_t)cols * cn || dstep < (int64_t)cols * cn) return fail(OMR_ERR_BADARG, "step too small");
    if (op != OMR_MORPH_ERODE && op != OMR_MORPH_DILATE) return fail(OMR_ERR_BADARG, "unknown morphology operation %d", op);
    if (it < 0) return fail(OMR_ERR_BADARG, "iterations %d < 0", it);
    if (s == d) return fail(OMR_ERR_BADARG, "erode / dilate cannot run in place");
    return OMR_OK;
}

struct Launch {  // one launch of a plan
    int kind;    // 0 rect, 1 LDS spans, 2 global spans
    int kw, kh, ax, ay, passes;
};

}  // namespace

int morph_check_args(const void *src, const void *dst, int64_t sstep, int64_t dstep, int rows, int cols, int cn, int op,
                     int shape, int kw, int kh, int ax, int ay, int iterations)
{
    int rc = check_morph(src, dst, sstep, dstep, rows, cols, cn, op, iterations);
    if (rc) return rc;
    return check_element(shape, kw, kh, &ax, &ay);
}

// arguments already checked (morph_check_args); synchronises `s` when it had to take a scratch image or a span table
int morph_device(const uint8_t *d_src, int64_t sstride, int64_t sstep, int n, int rows, int cols, int cn, int op, int shape,
                 int kw, int kh, int ax, int ay, int iterations, uint8_t *d_dst, int64_t dstride, int64_t dstep,
                 hipStream_t s)
{
    const int wb = cols * cn;
    std::vector<int32_t> spans;
    int rc = element_spans(shape, kw, kh, &ax, &ay, &spans);
    if (rc) return rc;
    if (iterations == 0 || (kw == 1 && kh == 1)) {
        for (int i = 0; i < n; i++)
            OMR_HIP(hipMemcpy2DAsync(d_dst + i * dstride, (size_t)dstep, d_src + i * sstride, (size_t)sstep, (size_t)wb,
                                     (size_t)rows, hipMemcpyDeviceToDevice, s));
        return OMR_OK;
    }
    bool full = true;
    for (int i = 0; i < kh && full; i++) full = spans[2 * i] == 0 && spans[2 * i + 1] == kw;

    std::vector<Launch> plan;
    if (full) {
        // reach of the folded element on each side, clamped to what a pixel of the image can see
        int64_t L = std::min<int64_t>((int64_t)iterations * ax, cols - 1), R = std::min<int64_t>((int64_t)iterations * (kw - 1 - ax), cols - 1);
        int64_t T = std::min<int64_t>((int64_t)iterations * ay, rows - 1), B = std::min<int64_t>((int64_t)iterations * (kh - 1 - ay), rows - 1);
        while (L || R || T || B || plan.empty()) {
            const int l = (int)std::min<int64_t>(L, MORPH_MAXK - 1), r = (int)std::min<int64_t>(R, MORPH_MAXK - 1 - l);
            const int t = (int)std::min<int64_t>(T, MORPH_MAXK - 1), b = (int)std::min<int64_t>(B, MORPH_MAXK - 1 - t);
            plan.push_back(Launch{0, l + r + 1, t + b + 1, l, t, 1});
            L -= l, R -= r, T -= t, B -= b;
        }
    } else {
        const int f = morph_spans_lds_max_passes(kw, kh, ax, cn);
        try {
            if (f == 0) {
                plan.assign((size_t)iterations, Launch{2, kw, kh, ax, ay, 1});
            } else {
                const int launches = (iterations + f - 1) / f;
                for (int k = 0, left = iterations; k < launches; k++) {
                    const int p = (left + (launches - k) - 1) / (launches - k);
                    plan.push_back(Launch{1, kw, kh, ax, ay, p});
                    left -= p;
                }
            }
        } catch (const std::bad_alloc &) {
            return fail(OMR_ERR_NOMEM, "out of host memory for %d passes", iterations);
        }
    }

    MorphSpans sp{};
    DevBuf d_spans, scratch;
    bool drain = false;
    if (!full && plan[0].kind == 1)
        for (int i = 0; i < kh; i++) sp.j1[i] = (uint8_t)spans[2 * i], sp.len[i] = (uint8_t)spans[2 * i + 1];
    if (!full && plan[0].kind == 2) {
        if (d_spans.alloc(spans.size() * sizeof(int32_t)) != hipSuccess)
            return fail(OMR_ERR_NOMEM, "out of device memory for %d element rows", kh);
        OMR_HIP(hipMemcpyAsync(d_spans.p, spans.data(), spans.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        drain = true;
    }
    const int64_t tstep = (wb + 3) & ~3, tstride = tstep * rows;
    if (plan.size() > 1) {
        if (scratch.alloc((size_t)tstride * n) != hipSuccess)
            return fail(OMR_ERR_NOMEM, "out of device memory for the %d x %d x %d intermediate images", n, cols, rows);
        drain = true;
    }
    for (size_t k = 0; k < plan.size(); k++) {
        const Launch &l = plan[k];
        // launch k reads what launch k - 1 wrote; the last one writes the destination
        const bool to_dst = ((plan.size() - 1 - k) & 1) == 0, from_src = k == 0;
        for (int i0 = 0; i0 < n; i0 += 65535) {
            MorphImg im;
            im.n = std::min(n - i0, 65535);
            im.rows = rows, im.wbytes = wb, im.cn = cn;
            if (from_src) im.src = d_src + i0 * sstride, im.sstride = sstride, im.sstep = sstep;
            else if (to_dst) im.src = scratch.as<uint8_t>() + i0 * tstride, im.sstride = tstride, im.sstep = tstep;
            else im.src = d_dst + i0 * dstride, im.sstride = dstride, im.sstep = dstep;
            if (to_dst) im.dst = d_dst + i0 * dstride, im.dstride = dstride, im.dstep = dstep;
            else im.dst = scratch.as<uint8_t>() + i0 * tstride, im.dstride = tstride, im.dstep = tstep;
            if (l.kind == 0) OMR_HIP(launch_morph_rect(im, op, l.kw, l.kh, l.ax, l.ay, s));
            else if (l.kind == 1) OMR_HIP(launch_morph_spans_lds(im, op, sp, l.kw, l.kh, l.ax, l.ay, l.passes, s));
            else OMR_HIP(launch_morph_spans_global(im, op, d_spans.as<int32_t>(), l.kh, l.ax, l.ay, s));
        }
    }
    if (drain) OMR_HIP(hipStreamSynchronize(s));  // the scratch image and the span table are freed on return
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" int omr_structuring_element(int32_t shape, int32_t kw, int32_t kh, int32_t ax, int32_t ay, uint8_t *out)
{
    if (!out) return fail(OMR_ERR_BADARG, "null output");
    std::vector<int32_t> spans;
    int rc = element_spans(shape, kw, kh, &ax, &ay, &spans);
    if (rc) return rc;
    memset(out, 0, (size_t)kw * kh);
    for (int i = 0; i < kh; i++) memset(out + (size_t)i * kw + spans[2 * i], 1, (size_t)spans[2 * i + 1]);
    return OMR_OK;
}

extern "C" int omr_morph_batch_device(const uint8_t *d_src, int32_t n, int64_t src_stride_bytes, int64_t src_step,
                                      int32_t rows, int32_t cols, int32_t channels, int32_t op, int32_t shape, int32_t kw,
                                      int32_t kh, int32_t ax, int32_t ay, int32_t iterations, uint8_t *d_dst,
                                      int64_t dst_stride_bytes, int64_t dst_step, void *stream)
{
    if (n < 1) return fail(OMR_ERR_BADARG, "batch of %d images", n);
    int rc = morph_check_args(d_src, d_dst, src_step, dst_step, rows, cols, channels, op, shape, kw, kh, ax, ay, iterations);
    if (rc) return rc;
    if (n > 1 && (src_stride_bytes < src_step * rows || dst_stride_bytes < dst_step * rows))
        return fail(OMR_ERR_BADARG, "image stride smaller than an image");
    return morph_device(d_src, src_stride_bytes, src_step, n, rows, cols, channels, op, shape, kw, kh, ax, ay, iterations,
                        d_dst, dst_stride_bytes, dst_step, (hipStream_t)stream);
}

extern "C" int omr_morph_device(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols, int32_t channels,
                                int32_t op, int32_t shape, int32_t kw, int32_t kh, int32_t ax, int32_t ay,
                                int32_t iterations, uint8_t *d_dst, int64_t dst_step, void *stream)
{
    int rc = morph_check_args(d_src, d_dst, src_step, dst_step, rows, cols, channels, op, shape, kw, kh, ax, ay, iterations);
    if (rc) return rc;
    return morph_device(d_src, 0, src_step, 1, rows, cols, channels, op, shape, kw, kh, ax, ay, iterations, d_dst, 0,
                        dst_step, (hipStream_t)stream);
}
