// oics_rotate.cpp -- the fixed-point weight tables of warpAffine's INTER_CUBIC and INTER_LANCZOS4 (OpenCV 4.6.0
// imgwarp.cpp initInterTab1D / initInterTab2D(method, fixpt = true)), built once per process on the host with the
// C library's sin / cos (the file is built -ffp-contract=off: every float and double operation rounds as OpenCV's
// scalar code does) and uploaded once per device.  warp_affine.hip reads them; omr_warp_coeff_table exports them.
// Below them, rotate_mat for a batch with an angle per image (omr_rotate_batch_canvas / omr_rotate_batch_device_ex):
// the n matrices come from the host's libm exactly as omr_rotate*'s do and travel in one upload; the kernels are
// omr_rotate_device_ex's, launched once with the image index in blockIdx.z.
#include <float.h>
#include <math.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/omrdeskew.h"
#include "engine.hpp"

namespace omr {
namespace {

const int INTER_TAB_SIZE = 32;
const int INTER_REMAP_COEF_SCALE = 1 << 15;

// interpolateCubic
void interpolate_cubic(float x, float *coeffs)
{
    const float A = -0.75f;
    coeffs[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    coeffs[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    coeffs[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    coeffs[3] = 1.f - coeffs[0] - coeffs[1] - coeffs[2];
}

// interpolateLanczos4
void interpolate_lanczos4(float x, float *coeffs)
{
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const double CV_PI_ = 3.1415926535897932384626433832795;
    if (x < FLT_EPSILON) {
        for (int i = 0; i < 8; i++) coeffs[i] = 0;
        coeffs[3] = 1;
        return;
    }
    float sum = 0;
    double y0 = -(x + 3) * CV_PI_ * 0.25, s0 = sin(y0), c0 = cos(y0);
    for (int i = 0; i < 8; i++) {
        float y0_ = (x + 3 - i);
        if (fabsf(y0_) >= 1e-6f) {
            double y = -y0_ * CV_PI_ * 0.25;
            coeffs[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        } else {
            coeffs[i] = 1e30f;  // the singular tap
        }
        sum += coeffs[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; i++) coeffs[i] *= sum;
}

short sat_short_f(float v)
{
    int r = (int)lrintf(v);  // cvRound: nearest, ties to even
    return (short)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}

// initInterTab2D(method, fixpt = true): entry (i = fy, j = fx), tap (k1 = row, k2 = col)
std::vector<int16_t> build_tab(int method)
{
    const int ksize = method == OMR_INTER_CUBIC ? 4 : 8;
    float tab1[8 * INTER_TAB_SIZE];
    for (int i = 0; i < INTER_TAB_SIZE; i++) {
        const float x = i * (1.f / INTER_TAB_SIZE);
        if (method == OMR_INTER_CUBIC) interpolate_cubic(x, tab1 + i * 4);
        else interpolate_lanczos4(x, tab1 + i * 8);
    }
    std::vector<int16_t> out((size_t)INTER_TAB_SIZE * INTER_TAB_SIZE * ksize * ksize);
    int16_t *itab = out.data();
    for (int i = 0; i < INTER_TAB_SIZE; i++)
        for (int j = 0; j < INTER_TAB_SIZE; j++, itab += ksize * ksize) {
            int isum = 0;
            for (int k1 = 0; k1 < ksize; k1++) {
                float vy = tab1[i * ksize + k1];
                for (int k2 = 0; k2 < ksize; k2++) {
                    float v = vy * tab1[j * ksize + k2];
                    isum += itab[k1 * ksize + k2] = sat_short_f(v * INTER_REMAP_COEF_SCALE);
                }
            }
            if (isum != INTER_REMAP_COEF_SCALE) {
                int diff = isum - INTER_REMAP_COEF_SCALE;
                int ksize2 = ksize / 2, Mk1 = ksize2, Mk2 = ksize2, mk1 = ksize2, mk2 = ksize2;
                for (int k1 = ksize2; k1 < ksize2 + 2; k1++)
                    for (int k2 = ksize2; k2 < ksize2 + 2; k2++) {
                        if (itab[k1 * ksize + k2] < itab[mk1 * ksize + mk2]) mk1 = k1, mk2 = k2;
                        else if (itab[k1 * ksize + k2] > itab[Mk1 * ksize + Mk2]) Mk1 = k1, Mk2 = k2;
                    }
                if (diff < 0) itab[Mk1 * ksize + Mk2] = (short)(itab[Mk1 * ksize + Mk2] - diff);
                else itab[mk1 * ksize + mk2] = (short)(itab[mk1 * ksize + mk2] - diff);
            }
        }
    return out;
}

std::mutex g_tab_mu;
const int16_t *g_dev_tab[16][2];  // [device][cubic, lanczos]: uploaded once, kept for the process

}  // namespace

const std::vector<int16_t> &warp_coeff_host(int interp)
{
    static const std::vector<int16_t> cubic = build_tab(OMR_INTER_CUBIC);  // magic statics: built once, thread-safe
    static const std::vector<int16_t> lanczos = build_tab(OMR_INTER_LANCZOS4);
    return interp == OMR_INTER_CUBIC ? cubic : lanczos;
}

int warp_coeff_device(int interp, const int16_t **d_tab)
{
    int dev;
    OMR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return fail(OMR_ERR_GPU, "device %d: at most 16 devices", dev);
    const int slot = interp == OMR_INTER_CUBIC ? 0 : 1;
    const std::vector<int16_t> &h = warp_coeff_host(interp);
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (!g_dev_tab[dev][slot]) {
        void *p = nullptr;
        OMR_HIP(hipMalloc(&p, h.size() * sizeof(int16_t)));
        hipError_t e = hipMemcpy(p, h.data(), h.size() * sizeof(int16_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fail_gpu("upload of the warp weight table", e);
        }
        g_dev_tab[dev][slot] = (const int16_t *)p;
    }
    *d_tab = g_dev_tab[dev][slot];
    return OMR_OK;
}

int rotate_batch_plan(int rows, int cols, const double *angles_deg, int n, double scale, int clip, bool inverse,
                      std::vector<WarpImg> *per, int *max_rows, int *max_cols)
{
    try {
        per->resize((size_t)n);
    } catch (const std::bad_alloc &) {
        return fail(OMR_ERR_NOMEM, "out of host memory for %d matrices", n);
    }
    *max_rows = *max_cols = 0;
    for (int i = 0; i < n; i++) {
        if (!isfinite(angles_deg[i])) return fail(OMR_ERR_BADARG, "angle %d is not finite", i);
        double M[6];
        int dr, dc;
        int rc = rotate_geometry(rows, cols, angles_deg[i], scale, clip, M, &dr, &dc);
        if (rc) return rc;
        WarpImg &w = (*per)[(size_t)i];
        if (inverse) memcpy(w.minv, M, sizeof w.minv);
        else invert_affine(M, w.minv);
        w.rows = dr, w.cols = dc;
        if (dr > *max_rows) *max_rows = dr;
        if (dc > *max_cols) *max_cols = dc;
    }
    return OMR_OK;
}

int rotate_batch_launch(const uint8_t *d_src, int64_t sstride, int64_t sstep, int rows, int cols, int cn,
                        const std::vector<WarpImg> &per, int max_rows, int max_cols, const WarpMode &m,
                        const uint8_t border_value[4], uint8_t *d_dst, int64_t dstride, int64_t dstep, hipStream_t s)
{
    const int n = (int)per.size();
    const int16_t *tab = nullptr;
    if (m.interp >= OMR_INTER_CUBIC) {
        int rc = warp_coeff_device(m.interp, &tab);
        if (rc) return rc;
    }
    const uint32_t border = (uint32_t)border_value[0] | ((uint32_t)border_value[1] << 8) | ((uint32_t)border_value[2] << 16) |
                            ((uint32_t)border_value[3] << 24);
    if (int rc = have_device()) return rc;
    if (n <= 3) {
        // the table's upload and the wait that gives it back cost about 20 us per call (profiles/r07_rotate_batch.md),
        // more than the launches they save: the same kernels, an image per launch, the matrix by value, no wait
        for (int i = 0; i < n; i++)
            OMR_HIP(launch_warp_affine(d_src + i * sstride, sstep, rows, cols, cn, d_dst + i * dstride, dstep, per[(size_t)i].rows,
                                       per[(size_t)i].cols, per[(size_t)i].minv, m.interp, m.border_mode, border, tab, s));
        return OMR_OK;
    }
    PoolScope scope(s);  // the table goes back to the block cache once `s` has drained
    DevBuf d_per;
    if (d_per.alloc(per.size() * sizeof(WarpImg)) != hipSuccess)
        return fail(OMR_ERR_NOMEM, "out of device memory for %d matrices", n);
    OMR_HIP(hipMemcpyAsync(d_per.p, per.data(), per.size() * sizeof(WarpImg), hipMemcpyHostToDevice, s));
    for (int i0 = 0; i0 < n; i0 += 65535)
        OMR_HIP(launch_warp_affine_batch(d_src + i0 * sstride, sstride, sstep, rows, cols, cn, d_dst + i0 * dstride, dstride, dstep,
                                         max_rows, max_cols, d_per.as<WarpImg>() + i0, n - i0 < 65535 ? n - i0 : 65535, m.interp,
                                         m.border_mode, border, tab, s));
    OMR_HIP(hipStreamSynchronize(s));  // the upload reads `per`, the kernels read the table: both go on return
    return OMR_OK;
}

}  // namespace omr

using namespace omr;

extern "C" int omr_rotate_batch_canvas(int32_t rows, int32_t cols, const double *angles_deg, int32_t n, int32_t clip,
                                       int32_t *max_rows, int32_t *max_cols, int32_t *out_size)
{
    if (!angles_deg || !max_rows || !max_cols || n <= 0 || rows <= 0 || cols <= 0) return fail(OMR_ERR_BADARG, "bad arguments");
    std::vector<WarpImg> per;
    int mr, mc, rc = rotate_batch_plan(rows, cols, angles_deg, n, 1.0, clip, false, &per, &mr, &mc);
    if (rc) return rc;
    if (out_size)
        for (int i = 0; i < n; i++) out_size[2 * i] = per[(size_t)i].rows, out_size[2 * i + 1] = per[(size_t)i].cols;
    *max_rows = mr;
    *max_cols = mc;
    return OMR_OK;
}

extern "C" int omr_rotate_batch_device_ex(const uint8_t *d_src, int32_t n, int64_t src_stride_bytes, int64_t src_step,
                                          int32_t rows, int32_t cols, int32_t channels, const double *angles_deg, double scale,
                                          int32_t flags, int32_t border_mode, const uint8_t border_value[4], int32_t clip,
                                          uint8_t *d_dst, int64_t dst_stride_bytes, int64_t dst_step, int32_t slot_rows,
                                          int32_t slot_cols, int32_t *out_size, void *stream)
{
    // omr_rotate_device_ex's checks and codes first, then the batch's own: all of them before any device work
    if (!d_src || !d_dst || !border_value) return fail(OMR_ERR_BADARG, "null pointer");
    if (n <= 0) return fail(OMR_ERR_BADARG, "batch of %d images", n);
    if (!angles_deg) return fail(OMR_ERR_BADARG, "null angle array");
    if (rows <= 0 || cols <= 0 || rows >= 32767 || cols >= 32767 || channels < 1 || channels > 4)
        return fail(OMR_ERR_ASSERT, "bad image shape");
    WarpMode m;
    int rc = rotate_ex_args(flags, border_mode, &m);
    if (rc) return rc;
    std::vector<WarpImg> per;
    int mr, mc;
    if ((rc = rotate_batch_plan(rows, cols, angles_deg, n, scale, clip, m.inverse, &per, &mr, &mc))) return rc;
    if (slot_rows < mr || slot_cols < mc) return fail(OMR_ERR_BADARG, "slot %dx%d smaller than the largest canvas %dx%d", slot_cols, slot_rows, mc, mr);
    if (src_step < (int64_t)cols * channels || dst_step < (int64_t)slot_cols * channels) return fail(OMR_ERR_BADARG, "step too small");
    if (src_stride_bytes < 0 || dst_stride_bytes < (int64_t)slot_rows * dst_step)
        return fail(OMR_ERR_BADARG, "image stride smaller than an image");
    // [first byte, last byte] of everything the call may read and may write
    const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (uint64_t)(n - 1) * src_stride_bytes + (uint64_t)(rows - 1) * src_step + (uint64_t)cols * channels;
    const uintptr_t t0 = (uintptr_t)d_dst, t1 = t0 + (uint64_t)(n - 1) * dst_stride_bytes + (uint64_t)(slot_rows - 1) * dst_step + (uint64_t)slot_cols * channels;
    if (s0 < t1 && t0 < s1) return fail(OMR_ERR_BADARG, "source and destination overlap");
    if (out_size)
        for (int i = 0; i < n; i++) out_size[2 * i] = per[(size_t)i].rows, out_size[2 * i + 1] = per[(size_t)i].cols;
    return rotate_batch_launch(d_src, src_stride_bytes, src_step, rows, cols, channels, per, mr, mc, m, border_value, d_dst,
                               dst_stride_bytes, dst_step, (hipStream_t)stream);
}

extern "C" int omr_warp_coeff_table(int32_t interp, int16_t *out, int32_t cap, int32_t *n_out)
{
    if (interp != OMR_INTER_CUBIC && interp != OMR_INTER_LANCZOS4)
        return fail(OMR_ERR_BADARG, "no weight table for interpolation %d", interp);
    const std::vector<int16_t> &t = warp_coeff_host(interp);
    if (n_out) *n_out = (int32_t)t.size();
    if (!out) return OMR_OK;
    if (cap < (int32_t)t.size()) return fail(OMR_ERR_BADARG, "cap %d < %d", cap, (int)t.size());
    memcpy(out, t.data(), t.size() * sizeof(int16_t));
    return OMR_OK;
}
