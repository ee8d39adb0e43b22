// oics_rotate.cpp -- the fixed-point weight tables of warpAffine's INTER_CUBIC and INTER_LANCZOS4 (OpenCV 4.6.0
// imgwarp.cpp initInterTab1D / initInterTab2D(method, fixpt = true)), built once per process on the host with the
// C library's sin / cos (the file is built -ffp-contract=off: every float and double operation rounds as OpenCV's
// scalar code does) and uploaded once per device.  warp_affine.hip reads them; omr_warp_coeff_table exports them.
#include <float.h>
#include <math.h>
#include <string.h>

#include <mutex>
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

}  // namespace omr

using namespace omr;

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
