/*
 * detector_deskew_c_abi.c -- the Hough and FFT deskew flows from plain C: sheets of two shapes in one call of
 * omr_deskew_with_hough_batch / omr_deskew_with_fft_batch, then the calls' error paths (an invalid image in the middle of a
 * batch, refused file contents), which must return nothing and leave nothing allocated.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/detector_deskew_c_abi.c -o /tmp/detector_deskew_c_abi \
 *       -Lomr-img-corrector_amd/lib -lomrdeskew -Wl,-rpath,$PWD/omr-img-corrector_amd/lib -lm
 *   /tmp/detector_deskew_c_abi   # without a HIP device the accepted calls return -217, after all their host-side checks
 *
 * With the library's host code built -fsanitize=address,undefined this is the driver for a sanitizer run of the
 * bucketing, the header parsing and the ownership of the outputs on the error paths.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omrdeskew.h"

#define N 5

static uint8_t *sheet(int rows, int cols, int cn, double skew_deg)
{
    /* white page with black bars, rotated by -skew about the centre */
    const double a = skew_deg * 3.14159265358979323846 / 180.0, c = cos(a), s = sin(a);
    uint8_t *p = (uint8_t *)malloc((size_t)rows * cols * cn);
    if (!p) exit(2);
    memset(p, 255, (size_t)rows * cols * cn);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            const double u = (x - cols / 2.0) * c - (y - rows / 2.0) * s + cols / 2.0;
            const double v = (x - cols / 2.0) * s + (y - rows / 2.0) * c + rows / 2.0;
            if (((int)floor(v) / 12) % 3 == 0 && u > cols * 0.1 && u < cols * 0.9 && v > rows * 0.1 && v < rows * 0.9)
                memset(p + ((size_t)y * cols + x) * cn, 0, (size_t)cn);
        }
    return p;
}

static int fails = 0;
static void expect(const char *what, int got, int want_a, int want_b)
{
    const int ok = got == want_a || got == want_b;
    printf("%-58s: %d%s\n", what, got, ok ? "" : "   <-- unexpected");
    if (!ok) fails++;
}

int main(void)
{
    const int gpu = omr_device_count() > 0;
    const int run = gpu ? OMR_OK : OMR_ERR_GPU; /* what an accepted call answers here */
    printf("libomrdeskew version %d, %d HIP device(s)\n", omr_version(), omr_device_count());
    const int shape[N][3] = {{300, 400, 3}, {240, 180, 1}, {300, 400, 3}, {240, 180, 1}, {300, 400, 1}};
    const double skew[N] = {3.0, -5.0, 8.0, 12.0, -2.0};
    const uint8_t white[4] = {255, 255, 255, 0};
    omr_image img[N];
    for (int i = 0; i < N; i++) {
        img[i].data = sheet(shape[i][0], shape[i][1], shape[i][2], skew[i]);
        img[i].rows = shape[i][0], img[i].cols = shape[i][1], img[i].channels = shape[i][2];
        img[i].step_bytes = (int64_t)shape[i][1] * shape[i][2];
    }
    double angle[N];
    int32_t rc[N];
    omr_image_owned out[N];

    /* the two flows: mixed shapes and channel counts, results at their own indices */
    memset(out, 0, sizeof out);
    int r = omr_deskew_with_hough_batch(img, N, 60.0, 5.0, OMR_INTER_LINEAR, OMR_BORDER_CONSTANT, white, OMR_CLIP_CONTAIN, angle, rc, out);
    expect("omr_deskew_with_hough_batch", r, run, run);
    for (int i = 0; r == OMR_OK && i < N; i++) {
        printf("  sheet %d: rc %d, %.3f deg, canvas %d x %d x %d\n", i, rc[i], angle[i], out[i].cols, out[i].rows, out[i].channels);
        omr_image_free(&out[i]);
    }
    memset(out, 0, sizeof out);
    r = omr_deskew_with_fft_batch(img, N, 30.0, 90.0, 40.0, 5.0, OMR_INTER_NEAREST, OMR_BORDER_CONSTANT, white, OMR_CLIP_DEFAULT, angle, NULL, out);
    expect("omr_deskew_with_fft_batch (rc = NULL)", r, run, run);
    for (int i = 0; r == OMR_OK && i < N; i++) {
        printf("  sheet %d: %.3f deg, canvas %d x %d x %d\n", i, angle[i], out[i].cols, out[i].rows, out[i].channels);
        omr_image_free(&out[i]);
    }

    /* an invalid image in the middle fails the whole call before any device work: nothing is written */
    omr_image bad[N];
    memcpy(bad, img, sizeof bad);
    bad[2].channels = 2;
    memset(out, 0, sizeof out);
    angle[0] = 7.5, rc[0] = 77;
    expect("a 2-channel image in the middle", omr_deskew_with_hough_batch(bad, N, 60.0, 5.0, 1, 0, white, 1, angle, rc, out), OMR_ERR_ASSERT, OMR_ERR_ASSERT);
    bad[2] = img[2], bad[3].step_bytes = 7;
    expect("a pitch below a row", omr_deskew_with_fft_batch(bad, N, 30.0, 90.0, 40.0, 5.0, 1, 0, white, 1, angle, rc, out), OMR_ERR_BADARG, OMR_ERR_BADARG);
    bad[3] = img[3], bad[4].rows = 30000, bad[4].cols = 30000, bad[4].step_bytes = 30000;
    expect("a canvas slot past the image limit", omr_deskew_with_hough_batch(bad, N, 60.0, 5.0, 1, 0, white, 1, angle, rc, out), OMR_ERR_ASSERT, OMR_ERR_ASSERT);
    expect("unknown flag bits", omr_deskew_with_hough_batch(img, N, 60.0, 5.0, 64, 0, white, 1, angle, rc, out), OMR_ERR_BADARG, OMR_ERR_BADARG);
    for (int i = 0; i < N; i++)
        if (out[i].data) fails++, printf("  image %d was returned by a refused call\n", i);
    if (angle[0] != 7.5 || rc[0] != 77) fails++, printf("  a refused call wrote its outputs\n");

    /* file contents: refused streams keep their decoder's code, the call returns 0 and allocates nothing */
    static const uint8_t junk[4] = {0, 1, 2, 3}, soi[3] = {0xff, 0xd8, 0xff}, png_sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    const uint8_t *streams[3] = {junk, soi, png_sig};
    const int64_t len[3] = {4, 3, 8};
    uint8_t *bytes[3] = {(uint8_t *)1, (uint8_t *)1, (uint8_t *)1};
    int64_t bytes_len[3] = {9, 9, 9};
    int32_t scan_rc[3] = {0, 0, 0};
    for (int fft = 0; fft < 2; fft++)
        for (int format = 0; format < 2; format++) {
            r = fft ? omr_deskew_with_fft_batch_streams(streams, len, 3, 3, 30.0, 90.0, 40.0, 5.0, 1, 0, white, 1, format, 1, angle, scan_rc, bytes, bytes_len)
                    : omr_deskew_with_hough_batch_streams(streams, len, 3, 3, 60.0, 5.0, 1, 0, white, 1, format, 95, angle, scan_rc, bytes, bytes_len);
            expect("three refused streams", r, OMR_OK, OMR_OK);
            for (int i = 0; i < 3; i++)
                if (scan_rc[i] == 0 || bytes[i] || bytes_len[i] || angle[i] != 0.0) fails++, printf("  stream %d: rc %d\n", i, scan_rc[i]);
        }
    expect("the angles alone (NULL outputs)", omr_deskew_with_hough_batch_streams(streams, len, 3, 1, 60.0, 5.0, 1, 0, NULL, 1, 0, 95, angle, scan_rc, NULL, NULL), OMR_OK, OMR_OK);
    expect("one of out / out_len", omr_deskew_with_fft_batch_streams(streams, len, 3, 3, 30.0, 90.0, 40.0, 5.0, 1, 0, white, 1, 0, 95, angle, scan_rc, bytes, NULL), OMR_ERR_BADARG, OMR_ERR_BADARG);

    int32_t mr = 0, mc = 0;
    expect("omr_detector_deskew_canvas(3508, 2480, CONTAIN)", omr_detector_deskew_canvas(3508, 2480, OMR_CLIP_CONTAIN, &mr, &mc), OMR_OK, OMR_OK);
    printf("  slot %d x %d\n", mc, mr);
    for (int i = 0; i < N; i++) free((void *)img[i].data);
    printf(fails ? "%d check(s) failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
