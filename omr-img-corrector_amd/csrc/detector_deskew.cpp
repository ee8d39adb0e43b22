// detector_deskew.cpp -- the Hough and FFT legs of the reference's benchmark (core/src/main.rs:96-170: find the angle of
// transfer_rgb_image_to_gray_image(original), rotate_mat the ORIGINAL by it, im_write) for batches:
//
//   device   omr_hough_deskew_batch_device / omr_fft_deskew_batch_device (their entry points stand with their detectors in
//            oics_hough.cpp / oics_fft.cpp): the batch gray kernel (stages.hip) into scratch for colour scans, the batch
//            detector as it is, omr_rotate_batch_device_ex on the originals by the angles it found.
//   host     omr_deskew_with_hough_batch / omr_deskew_with_fft_batch: host images of any mix of shapes, bucketed by shape,
//            32 scans of a shape a run.
//   streams  omr_deskew_with_hough_batch_streams / omr_deskew_with_fft_batch_streams: file contents in through the imread
//            layer (oics_imread.cpp), file contents out through the device encoders; only streams cross the link.
//
// Scan i's angle has the per-call detector's f64 bits for omr_rgb_to_gray of the scan; its canvas is omr_rotate_device_ex's
// for that angle, byte for byte.  No kernel of its own.
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "detector_deskew.hpp"
#include "encode_any.hpp"
#include "engine.hpp"
#include "flow_frame.hpp"
#include "host_threads.hpp"
#include "jpeg_dec.hpp"
#include "orient.hpp"
#include "png_dec.hpp"
#include "stream_sink.hpp"

using namespace omr;

namespace {

// the flow on checked arguments.  skip (may be null): scans that are neither detected on nor rotated (their angle 0.0,
// their code left to the caller).  rc is never null here.  max_rows x max_cols: detector_canvas's answer; d_out may be
// null: the angles alone.  Synchronises `s`.
int deskew_run(const Detector &d, const uint8_t *d_scans, int n, int64_t stride, int rows, int cols, int cn, int64_t step,
               int flags, int border_mode, const uint8_t *border_value, int clip, int max_rows, int max_cols, uint8_t *d_out,
               int64_t out_stride, int64_t out_step, int32_t *out_size, double *angles, int32_t *rc, int32_t *n_lines,
               const int32_t *skip, hipStream_t s)
{
    PoolScope scope(s);
    DevBuf gray;
    DrainOnExit drain{s};  // the scratch goes back on return, error returns included: nothing queued may still read it
    const uint8_t *det = d_scans;
    int64_t det_stride = stride, det_step = step;
    if (cn == 3) {  // transfer_rgb_image_to_gray_image of every scan, one launch
        const int64_t img = (int64_t)rows * cols;
        OMR_HIP(gray.alloc((size_t)n * (size_t)img));
        OMR_HIP(launch_rgb2gray_batch(d_scans, stride, step, rows, cols, 3, n, gray.as<uint8_t>(), img, cols, s));
        det = gray.as<uint8_t>(), det_stride = img, det_step = cols;
    }
    int err;
    if (d.fft) {
        err = omr_fft_angles_batch_device(det, n, det_stride, rows, cols, det_step, d.canny_1, d.canny_2, d.min_line_length,
                                          d.max_line_gap, angles, n_lines, nullptr, 0, 0, s);
        for (int i = 0; !err && i < n; i++) rc[i] = OMR_OK;  // no segment: angle 0.0, and a success (fft.rs:197-247)
    } else {
        err = omr_hough_angles_batch_device(det, n, det_stride, rows, cols, 1, det_step, d.min_line_length, d.max_line_gap, angles, rc,
                                            n_lines, nullptr, 0, 0, s);
    }
    if (err) return err;
    for (int i = 0; skip && i < n; i++)
        if (skip[i]) angles[i] = 0.0;
    if (!d_out) return OMR_OK;
    // rotate_mat of the ORIGINAL scans, run by run of the scans that have an angle: the slot of one without is not written
    for (int i0 = 0; i0 < n;) {
        if (rc[i0] != OMR_OK || (skip && skip[i0])) {
            out_size[2 * i0] = out_size[2 * i0 + 1] = 0;
            i0++;
            continue;
        }
        int i1 = i0 + 1;
        while (i1 < n && rc[i1] == OMR_OK && !(skip && skip[i1])) i1++;
        if ((err = omr_rotate_batch_device_ex(d_scans + (int64_t)i0 * stride, i1 - i0, stride, step, rows, cols, cn, angles + i0, 1.0, flags,
                                              border_mode, border_value, clip, d_out + (int64_t)i0 * out_stride, out_stride, out_step,
                                              max_rows, max_cols, out_size + 2 * i0, s)))
            return err;
        i0 = i1;
    }
    OMR_HIP(hipStreamSynchronize(s));  // (runs of up to 3 scans only enqueue)
    return OMR_OK;
}

// what the host and streams forms share of the call's rules: the rotate's flags, border mode and clip
int check_rotate_args(int flags, int border_mode, int clip)
{
    WarpMode m;
    int rc = rotate_ex_args(flags, border_mode, &m);
    if (rc) return rc;
    if (clip != OMR_CLIP_DEFAULT && clip != OMR_CLIP_CONTAIN) return fail(OMR_ERR_BADARG, "unknown clip strategy %d", clip);
    return OMR_OK;
}

// a host image these flows take: omr_get_angle_with_hough's rules for the pointer, shape and pitch, 1 or 3 channels, and a
// canvas slot that exists
int check_scan(const omr_image &im, int clip)
{
    int rc = check_image(&im, cn_projection_batch);
    if (rc) return rc;
    int mr, mc;
    return detector_canvas(im.rows, im.cols, clip, &mr, &mc);
}

// ---- the batch forms: the frame's walk (flow_frame.hpp) with this flow's few answers -------------------------------------
struct Rotate {
    int flags, border_mode;
    const uint8_t *border;
    int clip;
};

Flow detector_flow(const Detector &d, const Rotate &a)
{
    Flow f;
    f.accept = [a](const omr_image &im) { return check_scan(im, a.clip); };
    f.canvas = [a](int rows, int cols, int *R, int *C) { return detector_canvas(rows, cols, a.clip, R, C); };
    f.open = [a](int rows, int cols, int cn, bool canvases, FlowBucket *b) -> int {
        int mr = 0, mc = 0;
        if (canvases)
            if (int rc = detector_canvas(rows, cols, a.clip, &mr, &mc)) return rc;
        b->chunk = canvases ? kDeskewChunk : kDetectorAnglesChunk;
        b->canvas_rows = mr, b->canvas_cols = mc, b->out_step = ((int64_t)mc * cn + 3) & ~(int64_t)3;
        return OMR_OK;
    };
    f.run = [d, a](const FlowBucket &b, const FlowSlots &s, double *ang, int32_t *, int32_t *codes, int32_t *size) -> int {
        // damaged image data: the slot's content means nothing.  Cleared, so that the detector finds a blank scan there
        // whatever the slot held; its angle and canvas are not made
        for (int j = 0; s.zrc && j < s.z; j++)
            if (s.zrc[j]) OMR_HIP(hipMemsetAsync(s.din + (size_t)j * s.in_stride, 255, (size_t)s.in_stride, s.s));
        // BORDER_TRANSPARENT starts from zero-filled canvases, as omr_rotate_ex does
        if (s.dout && a.border_mode == OMR_BORDER_TRANSPARENT) OMR_HIP(hipMemsetAsync(s.dout, 0, (size_t)s.z * s.out_stride, s.s));
        return deskew_run(d, s.din, s.z, s.in_stride, s.rows, s.cols, s.cn, s.row, a.flags, a.border_mode, a.border, a.clip, b.canvas_rows,
                          b.canvas_cols, s.dout, s.out_stride, s.out_step, size, ang, codes, nullptr, s.zrc, s.s);
    };
    return f;
}

// both host forms
int host_form(const Detector &d, const omr_image *srcs, int n, int flags, int border_mode, const uint8_t *border, int clip,
              double *angles, int32_t *rc_out, omr_image_owned *rotated)
{
    clear_error();
    if (!srcs || n < 1 || !border || !angles || !rotated || (!d.fft && !rc_out)) return fail(OMR_ERR_BADARG, "bad batch arguments");
    int rc = check_rotate_args(flags, border_mode, clip);
    if (rc) return rc;
    FlowSink sink;
    sink.kind = FlowSink::CANVASES;
    FlowOut to;
    to.angle = angles, to.code = rc_out, to.rotated = rotated;
    return flow_host_call(detector_flow(d, Rotate{flags, border_mode, border, clip}), sink, srcs, n, to);
}

// file contents in, file contents out (out null, with out_len: the angles alone)
int streams_form(const Detector &d, const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels, int32_t flags,
                 int32_t border_mode, const uint8_t *border, int32_t clip, int32_t format, int32_t level, double *angles,
                 int32_t *scan_rc, uint8_t **out, int64_t *out_len, int32_t rows_per_strip = 0, int32_t dpi = 0, int32_t predictor = 1)
{
    clear_error();
    if (!streams || !len || n < 1 || !angles || !scan_rc) return fail(OMR_ERR_BADARG, "bad batch arguments");
    if (!out != !out_len) return fail(OMR_ERR_BADARG, "the streams and their lengths are returned together, or neither");
    if (out && !border) return fail(OMR_ERR_BADARG, "null border_value");
    if (channels != 1 && channels != 3) return fail(OMR_ERR_BADARG, "channels must be 1 or 3, got %d", channels);
    if (format != OUT_JPEG && format != OUT_PNG && format != OUT_TIFF && format != OUT_TIFF8) return fail(OMR_ERR_BADARG, "format %d (0 = JPEG, 1 = PNG)", format);
    const OutFormat fmt{(OutKind)format, level, predictor, rows_per_strip, dpi};
    if (int r = fmt.check_params(channels)) return r;
    if (int r = flow_check_streams(streams, len, n)) return r;
    int rc = check_rotate_args(flags, border_mode, clip);
    if (rc) return rc;
    FlowSink sink;
    if (out) sink.kind = FlowSink::STREAMS, sink.fmt = fmt;
    FlowOut to;
    to.angle = angles, to.code = scan_rc, to.out = out, to.out_len = out_len;
    // a sheet its decoder refuses, or whose canvas slot leaves the image limit, keeps its code (imread turns a JPEG by its
    // EXIF orientation: the scan's shape is the turned one)
    const bool canvases = out != nullptr;
    const auto parse = [channels, clip, canvases](ImreadRun &run, const uint8_t *stream, int64_t l) {
        ImreadParsed ps = run.append(stream, l, channels, false);
        int mr, mc;
        if (!ps.rc) ps.rc = canvases ? detector_canvas(ps.rows, ps.cols, clip, &mr, &mc) : check_image_shape(ps.rows, ps.cols);
        return ps;
    };
    return flow_streams_call(detector_flow(d, Rotate{flags, border_mode, border, clip}), sink, streams, len, n, channels, parse, to);
}

// a caller's format: anything but JPEG and PNG becomes a value streams_form refuses, the private one included
int public_format(int format) { return format == OUT_TIFF || format == OUT_TIFF8 ? OUT_TIFF - 1 : format; }

Detector hough_detector(double min_line_length, double max_line_gap)
{
    Detector d;
    d.min_line_length = min_line_length, d.max_line_gap = max_line_gap;
    return d;
}

Detector fft_detector(double canny_1, double canny_2, double min_line_length, double max_line_gap)
{
    Detector d;
    d.fft = true, d.canny_1 = canny_1, d.canny_2 = canny_2, d.min_line_length = min_line_length, d.max_line_gap = max_line_gap;
    return d;
}

}  // namespace

int omr::detector_canvas(int rows, int cols, int clip, int *max_rows, int *max_cols)
{
    int rc = check_image_shape(rows, cols);
    if (rc) return rc;
    if (clip == OMR_CLIP_DEFAULT) {
        *max_rows = rows, *max_cols = cols;
        return OMR_OK;
    }
    if (clip != OMR_CLIP_CONTAIN) return fail(OMR_ERR_BADARG, "unknown clip strategy %d", clip);
    // transfer.rs:487-498: width = ceil(rows |sin| + cols |cos|), height = ceil(cols |sin| + rows |cos|).  Either is at
    // most the diagonal; sin and cos of one rounded argument, two products and a sum can lift the computed value above it
    // by a few units in the last place, which matters where the diagonal is a whole number: 16 of them are allowed for
    const double diag = ceil(hypot((double)rows, (double)cols) * (1.0 + 16.0 * DBL_EPSILON));
    if (diag >= 32767.0) return fail(OMR_ERR_ASSERT, "a canvas of %d x %d could reach %.0f a side (32767 or more)", cols, rows, diag);
    *max_rows = *max_cols = (int)diag;
    return OMR_OK;
}

int omr::detector_deskew_device(const Detector &d, const uint8_t *d_scans, int n, int64_t stride, int rows, int cols, int cn,
                                int64_t step, int flags, int border_mode, const uint8_t *border_value, int clip, uint8_t *d_out,
                                int64_t out_stride, int64_t out_step, int32_t *out_size, double *angles, int32_t *rc_out,
                                int32_t *n_lines, hipStream_t s)
{
    clear_error();
    // the detector's rules, then the batch rotate's: all of them before any device work
    if (!d_scans || !d_out || !border_value || !out_size || !angles || (!d.fft && !rc_out)) return fail(OMR_ERR_BADARG, "null pointer");
    if (n <= 0) return fail(OMR_ERR_BADARG, "empty batch");
    int rc = check_image_shape(rows, cols);
    if (rc || (rc = cn_projection_batch(cn))) return rc;
    if (step < (int64_t)cols * cn) return fail(OMR_ERR_BADARG, "step_bytes too small");
    if (stride < 0) return fail(OMR_ERR_BADARG, "negative scan stride");
    if ((rc = check_rotate_args(flags, border_mode, clip))) return rc;
    int mr = 0, mc = 0;
    if ((rc = detector_canvas(rows, cols, clip, &mr, &mc))) return rc;
    // (by division: rows x pitch of an absurd pitch would leave 64 bits)
    if (out_step < (int64_t)mc * cn || out_stride / mr < out_step)
        return fail(OMR_ERR_BADARG, "every output slot must hold %d x %d x %d channels (omr_detector_deskew_canvas)", mr, mc, cn);
    // [first byte, last byte) of everything the call may read and may write
    const uintptr_t s0 = (uintptr_t)d_scans, s1 = s0 + (uint64_t)(n - 1) * stride + (uint64_t)(rows - 1) * step + (uint64_t)cols * cn;
    const uintptr_t t0 = (uintptr_t)d_out, t1 = t0 + (uint64_t)(n - 1) * out_stride + (uint64_t)(mr - 1) * out_step + (uint64_t)mc * cn;
    if (s0 < t1 && t0 < s1) return fail(OMR_ERR_BADARG, "source and destination overlap");
    if ((rc = have_device())) return rc;
    std::vector<int32_t> codes;
    if (!rc_out) codes.assign((size_t)n, OMR_OK), rc_out = codes.data();
    return deskew_run(d, d_scans, n, stride, rows, cols, cn, step, flags, border_mode, border_value, clip, mr, mc, d_out, out_stride,
                      out_step, out_size, angles, rc_out, n_lines, nullptr, s);
}

extern "C" {

int omr_detector_deskew_canvas(int32_t rows, int32_t cols, int32_t clip, int32_t *max_rows, int32_t *max_cols)
{
    clear_error();
    if (!max_rows || !max_cols) return fail(OMR_ERR_BADARG, "null output");
    int mr = 0, mc = 0;
    int rc = detector_canvas(rows, cols, clip, &mr, &mc);
    if (rc) return rc;
    *max_rows = mr, *max_cols = mc;
    return OMR_OK;
}

int omr_deskew_with_hough_batch(const omr_image *srcs, int32_t n, double min_line_length, double max_line_gap, int32_t flags,
                                int32_t border_mode, const uint8_t border_value[4], int32_t clip, double *angles, int32_t *rc,
                                omr_image_owned *rotated)
{
    return host_form(hough_detector(min_line_length, max_line_gap), srcs, n, flags, border_mode, border_value, clip, angles, rc, rotated);
}

int omr_deskew_with_fft_batch(const omr_image *srcs, int32_t n, double canny_threshold_1, double canny_threshold_2,
                              double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                              const uint8_t border_value[4], int32_t clip, double *angles, int32_t *rc, omr_image_owned *rotated)
{
    return host_form(fft_detector(canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), srcs, n, flags, border_mode,
                     border_value, clip, angles, rc, rotated);
}

int omr_deskew_with_hough_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                        double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                                        const uint8_t border_value[4], int32_t clip, int32_t format,
                                        int32_t quality_or_compression, double *angles, int32_t *scan_rc, uint8_t **out,
                                        int64_t *out_len)
{
    return streams_form(hough_detector(min_line_length, max_line_gap), streams, len, n, channels, flags, border_mode, border_value, clip,
                        public_format(format), quality_or_compression, angles, scan_rc, out, out_len);
}

int omr_deskew_with_fft_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                      double canny_threshold_1, double canny_threshold_2, double min_line_length,
                                      double max_line_gap, int32_t flags, int32_t border_mode, const uint8_t border_value[4],
                                      int32_t clip, int32_t format, int32_t quality_or_compression, double *angles,
                                      int32_t *scan_rc, uint8_t **out, int64_t *out_len)
{
    return streams_form(fft_detector(canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), streams, len, n, channels,
                        flags, border_mode, border_value, clip, public_format(format), quality_or_compression, angles, scan_rc, out, out_len);
}

int omr_deskew_with_hough_batch_streams_tiff(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                             double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                                             const uint8_t border_value[4], int32_t clip, int32_t threshold,
                                             int32_t rows_per_strip, int32_t dpi, double *angles, int32_t *scan_rc,
                                             uint8_t **out, int64_t *out_len)
{
    return streams_form(hough_detector(min_line_length, max_line_gap), streams, len, n, channels, flags, border_mode, border_value, clip,
                        OUT_TIFF, threshold, angles, scan_rc, out, out_len, rows_per_strip, dpi);
}

int omr_deskew_with_fft_batch_streams_tiff(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                           double canny_threshold_1, double canny_threshold_2, double min_line_length,
                                           double max_line_gap, int32_t flags, int32_t border_mode,
                                           const uint8_t border_value[4], int32_t clip, int32_t threshold,
                                           int32_t rows_per_strip, int32_t dpi, double *angles, int32_t *scan_rc,
                                           uint8_t **out, int64_t *out_len)
{
    return streams_form(fft_detector(canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), streams, len, n, channels,
                        flags, border_mode, border_value, clip, OUT_TIFF, threshold, angles, scan_rc, out, out_len, rows_per_strip, dpi);
}

int omr_deskew_with_hough_batch_streams_tiff8(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                              double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                                              const uint8_t border_value[4], int32_t clip, int32_t compression,
                                              int32_t predictor, int32_t rows_per_strip, int32_t dpi, double *angles,
                                              int32_t *scan_rc, uint8_t **out, int64_t *out_len)
{
    return streams_form(hough_detector(min_line_length, max_line_gap), streams, len, n, channels, flags, border_mode, border_value, clip,
                        OUT_TIFF8, compression, angles, scan_rc, out, out_len, rows_per_strip, dpi, predictor);
}

int omr_deskew_with_fft_batch_streams_tiff8(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                            double canny_threshold_1, double canny_threshold_2, double min_line_length,
                                            double max_line_gap, int32_t flags, int32_t border_mode,
                                            const uint8_t border_value[4], int32_t clip, int32_t compression,
                                            int32_t predictor, int32_t rows_per_strip, int32_t dpi, double *angles,
                                            int32_t *scan_rc, uint8_t **out, int64_t *out_len)
{
    return streams_form(fft_detector(canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), streams, len, n, channels,
                        flags, border_mode, border_value, clip, OUT_TIFF8, compression, angles, scan_rc, out, out_len, rows_per_strip, dpi,
                        predictor);
}

}  // extern "C"
