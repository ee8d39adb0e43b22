// encode_any.hpp -- the output format of a files-to-files flow (correct_batch.cpp, projection_batch.cpp, detector_deskew.cpp)
// as one object: which of the four encoders writes the canvases, with its parameters, and the four things a flow asks of
// it.  A fifth format is a fifth case in each switch below and an entry point; the flows themselves do not change.
#pragma once
#include "../../include/omrdeskew.h"
#include "jpeg.hpp"
#include "png_enc.hpp"
#include "tiff_enc.hpp"
#include "tiff_enc8.hpp"

#pragma GCC visibility push(hidden)  // the library's own: not in the dynamic symbol table
namespace omr {

// JPEG and PNG are the public `format` values of the detector flows' entry points; the TIFF kinds have values that only
// the _tiff and _tiff8 entry points pass (a public argument of either value is refused, detector_deskew.cpp)
enum OutKind { OUT_JPEG = 0, OUT_PNG = 1, OUT_TIFF = -26, OUT_TIFF8 = -29 };

struct OutFormat {
    OutKind kind;
    int level;           // JPEG: quality; PNG: compression level; TIFF: threshold; 8-bit TIFF: Compression
    int predictor = 1;       // the 8-bit TIFF form's
    int rows_per_strip = 0;  // the TIFF forms'
    int dpi = 0;

    // the parameters alone, for cn channels: what the TIFF writers refuse (the others clamp theirs)
    int check_params(int cn) const
    {
        switch (kind) {
        case OUT_TIFF: return tenc_check_params(cn, level, rows_per_strip, dpi);
        case OUT_TIFF8: return tenc8_check_params(cn, level, predictor, rows_per_strip, dpi);
        default: return OMR_OK;
        }
    }
    // a canvas slot the encoder's 32-bit offsets cannot take: host arithmetic, before any device work
    int check_canvas(int rows, int cols, int cn) const
    {
        switch (kind) {
        case OUT_TIFF8: return tenc8_check_shape(rows, cols, cn, level, rows_per_strip, nullptr);
        case OUT_TIFF: return tenc_check_shape(rows, cols, rows_per_strip, nullptr);
        case OUT_PNG: return penc_check_shape(rows, cols, cn);
        default: return jpeg_check_scan_bits(rows, cols, cn);
        }
    }
    // the public bound of one image's stream
    int bound(int rows, int cols, int cn, int64_t *bytes) const
    {
        switch (kind) {
        case OUT_TIFF8: return omr_tiff8_bound(rows, cols, cn, level, rows_per_strip, bytes);
        case OUT_TIFF: return omr_tiff_bound(rows, cols, rows_per_strip, bytes);
        case OUT_PNG: return omr_png_bound(rows, cols, cn, bytes);
        default: return omr_jpeg_bound(rows, cols, cn, bytes);
        }
    }
    // n canvases on the device -> their streams into `sink` (the encoders' *_encode_device)
    int encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n, JpegSink &sink,
                      hipStream_t s) const
    {
        switch (kind) {
        case OUT_TIFF8: return tiff8_encode_device(d_imgs, img_stride, step, cn, sizes, n, level, predictor, rows_per_strip, dpi, sink, s);
        case OUT_TIFF: return tiff_encode_device(d_imgs, img_stride, step, cn, sizes, n, level, rows_per_strip, dpi, sink, s);
        case OUT_PNG: return png_encode_device(d_imgs, img_stride, step, cn, sizes, n, level, sink, s);
        default: return jpeg_encode_device(d_imgs, img_stride, step, cn, sizes, n, level, sink, s);
        }
    }
    // one host canvas -> its stream in out[0 .. cap) (the public omr_*_encode)
    int encode_host(const omr_image *canvas, uint8_t *out, int64_t cap, int64_t *len) const
    {
        switch (kind) {
        case OUT_TIFF8: return omr_tiff8_encode(canvas, level, predictor, rows_per_strip, dpi, out, cap, len);
        case OUT_TIFF: return omr_tiff_encode(canvas, level, rows_per_strip, dpi, out, cap, len);
        case OUT_PNG: return omr_png_encode(canvas, level, out, cap, len);
        default: return omr_jpeg_encode(canvas, level, out, cap, len);
        }
    }
};

}  // namespace omr
#pragma GCC visibility pop
