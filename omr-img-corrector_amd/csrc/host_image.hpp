// host_image.hpp -- image and argument logic of the entry points that needs no device: the shape and channel checks of a
// host image, shrink_to's scale, OpenCV's resize() dispatch and the bucketing of a batch by shape.  Pure functions, no
// HIP call; every entry point that states one of these rules states it through this header.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/omrdeskew.h"

namespace omr {

int fail(int code, const char *fmt, ...);  // engine.cpp

inline int check_image_shape(int rows, int cols)
{
    if (rows <= 0 || cols <= 0) return fail(OMR_ERR_ASSERT, "empty image");
    if (rows >= 32767 || cols >= 32767) return fail(OMR_ERR_ASSERT, "image dimension >= SHRT_MAX");
    return OMR_OK;
}

// ---- channel rules: what an entry point accepts, and the code it answers the rest with
inline int cn_any(int cn)  // 1..4
{
    if (cn < 1 || cn > 4) return fail(OMR_ERR_ASSERT, "unsupported channel count %d", cn);
    return OMR_OK;
}
inline int cn_one(int cn)
{
    if (int rc = cn_any(cn)) return rc;
    if (cn != 1) return fail(OMR_ERR_ASSERT, "expected a 1-channel image, got %d", cn);
    return OMR_OK;
}
inline int cn_canny(int cn)  // Canny on gray, or on cvtColor's gray of 3 / 4 channels
{
    if (cn != 1 && cn != 3 && cn != 4) return fail(OMR_ERR_ASSERT, "Canny / HoughLinesP take 1, 3 or 4 channels, got %d", cn);
    return OMR_OK;
}
inline int cn_gray_source(int cn)  // 1..4 without 2: what RGB2GRAY (or its 1-channel copy) takes
{
    if (int rc = cn_any(cn)) return rc;
    if (cn == 2) return fail(OMR_ERR_ASSERT, "RGB2GRAY needs 3 or 4 channels");
    return OMR_OK;
}
inline int cn_projection_batch(int cn)  // the batch contexts take 1 or 3; 4 is valid for the per-call function
{
    if (cn == 4) return fail(OMR_ERR_NOTIMPL, "4-channel batches are not implemented (1 or 3 channels)");
    if (cn != 1 && cn != 3) return fail(OMR_ERR_ASSERT, "RGB2GRAY needs 3 or 4 channels, got %d", cn);
    return OMR_OK;
}
inline int cn_correct_batch(int cn)
{
    if (cn == 4) return fail(OMR_ERR_NOTIMPL, "4-channel batches are not implemented (1 or 3 channels)");
    if (cn == 2) return fail(OMR_ERR_ASSERT, "RGB2GRAY needs 3 or 4 channels");
    return cn_canny(cn);
}

// a host image an entry point may read: pointer, shape, the caller's channel rule, row pitch -- in this order
inline int check_image(const omr_image *im, int (*channel_rule)(int))
{
    if (!im || !im->data) return fail(OMR_ERR_BADARG, "null image");
    int rc = check_image_shape(im->rows, im->cols);
    if (rc || (rc = channel_rule(im->channels))) return rc;
    if (im->step_bytes < (int64_t)im->cols * im->channels) return fail(OMR_ERR_BADARG, "step_bytes too small");
    return OMR_OK;
}

// the scale that fits cols x rows into max_w x max_h, a bound <= 0 meaning none (transfer.rs:105-114, omr.rs:60-82);
// may exceed 1
inline double shrink_scale(int cols, int rows, int max_w, int max_h)
{
    const double ws = max_w <= 0 ? 1.0 : (double)max_w / (double)cols;
    const double hs = max_h <= 0 ? 1.0 : (double)max_h / (double)rows;
    return ws < hs ? ws : hs;
}

// OpenCV 4.6.0 resize() (resize.cpp) for INTER_AREA and INTER_LINEAR -- which code path a resize takes:
//   same size                         -> COPY
//   INTER_AREA, both axes shrink      -> AREA_INT (resizeAreaFast_, integer factors kx, ky) / AREA_GENERAL (resizeArea_)
//   INTER_AREA, an axis enlarges      -> LINEAR with area-mode coefficients (quirk B7)
//   INTER_LINEAR                      -> LINEAR (an exact 2x shrink is re-routed to INTER_AREA)
struct ResizeDispatch {
    enum Kind { COPY, LINEAR, AREA_INT, AREA_GENERAL } kind;
    bool area_mode;  // LINEAR
    int kx, ky;      // AREA_INT
};
inline ResizeDispatch resize_dispatch(int srows, int scols, int drows, int dcols, int interp)
{
    if (drows == srows && dcols == scols) return {ResizeDispatch::COPY, false, 1, 1};
    const double inv_scale_x = (double)dcols / scols, inv_scale_y = (double)drows / srows;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    const int iscale_x = (int)lrint(scale_x), iscale_y = (int)lrint(scale_y);
    const bool is_area_fast = fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON;
    if (interp == OMR_INTER_LINEAR && is_area_fast && iscale_x == 2 && iscale_y == 2) interp = OMR_INTER_AREA;
    if (!(interp == OMR_INTER_AREA && scale_x >= 1 && scale_y >= 1)) return {ResizeDispatch::LINEAR, interp == OMR_INTER_AREA, 0, 0};
    if (is_area_fast) return {ResizeDispatch::AREA_INT, false, iscale_x, iscale_y};
    return {ResizeDispatch::AREA_GENERAL, false, 0, 0};
}

// The reference corrects one file per call, any size, so a batch may mix shapes: its images grouped by
// (rows, cols, channels), the groups in order of first appearance, members[k] the positions of group k's images.
struct ImageShape {
    int rows, cols, cn;
    bool operator==(const ImageShape &o) const { return rows == o.rows && cols == o.cols && cn == o.cn; }
};
struct ShapeBuckets {
    std::vector<ImageShape> shapes;
    std::vector<std::vector<int>> members;
};
// check(srcs[i]) runs on image i before image i is bucketed: the first bad image of a batch decides the call's error
template <class Check>
int bucket_by_shape(const omr_image *srcs, int n, Check check, ShapeBuckets *out)
{
    for (int i = 0; i < n; i++) {
        if (int rc = check(srcs[i])) return rc;
        const ImageShape sh{srcs[i].rows, srcs[i].cols, srcs[i].channels};
        size_t k = 0;
        while (k < out->shapes.size() && !(out->shapes[k] == sh)) k++;
        if (k == out->shapes.size()) {
            out->shapes.push_back(sh);
            out->members.emplace_back();
        }
        out->members[k].push_back(i);
    }
    return OMR_OK;
}

}  // namespace omr
