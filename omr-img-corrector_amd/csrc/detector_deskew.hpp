// detector_deskew.hpp -- the Hough and FFT legs of the reference's benchmark as batch flows (detector_deskew.cpp,
// DESIGN.md section 4.24): gray, detector, rotate_mat of the original scans.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace omr {

// which detector a flow runs, with the reference's arguments for it
struct Detector {
    bool fft = false;
    double canny_1 = 0, canny_2 = 0;  // get_angle_with_fft's Canny thresholds (unused by get_angle_with_hough)
    double min_line_length = 0, max_line_gap = 0;
};

// The slot every canvas of rotate_mat(rows x cols, any angle, clip) fits: rows x cols for DEFAULT, the worst case over all
// angles for CONTAIN.  Host arithmetic.  OMR_ERR_ASSERT for an empty or oversized image or a slot of 32767 or more a side,
// OMR_ERR_BADARG for an unknown clip.
int detector_canvas(int rows, int cols, int clip, int *max_rows, int *max_cols);

// The body of omr_hough_deskew_batch_device / omr_fft_deskew_batch_device with every argument rule in front of it (rc may
// be null for the FFT detector only).  Synchronises `s`.
int detector_deskew_device(const Detector &d, const uint8_t *d_scans, int n, int64_t stride, int rows, int cols, int cn,
                           int64_t step, int flags, int border_mode, const uint8_t *border_value, int clip, uint8_t *d_out,
                           int64_t out_stride, int64_t out_step, int32_t *out_size, double *angles, int32_t *rc, int32_t *n_lines,
                           hipStream_t s);

}  // namespace omr
