// hough_select.hpp -- the detectors' rules on segment lists (x1, y1, x2, y2) as pure host functions: libm and the C ABI's
// constants, no HIP call or header, so that a host program can hold them to the float64 statements (tests/hough_exact.py).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/omrdeskew.h"

namespace omr {
namespace hh {

constexpr double kPi = 3.14159265358979323846;

// hough.rs:50-68 / omr.rs:257-267 on n segments: f32 angles with libm atan2f / fmodf (what Rust's f32::atan2 and % call)
inline void line_angles(const int32_t *l, size_t n, float *ang)
{
    const float pi32 = 3.14159274101257324f;  // std::f32::consts::PI
    for (size_t i = 0; i < n; i++) {
        const float x1 = (float)l[4 * i], y1 = (float)l[4 * i + 1], x2 = (float)l[4 * i + 2], y2 = (float)l[4 * i + 3];
        float angle = atan2f(y2 - y1, x2 - x1) * 180.0f / pi32;
        ang[i] = fmodf(angle, 45.0f);
    }
}

// omr.rs:268-301 on a scan's m angles and their counts: a strictly larger count restarts the candidates, an equal one
// appends (cand_len counts them all, candidates holds the first cand_cap).  No segment (the reference panics on
// angles[0], omr.rs:272 -- quirk B11): 0.0, no candidate, OMR_STATUS_NOT_A_RESULT; the caller decides what that means
inline void select_omr_rs(const float *ang, const int32_t *cnt, int m, double *angle, int32_t *status, double *candidates,
                          int32_t cand_cap, int32_t *cand_len)
{
    double target = m > 0 ? (double)ang[0] : 0.0;
    int best = 0, nc = 0;
    for (int i = 0; i < m; i++) {
        if (cnt[i] > best) {
            target = (double)ang[i];
            best = cnt[i];
            if (candidates && cand_cap > 0) candidates[0] = target;
            nc = 1;
        } else if (cnt[i] == best) {
            if (candidates && nc < cand_cap) candidates[nc] = (double)ang[i];
            nc++;
        }
    }
    *angle = target;
    if (cand_len) *cand_len = nc;
    if (status) *status = nc == 0 ? OMR_STATUS_NOT_A_RESULT : (nc == 1 ? OMR_STATUS_BELIEVED : OMR_STATUS_NEED_CHECK);
}

// fft.rs:197-247 on n segments: f64 angles (libm atan2) folded into [-45, 45]; the inner loop re-reads line i (quirk B10,
// fft.rs:231), so line i collects n - 1 votes iff its raw angle is within 0.1 of its folded angle, else none.  No
// segment, or no line with a vote: 0.0
inline void select_fft_rs(const int32_t *l, int n, double *angle_out)
{
    double average_angle = 0.0;
    int max_votes = 0;
    for (int i = 0; i < n; i++) {
        const double x1 = l[4 * i], y1 = l[4 * i + 1], x2 = l[4 * i + 2], y2 = l[4 * i + 3];
        const double raw = (atan2(y2 - y1, x2 - x1) * 180.0) / kPi;
        const double angle = raw < -45.0 ? raw + 90.0 : (raw > 45.0 ? raw - 90.0 : raw);
        int votes = 0;
        for (int j = 0; j < n; j++) {
            if (i == j) continue;
            if (fabs(raw - angle) < 0.1) votes++;
        }
        if (votes > max_votes) {
            max_votes = votes;
            average_angle = angle;
        }
        if (max_votes == n - 1 && n > 1) break;  // nothing can beat n - 1 with a strict '>'
    }
    *angle_out = average_angle;
}

}  // namespace hh
}  // namespace omr
