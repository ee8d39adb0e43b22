// hough_select_main.cpp -- tests/test_hough_select.py compiles this host program around csrc/hough_select.hpp, the
// detectors' pure host rules.  Standard input holds blocks of integers:
//   n cap_small cap_large, then n segments x1 y1 x2 y2, then n counts
// and every block is answered with four lines:
//   A  the n line_angles as f32 bit patterns (hex)
//   S  cap_small, then select_omr_rs's angle (f64 bits), status, cand_len and the candidates written (f64 bits)
//   S  the same for cap_large
//   F  select_fft_rs's angle (f64 bits)
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hough_select.hpp"

static unsigned long long bits64(double v)
{
    unsigned long long b;
    memcpy(&b, &v, sizeof b);
    return b;
}

int main()
{
    int n, caps[2];
    while (scanf("%d %d %d", &n, &caps[0], &caps[1]) == 3) {
        if (n < 0 || caps[0] < 0 || caps[1] < 0) return 2;
        // exactly n entries each, on the heap: a read or write behind them is the sanitizer's to find
        std::vector<int32_t> l((size_t)n * 4), cnt((size_t)n);
        std::vector<float> ang((size_t)n);
        for (auto &v : l)
            if (scanf("%d", &v) != 1) return 2;
        for (auto &v : cnt)
            if (scanf("%d", &v) != 1) return 2;
        omr::hh::line_angles(l.data(), (size_t)n, ang.data());
        printf("A");
        for (float a : ang) {
            unsigned b;
            memcpy(&b, &a, sizeof b);
            printf(" %08x", b);
        }
        printf("\n");
        for (int cap : caps) {
            std::vector<double> cand((size_t)cap);
            double angle = -1.0;
            int32_t status = -1, len = -1;
            omr::hh::select_omr_rs(ang.data(), cnt.data(), n, &angle, &status, cand.data(), cap, &len);
            printf("S %d %016llx %d %d", cap, bits64(angle), status, len);
            for (int k = 0; k < std::min(cap, len); k++) printf(" %016llx", bits64(cand[(size_t)k]));
            printf("\n");
        }
        double fft = -1.0;
        omr::hh::select_fft_rs(l.data(), n, &fft);
        printf("F %016llx\n", bits64(fft));
    }
    return 0;
}
