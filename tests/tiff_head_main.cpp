// tiff_head_main.cpp -- tests/test_tiff_head.py compiles this host program around csrc/tiff_head.hpp.  Every line of
// standard input describes one head:
//   rows cols rps ns bits samples compression photometric predictor t6_options dpi
// and is answered with one line: head_len off_pos cnt_pos data_at and the head's bytes as hex.
#include <stdio.h>

#include <vector>

#include "tiff_head.hpp"

int main()
{
    int rows, cols, rps, ns, bits, samples, compression, photometric, predictor, t6, dpi;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &rows, &cols, &rps, &ns, &bits, &samples, &compression, &photometric, &predictor, &t6,
                 &dpi) == 11) {
        // exactly the head's bytes as tiff_head_len promises them, on the heap: a write behind them is the sanitizer's to find
        std::vector<uint8_t> h((size_t)omr::tiff_head_len(dpi > 0, samples == 3, t6 != 0, predictor == 2), 0xAA);
        const omr::TiffHeadDesc d{rows, cols, rps, ns, bits, samples, compression, photometric, predictor, t6 != 0, dpi};
        const omr::TiffHead r = omr::tiff_head(d, h.data());
        if (r.head_len != (int)h.size()) return 2;
        printf("%d %d %d %d ", r.head_len, r.off_pos, r.cnt_pos, r.data_at);
        for (int i = 0; i < r.head_len; i++) printf("%02x", h[(size_t)i]);
        printf("\n");
    }
    return 0;
}
