// oics_tiff_enc.cpp -- host side of the Group 4 TIFF encoder (tiff_enc.hip): the bound of a file's
// length, the parameters and shapes it refuses, a group's layout and launches, and the cost that closes a group.  The
// file's head is tiff_head.hpp's from this writer's description; the entry points omr_tiff_encode* are the shared frame's
// (codec_host.hpp, section 4.28) with these handed in.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "tiff_dec.hpp"  // tdec_code_tables: the one set of T.4 codes
#include "tiff_enc.hpp"

using namespace omr;

namespace {

// bytes of row code segments in one group of launches (the largest part of the workspace)
constexpr int64_t kGroupCode = (int64_t)1 << 30;
constexpr int kGroupImages = 4096;

int pack_w_of(int cols) { return (cols + 31) / 32 + 1; }
int seg_w_of(int cols) { return (int)((tenc_row_bits(cols) + 31) / 32) + 1; }
int64_t strip_bytes_max(int rows_of_strip, int cols) { return ((int64_t)rows_of_strip * tenc_row_bits(cols) + TENC_EOFB_BITS + 7) / 8; }
// halvings that empty a range of v
int halvings(int v)
{
    int k = 1;
    while (((int64_t)1 << k) < v) k++;
    return k + 1;
}

// one group: images [i0, i0 + g)
int encode_group(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int i0, int g, int threshold,
                 int rows_per_strip, int dpi, JpegSink &sink, hipStream_t s)
{
    std::vector<TencImg> im((size_t)g);
    std::vector<TencDyn> dyn((size_t)g);
    GroupStreams out(sink, i0, g);
    DrainOnExit drain{s};  // behind the host objects that asynchronous copies read or write, before the device buffers
    StageTimer<TENC_STAGES> ev;
    if (int r = ev.begin(tenc_stats().on)) return r;
    int64_t pack_words = 0, code_words = 0, rows_all = 0, strips_all = 0, max_pack_bytes = 0;
    int max_rows = 0, max_cols = 0, max_strips = 0, max_rps = 0;
    for (int j = 0; j < g; j++) {
        TencImg &m = im[(size_t)j];
        memset(&m, 0, sizeof m);
        const int r = sizes[2 * (size_t)(i0 + j)], c = sizes[2 * (size_t)(i0 + j) + 1];
        m.src_off = (int64_t)(i0 + j) * img_stride;
        m.pack_off = pack_words, m.code_off = code_words, m.row0 = rows_all, m.strip0 = strips_all;
        if (r <= 0) continue;
        m.rows = r, m.cols = c;
        m.rps = rows_per_strip > 0 ? std::min(rows_per_strip, r) : r;
        m.ns = strips_of(r, m.rps);
        m.pack_w = pack_w_of(c), m.seg_w = seg_w_of(c);
        tenc_set_head(m, TiffHeadDesc{r, c, m.rps, m.ns, 1, 1, 4, 0, 1, true, dpi});  // bilevel, Group 4, white is zero, T6Options
        pack_words += ((int64_t)r + 1) * m.pack_w, code_words += (int64_t)r * m.seg_w, rows_all += r, strips_all += m.ns;
        max_pack_bytes = std::max(max_pack_bytes, ((int64_t)r + 1) * m.pack_w * 4);
        max_rows = std::max(max_rows, r), max_cols = std::max(max_cols, c);
        max_strips = std::max(max_strips, m.ns), max_rps = std::max(max_rps, m.rps);
    }
    if (rows_all == 0) return out.all_empty();
    uint32_t codes[2 * TENC_CODES];
    for (int k = 0; k < 2; k++) {
        int32_t run[TENC_CODES], code[TENC_CODES], bits[TENC_CODES];
        tdec_code_tables(k, run, code, bits);
        for (int t = 0; t < TENC_CODES; t++) codes[k * TENC_CODES + t] = (uint32_t)code[t] | (uint32_t)bits[t] << 16;
    }
    DevBuf d_im, d_dyn, d_codes, pack, code, rlen, roff, sbytes, soff;
    OMR_HIP(d_im.alloc(sizeof(TencImg) * (size_t)g));
    OMR_HIP(d_dyn.alloc(sizeof(TencDyn) * (size_t)g));
    OMR_HIP(d_codes.alloc(sizeof codes));
    OMR_HIP(pack.alloc((size_t)pack_words * 4));
    OMR_HIP(code.alloc((size_t)code_words * 4));
    OMR_HIP(rlen.alloc((size_t)rows_all * 4));
    OMR_HIP(roff.alloc((size_t)rows_all * 4));
    OMR_HIP(sbytes.alloc((size_t)strips_all * 4));
    OMR_HIP(soff.alloc((size_t)strips_all * 4));
    TencPass p;
    memset(&p, 0, sizeof p);
    p.src = d_imgs, p.step = step, p.imgs = d_im.as<TencImg>(), p.dyn = d_dyn.as<TencDyn>(), p.n = g, p.cn = cn;
    p.lim = cn == 1 ? (uint32_t)threshold : ((uint32_t)threshold + 1) << 15;
    p.codes = d_codes.as<uint32_t>(), p.pack = pack.as<uint32_t>(), p.code = code.as<uint32_t>();
    p.len = rlen.as<uint32_t>(), p.off = roff.as<uint32_t>(), p.sbytes = sbytes.as<uint32_t>(), p.soff = soff.as<uint32_t>();
    p.span_steps = max_cols / 2560 + 1, p.row_steps = 2 * max_cols + 2;
    p.lg_rows = halvings(max_rps), p.lg_strips = halvings(max_strips);
    // 1. everything up to the strips' sizes; the host learns every file's length
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(TencImg) * (size_t)g, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemcpyAsync(d_codes.p, codes, sizeof codes, hipMemcpyHostToDevice, s));
    int rc = ev.mark(0, s);
    if (rc || (rc = tenc_launch_pack(p, max_pack_bytes, s)) || (rc = ev.mark(1, s)) || (rc = tenc_launch_rows(p, max_rows, s)) || (rc = ev.mark(2, s)) ||
        (rc = tenc_launch_place(p, max_strips, max_rps, s)) || (rc = ev.mark(3, s)))
        return rc;
    OMR_HIP(hipMemcpyAsync(dyn.data(), d_dyn.p, sizeof(TencDyn) * (size_t)g, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    int64_t max_data = 0;
    for (int j = 0; j < g; j++)
        if (im[(size_t)j].rows) {
            out.len[(size_t)j] = (int64_t)im[(size_t)j].data_at + dyn[(size_t)j].data_len;
            max_data = std::max<int64_t>(max_data, dyn[(size_t)j].data_len);
        }
    // 2. the files, where the caller wants them
    if ((rc = out.place(im, d_im, s, &p.out))) return rc;
    if ((rc = tenc_launch_merge(p, max_data, max_strips, s)) || (rc = ev.mark(4, s))) return rc;
    OMR_HIP(hipStreamSynchronize(s));
    if ((rc = ev.finish(tenc_stats()))) return rc;
    return out.done();
}

}  // namespace

// A row's code in bits at most: 7 x cols + 32.  Every step of Fax3Encode2DRow moves a0 forward by d pixels and writes
//   pass        4 bits, d >= 1 (b2 > b1 >= a0);
//   vertical    at most 7 bits, d >= 1 -- except as a row's first step, where a1 may be 0: 7 bits for d = 0, once;
//   horizontal  3 bits and the codes of a white run and a black run of r1 + r2 = d pixels.  A run of r >= 1 takes at most
//               6 r bits when white and 6 r - 3 when black (the tables: white 1 is 6 bits, black 1 is 3, no terminating
//               code is longer than 12, make-up and terminating code together at most 25 for 64 or more pixels, 12 more
//               for every further 2560; tests/test_tiff_encode_abi.py checks every length), so the step takes at most
//               6 d bits -- alternating pixels reach that.  A run of 0 (at most 10 bits) occurs only as the first run of a
//               row's first step (white, 8 bits: at most 6 d + 8) and as the second run of its last (at most 6 d + 13).
// So the steps take at most 7 bits a pixel and 7 + 8 + 13 bits besides, and a row has at most cols + 1 steps.
int64_t omr::tenc_row_bits(int cols) { return 7 * (int64_t)cols + 32; }

// The file: header, IFD and resolutions (TENC_HEAD_MAX at most), the two strip arrays (8 bytes a strip), and per strip its
// rows' codes, the EOFB's 24 bits, the padding to a byte and one more to an even offset.
int64_t omr::tenc_bound(int rows, int cols, int rps)
{
    const int full = rows / rps, rest = rows % rps;
    int64_t b = TENC_HEAD_MAX + 8 * (int64_t)strips_of(rows, rps);
    b += full * even_offset(strip_bytes_max(rps, cols));
    if (rest) b += even_offset(strip_bytes_max(rest, cols));
    return b;
}

int omr::tenc_check_shape(int rows, int cols, int rows_per_strip, int *rps_out)
{
    if (rows_per_strip < 0) return fail(OMR_ERR_BADARG, "rows_per_strip %d is negative", rows_per_strip);
    if (rows <= 0 || cols <= 0) return fail(OMR_ERR_ASSERT, "empty image");
    if (rows > TENC_MAX_SIDE || cols > TENC_MAX_SIDE || (int64_t)rows * cols > TENC_MAX_PIXELS)
        return fail(OMR_ERR_ASSERT, "%d x %d is above imread's limits (2^20 a side, 2^30 pixels): not supported", rows, cols);
    const int rps = rows_per_strip > 0 ? std::min(rows_per_strip, rows) : rows;
    if ((int64_t)rps * tenc_row_bits(cols) + TENC_EOFB_BITS + 7 > TENC_MAX_STRIP_BITS)
        return fail(OMR_ERR_ASSERT, "a strip of %d rows of %d columns may take 2^31 bits or more: not supported (smaller strips)", rps, cols);
    if (tenc_bound(rows, cols, rps) > TENC_MAX_FILE)
        return fail(OMR_ERR_ASSERT, "a %d x %d image may take a file of 2^32 bytes or more: not supported", rows, cols);
    if (rps_out) *rps_out = rps;
    return OMR_OK;
}

int omr::tenc_check_params(int cn, int threshold, int rows_per_strip, int dpi)
{
    if (cn != 1 && cn != 3) return fail(OMR_ERR_BADARG, "TIFF takes 1 or 3 channels, got %d", cn);
    if (threshold < 0 || threshold > 254) return fail(OMR_ERR_BADARG, "threshold %d outside 0 .. 254", threshold);
    if (rows_per_strip < 0) return fail(OMR_ERR_BADARG, "rows_per_strip %d is negative", rows_per_strip);
    if (dpi < 0) return fail(OMR_ERR_BADARG, "dpi %d is negative", dpi);
    return OMR_OK;
}

TencStats &omr::tenc_stats() { return thread_stats<TencStats>(); }

int omr::tiff_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n, int threshold,
                            int rows_per_strip, int dpi, JpegSink &sink, hipStream_t s)
{
    tenc_stats().begin_call();
    int rc = tenc_check_params(cn, threshold, rows_per_strip, dpi);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (sizes[2 * (size_t)i] > 0)
            if ((rc = tenc_check_shape(sizes[2 * (size_t)i], sizes[2 * (size_t)i + 1], rows_per_strip, nullptr))) return rc;
    DrainOnExit drain{s};
    return for_each_run(
        sizes, n, kGroupImages, [](int r, int c) { return GroupCost{(int64_t)r * seg_w_of(c) * 4, 0}; },
        [](const GroupCost &sum, const GroupCost &m) { return sum.a + m.a <= kGroupCode; },
        [&](int i0, int g) { return encode_group(d_imgs, img_stride, step, cn, sizes, i0, g, threshold, rows_per_strip, dpi, sink, s); });
}

extern "C" {

int omr_tiff_bound(int32_t rows, int32_t cols, int32_t rows_per_strip, int64_t *bytes)
{
    clear_error();
    if (!bytes) return fail(OMR_ERR_BADARG, "null bytes");
    int rps = 0;
    if (int rc = tenc_check_shape(rows, cols, rows_per_strip, &rps)) return rc;
    *bytes = tenc_bound(rows, cols, rps);
    return OMR_OK;
}

int omr_tiff_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                                 int32_t channels, const int32_t *sizes, int32_t n, int32_t threshold, int32_t rows_per_strip,
                                 int32_t dpi, uint8_t *d_out, int64_t out_stride_bytes, int64_t *out_len)
{
    const BatchEncodeArgs a{d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, d_out, out_stride_bytes, out_len};
    int rps = 0;
    return encode_batch_entry(
        a, "omr_tiff_bound",
        [&] {
            const int rc = tenc_check_params(channels, threshold, rows_per_strip, dpi);
            return rc ? rc : tenc_check_shape(rows, cols, rows_per_strip, &rps);
        },
        [&] { return tenc_bound(rows, cols, rps); }, no_image_check, no_extra_check,
        [&](const int32_t *sz, JpegSink &sink, hipStream_t s) {
            return tiff_encode_device(d_imgs, img_stride_bytes, step_bytes, channels, sz, n, threshold, rows_per_strip, dpi, sink, s);
        });
}

int omr_tiff_encode(const omr_image *src, int32_t threshold, int32_t rows_per_strip, int32_t dpi, uint8_t *out, int64_t cap,
                    int64_t *len)
{
    return encode_one_entry(
        src, out, cap, len, "file",
        [&] {
            const int rc = tenc_check_params(src->channels, threshold, rows_per_strip, dpi);
            return rc ? rc : tenc_check_shape(src->rows, src->cols, rows_per_strip, nullptr);
        },
        no_extra_check,
        [&](const uint8_t *d_img, int64_t stride, int64_t step, const int32_t *size, JpegSink &sink, hipStream_t s) {
            return tiff_encode_device(d_img, stride, step, src->channels, size, 1, threshold, rows_per_strip, dpi, sink, s);
        });
}

int omr_tiff_encode_stats(int32_t enable, int32_t *groups, double *stage_ms)
{
    clear_error();
    tenc_stats().report(enable, groups, stage_ms);
    return OMR_OK;
}

}  // extern "C"
