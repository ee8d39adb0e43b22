// oics_tiff_enc.cpp -- host side of the Group 4 TIFF encoder (tiff_enc.hip): the bound of a file's
// length, the shapes it refuses, the file's head, the launches of a group and the entry points omr_tiff_bound /
// omr_tiff_encode*.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "stream_sink.hpp"
#include "tiff_dec.hpp"  // tdec_code_tables: the one set of T.4 codes
#include "tiff_enc.hpp"

using namespace omr;

namespace {

// bytes of row code segments in one group of launches (the largest part of the workspace)
constexpr int64_t kGroupCode = (int64_t)1 << 30;
constexpr int kGroupImages = 4096;

int pack_w_of(int cols) { return (cols + 31) / 32 + 1; }
int seg_w_of(int cols) { return (int)((tenc_row_bits(cols) + 31) / 32) + 1; }
int strips_of(int rows, int rps) { return (rows + rps - 1) / rps; }
int64_t strip_bytes_max(int rows_of_strip, int cols) { return ((int64_t)rows_of_strip * tenc_row_bits(cols) + TENC_EOFB_BITS + 7) / 8; }
// halvings that empty a range of v
int halvings(int v)
{
    int k = 1;
    while (((int64_t)1 << k) < v) k++;
    return k + 1;
}

void le16(uint8_t *d, uint32_t v) { d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8); }
void le32(uint8_t *d, uint32_t v) { le16(d, v), le16(d + 2, v >> 16); }

// The file's first bytes: "II" 42, the IFD at 8 with its tags in ascending order, the next-IFD pointer 0, the two
// resolutions.  Behind them, for more than one strip, StripOffsets' and StripByteCounts' arrays (LONG), then the strips.
void build_head(TencImg &m, int dpi)
{
    uint8_t *h = m.head;
    memset(h, 0, sizeof m.head);
    h[0] = h[1] = 'I', le16(h + 2, 42), le32(h + 4, 8);
    const int nt = dpi > 0 ? 13 : 10;
    const int ifd_end = 8 + 2 + 12 * nt + 4;
    const int res_at = ifd_end;
    m.head_len = ifd_end + (dpi > 0 ? 16 : 0);
    le16(h + 8, (uint32_t)nt);
    uint8_t *e = h + 10;
    auto entry = [&](int tag, int type, uint32_t count, uint32_t value) {
        le16(e, (uint32_t)tag), le16(e + 2, (uint32_t)type), le32(e + 4, count);
        if (type == 3) le16(e + 8, value);
        else le32(e + 8, value);
        e += 12;
        return (int)(e - 4 - h);  // where the value stands
    };
    const uint32_t ns = (uint32_t)m.ns;
    const int arrays_at = m.head_len;
    entry(256, 4, 1, (uint32_t)m.cols);
    entry(257, 4, 1, (uint32_t)m.rows);
    entry(258, 3, 1, 1);
    entry(259, 3, 1, 4);
    entry(262, 3, 1, 0);
    const int off_in = entry(273, 4, ns, ns > 1 ? (uint32_t)arrays_at : 0);
    entry(277, 3, 1, 1);
    entry(278, 4, 1, (uint32_t)m.rps);
    const int cnt_in = entry(279, 4, ns, ns > 1 ? (uint32_t)(arrays_at + 4 * ns) : 0);
    if (dpi > 0) entry(282, 5, 1, (uint32_t)res_at), entry(283, 5, 1, (uint32_t)res_at + 8);
    entry(293, 4, 1, 0);
    if (dpi > 0) {
        entry(296, 3, 1, 2);
        le32(h + res_at, (uint32_t)dpi), le32(h + res_at + 4, 1), le32(h + res_at + 8, (uint32_t)dpi), le32(h + res_at + 12, 1);
    }
    m.off_pos = ns > 1 ? arrays_at : off_in;
    m.cnt_pos = ns > 1 ? arrays_at + 4 * (int)ns : cnt_in;
    m.data_at = arrays_at + (ns > 1 ? 8 * (int)ns : 0);
}

// one group: images [i0, i0 + g)
int encode_group(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int i0, int g, int threshold,
                 int rows_per_strip, int dpi, JpegSink &sink, hipStream_t s)
{
    std::vector<TencImg> im((size_t)g);
    std::vector<TencDyn> dyn((size_t)g);
    std::vector<int64_t> len((size_t)g, 0), off((size_t)g, 0);
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
        build_head(m, dpi);
        pack_words += ((int64_t)r + 1) * m.pack_w, code_words += (int64_t)r * m.seg_w, rows_all += r, strips_all += m.ns;
        max_pack_bytes = std::max(max_pack_bytes, ((int64_t)r + 1) * m.pack_w * 4);
        max_rows = std::max(max_rows, r), max_cols = std::max(max_cols, c);
        max_strips = std::max(max_strips, m.ns), max_rps = std::max(max_rps, m.rps);
    }
    uint8_t *d_out = nullptr;
    if (rows_all == 0) {  // nothing but 0 x 0 entries
        if (int rc = sink.place(i0, g, len.data(), &d_out, off.data())) return rc;
        return sink.done(i0, g, len.data());
    }
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
            len[(size_t)j] = (int64_t)im[(size_t)j].data_at + dyn[(size_t)j].data_len;
            max_data = std::max<int64_t>(max_data, dyn[(size_t)j].data_len);
        }
    // 2. the files, where the caller wants them
    if ((rc = sink.place(i0, g, len.data(), &d_out, off.data()))) return rc;
    for (int j = 0; j < g; j++) im[(size_t)j].out_off = off[(size_t)j];
    p.out = d_out;
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(TencImg) * (size_t)g, hipMemcpyHostToDevice, s));
    if ((rc = tenc_launch_merge(p, max_data, max_strips, s)) || (rc = ev.mark(4, s))) return rc;
    OMR_HIP(hipStreamSynchronize(s));
    if ((rc = ev.finish(tenc_stats()))) return rc;
    return sink.done(i0, g, len.data());
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
    b += full * ((strip_bytes_max(rps, cols) + 1) & ~(int64_t)1);
    if (rest) b += (strip_bytes_max(rest, cols) + 1) & ~(int64_t)1;
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
    for (int i0 = 0; i0 < n;) {
        int g = 0;
        int64_t bytes = 0;
        while (i0 + g < n && g < kGroupImages) {
            const int r = sizes[2 * (size_t)(i0 + g)], c = sizes[2 * (size_t)(i0 + g) + 1];
            const int64_t b = r > 0 ? (int64_t)r * seg_w_of(c) * 4 : 0;
            if (g > 0 && bytes + b > kGroupCode) break;
            bytes += b, g++;
        }
        if ((rc = encode_group(d_imgs, img_stride, step, cn, sizes, i0, g, threshold, rows_per_strip, dpi, sink, s))) return rc;
        i0 += g;
    }
    return OMR_OK;
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
    clear_error();
    if (!d_imgs || !d_out || !out_len) return fail(OMR_ERR_BADARG, "null argument");
    if (n < 0) return fail(OMR_ERR_BADARG, "negative n");
    int rps = 0;
    int rc = tenc_check_params(channels, threshold, rows_per_strip, dpi);
    if (rc || (rc = tenc_check_shape(rows, cols, rows_per_strip, &rps))) return rc;
    if (step_bytes < (int64_t)cols * channels) return fail(OMR_ERR_BADARG, "step_bytes < cols x channels");
    if (img_stride_bytes < (int64_t)rows * step_bytes) return fail(OMR_ERR_BADARG, "img_stride_bytes < rows x step_bytes");
    std::vector<int32_t> sz(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const int r = sizes ? sizes[2 * (size_t)i] : rows, c = sizes ? sizes[2 * (size_t)i + 1] : cols;
        if (r < 0 || c < 0 || r > rows || c > cols || ((r == 0) != (c == 0)))
            return fail(OMR_ERR_BADARG, "sizes[%d] = %d x %d does not fit the %d x %d slot", i, r, c, rows, cols);
        sz[2 * (size_t)i] = r, sz[2 * (size_t)i + 1] = c;
    }
    if (out_stride_bytes < tenc_bound(rows, cols, rps))
        return fail(OMR_ERR_BADARG, "out_stride_bytes below omr_tiff_bound (%lld)", (long long)tenc_bound(rows, cols, rps));
    if (n == 0) return OMR_OK;
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    SlotSink sink;
    sink.d_out = d_out, sink.stride = out_stride_bytes, sink.out_len = out_len;
    return tiff_encode_device(d_imgs, img_stride_bytes, step_bytes, channels, sz.data(), n, threshold, rows_per_strip, dpi, sink, st.s);
}

int omr_tiff_encode(const omr_image *src, int32_t threshold, int32_t rows_per_strip, int32_t dpi, uint8_t *out, int64_t cap,
                    int64_t *len)
{
    clear_error();
    if (!src || !src->data || !len || cap < 0 || (!out && cap > 0)) return fail(OMR_ERR_BADARG, "null argument");
    int rc = tenc_check_params(src->channels, threshold, rows_per_strip, dpi);
    if (rc || (rc = tenc_check_shape(src->rows, src->cols, rows_per_strip, nullptr))) return rc;
    if (src->step_bytes < (int64_t)src->cols * src->channels) return fail(OMR_ERR_BADARG, "step_bytes too small");
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    const int64_t row = (int64_t)src->cols * src->channels;
    DevBuf in;
    OMR_HIP(in.alloc((size_t)(row * src->rows)));
    if ((rc = upload_rows(in.p, (size_t)row, src->data, (size_t)src->step_bytes, (size_t)row, (size_t)src->rows, st.s))) return rc;
    const int32_t size[2] = {src->rows, src->cols};
    HostSink sink;
    sink.out = out, sink.cap = cap, sink.s = st.s;
    rc = tiff_encode_device(in.as<uint8_t>(), row * src->rows, row, src->channels, size, 1, threshold, rows_per_strip, dpi, sink, st.s);
    if (rc) return rc;
    *len = sink.len;
    if (!sink.fits) return fail(OMR_ERR_NOMEM, "the file takes %lld bytes, the buffer holds %lld", (long long)sink.len, (long long)cap);
    return OMR_OK;
}

int omr_tiff_encode_stats(int32_t enable, int32_t *groups, double *stage_ms)
{
    clear_error();
    tenc_stats().report(enable, groups, stage_ms);
    return OMR_OK;
}

}  // extern "C"
