// oics_tiff_enc8.cpp -- host side of the 8-bit gray and RGB TIFF encoder (tiff_enc8.hip): the bound
// of a file's length, the shapes it refuses, the file's head, the launches of a group and the entry points omr_tiff8_bound /
// omr_tiff8_encode*.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "stream_sink.hpp"
#include "tiff_enc8.hpp"
#include "tiff_lzw_enc.hpp"

using namespace omr;

namespace {

// A group of launches closes at kGroupWork bytes of staged strips and coded segments -- but not before it holds a strip for
// every wave the device runs at once (kWavesPerCu a CU): a strip is one wave's, so with one strip a page a group cut by
// bytes alone (49 A4 gray pages) would leave most CUs idle, and the groups run one after another.  Such a group may take
// up to a quarter of the device's free memory.
constexpr int64_t kGroupWork = (int64_t)1 << 30;
constexpr int kGroupImages = 4096;
constexpr int kWavesPerCu = 6;  // tenc8_lzw_kernel: 26 016 bytes of LDS a workgroup of one wave

int strips_of(int rows, int rps) { return (rows + rps - 1) / rps; }
int64_t even(int64_t v) { return (v + 1) & ~(int64_t)1; }
// bytes of a strip of `raw` raw bytes at most
int64_t strip_max(int64_t raw, int compression) { return compression == TENC8_LZW ? tlzwe_strip_bound(raw) : raw; }

void le16(uint8_t *d, uint32_t v) { d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8); }
void le32(uint8_t *d, uint32_t v) { le16(d, v), le16(d + 2, v >> 16); }

// The file's first bytes: "II" 42, the IFD at 8 with its tags in ascending order, the next-IFD pointer 0, then the two
// resolutions (dpi > 0) and BitsPerSample's three values and two zeros (colour).  Behind them, for more than one strip,
// StripOffsets' and StripByteCounts' arrays (LONG), then the strips.
void build_head(TencImg &m, int cn, int compression, int predictor, int dpi)
{
    uint8_t *h = m.head;
    memset(h, 0, sizeof m.head);
    h[0] = h[1] = 'I', le16(h + 2, 42), le32(h + 4, 8);
    const int nt = 9 + (dpi > 0 ? 3 : 0) + (cn == 3 ? 1 : 0) + (predictor == 2 ? 1 : 0);
    const int ifd_end = 8 + 2 + 12 * nt + 4;
    const int res_at = ifd_end, bps_at = res_at + (dpi > 0 ? 16 : 0);
    m.head_len = bps_at + (cn == 3 ? 8 : 0);
    le16(h + 8, (uint32_t)nt);
    uint8_t *e = h + 10;
    auto entry = [&](int tag, int type, uint32_t count, uint32_t value) {
        le16(e, (uint32_t)tag), le16(e + 2, (uint32_t)type), le32(e + 4, count);
        if (type == 3 && count == 1) le16(e + 8, value);
        else le32(e + 8, value);
        e += 12;
        return (int)(e - 4 - h);  // where the value stands
    };
    const uint32_t ns = (uint32_t)m.ns;
    const int arrays_at = m.head_len;
    entry(256, 4, 1, (uint32_t)m.cols);
    entry(257, 4, 1, (uint32_t)m.rows);
    if (cn == 3) entry(258, 3, 3, (uint32_t)bps_at), le16(h + bps_at, 8), le16(h + bps_at + 2, 8), le16(h + bps_at + 4, 8);
    else entry(258, 3, 1, 8);
    entry(259, 3, 1, (uint32_t)compression);
    entry(262, 3, 1, cn == 3 ? 2 : 1);
    const int off_in = entry(273, 4, ns, ns > 1 ? (uint32_t)arrays_at : 0);
    entry(277, 3, 1, (uint32_t)cn);
    entry(278, 4, 1, (uint32_t)m.rps);
    const int cnt_in = entry(279, 4, ns, ns > 1 ? (uint32_t)(arrays_at + 4 * ns) : 0);
    if (dpi > 0) entry(282, 5, 1, (uint32_t)res_at), entry(283, 5, 1, (uint32_t)res_at + 8);
    if (cn == 3) entry(284, 3, 1, 1);
    if (dpi > 0) {
        entry(296, 3, 1, 2);
        le32(h + res_at, (uint32_t)dpi), le32(h + res_at + 4, 1), le32(h + res_at + 8, (uint32_t)dpi), le32(h + res_at + 12, 1);
    }
    if (predictor == 2) entry(317, 3, 1, 2);
    m.off_pos = ns > 1 ? arrays_at : off_in;
    m.cnt_pos = ns > 1 ? arrays_at + 4 * (int)ns : cnt_in;
    m.data_at = arrays_at + (ns > 1 ? 8 * (int)ns : 0);
}

// what image (r x c) takes of a group's workspace, in dwords: staged strips, coded segments
void work_of(int r, int c, int cn, int compression, int rps, int64_t *stage_dw, int64_t *code_dw, int *pack_w, int *seg_w)
{
    const int64_t raw = (int64_t)rps * c * cn;
    *pack_w = *seg_w = 0, *stage_dw = *code_dw = 0;
    if (compression != TENC8_LZW) return;
    *pack_w = (int)((raw + 3) / 4), *seg_w = (int)((tlzwe_strip_bound(raw) + 3) / 4) + 1;
    *stage_dw = (int64_t)strips_of(r, rps) * *pack_w, *code_dw = (int64_t)strips_of(r, rps) * *seg_w;
}

// one group: images [i0, i0 + g)
int encode_group(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int i0, int g, int compression,
                 int predictor, int rows_per_strip, int dpi, JpegSink &sink, hipStream_t s)
{
    std::vector<TencImg> im((size_t)g);
    std::vector<TencDyn> dyn((size_t)g);
    std::vector<int64_t> len((size_t)g, 0), off((size_t)g, 0);
    DrainOnExit drain{s};  // behind the host objects that asynchronous copies read or write, before the device buffers
    StageTimer<TENC8_STAGES> ev;
    if (int r = ev.begin(tenc8_stats().on)) return r;
    const bool lzw = compression == TENC8_LZW;
    int64_t stage_words = 0, code_words = 0, strips_all = 0, max_units = 0;
    int max_strips = 0, max_seg_w = 0;
    for (int j = 0; j < g; j++) {
        TencImg &m = im[(size_t)j];
        memset(&m, 0, sizeof m);
        const int r = sizes[2 * (size_t)(i0 + j)], c = sizes[2 * (size_t)(i0 + j) + 1];
        m.src_off = (int64_t)(i0 + j) * img_stride;
        m.pack_off = stage_words, m.code_off = code_words, m.strip0 = strips_all;
        if (r <= 0) continue;
        m.rows = r, m.cols = c;
        m.rps = tenc8_rps(r, c, cn, rows_per_strip);
        m.ns = strips_of(r, m.rps);
        int64_t sw, cw;
        work_of(r, c, cn, compression, m.rps, &sw, &cw, &m.pack_w, &m.seg_w);
        build_head(m, cn, compression, predictor, dpi);
        stage_words += sw, code_words += cw, strips_all += m.ns;
        max_units = std::max(max_units, (int64_t)r * ((c + 3) / 4));
        max_strips = std::max(max_strips, m.ns), max_seg_w = std::max(max_seg_w, m.seg_w);
    }
    uint8_t *d_out = nullptr;
    if (strips_all == 0) {  // nothing but 0 x 0 entries
        if (int rc = sink.place(i0, g, len.data(), &d_out, off.data())) return rc;
        return sink.done(i0, g, len.data());
    }
    DevBuf d_im, d_dyn, stage, code, sbytes, soff;
    OMR_HIP(d_im.alloc(sizeof(TencImg) * (size_t)g));
    OMR_HIP(d_dyn.alloc(sizeof(TencDyn) * (size_t)g));
    if (lzw) {
        OMR_HIP(stage.alloc((size_t)stage_words * 4));
        OMR_HIP(code.alloc((size_t)code_words * 4));
    }
    OMR_HIP(sbytes.alloc((size_t)strips_all * 4));
    OMR_HIP(soff.alloc((size_t)strips_all * 4));
    Tenc8Pass p;
    memset(&p, 0, sizeof p);
    p.t.src = d_imgs, p.t.step = step, p.t.imgs = d_im.as<TencImg>(), p.t.dyn = d_dyn.as<TencDyn>(), p.t.n = g, p.t.cn = cn;
    p.t.sbytes = sbytes.as<uint32_t>(), p.t.soff = soff.as<uint32_t>();
    p.predictor = predictor, p.raw_to_file = !lzw;
    p.stage = lzw ? stage.as<uint32_t>() : nullptr, p.code = lzw ? code.as<uint32_t>() : nullptr;
    // 1. everything up to the strips' sizes; the host learns every file's length
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(TencImg) * (size_t)g, hipMemcpyHostToDevice, s));
    int rc = ev.mark(0, s);
    if (rc) return rc;
    if (lzw) {
        if ((rc = tenc8_launch_stage(p, max_units, s)) || (rc = ev.mark(1, s)) || (rc = tenc8_launch_lzw(p, max_strips, s))) return rc;
    } else {
        if ((rc = ev.mark(1, s)) || (rc = tenc8_launch_rawlens(p, max_strips, s))) return rc;
    }
    if ((rc = ev.mark(2, s)) || (rc = tenc_launch_stripscan(p.t, max_strips, s)) || (rc = ev.mark(3, s))) return rc;
    OMR_HIP(hipMemcpyAsync(dyn.data(), d_dyn.p, sizeof(TencDyn) * (size_t)g, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < g; j++)
        if (im[(size_t)j].rows) len[(size_t)j] = (int64_t)im[(size_t)j].data_at + dyn[(size_t)j].data_len;
    // 2. the files, where the caller wants them
    if ((rc = sink.place(i0, g, len.data(), &d_out, off.data()))) return rc;
    for (int j = 0; j < g; j++) im[(size_t)j].out_off = off[(size_t)j];
    p.t.out = d_out;
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(TencImg) * (size_t)g, hipMemcpyHostToDevice, s));
    if ((rc = tenc_launch_head(p.t, max_strips, s))) return rc;
    if ((rc = lzw ? tenc8_launch_copy(p, max_strips, 4 * (int64_t)max_seg_w, s) : tenc8_launch_stage(p, max_units, s))) return rc;
    if ((rc = ev.mark(4, s))) return rc;
    OMR_HIP(hipStreamSynchronize(s));
    if ((rc = ev.finish(tenc8_stats()))) return rc;
    return sink.done(i0, g, len.data());
}

}  // namespace

int omr::tenc8_rps(int rows, int cols, int cn, int rows_per_strip)
{
    if (rows_per_strip > 0) return std::min(rows_per_strip, rows);
    const int64_t row = (int64_t)cols * cn;
    return (int)std::min<int64_t>(rows, std::max<int64_t>(1, TENC8_DEFAULT_STRIP / row));
}

// The file: header, IFD, resolutions and BitsPerSample (TENC8_HEAD_MAX at most), the two strip arrays (8 bytes a strip), and
// per strip its bytes and one more to an even offset.  A raw strip is its rows; an LZW strip of n raw bytes takes at most
// tlzwe_strip_bound(n) bytes (tiff_lzw_enc.hpp: 12 bits a byte, its Clears, its EOI, the pad), whatever the predictor.
int64_t omr::tenc8_bound(int rows, int cols, int cn, int compression, int rps)
{
    const int full = rows / rps, rest = rows % rps;
    const int64_t row = (int64_t)cols * cn;
    int64_t b = TENC8_HEAD_MAX + 8 * (int64_t)strips_of(rows, rps);
    b += full * even(strip_max(rps * row, compression));
    if (rest) b += even(strip_max(rest * row, compression));
    return b;
}

int omr::tenc8_check_shape(int rows, int cols, int cn, int compression, int rows_per_strip, int *rps_out)
{
    if (rows <= 0 || cols <= 0) return fail(OMR_ERR_ASSERT, "empty image");
    if (rows > TENC_MAX_SIDE || cols > TENC_MAX_SIDE || (int64_t)rows * cols > TENC_MAX_PIXELS)
        return fail(OMR_ERR_ASSERT, "%d x %d is above imread's limits (2^20 a side, 2^30 pixels): not supported", rows, cols);
    const int rps = tenc8_rps(rows, cols, cn, rows_per_strip);
    if (8 * strip_max((int64_t)rps * cols * cn, compression) > TENC_MAX_STRIP_BITS)
        return fail(OMR_ERR_ASSERT, "a strip of %d rows of %d columns may take 2^31 bits or more: not supported (smaller strips)", rps, cols);
    if (tenc8_bound(rows, cols, cn, compression, rps) > TENC_MAX_FILE)
        return fail(OMR_ERR_ASSERT, "a %d x %d image may take a file of 2^32 bytes or more: not supported", rows, cols);
    if (rps_out) *rps_out = rps;
    return OMR_OK;
}

int omr::tenc8_check_params(int cn, int compression, int predictor, int rows_per_strip, int dpi)
{
    if (cn != 1 && cn != 3) return fail(OMR_ERR_BADARG, "TIFF takes 1 or 3 channels, got %d", cn);
    if (compression != TENC8_NONE && compression != TENC8_LZW) return fail(OMR_ERR_BADARG, "compression %d (1 = none, 5 = LZW)", compression);
    if (predictor != 1 && predictor != 2) return fail(OMR_ERR_BADARG, "predictor %d (1 or 2)", predictor);
    if (predictor == 2 && compression != TENC8_LZW) return fail(OMR_ERR_BADARG, "predictor 2 goes with LZW only");
    if (rows_per_strip < 0) return fail(OMR_ERR_BADARG, "rows_per_strip %d is negative", rows_per_strip);
    if (dpi < 0) return fail(OMR_ERR_BADARG, "dpi %d is negative", dpi);
    return OMR_OK;
}

Tenc8Stats &omr::tenc8_stats() { return thread_stats<Tenc8Stats>(); }

int omr::tiff8_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n, int compression,
                             int predictor, int rows_per_strip, int dpi, JpegSink &sink, hipStream_t s)
{
    tenc8_stats().begin_call();
    int rc = tenc8_check_params(cn, compression, predictor, rows_per_strip, dpi);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (sizes[2 * (size_t)i] > 0)
            if ((rc = tenc8_check_shape(sizes[2 * (size_t)i], sizes[2 * (size_t)i + 1], cn, compression, rows_per_strip, nullptr))) return rc;
    DrainOnExit drain{s};
    int dev = 0, cus = 0;
    size_t mem_free = 0, mem_total = 0;
    OMR_HIP(hipGetDevice(&dev));
    OMR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    OMR_HIP(hipMemGetInfo(&mem_free, &mem_total));
    const int64_t fill = (int64_t)kWavesPerCu * cus, work_max = std::max<int64_t>(kGroupWork, (int64_t)(mem_free / 4));
    for (int i0 = 0; i0 < n;) {
        int g = 0;
        int64_t bytes = 0, strips = 0;
        while (i0 + g < n && g < kGroupImages) {
            const int r = sizes[2 * (size_t)(i0 + g)], c = sizes[2 * (size_t)(i0 + g) + 1];
            int64_t sw = 0, cw = 0;
            int pw, gw;
            if (r > 0) work_of(r, c, cn, compression, tenc8_rps(r, c, cn, rows_per_strip), &sw, &cw, &pw, &gw);
            const int64_t b = 4 * (sw + cw);
            if (g > 0 && ((bytes + b > kGroupWork && strips >= fill) || bytes + b > work_max)) break;
            bytes += b, g++;
            if (r > 0) strips += (r + tenc8_rps(r, c, cn, rows_per_strip) - 1) / tenc8_rps(r, c, cn, rows_per_strip);
        }
        if ((rc = encode_group(d_imgs, img_stride, step, cn, sizes, i0, g, compression, predictor, rows_per_strip, dpi, sink, s))) return rc;
        i0 += g;
    }
    return OMR_OK;
}

extern "C" {

int omr_tiff8_bound(int32_t rows, int32_t cols, int32_t channels, int32_t compression, int32_t rows_per_strip, int64_t *bytes)
{
    clear_error();
    if (!bytes) return fail(OMR_ERR_BADARG, "null bytes");
    int rps = 0;
    int rc = tenc8_check_params(channels, compression, 1, rows_per_strip, 0);
    if (rc || (rc = tenc8_check_shape(rows, cols, channels, compression, rows_per_strip, &rps))) return rc;
    *bytes = tenc8_bound(rows, cols, channels, compression, rps);
    return OMR_OK;
}

int omr_tiff8_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                                  int32_t channels, const int32_t *sizes, int32_t n, int32_t compression, int32_t predictor,
                                  int32_t rows_per_strip, int32_t dpi, uint8_t *d_out, int64_t out_stride_bytes, int64_t *out_len)
{
    clear_error();
    if (!d_imgs || !d_out || !out_len) return fail(OMR_ERR_BADARG, "null argument");
    if (n < 0) return fail(OMR_ERR_BADARG, "negative n");
    int slot_rps = 0;
    int rc = tenc8_check_params(channels, compression, predictor, rows_per_strip, dpi);
    if (rc || (rc = tenc8_check_shape(rows, cols, channels, compression, rows_per_strip, &slot_rps))) return rc;
    if (step_bytes < (int64_t)cols * channels) return fail(OMR_ERR_BADARG, "step_bytes < cols x channels");
    if (img_stride_bytes < (int64_t)rows * step_bytes) return fail(OMR_ERR_BADARG, "img_stride_bytes < rows x step_bytes");
    std::vector<int32_t> sz(2 * (size_t)n);
    // the slot's bound, and every image's own: a smaller image has strips of its own (the default depends on its width)
    int64_t need = tenc8_bound(rows, cols, channels, compression, slot_rps);
    for (int i = 0; i < n; i++) {
        const int r = sizes ? sizes[2 * (size_t)i] : rows, c = sizes ? sizes[2 * (size_t)i + 1] : cols;
        if (r < 0 || c < 0 || r > rows || c > cols || ((r == 0) != (c == 0)))
            return fail(OMR_ERR_BADARG, "sizes[%d] = %d x %d does not fit the %d x %d slot", i, r, c, rows, cols);
        sz[2 * (size_t)i] = r, sz[2 * (size_t)i + 1] = c;
        int rps = 0;
        if (r > 0) {
            if ((rc = tenc8_check_shape(r, c, channels, compression, rows_per_strip, &rps))) return rc;
            need = std::max(need, tenc8_bound(r, c, channels, compression, rps));
        }
    }
    if (out_stride_bytes < need)
        return fail(OMR_ERR_BADARG, "out_stride_bytes below omr_tiff8_bound of the slot and of every image (%lld)", (long long)need);
    if (n == 0) return OMR_OK;
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    SlotSink sink;
    sink.d_out = d_out, sink.stride = out_stride_bytes, sink.out_len = out_len;
    return tiff8_encode_device(d_imgs, img_stride_bytes, step_bytes, channels, sz.data(), n, compression, predictor, rows_per_strip, dpi, sink,
                               st.s);
}

int omr_tiff8_encode(const omr_image *src, int32_t compression, int32_t predictor, int32_t rows_per_strip, int32_t dpi, uint8_t *out,
                     int64_t cap, int64_t *len)
{
    clear_error();
    if (!src || !src->data || !len || cap < 0 || (!out && cap > 0)) return fail(OMR_ERR_BADARG, "null argument");
    int rc = tenc8_check_params(src->channels, compression, predictor, rows_per_strip, dpi);
    if (rc || (rc = tenc8_check_shape(src->rows, src->cols, src->channels, compression, rows_per_strip, nullptr))) return rc;
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
    rc = tiff8_encode_device(in.as<uint8_t>(), row * src->rows, row, src->channels, size, 1, compression, predictor, rows_per_strip, dpi, sink,
                             st.s);
    if (rc) return rc;
    *len = sink.len;
    if (!sink.fits) return fail(OMR_ERR_NOMEM, "the file takes %lld bytes, the buffer holds %lld", (long long)sink.len, (long long)cap);
    return OMR_OK;
}

int omr_tiff8_encode_stats(int32_t enable, int32_t *groups, double *stage_ms)
{
    clear_error();
    tenc8_stats().report(enable, groups, stage_ms);
    return OMR_OK;
}

}  // extern "C"
