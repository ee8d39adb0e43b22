// oics_tiff_enc8.cpp -- host side of the 8-bit gray and RGB TIFF encoder (tiff_enc8.hip): the bound
// of a file's length, the parameters and shapes it refuses, a group's layout and launches, and the rule that closes a
// group.  The file's head is tiff_head.hpp's from this writer's description; the entry points omr_tiff8_encode* are the
// shared frame's (codec_host.hpp, section 4.28) with these handed in, an image's own bound among them.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
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

// bytes of a strip of `raw` raw bytes at most
int64_t strip_max(int64_t raw, int compression) { return compression == TENC8_LZW ? tlzwe_strip_bound(raw) : raw; }

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
    GroupStreams out(sink, i0, g);
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
        tenc_set_head(m, TiffHeadDesc{r, c, m.rps, m.ns, 8, cn, compression, cn == 3 ? 2 : 1, predictor, false, dpi});
        stage_words += sw, code_words += cw, strips_all += m.ns;
        max_units = std::max(max_units, (int64_t)r * ((c + 3) / 4));
        max_strips = std::max(max_strips, m.ns), max_seg_w = std::max(max_seg_w, m.seg_w);
    }
    if (strips_all == 0) return out.all_empty();
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
        if (im[(size_t)j].rows) out.len[(size_t)j] = (int64_t)im[(size_t)j].data_at + dyn[(size_t)j].data_len;
    // 2. the files, where the caller wants them
    if ((rc = out.place(im, d_im, s, &p.t.out))) return rc;
    if ((rc = tenc_launch_head(p.t, max_strips, s))) return rc;
    if ((rc = lzw ? tenc8_launch_copy(p, max_strips, 4 * (int64_t)max_seg_w, s) : tenc8_launch_stage(p, max_units, s))) return rc;
    if ((rc = ev.mark(4, s))) return rc;
    OMR_HIP(hipStreamSynchronize(s));
    if ((rc = ev.finish(tenc8_stats()))) return rc;
    return out.done();
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
    b += full * even_offset(strip_max(rps * row, compression));
    if (rest) b += even_offset(strip_max(rest * row, compression));
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
    return for_each_run(
        sizes, n, kGroupImages,
        [&](int r, int c) {  // a: bytes of workspace, b: strips
            const int rps = tenc8_rps(r, c, cn, rows_per_strip);
            int64_t sw, cw;
            int pw, gw;
            work_of(r, c, cn, compression, rps, &sw, &cw, &pw, &gw);
            return GroupCost{4 * (sw + cw), strips_of(r, rps)};
        },
        // closes at kGroupWork only once the group's strips fill the device, and at work_max always
        [&](const GroupCost &sum, const GroupCost &m) { return sum.a + m.a <= (sum.b >= fill ? kGroupWork : work_max); },
        [&](int i0, int g) {
            return encode_group(d_imgs, img_stride, step, cn, sizes, i0, g, compression, predictor, rows_per_strip, dpi, sink, s);
        });
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
    const BatchEncodeArgs a{d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, d_out, out_stride_bytes, out_len};
    int slot_rps = 0;
    return encode_batch_entry(
        a, "omr_tiff8_bound of the slot and of every image",
        [&] {
            const int rc = tenc8_check_params(channels, compression, predictor, rows_per_strip, dpi);
            return rc ? rc : tenc8_check_shape(rows, cols, channels, compression, rows_per_strip, &slot_rps);
        },
        [&] { return tenc8_bound(rows, cols, channels, compression, slot_rps); },
        // the slot's bound, and every image's own: a smaller image has strips of its own (the default depends on its width)
        [&](int r, int c, int64_t *need) {
            int rps = 0;
            const int rc = tenc8_check_shape(r, c, channels, compression, rows_per_strip, &rps);
            if (!rc) *need = std::max(*need, tenc8_bound(r, c, channels, compression, rps));
            return rc;
        },
        no_extra_check,
        [&](const int32_t *sz, JpegSink &sink, hipStream_t s) {
            return tiff8_encode_device(d_imgs, img_stride_bytes, step_bytes, channels, sz, n, compression, predictor, rows_per_strip, dpi, sink, s);
        });
}

int omr_tiff8_encode(const omr_image *src, int32_t compression, int32_t predictor, int32_t rows_per_strip, int32_t dpi, uint8_t *out,
                     int64_t cap, int64_t *len)
{
    return encode_one_entry(
        src, out, cap, len, "file",
        [&] {
            const int rc = tenc8_check_params(src->channels, compression, predictor, rows_per_strip, dpi);
            return rc ? rc : tenc8_check_shape(src->rows, src->cols, src->channels, compression, rows_per_strip, nullptr);
        },
        no_extra_check,
        [&](const uint8_t *d_img, int64_t stride, int64_t step, const int32_t *size, JpegSink &sink, hipStream_t s) {
            return tiff8_encode_device(d_img, stride, step, src->channels, size, 1, compression, predictor, rows_per_strip, dpi, sink, s);
        });
}

int omr_tiff8_encode_stats(int32_t enable, int32_t *groups, double *stage_ms)
{
    clear_error();
    tenc8_stats().report(enable, groups, stage_ms);
    return OMR_OK;
}

}  // extern "C"
