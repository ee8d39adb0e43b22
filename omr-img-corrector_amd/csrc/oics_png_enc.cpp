// oics_png_enc.cpp -- host side of the PNG encoder (png_enc.hip): the bound of a stream's length,
// the shapes it refuses, a group's layout and launches, and the cost that closes a group.  The entry points
// omr_png_encode* are the shared frame's (codec_host.hpp, section 4.28) with these handed in.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "png_enc.hpp"

using namespace omr;

namespace {

// raw bytes of one group of launches; the workspace is about five times that (raw, two bytes of match / token entry per
// raw byte, the bit buffer, the code tables)
constexpr int64_t kGroupRaw = (int64_t)512 << 20;
constexpr int kGroupImages = 4096;

int64_t blocks_of(int64_t raw) { return (raw + PENC_BLOCK - 1) / PENC_BLOCK; }

// one group: images [i0, i0 + g)
int encode_group(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int i0, int g,
                 int compression, JpegSink &sink, hipStream_t s)
{
    std::vector<PencImg> im((size_t)g);
    std::vector<PencDyn> dyn((size_t)g);
    GroupStreams out(sink, i0, g);
    DrainOnExit drain{s};  // behind the host objects that asynchronous copies read or write, before the device buffers
    StageTimer<PENC_STAGES> ev;
    if (int r = ev.begin(penc_stats().on)) return r;
    int64_t raw_bytes = 0, blocks = 0, max_raw = 0;
    int max_rows = 0;
    for (int j = 0; j < g; j++) {
        PencImg &m = im[(size_t)j];
        memset(&m, 0, sizeof m);
        const int r = sizes[2 * (size_t)(i0 + j)], c = sizes[2 * (size_t)(i0 + j) + 1];
        const int64_t raw = r > 0 ? penc_raw_bytes(r, c, cn) : 0;
        m.src_off = (int64_t)(i0 + j) * img_stride;
        m.raw_off = raw_bytes, m.blk0 = blocks;
        m.raw_len = (uint32_t)raw, m.nblk = (uint32_t)blocks_of(raw), m.npiece = (uint32_t)((raw + PENC_PIECE - 1) / PENC_PIECE);
        m.rows = r, m.cols = c, m.row_bytes = c * cn;
        raw_bytes += up16(raw), blocks += m.nblk;
        max_raw = std::max(max_raw, raw), max_rows = std::max(max_rows, r);
    }
    if (blocks == 0) return out.all_empty();
    const int max_blocks = (int)blocks_of(max_raw), max_pieces = (int)((max_raw + PENC_PIECE - 1) / PENC_PIECE);
    const bool stored_only = compression == 0;
    DevBuf d_im, d_dyn, raw, mt, pcnt, pbit, blk, codes, hdr, zbuf;
    OMR_HIP(d_im.alloc(sizeof(PencImg) * (size_t)g));
    OMR_HIP(d_dyn.alloc(sizeof(PencDyn) * (size_t)g));
    OMR_HIP(raw.alloc((size_t)raw_bytes));
    OMR_HIP(blk.alloc(sizeof(PencBlk) * (size_t)blocks));
    if (!stored_only) {
        OMR_HIP(mt.alloc((size_t)raw_bytes * 2));
        OMR_HIP(pcnt.alloc((size_t)blocks * PENC_BLOCK_PIECES * 2));
        OMR_HIP(pbit.alloc((size_t)blocks * PENC_BLOCK_PIECES * 4));
        OMR_HIP(codes.alloc((size_t)blocks * PENC_CODES * 4));
        OMR_HIP(hdr.alloc((size_t)blocks * PENC_HDR_WORDS * 4));
        OMR_HIP(zbuf.alloc((size_t)blocks * PENC_ZBLOCK));
    }
    PencPass p;
    memset(&p, 0, sizeof p);
    p.src = d_imgs, p.step = step, p.imgs = d_im.as<PencImg>(), p.dyn = d_dyn.as<PencDyn>(), p.n = g, p.cn = cn;
    p.stored_only = stored_only;
    p.raw = raw.as<uint8_t>(), p.mt = mt.as<uint16_t>(), p.piece_cnt = pcnt.as<uint16_t>(), p.piece_bit = pbit.as<uint32_t>();
    p.blk = blk.as<PencBlk>(), p.codes = codes.as<uint32_t>(), p.hdr = hdr.as<uint32_t>(), p.zbuf = zbuf.as<uint32_t>();
    // 1. everything up to the blocks' sizes; the host learns every stream's length
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(PencImg) * (size_t)g, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemsetAsync(d_dyn.p, 0, sizeof(PencDyn) * (size_t)g, s));
    int rc = ev.mark(0, s);
    if (rc || (rc = penc_launch_filter(p, max_rows, s)) || (rc = ev.mark(1, s)) || (rc = penc_launch_adler(p, max_raw, s)) || (rc = ev.mark(2, s)))
        return rc;
    if (!stored_only && (rc = penc_launch_parse(p, max_raw, max_pieces, s))) return rc;
    if ((rc = ev.mark(3, s)) || (rc = penc_launch_blocks(p, max_blocks, s)) || (rc = ev.mark(4, s))) return rc;
    if (!stored_only) {
        OMR_HIP(hipMemsetAsync(zbuf.p, 0, (size_t)blocks * PENC_ZBLOCK, s));
        if ((rc = penc_launch_bits(p, max_blocks, s))) return rc;
    }
    if ((rc = ev.mark(5, s))) return rc;
    OMR_HIP(hipMemcpyAsync(dyn.data(), d_dyn.p, sizeof(PencDyn) * (size_t)g, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < g; j++)
        if (im[(size_t)j].nblk) out.len[(size_t)j] = (int64_t)PENC_BEFORE + dyn[(size_t)j].deflate_len + PENC_AFTER;
    // 2. the streams, where the caller wants them
    if ((rc = out.place(im, d_im, s, &p.out))) return rc;
    if ((rc = penc_launch_streams(p, max_blocks, s)) || (rc = ev.mark(6, s))) return rc;
    OMR_HIP(hipStreamSynchronize(s));
    if ((rc = ev.finish(penc_stats()))) return rc;
    return out.done();
}

}  // namespace

int64_t omr::penc_raw_bytes(int rows, int cols, int cn) { return (int64_t)rows * (1 + (int64_t)cols * cn); }

int64_t omr::penc_bound(int rows, int cols, int cn)
{
    const int64_t raw = penc_raw_bytes(rows, cols, cn);
    return PENC_BEFORE + raw + PENC_STORED_HEAD * blocks_of(raw) + PENC_AFTER;
}

int omr::penc_check_shape(int rows, int cols, int cn)
{
    if (cn != 1 && cn != 3 && cn != 4) return fail(OMR_ERR_ASSERT, "PNG takes 1, 3 or 4 channels, got %d", cn);
    if (rows <= 0 || cols <= 0) return fail(OMR_ERR_ASSERT, "empty image");
    if (rows > PENC_MAX_SIDE || cols > PENC_MAX_SIDE || (int64_t)rows * cols > PENC_MAX_PIXELS)
        return fail(OMR_ERR_ASSERT, "%d x %d is above imread's limits (2^20 a side, 2^30 pixels): not supported", rows, cols);
    const int64_t raw = penc_raw_bytes(rows, cols, cn);
    if (2 + raw + PENC_STORED_HEAD * blocks_of(raw) + 4 > PENC_MAX_IDAT)
        return fail(OMR_ERR_ASSERT, "a %d x %d x %d image may take an IDAT chunk of 2^31 bytes or more: not supported", rows, cols, cn);
    return OMR_OK;
}

PencStats &omr::penc_stats() { return thread_stats<PencStats>(); }

int omr::png_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n,
                           int compression, JpegSink &sink, hipStream_t s)
{
    penc_stats().begin_call();
    compression = std::min(std::max(compression, 0), 9);
    for (int i = 0; i < n; i++)
        if (sizes[2 * (size_t)i] > 0)
            if (int rc = penc_check_shape(sizes[2 * (size_t)i], sizes[2 * (size_t)i + 1], cn)) return rc;
    DrainOnExit drain{s};
    return for_each_run(
        sizes, n, kGroupImages, [&](int r, int c) { return GroupCost{penc_raw_bytes(r, c, cn), 0}; },
        [](const GroupCost &sum, const GroupCost &m) { return sum.a + m.a <= kGroupRaw; },
        [&](int i0, int g) { return encode_group(d_imgs, img_stride, step, cn, sizes, i0, g, compression, sink, s); });
}

extern "C" {

int omr_png_bound(int32_t rows, int32_t cols, int32_t channels, int64_t *bytes)
{
    clear_error();
    if (!bytes) return fail(OMR_ERR_BADARG, "null bytes");
    if (int rc = penc_check_shape(rows, cols, channels)) return rc;
    *bytes = penc_bound(rows, cols, channels);
    return OMR_OK;
}

int omr_png_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                                int32_t channels, const int32_t *sizes, int32_t n, int32_t compression, uint8_t *d_out,
                                int64_t out_stride_bytes, int64_t *out_len)
{
    const BatchEncodeArgs a{d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, d_out, out_stride_bytes, out_len};
    return encode_batch_entry(
        a, "omr_png_bound", [&] { return penc_check_shape(rows, cols, channels); }, [&] { return penc_bound(rows, cols, channels); },
        no_image_check, no_extra_check,
        [&](const int32_t *sz, JpegSink &sink, hipStream_t s) {
            return png_encode_device(d_imgs, img_stride_bytes, step_bytes, channels, sz, n, compression, sink, s);
        });
}

int omr_png_encode(const omr_image *src, int32_t compression, uint8_t *out, int64_t cap, int64_t *len)
{
    return encode_one_entry(
        src, out, cap, len, "stream", [&] { return penc_check_shape(src->rows, src->cols, src->channels); }, no_extra_check,
        [&](const uint8_t *d_img, int64_t stride, int64_t step, const int32_t *size, JpegSink &sink, hipStream_t s) {
            return png_encode_device(d_img, stride, step, src->channels, size, 1, compression, sink, s);
        });
}

int omr_png_encode_stats(int32_t enable, int32_t *groups, double *stage_ms)
{
    clear_error();
    penc_stats().report(enable, groups, stage_ms);
    return OMR_OK;
}

}  // extern "C"
