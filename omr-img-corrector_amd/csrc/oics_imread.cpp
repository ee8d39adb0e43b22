// oics_imread.cpp -- host side of the orientation transforms (orient.hip) and the imread layer above the three decoders
// (DESIGN.md sections 4.23 and 4.25): omr_orient*, omr_imread*.  imread(IMREAD_COLOR) turns a JPEG by its EXIF orientation; the
// decoders' own entry points refuse such a stream, this layer decodes it into a scratch buffer and turns it on the device.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "orient.hpp"

using namespace omr;

namespace {

int cn_orient(int cn)
{
    if (cn != 1 && cn != 3) return fail(OMR_ERR_BADARG, "an image to turn has 1 or 3 channels, got %d", cn);
    return OMR_OK;
}

int check_code(int code)
{
    if (code < 1 || code > 8) return fail(OMR_ERR_BADARG, "EXIF orientation %d (1..8)", code);
    return OMR_OK;
}

int check_flags(int flags)
{
    if (flags & ~OMR_IMREAD_IGNORE_ORIENTATION) return fail(OMR_ERR_BADARG, "flags %d (0 or OMR_IMREAD_IGNORE_ORIENTATION)", flags);
    return OMR_OK;
}

// the slot rules of the decoders' batch entry points
int check_slots(const void *p, int64_t stride, int64_t step, int rows, int cols, int channels, const char *side)
{
    if (!p) return fail(OMR_ERR_BADARG, "null %s", side);
    if (rows <= 0 || cols <= 0) return fail(OMR_ERR_BADARG, "empty %s slot", side);
    if (step < (int64_t)cols * channels) return fail(OMR_ERR_BADARG, "%s: step_bytes < cols x channels", side);
    if (stride / rows < step) return fail(OMR_ERR_BADARG, "%s: stride_bytes < rows x step_bytes", side);
    return OMR_OK;
}

}  // namespace

int omr::imread_turn_of(const JdecHeader &h, bool ignore)
{
    if (ignore || h.orient == 1) return 0;
    if (h.orient < 1 || h.orient > 8)
        return fail(OMR_ERR_NOTIMPL, "EXIF orientation %d is outside 1..8: what imread does with it is not established", h.orient);
    return 1;
}

ImreadParsed omr::imread_parse(const uint8_t *s, int64_t len, int channels, bool ignore, JdecHeader *h, PdecHeader *ph, TdecHeader *th)
{
    ImreadParsed p;
    if (pdec_is_png(s, len)) {
        p.kind = IMREAD_PNG;
        p.rc = pdec_parse(s, len, ph);
        p.rows = ph->rows, p.cols = ph->cols, p.orient = ph->orient;
        p.components = ph->rows ? (ph->color_type == 0 || ph->color_type == 4 ? 1 : 3) : 0;
        if (!p.rc && channels) p.rc = pdec_check_channels(*ph, channels);
        return p;
    }
    if (tdec_is_tiff(s, len)) {
        p.kind = IMREAD_TIFF;
        p.rc = tdec_parse(s, len, th);
        p.rows = th->rows, p.cols = th->cols, p.orient = th->orient;
        p.components = th->rows ? th->samples : 0;
        if (!p.rc && channels) p.rc = tdec_check_channels(*th, channels);
        return p;
    }
    p.rc = jdec_parse(s, len, h, false);
    p.rows = h->rows, p.cols = h->cols, p.components = h->ncomp, p.orient = h->orient;
    if (p.rc) return p;
    const int turn = imread_turn_of(*h, ignore);
    if (turn < 0) p.rc = turn;
    else if (turn && orient_transposes(h->orient)) std::swap(p.rows, p.cols);
    return p;
}

ImreadParsed ImreadRun::append(const uint8_t *stream, int64_t len, int channels, bool ignore)
{
    jpeg.emplace_back(), png.emplace_back(), tiff.emplace_back();
    const ImreadParsed p = imread_parse(stream, len, channels, ignore, &jpeg.back(), &png.back(), &tiff.back());
    kind.push_back((uint8_t)p.kind);
    return p;
}

void ImreadChunk::gather(const ImreadHeaders &src, const uint8_t *const *streams, const int64_t *len, const std::vector<int> &idx, int j0, int z)
{
    zs.resize((size_t)z), zlen.resize((size_t)z), zrc.assign((size_t)z, 0);
    hd.jpeg.resize((size_t)z), hd.png.resize((size_t)z), hd.tiff.resize((size_t)z), hd.kind.resize((size_t)z);
    for (int j = 0; j < z; j++) {
        const int k = idx[(size_t)(j0 + j)];
        zs[(size_t)j] = streams[k], zlen[(size_t)j] = len[k], hd.kind[(size_t)j] = src.kind[k];
        if (src.kind[k] == IMREAD_PNG) hd.png[(size_t)j] = src.png[k];
        else if (src.kind[k] == IMREAD_TIFF) hd.tiff[(size_t)j] = src.tiff[k];
        else hd.jpeg[(size_t)j] = src.jpeg[k];
    }
}

int omr::orient_device(const uint8_t *d_src, int64_t sstep, uint8_t *d_dst, int64_t dstep, int cn, std::vector<OrientImg> *recs,
                       hipStream_t s)
{
    const size_t n = recs->size();
    if (n == 0) return OMR_OK;
    DrainOnExit drain{s};  // the records' host copy and their device buffer stay until the stream has drained
    DevBuf d_recs;
    OMR_HIP(d_recs.alloc(sizeof(OrientImg) * n));
    for (size_t i0 = 0; i0 < n; i0 += 65535) {
        const int g = (int)std::min<size_t>(65535, n - i0);
        int max_tiles = 1;
        orient_plan(recs->data() + i0, g, cn, &max_tiles);
        OMR_HIP(hipMemcpyAsync(d_recs.as<OrientImg>() + i0, recs->data() + i0, sizeof(OrientImg) * (size_t)g, hipMemcpyHostToDevice, s));
        OMR_HIP(orient_launch(d_src, sstep, d_dst, dstep, cn, d_recs.as<OrientImg>() + i0, g, max_tiles, s));
    }
    OMR_HIP(hipStreamSynchronize(s));
    return OMR_OK;
}

int omr::imread_decode_device(const uint8_t *const *streams, const int64_t *len, const ImreadHeaders &hd, const int32_t *skip, int n,
                              int channels, bool ignore, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s)
{
    const JdecHeader *hdr = hd.jpeg;
    std::vector<int32_t> skip_jpeg((size_t)n, 1), skip_png((size_t)n, 1), skip_tiff((size_t)n, 1);
    std::vector<int> turn;
    int pngs = 0, tiffs = 0, direct = 0;
    for (int i = 0; i < n; i++) {
        if (skip && skip[i]) continue;
        if (hd.kind[i] == IMREAD_PNG) skip_png[(size_t)i] = 0, pngs++;
        else if (hd.kind[i] == IMREAD_TIFF) skip_tiff[(size_t)i] = 0, tiffs++;
        else if (!ignore && hdr[i].orient != 1) turn.push_back(i);
        else skip_jpeg[(size_t)i] = 0, direct++;
    }
    int r = OMR_OK;
    if (direct && (r = jpeg_decode_device(streams, len, hdr, skip_jpeg.data(), n, channels, d_out, out_stride, step, rc, s))) return r;
    if (pngs && (r = png_decode_device(streams, len, hd.png, skip_png.data(), n, channels, d_out, out_stride, step, rc, s))) return r;
    if (tiffs && (r = tiff_decode_device(streams, len, hd.tiff, skip_tiff.data(), n, channels, d_out, out_stride, step, rc, s))) return r;
    if (turn.empty()) return OMR_OK;

    // the members to turn, as a run of their own: decoded as stored into scratch slots that hold the largest of them
    const int m = (int)turn.size();
    int srows = 1, scols = 1;
    std::vector<const uint8_t *> ts((size_t)m);
    std::vector<int64_t> tlen((size_t)m);
    std::vector<JdecHeader> thdr((size_t)m);
    std::vector<int32_t> tskip((size_t)m, 0), trc((size_t)m, 0);
    for (int t = 0; t < m; t++) {
        const int i = turn[(size_t)t];
        ts[(size_t)t] = streams[i], tlen[(size_t)t] = len[i], thdr[(size_t)t] = hdr[i];
        srows = std::max(srows, hdr[i].rows), scols = std::max(scols, hdr[i].cols);
    }
    const int64_t tstep = ((int64_t)scols * channels + 3) & ~(int64_t)3, tstride = tstep * srows;
    DrainOnExit drain{s};
    DevBuf scratch;
    OMR_HIP(scratch.alloc((size_t)tstride * (size_t)m));
    if ((r = jpeg_decode_device(ts.data(), tlen.data(), thdr.data(), tskip.data(), m, channels, scratch.as<uint8_t>(), tstride, tstep,
                                trc.data(), s)))
        return r;
    std::vector<OrientImg> recs;
    for (int t = 0; t < m; t++) {
        const int i = turn[(size_t)t];
        if (trc[(size_t)t]) {  // damaged entropy data: the slot stays as it is
            rc[i] = trc[(size_t)t];
            continue;
        }
        recs.push_back(OrientImg{(int64_t)t * tstride, (int64_t)i * out_stride, hdr[i].rows, hdr[i].cols, hdr[i].orient, 0});
    }
    return orient_device(scratch.as<uint8_t>(), tstep, d_out, step, channels, &recs, s);
}

extern "C" {

int omr_orient_batch_device(const uint8_t *d_src, int64_t src_stride_bytes, int64_t src_step_bytes, int32_t rows, int32_t cols,
                            uint8_t *d_dst, int64_t dst_stride_bytes, int64_t dst_step_bytes, int32_t dst_rows, int32_t dst_cols,
                            int32_t channels, const int32_t *sizes, const int32_t *orient, int32_t n, int32_t *out_size)
{
    clear_error();
    if (n < 0) return fail(OMR_ERR_BADARG, "negative n");
    if (!orient || !out_size) return fail(OMR_ERR_BADARG, "null argument");
    if (int r = check_decoded_channels(channels)) return r;
    if (int r = check_slots(d_src, src_stride_bytes, src_step_bytes, rows, cols, channels, "source")) return r;
    if (int r = check_slots(d_dst, dst_stride_bytes, dst_step_bytes, dst_rows, dst_cols, channels, "destination")) return r;
    if (n == 0) return OMR_OK;
    std::vector<OrientImg> recs;
    for (int i = 0; i < n; i++) {
        const int r = sizes ? sizes[2 * (size_t)i] : rows, c = sizes ? sizes[2 * (size_t)i + 1] : cols;
        if (int e = check_code(orient[i])) return e;
        if (r < 0 || c < 0 || r > rows || c > cols || (r == 0) != (c == 0))
            return fail(OMR_ERR_BADARG, "image %d is %d x %d, its slot %d x %d", i, r, c, rows, cols);
        const bool t = orient_transposes(orient[i]);
        const int tr = t ? c : r, tc = t ? r : c;
        if (tr > dst_rows || tc > dst_cols)
            return fail(OMR_ERR_BADARG, "image %d is %d x %d after the turn, its destination slot %d x %d", i, tr, tc, dst_rows, dst_cols);
        if (r) recs.push_back(OrientImg{(int64_t)i * src_stride_bytes, (int64_t)i * dst_stride_bytes, r, c, orient[i], 0});
    }
    // out of place only: the bytes the slots span must not meet
    const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
    const uint64_t sext = (uint64_t)(n - 1) * (uint64_t)src_stride_bytes + (uint64_t)(rows - 1) * (uint64_t)src_step_bytes + (uint64_t)cols * channels;
    const uint64_t dext = (uint64_t)(n - 1) * (uint64_t)dst_stride_bytes + (uint64_t)(dst_rows - 1) * (uint64_t)dst_step_bytes + (uint64_t)dst_cols * channels;
    if (s0 < d0 + dext && d0 < s0 + sext) return fail(OMR_ERR_BADARG, "the source and destination slots overlap (out of place only)");
    for (int i = 0; i < n; i++) {
        const int r = sizes ? sizes[2 * (size_t)i] : rows, c = sizes ? sizes[2 * (size_t)i + 1] : cols;
        const bool t = orient_transposes(orient[i]);
        out_size[2 * (size_t)i] = t ? c : r, out_size[2 * (size_t)i + 1] = t ? r : c;
    }
    if (recs.empty()) return OMR_OK;
    if (int r = have_device()) return r;
    LeasedStream st;
    if (int r = st.create()) return r;
    return orient_device(d_src, src_step_bytes, d_dst, dst_step_bytes, channels, &recs, st.s);
}

int omr_orient(const omr_image *src, int32_t orientation, omr_image_owned *dst)
{
    clear_error();
    if (!dst) return fail(OMR_ERR_BADARG, "null argument");
    int r = check_image(src, cn_orient);
    if (r || (r = check_code(orientation))) return r;
    if ((r = have_device())) return r;
    LeasedStream st;
    if ((r = st.create())) return r;
    const int cn = src->channels;
    const bool t = orient_transposes(orientation);
    const int trows = t ? src->cols : src->rows, tcols = t ? src->rows : src->cols;
    const int64_t sstep = (int64_t)src->cols * cn, dstep = (int64_t)tcols * cn, bytes = sstep * src->rows;
    DrainOnExit drain{st.s};
    DevBuf in, out;
    OMR_HIP(in.alloc((size_t)bytes));
    OMR_HIP(out.alloc((size_t)bytes));
    if ((r = upload_rows(in.p, (size_t)sstep, src->data, (size_t)src->step_bytes, (size_t)sstep, (size_t)src->rows, st.s))) return r;
    std::vector<OrientImg> recs{OrientImg{0, 0, src->rows, src->cols, orientation, 0}};
    if ((r = orient_device(in.as<uint8_t>(), sstep, out.as<uint8_t>(), dstep, cn, &recs, st.s))) return r;
    *dst = omr_image_owned{nullptr, trows, tcols, cn, dstep};
    dst->data = (uint8_t *)malloc((size_t)bytes);
    if (!dst->data) return fail(OMR_ERR_NOMEM, "out of host memory");
    r = staged_d2h(dst->data, out.p, (size_t)bytes, st.s);
    if (r) omr_image_free(dst);
    return r;
}

int omr_imread_info(const uint8_t *stream, int64_t len, int32_t flags, int32_t *rows, int32_t *cols, int32_t *components,
                    int32_t *orientation, int32_t *kind)
{
    clear_error();
    if (!stream || len < 0) return fail(OMR_ERR_BADARG, "null stream");
    if (int r = check_flags(flags)) return r;
    ImreadRun run;
    const ImreadParsed p = run.append(stream, len, 0, (flags & OMR_IMREAD_IGNORE_ORIENTATION) != 0);
    if (rows) *rows = p.rows;
    if (cols) *cols = p.cols;
    if (components) *components = p.components;
    if (orientation) *orientation = p.orient;
    if (kind) *kind = p.kind;
    return p.rc;
}

int omr_imread_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels, int32_t flags,
                            uint8_t *d_out, int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                            int32_t *out_size, int32_t *rc)
{
    const bool ignore = (flags & OMR_IMREAD_IGNORE_ORIENTATION) != 0;
    ImreadRun run;
    return decode_batch_entry(
        BatchDecodeArgs{streams, len, n, channels, d_out, out_stride_bytes, step_bytes, rows, cols, out_size, rc},
        "stream %d is %d x %d as imread returns it, the slot %d x %d", [&] { return check_flags(flags); }, [&](size_t cnt) { run.reserve(cnt); },
        [&](int i) {
            const ImreadParsed p = run.append(streams[i], len[i], channels, ignore);
            return ParsedSize{p.rc, p.rows, p.cols};
        },
        [&](const int32_t *skip, hipStream_t s) {
            return imread_decode_device(streams, len, run.view(), skip, n, channels, ignore, d_out, out_stride_bytes, step_bytes, rc, s);
        });
}

int omr_imread(const uint8_t *stream, int64_t len, int32_t channels, int32_t flags, omr_image_owned *dst)
{
    const bool ignore = (flags & OMR_IMREAD_IGNORE_ORIENTATION) != 0;
    ImreadRun run;
    return decode_one_entry(
        stream, len, channels, dst,
        "the image data is damaged (what its decoder, omr_jpeg_decode, omr_png_decode or omr_tiff_decode, reports as OMR_ERR_ASSERT)",
        [&] { return check_flags(flags); },
        [&] {
            const ImreadParsed p = run.append(stream, len, channels, ignore);
            return ParsedSize{p.rc, p.rows, p.cols};
        },
        [&](uint8_t *d_out, int64_t stride, int64_t step, int32_t *rc, hipStream_t s) {
            return imread_decode_device(&stream, &len, run.view(), nullptr, 1, channels, ignore, d_out, stride, step, rc, s);
        });
}

}  // extern "C"
