// oics_png_dec.cpp -- host side of the PNG decoder (png_dec.hip): the chunk walk with what it
// refuses, the CRC-32 of the critical chunks (checked while the IDAT pieces are gathered for the upload, on the host's
// threads), the launches of a group and the entry points omr_png_info / omr_png_decode*.  The host visits the chunk
// headers, IHDR and PLTE only; everything inside IDAT is the device's.
//
// The decoder refuses a little more than libpng, which warns and carries on where this one answers OMR_ERR_ASSERT: inflated
// data longer than the image needs, a wrong Adler-32, a wrong CRC of a critical chunk, a missing IEND, a palette index
// beyond PLTE.  Bytes behind the zlib stream's trailer inside IDAT are ignored, as zlib does.  A refused file goes to the
// host codec.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "host_threads.hpp"
#include "png_dec.hpp"

using namespace omr;

namespace {

const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};

// CRC-32 (ISO 3309, as PNG uses it), eight bytes a step
struct CrcTables {
    uint32_t t[8][256];
    CrcTables()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (int j = 1; j < 8; j++)
            for (uint32_t i = 0; i < 256; i++) t[j][i] = t[0][t[j - 1][i] & 255] ^ (t[j - 1][i] >> 8);
    }
};

uint32_t crc32(const uint8_t *p, size_t n)
{
    static const CrcTables T;
    uint32_t c = 0xffffffffu;
    for (; n >= 8; n -= 8, p += 8) {
        const uint32_t a = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        c = T.t[7][a & 255] ^ T.t[6][(a >> 8) & 255] ^ T.t[5][(a >> 16) & 255] ^ T.t[4][a >> 24] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^
            T.t[1][p[6]] ^ T.t[0][p[7]];
    }
    for (; n; n--, p++) c = T.t[0][(c ^ *p) & 255] ^ (c >> 8);
    return ~c;
}

uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

int samples_of(int color_type) { return color_type == 0 ? 1 : color_type == 2 ? 3 : color_type == 3 ? 1 : color_type == 4 ? 2 : 4; }

int64_t row_bytes_of(const PdecHeader &h) { return ((int64_t)h.cols * samples_of(h.color_type) * h.depth + 7) / 8; }

constexpr int64_t kGroupRaw = (int64_t)4 << 30;  // inflated bytes of one group of launches: 160 A4 colour images, an image per CU
constexpr int64_t kGroupBytes = (int64_t)2 << 30;  // zlib streams of one group
constexpr int kGroupImages = 4096;

// one group: images idx[0 .. g)
int decode_group(const uint8_t *const *streams, const PdecHeader *hdr, const int *idx, int g, int channels, uint8_t *d_out,
                 int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s)
{
    // the host objects that asynchronous copies read or write stand before the drain
    std::vector<PdecImg> im((size_t)g);
    std::vector<PdecDyn> dyn((size_t)g);
    std::vector<uint8_t> host;
    DrainOnExit drain{s};
    StageTimer<PDEC_STAGES> ev;
    if (int r = ev.begin(pdec_stats().on)) return r;
    size_t src_bytes = 0, raw_bytes = 0;
    int max_chunks = 1;
    for (int j = 0; j < g; j++) {
        const int i = idx[j];
        const PdecHeader &h = hdr[i];
        PdecImg &m = im[(size_t)j];
        memset(&m, 0, sizeof m);
        m.src_off = (int64_t)src_bytes, m.src_len = (uint32_t)h.idat_bytes;
        src_bytes += up16(m.src_len);
        m.row_bytes = (int32_t)row_bytes_of(h);
        m.raw_len = (uint32_t)((int64_t)h.rows * (1 + (int64_t)m.row_bytes));
        m.raw_off = (int64_t)raw_bytes;
        raw_bytes += up16(m.raw_len);
        m.out_off = (int64_t)i * out_stride;
        m.rows = h.rows, m.cols = h.cols, m.color_type = h.color_type, m.depth = h.depth;
        m.bpp = std::max(1, samples_of(h.color_type) * h.depth / 8);
        m.npal = h.npal;
        memcpy(m.pal, h.pal, sizeof m.pal);
        max_chunks = std::max(max_chunks, (int)(((int64_t)m.raw_len + PDEC_ADLER_CHUNK - 1) / PDEC_ADLER_CHUNK));
    }
    // the zlib streams of the group, gathered piece by piece with the CRC of every critical chunk checked on the way
    host.resize(src_bytes);
    int r = on_threads(g, [&](hipStream_t, int lo, int hi) -> int {
        for (int j = lo; j < hi; j++) {
            const uint8_t *st = streams[idx[j]];
            const PdecHeader &h = hdr[idx[j]];
            uint8_t *to = host.data() + im[(size_t)j].src_off;
            for (const PdecPiece &pc : h.idat) memcpy(to, st + pc.off, pc.len), to += pc.len;
            for (const PdecPiece &c : h.critical)
                if (crc32(st + c.off, c.len) != be32(st + c.off + c.len)) im[(size_t)j].skip = 1;
        }
        return OMR_OK;
    });
    if (r) return r;
    DevBuf d_src, d_im, d_dyn, raw;
    OMR_HIP(d_src.alloc(std::max<size_t>(src_bytes, 16)));
    OMR_HIP(d_im.alloc(sizeof(PdecImg) * (size_t)g));
    OMR_HIP(d_dyn.alloc(sizeof(PdecDyn) * (size_t)g));
    OMR_HIP(raw.alloc(std::max<size_t>(raw_bytes, 16)));
    PdecPass p;
    memset(&p, 0, sizeof p);
    p.src = d_src.as<uint8_t>(), p.imgs = d_im.as<PdecImg>(), p.dyn = d_dyn.as<PdecDyn>(), p.raw = raw.as<uint8_t>();
    p.n = g, p.channels = channels, p.out = d_out, p.step = step;
    if ((r = ev.mark(0, s))) return r;
    if (src_bytes) OMR_HIP(hipMemcpyAsync(d_src.p, host.data(), src_bytes, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(PdecImg) * (size_t)g, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemsetAsync(d_dyn.p, 0, sizeof(PdecDyn) * (size_t)g, s));
    if ((r = ev.mark(1, s)) || (r = pdec_launch_inflate(p, s)) || (r = ev.mark(2, s)) || (r = pdec_launch_adler(p, max_chunks, s)) ||
        (r = ev.mark(3, s)) || (r = pdec_launch_unfilter(p, s)) || (r = ev.mark(4, s)))
        return r;
    OMR_HIP(hipMemcpyAsync(dyn.data(), d_dyn.p, sizeof(PdecDyn) * (size_t)g, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    if ((r = ev.finish(pdec_stats()))) return r;
    for (int j = 0; j < g; j++)
        if (im[(size_t)j].skip || dyn[(size_t)j].err) rc[idx[j]] = OMR_ERR_ASSERT;
    return OMR_OK;
}

}  // namespace

bool omr::pdec_is_png(const uint8_t *s, int64_t len) { return len >= 8 && !memcmp(s, kSignature, 8); }

int omr::pdec_parse(const uint8_t *s, int64_t len, PdecHeader *h)
{
    h->rows = h->cols = h->color_type = h->depth = h->npal = 0;
    h->orient = 1;
    h->idat.clear(), h->critical.clear(), h->idat_bytes = 0;
    memset(h->pal, 0, sizeof h->pal);
    if (!pdec_is_png(s, len)) return fail(OMR_ERR_BADARG, "not a PNG stream: no signature");
    bool have_ihdr = false, have_plte = false, have_iend = false, apng = false, idat_open = false;
    int interlace = 0, orient = 1;
    int64_t p = 8;
    while (p < len) {
        if (p + 12 > len) return fail(OMR_ERR_BADARG, "the chunk at byte %lld runs past the end", (long long)p);
        const int64_t n = be32(s + p);
        const uint8_t *type = s + p + 4, *body = s + p + 8;
        if (p + 12 + n > len) return fail(OMR_ERR_BADARG, "the chunk at byte %lld runs past the end", (long long)p);
        const bool is_ihdr = !memcmp(type, "IHDR", 4), is_idat = !memcmp(type, "IDAT", 4);
        if (!have_ihdr && !is_ihdr) return fail(OMR_ERR_BADARG, "IHDR is not the first chunk");
        if (!(type[0] & 0x20)) h->critical.push_back(PdecPiece{p + 4, (uint32_t)(4 + n)});
        if (!is_idat && !h->idat.empty()) idat_open = false;
        if (is_ihdr) {
            if (have_ihdr || n != 13) return fail(OMR_ERR_BADARG, "malformed IHDR");
            have_ihdr = true;
            const uint32_t w = be32(body), hh = be32(body + 4);
            const int d = body[8], ct = body[9];
            if (w == 0 || hh == 0 || w > 0x7fffffffu || hh > 0x7fffffffu) return fail(OMR_ERR_BADARG, "an image size of 0 (or above 2^31 - 1)");
            const bool pair = ct == 0   ? d == 1 || d == 2 || d == 4 || d == 8 || d == 16
                              : ct == 3 ? d == 1 || d == 2 || d == 4 || d == 8
                                        : (ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16);
            if (!pair) return fail(OMR_ERR_BADARG, "bit depth %d does not go with colour type %d", d, ct);
            if (body[10] != 0 || body[11] != 0 || body[12] > 1) return fail(OMR_ERR_BADARG, "malformed IHDR");
            h->rows = (int32_t)hh, h->cols = (int32_t)w, h->color_type = ct, h->depth = d, interlace = body[12];
        } else if (!memcmp(type, "PLTE", 4)) {
            if (n == 0 || n % 3 || n > 768 || have_plte || !h->idat.empty()) return fail(OMR_ERR_BADARG, "malformed PLTE");
            have_plte = true, h->npal = (int32_t)(n / 3);
            memcpy(h->pal, body, (size_t)n);
        } else if (is_idat) {
            if (!h->idat.empty() && !idat_open) return fail(OMR_ERR_BADARG, "IDAT chunks that are not consecutive");
            idat_open = true;
            h->idat.push_back(PdecPiece{p + 8, (uint32_t)n}), h->idat_bytes += n;
        } else if (!memcmp(type, "IEND", 4)) {
            have_iend = true;
            break;
        } else if (!(type[0] & 0x20)) {
            return fail(OMR_ERR_BADARG, "unknown critical chunk %.4s", (const char *)type);
        } else if (!memcmp(type, "acTL", 4)) {
            if (h->idat.empty()) apng = true;
        } else if (!memcmp(type, "eXIf", 4)) {
            const int o = exif_orientation_tiff(body, n);
            if (o != 1) orient = o;
        }
        p += 12 + n;
    }
    h->orient = orient;
    if (!have_ihdr) return fail(OMR_ERR_BADARG, "no IHDR");
    if (h->idat.empty()) return fail(OMR_ERR_BADARG, "no IDAT");
    if (h->color_type == 3 && !have_plte) return fail(OMR_ERR_BADARG, "a paletted image without PLTE");
    uint8_t z[2];
    int nz = 0;
    for (const PdecPiece &pc : h->idat)
        for (uint32_t k = 0; k < pc.len && nz < 2; k++) z[nz++] = s[pc.off + k];
    if (nz < 2 || (z[0] & 15) != 8 || (z[0] >> 4) > 7 || (z[1] & 0x20) || (z[0] << 8 | z[1]) % 31)
        return fail(OMR_ERR_BADARG, "bad zlib header");
    if (interlace) return fail(OMR_ERR_NOTIMPL, "Adam7 interlace is not implemented");
    if (h->depth == 16) return fail(OMR_ERR_NOTIMPL, "16-bit samples are not implemented");
    if (apng) return fail(OMR_ERR_NOTIMPL, "animated PNG (acTL) is not implemented");
    if (orient != 1) return fail(OMR_ERR_NOTIMPL, "EXIF orientation %d is not implemented (imread would turn the image)", orient);
    if (!have_iend) return fail(OMR_ERR_ASSERT, "no IEND: the stream is cut short");
    // OpenCV's imread fails above these (CV_IO_MAX_IMAGE_WIDTH / _HEIGHT / _PIXELS); they also keep a row's bytes, a
    // pixel's byte offset in its output row and every count of the kernels inside 32 bits
    if (h->cols > PDEC_MAX_SIDE || h->rows > PDEC_MAX_SIDE || (int64_t)h->rows * h->cols > PDEC_MAX_PIXELS)
        return fail(OMR_ERR_ASSERT, "%d x %d is above imread's limits (2^20 a side, 2^30 pixels): not supported", h->rows, h->cols);
    if ((int64_t)h->rows * (1 + row_bytes_of(*h)) >= ((int64_t)1 << 32))
        return fail(OMR_ERR_ASSERT, "raw data of 2^32 bytes or more: not supported");
    if (h->idat_bytes >= ((int64_t)1 << 28)) return fail(OMR_ERR_ASSERT, "IDAT data of 2^28 bytes or more: not supported");
    return OMR_OK;
}

int omr::pdec_check_channels(const PdecHeader &h, int channels)
{
    if (channels == 1 && h.color_type != 0 && h.color_type != 4)
        return fail(OMR_ERR_NOTIMPL, "a gray image from a colour or paletted stream is not implemented (libpng's rgb_to_gray is not cvtColor's)");
    return OMR_OK;
}

PdecStats &omr::pdec_stats() { return thread_stats<PdecStats>(); }

int omr::png_decode_device(const uint8_t *const *streams, const int64_t *, const PdecHeader *hdr, const int32_t *skip, int n,
                           int channels, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s)
{
    pdec_stats().begin_call();
    DrainOnExit drain{s};
    return for_each_group(
        n, skip, kGroupImages, kGroupRaw, kGroupBytes,
        [&](int i) { return GroupCost{(int64_t)hdr[i].rows * (1 + row_bytes_of(hdr[i])), hdr[i].idat_bytes, true}; },
        [&](const int *idx, int g) { return decode_group(streams, hdr, idx, g, channels, d_out, out_stride, step, rc, s); });
}

extern "C" {

int omr_png_info(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *color_type, int32_t *bit_depth)
{
    clear_error();
    if (!stream || len < 0) return fail(OMR_ERR_BADARG, "null stream");
    PdecHeader h;
    const int rc = pdec_parse(stream, len, &h);
    if (rows) *rows = h.rows;
    if (cols) *cols = h.cols;
    if (color_type) *color_type = h.color_type;
    if (bit_depth) *bit_depth = h.depth;
    return rc;
}

int omr_png_decode_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels, uint8_t *d_out,
                                int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols, int32_t *out_size,
                                int32_t *rc)
{
    std::vector<PdecHeader> hdr;
    return decode_batch_entry(
        BatchDecodeArgs{streams, len, n, channels, d_out, out_stride_bytes, step_bytes, rows, cols, out_size, rc},
        "stream %d is %d x %d, the slot %d x %d", no_extra_check, [&](size_t cnt) { hdr.reserve(cnt); },
        [&](int i) {
            hdr.emplace_back();
            int r = pdec_parse(streams[i], len[i], &hdr.back());
            if (r == OMR_OK) r = pdec_check_channels(hdr.back(), channels);
            return ParsedSize{r, hdr.back().rows, hdr.back().cols};
        },
        [&](const int32_t *skip, hipStream_t s) {
            return png_decode_device(streams, len, hdr.data(), skip, n, channels, d_out, out_stride_bytes, step_bytes, rc, s);
        });
}

int omr_png_decode_stats(int32_t enable, int32_t *groups, double *stage_ms)
{
    clear_error();
    pdec_stats().report(enable, groups, stage_ms);
    return OMR_OK;
}

int omr_png_decode(const uint8_t *stream, int64_t len, int32_t channels, omr_image_owned *dst)
{
    PdecHeader h;
    const int32_t skip = 0;
    return decode_one_entry(
        stream, len, channels, dst,
        "the image data is damaged (a chunk's CRC, the deflate stream, its Adler-32 or size, a filter byte or a palette index)", no_extra_check,
        [&] {
            int r = pdec_parse(stream, len, &h);
            if (r == OMR_OK) r = pdec_check_channels(h, channels);
            return ParsedSize{r, h.rows, h.cols};
        },
        [&](uint8_t *d_out, int64_t stride, int64_t step, int32_t *rc, hipStream_t s) {
            return png_decode_device(&stream, &len, &h, &skip, 1, channels, d_out, stride, step, rc, s);
        });
}

}  // extern "C"
