// oics_jpeg_dec.cpp -- host side of the JPEG decoder (jpeg_dec.hip): the marker parser with what it
// refuses, the code tables as the kernels look them up, the launches of a group and the entry points omr_jpeg_info /
// omr_jpeg_decode*.  The host visits the headers only; everything behind SOS is the device's.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "jpeg_dec.hpp"
#include "png_dec.hpp"

using namespace omr;

namespace {

struct Dht {
    bool set = false;
    uint8_t bits[16];
    uint8_t vals[256];
    int nval = 0;
};

// jdhuff.c's jpeg_make_d_derived_tbl, with a 9-bit first level
void derive(const Dht &h, JdecHuff *t)
{
    memset(t, 0, sizeof *t);
    memcpy(t->vals, h.vals, 256);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; len++) {
        t->valoff[len] = k - code;
        for (int i = 0; i < h.bits[len - 1]; i++, k++, code++) {
            if (len <= 9)
                for (int f = 0; f < (1 << (9 - len)); f++) t->look[(code << (9 - len)) | f] = (uint16_t)(len << 8 | h.vals[k]);
        }
        t->maxcode[len] = h.bits[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[0] = -1, t->valoff[0] = 0;
}

// the EXIF orientation of an APP1 body, or 1
int exif_orientation(const uint8_t *b, int64_t n)
{
    if (n < 14 || memcmp(b, "Exif\0\0", 6)) return 1;
    return exif_orientation_tiff(b + 6, n - 6);
}

constexpr int64_t kGroupBlocks = 4 << 20;     // blocks of one group of launches: 512 MB of coefficients
constexpr int64_t kGroupBytes = 256 << 20;    // entropy data of one group
constexpr int kGroupImages = 4096;

int64_t blocks_of(const JdecHeader &h)
{
    const int64_t mw = (h.cols + 8 * h.hs - 1) / (8 * h.hs), mh = (h.rows + 8 * h.vs - 1) / (8 * h.vs);
    return mw * mh * (h.hs * h.vs + (h.ncomp == 3 ? 2 : 0));
}

// one group: images idx[0 .. g)
int decode_group(const uint8_t *const *streams, const int64_t *len, const JdecHeader *hdr, const int *idx, int g, int channels,
                 uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s)
{
    // the host objects that asynchronous copies read or write stand before the drain: on every return path, the error
    // ones included, the stream has drained before they go
    std::vector<JdecImg> im((size_t)g);
    std::vector<JdecTables> tabs((size_t)g);
    std::vector<JdecDyn> dyn((size_t)g);
    std::vector<uint8_t> host;
    uint32_t h_changed = 0;
    DrainOnExit drain{s};
    JdecStats &stats = jdec_stats();
    StageTimer<JDEC_STAGES> ev;
    if (int r = ev.begin(stats.on)) return r;
    size_t src_bytes = 0, bit_bytes = 0, plane_bytes = 0;
    uint32_t blocks = 0, ivals = 0, subs = 0, chunks = 0, max_blocks = 1;
    int max_chunks = 1, max_groups = 1, max_rows = 1, max_cols = 1;
    for (int j = 0; j < g; j++) {
        const int i = idx[j];
        const JdecHeader &h = hdr[i];
        JdecImg &m = im[(size_t)j];
        memset(&m, 0, sizeof m);
        tabs[(size_t)j] = h.tab;
        m.src_off = (int64_t)src_bytes, m.src_len = (uint32_t)(len[i] - h.data);
        src_bytes += up16(m.src_len);
        m.bit_off = (int64_t)bit_bytes;
        bit_bytes += up16((size_t)m.src_len + JDEC_PAD);
        m.out_off = (int64_t)i * out_stride;
        m.rows = h.rows, m.cols = h.cols, m.ncomp = h.ncomp, m.hs = h.hs, m.vs = h.vs, m.ri = h.ri;
        m.mw = (h.cols + 8 * h.hs - 1) / (8 * h.hs), m.mh = (h.rows + 8 * h.vs - 1) / (8 * h.vs);
        m.bpm = h.hs * h.vs + (h.ncomp == 3 ? 2 : 0);
        m.nmcu = (uint32_t)m.mw * (uint32_t)m.mh, m.nblk = m.nmcu * (uint32_t)m.bpm;
        m.blk0 = blocks, blocks += m.nblk;
        m.nival = h.ri ? (m.nmcu + (uint32_t)h.ri - 1) / (uint32_t)h.ri : 1;
        m.ival0 = ivals, ivals += m.nival + 1;
        m.sub_cap = (uint32_t)(((uint64_t)m.src_len * 8 + JDEC_SUB_BITS - 1) / JDEC_SUB_BITS) + m.nival;
        m.sub0 = subs, subs += m.sub_cap;
        m.nchunk = (m.src_len + JDEC_BYTE_CHUNK - 1) / JDEC_BYTE_CHUNK;
        m.chunk0 = chunks, chunks += m.nchunk;
        m.ypitch = m.mw * h.hs * 8, m.cpitch = m.mw * 8;
        m.plane_off[0] = (int64_t)plane_bytes;
        plane_bytes += up16((size_t)m.ypitch * (size_t)(m.mh * h.vs * 8));
        for (int c = 1; c < h.ncomp; c++) {
            m.plane_off[c] = (int64_t)plane_bytes;
            plane_bytes += up16((size_t)m.cpitch * (size_t)(m.mh * 8));
        }
        max_chunks = std::max(max_chunks, (int)m.nchunk);
        max_groups = std::max(max_groups, (int)((m.sub_cap + JDEC_LANES - 1) / JDEC_LANES));
        max_blocks = std::max(max_blocks, m.nblk);
        max_rows = std::max(max_rows, h.rows), max_cols = std::max(max_cols, h.cols);
    }
    // the entropy data of the group, gathered and uploaded in one copy
    host.resize(src_bytes);
    for (int j = 0; j < g; j++) memcpy(host.data() + im[(size_t)j].src_off, streams[idx[j]] + hdr[idx[j]].data, im[(size_t)j].src_len);
    DevBuf d_src, d_im, d_tab, d_dyn, ck, cr, ce, co, cro, bitbuf, ist, isub, state, scnt, sex, chg, changed, coef, planes;
    OMR_HIP(d_src.alloc(src_bytes));
    OMR_HIP(d_im.alloc(sizeof(JdecImg) * (size_t)g));
    OMR_HIP(d_tab.alloc(sizeof(JdecTables) * (size_t)g));
    OMR_HIP(d_dyn.alloc(sizeof(JdecDyn) * (size_t)g));
    OMR_HIP(ck.alloc((size_t)chunks * 4));
    OMR_HIP(cr.alloc((size_t)chunks * 4));
    OMR_HIP(ce.alloc((size_t)chunks * 4));
    OMR_HIP(co.alloc((size_t)chunks * 4));
    OMR_HIP(cro.alloc((size_t)chunks * 4));
    OMR_HIP(bitbuf.alloc(bit_bytes));
    OMR_HIP(ist.alloc((size_t)ivals * 4));
    OMR_HIP(isub.alloc((size_t)ivals * 4));
    OMR_HIP(state.alloc((size_t)subs * 8));
    OMR_HIP(scnt.alloc((size_t)subs * 16));
    OMR_HIP(sex.alloc((size_t)subs * 16));
    OMR_HIP(chg.alloc((size_t)subs * 2));
    OMR_HIP(changed.alloc(4));
    OMR_HIP(coef.alloc((size_t)blocks * 128));
    OMR_HIP(planes.alloc(plane_bytes));
    JdecPass p;
    memset(&p, 0, sizeof p);
    p.src = d_src.as<uint8_t>(), p.imgs = d_im.as<JdecImg>(), p.tabs = d_tab.as<JdecTables>(), p.dyn = d_dyn.as<JdecDyn>();
    p.n = g, p.channels = channels;
    p.chunk_keep = ck.as<uint32_t>(), p.chunk_rst = cr.as<uint32_t>(), p.chunk_end = ce.as<uint32_t>();
    p.chunk_off = co.as<uint32_t>(), p.chunk_rst_off = cro.as<uint32_t>();
    p.bitbuf = bitbuf.as<uint8_t>(), p.ival_start = ist.as<uint32_t>(), p.ival_sub0 = isub.as<uint32_t>();
    p.state = state.as<uint64_t>(), p.sub_cnt = scnt.as<uint32_t>(), p.sub_ex = sex.as<uint32_t>();
    p.chg = chg.as<uint8_t>(), p.sub_total = subs, p.changed = changed.as<uint32_t>();
    p.coef = coef.as<int16_t>(), p.planes = planes.as<uint8_t>(), p.out = d_out, p.step = step;
    int r = ev.mark(0, s);
    if (r) return r;
    OMR_HIP(hipMemcpyAsync(d_src.p, host.data(), src_bytes, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(JdecImg) * (size_t)g, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemcpyAsync(d_tab.p, tabs.data(), sizeof(JdecTables) * (size_t)g, hipMemcpyHostToDevice, s));
    OMR_HIP(hipMemsetAsync(d_dyn.p, 0, sizeof(JdecDyn) * (size_t)g, s));
    OMR_HIP(hipMemsetAsync(bitbuf.p, 0, bit_bytes, s));
    OMR_HIP(hipMemsetAsync(coef.p, 0, (size_t)blocks * 128, s));
    OMR_HIP(hipMemsetAsync(chg.p, 0, (size_t)subs * 2, s));
    if ((r = ev.mark(1, s)) || (r = jdec_launch_unstuff(p, max_chunks, s)) || (r = ev.mark(2, s))) return r;
    // rounds until one changes nothing: after round k the first k subsequences of every interval stand, so the number of
    // subsequences bounds the rounds
    uint32_t round = 0;
    for (;; round++) {
        if (round > subs + 1) return fail(OMR_ERR_GPU, "the JPEG decoder's rounds did not end");
        if (round > 0) OMR_HIP(hipMemsetAsync(changed.p, 0, 4, s));
        if ((r = jdec_launch_sync(p, (int)round, max_groups, s))) return r;
        if (round == 0) continue;
        OMR_HIP(hipMemcpyAsync(&h_changed, changed.p, 4, hipMemcpyDeviceToHost, s));
        OMR_HIP(hipStreamSynchronize(s));
        if (h_changed == 0) break;
    }
    if ((r = ev.mark(3, s)) || (r = jdec_launch_finish(p, max_groups, max_blocks, max_rows, max_cols, s, ev.from(4))) || (r = ev.mark(6, s)))
        return r;
    OMR_HIP(hipMemcpyAsync(dyn.data(), d_dyn.p, sizeof(JdecDyn) * (size_t)g, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    if (stats.on) stats.rounds = std::max(stats.rounds, (int32_t)round + 1);
    if ((r = ev.finish(stats))) return r;
    for (int j = 0; j < g; j++)
        if (dyn[(size_t)j].err) rc[idx[j]] = OMR_ERR_ASSERT;
    return OMR_OK;
}

}  // namespace

int omr::jdec_parse(const uint8_t *s, int64_t len, JdecHeader *h, bool refuse_orientation)
{
    h->rows = h->cols = h->ncomp = h->hs = h->vs = h->ri = 0;
    h->orient = 1;
    h->data = 0;
    if (len < 4 || s[0] != 0xFF || s[1] != 0xD8) return fail(OMR_ERR_BADARG, "not a JPEG stream: no SOI");
    uint8_t qt[4][64];
    bool qt_set[4] = {false, false, false, false};
    Dht dht[2][4];
    bool jfif = false, adobe = false, have_frame = false;
    int orient = 1, nf = 0;
    uint8_t frame[4][4];  // id, h, v, tq
    const uint8_t *body = nullptr;
    int64_t blen = 0, p = 2;
    for (;;) {
        if (p + 4 > len) return fail(OMR_ERR_BADARG, "the stream ends before SOS");
        if (s[p] != 0xFF) return fail(OMR_ERR_BADARG, "no marker at byte %lld", (long long)p);
        const int m = s[p + 1];
        if (m == 0xFF) {
            p += 1;
            continue;
        }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {
            p += 2;
            continue;
        }
        if (m == 0xD9) return fail(OMR_ERR_BADARG, "EOI before SOS");
        const int64_t n = s[p + 2] << 8 | s[p + 3];
        if (n < 2 || p + 2 + n > len) return fail(OMR_ERR_BADARG, "the segment at byte %lld runs past the end", (long long)p);
        body = s + p + 4, blen = n - 2;
        p += 2 + n;
        if (m == 0xDB) {
            for (int64_t q = 0; q < blen; q += 65) {
                if (body[q] >> 4) return fail(OMR_ERR_NOTIMPL, "16-bit quantisation tables are not implemented");
                const int tq = body[q] & 15;
                if (tq > 3 || q + 65 > blen) return fail(OMR_ERR_BADARG, "malformed DQT");
                memcpy(qt[tq], body + q + 1, 64), qt_set[tq] = true;
            }
        } else if (m == 0xC4) {
            for (int64_t q = 0; q < blen;) {
                if (q + 17 > blen) return fail(OMR_ERR_BADARG, "malformed DHT");
                const int tc = body[q] >> 4, th = body[q] & 15;
                int nv = 0;
                for (int i = 0; i < 16; i++) nv += body[q + 1 + i];
                if (tc > 1 || th > 3 || nv > 256 || q + 17 + nv > blen) return fail(OMR_ERR_BADARG, "malformed DHT");
                int code = 0;
                for (int i = 0; i < 16; i++) {  // the code space must not overflow
                    code = (code + body[q + 1 + i]) << 1;
                    if (code > (2 << (i + 1))) return fail(OMR_ERR_BADARG, "malformed DHT: too many codes");
                }
                Dht &d = dht[tc][th];
                d.set = true, d.nval = nv;
                memcpy(d.bits, body + q + 1, 16);
                memset(d.vals, 0, 256);
                memcpy(d.vals, body + q + 17, (size_t)nv);
                q += 17 + nv;
            }
        } else if (m == 0xC0 || (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
            if (have_frame) return fail(OMR_ERR_BADARG, "two frame headers");
            if (blen < 6) return fail(OMR_ERR_BADARG, "malformed SOF");
            h->rows = body[1] << 8 | body[2], h->cols = body[3] << 8 | body[4];
            nf = body[5];
            if (m != 0xC0) return fail(OMR_ERR_NOTIMPL, "frame type SOF%d is not implemented (baseline SOF0 only)", m - 0xC0);
            if (body[0] != 8) return fail(OMR_ERR_NOTIMPL, "%d-bit samples are not implemented", body[0]);
            if (blen != 6 + 3 * (int64_t)nf) return fail(OMR_ERR_BADARG, "malformed SOF");
            if (h->cols == 0) return fail(OMR_ERR_BADARG, "an image size of 0");
            if (nf <= 4)
                for (int i = 0; i < nf; i++) {
                    frame[i][0] = body[6 + 3 * i], frame[i][1] = body[7 + 3 * i] >> 4, frame[i][2] = body[7 + 3 * i] & 15;
                    frame[i][3] = body[8 + 3 * i];
                }
            have_frame = true;
        } else if (m == 0xCC) {
            return fail(OMR_ERR_NOTIMPL, "arithmetic coding is not implemented");
        } else if (m == 0xDC) {
            return fail(OMR_ERR_NOTIMPL, "DNL is not implemented");
        } else if (m == 0xDD) {
            if (blen != 2) return fail(OMR_ERR_BADARG, "malformed DRI");
            h->ri = body[0] << 8 | body[1];
        } else if (m == 0xE0) {
            if (blen >= 14 && !memcmp(body, "JFIF\0", 5)) jfif = true;
        } else if (m == 0xE1) {
            const int o = exif_orientation(body, blen);
            if (o != 1) orient = o;
        } else if (m == 0xEE) {
            if (blen >= 12 && !memcmp(body, "Adobe", 5)) adobe = true;
        } else if (m == 0xDA) {
            break;
        }
    }
    if (!have_frame) return fail(OMR_ERR_BADARG, "SOS before SOF");
    if (h->rows == 0) return fail(OMR_ERR_BADARG, "an image size of 0");
    if (nf != 1 && nf != 3) return fail(OMR_ERR_NOTIMPL, "%d components are not implemented (1 or 3)", nf);
    const int ns = blen ? body[0] : 0;
    if (blen != 4 + 2 * (int64_t)ns || ns < 1 || ns > 4) return fail(OMR_ERR_BADARG, "malformed SOS");
    if (ns != nf) return fail(OMR_ERR_NOTIMPL, "more than one scan is not implemented");
    if (adobe) return fail(OMR_ERR_NOTIMPL, "streams with an Adobe APP14 segment are not implemented");
    if (nf == 3 && !jfif && frame[0][0] == 'R' && frame[1][0] == 'G' && frame[2][0] == 'B')
        return fail(OMR_ERR_NOTIMPL, "component ids R G B (not YCbCr) are not implemented");
    h->orient = orient;
    if (orient != 1 && refuse_orientation) return fail(OMR_ERR_NOTIMPL, "EXIF orientation %d is not implemented (imread would turn the image)", orient);
    // a one-component scan is not interleaved: its MCU is one block whatever factors SOF declares (T.81 A.2.2)
    if (nf == 1 && frame[0][1] >= 1 && frame[0][1] <= 4 && frame[0][2] >= 1 && frame[0][2] <= 4) frame[0][1] = frame[0][2] = 1;
    for (int i = 0; i < nf; i++) {
        const bool ok = i == 0 ? (frame[0][1] == 1 && frame[0][2] == 1) || (frame[0][1] == 2 && frame[0][2] <= 2 && frame[0][2] >= 1)
                               : frame[i][1] == 1 && frame[i][2] == 1;
        if (!ok) return fail(OMR_ERR_NOTIMPL, "these sampling factors are not implemented (4:4:4, 4:2:2, 4:2:0)");
    }
    if (body[1 + 2 * ns] != 0 || body[2 + 2 * ns] != 63 || body[3 + 2 * ns] != 0)
        return fail(OMR_ERR_NOTIMPL, "a spectral selection that is not a baseline scan's");
    h->ncomp = nf, h->hs = frame[0][1], h->vs = frame[0][2];
    memset(&h->tab, 0, sizeof h->tab);
    for (int i = 0; i < ns; i++) {
        const int cs = body[1 + 2 * i], td = body[2 + 2 * i] >> 4, ta = body[2 + 2 * i] & 15;
        if (cs != frame[i][0]) return fail(OMR_ERR_NOTIMPL, "scan components out of the frame's order are not implemented");
        if (frame[i][3] > 3 || td > 3 || ta > 3 || !qt_set[frame[i][3]] || !dht[0][td].set || !dht[1][ta].set)
            return fail(OMR_ERR_BADARG, "SOS names a table that no DQT / DHT defined");
        for (int k = 0; k < 64; k++) h->tab.quant[i][k] = qt[frame[i][3]][k];
        derive(dht[0][td], &h->tab.dc[i]);
        derive(dht[1][ta], &h->tab.ac[i]);
    }
    h->data = p;
    // bit offsets inside an image are 32-bit on the device (with room for a subsequence and the rounding to words)
    if ((len - p) * 8 > (int64_t)0xffffffffLL - 65536)
        return fail(OMR_ERR_ASSERT, "entropy data of %lld bytes exceeds 2^32 bits: not supported", (long long)(len - p));
    return OMR_OK;
}

int omr::exif_orientation_tiff(const uint8_t *t, int64_t n)
{
    if (n < 8) return 1;
    bool le;
    if (!memcmp(t, "II*\0", 4)) le = true;
    else if (!memcmp(t, "MM\0*", 4)) le = false;
    else return 1;
    auto u16 = [&](int64_t o) { return le ? t[o] | t[o + 1] << 8 : t[o] << 8 | t[o + 1]; };
    auto u32 = [&](int64_t o) {
        return le ? (int64_t)t[o] | (int64_t)t[o + 1] << 8 | (int64_t)t[o + 2] << 16 | (int64_t)t[o + 3] << 24
                  : (int64_t)t[o] << 24 | (int64_t)t[o + 1] << 16 | (int64_t)t[o + 2] << 8 | (int64_t)t[o + 3];
    };
    const int64_t ifd = u32(4);
    if (ifd + 2 > n) return 1;
    const int cnt = u16(ifd);
    for (int e = 0; e < cnt; e++) {
        const int64_t o = ifd + 2 + 12 * (int64_t)e;
        if (o + 12 > n) break;
        if (u16(o) == 0x0112) return u16(o + 8);
    }
    return 1;
}

JdecStats &omr::jdec_stats() { return thread_stats<JdecStats>(); }

int omr::jpeg_decode_device(const uint8_t *const *streams, const int64_t *len, const JdecHeader *hdr, const int32_t *skip, int n,
                            int channels, uint8_t *d_out, int64_t out_stride, int64_t step, int32_t *rc, hipStream_t s)
{
    jdec_stats().begin_call();
    DrainOnExit drain{s};
    return for_each_group(
        n, skip, kGroupImages, kGroupBlocks, kGroupBytes,
        [&](int i) {
            const int64_t bytes = len[i] - hdr[i].data;
            if (bytes <= 0) rc[i] = OMR_ERR_ASSERT;  // nothing behind SOS
            return GroupCost{blocks_of(hdr[i]), bytes, bytes > 0};
        },
        [&](const int *idx, int g) { return decode_group(streams, len, hdr, idx, g, channels, d_out, out_stride, step, rc, s); });
}

extern "C" {

int omr_jpeg_info(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *components, int32_t *sampling)
{
    clear_error();
    if (!stream || len < 0) return fail(OMR_ERR_BADARG, "null stream");
    std::vector<JdecHeader> h(1);
    const int rc = jdec_parse(stream, len, &h[0]);
    if (rows) *rows = h[0].rows;
    if (cols) *cols = h[0].cols;
    if (components) *components = h[0].ncomp;
    if (sampling) *sampling = h[0].hs << 4 | h[0].vs;
    return rc;
}

int omr_jpeg_decode_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels, uint8_t *d_out,
                                 int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols, int32_t *out_size,
                                 int32_t *rc)
{
    std::vector<JdecHeader> hdr;
    return decode_batch_entry(
        BatchDecodeArgs{streams, len, n, channels, d_out, out_stride_bytes, step_bytes, rows, cols, out_size, rc},
        "stream %d is %d x %d, the slot %d x %d", no_extra_check, [&](size_t cnt) { hdr.reserve(cnt); },
        [&](int i) {
            hdr.emplace_back();
            const int r = jdec_parse(streams[i], len[i], &hdr.back());
            return ParsedSize{r, hdr.back().rows, hdr.back().cols};
        },
        [&](const int32_t *skip, hipStream_t s) {
            return jpeg_decode_device(streams, len, hdr.data(), skip, n, channels, d_out, out_stride_bytes, step_bytes, rc, s);
        });
}

int omr_jpeg_decode_stats(int32_t enable, int32_t *sub_bits, int32_t *groups, int32_t *rounds, double *stage_ms)
{
    clear_error();
    if (sub_bits) *sub_bits = JDEC_SUB_BITS;
    if (rounds) *rounds = jdec_stats().rounds;
    jdec_stats().report(enable, groups, stage_ms);
    return OMR_OK;
}

int omr_jpeg_decode(const uint8_t *stream, int64_t len, int32_t channels, omr_image_owned *dst)
{
    std::vector<JdecHeader> h(1);
    const int32_t skip = 0;
    return decode_one_entry(
        stream, len, channels, dst, "the entropy data is not a scan of its header (cut short, an invalid code, or blocks left over)",
        no_extra_check,
        [&] {
            const int r = jdec_parse(stream, len, &h[0]);
            return ParsedSize{r, h[0].rows, h[0].cols};
        },
        [&](uint8_t *d_out, int64_t stride, int64_t step, int32_t *rc, hipStream_t s) {
            return jpeg_decode_device(&stream, &len, h.data(), &skip, 1, channels, d_out, stride, step, rc, s);
        });
}

}  // extern "C"
