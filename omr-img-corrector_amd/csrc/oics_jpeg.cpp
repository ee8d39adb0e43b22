// oics_jpeg.cpp -- host side of the JPEG encoder (jpeg.hip): libjpeg's default tables and header,
// the bound of a stream's length, the shapes it refuses, a group's layout and launches, and the cost that closes a group.
// The entry points omr_jpeg_encode* are the shared frame's (codec_host.hpp, section 4.28) with these handed in.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/omrdeskew.h"
#include "codec_host.hpp"
#include "jpeg.hpp"

using namespace omr;

namespace {

// Annex K.1 / K.2, natural order
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                               69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                               81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72,  92,  95,  98,  112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3 - K.6: bits[1..16], then the symbols
struct HuffSpec {
    uint8_t bits[16];
    int nval;
    const uint8_t *val;
};
const uint8_t kDcVal[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaVal[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaVal[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, kDcVal};
const HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, kDcVal};
const HuffSpec kAcLuma = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, kAcLumaVal};
const HuffSpec kAcChroma = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, kAcChromaVal};

// The longest code a block can take, in bits: a DC code of at most 11 bits with 11 value bits, and 63 AC coefficients of a
// 16-bit code with 10 value bits each (no ZRL and no EOB then).  The tables above have no longer codes.
constexpr int64_t kMaxBlockBits = 11 + 11 + 63 * (16 + 10);

// jpeg_set_quality(q, TRUE): jpeg_quality_scaling, then jpeg_add_quant_table with force_baseline
void quant_tables(int quality, uint16_t luma[64], uint16_t chroma[64])
{
    const int q = std::min(std::max(quality, 1), 100);
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; i++) {
        luma[i] = (uint16_t)std::min(std::max((kBaseLuma[i] * scale + 50) / 100, 1), 255);
        chroma[i] = (uint16_t)std::min(std::max((kBaseChroma[i] * scale + 50) / 100, 1), 255);
    }
}

// jpeg_make_c_derived_tbl: symbol -> code << 8 | length
void derive(const HuffSpec &h, uint32_t *out, int n_out)
{
    for (int i = 0; i < n_out; i++) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < h.bits[len - 1]; i++, k++, code++) out[h.val[k]] = (code << 8) | (uint32_t)len;
        code <<= 1;
    }
}

void put_segment(std::vector<uint8_t> *o, int marker, const std::vector<uint8_t> &body)
{
    o->push_back(0xFF), o->push_back((uint8_t)marker);
    o->push_back((uint8_t)((body.size() + 2) >> 8)), o->push_back((uint8_t)(body.size() + 2));
    o->insert(o->end(), body.begin(), body.end());
}

void put_dht(std::vector<uint8_t> *o, int ident, const HuffSpec &h)
{
    std::vector<uint8_t> b{(uint8_t)ident};
    b.insert(b.end(), h.bits, h.bits + 16);
    b.insert(b.end(), h.val, h.val + h.nval);
    put_segment(o, 0xC4, b);
}

// SOI .. SOS as jcmarker.c writes them (size 0 x 0: patched per image); *sof_off = where SOF0's rows / cols lie
std::vector<uint8_t> build_header(int cn, const uint16_t luma[64], const uint16_t chroma[64], int *sof_off)
{
    std::vector<uint8_t> o{0xFF, 0xD8};
    put_segment(&o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < (cn == 3 ? 2 : 1); t++) {
        std::vector<uint8_t> b{(uint8_t)t};
        for (int k = 0; k < 64; k++) b.push_back((uint8_t)(t ? chroma : luma)[kZigzag[k]]);
        put_segment(&o, 0xDB, b);
    }
    *sof_off = (int)o.size() + 5;
    if (cn == 3)
        put_segment(&o, 0xC0, {8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    else
        put_segment(&o, 0xC0, {8, 0, 0, 0, 0, 1, 1, 0x11, 0});
    put_dht(&o, 0x00, kDcLuma);
    put_dht(&o, 0x10, kAcLuma);
    if (cn == 3) {
        put_dht(&o, 0x01, kDcChroma);
        put_dht(&o, 0x11, kAcChroma);
        put_segment(&o, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    } else {
        put_segment(&o, 0xDA, {1, 1, 0x00, 0, 63, 0});
    }
    return o;
}

// blocks of the scan: 4:2:0 MCUs of six blocks (dummy ones included), or the gray image's own blocks
int64_t scan_blocks(int rows, int cols, int cn)
{
    if (cn == 3) return (int64_t)((rows + 15) / 16) * ((cols + 15) / 16) * 6;
    return (int64_t)((rows + 7) / 8) * ((cols + 7) / 8);
}

// Upper bound of a stream's length: header, the scan at kMaxBlockBits a block with every byte stuffed, EOI
int64_t stream_bound(int rows, int cols, int cn)
{
    const int64_t scan_bytes = (scan_blocks(rows, cols, cn) * kMaxBlockBits + 7) / 8;
    return JPEG_MAX_HEADER + 2 * scan_bytes + 2;
}

int check_jpeg_shape(int rows, int cols, int cn)
{
    if (cn == 4) return fail(OMR_ERR_NOTIMPL, "4-channel JPEG encoding is not implemented (1 or 3 channels)");
    if (cn != 1 && cn != 3) return fail(OMR_ERR_ASSERT, "JPEG takes 1 or 3 channels, got %d", cn);
    if (rows <= 0 || cols <= 0) return fail(OMR_ERR_ASSERT, "empty image");
    if (rows > 65535 || cols > 65535) return fail(OMR_ERR_ASSERT, "a JPEG image has at most 65535 rows and columns");
    return OMR_OK;
}

constexpr int64_t kGroupBlocks = 4 << 20;  // blocks of one group of launches: 512 MB of coefficients
constexpr int kGroupImages = 4096;

// one group: images [i0, i0 + g)
int encode_group(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int i0, int g,
                 const JpegTables *d_tab, const uint8_t *d_header, int header_len, int sof_off, JpegSink &sink, hipStream_t s)
{
    std::vector<JpegImg> im((size_t)g);
    GroupStreams out(sink, i0, g);
    std::vector<uint32_t> h_bits((size_t)g), h_ff((size_t)g);
    DrainOnExit drain{s};  // behind the host objects that asynchronous copies read or write, before the device buffers
    DevBuf d_im, coef, aclen, dcdiff, local, csum, coff, ibits, iff, bitbuf, fsum, foff;
    uint32_t blocks = 0, chunks = 0;
    int max_tx = 1, max_ty = 1, max_chunks = 1;
    for (int j = 0; j < g; j++) {
        JpegImg &m = im[(size_t)j];
        memset(&m, 0, sizeof m);
        const int r = sizes[2 * (size_t)(i0 + j)], c = sizes[2 * (size_t)(i0 + j) + 1];
        m.src_off = (int64_t)(i0 + j) * img_stride;
        m.rows = r, m.cols = c;
        m.bw = (c + 7) / 8, m.bh = (r + 7) / 8;
        m.mw = cn == 3 ? (c + 15) / 16 : m.bw, m.mh = cn == 3 ? (r + 15) / 16 : m.bh;
        m.blk0 = blocks, m.nblk = r > 0 ? (uint32_t)scan_blocks(r, c, cn) : 0;
        m.chunk0 = chunks, m.nchunk = (m.nblk + JPEG_CHUNK - 1) / JPEG_CHUNK;
        blocks += m.nblk, chunks += m.nchunk;
        max_tx = std::max(max_tx, (c + JPEG_TILE_W - 1) / JPEG_TILE_W);
        max_ty = std::max(max_ty, (r + JPEG_TILE_H - 1) / JPEG_TILE_H);
        max_chunks = std::max(max_chunks, (int)m.nchunk);
    }
    if (blocks == 0) return out.all_empty();
    OMR_HIP(d_im.alloc(sizeof(JpegImg) * (size_t)g));
    OMR_HIP(coef.alloc((size_t)blocks * 128));
    OMR_HIP(aclen.alloc((size_t)blocks * 2));
    OMR_HIP(dcdiff.alloc((size_t)blocks * 2));
    OMR_HIP(local.alloc((size_t)blocks * 4));
    OMR_HIP(csum.alloc((size_t)chunks * 4));
    OMR_HIP(coff.alloc((size_t)chunks * 4));
    OMR_HIP(ibits.alloc((size_t)g * 4));
    OMR_HIP(iff.alloc((size_t)g * 4));
    JpegPass p;
    memset(&p, 0, sizeof p);
    p.src = d_imgs, p.step = step, p.imgs = d_im.as<JpegImg>(), p.n = g, p.cn = cn, p.tab = d_tab;
    p.coef = coef.as<int16_t>(), p.aclen = aclen.as<uint16_t>(), p.dcdiff = dcdiff.as<int16_t>(), p.local = local.as<uint32_t>();
    p.chunk_sum = csum.as<uint32_t>(), p.chunk_off = coff.as<uint32_t>(), p.img_bits = ibits.as<uint32_t>();
    p.img_ff = iff.as<uint32_t>();
    p.header = d_header, p.header_len = header_len, p.sof_off = sof_off;
    // 1. coefficients and bit lengths; the host learns every image's scan length
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(JpegImg) * (size_t)g, hipMemcpyHostToDevice, s));
    int rc = jpeg_launch_blocks(p, max_tx, max_ty, s);
    if (rc || (rc = jpeg_launch_lengths(p, max_chunks, s))) return rc;
    OMR_HIP(hipMemcpyAsync(h_bits.data(), ibits.p, (size_t)g * 4, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    int64_t words = 0;
    uint32_t bchunks = 0;
    int max_bchunks = 1;
    for (int j = 0; j < g; j++) {
        JpegImg &m = im[(size_t)j];
        if (m.nblk == 0) continue;
        m.bits = h_bits[(size_t)j], m.nbytes = (m.bits + 7) / 8;  // no overflow: jpeg_check_scan_bits leaves that room
        m.bit_word = words;
        words += (int64_t)(m.bits + 31) / 32 + 1;
        m.bchunk0 = bchunks, m.nbchunk = (m.nbytes + JPEG_BYTE_CHUNK - 1) / JPEG_BYTE_CHUNK;
        bchunks += m.nbchunk;
        max_bchunks = std::max(max_bchunks, (int)m.nbchunk);
    }
    // 2. the bits, and how many bytes of them need stuffing
    OMR_HIP(bitbuf.alloc((size_t)words * 4));
    OMR_HIP(fsum.alloc((size_t)bchunks * 4));
    OMR_HIP(foff.alloc((size_t)bchunks * 4));
    p.bitbuf = bitbuf.as<uint32_t>(), p.ff_sum = fsum.as<uint32_t>(), p.ff_off = foff.as<uint32_t>();
    OMR_HIP(hipMemsetAsync(bitbuf.p, 0, (size_t)words * 4, s));
    OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(JpegImg) * (size_t)g, hipMemcpyHostToDevice, s));
    if ((rc = jpeg_launch_bits(p, max_chunks, max_bchunks, s))) return rc;
    OMR_HIP(hipMemcpyAsync(h_ff.data(), iff.p, (size_t)g * 4, hipMemcpyDeviceToHost, s));
    OMR_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < g; j++)
        if (im[(size_t)j].nblk) out.len[(size_t)j] = (int64_t)header_len + im[(size_t)j].nbytes + h_ff[(size_t)j] + 2;
    // 3. the streams, where the caller wants them
    if ((rc = out.place(im, d_im, s, &p.out))) return rc;
    if ((rc = jpeg_launch_streams(p, max_bchunks, s))) return rc;
    OMR_HIP(hipStreamSynchronize(s));
    return out.done();
}

}  // namespace

int omr::jpeg_check_scan_bits(int rows, int cols, int cn)
{
    // 64 bits of room for rounding up to bytes and dwords
    if (scan_blocks(rows, cols, cn) * kMaxBlockBits > (int64_t)0xffffffffLL - 64)
        return fail(OMR_ERR_ASSERT, "a %d x %d x %d image may take more than 2^32 bits of scan data: not supported", rows, cols, cn);
    return OMR_OK;
}

int omr::jpeg_encode_device(const uint8_t *d_imgs, int64_t img_stride, int64_t step, int cn, const int32_t *sizes, int n,
                            int quality, JpegSink &sink, hipStream_t s)
{
    for (int i = 0; i < n; i++)
        if (sizes[2 * (size_t)i] > 0)
            if (int rc = jpeg_check_scan_bits(sizes[2 * (size_t)i], sizes[2 * (size_t)i + 1], cn)) return rc;
    JpegTables tab;
    uint16_t ql[64], qc[64];
    quant_tables(quality, ql, qc);
    for (int i = 0; i < 64; i++) tab.div[0][i] = (uint16_t)(ql[i] * 8), tab.div[1][i] = (uint16_t)(qc[i] * 8);
    derive(kDcLuma, tab.dc[0], 12), derive(kDcChroma, tab.dc[1], 12);
    derive(kAcLuma, tab.ac[0], 256), derive(kAcChroma, tab.ac[1], 256);
    int sof_off = 0;
    const std::vector<uint8_t> header = build_header(cn, ql, qc, &sof_off);
    DrainOnExit drain{s};  // behind the tables and the header, which asynchronous copies read, before the device buffers
    DevBuf d_tab, d_header;
    if (int rc = upload_table(&d_tab, &tab, sizeof tab, s)) return rc;
    if (int rc = upload_table(&d_header, header.data(), header.size(), s)) return rc;
    return for_each_run(
        sizes, n, kGroupImages, [&](int r, int c) { return GroupCost{scan_blocks(r, c, cn), 0}; },
        [](const GroupCost &sum, const GroupCost &m) { return sum.a + m.a <= kGroupBlocks; },
        [&](int i0, int g) {
            return encode_group(d_imgs, img_stride, step, cn, sizes, i0, g, d_tab.as<JpegTables>(), d_header.as<uint8_t>(), (int)header.size(),
                                sof_off, sink, s);
        });
}

extern "C" {

int omr_jpeg_quant_tables(int32_t quality, uint16_t luma[64], uint16_t chroma[64])
{
    clear_error();
    if (!luma || !chroma) return fail(OMR_ERR_BADARG, "null table");
    quant_tables(quality, luma, chroma);
    return OMR_OK;
}

int omr_jpeg_bound(int32_t rows, int32_t cols, int32_t channels, int64_t *bytes)
{
    clear_error();
    if (!bytes) return fail(OMR_ERR_BADARG, "null bytes");
    if (int rc = check_jpeg_shape(rows, cols, channels)) return rc;
    *bytes = stream_bound(rows, cols, channels);
    return OMR_OK;
}

int omr_jpeg_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                                 int32_t channels, const int32_t *sizes, int32_t n, int32_t quality, uint8_t *d_out,
                                 int64_t out_stride_bytes, int64_t *out_len)
{
    const BatchEncodeArgs a{d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, d_out, out_stride_bytes, out_len};
    return encode_batch_entry(
        a, "omr_jpeg_bound", [&] { return check_jpeg_shape(rows, cols, channels); }, [&] { return stream_bound(rows, cols, channels); },
        no_image_check, [&] { return jpeg_check_scan_bits(rows, cols, channels); },
        [&](const int32_t *sz, JpegSink &sink, hipStream_t s) {
            return jpeg_encode_device(d_imgs, img_stride_bytes, step_bytes, channels, sz, n, quality, sink, s);
        });
}

int omr_jpeg_encode(const omr_image *src, int32_t quality, uint8_t *out, int64_t cap, int64_t *len)
{
    return encode_one_entry(
        src, out, cap, len, "stream", [&] { return check_jpeg_shape(src->rows, src->cols, src->channels); },
        [&] { return jpeg_check_scan_bits(src->rows, src->cols, src->channels); },
        [&](const uint8_t *d_img, int64_t stride, int64_t step, const int32_t *size, JpegSink &sink, hipStream_t s) {
            return jpeg_encode_device(d_img, stride, step, src->channels, size, 1, quality, sink, s);
        });
}

void omr_bytes_free(uint8_t *p) { free(p); }

}  // extern "C"
