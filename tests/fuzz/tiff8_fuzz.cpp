// tiff8_fuzz.cpp -- a stand-alone program that feeds the serial logic of the LZW decoder (csrc/tiff_lzw.hpp: the bit reader,
// the table update, every bound check and the error rules, as tdec_lzw applies them) and tdec_parse's 8-bit header variants
// damaged input under the host sanitizers: every prefix and every flipped byte of a few small LZW strips, and of small
// gray and RGB files.  CPU only.
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ -I omr-img-corrector_amd/csrc tests/fuzz/tiff8_fuzz.cpp -o tiff8_fuzz && ./tiff8_fuzz
// Every buffer handed over is an exact-size heap block, so one byte read or written past its end is reported.
#define TDEC_PARSER_ONLY
#include "oics_tiff_dec.cpp"
#include "tiff_lzw.hpp"

#include <stdarg.h>
#include <stdio.h>

namespace omr {
int fail(int code, const char *, ...) { return code; }
}  // namespace omr

// ---- a small LZW writer: Clear, the codes of a greedy match against entries kept as byte strings, EOI
static std::vector<uint8_t> lzw_write(const std::vector<uint8_t> &data)
{
    std::vector<uint8_t> out;
    uint32_t acc = 0, nb = 0, idx = 0;
    auto put = [&](uint32_t c, uint32_t w) {
        acc = acc << w | c, nb += w;
        while (nb >= 8) out.push_back((uint8_t)(acc >> (nb - 8))), nb -= 8;
        acc &= (1u << nb) - 1;
    };
    std::vector<std::vector<uint8_t>> tab;  // entry 258 + k
    put(omr::TLZW_CLEAR, 9);
    size_t p = 0;
    while (p < data.size()) {
        uint32_t best = data[p];
        size_t blen = 1;
        for (size_t k = 0; k < tab.size(); k++)
            if (tab[k].size() > blen && p + tab[k].size() <= data.size() && !memcmp(tab[k].data(), data.data() + p, tab[k].size()))
                best = 258 + (uint32_t)k, blen = tab[k].size();
        put(best, omr::tlzw_width(idx)), idx++;
        if (p + blen < data.size()) {
            std::vector<uint8_t> e(data.begin() + (long)p, data.begin() + (long)(p + blen + 1));
            tab.push_back(e);
        }
        p += blen;
        if (idx == 3836) put(omr::TLZW_CLEAR, 12), idx = 0, tab.clear();
    }
    put(omr::TLZW_EOI, omr::tlzw_width(idx));
    if (nb) out.push_back((uint8_t)(acc << (8 - nb)));
    return out;
}

static long decoded, refused;

// -> the error; the output and both tables are exact-size heap blocks
static uint32_t run_strip(const std::vector<uint8_t> &strip, uint32_t total, std::vector<uint8_t> *got)
{
    uint8_t *in = (uint8_t *)malloc(strip.size() ? strip.size() : 1);
    if (!strip.empty()) memcpy(in, strip.data(), strip.size());
    uint8_t *out = (uint8_t *)malloc(total);
    uint32_t *tp = (uint32_t *)malloc(sizeof(uint32_t) * omr::TLZW_ENTRIES);
    uint16_t *tl = (uint16_t *)malloc(sizeof(uint16_t) * omr::TLZW_ENTRIES);
    memset(out, 0, total);
    const uint32_t e = omr::tlzw_decode_serial(in, (uint32_t)strip.size(), out, total, tp, tl);
    if (e != 0 && e != omr::TLZW_ERR_INPUT && e != omr::TLZW_ERR_CODE && e != omr::TLZW_ERR_TABLE) abort();
    if (got) got->assign(out, out + total);
    (e ? refused : decoded)++;
    free(in), free(out), free(tp), free(tl);
    return e;
}

static void fuzz_strip(const std::vector<uint8_t> &data)
{
    const std::vector<uint8_t> strip = lzw_write(data);
    std::vector<uint8_t> got;
    if (run_strip(strip, (uint32_t)data.size(), &got) != 0 || got != data) abort();  // the strip itself decodes to its source
    if (run_strip(strip, (uint32_t)data.size() + 1, nullptr) != omr::TLZW_ERR_INPUT) abort();
    for (size_t n = 0; n < strip.size(); n++) run_strip(std::vector<uint8_t>(strip.begin(), strip.begin() + (long)n), (uint32_t)data.size(), nullptr);
    for (size_t i = 0; i < strip.size(); i++)
        for (int m : {0xff, 0x80, 0x10, 0x01}) {
            std::vector<uint8_t> v(strip);
            v[i] ^= (uint8_t)m;
            run_strip(v, (uint32_t)data.size(), nullptr);
        }
}

// ---- a small file: little-endian, the IFD behind the strips
static std::vector<uint8_t> tiff_write(int rows, int cols, int spp, int compression, int predictor, const std::vector<std::vector<uint8_t>> &strips, int rps)
{
    std::vector<uint8_t> f = {'I', 'I', 42, 0, 0, 0, 0, 0};
    auto p16 = [&](uint32_t v) { f.push_back((uint8_t)v), f.push_back((uint8_t)(v >> 8)); };
    auto p32 = [&](uint32_t v) { p16(v & 0xffff), p16(v >> 16); };
    std::vector<uint32_t> off, cnt;
    for (const auto &s : strips) {
        off.push_back((uint32_t)f.size()), cnt.push_back((uint32_t)s.size());
        f.insert(f.end(), s.begin(), s.end());
        if (f.size() & 1) f.push_back(0);
    }
    const uint32_t bps_at = (uint32_t)f.size();
    for (int k = 0; k < 3; k++) p16(8);
    const uint32_t off_at = (uint32_t)f.size();
    for (uint32_t v : off) p32(v);
    const uint32_t cnt_at = (uint32_t)f.size();
    for (uint32_t v : cnt) p32(v);
    const uint32_t ifd = (uint32_t)f.size();
    f[4] = (uint8_t)ifd, f[5] = (uint8_t)(ifd >> 8), f[6] = (uint8_t)(ifd >> 16), f[7] = (uint8_t)(ifd >> 24);
    const uint32_t ns = (uint32_t)strips.size();
    p16(11);
    auto ent = [&](uint32_t tag, uint32_t type, uint32_t count, uint32_t v) { p16(tag), p16(type), p32(count), p32(v); };
    ent(256, 4, 1, (uint32_t)cols), ent(257, 4, 1, (uint32_t)rows);
    ent(258, 3, (uint32_t)spp, spp == 3 ? bps_at : 8u), ent(259, 3, 1, (uint32_t)compression), ent(262, 3, 1, spp == 3 ? 2u : 1u);
    ent(273, 4, ns, ns == 1 ? off[0] : off_at), ent(277, 3, 1, (uint32_t)spp), ent(278, 4, 1, (uint32_t)rps);
    ent(279, 4, ns, ns == 1 ? cnt[0] : cnt_at), ent(284, 3, 1, 1), ent(317, 3, 1, (uint32_t)predictor);
    p32(0);
    return f;
}

static int counts[4];

static void feed(const std::vector<uint8_t> &v)
{
    uint8_t *p = (uint8_t *)malloc(v.size() ? v.size() : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size());
    omr::TdecHeader h;
    const int rc = omr::tdec_parse(p, (int64_t)v.size(), &h);
    if (rc == 0) {
        for (const omr::TdecPiece &s : h.strips)
            if (s.off < 0 || s.off + (int64_t)s.len > (int64_t)v.size()) abort();  // an accepted strip lies inside the stream
        if (h.rows < 1 || h.cols < 1 || h.strips.empty()) abort();
        if ((h.bits_per_sample != 1 && h.bits_per_sample != 8) || (h.samples != 1 && h.samples != 3) || (h.predictor != 1 && h.predictor != 2)) abort();
        if (h.samples == 3 && h.bits_per_sample != 8) abort();
    }
    counts[rc == 0 ? 0 : rc == OMR_ERR_BADARG ? 1 : rc == OMR_ERR_NOTIMPL ? 2 : 3]++;
    if (rc != 0 && rc != OMR_ERR_BADARG && rc != OMR_ERR_NOTIMPL && rc != OMR_ERR_ASSERT) abort();
    free(p);
}

static void fuzz_file(const std::vector<uint8_t> &base)
{
    const int before = counts[0];
    feed(base);
    if (counts[0] != before + 1) abort();  // the file itself is accepted
    for (size_t n = 0; n < base.size(); n++) feed(std::vector<uint8_t>(base.begin(), base.begin() + (long)n));
    for (size_t i = 0; i < base.size(); i++)
        for (int m : {0xff, 0x80, 0x09, 0x01}) {
            std::vector<uint8_t> v(base);
            v[i] ^= (uint8_t)m;
            feed(v);
        }
    for (size_t i = 0; i < base.size(); i++)
        for (int b : {0, 0xff}) {
            std::vector<uint8_t> v(base);
            v[i] = (uint8_t)b;
            if (i + 1 < v.size()) v[i + 1] = (uint8_t)b;
            feed(v);
        }
}

int main()
{
    uint32_t seed = 12345;
    auto rnd = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 24; };
    std::vector<std::vector<uint8_t>> datas;
    datas.push_back(std::vector<uint8_t>(300, 7));  // KwKwK at every step
    std::vector<uint8_t> d;
    for (int k = 0; k < 200; k++) d.push_back((uint8_t)(k & 1 ? 255 : 0));
    datas.push_back(d), d.clear();
    for (int k = 0; k < 700; k++) d.push_back((uint8_t)(rnd() & 3));  // crosses 9 -> 10 bits
    datas.push_back(d), d.clear();
    for (int k = 0; k < 5000; k++) d.push_back((uint8_t)rnd());  // every width, the table filled and cleared
    datas.push_back(d);
    for (size_t k = 0; k < datas.size(); k++) {
        if (k < 3) fuzz_strip(datas[k]);
        else {  // the long one: itself, and a few hundred cuts and flips
            const std::vector<uint8_t> strip = lzw_write(datas[k]);
            std::vector<uint8_t> got;
            if (run_strip(strip, (uint32_t)datas[k].size(), &got) != 0 || got != datas[k]) abort();
            for (int t = 0; t < 300; t++) {
                std::vector<uint8_t> v(strip);
                v[(rnd() << 8 | rnd()) % v.size()] ^= (uint8_t)(1u << (rnd() & 7));
                if (t & 1) v.resize((rnd() << 8 | rnd()) % v.size());
                run_strip(v, (uint32_t)datas[k].size(), nullptr);
            }
        }
    }
    const std::vector<uint8_t> g = datas[2], strip = lzw_write(std::vector<uint8_t>(g.begin(), g.begin() + 60));
    fuzz_file(tiff_write(4, 15, 1, 5, 2, {strip}, 4));
    fuzz_file(tiff_write(4, 5, 3, 5, 1, {lzw_write(std::vector<uint8_t>(g.begin(), g.begin() + 30)), lzw_write(std::vector<uint8_t>(g.begin() + 30, g.begin() + 60))}, 2));
    fuzz_file(tiff_write(4, 5, 3, 1, 1, {std::vector<uint8_t>(g.begin(), g.begin() + 60)}, 4));
    fuzz_file(tiff_write(4, 15, 1, 32773, 1, {{0xc5, 9}}, 4));  // one run of 60
    printf("strips: %ld decoded, %ld refused; headers: %d accepted, %d BADARG, %d NOTIMPL, %d ASSERT\n", decoded, refused, counts[0], counts[1], counts[2],
           counts[3]);
    return 0;
}
