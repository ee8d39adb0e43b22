// tiff_parse_fuzz.cpp -- a stand-alone program that feeds tdec_parse (csrc/oics_tiff_dec.cpp) damaged headers under the
// host sanitizers: every prefix of a small Group 4 file, every byte of it flipped in turn, and every byte of its IFD set to
// 0 and to 0xff.  The parser reads untrusted offsets; this is where reading outside the stream would show.  CPU only.
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ -I omr-img-corrector_amd/csrc tests/fuzz/tiff_parse_fuzz.cpp -o tiff_parse_fuzz && ./tiff_parse_fuzz small_g4.tif
// Every copy handed to the parser is an exact-size heap block, so one byte read past its end is reported.
#define TDEC_PARSER_ONLY
#include "oics_tiff_dec.cpp"

#include <stdarg.h>
#include <stdio.h>

namespace omr {
int fail(int code, const char *, ...) { return code; }
}  // namespace omr

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
    }
    counts[rc == 0 ? 0 : rc == OMR_ERR_BADARG ? 1 : rc == OMR_ERR_NOTIMPL ? 2 : 3]++;
    if (rc != 0 && rc != OMR_ERR_BADARG && rc != OMR_ERR_NOTIMPL && rc != OMR_ERR_ASSERT) abort();
    free(p);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> base;
    for (int c; (c = fgetc(f)) != EOF;) base.push_back((uint8_t)c);
    fclose(f);
    feed(base);
    if (counts[0] != 1) return 3;  // the file itself is accepted
    for (size_t n = 0; n < base.size(); n++) feed(std::vector<uint8_t>(base.begin(), base.begin() + n));
    for (size_t i = 0; i < base.size(); i++)
        for (int m : {0xff, 0x80, 0x01}) {
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
    printf("%zu bytes: %d accepted, %d BADARG, %d NOTIMPL, %d ASSERT\n", base.size(), counts[0], counts[1], counts[2], counts[3]);
    return 0;
}
