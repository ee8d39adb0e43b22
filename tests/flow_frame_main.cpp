// flow_frame_main.cpp -- the host-only bookkeeping of csrc/flow_frame.hpp in a program of its own (tests/test_flow_frame_abi.py
// builds it with the address and undefined-behaviour sanitizers where the compiler has their runtimes): the chunk bounds and
// the slot stride, the frame's temporaries and the write-back of a streams call's accepted sheets, against a plain
// restatement, for every pattern of refused sheets of small calls and for seeded larger ones.
#define OMR_FLOW_FRAME_BOOKKEEPING_ONLY
#include "flow_frame.hpp"

#include <stdio.h>
#include <string.h>

using namespace omr;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) printf("line %d: %s\n", __LINE__, #c), failures++; \
    } while (0)

// one streams call of n sheets; refused[i] != 0: the header pass's code.  early: the correct flow's contract
static void one_call(int n, const std::vector<int32_t> &refused, bool early, bool with_extra, bool with_out)
{
    std::vector<double> angle((size_t)n, 7.5);
    std::vector<int32_t> extra((size_t)n, 77), code((size_t)n, 77);
    std::vector<uint8_t *> out((size_t)n, (uint8_t *)&failures);
    std::vector<int64_t> out_len((size_t)n, 99);
    FlowOut to;
    to.angle = angle.data(), to.code = code.data();
    if (with_extra) to.extra = extra.data();
    if (with_out) to.out = out.data(), to.out_len = out_len.data();
    std::vector<int> at;
    for (int i = 0; i < n; i++)
        if (!refused[(size_t)i]) at.push_back(i);
    const int g = (int)at.size();
    FlowTemp tmp(g, -1, false, with_out);
    CHECK((int)tmp.angle.size() == g && tmp.rotated.empty() && (int)tmp.out.size() == (with_out ? g : 0));
    const FlowOut r = tmp.view();
    CHECK(r.rotated == nullptr && (r.out != nullptr) == (with_out && g > 0));
    for (int k = 0; k < g; k++) {
        CHECK(r.angle[k] == 0.0 && r.extra[k] == -1 && r.code[k] == 0);
        r.angle[k] = 0.25 * at[(size_t)k], r.extra[k] = 1000 + at[(size_t)k], r.code[k] = at[(size_t)k] % 5 == 4 ? -215 : 0;
        if (with_out) r.out[k] = (uint8_t *)malloc(3), r.out_len[k] = 3 + at[(size_t)k];
    }
    if (early)  // the header pass of such a flow wrote the refused sheets itself
        for (int i = 0; i < n; i++)
            if (refused[(size_t)i]) {
                angle[(size_t)i] = 0.0, code[(size_t)i] = refused[(size_t)i];
                if (with_extra) extra[(size_t)i] = -1;
                if (with_out) out[(size_t)i] = nullptr, out_len[(size_t)i] = 0;
            }
    flow_write_back(to, n, early ? nullptr : refused.data(), -1, at, r);
    for (int i = 0; i < n; i++) {
        const bool ok = !refused[(size_t)i];
        CHECK(angle[(size_t)i] == (ok ? 0.25 * i : 0.0));
        CHECK(code[(size_t)i] == (ok ? (i % 5 == 4 ? -215 : 0) : refused[(size_t)i]));
        CHECK(extra[(size_t)i] == (with_extra ? (ok ? 1000 + i : -1) : 77));
        if (with_out) {
            CHECK((out[(size_t)i] != nullptr) == ok && out_len[(size_t)i] == (ok ? 3 + i : 0));
            free(out[(size_t)i]);
        } else {
            CHECK(out[(size_t)i] == (uint8_t *)&failures && out_len[(size_t)i] == 99);
        }
    }
}

int main()
{
    CHECK(kDeskewChunk == 32 && kDetectorAnglesChunk == 64 && kAnglesChunk == 256);
    CHECK(flow_slot_stride(1, 1) == 256 && flow_slot_stride(256, 1) == 256 && flow_slot_stride(159, 37) == 5888);
    CHECK(flow_slot_stride(7440, 3508) == 26099712);                    // an A4 colour scan: 26 MB
    CHECK(flow_slot_stride(32766 * 3, 32766) == 3220832512LL);          // past 2^31
    for (int n = 1; n <= 6; n++)
        for (int mask = 0; mask < (1 << n); mask++) {
            std::vector<int32_t> refused((size_t)n);
            for (int i = 0; i < n; i++) refused[(size_t)i] = (mask >> i) & 1 ? -213 - 2 * (i % 2) : 0;
            for (int v = 0; v < 8; v++) one_call(n, refused, v & 1, v & 2, v & 4);
        }
    uint32_t x = 12345;
    for (int round = 0; round < 20; round++) {
        const int n = 200 + 37 * round;
        std::vector<int32_t> refused((size_t)n);
        for (int i = 0; i < n; i++) x = x * 1664525u + 1013904223u, refused[(size_t)i] = (x >> 28) == 0 ? -5 : 0;
        one_call(n, refused, round & 1, true, true);
    }
    printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
