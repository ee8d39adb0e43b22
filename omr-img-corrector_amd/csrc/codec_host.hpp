// codec_host.hpp -- the host frame the image codecs share: the per-thread stage statistics and
// the timer that fills them, the entry points' argument checks and bookkeeping for a batch of streams and for one
// stream, and the walk that cuts a batch into groups of launches.  Host only.  A codec supplies its parser, its
// *_decode_device with its decode_group, its caps and its "damaged" message; everything else is here, once.
//
// The order of declarations inside every decode_group / encode_group, which this frame relies on and no user may change:
//   1. the host vectors that asynchronous copies read or write,
//   2. then DrainOnExit (engine.hpp),
//   3. then the StageTimer,
//   4. then the DevBufs.
// Destruction runs backwards: the buffers go back (a pooled DevBuf waits for its stream itself), the events go, the drain
// waits for whatever an error return left queued, and only then do the host vectors go.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "codec_stats.hpp"
#include "engine.hpp"

#pragma GCC visibility push(hidden)  // the frame is the library's own: nothing of it enters the dynamic symbol table
namespace omr {

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

inline int check_decoded_channels(int channels)
{
    if (channels != 1 && channels != 3) return fail(OMR_ERR_BADARG, "a decoded image has 1 or 3 channels, got %d", channels);
    return OMR_OK;
}

// the one object of a codec's stats type (codec_stats.hpp) on the calling thread
template <class Stats>
Stats &thread_stats()
{
    static thread_local Stats st;
    return st;
}

// The events between a group's N stages.  begin(on) creates them only while the thread collects statistics; without them
// mark() records nothing and finish() adds nothing.
template <int N>
struct StageTimer {
    hipEvent_t e[N + 1] = {};
    int n = 0;  // events created: 0 or N + 1
    ~StageTimer()
    {
        for (int i = 0; i < n; i++) (void)hipEventDestroy(e[i]);
    }
    int begin(bool on)
    {
        for (; on && n <= N; n++) OMR_HIP(hipEventCreate(&e[n]));
        return OMR_OK;
    }
    int mark(int k, hipStream_t s)
    {
        if (n) OMR_HIP(hipEventRecord(e[k], s));
        return OMR_OK;
    }
    // for a launcher that records stage boundaries itself: the events from k on, or null
    hipEvent_t *from(int k) { return n ? &e[k] : nullptr; }
    // behind the group's final synchronise
    int finish(CodecStats<N> &stats)
    {
        if (!n) return OMR_OK;
        stats.groups++;
        for (int k = 0; k < N; k++) {
            float ms = 0;
            OMR_HIP(hipEventElapsedTime(&ms, e[k], e[k + 1]));
            stats.ms[k] += ms;
        }
        return OMR_OK;
    }
};

// ---- the walk of a *_decode_device over its n members: groups of at most max_images members whose two costs stay under
// their caps.  A group always takes its first member, whatever it costs.  cost(i) gives member i's costs, or take = false
// for a member the codec passes over (and answers for itself); run_group(idx, g) decodes members idx[0 .. g).
struct GroupCost {
    int64_t a, b;
    bool take;
};

template <class Cost, class RunGroup>
int for_each_group(int n, const int32_t *skip, int max_images, int64_t cap_a, int64_t cap_b, Cost cost, RunGroup run_group)
{
    std::vector<int> idx;
    for (int i0 = 0; i0 < n;) {
        idx.clear();
        int64_t a = 0, b = 0;
        int i = i0;
        for (; i < n && (int)idx.size() < max_images; i++) {
            if (skip[i]) continue;
            const GroupCost c = cost(i);
            if (!c.take) continue;
            if (!idx.empty() && (a + c.a > cap_a || b + c.b > cap_b)) break;
            a += c.a, b += c.b, idx.push_back(i);
        }
        if (!idx.empty())
            if (int r = run_group(idx.data(), (int)idx.size())) return r;
        i0 = i;
    }
    return OMR_OK;
}

// ---- the entry points
// the arguments of an omr_*_decode_batch_device, as the C ABI has them
struct BatchDecodeArgs {
    const uint8_t *const *streams;
    const int64_t *len;
    int32_t n, channels;
    uint8_t *d_out;
    int64_t out_stride_bytes, step_bytes;
    int32_t rows, cols;
    int32_t *out_size, *rc;
};

// what a header step finds for one stream: its code, and the size as the caller sees it
struct ParsedSize {
    int rc, rows, cols;
};

inline int no_extra_check() { return OMR_OK; }

// An omr_*_decode_batch_device: the argument checks, every stream's header step with the slot-size refusal (slot_fmt: its
// wording, with i, the stream's and the slot's size as arguments), the bookkeeping of rc, skip and out_size, the leased
// stream, the device call and, behind it, 0 x 0 for what the device found damaged.
//   extra_check()          a check of the caller's own between the channel check and the slot checks
//   reserve(n)             room for n headers, made once the arguments stand
//   parse(i)               -> ParsedSize; called for i = 0 .. n - 1 in order
//   device(skip, stream)   the codec's *_decode_device on the parsed headers
template <class ExtraCheck, class Reserve, class Parse, class Device>
int decode_batch_entry(const BatchDecodeArgs &a, const char *slot_fmt, ExtraCheck extra_check, Reserve reserve, Parse parse,
                       Device device)
{
    clear_error();
    const int n = a.n;
    if (n < 0) return fail(OMR_ERR_BADARG, "negative n");
    if (!a.streams || !a.len || !a.d_out || !a.out_size || !a.rc) return fail(OMR_ERR_BADARG, "null argument");
    if (int r = check_decoded_channels(a.channels)) return r;
    if (int r = extra_check()) return r;
    if (a.rows <= 0 || a.cols <= 0) return fail(OMR_ERR_BADARG, "empty slot");
    if (a.step_bytes < (int64_t)a.cols * a.channels) return fail(OMR_ERR_BADARG, "step_bytes < cols x channels");
    if (a.out_stride_bytes < (int64_t)a.rows * a.step_bytes) return fail(OMR_ERR_BADARG, "out_stride_bytes < rows x step_bytes");
    for (int i = 0; i < n; i++)
        if (!a.streams[i] || a.len[i] < 0) return fail(OMR_ERR_BADARG, "streams[%d] is null or has a negative length", i);
    if (n == 0) return OMR_OK;
    reserve((size_t)n);
    std::vector<int32_t> skip((size_t)n, 0);
    int good = 0;
    for (int i = 0; i < n; i++) {
        const ParsedSize p = parse(i);
        a.rc[i] = p.rc;
        if (a.rc[i] == OMR_OK && (p.rows > a.rows || p.cols > a.cols)) a.rc[i] = fail(OMR_ERR_BADARG, slot_fmt, i, p.rows, p.cols, a.rows, a.cols);
        skip[(size_t)i] = a.rc[i] != OMR_OK;
        a.out_size[2 * (size_t)i] = skip[(size_t)i] ? 0 : p.rows;
        a.out_size[2 * (size_t)i + 1] = skip[(size_t)i] ? 0 : p.cols;
        good += !skip[(size_t)i];
    }
    if (good == 0) return OMR_OK;  // every stream refused: the codes are in rc, there is no device work
    clear_error();
    if (int r = have_device()) return r;
    LeasedStream st;
    if (int r = st.create()) return r;
    const int r = device(skip.data(), st.s);
    for (int i = 0; r == OMR_OK && i < n; i++)
        if (a.rc[i]) a.out_size[2 * (size_t)i] = a.out_size[2 * (size_t)i + 1] = 0;
    return r;
}

// An omr_*_decode of one stream into a malloc'ed image: the argument checks, the header step, the leased stream, the device
// buffer, the device call with n = 1, the codec's `damaged` message (a plain text, no conversions) and the copy down.
//   parse()                                       -> ParsedSize
//   device(d_out, out_stride, step, &rc, stream)  the codec's *_decode_device on the one parsed header
template <class ExtraCheck, class Parse, class Device>
int decode_one_entry(const uint8_t *stream, int64_t len, int32_t channels, omr_image_owned *dst, const char *damaged,
                     ExtraCheck extra_check, Parse parse, Device device)
{
    clear_error();
    if (!stream || len < 0 || !dst) return fail(OMR_ERR_BADARG, "null argument");
    if (int r = check_decoded_channels(channels)) return r;
    if (int r = extra_check()) return r;
    const ParsedSize p = parse();
    int r = p.rc;
    if (r) return r;
    if ((r = have_device())) return r;
    LeasedStream st;
    if ((r = st.create())) return r;
    const int64_t step = (int64_t)p.cols * channels, bytes = step * p.rows;
    DrainOnExit drain{st.s};
    DevBuf out;
    OMR_HIP(out.alloc((size_t)bytes));
    int32_t rc1 = 0;
    if ((r = device(out.as<uint8_t>(), bytes, step, &rc1, st.s))) return r;
    if (rc1) return fail(rc1, damaged);
    *dst = omr_image_owned{nullptr, p.rows, p.cols, channels, step};
    dst->data = (uint8_t *)malloc((size_t)bytes);
    if (!dst->data) return fail(OMR_ERR_NOMEM, "out of host memory");
    r = staged_d2h(dst->data, out.p, (size_t)bytes, st.s);
    if (r) omr_image_free(dst);
    return r;
}

}  // namespace omr
#pragma GCC visibility pop
