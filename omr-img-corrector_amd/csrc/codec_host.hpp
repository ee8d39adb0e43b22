// codec_host.hpp -- the host frame the image codecs share: the per-thread stage statistics and
// the timer that fills them, the entry points' argument checks and bookkeeping for a batch of streams and for one
// stream, and the walk that cuts a batch into groups of launches.  Host only.  A decoder supplies its parser, its
// *_decode_device with its decode_group, its caps and its "damaged" message; an encoder its checks, its bound with the
// bound's name, its *_encode_device with its encode_group, and its group cost; everything else is here, once.
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
#include "stream_sink.hpp"

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
    bool take = true;
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

// ---- the encoders' half ------------------------------------------------------------------------------------------------
// The walk of a *_encode_device over its n images (image i is sizes[2 i] x sizes[2 i + 1]): contiguous groups
// [i0, i0 + g) of at most max_images members.  A 0 x 0 entry is a member that costs nothing; a group always takes its first
// member.  cost(rows, cols) gives an image's costs; fits(sum, c) says whether a member of cost c may join a group whose
// members cost `sum` so far; run_group(i0, g) encodes the group.
// (for_each_group's index lists did not fit: a sink is addressed by i0 and a count, so the 0 x 0 entries have to stay
// members, and one codec closes a group by a rule that two sums against two caps cannot say.)
template <class Cost, class Fits, class RunGroup>
int for_each_run(const int32_t *sizes, int n, int max_images, Cost cost, Fits fits, RunGroup run_group)
{
    for (int i0 = 0; i0 < n;) {
        int g = 0;
        GroupCost sum{0, 0};
        for (; i0 + g < n && g < max_images; g++) {
            const int r = sizes[2 * (size_t)(i0 + g)], c = sizes[2 * (size_t)(i0 + g) + 1];
            const GroupCost m = r > 0 ? cost(r, c) : GroupCost{0, 0};
            if (g > 0 && !fits(sum, m)) break;
            sum.a += m.a, sum.b += m.b;
        }
        if (int rc = run_group(i0, g)) return rc;
        i0 += g;
    }
    return OMR_OK;
}

// The streams of one group, images [i0, i0 + g): their lengths, which the codec fills in, and where the sink puts them.
// Host vectors that asynchronous copies read: an encode_group declares it among its first objects, before DrainOnExit.
struct GroupStreams {
    JpegSink &sink;
    const int i0, g;
    std::vector<int64_t> len, off;
    GroupStreams(JpegSink &to, int first, int count) : sink(to), i0(first), g(count), len((size_t)count, 0), off((size_t)count, 0) {}
    // a group of nothing but 0 x 0 entries: the sink hears of them, no device work
    int all_empty()
    {
        uint8_t *d_out = nullptr;
        if (int rc = sink.place(i0, g, len.data(), &d_out, off.data())) return rc;
        return done();
    }
    // the lengths stand: asks the sink where the streams go, writes that into the image table's out_off and uploads the
    // table again (im stays alive until `s` has drained); *d_out: the base of the offsets
    template <class Img>
    int place(std::vector<Img> &im, const DevBuf &d_im, hipStream_t s, uint8_t **d_out)
    {
        if (int rc = sink.place(i0, g, len.data(), d_out, off.data())) return rc;
        for (int j = 0; j < g; j++) im[(size_t)j].out_off = off[(size_t)j];
        OMR_HIP(hipMemcpyAsync(d_im.p, im.data(), sizeof(Img) * (size_t)g, hipMemcpyHostToDevice, s));
        return OMR_OK;
    }
    // behind the group's final synchronise
    int done() { return sink.done(i0, g, len.data()); }
};

// the arguments every omr_*_encode_batch_device shares, as the C ABI has them
struct BatchEncodeArgs {
    const uint8_t *d_imgs;
    int64_t img_stride_bytes, step_bytes;
    int32_t rows, cols, channels;
    const int32_t *sizes;
    int32_t n;
    uint8_t *d_out;
    int64_t out_stride_bytes;
    int64_t *out_len;
};

inline int no_image_check(int, int, int64_t *) { return OMR_OK; }

// An omr_*_encode_batch_device: the argument checks, the sizes (null: every image fills its slot) held to the slot, the
// bound of a slot's stream (bound_name: as the refusal calls it), the leased stream, the slot sink and the device call.
// No output is touched on a refusal.
//   check()                    the codec's parameters and the slot's shape
//   bound()                    the bound of the slot's stream, asked once check() has passed
//   image_check(r, c, &need)   for every image that is not 0 x 0, behind its size check: may refuse it, may raise need
//   late_check()               a check of the codec's own behind the bound's
//   device(sizes, sink, s)     the codec's *_encode_device
template <class Check, class Bound, class ImageCheck, class LateCheck, class Device>
int encode_batch_entry(const BatchEncodeArgs &a, const char *bound_name, Check check, Bound bound, ImageCheck image_check,
                       LateCheck late_check, Device device)
{
    clear_error();
    if (!a.d_imgs || !a.d_out || !a.out_len) return fail(OMR_ERR_BADARG, "null argument");
    const int n = a.n;
    if (n < 0) return fail(OMR_ERR_BADARG, "negative n");
    int rc = check();
    if (rc) return rc;
    int64_t need = bound();
    if (a.step_bytes < (int64_t)a.cols * a.channels) return fail(OMR_ERR_BADARG, "step_bytes < cols x channels");
    if (a.img_stride_bytes < (int64_t)a.rows * a.step_bytes) return fail(OMR_ERR_BADARG, "img_stride_bytes < rows x step_bytes");
    std::vector<int32_t> sz(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const int r = a.sizes ? a.sizes[2 * (size_t)i] : a.rows, c = a.sizes ? a.sizes[2 * (size_t)i + 1] : a.cols;
        if (r < 0 || c < 0 || r > a.rows || c > a.cols || ((r == 0) != (c == 0)))
            return fail(OMR_ERR_BADARG, "sizes[%d] = %d x %d does not fit the %d x %d slot", i, r, c, a.rows, a.cols);
        sz[2 * (size_t)i] = r, sz[2 * (size_t)i + 1] = c;
        if (r > 0 && (rc = image_check(r, c, &need))) return rc;
    }
    if (a.out_stride_bytes < need) return fail(OMR_ERR_BADARG, "out_stride_bytes below %s (%lld)", bound_name, (long long)need);
    if ((rc = late_check())) return rc;
    if (n == 0) return OMR_OK;
    if ((rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    SlotSink sink;
    sink.d_out = a.d_out, sink.stride = a.out_stride_bytes, sink.out_len = a.out_len;
    return device(sz.data(), sink, st.s);
}

// An omr_*_encode of one host image into the caller's buffer: the argument checks, the leased stream, the upload, the
// device call with n = 1, *len and OMR_ERR_NOMEM for a buffer the stream (`what`: "stream" or "file") does not fit.
//   check()                                      the codec's parameters and the image's shape
//   late_check()                                 a check of the codec's own behind the pitch's
//   device(d_img, stride, step, size, sink, s)   the codec's *_encode_device on the one packed image
template <class Check, class LateCheck, class Device>
int encode_one_entry(const omr_image *src, uint8_t *out, int64_t cap, int64_t *len, const char *what, Check check,
                     LateCheck late_check, Device device)
{
    clear_error();
    if (!src || !src->data || !len || cap < 0 || (!out && cap > 0)) return fail(OMR_ERR_BADARG, "null argument");
    int rc = check();
    if (rc) return rc;
    if (src->step_bytes < (int64_t)src->cols * src->channels) return fail(OMR_ERR_BADARG, "step_bytes too small");
    if ((rc = late_check()) || (rc = have_device())) return rc;
    LeasedStream st;
    if ((rc = st.create())) return rc;
    const int64_t row = (int64_t)src->cols * src->channels;
    DevBuf in;
    OMR_HIP(in.alloc((size_t)(row * src->rows)));
    if ((rc = upload_rows(in.p, (size_t)row, src->data, (size_t)src->step_bytes, (size_t)row, (size_t)src->rows, st.s))) return rc;
    const int32_t size[2] = {src->rows, src->cols};
    HostSink sink;
    sink.out = out, sink.cap = cap, sink.s = st.s;
    if ((rc = device(in.as<uint8_t>(), row * src->rows, row, size, sink, st.s))) return rc;
    *len = sink.len;
    if (!sink.fits) return fail(OMR_ERR_NOMEM, "the %s takes %lld bytes, the buffer holds %lld", what, (long long)sink.len, (long long)cap);
    return OMR_OK;
}

}  // namespace omr
#pragma GCC visibility pop
