// flow_frame.hpp -- the one bucket-and-chunk walk of the batch deskew flows (projection_batch.cpp, detector_deskew.cpp,
// correct_batch.cpp).  A call is source x flow x sink:
//   source  host images (upload_chunk) or file contents (ImreadChunk + imread_decode_device, with the members' decode
//           codes), chosen by the frame from what the entry point hands in
//   flow    a Flow: the few things that differ between the three
//   sink    none (the angles alone), host canvases (download_canvases) or encoded streams (OutFormat + StreamSink)
// flow_host_call and flow_streams_call own everything else: the checks of every sheet before any device work, the
// buckets by shape, the encoder's canvas check, the chunks of a bucket, the scatter of the results and what a failing
// call leaves behind.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "../../include/omrdeskew.h"

namespace omr {

// Sheets of one shape per run of a bucket.  With canvases a run carries 32: scan and canvas slot of an A4 colour sheet
// are 26 + 54 MB on the device (55 MB for the detectors' slot).  The detectors' angles alone: 64, their own host batches'
// bound.  The projection and correct contexts are made for 256 sheets; the correct flow runs that many with canvases too.
const int kDeskewChunk = 32;
const int kDetectorAnglesChunk = 64;
const int kAnglesChunk = 256;

// the scan slots of a chunk: rows packed, slots 256 bytes apart at least
inline int64_t flow_slot_stride(int64_t row_bytes, int rows) { return (row_bytes * rows + 255) & ~(int64_t)255; }

// Where a call's results stand, one entry per sheet: the caller's arrays, or the frame's own until the call has succeeded.
// extra is the flow's second column (best_idx; need_check), code the sheet's own code; any of them may be null.
struct FlowOut {
    double *angle = nullptr;
    int32_t *extra = nullptr, *code = nullptr;
    omr_image_owned *rotated = nullptr;  // sink: host canvases
    uint8_t **out = nullptr;             // sink: encoded streams, with their lengths
    int64_t *out_len = nullptr;
};

// the frame's own arrays for g sheets
struct FlowTemp {
    std::vector<double> angle;
    std::vector<int32_t> extra, code;
    std::vector<omr_image_owned> rotated;
    std::vector<uint8_t *> out;
    std::vector<int64_t> out_len;
    FlowTemp(int g, int32_t extra0, bool canvases, bool streams)
        : angle((size_t)g, 0.0), extra((size_t)g, extra0), code((size_t)g, 0),
          rotated(canvases ? (size_t)g : 0, omr_image_owned{nullptr, 0, 0, 0, 0}), out(streams ? (size_t)g : 0, nullptr),
          out_len(streams ? (size_t)g : 0, 0)
    {
    }
    FlowOut view()
    {
        FlowOut o;
        o.angle = angle.data(), o.extra = extra.data(), o.code = code.data();
        o.rotated = rotated.empty() ? nullptr : rotated.data();
        o.out = out.empty() ? nullptr : out.data(), o.out_len = out_len.empty() ? nullptr : out_len.data();
        return o;
    }
};

// "every sheet is decided": the n sheets of a streams call into the caller's arrays.  header_code[i] is what the header
// pass gave sheet i; the accepted ones (at[k] = i, in call order) carry `from`'s entry k.  With header_code null the
// refused sheets are left alone (the header pass wrote them already).
inline void flow_write_back(const FlowOut &to, int n, const int32_t *header_code, int32_t extra_refused, const std::vector<int> &at,
                            const FlowOut &from)
{
    for (int i = 0; header_code && i < n; i++) {
        to.angle[i] = 0.0, to.code[i] = header_code[i];
        if (to.extra) to.extra[i] = extra_refused;
        if (to.out) to.out[i] = nullptr, to.out_len[i] = 0;
    }
    for (size_t k = 0; k < at.size(); k++) {
        const int i = at[k];
        to.angle[i] = from.angle[k], to.code[i] = from.code[k];
        if (to.extra) to.extra[i] = from.extra[k];
        if (to.out) to.out[i] = from.out[k], to.out_len[i] = from.out_len[k];
    }
}

}  // namespace omr

#ifndef OMR_FLOW_FRAME_BOOKKEEPING_ONLY  // tests/flow_frame_main.cpp takes the part above alone
#include <string.h>

#include <algorithm>
#include <functional>
#include <memory>

#include "encode_any.hpp"
#include "engine.hpp"
#include "host_threads.hpp"
#include "orient.hpp"
#include "stream_sink.hpp"

#pragma GCC visibility push(hidden)  // the library's own: not in the dynamic symbol table
namespace omr {

struct FlowSink {
    enum Kind { NONE, CANVASES, STREAMS } kind = NONE;
    OutFormat fmt{OUT_JPEG, 0};  // STREAMS: what writes the canvases
};

// What the frame runs on: host images, or streams with the headers of their run (sheet k's in the array of hd.kind[k]).
struct FlowIn {
    const omr_image *imgs = nullptr;
    const uint8_t *const *streams = nullptr;
    const int64_t *len = nullptr;
    ImreadHeaders hd{};
};

// A flow's answer when the frame opens a bucket of one shape.
struct FlowBucket {
    enum How { RUN, PER_SHEET, ALL_CODE } how = RUN;  // chunk by chunk; sheet by sheet (per_sheet); every sheet gets `code`
    int code = OMR_OK;
    int chunk = 0;                         // RUN: slots per chunk,
    int canvas_rows = 0, canvas_cols = 0;  // the canvas slot when there is a sink
    int64_t out_step = 0;                  // and its row pitch
    std::shared_ptr<void> ctx;             // whatever `run` needs kept: the cached context
};

// z slots of a bucket on the device: scans in, canvases out (dout null: the angles alone)
struct FlowSlots {
    int rows, cols, cn, z;
    uint8_t *din;
    int64_t in_stride, row;
    uint8_t *dout;
    int64_t out_stride, out_step;
    const int32_t *zrc;  // the members' decode codes (null for host images): a damaged member's slot means nothing
    hipStream_t s;
};

struct Flow {
    // the correct flow's contract: the caller's arrays are the call's own -- outputs cleared once every sheet is checked,
    // freed and nulled again on failure, a streams call's refused sheets written during the header pass.  The other
    // flows write nothing unless the whole call succeeds.
    bool writes_early = false;
    int32_t extra_refused = 0;  // `extra` of a sheet that has a code
    // a host image the flow takes, as its per-call function checks it (the first bad one ends the call)
    std::function<int(const omr_image &)> accept;
    // the same rule on the parsed shapes of a streams call, where a bad one ends the call (may be empty: none does)
    std::function<int(const omr_image &)> accept_parsed;
    // the largest canvas of a shape, for the encoder's check: a code refuses the call, *R = 0 means the shape has none
    std::function<int(int rows, int cols, int *R, int *C)> canvas;
    std::function<int(int rows, int cols, int cn, bool canvases, FlowBucket *)> open;
    // the device run of s.z slots: ang, extra, code (cleared to OMR_OK) and size (2 per slot) of each
    std::function<int(const FlowBucket &, const FlowSlots &s, double *ang, int32_t *extra, int32_t *code, int32_t *size)> run;
    // PER_SHEET buckets: members idx of `in` through the per-call functions, into `r`
    std::function<int(const FlowIn &in, const std::vector<int> &idx, const FlowOut &r)> per_sheet;
};

inline int flow_bucket(const Flow &f, const FlowSink &sink, const FlowIn &in, int rows, int cols, int cn, const std::vector<int> &idx,
                       const FlowOut &r)
{
    const bool canvases = sink.kind != FlowSink::NONE;
    FlowBucket b;
    int rc = f.open(rows, cols, cn, canvases, &b);
    if (rc) return rc;
    if (b.how == FlowBucket::PER_SHEET) return f.per_sheet(in, idx, r);
    if (b.how == FlowBucket::ALL_CODE) {
        for (int i : idx) r.code[i] = b.code, r.angle[i] = 0.0, r.extra[i] = f.extra_refused;
        return OMR_OK;
    }
    const int m = (int)idx.size(), zmax = std::min(m, b.chunk);
    const int64_t row = (int64_t)cols * cn, in_stride = flow_slot_stride(row, rows), out_stride = b.out_step * b.canvas_rows;
    LeasedStream st;  // the batch's device buffers come from the block cache and return to it when the call ends
    if ((rc = st.create())) return rc;
    DevBuf din, dout;
    OMR_HIP(din.alloc((size_t)zmax * in_stride));
    if (canvases) OMR_HIP(dout.alloc((size_t)zmax * out_stride));
    std::vector<double> ang((size_t)zmax);
    std::vector<int32_t> extra((size_t)zmax), code((size_t)zmax), size(2 * (size_t)zmax, 0);
    ImreadChunk ck;
    for (int j0 = 0; j0 < m; j0 += zmax) {
        const int z = std::min(zmax, m - j0);
        if (in.streams) {
            // the chunk's streams -> the scan slots through the imread layer: each decoder fills its own members' slots, JPEG
            // members that imread turns -- the bucket's shape is their turned one -- go through a scratch buffer and orient.hip
            ck.gather(in.hd, in.streams, in.len, idx, j0, z);
            rc = imread_decode_device(ck.zs.data(), ck.zlen.data(), ck.hd.view(), nullptr, z, cn, false, din.as<uint8_t>(), in_stride, row,
                                      ck.zrc.data(), st.s);
        } else {  // host memory -> device, from several threads
            rc = upload_chunk(in.imgs, idx, j0, z, rows, row, din.as<uint8_t>(), in_stride);
        }
        if (rc) return rc;
        const int32_t *zrc = in.streams ? ck.zrc.data() : nullptr;
        const FlowSlots s{rows, cols, cn, z, din.as<uint8_t>(), in_stride, row, canvases ? dout.as<uint8_t>() : nullptr, out_stride, b.out_step, zrc, st.s};
        std::fill(code.begin(), code.end(), (int32_t)OMR_OK);
        if ((rc = f.run(b, s, ang.data(), extra.data(), code.data(), size.data()))) return rc;
        for (int j = 0; j < z; j++) {
            const int i = idx[(size_t)(j0 + j)];
            if (zrc && zrc[j]) code[(size_t)j] = zrc[j];
            if (code[(size_t)j])  // its code and no output
                ang[(size_t)j] = 0.0, extra[(size_t)j] = f.extra_refused, size[2 * (size_t)j] = size[2 * (size_t)j + 1] = 0;
            r.angle[i] = ang[(size_t)j], r.extra[i] = extra[(size_t)j], r.code[i] = code[(size_t)j];
        }
        if (sink.kind == FlowSink::CANVASES) {  // canvases -> fresh host images, from several threads
            rc = download_canvases(dout.as<uint8_t>(), out_stride, b.out_step, cn, size.data(), code.data(), idx, j0, z, r.rotated);
        } else if (sink.kind == FlowSink::STREAMS) {  // the canvases stay on the device: encoded there, only the streams come down
            StreamSink to(r.out, r.out_len, idx, j0);
            rc = sink.fmt.encode_device(dout.as<uint8_t>(), out_stride, b.out_step, cn, size.data(), z, to, st.s);
        }
        if (rc) return rc;
    }
    return OMR_OK;
}

// the encoders' offsets inside an image are 32-bit: a shape whose canvas slot could exceed them refuses the call, before
// any device work; then the device, and bucket by bucket
inline int flow_buckets(const Flow &f, const FlowSink &sink, const FlowIn &in, const ShapeBuckets &b, const FlowOut &r)
{
    int rc = OMR_OK;
    for (size_t k = 0; sink.kind == FlowSink::STREAMS && k < b.shapes.size(); k++) {
        int R = 0, C = 0;
        if ((rc = f.canvas(b.shapes[k].rows, b.shapes[k].cols, &R, &C))) return rc;
        if (R && (rc = sink.fmt.check_canvas(R, C, b.shapes[k].cn))) return rc;
    }
    if ((rc = have_device())) return rc;
    for (size_t k = 0; k < b.shapes.size() && rc == OMR_OK; k++)
        rc = flow_bucket(f, sink, in, b.shapes[k].rows, b.shapes[k].cols, b.shapes[k].cn, b.members[k], r);
    return rc;
}

// what a failed call had made so far
inline void flow_free(const FlowOut &r, int n)
{
    for (int i = 0; r.rotated && i < n; i++) omr_image_free(&r.rotated[i]);
    for (int i = 0; r.out && i < n; i++) free(r.out[i]), r.out[i] = nullptr, r.out_len[i] = 0;
}

// A call on n host images (arguments other than the images already checked): `to` names the caller's arrays.
inline int flow_host_call(const Flow &f, const FlowSink &sink, const omr_image *srcs, int n, const FlowOut &to)
{
    ShapeBuckets b;
    int rc = bucket_by_shape(srcs, n, f.accept, &b);
    if (rc) return rc;
    FlowTemp tmp(f.writes_early ? 0 : n, f.extra_refused, sink.kind == FlowSink::CANVASES, sink.kind == FlowSink::STREAMS);
    const FlowOut r = f.writes_early ? to : tmp.view();
    if (f.writes_early) {
        for (int i = 0; to.rotated && i < n; i++) to.rotated[i] = omr_image_owned{nullptr, 0, 0, 0, 0};
        for (int i = 0; to.out && i < n; i++) to.out[i] = nullptr, to.out_len[i] = 0;
    }
    FlowIn in;
    in.imgs = srcs;
    if ((rc = flow_buckets(f, sink, in, b, r))) {
        flow_free(r, n);
        return rc;
    }
    if (f.writes_early) return OMR_OK;
    memcpy(to.angle, r.angle, sizeof(double) * (size_t)n);
    if (to.extra) memcpy(to.extra, r.extra, sizeof(int32_t) * (size_t)n);
    if (to.code) memcpy(to.code, r.code, sizeof(int32_t) * (size_t)n);
    if (to.rotated) memcpy(to.rotated, r.rotated, sizeof(omr_image_owned) * (size_t)n);
    return OMR_OK;
}

// the streams of a call: each there, with a length
inline int flow_check_streams(const uint8_t *const *streams, const int64_t *len, int n)
{
    for (int i = 0; i < n; i++)
        if (!streams[i] || len[i] < 0) return fail(OMR_ERR_BADARG, "streams[%d] is null or has a negative length", i);
    return OMR_OK;
}

// A call on n streams decoded to cn channels (arguments already checked).  parse(run, stream, len) is the flow's header
// policy: the stream appended to `run` as its last member, its shape as the flow's slots take it and rc by the decoder's
// rules and the per-call function's -- a sheet with a code keeps it and leaves the batch here.
inline int flow_streams_call(const Flow &f, const FlowSink &sink, const uint8_t *const *streams, const int64_t *len, int n, int cn,
                             const std::function<ImreadParsed(ImreadRun &, const uint8_t *, int64_t)> &parse, const FlowOut &to)
{
    std::vector<int32_t> code((size_t)n, OMR_OK);
    ImreadRun run;
    std::vector<int> at;
    std::vector<omr_image> views;
    std::vector<const uint8_t *> zs;
    std::vector<int64_t> zlen;
    run.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        const ImreadParsed ps = parse(run, streams[i], len[i]);
        code[(size_t)i] = ps.rc;
        if (f.writes_early) {  // (the accepted sheets' entries are written again when the call has succeeded)
            to.angle[i] = 0.0, to.extra[i] = f.extra_refused, to.code[i] = ps.rc;
            if (to.out) to.out[i] = nullptr, to.out_len[i] = 0;
        }
        if (ps.rc) {
            run.drop_last();
            continue;
        }
        at.push_back(i), zs.push_back(streams[i]), zlen.push_back(len[i]);
        views.push_back(omr_image{streams[i], ps.rows, ps.cols, cn, (int64_t)ps.cols * cn});
    }
    clear_error();
    const int g = (int)at.size();
    FlowTemp tmp(g, f.extra_refused, false, sink.kind == FlowSink::STREAMS);
    if (g) {
        ShapeBuckets b;
        int rc = bucket_by_shape(views.data(), g, [&f](const omr_image &v) { return f.accept_parsed ? f.accept_parsed(v) : (int)OMR_OK; }, &b);
        if (rc) return rc;
        FlowIn in;
        in.streams = zs.data(), in.len = zlen.data(), in.hd = run.view();
        if ((rc = flow_buckets(f, sink, in, b, tmp.view()))) {
            flow_free(tmp.view(), g);
            return rc;
        }
    }
    // every sheet is decided: the caller's arrays are written only now
    flow_write_back(to, n, f.writes_early ? nullptr : code.data(), f.extra_refused, at, tmp.view());
    return OMR_OK;
}

}  // namespace omr
#pragma GCC visibility pop
#endif
