// stream_sink.hpp -- where the device encoders put a group's streams (the JpegSink protocol, jpeg.hpp: place, then done):
// SlotSink and HostSink for the encoders' own entry points, StreamSink for the files-to-files batch forms
// (correct_batch.cpp, projection_batch.cpp, detector_deskew.cpp): fresh host buffers, so that only the streams cross the link.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "engine.hpp"
#include "host_threads.hpp"
#include "jpeg.hpp"

namespace omr {

#pragma GCC visibility push(hidden)  // the library's own: not in the dynamic symbol table
// an omr_*_encode_batch_device's sink: slot i of the caller's buffer, lengths into the caller's host array
struct SlotSink : JpegSink {
    uint8_t *d_out;
    int64_t stride;
    int64_t *out_len;
    int place(int i0, int cnt, const int64_t *len, uint8_t **out, int64_t *off) override
    {
        *out = d_out;
        for (int j = 0; j < cnt; j++) off[j] = (int64_t)(i0 + j) * stride, out_len[i0 + j] = len[j];
        return OMR_OK;
    }
    int done(int, int, const int64_t *) override { return OMR_OK; }
};

// an omr_*_encode's sink: one stream, into the caller's host buffer when it fits
struct HostSink : JpegSink {
    uint8_t *out;
    int64_t cap, len = 0;
    hipStream_t s;
    DevBuf buf;
    bool fits = false;
    int place(int, int, const int64_t *l, uint8_t **d_out, int64_t *off) override
    {
        len = l[0], off[0] = 0;
        OMR_HIP(buf.alloc((size_t)len));
        *d_out = buf.as<uint8_t>();
        return OMR_OK;
    }
    int done(int, int, const int64_t *) override
    {
        fits = out && len <= cap;
        return fits ? staged_d2h(out, buf.p, (size_t)len, s) : OMR_OK;
    }
};
#pragma GCC visibility pop

// The streams of a chunk's canvases -> fresh host buffers: a device buffer of exactly the streams' size per group of the
// encoder, then one staged copy per stream from several threads.  Stream j belongs to sheet idx[j0 + j]: out[that]
// (malloc'ed) and out_len[that] receive it.
struct StreamSink : JpegSink {
    uint8_t **out;
    int64_t *out_len;
    const std::vector<int> &idx;
    int j0;
    DevBuf buf;
    std::vector<int64_t> off;
    StreamSink(uint8_t **streams, int64_t *lens, const std::vector<int> &members, int first)
        : out(streams), out_len(lens), idx(members), j0(first)
    {
    }
    int place(int, int cnt, const int64_t *len, uint8_t **d_out, int64_t *o) override
    {
        int64_t total = 0;
        off.assign((size_t)cnt, 0);
        for (int j = 0; j < cnt; j++) off[(size_t)j] = o[j] = total, total += (len[j] + 255) & ~(int64_t)255;
        buf.release();
        OMR_HIP(buf.alloc((size_t)std::max<int64_t>(total, 256)));
        *d_out = buf.as<uint8_t>();
        return OMR_OK;
    }
    int done(int i0, int cnt, const int64_t *len) override
    {
        return on_threads(cnt, [&](hipStream_t s, int lo, int hi) -> int {
            for (int j = lo; j < hi; j++) {
                if (len[j] == 0) continue;
                const int i = idx[(size_t)(j0 + i0 + j)];
                uint8_t *data = (uint8_t *)malloc((size_t)len[j]);
                if (!data) return fail(OMR_ERR_NOMEM, "out of host memory");
                out[i] = data, out_len[i] = len[j];
                if (int rc = staged_d2h(data, buf.as<uint8_t>() + off[(size_t)j], (size_t)len[j], s)) return rc;
            }
            return OMR_OK;
        });
    }
};

}  // namespace omr
