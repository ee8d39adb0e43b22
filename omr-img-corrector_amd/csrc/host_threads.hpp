// host_threads.hpp -- what the entry points that start in host memory share above the engine: the host-thread fan-out,
// chunk upload and canvas download of the batch forms (correct_batch.cpp, projection_batch.cpp) and the keyed cache of shared contexts
// (those two, and the per-call drivers' sweep plans in oics_host.cpp).
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace omr {

// fn(stream, lo, hi) on T host threads over [0, m) in contiguous slices; the first error wins.  Every thread leases its own
// stream and pinned staging block (LeasedStream), so pageable copies and the page faults of fresh result images run side by side.
template <class F>
int on_threads(int m, F fn)
{
    const int T = (int)std::max(1u, std::min<unsigned>((unsigned)m, std::min(std::thread::hardware_concurrency(), 16u)));
    std::vector<int> rcs((size_t)T, OMR_OK);
    std::vector<std::string> errs((size_t)T);
    std::vector<std::thread> pool;
    int dev = 0;
    OMR_HIP(hipGetDevice(&dev));
    for (int t = 0; t < T; t++)
        pool.emplace_back([&, t]() {
            if (hipSetDevice(dev) != hipSuccess) {
                rcs[(size_t)t] = fail(OMR_ERR_GPU, "hipSetDevice failed");
            } else {
                LeasedStream st;
                int rc = st.create();
                if (!rc) rc = fn(st.s, (int)((int64_t)m * t / T), (int)((int64_t)m * (t + 1) / T));
                rcs[(size_t)t] = rc;
            }
            if (rcs[(size_t)t]) errs[(size_t)t] = last_error();
        });
    for (auto &th : pool) th.join();
    for (int t = 0; t < T; t++)
        if (rcs[(size_t)t]) return fail(rcs[(size_t)t], "%s", errs[(size_t)t].c_str());
    return OMR_OK;
}

// Images srcs[idx[j0 .. j0 + z)], each `rows` rows of `row_bytes`, from host memory to slots 0 .. z of d_in (in_stride
// bytes apart, rows packed), from several threads; complete on return.
inline int upload_chunk(const omr_image *srcs, const std::vector<int> &idx, int j0, int z, int rows, int64_t row_bytes,
                        uint8_t *d_in, int64_t in_stride)
{
    return on_threads(z, [&](hipStream_t s, int lo, int hi) -> int {
        for (int j = lo; j < hi; j++) {
            const omr_image &im = srcs[idx[(size_t)(j0 + j)]];
            int rc = upload_rows(d_in + (size_t)j * in_stride, (size_t)row_bytes, im.data, (size_t)im.step_bytes, (size_t)row_bytes,
                                 (size_t)rows, s);
            if (rc) return rc;
        }
        OMR_HIP(hipStreamSynchronize(s));
        return OMR_OK;
    });
}

// Canvases of a chunk -> fresh host images, from several threads: canvas j (size[2 j] rows x size[2 j + 1] cols x cn, at the
// top left of slot j of d_out, rows out_step apart) is packed on the device and comes down in one staged copy into
// out[idx[j0 + j]], which the caller frees with omr_image_free.  skip (may be null): canvas j stays where skip[j] != 0.
inline int download_canvases(const uint8_t *d_out, int64_t out_stride, int64_t out_step, int cn, const int32_t *size,
                             const int32_t *skip, const std::vector<int> &idx, int j0, int z, omr_image_owned *out)
{
    return on_threads(z, [&](hipStream_t s, int lo, int hi) -> int {
        DevBuf pack;
        OMR_HIP(pack.alloc((size_t)out_stride));
        for (int j = lo; j < hi; j++) {
            if (skip && skip[j] != OMR_OK) continue;
            const int r = size[2 * (size_t)j], c = size[2 * (size_t)j + 1];
            omr_image_owned &o = out[idx[(size_t)(j0 + j)]];
            const int64_t ostep = (int64_t)c * cn;
            uint8_t *data = (uint8_t *)malloc((size_t)r * ostep);
            if (!data) return fail(OMR_ERR_NOMEM, "out of host memory");
            o = omr_image_owned{data, r, c, cn, ostep};
            OMR_HIP(hipMemcpy2DAsync(pack.p, (size_t)ostep, d_out + (size_t)j * out_stride, (size_t)out_step, (size_t)ostep, (size_t)r,
                                     hipMemcpyDeviceToDevice, s));
            int rc1 = staged_d2h(o.data, pack.p, (size_t)r * ostep, s);
            if (rc1) return rc1;
        }
        return OMR_OK;
    });
}

// Shared contexts by key, most recently used first, at most `capacity` of them: the app calls with one parameter set over
// and over.  A context that falls out lives on until its last user lets go.
template <class Key, class Ctx>
class ContextCache {
  public:
    explicit ContextCache(size_t capacity) : capacity_(capacity) {}
    // the context of `key`: the cached one, or what make(&ctx) creates (outside the lock: it takes device time)
    template <class Make>
    int get(const Key &key, Make make, std::shared_ptr<Ctx> *out)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (auto it = entries_.begin(); it != entries_.end(); ++it)
                if (it->first == key) {
                    *out = it->second;
                    entries_.splice(entries_.begin(), entries_, it);
                    return OMR_OK;
                }
        }
        std::shared_ptr<Ctx> sp;
        int rc = make(&sp);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(mu_);
        entries_.emplace_front(key, sp);
        while (entries_.size() > capacity_) entries_.pop_back();
        *out = sp;
        return OMR_OK;
    }

  private:
    std::mutex mu_;
    std::list<std::pair<Key, std::shared_ptr<Ctx>>> entries_;
    const size_t capacity_;
};

}  // namespace omr
