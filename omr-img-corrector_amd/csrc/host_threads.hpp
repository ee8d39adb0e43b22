// host_threads.hpp -- the host-thread fan-out of the batch entry points that start in host memory
// (correct_batch.cpp, projection_batch.cpp).
#pragma once
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "hough_host.hpp"

namespace omr {
namespace hh {

// fn(t, lo, hi) on T host threads over [0, m) in contiguous slices; the first error wins.  Every thread leases its own stream
// and pinned staging block (HStream), so pageable copies and the page faults of fresh result images run side by side.
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
                HStream st;
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

}  // namespace hh
}  // namespace omr
