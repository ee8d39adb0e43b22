// projection_front.hpp -- the launchers of projection_front.hip: scale_self (transfer.rs:66-91) for a batch of
// same-shape scans, one launch per stage, the image index in blockIdx.z.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "kernels.hpp"

namespace omr {

// How the INTER_AREA kernels tile one scan: a workgroup takes twp destination pixels x th destination rows and walks
// down their source rows, `chunk` rows at a time through LDS rows of `segd` dwords.  tiled = false: the segment of a
// single destination pixel does not fit (shrink factors in the thousands): one thread per destination byte, straight
// from memory.
struct PfTiling {
    bool tiled = false;
    int twp = 0, th = 0, segd = 0, chunk = 0;
};

// Arguments of the INTER_AREA kernels.  Integer factors (resizeAreaFast_): kx, ky > 0 and no tables.  Fractional
// factors (resizeArea_): kx = ky = 0 and the four tap tables of area_tab (xtab built with cn, ytab with 1).
struct PfArea {
    const uint8_t *src;
    int64_t scan_stride, sstep;
    uint8_t *dst;
    int64_t out_stride, dstep;
    int cn, scols, drows, dcols, kx, ky;
    const AreaTap *xtab, *ytab;
    const int32_t *xofs, *yofs;
};

// Tile shape for a context (host, once): the widest tile whose source segment fits the LDS budget.  Fractional
// factors hand in the host copies of the tap tables; integer factors hand in NULL.
PfTiling pf_area_tiling(int cn, int dcols, int kx, const std::vector<AreaTap> *xtab, const std::vector<int32_t> *xofs,
                        const std::vector<AreaTap> *ytab);
hipError_t launch_pf_area(const PfArea &p, const PfTiling &t, int n, hipStream_t s);
hipError_t launch_pf_linear(const uint8_t *d_src, int64_t scan_stride, int64_t sstep, int srows, int scols, int cn, int n,
                            uint8_t *d_dst, int64_t out_stride, int64_t dstep, int drows, int dcols, bool area_mode,
                            hipStream_t s);

}  // namespace omr
