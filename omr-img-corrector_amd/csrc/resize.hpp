// resize.hpp -- the launcher of resize.hip: OpenCV's resize() (INTER_AREA, INTER_LINEAR) for n same-shape images of
// 8-bit interleaved channels in one launch, the image index in blockIdx.z.  A per-call resize is a batch of one.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "host_image.hpp"

namespace omr {

// One tap of resizeArea_ (computeResizeAreaTab): source index, destination index (both times cn), weight.
struct AreaTap {
    int32_t si, di;
    float alpha;
};
// resizeArea_'s four tap tables on the device (area_tab: xtab built with cn, ytab with 1; xofs / yofs the CSR offsets of
// the taps of every destination column / row)
struct AreaTaps {
    const AreaTap *xtab = nullptr, *ytab = nullptr;
    const int32_t *xofs = nullptr, *yofs = nullptr;
};

// The images of one launch: image i at src + i * scan_stride, srows x scols pixels of cn channels, its result
// (drows x dcols) at dst + i * out_stride.  kx, ky and the tables are the launcher's to fill in.
struct ResizeImgs {
    const uint8_t *src;
    int64_t scan_stride, sstep;
    uint8_t *dst;
    int64_t out_stride, dstep;
    int cn, srows, scols, drows, dcols;
    int kx, ky;  // AREA_INT: the integer factors (resizeAreaFast_)
    AreaTaps t;  // AREA_GENERAL
};

// How the INTER_AREA tile kernel tiles one image: a workgroup takes twp destination pixels x th destination rows and
// walks down their source rows, `chunk` rows at a time through LDS rows of `segd` dwords.  tiled = false: the segment
// of a single destination pixel does not fit (shrink factors in the thousands).
struct PfTiling {
    bool tiled = false;
    int twp = 0, th = 0, segd = 0, chunk = 0;
};
// Tile shape for a context (host, once): the widest tile whose source segment fits the LDS budget.  Fractional
// factors hand in the host copies of the tap tables; integer factors hand in NULL.
PfTiling pf_area_tiling(int cn, int dcols, int kx, const std::vector<AreaTap> *xtab, const std::vector<int32_t> *xofs,
                        const std::vector<AreaTap> *ytab);

// The resize that resize() dispatches to `d` (LINEAR, AREA_INT or AREA_GENERAL; COPY stays with the caller) for the n
// images of `im`, in one launch on `s`.  `taps`: the tables of AREA_GENERAL.  The caller chooses the INTER_AREA kernel:
//   tiling == NULL   one thread per destination byte straight from memory -- or, for gray images shrunk by one integer
//                    factor k on both axes, the LDS kernels of that case (k <= 16 from dword-aligned rows, else k <= 8)
//   tiling != NULL   the tile kernel (cn 1 or 3) with that tiling; one thread per destination byte when it says
//                    tiled = false
// hipErrorInvalidValue: COPY, n outside 1..65535, integer factors that do not divide the source exactly, missing tables.
hipError_t launch_resize(const ResizeDispatch &d, const ResizeImgs &im, int n, hipStream_t s, const AreaTaps &taps = AreaTaps(),
                         const PfTiling *tiling = nullptr);

}  // namespace omr
