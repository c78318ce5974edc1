// rr_contrib.hpp — argument block and launchers of the per-Gaussian blend-contribution statistics
// (rr_contrib.hip; include/rain_raster.h rr_contributions).
#pragma once
#include "rr_common.hpp"

namespace rr {

struct ContribArgs {
    int P, W, H, gx, gy;
    const uint2* ranges;
    const uint2* ranges_b;  // phase-B lists (all {0,0} for single-phase binning)
    const uint32_t* point_list;
    const Splat* splats;
    const uint32_t* tile_max;
    const uint32_t* n_contrib;
    const float* pixel_weight;  // [H*W] or null (1 everywhere)
    uint32_t* out;              // [P][4]: sum_w, sum_gw, max_w (float bits), count
};
void launch_contrib_clear(uint32_t* out, int P, hipStream_t st);  // every record of out to zeros
void launch_contrib(const ContribArgs& a, hipStream_t st);        // adds the frame into out

}  // namespace rr
