// What stereo_sgm.hip works out on the host before it touches the device: the parameters that are refused, where the
// images, the two census images, the aggregation volume S and the per-pixel results lie in the ONE pooled allocation
// a matcher owns, the launch geometry of every kernel, and the refusal of a problem that does not fit the device's
// free memory (the caller passes that figure in). Plain structs in and out, no HIP type or call.
// tests/hostcheck/sgm_plan_check.cpp runs it under the host sanitizers.
//
// What a disparity image is: include/mrcal_amd.h, "stereo_matching_sgm".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "image_format.hpp"

namespace mrcal_amd {

#define SGM_DISPARITY_SCALE 16
// the census window, and the tile of pixels a workgroup of sgm_census_kernel covers (64 x 4 threads, 4 rows each)
#define SGM_CENSUS_RX 4
#define SGM_CENSUS_RY 3
#define SGM_CENSUS_TILE_X 64
#define SGM_CENSUS_TILE_Y 16
// a path (and, in the selection, a pixel) is carried by 16 lanes, a DPP row, each with D/16 consecutive disparities in
// registers: 4 paths a wavefront, and a wavefront a workgroup
#define SGM_LANES 16
#define SGM_WAVE_PATHS 4
#define SGM_PATH_THREADS 64
// the selection: 256 threads, 16 pixels a workgroup; the left-right check: a lane a pixel
#define SGM_SELECT_THREADS 256
#define SGM_SELECT_PIXELS (SGM_SELECT_THREADS/SGM_LANES)
#define SGM_CHECK_THREADS 256
#define SGM_MAX_D 256
#define SGM_MAX_P2 193          // 62 + P2 <= 255: L is a byte, S = sum of 8 of them 16 bits
#define SGM_ALIGN 256           // of every part of the pool, in bytes

struct SgmParams
{
    int disparity_min, disparity_max, P1, P2, paths, uniqueness_ratio, disp12_max_diff;
};

struct SgmPlan
{
    int    W = 0, H = 0, D = 0, dtype = 0;
    int    per_lane = 0;                    // D/16: the disparities a lane holds
    // offsets into the pool, in bytes, each a multiple of SGM_ALIGN
    size_t image[2]  = { 0, 0 };            // the two images on the device (W H pixels)
    size_t census[2] = { 0, 0 };            // uint64 a pixel
    size_t S = 0;                           // uint16 [H][W][D]
    size_t index_left = 0, index_right = 0; // uint8 a pixel: i* of the left image, i1 of the right one
    size_t disparity = 0;                   // int16 a pixel
    size_t bytes = 0;                       // of the pool
    // grids; the blocks are the constants above
    unsigned census_grid[2] = { 0, 0 };
    unsigned path_grid_horizontal = 0;      // a path a row
    unsigned path_grid_vertical = 0;        // a path a column (the diagonals too: they wrap around the image's sides)
    unsigned select_grid = 0, check_grid = 0;
};

inline size_t sgm_pixel_bytes(int dtype) { return image_pixel_bytes(dtype); }     // (the name sgm_plan_check.cpp asks by)
inline size_t sgm_aligned(size_t n) { return (n + SGM_ALIGN - 1)/SGM_ALIGN*SGM_ALIGN; }

// the parameters that cannot be matched, for whatever data: false, and why
inline bool sgm_params_ok(std::string* error, int W, int H, int dtype, const SgmParams& p)
{
    char buf[256];
    buf[0] = 0;
    const long D = (long)p.disparity_max - (long)p.disparity_min;
    if(!image_dtype_is_integer(dtype))
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): images are uint8 or uint16");
    else if(!image_size_ok(W, H))
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): images of %d x %d pixels cannot be matched", W, H);
    else if(D <= 0 || D > SGM_MAX_D || D % 16 != 0)
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): disparity_max - disparity_min must be a positive multiple of 16, at most %d. Got %ld",
                 SGM_MAX_D, D);
    else if(!(0 <= p.P1 && p.P1 <= p.P2 && p.P2 <= SGM_MAX_P2))
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): must have 0 <= P1 <= P2 <= %d. Got P1 = %d, P2 = %d", SGM_MAX_P2, p.P1, p.P2);
    else if(!(p.paths == 4 || p.paths == 8))
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): paths must be 4 or 8. Got %d", p.paths);
    else if(p.uniqueness_ratio < 0 || p.uniqueness_ratio > 99)
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): uniqueness_ratio must be in 0..99. Got %d", p.uniqueness_ratio);
    else if(SGM_DISPARITY_SCALE*((long)p.disparity_min - 1) < INT16_MIN || SGM_DISPARITY_SCALE*(long)p.disparity_max > INT16_MAX)
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): disparities %d..%d scaled by %d leave int16 (at most %d..%d)",
                 p.disparity_min, p.disparity_max, SGM_DISPARITY_SCALE, INT16_MIN/SGM_DISPARITY_SCALE + 1, INT16_MAX/SGM_DISPARITY_SCALE);
    if(buf[0] == 0) return true;
    *error = buf;
    return false;
}

// the whole plan. free_bytes: what the device has free. false: a refusal, with the reason in *error
inline bool sgm_plan(SgmPlan* plan, std::string* error, int W, int H, int dtype, const SgmParams& p, size_t free_bytes)
{
    *plan = SgmPlan();
    if(!sgm_params_ok(error, W, H, dtype, p)) return false;
    plan->W = W; plan->H = H; plan->dtype = dtype;
    plan->D = p.disparity_max - p.disparity_min;
    plan->per_lane = plan->D/SGM_LANES;
    const size_t N = (size_t)W*(size_t)H;
    size_t at = 0;
    for(int i = 0; i < 2; i++) { plan->image[i]  = at; at += sgm_aligned(N*image_pixel_bytes(dtype)); }
    for(int i = 0; i < 2; i++) { plan->census[i] = at; at += sgm_aligned(N*sizeof(uint64_t)); }
    plan->S           = at; at += sgm_aligned(N*(size_t)plan->D*sizeof(uint16_t));
    plan->index_left  = at; at += sgm_aligned(N);
    plan->index_right = at; at += sgm_aligned(N);
    plan->disparity   = at; at += sgm_aligned(N*sizeof(int16_t));
    plan->bytes = at;
    if(plan->bytes > free_bytes)
    {
        char buf[256];
        snprintf(buf, sizeof(buf), "stereo_matching_sgm(): %d x %d pixels with %d disparities need %zu bytes of device memory; %zu are free",
                 W, H, plan->D, plan->bytes, free_bytes);
        *error = buf;
        *plan = SgmPlan();
        return false;
    }
    plan->census_grid[0] = (unsigned)((W + SGM_CENSUS_TILE_X - 1)/SGM_CENSUS_TILE_X);
    plan->census_grid[1] = (unsigned)((H + SGM_CENSUS_TILE_Y - 1)/SGM_CENSUS_TILE_Y);
    plan->path_grid_horizontal = (unsigned)((H + SGM_WAVE_PATHS - 1)/SGM_WAVE_PATHS);
    plan->path_grid_vertical   = (unsigned)((W + SGM_WAVE_PATHS - 1)/SGM_WAVE_PATHS);
    plan->select_grid = (unsigned)((N + SGM_SELECT_PIXELS - 1)/SGM_SELECT_PIXELS);
    plan->check_grid  = (unsigned)((N + SGM_CHECK_THREADS - 1)/SGM_CHECK_THREADS);
    return true;
}

} // namespace mrcal_amd
