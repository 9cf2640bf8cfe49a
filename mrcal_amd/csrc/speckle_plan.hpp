// What speckle_filter.hip works out on the host before it touches the device: the arguments that are refused, where
// the image, the labels and the counts lie in the ONE pooled allocation a stand-alone filter owns (the resident stereo
// matcher lends its aggregation volume instead: the labels and the counts alone, speckle_workspace_bytes()), the
// launch geometry of every kernel, and the refusal of an image that does not fit the device's free memory (the caller
// passes that figure in). Plain structs in and out, no HIP type or call.
// tests/hostcheck/speckle_plan_check.cpp runs it under the host sanitizers.
//
// What the filter is: include/mrcal_amd.h, "filter_speckles".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "image_format.hpp"

namespace mrcal_amd {

// the tile of pixels a workgroup of speckle_label_tile_kernel labels in LDS: a wavefront a row, 4 rows each
#define SPECKLE_TILE_X 64
#define SPECKLE_TILE_Y 16
#define SPECKLE_THREADS 256         // of every kernel
#define SPECKLE_MAX_DIFF 65535      // the largest difference two int16 can have: a larger max_diff means this
#define SPECKLE_ALIGN 256           // of the parts of the pool, in bytes

struct SpeckleParams
{
    int new_value, max_speckle_size, max_diff;
};

// where the work is, for an image of W x H: the same for the stand-alone filter and inside the matcher
struct SpeckleGrids
{
    int      W = 0, H = 0;
    unsigned tiles_x = 0, tiles_y = 0;      // the tiles each way; speckle_label_tile_kernel: a workgroup a tile, in ONE dimension
    // the pixels that have a neighbour in another tile: first those below a horizontal border ((tiles_y - 1) W of
    // them), then those right of a vertical one ((tiles_x - 1) H). speckle_merge_borders_kernel: a lane each
    size_t   border_pixels = 0;
    unsigned tile_grid = 0, border_grid = 0, pixel_grid = 0;       // pixel_grid: a lane a pixel (flatten and count; apply)
};

struct SpecklePlan
{
    SpeckleGrids grids;
    // offsets into the pool, in bytes
    size_t image = 0;                       // int16 a pixel, filtered in place
    size_t label = 0, count = 0;            // int32 a pixel each, side by side
    size_t bytes = 0;                       // of the pool
};

inline size_t speckle_aligned(size_t n) { return (n + SPECKLE_ALIGN - 1)/SPECKLE_ALIGN*SPECKLE_ALIGN; }
// the labels and, right behind them, the counts: 8 bytes a pixel, with no padding in between
inline size_t speckle_workspace_bytes(size_t N) { return 2*N*sizeof(int32_t); }
inline size_t speckle_count_offset(size_t N)    { return N*sizeof(int32_t); }

// the arguments that cannot be filtered, for whatever data: false, and why
inline bool speckle_params_ok(std::string* error, int W, int H, long new_value, long max_speckle_size, long max_diff)
{
    char buf[256];
    buf[0] = 0;
    if(!image_size_ok(W, H))
        snprintf(buf, sizeof(buf), "filter_speckles(): images of %d x %d pixels cannot be filtered", W, H);
    else if(new_value < INT16_MIN || new_value > INT16_MAX)
        snprintf(buf, sizeof(buf), "filter_speckles(): new_value must be in %d..%d. Got %ld", INT16_MIN, INT16_MAX, new_value);
    else if(max_speckle_size < 0)
        snprintf(buf, sizeof(buf), "filter_speckles(): max_speckle_size must be a non-negative integer. Got %ld", max_speckle_size);
    else if(max_diff < 0)
        snprintf(buf, sizeof(buf), "filter_speckles(): max_diff must be a non-negative integer. Got %ld", max_diff);
    if(buf[0] == 0) return true;
    *error = buf;
    return false;
}

// what the matcher's two keywords mean: new_value = 16 (disparity_min - 1), max_diff = 16 speckle_range
inline bool speckle_params_of_matcher(SpeckleParams* p, std::string* error, int disparity_min, int disparity_scale,
                                      long speckle_window_size, long speckle_range)
{
    char buf[256];
    buf[0] = 0;
    if(speckle_window_size < 0)
        snprintf(buf, sizeof(buf), "filter_speckles(): speckle_window_size must be a non-negative integer. Got %ld", speckle_window_size);
    else if(speckle_range < 0)
        snprintf(buf, sizeof(buf), "filter_speckles(): speckle_range must be a non-negative integer. Got %ld", speckle_range);
    if(buf[0] != 0) { *error = buf; return false; }
    p->new_value        = disparity_scale*(disparity_min - 1);
    p->max_speckle_size = (int)(speckle_window_size < INT32_MAX ? speckle_window_size : INT32_MAX);
    p->max_diff         = speckle_range >= SPECKLE_MAX_DIFF/disparity_scale + 1 ? SPECKLE_MAX_DIFF : (int)(disparity_scale*speckle_range);
    return true;
}

// the arguments as the kernels take them: a region has at most 2^28 pixels and two int16 differ by at most 65535
inline SpeckleParams speckle_params(long new_value, long max_speckle_size, long max_diff)
{
    SpeckleParams p;
    p.new_value        = (int)new_value;
    p.max_speckle_size = (int)(max_speckle_size < INT32_MAX ? max_speckle_size : INT32_MAX);
    p.max_diff         = (int)(max_diff < SPECKLE_MAX_DIFF ? max_diff : SPECKLE_MAX_DIFF);
    return p;
}

// W, H: in order (speckle_params_ok())
inline SpeckleGrids speckle_grids(int W, int H)
{
    SpeckleGrids g;
    g.W = W; g.H = H;
    const size_t N = (size_t)W*(size_t)H;
    g.tiles_x = (unsigned)((W + SPECKLE_TILE_X - 1)/SPECKLE_TILE_X);
    g.tiles_y = (unsigned)((H + SPECKLE_TILE_Y - 1)/SPECKLE_TILE_Y);
    g.border_pixels = (size_t)(g.tiles_y - 1)*(size_t)W + (size_t)(g.tiles_x - 1)*(size_t)H;
    g.tile_grid   = g.tiles_x*g.tiles_y;
    g.border_grid = (unsigned)((g.border_pixels + SPECKLE_THREADS - 1)/SPECKLE_THREADS);
    g.pixel_grid  = (unsigned)((N + SPECKLE_THREADS - 1)/SPECKLE_THREADS);
    return g;
}

// the whole plan of a stand-alone filter. free_bytes: what the device has free. false: a refusal, with the reason in *error
inline bool speckle_plan(SpecklePlan* plan, std::string* error, int W, int H, size_t free_bytes)
{
    *plan = SpecklePlan();
    if(!speckle_params_ok(error, W, H, 0, 0, 0)) return false;
    const size_t N = (size_t)W*(size_t)H;
    plan->image = 0;
    plan->label = speckle_aligned(N*sizeof(int16_t));
    plan->count = plan->label + speckle_count_offset(N);
    plan->bytes = plan->label + speckle_aligned(speckle_workspace_bytes(N));
    if(plan->bytes > free_bytes)
    {
        char buf[256];
        snprintf(buf, sizeof(buf), "filter_speckles(): %d x %d pixels need %zu bytes of device memory; %zu are free",
                 W, H, plan->bytes, free_bytes);
        *error = buf;
        *plan = SpecklePlan();
        return false;
    }
    plan->grids = speckle_grids(W, H);
    return true;
}

} // namespace mrcal_amd
