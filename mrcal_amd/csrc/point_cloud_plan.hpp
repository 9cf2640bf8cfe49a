// What point_cloud.hip works out on the host before it touches the device: the arguments that are refused, where the
// disparities, the mask words, the per-workgroup counts and the bases lie in the ONE pooled allocation a point-cloud
// object owns, the launch geometry of the three kernels, how the output buffers grow, and the refusal of an image that
// is too large or does not fit the device's free memory (the caller passes that figure in). Plain structs in and out,
// no HIP type or call. tests/hostcheck/point_cloud_plan_check.cpp runs it under the host sanitizers.
//
// What a cloud is: include/mrcal_amd.h, "stereo_point_cloud".
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "image_format.hpp"

namespace mrcal_amd {

#define CLOUD_THREADS 256               // of cloud_mask_kernel and cloud_scatter_kernel
#define CLOUD_PIXELS_PER_LANE 4         // consecutive in memory: one 8-byte load of the disparities
#define CLOUD_SPAN (CLOUD_THREADS*CLOUD_PIXELS_PER_LANE)       // the pixels of a workgroup: 1024
#define CLOUD_WORDS_PER_GROUP (CLOUD_SPAN/64)                   // 64-bit mask words a workgroup: bit b of word w is pixel 64 w + b
#define CLOUD_SCAN_THREADS 1024         // cloud_scan_kernel is ONE workgroup of these
#define CLOUD_SCAN_MAX_PER_THREAD 256   // counts a thread of it sums serially, at most
#define CLOUD_MAX_PIXELS IMAGE_MAX_PIXELS     // (the name point_cloud_plan_check.cpp asks by)
#define CLOUD_ALIGN 256                 // of the parts of the pool, in bytes
#define CLOUD_CAPACITY_STEP 4096        // the output buffers hold a multiple of this many records

// At the largest image the count array still fits the one workgroup of the scan: a thread sums at most
// CLOUD_SCAN_MAX_PER_THREAD counts serially, and the tree over the threads' sums does the rest. And the total, at most
// a count a pixel, fits the uint32 it is summed in with room to spare
static_assert(IMAGE_MAX_PIXELS/CLOUD_SPAN <= (long)CLOUD_SCAN_THREADS*CLOUD_SCAN_MAX_PER_THREAD, "the scan is one workgroup");
static_assert(IMAGE_MAX_PIXELS < (1L << 31), "a rank is an int32");
static_assert(CLOUD_SPAN % 64 == 0 && CLOUD_THREADS % 64 == 0, "whole wavefronts, whole words");

struct CloudPlan
{
    int      W = 0, H = 0;
    unsigned groups = 0;                // workgroups of the mask and of the scatter kernel: a span each
    unsigned scan_per_thread = 0;       // counts a thread of the scan sums: groups <= CLOUD_SCAN_THREADS scan_per_thread
    // offsets into the pool, in bytes
    size_t   disparity = 0;             // uint16 a pixel
    size_t   words = 0;                 // uint64 [groups CLOUD_WORDS_PER_GROUP]: whole workgroups, the tail's bits 0
    size_t   counts = 0;                // uint32 [groups]
    size_t   bases = 0;                 // uint32 [groups + 1]: the exclusive scan of the counts, and the total N
    size_t   bytes = 0;                 // of the pool
};

inline size_t cloud_aligned(size_t n) { return (n + CLOUD_ALIGN - 1)/CLOUD_ALIGN*CLOUD_ALIGN; }

// the whole plan. free_bytes: what the device has free. false: a refusal, with the reason in *error
inline bool cloud_plan(CloudPlan* plan, std::string* error, int W, int H, size_t free_bytes)
{
    *plan = CloudPlan();
    char buf[256];
    if(!image_size_ok(W, H))
    {
        snprintf(buf, sizeof(buf), "stereo_point_cloud(): a disparity image of %d x %d pixels cannot be made a cloud of: at most %ld pixels",
                 W, H, IMAGE_MAX_PIXELS);
        *error = buf;
        return false;
    }
    const size_t N = (size_t)W*(size_t)H;
    CloudPlan p;
    p.W = W; p.H = H;
    p.groups          = (unsigned)((N + CLOUD_SPAN - 1)/CLOUD_SPAN);
    p.scan_per_thread = (p.groups + CLOUD_SCAN_THREADS - 1)/CLOUD_SCAN_THREADS;
    p.disparity = 0;
    p.words     = cloud_aligned(N*sizeof(uint16_t));
    p.counts    = p.words  + cloud_aligned((size_t)p.groups*CLOUD_WORDS_PER_GROUP*sizeof(uint64_t));
    p.bases     = p.counts + cloud_aligned((size_t)p.groups*sizeof(uint32_t));
    p.bytes     = p.bases  + cloud_aligned(((size_t)p.groups + 1)*sizeof(uint32_t));
    if(p.bytes > free_bytes)
    {
        snprintf(buf, sizeof(buf), "stereo_point_cloud(): %d x %d pixels need %zu bytes of device memory; %zu are free",
                 W, H, p.bytes, free_bytes);
        *error = buf;
        return false;
    }
    *plan = p;
    return true;
}

// How many records the output buffers hold once a cloud of N points of an image of `pixels` pixels has to fit, when
// they hold `capacity` now. They never shrink; they grow to N and a quarter more, in whole steps, and never beyond the
// image (N <= pixels)
inline size_t cloud_capacity(size_t capacity, size_t N, size_t pixels)
{
    if(N <= capacity) return capacity;
    size_t want = N + N/4;
    want = (want + CLOUD_CAPACITY_STEP - 1)/CLOUD_CAPACITY_STEP*CLOUD_CAPACITY_STEP;
    return want < pixels ? want : pixels;
}

// the arguments of a cloud that cannot be computed, for whatever data: false, and why.
// have_map: the object holds the rectification map of camera 0; image_*: 0 channels means no colour image
inline bool cloud_params_ok(std::string* error, long disparity_scaled_min, long disparity_scaled_max,
                            double range_min, double range_max, bool have_map,
                            int image_width, int image_height, int image_channels, int image_bytes_per_channel)
{
    char buf[256];
    buf[0] = 0;
    if(disparity_scaled_min >= disparity_scaled_max)
        snprintf(buf, sizeof(buf), "stereo_point_cloud(): must have disparity_scaled_max > disparity_scaled_min. Got %ld and %ld",
                 disparity_scaled_max, disparity_scaled_min);
    else if(!(range_min <= range_max))      // (a NaN too)
        snprintf(buf, sizeof(buf), "stereo_point_cloud(): must have range_min <= range_max. Got %g and %g", range_min, range_max);
    else if(image_channels != 0)
    {
        if(!(image_channels == 1 || image_channels == 3))
            snprintf(buf, sizeof(buf), "stereo_point_cloud(): a colour image has 1 or 3 channels, not %d", image_channels);
        else if(!(image_bytes_per_channel == 1 || image_bytes_per_channel == 2))
            snprintf(buf, sizeof(buf), "stereo_point_cloud(): a colour image is uint8 or uint16");
        else if(image_width <= 0 || image_height <= 0 || (long)image_width*image_height > (1L << 30) ||
                image_width >= (1 << 24) || image_height >= (1 << 24))      // (a pixel index is exact in float32)
            snprintf(buf, sizeof(buf), "stereo_point_cloud(): a colour image of %d x %d pixels cannot be read", image_width, image_height);
        else if(!have_map)
            snprintf(buf, sizeof(buf), "stereo_point_cloud(): a colour image needs the rectification map of camera 0, and none was given");
    }
    if(buf[0] == 0) return true;
    *error = buf;
    return false;
}

} // namespace mrcal_amd
