// stereo_point_cloud(): the disparities of a rectified pair to a compacted, coloured cloud of points
// (include/mrcal_amd.h, "stereo_point_cloud": the definition, to the bit). The tree's stream compaction.
//
//   cloud_mask_kernel      decides ONCE which pixels are kept. A lane owns 4 consecutive pixels in memory: one 8-byte
//                          load of the disparities and, with a colour image, two 16-byte loads of the map. The four
//                          tests (disparity, range, range limits, colour pixel); the range is worked out here for them.
//                          A wavefront's verdicts are four __ballot words, lane-major; lanes 0..3 interleave them into
//                          the four PIXEL-major 64-bit mask words of the wavefront's 256 pixels (bit b of word w is
//                          pixel 64 w + b) and store them. The workgroup stores the popcount of its 16 words
//   cloud_scan_kernel      ONE workgroup: every thread sums its share of the counts serially, an inclusive scan of the
//                          threads' sums in LDS, then every thread writes the exclusive bases of its share; the last
//                          entry is the total N, which the host reads (4 bytes) to size the outputs
//   cloud_scatter_kernel   a workgroup the same 1024 pixels, a lane a pixel, a wavefront a mask word at a time. The rank
//                          of a kept pixel: the workgroup's base, the popcounts of the workgroup's words before its own,
//                          the set bits below its lane. Only kept lanes work out the point (the range again, from the
//                          same __device__ source and the same operands: the same bits), the colour pixel and the
//                          three stores. The mask is read, never decided again
// The bookkeeping is integer arithmetic; no atomics of any kind, no flag and no look-back between workgroups: the same
// bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "stereo_range_device.hpp"
#include "point_cloud_plan.hpp"
#include "point_cloud.hpp"

namespace mrcal_amd {

namespace {

struct CloudArgs
{
    RangeArgs range;
    int       N, W;                     // the pixels of the disparity image, its width
    double    disparity_scale;
    int       dmin, dmax;               // in the units of the disparity image
    double    range_min, range_max;
    int       color;                    // a colour image is given: the colour-pixel test is made
    int       image_W, image_H;
    int       transform;                // p = R p_rect0 + t is made
    double    R[9], t[3];
    unsigned  capacity;                 // records the output buffers hold
};

// The disparity test, the range test and the range limits: the range of a pixel that passes all three, 0 of one that
// does not (stereo_range_one() gives 0 for a range that is not finite)
__device__ __forceinline__ double cloud_range(int d, int col, int row, const CloudArgs& a)
{
    if(d <= 0 || d < a.dmin || d > a.dmax) return 0.0;
    const double r = stereo_range_one((double)d/a.disparity_scale, (double)col, (double)row, a.range);
    return (r > 0.0 && r >= a.range_min && r <= a.range_max) ? r : 0.0;
}

// The pixel of the colour image the map entry (mx, my) means: the nearest one, a half rounding up. false: outside the
// image, or not a number
__device__ __forceinline__ bool cloud_color_pixel(int* ix, int* iy, float mx, float my, int W, int H)
{
    const float x = floorf(mx + 0.5f), y = floorf(my + 0.5f);
    const bool in = x >= 0.f && x < (float)W && y >= 0.f && y < (float)H;
    *ix = in ? (int)x : 0;
    *iy = in ? (int)y : 0;
    return in;
}

// bit i of the low 16 bits of x moves to bit 4 i
__device__ __forceinline__ uint64_t cloud_spread4(uint64_t x)
{
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x <<  6)) & 0x0303030303030303ull;
    x = (x | (x <<  3)) & 0x1111111111111111ull;
    return x;
}

__global__ __launch_bounds__(CLOUD_THREADS)
void cloud_mask_kernel(CloudArgs a, const uint16_t* __restrict__ disparity, const float* __restrict__ map,
                       uint64_t* __restrict__ words, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t wave_count[CLOUD_THREADS/64];
    const int i0 = CLOUD_PIXELS_PER_LANE*(blockIdx.x*CLOUD_THREADS + threadIdx.x);
    int   d[4] = { 0, 0, 0, 0 };
    float m[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if(i0 + 4 <= a.N)
    {
        const uint2 dd = *(const uint2*)(disparity + i0);
        d[0] = dd.x & 0xFFFF; d[1] = dd.x >> 16; d[2] = dd.y & 0xFFFF; d[3] = dd.y >> 16;
        if(a.color)
        {
            const float4 m0 = *(const float4*)(map + 2*(size_t)i0), m1 = *(const float4*)(map + 2*(size_t)i0 + 4);
            m[0] = m0.x; m[1] = m0.y; m[2] = m0.z; m[3] = m0.w; m[4] = m1.x; m[5] = m1.y; m[6] = m1.z; m[7] = m1.w;
        }
    }
    else
    {
#pragma unroll
        for(int k=0;k<4;k++)
            if(i0 + k < a.N)
            {
                d[k] = disparity[i0 + k];
                if(a.color) { m[2*k] = map[2*(size_t)(i0 + k)]; m[2*k+1] = map[2*(size_t)(i0 + k) + 1]; }
            }
    }
    int row = i0 / a.W, col = i0 - row*a.W;
    uint64_t ballot[4];
#pragma unroll
    for(int k=0;k<4;k++)
    {
        bool keep = i0 + k < a.N && cloud_range(d[k], col, row, a) > 0.0;
        if(keep && a.color)
        {
            int ix, iy;
            keep = cloud_color_pixel(&ix, &iy, m[2*k], m[2*k+1], a.image_W, a.image_H);
        }
        ballot[k] = __ballot(keep);
        if(++col == a.W) { col = 0; row++; }
    }
    // lane j < 4: the mask word of the lanes 16 j .. 16 j + 15, whose pixels are consecutive
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if(lane < 4)
    {
        const int s = 16*lane;
        words[(size_t)blockIdx.x*CLOUD_WORDS_PER_GROUP + 4*wave + lane] =
             cloud_spread4(ballot[0] >> s)       | (cloud_spread4(ballot[1] >> s) << 1) |
            (cloud_spread4(ballot[2] >> s) << 2) | (cloud_spread4(ballot[3] >> s) << 3);
    }
    if(lane == 0)
        wave_count[wave] = __popcll(ballot[0]) + __popcll(ballot[1]) + __popcll(ballot[2]) + __popcll(ballot[3]);
    __syncthreads();
    if(threadIdx.x == 0)
    {
        uint32_t n = 0;
#pragma unroll
        for(int w=0; w<CLOUD_THREADS/64; w++) n += wave_count[w];
        counts[blockIdx.x] = n;
    }
}

// bases [groups + 1]: the exclusive scan of counts [groups], and their total
__global__ __launch_bounds__(CLOUD_SCAN_THREADS)
void cloud_scan_kernel(unsigned groups, unsigned per_thread, const uint32_t* __restrict__ counts, uint32_t* __restrict__ bases)
{
    __shared__ uint32_t sum[CLOUD_SCAN_THREADS];
    const unsigned t = threadIdx.x;
    const unsigned lo = t*per_thread < groups ? t*per_thread : groups;
    const unsigned hi = lo + per_thread < groups ? lo + per_thread : groups;
    uint32_t mine = 0;
    for(unsigned g=lo; g<hi; g++) mine += counts[g];
    sum[t] = mine;
    __syncthreads();
    for(unsigned step=1; step<CLOUD_SCAN_THREADS; step*=2)
    {
        const uint32_t add = t >= step ? sum[t - step] : 0;
        __syncthreads();
        sum[t] += add;
        __syncthreads();
    }
    uint32_t at = sum[t] - mine;
    for(unsigned g=lo; g<hi; g++) { bases[g] = at; at += counts[g]; }
    if(t == CLOUD_SCAN_THREADS - 1) bases[groups] = sum[t];
}

// P: double or float, the points as they are stored. T, C: the colour image's channel type and channels; C = 0: none
template<class P, class T, int C>
__global__ __launch_bounds__(CLOUD_THREADS)
void cloud_scatter_kernel(CloudArgs a, const uint16_t* __restrict__ disparity, const float* __restrict__ map,
                          const T* __restrict__ image, const uint64_t* __restrict__ words, const uint32_t* __restrict__ bases,
                          P* __restrict__ points, T* __restrict__ color, int32_t* __restrict__ index)
{
    __shared__ uint64_t word_of[CLOUD_WORDS_PER_GROUP];
    __shared__ uint32_t before[CLOUD_WORDS_PER_GROUP];
    const uint32_t base = bases[blockIdx.x];
    if(bases[blockIdx.x + 1] == base) return;           // (the whole workgroup: nothing is kept here)
    if(threadIdx.x < CLOUD_WORDS_PER_GROUP) word_of[threadIdx.x] = words[(size_t)blockIdx.x*CLOUD_WORDS_PER_GROUP + threadIdx.x];
    __syncthreads();
    if(threadIdx.x == 0)
    {
        uint32_t n = base;
        for(int q=0; q<CLOUD_WORDS_PER_GROUP; q++) { before[q] = n; n += __popcll(word_of[q]); }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for(int q=wave; q<CLOUD_WORDS_PER_GROUP; q+=CLOUD_THREADS/64)
    {
        const uint64_t word = word_of[q];
        if(!((word >> lane) & 1)) continue;
        const uint32_t rank = before[q] + __popcll(word & ((1ull << lane) - 1));
        if(rank >= a.capacity) continue;                // (cannot be: the total is the sum of these very words)
        const int i = blockIdx.x*CLOUD_SPAN + 64*q + lane;      // (< N: the bit is set)
        const int row = i / a.W, col = i - row*a.W;
        const double r = cloud_range((int)disparity[i], col, row, a);
        double v[3];
        stereo_unit_vector(v, (double)col, (double)row, a.range);
        double p[3];
        for(int k=0;k<3;k++) p[k] = r*v[k];
        if(a.transform)
        {
            const double x = p[0], y = p[1], z = p[2];
            p[0] = a.R[0]*x + a.R[1]*y + a.R[2]*z + a.t[0];
            p[1] = a.R[3]*x + a.R[4]*y + a.R[5]*z + a.t[1];
            p[2] = a.R[6]*x + a.R[7]*y + a.R[8]*z + a.t[2];
        }
        for(int k=0;k<3;k++) points[3*(size_t)rank + k] = (P)p[k];
        index[rank] = i;
        if constexpr (C > 0)
        {
            int ix, iy;
            (void)cloud_color_pixel(&ix, &iy, map[2*(size_t)i], map[2*(size_t)i + 1], a.image_W, a.image_H);
#pragma unroll
            for(int c=0;c<C;c++) color[(size_t)rank*C + c] = image[((size_t)iy*a.image_W + ix)*C + c];
        }
    }
}

} // namespace

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_point_cloud
{
    DeviceBuffers mem;
    uint8_t*      pool = NULL;
    CloudPlan     plan;
    RangeArgs     range_args;
    const float*  map = NULL;           // the rectification map of camera 0, on the device: the caller's, or own_map
    float*        own_map = NULL;
    // the outputs: `capacity` records of the largest kind each
    uint8_t*      points = NULL;
    uint8_t*      color = NULL;
    int32_t*      index = NULL;
    size_t        capacity = 0;
    // the last cloud
    int           N = -1;
    size_t        point_bytes = 0, color_bytes = 0;     // of a record's point, of its colour
    StageEvents<5> events;              // around the mask, after the scan, around the scatter
};

static bool cloud_given(const mrcal_amd_point_cloud* c)
{
    if(c != NULL) return true;
    set_error("stereo_point_cloud(): the point cloud object is NULL");
    return false;
}

namespace mrcal_amd {

template<class P>
static void cloud_launch_scatter(const mrcal_amd_point_cloud* c, const CloudArgs& a, const uint16_t* d_disparity,
                                 const void* d_image, int channels, int dtype)
{
    const uint64_t* words = (const uint64_t*)(c->pool + c->plan.words);
    const uint32_t* bases = (const uint32_t*)(c->pool + c->plan.bases);
    const dim3 grid(c->plan.groups), block(CLOUD_THREADS);
#define CLOUD_SCATTER(T, C) hipLaunchKernelGGL((cloud_scatter_kernel<P,T,C>), grid, block, 0, NULL, a, d_disparity, c->map, \
                                               (const T*)d_image, words, bases, (P*)c->points, (T*)c->color, c->index)
    if(channels == 0)                         CLOUD_SCATTER(uint8_t, 0);
    else if(dtype == MRCAL_AMD_IMAGE_UINT8) { if(channels == 1) CLOUD_SCATTER(uint8_t, 1);  else CLOUD_SCATTER(uint8_t, 3); }
    else                                    { if(channels == 1) CLOUD_SCATTER(uint16_t, 1); else CLOUD_SCATTER(uint16_t, 3); }
#undef CLOUD_SCATTER
}

bool point_cloud_compute_device(mrcal_amd_point_cloud_t* c, const uint16_t* d_disparity,
                                const mrcal_amd_point_cloud_params_t* params, int* N, const void* d_color_image)
{
    c->N = -1;
    c->events.timed = false;
    const mrcal_amd_point_cloud_params_t& rq = *params;
    const int channels = rq.image == NULL ? 0 : rq.image_channels != 0 ? rq.image_channels : -1;     // (an image of 0 channels is none, and refused)
    const int channel_bytes = rq.image_dtype == MRCAL_AMD_IMAGE_UINT8 ? 1 : rq.image_dtype == MRCAL_AMD_IMAGE_UINT16 ? 2 : 0;
    std::string why;
    if(!cloud_params_ok(&why, rq.disparity_scaled_min, rq.disparity_scaled_max, rq.range_min, rq.range_max, c->map != NULL,
                        rq.image_width, rq.image_height, channels, channel_bytes))
    {
        set_error("%s", why.c_str());
        return false;
    }
    if(((uintptr_t)d_disparity & 7) != 0) { set_error("stereo_point_cloud(): the disparities on the device must be aligned to 8 bytes"); return false; }

    const CloudPlan& plan = c->plan;
    CloudArgs a;
    memset(&a, 0, sizeof(a));
    a.range = c->range_args;
    a.N = plan.W*plan.H; a.W = plan.W;
    a.disparity_scale = (double)rq.disparity_scale;
    a.dmin = rq.disparity_scaled_min; a.dmax = rq.disparity_scaled_max;
    a.range_min = rq.range_min; a.range_max = rq.range_max;
    a.color = channels > 0;
    a.image_W = rq.image_width; a.image_H = rq.image_height;
    a.transform = rq.Rt_out_rect0 != NULL;
    if(a.transform)
    {
        for(int i=0;i<9;i++) a.R[i] = rq.Rt_out_rect0[i];
        for(int i=0;i<3;i++) a.t[i] = rq.Rt_out_rect0[9 + i];
    }

    // (the colour image goes when this returns: the work is waited for before that)
    DeviceBuffers tmp;
    uint8_t* d_uploaded = NULL;
    if(channels > 0 && d_color_image == NULL &&
       !tmp.upload(&d_uploaded, (const uint8_t*)rq.image, (size_t)rq.image_width*rq.image_height*channels*channel_bytes))
        return false;
    const void* d_image = d_color_image != NULL ? d_color_image : d_uploaded;

    uint64_t* words  = (uint64_t*)(c->pool + plan.words);
    uint32_t* counts = (uint32_t*)(c->pool + plan.counts);
    uint32_t* bases  = (uint32_t*)(c->pool + plan.bases);
    if(!c->events.record(0)) return false;
    hipLaunchKernelGGL(cloud_mask_kernel, dim3(plan.groups), dim3(CLOUD_THREADS), 0, NULL, a, d_disparity, c->map, words, counts);
    HIP_TRY(hipGetLastError(), return false);
    if(!c->events.record(1)) return false;
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(CLOUD_SCAN_THREADS), 0, NULL, plan.groups, plan.scan_per_thread, counts, bases);
    HIP_TRY(hipGetLastError(), return false);
    if(!c->events.record(2)) return false;
    uint32_t total = 0;
    // (the copy waits for the launches)
    HIP_TRY(hipMemcpy(&total, bases + plan.groups, sizeof(total), hipMemcpyDeviceToHost), (void)hipDeviceSynchronize(); return false);
    if((size_t)total > (size_t)a.N) { set_error("stereo_point_cloud(): internal error: %u points of %d pixels", total, a.N); return false; }

    const size_t capacity = cloud_capacity(c->capacity, total, (size_t)a.N);
    if(capacity != c->capacity)
    {
        c->mem.release(&c->points); c->mem.release(&c->color); c->mem.release(&c->index);
        c->capacity = 0;
        if(!(c->mem.alloc(&c->points, capacity*3*sizeof(double)) && c->mem.alloc(&c->color, capacity*3*sizeof(uint16_t)) &&
             c->mem.alloc(&c->index, capacity)))
        {
            c->mem.release(&c->points); c->mem.release(&c->color); c->mem.release(&c->index);
            return false;
        }
        c->capacity = capacity;
    }
    a.capacity = (unsigned)c->capacity;
    if(total > 0)
    {
        if(!c->events.record(3)) return false;
        if(rq.points_float32) cloud_launch_scatter<float> (c, a, d_disparity, d_image, channels, rq.image_dtype);
        else                  cloud_launch_scatter<double>(c, a, d_disparity, d_image, channels, rq.image_dtype);
        HIP_TRY(hipGetLastError(), (void)hipDeviceSynchronize(); return false);
        if(!c->events.record(4)) { (void)hipDeviceSynchronize(); return false; }
    }
    HIP_TRY(hipStreamSynchronize(NULL), return false);
    c->N = (int)total;
    c->point_bytes = 3*(rq.points_float32 ? sizeof(float) : sizeof(double));
    c->color_bytes = (size_t)channels*channel_bytes;
    c->events.timed = true;
    *N = c->N;
    return true;
}

} // namespace mrcal_amd

extern "C" {

mrcal_amd_point_cloud_t*
mrcal_amd_point_cloud_create(const mrcal_lensmodel_type_t rectification_model_type, const double* fxycxy_rectified,
                             double baseline, int width, int height, const float* device_map0)
{
    last_error_string().clear();
    if(!(rectification_model_type == MRCAL_LENSMODEL_LATLON || rectification_model_type == MRCAL_LENSMODEL_PINHOLE))
    {
        set_error("Invalid rectification_model_type for rectification: %d; I know about MRCAL_LENSMODEL_LATLON and MRCAL_LENSMODEL_PINHOLE", (int)rectification_model_type);
        return NULL;
    }
    std::string why;
    CloudPlan plan;
    // (the refusals that need no device first)
    if(!cloud_plan(&plan, &why, width, height, SIZE_MAX)) { set_error("%s", why.c_str()); return NULL; }
    if(((uintptr_t)device_map0 & 15) != 0) { set_error("stereo_point_cloud(): the map on the device must be aligned to 16 bytes"); return NULL; }
    if(!have_device()) return NULL;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return NULL);
    if(!cloud_plan(&plan, &why, width, height, free_bytes)) { set_error("%s", why.c_str()); return NULL; }

    mrcal_amd_point_cloud* c = new mrcal_amd_point_cloud;
    c->plan = plan;
    c->range_args.fx = fxycxy_rectified[0]; c->range_args.fy = fxycxy_rectified[1];
    c->range_args.cx = fxycxy_rectified[2]; c->range_args.cy = fxycxy_rectified[3];
    c->range_args.baseline = baseline;
    c->range_args.latlon   = rectification_model_type == MRCAL_LENSMODEL_LATLON;
    c->map = device_map0;
    if(!c->mem.alloc(&c->pool, plan.bytes)) { delete c; return NULL; }
    if(!c->events.create()) { delete c; return NULL; }
    return c;
}

bool mrcal_amd_point_cloud_set_map(mrcal_amd_point_cloud_t* c, const float* map0)
{
    last_error_string().clear();
    if(!cloud_given(c) || !have_device()) return false;
    if(map0 == NULL) { set_error("stereo_point_cloud(): the map is NULL"); return false; }
    const size_t n = (size_t)2*c->plan.W*c->plan.H;
    if(c->own_map == NULL && !c->mem.alloc(&c->own_map, n)) return false;
    HIP_TRY(hipMemcpy(c->own_map, map0, n*sizeof(float), hipMemcpyHostToDevice), return false);
    c->map = c->own_map;
    return true;
}

bool mrcal_amd_point_cloud_compute(mrcal_amd_point_cloud_t* c, const uint16_t* disparity_scaled,
                                   const mrcal_amd_point_cloud_params_t* params, int* N)
{
    last_error_string().clear();
    if(!cloud_given(c)) return false;
    if(disparity_scaled == NULL || params == NULL || N == NULL) { set_error("stereo_point_cloud(): an argument is NULL"); return false; }
    if(!have_device()) return false;
    c->N = -1;
    uint16_t* d_disparity = (uint16_t*)(c->pool + c->plan.disparity);
    HIP_TRY(hipMemcpy(d_disparity, disparity_scaled, (size_t)c->plan.W*c->plan.H*sizeof(uint16_t), hipMemcpyHostToDevice), return false);
    return point_cloud_compute_device(c, d_disparity, params, N);
}

bool mrcal_amd_point_cloud_read(mrcal_amd_point_cloud_t* c, void* points, void* color, int32_t* index)
{
    last_error_string().clear();
    if(!cloud_given(c)) return false;
    if(c->N < 0) { set_error("stereo_point_cloud(): no cloud has been computed yet"); return false; }
    if(color != NULL && c->color_bytes == 0) { set_error("stereo_point_cloud(): the cloud was computed without a colour image"); return false; }
    const size_t N = (size_t)c->N;
    if(N == 0) return true;
    if(points != NULL) HIP_TRY(hipMemcpy(points, c->points, N*c->point_bytes, hipMemcpyDeviceToHost), return false);
    if(color  != NULL) HIP_TRY(hipMemcpy(color,  c->color,  N*c->color_bytes, hipMemcpyDeviceToHost), return false);
    if(index  != NULL) HIP_TRY(hipMemcpy(index,  c->index,  N*sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    return true;
}

bool mrcal_amd_point_cloud_stage_milliseconds(mrcal_amd_point_cloud_t* c, float* milliseconds)
{
    last_error_string().clear();
    if(!cloud_given(c)) return false;
    if(!c->events.timed) { set_error("stereo_point_cloud(): no cloud has been computed yet"); return false; }
    if(!c->events.elapsed(&milliseconds[0], 0, 1) || !c->events.elapsed(&milliseconds[1], 1, 2)) return false;
    milliseconds[2] = 0.f;              // (an empty cloud: nothing was scattered)
    return c->N == 0 || c->events.elapsed(&milliseconds[2], 3, 4);
}

void mrcal_amd_point_cloud_destroy(mrcal_amd_point_cloud_t* c) { delete c; }

} // extern "C"
