// filter_speckles(): connected regions of similar disparity that are too small to be a surface become invalid
// (include/mrcal_amd.h, "filter_speckles": the definition, to the bit; cv2.filterSpeckles() for CV_16S).
//
// Connected-component labelling by union-find. A label is the int32 linear index of a pixel of the same region that is
// not larger than the pixel's own; a root is a pixel that labels itself. Two roots are only ever joined by pointing the
// LARGER at the smaller, so a label only ever decreases, every loop below ends, and the root of a finished region is
// its smallest index whatever the order of execution: the labelling, the sizes and the output are the same bits on
// every call.
//
//   speckle_label_tile_kernel      a workgroup a tile of 64 x 16 pixels, a wavefront a row at a time. The row's runs
//                                  from one ballot (a pixel starts at the label of its run's first pixel), then the
//                                  vertical joins by union-find in LDS, then every pixel's label flattened to the
//                                  tile's root and written out as a global index. The sizes of the tile's regions are
//                                  summed in LDS, ONE integer atomicAdd a run of equal roots in a row, and written out
//                                  at the tile's roots (0 at every other pixel)
//   speckle_merge_borders_kernel   a lane a pixel that has a neighbour across a tile border: lock-free union-find in
//                                  global memory (atomicMin on labels)
//   speckle_count_kernel           a lane a pixel: the label flattened to the region's root and stored; a tile's root
//                                  that is not the region's adds its size to the region's: one global atomicAdd a tile
//                                  and region. (One a run of a wavefront's 64 pixels, the form before this one, took
//                                  2.2 ms at 6016 x 4016, hundreds of thousands of adds to the one address of a region
//                                  of millions of pixels; this one 0.33 ms: profiles/f11_speckle_filter.txt)
//   speckle_apply_kernel           a lane a pixel: new_value where count[root] <= max_speckle_size
// A join that three others imply is left out: where a pixel, its left neighbour, and the two above them are joined
// left-right twice and up-down once on the left, the up-down join on the right follows. Inside a tile and along a
// border that takes a run's vertical joins from one a pixel to one a run.
// No workgroup waits for another; integer atomics whose result does not depend on the order; no floating point.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "speckle_plan.hpp"
#include "speckle_filter.hpp"

namespace mrcal_amd {

namespace {

struct SpeckleArgs { int W, H, new_value, max_diff; };

#define SPECKLE_NO_PART (1 << 20)       // what a pixel that takes no part holds: further than 65535 from every int16

// a, b: values, or SPECKLE_NO_PART. The difference in 32 bits
__device__ __forceinline__ bool speckle_joined(int a, int b, int max_diff)
{
    return a != SPECKLE_NO_PART && b != SPECKLE_NO_PART && abs(a - b) <= max_diff;
}

__device__ __forceinline__ int speckle_load(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// The root of a. Ends: the label of a pixel that is no root is smaller than its index, so a decreases every turn.
// On the way a's label moves to its label's label: what is stored is a smaller index of the same region
__device__ __forceinline__ int speckle_find(int32_t* label, int a)
{
    for(;;)
    {
        const int l = speckle_load(&label[a]);
        if(l == a) return a;
        const int ll = speckle_load(&label[l]);
        if(ll == l) return l;
        atomicMin(&label[a], ll);
        a = ll;
    }
}

// Joins the regions of a and b. Ends: each turn either finishes or goes on from a label that is smaller than the root
// it has just failed to claim, and a label only ever decreases (atomicMin), with 0 as the least
__device__ __forceinline__ void speckle_union(int32_t* label, int a, int b)
{
    for(;;)
    {
        a = speckle_find(label, a);
        b = speckle_find(label, b);
        if(a == b) return;
        if(a < b) { const int t = a; a = b; b = t; }
        // a > b: a, a root when it was read, is pointed at b. If another lane pointed it elsewhere since (old < a),
        // label[a] now holds the smaller of the two, and the other one still has to meet it
        const int old = atomicMin(&label[a], b);
        if(old == a) return;
        a = old;
    }
}

////////////////////////////////////////////////////////////////////////////////
// a tile in LDS
////////////////////////////////////////////////////////////////////////////////
__global__ __launch_bounds__(SPECKLE_THREADS)
void speckle_label_tile_kernel(SpeckleArgs a, unsigned tiles_x, const int16_t* __restrict__ image,
                               int32_t* __restrict__ label, int32_t* __restrict__ count)
{
    constexpr int TX = SPECKLE_TILE_X, TY = SPECKLE_TILE_Y, WAVES = SPECKLE_THREADS/64;
    __shared__ int     value[TY][TX];
    __shared__ int32_t local[TY*TX];
    __shared__ int32_t size[TY*TX];
    const int tile_y = (int)(blockIdx.x / tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y*tiles_x);
    const int x0 = tile_x*TX, y0 = tile_y*TY;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;

    // the values, and the runs of every row: a lane a pixel, a wavefront a row
#pragma unroll
    for(int k = 0; k < TY/WAVES; k++)
    {
        const int ry = wave + WAVES*k, y = y0 + ry;
        int v = SPECKLE_NO_PART;
        if(x < a.W && y < a.H)
        {
            const int pixel = image[(size_t)y*a.W + x];
            if(pixel != a.new_value) v = pixel;
        }
        const int  left        = __shfl_up(v, 1);
        const bool joined_left = lane > 0 && speckle_joined(v, left, a.max_diff);
        // the lanes at which a run begins (lane 0 among them): mine is the last of those at or before me
        const unsigned long long begins = __ballot(!joined_left);
        const int begin = 63 - __clzll((long long)(begins & (~0ull >> (63 - lane))));
        value[ry][lane]      = v;
        local[ry*TX + lane]  = ry*TX + begin;
        size[ry*TX + lane]   = 0;
    }
    __syncthreads();

    // the vertical joins
#pragma unroll
    for(int k = 0; k < TY/WAVES; k++)
    {
        const int ry = wave + WAVES*k;
        if(ry == 0) continue;
        const int v = value[ry][lane], up = value[ry-1][lane];
        if(!speckle_joined(v, up, a.max_diff)) continue;
        if(lane > 0)
        {
            const int left = value[ry][lane-1], upleft = value[ry-1][lane-1];
            if(speckle_joined(v, left, a.max_diff) && speckle_joined(left, upleft, a.max_diff) && speckle_joined(upleft, up, a.max_diff))
                continue;               // (implied: the lane to the left, or one further on, makes the join)
        }
        speckle_union(local, ry*TX + lane, (ry - 1)*TX + lane);
    }
    __syncthreads();

    // every pixel to its tile's root, and the sizes of the tile's regions: the first lane of a run of equal roots in a
    // row adds the run's length to its root's size, in LDS
    int root[TY/WAVES];
#pragma unroll
    for(int k = 0; k < TY/WAVES; k++)
    {
        const int ry = wave + WAVES*k;
        root[k] = value[ry][lane] != SPECKLE_NO_PART ? speckle_find(local, ry*TX + lane) : -1;      // (outside the image: no part)
        const int  before = __shfl_up(root[k], 1);
        const bool begins = lane == 0 || root[k] != before;
        const unsigned long long all = __ballot(begins);
        if(begins && root[k] >= 0)
        {
            const unsigned long long later = lane == 63 ? 0ull : all & (~0ull << (lane + 1));
            const int next = later != 0 ? __ffsll((long long)later) - 1 : 64;
            atomicAdd(&size[root[k]], next - lane);
        }
    }
    __syncthreads();

    // the labels as global indices: the tile's row-major order is the image's. count: the size of the tile's region at
    // its root in the tile, 0 elsewhere
#pragma unroll
    for(int k = 0; k < TY/WAVES; k++)
    {
        const int ry = wave + WAVES*k, y = y0 + ry;
        if(!(x < a.W && y < a.H)) continue;
        const size_t pixel = (size_t)y*a.W + x;
        label[pixel] = root[k] >= 0 ? (y0 + root[k]/TX)*a.W + x0 + root[k]%TX : -1;
        count[pixel] = root[k] == ry*TX + lane ? size[ry*TX + lane] : 0;
    }
}

////////////////////////////////////////////////////////////////////////////////
// across the tiles' borders
////////////////////////////////////////////////////////////////////////////////
__device__ __forceinline__ int speckle_value(const SpeckleArgs& a, const int16_t* image, int x, int y)
{
    const int v = image[(size_t)y*a.W + x];
    return v == a.new_value ? SPECKLE_NO_PART : v;
}

__global__ __launch_bounds__(SPECKLE_THREADS)
void speckle_merge_borders_kernel(SpeckleArgs a, unsigned tiles_y, size_t border_pixels,
                                  const int16_t* __restrict__ image, int32_t* label)
{
    const size_t t = (size_t)blockIdx.x*SPECKLE_THREADS + threadIdx.x;
    if(t >= border_pixels) return;
    const size_t below = (size_t)(tiles_y - 1)*(size_t)a.W;         // the pixels below a horizontal border
    int x, y, xn, yn;                                               // the pixel, and its neighbour across the border
    bool implied_possible;
    if(t < below)
    {
        const int b = (int)(t / a.W);
        x = (int)(t - (size_t)b*a.W); y = (b + 1)*SPECKLE_TILE_Y;
        xn = x; yn = y - 1;
        implied_possible = x % SPECKLE_TILE_X != 0;
    }
    else
    {
        const size_t u = t - below;
        const int b = (int)(u / a.H);
        y = (int)(u - (size_t)b*a.H); x = (b + 1)*SPECKLE_TILE_X;
        xn = x - 1; yn = y;
        implied_possible = y % SPECKLE_TILE_Y != 0;
    }
    const int v = speckle_value(a, image, x, y), n = speckle_value(a, image, xn, yn);
    if(!speckle_joined(v, n, a.max_diff)) return;
    if(implied_possible)
    {
        // The pixel beside me along the border (m), and its neighbour across it (mn): m and I, and mn and n, are in
        // one tile each, where every join is made. m - mn is the join of this kind one pixel back along the border:
        // made, or implied in its turn; at a corner of four tiles, where the chain starts, nothing is left out
        const int dx = t < below ? 1 : 0, dy = 1 - dx;
        const int m = speckle_value(a, image, x - dx, y - dy), mn = speckle_value(a, image, xn - dx, yn - dy);
        if(speckle_joined(v, m, a.max_diff) && speckle_joined(m, mn, a.max_diff) && speckle_joined(mn, n, a.max_diff)) return;
    }
    speckle_union(label, y*a.W + x, yn*a.W + xn);
}

////////////////////////////////////////////////////////////////////////////////
// roots, sizes, the result
////////////////////////////////////////////////////////////////////////////////
__global__ __launch_bounds__(SPECKLE_THREADS)
void speckle_count_kernel(size_t N, int32_t* label, int32_t* count)
{
    const size_t pixel = (size_t)blockIdx.x*SPECKLE_THREADS + threadIdx.x;
    if(pixel >= N || speckle_load(&label[pixel]) < 0) return;
    const int root = speckle_find(label, (int)pixel);
    if(root == (int)pixel) return;
    // (another lane may be reading it on its way up: either value is a smaller index of the region)
    __atomic_store_n(&label[pixel], root, __ATOMIC_RELAXED);
    // A tile's root that is not the region's hands the size of its tile's region on: one atomicAdd a tile and region,
    // not one a pixel. Nothing is ever added to count[pixel] of such a pixel, and the region's root adds nothing
    const int mine = count[pixel];
    if(mine > 0) atomicAdd(&count[root], mine);
}

__global__ __launch_bounds__(SPECKLE_THREADS)
void speckle_apply_kernel(size_t N, int new_value, int max_speckle_size, const int32_t* __restrict__ label,
                          const int32_t* __restrict__ count, int16_t* __restrict__ image)
{
    const size_t pixel = (size_t)blockIdx.x*SPECKLE_THREADS + threadIdx.x;
    if(pixel >= N) return;
    const int root = label[pixel];
    if(root >= 0 && count[root] <= max_speckle_size) image[pixel] = (int16_t)new_value;
}

} // namespace

bool speckle_filter_device(const SpeckleGrids& g, const SpeckleParams& p, int16_t* image, void* workspace, SpecklePassEvents* pass_events)
{
    // (recorded only for the stand-alone filter, which reports its passes one by one)
#define SPECKLE_PASS_DONE(i) do { if(!record(pass_events, i)) return false; } while(0)
    const size_t N = (size_t)g.W*(size_t)g.H;
    int32_t* label = (int32_t*)workspace;
    int32_t* count = (int32_t*)((uint8_t*)workspace + speckle_count_offset(N));
    SpeckleArgs a;
    a.W = g.W; a.H = g.H; a.new_value = p.new_value; a.max_diff = p.max_diff;
    SPECKLE_PASS_DONE(0);
    hipLaunchKernelGGL(speckle_label_tile_kernel, dim3(g.tile_grid), dim3(SPECKLE_THREADS), 0, NULL, a, g.tiles_x, image, label, count);
    SPECKLE_PASS_DONE(1);
    if(g.border_grid > 0)
        hipLaunchKernelGGL(speckle_merge_borders_kernel, dim3(g.border_grid), dim3(SPECKLE_THREADS), 0, NULL,
                           a, g.tiles_y, g.border_pixels, image, label);
    SPECKLE_PASS_DONE(2);
    hipLaunchKernelGGL(speckle_count_kernel, dim3(g.pixel_grid), dim3(SPECKLE_THREADS), 0, NULL, N, label, count);
    SPECKLE_PASS_DONE(3);
    hipLaunchKernelGGL(speckle_apply_kernel, dim3(g.pixel_grid), dim3(SPECKLE_THREADS), 0, NULL,
                       N, p.new_value, p.max_speckle_size, label, count, image);
    SPECKLE_PASS_DONE(4);
#undef SPECKLE_PASS_DONE
    HIP_TRY(hipGetLastError(), return false);
    return true;
}

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_speckle_filter
{
    DeviceBuffers mem;
    uint8_t*      pool = NULL;
    SpecklePlan   plan;
    SpecklePassEvents events;       // before the first pass, and after each of the four
};

static bool speckle_given(const mrcal_amd_speckle_filter* f)
{
    if(f != NULL) return true;
    set_error("filter_speckles(): the filter is NULL");
    return false;
}

extern "C" {

mrcal_amd_speckle_filter_t* mrcal_amd_speckle_filter_create(int width, int height)
{
    last_error_string().clear();
    std::string why;
    if(!speckle_params_ok(&why, width, height, 0, 0, 0)) { set_error("%s", why.c_str()); return NULL; }
    if(!have_device()) return NULL;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return NULL);
    SpecklePlan plan;
    if(!speckle_plan(&plan, &why, width, height, free_bytes)) { set_error("%s", why.c_str()); return NULL; }

    mrcal_amd_speckle_filter* f = new mrcal_amd_speckle_filter;
    f->plan = plan;
    if(!f->mem.alloc(&f->pool, plan.bytes)) { delete f; return NULL; }
    if(!f->events.create()) { delete f; return NULL; }
    return f;
}

bool mrcal_amd_speckle_filter_apply(mrcal_amd_speckle_filter_t* f, const int16_t* in, int16_t* out,
                                    int new_value, int max_speckle_size, int max_diff)
{
    last_error_string().clear();
    if(!speckle_given(f)) return false;
    const SpeckleGrids& g = f->plan.grids;
    std::string why;
    if(!speckle_params_ok(&why, g.W, g.H, new_value, max_speckle_size, max_diff)) { set_error("%s", why.c_str()); return false; }
    if(in == NULL || out == NULL) { set_error("filter_speckles(): an image is NULL"); return false; }
    if(!have_device()) return false;
    const size_t bytes = (size_t)g.W*(size_t)g.H*sizeof(int16_t);
    int16_t* d_image = (int16_t*)(f->pool + f->plan.image);
    f->events.timed = false;
    HIP_TRY(hipMemcpy(d_image, in, bytes, hipMemcpyHostToDevice), return false);
    if(!speckle_filter_device(g, speckle_params(new_value, max_speckle_size, max_diff), d_image, f->pool + f->plan.label,
                              &f->events))
        return false;
    // (the copy waits for the launches)
    HIP_TRY(hipMemcpy(out, d_image, bytes, hipMemcpyDeviceToHost), return false);
    f->events.timed = true;
    return true;
}

bool mrcal_amd_speckle_filter_milliseconds(mrcal_amd_speckle_filter_t* f, float* milliseconds)
{
    last_error_string().clear();
    if(!speckle_given(f)) return false;
    if(!f->events.timed) { set_error("filter_speckles(): no image has been filtered yet"); return false; }
    return f->events.elapsed(milliseconds, 0, 4);
}

bool mrcal_amd_speckle_filter_pass_milliseconds(mrcal_amd_speckle_filter_t* f, float* milliseconds)
{
    last_error_string().clear();
    if(!speckle_given(f)) return false;
    if(!f->events.timed) { set_error("filter_speckles(): no image has been filtered yet"); return false; }
    for(int i = 0; i < 4; i++)
        if(!f->events.elapsed(&milliseconds[i], i, i+1)) return false;
    return true;
}

void mrcal_amd_speckle_filter_destroy(mrcal_amd_speckle_filter_t* f) { delete f; }

} // extern "C"
