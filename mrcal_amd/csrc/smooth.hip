// smooth_gaussian(): the anti-aliasing pre-filter of an image that is about to be remapped to fewer pixels
// (include/mrcal_amd.h, "smoothing": the definition, to the bit; the reference only has it on its to-do list).
//
//   smooth_kernel   ONE launch an image, a workgroup a tile of tile_w x tile_h pixels of the result
//                   (256 x 32 of a uint8 image at sigma = 2; the plan makes the tile lower for a larger radius):
//                     1. the tile's rows with their halo of Ry rows above and below and halo_x pixels left and right
//                        are staged in LDS as they are, four bytes a lane, clamped to the image where they leave it
//                     2. a lane makes the horizontal sums of 4 neighbouring pixels of a row and writes them to a second
//                        LDS tile, 16 bits each for a uint8 image and 32 for a uint16 one. uint8: the window slides over
//                        the staged dwords, v_alignbyte_b32 makes the three windows that begin inside a dword, and
//                        v_dot4_u32_u8 sums four taps a time. uint16, and an x axis that is not filtered: multiply-adds
//                     3. a lane makes 4 neighbouring pixels of a row of the result: it walks down its 8 (16) bytes of
//                        the sums' rows, which the lanes of a wavefront read side by side - one ds_read_b64 (b128) a
//                        tap, no two lanes of a group on one bank - rounds, shifts and stores 4 (8) bytes
//                   The horizontal sums never leave the LDS. Integers only and no atomics: the same bits on every call.
// The taps, the tile and the LDS are smooth_plan.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "smooth_plan.hpp"
#include "smooth.hpp"

namespace mrcal_amd {

namespace {

#define SMOOTH_WINDOW_LEAD 3        // zero taps in front of wx_window: the 4 pixels of a lane share one walk over the staged row

struct SmoothArgs
{
    int      W, H, Rx, Ry, halo_x, rows, tile_h, raw_dwords;
    unsigned grid_x, lds_t;
    int      stage_drow, stage_dcol;                    // SMOOTH_THREADS staged dwords on: so many rows and dwords
    // the x taps of the window that begins halo_x pixels left of a pixel: tap t has the weight wx_{t - halo_x}, or 0
    uint32_t wx_packed[SMOOTH_R_MAX/2 + 1];             // taps 4g .. 4g+3, a byte each
    int32_t  wx_window[SMOOTH_WINDOW_LEAD + 2*SMOOTH_R_MAX + 1 + 4];    // tap t at [t + SMOOTH_WINDOW_LEAD]
    int32_t  wy_window[2*SMOOTH_R_MAX + 1];             // tap t has the weight wy_{t - Ry}
};

__device__ __forceinline__ int clamped(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the horizontal sums of the 4 pixels whose window begins at `staged`, by multiply-adds
template<class T>
__device__ __forceinline__ void horizontal_mac(uint32_t* acc, const uint32_t* staged, const SmoothArgs& a)
{
    constexpr int PER_DWORD = 4/sizeof(T);
    const int dwords = (2*a.halo_x + SMOOTH_QUAD)/PER_DWORD;
    for(int g = 0; g < dwords; g++)
    {
        const uint32_t d = staged[g];
#pragma unroll
        for(int e = 0; e < PER_DWORD; e++)
        {
            const uint32_t v = sizeof(T) == 1 ? (d >> 8*e) & 0xFFu : (d >> 16*e) & 0xFFFFu;
            const int32_t* w = &a.wx_window[PER_DWORD*g + e + SMOOTH_WINDOW_LEAD];
#pragma unroll
            for(int j = 0; j < SMOOTH_QUAD; j++) acc[j] += (uint32_t)w[-j]*v;
        }
    }
}

// ... of a uint8 image, four taps an instruction. The taps are bytes: Rx > 0, whose centre tap is below 256
__device__ __forceinline__ void horizontal_dot4(uint32_t* acc, const uint32_t* staged, const SmoothArgs& a)
{
    const int groups = a.halo_x/2 + 1;
    uint32_t lo = staged[0];
    for(int g = 0; g < groups; g++)
    {
        const uint32_t hi = staged[g + 1], w = a.wx_packed[g];
        acc[0] = __builtin_amdgcn_udot4(lo, w, acc[0], false);
        acc[1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, lo, 1), w, acc[1], false);
        acc[2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, lo, 2), w, acc[2], false);
        acc[3] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, lo, 3), w, acc[3], false);
        lo = hi;
    }
}

template<class T>
__global__ __launch_bounds__(SMOOTH_THREADS)
void smooth_kernel(SmoothArgs a, const T* __restrict__ image, T* __restrict__ out)
{
    constexpr int PER_DWORD = 4/sizeof(T);
    constexpr int TILE_W    = SMOOTH_SUM_ROW_BYTES/(2*sizeof(T));
    constexpr int QUADS     = TILE_W/SMOOTH_QUAD;               // of a row of the tile
    constexpr int SUM_ROW_DWORDS = SMOOTH_SUM_ROW_BYTES/4;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* sums = lds + a.lds_t/4;

    const unsigned tile_y = blockIdx.x / a.grid_x, tile_x = blockIdx.x - tile_y*a.grid_x;
    const int X0 = (int)tile_x*TILE_W, Y0 = (int)tile_y*a.tile_h;

    // 1. the rows with their halo, as they are
    {
        int row = (int)threadIdx.x / a.raw_dwords, col = (int)threadIdx.x - row*a.raw_dwords;
        while(row < a.rows)
        {
            const int x = X0 - a.halo_x + col*PER_DWORD;
            const T* line = image + (size_t)clamped(Y0 - a.Ry + row, a.H)*(size_t)a.W;
            uint32_t d;
            if(x >= 0 && x + PER_DWORD <= a.W) __builtin_memcpy(&d, line + x, 4);
            else
            {
                d = 0;
#pragma unroll
                for(int e = 0; e < PER_DWORD; e++) d |= (uint32_t)line[clamped(x + e, a.W)] << (8*(int)sizeof(T)*e);
            }
            lds[row*a.raw_dwords + col] = d;
            row += a.stage_drow; col += a.stage_dcol;
            if(col >= a.raw_dwords) { col -= a.raw_dwords; row++; }
        }
    }
    __syncthreads();

    // 2. the horizontal sums
    // (measured: 0.077 ms with v_dot4_u32_u8 against 0.097 with the multiply-adds, uint8 at 6016 x 4016 and sigma = 2)
    const bool dot4 = sizeof(T) == 1 && a.Rx > 0;
    for(int i = (int)threadIdx.x; i < a.rows*QUADS; i += SMOOTH_THREADS)
    {
        const int row = i / QUADS, quad = i - row*QUADS;
        const uint32_t* staged = lds + row*a.raw_dwords + quad*(int)sizeof(T);
        uint32_t acc[SMOOTH_QUAD] = { 0u, 0u, 0u, 0u };
        if(dot4) horizontal_dot4(acc, staged, a);
        else     horizontal_mac<T>(acc, staged, a);
        uint32_t* to = sums + row*SUM_ROW_DWORDS;
        if(sizeof(T) == 1) *(uint2*)(to + 2*quad) = make_uint2(acc[0] | acc[1] << 16, acc[2] | acc[3] << 16);
        else               *(uint4*)(to + 4*quad) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    }
    __syncthreads();

    // 3. the vertical sums, and the result
    const int taps = 2*a.Ry + 1;
    for(int i = (int)threadIdx.x; i < a.tile_h*QUADS; i += SMOOTH_THREADS)
    {
        const int row = i / QUADS, quad = i - row*QUADS;
        const int x = X0 + quad*SMOOTH_QUAD, y = Y0 + row;
        if(x >= a.W || y >= a.H) continue;
        uint32_t acc[SMOOTH_QUAD] = { 32768u, 32768u, 32768u, 32768u };
        const uint32_t* from = sums + row*SUM_ROW_DWORDS + quad*2*(int)sizeof(T);
        for(int t = 0; t < taps; t++, from += SUM_ROW_DWORDS)
        {
            const uint32_t w = (uint32_t)a.wy_window[t];
            if(sizeof(T) == 1)
            {
                const uint2 s = *(const uint2*)from;
                acc[0] += w*(s.x & 0xFFFFu); acc[1] += w*(s.x >> 16);
                acc[2] += w*(s.y & 0xFFFFu); acc[3] += w*(s.y >> 16);
            }
            else
            {
                const uint4 s = *(const uint4*)from;
                acc[0] += w*s.x; acc[1] += w*s.y; acc[2] += w*s.z; acc[3] += w*s.w;
            }
        }
        T* o = out + (size_t)y*(size_t)a.W + x;
        T res[SMOOTH_QUAD];
#pragma unroll
        for(int j = 0; j < SMOOTH_QUAD; j++) res[j] = (T)(acc[j] >> 16);
        if(x + SMOOTH_QUAD <= a.W) __builtin_memcpy(o, res, sizeof(res));
        else
        {
#pragma unroll
            for(int j = 0; j < SMOOTH_QUAD - 1; j++)
                if(x + j < a.W) o[j] = res[j];
        }
    }
}

SmoothArgs args_of(const SmoothPlan& p)
{
    SmoothArgs a;
    memset(&a, 0, sizeof(a));
    a.W = p.W; a.H = p.H; a.Rx = p.Rx; a.Ry = p.Ry; a.halo_x = p.halo_x; a.rows = p.rows; a.tile_h = p.tile_h;
    a.raw_dwords = p.raw_dwords; a.grid_x = p.grid_x; a.lds_t = p.lds_t;
    a.stage_drow = SMOOTH_THREADS / p.raw_dwords; a.stage_dcol = SMOOTH_THREADS % p.raw_dwords;
    for(int t = 0; t <= 2*p.halo_x; t++) a.wx_window[t + SMOOTH_WINDOW_LEAD] = smooth_tap(p.wx, p.Rx, t - p.halo_x);
    // (an axis that is not filtered has the tap 256, which is no byte: it takes the multiply-adds)
    if(p.Rx > 0)
        for(int t = 0; t <= 2*p.halo_x; t++) a.wx_packed[t/4] |= (uint32_t)smooth_tap(p.wx, p.Rx, t - p.halo_x) << 8*(t%4);
    for(int t = 0; t <= 2*p.Ry; t++) a.wy_window[t] = smooth_tap(p.wy, p.Ry, t - p.Ry);
    return a;
}

} // namespace

SmoothParams smooth_params_of(const mrcal_amd_smooth_params_t* params)
{
    SmoothParams p;
    if(params != NULL) { p.sigma_x = params->sigma_x; p.sigma_y = params->sigma_y; }
    return p;
}

bool smooth_device(const SmoothPlan& p, const void* d_in, void* d_out, SmoothEvents* events)
{
    if(p.grid == 0) { set_error("smooth(): internal error: nothing is planned"); return false; }
    if(d_in == d_out) { set_error("smooth(): internal error: the result cannot replace the image"); return false; }
    const SmoothArgs a = args_of(p);
    if(!record(events, 0)) return false;
    if(p.dtype == IMAGE_DTYPE_UINT8)
        hipLaunchKernelGGL((smooth_kernel<uint8_t>),  dim3(p.grid), dim3(SMOOTH_THREADS), p.lds_bytes, NULL, a, (const uint8_t*)d_in,  (uint8_t*)d_out);
    else
        hipLaunchKernelGGL((smooth_kernel<uint16_t>), dim3(p.grid), dim3(SMOOTH_THREADS), p.lds_bytes, NULL, a, (const uint16_t*)d_in, (uint16_t*)d_out);
    if(!record(events, 1)) return false;
    HIP_TRY(hipGetLastError(), return false);
    return true;
}

bool smooth_resident(DeviceBuffers& result, const SmoothParams& params, const void* d_image, int W, int H, int dtype,
                     const void** d_smoothed)
{
    if(smooth_is_off(params)) { *d_smoothed = d_image; return true; }
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return false);
    SmoothPlan plan; std::string why;
    if(!smooth_plan(&plan, &why, W, H, dtype, params, free_bytes, false)) { set_error("%s", why.c_str()); return false; }
    uint8_t* d_out = NULL;
    if(!result.alloc(&d_out, (size_t)W*H*image_pixel_bytes(dtype))) return false;
    if(!smooth_device(plan, d_image, d_out)) return false;
    *d_smoothed = d_out;
    return true;
}

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_smoother
{
    DeviceBuffers mem;
    uint8_t*      pool = NULL;
    SmoothPlan    plan;
    SmoothEvents  events;
};

static bool smoother_given(const mrcal_amd_smoother* s)
{
    if(s != NULL) return true;
    set_error("smooth(): the smoother is NULL");
    return false;
}

extern "C" {

mrcal_amd_smoother_t* mrcal_amd_smoother_create(int width, int height, int dtype, const mrcal_amd_smooth_params_t* params)
{
    last_error_string().clear();
    if(params == NULL) { set_error("smooth(): the parameters are NULL"); return NULL; }
    const SmoothParams p = smooth_params_of(params);
    std::string why;
    if(!smooth_params_ok(&why, width, height, dtype, p)) { set_error("%s", why.c_str()); return NULL; }
    if(!have_device()) return NULL;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return NULL);
    SmoothPlan plan;
    if(!smooth_plan(&plan, &why, width, height, dtype, p, free_bytes)) { set_error("%s", why.c_str()); return NULL; }

    mrcal_amd_smoother* s = new mrcal_amd_smoother;
    s->plan = plan;
    if(!s->mem.alloc(&s->pool, plan.bytes)) { delete s; return NULL; }
    if(!s->events.create()) { delete s; return NULL; }
    return s;
}

bool mrcal_amd_smoother_apply(mrcal_amd_smoother_t* s, const void* in, void* out)
{
    last_error_string().clear();
    if(!smoother_given(s)) return false;
    if(in == NULL || out == NULL) { set_error("smooth(): an image is NULL"); return false; }
    if(!have_device()) return false;
    const SmoothPlan& p = s->plan;
    const size_t bytes = (size_t)p.W*(size_t)p.H*image_pixel_bytes(p.dtype);
    s->events.timed = false;
    HIP_TRY(hipMemcpy(s->pool + p.image, in, bytes, hipMemcpyHostToDevice), return false);
    if(!smooth_device(p, s->pool + p.image, s->pool + p.result, &s->events)) return false;
    // (the copy waits for the launch)
    HIP_TRY(hipMemcpy(out, s->pool + p.result, bytes, hipMemcpyDeviceToHost), return false);
    s->events.timed = true;
    return true;
}

bool mrcal_amd_smoother_milliseconds(mrcal_amd_smoother_t* s, float* milliseconds)
{
    last_error_string().clear();
    if(!smoother_given(s)) return false;
    if(!s->events.timed) { set_error("smooth(): no image has been smoothed yet"); return false; }
    return s->events.elapsed(milliseconds, 0, 1);
}

void mrcal_amd_smoother_destroy(mrcal_amd_smoother_t* s) { delete s; }

bool mrcal_amd_smooth_weights(double sigma, int* R, int* w)
{
    last_error_string().clear();
    if(R == NULL || w == NULL) { set_error("smooth(): an argument is NULL"); return false; }
    if(smooth_weights(R, w, sigma)) return true;
    set_error("smooth(): there are taps for sigma = 0 and for sigma > 0 with ceil(3 sigma) <= %d. Got %g", SMOOTH_R_MAX, sigma);
    return false;
}

} // extern "C"
