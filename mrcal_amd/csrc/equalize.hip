// equalize_clahe(), equalize_stretch(): what the reference's tools do to an image before they rectify and match it
// (include/mrcal_amd.h, "equalization": the definition, to the bit; cv2.createCLAHE().apply() and
// mrcal_image_uint8_load()'s stretch).
//
//   clahe_hist_kernel     a workgroup a band of EQUALIZE_BAND_ROWS rows of a tile of the PADDED image, which is never
//                         made: a padded pixel is read at its reflected index. uint8: every wavefront counts into its
//                         own 256 bins in LDS, the four copies are summed and added to the tile's bins in global memory,
//                         one integer atomicAdd a bin and band. uint16: 65536 bins a tile do not fit the LDS; integer
//                         atomicAdd straight into the tile's bins in global memory
//   clahe_lut_kernel      a tile each: a wavefront with 4 bins a lane (uint8) or 1024 threads with 64 bins each
//                         (uint16), the bins in registers. The clipped excess summed over the workgroup, the bins
//                         clipped, the excess handed back (the residual's increments are a closed form of the bin's
//                         index), an integer prefix sum, and the LUT
//   clahe_apply_kernel    a lane 4 pixels of a row at a time, a workgroup 1024 x 16 pixels: the four LUTs around the pixel
//                         read at its value and interpolated in float32, every operation rounded on its own. The
//                         uint8 LUTs of all tiles are staged in LDS when they fit (16 KiB at 8 x 8 tiles)
//   stretch_minmax_kernel the extremes: 16 bytes a lane at a time, reduced over the workgroup, then ONE integer atomicMin
//                         and atomicMax a workgroup, of at most 512
//   stretch_map_kernel    a lane a pixel: uint8(0.5f + float(v - min) 255.f / float(max - min))
// Integer sums and extremes are the same bits in whatever order they are taken, there is no floating-point atomic, and
// no workgroup waits for another: a call gives the same bits every time.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "equalize_plan.hpp"
#include "equalize.hpp"

static_assert(EQUALIZE_METHOD_NONE == MRCAL_AMD_EQUALIZE_NONE && EQUALIZE_METHOD_CLAHE == MRCAL_AMD_EQUALIZE_CLAHE &&
              EQUALIZE_METHOD_STRETCH == MRCAL_AMD_EQUALIZE_STRETCH, "equalize_plan.hpp restates the header's methods");

namespace mrcal_amd {

namespace {

struct ClaheArgs
{
    int   W, H, tiles_x, tiles_y, tw, th, clip;
    float lut_scale, inv_tw, inv_th;
};

// BORDER_REFLECT_101 of an index past the end: the padding is at most n-1 (equalize_params_ok()), so once is enough
__device__ __forceinline__ int reflected(int i, int n) { return i < n ? i : 2*(n - 1) - i; }

////////////////////////////////////////////////////////////////////////////////
// the histograms
////////////////////////////////////////////////////////////////////////////////
template<class T>
__global__ __launch_bounds__(EQUALIZE_THREADS)
void clahe_hist_kernel(ClaheArgs a, unsigned bands, const T* __restrict__ image, uint32_t* hist)
{
    constexpr bool IN_LDS = sizeof(T) == 1;
    constexpr int  WAVES  = EQUALIZE_THREADS/64;
    __shared__ uint32_t local[IN_LDS ? WAVES*256 : 1];
    const unsigned tile = blockIdx.x / bands, band = blockIdx.x - tile*bands;
    const int ty = (int)(tile / (unsigned)a.tiles_x), tx = (int)(tile - (unsigned)ty*(unsigned)a.tiles_x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if(IN_LDS)
    {
#pragma unroll
        for(int k = 0; k < WAVES; k++) local[k*256 + threadIdx.x] = 0;
        __syncthreads();
    }
    const int r0 = (int)band*EQUALIZE_BAND_ROWS;
    const int r1 = r0 + EQUALIZE_BAND_ROWS < a.th ? r0 + EQUALIZE_BAND_ROWS : a.th;
    uint32_t* mine = hist + (size_t)tile*(IN_LDS ? 256 : 65536);
    for(int r = r0 + wave; r < r1; r += WAVES)
    {
        const T* row = image + (size_t)reflected(ty*a.th + r, a.H)*a.W;
        for(int c = lane; c < a.tw; c += 64)
        {
            const unsigned v = row[reflected(tx*a.tw + c, a.W)];
            if(IN_LDS) atomicAdd(&local[wave*256 + v], 1u);
            else       atomicAdd(&mine[v], 1u);
        }
    }
    if(IN_LDS)
    {
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for(int k = 0; k < WAVES; k++) sum += local[k*256 + threadIdx.x];
        if(sum > 0) atomicAdd(&mine[threadIdx.x], sum);
    }
}

////////////////////////////////////////////////////////////////////////////////
// clip, hand back, sum, LUT
////////////////////////////////////////////////////////////////////////////////
// the sum of v over the workgroup, in every thread. part: LDS, a word a wavefront
template<int THREADS>
__device__ __forceinline__ uint32_t workgroup_sum(uint32_t v, uint32_t* part)
{
#pragma unroll
    for(int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if(THREADS == 64) return v;
    if((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for(int w = 0; w < THREADS/64; w++) sum += part[w];
    return sum;
}

// the sum of v over the threads before this one. part: LDS, a word a wavefront, not the one of workgroup_sum()
template<int THREADS>
__device__ __forceinline__ uint32_t workgroup_sum_before(uint32_t v, uint32_t* part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inclusive = v;
#pragma unroll
    for(int d = 1; d < 64; d <<= 1)
    {
        const uint32_t below = __shfl_up(inclusive, d);
        if(lane >= d) inclusive += below;
    }
    uint32_t before = inclusive - v;
    if(THREADS == 64) return before;
    if(lane == 63) part[wave] = inclusive;
    __syncthreads();
#pragma unroll
    for(int w = 0; w < THREADS/64; w++) if(w < wave) before += part[w];
    return before;
}

// THREADS x BINS = the bins of a histogram; a thread has BINS consecutive ones
template<class T, int THREADS, int BINS>
__global__ __launch_bounds__(THREADS)
void clahe_lut_kernel(ClaheArgs a, const uint32_t* __restrict__ hist, T* __restrict__ lut)
{
    constexpr int HIST = THREADS*BINS;
    static_assert(BINS % 4 == 0, "the bins are loaded four at a time");
    __shared__ uint32_t part_sum[THREADS/64], part_scan[THREADS/64];
    const size_t first = (size_t)blockIdx.x*HIST + (size_t)threadIdx.x*BINS;
    uint32_t h[BINS];
#pragma unroll
    for(int k = 0; k < BINS; k += 4)
    {
        const uint4 q = *(const uint4*)(hist + first + k);
        h[k] = q.x; h[k+1] = q.y; h[k+2] = q.z; h[k+3] = q.w;
    }
    const uint32_t clip = (uint32_t)a.clip;
    uint32_t excess = 0;
#pragma unroll
    for(int k = 0; k < BINS; k++)
        if(h[k] > clip) { excess += h[k] - clip; h[k] = clip; }
    const uint32_t clipped  = workgroup_sum<THREADS>(excess, part_sum);
    const uint32_t batch    = clipped / HIST;
    const uint32_t residual = clipped - batch*HIST;
    // the bins 0, step, 2 step ... get one more each, the first `residual` of them
    const uint32_t step = residual > 0 ? (HIST/residual > 1 ? HIST/residual : 1) : 1;
    const uint32_t i0 = threadIdx.x*BINS;
    uint32_t sum = 0;
#pragma unroll
    for(int k = 0; k < BINS; k++)
    {
        const uint32_t i = i0 + k, n = i/step;
        h[k] += batch + ((n*step == i && n < residual) ? 1u : 0u);
        sum += h[k];
        h[k] = sum;
    }
    const uint32_t before = workgroup_sum_before<THREADS>(sum, part_scan);
    // stored 4 bytes (uint8: the thread's 4 bins) or 16 bytes (uint16: 8 of its 64) at a time
    constexpr int GROUP = sizeof(T) == 1 ? 4 : 8;
    static_assert(BINS % GROUP == 0, "the LUT is stored in whole groups");
#pragma unroll
    for(int k0 = 0; k0 < BINS; k0 += GROUP)
    {
        T out[GROUP];
#pragma unroll
        for(int k = 0; k < GROUP; k++)
        {
            const int l = __float2int_rn(__fmul_rn((float)(before + h[k0 + k]), a.lut_scale));
            out[k] = (T)(l < 0 ? 0 : l > HIST - 1 ? HIST - 1 : l);
        }
        if(sizeof(T) == 1) { uint32_t q; memcpy(&q, out, sizeof(q)); *(uint32_t*)(lut + first + k0) = q; }
        else               { uint4    q; memcpy(&q, out, sizeof(q)); *(uint4*)   (lut + first + k0) = q; }
    }
}

////////////////////////////////////////////////////////////////////////////////
// the interpolation
////////////////////////////////////////////////////////////////////////////////
struct TileWeights { int t1, t2; float w1, w2; };

// the two tiles beside pixel i, and their weights. Every operation is rounded on its own (nothing is fused)
__device__ __forceinline__ TileWeights tile_weights(int i, float inv_size, int tiles)
{
    TileWeights t;
    const float scaled = __fmul_rn((float)i, inv_size);
    const float tf     = __fsub_rn(scaled, 0.5f);
    const float below  = floorf(tf);
    t.w2 = __fsub_rn(tf, below);
    t.w1 = __fsub_rn(1.0f, t.w2);
    const int t1 = (int)below, t2 = t1 + 1;
    t.t1 = t1 < 0 ? 0 : t1;
    t.t2 = t2 > tiles - 1 ? tiles - 1 : t2;
    return t;
}

template<class T, bool LUTS_IN_LDS>
__global__ __launch_bounds__(EQUALIZE_THREADS)
void clahe_apply_kernel(ClaheArgs a, unsigned blocks_across, const T* __restrict__ image, const T* __restrict__ lut, T* __restrict__ out)
{
    constexpr int HIST = sizeof(T) == 1 ? 256 : 65536;
    constexpr int NX   = EQUALIZE_APPLY_X;
    extern __shared__ uint4 staged[];
    const T* luts = lut;
    if(LUTS_IN_LDS)
    {
        // (a LUT of uint8 is 256 bytes: 16 uint4)
        const int n = a.tiles_x*a.tiles_y*16;
        for(int i = threadIdx.x; i < n; i += EQUALIZE_THREADS) staged[i] = ((const uint4*)lut)[i];
        __syncthreads();
        luts = (const T*)staged;
    }
    const unsigned block_y = blockIdx.x / blocks_across, block_x = blockIdx.x - block_y*blocks_across;
    const int x0 = (int)(block_x*EQUALIZE_THREADS + threadIdx.x)*NX;
    const int y0 = (int)block_y*EQUALIZE_APPLY_ROWS;
    if(x0 >= a.W) return;
    // whole groups of 4 pixels in every row, each aligned: a row begins at a multiple of 4 pixels
    const bool wide = a.W % NX == 0;
    TileWeights tx[NX];
#pragma unroll
    for(int k = 0; k < NX; k++) tx[k] = tile_weights(x0 + k, a.inv_tw, a.tiles_x);
    for(int r = 0; r < EQUALIZE_APPLY_ROWS; r++)
    {
        const int y = y0 + r;
        if(y >= a.H) break;
        const TileWeights ty = tile_weights(y, a.inv_th, a.tiles_y);
        const size_t at = (size_t)y*a.W + x0;
        T v[NX], res[NX];
        if(wide)
        {
            if(sizeof(T) == 1) { const uint32_t q = *(const uint32_t*)(image + at); memcpy(v, &q, sizeof(q)); }
            else               { const uint2    q = *(const uint2*)   (image + at); memcpy(v, &q, sizeof(q)); }
        }
        else
        {
#pragma unroll
            for(int k = 0; k < NX; k++) v[k] = x0 + k < a.W ? image[at + k] : (T)0;
        }
        const T* row1 = luts + (size_t)ty.t1*a.tiles_x*HIST;
        const T* row2 = luts + (size_t)ty.t2*a.tiles_x*HIST;
#pragma unroll
        for(int k = 0; k < NX; k++)
        {
            const float l11 = (float)row1[(size_t)tx[k].t1*HIST + v[k]], l12 = (float)row1[(size_t)tx[k].t2*HIST + v[k]];
            const float l21 = (float)row2[(size_t)tx[k].t1*HIST + v[k]], l22 = (float)row2[(size_t)tx[k].t2*HIST + v[k]];
            const float top    = __fadd_rn(__fmul_rn(l11, tx[k].w1), __fmul_rn(l12, tx[k].w2));
            const float bottom = __fadd_rn(__fmul_rn(l21, tx[k].w1), __fmul_rn(l22, tx[k].w2));
            const float value  = __fadd_rn(__fmul_rn(top, ty.w1), __fmul_rn(bottom, ty.w2));
            const int   l      = __float2int_rn(value);
            res[k] = (T)(l < 0 ? 0 : l > HIST - 1 ? HIST - 1 : l);
        }
        if(wide)
        {
            if(sizeof(T) == 1) { uint32_t q; memcpy(&q, res, sizeof(q)); *(uint32_t*)(out + at) = q; }
            else               { uint2    q; memcpy(&q, res, sizeof(q)); *(uint2*)   (out + at) = q; }
        }
        else
        {
#pragma unroll
            for(int k = 0; k < NX; k++) if(x0 + k < a.W) out[at + k] = res[k];
        }
    }
}

////////////////////////////////////////////////////////////////////////////////
// stretch
////////////////////////////////////////////////////////////////////////////////
// minmax: [0] the minimum (starts at all ones), [1] the maximum (starts at 0)
template<class T>
__global__ __launch_bounds__(EQUALIZE_THREADS)
void stretch_minmax_kernel(size_t N, const T* __restrict__ image, uint32_t* minmax)
{
    constexpr int    PER_WORD = 4/sizeof(T), BITS = 8*sizeof(T);
    constexpr uint32_t MASK = sizeof(T) == 1 ? 0xFFu : 0xFFFFu;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    // 16 bytes a lane at a time (the image begins at a multiple of 16 bytes), then what is left, a pixel a lane
    const size_t quads = N*sizeof(T)/16;
    for(size_t i = (size_t)blockIdx.x*EQUALIZE_THREADS + threadIdx.x; i < quads; i += (size_t)gridDim.x*EQUALIZE_THREADS)
    {
        const uint4 q = ((const uint4*)image)[i];
        const uint32_t word[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for(int w = 0; w < 4; w++)
#pragma unroll
            for(int k = 0; k < PER_WORD; k++)
            {
                const uint32_t v = (word[w] >> (BITS*k)) & MASK;
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
    }
    if(blockIdx.x == 0)
        for(size_t i = quads*(16/sizeof(T)) + threadIdx.x; i < N; i += EQUALIZE_THREADS)
        {
            const uint32_t v = image[i];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
#pragma unroll
    for(int d = 32; d >= 1; d >>= 1)
    {
        const uint32_t l = __shfl_xor(lo, d), h = __shfl_xor(hi, d);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    // one pair of atomics a workgroup: thousands of them on the same two words are what this kernel would wait for
    __shared__ uint32_t wave_lo[EQUALIZE_THREADS/64], wave_hi[EQUALIZE_THREADS/64];
    if((threadIdx.x & 63) == 0) { wave_lo[threadIdx.x >> 6] = lo; wave_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if(threadIdx.x == 0)
    {
#pragma unroll
        for(int w = 1; w < EQUALIZE_THREADS/64; w++)
        {
            lo = wave_lo[w] < lo ? wave_lo[w] : lo;
            hi = wave_hi[w] > hi ? wave_hi[w] : hi;
        }
        atomicMin(&minmax[0], lo);
        atomicMax(&minmax[1], hi);
    }
}

template<class T>
__global__ __launch_bounds__(EQUALIZE_THREADS)
void stretch_map_kernel(size_t N, const T* __restrict__ image, const uint32_t* __restrict__ minmax, uint8_t* __restrict__ out)
{
    const uint32_t lo = minmax[0], hi = minmax[1];
    const float    span = (float)(hi - lo);
    const size_t   base = (size_t)blockIdx.x*EQUALIZE_THREADS*EQUALIZE_MAP_PIXELS;
#pragma unroll
    for(int k = 0; k < EQUALIZE_MAP_PIXELS; k++)
    {
        const size_t i = base + (size_t)k*EQUALIZE_THREADS + threadIdx.x;
        if(i >= N) continue;
        // (a constant image, which the reference divides by zero for: all zeros)
        uint8_t o = 0;
        if(hi > lo)
        {
            const float scaled = __fmul_rn((float)((uint32_t)image[i] - lo), 255.f);
            o = (uint8_t)(int)__fadd_rn(0.5f, __fdiv_rn(scaled, span));
        }
        out[i] = o;
    }
}

template<class T>
void launch_clahe(const EqualizePlan& p, const ClaheArgs& a, const void* d_in, void* d_out, uint32_t* hist, void* lut,
                  EqualizeStageEvents* event)
{
    hipLaunchKernelGGL((clahe_hist_kernel<T>), dim3(p.hist_grid), dim3(EQUALIZE_THREADS), 0, NULL, a, p.bands, (const T*)d_in, hist);
    (void)record(event, 1);
    if constexpr(sizeof(T) == 1) hipLaunchKernelGGL((clahe_lut_kernel<T,   64,  4>), dim3(p.lut_grid), dim3(64),   0, NULL, a, hist, (T*)lut);
    else                         hipLaunchKernelGGL((clahe_lut_kernel<T, 1024, 64>), dim3(p.lut_grid), dim3(1024), 0, NULL, a, hist, (T*)lut);
    (void)record(event, 2);
    const dim3 grid(p.apply_grid);
    if(p.luts_in_lds)
        hipLaunchKernelGGL((clahe_apply_kernel<T, true>), grid, dim3(EQUALIZE_THREADS), (size_t)p.tiles_x*p.tiles_y*256, NULL,
                           a, p.apply_grid_x, (const T*)d_in, (const T*)lut, (T*)d_out);
    else
        hipLaunchKernelGGL((clahe_apply_kernel<T, false>), grid, dim3(EQUALIZE_THREADS), 0, NULL,
                           a, p.apply_grid_x, (const T*)d_in, (const T*)lut, (T*)d_out);
}

template<class T>
void launch_stretch(const EqualizePlan& p, const void* d_in, void* d_out, uint32_t* minmax, EqualizeStageEvents* event)
{
    const size_t N = (size_t)p.W*(size_t)p.H;
    hipLaunchKernelGGL((stretch_minmax_kernel<T>), dim3(p.minmax_grid), dim3(EQUALIZE_THREADS), 0, NULL, N, (const T*)d_in, minmax);
    (void)record(event, 1); (void)record(event, 2);
    hipLaunchKernelGGL((stretch_map_kernel<T>), dim3(p.map_grid), dim3(EQUALIZE_THREADS), 0, NULL, N, (const T*)d_in, minmax, (uint8_t*)d_out);
}

} // namespace

EqualizeParams equalize_params_of(const mrcal_amd_equalize_params_t* params)
{
    EqualizeParams p;
    if(params != NULL)
    {
        p.method = params->method; p.clip_limit = params->clip_limit;
        p.tiles_x = params->tiles_x; p.tiles_y = params->tiles_y;
    }
    return p;
}

bool equalize_device(const EqualizePlan& p, const void* d_in, void* d_out, uint8_t* pool, EqualizeStageEvents* event)
{
    if(p.method != EQUALIZE_METHOD_CLAHE && p.method != EQUALIZE_METHOD_STRETCH)
    { set_error("equalize(): internal error: no method to run"); return false; }
    if((((uintptr_t)d_in | (uintptr_t)d_out) & 15) != 0) { set_error("equalize(): the images on the device must be aligned to 16 bytes"); return false; }
    if(p.method == EQUALIZE_METHOD_CLAHE)
    {
        ClaheArgs a;
        a.W = p.W; a.H = p.H; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.tw = p.tw; a.th = p.th; a.clip = p.clip;
        a.lut_scale = p.lut_scale; a.inv_tw = p.inv_tw; a.inv_th = p.inv_th;
        uint32_t* hist = (uint32_t*)(pool + p.hist);
        HIP_TRY(hipMemsetAsync(hist, 0, p.hist_bytes, NULL), return false);
        if(!record(event, 0)) return false;
        if(p.dtype == IMAGE_DTYPE_UINT8) launch_clahe<uint8_t> (p, a, d_in, d_out, hist, pool + p.lut, event);
        else                                launch_clahe<uint16_t>(p, a, d_in, d_out, hist, pool + p.lut, event);
    }
    else
    {
        uint32_t* minmax = (uint32_t*)(pool + p.minmax);
        HIP_TRY(hipMemsetAsync(minmax,     0xFF, sizeof(uint32_t), NULL), return false);
        HIP_TRY(hipMemsetAsync(minmax + 1, 0,    sizeof(uint32_t), NULL), return false);
        if(!record(event, 0)) return false;
        if(p.dtype == IMAGE_DTYPE_UINT8) launch_stretch<uint8_t> (p, d_in, d_out, minmax, event);
        else                                launch_stretch<uint16_t>(p, d_in, d_out, minmax, event);
    }
    if(!record(event, 3)) return false;
    HIP_TRY(hipGetLastError(), return false);
    return true;
}

bool equalize_resident(DeviceBuffers& result, DeviceBuffers& workspace, const EqualizeParams& params,
                       const void* d_image, int W, int H, int dtype, const void** d_equalized, int* dtype_equalized)
{
    if(params.method == EQUALIZE_METHOD_NONE)
    {
        // (an unknown method is refused below; this one is none)
        *d_equalized = d_image; *dtype_equalized = dtype;
        return true;
    }
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return false);
    EqualizePlan plan; std::string why;
    if(!equalize_plan(&plan, &why, W, H, dtype, params, free_bytes, false)) { set_error("%s", why.c_str()); return false; }
    uint8_t *d_out = NULL, *pool = NULL;
    if(!(result.alloc(&d_out, (size_t)W*H*image_pixel_bytes(plan.dtype_out)) && workspace.alloc(&pool, plan.bytes))) return false;
    if(!equalize_device(plan, d_image, d_out, pool)) return false;
    *d_equalized = d_out; *dtype_equalized = plan.dtype_out;
    return true;
}

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_equalizer
{
    DeviceBuffers mem;
    uint8_t*      pool = NULL;
    EqualizePlan  plan;
    EqualizeStageEvents events;
};

static bool equalizer_given(const mrcal_amd_equalizer* e)
{
    if(e != NULL) return true;
    set_error("equalize(): the equalizer is NULL");
    return false;
}

extern "C" {

mrcal_amd_equalizer_t* mrcal_amd_equalizer_create(int width, int height, int dtype, const mrcal_amd_equalize_params_t* params)
{
    last_error_string().clear();
    if(params == NULL) { set_error("equalize(): the parameters are NULL"); return NULL; }
    const EqualizeParams p = equalize_params_of(params);
    std::string why;
    if(!equalize_params_ok(&why, width, height, dtype, p)) { set_error("%s", why.c_str()); return NULL; }
    if(p.method == EQUALIZE_METHOD_NONE) { set_error("equalize(): an equalizer needs a method: MRCAL_AMD_EQUALIZE_CLAHE or _STRETCH"); return NULL; }
    if(!have_device()) return NULL;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &total_bytes), return NULL);
    EqualizePlan plan;
    if(!equalize_plan(&plan, &why, width, height, dtype, p, free_bytes)) { set_error("%s", why.c_str()); return NULL; }

    mrcal_amd_equalizer* e = new mrcal_amd_equalizer;
    e->plan = plan;
    if(!e->mem.alloc(&e->pool, plan.bytes)) { delete e; return NULL; }
    if(!e->events.create()) { delete e; return NULL; }
    return e;
}

bool mrcal_amd_equalizer_apply(mrcal_amd_equalizer_t* e, const void* in, void* out)
{
    last_error_string().clear();
    if(!equalizer_given(e)) return false;
    if(in == NULL || out == NULL) { set_error("equalize(): an image is NULL"); return false; }
    if(!have_device()) return false;
    const EqualizePlan& p = e->plan;
    const size_t N = (size_t)p.W*(size_t)p.H;
    e->events.timed = false;
    HIP_TRY(hipMemcpy(e->pool + p.image, in, N*image_pixel_bytes(p.dtype), hipMemcpyHostToDevice), return false);
    if(!equalize_device(p, e->pool + p.image, e->pool + p.result, e->pool, &e->events)) return false;
    // (the copy waits for the launches)
    HIP_TRY(hipMemcpy(out, e->pool + p.result, N*image_pixel_bytes(p.dtype_out), hipMemcpyDeviceToHost), return false);
    e->events.timed = true;
    return true;
}

bool mrcal_amd_equalizer_stage_milliseconds(mrcal_amd_equalizer_t* e, float* milliseconds)
{
    last_error_string().clear();
    if(!equalizer_given(e)) return false;
    if(!e->events.timed) { set_error("equalize(): no image has been equalized yet"); return false; }
    for(int i = 0; i < 3; i++)
        if(!e->events.elapsed(&milliseconds[i], i, i+1)) return false;
    // (stretch has no such stage: what lies between its two events is no work)
    if(e->plan.method == EQUALIZE_METHOD_STRETCH) milliseconds[1] = 0.f;
    return true;
}

void mrcal_amd_equalizer_destroy(mrcal_amd_equalizer_t* e) { delete e; }

} // extern "C"
