// What equalize.hip works out on the host before it touches the device: the arguments that are refused, the padded
// and the tile sizes of CLAHE, its clip limit and LUT scale, where the image, the result, the histograms, the LUTs and
// the extremes lie in the ONE pooled allocation an equalizer owns, the launch geometry of every kernel, and the refusal
// of an image that does not fit the device's free memory (the caller passes that figure in). Plain structs in and out,
// no HIP type or call. tests/hostcheck/equalize_plan_check.cpp runs it under the host sanitizers.
//
// What the equalization is: include/mrcal_amd.h, "equalization".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "image_format.hpp"

namespace mrcal_amd {

// (the values of MRCAL_AMD_EQUALIZE_*, which this file does not include)
#define EQUALIZE_METHOD_NONE    0
#define EQUALIZE_METHOD_CLAHE   1
#define EQUALIZE_METHOD_STRETCH 2
#define EQUALIZE_DTYPE_UINT8    IMAGE_DTYPE_UINT8       // (the name equalize_plan_check.cpp asks by)

#define EQUALIZE_MAX_TILES  4096        // tiles_x tiles_y: what the histograms of a uint16 image may still cost (1 GiB)
#define EQUALIZE_ALIGN      256         // of the parts of the pool, in bytes
#define EQUALIZE_THREADS    256         // of the histogram, apply, extremes and map kernels
#define EQUALIZE_BAND_ROWS  32          // the rows of a tile one workgroup of the histogram kernel counts
#define EQUALIZE_APPLY_X    4           // the pixels of a row one lane of the apply kernel interpolates
#define EQUALIZE_APPLY_ROWS 16          // the rows a workgroup of the apply kernel covers, 256 x 4 pixels wide
#define EQUALIZE_LDS_LUT_BYTES 32768    // the uint8 LUTs of all tiles are staged in LDS if they fit this
#define EQUALIZE_MAP_PIXELS 4           // the pixels one lane of the stretch's two kernels takes at a time
#define EQUALIZE_MINMAX_GRID_MAX 512     // workgroups of the extremes: each ends in one pair of atomics on the same two words

struct EqualizeParams
{
    int    method = EQUALIZE_METHOD_NONE;
    double clip_limit = 8.0;
    int    tiles_x = 8, tiles_y = 8;
};

struct EqualizePlan
{
    int      method = EQUALIZE_METHOD_NONE, dtype = 0, dtype_out = 0;
    int      W = 0, H = 0;
    // CLAHE
    int      tiles_x = 0, tiles_y = 0;
    int      Wpad = 0, Hpad = 0, tw = 0, th = 0;
    int      hist_size = 0;
    int      clip = 0;                      // INT32_MAX: no clipping
    float    lut_scale = 0.f, inv_tw = 0.f, inv_th = 0.f;
    bool     luts_in_lds = false;
    unsigned bands = 0;                     // row bands a tile: hist grid = tiles_x tiles_y bands
    unsigned hist_grid = 0, lut_grid = 0, lut_threads = 0;
    unsigned apply_grid_x = 0, apply_grid_y = 0, apply_grid = 0;     // blocks across and down; the grid is their product, in ONE dimension
    // stretch
    unsigned minmax_grid = 0, map_grid = 0;
    // offsets into the pool, in bytes
    size_t   image = 0, result = 0;         // the input and the output, dense
    size_t   hist = 0, hist_bytes = 0;      // uint32 [tiles_y][tiles_x][hist_size]
    size_t   lut = 0;                       // the image's type [tiles_y][tiles_x][hist_size]
    size_t   minmax = 0;                    // uint32 [2]
    size_t   workspace = 0;                 // the first byte after image and result: hist, lut, minmax
    size_t   bytes = 0;                     // of the pool
};

inline size_t equalize_aligned(size_t n) { return (n + EQUALIZE_ALIGN - 1)/EQUALIZE_ALIGN*EQUALIZE_ALIGN; }
// stretch makes uint8 of everything; CLAHE keeps the type
inline int equalize_dtype_out(int method, int dtype) { return method == EQUALIZE_METHOD_STRETCH ? IMAGE_DTYPE_UINT8 : dtype; }

// the arguments that cannot be equalized, for whatever data: false, and why
inline bool equalize_params_ok(std::string* error, int W, int H, int dtype, const EqualizeParams& p)
{
    char buf[256];
    buf[0] = 0;
    if(!(p.method == EQUALIZE_METHOD_NONE || p.method == EQUALIZE_METHOD_CLAHE || p.method == EQUALIZE_METHOD_STRETCH))
        snprintf(buf, sizeof(buf), "equalize(): the method must be one of MRCAL_AMD_EQUALIZE_* (0..2), not %d", p.method);
    else if(!image_dtype_is_integer(dtype))
        snprintf(buf, sizeof(buf), "equalize(): images are uint8 or uint16");
    else if(!image_size_ok(W, H))
        snprintf(buf, sizeof(buf), "equalize(): images of %d x %d pixels cannot be equalized", W, H);
    else if(p.method == EQUALIZE_METHOD_CLAHE)
    {
        if(p.tiles_x < 1 || p.tiles_y < 1 || (long)p.tiles_x*p.tiles_y > EQUALIZE_MAX_TILES)
            snprintf(buf, sizeof(buf), "equalize(): tiles must be at least (1,1) and at most %d in all. Got (%d,%d)",
                     EQUALIZE_MAX_TILES, p.tiles_x, p.tiles_y);
        else if(!(p.clip_limit == p.clip_limit))
            snprintf(buf, sizeof(buf), "equalize(): clip_limit is not a number");
        else if(W % p.tiles_x != 0 || H % p.tiles_y != 0)
        {
            // both sides are padded, the divisible one by a whole `tiles`; by reflection, which reaches W-1, H-1 pixels back
            const int px = p.tiles_x - W % p.tiles_x, py = p.tiles_y - H % p.tiles_y;
            if(px > W - 1 || py > H - 1)
                snprintf(buf, sizeof(buf), "equalize(): an image of %d x %d pixels is too small for (%d,%d) tiles: it would be padded by (%d,%d) pixels, and a reflection reaches (%d,%d)",
                         W, H, p.tiles_x, p.tiles_y, px, py, W - 1, H - 1);
        }
    }
    if(buf[0] == 0) return true;
    *error = buf;
    return false;
}

// the whole plan. free_bytes: what the device has free. false: a refusal, with the reason in *error.
// with_images: the pool holds the input and the output too (a stand-alone equalizer); without, the workspace alone
inline bool equalize_plan(EqualizePlan* plan, std::string* error, int W, int H, int dtype, const EqualizeParams& p,
                          size_t free_bytes, bool with_images = true)
{
    *plan = EqualizePlan();
    if(!equalize_params_ok(error, W, H, dtype, p)) return false;
    EqualizePlan q;
    q.method = p.method; q.dtype = dtype; q.dtype_out = equalize_dtype_out(p.method, dtype);
    q.W = W; q.H = H;
    const size_t N = (size_t)W*(size_t)H;
    if(with_images)
    {
        q.image     = 0;
        q.result    = equalize_aligned(N*image_pixel_bytes(dtype));
        q.workspace = q.result + equalize_aligned(N*image_pixel_bytes(q.dtype_out));
    }
    q.hist = q.lut = q.minmax = q.bytes = q.workspace;
    if(p.method == EQUALIZE_METHOD_CLAHE)
    {
        q.tiles_x = p.tiles_x; q.tiles_y = p.tiles_y;
        const bool pad = W % p.tiles_x != 0 || H % p.tiles_y != 0;
        q.Wpad = pad ? W + p.tiles_x - W % p.tiles_x : W;
        q.Hpad = pad ? H + p.tiles_y - H % p.tiles_y : H;
        q.tw = q.Wpad/p.tiles_x; q.th = q.Hpad/p.tiles_y;
        q.hist_size = dtype == IMAGE_DTYPE_UINT8 ? 256 : 65536;
        const int total = q.tw*q.th;                    // (<= 2^28 + what the padding adds: fits)
        q.lut_scale = (float)(q.hist_size - 1) / (float)total;
        q.inv_tw = 1.0f / (float)q.tw;
        q.inv_th = 1.0f / (float)q.th;
        q.clip = INT32_MAX;
        if(p.clip_limit > 0.0)
        {
            const double c = p.clip_limit*(double)total/(double)q.hist_size;
            q.clip = c >= (double)INT32_MAX ? INT32_MAX : (int)c;
            if(q.clip < 1) q.clip = 1;
        }
        const size_t tiles = (size_t)q.tiles_x*(size_t)q.tiles_y;
        q.luts_in_lds = dtype == IMAGE_DTYPE_UINT8 && tiles*256 <= EQUALIZE_LDS_LUT_BYTES;
        q.bands       = (unsigned)((q.th + EQUALIZE_BAND_ROWS - 1)/EQUALIZE_BAND_ROWS);
        q.hist_grid   = (unsigned)tiles*q.bands;
        q.lut_grid    = (unsigned)tiles;
        q.lut_threads = dtype == IMAGE_DTYPE_UINT8 ? 64 : 1024;
        q.apply_grid_x = (unsigned)((W + EQUALIZE_THREADS*EQUALIZE_APPLY_X - 1)/(EQUALIZE_THREADS*EQUALIZE_APPLY_X));
        q.apply_grid_y = (unsigned)((H + EQUALIZE_APPLY_ROWS - 1)/EQUALIZE_APPLY_ROWS);
        q.apply_grid   = q.apply_grid_x*q.apply_grid_y;          // (<= 2^28/16 + what the edges add)
        q.hist_bytes = tiles*(size_t)q.hist_size*sizeof(uint32_t);
        q.hist  = q.workspace;
        q.lut   = q.hist + equalize_aligned(q.hist_bytes);
        q.bytes = q.lut + equalize_aligned(tiles*(size_t)q.hist_size*image_pixel_bytes(dtype));
        q.minmax = q.bytes;
    }
    else if(p.method == EQUALIZE_METHOD_STRETCH)
    {
        const size_t per_block = (size_t)EQUALIZE_THREADS*EQUALIZE_MAP_PIXELS;
        const size_t blocks = (N + per_block - 1)/per_block;
        q.map_grid    = (unsigned)blocks;
        q.minmax_grid = (unsigned)(blocks < EQUALIZE_MINMAX_GRID_MAX ? blocks : EQUALIZE_MINMAX_GRID_MAX);
        q.minmax = q.workspace;
        q.bytes  = q.minmax + EQUALIZE_ALIGN;
    }
    if(q.bytes == 0) q.bytes = EQUALIZE_ALIGN;          // (no method and no images: nothing is needed)
    if(q.bytes > free_bytes)
    {
        char buf[256];
        snprintf(buf, sizeof(buf), "equalize(): %d x %d pixels need %zu bytes of device memory; %zu are free", W, H, q.bytes, free_bytes);
        *error = buf;
        return false;
    }
    *plan = q;
    return true;
}

} // namespace mrcal_amd
