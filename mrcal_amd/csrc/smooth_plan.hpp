// What smooth.hip works out on the host before it touches the device: the arguments that are refused, the integer taps
// of both axes, the tile a workgroup makes with its halo, the LDS it needs for that, the grid, where the image and the
// result lie in the ONE pooled allocation a smoother owns, and the refusal of an image that does not fit the device's
// free memory (the caller passes that figure in). Plain structs in and out, no HIP type or call.
// tests/hostcheck/smooth_plan_check.cpp runs it under the host sanitizers.
//
// What the filter is: include/mrcal_amd.h, "smoothing".
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "image_format.hpp"

namespace mrcal_amd {

#define SMOOTH_SIGMA_MIN    0.5
#define SMOOTH_SIGMA_MAX    8.0
#define SMOOTH_R_MAX        24          // ceil(3 SMOOTH_SIGMA_MAX)
#define SMOOTH_ALIGN        256         // of the parts of the pool, in bytes
#define SMOOTH_THREADS      256
#define SMOOTH_QUAD         4           // the pixels of a row one lane makes at a time
#define SMOOTH_SUM_ROW_BYTES 512        // of a tile's row of horizontal sums in LDS: 256 uint16 of a uint8 image, 128 uint32 of a uint16 one
#define SMOOTH_LDS_TARGET   40960       // the tile is as high (64, 32, 16 or 8 rows) as this allows: four workgroups a CU
#define SMOOTH_LDS_MAX      65536       // ... and 8 rows fit this at every radius

struct SmoothParams
{
    double sigma_x = 0.0, sigma_y = 0.0;
};

struct SmoothPlan
{
    int      dtype = 0;
    int      W = 0, H = 0;
    int      Rx = 0, Ry = 0;
    int      wx[SMOOTH_R_MAX + 1] = {}, wy[SMOOTH_R_MAX + 1] = {};     // w_0 .. w_R; w_-k = w_k
    // the tile: tile_w x tile_h pixels of the result a workgroup. It stages rows x (tile_w + 2 halo_x) pixels of the
    // image, halo_x = Rx rounded up to whole quads, and keeps rows x tile_w horizontal sums
    int      tile_w = 0, tile_h = 0, halo_x = 0, rows = 0;
    int      raw_dwords = 0;                // of a staged row: its pixels and one dword more, which the last window reads into
    unsigned lds_t = 0, lds_bytes = 0;      // the staged rows lie at 0, the sums at lds_t
    unsigned grid_x = 0, grid_y = 0, grid = 0;      // tiles across and down; the grid is their product, in ONE dimension
    // offsets into the pool, in bytes
    size_t   image = 0, result = 0;
    size_t   bytes = 0;
};

inline size_t smooth_aligned(size_t n) { return (n + SMOOTH_ALIGN - 1)/SMOOTH_ALIGN*SMOOTH_ALIGN; }
// 0, or in [0.5, 8]; a NaN is neither
inline bool smooth_sigma_ok(double sigma) { return sigma == 0.0 || (sigma >= SMOOTH_SIGMA_MIN && sigma <= SMOOTH_SIGMA_MAX); }
inline bool smooth_is_off(const SmoothParams& p) { return p.sigma_x == 0.0 && p.sigma_y == 0.0; }

// The integer taps of one axis, w[0..R], summing to 256 with their mirror images (include/mrcal_amd.h, "smoothing": taps).
// Any sigma > 0 whose radius is at most SMOOTH_R_MAX is served; sigma == 0: the one tap 256
inline bool smooth_weights(int* R, int* w, double sigma)
{
    if(sigma == 0.0) { *R = 0; w[0] = 256; return true; }
    if(!(sigma > 0.0) || ceil(3.0*sigma) > (double)SMOOTH_R_MAX) return false;
    const int r = (int)ceil(3.0*sigma);
    double g[SMOOTH_R_MAX + 1];
    double S = 0.0;
    for(int k = 0; k <= r; k++) g[k] = exp(-(double)(k*k)/(2.0*sigma*sigma));
    for(int k = 1; k <= r; k++) S += g[k];
    S = g[0] + 2.0*S;
    // error diffusion from the outside in: what rounding one tap loses, the next one is given
    double e = 0.0;
    int sum = 0;
    for(int k = r; k >= 1; k--)
    {
        const double a = 256.0*g[k]/S;
        w[k] = (int)floor(a + e + 0.5);
        e += a - (double)w[k];
        sum += w[k];
    }
    w[0] = 256 - 2*sum;
    *R = r;
    return true;
}

// tap k of an axis, k = -R .. R, and 0 beyond: the windows of the kernel are made of these
inline int smooth_tap(const int* w, int R, int k) { k = k < 0 ? -k : k; return k <= R ? w[k] : 0; }

// the arguments that cannot be smoothed, for whatever data: false, and why
inline bool smooth_params_ok(std::string* error, int W, int H, int dtype, const SmoothParams& p)
{
    char buf[256];
    buf[0] = 0;
    if(!smooth_sigma_ok(p.sigma_x) || !smooth_sigma_ok(p.sigma_y))
        snprintf(buf, sizeof(buf), "smooth(): a sigma is 0 (that axis is not filtered) or lies in [%g, %g]. Got (%g,%g)",
                 SMOOTH_SIGMA_MIN, SMOOTH_SIGMA_MAX, p.sigma_x, p.sigma_y);
    else if(smooth_is_off(p))
        snprintf(buf, sizeof(buf), "smooth(): both sigmas are 0: there is nothing to run");
    else if(!image_dtype_is_integer(dtype))
        snprintf(buf, sizeof(buf), "smooth(): images are uint8 or uint16");
    else if(!image_size_ok(W, H))
        snprintf(buf, sizeof(buf), "smooth(): images of %d x %d pixels cannot be smoothed", W, H);
    if(buf[0] == 0) return true;
    *error = buf;
    return false;
}

// the whole plan. free_bytes: what the device has free. false: a refusal, with the reason in *error.
// with_images: the pool holds the input and the output (a stand-alone smoother); without, there is no pool
inline bool smooth_plan(SmoothPlan* plan, std::string* error, int W, int H, int dtype, const SmoothParams& p,
                        size_t free_bytes, bool with_images = true)
{
    *plan = SmoothPlan();
    if(!smooth_params_ok(error, W, H, dtype, p)) return false;
    SmoothPlan q;
    q.dtype = dtype; q.W = W; q.H = H;
    if(!smooth_weights(&q.Rx, q.wx, p.sigma_x) || !smooth_weights(&q.Ry, q.wy, p.sigma_y))
    { *error = "smooth(): internal error: a sigma that was accepted has no taps"; return false; }

    const int px = (int)image_pixel_bytes(dtype);
    q.tile_w     = SMOOTH_SUM_ROW_BYTES/(2*px);                // a sum has twice the pixel's bytes
    q.halo_x     = (q.Rx + SMOOTH_QUAD - 1)/SMOOTH_QUAD*SMOOTH_QUAD;
    q.raw_dwords = (q.tile_w + 2*q.halo_x)*px/4 + 1;
    for(q.tile_h = 64; ; q.tile_h /= 2)
    {
        q.rows      = q.tile_h + 2*q.Ry;
        q.lds_t     = (unsigned)((q.rows*q.raw_dwords*4 + 15)/16*16);
        q.lds_bytes = q.lds_t + (unsigned)(q.rows*SMOOTH_SUM_ROW_BYTES);
        if(q.lds_bytes <= SMOOTH_LDS_TARGET || q.tile_h == 8) break;
    }
    if(q.lds_bytes > SMOOTH_LDS_MAX) { *error = "smooth(): internal error: the tile does not fit the LDS"; return false; }
    q.grid_x = (unsigned)((W + q.tile_w - 1)/q.tile_w);
    q.grid_y = (unsigned)((H + q.tile_h - 1)/q.tile_h);
    q.grid   = q.grid_x*q.grid_y;                           // (<= 2^28/(128 8) + what the edges add)

    if(with_images)
    {
        const size_t N = (size_t)W*(size_t)H;
        q.image  = 0;
        q.result = smooth_aligned(N*px);
        q.bytes  = q.result + smooth_aligned(N*px);
    }
    if(q.bytes > free_bytes)
    {
        char buf[256];
        snprintf(buf, sizeof(buf), "smooth(): %d x %d pixels need %zu bytes of device memory; %zu are free", W, H, q.bytes, free_bytes);
        *error = buf;
        return false;
    }
    *plan = q;
    return true;
}

} // namespace mrcal_amd
