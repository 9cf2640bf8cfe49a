// What match_feature.hip works out on the host before it touches the device: where each feature's template sits in
// image1, which part of image1 is searched, how large the match surface is and where it lies in the ONE pooled buffer
// all surfaces of a call share, the map each template is remapped through, and the sizes that are refused. Plain
// structs and vectors in and out, no HIP type or call. tests/hostcheck/match_plan_check.cpp runs it under the host
// sanitizers.
//
// A feature, with q1e its estimate in image1 and (tw,th) the template's size (include/mrcal_amd.h, "match_feature"):
//   tmin = rint(q1e - ((tw,th) - 1)/2), tmax = tmin + (tw,th) - 1        both inside image1, or the status is 3
//   map  = H01 applied to the integer pixels tmin..tmax, as float32      its four corners inside image0, or 4
//   qmin = max(tmin - r, 0), qmax = min(tmin + r + (tw,th) - 1, size1 - 1)
//   the surface has (qmax - qmin + 1) - (tw,th) + 1 entries each way
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "image_format.hpp"

namespace mrcal_amd {

enum { MATCH_OK = 0, MATCH_OPTIMUM_ON_EDGE = 1, MATCH_SUBPIXEL_DEGENERATE = 2, MATCH_OUTSIDE_IMAGE1 = 3, MATCH_OUTSIDE_IMAGE0 = 4 };

// the correlation kernel's tile of surface entries, and what a workgroup may stage
#define MATCH_TILE_X 64
#define MATCH_TILE_Y 16
#define MATCH_LDS_BYTES (160*1024)
// 2^32/255^2: as many products of two uint8 as a 32-bit sum holds exactly
#define MATCH_UINT8_TEMPLATE_PIXELS 66051

struct MatchFeaturePlan
{
    int    status;          // MATCH_OK, MATCH_OUTSIDE_IMAGE1 or MATCH_OUTSIDE_IMAGE0: what the host can tell
    int    tmin[2];         // the template's first pixel in image1 (x,y)
    int    qmin[2];         // the searched cut's first pixel in image1
    int    cut[2];          // its size (w,h)
    int    out[2];          // the surface's size (w,h); 0 for a feature that is not matched
    size_t offset;          // of the surface in the pooled buffer, in entries
    double qshift[2];       // qmin + q1e - tmin: surface coordinates -> image1 coordinates of the feature
};

struct MatchPlan
{
    std::vector<MatchFeaturePlan> features;
    size_t Nsurface = 0;            // entries of the pooled buffer
    int    tiles[2] = { 0, 0 };     // of the largest surface (x,y)
    int    pitch   = 0;             // of a staged row of image1: 32-bit words (uint8) or pixels
    int    tpitch  = 0;             // of a staged row of the template, likewise
    size_t lds_bytes = 0;
};

inline size_t match_pixel_bytes(int dtype) { return image_pixel_bytes(dtype); }   // (the name match_plan_check.cpp asks by)

// LDS of a workgroup: the patch of image1 under a tile (tile + template - 1) and the template.
// uint8 is staged as 32-bit words of four pixels; a lane reads the words tx .. tx + tpitch of a row, and the 16 lanes
// of the next row of the tile read theirs in the same instruction: with pitch = 16 mod 32 words the two rows fall on
// disjoint halves of the 32 banks a 4-byte read sees
inline void match_lds_layout(int* pitch, int* tpitch, size_t* bytes, int tw, int th, int dtype)
{
    const size_t rows = (size_t)MATCH_TILE_Y + th - 1;
    if(dtype == 0)
    {
        *tpitch = (tw + 3)/4;
        const int need = MATCH_TILE_X/4 + *tpitch;
        *pitch = 16 + 32*((need - 16 + 31)/32);
        *bytes = 4*(rows*(size_t)*pitch + (size_t)th*(size_t)*tpitch);
    }
    else
    {
        *tpitch = tw;
        *pitch  = MATCH_TILE_X + tw - 1;
        *bytes  = image_pixel_bytes(dtype)*(rows*(size_t)*pitch + (size_t)th*(size_t)tw);
    }
}

// the sizes that cannot be matched, for whatever data: false, and why
inline bool match_sizes_ok(std::string* error, int N, int tw, int th, int radius, int w0, int h0, int w1, int h1, int dtype)
{
    char buf[256];
    buf[0] = 0;
    if(!(image_dtype_is_integer(dtype) || dtype == IMAGE_DTYPE_FLOAT))
        snprintf(buf, sizeof(buf), "match_feature(): images are uint8, uint16 or float32");
    else if(N < 0 || N > (1 << 20))
        snprintf(buf, sizeof(buf), "match_feature(): %d features cannot be matched in one call (at most %d)", N, 1 << 20);
    else if(tw <= 0 || th <= 0)
        snprintf(buf, sizeof(buf), "match_feature(): Each element of template_size1 must be an integer > 0. Got (%d,%d)", tw, th);
    else if(radius < 0)
        snprintf(buf, sizeof(buf), "match_feature(): search_radius1 must be >= 0. Got %d", radius);
    else if(w0 <= 0 || h0 <= 0 || w1 <= 0 || h1 <= 0 || (long)w0*h0 > (1L << 30) || (long)w1*h1 > (1L << 30))
        snprintf(buf, sizeof(buf), "match_feature(): images of %d x %d and %d x %d pixels cannot be matched", w0, h0, w1, h1);
    else if(tw <= w1 && th <= h1)       // (a template larger than image1 fits nowhere: every feature gets status 3)
    {
        int pitch, tpitch; size_t bytes;
        match_lds_layout(&pitch, &tpitch, &bytes, tw, th, dtype);
        if(dtype == 0 && (long)tw*th > MATCH_UINT8_TEMPLATE_PIXELS)
            snprintf(buf, sizeof(buf), "match_feature(): a uint8 template of %d x %d pixels cannot be summed exactly in 32 bits (at most %d pixels)",
                     tw, th, MATCH_UINT8_TEMPLATE_PIXELS);
        else if(bytes > MATCH_LDS_BYTES)
            snprintf(buf, sizeof(buf), "match_feature(): a template of %d x %d pixels needs %zu bytes of LDS a workgroup; there are %d",
                     tw, th, bytes, MATCH_LDS_BYTES);
    }
    if(buf[0] == 0) return true;
    *error = buf;
    return false;
}

// One entry of the template map: H01 applied to the image1 pixel (x,y), in double, rounded to float32. Every product
// is its own statement, so that nothing is contracted into a fused multiply-add: the bits of the numpy expression
// ((h00*x + h01*y) + h02) / ((h20*x + h21*y) + h22)
inline void match_map_entry(float* mx, float* my, const double* H, double x, double y)
{
    const double h00x = H[0]*x; const double h01y = H[1]*y; const double nx0 = h00x + h01y; const double nx = nx0 + H[2];
    const double h10x = H[3]*x; const double h11y = H[4]*y; const double ny0 = h10x + h11y; const double ny = ny0 + H[5];
    const double h20x = H[6]*x; const double h21y = H[7]*y; const double d0  = h20x + h21y; const double d  = d0  + H[8];
    *mx = (float)(nx/d);
    *my = (float)(ny/d);
}

// the map (th,tw,2) of a feature whose template lies inside image1
inline void match_template_map(float* map, const MatchFeaturePlan& f, const double* H01, int tw, int th)
{
    for(int i = 0; i < th; i++)
        for(int j = 0; j < tw; j++)
            match_map_entry(&map[2*((size_t)i*tw + j)], &map[2*((size_t)i*tw + j) + 1], H01,
                            (double)(f.tmin[0] + j), (double)(f.tmin[1] + i));
}

// steps 1 and 3 of a feature, and the reference's four-corner test of step 2. q1e (2), H01 (9)
inline MatchFeaturePlan match_plan_feature(const double* q1e, const double* H01, int tw, int th, int radius,
                                           int w0, int h0, int w1, int h1)
{
    MatchFeaturePlan f;
    f.status = MATCH_OUTSIDE_IMAGE1;
    f.offset = 0;
    for(int k = 0; k < 2; k++) { f.tmin[k] = f.qmin[k] = f.cut[k] = f.out[k] = 0; f.qshift[k] = 0.0; }
    const int ts[2] = { tw, th }, size1[2] = { w1, h1 };
    for(int k = 0; k < 2; k++)
    {
        const double t = rint(q1e[k] - ((double)ts[k] - 1.)/2.);      // (halves to even, as numpy.round)
        if(!(t >= 0.0 && t + (double)ts[k] - 1. < (double)size1[k])) return f;          // (a NaN: outside)
        f.tmin[k] = (int)t;
    }
    f.status = MATCH_OUTSIDE_IMAGE0;
    for(int corner = 0; corner < 4; corner++)
    {
        float x, y;
        match_map_entry(&x, &y, H01, (double)(f.tmin[0] + ((corner & 1) ? tw - 1 : 0)), (double)(f.tmin[1] + ((corner & 2) ? th - 1 : 0)));
        if(!(x >= 0.f && y >= 0.f && x < (float)w0 && y < (float)h0)) return f;
    }
    f.status = MATCH_OK;
    for(int k = 0; k < 2; k++)
    {
        // (in long: a radius near INT_MAX is a legitimate way to say "everywhere")
        const long lo = (long)f.tmin[k] - radius, hi = (long)f.tmin[k] + radius + ts[k] - 1;
        f.qmin[k]   = (int)(lo > 0 ? lo : 0);
        const int qmax = (int)(hi < size1[k] - 1 ? hi : size1[k] - 1);
        f.cut[k]    = qmax - f.qmin[k] + 1;
        f.out[k]    = f.cut[k] - ts[k] + 1;
        const double a = (double)f.qmin[k] + q1e[k];
        f.qshift[k] = a - (double)f.tmin[k];
    }
    return f;
}

// the whole call. q1e (N,2), H01 (N,3,3). false: a size that is refused, with the reason in *error
inline bool match_plan(MatchPlan* plan, std::string* error, int N, const double* q1e, const double* H01,
                       int tw, int th, int radius, int w0, int h0, int w1, int h1, int dtype)
{
    *plan = MatchPlan();
    if(!match_sizes_ok(error, N, tw, th, radius, w0, h0, w1, h1, dtype)) return false;
    match_lds_layout(&plan->pitch, &plan->tpitch, &plan->lds_bytes, tw, th, dtype);
    plan->features.reserve((size_t)N);
    for(int i = 0; i < N; i++)
    {
        MatchFeaturePlan f = match_plan_feature(q1e + 2*(size_t)i, H01 + 9*(size_t)i, tw, th, radius, w0, h0, w1, h1);
        if(f.status != MATCH_OK) f.out[0] = f.out[1] = 0;
        f.offset = plan->Nsurface;
        plan->Nsurface += (size_t)f.out[0]*(size_t)f.out[1];
        for(int k = 0; k < 2; k++)
        {
            const int tile  = k == 0 ? MATCH_TILE_X : MATCH_TILE_Y;
            const int tiles = (f.out[k] + tile - 1)/tile;
            if(tiles > plan->tiles[k]) plan->tiles[k] = tiles;
        }
        plan->features.push_back(f);
    }
    // a workgroup per tile of the LARGEST surface and feature, in one launch
    const size_t groups = (size_t)plan->tiles[0]*(size_t)plan->tiles[1]*(size_t)N;
    if(plan->Nsurface > ((size_t)1 << 31) || groups > ((size_t)1 << 30))
    {
        char buf[256];
        snprintf(buf, sizeof(buf), "match_feature(): %d features with %zu surface entries in all are too many for one call (at most 2^31)", N, plan->Nsurface);
        *error = buf;
        return false;
    }
    return true;
}

} // namespace mrcal_amd
