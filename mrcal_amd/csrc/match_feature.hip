// match_feature(): template matching between two images (include/mrcal_amd.h, "match_feature"). Reference:
// mrcal/stereo.py:1609-2090, which hands the correlation to cv2.matchTemplate().
//
//   the templates    ONE remap_device() call (rectification.hip, through remap.hpp) for the N templates of a call: the
//                    maps are made on the host (match_plan.hpp) and uploaded as one array
//   mf_template_sums_kernel<T>
//                    a workgroup a feature: ST and ST2 of its template, summed in a fixed order
//   mf_correlate_kernel<T,METHOD>
//                    the hot path. ONE launch for all features: a workgroup covers a 64 x 16 tile of one feature's
//                    match surface. It stages the patch of image1 under the tile (tile + template - 1) and the
//                    template in LDS, and takes IT = sum I T, SI = sum I, SI2 = sum I^2 of each window from that
//                    staged data: image1 is read from memory once a tile.
//                      uint8:   four pixels to a 32-bit word. A lane owns 4 consecutive entries of a row: it reads
//                               the ALIGNED words of the patch row, makes the words that begin 1, 2, 3 bytes later
//                               with v_alignbyte_b32 in registers, and sums with v_dot4_u32_u8 into 32 bits: exact up
//                               to 66051 template pixels, more are refused. The only LDS reads are aligned 4-byte ones:
//                               16 consecutive words for the 16 lanes of a tile row, and with a pitch of 16 mod 32
//                               words the two tile rows of a 32-lane group use disjoint banks
//                      uint16:  64-bit integer multiply-adds, exact
//                      float32: double (a product of two float32 is exact in double), summed row by row, left to right
//                               a lane of the latter two owns the column tx of 4 tile rows: the 64 lanes of a wave read 64
//                               consecutive pixels
//                    then the method's formula in double, rounded to float32
//   mf_peak_kernel   a workgroup a feature: the optimum of the surface by a fixed-order reduction that carries
//                    (value, flat index), the first index winning ties as numpy.argmax does; then one thread does the
//                    edge test, the subpixel fit and q1
// No atomics: the same bits on every call. The surfaces leave the device only when they are asked for.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/mrcal_amd.h"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "remap.hpp"
#include "equalize.hpp"
#include "image_prepare.hpp"
#include "match_plan.hpp"

namespace mrcal_amd {

namespace {

#define MF_THREADS 256

// a feature as the kernels see it
struct MfFeature
{
    int       status;
    int       qmin[2];      // the cut's first pixel in image1
    int       cut[2];       // its size
    int       out[2];       // the surface's size
    long long offset;       // of the surface in the pool
    double    qshift[2];
};
struct MfArgs
{
    int W1;                 // image1's width
    int tw, th;
    int tiles[2];           // of the largest surface
    int pitch, tpitch;      // match_plan.hpp: match_lds_layout()
};
struct MfTemplateSums { double ST, ST2; };

template<int METHOD> struct MfNeeds
{
    static constexpr bool SI  = METHOD == MRCAL_AMD_TM_CCOEFF || METHOD == MRCAL_AMD_TM_CCOEFF_NORMED;
    static constexpr bool SI2 = METHOD == MRCAL_AMD_TM_SQDIFF || METHOD == MRCAL_AMD_TM_SQDIFF_NORMED ||
                                METHOD == MRCAL_AMD_TM_CCORR_NORMED || METHOD == MRCAL_AMD_TM_CCOEFF_NORMED;
};

// The six formulas, in double; every product its own statement. A denominator that is not > 0: 0 (1 for SQDIFF_NORMED)
template<int METHOD>
__device__ __forceinline__
float mf_score(double IT, double SI, double SI2, double ST, double ST2, double N)
{
    if(METHOD == MRCAL_AMD_TM_CCORR) return (float)IT;
    if(METHOD == MRCAL_AMD_TM_SQDIFF || METHOD == MRCAL_AMD_TM_SQDIFF_NORMED)
    {
        const double twice = 2.0*IT;
        const double d     = SI2 - twice;
        const double num   = d + ST2;
        if(METHOD == MRCAL_AMD_TM_SQDIFF) return (float)num;
        const double p   = SI2*ST2;
        const double den = sqrt(p);
        return den > 0.0 ? (float)(num/den) : 1.f;
    }
    if(METHOD == MRCAL_AMD_TM_CCORR_NORMED)
    {
        const double p   = SI2*ST2;
        const double den = sqrt(p);
        return den > 0.0 ? (float)(IT/den) : 0.f;
    }
    const double sist = SI*ST;
    const double mean = sist/N;
    const double num  = IT - mean;
    if(METHOD == MRCAL_AMD_TM_CCOEFF) return (float)num;
    const double sisi = SI*SI;
    const double qi   = sisi/N;
    const double vi   = fmax(SI2 - qi, 0.0);
    const double stst = ST*ST;
    const double qt   = stst/N;
    const double vt   = fmax(ST2 - qt, 0.0);
    const double p    = vi*vt;
    const double den  = sqrt(p);
    return den > 0.0 ? (float)(num/den) : 0.f;
}

// which tile of which feature this workgroup has; false: none (the feature is not matched, or its surface is smaller
// than the largest one). Uniform over the workgroup
__device__ __forceinline__
bool mf_tile(MfFeature* F, int* ifeature, int* x0, int* y0, const MfArgs& a, const MfFeature* __restrict__ features)
{
    const int tiles = a.tiles[0]*a.tiles[1];
    const int f = blockIdx.x / tiles, t = blockIdx.x - f*tiles;
    const int ty = t / a.tiles[0];
    *F = features[f];
    *ifeature = f;
    *x0 = (t - ty*a.tiles[0])*MATCH_TILE_X;
    *y0 = ty*MATCH_TILE_Y;
    return F->status == MATCH_OK && *x0 < F->out[0] && *y0 < F->out[1];
}

////////////////////////////////////////////////////////////////////////////////
// uint8
////////////////////////////////////////////////////////////////////////////////
template<int METHOD>
__global__ __launch_bounds__(MF_THREADS)
void mf_correlate_u8_kernel(MfArgs a, const uint8_t* __restrict__ image1, const uint8_t* __restrict__ templates,
                            const MfFeature* __restrict__ features, const MfTemplateSums* __restrict__ sums,
                            float* __restrict__ surfaces)
{
    extern __shared__ uint32_t mf_lds[];
    MfFeature F; int f, x0, y0;
    if(!mf_tile(&F, &f, &x0, &y0, a, features)) return;

    const int prows = MATCH_TILE_Y + a.th - 1;
    uint32_t* patch = mf_lds;                       // [prows][pitch]
    uint32_t* tpl   = mf_lds + prows*a.pitch;       // [th][tpitch], the last word of a row padded with zeros
    const uint8_t* T = templates + (size_t)f*a.tw*a.th;
    for(int i = threadIdx.x; i < a.th*a.tpitch; i += MF_THREADS)
    {
        const int r = i / a.tpitch, c = 4*(i - r*a.tpitch);
        uint32_t w = 0;
#pragma unroll
        for(int b = 0; b < 4; b++)
            if(c + b < a.tw) w |= (uint32_t)T[r*a.tw + c + b] << (8*b);
        tpl[i] = w;
    }
    // the patch: what lies beyond the cut (only entries that are not stored look at it) is 0
    const int gx0 = F.qmin[0] + x0, gy0 = F.qmin[1] + y0;
    const int gx1 = F.qmin[0] + F.cut[0], gy1 = F.qmin[1] + F.cut[1];      // one past the cut
    for(int i = threadIdx.x; i < prows*a.pitch; i += MF_THREADS)
    {
        const int r = i / a.pitch, c = 4*(i - r*a.pitch);
        const int gy = gy0 + r, gx = gx0 + c;
        uint32_t w = 0;
        if(gy < gy1)
        {
            const uint8_t* row = image1 + (size_t)gy*a.W1;
#pragma unroll
            for(int b = 0; b < 4; b++)
                if(gx + b < gx1) w |= (uint32_t)row[gx + b] << (8*b);
        }
        patch[i] = w;
    }
    __syncthreads();

    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    uint32_t IT[4] = { 0, 0, 0, 0 }, SI[4] = { 0, 0, 0, 0 }, SI2[4] = { 0, 0, 0, 0 };
    // the window of entry s of this lane begins s bytes into word tx of the row
    auto step = [&](uint32_t w0, uint32_t w1, uint32_t t, uint32_t mask)
    {
        const uint32_t v[4] = { w0, __builtin_amdgcn_alignbyte(w1, w0, 1), __builtin_amdgcn_alignbyte(w1, w0, 2),
                                __builtin_amdgcn_alignbyte(w1, w0, 3) };
#pragma unroll
        for(int s = 0; s < 4; s++)
        {
            IT[s] = __builtin_amdgcn_udot4(v[s], t, IT[s], false);
            if(MfNeeds<METHOD>::SI)  SI[s]  = __builtin_amdgcn_udot4(v[s], mask & 0x01010101u, SI[s], false);
            if(MfNeeds<METHOD>::SI2) SI2[s] = __builtin_amdgcn_udot4(v[s] & mask, v[s], SI2[s], false);
        }
    };
    const int      nfull    = a.tw/4;
    const uint32_t lastmask = (a.tw & 3) ? 0xFFFFFFFFu >> (8*(4 - (a.tw & 3))) : 0xFFFFFFFFu;   // (the pixels of the last word that are the template's)
    for(int dy = 0; dy < a.th; dy++)
    {
        const uint32_t* prow = patch + (ty + dy)*a.pitch + tx;
        const uint32_t* trow = tpl + dy*a.tpitch;
        uint32_t w0 = prow[0];
        for(int k = 0; k < nfull; k++)
        {
            const uint32_t w1 = prow[k + 1];
            step(w0, w1, trow[k], 0xFFFFFFFFu);
            w0 = w1;
        }
        if(nfull < a.tpitch) step(w0, prow[nfull + 1], trow[nfull], lastmask);
    }

    const MfTemplateSums S = sums[f];
    const double N = (double)(a.tw*a.th);
    const int y = y0 + ty;
    if(y >= F.out[1]) return;
    float* out = surfaces + F.offset + (size_t)y*F.out[0];
#pragma unroll
    for(int s = 0; s < 4; s++)
    {
        const int x = x0 + 4*tx + s;
        if(x < F.out[0]) out[x] = mf_score<METHOD>((double)IT[s], (double)SI[s], (double)SI2[s], S.ST, S.ST2, N);
    }
}

////////////////////////////////////////////////////////////////////////////////
// uint16, float32
////////////////////////////////////////////////////////////////////////////////
template<class T> struct MfSum;
template<> struct MfSum<uint8_t>  { typedef uint64_t type; };
template<> struct MfSum<uint16_t> { typedef uint64_t type; };
template<> struct MfSum<float>    { typedef double   type; };

// acc + a b, exactly: uint16 in 64-bit integers; float32 in double, where the product is exact and only the sum rounds
__device__ __forceinline__ uint64_t mf_mad(uint64_t acc, uint16_t a, uint16_t b) { return acc + (uint64_t)((uint32_t)a*(uint32_t)b); }
__device__ __forceinline__ uint64_t mf_mad(uint64_t acc, uint8_t a, uint8_t b)   { return acc + (uint64_t)((uint32_t)a*(uint32_t)b); }
__device__ __forceinline__ double   mf_mad(double acc, float a, float b)         { const double p = (double)a*(double)b; return acc + p; }

template<class T, int METHOD>
__global__ __launch_bounds__(MF_THREADS)
void mf_correlate_kernel(MfArgs a, const T* __restrict__ image1, const T* __restrict__ templates,
                         const MfFeature* __restrict__ features, const MfTemplateSums* __restrict__ sums,
                         float* __restrict__ surfaces)
{
    typedef typename MfSum<T>::type Sum;
    extern __shared__ uint32_t mf_lds[];
    MfFeature F; int f, x0, y0;
    if(!mf_tile(&F, &f, &x0, &y0, a, features)) return;

    const int prows = MATCH_TILE_Y + a.th - 1;
    T* patch = (T*)mf_lds;                          // [prows][pitch]
    T* tpl   = patch + prows*a.pitch;               // [th][tw]
    const T* Tf = templates + (size_t)f*a.tw*a.th;
    for(int i = threadIdx.x; i < a.th*a.tw; i += MF_THREADS) tpl[i] = Tf[i];
    const int gx0 = F.qmin[0] + x0, gy0 = F.qmin[1] + y0;
    const int gx1 = F.qmin[0] + F.cut[0], gy1 = F.qmin[1] + F.cut[1];
    for(int i = threadIdx.x; i < prows*a.pitch; i += MF_THREADS)
    {
        const int r = i / a.pitch, c = i - r*a.pitch;
        const int gy = gy0 + r, gx = gx0 + c;
        patch[i] = (gy < gy1 && gx < gx1) ? image1[(size_t)gy*a.W1 + gx] : (T)0;
    }
    __syncthreads();

    // a lane: the column tx of the tile rows ty, ty + 4, ty + 8, ty + 12
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    Sum IT[4] = { 0, 0, 0, 0 }, SI[4] = { 0, 0, 0, 0 }, SI2[4] = { 0, 0, 0, 0 };
    for(int dy = 0; dy < a.th; dy++)
        for(int dx = 0; dx < a.tw; dx++)
        {
            const T t = tpl[dy*a.tw + dx];
#pragma unroll
            for(int k = 0; k < 4; k++)
            {
                const T v = patch[(ty + 4*k + dy)*a.pitch + tx + dx];
                IT[k] = mf_mad(IT[k], v, t);
                if(MfNeeds<METHOD>::SI)  SI[k]  = SI[k] + (Sum)v;
                if(MfNeeds<METHOD>::SI2) SI2[k] = mf_mad(SI2[k], v, v);
            }
        }

    const MfTemplateSums S = sums[f];
    const double N = (double)(a.tw*a.th);
    const int x = x0 + tx;
    if(x >= F.out[0]) return;
#pragma unroll
    for(int k = 0; k < 4; k++)
    {
        const int y = y0 + ty + 4*k;
        if(y < F.out[1])
            surfaces[F.offset + (size_t)y*F.out[0] + x] = mf_score<METHOD>((double)IT[k], (double)SI[k], (double)SI2[k], S.ST, S.ST2, N);
    }
}

////////////////////////////////////////////////////////////////////////////////
// the template's own sums
////////////////////////////////////////////////////////////////////////////////
// lane i sums the pixels i, i + 256, ... in that order; then the 256 partial sums pairwise, the same pairs every time
template<class T>
__global__ __launch_bounds__(MF_THREADS)
void mf_template_sums_kernel(int Npixels, const T* __restrict__ templates, MfTemplateSums* __restrict__ sums)
{
    typedef typename MfSum<T>::type Sum;
    __shared__ Sum s1[MF_THREADS], s2[MF_THREADS];
    const T* Tf = templates + (size_t)blockIdx.x*Npixels;
    Sum a1 = 0, a2 = 0;
    for(int i = threadIdx.x; i < Npixels; i += MF_THREADS)
    {
        const T v = Tf[i];
        a1 = a1 + (Sum)v;
        a2 = mf_mad(a2, v, v);
    }
    s1[threadIdx.x] = a1; s2[threadIdx.x] = a2;
    __syncthreads();
    for(int n = MF_THREADS/2; n > 0; n >>= 1)
    {
        if((int)threadIdx.x < n) { s1[threadIdx.x] += s1[threadIdx.x + n]; s2[threadIdx.x] += s2[threadIdx.x + n]; }
        __syncthreads();
    }
    if(threadIdx.x == 0) { sums[blockIdx.x].ST = (double)s1[0]; sums[blockIdx.x].ST2 = (double)s2[0]; }
}

////////////////////////////////////////////////////////////////////////////////
// the optimum and the subpixel fit
////////////////////////////////////////////////////////////////////////////////
struct MfPeak { float v; int i; };      // i < 0: nothing yet
// b takes a's place: it is better, or as good and earlier
__device__ __forceinline__ bool mf_better(const MfPeak& b, const MfPeak& a, int minimize)
{
    if(b.i < 0) return false;
    if(a.i < 0) return true;
    if(minimize ? b.v < a.v : b.v > a.v) return true;
    return b.v == a.v && b.i < a.i;
}

__global__ __launch_bounds__(MF_THREADS)
void mf_peak_kernel(int minimize, const MfFeature* __restrict__ features, const float* __restrict__ surfaces,
                    double* __restrict__ q1, int* __restrict__ status, double* __restrict__ subpixel_at,
                    double* __restrict__ subpixel)
{
    __shared__ MfPeak best[MF_THREADS];
    const int f = blockIdx.x;
    const MfFeature F = features[f];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if(F.status != MATCH_OK)                // (uniform over the workgroup)
    {
        if(threadIdx.x == 0)
        {
            status[f] = F.status;
            q1[2*f] = q1[2*f+1] = subpixel_at[2*f] = subpixel_at[2*f+1] = subpixel[f] = nan;
        }
        return;
    }
    const float* z = surfaces + F.offset;
    const int n = F.out[0]*F.out[1];
    MfPeak mine = { 0.f, -1 };
    for(int i = threadIdx.x; i < n; i += MF_THREADS)
    {
        const MfPeak p = { z[i], i };
        if(mf_better(p, mine, minimize)) mine = p;
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for(int m = MF_THREADS/2; m > 0; m >>= 1)
    {
        if((int)threadIdx.x < m && mf_better(best[threadIdx.x + m], best[threadIdx.x], minimize))
            best[threadIdx.x] = best[threadIdx.x + m];
        __syncthreads();
    }
    if(threadIdx.x != 0) return;

    int    st = MATCH_OK;
    double at[2] = { nan, nan }, value = nan, q[2] = { nan, nan };
    const int w = F.out[0], h = F.out[1];
    const int oy = best[0].i / w, ox = best[0].i - oy*w;
    if(best[0].i < 0 || ox <= 0 || oy <= 0 || ox >= w - 1 || oy >= h - 1) st = MATCH_OPTIMUM_ON_EDGE;
    else
    {
        // The least-squares quadric z ~ c00 + c10 x + c01 y + c20 x^2 + c11 xy + c02 y^2 through the 3 x 3 entries
        // around the optimum, x and y in {-1,0,1}: there the normal equations are diagonal but for the coupling of
        // c00, c20 and c02, and solve in closed form
        double S0 = 0., Sx = 0., Sy = 0., Sxx = 0., Sxy = 0., Syy = 0.;
        for(int j = -1; j <= 1; j++)
            for(int i = -1; i <= 1; i++)
            {
                const double v = (double)z[(size_t)(oy + j)*w + (ox + i)];
                S0 += v; Sx += i*v; Sy += j*v; Sxx += (i*i)*v; Sxy += (i*j)*v; Syy += (j*j)*v;
            }
        const double c10 = Sx/6., c01 = Sy/6., c11 = Sxy/4.;
        const double c20 = Sxx/2. - S0/3., c02 = Syy/2. - S0/3.;
        const double c00 = 5.*S0/9. - Sxx/3. - Syy/3.;
        const double det = 4.*c20*c02 - c11*c11;
        const double x = -(2.*c10*c02 - c01*c11)/det, y = -(2.*c01*c20 - c10*c11)/det;
        const double zfit = c00 + c10*x + c01*y + c20*x*x + c11*x*y + c02*y*y;
        if(det == 0.0 || !isfinite(x) || !isfinite(y) || !isfinite(zfit)) st = MATCH_SUBPIXEL_DEGENERATE;
        else
        {
            at[0] = (double)ox + x; at[1] = (double)oy + y;
            value = zfit;
            q[0] = at[0] + F.qshift[0]; q[1] = at[1] + F.qshift[1];
        }
    }
    status[f] = st;
    q1[2*f] = q[0]; q1[2*f+1] = q[1];
    subpixel_at[2*f] = at[0]; subpixel_at[2*f+1] = at[1];
    subpixel[f] = value;
}

////////////////////////////////////////////////////////////////////////////////
// host
////////////////////////////////////////////////////////////////////////////////
template<class T, int METHOD>
bool launch_correlate_tm(const MfArgs& a, int Ngroups, size_t lds, const void* image1, const void* templates,
                         const MfFeature* features, const MfTemplateSums* sums, float* surfaces)
{
    if constexpr (sizeof(T) == 1)
    {
        if(lds > 64*1024)
            HIP_TRY(hipFuncSetAttribute((const void*)mf_correlate_u8_kernel<METHOD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), return false);
        hipLaunchKernelGGL((mf_correlate_u8_kernel<METHOD>), dim3(Ngroups), dim3(MF_THREADS), lds, NULL,
                           a, (const uint8_t*)image1, (const uint8_t*)templates, features, sums, surfaces);
    }
    else
    {
        if(lds > 64*1024)
            HIP_TRY(hipFuncSetAttribute((const void*)mf_correlate_kernel<T,METHOD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), return false);
        hipLaunchKernelGGL((mf_correlate_kernel<T,METHOD>), dim3(Ngroups), dim3(MF_THREADS), lds, NULL,
                           a, (const T*)image1, (const T*)templates, features, sums, surfaces);
    }
    HIP_TRY(hipGetLastError(), return false);
    return true;
}

template<class T>
bool launch_correlate_t(int method, const MfArgs& a, int Ngroups, size_t lds, const void* image1, const void* templates,
                        const MfFeature* features, const MfTemplateSums* sums, float* surfaces)
{
    switch(method)
    {
#define MF_CASE(M) case M: return launch_correlate_tm<T,M>(a, Ngroups, lds, image1, templates, features, sums, surfaces)
        MF_CASE(MRCAL_AMD_TM_SQDIFF);
        MF_CASE(MRCAL_AMD_TM_SQDIFF_NORMED);
        MF_CASE(MRCAL_AMD_TM_CCORR);
        MF_CASE(MRCAL_AMD_TM_CCORR_NORMED);
        MF_CASE(MRCAL_AMD_TM_CCOEFF);
        MF_CASE(MRCAL_AMD_TM_CCOEFF_NORMED);
#undef MF_CASE
    }
    set_error("match_feature(): method must be one of MRCAL_AMD_TM_* (0..5), not %d", method);
    return false;
}

} // namespace

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_feature_matcher
{
    DeviceBuffers images;                   // the two images: uploaded once
    void*         image[2] = { NULL, NULL };
    int           W[2] = { 0, 0 }, H[2] = { 0, 0 };
    int           dtype = 0;
    // what the last match() left
    DeviceBuffers last;
    MatchPlan     plan;
    int           tw = 0, th = 0;
    float*        surfaces  = NULL;
    void*         templates = NULL;
};

static bool matcher_given(const mrcal_amd_feature_matcher* m)
{
    if(m != NULL) return true;
    set_error("the feature matcher is NULL");
    return false;
}

extern "C" {

mrcal_amd_feature_matcher_t*
mrcal_amd_feature_matcher_create(const void* image0, int width0, int height0,
                                 const void* image1, int width1, int height1, int dtype)
{
    return mrcal_amd_feature_matcher_create_equalized(image0, width0, height0, image1, width1, height1, dtype, NULL);
}

// _create(), both images equalized on the device after the upload (equalize.hip); params NULL or the method NONE: as
// they are
mrcal_amd_feature_matcher_t*
mrcal_amd_feature_matcher_create_equalized(const void* image0, int width0, int height0,
                                           const void* image1, int width1, int height1, int dtype,
                                           const mrcal_amd_equalize_params_t* params)
{
    last_error_string().clear();
    ImagePreparation preparation;
    preparation.equalization = equalize_params_of(params);
    std::string why;
    if(!match_sizes_ok(&why, 0, 1, 1, 0, width0, height0, width1, height1, dtype) ||
       !preparation.ok(&why, width0, height0, 1, dtype) || !preparation.ok(&why, width1, height1, 1, dtype))
    { set_error("%s", why.c_str()); return NULL; }
    if(!have_device()) return NULL;
    mrcal_amd_feature_matcher* m = new mrcal_amd_feature_matcher;
    m->dtype = dtype;
    m->W[0] = width0; m->H[0] = height0; m->W[1] = width1; m->H[1] = height1;
    const void* host[2] = { image0, image1 };
    {
        // the raw images, the histograms and the LUTs go when this scope ends; the prepared images are the matcher's
        DeviceBuffers tmp;
        for(int i = 0; i < 2; i++)
        {
            const void* d = NULL;
            if(!preparation.upload(m->images, tmp, host[i], m->W[i], m->H[i], 1, dtype, &d, &m->dtype))
            { (void)hipDeviceSynchronize(); delete m; return NULL; }
            m->image[i] = (void*)d;
        }
        // (nothing was queued for images that are taken as they are)
        if(!preparation.off()) HIP_TRY(hipStreamSynchronize(NULL), delete m; return NULL);
    }
    return m;
}

bool mrcal_amd_feature_matcher_match(mrcal_amd_feature_matcher_t* m, int N, const double* q1_estimate, const double* H01,
                                     int template_width, int template_height, int search_radius, int method,
                                     double* q1, int* status, double* optimum_subpixel_at, double* optimum_subpixel,
                                     int* qmin, int* output_size)
{
    last_error_string().clear();
    if(!matcher_given(m)) return false;
    if(method < MRCAL_AMD_TM_SQDIFF || method > MRCAL_AMD_TM_CCOEFF_NORMED)
    { set_error("match_feature(): method must be one of MRCAL_AMD_TM_* (0..5), not %d", method); return false; }
    // what the last call left goes first: a call that is refused leaves nothing behind
    m->last.free_all();
    m->surfaces = NULL; m->templates = NULL;
    m->plan = MatchPlan();
    std::string why;
    MatchPlan plan;
    if(!match_plan(&plan, &why, N, q1_estimate, H01, template_width, template_height, search_radius,
                   m->W[0], m->H[0], m->W[1], m->H[1], m->dtype))
    { set_error("%s", why.c_str()); return false; }
    if(N == 0) return true;
    if(!have_device()) return false;

    const int    tw = template_width, th = template_height;
    const size_t Npixels = (size_t)tw*th;
    if(Npixels*(size_t)N > ((size_t)1 << 28))
    { set_error("match_feature(): %d templates of %d x %d pixels are too many for one call", N, tw, th); return false; }

    // the maps of all N templates, one after the other; a feature that is not matched: NaN, which remaps to 0
    std::vector<float>     map(2*Npixels*(size_t)N, nanf(""));
    std::vector<MfFeature> features((size_t)N);
    for(int i = 0; i < N; i++)
    {
        const MatchFeaturePlan& p = plan.features[i];
        if(p.status == MATCH_OK) match_template_map(&map[2*Npixels*(size_t)i], p, H01 + 9*(size_t)i, tw, th);
        MfFeature& F = features[i];
        F.status = p.status;
        for(int k = 0; k < 2; k++) { F.qmin[k] = p.qmin[k]; F.cut[k] = p.cut[k]; F.out[k] = p.out[k]; F.qshift[k] = p.qshift[k]; }
        F.offset = (long long)p.offset;
    }

    float*          d_map = NULL;
    MfFeature*      d_features = NULL;
    MfTemplateSums* d_sums = NULL;
    uint8_t*        d_templates = NULL;
    double *d_q1 = NULL, *d_at = NULL, *d_sub = NULL;
    int*    d_status = NULL;
    DeviceBuffers tmp;
    if(!(tmp.upload(&d_map, map) && tmp.upload(&d_features, features) && tmp.alloc(&d_sums, (size_t)N) &&
         tmp.alloc(&d_q1, (size_t)2*N) && tmp.alloc(&d_at, (size_t)2*N) && tmp.alloc(&d_sub, (size_t)N) && tmp.alloc(&d_status, (size_t)N) &&
         m->last.alloc(&d_templates, Npixels*(size_t)N*image_pixel_bytes(m->dtype)) && m->last.alloc(&m->surfaces, plan.Nsurface)))
    { m->last.free_all(); m->surfaces = NULL; return false; }
    m->templates = d_templates;

    bool ok = remap_device(m->image[0], m->W[0], m->H[0], 1, m->dtype, d_map, d_templates, (int)(Npixels*(size_t)N),
                           MRCAL_AMD_INTER_LINEAR, MRCAL_AMD_BORDER_CONSTANT, NULL);
    MfArgs a;
    a.W1 = m->W[1]; a.tw = tw; a.th = th;
    a.tiles[0] = plan.tiles[0]; a.tiles[1] = plan.tiles[1];
    a.pitch = plan.pitch; a.tpitch = plan.tpitch;
    const int Ngroups = plan.tiles[0]*plan.tiles[1]*N;
    if(ok)
    {
        if(m->dtype == MRCAL_AMD_IMAGE_UINT8)
            hipLaunchKernelGGL(mf_template_sums_kernel<uint8_t>,  dim3(N), dim3(MF_THREADS), 0, NULL, (int)Npixels, (const uint8_t*)d_templates,  d_sums);
        else if(m->dtype == MRCAL_AMD_IMAGE_UINT16)
            hipLaunchKernelGGL(mf_template_sums_kernel<uint16_t>, dim3(N), dim3(MF_THREADS), 0, NULL, (int)Npixels, (const uint16_t*)d_templates, d_sums);
        else
            hipLaunchKernelGGL(mf_template_sums_kernel<float>,    dim3(N), dim3(MF_THREADS), 0, NULL, (int)Npixels, (const float*)d_templates,    d_sums);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    if(ok && Ngroups > 0)       // (no feature is matched: no tile)
    {
        if(m->dtype == MRCAL_AMD_IMAGE_UINT8)
            ok = launch_correlate_t<uint8_t>(method, a, Ngroups, plan.lds_bytes, m->image[1], d_templates, d_features, d_sums, m->surfaces);
        else if(m->dtype == MRCAL_AMD_IMAGE_UINT16)
            ok = launch_correlate_t<uint16_t>(method, a, Ngroups, plan.lds_bytes, m->image[1], d_templates, d_features, d_sums, m->surfaces);
        else
            ok = launch_correlate_t<float>(method, a, Ngroups, plan.lds_bytes, m->image[1], d_templates, d_features, d_sums, m->surfaces);
    }
    if(ok)
    {
        const int minimize = method == MRCAL_AMD_TM_SQDIFF || method == MRCAL_AMD_TM_SQDIFF_NORMED;
        hipLaunchKernelGGL(mf_peak_kernel, dim3(N), dim3(MF_THREADS), 0, NULL, minimize, d_features, m->surfaces, d_q1, d_status, d_at, d_sub);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    // (the copies wait for the launches: the temporaries may go when this returns)
    if(ok) HIP_TRY(hipMemcpy(q1, d_q1, (size_t)2*N*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    if(ok) HIP_TRY(hipMemcpy(status, d_status, (size_t)N*sizeof(int), hipMemcpyDeviceToHost), ok = false);
    if(ok) HIP_TRY(hipMemcpy(optimum_subpixel_at, d_at, (size_t)2*N*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    if(ok) HIP_TRY(hipMemcpy(optimum_subpixel, d_sub, (size_t)N*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    if(!ok)
    {
        (void)hipDeviceSynchronize();
        m->last.free_all(); m->surfaces = NULL; m->templates = NULL;
        return false;
    }
    for(int i = 0; i < N; i++)
        for(int k = 0; k < 2; k++) { qmin[2*i + k] = plan.features[i].qmin[k]; output_size[2*i + k] = plan.features[i].out[k]; }
    m->plan = plan; m->tw = tw; m->th = th;
    return true;
}

static bool matcher_feature_given(const mrcal_amd_feature_matcher* m, int i)
{
    if(!matcher_given(m)) return false;
    if(m->surfaces == NULL || i < 0 || i >= (int)m->plan.features.size())
    {
        set_error("feature %d: the last match() left %d features", i, m->surfaces == NULL ? 0 : (int)m->plan.features.size());
        return false;
    }
    return true;
}

bool mrcal_amd_feature_matcher_matchoutput(mrcal_amd_feature_matcher_t* m, int i, float* matchoutput)
{
    last_error_string().clear();
    if(!matcher_feature_given(m, i)) return false;
    const MatchFeaturePlan& p = m->plan.features[i];
    const size_t n = (size_t)p.out[0]*p.out[1];
    if(n > 0) HIP_TRY(hipMemcpy(matchoutput, m->surfaces + p.offset, n*sizeof(float), hipMemcpyDeviceToHost), return false);
    return true;
}

bool mrcal_amd_feature_matcher_template(mrcal_amd_feature_matcher_t* m, int i, void* template_image)
{
    last_error_string().clear();
    if(!matcher_feature_given(m, i)) return false;
    const size_t n = (size_t)m->tw*m->th*image_pixel_bytes(m->dtype);
    HIP_TRY(hipMemcpy(template_image, (const uint8_t*)m->templates + (size_t)i*n, n, hipMemcpyDeviceToHost), return false);
    return true;
}

void mrcal_amd_feature_matcher_destroy(mrcal_amd_feature_matcher_t* m) { delete m; }

} // extern "C"
