// Stereo rectification and image reprojection: the maps, the remap and the ranges (include/mrcal_amd.h, "stereo
// rectification and image reprojection"). Reference: stereo.c:783-972, 1242-1417; mrcal/image_transforms.py:276-590.
//
//   reproject_map_kernel<PROJ,NDIST> / reproject_map_splined_kernel
//       ONE family for mrcal_rectification_maps() (a launch per camera) and mrcal_amd_image_transformation_map().
//       Per pixel of the TO imager: its observation vector v; p = A (v, or v/|v| d) + t; q = project_from(p), without
//       gradients; the optional valid-region test; two float32. A lane owns 2 consecutive pixels (in memory order:
//       a pair may straddle two rows, which costs an integer division and nothing else) and stores them as 16 B.
//       v of PINHOLE, STEREOGRAPHIC, LONLAT, LATLON comes from the pixel index (a wave-uniform switch; sin and cos
//       in FP64 PER PIXEL: nothing is carried from one pixel to the next, unlike the reference's serial recurrence);
//       any other TO model: v is read from a buffer launch_unproject_points() filled.
//   remap_kernel<T,C,INTERP,BORDER>
//       A lane owns 4 consecutive output pixels (again in memory order, so there is one scalar tail per image and
//       none per row): two 16-B map loads, and the 4 C sizeof(T) bytes of output stored as the widest stores their
//       offset is aligned for (float: 16 B, one or three of them; uint16: 8 B; uint8: 4 B). Exact bilinear weights in
//       float32.
//   stereo_range_dense_kernel / stereo_range_sparse_kernel: a lane an entry.
// No atomics anywhere: the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "problem.hpp"
#include "device_math.hpp"
#include "lens_models.hpp"
#include "lens_dispatch.hpp"
#include "kernels.hpp"
#include "host_state.hpp"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "stereo_geometry.hpp"
#include "remap.hpp"
#include "stereo_sgm.hpp"
#include "speckle_plan.hpp"
#include "equalize.hpp"
#include "smooth.hpp"
#include "image_prepare.hpp"
#include "stereo_range_device.hpp"
#include "point_cloud.hpp"

namespace mrcal_amd {

namespace {

////////////////////////////////////////////////////////////////////////////////
// 1. the maps
////////////////////////////////////////////////////////////////////////////////
struct ReprojectArgs
{
    double A[9], t[3];
    double distance;                        // > 0: p = A v/|v| distance + t
    double to_f_recip[2], to_c_over_f[2];   // the TO model's (1/fx, 1/fy), (cx/fx, cy/fy)
    int    to_type;                         // one of the four models with a formula; < 0: v is read from the buffer
    int    W;                               // of the TO imager
    int    N;                               // its pixels
    int    mask;                            // the valid-region test is made
    int    Nedges;                          // edges of the region's contour that a horizontal ray can cross
};
// an edge of the contour as the crossing-number test wants it: x = x0 + slope (y - y0) for y between y0 and y1. Made on
// the host once, so that the test is two comparisons, a multiply-add and a comparison an edge, without a division
struct RegionEdge { double y0, y1, x0, slope; };
#define MAX_REGION_VERTICES 2048            // 64 kB of LDS

#define REPROJECT_THREADS 256

// PROJECT(q, p): the FROM model
template<class PROJECT>
__device__ __forceinline__
void reproject_pixels(const ReprojectArgs& a, const double* __restrict__ vbuf, const RegionEdge* __restrict__ region,
                      float* __restrict__ map, PROJECT&& project)
{
    extern __shared__ RegionEdge edges[];   // [Nedges]
    if(a.Nedges > 0)                        // (uniform over the launch)
    {
        for(int k=threadIdx.x; k<a.Nedges; k+=blockDim.x) edges[k] = region[k];
        __syncthreads();
    }
    const int i0 = 2*(blockIdx.x*REPROJECT_THREADS + threadIdx.x);
    if(i0 >= a.N) return;
    float out0 = 0.f, out1 = 0.f, out2 = 0.f, out3 = 0.f;
#pragma unroll
    for(int k=0;k<2;k++)
    {
        const int i = i0 + k;
        if(i >= a.N) break;
        double v[3];
        if(a.to_type < 0)
        {
            v[0] = vbuf[3*(size_t)i]; v[1] = vbuf[3*(size_t)i + 1]; v[2] = vbuf[3*(size_t)i + 2];
        }
        else
        {
            const int row = i / a.W, col = i - row*a.W;
            const double ux = (double)col*a.to_f_recip[0] - a.to_c_over_f[0];
            const double uy = (double)row*a.to_f_recip[1] - a.to_c_over_f[1];
            if(a.to_type == MRCAL_LENSMODEL_PINHOLE)            { v[0] = ux; v[1] = uy; v[2] = 1.0; }
            else if(a.to_type == MRCAL_LENSMODEL_STEREOGRAPHIC) { v[0] = ux; v[1] = uy; v[2] = 1.0 - (ux*ux + uy*uy)/4.0; }
            else
            {
                double sx, cx, sy, cy;
                sincos(ux, &sx, &cx);
                sincos(uy, &sy, &cy);
                if(a.to_type == MRCAL_LENSMODEL_LONLAT) { v[0] = cy*sx; v[1] = sy;    v[2] = cy*cx; }   // q = (lon, lat) f + c
                else                                    { v[0] = sx;    v[1] = cx*sy; v[2] = cx*cy; }   // q = (lat, lon) f + c
            }
        }
        if(a.distance > 0.0)
        {
            const double s = a.distance/sqrt(v[0]*v[0] + v[1]*v[1] + v[2]*v[2]);
            v[0] *= s; v[1] *= s; v[2] *= s;
        }
        const double p[3] = { a.A[0]*v[0] + a.A[1]*v[1] + a.A[2]*v[2] + a.t[0],
                              a.A[3]*v[0] + a.A[4]*v[1] + a.A[5]*v[2] + a.t[1],
                              a.A[6]*v[0] + a.A[7]*v[1] + a.A[8]*v[2] + a.t[2] };
        double q[2];
        project(q, p);
        if(a.mask)
        {
            // crossing number: the edges a ray from q towards +x meets. A NaN q meets none: outside
            bool inside = false;
            for(int e=0; e<a.Nedges; e++)
            {
                const RegionEdge E = edges[e];
                if(((E.y0 > q[1]) != (E.y1 > q[1])) && (q[0] < E.slope*(q[1] - E.y0) + E.x0))
                    inside = !inside;
            }
            if(!inside) q[0] = q[1] = -1.0;
        }
        if(k == 0) { out0 = (float)q[0]; out1 = (float)q[1]; }
        else       { out2 = (float)q[0]; out3 = (float)q[1]; }
    }
    // (the map is its own allocation: pixel pair i0/2 sits at a multiple of 16 B)
    if(i0 + 1 < a.N) *(float4*)(map + 2*(size_t)i0) = make_float4(out0, out1, out2, out3);
    else             *(float2*)(map + 2*(size_t)i0) = make_float2(out0, out1);
}

template<int PROJ, int NDIST>
__global__ __launch_bounds__(REPROJECT_THREADS)
void reproject_map_kernel(ReprojectArgs a, LensConfig cfg, const double* __restrict__ intr_in,
                          const double* __restrict__ vbuf, const RegionEdge* __restrict__ region, float* __restrict__ map)
{
    double intr[4 + NDIST];
#pragma unroll
    for(int k=0;k<4+NDIST;k++) intr[k] = intr_in[k];
    reproject_pixels(a, vbuf, region, map, [&](double* q, const double* p)
                     {
                         project_lens<PROJ,NDIST,false>(q, NULL, NULL, p, intr, cfg);
                     });
}
__global__ __launch_bounds__(REPROJECT_THREADS)
void reproject_map_splined_kernel(ReprojectArgs a, LensConfig cfg, const double* __restrict__ intr,
                                  const double* __restrict__ vbuf, const RegionEdge* __restrict__ region, float* __restrict__ map)
{
    reproject_pixels(a, vbuf, region, map, [&](double* q, const double* p)
                     {
                         double dfxy[2], cfx[4], cfy[4]; int ivar0;
                         project_splined<false>(q, NULL, dfxy, &ivar0, cfx, cfy, p, intr, cfg);
                     });
}

// the pixel grid of a W-wide imager, for the TO models that are unprojected iteratively
__global__ __launch_bounds__(256)
void pixel_grid_kernel(int N, int W, double* __restrict__ q)
{
    const int i = blockIdx.x*256 + threadIdx.x;
    if(i >= N) return;
    const int row = i / W;
    q[2*(size_t)i] = (double)(i - row*W); q[2*(size_t)i + 1] = (double)row;
}

bool cahvore_is_central(const mrcal_lensmodel_t* m, const double* intrinsics)
{
    if(m->type != MRCAL_LENSMODEL_CAHVORE) return true;
    for(int i=9;i<12;i++) if(intrinsics[i] != 0.) return false;
    return true;
}

// d_map [N][2] on the device = the map of the TO imager (W x H) into the FROM camera. Returns with the work done
bool reproject_map(float* d_map,
                   const mrcal_lensmodel_t* from, const double* intrinsics_from,
                   const mrcal_lensmodel_t* to,   const double* intrinsics_to, int W, int H,
                   const double* A, const double* t, double distance, const double* region, int Nregion)
{
    if(!lens_supported(from->type) || !lens_supported(to->type))
    {
        set_error("lens model %d is not supported", (int)(lens_supported(from->type) ? to->type : from->type));
        return false;
    }
    if(W <= 0 || H <= 0 || (long)W*(long)H > (1L << 30))
    {
        set_error("an imager of %d x %d pixels cannot be mapped", W, H);
        return false;
    }
    if(region != NULL && (Nregion < 0 || Nregion > MAX_REGION_VERTICES))
    {
        set_error("the valid-intrinsics region has %d vertices; at most %d can be tested", Nregion, MAX_REGION_VERTICES);
        return false;
    }
    ReprojectArgs a;
    memset(&a, 0, sizeof(a));
    for(int i=0;i<9;i++) a.A[i] = A[i];
    for(int i=0;i<3;i++) a.t[i] = t != NULL ? t[i] : 0.0;
    a.distance = distance > 0.0 ? distance : 0.0;
    a.W = W; a.N = W*H;
    a.to_type = -1;

    DeviceBuffers tmp;
    double *d_intr = NULL, *d_v = NULL;
    RegionEdge* d_region = NULL;
    bool ok = tmp.upload(&d_intr, intrinsics_from, (size_t)lensmodel_num_params(*from));
    if(ok && region != NULL)
    {
        // (a region that is valid nowhere has no vertices and no edges: nothing is inside of it)
        a.mask = 1;
        std::vector<RegionEdge> table;
        for(int e=0; e+1<Nregion; e++)
        {
            const double x0 = region[2*e], y0 = region[2*e+1], x1 = region[2*e+2], y1 = region[2*e+3];
            if(y0 != y1) table.push_back(RegionEdge{ y0, y1, x0, (x1 - x0)/(y1 - y0) });      // (a horizontal edge is never crossed)
        }
        a.Nedges = (int)table.size();
        ok = tmp.upload(&d_region, table);
    }
    if(lens_has_closed_form_inverse(to->type))
    {
        a.to_type = (int)to->type;
        a.to_f_recip[0]  = 1./intrinsics_to[0];               a.to_f_recip[1]  = 1./intrinsics_to[1];
        a.to_c_over_f[0] = intrinsics_to[2]*a.to_f_recip[0];  a.to_c_over_f[1] = intrinsics_to[3]*a.to_f_recip[1];
    }
    else
    {
        if(!cahvore_is_central(to, intrinsics_to))
        {
            set_error("unproject() currently only works with a central projection. So I cannot unproject(CAHVORE,E!=0). Please set E=0 to centralize this model");
            return false;
        }
        const int Ni = lensmodel_num_params(*to);
        double *d_q = NULL, *d_intr_to = NULL;
        ok = ok && tmp.alloc(&d_q, (size_t)2*a.N) && tmp.alloc(&d_v, (size_t)3*a.N) && tmp.upload(&d_intr_to, intrinsics_to, (size_t)Ni);
        if(ok)
        {
            hipLaunchKernelGGL(pixel_grid_kernel, dim3((a.N + 255)/256), dim3(256), 0, NULL, a.N, W, d_q);
            HIP_TRY(launch_unproject_points((int)to->type, lens_config_of(*to), a.N, Ni, d_q, d_intr_to, d_v, NULL, NULL,
                                            NULL, NULL, NULL, false, NULL), ok = false);
        }
    }
    if(!ok) return false;

    const LensConfig cfg = lens_config_of(*from);
    const dim3 grid(((a.N + 1)/2 + REPROJECT_THREADS - 1)/REPROJECT_THREADS), block(REPROJECT_THREADS);
    const size_t lds = (size_t)a.Nedges*sizeof(RegionEdge);
    if(!for_parametric_lens(from->type, [&](auto k)
       {
           using K = decltype(k);
           hipLaunchKernelGGL((reproject_map_kernel<K::PROJ,K::NDIST>), grid, block, lds, NULL, a, cfg, d_intr, d_v, d_region, d_map);
       }))
        hipLaunchKernelGGL(reproject_map_splined_kernel, grid, block, lds, NULL, a, cfg, d_intr, d_v, d_region, d_map);
    HIP_TRY(hipGetLastError(), return false);
    // (the temporaries go when this returns)
    HIP_TRY(hipStreamSynchronize(NULL), return false);
    return true;
}

bool rectification_model_ok(mrcal_lensmodel_type_t t, const char* who)
{
    if(t == MRCAL_LENSMODEL_LATLON || t == MRCAL_LENSMODEL_PINHOLE) return true;
    set_error("%s() supports MRCAL_LENSMODEL_LATLON and MRCAL_LENSMODEL_PINHOLE only", who);
    return false;
}

// R_cam_rect = R_cam_ref R_rect0_ref^T
void R_cam_rect_of(double* R_cam_rect, const double* r_cam_ref, const double* r_rect0_ref)
{
    double Rc[9], Rr[9];
    R_from_r_host(Rc, r_cam_ref);
    R_from_r_host(Rr, r_rect0_ref);
    for(int i=0;i<3;i++) for(int j=0;j<3;j++)
        R_cam_rect[3*i+j] = Rc[3*i]*Rr[3*j] + Rc[3*i+1]*Rr[3*j+1] + Rc[3*i+2]*Rr[3*j+2];
}

////////////////////////////////////////////////////////////////////////////////
// 2. the remap
////////////////////////////////////////////////////////////////////////////////
template<class T> __device__ __forceinline__ T pixel_from_float(float v);
template<> __device__ __forceinline__ float    pixel_from_float<float>(float v)    { return v; }
// round to nearest, saturate (a NaN: 0)
template<> __device__ __forceinline__ uint8_t  pixel_from_float<uint8_t>(float v)  { return (uint8_t) fminf(fmaxf(rintf(v), 0.f), 255.f); }
template<> __device__ __forceinline__ uint16_t pixel_from_float<uint16_t>(float v) { return (uint16_t)fminf(fmaxf(rintf(v), 0.f), 65535.f); }

template<int NW> __device__ __forceinline__ void store_words(void* dst, const uint32_t* w)
{
    if constexpr (NW % 4 == 0)
    {
#pragma unroll
        for(int k=0;k<NW/4;k++) ((uint4*)dst)[k] = make_uint4(w[4*k], w[4*k+1], w[4*k+2], w[4*k+3]);
    }
    else if constexpr (NW % 2 == 0)
    {
#pragma unroll
        for(int k=0;k<NW/2;k++) ((uint2*)dst)[k] = make_uint2(w[2*k], w[2*k+1]);
    }
    else
    {
#pragma unroll
        for(int k=0;k<NW;k++) ((uint32_t*)dst)[k] = w[k];
    }
}

struct BorderValue { float v[3]; };

#define REMAP_THREADS 256
template<class T, int C, int INTERP, int BORDER>
__global__ __launch_bounds__(REMAP_THREADS)
void remap_kernel(const T* __restrict__ src, int W, int H, const float* __restrict__ map, T* __restrict__ out, int Nout,
                  BorderValue border)
{
    const int i0 = 4*(blockIdx.x*REMAP_THREADS + threadIdx.x);
    if(i0 >= Nout) return;
    const bool full = i0 + 4 <= Nout;
    float m[8];
    if(full)
    {
        const float4 m0 = *(const float4*)(map + 2*(size_t)i0), m1 = *(const float4*)(map + 2*(size_t)i0 + 4);
        m[0] = m0.x; m[1] = m0.y; m[2] = m0.z; m[3] = m0.w; m[4] = m1.x; m[5] = m1.y; m[6] = m1.z; m[7] = m1.w;
    }
    else
    {
#pragma unroll
        for(int k=0;k<4;k++)
        {
            const bool have = i0 + k < Nout;
            m[2*k]   = have ? map[2*(size_t)(i0 + k)]     : 0.f;
            m[2*k+1] = have ? map[2*(size_t)(i0 + k) + 1] : 0.f;
        }
    }

    union { T o[4*C]; uint32_t w[C*sizeof(T)]; } px;
    bool write[4];
#pragma unroll
    for(int k=0;k<4;k++)
    {
        const float x = m[2*k], y = m[2*k+1];
        write[k] = true;
        // some neighbour can be inside (a NaN or an infinity: none; and the integer conversions below are safe)
        const bool reach = x > -1.f && x < (float)W && y > -1.f && y < (float)H;
        if(INTERP == MRCAL_AMD_INTER_NEAREST)
        {
            const int ix = reach ? (int)rintf(x) : -1, iy = reach ? (int)rintf(y) : -1;
            const bool in = ix >= 0 && ix < W && iy >= 0 && iy < H;
            if(BORDER == MRCAL_AMD_BORDER_TRANSPARENT && !in) write[k] = false;
#pragma unroll
            for(int c=0;c<C;c++)
                px.o[k*C + c] = in ? src[((size_t)iy*W + ix)*C + c] : pixel_from_float<T>(border.v[c]);
        }
        else
        {
            const float x0 = floorf(x), y0 = floorf(y);
            const int   ix = reach ? (int)x0 : -1, iy = reach ? (int)y0 : -1;
            const float fx = x - x0, fy = y - y0;
            const bool  xin0 = reach && ix >= 0, xin1 = reach && ix + 1 < W, yin0 = reach && iy >= 0, yin1 = reach && iy + 1 < H;
            if(BORDER == MRCAL_AMD_BORDER_TRANSPARENT && !(xin0 && xin1 && yin0 && yin1)) write[k] = false;
            const size_t at = ((size_t)(iy > 0 ? iy : 0)*W + (ix > 0 ? ix : 0))*C;
#pragma unroll
            for(int c=0;c<C;c++)
            {
                const float b   = border.v[c];
                const float v00 = xin0 && yin0 ? (float)src[at + c]                                               : b;
                const float v01 = xin1 && yin0 ? (float)src[((size_t)(iy > 0 ? iy : 0)*W + (ix + 1))*C + c]        : b;
                const float v10 = xin0 && yin1 ? (float)src[((size_t)(iy + 1)*W + (ix > 0 ? ix : 0))*C + c]        : b;
                const float v11 = xin1 && yin1 ? (float)src[((size_t)(iy + 1)*W + (ix + 1))*C + c]                 : b;
                // on a pixel: that pixel, to the bit
                const float v = (fx == 0.f && fy == 0.f) ? v00
                              : (1.f - fy)*((1.f - fx)*v00 + fx*v01) + fy*((1.f - fx)*v10 + fx*v11);
                px.o[k*C + c] = reach ? pixel_from_float<T>(v) : pixel_from_float<T>(b);
            }
        }
    }
    if(full && write[0] && write[1] && write[2] && write[3])
        store_words<C*(int)sizeof(T)>(out + (size_t)i0*C, px.w);
    else
    {
#pragma unroll
        for(int k=0;k<4;k++)
            if(i0 + k < Nout && write[k])
            {
#pragma unroll
                for(int c=0;c<C;c++) out[(size_t)(i0 + k)*C + c] = px.o[k*C + c];
            }
    }
}

template<class T, int C>
void launch_remap_tc(const void* src, int W, int H, const float* map, void* out, int Nout, int interp, int border_mode,
                     const BorderValue& bv)
{
    const dim3 grid(((Nout + 3)/4 + REMAP_THREADS - 1)/REMAP_THREADS), block(REMAP_THREADS);
#define REMAP_LAUNCH(I, B) hipLaunchKernelGGL((remap_kernel<T,C,I,B>), grid, block, 0, NULL, (const T*)src, W, H, map, (T*)out, Nout, bv)
    if(interp == MRCAL_AMD_INTER_NEAREST)
    {
        if(border_mode == MRCAL_AMD_BORDER_CONSTANT) REMAP_LAUNCH(MRCAL_AMD_INTER_NEAREST, MRCAL_AMD_BORDER_CONSTANT);
        else                                         REMAP_LAUNCH(MRCAL_AMD_INTER_NEAREST, MRCAL_AMD_BORDER_TRANSPARENT);
    }
    else
    {
        if(border_mode == MRCAL_AMD_BORDER_CONSTANT) REMAP_LAUNCH(MRCAL_AMD_INTER_LINEAR, MRCAL_AMD_BORDER_CONSTANT);
        else                                         REMAP_LAUNCH(MRCAL_AMD_INTER_LINEAR, MRCAL_AMD_BORDER_TRANSPARENT);
    }
#undef REMAP_LAUNCH
}

bool remap_arguments_ok(int width, int height, int channels, int dtype, int width_out, int height_out,
                        int interpolation, int border_mode)
{
    if(!(dtype == MRCAL_AMD_IMAGE_UINT8 || dtype == MRCAL_AMD_IMAGE_UINT16 || dtype == MRCAL_AMD_IMAGE_FLOAT))
    { set_error("transform_image(): images are uint8, uint16 or float32"); return false; }
    if(!(channels == 1 || channels == 3))
    { set_error("transform_image(): an image has 1 or 3 channels, not %d", channels); return false; }
    if(!(interpolation == MRCAL_AMD_INTER_NEAREST || interpolation == MRCAL_AMD_INTER_LINEAR))
    { set_error("transform_image(): interpolation is 'nearest' (0) or 'linear' (1), not %d", interpolation); return false; }
    if(!(border_mode == MRCAL_AMD_BORDER_CONSTANT || border_mode == MRCAL_AMD_BORDER_TRANSPARENT))
    { set_error("transform_image(): borderMode is 'constant' (0) or 'transparent' (5), not %d", border_mode); return false; }
    if(width <= 0 || height <= 0 || width_out <= 0 || height_out <= 0 ||
       (long)width*height > (1L << 30) || (long)width_out*height_out > (1L << 28))
    { set_error("transform_image(): images of %d x %d -> %d x %d pixels cannot be transformed", width, height, width_out, height_out); return false; }
    return true;
}

} // namespace
// device arrays; the arguments have been checked (remap.hpp: match_feature.hip makes its templates with it)
bool remap_device(const void* d_src, int W, int H, int C, int dtype, const float* d_map, void* d_out, int Nout,
                  int interp, int border_mode, const double* border_value)
{
    BorderValue bv;
    for(int c=0;c<3;c++) bv.v[c] = (border_value != NULL && c < C) ? (float)border_value[c] : 0.f;
    if(dtype == MRCAL_AMD_IMAGE_UINT8)
    {
        if(C == 1) launch_remap_tc<uint8_t,1>(d_src, W, H, d_map, d_out, Nout, interp, border_mode, bv);
        else       launch_remap_tc<uint8_t,3>(d_src, W, H, d_map, d_out, Nout, interp, border_mode, bv);
    }
    else if(dtype == MRCAL_AMD_IMAGE_UINT16)
    {
        if(C == 1) launch_remap_tc<uint16_t,1>(d_src, W, H, d_map, d_out, Nout, interp, border_mode, bv);
        else       launch_remap_tc<uint16_t,3>(d_src, W, H, d_map, d_out, Nout, interp, border_mode, bv);
    }
    else
    {
        if(C == 1) launch_remap_tc<float,1>(d_src, W, H, d_map, d_out, Nout, interp, border_mode, bv);
        else       launch_remap_tc<float,3>(d_src, W, H, d_map, d_out, Nout, interp, border_mode, bv);
    }
    HIP_TRY(hipGetLastError(), return false);
    return true;
}

static_assert(IMAGE_DTYPE_UINT8 == MRCAL_AMD_IMAGE_UINT8 && IMAGE_DTYPE_UINT16 == MRCAL_AMD_IMAGE_UINT16 &&
              IMAGE_DTYPE_FLOAT == MRCAL_AMD_IMAGE_FLOAT, "image_format.hpp restates the header's image types");

// (image_prepare.hpp: match_feature.hip prepares its two images with it too)
bool ImagePreparation::upload(DeviceBuffers& result, DeviceBuffers& workspace, const void* host_image, int W, int H, int C, int dtype,
                              const void** d_image, int* dtype_image, const void** d_unfiltered) const
{
    const bool filtered = !smooth_is_off(antialias);
    uint8_t* d_raw = NULL;
    const void* d_equalized = NULL;
    if(!((off() ? result : workspace).upload(&d_raw, (const uint8_t*)host_image, (size_t)W*H*C*image_pixel_bytes(dtype)) &&
         equalize_resident(filtered ? workspace : result, workspace, equalization, d_raw, W, H, dtype, &d_equalized, dtype_image)))
        return false;
    if(d_unfiltered != NULL) *d_unfiltered = d_equalized;
    return smooth_resident(result, antialias, d_equalized, W, H, *dtype_image, d_image);
}
namespace {

// a pair of raw images of one type that the remap and the preparation take: false, and why
bool pair_arguments_ok(const ImagePreparation& preparation, int width0, int height0, int width1, int height1, int channels, int dtype,
                       int width_out, int height_out, int interpolation, int border_mode)
{
    if(!remap_arguments_ok(width0, height0, channels, dtype, width_out, height_out, interpolation, border_mode) ||
       !remap_arguments_ok(width1, height1, channels, dtype, width_out, height_out, interpolation, border_mode))
        return false;
    std::string why;
    if(preparation.ok(&why, width0, height0, channels, dtype) && preparation.ok(&why, width1, height1, channels, dtype)) return true;
    set_error("%s", why.c_str());
    return false;
}

// host image -> remapped host image through a map that is on the device already. preparation: of the image, on the
// device, before the remap; out is then of the prepared type
bool remap_host_image(void* out, const void* image, int W, int H, int C, int dtype, const float* d_map, int Nout,
                      int interp, int border_mode, const double* border_value, const ImagePreparation& preparation)
{
    DeviceBuffers tmp;
    const void* d_image = NULL; uint8_t* d_out = NULL;
    int dtype_image = dtype;
    if(!preparation.upload(tmp, tmp, image, W, H, C, dtype, &d_image, &dtype_image)) return false;
    const size_t nout = (size_t)Nout*C*image_pixel_bytes(dtype_image);
    // a transparent border keeps what out had
    if(!(border_mode == MRCAL_AMD_BORDER_TRANSPARENT ? tmp.upload(&d_out, (const uint8_t*)out, nout) : tmp.alloc(&d_out, nout)))
        return false;
    if(!remap_device(d_image, W, H, C, dtype_image, d_map, d_out, Nout, interp, border_mode, border_value)) return false;
    // (the temporaries go when this returns: after a copy that failed, not before the launches have)
    HIP_TRY(hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost), (void)hipDeviceSynchronize(); return false);
    return true;
}

////////////////////////////////////////////////////////////////////////////////
// 3. the ranges (stereo.c:1263-1417; the derivation: the docstring of mrcal.stereo_range())
////////////////////////////////////////////////////////////////////////////////
// RangeArgs, stereo_range_one() and stereo_unit_vector(): stereo_range_device.hpp, shared with point_cloud.hip

__global__ __launch_bounds__(256)
void stereo_range_dense_kernel(RangeArgs a, int N, int W, const uint16_t* __restrict__ disparity_scaled,
                               double disparity_scale, int dmin, int dmax, double* __restrict__ range)
{
    const int i = blockIdx.x*256 + threadIdx.x;
    if(i >= N) return;
    const int d = disparity_scaled[i];
    const int row = i / W;
    range[i] = (d <= 0 || d < dmin || d > dmax) ? 0.0
             : stereo_range_one((double)d/disparity_scale, (double)(i - row*W), (double)row, a);
}

// p (N,3) may be NULL, and so may range
__global__ __launch_bounds__(256)
void stereo_range_sparse_kernel(RangeArgs a, int N, const double* __restrict__ disparity, const double* __restrict__ qrect0,
                                double dmin, double dmax, double* __restrict__ range, double* __restrict__ p)
{
    const int i = blockIdx.x*256 + threadIdx.x;
    if(i >= N) return;
    const double d = disparity[i], qx = qrect0[2*(size_t)i], qy = qrect0[2*(size_t)i + 1];
    // (a NaN disparity passes the three tests, as in the reference, and gives a range that is not finite: 0)
    const double r = (d <= 0.0 || d < dmin || d > dmax) ? 0.0 : stereo_range_one(d, qx, qy, a);
    if(range != NULL) range[i] = r;
    if(p != NULL)
    {
        double v[3];
        stereo_unit_vector(v, qx, qy, a);
        for(int k=0;k<3;k++) p[3*(size_t)i + k] = r*v[k];
    }
}

bool range_arguments(RangeArgs* a, mrcal_lensmodel_type_t t, const double* fxycxy, double baseline)
{
    if(!(t == MRCAL_LENSMODEL_LATLON || t == MRCAL_LENSMODEL_PINHOLE))
    {
        set_error("Invalid rectification_model_type for rectification: %d; I know about MRCAL_LENSMODEL_LATLON and MRCAL_LENSMODEL_PINHOLE", (int)t);
        return false;
    }
    a->fx = fxycxy[0]; a->fy = fxycxy[1]; a->cx = fxycxy[2]; a->cy = fxycxy[3];
    a->baseline = baseline;
    a->latlon   = t == MRCAL_LENSMODEL_LATLON;
    return true;
}

// dense (H,W) uint16 host array -> (H,W) double host array
bool range_dense(double* range, const uint16_t* disparity_scaled, int W, int H, const RangeArgs& a,
                 uint16_t disparity_scale, uint16_t dmin, uint16_t dmax)
{
    if(dmin >= dmax) { set_error("Must have disparity_scaled_max > disparity_scaled_min"); return false; }
    if(W <= 0 || H <= 0 || (long)W*H > (1L << 28)) { set_error("a disparity image of %d x %d pixels cannot be ranged", W, H); return false; }
    const int N = W*H;
    DeviceBuffers tmp;
    uint16_t* d_d = NULL; double* d_r = NULL;
    if(!(tmp.upload(&d_d, disparity_scaled, (size_t)N) && tmp.alloc(&d_r, (size_t)N))) return false;
    hipLaunchKernelGGL(stereo_range_dense_kernel, dim3((N + 255)/256), dim3(256), 0, NULL,
                       a, N, W, d_d, (double)disparity_scale, (int)dmin, (int)dmax, d_r);
    HIP_TRY(hipGetLastError(), return false);
    HIP_TRY(hipMemcpy(range, d_r, (size_t)N*sizeof(double), hipMemcpyDeviceToHost), return false);
    return true;
}

} // namespace

} // namespace mrcal_amd

using namespace mrcal_amd;

struct mrcal_amd_rectification
{
    DeviceBuffers mem;
    float*        map[2] = { NULL, NULL };     // each its own allocation: [Nel][Naz][2]
    int           W = 0, H = 0;
    RangeArgs     range_args;
    // point_cloud.hip's object, made by the first cloud: it reads map[0] where it lies
    mrcal_amd_point_cloud_t* cloud = NULL;
    mrcal_lensmodel_type_t   rectification_model_type = MRCAL_LENSMODEL_LATLON;
    double                   fxycxy[4] = { 0., 0., 0., 0. };
    // of every raw image, between its upload and the remap: _set_equalization() and _set_antialias() fill its halves
    ImagePreparation         preparation;
    ~mrcal_amd_rectification() { mrcal_amd_point_cloud_destroy(cloud); }
};

static mrcal_amd_point_cloud_t* rectification_cloud(mrcal_amd_rectification* r)
{
    if(r->cloud == NULL)
        r->cloud = mrcal_amd_point_cloud_create(r->rectification_model_type, r->fxycxy, r->range_args.baseline, r->W, r->H, r->map[0]);
    return r->cloud;
}

static bool rectification_given(const mrcal_amd_rectification* r)
{
    if(r != NULL) return true;
    set_error("the rectification is NULL");
    return false;
}

extern "C" {

bool mrcal_amd_image_transformation_map(float* mapxy,
                                        const mrcal_lensmodel_t* lensmodel_from, const double* intrinsics_from,
                                        const mrcal_lensmodel_t* lensmodel_to,   const double* intrinsics_to,
                                        const unsigned int* imagersize_to,
                                        const double* A, const double* t, double distance,
                                        const double* region, int Nregion)
{
    last_error_string().clear();
    if(!have_device()) return false;
    const int W = (int)imagersize_to[0], H = (int)imagersize_to[1];
    if(W <= 0 || H <= 0 || (long)W*(long)H > (1L << 30)) { set_error("an imager of %d x %d pixels cannot be mapped", W, H); return false; }
    DeviceBuffers tmp;
    float* d_map = NULL;
    if(!tmp.alloc(&d_map, (size_t)2*W*H)) return false;
    if(!reproject_map(d_map, lensmodel_from, intrinsics_from, lensmodel_to, intrinsics_to, W, H, A, t, distance, region, Nregion))
        return false;
    HIP_TRY(hipMemcpy(mapxy, d_map, (size_t)2*W*H*sizeof(float), hipMemcpyDeviceToHost), return false);
    return true;
}

mrcal_amd_rectification_t*
mrcal_amd_rectification_create(const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0, const double* r_cam0_ref,
                               const mrcal_lensmodel_t* lensmodel1, const double* intrinsics1, const double* r_cam1_ref,
                               const mrcal_lensmodel_type_t rectification_model_type,
                               const double* fxycxy_rectified, const unsigned int* imagersize_rectified,
                               const double* r_rect0_ref, double baseline)
{
    last_error_string().clear();
    if(!rectification_model_ok(rectification_model_type, "mrcal_rectification_maps")) return NULL;
    if(!have_device()) return NULL;
    const int W = (int)imagersize_rectified[0], H = (int)imagersize_rectified[1];
    if(W <= 0 || H <= 0 || (long)W*(long)H > (1L << 30)) { set_error("a rectified imager of %d x %d pixels cannot be mapped", W, H); return NULL; }

    mrcal_amd_rectification* r = new mrcal_amd_rectification;
    r->W = W; r->H = H;
    range_arguments(&r->range_args, rectification_model_type, fxycxy_rectified, baseline);
    r->rectification_model_type = rectification_model_type;
    for(int i=0;i<4;i++) r->fxycxy[i] = fxycxy_rectified[i];
    mrcal_lensmodel_t rectified; memset(&rectified, 0, sizeof(rectified));
    rectified.type = rectification_model_type;
    const mrcal_lensmodel_t* lensmodels[2] = { lensmodel0, lensmodel1 };
    const double* intrinsics[2] = { intrinsics0, intrinsics1 };
    const double* r_cam_ref[2]  = { r_cam0_ref,  r_cam1_ref  };
    for(int icam=0; icam<2; icam++)
    {
        double R_cam_rect[9];
        R_cam_rect_of(R_cam_rect, r_cam_ref[icam], r_rect0_ref);
        if(!(r->mem.alloc(&r->map[icam], (size_t)2*W*H) &&
             reproject_map(r->map[icam], lensmodels[icam], intrinsics[icam], &rectified, fxycxy_rectified, W, H,
                           R_cam_rect, NULL, 0.0, NULL, 0)))
        {
            delete r;
            return NULL;
        }
    }
    return r;
}

bool mrcal_amd_rectification_maps(mrcal_amd_rectification_t* r, float* rectification_maps)
{
    last_error_string().clear();
    if(!rectification_given(r)) return false;
    const size_t n = (size_t)2*r->W*r->H;
    for(int icam=0; icam<2; icam++)
        HIP_TRY(hipMemcpy(rectification_maps + icam*n, r->map[icam], n*sizeof(float), hipMemcpyDeviceToHost), return false);
    return true;
}

bool mrcal_amd_rectification_rectify(mrcal_amd_rectification_t* r, void* out0, void* out1,
                                     const void* image0, int width0, int height0,
                                     const void* image1, int width1, int height1, int channels, int dtype,
                                     int interpolation, int border_mode, const double* border_value)
{
    last_error_string().clear();
    if(!rectification_given(r) || !have_device()) return false;
    if(!pair_arguments_ok(r->preparation, width0, height0, width1, height1, channels, dtype, r->W, r->H, interpolation, border_mode))
        return false;
    return remap_host_image(out0, image0, width0, height0, channels, dtype, r->map[0], r->W*r->H, interpolation, border_mode, border_value, r->preparation)
        && remap_host_image(out1, image1, width1, height1, channels, dtype, r->map[1], r->W*r->H, interpolation, border_mode, border_value, r->preparation);
}

bool mrcal_amd_rectification_set_equalization(mrcal_amd_rectification_t* r, const mrcal_amd_equalize_params_t* params)
{
    last_error_string().clear();
    if(!rectification_given(r)) return false;
    if(params == NULL) { set_error("equalize(): the parameters are NULL"); return false; }
    const EqualizeParams p = equalize_params_of(params);
    // (what can be refused without an image; the rest when one comes)
    std::string why;
    if(!equalize_params_ok(&why, p.tiles_x > 0 ? p.tiles_x : 1, p.tiles_y > 0 ? p.tiles_y : 1, MRCAL_AMD_IMAGE_UINT8, p))
    { set_error("%s", why.c_str()); return false; }
    r->preparation.equalization = p;
    return true;
}

bool mrcal_amd_rectification_set_antialias(mrcal_amd_rectification_t* r, const mrcal_amd_smooth_params_t* params)
{
    last_error_string().clear();
    if(!rectification_given(r)) return false;
    const SmoothParams p = smooth_params_of(params);
    // (what can be refused without an image; the rest when one comes)
    std::string why;
    if(!smooth_is_off(p) && !smooth_params_ok(&why, 1, 1, MRCAL_AMD_IMAGE_UINT8, p)) { set_error("%s", why.c_str()); return false; }
    r->preparation.antialias = p;
    return true;
}

bool mrcal_amd_rectification_range(mrcal_amd_rectification_t* r, double* range, const uint16_t* disparity_scaled,
                                   uint16_t disparity_scale, uint16_t disparity_scaled_min, uint16_t disparity_scaled_max)
{
    last_error_string().clear();
    if(!rectification_given(r) || !have_device()) return false;
    return range_dense(range, disparity_scaled, r->W, r->H, r->range_args, disparity_scale, disparity_scaled_min, disparity_scaled_max);
}

// What _disparity_filtered() and _point_cloud_of_images() do alike: the refusals before any device work (the matcher
// says the same of the speckle pair again), a new matcher (stereo_sgm.hip) with its speckle filter set (a window of 0:
// no filter, and nothing of it runs), and both images prepared and rectified straight into its device buffers. The raw
// and the prepared images are tmp's, which may go once the NULL stream has run dry. If they are wanted: *cloud, the
// rectification's point-cloud object, made before the matcher; *d_unfiltered0, of *dtype_unfiltered0, image0 as it was
// before the anti-aliasing filter. NULL: a refusal or a failure, and nothing is left running
static mrcal_amd_stereo_sgm_t* rectified_pair_matcher(mrcal_amd_rectification* r, DeviceBuffers& tmp,
                                                      const void* image0, int width0, int height0,
                                                      const void* image1, int width1, int height1, int dtype,
                                                      const mrcal_amd_stereo_sgm_params_t* params,
                                                      int speckle_window_size, int speckle_range, mrcal_amd_point_cloud_t** cloud = NULL,
                                                      const void** d_unfiltered0 = NULL, int* dtype_unfiltered0 = NULL)
{
    SpeckleParams p; std::string why;
    if(!speckle_params_of_matcher(&p, &why, 0, 1, speckle_window_size, speckle_range)) { set_error("%s", why.c_str()); return NULL; }
    if(!rectification_given(r) || !have_device()) return NULL;
    if(!pair_arguments_ok(r->preparation, width0, height0, width1, height1, 1, dtype, r->W, r->H,
                          MRCAL_AMD_INTER_LINEAR, MRCAL_AMD_BORDER_CONSTANT))
        return NULL;
    if(cloud != NULL && (*cloud = rectification_cloud(r)) == NULL) return NULL;
    mrcal_amd_stereo_sgm_t* m = mrcal_amd_stereo_sgm_create(r->W, r->H, r->preparation.dtype_out(dtype), params);
    if(m == NULL) return NULL;
    // (destroy clears nothing: the error of a failure stays)
    if(!mrcal_amd_stereo_sgm_set_speckle_filter(m, speckle_window_size, speckle_range)) { mrcal_amd_stereo_sgm_destroy(m); return NULL; }
    const void* image[2] = { image0, image1 };
    const int   W[2] = { width0, width1 }, H[2] = { height0, height1 };
    for(int i = 0; i < 2; i++)
    {
        const void *d_src = NULL, *d_unfiltered = NULL; int dtype_src = dtype;
        if(!(r->preparation.upload(tmp, tmp, image[i], W[i], H[i], 1, dtype, &d_src, &dtype_src, &d_unfiltered) &&
             remap_device(d_src, W[i], H[i], 1, dtype_src, r->map[i], sgm_device_image(m, i), r->W*r->H,
                          MRCAL_AMD_INTER_LINEAR, MRCAL_AMD_BORDER_CONSTANT, NULL)))
        {
            (void)hipDeviceSynchronize();
            mrcal_amd_stereo_sgm_destroy(m);
            return NULL;
        }
        if(i == 0 && d_unfiltered0 != NULL) { *d_unfiltered0 = d_unfiltered; *dtype_unfiltered0 = dtype_src; }
    }
    return m;
}

// image pair -> disparity: both images rectified straight into the matcher's device buffers (stereo_sgm.hip)
bool mrcal_amd_rectification_disparity(mrcal_amd_rectification_t* r,
                                       const void* image0, int width0, int height0,
                                       const void* image1, int width1, int height1, int dtype,
                                       const mrcal_amd_stereo_sgm_params_t* params, int16_t* disparity)
{
    return mrcal_amd_rectification_disparity_filtered(r, image0, width0, height0, image1, width1, height1, dtype, params, 0, 0, disparity);
}

bool mrcal_amd_rectification_disparity_filtered(mrcal_amd_rectification_t* r,
                                                const void* image0, int width0, int height0,
                                                const void* image1, int width1, int height1, int dtype,
                                                const mrcal_amd_stereo_sgm_params_t* params,
                                                int speckle_window_size, int speckle_range, int16_t* disparity)
{
    last_error_string().clear();
    DeviceBuffers tmp;
    mrcal_amd_stereo_sgm_t* m = rectified_pair_matcher(r, tmp, image0, width0, height0, image1, width1, height1, dtype, params,
                                                       speckle_window_size, speckle_range);
    if(m == NULL) return false;
    // (its copy waits for the launches: the images and the matcher may go when this returns)
    const bool ok = sgm_match_device(m, disparity);
    if(!ok) (void)hipDeviceSynchronize();
    mrcal_amd_stereo_sgm_destroy(m);
    return ok;
}

// ---- the point cloud (point_cloud.hip) through the rectification's map of camera 0
bool mrcal_amd_rectification_point_cloud(mrcal_amd_rectification_t* r, const uint16_t* disparity_scaled,
                                         const mrcal_amd_point_cloud_params_t* params, int* N)
{
    last_error_string().clear();
    if(!rectification_given(r) || !have_device()) return false;
    mrcal_amd_point_cloud_t* c = rectification_cloud(r);
    return c != NULL && mrcal_amd_point_cloud_compute(c, disparity_scaled, params, N);
}

// image pair -> cloud: rectified into the matcher's buffers, matched (and filtered) there, and the cloud made of the
// disparities where the matcher left them
bool mrcal_amd_rectification_point_cloud_of_images(mrcal_amd_rectification_t* r,
                                                   const void* image0, int width0, int height0,
                                                   const void* image1, int width1, int height1, int dtype,
                                                   const mrcal_amd_stereo_sgm_params_t* sgm_params,
                                                   int speckle_window_size, int speckle_range,
                                                   const mrcal_amd_point_cloud_params_t* params, int* N)
{
    last_error_string().clear();
    if(sgm_params == NULL || params == NULL || N == NULL) { set_error("stereo_point_cloud(): an argument is NULL"); return false; }
    if(sgm_params->disparity_min < 0)
    {
        set_error("stereo_point_cloud(): disparity_min must not be negative: the cast to uint16 of stereo_range() has no meaning for negative disparities. Got %d",
                  sgm_params->disparity_min);
        return false;
    }
    DeviceBuffers tmp;
    mrcal_amd_point_cloud_t* c = NULL;
    const void* d_unfiltered0 = NULL; int dtype_unfiltered0 = dtype;
    mrcal_amd_stereo_sgm_t* m = rectified_pair_matcher(r, tmp, image0, width0, height0, image1, width1, height1, dtype, sgm_params,
                                                       speckle_window_size, speckle_range, &c, &d_unfiltered0, &dtype_unfiltered0);
    if(m == NULL) return false;
    // the disparities are the matcher's: its scale, and everything from its smallest disparity up is valid
    mrcal_amd_point_cloud_params_t p = *params;
    p.disparity_scale      = 16;
    p.disparity_scaled_min = (uint16_t)(16*sgm_params->disparity_min);
    p.disparity_scaled_max = 0x7FFF;
    // colours from image0 itself: from the equalized one, where it lies, as it was before the anti-aliasing filter
    const void* d_color = NULL;
    if(r->preparation.equalization.method != EQUALIZE_METHOD_NONE && p.image != NULL && p.image == image0 &&
       p.image_width == width0 && p.image_height == height0 && p.image_channels == 1 && p.image_dtype == dtype)
    { d_color = d_unfiltered0; p.image_dtype = dtype_unfiltered0; }
    const int16_t* d_disparity = NULL;
    // (the cloud waits for its launches, and so for these: the images and the matcher may go when this returns)
    const bool ok = sgm_match_device_resident(m, &d_disparity) && point_cloud_compute_device(c, (const uint16_t*)d_disparity, &p, N, d_color);
    if(!ok) (void)hipDeviceSynchronize();
    mrcal_amd_stereo_sgm_destroy(m);
    return ok;
}

bool mrcal_amd_rectification_point_cloud_read(mrcal_amd_rectification_t* r, void* points, void* color, int32_t* index)
{
    last_error_string().clear();
    if(!rectification_given(r)) return false;
    if(r->cloud == NULL) { set_error("stereo_point_cloud(): no cloud has been computed yet"); return false; }
    return mrcal_amd_point_cloud_read(r->cloud, points, color, index);
}

bool mrcal_amd_rectification_point_cloud_stage_milliseconds(mrcal_amd_rectification_t* r, float* milliseconds)
{
    last_error_string().clear();
    if(!rectification_given(r)) return false;
    if(r->cloud == NULL) { set_error("stereo_point_cloud(): no cloud has been computed yet"); return false; }
    return mrcal_amd_point_cloud_stage_milliseconds(r->cloud, milliseconds);
}

void mrcal_amd_rectification_destroy(mrcal_amd_rectification_t* r) { delete r; }

bool mrcal_rectification_maps(float* rectification_maps,
                              const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0, const double* r_cam0_ref,
                              const mrcal_lensmodel_t* lensmodel1, const double* intrinsics1, const double* r_cam1_ref,
                              const mrcal_lensmodel_type_t rectification_model_type,
                              const double* fxycxy_rectified, const unsigned int* imagersize_rectified,
                              const double* r_rect0_ref)
{
    mrcal_amd_rectification_t* r =
        mrcal_amd_rectification_create(lensmodel0, intrinsics0, r_cam0_ref, lensmodel1, intrinsics1, r_cam1_ref,
                                       rectification_model_type, fxycxy_rectified, imagersize_rectified, r_rect0_ref, 0.0);
    if(r == NULL) return false;
    const bool ok = mrcal_amd_rectification_maps(r, rectification_maps);
    mrcal_amd_rectification_destroy(r);
    return ok;
}

bool mrcal_amd_transform_image(void* out, const void* image, int width, int height, int channels, int dtype,
                               const float* mapxy, int width_out, int height_out,
                               int interpolation, int border_mode, const double* border_value)
{
    return mrcal_amd_transform_image_smoothed(out, image, width, height, channels, dtype, mapxy, width_out, height_out,
                                              interpolation, border_mode, border_value, NULL);
}

bool mrcal_amd_transform_image_smoothed(void* out, const void* image, int width, int height, int channels, int dtype,
                                        const float* mapxy, int width_out, int height_out,
                                        int interpolation, int border_mode, const double* border_value,
                                        const mrcal_amd_smooth_params_t* params)
{
    last_error_string().clear();
    if(!remap_arguments_ok(width, height, channels, dtype, width_out, height_out, interpolation, border_mode)) return false;
    ImagePreparation preparation;
    preparation.antialias = smooth_params_of(params);
    std::string why;
    if(!preparation.ok(&why, width, height, channels, dtype)) { set_error("%s", why.c_str()); return false; }
    if(!have_device()) return false;
    DeviceBuffers tmp;
    float* d_map = NULL;
    if(!tmp.upload(&d_map, mapxy, (size_t)2*width_out*height_out)) return false;
    return remap_host_image(out, image, width, height, channels, dtype, d_map, width_out*height_out,
                            interpolation, border_mode, border_value, preparation);
}

bool mrcal_amd_stereo_range_sparse(double* range, double* p, const double* disparity, const mrcal_point2_t* qrect0,
                                   const int N, const double disparity_min, const double disparity_max,
                                   const mrcal_lensmodel_type_t rectification_model_type,
                                   const double* fxycxy_rectified, const double baseline)
{
    last_error_string().clear();
    RangeArgs a;
    if(!range_arguments(&a, rectification_model_type, fxycxy_rectified, baseline)) return false;
    if(disparity_min >= disparity_max) { set_error("Must have disparity_max > disparity_min"); return false; }
    if(N <= 0) return true;
    if(!have_device()) return false;
    DeviceBuffers tmp;
    double *d_d = NULL, *d_q = NULL, *d_r = NULL, *d_p = NULL;
    bool ok = tmp.upload(&d_d, disparity, (size_t)N) && tmp.upload(&d_q, (const double*)qrect0, (size_t)2*N);
    if(range != NULL) ok = ok && tmp.alloc(&d_r, (size_t)N);
    if(p     != NULL) ok = ok && tmp.alloc(&d_p, (size_t)3*N);
    if(!ok) return false;
    hipLaunchKernelGGL(stereo_range_sparse_kernel, dim3((N + 255)/256), dim3(256), 0, NULL,
                       a, N, d_d, d_q, disparity_min, disparity_max, d_r, d_p);
    HIP_TRY(hipGetLastError(), return false);
    if(range != NULL) HIP_TRY(hipMemcpy(range, d_r, (size_t)N*sizeof(double),   hipMemcpyDeviceToHost), return false);
    if(p     != NULL) HIP_TRY(hipMemcpy(p,     d_p, (size_t)3*N*sizeof(double), hipMemcpyDeviceToHost), return false);
    return true;
}

bool mrcal_stereo_range_sparse(double* range, const double* disparity, const mrcal_point2_t* qrect0, const int N,
                               const double disparity_min, const double disparity_max,
                               const mrcal_lensmodel_type_t rectification_model_type,
                               const double* fxycxy_rectified, const double baseline)
{
    return mrcal_amd_stereo_range_sparse(range, NULL, disparity, qrect0, N, disparity_min, disparity_max,
                                         rectification_model_type, fxycxy_rectified, baseline);
}

bool mrcal_stereo_range_dense(mrcal_image_double_t* range, const mrcal_image_uint16_t* disparity_scaled,
                              const uint16_t disparity_scale,
                              const uint16_t disparity_scaled_min, const uint16_t disparity_scaled_max,
                              const mrcal_lensmodel_type_t rectification_model_type,
                              const double* fxycxy_rectified, const double baseline)
{
    last_error_string().clear();
    RangeArgs a;
    if(!range_arguments(&a, rectification_model_type, fxycxy_rectified, baseline)) return false;
    if(disparity_scaled_min >= disparity_scaled_max) { set_error("Must have disparity_scaled_max > disparity_scaled_min"); return false; }
    if(range->width != disparity_scaled->width || range->height != disparity_scaled->height)
    {
        set_error("range and disparity_scaled MUST have the same dimensions. Got (W,H): (%d,%d) and (%d,%d) respectively",
                  range->width, range->height, disparity_scaled->width, disparity_scaled->height);
        return false;
    }
    if(!have_device()) return false;
    const int W = range->width, H = range->height;
    if(W <= 0 || H <= 0) return true;
    // the strides are the host's business: dense copies either side of the launch
    const bool dense_d = disparity_scaled->stride == W*(int)sizeof(uint16_t), dense_r = range->stride == W*(int)sizeof(double);
    std::vector<uint16_t> d; std::vector<double> r;
    if(!dense_d)
    {
        d.resize((size_t)W*H);
        for(int i=0;i<H;i++) memcpy(&d[(size_t)i*W], (const char*)disparity_scaled->data + (size_t)i*disparity_scaled->stride, W*sizeof(uint16_t));
    }
    if(!dense_r) r.resize((size_t)W*H);
    if(!range_dense(dense_r ? range->data : r.data(), dense_d ? disparity_scaled->data : d.data(), W, H, a,
                    disparity_scale, disparity_scaled_min, disparity_scaled_max))
        return false;
    if(!dense_r)
        for(int i=0;i<H;i++) memcpy((char*)range->data + (size_t)i*range->stride, &r[(size_t)i*W], W*sizeof(double));
    return true;
}

} // extern "C"
