// The valid-intrinsics region (include/mrcal_amd.h, "valid-intrinsics region"): making its mask, and applying one.
//
// Making (mrcal/calibration.py:1611-1700): the grid of sample_imager() is made on the device, unprojected through
// the model to unit vectors, scaled by the distance, handed to uncertainty_evaluate_device() for the worst-direction
// standard deviation, and vr_mask_kernel applies the rule against the resident regional statistics. Only the mask
// crosses to the host (and the uncertainties, where the caller asks to see them). The outline of the mask is host
// code: region_outline.cpp.
//
// Applying (mrcal/model_analysis.py:2106-2149): vr_polygon_kernel, a lane a point, the even-odd rule against every
// edge, the vertices in LDS up to VR_LDS_VERTICES of them and read from global memory beyond. Strictly inside: a point
// on an edge or a vertex is outside. With integer vertices and an integer-valued point, all below 2^24 in size, every
// difference (< 2^25), product (< 2^50) and difference of products (< 2^51) is an integer a double holds: the
// decision is exact, fused or not. For other points the decision within rounding of an edge is not specified.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "layout.hpp"
#include "kernels.hpp"
#include "host_state.hpp"
#include "lens_dispatch.hpp"
#include "device_memory.hpp"
#include "noise_propagation.hpp"
#include "regional_stats_plan.hpp"
#include "regional_stats.hpp"
#include "../../include/mrcal_amd.h"

using namespace mrcal_amd;

namespace {

constexpr int VR_LDS_VERTICES = 4096;          // 64 KB of LDS

// sample_imager(): q[j][i] = (cx[i], cy[j]), the centres by THE formula (regional_stats_plan.hpp)
__global__ __launch_bounds__(256)
void vr_grid_kernel(int gw, int gh, int W, int H, double* __restrict__ q)
{
    const int n = blockIdx.x*blockDim.x + threadIdx.x;
    if(n >= gw*gh) return;
    const int i = n % gw, j = n / gw;
    const double stepx = (double)(W - 1)/(double)(gw - 1), stepy = (double)(H - 1)/(double)(gh - 1);
    q[2*(size_t)n]     = i == gw - 1 ? (double)(W - 1) : (double)i*stepx;
    q[2*(size_t)n + 1] = j == gh - 1 ? (double)(H - 1) : (double)j*stepy;
}

__global__ __launch_bounds__(256)
void vr_scale_kernel(int n, double distance, double* __restrict__ v)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i < n) v[i] = v[i]*distance;
}

struct MaskThresholds { double uncertainty, mean, stdev, count; };

__global__ __launch_bounds__(256)
void vr_mask_kernel(int N, const double* __restrict__ uncertainty, const double* __restrict__ mean, const double* __restrict__ stdev,
                    const int* __restrict__ count, bool with_statistics, MaskThresholds t, unsigned char* __restrict__ mask)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= N) return;
    double u = uncertainty[i];
    if(!isfinite(u)) u = 1.0e9;
    bool m = u < t.uncertainty;
    if(with_statistics)
        m = m && mean[i] < t.mean && stdev[i] < t.stdev && (double)count[i] > t.count;
    mask[i] = m ? 1 : 0;
}

// q == NULL: the pixel centres of a W-wide image, point p = (p % W, p / W)
template<bool LDS>
__global__ __launch_bounds__(256)
void vr_polygon_kernel(long long N, const double* __restrict__ q, int W, const double* __restrict__ vertices, int Nvertices,
                       unsigned char* __restrict__ out)
{
    extern __shared__ double sV[];
    const double* __restrict__ V = vertices;
    if(LDS)
    {
        for(int i = threadIdx.x; i < 2*Nvertices; i += blockDim.x) sV[i] = vertices[i];
        __syncthreads();
        V = sV;
    }
    for(long long p = (long long)blockIdx.x*blockDim.x + threadIdx.x; p < N; p += (long long)gridDim.x*blockDim.x)
    {
        double px, py;
        if(q != NULL) { px = q[2*p]; py = q[2*p + 1]; }
        else          { px = (double)(p % W); py = (double)(p / W); }
        bool inside = false, on_border = false;
        for(int e = 0; e + 1 < Nvertices; e++)
        {
            const double x0 = V[2*e], y0 = V[2*e + 1], x1 = V[2*e + 2], y1 = V[2*e + 3];
            const double dx = x1 - x0, dy = y1 - y0, rx = px - x0, ry = py - y0;
            const double a = dx*ry, b = dy*rx;
            if(a == b)
            {
                // on the line of the edge: on the edge itself if inside its box
                if(px >= fmin(x0, x1) && px <= fmax(x0, x1) && py >= fmin(y0, y1) && py <= fmax(y0, y1)) on_border = true;
            }
            else if((y0 > py) != (y1 > py))
            {
                // the edge crosses the point's row: to the right of the point?
                if((a > b) == (dy > 0.0)) inside = !inside;
            }
        }
        out[p] = (inside && !on_border && isfinite(px) && isfinite(py)) ? 1 : 0;
    }
}

bool launch_polygon(long long N, const double* d_q, int W, const double* d_vertices, int Nvertices, unsigned char* d_out)
{
    if(N <= 0) return true;
    const unsigned blocks = (unsigned)std::min<long long>((N + 255)/256, 65536);
    if(Nvertices <= VR_LDS_VERTICES)
        hipLaunchKernelGGL(vr_polygon_kernel<true>, dim3(blocks), dim3(256), (size_t)2*std::max(Nvertices, 1)*sizeof(double), NULL,
                           N, d_q, W, d_vertices, Nvertices, d_out);
    else
        hipLaunchKernelGGL(vr_polygon_kernel<false>, dim3(blocks), dim3(256), 0, NULL, N, d_q, W, d_vertices, Nvertices, d_out);
    HIP_TRY(hipGetLastError(), return false);
    return true;
}

bool polygon_arguments_ok(const double* vertices, int Nvertices)
{
    if(mrcal_amd_device_count() <= 0)
    {
        set_error("no HIP device is visible: libmrcal_amd has no CPU fallback");
        return false;
    }
    if(Nvertices < 0 || (Nvertices > 0 && vertices == NULL)) { set_error("valid-intrinsics region: no vertices"); return false; }
    return true;
}

} // namespace

extern "C" {

int mrcal_amd_valid_region_lds_vertices(void) { return VR_LDS_VERTICES; }

bool mrcal_amd_valid_region_mask(mrcal_amd_uncertainty_t* u, const mrcal_amd_regional_statistics_t* s, int icam_intrinsics,
                                 const mrcal_lensmodel_t* lensmodel, const double* intrinsics, int W, int H,
                                 int gridn_width, int gridn_height, double distance,
                                 double threshold_uncertainty, double threshold_mean, double threshold_stdev, double threshold_count,
                                 uint8_t* mask, double* uncertainty)
{
    last_error_string().clear();
    if(u == NULL) { set_error("no uncertainty context"); return false; }
    if(lensmodel == NULL || intrinsics == NULL || mask == NULL) { set_error("valid-intrinsics region: a NULL argument"); return false; }
    if(gridn_width < 2 || gridn_height < 2 || (int64_t)gridn_width*gridn_height > RS_MAX_CELLS)
    {
        set_error("valid-intrinsics region: gridn_width and gridn_height must be >= 2 (and have at most %d cells): got %d, %d",
                  RS_MAX_CELLS, gridn_width, gridn_height);
        return false;
    }
    if(W < 2 || H < 2) { set_error("valid-intrinsics region: the imager must be at least 2x2 pixels"); return false; }
    if(!lens_supported((int)lensmodel->type)) { set_error("valid-intrinsics region: lens model %d is not supported", (int)lensmodel->type); return false; }
    const bool with_statistics = lensmodel->type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC;
    const double *d_mean = NULL, *d_stdev = NULL;
    const int* d_count = NULL;
    if(with_statistics)
    {
        int gw, gh;
        if(!regional_statistics_device(s, icam_intrinsics, &gw, &gh, &d_mean, &d_stdev, &d_count)) return false;
        if(gw != gridn_width || gh != gridn_height)
        {
            set_error("valid-intrinsics region: the regional statistics are on a %d x %d grid, the region on a %d x %d grid", gw, gh, gridn_width, gridn_height);
            return false;
        }
    }
    const int N = gridn_width*gridn_height, Ni = lensmodel_num_params(*lensmodel);
    DeviceBuffers tmp;
    double *d_q = NULL, *d_i = NULL, *d_v = NULL, *d_u = NULL;
    unsigned char* d_mask = NULL;
    if(!tmp.alloc(&d_q, (size_t)2*N) || !tmp.upload(&d_i, intrinsics, (size_t)Ni) || !tmp.alloc(&d_v, (size_t)3*N) ||
       !tmp.alloc(&d_u, (size_t)N) || !tmp.alloc(&d_mask, (size_t)N))
        return false;
    bool ok = true;
    hipLaunchKernelGGL(vr_grid_kernel, dim3((N + 255)/256), dim3(256), 0, NULL, gridn_width, gridn_height, W, H, d_q);
    HIP_TRY(hipGetLastError(), ok = false);
    if(ok) HIP_TRY(launch_unproject_points((int)lensmodel->type, lens_config_of(*lensmodel), N, Ni, d_q, d_i, d_v, NULL, NULL,
                                           NULL, NULL, NULL, true, NULL), ok = false);
    if(ok && distance > 0.0)
    {
        hipLaunchKernelGGL(vr_scale_kernel, dim3((3*N + 255)/256), dim3(256), 0, NULL, 3*N, distance, d_v);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    ok = ok && uncertainty_evaluate_device(u, d_v, N, !(distance > 0.0), MRCAL_AMD_UNCERTAINTY_WORSTDIRECTION_STDEV, d_u, NULL);
    if(ok)
    {
        const MaskThresholds t = { threshold_uncertainty, threshold_mean, threshold_stdev, threshold_count };
        hipLaunchKernelGGL(vr_mask_kernel, dim3((N + 255)/256), dim3(256), 0, NULL, N, d_u, d_mean, d_stdev, d_count, with_statistics, t, d_mask);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    if(ok) HIP_TRY(hipMemcpy(mask, d_mask, (size_t)N, hipMemcpyDeviceToHost), ok = false);
    if(ok && uncertainty != NULL) HIP_TRY(hipMemcpy(uncertainty, d_u, (size_t)N*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    // (also on failure: nothing queued may still be using the temporaries)
    HIP_TRY(hipStreamSynchronize(NULL), ok = false);
    return ok;
}

bool mrcal_amd_valid_region_contains(uint8_t* out, const double* q, int64_t N, const double* vertices, int Nvertices)
{
    last_error_string().clear();
    if(!polygon_arguments_ok(vertices, Nvertices)) return false;
    if(N <= 0) return true;
    if(q == NULL || out == NULL) { set_error("valid-intrinsics region: a NULL argument"); return false; }
    DeviceBuffers tmp;
    double *d_q = NULL, *d_v = NULL;
    unsigned char* d_out = NULL;
    bool ok = tmp.upload(&d_q, q, (size_t)2*N) && tmp.upload(&d_v, vertices, (size_t)2*Nvertices) && tmp.alloc(&d_out, (size_t)N) &&
              launch_polygon(N, d_q, 1, d_v, Nvertices, d_out);
    if(ok) HIP_TRY(hipMemcpy(out, d_out, (size_t)N, hipMemcpyDeviceToHost), ok = false);
    HIP_TRY(hipStreamSynchronize(NULL), ok = false);
    return ok;
}

bool mrcal_amd_valid_region_image(uint8_t* out, int W, int H, const double* vertices, int Nvertices)
{
    last_error_string().clear();
    if(!polygon_arguments_ok(vertices, Nvertices)) return false;
    if(W <= 0 || H <= 0 || out == NULL) { set_error("valid-intrinsics region: the image must have a size"); return false; }
    const long long N = (long long)W*H;
    DeviceBuffers tmp;
    double* d_v = NULL;
    unsigned char* d_out = NULL;
    bool ok = tmp.upload(&d_v, vertices, (size_t)2*Nvertices) && tmp.alloc(&d_out, (size_t)N) &&
              launch_polygon(N, NULL, W, d_v, Nvertices, d_out);
    if(ok) HIP_TRY(hipMemcpy(out, d_out, (size_t)N, hipMemcpyDeviceToHost), ok = false);
    HIP_TRY(hipStreamSynchronize(NULL), ok = false);
    return ok;
}

} // extern "C"
