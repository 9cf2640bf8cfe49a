// Regional statistics of the board residuals (include/mrcal_amd.h, "regional statistics"; the reference:
// mrcal/calibration.py:1720-1866, _report_regional_statistics()): per camera a grid of cells over the imager, per cell
// the mean, the population standard deviation and the count of the x and y residuals of the corners inside it. All
// the cameras of a problem in one pass, a stable counting sort of the corners by (camera, cell) followed by one
// wavefront per cell (the sizes: regional_stats_plan.hpp):
//   rs_key_kernel         a lane a corner: its (up to RS_SLOTS) cells by the two strict inequalities against the table
//                         of centres, counted into hist[chunk][cell] (integer atomics: a count has no order)
//   rs_chunk_scan_kernel  a lane a cell: hist[.][cell] scanned down the chunks, the cell's total
//   rs_cell_scan_kernel   one workgroup: the totals scanned into start[]
//   rs_rank_kernel        a wavefront a chunk, 64 corners at a time in order: an entry's place is start[cell] + the
//                         entries of earlier chunks + those of earlier passes of this chunk + those of lower lanes
//                         of this pass. The running count of a chunk's row of hist is read and written by this one
//                         wavefront only
//   rs_reduce_kernel      a wavefront a cell: lane l sums values l, l + 64, ... of the cell's run (value v = the x
//                         (v even) or y (v odd) residual of entry v/2), the lanes are summed by the butterfly
//                         xor 32, 16 .. 1; the mean; the squared deviations the same way
// No floating-point atomics: the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <memory>
#include <vector>
#include "layout.hpp"
#include "host_state.hpp"
#include "problem_object.hpp"
#include "noise_propagation.hpp"
#include "regional_stats_plan.hpp"
#include "regional_stats.hpp"
#include "resident_common.hpp"
#include "wave_sum.hpp"
#include "../../include/mrcal_amd.h"

using namespace mrcal_amd;

namespace {

// the (up to two) cells along one axis whose inequality |q - centre[i]| < half the coordinate q meets: -1 for none
__device__ inline void rs_cells_of(int out[2], double q, const double* __restrict__ centre, int n, double cell, double half)
{
    out[0] = out[1] = -1;
    if(!(fabs(q) < 1.0e9)) return;                          // (nan and inf as well)
    const double t = q/cell;
    const int i0 = (int)floor(t + 0.5);
    int k = 0;
    for(int i = i0 - 1; i <= i0 + 1 && k < 2; i++)
    {
        if(i < 0 || i >= n) continue;
        // (a subtraction alone: nothing here for the compiler to fuse)
        const double d = q - centre[i];
        if(fabs(d) < half) out[k++] = i;
    }
}

__global__ __launch_bounds__(256)
void rs_key_kernel(int Ncorners, int HW, int Ncells, const BoardObsMeta* __restrict__ meta, const double* __restrict__ pool,
                   const RegionalCamera* __restrict__ cams, const double* __restrict__ centres,
                   int* __restrict__ keys /* [Ncorners][RS_SLOTS] */, int* __restrict__ hist)
{
    const int chunk = blockIdx.x;
    for(int t = threadIdx.x; t < RS_CHUNK; t += blockDim.x)
    {
        const int g = chunk*RS_CHUNK + t;
        if(g >= Ncorners) break;
        int key[RS_SLOTS] = { -1, -1, -1, -1 };
        const double qx = pool[3*(size_t)g], qy = pool[3*(size_t)g + 1], w = pool[3*(size_t)g + 2];
        if(w > 0.0)
        {
            const RegionalCamera cam = cams[meta[g/HW].icam_intrinsics];
            int ix[2], iy[2];
            rs_cells_of(ix, qx, centres + cam.centre0,                   cam.gridn_width,  cam.wcell, cam.half_w);
            rs_cells_of(iy, qy, centres + cam.centre0 + cam.gridn_width, cam.gridn_height, cam.hcell, cam.half_h);
            int k = 0;
            for(int b = 0; b < 2; b++)
                for(int a = 0; a < 2; a++)
                    if(ix[a] >= 0 && iy[b] >= 0) key[k++] = cam.cell0 + iy[b]*cam.gridn_width + ix[a];
        }
        for(int e = 0; e < RS_SLOTS; e++)
        {
            keys[(size_t)RS_SLOTS*g + e] = key[e];
            if(key[e] >= 0 && key[e] < Ncells) atomicAdd(&hist[(size_t)chunk*Ncells + key[e]], 1);
        }
    }
}

__global__ __launch_bounds__(256)
void rs_chunk_scan_kernel(int Nchunks, int Ncells, int* __restrict__ hist, int* __restrict__ total)
{
    const int cell = blockIdx.x*blockDim.x + threadIdx.x;
    if(cell >= Ncells) return;
    int run = 0;
    for(int c = 0; c < Nchunks; c++)
    {
        const int n = hist[(size_t)c*Ncells + cell];
        hist[(size_t)c*Ncells + cell] = run;
        run += n;
    }
    total[cell] = run;
}

// start[i] = total[0] + .. + total[i-1], i = 0 .. Ncells: thread t owns the items t*per .. t*per + per - 1
__global__ __launch_bounds__(RS_SCAN_THREADS)
void rs_cell_scan_kernel(int Ncells, int per, const int* __restrict__ total, int* __restrict__ start)
{
    __shared__ int part[RS_SCAN_THREADS];
    const int t = threadIdx.x, i0 = t*per, i1 = min(i0 + per, Ncells);
    int s = 0;
    for(int i = i0; i < i1; i++) s += total[i];
    part[t] = s;
    __syncthreads();
    for(int off = 1; off < RS_SCAN_THREADS; off <<= 1)
    {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for(int i = i0; i < i1; i++) { start[i] = run; run += total[i]; }
    if(t == RS_SCAN_THREADS - 1) start[Ncells] = part[t];
}

__global__ __launch_bounds__(64)
void rs_rank_kernel(int Ncorners, int HW, int Ncells, int Nentries_max, const BoardObsMeta* __restrict__ meta,
                    const int* __restrict__ keys, const int* __restrict__ start, int* hist, int* __restrict__ sorted)
{
    const int chunk = blockIdx.x, lane = threadIdx.x;
    int* running = hist + (size_t)chunk*Ncells;
    for(int pass = 0; pass < RS_CHUNK/64; pass++)
    {
        const int g0 = chunk*RS_CHUNK + pass*64;
        if(g0 >= Ncorners) break;
        const int g = g0 + lane;
        int key[RS_SLOTS], before[RS_SLOTS], inpass[RS_SLOTS];
#pragma unroll
        for(int e = 0; e < RS_SLOTS; e++)
        {
            key[e] = g < Ncorners ? keys[(size_t)RS_SLOTS*g + e] : -1;
            if(key[e] >= Ncells) key[e] = -1;
            before[e] = inpass[e] = 0;
        }
        // the entries of this pass with my keys: in lower lanes, and in all (a lane holds a key once at the most)
#pragma unroll
        for(int f = 0; f < RS_SLOTS; f++)
        {
            if(__ballot(key[f] >= 0) == 0) continue;                     // (wave-uniform: usually only f == 0 has any)
            for(int l = 0; l < 64; l++)
            {
                const int kl = __shfl(key[f], l);
                if(kl < 0) continue;                                     // (wave-uniform)
#pragma unroll
                for(int e = 0; e < RS_SLOTS; e++)
                    if(key[e] == kl) { inpass[e]++; if(l < lane) before[e]++; }
            }
        }
#pragma unroll
        for(int e = 0; e < RS_SLOTS; e++)
        {
            if(key[e] < 0) continue;
            const int base = __hip_atomic_load(&running[key[e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int pos  = start[key[e]] + base + before[e];
            if(pos >= 0 && pos < Nentries_max)
                sorted[pos] = meta[g/HW].i_meas0 + 2*(g % HW);
        }
        // every load of the running counts is back before any of them moves on
        __threadfence();
#pragma unroll
        for(int e = 0; e < RS_SLOTS; e++)
        {
            if(key[e] < 0 || before[e] != 0) continue;                   // the first lane of a key moves its count on
            const int base = __hip_atomic_load(&running[key[e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&running[key[e]], base + inpass[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence();
    }
}

__global__ __launch_bounds__(256)
void rs_reduce_kernel(int Ncells, int Nmeas, const int* __restrict__ start, const int* __restrict__ sorted, const double* __restrict__ x,
                      double* __restrict__ mean, double* __restrict__ stdev, int* __restrict__ count)
{
    const int cell = blockIdx.x*(blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if(cell >= Ncells) return;                                           // (a whole wavefront)
    const int e0 = start[cell], n = 2*(start[cell + 1] - e0);
    double m = 0.0, sd = 0.0;
    if(n > RS_SMALL_COUNT)
    {
        double s = 0.0;
        for(int v = lane; v < n; v += 64)
        {
            const int i = sorted[e0 + (v >> 1)] + (v & 1);
            s += (i >= 0 && i < Nmeas) ? x[i] : 0.0;
        }
        m = wave_sum(s)/(double)n;
        double s2 = 0.0;
        for(int v = lane; v < n; v += 64)
        {
            const int i = sorted[e0 + (v >> 1)] + (v & 1);
            const double d  = ((i >= 0 && i < Nmeas) ? x[i] : 0.0) - m;
            const double dd = d*d;
            s2 += dd;
        }
        sd = sqrt(wave_sum(s2)/(double)n);
    }
    if(lane == 0) { mean[cell] = m; stdev[cell] = sd; count[cell] = n; }
}

} // namespace

struct mrcal_amd_regional_statistics
{
    RegionalStatsPlan plan;
    double* d_mean  = NULL;          // [Ncells], camera by camera
    double* d_stdev = NULL;
    int*    d_count = NULL;
    double  binning_ms = 0.0;        // device time of the launches of create()
    DeviceBuffers mem;
};

namespace mrcal_amd {
bool regional_statistics_device(const mrcal_amd_regional_statistics_t* s, int icam, int* gridn_width, int* gridn_height,
                                const double** d_mean, const double** d_stdev, const int** d_count)
{
    if(s == NULL) { set_error("no regional statistics"); return false; }
    if(icam < 0 || icam >= s->plan.Ncameras)
    {
        set_error("icam_intrinsics MUST be in [0,Ncameras_intrinsics-1]. got %d NOT in [0,%d]", icam, s->plan.Ncameras - 1);
        return false;
    }
    const RegionalCamera& c = s->plan.cameras[icam];
    if(gridn_width)  *gridn_width  = c.gridn_width;
    if(gridn_height) *gridn_height = c.gridn_height;
    if(d_mean)  *d_mean  = s->d_mean  + c.cell0;
    if(d_stdev) *d_stdev = s->d_stdev + c.cell0;
    if(d_count) *d_count = s->d_count + c.cell0;
    return true;
}
}

extern "C" {

mrcal_amd_regional_statistics_t*
mrcal_amd_regional_statistics_create(mrcal_amd_problem_t* P, int gridn_width, int gridn_height)
{
    last_error_string().clear();
    if(P == NULL) { set_error("no problem"); return NULL; }
    if(propagation_refuses_shard(P, "regional statistics")) return NULL;
    const Layout& L = P->L;
    if(L.dims.Nobservations_board <= 0)
    {
        set_error("regional statistics: the problem has no board observations, and only those are binned");
        return NULL;
    }
    std::unique_ptr<mrcal_amd_regional_statistics> s(new mrcal_amd_regional_statistics());
    RegionalStatsPlan& plan = s->plan;
    const int Ncameras = L.dims.Ncameras_intrinsics, HW = L.dims.object_width_n*L.dims.object_height_n;
    std::vector<int> imagersizes((size_t)2*Ncameras);
    HIP_TRY(hipMemcpy(imagersizes.data(), P->d_imagersizes, imagersizes.size()*sizeof(int), hipMemcpyDeviceToHost), return NULL);
    std::string err;
    if(!plan_regional_stats(&plan, Ncameras, imagersizes.data(), L.dims.Nobservations_board, HW, gridn_width, gridn_height, &err))
    {
        set_error("regional statistics: %s", err.c_str());
        return NULL;
    }
    // x at the problem's state
    if(!mrcal_amd_problem_evaluate(P, false, true)) return NULL;

    const int Ncorners = (int)plan.Ncorners, Ncells = plan.Ncells;
    DeviceBuffers tmp;
    RegionalCamera* d_cams = NULL;
    double* d_centres = NULL;
    int *d_keys = NULL, *d_hist = NULL, *d_total = NULL, *d_start = NULL, *d_sorted = NULL;
    if(!s->mem.alloc(&s->d_mean, (size_t)Ncells) || !s->mem.alloc(&s->d_stdev, (size_t)Ncells) || !s->mem.alloc(&s->d_count, (size_t)Ncells) ||
       !tmp.upload(&d_cams, plan.cameras) || !tmp.upload(&d_centres, plan.centres) ||
       !tmp.alloc(&d_keys, (size_t)plan.Nentries_max) || !tmp.alloc(&d_hist, (size_t)plan.hist_ints) ||
       !tmp.alloc(&d_total, (size_t)Ncells) || !tmp.alloc(&d_start, (size_t)Ncells + 1) ||
       !tmp.alloc_zeroed(&d_sorted, (size_t)plan.Nentries_max))
        return NULL;

    hipStream_t st = P->stream;
    StageEvents<2> events;          // around the binning
    if(!events.create()) return NULL;
    bool ok = events.record(0, st);
    if(ok) HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)plan.hist_ints*sizeof(int), st), ok = false);
    if(ok)
    {
        hipLaunchKernelGGL(rs_key_kernel, dim3(plan.Nchunks), dim3(256), 0, st, Ncorners, HW, Ncells, P->d_board_meta,
                           P->d_board_pool, d_cams, d_centres, d_keys, d_hist);
        hipLaunchKernelGGL(rs_chunk_scan_kernel, dim3((Ncells + 255)/256), dim3(256), 0, st, plan.Nchunks, Ncells, d_hist, d_total);
        hipLaunchKernelGGL(rs_cell_scan_kernel, dim3(1), dim3(RS_SCAN_THREADS), 0, st, Ncells, plan.scan_items_per_thread, d_total, d_start);
        hipLaunchKernelGGL(rs_rank_kernel, dim3(plan.Nchunks), dim3(64), 0, st, Ncorners, HW, Ncells, (int)plan.Nentries_max,
                           P->d_board_meta, d_keys, d_start, d_hist, d_sorted);
        hipLaunchKernelGGL(rs_reduce_kernel, dim3((Ncells + 3)/4), dim3(256), 0, st, Ncells, L.Nmeas, d_start, d_sorted,
                           P->op[P->icur].x, s->d_mean, s->d_stdev, s->d_count);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    ok = ok && events.record(1, st);
    // (also on failure: nothing queued may still be using the temporaries)
    HIP_TRY(hipStreamSynchronize(st), ok = false);
    if(ok)
    {
        float ms = 0.f;
        ok = events.elapsed(&ms, 0, 1);
        s->binning_ms = ms;
    }
    return ok ? s.release() : NULL;
}

bool mrcal_amd_regional_statistics_grid(const mrcal_amd_regional_statistics_t* s, int icam, int* gridn_width, int* gridn_height)
{
    last_error_string().clear();
    return regional_statistics_device(s, icam, gridn_width, gridn_height, NULL, NULL, NULL);
}

bool mrcal_amd_regional_statistics_get(const mrcal_amd_regional_statistics_t* s, int icam, double* mean, double* stdev, int32_t* count)
{
    last_error_string().clear();
    int gw, gh;
    const double *d_mean, *d_stdev;
    const int* d_count;
    if(!regional_statistics_device(s, icam, &gw, &gh, &d_mean, &d_stdev, &d_count)) return false;
    const size_t n = (size_t)gw*gh;
    if(mean)  HIP_TRY(hipMemcpy(mean,  d_mean,  n*sizeof(double),  hipMemcpyDeviceToHost), return false);
    if(stdev) HIP_TRY(hipMemcpy(stdev, d_stdev, n*sizeof(double),  hipMemcpyDeviceToHost), return false);
    if(count) HIP_TRY(hipMemcpy(count, d_count, n*sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    return true;
}

double mrcal_amd_regional_statistics_binning_ms(const mrcal_amd_regional_statistics_t* s)
{
    return s ? s->binning_ms : -1.0;
}

void mrcal_amd_regional_statistics_destroy(mrcal_amd_regional_statistics_t* s) { delete s; }

} // extern "C"
