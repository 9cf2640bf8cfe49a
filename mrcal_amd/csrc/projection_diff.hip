// Projection differences between camera models (mrcal.projection_diff(), mrcal/model_analysis.py:1520-1928) and the
// fit in their middle, the implied transformation (implied_Rt10__from_unprojections(), :27-395), on the device.
//
// The fit. Point i has the camera-0 point p0_i, the camera-1 unit vector v1_i and a weight w_i; with p = R(r) p0_i (+ t)
//   x_i = 2 (1 - v1_i . p/|p|) w_i          (at infinity |p| = 1 is taken for granted, as the reference does)
//   F   = 1/2 sum C^2 rho(x_i^2/C^2)        C = (5 deg)^2,  rho(z) = z (z <= 1), 2 sqrt(z) - 1 (else): scipy's 'huber'
// minimised over r (at infinity) or (r,t) by damped Gauss-Newton on the IRLS form: omega_i = rho'(z_i),
// H = sum omega_i j_i j_i^T, g = sum omega_i j_i x_i, (H + lambda diag(H)) d = -g, a trial kept only if F does not rise.
// The start is rt = 0. x_i is an angle SQUARED: its gradient vanishes at a perfect fit, where the steps halve the
// error each time rather than squaring it; the loop then ends at the rounding of 1 - cos (FIT_NOISE below).
//
// Kernels:
//   pd_fit_kernel<NP>   ONE fit a workgroup (blockIdx.x: which), every iteration inside the launch. Threads stride over
//                       the points and keep 1 + NP + NP(NP+1)/2 partial sums (F, g, the upper triangle of H: 28 for
//                       (r,t), 10 for r), summed in a fixed order: a thread's points in order, a butterfly over the
//                       wave, the waves in order by thread 0 from LDS. Thread 0 factors H, accepts or rejects, moves
//                       lambda, decides termination and publishes the next trial (R, dR/dr, t) and the verdict in
//                       LDS: every thread takes the same branch at every barrier. No floating-point atomics: the same
//                       bits on every call. The input is sanitised as it is read (the reference's rules, and one more:
//                       a zero vector, which is what a failed unprojection normalizes to, takes no part)
//   pd_scale_kernel     p = v d for every distance
//   pd_weights_kernel   w = 1/(u0 u1)^2
//   pd_transform_kernel p1 = Rt10 p0 for every fit
//   pd_diff_kernel      q1 - q0, and its length (the root-mean-square over the fits when there are several)
// The projection and the unprojection are the existing launchers (project_kernels.hip), the uncertainties the existing
// per-point kernel (projection_uncertainty.hip) through its device-pointer form.
#include <hip/hip_runtime.h>
#include <math.h>
#include <float.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "layout.hpp"
#include "kernels.hpp"
#include "host_state.hpp"
#include "lens_models.hpp"
#include "lens_dispatch.hpp"
#include "device_math.hpp"
#include "damped_newton.hpp"
#include "wave_sum.hpp"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "noise_propagation.hpp"
#include "../../include/mrcal_amd.h"

using namespace mrcal_amd;

namespace {

// The loop's bound on cost evaluations, the first one included. The slowest case rehearsed on the CPU (one finite
// distance, a region of gross misfit: the Huber weights move a little each time) took about 200; a fit that has not
// converged by 400 is reported as such (FIT_STATUS_BOUND), not repeated
constexpr int    FIT_MAX_EVALUATIONS = 400;
constexpr double FIT_C               = (5.0*M_PI/180.0)*(5.0*M_PI/180.0);
constexpr double FIT_LAMBDA0         = 1e-3;
constexpr double FIT_LAMBDA_MIN      = 1e-15;
constexpr double FIT_LAMBDA_MAX      = 1e10;      // beyond it a step is < 1e-10 of the Gauss-Newton step: no descent to be had
                                                  // (lambda doubles, quadruples, ... after rejections: 9 in a row get there from 1e-3)
constexpr double FIT_FTOL            = 1e-12;     // an accepted step that gains less than this part of F ends the fit
// 1 - v1.p/|p| is computed from unit vectors: the dot product and the division leave it good to an ulp or so of 1, and
// x_i/w_i = 2 (1 - cos) to 2..3 eps. A cost at or below 1/2 sum (3 eps w_i)^2 is a perfect fit as far as doubles can
// tell, and steps from there would follow the rounding. (A model against itself ends here at the start: the identity)
constexpr double FIT_NOISE           = 3.0*DBL_EPSILON;
// (512, not 1024: the 28 sums of a thread and the 39 values of R, dR/dr, t it multiplies every point by are 134
//  VGPRs between them, and a workgroup of 1024 leaves a thread 128: it spilled 496 bytes)
constexpr int    FIT_MAX_THREADS     = 512;
constexpr int    FIT_MAX_WAVES       = FIT_MAX_THREADS/64;
constexpr int    FIT_NSUMS_MAX       = 28;

enum { FIT_STATUS_CONVERGED = 0, FIT_STATUS_BOUND = 1, FIT_STATUS_TOO_FEW_POINTS = 2, FIT_STATUS_STALLED = 3 };
// what a fit writes: rt (6), F, evaluations, points used, status
constexpr int FIT_RES_N = 10;

struct FitArgs
{
    int    M, N;            // p0 [M][N][3], weights [M][N]: every m takes part in the one fit
    double fc[2], r2;       // focus: points with |q0 - fc|^2 < r2
    size_t v1_stride;       // per fit (blockIdx.x), in doubles
    size_t w_stride;
};

struct FitState
{
    double rt[6], F, g[6], H[21];
    Damping damp;
    double pred, floor;
    double R[9], dR[27], t[6];      // the trial the threads evaluate: t[0..2] r, t[3..5] the translation
    double L[6][6], d[6];           // thread 0's factorization (in LDS: indexed by loop counters, it would spill)
    int    done, status, nevals, nused;
};

// One point, sanitised: false if it takes no part (outside the focus region, or weight 0 - which includes every point
// a non-finite value was found in)
__device__ __forceinline__
bool fit_load_point(double* p0, double* v1, double* w, const FitArgs& a, int idx,
                    const double* __restrict__ q0, const double* __restrict__ p0g, const double* __restrict__ v1g,
                    const double* __restrict__ wg)
{
    const int n = idx % a.N;
    const double dx = q0[2*(size_t)n] - a.fc[0], dy = q0[2*(size_t)n + 1] - a.fc[1];
    if(!(dx*dx + dy*dy < a.r2)) return false;
    double ww = wg != NULL ? wg[idx] : 1.0;
    if(!isfinite(ww)) ww = 0.0;
#pragma unroll
    for(int k = 0; k < 3; k++)
    {
        p0[k] = p0g[3*(size_t)idx + k];
        v1[k] = v1g[3*(size_t)n + k];
        if(!isfinite(p0[k])) { p0[k] = 0.0; ww = 0.0; }
        if(!isfinite(v1[k])) { v1[k] = 0.0; ww = 0.0; }
    }
    // A zero vector is what a failed unprojection normalizes to (mrcal/projections.py:336-344). A zero v1 makes x_i a
    // constant in the reference's cost; a zero p0 does at infinity, and at a finite distance leaves p = t, 0/0 at the
    // start: neither says anything about the transformation, and they take no part here
    if((p0[0] == 0.0 && p0[1] == 0.0 && p0[2] == 0.0) || (v1[0] == 0.0 && v1[1] == 0.0 && v1[2] == 0.0)) ww = 0.0;
    *w = ww;
    return ww != 0.0;
}

// acc[0..NS) of every thread summed: the wave by a butterfly, then the waves in order by thread 0 into tot. Ends in a
// barrier-free state: the caller synchronises before anybody else reads what thread 0 makes of tot
template<int NS>
__device__ __forceinline__
void fit_sum(double* tot, double* acc, double (*s_red)[FIT_NSUMS_MAX])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Nwaves = (blockDim.x + 63) >> 6;
#pragma unroll
    for(int k = 0; k < NS; k++)
    {
        const double s = wave_sum(acc[k]);
        if(lane == 0) s_red[wave][k] = s;
    }
    __syncthreads();
    if(threadIdx.x == 0)
#pragma unroll
        for(int k = 0; k < NS; k++)
        {
            double s = s_red[0][k];
            for(int w = 1; w < Nwaves; w++) s += s_red[w][k];
            tot[k] = s;
        }
}

// Thread 0, after evaluation number eval (0: the start) gave tot = (F, g, H) at S.t: keep the trial or not, lambda,
// termination, the next trial. The step itself: damped_newton.hpp
template<int NP>
__device__
void fit_control(FitState& S, const double* tot, int eval)
{
    constexpr int NH = NP*(NP + 1)/2;
    const double Fn = tot[0];
    bool done = false;
    int status = FIT_STATUS_CONVERGED;
    if(eval == 0 || Fn <= S.F)
    {
        const double dF = eval == 0 ? 0.0 : S.F - Fn;
        double gmax = 0.0;
        for(int k = 0; k < NP; k++) { S.rt[k] = S.t[k]; S.g[k] = tot[1 + k]; gmax = fmax(gmax, fabs(S.g[k])); }
        for(int k = 0; k < NH; k++) S.H[k] = tot[1 + NP + k];
        S.F = Fn;
        if(eval > 0) S.damp.accepted(dF, S.pred, FIT_LAMBDA_MIN);
        bool gfinite = true;
        for(int k = 0; k < NP; k++) gfinite = gfinite && isfinite(S.g[k]);
        if(Fn <= S.floor || (gfinite && gmax == 0.0) || (eval > 0 && dF <= FIT_FTOL*Fn)) done = true;
    }
    else S.damp.rejected();
    if(!done && eval + 1 >= FIT_MAX_EVALUATIONS) { done = true; status = FIT_STATUS_BOUND; }

    while(!done)
    {
        if(!(S.damp.lambda <= FIT_LAMBDA_MAX)) { done = true; status = FIT_STATUS_STALLED; break; }
        double pred;
        bool ok = damped_step<false>(S.L, S.d, &pred, S.H, S.g, NP, S.damp.lambda);
        if(ok)
        {
            // F = 1/2 sum: half of what the step promises for x.x
            S.pred = 0.5*pred;
            for(int k = 0; k < NP; k++) { S.t[k] = S.rt[k] + S.d[k]; ok = ok && isfinite(S.t[k]); }
        }
        if(ok) break;
        S.damp.rejected();
    }
    if(!done) R_from_r_with_grad(S.R, S.dR, S.t);
    S.done   = done ? 1 : 0;
    S.status = status;
    S.nevals = eval + 1;
}

template<int NP>        // 3: the rotation alone (at infinity); 6: rotation and translation
__global__ __launch_bounds__(FIT_MAX_THREADS)
void pd_fit_kernel(FitArgs a, const double* __restrict__ q0, const double* __restrict__ p0g, const double* __restrict__ v1_all,
                   const double* __restrict__ w_all, double* __restrict__ res_all, double* __restrict__ Rt_all)
{
    constexpr int NH = NP*(NP + 1)/2, NS = 1 + NP + NH;
    __shared__ double   s_red[FIT_MAX_WAVES][FIT_NSUMS_MAX];
    __shared__ double   s_tot[FIT_NSUMS_MAX];
    __shared__ FitState S;
    const double* __restrict__ v1g = v1_all + (size_t)blockIdx.x*a.v1_stride;
    const double* __restrict__ wg  = w_all != NULL ? w_all + (size_t)blockIdx.x*a.w_stride : NULL;
    double* __restrict__ res = res_all + (size_t)blockIdx.x*FIT_RES_N;
    double* __restrict__ Rt  = Rt_all  + (size_t)blockIdx.x*12;
    const int Npoints = a.M*a.N;

    // the grid points inside the focus region (the reference counts these, whatever their weights), and the cost
    // that rounding alone explains
    {
        double acc[2] = { 0.0, 0.0 };
        for(int idx = threadIdx.x; idx < Npoints; idx += blockDim.x)
        {
            double p0[3], v1[3], w;
            if(idx < a.N)
            {
                const double dx = q0[2*(size_t)idx] - a.fc[0], dy = q0[2*(size_t)idx + 1] - a.fc[1];
                if(dx*dx + dy*dy < a.r2) acc[0] += 1.0;
            }
            if(fit_load_point(p0, v1, &w, a, idx, q0, p0g, v1g, wg)) acc[1] += w*w;
        }
        fit_sum<2>(s_tot, acc, s_red);
        if(threadIdx.x == 0)
        {
            S.nused  = (int)s_tot[0];
            S.floor  = 0.5*FIT_NOISE*FIT_NOISE*s_tot[1];
            S.damp   = { FIT_LAMBDA0, 2.0 };
            S.pred   = 0.0;
            S.F      = 0.0;
            S.nevals = 0;
            for(int k = 0; k < 6; k++) S.rt[k] = S.t[k] = 0.0;
            R_from_r_with_grad(S.R, S.dR, S.t);
            S.done   = S.nused < 3 ? 1 : 0;
            S.status = S.nused < 3 ? FIT_STATUS_TOO_FEW_POINTS : FIT_STATUS_CONVERGED;
        }
        __syncthreads();
    }

    // (the bound is on the loop itself: S.done can only end it sooner)
    for(int eval = 0; eval < FIT_MAX_EVALUATIONS; eval++)
    {
        if(S.done) break;
        double acc[NS];
#pragma unroll
        for(int k = 0; k < NS; k++) acc[k] = 0.0;
        for(int idx = threadIdx.x; idx < Npoints; idx += blockDim.x)
        {
            double p0[3], v1[3], w;
            if(!fit_load_point(p0, v1, &w, a, idx, q0, p0g, v1g, wg)) continue;
            double p[3];
#pragma unroll
            for(int i = 0; i < 3; i++)
            {
                p[i] = S.R[3*i]*p0[0] + S.R[3*i + 1]*p0[1] + S.R[3*i + 2]*p0[2];
                if(NP == 6) p[i] += S.t[3 + i];
            }
            // c = cos of the angle; e = dc/dp
            double c, e[3];
            if(NP == 6)
            {
                const double m = sqrt(p[0]*p[0] + p[1]*p[1] + p[2]*p[2]);
                const double u[3] = { p[0]/m, p[1]/m, p[2]/m };
                c = v1[0]*u[0] + v1[1]*u[1] + v1[2]*u[2];
#pragma unroll
                for(int i = 0; i < 3; i++) e[i] = (v1[i] - c*u[i])/m;
            }
            else
            {
                c = v1[0]*p[0] + v1[1]*p[1] + v1[2]*p[2];
#pragma unroll
                for(int i = 0; i < 3; i++) e[i] = v1[i];
            }
            const double x = 2.0*(1.0 - c)*w;
            double j[NP];
#pragma unroll
            for(int k = 0; k < 3; k++)
            {
                double s = 0.0;
#pragma unroll
                for(int i = 0; i < 3; i++)
                    s += e[i]*(S.dR[9*i + k]*p0[0] + S.dR[9*i + 3 + k]*p0[1] + S.dR[9*i + 6 + k]*p0[2]);
                j[k] = -2.0*w*s;
                if(NP == 6) j[3 + k] = -2.0*w*e[k];
            }
            const double z = x*x/(FIT_C*FIT_C);
            double rho, omega;
            if(z <= 1.0) { rho = z; omega = 1.0; }
            else         { const double sz = sqrt(z); rho = 2.0*sz - 1.0; omega = 1.0/sz; }
            acc[0] += 0.5*FIT_C*FIT_C*rho;
            int ih = 1 + NP;
#pragma unroll
            for(int k = 0; k < NP; k++)
            {
                const double oj = omega*j[k];
                acc[1 + k] += oj*x;
#pragma unroll
                for(int l = k; l < NP; l++, ih++) acc[ih] += oj*j[l];
            }
        }
        fit_sum<NS>(s_tot, acc, s_red);
        if(threadIdx.x == 0) fit_control<NP>(S, s_tot, eval);
        __syncthreads();
    }

    if(threadIdx.x == 0)
    {
        // (the loop's own bound ended it: the last trial was judged, and fit_control() said so)
        for(int k = 0; k < 6; k++) res[k] = k < NP ? S.rt[k] : 0.0;
        res[6] = S.F;
        res[7] = (double)S.nevals;
        res[8] = (double)S.nused;
        res[9] = (double)S.status;
        R_from_r_with_grad(Rt, S.dR, S.rt);
        for(int k = 0; k < 3; k++) Rt[9 + k] = NP == 6 ? S.rt[3 + k] : 0.0;
    }
}

// p[d][n] = v[n] dist[d]
__global__ __launch_bounds__(256)
void pd_scale_kernel(int N, int Nd, const double* __restrict__ v, const double* __restrict__ dist, double* __restrict__ p)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= Nd*N) return;
    const int n = i % N;
    const double d = dist[i / N];
#pragma unroll
    for(int k = 0; k < 3; k++) p[3*(size_t)i + k] = v[3*(size_t)n + k]*d;
}

// w = 1/(u0 u1), squared (model_analysis.py:1822-1829)
__global__ __launch_bounds__(256)
void pd_weights_kernel(int n, const double* __restrict__ u0, const double* __restrict__ u1, double* __restrict__ w)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= n) return;
    const double t = 1.0/(u0[i]*u1[i]);
    w[i] = t*t;
}

// p1[f][i] = R_f p0[i] + t_f;  Rt [Nfits][12]: R row-major, then t
__global__ __launch_bounds__(256)
void pd_transform_kernel(int Nfits, int n, const double* __restrict__ Rt, const double* __restrict__ p0, double* __restrict__ p1)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= Nfits*n) return;
    const double* __restrict__ T = Rt + 12*(size_t)(i / n);
    const double* __restrict__ p = p0 + 3*(size_t)(i % n);
#pragma unroll
    for(int k = 0; k < 3; k++) p1[3*(size_t)i + k] = T[3*k]*p[0] + T[3*k + 1]*p[1] + T[3*k + 2]*p[2] + T[9 + k];
}

// diff[f][d][n] = q1[f][d][n] - q0[n]; difflen[d][n] = sqrt(mean over f of |diff|^2)
__global__ __launch_bounds__(256)
void pd_diff_kernel(int Nfits, int Nd, int N, const double* __restrict__ q1, const double* __restrict__ q0,
                    double* __restrict__ diff, double* __restrict__ difflen)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= Nd*N) return;
    const int n = i % N;
    double s = 0.0;
    for(int f = 0; f < Nfits; f++)
    {
        const size_t o = 2*((size_t)f*Nd*N + i);
        const double dx = q1[o] - q0[2*(size_t)n], dy = q1[o + 1] - q0[2*(size_t)n + 1];
        diff[o] = dx; diff[o + 1] = dy;
        s += dx*dx + dy*dy;
    }
    difflen[i] = sqrt(s/(double)Nfits);
}

// Nfits fits in one launch: fit f takes v1 + f v1_stride and (if any) weights + f w_stride; all share q0 and p0
hipError_t launch_fit(int Nfits, int M, int N, bool atinfinity, const double focus_center[2], double focus_radius,
                      const double* d_q0, const double* d_p0, const double* d_v1, size_t v1_stride,
                      const double* d_w, size_t w_stride, double* d_res, double* d_Rt, hipStream_t stream)
{
    FitArgs a;
    a.M = M; a.N = N;
    a.fc[0] = focus_center[0]; a.fc[1] = focus_center[1];
    a.r2 = focus_radius*focus_radius;
    a.v1_stride = v1_stride; a.w_stride = w_stride;
    // whole waves, as many as there are points to go round, at most FIT_MAX_THREADS
    const int threads = std::max(64, std::min(FIT_MAX_THREADS, (M*N + 63)/64*64));
    if(atinfinity) hipLaunchKernelGGL(pd_fit_kernel<3>, dim3(Nfits), dim3(threads), 0, stream, a, d_q0, d_p0, d_v1, d_w, d_res, d_Rt);
    else           hipLaunchKernelGGL(pd_fit_kernel<6>, dim3(Nfits), dim3(threads), 0, stream, a, d_q0, d_p0, d_v1, d_w, d_res, d_Rt);
    return hipGetLastError();
}

bool fit_sizes_ok(int M, int N)
{
    if(M >= 1 && N >= 1 && (int64_t)M*N <= (int64_t)INT32_MAX/4) return true;
    set_error("implied Rt10: M = %d, N = %d: need M >= 1, N >= 1 and M N < 2^29", M, N);
    return false;
}

} // namespace

struct mrcal_amd_projection_diff
{
    int Nmodels = 0, N = 0;
    std::vector<mrcal_lensmodel_t> lensmodels;
    std::vector<int>               Nintrinsics;
    std::vector<double*>           d_intr;      // [Nmodels] of [Nintrinsics]
    double* d_q0 = NULL;        // [N][2]
    double* d_v  = NULL;        // [Nmodels][N][3], unit vectors
    // sized for capacity distances
    int     capacity = 0;
    double* d_dist    = NULL;   // [Nd]
    double* d_p       = NULL;   // [Nmodels][Nd][N][3]: v d; model 0's are the fit's p0
    double* d_u       = NULL;   // [Nmodels][Nd][N]
    double* d_w       = NULL;   // [Nfits][Nd][N]
    double* d_p1      = NULL;   // [Nfits][Nd][N][3]
    double* d_q1      = NULL;   // [Nfits][Nd][N][2]
    double* d_diff    = NULL;   // [Nfits][Nd][N][2]
    double* d_difflen = NULL;   // [Nd][N]
    double* d_res     = NULL;   // [Nfits][FIT_RES_N]
    double* d_Rt      = NULL;   // [Nfits][12]
    hipStream_t   stream = NULL;
    StageEvents<2> events;                      // around the fit's launch, if asked for
    bool          time_fit = false;
    float         fit_ms = -1.0f;
    DeviceBuffers mem;
    ~mrcal_amd_projection_diff()
    {
        mem.free_all();
        if(stream) hipStreamDestroy(stream);
    }
};

extern "C" {

bool mrcal_amd_implied_rt10(double* rt10, double* cost, int* Nevaluations, int* Nused, int* status,
                            const double* q0, const double* p0, const double* v1, const double* weights,
                            int M, int N, bool atinfinity, const double focus_center[2], double focus_radius)
{
    last_error_string().clear();
    if(!fit_sizes_ok(M, N) || !have_device()) return false;
    DeviceBuffers tmp;
    double *d_q0 = NULL, *d_p0 = NULL, *d_v1 = NULL, *d_w = NULL, *d_res = NULL, *d_Rt = NULL;
    bool ok = tmp.upload(&d_q0, q0, (size_t)2*N) && tmp.upload(&d_p0, p0, (size_t)3*M*N) && tmp.upload(&d_v1, v1, (size_t)3*N) &&
              tmp.alloc(&d_res, FIT_RES_N) && tmp.alloc(&d_Rt, 12);
    if(weights != NULL) ok = ok && tmp.upload(&d_w, weights, (size_t)M*N);
    if(!ok) return false;
    HIP_TRY(launch_fit(1, M, N, atinfinity, focus_center, focus_radius, d_q0, d_p0, d_v1, 0, d_w, 0, d_res, d_Rt, NULL), return false);
    double res[FIT_RES_N];
    HIP_TRY(hipMemcpy(res, d_res, sizeof(res), hipMemcpyDeviceToHost), return false);
    for(int k = 0; k < 6; k++) rt10[k] = res[k];
    if(cost)         *cost         = res[6];
    if(Nevaluations) *Nevaluations = (int)res[7];
    if(Nused)        *Nused        = (int)res[8];
    if(status)       *status       = (int)res[9];
    if((int)res[9] == FIT_STATUS_TOO_FEW_POINTS)
    {
        set_error("Focus region contained too few points");
        return false;
    }
    return true;
}

mrcal_amd_projection_diff_t*
mrcal_amd_projection_diff_create(int Nmodels, const mrcal_lensmodel_t* lensmodels, const double* const* intrinsics,
                                 const double* q0, int N)
{
    last_error_string().clear();
    if(Nmodels < 2) { set_error("At least 2 models are required to compute the diff"); return NULL; }
    if(!fit_sizes_ok(1, N) || !have_device()) return NULL;
    for(int i = 0; i < Nmodels; i++)
    {
        if(!lens_supported((int)lensmodels[i].type))
        {
            set_error("projection diff: lens model %d is not supported", (int)lensmodels[i].type);
            return NULL;
        }
        if(lensmodels[i].type == MRCAL_LENSMODEL_CAHVORE)
            for(int k = 9; k < 12; k++)
                if(intrinsics[i][k] != 0.)
                {
                    set_error("unproject() currently only works with a central projection. So I cannot unproject(CAHVORE,E!=0). Please set E=0 to centralize this model");
                    return NULL;
                }
    }
    mrcal_amd_projection_diff* pd = new mrcal_amd_projection_diff();
    pd->Nmodels = Nmodels; pd->N = N;
    pd->lensmodels.assign(lensmodels, lensmodels + Nmodels);
    pd->d_intr.assign(Nmodels, NULL);
    bool ok = true;
    HIP_TRY(hipStreamCreateWithFlags(&pd->stream, hipStreamNonBlocking), ok = false);
    ok = ok && pd->mem.upload(&pd->d_q0, q0, (size_t)2*N) && pd->mem.alloc(&pd->d_v, (size_t)Nmodels*N*3);
    for(int i = 0; i < Nmodels && ok; i++)
    {
        const int Ni = lensmodel_num_params(lensmodels[i]);
        pd->Nintrinsics.push_back(Ni);
        ok = pd->mem.upload(&pd->d_intr[i], intrinsics[i], (size_t)Ni);
        // (no gradients: no scratch)
        if(ok) HIP_TRY(launch_unproject_points((int)lensmodels[i].type, lens_config_of(lensmodels[i]), N, Ni, pd->d_q0, pd->d_intr[i],
                                               pd->d_v + (size_t)i*N*3, NULL, NULL, NULL, NULL, NULL, true, pd->stream), ok = false);
    }
    if(ok) HIP_TRY(hipStreamSynchronize(pd->stream), ok = false);
    if(!ok) { delete pd; return NULL; }
    return pd;
}

void mrcal_amd_projection_diff_destroy(mrcal_amd_projection_diff_t* pd) { delete pd; }

double mrcal_amd_projection_diff_time_fit(mrcal_amd_projection_diff_t* pd, bool on)
{
    if(pd == NULL) return -1.0;
    const double last = (double)pd->fit_ms;
    pd->time_fit = on;
    pd->fit_ms = -1.0f;
    return last;
}

bool mrcal_amd_projection_diff_evaluate(mrcal_amd_projection_diff_t* pd,
                                        const double* distances, int Ndistances, bool atinfinity,
                                        mrcal_amd_uncertainty_t* const* uncertainties,
                                        bool fit, const double focus_center[2], double focus_radius,
                                        double* Rt10, double* rt10, double* cost, int* Nevaluations, int* Nused, int* status,
                                        double* difflen, double* diff)
{
    last_error_string().clear();
    if(pd == NULL) { set_error("no projection-diff context"); return false; }
    const int N = pd->N, Nd = Ndistances, Nmodels = pd->Nmodels, Nfits = Nmodels - 1;
    if(!fit_sizes_ok(Nd, N)) return false;
    const size_t DN = (size_t)Nd*N;
    hipStream_t st = pd->stream;
    if(pd->capacity < Nd)
    {
        double** all[] = { &pd->d_dist, &pd->d_p, &pd->d_u, &pd->d_w, &pd->d_p1, &pd->d_q1, &pd->d_diff, &pd->d_difflen, &pd->d_res, &pd->d_Rt };
        for(double** b : all) pd->mem.release(b);
        pd->capacity = 0;
        if(!(pd->mem.alloc(&pd->d_dist, (size_t)Nd) && pd->mem.alloc(&pd->d_p, Nmodels*DN*3) && pd->mem.alloc(&pd->d_u, Nmodels*DN) &&
             pd->mem.alloc(&pd->d_w, Nfits*DN) && pd->mem.alloc(&pd->d_p1, Nfits*DN*3) && pd->mem.alloc(&pd->d_q1, Nfits*DN*2) &&
             pd->mem.alloc(&pd->d_diff, Nfits*DN*2) && pd->mem.alloc(&pd->d_difflen, DN) &&
             pd->mem.alloc(&pd->d_res, (size_t)Nfits*FIT_RES_N) && pd->mem.alloc(&pd->d_Rt, (size_t)Nfits*12)))
            return false;
        pd->capacity = Nd;
    }
    const dim3 block(256), grid_dn((unsigned)((DN + 255)/256));
    HIP_TRY(hipMemcpyAsync(pd->d_dist, distances, (size_t)Nd*sizeof(double), hipMemcpyHostToDevice, st), return false);
    const bool weighted = fit && uncertainties != NULL;
    for(int i = 0; i < (weighted ? Nmodels : 1); i++)
        hipLaunchKernelGGL(pd_scale_kernel, grid_dn, block, 0, st, N, Nd, pd->d_v + (size_t)i*N*3, pd->d_dist, pd->d_p + i*DN*3);
    HIP_TRY(hipGetLastError(), return false);
    if(weighted)
    {
        for(int i = 0; i < Nmodels; i++)
            if(!uncertainty_evaluate_device(uncertainties[i], pd->d_p + i*DN*3, (int)DN, atinfinity,
                                            MRCAL_AMD_UNCERTAINTY_WORSTDIRECTION_STDEV, pd->d_u + i*DN, st))
                return false;
        for(int f = 0; f < Nfits; f++)
            hipLaunchKernelGGL(pd_weights_kernel, grid_dn, block, 0, st, (int)DN, pd->d_u, pd->d_u + (f + 1)*DN, pd->d_w + f*DN);
        HIP_TRY(hipGetLastError(), return false);
    }
    if(fit)
    {
        if(pd->time_fit)
        {
            // (made when first asked for)
            if(!pd->events.create() || !pd->events.record(0, st)) return false;
        }
        HIP_TRY(launch_fit(Nfits, Nd, N, atinfinity, focus_center, focus_radius, pd->d_q0, pd->d_p, pd->d_v + (size_t)N*3, (size_t)N*3,
                           weighted ? pd->d_w : NULL, DN, pd->d_res, pd->d_Rt, st), return false);
        if(pd->time_fit && !pd->events.record(1, st)) return false;
        // the verdicts before anything else is queued: too few points is the caller's exception
        std::vector<double> res((size_t)Nfits*FIT_RES_N);
        HIP_TRY(hipMemcpyAsync(res.data(), pd->d_res, res.size()*sizeof(double), hipMemcpyDeviceToHost, st), return false);
        HIP_TRY(hipMemcpyAsync(Rt10, pd->d_Rt, (size_t)Nfits*12*sizeof(double), hipMemcpyDeviceToHost, st), return false);
        HIP_TRY(hipStreamSynchronize(st), return false);
        if(pd->time_fit && !pd->events.elapsed(&pd->fit_ms, 0, 1)) return false;
        bool too_few = false;
        for(int f = 0; f < Nfits; f++)
        {
            const double* r = &res[(size_t)f*FIT_RES_N];
            if(rt10)         for(int k = 0; k < 6; k++) rt10[6*f + k] = r[k];
            if(cost)         cost[f]         = r[6];
            if(Nevaluations) Nevaluations[f] = (int)r[7];
            if(Nused)        Nused[f]        = (int)r[8];
            if(status)       status[f]       = (int)r[9];
            too_few = too_few || (int)r[9] == FIT_STATUS_TOO_FEW_POINTS;
        }
        if(too_few) { set_error("Focus region contained too few points"); return false; }
    }
    else
        HIP_TRY(hipMemcpyAsync(pd->d_Rt, Rt10, (size_t)Nfits*12*sizeof(double), hipMemcpyHostToDevice, st), return false);

    hipLaunchKernelGGL(pd_transform_kernel, dim3((unsigned)((Nfits*DN + 255)/256)), block, 0, st, Nfits, (int)DN, pd->d_Rt, pd->d_p, pd->d_p1);
    HIP_TRY(hipGetLastError(), return false);
    for(int f = 0; f < Nfits; f++)
        HIP_TRY(launch_project_points((int)pd->lensmodels[f + 1].type, lens_config_of(pd->lensmodels[f + 1]), (int)DN, pd->Nintrinsics[f + 1],
                                      pd->d_p1 + f*DN*3, pd->d_intr[f + 1], pd->d_q1 + f*DN*2, NULL, NULL, st), return false);
    hipLaunchKernelGGL(pd_diff_kernel, grid_dn, block, 0, st, Nfits, Nd, N, pd->d_q1, pd->d_q0, pd->d_diff, pd->d_difflen);
    HIP_TRY(hipGetLastError(), return false);
    HIP_TRY(hipMemcpyAsync(difflen, pd->d_difflen, DN*sizeof(double), hipMemcpyDeviceToHost, st), return false);
    if(diff != NULL) HIP_TRY(hipMemcpyAsync(diff, pd->d_diff, Nfits*DN*2*sizeof(double), hipMemcpyDeviceToHost, st), return false);
    HIP_TRY(hipStreamSynchronize(st), return false);
    return true;
}

} // extern "C"
