// The lens-model fit (include/mrcal_amd.h, "lens-model fit"): the sampled problem of the reference's
// mrcal-convert-lensmodel (:725-792) as mrcal_optimize() sees it - fixed points, the intrinsics of ONE parametric model
// and, in a second stage, the pose rt_cam_ref as unknowns - minimised on the device, every start of a call in one launch.
//
//   x = w_i (project(T p_i) - q_i)  two rows a point,  + the regularization rows of mrcal.c:5655-5901
//   F = x.x,  H = J^T J,  g = J^T x,  (H + lambda diag(H)) d = -g,  a trial kept only if F does not rise
//
// lensfit_kernel<PROJ,NDIST>  ONE trial a workgroup (blockIdx.x: which), both stages and every iteration inside the
//   launch. pd_fit_kernel (projection_diff.hip) keeps the 28 sums of its 6 unknowns in a thread's registers; with up
//   to 22 unknowns there are 276, so the sums are turned round: a chunk of C rows of [J x] is staged in LDS (a lane
//   forms the two rows of a point through project_lens<PROJ,NDIST,true> and R, dR/dr of the trial pose), then a
//   thread owns ONE entry of the upper triangle of [J x]^T [J x] - an entry of H, of g, or F itself - and sums down the
//   chunk's rows in order. Where the threads outnumber the entries, the rows are dealt to `slices` threads an entry
//   (row r to slice r mod slices) and the slices are added in order at the end. No cross-lane reduction, no
//   floating-point atomics: the same bits on every call, and for a trial alone or among others.
//   Thread 0 adds the regularization rows, factors H (+ lambda diag H) from LDS, accepts or rejects, moves lambda,
//   decides termination and publishes the next trial; every thread takes the same branch at every barrier.
//
// The planning - which instantiation, the unknowns, threads, C, LDS, refusals - is host code: lensfit_plan.hpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <float.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "layout.hpp"
#include "host_state.hpp"
#include "lens_models.hpp"
#include "lens_dispatch.hpp"
#include "device_math.hpp"
#include "damped_newton.hpp"
#include "device_memory.hpp"
#include "resident_common.hpp"
#include "lensfit_plan.hpp"
#include "../../include/mrcal_amd.h"

using namespace mrcal_amd;

namespace {

constexpr int    LF_THREADS_MAX = 320;      // lensfit_num_sums(22) = 276, in whole waves
constexpr int    LF_NI_MAX      = 16;       // OPENCV12
constexpr int    LF_NP_MAX      = LENSFIT_NP_MAX;
constexpr int    LF_NH_MAX      = LF_NP_MAX*(LF_NP_MAX + 1)/2;
constexpr int    LF_NE_MAX      = (LF_NP_MAX + 1)*(LF_NP_MAX + 2)/2;
// A stage starts far from its minimum - distortion terms seeded at 1e-3 or less, a pose left out of stage 1 - and the
// rational models have more than one basin: the nearly undamped first steps of lambda = 1e-3 took OPENCV8 with a pose to
// a minimum of 0.06 px on data the truth fits exactly. From lambda = 1 (half the Gauss-Newton step where the problem is
// well scaled; lambda falls to a third with every step that pays) it ends at the truth, for about six evaluations more
constexpr double LF_LAMBDA0     = 1.0;
constexpr double LF_LAMBDA_MIN  = 1e-15;
constexpr double LF_LAMBDA_MAX  = 1e10;     // beyond it a step is < 1e-10 of the Gauss-Newton step: no descent to be had
constexpr double LF_LAMBDA_GN   = 1.0;      // up to here a step is at least half the Gauss-Newton step: what it gains, or
                                            // is promised, says something about how far the minimum is
constexpr double LF_FTOL        = 1e-12;    // a step that gains, or is promised, less than this part of F ends the fit
// A projection to a pixel q rounds at a few ulps of |q| (1e-12 px at q = 2000), and so does x_i/w_i. A cost at or below
// sum w_i^2 (64 eps)^2 (|q_i|^2 + 1) is a perfect fit as far as doubles can tell: steps from there follow the rounding
constexpr double LF_NOISE       = 64.0*DBL_EPSILON;
// what a trial writes: intrinsics (16), rt (6), F, rms, evaluations, status, points used
constexpr int    LF_RES_N       = 28;

struct LfArgs
{
    int    N, ivar0, Nstages, NP[2], C, max_evals, Nmeasurements;
    bool   have_w, have_rt;
    double reg_distortion[12];      // the scale of each term's row; all 0: none
    double reg_center;              // 0: none
    double center_target[2];
    LensConfig cfg;
};

struct LfState
{
    double intr[LF_NI_MAX], rt[6];          // the best point so far
    double tintr[LF_NI_MAX], trt[6];        // the trial the threads evaluate
    double R[9], dR[27];                    // of trt
    double F;
    Damping damp;
    double pred, floor;
    double g[LF_NP_MAX], H[LF_NH_MAX];      // at the best point: the upper triangle row by row
    double L[LF_NP_MAX][LF_NP_MAX], d[LF_NP_MAX];
    double tot[LF_NE_MAX];                  // the sums of the evaluation just made
    int    done, status, nevals, nused, failed;
};
static_assert(sizeof(LfState) + LF_THREADS_MAX*sizeof(double) <= LENSFIT_STATE_LDS_BYTES, "the plan's LENSFIT_STATE_LDS_BYTES is too small");

// One point, sanitised: false if it takes no part (weight <= 0, or anything non-finite)
__device__ __forceinline__
bool lf_load_point(double* p, double* q, double* w, const LfArgs& a, int idx,
                   const double* __restrict__ pg, const double* __restrict__ qg, const double* __restrict__ wg)
{
    double ww = a.have_w ? wg[idx] : 1.0;
    bool ok = isfinite(ww) && ww > 0.0;
#pragma unroll
    for(int k = 0; k < 3; k++) { p[k] = pg[3*(size_t)idx + k]; ok = ok && isfinite(p[k]); }
#pragma unroll
    for(int k = 0; k < 2; k++) { q[k] = qg[2*(size_t)idx + k]; ok = ok && isfinite(q[k]); }
    *w = ww;
    return ok;
}

// Thread 0, after evaluation number eval of this stage (0: its start) summed S.tot = [J x]^T [J x] at the trial: the
// regularization rows, keep the trial or not, lambda, termination, the next trial
template<int NI>
__device__
void lf_control(LfState& S, const LfArgs& a, int NP, bool pose, int eval)
{
    const int NIa = NI - a.ivar0;           // active intrinsics: columns [0, NIa); the pose behind them
    const int cdist = 4 - a.ivar0;          // column of the first distortion term
    double Fn = S.tot[(NP + 1)*(NP + 2)/2 - 1];
    for(int j = 0; j < NI - 4; j++)
    {
        const double xr = a.reg_distortion[j]*S.tintr[4 + j];
        Fn += xr*xr;
    }
    if(a.reg_center != 0.0)
        for(int k = 0; k < 2; k++)
        {
            const double xr = a.reg_center*(S.tintr[2 + k] - a.center_target[k]);
            Fn += xr*xr;
        }

    bool done = false;
    int status = LENSFIT_CONVERGED;
    if(eval == 0 || Fn <= S.F)
    {
        const double dF = eval == 0 ? 0.0 : S.F - Fn;
        for(int k = 0; k < NI; k++) S.intr[k] = S.tintr[k];
        for(int k = 0; k < 6;  k++) S.rt[k]   = S.trt[k];
        int it = 0, ih = 0;
        for(int i = 0; i < NP; i++)
            for(int j = i; j <= NP; j++, it++)
            {
                if(j < NP) S.H[ih++] = S.tot[it];
                else       S.g[i]    = S.tot[it];
            }
        for(int j = 0; j < NI - 4; j++)
        {
            const int c = cdist + j;
            const double s = a.reg_distortion[j];
            S.H[packed_diagonal(c, NP)] += s*s;
            S.g[c] += s*(s*S.tintr[4 + j]);
        }
        if(a.reg_center != 0.0)
            for(int k = 0; k < 2; k++)
            {
                const int c = 2 + k;
                S.H[packed_diagonal(c, NP)] += a.reg_center*a.reg_center;
                S.g[c] += a.reg_center*(a.reg_center*(S.tintr[2 + k] - a.center_target[k]));
            }
        S.F = Fn;
        double gmax = 0.0;
        bool gfinite = true;
        for(int k = 0; k < NP; k++) { gmax = fmax(gmax, fabs(S.g[k])); gfinite = gfinite && isfinite(S.g[k]); }
        const double lambda_used = S.damp.lambda;
        if(eval > 0) S.damp.accepted(dF, S.pred, LF_LAMBDA_MIN);
        if(!isfinite(Fn) || !gfinite)              { done = true; status = LENSFIT_STALLED; S.failed = 1; }
        else if(Fn <= S.floor || gmax == 0.0)      done = true;
        else if(eval > 0 && dF <= LF_FTOL*Fn && lambda_used <= LF_LAMBDA_GN) done = true;
    }
    else S.damp.rejected();
    if(!done && eval + 1 >= a.max_evals) { done = true; status = LENSFIT_BOUND; }

    while(!done)
    {
        if(!(S.damp.lambda <= LF_LAMBDA_MAX)) { done = true; status = LENSFIT_STALLED; break; }
        double pred;
        bool ok = damped_step<true>(S.L, S.d, &pred, S.H, S.g, NP, S.damp.lambda);
        if(ok)
        {
            // F = x.x: what the step promises, as it stands
            S.pred = pred;
            for(int k = 0; k < NP; k++) ok = ok && isfinite(S.d[k]);
            if(ok && pred <= LF_FTOL*S.F && S.damp.lambda <= LF_LAMBDA_GN) { done = true; break; }
        }
        if(ok) break;
        S.damp.rejected();
    }
    if(!done)
    {
        for(int k = 0; k < NIa; k++) S.tintr[a.ivar0 + k] = S.intr[a.ivar0 + k] + S.d[k];
        if(pose)
        {
            for(int k = 0; k < 6; k++) S.trt[k] = S.rt[k] + S.d[NIa + k];
            R_from_r_with_grad(S.R, S.dR, S.trt);
        }
    }
    S.done   = done ? 1 : 0;
    S.status = status;
    S.nevals++;
}

template<int PROJ, int NDIST>
__global__ __launch_bounds__(LF_THREADS_MAX)
void lensfit_kernel(LfArgs a, const double* __restrict__ pg, const double* __restrict__ qg, const double* __restrict__ wg,
                    const double* __restrict__ intr_seed, const double* __restrict__ rt_seed, double* __restrict__ res_all)
{
    constexpr int NI = 4 + NDIST;
    extern __shared__ double s_rows[];                  // [C][W] of the stage: the active columns of J, then x
    __shared__ LfState S;
    __shared__ double  s_part[LF_THREADS_MAX];
    const int tid = threadIdx.x, T = blockDim.x, N = a.N;
    double* __restrict__ res = res_all + (size_t)blockIdx.x*LF_RES_N;

    // the points that take part, and the cost that rounding alone explains. Every thread its points in order, then
    // thread 0 the threads in order
    {
        double cnt = 0.0, fl = 0.0;
        for(int idx = tid; idx < N; idx += T)
        {
            double p[3], q[2], w;
            if(lf_load_point(p, q, &w, a, idx, pg, qg, wg)) { cnt += 1.0; fl += w*w*(q[0]*q[0] + q[1]*q[1] + 1.0); }
        }
        s_part[tid] = cnt;
        __syncthreads();
        if(tid == 0) { double s = 0.0; for(int k = 0; k < T; k++) s += s_part[k]; S.nused = (int)s; }
        __syncthreads();
        s_part[tid] = fl;
        __syncthreads();
        if(tid == 0)
        {
            double s = 0.0; for(int k = 0; k < T; k++) s += s_part[k];
            S.floor  = LF_NOISE*LF_NOISE*s;
            S.F      = 0.0;
            S.nevals = 0;
            S.failed = 0;
            S.done   = 1;
            S.status = LENSFIT_CONVERGED;
            for(int k = 0; k < NI; k++) S.intr[k] = S.tintr[k] = intr_seed[(size_t)blockIdx.x*NI + k];
            for(int k = 0; k < 6;  k++) S.rt[k] = S.trt[k] = 0.0;
        }
    }

    for(int stage = 0; stage < a.Nstages; stage++)
    {
        const int  NP   = a.NP[stage];
        const bool pose = stage == 1;
        if(NP == 0) continue;
        // (everybody has read the verdict of the stage before)
        __syncthreads();
        if(tid == 0)
        {
            if(pose)
                for(int k = 0; k < 6; k++) S.rt[k] = a.have_rt ? rt_seed[(size_t)blockIdx.x*6 + k] : 0.0;
            for(int k = 0; k < NI; k++) S.tintr[k] = S.intr[k];
            for(int k = 0; k < 6;  k++) S.trt[k]   = S.rt[k];
            R_from_r_with_grad(S.R, S.dR, S.trt);
            S.damp   = { LF_LAMBDA0, 2.0 };
            S.pred   = 0.0;
            if(S.failed) S.done = 1;
            else if(2*S.nused < NP) { S.done = 1; S.status = LENSFIT_TOO_FEW_POINTS; S.failed = 1; S.F = NAN; }
            else S.done = 0;
        }
        __syncthreads();

        // the entry (ci,cj) of the upper triangle of [J x]^T [J x] this thread sums, and its share of the rows
        const int W = NP + 1, NE = (NP + 1)*(NP + 2)/2, slices = T/NE;
        const int slice = tid/NE;
        const bool summing = slice < slices;
        int ci = 0, cj;
        {
            int k = tid - slice*NE;
            while(k >= W - ci) { k -= W - ci; ci++; }
            cj = ci + k;
        }
        const int cdist = 4 - a.ivar0, cpose = NI - a.ivar0;

        // (the bound is on the loop itself: S.done can only end it sooner)
        for(int eval = 0; eval < a.max_evals; eval++)
        {
            if(S.done) break;
            double acc = 0.0;
            for(int base = 0; base < N; base += a.C/2)
            {
                if(tid < a.C/2)
                {
                    double* __restrict__ r0 = s_rows + (size_t)(2*tid)*W;
                    double* __restrict__ r1 = r0 + W;
                    const int idx = base + tid;
                    double p[3], qo[2], w;
                    if(idx < N && lf_load_point(p, qo, &w, a, idx, pg, qg, wg))
                    {
                        double intr[NI];
#pragma unroll
                        for(int k = 0; k < NI; k++) intr[k] = S.tintr[k];
                        double pc[3];
                        if(pose)
                        {
#pragma unroll
                            for(int i = 0; i < 3; i++) pc[i] = S.R[3*i]*p[0] + S.R[3*i + 1]*p[1] + S.R[3*i + 2]*p[2] + S.trt[3 + i];
                        }
                        else
                        {
#pragma unroll
                            for(int i = 0; i < 3; i++) pc[i] = p[i];
                        }
                        double qq[2], g[2][3], gk[2][NDIST > 0 ? NDIST : 1];
                        // (false: CAHVORE's Newton solve found no root, and q and every gradient come back 0
                        //  (lens_models.hpp). The point stays in the sums as the reference keeps it: x = w (0 - q), the
                        //  focal lengths' and the distortions' columns 0, the centre pixel's w)
                        const bool ok = project_lens<PROJ,NDIST,true>(qq, g, gk, pc, intr, a.cfg);
                        if(a.ivar0 == 0)
                        {
                            // q = f u + c
                            r0[0] = ok ? w*((qq[0] - intr[2])/intr[0]) : 0.0;  r0[1] = 0.0;  r0[2] = w;    r0[3] = 0.0;
                            r1[0] = 0.0;  r1[1] = ok ? w*((qq[1] - intr[3])/intr[1]) : 0.0;  r1[2] = 0.0;  r1[3] = w;
                        }
#pragma unroll
                        for(int k = 0; k < NDIST; k++) { r0[cdist + k] = w*gk[0][k]; r1[cdist + k] = w*gk[1][k]; }
                        if(pose)
                        {
#pragma unroll
                            for(int k = 0; k < 3; k++)
                            {
                                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                                for(int i = 0; i < 3; i++)
                                {
                                    const double dpc = S.dR[9*i + k]*p[0] + S.dR[9*i + 3 + k]*p[1] + S.dR[9*i + 6 + k]*p[2];
                                    s0 += g[0][i]*dpc;
                                    s1 += g[1][i]*dpc;
                                }
                                r0[cpose + k]     = w*s0;       r1[cpose + k]     = w*s1;
                                r0[cpose + 3 + k] = w*g[0][k];  r1[cpose + 3 + k] = w*g[1][k];
                            }
                        }
                        r0[NP] = w*(qq[0] - qo[0]);
                        r1[NP] = w*(qq[1] - qo[1]);
                    }
                    else
                        for(int k = 0; k < W; k++) r0[k] = r1[k] = 0.0;
                }
                __syncthreads();
                if(summing)
                {
                    const int nrows = 2*min(a.C/2, N - base);
                    const double* __restrict__ ri = s_rows + ci;
                    const double* __restrict__ rj = s_rows + cj;
                    for(int r = slice; r < nrows; r += slices) acc += ri[(size_t)r*W]*rj[(size_t)r*W];
                }
                __syncthreads();
            }
            s_part[tid] = summing ? acc : 0.0;
            __syncthreads();
            if(tid < NE)
            {
                double s = s_part[tid];
                for(int k = 1; k < slices; k++) s += s_part[k*NE + tid];
                S.tot[tid] = s;
            }
            __syncthreads();
            if(tid == 0) lf_control<NI>(S, a, NP, pose, eval);
            __syncthreads();
        }
    }

    __syncthreads();
    if(tid == 0)
    {
        for(int k = 0; k < LF_NI_MAX; k++) res[k] = k < NI ? S.intr[k] : 0.0;
        for(int k = 0; k < 6; k++) res[LF_NI_MAX + k] = S.rt[k];
        res[22] = S.F;
        res[23] = sqrt(S.F/(double)a.Nmeasurements);
        res[24] = (double)S.nevals;
        res[25] = (double)S.status;
        res[26] = (double)S.nused;
        res[27] = 0.0;
    }
}

} // namespace

struct mrcal_amd_lensfit
{
    int     capN = 0, capT = 0;
    double* d_p = NULL;         // [N][3]
    double* d_q = NULL;         // [N][2]
    double* d_w = NULL;         // [N]
    double* d_seed = NULL;      // [Ntrials][16]: a trial's Nintrinsics, packed
    double* d_rt   = NULL;      // [Ntrials][6]
    double* d_res  = NULL;      // [Ntrials][LF_RES_N]
    hipStream_t   stream = NULL;
    StageEvents<2> events;      // around the fit's launch
    float         fit_ms = -1.0f;
    DeviceBuffers mem;
    ~mrcal_amd_lensfit()
    {
        mem.free_all();
        if(stream) hipStreamDestroy(stream);
    }
};

extern "C" {

mrcal_amd_lensfit_t* mrcal_amd_lensfit_create(void)
{
    last_error_string().clear();
    if(!have_device()) return NULL;
    mrcal_amd_lensfit* lf = new mrcal_amd_lensfit();
    HIP_TRY(hipStreamCreateWithFlags(&lf->stream, hipStreamNonBlocking), delete lf; return NULL);
    if(!lf->events.create()) { delete lf; return NULL; }
    return lf;
}

void mrcal_amd_lensfit_destroy(mrcal_amd_lensfit_t* lf) { delete lf; }

bool mrcal_amd_lensfit_plan(int* plan_out, const mrcal_lensmodel_t* lensmodel, int N, int Ntrials, const int imagersize[2],
                            bool optimize_core, bool optimize_extrinsics, bool apply_regularization)
{
    last_error_string().clear();
    LensfitPlan plan;
    std::string why;
    if(!lensfit_plan(&plan, &why, *lensmodel, N, Ntrials, imagersize, optimize_core, optimize_extrinsics, apply_regularization))
    {
        set_error("%s", why.c_str());
        return false;
    }
    const int out[MRCAL_AMD_LENSFIT_PLAN_N] = { plan.proj, plan.ndist, plan.Nintrinsics, plan.ivar0, plan.Nstages, plan.NP[0], plan.NP[1],
                                                plan.NE, plan.threads, plan.row_doubles, plan.chunk_rows, (int)plan.lds_bytes,
                                                plan.Nmeasurements, LENSFIT_LDS_BYTES };
    for(int k = 0; k < MRCAL_AMD_LENSFIT_PLAN_N; k++) plan_out[k] = out[k];
    return true;
}

double mrcal_amd_lensfit_last_ms(const mrcal_amd_lensfit_t* lf) { return lf == NULL ? -1.0 : (double)lf->fit_ms; }

bool mrcal_amd_lensfit_fit(mrcal_amd_lensfit_t* lf,
                           const double* p, const double* q, const double* w, int N,
                           const mrcal_lensmodel_t* lensmodel, const int imagersize[2],
                           const double* intrinsics_seed, const double* rt_seed, int Ntrials,
                           bool optimize_core, bool optimize_extrinsics, bool apply_regularization, int max_evaluations,
                           double* intrinsics, double* rt, double* cost, double* rms, int* Nevaluations, int* status,
                           int* ibest)
{
    last_error_string().clear();
    if(lf == NULL) { set_error("no lens-fit context"); return false; }
    if(p == NULL || q == NULL || lensmodel == NULL || imagersize == NULL || intrinsics_seed == NULL)
    {
        set_error("lens-model fit: p, q, the lens model, the imager size and the seeds are required");
        return false;
    }
    LensfitPlan plan;
    std::string why;
    if(!lensfit_plan(&plan, &why, *lensmodel, N, Ntrials, imagersize, optimize_core, optimize_extrinsics, apply_regularization))
    {
        set_error("%s", why.c_str());
        return false;
    }
    if(max_evaluations < 0) { set_error("lens-model fit: max_evaluations = %d", max_evaluations); return false; }
    const int NI = plan.Nintrinsics;

    if(lf->capN < N)
    {
        double** all[] = { &lf->d_p, &lf->d_q, &lf->d_w };
        for(double** b : all) lf->mem.release(b);
        lf->capN = 0;
        if(!(lf->mem.alloc(&lf->d_p, (size_t)3*N) && lf->mem.alloc(&lf->d_q, (size_t)2*N) && lf->mem.alloc(&lf->d_w, (size_t)N))) return false;
        lf->capN = N;
    }
    if(lf->capT < Ntrials)
    {
        double** all[] = { &lf->d_seed, &lf->d_rt, &lf->d_res };
        for(double** b : all) lf->mem.release(b);
        lf->capT = 0;
        if(!(lf->mem.alloc(&lf->d_seed, (size_t)LF_NI_MAX*Ntrials) && lf->mem.alloc(&lf->d_rt, (size_t)6*Ntrials) &&
             lf->mem.alloc(&lf->d_res, (size_t)LF_RES_N*Ntrials))) return false;
        lf->capT = Ntrials;
    }
    hipStream_t st = lf->stream;
    HIP_TRY(hipMemcpyAsync(lf->d_p, p, (size_t)3*N*sizeof(double), hipMemcpyHostToDevice, st), return false);
    HIP_TRY(hipMemcpyAsync(lf->d_q, q, (size_t)2*N*sizeof(double), hipMemcpyHostToDevice, st), return false);
    if(w != NULL) HIP_TRY(hipMemcpyAsync(lf->d_w, w, (size_t)N*sizeof(double), hipMemcpyHostToDevice, st), return false);
    HIP_TRY(hipMemcpyAsync(lf->d_seed, intrinsics_seed, (size_t)NI*Ntrials*sizeof(double), hipMemcpyHostToDevice, st), return false);
    const bool have_rt = optimize_extrinsics && rt_seed != NULL;
    if(have_rt) HIP_TRY(hipMemcpyAsync(lf->d_rt, rt_seed, (size_t)6*Ntrials*sizeof(double), hipMemcpyHostToDevice, st), return false);

    LfArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.ivar0 = plan.ivar0; a.Nstages = plan.Nstages; a.NP[0] = plan.NP[0]; a.NP[1] = plan.NP[1];
    a.C = plan.chunk_rows;
    a.max_evals = max_evaluations == 0 ? LENSFIT_DEFAULT_MAX_EVALUATIONS : max_evaluations;
    a.Nmeasurements = plan.Nmeasurements;
    a.have_w = w != NULL; a.have_rt = have_rt;
    for(int j = 0; j < plan.Nreg_distortion; j++) a.reg_distortion[j] = lensfit_distortion_scale((int)lensmodel->type, j);
    if(plan.Nreg_centerpixel > 0)
    {
        a.reg_center = lensfit_centerpixel_scale(imagersize);
        for(int k = 0; k < 2; k++) a.center_target[k] = 0.5*(double)(imagersize[k] - 1);
    }
    a.cfg = lens_config_of(*lensmodel);

    if(!lf->events.record(0, st)) return false;
    for_parametric_lens((int)lensmodel->type, [&](auto k)
    {
        using K = decltype(k);
        hipLaunchKernelGGL((lensfit_kernel<K::PROJ, K::NDIST>), dim3(Ntrials), dim3(plan.threads), plan.rows_lds_bytes, st,
                           a, lf->d_p, lf->d_q, lf->d_w, lf->d_seed, lf->d_rt, lf->d_res);
    });
    HIP_TRY(hipGetLastError(), return false);
    if(!lf->events.record(1, st)) return false;
    std::vector<double> res((size_t)Ntrials*LF_RES_N);
    HIP_TRY(hipMemcpyAsync(res.data(), lf->d_res, res.size()*sizeof(double), hipMemcpyDeviceToHost, st), return false);
    HIP_TRY(hipStreamSynchronize(st), return false);
    if(!lf->events.elapsed(&lf->fit_ms, 0, 1)) return false;

    // the best trial: the lowest rms among those that did not fail, the first of equals
    int best = -1;
    for(int t = 0; t < Ntrials; t++)
    {
        const double* r = &res[(size_t)t*LF_RES_N];
        if(intrinsics)   for(int k = 0; k < NI; k++) intrinsics[(size_t)t*NI + k] = r[k];
        if(rt)           for(int k = 0; k < 6; k++)  rt[(size_t)t*6 + k] = r[LF_NI_MAX + k];
        if(cost)         cost[t]         = r[22];
        if(rms)          rms[t]          = r[23];
        if(Nevaluations) Nevaluations[t] = (int)r[24];
        if(status)       status[t]       = (int)r[25];
        if((int)r[25] == LENSFIT_TOO_FEW_POINTS || !isfinite(r[23])) continue;
        if(best < 0 || r[23] < res[(size_t)best*LF_RES_N + 23]) best = t;
    }
    if(ibest) *ibest = best;
    return true;
}

} // extern "C"
