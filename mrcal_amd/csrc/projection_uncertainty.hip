// Projection uncertainty (mrcal.projection_uncertainty(), mrcal/model_analysis.py:1192-1517) with the propagation
// resident on the device: the cross-reprojection methods "cross-reprojection-ccp" (model_analysis.py:1347-1393) and
// "cross-reprojection-rrp-Jfp" (:873-936, 1040-1090), in packed units throughout.
//
// For both methods the gradient of a projection with respect to the packed state is a fixed linear map of a small
// per-point matrix:
//
//   dq/db*(p) = G(p) M       G (2 x k): [ dq/dintrinsics | dq/dpcam dpcam/drt_cam_ref (rrp) | dq/dpref skew(pref) | -dq/dpref ]
//                            M (k x Nstate): the unit rows of this camera's optimized intrinsics (and, rrp, of its
//                            extrinsics) times their scales; then K = drt_cross_reprojection__dbpacked() as it comes
//
// so Var(q) = sigma^2 G C G^T with ONE k x k matrix per (model, method). _propagate_calibration_uncertainty()
// (model_analysis.py:560-870) with J*[obs]^T J*[obs] = J*^T J* - J*[reg]^T J*[reg] (its own derivation, :645-660) gives
//
//   X = (J*^T J*)^-1 M^T          (Nstate x k: k right-hand sides on the resident factorization)
//   C = M X - (J*[reg] X)^T (J*[reg] X)
//
// which reads only the few regularization rows of J (without regularization the second term is empty, the
// reference's "simplified expression"). The solve, the K rows of M X, J*[reg] X and the combination are
// noise_propagation.hpp's steps. Kernels of this file:
//   pu_rhs_kernel         M, written into the solve's right-hand sides (no copy of size Nstate crosses PCIe but K)
//   pu_MX_kernel          M X: a unit row's entries are picked out of X and scaled, a K row's are its dot products
//   pu_points_kernel      a wavefront a point: the projection with gradients through lens_models.hpp, one nonzero
//                         entry of G a lane (a splined model's G has only the core, the (order+1)^2 patch of each
//                         image row and the pose columns), G C G^T by shuffles, C in LDS when it fits
// Nothing uses floating-point atomics: every result is the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include <memory>
#include "layout.hpp"
#include "host_state.hpp"
#include "problem_object.hpp"
#include "analysis_plan.hpp"
#include "noise_propagation.hpp"
#include "lens_models.hpp"
#include "lens_dispatch.hpp"
#include "device_math.hpp"
#include "wave_sum.hpp"
#include "../../include/mrcal_amd.h"

using namespace mrcal_amd;

namespace {

constexpr int PU_WAVES = 4;             // wavefronts (= points at a time) in a workgroup of the per-point kernel
constexpr int PU_LDS_C_MAX = 6144;      // C (k^2 doubles) in LDS up to 48 KB: k <= 78

// the rows of M: a unit row (col >= 0) times scale, or row -col-1 of K
__global__ __launch_bounds__(256)
void pu_rhs_kernel(int k, int Nstate, const int* __restrict__ col, const double* __restrict__ scale,
                   const double* __restrict__ K, double* __restrict__ rhs)
{
    const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= (int64_t)k*Nstate) return;
    const int a = (int)(i / Nstate), s = (int)(i % Nstate);
    const int c = col[a];
    rhs[i] = c >= 0 ? (s == c ? scale[a] : 0.0) : K[(size_t)(-c-1)*Nstate + s];
}

// MX[a][b], M's row a times X's column b: a unit row picks scale[a] X[b][col[a]], a K row has its dot product in KX
__global__ __launch_bounds__(256)
void pu_MX_kernel(int k, int Nstate, const int* __restrict__ col, const double* __restrict__ scale,
                  const double* __restrict__ X, const double* __restrict__ KX, double* __restrict__ MX)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= k*k) return;
    const int a = i / k, b = i % k;
    const int c = col[a];
    MX[i] = c >= 0 ? scale[a]*X[(size_t)b*Nstate + c] : KX[(size_t)(-c-1)*k + b];
}

// A wavefront a point. pose (rrp): R (9), dR[i][j]/dr[k] at 9 + 9i + 3j + k (27), t (3)
template<int PROJ, int NDIST, bool LDS_C>
__global__ __launch_bounds__(64*PU_WAVES)
void pu_points_kernel(PUArgs a, const double* __restrict__ C, const double* __restrict__ intr_g, const double* __restrict__ pose,
                      const double* __restrict__ p_cam, double* __restrict__ out)
{
    extern __shared__ double sC[];
    const double* __restrict__ Cm = C;
    if(LDS_C)
    {
        for(int i = threadIdx.x; i < a.k*a.k; i += blockDim.x) sC[i] = C[i];
        __syncthreads();
        Cm = sC;
    }
    const int lane = threadIdx.x & 63;
    for(int ip = blockIdx.x*PU_WAVES + (threadIdx.x >> 6); ip < a.N; ip += gridDim.x*PU_WAVES)
    {
        const double pc[3] = { p_cam[3*(size_t)ip], p_cam[3*(size_t)ip + 1], p_cam[3*(size_t)ip + 2] };
        double q[2], dq_dp[2][3];
        // this lane's entry of G: its row of C and the two image rows' partials
        int row = -1;
        double g0 = 0.0, g1 = 0.0;
        if constexpr(PROJ == PROJ_SPLINED)
        {
            double dfxy[2], cfx[4], cfy[4];
            int ivar0;
            project_splined<true>(q, dq_dp, dfxy, &ivar0, cfx, cfy, pc, intr_g, a.cfg);
            if(lane < a.Ncore_state)
            {
                row = lane;
                if(lane == 0) g0 = dfxy[0]; else if(lane == 1) g1 = dfxy[1]; else if(lane == 2) g0 = 1.0; else g1 = 1.0;
            }
            else if(lane < a.Ncore_state + a.Npatch)
            {
                const int n = a.cfg.spline_order + 1;
                const int e = lane - a.Ncore_state, jy = e/(2*n), jx = (e >> 1) % n, c = e & 1;
                double cx = cfx[0], cy = cfy[0];
#pragma unroll
                for(int j = 1; j < 4; j++) { if(jx == j) cx = cfx[j]; if(jy == j) cy = cfy[j]; }
                const double v = cx*cy*(c ? intr_g[1] : intr_g[0]);
                row = a.Ncore_state + (ivar0 - 4) + jy*2*a.cfg.spline_Nx + 2*jx + c;
                if(c) g1 = v; else g0 = v;
            }
        }
        else
        {
            double intr[4 + NDIST];
#pragma unroll
            for(int i = 0; i < 4 + NDIST; i++) intr[i] = intr_g[i];
            double gk[2][NDIST > 0 ? NDIST : 1];
            project_lens<PROJ,NDIST,true>(q, dq_dp, gk, pc, intr, a.cfg);
            if(lane < a.Nint)
            {
                // dq/dintrinsics as mrcal_project() gives it (project_kernels.hip)
                const int arg = a.arg0 + lane;
                row = lane;
                if(arg == 0)      g0 = (q[0] - intr[2])/intr[0];
                else if(arg == 1) g1 = (q[1] - intr[3])/intr[1];
                else if(arg == 2) g0 = 1.0;
                else if(arg == 3) g1 = 1.0;
#pragma unroll
                for(int i = 0; i < NDIST; i++) if(arg == 4 + i) { g0 = gk[0][i]; g1 = gk[1][i]; }
            }
        }

        // the reference frame's point and dq/dpref: through rt_cam_ref (rrp), or the camera's own (ccp)
        double pref[3], dq_dref[2][3];
        if(a.rrp)
        {
            double d[3];
#pragma unroll
            for(int i = 0; i < 3; i++) d[i] = a.atinfinity ? pc[i] : pc[i] - pose[36 + i];
#pragma unroll
            for(int i = 0; i < 3; i++) pref[i] = pose[i]*d[0] + pose[3 + i]*d[1] + pose[6 + i]*d[2];
#pragma unroll
            for(int xy = 0; xy < 2; xy++)
#pragma unroll
                for(int j = 0; j < 3; j++)
                    dq_dref[xy][j] = dq_dp[xy][0]*pose[j] + dq_dp[xy][1]*pose[3 + j] + dq_dp[xy][2]*pose[6 + j];
        }
        else
        {
#pragma unroll
            for(int i = 0; i < 3; i++) { pref[i] = pc[i]; dq_dref[0][i] = dq_dp[0][i]; dq_dref[1][i] = dq_dp[1][i]; }
        }
        const int e_ext = a.Nint_entries, e_K = e_ext + a.Next, NE = e_K + 6;
        if(lane >= e_ext && lane < e_K)
        {
            // dq/dpcam dpcam/drt_cam_ref (transform_point_rt()'s gradient; rotate_point_r()'s at infinity)
            const int j = lane - e_ext;
            row = a.Nint + j;
            double dpc[3];
#pragma unroll
            for(int i = 0; i < 3; i++)
                dpc[i] = j < 3 ? pose[9 + 9*i + j]*pref[0] + pose[9 + 9*i + 3 + j]*pref[1] + pose[9 + 9*i + 6 + j]*pref[2]
                               : ((i == j - 3 && !a.atinfinity) ? 1.0 : 0.0);
            g0 = dq_dp[0][0]*dpc[0] + dq_dp[0][1]*dpc[1] + dq_dp[0][2]*dpc[2];
            g1 = dq_dp[1][0]*dpc[0] + dq_dp[1][1]*dpc[1] + dq_dp[1][2]*dpc[2];
        }
        else if(lane >= e_K && lane < NE)
        {
            // dq/dpref skew(pref) against K's rotation rows, -dq/dpref against its translation rows
            const int j = lane - e_K;
            row = a.Nint + a.Next + j;
            double s[3];
            if(j == 0)      { s[0] = 0.0;      s[1] = pref[2];  s[2] = -pref[1]; }
            else if(j == 1) { s[0] = -pref[2]; s[1] = 0.0;      s[2] = pref[0];  }
            else if(j == 2) { s[0] = pref[1];  s[1] = -pref[0]; s[2] = 0.0;      }
            else
            {
#pragma unroll
                for(int i = 0; i < 3; i++) s[i] = (i == j - 3 && !a.atinfinity) ? -1.0 : 0.0;
            }
            g0 = dq_dref[0][0]*s[0] + dq_dref[0][1]*s[1] + dq_dref[0][2]*s[2];
            g1 = dq_dref[1][0]*s[0] + dq_dref[1][1]*s[1] + dq_dref[1][2]*s[2];
        }
        if(row >= a.k) { row = -1; g0 = g1 = NAN; }      // (cannot happen with a consistent model; never read out of C)

        // h = G C (this lane's column), then G C G^T summed over the lanes by a fixed butterfly
        double h0 = 0.0, h1 = 0.0;
        for(int e = 0; e < NE; e++)
        {
            const int    re  = __shfl(row, e);
            const double ge0 = __shfl(g0, e), ge1 = __shfl(g1, e);
            if(row >= 0 && re >= 0)
            {
                const double c = Cm[(size_t)re*a.k + row];
                h0 += ge0*c;
                h1 += ge1*c;
            }
        }
        const double v00 = wave_sum(h0*g0), v01 = wave_sum(h0*g1), v11 = wave_sum(h1*g1);
        if(lane == 0)
        {
            const double sg = a.sigma;
            if(a.what == MRCAL_AMD_UNCERTAINTY_COVARIANCE)
            {
                // (the reference's Var_dF * sigma*sigma, left to right)
                double* o = out + 4*(size_t)ip;
                o[0] = v00*sg*sg; o[1] = v01*sg*sg; o[2] = v01*sg*sg; o[3] = v11*sg*sg;
            }
            else if(a.what == MRCAL_AMD_UNCERTAINTY_WORSTDIRECTION_STDEV)
                out[ip] = sqrt((v00 + v11)/2 + sqrt((v00 - v11)*(v00 - v11)/4 + v01*v01)) * sg;
            else
                out[ip] = sqrt((v00 + v11)/2) * sg;
        }
    }
}

template<int PROJ, int NDIST>
hipError_t launch_points(const PUArgs& a, const double* C, const double* intr, const double* pose,
                         const double* p, double* out, hipStream_t stream)
{
    const int blocks = std::max(1, std::min((a.N + PU_WAVES - 1)/PU_WAVES, 2048));
    if(a.k*a.k <= PU_LDS_C_MAX)
        hipLaunchKernelGGL((pu_points_kernel<PROJ,NDIST,true>), dim3(blocks), dim3(64*PU_WAVES),
                           (size_t)a.k*a.k*sizeof(double), stream, a, C, intr, pose, p, out);
    else
        hipLaunchKernelGGL((pu_points_kernel<PROJ,NDIST,false>), dim3(blocks), dim3(64*PU_WAVES), 0, stream, a, C, intr, pose, p, out);
    return hipGetLastError();
}

} // namespace

struct mrcal_amd_uncertainty
{
    int                method = 0;
    mrcal_lensmodel_t  lensmodel;
    PUArgs             args;            // N, atinfinity, what are set per evaluation
    double             sigma = 0.0;
    double*            d_C    = NULL;   // [k][k]
    double*            d_intr = NULL;   // [Nintrinsics] of this camera at the solve
    double*            d_pose = NULL;   // [39] (rrp)
    double*            d_p    = NULL;   // [capacity][3]
    double*            d_out  = NULL;   // [capacity][4]
    int                capacity = 0;
    hipStream_t        stream = NULL;
    DeviceBuffers      mem;
    ~mrcal_amd_uncertainty()
    {
        mem.free_all();
        if(stream) hipStreamDestroy(stream);
    }
};

static bool what_is_known(int what)
{
    if(what == MRCAL_AMD_UNCERTAINTY_COVARIANCE || what == MRCAL_AMD_UNCERTAINTY_WORSTDIRECTION_STDEV ||
       what == MRCAL_AMD_UNCERTAINTY_RMS_STDEV)
        return true;
    set_error("unknown 'what': %d", what);
    return false;
}

namespace mrcal_amd {
// evaluate() on device pointers (noise_propagation.hpp), for projection_diff.hip, whose points and weights never leave
// the device
bool uncertainty_evaluate_device(mrcal_amd_uncertainty_t* u, const double* d_p_cam, int N, bool atinfinity, int what,
                                 double* d_out, hipStream_t stream)
{
    if(u == NULL) { set_error("no uncertainty context"); return false; }
    if(!what_is_known(what)) return false;
    if(N <= 0) return true;
    PUArgs a = u->args;
    a.N = N; a.atinfinity = atinfinity ? 1 : 0; a.what = what;
    hipError_t e = hipSuccess;
    if(!for_parametric_lens(u->lensmodel.type, [&](auto k)
       {
           using K = decltype(k);
           e = launch_points<K::PROJ,K::NDIST>(a, u->d_C, u->d_intr, u->d_pose, d_p_cam, d_out, stream);
       }))
    {
        if(u->lensmodel.type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
        {
            set_error("lens model %d is not supported", (int)u->lensmodel.type);
            return false;
        }
        e = launch_points<PROJ_SPLINED,0>(a, u->d_C, u->d_intr, u->d_pose, d_p_cam, d_out, stream);
    }
    HIP_TRY(e, return false);
    return true;
}
}

namespace {

bool check_arguments(const mrcal_amd_problem* P, int icam_intrinsics, int method)
{
    if(P == NULL) { set_error("no problem"); return false; }
    if(propagation_refuses_shard(P, "projection uncertainty")) return false;
    if(method != MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_CCP && method != MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_RRP_JFP)
    {
        set_error("Unknown uncertainty method: %d", method);
        return false;
    }
    const int Ncameras = P->L.dims.Ncameras_intrinsics;
    if(icam_intrinsics < 0 || icam_intrinsics >= Ncameras)
    {
        set_error("icam_intrinsics MUST be in [0,Ncameras_intrinsics-1]. got %d NOT in [0,%d]", icam_intrinsics, Ncameras-1);
        return false;
    }
    return !propagation_refuses_measurements(P->L);
}

// This camera's extrinsics, from the observations (model_analysis.py:1455-1492); -1: at the reference, or not asked
// for (ccp). false: set_error() says why
bool corresponding_extrinsics(int* icam_e, mrcal_amd_problem* P, int icam_intrinsics, bool rrp)
{
    const Layout& L = P->L;
    *icam_e = -1;
    if(!rrp) return true;
    std::vector<BoardObsMeta> bm((size_t)std::max(L.dims.Nobservations_board, 1));
    std::vector<PointObsMeta> pm((size_t)std::max(L.dims.Nobservations_point, 1));
    if(L.dims.Nobservations_board > 0)
        HIP_TRY(hipMemcpy(bm.data(), P->d_board_meta, (size_t)L.dims.Nobservations_board*sizeof(BoardObsMeta), hipMemcpyDeviceToHost), return false);
    if(L.dims.Nobservations_point > 0)
        HIP_TRY(hipMemcpy(pm.data(), P->d_point_meta, (size_t)L.dims.Nobservations_point*sizeof(PointObsMeta), hipMemcpyDeviceToHost), return false);
    std::vector<int> ie;
    for(int i = 0; i < L.dims.Nobservations_board; i++) if(bm[i].icam_intrinsics == icam_intrinsics) ie.push_back(bm[i].icam_extrinsics);
    for(int i = 0; i < L.dims.Nobservations_point; i++) if(pm[i].icam_intrinsics == icam_intrinsics) ie.push_back(pm[i].icam_extrinsics);
    std::sort(ie.begin(), ie.end());
    ie.erase(std::unique(ie.begin(), ie.end()), ie.end());
    if(ie.empty())
    {
        set_error("No extrinsics corresponding to icam_intrinsics=%d. I don't know what to do", icam_intrinsics);
        return false;
    }
    if(ie.size() > 1)
    {
        for(size_t i = 1; i < ie.size(); i++)
            if(ie[i] != ie[i-1] + 1)
            {
                set_error("At this point I'm only supporting consecutive block of extrinsics for a given icam_intrinsics");
                return false;
            }
        set_error(ie[0] < 0 ? "Have moving camera, some poses are at the reference. This isn't supported yet"
                            : "I only handle stationary cameras for now");
        return false;
    }
    *icam_e = ie[0];
    return true;
}

// C = sym(M X) - (J*[reg] X)^T (J*[reg] X) into u->d_C, with X = (J*^T J*)^-1 M^T: M into the right-hand sides, the
// shared steps, M X. Waits for np's stream, also on failure: nothing queued may still be using the temporaries
bool propagate_C(mrcal_amd_uncertainty* u, NoisePropagation& np, const std::vector<int>& col, const std::vector<double>& scale,
                 const std::vector<double>& K)
{
    const int k = u->args.k, Nstate = np.L.Nstate;
    DeviceBuffers tmp;
    double *d_K = NULL, *d_scale = NULL, *d_rhs = NULL, *d_X = NULL, *d_KX = NULL, *d_JX = NULL, *d_MX = NULL;
    int* d_col = NULL;
    bool ok = tmp.upload(&d_K, K) && tmp.upload(&d_scale, scale) && tmp.upload(&d_col, col) &&
              tmp.alloc(&d_rhs, (size_t)k*Nstate) && tmp.alloc(&d_X, (size_t)k*Nstate) && tmp.alloc(&d_KX, (size_t)6*k) &&
              tmp.alloc(&d_JX, (size_t)std::max(np.Nreg, 1)*k) && tmp.alloc(&d_MX, (size_t)k*k);
    if(ok)
    {
        const int64_t n = (int64_t)k*Nstate;
        hipLaunchKernelGGL(pu_rhs_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, np.stream, k, Nstate, d_col, d_scale, d_K, d_rhs);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    ok = ok && np.solve(d_rhs, k, d_X) && np.row_dots(d_K, 6, d_X, k, d_KX) && np.reg_rows_times(d_X, k, d_JX);
    if(ok)
    {
        hipLaunchKernelGGL(pu_MX_kernel, dim3((k*k + 255)/256), dim3(256), 0, np.stream, k, Nstate, d_col, d_scale, d_X, d_KX, d_MX);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    ok = ok && np.combine(d_MX, d_JX, k, 1.0, u->d_C);
    HIP_TRY(hipStreamSynchronize(np.stream), ok = false);
    return ok;
}

} // namespace

extern "C" {

mrcal_amd_uncertainty_t*
mrcal_amd_uncertainty_create(mrcal_amd_problem_t* P, int icam_intrinsics, int method, double observed_pixel_uncertainty)
{
    last_error_string().clear();
    if(!check_arguments(P, icam_intrinsics, method)) return NULL;
    const Layout& L = P->L;
    const bool rrp = method == MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_RRP_JFP;
    int icam_e = -1;
    if(!corresponding_extrinsics(&icam_e, P, icam_intrinsics, rrp)) return NULL;

    std::unique_ptr<mrcal_amd_uncertainty> u(new mrcal_amd_uncertainty());
    u->method = method;
    u->lensmodel = L.lensmodel;
    PUArgs& a = u->args;
    // the rows of M: unit rows times the unpacking scales (intrinsics, extrinsics), then K
    std::vector<int>    col;
    std::vector<double> scale;
    plan_uncertainty_rows(&a, &col, &scale, L, icam_intrinsics, icam_e, rrp);
    if(a.Nint_entries + a.Next + 6 > 64)
    {
        set_error("projection uncertainty: %d nonzero entries of dq/db a point; at most 64 are supported", a.Nint_entries + a.Next + 6);
        return NULL;
    }

    // K from the resident J (evaluates x and J at the problem's state), then the factorization of the same normal equations
    std::vector<double> K((size_t)6*L.Nstate);
    if(!mrcal_amd_problem_drt_cross_reprojection(P, rrp ? -1 : icam_intrinsics, K.data())) return NULL;
    const bool want_sigma = !(observed_pixel_uncertainty > 0.0);
    std::unique_ptr<NoisePropagation> np = NoisePropagation::create(P, "projection uncertainty", want_sigma);
    if(!np) return NULL;
    if(want_sigma && np->sigma_estimate < 0.0) { set_error_no_sigma_estimate(); return NULL; }
    u->sigma = a.sigma = want_sigma ? np->sigma_estimate : observed_pixel_uncertainty;

    // this camera's intrinsics and pose at the solve
    ProblemStateArrays s;
    if(!problem_state_arrays(P, &s)) return NULL;
    double pose[39];
    memset(pose, 0, sizeof(pose));
    {
        double r[3] = { 0, 0, 0 };
        if(rrp && icam_e >= 0) for(int i = 0; i < 3; i++) { r[i] = s.rt_cam_ref[icam_e].r.xyz[i]; pose[36 + i] = s.rt_cam_ref[icam_e].t.xyz[i]; }
        R_from_r_with_grad(pose, pose + 9, r);
    }
    HIP_TRY(hipStreamCreateWithFlags(&u->stream, hipStreamNonBlocking), return NULL);
    if(!u->mem.alloc(&u->d_C, (size_t)a.k*a.k) ||
       !u->mem.upload(&u->d_intr, s.intrinsics.data() + (size_t)icam_intrinsics*L.Nintrinsics, (size_t)L.Nintrinsics) ||
       !u->mem.upload(&u->d_pose, pose, sizeof(pose)/sizeof(double)) ||
       !propagate_C(u.get(), *np, col, scale, K))
        return NULL;
    return u.release();
}

double mrcal_amd_uncertainty_observed_pixel_uncertainty(const mrcal_amd_uncertainty_t* u)
{
    return u ? u->sigma : -1.0;
}

bool mrcal_amd_uncertainty_evaluate(mrcal_amd_uncertainty_t* u, const double* p_cam, int N, bool atinfinity, int what, double* out)
{
    last_error_string().clear();
    if(u == NULL) { set_error("no uncertainty context"); return false; }
    if(!what_is_known(what)) return false;
    if(N <= 0) return true;
    if(u->capacity < N)
    {
        u->mem.release(&u->d_p); u->mem.release(&u->d_out);
        u->capacity = 0;
        if(!u->mem.alloc(&u->d_p, (size_t)N*3) || !u->mem.alloc(&u->d_out, (size_t)N*4)) return false;
        u->capacity = N;
    }
    const size_t nout = (size_t)N*(what == MRCAL_AMD_UNCERTAINTY_COVARIANCE ? 4 : 1);
    HIP_TRY(hipMemcpyAsync(u->d_p, p_cam, (size_t)N*3*sizeof(double), hipMemcpyHostToDevice, u->stream), return false);
    if(!uncertainty_evaluate_device(u, u->d_p, N, atinfinity, what, u->d_out, u->stream)) return false;
    HIP_TRY(hipMemcpyAsync(out, u->d_out, nout*sizeof(double), hipMemcpyDeviceToHost, u->stream), return false);
    HIP_TRY(hipStreamSynchronize(u->stream), return false);
    return true;
}

void mrcal_amd_uncertainty_destroy(mrcal_amd_uncertainty_t* u) { delete u; }

} // extern "C"
