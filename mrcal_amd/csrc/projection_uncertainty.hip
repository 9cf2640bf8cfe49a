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
// reference's "simplified expression"). Kernels:
//   pu_rhs_kernel         M, written into the solve's right-hand sides (no copy of size Nstate crosses PCIe but K)
//   pu_KX_kernel          the K rows of M X: a wavefront a dot product, fixed-order sum
//   pu_JX_kernel          J*[reg] X: a lane per (row, column), the row's entries in CSR order
//   pu_C_kernel           C: a lane per entry, symmetrized, the regularization rows summed in row order
//   pu_sigma_kernel       the sigma estimate's sum of squares (model_analysis.py:491-557): one workgroup, fixed tree
//   pu_points_kernel      a wavefront a point: the projection with gradients through lens_models.hpp, one nonzero
//                         entry of G a lane (a splined model's G has only the core, the (order+1)^2 patch of each
//                         image row and the pose columns), G C G^T by shuffles, C in LDS when it fits
// Nothing uses floating-point atomics: every result is the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "layout.hpp"
#include "host_state.hpp"
#include "problem_object.hpp"
#include "lens_models.hpp"
#include "lens_dispatch.hpp"
#include "device_math.hpp"
#include "../../include/mrcal_amd.h"

using namespace mrcal_amd;

namespace mrcal_amd {
// factorization.cpp (internal)
hipStream_t factorization_stream(mrcal_amd_factorization_t* f);
bool factorization_solve_device(mrcal_amd_factorization_t* f, int sys, const double* d_bt, int Nrhs, double* d_xt);
}

namespace {

// What the per-point kernel needs to know of G's layout
struct PUArgs
{
    LensConfig cfg;
    int N;
    int k;              // rows / columns of C
    int Nint;           // rows of C that are this camera's optimized intrinsics
    int arg0;           // parametric models: the intrinsics argument of row 0 (4 if the core is not optimized)
    int Nint_entries;   // entries of G in the intrinsics rows: Nint, or for the splined models core + patch
    int Ncore_state;    // splined: 4 if the core is optimized, else 0
    int Npatch;         // splined: 2 (order+1)^2 if the distortions are optimized, else 0
    int Next;           // 6: rrp, and this camera's extrinsics are in the state; else 0
    int rrp;
    int atinfinity;
    int what;
    double sigma;
};
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

// KX[r][b] = sum_s K[r][s] X[b][s]: a wavefront per (r,b); lane l sums s = l, l+64, ... in order, then a fixed butterfly
__global__ __launch_bounds__(256)
void pu_KX_kernel(int k, int Nstate, const double* __restrict__ K, const double* __restrict__ X, double* __restrict__ KX)
{
    const int w = blockIdx.x*(blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if(w >= 6*k) return;
    const int r = w / k, b = w % k;
    const double* __restrict__ Kr = K + (size_t)r*Nstate;
    const double* __restrict__ Xb = X + (size_t)b*Nstate;
    double s = 0.0;
    for(int i = lane; i < Nstate; i += 64) s += Kr[i]*Xb[i];
    for(int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if(lane == 0) KX[w] = s;
}

// JX[r][a] = sum over the entries of regularization row r of J[r][c] X[a][c], in CSR order
__global__ __launch_bounds__(256)
void pu_JX_kernel(int Nreg, int i_meas_reg, int k, int Nstate, const int32_t* __restrict__ Jp, const int32_t* __restrict__ Ji,
                  const double* __restrict__ Jx, const double* __restrict__ X, double* __restrict__ JX)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= Nreg*k) return;
    const int r = i / k, a = i % k;
    const double* __restrict__ Xa = X + (size_t)a*Nstate;
    double s = 0.0;
    for(int32_t e = Jp[i_meas_reg + r]; e < Jp[i_meas_reg + r + 1]; e++) s += Jx[e]*Xa[Ji[e]];
    JX[i] = s;
}

// C[a][b] = (MX[a][b] + MX[b][a])/2 - sum_r JX[r][a] JX[r][b]
__device__ __forceinline__
double pu_MX(int a, int b, int k, int Nstate, const int* __restrict__ col, const double* __restrict__ scale,
             const double* __restrict__ X, const double* __restrict__ KX)
{
    const int c = col[a];
    return c >= 0 ? scale[a]*X[(size_t)b*Nstate + c] : KX[(size_t)(-c-1)*k + b];
}
__global__ __launch_bounds__(256)
void pu_C_kernel(int k, int Nstate, int Nreg, const int* __restrict__ col, const double* __restrict__ scale,
                 const double* __restrict__ X, const double* __restrict__ KX, const double* __restrict__ JX, double* __restrict__ C)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= k*k) return;
    const int a = i / k, b = i % k;
    double s = 0.0;
    for(int r = 0; r < Nreg; r++) s += JX[(size_t)r*k + a]*JX[(size_t)r*k + b];
    C[i] = 0.5*(pu_MX(a, b, k, Nstate, col, scale, X, KX) + pu_MX(b, a, k, Nstate, col, scale, X, KX)) - s;
}

// sum of squares and count of the board and point measurements whose observation has a positive weight
// (measurements_board() / measurements_point(), mrcal/utils.py:1286-1500). One workgroup of 256, fixed order
__global__ __launch_bounds__(256)
void pu_sigma_kernel(int Ncorners, const double* __restrict__ board_pool, int i_meas_boards,
                     int Npoint_obs, const double* __restrict__ point_pool, int i_meas_points,
                     const double* __restrict__ x, double* __restrict__ out)
{
    __shared__ double ss[256], nn[256];
    double s = 0.0, n = 0.0;
    for(int c = threadIdx.x; c < Ncorners; c += 256)
        if(board_pool[3*(size_t)c + 2] > 0.0)
        {
            const double x0 = x[i_meas_boards + 2*(size_t)c], x1 = x[i_meas_boards + 2*(size_t)c + 1];
            s += x0*x0 + x1*x1; n += 2.0;
        }
    for(int c = threadIdx.x; c < Npoint_obs; c += 256)
        if(point_pool[3*(size_t)c + 2] > 0.0)
        {
            const double x0 = x[i_meas_points + 2*c], x1 = x[i_meas_points + 2*c + 1];
            s += x0*x0 + x1*x1; n += 2.0;
        }
    ss[threadIdx.x] = s; nn[threadIdx.x] = n;
    __syncthreads();
    for(int h = 128; h >= 1; h >>= 1)
    {
        if((int)threadIdx.x < h) { ss[threadIdx.x] += ss[threadIdx.x + h]; nn[threadIdx.x] += nn[threadIdx.x + h]; }
        __syncthreads();
    }
    if(threadIdx.x == 0) { out[0] = ss[0]; out[1] = nn[0]; }
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
        double v00 = h0*g0, v01 = h0*g1, v11 = h1*g1;
#pragma unroll
        for(int off = 32; off >= 1; off >>= 1)
        {
            v00 += __shfl_xor(v00, off);
            v01 += __shfl_xor(v01, off);
            v11 += __shfl_xor(v11, off);
        }
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

namespace mrcal_amd {
// The estimate of the observed pixel uncertainty (model_analysis.py:491-557), for this file and triangulation.hip.
// Queues on st: the sums over the board and point measurements of x at the problem's current operating point
// (d_sig[2], a device buffer of the caller's), and their copy to sig[2], which is complete once st has been waited for
bool queue_observed_pixel_sums(mrcal_amd_problem* P, double* d_sig, double* sig, hipStream_t st)
{
    const Layout& L = P->L;
    hipLaunchKernelGGL(pu_sigma_kernel, dim3(1), dim3(256), 0, st,
                       L.dims.Nobservations_board*L.dims.object_width_n*L.dims.object_height_n, P->d_board_pool, L.i_meas_boards,
                       L.dims.Nobservations_point, P->d_point_pool, L.i_meas_points, P->op[P->icur].x, d_sig);
    HIP_TRY(hipGetLastError(), return false);
    HIP_TRY(hipMemcpyAsync(sig, d_sig, 2*sizeof(double), hipMemcpyDeviceToHost, st), return false);
    return true;
}
// ... and the estimate from them: RMS / sqrt(1 - Nstate/Nmeasurements)
bool observed_pixel_uncertainty_from_sums(double* sigma, const double* sig, int Nstate)
{
    if(sig[1] == 0.0)
    {
        set_error("observed_pixel_uncertainty cannot be computed because we don't have any board or point observations");
        return false;
    }
    const double f_ = sqrt(1.0 - (double)Nstate/sig[1]);
    *sigma = sqrt(sig[0]/sig[1]) / f_;
    return true;
}
}

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
// evaluate() on device pointers: p_cam [N][3] in, out [N][4] (covariance) or [N], queued on the caller's stream and not
// waited for. For projection_diff.hip, whose points and weights never leave the device. (C and the camera's
// intrinsics were complete when _create() returned: any stream may read them)
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

extern "C" {

mrcal_amd_uncertainty_t*
mrcal_amd_uncertainty_create(mrcal_amd_problem_t* P, int icam_intrinsics, int method, double observed_pixel_uncertainty)
{
    last_error_string().clear();
    if(P == NULL) { set_error("no problem"); return NULL; }
    const Layout& L = P->L;
    if((int)P->board_sel.size() != L.dims.Nobservations_board || P->comm != NULL)
    {
        set_error("projection uncertainty: this problem is a shard (it holds a part of the rows)");
        return NULL;
    }
    if(method != MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_CCP && method != MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_RRP_JFP)
    {
        set_error("Unknown uncertainty method: %d", method);
        return NULL;
    }
    if(icam_intrinsics < 0 || icam_intrinsics >= L.dims.Ncameras_intrinsics)
    {
        set_error("icam_intrinsics MUST be in [0,Ncameras_intrinsics-1]. got %d NOT in [0,%d]", icam_intrinsics, L.dims.Ncameras_intrinsics-1);
        return NULL;
    }
    if(L.Nmeas_triangulated > 0)
    {
        set_error("Some measurements other than boards, points and regularization are present. Don't know what to do");
        return NULL;
    }
    const int Nreg = L.Nmeas_regularization;
    if(Nreg > 0 && L.Nmeas_boards + L.Nmeas_points == 0)
    {
        set_error("No non-regularization measurements. Don't know what to do");
        return NULL;
    }
    const bool rrp = method == MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_RRP_JFP;
    const int Nstate = L.Nstate;

    // this camera's extrinsics, from the observations (model_analysis.py:1455-1492)
    int icam_e = -1;
    {
        std::vector<BoardObsMeta> bm((size_t)std::max(L.dims.Nobservations_board, 1));
        std::vector<PointObsMeta> pm((size_t)std::max(L.dims.Nobservations_point, 1));
        if(L.dims.Nobservations_board > 0)
            HIP_TRY(hipMemcpy(bm.data(), P->d_board_meta, (size_t)L.dims.Nobservations_board*sizeof(BoardObsMeta), hipMemcpyDeviceToHost), return NULL);
        if(L.dims.Nobservations_point > 0)
            HIP_TRY(hipMemcpy(pm.data(), P->d_point_meta, (size_t)L.dims.Nobservations_point*sizeof(PointObsMeta), hipMemcpyDeviceToHost), return NULL);
        std::vector<int> ie;
        for(int i = 0; i < L.dims.Nobservations_board; i++) if(bm[i].icam_intrinsics == icam_intrinsics) ie.push_back(bm[i].icam_extrinsics);
        for(int i = 0; i < L.dims.Nobservations_point; i++) if(pm[i].icam_intrinsics == icam_intrinsics) ie.push_back(pm[i].icam_extrinsics);
        std::sort(ie.begin(), ie.end());
        ie.erase(std::unique(ie.begin(), ie.end()), ie.end());
        if(rrp)
        {
            if(ie.empty())
            {
                set_error("No extrinsics corresponding to icam_intrinsics=%d. I don't know what to do", icam_intrinsics);
                return NULL;
            }
            if(ie.size() > 1)
            {
                for(size_t i = 1; i < ie.size(); i++)
                    if(ie[i] != ie[i-1] + 1)
                    {
                        set_error("At this point I'm only supporting consecutive block of extrinsics for a given icam_intrinsics");
                        return NULL;
                    }
                set_error(ie[0] < 0 ? "Have moving camera, some poses are at the reference. This isn't supported yet"
                                    : "I only handle stationary cameras for now");
                return NULL;
            }
            icam_e = ie[0];
        }
    }

    mrcal_amd_uncertainty* u = new mrcal_amd_uncertainty();
    u->method = method;
    u->lensmodel = L.lensmodel;
    memset(&u->args, 0, sizeof(u->args));
    PUArgs& a = u->args;
    a.rrp = rrp ? 1 : 0;
    a.cfg = lens_config_of(L.lensmodel);
    a.Nint = L.Nintr_state;
    a.arg0 = L.Ncore - L.Ncore_state;
    if(L.lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
    {
        const int n = a.cfg.spline_order + 1;
        a.Ncore_state  = L.Ncore_state;
        a.Npatch       = L.Ndist_state > 0 ? 2*n*n : 0;
        a.Nint_entries = a.Ncore_state + a.Npatch;
    }
    else
        a.Nint_entries = a.Nint;
    a.Next = (rrp && icam_e >= 0 && L.i_state_extrinsics >= 0) ? 6 : 0;
    a.k = a.Nint + a.Next + 6;
    const int k = a.k;
    if(a.Nint_entries + a.Next + 6 > 64)
    {
        set_error("projection uncertainty: %d nonzero entries of dq/db a point; at most 64 are supported", a.Nint_entries + a.Next + 6);
        delete u; return NULL;
    }

    // the rows of M: unit rows times the unpacking scales (intrinsics, extrinsics), then K
    std::vector<int>    col(k);
    std::vector<double> scale(k, 0.0);
    for(int j = 0; j < a.Nint; j++)
    {
        col[j] = L.i_state_intrinsics + icam_intrinsics*L.Nintr_state + j;
        scale[j] = L.Ncore_state && j < 2 ? SCALE_INTRINSICS_FOCAL_LENGTH :
                   L.Ncore_state && j < 4 ? SCALE_INTRINSICS_CENTER_PIXEL : SCALE_DISTORTION;
    }
    for(int j = 0; j < a.Next; j++)
    {
        col[a.Nint + j] = L.i_state_extrinsics + 6*icam_e + j;
        scale[a.Nint + j] = j < 3 ? SCALE_ROTATION_CAMERA : SCALE_TRANSLATION_CAMERA;
    }
    for(int j = 0; j < 6; j++) col[a.Nint + a.Next + j] = -j - 1;

    // K from the resident J (evaluates x and J at the problem's state: with values, whatever the solver's
    // Jacobian stream was set to), then the factorization of the same normal equations
    std::vector<double> K((size_t)6*Nstate);
    if(!mrcal_amd_problem_drt_cross_reprojection(P, rrp ? -1 : icam_intrinsics, K.data())) { delete u; return NULL; }
    mrcal_amd_factorization_t* f = mrcal_amd_factorization_create_from_problem(P);
    if(f == NULL)
    {
        if(mrcal_amd_factorization_last_status() == 1)
            set_error("Cannot compute the uncertainty: factorization computation failed");
        delete u; return NULL;
    }
    if(!problem_ensure_jacobian(P)) { mrcal_amd_factorization_destroy(f); delete u; return NULL; }

    // this camera's intrinsics and pose at the solve: the seeds with the state unpacked over them
    std::vector<double> b((size_t)std::max(Nstate, 1));
    std::vector<double> intr_all((size_t)L.dims.Ncameras_intrinsics*L.Nintrinsics);
    std::vector<mrcal_pose_t> rt((size_t)std::max(L.dims.Ncameras_extrinsics, 1));
    std::vector<mrcal_pose_t> frames((size_t)std::max(L.dims.Nframes, 1));
    std::vector<mrcal_point3_t> points((size_t)std::max(L.dims.Npoints, 1));
    mrcal_calobject_warp_t warp;
    bool ok = mrcal_amd_problem_get_b_packed(P, b.data());
    if(ok) HIP_TRY(hipMemcpy(intr_all.data(), P->d_seed_intrinsics, intr_all.size()*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    if(ok && L.dims.Ncameras_extrinsics > 0)
        HIP_TRY(hipMemcpy(rt.data(), P->d_seed_rt_cam_ref, (size_t)L.dims.Ncameras_extrinsics*sizeof(mrcal_pose_t), hipMemcpyDeviceToHost), ok = false);
    if(!ok) { mrcal_amd_factorization_destroy(f); delete u; return NULL; }
    unpack_state_to_arrays(b.data(), L, intr_all.data(), rt.data(), frames.data(), points.data(), &warp);
    double pose[39];
    memset(pose, 0, sizeof(pose));
    {
        double r[3] = { 0, 0, 0 };
        if(rrp && icam_e >= 0) for(int i = 0; i < 3; i++) { r[i] = rt[icam_e].r.xyz[i]; pose[36 + i] = rt[icam_e].t.xyz[i]; }
        R_from_r_with_grad(pose, pose + 9, r);
    }

    hipStream_t st = factorization_stream(f);
    DeviceBuffers tmp;      // what only this function needs
    double *d_K = NULL, *d_rhs = NULL, *d_X = NULL, *d_KX = NULL, *d_JX = NULL, *d_scale = NULL, *d_sig = NULL;
    int* d_col = NULL;
    HIP_TRY(hipStreamCreateWithFlags(&u->stream, hipStreamNonBlocking), ok = false);
    ok = ok && tmp.alloc(&d_K,     (size_t)6*Nstate);
    ok = ok && tmp.alloc(&d_rhs,   (size_t)k*Nstate);
    ok = ok && tmp.alloc(&d_X,     (size_t)k*Nstate);
    ok = ok && tmp.alloc(&d_KX,    (size_t)6*k);
    ok = ok && tmp.alloc(&d_JX,    (size_t)std::max(Nreg, 1)*k);
    ok = ok && tmp.alloc(&d_scale, (size_t)k);
    ok = ok && tmp.alloc(&d_col,   (size_t)k);
    ok = ok && tmp.alloc(&d_sig,   2);
    ok = ok && u->mem.alloc(&u->d_C,    (size_t)k*k);
    ok = ok && u->mem.alloc(&u->d_intr, (size_t)L.Nintrinsics);
    ok = ok && u->mem.alloc(&u->d_pose, sizeof(pose)/sizeof(double));
    if(ok) HIP_TRY(hipMemcpyAsync(d_K, K.data(), (size_t)6*Nstate*sizeof(double), hipMemcpyHostToDevice, st), ok = false);
    if(ok) HIP_TRY(hipMemcpyAsync(d_scale, scale.data(), (size_t)k*sizeof(double), hipMemcpyHostToDevice, st), ok = false);
    if(ok) HIP_TRY(hipMemcpyAsync(d_col, col.data(), (size_t)k*sizeof(int), hipMemcpyHostToDevice, st), ok = false);
    if(ok) HIP_TRY(hipMemcpyAsync(u->d_intr, intr_all.data() + (size_t)icam_intrinsics*L.Nintrinsics, (size_t)L.Nintrinsics*sizeof(double),
                                  hipMemcpyHostToDevice, st), ok = false);
    if(ok) HIP_TRY(hipMemcpyAsync(u->d_pose, pose, sizeof(pose), hipMemcpyHostToDevice, st), ok = false);
    // (the problem's stream wrote x and J: the factorization's stream is not ordered behind it)
    if(ok) HIP_TRY(hipStreamSynchronize(P->stream), ok = false);
    const int64_t nrhs_el = (int64_t)k*Nstate;
    if(ok)
    {
        hipLaunchKernelGGL(pu_rhs_kernel, dim3((unsigned)((nrhs_el + 255)/256)), dim3(256), 0, st, k, Nstate, d_col, d_scale, d_K, d_rhs);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    ok = ok && factorization_solve_device(f, FSOLVE_A, d_rhs, k, d_X);
    if(ok)
    {
        hipLaunchKernelGGL(pu_KX_kernel, dim3((6*k + 3)/4), dim3(256), 0, st, k, Nstate, d_K, d_X, d_KX);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    if(ok && Nreg > 0)
    {
        hipLaunchKernelGGL(pu_JX_kernel, dim3((Nreg*k + 255)/256), dim3(256), 0, st, Nreg, L.i_meas_regularization, k, Nstate,
                           P->d_Jp, P->d_Ji, P->op[P->icur].Jv, d_X, d_JX);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    if(ok)
    {
        hipLaunchKernelGGL(pu_C_kernel, dim3((k*k + 255)/256), dim3(256), 0, st, k, Nstate, Nreg, d_col, d_scale, d_X, d_KX, d_JX, u->d_C);
        HIP_TRY(hipGetLastError(), ok = false);
    }
    double sig[2] = { 0.0, 0.0 };
    if(ok && !(observed_pixel_uncertainty > 0.0))
        ok = queue_observed_pixel_sums(P, d_sig, sig, st);
    if(ok) HIP_TRY(hipStreamSynchronize(st), ok = false);
    tmp.free_all();
    mrcal_amd_factorization_destroy(f);
    if(!ok) { delete u; return NULL; }

    if(observed_pixel_uncertainty > 0.0)
        u->sigma = observed_pixel_uncertainty;
    else
    {
        if(!observed_pixel_uncertainty_from_sums(&u->sigma, sig, Nstate)) { delete u; return NULL; }
    }
    a.sigma = u->sigma;
    return u;
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
