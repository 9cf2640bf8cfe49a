// mrcal.triangulate_*(): a batch of ray pairs -> points and their gradients.
//
// Reference: triangulation.cc (the six mrcal_triangulate_...()), broadcast by
// mrcal/triangulation.py:61-949. The arithmetic is triangulation_math.hpp, the
// source the CPU tests build for the host; here one lane takes one pair. Pairs
// are independent and nothing is summed across lanes: no atomics, the same bits
// on every call.
//
// mrcal.triangulate() (mrcal/triangulation.py:1090-2018): pixel pairs through calibrated cameras -> points, with the
// observation-time and the calibration-time noise propagated. tri_pairs_kernel is the body of
// _triangulation_uncertainty_internal() for one pair, one lane a pair, behind launch_unproject_points() once per
// distinct camera:
//   rt01 = compose(rt_0ref, invert(rt_1ref)), v1 = R(r01) vlocal1, p = method(vlocal0, v1, t01)
//   dp/dq (3x4), Var_p_observation = dp/dq Var_q dp/dq^T
//   F = dp/db_packed: the pair's three rows of it (zeroed by the block that owns them first)
// The gradients of the method come from tri_eval() (three partials a pass), those of the pose arithmetic from
// Dual<3> passes over compose_r_dual() / rotate_point_r_dual(), and the chain is small matrix products, as in the
// reference. The propagation, with F (3N x Nstate):
//   X = (J*^T J*)^-1 F^T                                            (the resident factorization)
//   Var_p_calibration = sigma^2 ( sym(F X) - (J*[reg] X)^T (J*[reg] X) )
// which are noise_propagation.hpp's steps with F dense: F X is its row-dot kernel over all of F.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include <memory>
#include "triangulation_math.hpp"
#include "layout.hpp"
#include "kernels.hpp"
#include "lens_dispatch.hpp"
#include "problem_object.hpp"
#include "device_memory.hpp"
#include "host_state.hpp"
#include "analysis_plan.hpp"
#include "noise_propagation.hpp"
#include "../../include/mrcal_amd.h"

using namespace mrcal_amd;

namespace {

constexpr int TRI_THREADS = 256;
// Partials carried at a time (triangulation_math.hpp tri_eval()). With 3 the largest instantiation (Lindstrom, its
// eighteen variables in six passes) holds 8 registers a scalar instead of 38, and no instantiation needs scratch
// 
constexpr int TRI_NCHUNK = 3;

// v0, v1 (N,3); pose (N,3): t01, or for Lindstrom (N,12): Rt01. p (N,3); WITH_GRAD: dp_dv0, dp_dv1 (N,3,3) and
// dp_dpose (N,3,3), Lindstrom's (N,3,12)
template<int METHOD, bool WITH_GRAD>
__global__ void __launch_bounds__(TRI_THREADS)
tri_method_kernel(int N, const double* __restrict__ v0, const double* __restrict__ v1, const double* __restrict__ pose,
                  double* __restrict__ p, double* __restrict__ dp_dv0, double* __restrict__ dp_dv1, double* __restrict__ dp_dpose)
{
    constexpr int NP = tri_pose_size(METHOD);
    const int i = blockIdx.x*TRI_THREADS + threadIdx.x;
    if(i >= N) return;
    double a[3], b[3], c[NP];
    for(int k=0;k<3;k++)  { a[k] = v0[(size_t)3*i + k]; b[k] = v1[(size_t)3*i + k]; }
    for(int k=0;k<NP;k++) c[k] = pose[(size_t)NP*i + k];
    tri_eval<METHOD, WITH_GRAD, TRI_NCHUNK>(p + (size_t)3*i,
                                            WITH_GRAD ? dp_dv0   + (size_t)9*i    : NULL,
                                            WITH_GRAD ? dp_dv1   + (size_t)9*i    : NULL,
                                            WITH_GRAD ? dp_dpose + (size_t)3*NP*i : NULL,
                                            a, b, c);
}

template<int METHOD>
hipError_t launch_tri_method(int N, const double* v0, const double* v1, const double* pose,
                             double* p, double* g0, double* g1, double* gp, hipStream_t stream)
{
    const int Nblocks = (N + TRI_THREADS - 1)/TRI_THREADS;
    if(g0 != NULL) tri_method_kernel<METHOD, true ><<<Nblocks, TRI_THREADS, 0, stream>>>(N, v0, v1, pose, p, g0, g1, gp);
    else           tri_method_kernel<METHOD, false><<<Nblocks, TRI_THREADS, 0, stream>>>(N, v0, v1, pose, p, NULL, NULL, NULL);
    return hipGetLastError();
}

// Host arrays in and out. Any of the gradients may be NULL; with one of them asked for, the device forms all three
bool triangulate_host(int method, const char* name, int N, const double* v0, const double* v1, const double* pose,
                      double* p, double* dp_dv0, double* dp_dv1, double* dp_dpose)
{
    last_error_string().clear();
    if(mrcal_amd_device_count() <= 0)
    {
        set_error("no HIP device is visible: libmrcal_amd has no CPU fallback");
        return false;
    }
    if(N < 0 || (N > 0 && (v0 == NULL || v1 == NULL || pose == NULL || p == NULL)))
    {
        set_error("mrcal_amd_triangulate_%s(): N >= 0, and v0, v1, the pose and p must be given", name);
        return false;
    }
    if(N == 0) return true;
    const int  NP    = tri_pose_size(method);
    const bool grads = dp_dv0 != NULL || dp_dv1 != NULL || dp_dpose != NULL;
    DeviceBuffers tmp;
    double *d_v0 = NULL, *d_v1 = NULL, *d_pose = NULL, *d_p = NULL, *d_g0 = NULL, *d_g1 = NULL, *d_gp = NULL;
    bool ok = tmp.upload(&d_v0, v0, (size_t)3*N) && tmp.upload(&d_v1, v1, (size_t)3*N) &&
              tmp.upload(&d_pose, pose, (size_t)NP*N) && tmp.alloc(&d_p, (size_t)3*N);
    if(grads) ok = ok && tmp.alloc(&d_g0, (size_t)9*N) && tmp.alloc(&d_g1, (size_t)9*N) && tmp.alloc(&d_gp, (size_t)3*NP*N);
    if(!ok) return false;
    hipError_t e = hipErrorInvalidValue;
    switch(method)
    {
    case TRI_GEOMETRIC:       e = launch_tri_method<TRI_GEOMETRIC      >(N, d_v0, d_v1, d_pose, d_p, d_g0, d_g1, d_gp, NULL); break;
    case TRI_LINDSTROM:       e = launch_tri_method<TRI_LINDSTROM      >(N, d_v0, d_v1, d_pose, d_p, d_g0, d_g1, d_gp, NULL); break;
    case TRI_LEECIVERA_L1:    e = launch_tri_method<TRI_LEECIVERA_L1   >(N, d_v0, d_v1, d_pose, d_p, d_g0, d_g1, d_gp, NULL); break;
    case TRI_LEECIVERA_LINF:  e = launch_tri_method<TRI_LEECIVERA_LINF >(N, d_v0, d_v1, d_pose, d_p, d_g0, d_g1, d_gp, NULL); break;
    case TRI_LEECIVERA_MID2:  e = launch_tri_method<TRI_LEECIVERA_MID2 >(N, d_v0, d_v1, d_pose, d_p, d_g0, d_g1, d_gp, NULL); break;
    case TRI_LEECIVERA_WMID2: e = launch_tri_method<TRI_LEECIVERA_WMID2>(N, d_v0, d_v1, d_pose, d_p, d_g0, d_g1, d_gp, NULL); break;
    }
    HIP_TRY(e, return false);
    HIP_TRY(hipMemcpy(p, d_p, (size_t)3*N*sizeof(double), hipMemcpyDeviceToHost), return false);
    if(dp_dv0   != NULL) HIP_TRY(hipMemcpy(dp_dv0,   d_g0, (size_t)9*N*sizeof(double),    hipMemcpyDeviceToHost), return false);
    if(dp_dv1   != NULL) HIP_TRY(hipMemcpy(dp_dv1,   d_g1, (size_t)9*N*sizeof(double),    hipMemcpyDeviceToHost), return false);
    if(dp_dpose != NULL) HIP_TRY(hipMemcpy(dp_dpose, d_gp, (size_t)3*NP*N*sizeof(double), hipMemcpyDeviceToHost), return false);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// triangulate()

// a camera of the context's table
struct TriCamDev
{
    double rt[6];           // rt_cam_ref
    int    istate_i;        // first state of its optimized intrinsics; -1: none
    int    istate_e;        // first state of its extrinsics; -1: none (at the reference, or not optimized)
};
struct TriPairsArgs
{
    int    N;
    int    Ni;              // lens parameters of a camera (the stride of dv_di's rows); WITH_F only
    int    Nstate;
    int    Nintr_state;     // optimized intrinsics of a camera, and the first of them among its parameters
    int    intr0;
    int    Ncore_state;
    int    stabilize;
    int    Nframes;         // frames in the state, if stabilizing; else 0
    int    istate_f0;
    double var, var_cross;  // Var_q: the diagonal, and the (q0x,q1x), (q0y,q1y) terms
};

// out (3x3) = a (3x3) b (3x3)
__device__ __forceinline__ void mul33(double (*out)[3], const double (*a)[3], const double (*b)[3])
{
#pragma unroll
    for(int i=0;i<3;i++)
#pragma unroll
        for(int j=0;j<3;j++) out[i][j] = a[i][0]*b[0][j] + a[i][1]*b[1][j] + a[i][2]*b[2][j];
}

// rt01 = compose(rt0, invert(rt1)) with the independent variables [ivar0, ivar0 + N) of (r0, t0, r1, t1)
template<int N> __device__ __forceinline__
void tri_rt01_pass(Dual<N>* r01, Dual<N>* t01, int ivar0, const double* rt0, const double* rt1)
{
    Dual<N> r0[3], t0[3], r1[3], t1[3], r_ref1[3], tmp[3], t_ref1[3], rot[3];
#pragma unroll
    for(int i=0;i<3;i++)
    {
        r0[i] = Dual<N>::variable(rt0[i],     i - ivar0);
        t0[i] = Dual<N>::variable(rt0[3 + i], 3 + i - ivar0);
        r1[i] = Dual<N>::variable(rt1[i],     6 + i - ivar0);
        t1[i] = Dual<N>::variable(rt1[3 + i], 9 + i - ivar0);
    }
    // invert_rt(): r' = -r, t' = -R(-r) t
    rotate_point_r_dual(tmp, r1, t1, true);
#pragma unroll
    for(int i=0;i<3;i++) { r_ref1[i] = -r1[i]; t_ref1[i] = -tmp[i]; }
    // compose_rt(): r01 = compose_r(r0, r'), t01 = R(r0) t' + t0
    compose_r_dual(r01, r0, r_ref1);
    rotate_point_r_dual(rot, r0, t_ref1, false);
#pragma unroll
    for(int i=0;i<3;i++) t01[i] = rot[i] + t0[i];
}

// One lane a pair. pair_cam, pair_row [2N]: the camera of each of the pair's two pixels, and its row of v (.,3),
// dv_dq (.,3,2), dv_di (.,3,Ni). p (N,3); WITH_VAR: var_obs (N,3,3); WITH_F: F (3N, Nstate). METHOD == TRI_LINDSTROM: p alone
template<int METHOD, bool WITH_VAR, bool WITH_F>
__global__ void __launch_bounds__(TRI_THREADS)
tri_pairs_kernel(TriPairsArgs a, const TriCamDev* __restrict__ cams, const int* __restrict__ pair_cam, const int* __restrict__ pair_row,
                 const double* __restrict__ v, const double* __restrict__ dv_dq, const double* __restrict__ dv_di,
                 const double* __restrict__ frames, double* __restrict__ p_out, double* __restrict__ var_obs, double* __restrict__ F)
{
    static_assert(!(WITH_F && !WITH_VAR), "F comes with the gradients");
    static_assert(!(METHOD == TRI_LINDSTROM && WITH_VAR), "Lindstrom: no noise is propagated");
    constexpr bool GRAD = WITH_VAR;
    const int i = blockIdx.x*TRI_THREADS + threadIdx.x;
    if constexpr(WITH_F)
    {
        // this block's rows of F, all of them zero first
        const int    i0 = blockIdx.x*TRI_THREADS, n = min(a.N - i0, TRI_THREADS);
        double*      F0 = F + (size_t)3*i0*a.Nstate;
        const size_t nz = (size_t)3*n*a.Nstate;
        for(size_t k = threadIdx.x; k < nz; k += TRI_THREADS) F0[k] = 0.0;
        __syncthreads();
    }
    if(i >= a.N) return;
    const int c0 = pair_cam[2*i], c1 = pair_cam[2*i + 1], row0 = pair_row[2*i], row1 = pair_row[2*i + 1];
    double rt0[6], rt1[6], vl0[3], vl1[3];
#pragma unroll
    for(int k=0;k<6;k++) { rt0[k] = cams[c0].rt[k]; rt1[k] = cams[c1].rt[k]; }
#pragma unroll
    for(int k=0;k<3;k++) { vl0[k] = v[(size_t)3*row0 + k]; vl1[k] = v[(size_t)3*row1 + k]; }

    // rt01, and its gradients: dr01 (3x6: r0 | r1), dt01 (3x12: r0, t0, r1, t1)
    double rt01[6], dr01[3][6], dt01[3][12];
    {
        Dual<0> r[3], t[3];
        tri_rt01_pass<0>(r, t, 0, rt0, rt1);
#pragma unroll
        for(int k=0;k<3;k++) { rt01[k] = r[k].x; rt01[3 + k] = t[k].x; }
    }
    if constexpr(GRAD)
    {
#pragma unroll
        for(int pass = 0; pass < 4; pass++)
        {
            Dual<3> r[3], t[3];
            tri_rt01_pass<3>(r, t, 3*pass, rt0, rt1);
#pragma unroll
            for(int k=0;k<3;k++)
#pragma unroll
                for(int j=0;j<3;j++)
                {
                    dt01[k][3*pass + j] = t[k].d[j];
                    if(pass == 0) dr01[k][j]     = r[k].d[j];
                    if(pass == 2) dr01[k][3 + j] = r[k].d[j];
                }
        }
    }

    // v1 = R(r01) vlocal1; R01 = dv1/dvlocal1; dv1/dr01
    double v1[3], R01[3][3], dv1_dr01[3][3];
    {
        Dual<3> r[3], x[3], y[3];
#pragma unroll
        for(int k=0;k<3;k++) { r[k] = Dual<3>(rt01[k]); x[k] = Dual<3>::variable(vl1[k], k); }
        rotate_point_r_dual(y, r, x, false);
#pragma unroll
        for(int k=0;k<3;k++)
        {
            v1[k] = y[k].x;
#pragma unroll
            for(int j=0;j<3;j++) R01[k][j] = y[k].d[j];
        }
        if constexpr(GRAD)
        {
#pragma unroll
            for(int k=0;k<3;k++) { r[k] = Dual<3>::variable(rt01[k], k); x[k] = Dual<3>(vl1[k]); }
            rotate_point_r_dual(y, r, x, false);
#pragma unroll
            for(int k=0;k<3;k++)
#pragma unroll
                for(int j=0;j<3;j++) dv1_dr01[k][j] = y[k].d[j];
        }
    }

    double p[3], dp_dv0[3][3], dp_dv1[3][3], dp_dt01[3][3];
    if constexpr(METHOD == TRI_LINDSTROM)
    {
        // local vectors and the whole Rt01
        double Rt[12];
#pragma unroll
        for(int k=0;k<3;k++)
        {
#pragma unroll
            for(int j=0;j<3;j++) Rt[3*k + j] = R01[k][j];
            Rt[9 + k] = rt01[3 + k];
        }
        tri_eval<METHOD, false, TRI_NCHUNK>(p, NULL, NULL, NULL, vl0, vl1, Rt);
    }
    else
        tri_eval<METHOD, GRAD, TRI_NCHUNK>(p, &dp_dv0[0][0], &dp_dv1[0][0], &dp_dt01[0][0], vl0, v1, rt01 + 3);
#pragma unroll
    for(int k=0;k<3;k++) p_out[(size_t)3*i + k] = p[k];

    if constexpr(GRAD)
    {
        // dp/dq = [ dp/dv0 dvlocal0/dq0 | dp/dv1 R01 dvlocal1/dq1 ]
        double A1[3][3], D[3][4];
        mul33(A1, dp_dv1, R01);
        {
            const double* __restrict__ g0 = dv_dq + (size_t)6*row0;
            const double* __restrict__ g1 = dv_dq + (size_t)6*row1;
#pragma unroll
            for(int k=0;k<3;k++)
#pragma unroll
                for(int j=0;j<2;j++)
                {
                    D[k][j]     = dp_dv0[k][0]*g0[j] + dp_dv0[k][1]*g0[2 + j] + dp_dv0[k][2]*g0[4 + j];
                    D[k][2 + j] = A1[k][0]*g1[j]     + A1[k][1]*g1[2 + j]     + A1[k][2]*g1[4 + j];
                }
        }
        // dp/dq Var_q dp/dq^T: the upper triangle, mirrored
        double T[3][4];
#pragma unroll
        for(int k=0;k<3;k++)
        {
            T[k][0] = a.var*D[k][0] + a.var_cross*D[k][2];
            T[k][1] = a.var*D[k][1] + a.var_cross*D[k][3];
            T[k][2] = a.var_cross*D[k][0] + a.var*D[k][2];
            T[k][3] = a.var_cross*D[k][1] + a.var*D[k][3];
        }
#pragma unroll
        for(int k=0;k<3;k++)
#pragma unroll
            for(int j=k;j<3;j++)
            {
                const double s = T[k][0]*D[j][0] + T[k][1]*D[j][1] + T[k][2]*D[j][2] + T[k][3]*D[j][3];
                var_obs[(size_t)9*i + 3*k + j] = s;
                var_obs[(size_t)9*i + 3*j + k] = s;
            }

        if constexpr(WITH_F)
        {
            double* __restrict__ Frow[3] = { F + ((size_t)3*i    )*a.Nstate, F + ((size_t)3*i + 1)*a.Nstate,
                                             F + ((size_t)3*i + 2)*a.Nstate };
            // the intrinsics of both cameras (camera 1's last, as the reference writes them)
#pragma unroll
            for(int cam = 0; cam < 2; cam++)
            {
                const int is = cam == 0 ? cams[c0].istate_i : cams[c1].istate_i;
                if(is < 0) continue;
                const double* __restrict__ gi = dv_di + (size_t)3*(cam == 0 ? row0 : row1)*a.Ni + a.intr0;
                for(int j = 0; j < a.Nintr_state; j++)
                {
                    const double sc = j < a.Ncore_state ? (j < 2 ? SCALE_INTRINSICS_FOCAL_LENGTH : SCALE_INTRINSICS_CENTER_PIXEL)
                                                        : SCALE_DISTORTION;
                    const double g0 = gi[j], g1 = gi[a.Ni + j], g2 = gi[2*a.Ni + j];
#pragma unroll
                    for(int k=0;k<3;k++)
                    {
                        const double* m = cam == 0 ? dp_dv0[k] : A1[k];
                        Frow[k][is + j] = (m[0]*g0 + m[1]*g1 + m[2]*g2)*sc;
                    }
                }
            }
            // the extrinsics: camera 1's, then camera 0's
            double B[3][3];
            mul33(B, dp_dv1, dv1_dr01);
            const int e1 = cams[c1].istate_e, e0 = cams[c0].istate_e;
            if(e1 >= 0)
            {
#pragma unroll
                for(int k=0;k<3;k++)
#pragma unroll
                    for(int j=0;j<3;j++)
                    {
                        double s = 0.0, u = 0.0;
#pragma unroll
                        for(int m=0;m<3;m++) { s += B[k][m]*dr01[m][3 + j] + dp_dt01[k][m]*dt01[m][6 + j]; u += dp_dt01[k][m]*dt01[m][9 + j]; }
                        Frow[k][e1 + j]     = s*SCALE_ROTATION_CAMERA;
                        Frow[k][e1 + 3 + j] = u*SCALE_TRANSLATION_CAMERA;
                    }
            }
            // R0, and the stabilized point's direct dependence on rt_0ref: R0 d( R0^T (p - t0) )/drt_0ref
            double R0[3][3], stab_r[3][3], p_ref[3];
            if(a.stabilize)
            {
                Dual<3> r[3], x[3], y[3], w[3];
#pragma unroll
                for(int k=0;k<3;k++) { r[k] = Dual<3>(rt0[k]); x[k] = Dual<3>::variable(0.0, k); }
                rotate_point_r_dual(y, r, x, false);
#pragma unroll
                for(int k=0;k<3;k++)
#pragma unroll
                    for(int j=0;j<3;j++) R0[k][j] = y[k].d[j];
#pragma unroll
                for(int k=0;k<3;k++) { r[k] = Dual<3>::variable(rt0[k], k); x[k] = Dual<3>(p[k] - rt0[3 + k]); }
                rotate_point_r_dual(y, r, x, true);
#pragma unroll
                for(int k=0;k<3;k++) { p_ref[k] = y[k].x; r[k] = Dual<3>(rt0[k]); }
                rotate_point_r_dual(w, r, y, false);
#pragma unroll
                for(int k=0;k<3;k++)
#pragma unroll
                    for(int j=0;j<3;j++) stab_r[k][j] = w[k].d[j];
            }
            if(e0 >= 0)
            {
#pragma unroll
                for(int k=0;k<3;k++)
#pragma unroll
                    for(int j=0;j<3;j++)
                    {
                        double s = 0.0, u = 0.0;
#pragma unroll
                        for(int m=0;m<3;m++) { s += B[k][m]*dr01[m][j] + dp_dt01[k][m]*dt01[m][j]; u += dp_dt01[k][m]*dt01[m][3 + j]; }
                        if(a.stabilize) { s += stab_r[k][j]; u += (k == j) ? -1.0 : 0.0; }
                        Frow[k][e0 + j]     = s*SCALE_ROTATION_CAMERA;
                        Frow[k][e0 + 3 + j] = u*SCALE_TRANSLATION_CAMERA;
                    }
            }
            // every frame: R0 Rf d( Rf^T (p_ref - tf) )/drt_f / Nframes
            for(int f = 0; f < a.Nframes; f++)
            {
                const double* __restrict__ rtf = frames + (size_t)6*f;
                Dual<3> r[3], x[3], y[3], z[3], w[3];
#pragma unroll
                for(int k=0;k<3;k++) { r[k] = Dual<3>::variable(rtf[k], k); x[k] = Dual<3>(p_ref[k] - rtf[3 + k]); }
                rotate_point_r_dual(y, r, x, true);
#pragma unroll
                for(int k=0;k<3;k++) r[k] = Dual<3>(rtf[k]);
                rotate_point_r_dual(z, r, y, false);
#pragma unroll
                for(int k=0;k<3;k++) r[k] = Dual<3>(rt0[k]);
                rotate_point_r_dual(w, r, z, false);
                const double inv = 1.0/(double)a.Nframes;
#pragma unroll
                for(int k=0;k<3;k++)
#pragma unroll
                    for(int j=0;j<3;j++)
                    {
                        Frow[k][a.istate_f0 + 6*f + j]     = w[k].d[j]*inv*SCALE_ROTATION_FRAME;
                        Frow[k][a.istate_f0 + 6*f + 3 + j] = -R0[k][j]*inv*SCALE_TRANSLATION_FRAME;
                    }
            }
        }
    }
}

template<int METHOD>
hipError_t launch_tri_pairs(bool with_var, bool with_F, const TriPairsArgs& a, const TriCamDev* cams, const int* pair_cam,
                            const int* pair_row, const double* v, const double* dv_dq, const double* dv_di,
                            const double* frames, double* p, double* var_obs, double* F, hipStream_t st)
{
    const dim3 grid((a.N + TRI_THREADS - 1)/TRI_THREADS), block(TRI_THREADS);
    if constexpr(METHOD == TRI_LINDSTROM)
    {
        if(with_var || with_F) return hipErrorInvalidValue;
        tri_pairs_kernel<METHOD, false, false><<<grid, block, 0, st>>>(a, cams, pair_cam, pair_row, v, dv_dq, dv_di, frames, p, var_obs, F);
    }
    else
    {
        if(with_F)        tri_pairs_kernel<METHOD, true,  true ><<<grid, block, 0, st>>>(a, cams, pair_cam, pair_row, v, dv_dq, dv_di, frames, p, var_obs, F);
        else if(with_var) tri_pairs_kernel<METHOD, true,  false><<<grid, block, 0, st>>>(a, cams, pair_cam, pair_row, v, dv_dq, dv_di, frames, p, var_obs, F);
        else              tri_pairs_kernel<METHOD, false, false><<<grid, block, 0, st>>>(a, cams, pair_cam, pair_row, v, dv_dq, dv_di, frames, p, var_obs, F);
    }
    return hipGetLastError();
}

} // namespace

extern "C" {

bool mrcal_amd_triangulate_geometric(int N, const double* v0, const double* v1, const double* t01,
                                     double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01)
{ return triangulate_host(TRI_GEOMETRIC, "geometric", N, v0, v1, t01, p, dp_dv0, dp_dv1, dp_dt01); }

bool mrcal_amd_triangulate_lindstrom(int N, const double* v0_local, const double* v1_local, const double* Rt01,
                                     double* p, double* dp_dv0, double* dp_dv1, double* dp_dRt01)
{ return triangulate_host(TRI_LINDSTROM, "lindstrom", N, v0_local, v1_local, Rt01, p, dp_dv0, dp_dv1, dp_dRt01); }

bool mrcal_amd_triangulate_leecivera_l1(int N, const double* v0, const double* v1, const double* t01,
                                        double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01)
{ return triangulate_host(TRI_LEECIVERA_L1, "leecivera_l1", N, v0, v1, t01, p, dp_dv0, dp_dv1, dp_dt01); }

bool mrcal_amd_triangulate_leecivera_linf(int N, const double* v0, const double* v1, const double* t01,
                                          double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01)
{ return triangulate_host(TRI_LEECIVERA_LINF, "leecivera_linf", N, v0, v1, t01, p, dp_dv0, dp_dv1, dp_dt01); }

bool mrcal_amd_triangulate_leecivera_mid2(int N, const double* v0, const double* v1, const double* t01,
                                          double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01)
{ return triangulate_host(TRI_LEECIVERA_MID2, "leecivera_mid2", N, v0, v1, t01, p, dp_dv0, dp_dv1, dp_dt01); }

bool mrcal_amd_triangulate_leecivera_wmid2(int N, const double* v0, const double* v1, const double* t01,
                                           double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01)
{ return triangulate_host(TRI_LEECIVERA_WMID2, "leecivera_wmid2", N, v0, v1, t01, p, dp_dv0, dp_dv1, dp_dt01); }

} // extern "C"

struct mrcal_amd_triangulation
{
    struct Camera
    {
        mrcal_lensmodel_t   lensmodel;
        LensConfig          cfg;
        int                 Ni = 0;
        double*             d_intr = NULL;
    };
    std::vector<Camera>               cams;
    std::unique_ptr<NoisePropagation> np;                  // with a problem: its factorization, regularization rows, sigma
    TriCamDev*                        d_cams   = NULL;
    double*                           d_frames = NULL;     // rt_ref_frame [Nframes][6] at the problem's state
    hipStream_t                       stream = NULL;       // without a problem; with one, np's stream is used
    DeviceBuffers                     mem;
    ~mrcal_amd_triangulation()
    {
        mem.free_all();
        if(stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

bool check_cameras(int Ncameras, const mrcal_amd_triangulation_camera_t* cameras)
{
    if(Ncameras < 1 || cameras == NULL) { set_error("mrcal_amd_triangulation_create(): no cameras"); return false; }
    for(int c = 0; c < Ncameras; c++)
    {
        const mrcal_lensmodel_type_t t = cameras[c].lensmodel.type;
        if(!lens_supported((int)t)) { set_error("mrcal_amd_triangulation_create(): lens model %d is not supported", (int)t); return false; }
        if(t == MRCAL_LENSMODEL_CAHVORE)
            for(int i = 9; i < 12; i++)
                if(cameras[c].intrinsics[i] != 0.)
                {
                    set_error("unproject() currently only works with a central projection. So I cannot unproject(CAHVORE,E!=0). Please set E=0 to centralize this model");
                    return false;
                }
    }
    return true;
}

bool check_cameras_against_problem(const mrcal_amd_problem* P, int Ncameras, const mrcal_amd_triangulation_camera_t* cameras)
{
    const Layout& L = P->L;
    if(propagation_refuses_shard(P, "triangulation") || propagation_refuses_measurements(L)) return false;
    for(int c = 0; c < Ncameras; c++)
    {
        if(cameras[c].icam_intrinsics < 0 || cameras[c].icam_intrinsics >= L.dims.Ncameras_intrinsics)
        {
            set_error("icam_intrinsics MUST be in [0,Ncameras_intrinsics-1]. got %d NOT in [0,%d]", cameras[c].icam_intrinsics, L.dims.Ncameras_intrinsics-1);
            return false;
        }
        if(cameras[c].icam_extrinsics >= L.dims.Ncameras_extrinsics)
        {
            set_error("icam_extrinsics MUST be < 0 (at the reference) or in [0,Ncameras_extrinsics-1]. got %d NOT in [0,%d]", cameras[c].icam_extrinsics, L.dims.Ncameras_extrinsics-1);
            return false;
        }
        if(memcmp(&cameras[c].lensmodel, &L.lensmodel, sizeof(mrcal_lensmodel_t)) != 0)
        {
            set_error("triangulation: camera %d does not have the problem's lens model", c);
            return false;
        }
    }
    return true;
}

// each camera's lens parameters, and the table the pair kernel reads. L: the problem's layout, or NULL
bool upload_cameras(mrcal_amd_triangulation* t, const Layout* L, int Ncameras, const mrcal_amd_triangulation_camera_t* cameras)
{
    t->cams.resize((size_t)Ncameras);
    std::vector<TriCamDev> table((size_t)Ncameras);
    for(int c = 0; c < Ncameras; c++)
    {
        mrcal_amd_triangulation::Camera& cam = t->cams[c];
        cam.lensmodel = cameras[c].lensmodel;
        cam.cfg       = lens_config_of(cam.lensmodel);
        cam.Ni        = lensmodel_num_params(cam.lensmodel);
        if(!t->mem.upload(&cam.d_intr, cameras[c].intrinsics, (size_t)cam.Ni)) return false;
        for(int k = 0; k < 6; k++) table[c].rt[k] = cameras[c].rt_cam_ref[k];
        table[c].istate_i = table[c].istate_e = -1;
        if(L != NULL)
        {
            if(L->i_state_intrinsics >= 0 && L->Nintr_state > 0)
                table[c].istate_i = L->i_state_intrinsics + cameras[c].icam_intrinsics*L->Nintr_state;
            if(L->i_state_extrinsics >= 0 && cameras[c].icam_extrinsics >= 0)
                table[c].istate_e = L->i_state_extrinsics + 6*cameras[c].icam_extrinsics;
        }
    }
    return t->mem.upload(&t->d_cams, table);
}

// the frames at the problem's state, if they are in it
bool upload_frames(mrcal_amd_triangulation* t, mrcal_amd_problem* P)
{
    const Layout& L = P->L;
    if(!L.sel.do_optimize_frames || L.dims.Nframes == 0) return true;
    ProblemStateArrays s;
    return problem_state_arrays(P, &s) && t->mem.upload(&t->d_frames, (const double*)s.rt_ref_frame.data(), (size_t)6*L.dims.Nframes);
}

} // namespace

extern "C" {

mrcal_amd_triangulation_t*
mrcal_amd_triangulation_create(mrcal_amd_problem_t* P, int Ncameras, const mrcal_amd_triangulation_camera_t* cameras)
{
    last_error_string().clear();
    if(mrcal_amd_device_count() <= 0)
    {
        set_error("no HIP device is visible: libmrcal_amd has no CPU fallback");
        return NULL;
    }
    if(!check_cameras(Ncameras, cameras)) return NULL;
    if(P != NULL && !check_cameras_against_problem(P, Ncameras, cameras)) return NULL;

    std::unique_ptr<mrcal_amd_triangulation> t(new mrcal_amd_triangulation());
    if(!upload_cameras(t.get(), P ? &P->L : NULL, Ncameras, cameras)) return NULL;
    if(P == NULL)
    {
        HIP_TRY(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking), return NULL);
        return t.release();
    }
    t->np = NoisePropagation::create(P, "triangulation", true);
    if(!t->np || !upload_frames(t.get(), P)) return NULL;
    return t.release();
}

double mrcal_amd_triangulation_observed_pixel_uncertainty(const mrcal_amd_triangulation_t* t)
{
    return t && t->np ? t->np->sigma_estimate : -1.0;
}

} // extern "C"

namespace {

// what one evaluate() asks for
struct TriRequest
{
    int    N, method;
    bool   with_cal, with_obs, stabilize;
    double sigma;                   // of the calibration-time noise, if with_cal
    double obs_stdev, obs_correlation;
    NoisePropagation* np;           // the context's, if with_cal; else NULL
    bool   grads() const { return with_cal || with_obs; }
};

bool check_request(TriRequest* r, const mrcal_amd_triangulation* t, const double* q, const int* icam,
                   double q_calibration_stdev, const double* p, const double* Var_p_observation, const double* Var_p_calibration)
{
    if(t == NULL) { set_error("no triangulation context"); return false; }
    if(r->method < 0 || r->method >= TRI_NMETHODS) { set_error("unknown triangulation method %d", r->method); return false; }
    r->with_cal = q_calibration_stdev != 0.0;
    r->with_obs = r->obs_stdev > 0.0;
    if(r->obs_stdev < 0.0) { set_error("q_observation_stdev MUST be None or >= 0"); return false; }
    if(r->method == TRI_LINDSTROM && r->grads())
    {
        set_error("Triangulation gradients not supported (yet?) with method=triangulate_lindstrom. It has slightly different inputs and slightly different gradients");
        return false;
    }
    if(r->with_cal && !t->np)
    {
        set_error("optimization_inputs are not available, so I cannot propagate calibration-time noise");
        return false;
    }
    if(r->N < 0 || (r->N > 0 && (q == NULL || icam == NULL || p == NULL)) || (r->with_obs && Var_p_observation == NULL) ||
       (r->with_cal && Var_p_calibration == NULL))
    {
        set_error("mrcal_amd_triangulation_evaluate(): N >= 0, and q, icam, p and the covariances asked for must be given");
        return false;
    }
    r->sigma = q_calibration_stdev;
    if(r->with_cal && !(r->sigma > 0.0))
    {
        if(!(t->np->sigma_estimate > 0.0)) { set_error_no_sigma_estimate(); return false; }
        r->sigma = t->np->sigma_estimate;
    }
    r->np = r->with_cal ? t->np.get() : NULL;
    return true;
}

// the temporaries of one evaluate(): NULL where the request has no use for one
struct TriBuffers
{
    DeviceBuffers mem;
    double *q = NULL, *v = NULL, *gq = NULL, *gi = NULL, *s_q = NULL, *s_gv = NULL, *s_gi = NULL;
    double *p = NULL, *vo = NULL, *F = NULL, *X = NULL, *FX = NULL, *JX = NULL, *var = NULL;
    int    *cam = NULL, *row = NULL;
};
// iterative: a camera in use has no closed-form unprojection
bool allocate(TriBuffers* b, const TriRequest& r, const PixelsByCamera& g, const int* icam, bool iterative)
{
    const size_t N = (size_t)r.N, n3 = 3*N;
    bool ok = b->mem.upload(&b->q, g.qs) && b->mem.upload(&b->cam, icam, 2*N) && b->mem.upload(&b->row, g.rows) &&
              b->mem.alloc(&b->v, 6*N) && b->mem.alloc(&b->p, 3*N);
    if(r.grads()) ok = ok && b->mem.alloc(&b->gq, 12*N) && b->mem.alloc(&b->vo, 9*N);
    if(r.grads() && iterative) ok = ok && b->mem.alloc(&b->s_q, 4*N) && b->mem.alloc(&b->s_gv, 12*N);
    if(r.with_cal)
    {
        const size_t Ni = (size_t)r.np->L.Nintrinsics, Nstate = (size_t)r.np->L.Nstate;
        ok = ok && b->mem.alloc(&b->gi, 6*N*Ni) && b->mem.alloc(&b->F, n3*Nstate) && b->mem.alloc(&b->X, n3*Nstate) &&
             b->mem.alloc(&b->FX, n3*n3) && b->mem.alloc(&b->JX, (size_t)std::max(r.np->Nreg, 1)*n3) && b->mem.alloc(&b->var, n3*n3);
        if(iterative) ok = ok && b->mem.alloc(&b->s_gi, 4*N*Ni);
    }
    return ok;
}

// each camera's pixels -> its rows of v, dv_dq, dv_di
bool unproject_by_camera(const mrcal_amd_triangulation* t, const TriRequest& r, const PixelsByCamera& g, const TriBuffers& b, hipStream_t st)
{
    const int Ni = r.with_cal ? r.np->L.Nintrinsics : 0;
    for(int c = 0; c < (int)t->cams.size(); c++)
    {
        const int n = g.off[c + 1] - g.off[c], o = g.off[c];
        if(n == 0) continue;
        const mrcal_amd_triangulation::Camera& cam = t->cams[c];
        const int ni = r.with_cal ? Ni : cam.Ni;
        HIP_TRY(launch_unproject_points((int)cam.lensmodel.type, cam.cfg, n, ni, b.q + (size_t)2*o, cam.d_intr, b.v + (size_t)3*o,
                                        r.grads() ? b.gq + (size_t)6*o : NULL, r.with_cal ? b.gi + (size_t)3*o*Ni : NULL,
                                        b.s_q ? b.s_q + (size_t)2*o : NULL, b.s_gv ? b.s_gv + (size_t)6*o : NULL,
                                        b.s_gi ? b.s_gi + (size_t)2*o*Ni : NULL, false, st), return false);
    }
    return true;
}

TriPairsArgs pairs_args(const TriRequest& r)
{
    TriPairsArgs a;
    memset(&a, 0, sizeof(a));
    a.N = r.N;
    a.var = r.obs_stdev*r.obs_stdev;
    const double sc = r.obs_stdev*r.obs_correlation;
    a.var_cross = sc*sc;
    if(!r.with_cal) return a;
    const Layout* L = &r.np->L;
    a.Ni          = L->Nintrinsics;
    a.Nstate      = L->Nstate;
    a.Nintr_state = L->Nintr_state;
    a.intr0       = L->Ncore - L->Ncore_state;
    a.Ncore_state = L->Ncore_state;
    a.stabilize   = r.stabilize ? 1 : 0;
    if(r.stabilize && L->sel.do_optimize_frames && L->i_state_frames >= 0 && L->dims.Nframes > 0)
    {
        a.Nframes   = L->dims.Nframes;
        a.istate_f0 = L->i_state_frames;
    }
    return a;
}

bool launch_pairs(const mrcal_amd_triangulation* t, const TriRequest& r, const TriPairsArgs& a, const TriBuffers& b, hipStream_t st)
{
    hipError_t e = hipErrorInvalidValue;
    switch(r.method)
    {
#define TRI_CASE(M) case M: e = launch_tri_pairs<M>(r.grads(), r.with_cal, a, t->d_cams, b.cam, b.row, b.v, b.gq, b.gi, t->d_frames, b.p, b.vo, b.F, st); break;
    TRI_CASE(TRI_GEOMETRIC) TRI_CASE(TRI_LINDSTROM) TRI_CASE(TRI_LEECIVERA_L1) TRI_CASE(TRI_LEECIVERA_LINF)
    TRI_CASE(TRI_LEECIVERA_MID2) TRI_CASE(TRI_LEECIVERA_WMID2)
#undef TRI_CASE
    }
    HIP_TRY(e, return false);
    return true;
}

// everything of one evaluate() that is queued on st; nothing is waited for
bool queue_evaluate(const mrcal_amd_triangulation* t, const TriRequest& r, const PixelsByCamera& g, const TriBuffers& b, hipStream_t st,
                    double* p, double* Var_p_observation, double* Var_p_calibration)
{
    NoisePropagation* np = r.np;
    const int n3 = 3*r.N;
    if(!unproject_by_camera(t, r, g, b, st) || !launch_pairs(t, r, pairs_args(r), b, st)) return false;
    if(np != NULL)
    {
        if(!np->solve(b.F, n3, b.X) || !np->row_dots(b.F, n3, b.X, n3, b.FX) || !np->reg_rows_times(b.X, n3, b.JX) ||
           !np->combine(b.FX, b.JX, n3, r.sigma, b.var))
            return false;
        HIP_TRY(hipMemcpyAsync(Var_p_calibration, b.var, (size_t)n3*n3*sizeof(double), hipMemcpyDeviceToHost, st), return false);
    }
    HIP_TRY(hipMemcpyAsync(p, b.p, (size_t)n3*sizeof(double), hipMemcpyDeviceToHost, st), return false);
    if(r.with_obs) HIP_TRY(hipMemcpyAsync(Var_p_observation, b.vo, (size_t)9*r.N*sizeof(double), hipMemcpyDeviceToHost, st), return false);
    return true;
}

} // namespace

extern "C" {

bool mrcal_amd_triangulation_evaluate(mrcal_amd_triangulation_t* t, int N, const double* q, const int* icam, int method,
                                      double q_calibration_stdev, double q_observation_stdev, double q_observation_stdev_correlation,
                                      bool stabilize_coords, double* p, double* Var_p_observation, double* Var_p_calibration)
{
    last_error_string().clear();
    TriRequest r = { N, method, false, false, stabilize_coords, 0.0, q_observation_stdev, q_observation_stdev_correlation, NULL };
    if(!check_request(&r, t, q, icam, q_calibration_stdev, p, Var_p_observation, Var_p_calibration)) return false;
    if(N == 0) return true;
    const int Ncameras = (int)t->cams.size();
    PixelsByCamera g;
    const int bad = group_pixels_by_camera(&g, Ncameras, N, q, icam);
    if(bad >= 0) { set_error("pair %d: camera %d is not in the table of %d", bad/2, icam[bad], Ncameras); return false; }
    bool iterative = false;
    for(int c = 0; c < Ncameras; c++)
        if(g.off[c + 1] > g.off[c] && !lens_has_closed_form_inverse(t->cams[c].lensmodel.type)) iterative = true;

    hipStream_t st = t->np ? t->np->stream : t->stream;
    TriBuffers b;
    if(!allocate(&b, r, g, icam, iterative)) return false;
    bool ok = queue_evaluate(t, r, g, b, st, p, Var_p_observation, Var_p_calibration);
    // (also on failure: the temporaries are freed on return, and nothing queued may still be using them)
    if(hipStreamSynchronize(st) != hipSuccess && ok) { set_error("mrcal_amd_triangulation_evaluate(): the device reported an error"); ok = false; }
    return ok;
}

void mrcal_amd_triangulation_destroy(mrcal_amd_triangulation_t* t) { delete t; }

} // extern "C"
