// noise_propagation.hpp: the context and the steps. Kernels:
//   np_sigma_kernel      the sigma estimate's sum of squares (model_analysis.py:491-557): one workgroup, fixed tree
//   np_row_dots_kernel   a wavefront a dot product, fixed-order sum
//   np_reg_rows_kernel   J*[reg] X: a lane per (row, column), the row's entries in CSR order
//   np_combine_kernel    a lane an entry: symmetrized, the regularization rows summed in row order
// Nothing uses floating-point atomics: every result is the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <vector>
#include "noise_propagation.hpp"
#include "problem_object.hpp"
#include "host_state.hpp"

using namespace mrcal_amd;

namespace {

// sum of squares and count of the board and point measurements whose observation has a positive weight
// (measurements_board() / measurements_point(), mrcal/utils.py:1286-1500). One workgroup of 256, fixed order
__global__ __launch_bounds__(256)
void np_sigma_kernel(int Ncorners, const double* __restrict__ board_pool, int i_meas_boards,
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

// out[a][b] = sum_s A[a][s] B[b][s]: a wavefront per (a,b)
__global__ __launch_bounds__(256)
void np_row_dots_kernel(int na, int nb, int Nstate, const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ out)
{
    const int64_t w = (int64_t)blockIdx.x*(blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if(w >= (int64_t)na*nb) return;
    const int ra = (int)(w / nb), rb = (int)(w % nb);
    const double* __restrict__ Aa = A + (size_t)ra*Nstate;
    const double* __restrict__ Bb = B + (size_t)rb*Nstate;
    double s = 0.0;
    for(int i = lane; i < Nstate; i += 64) s += Aa[i]*Bb[i];
    for(int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if(lane == 0) out[w] = s;
}
// JX[r][a] = sum over the entries of regularization row r of J[r][c] X[a][c], in CSR order. Jp: the rows' own
// row pointers, whose entries start at e0 of the problem's CSR (Ji, Jx hold them from 0)
__global__ __launch_bounds__(256)
void np_reg_rows_kernel(int Nreg, int n, int Nstate, const int32_t* __restrict__ Jp, int32_t e0, const int32_t* __restrict__ Ji,
                        const double* __restrict__ Jx, const double* __restrict__ X, double* __restrict__ JX)
{
    const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= (int64_t)Nreg*n) return;
    const int r = (int)(i / n), c = (int)(i % n);
    const double* __restrict__ Xc = X + (size_t)c*Nstate;
    double s = 0.0;
    for(int32_t e = Jp[r] - e0; e < Jp[r + 1] - e0; e++) s += Jx[e]*Xc[Ji[e]];
    JX[i] = s;
}
// out[a][b] = sigma^2 ( (MX[a][b] + MX[b][a])/2 - sum_r JX[r][a] JX[r][b] )
__global__ __launch_bounds__(256)
void np_combine_kernel(int n, int Nreg, double sigma, const double* __restrict__ MX, const double* __restrict__ JX, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
    if(i >= (int64_t)n*n) return;
    const int ra = (int)(i / n), rb = (int)(i % n);
    double s = 0.0;
    for(int r = 0; r < Nreg; r++) s += JX[(size_t)r*n + ra]*JX[(size_t)r*n + rb];
    out[i] = (0.5*(MX[(size_t)ra*n + rb] + MX[(size_t)rb*n + ra]) - s)*sigma*sigma;
}

// The copy of the regularization rows of J (the problem's stream has been waited for), queued on np->stream
bool copy_regularization_rows(NoisePropagation* np, mrcal_amd_problem* P)
{
    const Layout& L = np->L;
    np->Nreg = L.Nmeas_regularization;
    if(np->Nreg == 0) return true;
    std::vector<int32_t> Jp((size_t)np->Nreg + 1);
    HIP_TRY(hipMemcpy(Jp.data(), P->d_Jp + L.i_meas_regularization, Jp.size()*sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    np->reg_e0 = Jp[0];
    const size_t n = (size_t)(Jp[np->Nreg] - Jp[0]);
    if(!np->mem.upload(&np->d_regJp, Jp) || !np->mem.alloc(&np->d_regJi, n) || !np->mem.alloc(&np->d_regJx, n)) return false;
    if(n == 0) return true;
    HIP_TRY(hipMemcpyAsync(np->d_regJi, P->d_Ji + Jp[0], n*sizeof(int32_t), hipMemcpyDeviceToDevice, np->stream), return false);
    HIP_TRY(hipMemcpyAsync(np->d_regJx, P->op[P->icur].Jv + Jp[0], n*sizeof(double), hipMemcpyDeviceToDevice, np->stream), return false);
    return true;
}

// The estimate of the observed pixel uncertainty (model_analysis.py:491-557): the sums over the board and point
// measurements of x at the problem's operating point, then RMS / sqrt(1 - Nstate/Nmeasurements). Waits for np->stream
bool estimate_sigma(NoisePropagation* np, mrcal_amd_problem* P)
{
    const Layout& L = np->L;
    DeviceBuffers tmp;
    double* d_sig = NULL;
    double sig[2] = { 0.0, 0.0 };
    if(!tmp.alloc(&d_sig, 2)) return false;
    hipLaunchKernelGGL(np_sigma_kernel, dim3(1), dim3(256), 0, np->stream,
                       L.dims.Nobservations_board*L.dims.object_width_n*L.dims.object_height_n, P->d_board_pool, L.i_meas_boards,
                       L.dims.Nobservations_point, P->d_point_pool, L.i_meas_points, P->op[P->icur].x, d_sig);
    HIP_TRY(hipGetLastError(), return false);
    HIP_TRY(hipMemcpyAsync(sig, d_sig, 2*sizeof(double), hipMemcpyDeviceToHost, np->stream), return false);
    HIP_TRY(hipStreamSynchronize(np->stream), return false);
    // (no observations to estimate from: an error only once the estimate is asked for)
    if(sig[1] != 0.0) np->sigma_estimate = sqrt(sig[0]/sig[1]) / sqrt(1.0 - (double)L.Nstate/sig[1]);
    return true;
}

} // namespace

namespace mrcal_amd {

bool propagation_refuses_shard(const mrcal_amd_problem* P, const char* who)
{
    if((int)P->board_sel.size() == P->L.dims.Nobservations_board && P->comm == NULL) return false;
    set_error("%s: this problem is a shard (it holds a part of the rows)", who);
    return true;
}
bool propagation_refuses_measurements(const Layout& L)
{
    if(L.Nmeas_triangulated > 0)
    {
        set_error("Some measurements other than boards, points and regularization are present. Don't know what to do");
        return true;
    }
    if(L.Nmeas_regularization > 0 && L.Nmeas_boards + L.Nmeas_points == 0)
    {
        set_error("No non-regularization measurements. Don't know what to do");
        return true;
    }
    return false;
}
void set_error_no_sigma_estimate()
{
    set_error("observed_pixel_uncertainty cannot be computed because we don't have any board or point observations");
}

NoisePropagation::~NoisePropagation()
{
    mem.free_all();
    if(f) mrcal_amd_factorization_destroy(f);
}

std::unique_ptr<NoisePropagation> NoisePropagation::create(mrcal_amd_problem* P, const char* who, bool want_sigma)
{
    if(propagation_refuses_shard(P, who) || propagation_refuses_measurements(P->L)) return nullptr;
    std::unique_ptr<NoisePropagation> np(new NoisePropagation());
    np->L = P->L;
    // the factorization at the problem's state (evaluates x and J there: with values, whatever the solver's
    // Jacobian stream was set to)
    np->f = mrcal_amd_factorization_create_from_problem(P);
    if(np->f == NULL)
    {
        if(mrcal_amd_factorization_last_status() == 1)
            set_error("Cannot compute the uncertainty: factorization computation failed");
        return nullptr;
    }
    np->stream = factorization_stream(np->f);
    if(!problem_ensure_jacobian(P)) return nullptr;
    // (the problem's stream wrote x and J: the factorization's stream is not ordered behind it)
    HIP_TRY(hipStreamSynchronize(P->stream), return nullptr);
    if(!copy_regularization_rows(np.get(), P)) return nullptr;
    if(want_sigma && !estimate_sigma(np.get(), P)) return nullptr;
    HIP_TRY(hipStreamSynchronize(np->stream), return nullptr);
    return np;
}

bool NoisePropagation::solve(const double* d_F, int n, double* d_X)
{
    return factorization_solve_device(f, FSOLVE_A, d_F, n, d_X);
}
bool NoisePropagation::row_dots(const double* d_A, int na, const double* d_B, int nb, double* d_out)
{
    const int64_t nw = (int64_t)na*nb;
    hipLaunchKernelGGL(np_row_dots_kernel, dim3((unsigned)((nw + 3)/4)), dim3(256), 0, stream, na, nb, L.Nstate, d_A, d_B, d_out);
    HIP_TRY(hipGetLastError(), return false);
    return true;
}
bool NoisePropagation::reg_rows_times(const double* d_X, int n, double* d_JX)
{
    const int64_t ne = (int64_t)Nreg*n;
    if(ne == 0) return true;
    hipLaunchKernelGGL(np_reg_rows_kernel, dim3((unsigned)((ne + 255)/256)), dim3(256), 0, stream, Nreg, n, L.Nstate,
                       d_regJp, reg_e0, d_regJi, d_regJx, d_X, d_JX);
    HIP_TRY(hipGetLastError(), return false);
    return true;
}
bool NoisePropagation::combine(const double* d_MX, const double* d_JX, int n, double sigma, double* d_out)
{
    const int64_t ne = (int64_t)n*n;
    hipLaunchKernelGGL(np_combine_kernel, dim3((unsigned)((ne + 255)/256)), dim3(256), 0, stream, n, Nreg, sigma, d_MX, d_JX, d_out);
    HIP_TRY(hipGetLastError(), return false);
    return true;
}

}
