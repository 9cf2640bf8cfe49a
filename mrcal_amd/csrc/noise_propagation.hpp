// The propagation of calibration-time noise through the resident factorization
// (_propagate_calibration_uncertainty(), mrcal/model_analysis.py:560-870), for every analysis that needs it:
// projection_uncertainty.hip, triangulation.hip. With F (n x Nstate) the gradient of the n quantities with respect to
// the packed state, and J*[obs]^T J*[obs] = J*^T J* - J*[reg]^T J*[reg] (the reference's own derivation, :645-660):
//
//   X   = (J*^T J*)^-1 F^T                                        n right-hand sides on the resident factorization
//   Var = sigma^2 ( sym(F X) - (J*[reg] X)^T (J*[reg] X) )        only the regularization rows of J are read
//
// A NoisePropagation is made from a problem at its current state and owns what it holds: its destructor is the only
// clean-up. Its steps take device pointers, queue on stream and wait for nothing. HOST code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <memory>
#include "layout.hpp"
#include "device_memory.hpp"
#include "../../include/mrcal_amd.h"

struct mrcal_amd_problem;

namespace mrcal_amd {

// factorization.cpp: the stream a factorization's work is queued on; Nrhs right-hand sides [Nrhs][Nstate] that are
// on the device -> solutions that stay there
hipStream_t factorization_stream(mrcal_amd_factorization_t* f);
bool factorization_solve_device(mrcal_amd_factorization_t* f, int sys, const double* d_bt, int Nrhs, double* d_xt);
// projection_uncertainty.hip: evaluate() on device pointers: p_cam [N][3] in, out [N][4] (covariance) or [N], queued on
// the caller's stream and not waited for. (C and the camera's intrinsics were complete when _create() returned: any
// stream may read them)
bool uncertainty_evaluate_device(mrcal_amd_uncertainty_t* u, const double* d_p_cam, int N, bool atinfinity, int what,
                                 double* d_out, hipStream_t stream);

// The refusals of a problem that cannot be propagated through, with the reference's messages; who: the caller's name
// in them. create() makes both; a caller with checks of its own between them makes them there first
bool propagation_refuses_shard(const mrcal_amd_problem* P, const char* who);
bool propagation_refuses_measurements(const Layout& L);

struct NoisePropagation
{
    Layout                     L;                       // of the problem
    mrcal_amd_factorization_t* f      = NULL;           // of J*^T J* at the problem's state
    hipStream_t                stream = NULL;           // the factorization's
    int                        Nreg   = 0;              // the regularization rows of J: a copy
    int32_t                    reg_e0 = 0;              // their first entry in the problem's CSR
    int32_t*                   d_regJp = NULL;          // [Nreg + 1], as in the problem's CSR
    int32_t*                   d_regJi = NULL;          // the entries from reg_e0 on
    double*                    d_regJx = NULL;
    double                     sigma_estimate = -1.0;   // the observed pixel uncertainty; -1: not asked for, or no observations to estimate from
    DeviceBuffers              mem;
    ~NoisePropagation();

    // Evaluates x and J at the problem's state if need be, factors, copies the regularization rows and (want_sigma)
    // estimates sigma. Nothing of the problem is read once this has returned. NULL: set_error() says why
    static std::unique_ptr<NoisePropagation> create(mrcal_amd_problem* P, const char* who, bool want_sigma);

    // X [n][Nstate] = (J*^T J*)^-1 F^T
    bool solve(const double* d_F, int n, double* d_X);
    // out [na][nb] = A[a] . B[b], rows of length Nstate: a wavefront an entry, lane l sums s = l, l+64, ... in order, then a fixed butterfly
    bool row_dots(const double* d_A, int na, const double* d_B, int nb, double* d_out);
    // JX [Nreg][n] = J*[reg] X: a lane per (row, column), the row's entries in CSR order. Nothing if Nreg == 0
    bool reg_rows_times(const double* d_X, int n, double* d_JX);
    // out [n][n] = ( (MX[a][b] + MX[b][a])/2 - sum_r JX[r][a] JX[r][b] ) sigma^2: a lane an entry, r ascending
    bool combine(const double* d_MX, const double* d_JX, int n, double sigma, double* d_out);
};

// "no observations to estimate sigma from", raised by each caller where the estimate is first needed
void set_error_no_sigma_estimate();

}
