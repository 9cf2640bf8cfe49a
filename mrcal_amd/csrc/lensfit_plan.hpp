// What lensfit.hip works out on the host before it touches the device: which (PROJ, NDIST) row of the lens table the
// kernel is instantiated with, which intrinsics are unknowns, how many unknowns each of the two stages of a trial has,
// the threads of a workgroup, the chunk of Jacobian rows it stages in LDS, the LDS it takes, the measurement counts
// the reference's rms is divided by, and what is refused. Plain structs in and out, no HIP type or call.
// tests/hostcheck/lensfit_plan_check.cpp runs it under the host sanitizers.
//
// The fit (include/mrcal_amd.h, "lens-model fit"): N fixed points, 2 pixel rows each, the unknowns
//   intrinsics[ivar0 .. Nintrinsics)     ivar0 = 0, or 4 when the core (fx,fy,cx,cy) is not optimized
//   rt_cam_ref[0 .. 6)                   stage 2 only, when the pose is optimized
// A staged row holds the NP active columns of J and the residual x behind them: W = NP + 1 doubles, and the kernel sums
// the upper triangle of [J x]^T [J x] - J^T J, J^T x and x.x at once: NE = (NP + 1)(NP + 2)/2 sums, one a thread.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "lens_dispatch.hpp"

namespace mrcal_amd {

enum { LENSFIT_CONVERGED = 0, LENSFIT_BOUND = 1, LENSFIT_TOO_FEW_POINTS = 2, LENSFIT_STALLED = 3 };

// what a workgroup may take of the LDS in all (the device has 160 KiB a CU; 64 KiB needs no opt-in at launch), what
// the kernel's own state takes of that (lensfit.hip asserts that it fits), and the rest: the staged rows
#define LENSFIT_LDS_BYTES        65536
#define LENSFIT_STATE_LDS_BYTES  12288
#define LENSFIT_NP_MAX           22                 // OPENCV12 with its core and a pose
#define LENSFIT_THREADS_MIN      256
#define LENSFIT_CHUNK_ROWS_MAX   (2*LENSFIT_THREADS_MIN)    // a lane forms the two rows of a point
#define LENSFIT_DEFAULT_MAX_EVALUATIONS 200
#define LENSFIT_MAX_TRIALS       65536
#define LENSFIT_MAX_POINTS       (1 << 24)

struct LensfitPlan
{
    int    proj = -1, ndist = -1;   // the row of for_parametric_lens() the kernel is instantiated with
    int    Nintrinsics = 0;         // 4 + ndist
    int    ivar0 = 0;               // the first intrinsic that is an unknown
    int    Nstages = 0;             // 1: the intrinsics alone; 2: then with the pose
    int    NP[2] = { 0, 0 };        // unknowns of each stage (stage 1 with NP = 0 is skipped: nothing to fit yet)
    int    NE = 0;                  // sums of the larger stage
    int    threads = 0;
    int    row_doubles = 0;         // W of the larger stage: the pitch of a staged row
    int    chunk_rows = 0;          // C: rows staged at a time, a multiple of 64
    size_t rows_lds_bytes = 0;      // C W 8: dynamic
    size_t lds_bytes = 0;           // with the kernel's own state
    int    Nreg_distortion = 0, Nreg_centerpixel = 0;       // regularization rows
    int    Nmeasurements = 0;       // 2 N + the regularization rows: what the rms is divided by
};

inline int lensfit_num_sums(int NP) { return (NP + 1)*(NP + 2)/2; }

// false: refused, with the reason in *error
inline bool lensfit_plan(LensfitPlan* plan, std::string* error, const mrcal_lensmodel_t& lensmodel, int N, int Ntrials,
                         const int imagersize[2], bool optimize_core, bool optimize_extrinsics, bool apply_regularization)
{
    *plan = LensfitPlan();
    char buf[256];
    buf[0] = 0;
    int proj = -1, ndist = -1;
    const bool parametric = for_parametric_lens((int)lensmodel.type, [&](auto k) { proj = decltype(k)::PROJ; ndist = decltype(k)::NDIST; });
    if(lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
        snprintf(buf, sizeof(buf), "lens-model fit: a splined model has thousands of unknowns, each seen by a few points: it is fitted by optimize(), not by this kernel");
    else if(!parametric)
        snprintf(buf, sizeof(buf), "lens-model fit: lens model %d is not supported", (int)lensmodel.type);
    else if(N < 1 || N > LENSFIT_MAX_POINTS)
        snprintf(buf, sizeof(buf), "lens-model fit: %d points cannot be fitted (1 to %d)", N, LENSFIT_MAX_POINTS);
    else if(Ntrials < 1 || Ntrials > LENSFIT_MAX_TRIALS)
        snprintf(buf, sizeof(buf), "lens-model fit: %d trials cannot be run in one call (1 to %d)", Ntrials, LENSFIT_MAX_TRIALS);
    else if(imagersize[0] < 1 || imagersize[1] < 1)
        snprintf(buf, sizeof(buf), "lens-model fit: an imager of %d x %d pixels", imagersize[0], imagersize[1]);
    if(buf[0] == 0)
    {
        plan->proj = proj; plan->ndist = ndist;
        plan->Nintrinsics = 4 + ndist;
        plan->ivar0       = optimize_core ? 0 : 4;
        plan->Nstages     = optimize_extrinsics ? 2 : 1;
        plan->NP[0]       = plan->Nintrinsics - plan->ivar0;
        plan->NP[1]       = optimize_extrinsics ? plan->NP[0] + 6 : 0;
        const int NPmax   = plan->NP[plan->Nstages - 1];
        if(NPmax == 0)
            snprintf(buf, sizeof(buf), "lens-model fit: nothing to fit: this model has no distortion terms, and neither its core nor the pose is optimized");
        else if(2*(int64_t)N < NPmax)
            snprintf(buf, sizeof(buf), "lens-model fit: %d points give %d pixel rows: fewer than the %d unknowns", N, 2*N, NPmax);
        else
        {
            plan->NE          = lensfit_num_sums(NPmax);
            plan->threads     = plan->NE > LENSFIT_THREADS_MIN ? (plan->NE + 63)/64*64 : LENSFIT_THREADS_MIN;
            plan->row_doubles = NPmax + 1;
            const size_t room = LENSFIT_LDS_BYTES - LENSFIT_STATE_LDS_BYTES;
            int C = (int)(room/(8*(size_t)plan->row_doubles))/64*64;
            if(C > LENSFIT_CHUNK_ROWS_MAX) C = LENSFIT_CHUNK_ROWS_MAX;
            plan->chunk_rows     = C;
            plan->rows_lds_bytes = (size_t)C*plan->row_doubles*8;
            plan->lds_bytes      = plan->rows_lds_bytes + LENSFIT_STATE_LDS_BYTES;
            // mrcal.c:5681-5689: the distortion terms when there are any to optimize, the centre pixel with the core
            plan->Nreg_distortion  = apply_regularization ? ndist : 0;
            plan->Nreg_centerpixel = apply_regularization && optimize_core ? 2 : 0;
            plan->Nmeasurements    = 2*N + plan->Nreg_distortion + plan->Nreg_centerpixel;
        }
    }
    if(buf[0] == 0) return true;
    *plan = LensfitPlan();
    *error = buf;
    return false;
}

// The regularization row of distortion term j: x = scale k_j (mrcal.c:5787-5850). The terms of the denominator of the
// rational models (OPENCV8 and up, j = 5..7) five times as strongly
inline double lensfit_distortion_scale(int lens_type, int j)
{
    const bool rational = (lens_type == MRCAL_LENSMODEL_OPENCV8 || lens_type == MRCAL_LENSMODEL_OPENCV12) && 5 <= j && j <= 7;
    return rational ? 0.1*5. : 0.1;
}
// ... and of the centre pixel: x = scale (c - (size - 1)/2), BOTH with the imager's width (mrcal.c:5859)
inline double lensfit_centerpixel_scale(const int imagersize[2]) { return 0.1/((double)imagersize[0]*0.1); }

} // namespace mrcal_amd
