// By which route the camera block (the Schur complement S of a trial step) is factored: decided HERE, once per queued
// step, from a handful of ints and bools; the launchers (step.hip, cholesky_large.hip) only read the result. HOST code:
// no HIP runtime call, no problem object; tests/test_camblock_route.py executes it on the CPU.
//   the one-workgroup LDS Cholesky (cholesky_lds.hip), with or without the packed copy of S    in_lds (S_packed)
//   the launch-per-panel Cholesky (cholesky_large.hip), plain                                   nothing else set
//   ... of the camera block without its isolated variables (LcholCompact, lchol_tail_kernel)     compact (with_tail)
//   ... and in a nested-dissection order (lchol_nd_*)                                            nd_launches
//   ... with the solve by the backward sweep                                                     sweep
#pragma once

namespace mrcal_amd {

// what the host provided launches of the dissection for: [0] rounds (panels a side; 0: none - the plans are made and not
// used) | [1] the largest separator
struct NdLimits { int rounds, ns_max; };

// What the problem allows at present (FactorBuffers::mode). That a buffer is allocated says nothing about it: the
// buffers stay the problem's when a mode goes off (problem_set_camblock_mode())
struct CamBlockMode
{
    bool compact;   // the splined models: S without the control points no board covers (spl_compact_kernel makes OpDev::cperm)
    bool dissect;   // ... and in a nested-dissection order where a point's plan fits (OpDev::ndp). Only with compact
    bool sweep;     // the large Cholesky's solve by the backward sweep in groups of panels (backward stable; slower: no explicit
                    // L^-1, no compaction, the end-of-trial logic in launches of its own) instead of d = -Y^T z. Set by the
                    // automatic fallback (solver.cpp: a factor whose diagonal spans more than 1e10) or by a test hook
};

struct CamBlockRoute
{
    bool in_lds;         // the one-workgroup LDS Cholesky serves (chol_fits_lds())
    bool finish_rides;   // the end-of-trial logic rides in the reduction's launch
    bool S_packed;       // the reduction leaves a packed copy of S (factor_S_packed()) that the one-workgroup Cholesky reads
    bool compact;        // the reduction and the factorization go by FactorBuffers::cperm_cur / iso
    bool nd_plans;       // the reduction keeps the plan of the point it reduced (FactorBuffers::ndp_cur) ...
    bool nd_launches;    // ... and the dissection's launches follow it (FactorBuffers::nd_lim)
    bool sweep;
    bool with_tail;      // the launches past l_last are lchol_tail_kernel's
    int  likely_panels;  // launches of the large Cholesky the host provides one by one (learn_likely_size()); 0: all
    int  l_last;         // the last of lchol_panel_kernel's launches
};

#define CAMBLOCK_PANEL 64        // = LCH_NB: columns of a panel of the launch-per-panel Cholesky

// false: a combination that does not exist - the compaction with the backward sweep (which knows nothing of a size the
// device decides) or sharded (the ranks sum their camera blocks entry by entry: no rank puts its own in another
// order), a dissection of what is not compacted
bool camblock_route(CamBlockRoute* out, int Nc, bool sharded, const CamBlockMode& mode,
                    NdLimits provided, int lchol_likely_panels, int nd_likely_panels);

} // namespace mrcal_amd
