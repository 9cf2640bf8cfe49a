// camblock_route(): see camblock_route.hpp
#include "chol_diag16.hpp"

namespace mrcal_amd {

bool camblock_route(CamBlockRoute* out, int Nc, bool sharded, const CamBlockMode& mode,
                    NdLimits provided, int lchol_likely_panels, int nd_likely_panels)
{
    if(mode.compact && (mode.sweep || sharded)) return false;
    if(mode.dissect && !mode.compact) return false;
    const int npanels = (Nc + CAMBLOCK_PANEL - 1)/CAMBLOCK_PANEL;
    CamBlockRoute r;
    r.in_lds = chol_fits_lds(Nc);
    // Does the end-of-trial logic (step2_finish) ride in the reduction's launch (round 5)? On a single GPU the tail it
    // reads - g_S, |x|^2, the block elimination's status - is complete when the reduction's last workgroup has written it,
    // and that workgroup can decide the trial there and then, beside the others: the factorization's first launch starts
    // on its matrix at once (and may be several workgroups: the dissection's). Sharded, the tail is summed over the ranks
    // behind that launch. With the backward sweep the end-of-trial logic and the verdict are launches of their own
    r.finish_rides = !sharded && !mode.sweep;
    r.S_packed     = r.finish_rides && r.in_lds;
    r.compact      = mode.compact;
    r.nd_plans     = mode.compact && mode.dissect;
    // (where the host has provided for the dissection's launches - learn_likely_size() -, the reduction fills the
    //  dissection's matrices with more workgroups, and the factorization goes through those launches)
    r.nd_launches  = r.finish_rides && r.nd_plans && provided.rounds > 0;
    r.sweep        = mode.sweep;
    r.likely_panels = r.nd_launches ? nd_likely_panels : lchol_likely_panels;
    r.with_tail    = r.compact && !r.sweep && r.likely_panels > 0 && r.likely_panels < npanels;
    r.l_last       = r.with_tail ? r.likely_panels : npanels;
    *out = r;
    return true;
}

} // namespace mrcal_amd

// dev / tests (no declaration in include/: not part of the interface). mode: bit 0 compact, 1 dissect, 2 sweep.
// out[10]: the route's fields in their order. Returns 0 where camblock_route() refuses. Needs no GPU
extern "C" int mrcal_amd_debug_camblock_route(int Nc, int sharded, int mode, int nd_rounds, int nd_ns_max,
                                              int lchol_likely_panels, int nd_likely_panels, int* out)
{
    mrcal_amd::CamBlockRoute r;
    const mrcal_amd::CamBlockMode m = { (mode & 1) != 0, (mode & 2) != 0, (mode & 4) != 0 };
    if(!mrcal_amd::camblock_route(&r, Nc, sharded != 0, m, mrcal_amd::NdLimits{ nd_rounds, nd_ns_max },
                                  lchol_likely_panels, nd_likely_panels)) return 0;
    out[0] = r.in_lds;   out[1] = r.finish_rides; out[2] = r.S_packed; out[3] = r.compact; out[4] = r.nd_plans;
    out[5] = r.nd_launches; out[6] = r.sweep;     out[7] = r.with_tail; out[8] = r.likely_panels; out[9] = r.l_last;
    return 1;
}
