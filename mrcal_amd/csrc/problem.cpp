// The resident problem object and the compute half of the C ABI.
//
// mrcal_amd_problem_t owns every HBM buffer of one calibration problem (or of
// one frame-shard of it) and the HIP stream its kernels run on. The drop-in
// mrcal_optimizer_callback() is a thin shell over it: create, evaluate, copy
// out, destroy.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "layout.hpp"
#include "host_state.hpp"
#include "problem.hpp"
#include "kernels.hpp"
#include "lens_dispatch.hpp"
#include "problem_object.hpp"
#include "host_copy.hpp"
#include "solver_plan.hpp"
#include "problem_plan.hpp"
#include <utility>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <chrono>
#include <unistd.h>

using namespace mrcal_amd;

mrcal_amd_problem::~mrcal_amd_problem()
{
    // (the buffers before the streams, whatever the order of the members)
    mem.free_all();
    for(hipEvent_t e : ctl_events) hipEventDestroy(e);
    for(hipEvent_t e : ev_pool) hipEventDestroy(e);
    if(ev_j0)  hipEventDestroy(ev_j0);
    if(ev_j1)  hipEventDestroy(ev_j1);
    if(ev_fork) hipEventDestroy(ev_fork);
    if(ev_join) hipEventDestroy(ev_join);
    if(side_stream) hipStreamDestroy(side_stream);
    if(stream) hipStreamDestroy(stream);
}

namespace mrcal_amd {

// ---- problem_prepare_solver(): what the solver holds beyond the evaluation's buffers, one step after the other ----

// the second operating point, and both points' normal equations
static bool alloc_normal_equations(mrcal_amd_problem* P)
{
    const Layout& L = P->L;
    const NormalDims& nd = P->nd;
    const bool splined = L.lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC;
    bool ok = true;
    ok = ok && P->mem.alloc(&P->op[1].b,  (size_t)L.Nstate);
    ok = ok && P->mem.alloc(&P->op[1].x,  (size_t)L.Nmeas);
    ok = ok && P->mem.alloc(&P->op[1].Jv, (size_t)P->Nnz);
    if(P->op[0].spl_box != NULL) ok = ok && P->mem.alloc(&P->op[1].spl_box, (size_t)4*P->D.Nobs_board);
    if(!splined && (size_t)P->D.Nobs_board*gram_stride(L.Ndist) >= ((size_t)1 << 32))
    {
        // (reduce_pair_chunk() addresses the Grams with 32-bit element offsets; this is 34 GB of Grams)
        set_error("too many board observations: %d Grams of %d doubles", P->D.Nobs_board, gram_stride(L.Ndist));
        return false;
    }
    ok = ok && P->mem.alloc(&P->d_gram, splined ? (size_t)1 : (size_t)P->D.Nobs_board*gram_stride(L.Ndist));
    for(int i=0;i<2 && ok;i++)
    {
        ok = ok && P->mem.alloc(&P->op[i].A,       (size_t)nd.Nc*nd.Nc);
        // (rows of blocks nobody writes - frames without observations in this shard - must read as zero)
        ok = ok && P->mem.alloc_zeroed(&P->op[i].Bt, (size_t)nd.NE*nd.Nc);
        ok = ok && P->mem.alloc_zeroed(&P->op[i].D,  (size_t)nd.NEb*36);
        ok = ok && P->mem.alloc_zeroed(&P->op[i].g,  (size_t)nd.Nstate);
        ok = ok && P->mem.alloc(&P->op[i].scalars, (size_t)NSCALARS);
        ok = ok && P->mem.alloc_zeroed(&P->op[i].step_cauchy, (size_t)nd.Nstate);
        ok = ok && P->mem.alloc_zeroed(&P->op[i].step_gn,     (size_t)nd.Nstate);
    }
    return ok;
}

// the factorization's scratch (FactorBuffers), the step and the dog-leg control block
static bool alloc_factor_scratch(mrcal_amd_problem* P)
{
    const NormalDims& nd = P->nd;
    bool ok = true;
    ok = ok && P->mem.alloc(&P->F.Spart, schur_partial_doubles(nd));
    ok = ok && P->mem.alloc(&P->F.Linv,  cholesky_large_workspace_doubles(nd.Nc));
    if(cholesky_large_workspace_doubles(nd.Nc) > 1) ok = ok && P->mem.alloc(&P->F.diag_minmax, 2);
    // the tile occupancy of Wt: only where the couplings are sparse (the splined models) and the strip SYRK runs
    if(P->L.lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC && nd.Nc > 256 && nd.Nc <= 4096)
    {
        ok = ok && P->mem.alloc(&P->F.occ, (size_t)nd.NEb*occ_words(nd));
        ok = ok && P->mem.alloc(&P->F.Wtile, (size_t)((nd.Nc + 15)/16)*16*(size_t)nd.NE);
    }
    ok = ok && P->mem.alloc((char**)&P->d_ctl, solver_ctl_bytes());
    // (rows of blocks this shard does not own are never written: they must read as 0)
    ok = ok && P->mem.alloc_zeroed(&P->F.Wt, (size_t)nd.NE*nd.Nc);
    ok = ok && P->mem.alloc(&P->F.LD, (size_t)nd.NEb*36);
    ok = ok && P->mem.alloc_zeroed(&P->F.y,  (size_t)nd.NE);
    // S and r contiguous: one all-reduce moves both
    // [S | r | g_S | |x|^2 | status]: comm1 of the sharded step (step2_comm1_doubles())
    // (round 6: + a packed copy of the lower triangle behind them, for the one-workgroup Cholesky: factor_S_packed())
    ok = ok && P->mem.alloc(&P->F.S,  (size_t)nd.Nc*nd.Nc + 2*nd.Nc + 2 + 64 + ((((size_t)nd.Nc*(nd.Nc + 1)) >> 1) + nd.Nc + 2));
    P->F.r = ok ? P->F.S + (size_t)nd.Nc*nd.Nc : NULL;
    ok = ok && P->mem.alloc(&P->F.status, 1);
    ok = ok && P->mem.alloc(&P->d_step,   (size_t)nd.Nstate);
    ok = ok && P->mem.alloc(&P->d_comm,   (size_t)nd.Nstate + 64);
    ok = ok && P->mem.alloc(&P->d_counts, 4);
    ok = ok && P->mem.alloc(&P->d_outlier_part, outlier_partial_doubles());
    if(!ok) return false;
    // only the lower triangle of S is ever written; the rest rides along in the
    // all-reduce of [S | r] and should be numbers
    HIP_TRY(hipMemset(P->F.S, 0, ((size_t)nd.Nc*nd.Nc + 2*nd.Nc + 2)*sizeof(double)), return false);
    return P->mem.alloc_pinned(&P->h_scalars, 64);
}

// The splined models' camera block without the control points no board covers (round 5; assembly_splined.hip,
// spl_compact_kernel / LcholCompact): where the big camera block's launch-per-panel Cholesky runs, every row that
// touches a control point is a board's (no discrete points: they have no boxes) and all rows are here (not a shard:
// the ranks of a sharded solve sum their camera blocks entry by entry; nor with the backward sweep, which knows nothing
// of a size the device decides). MRCAL_AMD_NO_SPL_COMPACT=1: off. Only allocates: what is in use is the mode's to say
static bool alloc_splined_compaction(mrcal_amd_problem* P, bool sweep)
{
    const Layout& L = P->L;
    const NormalDims& nd = P->nd;
    static const bool env_off = (getenv("MRCAL_AMD_NO_SPL_COMPACT") != NULL);
    const bool off = env_off || sweep;
    const bool whole = (int)P->board_sel.size() == L.dims.Nobservations_board && P->comm == NULL;
    if(off || !whole || L.lensmodel.type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC || cholesky_large_workspace_doubles(nd.Nc) <= 1 || nd.Nc > 4096 ||
       P->D.Nobs_board <= 0 || P->D.Nobs_point != 0 || P->D.Ndist_state <= 0 || nd.elim_extrinsics)
        return true;
    // (until the first evaluation: the identity)
    std::vector<int> id((size_t)2*nd.Nc + 1);
    for(int c = 0; c < nd.Nc; c++) { id[c] = c; id[nd.Nc + c] = c; }
    id[2*nd.Nc] = nd.Nc;
    bool ok = P->mem.upload(&P->op[0].cperm, id) && P->mem.upload(&P->op[1].cperm, id);
    ok = ok && P->mem.alloc(&P->F.cperm_cur, (size_t)2*nd.Nc + 2);
    ok = ok && P->mem.alloc(&P->F.iso, (size_t)4*(nd.Nc/2 + 1) + nd.Nc + 2);
    // ... and in a nested-dissection order where the boards leave a strip worth having (cholesky_large.hip,
    // lchol_nd_*): one camera's grid. MRCAL_AMD_NO_ND=1: off
    static const bool nd_off = (getenv("MRCAL_AMD_NO_ND") != NULL);
    if(!nd_off && P->D.Ncameras_intrinsics == 1)
    {
        const size_t Npos = (size_t)nd.Nc + 2*ND_PANEL;
        const size_t W = LCH_ND_WMAX, wsz = (W/ND_PANEL)*ND_PANEL*ND_PANEL + W*W + W;
        std::vector<int> h0(nd_plan_ints(nd.Nc), 0);
        h0[NDH_NS] = nd.Nc; h0[NDH_NSEFF] = nd.Nc;
        ok = ok && P->mem.upload(&P->op[0].ndp, h0) && P->mem.upload(&P->op[1].ndp, h0) && P->mem.upload(&P->F.ndp_cur, h0);
        ok = ok && P->mem.alloc(&P->F.ndMA, (Npos + 1)*Npos) && P->mem.alloc(&P->F.ndMB, (Npos + 1)*Npos);
        ok = ok && P->mem.alloc(&P->F.ndLinvA, wsz) && P->mem.alloc(&P->F.ndLinvB, wsz);
        ok = ok && P->mem.alloc(&P->F.ndPart, (size_t)((nd.Nc + 15)/16)*2*LCH_ND_WMAX);
        ok = ok && P->mem.alloc_zeroed(&P->F.nd_lim_dev, 2);
        P->F.nd_lim = NdLimits{0, 0}; P->F.nd_likely_panels = 0;
    }
    return ok;
}

// the rows of a splined problem that no plan covers: their three levels of pre-rounded sums (ReproStep), zero at rest
static bool alloc_repro_levels(mrcal_amd_problem* P)
{
    if(!splined_needs_repro_rows(P->D)) return true;
    const NormalDims& nd = P->nd;
    ReproStep& rs = P->plan.repro;
    rs.one = (size_t)nd.Nc*nd.Nc + (size_t)nd.NE*nd.Nc + (size_t)nd.NEb*36 + (size_t)nd.Nstate + 1;
    bool ok = true;
    for(int l = 0; l < 3 && ok; l++) ok = ok && P->mem.alloc_zeroed(&rs.lvl[l], rs.one);
    return ok && P->mem.alloc_zeroed(&rs.cmax, (size_t)nd.Nstate + 1) && P->mem.alloc_zeroed(&rs.any, 1);
}

// the lists the board observations' Grams are summed by (plan_board_grams()), and the partial sums' own buffers
static bool upload_board_gram_plan(mrcal_amd_problem* P)
{
    const NormalDims& nd = P->nd;
    DeviceBuffers& mem = P->mem;
    AssemblyPlan& A = P->plan;
    const int Nobs = P->D.Nobs_board;
    std::vector<BoardObsMeta> meta(Nobs);
    if(Nobs > 0)
        HIP_TRY(hipMemcpy(meta.data(), P->d_board_meta, (size_t)Nobs*sizeof(BoardObsMeta), hipMemcpyDeviceToHost), return false);
    BoardGramPlan bp;
    if(!plan_board_grams(P->D, nd, meta.data(), nd.elim_extrinsics ? P->D.Ncameras_extrinsics : P->L.dims.Nframes, &bp)) return false;
    A.Nchunks = bp.Nchunks; A.Npairs = bp.Npairs; A.Ndest = (int)bp.dest.id.size();
    bool ok = mem.upload(&A.frame_obs_begin, bp.frame_obs_begin) &&
              (!nd.elim_extrinsics || mem.upload(&A.frame_obs, bp.frame_obs)) &&
              mem.upload(&A.chunk_begin, bp.chunk_begin) && mem.upload(&A.pair_obs,   bp.pair_obs)   &&
              mem.upload(&A.pos_table,   bp.pos_table)   && mem.upload(&A.pair_table, bp.pair_table) &&
              mem.upload(&A.frame_pos,   bp.frame_pos)   && mem.upload(&A.obs_cols,   bp.obs_cols)   &&
              mem.upload(&A.obs_pair,    bp.obs_pair)    && mem.upload(&A.chunk_pair, bp.chunk_pair) &&
              mem.upload(&A.dest_id,     bp.dest.id)     && mem.upload(&A.dest_begin, bp.dest.begin) &&
              mem.upload(&A.dest_src,    bp.dest.src)    && mem.upload(&A.pair_chunk_begin, bp.pair_chunk_begin);
    if(P->D.lens_type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
        return ok && mem.alloc(&A.chunk_part, (size_t)A.Nchunks*bp.pos_table.size());
    if(Nobs == 0) return ok && mem.alloc(&A.chunk_part, 1);
    // splined models: the staged Grams of assemble_splined_kernel (two passes per observation), the knot
    // boxes, and the parts of the rows of the camera block that are not knots (+ the x row)
    const int nknotrows = P->D.Nintr_state > 0 ? P->D.Ncameras_intrinsics*(P->D.Nintr_state - P->D.Ncore_state) : 0;
    return ok && mem.alloc(&A.chunk_part, (size_t)2*Nobs*SPL_TRI) && mem.alloc(&A.spl_hdr, (size_t)Nobs) &&
           mem.alloc(&A.spl_part, (size_t)(nd.Nc + 1 - nknotrows)*SPLG_E*(nd.Nc + 1));
}

// The fixed-order plan of the point and pair rows (plan_gen_rows()), from the CSR structure itself, which does not
// change between evaluations (except the splined models' patch columns: no plan then, those rows keep the atomics)
static bool upload_gen_rows_plan(mrcal_amd_problem* P)
{
    GenPlan& G = P->plan.gen;
    memset(&G, 0, sizeof(G));
    const Layout& L = P->L;
    DeviceBuffers& mem = P->mem;
    const int r0 = L.i_meas_points, r1 = L.i_meas_regularization;
    G.row_first = r0; G.row_end = r1;
    if(r1 <= r0) return true;
    if(L.lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC && L.Nmeas_points > 0 && L.Ndist_state > 0) return true;
    std::vector<int32_t> Jp((size_t)(r1 - r0) + 1);
    HIP_TRY(hipMemcpy(Jp.data(), P->d_Jp + r0, Jp.size()*sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    const int32_t p0 = Jp[0], p1 = Jp[r1 - r0];
    std::vector<int32_t> Ji((size_t)(p1 - p0));
    if(p1 > p0) HIP_TRY(hipMemcpy(Ji.data(), P->d_Ji + p0, Ji.size()*sizeof(int32_t), hipMemcpyDeviceToHost), return false);
    const GenRowsPlan gp = plan_gen_rows(P->nd, r0, r1, Jp.data(), Ji.data());
    if(gp.Nrows == 0) return true;
    if(!(mem.upload(&G.rows,        gp.rows)        && mem.upload(&G.chunk_begin, gp.chunk_begin) &&
         mem.upload(&G.chunk_group, gp.chunk_group) && mem.upload(&G.group_k,     gp.group_k)     &&
         mem.upload(&G.group_off,   gp.group_off)   && mem.upload(&G.spos,        gp.spos)        &&
         mem.upload(&G.scol,        gp.scol)        && mem.upload(&G.dest_id,     gp.dest.id)     &&
         mem.upload(&G.dest_begin,  gp.dest.begin)  && mem.upload(&G.dest_src,    gp.dest.src)    &&
         mem.upload(&G.group_chunk_begin, gp.group_chunk_begin) &&
         mem.upload(&G.eb_block,    gp.eb_block)    && mem.upload(&G.eb_begin,    gp.eb_begin)    &&
         mem.upload(&G.eb_rows,     gp.eb_rows)     && mem.upload(&G.eb_group,    gp.eb_group)    &&
         mem.upload(&G.eb_epos,     gp.eb_epos)     && mem.alloc(&G.part, (size_t)gp.Nchunks*gp.stride)))
        return false;
    G.Nrows = gp.Nrows; G.Nchunks = gp.Nchunks; G.Ngroups = gp.Ngroups; G.stride = gp.stride; G.kmax = gp.kmax;
    G.Ndest = (int)gp.dest.id.size(); G.Neblocks = (int)gp.eb_block.size();
    return true;
}

// the per-workgroup partial sums of the step's reductions
static bool alloc_step_partials(mrcal_amd_problem* P)
{
    const NormalDims& nd = P->nd;
    AssemblyPlan& A = P->plan;
    const int Nobs = P->D.Nobs_board;
    // (with the plan above, the row-by-row workgroups of the assembly take the regularization rows only)
    const int row0 = (A.gen.Nrows > 0) ? P->L.i_meas_regularization : 2*P->D.W*P->D.H*Nobs;
    A.row_part_n = (Nobs > 0 && P->L.Nmeas > row0) ? (P->L.Nmeas - row0 + 255)/256 : 0;
    A.qf_part_n  = (nd.Nc + nd.NE + 4*QF_ROWS_PER_WAVE - 1)/(4*QF_ROWS_PER_WAVE);
    return P->mem.alloc(&A.row_part, (size_t)A.row_part_n) && P->mem.alloc(&A.qf_part, (size_t)4*A.qf_part_n) &&
           P->mem.alloc(&A.dots_part, (size_t)2*nd.NEb);
}

// (the second, third and fourth sub-boxes of the splined models' close-ups, which mostly nobody touches: last)
static bool alloc_splined_closeups(mrcal_amd_problem* P)
{
    if(P->plan.spl_hdr == NULL) return true;
    const size_t Nobs = (size_t)P->D.Nobs_board;
    return P->mem.alloc(&P->plan.chunk_extra,   (size_t)2*Nobs*(SPL_MAXSUB - 1)*SPL_TRI) &&
           P->mem.alloc(&P->plan.spl_hdr_extra, Nobs*(SPL_MAXSUB - 1));
}

// The one place that says what of the camera block's compaction is in use, on the host (FactorBuffers::mode, which
// camblock_route() goes by) and for the evaluation's kernels (AssemblyPlan, passed by value)
void problem_set_camblock_mode(mrcal_amd_problem* P, const CamBlockMode& mode)
{
    P->F.mode = mode;
    P->plan.spl_compact = mode.compact ? 1 : 0;
    P->plan.nd_lim      = mode.dissect ? P->F.nd_lim_dev : NULL;
}

static bool allocate_solver_buffers(mrcal_amd_problem* P)
{
    // (the tests' hook: the backward sweep from the start)
    const bool sweep = test_hooks().lchol_sweep != 0;
    if(!(alloc_normal_equations(P) && alloc_factor_scratch(P) && alloc_splined_compaction(P, sweep))) return false;
    // what was allocated is in use, until a communicator, the fallback to the sweep or error 3 say otherwise (solver.cpp)
    problem_set_camblock_mode(P, CamBlockMode{ P->F.cperm_cur != NULL, P->F.ndMA != NULL, sweep });
    return alloc_repro_levels(P) &&
           problem_sync_ops(P) &&
           upload_board_gram_plan(P) && upload_gen_rows_plan(P) && alloc_step_partials(P) && alloc_splined_closeups(P);
}

// A preparation that failed stays failed: what it had allocated by then is the problem's until the problem goes, and
// the next call reports the same error instead of allocating everything a second time
bool problem_prepare_solver(mrcal_amd_problem* P)
{
    if(P->solver_ready) return true;
    if(P->prepare_error.empty())
    {
        P->solver_ready = allocate_solver_buffers(P);
        if(P->solver_ready) return true;
        P->prepare_error = last_error_string().empty() ? "the solver's buffers could not be allocated" : last_error_string();
        return false;
    }
    set_error("%s", P->prepare_error.c_str());
    return false;
}

bool problem_sync_ops(mrcal_amd_problem* P)
{
    if(P->d_ops == NULL && !P->mem.alloc(&P->d_ops, 2)) return false;
    OpDev h[2] = { P->op[0], P->op[1] };
    HIP_TRY(hipMemcpy(P->d_ops, h, sizeof(h), hipMemcpyHostToDevice), return false);
    return true;
}

bool problem_evaluate_ref(mrcal_amd_problem* P, const OpRef& R, bool with_jacobian, bool with_normal, int parts,
                          hipStream_t stream, const ChooseArgs* choose)
{
    if(with_normal && !P->solver_ready) { set_error("solver buffers are not allocated"); return false; }
    if(stream == NULL) stream = P->stream;
    EvalBuffers B = P->eval_buffers(R, with_normal);
    if(choose != NULL && !((parts & EVAL_PART_PROLOGUE) && prologue_takes_choose(P->D)))
    {
        set_error("internal error: this evaluation has no prologue launch to choose the trial point in");
        return false;
    }
    B.choose = choose;
    // (round 6) a solve that was told to leave the Jacobian stream out: only the solver's own evaluations, and only
    // where the board kernel is the rows' one reader (never the splined models, whose assembly reads them back)
    if(P->jfree_now && with_normal && with_jacobian && problem_has_grams(P->D))
    {
        B.store_jacobian = false;
        if(parts & EVAL_PART_BOARD) P->jacobian_stale = true;
    }
    if(with_normal && (parts & EVAL_PART_ZERO))
    {
        if((parts & EVAL_PART_PROLOGUE) && P->D.Nobs_board > 0)
        {
            // the prologue kernel clears the normal equations on the side
            const NormalDims& nd = P->nd;
            B.zero_n[0] = (long long)nd.Nc*nd.Nc; B.zero_n[1] = (long long)nd.NE*nd.Nc; B.zero_n[2] = (long long)nd.NEb*36;
            B.zero_n[3] = nd.Nstate;               B.zero_n[4] = NSCALARS;
            B.zero_total = B.zero_n[0] + B.zero_n[1] + B.zero_n[2] + B.zero_n[3] + B.zero_n[4];
        }
        else
            HIP_TRY(launch_zero_normal(P->nd, R, stream), return false);
    }
    // An event pair around the Jacobian kernel costs ~5.6 us on EACH side of it on the stream (measured: the
    // gaps prologue -> kernel -> assembly in a kernel trace; every other boundary of the step is back to
    // back). So: none inside the solver's steps unless the benchmark asked for timings, and then only around
    // every ev_pool_stride-th launch; a host-driven evaluate() keeps its pair (last_jacobian_kernel_ms())
    hipEvent_t e0 = NULL, e1 = NULL;
    if(with_jacobian && (parts & EVAL_PART_BOARD))
    {
        if(P->ev_pool_enabled)
        {
            if((P->ev_pool_seen++ % P->ev_pool_stride) == 0 && P->ev_pool_used + 2 <= (int)P->ev_pool.size())
            {
                e0 = P->ev_pool[P->ev_pool_used++];
                e1 = P->ev_pool[P->ev_pool_used++];
            }
        }
        else if(parts == EVAL_PART_ALL) { e0 = P->ev_j0; e1 = P->ev_j1; }
    }
    HIP_TRY(launch_evaluate(P->D, B, with_jacobian, P->lds_bytes, stream, e0, e1, parts),
            return false);
    if(parts & EVAL_PART_BOARD)
        P->have_jacobian_timing = with_jacobian && P->D.Nobs_board > 0 && e0 != NULL;
    if(with_normal && (parts & EVAL_PART_ASSEMBLE))
        HIP_TRY(launch_assemble(P->D, P->nd, P->br, P->plan, B, stream), return false);
    return true;
}

bool problem_ensure_jacobian(mrcal_amd_problem* P)
{
    if(!P->jacobian_stale) return true;
    if(!problem_evaluate_op(P, P->icur, true, false)) return false;
    HIP_TRY(hipStreamSynchronize(P->stream), return false);
    return true;
}

bool problem_evaluate_op(mrcal_amd_problem* P, int i, bool with_jacobian, bool with_normal)
{
    if(!problem_evaluate_ref(P, P->opref(i), with_jacobian, with_normal, EVAL_PART_ALL)) return false;
    // (a host-driven evaluation always streams J: jfree_now is up only inside the solver's entry points)
    if(with_jacobian && i == P->icur) P->jacobian_stale = false;
    P->stats.Nevaluations++;
    if(with_normal) P->op[i].have_normal = true;
    return true;
}

bool problem_state_arrays(mrcal_amd_problem* P, ProblemStateArrays* s)
{
    const Layout& L = P->L;
    std::vector<double> b((size_t)std::max(L.Nstate, 1));
    s->intrinsics.assign((size_t)L.dims.Ncameras_intrinsics*L.Nintrinsics, 0.0);
    s->rt_cam_ref.assign((size_t)std::max(L.dims.Ncameras_extrinsics, 1), mrcal_pose_t());
    s->rt_ref_frame.assign((size_t)std::max(L.dims.Nframes, 1), mrcal_pose_t());
    // (unpacked into and not handed out: nobody has asked for them yet)
    std::vector<mrcal_point3_t> points((size_t)std::max(L.dims.Npoints, 1));
    mrcal_calobject_warp_t warp;
    if(!mrcal_amd_problem_get_b_packed(P, b.data())) return false;
    HIP_TRY(hipMemcpy(s->intrinsics.data(), P->d_seed_intrinsics, s->intrinsics.size()*sizeof(double), hipMemcpyDeviceToHost), return false);
    if(L.dims.Ncameras_extrinsics > 0)
        HIP_TRY(hipMemcpy(s->rt_cam_ref.data(), P->d_seed_rt_cam_ref, (size_t)L.dims.Ncameras_extrinsics*sizeof(mrcal_pose_t), hipMemcpyDeviceToHost), return false);
    if(L.dims.Nframes > 0)
        HIP_TRY(hipMemcpy(s->rt_ref_frame.data(), P->d_seed_rt_ref_frame, (size_t)L.dims.Nframes*sizeof(mrcal_pose_t), hipMemcpyDeviceToHost), return false);
    unpack_state_to_arrays(b.data(), L, s->intrinsics.data(), s->rt_cam_ref.data(), s->rt_ref_frame.data(), points.data(), &warp);
    return true;
}

} // namespace mrcal_amd

namespace {
int& elimination_policy() { static int policy = 0; return policy; }
// Which pose blocks the next problem eliminates where it can choose (plan_problem()): 0 auto, 1 frames, 2 extrinsics.
// mrcal_amd_set_elimination() wins; without a call the environment variable MRCAL_AMD_ELIMINATE=frames|extrinsics
// says (for a process that cannot make one)
int effective_elimination()
{
    if(elimination_policy() != 0) return elimination_policy();
    const char* env = getenv("MRCAL_AMD_ELIMINATE");
    if(env && !strcmp(env, "frames"))     return 1;
    if(env && !strcmp(env, "extrinsics")) return 2;
    return 0;
}
}

// ---- problem_create(): the plan (problem_plan.cpp) says what; here it is allocated, uploaded and launched ----
namespace mrcal_amd {

static bool create_streams(mrcal_amd_problem* P)
{
    bool ok = true;
    HIP_TRY(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking), ok = false);
    HIP_TRY(hipStreamCreateWithFlags(&P->side_stream, hipStreamNonBlocking), ok = false);
    HIP_TRY(hipEventCreateWithFlags(&P->ev_fork, hipEventDisableTiming), ok = false);
    HIP_TRY(hipEventCreateWithFlags(&P->ev_join, hipEventDisableTiming), ok = false);
    HIP_TRY(hipEventCreate(&P->ev_j0), ok = false);
    HIP_TRY(hipEventCreate(&P->ev_j1), ok = false);
    return ok;
}

// the seeds, the observations' records and their pools: of a shard's pools the rows it owns, gathered here
static bool upload_inputs(mrcal_amd_problem* P, const ProblemInputs& in, const ProblemPlan& plan, bool sharded)
{
    const Layout& L = P->L;
    const int Nboard_local = P->D.Nobs_board, Npoint_local = P->D.Nobs_point, NPTS = P->D.W*P->D.H;
    std::vector<mrcal_point3_t> pool_local;
    const mrcal_point3_t* pool_src = in.observations_board_pool;
    if(sharded)
    {
        pool_local.resize((size_t)Nboard_local*NPTS);
        for(int j=0; j<Nboard_local; j++)
            memcpy(&pool_local[(size_t)j*NPTS], &in.observations_board_pool[(size_t)P->board_sel[j]*NPTS],
                   NPTS*sizeof(mrcal_point3_t));
        pool_src = pool_local.data();
    }
    std::vector<mrcal_point3_t> point_pool_local((size_t)(Npoint_local > 0 ? Npoint_local : 1));
    for(int j=0; j<Npoint_local; j++) point_pool_local[j] = in.observations_point_pool[plan.point_sel[j]];
    // the triangulated observations' vectors and outlier marks: host copies too, for the outlier logic
    const int Nt = plan.tri_o1 - plan.tri_o0;
    P->tri_px_host.resize((size_t)3*Nt + 1);
    P->tri_outlier_host.resize((size_t)Nt + 1);
    for(int i=0;i<Nt;i++)
    {
        const mrcal_observation_point_triangulated_t& o = in.observations_point_triangulated[plan.tri_o0 + i];
        for(int j=0;j<3;j++) P->tri_px_host[3*i+j] = o.px.xyz[j];
        P->tri_outlier_host[i] = o.outlier ? 1 : 0;
    }

    DeviceBuffers& mem = P->mem;
    return mem.upload(&P->d_seed_intrinsics,   in.intrinsics,                  (size_t)in.Ncameras_intrinsics*L.Nintrinsics) &&
           mem.upload(&P->d_seed_rt_cam_ref,   (const double*)in.rt_cam_ref,   (size_t)in.Ncameras_extrinsics*6) &&
           mem.upload(&P->d_seed_rt_ref_frame, (const double*)in.rt_ref_frame, (size_t)in.Nframes*6) &&
           mem.upload(&P->d_seed_points,       (const double*)in.points,       (size_t)in.Npoints*3) &&
           mem.upload(&P->d_board_meta,        plan.bmeta.data(),              (size_t)Nboard_local) &&
           mem.upload(&P->d_board_pool,        (const double*)pool_src,        (size_t)Nboard_local*NPTS*3) &&
           mem.upload(&P->d_point_meta,        plan.pmeta.data(),              (size_t)Npoint_local) &&
           mem.upload(&P->d_point_pool,        (const double*)point_pool_local.data(), (size_t)Npoint_local*3) &&
           mem.upload(&P->d_imagersizes,       in.imagersizes,                 (size_t)in.Ncameras_intrinsics*2) &&
           mem.upload(&P->d_tri_meta,          P->tri_meta_host.data(),        P->tri_meta_host.size()) &&
           mem.upload(&P->d_tri_px,            P->tri_px_host.data(),          (size_t)3*Nt) &&
           mem.upload(&P->d_tri_outlier,       P->tri_outlier_host.data(),     (size_t)Nt);
}

// what an evaluation writes: the first operating point, the joint pose records, the CSR structure
static bool alloc_evaluation_buffers(mrcal_amd_problem* P)
{
    const Layout& L = P->L;
    const int Nboard_local = P->D.Nobs_board;
    DeviceBuffers& mem = P->mem;
    bool ok = mem.alloc(&P->op[0].b,  (size_t)L.Nstate) &&
              // + the unpacked intrinsics and warp (DeviceProblem::unpacked)
              mem.alloc(&P->d_joint,  (size_t)Nboard_local*JOINT_STRIDE + (size_t)P->D.Ncameras_intrinsics*L.Nintrinsics + 2) &&
              mem.alloc(&P->op[0].x,  (size_t)L.Nmeas) &&
              mem.alloc(&P->op[0].Jv, (size_t)P->Nnz);
    if(L.lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC && Nboard_local > 0)
        ok = ok && mem.alloc(&P->op[0].spl_box, (size_t)4*Nboard_local);
    return ok && mem.alloc(&P->d_Jp, (size_t)L.Nmeas+1) && mem.alloc(&P->d_Ji, (size_t)P->Nnz) && problem_sync_ops(P);
}

static void set_device_pointers(mrcal_amd_problem* P)
{
    DeviceProblem& D = P->D;
    D.seed_intrinsics   = P->d_seed_intrinsics;
    D.seed_rt_cam_ref   = P->d_seed_rt_cam_ref;
    D.seed_rt_ref_frame = P->d_seed_rt_ref_frame;
    D.seed_points       = P->d_seed_points;
    D.board_meta        = P->d_board_meta;
    D.board_pool        = P->d_board_pool;
    D.point_meta        = P->d_point_meta;
    D.point_pool        = P->d_point_pool;
    D.imagersizes       = P->d_imagersizes;
    D.tri_meta          = P->d_tri_meta;
    D.tri_px            = P->d_tri_px;
    D.tri_outlier       = P->d_tri_outlier;
    D.unpacked          = P->d_joint + (size_t)D.Nobs_board*JOINT_STRIDE;
}

// the seed state, packed, and the iteration-invariant CSR structure
static bool upload_seed_and_structure(mrcal_amd_problem* P, const ProblemInputs& in)
{
    const Layout& L = P->L;
    P->b_host.assign(L.Nstate > 0 ? L.Nstate : 1, 0.0);
    pack_state_from_arrays(P->b_host.data(), L, in.intrinsics, in.rt_cam_ref, in.rt_ref_frame, in.points, in.calobject_warp);
    HIP_TRY(hipMemcpyAsync(P->op[0].b, P->b_host.data(), (size_t)L.Nstate*sizeof(double),
                           hipMemcpyHostToDevice, P->stream), return false);
    HIP_TRY(launch_structure(P->D, P->eval_buffers(0,false), P->stream), return false);
    if(L.Nmeas_regularization <= 0)
    {
        const int32_t last = (int32_t)P->Nnz;
        HIP_TRY(hipMemcpyAsync(&P->d_Jp[L.Nmeas], &last, sizeof(last), hipMemcpyHostToDevice, P->stream), return false);
    }
    HIP_TRY(hipStreamSynchronize(P->stream), return false);
    return true;
}

mrcal_amd_problem* problem_create(const ProblemInputs& in, const ShardRanges& shard)
{
    last_error_string().clear();
    if(mrcal_amd_device_count() <= 0)
    {
        set_error("no HIP device is visible: libmrcal_amd has no CPU fallback");
        return NULL;
    }
    if(!lens_supported(in.lensmodel->type))
    {
        char name[128] = "?";
        mrcal_lensmodel_name(name, sizeof(name), in.lensmodel);
        set_error("lens model %s (%d) is not implemented on the GPU yet", name, (int)in.lensmodel->type);
        return NULL;
    }
    ProblemPlan plan;
    std::string refusal;
    if(!plan_problem(&plan, &refusal, in, shard, effective_elimination()))
    {
        set_error("%s", refusal.c_str());
        return NULL;
    }

    mrcal_amd_problem* P = new mrcal_amd_problem();
    P->L = plan.L;  P->D = plan.D;  P->nd = plan.nd;  P->br = plan.br;  P->is_leader = plan.is_leader;
    P->Nnz = plan.Nnz;  P->board_alg_bytes = plan.board_alg_bytes;  P->lds_bytes = plan.lds_bytes;
    P->board_sel     = std::move(plan.board_sel);
    P->tri_meta_host = std::move(plan.tmeta);
    P->tri_obs0      = plan.tri_o0;

    bool ok = create_streams(P) && upload_inputs(P, in, plan, /* sharded = */ shard.end_frame >= 0) &&
              alloc_evaluation_buffers(P);
    if(ok)
    {
        set_device_pointers(P);
        ok = upload_seed_and_structure(P, in);
    }
    if(!ok) { delete P; return NULL; }
    return P;
}

} // namespace mrcal_amd

// (round 6) The drop-in entry points make a problem, use it once and tear it down: a hipFree call per buffer, each of
// which waits for the device - 4 ms at the metric's size, a tenth of an mrcal_optimize() call. A problem that nobody can
// reach any more is torn down by a thread of its own instead, while the caller already has its results; at most two
// are in line at a time (a caller in a loop does not pile up gigabytes: the third it tears down itself, as before)
namespace mrcal_amd {
class ProblemReaper
{
    std::mutex m; std::condition_variable cv, cv_idle;
    std::deque<mrcal_amd_problem*> q;
    bool busy = false;
    pid_t owner = 0;        // the process the thread was started in (a fork()ed child has the object and no thread)
    int  device = 0;
    void run()
    {
        (void)hipSetDevice(device);
        for(;;)
        {
            mrcal_amd_problem* P = NULL;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return !q.empty(); });
                P = q.front(); q.pop_front(); busy = true;
            }
            delete P;
            { std::lock_guard<std::mutex> lk(m); busy = false; }
            cv_idle.notify_all();
        }
    }
public:
    // (never destroyed: its thread waits on it for as long as the process lives. What IS done when the process ends:
    //  what is in line is torn down before the runtime's own destructors run - Drain)
    static ProblemReaper& get()
    {
        static ProblemReaper* r = new ProblemReaper;
        static struct Drain { ProblemReaper* r; ~Drain() { r->drain(); } } d{r};
        return *r;
    }
    void later(mrcal_amd_problem* P)
    {
        if(P == NULL) return;
        {
            std::unique_lock<std::mutex> lk(m);
            if(owner != getpid())
            {
                q.clear(); busy = false; owner = getpid();
                (void)hipGetDevice(&device);
                std::thread([this] { run(); }).detach();
            }
            // (never a wait for the thread here: with two in line already the caller tears this one down itself)
            if(q.size() + (busy ? 1 : 0) < 2) { q.push_back(P); P = NULL; }
        }
        if(P == NULL) cv.notify_one();
        else          delete P;
    }
    void drain()
    {
        std::unique_lock<std::mutex> lk(m);
        if(owner == getpid()) cv_idle.wait_for(lk, std::chrono::seconds(5), [&] { return q.empty() && !busy; });
    }
};
void problem_destroy_later(mrcal_amd_problem* P) { ProblemReaper::get().later(P); }

bool dropin_inputs_ok(mrcal_problem_selections_t problem_selections,
                      const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                      int Nobservations_point_triangulated,
                      int Nobservations_board, const mrcal_calobject_warp_t* calobject_warp,
                      bool warp_seed_first)
{
    const bool bad_triangulated =
        observations_point_triangulated != NULL && Nobservations_point_triangulated &&
        !(!problem_selections.do_optimize_intrinsics_core &&
          !problem_selections.do_optimize_intrinsics_distortions &&
          problem_selections.do_optimize_extrinsics);
    const bool bad_warp_seed =
        Nobservations_board > 0 && problem_selections.do_optimize_calobject_warp && calobject_warp == NULL;
    if(bad_warp_seed && (warp_seed_first || !bad_triangulated))
    {
        set_error("ERROR: We're optimizing the calibration object warp, so a buffer with a seed MUST be passed in.");
        return false;
    }
    if(bad_triangulated)
    {
        set_error("ERROR: We have triangulated points. At this time this is only allowed if we're NOT optimizing intrinsics AND if we ARE optimizing extrinsics.");
        return false;
    }
    return true;
}
} // namespace mrcal_amd

extern "C" {

// 0: the library chooses (default); 1: the frames and points are eliminated; 2: the extrinsics, where the problem
// allows it. For the problems created AFTER the call. Returns the previous setting
int mrcal_amd_set_elimination(int policy)
{
    const int old = elimination_policy();
    if(policy >= 0 && policy <= 2) elimination_policy() = policy;
    return old;
}

const char* mrcal_amd_last_error(void)
{
    return last_error_string().c_str();
}

long mrcal_amd_device_buffers_live(void)
{
    return DeviceBuffers::live();
}

int mrcal_amd_device_count(void)
{
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

mrcal_amd_problem_t*
mrcal_amd_problem_create_sharded(const double*                 intrinsics,
                         const mrcal_pose_t*           rt_cam_ref,
                         const mrcal_pose_t*           rt_ref_frame,
                         const mrcal_point3_t*         points,
                         const mrcal_calobject_warp_t* calobject_warp,
                         int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                         int Npoints, int Npoints_fixed,
                         const mrcal_observation_board_t* observations_board,
                         const mrcal_observation_point_t* observations_point,
                         int Nobservations_board,
                         int Nobservations_point,
                         const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                         int Nobservations_point_triangulated,
                         const mrcal_point3_t* observations_board_pool,
                         const mrcal_point3_t* observations_point_pool,
                         const mrcal_lensmodel_t* lensmodel,
                         const int* imagersizes,
                         mrcal_problem_selections_t problem_selections,
                         double calibration_object_spacing,
                         int calibration_object_width_n,
                         int calibration_object_height_n,
                         int shard_begin_frame, int shard_end_frame,
                         int shard_begin_point, int shard_end_point,
                         int shard_begin_tripoint, int shard_end_tripoint,
                         bool is_shard_leader)
{
    const ProblemInputs in = { intrinsics, rt_cam_ref, rt_ref_frame, points, calobject_warp,
                               Ncameras_intrinsics, Ncameras_extrinsics, Nframes, Npoints, Npoints_fixed,
                               observations_board, observations_point, Nobservations_board, Nobservations_point,
                               observations_point_triangulated, Nobservations_point_triangulated,
                               observations_board_pool, observations_point_pool, lensmodel, imagersizes,
                               problem_selections, calibration_object_spacing,
                               calibration_object_width_n, calibration_object_height_n };
    return problem_create(in, ShardRanges{ shard_begin_frame, shard_end_frame, shard_begin_point, shard_end_point,
                                           shard_begin_tripoint, shard_end_tripoint, is_shard_leader });
}

mrcal_amd_problem_t*
mrcal_amd_problem_create(const double*                 intrinsics,
                         const mrcal_pose_t*           rt_cam_ref,
                         const mrcal_pose_t*           rt_ref_frame,
                         const mrcal_point3_t*         points,
                         const mrcal_calobject_warp_t* calobject_warp,
                         int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                         int Npoints, int Npoints_fixed,
                         const mrcal_observation_board_t* observations_board,
                         const mrcal_observation_point_t* observations_point,
                         int Nobservations_board,
                         int Nobservations_point,
                         const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                         int Nobservations_point_triangulated,
                         const mrcal_point3_t* observations_board_pool,
                         const mrcal_point3_t* observations_point_pool,
                         const mrcal_lensmodel_t* lensmodel,
                         const int* imagersizes,
                         mrcal_problem_selections_t problem_selections,
                         double calibration_object_spacing,
                         int calibration_object_width_n,
                         int calibration_object_height_n,
                         int shard_begin_frame, int shard_end_frame,
                         bool is_shard_leader)
{
    const ProblemInputs in = { intrinsics, rt_cam_ref, rt_ref_frame, points, calobject_warp,
                               Ncameras_intrinsics, Ncameras_extrinsics, Nframes, Npoints, Npoints_fixed,
                               observations_board, observations_point, Nobservations_board, Nobservations_point,
                               observations_point_triangulated, Nobservations_point_triangulated,
                               observations_board_pool, observations_point_pool, lensmodel, imagersizes,
                               problem_selections, calibration_object_spacing,
                               calibration_object_width_n, calibration_object_height_n };
    // the shard leader owns every discrete and triangulated point
    return problem_create(in, ShardRanges{ shard_begin_frame, shard_end_frame, 0, -1, 0, -1, is_shard_leader });
}

void mrcal_amd_problem_destroy(mrcal_amd_problem_t* problem)
{
    delete problem;
}

int     mrcal_amd_problem_Nstate       (const mrcal_amd_problem_t* p) { return p->L.Nstate; }
int     mrcal_amd_problem_Nmeasurements(const mrcal_amd_problem_t* p) { return p->L.Nmeas;  }
int64_t mrcal_amd_problem_Nnz          (const mrcal_amd_problem_t* p) { return p->Nnz;      }
int64_t mrcal_amd_problem_jacobian_algorithmic_bytes(const mrcal_amd_problem_t* p) { return p->board_alg_bytes; }
bool    mrcal_amd_problem_synchronize  (mrcal_amd_problem_t* p)
{
    HIP_TRY(hipStreamSynchronize(p->stream), return false);
    return true;
}

double*  mrcal_amd_problem_dev_b_packed(mrcal_amd_problem_t* p) { return p->op[p->icur].b;  }
double*  mrcal_amd_problem_dev_x       (mrcal_amd_problem_t* p) { return p->op[p->icur].x;  }
int32_t* mrcal_amd_problem_dev_J_rowptr(mrcal_amd_problem_t* p) { return p->d_Jp; }
int32_t* mrcal_amd_problem_dev_J_colidx(mrcal_amd_problem_t* p) { return p->d_Ji; }
double*  mrcal_amd_problem_dev_J_values(mrcal_amd_problem_t* p) { return problem_ensure_jacobian(p) ? p->op[p->icur].Jv : NULL; }
// (round 6) stream != 0 (the default): every evaluation of the solver writes the CSR values of J to HBM, as the
// metric defines a step and as a caller who reads J between steps needs it. 0: mrcal_amd_problem_solve()
// / _run_steps() leave the stream out where nothing in the solve reads it (boards under a parametric lens model): the
// same x, b_packed, outliers - the same bits -, J made on demand (_get_J(), _dev_J_values(), _evaluate()) afterwards.
// Returns the previous setting
int mrcal_amd_problem_set_jacobian_stream(mrcal_amd_problem_t* p, int stream)
{
    const int old = p->solve_stores_jacobian ? 1 : 0;
    p->solve_stores_jacobian = (stream != 0);
    return old;
}
// does a solve of this problem go without the Jacobian stream when told to?
int mrcal_amd_problem_jacobian_stream_is_optional(mrcal_amd_problem_t* p)
{
    return problem_has_grams(p->D) ? 1 : 0;
}
void*    mrcal_amd_problem_stream      (mrcal_amd_problem_t* p) { return (void*)p->stream; }

bool mrcal_amd_problem_set_b_packed(mrcal_amd_problem_t* p, const double* b)
{
    HIP_TRY(hipMemcpyAsync(p->op[p->icur].b, b, (size_t)p->L.Nstate*sizeof(double), hipMemcpyHostToDevice, p->stream), return false);
    HIP_TRY(hipStreamSynchronize(p->stream), return false);
    return true;
}
bool mrcal_amd_problem_get_b_packed(mrcal_amd_problem_t* p, double* b)
{
    HIP_TRY(hipMemcpyAsync(b, p->op[p->icur].b, (size_t)p->L.Nstate*sizeof(double), hipMemcpyDeviceToHost, p->stream), return false);
    HIP_TRY(hipStreamSynchronize(p->stream), return false);
    return true;
}
bool mrcal_amd_problem_get_x(mrcal_amd_problem_t* p, double* x)
{
    if(!device_to_host(x, p->op[p->icur].x, (size_t)p->L.Nmeas*sizeof(double), p->stream))
    {
        set_error("copying x to the host failed: %s", hipGetErrorString(hipGetLastError()));
        return false;
    }
    return true;
}
bool mrcal_amd_problem_get_J(mrcal_amd_problem_t* p, int32_t* rowptr, int32_t* colidx, double* values)
{
    if(values && !problem_ensure_jacobian(p)) return false;
    // (round 6: the big ones through a pinned ring and a pool of copying threads - host_copy.hpp: the caller's arrays are
    //  fresh pages, and one thread copying out of the runtime's staging buffer was 10 GB/s)
    bool ok = true;
    if(rowptr) ok = ok && device_to_host(rowptr, p->d_Jp, ((size_t)p->L.Nmeas+1)*sizeof(int32_t), p->stream);
    if(colidx) ok = ok && device_to_host(colidx, p->d_Ji, (size_t)p->Nnz*sizeof(int32_t), p->stream);
    if(values) ok = ok && device_to_host(values, p->op[p->icur].Jv, (size_t)p->Nnz*sizeof(double), p->stream);
    if(!ok) { set_error("copying the Jacobian to the host failed: %s", hipGetErrorString(hipGetLastError())); return false; }
    return true;
}

bool mrcal_amd_problem_evaluate(mrcal_amd_problem_t* p, bool with_jacobian, bool sync)
{
    if(!problem_evaluate_op(p, p->icur, with_jacobian, false)) return false;
    if(sync) HIP_TRY(hipStreamSynchronize(p->stream), return false);
    return true;
}

// Starts (capacity>0) or stops (capacity<=0) recording one HIP event pair
// around every Jacobian-kernel launch on the problem's stream
bool mrcal_amd_problem_jacobian_timing_begin(mrcal_amd_problem_t* p, int capacity)
{
    return mrcal_amd_problem_jacobian_timing_begin_strided(p, capacity, 1);
}
bool mrcal_amd_problem_jacobian_timing_begin_strided(mrcal_amd_problem_t* p, int capacity, int stride)
{
    p->ev_pool_used = 0;
    p->ev_pool_seen = 0;
    p->ev_pool_stride = stride > 0 ? stride : 1;
    p->ev_pool_enabled = capacity > 0;
    while((int)p->ev_pool.size() < 2*capacity)
    {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e), return false);
        p->ev_pool.push_back(e);
    }
    return true;
}
// Collects what was recorded since _begin(): number of launches and their
// total / min / max duration in ms. Stops the recording
bool mrcal_amd_problem_jacobian_timing_end(mrcal_amd_problem_t* p, int* Nlaunches,
                                           double* total_ms, double* min_ms, double* max_ms)
{
    HIP_TRY(hipStreamSynchronize(p->stream), return false);
    int n = 0; double tot = 0, mn = 1e300, mx = 0;
    for(int i=0; i+1<p->ev_pool_used; i+=2)
    {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev_pool[i], p->ev_pool[i+1]), return false);
        n++; tot += ms; if(ms < mn) mn = ms; if(ms > mx) mx = ms;
    }
    p->ev_pool_enabled = false;
    p->ev_pool_used = 0;
    if(Nlaunches) *Nlaunches = n;
    if(total_ms)  *total_ms  = tot;
    if(min_ms)    *min_ms    = n ? mn : 0;
    if(max_ms)    *max_ms    = mx;
    return true;
}

// dev tool: average duration (ms) of nrep back-to-back launches of the
// evaluation kernels alone, with the given debug_ablate bits
double mrcal_amd_problem_debug_time_evaluate(mrcal_amd_problem_t* p, bool with_gram, int ablate, int nrep)
{
    if(with_gram && !problem_prepare_solver(p)) return -1.0;
#ifdef MRCAL_AMD_DEV
    const int saved = p->D.debug_ablate;
    p->D.debug_ablate = ablate;
#else
    if(ablate != 0) { set_error("the ablation knob exists in measurement builds only (build.sh -DMRCAL_AMD_DEV)"); return -1.0; }
#endif
    const EvalBuffers B = p->eval_buffers(p->icur, with_gram);
    double total = 0.0;
    for(int i=0; i<nrep+1; i++)
    {
        if(launch_evaluate(p->D, B, true, p->lds_bytes, p->stream, p->ev_j0, p->ev_j1) != hipSuccess) return -1.0;
        if(hipStreamSynchronize(p->stream) != hipSuccess) return -1.0;
        float ms = 0;
        hipEventElapsedTime(&ms, p->ev_j0, p->ev_j1);
        if(i > 0) total += ms;
    }
#ifdef MRCAL_AMD_DEV
    p->D.debug_ablate = saved;
#endif
    return total/nrep;
}

#if defined(MRCAL_AMD_DEV) && defined(BOARD_TS)
// measurement builds (-DMRCAL_AMD_DEV -DBOARD_TS): per-observation phase timestamps of ONE board
// kernel launch, out[Nobs_board][8]. Returns the number of observations
int mrcal_amd_problem_debug_timestamps(mrcal_amd_problem_t* p, bool with_gram, long long* out)
{
    if(with_gram && !problem_prepare_solver(p)) return -1;
    const size_t n = (size_t)p->D.Nobs_board*10;
    DeviceBuffers mem;
    long long* d = NULL;
    if(!mem.alloc_zeroed(&d, n)) return -1;
    const EvalBuffers B = p->eval_buffers(p->icur, with_gram);
    for(int i=0;i<3;i++)
    {
        p->D.debug_ts = (i == 2) ? d : NULL;
        if(launch_evaluate(p->D, B, true, p->lds_bytes, p->stream, p->ev_j0, p->ev_j1) != hipSuccess) return -1;
        hipStreamSynchronize(p->stream);
    }
    p->D.debug_ts = NULL;
    hipMemcpy(out, d, n*sizeof(long long), hipMemcpyDeviceToHost);
    return p->D.Nobs_board;
}
#endif

double mrcal_amd_problem_last_jacobian_kernel_ms(mrcal_amd_problem_t* p)
{
    if(!p->have_jacobian_timing) return -1.0;
    if(hipEventSynchronize(p->ev_j1) != hipSuccess) return -1.0;
    float ms = -1.0f;
    if(hipEventElapsedTime(&ms, p->ev_j0, p->ev_j1) != hipSuccess) return -1.0;
    return (double)ms;
}

////////////////////////////////////////////////////////////////////////////////
// drop-in: one evaluation
////////////////////////////////////////////////////////////////////////////////
bool mrcal_optimizer_callback(double* b_packed, int buffer_size_b_packed,
                              double* x,        int buffer_size_x,
                              struct cholmod_sparse_struct* Jt,
                              const double*                 intrinsics,
                              const mrcal_pose_t*           rt_cam_ref,
                              const mrcal_pose_t*           rt_ref_frame,
                              const mrcal_point3_t*         points,
                              const mrcal_calobject_warp_t* calobject_warp,
                              int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                              int Npoints, int Npoints_fixed,
                              const mrcal_observation_board_t* observations_board,
                              const mrcal_observation_point_t* observations_point,
                              int Nobservations_board,
                              int Nobservations_point,
                              const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                              int Nobservations_point_triangulated,
                              const mrcal_point3_t* observations_board_pool,
                              const mrcal_point3_t* observations_point_pool,
                              const mrcal_lensmodel_t* lensmodel,
                              const int* imagersizes,
                              mrcal_problem_selections_t       problem_selections,
                              const mrcal_problem_constants_t* problem_constants,
                              double calibration_object_spacing,
                              int calibration_object_width_n,
                              int calibration_object_height_n,
                              bool verbose)
{
    (void)problem_constants; (void)verbose;
    last_error_string().clear();

    if(!dropin_inputs_ok(problem_selections, observations_point_triangulated, Nobservations_point_triangulated,
                         Nobservations_board, calobject_warp, /* warp_seed_first = */ false))
        return false;
    const mrcal_problem_selections_t sel =
        effective_selections(problem_selections, *lensmodel, Nobservations_board);
    if(!sel.do_optimize_intrinsics_core && !sel.do_optimize_intrinsics_distortions &&
       !sel.do_optimize_extrinsics      && !sel.do_optimize_frames &&
       !sel.do_optimize_calobject_warp)
    {
        set_error("Not optimizing any of our variables!");
        return false;
    }

    const int Nstate =
        mrcal_num_states(Ncameras_intrinsics, Ncameras_extrinsics, Nframes,
                         Npoints, Npoints_fixed, Nobservations_board, sel, lensmodel);
    if(buffer_size_b_packed != Nstate*(int)sizeof(double))
    {
        set_error("The buffer passed to fill-in b_packed has the wrong size. Needed exactly %d bytes, but got %d bytes",
                  Nstate*(int)sizeof(double), buffer_size_b_packed);
        return false;
    }
    const int Nmeas =
        mrcal_num_measurements(Nobservations_board, Nobservations_point,
                               observations_point_triangulated, Nobservations_point_triangulated,
                               calibration_object_width_n, calibration_object_height_n,
                               Ncameras_intrinsics, Ncameras_extrinsics, Nframes,
                               Npoints, Npoints_fixed, sel, lensmodel);
    if(buffer_size_x != Nmeas*(int)sizeof(double))
    {
        set_error("The buffer passed to fill-in x has the wrong size. Needed exactly %d bytes, but got %d bytes",
                  Nmeas*(int)sizeof(double), buffer_size_x);
        return false;
    }

    const ProblemInputs in = { intrinsics, rt_cam_ref, rt_ref_frame, points, calobject_warp,
                               Ncameras_intrinsics, Ncameras_extrinsics, Nframes, Npoints, Npoints_fixed,
                               observations_board, observations_point, Nobservations_board, Nobservations_point,
                               observations_point_triangulated, Nobservations_point_triangulated,
                               observations_board_pool, observations_point_pool, lensmodel, imagersizes,
                               sel, calibration_object_spacing,
                               calibration_object_width_n, calibration_object_height_n };
    mrcal_amd_problem_t* P = problem_create(in, ShardRanges{ 0, -1, 0, -1, 0, -1, true });
    if(P == NULL) return false;

    bool ok = false;
    if(P->L.Nstate != Nstate || P->L.Nmeas != Nmeas)
    {
        set_error("internal error: layout mismatch (%d,%d) vs (%d,%d)", P->L.Nstate, P->L.Nmeas, Nstate, Nmeas);
        goto done;
    }
    memcpy(b_packed, P->b_host.data(), (size_t)Nstate*sizeof(double));
    if(!mrcal_amd_problem_evaluate(P, Jt != NULL, true)) goto done;
    if(!mrcal_amd_problem_get_x(P, x)) goto done;
    if(Jt != NULL)
        if(!mrcal_amd_problem_get_J(P, (int32_t*)Jt->p, (int32_t*)Jt->i, (double*)Jt->x)) goto done;
    ok = true;
 done:
    // (hipStreamSynchronize()d by the copies above: nothing of P is in flight)
    problem_destroy_later(P);
    return ok;
}

////////////////////////////////////////////////////////////////////////////////
// drop-in: stand-alone projection (mrcal.h:165-174)
////////////////////////////////////////////////////////////////////////////////
bool mrcal_project(mrcal_point2_t* q, mrcal_point3_t* dq_dp, double* dq_dintrinsics,
                   const mrcal_point3_t* p, int N,
                   const mrcal_lensmodel_t* lensmodel, const double* intrinsics)
{
    last_error_string().clear();
    if(mrcal_amd_device_count() <= 0)
    {
        set_error("no HIP device is visible: libmrcal_amd has no CPU fallback");
        return false;
    }
    if(!lens_supported(lensmodel->type))
    {
        set_error("mrcal_project(): lens model %d is not supported", (int)lensmodel->type);
        return false;
    }
    if(N <= 0) return true;
    const int Ni = lensmodel_num_params(*lensmodel);
    const LensConfig cfg = lens_config_of(*lensmodel);

    DeviceBuffers mem;
    double *d_p = NULL, *d_i = NULL, *d_q = NULL, *d_g = NULL, *d_gi = NULL;
    bool ok = true;
    ok = ok && mem.upload(&d_p, (const double*)p, (size_t)3*N);
    ok = ok && mem.upload(&d_i, intrinsics, (size_t)Ni);
    ok = ok && mem.alloc(&d_q, (size_t)2*N);
    if(dq_dp)          ok = ok && mem.alloc(&d_g,  (size_t)6*N);
    if(dq_dintrinsics) ok = ok && mem.alloc_zeroed(&d_gi, (size_t)2*N*Ni);
    if(ok) HIP_TRY(launch_project_points((int)lensmodel->type, cfg, N, Ni, d_p, d_i, d_q, d_g, d_gi, NULL), ok = false);
    if(ok) HIP_TRY(hipMemcpy(q, d_q, (size_t)2*N*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    if(ok && dq_dp)          HIP_TRY(hipMemcpy(dq_dp, d_g, (size_t)6*N*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    if(ok && dq_dintrinsics) HIP_TRY(hipMemcpy(dq_dintrinsics, d_gi, (size_t)2*N*Ni*sizeof(double), hipMemcpyDeviceToHost), ok = false);
    return ok;
}

} // extern "C"
