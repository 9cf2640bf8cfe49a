// The plan of a problem (problem_plan.hpp): one small step after the other, in the order plan_problem() calls them.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "problem_plan.hpp"
#include "kernels.hpp"
#include "lens_dispatch.hpp"

namespace mrcal_amd {

static bool refuse(std::string* error, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    *error = buf;
    return false;
}

// no triangulated observations is (NULL, 0), no board observations is a 0x0 board; the selections as the reference
// adjusts them (effective_selections())
static bool normalise_inputs(ProblemInputs* in, std::string* error)
{
    if(in->observations_point_triangulated == NULL || in->Nobservations_point_triangulated <= 0)
    {
        in->observations_point_triangulated = NULL;
        in->Nobservations_point_triangulated = 0;
    }
    if(in->Nobservations_board > 0 &&
       (in->calibration_object_width_n <= 0 || in->calibration_object_height_n <= 0))
        return refuse(error, "board observations given, but the board has no corners");
    if(in->Nobservations_board <= 0) { in->Nobservations_board = 0; in->calibration_object_width_n = in->calibration_object_height_n = 0; }
    if(in->Nobservations_point <= 0)   in->Nobservations_point = 0;
    in->problem_selections = effective_selections(in->problem_selections, *in->lensmodel, in->Nobservations_board);
    return true;
}

// the ranges with their defaults resolved: the whole problem is its own leader; a point / point-set range that was
// not given is everything on the leader and nothing elsewhere. (The frame range stays as given: end_frame >= 0 is
// what says "a shard")
static ShardRanges normalise_shard(ShardRanges s, int Npoints)
{
    const bool sharded = s.end_frame >= 0;
    if(!sharded) s.is_shard_leader = true;
    if(!sharded || s.end_point < 0)    { s.begin_point = 0;    s.end_point    = s.is_shard_leader ? Npoints    : 0; }
    if(!sharded || s.end_tripoint < 0) { s.begin_tripoint = 0; s.end_tripoint = s.is_shard_leader ? 0x7fffffff : 0; }
    return s;
}

// board observations: those of the shard's frames
static std::vector<int> select_boards(const ProblemInputs& in, const ShardRanges& shard)
{
    const bool sharded = shard.end_frame >= 0;
    std::vector<int> sel;
    sel.reserve(in.Nobservations_board);
    for(int i=0; i<in.Nobservations_board; i++)
    {
        const int f = in.observations_board[i].iframe;
        if(!sharded || (f >= shard.begin_frame && f < shard.end_frame))
            sel.push_back(i);
    }
    return sel;
}

// discrete points: the shard owns the points [begin_point, end_point) (their 3x3 blocks of JtJ, their rows of x and
// J) wherever their observations sit in the caller's array (the API does not promise point-sorted
// observations)
static std::vector<int> select_points(const ProblemInputs& in, const ShardRanges& shard)
{
    std::vector<int> sel;
    for(int i=0; i<in.Nobservations_point; i++)
    {
        const int ip = in.observations_point[i].i_point;
        if(ip >= shard.begin_point && ip < shard.end_point) sel.push_back(i);
    }
    return sel;
}

// triangulated points: a point's observations are consecutive (last_in_set ends the set) and its pairs are its own,
// so the shard takes the point SETS [begin_tripoint, end_tripoint): one contiguous range of observations [*o0, *o1)
static void select_triangulated(int* o0, int* o1, const ProblemInputs& in, const ShardRanges& shard)
{
    *o0 = *o1 = 0;
    int iset = 0;
    bool in_range = false;
    for(int i=0; i<in.Nobservations_point_triangulated; i++)
    {
        const bool mine = iset >= shard.begin_tripoint && iset < shard.end_tripoint;
        if(mine && !in_range) { *o0 = i; in_range = true; }
        if(mine) *o1 = i + 1;
        if(in.observations_point_triangulated[i].last_in_set) iset++;
    }
    if(!in_range) *o0 = *o1 = 0;
}

// The STATE layout is global: every shard sees the whole state vector. The MEASUREMENT layout is local to the shard:
// its observations, and the regularization rows on the leader only
static Layout local_layout(const ProblemInputs& in, const ProblemPlan& plan)
{
    const Dims dg = make_dims(in.Ncameras_intrinsics, in.Ncameras_extrinsics, in.Nframes, in.Npoints, in.Npoints_fixed,
                              in.Nobservations_board, in.Nobservations_point,
                              in.calibration_object_width_n, in.calibration_object_height_n);
    Layout L = make_layout(dg, in.problem_selections, *in.lensmodel,
                           in.observations_point_triangulated, in.Nobservations_point_triangulated);
    const int Nboard_local = (int)plan.board_sel.size(), Npoint_local = (int)plan.point_sel.size();
    const int Ntri_local = plan.tri_o1 - plan.tri_o0;
    L.dims.Nobservations_board = Nboard_local;   // NOTE: has_warp etc. stay global
    L.dims.Nobservations_point = Npoint_local;
    L.Nmeas_boards         = Nboard_local * in.calibration_object_width_n*in.calibration_object_height_n * 2;
    L.Nmeas_points         = Npoint_local * 2;
    L.Nmeas_triangulated   = num_measurements_triangulated_initial(
        Ntri_local > 0 ? in.observations_point_triangulated + plan.tri_o0 : NULL, Ntri_local, -1);
    if(!plan.is_leader) { L.Nmeas_regularization = 0; L.has_unity_cam01 = false; L.Nreg_percamera = 0; }
    L.i_meas_boards         = 0;
    L.i_meas_points         = L.Nmeas_boards;
    L.i_meas_triangulated   = L.i_meas_points + L.Nmeas_points;
    L.i_meas_regularization = L.i_meas_triangulated + L.Nmeas_triangulated;
    L.Nmeas                 = L.i_meas_regularization + L.Nmeas_regularization;
    return L;
}

// where the next observation's rows and CSR entries begin: the three builders below pass it on
struct RowCursor { int imeas = 0; int64_t innz = 0; };

static std::vector<BoardObsMeta> build_board_meta(const ProblemInputs& in, const ProblemPlan& plan, RowCursor* at)
{
    const Layout& L = plan.L;
    const int NPTS = in.calibration_object_width_n*in.calibration_object_height_n;
    std::vector<BoardObsMeta> bmeta(plan.board_sel.size());
    for(size_t j=0; j<bmeta.size(); j++)
    {
        const mrcal_observation_board_t& o = in.observations_board[plan.board_sel[j]];
        const CameraStateIndex ic = camera_state_index(L, o.icam);
        BoardObsMeta& m = bmeta[j];
        memset(&m, 0, sizeof(m));
        m.icam_intrinsics    = o.icam.intrinsics;
        m.icam_extrinsics    = o.icam.extrinsics;
        m.iframe             = o.iframe;
        m.nnz_per_row        = nnz_per_board_row(L, o.icam.extrinsics);
        m.i_state_intrinsics = ic.intrinsics;
        m.i_state_extrinsics = ic.extrinsics;
        m.i_state_frame      = (L.Nstate_frames > 0) ? L.i_state_frames + 6*o.iframe : -1;
        m.i_meas0            = at->imeas;
        m.i_nnz0             = at->innz;
        at->imeas += 2*NPTS;
        at->innz  += (int64_t)2*NPTS*m.nnz_per_row;
    }
    return bmeta;
}

static std::vector<PointObsMeta> build_point_meta(const ProblemInputs& in, const ProblemPlan& plan, RowCursor* at)
{
    const Layout& L = plan.L;
    std::vector<PointObsMeta> pmeta(plan.point_sel.size());
    for(size_t j=0; j<pmeta.size(); j++)
    {
        const mrcal_observation_point_t& o = in.observations_point[plan.point_sel[j]];
        const CameraStateIndex ic = camera_state_index(L, o.icam);
        PointObsMeta& m = pmeta[j];
        memset(&m, 0, sizeof(m));
        const bool variable = in.problem_selections.do_optimize_frames && o.i_point < in.Npoints - in.Npoints_fixed;
        m.icam_intrinsics    = o.icam.intrinsics;
        m.icam_extrinsics    = o.icam.extrinsics;
        m.i_point            = o.i_point;
        m.nnz_per_row        = nnz_per_point_row(L, o.icam.extrinsics, o.i_point);
        m.i_state_intrinsics = ic.intrinsics;
        m.i_state_extrinsics = ic.extrinsics;
        m.i_state_point      = variable ? L.i_state_points + 3*o.i_point : -1;
        m.i_meas0            = at->imeas;
        m.i_nnz0             = at->innz;
        at->imeas += 2;
        at->innz  += 2*m.nnz_per_row;
    }
    return pmeta;
}

// triangulated points: one row per pair (i0 < i1) of observations of a point. A row has the columns of the two
// cameras' extrinsics and no others: the intrinsics are locked where there are triangulated points (dropin_inputs_ok())
static std::vector<TriPairMeta> build_tri_meta(const ProblemInputs& in, const ProblemPlan& plan, RowCursor* at)
{
    const int Ntri_local = plan.tri_o1 - plan.tri_o0;
    std::vector<TriPairMeta> tmeta;
    if(plan.L.Nmeas_triangulated <= 0) return tmeta;
    const mrcal_observation_point_triangulated_t* ot = in.observations_point_triangulated + plan.tri_o0;   // (indices local to the shard's range)
    for(int i0 = 0; i0 < Ntri_local; i0++)
    {
        if(ot[i0].last_in_set) continue;
        for(int i1 = i0+1; i1 < Ntri_local; i1++)
        {
            TriPairMeta m;
            memset(&m, 0, sizeof(m));
            m.i0 = i0; m.i1 = i1;
            m.icam_extrinsics0 = ot[i0].icam.extrinsics;
            m.icam_extrinsics1 = ot[i1].icam.extrinsics;
            m.i_state_extrinsics0 = camera_state_index(plan.L, ot[i0].icam).extrinsics;
            m.i_state_extrinsics1 = camera_state_index(plan.L, ot[i1].icam).extrinsics;
            m.i_meas = at->imeas;
            m.i_nnz0 = at->innz;
            at->imeas += 1;
            at->innz  += (m.i_state_extrinsics0 >= 0 ? 6 : 0) + (m.i_state_extrinsics1 >= 0 ? 6 : 0);
            tmeta.push_back(m);
            if(ot[i1].last_in_set) break;
        }
    }
    return tmeta;
}

// Which pose blocks are eliminated (NormalDims, solver_kernels.hpp): the frames and points, unless the extrinsics are
// the numerous ones - a moving camera against a stationary board, many rt_cam_ref and few frames
// (test_calibration_helpers.py:422-493 builds such problems) - and every row touches at most one of them, and only
// board rows touch them: a camera's block is then written whole by the workgroup that sums its observations' Grams, as
// a frame's is (no triangulated pairs, no discrete points, no unity_cam01 row). The splined models' assembly and the
// sharding know frames only. elimination = 1 / 2 (mrcal_amd_set_elimination(), or for a process that cannot call it
// the environment variable MRCAL_AMD_ELIMINATE=frames|extrinsics: problem.cpp, effective_elimination()) overrides the
// choice where both are possible
static bool choose_elim_extrinsics(const ProblemInputs& in, const ProblemPlan& plan, bool sharded, int elimination)
{
    const Layout& L = plan.L;
    const bool possible = !sharded && in.lensmodel->type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC &&
                          plan.tri_o1 == plan.tri_o0 && plan.point_sel.empty() &&
                          !in.problem_selections.do_apply_regularization_unity_cam01 && L.Nstate_extrinsics > 0;
    if(!possible || elimination == 1) return false;
    if(elimination == 2)              return true;
    return in.Ncameras_extrinsics >= 4 && L.Nstate_frames + L.Nstate_points < L.Nstate_extrinsics;
}

static NormalDims make_partition(const Layout& L, bool elim_extrinsics)
{
    NormalDims nd;
    memset(&nd, 0, sizeof(nd));
    nd.Nstate       = L.Nstate;
    nd.Nwarp        = L.Nstate_warp;
    nd.i_state_warp = L.i_state_warp;
    if(!elim_extrinsics)
    {
        nd.Nc  = L.Nstate_intrinsics + L.Nstate_extrinsics + nd.Nwarp;
        nd.NE  = L.Nstate_frames + L.Nstate_points;
        nd.Nfb = L.Nstate_frames/6;
        nd.Npb = L.Nstate_points/3;
        normal_dims_set_partition(nd, L.Nstate_intrinsics + L.Nstate_extrinsics);
    }
    else
    {
        nd.NE  = L.Nstate_extrinsics;
        nd.Nc  = L.Nstate - nd.NE;
        nd.Nfb = L.Nstate_extrinsics/6;
        nd.Npb = 0;
        nd.S_split = L.Nstate_intrinsics; nd.S_shift = nd.NE; nd.E_state0 = L.Nstate_intrinsics;
        nd.elim_extrinsics = 1;
    }
    nd.NEb = nd.Nfb + nd.Npb;
    return nd;
}

// the E blocks the shard owns: its frames, and the point blocks (the variable points only) of its point range
static BlockRanges owned_blocks(const NormalDims& nd, const ShardRanges& shard, int Nframes)
{
    BlockRanges br = { 0, nd.Nfb, 0, 0 };
    if(shard.end_frame >= 0 && nd.Nfb > 0)
    {
        br.frame_lo = shard.begin_frame < 0 ? 0 : shard.begin_frame;
        br.frame_hi = shard.end_frame > Nframes ? Nframes : shard.end_frame;
    }
    auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    br.point_lo = nd.Nfb + clampi(shard.begin_point, 0, nd.Npb);
    br.point_hi = nd.Nfb + clampi(shard.end_point,   0, nd.Npb);
    if(br.point_hi < br.point_lo) br.point_hi = br.point_lo;
    return br;
}

static DeviceProblem device_scalars(const ProblemInputs& in, const ProblemPlan& plan)
{
    const Layout& L = plan.L;
    const mrcal_problem_selections_t& sel = in.problem_selections;
    DeviceProblem D;
    memset(&D, 0, sizeof(D));
    D.lens_type   = (int)in.lensmodel->type;
    D.Nintrinsics = L.Nintrinsics;   D.Ncore = L.Ncore;        D.Ncore_state = L.Ncore_state;
    D.Ndist       = L.Ndist;         D.Ndist_state = L.Ndist_state; D.Nintr_state = L.Nintr_state;
    D.Ndist_row   = L.Nintr_per_row - (L.Ncore_state ? 2 : 0);
    D.i_state_intrinsics = L.i_state_intrinsics < 0 ? 0 : L.i_state_intrinsics;
    D.i_state_extrinsics = L.i_state_extrinsics;
    D.i_state_frames     = L.i_state_frames;
    D.i_state_points     = L.i_state_points;
    D.i_state_warp       = L.i_state_warp;
    D.Nstate = L.Nstate;  D.Nmeas = L.Nmeas;
    D.do_optimize_extrinsics = L.Nstate_extrinsics > 0;
    D.do_optimize_frames     = sel.do_optimize_frames;
    D.elim_extrinsics        = plan.nd.elim_extrinsics;
    D.has_warp_state         = L.has_warp;
    D.has_warp_seed          = (in.calobject_warp != NULL);
    D.Ncameras_intrinsics = in.Ncameras_intrinsics; D.Ncameras_extrinsics = in.Ncameras_extrinsics;
    D.Nframes = in.Nframes; D.Npoints = in.Npoints; D.Npoints_fixed = in.Npoints_fixed;
    D.Nobs_board = (int)plan.board_sel.size(); D.Nobs_point = (int)plan.point_sel.size();
    D.W = in.calibration_object_width_n; D.H = in.calibration_object_height_n;
    D.spacing = in.calibration_object_spacing;
    D.inv_Wm1 = 1.0/(double)(D.W - 1);      // (W = 1 or H = 1 with a warp: the reference divides by zero just the same)
    D.inv_Hm1 = 1.0/(double)(D.H - 1);
    if(in.calobject_warp) { D.seed_warp[0] = in.calobject_warp->x2; D.seed_warp[1] = in.calobject_warp->y2; }
    D.cfg = lens_config_of(*in.lensmodel);
    D.do_apply_regularization = sel.do_apply_regularization && plan.is_leader;
    D.has_unity_cam01         = L.has_unity_cam01;
    D.i_meas_regularization   = L.i_meas_regularization;
    D.i_nnz_regularization    = plan.innz_reg;
    D.imager_width_cam0       = (in.Ncameras_intrinsics > 0) ? (double)in.imagersizes[0] : 1.0;
    D.Npairs_tri              = (int)plan.tmeta.size();
    return D;
}

// per board observation 24 P (read qx,qy,w) + 16 P (write x) + 16 P k (write J values: innz_boards
// of them). Where the triangulated pairs ride in the board kernel's launch (board_tri_kernel) the launch the benchmark
// times carries their bytes too: per pair two observation vectors and the record read, x and the (up to) 12 partials
// written
static int64_t board_algorithmic_bytes(const ProblemPlan& plan, int NPTS, int64_t innz_boards)
{
    int64_t bytes = (int64_t)plan.board_sel.size()*NPTS*(24 + 16) + innz_boards*8;
    if(board_launch_takes_triangulated(plan.D))
        for(const TriPairMeta& m : plan.tmeta)
            bytes += 2*24 + (int64_t)sizeof(TriPairMeta) + 8 + 8*((m.i_state_extrinsics0 >= 0 ? 6 : 0) + (m.i_state_extrinsics1 >= 0 ? 6 : 0));
    return bytes;
}

bool plan_problem(ProblemPlan* out, std::string* error, const ProblemInputs& inputs, const ShardRanges& ranges,
                  int elimination)
{
    ProblemInputs in = inputs;
    if(!normalise_inputs(&in, error)) return false;
    const ShardRanges shard = normalise_shard(ranges, in.Npoints);
    const int NPTS = in.calibration_object_width_n*in.calibration_object_height_n;
    ProblemPlan& plan = *out;

    plan.is_leader = shard.is_shard_leader;
    plan.board_sel = select_boards(in, shard);
    plan.point_sel = select_points(in, shard);
    select_triangulated(&plan.tri_o0, &plan.tri_o1, in, shard);
    plan.L = local_layout(in, plan);
    const Layout& L = plan.L;

    // per-observation metadata + CSR offsets
    RowCursor at;
    plan.bmeta = build_board_meta(in, plan, &at);
    const int64_t innz_boards = at.innz;
    plan.pmeta = build_point_meta(in, plan, &at);
    plan.tmeta = build_tri_meta(in, plan, &at);
    if((int)plan.tmeta.size() != L.Nmeas_triangulated)
        return refuse(error, "internal error: %d triangulated pairs, the layout says %d", (int)plan.tmeta.size(), L.Nmeas_triangulated);
    plan.innz_reg = at.innz;
    plan.Nnz      = at.innz + num_j_nonzero_regularization(L);
    // the reference's CSR uses int32 offsets (cholmod itype int); so do we
    if(plan.Nnz > 0x7fffffffLL)
        return refuse(error, "Jacobian has %lld nonzeros: more than int32 CSR offsets can address. Shard the problem", (long long)plan.Nnz);
    // LDS of the board kernel: the 64-row tile (columns: k, +2 for the full core, +1 for the residual: board_kernel) +
    // the staged observation's pixels and weights (in whole 64-element chunks) + the joint pose record. The splined
    // models' kernels use none
    const bool splined = (in.lensmodel->type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC);
    plan.lds_bytes = splined ? 0 : (64*tile_stride(L.Ndist) + ((3*NPTS + 63) & ~63) + JOINT_REC + 4) * (int)sizeof(double);
    if(plan.lds_bytes > 160*1024)
        return refuse(error, "the board has %d corners and the lens model %d distortion parameters: the LDS tile would not fit", NPTS, L.Ndist);

    plan.nd = make_partition(L, choose_elim_extrinsics(in, plan, shard.end_frame >= 0, elimination));
    plan.br = owned_blocks(plan.nd, shard, in.Nframes);
    plan.D  = device_scalars(in, plan);
    plan.board_alg_bytes = board_algorithmic_bytes(plan, NPTS, innz_boards);
    return true;
}

} // namespace mrcal_amd

// ---- dev export: the plan of a problem, for tests/test_problem_plan.py (no declaration in include/) ----
// The arguments of mrcal_amd_problem_create_sharded(), the elimination (0 auto, 1 frames, 2 extrinsics), then out:
// the scalars below in their order, then [count | entries] lists: board_sel, point_sel, and the records of bmeta,
// pmeta and tmeta field by field in the order of their declarations (without the padding). Returns the number of
// values (nothing is written if capacity is less), or -1 with the refusal's text in error
extern "C" int mrcal_amd_debug_plan_problem(const double* intrinsics, const mrcal_pose_t* rt_cam_ref, const mrcal_pose_t* rt_ref_frame,
                                            const mrcal_point3_t* points, const mrcal_calobject_warp_t* calobject_warp,
                                            int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes, int Npoints, int Npoints_fixed,
                                            const mrcal_observation_board_t* observations_board,
                                            const mrcal_observation_point_t* observations_point,
                                            int Nobservations_board, int Nobservations_point,
                                            const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                                            int Nobservations_point_triangulated,
                                            const mrcal_point3_t* observations_board_pool, const mrcal_point3_t* observations_point_pool,
                                            const mrcal_lensmodel_t* lensmodel, const int* imagersizes,
                                            mrcal_problem_selections_t problem_selections, double calibration_object_spacing,
                                            int calibration_object_width_n, int calibration_object_height_n,
                                            int shard_begin_frame, int shard_end_frame, int shard_begin_point, int shard_end_point,
                                            int shard_begin_tripoint, int shard_end_tripoint, bool is_shard_leader,
                                            int elimination, int64_t* out, int capacity, char* error, int error_size)
{
    using namespace mrcal_amd;
    const ProblemInputs in = { intrinsics, rt_cam_ref, rt_ref_frame, points, calobject_warp,
                               Ncameras_intrinsics, Ncameras_extrinsics, Nframes, Npoints, Npoints_fixed,
                               observations_board, observations_point, Nobservations_board, Nobservations_point,
                               observations_point_triangulated, Nobservations_point_triangulated,
                               observations_board_pool, observations_point_pool, lensmodel, imagersizes,
                               problem_selections, calibration_object_spacing,
                               calibration_object_width_n, calibration_object_height_n };
    const ShardRanges shard = { shard_begin_frame, shard_end_frame, shard_begin_point, shard_end_point,
                                shard_begin_tripoint, shard_end_tripoint, is_shard_leader };
    ProblemPlan plan;
    std::string why;
    if(!plan_problem(&plan, &why, in, shard, elimination))
    {
        if(error != NULL && error_size > 0) snprintf(error, error_size, "%s", why.c_str());
        return -1;
    }
    const Layout& L = plan.L; const NormalDims& nd = plan.nd; const DeviceProblem& D = plan.D;
    std::vector<int64_t> v = {
        L.Nstate, L.Nmeas, L.Nmeas_boards, L.Nmeas_points, L.Nmeas_triangulated, L.Nmeas_regularization,
        L.i_meas_boards, L.i_meas_points, L.i_meas_triangulated, L.i_meas_regularization,
        L.i_state_intrinsics, L.i_state_extrinsics, L.i_state_frames, L.i_state_points, L.i_state_warp,
        L.Nstate_intrinsics, L.Nstate_extrinsics, L.Nstate_frames, L.Nstate_points, L.Nstate_warp,
        L.Nintr_state, L.Nintr_per_row, L.Nreg_percamera, L.has_unity_cam01,
        plan.tri_o0, plan.tri_o1, plan.Nnz, plan.innz_reg, plan.lds_bytes, plan.board_alg_bytes, plan.is_leader,
        nd.Nstate, nd.Nwarp, nd.i_state_warp, nd.Nc, nd.NE, nd.Nfb, nd.Npb, nd.NEb, nd.S_split, nd.S_shift, nd.E_state0, nd.elim_extrinsics,
        plan.br.frame_lo, plan.br.frame_hi, plan.br.point_lo, plan.br.point_hi,
        D.Nstate, D.Nmeas, D.Nobs_board, D.Nobs_point, D.Npairs_tri, D.W, D.H, D.elim_extrinsics,
        D.do_apply_regularization, D.has_unity_cam01, D.i_meas_regularization, D.i_nnz_regularization };
    auto list = [&v](size_t count) { v.push_back((int64_t)count); };
    list(plan.board_sel.size()); v.insert(v.end(), plan.board_sel.begin(), plan.board_sel.end());
    list(plan.point_sel.size()); v.insert(v.end(), plan.point_sel.begin(), plan.point_sel.end());
    list(9*plan.bmeta.size());
    for(const BoardObsMeta& m : plan.bmeta)
        v.insert(v.end(), { m.icam_intrinsics, m.icam_extrinsics, m.iframe, m.nnz_per_row,
                            m.i_state_intrinsics, m.i_state_extrinsics, m.i_state_frame, m.i_meas0, m.i_nnz0 });
    list(9*plan.pmeta.size());
    for(const PointObsMeta& m : plan.pmeta)
        v.insert(v.end(), { m.icam_intrinsics, m.icam_extrinsics, m.i_point, m.nnz_per_row,
                            m.i_state_intrinsics, m.i_state_extrinsics, m.i_state_point, m.i_meas0, m.i_nnz0 });
    list(8*plan.tmeta.size());
    for(const TriPairMeta& m : plan.tmeta)
        v.insert(v.end(), { m.i0, m.i1, m.icam_extrinsics0, m.icam_extrinsics1,
                            m.i_state_extrinsics0, m.i_state_extrinsics1, m.i_meas, m.i_nnz0 });
    if((int)v.size() <= capacity) memcpy(out, v.data(), v.size()*sizeof(int64_t));
    return (int)v.size();
}
