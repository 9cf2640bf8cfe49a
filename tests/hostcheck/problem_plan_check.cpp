// TEST-ONLY stand-alone program: plan_problem() (mrcal_amd/csrc/problem_plan.cpp) under the host sanitizers, on the
// problems of tests/test_problem_plan.py - case A whole, its shards, with triangulated points, and the three refusals.
// Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("problem_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../mrcal_amd/csrc/problem_plan.hpp"
#include "../../mrcal_amd/csrc/lens_dispatch.hpp"

using namespace mrcal_amd;

// The one function the plan calls that is compiled with the kernels (kernels.hip, not linked here): whether the
// triangulated pairs ride in the board kernel's launch. Restated for this program only
namespace mrcal_amd {
bool board_launch_takes_triangulated(const DeviceProblem& P)
{
    const int ndist = lens_ndist(P.lens_type);
    const bool allopt = ((16 + ndist) & 1) == 0 && P.Ncore_state && (ndist == 0 || P.Ndist_state) && P.do_optimize_extrinsics &&
                        P.do_optimize_frames && P.has_warp_state && P.has_warp_seed;
    return P.Nobs_board > 0 && P.Npairs_tri > 0 && P.lens_type != MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC && !allopt;
}
}

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

struct CaseA
{
    std::vector<double> intrinsics = std::vector<double>(2*8, 0.5);
    mrcal_pose_t rt_cam_ref[1] = {}, rt_ref_frame[3] = {};
    mrcal_point3_t points[3] = {};
    mrcal_calobject_warp_t warp = {};
    mrcal_observation_board_t boards[6];
    mrcal_observation_point_t pts[4];
    mrcal_observation_point_triangulated_t tri[5];
    std::vector<mrcal_point3_t> board_pool = std::vector<mrcal_point3_t>(6*6), point_pool = std::vector<mrcal_point3_t>(4);
    mrcal_lensmodel_t lensmodel;
    int imagersizes[4] = { 640, 480, 640, 480 };
    CaseA()
    {
        memset(&lensmodel, 0, sizeof(lensmodel)); lensmodel.type = MRCAL_LENSMODEL_OPENCV4;
        for(int f = 0; f < 3; f++) for(int c = 0; c < 2; c++) { boards[2*f + c].icam = { c, c - 1 }; boards[2*f + c].iframe = f; }
        const int p[4][3] = { {0, 0, -1}, {1, 1, 0}, {0, 1, 0}, {2, 0, -1} };
        for(int i = 0; i < 4; i++) { pts[i].i_point = p[i][0]; pts[i].icam = { p[i][1], p[i][2] }; }
        memset(tri, 0, sizeof(tri));
        const int t[5][2] = { {0, -1}, {1, 0}, {1, 0}, {1, 0}, {0, -1} };
        for(int i = 0; i < 5; i++) tri[i].icam = { t[i][0], t[i][1] };
        tri[2].last_in_set = true; tri[4].last_in_set = true;
    }
    ProblemInputs inputs(bool triangulated) const
    {
        mrcal_problem_selections_t sel;
        memset(&sel, 0, sizeof(sel));
        sel.do_optimize_intrinsics_core = sel.do_optimize_intrinsics_distortions = !triangulated;
        sel.do_optimize_extrinsics = sel.do_optimize_frames = sel.do_optimize_calobject_warp = true;
        sel.do_apply_regularization = sel.do_apply_regularization_unity_cam01 = true;
        return ProblemInputs{ intrinsics.data(), rt_cam_ref, rt_ref_frame, points, &warp, 2, 1, 3, 3, 1,
                              boards, pts, 6, 4, triangulated ? tri : NULL, triangulated ? 5 : 0,
                              board_pool.data(), point_pool.data(), &lensmodel, imagersizes, sel, 0.1, 3, 2 };
    }
};

static ProblemPlan planned(const ProblemInputs& in, const ShardRanges& shard, int elimination = 0)
{
    ProblemPlan plan;
    std::string error;
    CHECK(plan_problem(&plan, &error, in, shard, elimination));
    CHECK((int)plan.bmeta.size() == plan.D.Nobs_board && (int)plan.pmeta.size() == plan.D.Nobs_point);
    CHECK((int)plan.tmeta.size() == plan.L.Nmeas_triangulated && plan.nd.Nc + plan.nd.NE == plan.L.Nstate);
    return plan;
}

static std::string refused(const ProblemInputs& in)
{
    ProblemPlan plan;
    std::string error;
    CHECK(!plan_problem(&plan, &error, in, ShardRanges{ 0, -1, 0, -1, 0, -1, true }, 0));
    return error;
}

int main()
{
    const CaseA A;
    const ShardRanges whole = { 0, -1, 0, -1, 0, -1, true };
    for(int triangulated = 0; triangulated < 2; triangulated++)
    {
        const ProblemInputs in = A.inputs(triangulated != 0);
        const ProblemPlan W = planned(in, whole);
        CHECK(W.tmeta.size() == (triangulated ? 4u : 0u) && W.L.has_unity_cam01);
        const std::vector<std::vector<ShardRanges>> shardings = {
            { { 0, 2, 0, 2, 0, 1, true }, { 2, 3, 2, 3, 1, 2, false } },
            { { 0, 1, 0, 1, 0, 1, false }, { 1, 2, 1, 2, 1, 2, true }, { 2, 3, 2, 3, 2, 2, false } },
            { { 0, 0, 0, -1, 0, -1, false }, { 0, 3, 0, -1, 0, -1, true } } };
        for(const auto& shards : shardings)
        {
            int Nmeas = 0; int64_t Nnz = 0;
            for(const ShardRanges& s : shards) { const ProblemPlan P = planned(in, s); Nmeas += P.L.Nmeas; Nnz += P.Nnz; }
            CHECK(Nmeas == W.L.Nmeas && Nnz == W.Nnz);
        }
        for(int policy = 0; policy < 3; policy++) CHECK(!planned(in, whole, policy).nd.elim_extrinsics);
    }
    // the refusals: a 0-wide board; more nonzeros than int32 offsets address (counts alone, every pool NULL); an LDS
    // tile that does not fit
    ProblemInputs in = A.inputs(false);
    in.calibration_object_width_n = 0;
    CHECK(refused(in) == "board observations given, but the board has no corners");
    const int Nobs = 5369;
    std::vector<mrcal_observation_board_t> many(Nobs);
    for(int i = 0; i < Nobs; i++) { many[i].icam = { 0, 0 }; many[i].iframe = i; }
    in = A.inputs(false);
    in.intrinsics = NULL; in.rt_cam_ref = NULL; in.rt_ref_frame = NULL; in.points = NULL; in.calobject_warp = NULL;
    in.observations_board_pool = NULL; in.observations_point_pool = NULL; in.observations_point = NULL;
    in.Ncameras_intrinsics = 1; in.Nframes = Nobs; in.Npoints = in.Npoints_fixed = 0; in.Nobservations_point = 0;
    in.observations_board = many.data(); in.Nobservations_board = Nobs;
    in.calibration_object_width_n = in.calibration_object_height_n = 100;
    in.problem_selections.do_apply_regularization_unity_cam01 = false;
    CHECK(refused(in) == "Jacobian has 2147600006 nonzeros: more than int32 CSR offsets can address. Shard the problem");
    in.Nobservations_board = 1; in.Nframes = 1;
    in.calibration_object_width_n = in.calibration_object_height_n = 80;
    CHECK(refused(in) == "the board has 6400 corners and the lens model 4 distortion parameters: the LDS tile would not fit");
    printf("ok\n");
    return 0;
}
