// What mrcal_amd_problem_create_sharded() works out before it touches the device: which observations the shard owns,
// the measurement layout local to it, every observation's record with its CSR offsets, the sizes that follow, the
// elimination partition and the scalar half of DeviceProblem. HOST code, arithmetic on the caller's arrays only: no
// HIP runtime call, no problem object, no environment. problem_create() (problem.cpp) allocates and uploads what the
// plan says and decides nothing; tests/test_problem_plan.py holds the plan to the reference on the CPU.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "layout.hpp"
#include "problem.hpp"
#include "solver_kernels.hpp"

namespace mrcal_amd {

// the arguments of mrcal_amd_problem_create_sharded() up to the board's size, as given: nothing is copied
struct ProblemInputs
{
    const double*                 intrinsics;
    const mrcal_pose_t*           rt_cam_ref;
    const mrcal_pose_t*           rt_ref_frame;
    const mrcal_point3_t*         points;
    const mrcal_calobject_warp_t* calobject_warp;
    int Ncameras_intrinsics, Ncameras_extrinsics, Nframes;
    int Npoints, Npoints_fixed;
    const mrcal_observation_board_t* observations_board;
    const mrcal_observation_point_t* observations_point;
    int Nobservations_board;
    int Nobservations_point;
    const mrcal_observation_point_triangulated_t* observations_point_triangulated;
    int Nobservations_point_triangulated;
    const mrcal_point3_t* observations_board_pool;
    const mrcal_point3_t* observations_point_pool;
    const mrcal_lensmodel_t* lensmodel;
    const int* imagersizes;
    mrcal_problem_selections_t problem_selections;
    double calibration_object_spacing;
    int calibration_object_width_n;
    int calibration_object_height_n;
};

// ... and the rest of them. end_frame < 0: the whole problem. Anything else is a shard, even an empty frame range (a
// points-only problem under the multi-GPU driver gives every rank the range (0,0)). end_point / end_tripoint < 0: all
// the discrete points / triangulated point sets with the leader, none elsewhere
struct ShardRanges
{
    int begin_frame, end_frame;
    int begin_point, end_point;
    int begin_tripoint, end_tripoint;
    bool is_shard_leader;
};

struct ProblemPlan
{
    Layout                    L;                  // state layout global, measurement layout local to the shard
    std::vector<int>          board_sel;          // the caller's index of each local board observation
    std::vector<int>          point_sel;          // ... of each local point observation
    int                       tri_o0 = 0, tri_o1 = 0;   // the shard's triangulated observations [tri_o0, tri_o1) of the caller's
    std::vector<BoardObsMeta> bmeta;
    std::vector<PointObsMeta> pmeta;
    std::vector<TriPairMeta>  tmeta;              // (i0, i1: local to [tri_o0, tri_o1))
    int64_t                   Nnz = 0;
    int64_t                   innz_reg = 0;       // first CSR entry of the regularization rows
    int                       lds_bytes = 0;      // LDS of the board kernel
    int64_t                   board_alg_bytes = 0;// algorithmic HBM bytes of one board-kernel launch
    NormalDims                nd;
    BlockRanges               br;
    bool                      is_leader = true;
    DeviceProblem             D;                  // every scalar set, every pointer NULL
};

// elimination: 0 the plan chooses, 1 the frames and points, 2 the extrinsics where the problem allows it.
// false: *error says why the inputs are refused, *out is not to be used
bool plan_problem(ProblemPlan* out, std::string* error, const ProblemInputs& in, const ShardRanges& shard,
                  int elimination /* 0 auto, 1 frames, 2 extrinsics */);

} // namespace mrcal_amd
