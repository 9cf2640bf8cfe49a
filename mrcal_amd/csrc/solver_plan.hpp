// The solver's work lists, planned on the host: what problem_prepare_solver() uploads into AssemblyPlan and GenPlan
// (solver_kernels.hpp). HOST code, index arithmetic only: no HIP runtime call, no problem object. Every sum of the solve
// goes by these lists in a fixed order, so they define the numbers it produces; tests/test_solver_plan.py executes them
// on the CPU.
#pragma once
#include <stdint.h>
#include <map>
#include <vector>
#include "solver_kernels.hpp"

namespace mrcal_amd {

// The finalize lists of both plans (AssemblyPlan::dest_*, GenPlan::dest_*): for every destination - [0,Nc^2) entry of
// A, then Nc entries of g (S index), then |x|^2 - its sources (pair or group) << 10 | position, in the order given
typedef std::map<int, std::vector<int>> DestSources;
struct DestLists { std::vector<int> id, begin, src; };
DestLists make_dest_lists(const DestSources& sources);

// The lists of AssemblyPlan that the board observations' Grams are summed by, named as its fields
struct BoardGramPlan
{
    int Nchunks = 0, Npairs = 0;
    std::vector<int>    frame_obs_begin, frame_obs;      // (frame_obs: with elim_extrinsics only)
    std::vector<int>    chunk_begin, pair_obs, obs_pair, chunk_pair;
    std::vector<int>    pos_table;
    std::vector<PairOp> pair_table;
    std::vector<int>    frame_pos, obs_cols;
    std::vector<int>    pair_chunk_begin;
    DestLists           dest;
};
// meta: the D.Nobs_board observations, sorted by frame. Neblocks: the 6x6 blocks an observation's eliminated pose can
// be (the frames; with elim_extrinsics the cameras that have extrinsics). false: set_error() says why
bool plan_board_grams(const DeviceProblem& D, const NormalDims& nd, const BoardObsMeta* meta, int Neblocks, BoardGramPlan* plan);

// The lists of GenPlan, named as its fields. Nrows == 0: no plan, the rows go one lane each
struct GenRowsPlan
{
    int Nrows = 0, Nchunks = 0, Ngroups = 0, stride = 0, kmax = 0;
    std::vector<int> rows, chunk_begin, chunk_group, group_k, group_off, spos, scol;
    DestLists        dest;
    std::vector<int> group_chunk_begin;
    std::vector<int> eb_block, eb_begin, eb_rows, eb_group, eb_epos;
};
// rows [r0, r1) of the CSR structure: rowptr[0 .. r1-r0] as the whole matrix has them, colidx from rowptr[0] on
GenRowsPlan plan_gen_rows(const NormalDims& nd, int r0, int r1, const int32_t* rowptr, const int32_t* colidx);

} // namespace mrcal_amd
