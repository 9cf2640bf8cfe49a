// The problem as the kernels see it: a POD passed by value at launch, pointing
// at HBM-resident arrays that live for the life of a mrcal_amd_problem_t.
//
// HBM layout (all allocated once in mrcal_amd_problem_create()):
//
//   seeds (unpacked units; used for any block that is locked down)
//     seed_intrinsics   double[Nci][Nintrinsics]
//     seed_rt_cam_ref   double[Nce][6]
//     seed_rt_ref_frame double[Nf][6]
//     seed_points       double[Npoints][3]
//   observations
//     board_meta        BoardObsMeta[Nobs_board]     (indices + CSR offsets)
//     board_pool        double[Nobs_board][H][W][3]  (qx,qy,weight)
//     point_meta        PointObsMeta[Nobs_point]
//     point_pool        double[Nobs_point][3]
//   per-evaluation scratch
//     joint             double[Nobs_board][JOINT_STRIDE]   (see JointPose below)
//   outputs
//     b_packed          double[Nstate]
//     x                 double[Nmeas]
//     J_rowptr          int32[Nmeas+1]    } CSR of J, identical to what the
//     J_colidx          int32[Nnz]        } reference's callback writes into
//     J_values          double[Nnz]       } Jt->p, Jt->i, Jt->x
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "layout.hpp"
#include "lens_models.hpp"

namespace mrcal_amd {

// iteration-invariant description of one board observation
struct BoardObsMeta
{
    int32_t icam_intrinsics;
    int32_t icam_extrinsics;   // <0: camera sits at the reference
    int32_t iframe;
    int32_t nnz_per_row;       // k
    int32_t i_state_intrinsics;// first state index of this camera's intrinsics; <0 if none
    int32_t i_state_extrinsics;// <0 if none in this row
    int32_t i_state_frame;     // <0 if none
    int32_t i_meas0;           // first measurement row of this observation
    int64_t i_nnz0;            // first CSR entry of this observation
    int64_t _pad;
};
static_assert(sizeof(BoardObsMeta) == 48, "BoardObsMeta layout");

struct PointObsMeta
{
    int32_t icam_intrinsics;
    int32_t icam_extrinsics;
    int32_t i_point;
    int32_t nnz_per_row;
    int32_t i_state_intrinsics;
    int32_t i_state_extrinsics;
    int32_t i_state_point;     // <0 if this point is fixed / not optimized
    int32_t i_meas0;
    int64_t i_nnz0;
    int64_t _pad;
};
static_assert(sizeof(PointObsMeta) == 48, "PointObsMeta layout");

// One row of the triangulated-point residuals: a pair (i0 < i1) of observations
// of one point (mrcal.c:5180-5653)
struct TriPairMeta
{
    int32_t i0, i1;                 // indices into the triangulated observations
    int32_t icam_extrinsics0;       // <0: that camera sits at the reference
    int32_t icam_extrinsics1;
    int32_t i_state_extrinsics0;    // first state index of camera 0's rt; <0 if none in this row
    int32_t i_state_extrinsics1;
    int32_t i_meas;
    int32_t _pad;
    int64_t i_nnz0;
};
static_assert(sizeof(TriPairMeta) == 40, "TriPairMeta layout");

// The per-observation geometry the board kernel needs, produced by the
// prologue kernel (one lane per observation) and consumed wave-uniformly.
//
// With the joint transform  p = Rj pt + tj,  pt = (X,Y,Z) a board corner:
//   dp_i/drc_l = X Mc[0][i][l] + Y Mc[1][i][l] + Z Mc[2][i][l] + dtj_drc[i][l]
//   dp_i/drf_l = X Mf[0][i][l] + Y Mf[1][i][l] + Z Mf[2][i][l]
//   dp/dtc     = I,   dp/dtf = dtj_dtf
// where M?[j][i][l] = sum_k dRj[i][j]/drj[k] drj[k]/dr?[l]. Folding the chain
// rule through the joint rotation ONCE per observation turns the reference's
// per-point 3x(3x3)(3x3) products (mrcal.c:2304-2361) into 3 axpys per point
enum
{
    JOINT_R       = 0,    // 9
    JOINT_T       = 9,    // 3
    JOINT_MC      = 12,   // 27
    JOINT_DTJ_DRC = 39,   // 9
    JOINT_MF      = 48,   // 27
    JOINT_DTJ_DTF = 75,   // 9
    JOINT_REC     = 84,   // what the board kernels read of a record
    JOINT_STRIDE  = 112   // doubles between records: 896 bytes, 7 cache lines
};

// The Jacobian tile of a board observation, as the board kernel lays it out in
// LDS: one row per measurement, columns at FIXED positions that depend on the
// lens model only (NDIST = its number of distortion parameters), whether or
// not the corresponding block is being optimized:
//
//   [0..3]   fx fy cx cy      an x row holds (dq/dfx, 0, w, 0), a y row (0, dq/dfy, 0, w)
//   [4..)    distortions      NDIST
//   [EXT0..) r_cam t_cam      6
//   [FRAME0..) r_frame t_frame 6
//   [WARP0..) warp            2
//   [XCOL]   the residual x
//   padding to a multiple of 4, zero
//
// Blocks that are not in the state (or a camera that sits at the reference)
// hold zeros. The fixed layout costs a few zero columns in the Gram; it buys
// compile-time register indexing in the kernel.
__host__ __device__ inline int tile_ext0  (int ndist) { return 4 + ndist; }
__host__ __device__ inline int tile_frame0(int ndist) { return 4 + ndist + 6; }
__host__ __device__ inline int tile_warp0 (int ndist) { return 4 + ndist + 12; }
__host__ __device__ inline int tile_xcol  (int ndist) { return 4 + ndist + 14; }
__host__ __device__ inline int tile_ncols (int ndist) { return 4 + ndist + 15; }
__host__ __device__ inline int tile_nblk  (int ndist) { return (tile_ncols(ndist) + 3) >> 2; }
// LDS row stride in doubles: odd (conflict-free per-lane column writes), >= 4 nblk
__host__ __device__ inline int tile_stride_blk(int nblk) { return (4*nblk) | 1; }
__host__ __device__ inline int tile_stride(int ndist) { return tile_stride_blk(tile_nblk(ndist)); }
// The ROWS of the tile. A pass of the board kernel takes 64 corners, a lane each, and sends their 128 rows through
// the 64-row tile in two halves of 32 corners; logical row r = 2 c + xy of a half is the x or y row of its corner c.
// The kernels with everything optimized write one tile row a lane, lanes 0..31 the half's x rows and lanes 32..63
// its y rows: sixteen lanes, sixteen consecutive rows of odd stride, no two on one LDS bank. Which corner a lane
// takes is then free, and it is chosen for the Gram: a full k-step s sums the logical rows s, s+16, s+32, s+48 -
// corners c, c+8, c+16, c+24 - and the two rows that a 32-lane half of the wave reads must lie 16 tile rows
// (32 banks) apart. In-half lane j takes corner j/2 + 16 (j%2): corner c sits in lane 2c (mod 32) + c/16, the corners
// 8 apart in lanes 16 apart. The other board kernels keep lane = corner and the rows in order, tile row = r.
__host__ __device__ constexpr int board_lane_corner(int lane) { return (lane & 32) | ((lane >> 1) & 15) | ((lane & 1) << 4); }
__host__ __device__ constexpr int board_tile_row(bool row_a_lane, int r)
{
    return row_a_lane ? 32*(r & 1) + ((r & ~1) & 31) + (r >> 5) : r;
}
// The tile row that lanes 16k..16k+15 read at k-step s of the Gram: a full half sums the logical rows s + 16k in a
// k-step, a partial one (the last corners of a board) the rows 4s + k. The kernel adds a lane's row of step 0 and
// the step's row for k = 0: board_gram_row(s, k) = board_gram_row(s, 0) + board_gram_row(0, k) in both layouts
// (tests/hostcheck/gram_banks_check.cpp)
__host__ __device__ constexpr int board_gram_row(bool row_a_lane, bool full, int s, int k)
{
    return board_tile_row(row_a_lane, full ? s + 16*k : 4*s + k);
}

// Per-board-observation Gram matrix G = Tt T of the tile, formed with
// v_mfma_f64_4x4x4f64 (4 independent 4x4 products per instruction, one per
// "slot"; k = 4 tile rows per step). Measured operand layout on gfx950
// (tools/mfma_f64_4x4x4_layout_probe.hip):
//   A lane = 16 k + 4 slot + i     B lane = 16 k + 4 slot + j     D lane = 16 i + 4 slot + j
// G is cut into 4x4 blocks (NBLK = ncols/4 of them per side). An operand is ONE
// LDS read per lane, tile[row 4 step + l/16][4 blk(slot) + l%4], which serves
// as A or B alike and holds one column block per slot - any four blocks: the
// lane's column is a loop invariant, so an arbitrary choice costs an address
// register and nothing else. An operand may instead be another one with its
// slots rotated (DPP row_ror, no LDS traffic, two vector moves).
// An MFMA multiplies two operands slot by slot: slot s yields the block pair
// (A.blk[s], B.blk[s]). A packing (GramPacking) lists the operands and the
// MFMAs of one k-step so that every unordered block pair sits in exactly one
// "valid" slot; the other slots repeat a pair and are ignored downstream.
// NBLK(NBLK+1)/2 pairs in 4 slots an instruction: 7 MFMAs for the 7 blocks
// (27 columns) of OPENCV8, 28 pairs in 28 slots, and 6 for 6 blocks, where
// forming everything from X = (0,1,2,3), Y = the rest and their rotations costs
// 10, and X, its rotations and cyclic operands Y_q (slot s: block 4 + (s+q) % ny)
// cost 8 and 7. The matrix instructions and the rotations' moves go down the
// one FP64 pipe that limits the board kernel, the LDS reads do not: at 6 and 7
// blocks every operand is a read, 8 a k-step for 7 blocks (measured: LEDGER,
// "The Gram in the fewest matrix instructions"). 5 and 8 blocks keep X, Y and
// rotations.
// WHICH four blocks share an operand decides its LDS bank conflicts. A 32-lane
// half of a ds_read_b64 reads two tile rows, 16 rows apart in a full half-tile:
// 16 odd strides = 32 (mod 64) dwords, and a column block is 8 dwords wide, so
// block b of the one row and block b+4 of the other share their banks. At 6 and
// 7 blocks no operand holds a block together with the block four positions on
// (Z, P and Q at 7 and X2, Z at 6 are chosen for that): every read of a full
// half is conflict-free. gram_read_extra_cycles() counts it.
// The accumulators are stored as they are, gram[iobs][m][lane]: lane l of
// accumulator m holds G[4 bA + l/16][4 bB + l%4], (bA,bB) the pair in slot (l%16)/4.
enum { GRAM_MAXOP = 10, GRAM_MAXMFMA = 10 };
struct GramOperand
{
    int blk[4];     // the column block in each slot
    int src, rot;   // src < 0: an LDS read. Else operand `src` rotated: slot s holds src's slot (s + rot) % 4
};
struct GramMfma { int a, b, valid; };  // operands; bit s of valid: slot s holds a pair that no other slot does
struct GramPacking
{
    int nop, nmfma;
    GramOperand op[GRAM_MAXOP];       // the LDS reads first: read number = operand number
    GramMfma    mfma[GRAM_MAXMFMA];
};
__host__ __device__ constexpr void gram_add_read(GramPacking& p, int b0, int b1, int b2, int b3)
{
    p.op[p.nop++] = GramOperand{ {b0, b1, b2, b3}, -1, 0 };
}
__host__ __device__ constexpr void gram_add_rot(GramPacking& p, int src, int rot)
{
    const GramOperand& o = p.op[src];
    p.op[p.nop++] = GramOperand{ {o.blk[rot & 3], o.blk[(1+rot) & 3], o.blk[(2+rot) & 3], o.blk[(3+rot) & 3]}, src, rot };
}
__host__ __device__ constexpr void gram_add_mfma(GramPacking& p, int a, int b, int valid = 0xf)
{
    p.mfma[p.nmfma++] = GramMfma{ a, b, valid };
}
// board tiles have 5..8 column blocks (NDIST = 0..12)
__host__ __device__ constexpr GramPacking gram_packing(int nblk)
{
    GramPacking p{};
    if(nblk == 5)
    {
        gram_add_read(p, 0,1,2,3);                  // 0: X
        gram_add_read(p, 4,4,4,4);                  // 1: Y
        gram_add_rot (p, 0, 1);                     // 2: X1 = (1,2,3,0)
        gram_add_rot (p, 0, 2);                     // 3: X2 = (2,3,0,1)
        gram_add_mfma(p, 0, 0);                     // the diagonal blocks of X
        gram_add_mfma(p, 0, 2);                     // (0,1) (1,2) (2,3) and the mirrored (3,0)
        gram_add_mfma(p, 0, 3, 0x3);                // (0,2) (1,3)
        gram_add_mfma(p, 1, 1, 0x1);                // (4,4)
        gram_add_mfma(p, 0, 1);                     // (s,4)
    }
    else if(nblk == 6)
    {
        gram_add_read(p, 0,1,2,3);                  // 0: X
        gram_add_read(p, 1,2,3,0);                  // 1: X1
        gram_add_read(p, 2,3,0,1);                  // 2: X2
        gram_add_read(p, 4,5,4,5);                  // 3: Y_0
        gram_add_read(p, 5,4,5,4);                  // 4: Y_1
        gram_add_read(p, 4,5,5,4);                  // 5: Z
        gram_add_mfma(p, 0, 0);                     // the diagonal blocks of X
        gram_add_mfma(p, 0, 1);                     // (0,1) (1,2) (2,3) and the mirrored (3,0)
        gram_add_mfma(p, 0, 2, 0x3);                // (0,2) (1,3)
        gram_add_mfma(p, 0, 3);                     // (0,4) (1,5) (2,4) (3,5)
        gram_add_mfma(p, 0, 4);                     // (0,5) (1,4) (2,5) (3,4)
        gram_add_mfma(p, 3, 5, 0x7);                // (4,4) (5,5) (4,5)
    }
    else if(nblk == 7)
    {
        gram_add_read(p, 0,1,2,3);                  // 0: X
        gram_add_read(p, 1,2,3,0);                  // 1: X1
        gram_add_read(p, 4,5,6,4);                  // 2, 3, 4: Y_q, slot s holds block 4 + (s+q)%3
        gram_add_read(p, 5,6,4,5);
        gram_add_read(p, 6,4,5,6);
        gram_add_read(p, 4,5,6,5);                  // 5: Z
        gram_add_read(p, 0,1,6,6);                  // 6: P
        gram_add_read(p, 2,3,4,5);                  // 7: Q
        gram_add_mfma(p, 0, 0);                     // the diagonal blocks of X
        gram_add_mfma(p, 0, 1);                     // (0,1) (1,2) (2,3) and the mirrored (3,0)
        gram_add_mfma(p, 0, 2);                     // X x Y: (s, 4 + (s+q)%3), q = 0,1,2
        gram_add_mfma(p, 0, 3);
        gram_add_mfma(p, 0, 4);
        gram_add_mfma(p, 2, 5);                     // (4,4) (5,5) (6,6) (4,5)
        gram_add_mfma(p, 6, 7);                     // (0,2) (1,3) (6,4) (6,5)
    }
    else if(nblk == 8)
    {
        gram_add_read(p, 0,1,2,3);                  // 0: X
        gram_add_read(p, 4,5,6,7);                  // 1: Y
        gram_add_rot (p, 0, 1);                     // 2, 3: X1, X2
        gram_add_rot (p, 0, 2);
        gram_add_rot (p, 1, 1);                     // 4, 5, 6: Y1, Y2, Y3
        gram_add_rot (p, 1, 2);
        gram_add_rot (p, 1, 3);
        gram_add_mfma(p, 0, 0);
        gram_add_mfma(p, 0, 2);
        gram_add_mfma(p, 0, 3, 0x3);
        gram_add_mfma(p, 1, 1);
        gram_add_mfma(p, 1, 4);
        gram_add_mfma(p, 1, 5, 0x3);
        gram_add_mfma(p, 0, 1);                     // X x Y: (s, 4 + (s+r)%4), r = 0..3
        gram_add_mfma(p, 0, 4);
        gram_add_mfma(p, 0, 5);
        gram_add_mfma(p, 0, 6);
    }
    return p;
}
// LDS reads per step (they come first among the operands)
__host__ __device__ constexpr int gram_nreads(int nblk)
{
    const GramPacking p = gram_packing(nblk);
    int n = 0;
    for(int o = 0; o < p.nop; o++) if(p.op[o].src < 0) n++;
    return n;
}
// number of accumulators. (Spelt out: device code asks at run time)
__host__ __device__ constexpr int gram_nmfma_blk(int nblk) { return nblk == 8 ? 10 : (nblk >= 5 && nblk <= 7) ? nblk : 0; }
static_assert(gram_packing(5).nmfma == gram_nmfma_blk(5) && gram_packing(6).nmfma == gram_nmfma_blk(6) &&
              gram_packing(7).nmfma == gram_nmfma_blk(7) && gram_packing(8).nmfma == gram_nmfma_blk(8), "gram_nmfma_blk()");
__host__ __device__ inline int gram_stride(int ndist) { return gram_nmfma_blk(tile_nblk(ndist))*64; }
// position pos = 64 m + lane of a stored Gram -> the entry G[i][j] it holds.
// diag: the entry is in a diagonal 4x4 block, where (i,j) and (j,i) are both
// stored; elsewhere only one of them is (i > j can happen: mirrored blocks).
// Returns false for the slots that repeat a pair
__host__ __device__ inline bool gram_pos_to_entry(int nblk, int pos, int* i, int* j, bool* diag)
{
    const GramPacking p = gram_packing(nblk);
    const int lane = pos & 63, s = (lane >> 2) & 3, m = pos >> 6;
    if(m >= p.nmfma || !((p.mfma[m].valid >> s) & 1)) return false;
    const int bA = p.op[p.mfma[m].a].blk[s], bB = p.op[p.mfma[m].b].blk[s];
    *i = 4*bA + (lane >> 4);
    *j = 4*bB + (lane & 3);
    *diag = (bA == bB);
    return true;
}
// tile column this lane reads for operand `iread` < gram_nreads()
__host__ __device__ inline int gram_read_col(int nblk, int iread, int lane)
{
    return 4*gram_packing(nblk).op[iread].blk[(lane >> 2) & 3] + (lane & 3);
}
// Extra LDS cycles (what SQ_LDS_BANK_CONFLICT counts) of ONE k-step's read of operand `iread`, by the bank rule of
// ds_read_b64: the two 32-lane halves of the wave are served one after the other; the bank of a dword is its index
// mod 64; lanes of a half at the same address are one access; a half costs as many cycles as its busiest bank has
// distinct dwords. The rows are the kernel's (kernels.hip, gram_copy_fused()): lanes 16k..16k+15 read row s + 16k of
// a full half-tile and row 4s + k of a partial one; s shifts every address alike and changes nothing. Host only
inline int gram_read_extra_cycles(int nblk, int iread, bool full)
{
    const int ks = tile_stride_blk(nblk);
    int extra = 0;
    for(int half = 0; half < 2; half++)
    {
        int dwords[64][64], n[64] = {0};        // the distinct dwords asked of each bank
        for(int lane = 32*half; lane < 32*half + 32; lane++)
        {
            const int row = (full ? 16 : 1)*(lane >> 4);
            for(int w = 0; w < 2; w++)
            {
                const int dword = 2*(row*ks + gram_read_col(nblk, iread, lane)) + w, bank = dword & 63;
                bool seen = false;
                for(int i = 0; i < n[bank]; i++) seen = seen || dwords[bank][i] == dword;
                if(!seen) dwords[bank][n[bank]++] = dword;
            }
        }
        int busiest = 1;
        for(int bank = 0; bank < 64; bank++) if(n[bank] > busiest) busiest = n[bank];
        extra += busiest - 1;
    }
    return extra;
}

struct DeviceProblem
{
    // layout
    int lens_type;
    int Nintrinsics, Ncore, Ncore_state, Ndist, Ndist_state, Nintr_state;
    int Ndist_row;       // distortion columns in one board/point row: Ndist_state, or (order+1)^2 for splined models
    int i_state_intrinsics, i_state_extrinsics, i_state_frames, i_state_points, i_state_warp;
    int Nstate, Nmeas;
    int do_optimize_extrinsics, do_optimize_frames;
    int elim_extrinsics;       // the solver eliminates the extrinsics blocks, not the frames (NormalDims, solver_kernels.hpp)
    int has_warp_state;  // warp is a state variable
    int has_warp_seed;   // a warp was given (it is applied whether optimized or not)
    int Ncameras_intrinsics, Ncameras_extrinsics, Nframes, Npoints, Npoints_fixed;
    int Nobs_board, Nobs_point;
    int W, H;
    double spacing;
    double inv_Wm1, inv_Hm1;   // 1/(W-1), 1/(H-1): the board warp's normalized coordinates
    double seed_warp[2];

    // model configuration that is not in the intrinsics vector
    LensConfig cfg;

#ifdef MRCAL_AMD_DEV
    // MEASUREMENT BUILDS ONLY (bash csrc/build.sh -DMRCAL_AMD_DEV [-DBOARD_TS ...] -> libmrcal_amd_dev.so; the shipped
    // library has neither field nor any of the code behind them). Ablation knob of tools/probe_board.py: bit0 skip the J
    // copy-out, bit1 skip the MFMAs, bit2 skip the projection arithmetic, bit4 exit after the start-up loads,
    // bit5 (32) write the tile's rows by lane where the kernel keeps them in order (wrong results, no write conflicts)
    int debug_ablate;
    long long* debug_ts;     // per-observation phase timestamps (-DBOARD_TS)
#endif

    // regularization
    int do_apply_regularization;
    int has_unity_cam01;
    int i_meas_regularization;
    int64_t i_nnz_regularization;
    double imager_width_cam0;

    const double* seed_intrinsics;
    const double* seed_rt_cam_ref;
    const double* seed_rt_ref_frame;
    const double* seed_points;

    const BoardObsMeta* board_meta;
    const double*       board_pool;
    const PointObsMeta* point_meta;
    const double*       point_pool;
    // triangulated points: pairs, the observation vectors (3 doubles each, in
    // their camera's coordinates) and the outlier marks (one int per observation)
    int                 Npairs_tri;
    const TriPairMeta*  tri_meta;
    const double*       tri_px;
    const int*          tri_outlier;
    const int*          imagersizes;

    // state unpacked by the prologue kernel, every evaluation:
    //   [Ncameras_intrinsics][Nintrinsics] intrinsics, then the 2 warp values
    const double*       unpacked;
};

// The input checks mrcal_optimize() and mrcal_optimizer_callback() share (mrcal.c:6049-6060, 6250-6270), with the
// reference's messages (set_error): triangulated points only with the intrinsics locked and the extrinsics optimized; a
// warp that is optimized needs a seed. warp_seed_first: which of the two is reported when both fail - the reference's
// mrcal_optimize() looks at the warp seed first, its callback at the triangulated points
bool dropin_inputs_ok(mrcal_problem_selections_t problem_selections,
                      const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                      int Nobservations_point_triangulated,
                      int Nobservations_board, const mrcal_calobject_warp_t* calobject_warp,
                      bool warp_seed_first);

} // namespace mrcal_amd
