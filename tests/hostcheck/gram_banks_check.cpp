// TEST-ONLY stand-alone program: the LDS bank conflicts of the board kernel's tile traffic, counted on the host by the
// bank rules of the DS instructions, for the packings of mrcal_amd/csrc/problem.hpp:
//   - at 6 and 7 column blocks every operand read of a FULL half-tile costs 0 extra LDS cycles by
//     gram_read_extra_cycles(); the function agrees with an independent count made here from first principles
//   - the per-source table of one 10x10 OPENCV8 observation (7 blocks, row stride 29 doubles, 24 nonzeros a row: three
//     full halves of 16 k-steps and a partial one of 2) is printed: what SQ_LDS_BANK_CONFLICT should read per wave.
//     The copy-out's addresses and the tile writes' rows are restated here from kernels.hip (copy_out_invariants(),
//     fused_step(), board_observation()): a model of the kernel, not the kernel. Both layouts of the tile's rows are
//     counted: the rows in order (the general kernels) and one row a lane (the kernels with everything optimized)
//   - one row a lane (problem.hpp, board_lane_corner(), board_tile_row(), board_gram_row()): the lanes' rows are a
//     bijection of the 64 lanes onto the 64 tile rows and every 16-lane group writes without a conflict; on an
//     integer tile, for every shape of a half (32 corners, or 1..31), every k-step reads the logical rows that the
//     rows-in-order layout reads, in its k order, through the kernel's sum "the lane's row of step 0 + the step's row
//     for k = 0"; the copy-out's restated addresses fetch every stored row of every row group from the tile row that
//     holds it, each of the 64 rows exactly once, for every lens model's row length, and stay inside the LDS
//     allocation of the smallest board
// Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("gram_banks_check"): a row of its PROGRAMS. No arguments
//   (prints the table, then "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <map>
#include <vector>
#include "../../mrcal_amd/csrc/problem.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

// Extra cycles of one DS instruction moving 8 bytes a lane: the lanes are served in groups of `group` contiguous lanes,
// a group takes as many cycles as its busiest bank has distinct dwords; bank = dword index mod `nbanks`
static int extra_cycles_b64(const std::vector<int>& byte_address, int group, int nbanks)
{
    int extra = 0;
    for(size_t l0 = 0; l0 < byte_address.size(); l0 += group)
    {
        std::map<int, std::set<int>> dwords;
        for(size_t l = l0; l < l0 + group; l++)
            for(int w = 0; w < 2; w++)
            {
                CHECK(byte_address[l] >= 0 && byte_address[l] % 8 == 0);
                const int dword = byte_address[l]/4 + w;
                dwords[dword % nbanks].insert(dword);
            }
        size_t busiest = 1;
        for(const auto& b : dwords) if(b.second.size() > busiest) busiest = b.second.size();
        extra += (int)busiest - 1;
    }
    return extra;
}
// ds_read_b64: two groups of 32 lanes, 64 banks. ds_write_b64: four groups of 16 contiguous lanes, 32 banks (a
// ds_write2_b64 is taken as two of them: an assumption, which the measured counter supports - LEDGER)
static int read_b64_extra (const std::vector<int>& a) { return extra_cycles_b64(a, 32, 64); }
static int write_b64_extra(const std::vector<int>& a) { return extra_cycles_b64(a, 16, 32); }

// one operand read of k-step `step`, from first principles: the kernel's row choice and gram_read_col()
static int gram_read_extra_here(int nblk, int iread, bool full, int step)
{
    const int ks = tile_stride_blk(nblk);
    std::vector<int> a(64);
    for(int lane = 0; lane < 64; lane++)
    {
        const int row = full ? step + 16*(lane >> 4) : 4*step + (lane >> 4);
        a[lane] = 8*(row*ks + gram_read_col(nblk, iread, lane));
    }
    return read_b64_extra(a);
}

// the fused loop's copy-out of a lane (kernels.hip, copy_out_invariants(): everything optimized, the camera not at the
// reference, or at it): tile byte offsets of its CSR pair in row rsub (A0, A1) and in row rsub + R (B0, B1)
static void copy_out_offsets(bool rowl, int K, int ndist, int ks, bool has_ext, int lane, int* A0, int* A1, int* B0, int* B1, int* rsub_out)
{
    const int PPR = K/2, RPI = 64/PPR, NACT = RPI*PPR;
    const int b1 = 2, b2 = 2 + ndist, b3 = b2 + (has_ext ? 6 : 0), b4 = b3 + 6;
    const int cl = lane < NACT ? lane : lane - NACT, rsub = cl/PPR, c0 = 2*(cl - rsub*PPR);
    auto tcol = [&](int c, int xy)
    {
        if(c < b1) return 2*c + xy;
        if(c < b2) return 4 + (c - b1);
        if(c < b3) return tile_ext0(ndist)   + (c - b2);
        if(c < b4) return tile_frame0(ndist) + (c - b3);
        return tile_warp0(ndist) + (c - b4);
    };
    const int y0 = rsub & 1, y1 = (rsub + RPI) & 1;
    const int ra = rsub + (rowl ? 31*y0 : 0), rb = rsub + RPI + (rowl ? 31*y1 : 0);
    *A0 = 8*(ra*ks + tcol(c0,   y0));
    *A1 = 8*(ra*ks + tcol(c0+1, y0));
    *B0 = 8*(rb*ks + tcol(c0,   y1));
    *B1 = 8*(rb*ks + tcol(c0+1, y1));
    *rsub_out = rsub;
}
// ... and the row group of step S (fused_step()): is there one, which of the lane's two rows, the double step's tile
// rows, the group's first logical row and the end of its block of rows
struct CopyGroup { bool have; int u, go_rows, rb, re; };
static CopyGroup copy_group(bool rowl, int K, int S)
{
    const int R = 64/(K/2), BLKROWS = rowl ? 32 : 64, NGB = (BLKROWS + R - 1)/R, NGRP = (64/BLKROWS)*NGB;
    const int blk = S/NGB, g = S % NGB;
    CHECK(NGRP <= 16 && R >= 4 && 4*NGB <= BLKROWS);
    return CopyGroup{ S < NGRP, g & 1, (g >> 1)*2*R + (rowl ? blk : 0), blk*BLKROWS + g*R, (blk + 1)*BLKROWS };
}

// the extra cycles of one 10x10 OPENCV8 observation by source, printed
static void observation_table(bool rowl, int* gram_full_out)
{
    const int ndist = 8, nblk = tile_nblk(ndist), ks = tile_stride(ndist), K = 2 + ndist + 14, ncorners = 100;
    CHECK(nblk == 7 && ks == 29 && K == 24);
    const int nfull = ncorners/32, nrows_partial = 2*(ncorners % 32), nsteps_partial = (nrows_partial + 3)/4;
    int gram_full = 0, gram_partial = 0, copy_full = 0, copy_partial = 0, writes = 0;
    for(int o = 0; o < gram_nreads(nblk); o++)
        for(int full = 0; full < 2; full++)
            for(int step = 0; step < (full ? 16 : nsteps_partial); step++)
            {
                std::vector<int> a(64);
                for(int lane = 0; lane < 64; lane++)
                    a[lane] = 8*(board_gram_row(rowl, full != 0, step, lane >> 4)*ks + gram_read_col(nblk, o, lane));
                const int e = read_b64_extra(a);
                if(!rowl) CHECK(e == gram_read_extra_cycles(nblk, o, full != 0));
                if(full) gram_full += nfull*e; else gram_partial += e;
            }
    // copy-out (fused_step()): step S reads its row group, if there is one; two reads a lane
    for(int S = 0; S < 16; S++)
    {
        const CopyGroup G = copy_group(rowl, K, S);
        if(!G.have) continue;
        std::vector<int> a0(64), a1(64);
        for(int lane = 0; lane < 64; lane++)
        {
            int A0, A1, B0, B1, rsub;
            copy_out_offsets(rowl, K, ndist, ks, true, lane, &A0, &A1, &B0, &B1, &rsub);
            a0[lane] = 8*G.go_rows*ks + (G.u ? B0 : A0);
            a1[lane] = 8*G.go_rows*ks + (G.u ? B1 : A1);
            // (a lane past the tile's last row reads the pixels staged behind it, as the kernel's does)
        }
        const int e = read_b64_extra(a0) + read_b64_extra(a1);
        copy_full += nfull*e;
        if(4*S < nrows_partial) copy_partial += e;
    }
    // tile writes (board_observation()): one store a column, every half; lane l writes row 2 (l % 32) + l/32, or row l
    for(int c = 0; c < 4*nblk; c++)
    {
        std::vector<int> a(64);
        for(int lane = 0; lane < 64; lane++) a[lane] = 8*((rowl ? lane : 2*(lane & 31) + (lane >> 5))*ks + c);
        writes += (nfull + (nrows_partial > 0))*write_b64_extra(a);
    }
    printf("10x10 OPENCV8 observation, %s, extra LDS cycles by source:\n", rowl ? "one tile row a lane (everything optimized)" : "the rows in order (the general kernels)");
    printf("  Gram reads, full halves    %4d\n", gram_full);
    printf("  Gram reads, partial half   %4d\n", gram_partial);
    printf("  copy-out reads             %4d  (%d a full half, %d in the partial one)\n", copy_full + copy_partial, copy_full/nfull, copy_partial);
    printf("  tile writes                %4d\n", writes);
    printf("  sum                        %4d\n", gram_full + gram_partial + copy_full + copy_partial + writes);
    *gram_full_out = gram_full;
}

// ---- one tile row a lane
static void check_row_a_lane()
{
    // who writes what: lane l holds, after the exchange of the halves, the x row (l < 32) or the y row of the corner
    // that in-half lane l % 32 computed, and writes tile row l
    int seen[64] = {0};
    for(int lane = 0; lane < 64; lane++)
    {
        for(int h = 0; h < 2; h++) CHECK((board_lane_corner((lane & 31) + 32*h) >> 5) == h);     // a lane stays in its half
        const int r = 2*(board_lane_corner(lane & 31) & 31) + (lane >> 5);
        CHECK(board_tile_row(true, r) == lane && board_tile_row(false, r) == r);
        seen[board_tile_row(true, r)]++;
    }
    for(int row = 0; row < 64; row++) CHECK(seen[row] == 1);
    for(int nblk = 5; nblk <= 8; nblk++)
        for(int c = 0; c < 4*nblk; c++)
        {
            std::vector<int> a(64);
            for(int lane = 0; lane < 64; lane++) a[lane] = 8*(lane*tile_stride_blk(nblk) + c);
            CHECK(write_b64_extra(a) == 0);
        }

    // what a k-step reads, on an integer tile: L the half's logical rows, T the tile
    const int ncols = 28;
    std::vector<int> L(64*ncols), T(64*ncols);
    for(int rowl = 0; rowl < 2; rowl++)
        for(int nc = 1; nc <= 32; nc++)
        {
            const int nrows = 2*nc;
            for(int r = 0; r < 64; r++)
                for(int c = 0; c < ncols; c++)
                {
                    L[r*ncols + c] = r < nrows ? 1 + rand() % 1000 : 0;
                    T[board_tile_row(rowl != 0, r)*ncols + c] = L[r*ncols + c];
                }
            const bool full = nrows == 64;
            for(int s = 0; 4*s < nrows; s++)
                for(int k = 0; k < 4; k++)
                {
                    const int logical = full ? s + 16*k : 4*s + k;          // the rows-in-order layout's row: its own number
                    const int row = board_gram_row(rowl != 0, full, 0, k) + board_gram_row(rowl != 0, full, s, 0);    // the kernel's sum
                    CHECK(row == board_gram_row(rowl != 0, full, s, k) && row >= 0 && row < 64);
                    for(int c = 0; c < ncols; c++) CHECK(T[row*ncols + c] == L[logical*ncols + c]);
                }
        }

    // the copy-out: every stored row from the tile row that holds it, the 64 rows once each
    for(int rowl = 0; rowl < 2; rowl++)
        for(int ndist = 0; ndist <= 12; ndist += 4)        // the lens models with an even row length: 0, 4, 8, 12 distortions
            for(int ext = 0; ext < 2; ext++)
            {
                const int K = 2 + ndist + 8 + 6*ext, ks = tile_stride(ndist), R = 64/(K/2);
                std::vector<int> stored(64*K, 0);
                for(int S = 0; S < 16; S++)
                {
                    const CopyGroup G = copy_group(rowl != 0, K, S);
                    if(!G.have) continue;
                    CHECK(G.rb >= 4*S);         // a partial half that stops before step S has no row of this group
                    for(int lane = 0; lane < 64; lane++)
                    {
                        int A0, A1, B0, B1, rsub;
                        copy_out_offsets(rowl != 0, K, ndist, ks, ext != 0, lane, &A0, &A1, &B0, &B1, &rsub);
                        const int a[2] = { 8*G.go_rows*ks + (G.u ? B0 : A0), 8*G.go_rows*ks + (G.u ? B1 : A1) };
                        // inside the LDS of a board of one corner: the tile, 64 pixels' worth, the joint record, 4.
                        // (Lanes whose store is predicated off read past the tile. The rows in order reach 8 rows
                        //  past it at 10 nonzeros a row, more than this bound; one row a lane at most 4)
                        for(int i = 0; i < 2; i++) CHECK(a[i] >= 0 && (!rowl || a[i]/8 < 64*ks + 64 + JOINT_REC + 4));
                        const int r = G.rb + rsub;
                        if(!(G.rb + R - 1 < G.re || rsub < G.re - G.rb)) continue;       // the store's predicate
                        const int cl = lane < R*(K/2) ? lane : lane - R*(K/2), c0 = 2*(cl - rsub*(K/2));
                        for(int i = 0; i < 2; i++)
                        {
                            CHECK(a[i]/8/ks == board_tile_row(rowl != 0, r) && a[i]/8 % ks < 4*tile_nblk(ndist));
                            if(lane == cl) stored[r*K + c0 + i]++;
                        }
                    }
                }
                for(int e = 0; e < 64*K; e++) CHECK(stored[e] == 1);
            }
}

int main()
{
    // ---- 6 and 7 blocks: no operand read of a full half conflicts; the function against the count made here
    for(int nblk = 5; nblk <= 8; nblk++)
        for(int o = 0; o < gram_nreads(nblk); o++)
            for(int full = 0; full < 2; full++)
            {
                const int e = gram_read_extra_cycles(nblk, o, full != 0);
                for(int step = 0; step < (full ? 16 : 2); step++) CHECK(e == gram_read_extra_here(nblk, o, full != 0, step));
                if(full && (nblk == 6 || nblk == 7)) CHECK(e == 0);
                printf("blocks %d read %d %s half: %d extra cycles\n", nblk, o, full ? "full   " : "partial", e);
            }

    check_row_a_lane();
    int gram_full[2];
    for(int rowl = 0; rowl < 2; rowl++) observation_table(rowl != 0, &gram_full[rowl]);
    CHECK(gram_full[0] == 0 && gram_full[1] == 0);
    printf("ok\n");
    return 0;
}
