// TEST-ONLY stand-alone program: the board kernel's Gram packings (mrcal_amd/csrc/problem.hpp, gram_packing()) checked
// on the host, for every number of column blocks a board tile can have (5..8):
//   - the descriptor is well formed: the LDS reads come first, a rotation names an earlier operand, at most 8 reads
//   - every unordered block pair {a,b}, a <= b < NBLK, sits in exactly one valid slot
//   - 7 blocks take ceil(7*8/8) = 7 instructions a k-step, 6 blocks ceil(6*7/8) = 6
//   - the scheme, emulated lane by lane on a random integer-valued tile of 9 rows (a partial last k-step): operands
//     fetched through gram_read_col() and the named rotations, products by the measured lane layout of
//     v_mfma_f64_4x4x4f64 that problem.hpp documents. Every position that gram_pos_to_entry() declares holds
//     (Tt T)[i][j] exactly; every entry of a stored block has exactly one home; an undeclared position is nobody's.
// Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("gram_packing_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../mrcal_amd/csrc/problem.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: NBLK %d: check failed: %s\n", __FILE__, __LINE__, nblk, #cond); exit(1); } } while(0)

static const int NROWS = 9;

// D lane = 16 i + 4 slot + j  +=  sum_k A[16 k + 4 slot + i] B[16 k + 4 slot + j]
static void mfma_f64_4x4x4(double (&d)[64], const double (&a)[64], const double (&b)[64])
{
    for(int i = 0; i < 4; i++)
        for(int s = 0; s < 4; s++)
            for(int j = 0; j < 4; j++)
                for(int k = 0; k < 4; k++)
                    d[16*i + 4*s + j] += a[16*k + 4*s + i]*b[16*k + 4*s + j];
}

static void check(int nblk)
{
    const GramPacking p = gram_packing(nblk);
    const int ncols = 4*nblk, nreads = gram_nreads(nblk), nm = gram_nmfma_blk(nblk);

    // ---- the descriptor itself
    CHECK(p.nop >= 2 && p.nop <= GRAM_MAXOP && p.nmfma >= 1 && p.nmfma <= GRAM_MAXMFMA && nm == p.nmfma);
    CHECK(nreads >= 2 && nreads <= 8);
    for(int o = 0; o < p.nop; o++)
    {
        const GramOperand& op = p.op[o];
        for(int s = 0; s < 4; s++) CHECK(op.blk[s] >= 0 && op.blk[s] < nblk);
        if(o < nreads) CHECK(op.src < 0);
        else
        {
            CHECK(op.src >= 0 && op.src < o && op.rot >= 1 && op.rot <= 3);
            for(int s = 0; s < 4; s++) CHECK(op.blk[s] == p.op[op.src].blk[(s + op.rot) & 3]);
        }
    }
    if(nblk == 7 || nblk == 6) CHECK(nm == (nblk*(nblk+1) + 7)/8);
    for(int ndist = 0; ndist <= 12; ndist++)
        if(tile_nblk(ndist) == nblk) CHECK(gram_stride(ndist) == 64*nm);

    // ---- every unordered block pair in exactly one valid slot
    std::vector<int> pair_count(nblk*nblk, 0);
    for(int m = 0; m < nm; m++)
    {
        CHECK(p.mfma[m].a >= 0 && p.mfma[m].a < p.nop && p.mfma[m].b >= 0 && p.mfma[m].b < p.nop);
        CHECK(p.mfma[m].valid > 0 && p.mfma[m].valid <= 0xf);
        for(int s = 0; s < 4; s++)
            if((p.mfma[m].valid >> s) & 1)
            {
                const int a = p.op[p.mfma[m].a].blk[s], b = p.op[p.mfma[m].b].blk[s];
                pair_count[(a < b ? a : b)*nblk + (a < b ? b : a)]++;
            }
    }
    for(int a = 0; a < nblk; a++)
        for(int b = a; b < nblk; b++) CHECK(pair_count[a*nblk + b] == 1);

    // ---- the scheme on a tile of small integers: every sum is exact
    std::vector<double> T(NROWS*ncols), G(ncols*ncols, 0.0);
    for(size_t i = 0; i < T.size(); i++) T[i] = (double)(rand() % 19 - 9);
    for(int r = 0; r < NROWS; r++)
        for(int i = 0; i < ncols; i++)
            for(int j = 0; j < ncols; j++) G[i*ncols + j] += T[r*ncols + i]*T[r*ncols + j];

    std::vector<double> stored(64*nm, 0.0);
    double (*acc)[64] = reinterpret_cast<double (*)[64]>(stored.data());
    for(int step = 0; 4*step < NROWS; step++)
    {
        double op[GRAM_MAXOP][64];
        for(int o = 0; o < p.nop; o++)
            for(int lane = 0; lane < 64; lane++)
                if(p.op[o].src < 0)
                {
                    // the kernel's read: tile[4 step + lane/16][gram_read_col()]; the rows past the last hold zeros
                    const int row = 4*step + (lane >> 4), col = gram_read_col(nblk, o, lane);
                    CHECK(col >= 0 && col < ncols);
                    CHECK(col == 4*p.op[o].blk[(lane >> 2) & 3] + (lane & 3));
                    op[o][lane] = row < NROWS ? T[row*ncols + col] : 0.0;
                }
                else    // slot s takes the source's slot s + rot, inside each row of 16 lanes
                    op[o][lane] = op[p.op[o].src][(lane & ~15) | ((lane + 4*p.op[o].rot) & 15)];
        for(int m = 0; m < nm; m++) mfma_f64_4x4x4(acc[m], op[p.mfma[m].a], op[p.mfma[m].b]);
    }

    std::vector<int> homes(ncols*ncols, 0);
    int ndeclared = 0, nvalid_slots = 0;
    for(int m = 0; m < nm; m++)
        for(int s = 0; s < 4; s++) nvalid_slots += (p.mfma[m].valid >> s) & 1;
    for(int pos = 0; pos < 64*nm; pos++)
    {
        int i = -7, j = -7; bool diag = false;
        if(!gram_pos_to_entry(nblk, pos, &i, &j, &diag))
        {
            CHECK(i == -7 && j == -7 && !diag);         // nobody's: nothing is said about it
            continue;
        }
        ndeclared++;
        CHECK(i >= 0 && i < ncols && j >= 0 && j < ncols && diag == (i/4 == j/4));
        CHECK(stored[pos] == G[i*ncols + j]);
        homes[i*ncols + j]++;
    }
    CHECK(ndeclared == 16*nvalid_slots && nvalid_slots == nblk*(nblk+1)/2);
    // a diagonal block stores (i,j) and (j,i) both, any other pair of blocks one of the two
    for(int i = 0; i < ncols; i++)
        for(int j = 0; j < ncols; j++)
            if(i/4 == j/4) CHECK(homes[i*ncols + j] == 1);
            else           CHECK(homes[i*ncols + j] + homes[j*ncols + i] == 1);
    int i, j; bool diag;
    CHECK(!gram_pos_to_entry(nblk, 64*nm, &i, &j, &diag));      // past the last accumulator
}

int main()
{
    srand(12345);
    for(int nblk = 5; nblk <= 8; nblk++) check(nblk);
    printf("ok\n");
    return 0;
}
