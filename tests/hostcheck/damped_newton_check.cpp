// TEST-ONLY stand-alone program: the damped Gauss-Newton step that the in-kernel fits share
// (mrcal_amd/csrc/damped_newton.hpp), built for the host, under the host sanitizers. The solve is held to the backward
// error of a Cholesky solve and the predicted decrease to its rounding, both against sums formed here in long double;
// a variable nothing depends on stays put; what cannot be factored is refused; Damping moves lambda and nu exactly as
// written. Not a product path, and nothing loads it into Python.
//
// Built and run by tests/hostbuild.py, a row of its PROGRAMS: build_program("damped_newton_check"), no arguments
// (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <math.h>
#include <float.h>
#include <vector>
#include "../../mrcal_amd/csrc/damped_newton.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

// a fixed linear-congruential generator: uniform in (-1, 1)
static uint64_t lcg_state;
static double lcg()
{
    lcg_state = lcg_state*6364136223846793005ULL + 1442695040888963407ULL;
    return ((double)(lcg_state >> 12) + 0.5)*ldexp(1.0, -51) - 1.0;
}

struct Problem
{
    int NP;
    std::vector<double> H, g;       // exactly NP(NP+1)/2 and NP long: a read past either end is a sanitizer report
    double  h(int i, int j) const { if(i > j) { int t = i; i = j; j = t; } return H[packed_diagonal(i, NP) + j - i]; }
    double& h(int i, int j)       { if(i > j) { int t = i; i = j; j = t; } return H[packed_diagonal(i, NP) + j - i]; }
};

// H = A^T A, g = A^T x, A of 3 NP rows
static Problem make_problem(int NP, uint64_t seed)
{
    lcg_state = seed;
    const int rows = 3*NP;
    std::vector<double> A(rows*NP), x(rows);
    for(double& v : A) v = lcg();
    for(double& v : x) v = lcg();
    Problem P;
    P.NP = NP;
    P.H.assign(NP*(NP + 1)/2, 0.0);
    P.g.assign(NP, 0.0);
    for(int i = 0; i < NP; i++)
    {
        for(int j = i; j < NP; j++)
            for(int r = 0; r < rows; r++) P.h(i, j) += A[r*NP + i]*A[r*NP + j];
        for(int r = 0; r < rows; r++) P.g[i] += A[r*NP + i]*x[r];
    }
    return P;
}

// damped_step() on scratch that holds NaN wherever the step has no business reading before it writes
template<bool RECIPROCAL_PIVOT, int LD>
static bool step(std::vector<double>& d, double* pred, const Problem& P, double lambda)
{
    CHECK(P.NP <= LD);
    double L[LD][LD];
    for(int i = 0; i < LD; i++) for(int j = 0; j < LD; j++) L[i][j] = NAN;
    d.assign(P.NP, NAN);
    *pred = NAN;
    return damped_step<RECIPROCAL_PIVOT>(L, d.data(), pred, P.H.data(), P.g.data(), P.NP, lambda);
}

template<bool RECIPROCAL_PIVOT, int LD>
static void check_solve(int NP, double lambda, uint64_t seed)
{
    const Problem P = make_problem(NP, seed);
    std::vector<double> d;
    double pred;
    CHECK((step<RECIPROCAL_PIVOT, LD>(d, &pred, P, lambda)));
    // (fmaxl() below passes a NaN over)
    for(int j = 0; j < NP; j++) CHECK(isfinite(d[j]));

    // the backward error of the solve: M = H + lambda diag(H), max |M d + g| against 4 NP eps max(|M| |d| + |g|)
    long double worst = 0.0L, scale = 0.0L;
    for(int i = 0; i < NP; i++)
    {
        long double r = (long double)P.g[i], a = fabsl((long double)P.g[i]);
        for(int j = 0; j < NP; j++)
        {
            long double m = (long double)P.h(i, j);
            if(i == j) m += (long double)lambda*m;
            r += m*(long double)d[j];
            a += fabsl(m)*fabsl((long double)d[j]);
        }
        worst = fmaxl(worst, fabsl(r));
        scale = fmaxl(scale, a);
    }
    CHECK(isfinite((double)worst) && worst <= 4.0L*NP*DBL_EPSILON*scale);

    // pred = d^T (lambda diag(H) d - g): three roundings a term, 2 NP additions
    long double exact = 0.0L, terms = 0.0L;
    for(int k = 0; k < NP; k++)
    {
        const long double dk = (long double)d[k], t = (long double)lambda*(long double)P.h(k, k)*dk;
        exact += dk*(t - (long double)P.g[k]);
        terms += fabsl(dk)*(fabsl(t) + fabsl((long double)P.g[k]));
    }
    CHECK(fabsl((long double)pred - exact) <= (2.0L*NP + 3.0L)*DBL_EPSILON*terms);
}

// row and column k of H and g[k] are zero: the step succeeds and leaves d[k] exactly 0
template<bool RECIPROCAL_PIVOT, int LD>
static void check_unused_variable(int NP, double lambda, uint64_t seed)
{
    const int ks[3] = { 0, NP/2, NP - 1 };
    for(int k : ks)
    {
        Problem P = make_problem(NP, seed);
        for(int j = 0; j < NP; j++) P.h(k, j) = 0.0;
        P.g[k] = 0.0;
        std::vector<double> d;
        double pred;
        CHECK((step<RECIPROCAL_PIVOT, LD>(d, &pred, P, lambda)));
        CHECK(d[k] == 0.0);
        for(int j = 0; j < NP; j++) CHECK(isfinite(d[j]));
        CHECK(isfinite(pred));
    }
}

template<bool RECIPROCAL_PIVOT, int LD>
static void check_refusals()
{
    std::vector<double> d;
    double pred;
    const double lambda = 1e-3;
    // a negative diagonal entry: first, middle, last
    for(int k = 0; k < 3; k++)
    {
        Problem P = make_problem(3, 7);
        P.h(k, k) = -1.0;
        CHECK(!(step<RECIPROCAL_PIVOT, LD>(d, &pred, P, lambda)));
    }
    // an indefinite 2x2
    {
        Problem P = make_problem(2, 7);
        P.h(0, 0) = 1.0; P.h(0, 1) = 2.0; P.h(1, 1) = 1.0;
        CHECK(!(step<RECIPROCAL_PIVOT, LD>(d, &pred, P, lambda)));
    }
    // a NaN, an infinity: in every place of H
    const double bad[3] = { NAN, INFINITY, -INFINITY };
    for(double b : bad)
        for(int NP = 1; NP <= 3; NP++)
            for(int e = 0; e < NP*(NP + 1)/2; e++)
            {
                Problem P = make_problem(NP, 7);
                P.H[e] = b;
                CHECK(!(step<RECIPROCAL_PIVOT, LD>(d, &pred, P, lambda)));
            }
}

template<bool RECIPROCAL_PIVOT>
static void check_steps()
{
    const double lambdas[4] = { 1e-15, 1e-3, 1.0, 1e10 };
    const int NPs[6] = { 1, 2, 3, 6, 7, 22 };
    for(uint64_t seed = 1; seed <= 8; seed++)
        for(double lambda : lambdas)
        {
            for(int NP : NPs)
            {
                check_solve<RECIPROCAL_PIVOT, 22>(NP, lambda, seed);
                check_unused_variable<RECIPROCAL_PIVOT, 22>(NP, lambda, seed);
            }
            // (the array exactly as large as the problem, and larger: pd_fit_kernel<6> and <3> in L[6][6])
            for(int NP : { 3, 6 })
            {
                check_solve<RECIPROCAL_PIVOT, 6>(NP, lambda, seed);
                check_unused_variable<RECIPROCAL_PIVOT, 6>(NP, lambda, seed);
            }
        }
    check_refusals<RECIPROCAL_PIVOT, 22>();
    check_refusals<RECIPROCAL_PIVOT, 6>();
}

static void check_damping()
{
    // rejections: lambda doubles, quadruples, ...: powers of two, exact
    int first_beyond = 0;
    for(int k = 1; k <= 9; k++)
    {
        Damping D = { 1e-3, 2.0 };
        for(int i = 0; i < k; i++) D.rejected();
        CHECK(D.lambda == ldexp(1e-3, k*(k + 1)/2));
        CHECK(D.nu == ldexp(1.0, k + 1));
        if(first_beyond == 0 && D.lambda > 1e10) first_beyond = k;
    }
    CHECK(first_beyond == 9);

    const double lambda_min = 1e-15;
    // a step as good as predicted: a third
    {
        Damping D = { 0.25, 64.0 };
        D.accepted(3.0, 3.0, lambda_min);
        CHECK(D.lambda == 0.25*fmax(1.0/3.0, 0.0) && D.nu == 2.0);
    }
    // half as good: lambda stays
    {
        Damping D = { 0.25, 64.0 };
        D.accepted(1.5, 3.0, lambda_min);
        CHECK(D.lambda == 0.25 && D.nu == 2.0);
    }
    // three quarters as good: q = 1/2, and its cube is what counts; no gain at all: q = -1, lambda doubles
    {
        Damping D = { 0.25, 64.0 };
        D.accepted(2.25, 3.0, lambda_min);
        CHECK(D.lambda == 0.25*0.875 && D.nu == 2.0);
        D.accepted(0.0, 3.0, lambda_min);
        CHECK(D.lambda == 0.5*0.875 && D.nu == 2.0);
    }
    // nothing was promised: as gain 1
    for(double pred : { 0.0, -1.0 })
    {
        Damping D = { 0.25, 64.0 };
        D.accepted(5.0, pred, lambda_min);
        CHECK(D.lambda == 0.25*fmax(1.0/3.0, 0.0) && D.nu == 2.0);
    }
    // the clamp
    {
        Damping D = { 2e-15, 64.0 };
        D.accepted(3.0, 3.0, lambda_min);
        CHECK(D.lambda == lambda_min && D.nu == 2.0);
    }
}

int main()
{
    for(int NP = 1; NP <= 22; NP++)
        for(int i = 0, ih = 0; i < NP; i++)
            for(int j = i; j < NP; j++, ih++)
                if(i == j) CHECK(packed_diagonal(i, NP) == ih);
    check_steps<false>();
    check_steps<true>();
    check_damping();
    printf("ok\n");
    return 0;
}
