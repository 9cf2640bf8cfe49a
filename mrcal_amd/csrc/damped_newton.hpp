// One damped Gauss-Newton step, as thread 0 of an in-kernel fit takes it (pd_fit_kernel of projection_diff.hip,
// lensfit_kernel of lensfit.hip): the damped normal equations solved by Cholesky, the decrease they promise, and
// Nielsen's rule for the damping. Plain arithmetic for host and device, no HIP call and no lane operation:
// tests/hostcheck/damped_newton_check.cpp runs it under the host sanitizers.
//
// What is a fit's own stays with the fit: its constants and status codes, when a trial is kept, when the fit ends, its
// regularization rows, how the next trial point is formed from d, the scale of its cost (F = x.x or 1/2 of it) and
// which quantity it tests for finiteness.
#pragma once
#include <math.h>
#include "device_math.hpp"

namespace mrcal_amd {

// where H[c][c] is in the upper triangle of an NP x NP matrix packed row by row
MRCAL_AMD_HD int packed_diagonal(int c, int NP) { return c*NP - c*(c - 1)/2; }

struct Damping
{
    double lambda, nu;

    // Nielsen's update from the gain ratio of a step that was kept (dF: what it gained, pred: what damped_step()
    // promised, in the same units): lambda falls to a third after a step as good as predicted, and hardly at all
    // after one that barely paid. (Dividing and multiplying by 10 had the implied-transformation fit reject every
    // other trial in the flat valley of the Huber weights: 400 evaluations were not enough there)
    MRCAL_AMD_HD void accepted(double dF, double pred, double lambda_min)
    {
        const double gain = pred > 0.0 ? dF/pred : 1.0, q = 2.0*gain - 1.0;
        lambda = fmax(lambda*fmax(1.0/3.0, 1.0 - q*q*q), lambda_min);
        nu = 2.0;
    }
    // after a trial that was not kept, or a matrix that could not be factored: lambda doubles, quadruples, ...
    MRCAL_AMD_HD void rejected() { lambda *= nu; nu *= 2.0; }
};

// (H + lambda diag(H)) d = -g by L L^T, for the upper triangle of H packed row by row; a variable nothing depends on
// (H[c][c] == 0) stays put. Leaves d and pred = d^T (lambda diag(H) d - g), the decrease of x.x that the quadratic
// model promises; L [NP][NP] of an array [.][LD] is scratch. false: a pivot was not positive and finite, and d and
// pred say nothing.
// RECIPROCAL_PIVOT: a column of L is multiplied by 1/L[j][j] (the lens-model fit) or divided by L[j][j] (the
// implied transformation). The difference is inherited from the two fits this was taken out of, not designed: each
// keeps the roundings it had.
template<bool RECIPROCAL_PIVOT, int LD>
MRCAL_AMD_HD bool damped_step(double (*L)[LD], double* d, double* pred, const double* H, const double* g, int NP, double lambda)
{
    int ih = 0;
    for(int i = 0; i < NP; i++)
        for(int j = i; j < NP; j++, ih++)
            L[j][i] = (i == j) ? (H[ih] == 0.0 ? 1.0 : H[ih]*(1.0 + lambda)) : H[ih];
    for(int j = 0; j < NP; j++)
    {
        double s = L[j][j];
        for(int k = 0; k < j; k++) s -= L[j][k]*L[j][k];
        if(!(s > 0.0) || !isfinite(s)) return false;
        const double ljj = sqrt(s), iljj = 1.0/ljj;
        L[j][j] = ljj;
        for(int i = j + 1; i < NP; i++)
        {
            double v = L[i][j];
            for(int k = 0; k < j; k++) v -= L[i][k]*L[j][k];
            L[i][j] = RECIPROCAL_PIVOT ? v*iljj : v/ljj;
        }
    }
    for(int i = 0; i < NP; i++)
    {
        double v = -g[i];
        for(int k = 0; k < i; k++) v -= L[i][k]*d[k];
        d[i] = v/L[i][i];
    }
    for(int i = NP - 1; i >= 0; i--)
    {
        double v = d[i];
        for(int k = i + 1; k < NP; k++) v -= L[k][i]*d[k];
        d[i] = v/L[i][i];
    }
    double p = 0.0;
    for(int k = 0; k < NP; k++) p += d[k]*(lambda*H[packed_diagonal(k, NP)]*d[k] - g[k]);
    *pred = p;
    return true;
}

} // namespace mrcal_amd
