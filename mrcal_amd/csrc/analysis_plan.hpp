// What projection_uncertainty.hip and triangulation.hip work out on the host before they touch the device: plain
// structs and vectors in and out, no HIP call. tests/hostcheck/analysis_plan_check.cpp runs them under the host
// sanitizers.
#pragma once
#include <string.h>
#include <vector>
#include "layout.hpp"
#include "lens_dispatch.hpp"

namespace mrcal_amd {

// What the uncertainty's per-point kernel needs to know of G's layout
struct PUArgs
{
    LensConfig cfg;
    int N;
    int k;              // rows / columns of C
    int Nint;           // rows of C that are this camera's optimized intrinsics
    int arg0;           // parametric models: the intrinsics argument of row 0 (4 if the core is not optimized)
    int Nint_entries;   // entries of G in the intrinsics rows: Nint, or for the splined models core + patch
    int Ncore_state;    // splined: 4 if the core is optimized, else 0
    int Npatch;         // splined: 2 (order+1)^2 if the distortions are optimized, else 0
    int Next;           // 6: rrp, and this camera's extrinsics are in the state; else 0
    int rrp;
    int atinfinity;
    int what;
    double sigma;
};

// PUArgs (N, atinfinity, what and sigma are set later) and the k rows of M: a unit row at state col[j] >= 0 times
// scale[j] (this camera's intrinsics, then its extrinsics icam_extrinsics if rrp has them in the state), or row
// -col[j]-1 of K
inline void plan_uncertainty_rows(PUArgs* args, std::vector<int>* col, std::vector<double>* scale,
                                  const Layout& L, int icam_intrinsics, int icam_extrinsics, bool rrp)
{
    memset(args, 0, sizeof(*args));
    PUArgs& a = *args;
    a.rrp = rrp ? 1 : 0;
    a.cfg = lens_config_of(L.lensmodel);
    a.Nint = L.Nintr_state;
    a.arg0 = L.Ncore - L.Ncore_state;
    if(L.lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
    {
        const int n = a.cfg.spline_order + 1;
        a.Ncore_state  = L.Ncore_state;
        a.Npatch       = L.Ndist_state > 0 ? 2*n*n : 0;
        a.Nint_entries = a.Ncore_state + a.Npatch;
    }
    else
        a.Nint_entries = a.Nint;
    a.Next = (rrp && icam_extrinsics >= 0 && L.i_state_extrinsics >= 0) ? 6 : 0;
    a.k = a.Nint + a.Next + 6;

    col->assign((size_t)a.k, 0);
    scale->assign((size_t)a.k, 0.0);
    for(int j = 0; j < a.Nint; j++)
    {
        (*col)[j] = L.i_state_intrinsics + icam_intrinsics*L.Nintr_state + j;
        (*scale)[j] = L.Ncore_state && j < 2 ? SCALE_INTRINSICS_FOCAL_LENGTH :
                      L.Ncore_state && j < 4 ? SCALE_INTRINSICS_CENTER_PIXEL : SCALE_DISTORTION;
    }
    for(int j = 0; j < a.Next; j++)
    {
        (*col)[a.Nint + j] = L.i_state_extrinsics + 6*icam_extrinsics + j;
        (*scale)[a.Nint + j] = j < 3 ? SCALE_ROTATION_CAMERA : SCALE_TRANSLATION_CAMERA;
    }
    for(int j = 0; j < 6; j++) (*col)[a.Nint + a.Next + j] = -j - 1;
}

// The 2N pixels of N pairs grouped by camera: camera c's are rows [off[c], off[c+1]) of qs (.,2), in the order they
// come; rows[i]: where pixel i went. Returns the first pixel whose camera is not in [0, Ncameras) - nothing is
// grouped then - or -1
struct PixelsByCamera
{
    std::vector<int>    off, rows;
    std::vector<double> qs;
};
inline int group_pixels_by_camera(PixelsByCamera* g, int Ncameras, int N, const double* q, const int* icam)
{
    for(int i = 0; i < 2*N; i++)
        if(icam[i] < 0 || icam[i] >= Ncameras) return i;
    std::vector<int> fill((size_t)Ncameras, 0);
    g->off.assign((size_t)Ncameras + 1, 0);
    g->rows.assign((size_t)2*N, 0);
    g->qs.assign((size_t)4*N, 0.0);
    for(int i = 0; i < 2*N; i++) g->off[(size_t)icam[i] + 1]++;
    for(int c = 0; c < Ncameras; c++) g->off[c + 1] += g->off[c];
    for(int i = 0; i < 2*N; i++)
    {
        const int r = g->off[icam[i]] + fill[icam[i]]++;
        g->rows[i] = r;
        g->qs[(size_t)2*r] = q[(size_t)2*i]; g->qs[(size_t)2*r + 1] = q[(size_t)2*i + 1];
    }
    return -1;
}

}
