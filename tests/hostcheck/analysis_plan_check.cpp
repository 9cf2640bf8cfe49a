// TEST-ONLY stand-alone program: the host-only steps of projection_uncertainty.hip and triangulation.hip
// (mrcal_amd/csrc/analysis_plan.hpp) under the host sanitizers: the rows of M for a parametric and a splined model, with
// and without the core and the extrinsics, and the grouping of pixel pairs by camera. Not a product path, and nothing
// loads it into Python.
//
//   built by tests/hostbuild.py, build_program("analysis_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../mrcal_amd/csrc/analysis_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static Layout layout(mrcal_lensmodel_type_t type, bool core, bool distortions, bool extrinsics)
{
    mrcal_lensmodel_t m;
    memset(&m, 0, sizeof(m));
    m.type = type;
    if(type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
    {
        m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.order = 3;
        m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.Nx = 8;
        m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.Ny = 6;
        m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.fov_x_deg = 80;
    }
    mrcal_problem_selections_t sel;
    memset(&sel, 0, sizeof(sel));
    sel.do_optimize_intrinsics_core = core; sel.do_optimize_intrinsics_distortions = distortions;
    sel.do_optimize_extrinsics = extrinsics; sel.do_optimize_frames = true; sel.do_apply_regularization = true;
    // 3 cameras, 2 of them with extrinsics, 8 frames of an 8x7 board seen by each
    return make_layout(make_dims(3, 2, 8, 0, 0, 24, 0, 8, 7), sel, m, NULL, 0);
}

static void check_rows(const Layout& L, int icam, int icam_e, bool rrp)
{
    PUArgs a;
    std::vector<int> col;
    std::vector<double> scale;
    plan_uncertainty_rows(&a, &col, &scale, L, icam, icam_e, rrp);
    const bool ext = rrp && icam_e >= 0 && L.i_state_extrinsics >= 0;
    CHECK(a.Nint == L.Nintr_state && a.Next == (ext ? 6 : 0) && a.k == a.Nint + a.Next + 6 && a.rrp == (rrp ? 1 : 0));
    CHECK((int)col.size() == a.k && (int)scale.size() == a.k);
    for(int j = 0; j < a.k - 6; j++)
    {
        // a unit row: a state of this camera's, times that state's scale
        CHECK(col[j] >= 0 && col[j] < L.Nstate && scale[j] == state_scale(L, col[j]));
        if(j > 0) CHECK(col[j] == col[j-1] + 1 || j == a.Nint);
    }
    if(a.Nint > 0) CHECK(col[0] == L.i_state_intrinsics + icam*L.Nintr_state);
    if(ext)        CHECK(col[a.Nint] == L.i_state_extrinsics + 6*icam_e);
    for(int j = 0; j < 6; j++) CHECK(col[a.k - 6 + j] == -j - 1 && scale[a.k - 6 + j] == 0.0);
    if(L.lensmodel.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
        CHECK(a.Npatch == (L.Ndist_state ? 32 : 0) && a.Nint_entries == L.Ncore_state + a.Npatch && a.cfg.spline_order == 3);
    else
        CHECK(a.Nint_entries == a.Nint && a.arg0 == (L.Ncore_state ? 0 : 4));
}

int main()
{
    for(mrcal_lensmodel_type_t type : { MRCAL_LENSMODEL_PINHOLE, MRCAL_LENSMODEL_OPENCV8, MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC })
        for(int flags = 0; flags < 8; flags++)
        {
            const Layout L = layout(type, flags & 1, flags & 2, flags & 4);
            for(int icam = 0; icam < 3; icam++)
                for(int rrp = 0; rrp < 2; rrp++) check_rows(L, icam, icam - 1, rrp != 0);
        }

    // 5 pairs over 3 cameras, camera 1 unused; then a camera that is not in the table; then no pairs at all
    const double q[20] = { 0,1, 2,3, 4,5, 6,7, 8,9, 10,11, 12,13, 14,15, 16,17, 18,19 };
    int icam[10] = { 2,0, 0,2, 2,2, 0,0, 0,2 };
    PixelsByCamera g;
    CHECK(group_pixels_by_camera(&g, 3, 5, q, icam) == -1);
    CHECK((g.off == std::vector<int>{ 0, 5, 5, 10 }) && g.rows.size() == 10 && g.qs.size() == 20);
    std::vector<int> seen(10, 0);
    for(int i = 0; i < 10; i++)
    {
        const int r = g.rows[i];
        CHECK(r >= g.off[icam[i]] && r < g.off[icam[i] + 1] && !seen[r]++);
        CHECK(g.qs[2*r] == q[2*i] && g.qs[2*r + 1] == q[2*i + 1]);
        // in the order they come
        for(int j = 0; j < i; j++) if(icam[j] == icam[i]) CHECK(g.rows[j] < r);
    }
    icam[7] = 3;
    CHECK(group_pixels_by_camera(&g, 3, 5, q, icam) == 7);
    icam[7] = -1;
    CHECK(group_pixels_by_camera(&g, 3, 5, q, icam) == 7);
    CHECK(group_pixels_by_camera(&g, 3, 0, NULL, NULL) == -1 && g.rows.empty() && g.qs.empty() && g.off.size() == 4);
    printf("ok\n");
    return 0;
}
