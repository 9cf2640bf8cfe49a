// TEST-ONLY stand-alone program: the host-only planning of lensfit.hip (mrcal_amd/csrc/lensfit_plan.hpp) under the host
// sanitizers: every row of for_parametric_lens() with and without the core and with and without the pose - the
// instantiation, the unknowns of each stage, the sums, threads, the chunk of rows, LDS within the limit - the
// regularization scales, the measurement counts, and every refusal. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("lensfit_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "../../mrcal_amd/csrc/lensfit_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static mrcal_lensmodel_t model(int type)
{
    mrcal_lensmodel_t m;
    memset(&m, 0, sizeof(m));
    m.type = (mrcal_lensmodel_type_t)type;
    return m;
}

int main()
{
    const int size[2] = { 4000, 2200 };
    struct Row { int type, proj, ndist; };
    const Row rows[] = { { MRCAL_LENSMODEL_PINHOLE, PROJ_OPENCV, 0 }, { MRCAL_LENSMODEL_STEREOGRAPHIC, PROJ_STEREOGRAPHIC, 0 },
                         { MRCAL_LENSMODEL_LONLAT, PROJ_LONLAT, 0 }, { MRCAL_LENSMODEL_LATLON, PROJ_LATLON, 0 },
                         { MRCAL_LENSMODEL_OPENCV4, PROJ_OPENCV, 4 }, { MRCAL_LENSMODEL_OPENCV5, PROJ_OPENCV, 5 },
                         { MRCAL_LENSMODEL_OPENCV8, PROJ_OPENCV, 8 }, { MRCAL_LENSMODEL_OPENCV12, PROJ_OPENCV, 12 },
                         { MRCAL_LENSMODEL_CAHVOR, PROJ_CAHVOR, 5 }, { MRCAL_LENSMODEL_CAHVORE, PROJ_CAHVORE, 8 } };
    int Nrows = 0, NPlargest = 0;
    for(const Row& r : rows)
    {
        // (the table itself says the same: this list has not drifted from it)
        int proj = -1, ndist = -1;
        CHECK(for_parametric_lens(r.type, [&](auto k) { proj = decltype(k)::PROJ; ndist = decltype(k)::NDIST; }));
        CHECK(proj == r.proj && ndist == r.ndist);
        Nrows++;
        for(int core = 0; core < 2; core++)
            for(int pose = 0; pose < 2; pose++)
                for(int reg = 0; reg < 2; reg++)
                {
                    LensfitPlan plan; std::string why;
                    const int N = 600;
                    const bool ok = lensfit_plan(&plan, &why, model(r.type), N, 3, size, core, pose, reg);
                    const int NI = 4 + r.ndist, NP1 = NI - (core ? 0 : 4), NP = NP1 + (pose ? 6 : 0);
                    if(NP == 0)
                    {
                        CHECK(!ok && why.find("nothing to fit") != std::string::npos && plan.threads == 0);
                        continue;
                    }
                    CHECK(ok);
                    CHECK(plan.proj == r.proj && plan.ndist == r.ndist && plan.Nintrinsics == NI && plan.ivar0 == (core ? 0 : 4));
                    CHECK(plan.Nstages == (pose ? 2 : 1) && plan.NP[0] == NP1 && plan.NP[1] == (pose ? NP : 0));
                    CHECK(NP >= 1 && NP <= LENSFIT_NP_MAX);
                    if(NP > NPlargest) NPlargest = NP;
                    CHECK(plan.NE == NP + NP*(NP + 1)/2 + 1 && plan.NE == lensfit_num_sums(NP));
                    // a thread an entry, whole waves, and a lane for each point of a chunk
                    CHECK(plan.threads % 64 == 0 && plan.threads >= plan.NE && plan.threads <= 320 && 2*plan.threads >= plan.chunk_rows);
                    CHECK(plan.row_doubles == NP + 1);
                    CHECK(plan.chunk_rows % 64 == 0 && plan.chunk_rows >= 64 && plan.chunk_rows <= LENSFIT_CHUNK_ROWS_MAX);
                    CHECK(plan.rows_lds_bytes == (size_t)plan.chunk_rows*(NP + 1)*8);
                    CHECK(plan.lds_bytes == plan.rows_lds_bytes + LENSFIT_STATE_LDS_BYTES && plan.lds_bytes <= LENSFIT_LDS_BYTES);
                    // the largest chunk that fits, up to the cap
                    CHECK(plan.chunk_rows == LENSFIT_CHUNK_ROWS_MAX ||
                          (size_t)(plan.chunk_rows + 64)*(NP + 1)*8 + LENSFIT_STATE_LDS_BYTES > LENSFIT_LDS_BYTES);
                    CHECK(plan.Nreg_distortion == (reg ? r.ndist : 0) && plan.Nreg_centerpixel == (reg && core ? 2 : 0));
                    CHECK(plan.Nmeasurements == 2*N + plan.Nreg_distortion + plan.Nreg_centerpixel);
                }
    }
    CHECK(Nrows == 10 && NPlargest == LENSFIT_NP_MAX);
    // 22 unknowns: 276 sums, five waves, 256 rows of 23 doubles
    {
        LensfitPlan plan; std::string why;
        CHECK(lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV12), 100, 1, size, true, true, true));
        CHECK(plan.NE == 276 && plan.threads == 320 && plan.row_doubles == 23 && plan.chunk_rows == 256 && plan.lds_bytes == 256*23*8 + 12288);
        CHECK(lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_PINHOLE), 100, 1, size, true, false, true));
        CHECK(plan.NE == 15 && plan.threads == 256 && plan.chunk_rows == 512);
    }
    // the regularization scales: mrcal.c:5787-5850, 5859
    {
        for(int j = 0; j < 12; j++)
        {
            CHECK(lensfit_distortion_scale(MRCAL_LENSMODEL_OPENCV8,  j) == ((j >= 5 && j <= 7) ? 0.5 : 0.1));
            CHECK(lensfit_distortion_scale(MRCAL_LENSMODEL_OPENCV12, j) == ((j >= 5 && j <= 7) ? 0.5 : 0.1));
            CHECK(lensfit_distortion_scale(MRCAL_LENSMODEL_OPENCV5,  j) == 0.1);
            CHECK(lensfit_distortion_scale(MRCAL_LENSMODEL_CAHVORE,  j) == 0.1);
        }
        CHECK(lensfit_centerpixel_scale(size) == 0.1/(4000.*0.1));
    }
    // the refusals
    {
        LensfitPlan plan; std::string why;
        mrcal_lensmodel_t splined = model(MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC);
        splined.LENSMODEL_SPLINED_STEREOGRAPHIC__config.order = 3;
        splined.LENSMODEL_SPLINED_STEREOGRAPHIC__config.Nx = 8;
        splined.LENSMODEL_SPLINED_STEREOGRAPHIC__config.Ny = 6;
        splined.LENSMODEL_SPLINED_STEREOGRAPHIC__config.fov_x_deg = 80;
        CHECK(!lensfit_plan(&plan, &why, splined, 100, 1, size, true, false, true) && why.find("splined") != std::string::npos);
        // (values the enumeration's type can hold: one of its own "invalid" marks, and one past the splined model)
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_INVALID), 100, 1, size, true, false, true) && why.find("not supported") != std::string::npos);
        CHECK(!lensfit_plan(&plan, &why, model(15), 100, 1, size, true, false, true) && why.find("not supported") != std::string::npos);
        // fewer pixel rows than unknowns: 16 unknowns need 8 points, 22 need 11
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV12), 7, 1, size, true, false, true) && why.find("fewer than the 16 unknowns") != std::string::npos);
        CHECK( lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV12), 8, 1, size, true, false, true));
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV12), 10, 1, size, true, true, true) && why.find("fewer than the 22 unknowns") != std::string::npos);
        CHECK( lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV12), 11, 1, size, true, true, true));
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_PINHOLE), 100, 1, size, false, false, true) && why.find("nothing to fit") != std::string::npos);
        CHECK( lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_PINHOLE), 100, 1, size, false, true, true) && plan.NP[0] == 0 && plan.NP[1] == 6);
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV4), 0, 1, size, true, false, true) && why.find("points cannot be fitted") != std::string::npos);
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV4), -3, 1, size, true, false, true) && why.find("points cannot be fitted") != std::string::npos);
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV4), LENSFIT_MAX_POINTS + 1, 1, size, true, false, true));
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV4), 100, 0, size, true, false, true) && why.find("trials") != std::string::npos);
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV4), 100, LENSFIT_MAX_TRIALS + 1, size, true, false, true) && why.find("trials") != std::string::npos);
        const int nosize[2] = { 0, 2200 };
        CHECK(!lensfit_plan(&plan, &why, model(MRCAL_LENSMODEL_OPENCV4), 100, 1, nosize, true, false, true) && why.find("imager") != std::string::npos);
        // a refused plan is left empty
        CHECK(plan.threads == 0 && plan.chunk_rows == 0 && plan.lds_bytes == 0);
    }
    printf("ok\n");
    return 0;
}
