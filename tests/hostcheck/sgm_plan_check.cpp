// TEST-ONLY stand-alone program: the host-only planning of stereo_sgm.hip (mrcal_amd/csrc/sgm_plan.hpp) under the host
// sanitizers: every refusal with its message, the offsets of the parts of the pooled allocation (aligned, in order,
// none overlapping the next, the last one ending the pool), the launch geometry at the sizes where a tile, a wavefront
// of 4 paths or a workgroup of 16 pixels is just full or just not, and the refusal of a problem that does not fit
// the free device memory. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("sgm_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../mrcal_amd/csrc/sgm_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const size_t PLENTY = (size_t)1 << 40;

static SgmParams defaults(int dmin, int dmax)
{
    SgmParams p;
    p.disparity_min = dmin; p.disparity_max = dmax; p.P1 = 10; p.P2 = 120; p.paths = 8; p.uniqueness_ratio = 10; p.disp12_max_diff = 1;
    return p;
}

static bool refused(int W, int H, int dtype, const SgmParams& p, const char* words, size_t free_bytes = PLENTY)
{
    SgmPlan plan; std::string why;
    if(sgm_plan(&plan, &why, W, H, dtype, p, free_bytes)) return false;
    if(plan.bytes != 0 || plan.select_grid != 0) return false;          // (a refusal leaves no plan)
    if(why.find("stereo_matching_sgm()") != 0) return false;
    return why.find(words) != std::string::npos;
}

int main()
{
    // the refusals
    {
        CHECK(refused(100, 80, 2, defaults(0, 64), "uint8 or uint16"));
        CHECK(refused(100, 80, -1, defaults(0, 64), "uint8 or uint16"));
        CHECK(refused(0, 80, 0, defaults(0, 64), "images of 0 x 80 pixels cannot be matched"));
        CHECK(refused(100, -1, 0, defaults(0, 64), "cannot be matched"));
        CHECK(refused(1 << 15, 1 << 14, 0, defaults(0, 64), "cannot be matched"));         // 2^29 pixels
        CHECK(refused(100, 80, 0, defaults(0, 0), "positive multiple of 16, at most 256. Got 0"));
        CHECK(refused(100, 80, 0, defaults(5, 0), "positive multiple of 16"));
        CHECK(refused(100, 80, 0, defaults(0, 40), "positive multiple of 16, at most 256. Got 40"));
        CHECK(refused(100, 80, 0, defaults(0, 272), "at most 256. Got 272"));
        CHECK(refused(100, 80, 0, defaults(INT32_MIN, INT32_MAX), "positive multiple of 16"));      // (no overflow on the way)
        SgmParams p = defaults(0, 64);
        p.P1 = -1;            CHECK(refused(100, 80, 0, p, "0 <= P1 <= P2 <= 193. Got P1 = -1, P2 = 120"));
        p.P1 = 121;           CHECK(refused(100, 80, 0, p, "0 <= P1 <= P2 <= 193"));
        p.P1 = 10; p.P2 = 194; CHECK(refused(100, 80, 0, p, "0 <= P1 <= P2 <= 193. Got P1 = 10, P2 = 194"));
        p = defaults(0, 64);
        p.paths = 5;          CHECK(refused(100, 80, 0, p, "paths must be 4 or 8. Got 5"));
        p.paths = 0;          CHECK(refused(100, 80, 0, p, "paths must be 4 or 8"));
        p = defaults(0, 64);
        p.uniqueness_ratio = -1;  CHECK(refused(100, 80, 0, p, "uniqueness_ratio must be in 0..99. Got -1"));
        p.uniqueness_ratio = 100; CHECK(refused(100, 80, 0, p, "uniqueness_ratio must be in 0..99. Got 100"));
        // the scaled values leave int16: 16 (dmin - 1) >= -32768 and 16 dmax <= 32767
        CHECK(refused(100, 80, 0, defaults(2032, 2048), "leave int16"));
        CHECK(refused(100, 80, 0, defaults(-2048, -2032), "leave int16"));
        // ... and what is just inside them is planned, as are the ends of every other range
        SgmPlan plan; std::string why;
        CHECK(sgm_plan(&plan, &why, 100, 80, 0, defaults(2031, 2047), PLENTY));
        CHECK(sgm_plan(&plan, &why, 100, 80, 0, defaults(-2047, -2031), PLENTY));
        p = defaults(-20, 236); p.P1 = 0; p.P2 = 0; p.paths = 4; p.uniqueness_ratio = 0; p.disp12_max_diff = -1;
        CHECK(sgm_plan(&plan, &why, 100, 80, 1, p, PLENTY) && plan.D == 256 && plan.per_lane == 16);
        p.P1 = 193; p.P2 = 193; p.uniqueness_ratio = 99;
        CHECK(sgm_plan(&plan, &why, 1, 1, 0, p, PLENTY));
    }
    // the pool and the grids, at the sizes where a tile, a wavefront or a workgroup is just full or just not
    const int sizes[][2] = { { 9, 7 }, { 63, 8 }, { 64, 9 }, { 65, 10 }, { 17, 64 }, { 130, 65 }, { 131, 130 }, { 1, 1 }, { 4, 4 },
                             { 16, 1 }, { 17, 1 }, { 1024, 768 }, { 6016, 4016 } };       // (W,H)
    const int Ds[] = { 16, 48, 64, 80, 128, 256 };
    for(const auto& size : sizes)
        for(int D : Ds)
            for(int dtype = 0; dtype < 2; dtype++)
            {
                const int W = size[0], H = size[1];
                SgmPlan plan; std::string why;
                CHECK(sgm_plan(&plan, &why, W, H, dtype, defaults(-20, -20 + D), PLENTY));
                CHECK(plan.W == W && plan.H == H && plan.D == D && plan.dtype == dtype && plan.per_lane*SGM_LANES == D);
                const size_t N = (size_t)W*H;
                // the parts in order, what each needs
                const size_t at[]   = { plan.image[0], plan.image[1], plan.census[0], plan.census[1], plan.S,
                                        plan.index_left, plan.index_right, plan.disparity, plan.bytes };
                const size_t need[] = { N*sgm_pixel_bytes(dtype), N*sgm_pixel_bytes(dtype), N*8, N*8, N*D*2, N, N, N*2 };
                CHECK(at[0] == 0);
                for(int i = 0; i < 8; i++)
                {
                    CHECK(at[i] % SGM_ALIGN == 0);
                    CHECK(at[i] + need[i] <= at[i+1] && at[i+1] - at[i] < need[i] + SGM_ALIGN);
                }
                // every pixel, row and column is covered, and no workgroup is idle
                CHECK((size_t)plan.census_grid[0]*SGM_CENSUS_TILE_X >= (size_t)W && (size_t)(plan.census_grid[0] - 1)*SGM_CENSUS_TILE_X < (size_t)W);
                CHECK((size_t)plan.census_grid[1]*SGM_CENSUS_TILE_Y >= (size_t)H && (size_t)(plan.census_grid[1] - 1)*SGM_CENSUS_TILE_Y < (size_t)H);
                CHECK((size_t)plan.path_grid_horizontal*SGM_WAVE_PATHS >= (size_t)H && (size_t)(plan.path_grid_horizontal - 1)*SGM_WAVE_PATHS < (size_t)H);
                CHECK((size_t)plan.path_grid_vertical*SGM_WAVE_PATHS >= (size_t)W && (size_t)(plan.path_grid_vertical - 1)*SGM_WAVE_PATHS < (size_t)W);
                CHECK((size_t)plan.select_grid*SGM_SELECT_PIXELS >= N && (size_t)(plan.select_grid - 1)*SGM_SELECT_PIXELS < N);
                CHECK((size_t)plan.check_grid*SGM_CHECK_THREADS >= N && (size_t)(plan.check_grid - 1)*SGM_CHECK_THREADS < N);
                // what does not fit is refused with its size; what just fits is not
                CHECK(sgm_plan(&plan, &why, W, H, dtype, defaults(-20, -20 + D), at[8]));
                char size_words[64];
                snprintf(size_words, sizeof(size_words), "need %zu bytes of device memory; %zu are free", at[8], at[8] - 1);
                CHECK(refused(W, H, dtype, defaults(-20, -20 + D), size_words, at[8] - 1));
            }
    // the real calibration's size with 128 disparities: S alone is 2 W H D bytes
    {
        SgmPlan plan; std::string why;
        CHECK(sgm_plan(&plan, &why, 6016, 4016, 0, defaults(0, 128), PLENTY));
        CHECK(plan.disparity - plan.S >= (size_t)2*6016*4016*128 && plan.bytes > ((size_t)6 << 30) && plan.bytes < ((size_t)7 << 30));
        CHECK(refused(6016, 4016, 0, defaults(0, 128), "6016 x 4016 pixels with 128 disparities need", (size_t)4 << 30));
        CHECK(refused(6016, 4016, 0, defaults(0, 128), "are free", 0));
    }
    printf("ok\n");
    return 0;
}
