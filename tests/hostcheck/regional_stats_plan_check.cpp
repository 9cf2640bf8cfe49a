// Drives csrc/regional_stats_plan.hpp as a stand-alone program (built with ASan + UBSan by
// tests/hostbuild.py, a row of its PROGRAMS). Prints "ok" and returns 0 if every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "../../mrcal_amd/csrc/regional_stats_plan.hpp"

using namespace mrcal_amd;

static int failures = 0;
#define CHECK(c) do { if(!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while(0)

// one board of n corners, one camera 4000x2200, a 30x20 grid
static RegionalStatsPlan with_corners(int64_t n)
{
    RegionalStatsPlan p;
    std::string err;
    const int size[2] = { 4000, 2200 };
    CHECK(plan_regional_stats(&p, 1, size, 1, (int)n, 30, 20, &err));
    return p;
}

int main()
{
    std::string err;
    // 1 corner; one less than, exactly, one more than a chunk
    {
        RegionalStatsPlan p = with_corners(1);
        CHECK(p.Ncorners == 1 && p.Nchunks == 1 && p.Nentries_max == RS_SLOTS && p.Ncells == 600 && p.hist_ints == 600);
        CHECK(p.scan_items_per_thread == 1);
        p = with_corners(RS_CHUNK - 1); CHECK(p.Nchunks == 1 && p.hist_ints == 600);
        p = with_corners(RS_CHUNK);     CHECK(p.Nchunks == 1);
        p = with_corners(RS_CHUNK + 1); CHECK(p.Nchunks == 2 && p.hist_ints == 1200 && p.Nentries_max == (int64_t)RS_SLOTS*(RS_CHUNK + 1));
    }
    // the benchmark: 8 cameras x 1000 frames x 100 corners, 600 cells a camera
    {
        RegionalStatsPlan p;
        int sizes[16];
        for(int c = 0; c < 8; c++) { sizes[2*c] = 4000; sizes[2*c + 1] = 2200; }
        CHECK(plan_regional_stats(&p, 8, sizes, 8000, 100, 30, 20, &err));
        CHECK(p.Ncorners == 800000 && p.Ncells == 4800 && p.Nchunks == 391 && p.hist_ints == (int64_t)391*4800);
        CHECK(p.Nentries_max == 3200000 && p.scan_items_per_thread == 5);
        CHECK(p.scan_items_per_thread*RS_SCAN_THREADS >= p.Ncells);
        CHECK(p.cameras.size() == 8 && p.centres.size() == 8*50);
        for(int c = 0; c < 8; c++)
        {
            const RegionalCamera& cam = p.cameras[c];
            CHECK(cam.cell0 == 600*c && cam.centre0 == 50*c && cam.gridn_width == 30 && cam.gridn_height == 20);
            CHECK(p.centres[cam.centre0] == 0.0 && p.centres[cam.centre0 + 29] == 3999.0 && p.centres[cam.centre0 + 30 + 19] == 2199.0);
            CHECK(cam.half_w == 3999.0/29.0/2.0 && cam.half_h == 2199.0/19.0/2.0);
        }
        // gridn_height None, per camera by its own imager, halves to even
        sizes[2] = 1000; sizes[3] = 1000;            // square: 30
        sizes[4] = 4000; sizes[5] = 2200;            // 16.5 -> 16
        sizes[6] = 4000; sizes[7] = 2334;            // 17.505 -> 18
        CHECK(plan_regional_stats(&p, 8, sizes, 8000, 100, 30, -1, &err));
        CHECK(p.cameras[0].gridn_height == 16 && p.cameras[1].gridn_height == 30 && p.cameras[2].gridn_height == 16 && p.cameras[3].gridn_height == 18);
        CHECK(p.cameras[2].cell0 == 30*16 + 30*30);
        CHECK((double)2200/4000*30 == 16.5);
    }
    // the centre formula is np.linspace's: i*step, and the end exactly
    CHECK(regional_cell_centre(0, 3, 10) == 0.0 && regional_cell_centre(1, 3, 10) == 4.5 && regional_cell_centre(2, 3, 10) == 9.0);
    CHECK(regional_cell_centre(7, 30, 4000) == 7.0*(3999.0/29.0));
    // what is int32 stays int32; what does not fit is refused
    {
        RegionalStatsPlan p;
        const int size[2] = { 4000, 2200 };
        const int64_t most = (int64_t)INT32_MAX/RS_SLOTS;
        CHECK(plan_regional_stats(&p, 1, size, most, 1, 2, 2, &err));
        CHECK(p.Nentries_max <= INT32_MAX && p.Nentries_max == most*RS_SLOTS);
        CHECK((int64_t)p.Nchunks*RS_CHUNK >= p.Ncorners && (int64_t)(p.Nchunks - 1)*RS_CHUNK < p.Ncorners);
        CHECK((int64_t)p.Nchunks*RS_CHUNK + RS_CHUNK <= INT32_MAX);      // the kernels' chunk*RS_CHUNK + t
        CHECK(!plan_regional_stats(&p, 1, size, most + 1, 1, 2, 2, &err) && err.find("corners") != std::string::npos);
        CHECK(!plan_regional_stats(&p, 1, size, 10, 100, 1, 2, &err) && err.find("gridn_width must be >= 2") != std::string::npos);
        CHECK(!plan_regional_stats(&p, 1, size, 10, 100, 2, 1, &err) && err.find("gridn_height must be >= 2") != std::string::npos);
        CHECK(!plan_regional_stats(&p, 1, size, 10, 100, 2000, 2000, &err) && err.find("cells") != std::string::npos);
        CHECK(plan_regional_stats(&p, 1, size, 10, 100, 1024, 1024, &err) && p.Ncells == RS_MAX_CELLS && p.scan_items_per_thread == 1024);
        const int wide[2] = { 4000, 100 };           // None: round(0.75) = 1 < 2
        CHECK(!plan_regional_stats(&p, 1, wide, 10, 100, 30, -1, &err));
        CHECK(!plan_regional_stats(&p, 0, size, 10, 100, 30, 20, &err));
    }
    if(failures == 0) printf("ok\n");
    return failures == 0 ? 0 : 1;
}
