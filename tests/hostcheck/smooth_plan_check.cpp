// TEST-ONLY stand-alone program: the host-only planning of smooth.hip (mrcal_amd/csrc/smooth_plan.hpp) under the host
// sanitizers: the integer taps over a sweep of sigma (their sum, their symmetry, their range, their distance from the
// Gaussian they round), every refusal with its message, the tile with its halo and the LDS it needs, the grid, the
// offsets of the parts of the pooled allocation, and the refusal of an image that does not fit the free device memory.
// Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("smooth_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "../../mrcal_amd/csrc/smooth_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const size_t PLENTY = (size_t)1 << 40;

static SmoothParams params(double sigma_x, double sigma_y)
{
    SmoothParams p;
    p.sigma_x = sigma_x; p.sigma_y = sigma_y;
    return p;
}

static bool refused(int W, int H, int dtype, const SmoothParams& p, const char* words, size_t free_bytes = PLENTY)
{
    SmoothPlan plan; std::string why;
    if(smooth_plan(&plan, &why, W, H, dtype, p, free_bytes)) return false;
    if(plan.bytes != 0 || plan.grid != 0 || plan.lds_bytes != 0) return false;      // (a refusal leaves no plan)
    return why.find("smooth():") == 0 && why.find(words) != std::string::npos;
}

int main()
{
    // the taps: sigma = 0.50 .. 8.00 in steps of 0.01
    {
        int largest_centre = 0;
        for(int i = 50; i <= 800; i++)
        {
            const double sigma = (double)i/100.0;
            int R = -1, w[SMOOTH_R_MAX + 1];
            CHECK(smooth_weights(&R, w, sigma));
            CHECK(R == (int)ceil(3.0*sigma) && R >= 2 && R <= SMOOTH_R_MAX);
            int sum = 0;
            for(int k = -R; k <= R; k++)
            {
                sum += smooth_tap(w, R, k);
                CHECK(smooth_tap(w, R, k) == smooth_tap(w, R, -k));
            }
            CHECK(sum == 256);
            CHECK(smooth_tap(w, R, R + 1) == 0 && smooth_tap(w, R, -R - 1) == 0);
            double S = 0.0;
            for(int k = -R; k <= R; k++) S += exp(-(double)(k*k)/(2.0*sigma*sigma));
            for(int k = 0; k <= R; k++)
            {
                CHECK(0 <= w[k] && w[k] <= 255);
                const double a = 256.0*exp(-(double)(k*k)/(2.0*sigma*sigma))/S;
                CHECK(fabs((double)w[k] - a) <= 1.0);
            }
            if(w[0] > largest_centre) largest_centre = w[0];
        }
        CHECK(largest_centre == 202);           // (at sigma = 0.5)
        int R = -1, w[SMOOTH_R_MAX + 1];
        CHECK(smooth_weights(&R, w, 0.0) && R == 0 && w[0] == 256);
        CHECK(smooth_weights(&R, w, 0.5) && R == 2 && w[0] == 202);
        CHECK(!smooth_weights(&R, w, -1.0) && !smooth_weights(&R, w, NAN) && !smooth_weights(&R, w, 8.01) && !smooth_weights(&R, w, INFINITY));
    }
    // the refusals
    {
        const SmoothParams two = params(2.0, 2.0);
        CHECK(refused(100, 80, 0, params(0.49, 2.0), "a sigma is 0 (that axis is not filtered) or lies in [0.5, 8]. Got (0.49,2)"));
        CHECK(refused(100, 80, 0, params(2.0, 8.01), "Got (2,8.01)"));
        CHECK(refused(100, 80, 1, params(-1.0, 2.0), "Got (-1,2)"));
        CHECK(refused(100, 80, 1, params(2.0, NAN), "or lies in [0.5, 8]"));
        CHECK(refused(100, 80, 0, params(INFINITY, 0.0), "or lies in [0.5, 8]"));
        CHECK(refused(100, 80, 0, params(0.0, 0.0), "both sigmas are 0: there is nothing to run"));
        CHECK(refused(0, 80, 0, two, "images of 0 x 80 pixels cannot be smoothed"));
        CHECK(refused(100, 0, 1, two, "images of 100 x 0 pixels cannot be smoothed"));
        CHECK(refused(100, -1, 1, two, "images of 100 x -1 pixels cannot be smoothed"));
        CHECK(refused(1 << 15, (1 << 13) + 1, 0, two, "cannot be smoothed"));              // 2^28 + 2^15 pixels
        CHECK(refused(INT32_MAX, INT32_MAX, 0, two, "cannot be smoothed"));                // (no overflow on the way)
        CHECK(refused(100, 80, 2, two, "images are uint8 or uint16"));
        CHECK(refused(100, 80, -1, two, "images are uint8 or uint16"));
        CHECK(refused(100, 80, 0, two, "100 x 80 pixels need 16384 bytes of device memory; 16383 are free", 16383));
        // ... and what is just inside is not
        SmoothPlan plan; std::string why;
        CHECK(smooth_plan(&plan, &why, 100, 80, 0, two, 16384));
        CHECK(smooth_plan(&plan, &why, 1, 1, 0, params(0.5, 0.0), PLENTY));
        CHECK(smooth_plan(&plan, &why, 1, 1, 1, params(0.0, 8.0), PLENTY));
        CHECK(smooth_plan(&plan, &why, 1 << 15, 1 << 13, 0, two, PLENTY));                  // 2^28 pixels
        CHECK(smooth_plan(&plan, &why, 1, 1 << 28, 1, params(8.0, 8.0), PLENTY) && plan.grid == (1u << 25));
    }
    // the tile, the LDS, the grid and the pool. { W, H }
    const int sizes[][2] = { { 1, 1 }, { 70, 1 }, { 1, 70 }, { 5, 3 }, { 67, 35 }, { 130, 70 }, { 256, 64 }, { 257, 65 }, { 300, 9 },
                             { 722, 482 }, { 6016, 4016 }, { 1 << 14, 1 << 14 } };
    const double sigmas[] = { 0.0, 0.5, 0.87, 1.3, 1.936, 2.0, 3.3, 5.0, 8.0 };
    for(const auto& s : sizes)
        for(int dtype = 0; dtype < 2; dtype++)
            for(const double sigma_x : sigmas)
                for(const double sigma_y : sigmas)
                {
                    if(sigma_x == 0.0 && sigma_y == 0.0) continue;
                    const int W = s[0], H = s[1], pixel = dtype == 0 ? 1 : 2;
                    SmoothPlan q; std::string why;
                    CHECK(smooth_plan(&q, &why, W, H, dtype, params(sigma_x, sigma_y), PLENTY));
                    CHECK(q.dtype == dtype && q.W == W && q.H == H);
                    CHECK(q.Rx == (int)ceil(3.0*sigma_x) && q.Ry == (int)ceil(3.0*sigma_y));
                    // a lane makes 4 pixels, a wavefront reads whole rows of sums side by side
                    CHECK(q.tile_w*2*pixel == SMOOTH_SUM_ROW_BYTES && q.tile_w % SMOOTH_QUAD == 0);
                    CHECK(q.tile_h == 64 || q.tile_h == 32 || q.tile_h == 16 || q.tile_h == 8);
                    CHECK(q.halo_x % SMOOTH_QUAD == 0 && q.halo_x >= q.Rx && q.halo_x < q.Rx + SMOOTH_QUAD);
                    CHECK(q.rows == q.tile_h + 2*q.Ry);
                    // the staged row: the tile with its halo on both sides, in whole dwords, and the dword that the
                    // window of the last quad reads into: a window is 2 halo_x + 4 pixels long
                    CHECK((q.tile_w + 2*q.halo_x)*pixel % 4 == 0 && q.raw_dwords == (q.tile_w + 2*q.halo_x)*pixel/4 + 1);
                    const int last_quad_pixel = q.tile_w - SMOOTH_QUAD;
                    CHECK((last_quad_pixel + 2*q.halo_x + SMOOTH_QUAD)*pixel <= 4*q.raw_dwords);             // multiply-adds
                    if(dtype == 0) CHECK(last_quad_pixel/4 + q.halo_x/2 + 1 <= q.raw_dwords - 1);              // dot4: dwords [quad, quad + groups]
                    CHECK(q.raw_dwords <= SMOOTH_THREADS);
                    // the LDS: the staged rows, then the sums, aligned to 16 bytes
                    CHECK(q.lds_t % 16 == 0 && q.lds_t >= (unsigned)(q.rows*q.raw_dwords*4));
                    CHECK(q.lds_bytes == q.lds_t + (unsigned)q.rows*SMOOTH_SUM_ROW_BYTES);
                    CHECK(q.lds_bytes <= SMOOTH_LDS_MAX && q.lds_bytes <= 160*1024);
                    CHECK(q.lds_bytes <= SMOOTH_LDS_TARGET || q.tile_h == 8);
                    // (twice as high would not have fitted)
                    if(q.tile_h < 64) CHECK((2*q.tile_h + 2*q.Ry)*(q.raw_dwords*4 + SMOOTH_SUM_ROW_BYTES) > SMOOTH_LDS_TARGET - 16);
                    // every pixel is in one tile, and no workgroup is idle
                    CHECK((size_t)q.grid_x*q.tile_w >= (size_t)W && (size_t)(q.grid_x - 1)*q.tile_w < (size_t)W);
                    CHECK((size_t)q.grid_y*q.tile_h >= (size_t)H && (size_t)(q.grid_y - 1)*q.tile_h < (size_t)H);
                    CHECK((size_t)q.grid == (size_t)q.grid_x*q.grid_y && (size_t)q.grid_x*q.grid_y < ((size_t)1 << 31));
                    // the pool: the image, the result, 16-byte aligned and inside
                    const size_t N = (size_t)W*H;
                    CHECK(q.image % 16 == 0 && q.result % 16 == 0 && q.image % SMOOTH_ALIGN == 0 && q.result % SMOOTH_ALIGN == 0);
                    CHECK(q.image + N*pixel <= q.result && q.result + N*pixel <= q.bytes && q.bytes - q.result < N*pixel + SMOOTH_ALIGN);
                    // without the images there is no pool
                    SmoothPlan w;
                    CHECK(smooth_plan(&w, &why, W, H, dtype, params(sigma_x, sigma_y), 0, false));
                    CHECK(w.bytes == 0 && w.grid == q.grid && w.lds_bytes == q.lds_bytes);
                    // what does not fit is refused with its size; what just fits is not
                    CHECK(smooth_plan(&w, &why, W, H, dtype, params(sigma_x, sigma_y), q.bytes));
                    char words[128];
                    snprintf(words, sizeof(words), "%d x %d pixels need %zu bytes of device memory; %zu are free", W, H, q.bytes, q.bytes - 1);
                    CHECK(refused(W, H, dtype, params(sigma_x, sigma_y), words, q.bytes - 1));
                }
    // the widest halo, and the images of the real calibration at the sigma the reference's note names
    {
        SmoothPlan q; std::string why;
        for(int dtype = 0; dtype < 2; dtype++)
        {
            CHECK(smooth_plan(&q, &why, 6016, 4016, dtype, params(8.0, 8.0), PLENTY));
            CHECK(q.Rx == 24 && q.Ry == 24 && q.halo_x == 24 && q.tile_h == 8 && q.rows == 56 && q.lds_bytes <= 160*1024);
        }
        CHECK(smooth_plan(&q, &why, 6016, 4016, 0, params(2.0, 2.0), PLENTY));
        CHECK(q.Rx == 6 && q.halo_x == 8 && q.tile_w == 256 && q.tile_h == 32 && q.raw_dwords == 69 && q.grid_x == 24 && q.grid_y == 126);
        CHECK(q.wx[0] + 2*(q.wx[1] + q.wx[2] + q.wx[3] + q.wx[4] + q.wx[5] + q.wx[6]) == 256);
        CHECK(smooth_plan(&q, &why, 6016, 4016, 1, params(2.0, 2.0), PLENTY));
        CHECK(q.tile_w == 128 && q.tile_h == 32 && q.raw_dwords == 73 && q.grid_x == 47 && q.grid_y == 126);
    }
    printf("ok\n");
    return 0;
}
