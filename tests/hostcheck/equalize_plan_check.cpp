// TEST-ONLY stand-alone program: the host-only planning of equalize.hip (mrcal_amd/csrc/equalize_plan.hpp) under the
// host sanitizers: every refusal with its message, the padded and tile sizes (the divisible side that gets a whole
// extra `tiles` among them), the clip limit and the LUT scale, the offsets of the parts of the pooled allocation (in
// order, none overlapping the next, the last one ending the pool), the launch geometry, and the refusal of an image
// that does not fit the free device memory. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("equalize_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "../../mrcal_amd/csrc/equalize_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const size_t PLENTY = (size_t)1 << 40;

static EqualizeParams params(int method, double clip_limit = 8.0, int tiles_x = 8, int tiles_y = 8)
{
    EqualizeParams p;
    p.method = method; p.clip_limit = clip_limit; p.tiles_x = tiles_x; p.tiles_y = tiles_y;
    return p;
}

static bool refused(int W, int H, int dtype, const EqualizeParams& p, const char* words, size_t free_bytes = PLENTY)
{
    EqualizePlan plan; std::string why;
    if(equalize_plan(&plan, &why, W, H, dtype, p, free_bytes)) return false;
    if(plan.bytes != 0 || plan.hist_grid != 0 || plan.map_grid != 0) return false;      // (a refusal leaves no plan)
    return why.find("equalize():") == 0 && why.find(words) != std::string::npos;
}

int main()
{
    const EqualizeParams clahe = params(EQUALIZE_METHOD_CLAHE), stretch = params(EQUALIZE_METHOD_STRETCH);
    // the refusals
    {
        CHECK(refused(100, 80, 0, params(3), "the method must be one of MRCAL_AMD_EQUALIZE_* (0..2), not 3"));
        CHECK(refused(100, 80, 0, params(-1), "not -1"));
        CHECK(refused(100, 80, 2, clahe, "images are uint8 or uint16"));
        CHECK(refused(100, 80, -1, stretch, "images are uint8 or uint16"));
        CHECK(refused(0, 80, 0, clahe, "images of 0 x 80 pixels cannot be equalized"));
        CHECK(refused(100, -1, 1, stretch, "images of 100 x -1 pixels cannot be equalized"));
        CHECK(refused(1 << 15, (1 << 13) + 1, 0, clahe, "cannot be equalized"));           // 2^28 + 2^15 pixels
        CHECK(refused(INT32_MAX, INT32_MAX, 0, stretch, "cannot be equalized"));           // (no overflow on the way)
        CHECK(refused(100, 80, 0, params(EQUALIZE_METHOD_CLAHE, 8.0, 0, 8), "tiles must be at least (1,1) and at most 4096 in all. Got (0,8)"));
        CHECK(refused(100, 80, 0, params(EQUALIZE_METHOD_CLAHE, 8.0, 8, -2), "Got (8,-2)"));
        CHECK(refused(100, 80, 0, params(EQUALIZE_METHOD_CLAHE, 8.0, 65, 64), "Got (65,64)"));
        CHECK(refused(100, 80, 0, params(EQUALIZE_METHOD_CLAHE, 8.0, INT32_MAX, INT32_MAX), "at most 4096"));
        CHECK(refused(100, 80, 0, params(EQUALIZE_METHOD_CLAHE, NAN), "clip_limit is not a number"));
        // (5,3) = (H,W) with 8 x 8 tiles: padded by (5,3), and a reflection reaches (2,4)
        CHECK(refused(3, 5, 0, clahe, "an image of 3 x 5 pixels is too small for (8,8) tiles: it would be padded by (5,3) pixels, and a reflection reaches (2,4)"));
        CHECK(refused(8, 9, 1, clahe, "padded by (8,7) pixels, and a reflection reaches (7,8)"));          // the divisible side's whole 8
        // ... and what is just inside is not, nor is what the other method does not read
        EqualizePlan plan; std::string why;
        CHECK(equalize_plan(&plan, &why, 9, 9, 0, clahe, PLENTY));                          // padded by (7,7), reaches (8,8)
        CHECK(equalize_plan(&plan, &why, 8, 8, 1, clahe, PLENTY));
        CHECK(equalize_plan(&plan, &why, 3, 5, 0, stretch, PLENTY));
        CHECK(equalize_plan(&plan, &why, 3, 5, 0, params(EQUALIZE_METHOD_STRETCH, NAN, 0, 0), PLENTY));
        CHECK(equalize_plan(&plan, &why, 1 << 15, 1 << 13, 0, clahe, PLENTY));              // 2^28 pixels
        CHECK(equalize_plan(&plan, &why, 64, 64, 0, params(EQUALIZE_METHOD_CLAHE, -1.0, 64, 64), PLENTY));
    }
    // CLAHE: the padding, the tiles, the limits. { W, H, tiles_x, tiles_y, Wpad, Hpad }
    const int sizes[][6] = { { 8, 8, 8, 8, 8, 8 }, { 16, 16, 8, 8, 16, 16 }, { 16, 17, 8, 8, 24, 24 }, { 23, 17, 8, 8, 24, 24 },
                             { 64, 9, 8, 8, 72, 16 }, { 130, 65, 8, 8, 136, 72 }, { 257, 131, 8, 8, 264, 136 }, { 47, 31, 3, 5, 48, 35 },
                             { 722, 482, 8, 8, 728, 488 }, { 6016, 4016, 8, 8, 6016, 4016 }, { 300, 200, 1, 1, 300, 200 },
                             { 1 << 14, 1 << 14, 64, 64, 1 << 14, 1 << 14 }, { (1 << 14) - 1, 1 << 14, 64, 64, 1 << 14, (1 << 14) + 64 } };
    for(const auto& s : sizes)
        for(int dtype = 0; dtype < 2; dtype++)
            for(const double clip_limit : { 2.0, 8.0, 40.0, 0.0, -3.0, 1e300 })
            {
                const int W = s[0], H = s[1];
                const EqualizeParams p = params(EQUALIZE_METHOD_CLAHE, clip_limit, s[2], s[3]);
                EqualizePlan q; std::string why;
                CHECK(equalize_plan(&q, &why, W, H, dtype, p, PLENTY));
                CHECK(q.method == EQUALIZE_METHOD_CLAHE && q.dtype == dtype && q.dtype_out == dtype && q.W == W && q.H == H);
                CHECK(q.Wpad == s[4] && q.Hpad == s[5]);
                CHECK(q.tw*s[2] == q.Wpad && q.th*s[3] == q.Hpad);
                // what is read by reflection lies inside the image
                CHECK(q.Wpad - 1 <= 2*(W - 1) || q.Wpad == W);
                CHECK(q.Hpad - 1 <= 2*(H - 1) || q.Hpad == H);
                const int hist = dtype == 0 ? 256 : 65536;
                CHECK(q.hist_size == hist);
                const long total = (long)q.tw*q.th;
                CHECK(q.lut_scale == (float)(hist - 1)/(float)total && q.inv_tw == 1.0f/(float)q.tw && q.inv_th == 1.0f/(float)q.th);
                if(clip_limit <= 0.0) CHECK(q.clip == INT32_MAX);
                else if(clip_limit > 1e100) CHECK(q.clip == INT32_MAX);
                else
                {
                    long expected = (long)(clip_limit*(double)total/(double)hist);
                    if(expected < 1) expected = 1;
                    CHECK(q.clip == expected);
                }
                // every row of a tile is in one band, and no workgroup is idle
                const size_t tiles = (size_t)s[2]*s[3];
                CHECK((size_t)q.bands*EQUALIZE_BAND_ROWS >= (size_t)q.th && (size_t)(q.bands - 1)*EQUALIZE_BAND_ROWS < (size_t)q.th);
                CHECK((size_t)q.hist_grid == tiles*q.bands && (size_t)q.lut_grid == tiles);
                CHECK((size_t)q.lut_threads*(dtype == 0 ? 4 : 64) == (size_t)hist);
                const size_t across = (size_t)EQUALIZE_THREADS*EQUALIZE_APPLY_X;
                CHECK(q.apply_grid_x*across >= (size_t)W && (q.apply_grid_x - 1)*across < (size_t)W);
                CHECK((size_t)q.apply_grid_y*EQUALIZE_APPLY_ROWS >= (size_t)H && (size_t)(q.apply_grid_y - 1)*EQUALIZE_APPLY_ROWS < (size_t)H);
                CHECK((size_t)q.apply_grid == (size_t)q.apply_grid_x*q.apply_grid_y);
                CHECK(q.luts_in_lds == (dtype == 0 && tiles*256 <= EQUALIZE_LDS_LUT_BYTES));
                // the parts in order, what each needs
                const size_t N = (size_t)W*H, pixel = dtype == 0 ? 1 : 2;
                CHECK(q.image == 0 && q.result % EQUALIZE_ALIGN == 0 && q.hist % EQUALIZE_ALIGN == 0 && q.lut % EQUALIZE_ALIGN == 0);
                CHECK(q.image + N*pixel <= q.result && q.result + N*pixel <= q.workspace && q.workspace == q.hist);
                CHECK(q.hist_bytes == tiles*hist*4 && q.hist + q.hist_bytes <= q.lut);
                CHECK(q.lut + tiles*hist*pixel <= q.bytes && q.bytes - q.lut < tiles*hist*pixel + EQUALIZE_ALIGN);
                // the workspace alone: the same parts, from 0
                EqualizePlan w;
                CHECK(equalize_plan(&w, &why, W, H, dtype, p, PLENTY, false));
                CHECK(w.workspace == 0 && w.hist == 0 && w.lut == q.lut - q.hist && w.bytes == q.bytes - q.workspace);
                // what does not fit is refused with its size; what just fits is not
                CHECK(equalize_plan(&w, &why, W, H, dtype, p, q.bytes));
                char words[128];
                snprintf(words, sizeof(words), "%d x %d pixels need %zu bytes of device memory; %zu are free", W, H, q.bytes, q.bytes - 1);
                CHECK(refused(W, H, dtype, p, words, q.bytes - 1));
            }
    // the default tile of the real calibration's images, and mrcal's clip limit there
    {
        EqualizePlan q; std::string why;
        CHECK(equalize_plan(&q, &why, 6016, 4016, 0, clahe, PLENTY));
        CHECK(q.tw == 752 && q.th == 502 && q.clip == 11797 && q.bands == 16 && q.hist_grid == 1024 && q.luts_in_lds);
        CHECK(equalize_plan(&q, &why, 6016, 4016, 1, clahe, PLENTY));
        CHECK(q.clip == 46 && q.hist_bytes == (size_t)16 << 20 && !q.luts_in_lds);
        // (8,8): tiles of one pixel, the clip limit held at 1
        CHECK(equalize_plan(&q, &why, 8, 8, 0, clahe, PLENTY));
        CHECK(q.tw == 1 && q.th == 1 && q.clip == 1 && q.bands == 1);
    }
    // stretch
    for(const auto& s : sizes)
        for(int dtype = 0; dtype < 2; dtype++)
        {
            const int W = s[0], H = s[1];
            EqualizePlan q; std::string why;
            CHECK(equalize_plan(&q, &why, W, H, dtype, stretch, PLENTY));
            CHECK(q.method == EQUALIZE_METHOD_STRETCH && q.dtype == dtype && q.dtype_out == EQUALIZE_DTYPE_UINT8);
            const size_t N = (size_t)W*H, per = (size_t)EQUALIZE_THREADS*EQUALIZE_MAP_PIXELS;
            CHECK((size_t)q.map_grid*per >= N && (size_t)(q.map_grid - 1)*per < N);
            CHECK(q.minmax_grid >= 1 && q.minmax_grid <= EQUALIZE_MINMAX_GRID_MAX && q.minmax_grid <= q.map_grid);
            CHECK(q.image == 0 && q.image + N*(dtype == 0 ? 1 : 2) <= q.result && q.result + N <= q.minmax);
            CHECK(q.minmax % EQUALIZE_ALIGN == 0 && q.minmax + 2*sizeof(uint32_t) <= q.bytes);
            CHECK(q.hist_grid == 0 && q.lut_grid == 0);
        }
    printf("ok\n");
    return 0;
}
