// TEST-ONLY stand-alone program: the host-only planning of speckle_filter.hip (mrcal_amd/csrc/speckle_plan.hpp) under
// the host sanitizers: every refusal with its message, the offsets of the parts of the pooled allocation (in order,
// none overlapping the next, the last one ending the pool), the launch geometry at the sizes where a tile is just full
// or just not, what the matcher's two keywords become, and the refusal of an image that does not fit the free device
// memory. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("speckle_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../mrcal_amd/csrc/speckle_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const size_t PLENTY = (size_t)1 << 40;

static bool words_are(const std::string& why, const char* words)
{
    return why.find("filter_speckles():") == 0 && why.find(words) != std::string::npos;
}

static bool plan_refused(int W, int H, const char* words, size_t free_bytes = PLENTY)
{
    SpecklePlan plan; std::string why;
    if(speckle_plan(&plan, &why, W, H, free_bytes)) return false;
    if(plan.bytes != 0 || plan.grids.pixel_grid != 0 || plan.grids.tile_grid != 0) return false;     // (a refusal leaves no plan)
    return words_are(why, words);
}

static bool params_refused(long new_value, long max_speckle_size, long max_diff, const char* words)
{
    std::string why;
    return !speckle_params_ok(&why, 100, 80, new_value, max_speckle_size, max_diff) && words_are(why, words);
}

static bool matcher_refused(long window, long range, const char* words)
{
    SpeckleParams p; std::string why;
    return !speckle_params_of_matcher(&p, &why, 0, 16, window, range) && words_are(why, words);
}

int main()
{
    // the refusals
    {
        CHECK(plan_refused(0, 80, "images of 0 x 80 pixels cannot be filtered"));
        CHECK(plan_refused(100, -1, "images of 100 x -1 pixels cannot be filtered"));
        CHECK(plan_refused(1 << 15, (1 << 13) + 1, "cannot be filtered"));           // 2^28 + 2^15 pixels
        CHECK(plan_refused(INT32_MAX, INT32_MAX, "cannot be filtered"));             // (no overflow on the way)
        CHECK(params_refused(-32769, 0, 0, "new_value must be in -32768..32767. Got -32769"));
        CHECK(params_refused(32768, 0, 0, "new_value must be in -32768..32767. Got 32768"));
        CHECK(params_refused(0, -1, 0, "max_speckle_size must be a non-negative integer. Got -1"));
        CHECK(params_refused(0, 0, -1, "max_diff must be a non-negative integer. Got -1"));
        CHECK(matcher_refused(-1, 0, "speckle_window_size must be a non-negative integer. Got -1"));
        CHECK(matcher_refused(0, -2, "speckle_range must be a non-negative integer. Got -2"));
        // ... and what is just inside is not
        std::string why;
        CHECK(speckle_params_ok(&why, 1 << 15, 1 << 13, -32768, 0, 0));              // 2^28 pixels
        CHECK(speckle_params_ok(&why, 1, 1, 32767, INT32_MAX, (long)1 << 40));
    }
    // the arguments as the kernels take them
    {
        SpeckleParams p = speckle_params(-16, 200, 32);
        CHECK(p.new_value == -16 && p.max_speckle_size == 200 && p.max_diff == 32);
        p = speckle_params(5, (long)1 << 40, 65536);
        CHECK(p.new_value == 5 && p.max_speckle_size == INT32_MAX && p.max_diff == 65535);
        p = speckle_params(5, 0, 65535);
        CHECK(p.max_diff == 65535);
        std::string why;
        CHECK(speckle_params_of_matcher(&p, &why, -3, 16, 200, 2));
        CHECK(p.new_value == -64 && p.max_speckle_size == 200 && p.max_diff == 32);
        CHECK(speckle_params_of_matcher(&p, &why, 0, 16, 0, 0));
        CHECK(p.new_value == -16 && p.max_speckle_size == 0 && p.max_diff == 0);
        CHECK(speckle_params_of_matcher(&p, &why, 2031, 16, (long)1 << 40, 4095));
        CHECK(p.new_value == 32480 && p.max_speckle_size == INT32_MAX && p.max_diff == 65520);
        CHECK(speckle_params_of_matcher(&p, &why, -2047, 16, 1, 4096));
        CHECK(p.new_value == -32768 && p.max_diff == 65535);
        CHECK(speckle_params_of_matcher(&p, &why, 0, 16, 1, (long)1 << 60));         // (no overflow on the way)
        CHECK(p.max_diff == 65535);
    }
    // the pool and the grids, at the sizes where a tile is just full or just not
    const int sizes[][2] = { { 9, 7 }, { 63, 8 }, { 64, 9 }, { 65, 10 }, { 17, 64 }, { 130, 65 }, { 131, 130 }, { 150, 35 }, { 1, 1 },
                             { 64, 16 }, { 65, 16 }, { 64, 17 }, { 128, 32 }, { 129, 33 }, { 1024, 768 }, { 6016, 4016 },
                             { 1, 1 << 28 }, { 1 << 28, 1 }, { 1 << 14, 1 << 14 } };       // (W,H)
    for(const auto& size : sizes)
    {
        const int W = size[0], H = size[1];
        SpecklePlan plan; std::string why;
        CHECK(speckle_plan(&plan, &why, W, H, PLENTY));
        const SpeckleGrids& g = plan.grids;
        CHECK(g.W == W && g.H == H);
        const size_t N = (size_t)W*H;
        // the parts in order, what each needs
        CHECK(plan.image == 0 && plan.label % SPECKLE_ALIGN == 0 && plan.count % sizeof(int32_t) == 0);
        CHECK(plan.image + N*2 <= plan.label && plan.label - plan.image < N*2 + SPECKLE_ALIGN);
        CHECK(plan.label + N*4 == plan.count);
        CHECK(plan.count + N*4 <= plan.bytes && plan.bytes - plan.count < N*4 + SPECKLE_ALIGN);
        // ... and the workspace the matcher lends: 8 bytes a pixel, no more than S's 32, the counts right behind the labels
        CHECK(speckle_workspace_bytes(N) == 8*N && speckle_count_offset(N) == 4*N);
        CHECK(plan.count - plan.label == speckle_count_offset(N));
        // every pixel is in one tile, and no workgroup is idle
        CHECK((size_t)g.tiles_x*SPECKLE_TILE_X >= (size_t)W && (size_t)(g.tiles_x - 1)*SPECKLE_TILE_X < (size_t)W);
        CHECK((size_t)g.tiles_y*SPECKLE_TILE_Y >= (size_t)H && (size_t)(g.tiles_y - 1)*SPECKLE_TILE_Y < (size_t)H);
        CHECK((size_t)g.tile_grid == (size_t)g.tiles_x*g.tiles_y);
        CHECK((size_t)g.pixel_grid*SPECKLE_THREADS >= N && (size_t)(g.pixel_grid - 1)*SPECKLE_THREADS < N);
        // the pixels across a border: counted by hand
        size_t borders = 0;
        for(int y = SPECKLE_TILE_Y; y < H; y += SPECKLE_TILE_Y) borders += (size_t)W;
        for(int x = SPECKLE_TILE_X; x < W; x += SPECKLE_TILE_X) borders += (size_t)H;
        CHECK(g.border_pixels == borders);
        CHECK((size_t)g.border_grid*SPECKLE_THREADS >= borders);
        CHECK(borders == 0 ? g.border_grid == 0 : (size_t)(g.border_grid - 1)*SPECKLE_THREADS < borders);
        // an index fits 31 bits
        CHECK(N <= (size_t)INT32_MAX && borders <= (size_t)INT32_MAX);
        // what does not fit is refused with its size; what just fits is not
        CHECK(speckle_plan(&plan, &why, W, H, plan.bytes));
        const size_t bytes = plan.bytes;
        char size_words[96];
        snprintf(size_words, sizeof(size_words), "%d x %d pixels need %zu bytes of device memory; %zu are free", W, H, bytes, bytes - 1);
        CHECK(plan_refused(W, H, size_words, bytes - 1));
        CHECK(plan_refused(W, H, "are free", 0));
    }
    // the real calibration's size: 10 bytes a pixel
    {
        SpecklePlan plan; std::string why;
        CHECK(speckle_plan(&plan, &why, 6016, 4016, PLENTY));
        CHECK(plan.bytes >= (size_t)10*6016*4016 && plan.bytes < (size_t)10*6016*4016 + 2*SPECKLE_ALIGN);
    }
    printf("ok\n");
    return 0;
}
