// TEST-ONLY stand-alone program: the image pyramid's plan (mrcal_amd/csrc/chessboard_plan.hpp,
// chessboard_pyramid_plan()) under the host sanitizers: the sizes of the levels for odd and even sides, the largest
// pyramid_levels of a size, every refusal with its message, pyramid_levels = 0 equal to chessboard_plan() field for
// field, where the level images and the corner records lie in the pool (in order, aligned, none overlapping the next),
// that a level's shared parts fit where level 0's are, the decimation's launch geometry, and what just fits the free
// device memory. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("chessboard_pyramid_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../mrcal_amd/csrc/chessboard_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const size_t PLENTY = (size_t)1 << 40;

static bool same_plan(const ChessboardPlan& a, const ChessboardPlan& b)
{
    return a.W == b.W && a.H == b.H && a.bytes_per_pixel == b.bytes_per_pixel && a.threshold_256 == b.threshold_256 &&
           a.nms_radius == b.nms_radius && a.max_candidates == b.max_candidates && a.tiles_x == b.tiles_x && a.tiles_y == b.tiles_y &&
           a.words_per_row == b.words_per_row && a.chunks == b.chunks && a.scan_per_thread == b.scan_per_thread &&
           a.refine_groups == b.refine_groups && a.image == b.image && a.response == b.response && a.words == b.words &&
           a.bases == b.bases && a.response_max == b.response_max && a.xy == b.xy && a.candidate_response == b.candidate_response &&
           a.q == b.q && a.status == b.status && a.bytes == b.bytes;
}

static bool refused(int W, int H, int bpp, int levels, const char* words, size_t free_bytes = PLENTY, int radius = 7, int max_candidates = 4096)
{
    ChessboardPyramidPlan plan; std::string why;
    if(chessboard_pyramid_plan(&plan, &why, W, H, bpp, 51, radius, max_candidates, levels, free_bytes)) return false;
    if(plan.bytes != 0 || plan.levels != 0 || plan.level[0].bytes != 0) return false;      // (a refusal leaves no plan)
    if(why.find("find_chessboard_corners():") != 0 || why.find(words) == std::string::npos) { fprintf(stderr, "got: %s\n", why.c_str()); return false; }
    return true;
}

static void check_plan(int W, int H, int bpp, int levels, int max_candidates)
{
    ChessboardPyramidPlan p; ChessboardPlan flat; std::string why;
    CHECK(chessboard_pyramid_plan(&p, &why, W, H, bpp, 51, 7, max_candidates, levels, PLENTY));
    CHECK(chessboard_plan(&flat, &why, W, H, bpp, 51, 7, max_candidates, PLENTY));
    CHECK(p.levels == levels);
    CHECK(same_plan(p.level[0], flat));                                                    // (level 0 IS the plan there was)
    if(levels == 0) { CHECK(p.bytes == flat.bytes && p.descent_q == 0 && p.descent_level == 0); return; }
    size_t end = flat.bytes;
    int w = W, h = H;
    for(int l=1; l<=levels; l++)
    {
        const ChessboardPlan& q = p.level[l];
        const ChessboardPlan& z = p.level[0];
        w /= 2; h /= 2;                                                                     // (an odd last row or column is dropped)
        CHECK(q.W == w && q.H == h && q.W >= CB_MIN_SIDE && q.H >= CB_MIN_SIDE && q.bytes_per_pixel == bpp);
        ChessboardPlan alone;
        CHECK(chessboard_plan(&alone, &why, w, h, bpp, 51, 7, max_candidates, PLENTY));
        CHECK(q.tiles_x == alone.tiles_x && q.tiles_y == alone.tiles_y && q.words_per_row == alone.words_per_row && q.chunks == alone.chunks &&
              q.scan_per_thread == alone.scan_per_thread && q.refine_groups == alone.refine_groups);
        // the image behind everything before it; the rest where level 0's is, and no larger
        CHECK(q.image == end && q.image % CB_ALIGN == 0);
        end = q.image + cb_aligned((size_t)w*h*bpp);
        CHECK(q.response == z.response && q.words == z.words && q.bases == z.bases && q.response_max == z.response_max && q.xy == z.xy &&
              q.candidate_response == z.candidate_response && q.q == z.q && q.status == z.status);
        CHECK(q.response + (size_t)w*h*4 <= q.words);
        CHECK(q.words + (size_t)q.chunks*CB_CHUNK_WORDS*8 <= q.bases && q.chunks <= z.chunks);
        CHECK(q.bases + ((size_t)q.chunks + 1)*4 <= q.response_max);
        // the decimation: whole 16-byte words of the rows above, or a lane an output pixel
        const size_t row_bytes = (size_t)p.level[l - 1].W*bpp;
        CHECK(p.decimate_wide[l] == (row_bytes % 16 == 0));
        const size_t lanes = p.decimate_wide[l] ? row_bytes/16*(size_t)h : (size_t)w*h;
        CHECK((size_t)p.decimate_groups[l]*CB_THREADS >= lanes && ((size_t)p.decimate_groups[l] - 1)*CB_THREADS < lanes);
        if(p.decimate_wide[l])
        {
            CHECK(p.level[l - 1].W % 2 == 0 && row_bytes/16*8 == (size_t)w*bpp);            // (a word of two rows is 8 bytes of outputs: a whole row)
            CHECK(p.level[l - 1].image % 16 == 0 && q.image % 8 == 0);
            CHECK((2*(size_t)h - 1)*row_bytes + row_bytes <= (size_t)p.level[l - 1].W*p.level[l - 1].H*bpp);   // (the last row read is inside)
        }
        else
            CHECK(2*((size_t)h - 1) + 1 < (size_t)p.level[l - 1].H && 2*((size_t)w - 1) + 1 < (size_t)p.level[l - 1].W);
    }
    CHECK(p.descent_q == end && p.descent_level == p.descent_q + cb_aligned((size_t)max_candidates*16));
    CHECK(p.bytes == p.descent_level + cb_aligned((size_t)max_candidates*4));
    CHECK(p.bytes - flat.bytes <= (size_t)W*H*bpp/3 + (size_t)levels*CB_ALIGN + (size_t)max_candidates*20 + 2*CB_ALIGN);   // (+1/3 of the image)
    // what just fits, and what does not
    ChessboardPyramidPlan again;
    CHECK(chessboard_pyramid_plan(&again, &why, W, H, bpp, 51, 7, max_candidates, levels, p.bytes) && again.bytes == p.bytes);
    CHECK(refused(W, H, bpp, levels, "bytes of device memory", p.bytes - 1, 7, max_candidates));
    // (level 0 alone would fit: the levels are counted)
    CHECK(refused(W, H, bpp, levels, "bytes of device memory", flat.bytes, 7, max_candidates));
}

int main()
{
    // the largest pyramid_levels of a size
    CHECK(chessboard_max_pyramid_levels(32, 32) == 0 && chessboard_max_pyramid_levels(63, 64) == 0);
    CHECK(chessboard_max_pyramid_levels(64, 65) == 1 && chessboard_max_pyramid_levels(65, 64) == 1 && chessboard_max_pyramid_levels(127, 4000) == 1);
    CHECK(chessboard_max_pyramid_levels(800, 640) == 4 && chessboard_max_pyramid_levels(1200, 900) == 4 && chessboard_max_pyramid_levels(6016, 4016) == 6);
    CHECK(chessboard_max_pyramid_levels(1 << 14, 1 << 14) == 8 && chessboard_max_pyramid_levels(1 << 13, 1 << 14) == 8 && chessboard_max_pyramid_levels(8191, 1 << 14) == 7);

    // the refusals
    CHECK(refused(800, 640, 1, -1, "pyramid_levels must be in 0..8, got -1"));
    CHECK(refused(800, 640, 1, 9, "pyramid_levels must be in 0..8, got 9"));
    CHECK(refused(1 << 14, 1 << 14, 2, 9, "pyramid_levels must be in 0..8, got 9"));
    CHECK(refused(32, 32, 1, 1, "an image of 32 x 32 pixels is too small for pyramid_levels = 1: level 1 would have 16 x 16 pixels, at least 32 x 32; at most pyramid_levels = 0"));
    CHECK(refused(64, 65, 1, 2, "an image of 64 x 65 pixels is too small for pyramid_levels = 2: level 2 would have 16 x 16 pixels, at least 32 x 32; at most pyramid_levels = 1"));
    CHECK(refused(800, 640, 2, 5, "an image of 800 x 640 pixels is too small for pyramid_levels = 5: level 5 would have 25 x 20 pixels, at least 32 x 32; at most pyramid_levels = 4"));
    CHECK(refused(800, 640, 2, 8, "at most pyramid_levels = 4"));
    // (those of one level come first, as they were)
    CHECK(refused(31, 640, 1, 3, "an image of 31 x 640 pixels is too small: at least 32 x 32"));
    CHECK(refused(800, 640, 3, 3, "images must have dtype uint8 or uint16, not 3 bytes a pixel"));
    CHECK(refused(800, 640, 1, 9, "nms_radius must be in 1..16, got 17", PLENTY, 17));
    CHECK(refused(1 << 14, (1 << 14) + 1, 1, 2, "is too large: at most 268435456 pixels"));

    // the plans: odd and even sides, the smallest legal levels, the largest images
    const int sizes[][2] = { {32, 32}, {64, 64}, {65, 67}, {64, 65}, {130, 97}, {131, 97}, {480, 400}, {800, 640}, {1200, 900}, {6016, 4016}, {6017, 4015},
                             {1 << 14, 1 << 14}, {64, 1 << 22}, {1 << 22, 64}, {16383, 16385} };
    int plans = 0;
    for(const auto& s : sizes) for(int bpp=1; bpp<=2; bpp++)
    {
        const int most = chessboard_max_pyramid_levels(s[0], s[1]);
        for(int levels=0; levels<=most; levels++)
            for(int max_candidates : { 1, 4096, 65536 }) { check_plan(s[0], s[1], bpp, levels, max_candidates); plans++; }
        if(most < CB_MAX_LEVELS) CHECK(refused(s[0], s[1], bpp, most + 1, "at most pyramid_levels ="));
    }
    CHECK(plans > 300);
    printf("ok\n");
    return 0;
}
