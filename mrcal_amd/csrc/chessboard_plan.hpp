// What chessboard.hip works out on the host before it touches the device: the arguments that are refused and the
// messages, where the image, the response, the mask words, the bases, the maximum and the candidate records lie in the
// ONE pooled allocation a detector owns, and the launch geometry of the five kernels. Plain structs in and out, no HIP
// type or call. tests/hostcheck/chessboard_grid_check.cpp runs it under the host sanitizers. With an image pyramid
// (chessboard_pyramid_plan()): the geometry of every level, where the level images lie behind the level-0 pool, and the
// refusals of pyramid_levels; tests/hostcheck/chessboard_pyramid_plan_check.cpp walks that.
//
// What a corner is: include/mrcal_amd.h, "chessboard corners".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "image_format.hpp"

namespace mrcal_amd {

#define CB_THREADS 256                  // of every kernel but the scan
#define CB_TX 64                        // a tile of cb_response_kernel and cb_candidates_kernel: 64 x 16 pixels. A wavefront
#define CB_TY 16                        //   is a row of it: its verdicts are ONE __ballot, one mask word
#define CB_HALO 6                       // of the image around a tile of R: 5 for the ring and 1 for the blur
#define CB_RING 5                       // of the blurred image around a tile of R
#define CB_NMS_RADIUS_MAX 16            // the LDS tile of cb_candidates_kernel is laid out for this radius
#define CB_CHUNK_WORDS 16               // mask words a workgroup of cb_scatter_kernel places: the unit of the scan
#define CB_SCAN_THREADS 1024            // cb_scan_kernel is ONE workgroup of these
#define CB_MIN_SIDE 32
#define CB_MAX_CANDIDATES 65536
#define CB_ALIGN 256                    // of the parts of the pool, in bytes
#define CB_WINDOW 5                     // the refinement window: offsets -5..5
#define CB_REFINE_ITERATIONS 20
#define CB_STATUS_OK 0
#define CB_STATUS_SINGULAR 1
#define CB_STATUS_LEFT 2
#define CB_MAX_LEVELS 8                 // pyramid_levels is 0..8
#define CB_DESCENT_AGREEMENT 0.3        // tau of p3, in pixels of the level a corner descends to
#define CB_DECIMATE_BYTES 16            // of each of two rows a lane of the wide cb_decimate_kernel loads

static_assert(CB_THREADS == 4*CB_TX && CB_TY % 4 == 0, "a wavefront is a row of the tile, four rows at a time");
static_assert(IMAGE_MAX_PIXELS < (1L << 31), "a pixel index is an int32");

struct ChessboardPlan
{
    int      W = 0, H = 0, bytes_per_pixel = 0;
    int      threshold_256 = 0, nms_radius = 0, max_candidates = 0;
    unsigned tiles_x = 0, tiles_y = 0;  // of the response and candidates kernels: ONE grid dimension, tiles_x tiles_y
    unsigned words_per_row = 0;         // = tiles_x: bit b of word (y, k) is pixel (64 k + b, y)
    unsigned chunks = 0;                // workgroups of the scatter: CB_CHUNK_WORDS words each, in row-major word order
    unsigned scan_per_thread = 0;       // chunks a thread of the scan sums: chunks <= CB_SCAN_THREADS scan_per_thread
    unsigned refine_groups = 0;         // workgroups of the refinement: a wavefront a candidate, max_candidates of them
    // offsets into the pool, in bytes
    size_t   image = 0;                 // bytes_per_pixel a pixel
    size_t   response = 0;              // int32 a pixel
    size_t   words = 0;                 // uint64 [chunks CB_CHUNK_WORDS]; those past H words_per_row stay 0
    size_t   bases = 0;                 // uint32 [chunks + 1]: the exclusive scan of the chunks' counts, and the total
    size_t   response_max = 0;          // int32
    size_t   xy = 0;                    // int32 [max_candidates][2]
    size_t   candidate_response = 0;    // int32 [max_candidates]
    size_t   q = 0;                     // double [max_candidates][2]
    size_t   status = 0;                // int32 [max_candidates]
    size_t   bytes = 0;                 // of the pool
};

inline size_t cb_aligned(size_t n) { return (n + CB_ALIGN - 1)/CB_ALIGN*CB_ALIGN; }

// the whole plan. free_bytes: what the device has free. false: a refusal, with the reason in *error
inline bool chessboard_plan(ChessboardPlan* plan, std::string* error, int W, int H, int bytes_per_pixel,
                            int threshold_256, int nms_radius, int max_candidates, size_t free_bytes)
{
    *plan = ChessboardPlan();
    char buf[256];
    buf[0] = 0;
    if(!(bytes_per_pixel == 1 || bytes_per_pixel == 2))
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): images must have dtype uint8 or uint16, not %d bytes a pixel", bytes_per_pixel);
    else if(W < CB_MIN_SIDE || H < CB_MIN_SIDE)
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): an image of %d x %d pixels is too small: at least %d x %d",
                 W, H, CB_MIN_SIDE, CB_MIN_SIDE);
    else if(!image_size_ok(W, H))
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): an image of %d x %d pixels is too large: at most %ld pixels",
                 W, H, IMAGE_MAX_PIXELS);
    else if(threshold_256 < 0 || threshold_256 > 255)
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): threshold_256 must be in 0..255, got %d", threshold_256);
    else if(nms_radius < 1 || nms_radius > CB_NMS_RADIUS_MAX)
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): nms_radius must be in 1..%d, got %d", CB_NMS_RADIUS_MAX, nms_radius);
    else if(max_candidates < 1 || max_candidates > CB_MAX_CANDIDATES)
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): max_candidates must be in 1..%d, got %d", CB_MAX_CANDIDATES, max_candidates);
    if(buf[0] != 0) { *error = buf; return false; }

    const size_t N = (size_t)W*(size_t)H;
    ChessboardPlan p;
    p.W = W; p.H = H; p.bytes_per_pixel = bytes_per_pixel;
    p.threshold_256 = threshold_256; p.nms_radius = nms_radius; p.max_candidates = max_candidates;
    p.tiles_x         = (unsigned)((W + CB_TX - 1)/CB_TX);
    p.tiles_y         = (unsigned)((H + CB_TY - 1)/CB_TY);
    p.words_per_row   = p.tiles_x;
    const size_t words = (size_t)p.words_per_row*(size_t)H;
    p.chunks          = (unsigned)((words + CB_CHUNK_WORDS - 1)/CB_CHUNK_WORDS);
    p.scan_per_thread = (p.chunks + CB_SCAN_THREADS - 1)/CB_SCAN_THREADS;
    p.refine_groups   = ((unsigned)max_candidates + CB_THREADS/64 - 1)/(CB_THREADS/64);
    p.image              = 0;
    p.response           = cb_aligned(N*(size_t)bytes_per_pixel);
    p.words              = p.response           + cb_aligned(N*sizeof(int32_t));
    p.bases              = p.words              + cb_aligned((size_t)p.chunks*CB_CHUNK_WORDS*sizeof(uint64_t));
    p.response_max       = p.bases              + cb_aligned(((size_t)p.chunks + 1)*sizeof(uint32_t));
    p.xy                 = p.response_max       + cb_aligned(sizeof(int32_t));
    p.candidate_response = p.xy                 + cb_aligned((size_t)max_candidates*2*sizeof(int32_t));
    p.q                  = p.candidate_response + cb_aligned((size_t)max_candidates*sizeof(int32_t));
    p.status             = p.q                  + cb_aligned((size_t)max_candidates*2*sizeof(double));
    p.bytes              = p.status             + cb_aligned((size_t)max_candidates*sizeof(int32_t));
    if(p.bytes > free_bytes)
    {
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): %d x %d pixels need %zu bytes of device memory; %zu are free",
                 W, H, p.bytes, free_bytes);
        *error = buf;
        return false;
    }
    *plan = p;
    return true;
}

// a board that cannot be looked for (a seed is the middle of 3 x 3 corners)
inline bool chessboard_board_ok(std::string* error, int board_width, int board_height)
{
    if(board_width >= 3 && board_height >= 3 && board_width <= 256 && board_height <= 256) return true;
    char buf[256];
    snprintf(buf, sizeof(buf), "find_chessboard_corners(): a board has 3..256 corners a side, got %d x %d", board_width, board_height);
    *error = buf;
    return false;
}

// ------------------------------------------------------------------------------------------------------ the pyramid
// Level l has (W >> l) x (H >> l) pixels. level[0] IS chessboard_plan()'s plan, field for field. level[l], l >= 1, is
// the plan of an image of that level's size whose response, words, bases, maximum and candidate records lie where level
// 0's do (they are smaller, and one level is looked at at a time) and whose image lies behind level 0's pool.
struct ChessboardPyramidPlan
{
    int            levels = 0;                          // pyramid_levels: levels 0..levels exist
    ChessboardPlan level[CB_MAX_LEVELS + 1];
    // cb_decimate_kernel making level l (l >= 1) from level l - 1
    bool           decimate_wide[CB_MAX_LEVELS + 1] = {};   // rows of level l - 1 are whole 16-byte words: a lane takes a word of two rows
    unsigned       decimate_groups[CB_MAX_LEVELS + 1] = {}; // workgroups of CB_THREADS: a lane a word pair (wide) or an output pixel
    size_t         descent_q = 0;                       // double [max_candidates][2]: the board's corners, each in the pixels of its level
    size_t         descent_level = 0;                   // int32 [max_candidates]
    size_t         bytes = 0;                           // of the pool
};

// the largest pyramid_levels an image of W x H pixels allows: every level has CB_MIN_SIDE pixels a side
inline int chessboard_max_pyramid_levels(int W, int H)
{
    int n = 0;
    while(n < CB_MAX_LEVELS && (W >> (n + 1)) >= CB_MIN_SIDE && (H >> (n + 1)) >= CB_MIN_SIDE) n++;
    return n;
}

inline bool chessboard_pyramid_plan(ChessboardPyramidPlan* plan, std::string* error, int W, int H, int bytes_per_pixel,
                                    int threshold_256, int nms_radius, int max_candidates, int pyramid_levels, size_t free_bytes)
{
    *plan = ChessboardPyramidPlan();
    ChessboardPyramidPlan p;
    // (the refusals of one level first, in their order; the memory is looked at below, for the whole pool)
    if(!chessboard_plan(&p.level[0], error, W, H, bytes_per_pixel, threshold_256, nms_radius, max_candidates, SIZE_MAX)) return false;
    char buf[256];
    if(pyramid_levels < 0 || pyramid_levels > CB_MAX_LEVELS)
    {
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): pyramid_levels must be in 0..%d, got %d", CB_MAX_LEVELS, pyramid_levels);
        *error = buf;
        return false;
    }
    const int most = chessboard_max_pyramid_levels(W, H);
    if(pyramid_levels > most)
    {
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): an image of %d x %d pixels is too small for pyramid_levels = %d: "
                 "level %d would have %d x %d pixels, at least %d x %d; at most pyramid_levels = %d",
                 W, H, pyramid_levels, most + 1, W >> (most + 1), H >> (most + 1), CB_MIN_SIDE, CB_MIN_SIDE, most);
        *error = buf;
        return false;
    }
    p.levels = pyramid_levels;
    p.bytes  = p.level[0].bytes;
    for(int l=1; l<=pyramid_levels; l++)
    {
        ChessboardPlan& q = p.level[l];
        if(!chessboard_plan(&q, error, W >> l, H >> l, bytes_per_pixel, threshold_256, nms_radius, max_candidates, SIZE_MAX)) return false;
        const ChessboardPlan& z = p.level[0];
        q.response = z.response; q.words = z.words; q.bases = z.bases; q.response_max = z.response_max;
        q.xy = z.xy; q.candidate_response = z.candidate_response; q.q = z.q; q.status = z.status;
        q.image = p.bytes;
        p.bytes += cb_aligned((size_t)q.W*(size_t)q.H*(size_t)bytes_per_pixel);
        q.bytes = p.bytes;
        const size_t row_bytes = (size_t)p.level[l - 1].W*(size_t)bytes_per_pixel;
        p.decimate_wide[l] = row_bytes % CB_DECIMATE_BYTES == 0;
        const size_t lanes = p.decimate_wide[l] ? row_bytes/CB_DECIMATE_BYTES*(size_t)q.H : (size_t)q.W*(size_t)q.H;
        p.decimate_groups[l] = (unsigned)((lanes + CB_THREADS - 1)/CB_THREADS);
    }
    if(pyramid_levels > 0)
    {
        p.descent_q     = p.bytes;
        p.descent_level = p.descent_q     + cb_aligned((size_t)max_candidates*2*sizeof(double));
        p.bytes         = p.descent_level + cb_aligned((size_t)max_candidates*sizeof(int32_t));
    }
    if(p.bytes > free_bytes)
    {
        snprintf(buf, sizeof(buf), "find_chessboard_corners(): %d x %d pixels need %zu bytes of device memory; %zu are free",
                 W, H, p.bytes, free_bytes);
        *error = buf;
        return false;
    }
    *plan = p;
    return true;
}

} // namespace mrcal_amd
