// TEST-ONLY stand-alone program: the host-only parts of find_chessboard_corners() under the host sanitizers: the plan
// (mrcal_amd/csrc/chessboard_plan.hpp: every refusal with its message, the offsets of the parts of the pooled
// allocation in order and none overlapping the next, the grids from 32 x 32 to 2^28 pixels, what just fits the free
// device memory) and the lattice finder (mrcal_amd/csrc/chessboard_grid.cpp) on boards of 10 x 10, 10 x 7 and 4 x 3
// corners, turned by 0, +-40 and 180 degrees, with perspective, radial distortion down to k1 = -0.5, 0.1 px of jitter
// and 30 points of clutter: found in the order of the definition; a corner removed, only clutter: not found; a corner
// duplicated 0.4 of a step away: not taken. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("chessboard_grid_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../mrcal_amd/csrc/chessboard_plan.hpp"
#include "../../mrcal_amd/csrc/chessboard_grid.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const size_t PLENTY = (size_t)1 << 40;

static bool plan_refused(int W, int H, int bpp, int threshold, int radius, int max_candidates, const char* words, size_t free_bytes = PLENTY)
{
    ChessboardPlan plan; std::string why;
    if(chessboard_plan(&plan, &why, W, H, bpp, threshold, radius, max_candidates, free_bytes)) return false;
    if(plan.bytes != 0 || plan.tiles_x != 0 || plan.chunks != 0) return false;              // (a refusal leaves no plan)
    return why.find("find_chessboard_corners():") == 0 && why.find(words) != std::string::npos;
}

static void check_plan(int W, int H, int bpp, int max_candidates)
{
    ChessboardPlan p; std::string why;
    CHECK(chessboard_plan(&p, &why, W, H, bpp, 51, 7, max_candidates, PLENTY));
    const size_t N = (size_t)W*H;
    CHECK(p.tiles_x*(size_t)CB_TX >= (size_t)W && (p.tiles_x - 1)*(size_t)CB_TX < (size_t)W);
    CHECK(p.tiles_y*(size_t)CB_TY >= (size_t)H && (p.tiles_y - 1)*(size_t)CB_TY < (size_t)H);
    CHECK((size_t)p.tiles_x*p.tiles_y < ((size_t)1 << 31));                                // (ONE grid dimension)
    CHECK(p.words_per_row == p.tiles_x);
    CHECK((size_t)p.chunks*CB_CHUNK_WORDS >= (size_t)p.words_per_row*H && ((size_t)p.chunks - 1)*CB_CHUNK_WORDS < (size_t)p.words_per_row*H);
    CHECK((size_t)p.scan_per_thread*CB_SCAN_THREADS >= p.chunks);
    CHECK((size_t)p.refine_groups*(CB_THREADS/64) >= (size_t)max_candidates);
    // the parts in order, each with room for what it holds, aligned, the last one ending the pool
    const size_t at[]   = { p.image, p.response, p.words, p.bases, p.response_max, p.xy, p.candidate_response, p.q, p.status, p.bytes };
    const size_t need[] = { N*bpp, N*4, (size_t)p.chunks*CB_CHUNK_WORDS*8, ((size_t)p.chunks + 1)*4, 4, (size_t)max_candidates*8,
                            (size_t)max_candidates*4, (size_t)max_candidates*16, (size_t)max_candidates*4 };
    CHECK(at[0] == 0);
    for(int k=0; k<9; k++)
    {
        CHECK(at[k] % CB_ALIGN == 0);
        CHECK(at[k] + need[k] <= at[k+1] && at[k+1] - at[k] < need[k] + CB_ALIGN);
    }
    // what just fits, and what does not
    ChessboardPlan again;
    CHECK(chessboard_plan(&again, &why, W, H, bpp, 51, 7, max_candidates, p.bytes) && again.bytes == p.bytes);
    CHECK(plan_refused(W, H, bpp, 51, 7, max_candidates, "bytes of device memory", p.bytes - 1));
}

// ---------------------------------------------------------------------------------------------------------- boards
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform()                 // [0,1)
{
    rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11)/(double)(1ull << 53);
}

struct Board
{
    int W, H;
    double step;
    std::vector<double> native;         // (H,W,2): the labelling the points were made in
};

// the corners of a board in an 800 x 600 image, row-major in the board's own labelling
static Board make_board(int W, int H, double step, double degrees, double px, double py, double k1, double jitter)
{
    Board b{ W, H, step, {} };
    const double c = cos(degrees*M_PI/180.), s = sin(degrees*M_PI/180.), cx = 399.5, cy = 299.5, focal = 800.;
    for(int j=0;j<H;j++) for(int i=0;i<W;i++)
    {
        const double u = (i - (W - 1)/2.)*step, v = (j - (H - 1)/2.)*step;
        double x = c*u - s*v, y = s*u + c*v;
        const double w = 1. + px*x + py*y;
        x /= w; y /= w;
        const double r2 = (x*x + y*y)/(focal*focal);
        x *= 1. + k1*r2; y *= 1. + k1*r2;
        b.native.push_back(cx + x + (2.*uniform() - 1.)*jitter);
        b.native.push_back(cy + y + (2.*uniform() - 1.)*jitter);
    }
    return b;
}

// clutter: anywhere in the image but within 0.5 of a step of a corner, where it would BE a corner
static void add_clutter(std::vector<double>* q, const Board& b, int n)
{
    while(n > 0)
    {
        const double x = 800.*uniform(), y = 600.*uniform();
        bool near = false;
        for(size_t k=0; k<b.native.size(); k+=2)
            if(hypot(x - b.native[k], y - b.native[k+1]) < 0.5*b.step) near = true;
        if(near) continue;
        q->push_back(x); q->push_back(y);
        n--;
    }
}

// the points in an order that says nothing: reversed, then every third moved to the front
static std::vector<double> shuffled(const std::vector<double>& q)
{
    std::vector<double> out;
    const int n = (int)q.size()/2;
    for(int pass=0; pass<3; pass++)
        for(int k=n-1-pass; k>=0; k-=3) { out.push_back(q[2*k]); out.push_back(q[2*k+1]); }
    return out;
}

static bool found_as(const std::vector<double>& q, const Board& b, bool reversed)
{
    std::vector<double> corners(2*b.W*b.H, -1.);
    if(!chessboard_grid((int)q.size()/2, q.data(), NULL, NULL, b.W, b.H, corners.data())) return false;
    const int n = b.W*b.H;
    for(int k=0; k<n; k++)
    {
        const int from = reversed ? n - 1 - k : k;
        if(corners[2*k] != b.native[2*from] || corners[2*k+1] != b.native[2*from+1]) return false;
    }
    return true;
}

static bool not_found(const std::vector<double>& q, int W, int H)
{
    std::vector<double> corners(2*W*H, -7.);
    if(chessboard_grid((int)q.size()/2, q.data(), NULL, NULL, W, H, corners.data())) return false;
    for(double c : corners) if(c != -7.) return false;          // (untouched)
    return true;
}

int main()
{
    // the refusals
    CHECK(plan_refused(640, 480, 4, 51, 7, 4096, "images must have dtype uint8 or uint16, not 4 bytes a pixel"));
    CHECK(plan_refused(640, 480, 0, 51, 7, 4096, "images must have dtype uint8 or uint16"));
    CHECK(plan_refused(31, 480, 1, 51, 7, 4096, "an image of 31 x 480 pixels is too small: at least 32 x 32"));
    CHECK(plan_refused(640, 31, 2, 51, 7, 4096, "an image of 640 x 31 pixels is too small"));
    CHECK(plan_refused(-5, 0, 1, 51, 7, 4096, "is too small"));
    CHECK(plan_refused(1 << 14, (1 << 14) + 1, 1, 51, 7, 4096, "an image of 16384 x 16385 pixels is too large: at most 268435456 pixels"));
    CHECK(plan_refused(INT32_MAX, INT32_MAX, 1, 51, 7, 4096, "is too large"));             // (no overflow on the way)
    CHECK(plan_refused(640, 480, 1, -1, 7, 4096, "threshold_256 must be in 0..255, got -1"));
    CHECK(plan_refused(640, 480, 1, 256, 7, 4096, "threshold_256 must be in 0..255, got 256"));
    CHECK(plan_refused(640, 480, 1, 51, 0, 4096, "nms_radius must be in 1..16, got 0"));
    CHECK(plan_refused(640, 480, 1, 51, 17, 4096, "nms_radius must be in 1..16, got 17"));
    CHECK(plan_refused(640, 480, 1, 51, 7, 0, "max_candidates must be in 1..65536, got 0"));
    CHECK(plan_refused(640, 480, 1, 51, 7, 65537, "max_candidates must be in 1..65536, got 65537"));
    CHECK(plan_refused(640, 480, 1, 51, 7, 4096, "640 x 480 pixels need", 1000));
    { std::string why; CHECK(!chessboard_board_ok(&why, 2, 7) && why.find("a board has 3..256 corners a side, got 2 x 7") != std::string::npos);
      CHECK(!chessboard_board_ok(&why, 10, 257)); CHECK(chessboard_board_ok(&why, 3, 256)); }

    // the plans
    const int sizes[][2] = { {32, 32}, {45, 39}, {64, 16*3}, {65, 33}, {131, 97}, {640, 480}, {6016, 4016}, {1 << 14, 1 << 14}, {32, 1 << 23}, {1 << 23, 32}, {65, 4129776} };
    for(const auto& s : sizes) for(int bpp=1; bpp<=2; bpp++) { check_plan(s[0], s[1], bpp, 4096); check_plan(s[0], s[1], bpp, 1); check_plan(s[0], s[1], bpp, 65536); }

    // the lattice
    const int    boards[][2] = { {10, 10}, {10, 7}, {4, 3} };
    const double angles[]    = { 0., 40., -40., 180. };
    int cases = 0;
    for(const auto& wh : boards) for(double angle : angles) for(int variant=0; variant<3; variant++)
    {
        const int W = wh[0], H = wh[1];
        // plain; perspective; perspective and the strongest distortion
        const double step = variant == 0 ? 31. : variant == 1 ? 38. : 26.;
        const Board b = make_board(W, H, step, angle, variant >= 1 ? 3e-4 : 0., variant >= 1 ? -2e-4 : 0., variant == 2 ? -0.5 : 0., 0.1);
        const bool reversed = angle == 180.;

        std::vector<double> q = b.native;
        add_clutter(&q, b, 30);
        CHECK(found_as(q, b, reversed));
        CHECK(found_as(shuffled(q), b, reversed));

        // a corner removed: the first, the last, one on an edge, one inside
        for(int gone : { 0, W*H - 1, W/2, (H/2)*W + W/2 })
        {
            std::vector<double> less = q;
            less.erase(less.begin() + 2*gone, less.begin() + 2*gone + 2);
            CHECK(not_found(less, W, H));
        }
        // a corner duplicated 0.4 of a step away, towards its neighbour along the row and away from the board
        for(int which : { 0, (H/2)*W + W/2 }) for(double sign : { 1., -1. })
        {
            std::vector<double> more = q;
            const double dx = b.native[2*(which+1)] - b.native[2*which], dy = b.native[2*(which+1)+1] - b.native[2*which+1];
            more.insert(more.begin(), { b.native[2*which] + sign*0.4*dx, b.native[2*which+1] + sign*0.4*dy });
            CHECK(found_as(more, b, reversed));
        }
        // only clutter
        std::vector<double> clutter(q.begin() + 2*W*H, q.end());
        CHECK(not_found(clutter, W, H));
        // the wrong board is not this one
        CHECK(not_found(q, W + 1, H));
        cases++;
    }
    CHECK(cases == 36);
    // statuses and coordinates that are not numbers are not looked at; the response orders the seeds and nothing else
    {
        const Board b = make_board(10, 7, 30., 0., 0., 0., 0., 0.);
        std::vector<double> q = b.native;
        std::vector<int32_t> status(70, 0), response(70, 5);
        q.push_back(NAN); q.push_back(3.); status.push_back(0); response.push_back(900);
        q.push_back(b.native[0] + 3.); q.push_back(b.native[1]); status.push_back(2); response.push_back(800);
        std::vector<double> corners(140);
        CHECK(chessboard_grid(72, q.data(), response.data(), status.data(), 10, 7, corners.data()));
        CHECK(memcmp(corners.data(), b.native.data(), 140*sizeof(double)) == 0);
        status[5] = 1;
        CHECK(!chessboard_grid(72, q.data(), response.data(), status.data(), 10, 7, corners.data()));
        CHECK(!chessboard_grid(0, NULL, NULL, NULL, 10, 7, corners.data()));
    }
    printf("ok\n");
    return 0;
}
