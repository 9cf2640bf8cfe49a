// TEST-ONLY stand-alone program: the host-only planning of match_feature.hip (mrcal_amd/csrc/match_plan.hpp) under the
// host sanitizers: search windows clipped at each of the four borders of image1, radius 0, a template as large as the
// image, the two "outside" statuses, the sizes that are refused, the template map against the plain expression, and the
// offsets into the pooled surface buffer for 1, 2 and 65 features. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("match_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../mrcal_amd/csrc/match_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const double IDENTITY[9] = { 1,0,0, 0,1,0, 0,0,1 };
static const int W0 = 300, H0 = 200, W1 = 100, H1 = 80;

static MatchFeaturePlan one(double x, double y, int tw, int th, int radius, const double* H01 = IDENTITY)
{
    const double q1e[2] = { x, y };
    return match_plan_feature(q1e, H01, tw, th, radius, W0, H0, W1, H1);
}

int main()
{
    // in the middle: nothing is clipped. An odd template is centred on the estimate, an even one begins half a pixel
    // to the left of it, rounded to even
    {
        const MatchFeaturePlan f = one(50., 40., 5, 7, 10);
        CHECK(f.status == MATCH_OK && f.tmin[0] == 48 && f.tmin[1] == 37);
        CHECK(f.qmin[0] == 38 && f.qmin[1] == 27 && f.cut[0] == 25 && f.cut[1] == 27 && f.out[0] == 21 && f.out[1] == 21);
        CHECK(f.qshift[0] == 38. + 50. - 48. && f.qshift[1] == 27. + 40. - 37.);
        const MatchFeaturePlan g = one(50., 40., 4, 2, 1);
        CHECK(g.status == MATCH_OK && g.tmin[0] == 48 && g.tmin[1] == 40);      // rint(48.5) = 48, rint(39.5) = 40
        CHECK(g.out[0] == 3 && g.out[1] == 3);
    }
    // clipped at the left, the top, the right, the bottom
    {
        MatchFeaturePlan f = one(4., 40., 5, 5, 10);
        CHECK(f.status == MATCH_OK && f.tmin[0] == 2 && f.qmin[0] == 0 && f.cut[0] == 2 + 10 + 5 && f.out[0] == 13 && f.out[1] == 21);
        f = one(50., 3., 5, 5, 10);
        CHECK(f.status == MATCH_OK && f.tmin[1] == 1 && f.qmin[1] == 0 && f.cut[1] == 1 + 10 + 5 && f.out[1] == 12 && f.out[0] == 21);
        f = one(95., 40., 5, 5, 10);
        CHECK(f.status == MATCH_OK && f.tmin[0] == 93 && f.qmin[0] == 83 && f.qmin[0] + f.cut[0] == W1 && f.out[0] == 13);
        f = one(50., 76., 5, 5, 10);
        CHECK(f.status == MATCH_OK && f.tmin[1] == 74 && f.qmin[1] == 64 && f.qmin[1] + f.cut[1] == H1 && f.out[1] == 12);
        // at all four at once: a radius that is larger than the image
        f = one(50., 40., 5, 5, 1 << 30);
        CHECK(f.status == MATCH_OK && f.qmin[0] == 0 && f.qmin[1] == 0 && f.cut[0] == W1 && f.cut[1] == H1 && f.out[0] == W1 - 4 && f.out[1] == H1 - 4);
    }
    // radius 0: one entry. A template as large as image1: one entry whatever the radius
    {
        MatchFeaturePlan f = one(50., 40., 5, 5, 0);
        CHECK(f.status == MATCH_OK && f.out[0] == 1 && f.out[1] == 1 && f.qmin[0] == f.tmin[0] && f.qmin[1] == f.tmin[1]);
        f = one((W1 - 1)/2., (H1 - 1)/2., W1, H1, 7);
        CHECK(f.status == MATCH_OK && f.tmin[0] == 0 && f.tmin[1] == 0 && f.cut[0] == W1 && f.cut[1] == H1 && f.out[0] == 1 && f.out[1] == 1);
    }
    // outside image1 (each side, a template that is too large, an estimate that is not a number); outside image0
    {
        CHECK(one(1., 40., 5, 5, 3).status == MATCH_OUTSIDE_IMAGE1);
        CHECK(one(50., 1., 5, 5, 3).status == MATCH_OUTSIDE_IMAGE1);
        CHECK(one(98., 40., 5, 5, 3).status == MATCH_OUTSIDE_IMAGE1);
        CHECK(one(50., 78., 5, 5, 3).status == MATCH_OUTSIDE_IMAGE1);
        CHECK(one(50., 40., 5000, 5000, 3).status == MATCH_OUTSIDE_IMAGE1);
        CHECK(one(NAN, 40., 5, 5, 3).status == MATCH_OUTSIDE_IMAGE1);
        CHECK(one(1e300, 40., 5, 5, 3).status == MATCH_OUTSIDE_IMAGE1);
        const double left[9]  = { 1,0,-47, 0,1,0, 0,0,1 }, right[9] = { 1,0,250, 0,1,0, 0,0,1 };
        const double up[9]    = { 1,0,0, 0,1,-39, 0,0,1 }, down[9]  = { 1,0,0, 0,1,160, 0,0,1 };
        const double zero[9]  = { 0,0,0, 0,0,0, 0,0,0 };
        CHECK(one(50., 40., 5, 5, 3, left).status == MATCH_OK && one(50., 40., 5, 5, 3, right).status == MATCH_OUTSIDE_IMAGE0);
        const double left1[9] = { 1,0,-49, 0,1,0, 0,0,1 };
        CHECK(one(50., 40., 5, 5, 3, left1).status == MATCH_OUTSIDE_IMAGE0);
        CHECK(one(50., 40., 5, 5, 3, up).status == MATCH_OUTSIDE_IMAGE0 && one(50., 40., 5, 5, 3, down).status == MATCH_OUTSIDE_IMAGE0);
        CHECK(one(50., 40., 5, 5, 3, zero).status == MATCH_OUTSIDE_IMAGE0);
    }
    // the map: the plain expression, rounded to float32
    {
        const double H[9] = { 0.7, 0.3, 1., -0.4, 0.95, 2., 3e-5, 4e-6, 1. };
        const MatchFeaturePlan f = one(50., 40., 3, 2, 3, H);
        CHECK(f.status == MATCH_OK);
        std::vector<float> map(2*3*2);
        match_template_map(map.data(), f, H, 3, 2);
        for(int i = 0; i < 2; i++)
            for(int j = 0; j < 3; j++)
            {
                const volatile double x = f.tmin[0] + j, y = f.tmin[1] + i;
                const volatile double a = H[0]*x, b = H[1]*y, c = H[3]*x, d = H[4]*y, e = H[6]*x, g = H[7]*y;
                const double den = (e + g) + H[8];
                CHECK(map[2*(i*3 + j)] == (float)(((a + b) + H[2])/den) && map[2*(i*3 + j) + 1] == (float)(((c + d) + H[5])/den));
            }
    }
    // the pool: every surface after the one before it, those that are not matched taking nothing
    for(int N : { 1, 2, 65 })
    {
        std::vector<double> q1e(2*N), H01(9*N);
        for(int i = 0; i < N; i++)
        {
            q1e[2*i]   = (i % 5 == 3) ? -20. : 10. + i;         // every fifth: outside image1
            q1e[2*i+1] = 40.;
            memcpy(&H01[9*i], IDENTITY, sizeof(IDENTITY));
            if(i % 7 == 5) H01[9*i + 2] = 1000.;                // every seventh: outside image0
        }
        for(int dtype = 0; dtype < 3; dtype++)
        {
            MatchPlan plan; std::string why;
            CHECK(match_plan(&plan, &why, N, q1e.data(), H01.data(), 5, 7, 20, W0, H0, W1, H1, dtype));
            CHECK((int)plan.features.size() == N);
            size_t at = 0; int tx = 0, ty = 0;
            for(int i = 0; i < N; i++)
            {
                const MatchFeaturePlan& f = plan.features[i];
                CHECK(f.status == (i % 5 == 3 ? MATCH_OUTSIDE_IMAGE1 : i % 7 == 5 ? MATCH_OUTSIDE_IMAGE0 : MATCH_OK));
                CHECK(f.offset == at);
                if(f.status != MATCH_OK) { CHECK(f.out[0] == 0 && f.out[1] == 0); continue; }
                CHECK(f.out[0] > 0 && f.out[1] > 0 && f.out[0] == f.cut[0] - 4 && f.out[1] == f.cut[1] - 6);
                CHECK(f.qmin[0] >= 0 && f.qmin[1] >= 0 && f.qmin[0] + f.cut[0] <= W1 && f.qmin[1] + f.cut[1] <= H1);
                at += (size_t)f.out[0]*f.out[1];
                if((f.out[0] + MATCH_TILE_X - 1)/MATCH_TILE_X > tx) tx = (f.out[0] + MATCH_TILE_X - 1)/MATCH_TILE_X;
                if((f.out[1] + MATCH_TILE_Y - 1)/MATCH_TILE_Y > ty) ty = (f.out[1] + MATCH_TILE_Y - 1)/MATCH_TILE_Y;
            }
            CHECK(plan.Nsurface == at && plan.tiles[0] == tx && plan.tiles[1] == ty);
            // a staged row holds what the lanes of a tile row read
            if(dtype == 0) CHECK(plan.tpitch == 2 && plan.pitch % 32 == 16 && plan.pitch >= MATCH_TILE_X/4 + plan.tpitch);
            else           CHECK(plan.tpitch == 5 && plan.pitch == MATCH_TILE_X + 4);
            CHECK(plan.lds_bytes == match_pixel_bytes(dtype)*(dtype == 0 ? 4 : 1)*((size_t)(MATCH_TILE_Y + 6)*plan.pitch + (size_t)7*plan.tpitch));
        }
    }
    // the uint8 pitch over a range of widths
    for(int tw = 1; tw <= 300; tw++)
    {
        int pitch, tpitch; size_t bytes;
        match_lds_layout(&pitch, &tpitch, &bytes, tw, 3, 0);
        CHECK(tpitch == (tw + 3)/4 && pitch % 32 == 16 && pitch >= 16 + tpitch && pitch < 16 + tpitch + 32);
    }
    // the refusals
    {
        MatchPlan plan; std::string why;
        const double q1e[2] = { 50., 40. };
        CHECK(!match_plan(&plan, &why, 1, q1e, IDENTITY, 0, 5, 3, W0, H0, W1, H1, 0) && why.find("integer > 0") != std::string::npos);
        CHECK(!match_plan(&plan, &why, 1, q1e, IDENTITY, 5, 5, -1, W0, H0, W1, H1, 0) && why.find("search_radius1") != std::string::npos);
        CHECK(!match_plan(&plan, &why, 1, q1e, IDENTITY, 5, 5, 3, W0, H0, W1, H1, 3) && why.find("uint8, uint16 or float32") != std::string::npos);
        CHECK(!match_plan(&plan, &why, -1, q1e, IDENTITY, 5, 5, 3, W0, H0, W1, H1, 0) && why.find("features") != std::string::npos);
        CHECK(!match_plan(&plan, &why, 1, q1e, IDENTITY, 5, 5, 3, 0, H0, W1, H1, 0) && why.find("cannot be matched") != std::string::npos);
        // 300 x 300 = 90000 uint8 pixels: more than 32 bits hold; as uint16 or float32: more than the LDS holds
        CHECK(!match_plan(&plan, &why, 1, q1e, IDENTITY, 300, 300, 3, 1000, 1000, 1000, 1000, 0) && why.find("exactly in 32 bits") != std::string::npos);
        CHECK(!match_plan(&plan, &why, 1, q1e, IDENTITY, 300, 300, 3, 1000, 1000, 1000, 1000, 1) && why.find("bytes of LDS") != std::string::npos);
        CHECK(!match_plan(&plan, &why, 1, q1e, IDENTITY, 300, 300, 3, 1000, 1000, 1000, 1000, 2) && why.find("bytes of LDS") != std::string::npos);
        // a template that is larger than image1 is no refusal: a status
        CHECK(match_plan(&plan, &why, 1, q1e, IDENTITY, 5000, 5000, 3, W0, H0, W1, H1, 0) && plan.features[0].status == MATCH_OUTSIDE_IMAGE1 && plan.Nsurface == 0);
        // no feature at all
        CHECK(match_plan(&plan, &why, 0, NULL, NULL, 5, 5, 3, W0, H0, W1, H1, 0) && plan.features.empty() && plan.Nsurface == 0);
    }
    printf("ok\n");
    return 0;
}
