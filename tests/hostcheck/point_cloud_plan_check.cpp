// TEST-ONLY stand-alone program: the host-only planning of point_cloud.hip (mrcal_amd/csrc/point_cloud_plan.hpp) under
// the host sanitizers: every refusal with its message, the offsets of the parts of the pooled allocation (in order,
// none overlapping the next, the last one ending the pool), the grids and the counts from 1 x 1 to 2^28 pixels, that the
// scan of the counts fits its one workgroup at the largest size, how the output buffers grow, and what just fits the
// free device memory and what does not. Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("point_cloud_plan_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../mrcal_amd/csrc/point_cloud_plan.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static const size_t PLENTY = (size_t)1 << 40;

static bool words_are(const std::string& why, const char* words)
{
    return why.find("stereo_point_cloud():") == 0 && why.find(words) != std::string::npos;
}

static bool plan_refused(int W, int H, const char* words, size_t free_bytes = PLENTY)
{
    CloudPlan plan; std::string why;
    if(cloud_plan(&plan, &why, W, H, free_bytes)) return false;
    if(plan.bytes != 0 || plan.groups != 0 || plan.scan_per_thread != 0) return false;      // (a refusal leaves no plan)
    return words_are(why, words);
}

static bool params_refused(long dmin, long dmax, double rmin, double rmax, bool have_map, int iw, int ih, int channels, int bytes,
                           const char* words)
{
    std::string why;
    return !cloud_params_ok(&why, dmin, dmax, rmin, rmax, have_map, iw, ih, channels, bytes) && words_are(why, words);
}

int main()
{
    // the refusals
    {
        CHECK(plan_refused(0, 80, "a disparity image of 0 x 80 pixels cannot be made a cloud of"));
        CHECK(plan_refused(100, -1, "a disparity image of 100 x -1 pixels cannot be made a cloud of"));
        CHECK(plan_refused(1 << 15, (1 << 13) + 1, "at most 268435456 pixels"));       // 2^28 + 2^15 pixels
        CHECK(plan_refused(INT32_MAX, INT32_MAX, "cannot be made a cloud of"));        // (no overflow on the way)
        CHECK(params_refused(5, 5, 0., INFINITY, false, 0, 0, 0, 0, "must have disparity_scaled_max > disparity_scaled_min. Got 5 and 5"));
        CHECK(params_refused(6, 5, 0., INFINITY, false, 0, 0, 0, 0, "Got 5 and 6"));
        CHECK(params_refused(0, 5, 2., 1., false, 0, 0, 0, 0, "must have range_min <= range_max. Got 2 and 1"));
        CHECK(params_refused(0, 5, NAN, 1., false, 0, 0, 0, 0, "must have range_min <= range_max"));
        CHECK(params_refused(0, 5, 0., NAN, false, 0, 0, 0, 0, "must have range_min <= range_max"));
        CHECK(params_refused(0, 5, 0., 1., true, 10, 10, 2, 1, "a colour image has 1 or 3 channels, not 2"));
        CHECK(params_refused(0, 5, 0., 1., true, 10, 10, -1, 1, "a colour image has 1 or 3 channels, not -1"));
        CHECK(params_refused(0, 5, 0., 1., true, 10, 10, 3, 4, "a colour image is uint8 or uint16"));
        CHECK(params_refused(0, 5, 0., 1., true, 10, 10, 1, 0, "a colour image is uint8 or uint16"));
        CHECK(params_refused(0, 5, 0., 1., true, 0, 10, 1, 1, "a colour image of 0 x 10 pixels cannot be read"));
        CHECK(params_refused(0, 5, 0., 1., true, 1 << 24, 1, 1, 1, "cannot be read"));
        CHECK(params_refused(0, 5, 0., 1., true, 1 << 16, 1 << 15, 1, 1, "cannot be read"));    // 2^31 pixels
        CHECK(params_refused(0, 5, 0., 1., false, 10, 10, 3, 2, "a colour image needs the rectification map of camera 0"));
        // ... and what is just inside is not
        std::string why;
        CHECK(cloud_params_ok(&why, 0, 1, 0., 0., false, 0, 0, 0, 0));
        CHECK(cloud_params_ok(&why, 0, 0xFFFF, 0., INFINITY, true, (1 << 24) - 1, 1, 3, 2));
        CHECK(cloud_params_ok(&why, 16, 0x7FFF, 1.5, 1.5, true, 1 << 15, 1 << 15, 1, 1));       // 2^30 pixels
    }
    // the pool and the grids, at the sizes where a span is just full or just not
    const int sizes[][2] = { { 1, 1 }, { 9, 7 }, { 63, 8 }, { 64, 9 }, { 65, 10 }, { 17, 64 }, { 130, 65 }, { 131, 130 },
                             { 1023, 1 }, { 1024, 1 }, { 1025, 1 }, { 1, 1024 }, { 1024, 1024 }, { 1024, 1025 }, { 1024*1024 + 1, 1 },
                             { 1024, 768 }, { 6016, 4016 }, { 1, 1 << 28 }, { 1 << 28, 1 }, { 1 << 14, 1 << 14 }, { (1 << 28) - 1, 1 } };    // (W,H)
    for(const auto& size : sizes)
    {
        const int W = size[0], H = size[1];
        CloudPlan plan; std::string why;
        CHECK(cloud_plan(&plan, &why, W, H, PLENTY));
        CHECK(plan.W == W && plan.H == H);
        const size_t N = (size_t)W*H;
        // every pixel is in one workgroup's span, and no workgroup is idle; every word of a workgroup exists
        CHECK((size_t)plan.groups*CLOUD_SPAN >= N && (size_t)(plan.groups - 1)*CLOUD_SPAN < N);
        CHECK((size_t)plan.groups*CLOUD_WORDS_PER_GROUP*64 >= N);
        // the scan: every count is some thread's, a thread sums no more than it may, and no thread's share is wasted
        CHECK((size_t)plan.scan_per_thread*CLOUD_SCAN_THREADS >= plan.groups);
        CHECK(plan.scan_per_thread >= 1 && plan.scan_per_thread <= CLOUD_SCAN_MAX_PER_THREAD);
        CHECK((size_t)(plan.scan_per_thread - 1)*CLOUD_SCAN_THREADS < plan.groups);
        CHECK((size_t)(CLOUD_SCAN_THREADS - 1)*plan.scan_per_thread <= UINT32_MAX);     // (the first count of the last thread)
        // the parts in order, what each needs, each aligned
        CHECK(plan.disparity == 0);
        CHECK(plan.words % CLOUD_ALIGN == 0 && plan.counts % CLOUD_ALIGN == 0 && plan.bases % CLOUD_ALIGN == 0 && plan.bytes % CLOUD_ALIGN == 0);
        CHECK(plan.disparity + N*2 <= plan.words && plan.words - plan.disparity < N*2 + CLOUD_ALIGN);
        CHECK(plan.words + (size_t)plan.groups*CLOUD_WORDS_PER_GROUP*8 <= plan.counts);
        CHECK(plan.counts - plan.words < (size_t)plan.groups*CLOUD_WORDS_PER_GROUP*8 + CLOUD_ALIGN);
        CHECK(plan.counts + (size_t)plan.groups*4 <= plan.bases && plan.bases - plan.counts < (size_t)plan.groups*4 + CLOUD_ALIGN);
        CHECK(plan.bases + ((size_t)plan.groups + 1)*4 <= plan.bytes && plan.bytes - plan.bases < ((size_t)plan.groups + 1)*4 + CLOUD_ALIGN);
        // an index and a rank fit 31 bits
        CHECK(N <= (size_t)INT32_MAX && (size_t)plan.groups*CLOUD_SPAN <= (size_t)INT32_MAX);
        // what does not fit is refused with its size; what just fits is not
        CHECK(cloud_plan(&plan, &why, W, H, plan.bytes));
        const size_t bytes = plan.bytes;
        char size_words[128];
        snprintf(size_words, sizeof(size_words), "%d x %d pixels need %zu bytes of device memory; %zu are free", W, H, bytes, bytes - 1);
        CHECK(plan_refused(W, H, size_words, bytes - 1));
        CHECK(plan_refused(W, H, "are free", 0));
    }
    // the largest image: the scan's one workgroup is exactly full, and the total fits the uint32 it is summed in
    {
        CloudPlan plan; std::string why;
        CHECK(cloud_plan(&plan, &why, 1 << 14, 1 << 14, PLENTY));
        CHECK(plan.groups == (1u << 18) && plan.scan_per_thread == CLOUD_SCAN_MAX_PER_THREAD);
        CHECK((size_t)plan.groups*CLOUD_SPAN == (size_t)CLOUD_MAX_PIXELS && (size_t)CLOUD_MAX_PIXELS < (size_t)UINT32_MAX);
    }
    // the real calibration's size: a bit a pixel is 3 MB, the disparities 48
    {
        CloudPlan plan; std::string why;
        CHECK(cloud_plan(&plan, &why, 6016, 4016, PLENTY));
        const size_t N = (size_t)6016*4016;
        CHECK(plan.counts - plan.words >= N/8 && plan.counts - plan.words < N/8 + CLOUD_SPAN/8 + CLOUD_ALIGN);
        CHECK(plan.bytes < 2*N + N/8 + N/100);
    }
    // the capacity of the output buffers
    {
        const size_t pixels = (size_t)6016*4016;
        CHECK(cloud_capacity(0, 0, pixels) == 0);                                   // an empty cloud needs nothing
        CHECK(cloud_capacity(0, 1, pixels) == CLOUD_CAPACITY_STEP);
        CHECK(cloud_capacity(4096, 4096, pixels) == 4096);                          // what fits stays
        CHECK(cloud_capacity(4096, 17, pixels) == 4096);                            // ... and never shrinks
        CHECK(cloud_capacity(4096, 4097, pixels) == 2*CLOUD_CAPACITY_STEP);         // 4097 + 1024 -> 8192
        CHECK(cloud_capacity(8192, 100000, pixels) == 126976);                      // 125000 -> 31 steps
        CHECK(cloud_capacity(0, pixels, pixels) == pixels);                         // never beyond the image
        CHECK(cloud_capacity(0, pixels - 1, pixels) == pixels);
        CHECK(cloud_capacity(0, 1, 1) == 1 && cloud_capacity(0, 63, 63) == 63 && cloud_capacity(1, 1, 1) == 1);
        for(size_t have : { (size_t)0, (size_t)4096, (size_t)1 << 20 })
            for(size_t N = 0; N <= pixels; N += 99991)
            {
                const size_t c = cloud_capacity(have, N, pixels);
                CHECK(c >= N && c >= have && (c <= pixels || c == have));
                CHECK(c == have || c == pixels || (c % CLOUD_CAPACITY_STEP == 0 && c < N + N/4 + CLOUD_CAPACITY_STEP));
            }
    }
    printf("ok\n");
    return 0;
}
