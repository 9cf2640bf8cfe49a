// TEST-ONLY stand-alone program: what is decided about a raw image before any device work (mrcal_amd/csrc/image_format.hpp
// and ImagePreparation::ok() of mrcal_amd/csrc/image_prepare.hpp) under the host sanitizers: the bytes of a pixel, the
// largest image, and every refusal in its words and its order, the equalization first, then the anti-aliasing filter on
// the type the equalization leaves. The words are those the Python tests pin (tests/test_equalization.py,
// tests/test_smooth.py, tests/test_smooth_host.py). Not a product path, and nothing loads it into Python.
//
//   built by tests/hostbuild.py, build_program("image_prepare_check"): a row of its PROGRAMS. No arguments
//   (prints "ok"; a sanitizer report or a failed check ends it with a non-zero status)
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "../../mrcal_amd/csrc/image_prepare.hpp"

using namespace mrcal_amd;

#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while(0)

static ImagePreparation preparation(int method, double sigma_x, double sigma_y)
{
    ImagePreparation p;
    p.equalization.method = method;
    p.antialias.sigma_x = sigma_x; p.antialias.sigma_y = sigma_y;
    return p;
}

// ok() says no in exactly these words; words NULL: it says yes, and nothing else
static bool says(const ImagePreparation& p, int W, int H, int C, int dtype, const char* words)
{
    std::string why;
    const bool ok = p.ok(&why, W, H, C, dtype);
    if(words != NULL && why != words) fprintf(stderr, "refused with '%s'\n", why.c_str());
    return words == NULL ? ok && why.empty() : !ok && why == words;
}

int main()
{
    CHECK(image_pixel_bytes(IMAGE_DTYPE_UINT8) == 1 && image_pixel_bytes(IMAGE_DTYPE_UINT16) == 2 && image_pixel_bytes(IMAGE_DTYPE_FLOAT) == 4);
    CHECK(image_dtype_is_integer(IMAGE_DTYPE_UINT8) && image_dtype_is_integer(IMAGE_DTYPE_UINT16) && !image_dtype_is_integer(IMAGE_DTYPE_FLOAT));
    // IMAGE_MAX_PIXELS pixels, and one more
    CHECK(IMAGE_MAX_PIXELS == 268435456L && image_size_ok(1 << 14, 1 << 14) && image_size_ok(1 << 28, 1) && image_size_ok(1, 1 << 28));
    CHECK(!image_size_ok((1 << 28) + 1, 1) && !image_size_ok((1 << 14) + 1, 1 << 14) && !image_size_ok(INT32_MAX, INT32_MAX));
    CHECK(!image_size_ok(0, 5) && !image_size_ok(5, 0) && !image_size_ok(-1, -1));

    const ImagePreparation off;
    const ImagePreparation clahe = preparation(EQUALIZE_METHOD_CLAHE, 0, 0), stretch = preparation(EQUALIZE_METHOD_STRETCH, 0, 0);
    const ImagePreparation filter = preparation(EQUALIZE_METHOD_NONE, 2, 0), both = preparation(EQUALIZE_METHOD_STRETCH, 0.5, 8);
    CHECK(off.off() && !clahe.off() && !stretch.off() && !filter.off() && !both.off());

    // everything off: whatever the remap takes, and the type stays
    for(int C : { 1, 3 })
        for(int dtype : { IMAGE_DTYPE_UINT8, IMAGE_DTYPE_UINT16, IMAGE_DTYPE_FLOAT })
            CHECK(says(off, 3, 5, C, dtype, NULL) && off.dtype_out(dtype) == dtype);
    // the equalization: grey uint8 or uint16 images that the tiles fit
    CHECK(says(clahe, 64, 48, 1, IMAGE_DTYPE_UINT16, NULL) && clahe.dtype_out(IMAGE_DTYPE_UINT16) == IMAGE_DTYPE_UINT16);
    CHECK(says(clahe, 64, 48, 3, IMAGE_DTYPE_UINT8, "equalize(): an image that is equalized is grey, not of 3 channels"));
    CHECK(says(clahe, 64, 48, 1, IMAGE_DTYPE_FLOAT, "equalize(): images are uint8 or uint16"));
    CHECK(says(clahe, 3, 5, 1, IMAGE_DTYPE_UINT8,
               "equalize(): an image of 3 x 5 pixels is too small for (8,8) tiles: it would be padded by (5,3) pixels, and a reflection reaches (2,4)"));
    CHECK(says(stretch, 3, 5, 1, IMAGE_DTYPE_UINT8, NULL));
    CHECK(says(stretch, 16384, 16384, 1, IMAGE_DTYPE_UINT8, NULL));
    CHECK(says(stretch, 16385, 16384, 1, IMAGE_DTYPE_UINT8, "equalize(): images of 16385 x 16384 pixels cannot be equalized"));
    // the filter: grey uint8 or uint16 images
    CHECK(says(filter, 30, 20, 1, IMAGE_DTYPE_UINT16, NULL));
    CHECK(says(filter, 30, 20, 3, IMAGE_DTYPE_UINT8, "smooth(): an image that is filtered is grey, not of 3 channels"));
    CHECK(says(filter, 30, 20, 1, IMAGE_DTYPE_FLOAT, "smooth(): images are uint8 or uint16"));
    CHECK(says(filter, 16384, 16384, 1, IMAGE_DTYPE_UINT8, NULL));
    CHECK(says(filter, 16385, 16384, 1, IMAGE_DTYPE_UINT8, "smooth(): images of 16385 x 16384 pixels cannot be smoothed"));
    // ... of the type the equalization leaves: after a stretch of a uint16 image the filter sees uint8
    CHECK(says(both, 30, 20, 1, IMAGE_DTYPE_UINT16, NULL) && both.dtype_out(IMAGE_DTYPE_UINT16) == IMAGE_DTYPE_UINT8);
    // both on: the equalization speaks first
    CHECK(says(both, 30, 20, 3, IMAGE_DTYPE_UINT8, "equalize(): an image that is equalized is grey, not of 3 channels"));
    CHECK(says(both, 30, 20, 1, IMAGE_DTYPE_FLOAT, "equalize(): images are uint8 or uint16"));
    printf("ok\n");
    return 0;
}
