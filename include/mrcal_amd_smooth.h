/* mrcal_amd: the anti-aliasing Gaussian pre-filter, and the remaps that apply it first.

   A header of its own beside mrcal_amd.h, which it includes and whose conventions it keeps: bool results, false with
   the reason in mrcal_amd_last_error(); images dense, MRCAL_AMD_IMAGE_UINT8 or _UINT16 here.

   ---- smoothing: a separable Gaussian of a grey image, before it is remapped to fewer pixels ----
   A remap reads 4 pixels of its source for a pixel of its result, whatever the scale: one that makes the image 3-8 x
   smaller, as the rectification of a large pair to the matcher's disparity range does, drops most of the image and
   aliases the rest. The reference's to-do list has the entry (doc/news-3.0.org: "mrcal-stereo should have an
   anti-aliasing filter ... when I downsample, just before mrcal.transform_image()", with cv2.GaussianBlur(sigmaX = 2)),
   which it never built. Here it is csrc/smooth.hip, planned on the host by csrc/smooth_plan.hpp. cv2 is no part of
   this project and no equality with cv2.GaussianBlur() is claimed: this text is the authority, and
   tests/smooth_checker.py restates it twice.

   The image: grey, dense (H,W), uint8 or uint16; the result has its shape and type. sigma_x, sigma_y: each is 0 (that
   axis is not filtered) or lies in [0.5, 8].
   Taps, per axis, from its sigma:
     1. R = ceil(3 sigma), so R <= 24; g_k = exp(-k^2 / (2 sigma^2)) for k = 0..R, in double
     2. S = g_0 + 2 sum_{k>=1} g_k; a_k = 256 g_k / S
     3. integer weights by error diffusion from the outside in: e = 0; for k = R, R-1, ..., 1:
        w_k = floor(a_k + e + 0.5), then e += a_k - w_k. Last w_0 = 256 - 2 sum_{k>=1} w_k, and w_-k = w_k
     4. sigma = 0: the single tap w_0 = 256
   They sum to 256, 0 <= w_k <= 255 for every sigma in [0.5, 8], and |w_k - a_k| <= 1; above sigma ~ 3.3 they are not
   monotone in k: eight bits are too coarse for that.
   Arithmetic: integers only; a coordinate outside the image is clamped to it (the border is replicated).
     horizontal   T[y][x] = sum_k wx_k I[y][clamp(x + k)]                         no rounding, no shift
     vertical     O[y][x] = (sum_k wy_k T[clamp(y + k)][x] + 32768) >> 16
   The largest value, of a uint16 image, is 65535 256 256 + 32768 = 2^32 - 32768: an unsigned 32-bit accumulator holds
   it. A constant image comes back unchanged. No floating point on the device and no atomics: the same bits on every
   call.
   Refused: a sigma that is neither 0 nor in [0.5, 8] (a NaN is neither), both sigmas 0 (there is nothing to run), a type
   that is neither uint8 nor uint16, an image that is empty or has more than 2^28 pixels, an image that does not fit
   the free device memory.
   _create(): the handle owns ONE device allocation: the image and the result. _apply(): host arrays, dense.
   _milliseconds(): how long the one launch of the last _apply() took on the device, without the copies.
   mrcal_amd_smooth_weights(): R and w_0..w_R of one sigma (0, or > 0 with R <= 24), on the host: no device is needed.
   mrcal_amd_rectification_set_antialias(): NULL or both sigmas 0 (what a new handle has): nothing of this runs and
   every result is what it was. Otherwise every later _rectify(), _disparity(), _disparity_filtered() and
   _point_cloud_of_images() filters each raw image on the device, after its upload and after its equalization if one is
   set, before the remap; the images are then grey, uint8 or uint16. The colours of _point_cloud_of_images() are NOT
   filtered: they come from the image as it was before the filter.
   mrcal_amd_transform_image_smoothed(): mrcal_amd_transform_image() of the image filtered so, on the device between the
   upload and the remap; params NULL or both sigmas 0: mrcal_amd_transform_image() */
#pragma once
#include "mrcal_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct
{
    double sigma_x, sigma_y;    /* each 0, or in [0.5, 8] */
} mrcal_amd_smooth_params_t;
typedef struct mrcal_amd_smoother mrcal_amd_smoother_t;
mrcal_amd_smoother_t* mrcal_amd_smoother_create(int width, int height, int dtype, const mrcal_amd_smooth_params_t* params);
bool mrcal_amd_smoother_apply(mrcal_amd_smoother_t* s, const void* in, void* out);
bool mrcal_amd_smoother_milliseconds(mrcal_amd_smoother_t* s, float* milliseconds);
void mrcal_amd_smoother_destroy(mrcal_amd_smoother_t* s);
bool mrcal_amd_smooth_weights(double sigma, int* R, int* w /* up to 25: w_0..w_R */);
bool mrcal_amd_rectification_set_antialias(mrcal_amd_rectification_t* r, const mrcal_amd_smooth_params_t* params);
bool mrcal_amd_transform_image_smoothed(void* out, const void* image, int width, int height, int channels, int dtype,
                                        const float* mapxy, int width_out, int height_out,
                                        int interpolation, int border_mode, const double* border_value,
                                        const mrcal_amd_smooth_params_t* params);

#ifdef __cplusplus
}
#endif
