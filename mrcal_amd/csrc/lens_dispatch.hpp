// Which kernels a lens model runs: mrcal_lensmodel_type_t -> the (PROJ_*, NDIST) its kernels are instantiated with.
// THE table, written once (for_parametric_lens); every launcher and the host's unprojection go through it, so a model
// cannot run another model's arithmetic at one entry point only.
//
// Host code, no HIP runtime types: the .hip units, unproject.cpp and tests/hostcheck/ can all include it.
// The splined model is not in the table: it has kernels of its own and its own branch at every site.
#pragma once
#include <string.h>
#include "lens_models.hpp"
#include "../../include/mrcal_amd.h"

namespace mrcal_amd {

// the compile-time tag a call site is handed
template<int PROJ_, int NDIST_> struct LensKernels
{
    static constexpr int  PROJ = PROJ_, NDIST = NDIST_;
    // unprojection is a formula; the others are inverted iteratively, and only they instantiate the kernels of that
    // iteration. AN INVARIANT OF THE TABLE BELOW, not a law: its rows without distortion terms (pinhole, stereographic,
    // lonlat, latlon) are exactly the ones unproject_closed_form_kernel and mrcal_unproject() have a formula for. A row
    // with NDIST = 0 and no such formula must carry the property itself instead
    static constexpr bool has_closed_form_inverse = (NDIST_ == 0);
};

// f(LensKernels<PROJ,NDIST>{}) for a parametric model: true. Anything else, the splined model included: false, f not called
template<class F> bool for_parametric_lens(int lens_type, F&& f)
{
    switch(lens_type)
    {
    case MRCAL_LENSMODEL_PINHOLE:       f(LensKernels<PROJ_OPENCV,        0 >{}); return true;
    case MRCAL_LENSMODEL_STEREOGRAPHIC: f(LensKernels<PROJ_STEREOGRAPHIC, 0 >{}); return true;
    case MRCAL_LENSMODEL_LONLAT:        f(LensKernels<PROJ_LONLAT,        0 >{}); return true;
    case MRCAL_LENSMODEL_LATLON:        f(LensKernels<PROJ_LATLON,        0 >{}); return true;
    case MRCAL_LENSMODEL_OPENCV4:       f(LensKernels<PROJ_OPENCV,        4 >{}); return true;
    case MRCAL_LENSMODEL_OPENCV5:       f(LensKernels<PROJ_OPENCV,        5 >{}); return true;
    case MRCAL_LENSMODEL_OPENCV8:       f(LensKernels<PROJ_OPENCV,        8 >{}); return true;
    case MRCAL_LENSMODEL_OPENCV12:      f(LensKernels<PROJ_OPENCV,        12>{}); return true;
    case MRCAL_LENSMODEL_CAHVOR:        f(LensKernels<PROJ_CAHVOR,        5 >{}); return true;
    case MRCAL_LENSMODEL_CAHVORE:       f(LensKernels<PROJ_CAHVORE,       8 >{}); return true;
    default:                            return false;
    }
}

// distortion parameters of a parametric model; 0 for anything else
inline int lens_ndist(int lens_type)
{
    int ndist = 0;
    for_parametric_lens(lens_type, [&](auto k) { ndist = decltype(k)::NDIST; });
    return ndist;
}
inline bool lens_has_closed_form_inverse(int lens_type)
{
    bool closed = false;
    for_parametric_lens(lens_type, [&](auto k) { closed = decltype(k)::has_closed_form_inverse; });
    return closed;
}
// the models that have kernels at all
inline bool lens_supported(int lens_type)
{
    return lens_type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC || for_parametric_lens(lens_type, [](auto) {});
}

// the model configuration that is not in the intrinsics vector
inline LensConfig lens_config_of(const mrcal_lensmodel_t& m)
{
    LensConfig cfg; memset(&cfg, 0, sizeof(cfg));
    if(m.type == MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC)
    {
        cfg.spline_order = m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.order;
        cfg.spline_Nx    = m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.Nx;
        cfg.spline_Ny    = m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.Ny;
        cfg.spline_segments_per_u =
            spline_segments_per_u(cfg.spline_order, cfg.spline_Nx,
                                  (double)m.LENSMODEL_SPLINED_STEREOGRAPHIC__config.fov_x_deg);
    }
    if(m.type == MRCAL_LENSMODEL_CAHVORE)
        cfg.cahvore_linearity = m.LENSMODEL_CAHVORE__config.linearity;
    return cfg;
}

} // namespace mrcal_amd
