"""The host planning of the lens-model fit (csrc/lensfit_plan.hpp), without a GPU: as a stand-alone program under the host
sanitizers (tests/hostcheck/lensfit_plan_check.cpp), and through the library's mrcal_amd_lensfit_plan() - the same
function, as fit_lensmodel() calls it: for every row of the lens table, with and without the core and the pose, the
instantiation, the unknowns, the threads, the chunk and an LDS size within the limit the plan states; every refusal."""
import pytest

import hostbuild

# for_parametric_lens(), restated: (model, PROJ, NDIST). PROJ_*: csrc/lens_models.hpp
PROJ_OPENCV, PROJ_STEREOGRAPHIC, PROJ_LONLAT, PROJ_LATLON, PROJ_CAHVOR, PROJ_CAHVORE = range(6)
TABLE = (("LENSMODEL_PINHOLE", PROJ_OPENCV, 0), ("LENSMODEL_STEREOGRAPHIC", PROJ_STEREOGRAPHIC, 0),
         ("LENSMODEL_LONLAT", PROJ_LONLAT, 0), ("LENSMODEL_LATLON", PROJ_LATLON, 0),
         ("LENSMODEL_OPENCV4", PROJ_OPENCV, 4), ("LENSMODEL_OPENCV5", PROJ_OPENCV, 5), ("LENSMODEL_OPENCV8", PROJ_OPENCV, 8),
         ("LENSMODEL_OPENCV12", PROJ_OPENCV, 12), ("LENSMODEL_CAHVOR", PROJ_CAHVOR, 5),
         ("LENSMODEL_CAHVORE_linearity=0.30", PROJ_CAHVORE, 8))
SPLINED = "LENSMODEL_SPLINED_STEREOGRAPHIC_order=3_Nx=8_Ny=6_fov_x_deg=80"


def test_lensfit_plan_under_the_host_sanitizers():
    """csrc/lensfit_plan.hpp driven by a stand-alone program with its own main, built with ASan and UBSan"""
    hostbuild.assert_prints_ok("lensfit_plan_check")


@pytest.mark.parametrize("lensmodel,proj,ndist", TABLE)
def test_plan_table(amd, lensmodel, proj, ndist):
    N = 700
    for core in (True, False):
        for pose in (True, False):
            for reg in (True, False):
                NP1 = 4 + ndist - (0 if core else 4)
                NP = NP1 + (6 if pose else 0)
                kw = dict(imagersize=(4000, 2200), optimize_core=core, optimize_extrinsics=pose, do_apply_regularization=reg)
                if NP == 0:
                    with pytest.raises(Exception, match="nothing to fit"):
                        amd.fit_lensmodel_plan(lensmodel, N, **kw)
                    continue
                plan = amd.fit_lensmodel_plan(lensmodel, N, **kw)
                assert (plan["proj"], plan["ndist"], plan["Nintrinsics"]) == (proj, ndist, 4 + ndist)
                assert plan["ivar0"] == (0 if core else 4)
                assert (plan["Nstages"], plan["NP1"], plan["NP2"]) == ((2, NP1, NP) if pose else (1, NP1, 0))
                assert 1 <= NP <= 22
                assert plan["Nsums"] == (NP + 1)*(NP + 2)//2
                assert plan["threads"] % 64 == 0 and plan["Nsums"] <= plan["threads"] <= 320
                assert plan["row_doubles"] == NP + 1
                C = plan["chunk_rows"]
                assert C % 64 == 0 and 64 <= C <= 2*plan["threads"]
                assert plan["lds_limit"] == 64*1024
                assert C*(NP + 1)*8 < plan["lds_bytes"] <= plan["lds_limit"]
                assert plan["Nmeasurements"] == 2*N + (ndist if reg else 0) + (2 if reg and core else 0)


def test_plan_refusals(amd):
    with pytest.raises(Exception, match="splined model .* fitted by optimize\\(\\)"):
        amd.fit_lensmodel_plan(SPLINED, 100)
    with pytest.raises(Exception, match="Couldn't parse 'lensmodel'"):
        amd.fit_lensmodel_plan("LENSMODEL_BOGUS", 100)
    with pytest.raises(Exception, match="7 points give 14 pixel rows: fewer than the 16 unknowns"):
        amd.fit_lensmodel_plan("LENSMODEL_OPENCV12", 7)
    assert amd.fit_lensmodel_plan("LENSMODEL_OPENCV12", 8)["NP1"] == 16
    with pytest.raises(Exception, match="fewer than the 22 unknowns"):
        amd.fit_lensmodel_plan("LENSMODEL_OPENCV12", 10, optimize_extrinsics=True)
    with pytest.raises(Exception, match="nothing to fit"):
        amd.fit_lensmodel_plan("LENSMODEL_STEREOGRAPHIC", 100, optimize_core=False)
    with pytest.raises(Exception, match="0 points cannot be fitted"):
        amd.fit_lensmodel_plan("LENSMODEL_OPENCV4", 0)
    with pytest.raises(Exception, match="0 trials"):
        amd.fit_lensmodel_plan("LENSMODEL_OPENCV4", 100, Ntrials=0)
    with pytest.raises(Exception, match="an imager of 0 x 10 pixels"):
        amd.fit_lensmodel_plan("LENSMODEL_OPENCV4", 100, imagersize=(0, 10))
