"""The valid-intrinsics region (include/mrcal_amd.h, "regional statistics" and "valid-intrinsics region"):
RegionalStatistics and _report_regional_statistics() (csrc/regional_stats.hip), _compute_valid_intrinsics_region() and
valid_intrinsics_regions() (csrc/valid_region.hip, csrc/region_outline.cpp), is_within_valid_intrinsics_region() and
valid_intrinsics_mask() (csrc/valid_region.hip).

The checkers are in valid_region_checker.py. The statistics are compared on the x read back from the SAME resident
problem, so the comparison is of the binning and the sums alone. Bounds: count exactly; mean within 4 n 2^-53 max|x| and
the VARIANCE stdev^2 within 8 n 2^-53 max|x|^2 of the checker's, n the cell's count: the bounds of sums of n terms taken
in another order, not measured numbers. The host units (the plan, the outline) are tested in test_valid_region_host.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT, golden_case_inputs
import valid_region_checker as chk

EPS = 2.0**-53


# ------------------------------------------------------------------------------------------------ GPU: statistics
def natural_problem(amd, **kw):
    from mrcal_amd.synthetic import make_calibration_problem
    args = dict(Ncameras=3, Nframes=8, seed=3)
    args.update(kw)
    return make_calibration_problem(amd._api, **args)[0]


def crafted_problem(amd):
    """3 cameras x 12 frames. Camera 0: every corner placed by hand on a 30x20 grid of its 4000x2200 imager. Camera 1:
    a smaller imager, so that natural corners fall outside it on the right and below. Camera 2: no observations"""
    oi = natural_problem(amd, Nframes=12, seed=5)
    idx = oi["indices_frame_camintrinsics_camextrinsics"]
    keep = idx[:, 1] != 2
    oi["indices_frame_camintrinsics_camextrinsics"] = np.ascontiguousarray(idx[keep])
    obs = np.ascontiguousarray(oi["observations_board"][keep])
    oi["imagersizes"] = np.array(((4000, 2200), (2500, 1500), (4000, 2200)), dtype=np.int32)
    W, H, gw, gh = 4000, 2200, 30, 20
    cx, cy = np.linspace(0, W - 1, gw), np.linspace(0, H - 1, gh)
    rng = np.random.default_rng(9)
    mine = np.nonzero(oi["indices_frame_camintrinsics_camextrinsics"][:, 1] == 0)[0]
    q = obs[mine][..., :2].reshape(-1, 2).copy()
    w = np.abs(obs[mine][..., 2].reshape(-1)).copy()
    # the bulk: the right half of the imager only, so that the left half has cells with no corner
    q[:, 0] = rng.uniform(W/2, W + 40, q.shape[0])
    q[:, 1] = rng.uniform(-40, H + 40, q.shape[0])
    k = 0
    def place(x, y, weight=None):
        nonlocal k
        q[k] = (x, y)
        if weight is not None: w[k] = weight
        k += 1
    place(cx[3], cy[4]); place(cx[3], cy[4])                                  # cell (3,4): 2 corners exactly on the centre
    place(cx[3] + 1., cy[4] - 1., -1.)                                        # ... and an outlier, which does not count
    place(cx[5], cy[6]); place(cx[5] + 20., cy[6] - 7.); place(cx[5] - 3., cy[6] + 11.)      # cell (5,6): 3 corners
    for i in (7, 8, 9, 10, 11):                                               # exactly on the borders between cells
        place((cx[i] + cx[i + 1])/2., cy[9])
        place(cx[2], (cy[i] + cy[i + 1])/2.)
        place((cx[i] + cx[i + 1])/2., (cy[i] + cy[i + 1])/2.)
        place(np.nextafter((cx[i] + cx[i + 1])/2., 0.), cy[2])
        place(np.nextafter((cx[i] + cx[i + 1])/2., W), cy[2])
    place(-0.5, cy[1]); place(-1e-9, cy[1]); place(cx[1], -0.5)               # inside the outermost half cells, off the imager
    place(-(W - 1.)/(gw - 1)/2., cy[3]); place(cx[1], -(H - 1.)/(gh - 1)/2.)  # exactly on their outer border
    place(-500., 100.); place(W + 500., 100.); place(100., -500.); place(100., H + 500.)     # outside on every side
    place(np.nan, 100.); place(100., np.inf); place(1e300, -1e300)
    obs_mine = obs[mine]
    obs_mine[..., :2] = q.reshape(obs_mine.shape[:-1] + (2,))
    obs_mine[..., 2]  = w.reshape(obs_mine.shape[:-1])
    obs[mine] = obs_mine
    oi["observations_board"] = obs
    return oi


def single_observation_problem(amd):
    oi = natural_problem(amd, Ncameras=1, Nframes=2, seed=1)
    oi["indices_frame_camintrinsics_camextrinsics"] = np.ascontiguousarray(oi["indices_frame_camintrinsics_camextrinsics"][:1])
    oi["observations_board"] = np.ascontiguousarray(oi["observations_board"][:1])
    oi["rt_ref_frame"] = np.ascontiguousarray(oi["rt_ref_frame"][:1])
    return oi


def golden_problem(amd):
    """boards, discrete points and regularization together: only the boards are binned"""
    return golden_case_inputs(np.load(os.path.join(GOLDEN_DIR, "optimizer_callback_golden.npz")), 4)


PROBLEMS = {
    "natural":  (natural_problem, ((2, 2), (3, 2), (30, 20), (20, None))),
    "crafted":  (crafted_problem, ((30, 20), (7, None))),
    "single":   (single_observation_problem, ((30, 20), (2, 2))),
    "board2x2": (lambda amd: natural_problem(amd, Ncameras=2, Nframes=40, object_width_n=2, object_height_n=2, seed=2), ((30, 20), (3, 2))),
    "golden":   (golden_problem, ((30, 20), (2, 2))),
}


def compare_statistics(amd, oi, gw, gh):
    """RegionalStatistics of every camera against the checker, on the x of the same resident problem. Returns the
    statistics per camera"""
    from mrcal_amd.resident import Problem
    live = amd.device_buffers_live()
    with Problem(**oi) as p:
        with amd.RegionalStatistics(oi, gw, gh, problem=p) as s, amd.RegionalStatistics(oi, gw, gh, problem=p) as s2:
            x = p.x()
            Ncameras = len(oi["imagersizes"])
            got = [s.of_camera(i) for i in range(Ncameras)]
            again = [s2.of_camera(i) for i in range(Ncameras)]
    assert amd.device_buffers_live() == live
    obs = oi["observations_board"]
    xb = x[:obs[..., 0].size*2].reshape(obs.shape[:-1] + (2,))
    for icam in range(Ncameras):
        W, H = (int(v) for v in oi["imagersizes"][icam])
        # max|x| over the corners of this camera that can be in a cell at all (a corner placed at nan has x = nan, and is in none)
        with np.errstate(invalid="ignore"):
            binned = (obs[..., 2] > 0) & (np.abs(obs[..., 0] - (W - 1)/2.) < W) & (np.abs(obs[..., 1] - (H - 1)/2.) < H)
        binned[oi["indices_frame_camintrinsics_camextrinsics"][:, 1] != icam] = False
        xmax = float(np.max(np.abs(xb[binned]))) if binned.any() else 0.
        mean, stdev, count = chk.regional_statistics(x, oi["observations_board"], oi["indices_frame_camintrinsics_camextrinsics"],
                                                     icam, W, H, gw, gh)
        m, sd, n = got[icam]
        assert m.shape == mean.shape and sd.shape == mean.shape and n.shape == mean.shape
        assert np.array_equal(n, count), f"camera {icam}: the counts differ in {np.count_nonzero(n != count)} cells"
        err_mean, err_var = np.abs(m - mean), np.abs(sd*sd - stdev*stdev)
        print(f"camera {icam} grid {gw}x{gh}: max count {count.max()}, max |mean - checker| {err_mean.max():.3g}, "
              f"max |var - checker| {err_var.max():.3g}, max|x| {xmax:.3g}")
        assert np.all(err_mean <= 4*count*EPS*xmax)
        assert np.all(err_var <= 8*count*EPS*xmax*xmax)
        assert np.all(m[count <= 5] == 0) and np.all(sd[count <= 5] == 0)
        # the same bits on two calls
        for a, b in zip(got[icam], again[icam]): assert np.array_equal(a, b)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_regional_statistics_against_the_checker(amd, name):
    make, grids = PROBLEMS[name]
    oi = make(amd)
    for gw, gh in grids:
        got = compare_statistics(amd, oi, gw, gh)
        counts = [g[2] for g in got]
        if name == "natural" and (gw, gh) == (2, 2):
            # more entries a cell than one wavefront's 64 lanes, from more than one chunk of 2048 corners
            assert max(c.max() for c in counts) > 2*64 and oi["observations_board"][..., 0].size > 2048
        if name == "crafted" and (gw, gh) == (30, 20):
            c = counts[0]
            assert c[4, 3] == 4 and c[6, 5] == 6 and c[:, :14].min() == 0            # 2 corners (zeroed), 3 (kept), none
            assert got[0][0][4, 3] == 0 and got[0][1][4, 3] == 0 and got[0][1][6, 5] > 0
            assert counts[2].max() == 0                                              # the camera without observations
            assert counts[1].max() > 5
        if name == "single":
            assert sum(int(c.sum()) for c in counts) <= 2*100 and counts[0].sum() > 0


@pytest.mark.gpu
def test_regional_statistics_one_shot_and_refusals(amd):
    oi = natural_problem(amd)
    live = amd.device_buffers_live()
    model = amd.cameramodel(optimization_inputs=oi, icam_intrinsics=1)
    with amd.RegionalStatistics(oi, 20) as s:
        assert s.grid_of_camera(1) == (20, 11)
        resident = s.of_camera(1)
    mean, stdev, count, using = amd.calibration._report_regional_statistics(model, gridn_width=20)
    for a, b in zip(resident, (mean, stdev, count)): assert np.array_equal(a, b)
    assert using == '($1*{}):($2*{}):3'.format(3999./19, 2199./10)
    with pytest.raises(Exception, match="this RegionalStatistics has been closed"):
        s.of_camera(0)
    with pytest.raises(Exception, match="gridn_width must be >= 2"):
        amd.RegionalStatistics(oi, 1)
    with pytest.raises(Exception, match="gridn_height must be >= 2"):
        amd.RegionalStatistics(oi, 20, 1)
    with pytest.raises(Exception, match="icam_intrinsics MUST be in"):
        with amd.RegionalStatistics(oi, 4) as s3: s3.of_camera(3)
    noboards = dict(oi, observations_board=None, indices_frame_camintrinsics_camextrinsics=None)
    with pytest.raises(Exception, match="no board observations"):
        amd.RegionalStatistics(noboards, 20)
    assert amd.device_buffers_live() == live


def test_measurement_selections_on_the_host(amd):
    """measurements_board() / measurements_point() are numpy selections: no GPU with x given"""
    oi = golden_problem(amd)
    oi["observations_board"][0, 1, 2, 2] = -1.              # an outlier
    Nb = amd.num_measurements_boards(**oi)
    Np = amd.num_measurements_points(**oi)
    x = np.arange(amd.num_measurements(**oi), dtype=float)
    obs = oi["observations_board"]
    got, q = amd.measurements_board(oi, x=x, return_observations=True)
    keep = obs[..., 2] > 0
    assert np.array_equal(got, x[:Nb].reshape(obs.shape[:-1] + (2,))[keep]) and np.array_equal(q, obs[keep][:, :2])
    assert 0 < got.shape[0] < obs[..., 0].size
    cam1 = amd.measurements_board(oi, x=x, icam_intrinsics=1)
    assert np.array_equal(cam1, amd.residuals_board(oi, residuals=x, i_cam=1)) and 0 < cam1.shape[0] < got.shape[0]
    pts = amd.measurements_point(oi, x=x)
    i0 = amd.measurement_index_points(0, **oi)
    Nobs = len(oi["observations_point"])
    assert pts.shape == (int(np.count_nonzero(oi["observations_point"][:, 2] > 0)), 2)
    assert np.array_equal(pts, x[i0:i0 + Np].reshape(Nobs, -1)[:, :2][oi["observations_point"][:, 2] > 0])
    assert np.array_equal(amd.residuals_point(oi, residuals=x, icam_intrinsics=0), amd.measurements_point(oi, x=x, icam_intrinsics=0))
    empty = dict(oi, observations_board=None, observations_point=None)
    assert amd.measurements_board(empty, x=x).shape == (0, 2) and amd.measurements_point(empty, x=x).shape == (0, 2)


# ------------------------------------------------------------------------------------------------ GPU: the region
@pytest.fixture(scope="module")
def solved_models(amd):
    from mrcal_amd.synthetic import make_calibration_problem
    oi, _ = make_calibration_problem(amd._api, Ncameras=3, Nframes=8, object_width_n=8, object_height_n=7, seed=3)
    amd.optimize(**oi)
    return [amd.cameramodel(optimization_inputs=oi, icam_intrinsics=i) for i in range(3)]


def region_thresholds(amd, model, parameters=(1, 0.5, 1.5, 3, 0)):
    oi = model.optimization_inputs()
    sigma = np.std(amd.measurements_board(oi).ravel())
    return [parameters[0]*sigma, parameters[1], parameters[2]*sigma, parameters[3]]


def check_region(amd, model, distance, gw=30):
    splined = model.intrinsics()[0].startswith("LENSMODEL_SPLINED_")
    W, H = (int(v) for v in model.imagersize())
    gh = chk.grid_height(gw, None, W, H)
    t = region_thresholds(amd, model)
    with amd.ProjectionUncertainty(model) as u, amd.RegionalStatistics(model.optimization_inputs(), gw, gh) as s:
        q = amd.sample_imager(gw, gh, W, H)
        v = amd.unproject(q, *model.intrinsics(), normalize=True)
        expected_u = u.evaluate(v if distance <= 0 else v*distance, atinfinity=distance <= 0, what='worstdirection-stdev')
        finite = expected_u[np.isfinite(expected_u)]
        # the uncertainty threshold scaled to the data, so that the mask is neither empty nor full
        t[0] = float(np.median(finite))
        if splined: t[3] = 1e9                       # would empty the mask if a splined model looked at the counts
        stats = s.of_camera(model.icam_intrinsics())
        contour, d = amd.calibration._compute_valid_intrinsics_region(model, *t, distance, gw, None,
                                                                      uncertainty=u, statistics=s, return_details=True)
        alone = amd.calibration._compute_valid_intrinsics_region(model, *t, distance, gw)
    assert np.array_equal(d['uncertainty'], expected_u, equal_nan=True)
    for a, b in zip(stats, (d['mean'], d['stdev'], d['count'])): assert np.array_equal(a, b)
    mask = chk.mask_rule(d['uncertainty'], d['mean'], d['stdev'], d['count'], t, splined)
    assert d['mask'].dtype == np.uint8 and np.array_equal(d['mask'], mask)
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(contour, chk.contour_of_mask(mask, W, H)) and np.array_equal(contour, alone)
    if contour.shape[0]:
        assert contour.dtype == np.int32 and np.array_equal(contour[0], contour[-1]) and contour.shape[0] >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (0, 5))
def test_region_of_a_solved_synthetic_camera(amd, solved_models, distance):
    check_region(amd, solved_models[0], distance, gw=12)


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (0, 5))
@pytest.mark.parametrize("name", ("real_opencv8-0", "real_splined-0"))
def test_region_of_a_real_camera(amd, name, distance):
    check_region(amd, amd.cameramodel(os.path.join(GOLDEN_DIR, name + ".cameramodel")), distance, gw=20)


@pytest.mark.gpu
def test_valid_intrinsics_regions_of_one_solve(amd, solved_models, tmp_path, capsys):
    models = [amd.cameramodel(m) for m in solved_models]
    live = amd.device_buffers_live()
    regions = amd.valid_intrinsics_regions(models, parameters=(1000, 0.5, 1.5, 3, 0), gridn_width=12)
    assert amd.device_buffers_live() == live
    for i, (m, r) in enumerate(zip(models, regions)):
        assert r is not None and np.array_equal(m.valid_intrinsics_region(), r)
        t = region_thresholds(amd, m, (1000, 0.5, 1.5, 3, 0))
        assert np.array_equal(r, amd.calibration._compute_valid_intrinsics_region(m, *t, 0, 12))
        path = str(tmp_path / f"camera{i}.cameramodel")
        m.write(path)
        assert np.array_equal(amd.cameramodel(path).valid_intrinsics_region(), r)
    assert any(r.shape[0] >= 4 for r in regions)
    # a camera made to fail: a warning, and no region
    class Failing(amd.cameramodel):
        def intrinsics(self, *a, **kw):
            if not a and not kw and getattr(self, "fail", False): raise Exception("made to fail")
            return super().intrinsics(*a, **kw)
    models = [amd.cameramodel(solved_models[0]), Failing(solved_models[1])]
    models[1].fail = True
    capsys.readouterr()
    regions = amd.valid_intrinsics_regions(models, parameters=(1000, 0.5, 1.5, 3, 0), gridn_width=12)
    assert regions[0] is not None and regions[1] is None and models[1].valid_intrinsics_region() is None
    assert "WARNING: Couldn't compute valid-intrinsics region for camera 1" in capsys.readouterr().err


# --------------------------------------------------------------------------------------------- GPU: applying one
POLYGONS = {
    "convex":            [(5, 4), (50, 6), (58, 30), (30, 44), (8, 35)],
    "concave":           [(4, 4), (60, 4), (60, 44), (32, 20), (4, 44)],
    "spur":              [(10, 10), (40, 10), (40, 20), (55, 20), (40, 20), (40, 40), (10, 40)],
    "vertex on a pixel": [(20, 5), (45, 25), (20, 45), (3, 25)],
    "pixels on edges":   [(8, 8), (56, 8), (56, 40), (32, 16), (8, 40)],
}


def model_with_region(amd, vertices, W=64, H=48):
    m = amd.cameramodel(intrinsics=("LENSMODEL_PINHOLE", np.array((50., 50., (W - 1)/2., (H - 1)/2.))), imagersize=(W, H))
    if vertices is not None:
        m.valid_intrinsics_region(np.array(vertices, dtype=float).reshape(-1, 2))
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POLYGONS))
def test_mask_of_a_region_at_every_pixel(amd, name):
    m = model_with_region(amd, POLYGONS[name])
    closed = m.valid_intrinsics_region().astype(int).tolist()
    expected = np.array([[chk.inside_exact(x, y, closed) for x in range(64)] for y in range(48)], dtype=np.uint8)
    mask = amd.valid_intrinsics_mask(m)
    assert mask.dtype == np.uint8 and mask.shape == (48, 64) and np.array_equal(mask, expected)
    assert 0 < expected.sum() < expected.size
    on_border = sum(1 for y in range(48) for x in range(64)
                    if not expected[y, x] and chk.distance_to_edges(np.array(((x, y),), dtype=float), closed)[0] == 0)
    assert on_border > 0
    q = np.stack(np.meshgrid(np.arange(20, 25), np.arange(7, 46, 16)), axis=-1).astype(float)        # (3,5,2)
    within = amd.is_within_valid_intrinsics_region(q, m)
    assert within.dtype == bool and within.shape == (3, 5)
    assert np.array_equal(within, expected[q[..., 1].astype(int), q[..., 0].astype(int)].astype(bool))


@pytest.mark.gpu
def test_points_off_the_pixel_grid_and_the_edge_cases(amd):
    m = model_with_region(amd, POLYGONS["concave"])
    closed = m.valid_intrinsics_region()
    rng = np.random.default_rng(3)
    candidates = rng.uniform((-5, -5), (69, 53), size=(10100, 2))
    far = chk.distance_to_edges(candidates, closed) > 1e-6
    assert np.count_nonzero(~far) < 0.01*candidates.shape[0]
    q = candidates[far][:10000]
    assert q.shape[0] == 10000
    got = amd.is_within_valid_intrinsics_region(q, m)
    expected = chk.inside_float(q, closed)
    assert np.array_equal(got, expected) and 0.2 < expected.mean() < 0.8
    # no region: None. An empty region: nothing is inside
    assert amd.is_within_valid_intrinsics_region(q, model_with_region(amd, None)) is None
    assert amd.valid_intrinsics_mask(model_with_region(amd, None)) is None
    empty = model_with_region(amd, np.zeros((0, 2)))
    assert not amd.is_within_valid_intrinsics_region(q, empty).any() and amd.is_within_valid_intrinsics_region(q, empty).shape == (10000,)
    assert amd.valid_intrinsics_mask(empty).shape == (48, 64) and not amd.valid_intrinsics_mask(empty).any()
    assert amd.is_within_valid_intrinsics_region(np.zeros((0, 2)), m).shape == (0,)
    # more vertices than are kept in LDS: a saw-toothed band
    limit = amd._lib.lib.mrcal_amd_valid_region_lds_vertices()
    assert limit == 4096
    n = limit + 50
    top = [(2*i, 10 + 6*(i % 2)) for i in range(n)]
    big = top + [(2*(n - 1), 900), (0, 900)]
    mb = model_with_region(amd, big, W=2*n, H=1000)
    closed = mb.valid_intrinsics_region().astype(int).tolist()
    assert len(closed) > limit
    qi = np.stack((rng.integers(0, 2*n, 300), rng.integers(0, 40, 300)), axis=-1).astype(float)
    expected = np.array([chk.inside_exact(x, y, closed) for x, y in qi])
    assert np.array_equal(amd.is_within_valid_intrinsics_region(qi, mb), expected) and 0.2 < expected.mean() < 0.9
