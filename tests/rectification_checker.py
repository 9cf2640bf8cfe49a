"""What tests/test_stereo.py and tests/test_image_transforms.py are held against: numpy written for the tests, around the
reference's compiled mrcal_project() / mrcal_unproject() (ref_api). Nothing here calls the product"""
import numpy as np


def rotation(r):
    """Rodrigues, written out for the tests"""
    r = np.asarray(r, dtype=float)
    th = np.linalg.norm(r)
    if th < 1e-12: return np.eye(3)
    k = r/th
    K = np.array(((0, -k[2], k[1]), (k[2], 0, -k[0]), (-k[1], k[0], 0)))
    return np.eye(3) + np.sin(th)*K + (1 - np.cos(th))*(K @ K)


def grid(W, H):
    """(H,W,2) pixel coordinates (x,y)"""
    return np.ascontiguousarray(np.stack(np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float)), axis=-1))


def vectors_of_rectified_model(lensmodel, fxycxy, q):
    fx, fy, cx, cy = fxycxy
    ux, uy = (q[..., 0] - cx)/fx, (q[..., 1] - cy)/fy
    if lensmodel == "LENSMODEL_LATLON":
        return np.stack((np.sin(ux), np.cos(ux)*np.sin(uy), np.cos(ux)*np.cos(uy)), axis=-1)
    assert lensmodel == "LENSMODEL_PINHOLE"
    return np.stack((ux, uy, np.ones(ux.shape)), axis=-1)


def rectification_maps_checker(ref_api, models, models_rectified):
    """float32 (2,Nel,Naz,2): the grid vector of the rectified model, times R_cam_rect, through the reference's projection"""
    lensmodel, fxycxy = models_rectified[0].intrinsics()
    Naz, Nel = (int(x) for x in models_rectified[0].imagersize())
    v = vectors_of_rectified_model(lensmodel, fxycxy, grid(Naz, Nel))
    R_rect_ref = rotation(models_rectified[0].rt_cam_ref()[:3])
    out = []
    for m in models:
        R_cam_rect = rotation(m.rt_cam_ref()[:3]) @ R_rect_ref.T
        out.append(ref_api.project(v @ R_cam_rect.T, *m.intrinsics()))
    return np.array(out)           # float64: the caller casts


def compare_map(mine, checker64, label, max_left_out=0.01, max_unequal=1e-3):
    """The criterion of the maps, for ONE map. Entries where the checker is not finite or beyond 1e6 are left out (at most
    max_left_out of them); every other entry is equal to float32(checker) or one float32 spacing away, and at most
    max_unequal of them are unequal: in a map of fewer than a thousand entries, none. Prints what it saw"""
    assert mine.dtype == np.float32 and mine.shape == checker64.shape
    use = np.isfinite(checker64) & (np.abs(checker64) <= 1e6)
    left_out = 1. - use.mean()
    c = checker64[use].astype(np.float32)
    m = mine[use]
    unequal = float((m != c).mean()) if m.size else 0.
    spacings = np.abs(m.astype(np.float64) - c.astype(np.float64))/np.spacing(np.abs(c)).astype(np.float64)
    worst = float(spacings.max()) if m.size else 0.
    print(f"{label}: {mine.size} entries, left out {left_out:.4%}, unequal {unequal:.3e}, worst {worst:.2f} float32 spacings")
    assert left_out <= max_left_out, f"{label}: {left_out:.3%} of the checker's entries are unusable"
    assert np.all(np.isfinite(m)), f"{label}: non-finite entries where the checker is finite"
    assert worst <= 1.0, f"{label}: an entry is {worst} float32 spacings from the checker"
    assert unequal <= max_unequal, f"{label}: {unequal:.3e} of the entries differ from the checker"


def pinhole_cxy_restated(fxy, tanazel0, fov_deg, polish=False):
    """the reference's compute_pinhole_cxy() with numpy.roots for its LAPACK call. None: no valid root.

    polish: the roots that pass the first filter are refined by Newton on the equation BEFORE it was squared,
    cos(fov) sqrt((1+C^2)(1+C^2+K^2+2KC)) = 1 - KC - C^2. Where cos(fov) = 0 (fov = 90 degrees) the quartic is minus a
    square, each of its roots is double, and an eigenvalue solver returns them to sqrt(DBL_EPSILON) only: 1e-8
    relative, 2e-6 pixels at a focal length of 200. The unsquared equation has simple roots there"""
    cosfov = np.cos(fov_deg*np.pi/180.)
    c2, K = cosfov*cosfov, 2.*tanazel0
    roots = np.roots((1., 2.*K, K*K + 2 + 4./(c2 - 1), 2.*K + K*4./(c2 - 1), K*K + 1. + K*K/(c2 - 1)))
    C = roots[np.abs(roots.imag) <= 1e-7].real
    C = C[cosfov*(1. - K*C - C*C) >= -1e-9]
    if polish:
        for _ in range(4):
            S  = (1 + C*C)*(1 + C*C + K*K + 2*K*C)
            dS = 2*C*(1 + C*C + K*K + 2*K*C) + (1 + C*C)*(2*C + 2*K)
            g  = (1. - K*C - C*C) - cosfov*np.sqrt(S)
            C  = C - g/(-K - 2*C - cosfov*dS/(2*np.sqrt(S)))
    C = C[(tanazel0*fxy + C*fxy)*2. + 1. > 0]
    if C.size == 0: return None
    return C[np.argmax(cosfov*(1. - K*C - C*C))]*fxy


def rectified_system_restated(ref_api, models, *, az_fov_deg, el_fov_deg, el0_deg, pixels_per_deg_az, pixels_per_deg_el,
                              rectification_model, az_edge_margin_deg=10.):
    """numpy restatement of the rectified system with az0 autodetected:
    -> fxycxy, (Naz,Nel), R_rect0_cam0, baseline, az0_deg"""
    def Rt(m): return rotation(m.rt_cam_ref()[:3]), np.asarray(m.rt_cam_ref()[3:], dtype=float)
    (R0, t0), (R1, t1) = Rt(models[0]), Rt(models[1])
    R01 = R0 @ R1.T
    t01 = t0 - R01 @ t1
    baseline = np.linalg.norm(t01)
    right = t01/baseline
    forward01 = R01[:, 2] + np.array((0, 0, 1.))
    forward = forward01 - np.dot(forward01, right)*right
    forward /= np.linalg.norm(forward)
    down = np.cross(forward, right)
    R_rect0_cam0 = np.array((right, down, forward))

    az0_deg = np.degrees(np.arcsin(np.dot(forward01, right)/np.linalg.norm(forward01)))
    loose = az_edge_margin_deg - 1e-3
    if not az0_deg - az_fov_deg/2. > -90. + loose:   az0_deg = -90. + az_edge_margin_deg + az_fov_deg/2.
    elif not az0_deg + az_fov_deg/2. < 90. - loose:  az0_deg =  90. - az_edge_margin_deg - az_fov_deg/2.
    az0, el0 = np.radians(az0_deg), np.radians(el0_deg)

    if rectification_model == "LENSMODEL_LATLON":
        v      = np.array((np.sin(az0), np.cos(az0)*np.sin(el0), np.cos(az0)*np.cos(el0)))
        dv_daz = np.array((np.cos(az0), -np.sin(az0)*np.sin(el0), -np.sin(az0)*np.cos(el0)))
        dv_del = np.array((0., np.cos(az0)*np.cos(el0), -np.cos(az0)*np.sin(el0)))
    else:
        v      = np.array((np.tan(az0), np.tan(el0), 1.))
        dv_daz = np.array((1./np.cos(az0)**2, 0., 0.))
        dv_del = np.array((0., 1./np.cos(el0)**2, 0.))
    R_cam0_rect0 = R_rect0_cam0.T
    _, dq_dv0, _ = ref_api.project(R_cam0_rect0 @ v, *models[0].intrinsics(), get_gradients=True)
    ppd_az = -pixels_per_deg_az*np.linalg.norm(dq_dv0 @ R_cam0_rect0 @ dv_daz)*np.pi/180.
    ppd_el = -pixels_per_deg_el*np.linalg.norm(dq_dv0 @ R_cam0_rect0 @ dv_del)*np.pi/180.
    if rectification_model == "LENSMODEL_LATLON":
        Naz, Nel = int(round(az_fov_deg*ppd_az)), int(round(el_fov_deg*ppd_el))
        ppd_az, ppd_el = Naz/az_fov_deg, Nel/el_fov_deg
        fx, fy = ppd_az/np.pi*180., ppd_el/np.pi*180.
        fxycxy = np.array((fx, fy, (Naz - 1.)/2. - az0*fx, (Nel - 1.)/2. - el0*fy))
    else:
        fx, fy = ppd_az/np.pi*180.*np.cos(az0)**2, ppd_el/np.pi*180.*np.cos(el0)**2
        cx, cy = pinhole_cxy_restated(fx, np.tan(az0), az_fov_deg, True), pinhole_cxy_restated(fy, np.tan(el0), el_fov_deg, True)
        Naz, Nel = int(round((np.tan(az0)*fx + cx)*2.)) + 1, int(round((np.tan(el0)*fy + cy)*2.)) + 1
        fxycxy = np.array((fx, fy, cx, cy))
    return fxycxy, (Naz, Nel), R_rect0_cam0, baseline, az0_deg


def inside_polygon(poly, q):
    """crossing number of a closed contour (N,2) for the points q (...,2): a ray towards +x"""
    x, y = q[..., 0], q[..., 1]
    inside = np.zeros(x.shape, dtype=bool)
    for (x0, y0), (x1, y1) in zip(poly[:-1], poly[1:]):
        if y0 == y1: continue
        with np.errstate(invalid="ignore"):
            cross = ((y0 > y) != (y1 > y)) & (x < (x1 - x0)*(y - y0)/(y1 - y0) + x0)
        inside ^= cross
    return inside


def distance_to_polygon(poly, q):
    """distance of the points q (...,2) to the nearest edge of the contour"""
    best = np.full(q.shape[:-1], np.inf)
    for a, b in zip(poly[:-1], poly[1:]):
        ab = b - a
        s = np.clip(((q - a) @ ab)/np.dot(ab, ab), 0., 1.)
        best = np.minimum(best, np.linalg.norm(q - (a + s[..., None]*ab), axis=-1))
    return best


def stereo_range_one(disparity, qrect0, lensmodel, fxycxy, baseline):
    """the reference's _stereo_range_one(), in numpy; not finite: 0"""
    fx, fy, cx, cy = fxycxy
    with np.errstate(all="ignore"):
        if lensmodel == "LENSMODEL_LATLON":
            az0 = (qrect0[..., 0] - cx)/fx
            r = baseline*np.cos(az0 - disparity/fx)/np.sin(disparity/fx)
        else:
            tanaz0 = (qrect0[..., 0] - cx)/fx
            tanel  = (qrect0[..., 1] - cy)/fy
            s = tanel*tanel + 1.
            dt = disparity/fx
            r = baseline/np.sqrt(s + tanaz0*tanaz0)*((s + tanaz0*(tanaz0 - dt))/dt + tanaz0)
    return np.where(np.isfinite(r), r, 0.)


def bilinear(image, mapxy, border_value):
    """exact bilinear interpolation in double: the image padded by border_value, four neighbours. Returns
    (values (H,W,C) float64, any neighbour outside (H,W) bool, the largest |neighbour| (H,W,C)). A map entry that is not
    finite gives border_value, and counts as outside"""
    src = image.astype(np.float64)
    if src.ndim == 2: src = src[..., None]
    Hs, Ws, C = src.shape
    bv = np.broadcast_to(np.asarray(border_value, dtype=np.float64), (C,))
    x, y = mapxy[..., 0].astype(np.float64), mapxy[..., 1].astype(np.float64)
    finite = np.isfinite(x) & np.isfinite(y)
    far = ~finite | (x <= -1) | (x >= Ws) | (y <= -1) | (y >= Hs)
    xs, ys = np.where(far, 0., x), np.where(far, 0., y)
    x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    fx, fy = (xs - x0)[..., None], (ys - y0)[..., None]
    def at(ix, iy):
        ok = (ix >= 0) & (ix < Ws) & (iy >= 0) & (iy < Hs)
        v = np.where(ok[..., None], src[np.clip(iy, 0, Hs-1), np.clip(ix, 0, Ws-1)], bv)
        return v, ok
    (v00, k00), (v01, k01), (v10, k10), (v11, k11) = at(x0, y0), at(x0+1, y0), at(x0, y0+1), at(x0+1, y0+1)
    val = (1-fy)*((1-fx)*v00 + fx*v01) + fy*((1-fx)*v10 + fx*v11)
    val = np.where(far[..., None], bv, val)
    outside = far | ~(k00 & k01 & k10 & k11)
    largest = np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11)))
    largest = np.where(far[..., None], np.abs(bv), largest)
    return val, outside, largest
