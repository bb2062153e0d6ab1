"""
TEST INFRASTRUCTURE — constructed cameras for the fused row kernel (k_georef_rows, camera-model form), its host-side sky bands
and the two bounding-box reductions on camera frames.

A case is the float64 content of amt_frame_params — width, height, fast_center, cd, crpix, rot, cam, a, b, a0, b0, m_geo, m_sm:
the exact inputs of the kernel and of the references of tests/_camera_oracle.py — plus name, family, claims (what the case says
about itself, checked on the reference by tests/test_camera_cases_cpu.py) and the equivalent WCS header cards with camera and
time for the pipeline (`header`, `time`; `rot` is oracle.ref_numpy.wcs_rotation of that very header).

A camera is placed at geodetic (lat, lon, height) and looks `nadir_angle` degrees away from the geocentric nadir towards
`azimuth`; CD is rolled so that the nadir lies towards growing rows ("Earth below") and then by `roll` degrees more.

Families (the code they aim at is in auromat_amd/csrc/amt_georef.hip):
  cd        make_affine_cam / affine_ray: CD a rotation by 0, 37, 90, 180 deg, flipped parity (det < 0), anisotropic, sheared;
            CRPIX non-integer, at a frame corner, 1000 px outside the frame; m_geo = rot^T, so that m_geo rot has entries of
            order 1e-17; frames around one strip (63 corner columns) and one chunk (16 rows)
  wide      130 x 100 at 0.3 - 0.52 deg / px, the boresight 40 - 100 deg from the nadir: the limb an ellipse, a near-parabola, a
            hyperbola; scales on both sides of the apparent-size gate of sky_bands (asin(sin_rho) > 8 * 18 * pixel angle; from
            400 km, where sin_rho = 0.9588, the limit is 0.5104 deg / px: 0.45 and 0.5 pass, 0.52 does not).  A frame of this size
            around its reference pixel reaches 33 deg off the boresight; with the reference pixel outside the frame the last
            corner of wide-far-corner is 60 deg off
  limb      the extreme row of the limb -2, -1, -0.5, 0, 0.5, 1, 2 rows from a band edge (CRPIX2 moves it), Earth below and
            above, to the left and to the right, the limb through one frame corner; 62 x 50, 70 x 83, 130 x 49: 1, 2, 3 strips,
            the last corner row inside and outside a sky band
  far       42 000 km: the disc wholly inside 330 x 340 at 0.05 deg / px with a sky band above and below (the smallest frame at
            which the gate lets bands exist), the same disc cut by the left side, and at 100 x 100, 0.2 deg / px (gate refuses)
  low       2.5 km above the shell looking at the horizon; a frame of pure sky, a frame of pure ground
  inside    below the shell: every ray hits, the far root, no bands
  exact     fast_center = 0: limbs that cross pixels diagonally (centres that hit with 1 or 2 missing corners, pixels with four
            corners beside them), a disc smaller than a pixel (a centre that hits with 3 and with 4 missing corners: the part of
            a pixel outside a convex disc is not convex only when the disc is that small), a nadir frame (elevations above 89.9
            deg), cd and wide cameras
  pole      the geographic north pole inside a pixel
  dateline  longitudes across +-180 deg

Condition on every case: no corner ray and no exact-centre ray has a relative discriminant |rel| below r_min(), the smallest
|rel| of the limb family of tests/_rowfield_cases.py; CRPIX is nudged by multiples of 2^-10 px until that holds in float64 with
a factor 2 to spare (test_camera_cases_cpu.py asserts it on the longdouble reference).
"""
from datetime import datetime

import numpy as np

from oracle import ref_numpy as O

import _coord_oracle as C
import _rowfield_cases as K
import _rowfield_oracle as R

A0, B0 = K.A0, K.B0
T0 = datetime(2012, 3, 4, 17, 19, 0)
M_GEO, M_SM = K.M_GEO, K.M_SM
NUDGE = 2.0 ** -10
BAND = 16                                   # rows of a work item (shape_of in amt_georef.hip)
SIZES = K.OWNERSHIP_SIZES
LIMB_OFFSETS = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
GATE = 8 * (BAND + 2)                       # sky_bands: asin(sin_rho) > GATE * pixel angle

_RMIN = []


def r_min():
    """the smallest |rel| of the limb family of tests/_rowfield_cases.py (test_gpu_rowfield.py demands identical NaN patterns
    at this margin)"""
    if not _RMIN:
        rel = [np.abs(np.asarray(K.reference_longdouble(c['name'])['rel'], dtype=np.float64)).min() for c in K.family('limb')]
        _RMIN.append(float(min(rel)))
    return _RMIN[0]


# ---- geometry of the construction (float64: it only chooses the numbers of a case) ------------------------------------------------
def rot2(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s], [s, c]])


def boresight(cam, nadir_angle, azimuth):
    up = K.unit(cam)
    east = K.unit(np.cross([0.0, 0.0, 1.0], up))
    north = np.cross(up, east)
    na, az = np.deg2rad(nadir_angle), np.deg2rad(azimuth)
    return -np.cos(na) * up + np.sin(na) * (np.cos(az) * north + np.sin(az) * east)


def header_of(w, h, bore, cd, crpix):
    return {'CTYPE1': 'RA---TAN', 'CTYPE2': 'DEC--TAN', 'LONPOLE': 180.0, 'LATPOLE': 0.0,
            'CRVAL1': float(np.degrees(np.arctan2(bore[1], bore[0])) % 360.0), 'CRVAL2': float(np.degrees(np.arcsin(bore[2]))),
            'CRPIX1': float(crpix[0]), 'CRPIX2': float(crpix[1]),
            'CD1_1': float(cd[0, 0]), 'CD1_2': float(cd[0, 1]), 'CD2_1': float(cd[1, 0]), 'CD2_2': float(cd[1, 1]),
            'IMAGEW': int(w), 'IMAGEH': int(h)}


def earth_below(rot, cam, cd):
    """cd R with R the rotation of the pixel plane after which the nadir lies towards growing rows"""
    ex, ey = rot @ np.array([-cd[1, 0], cd[0, 0], 0.0]), rot @ np.array([-cd[1, 1], cd[0, 1], 0.0])    # d direction / d column, d row
    b, n = rot[:, 2], -K.unit(cam)
    perp = n - (n @ b) * b
    if np.sqrt(perp @ perp) < 1e-9:
        return cd
    g = np.linalg.lstsq(np.stack([ex, ey], axis=1), perp, rcond=None)[0]
    g = g / np.sqrt(g @ g)
    return cd @ np.array([[g[1], g[0]], [-g[0], g[1]]])


def rays(P, x, y):
    """float64: pixel coordinates -> (relative discriminant, hit) of their rays"""
    with np.errstate(invalid='ignore', divide='ignore'):
        d = C._tan_direction(C._F64, P, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        p, rel = R.shell_hit(C._F64, d, P)
    return rel, ~np.isnan(p[0])


def all_rays(c):
    """(rel, hit) of every corner ray and, with exact centres, every centre ray of a case"""
    h, w = c['height'], c['width']
    i, j = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    rel, hit = rays(c, j - 0.5, i - 0.5)
    if c['fast_center']:
        return rel.ravel(), hit.ravel()
    rel_c, hit_c = rays(c, j[:-1, :-1], i[:-1, :-1])
    return np.concatenate((rel.ravel(), rel_c.ravel())), np.concatenate((hit.ravel(), hit_c.ravel()))


def limb_rows(c, sky, ground, columns=None):
    """row coordinate (corner row i is at i; y = i - 1/2) at which the limb crosses each column coordinate, by bisection
    between a row of sky and a row of ground"""
    x = np.arange(-0.5, c['width'] + 0.5 + 1e-9, 0.125) if columns is None else np.asarray(columns, dtype=np.float64)
    lo, hi = np.full(x.shape, float(sky)), np.full(x.shape, float(ground))
    assert not rays(c, x, lo - 0.5)[1].any() and rays(c, x, hi - 0.5)[1].all(), c['name']
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        hit = rays(c, x, mid - 0.5)[1]
        lo, hi = np.where(hit, lo, mid), np.where(hit, mid, hi)
    return hi


def move(c, dx=0.0, dy=0.0):
    """the same sky dx columns to the right and dy rows further down"""
    c['crpix'] = (c['crpix'][0] + dx, c['crpix'][1] + dy)
    return c


def camera(name, family, w, h, lat, lon, height, nadir_angle=None, azimuth=0.0, scale=0.05, roll=0.0, cd=None, crpix=None, fast=1,
           altitude=110.0, aim=None, **claims):
    """`aim`: geodetic (lat, lon) of the point of the shell the boresight looks at, instead of nadir_angle and azimuth"""
    cam = K.ecef(lat, lon, height) @ M_GEO                      # J2000
    bore = boresight(cam, nadir_angle, azimuth) if aim is None else K.unit(K.ecef(aim[0], aim[1], altitude) @ M_GEO - cam)
    base = scale * np.eye(2) if cd is None else np.asarray(cd, dtype=np.float64)
    probe = header_of(w, h, bore, base, (0.0, 0.0))
    cdm = earth_below(O.wcs_rotation(probe), cam, base) @ rot2(roll)
    return dict(name=name, family=family, width=int(w), height=int(h), fast_center=int(fast), cd_matrix=cdm, bore=bore,
                crpix=(w / 2.0 + 0.5, h / 2.0 + 0.5) if crpix is None else tuple(float(v) for v in crpix), cam=cam,
                altitude=float(altitude), a=A0 + altitude, b=B0 + altitude, a0=A0, b0=B0, m_geo=M_GEO, m_sm=M_SM, time=T0,
                scale=scale, claims=dict(claims), **_wcs(probe, cdm))


def _wcs(probe, cdm):
    return dict(cd=tuple(float(v) for v in cdm.ravel()), rot=np.ascontiguousarray(O.wcs_rotation(probe)))


def finish(c):
    """nudges CRPIX until no ray grazes, writes the header, freezes the arrays"""
    margin = 2.0 * r_min()
    for k in range(400):
        rel, _ = all_rays(c)
        with np.errstate(invalid='ignore'):
            if not (np.abs(rel) < margin).any():
                break
        move(c, NUDGE * (1 + k % 3), NUDGE * (1 + k % 5))
    else:
        raise AssertionError('%s: a ray grazes the shell whatever the nudge' % c['name'])
    c['nudges'] = k
    c['header'] = header_of(c['width'], c['height'], c.pop('bore'), c.pop('cd_matrix'), c['crpix'])
    assert np.array_equal(O.wcs_rotation(c['header']), c['rot'])
    for k in ('rot', 'cam', 'm_geo', 'm_sm'):
        c[k] = np.ascontiguousarray(c[k], dtype=np.float64)
        c[k].setflags(write=False)
    return c


def exact(c, name=None, **claims):
    """the same camera with exact centres"""
    d = dict(c, name=name or 'exact-' + c['name'], family='exact', fast_center=0,
             claims=dict(c['claims'], **claims))
    return d


# ---- the families ------------------------------------------------------------------------------------------------------------------
ISS = dict(lat=49.0, lon=14.0, height=400.0)


def _cd():
    out = []
    for deg in (0, 37, 90, 180):
        out.append(camera('cd-rotation-%d' % deg, 'cd', 40, 30, nadir_angle=30.0, azimuth=20.0, roll=deg, **ISS))
    s = 0.05
    out.append(camera('cd-flipped', 'cd', 40, 30, nadir_angle=30.0, azimuth=20.0, cd=[[-s, 0.0], [0.0, s]], roll=11.0, negative_det=True, **ISS))
    out.append(camera('cd-anisotropic', 'cd', 40, 30, nadir_angle=30.0, azimuth=20.0, cd=[[s, 0.0], [0.0, 1.6 * s]], roll=11.0, **ISS))
    out.append(camera('cd-sheared', 'cd', 40, 30, nadir_angle=30.0, azimuth=20.0, cd=[[s, 0.4 * s], [0.0, s]], roll=11.0, **ISS))
    out.append(camera('cd-crpix-fraction', 'cd', 40, 30, nadir_angle=30.0, azimuth=20.0, crpix=(17.31, 9.77), **ISS))
    out.append(camera('cd-crpix-corner', 'cd', 40, 30, nadir_angle=30.0, azimuth=20.0, crpix=(0.5, 0.5), **ISS))
    # the frame is 1000 px (41 deg in the tangent plane) from the reference pixel, on the nadir's side of a boresight at 60 deg
    out.append(camera('cd-crpix-outside', 'cd', 40, 30, nadir_angle=60.0, azimuth=20.0, crpix=(20.5, -1000.0), **ISS))
    c = camera('cd-rot-cancels', 'cd', 40, 30, nadir_angle=30.0, azimuth=20.0, roll=11.0, rot_cancels=True, **ISS)
    c['m_geo'] = np.ascontiguousarray(c['rot'].T)               # m_geo rot = I + O(1e-17): "GEO" is the camera's native frame
    c['time'] = None                                            # (no photo time gives this matrix: no header form)
    out.append(c)
    for w, h in SIZES:
        out.append(camera('cd-%dx%d' % (w, h), 'cd', w, h, nadir_angle=30.0, azimuth=-50.0, roll=23.0, **ISS))
    return out


def rho_of(c):
    """apparent radius of the shell as sky_bands takes it: asin(a / |camera|), radians"""
    return float(np.arcsin(min(1.0, c['a'] / np.sqrt(c['cam'] @ c['cam']))))


def gate_passes(c):
    cd = np.asarray(c['cd']).reshape(2, 2)
    pixel = np.deg2rad(np.sqrt(max(cd[0, 0] ** 2 + cd[1, 0] ** 2, cd[0, 1] ** 2 + cd[1, 1] ** 2)))
    return rho_of(c) > GATE * pixel


def _wide():
    out = []
    high = dict(lat=49.0, lon=14.0, height=3000.0)              # apparent radius 43.8 deg
    for tag, where, na, scale, conic in (('ellipse', high, 40.0, 0.3, 'ellipse'), ('parabola', high, 46.2, 0.3, 'near-parabola'),
                                         ('hyperbola-70', ISS, 70.0, 0.45, 'hyperbola'), ('gate-0.5', ISS, 75.0, 0.5, 'hyperbola'),
                                         ('gate-0.52', ISS, 75.0, 0.52, 'hyperbola')):
        out.append(camera('wide-' + tag, 'wide', 130, 100, nadir_angle=na, azimuth=35.0, scale=scale, roll=14.0, conic=conic, **where))
    # boresight 100 deg from the nadir, above the horizon: the limb is 26.5 deg (28.6 deg of the tangent plane) below it, so the
    # frame lies 45 rows and more below the reference pixel
    out.append(camera('wide-hyperbola-100', 'wide', 130, 100, nadir_angle=100.0, azimuth=35.0, scale=0.4, roll=14.0, crpix=(65.5, -44.5),
                      conic='hyperbola', **ISS))
    # ... and with the reference pixel at the first column too, the last corner is 60 deg off the boresight (a frame of this
    # size around its reference pixel reaches 33 deg at these scales)
    out.append(camera('wide-far-corner', 'wide', 130, 100, nadir_angle=100.0, azimuth=35.0, scale=0.52, roll=0.0, crpix=(0.5, -44.5),
                      conic='hyperbola', corner_off=60.0, **ISS))
    for c in out:
        c['claims']['gate'] = bool(gate_passes(c))
    return out


def _limb():
    out = []

    def on_the_limb(name, w, h, roll, **claims):
        return camera(name, 'limb', w, h, nadir_angle=73.0, azimuth=-20.0, roll=roll, **dict(ISS, **claims))
    for off in LIMB_OFFSETS:
        c = on_the_limb('limb-below%+g' % off, 62, 50, 0.0, earth='below', limb_row=2 * BAND + off)
        top = limb_rows(c, -300.0, 400.0).min()
        out.append(move(c, dy=c['claims']['limb_row'] - top))
        c = on_the_limb('limb-above%+g' % off, 70, 83, 180.0, earth='above', limb_row=2 * BAND + off)
        bottom = limb_rows(c, 400.0, -300.0).max()
        out.append(move(c, dy=c['claims']['limb_row'] - bottom))
    for off in (-0.5, 0.5):
        c = on_the_limb('limb-below-3-strips%+g' % off, 130, 49, 0.0, earth='below', limb_row=2 * BAND + off)
        out.append(move(c, dy=c['claims']['limb_row'] - limb_rows(c, -300.0, 400.0).min()))
    out.append(on_the_limb('limb-right', 62, 50, 90.0, earth='side'))
    out.append(on_the_limb('limb-left', 62, 50, 270.0, earth='side'))
    # the limb through the last corner of the frame alone: Earth towards that corner, the limb 1.5 px inside it on the diagonal
    c = on_the_limb('limb-corner', 70, 83, 45.0, earth='corner')
    lo, hi = -400.0, 400.0                                      # shift along the diagonal: sky ... ground at the corner ray
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        t = dict(c, crpix=(c['crpix'][0] - mid, c['crpix'][1] - mid))
        lo, hi = (lo, mid) if rays(t, c['width'] - 0.5, c['height'] - 0.5)[1] else (mid, hi)
    out.append(move(c, -(hi + 1.5 / np.sqrt(2.0)), -(hi + 1.5 / np.sqrt(2.0))))
    return out


GEO_ORBIT = dict(lat=5.0, lon=30.0, height=42000.0)


def _far():
    c = camera('far-disc-inside', 'far', 330, 340, nadir_angle=0.0, disc='inside', bands=(1, 1), **GEO_ORBIT)
    mid = [c['crpix'][0] - 1.0]
    top = limb_rows(c, -200.0, c['crpix'][1] - 0.5, columns=mid)[0]
    bottom = limb_rows(c, 600.0, c['crpix'][1] - 0.5, columns=mid)[0]
    move(c, dy=0.5 * (c['height'] - (top + bottom)) + 5.0)      # 15 rows above the disc would leave no band: 20 above, 10 + 4 below
    cut = camera('far-disc-cut', 'far', 120, 340, nadir_angle=0.0, disc='cut', **GEO_ORBIT)         # the disc's right part
    move(cut, dx=-120.0, dy=c['crpix'][1] - cut['crpix'][1])
    small = camera('far-gate-refuses', 'far', 100, 100, nadir_angle=0.0, scale=0.2, disc='inside', **GEO_ORBIT)
    out = [c, cut, small]
    for k in out:
        k['claims']['gate'] = bool(gate_passes(k))
    return out


def _low_and_inside():
    out = [camera('low-horizon', 'low', 40, 35, lat=49.0, lon=14.0, height=112.5, nadir_angle=88.4, azimuth=60.0, earth='below'),
           camera('low-sky', 'low', 40, 35, nadir_angle=180.0, pure='sky', **ISS),
           camera('low-ground', 'low', 40, 35, nadir_angle=0.0, pure='ground', **ISS),
           camera('inside', 'inside', 70, 40, lat=65.0, lon=25.0, height=50.0, nadir_angle=95.0, azimuth=10.0, scale=0.3, inside=True)]
    return out


def _exact():
    out = []
    # (at 45 deg exactly the limb cuts off one corner of a pixel at a time: two corners miss together with the centre)
    for roll, missing in ((37.0, (1, 2)), (-45.0, (1,))):
        c = camera('exact-diagonal%+d' % roll, 'exact', 62, 50, nadir_angle=73.0, azimuth=-20.0, roll=roll, fast=0,
                   missing_corners=missing, **ISS)
        out.append(c)
    # a disc of 7.7 deg in pixels of 21 deg: its centre a quarter of a pixel from the centre of pixel (1, 1) towards a corner
    # (that corner hits, three miss), and next to the centre of a pixel (four miss)
    for tag, off, n in (('3', 0.25, 3), ('4', 0.05, 4)):
        c = camera('exact-tiny-disc-' + tag, 'exact', 4, 4, nadir_angle=0.0, scale=21.0, fast=0, missing_corners=(n,), **GEO_ORBIT)
        c['crpix'] = (2.0 + off, 2.0 + off)                     # the reference pixel (the nadir) at pixel coordinates (1 + off, 1 + off)
        out.append(c)
    out.append(camera('exact-nadir', 'exact', 40, 30, nadir_angle=0.0, crpix=(20.7, 15.4), fast=0, steep=True, **ISS))
    return out


def _pole_and_dateline():
    return [camera('pole', 'pole', 40, 30, lat=89.2, lon=40.0, height=400.0, aim=(89.97, 100.0), scale=0.1, roll=20.0, pole=1),
            camera('dateline', 'dateline', 40, 30, lat=20.0, lon=179.8, height=400.0, aim=(20.0, 180.0), roll=5.0, dateline=True)]


FAMILIES = ('cd', 'wide', 'limb', 'far', 'low', 'inside', 'exact', 'pole', 'dateline')
_CASES = []


def cases():
    if not _CASES:
        made = []
        for make in (_cd, _wide, _limb, _far, _low_and_inside, _exact, _pole_and_dateline):
            made.extend(make())
        by = {c['name']: c for c in made}
        for src in ('cd-rotation-37', 'cd-sheared', 'cd-crpix-outside', 'cd-63x16', 'cd-64x17', 'limb-below+0.5', 'limb-above-1',
                    'limb-corner', 'wide-hyperbola-70', 'low-horizon'):
            made.append(exact(by[src]))
        _CASES.extend(finish(c) for c in made)
        assert {c['family'] for c in _CASES} == set(FAMILIES) and len({c['name'] for c in _CASES}) == len(_CASES)
    return _CASES


def names():
    return [c['name'] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c['name'] == name)


def family(name):
    return [c for c in cases() if c['family'] == name]


# the cases in which amt_georef_sky_rows finds a sky band (tests/test_camera_cases_cpu.py holds the list to the host function)
SKY_BAND_NAMES = ('wide-ellipse', 'wide-parabola', 'wide-hyperbola-70', 'wide-gate-0.5') + \
    tuple('limb-%s%+g' % (e, o) for o in LIMB_OFFSETS for e in ('below', 'above')) + \
    ('limb-below-3-strips-0.5', 'limb-below-3-strips+0.5', 'limb-corner', 'far-disc-inside', 'far-disc-cut', 'low-horizon', 'low-sky',
     'exact-limb-below+0.5', 'exact-limb-above-1', 'exact-limb-corner', 'exact-wide-hyperbola-70', 'exact-low-horizon')

# the header form of the cases for the two plans of the pipeline.  Left out: cd-rot-cancels (its m_geo belongs to no photo
# time, so it has no header form), cd-1x1 (fused binning needs at least 3 pixels, prepare_georef), pole (a pole in view takes
# the pole plan, pinned by tests/test_pole_frames.py), low-sky (no pixel to bin: an empty frame has no plan) and the two
# tiny-disc frames (their only pixels with four corners do not exist: nothing is binned)
NO_PLAN = ('cd-rot-cancels', 'cd-1x1', 'pole', 'low-sky', 'exact-tiny-disc-3', 'exact-tiny-disc-4')
PLAN_NAMES = ('cd-rotation-37', 'cd-flipped', 'cd-crpix-outside', 'cd-64x17', 'cd-127x33', 'wide-ellipse', 'wide-hyperbola-70',
              'limb-below+0.5', 'limb-above-1', 'limb-below-3-strips-0.5', 'limb-corner', 'far-disc-inside', 'low-horizon',
              'low-ground', 'inside', 'exact-diagonal+37', 'exact-limb-above-1', 'exact-cd-sheared', 'dateline')


def native_params(c, fast_center=None):
    """the amt_frame_params block of a case: its numbers as they are"""
    from auromat_amd._native import FrameParams
    p = FrameParams()
    p.width, p.height = c['width'], c['height']
    p.fast_center = c['fast_center'] if fast_center is None else int(fast_center)
    p.cd[:] = list(c['cd'])
    p.crpix[:] = list(c['crpix'])
    for k in ('rot', 'cam', 'm_geo', 'm_sm'):
        getattr(p, k)[:] = [float(v) for v in np.asarray(c[k]).ravel()]
    p.a, p.b, p.a0, p.b0 = c['a'], c['b'], c['a0'], c['b0']
    return p


# ---- references, computed once per process ----------------------------------------------------------------------------------------
_REF, _F64, _RAW = {}, {}, {}


def reference(name):
    import _camera_oracle as Q
    if name not in _REF:
        r = Q.reference(by_name(name))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def reference_longdouble(name):
    import _camera_oracle as Q
    if name not in _RAW:
        _RAW[name] = Q.reference(by_name(name), substitute=False)
    return _RAW[name]


def float64_oracle(name):
    import _camera_oracle as Q
    if name not in _F64:
        _F64[name] = Q.float64_oracle(by_name(name))
    return _F64[name]


def e_ref(fam, array):
    """distance of the float64 oracle from the reference, the largest over the family's cases"""
    import _camera_oracle as Q
    return max(float(Q.distance(array, float64_oracle(c['name']), reference(c['name'])).max()) for c in family(fam))


def bounds(fam):
    import _camera_oracle as Q
    return {k: Q.bound(k, e_ref(fam, k)) for k in Q.ARRAYS}
