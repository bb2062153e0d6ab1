"""
The statement of world -> pixel (include/auromat_hip.h "inverse georeferencing"; tests/_inverse_oracle.py) against the forward
direction, in mpmath, and the host pieces built on it.  No GPU.

Measured here (mpmath, 50 digits; the inputs of the inverse are the forward's results rounded to float64):
  inverse o forward, exact geodetic latitude        largest distance 7.6e-12 px (bound 2e-9 px, see ROUND_TRIP_BOUND)
  inverse o forward, one-step Bowring latitude      printed by test_bowring_residual; it goes into the round-trip bound of
                                                    tests/test_gpu_inverse_points.py
"""
import numpy as np
import pytest

import _inverse_cases as IC
import _inverse_oracle as O

# The inverse's inputs are float64 degrees: half a unit in the last place of 180 deg is 1.4e-14 deg = 2.5e-16 rad, 1.6e-12 km on
# the shell; seen from the closest camera of the cases (low-horizon, 2.5 km above the shell) that is 6.5e-13 rad = 3.7e-11 deg, at
# 0.05 deg / px 7.4e-10 px per coordinate; two coordinates and the same again for the pixel position's own rounding: 2e-9 px.
ROUND_TRIP_BOUND = 2e-9


@pytest.mark.parametrize('frame', ['geodetic', 'sm', 'j2000'])
def test_inverse_of_forward_is_identity(frame):
    worst, n = 0.0, 0
    for name in IC.names():
        r = IC.points(name)[frame]
        assert not (r['ref']['flags'] & O.NO_PIXEL).any(), name
        d = IC.distance(r)
        n += d.size
        worst = max(worst, float(d.max()) if d.size else 0.0)
    print('%s: %d points, largest distance %.3e px' % (frame, n, worst))
    assert n > 900 and worst <= ROUND_TRIP_BOUND


def test_bowring_residual():
    res = IC.bowring_residual()
    print('one-step Bowring latitude instead of the exact one: %.3e px' % res)
    # one Bowring step is good to ~1e-11 deg at the shell's height; through the same geometry as above that is well below a
    # thousandth of a pixel.  The number itself is not asserted to be small here beyond that: it is a property of the forward.
    assert 0.0 < res < 1e-3


def test_visibility_is_the_forwards_root_choice():
    for name in IC.names():
        cam = IC.by_name(name)
        inside = sum((cam['cam'][i] / (cam['a'], cam['a'], cam['b'])[i]) ** 2 for i in range(3)) < 1
        for frame in ('geodetic', 'sm'):
            r = IC.points(name)[frame]
            hidden = (r['ref']['flags'] & O.HIDDEN) != 0
            assert np.array_equal(hidden, r['expect_hidden']), (name, frame)
            if inside:
                assert not hidden.any(), name
            elif len(hidden):
                assert hidden.any() and not hidden.all(), name      # near roots visible, far roots hidden
        r = IC.points(name)['j2000']
        assert np.array_equal((r['ref']['flags'] & O.HIDDEN) != 0, r['expect_hidden']), name


def test_no_point_is_ambiguous():
    """the cap on points left out of the flag comparison of the GPU test is 0: every point is this far from every decision"""
    for name in IC.names():
        for frame, _ in IC.FRAMES:
            r = IC.points(name)[frame]
            if len(r['c0']):
                assert r['ref']['margin'].min() >= IC.AMBIGUOUS, (name, frame, r['ref']['margin'].min())


def test_outside_points_are_flagged_outside():
    for name in IC.names():
        cam = IC.by_name(name)
        r = IC.points(name)['j2000']
        out = (r['px'] < -0.5) | (r['px'] > cam['width'] - 0.5) | (r['py'] < -0.5) | (r['py'] > cam['height'] - 0.5)
        assert out.sum() == 2 and np.array_equal((r['ref']['flags'] & O.OUTSIDE) != 0, out), name


@pytest.mark.parametrize('frame', ['geodetic', 'sm', 'j2000'])
def test_float64_statement_agrees_with_mpmath(frame):
    code = dict(IC.FRAMES)[frame]
    worst = 0.0
    for name in IC.names():
        r = IC.points(name)[frame]
        if not len(r['c0']):
            continue
        got = O.inverse_arrays(O.F64, IC.by_name(name), code, r['c0'], r['c1'])
        assert np.array_equal(got['flags'], r['ref']['flags']), name
        worst = max(worst, float(np.nanmax(np.hypot(got['x'] - r['ref']['x'], got['y'] - r['ref']['y']))))
    print('%s: float64 statement against mpmath, largest distance %.3e px' % (frame, worst))
    assert worst <= 1e-8


def test_edge_inputs_of_the_statement():
    cam = IC.by_name('cd-rotation-37')
    for c0, c1 in ((np.nan, 0.0), (0.0, np.inf), (90.0000001, 0.0), (-91.0, 10.0)):
        r = O.inverse(O.F64, cam, O.GEODETIC, c0, c1)
        assert r['flags'] == O.INVALID and np.isnan(r['x']) and np.isnan(r['y'])
    for frame in (O.GEODETIC, O.SM, O.J2000):
        a, b, c = (O.inverse(O.F64, cam, frame, 30.0, lon) for lon in (180.0, -180.0, 540.0))
        assert a['flags'] == b['flags'] == c['flags']
        assert (a['x'], a['y']) == (b['x'], b['y']) == (c['x'], c['y']) or a['flags'] & O.NO_PIXEL
        assert O.inverse(O.F64, cam, frame, 90.0, 12.0)['flags'] & O.INVALID == 0
    # the boresight itself: rho = 0, CRPIX - 1 exactly (mpmath: the float64 angles of CRVAL do not hit rho = 0 exactly)
    d = O.forward_mp(cam, cam['crpix'][0] - 1, cam['crpix'][1] - 1)
    r = O.inverse(O.MP(), cam, O.J2000, d['dec'], d['ra'])
    assert abs(float(r['x']) - (cam['crpix'][0] - 1)) < 1e-11 and abs(float(r['y']) - (cam['crpix'][1] - 1)) < 1e-11
    # behind a TAN camera, and the domain limits of SIN and STG
    behind = O.inverse(O.F64, cam, O.J2000, -d['dec'], d['ra'] + 180.0)
    assert behind['flags'] & O.UNPROJECTABLE and np.isnan(behind['x'])
    sin_cam, stg_cam = IC.by_name('zen-SIN'), IC.by_name('zen-STG')
    ds = O.forward_mp(sin_cam, sin_cam['crpix'][0] - 1, sin_cam['crpix'][1] - 1)
    assert O.inverse(O.F64, sin_cam, O.J2000, -ds['dec'], ds['ra'] + 180.0)['flags'] & O.UNPROJECTABLE
    assert not O.inverse(O.F64, sin_cam, O.J2000, ds['dec'] - 89.0, ds['ra'])['flags'] & O.UNPROJECTABLE
    assert O.inverse(O.F64, sin_cam, O.J2000, ds['dec'] - 91.0, ds['ra'])['flags'] & O.UNPROJECTABLE
    dg = O.forward_mp(stg_cam, stg_cam['crpix'][0] - 1, stg_cam['crpix'][1] - 1)
    assert not O.inverse(O.F64, stg_cam, O.J2000, dg['dec'] - 170.0, dg['ra'])['flags'] & O.UNPROJECTABLE


def test_sip_fold_over_does_not_converge():
    cam = IC.by_name('sip-fold')
    plain = dict(cam, sip_a=None, sip_b=None)
    # pixel offsets U = -14 < -12.5 have no preimage under u + 0.02 u^2: the sky position that the undistorted camera sees there
    d = O.forward_mp(plain, cam['crpix'][0] - 1 - 14.0, 20.0)
    for xp in (O.F64, O.MP()):
        r = O.inverse(xp, cam, O.J2000, d['dec'], d['ra'])
        assert r['flags'] & O.NOT_CONVERGED and not r['flags'] & O.OUTSIDE
        assert np.isnan(float(r['x'])) and np.isnan(float(r['y']))
    # on the near side of the fold the inverse is the identity (the lattice of the case lies there)
    assert IC.distance(IC.points('sip-fold')['j2000']).max() < ROUND_TRIP_BOUND


# ---- host pieces -----------------------------------------------------------------------------------------------------------
class _Box(object):
    def __init__(self, south, west, north, east, pole=False):
        self.latSouth, self.lonWest, self.latNorth, self.lonEast, self.containsPole = south, west, north, east, pole
        self.containsDiscontinuity = west > east


class _StatementMapping(object):
    """latLonToPixel by the float64 statement: what graticulePixels needs of a mapping"""

    def __init__(self, cam, box):
        self.cam, self.boundingBox = cam, box

    def latLonToPixel(self, lat, lon, altitude=None, returnFlags=False):
        import numpy.ma as ma
        cam = self.cam if altitude is None else dict(self.cam, a=self.cam['a0'] + altitude, b=self.cam['b0'] + altitude)
        r = O.inverse_arrays(O.F64, cam, O.GEODETIC, lat, lon)
        mask = (r['flags'] & (O.NO_PIXEL | O.HIDDEN)) != 0
        return ma.masked_array(r['x'], mask=mask), ma.masked_array(r['y'], mask=mask)


def test_graticule_lines():
    from auromat_amd.draw import graticule_lines
    par, mer = graticule_lines(_Box(47.3, 9.1, 52.0, 15.95), every=2, step=0.2)
    assert [p[0] for p in par] == [48, 50, 52] and [m[0] for m in mer] == [10, 12, 14]
    for deg, la, lo in par:
        assert np.all(la == deg) and lo[0] == 9.1 and lo[-1] == 15.95 and np.allclose(np.diff(lo)[:-1], 0.2)
    for deg, la, lo in mer:
        assert np.all(lo == deg) and la[0] == 47.3 and la[-1] == 52.0 and len(la) == 25
    # across the date line: from the west edge eastwards through 180 deg; longitudes come back in [-180, 180)
    par, mer = graticule_lines(_Box(-3.0, 176.5, 1.0, -177.0), every=2, step=0.5)
    assert [m[0] for m in mer] == [178, -180, -178] and [p[0] for p in par] == [-2, 0]
    lo = par[0][2]
    assert lo[0] == 176.5 and lo[-1] == -177.0 and lo.min() >= -180.0 and lo.max() < 180.0 and len(lo) == 14
    # a pole in view: all the way around, +180 is not drawn twice
    par, mer = graticule_lines(_Box(80.0, -180, 90, 180, pole=True), every=30, step=1.0)
    assert [m[0] for m in mer] == list(range(-180, 180, 30)) and [p[0] for p in par] == [90]
    with pytest.raises(ValueError):
        graticule_lines(_Box(0, 0, 1, 1), every=0)


def test_graticule_pixels_against_the_statement():
    from auromat_amd.draw import graticulePixels
    cam = IC.by_name('cd-rotation-37')
    geo = IC.points('cd-rotation-37')['geodetic']
    vis = ~geo['expect_hidden'] & (geo['ref']['flags'] == 0)
    box = _Box(geo['c0'][vis].min() - 0.02, geo['c1'][vis].min() - 0.02, geo['c0'][vis].max() + 0.02, geo['c1'][vis].max() + 0.02)
    par, mer = graticulePixels(_StatementMapping(cam, box), every=0.05, step=0.01)
    assert len(par) >= 2 and len(mer) >= 2
    inside = 0
    for lines, lat_is_key in ((par, True), (mer, False)):
        for deg, xy in lines.items():
            assert xy.dtype == np.float64 and xy.ndim == 2 and xy.shape[1] == 2
            n = xy.shape[0]
            lo = np.concatenate((box.lonWest + 0.01 * np.arange(n - 1), [box.lonEast]))[:n]
            la = np.concatenate((box.latSouth + 0.01 * np.arange(n - 1), [box.latNorth]))[:n]
            for i in (0, n // 2, n - 1):
                r = O.inverse(O.F64, cam, O.GEODETIC, deg if lat_is_key else la[i], lo[i] if lat_is_key else deg)
                if r['flags'] & (O.NO_PIXEL | O.HIDDEN):
                    assert np.isnan(xy[i]).all()
                else:
                    assert abs(xy[i, 0] - r['x']) < 1e-6 and abs(xy[i, 1] - r['y']) < 1e-6, (deg, i)
            inside += int(((xy[:, 0] > 0) & (xy[:, 0] < cam['width']) & (xy[:, 1] > 0) & (xy[:, 1] < cam['height'])).sum())
    assert inside > 20
    # the ground below: other pixels
    par0, _ = graticulePixels(_StatementMapping(cam, box), every=0.05, step=0.01, altitude=0.0)
    k = sorted(par)[len(par) // 2]
    assert np.nanmax(np.abs(par0[k] - par[k])) > 1.0


def test_gather_statement_on_a_tiny_frame():
    cam = IC.by_name('cd-rotation-37')
    geo = IC.points('cd-rotation-37')['geodetic']
    vis = ~geo['expect_hidden']
    lat_axis = np.linspace(geo['c0'][vis].max() + 0.3, geo['c0'][vis].min() - 0.3, 9)
    lon_axis = np.linspace(geo['c1'][vis].min() - 0.3, geo['c1'][vis].max() + 0.3, 11)
    rng = np.random.RandomState(5)
    image = rng.randint(0, 256, size=(cam['height'], cam['width'], 3)).astype(np.uint8)
    la, lo = np.meshgrid(lat_axis, lon_axis, indexing='ij')
    ref = O.inverse_arrays(O.MP(), cam, O.GEODETIC, la, lo)
    assert ref['margin'].min() > 1e-9
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        s = O.gather_statement(cam, O.GEODETIC, lat_axis, lon_axis, image, interpolation)
        supported = (ref['x'] >= 0) & (ref['x'] <= cam['width'] - 1) & (ref['y'] >= 0) & (ref['y'] <= cam['height'] - 1)
        want = (ref['flags'] != 0) | (~supported if interpolation != 'nearest' else False)
        assert np.array_equal(s['mask'], want) and 0 < s['mask'].sum() < s['mask'].size
        assert s['img'].shape == (9, 11, 3) and s['img'].dtype == np.uint8
    s = O.gather_statement(cam, O.GEODETIC, lat_axis, lon_axis, image, 'nearest')
    i, j = np.argwhere(~s['mask'])[0]
    assert np.array_equal(s['img'][i, j], image[int(np.rint(ref['y'][i, j])), int(np.rint(ref['x'][i, j]))])
    cm = np.zeros(image.shape[:2], dtype=bool)
    cm[int(np.rint(ref['y'][i, j])), int(np.rint(ref['x'][i, j]))] = True
    assert O.gather_statement(cam, O.GEODETIC, lat_axis, lon_axis, image, 'nearest', center_mask=cm)['mask'][i, j]
    e = float(s['elevation'][i, j])
    assert O.gather_statement(cam, O.GEODETIC, lat_axis, lon_axis, image, 'nearest', min_elevation=e + 1e-3)['mask'][i, j]
    assert not O.gather_statement(cam, O.GEODETIC, lat_axis, lon_axis, image, 'nearest', min_elevation=e - 1e-3)['mask'][i, j]


# ---- argument checks and what is not built -----------------------------------------------------------------------------------
def test_not_implemented_cases():
    from auromat_amd.mapping.astrometry import DirectionArrayMapping
    from auromat_amd.mapping.mapping import BaseMapping, MappingCollection
    from auromat_amd.mapping.miracle import MIRACLEMapping
    from auromat_amd.mapping.themis import ThemisMapping
    from auromat_amd.resample import resampleGather, resampleGatherMLatMLT
    cam = IC.by_name('cd-rotation-37')
    dirs = np.zeros((cam['height'] + 1, cam['width'] + 1, 3))
    dirs[..., 2] = 1.0
    img = np.zeros((cam['height'], cam['width'], 3), dtype=np.uint8)
    bare = DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'bare')
    for call in (lambda: bare.latLonToPixel([0.0], [0.0]), lambda: bare.mLatMltToPixel([0.0], [0.0]),
                 lambda: bare.raDecToPixel([0.0], [0.0]), lambda: resampleGather(bare), lambda: resampleGatherMLatMLT(bare)):
        with pytest.raises(NotImplementedError, match='direction'):
            call()
    lens = DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'raw', noInverse='a raw frame with its lens distortion')
    with pytest.raises(NotImplementedError, match='lens'):
        lens.latLonToPixel([0.0], [0.0])
    for cls in (MIRACLEMapping, ThemisMapping):
        assert cls._inverse_model is BaseMapping._inverse_model and cls.latLonToPixel is BaseMapping.latLonToPixel
        with pytest.raises(NotImplementedError, match='camera model'):
            cls.__new__(cls).latLonToPixel([0.0], [0.0])
    for what in ([bare], MappingCollection([bare], 'c')):
        with pytest.raises(NotImplementedError, match='collections'):
            resampleGather(what)
    with pytest.raises(ValueError, match='interpolation'):
        resampleGather(bare, interpolation='cubic')


def test_new_entry_points_are_declared():
    import os
    from auromat_amd import _native
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'auromat_hip.h')).read()
    for name in ('amt_world_to_pixel', 'amt_grid_to_pixel'):
        assert name in _native._SIGNATURES and ('int %s(amt_ctx* ctx' % name) in header
    assert '#define AMT_ABI_VERSION 10' in header and _native.ABI_VERSION == 10
    from auromat_amd.coordinates import inverse as I
    for name in ('INVALID', 'HIDDEN', 'UNPROJECTABLE', 'NOT_CONVERGED', 'OUTSIDE'):
        assert ('#define AMT_W2P_%s %d' % (name, getattr(I, name))) in header and getattr(O, name) == getattr(I, name)
