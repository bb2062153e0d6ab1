"""
Without a GPU: the projection oracle (tests/_projection_oracle.py) against Snyder's worked examples and against itself in three
number types, the host constants of the library (``amt_projection_stereographic`` / ``amt_projection_polar_aeqd``,
auromat_amd/csrc/amt_params.h) against mpmath, that every family of tests/_projection_cases.py aims where it claims to, the grid
and default-geometry rules of the three public functions of auromat_amd.resample against hand-computed values, and
``saveMapImage`` read back.  tests/test_gpu_projection.py runs the same cases on the device.
"""
import ctypes as C

import numpy as np
import numpy.ma as ma
import pytest

import _projection_cases as K
import _projection_oracle as O

F64, LD, MP = O.Float64(), O.LongDouble(), O.MultiPrecision()
EPS = float(np.finfo(np.float64).eps)


def test_snyder_oblique_example():
    """Snyder p. 313: Clarke 1866, phi1 = 40, lambda0 = -100, k0 = 0.9999; 30 N 90 W -> x = 971 630.8 m, y = -1 063 049.3 m"""
    a, e2 = 6378206.4, 0.00676866
    P = O.stere(40.0, -100.0, a, a * np.sqrt(1 - e2))
    for xp in (F64, LD, MP):
        x, y = O.points(xp, O.forward, P, [30.0], [-90.0])
        assert abs(float(x[0]) * 0.9999 - 971630.8) < 0.05 and abs(float(y[0]) * 0.9999 + 1063049.3) < 0.05, (xp.name, x, y)
        la, lo = O.points(xp, O.inverse, P, x.astype(np.float64), y.astype(np.float64))
        assert abs(float(la[0]) - 30.0) < 1e-9 and abs(float(lo[0]) + 90.0) < 1e-9


def test_snyder_polar_example():
    """Snyder p. 315-316: International ellipsoid, south polar, lambda0 = -100; 75 S 150 E.  With k0 = 0.994 at the pole:
    x = -1 573 645.4 m, y = -572 760.1 m; with the scale true along 71 S (21-34: rho = a m_c t / t_c):
    x = -1 540 033.6 m, y = -560 526.4 m.  The text carries t with seven digits (0.1325120): 0.3 m of rho."""
    a, e2 = 6378388.0, 0.00672267
    P = O.stere(-90.0, -100.0, a, a * np.sqrt(1 - e2))
    e = np.sqrt(e2)
    for xp in (F64, LD, MP):
        x, y = (float(v[0]) for v in O.points(xp, O.forward, P, [-75.0], [150.0]))
        assert abs(x * 0.994 + 1573645.4) < 0.5 and abs(y * 0.994 + 572760.1) < 0.5, (xp.name, x, y)
        # the pole's scale factor of a map that is true along 71 S: rho_true(71 S) / rho_k0=1(71 S)
        xc, yc = (float(v[0]) for v in O.points(xp, O.forward, P, [-71.0], [-100.0]))
        m_c = np.cos(np.deg2rad(71.0)) / np.sqrt(1 - e2 * np.sin(np.deg2rad(71.0)) ** 2)
        k0 = a * m_c / np.hypot(xc, yc)
        assert abs(x * k0 + 1540033.6) < 0.5 and abs(y * k0 + 560526.4) < 0.5, (xp.name, x * k0, y * k0)
        assert xc == 0.0 or abs(xc) < 1e-6                     # on the central meridian, towards +y (south polar)
        assert yc > 0
    assert abs(e - 0.0819918) < 1e-6


def _lib():
    from auromat_amd._native import lib
    return lib()


def _constants(P):
    from auromat_amd._native import Projection
    p = Projection()
    if P['kind'] == 'paeqd':
        rc = _lib().amt_projection_polar_aeqd(1 if P['north'] else 0, P['lon0'], P['a'], C.byref(p))
    else:
        rc = _lib().amt_projection_stereographic(P['lat0'], P['lon0'], P['a'], P['b'], C.byref(p))
    assert rc == 0
    return p


@pytest.mark.parametrize('name,P', K.projections() + [('stere_almost_polar', O.stere(90 - 2e-8, 5.0)),
                                                      ('stere_just_polar', O.stere(-(90 - 0.5e-8), 5.0))], ids=lambda v: v if isinstance(v, str) else '')
def test_host_constants_against_mpmath(name, P):
    """Every constant within 8 eps of its mpmath value, relative (sin chi1, cos chi1: of 1 as well — they are direction
    cosines): a constant is the result of about ten roundings of half an eps and a few library functions of one."""
    p, want = _constants(P), O.constants(MP, P)
    assert p.kind == (2 if P['kind'] == 'paeqd' else 1)
    assert p.mode == want['mode']
    if P['kind'] == 'stere':
        assert (p.mode != 0) == (90 - abs(P['lat0']) < 1e-8), name
    assert (p.lat0, p.lon0, p.a) == (P['lat0'], P['lon0'], P['a'])
    for key in ('e', 'sin_chi1', 'cos_chi1', 'm1', 'k'):
        got, ref = getattr(p, key), want[key]
        tol = 8 * EPS * (abs(float(ref)) if key in ('e', 'm1', 'k') else max(abs(float(ref)), 0.0))
        assert abs(MP.num(got) - ref) <= tol, (name, key, got, float(ref), float(abs(MP.num(got) - ref)) / EPS)
    if p.mode:
        assert (p.sin_chi1, p.cos_chi1, p.m1) == (float(p.mode), 0.0, 0.0)


def test_polar_switch():
    assert _constants(O.stere(90 - 2e-8, 0.0)).mode == 0
    assert _constants(O.stere(90 - 0.5e-8, 0.0)).mode == 1
    assert _constants(O.stere(-90 + 0.5e-8, 0.0)).mode == -1
    assert _constants(O.stere(-90.0, 0.0)).mode == -1
    assert _constants(O.stere(0.0, 0.0)).mode == 0


def test_bad_arguments_are_einval():
    from auromat_amd._native import Projection
    L, p = _lib(), Projection()
    nan, inf = float('nan'), float('inf')
    for args in ((90.0000001, 0, 6378.137, 6356.75), (-91, 0, 6378.137, 6356.75), (nan, 0, 6378.137, 6356.75),
                 (10, inf, 6378.137, 6356.75), (10, nan, 6378.137, 6356.75), (10, 0, 6356.0, 6378.0), (10, 0, 0.0, 0.0),
                 (10, 0, -1.0, -2.0), (10, 0, inf, 1.0), (10, 0, 6378.137, nan), (10, 0, 6378.137, 0.0)):
        assert L.amt_projection_stereographic(*[float(v) for v in args], C.byref(p)) == -1, args
    assert L.amt_projection_stereographic(10.0, 0.0, 6378.137, 6356.75, None) == -1
    for args in ((1, nan, 6370.997), (1, inf, 6370.997), (0, 180.0, 0.0), (0, 180.0, -5.0), (1, 180.0, nan), (1, 180.0, inf)):
        assert L.amt_projection_polar_aeqd(args[0], float(args[1]), float(args[2]), C.byref(p)) == -1, args
    assert L.amt_projection_polar_aeqd(1, 180.0, 6370.997, None) == -1
    assert L.amt_projection_stereographic(10.0, 0.0, 6378.137, 6378.137, C.byref(p)) == 0 and p.e == 0.0      # a sphere
    from auromat_amd.coordinates.projection import PolarAzimuthalEquidistant, Stereographic
    with pytest.raises(ValueError):
        Stereographic(91, 0)
    with pytest.raises(ValueError):
        PolarAzimuthalEquidistant(True, radius=0)
    assert PolarAzimuthalEquidistant(False).north is False and Stereographic(-90, 3).params.mode == -1


CASES = K.cases()


def test_the_cases_cover_the_issue():
    assert set(c['family'] for c in CASES) == set(K.FAMILIES)
    centres = set((c['projection']['lat0'], c['projection']['lon0']) for c in CASES if c['projection']['kind'] == 'stere')
    assert centres == set(K.CENTRES)
    assert sorted(c['lat'].size for c in CASES if c['family'].startswith('len_')) == sorted(K.LENGTHS)
    assert set(c['projection']['kind'] for c in CASES) == {'stere', 'paeqd'}


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_case_aims_where_it_claims(case):
    """Which points are outside the domain is certain: D (mpmath, on the float64 inputs) keeps at least 5e-13 from 1 — the
    float64 arithmetic of a kernel is 1e-16 from it —, the limit families sit at 1 +- 1e-12 on their sides, 'near' is 1e-9 degrees
    from the centre, and the three number types agree on the NaN pattern, which is the domain rule plus the non-finite inputs."""
    P, fam = case['projection'], case['family']
    finite = np.isfinite(case['lat']) & np.isfinite(case['lon'])
    D = np.array([float(O.domain_D(MP, P, la, lo)) if ok else np.nan for la, lo, ok in zip(case['lat'], case['lon'], finite)])
    assert np.all(np.abs(D[finite] - 1) >= 5e-13), (case['name'], D)
    if fam == 'limit_in':
        assert np.all((D - 1 > 0.5e-12) & (D - 1 < 2e-12)), D - 1
    if fam == 'limit_out':
        assert np.all((1 - D > 0.5e-12) & (1 - D < 2e-12)), D - 1
    if fam in ('centre', 'near'):
        assert np.all(np.abs(D - 2) < 1e-15)                   # (1e-9 degrees away: 2 - D = 1.5e-22)
    if fam == 'near':
        x, y = K.reference(case, 'forward')
        rho = np.hypot(x.astype(np.float64), y.astype(np.float64))
        assert np.all(np.abs(rho / (P['a'] * np.deg2rad(1e-9)) - 1) < 0.01), rho
    if fam == 'nonfinite':
        assert not finite.any()
    if fam == 'dateline':
        assert np.all(np.abs(np.abs(case['lon']) - 180) < 1e-13)
    if fam.startswith('len_') or fam == 'limit_in' or fam == 'near' or fam == 'centre':
        assert np.all(D >= 1)
    if fam == 'spread':
        assert (D < 1).sum() >= 4 and (D > 1).sum() >= 30
    ref = K.reference(case, 'forward')
    want_nan = ~finite | (np.nan_to_num(D, nan=0.0) < 1)
    for xp in (F64, LD):
        got = O.points(xp, O.forward, P, case['lat'], case['lon'])
        for g, r in zip(got, ref):
            assert np.array_equal(np.isnan(g), want_nan) and np.array_equal(np.isnan(r), want_nan), (case['name'], xp.name)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_forward_then_inverse_is_the_identity_in_mpmath(case):
    """inverse(forward(p)) = p to 1e-40 degrees of arc in mpmath, the plane point handed on unrounded"""
    P = case['projection']
    mp = MP.mp
    for la, lo in zip(case['lat'], case['lon']):
        if not (np.isfinite(la) and np.isfinite(lo)):
            continue
        x, y = O.forward(MP, P, la, lo)
        if mp.isnan(x):
            continue
        la2, lo2 = _inverse_unrounded(P, x, y)
        assert abs(la2 - MP.num(la)) < mp.mpf(10) ** -40, (case['name'], la, lo, la2)
        if abs(la) < 90:
            d = (lo2 - MP.num(lo) + 180) % 360 - 180
            # (a longitude of 180 comes back as -180; within 1e-40 degrees of arc on the parallel)
            assert abs(d) * mp.cos(MP.num(la) * mp.pi / 180) < mp.mpf(10) ** -40, (case['name'], la, lo, lo2)


class _Exact(O.MultiPrecision):
    def num(self, v):
        return v if isinstance(v, self.mp.mpf) else self.mp.mpf(float(v))


def _inverse_unrounded(P, x, y):
    """O.inverse on mpmath numbers as they are (xp.num would round them to float64)"""
    xp = _Exact()
    return O.inverse(xp, P, xp.mp.mpf(x), xp.mp.mpf(y))


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_longdouble_against_mpmath(case):
    """The longdouble statement keeps within 64 longdouble eps of the scale of the mpmath one, both directions (its eps is
    2^-63; the textbook form loses up to 1 / cos(chi1) at a centre one degree from a pole: 57)."""
    eps_ld = float(np.finfo(np.longdouble).eps)
    for direction in ('forward', 'inverse'):
        inp = (case['lat'], case['lon']) if direction == 'forward' else K.inverse_inputs(case)
        got = O.points(LD, getattr(O, direction), case['projection'], *inp)
        ref = K.reference(case, direction)
        for (dist, eps_scale), g, r in zip(K.distances_and_scales(case, direction, got, ref), got, ref):
            assert np.array_equal(np.isnan(g), np.isnan(r)), (case['name'], direction)
            ok = ~np.isnan(dist)
            assert np.all(dist[ok] <= 64 * eps_ld * (eps_scale[ok] / K.EPS)), (case['name'], direction,
                                                                             float(np.max(dist[ok] / (eps_scale[ok] / K.EPS))) / eps_ld)


# ---- the host rules of the public functions -------------------------------------------------------------------------------------
def test_resolution_and_edges():
    from auromat_amd import resample as R
    # 100 arcsec of arc on the equator: 6378.137 km * (100 / 3600 deg) * pi / 180 = 3.09220807759... km
    assert abs(R.projected_km_per_px(None, 100) - 3.0922080775909) < 1e-12
    assert R.projected_km_per_px(10, 100) == 10.0 and R.projected_km_per_px(2.5, None) == 2.5
    assert abs(R.projected_km_per_px(None, 3600) - 6378.137 * np.pi / 180) < 1e-12
    # the 747 x 728 km map of the issue: 75 x 73 cells at 10 km, 242 x 236 at 100 arcsec
    ex, ey = R.projected_edges(747.0, 10.0), R.projected_edges(728.0, 10.0)
    assert len(ex) == 76 and len(ey) == 74
    assert np.array_equal(ex, np.arange(-375.0, 376.0, 10.0)) and np.array_equal(ey, np.arange(-365.0, 366.0, 10.0))
    km = R.projected_km_per_px(None, 100)
    assert len(R.projected_edges(747.0, km)) == 243 and len(R.projected_edges(728.0, km)) == 237
    e = R.projected_edges(747.0, km)
    assert e[0] == -121 * km and e[-1] == 121 * km and np.array_equal(e, np.linspace(-242 * km / 2, 242 * km / 2, 243))
    assert len(R.projected_edges(30.0, 10.0)) == 4 and len(R.projected_edges(30.000001, 10.0)) == 5
    for extent in (0.0, -5.0, float('nan')):
        with pytest.raises(ValueError):
            R.projected_edges(extent, 10.0)
    for bad in (dict(kmPerPx=-1), dict(kmPerPx=None, arcsecPerPx=0), dict(kmPerPx=float('inf'))):
        with pytest.raises(ValueError):
            R.projected_km_per_px(**bad)


def test_stereographic_geometry():
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import BoundingBox
    a, b = BoundingBox(60.0, -10.0, 70.0, 10.0), BoundingBox(64.0, 5.0, 75.0, 30.0)
    merged = BoundingBox(60.0, -10.0, 75.0, 30.0)
    got = R.stereographic_geometry([a, b])
    want = (merged.center.lat, merged.center.lon, merged.size.width * 1.05, merged.size.height * 1.05)
    assert got == want
    # the merged box: 40 degrees of longitude along 60 N, the equatorward and longer edge, are about 2200 km
    assert 2100 < got[2] / 1.05 < 2300 and 60 < got[0] < 75 and abs(got[1] - 10.0) < 1e-12
    assert R.stereographic_geometry([a, b], sizeFactor=2)[2:] == (want[2] * 2, want[3] * 2)
    assert R.stereographic_geometry([a], boundingBox=b)[:2] == (b.center.lat, b.center.lon)
    assert R.stereographic_geometry([a], lat0=1, lon0=2)[:2] == (1.0, 2.0)
    assert R.stereographic_geometry([a], lat0=1, lon0=2)[2:] == (a.size.width * 1.05, a.size.height * 1.05)

    def boom():
        raise AssertionError('the boxes are not looked at when nothing is missing')
        yield
    assert R.stereographic_geometry(boom(), 1, 2, 300, 400) == (1.0, 2.0, 300.0, 400.0)


def test_polar_geometry():
    from auromat_amd import resample as R
    Rk = 6370.997
    # north: bounding latitude 60 - 5; half width R * 35 deg in radians = 3891.82 km
    north, bounding, half = R.polar_geometry(60.0, 80.0, Rk)
    assert (north, bounding) == (True, 55.0) and abs(half - 3891.8206) < 1e-3 and half == Rk * 35 * np.pi / 180
    assert R.polar_geometry(-80.0, -60.0, Rk) == (False, -55.0, Rk * 35 * np.pi / 180)
    # a range centred on the equator is a south polar map (the reference's `> 0`), bounding latitude latNorth + 5
    assert R.polar_geometry(-10.0, 10.0, Rk) == (False, 15.0, Rk * 75 * np.pi / 180)
    assert R.polar_geometry(-10.0, 10.5, Rk)[:2] == (True, -15.0)


def test_public_functions_check_their_arguments_first():
    from auromat_amd import resample as R
    for fn in (R.resampleStereographic, R.resampleStereographicMLatMLT, R.resampleMLatMLTPolar):
        for bad in (-0.1, 1.5, float('nan')):
            with pytest.raises(ValueError):
                fn(object(), minCoverage=bad)
    with pytest.raises(ValueError):
        R.resampleStereographic([])
    with pytest.raises(ValueError):
        R.resampleStereographic(object())


# ---- the image writer -----------------------------------------------------------------------------------------------------------
class _Img(object):
    def __init__(self, img):
        self.img = img


@pytest.mark.parametrize('dtype,nch', [(np.uint8, 3), (np.uint16, 3), (np.uint8, 1), (np.uint16, 1), (np.uint8, 4)])
def test_save_map_image(tmp_path, dtype, nch):
    from PIL import Image
    from auromat_amd.draw import saveMapImage
    rng = np.random.RandomState(3)
    data = rng.randint(0, int(np.iinfo(dtype).max) + 1, (7, 9, nch)).astype(dtype)
    mask = rng.rand(7, 9) < 0.3
    mask[0, 0], mask[6, 8] = True, False
    img = ma.masked_array(data, mask=np.repeat(mask[:, :, None], nch, 2))
    path = str(tmp_path / 'map.png')
    saveMapImage(_Img(img), path)
    back = np.asarray(Image.open(path))
    assert back.shape == (7, 9, 4) and back.dtype == np.uint8
    assert np.array_equal(back[:, :, 3], np.where(mask, 0, 255))
    want = (data >> 8).astype(np.uint8) if dtype == np.uint16 else data
    want = np.repeat(want, 3, axis=2) if nch == 1 else want[:, :, :3]
    assert np.array_equal(back[:, :, :3][~mask], want[~mask])
    assert not back[:, :, :3][mask].any()
