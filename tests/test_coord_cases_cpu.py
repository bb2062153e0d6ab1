"""
No GPU: the constructed inputs of tests/_coord_cases.py hold what they claim, and the references of tests/_coord_oracle.py that
tests/test_gpu_coord_ops.py compares the operator kernels of amt_coords.hip with are right — the longdouble run of every
operation equals the mpmath run (50 digits) to 1e-15 of the output's scale (90 or 180 deg, the largest coordinate in km, 1 for unit
vectors), under a derived, looser tolerance where a ray all but grazes; the float64 oracle (oracle/ref_numpy.py,
coordinates.wcs.zenithal_pix2world) has the reference's NaN and boolean patterns on every case; no ray is closer to a decision
than the margins of the cases module; every point that reaches Bowring's formula lies outside the evolute.

The truncation error of one-step Bowring ITSELF (test_truncation_of_one_step_bowring; documentation of the algorithm that kernel
and reference share, no assertion about the kernel): on the geodetic family the one-step latitude is at most 1.3e-11 deg from
the Bowring iteration run to convergence in mpmath on WGS84 (heights 0 to 1000 km), and 3.6e-4 deg on the ellipsoid with b / a = 0.9.
"""
import numpy as np
import pytest

import _coord_cases as K
import _coord_oracle as Q
import _rowfield_oracle as R
from oracle import ref_numpy as O


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- what the families claim ----------------------------------------------------------------------------------------------------
def test_lengths_cover_every_entry_point():
    fam = K.family('lengths')
    assert {c['op'] for c in fam} == set(Q.OPS) and len(Q.OPS) == 19
    for op in Q.OPS:
        n = sorted({Q.n_points(op, c['args']) for c in fam if c['op'] == op})
        if op == 'georef_allsky':
            assert n == sorted({s * s for s in K.ALLSKY_LENGTH_SIZES} | {(s + 1) ** 2 for s in K.ALLSKY_LENGTH_SIZES})
            assert 1 in n and 64 in n and 256 in n and any(64 < v < 128 for v in n) and any(256 < v < 320 for v in n)
        else:
            assert n == [v for v in K.LENGTHS if v or op not in K.GRID_OPS], op
    assert any(c['op'] == 'rotate_pole' for c in fam) and any(c['op'] == 'rotate_pole_deg' for c in fam)   # both instances
    assert any(c['args'].get('with_r') is False for c in fam) and any(c['op'] == 'spherical_to_cartesian' and c['args']['r'] is None
                                                                      for c in fam)


def test_stride_needs_a_second_trip_through_the_grid():
    fam = K.family('stride')
    assert [c['op'] for c in fam] == ['rotate_vectors', 'ecef_to_geodetic', 'intersects_ellipsoid']
    for c in fam:
        assert Q.n_points(c['op'], c['args']) == 4096 * 256 + 257
    assert all(len(K.family(f)) == 0 or max(Q.n_points(c['op'], c['args']) for c in K.family(f)) <= 4000
               for f in K.FAMILIES if f != 'stride')


def bowring_points(c):
    """the float64 ECEF points an operation hands to Bowring's formula, or None"""
    op, A = c['op'], c['args']
    with np.errstate(invalid='ignore', divide='ignore'):
        if op == 'ecef_to_geodetic':
            return np.stack((A['x'], A['y'], A['z']), axis=-1), A['a'], A['b']
        if op == 'rotate_to_latlon':
            return O.rotate_vectors(f64(A['m']).reshape(3, 3), np.array(A['xyz'])), A['a'], A['b']
        if op in ('rotate_pole', 'rotate_pole_deg'):
            lat, lon = (A['lat'], A['lon']) if op == 'rotate_pole' else (np.deg2rad(A['lat']), np.deg2rad(A['lon']))
            g = np.asarray(O.geodetic_to_ecef(lat, lon, A['altitude'], A['a'], A['b'])).T
            return O.rotate_vectors(f64(A['rot']).reshape(3, 3), g), A['a'], A['b']
        if op == 'sm_to_latlon':
            s = np.asarray(O.spherical_to_cartesian(1, np.deg2rad(A['smlat']), np.deg2rad(A['smlon']))).T
            return O.rotate_vectors(f64(A['m']).reshape(3, 3), s), A['a'], A['b']
        if op == 'georef_allsky':
            d = Q.float64_oracle(op, A)['dirs']
            return O.ellipsoid_line_intersection(A['a'], A['b'], A['station'], d), A['a0'], A['b0']
        if op == 'reproject_altitude':
            cam = np.array(O.geodetic_to_ecef_zero(np.deg2rad(A['station_lat']), np.deg2rad(A['station_lon'])))
            g = np.asarray(O.geodetic_to_ecef(np.deg2rad(A['lat']), np.deg2rad(A['lon']), A['height_ref'])).T
            return O.ellipsoid_line_intersection(A['a'] + A['height_new'], A['b'] + A['height_new'], cam, g - cam), A['a'], A['b']
    return None


@pytest.mark.parametrize('fam', K.FAMILIES)
def test_every_point_lies_outside_the_evolute(fam):
    """p > e^2 a cos^3 u wherever the latitude is a number: arctan(num / den) and atan2(num, den) are then the same angle"""
    seen = 0
    for c in K.family(fam):
        got = bowring_points(c)
        if got is None:
            continue
        g, a, b = got
        if len(g) == 0:
            continue
        with np.errstate(invalid='ignore', divide='ignore'):
            margin = Q.evolute_margin(Q._LD, tuple(np.asarray(g[:, i], dtype=np.longdouble) for i in range(3)), a, b)
        lat = K.reference(c['name'])['lat']
        assert np.array_equal(np.isnan(margin), np.isnan(lat)), c['name']
        assert np.all(margin[~np.isnan(lat)] > 0), c['name']
        seen += 1
    assert seen or fam in ('rays', 'wcs')


def test_geodetic_family_holds_its_edges():
    fam = K.family('geodetic')
    for tag, a, b in K.ELLIPSOIDS:
        for h in K.HEIGHTS:
            c = K.by_name('geodetic-to-ecef-%s-%g' % (tag, h))
            lat, lon = np.rad2deg(c['args']['lat']), np.rad2deg(c['args']['lon'])
            for k in (3, 6, 9, 12):
                for s in (1, -1):
                    assert (lat == np.rad2deg(np.deg2rad(s * (90.0 - 10.0 ** -k)))).any()
            assert (np.abs(lat) == 90).sum() >= 2 and (lat == 0).sum() >= 2 and np.signbit(c['args']['lat'][lat == 0]).any()
            assert (np.abs(lon) == 180).any() and ((np.abs(lon) < 180) & (np.abs(lon) > 179.9999)).any() and (lon == 0).any()
            r = K.reference('geodetic-from-ecef-%s-%g' % (tag, h))
            assert not np.isnan(r['lat']).any()
            assert np.max(np.abs(f64(r['lat']) - lat)) < (1e-9 if tag == 'wgs84' else 1e-3)      # (one step: the truncation)
        assert abs(b / a - (0.9 if tag == 'flat' else 1 - 1 / 298.257223563)) < 1e-15
        c = K.by_name('geodetic-from-ecef-%s-special' % tag)
        A, r, f = c['args'], K.reference(c['name']), K.float64_oracle(c['name'])
        axis = np.zeros(len(A['x']), bool)
        axis[c['on_axis']] = True
        assert np.array_equal((A['x'] == 0) & (A['y'] == 0), axis)
        assert np.array_equal(np.isnan(r['lat']), axis) and np.array_equal(np.isnan(f['lat']), axis)     # NaN exactly there
        assert not np.isnan(f['lon']).any() and not np.isnan(r['lon']).any()
        half = c['half_turn']
        assert np.all(A['y'][half] == 0) and np.all(A['x'][half] < 0) and np.signbit(A['y'][half]).tolist() == [False, True] * 2
        assert f64(r['lon'])[half].tolist() == [180.0, -180.0, 180.0, -180.0]
        p = np.hypot(A['x'], A['y'])[12:]
        assert sorted(set(np.round(np.log10(p)).astype(int))) == [-9, -7, -5, -3]
    assert len(fam) == 14


def test_rotate_pole_family():
    plus, minus = (f64(m) for _, m in K.ROTATIONS[:2])
    assert plus[1, 1] == plus[2, 2] == np.cos(np.pi / 2) and 0 < plus[1, 1] < 1e-16          # 6.1e-17, not 0
    assert plus[1, 2] == -1 and plus[2, 1] == 1 and minus[1, 2] == 1 and minus[2, 1] == -1 and plus[0, 0] == 1
    from auromat_amd.coordinates.transform import rotation_matrix
    assert np.array_equal(plus, rotation_matrix(np.deg2rad(90), [1, 0, 0])[:3, :3])        # what _rot_x(90) hands over
    assert np.array_equal(minus, rotation_matrix(np.deg2rad(-90), [1, 0, 0])[:3, :3])
    assert np.array_equal(f64(K.ROTATIONS[3][1]), np.eye(3))
    for c in K.family('rotate_pole'):
        A, r = c['args'], K.reference(c['name'])
        lat_in = A['lat'] if c['op'] == 'rotate_pole_deg' else A['lat'] * K.K_RAD2DEG
        lon_in = A['lon'] if c['op'] == 'rotate_pole_deg' else A['lon'] * K.K_RAD2DEG
        assert (np.abs(lat_in) == 90).sum() >= 4 or c['op'] == 'rotate_pole'
        assert (np.abs(np.abs(lat_in) - 90) < 1e-12).sum() >= 4
        assert (np.abs(np.abs(lon_in) - 180) < 1e-12).sum() >= 2 and (np.abs(np.abs(lon_in) - 180) < 1e-8).sum() >= 4
        lat = f64(r['lat'])
        assert not np.isnan(lat).any()
        assert (lat > 90 - 1e-5).any() and (lat < -90 + 1e-5).any(), c['name']              # points taken to both poles
        assert A['altitude'] in K.HEIGHTS
    # the rad cases are the deg cases times kDeg2Rad, the products NumPy's
    for c in K.family('rotate_pole'):
        if c['op'] == 'rotate_pole':
            d = K.by_name(c['name'][:-3] + 'deg')['args']
            assert np.array_equal(c['args']['lat'], d['lat'] * K.K_DEG2RAD) and np.array_equal(c['args']['lon'], d['lon'] * K.K_DEG2RAD)


@pytest.mark.parametrize('case', K.family('rays'), ids=lambda c: c['name'])
def test_rays_keep_their_margins_and_do_what_their_tags_say(case):
    A, r, tags = case['args'], K.reference(case['name']), np.array(case['tags'])
    directed, origin = bool(A['directed']), f64(A['origin'])
    rel, t = f64(r['rel']), f64(r['t'])
    is_nan = tags == 'nan'
    assert is_nan.sum() == (0 if 'nonunit' in case['name'] else 2) and np.array_equal(np.isnan(rel), is_nan) and np.isnan(A['dirs'][is_nan]).any(axis=1).all()
    assert np.all(np.abs(rel[~is_nan]) >= 1e-9)                              # no ray grazes
    length = np.sqrt((A['dirs'] ** 2).sum(axis=1))
    hits_line = rel > 0
    if directed:
        # (t in units of the direction's length: a distance of t |d| along the ray)
        dist = np.abs(t * length)[hits_line & ~is_nan]
        assert np.all(dist >= 1e-9 * np.sqrt(origin @ origin))
    elif origin.any():
        d_o, root = f64(r['d_o']), f64(r['root'])
        ok = hits_line & ~is_nan
        assert np.all(np.abs(d_o[ok]) >= 1e-9 * root[ok])                     # which root is nearer is beyond doubt
    else:
        assert np.all(f64(r['d_o'])[~is_nan] == 0)                            # the centre: |t1| == |t2| exactly
        assert np.all(t[~is_nan] > 0)                                         # ... and the reference takes t2
    inside = case['name'].split('-')[2] in ('inside', 'centre')
    out = r['hit'] if case['op'] == 'intersects_ellipsoid' else ~np.isnan(r['xyz']).any(axis=1)
    if case['op'] == 'intersects_ellipsoid' and directed:
        pass
    for tag in set(tags):
        m = tags == tag
        if tag == 'nan':
            assert not out[m].any()
        elif tag in ('outside-cone', 'away-outside-cone'):
            assert not out[m].any() and np.all(rel[m] < 0) and np.all(np.abs(rel[m]) < 1e-4)
        elif tag == 'inside-cone':
            assert out[m].all() and np.all(rel[m] > 0) and np.all(rel[m] < 1e-4)
        elif tag in ('away', 'long-away', 'away-inside-cone'):
            # directed from outside: nothing ahead; from inside: the shell is all around; undirected: the hit behind (t < 0)
            assert out[m].all() == (inside or not directed) and out[m].any() == (inside or not directed)
            if not directed and not inside:
                assert np.all(t[m] < 0)
        else:
            assert out[m].all(), tag
    if 'nonunit' in case['name']:
        assert np.all(np.abs(length[~is_nan] - (1 + 2.0 ** -10)) < 1e-15)
    elif case['op'] == 'intersect_sphere':
        assert np.all(np.abs(length[~is_nan] - 1) < 1e-15)
    else:
        assert (np.abs(length / 1e-3 - 1) < 1e-12).sum() == 4 and (np.abs(length / 1e3 - 1) < 1e-12).sum() == 6
    # the float64 oracle decides every ray as the reference does
    f = K.float64_oracle(case['name'])
    got = f['hit'] if case['op'] == 'intersects_ellipsoid' else ~np.isnan(f['xyz']).any(axis=1)
    assert np.array_equal(got, out)


def test_ray_origins():
    a, b = K.A0 + 110.0, K.B0 + 110.0
    q = lambda o, rad: float(((o / rad) ** 2).sum())
    assert q(K.ORIGIN_OUT, np.array([a, a, b])) > 1 and q(K.ORIGIN_OUT, K.SPHERE_RADIUS) > 1
    assert q(K.ORIGIN_IN, np.array([a, a, b])) < 1 and q(K.ORIGIN_IN, K.SPHERE_RADIUS) < 1
    names = [c['name'] for c in K.family('rays')]
    for op in ('intersect_ellipsoid', 'intersects_ellipsoid', 'intersect_sphere'):
        for where in ('outside', 'inside', 'centre'):
            for kind in ('directed', 'undirected'):
                assert 'rays-%s-%s-%s' % (op, where, kind) in names
    c = K.by_name('rays-intersect_ellipsoid-outside-directed')
    assert {'inside-cone', 'outside-cone', 'short', 'long', 'nan', 'away', 'towards'} <= set(c['tags'])


def test_magnetic_family():
    c = K.by_name('magnetic-mlt-zero')
    r, xyz = K.reference(c['name']), c['args']['xyz']
    m = c['midnight']
    assert np.all(xyz[m, 0] < 0) and np.all(xyz[m, 1] == 0) and np.signbit(xyz[m, 1]).tolist() == [False, True, False, True]
    assert f64(r['mlt'])[m].tolist() == [24.0, 0.0, 24.0, 0.0]
    assert f64(r['mlat'])[c['axis']].tolist() == [90.0, -90.0]
    mlt = f64(r['mlt'])
    assert 23.99 < mlt[7] < 24 and 0 < mlt[8] < 0.01 and abs(mlt[6] - 12) < 1e-9              # beside midnight, and noon
    for i in (0, 1):
        assert np.array_equal(K.by_name('magnetic-j2000-to-mlat-mlt-%d' % i)['args']['m'], O.mat_j2000_to_sm(K.ET[i]))
        assert np.array_equal(K.by_name('magnetic-geo-to-mlat-mlt-%d' % i)['args']['m'], O.mat_geo_to_sm(K.ET[i]))
        assert np.array_equal(K.by_name('magnetic-sm-to-latlon-%d' % i)['args']['m'], O.mat_geo_to_sm(K.ET[i]).T)
        A = K.by_name('magnetic-sm-to-latlon-%d' % i)['args']
        assert (np.abs(A['smlat']) == 90).sum() == 2 and (np.abs(A['smlon']) == 180).sum() == 4
    assert not np.array_equal(K.M_SM[0], K.M_SM[1])
    from auromat_amd.coordinates.transform import mat_geo_to_sm, mat_j2000_to_sm
    assert np.array_equal(mat_j2000_to_sm(K.ET[0]), K.M_SM[0]) and np.array_equal(mat_geo_to_sm(K.ET[1]), K.M_GEO_SM[1])


def test_wcs_family():
    from auromat_amd.coordinates.wcs import celestial_rotation
    for w, h in K.WCS_TAN_SIZES:
        for corner in (0, 1):
            A = K.by_name('wcs-tan-grid-%dx%d-corner%d' % (w, h, corner))['args']
            assert (A['width'], A['height'], A['corner']) == (w, h, corner) and len(A['row']) == (w + corner) * (h + corner)
            assert np.array_equal(A['rot'], celestial_rotation(A['header']))
        for origin in (0, 1):
            A = K.by_name('wcs-tan-points-%dx%d-origin%d' % (w, h, origin))['args']
            assert len(A['px']) == w * h and A['origin'] == origin
            assert A['px'][0] - origin - A['crpix'][0] + 1 == 0 and A['py'][0] - origin - A['crpix'][1] + 1 == 0
    # the reference pixel itself: the direction there is the third column of the rotation (r = 0, theta = 90 deg)
    for c in K.family('wcs'):
        A, r = c['args'], K.reference(c['name'])
        if c['op'] == 'directions_tan' and not A['corner']:
            i = int(A['crpix'][1] - 1) * A['width'] + int(A['crpix'][0] - 1)
            assert np.max(np.abs(f64(r['dirs'][i]) - f64(A['rot'])[:, 2])) < 1e-16
        if c['op'] == 'directions_zenithal':
            w = A['w']
            native_z = f64(r['dirs']) @ f64(list(w.rot)).reshape(3, 3)[:, 2]
            if c.get('crpix_on_pixel'):
                assert (A['col'] + w.start_x - w.crpix[0] + 1 == 0).any() and (A['row'] + w.start_y - w.crpix[1] + 1 == 0).any()
                assert native_z.max() > 1 - 1e-16
            if Q.ZENITHAL[w.projection] in ('SIN', 'ZEA'):
                # cos(theta) = r / k for SIN: within 0.9 of the rim; ZEA's r / 2k = sin((90 - theta) / 2) is far below it
                assert np.sqrt(1 - native_z.min() ** 2) < 0.9
            assert (w.sip_order_a, w.sip_order_b) == (c['orders'] or (0, 0))
            assert not np.isnan(r['dirs']).any()
    zen = [c for c in K.family('wcs') if c['op'] == 'directions_zenithal']
    assert {(Q.ZENITHAL[c['args']['w'].projection], c['args']['w'].width, c['args']['w'].height) for c in zen} >= \
        {(p, w, h) for p in Q.ZENITHAL for w, h in K.WCS_ZEN_SIZES}
    orders = {c['orders'] for c in zen}
    assert {(3, 2), (0, 4), (9, 9), (2, 0), None} <= orders
    assert any(c['args']['w'].start_x != 0 and c['args']['w'].start_y != 0 for c in zen)
    assert {c['args']['w'].corner for c in zen} == {0, 1}
    # the SIP terms matter: without them the directions move by far more than any bound
    c = K.by_name('wcs-zenithal-TAN-sip-9-9')
    plain = Q.run(Q._LD, 'directions_zenithal', dict(c['args'], sip=False))['dirs']
    assert np.max(np.abs(f64(plain - K.reference(c['name'])['dirs']))) > 1e-4


def test_allsky_family():
    from auromat_amd.coordinates.transform import Y, Z, rotation_matrix
    sizes, low, high = set(), False, False
    for c in K.family('allsky'):
        A, r = c['args'], K.reference(c['name'])
        sizes.add(A['size'])
        # the matrix mapping.miracle.allsky_params hands over (its station comes from the device: the GPU test compares that)
        to_geo = np.dot(rotation_matrix(np.deg2rad(-A['cal']['lon']), Z)[:3, :3], rotation_matrix(np.deg2rad(90 - A['cal']['lat']), Y)[:3, :3])
        assert np.array_equal(to_geo, A['to_geo'])
        assert (A['xc'], A['yc'], A['k']) == tuple(A['cal'][k] * (A['size'] / 512) for k in ('xc', 'yc', 'k'))
        n = A['size'] + A['corner']
        az, el = f64(r['az']).reshape(n, n), f64(r['el']).reshape(n, n)
        assert not any(np.isnan(r[k]).any() for k in ('az', 'el', 'dirs', 'lat', 'lon'))
        assert np.all((az >= 0) & (az < 360))
        edge = np.minimum(az, 360 - az)
        assert np.all((edge > 1e-9) | (az == 0))                      # the floor of the wrap is beyond doubt
        if c['zenith'] is not None:
            off = 0.0 if A['corner'] else 0.5
            i, j = int(c['zenith'][0] - off), int(c['zenith'][1] - off)
            assert (i + off == A['xc']) and (j + off == A['yc']) and el[i, j] == 90.0
        low, high = low or bool((az < 20).any()), high or bool((az > 340).any())
        if A['rotation'] == 7.0:
            raw = np.rad2deg(np.arctan2(A['col'] - A['yc'], -(A['row'] - A['xc'])) - 7.0)
            assert (raw < -360).any()                                 # more than one turn to take off
    assert sizes == {1, 2, 33} and low and high
    assert {c['args']['corner'] for c in K.family('allsky')} == {0, 1}
    assert ('az',) in K.ALLSKY_SUBSETS and ('dirs',) in K.ALLSKY_SUBSETS and ('lat',) in K.ALLSKY_SUBSETS


def test_themis_family():
    fam = K.family('themis')
    assert {c['args']['height_new'] for c in fam} == {90.0, 110.0, 150.0} and {c['args']['height_ref'] for c in fam} == {110.0}
    assert sorted({c['args']['station_lat'] for c in fam}) == [45.3, 78.1]
    for c in fam:
        A, r = c['args'], K.reference(c['name'])
        assert A['lat'][0] == A['station_lat'] and A['lon'][0] == A['station_lon']              # the station's own zenith
        assert abs(float(r['lat'][0]) - A['station_lat']) < 1e-9             # (to the truncation of one Bowring step)
        x = K.ecef(A['lat'], A['lon'], 0.0)
        angle = np.degrees(np.arccos(np.clip((K.unit(x) * K.unit(x[0])).sum(axis=1), -1, 1)))
        assert (np.abs(angle[1:9] - 8.0) < 0.5).all()                  # 8 deg away (the offsets are laid out on a flat map)
        assert not np.isnan(r['lat']).any()
        if A['height_new'] == A['height_ref']:
            # the same height: the reference points come back, as far as the shell (a + h, b + h) is the surface of height h
            assert np.max(np.abs(f64(r['lat']) - A['lat'])) < 1e-5


# ---- the references ---------------------------------------------------------------------------------------------------------
def _sample(fam, n=120):
    pts = [(c['name'], i) for c in K.family(fam) for i in range(min(Q.n_points(c['op'], c['args']), 400))]
    if len(pts) <= n:
        return pts
    rng = np.random.RandomState(7)
    keep = set(rng.choice(len(pts), size=n, replace=False).tolist()) | {0, len(pts) - 1}
    if fam == 'rays':                                          # every ray beside the tangent cone
        keep |= {k for k, (name, i) in enumerate(pts) if 'cone' in K.by_name(name)['tags'][i]}
    if fam == 'geodetic':
        keep |= {k for k, (name, i) in enumerate(pts) if name.endswith('special')}
    return [pts[k] for k in sorted(keep)]


def _scale(c, name, kind):
    return K.scale(c['family'], c['op'], name)


@pytest.mark.parametrize('fam', K.FAMILIES)
def test_longdouble_reference_equals_mpmath(fam):
    """longdouble THROUGHOUT against mpmath at every sampled point: 1e-15 of the output's scale; where a ray all but grazes
    (|rel| < 1e-3: the root of a discriminant that has lost 1 / rel of its digits) sqrt(1e-3 / |rel|) times that."""
    assert float(np.finfo(np.longdouble).eps) < 2e-19, 'np.longdouble is not the 80-bit type here'
    pts = _sample(fam)
    assert len(pts) >= 60
    worst, loose = {}, 0
    for name, i in pts:
        c = K.by_name(name)
        raw, ref = K.reference_longdouble(name), K.reference(name)
        m = Q.reference_mp(c['op'], c['args'], i)
        graze = 1.0
        if 'rel' in raw and abs(float(raw['rel'][i])) < Q.GRAZING:
            graze = float(np.sqrt(Q.GRAZING / abs(float(raw['rel'][i]))))
        for out, kind in K.outputs(c):
            if kind == 'hit':
                assert bool(raw[out][i]) == bool(m[out]), (name, i)
                continue
            d = Q.mp_distance(raw[out][i], m[out])
            if kind in ('lon', 'mlt', 'az') and np.isfinite(d):
                period = 24.0 if kind == 'mlt' else 360.0
                d = min(d, abs(period - d))                   # a signed zero: +180 here, -180 there
                if kind != 'az':
                    partner = f64(raw['lat' if kind == 'lon' else 'mlat'][i])
                    if np.isnan(partner):
                        continue          # on the axis: atan2 of two signed zeros, 0 or 180 by convention; mpmath has no -0
                    d *= float(np.cos(np.deg2rad(partner))) * (15.0 if kind == 'mlt' else 1.0)
            tol = 1e-15 * _scale(c, out, kind) * graze
            assert d <= tol, (name, out, i, d, tol)
            worst[c['op'], out] = max(worst.get((c['op'], out), 0.0), d / tol)
            if graze > 1:
                loose += 1
                assert Q.mp_distance(ref[out][i], m[out]) <= 1e-17 * _scale(c, out, kind), (name, out, i)   # substituted
    print(fam, len(pts), 'points; largest distance / tolerance:', ' '.join('%s.%s %.2g' % (k + (v,)) for k, v in sorted(worst.items())))
    assert loose or fam != 'rays'


@pytest.mark.parametrize('case', K.cases(), ids=lambda c: c['name'])
def test_float64_oracle_has_the_reference_patterns(case):
    r, f = K.reference(case['name']), K.float64_oracle(case['name'])
    n = Q.n_points(case['op'], case['args'])
    for out, kind in K.outputs(case):
        assert f[out].shape == r[out].shape == ((n, 3) if out in ('xyz', 'dirs') else (n,)), (out, f[out].shape, r[out].shape)
        if kind == 'hit':
            assert np.array_equal(np.asarray(f[out], bool), np.asarray(r[out], bool))
        else:
            assert np.array_equal(np.isnan(f[out]), np.isnan(r[out])), out


def test_bounds_come_from_the_float64_oracle():
    for fam in K.FAMILIES:
        for op, out in K.keys(fam):
            e, s = K.e_ref(fam, op, out), K.scale(fam, op, out)
            seed = 4.1e-15 * s if Q.seeded(op, out) else 0.0
            assert K.bound(fam, op, out) == 8 * max(e, R.EPS * s, seed)
            assert e < 1e-12 * s or fam == 'rays'              # the float64 oracle is nowhere worse, but beside the tangent cone
            assert s in (90.0, 180.0, 1.0) or 5000 < s < 8000
    assert Q.seeded('georef_allsky', 'lat') and not Q.seeded('georef_allsky', 'az') and not Q.seeded('rotate_to_mlat_mlt', 'mlt')
    assert not Q.seeded('intersect_ellipsoid', 'xyz') and not Q.seeded('cartesian_to_spherical', 'lat')


def test_truncation_of_one_step_bowring():
    """How far one step of Bowring's iteration (what transform.py, the oracle and the kernel compute) is from the iteration run
    to convergence, in mpmath, on the geodetic family: the figures of the module docstring."""
    xp = R._mp()
    mp = xp.mp
    worst = {}
    for c in K.family('geodetic'):
        if c['op'] != 'ecef_to_geodetic':
            continue
        A = c['args']
        a, b = mp.mpf(A['a']), mp.mpf(A['b'])
        e2a, dd = (a * a - b * b) / a, (a * a - b * b) / b
        for i in range(len(A['x'])):
            x, y, z = (mp.mpf(float(A[k][i])) for k in 'xyz')
            p = mp.sqrt(x * x + y * y)
            if p == 0:
                continue
            tu = b * z * (1 + dd / mp.sqrt(p * p + z * z)) / (a * p)
            first = None
            for _ in range(60):
                cu = 1 / mp.sqrt(1 + tu * tu)
                su = tu * cu
                lat = mp.atan2(z + dd * su ** 3, p - e2a * cu ** 3)
                if first is None:
                    first = lat
                tu = (b / a) * mp.tan(lat) if abs(lat) < mp.pi / 2 else tu
            one = Q._geodetic(xp, (x, y, z), A['a'], A['b'])[0]
            assert abs(mp.degrees(first) - one) < mp.mpf(10) ** -40          # the oracle's geodetic_deg IS that first step
            tag = 'flat' if A['b'] == K.FLAT_B else 'wgs84'
            worst[tag] = max(worst.get(tag, 0.0), float(abs(mp.degrees(lat - first))))
    print('one-step Bowring against the converged iteration, degrees:', worst)
    assert set(worst) == {'wgs84', 'flat'}
