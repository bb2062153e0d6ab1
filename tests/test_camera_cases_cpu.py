"""
No GPU: the constructed cameras of tests/_camera_cases.py hold what they claim, the reference of tests/_camera_oracle.py that
tests/test_gpu_camera_rows.py compares the row kernel with is right — its longdouble run equals the mpmath run (50 digits) on
a sample of points and on every point whose mpmath value it takes, and the float64 oracle gives the same NaN pattern —, no ray
of any case is closer to grazing the shell than r_min(), and the host functions amt_georef_sky_rows / amt_georef_image_rows
are sound and tight on every case: no band they declare sky holds a hit corner or a hit centre (fast or exact) of the
reference, and they leave at most the bands unused that tests/test_sky_rows.py allows.
"""
import ctypes as C

import numpy as np
import pytest

import _camera_cases as K
import _camera_oracle as Q
import _rowfield_oracle as R

BAND = K.BAND


def f64(a):
    return np.asarray(a, dtype=np.float64)


def hits(name):
    return ~np.isnan(K.reference(name)['lat'])


# ---- what the cases claim ------------------------------------------------------------------------------------------------------
def test_families_and_sizes():
    assert [(c['width'], c['height']) for c in K.family('cd')[-len(K.SIZES):]] == list(K.SIZES)
    assert {(c['width'], c['height']) for c in K.family('limb')} == {(62, 50), (70, 83), (130, 49)}
    for name in K.PLAN_NAMES:
        assert name not in K.NO_PLAN and K.by_name(name)['time'] is not None
    assert {K.by_name(n)['family'] for n in K.PLAN_NAMES} >= {'cd', 'wide', 'limb', 'far', 'low', 'exact'}
    for c in K.cases():
        assert set(c) >= {'width', 'height', 'fast_center', 'cd', 'crpix', 'rot', 'cam', 'a', 'b', 'a0', 'b0', 'm_geo', 'm_sm'}
        assert (c['family'] == 'exact') == (c['fast_center'] == 0)


def test_cd_family():
    det = {c['name']: c['cd'][0] * c['cd'][3] - c['cd'][1] * c['cd'][2] for c in K.family('cd')}
    assert det['cd-flipped'] < 0 and all(v > 0 for k, v in det.items() if k != 'cd-flipped')
    for deg in (0, 37, 90, 180):                               # the same boresight rolled: CD(deg) = CD(0) R(deg)
        cd0, cd = (np.array(K.by_name('cd-rotation-%d' % d)['cd']).reshape(2, 2) for d in (0, deg))
        assert np.allclose(cd, cd0 @ K.rot2(deg), atol=1e-15)
    # (a roll multiplies CD by a rotation from the right: its singular values say what the pixel grid is)
    sv = {c['name']: np.linalg.svd(np.array(c['cd']).reshape(2, 2), compute_uv=False) for c in K.family('cd')}
    assert abs(sv['cd-anisotropic'][0] / sv['cd-anisotropic'][1] - 1.6) < 1e-12
    assert np.allclose(sv['cd-sheared'], np.linalg.svd(0.05 * np.array([[1.0, 0.4], [0.0, 1.0]]), compute_uv=False), rtol=1e-12)
    assert sv['cd-sheared'][0] / sv['cd-sheared'][1] > 1.4 and abs(sv['cd-rotation-37'][0] / sv['cd-rotation-37'][1] - 1) < 1e-12
    c = K.by_name('cd-crpix-fraction')
    assert c['crpix'][0] % 1 and c['crpix'][1] % 1
    assert K.by_name('cd-crpix-corner')['crpix'] == (0.5, 0.5)   # pixel coordinates (-1/2, -1/2): the frame's first corner
    assert K.by_name('cd-crpix-outside')['crpix'][1] <= -1000.0
    c = K.by_name('cd-rot-cancels')
    m = f64(c['m_geo']) @ f64(c['rot'])
    off = np.abs(m - np.eye(3))
    assert 0 < off.max() < 1e-15 and (off[~np.eye(3, dtype=bool)] > 0).any()
    for c in K.family('cd'):
        assert hits(c['name']).all()


def conic_of(c):
    """the limb in the image: disc of the un-normalised direction w = rot (-Y, X, 180 / pi), which is affine in the pixel, is a
    quadratic in (x, y); its second-order part decides ellipse (det > 0) / hyperbola (det < 0) -> det / trace^2"""
    pts = np.array([(x, y) for x in (-200.0, 0.0, 300.0) for y in (-150.0, 50.0, 250.0)])
    cd, k = f64(c['cd']), 180.0 / np.pi
    px, py = pts[:, 0] - c['crpix'][0] + 1, pts[:, 1] - c['crpix'][1] + 1
    X, Y = cd[0] * px + cd[1] * py, cd[2] * px + cd[3] * py
    w = np.stack([-Y, X, np.full(len(pts), k)], axis=1) @ f64(c['rot']).T
    rad = np.array([c['a'], c['a'], c['b']])
    ds, os_ = w / rad, -f64(c['cam']) / rad
    d_o, d_d, o_o = ds @ os_, (ds * ds).sum(axis=1), os_ @ os_
    disc = d_o * d_o - o_o * d_d + d_d
    x, y = pts[:, 0] / 100.0, pts[:, 1] / 100.0
    q = np.linalg.lstsq(np.stack([x * x, x * y, y * y, x, y, np.ones_like(x)], axis=1), disc, rcond=None)[0]
    return (q[0] * q[2] - 0.25 * q[1] * q[1]) / (q[0] + q[2]) ** 2


def test_wide_family():
    seen = set()
    for c in K.family('wide'):
        v, conic = conic_of(c), c['claims']['conic']
        print(c['name'], 'det / trace^2 of the limb conic', v, 'gate', c['claims']['gate'])
        assert {'ellipse': v > 0.02, 'near-parabola': abs(v) < 0.02, 'hyperbola': v < -0.02}[conic], (c['name'], v)
        seen.add(conic)
        assert (c['width'], c['height']) == (130, 100) and 0.3 <= c['scale'] <= 0.52
        h = hits(c['name'])
        assert h.any() and not h.all()                            # the limb is in the frame
        na = np.degrees(np.arccos(-K.K.unit(f64(c['cam'])) @ f64(c['rot'])[:, 2]))
        assert 39.9 < na < 100.1
    assert seen == {'ellipse', 'near-parabola', 'hyperbola'}
    gates = {c['scale']: c['claims']['gate'] for c in K.family('wide') if c['name'].startswith('wide-gate')}
    assert gates == {0.5: True, 0.52: False} and K.by_name('wide-hyperbola-70')['claims']['gate']
    c = K.by_name('wide-far-corner')
    d = Q.direction(R._LD, Q.params_of(c), c['width'] - 0.5, c['height'] - 0.5)
    off = np.degrees(np.arccos(float(sum(d[i] * c['rot'][i, 2] for i in range(3)))))
    assert off >= c['claims']['corner_off'], off


@pytest.mark.parametrize('case', [c for c in K.cases() if 'limb_row' in c['claims']], ids=lambda c: c['name'])
def test_limb_extreme_row_is_where_it_says(case):
    rows = np.flatnonzero(hits(case['name']).any(axis=1))
    target = case['claims']['limb_row']
    if case['claims']['earth'] == 'below':
        got, want = rows[0], (np.ceil(target - 1 / 64.0), np.ceil(target + 1 / 64.0))
        assert rows[-1] == case['height']
    else:
        got, want = rows[-1], (np.floor(target - 1 / 64.0), np.floor(target + 1 / 64.0))
        assert rows[0] == 0
    assert want[0] <= got <= want[1], (case['name'], got, target)
    assert len(rows) == rows[-1] - rows[0] + 1
    assert abs(target - round(target / BAND) * BAND) <= 2


def test_limb_family_sides_and_corner():
    offs = {(c['claims']['earth'], c['claims']['limb_row'] - 2 * BAND) for c in K.family('limb') if (c['width'], c['height']) != (130, 49)
            and 'limb_row' in c['claims']}
    assert offs == {(e, o) for e in ('below', 'above') for o in K.LIMB_OFFSETS}
    assert [c['claims']['limb_row'] for c in K.family('limb') if c['width'] == 130] == [2 * BAND - 0.5, 2 * BAND + 0.5]
    for name in ('limb-left', 'limb-right'):
        h = hits(name)
        assert h.any(axis=1).all() and not h.all(axis=1).any()           # every corner row holds hits and misses
    assert hits('limb-left')[:, 0].all() and not hits('limb-left')[:, -1].any()
    assert hits('limb-right')[:, -1].all() and not hits('limb-right')[:, 0].any()
    h = hits('limb-corner')
    assert h[-1, -1] and 1 <= h.sum() <= 10 and not h[:-3].any() and not h[:, :-3].any()


def test_far_family():
    h = hits('far-disc-inside')
    assert h.any() and not (h[0].any() or h[-1].any() or h[:, 0].any() or h[:, -1].any())
    rows = np.flatnonzero(h.any(axis=1))
    assert rows[0] > BAND + 2 and rows[-1] < 21 * BAND - 1, rows[[0, -1]]      # a whole band (and a pixel) of sky on either side
    h = hits('far-disc-cut')
    assert h[:, 0].any() and not (h[0].any() or h[-1].any() or h[:, -1].any())
    h = hits('far-gate-refuses')
    assert h.any() and not (h[0].any() or h[-1].any() or h[:, 0].any() or h[:, -1].any())
    assert [c['claims']['gate'] for c in K.family('far')] == [True, True, False]
    for c in K.family('far'):
        assert 41999.0 < np.sqrt(c['cam'] @ c['cam']) - 6378.0 < 42030.0


def test_low_and_inside_families():
    c = K.by_name('low-horizon')
    r = K.reference('low-horizon')
    g = R._rot(R._LD, c['m_geo'], [np.longdouble(v) for v in c['cam']])
    # height of the camera above the shell along the ray to the Earth's centre, km
    s = 1 / np.sqrt(float((g[0] / c['a']) ** 2 + (g[1] / c['a']) ** 2 + (g[2] / c['b']) ** 2))
    assert 2.0 < (1 - s) * np.sqrt(c['cam'] @ c['cam']) < 3.0
    h = hits('low-horizon')
    assert h.any() and not h.all() and h[-1].all() and not h[0].any()
    assert float(np.nanmin(f64(r['elev']))) < 1.0               # grazing views of the shell
    assert not hits('low-sky').any() and hits('low-ground').all()
    c, r = K.by_name('inside'), K.reference('inside')
    assert (c['cam'][0] / c['a']) ** 2 + (c['cam'][1] / c['a']) ** 2 + (c['cam'][2] / c['b']) ** 2 < 1
    assert not any(np.isnan(r[k]).any() for k in Q.ARRAYS)
    assert float(r['elev'].max()) < 0                            # seen from below: the far root


def missing_corner_counts(name):
    """(pixels whose centre hits, per pixel the number of its corners that miss)"""
    r = K.reference(name)
    miss = np.isnan(r['lat']).astype(int)
    n = miss[:-1, :-1] + miss[:-1, 1:] + miss[1:, 1:] + miss[1:, :-1]
    return ~np.isnan(r['lat_c']), n


def test_exact_family():
    lo, hi = 90.0, 0.0
    for c in K.family('exact'):
        centre_hit, n = missing_corner_counts(c['name'])
        got = set(n[centre_hit].tolist())
        want = set(c['claims'].get('missing_corners', ()))
        assert want <= got, (c['name'], got)
        if 1 in want:
            # the limb crosses pixels diagonally: pixels with a hit centre and a missing corner lie beside pixels with all four
            partial, full = centre_hit & (n > 0), centre_hit & (n == 0)
            beside = np.zeros_like(full)
            beside[:, 1:] |= full[:, :-1]
            beside[:, :-1] |= full[:, 1:]
            beside[1:] |= full[:-1]
            beside[:-1] |= full[1:]
            assert (partial & (n == 1)).sum() >= 10 and (partial & beside).sum() >= 10
            assert 2 not in want or (partial & (n == 2)).sum() >= 3
            # ... and a centre may miss while a corner of its pixel hits
            assert (~centre_hit & (n < 4)).any()
        el = f64(K.reference(c['name'])['elev'])
        if np.isfinite(el).any():
            lo, hi = min(lo, float(np.nanmin(el))), max(hi, float(np.nanmax(el)))
    assert lo < 0.5 and hi > 89.9, (lo, hi)
    assert float(np.nanmax(f64(K.reference('exact-nadir')['elev']))) > 89.9
    assert {'exact-limb-below+0.5', 'exact-limb-above-1', 'exact-cd-sheared', 'exact-cd-63x16'} <= set(K.names())


def test_pole_and_dateline():
    r = K.reference('pole')
    lon = f64(r['lon'])
    winds = R.quad_winds_pole(lon[:-1, :-1], lon[:-1, 1:], lon[1:, 1:], lon[1:, :-1])
    assert winds.sum() == 1 and float(r['lat'].max()) < 90
    i, j = np.argwhere(winds)[0]
    assert 0 < i < 29 and 0 < j < 39                            # inside the frame, away from its border
    lon = f64(K.reference('dateline')['lon'])
    assert (lon > 179.9).any() and (lon < -179.9).any() and np.abs(lon).min() > 179.0


@pytest.mark.parametrize('case', [c for c in K.cases() if c['time'] is not None], ids=lambda c: c['name'])
def test_header_form_gives_the_same_numbers(case):
    """the WCS cards, camera and time of a case give the library the case's own amt_frame_params, to the bit"""
    from auromat_amd.mapping.astrometry import frame_params
    p = frame_params(case['header'], case['altitude'], case['cam'], case['time'], bool(case['fast_center']))
    q = K.native_params(case)
    for k in ('width', 'height', 'fast_center', 'a', 'b', 'a0', 'b0'):
        assert getattr(p, k) == getattr(q, k), k
    for k in ('cd', 'crpix', 'rot', 'cam', 'm_geo', 'm_sm'):
        assert list(getattr(p, k)) == list(getattr(q, k)), k


# ---- the condition on every case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.cases(), ids=lambda c: c['name'])
def test_no_ray_grazes_and_the_float64_oracle_agrees(case):
    r, f = K.reference(case['name']), K.float64_oracle(case['name'])
    h, w = case['height'], case['width']
    for k in Q.ARRAYS:
        assert r[k].shape == f[k].shape == ((h + 1, w + 1) if k in Q.CORNER_ARRAYS else (h, w))
        assert np.array_equal(np.isnan(r[k]), np.isnan(f[k])), k
    raw = K.reference_longdouble(case['name'])
    rel = [f64(raw['rel']).ravel()] + ([] if case['fast_center'] else [f64(raw['rel_c']).ravel()])
    rel = np.concatenate(rel)
    assert not np.isnan(rel).any() and np.abs(rel).min() >= K.r_min(), (np.abs(rel).min(), K.r_min())
    # hit or miss is the sign of rel for a ray that points at the Earth; NaN patterns of the substituted and the raw run agree
    for k in Q.ARRAYS:
        assert np.array_equal(np.isnan(r[k]), np.isnan(raw[k])), k
    # no elevation so close to a threshold of the box tests that the kernel could legitimately decide otherwise
    for thr in (10.0,):
        for k in ('elev', 'elev_corner'):
            v = f64(r[k])
            assert not (np.abs(v[~np.isnan(v)] - thr) < 1e-8).any(), (k, thr)


def test_r_min_is_the_margin_of_the_rowfield_limb_family():
    import _rowfield_cases as F
    rel = np.abs(f64(F.reference('limb')['rel']))
    assert K.r_min() == float(rel.min()) and 1e-8 < K.r_min() < 1e-7


# ---- longdouble against mpmath -----------------------------------------------------------------------------------------------------
LD_EPS = float(np.finfo(np.longdouble).eps)
WEIGHT = dict(lon='lat', lon_c='lat_c', mlt='mlat', mlt_c='mlat_c')


def tolerance(k, rel, elev, lever=1.0):
    """What the longdouble run owes the mpmath run at one point, degrees (the rule of tests/test_rowfield_cases_cpu.py): 1e-15;
    times sqrt(GRAZING / |rel|) where the ray — for a fast centre the nearest of its four corner rays — all but grazes the shell
    (the root of a discriminant that has lost 1 / rel of its digits), and there times `lever` = |camera| / a when that is above
    1: in the shell's units the root is sqrt(rel) d_o with d_o ~ |camera| / a, and the rounding of d_o^2 - o_o d_d, eps d_o^2,
    moves it by eps d_o / (2 sqrt(rel)) (7.5 times more from 42 000 km than from the 400 km the rule was written at); for an
    elevation beyond STEEP at least 8 eps (180 / pi)^2 / (90 - |elev|) (the arc cosine next to 1)."""
    tol = 1e-15
    if rel < Q.GRAZING:
        tol *= float(np.sqrt(Q.GRAZING / rel)) * max(1.0, lever)
    if k == 'elev':
        off = 90.0 - abs(float(elev))
        if 0 < off < 90.0 - Q.STEEP:
            tol = max(tol, 8 * LD_EPS * (180 / np.pi) ** 2 / off)
    return tol


def check_point(case, raw, kind, i, j, values, worst):
    """the longdouble values of corner / pixel (i, j) against the mpmath values `values`"""
    arrays = Q.CORNER_ARRAYS if kind == 'corner' else Q.CENTRE_ARRAYS
    rel = np.abs(f64(raw['rel']))
    if kind == 'corner':
        r = rel[i, j]
    elif case['fast_center']:
        r = np.min(rel[i:i + 2, j:j + 2])
    else:
        r = abs(float(raw['rel_c'][i, j]))
    for k in arrays:
        d = R.mp_distance(raw[k][i, j], values[k])
        if k in WEIGHT and np.isfinite(d) and not np.isnan(raw[k][i, j]):
            period = 360.0 if k.startswith('lon') else 24.0
            d = min(d, abs(period - d))
            d *= float(np.cos(np.deg2rad(f64(raw[WEIGHT[k]][i, j])))) * (1.0 if k.startswith('lon') else 15.0)
        tol = tolerance(k, r, raw['elev'][i, j] if k == 'elev' else 0.0, float(np.sqrt(case['cam'] @ case['cam'])) / case['a'])
        assert d <= tol, (case['name'], kind, k, i, j, d, tol)
        worst[k] = max(worst.get(k, 0.0), d / tol)


@pytest.mark.parametrize('fam', K.FAMILIES)
def test_longdouble_reference_equals_mpmath(fam):
    """longdouble THROUGHOUT against mpmath: a sample of corners and pixels of every case, and every point at which
    reference() hands out the mpmath value (those values are kept by reference(): nothing is computed twice)"""
    assert LD_EPS < 2e-19, 'np.longdouble is not the 80-bit type here'
    rng = np.random.RandomState(11)
    worst, n_sample, n_taken = {}, 0, 0
    for c in K.family(fam):
        raw, r = K.reference_longdouble(c['name']), K.reference(c['name'])
        h, w = c['height'], c['width']
        for _ in range(max(4, 80 // len(K.family(fam)))):
            i, j = int(rng.randint(0, h + 1)), int(rng.randint(0, w + 1))
            check_point(c, raw, 'corner', i, j, Q.corner_mp(c, i, j), worst)
            i, j = int(rng.randint(0, h)), int(rng.randint(0, w))
            check_point(c, raw, 'centre', i, j, Q.centre_mp(c, i, j), worst)
            n_sample += 2
        for (i, j), v in r['mp_corners'].items():
            check_point(c, raw, 'corner', i, j, v, worst)
            assert all(R.mp_distance(r[k][i, j], v[k]) <= 1e-17 for k in Q.CORNER_ARRAYS)
        for (i, j), v in r['mp_centres'].items():
            check_point(c, raw, 'centre', i, j, v, worst)
            assert all(R.mp_distance(r[k][i, j], v[k]) <= 1e-17 for k in Q.CENTRE_ARRAYS)
        n_taken += len(r['mp_corners']) + len(r['mp_centres'])
    print(fam, n_sample, 'sampled points,', n_taken, 'taken from mpmath; largest distance / tolerance:',
          ' '.join('%s %.2f' % kv for kv in sorted(worst.items())))
    assert n_taken > 0 or fam in ('cd', 'inside', 'pole', 'dateline')


def test_bounds_come_from_the_float64_oracle():
    for fam in K.FAMILIES:
        b = K.bounds(fam)
        print(fam, ' '.join('%s E_ref %.1e bound %.1e' % (k, K.e_ref(fam, k), b[k]) for k in Q.ARRAYS))
        for k in Q.ARRAYS:
            assert b[k] == max(8 * max(K.e_ref(fam, k), R.EPS * R.SCALE[k]), 1e-10)
            assert b[k] < 1e-9


# ---- the host functions ---------------------------------------------------------------------------------------------------------
def sky_rows(case, fast_center=None):
    from auromat_amd import _native
    p = K.native_params(case, fast_center)
    out = [C.c_int32(0) for _ in range(4)]
    assert _native.lib().amt_georef_sky_rows(C.byref(p), *[C.byref(o) for o in out]) == 0
    return [o.value for o in out]


def image_rows(case, min_elev, fast_center):
    from auromat_amd import _native
    p = K.native_params(case, fast_center)
    r0, r1 = C.c_int32(-1), C.c_int32(-1)
    assert _native.lib().amt_georef_image_rows(C.byref(p), float(min_elev), C.byref(r0), C.byref(r1)) == 0
    return r0.value, r1.value


def elevation_gate_passes(case, min_elev):
    """the apparent-size gate of elevation_bands: the cone of elevations >= min_elev about the nadir, asin(max(a, b) / |camera|
    cos(min_elev)), against the same 8 * 18 pixel angles"""
    k = max(case['a'], case['b']) / np.sqrt(case['cam'] @ case['cam']) * np.cos(np.deg2rad(min_elev))
    cd = np.asarray(case['cd']).reshape(2, 2)
    pixel = np.deg2rad(np.sqrt(max(cd[0, 0] ** 2 + cd[1, 0] ** 2, cd[0, 1] ** 2 + cd[1, 1] ** 2)))
    return k < 1 and np.arcsin(k) > K.GATE * pixel


_OTHER = {}


def centres_of(case, fast_center):
    """(centre hits, elevation) of a case in the given centre mode: its reference, or for the other mode the longdouble run"""
    if bool(fast_center) == bool(case['fast_center']):
        r = K.reference(case['name'])
    else:
        if case['name'] not in _OTHER:
            _OTHER[case['name']] = Q.reference(dict(case, fast_center=int(fast_center)), substitute=False)
        r = _OTHER[case['name']]
    return ~np.isnan(r['lat_c']), f64(r['elev'])


@pytest.mark.parametrize('case', K.cases(), ids=lambda c: c['name'])
def test_sky_rows_are_sound_and_tight(case):
    rows, n, top, bottom = sky_rows(case)
    h = case['height']
    assert rows == BAND and n == (h + BAND - 1) // BAND and 0 <= top <= bottom <= n
    corner_hit = hits(case['name']).any(axis=1)                  # (h + 1,)
    centre_hit = np.zeros(h, bool)
    for fast in (1, 0):                                          # the bands do not depend on the centre mode: sound for both
        centre_hit |= centres_of(case, fast)[0].any(axis=1)
        assert sky_rows(case, fast) == [rows, n, top, bottom]
    for c in list(range(top)) + list(range(bottom, n)):
        assert not corner_hit[c * rows:min((c + 1) * rows, h) + 1].any(), (case['name'], c, 'a corner hits in a sky band')
        assert not centre_hit[c * rows:min((c + 1) * rows, h)].any(), (case['name'], c, 'a centre hits in a sky band')
    print(case['name'], 'bands', n, 'sky', (top, bottom), 'corner rows with hits',
          tuple(np.flatnonzero(corner_hit)[[0, -1]]) if corner_hit.any() else None)
    inside = (case['cam'][0] / case['a']) ** 2 + (case['cam'][1] / case['a']) ** 2 + (case['cam'][2] / case['b']) ** 2 < 1
    if inside or not case['claims'].get('gate', True):
        assert (top, bottom) == (0, n)
        return
    if not corner_hit.any() and not centre_hit.any():
        assert top == n
        return
    if not K.gate_passes(case):
        assert (top, bottom) == (0, n)
        return
    first, last = np.flatnonzero(corner_hit)[[0, -1]] if corner_hit.any() else np.flatnonzero(centre_hit)[[0, -1]]
    assert top >= first // rows - 1 and bottom <= last // rows + 2, (case['name'], top, bottom, first, last)
    if case['claims'].get('bands'):
        assert (top, n - bottom) == case['claims']['bands']


def test_list_of_cases_with_sky_bands():
    got = [c['name'] for c in K.cases() if sky_rows(c)[2] > 0 or sky_rows(c)[3] < sky_rows(c)[1]]
    assert sorted(got) == sorted(K.SKY_BAND_NAMES)


@pytest.mark.parametrize('case', K.cases(), ids=lambda c: c['name'])
def test_image_rows_are_sound_and_tight(case):
    h = case['height']
    rows, n, top, bottom = sky_rows(case)
    for fast in (1, 0):
        centre_hit, elev = centres_of(case, fast)
        for min_elev in (-np.inf, 0.0, 10.0, 60.0):
            r0, r1 = image_rows(case, min_elev, fast)
            assert 0 <= r0 <= r1 <= h
            with np.errstate(invalid='ignore'):
                need = (centre_hit & (elev >= min_elev)).any(axis=1)
            assert not need[:r0].any() and not need[r1:].any(), (case['name'], fast, min_elev, r0, r1, np.flatnonzero(need)[[0, -1]])
            if not min_elev > 0:
                assert (r0, r1) == ((top * rows, min(h, bottom * rows)) if top < bottom else (0, 0))
            if not need.any() or not K.gate_passes(case) or (min_elev > 0 and not elevation_gate_passes(case, min_elev)):
                continue                                         # (no bands by design: everything is uploaded, soundly)
            first, last = np.flatnonzero(need)[[0, -1]]
            assert r0 >= (first // BAND - 3) * BAND and r1 <= (last // BAND + 4) * BAND, (case['name'], fast, min_elev, r0, r1, first, last)
