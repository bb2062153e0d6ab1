"""
No GPU: the constructed direction fields of tests/_rowfield_cases.py hold what they claim, and the references of
tests/_rowfield_oracle.py that tests/test_gpu_rowfield.py compares the row kernel with are right — the longdouble run of the
chain equals the mpmath run (50 digits) to 1e-15 deg, the float64 pieces of oracle/ref_numpy.py give the same NaN pattern, and
no ray of any field is closer to grazing the shell than a relative discriminant of 1e-9 (a condition on the inputs: hit or miss
is then beyond doubt in float64, and no corner has to be left out of any comparison).
"""
import numpy as np
import pytest

import _rowfield_cases as K
import _rowfield_oracle as R


def f64(a):
    return np.asarray(a, dtype=np.float64)


def wrapped(d):
    return d - 360.0 * np.rint(d / 360.0)


def test_ownership_sizes_surround_one_strip_and_one_chunk():
    assert [(c['width'], c['height']) for c in K.family('ownership')] == list(K.OWNERSHIP_SIZES)
    for c in K.family('ownership'):
        r = K.reference(c['name'])
        assert not np.isnan(r['lat']).any() and not np.isnan(r['elev']).any()
        if c['height'] > 1:
            step = np.abs(np.diff(f64(r['lat']), axis=0))
            assert 0.04 < step.min() and step.max() < 0.06


@pytest.mark.parametrize('name,array,axis,steps', [
    ('step-lat-rows', 'lat', 0, K.STEPS), ('step-lon-rows', 'lon', 0, K.STEPS),
    ('step-lat-columns', 'lat', 1, K.STEPS_COLUMNS), ('step-lon-columns', 'lon', 1, K.STEPS_COLUMNS)])
def test_steps_lie_on_both_sides_of_the_small_angle_limit(name, array, axis, steps):
    r = K.reference(name)
    got = np.abs(np.diff(f64(r[array]), axis=axis))
    for s in steps:                                           # every step of the set is there, to 0.002 deg
        assert (np.abs(got - s) < 2e-3).any(), (name, s)
    assert ((got > 1.69) & (got < K.LIMIT_DEG)).any() and ((got > K.LIMIT_DEG) & (got < 1.74)).any()
    other = np.abs(np.diff(f64(r['lon' if array == 'lat' else 'lat']), axis=axis))
    assert other.max() < 0.5                                  # ... in that coordinate alone
    if axis == 1:
        # a centre is taken relative to its lane's corner of the current row (the pixel's lower left one)
        off = np.abs(f64(r[array + '_c']) - f64(r[array])[1:, :-1])
        assert ((off > 1.69) & (off < K.LIMIT_DEG)).any() and ((off > K.LIMIT_DEG) & (off < 1.74)).any()


@pytest.mark.parametrize('name', ['dateline-east-rows', 'dateline-west-rows', 'dateline-east-columns',
                                  'dateline-west-columns'])
def test_date_line_marches_start_on_both_sides_of_178(name):
    r = K.reference(name)
    lon = f64(r['lon']) if name.endswith('rows') else f64(r['lon']).T
    sign = 1.0 if 'east' in name else -1.0
    step = wrapped(np.diff(lon, axis=0))
    assert np.all(np.abs(step - sign * 1.6) < 0.01)
    before = sign * lon[:-1]                                   # the corner a step starts from
    assert ((before > 177.89) & (before < 178.0)).sum() >= 3 and ((before > 178.0) & (before < 178.11)).sum() >= 3
    assert ((before > 178.0) & (sign * lon[1:] < -178.0)).any()        # a step over the line from beyond the guard
    assert (lon > 0).any() and (lon < 0).any()
    sm_lon = (f64(r['mlt']) - 12.0) * 15.0                     # m_sm = m_geo: the SM longitude is the longitude
    assert np.max(np.abs(wrapped(sm_lon - f64(r['lon'])))) < 1e-9


@pytest.mark.parametrize('name,negative', [('dateline-zero-plus', False), ('dateline-zero-minus', True)])
def test_date_line_corner_with_a_signed_zero(name, negative):
    c = K.by_name(name)
    assert np.array_equal(c['m_geo'], np.eye(3))
    assert c['cam'][1] == 0 and c['dirs'][1, 2, 1] == 0
    assert bool(np.signbit(c['cam'][1])) == negative and bool(np.signbit(c['dirs'][1, 2, 1])) == negative
    assert c['dirs'][1, 2, 0] > 0 and c['cam'][0] < 0         # the hit has x < 0
    r = K.reference(name)
    assert abs(float(r['lon'][1, 2])) == 180.0
    others = np.ones((4, 4), bool)
    others[1, 2] = False
    assert np.all(np.abs(f64(r['lon'])[others]) < 180.0)
    assert (f64(r['lon']) > 0).any() and (f64(r['lon']) < 0).any()


@pytest.mark.parametrize('case', K.family('pole'), ids=lambda c: c['name'])
def test_pole_lies_inside_one_pixel(case):
    r = K.reference(case['name'])
    dist = case['pole_distance']
    colat = 90.0 - case['pole'] * r['lat']
    assert 0.5 * dist < float(colat.min()) < 2.0 * dist       # (the shell's axis is J2000's: a target is hit within ~ 0.1 m)
    assert float(colat.min()) > 0
    lon = f64(r['lon'])
    winds = R.quad_winds_pole(lon[:-1, :-1], lon[:-1, 1:], lon[1:, 1:], lon[1:, :-1])
    assert winds.sum() == 1 and winds[3, 3]
    assert R.reference_box(r, None)[4] is True


def test_limb_field_misses_where_it_says():
    c, r = K.by_name('limb'), K.reference('limb')
    eps, away = K.limb_offsets()
    miss = np.isnan(r['lat'])
    assert np.array_equal(miss, (eps > 0) | away)
    rel = f64(r['rel'])
    for e in K.LIMB_OFFSETS:                                   # d(rel) / d(angle) = 0.555 at this camera
        for s in (1, -1):
            m = (eps == s * e) & ~away
            assert m.any() and np.all(np.sign(rel[m]) == -s) and np.all(np.abs(np.abs(rel[m]) / (0.555 * e) - 1) < 0.05)
    assert np.all(rel[away] > 0)                               # the line meets the shell, behind the camera
    rows = miss[:, :9].all(axis=1)
    assert list(np.nonzero(rows)[0]) == [4, 5, 9]              # whole miss rows between hit rows of the chunk of rows 0 .. 16
    assert not miss[[3, 6, 8, 10], :9].all(axis=1).any()
    for i, j in ((2, 3), (7, 5), (11, 1), (12, 6), (14, 4), (16, 7)):
        assert miss[i, j] and not miss[i, j - 1] and not miss[i, j + 1]
    assert miss[:7, 9].all() and not miss[7, 9] and miss[:13, 10].all() and not miss[13, 10]
    assert (~np.isnan(r['elev'])).sum() >= 20                  # some pixels have all four corners
    assert c['height'] == 17


def test_inside_camera_hits_with_every_ray():
    c, r = K.by_name('inside'), K.reference('inside')
    assert (c['cam'][0] / c['a']) ** 2 + (c['cam'][1] / c['a']) ** 2 + (c['cam'][2] / c['b']) ** 2 < 1
    assert not any(np.isnan(r[k]).any() for k in R.ARRAYS)
    assert float(r['elev'].max()) < 0                          # seen from below


def test_elevations_spread_with_clusters_at_45_and_at_the_nadir():
    el = f64(K.reference('elevation')['elev'])
    assert not np.isnan(el).any()
    for lo in range(0, 90, 10):
        assert ((el >= lo) & (el < lo + 10)).any(), lo
    assert (el < 1).any()
    assert ((el > 44.9) & (el < 45.0)).sum() >= 4 and ((el > 45.0) & (el < 45.1)).sum() >= 4
    assert (np.abs(el - 45.0) < 0.005).any()
    assert (el == 90.0).sum() >= 8                             # directions longer than 1: the cosine is clamped to 1
    assert ((el > 85) & (el < 89.9)).any() and ((el > 89.9) & (el < 89.99)).any() and ((el > 89.99) & (el < 90)).any()
    d = K.by_name('elevation')['dirs']
    assert np.all((d[-3:] ** 2).sum(axis=-1) > 1.0)


def test_scaled_and_broken_fields():
    half, three, broken = (K.reference(n) for n in ('scaled-0.5', 'scaled-3', 'broken'))
    assert np.max(np.abs(f64(half['lat'] - three['lat']))) < 1e-12          # the hit does not depend on the length
    assert np.all(f64(three['elev']) == 90.0) and np.all(f64(half['elev']) < 30.0)
    corners = np.zeros(broken['lat'].shape, bool)
    pixels = np.zeros(broken['elev'].shape, bool)
    for i, j in K.BROKEN_CORNERS:
        corners[i, j] = True
        pixels[max(i - 1, 0):i + 1, max(j - 1, 0):j + 1] = True
    assert np.isnan(K.by_name('broken')['dirs']).all(axis=-1).sum() == len(K.BROKEN_CORNERS)
    for k in R.ARRAYS:
        assert np.array_equal(np.isnan(broken[k]), corners if k in R.CORNER_ARRAYS else pixels), k
    assert pixels.sum() == 1 + 4 + 1 + 4


# ---- the references ---------------------------------------------------------------------------------------------------------
def _sample(fam, n=110):
    pts = [(c['name'], i, j) for c in K.family(fam) for i in range(c['height'] + 1) for j in range(c['width'] + 1)]
    if len(pts) <= n:
        return pts
    rng = np.random.RandomState(7)
    keep = set(rng.choice(len(pts), size=n, replace=False).tolist()) | {0, len(pts) - 1}
    return [pts[k] for k in sorted(keep)]


LD_EPS = float(np.finfo(np.longdouble).eps)


def longdouble_tolerance(k, raw, i, j):
    """What the longdouble run owes the mpmath run at one point, degrees: 1e-15, but for the two places where the chain itself
    is ill-conditioned and reference() therefore takes the mpmath value.  A ray that all but grazes the shell: the root of a
    discriminant that has lost 1 / rel of its digits moves the hit by eps / sqrt(rel), so 1e-15 at |rel| = 1e-3 grows by
    sqrt(1e-3 / |rel|) (135 times at 1e-7 rad from the tangent cone).  An elevation next to the nadir: the arc cosine of a
    cosine that a dozen roundings have moved by up to 8 eps is off by 8 eps / sin(angle from the vertical)."""
    rel = np.abs(f64(raw['rel']))
    if k in R.CORNER_ARRAYS:
        r = rel[i, j]
    else:
        r = np.min(rel[i:i + 2, j:j + 2])                      # (NaN: the value is NaN as well)
    tol = 1e-15
    if r < R.GRAZING:
        tol *= float(np.sqrt(R.GRAZING / r))
    if k == 'elev':
        off = 90.0 - abs(float(raw['elev'][i, j]))
        if 0 < off < 90.0 - R.STEEP:
            tol = max(tol, 8 * LD_EPS * (180 / np.pi) ** 2 / off)
    return tol


@pytest.mark.parametrize('fam', K.FAMILIES)
def test_longdouble_reference_equals_mpmath(fam):
    """longdouble THROUGHOUT (not what reference() substitutes) against mpmath, every sampled point under its own tolerance"""
    assert LD_EPS < 2e-19, 'np.longdouble is not the 80-bit type here'
    pts = _sample(fam)
    assert len(pts) >= 100
    worst, loose, seen = {}, {}, set()
    for name, i, j in pts:
        c, raw, r = K.by_name(name), K.reference_longdouble(name), K.reference(name)
        m = R.reference_mp(c['dirs'], R.params_of(c), i, j)
        for k, v in m.items():
            if k == 'rel':
                continue
            seen.add(k)
            d = R.mp_distance(raw[k][i, j], v)
            if k in ('lon', 'lon_c', 'mlt', 'mlt_c') and np.isfinite(d) and not np.isnan(raw[k][i, j]):
                period = 360.0 if k.startswith('lon') else 24.0
                d = min(d, abs(period - d))                    # a signed zero may come out as +180 here and -180 there
                partner = raw[{'lon': 'lat', 'lon_c': 'lat_c', 'mlt': 'mlat', 'mlt_c': 'mlat_c'}[k]][i, j]
                d *= float(np.cos(np.deg2rad(f64(partner)))) * (1.0 if k.startswith('lon') else 15.0)
            tol = longdouble_tolerance(k, raw, i, j)
            assert d <= tol, (name, k, i, j, d, tol)
            into = worst if tol == 1e-15 else loose
            into[k] = max(into.get(k, (0.0, 0.0)), (d, tol))
            # what reference() hands out is the mpmath value wherever the tolerance above is loosened
            if tol > 1e-15:
                assert R.mp_distance(r[k][i, j], v) <= 1e-17, (name, k, i, j)
    print(fam, len(pts), 'points, at 1e-15:', ' '.join('%s %.1e' % (k, v[0]) for k, v in sorted(worst.items())))
    if loose:
        print(fam, 'ill-conditioned points, distance / tolerance:', ' '.join('%s %.1e / %.1e' % ((k,) + v) for k, v in sorted(loose.items())))
    assert seen == set(R.ARRAYS)
    assert loose or fam not in ('limb', 'elevation')           # those two are made of such points


def test_ring_longitudes_of_the_mask_test_wind_once():
    """the constructed longitudes of tests/test_gpu_mask_cells.py: exactly the pole pixel winds, by rational arithmetic"""
    import test_gpu_mask_cells as M
    for h, w in M.SHAPES[:4]:
        for pi, pj in ((h // 2, w // 2), (0, w - 1)):
            lon = M.ring_longitudes(h, w, pi, pj)
            for r in range(h):
                for q in range(w):
                    assert M.winds_exact(lon[r, q], lon[r, q + 1], lon[r + 1, q + 1], lon[r + 1, q]) == ((r, q) == (pi, pj))
            assert np.array_equal(M.winds_numpy(lon), np.array([[(r, q) == (pi, pj) for q in range(w)] for r in range(h)]))


@pytest.mark.parametrize('case', K.cases(), ids=lambda c: c['name'])
def test_float64_oracle_has_the_reference_nan_pattern_and_no_ray_grazes(case):
    r, f = K.reference(case['name']), K.float64_oracle(case['name'])
    for k in R.ARRAYS:
        assert r[k].shape == f[k].shape == ((case['height'] + 1, case['width'] + 1) if k in R.CORNER_ARRAYS else
                                            (case['height'], case['width']))
        assert np.array_equal(np.isnan(r[k]), np.isnan(f[k])), k
    rel = f64(r['rel'])
    no_ray = np.isnan(case['dirs']).any(axis=-1)
    assert np.array_equal(np.isnan(rel), no_ray)
    assert np.all(np.abs(rel[~no_ray]) >= 1e-9)
    from oracle import ref_numpy as O
    hits = O.ellipsoid_line_intersects(case['a'], case['b'], case['cam'], case['dirs'].reshape(-1, 3))
    assert np.array_equal(hits.reshape(rel.shape), ~np.isnan(r['lat']))


def test_bounds_come_from_the_float64_oracle():
    for fam in K.FAMILIES:
        b = K.bounds(fam)
        print(fam, ' '.join('%s E_ref %.1e bound %.1e' % (k, K.e_ref(fam, k), b[k]) for k in R.ARRAYS))
        for k in R.ARRAYS:
            assert b[k] == max(8 * max(K.e_ref(fam, k), R.EPS * R.SCALE[k]), 1e-10)
            assert b[k] < 1e-9                                 # the float64 oracle itself is nowhere worse than 1.2e-10 deg
