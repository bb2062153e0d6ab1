"""
TEST INFRASTRUCTURE — constructed corner-direction fields for the fused row kernel (k_georef_rows, directions-in form).

Every field is built by aiming from a chosen camera at chosen target points on (or, for the limb, beside) the shell and
rounding the directions to float64; what the kernel and the references of tests/_rowfield_oracle.py get are those float64
numbers.  A case is a dict: name, family, dirs (h + 1, w + 1, 3), cam (J2000), a, b, a0, b0, m_geo, m_sm, and what the family
claims (pole: +1 / -1 / 0 in view, dateline: crosses +-180 deg).  tests/test_rowfield_cases_cpu.py checks the claims on the
longdouble reference.

Families (the code they aim at is in auromat_amd/csrc/amt_georef.hip and fx:: of amt_common.h):
  ownership   smooth 0.05 deg / px fields at sizes around one strip (63 corner columns) and one chunk (16 rows)
  step        row-to-row and column-to-column steps in latitude, and separately in longitude, on both sides of the small-angle
              limit tan^2 <= 9e-4 (1.718 deg); a centre is taken relative to its lane's corner, half a column away: 3.40 / 3.46
  dateline    columns that march across +-180 deg eastwards and westwards from within 0.1 deg of +-178 deg (the guard of the
              small-angle sum), the same along rows, and with m_geo = I a corner whose y is exactly +0 / -0 at x < 0
  pole        north / south pole inside a pixel, the nearest corner 1e-6, 1e-3, 0.1 deg away
  limb        rays 1e-3, 1e-5, 1e-7 rad inside and outside the tangent cone: whole miss rows inside a chunk, single missing
              lanes, first hits after misses in a column, rays pointing away from the Earth
  inside      camera below the shell: every ray hits, the far root
  elevation   centre elevations from the limb to 89.999 deg, dense around 45 deg, and nadir rows whose directions are longer than 1
              by 2^-20: the clamp to 1
  scaled      one smooth field times 0.5 and times 3
  broken      the same field with isolated NaN corners
"""
from datetime import datetime

import numpy as np

from oracle import ref_numpy as O

A0, B0 = O.WGS84_A, O.WGS84_B
ET = O.date2es(datetime(2012, 3, 4, 17, 19, 0))
M_GEO = np.ascontiguousarray(O.mat_j2000_to_geo(ET))
M_SM = np.ascontiguousarray(O.mat_j2000_to_sm(ET))
EYE = np.eye(3)

STEPS = (0.2, 1.0, 1.6, 1.70, 1.73, 3.0, 6.0, 20.0)
STEPS_COLUMNS = STEPS + (3.40, 3.46)
LIMIT_DEG = float(np.degrees(np.arctan(np.sqrt(9.0e-4))))          # 1.7184 deg
OWNERSHIP_SIZES = ((1, 1), (3, 1), (62, 15), (63, 16), (64, 17), (127, 33), (2, 40))
POLE_DISTANCES = (1e-6, 1e-3, 0.1)
LIMB_OFFSETS = (1e-3, 1e-5, 1e-7)


def ecef(lat, lon, height):
    """geodetic degrees, km -> (..., 3) GEO"""
    x, y, z = O.geodetic_to_ecef(np.deg2rad(lat), np.deg2rad(lon), height)
    return np.stack(np.broadcast_arrays(x, y, z), axis=-1)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def case(name, family, dirs_geo, cam_geo, m_geo=M_GEO, m_sm=M_SM, altitude=110.0, pole=0, dateline=False, j2000=False):
    """directions and camera given in GEO -> the J2000 numbers the kernel gets (d = m_geo^T d_geo, rounded); `j2000`: they are
    given in J2000 already (the shell's axis is the z axis of J2000, as in the reference: what has to graze the shell is
    built there)"""
    dirs_geo = np.asarray(dirs_geo, dtype=np.float64)
    m_geo = np.ascontiguousarray(m_geo, dtype=np.float64)
    if j2000 or np.array_equal(m_geo, EYE):
        dirs, cam = dirs_geo.copy(), np.array(cam_geo, dtype=np.float64)      # (m_geo = I: keeps signed zeros)
    else:
        dirs = np.ascontiguousarray(dirs_geo @ m_geo)       # rows: m_geo^T d
        cam = np.asarray(cam_geo, dtype=np.float64) @ m_geo
    dirs.setflags(write=False)
    return dict(name=name, family=family, dirs=dirs, cam=cam, a=A0 + altitude, b=B0 + altitude, a0=A0, b0=B0,
                m_geo=m_geo, m_sm=np.ascontiguousarray(m_sm, dtype=np.float64), altitude=altitude, pole=pole,
                dateline=dateline, height=dirs.shape[0] - 1, width=dirs.shape[1] - 1)


def aimed(name, family, lat, lon, cam_geo, **kw):
    """corner (i, j) looks at the point of geodetic (lat, lon)[i, j] at the shell's altitude"""
    altitude = kw.get('altitude', 110.0)
    return case(name, family, unit(ecef(lat, lon, altitude) - cam_geo), cam_geo, **kw)


def smooth(w, h, lat0=50.0, lon0=10.0):
    i, j = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    return lat0 - 0.05 * i + 0.002 * j, lon0 + 0.07 * j + 0.003 * i


def cumulative(steps, n):
    """0 and n partial sums of +s0, -s1, +s2, ... with the signs of every other cycle flipped (the walk stays near 0)"""
    out, k = [0.0], 0
    while len(out) <= n:
        cycle, s = k // len(steps), steps[k % len(steps)]
        sign = (1 if (k % len(steps)) % 2 == 0 else -1) * (1 if cycle % 2 == 0 else -1)
        out.append(out[-1] + sign * s)
        k += 1
    return np.array(out)


def _ownership():
    cam = ecef(49.0, 14.0, 400.0)
    return [aimed('ownership-%dx%d' % (w, h), 'ownership', *smooth(w, h), cam_geo=cam) for w, h in OWNERSHIP_SIZES]


def _step():
    cam = ecef(5.0, 30.0, 36000.0)
    rows, cols = cumulative(STEPS, 17), cumulative(STEPS_COLUMNS, 20)
    small_r, small_c = 0.1 * np.arange(5.0), 0.1 * np.arange(4.0)
    return [
        aimed('step-lat-rows', 'step', 13.0 + rows[:, None] + 0 * small_r, 30.0 + small_r + 0 * rows[:, None], cam),
        aimed('step-lon-rows', 'step', 10.0 + small_r + 0 * rows[:, None], 38.0 + rows[:, None] + 0 * small_r, cam),
        aimed('step-lat-columns', 'step', 13.0 + cols + 0 * small_c[:, None], 30.0 + small_c[:, None] + 0 * cols, cam),
        aimed('step-lon-columns', 'step', 10.0 + small_c[:, None] + 0 * cols, 38.0 + cols + 0 * small_c[:, None], cam),
    ]


def _dateline():
    cam = ecef(20.0, 180.0, 36000.0)
    off = np.array([-0.1, -0.05, -0.01, 0.01, 0.05, 0.1])
    march = 178.0 - 4.8 + 1.6 * np.arange(9.0)                  # 173.2 ... 178.0 (index 3) ... 186.0
    lon = march[:, None] + off
    lat = 20.0 + 0.1 * np.arange(6.0) + 0 * march[:, None]
    kw = dict(m_sm=M_GEO, dateline=True)                        # "SM" longitude = longitude: the twin guard sees the same
    out = [aimed('dateline-east-rows', 'dateline', lat, lon, cam, **kw),
           aimed('dateline-west-rows', 'dateline', lat, -lon, cam, **kw),
           aimed('dateline-east-columns', 'dateline', lat.T, lon.T, cam, **kw),
           aimed('dateline-west-columns', 'dateline', lat.T, -lon.T, cam, **kw)]
    i, j = np.mgrid[0:4, 0:4].astype(np.float64)
    lat, lon = 15.0 + 0.3 * i, 180.0 + 0.3 * (j - 2) + 0.05 * (i - 1)        # corner (1, 2) is on the date line
    for tag, zero in (('plus', 0.0), ('minus', -0.0)):
        cam = np.array([-20000.0, zero, 8000.0])
        d = unit(ecef(lat, lon, 110.0) - cam)
        d[1, 2, 1] = zero                                       # cam.y + t d.y is exactly +0 / -0
        out.append(case('dateline-zero-' + tag, 'dateline', d, cam, m_geo=EYE, m_sm=EYE, dateline=True))
    return out


def _pole():
    out = []
    i, j = np.mgrid[0:9, 0:9].astype(np.float64)
    for sign, tag in ((1, 'north'), (-1, 'south')):
        cam = ecef(sign * 75.0, 40.0, 3000.0)
        for dist in POLE_DISTANCES:
            x, y = (j - 4) * 0.3 + dist / np.sqrt(2.0), (i - 4) * 0.3 + dist / np.sqrt(2.0)
            lat = sign * (90.0 - np.hypot(x, y))
            lon = np.degrees(np.arctan2(y, x)) + 25.0
            out.append(dict(aimed('pole-%s-%g' % (tag, dist), 'pole', lat, lon, cam, pole=sign), pole_distance=dist))
    return out


def limb_offsets():
    """(18, 12) angles from the tangent cone in rad (negative: inside, a hit) and the mask of rays turned away"""
    e = np.empty((18, 12))
    for i in range(18):
        for j in range(12):
            e[i, j] = -LIMB_OFFSETS[(i + j) % 3]
    for i, k in ((4, 0), (5, 1), (9, 2)):                       # whole miss rows inside the first chunk
        e[i, :] = LIMB_OFFSETS[k]
    for n, (i, j) in enumerate(((2, 3), (7, 5), (11, 1), (12, 6), (14, 4), (16, 7))):      # single missing lanes
        e[i, j] = LIMB_OFFSETS[n % 3]
    e[:7, 9] = [LIMB_OFFSETS[i % 3] for i in range(7)]          # first hits after misses in a column
    e[:13, 10] = [LIMB_OFFSETS[(i + 1) % 3] for i in range(13)]
    away = np.zeros(e.shape, bool)
    away[:, 11] = True
    e[:, 11] = -LIMB_OFFSETS[0]
    return e, away


def _limb():
    cam = ecef(45.0, -70.0, 400.0) @ M_GEO                      # J2000
    rad = np.array([A0 + 110.0, A0 + 110.0, B0 + 110.0])
    os_ = cam / rad                                             # the shell is the unit sphere in these coordinates
    dist = np.sqrt(os_ @ os_)
    axis = -os_ / dist
    f = unit(np.cross(axis, [0.0, 0.0, 1.0]))
    g = np.cross(axis, f)
    eps, away = limb_offsets()
    i, j = np.mgrid[0:18, 0:12].astype(np.float64)
    theta = np.arcsin(1.0 / dist) + eps
    phi = 0.4 + 0.01 * j + 0.001 * i
    ds = np.cos(theta)[..., None] * axis + np.sin(theta)[..., None] * (np.cos(phi)[..., None] * f + np.sin(phi)[..., None] * g)
    d = unit(ds * rad)
    d[away] = -d[away]
    return [case('limb', 'limb', d, cam, j2000=True)]


def _inside():
    lat, lon = 65.0, 25.0
    cam = ecef(lat, lon, 0.0)
    la, lo = np.deg2rad(lat), np.deg2rad(lon)
    east = np.array([-np.sin(lo), np.cos(lo), 0.0])
    north = np.array([-np.sin(la) * np.cos(lo), -np.sin(la) * np.sin(lo), np.cos(la)])
    up = np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    y, x = np.meshgrid(np.linspace(3, -3, 17), np.linspace(-3, 3, 17), indexing='ij')
    return [case('inside', 'inside', unit(x[..., None] * east + y[..., None] * north + up), cam)]


ELEVATIONS = (0.3, 1.0, 5.0, 10.0, 20.0, 30.0, 40.0, 44.0, 44.8, 44.98, 44.998, 45.002, 45.02, 45.2, 46.0, 50.0, 60.0, 70.0,
              80.0, 87.0, 89.5, 89.9, 89.99, 89.999)


def _elevation():
    cam = ecef(-30.0, 100.0, 400.0) @ M_GEO                       # J2000
    axis = -unit(cam)                                             # the ray along it has elevation 90 deg exactly
    f = unit(np.cross(axis, [0.0, 0.0, 1.0]))
    g = np.cross(axis, f)

    def elevation_at(theta, phi=0.3002):
        d = np.cos(theta) * axis + np.sin(theta) * (np.cos(phi) * f + np.sin(phi) * g)
        with np.errstate(invalid='ignore'):
            p = O.ellipsoid_line_intersection(A0 + 110.0, B0 + 110.0, cam, d[None, :])
            return float(O.elevation_deg(d[None, None, :], p[None, :, :])[0, 0])

    def angle_for(elevation):                                     # bisection: the elevation falls as the ray leaves the nadir
        lo, hi = 0.0, 1.3
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            e = elevation_at(mid)
            lo, hi = (mid, hi) if e > elevation else (lo, mid)    # (a miss, NaN: too far out)
        return lo
    theta = np.array([angle_for(e) for e in ELEVATIONS])
    theta = np.concatenate((theta, [2e-6, 1e-6, 0.0]))            # three nadir rows
    length = np.concatenate((np.ones(len(ELEVATIONS)), np.full(3, 1.0 + 2.0 ** -20)))
    phi = 0.3 + 1e-4 * np.arange(5.0)
    d = np.cos(theta)[:, None, None] * axis + np.sin(theta)[:, None, None] * (np.cos(phi)[None, :, None] * f +
                                                                             np.sin(phi)[None, :, None] * g)
    return [case('elevation', 'elevation', unit(d) * length[:, None, None], cam, j2000=True)]


BROKEN_CORNERS = ((0, 0), (4, 7), (9, 16), (6, 3))


def _scaled_and_broken():
    cam = ecef(49.0, 14.0, 400.0)
    base = aimed('base', 'scaled', *smooth(16, 9), cam_geo=cam)
    d_geo = np.array(base['dirs']) @ M_GEO.T
    out = [case('scaled-0.5', 'scaled', d_geo * 0.5, cam), case('scaled-3', 'scaled', d_geo * 3.0, cam)]
    hole = d_geo.copy()
    for i, j in BROKEN_CORNERS:
        hole[i, j] = np.nan
    out.append(case('broken', 'broken', hole, cam))
    return out


FAMILIES = ('ownership', 'step', 'dateline', 'pole', 'limb', 'inside', 'elevation', 'scaled', 'broken')
_CASES = []


def cases():
    if not _CASES:
        for make in (_ownership, _step, _dateline, _pole, _limb, _inside, _elevation, _scaled_and_broken):
            _CASES.extend(make())
        assert {c['family'] for c in _CASES} == set(FAMILIES)
    return _CASES


def names():
    return [c['name'] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c['name'] == name)


def family(name):
    return [c for c in cases() if c['family'] == name]


# ---- references, computed once per process ----------------------------------------------------------------------------------
_REF, _F64, _RAW = {}, {}, {}


def reference(name):
    """the longdouble arrays of tests/_rowfield_oracle.reference (read-only)"""
    import _rowfield_oracle as R
    if name not in _REF:
        c = by_name(name)
        r = R.reference(c['dirs'], R.params_of(c))
        for v in r.values():
            v.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def reference_longdouble(name):
    """longdouble throughout: without the mpmath values that reference() takes at ill-conditioned points"""
    import _rowfield_oracle as R
    c = by_name(name)
    if name not in _RAW:
        _RAW[name] = R.reference(c['dirs'], R.params_of(c), substitute=False)
    return _RAW[name]


def float64_oracle(name):
    import _rowfield_oracle as R
    if name not in _F64:
        c = by_name(name)
        _F64[name] = R.float64_oracle(c['dirs'], R.params_of(c))
    return _F64[name]


def e_ref(fam, array):
    """distance of the float64 oracle from the longdouble reference, the largest over the family's cases"""
    import _rowfield_oracle as R
    return max(float(R.distance(array, float64_oracle(c['name']), reference(c['name'])).max()) for c in family(fam))


def bounds(fam):
    import _rowfield_oracle as R
    return {k: R.bound(k, e_ref(fam, k)) for k in R.ARRAYS}
