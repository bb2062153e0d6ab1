"""
TEST INFRASTRUCTURE — high-precision reference of what the fused row kernel (k_georef_rows, directions-in form) computes.

The chain of oracle/ref_numpy.py (georef_frame with fast centres) restated ONCE, generic over the number type: it runs in
np.longdouble (80-bit, eps 1.08e-19) on whole direction fields and in mpmath (50 digits) on single corners and centres.  Its
inputs are the float64 numbers the kernel receives — the direction field (h + 1, w + 1, 3) and cam, a, b, a0, b0, m_geo, m_sm
of its FrameParams — taken as exact; directions are used as supplied, never normalised.

Corner:  hit of the directed ray cam + t d with the shell (a, a, b) (ellipsoid_line_intersection: the far root when the camera
is inside the shell, NaN for t < 0 or a negative discriminant; intersected in J2000 and then rotated, as ref_numpy does),
g = m_geo p -> Bowring (ecef_to_geodetic) on (a0, b0), s = m_sm p -> _to_mlat_mlt with sm_lon_to_mlt.
Fast centre:  mean of the four corner hits and of the four directions (calc_centers), coordinates of the mean point,
elevation_deg of the mean direction at the mean point.
Every corner also gets its relative discriminant disc / max(d_o^2, o_o d_d): how far the ray is from grazing the shell.

Where a ray all but grazes the shell (|relative discriminant| < 1e-3), and where an elevation is beyond 89.6 deg (the arc cosine
next to 1), the field's values are those of the mpmath run: longdouble alone does not reach 1e-15 deg there.

tests/test_rowfield_cases_cpu.py checks the longdouble run (substitute=False: longdouble throughout) against the mpmath one,
under a derived tolerance where it is ill-conditioned, and the NaN patterns against ref_numpy.
"""
import mpmath
import numpy as np

ARRAYS = ('lat', 'lon', 'lat_c', 'lon_c', 'elev', 'mlat', 'mlt', 'mlat_c', 'mlt_c')
CORNER_ARRAYS = ('lat', 'lon', 'mlat', 'mlt')


class LongDouble(object):
    """np.longdouble arrays"""
    name = 'longdouble'

    def __init__(self):
        self.pi = np.longdouble(4) * np.arctan(np.longdouble(1))
        self.nan = np.longdouble('nan')

    def num(self, x):
        return np.asarray(x, dtype=np.longdouble)          # float64 -> longdouble is exact

    def sqrt(self, x):
        with np.errstate(invalid='ignore'):
            return np.sqrt(x)                              # NaN below zero

    def atan(self, x):
        return np.arctan(x)

    def atan2(self, y, x):
        return np.arctan2(y, x)

    def acos(self, x):
        return np.arccos(x)

    def asin(self, x):
        return np.arcsin(x)

    def sin(self, x):
        return np.sin(x)

    def cos(self, x):
        return np.cos(x)

    def tan(self, x):
        return np.tan(x)

    def floor(self, x):
        return np.floor(x)

    def where(self, c, a, b):
        return np.where(c, a, b)

    def lt(self, a, b):
        with np.errstate(invalid='ignore'):
            return a < b

    def div(self, a, b):
        with np.errstate(invalid='ignore', divide='ignore'):
            return a / b


class MultiPrecision(object):
    """mpmath scalars at 50 digits"""
    name = 'mpmath'

    def __init__(self, digits=50):
        self.mp = mpmath.mp.clone()
        self.mp.dps = digits
        self.pi = +self.mp.pi
        self.nan = self.mp.nan

    def num(self, x):
        return self.mp.mpf(float(x))                       # exact

    def _bad(self, *v):
        return any(self.mp.isnan(x) for x in v)

    def sqrt(self, x):
        return self.nan if self._bad(x) or x < 0 else self.mp.sqrt(x)

    def atan(self, x):
        return self.nan if self._bad(x) else self.mp.atan(x)

    def atan2(self, y, x):
        return self.nan if self._bad(x, y) else self.mp.atan2(y, x)

    def acos(self, x):
        return self.nan if self._bad(x) else self.mp.acos(x)

    def asin(self, x):
        return self.nan if self._bad(x) else self.mp.asin(x)

    def sin(self, x):
        return self.nan if self._bad(x) else self.mp.sin(x)

    def cos(self, x):
        return self.nan if self._bad(x) else self.mp.cos(x)

    def tan(self, x):
        return self.nan if self._bad(x) else self.mp.tan(x)

    def floor(self, x):
        return self.nan if self._bad(x) else self.mp.floor(x)

    def where(self, c, a, b):
        return a if c else b

    def lt(self, a, b):
        return (not self._bad(a, b)) and a < b

    def div(self, a, b):
        return self.nan if self._bad(a, b) or b == 0 else a / b


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _rot(xp, m, v):
    m = [xp.num(x) for x in np.asarray(m, dtype=np.float64).ravel()]
    return tuple(m[3 * i] * v[0] + m[3 * i + 1] * v[1] + m[3 * i + 2] * v[2] for i in range(3))


def shell_hit(xp, d, P):
    """ellipsoid_line_intersection(a, b, cam, d, directed=True) -> (point, relative discriminant)"""
    cam = [xp.num(x) for x in P['cam']]
    rad = (xp.num(P['a']), xp.num(P['a']), xp.num(P['b']))
    ds = tuple(d[i] / rad[i] for i in range(3))
    os_ = tuple(-cam[i] / rad[i] for i in range(3))
    d_o, d_d, o_o = _dot(ds, os_), _dot(ds, ds), _dot(os_, os_)
    disc = d_o * d_o - o_o * d_d + d_d
    big = xp.where(xp.lt(d_o * d_o, o_o * d_d), o_o * d_d, d_o * d_o)
    rel = xp.div(disc, big)
    root = xp.sqrt(disc)
    inside = bool(o_o < 1)
    t = d_o + root if inside else d_o - root
    t = xp.where(xp.lt(t, 0 * t), xp.nan, t)
    t = xp.div(t, d_d)
    return tuple(d[i] * t + cam[i] for i in range(3)), rel


def geodetic_deg(xp, g, P):
    """ecef_to_geodetic (Bowring 1985, one step) on (a0, b0) -> (lat, lon) in degrees"""
    a, b = xp.num(P['a0']), xp.num(P['b0'])
    x, y, z = g
    e2 = (a * a - b * b) / (a * a)
    dd = (a * a - b * b) / b
    p2 = x * x + y * y
    p = xp.sqrt(p2)
    r = xp.sqrt(p2 + z * z)
    tu = xp.div(b * z * (1 + xp.div(dd, r)), a * p)
    tu2 = tu * tu
    cu = xp.div(1 + 0 * tu2, xp.sqrt(1 + tu2))
    cu3 = cu * cu * cu
    su3 = tu * cu3 * tu2
    tp = xp.div(z + dd * su3, p - e2 * a * cu3)
    k = 180 / xp.pi
    return xp.atan(tp) * k, xp.atan2(y, x) * k


def mlat_mlt(xp, s):
    """_to_mlat_mlt: cartesian_to_spherical in degrees, MLT = SM longitude * 24 / 360 + 12"""
    x, y, z = s
    k = 180 / xp.pi
    return xp.atan2(z, xp.sqrt(x * x + y * y)) * k, xp.atan2(y, x) * k * 24 / 360 + 12


def corner(xp, d, P):
    """d: 3 numbers / arrays (float64 values, exact) -> dict(p, lat, lon, mlat, mlt, rel)"""
    d = tuple(xp.num(v) for v in d)
    p, rel = shell_hit(xp, d, P)
    lat, lon = geodetic_deg(xp, _rot(xp, P['m_geo'], p), P)
    ml, mt = mlat_mlt(xp, _rot(xp, P['m_sm'], p))
    return dict(p=p, d=d, lat=lat, lon=lon, mlat=ml, mlt=mt, rel=rel)


def centre(xp, c00, c01, c11, c10, P):
    """Fast centre of the pixel whose corners are c00 (row, col), c01 (row, col + 1), c11, c10 (calc_centers' order)."""
    pm = tuple((c00['p'][i] + c01['p'][i] + c11['p'][i] + c10['p'][i]) / 4 for i in range(3))
    dm = tuple((c00['d'][i] + c01['d'][i] + c11['d'][i] + c10['d'][i]) / 4 for i in range(3))
    lat, lon = geodetic_deg(xp, _rot(xp, P['m_geo'], pm), P)
    ml, mt = mlat_mlt(xp, _rot(xp, P['m_sm'], pm))
    n = xp.sqrt(_dot(pm, pm))
    dot = -xp.div(_dot(dm, pm), n)
    one = 1 + 0 * dot
    dot = xp.where(xp.lt(one, dot), one, xp.where(xp.lt(dot, -one), -one, dot))
    elev = 90 - xp.acos(dot) * (180 / xp.pi)
    return dict(lat_c=lat, lon_c=lon, mlat_c=ml, mlt_c=mt, elev=elev)


def params_of(case):
    return {k: case[k] for k in ('cam', 'a', 'b', 'a0', 'b0', 'm_geo', 'm_sm')}


_LD = LongDouble()
_MP = []


def reference(dirs, P, substitute=True):
    """The whole field in longdouble -> dict of the nine arrays (longdouble, NaN = miss) plus 'rel' per corner.
    `substitute=False`: longdouble throughout, also where it is ill-conditioned (what the CPU test compares with mpmath)."""
    xp = _LD
    dirs = np.asarray(dirs, dtype=np.float64)
    c = corner(xp, (dirs[..., 0], dirs[..., 1], dirs[..., 2]), P)

    def part(sl):
        return dict(p=tuple(v[sl] for v in c['p']), d=tuple(v[sl] for v in c['d']))
    s00, s01 = (slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None))
    s11, s10 = (slice(1, None), slice(1, None)), (slice(1, None), slice(None, -1))
    m = centre(xp, part(s00), part(s01), part(s11), part(s10), P)
    out = {k: np.array(c[k]) for k in CORNER_ARRAYS}
    out['rel'] = np.array(c['rel'])
    out.update({k: np.array(v) for k, v in m.items()})
    if not substitute:
        return out
    # A ray that all but grazes the shell loses digits in the discriminant (7 of longdouble's 19 at 1e-7 rad from the tangent
    # cone): such corners, and the centres they are part of, are taken from the mpmath run instead
    with np.errstate(invalid='ignore'):
        grazing = np.argwhere(np.abs(out['rel']) < GRAZING)
    # ... and so does the arc cosine of an elevation next to the nadir (the cosine is a rounded number next to 1)
    with np.errstate(invalid='ignore'):
        pixels = set((int(r), int(q)) for r, q in np.argwhere(np.abs(out['elev']) > STEEP))
    for i, j in grazing:
        v = reference_mp(dirs, P, i, j)
        for k in CORNER_ARRAYS:
            out[k][i, j] = _to_longdouble(v[k])
        pixels.update((r, q) for r in (i - 1, i) for q in (j - 1, j) if 0 <= r < dirs.shape[0] - 1 and 0 <= q < dirs.shape[1] - 1)
    for r, q in sorted(pixels):
        v = reference_mp(dirs, P, r, q)
        for k in m:
            out[k][r, q] = _to_longdouble(v[k])
    return out


GRAZING = 1e-3
STEEP = 89.6


def _to_longdouble(v):
    xp = _mp()
    if xp.mp.isnan(v):
        return np.longdouble('nan')
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - xp.mp.mpf(hi)))


def _mp():
    if not _MP:
        _MP.append(MultiPrecision())
    return _MP[0]


def reference_mp(dirs, P, i, j):
    """Corner (i, j) and, when pixel (i, j) exists, its centre, in mpmath -> dict of array name -> mpf"""
    xp = _mp()
    dirs = np.asarray(dirs, dtype=np.float64)
    cs = {}

    def at(r, q):
        if (r, q) not in cs:
            cs[r, q] = corner(xp, tuple(dirs[r, q]), P)
        return cs[r, q]
    c = at(i, j)
    out = {k: c[k] for k in CORNER_ARRAYS}
    out['rel'] = c['rel']
    if i + 1 < dirs.shape[0] and j + 1 < dirs.shape[1]:
        out.update(centre(xp, at(i, j), at(i, j + 1), at(i + 1, j + 1), at(i + 1, j), P))
    return out


def mp_distance(value_ld, value_mp):
    """|longdouble - mpmath| as a float; both NaN -> 0, one NaN -> inf"""
    xp = _mp()
    a_nan, b_nan = bool(np.isnan(value_ld)), bool(xp.mp.isnan(value_mp))
    if a_nan or b_nan:
        return 0.0 if a_nan and b_nan else float('inf')
    m, e = np.frexp(np.longdouble(value_ld))
    hi = np.float64(m)                                              # split the 64-bit mantissa into two doubles: exact
    lo = np.float64(m - np.longdouble(hi))
    exact = (xp.mp.mpf(float(hi)) + xp.mp.mpf(float(lo))) * xp.mp.mpf(2) ** int(e)
    return float(abs(exact - value_mp))


def float64_oracle(dirs, P):
    """The float64 pieces of oracle/ref_numpy.py on the same inputs -> dict of the nine arrays."""
    from oracle import ref_numpy as O
    dirs = np.asarray(dirs, dtype=np.float64)
    shape = dirs.shape[:2]
    cam, m_geo, m_sm = np.asarray(P['cam'], dtype=np.float64), np.asarray(P['m_geo']), np.asarray(P['m_sm'])
    p_c = O.ellipsoid_line_intersection(P['a'], P['b'], cam, dirs.reshape(-1, 3)).reshape(dirs.shape)
    d_m = O.calc_centers(dirs)
    with np.errstate(invalid='ignore'):
        p_m = O.calc_centers(p_c)

    def geo(p):
        with np.errstate(invalid='ignore', divide='ignore'):
            gx, gy, gz = O.rotate_vectors(m_geo, p.reshape(-1, 3)).T
            la, lo = O.ecef_to_geodetic(gx, gy, gz, P['a0'], P['b0'])
        return np.rad2deg(la).reshape(p.shape[:2]), np.rad2deg(lo).reshape(p.shape[:2])

    def mag(p):
        with np.errstate(invalid='ignore'):
            ml, mt = O._to_mlat_mlt(m_sm, p.reshape(-1, 3))
        return ml.reshape(p.shape[:2]), mt.reshape(p.shape[:2])
    out = {}
    out['lat'], out['lon'] = geo(p_c)
    out['lat_c'], out['lon_c'] = geo(p_m)
    out['mlat'], out['mlt'] = mag(p_c)
    out['mlat_c'], out['mlt_c'] = mag(p_m)
    out['elev'] = O.elevation_deg(d_m, p_m)
    assert out['lat'].shape == shape
    return out


# ---- distances and the bound ------------------------------------------------------------------------------------------------
EPS = float(np.finfo(np.float64).eps)
FLOOR_DEG = 1e-10           # the level tests/test_gpu_cameras.py asserts for these arrays
SCALE = dict(lat=90.0, lat_c=90.0, mlat=90.0, mlat_c=90.0, elev=90.0, lon=180.0, lon_c=180.0, mlt=180.0, mlt_c=180.0)
_PARTNER = dict(lon='lat', lon_c='lat_c', mlt='mlat', mlt_c='mlat_c')


def distance(name, got, ref):
    """Per element, degrees, where the reference is a number (elsewhere 0): |d lat|, |d elev|, |d lon wrapped| cos(lat),
    |d MLT wrapped at 24 h| 15 cos(MLat).  `got`: dict of float64 arrays, `ref`: the longdouble dict."""
    want = ref[name]
    ok = ~np.isnan(want) & ~np.isnan(got[name])
    d = np.asarray(got[name], dtype=np.longdouble) - want
    if name in _PARTNER:
        period = np.longdouble(360) if name.startswith('lon') else np.longdouble(24)
        with np.errstate(invalid='ignore'):
            d = d - period * np.rint(d / period)
            d = d * np.cos(ref[_PARTNER[name]] * (_LD.pi / 180))
        if not name.startswith('lon'):
            d = d * 15
    return np.where(ok, np.abs(d), 0).astype(np.float64)


def bound(name, e_ref):
    """8 max(E_ref, eps scale), not below the floor"""
    return max(8.0 * max(float(e_ref), EPS * SCALE[name]), FLOOR_DEG)


def quad_winds_pole(o00, o01, o11, o10):
    """Pixels whose corner longitudes (degrees) wind once around a pole: wrapped steps sum to +-360 (geodesic.py:183)."""
    def step(a, b):
        d = b - a
        return d - 360.0 * np.rint(d / 360.0)
    with np.errstate(invalid='ignore'):
        return np.abs(step(o00, o01) + step(o01, o11) + step(o11, o10) + step(o10, o00)) > 180.0


def reference_box(ref, min_elevation):
    """The bounding-box rule (reference mapping.py:693-743) on the reference arrays, corners kept as sanitize_masks /
    mask_by_elevation keep them -> (latSouth, lonWest, latNorth, lonEast, pole in view, crosses the date line), or None
    when nothing is kept."""
    from oracle import ref_numpy as O
    lat, lon, elev = (np.asarray(ref[k], dtype=np.float64) for k in ('lat', 'lon', 'elev'))
    corner_nan = np.isnan(lat)
    if min_elevation is None:
        corner_mask, centre_mask = O.sanitize_masks(corner_nan, np.isnan(elev))
    else:
        with np.errstate(invalid='ignore'):
            if not (elev >= min_elevation).any():
                return None
        corner_mask, centre_mask = O.mask_by_elevation(elev, corner_nan, min_elevation)
    if corner_mask.all():
        return None
    la, lo = lat[~corner_mask], lon[~corner_mask]
    pole = bool((quad_winds_pole(lon[:-1, :-1], lon[:-1, 1:], lon[1:, 1:], lon[1:, :-1]) & ~centre_mask).any())
    if pole:
        if la.max() < 0:
            return -90.0, -180.0, la.max(), 180.0, True, False
        return la.min(), -180.0, 90.0, 180.0, True, False
    if lo.max() - lo.min() > 180:
        return la.min(), lo[lo > 0].min(), la.max(), lo[~(lo > 0)].max(), False, True
    return la.min(), lo.min(), la.max(), lo.max(), False, False
