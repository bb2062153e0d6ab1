"""
TEST INFRASTRUCTURE — high-precision reference of the 19 operator kernels of auromat_amd/csrc/amt_coords.hip.

Every operation of oracle/ref_numpy.py (and of coordinates.wcs.zenithal_pix2world) that such a kernel stands for, restated ONCE,
generic over the number type as tests/_rowfield_oracle.py is, whose LongDouble and MultiPrecision classes and whose shell_hit,
geodetic_deg and mlat_mlt are used here: np.longdouble on whole arrays, mpmath (50 digits) on single points.  The inputs are the
float64 numbers the kernel receives, taken as exact — rotation matrices as 9 doubles, axes, heights, the SIP tables.  What is
restated is the reference's OPERATION, not the kernel's arithmetic: one-step Bowring as transform.py defines it (no seeds, no
Newton steps, and not the true geodetic latitude), the TAN direction through its two native angles, Angle.wrap_at as a floor.

All angles come out in DEGREES and MLT in hours, also for the entry points that work in radians (amt_ecef_to_geodetic,
amt_rotate_pole, amt_cartesian_to_spherical): `comparable` converts a kernel's radians the same way, in longdouble, so that every
distance is in degrees or km.  An operation is a function (xp, A) -> dict of outputs, A the arguments of a case with the per-point
ones (POINT_ARGS) as arrays (longdouble run) or as single numbers (mpmath run).

Where a ray all but grazes its body (|relative discriminant| < 1e-3) `reference` takes the mpmath value: longdouble alone does not
reach 1e-15 of the scale there.  tests/test_coord_cases_cpu.py compares the longdouble run with the mpmath one.
"""
import numpy as np

import _rowfield_oracle as R
from _rowfield_oracle import LongDouble, MultiPrecision, geodetic_deg, mlat_mlt, shell_hit

ZENITHAL = ('TAN', 'SIN', 'ARC', 'STG', 'ZEA')

# entry point (without amt_) -> ((output, kind), ...); kinds: lat / mlat / el (plain degrees), lon / az (wrapped at 360, lon
# weighted by cos lat), mlt (wrapped at 24 h, weighted by 15 cos MLat), km, unit (components of unit vectors), hit (bytes)
OUT = dict(
    intersect_ellipsoid=(('xyz', 'km'),),
    intersects_ellipsoid=(('hit', 'hit'),),
    intersect_sphere=(('xyz', 'km'),),
    ecef_to_geodetic=(('lat', 'lat'), ('lon', 'lon')),
    geodetic_to_ecef=(('x', 'km'), ('y', 'km'), ('z', 'km')),
    rotate_to_latlon=(('lat', 'lat'), ('lon', 'lon')),
    rotate_to_mlat_mlt=(('mlat', 'mlat'), ('mlt', 'mlt')),
    rotate_vectors=(('xyz', 'km'),),
    latlon_to_mlat_mlt=(('mlat', 'mlat'), ('mlt', 'mlt')),
    sm_to_latlon=(('lat', 'lat'), ('lon', 'lon')),
    cartesian_to_spherical=(('r', 'km'), ('lat', 'lat'), ('lon', 'lon')),
    spherical_to_cartesian=(('x', 'km'), ('y', 'km'), ('z', 'km')),
    rotate_pole=(('lat', 'lat'), ('lon', 'lon')),
    rotate_pole_deg=(('lat', 'lat'), ('lon', 'lon')),
    directions_tan=(('dirs', 'unit'),),
    directions_tan_points=(('dirs', 'unit'),),
    directions_zenithal=(('dirs', 'unit'),),
    georef_allsky=(('az', 'az'), ('el', 'el'), ('dirs', 'unit'), ('lat', 'lat'), ('lon', 'lon')),
    reproject_altitude=(('lat', 'lat'), ('lon', 'lon')),
)
OPS = tuple(OUT)
# the arguments of an operation that hold one number (or one row of three) per point
POINT_ARGS = dict(
    intersect_ellipsoid=('dirs',), intersects_ellipsoid=('dirs',), intersect_sphere=('dirs',),
    ecef_to_geodetic=('x', 'y', 'z'), geodetic_to_ecef=('lat', 'lon'), rotate_to_latlon=('xyz',), rotate_to_mlat_mlt=('xyz',),
    rotate_vectors=('xyz',), latlon_to_mlat_mlt=('lat', 'lon'), sm_to_latlon=('smlat', 'smlon'),
    cartesian_to_spherical=('x', 'y', 'z'), spherical_to_cartesian=('r', 'lat', 'lon'), rotate_pole=('lat', 'lon'),
    rotate_pole_deg=('lat', 'lon'), directions_tan=('row', 'col'), directions_tan_points=('px', 'py'),
    directions_zenithal=('row', 'col'), georef_allsky=('row', 'col'), reproject_altitude=('lat', 'lon'),
)
# entry points whose angles are radians (inputs and outputs)
RADIANS = ('ecef_to_geodetic', 'rotate_pole', 'cartesian_to_spherical')
# outputs that pass through a hardware seed refined by one Newton step (amt_common.h: ecef_to_geodetic, geodetic_to_ecef,
# rotate_pole_rad and the kernels composed of them)
SEEDED = ('ecef_to_geodetic', 'geodetic_to_ecef', 'rotate_pole', 'rotate_pole_deg', 'rotate_to_latlon', 'latlon_to_mlat_mlt',
          'sm_to_latlon', 'reproject_altitude')
SEED_REL = 4.1e-15          # v_rsq_f64 + one Newton step, as amt_common.h records it from tools/probe_f64_approx.hip


def seeded(op, out):
    return op in SEEDED or (op == 'georef_allsky' and out in ('lat', 'lon'))


class Float64(LongDouble):
    """the same restatement in float64: the float64 oracle of the operations oracle/ref_numpy.py has no function for"""
    name = 'float64'

    def __init__(self):
        self.pi = np.float64(np.pi)
        self.nan = np.float64('nan')

    def num(self, x):
        return np.asarray(x, dtype=np.float64)


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _rot(xp, m, v):
    return R._rot(xp, m, v)


def _vec(xp, a):
    """(..., 3) float64 array or a row of three numbers -> three numbers of xp"""
    a = np.asarray(a, dtype=np.float64)
    return tuple(xp.num(a[..., i]) for i in range(3))


def _rad(xp, v):
    return v * (xp.pi / 180)


def _deg(xp, v):
    return v * (180 / xp.pi)


def _abs(xp, v):
    return xp.where(xp.lt(v, 0 * v), -v, v)


# ---- rays ----------------------------------------------------------------------------------------------------------------------
def ray_terms(xp, d, origin, a, b):
    """intersection.py:63-74: (origin, d_o, d_d, o_o, discriminant, relative discriminant) in the scaled space"""
    o = [xp.num(v) for v in origin]
    rad = (xp.num(a), xp.num(a), xp.num(b))
    ds = tuple(d[i] / rad[i] for i in range(3))
    os_ = tuple(-o[i] / rad[i] for i in range(3))
    d_o, d_d, o_o = _dot(ds, os_), _dot(ds, ds), _dot(os_, os_)
    disc = d_o * d_o - o_o * d_d + d_d
    big = xp.where(xp.lt(d_o * d_o, o_o * d_d), o_o * d_d, d_o * d_o)
    return o, d_o, d_d, o_o, disc, xp.div(disc, big)


def intersect_ellipsoid(xp, A):
    d = _vec(xp, A['dirs'])
    if A['directed']:
        p, rel = shell_hit(xp, d, dict(cam=A['origin'], a=A['a'], b=A['b']))
        o, d_o, d_d, o_o, disc, _ = ray_terms(xp, d, A['origin'], A['a'], A['b'])
        root = xp.sqrt(disc)
        t = xp.div(d_o + root if bool(o_o < 1) else d_o - root, d_d)
        return dict(xyz=p, rel=rel, t=t, d_o=d_o, root=root)
    o, d_o, d_d, o_o, disc, rel = ray_terms(xp, d, A['origin'], A['a'], A['b'])
    root = xp.sqrt(disc)
    t1, t2 = d_o - root, d_o + root
    t = xp.div(xp.where(xp.lt(_abs(xp, t1), _abs(xp, t2)), t1, t2), d_d)            # intersection.py:243-250
    return dict(xyz=tuple(d[i] * t + o[i] for i in range(3)), rel=rel, t=t, d_o=d_o, root=root)


def intersects_ellipsoid(xp, A):
    """intersection.py:165-201"""
    d = _vec(xp, A['dirs'])
    o, d_o, d_d, o_o, disc, rel = ray_terms(xp, d, A['origin'], A['a'], A['b'])
    root = xp.sqrt(disc)
    if A['directed']:
        t = d_o + root if bool(o_o < 1) else d_o - root
    else:
        t = disc
    hit = xp.where(xp.lt(t, 0 * t), False, t == t)
    if not A['directed']:
        t1, t2 = d_o - root, d_o + root
        t = xp.where(xp.lt(_abs(xp, t1), _abs(xp, t2)), t1, t2)
    return dict(hit=hit, rel=rel, t=xp.div(t, d_d), d_o=d_o, root=root)


def intersect_sphere(xp, A):
    """intersection.py:12-48: the formula for unit directions, on whatever directions it is given"""
    d = _vec(xp, A['dirs'])
    o = [xp.num(v) for v in A['origin']]
    r = xp.num(A['radius'])
    dp, oo = _dot(d, o), _dot(o, o)
    disc = dp * dp - oo + r * r
    root = xp.sqrt(disc)
    if A['directed']:
        raw = -dp + root if bool(xp.sqrt(oo) < r) else -dp - root
        t = xp.where(xp.lt(raw, 0 * raw), xp.nan, raw)
    else:
        t1, t2 = -dp - root, -dp + root
        raw = t = xp.where(xp.lt(_abs(xp, t1), _abs(xp, t2)), t1, t2)
    big = xp.where(xp.lt(dp * dp, oo + 0 * dp), oo + 0 * dp, dp * dp)
    return dict(xyz=tuple(o[i] + t * d[i] for i in range(3)), rel=xp.div(disc, big), t=raw, d_o=-dp, root=root)


# ---- geodetic ------------------------------------------------------------------------------------------------------------------
def _geodetic(xp, g, a, b):
    return geodetic_deg(xp, g, dict(a0=a, b0=b))


def _ecef(xp, lat, lon, h, a, b):
    """transform.py:156-178, radians in"""
    a, b, h = xp.num(a), xp.num(b), xp.num(h)
    e2 = (a * a - b * b) / (a * a)
    sl, cl = xp.sin(lat), xp.cos(lat)
    n = a / xp.sqrt(1 - e2 * sl * sl)
    nh = n + h
    return nh * cl * xp.cos(lon), nh * cl * xp.sin(lon), (n * (1 - e2) + h) * sl


def evolute_margin(xp, g, a, b):
    """p - e^2 a cos^3 u of the one-step Bowring, the denominator of its latitude: positive outside the evolute, where the
    reference's arctan(num / den) and the kernel's atan2(num, den) are the same angle"""
    a, b = xp.num(a), xp.num(b)
    x, y, z = g
    e2 = (a * a - b * b) / (a * a)
    dd = (a * a - b * b) / b
    p = xp.sqrt(x * x + y * y)
    r = xp.sqrt(x * x + y * y + z * z)
    tu = xp.div(b * z * (1 + xp.div(dd, r)), a * p)
    cu = xp.div(1 + 0 * tu, xp.sqrt(1 + tu * tu))
    return p - e2 * a * cu * cu * cu


def ecef_to_geodetic(xp, A):
    lat, lon = _geodetic(xp, (xp.num(A['x']), xp.num(A['y']), xp.num(A['z'])), A['a'], A['b'])
    return dict(lat=lat, lon=lon)


def geodetic_to_ecef(xp, A):
    x, y, z = _ecef(xp, xp.num(A['lat']), xp.num(A['lon']), A['h'], A['a'], A['b'])
    return dict(x=x, y=y, z=z)


def rotate_pole(xp, A):
    """transform.py:301-322 with the rotation as its 9 doubles; radians in"""
    g = _ecef(xp, xp.num(A['lat']), xp.num(A['lon']), A['altitude'], A['a'], A['b'])
    lat, lon = _geodetic(xp, _rot(xp, A['rot'], g), A['a'], A['b'])
    return dict(lat=lat, lon=lon)


def rotate_pole_deg(xp, A):
    g = _ecef(xp, _rad(xp, xp.num(A['lat'])), _rad(xp, xp.num(A['lon'])), A['altitude'], A['a'], A['b'])
    lat, lon = _geodetic(xp, _rot(xp, A['rot'], g), A['a'], A['b'])
    return dict(lat=lat, lon=lon)


# ---- rotations and magnetic coordinates ----------------------------------------------------------------------------------------
def rotate_to_latlon(xp, A):
    lat, lon = _geodetic(xp, _rot(xp, A['m'], _vec(xp, A['xyz'])), A['a'], A['b'])
    return dict(lat=lat, lon=lon)


def rotate_to_mlat_mlt(xp, A):
    mlat, mlt = mlat_mlt(xp, _rot(xp, A['m'], _vec(xp, A['xyz'])))
    return dict(mlat=mlat, mlt=mlt)


def rotate_vectors(xp, A):
    return dict(xyz=_rot(xp, A['m'], _vec(xp, A['xyz'])))


def latlon_to_mlat_mlt(xp, A):
    g = _ecef(xp, _rad(xp, xp.num(A['lat'])), _rad(xp, xp.num(A['lon'])), A['h'], A['a'], A['b'])
    mlat, mlt = mlat_mlt(xp, _rot(xp, A['m'], g))
    return dict(mlat=mlat, mlt=mlt)


def sm_to_latlon(xp, A):
    """transform.py:461-485: unit sphere, the matrix is SM -> GEO"""
    la, lo = _rad(xp, xp.num(A['smlat'])), _rad(xp, xp.num(A['smlon']))
    s = (xp.cos(la) * xp.cos(lo), xp.cos(la) * xp.sin(lo), xp.sin(la))
    lat, lon = _geodetic(xp, _rot(xp, A['m'], s), A['a'], A['b'])
    return dict(lat=lat, lon=lon)


def cartesian_to_spherical(xp, A):
    x, y, z = xp.num(A['x']), xp.num(A['y']), xp.num(A['z'])
    s2 = x * x + y * y
    out = dict(lat=_deg(xp, xp.atan2(z, xp.sqrt(s2))), lon=_deg(xp, xp.atan2(y, x)))
    if A['with_r']:
        out['r'] = xp.sqrt(s2 + z * z)
    return out


def spherical_to_cartesian(xp, A):
    lat, lon = xp.num(A['lat']), xp.num(A['lon'])
    r = 1 if A['r'] is None else xp.num(A['r'])
    return dict(x=r * xp.cos(lat) * xp.cos(lon), y=r * xp.cos(lat) * xp.sin(lon), z=r * xp.sin(lat))


# ---- WCS directions ------------------------------------------------------------------------------------------------------------
def _tan_direction(xp, W, x, y):
    """wcs.py:93-142: pixel (0-based) -> native angles -> unit vector -> celestial"""
    cd, crpix = [xp.num(v) for v in W['cd']], [xp.num(v) for v in W['crpix']]
    px, py = x - crpix[0] + 1, y - crpix[1] + 1
    X, Y = cd[0] * px + cd[1] * py, cd[2] * px + cd[3] * py
    r = xp.sqrt(X * X + Y * Y)
    lon = xp.atan2(X, -Y)
    lat = xp.atan2(180 / xp.pi + 0 * r, r)                      # arctan((180 / pi) / r), pi / 2 at the reference pixel
    return _rot(xp, W['rot'], (xp.cos(lat) * xp.cos(lon), xp.cos(lat) * xp.sin(lon), xp.sin(lat)))


def directions_tan(xp, A):
    off = xp.num(-0.5 if A['corner'] else 0.0)
    return dict(dirs=_tan_direction(xp, A, xp.num(A['col']) + off, xp.num(A['row']) + off))


def directions_tan_points(xp, A):
    return dict(dirs=_tan_direction(xp, A, xp.num(A['px']) - A['origin'], xp.num(A['py']) - A['origin']))


def _sip(xp, table, order, u, v):
    f = 0 * u
    up = 1 + 0 * u
    for p in range(order + 1):
        vq = 1 + 0 * u
        for q in range(order + 1 - p):
            c = float(table[p][q])
            if c:
                f = f + xp.num(c) * up * vq
            vq = vq * v
        up = up * u
    return f


def directions_zenithal(xp, A):
    """coordinates.wcs.zenithal_pix2world on the numbers of the amt_zenithal_wcs block `w` (a ctypes structure)"""
    w = A['w']
    off = -0.5 if w.corner else 0.0
    u = xp.num(A['col']) + xp.num(w.start_x + off) - xp.num(w.crpix[0]) + 1
    v = xp.num(A['row']) + xp.num(w.start_y + off) - xp.num(w.crpix[1]) + 1
    if A['sip']:
        u, v = u + _sip(xp, w.sip_a, w.sip_order_a, u, v), v + _sip(xp, w.sip_b, w.sip_order_b, u, v)
    cd = [xp.num(c) for c in w.cd]
    x, y = cd[0] * u + cd[1] * v, cd[2] * u + cd[3] * v
    r = xp.sqrt(x * x + y * y)
    phi = xp.atan2(x, -y)
    k = 180 / xp.pi
    proj = ZENITHAL[w.projection]
    if proj == 'TAN':
        theta = xp.atan2(k + 0 * r, r)
    elif proj == 'SIN':
        theta = xp.acos(r / k)
    elif proj == 'ARC':
        theta = _rad(xp, 90 - r)
    elif proj == 'STG':
        theta = xp.pi / 2 - 2 * xp.atan(r / (2 * k))
    else:
        theta = xp.pi / 2 - 2 * xp.asin(r / (2 * k))
    ct = xp.cos(theta)
    return dict(dirs=_rot(xp, list(w.rot), (ct * xp.cos(phi), ct * xp.sin(phi), xp.sin(theta))))


# ---- cameras -------------------------------------------------------------------------------------------------------------------
def georef_allsky(xp, A):
    """miracle.py:314-347 (az, el), :239-258 (direction), then the shell and Bowring; A: the amt_allsky_params numbers"""
    off = xp.num(0.0 if A['corner'] else A['center_offset'])
    v0, v1 = xp.num(A['row']) + off - xp.num(A['xc']), xp.num(A['col']) + off - xp.num(A['yc'])
    n0, n1 = xp.num(-1.0), xp.num(0.0)                                  # north = (-1, 0): utils.py:48-56 literally, so that
    az = xp.atan2(v0 * n1 - v1 * n0, v0 * n0 + v1 * n1)                 # the zenith pixel keeps the signs of its zeros
    az = _deg(xp, az - xp.num(A['rotation']))
    az = az - xp.floor(az / 360) * 360                                  # Angle.wrap_at(360 deg)
    el = 90 - _deg(xp, xp.sqrt(v0 * v0 + v1 * v1) / xp.num(A['k']))
    e, z = _rad(xp, el), _rad(xp, -(az - 180))
    local = (xp.cos(e) * xp.cos(z), xp.cos(e) * xp.sin(z), xp.sin(e))
    d = _rot(xp, A['to_geo'], local)
    p, rel = shell_hit(xp, d, dict(cam=A['station'], a=A['a'], b=A['b']))
    lat, lon = _geodetic(xp, p, A['a0'], A['b0'])
    return dict(az=az, el=el, dirs=d, lat=lat, lon=lon, rel=rel)


def reproject_altitude(xp, A):
    """themis.py:224-253, with the station's geodetic2EcefZero (transform.py:180-197)"""
    a0, b0 = A['a'], A['b']
    station = _ecef(xp, _rad(xp, xp.num(A['station_lat'])), _rad(xp, xp.num(A['station_lon'])), 0.0, a0, b0)
    g = _ecef(xp, _rad(xp, xp.num(A['lat'])), _rad(xp, xp.num(A['lon'])), A['height_ref'], a0, b0)
    d = tuple(g[i] - station[i] for i in range(3))
    # (shell_hit takes its origin as float64 numbers; the station here is a high-precision point, so the same lines again)
    rad = (xp.num(a0) + xp.num(A['height_new']), xp.num(a0) + xp.num(A['height_new']), xp.num(b0) + xp.num(A['height_new']))
    ds = tuple(d[i] / rad[i] for i in range(3))
    os_ = tuple(-station[i] / rad[i] for i in range(3))
    d_o, d_d, o_o = _dot(ds, os_), _dot(ds, ds), _dot(os_, os_)
    disc = d_o * d_o - o_o * d_d + d_d
    root = xp.sqrt(disc)
    t = d_o + root if bool(o_o < 1) else d_o - root
    t = xp.div(xp.where(xp.lt(t, 0 * t), xp.nan, t), d_d)
    lat, lon = _geodetic(xp, tuple(d[i] * t + station[i] for i in range(3)), a0, b0)
    big = xp.where(xp.lt(d_o * d_o, o_o * d_d), o_o * d_d, d_o * d_o)
    return dict(lat=lat, lon=lon, rel=xp.div(disc, big))


FUNCTIONS = {op: globals()[op] for op in OPS}

_LD, _F64 = LongDouble(), Float64()
GRAZING = R.GRAZING


def _array(v):
    """an output of the longdouble run -> array; a vector (three arrays) -> (n, 3)"""
    if isinstance(v, tuple):
        return np.stack([np.asarray(c) for c in np.broadcast_arrays(*v)], axis=-1)
    return np.array(v)


def run(xp, op, A):
    """the whole case in an array type (LongDouble or Float64) -> dict of arrays: the outputs and the by-products (rel, t ...)"""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        return {k: _array(v) for k, v in FUNCTIONS[op](xp, A).items()}


def n_points(op, A):
    k = next(k for k in POINT_ARGS[op] if A[k] is not None)
    return int(np.asarray(A[k]).reshape(-1, 3).shape[0] if k in ('dirs', 'xyz') else np.asarray(A[k]).size)


def point(op, A, i):
    """the arguments of point i alone"""
    B = dict(A)
    for k in POINT_ARGS[op]:
        if A[k] is not None:
            B[k] = np.asarray(A[k])[i]
    return B


def reference_mp(op, A, i):
    """point i in mpmath -> dict of output -> mpf (vectors: tuples of three)"""
    return FUNCTIONS[op](R._mp(), point(op, A, i))


def reference(op, A, substitute=True):
    """The case in longdouble -> dict of output -> array (NaN = miss; 'hit': bool).  `substitute=False`: longdouble throughout,
    also where a ray all but grazes (what the CPU test compares with mpmath)."""
    out = run(_LD, op, A)
    if substitute and 'rel' in out:
        with np.errstate(invalid='ignore'):
            grazing = np.nonzero(np.abs(out['rel']) < GRAZING)[0]
        for i in grazing:
            m = reference_mp(op, A, int(i))
            for name, kind in OUT[op]:
                if kind == 'hit' or name not in out:
                    continue
                v = m[name]
                out[name][i] = [R._to_longdouble(c) for c in v] if isinstance(v, tuple) else R._to_longdouble(v)
    return out


def mp_distance(value_ld, value_mp):
    """|longdouble - mpmath|, the largest over the components of a vector"""
    if isinstance(value_mp, tuple):
        return max(R.mp_distance(a, b) for a, b in zip(np.asarray(value_ld).ravel(), value_mp))
    return R.mp_distance(value_ld, value_mp)


# ---- the float64 oracle ----------------------------------------------------------------------------------------------------------
def float64_oracle(op, A):
    """The matching functions of oracle/ref_numpy.py on the same inputs -> dict of output -> float64 array, angles in the unit
    of the entry point (radians for RADIANS).  directions_zenithal: coordinates.wcs.zenithal_pix2world; directions_tan_points
    (ref_numpy has the grid form only): this module's restatement run in float64."""
    from oracle import ref_numpy as O
    f = np.float64
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if op == 'intersect_ellipsoid':
            return dict(xyz=O.ellipsoid_line_intersection(A['a'], A['b'], np.array(A['origin'], f), np.array(A['dirs'], f),
                                                          directed=bool(A['directed'])))
        if op == 'intersects_ellipsoid':
            return dict(hit=O.ellipsoid_line_intersects(A['a'], A['b'], np.array(A['origin'], f), np.array(A['dirs'], f),
                                                        directed=bool(A['directed'])))
        if op == 'intersect_sphere':
            return dict(xyz=O.sphere_line_intersection(A['radius'], np.array(A['origin'], f), np.array(A['dirs'], f),
                                                       directed=bool(A['directed'])))
        if op == 'ecef_to_geodetic':
            lat, lon = O.ecef_to_geodetic(A['x'], A['y'], A['z'], A['a'], A['b'])
            return dict(lat=lat, lon=lon)
        if op == 'geodetic_to_ecef':
            x, y, z = O.geodetic_to_ecef(A['lat'], A['lon'], A['h'], A['a'], A['b'])
            return dict(x=x, y=y, z=z)
        if op in ('rotate_pole', 'rotate_pole_deg'):
            lat, lon = (A['lat'], A['lon']) if op == 'rotate_pole' else (np.deg2rad(A['lat']), np.deg2rad(A['lon']))
            x, y, z = O.geodetic_to_ecef(lat, lon, A['altitude'], A['a'], A['b'])
            r = O.rotate_vectors(np.asarray(A['rot'], f).reshape(3, 3), np.asarray([x, y, z]).T)
            lat, lon = O.ecef_to_geodetic(r[:, 0], r[:, 1], r[:, 2], A['a'], A['b'])
            return dict(lat=lat, lon=lon) if op == 'rotate_pole' else dict(lat=np.rad2deg(lat), lon=np.rad2deg(lon))
        if op == 'rotate_to_latlon':
            gx, gy, gz = O.rotate_vectors(np.asarray(A['m'], f).reshape(3, 3), np.array(A['xyz'], f)).T
            lat, lon = O.ecef_to_geodetic(gx, gy, gz, A['a'], A['b'])
            return dict(lat=np.rad2deg(lat), lon=np.rad2deg(lon))
        if op == 'rotate_to_mlat_mlt':
            mlat, mlt = O._to_mlat_mlt(np.asarray(A['m'], f).reshape(3, 3), np.array(A['xyz'], f))
            return dict(mlat=mlat, mlt=mlt)
        if op == 'rotate_vectors':
            return dict(xyz=O.rotate_vectors(np.asarray(A['m'], f).reshape(3, 3), np.array(A['xyz'], f)))
        if op == 'latlon_to_mlat_mlt':
            x, y, z = O.geodetic_to_ecef(np.deg2rad(A['lat']), np.deg2rad(A['lon']), A['h'], A['a'], A['b'])
            mlat, mlt = O.geo_to_mlat_mlt(np.asarray([x, y, z]).T, np.asarray(A['m'], f).reshape(3, 3))
            return dict(mlat=mlat, mlt=mlt)
        if op == 'sm_to_latlon':
            assert (A['a'], A['b']) == (O.WGS84_A, O.WGS84_B)
            lat, lon = O.sm_to_latlon(np.array(A['smlat'], f), np.array(A['smlon'], f), np.asarray(A['m'], f).reshape(3, 3).T)
            return dict(lat=lat, lon=lon)
        if op == 'cartesian_to_spherical':
            r, lat, lon = O.cartesian_to_spherical(np.array(A['x'], f), np.array(A['y'], f), np.array(A['z'], f))
            return dict(r=r, lat=lat, lon=lon) if A['with_r'] else dict(lat=lat, lon=lon)
        if op == 'spherical_to_cartesian':
            x, y, z = O.spherical_to_cartesian(None if A['r'] is None else np.array(A['r'], f), np.array(A['lat'], f),
                                               np.array(A['lon'], f))
            return dict(x=x, y=y, z=z)
        if op == 'directions_tan':
            return dict(dirs=O.pixel_directions(A['header'], corner=bool(A['corner'])).reshape(-1, 3))
        if op == 'directions_tan_points':
            return {k: v for k, v in run(_F64, op, A).items()}
        if op == 'directions_zenithal':
            from auromat_amd.coordinates.wcs import zenithal_pix2world
            w = A['w']
            return dict(dirs=zenithal_pix2world(A['header'], w.width, w.height, A['startX'], A['startY'],
                                                corner=bool(w.corner)).reshape(-1, 3))
        if op == 'georef_allsky':
            cal, center = A['cal'], not A['corner']
            az, el = O.allsky_az_el(A['size'], cal['xc'], cal['yc'], cal['k'], cal['rotation'], center, A['center_offset'])
            dirs = O.allsky_directions(el, az, cal['lat'], cal['lon'])
            hit = O.ellipsoid_line_intersection(A['a'], A['b'], np.array(A['station'], f), dirs.reshape(-1, 3))
            lat, lon = O.ecef_to_geodetic(hit[:, 0], hit[:, 1], hit[:, 2], A['a0'], A['b0'])
            return dict(az=az.ravel(), el=el.ravel(), dirs=dirs.reshape(-1, 3), lat=np.rad2deg(lat), lon=np.rad2deg(lon))
        if op == 'reproject_altitude':
            assert (A['a'], A['b']) == (O.WGS84_A, O.WGS84_B)
            lat, lon = O.themis_reproject((A['station_lat'], A['station_lon']), np.array(A['lat'], f), np.array(A['lon'], f),
                                          A['height_ref'], A['height_new'])
            return dict(lat=lat, lon=lon)
    raise KeyError(op)


# ---- distances and the bound -------------------------------------------------------------------------------------------------------
EPS = R.EPS


def comparable(op, got):
    """float64 outputs of an entry point (or of the float64 oracle) -> longdouble arrays in degrees / hours / km"""
    out = {}
    for name, kind in OUT[op]:
        if name not in got or kind == 'hit':
            continue
        v = np.asarray(got[name], dtype=np.longdouble)
        if op in RADIANS and kind in ('lat', 'lon'):
            v = v * (180 / _LD.pi)
        out[name] = v
    return out


def distance(op, name, got, ref):
    """Per element, where both are numbers (elsewhere 0).  Angles through _rowfield_oracle.distance: |d lat|, |d lon wrapped|
    cos(lat), |d MLT wrapped at 24 h| 15 cos(MLat) (a longitude whose latitude is NaN — a point on the axis — unweighted);
    azimuth wrapped at 360; absolute km; absolute components of unit vectors.  `got`: comparable()."""
    kind = dict(OUT[op])[name]
    if kind in ('lat', 'mlat', 'el'):
        return R.distance('lat', dict(lat=got[name]), dict(lat=ref[name]))
    if kind in ('lon', 'mlt'):
        partner = 'lat' if kind == 'lon' else 'mlat'
        weight = np.where(np.isnan(ref[partner]), 0, ref[partner])
        return R.distance(kind, {kind: got[name]}, {kind: ref[name], partner: weight})
    if kind == 'az':
        return R.distance('lon', dict(lon=got[name]), dict(lon=ref[name], lat=np.zeros_like(ref[name])))
    want = ref[name]
    ok = ~np.isnan(want) & ~np.isnan(got[name])
    return np.where(ok, np.abs(got[name] - want), 0).astype(np.float64)


def scale(op, name, ref_arrays):
    """90 or 180 deg, 1 for unit vectors, the largest |coordinate| of the references (km)"""
    kind = dict(OUT[op])[name]
    if kind in ('lat', 'mlat', 'el'):
        return 90.0
    if kind in ('lon', 'mlt', 'az'):
        return 180.0
    if kind == 'unit':
        return 1.0
    big = [float(np.nanmax(np.abs(a))) for a in ref_arrays if a.size and not np.isnan(a).all()]
    return max(big) if big else 0.0


def bound(op, name, e_ref, scale_):
    """8 max(E_ref, eps scale, S): S = 4.1e-15 scale behind a refined hardware seed, else 0.  No floor."""
    s = SEED_REL * scale_ if seeded(op, name) else 0.0
    return 8.0 * max(float(e_ref), EPS * scale_, s)
