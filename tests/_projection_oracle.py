"""
TEST INFRASTRUCTURE — the two map projections of auromat_amd/csrc/amt_project.hip (``amt_project_forward`` /
``amt_project_inverse``) stated ONCE, generic over the number type: np.float64 and np.longdouble on whole arrays, mpmath (50
digits) on single points — the number classes of tests/_rowfield_oracle.py and tests/_coord_oracle.py with exp, log and a
finiteness test added.

What is stated is Snyder's text (Map Projections - A Working Manual), not the kernel's arithmetic:
  * the conformal latitude by (3-1), chi = 2 atan[tan(pi/4 + phi/2) ((1 - e sin phi) / (1 + e sin phi))^(e/2)] - pi/2;
  * the oblique stereographic by (21-27), (21-24), (21-25) with k0 = 1, its polar form by (21-33), (21-30), (21-31), (15-9);
  * the inverse by (21-15), (20-14) / (20-15) on the conformal sphere — the point as (sin chi, cos chi cos dlon, cos chi sin dlon),
    so that chi comes from an atan2 and not from an asin — and the latitude by the iteration (3-4); the polar inverse by (21-39),
    (7-9), (20-16) / (20-17);
  * the polar azimuthal equidistant projection of a sphere by (25-1), (25-2) at the poles.
tan(pi/4 + chi/2) is written (1 + sin chi) / cos chi: pi/4 + chi/2 rounds past pi/2 in some number types.

A projection is a dict: ``stere(lat0, lon0, a, b)`` or ``paeqd(north, lon0, radius)``.  Outputs: x, y in the unit of a / radius;
lat, lon in degrees, lon in [-180, 180).  The domain rule and the NaN rule are the header's: forward, a point more than 90 degrees
from the centre (D < 1 on the conformal sphere; the other hemisphere) and any non-finite input give NaN in both outputs.
"""
import math

import numpy as np

import _coord_oracle as CO
import _rowfield_oracle as RO

POLAR_LIMIT = 1e-8          # degrees: a centre closer than this to a pole takes the polar form
WGS84_A, WGS84_B = 6378.137, 6356.752314245179
BASEMAP_RADIUS = 6370.997


class _ArrayExtras(object):
    def exp(self, x):
        return np.exp(x)

    def log(self, x):
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.log(x)

    def finite(self, x):
        return np.isfinite(x)

    def eq(self, a, b):
        return a == b

    def no(self, c):
        return ~np.asarray(c)


class Float64(_ArrayExtras, CO.Float64):
    iterations = 10


class LongDouble(_ArrayExtras, RO.LongDouble):
    iterations = 12


class MultiPrecision(RO.MultiPrecision):
    iterations = 26             # e^2 = 0.0067 per step of (3-4): below 1e-50

    def exp(self, x):
        return self.nan if self._bad(x) else self.mp.exp(x)

    def log(self, x):
        return self.nan if self._bad(x) or x <= 0 else self.mp.log(x)

    def finite(self, x):
        return bool(self.mp.isfinite(x))

    def eq(self, a, b):
        return (not self._bad(a, b)) and a == b

    def no(self, c):
        return not c


def stere(lat0, lon0, a=WGS84_A, b=WGS84_B):
    return dict(kind='stere', lat0=float(lat0), lon0=float(lon0), a=float(a), b=float(b))


def paeqd(north, lon0=180.0, radius=BASEMAP_RADIUS):
    return dict(kind='paeqd', north=bool(north), lat0=90.0 if north else -90.0, lon0=float(lon0), a=float(radius), b=float(radius))


def is_polar(P):
    return P['kind'] == 'paeqd' or 90.0 - abs(P['lat0']) < POLAR_LIMIT


def _rad(xp, v):
    return v * (xp.pi / 180)


def _deg(xp, v):
    return v * (180 / xp.pi)


def _pow_ratio(xp, e, s, power):
    """((1 - e s) / (1 + e s))^power"""
    return xp.exp(power * xp.log(xp.div(1 - e * s, 1 + e * s)))


def eccentricity(xp, P):
    a, b = xp.num(P['a']), xp.num(P['b'])
    return xp.sqrt(1 - (b / a) * (b / a))


def conformal(xp, e, lat):
    """chi (radians) of the geodetic latitude lat (degrees), (3-1); +-pi/2 at the poles themselves"""
    phi = _rad(xp, lat)
    chi = 2 * xp.atan(xp.tan(xp.pi / 4 + phi / 2) * _pow_ratio(xp, e, xp.sin(phi), e / 2)) - xp.pi / 2
    chi = xp.where(xp.eq(lat, xp.num(90.0)), xp.pi / 2 + 0 * lat, chi)
    return xp.where(xp.eq(lat, xp.num(-90.0)), -xp.pi / 2 + 0 * lat, chi)


def polar_constant(xp, P):
    """2 a / sqrt((1 + e)^(1 + e) (1 - e)^(1 - e))  (21-33)"""
    e = eccentricity(xp, P)
    return 2 * xp.num(P['a']) / xp.sqrt(xp.exp((1 + e) * xp.log(1 + e)) * xp.exp((1 - e) * xp.log(1 - e)))


def constants(xp, P):
    """dict(e, mode, sin_chi1, cos_chi1, m1, k) as amt_projection holds them"""
    if P['kind'] == 'paeqd':
        mode = 1 if P['north'] else -1
        return dict(e=xp.num(0.0), mode=mode, sin_chi1=xp.num(float(mode)), cos_chi1=xp.num(0.0), m1=xp.num(0.0), k=xp.num(P['a']))
    e = eccentricity(xp, P)
    if is_polar(P):
        mode = 1 if P['lat0'] > 0 else -1
        return dict(e=e, mode=mode, sin_chi1=xp.num(float(mode)), cos_chi1=xp.num(0.0), m1=xp.num(0.0), k=polar_constant(xp, P))
    phi1 = _rad(xp, xp.num(P['lat0']))
    chi1 = conformal(xp, e, xp.num(P['lat0']))
    s1 = xp.sin(phi1)
    m1 = xp.cos(phi1) / xp.sqrt(1 - e * e * s1 * s1)
    return dict(e=e, mode=0, sin_chi1=xp.sin(chi1), cos_chi1=xp.cos(chi1), m1=m1, k=2 * xp.num(P['a']) * m1 / xp.cos(chi1))


def _wrap(xp, lon):
    w = lon - 360 * xp.floor((lon + 180) / 360)
    # (in float64 lon + 180 may round up to a multiple of 360 from just below it)
    w = xp.where(xp.lt(w, -180 + 0 * w), w + 360, w)
    return xp.where(xp.lt(w, 180 + 0 * w), w, w - 360)


def domain_D(xp, P, lat, lon):
    """D = 1 + cos(angular distance from the centre), on the conformal sphere for the stereographic projection: the forward
    direction is defined where D >= 1."""
    lat, lon = xp.num(lat), xp.num(lon)
    dl = _rad(xp, lon - xp.num(P['lon0']))
    if P['kind'] == 'paeqd':
        return 1 + (1 if P['north'] else -1) * xp.sin(_rad(xp, lat))
    K = constants(xp, P)
    chi = conformal(xp, K['e'], lat)
    return 1 + K['sin_chi1'] * xp.sin(chi) + K['cos_chi1'] * xp.cos(chi) * xp.cos(dl)


def forward(xp, P, lat, lon):
    """(x, y) of (lat, lon) in degrees"""
    lat, lon = xp.num(lat), xp.num(lon)
    ok = xp.finite(lat) & xp.finite(lon)
    dl = _rad(xp, lon - xp.num(P['lon0']))
    K = constants(xp, P)
    if P['kind'] == 'paeqd':
        sgn = K['mode']
        colat = 90 - sgn * lat
        rho = K['k'] * _rad(xp, colat)
        x, y = rho * xp.sin(dl), -sgn * rho * xp.cos(dl)
        inside = xp.no(xp.lt(xp.num(90.0), colat))
    else:
        e = K['e']
        chi = conformal(xp, e, lat)
        if K['mode']:
            sgn = K['mode']
            D = 1 + sgn * xp.sin(chi)
            ph = sgn * _rad(xp, lat)
            t = xp.div(xp.tan(xp.pi / 4 - ph / 2), _pow_ratio(xp, e, xp.sin(ph), e / 2))          # (15-9)
            rho = K['k'] * t
            x, y = rho * xp.sin(dl), -sgn * rho * xp.cos(dl)
        else:
            D = 1 + K['sin_chi1'] * xp.sin(chi) + K['cos_chi1'] * xp.cos(chi) * xp.cos(dl)
            A = xp.div(K['k'], D)
            x = A * xp.cos(chi) * xp.sin(dl)
            y = A * (K['cos_chi1'] * xp.sin(chi) - K['sin_chi1'] * xp.cos(chi) * xp.cos(dl))
        inside = xp.no(xp.lt(D, 1 + 0 * D))
    keep = ok & inside
    return xp.where(keep, x, xp.nan + 0 * lat), xp.where(keep, y, xp.nan + 0 * lat)


def _latitude_of(xp, e, S, H):
    """phi (radians) of the conformal latitude with sin chi : cos chi = S : H (H >= 0, not both 0) by the iteration (3-4)"""
    n = xp.sqrt(S * S + H * H)
    Hs = xp.where(xp.eq(H, 0 * H), 1 + 0 * H, H)
    up = xp.div(n + S, Hs)                              # tan(pi/4 + chi/2) = (1 + sin chi) / cos chi
    down = xp.div(Hs, n - S)
    T = xp.where(xp.lt(S, 0 * S), down, up)
    phi = 2 * xp.atan(T) - xp.pi / 2
    for _ in range(xp.iterations):
        phi = 2 * xp.atan(T * xp.div(1 + 0 * T, _pow_ratio(xp, e, xp.sin(phi), e / 2))) - xp.pi / 2
    pole = xp.where(xp.lt(S, 0 * S), -xp.pi / 2 + 0 * S, xp.pi / 2 + 0 * S)
    return xp.where(xp.eq(H, 0 * H), pole, phi)


def inverse(xp, P, x, y):
    """(lat, lon) in degrees of the plane point (x, y); lon in [-180, 180)"""
    x, y = xp.num(x), xp.num(y)
    ok = xp.finite(x) & xp.finite(y)
    K = constants(xp, P)
    lon0 = xp.num(P['lon0'])
    rho = xp.sqrt(x * x + y * y)
    if P['kind'] == 'paeqd':
        sgn = K['mode']
        colat = _deg(xp, rho / K['k'])
        lat = sgn * (90 - colat)
        dl = xp.atan2(x, (0 - y) if sgn > 0 else (y + 0))
        ok = ok & xp.no(xp.lt(xp.num(180.0), colat))
    elif K['mode']:
        sgn = K['mode']
        # (21-39): t = rho / k, chi = +-(pi/2 - 2 atan t): sin chi : cos chi = +-(1 - t^2) : 2 t
        t = rho / K['k']
        lat = _deg(xp, _latitude_of(xp, K['e'], sgn * (1 - t * t), 2 * t))
        dl = xp.atan2(x, (0 - y) if sgn > 0 else (y + 0))
    else:
        c = 2 * xp.atan(rho / K['k'])                                                       # (21-15)
        safe = xp.where(xp.eq(rho, 0 * rho), 1 + 0 * rho, rho)
        S = xp.cos(c) * K['sin_chi1'] + (y / safe) * xp.sin(c) * K['cos_chi1']              # sin chi
        Cc = xp.cos(c) * K['cos_chi1'] - (y / safe) * xp.sin(c) * K['sin_chi1']             # cos chi cos dlon
        Cs = (x / safe) * xp.sin(c)                                                         # cos chi sin dlon
        lat = _deg(xp, _latitude_of(xp, K['e'], S, xp.sqrt(Cc * Cc + Cs * Cs)))
        dl = xp.atan2(Cs, Cc)
    lon = _wrap(xp, lon0 + _deg(xp, dl))
    return xp.where(ok, lat, xp.nan + 0 * x), xp.where(ok, lon, xp.nan + 0 * x)


def points(xp, fn, P, u, v):
    """fn (forward / inverse) on arrays u, v: whole arrays for the array types, point by point for mpmath -> two arrays of
    np.longdouble (the mpmath values rounded to it)"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if not isinstance(xp, RO.MultiPrecision):
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            a, b = fn(xp, P, u, v)
        return np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    out = np.empty((2, u.size), dtype=np.longdouble)
    for i, (p, q) in enumerate(zip(u.ravel(), v.ravel())):
        if not (math.isfinite(p) and math.isfinite(q)):
            out[:, i] = np.nan
            continue
        a, b = fn(xp, P, p, q)
        out[0, i], out[1, i] = to_longdouble(xp, a), to_longdouble(xp, b)
    return out[0].reshape(u.shape), out[1].reshape(u.shape)


def to_longdouble(xp, v):
    """an mpmath number as np.longdouble: the float64 nearest to it plus the remainder"""
    if xp.mp.isnan(v):
        return np.longdouble('nan')
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - xp.mp.mpf(hi)))
