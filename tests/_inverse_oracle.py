"""
TEST INFRASTRUCTURE — the statement of include/auromat_hip.h "inverse georeferencing" (world -> pixel), once, over a small
arithmetic interface: in mpmath at 50 digits (`MP`: the reference of the accuracy tests) and in Python floats (`F64`: the NumPy /
float64 statement that the host pieces, the flags and resampleGather are held to).  The forward direction (pixel -> world) that
the round trips need is put together from the pieces tests/_coord_oracle.py, _rowfield_oracle.py and _camera_oracle.py already
hold (zenithal directions, shell hit, one-step Bowring, MLat / MLT, ray elevation); only the exact geodetic latitude is new.

A camera is a dict: width, height, cam, a, b, a0, b0, m_geo, m_sm (as tests/_camera_cases.py), cd, crpix, rot, and optionally
projection (0 TAN ... 4 ZEA), sip_a / sip_b (tables [p][q] or None), start_x, start_y.
"""
import math

import numpy as np

import _camera_oracle as Q
import _coord_oracle as C
import _rowfield_oracle as R

GEODETIC, SM, J2000 = 0, 1, 2
INVALID, HIDDEN, UNPROJECTABLE, NOT_CONVERGED, OUTSIDE = 1, 2, 4, 8, 16
NO_PIXEL = INVALID | UNPROJECTABLE | NOT_CONVERGED
SIP_STEPS, SIP_TOL = 20, 2.0 ** -40
ZENITHAL = C.ZENITHAL


class Float(object):
    """Python floats (IEEE double), the operations rounded one by one"""
    name = 'float64'
    pi, nan = math.pi, float('nan')
    num = staticmethod(float)
    sqrt, sin, cos, atan2, floor = (staticmethod(f) for f in (math.sqrt, math.sin, math.cos, math.atan2, math.floor))

    @staticmethod
    def finite(x):
        return math.isfinite(x)


class Multi(object):
    """mpmath at 50 digits"""
    name = 'mpmath'

    def __init__(self):
        mp = self.mp = R._mp().mp
        self.pi, self.nan = +mp.pi, mp.nan
        self.sqrt, self.sin, self.cos, self.atan2, self.floor = mp.sqrt, mp.sin, mp.cos, mp.atan2, mp.floor

    def num(self, x):
        return self.mp.mpf(float(x))

    def finite(self, x):
        return bool(self.mp.isfinite(x))


F64 = Float()
_MP = []


def MP():
    if not _MP:
        _MP.append(Multi())
    return _MP[0]


def _sip_d(xp, table, order, u, v):
    """f = sum c[p][q] u^p v^q and its partial derivatives"""
    f = fu = fv = 0 * u
    for p in range(order + 1):
        for q in range(order + 1 - p):
            c = float(table[p][q])
            if c:
                c = xp.num(c)
                f = f + c * u ** p * v ** q
                if p:
                    fu = fu + c * p * u ** (p - 1) * v ** q
                if q:
                    fv = fv + c * q * u ** p * v ** (q - 1)
    return f, fu, fv


def sip_orders(cam):
    def order(t):
        if t is None:
            return 0
        return max([p + q for p in range(len(t)) for q in range(len(t[p])) if t[p][q]] or [0])
    return order(cam.get('sip_a')), order(cam.get('sip_b'))


def world_point(xp, cam, frame, c0, c1):
    """-> (P or direction in J2000 as a 3-tuple, None) or (None, INVALID)"""
    if not (math.isfinite(c0) and math.isfinite(c1)) or abs(c0) > 90:
        return None, INVALID
    k = xp.pi / 180
    lat, lon = xp.num(c0), xp.num(c1)
    lon = lon - 360 * xp.floor((lon + 180) / 360)
    s, c, so, co = xp.sin(lat * k), xp.cos(lat * k), xp.sin(lon * k), xp.cos(lon * k)
    a, b = xp.num(cam['a']), xp.num(cam['b'])
    if frame == J2000:
        return (c * co, c * so, s), None
    if frame == SM:
        u = (c * co, c * so, s)
        m = [xp.num(v) for v in np.asarray(cam['m_sm'], dtype=np.float64).ravel()]
        j = tuple(m[i] * u[0] + m[3 + i] * u[1] + m[6 + i] * u[2] for i in range(3))
        n = xp.sqrt((j[0] / a) ** 2 + (j[1] / a) ** 2 + (j[2] / b) ** 2)
        return tuple(v / n for v in j), None
    a0, b0 = xp.num(cam['a0']), xp.num(cam['b0'])
    e2 = (a0 * a0 - b0 * b0) / (a0 * a0)
    n = a0 / xp.sqrt(1 - e2 * s * s)
    nz = n * (1 - e2)
    m = [xp.num(v) for v in np.asarray(cam['m_geo'], dtype=np.float64).ravel()]

    def to_j2000(g):
        return tuple(m[i] * g[0] + m[3 + i] * g[1] + m[6 + i] * g[2] for i in range(3))
    # P(h) = P0 + h nu (the point of the WGS84 ellipsoid and its normal, in J2000) on the shell, whose axes are J2000's as in the
    # forward: the larger root of A h^2 + 2 B h + Cq = 0 (B > 0)
    p0, nu = to_j2000((n * c * co, n * c * so, nz * s)), to_j2000((c * co, c * so, s))
    rad = (a, a, b)
    A = sum((nu[i] / rad[i]) ** 2 for i in range(3))
    B = sum(nu[i] * p0[i] / rad[i] ** 2 for i in range(3))
    Cq = sum((p0[i] / rad[i]) ** 2 for i in range(3)) - 1
    h = -Cq / (B + xp.sqrt(B * B - A * Cq))
    return tuple(p0[i] + h * nu[i] for i in range(3)), None


def inverse(xp, cam, frame, c0, c1):
    """The statement for one point -> dict(x, y, elev, flags, margin).  `margin`: how far the point is from the nearest yes / no
    decision of its flags (visibility, the projection's domain, the frame's border [px]), relative numbers; a point whose
    margin is tiny is ambiguous in float64."""
    nan = xp.nan
    out = dict(x=nan, y=nan, elev=nan, flags=0, margin=float('inf'))
    P, bad = world_point(xp, cam, frame, float(c0), float(c1))
    if bad:
        out['flags'] = bad
        return out
    cam_ = [xp.num(v) for v in cam['cam']]
    rad = (xp.num(cam['a']), xp.num(cam['a']), xp.num(cam['b']))
    cs = [cam_[i] / rad[i] for i in range(3)]
    cc = sum(v * v for v in cs)
    flags, margin = 0, float('inf')
    k = 180 / xp.pi
    if frame == J2000:
        d = P
        ds = [d[i] / rad[i] for i in range(3)]
        d_o, d_d = -sum(ds[i] * cs[i] for i in range(3)), sum(v * v for v in ds)
        disc = d_o * d_o - cc * d_d + d_d
        big = max(d_o * d_o, cc * d_d)
        margin = min(margin, abs(float(disc / big)))
        if disc >= 0:
            root = xp.sqrt(disc)
            t = d_o + root if cc < 1 else d_o - root
            margin = min(margin, abs(float(t)))
            if t >= 0:
                flags |= HIDDEN
        elev = nan
    else:
        w = [P[i] - cam_[i] for i in range(3)]
        dist = xp.sqrt(sum(v * v for v in w))
        if dist == 0:
            out['flags'] = UNPROJECTABLE
            return out
        d = tuple(v / dist for v in w)
        qc = sum(P[i] / rad[i] * cs[i] for i in range(3))
        if not cc < 1:
            margin = min(margin, abs(float(qc - 1)))
            if not qc > 1:
                flags |= HIDDEN
        cr = (d[1] * P[2] - d[2] * P[1], d[2] * P[0] - d[0] * P[2], d[0] * P[1] - d[1] * P[0])
        elev = xp.atan2(-sum(d[i] * P[i] for i in range(3)), xp.sqrt(sum(v * v for v in cr))) * k
    out['elev'] = elev
    r = [xp.num(v) for v in np.asarray(cam['rot'], dtype=np.float64).ravel()]
    l, m, n = (r[i] * d[0] + r[3 + i] * d[1] + r[6 + i] * d[2] for i in range(3))
    rho = xp.sqrt(l * l + m * m)
    proj = int(cam.get('projection', 0))
    if proj == 0:
        ok, edge = n > 0, n
    elif proj == 1:
        ok, edge = n >= 0, n
    elif proj == 2:
        ok, edge = (rho > 0 or n > 0), 1 + n
    else:
        ok, edge = n > -1, 1 + n
    if rho == 0 and not n > 0:
        ok = False
    margin = min(margin, abs(float(edge)))
    if not ok:
        out.update(flags=flags | UNPROJECTABLE, margin=margin)
        return out
    if rho == 0:
        x = y = 0 * rho
    else:
        f = (lambda: k / n, lambda: k, lambda: k * xp.atan2(rho, n) / rho, lambda: 2 * k / (1 + n),
             lambda: k * xp.sqrt(2 / (1 + n)))[proj]()
        x, y = f * m, -(f * l)
    cd = [xp.num(v) for v in cam['cd']]
    det = cd[0] * cd[3] - cd[1] * cd[2]
    U, V = (cd[3] * x - cd[1] * y) / det, (cd[0] * y - cd[2] * x) / det
    u, v = U, V
    oa, ob = sip_orders(cam)
    if oa or ob:
        done = False
        for _ in range(SIP_STEPS):
            if max(abs(u), abs(v)) > 1e30:          # (diverged: a float power would overflow)
                break
            fa, fau, fav = _sip_d(xp, cam['sip_a'], oa, u, v) if oa else (0 * u, 0 * u, 0 * u)
            fb, fbu, fbv = _sip_d(xp, cam['sip_b'], ob, u, v) if ob else (0 * u, 0 * u, 0 * u)
            j00, j11 = 1 + fau, 1 + fbv
            jd = j00 * j11 - fav * fbu
            margin = min(margin, abs(float(jd)))
            if not jd > 0:
                break
            r0, r1 = (u + fa) - U, (v + fb) - V
            du, dv = (j11 * r0 - fav * r1) / jd, (j00 * r1 - fbu * r0) / jd
            u, v = u - du, v - dv
            if not (xp.finite(u) and xp.finite(v)):
                break
            if max(abs(du), abs(dv)) <= SIP_TOL * max(1, abs(u), abs(v)):
                done = True
                break
        if not done:
            out.update(flags=flags | NOT_CONVERGED, margin=margin)
            return out
    X = u + (xp.num(cam['crpix'][0]) - 1 - xp.num(cam.get('start_x', 0.0)))
    Y = v + (xp.num(cam['crpix'][1]) - 1 - xp.num(cam.get('start_y', 0.0)))
    w_, h_ = cam['width'], cam['height']
    border = min(abs(float(X + 0.5)), abs(float(X - (w_ - 0.5))), abs(float(Y + 0.5)), abs(float(Y - (h_ - 0.5))))
    margin = min(margin, border)
    if not (X >= -0.5 and X <= w_ - 0.5 and Y >= -0.5 and Y <= h_ - 0.5):
        flags |= OUTSIDE
    out.update(x=X, y=Y, flags=flags, margin=margin)
    return out


def inverse_arrays(xp, cam, frame, c0, c1):
    """`inverse` over arrays -> dict of arrays (x, y, elev as float64 — an mpmath value is rounded once —, flags, margin)"""
    c0, c1 = np.asarray(c0, dtype=np.float64), np.asarray(c1, dtype=np.float64)
    res = [inverse(xp, cam, frame, a, b) for a, b in zip(c0.ravel(), c1.ravel())]
    out = {k: np.array([float(r[k]) for r in res], dtype=np.float64).reshape(c0.shape) for k in ('x', 'y', 'elev', 'margin')}
    out['flags'] = np.array([r['flags'] for r in res], dtype=np.uint8).reshape(c0.shape)
    out['raw'] = res
    return out


# ---- the forward direction, from the pieces the other oracles hold ---------------------------------------------------------------
def zen_struct(cam, corner=0):
    """the amt_zenithal_wcs block of a camera (also of a plain TAN one: projection 0, no SIP)"""
    from auromat_amd._native import ZenithalWcs
    w = ZenithalWcs()
    w.width, w.height, w.corner, w.projection = cam['width'], cam['height'], corner, int(cam.get('projection', 0))
    w.cd[:] = [float(v) for v in cam['cd']]
    w.crpix[:] = [float(v) for v in cam['crpix']]
    w.rot[:] = [float(v) for v in np.asarray(cam['rot']).ravel()]
    w.start_x, w.start_y = float(cam.get('start_x', 0.0)), float(cam.get('start_y', 0.0))
    w.sip_order_a, w.sip_order_b = sip_orders(cam)
    for name in ('sip_a', 'sip_b'):
        t = cam.get(name)
        if t is not None:
            for p in range(len(t)):
                for q in range(len(t[p])):
                    getattr(w, name)[p][q] = float(t[p][q])
    return w


def is_plain_tan(cam):
    return int(cam.get('projection', 0)) == 0 and sip_orders(cam) == (0, 0) and not cam.get('start_x') and not cam.get('start_y')


def exact_geodetic_deg(xp, g, cam):
    """geodetic latitude (exact: Bowring's step iterated to its fixed point) and longitude of an ECEF point, degrees"""
    a, b = xp.num(cam['a0']), xp.num(cam['b0'])
    x, y, z = g
    e2, ep2 = (a * a - b * b) / (a * a), (a * a - b * b) / (b * b)
    p = xp.sqrt(x * x + y * y)
    beta = xp.atan2(a * z, b * p)
    lat = beta
    for _ in range(60):
        lat = xp.atan2(z + ep2 * b * xp.sin(beta) ** 3, p - e2 * a * xp.cos(beta) ** 3)
        new = xp.atan2(b * xp.sin(lat), a * xp.cos(lat))
        if abs(new - beta) < xp.num(1e-45):
            break
        beta = new
    return lat * (180 / xp.pi), xp.atan2(y, x) * (180 / xp.pi)


def forward_mp(cam, x, y):
    """pixel (x, y) [0-based, centre at (column, row)] in mpmath -> dict(d, hit, rel, p, far, lat, lon [exact geodetic],
    lat_bowring, lon_bowring [the forward kernels' one step], mlat, smlon, elev, ra, dec); `far`: the other root of the ray"""
    xp = R._mp()
    w = zen_struct(cam)
    sip = sip_orders(cam) != (0, 0)
    d = C.directions_zenithal(xp, dict(w=w, col=x, row=y, sip=sip))['dirs']
    P = {k: cam[k] for k in ('cam', 'a', 'b', 'a0', 'b0', 'm_geo', 'm_sm')}
    p, rel = R.shell_hit(xp, d, P)
    k = 180 / xp.pi
    out = dict(d=d, rel=float(rel), hit=not xp.mp.isnan(p[0]), ra=float(xp.atan2(d[1], d[0]) * k) % 360.0,
               dec=float(xp.atan2(d[2], xp.sqrt(d[0] * d[0] + d[1] * d[1])) * k))
    if not out['hit']:
        return out
    camv = [xp.num(v) for v in cam['cam']]
    rad = (xp.num(cam['a']), xp.num(cam['a']), xp.num(cam['b']))
    ds, os_ = [d[i] / rad[i] for i in range(3)], [-camv[i] / rad[i] for i in range(3)]
    d_o, d_d, o_o = R._dot(ds, os_), R._dot(ds, ds), R._dot(os_, os_)
    root = xp.sqrt(d_o * d_o - o_o * d_d + d_d)
    t_far = ((d_o - root) if o_o < 1 else (d_o + root)) / d_d
    far = tuple(d[i] * t_far + camv[i] for i in range(3))

    def coords(pt):
        g = R._rot(xp, cam['m_geo'], pt)
        la, lo = exact_geodetic_deg(xp, g, cam)
        lb, lob = R.geodetic_deg(xp, g, P)
        ml, mt = R.mlat_mlt(xp, R._rot(xp, cam['m_sm'], pt))
        return dict(lat=float(la), lon=float(lo), lat_bowring=float(lb), lon_bowring=float(lob), mlat=float(ml),
                    smlon=float((mt - 12) * 15))
    out.update(coords(p))
    out['p'] = p
    out['elev'] = float(Q.ray_elevation(xp, d, p))
    out['far'] = coords(far)
    out['far_ahead'] = bool(t_far > 0)
    return out


# ---- sampling: the remap statement of tests/_lens_oracle.py and the masking rules of resampleGather ----------------------------------
def gather_statement(cam, frame, lat_axis, lon_axis, image, interpolation, min_elevation=None, center_mask=None, xy=None, elev=None,
                     flags=None):
    """resampleGather in NumPy on the cell centres lat_axis x lon_axis: dict(img, values, magnitude [for _lens_oracle.compare], mask,
    elevation).  `xy`, `elev`, `flags`: the
    coordinates of the point entry when they are given (the GPU tests hand them in), else the float64 statement's."""
    import _lens_oracle as L
    if xy is None:
        la, lo = np.meshgrid(np.asarray(lat_axis, dtype=np.float64), np.asarray(lon_axis, dtype=np.float64), indexing='ij')
        r = inverse_arrays(F64, cam, frame, la, lo)
        xy, elev, flags = np.stack((r['x'], r['y']), axis=-1), r['elev'], r['flags']
    h, w = image.shape[:2]
    xs, ys = xy[..., 0].astype(np.float32), xy[..., 1].astype(np.float32)
    mask = flags != 0
    with np.errstate(invalid='ignore'):
        ix = np.clip(np.nan_to_num(np.rint(xy[..., 0]), nan=0.0, posinf=0.0, neginf=0.0), 0, w - 1).astype(np.int64)
        iy = np.clip(np.nan_to_num(np.rint(xy[..., 1]), nan=0.0, posinf=0.0, neginf=0.0), 0, h - 1).astype(np.int64)
    if center_mask is not None:
        mask = mask | center_mask[iy, ix]
    values = magnitude = None
    if interpolation == 'nearest':
        img = image[iy, ix]
    else:
        values, support = L.sample(image, xs, ys, interpolation)
        magnitude, _ = L.sample(image, xs, ys, interpolation, absolute=True)
        img = L.convert(values, image.dtype)
        mask = mask | (support == 0)
    if min_elevation is not None:
        with np.errstate(invalid='ignore'):
            mask = mask | ~(elev >= min_elevation)
    return dict(img=img, values=values, magnitude=magnitude, mask=mask, elevation=elev)
