"""
TEST INFRASTRUCTURE — cameras and points for the world -> pixel kernels (amt_world_to_pixel, amt_grid_to_pixel).

Cameras: the constructed cameras of tests/_camera_cases.py (families cd, wide, limb, far, low, inside, pole, dateline: flipped and
sheared CD, CRPIX 1000 px outside the frame, limbs, a camera inside the shell, a pole, the date line), plus zenithal cameras for
SIN, ARC, STG and ZEA and SIP polynomials of order 2 and 3, one of which folds over inside the frame.

Points of a camera (`points(name)`, computed once per process in mpmath): pixel positions — the centres of the four corner
pixels, the frame's centre, a 3 x 3 lattice of pixel corners inside the frame and two positions outside it — go through the mpmath
forward; what comes out is rounded to float64 and is the input of the inverse:
  geodetic / sm   lat, lon / MLat, SM longitude of every position whose ray hits the shell (visible), and of the far root of the
                  same ray (hidden, except for a camera inside the shell)
  j2000           declination and right ascension of every position's ray (hidden exactly where the ray hits)
  bowring         the visible geodetic points again, with the latitude of the forward kernels' one Bowring step instead of the exact
                  one: how far their inverse lands from the pixel is the statement's own inconsistency (`bowring_residual`)
with the pixel position each came from and the mpmath inverse of the float64 input (x, y, elev, flags, margin).
"""
import numpy as np

import _camera_cases as K
import _inverse_oracle as O

CAMERA_FAMILIES = ('cd', 'wide', 'limb', 'far', 'low', 'inside', 'pole', 'dateline')
FRAMES = (('geodetic', O.GEODETIC), ('sm', O.SM), ('j2000', O.J2000))
AMBIGUOUS = 1e-9            # a point whose margin (see _inverse_oracle.inverse) is below this has no certain flags in float64

_ZEN = []


def _zenithal():
    if _ZEN:
        return _ZEN
    out = []

    def cam(name, proj, sip_a=None, sip_b=None, **kw):
        args = dict(w=64, h=48, nadir_angle=72.0, azimuth=35.0, scale=0.4, roll=14.0, crpix=(30.3, 25.6))
        args.update(kw)
        c = K.camera(name, 'zenithal', args.pop('w'), args.pop('h'), **dict(K.ISS, **args))
        c = K.finish(c)
        c = dict(c, projection=O.ZENITHAL.index(proj), sip_a=sip_a, sip_b=sip_b)
        return c
    for proj in ('SIN', 'ARC', 'STG', 'ZEA'):
        out.append(cam('zen-' + proj, proj))
    # the reference pixel 180 px (72 deg at 0.4 deg / px) to the left of the frame: far off the axis of the projection
    out.append(cam('zen-ARC-wide', 'ARC', crpix=(-180.0, 25.6)))
    out.append(cam('zen-ZEA-wide', 'ZEA', crpix=(-180.0, 25.6)))
    a2 = [[0.0, 1e-3, 5e-5], [-2e-3, -1e-4, 0.0], [2e-4, 0.0, 0.0]]
    b2 = [[0.0, 0.0, -1.5e-4], [1e-3, 8e-5, 0.0], [-6e-5, 0.0, 0.0]]
    out.append(cam('sip-2', 'TAN', a2, b2))
    a3 = [[0.0, 0.0, 3e-5, -1e-6], [0.0, -4e-5, 2e-6, 0.0], [1e-4, 1e-6, 0.0, 0.0], [2e-6, 0.0, 0.0, 0.0]]
    b3 = [[0.0, 0.0, -5e-5, 2e-6], [0.0, 6e-5, -1e-6, 0.0], [2e-5, 3e-6, 0.0, 0.0], [-1e-6, 0.0, 0.0, 0.0]]
    out.append(cam('sip-3', 'STG', a3, b3))
    # u + 0.02 u^2 folds over at u = -25, column 4.3 of the frame: pixel offsets U < -12.5 have no preimage
    fold = cam('sip-fold', 'TAN', [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.02, 0.0, 0.0]], None)
    fold['lattice_x_min'] = 14.0
    out.append(fold)
    _ZEN.extend(out)
    return _ZEN


def cameras():
    return [c for c in K.cases() if c['family'] in CAMERA_FAMILIES] + _zenithal()


def names():
    return [c['name'] for c in cameras()]


def by_name(name):
    return next(c for c in cameras() if c['name'] == name)


def positions(c):
    """pixel positions (x, y) of a camera's points"""
    w, h = c['width'], c['height']
    x0 = float(c.get('lattice_x_min', 0.0))
    pts = [(x0, 0.0), (w - 1.0, 0.0), (x0, h - 1.0), (w - 1.0, h - 1.0), ((x0 + w - 1.0) / 2.0, (h - 1.0) / 2.0)]
    if w >= 4 and h >= 4:
        for fy in (0.25, 0.5, 0.75):
            for fx in (0.25, 0.5, 0.75):
                pts.append((np.floor(x0 + fx * (w - x0)) - 0.5, np.floor(fy * h) - 0.5))
    pts += [(x0 - 3.25 if x0 == 0.0 else w + 2.75, -2.75), (w + 5.5, (h - 1.0) / 2.0 + 0.125)]
    return pts


_POINTS = {}


def points(name):
    """dict frame name -> dict(c0, c1, px, py [the positions they came from], expect_hidden, ref [mpmath inverse, arrays])"""
    if name in _POINTS:
        return _POINTS[name]
    c = by_name(name)
    rows = {k: [] for k in ('geodetic', 'sm', 'j2000', 'bowring')}
    inside = bool(sum((c['cam'][i] / (c['a'], c['a'], c['b'])[i]) ** 2 for i in range(3)) < 1)
    for (x, y) in positions(c):
        f = O.forward_mp(c, x, y)
        rows['j2000'].append((f['dec'], f['ra'], x, y, f['hit'], abs(f['rel']), 0.0))
        if f['hit']:
            rows['geodetic'].append((f['lat'], f['lon'], x, y, False, abs(f['rel']), 0.0))
            rows['bowring'].append((f['lat_bowring'], f['lon_bowring'], x, y, False, abs(f['rel']), 0.0))
            rows['sm'].append((f['mlat'], f['smlon'], x, y, False, abs(f['rel']), 0.0))
            if f['far_ahead'] or inside:
                # (the far root behind an outside camera cannot be: both roots of a hit lie ahead; inside it lies behind and
                # projects to the antipode of the pixel, so it is only used where it is ahead)
                if not inside:
                    rows['geodetic'].append((f['far']['lat'], f['far']['lon'], x, y, True, abs(f['rel']), 0.0))
                    rows['sm'].append((f['far']['mlat'], f['far']['smlon'], x, y, True, abs(f['rel']), 0.0))
    out = {}
    for key, frame in FRAMES + (('bowring', O.GEODETIC),):
        r = np.array(rows[key], dtype=np.float64).reshape(-1, 7)
        ref = O.inverse_arrays(O.MP(), c, frame, r[:, 0], r[:, 1])
        ref.pop('raw')
        out[key] = dict(c0=r[:, 0].copy(), c1=r[:, 1].copy(), px=r[:, 2].copy(), py=r[:, 3].copy(), expect_hidden=r[:, 4] != 0,
                        rel=r[:, 5].copy(), ref=ref)
    _POINTS[name] = out
    return out


def native(c):
    """(amt_frame_params, amt_zenithal_wcs or None) of a camera as the entry points take them"""
    p = K.native_params(c)
    return p, None if O.is_plain_tan(c) else O.zen_struct(c)


def distance(r):
    """pixels between the mpmath inverse of a point set and the positions the points came from (0 where there is no pixel)"""
    ok = (r['ref']['flags'] & O.NO_PIXEL) == 0
    return np.where(ok, np.hypot(r['ref']['x'] - r['px'], r['ref']['y'] - r['py']), 0.0)


def bowring_residual():
    """the largest distance [px], over all cameras, between a pixel position and the exact inverse of the coordinates that the
    forward's one-step Bowring latitude gives it"""
    return max([float(distance(points(n)['bowring']).max()) for n in names() if len(points(n)['bowring']['c0'])] + [0.0])


def header_of(cam):
    """the WCS header of a camera: its TAN header with the CTYPEs of its projection and its SIP cards"""
    h = dict(cam['header'])
    proj = O.ZENITHAL[int(cam.get('projection', 0))]
    oa, ob = O.sip_orders(cam)
    sip = '-SIP' if (oa or ob) else ''
    h['CTYPE1'], h['CTYPE2'] = 'RA---' + proj + sip, 'DEC--' + proj + sip
    for prefix, t, order in (('A', cam.get('sip_a'), oa), ('B', cam.get('sip_b'), ob)):
        if order:
            h[prefix + '_ORDER'] = order
            for i in range(order + 1):
                for j in range(order + 1 - i):
                    if t[i][j]:
                        h['%s_%d_%d' % (prefix, i, j)] = t[i][j]
    return h
