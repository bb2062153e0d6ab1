"""
TEST INFRASTRUCTURE — high-precision reference of what the fused row kernel (k_georef_rows, camera-model form) computes, and of
the two bounding-box reductions on camera frames.

The inputs are the float64 numbers of a case of tests/_camera_cases.py — the content of amt_frame_params — taken as exact.
Nothing is restated that another test module already holds:
  directions     the generic TAN direction of tests/_coord_oracle.py (_tan_direction: wcs.py:93-142 through the two native
                 angles) at corner (column - 1/2, row - 1/2) and, for exact centres, at (column, row)
  corners        shell_hit, geodetic_deg and mlat_mlt of tests/_rowfield_oracle.py, composed as its `corner` composes them
  fast centres   `centre` of tests/_rowfield_oracle.py: mean of four hits and four directions
  exact centres  `exact_centre` below: the pixel's own ray, its own hit, the elevation of that ray at that hit
                 (astrometry.py:103-105, 200-212) — not the kernel's half-column step from the corner's ray
np.longdouble on whole frames, mpmath (50 digits) on single corners and centres; where a ray all but grazes the shell
(|relative discriminant| < GRAZING) or an elevation is beyond STEEP the frame's values are those of the mpmath run, as in
_rowfield_oracle.reference.  E_ref comes from oracle/ref_numpy.py::georef_frame on the same parameters (the case's header holds
the same CD, CRPIX and the angles its `rot` was made from); distance and bound are those of _rowfield_oracle.

Sky rows: corner rows and pixel rows on which any corner / centre hits.  Boxes: `kernel_box` — the rule of
amt_georef_out.bbox (a pixel counts when its centre's elevation is a number >= the threshold and, with exact centres, its four
corners hit; a corner is kept when it hits and one of the up to four pixels around it counts) — and `coarse_box` — the rule
of amt_georef_coarse_bbox (lattice corners min(i stride, width), a corner counting by its own ray's elevation).
"""
import numpy as np

import _coord_oracle as C
import _rowfield_oracle as R

ARRAYS = R.ARRAYS
CORNER_ARRAYS = R.CORNER_ARRAYS
CENTRE_ARRAYS = ('lat_c', 'lon_c', 'elev', 'mlat_c', 'mlt_c')
GRAZING, STEEP = R.GRAZING, R.STEEP
distance, bound = R.distance, R.bound
_LD = R._LD


def params_of(case):
    return {k: case[k] for k in ('cd', 'crpix', 'rot', 'cam', 'a', 'b', 'a0', 'b0', 'm_geo', 'm_sm')}


def direction(xp, P, x, y):
    """pixel coordinates (0-based: a pixel's centre is (column, row)) -> unit vector, J2000"""
    return C._tan_direction(xp, P, xp.num(x), xp.num(y))


def ray_elevation(xp, d, p):
    """elevation_deg of the ray d at its own hit p (astrometry.py:200-212, utils.py:28-46): 90 - angle(-d, p / |p|)"""
    dot = -xp.div(R._dot(d, p), xp.sqrt(R._dot(p, p)))
    one = 1 + 0 * dot
    dot = xp.where(xp.lt(one, dot), one, xp.where(xp.lt(dot, -one), -one, dot))
    return 90 - xp.acos(dot) * (180 / xp.pi)


def corner(xp, d, P):
    """_rowfield_oracle.corner for a direction that is a high-precision number already (that one takes float64 directions and
    would round this one): the same four pieces in the same order"""
    p, rel = R.shell_hit(xp, d, P)
    lat, lon = R.geodetic_deg(xp, R._rot(xp, P['m_geo'], p), P)
    ml, mt = R.mlat_mlt(xp, R._rot(xp, P['m_sm'], p))
    return dict(p=p, d=d, lat=lat, lon=lon, mlat=ml, mlt=mt, rel=rel)


def exact_centre(xp, d, P):
    """A pixel's own ray (astrometry.py:103-105): own hit, coordinates of that hit, elevation from that ray"""
    c = corner(xp, d, P)
    return dict(lat_c=c['lat'], lon_c=c['lon'], mlat_c=c['mlat'], mlt_c=c['mlt'], elev=ray_elevation(xp, c['d'], c['p']),
                rel_c=c['rel'])


def _corner_xy(i, j):
    return j - 0.5, i - 0.5


def corner_mp(case, i, j, seen=None):
    """corner (i, j) in mpmath; `seen`: a dict that keeps the corners of one frame (a fast centre needs four of them)"""
    if seen is not None and (i, j) in seen:
        return seen[i, j]
    xp, P = R._mp(), params_of(case)
    x, y = _corner_xy(i, j)
    c = corner(xp, direction(xp, P, x, y), P)
    c['elev_corner'] = ray_elevation(xp, c['d'], c['p'])
    if seen is not None:
        seen[i, j] = c
    return c


def centre_mp(case, r, q, seen=None):
    """pixel (r, q) in mpmath -> the five centre values (and rel_c of an exact centre)"""
    xp, P = R._mp(), params_of(case)
    if case['fast_center']:
        c = [corner_mp(case, r + a, q + b, seen) for a, b in ((0, 0), (0, 1), (1, 1), (1, 0))]
        return R.centre(xp, c[0], c[1], c[2], c[3], P)
    return exact_centre(xp, direction(xp, P, q, r), P)


def reference(case, substitute=True):
    """The whole frame in longdouble -> the nine arrays (NaN = miss) plus 'rel' and 'elev_corner' (the elevation of a corner's
    own ray) per corner and, with exact centres, 'rel_c' per pixel.  `substitute=False`: longdouble throughout."""
    xp, P = _LD, params_of(case)
    h, w = case['height'], case['width']
    i, j = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = corner(xp, direction(xp, P, *_corner_xy(i, j)), P)
        out = {k: np.array(c[k]) for k in CORNER_ARRAYS}
        out['rel'] = np.array(c['rel'])
        out['elev_corner'] = np.array(ray_elevation(xp, c['d'], c['p']))
        if case['fast_center']:
            def part(sl):
                return dict(p=tuple(v[sl] for v in c['p']), d=tuple(v[sl] for v in c['d']))
            s00, s01 = (slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None))
            s11, s10 = (slice(1, None), slice(1, None)), (slice(1, None), slice(None, -1))
            m = R.centre(xp, part(s00), part(s01), part(s11), part(s10), P)
        else:
            m = exact_centre(xp, direction(xp, P, j[:-1, :-1], i[:-1, :-1]), P)
    out.update({k: np.array(v) for k, v in m.items()})
    if not substitute:
        return out
    with np.errstate(invalid='ignore'):
        grazing = np.argwhere(np.abs(out['rel']) < GRAZING)
        pixels = set((int(r), int(q)) for r, q in np.argwhere(np.abs(out['elev']) > STEEP))
        if not case['fast_center']:
            pixels.update((int(r), int(q)) for r, q in np.argwhere(np.abs(out['rel_c']) < GRAZING))
    seen, mp_centres = {}, {}
    for i, j in grazing:
        v = corner_mp(case, int(i), int(j), seen)
        for k in CORNER_ARRAYS + ('elev_corner',):
            out[k][i, j] = R._to_longdouble(v[k])
        if case['fast_center']:
            pixels.update((r, q) for r in (i - 1, i) for q in (j - 1, j) if 0 <= r < h and 0 <= q < w)
    for r, q in sorted(pixels):
        v = mp_centres[r, q] = centre_mp(case, r, q, seen)
        for k in CENTRE_ARRAYS:
            out[k][r, q] = R._to_longdouble(v[k])
    # the mpmath values that were taken (tests/test_camera_cases_cpu.py compares the longdouble run with every one of them)
    out['mp_corners'] = {(int(i), int(j)): seen[int(i), int(j)] for i, j in grazing}
    out['mp_centres'] = mp_centres
    return out


def float64_oracle(case):
    """oracle/ref_numpy.py::georef_frame on the same parameters -> the nine arrays"""
    from oracle import ref_numpy as O
    hdr = case['header']
    assert np.array_equal(O.wcs_rotation(hdr).ravel(), np.asarray(case['rot']).ravel())
    assert [hdr['CD1_1'], hdr['CD1_2'], hdr['CD2_1'], hdr['CD2_2'], hdr['CRPIX1'], hdr['CRPIX2']] == list(case['cd']) + list(case['crpix'])
    assert case['a'] == O.WGS84_A + case['altitude'] and case['b'] == O.WGS84_B + case['altitude']
    with np.errstate(invalid='ignore', divide='ignore'):
        g = O.georef_frame(hdr, case['altitude'], np.asarray(case['cam']), np.asarray(case['m_geo']).reshape(3, 3),
                           np.asarray(case['m_sm']).reshape(3, 3), fast=bool(case['fast_center']))
    return {k: np.asarray(g[k], dtype=np.float64) for k in ARRAYS}


# ---- sky rows -------------------------------------------------------------------------------------------------------------------
def hit_rows(ref):
    """-> (corner rows with a hit corner (h + 1,), pixel rows with a hit centre (h,))"""
    return (~np.isnan(ref['lat'])).any(axis=1), (~np.isnan(ref['lat_c'])).any(axis=1)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------
def _reduce(lat, lon, keep):
    """the eight slots of the reductions over the kept corners: min / max latitude, min / max longitude, smallest positive and
    largest non-positive longitude, and for each of the six the latitude of the corner that sets it (the weight of a longitude
    distance) -> (slots[6], latitudes[6])"""
    la, lo = np.asarray(lat, dtype=np.float64)[keep], np.asarray(lon, dtype=np.float64)[keep]
    inf = float('inf')
    slots, lats = [inf, -inf, inf, -inf, inf, -inf], [0.0] * 6
    if la.size == 0:
        return slots, lats

    def take(k, values, lats_of, pick):
        if values.size:
            n = int(pick(values))
            slots[k], lats[k] = float(values[n]), float(lats_of[n])
    take(0, la, la, np.argmin)
    take(1, la, la, np.argmax)
    take(2, lo, la, np.argmin)
    take(3, lo, la, np.argmax)
    pos = lo > 0
    take(4, lo[pos], la[pos], np.argmin)
    take(5, lo[~pos], la[~pos], np.argmax)
    return slots, lats


def kernel_box(case, ref, min_elevation, magnetic=False):
    """amt_georef_out.bbox -> (slots 0-5, their latitudes, slot 6 = the number of pixels that count)"""
    elev = np.asarray(ref['elev'], dtype=np.float64)
    hit = ~np.isnan(ref['lat'])
    with np.errstate(invalid='ignore'):
        valid = elev >= min_elevation
    if not case['fast_center']:
        valid &= hit[:-1, :-1] & hit[:-1, 1:] & hit[1:, 1:] & hit[1:, :-1]
    keep = np.zeros(hit.shape, bool)
    keep[:-1, :-1] |= valid
    keep[:-1, 1:] |= valid
    keep[1:, 1:] |= valid
    keep[1:, :-1] |= valid
    keep &= hit
    lat, lon = (ref['mlat'], (np.asarray(ref['mlt'], dtype=np.float64) - 12.0) * 15.0) if magnetic else (ref['lat'], ref['lon'])
    slots, lats = _reduce(lat, lon, keep)
    return slots, lats, int(valid.sum())


def coarse_box(case, ref, stride, min_elevation, magnetic=False):
    """amt_georef_coarse_bbox -> (slots 0-5, their latitudes, slot 6 = corners that count, slot 7 = sx 2^20 + sy over the lattice
    corners that hit: sx / sy the sum of the signs of (2 column - width) / (2 row - height))"""
    h, w = case['height'], case['width']
    gy = np.minimum(np.arange((h + stride - 1) // stride + 1) * stride, h)
    gx = np.minimum(np.arange((w + stride - 1) // stride + 1) * stride, w)
    iy, ix = np.meshgrid(gy, gx, indexing='ij')
    hit = ~np.isnan(ref['lat'])[iy, ix]
    with np.errstate(invalid='ignore'):
        keep = hit & (np.asarray(ref['elev_corner'], dtype=np.float64)[iy, ix] >= min_elevation)
    lat, lon = (ref['mlat'], (np.asarray(ref['mlt'], dtype=np.float64) - 12.0) * 15.0) if magnetic else (ref['lat'], ref['lon'])
    slots, lats = _reduce(np.asarray(lat)[iy, ix], np.asarray(lon)[iy, ix], keep)
    sx, sy = int(np.sign(2 * ix - w)[hit].sum()), int(np.sign(2 * iy - h)[hit].sum())
    return slots, lats, int(keep.sum()), float(sx * (1 << 20) + sy)


def box_distance(k, got, want, want_lat):
    """degrees between slot k of a reduction and the reference's: latitudes plain, longitudes weighted by cos(latitude) of the
    corner that sets the slot (raw longitude is ill-conditioned at a pole); both infinite (an empty slot) -> 0"""
    if np.isinf(want) or np.isinf(got):
        return 0.0 if got == want else float('inf')
    d = abs(got - want)
    return d if k < 2 else d * float(np.cos(np.deg2rad(want_lat)))
