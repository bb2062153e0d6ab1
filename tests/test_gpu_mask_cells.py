"""
The mask kernels of auromat_amd/csrc/amt_masks.hip on constructed masks: ``amt_mask_by_elevation``, ``amt_sanitize_masks`` and
``amt_bbox_corners`` against oracle.ref_numpy.mask_by_elevation / sanitize_masks and plain NumPy reductions — every output
exactly equal.  Shapes 1 x 1, 1 x 7, 7 x 1, 5 x 7 and 1024 x 1025 (more elements than the grid cap of 256 * 16 * 256 threads:
the stride loop runs twice).  Masks: nothing and everything masked (no valid pixel: n_valid = 0 and infinities), checkerboard,
one valid pixel in a corner and on an edge, holes, NaN elevations and NaN corner latitudes, an image mask with after_masking 0
and 1.  The pole-quad count: rings of dyadic longitudes around a pixel (no step is exactly +-180 deg), counted with rational
arithmetic, for each choice of mask — centre mask, corner mask, neither (tests/test_rowfield_cases_cpu.py checks without a
GPU that exactly the ring's pixel winds).
"""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (5, 7), (1024, 1025)]          # (height, width)
POISON = 0xA5


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


def dev(a, dtype):
    return _ctx().to_device(np.ascontiguousarray(a, dtype=dtype), dtype)


def poisoned(shape, dtype):
    import torch
    t = _ctx().empty(shape, dtype)
    t.view(torch.uint8).fill_(POISON)
    return t


def ring_longitudes(h, w, pi, pj):
    """corner longitudes (multiples of 1/8 deg) that go once around the centre of pixel (pi, pj)"""
    i, j = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    lon = np.degrees(np.arctan2(i - (pi + 0.5), j - (pj + 0.5)))
    return np.rint(lon * 8.0) / 8.0


def winds_exact(o00, o01, o11, o10):
    """quad_winds_pole in rational arithmetic (the longitudes are dyadic: Fraction(float) is exact)"""
    def step(a, b):
        d = Fraction(b) - Fraction(a)
        k = d / 360
        n = int(np.floor(k + Fraction(1, 2)))
        assert abs(d - 360 * n) != 180, 'a step of exactly 180 deg'
        return d - 360 * n
    return abs(step(o00, o01) + step(o01, o11) + step(o11, o10) + step(o10, o00)) > 180


def winds_numpy(lon):
    def step(a, b):
        d = b - a
        return d - 360.0 * np.rint(d / 360.0)
    o00, o01, o11, o10 = lon[:-1, :-1], lon[:-1, 1:], lon[1:, 1:], lon[1:, :-1]
    with np.errstate(invalid='ignore'):
        return np.abs(step(o00, o01) + step(o01, o11) + step(o11, o10) + step(o10, o00)) > 180.0


def scenarios(h, w):
    """(name, elevation (h, w), corner latitude (h + 1, w + 1), image mask (h, w))"""
    rng = np.random.RandomState(h * 1000 + w)
    lat = np.rint(rng.uniform(-80, 80, size=(h + 1, w + 1)) * 64.0) / 64.0
    high = np.full((h, w), 50.0)
    no_img = np.zeros((h, w), bool)
    i, j = np.mgrid[0:h, 0:w]
    out = [('none masked', high, lat, no_img), ('all masked', np.zeros((h, w)), lat, no_img),
           ('checkerboard', np.where((i + j) % 2 == 0, 50.0, 0.0), lat, no_img)]
    for name, (r, q) in (('one valid pixel in a corner', (h - 1, w - 1)), ('one valid pixel on an edge', (0, w // 2))):
        e = np.zeros((h, w))
        e[r, q] = 10.0                                          # exactly the threshold: kept
        out.append((name, e, lat, no_img))
    holes = high.copy()
    holes[rng.uniform(size=(h, w)) < 0.1] = 9.999
    holes[h // 3:h // 3 + 3, w // 2:w // 2 + 4] = -5.0
    out.append(('holes', holes, lat, no_img))
    nan_e = high.copy()
    nan_e[rng.uniform(size=(h, w)) < 0.15] = np.nan
    nan_l = lat.copy()
    nan_l[rng.uniform(size=lat.shape) < 0.15] = np.nan
    out.append(('NaN elevations', nan_e, lat, no_img))
    out.append(('NaN corner latitudes', high, nan_l, no_img))
    out.append(('NaN elevations and corner latitudes', nan_e, nan_l, no_img))
    out.append(('image mask', holes, nan_l, rng.uniform(size=(h, w)) < 0.2))
    return out


def reference_masks(elev, corner_nan, min_elevation):
    from oracle import ref_numpy as O
    with np.errstate(invalid='ignore'):
        centre = ~(elev >= min_elevation)
    if centre.all():                                            # (mask_by_elevation refuses to mask everything)
        return O.sanitize_masks(corner_nan, centre, after_masking=True)
    corner, centre2 = O.mask_by_elevation(elev, corner_nan, min_elevation)
    assert np.array_equal(centre, centre2)
    return corner, centre2


def reference_reduction(lat, lon, corner_mask, centre_mask):
    kept = ~np.isnan(lat)
    if corner_mask is not None:
        kept &= ~corner_mask
    la, lo = lat[kept], lon[kept]
    inf = np.inf
    pos, neg = lo[lo > 0], lo[~(lo > 0)]
    red = [la.min() if la.size else inf, la.max() if la.size else -inf, lo.min() if lo.size else inf,
           lo.max() if lo.size else -inf, pos.min() if pos.size else inf, neg.max() if neg.size else -inf, float(kept.sum())]
    if centre_mask is not None:
        ok = ~centre_mask
    elif corner_mask is not None:
        ok = ~(corner_mask[:-1, :-1] | corner_mask[:-1, 1:] | corner_mask[1:, :-1] | corner_mask[1:, 1:])
    else:
        ok = np.ones((lat.shape[0] - 1, lat.shape[1] - 1), bool)
    nan = np.isnan(lon)
    ok = ok & ~(nan[:-1, :-1] | nan[:-1, 1:] | nan[1:, :-1] | nan[1:, 1:])
    winds = winds_numpy(lon)
    if lon.size <= 64:                                          # the small shapes: rational arithmetic, quad by quad
        for r, q in np.argwhere(ok):
            assert winds_exact(lon[r, q], lon[r, q + 1], lon[r + 1, q + 1], lon[r + 1, q]) == bool(winds[r, q]), (r, q)
    red.append(float((winds & ok).sum()))
    return np.array(red)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_mask_kernels_equal_the_reference_rules(shape):
    import torch
    from auromat_amd._native import ptr
    h, w = shape
    ctx = _ctx()
    assert (h + 1) * (w + 1) <= 256 * 16 * 256 or shape == SHAPES[-1]
    rings = [ring_longitudes(h, w, h // 2, w // 2), ring_longitudes(h, w, 0, w - 1),
             np.rint(np.random.RandomState(5).uniform(-180, 180, size=(h + 1, w + 1)) * 8.0) / 8.0 if h * w < 100 else
             ring_longitudes(h, w, h - 1, 0) * 0.5]
    for n, (name, elev, lat, img_mask) in enumerate(scenarios(h, w)):
        corner_nan = np.isnan(lat)
        what = '%dx%d %s' % (h, w, name)
        # ---- amt_mask_by_elevation
        d_elev, d_lat = dev(elev, np.float64), dev(lat, np.float64)
        centre, corner, n_valid = poisoned((h, w), torch.uint8), poisoned((h + 1, w + 1), torch.uint8), poisoned((1,), torch.int64)
        ctx.call('amt_mask_by_elevation', ptr(d_elev), ptr(d_lat), h, w, 10.0, ptr(centre), ptr(corner), ptr(n_valid))
        want_corner, want_centre = reference_masks(elev, corner_nan, 10.0)
        got_centre, got_corner = centre.cpu().numpy(), corner.cpu().numpy()
        assert np.array_equal(got_centre, want_centre.astype(np.uint8)), what
        assert np.array_equal(got_corner, want_corner.astype(np.uint8)), what
        assert int(n_valid.cpu()[0]) == int((~want_centre).sum()), what
        if name == 'all masked':
            assert int(n_valid.cpu()[0]) == 0 and got_centre.all() and got_corner.all()
        # centre mask alone (no corner arrays)
        centre2 = poisoned((h, w), torch.uint8)
        ctx.call('amt_mask_by_elevation', ptr(d_elev), None, h, w, 10.0, ptr(centre2), None, None)
        assert np.array_equal(centre2.cpu().numpy(), got_centre), what
        # ---- amt_sanitize_masks
        from oracle import ref_numpy as O
        for after in (0, 1):
            for use_img in ((False, True) if img_mask.any() else (False,)):
                d_corner, d_centre = dev(corner_nan, np.uint8), dev(want_centre, np.uint8)
                d_img = dev(img_mask, np.uint8) if use_img else None
                ctx.call('amt_sanitize_masks', ptr(d_corner), ptr(d_centre), None if d_img is None else ptr(d_img), h, w, after)
                s_corner, s_centre = O.sanitize_masks(corner_nan, want_centre, img_mask if use_img else None, bool(after))
                assert np.array_equal(d_corner.cpu().numpy(), s_corner.astype(np.uint8)), (what, after, use_img)
                assert np.array_equal(d_centre.cpu().numpy(), s_centre.astype(np.uint8)), (what, after, use_img)
        # ---- amt_bbox_corners: every choice of mask, on a ring of longitudes
        lon = np.where(corner_nan, np.nan, rings[n % len(rings)])
        d_lon = dev(lon, np.float64)
        s_corner, s_centre = O.sanitize_masks(corner_nan, want_centre, None, False)
        for choice in ('centre', 'corner', 'neither', 'both'):
            cm = s_corner if choice in ('corner', 'both') else None
            pm = s_centre if choice in ('centre', 'both') else None
            d_cm, d_pm = (None if cm is None else dev(cm, np.uint8)), (None if pm is None else dev(pm, np.uint8))
            red = poisoned((8,), torch.float64)
            ctx.call('amt_bbox_corners', ptr(d_lat), ptr(d_lon), None if d_cm is None else ptr(d_cm),
                     None if d_pm is None else ptr(d_pm), h, w, ptr(red))
            want = reference_reduction(lat, lon, cm, pm)
            got = red.cpu().numpy()
            assert np.array_equal(got, want), (what, choice, got.tolist(), want.tolist())
            if name == 'all masked' and choice in ('corner', 'both'):
                assert got[6] == 0 and np.all(np.isinf(got[:6])) and got[7] == 0
    torch.cuda.synchronize()
