"""
The statement the lens kernels are tested against (include/auromat_hip.h, "lens distortion"), in NumPy float64, and its inverse
in mpmath at 30 digits.  lensfunpy is not available, so this — not lensfun's output — is the yardstick.

Radius convention (reference draw.py:1104-1148): cx = (w-1)/2, cy = (h-1)/2, norm = 2/(min(w,h)-1) (a frame one pixel wide:
norm = 2), u = (x-cx) norm, v = (y-cy) norm, r^2 = u^2+v^2;
  poly3(k1): g = 1-k1+k1 r^2      poly5(k1,k2): g = 1+k1 r^2+k2 r^4      ptlens(a,b,c): g = a r^3+b r^2+c r+1-a-b-c
Forward: corrected pixel (x, y) samples the raw frame at (cx + u g/norm, cy + v g/norm); a factor of exactly 1 gives (x, y) itself
((a n)/n need not round back to a).  Inverse: the ru with ru g(ru) = rd on the branch that starts at the centre; none beyond the
first radius where d(ru g)/dru = 0 (the model folds over there).
"""
import functools

import numpy as np

SAMPLE_MAX = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0}
BOUNDARY = 1e-6          # outputs whose exact value lies this close (in counts) to a rounding boundary may differ by one count


def constants(w, h):
    side = min(w, h) - 1
    return (w - 1) / 2.0, (h - 1) / 2.0, 2.0 / (side if side >= 1 else 1)


def g_of(model, params, r2):
    """g from r^2 (float64 arrays), the operations in the order the header states them"""
    r2 = np.asarray(r2, dtype=np.float64)
    if model == 'poly3':
        k1, = params
        return (1.0 - k1) + k1 * r2
    if model == 'poly5':
        k1, k2 = params
        return (1.0 + k1 * r2) + k2 * (r2 * r2)
    if model == 'ptlens':
        a, b, c = params
        r = np.sqrt(r2)
        return ((a * (r2 * r) + b * r2) + c * r) + (((1.0 - a) - b) - c)
    assert model == 'none'
    return np.ones_like(r2)


def radial_poly(model, params):
    """coefficients (lowest power first) of ru g(ru) as a polynomial in ru"""
    if model == 'poly3':
        k1, = params
        return [0.0, 1.0 - k1, 0.0, k1]
    if model == 'poly5':
        k1, k2 = params
        return [0.0, 1.0, 0.0, k1, 0.0, k2]
    if model == 'ptlens':
        a, b, c = params
        return [0.0, 1.0 - a - b - c, c, b, a]
    return [0.0, 1.0]


def forward(model, params, w, h, x, y):
    """raw-frame sample point of the corrected full-frame coordinates (x, y)"""
    cx, cy, norm = constants(w, h)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        u, v = (x - cx) * norm, (y - cy) * norm
        g = g_of(model, params, u * u + v * v)
        xs = np.where(g == 1.0, x, cx + (u * g) / norm)
        ys = np.where(g == 1.0, y, cy + (v * g) / norm)
    return xs, ys


def lattice(cols, rows, corner, x0=0, y0=0):
    off = -0.5 if corner else 0.0
    c = 1 if corner else 0
    xx = x0 + off + np.arange(cols + c, dtype=np.float64)
    yy = y0 + off + np.arange(rows + c, dtype=np.float64)
    return np.meshgrid(xx, yy)


def forward_grid(model, params, w, h, crop=None, corner=False):
    """(rows[+1], cols[+1], 2) forward coordinates of the (cropped) corrected image; crop = (left, top, width, height)"""
    left, top, cw, ch = crop if crop else (0, 0, w, h)
    x, y = lattice(cw, ch, corner)
    xs, ys = forward(model, params, w, h, x + left, y + top)
    return np.stack((xs, ys), axis=-1)


# ---- the inverse, in mpmath -------------------------------------------------------------------------------------------
def fold_radius(model, params):
    """The smallest ru > 0 with d(ru g)/dru = 0 as an mpf, or None when the model never folds"""
    import mpmath as mp
    p = radial_poly(model, params)
    d = [k * p[k] for k in range(1, len(p))]                   # derivative, lowest power first
    while d and d[-1] == 0.0:
        d.pop()
    if len(d) < 2:
        return None
    with mp.workdps(40):
        roots = mp.polyroots([mp.mpf(c) for c in reversed(d)], maxsteps=200, extraprec=200)
        real = sorted(mp.re(r) for r in roots if abs(mp.im(r)) < mp.mpf(10) ** -25 and mp.re(r) > 0)
    return real[0] if real else None


def _mp_eval(p, r):
    import mpmath as mp
    return mp.polyval([mp.mpf(c) for c in reversed(p)], r)


@functools.lru_cache(maxsize=None)
def _inverse_table(model, params, w, h):
    """{(|x - cx|, |y - cy|): ru / rd as mpf, or None} filled on demand; the fold's radius and largest invertible rd"""
    import mpmath as mp
    with mp.workdps(40):
        rstar = fold_radius(model, list(params))
        rd_max = _mp_eval(radial_poly(model, list(params)), rstar) if rstar is not None else None
    return {}, rstar, rd_max


def inverse_scale(model, params, w, h, dx, dy):
    """(ru / rd as mpf or None when there is no inverse, slope at ru, distance of rd from the fold's rd or None) for the raw point
    at offsets (dx, dy) pixels from the centre, at 30 digits"""
    import mpmath as mp
    table, rstar, rd_max = _inverse_table(model, tuple(params), w, h)
    key = (abs(dx), abs(dy))
    if key in table:
        return table[key]
    p = radial_poly(model, params)
    with mp.workdps(40):
        side = min(w, h) - 1
        norm = mp.mpf(2) / (side if side >= 1 else 1)
        rd = mp.sqrt((mp.mpf(dx) * norm) ** 2 + (mp.mpf(dy) * norm) ** 2)
        margin = abs(rd - rd_max) if rd_max is not None else None
        if rd_max is not None and (rd >= rd_max or rd_max <= 0):
            res = (None, None, margin)
        else:
            f = lambda r: _mp_eval(p, r) - rd                                    # noqa: E731
            if rstar is not None:
                hi = rstar
            else:
                hi = max(rd, mp.mpf(1))
                while f(hi) <= 0:
                    hi *= 2
            ru = mp.findroot(f, (mp.mpf(0), hi), solver='anderson', tol=mp.mpf(10) ** -60, maxsteps=400)
            assert 0 <= ru <= hi and abs(f(ru)) < mp.mpf(10) ** -28, (model, params, dx, dy, ru)
            d = [k * p[k] for k in range(1, len(p))]
            res = (ru / rd, _mp_eval(d, ru), margin)
    table[key] = res
    return res


def inverse_grid(model, params, w, h, crop=None, corner=False):
    """(rows[+1], cols[+1], 2) float64: where the raw frame's pixels (corners) lie in the (cropped) corrected frame, NaN where the
    model has no inverse; also the slope d(ru g)/dru there (NaN where none) and the smallest distance, in radius units, of a lattice
    point from the fold (inf without one)"""
    import mpmath as mp
    cx, cy, _ = constants(w, h)
    left, top = (crop[0], crop[1]) if crop else (0, 0)
    x, y = lattice(w, h, corner)
    out = np.full(x.shape + (2,), np.nan)
    slope = np.full(x.shape, np.nan)
    nearest = np.inf
    if any(np.isnan(k) for k in params):
        return out, slope, nearest
    for j in range(x.shape[0]):
        for i in range(x.shape[1]):
            dx, dy = float(x[j, i] - cx), float(y[j, i] - cy)          # exact: halves
            if dx == 0.0 and dy == 0.0:
                out[j, i] = (cx - left, cy - top)
                slope[j, i] = radial_poly(model, params)[1]
                continue
            s, sl, margin = inverse_scale(model, params, w, h, dx, dy)
            if margin is not None:
                nearest = min(nearest, float(margin))
            if s is None:
                continue
            with mp.workdps(40):
                out[j, i] = (float(mp.mpf(cx) + mp.mpf(dx) * s - left), float(mp.mpf(cy) + mp.mpf(dy) * s - top))
            slope[j, i] = float(sl)
    return out, slope, nearest


def inverse_newton(model, params, w, h, x, y, cap=24):
    """The kernel's inverse restated in NumPy float64: Newton's method from ru = rd, at most `cap` steps, NaN where the slope is not
    positive on the way or the steps do not settle (|step| <= 1e-13 ru).  Arrays of raw coordinates in, (X, Y) in the full corrected
    frame out.  tests/test_lens_cpu.py holds it to the mpmath inverse; it serves where a whole frame's inverse is needed."""
    cx, cy, norm = constants(w, h)
    p = radial_poly(model, params)
    d = [k * p[k] for k in range(1, len(p))]
    val = lambda c, r: sum(ck * r ** k for k, ck in enumerate(c))              # noqa: E731
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    u, v = (x - cx) * norm, (y - cy) * norm
    rd = np.sqrt(u * u + v * v)
    ru = rd.copy()
    active = rd > 0.0
    ok = np.zeros(rd.shape, dtype=bool)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for _ in range(cap):
            sl = val(d, ru)
            active &= sl > 0.0
            step = (val(p, ru) - rd) / sl
            ru = np.where(active, ru - step, ru)
            active &= ru > 0.0
            settled = active & (np.abs(step) <= 1e-13 * ru)
            ok |= settled & (val(d, ru) > 0.0)
            active &= ~settled
        s = np.where(ok, ru / rd, np.nan)
        X = np.where(s == 1.0, x, cx + (u * s) / norm)
        Y = np.where(s == 1.0, y, cy + (v * s) / norm)
    centre = rd == 0.0
    bad = any(np.isnan(k) for k in params)
    X = np.where(centre, np.nan if bad else cx, X)
    Y = np.where(centre, np.nan if bad else cy, Y)
    return X, Y


# ---- sampling ---------------------------------------------------------------------------------------------------------
def lanczos(t):
    """L(t) = sinc(t) sinc(t/4) for |t| < 4, else 0; exactly 1 at 0 and exactly 0 at the other integers"""
    t = np.asarray(t, dtype=np.float64)
    val = np.sinc(t) * np.sinc(t / 4.0)
    val = np.where(t == np.rint(t), (t == 0.0).astype(np.float64), val)
    return np.where(np.abs(t) < 4.0, val, 0.0)


def tap_weights(f, interpolation):
    """(first tap offset, weights (..., n)) of one axis for fractional positions f in [0, 1)"""
    f = np.asarray(f, dtype=np.float64)
    if interpolation == 'linear':
        return 0, np.stack((1.0 - f, f), axis=-1)
    assert interpolation == 'lanczos4'
    offs = np.arange(-3, 5, dtype=np.float64)
    w = lanczos(offs - f[..., None])
    total = np.zeros_like(f)
    for i in range(8):
        total = total + w[..., i]
    return -3, w / total[..., None]


def sample(im, xs, ys, interpolation='lanczos4', absolute=False):
    """The exact (float64) value of every output sample and the support bytes: im (h, w, c) sampled at (xs, ys).  Taps outside the
    image count 0 without renormalising; a non-finite coordinate gives 0.  absolute=True: the sum of the |weight x tap| instead, the
    magnitude that the rounding errors of any such accumulation scale with."""
    im = np.asarray(im)
    if im.ndim == 2:
        im = im[:, :, None]
    h, w, c = im.shape
    src = im.astype(np.float64)
    if absolute:
        src = np.abs(src)
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    finite = np.isfinite(xs) & np.isfinite(ys)
    with np.errstate(invalid='ignore'):
        support = finite & (xs >= 0) & (xs <= w - 1) & (ys >= 0) & (ys <= h - 1)
    # far outside no tap lies in the image wherever exactly: clamp so that the integer parts stay small
    xc = np.where(finite, np.clip(xs, -16.0, w + 16.0), -16.0)
    yc = np.where(finite, np.clip(ys, -16.0, h + 16.0), -16.0)
    ix, iy = np.floor(xc), np.floor(yc)
    lo, wx = tap_weights(xc - ix, interpolation)
    _, wy = tap_weights(yc - iy, interpolation)
    if absolute:
        wx, wy = np.abs(wx), np.abs(wy)
    ix, iy = ix.astype(np.int64) + lo, iy.astype(np.int64) + lo
    n = wx.shape[-1]
    acc = np.zeros(xs.shape + (c,))
    for j in range(n):
        row = np.zeros(xs.shape + (c,))
        ty = iy + j
        for i in range(n):
            tx = ix + i
            inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            taps = src[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)] * inside[..., None]
            row = row + wx[..., i, None] * taps
        acc = acc + wy[..., j, None] * row
    acc[~finite] = 0.0
    return acc, support.astype(np.uint8)


def convert(values, dtype):
    """exact values -> samples of `dtype`: clip(rint(v), 0, max) for uint8 / uint16 (half to even), float32 unrounded"""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return values.astype(np.float32)
    return np.clip(np.rint(values), 0.0, SAMPLE_MAX[dtype]).astype(dtype)


FLOAT_WINDOW = 2.0 ** -40


def near_boundary(values, dtype, magnitude=None):
    """Boolean array: the exact value lies inside the boundary window of a rounding boundary of `dtype`.  uint8 / uint16: within
    BOUNDARY of x.5.  float32: within 2^-40 of the sample's `magnitude` (sample(..., absolute=True)) of the midpoint of two
    float32 neighbours — a float64 accumulation of 64 products is good to about 2^-46 of that magnitude, weights that differ in their
    last bits to 2^-50 of it, so the window leaves a factor of 64; where the magnitude is 0 nothing may differ."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        lo = values.astype(np.float32)
        up = np.nextafter(lo, np.float32(np.inf)).astype(np.float64)
        dn = np.nextafter(lo, np.float32(-np.inf)).astype(np.float64)
        mid_up, mid_dn = (lo.astype(np.float64) + up) / 2, (lo.astype(np.float64) + dn) / 2
        return (np.minimum(np.abs(values - mid_up), np.abs(values - mid_dn)) <= FLOAT_WINDOW * magnitude) & (magnitude > 0)
    frac = values - np.floor(values)
    return np.abs(frac - 0.5) <= BOUNDARY


def compare(got, values, dtype, magnitude=None):
    """Number of samples of `got` that break the rule: equal to convert(values), except that a sample inside the boundary window may
    differ by one count (float32: by one float32 step of the value, or by the window where that is wider)."""
    dtype = np.dtype(dtype)
    want = convert(values, dtype)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    differs = got != want
    if not differs.any():
        return 0
    window = near_boundary(values, dtype, magnitude)
    if dtype == np.float32:
        step = np.maximum(np.spacing(np.abs(want)).astype(np.float64), FLOAT_WINDOW * magnitude)
        close = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= step
    else:
        close = np.abs(got.astype(np.int64) - want.astype(np.int64)) <= 1
    return int((differs & ~(window & close)).sum())


def remap(im, xs, ys, interpolation='lanczos4'):
    """(image of im's dtype, support) of :func:`sample`"""
    values, support = sample(im, xs, ys, interpolation)
    out = convert(values, np.asarray(im).dtype)
    return (out[:, :, 0] if np.asarray(im).ndim == 2 else out), support
