"""
Plain references for the interpolating kernels of auromat_amd/csrc/amt_nearest.hip, for tests/_interp_cases.py,
tests/test_interp_cases_cpu.py and tests/test_gpu_interp_cells.py.  NumPy, fractions and Python loops only; nothing here is
taken from the library.

* ``relax``: scipy's Gauss-Seidel gradient estimator (the operations of oracle.ref_numpy.clough_tocher_gradients, with
  sqrt(ex*ex + ey*ey) cubed by multiplication) for a fixed number of sweeps, in np.float64 or np.longdouble, with the
  per-sweep errors.
* ``clough_tocher_exact``: the Clough-Tocher element of oracle.ref_numpy.clough_tocher_value in rational arithmetic, with
  exact barycentric coordinates (the element has no square root: for float inputs the result is THE value).
* ``nearest_exact``: brute-force nearest neighbour on integers (coordinates times 64), lowest flat index on a tie.
* ``gather``: amt_nearest_gather as NumPy fancy indexing.
"""
from fractions import Fraction

import numpy as np

UNITS = 64              # dyadic coordinates: multiples of 1 / 64


# ---- gradient relaxation ---------------------------------------------------------------------------------------------------
def relax(points, indptr, indices, values, sweeps, dtype=np.float64):
    """``sweeps`` sequential Gauss-Seidel sweeps over the points in their order from zero gradients.  points (n, 2), values
    (n,).  Returns ((n, 2) gradients of ``dtype``, [largest relative change of every sweep]); a NaN change is not counted
    (Python's max(err, change) keeps err).  A point without neighbours gets NaN (0 / 0)."""
    T = dtype
    pts = np.asarray(points, dtype=np.float64).astype(T)
    f = np.asarray(values, dtype=np.float64).astype(T)
    n = len(pts)
    y = np.zeros((n, 2), dtype=T)
    nb = [[int(j) for j in indices[indptr[i]:indptr[i + 1]]] for i in range(n)]
    # the geometry does not change from sweep to sweep: the same operations on the same numbers
    geo = []
    for i in range(n):
        q0 = q1 = q3 = T(0)
        terms = []
        for j in nb[i]:
            ex, ey = pts[j, 0] - pts[i, 0], pts[j, 1] - pts[i, 1]
            l = np.sqrt(ex * ex + ey * ey)
            l3 = l * l * l
            q0 = q0 + 4 * ex * ex / l3
            q1 = q1 + 4 * ex * ey / l3
            q3 = q3 + 4 * ey * ey / l3
            terms.append((j, ex, ey, l3))
        geo.append((q0, q1, q3, terms))
    errors = []
    one = T(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        for _ in range(sweeps):
            err = T(0)
            for i in range(n):
                q0, q1, q3, terms = geo[i]
                s0 = s1 = T(0)
                fi = f[i]
                for j, ex, ey, l3 in terms:
                    df2 = -ex * y[j, 0] - ey * y[j, 1]
                    t = (6 * (fi - f[j]) - 2 * df2) / l3
                    s0 = s0 + t * ex
                    s1 = s1 + t * ey
                det = q0 * q3 - q1 * q1
                r0, r1 = (q3 * s0 - q1 * s1) / det, (-q1 * s0 + q0 * s1) / det
                change = max(abs(y[i, 0] + r0), abs(y[i, 1] + r1)) / max(one, abs(r0), abs(r1))
                y[i, 0], y[i, 1] = -r0, -r1
                if change > err:                 # False for a NaN change
                    err = change
            errors.append(err)
    return y, errors


def stopping_sweep(errors, tol):
    """First sweep (1-based) whose error is below tol, as scipy stops; None if none is."""
    for k, e in enumerate(errors):
        if e < tol:
            return k + 1
    return None


# ---- the Clough-Tocher element, exactly ------------------------------------------------------------------------------------
def _F(v):
    return Fraction(float(v))


def barycentric_exact(tri_xy, p):
    (x0, y0), (x1, y1), (x2, y2) = [(_F(a), _F(b)) for a, b in tri_xy]
    px, py = _F(p[0]), _F(p[1])
    det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    b1 = ((px - x0) * (y2 - y0) - (x2 - x0) * (py - y0)) / det
    b2 = ((x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)) / det
    return (1 - b1 - b2, b1, b2)


def barycentric_float(tri_xy, p):
    """The barycentric coordinates as float64 arithmetic gives them (the expressions of scipy and of the kernel)."""
    (x0, y0), (x1, y1), (x2, y2) = [(float(a), float(b)) for a, b in tri_xy]
    px, py = float(p[0]), float(p[1])
    det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    b1 = ((px - x0) * (y2 - y0) - (x2 - x0) * (py - y0)) / det
    b2 = ((x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)) / det
    return (1.0 - b1 - b2, b1, b2)


def clough_tocher_exact(tri_xy, p, f, grad, neighbour_centroids):
    """The element of triangle tri_xy (3, 2) at the point p, vertex values f (3,), vertex gradients grad (3, 2);
    neighbour_centroids[k]: centroid of the triangle across the edge opposite vertex k, or None on the hull.  All inputs are
    taken as the exact values of their floats; returns a Fraction."""
    P = [(_F(a), _F(b)) for a, b in tri_xy]
    f1, f2, f3 = [_F(v) for v in f]
    d = [(_F(a), _F(b)) for a, b in grad]

    def dot(u, v):
        return u[0] * v[0] + u[1] * v[1]
    e12 = (P[1][0] - P[0][0], P[1][1] - P[0][1])
    e23 = (P[2][0] - P[1][0], P[2][1] - P[1][1])
    e31 = (P[0][0] - P[2][0], P[0][1] - P[2][1])
    df12, df21 = dot(d[0], e12), -dot(d[1], e12)
    df23, df32 = dot(d[1], e23), -dot(d[2], e23)
    df31, df13 = dot(d[2], e31), -dot(d[0], e31)
    c3000, c2100, c2010 = f1, (df12 + 3 * f1) / 3, (df13 + 3 * f1) / 3
    c0300, c1200, c0210 = f2, (df21 + 3 * f2) / 3, (df23 + 3 * f2) / 3
    c0030, c1020, c0120 = f3, (df31 + 3 * f3) / 3, (df32 + 3 * f3) / 3
    c2001 = (c2100 + c2010 + c3000) / 3
    c0201 = (c1200 + c0300 + c0210) / 3
    c0021 = (c1020 + c0120 + c0030) / 3
    g = [Fraction(-1, 2)] * 3
    for k in range(3):
        if neighbour_centroids[k] is None:
            continue
        c = barycentric_exact(tri_xy, neighbour_centroids[k])
        if k == 0:
            g[k] = (2 * c[2] + c[1] - 1) / (2 - 3 * c[2] - 3 * c[1])
        elif k == 1:
            g[k] = (2 * c[0] + c[2] - 1) / (2 - 3 * c[0] - 3 * c[2])
        else:
            g[k] = (2 * c[1] + c[0] - 1) / (2 - 3 * c[1] - 3 * c[0])
    c0111 = (g[0] * (-c0300 + 3 * c0210 - 3 * c0120 + c0030) + (-c0300 + 2 * c0210 - c0120 + c0021 + c0201)) / 2
    c1011 = (g[1] * (-c0030 + 3 * c1020 - 3 * c2010 + c3000) + (-c0030 + 2 * c1020 - c2010 + c2001 + c0021)) / 2
    c1101 = (g[2] * (-c3000 + 3 * c2100 - 3 * c1200 + c0300) + (-c3000 + 2 * c2100 - c1200 + c2001 + c0201)) / 2
    c1002 = (c1101 + c1011 + c2001) / 3
    c0102 = (c1101 + c0111 + c0201) / 3
    c0012 = (c1011 + c0111 + c0021) / 3
    c0003 = (c1002 + c0102 + c0012) / 3
    b = barycentric_exact(tri_xy, p)
    m = min(b)
    b1, b2, b3, b4 = b[0] - m, b[1] - m, b[2] - m, 3 * m
    return (b1 ** 3 * c3000 + 3 * b1 ** 2 * b2 * c2100 + 3 * b1 ** 2 * b3 * c2010 + 3 * b1 ** 2 * b4 * c2001
            + 3 * b1 * b2 ** 2 * c1200 + 6 * b1 * b2 * b4 * c1101 + 3 * b1 * b3 ** 2 * c1020 + 6 * b1 * b3 * b4 * c1011
            + 3 * b1 * b4 ** 2 * c1002 + b2 ** 3 * c0300 + 3 * b2 ** 2 * b3 * c0210 + 3 * b2 ** 2 * b4 * c0201
            + 3 * b2 * b3 ** 2 * c0120 + 6 * b2 * b3 * b4 * c0111 + 3 * b2 * b4 ** 2 * c0102 + b3 ** 3 * c0030
            + 3 * b3 ** 2 * b4 * c0021 + 3 * b3 * b4 ** 2 * c0012 + b4 ** 3 * c0003)


# ---- nearest neighbour on integers -----------------------------------------------------------------------------------------
def to_units(a):
    """Dyadic coordinates -> int64 multiples of 1 / 64; asserts that nothing is lost (NaN stays out through `where`)."""
    a = np.asarray(a, dtype=np.float64)
    ok = np.isfinite(a)
    u = np.zeros(a.shape, dtype=np.int64)
    s = a[ok] * UNITS
    assert np.array_equal(s, np.rint(s)) and np.all(np.abs(s) < 2.0 ** 40), 'coordinates are no multiples of 1/64'
    u[ok] = s.astype(np.int64)
    return u


def wrap_shift_units(x):
    """wrap180_shifted on integer units: (lon + 180) wrapped into [-180, 180)."""
    full = 360 * UNITS
    return (x + 360 * UNITS) % full - 180 * UNITS


def valid_sources(lat, lon, elev=None, center_mask=None, min_elevation=None):
    """Flat bool array: the sources the kernel takes (source_xy): finite coordinates, not masked, elev >= threshold where an
    elevation array and a threshold other than -inf are given (a NaN elevation then fails)."""
    lat, lon = np.asarray(lat, dtype=np.float64).ravel(), np.asarray(lon, dtype=np.float64).ravel()
    ok = ~np.isnan(lat) & ~np.isnan(lon)
    if center_mask is not None:
        ok &= np.asarray(center_mask).ravel() == 0
    if elev is not None and min_elevation is not None and not (np.isinf(min_elevation) and min_elevation < 0):
        with np.errstate(invalid='ignore'):
            ok &= np.asarray(elev, dtype=np.float64).ravel() >= min_elevation
    return ok


def source_units(lat, lon, lon_wrap):
    """(y, x) of every source in integer units, x shifted like the device's where lon_wrap is set (invalid ones: 0)."""
    y, x = to_units(np.asarray(lat).ravel()), to_units(np.asarray(lon).ravel())
    if lon_wrap:
        x = wrap_shift_units(x)
    return y, x


def nearest_exact(lat, lon, valid, lon_wrap, target_lat, target_lon, target_mask=None):
    """(ny, nx) int64: flat index of the valid source nearest to every (target_lat[row], target_lon[col]), squared distances
    as exact integers, the lowest flat index on a tie; -1 where the target is masked or no source is valid."""
    y, x = source_units(lat, lon, lon_wrap)
    src = np.flatnonzero(valid)
    ty, tx = to_units(target_lat), to_units(target_lon)
    out = np.full((len(ty), len(tx)), -1, dtype=np.int64)
    if len(src):
        ys, xs = y[src], x[src]
        dx2 = (xs[None, :] - tx[:, None]) ** 2                       # (nx, sources)
        for row in range(len(ty)):
            d = dx2 + ((ys - ty[row]) ** 2)[None, :]
            out[row] = src[np.argmin(d, axis=1)]                      # argmin: the first = lowest index on a tie
    if target_mask is not None:
        out[np.asarray(target_mask) != 0] = -1
    return out


def cells_of(y, x, yedges_u, xedges_u):
    """Histogram cell (iy, ix) of integer coordinates on integer edges, half-open [e_i, e_i+1), clamped to the border cells
    as source_cell clamps them."""
    ny, nx = len(yedges_u) - 1, len(xedges_u) - 1
    iy = np.clip(np.searchsorted(yedges_u, y, side='right') - 1, 0, ny - 1)
    ix = np.clip(np.searchsorted(xedges_u, x, side='right') - 1, 0, nx - 1)
    return iy, ix


# ---- gather ----------------------------------------------------------------------------------------------------------------
def gather(index, img, elev):
    """amt_nearest_gather: (mean (t, nchan + 1) float64, out_img (t, nchan), out_mask (t,) uint8) for flat indices, -1 = none."""
    index = np.asarray(index, dtype=np.int64).ravel()
    nchan = img.shape[1]
    none = index < 0
    safe = np.where(none, 0, index)
    out_img = img[safe].copy()
    out_img[none] = 0
    mean = np.full((len(index), nchan + 1), np.nan)
    mean[:, :nchan] = out_img
    mean[none, :nchan] = np.nan
    if elev is not None:
        mean[:, nchan] = np.where(none, np.nan, np.asarray(elev, dtype=np.float64).ravel()[safe])
    return mean, out_img, none.astype(np.uint8)
