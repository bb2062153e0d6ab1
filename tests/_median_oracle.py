"""
NumPy statement of median binning (auromat_amd.resample.resampleMedian): the pixels histogram2d puts into a cell
(oracle.ref_numpy.histogram2d's rule: searchsorted(edges, v, 'right') and the right-most-edge rule), then np.median of
each channel over them, by one lexsort on (cell, value).  A plain helper module for the median tests.
"""
import numpy as np


def axis_index(v, edges):
    """1-based bin of every value by histogram2d's rule (util/histogram.py:178-224); 0 and len(edges) are outliers."""
    v = np.asarray(v, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    c = np.searchsorted(edges, v, 'right')
    mindiff = np.diff(edges).min()
    if not np.isinf(mindiff):
        decimal = int(-np.log10(mindiff)) + 6
        with np.errstate(invalid='ignore'):
            on_edge = np.around(v, decimal) == np.around(edges[-1], decimal)
            c[np.where(on_edge & (v >= edges[-1]))[0]] -= 1
    return c


def cell_index(x, y, xedges, yedges):
    """Flat cell of every point in the output layout of resample (rows north to south: row = ny-1-iy, column = ix),
    -1 for points outside the edges or with a NaN coordinate."""
    nx, ny = len(xedges) - 1, len(yedges) - 1
    ix = axis_index(np.ravel(x), xedges) - 1
    iy = axis_index(np.ravel(y), yedges) - 1
    ok = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    return np.where(ok, (ny - 1 - iy) * nx + ix, -1)


def median_bins(x, y, values, xedges, yedges, keep=None):
    """np.median per cell and channel of `values` (n, k) over the points of each cell.
    keep: optional bool mask of the points to bin.  Returns (median (ny, nx, k) float64 NaN where empty, count (ny, nx))."""
    nx, ny = len(xedges) - 1, len(yedges) - 1
    values = np.asarray(values).reshape(len(np.ravel(x)), -1)
    flat = cell_index(x, y, xedges, yedges)
    if keep is not None:
        flat = np.where(np.ravel(keep), flat, -1)
    sel = flat >= 0
    f, v = flat[sel], values[sel]
    count = np.bincount(f, minlength=nx * ny)
    start = np.concatenate(([0], np.cumsum(count)[:-1]))
    full = count > 0
    n = count[full]
    lo, hi = start[full] + (n - 1) // 2, start[full] + n // 2
    med = np.full((nx * ny, v.shape[1]), np.nan)
    for k in range(v.shape[1]):
        sv = v[np.lexsort((v[:, k], f)), k]
        med[full, k] = (sv[lo].astype(np.float64) + sv[hi].astype(np.float64)) / 2
    return med.reshape(ny, nx, v.shape[1]), count.reshape(ny, nx).astype(np.float64)


def median_loop(x, y, values, xedges, yedges, keep=None):
    """The same by a plain loop over the cells with np.median (what median_bins is checked against)."""
    nx, ny = len(xedges) - 1, len(yedges) - 1
    values = np.asarray(values).reshape(len(np.ravel(x)), -1)
    flat = cell_index(x, y, xedges, yedges)
    if keep is not None:
        flat = np.where(np.ravel(keep), flat, -1)
    med = np.full((nx * ny, values.shape[1]), np.nan)
    for c in np.unique(flat[flat >= 0]):
        med[c] = np.median(values[flat == c], axis=0)
    return med.reshape(ny, nx, values.shape[1])


def odd_gap_pairs(x, y, values, xedges, yedges, keep=None):
    """Number of (cell, channel) pairs with an even count whose two middle values differ by an odd amount (their mean
    ends in .5: the image's rounding half to even decides it)."""
    nx, ny = len(xedges) - 1, len(yedges) - 1
    values = np.asarray(values).reshape(len(np.ravel(x)), -1)
    flat = cell_index(x, y, xedges, yedges)
    if keep is not None:
        flat = np.where(np.ravel(keep), flat, -1)
    sel = flat >= 0
    f, v = flat[sel], values[sel].astype(np.int64)
    count = np.bincount(f, minlength=nx * ny)
    start = np.concatenate(([0], np.cumsum(count)[:-1]))
    even = (count > 0) & (count % 2 == 0)
    n = count[even]
    total = 0
    for k in range(v.shape[1]):
        sv = v[np.lexsort((v[:, k], f)), k]
        a, b = sv[start[even] + n // 2 - 1], sv[start[even] + n // 2]
        total += int(((b - a) % 2 == 1).sum())
    return total
