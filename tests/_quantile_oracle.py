"""
NumPy statement of quantile binning (auromat_amd.resample.resampleQuantile): the pixels histogram2d puts into a cell (the
membership of tests/_median_oracle.py), then ``np.quantile(values.astype(float64), q)`` of every plane over them, NumPy's
default method 'linear'.  ``quantile_loop`` says exactly that, cell by cell; ``quantile_bins`` restates NumPy's arithmetic
(numpy/lib/_function_base_impl.py: _quantile, _get_indexes, _get_gamma, _lerp) over one lexsort for frames with many cells,
and tests/test_quantile_cpu.py holds the two equal bit for bit.  A plain helper module; nothing here comes from the library.
"""
import numpy as np

import _median_oracle as M


def _flat(x, y, xedges, yedges, keep):
    flat = M.cell_index(x, y, xedges, yedges)
    if keep is not None:
        flat = np.where(np.ravel(keep), flat, -1)
    return flat


def rank_pair(n, q):
    """(k, k2, g) of np.quantile's method 'linear' for n >= 1 values and 0 <= q <= 1 (arrays broadcast): the two ranks read
    from the sorted values and the weight of the lerp.  vi = (n-1) * q in float64, k = floor(vi), g = vi - k; where
    vi >= n-1 NumPy takes index -1 for both, the last value, and g = vi - (-1) (which decides the sign of a zero result)."""
    n = np.asarray(n, dtype=np.int64)
    q = np.asarray(q, dtype=np.float64)
    top = (n - 1).astype(np.float64)
    vi = top * q
    fl = np.floor(vi)
    above = vi >= top
    g = np.where(above, vi + 1.0, vi - fl)
    k = np.where(above, n - 1, fl.astype(np.int64))
    k2 = np.where(above, n - 1, k + 1)
    return k, k2, g


def lerp(a, b, g):
    """numpy's _lerp, operation by operation: a + (b-a)*g, and b - (b-a)*(1-g) where g >= 0.5."""
    a, b, g = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(g, dtype=np.float64)
    d = b - a
    with np.errstate(invalid='ignore'):
        return np.where(g >= 0.5, b - d * (1 - g), a + d * g)


def quantile_loop(x, y, values, xedges, yedges, qs, keep=None):
    """(nq, ny, nx, k) float64, NaN where a cell is empty: a literal np.quantile per non-empty cell and plane."""
    nx, ny = len(xedges) - 1, len(yedges) - 1
    values = np.asarray(values).reshape(len(np.ravel(x)), -1)
    qs = np.asarray(qs, dtype=np.float64).reshape(-1)
    flat = _flat(x, y, xedges, yedges, keep)
    out = np.full((len(qs), nx * ny, values.shape[1]), np.nan)
    if values.shape[1]:
        order = np.argsort(flat, kind='stable')
        f = flat[order]
        cells, first = np.unique(f, return_index=True)
        last = np.concatenate((first[1:], [len(f)]))
        for c, i0, i1 in zip(cells, first, last):
            if c < 0:
                continue
            out[:, c, :] = np.quantile(values[order[i0:i1]].astype(np.float64), qs, axis=0)
    return out.reshape(len(qs), ny, nx, values.shape[1])


def quantile_bins(x, y, values, xedges, yedges, qs, keep=None):
    """The same by one lexsort per plane and NumPy's arithmetic restated.  Returns (quantile (nq, ny, nx, k), count (ny, nx))."""
    nx, ny = len(xedges) - 1, len(yedges) - 1
    values = np.asarray(values).reshape(len(np.ravel(x)), -1)
    qs = np.asarray(qs, dtype=np.float64).reshape(-1)
    flat = _flat(x, y, xedges, yedges, keep)
    sel = flat >= 0
    f, v = flat[sel], values[sel]
    count = np.bincount(f, minlength=nx * ny)
    start = np.concatenate(([0], np.cumsum(count)[:-1]))
    full = count > 0
    n = count[full]
    out = np.full((len(qs), nx * ny, v.shape[1]), np.nan)
    for p in range(v.shape[1]):
        sv = v[np.lexsort((v[:, p], f)), p].astype(np.float64)
        for j, q in enumerate(qs):
            k, k2, g = rank_pair(n, q)
            out[j, full, p] = lerp(sv[start[full] + k], sv[start[full] + k2], g)
    return out.reshape(len(qs), ny, nx, v.shape[1]), count.reshape(ny, nx).astype(np.float64)
