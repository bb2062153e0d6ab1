"""
NumPy statement of mosaic binning (auromat_amd.resample.resampleMosaic): every member's kept centres binned on the common
edges by oracle.ref_numpy.histogram2d, restricted to the member's window of the grid, then the overlap rule — the union
(the sums of every member) or the highest mean elevation (the lower member index on a tie).  A plain helper module for
the mosaic tests.
"""
import numpy as np

from oracle import ref_numpy as O


def member_planes(x, y, keep, values, xedges, yedges, window=None):
    """histogram2d of one member: (count (nx, ny), sums (k, nx, ny)) of the kept points, zero outside `window`
    ((x0, y0, nx, ny) in cells; None: the whole grid).  values: (n, k) float64."""
    x, y = np.ravel(x).astype(np.float64), np.ravel(y).astype(np.float64)
    keep = np.ravel(keep).astype(bool)
    values = np.asarray(values, dtype=np.float64).reshape(len(x), -1)
    x, y, values = x[keep], y[keep], values[keep]
    hs, _, _ = O.histogram2d(x, y, bins=[np.asarray(xedges), np.asarray(yedges)],
                             weights=[None] + [values[:, k] for k in range(values.shape[1])])
    count, sums = hs[0], np.array(hs[1:]).reshape(values.shape[1], *hs[0].shape)
    if window is not None:
        x0, y0, wnx, wny = window
        inside = np.zeros(count.shape, bool)
        inside[x0:x0 + wnx, y0:y0 + wny] = True
        count = np.where(inside, count, 0.0)
        sums = np.where(inside[None], sums, 0.0)
    return count, sums


def _layout(a):
    """(nx, ny) histogram plane -> rows north to south (ny, nx), as resample lays it out"""
    return np.flipud(a.T)


def mosaic(members, xedges, yedges, rule, nchan):
    """members: list of (x, y, keep, values (n, nchan + 1: image channels then elevation), window).
    Returns dict(mean (ny, nx, nchan + 1) NaN where empty, img (ny, nx, nchan) round-half-even of the channel means,
    count (ny, nx), source (ny, nx) int (-1 empty), elev (n_members, ny, nx) each member's own mean elevation)."""
    planes = [member_planes(x, y, keep, values, xedges, yedges, window) for x, y, keep, values, window in members]
    counts = np.array([_layout(c) for c, _ in planes])                             # (m, ny, nx)
    sums = np.array([[_layout(s) for s in ss] for _, ss in planes])                # (m, k, ny, nx)
    with np.errstate(invalid='ignore', divide='ignore'):
        own = sums / counts[:, None]
    present = counts > 0
    first = np.where(present.any(0), np.argmax(present, axis=0), -1)
    if rule == 0:
        count = counts.sum(0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = np.moveaxis(sums.sum(0) / count, 0, -1)
        source = first
    else:
        el = np.where(present, own[:, -1], -np.inf)
        source = np.where(present.any(0), np.argmax(el, axis=0), -1)            # argmax: the first of equal maxima
        pick = np.clip(source, 0, None)
        count = np.where(source >= 0, np.take_along_axis(counts, pick[None], 0)[0], 0.0)
        mean = np.moveaxis(np.take_along_axis(own, pick[None, None], 0)[0], 0, -1)
    mean = np.where((count > 0)[..., None], mean, np.nan)
    img = np.where((count > 0)[..., None], np.rint(np.nan_to_num(mean[..., :nchan])), 0)
    return dict(mean=mean, img=img, count=count, source=source, elev=np.where(present, own[:, -1], np.nan))
