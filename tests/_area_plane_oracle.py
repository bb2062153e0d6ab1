"""
TEST INFRASTRUCTURE — the contract of ``amt_area_plane_frame`` (auromat_amd/csrc/amt_area.hip, the plane form of the area-weighted
binning) in NumPy, for tests/test_gpu_area_plane_cells.py and tests/test_gpu_resample_projected.py.  A case is an
``AreaCase`` of tests/_area_cases.py whose ``lon`` / ``lat`` arrays hold the corners' x / y.  The weights and the candidate cells are
those of tests/_area_oracle.py; the admission rule is stated here, because it is the one thing that differs: there is no wrap and
no rule on a quadrilateral's extent in x.
"""
import numpy as np

import _area_oracle as O


def admitted(case):
    """flat indices of the pixels that take part, X (n, 4), Y (n, 4): corners (r, c), (r, c+1), (r+1, c+1), (r+1, c)"""
    h, w = case.height, case.width
    ok = np.isfinite(np.asarray(case.lat_c, dtype=np.float64).reshape(h * w))
    if case.elev is not None and not (np.isinf(case.min_elevation) and case.min_elevation < 0):
        with np.errstate(invalid='ignore'):
            ok &= np.asarray(case.elev, dtype=np.float64).reshape(h * w) >= case.min_elevation
    if case.mask is not None:
        ok &= np.asarray(case.mask).reshape(h * w) == 0
    y, x = (np.asarray(v, dtype=np.float64).reshape(h + 1, w + 1) for v in (case.lat, case.lon))
    corner = lambda v: np.stack([v[:-1, :-1], v[:-1, 1:], v[1:, 1:], v[1:, :-1]], axis=2).reshape(h * w, 4)
    Y, X = corner(y), corner(x)
    ok &= np.isfinite(Y).all(axis=1) & np.isfinite(X).all(axis=1)
    idx = np.nonzero(ok)[0]
    return idx, X[idx], Y[idx]


def accumulate(case):
    """The accumulators of ``amt_area_plane_frame``: int64 (nch + 2, nx, ny)"""
    xedges, yedges = np.asarray(case.xedges, dtype=np.float64), np.asarray(case.yedges, dtype=np.float64)
    nx, ny = len(xedges) - 1, len(yedges) - 1
    h, w = case.height, case.width
    img = np.asarray(case.img).reshape(h * w, -1)
    nch = img.shape[1]
    idx, X, Y = admitted(case)
    ix0, nxr, iy0, nyr = O.candidate_ranges(X, Y, xedges, yedges)
    counts = nxr * nyr
    pix = np.repeat(np.arange(len(idx)), counts)
    k = np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)
    ix, iy = ix0[pix] + k // np.maximum(nyr[pix], 1), iy0[pix] + k % np.maximum(nyr[pix], 1)
    W = O.cell_weights(X[pix], Y[pix], xedges[ix], xedges[ix + 1], yedges[iy], yedges[iy + 1])
    acc = np.zeros((nch + 2, nx * ny), dtype=np.int64)
    cell = ix * ny + iy
    np.add.at(acc[0], cell, W)
    for c in range(nch):
        np.add.at(acc[1 + c], cell, W * img[idx[pix], c].astype(np.int64))
    if case.elev is not None:
        elev = np.asarray(case.elev, dtype=np.float64).reshape(h * w)[idx]
        E = np.rint(np.where(np.isnan(elev), 0.0, elev) * O.ELEV_FIX).astype(np.int64)
        np.add.at(acc[1 + nch], cell, W * E[pix])
    return acc.reshape(nch + 2, nx, ny), counts
