"""
The contract of the area-weighted binning (``amt_area_frame`` + ``amt_area_frame_finalize``, auromat_amd/csrc/amt_area.hip)
in NumPy, per pixel and per cell.  A plain helper module for tests/test_area_cpu.py, tests/test_gpu_area_cells.py and
tests/test_gpu_area.py.

``cell_weights`` is the twin of the kernel's ``cell_weight``: the same operations in the same order, every one rounded on its
own (NumPy never contracts a product and a sum), so the integer weights, and with them the integer accumulators, agree bit for
bit.  Nothing here looks at which cell holds a pixel's centre.
"""
import numpy as np

ONE = 4294967296.0           # 2^32: the weight of a cell that a pixel covers whole
ELEV_FIX = 65536.0           # E = rint(elev * 2^16)
LIMIT = 1 << 40              # a cell with a larger total weight: AMT_EDOMAIN


def wrap180_shifted(v):
    """wrap_at(v + 180, 180 deg) as the kernels compute it (amt_common.h)."""
    a = np.asarray(v, dtype=np.float64) + 180.0
    wraps = np.floor((a + 180.0) / 360.0)
    a = a - wraps * 360.0
    a = np.where(a >= 180.0, a - 360.0, a)
    return np.where(a < -180.0, a + 360.0, a)


def _clamp(v, hi):
    return np.minimum(np.maximum(v, 0.0), hi)


def cell_weights(X, Y, x0, x1, y0, y1):
    """W (int64, n) of quadrilaterals X, Y (n, 4) and cells [x0, x1] x [y0, y1] (n each): the boundary integral of
    clamp(y, 0, b) d clamp(x, 0, a) over the edges, every edge split at its crossings with the cell's four lines."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    a, b = x1 - x0, y1 - y0
    px, py = X - x0[:, None], Y - y0[:, None]
    S = np.zeros(len(a))
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(4):
            ax, ay, bx, by = px[:, i], py[:, i], px[:, (i + 1) & 3], py[:, (i + 1) & 3]
            dx, dy = bx - ax, by - ay
            t0 = np.where(dx != 0.0, (0.0 - ax) / dx, 0.0)
            t1 = np.where(dx != 0.0, (a - ax) / dx, 0.0)
            t2 = np.where(dy != 0.0, (0.0 - ay) / dy, 0.0)
            t3 = np.where(dy != 0.0, (b - ay) / dy, 0.0)
            t0, t1, t2, t3 = _clamp(t0, 1.0), _clamp(t1, 1.0), _clamp(t2, 1.0), _clamp(t3, 1.0)
            t0, t1 = np.minimum(t0, t1), np.maximum(t0, t1)
            t2, t3 = np.minimum(t2, t3), np.maximum(t2, t3)
            t0, t2 = np.minimum(t0, t2), np.maximum(t0, t2)
            t1, t3 = np.minimum(t1, t3), np.maximum(t1, t3)
            t1, t2 = np.minimum(t1, t2), np.maximum(t1, t2)
            ux, uy = _clamp(ax, a), _clamp(ay, b)
            for k, t in enumerate((t0, t1, t2, t3, None)):
                if t is None:
                    x, y = bx, by
                else:
                    mx, my = t * dx, t * dy
                    x, y = ax + mx, ay + my
                vx, vy = _clamp(x, a), _clamp(y, b)
                w, h = vx - ux, uy + vy
                S = S + w * h
                ux, uy = vx, vy
    A = np.abs(S) * 0.5
    f = A / (a * b)
    return np.rint(f * ONE).astype(np.int64)


def admitted(case):
    """(flat indices of the pixels that take part, X (n, 4), Y (n, 4)) and a dict with the number of pixels every skip rule
    removes, in the order the rules are stated."""
    h, w = case.height, case.width
    lat_c = np.asarray(case.lat_c, dtype=np.float64).reshape(h * w)
    skipped = {}
    ok = np.isfinite(lat_c)
    skipped['centre'] = int((~ok).sum())
    if case.elev is not None and not (np.isinf(case.min_elevation) and case.min_elevation < 0):
        with np.errstate(invalid='ignore'):
            e_ok = np.asarray(case.elev, dtype=np.float64).reshape(h * w) >= case.min_elevation
        skipped['elevation'] = int((ok & ~e_ok).sum())
        ok &= e_ok
    if case.mask is not None:
        m_ok = np.asarray(case.mask).reshape(h * w) == 0
        skipped['mask'] = int((ok & ~m_ok).sum())
        ok &= m_ok
    lat, lon = (np.asarray(v, dtype=np.float64).reshape(h + 1, w + 1) for v in (case.lat, case.lon))
    corner = lambda v: np.stack([v[:-1, :-1], v[:-1, 1:], v[1:, 1:], v[1:, :-1]], axis=2).reshape(h * w, 4)
    Y, Xraw = corner(lat), corner(lon)
    fin = np.isfinite(Y).all(axis=1) & np.isfinite(Xraw).all(axis=1)
    skipped['corner'] = int((ok & ~fin).sum())
    ok &= fin
    X = wrap180_shifted(np.where(fin[:, None], Xraw, 0.0)) if case.lon_wrap else Xraw
    with np.errstate(invalid='ignore'):
        narrow = X.max(axis=1) - X.min(axis=1) < 180.0
    skipped['extent'] = int((ok & ~narrow).sum())
    ok &= narrow
    idx = np.nonzero(ok)[0]
    return idx, X[idx], Y[idx], skipped


def candidate_ranges(X, Y, xedges, yedges):
    """(ix0, nxr, iy0, nyr): the cells whose rectangles the quadrilaterals' bounding boxes can meet (0 cells for one wholly
    outside the grid)."""
    def axis(v, edges):
        n = len(edges) - 1
        lo = np.clip(np.searchsorted(edges, v.min(axis=1), side='right') - 1, 0, n - 1)
        hi = np.clip(np.searchsorted(edges, v.max(axis=1), side='right') - 1, 0, n - 1)
        outside = (v.max(axis=1) <= edges[0]) | (v.min(axis=1) >= edges[-1])
        return lo, np.where(outside, 0, hi - lo + 1)
    ix0, nxr = axis(X, xedges)
    iy0, nyr = axis(Y, yedges)
    nxr, nyr = np.where(nyr == 0, 0, nxr), np.where(nxr == 0, 0, nyr)
    return ix0, nxr, iy0, nyr


def accumulate(case):
    """The integer accumulators of ``amt_area_frame``: int64 (nch + 2, nx, ny) (cell ix * ny + iy when flattened), and the
    number of pixels with W > 0 per cell, int64 (nx, ny)."""
    xedges, yedges = np.asarray(case.xedges, dtype=np.float64), np.asarray(case.yedges, dtype=np.float64)
    nx, ny = len(xedges) - 1, len(yedges) - 1
    h, w = case.height, case.width
    img = np.asarray(case.img).reshape(h * w, -1)
    nch = img.shape[1]
    idx, X, Y, _ = admitted(case)
    ix0, nxr, iy0, nyr = candidate_ranges(X, Y, xedges, yedges)
    counts = nxr * nyr
    pix = np.repeat(np.arange(len(idx)), counts)
    k = np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)
    ix, iy = ix0[pix] + k // np.maximum(nyr[pix], 1), iy0[pix] + k % np.maximum(nyr[pix], 1)
    W = cell_weights(X[pix], Y[pix], xedges[ix], xedges[ix + 1], yedges[iy], yedges[iy + 1])
    acc = np.zeros((nch + 2, nx * ny), dtype=np.int64)
    hits = np.zeros(nx * ny, dtype=np.int64)
    cell = ix * ny + iy
    keep = W > 0
    np.add.at(hits, cell[keep], 1)
    np.add.at(acc[0], cell, W)
    for c in range(nch):
        np.add.at(acc[1 + c], cell, W * img[idx[pix], c].astype(np.int64))
    if case.elev is not None:
        elev = np.asarray(case.elev, dtype=np.float64).reshape(h * w)[idx]
        E = np.where(np.isnan(elev), 0.0, np.rint(np.where(np.isnan(elev), 0.0, elev) * ELEV_FIX)).astype(np.int64)
        np.add.at(acc[1 + nch], cell, W * E[pix])
    return acc.reshape(nch + 2, nx, ny), hits.reshape(nx, ny)


def min_weight(min_coverage):
    return max(1, int(np.rint(min_coverage * ONE)))


def finalize(acc, dtype, min_coverage=0.5, least=None):
    """The outputs of ``amt_area_frame_finalize`` for accumulators (nch + 2, nx, ny): dict(area (ny, nx, nch + 1), img (ny, nx,
    nch), mask (ny, nx) uint8, coverage (ny, nx), over: a cell's total weight exceeds 2^40).  `least`: the minimum weight itself
    in place of `min_coverage`."""
    acc = np.asarray(acc, dtype=np.int64)
    nch = acc.shape[0] - 2
    lay = lambda p: np.flipud(p.T)              # cell (ix, iy) -> row ny - 1 - iy, column ix
    w = lay(acc[0])
    least = min_weight(min_coverage) if least is None else max(1, int(least))
    valid = w >= least
    dw = w.astype(np.float64)
    area = np.full(w.shape + (nch + 1,), np.nan)
    img = np.zeros(w.shape + (nch,), dtype=dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in range(nch):
            m = lay(acc[1 + k]).astype(np.float64) / dw
            area[:, :, k] = np.where(valid, m, np.nan)
            img[:, :, k] = np.where(valid, np.rint(np.where(valid, m, 0.0)), 0).astype(dtype)
        e = lay(acc[1 + nch]).astype(np.float64) / dw
        area[:, :, nch] = np.where(valid, e / ELEV_FIX, np.nan)
    return dict(area=area, img=img, mask=(~valid).astype(np.uint8), coverage=dw / ONE, over=bool((w > LIMIT).any()))


def acc_layout(acc):
    """Accumulators (nch + 2, nx, ny) as planes in the output layout (nch + 2, ny, nx)."""
    return np.stack([np.flipud(p.T) for p in acc])


def same_bits(a, b):
    """Equal bit for bit, any NaN equal to any NaN (the device's NaN and NumPy's differ in their payload bits only)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
