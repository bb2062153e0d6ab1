"""
NumPy and Python-integer statement of mean binning (amt_bin_frame + amt_bin_frame_finalize[_window]), of the mosaic
(amt_mosaic_frames) and of the float histogram (amt_hist2d_accumulate + amt_hist2d_finalize_mean).  A plain helper module
for tests/test_gpu_bin_cells.py and tests/test_bin_cases_cpu.py; nothing in it is taken from the library.

Membership: _median_oracle.cell_index (pinned to the reference's histogram2d rule) after the keep rule of
_median_cases.Case.keep().  On top of it, per cell (and per member of a mosaic, restricted to the member's window):

* count by np.bincount, channel sums in int64 by np.add.at (exact);
* the elevation twice.  (1) The fixed-point statement of the feature: fx = sum(rint(elev * 2**32)) in int64 — elev * 2**32
  is exact in float64 and np.rint rounds half to even — and the mean (float64(fx) / 2**32) / float64(count): the device
  must give these bits, and fx itself where its accumulators are visible.  (2) The exact mean of the cell's elevations as a
  fractions.Fraction: the device must lie within EXACT_BOUND(mean) = 2**-33 + 2 * spacing(|mean|) of it — every sample is
  rounded by at most 2**-33 deg, the integer sum is exact, and of the steps that follow (fx to float64, the division by
  2**32, the division by the count) the middle one is exact and the other two each round by at most half a spacing of
  their result; the first one's half spacing, of the sum, is at most one spacing of the mean once divided by the count.
  A frame without an elevation array sums zeros: fx = 0, mean elevation 0.0 in every non-empty cell.
* channel mean float64(sum) / float64(count), one correctly rounded division (every sum stays below 2**53: asserted);
  image np.rint of it, cast; mask count == 0; NaN / 0 in empty cells.
* mosaic: rule 0 adds the members' integer planes (source: the first member present); rule 1 takes the member with the
  largest (float64(fx) / 2**32) / count, the first on a tie.  All from integers, so `source` is exact.
* hist2d: counts by bincount; sums of integer-valued weights exactly; sums of real weights by math.fsum per cell with the
  bound (n_cell - 1) * 2**-53 * sum(|w|) of a float64 summation in any order.
"""
import math
from fractions import Fraction

import numpy as np

import _median_oracle as M

FIX = 2.0 ** 32


def cell_xy(case):
    """0-based (ix, iy) of every pixel on the case's axes (iy ascending with latitude), -1 / -1 for the pixels that the keep
    rule or the edges exclude."""
    nx, ny = len(case.xedges) - 1, len(case.yedges) - 1
    ix = M.axis_index(np.ravel(case.lon_binned), case.xedges) - 1
    iy = M.axis_index(np.ravel(case.lat), case.yedges) - 1
    ok = case.keep() & (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    return np.where(ok, ix, -1), np.where(ok, iy, -1)


def cells(case, window=None):
    """Output cell (rows north to south) of every pixel, -1 for excluded ones; window = (x0, y0, nx, ny) in cells."""
    flat = case.flat()
    if window is not None:
        x0, y0, wnx, wny = window
        ix, iy = cell_xy(case)
        flat = np.where((ix >= x0) & (ix < x0 + wnx) & (iy >= y0) & (iy < y0 + wny), flat, -1)
    return flat


def fixed_point(elev):
    """rint(elev * 2**32) as int64: the 31.32 fixed-point value of every sample."""
    scaled = np.asarray(elev, dtype=np.float64) * FIX            # exact: a power of two
    assert np.all(np.abs(scaled) < 2.0 ** 62)
    return np.rint(scaled).astype(np.int64)


def planes(case, window=None):
    """Integer planes of one frame in the output layout: dict(count (ny, nx) int64, sums (ny, nx, nch) int64, fx (ny, nx) int64)."""
    ny, nx = case.shape
    nch = case.img.shape[1]
    flat = cells(case, window)
    sel = flat >= 0
    f = flat[sel]
    count = np.bincount(f, minlength=nx * ny).astype(np.int64)
    sums = np.zeros((nx * ny, nch), dtype=np.int64)
    for ch in range(nch):
        np.add.at(sums[:, ch], f, case.img[sel, ch].astype(np.int64))
    assert (sums < 2 ** 53).all()
    fx = np.zeros(nx * ny, dtype=np.int64)
    if case.elev is not None:
        e = case.elev[sel]
        assert not np.isnan(e).any(), 'a kept pixel has a NaN elevation'
        fxs = fixed_point(e)
        assert np.abs(fxs).astype(np.float64).sum() < 2.0 ** 63, 'the 31.32 sum would overflow'
        np.add.at(fx, f, fxs)
    return dict(count=count.reshape(ny, nx), sums=sums.reshape(ny, nx, nch), fx=fx.reshape(ny, nx))


def finalize(p, dtype):
    """Mean, image, mask and count from integer planes."""
    count, sums, fx = p['count'], p['sums'], p['fx']
    assert (sums < 2 ** 53).all()
    dc = count.astype(np.float64)
    full = count > 0
    safe = np.where(full, dc, 1.0)
    chan = np.where(full[..., None], sums.astype(np.float64) / safe[..., None], np.nan)
    el = np.where(full, (fx.astype(np.float64) / FIX) / safe, np.nan)
    img = np.where(full[..., None], np.rint(np.nan_to_num(chan)), 0).astype(dtype)
    out = dict(p)
    out.update(mean=np.concatenate([chan, el[..., None]], axis=2), img=img, mask=(~full).astype(np.uint8), count_f=dc)
    return out


def frame(case, window=None):
    return finalize(planes(case, window), case.img.dtype)


def mosaic(members, windows, rule):
    """members: Cases on common edges; windows: (x0, y0, nx, ny) per member (nx or ny 0: empty).  Returns the finalised dict
    with `source` (ny, nx) int32 (-1 where empty) and the members' own planes (`members`)."""
    own = [planes(c, w) for c, w in zip(members, windows)]
    counts = np.array([p['count'] for p in own])
    present = counts > 0
    anyone = present.any(0)
    if rule == 0:
        total = dict(count=counts.sum(0), sums=sum(p['sums'] for p in own), fx=sum(p['fx'] for p in own))
        source = np.where(anyone, np.argmax(present, axis=0), -1)
    else:
        with np.errstate(invalid='ignore', divide='ignore'):
            el = np.array([(p['fx'].astype(np.float64) / FIX) / p['count'].astype(np.float64) for p in own])
        el = np.where(present, el, -np.inf)
        pick = np.argmax(el, axis=0)                                # the first of equal maxima
        source = np.where(anyone, pick, -1)
        take = lambda key: np.where(anyone.reshape(anyone.shape + (1,) * (own[0][key].ndim - 2)),
                                    np.take_along_axis(np.array([p[key] for p in own]),
                                                       pick.reshape((1,) + pick.shape + (1,) * (own[0][key].ndim - 2)), 0)[0], 0)
        total = dict(count=take('count'), sums=take('sums'), fx=take('fx'))
    out = finalize(total, members[0].img.dtype)
    out.update(source=source.astype(np.int32), members=own)
    return out


# ---- the exact mean ----------------------------------------------------------------------------------------------------
def exact_sum(values):
    """Sum of float64 values as a Fraction (Python integers over the largest power-of-two denominator)."""
    v, n = np.unique(np.asarray(values, dtype=np.float64), return_counts=True)
    ratios = [x.as_integer_ratio() for x in v.tolist()]
    den = max(d for _, d in ratios)
    return Fraction(sum(k * num * (den // d) for (num, d), k in zip(ratios, n.tolist())), den)


def exact_bound(mean):
    return Fraction(1, 2 ** 33) + 2 * Fraction(float(np.spacing(abs(float(mean)))))


def exact_means(flat, elev):
    """[(output cell, count, exact mean elevation as a Fraction)] of every non-empty cell."""
    sel = np.flatnonzero(flat >= 0)
    order = sel[np.argsort(flat[sel], kind='stable')]
    f = flat[order]
    e = np.asarray(elev, dtype=np.float64)[order]
    cut = np.flatnonzero(np.diff(f)) + 1
    starts = np.concatenate(([0], cut)).tolist()
    ends = np.concatenate((cut, [len(f)])).tolist()
    return [(int(f[a]), b - a, exact_sum(e[a:b]) / (b - a)) for a, b in zip(starts, ends)]


def worst_exact_error(means, got_elevation):
    """(largest |got - exact| / bound over the cells, its cell) — the check is that this is <= 1."""
    got = np.ravel(got_elevation)
    worst, where = Fraction(0), -1
    for cell, _, mean in means:
        r = abs(Fraction(float(got[cell])) - mean) / exact_bound(mean)
        if r > worst:
            worst, where = r, cell
    return float(worst), where


# ---- the float histogram -----------------------------------------------------------------------------------------------
def hist2d(x, y, weights, xedges, yedges):
    """Accumulator planes in the device's layout (nx * ny, cell ix * ny + iy): count float64, and per weight array
    (sum float64 by math.fsum, bound of a float64 summation in any order — 0 where every weight is an integer)."""
    nx, ny = len(xedges) - 1, len(yedges) - 1
    ix = M.axis_index(np.ravel(x), xedges) - 1
    iy = M.axis_index(np.ravel(y), yedges) - 1
    ok = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    cell = ix[ok] * ny + iy[ok]
    count = np.bincount(cell, minlength=nx * ny)
    order = np.argsort(cell, kind='stable')
    bounds = np.concatenate(([0], np.cumsum(count)))
    out = []
    for w in weights:
        w = np.asarray(w, dtype=np.float64)[ok]
        if np.array_equal(w, np.rint(w)):
            s = np.zeros(nx * ny, dtype=np.int64)
            np.add.at(s, cell, w.astype(np.int64))
            a = np.zeros(nx * ny, dtype=np.int64)
            np.add.at(a, cell, np.abs(w).astype(np.int64))
            assert (a < 2 ** 53).all()
            out.append((s.astype(np.float64), np.zeros(nx * ny)))
            continue
        ws = w[order]
        s, bound = np.zeros(nx * ny), np.zeros(nx * ny)
        for c in np.flatnonzero(count):
            part = ws[bounds[c]:bounds[c + 1]]
            s[c] = math.fsum(part)
            bound[c] = (len(part) - 1) * 2.0 ** -53 * math.fsum(np.abs(part))
        out.append((s, bound))
    return count.astype(np.float64), out


def hist_layout(plane, nx, ny):
    """(nx * ny) accumulator plane -> (ny, nx) rows north to south"""
    return np.flipud(np.asarray(plane).reshape(nx, ny).T)
