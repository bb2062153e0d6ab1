"""
NumPy statement of the median and quantile mosaics (``amt_mosaic_median_frames``, ``amt_mosaic_quantile_frames``;
auromat_amd.resample.resampleMosaic(statistic='median' | 'quantile')).  A plain helper module for
tests/test_gpu_mosaic_quantile_cells.py and tests/test_mosaic_quantile_cpu.py; nothing in it is taken from the library.

Per member the output cell of every pixel inside the member's window (``_bin_oracle.cells``); for rule 1 a pixel stays only
where ``_bin_oracle.mosaic`` elects its member (`source`, exact: integer sums); the members concatenated; then a literal
``np.median`` / ``np.quantile(values.astype(float64), qs)`` over the pixels of every non-empty cell, all planes of the cell in
one call along axis 0 (as ``_median_oracle.median_loop`` and ``_quantile_oracle.quantile_loop`` do), and the image through
``oracle.ref_numpy.finalize_image``.  count, mask and source are the mean mosaic's.  ``restated`` says the same through
``_quantile_oracle.quantile_bins`` / ``_median_oracle.median_bins`` on the concatenated, filtered pixels.
"""
import numpy as np

import _bin_oracle as B
import _median_oracle as M
import _quantile_oracle as Q


def member_flats(mosaic, rule, mean=None):
    """[output cell of every pixel, -1 where it does not count] per member, and the mean mosaic's oracle dict."""
    mean = B.mosaic(mosaic.members, mosaic.windows, rule) if mean is None else mean
    flats = [B.cells(c, w) for c, w in zip(mosaic.members, mosaic.windows)]
    if rule == 1:
        source = mean['source'].ravel()
        flats = [np.where(source[np.maximum(f, 0)] == k, f, -1) for k, f in enumerate(flats)]
    return flats, mean


def has_elev(mosaic):
    return all(c.elev is not None for c in mosaic.members)


def values(mosaic):
    """(n, nch [+ 1]) float64: the planes of the concatenated pixels (the elevation when every member has one)."""
    parts = []
    for c in mosaic.members:
        cols = [c.img.astype(np.float64)]
        if has_elev(mosaic):
            cols.append(np.asarray(c.elev, dtype=np.float64)[:, None])
        parts.append(np.concatenate(cols, axis=1))
    return np.concatenate(parts, axis=0)


def _finish(mosaic, stat, mean):
    """stat (k, ny * nx, planes) -> the expected outputs."""
    from oracle import ref_numpy as O
    ny, nx = mosaic.shape
    first = mosaic.members[0]
    nch = first.img.shape[1]
    k = stat.shape[0]
    stat = stat.reshape(k, ny, nx, -1)
    el = stat[..., nch:] if has_elev(mosaic) else np.full((k, ny, nx, 1), np.nan)
    stat = np.concatenate([stat[..., :nch], el], axis=3)
    img, _ = O.finalize_image(stat[..., :nch], first.img.dtype)
    return dict(stat=stat, img=img, mask=mean['mask'], count=mean['count_f'], source=mean['source'])


def expected(mosaic, rule, qs=None, mean=None):
    """dict(stat (k, ny, nx, nch + 1), img (k, ny, nx, nch), mask, count, source): the median (qs None, k = 1) or the quantiles
    qs (k = len(qs)) by a literal np.median / np.quantile per non-empty cell."""
    flats, mean = member_flats(mosaic, rule, mean)
    flat = np.concatenate(flats)
    v = values(mosaic)
    ny, nx = mosaic.shape
    k = 1 if qs is None else len(qs)
    out = np.full((k, nx * ny, v.shape[1]), np.nan)
    order = np.argsort(flat, kind='stable')
    f = flat[order]
    cells, start = np.unique(f, return_index=True)
    end = np.concatenate((start[1:], [len(f)]))
    for c, i0, i1 in zip(cells, start, end):
        if c < 0 or v.shape[1] == 0:
            continue
        mine = v[order[i0:i1]].astype(np.float64)
        out[:, c, :] = np.median(mine, axis=0)[None] if qs is None else np.quantile(mine, np.asarray(qs, dtype=np.float64), axis=0)
    count = np.bincount(flat[flat >= 0], minlength=nx * ny).reshape(ny, nx)
    assert np.array_equal(count, mean['count']), 'the filtered pixels are not the mean mosaic\'s'
    return _finish(mosaic, out, mean)


def restated(mosaic, rule, qs=None, mean=None):
    """The same through median_bins / quantile_bins (one lexsort per plane, NumPy's arithmetic restated)."""
    flats, mean = member_flats(mosaic, rule, mean)
    flat = np.concatenate(flats)
    first = mosaic.members[0]
    x = np.concatenate([np.ravel(c.lon_binned) for c in mosaic.members])
    y = np.concatenate([np.ravel(c.lat) for c in mosaic.members])
    assert np.array_equal(M.cell_index(x, y, first.xedges, first.yedges)[flat >= 0], flat[flat >= 0])
    v = values(mosaic)
    ny, nx = mosaic.shape
    if v.shape[1] == 0:
        stat = np.full((1 if qs is None else len(qs), ny * nx, 0), np.nan)
    elif qs is None:
        med, count = M.median_bins(x, y, v, first.xedges, first.yedges, keep=flat >= 0)
        # (np.median is np.mean of the middle pair, whose sum starts from +0.0: a pair of -0.0 gives +0.0; x + 0.0 is x otherwise)
        stat = med.reshape(1, ny * nx, -1) + 0.0
    else:
        quant, count = Q.quantile_bins(x, y, v, first.xedges, first.yedges, qs, keep=flat >= 0)
        stat = quant.reshape(len(qs), ny * nx, -1)
    return _finish(mosaic, stat, mean)
