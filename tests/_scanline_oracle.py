"""
NumPy restatements of the scan-line kernels' contracts (include/auromat_hip.h: amt_scanline_select, amt_scanline_pack,
amt_scanline_compose), for tests/test_scanline_cpu.py, tests/test_gpu_scanline_cells.py and tests/test_gpu_scanlines.py.
The point test is matplotlib's, which the reference's pointsInsidePolygon calls (utils.py:58-74).
"""
import numpy as np

INT64_MAX, INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def corners_inside(lat_axis, lon_axis, polygon):
    """(ny + 1, nx + 1) bool: Path(polygon).contains_points of every corner (lat_axis[i], lon_axis[j]), x = latitude"""
    import matplotlib.path
    la, lo = np.meshgrid(np.asarray(lat_axis, dtype=np.float64), np.asarray(lon_axis, dtype=np.float64), indexing='ij')
    polygon = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    if len(polygon) < 3:
        return np.zeros(la.shape, dtype=bool)
    pts = np.column_stack((la.ravel(), lo.ravel()))
    return matplotlib.path.Path(polygon).contains_points(pts).reshape(la.shape)


def four_corner_rule(inside, mask):
    """(ny, nx) bool: the cell is unmasked and its four corners are inside (BaseMapping.maskedByPolygon)"""
    return inside[:-1, :-1] & inside[1:, :-1] & inside[:-1, 1:] & inside[1:, 1:] & (np.asarray(mask) == 0)


def stats_of(kept):
    """int64 (5) of a whole-frame keep array: count, min row, max row, min col, max col (identities when nothing is kept)"""
    rows, cols = np.nonzero(kept)
    if rows.size == 0:
        return np.array([0, INT64_MAX, INT64_MIN, INT64_MAX, INT64_MIN], dtype=np.int64)
    return np.array([rows.size, rows.min(), rows.max(), cols.min(), cols.max()], dtype=np.int64)


def select(lat_axis, lon_axis, polygon, mask, window, inside=None):
    """(keep (rows, cols) uint8, stats int64 (5)) of amt_scanline_select; `inside`: the corner test's result when the caller
    has one already (the case against amt_points_in_polygon)"""
    row0, col0, rows, cols = window
    inside = corners_inside(lat_axis, lon_axis, polygon) if inside is None else inside
    kept = np.zeros(np.asarray(mask).shape, dtype=bool)
    win = (slice(row0, row0 + rows), slice(col0, col0 + cols))
    kept[win] = four_corner_rule(inside, mask)[win]
    return kept[win].astype(np.uint8), stats_of(kept)


def pack(keep, window, planes, img, row_offset=0, col_offset=0):
    """The records of amt_scanline_pack sorted by (row, col): dict(row, col int32 (n), planes (P, n), img (C, n))"""
    row0, col0, rows, cols = window
    r, c = np.nonzero(np.asarray(keep).reshape(rows, cols))            # (row-major: sorted by (row, col))
    r, c = r + row0, c + col0
    return dict(row=(r + row_offset).astype(np.int32), col=(c + col_offset).astype(np.int32),
                planes=np.ascontiguousarray(np.moveaxis(planes[r, c], -1, 0)), img=np.ascontiguousarray(np.moveaxis(img[r, c], -1, 0)))


def sort_records(rec):
    """records in any order -> sorted by (row, col)"""
    order = np.lexsort((rec['col'], rec['row']))
    return dict(row=rec['row'][order], col=rec['col'][order], planes=rec['planes'][:, order], img=rec['img'][:, order])


def compose(strips, frames, row_base, col_base, NY, NX, nplane, nchan, img_dtype=np.uint8):
    """amt_scanline_compose: (planes (NY, NX, nplane), img (NY, NX, nchan), mask (NY, NX) uint8, frameIndex (NY, NX) int32,
    outside: a record lay outside the raster).  The largest frame index wins a cell, whatever the order of `strips`."""
    planes = np.full((NY, NX, nplane), np.nan)
    img = np.zeros((NY, NX, nchan), dtype=img_dtype)
    mask = np.ones((NY, NX), dtype=np.uint8)
    index = np.full((NY, NX), -1, dtype=np.int32)
    outside = False
    for s, k in sorted(zip(strips, frames), key=lambda sk: sk[1]):      # ascending: later strips paint over earlier ones
        y, x = s['row'].astype(np.int64) - row_base, s['col'].astype(np.int64) - col_base
        ok = (y >= 0) & (y < NY) & (x >= 0) & (x < NX)
        outside |= bool((~ok).any())
        y, x = y[ok], x[ok]
        planes[y, x] = s['planes'][:nplane, ok].T
        img[y, x] = s['img'][:nchan, ok].T
        mask[y, x] = 0
        index[y, x] = k
    return planes, img, mask, index, outside
