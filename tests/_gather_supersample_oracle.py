"""
TEST INFRASTRUCTURE — the oracle of supersampled gathering (amt_gather_mosaic_supersampled, include/auromat_hip.h).

Two independent restatements in NumPy: where the n x n sub-samples of a cell lie (`sub_axis`), and how the results at the
sub-sample points — what amt_gather_mosaic gives on the (ny n, nx n) fine grid — reduce to cells (`reduce_cells`).  The sums that
the contract orders are written as sequential float64 sums over (s, t), s outer, t inner; the first seen value starts a sum.
"""
import numpy as np


def sub_axis(corners, n):
    """sub-sample s of cell i of an axis with the corners c: c[i] + (c[i + 1] - c[i]) * ((2 s + 1) / (2 n)), cell by cell"""
    c = np.asarray(corners, dtype=np.float64)
    out = np.empty((c.size - 1) * n, dtype=np.float64)
    for i in range(c.size - 1):
        for s in range(n):
            out[i * n + s] = c[i] + (c[i + 1] - c[i]) * np.float64((2 * s + 1) / (2 * n))
    return out


def _ordered_mean(values, seen, n, count):
    """per cell: the float64 sum of values[i n + s, j n + t] over the seen (s, t) in row-major order, divided by count"""
    ny, nx = count.shape
    acc = np.zeros((ny, nx), dtype=np.float64)
    started = np.zeros((ny, nx), dtype=bool)
    with np.errstate(invalid='ignore'):
        for s in range(n):
            for t in range(n):
                v = values[s::n, t::n].astype(np.float64)
                sn = seen[s::n, t::n]
                acc = np.where(sn, np.where(started, acc + v, v), acc)
                started |= sn
        return acc / count.astype(np.float64)


def reduce_cells(fine, n, min_count):
    """
    fine: dict(img (ny n, nx n, C), mask (ny n, nx n) bool, elevation (ny n, nx n) float64, source (ny n, nx n) int32) on the
    sub-sample points.  Returns dict(img, mask, elevation, source, count) on the (ny, nx) cells by the contract.
    """
    img, seen = np.asarray(fine['img']), ~np.asarray(fine['mask'], dtype=bool)
    elev, src = np.asarray(fine['elevation'], dtype=np.float64), np.asarray(fine['source'])
    assert 1 <= min_count <= n * n and img.shape[0] % n == 0 and img.shape[1] % n == 0
    ny, nx, C = img.shape[0] // n, img.shape[1] // n, img.shape[2]
    count = np.zeros((ny, nx), dtype=np.int64)
    for s in range(n):
        for t in range(n):
            count += seen[s::n, t::n]
    valid = count >= min_count
    out = np.zeros((ny, nx, C), dtype=img.dtype)
    for c in range(C):
        if img.dtype == np.float32:
            mean = _ordered_mean(img[:, :, c], seen, n, count).astype(np.float32)
        else:
            total = np.zeros((ny, nx), dtype=np.int64)
            for s in range(n):
                for t in range(n):
                    total += np.where(seen[s::n, t::n], img[s::n, t::n, c].astype(np.int64), 0)
            with np.errstate(invalid='ignore', divide='ignore'):
                mean = np.rint(total.astype(np.float64) / count.astype(np.float64))          # (half to even)
            mean = np.where(valid, mean, 0.0).astype(img.dtype)
        out[:, :, c] = np.where(valid, mean, np.zeros((), dtype=img.dtype))
    elevation = np.where(valid, _ordered_mean(elev, seen, n, count), np.nan)
    # the member that won the most sub-samples, the lower index on a tie
    source = np.full((ny, nx), -1, dtype=np.int32)
    most = np.zeros((ny, nx), dtype=np.int64)
    for m in sorted(set(np.unique(src[seen]).tolist())):
        won = np.zeros((ny, nx), dtype=np.int64)
        for s in range(n):
            for t in range(n):
                won += seen[s::n, t::n] & (src[s::n, t::n] == m)
        better = won > most
        source[better], most[better] = m, won[better]
    source[~valid] = -1
    return dict(img=out, mask=~valid, elevation=elevation, source=source, count=count.astype(np.uint8))
