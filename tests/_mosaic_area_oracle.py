"""
The contract of the area-weighted mosaic (``amt_area_mosaic_frames``, auromat_amd/csrc/amt_area.hip;
``resampleMosaic(statistic='area')``) in NumPy.  A plain helper module for tests/test_mosaic_area_cpu.py,
tests/test_gpu_mosaic_area_cells.py and tests/test_gpu_mosaic_area.py.

Per member: the integer accumulators of ``_area_oracle.accumulate`` on the common edges, cropped to the member's window (zero
outside it).  Then the overlap rule with ``_area_oracle.finalize``'s arithmetic, and the overflow flag.
"""
import numpy as np

import _area_oracle as O


def member_accumulators(case, window):
    """int64 (nch + 2, nx, ny): ``accumulate(case)`` on the whole common grid inside `window` (x0, y0, nx, ny), zero outside."""
    acc, _ = O.accumulate(case)
    x0, y0, wnx, wny = window
    out = np.zeros_like(acc)
    if wnx and wny:
        out[:, x0:x0 + wnx, y0:y0 + wny] = acc[:, x0:x0 + wnx, y0:y0 + wny]
    return out


def elect(accs, rule, dtype, least):
    """The two rules on the members' accumulators (a sequence of (nch + 2, nx, ny) int64, zero outside each window), `least`
    the minimum weight itself.  dict(area (ny, nx, nch + 1), img (ny, nx, nch), mask uint8, coverage, source int32 (all in the
    output layout, rows north to south), over: the call returns AMT_EDOMAIN)."""
    accs = np.asarray(accs, dtype=np.int64)
    least = max(1, int(least))
    lay = lambda p: np.flipud(p.T)
    w = np.array([lay(a[0]) for a in accs])                           # (m, ny, nx)
    over = bool((w > O.LIMIT).any())
    if rule == 0:
        total = accs.sum(axis=0)
        out = O.finalize(total, dtype, least=least)
        over = over or out['over']
        present = w > 0
        first = np.where(present.any(0), np.argmax(present, axis=0), -1)
        out['source'] = np.where(out['mask'] == 0, first, -1).astype(np.int32)
        out['over'] = over
        return out
    fins = [O.finalize(a, dtype, least=least) for a in accs]
    cand = w >= least
    with np.errstate(divide='ignore', invalid='ignore'):
        el = np.array([lay(a[-1]).astype(np.float64) for a in accs]) / w.astype(np.float64)
    el = np.where(cand, el, -np.inf)
    source = np.where(cand.any(0), np.argmax(el, axis=0), -1)         # argmax: the first of equal maxima
    pick = np.clip(source, 0, None)
    take = lambda key: np.take_along_axis(np.array([f[key] for f in fins]),
                                          pick.reshape((1,) + pick.shape + (1,) * (fins[0][key].ndim - 2)), 0)[0]
    none = source < 0
    area, img, mask, coverage = take('area'), take('img'), take('mask'), take('coverage')
    area = np.where(none[..., None], np.nan, area)
    img = np.where(none[..., None], 0, img).astype(fins[0]['img'].dtype)
    mask = np.where(none, 1, mask).astype(np.uint8)
    coverage = np.where(none, w.max(axis=0).astype(np.float64) / O.ONE, coverage)
    return dict(area=area, img=img, mask=mask, coverage=coverage, source=source.astype(np.int32), over=over)


def mosaic(members, windows, rule, min_coverage=0.5, least=None):
    """The mosaic of `members` (``_area_cases.AreaCase``-like objects on ONE pair of edges, one image dtype and channel count)
    with their `windows`; see :func:`elect`."""
    least = O.min_weight(min_coverage) if least is None else least
    accs = [member_accumulators(m, win) for m, win in zip(members, windows)]
    return elect(accs, rule, members[0].img.dtype, least)
