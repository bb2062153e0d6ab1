"""
TEST INFRASTRUCTURE — the NumPy statement of the gather mosaic's election (include/auromat_hip.h, amt_gather_mosaic).

`elect`: per-member (seen, elevation) arrays -> the winning member's index per cell.  rule 1: of the members that see the cell the
one with the highest elevation, the lower index on a tie; rule 0: the lowest index that sees it.  A NaN elevation never wins;
nobody: -1.
`compose`: the mosaic from the members' own gather_frame results on the mosaic's grid — the winner's sample and elevation, image 0
and elevation NaN where nobody sees the cell.
"""
import numpy as np


def elect(seen, elev, rule):
    seen, elev = np.asarray(seen, dtype=bool), np.asarray(elev, dtype=np.float64)
    assert seen.shape == elev.shape and rule in (0, 1)
    cand = seen & ~np.isnan(elev)
    source = np.full(seen.shape[1:], -1, dtype=np.int32)
    best = np.full(seen.shape[1:], -np.inf)
    for m in range(seen.shape[0]):
        with np.errstate(invalid='ignore'):
            take = cand[m] & (source < 0) if rule == 0 else cand[m] & ((source < 0) | (elev[m] > best))
        source[take] = m
        best[take] = elev[m][take]
    return source


def compose(results, rule):
    """results: one dict(img, mask, elevation) per member, all on one grid -> dict(img, mask, elevation, source)"""
    source = elect(np.stack([~np.asarray(r['mask'], dtype=bool) for r in results]), np.stack([r['elevation'] for r in results]), rule)
    img = np.zeros_like(results[0]['img'])
    elevation = np.full(source.shape, np.nan)
    for m, r in enumerate(results):
        won = source == m
        img[won] = r['img'][won]
        elevation[won] = r['elevation'][won]
    return dict(img=img, mask=source < 0, elevation=elevation, source=source)
