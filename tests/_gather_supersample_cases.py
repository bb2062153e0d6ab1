"""
TEST INFRASTRUCTURE — plans, the exact oracle's device half and the comparison for supersampled gathering
(amt_gather_mosaic_supersampled; tests/test_gpu_gather_supersample_cells.py, tests/test_gpu_gather_supersample.py).

`fine` calls the existing amt_gather_mosaic directly on the sub-sample points that gather_subsample_coordinates returns; the NumPy
reduction of tests/_gather_supersample_oracle.py turns its host results into what the fused kernel has to give, bit for bit.
"""
import numpy as np

import _gather_mosaic_cases as GC
import _gather_supersample_oracle as SO

CODES = dict(linear=0, lanczos4=1, nearest=2)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def plan_of(members, mayOverlap=True, magnetic=False, **kw):
    from auromat_amd.resample import gather_mosaic_plan
    return gather_mosaic_plan(GC.collection(members, mayOverlap), magnetic=magnetic, **kw)


def pair(dtype=np.uint8, channels=3, **kw):
    a, b = GC.by_name('gm-a'), GC.by_name('gm-b')
    return [GC.mapping(a, GC.image(a, dtype, channels, seed=1), **kw), GC.mapping(b, GC.image(b, dtype, channels, seed=2), **kw)]


def pair_plan(dtype=np.uint8, channels=3, mayOverlap=True, magnetic=False, **kw):
    """gm-a and gm-b on one grid, laid out with uint8 RGB images and handed the images under test"""
    plan = plan_of(pair(), mayOverlap, magnetic, **kw)
    for m, name, seed in zip(plan['members'], ('gm-a', 'gm-b'), (1, 2)):
        m['image'] = GC.image(GC.by_name(name), dtype, channels, seed=seed)
    return plan


def wide_plan(dtype=np.uint8, channels=3, pxPerDeg=8):
    cam = GC.by_name('gm-wide')
    # (the mapping only remembers its threshold with the image kinds the fused frame kernel takes: the plan is laid out with
    # such an image and handed the one under test)
    plan = plan_of([GC.mapping(cam, lazy_elevation=5)], pxPerDeg=pxPerDeg)
    plan['members'][0]['image'] = GC.image(cam, dtype, channels)
    assert plan['members'][0]['min_elevation'] == 5.0
    return plan


def fine(plan, n, interpolation='linear', magnetic=False):
    """amt_gather_mosaic itself on the n x n sub-sample points of every cell: host results on the (ny n, nx n) points"""
    import torch
    from auromat_amd import resample as R
    from auromat_amd._native import Context, ptr, to_host
    ctx = Context.current()
    members = plan['members']
    table, keep, nch, tdtype, np_dtype = R._gather_member_table(ctx, members, [m['image'] for m in members])
    sub = R.gather_subsample_coordinates(plan, n)
    d = {k: None if v is None else ctx.to_device(np.ascontiguousarray(v)) for k, v in sub.items()}
    ny, nx = plan['grid'].ny * n, plan['grid'].nx * n
    if plan['contains_pole']:
        assert sub['lat'] is None and sub['cell_lat'].shape == (ny, nx) and sub['cell_lon'].shape == (ny, nx)
    else:
        assert sub['cell_lat'] is None and sub['lat'].shape == (ny,) and sub['lon'].shape == (nx,)
    img = torch.empty((ny, nx, nch), dtype=tdtype, device=ctx.device)
    mask, elev, source = ctx.empty((ny, nx), torch.uint8), ctx.empty((ny, nx)), ctx.empty((ny, nx), torch.int32)
    ctx.call('amt_gather_mosaic', table, len(members), 1 if magnetic else 0, ptr(d['lat']), ny, ptr(d['lon']), nx, ptr(d['cell_lat']),
             ptr(d['cell_lon']), img.element_size(), nch, CODES[interpolation], int(plan['rule']), ptr(img), ptr(mask), ptr(elev),
             ptr(source), None, None)
    out = dict(img=to_host(img, dtype=np_dtype), mask=to_host(mask).astype(bool), elevation=to_host(elev),
               source=to_host(source, dtype=np.int32))
    del keep, d
    return out


def agree(res, want, what):
    assert np.array_equal(res['count'], want['count']) and res['count'].dtype == np.uint8, what
    assert np.array_equal(res['mask'], want['mask']), what
    assert np.array_equal(res['source'], want['source']) and res['source'].dtype == np.int32, what
    assert same_bits(res['img'], want['img']), what
    assert np.isnan(res['elevation'][want['mask']]).all(), what
    assert same_bits(np.where(want['mask'], 0.0, res['elevation']), np.where(want['mask'], 0.0, want['elevation'])), what


def check(plan, n, interpolation='linear', magnetic=False, minCoverage=None, what=None, points=None, **kw):
    from auromat_amd.resample import gather_mosaic_frames, supersample_min_count
    res = gather_mosaic_frames(plan, None, interpolation, magnetic, supersample=n, minCoverage=minCoverage, **kw)
    points = fine(plan, n, interpolation, magnetic) if points is None else points
    want = SO.reduce_cells(points, n, supersample_min_count(minCoverage, n))
    what = (what, n, interpolation, magnetic, minCoverage)
    agree(res, want, what)
    g = plan['grid']
    assert res['img'].shape == (g.ny, g.nx, points['img'].shape[2]) and res['img'].dtype == points['img'].dtype, what
    assert 0 < res['mask'].sum() < res['mask'].size, what
    assert 'xy' not in res and 'flags' not in res
    return res, points


def mixed_cells(points, n):
    """cells whose seen sub-samples have more than one winner"""
    s, seen = points['source'], ~points['mask']
    big = np.iinfo(np.int32).max
    lo = np.stack([np.where(seen, s, big)[a::n, b::n] for a in range(n) for b in range(n)]).min(0)
    hi = np.stack([np.where(seen, s, -1)[a::n, b::n] for a in range(n) for b in range(n)]).max(0)
    return (hi >= 0) & (lo != hi)
