"""
amt_gather_mosaic_supersampled on constructed cameras (tests/_gather_mosaic_cases.py), against an exact oracle: the existing
amt_gather_mosaic is called directly on the sub-sample points that gather_subsample_coordinates returns — a grid n times as fine
per axis — and its host results go through the NumPy reduction of tests/_gather_supersample_oracle.py.  `img`, `mask`, `source`,
`count` and the unmasked `elevation` of the fused kernel must agree with that bit for bit: no tolerance anywhere.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

import _gather_mosaic_cases as GC
import _gather_supersample_oracle as SO
from _gather_supersample_cases import agree, check, fine, mixed_cells, pair, pair_plan, plan_of, same_bits, wide_plan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6, 7, 8])
def test_every_factor(n):
    plan = wide_plan()
    g = plan['grid']
    assert g.ny > 32 // n and g.nx > 32 // n                               # more than one block either way
    res, points = check(plan, n, what='wide', debug=dict(tile_path=True))
    assert ((res['count'] > 0) & (res['count'] < n * n)).any()              # cells on the footprint's edge
    assert res['count'].max() == n * n and (res['source'][~res['mask']] == 0).all()
    # the remembered threshold bites at the sub-samples
    with np.errstate(invalid='ignore'):
        assert (points['elevation'][~points['mask']] >= 5.0).all() and (points['elevation'][~points['mask']] < 6.0).any()
    T = 32 // n
    assert res['tile_path'].shape == ((g.ny + T - 1) // T, (g.nx + T - 1) // T)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize('channels', [1, 3, 4])
def test_sample_types_channels_and_interpolations(dtype, channels):
    plan = wide_plan(dtype, channels)
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        for n in (3, 4):
            res, _ = check(plan, n, interpolation, what=(dtype, channels), debug=dict(tile_path=True))
            assert res['img'][~res['mask']].any() and not res['img'][res['mask']].any()
            if interpolation == 'nearest':
                assert not (res['tile_path'] == 1).any()                    # no window to stage


@pytest.mark.parametrize('magnetic', [False, True])
def test_two_cameras_both_rules(magnetic):
    """gm-a and gm-b: footprints that overlap in part, so that cells along the line where the higher camera changes hold
    sub-samples of both winners (the SM frame on the same pair)"""
    for n in (2, 4):
        by_rule = {}
        for mayOverlap in (True, False):
            plan = plan_of(pair(), mayOverlap, magnetic, pxPerDeg=10)
            assert plan['rule'] == int(mayOverlap)
            res, points = check(plan, n, 'linear', magnetic, what=('pair', mayOverlap), debug=dict(tile_path=True))
            by_rule[mayOverlap] = res
            assert (res['source'] == 0).any() and (res['source'] == 1).any()
            assert mixed_cells(points, n).any()                            # the majority, and the means over two images, are exercised
        assert not np.array_equal(by_rule[True]['source'], by_rule[False]['source'])
        assert np.array_equal(by_rule[True]['count'], by_rule[False]['count'])


def test_exact_copies_centre_mask_and_threshold():
    import torch
    cam = GC.by_name('gm-a')
    members = [GC.mapping(cam, GC.image(cam, seed=1), identifier='t0'),
               GC.mapping(cam, GC.image(cam, seed=2), lazy_elevation=10, identifier='t1'),
               GC.mapping(cam, GC.image(cam, seed=3), identifier='t2')]
    plan = plan_of(members, pxPerDeg=8)
    for n in (2, 3):
        res, _ = check(plan, n, what='copies')
        assert (res['source'][~res['mask']] == 0).all()                     # three copies tie exactly at every sub-sample
    # a rectangle of member 0's centre mask hands those sub-samples to member 1, and below member 1's threshold to member 2
    cm = torch.zeros((cam['height'], cam['width']), dtype=torch.uint8, device='cuda')
    cm[:, 12:52] = 1
    plan['members'][0]['center_mask'] = cm
    for n, interpolation in ((2, 'nearest'), (3, 'linear'), (4, 'lanczos4')):
        res, points = check(plan, n, interpolation, what='copies, masked', debug=dict(tile_path=True))
        assert set(np.unique(res['source']).tolist()) == {-1, 0, 1, 2}
        assert mixed_cells(points, n).any()


def test_date_line_and_a_grid_narrower_than_a_tile():
    a, b = GC.by_name('dateline'), GC.by_name('gm-dateline-b')
    members = [GC.mapping(a, GC.image(a, np.uint16, 3, seed=1)), GC.mapping(b, GC.image(b, np.uint16, 3, seed=2))]
    plan = plan_of(members, pxPerDeg=200)
    assert plan['contains_discontinuity'] and not plan['contains_pole'] and plan['grid'].nx < 32
    for n, interpolation in ((2, 'nearest'), (2, 'linear'), (5, 'linear')):
        res, _ = check(plan, n, interpolation, what='dateline')
        assert (res['source'] == 0).any() and (res['source'] == 1).any()


def test_pole_takes_the_point_form():
    a, b = GC.by_name('pole'), GC.by_name('gm-pole-b')
    members = [GC.mapping(a, GC.image(a, seed=1)), GC.mapping(b, GC.image(b, seed=2))]
    plan = plan_of(members, pxPerDeg=200)
    assert plan['contains_pole'] and all(m['center_mask'] is not None for m in plan['members'])
    for n, interpolation in ((2, 'nearest'), (3, 'linear')):
        res, _ = check(plan, n, interpolation, what='pole')
        assert (res['source'] == 0).any() and (res['source'] == 1).any()


def test_min_count_and_nested_masks():
    plan = pair_plan(np.uint16, 3, pxPerDeg=10)
    n = 3
    points = fine(plan, n)
    loose, _ = check(plan, n, minCoverage=1e-9, points=points, what='min_count 1')
    half, _ = check(plan, n, points=points, what='the default')
    full, _ = check(plan, n, minCoverage=1.0, points=points, what='every sub-sample')
    assert np.array_equal(loose['mask'], loose['count'] < 1) and np.array_equal(half['mask'], half['count'] < 5)
    assert np.array_equal(full['mask'], full['count'] < 9)
    assert (loose['mask'] <= half['mask']).all() and (half['mask'] <= full['mask']).all()
    assert loose['mask'].sum() < half['mask'].sum() < full['mask'].sum()
    for r in (half, full):
        assert np.array_equal(r['count'], loose['count'])                   # the real count, also of the cells that are masked
        keep = ~r['mask']
        assert same_bits(r['img'][keep], loose['img'][keep]) and same_bits(r['elevation'][keep], loose['elevation'][keep])


def test_factor_one_is_the_gather_mosaic():
    from auromat_amd import resample as R
    plan = pair_plan(np.float32, 4, pxPerDeg=10)
    images = [m['image'] for m in plan['members']]
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        res = R._gather_mosaic_call(plan, plan['members'], images, interpolation, False, plan['rule'], 1, 1, dict(tile_path=True),
                                    supersampled=True)
        one = fine(plan, 1, interpolation)
        for k in ('img', 'mask', 'source'):
            assert same_bits(res[k], one[k]), (interpolation, k)
        assert np.array_equal(res['elevation'], one['elevation'], equal_nan=True)
        assert same_bits(np.nan_to_num(res['elevation'], nan=0.0), np.nan_to_num(one['elevation'], nan=0.0))
        assert np.array_equal(res['count'], (~res['mask']).astype(np.uint8))
        assert res['tile_path'].shape == ((plan['grid'].ny + 31) // 32, (plan['grid'].nx + 31) // 32)


@pytest.mark.parametrize('dtype,value', [(np.uint8, 200), (np.float32, 123.25)])
def test_a_constant_image_stays_the_constant(dtype, value):
    from auromat_amd.resample import gather_mosaic_frames
    plan = plan_of(pair(), pxPerDeg=10)
    images = [np.full(m['image'].shape, value, dtype=dtype) for m in plan['members']]
    # (nearest and linear: every tap with a weight lies inside the frame by the support rule, and the weights sum to 1 up to a
    # rounding far below the sample's; Lanczos-4 does not keep a constant near the frame's edge, where taps outside count 0)
    for n, interpolation in ((2, 'nearest'), (3, 'linear'), (8, 'linear'), (5, 'nearest')):
        res = gather_mosaic_frames(plan, images, interpolation, supersample=n, minCoverage=1e-9)
        assert (~res['mask']).sum() > 100 and ((res['count'] > 0) & (res['count'] < n * n)).any()
        assert (res['img'][~res['mask']] == dtype(value)).all() and not res['img'][res['mask']].any(), (n, interpolation)


def test_auto_and_forced_per_cell_path():
    from auromat_amd.resample import GATHER_PATH_CELL, gather_mosaic_frames
    plan = pair_plan(np.uint16, 3, pxPerDeg=10)
    g = plan['grid']
    for n, interpolation in ((2, 'linear'), (3, 'lanczos4'), (8, 'linear')):
        T = 32 // n
        auto, points = check(plan, n, interpolation, what='auto', debug=dict(tile_path=True))
        cell = gather_mosaic_frames(plan, None, interpolation, supersample=n, debug=dict(force_path=GATHER_PATH_CELL, tile_path=True))
        tiles = auto['tile_path']
        assert tiles.shape == cell['tile_path'].shape == ((g.ny + T - 1) // T, (g.nx + T - 1) // T)
        assert not (cell['tile_path'] == 1).any() and np.array_equal(cell['tile_path'] == 0, tiles == 0)
        for k in ('img', 'mask', 'source', 'count'):
            assert same_bits(auto[k], cell[k]), (n, interpolation, k)
        assert np.array_equal(auto['elevation'], cell['elevation'], equal_nan=True)
        s = np.where(points['mask'], -1, points['source'])
        for i in range(tiles.shape[0]):
            for j in range(tiles.shape[1]):
                won = set(np.unique(s[T * n * i:T * n * (i + 1), T * n * j:T * n * (j + 1)]).tolist()) - {-1}
                assert (tiles[i, j] == 0) == (not won), (n, i, j)
                assert tiles[i, j] != 1 or len(won) == 1, (n, i, j)
                assert len(won) < 2 or tiles[i, j] == 2, (n, i, j)
        # nobody (a tile outside every footprint), staged (one winner), per cell (mixed winners)
        assert set(np.unique(tiles).tolist()) == {0, 1, 2}, (n, interpolation)


def _table(ctx, plan, keep):
    from auromat_amd._native import GatherMember, ptr
    t = (GatherMember * len(plan['members']))()
    for e, m in zip(t, plan['members']):
        C.memmove(C.byref(e.params), C.byref(m['params']), C.sizeof(m['params']))
        img = ctx.to_device(m['image'], dtype=np.uint8)
        keep.append(img)
        e.img, e.min_elevation = ptr(img).value, float('nan')
    return t


def test_argument_errors_write_nothing():
    import torch
    from auromat_amd._native import Context, GatherDebug, ptr
    from auromat_amd.resample import gather_subsample_coordinates
    plan = plan_of(pair(), pxPerDeg=4)
    ctx = Context.current()
    ny, nx, n = plan['grid'].ny, plan['grid'].nx, 3
    sub = gather_subsample_coordinates(plan, n)
    keep = []
    lat, lon = ctx.to_device(sub['lat']), ctx.to_device(sub['lon'])
    cells = (ctx.to_device(np.ascontiguousarray(np.repeat(sub['lat'][:, None], nx * n, 1))),
             ctx.to_device(np.ascontiguousarray(np.repeat(sub['lon'][None, :], ny * n, 0))))
    outs = dict(img=torch.full((ny, nx, 3), 0x5A, dtype=torch.uint8, device=ctx.device),
                mask=torch.full((ny, nx), 0x5A, dtype=torch.uint8, device=ctx.device),
                elev=torch.full((ny, nx), 1234.5, dtype=torch.float64, device=ctx.device),
                source=torch.full((ny, nx), 77, dtype=torch.int32, device=ctx.device),
                count=torch.full((ny, nx), 0x5A, dtype=torch.uint8, device=ctx.device))

    def call(**kw):
        a = dict(members=_table(ctx, plan, keep), n=2, frame=0, lat=ptr(lat), ny=ny, lon=ptr(lon), nx=nx, cell_lat=None, cell_lon=None,
                 factor=n, min_count=5, bytes=1, channels=3, interpolation=0, rule=1, img=ptr(outs['img']), mask=ptr(outs['mask']),
                 elev=ptr(outs['elev']), source=ptr(outs['source']), count=ptr(outs['count']), debug=None)
        a.update(kw)
        rc = ctx._lib.amt_gather_mosaic_supersampled(ctx.handle, a['members'], a['n'], a['frame'], a['lat'], a['ny'], a['lon'], a['nx'],
                                                     a['cell_lat'], a['cell_lon'], a['factor'], a['min_count'], a['bytes'], a['channels'],
                                                     a['interpolation'], a['rule'], a['img'], a['mask'], a['elev'], a['source'],
                                                     a['count'], a['debug'])
        return rc, (ctx._lib.amt_last_error(ctx.handle) or b'').decode()

    singular, no_image = _table(ctx, plan, keep), _table(ctx, plan, keep)
    singular[1].params.cd[:] = [0.0, 0.0, 0.0, 0.0]
    no_image[0].img = None
    bad_force = GatherDebug()
    bad_force.force_path = 5
    cases = [dict(factor=0), dict(factor=9), dict(factor=-2), dict(min_count=0), dict(min_count=n * n + 1), dict(factor=1, min_count=2),
             dict(count=None),
             # a sample of what amt_gather_mosaic refuses
             dict(members=None), dict(img=None), dict(mask=None), dict(elev=None), dict(source=None), dict(n=0), dict(ny=0), dict(nx=-1),
             dict(cell_lat=ptr(cells[0]), cell_lon=ptr(cells[1])), dict(lat=None, lon=None), dict(lat=None), dict(frame=2),
             dict(interpolation=3), dict(rule=2), dict(bytes=3), dict(channels=2), dict(debug=C.byref(bad_force))]
    for kw in cases:
        rc, err = call(**kw)
        assert rc == -1 and 'amt_gather_mosaic_supersampled' in err, (kw, err)      # AMT_EINVAL
    for members, word in ((singular, 'member 1: singular'), (no_image, 'member 0: member without image')):
        rc, err = call(members=members)
        assert rc == -1 and word in err, (word, err)
    ctx.synchronize()
    assert (outs['img'] == 0x5A).all() and (outs['mask'] == 0x5A).all() and (outs['source'] == 77).all()
    assert (outs['elev'] == 1234.5).all() and (outs['count'] == 0x5A).all()
    # and the same arguments unchanged are accepted, in either coordinate form, with the same result
    rc, err = call()
    assert rc == 0, err
    ctx.synchronize()
    first = {k: v.clone() for k, v in outs.items()}
    assert (first['source'] >= 0).any() and (first['source'] < 0).any() and int(first['count'].max()) == n * n
    rc, err = call(lat=None, lon=None, cell_lat=ptr(cells[0]), cell_lon=ptr(cells[1]))
    assert rc == 0, err
    ctx.synchronize()
    for k in ('img', 'mask', 'source', 'count'):
        assert torch.equal(first[k], outs[k]), k
    assert torch.equal(torch.nan_to_num(first['elev'], nan=-1.0), torch.nan_to_num(outs['elev'], nan=-1.0))
    del keep


def test_behind_a_gated_side_stream():
    """The images and the sub-sample axes are written behind the gate.  No input of this call is used as an index: the axes
    decide which taps are read, and every tap is tested against the image's frame by the kernel itself (the support rule, the
    window's zero fill, the per-tap test of the global fetch); the member table holds pointers and sizes from the host, the same
    for the true arrays and the decoys.  So the decoys — other images, axes shifted by a fraction of a degree — are harmless."""
    import _gated_stream as GS
    from auromat_amd._native import GatherMember
    from auromat_amd.resample import gather_subsample_coordinates
    plan = pair_plan(np.uint16, 3, pxPerDeg=6)
    ny, nx, n = plan['grid'].ny, plan['grid'].nx, 3
    sub = gather_subsample_coordinates(plan, n)
    a, b = GC.by_name('gm-a'), GC.by_name('gm-b')
    inputs = OrderedDict(img_a=(plan['members'][0]['image'], GC.image(a, np.uint16, 3, seed=11)),
                         img_b=(plan['members'][1]['image'], GC.image(b, np.uint16, 3, seed=12)),
                         lat=(sub['lat'], sub['lat'] + 0.37), lon=(sub['lon'], sub['lon'] - 0.61))
    outputs = OrderedDict([('img', ((ny, nx, 3), np.uint16)), ('mask', ((ny, nx), np.uint8)), ('elev', ((ny, nx), np.float64)),
                           ('source', ((ny, nx), np.int32)), ('count', ((ny, nx), np.uint8))])

    def call(env):
        i, o = env.inp, env.out
        t = (GatherMember * 2)()
        for e, m, img in zip(t, plan['members'], (i['img_a'], i['img_b'])):
            C.memmove(C.byref(e.params), C.byref(m['params']), C.sizeof(m['params']))
            e.img, e.min_elevation = img.data_ptr(), float('nan')
        env.ctx.call('amt_gather_mosaic_supersampled', t, 2, 0, i['lat'].data_ptr(), ny, i['lon'].data_ptr(), nx, None, None, n, 5, 2, 3,
                     0, 1, o['img'].data_ptr(), o['mask'].data_ptr(), o['elev'].data_ptr(), o['source'].data_ptr(),
                     o['count'].data_ptr(), None)
        env.closed('amt_gather_mosaic_supersampled')

    case = GS.Case('gather_mosaic_supersampled', 'B', inputs, outputs, call,
                   harmless='no input is used as an index: coordinates select taps that the kernel tests against the frame')
    want, _, _ = GS.baseline(case)
    # the baseline is what the oracle says, so the gated run is compared with the right bytes
    res = dict(img=want['img'].view(np.uint16).reshape(ny, nx, 3), mask=want['mask'].reshape(ny, nx).astype(bool),
               elevation=want['elev'].view(np.float64).reshape(ny, nx), source=want['source'].view(np.int32).reshape(ny, nx),
               count=want['count'].reshape(ny, nx))
    agree(res, SO.reduce_cells(fine(plan, n), n, 5), 'gated baseline')
    GS.run_gated(case)
