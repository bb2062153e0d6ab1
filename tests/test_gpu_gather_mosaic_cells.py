"""
amt_gather_mosaic on constructed cameras (tests/_gather_mosaic_cases.py), against an exact oracle: every member goes through the
existing gather_frame (amt_grid_to_pixel / amt_world_to_pixel + amt_remap_coords + the masks) on a plan whose grid is the mosaic's,
and the NumPy election of tests/_gather_mosaic_oracle.py composes those results.  `source`, `mask`, `elevation` and `img` of the
fused kernel must agree with that bit for bit: no tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

import _gather_mosaic_cases as GC
import _gather_mosaic_oracle as GO

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def member_plan(plan, i):
    """the gather_plan of member i alone on the mosaic's grid"""
    m = plan['members'][i]
    return dict(grid=plan['grid'], contains_pole=plan['contains_pole'], contains_discontinuity=plan['contains_discontinuity'],
                altitude=plan['altitude'], params=m['params'], zenithal=m['zenithal'], min_elevation=m['min_elevation'],
                center_mask=m['center_mask'])


def member_results(plan, interpolation, magnetic):
    from auromat_amd.resample import gather_frame
    return [gather_frame(member_plan(plan, i), m['image'], interpolation, magnetic) for i, m in enumerate(plan['members'])]


def agree(res, want, what):
    assert np.array_equal(res['source'], want['source']) and res['source'].dtype == np.int32, what
    assert np.array_equal(res['mask'], want['mask']), what
    assert same_bits(res['img'], want['img']), what
    assert np.isnan(res['elevation'][want['mask']]).all(), what
    assert same_bits(np.where(want['mask'], 0.0, res['elevation']), np.where(want['mask'], 0.0, want['elevation'])), what


def check(plan, interpolation='linear', magnetic=False, winners=(0,), what=None, **kw):
    from auromat_amd.resample import gather_mosaic_frames
    res = gather_mosaic_frames(plan, None, interpolation, magnetic, **kw)
    members = member_results(plan, interpolation, magnetic)
    want = GO.compose(members, plan['rule'])
    what = (what, interpolation, magnetic)
    agree(res, want, what)
    assert res['img'].shape[:2] == (plan['grid'].ny, plan['grid'].nx) and res['img'].dtype == members[0]['img'].dtype, what
    assert 0 < res['mask'].sum() < res['mask'].size, what
    for w in winners:
        assert (res['source'] == w).sum() > 0, (what, 'member %d wins nothing' % w)
    return res, members


def plan_of(members, mayOverlap=True, magnetic=False, **kw):
    from auromat_amd.resample import gather_mosaic_plan
    return gather_mosaic_plan(GC.collection(members, mayOverlap), magnetic=magnetic, **kw)


def pair(dtype=np.uint8, channels=3, **kw):
    a, b = GC.by_name('gm-a'), GC.by_name('gm-b')
    return [GC.mapping(a, GC.image(a, dtype, channels, seed=1), **kw), GC.mapping(b, GC.image(b, dtype, channels, seed=2), **kw)]


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize('channels', [1, 3, 4])
def test_one_member_is_gather_frame(dtype, channels):
    cam = GC.by_name('gm-wide')
    # (the mapping only remembers its threshold with the image kinds the fused frame kernel takes: the plan is laid out with
    # such an image and handed the one under test)
    plan = plan_of([GC.mapping(cam, lazy_elevation=5)], pxPerDeg=10)
    plan['members'][0]['image'] = GC.image(cam, dtype, channels)
    assert plan['members'][0]['min_elevation'] == 5.0 and plan['members'][0]['center_mask'] is None
    assert plan['grid'].ny > 32 and plan['grid'].nx > 32
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        res, (one,) = check(plan, interpolation, what=(dtype, channels))
        # the mosaic of one member is that member's gather_frame: mask, elevation and every unmasked sample
        assert np.array_equal(res['mask'], one['mask'])
        keep = ~one['mask']
        assert same_bits(res['img'][keep], one['img'][keep]) and same_bits(res['elevation'][keep], one['elevation'][keep])
        assert not res['img'][one['mask']].any()
        with np.errstate(invalid='ignore'):
            assert (one['mask'] & (one['flags'] == 0) & (one['elevation'] < 5.0)).any()        # the remembered threshold bites


def test_exact_ties_centre_mask_and_remembered_threshold():
    import torch
    cam = GC.by_name('gm-a')
    members = [GC.mapping(cam, GC.image(cam, seed=1), identifier='t0'),
               GC.mapping(cam, GC.image(cam, seed=2), lazy_elevation=10, identifier='t1'),
               GC.mapping(cam, GC.image(cam, seed=3), identifier='t2')]
    plan = plan_of(members, pxPerDeg=10)
    assert [m['min_elevation'] for m in plan['members']] == [None, 10.0, None]
    for interpolation in ('nearest', 'linear'):
        res, _ = check(plan, interpolation, what='ties')
        assert (res['source'][~res['mask']] == 0).all()                 # three copies tie exactly: the lowest index
    # a rectangle of member 0's centre mask hands those cells to member 1, and below member 1's threshold to member 2
    cm = torch.zeros((cam['height'], cam['width']), dtype=torch.uint8, device='cuda')
    cm[:, 12:52] = 1
    plan['members'][0]['center_mask'] = cm
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        res, _ = check(plan, interpolation, winners=(0, 1, 2), what='ties, masked')
        assert (res['elevation'][res['source'] == 1] >= 10.0).all() and (res['elevation'][res['source'] == 2] < 10.0).all()


@pytest.mark.parametrize('magnetic', [False, True])
def test_two_cameras_both_rules(magnetic):
    """gm-a and gm-b: different positions and azimuths, footprints that overlap in part (the SM frame on the same pair)"""
    by_rule = {}
    for mayOverlap in (True, False):
        plan = plan_of(pair(), mayOverlap, magnetic, pxPerDeg=10)
        assert plan['rule'] == int(mayOverlap) and plan['grid'].ny % 32 and plan['grid'].nx % 32
        res, members = check(plan, 'linear', magnetic, winners=(0, 1), what=('pair', mayOverlap))
        by_rule[mayOverlap] = res
        both = ~members[0]['mask'] & ~members[1]['mask']
        assert both.sum() > 100
        if mayOverlap:
            # the overlap is shared by elevation, and some 32 x 32 tile holds both winners
            assert (res['source'][both] == 0).any() and (res['source'][both] == 1).any()
            s = res['source']
            mixed = [1 for i in range(0, s.shape[0], 32) for j in range(0, s.shape[1], 32)
                     if {0, 1} <= set(np.unique(s[i:i + 32, j:j + 32]).tolist())]
            assert mixed
        else:
            assert (res['source'][both] == 0).all()                     # the lower index wins the overlap
    assert not np.array_equal(by_rule[True]['source'], by_rule[False]['source'])
    assert np.array_equal(by_rule[True]['mask'], by_rule[False]['mask'])


def test_paths_and_winner_coordinates():
    from auromat_amd.coordinates.inverse import W2P_GEODETIC, world_to_pixel
    from auromat_amd.resample import GATHER_PATH_CELL, gather_mosaic_frames
    plan = plan_of(pair(np.uint16, 3), True, pxPerDeg=10)
    res, _ = check(plan, 'linear', winners=(0, 1), what='paths', debug=dict(tile_path=True), xy=True)
    tiles = res['tile_path']
    assert tiles.shape == ((plan['grid'].ny + 31) // 32, (plan['grid'].nx + 31) // 32)
    # nobody (a tile outside every footprint), staged (one winner: the interior of a footprint), per cell (mixed winners)
    assert set(np.unique(tiles).tolist()) == {0, 1, 2}
    s = res['source']
    for i in range(tiles.shape[0]):
        for j in range(tiles.shape[1]):
            won = set(np.unique(s[32 * i:32 * i + 32, 32 * j:32 * j + 32]).tolist()) - {-1}
            assert (tiles[i, j] == 0) == (not won)
            assert tiles[i, j] != 1 or len(won) == 1
            assert len(won) < 2 or tiles[i, j] == 2
    for interpolation in ('linear', 'lanczos4'):
        auto = gather_mosaic_frames(plan, None, interpolation, debug=dict(tile_path=True))
        cell = gather_mosaic_frames(plan, None, interpolation, debug=dict(force_path=GATHER_PATH_CELL, tile_path=True))
        assert (auto['tile_path'] == 1).any() and not (cell['tile_path'] == 1).any()
        assert np.array_equal(cell['tile_path'] == 0, auto['tile_path'] == 0)
        for k in ('img', 'mask', 'source'):
            assert same_bits(auto[k], cell[k]), (interpolation, k)
        assert np.array_equal(auto['elevation'], cell['elevation'], equal_nan=True)
    # out_xy: the winner's world_to_pixel coordinates
    want = np.full(s.shape + (2,), np.nan)
    for i, m in enumerate(plan['members']):
        xy, _, _ = world_to_pixel(m['params'], m['zenithal'], W2P_GEODETIC, np.ascontiguousarray(res['lat_c']),
                                  np.ascontiguousarray(res['lon_c']))
        want[s == i] = xy[s == i]
    assert np.isnan(res['xy'][s < 0]).all() and same_bits(res['xy'][s >= 0], want[s >= 0])


def test_33_members():
    import torch
    cam = GC.by_name('gm-a')
    members = [GC.mapping(cam, GC.image(cam, seed=10 + i), identifier='m%d' % i) for i in range(33)]
    plan = plan_of(members, pxPerDeg=8)
    assert len(plan['members']) == 33
    # all but the last member are blind in a rectangle of the frame: those cells are the last member's
    cm = torch.zeros((cam['height'], cam['width']), dtype=torch.uint8, device='cuda')
    cm[10:40, 8:50] = 1
    for m in plan['members'][:32]:
        m['center_mask'] = cm
    res, _ = check(plan, 'linear', winners=(0, 32), what='33 members')
    assert set(np.unique(res['source']).tolist()) == {-1, 0, 32}


def test_date_line_and_a_narrow_grid():
    a, b = GC.by_name('dateline'), GC.by_name('gm-dateline-b')
    members = [GC.mapping(a, GC.image(a, np.uint16, 3, seed=1)), GC.mapping(b, GC.image(b, np.uint16, 3, seed=2))]
    plan = plan_of(members, pxPerDeg=200)
    assert plan['contains_discontinuity'] and not plan['contains_pole'] and plan['grid'].nx < 32
    for interpolation in ('nearest', 'linear'):
        check(plan, interpolation, winners=(0, 1), what='dateline')


def test_pole_takes_the_point_form():
    a, b = GC.by_name('pole'), GC.by_name('gm-pole-b')
    members = [GC.mapping(a, GC.image(a, seed=1)), GC.mapping(b, GC.image(b, seed=2))]
    plan = plan_of(members, pxPerDeg=200)
    assert plan['contains_pole'] and all(m['center_mask'] is not None for m in plan['members'])
    for interpolation in ('nearest', 'linear'):
        check(plan, interpolation, winners=(0, 1), what='pole')


def test_projections_and_sip_share_one_launch():
    sip, zea, tan = GC.by_name('sip-3'), GC.by_name('zen-ZEA'), GC.by_name('gm-b')
    members = [GC.mapping(sip, GC.image(sip, seed=1)).maskedByElevation(12), GC.mapping(zea, GC.image(zea, seed=2)),
               GC.mapping(tan, GC.image(tan, seed=3))]
    plan = plan_of(members, pxPerDeg=10)
    assert [m['zenithal'] is not None for m in plan['members']] == [True, True, False]
    for interpolation in ('linear', 'lanczos4'):
        check(plan, interpolation, winners=(0, 1, 2), what='projections')


def test_argument_errors_write_nothing():
    import torch
    from auromat_amd._native import Context, GatherDebug, GatherMember, ZenithalWcs, ptr
    plan = plan_of(pair(), pxPerDeg=4)
    ctx = Context.current()
    ny, nx = plan['grid'].ny, plan['grid'].nx
    keep = []

    def table(n=2):
        t = (GatherMember * n)()
        for e, m in zip(t, plan['members']):
            C.memmove(C.byref(e.params), C.byref(m['params']), C.sizeof(m['params']))
            img = ctx.to_device(m['image'], dtype=np.uint8)
            keep.append(img)
            e.img, e.min_elevation = ptr(img).value, float('nan')
        return t
    lat = ctx.to_device(np.ascontiguousarray(plan['grid'].lat_c[:, 0]))
    lon = ctx.to_device(np.ascontiguousarray(plan['grid'].lon_c[0, :]))
    cells = ctx.to_device(np.ascontiguousarray(plan['grid'].lat_c)), ctx.to_device(np.ascontiguousarray(plan['grid'].lon_c))
    outs = dict(img=torch.full((ny, nx, 3), 0x5A, dtype=torch.uint8, device=ctx.device),
                mask=torch.full((ny, nx), 0x5A, dtype=torch.uint8, device=ctx.device),
                elev=torch.full((ny, nx), 1234.5, dtype=torch.float64, device=ctx.device),
                source=torch.full((ny, nx), 77, dtype=torch.int32, device=ctx.device),
                xy=torch.full((ny, nx, 2), 1234.5, dtype=torch.float64, device=ctx.device))

    def call(**kw):
        a = dict(members=table(), n=2, frame=0, lat=ptr(lat), ny=ny, lon=ptr(lon), nx=nx, cell_lat=None, cell_lon=None, bytes=1,
                 channels=3, interpolation=0, rule=1, img=ptr(outs['img']), mask=ptr(outs['mask']), elev=ptr(outs['elev']),
                 source=ptr(outs['source']), xy=ptr(outs['xy']), debug=None)
        a.update(kw)
        rc = ctx._lib.amt_gather_mosaic(ctx.handle, a['members'], a['n'], a['frame'], a['lat'], a['ny'], a['lon'], a['nx'], a['cell_lat'],
                                        a['cell_lon'], a['bytes'], a['channels'], a['interpolation'], a['rule'], a['img'], a['mask'],
                                        a['elev'], a['source'], a['xy'], a['debug'])
        return rc, (ctx._lib.amt_last_error(ctx.handle) or b'').decode()

    singular, no_image, bad_projection = table(), table(), table()
    singular[1].params.cd[:] = [0.0, 0.0, 0.0, 0.0]
    no_image[0].img = None
    zen = ZenithalWcs()
    zen.projection, zen.cd[:] = 9, [1.0, 0.0, 0.0, 1.0]
    bad_projection[1].zenithal = C.pointer(zen)
    bad_force = GatherDebug()
    bad_force.force_path = 5
    cases = [dict(members=None), dict(img=None), dict(mask=None), dict(elev=None), dict(source=None), dict(n=0), dict(n=-3),
             dict(ny=0), dict(nx=0), dict(cell_lat=ptr(cells[0]), cell_lon=ptr(cells[1])), dict(lat=None, lon=None), dict(lat=None),
             dict(lon=None, cell_lon=ptr(cells[1])), dict(frame=2), dict(frame=7), dict(interpolation=3), dict(interpolation=-1),
             dict(rule=2), dict(bytes=3), dict(bytes=8), dict(channels=2), dict(debug=C.byref(bad_force))]
    for kw in cases:
        rc, _ = call(**kw)
        assert rc == -1, kw                                            # AMT_EINVAL
    for members, word in ((singular, 'member 1: singular'), (no_image, 'member 0: member without image'),
                          (bad_projection, 'member 1: projection')):
        rc, err = call(members=members)
        assert rc == -1 and word in err, (word, err)
    ctx.synchronize()
    assert (outs['img'] == 0x5A).all() and (outs['mask'] == 0x5A).all() and (outs['source'] == 77).all()
    assert (outs['elev'] == 1234.5).all() and (outs['xy'] == 1234.5).all()
    # and the same arguments unchanged are accepted, in either coordinate form, with the same result
    rc, err = call()
    assert rc == 0, err
    ctx.synchronize()
    first = {k: v.clone() for k, v in outs.items()}
    assert (first['source'] >= 0).any() and (first['source'] < 0).any()
    rc, err = call(lat=None, lon=None, cell_lat=ptr(cells[0]), cell_lon=ptr(cells[1]))
    assert rc == 0, err
    ctx.synchronize()
    for k in ('img', 'mask', 'source'):
        assert torch.equal(first[k], outs[k]), k
    assert torch.equal(torch.nan_to_num(first['elev'], nan=-1.0), torch.nan_to_num(outs['elev'], nan=-1.0))
    del keep
