"""
amt_gather_mosaic_lens, amt_gather_mosaic_supersampled_lens and amt_gather_frames_lens on hand-made plans
(tests/_lens_gather_cases.py: cameras gm-a / gm-b of tests/_gather_mosaic_cases.py as raw frames with a lens, on a grid of
40 x 70 cells: two tile rows and three tile columns, with tails), against an exact oracle: every member alone through
amt_grid_to_pixel_lens (amt_world_to_pixel_lens for the point form) + amt_remap_coords on its RAW image + the masking rules, the
members composed by the NumPy election of tests/_gather_mosaic_oracle.py, sub-samples reduced to cells by
tests/_gather_supersample_oracle.py.  Every output must agree bit for bit: no tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

import _gather_mosaic_oracle as GO
import _gather_supersample_oracle as SO
import _lens_gather_cases as G

pytestmark = pytest.mark.gpu

CODES = dict(linear=0, lanczos4=1, nearest=2)
AUTO, STAGED, CELL = 0, 1, 2


@pytest.fixture(scope='module')
def ctx():
    from auromat_amd._native import Context
    return Context.current()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- the oracle: one member alone, through the point entry points and amt_remap_coords ---------------------------------------------
def member_alone(ctx, m, frame, lat, lon, points, interpolation):
    """dict(img, mask, elevation, xy) of member `m` on the points lat x lon (`points`: lat, lon are 2-d arrays of points)"""
    import torch
    from auromat_amd._native import ptr, to_host
    from auromat_amd.coordinates.inverse import grid_to_pixel, world_to_pixel
    from auromat_amd.util.lensdistortion import _image_to_device
    a, b = ctx.to_device(np.ascontiguousarray(lat)), ctx.to_device(np.ascontiguousarray(lon))
    if points:
        xy, elev, flags = world_to_pixel(m['params'], m['zenithal'], frame, a, b, lens=m['lens'])
        xy32 = xy.to(torch.float32)
    else:
        xy32, xy, elev, flags = grid_to_pixel(ctx, m['params'], m['zenithal'], frame, a, b, xy64=True, lens=m['lens'])
    src, np_dtype, _ = _image_to_device(ctx, m['image'])
    h, w, nch = (int(v) for v in src.shape)
    assert (w, h) == (m['params'].width, m['params'].height)
    ny, nx = int(flags.shape[0]), int(flags.shape[1])
    mask = flags != 0
    near = torch.nan_to_num(torch.round(xy), nan=0.0, posinf=0.0, neginf=0.0)
    ix, iy = near[..., 0].clamp_(0, w - 1).to(torch.int64), near[..., 1].clamp_(0, h - 1).to(torch.int64)
    if m['center_mask'] is not None:
        mask |= m['center_mask'].reshape(h, w)[iy, ix] != 0
    if interpolation == 'nearest':
        dst = src[iy, ix]
    else:
        dst = torch.empty((ny, nx, nch), dtype=src.dtype, device=src.device)
        support = torch.empty((ny, nx), dtype=torch.uint8, device=src.device)
        ctx.call('amt_remap_coords', ptr(src), w, h, src.element_size(), nch, ptr(xy32.contiguous()), nx, ny, CODES[interpolation],
                 ptr(dst), ptr(support), None)
        mask |= support == 0
    if m['min_elevation'] is not None:
        mask |= ~(elev >= float(m['min_elevation']))
    return dict(img=to_host(dst.contiguous(), dtype=np_dtype), mask=to_host(mask.to(torch.uint8)).astype(bool), elevation=to_host(elev),
                xy=to_host(xy))


def composed(ctx, plan, frame, lat, lon, points, interpolation):
    alone = [member_alone(ctx, m, frame, lat, lon, points, interpolation) for m in plan['members']]
    want = GO.compose(alone, plan['rule'])
    want['xy'] = np.full(want['source'].shape + (2,), np.nan)
    for i, r in enumerate(alone):
        want['xy'][want['source'] == i] = r['xy'][want['source'] == i]
    return want, alone


# ---- the fused calls -------------------------------------------------------------------------------------------------------------------
def fused(ctx, plan, frame, lat, lon, points, interpolation, ny, nx, factor=None, min_count=1, force=AUTO, lenses='plan', old=False):
    """amt_gather_mosaic[_supersampled]_lens (old: the entry point without _lens) on (ny, nx) cells whose coordinates (of the
    cells, or with `factor` of their factor x factor sub-samples) are lat, lon -> dict of host arrays, tile_path included"""
    import torch
    from auromat_amd import resample as R
    from auromat_amd._native import GatherDebug, ptr, to_host
    members = plan['members']
    table, keep, nch, tdtype, np_dtype = R._gather_member_table(ctx, members, [m['image'] for m in members])
    lens_table = R._gather_lens_table(members) if lenses == 'plan' else lenses
    a, b = ctx.to_device(np.ascontiguousarray(lat)), ctx.to_device(np.ascontiguousarray(lon))
    form = (None, None, ptr(a), ptr(b)) if points else (ptr(a), ptr(b), None, None)
    img = torch.empty((ny, nx, nch), dtype=tdtype, device=ctx.device)
    img.view(torch.uint8).fill_(0x5A)
    mask = torch.full((ny, nx), 0x5A, dtype=torch.uint8, device=ctx.device)
    elev = torch.full((ny, nx), 1234.5, dtype=torch.float64, device=ctx.device)
    source = torch.full((ny, nx), 77, dtype=torch.int32, device=ctx.device)
    T = 32 // (factor or 1)
    tiles = torch.zeros(((ny + T - 1) // T, (nx + T - 1) // T), dtype=torch.uint8, device=ctx.device)
    dbg = GatherDebug()
    dbg.force_path, dbg.tile_path = force, ptr(tiles).value
    head = (table, len(members), frame, form[0], ny, form[1], nx, form[2], form[3])
    tail = (img.element_size(), nch, CODES[interpolation], int(plan['rule']), ptr(img), ptr(mask), ptr(elev), ptr(source))
    extra = () if old else (lens_table,)
    out = {}
    if factor is None:
        xy = torch.full((ny, nx, 2), 1234.5, dtype=torch.float64, device=ctx.device)
        ctx.call('amt_gather_mosaic' + ('' if old else '_lens'), *(head + tail + (ptr(xy), C.byref(dbg)) + extra))
        out['xy'] = to_host(xy)
    else:
        count = torch.full((ny, nx), 0x5A, dtype=torch.uint8, device=ctx.device)
        ctx.call('amt_gather_mosaic_supersampled' + ('' if old else '_lens'),
                 *(head + (factor, min_count) + tail + (ptr(count), C.byref(dbg)) + extra))
        out['count'] = to_host(count, dtype=np.uint8)
    out.update(img=to_host(img.contiguous(), dtype=np_dtype), mask=to_host(mask).astype(bool), elevation=to_host(elev),
               source=to_host(source, dtype=np.int32), tile_path=to_host(tiles))
    del keep
    return out


def agree(res, want, what, keys=('source', 'mask', 'img', 'elevation')):
    assert np.array_equal(res['source'], want['source']), what
    assert np.array_equal(res['mask'], want['mask']), what
    assert same_bits(res['img'], want['img']), what
    assert np.isnan(res['elevation'][want['mask']]).all(), what
    assert same_bits(np.where(want['mask'], 0.0, res['elevation']), np.where(want['mask'], 0.0, want['elevation'])), what
    if 'xy' in res and 'xy' in want:
        won = want['source'] >= 0
        assert np.isnan(res['xy'][~won]).all() and same_bits(res['xy'][won], want['xy'][won]), what
    if 'count' in want:
        assert np.array_equal(res['count'], want['count']), what


def axes_of(plan, points):
    g = plan['grid']
    lat, lon = np.ascontiguousarray(g.lat_c[:, 0]), np.ascontiguousarray(g.lon_c[0, :])
    if points:
        la, lo = np.meshgrid(lat, lon, indexing='ij')
        return np.ascontiguousarray(la), np.ascontiguousarray(lo)
    return lat, lon


def check(ctx, plan, interpolation, frame=0, points=False, force=AUTO, what=None):
    g = plan['grid']
    lat, lon = axes_of(plan, points)
    res = fused(ctx, plan, frame, lat, lon, points, interpolation, g.ny, g.nx, force=force)
    want, alone = composed(ctx, plan, frame, lat, lon, points, interpolation)
    agree(res, want, (what, interpolation, frame, points, force))
    assert not res['mask'].all(), what
    return res, alone


# ---- one member: every lens model, image type and path ------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['poly3', 'ptlens', 'magnify', 'outside', 'fold'])
def test_one_member_every_model_and_path(ctx, model):
    plan = G.plan_of([G.member('gm-a', model, crop=True, dtype=np.uint16, channels=3, min_elevation=4.0)])
    assert (plan['grid'].ny, plan['grid'].nx) == (40, 70)
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        for points in (False, True):
            auto, _ = check(ctx, plan, interpolation, points=points, what=model)
            cell, _ = check(ctx, plan, interpolation, points=points, force=CELL, what=model)
            assert auto['tile_path'].shape == (2, 3) and not (cell['tile_path'] == STAGED).any()
            assert np.array_equal(cell['tile_path'] == 0, auto['tile_path'] == 0)
            if interpolation != 'nearest':
                paths = set(np.unique(auto['tile_path']).tolist())
                # a strong magnification spreads a tile's taps over more than the window holds: those tiles go per cell
                assert (CELL in paths) if model == 'magnify' else (STAGED in paths), (model, interpolation, paths)
            for k in ('img', 'mask', 'source'):
                assert same_bits(auto[k], cell[k]), (model, interpolation, k)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize('channels', [1, 3, 4])
def test_every_image_type(ctx, dtype, channels):
    frame = 1 if channels == 3 else 0                      # (MLat / SM longitude for one of the three)
    plan = G.plan_of([G.member('gm-a', 'ptlens', crop=False, dtype=dtype, channels=channels),
                      G.member('gm-b', 'poly3', crop=True, dtype=dtype, channels=channels, seed=4)], grid=G.grid_40x70(sm=frame == 1))
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        res, _ = check(ctx, plan, interpolation, frame=frame, what=(dtype, channels))
        assert set(np.unique(res['source']).tolist()) >= {0, 1}


# ---- mosaics: members with and without a lens ---------------------------------------------------------------------------------------------
def test_three_members_both_rules_a_tie_a_mask_and_a_threshold(ctx):
    import torch
    cm = torch.zeros((48 + G.GROW[1], 64 + G.GROW[0]), dtype=torch.uint8, device='cuda')
    cm[:, 20:55] = 1
    for rule in (1, 0):
        for frame in (0, 1):
            # members 0 and 1 have different lenses, member 2 has none; 0 is blind in a rectangle of its RAW frame and 1 below 9
            # degrees; 0 and 2 are one camera and tie exactly where both see a cell: those cells are member 0's
            plan = G.plan_of([G.member('gm-a', 'ptlens', crop=True, seed=3, center_mask=cm),
                              G.member('gm-b', 'poly3', crop=False, seed=2, min_elevation=9.0), G.member('gm-a', None, seed=1)],
                             rule=rule, grid=G.grid_40x70(sm=frame == 1))
            for interpolation in ('nearest', 'linear', 'lanczos4'):
                res, alone = check(ctx, plan, interpolation, frame=frame, what=('three', rule))
                winners = set(np.unique(res['source']).tolist())
                assert {0, 1, 2} <= winners, (rule, frame, winners)
                with np.errstate(invalid='ignore'):
                    assert (res['elevation'][res['source'] == 1] >= 9.0).all()
                both = ~alone[0]['mask'] & ~alone[2]['mask']
                assert both.any() and (alone[0]['mask'] & ~alone[2]['mask']).any()
                if rule == 0:
                    assert (res['source'][both] == 0).all()
            check(ctx, plan, 'linear', frame=frame, points=True, what=('three, point form', rule))
    # an exact tie: the same camera and lens twice: the lower index wins wherever both see the cell
    plan = G.plan_of([G.member('gm-a', 'poly5', crop=True, seed=1), G.member('gm-a', 'poly5', crop=True, seed=2)])
    res, _ = check(ctx, plan, 'linear', what='tie')
    assert (res['source'][~res['mask']] == 0).all()


# ---- supersampled ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('factor', [1, 3, 8])
def test_supersampled_against_the_pointwise_composition(ctx, factor):
    from auromat_amd.resample import gather_subsample_coordinates
    plan = G.plan_of([G.member('gm-a', None, seed=1), G.member('gm-b', 'poly3', crop=True, seed=2),
                      G.member('gm-a', 'fold', crop=False, seed=3)])
    g = plan['grid']
    sub = gather_subsample_coordinates(plan, factor)
    lat, lon = np.ascontiguousarray(sub['lat']), np.ascontiguousarray(sub['lon'])
    assert lat.shape == (g.ny * factor,) and lon.shape == (g.nx * factor,)
    min_count = max(1, (factor * factor) // 2)
    for interpolation in ('linear', 'lanczos4') if factor != 8 else ('linear',):
        fine, _ = composed(ctx, plan, 0, lat, lon, False, interpolation)
        want = SO.reduce_cells(fine, factor, min_count)
        res = fused(ctx, plan, 0, lat, lon, False, interpolation, g.ny, g.nx, factor=factor, min_count=min_count)
        agree(res, want, ('supersampled', factor, interpolation))
        assert 0 < res['mask'].sum() < res['mask'].size and len(set(np.unique(res['source']).tolist()) - {-1}) >= 2
        if factor == 3:
            la, lo = np.meshgrid(lat, lon, indexing='ij')
            pts = fused(ctx, plan, 0, np.ascontiguousarray(la), np.ascontiguousarray(lo), True, interpolation, g.ny, g.nx, factor=factor,
                        min_count=min_count)
            for k in ('img', 'mask', 'source', 'count'):
                assert same_bits(pts[k], res[k]), k


# ---- a batch of frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
def test_gather_frames_lens_is_one_mosaic_call_per_job(ctx, n):
    import torch
    from auromat_amd import resample as R
    from auromat_amd._native import to_host
    members = [G.member('gm-a', 'poly3', crop=True, seed=1, min_elevation=3.0), G.member('gm-b', None, seed=2),
               G.member('gm-wide', 'ptlens', crop=False, seed=3)]
    from auromat_amd.resample import cached_grid
    grids = [G.grid_40x70(), cached_grid((10.0, 10.0), 54.01, 57.29, 17.01, 21.29), cached_grid((8.0, 8.0), 51.6, 54.9, 17.1, 22.9)]
    plans = [dict(G.member_plan(G.plan_of([m], grid=g), 0), image=m['image']) for m, g in zip(members, grids)]
    min_count = 1 if n == 1 else 4
    poison = {}

    def arena(cells, nch, tdtype, n_):
        spare = 4096
        poison.update(img=torch.full(((cells + spare) * nch,), 0x5A, dtype=torch.uint8, device=ctx.device),
                      mask=torch.full((cells + spare,), 0x5A, dtype=torch.uint8, device=ctx.device),
                      elevation=torch.full((cells + spare,), 1234.5, dtype=torch.float64, device=ctx.device), cells=cells, nch=nch)
        if n_ > 1:
            poison['count'] = torch.full((cells + spare,), 0x5A, dtype=torch.uint8, device=ctx.device)
        return {k: v for k, v in poison.items() if k not in ('cells', 'nch')}
    for interpolation in ('linear', 'lanczos4'):
        outs, _, _ = R._gather_frames_call(ctx, plans, [p['image'] for p in plans], interpolation, False, n, min_count, arena=arena)
        ctx.synchronize()
        cells, nch = poison['cells'], poison['nch']
        assert cells == sum(p['grid'].ny * p['grid'].nx for p in plans)
        # every byte of the arena: the jobs' outputs one after the other, then the poison
        assert (poison['img'][cells * nch:] == 0x5A).all() and (poison['mask'][cells:] == 0x5A).all()
        assert (poison['elevation'][cells:] == 1234.5).all() and (n == 1 or (poison['count'][cells:] == 0x5A).all())
        for plan, m, out in zip(plans, members, outs):
            g = plan['grid']
            one = G.plan_of([m], grid=g)
            if n == 1:
                lat, lon = axes_of(one, False)
                want = fused(ctx, one, 0, lat, lon, False, interpolation, g.ny, g.nx)
            else:
                sub = R.gather_subsample_coordinates(one, n)
                want = fused(ctx, one, 0, np.ascontiguousarray(sub['lat']), np.ascontiguousarray(sub['lon']), False, interpolation, g.ny,
                             g.nx, factor=n, min_count=min_count)
                assert np.array_equal(to_host(out['count'], dtype=np.uint8), want['count'])
            assert same_bits(to_host(out['img'].contiguous(), dtype=m['image'].dtype), want['img']), interpolation
            assert np.array_equal(to_host(out['mask']).astype(bool), want['mask'])
            assert same_bits(np.nan_to_num(to_host(out['elevation']), nan=-1.0), np.nan_to_num(want['elevation'], nan=-1.0))
            assert 0 < want['mask'].sum() < want['mask'].size


# ---- unchanged outputs, and arguments --------------------------------------------------------------------------------------------------------
def test_without_lenses_the_bytes_of_the_old_entry_points(ctx):
    from auromat_amd._native import LensModel
    plan = G.plan_of([G.member('gm-a', None, seed=1), G.member('gm-b', None, seed=2, min_elevation=6.0)])
    g = plan['grid']
    lat, lon = axes_of(plan, False)
    none = LensModel()
    nulls = (C.POINTER(LensModel) * 2)()
    kinds_none = (C.POINTER(LensModel) * 2)(C.pointer(none), C.pointer(none))
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        old = fused(ctx, plan, 0, lat, lon, False, interpolation, g.ny, g.nx, old=True)
        assert 0 < old['mask'].sum() < old['mask'].size
        for lenses in (None, nulls, kinds_none):
            new = fused(ctx, plan, 0, lat, lon, False, interpolation, g.ny, g.nx, lenses=lenses)
            for k in ('img', 'mask', 'source', 'tile_path'):
                assert same_bits(old[k], new[k]), (interpolation, k)
            assert same_bits(np.nan_to_num(old['elevation'], nan=-1.0), np.nan_to_num(new['elevation'], nan=-1.0))
            assert same_bits(np.nan_to_num(old['xy'], nan=-1.0), np.nan_to_num(new['xy'], nan=-1.0))
    from auromat_amd.resample import gather_subsample_coordinates
    sub = gather_subsample_coordinates(plan, 3)
    a, b = np.ascontiguousarray(sub['lat']), np.ascontiguousarray(sub['lon'])
    old = fused(ctx, plan, 0, a, b, False, 'linear', g.ny, g.nx, factor=3, min_count=4, old=True)
    new = fused(ctx, plan, 0, a, b, False, 'linear', g.ny, g.nx, factor=3, min_count=4, lenses=None)
    for k in ('img', 'mask', 'source', 'count', 'tile_path'):
        assert same_bits(old[k], new[k]), k
    # the identity lens without a crop: the same cells as without a lens
    ident = G.plan_of([G.member('gm-a', 'identity', seed=1), G.member('gm-b', 'identity', seed=2, min_elevation=6.0)])
    for interpolation in ('linear', 'lanczos4'):
        old = fused(ctx, plan, 0, lat, lon, False, interpolation, g.ny, g.nx, old=True)
        new = fused(ctx, ident, 0, lat, lon, False, interpolation, g.ny, g.nx)
        for k in ('img', 'mask', 'source', 'tile_path'):
            assert same_bits(old[k], new[k]), (interpolation, k)


def test_frames_without_lenses_the_bytes_of_the_old_entry_point(ctx, monkeypatch):
    """amt_gather_frames_lens with lenses = NULL, with an array of NULLs and with models of kind AMT_LENS_NONE against
    amt_gather_frames: three jobs into one poisoned arena, every byte of it"""
    import torch
    from auromat_amd import resample as R
    from auromat_amd._native import LensModel, to_host
    from auromat_amd.resample import cached_grid
    members = [G.member('gm-a', None, seed=1, min_elevation=3.0), G.member('gm-b', None, seed=2), G.member('gm-wide', None, seed=3)]
    grids = [G.grid_40x70(), cached_grid((10.0, 10.0), 54.01, 57.29, 17.01, 21.29), cached_grid((8.0, 8.0), 51.6, 54.9, 17.1, 22.9)]
    plans = [dict(G.member_plan(G.plan_of([m], grid=g), 0), image=m['image']) for m, g in zip(members, grids)]
    none = LensModel()
    tables = dict(old=None,                                                 # -> amt_gather_frames
                  null=C.POINTER(C.POINTER(LensModel))(),                    # -> amt_gather_frames_lens(..., NULL)
                  nulls=(C.POINTER(LensModel) * 3)(),
                  kind_none=(C.POINTER(LensModel) * 3)(C.pointer(none), C.pointer(none), C.pointer(none)))
    called = []
    real_call = type(ctx).call

    def spy(self, name, *args):
        called.append(name)
        return real_call(self, name, *args)
    monkeypatch.setattr(type(ctx), 'call', spy)
    for n, min_count in ((1, 1), (3, 4)):
        for interpolation in ('nearest', 'linear', 'lanczos4'):
            arenas = {}
            for key, table in tables.items():
                monkeypatch.setattr(R, '_gather_lens_table', lambda members_, t=table: t)
                made = {}

                def arena(cells, nch, tdtype, n_):
                    spare = 4096
                    made.update(img=torch.full(((cells + spare) * nch,), 0x5A, dtype=torch.uint8, device=ctx.device),
                                mask=torch.full((cells + spare,), 0x5A, dtype=torch.uint8, device=ctx.device),
                                elevation=torch.full((cells + spare,), 1234.5, dtype=torch.float64, device=ctx.device))
                    if n_ > 1:
                        made['count'] = torch.full((cells + spare,), 0x5A, dtype=torch.uint8, device=ctx.device)
                    return dict(made)
                del called[:]
                R._gather_frames_call(ctx, plans, [p['image'] for p in plans], interpolation, False, n, min_count, arena=arena)
                ctx.synchronize()
                assert [c for c in called if c.startswith('amt_gather')] == ['amt_gather_frames' + ('' if key == 'old' else '_lens')]
                arenas[key] = {k: to_host(v) for k, v in made.items()}
            old = arenas['old']
            assert (old['mask'] == 0).any() and (old['mask'] == 1).any() and (old['mask'][-4096:] == 0x5A).all()
            for key in ('null', 'nulls', 'kind_none'):
                for k, v in old.items():
                    assert same_bits(arenas[key][k], v), (n, interpolation, key, k)


def test_lens_errors_name_the_member_and_write_nothing(ctx):
    import torch
    from auromat_amd import resample as R
    from auromat_amd._native import GatherJob, LensModel, ptr
    plan = G.plan_of([G.member('gm-a', 'poly3', crop=True, seed=1), G.member('gm-b', 'ptlens', crop=True, seed=2)])
    g = plan['grid']
    members = plan['members']
    table, keep, nch, tdtype, _ = R._gather_member_table(ctx, members, [m['image'] for m in members])
    lat, lon = (ctx.to_device(v) for v in axes_of(plan, False))
    outs = dict(img=torch.full((g.ny, g.nx, nch), 0x5A, dtype=torch.uint8, device=ctx.device),
                mask=torch.full((g.ny, g.nx), 0x5A, dtype=torch.uint8, device=ctx.device),
                elev=torch.full((g.ny, g.nx), 1234.5, dtype=torch.float64, device=ctx.device),
                source=torch.full((g.ny, g.nx), 77, dtype=torch.int32, device=ctx.device),
                count=torch.full((g.ny, g.nx), 0x5A, dtype=torch.uint8, device=ctx.device))

    def lenses(**kw):
        t = (C.POINTER(LensModel) * 2)()
        made = []
        for i, m in enumerate(members):
            ln = LensModel()
            C.memmove(C.byref(ln), C.byref(m['lens']), C.sizeof(ln))
            if i == 1:
                for k, v in kw.items():
                    setattr(ln, k, v)
            made.append(ln)
            t[i] = C.pointer(ln)
        return t, made
    last = lambda: (ctx._lib.amt_last_error(ctx.handle) or b'').decode()            # noqa: E731
    jobs = (GatherJob * 2)()
    for j, t in zip(jobs, table):
        C.memmove(C.byref(j.member), C.byref(t), C.sizeof(t))
        j.ny, j.nx, j.lat, j.lon = g.ny, g.nx, ptr(lat).value, ptr(lon).value
        j.out_img, j.out_mask, j.out_elev, j.out_count = (ptr(outs[k]).value for k in ('img', 'mask', 'elev', 'count'))
    cases = [(dict(kind=9), 'unknown lens kind'), (dict(width=0), 'empty raw frame'), (dict(crop_x=70), 'crop window'),
             (dict(width=members[1]['lens'].width + 2), "params' width x height")]
    for kw, word in cases:
        t, made = lenses(**kw)
        rc = ctx._lib.amt_gather_mosaic_lens(ctx.handle, table, 2, 0, ptr(lat), g.ny, ptr(lon), g.nx, None, None, 1, nch, 0, 1,
                                             ptr(outs['img']), ptr(outs['mask']), ptr(outs['elev']), ptr(outs['source']), None, None, t)
        err = last()
        assert rc == -1 and err.startswith('amt_gather_mosaic_lens: member 1: ') and word in err, (kw, err)
        rc = ctx._lib.amt_gather_mosaic_supersampled_lens(ctx.handle, table, 2, 0, ptr(lat), g.ny, ptr(lon), g.nx, None, None, 1, 1, 1, nch,
                                                          0, 1, ptr(outs['img']), ptr(outs['mask']), ptr(outs['elev']),
                                                          ptr(outs['source']), ptr(outs['count']), None, t)
        err = last()
        assert rc == -1 and err.startswith('amt_gather_mosaic_supersampled_lens: member 1: ') and word in err, (kw, err)
        rc = ctx._lib.amt_gather_frames_lens(ctx.handle, jobs, 2, 0, 1, 1, 1, nch, 0, None, t)
        err = last()
        assert rc == -1 and err.startswith('amt_gather_frames_lens: job 1: ') and word in err, (kw, err)
    ctx.synchronize()
    assert (outs['img'] == 0x5A).all() and (outs['mask'] == 0x5A).all() and (outs['source'] == 77).all()
    assert (outs['elev'] == 1234.5).all() and (outs['count'] == 0x5A).all()
    del keep
