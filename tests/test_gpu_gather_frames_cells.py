"""
amt_gather_frames on the constructed jobs of tests/_gather_frames_cases.py against one amt_gather_mosaic (factor 1) or
amt_gather_mosaic_supersampled (factor > 1) call per job on a table of that job's one member: every byte of every output, the
masked cells included.  Each job's outputs lie back to back in one poisoned arena at 256-byte-aligned offsets; the bytes between
and after them must stay poison (_gather_frames_cases.run asserts both).  No tolerance anywhere.
"""
import numpy as np
import pytest

import _gather_frames_cases as FC

pytestmark = pytest.mark.gpu

_PATHS = set()          # every tile_path value seen by the tests of this module that ran so far


def _note(res):
    for r in res['jobs']:
        _PATHS.update(np.unique(r['tile_path']).tolist())
    return res


def test_one_job():
    res = _note(FC.run(FC.ONE))
    m = res['jobs'][0]['mask2']
    assert set(np.unique(m).tolist()) == {0, 1}


@pytest.mark.parametrize('batch', ['FIVE', 'FIVE_OTHER_ORDER'])
def test_five_jobs_of_unequal_grids(batch):
    names = FC.BATCHES[batch]
    assert sorted(names) == sorted(FC.FIVE)
    shapes = [(FC.by_name(n)['ny'], FC.by_name(n)['nx']) for n in FC.FIVE]
    assert shapes[:3] == [(1, 1), (33, 31), (32, 64)]
    res = _note(FC.run(names))
    for n, r in zip(names, res['jobs']):
        assert (r['mask2'] == 0).any(), n
    # the same job gives the same bytes wherever it stands in the table
    if batch == 'FIVE_OTHER_ORDER':
        first = FC.run(FC.FIVE, want=[res['want'][names.index(n)] for n in FC.FIVE])
        assert len(first['jobs']) == 5


def test_a_job_nobody_sees_between_two_that_are_seen():
    res = _note(FC.run(FC.UNSEEN_BETWEEN))
    seen_a, nobody, seen_b = res['jobs']
    assert (nobody['mask'] == 1).all() and not nobody['img'].any() and np.isnan(nobody['elev2']).all()
    assert (nobody['tile_path'] == 0).all()
    assert (seen_a['mask'] == 0).all() and (seen_b['mask'] == 0).all()


def test_the_same_camera_with_and_without_centre_mask_and_threshold():
    res = _note(FC.run(FC.MASKED_AND_NOT))
    masked, plain = (r['mask2'] != 0 for r in res['jobs'])
    assert (plain <= masked).all() and masked.sum() > plain.sum() and not masked.all()
    keep = ~masked
    assert (res['jobs'][0]['elev2'][keep] >= 10.0).all() and (res['jobs'][1]['elev2'][~plain] < 10.0).any()
    assert FC.same_bits(res['jobs'][0]['img2'][keep], res['jobs'][1]['img2'][keep])


@pytest.mark.parametrize('interpolation', ['nearest', 'linear'])
def test_point_form_and_date_line_among_axes_form_jobs(interpolation):
    assert [FC.by_name(n)['points'] for n in FC.FORMS] == [False, True, False, False]
    sizes = {(FC.camera(n)['width'], FC.camera(n)['height']) for n in FC.FORMS}
    assert len(sizes) > 1                                   # images of different sizes share the call
    res = _note(FC.run(FC.FORMS, np.uint16, 3, interpolation))
    for r in res['jobs']:
        assert (r['mask2'] == 0).any()


def test_sm_frame():
    res = _note(FC.run(FC.SM, frame='sm'))
    for r in res['jobs']:
        assert set(np.unique(r['mask']).tolist()) == {0, 1}


def test_zenithal_and_sip_members_among_tan_ones():
    from _inverse_oracle import is_plain_tan
    assert [is_plain_tan(FC.camera(n)) for n in FC.ZENITHAL] == [True, False, False, True]
    for interpolation in ('linear', 'lanczos4'):
        res = _note(FC.run(FC.ZENITHAL, np.float32, 1, interpolation))
        for r in res['jobs']:
            assert (r['mask2'] == 0).any()


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize('channels', [1, 3, 4])
def test_sample_types_channels_and_interpolations(dtype, channels):
    for interpolation in ('nearest', 'linear', 'lanczos4'):
        res = _note(FC.run(FC.TYPES, dtype, channels, interpolation))
        r = res['jobs'][1]
        assert r['img2'][r['mask2'] == 0].any() and not r['img2'][r['mask2'] != 0].any()
        if interpolation == 'nearest':
            assert not any((q['tile_path'] == FC.PATH_STAGED).any() for q in res['jobs'])       # no window to stage


@pytest.mark.parametrize('n', [2, 3, 5, 8])
def test_factors_and_min_counts(n):
    assert FC.TILE // n == {2: 16, 3: 10, 5: 6, 8: 4}[n]
    masked = []
    for min_count in (1, (n * n + 1) // 2, n * n):
        res = _note(FC.run(FC.SUPERSAMPLED, np.uint16, 3, 'linear', n=n, min_count=min_count))
        counts = [r['count'] for r in res['jobs']]
        assert all(int(c.max()) <= n * n for c in counts) and int(counts[3].max()) == n * n
        assert ((counts[3] > 0) & (counts[3] < n * n)).any()                # cells on the footprint's edge
        for r in res['jobs']:
            assert np.array_equal(r['mask'] != 0, r['count'] < min_count)
        assert (res['jobs'][2]['count'] == 0).all() and (res['jobs'][2]['mask'] == 1).all()      # the job nobody sees
        masked.append(int(sum((r['mask'] != 0).sum() for r in res['jobs'])))
    assert masked[0] < masked[1] < masked[2]


def test_supersampled_types_and_interpolations():
    for dtype, channels, interpolation, n in ((np.uint8, 4, 'nearest', 2), (np.float32, 4, 'lanczos4', 3), (np.float32, 1, 'linear', 4),
                                              (np.uint8, 1, 'lanczos4', 8)):
        _note(FC.run(['g33x31', 'sip-3', 'dateline'], dtype, channels, interpolation, n=n, min_count=2))


def test_sixty_four_one_tile_jobs_and_one_too_many():
    import torch
    from auromat_amd._native import Context
    jobs = [FC.small(k) for k in range(FC.MAX_JOBS)]
    assert all(FC.tiles(j) == (1, 1) for j in jobs)
    res = _note(FC.run(jobs))
    assert all((r['mask'] == 0).all() for r in res['jobs'])
    ctx = Context.current()
    inp = FC.Inputs(jobs + [FC.small(FC.MAX_JOBS)])
    _, size = FC.layout(inp.jobs, 1, 3, 1)
    arena = torch.full((size,), FC.POISON, dtype=torch.uint8, device='cuda')
    rc, err = FC.frames_call(ctx, inp, arena)
    assert rc == -1 and 'amt_gather_frames' in err and 'n_jobs' in err, err
    ctx.synchronize()
    assert (arena == FC.POISON).all()


@pytest.mark.parametrize('n', [1, 3])
def test_refusals_write_nothing(n):
    import ctypes as C

    import torch
    from auromat_amd._native import Context, GatherDebug
    ctx = Context.current()
    names = ['g33x31', 'pole-points', 'g32x64']
    inp = FC.Inputs(names, np.uint8, 3, n)
    _, size = FC.layout(inp.jobs, 1, 3, n)
    arena = torch.full((size,), FC.POISON, dtype=torch.uint8, device='cuda')
    bad_force = GatherDebug()
    bad_force.force_path = 5

    def arg(**kw):
        return lambda a, t: a.update(kw)

    def field(k, **kw):
        def edit(a, t):
            for name, v in kw.items():
                setattr(t[k], name, v)
        return edit

    def member(k, what):
        def edit(a, t):
            if what == 'singular':
                t[k].member.params.cd[:] = [0.0, 0.0, 0.0, 0.0]
            else:
                t[k].member.img = None
        return edit

    some = inp.coords[0][0]
    per_call = [arg(jobs=None), arg(n_jobs=0), arg(n_jobs=-3), arg(n_jobs=FC.MAX_JOBS + 1), arg(frame=2), arg(frame=-1),
                arg(interpolation=3), arg(bytes=3), arg(channels=2), arg(debug=C.byref(bad_force)), arg(factor=0), arg(factor=9),
                arg(min_count=0), arg(min_count=n * n + 1)]
    for edit in per_call:
        rc, err = FC.frames_call(ctx, inp, arena, min_count=n * n, edit=edit)
        assert rc == -1 and 'amt_gather_frames' in err, err
    per_job = [field(1, out_img=None), field(2, out_mask=None), field(0, out_elev=None), field(1, ny=0), field(2, nx=-1),
               field(0, lat=None), field(0, lat=None, lon=None), field(0, cell_lat=some, cell_lon=some), field(1, cell_lon=None),
               field(1, lat=some, lon=some), member(2, 'singular'), member(1, 'no image')]
    index = [1, 2, 0, 1, 2, 0, 0, 0, 1, 1, 2, 1]
    if n > 1:
        per_job.append(field(2, out_count=None))
        index.append(2)
    for edit, k in zip(per_job, index):
        rc, err = FC.frames_call(ctx, inp, arena, min_count=n * n, edit=edit)
        assert rc == -1 and 'amt_gather_frames' in err and ('job %d' % k) in err, (k, err)
    # a total tile count that does not fit the launch: 2^31 / 64 tiles in each of 64 jobs (refused before any address is used)
    big = FC.Inputs(['g33x31'] * FC.MAX_JOBS, np.uint8, 3, n)

    def huge(a, t):
        T = FC.TILE // n
        for k in range(FC.MAX_JOBS):
            t[k].ny, t[k].nx = T * 8192, T * 4096
    rc, err = FC.frames_call(ctx, big, torch.full((FC.layout(big.jobs, 1, 3, n)[1],), FC.POISON, dtype=torch.uint8, device='cuda'),
                             min_count=1, edit=huge)
    assert rc == -1 and 'do not fit one launch' in err, err
    ctx.synchronize()
    assert (arena == FC.POISON).all()
    # and the same arguments unchanged are accepted
    rc, err = FC.frames_call(ctx, inp, arena, min_count=n * n)
    assert rc == 0, err
    ctx.synchronize()
    assert (arena != FC.POISON).any()


@pytest.mark.parametrize('n,interpolation', [(1, 'linear'), (1, 'lanczos4'), (4, 'linear')])
def test_forced_per_cell_path_gives_the_same_bytes(n, interpolation):
    auto = _note(FC.run(FC.FIVE, np.uint16, 3, interpolation, n=n, min_count=1))
    assert any((r['tile_path'] == FC.PATH_STAGED).any() for r in auto['jobs'])
    cell = FC.run(FC.FIVE, np.uint16, 3, interpolation, n=n, min_count=1, force_path=FC.PATH_CELL, want=auto['want'])
    assert not any((r['tile_path'] == FC.PATH_STAGED).any() for r in cell['jobs'])


def test_every_tile_path_occurs():
    """a condition on the cases, not a measurement: across them at least one tile is staged, one takes the per-cell path and one
    is seen by nobody (a batch of its own, so that the test does not depend on which others ran)"""
    seen = set()
    for names, interpolation in ((FC.FIVE, 'linear'), (FC.UNSEEN_BETWEEN, 'nearest'), (FC.MASKED_AND_NOT, 'lanczos4')):
        for r in FC.run(names, interpolation=interpolation)['jobs']:
            seen.update(np.unique(r['tile_path']).tolist())
    assert seen == {0, FC.PATH_STAGED, FC.PATH_CELL}, seen
    assert _PATHS <= seen
