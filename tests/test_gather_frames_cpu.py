"""
The gathered frames without a GPU: the constructed jobs of tests/_gather_frames_cases.py hold what they claim (the float64 inverse
statement of tests/_inverse_oracle.py), the batches are what tests/test_gpu_gather_frames_cells.py says they are, the decoys of
the gated cases are harmless, every Python-side refusal comes before device work (this machine has no device: a device call
would raise NativeError), and the parser of auromat-convert refuses what it should.
"""
import os

import numpy as np
import pytest

import _gated_gather_frames_cases as GK
import _gather_frames_cases as FC


@pytest.mark.parametrize('name', FC.names())
def test_every_job_holds_what_it_claims(name):
    j = FC.by_name(name)
    seen = FC.check_claims(name)
    assert seen.shape == (j['ny'], j['nx']) and j['claims']
    a, b, points = FC.coordinates(name)
    assert points == j['points'] and np.isfinite(a).all() and np.isfinite(b).all()
    assert (a.shape, b.shape) == (((j['ny'], j['nx']),) * 2 if points else ((j['ny'],), (j['nx'],)))
    assert (np.abs(a) <= 90).all() and (np.abs(b) <= 180).all()
    # the sub-samples of a factor split every cell: their mean is the centre, and the corner ones lie inside the cell
    if not points and 'wraps' not in j['claims']:
        for n in (2, 3, 8):
            sa = FC.coordinates(name, n)[0]
            assert sa.shape == (j['ny'] * n,) and np.allclose(sa.reshape(-1, n).mean(1), a, rtol=0, atol=1e-9)
            assert (sa.reshape(-1, n)[:, 0] > j['lat_corners'][:-1]).all() and (sa.reshape(-1, n)[:, -1] < j['lat_corners'][1:]).all()


def test_the_claims_cover_the_ground():
    claims = {n: set(FC.by_name(n)['claims']) for n in FC.names()}
    assert any('nobody' in c for c in claims.values()) and any('all-seen' in c for c in claims.values())
    assert any({'seen', 'unseen', 'tail-y', 'tail-x'} <= c for c in claims.values())
    assert any('wraps' in c for c in claims.values()) and any('unseen-tile' in c for c in claims.values())
    assert [FC.by_name(n)['points'] for n in FC.names()].count(True) == 1
    assert {FC.by_name(n)['frame'] for n in FC.names()} == {'geodetic', 'sm'}
    # a seen point stays seen at its sub-samples' level: the supersampled runs have partly seen cells
    seen = FC.seen_points('gm-a', 2)
    cells = seen.reshape(95, 2, 155, 2).sum(axis=(1, 3))
    assert ((cells > 0) & (cells < 4)).any() and (cells == 4).any() and (cells == 0).any()


def test_the_batches():
    shapes = [(FC.by_name(n)['ny'], FC.by_name(n)['nx']) for n in FC.FIVE]
    assert shapes[:3] == [(1, 1), (33, 31), (32, 64)] and FC.FIVE[3:] == ['gm-a', 'gm-wide']
    assert sorted(FC.FIVE_OTHER_ORDER) == sorted(FC.FIVE) and FC.FIVE_OTHER_ORDER != FC.FIVE
    assert FC.tiles('g33x31') == (2, 1) and FC.tiles('g32x64') == (1, 2) and FC.tiles('one-cell') == (1, 1)
    assert FC.tiles('g33x31', 8) == (9, 8) and FC.tiles('g32x64', 5) == (6, 11)
    assert 'nobody' in FC.by_name(FC.UNSEEN_BETWEEN[1])['claims']
    assert all('all-seen' in FC.by_name(n)['claims'] for n in (FC.UNSEEN_BETWEEN[0], FC.UNSEEN_BETWEEN[2]))
    a, b = (FC.by_name(n) for n in FC.MASKED_AND_NOT)
    assert a['cam'] == b['cam'] and a['masked_columns'] and a['min_elevation'] == 10.0 and not b['masked_columns']
    assert np.array_equal(a['lat_corners'], b['lat_corners']) and np.array_equal(a['lon_corners'], b['lon_corners'])
    assert FC.center_mask(a).sum() == 40 * FC.camera(a)['height'] and FC.center_mask(b) is None
    assert all(FC.by_name(n)['frame'] == 'sm' for n in FC.SM)
    for names in FC.BATCHES.values():
        assert 1 <= len(names) <= FC.MAX_JOBS and all(n in FC.names() for n in names)
    assert len({(FC.camera(n)['width'], FC.camera(n)['height']) for n in FC.FORMS}) > 1


@pytest.mark.parametrize('k', range(0, FC.MAX_JOBS + 1, 7))
def test_the_one_tile_jobs(k):
    j = FC.small(k)
    assert FC.tiles(j) == (1, 1) and 1 <= j['ny'] <= 32 and 1 <= j['nx'] <= 32
    FC.check_claims(j)


def test_the_arena_layout():
    jobs = [FC.by_name(n) for n in FC.FIVE]
    for itemsize, channels, n in ((1, 3, 1), (2, 4, 3), (4, 1, 8)):
        offsets, size = FC.layout(jobs, itemsize, channels, n)
        spans = sorted(v for o in offsets for v in o.values())
        assert all(at % FC.ALIGN == 0 for at, _ in spans) and spans[0][0] == 0
        assert all(a + na <= b for (a, na), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] < size
        assert all(('count' in o) == (n > 1) for o in offsets)
        assert [o['img'][1] for o in offsets] == [j['ny'] * j['nx'] * channels * itemsize for j in jobs]


@pytest.mark.parametrize('n', [1, 3])
def test_the_gated_decoys_are_harmless(n):
    assert len(GK.HARMLESS) > 100 and 'index' in GK.HARMLESS
    inputs, outputs = GK.inputs(n), GK.outputs(n)
    assert 'center_mask' in inputs and sum(k.startswith('img_') for k in inputs) == len(GK.JOBS)
    for name, (true, decoy) in inputs.items():
        assert true.shape == decoy.shape and true.dtype == decoy.dtype and not np.array_equal(true, decoy), name
        for a in (true, decoy):
            assert np.isfinite(a.astype(np.float64)).all(), name
            if name.startswith('lat_'):
                assert (np.abs(a) <= 90).all(), name
            if name.startswith('lon_'):
                assert (np.abs(a) <= 180).all(), name
            if name == 'center_mask':
                assert set(np.unique(a)) == {0, 1}
            # no integer input wider than a sample: nothing the kernel could take for an index
            assert a.dtype.kind == 'f' or a.dtype.itemsize <= 2, name
    assert ('count_0' in outputs) == (n > 1) and len(outputs) == len(GK.JOBS) * (4 if n > 1 else 3)


def test_symbols():
    from auromat_amd import _native
    from auromat_amd import pipeline as P
    from auromat_amd import resample as R
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'auromat_hip.h')).read()
    assert 'amt_gather_frames' in _native._SIGNATURES and 'int amt_gather_frames(amt_ctx* ctx' in header
    assert 'amt_gather_frames' in _native.exported_symbols()
    assert '#define AMT_ABI_VERSION 10' in header and _native.ABI_VERSION == 10
    assert '#define AMT_GATHER_MAX_JOBS 64' in header and _native.GATHER_MAX_JOBS == FC.MAX_JOBS == 64
    assert 'typedef struct amt_gather_job' in header
    assert [f[0] for f in _native.GatherJob._fields_] == ['member', 'ny', 'nx', 'lat', 'lon', 'cell_lat', 'cell_lon', 'out_img',
                                                          'out_mask', 'out_elev', 'out_count']
    assert len(_native._SIGNATURES['amt_gather_frames'][0]) == 10
    assert callable(R.gather_frames) and callable(R.gather_frames_coordinates) and callable(P.GatherSequence)


def test_gather_frames_refuses_before_device_work():
    from auromat_amd.resample import gather_frames
    with pytest.raises(ValueError, match='interpolation'):
        gather_frames([object()], [], interpolation='cubic', supersample=0)         # the interpolation first
    with pytest.raises(ValueError, match='supersample'):
        gather_frames([object()], [], supersample=0, minCoverage=7)                 # then the factor
    for bad in (9, True, 2.0, '2'):
        with pytest.raises(ValueError, match='supersample'):
            gather_frames([], [], supersample=bad)
    with pytest.raises(ValueError, match='minCoverage'):
        gather_frames([object()], [], supersample=2, minCoverage=0)                 # then the coverage
    with pytest.raises(ValueError, match='minCoverage.*supersample'):
        gather_frames([object()], [], minCoverage=0.5)
    with pytest.raises(ValueError, match='2 images for 1 plans'):                   # then the lists
        gather_frames([object()], [object(), object()])
    with pytest.raises(ValueError, match='0 images for 3 plans'):
        gather_frames(iter([1, 2, 3]), (), 'nearest', supersample=8, minCoverage=1.0)


def test_gather_sequence_validates_its_arguments_before_device_work():
    from auromat_amd.pipeline import GatherSequence
    for kw, word in ((dict(interpolation='cubic', supersample=0), 'interpolation'), (dict(supersample=0, batch=0), 'supersample'),
                     (dict(supersample=9), 'supersample'), (dict(supersample=True), 'supersample'),
                     (dict(supersample=2, minCoverage=1.5), 'minCoverage'), (dict(minCoverage=0.5), 'minCoverage'),
                     (dict(batch=0), 'batch'), (dict(batch=65), 'batch'), (dict(batch=2.5), 'batch'), (dict(batch=True), 'batch'),
                     (dict(nchan=2), 'nchan'), (dict(img_dtype=np.float64), 'img_dtype'), (dict(img_dtype=np.int16), 'img_dtype'),
                     (dict(arcsecPerPx=-100), 'arcsecPerPx')):
        with pytest.raises(ValueError, match=word):
            GatherSequence(64, 48, **kw)
    with pytest.raises(ValueError, match='width'):
        GatherSequence(0, 48)


def test_convert_parser(capsys):
    from auromat_amd.cli.convert import getParser, parseargs
    base = ['--data', '/nonexistent', '--format', 'netcdf']
    a = parseargs(base + ['--resample', '--gather', 'linear'])
    assert (a.gather, a.supersample, a.minCoverage, a.statistic) == ('linear', 1, None, 'mean')
    a = parseargs(base + ['--resample', '--gather', 'lanczos4', '--supersample', '8', '--min-coverage', '1', '--grid', 'geo'])
    assert (a.gather, a.supersample, a.minCoverage) == ('lanczos4', 8, 1.0)
    assert parseargs(base + ['--resample', '--gather', 'nearest', '--supersample', '4']).minCoverage is None
    a = parseargs(base + ['--resample'])
    assert a.gather is None and a.supersample is None
    for bad, message in ((['--gather', 'linear'], '--gather needs --resample'),
                         (['--resample', '--gather', 'linear', '--statistic', 'median'], 'not with --statistic median'),
                         (['--resample', '--gather', 'linear', '--statistic', 'area'], 'not with --statistic area'),
                         (['--resample', '--gather', 'linear', '--statistic', 'quantile', '--quantile', '0.5'], 'not with --statistic quantile'),
                         (['--resample', '--supersample', '2'], '--supersample is only usable with --gather'),
                         (['--supersample', '2'], '--supersample is only usable with --gather'),
                         (['--resample', '--gather', 'linear', '--lens-route', 'raw'], '--lens-route raw'),
                         (['--resample', '--gather', 'linear', '--supersample', '0'], '--supersample must be in the range 1 ... 8'),
                         (['--resample', '--gather', 'linear', '--supersample', '9'], '--supersample must be in the range 1 ... 8'),
                         (['--resample', '--gather', 'linear', '--min-coverage', '0.5'], '--min-coverage goes with --supersample above 1'),
                         (['--resample', '--gather', 'linear', '--supersample', '2', '--min-coverage', '0'], 'range (0, 1]'),
                         (['--resample', '--gather', 'linear', '--supersample', '2', '--min-coverage', '1.5'], 'range (0, 1]'),
                         (['--resample', '--gather', 'cubic'], 'invalid choice'),
                         # unchanged without --gather
                         (['--resample', '--min-coverage', '0.5'], '--min-coverage is only usable with --statistic area')):
        with pytest.raises(SystemExit) as e:
            parseargs(base + bad)
        assert e.value.code != 0
        assert message in capsys.readouterr().err, bad
    text = getParser().format_help()
    assert '--gather' in text and '--supersample' in text
