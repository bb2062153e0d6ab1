"""
Area-weighted sequences on the MI355X: ``SequencePipeline(statistic='area')`` (the native runner's area pass,
amt_run_config.statistic = 2, amt_area_frame_async) against the class API (``resampleArea`` / ``resampleAreaMLatMLT``, i.e.
``resample_frame_area`` on the mapping, or on its SM mapping), bit for bit.

The frames are small on purpose (264 x 176): at 25 px/deg their pixels near the limb are wider than 16 grid cells, so the lane
path and the wave path of k_area_frame both run in a sequence of a few milliseconds; the test asserts that from the corner arrays
of the class API's mapping with the candidate-range rule of tests/_area_cases.py.
"""
import os

import numpy as np
import pytest

import _area_cases as K
from conftest import GOLDEN
from test_gpu_median_sequence import feed_of, mapping_of
from test_gpu_sequence import build_sequence, host

pytestmark = pytest.mark.gpu

KEYS = ('area', 'coverage', 'img', 'mask')
JPG = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.jpg')
WCS = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.wcs')
W, H, N = 264, 176, 12


def grid_mapping_of(m, magnetic):
    from auromat_amd.mapping.mapping import convertMappingToSM
    return convertMappingToSM(m) if magnetic else m


def class_area(m, magnetic, pxPerDeg=None, arcsecPerPx=None, minCoverage=0.5):
    """What resampleArea / resampleAreaMLatMLT bin, as arrays: resample_frame_area on the (SM) mapping, with the arguments
    resampleArea passes.  None where the class API has no grid (no valid pixel, or a pole in view with arcsecPerPx)."""
    from auromat_amd import resample as R
    if m is None:
        return None
    try:
        m = grid_mapping_of(m, magnetic)
        bb = m.boundingBox
    except ValueError:
        return None                     # no valid pixel
    pole = m.containsPole
    if arcsecPerPx:
        ppd = R.plateCarreeResolution(bb, arcsecPerPx)
        if not ppd[1] > 0:
            return None
    else:
        ppd = (pxPerDeg, pxPerDeg)
    return R.resample_frame_area(m.frame(), m.altitude, bb, ppd, m.containsDiscontinuity, pole,
                                 outline=m.outline if pole else None, minCoverage=minCoverage)


def assert_same(got, want, what):
    if want is None:
        assert got is None, what
        return
    assert got is not None, what
    g = host(got)
    assert 'mean' not in g and 'count' not in g, what
    for key in KEYS:
        a, b = np.asarray(g[key]), np.asarray(want[key])
        if key == 'img':
            a = a.view(b.dtype)
        if key == 'mask':
            a = a.astype(bool)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        if not np.array_equal(a, b, equal_nan=True):
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            at = tuple(bad[0])
            raise AssertionError('%r: %s differs in %d of %d elements, first at %r: %r != %r (coverage there %r, wanted %r)' % (
                what, key, len(bad), a.size, at, a[at], b[at], np.asarray(g['coverage'])[at[:2]], want['coverage'][at[:2]]))


def candidate_cells(m, magnetic, res):
    """Candidate cells per admitted pixel of the mapping on the grid of its class-API result `res`."""
    m = grid_mapping_of(m, magnetic)
    fd = m.frame()
    grid = res['grid']
    assert not res['contains_pole']
    case = K.AreaCase('frame', fd.host('lat'), fd.host('lon'), grid.xedges, grid.yedges, lat_c=fd.host('lat_c'),
                      elev=fd.host('elev'), mask=fd.host_mask('center'), lon_wrap=int(bool(res['contains_discontinuity'])), nch=0)
    return K.candidate_counts(case)


RESOLUTIONS = {'ppd25': dict(pxPerDeg=25), 'ppd10': dict(pxPerDeg=10), 'arcsec100': dict(arcsecPerPx=100)}


@pytest.fixture(scope='module')
def sequence():
    """The frames, their mappings and the class API's area-weighted grids of every frame, for geo / mag grids at the three
    resolutions (computed before any sequence runs)."""
    import torch
    frames = build_sequence(W, H, N, every_pole=5, empty_at=(7,))
    mappings = [mapping_of(f) for f in frames]
    want = {}
    for magnetic in (False, True):
        for name, kw in RESOLUTIONS.items():
            want[magnetic, name] = [class_area(m, magnetic, **kw) for m in mappings]
            torch.cuda.synchronize()
    for coverage in (0.0, 1.0):
        want['coverage', coverage] = [class_area(m, False, pxPerDeg=25, minCoverage=coverage) for m in mappings]
        torch.cuda.synchronize()
    return frames, mappings, want


@pytest.mark.parametrize('magnetic', [False, True], ids=['geo', 'mag'])
def test_both_regimes_occur(sequence, magnetic):
    """Frame 0: at 25 px/deg admitted pixels with at most 16 candidate cells (the lane path) and with more (the wave path); at
    10 px/deg the lane path alone."""
    frames, mappings, wants = sequence
    fine = candidate_cells(mappings[0], magnetic, wants[magnetic, 'ppd25'][0])
    print('25 px/deg: %d pixels with <= 16 candidate cells, %d with more' % ((fine <= K.LANE_CELLS).sum(), (fine > K.LANE_CELLS).sum()))
    assert (fine <= K.LANE_CELLS).sum() > 10000 and (fine > K.LANE_CELLS).sum() > 500
    coarse = candidate_cells(mappings[0], magnetic, wants[magnetic, 'ppd10'][0])
    assert 0 < coarse.max() <= K.LANE_CELLS


@pytest.mark.parametrize('magnetic', [False, True], ids=['geo', 'mag'])
@pytest.mark.parametrize('res', sorted(RESOLUTIONS))
def test_area_sequence_equals_the_class_api(sequence, magnetic, res):
    from auromat_amd.pipeline import SequencePipeline
    frames, _, wants = sequence
    kw = RESOLUTIONS[res]
    want = wants[magnetic, res]
    assert want[7] is None
    poles = [k for k in range(N) if want[k] is not None and want[k]['contains_pole']]
    if not magnetic and 'pxPerDeg' in kw:
        assert poles
    for how in ('resident', 'pinned'):
        feed = feed_of(frames, how)
        for batch in (1, 3):
            seq = SequencePipeline(W, H, magnetic=magnetic, batch=batch, statistic='area', minCoverage=0.5, **kw)
            for rep in range(2):
                got = seq.process(feed, keep_on_device=True)
                assert len(got) == N
                assert seq.plans[7] == 'empty'
                assert 'area' in seq.plans
                for k in poles:
                    assert seq.plans[k] == 'two-pass'       # the fall-back: FramePipeline.run(statistic='area')
                for k in range(N):
                    assert_same(got[k], want[k], (magnetic, res, how, batch, rep, k))


def test_min_coverage(sequence):
    from auromat_amd.pipeline import SequencePipeline
    frames, mappings, wants = sequence
    half = wants[False, 'ppd25']
    feed = feed_of(frames, 'resident')
    for coverage in (0.0, 1.0):
        want = wants['coverage', coverage]
        assert not np.array_equal(want[0]['mask'], half[0]['mask'])
        seq = SequencePipeline(W, H, pxPerDeg=25, statistic='area', minCoverage=coverage)
        got = seq.process(feed, keep_on_device=True)
        for k in range(N):
            assert_same(got[k], want[k], (coverage, k))
    # the default is 0.5
    got = SequencePipeline(W, H, pxPerDeg=25, statistic='area').process(feed, keep_on_device=True)
    for k in range(N):
        assert_same(got[k], half[k], ('default', k))
    with pytest.raises(ValueError):
        SequencePipeline(W, H, pxPerDeg=25, statistic='area', minCoverage=1.5)
    with pytest.raises(ValueError):
        SequencePipeline(W, H, pxPerDeg=25, statistic='area', quantile=0.5)
    with pytest.raises(ValueError):
        SequencePipeline(W, H, pxPerDeg=25, statistic='median', minCoverage=0.5)


def test_frame_pipeline_statistic_area(sequence):
    """FramePipeline.run / resample(statistic='area') are resample_frame_area, on both grids; minCoverage with another statistic
    is refused."""
    from auromat_amd.pipeline import FramePipeline
    frames, _, wants = sequence
    hdr, cam, t, img = frames[0]
    for magnetic in (False, True):
        pipe = FramePipeline(W, H, with_mag=magnetic)
        got = pipe.run(hdr, 110, cam, t, img=img, pxPerDeg=25, magnetic=magnetic, statistic='area', minCoverage=0.5)
        assert pipe.last_plan == 'two-pass'
        assert_same(got, wants[magnetic, 'ppd25'][0], magnetic)
        assert_same(pipe.resample(25, magnetic=magnetic, statistic='area'), wants[magnetic, 'ppd25'][0], magnetic)
        with pytest.raises(ValueError):
            pipe.resample(25, magnetic=magnetic, statistic='median', minCoverage=0.5)
        with pytest.raises(ValueError):
            pipe.resample(25, magnetic=magnetic, statistic='area', minCoverage=-0.1)


def test_pageable_images_and_keep_on_device_false(sequence):
    from auromat_amd.pipeline import SequencePipeline
    frames, _, wants = sequence
    want = wants[False, 'ppd10']
    seq = SequencePipeline(W, H, statistic='area', keep_coordinates=False)
    got = seq.process(iter(frames), keep_on_device=False)
    for k in range(N):
        assert_same(got[k], want[k], k)
        if got[k] is not None:
            assert isinstance(got[k]['area'], np.ndarray) and got[k]['lat'].shape == (want[k]['area'].shape[0] + 1,
                                                                                        want[k]['area'].shape[1] + 1)


def test_full_size_reference_frame_as_a_sequence():
    import numpy.ma as ma
    import torch
    from auromat_amd.cli.convert import read_header, read_image
    from auromat_amd.mapping.spacecraft import frame_inputs, getMapping
    from auromat_amd.pipeline import SequencePipeline
    from auromat_amd.resample import resampleArea
    hdr = read_header(WCS)
    img = read_image(JPG)
    cam, t = frame_inputs(hdr)
    m = getMapping(JPG, WCS, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
    want = class_area(m, False, pxPerDeg=10)
    r = resampleArea(m, pxPerDeg=10)
    assert np.array_equal(np.asarray(ma.getdata(r.img)), want['img'])
    dev = torch.from_numpy(np.array(img)).cuda()
    seq = SequencePipeline(img.shape[1], img.shape[0], img_dtype=img.dtype, pxPerDeg=10, statistic='area')
    got = seq.process([(hdr, cam, t, dev)] * 3)
    assert seq.plans == ['area'] * 3
    for k in range(3):
        assert_same(got[k], want, k)


def test_overflow_flags(sequence, monkeypatch):
    """A clean sequence reads zeros from amt_run_area_overflow after every runner call; a set word raises resample_frame_area's
    ValueError with the frame's index.  (No real geometry covers a cell 256 times over: the device side of the flag is
    tested at the entry point, tests/test_gpu_area_async.py.)"""
    from auromat_amd.pipeline import SequencePipeline
    frames, _, wants = sequence
    feed = feed_of(frames, 'resident')
    seq = SequencePipeline(W, H, pxPerDeg=10, statistic='area')
    read = []
    real = seq._area_overflow
    monkeypatch.setattr(seq, '_area_overflow', lambda n: read.append(real(n).copy()) or read[-1])
    got = seq.process(feed, keep_on_device=True)
    assert_same(got[0], wants[False, 'ppd10'][0], 0)
    assert sum(len(r) for r in read) == N and all(r.dtype == np.int32 and not r.any() for r in read)

    def frame_2_set(n):
        flags = np.zeros(n, dtype=np.int32)
        flags[2] = 1
        return flags
    monkeypatch.setattr(seq, '_area_overflow', frame_2_set)
    with pytest.raises(ValueError, match=r'256 times over.*frame 2 '):
        seq.process(feed, keep_on_device=True)
    # the pipeline goes on after the error
    monkeypatch.setattr(seq, '_area_overflow', real)
    got = seq.process(feed, keep_on_device=True)
    for k in range(N):
        assert_same(got[k], wants[False, 'ppd10'][k], k)


def test_mean_and_median_sequences_share_the_context_with_an_area_sequence(sequence):
    from auromat_amd.pipeline import SequencePipeline
    frames, _, wants = sequence
    feed = feed_of(frames, 'resident')

    def run(statistic):
        seq = SequencePipeline(W, H, pxPerDeg=10, statistic=statistic)
        return [None if r is None else host(r) for r in seq.process(feed, keep_on_device=True)]

    before = {s: run(s) for s in ('mean', 'median')}
    area = run('area')
    for k in range(N):
        assert_same(area[k], wants[False, 'ppd10'][k], k)
    for s in ('mean', 'median'):
        after = run(s)
        for a, b in zip(before[s], after):
            assert (a is None) == (b is None)
            if a is not None:
                for key in (s, 'count', 'img', 'mask'):
                    assert np.array_equal(a[key], b[key], equal_nan=True), (s, key)
