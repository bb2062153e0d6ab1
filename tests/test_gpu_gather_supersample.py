"""
resampleGather, resampleGatherMLatMLT, resampleGatherMosaic and resampleGatherMosaicMLatMLT with ``supersample`` on the GPU.

Constructed cameras (tests/_gather_mosaic_cases.py): what the public functions return is what gather_frame / gather_mosaic_frames
give for the same plan, and that is the exact oracle of tests/_gather_supersample_cases.py — amt_gather_mosaic on the sub-sample
points, reduced in NumPy — bit for bit; `.coverage` is count / n^2; ``supersample=1`` is the call without the argument.

The reference's frame ISS030-E-102170_dc (4256 x 2832), masked by elevation 10, at 2 px / deg — cells of half a degree, some
hundred pixels across — with 4 x 4 sub-samples: every output equals the oracle, and every unmasked cell lies inside the footprint
that 8 x 8 sub-samples with a least count of one draw.
"""
import os

import numpy as np
import numpy.ma as ma
import pytest

import _gather_mosaic_cases as GC
import _gather_supersample_oracle as SO
from _gather_supersample_cases import agree, check, fine, pair, plan_of, same_bits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
JPG = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.jpg')
WCS = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.wcs')


def as_mosaic_plan(plan, image):
    """a gather_plan as the plan of a mosaic of this one member, which the oracle's device half takes"""
    member = dict(params=plan['params'], zenithal=plan['zenithal'], min_elevation=plan['min_elevation'],
                  center_mask=plan['center_mask'], image=image)
    return dict(plan, members=[member], rule=1)


def frame_agrees(res, want, what):
    assert 'flags' not in res and 'support' not in res and 'source' not in res, what
    agree(dict(res, source=want['source']), want, what)


def mapping_is(g, res, n, what):
    """the returned mapping holds the frame result's arrays, masked, and the coverage"""
    keep = ~res['mask']
    assert np.array_equal(ma.getmaskarray(g.img), np.repeat(res['mask'][:, :, None], res['img'].shape[2], 2)), what
    assert same_bits(np.asarray(g.img.data)[keep], res['img'][keep]) and g.img.dtype == res['img'].dtype, what
    assert np.array_equal(ma.getmaskarray(g.elevation), res['mask']), what           # (an unmasked cell's mean elevation is a number)
    assert same_bits(np.asarray(g.elevation.data)[keep], res['elevation'][keep]), what
    assert isinstance(g.coverage, np.ndarray) and not isinstance(g.coverage, ma.MaskedArray) and g.coverage.dtype == np.float64, what
    assert np.array_equal(g.coverage, res['count'] / float(n * n)) and g.coverage.shape == res['mask'].shape, what
    assert g.coverage.max() == 1.0 and ((g.coverage > 0) & (g.coverage < 1)).any(), what


@pytest.mark.parametrize('n', [2, 4])
@pytest.mark.parametrize('magnetic', [False, True])
def test_resample_gather(n, magnetic):
    from auromat_amd.resample import gather_frame, gather_plan, resampleGather, resampleGatherMLatMLT, supersample_min_count
    cam = GC.by_name('gm-wide')
    image = GC.image(cam, np.uint8, 3)
    call = resampleGatherMLatMLT if magnetic else resampleGather
    for minCoverage in (None, 0.25):
        g = call(GC.mapping(cam, image, lazy_elevation=5), pxPerDeg=8, supersample=n, minCoverage=minCoverage)
        plan = gather_plan(GC.mapping(cam, image, lazy_elevation=5), pxPerDeg=8, magnetic=magnetic)
        assert plan['min_elevation'] == 5.0
        res = gather_frame(plan, image, 'linear', magnetic, supersample=n, minCoverage=minCoverage)
        points = fine(as_mosaic_plan(plan, image), n, 'linear', magnetic)
        least = supersample_min_count(minCoverage, n)
        what = (n, magnetic, minCoverage)
        frame_agrees(res, SO.reduce_cells(points, n, least), what)
        assert np.array_equal(res['mask'], res['count'] < least) and 0 < res['mask'].sum() < res['mask'].size
        mapping_is(g, res, n, what)
        assert g.img.shape[:2] == (plan['grid'].ny, plan['grid'].nx)


@pytest.mark.parametrize('n', [2, 4])
@pytest.mark.parametrize('magnetic', [False, True])
def test_resample_gather_mosaic(n, magnetic):
    from auromat_amd.resample import resampleGatherMosaic, resampleGatherMosaicMLatMLT
    call = resampleGatherMosaicMLatMLT if magnetic else resampleGatherMosaic
    for mayOverlap, interpolation, minCoverage in ((True, 'linear', None), (False, 'nearest', 1.0)):
        g = call(GC.collection(pair(), mayOverlap), pxPerDeg=10, interpolation=interpolation, supersample=n, minCoverage=minCoverage)
        plan = plan_of(pair(), mayOverlap, magnetic, pxPerDeg=10)
        res, _ = check(plan, n, interpolation, magnetic, minCoverage, what='public')
        what = (n, magnetic, mayOverlap)
        mapping_is(g, res, n, what)
        assert np.array_equal(ma.getmaskarray(g.source), res['source'] < 0) and np.array_equal(res['source'] < 0, res['mask']), what
        assert np.array_equal(np.asarray(g.source.data), res['source']) and list(g.members) == plan['identifiers'], what
        assert (res['source'] == 0).any() and (res['source'] == 1).any(), what


def test_supersample_one_is_the_call_without_it():
    from auromat_amd.resample import resampleGather, resampleGatherMLatMLT, resampleGatherMosaic, resampleGatherMosaicMLatMLT
    cam = GC.by_name('gm-wide')
    image = GC.image(cam, np.uint8, 3, seed=7)
    calls = [(resampleGather, lambda: GC.mapping(cam, image, lazy_elevation=5)),
             (resampleGatherMLatMLT, lambda: GC.mapping(cam, image, lazy_elevation=5)),
             (resampleGatherMosaic, pair), (resampleGatherMosaicMLatMLT, pair)]
    for call, what in calls:
        a, b = call(what(), pxPerDeg=10), call(what(), pxPerDeg=10, supersample=1)
        assert not hasattr(a, 'coverage') and not hasattr(b, 'coverage'), call.__name__
        for k in ('img', 'elevation', 'lats', 'lons', 'latsCenter', 'lonsCenter'):
            x, y = getattr(a, k), getattr(b, k)
            assert np.array_equal(ma.getmaskarray(x), ma.getmaskarray(y)), (call.__name__, k)
            assert same_bits(np.asarray(ma.getdata(x)), np.asarray(ma.getdata(y))), (call.__name__, k)
        assert 0 < ma.getmaskarray(a.img).sum() < a.img.size
        # and a supersampled call of the same arguments lays out the same grid
        c = call(what(), pxPerDeg=10, supersample=2)
        for k in ('lats', 'lons', 'latsCenter', 'lonsCenter'):
            assert same_bits(np.asarray(ma.getdata(getattr(a, k))), np.asarray(ma.getdata(getattr(c, k)))), (call.__name__, k)
        assert hasattr(c, 'coverage')


def test_real_frame_at_half_a_degree():
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import _gather_image, gather_frame, gather_plan, resample, resampleGather, supersample_min_count

    def lazy():
        return getMapping(JPG, WCS, fastCenterCalculation=True).maskedByElevation(10)
    n, ppd = 4, 2
    m = lazy()
    g = resampleGather(m, pxPerDeg=ppd, supersample=n)
    assert m._frame is None                                                 # no per-pixel array of the frame was computed
    plan = gather_plan(lazy(), pxPerDeg=ppd)
    image = _gather_image(m)
    res = gather_frame(plan, image, 'linear', False, supersample=n)
    points = fine(as_mosaic_plan(plan, image), n)
    frame_agrees(res, SO.reduce_cells(points, n, supersample_min_count(None, n)), 'real frame')
    mapping_is(g, res, n, 'real frame')
    # the grid is the one resample() chooses
    b = resample(lazy(), pxPerDeg=ppd)
    for a in ('lats', 'lons', 'latsCenter', 'lonsCenter'):
        assert same_bits(np.asarray(ma.getdata(getattr(g, a))), np.asarray(ma.getdata(getattr(b, a)))), a
    # every valid cell lies inside the footprint that a single seen one of 8 x 8 sub-samples draws
    foot = resampleGather(lazy(), pxPerDeg=ppd, supersample=8, minCoverage=1e-9)
    gm, fm = ma.getmaskarray(g.img)[..., 0], ma.getmaskarray(foot.img)[..., 0]
    assert np.array_equal(fm, foot.coverage == 0) and (~gm).sum() > 100 and (gm & ~fm).sum() > 0
    assert not (~gm & fm).any()
    with np.errstate(invalid='ignore'):
        assert (np.asarray(g.elevation.data)[~gm] >= 10.0).all()
    print('real frame at %d px / deg, %d x %d sub-samples: grid %s, %d cells valid, %d more with any of 8 x 8 seen'
          % (ppd, n, n, gm.shape, int((~gm).sum()), int((gm & ~fm).sum())))
