"""
gather_frames and GatherSequence against the existing entry points, bit for bit: gather_mosaic_frames on one-member plans (every
cell), gather_frame (the mask, and every unmasked cell; everything where supersampled), and resampleGather /
resampleGatherMLatMLT of every frame of a sequence.  No tolerance anywhere.
"""
import glob
import os
from datetime import timedelta

import numpy as np
import numpy.ma as ma
import pytest

import _gather_mosaic_cases as GC

pytestmark = pytest.mark.gpu

W, H = 265, 177
ELEVATION = 10.0


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def same_nan(a, b):
    """equal floats, NaN where the other has NaN, the same bits elsewhere"""
    return np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0))


# ---- gather_frames ------------------------------------------------------------------------------------------------------------

_PLANS = {}


def plans():
    """gather_plan of six constructed cameras, each with its image: an elevation threshold, the date line, a pole (the point
    form, with a centre mask from the arrays), a zenithal and a SIP model; images of three sizes"""
    from auromat_amd.resample import gather_plan
    if not _PLANS:
        specs = [('gm-a', 10, None), ('gm-b', 10, None), ('gm-wide', 10, 5), ('dateline', 200, None), ('pole', 200, None),
                 ('zen-ARC', 10, None), ('sip-2', 8, None)]
        made, images = [], []
        for name, ppd, lazy in specs:
            cam = GC.by_name(name)
            img = GC.image(cam, seed=len(made) + 1)
            made.append(gather_plan(GC.mapping(cam, img, lazy_elevation=lazy), pxPerDeg=ppd))
            images.append(img)
        _PLANS.update(plans=made, images=images, names=[s[0] for s in specs])
    return _PLANS['plans'], _PLANS['images'], _PLANS['names']


def mosaic_plan_of(plan, image):
    """the gather_mosaic_plan of this one member on the plan's grid"""
    member = dict(params=plan['params'], zenithal=plan['zenithal'], min_elevation=plan['min_elevation'],
                  center_mask=plan['center_mask'], image=image)
    return dict(grid=plan['grid'], contains_pole=plan['contains_pole'], contains_discontinuity=plan['contains_discontinuity'],
                altitude=plan['altitude'], rule=1, members=[member])


@pytest.mark.parametrize('interpolation,n', [('nearest', 1), ('linear', 1), ('lanczos4', 1), ('linear', 3), ('nearest', 8)])
def test_gather_frames_is_the_one_member_mosaic_in_every_cell(interpolation, n):
    from auromat_amd.resample import gather_frames, gather_mosaic_frames
    P, images, names = plans()
    assert P[3]['contains_discontinuity'] and P[4]['contains_pole'] and P[2]['min_elevation'] == 5.0
    assert P[4]['center_mask'] is not None and P[5]['zenithal'] is not None
    got = gather_frames(P, images, interpolation, supersample=n)
    assert len(got) == len(P)
    for name, plan, image, res in zip(names, P, images, got):
        want = gather_mosaic_frames(mosaic_plan_of(plan, image), None, interpolation, supersample=n)
        assert 'flags' not in res and 'support' not in res and 'source' not in res and ('count' in res) == (n > 1)
        assert same_bits(res['img'], want['img']) and np.array_equal(res['mask'], want['mask']) and res['mask'].dtype == np.bool_, name
        assert same_nan(res['elevation'], want['elevation']), name
        if n > 1:
            assert same_bits(res['count'], want['count']), name
        for k in ('lat', 'lon', 'lat_c', 'lon_c'):
            assert same_bits(res[k], want[k]), (name, k)
        assert res['grid'] is plan['grid'] and 0 < res['mask'].sum() < res['mask'].size, name


@pytest.mark.parametrize('interpolation', ['nearest', 'linear', 'lanczos4'])
def test_gather_frames_against_gather_frame(interpolation):
    from auromat_amd.resample import gather_frame, gather_frames
    P, images, names = plans()
    got = gather_frames(P, images, interpolation)
    for name, plan, image, res in zip(names, P, images, got):
        one = gather_frame(plan, image, interpolation)
        assert np.array_equal(res['mask'], one['mask']), name
        keep = ~one['mask']
        assert same_bits(res['img'][keep], one['img'][keep]) and same_bits(res['elevation'][keep], one['elevation'][keep]), name
        assert not res['img'][one['mask']].any() and np.isnan(res['elevation'][one['mask']]).all(), name
    # supersampled: everything
    for n, cov in ((2, None), (4, 0.25)):
        got = gather_frames(P, images, interpolation, supersample=n, minCoverage=cov)
        for name, plan, image, res in zip(names, P, images, got):
            one = gather_frame(plan, image, interpolation, supersample=n, minCoverage=cov)
            assert same_bits(res['img'], one['img']) and np.array_equal(res['mask'], one['mask']), (name, n)
            assert same_bits(res['count'], one['count']) and same_nan(res['elevation'], one['elevation']), (name, n)


def test_gather_frames_more_plans_than_one_call_takes_and_on_the_device():
    import torch
    from auromat_amd._native import GATHER_MAX_JOBS, to_host
    from auromat_amd.resample import gather_frames
    P, images, _ = plans()
    many = [P[k % 2] for k in range(GATHER_MAX_JOBS + 3)]
    pictures = [images[k % 2] for k in range(len(many))]
    got = gather_frames(many, pictures, 'linear', keep_on_device=True)
    assert len(got) == GATHER_MAX_JOBS + 3 and all(isinstance(r['img'], torch.Tensor) and r['img'].is_cuda for r in got)
    first = gather_frames(P[:2], images[:2], 'linear')
    for k, r in enumerate(got):
        assert same_bits(to_host(r['img'].contiguous(), dtype=np.uint8), first[k % 2]['img']), k
        assert np.array_equal(to_host(r['mask'].contiguous()).astype(bool), first[k % 2]['mask']), k


# ---- GatherSequence -------------------------------------------------------------------------------------------------------------

def sky(hdr, cam):
    """the same camera looking at the zenith: no ray hits the shell"""
    up = np.asarray(cam, dtype=np.float64) / np.linalg.norm(cam)
    return dict(hdr, CRVAL1=float(np.rad2deg(np.arctan2(up[1], up[0])) % 360), CRVAL2=float(np.rad2deg(np.arcsin(up[2]))))


_FRAMES = []


def frames():
    """seven frames: 0, 1, 3, 6 of the synthetic sequence, 2 without a valid pixel, 4 with a pole in view, 5 across the date line"""
    from auromat_amd.synthetic import frame_header, frame_image, pole_frame, sequence_frame
    if not _FRAMES:
        for k in range(7):
            hdr, cam, t, seed = sequence_frame(k, W, H)
            if k == 2:
                hdr = sky(hdr, cam)
            elif k == 4:
                hdr, cam, t = pole_frame(W, H)
            elif k == 5:
                hdr, cam, t = frame_header(W, H, 'iss029')
                t = t - timedelta(minutes=80)
            _FRAMES.append((hdr, cam, t, frame_image(W, H, seed=seed)))
    return list(_FRAMES)


KINDS = ['gather', 'gather', 'empty', 'gather', 'class', 'gather', 'gather']
_WANT = {}


def reference(k, magnetic=False, **kw):
    """resampleGather / resampleGatherMLatMLT of frame k's mapping, masked by elevation; computed once per argument set"""
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.resample import resampleGather, resampleGatherMLatMLT
    key = (k, magnetic, tuple(sorted(kw.items())))
    if key not in _WANT:
        hdr, cam, t, img = frames()[k]
        m = ArraySpacecraftMapping(hdr, 110, img, cam, t, 'frame%d' % k, fastCenterCalculation=True).maskedByElevation(ELEVATION)
        _WANT[key] = (resampleGatherMLatMLT if magnetic else resampleGather)(m, **kw)
    return _WANT[key]


def host(res):
    """a result of process() as host arrays"""
    import torch
    from auromat_amd._native import to_host
    if res is None or not isinstance(res['img'], torch.Tensor):
        return res
    out = dict(res, img=to_host(res['img'].contiguous(), dtype=np.uint16), mask=to_host(res['mask'].contiguous()).astype(bool),
               elevation=to_host(res['elevation'].contiguous()))
    if 'count' in res:
        out['count'] = to_host(res['count'].contiguous(), dtype=np.uint8)
    return out


def agrees(res, want, what, coordinates=True, n=1):
    mask = ma.getmaskarray(want.img)[:, :, 0]
    assert np.array_equal(res['mask'], mask), what
    assert same_bits(np.where(mask[:, :, None], 0, res['img']).astype(res['img'].dtype), want.img.filled(0)), what
    assert np.array_equal(ma.getmaskarray(want.elevation), mask), what
    assert same_bits(np.where(mask, 0.0, res['elevation']), want.elevation.filled(0.0)), what
    if coordinates:
        for k, a in (('lat', want.lats), ('lon', want.lons), ('lat_c', want.latsCenter), ('lon_c', want.lonsCenter)):
            assert same_bits(np.asarray(res[k]), np.asarray(a)), (what, k)
    if n > 1:
        assert same_bits(res['count'] / float(n * n), want.coverage), what


def test_sequence_of_seven_in_batches_of_three():
    from auromat_amd.pipeline import GatherSequence
    seq = GatherSequence(W, H, pxPerDeg=10, min_elevation=ELEVATION, batch=3)
    seen = []
    res = seq.process(frames(), keep_on_device=True, on_batch=lambda k0, part: seen.append((k0, len(part))))
    assert seen == [(0, 3), (3, 3), (6, 1)] and seq.gather_calls == 3
    assert seq.plans == KINDS
    assert res[2] is None and [r is None for r in res].count(True) == 1
    assert res[5]['contains_discontinuity'] and not res[0]['contains_discontinuity'] and res[4]['contains_pole']
    for k, r in enumerate(res):
        if r is not None:
            agrees(host(r), reference(k, pxPerDeg=10), k)
            assert tuple(r['pxPerDeg']) == (10, 10)
    assert res[0]['bbox'] is not None and len(res[0]['bbox']) == 8
    # a second process() on the same object gives the first one's results, also read back by the pipeline itself
    first = [host(r) for r in res]
    again = seq.process(frames(), keep_on_device=False)
    assert seq.plans[4] == 'class' and again[2] is None
    for k, (a, b) in enumerate(zip(first, again)):
        if a is not None:
            assert same_bits(a['img'], b['img']) and np.array_equal(a['mask'], b['mask']) and b['mask'].dtype == np.bool_, k
            if k != 4:              # (the class route leaves the coordinates' samples in masked cells)
                assert same_nan(a['elevation'], b['elevation']), k


@pytest.mark.parametrize('batch', [1, 8])
def test_every_batch_size_gives_the_same_bits(batch):
    from auromat_amd.pipeline import GatherSequence
    want = [host(r) for r in GatherSequence(W, H, pxPerDeg=10, min_elevation=ELEVATION, batch=3).process(frames())]
    seq = GatherSequence(W, H, pxPerDeg=10, min_elevation=ELEVATION, batch=batch)
    got = [host(r) for r in seq.process(frames())]
    assert seq.gather_calls == {1: 5, 8: 1}[batch]
    for k, (a, b) in enumerate(zip(want, got)):
        assert (a is None) == (b is None), k
        if a is not None:
            assert same_bits(a['img'], b['img']) and np.array_equal(a['mask'], b['mask']) and same_nan(a['elevation'], b['elevation']), k


def test_magnetic_grid():
    from auromat_amd.pipeline import GatherSequence
    seq = GatherSequence(W, H, pxPerDeg=10, min_elevation=ELEVATION, magnetic=True, batch=3)
    res = seq.process(frames(), keep_on_device=False)
    assert res[2] is None and seq.plans[2] == 'empty' and set(seq.plans) <= {'gather', 'empty', 'class'}
    for k, r in enumerate(res):
        if r is not None:
            agrees(r, reference(k, True, pxPerDeg=10), ('magnetic', k), coordinates=False)


def test_resolution_per_frame():
    from auromat_amd.pipeline import GatherSequence
    seq = GatherSequence(W, H, arcsecPerPx=400, min_elevation=ELEVATION, batch=3)
    res = seq.process(frames())
    assert seq.plans == ['gather', 'gather', 'empty', 'gather', 'pole-without-resolution', 'gather', 'gather']
    assert res[2] is None and res[4] is None
    for k, r in enumerate(res):
        if r is not None:
            agrees(host(r), reference(k, arcsecPerPx=400), ('arcsec', k))
            assert r['pxPerDeg'][0] == 9.0 and 0 < r['pxPerDeg'][1] <= 9.0


def test_supersampled_sequence():
    from auromat_amd.pipeline import GatherSequence
    seq = GatherSequence(W, H, pxPerDeg=4, min_elevation=ELEVATION, supersample=4, minCoverage=0.25, interpolation='nearest', batch=3)
    res = seq.process(frames(), keep_on_device=False)
    assert seq.plans[4] == 'class' and seq.plans[2] == 'empty'
    for k, r in enumerate(res):
        if r is not None:
            agrees(r, reference(k, pxPerDeg=4, supersample=4, minCoverage=0.25, interpolation='nearest'), ('x4', k), n=4)
            assert same_bits(r['coverage'], r['count'] / 16.0) and ((r['count'] > 0) & (r['count'] < 16)).any()


def test_a_generator_is_consumed_exactly_once_and_host_tensors_are_taken():
    import torch
    from auromat_amd.pipeline import GatherSequence
    taken = []

    def feed():
        for k, (hdr, cam, t, img) in enumerate(frames()):
            taken.append(k)
            # (every second image as a page-locked tensor of the buffer's type: the asynchronous upload)
            yield hdr, cam, t, (torch.from_numpy(img.view(np.int16)).pin_memory() if k % 2 else img)

    gen = feed()
    seq = GatherSequence(W, H, pxPerDeg=10, min_elevation=ELEVATION, batch=3)
    res = seq.process(gen)
    assert taken == list(range(7)) and next(gen, None) is None
    assert seq.uploaded_bytes == 5 * W * H * 3 * 2              # (not the empty frame's, not the class route's)
    for k, r in enumerate(res):
        if r is not None:
            agrees(host(r), reference(k, pxPerDeg=10), ('generator', k))
    with pytest.raises(NotImplementedError, match='resampleGather'):
        seq.process([(dict(frames()[0][0], CTYPE1='RA---ARC', CTYPE2='DEC--ARC'),) + frames()[0][1:]])


def test_the_references_ten_headers_at_full_size_with_one_device_image():
    from auromat_amd._native import Context
    from auromat_amd.fits import getSpacecraftPosition, readHeader
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.pipeline import GatherSequence
    from auromat_amd.resample import resampleGather
    from auromat_amd.synthetic import frame_image
    paths = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'resources', 'seq', '*.wcs')))
    assert len(paths) == 10
    w, h = 4256, 2832
    img = frame_image(w, h, seed=7)
    dev = Context.current().to_device(img, dtype=np.uint16)
    metas = []
    for p in paths:
        hdr = readHeader(p)
        metas.append((hdr,) + tuple(getSpacecraftPosition(hdr)))
    seq = GatherSequence(w, h, pxPerDeg=10, min_elevation=ELEVATION)
    res = seq.process([(hdr, cam, t, dev) for hdr, cam, t in metas])
    assert seq.plans == ['gather'] * 10 and seq.gather_calls == 2 and seq.uploaded_bytes == 0
    for k, ((hdr, cam, t), r) in enumerate(zip(metas, res)):
        m = ArraySpacecraftMapping(hdr, 110, img, cam, t, 'real%d' % k, fastCenterCalculation=True).maskedByElevation(ELEVATION)
        agrees(host(r), resampleGather(m, pxPerDeg=10), ('real', k))
