"""
Median sequences on the MI355X: ``SequencePipeline(statistic='median')`` (the native runner's median pass,
amt_run_config.statistic) against the class API's median (``resampleMedian`` / ``resampleMedianMLatMLT``, i.e.
``resample_frame_median`` on the mapping, or on its SM mapping), bit for bit; and ``amt_median_frame_async`` against
``amt_median_frame``.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_sequence import build_sequence, host

pytestmark = pytest.mark.gpu

KEYS = ('median', 'count', 'img', 'mask')
JPG = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.jpg')
WCS = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.wcs')


def class_median(m, magnetic, pxPerDeg=None, arcsecPerPx=None):
    """What resampleMedian / resampleMedianMLatMLT bin, as arrays: resample_frame_median on the (SM) mapping, with the
    arguments resampleMedian passes.  None where the class API has no grid (no valid pixel, or a pole in view with
    arcsecPerPx)."""
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import convertMappingToSM
    if m is None:
        return None
    try:
        if magnetic:
            m = convertMappingToSM(m)
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
    return R.resample_frame_median(m.frame(), m.altitude, bb, ppd, m.containsDiscontinuity, pole,
                                   outline=m.outline if pole else None)


def mapping_of(frame):
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    hdr, cam, t, img = frame[:4]
    try:
        return ArraySpacecraftMapping(hdr, 110, img, cam, t, 'f', fastCenterCalculation=True).maskedByElevation(10)
    except ValueError:
        return None                     # no valid pixel


def assert_same(got, want, what):
    if want is None:
        assert got is None, what
        return
    assert got is not None, what
    g = host(got)
    for key in KEYS:
        a, b = np.asarray(g[key]), np.asarray(want[key])
        if key == 'img':
            a = a.view(b.dtype)
        if key == 'mask':
            a = a.astype(bool)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, key)


def feed_of(frames, how):
    import torch
    if how == 'pinned':
        return [(hd, c, t, torch.from_numpy(im.view(np.int16)).pin_memory()) for hd, c, t, im in frames]
    if how == 'resident':
        return [(hd, c, t, torch.from_numpy(im.view(np.int16)).cuda()) for hd, c, t, im in frames]
    return frames


RESOLUTIONS = {'ppd10': dict(pxPerDeg=10), 'arcsec100': dict(arcsecPerPx=100)}


@pytest.fixture(scope='module')
def sequence():
    """The frames and the class API's medians of every frame, for geo / mag grids at both resolutions (computed before any
    sequence runs)."""
    import torch
    w, h = 1060, 708
    frames = build_sequence(w, h, 12, every_pole=5, empty_at=(7,))
    want = {}
    for magnetic in (False, True):
        for name, kw in RESOLUTIONS.items():
            want[magnetic, name] = [class_median(mapping_of(f), magnetic, **kw) for f in frames]
            torch.cuda.synchronize()
    return w, h, frames, want


@pytest.mark.parametrize('magnetic', [False, True], ids=['geo', 'mag'])
@pytest.mark.parametrize('res', sorted(RESOLUTIONS))
def test_median_sequence_equals_the_class_api(sequence, magnetic, res):
    from auromat_amd.pipeline import SequencePipeline
    w, h, frames, wants = sequence
    kw = RESOLUTIONS[res]
    want = wants[magnetic, res]
    assert want[7] is None
    for how in ('resident', 'pinned'):
        feed = feed_of(frames, how)
        for batch in (1, 3):
            seq = SequencePipeline(w, h, magnetic=magnetic, batch=batch, statistic='median', **kw)
            for rep in range(2):
                got = seq.process(feed, keep_on_device=True)
                assert len(got) == len(frames)
                assert seq.plans[7] == 'empty'
                assert 'median' in seq.plans
                for k in range(len(frames)):
                    if got[k] is not None:
                        assert 'mean' not in got[k]
                    assert_same(got[k], want[k], (magnetic, res, how, batch, rep, k))


def test_pageable_images_and_keep_on_device_false(sequence):
    from auromat_amd.pipeline import SequencePipeline
    w, h, frames, wants = sequence
    want = wants[False, 'ppd10']
    seq = SequencePipeline(w, h, statistic='median', keep_coordinates=False)
    got = seq.process(iter(frames), keep_on_device=False)
    for k in range(len(frames)):
        assert_same(got[k], want[k], k)


def test_mean_sequence_is_unchanged_by_the_statistic_switch(sequence):
    from auromat_amd.pipeline import SequencePipeline
    w, h, frames, _ = sequence
    feed = feed_of(frames, 'resident')
    a = SequencePipeline(w, h, pxPerDeg=10).process(feed, keep_on_device=True)
    b = SequencePipeline(w, h, pxPerDeg=10, statistic='mean').process(feed, keep_on_device=True)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(host(x)['mean'], host(y)['mean'], equal_nan=True)


def test_coarse_grid_has_all_three_tiers():
    from auromat_amd.pipeline import SequencePipeline
    w, h = 2128, 1416
    frames = build_sequence(w, h, 4, every_pole=0)
    wants = {magnetic: [class_median(mapping_of(f), magnetic, pxPerDeg=0.5) for f in frames] for magnetic in (False, True)}
    feed = feed_of(frames, 'resident')
    counts = []
    for magnetic in (False, True):
        want = wants[magnetic]
        got = SequencePipeline(w, h, pxPerDeg=0.5, magnetic=magnetic, batch=3, statistic='median').process(feed)
        for k in range(len(frames)):
            assert_same(got[k], want[k], (magnetic, k))
            counts.append(want[k]['count'].ravel())
    c = np.concatenate(counts)
    assert ((c > 0) & (c <= 64)).any() and ((c > 64) & (c <= 16384)).any() and (c > 16384).any()


def test_full_size_reference_frame_as_a_sequence():
    import torch
    from auromat_amd.cli.convert import read_header, read_image
    from auromat_amd.mapping.spacecraft import frame_inputs, getMapping
    from auromat_amd.pipeline import SequencePipeline
    from auromat_amd.resample import resampleMedian
    import numpy.ma as ma
    hdr = read_header(WCS)
    img = read_image(JPG)
    cam, t = frame_inputs(hdr)
    m = getMapping(JPG, WCS, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
    want = class_median(m, False, pxPerDeg=10)
    r = resampleMedian(m, pxPerDeg=10)
    assert np.array_equal(np.asarray(ma.getdata(r.img)), want['img'])
    dev = torch.from_numpy(np.array(img)).cuda()
    seq = SequencePipeline(img.shape[1], img.shape[0], img_dtype=img.dtype, pxPerDeg=10, statistic='median')
    got = seq.process([(hdr, cam, t, dev)] * 5)
    assert seq.plans == ['median'] * 5
    for k in range(5):
        assert_same(got[k], want, k)


@pytest.mark.parametrize('ppd', [10, 0.5, 0.05])
def test_async_entry_point_equals_the_synchronous_one_and_does_not_wait(ppd):
    import torch
    from auromat_amd import resample as R
    from auromat_amd._native import ptr
    from auromat_amd.mapping.spacecraft import getMapping
    m = getMapping(JPG, WCS, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
    fd = m.frame()
    ctx = fd.ctx
    grid, lat_c, lon_c, lon_wrap = R._frame_grid(fd, m.altitude, m.boundingBox, (ppd, ppd), m.containsDiscontinuity, False,
                                                 None, None, None)
    xaxis, yaxis = grid.axes(ctx)
    outs = []
    for name in ('amt_median_frame', 'amt_median_frame_async'):
        med = ctx.empty((grid.ny, grid.nx, 4))
        img = ctx.empty((grid.ny, grid.nx, 3), torch.uint8)
        mask = ctx.empty((grid.ny, grid.nx), torch.uint8)
        count = ctx.empty((grid.ny, grid.nx))
        args = [ptr(lat_c), ptr(lon_c), ptr(fd.elev), ptr(fd.img), fd.img_dtype_code, 3, ptr(fd.center_mask), fd.height,
                fd.width, float('-inf'), C.byref(xaxis), C.byref(yaxis), lon_wrap]
        if name == 'amt_median_frame_async':
            # (once to size the workspace: growing it synchronises the stream, as for every user of the workspace)
            ctx.call(name, *(args + [0, ptr(med), ptr(img), ptr(mask), ptr(count)]))
            torch.cuda.synchronize()
            med.fill_(0)
            img.fill_(0)
            mask.fill_(0)
            count.fill_(0)
            torch.cuda.synchronize()
            torch.cuda._sleep(200000000)                # tens of ms of GPU time ahead of the pass on the same stream
            slept = torch.cuda.Event()
            slept.record()
            ctx.call(name, *(args + [0, ptr(med), ptr(img), ptr(mask), ptr(count)]))
            assert not slept.query(), 'amt_median_frame_async waited for the stream'
        else:
            ctx.call(name, *(args + [ptr(med), ptr(img), ptr(mask), ptr(count)]))
        torch.cuda.synchronize()
        outs.append([x.cpu().numpy() for x in (med, img, mask, count)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True), ppd
    c = outs[0][3]
    if ppd == 0.05:
        assert c.max() > 16384
    if ppd == 0.5:
        assert ((c > 64) & (c <= 16384)).any()
