"""
Quantile sequences on the MI355X: ``SequencePipeline(statistic='quantile', quantile=q)`` — the native runner's median pass
turned into a one-quantile pass by amt_run_set_quantile — against the class API (``resampleQuantile`` /
``resampleQuantileMLatMLT``, i.e. ``resample_frame_quantile`` on the mapping or on its SM mapping), bit for bit; pole frames,
which the runner hands back, and a frame without a valid pixel included.  Mean and median sequences run afterwards in the
same process are unchanged.
"""
import numpy as np
import pytest

from test_gpu_median_sequence import class_median, feed_of, mapping_of
from test_gpu_sequence import build_sequence, host

pytestmark = pytest.mark.gpu

Q = 0.25
RESOLUTIONS = {'ppd10': dict(pxPerDeg=10), 'arcsec100': dict(arcsecPerPx=100)}


def class_quantile(m, magnetic, q, pxPerDeg=None, arcsecPerPx=None):
    """What resampleQuantile / resampleQuantileMLatMLT bin, as arrays, with the arguments resampleQuantile passes; the one
    quantile without its leading axis.  None where the class API has no grid."""
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
    res = R.resample_frame_quantile(m.frame(), m.altitude, bb, ppd, q, m.containsDiscontinuity, pole,
                                    outline=m.outline if pole else None)
    assert res['quantile'].shape[0] == res['img'].shape[0] == 1
    res['quantile'], res['img'] = res['quantile'][0], res['img'][0]
    return res


def assert_same(got, want, what, keys=('quantile', 'count', 'img', 'mask')):
    if want is None:
        assert got is None, what
        return
    assert got is not None, what
    g = host(got)
    for key in keys:
        a, b = np.asarray(g[key]), np.asarray(want[key])
        if key == 'img':
            a = a.view(b.dtype)
        if key == 'mask':
            a = a.astype(bool)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, key)


@pytest.fixture(scope='module')
def sequence():
    """Seven frames — the fifth with a pole in view, the fourth without a valid pixel — and the class API's quantile of every
    frame for geo / mag grids at both resolutions (computed before any sequence runs)."""
    import torch
    w, h = 1060, 708
    frames = build_sequence(w, h, 7, every_pole=5, empty_at=(3,))
    maps = [mapping_of(f) for f in frames]
    want = {}
    for magnetic in (False, True):
        for name, kw in RESOLUTIONS.items():
            want[magnetic, name] = [class_quantile(m, magnetic, Q, **kw) for m in maps]
            torch.cuda.synchronize()
    return w, h, frames, maps, want


@pytest.mark.parametrize('magnetic', [False, True], ids=['geo', 'mag'])
@pytest.mark.parametrize('res', sorted(RESOLUTIONS))
def test_quantile_sequence_equals_the_class_api(sequence, magnetic, res):
    from auromat_amd.pipeline import SequencePipeline
    w, h, frames, _, wants = sequence
    kw = RESOLUTIONS[res]
    want = wants[magnetic, res]
    assert want[3] is None
    feed = feed_of(frames, 'resident')
    seq = SequencePipeline(w, h, magnetic=magnetic, batch=3, statistic='quantile', quantile=Q, **kw)
    for rep in range(2):
        got = seq.process(feed, keep_on_device=True)
        assert len(got) == len(frames)
        assert seq.plans[3] == 'empty' and 'quantile' in seq.plans and 'median' not in seq.plans
        if 'pxPerDeg' in kw and not magnetic:
            # the pole frame: handed back by the runner, finished by resample_frame_quantile
            assert want[4]['contains_pole'] and seq.plans[4] not in ('quantile', 'empty', 'single-pass')
        for k in range(len(frames)):
            if got[k] is not None:
                assert 'mean' not in got[k] and 'median' not in got[k]
                assert tuple(got[k]['quantile'].shape[2:]) == (4,) and got[k]['quantile'].dim() == 3
            assert_same(got[k], want[k], (magnetic, res, rep, k))


def test_sequence_quantile_is_not_its_median_and_equals_the_classes(sequence):
    """The lower quartile differs from the median on these frames (a sequence that ignored its quantile would pass the test
    above against nothing), and the result equals resampleQuantile's mapping."""
    import numpy.ma as ma
    from auromat_amd.pipeline import SequencePipeline
    from auromat_amd.resample import resampleQuantile
    w, h, frames, maps, wants = sequence
    got = SequencePipeline(w, h, pxPerDeg=10, statistic='quantile', quantile=Q).process(iter(frames[:2]), keep_on_device=False)
    med = SequencePipeline(w, h, pxPerDeg=10, statistic='median').process(iter(frames[:2]), keep_on_device=False)
    for k in range(2):
        assert_same(got[k], wants[False, 'ppd10'][k], k)
        assert np.array_equal(got[k]['count'], med[k]['count'])
        assert not np.array_equal(got[k]['img'], med[k]['img'])
        r = resampleQuantile(mapping_of(frames[k]), Q, pxPerDeg=10)         # (a mapping of its own, as a user has it)
        assert np.array_equal(np.asarray(ma.getdata(r.img)), got[k]['img'])
        assert np.array_equal(ma.filled(r.elevation, np.nan), got[k]['quantile'][..., -1], equal_nan=True)


def test_one_quantile_per_pipeline():
    from auromat_amd.pipeline import SequencePipeline
    with pytest.raises(ValueError):
        SequencePipeline(64, 48, statistic='quantile', quantile=(0.25, 0.75))
    with pytest.raises(AssertionError):
        SequencePipeline(64, 48, statistic='quantile')
    with pytest.raises(AssertionError):
        SequencePipeline(64, 48, statistic='median', quantile=0.5)


def test_mean_and_median_sequences_afterwards_are_unchanged(sequence):
    """After the quantile sequences of this module, in the same process: a median sequence still equals the class API's
    median, and a mean sequence the frame pipeline's mean."""
    import torch
    from auromat_amd.pipeline import FramePipeline, SequencePipeline
    w, h, frames, maps, _ = sequence
    feed = feed_of(frames, 'resident')
    SequencePipeline(w, h, pxPerDeg=10, statistic='quantile', quantile=0.9).process(feed)
    want = [class_median(m, False, pxPerDeg=10) for m in maps]
    torch.cuda.synchronize()
    got = SequencePipeline(w, h, pxPerDeg=10, statistic='median').process(feed)
    for k in range(len(frames)):
        assert_same(got[k], want[k], ('median', k), keys=('median', 'count', 'img', 'mask'))
    single = FramePipeline(w, h)
    mean = SequencePipeline(w, h, pxPerDeg=10).process(feed)
    for k, (hdr, cam, t, img) in enumerate(frames):
        if k == 3:
            assert mean[k] is None
            continue
        one = single.run(hdr, 110, cam, t, img=img, pxPerDeg=10)
        assert_same(mean[k], one, ('mean', k), keys=('mean', 'count', 'img', 'mask'))
