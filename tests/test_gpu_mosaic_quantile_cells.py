"""
The median and quantile mosaics (``amt_mosaic_median_frames``, ``amt_mosaic_quantile_frames``: the member-table front of
auromat_amd/csrc/amt_median.hip) on constructed cells, as plain device arrays through the C ABI (``Frame`` / ``member`` of
tests/test_gpu_bin_cells.py), outputs pre-filled with a poison byte.  Every cell of every output is compared with
tests/_mosaic_quantile_oracle.py — a literal ``np.median`` / ``np.quantile(values.astype(float64), q)`` per cell and plane over the
pixels the rule selects — bit for bit, the sign of a zero included; no cell is left out and nothing is allowed for.  On top:
count, mask and source equal ``amt_mosaic_frames`` on the same table; two runs and (outside exact ties) reversed members give
the same bytes; a one-member mosaic equals ``amt_median_frame`` / ``amt_quantile_frame``; refused arguments leave the poison.
tests/test_mosaic_quantile_cpu.py checks without a GPU that the cases hold what they claim.
"""
import ctypes as C

import numpy as np
import pytest

import _bin_cases as K
import _bin_oracle as B
import _median_cases as MC
import _mosaic_quantile_cases as X
import _mosaic_quantile_oracle as OR

pytestmark = pytest.mark.gpu

POISON = 0xA5
TABLE_QS = (0.0, 1.0, 0.5, 0.25, 0.75, 1.0 / 3.0, 0.999, 1e-9)
SINGLE_QS = (0.9,)
KEYS = ('stat', 'img', 'mask', 'count', 'source')
U8_U16 = pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])


def frames_of(mosaic):
    from test_gpu_bin_cells import Frame
    return [Frame(c) for c in mosaic.members]


def run(mosaic, rule, qs=None, frames=None, raw_q=None, source=True):
    """One call of amt_mosaic_median_frames (qs None) or amt_mosaic_quantile_frames on poisoned outputs -> host arrays
    (stat with a leading axis of 1 for the median), and the status when `raw_q` (values, nq) is given instead of raising."""
    import torch
    from auromat_amd._native import Context, MosaicMember, ptr
    ctx = Context.current()
    frames = frames or frames_of(mosaic)
    first = mosaic.members[0]
    ny, nx = mosaic.shape
    nch, dtype = first.img.shape[1], first.img.dtype
    lead = () if qs is None else (len(qs),)
    table = (MosaicMember * len(frames))(*[f.member(w) for f, w in zip(frames, mosaic.windows)])
    out = dict(stat=ctx.empty(lead + (ny, nx, nch + 1)),
               img=ctx.empty(lead + (ny, nx, nch), torch.int16 if dtype == np.uint16 else torch.uint8),
               mask=ctx.empty((ny, nx), torch.uint8), count=ctx.empty((ny, nx)), source=ctx.empty((ny, nx), torch.int32))
    for t in out.values():
        t.view(torch.uint8).fill_(POISON)
    head = [table, len(frames), frames[0].code, nch, float(first.min_elevation), C.byref(frames[0].xaxis),
            C.byref(frames[0].yaxis), first.lon_wrap, rule]
    tail = [ptr(out['stat']), ptr(out['img']) if nch else None, ptr(out['mask']), ptr(out['count']),
            ptr(out['source']) if source else None]
    if qs is None:
        ctx.call('amt_mosaic_median_frames', *(head + tail))
    else:
        raw, nq = (list(qs), len(qs)) if raw_q is None else raw_q
        ctx.call('amt_mosaic_quantile_frames', *(head + [(C.c_double * max(len(raw), 1))(*raw), nq] + tail))
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got['img'] = got['img'].view(dtype)
    if qs is None:
        got['stat'], got['img'] = got['stat'][None], got['img'][None]
    return got


def poisoned(shape_like):
    return all((np.ascontiguousarray(a).view(np.uint8) == POISON).all() for a in shape_like.values())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.kind == 'f' else a


def check(mosaic, rule, qs, got, want, what=''):
    """Every cell of every output against the oracle, bit for bit; the message names the first differing result."""
    what = '%s rule %d %s %s' % (mosaic.name, rule, 'median' if qs is None else 'q=%r' % (tuple(qs),), what)
    count = want['count']
    nch = mosaic.members[0].img.shape[1]
    for key in ('count', 'mask', 'source'):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)
    for key in ('stat', 'img'):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (what, key, got[key].shape, want[key].shape)
        same = _bits(got[key]) == _bits(want[key])
        if same.all():
            continue
        j, row, col, plane = [int(v[0]) for v in np.nonzero(~same)]
        n = int(count[row, col])
        raise AssertionError('%s: %s differs in %d values; first: result %d, output cell (%d, %d), plane %d of %d+1, count %d '
                             '(%s tier), source %d: got %r, want %r' % (
                                 what, key, int((~same).sum()), j, row, col, plane, nch, n,
                                 MC.TIERS[int(MC.tier_of(n))] if n else 'empty', int(want['source'][row, col]),
                                 got[key][j, row, col, plane], want[key][j, row, col, plane]))
    empty = count == 0
    assert np.isnan(got['stat'][:, empty]).all() and (got['img'][:, empty] == 0).all() and (got['source'][empty] == -1).all(), what


def same_bytes(a, b, what, keys=KEYS):
    for key in keys:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


def run_mean(mosaic, rule, frames):
    from test_gpu_bin_cells import run_mosaic
    return run_mosaic(mosaic, rule, frames)


def full_check(mosaic, rule, frames=None, reversed_too=True, ties=False):
    """Median, the eight quantiles in one call and a single 0.9 against the oracle; count, mask and source against
    amt_mosaic_frames; two runs; the members reversed.  Returns the outputs by statistic."""
    frames = frames or frames_of(mosaic)
    mean_want = B.mosaic(mosaic.members, mosaic.windows, rule)
    mean_got = run_mean(mosaic, rule, frames)
    outs = {}
    for qs in (None, TABLE_QS, SINGLE_QS):
        got = outs[qs] = run(mosaic, rule, qs, frames)
        check(mosaic, rule, qs, got, OR.expected(mosaic, rule, qs, mean_want))
        same_bytes(got, mean_got, (mosaic.name, rule, qs, 'and amt_mosaic_frames'), ('count', 'mask', 'source'))
        same_bytes(got, run(mosaic, rule, qs, frames), (mosaic.name, rule, qs, 'two runs'))
    # a single quantile is its entry of the eight
    j = TABLE_QS.index(0.25)
    assert run(mosaic, rule, (0.25,), frames)['stat'][0].tobytes() == outs[TABLE_QS]['stat'][j].tobytes()
    if reversed_too:
        r = mosaic.reversed()
        n = len(frames)
        for qs in (None, TABLE_QS):
            back = run(r, rule, qs, frames[::-1])
            if rule == 0:
                same_bytes(outs[qs], back, (mosaic.name, qs, 'reversed members'), ('stat', 'img', 'mask', 'count'))
                first = outs[qs]['source']
                assert ((back['source'] >= 0) == (first >= 0)).all()
            elif not ties:
                same_bytes(outs[qs], back, (mosaic.name, qs, 'reversed members'), ('stat', 'img', 'mask', 'count'))
                assert np.array_equal(back['source'], np.where(outs[qs]['source'] >= 0, n - 1 - outs[qs]['source'], -1))
            else:
                check(r, rule, qs, back, OR.expected(r, rule, qs), 'reversed')
    return outs


# ---- the constructed cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', [0, 1])
@U8_U16
def test_union_tiers(dtype, rule):
    m = X.union_tiers(dtype)
    outs = full_check(m, rule, ties=rule == 1)          # (the all-equal family ties under rule 1)
    if rule == 0:
        ny = len(X.FAMILIES)
        assert outs[None]['count'][ny - 1].astype(int).tolist() == list(X.TOTALS)


@pytest.mark.parametrize('rule', [0, 1])
@U8_U16
def test_winner_tiers(dtype, rule):
    m = X.winner_tiers(dtype)
    outs = full_check(m, rule, ties=True)               # (the last cell is an exact tie)
    if rule == 1:
        assert outs[None]['source'][0].tolist() == list(m.promises()['winners'])
        assert outs[None]['count'][0, :3].astype(int).tolist() == [40, MC.K_LARGE_MIN + 1, 1]


@pytest.mark.parametrize('rule', [0, 1])
@U8_U16
def test_seams(dtype, rule):
    full_check(X.seams(dtype), rule)


@pytest.mark.parametrize('nch,with_elev', [(0, True), (1, False), (4, True), (0, False)])
def test_channel_layouts(nch, with_elev):
    """0, 1 and 4 channels; without elevation (rule 0 only) the elevation plane is NaN and nothing is thresholded."""
    m = X.seams(np.uint16 if nch == 4 else np.uint8, nch)
    if not with_elev:
        for c in m.members:
            c.elev = None
    rules = (0, 1) if with_elev else (0,)
    for rule in rules:
        frames = frames_of(m)
        for qs in (None, (0.75, 1.0 / 3.0, 1.0)):
            got = run(m, rule, qs, frames)
            check(m, rule, qs, got, OR.expected(m, rule, qs))
            if not with_elev:
                assert np.isnan(got['stat'][..., nch]).all()


def test_source_is_optional_for_rule_0():
    m = X.seams(np.uint8)
    frames = frames_of(m)
    with_source, without = run(m, 0, SINGLE_QS, frames), run(m, 0, SINGLE_QS, frames, source=False)
    same_bytes(with_source, without, 'source NULL', ('stat', 'img', 'mask', 'count'))
    assert (without['source'].view(np.uint8) == POISON).all()
    with_source, without = run(m, 1, None, frames), run(m, 1, None, frames, source=False)
    same_bytes(with_source, without, 'source NULL, rule 1', ('stat', 'img', 'mask', 'count'))


# ---- the existing mosaic cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_elevation', [-np.inf, 'threshold'], ids=['nothreshold', 'threshold'])
@pytest.mark.parametrize('nch', [0, 3])
@U8_U16
@pytest.mark.parametrize('rule', [0, 1])
@pytest.mark.parametrize('name', sorted(K.MOSAIC_CASES))
def test_mosaic_cases(name, rule, dtype, nch, min_elevation):
    if min_elevation == 'threshold':
        min_elevation = K.TIES_THRESHOLD if name == 'ties' else 0.0
    m = K.MOSAIC_CASES[name](dtype, nch, min_elevation)
    outs = full_check(m, rule, ties=name == 'ties')
    if name == 'ties' and rule == 1:
        assert outs[None]['source'].tolist() == [list(K.TIES_WINNERS)]


# ---- one member ------------------------------------------------------------------------------------------------------------------------
@U8_U16
def test_single_member_equals_the_frame_entry_points(dtype):
    import test_gpu_quantile_cells as QC
    case = MC.tier_table(dtype, 3, True, 'shuffled')
    ny, nx = case.shape
    m = K.Mosaic(case.name + '-as-mosaic', [case], [(0, 0, nx, ny)])
    frames = frames_of(m)
    for rule in (0, 1):
        for qs, entry in ((None, 'amt_median_frame'), (TABLE_QS, 'amt_quantile_frame')):
            alone = QC.run(case, entry, qs)
            got = run(m, rule, qs, frames)
            stat, img = (alone['quantile'][None], alone['img'][None]) if qs is None else (alone['quantile'], alone['img'])
            assert got['stat'].tobytes() == stat.tobytes() and got['img'].tobytes() == img.tobytes(), (rule, entry)
            assert got['mask'].tobytes() == alone['mask'].tobytes() and got['count'].tobytes() == alone['count'].tobytes()
            assert np.array_equal(got['source'], np.where(alone['count'] > 0, 0, -1))
    count = got['count']
    assert set(MC.COUNTS) | {MC.BIG} <= set(count.ravel().astype(int).tolist())


# ---- refused arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched():
    import torch
    from auromat_amd._native import Context, MosaicMember, NativeError, ptr
    m = X.seams(np.uint8)
    frames = frames_of(m)
    ctx = Context.current()
    ny, nx = m.shape
    nch = 3

    def call(entry, rule, table, extra=()):
        out = dict(stat=ctx.empty((8, ny, nx, nch + 1)), img=ctx.empty((8, ny, nx, nch), torch.uint8),
                   mask=ctx.empty((ny, nx), torch.uint8), count=ctx.empty((ny, nx)), source=ctx.empty((ny, nx), torch.int32))
        for t in out.values():
            t.view(torch.uint8).fill_(POISON)
        with pytest.raises(NativeError):
            ctx.call(entry, table, len(frames), 1, nch, float('-inf'), C.byref(frames[0].xaxis), C.byref(frames[0].yaxis), 0, rule,
                     *(list(extra) + [ptr(out[k]) for k in KEYS]))
        torch.cuda.synchronize()
        assert poisoned({k: t.cpu().numpy() for k, t in out.items()}), (entry, rule, extra)

    table = (MosaicMember * len(frames))(*[f.member(w) for f, w in zip(frames, m.windows)])
    for raw, nq in (([float('nan')], 1), ([0.5] * 9, 9), ([-0.1], 1)):
        for rule in (0, 1):
            call('amt_mosaic_quantile_frames', rule, table, ((C.c_double * len(raw))(*raw), nq))
    no_elev = (MosaicMember * len(frames))(*[f.member(w) for f, w in zip(frames, m.windows)])
    no_elev[3].elev = None
    call('amt_mosaic_median_frames', 1, no_elev)
    call('amt_mosaic_quantile_frames', 1, no_elev, ((C.c_double * 1)(0.5), 1))
    # and the context still works
    check(m, 1, SINGLE_QS, run(m, 1, SINGLE_QS, frames), OR.expected(m, 1, SINGLE_QS))
