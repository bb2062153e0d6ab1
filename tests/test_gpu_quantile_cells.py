"""
The quantile entry points (``amt_quantile_frame``, ``amt_quantile_frame_async``: auromat_amd/csrc/amt_median.hip under
np.quantile's rank rule) on the constructed cells of tests/_median_cases.py, as plain device arrays, outputs pre-filled with a
poison byte.  Every cell of every output is compared with tests/_quantile_oracle.py's ``quantile_loop`` — a literal
``np.quantile(values.astype(float64), q)`` per cell and plane — bit for bit, no cell left out, no allowance.

The eight quantiles of the tier table, by what they reach: 0 and 1e-9 select rank 0; 1 takes the ``vi >= n-1`` clamp; 0.5,
0.25 and 0.75 give a weight of exactly 0 or 0.5 (the branch of the lerp) depending on n mod 4; 1/3 gives an inexact virtual
index; 0.999 a pair among the top keys, across a digit carry in the larger cells.  The table's value families hold all-equal
cells, equal and differing neighbouring pairs, and negative elevations straddling zero.
"""
import ctypes as C

import numpy as np
import pytest

import _median_cases as K
import _quantile_oracle as Q

pytestmark = pytest.mark.gpu

ENTRIES = ('amt_quantile_frame', 'amt_quantile_frame_async')
KEYS = ('quantile', 'img', 'mask', 'count')
POISON = 0xA5
TABLE_QS = (0.0, 1.0, 0.5, 0.25, 0.75, 1.0 / 3.0, 0.999, 1e-9)
FAMILY_QS = (0.25, 0.9)

_expected = {}


def expected(case, qs):
    """dict(quantile (nq, ny, nx, nchan+1), img (nq, ny, nx, nchan), mask, count) of a case by quantile_loop.  The oracle
    runs once per case and set of quantiles (the table: once per dtype, on all planes, whatever the order), and single
    quantiles are cut out of the set they belong to."""
    from oracle import ref_numpy as O
    base = TABLE_QS if all(q in TABLE_QS for q in qs) and case.oracle_key[0] == 'table' else FAMILY_QS
    assert all(q in base for q in qs)
    table = case.oracle_key[0] == 'table'
    key = (case.oracle_key[:2] if table else case.oracle_key, base)
    if key not in _expected:
        full = K.tier_table(case.oracle_key[1], 4, True, 'sorted') if table else case
        keep = full.keep()
        flat = full.flat()
        ny, nx = full.shape
        count = np.bincount(flat[flat >= 0], minlength=nx * ny).reshape(ny, nx).astype(np.float64)
        planes = [full.img.astype(np.float64)] + ([full.elev[:, None]] if full.elev is not None else [])
        quant = Q.quantile_loop(full.lon_binned, full.lat, np.concatenate(planes, axis=1), full.xedges, full.yedges, base,
                                keep=keep)
        assert np.array_equal(np.isnan(quant[0, ..., 0]), count == 0) or quant.shape[-1] == 0
        _expected[key] = (quant, count, full.img.shape[1], full.elev is not None)
    quant, count, full_nch, full_elev = _expected[key]
    nch = case.img.shape[1]
    pick = [base.index(q) for q in qs]
    el = quant[pick][..., full_nch:] if (case.elev is not None and full_elev) else np.full((len(qs),) + count.shape + (1,), np.nan)
    want = np.concatenate([quant[pick][..., :nch], el], axis=3)
    img, _ = O.finalize_image(want[..., :nch], case.img.dtype)
    return dict(quantile=want, img=img, mask=(count == 0).astype(np.uint8), count=count)


def upload(case):
    from auromat_amd._native import Context, ptr
    from auromat_amd.util.histogram import make_axis
    ctx = Context.current()
    nch = case.img.shape[1]
    assert case.img.dtype in (np.uint8, np.uint16)
    xaxis, xkeep = make_axis(ctx, case.xedges, uniform=case.uniform)
    yaxis, ykeep = make_axis(ctx, case.yedges, uniform=case.uniform)
    lat, lon = ctx.to_device(case.lat), ctx.to_device(case.lon)
    elev = None if case.elev is None else ctx.to_device(case.elev)
    img = ctx.to_device(case.img, case.img.dtype) if nch else None
    mask = None if case.mask is None else ctx.to_device(case.mask, np.uint8)
    args = [ptr(lat), ptr(lon), ptr(elev), ptr(img), 2 if case.img.dtype == np.uint16 else 1, nch, ptr(mask), case.height,
            case.width, float(case.min_elevation), C.byref(xaxis), C.byref(yaxis), case.lon_wrap]
    return ctx, args, (xaxis, xkeep, yaxis, ykeep, lat, lon, elev, img, mask)


def run(case, entry, qs=None, raw_q=None):
    """Uploads a case, calls one entry point (a quantile one with `qs`, a median one without) on outputs pre-filled with a
    poison byte, returns the outputs as host arrays (the median's under 'quantile', without the leading axis)."""
    import torch
    from auromat_amd._native import ptr
    ctx, args, alive = upload(case)
    ny, nx = case.shape
    nch = case.img.shape[1]
    u16 = case.img.dtype == np.uint16
    lead = () if qs is None else (len(qs),)
    quant = ctx.empty(lead + (ny, nx, nch + 1))
    out_img = ctx.empty(lead + (ny, nx, nch), torch.int16 if u16 else torch.uint8) if nch else None
    out_mask = ctx.empty((ny, nx), torch.uint8)
    count = ctx.empty((ny, nx))
    for t in (quant, out_img, out_mask, count):
        if t is not None:
            t.view(torch.uint8).fill_(POISON)
    if entry.endswith('_async'):
        args.append(case.lon_from_mlt)
    else:
        assert not case.lon_from_mlt
    if qs is not None:
        raw = list(qs) if raw_q is None else raw_q[0]
        args += [(C.c_double * max(len(raw), 1))(*raw), len(qs) if raw_q is None else raw_q[1]]
    ctx.call(entry, *(args + [ptr(quant), ptr(out_img), ptr(out_mask), ptr(count)]))
    torch.cuda.synchronize()
    del alive
    got_img = np.zeros(lead + (ny, nx, 0), dtype=case.img.dtype)
    if nch:
        got_img = out_img.cpu().numpy().view(case.img.dtype)
    return dict(quantile=quant.cpu().numpy(), img=got_img, mask=out_mask.cpu().numpy(), count=count.cpu().numpy())


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == 'f':
        return got.view(np.uint64) == want.view(np.uint64)
    return got == want


def check(case, qs, got, what=''):
    """Every cell of every output against the oracle, bit for bit (NaN only where the oracle has NaN, the sign of a zero
    included); the message names the first differing quantile, cell, plane, count and tier."""
    want = expected(case, qs)
    what = '%s %s q=%r' % (case.name, what, tuple(qs))
    count = want['count']
    nch = case.img.shape[1]
    assert got['count'].tobytes() == count.tobytes(), (what, 'count')
    assert got['mask'].tobytes() == want['mask'].tobytes(), (what, 'mask')
    for key in ('quantile', 'img'):
        same = _same_bits(got[key], want[key])
        if same.all():
            continue
        j, row, col, plane = [int(v[0]) for v in np.nonzero(~same)]
        n = int(count[row, col])
        raise AssertionError('%s: %s differs in %d values; first: q=%r, output cell (%d, %d), plane %d of %d+1, count %d (%s '
                             'tier): got %r, want %r' % (what, key, int((~same).sum()), qs[j], row, col, plane, nch, n,
                                                         K.TIERS[int(K.tier_of(n))] if n else 'empty',
                                                         got[key][j, row, col, plane], want[key][j, row, col, plane]))
    empty = count == 0
    assert np.isnan(got['quantile'][:, empty]).all() and (got['img'][:, empty] == 0).all(), what
    assert not np.isnan(got['quantile'][:, ~empty][..., :nch]).any(), what
    if case.elev is None:
        assert np.isnan(got['quantile'][..., nch]).all(), what


def same_bytes(a, b, what):
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


# ---- the tier table: eight quantiles in one call -----------------------------------------------------------------------
_table_outputs = {}


def table_outputs(dtype, order, entry):
    key = (np.dtype(dtype).name, order, entry)
    if key not in _table_outputs:
        _table_outputs[key] = run(K.tier_table(dtype, 3, True, order), entry, TABLE_QS)
    return _table_outputs[key]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('order', ['sorted', 'shuffled'])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_tier_table(dtype, order, entry):
    case = K.tier_table(dtype, 3, True, order)
    count = expected(case, TABLE_QS)['count']
    assert set(K.COUNTS) | {K.BIG} <= set(count.ravel().astype(int).tolist()) and (count > 0).sum() > 120
    check(case, TABLE_QS, table_outputs(dtype, order, entry), entry)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_tier_table_same_bytes_in_both_orders_from_both_entry_points(dtype):
    first = table_outputs(dtype, 'sorted', ENTRIES[0])
    for order in ('sorted', 'shuffled'):
        for entry in ENTRIES:
            same_bytes(table_outputs(dtype, order, entry), first, (order, entry))


def test_tier_table_reaches_what_its_quantiles_are_for():
    """From the oracle's side alone: both branches of the lerp and a weight of exactly 0 occur in every tier, the clamp and
    rank 0 are taken, and -0.0 results exist (the sign of a zero is part of the bits compared)."""
    case = K.tier_table(np.uint16, 3, True, 'sorted')
    count = expected(case, TABLE_QS)['count']
    n = count[count > 0].astype(np.int64)
    for t in range(3):
        in_tier = n[K.tier_of(n) == t]
        g = np.concatenate([Q.rank_pair(in_tier, q)[2] for q in (0.5, 0.25, 0.75)])
        assert (g == 0).any() and (g == 0.5).any() and ((g > 0) & (g < 0.5)).any() and (g > 0.5).any(), K.TIERS[t]
        k, k2, g = Q.rank_pair(in_tier, 1.0 / 3.0)
        assert ((g != 0) & (k2 == k + 1)).any()
    assert all((Q.rank_pair(n, q)[0] == 0).all() for q in (0.0, 1e-9))
    assert (Q.rank_pair(n, 1.0)[0] == n - 1).all() and (Q.rank_pair(n, 1.0)[1] == n - 1).all()
    large = n[n > K.K_LARGE_MIN]
    assert (Q.rank_pair(large, 0.999)[0] >= 0.998 * large).all()


# ---- the other case families: one quantile per call --------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('size', K.TAIL_SIZES, ids=['%dx%d' % s for s in K.TAIL_SIZES])
def test_tails_and_tiny_frames(size, entry):
    assert any(s[0] * s[1] % 4 for s in K.TAIL_SIZES)
    for dtype in (np.uint8, np.uint16):
        for ncell in K.TAIL_CELLS:
            case = K.tails(dtype, size[0], size[1], ncell)
            for q in FAMILY_QS:
                check(case, (q,), run(case, entry, (q,)), entry)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('coord', ['plain', 'wrap', 'mlt'])
@pytest.mark.parametrize('axis', ['uniform', 'nonuniform'])
def test_membership(axis, coord, entry):
    if coord == 'mlt' and not entry.endswith('_async'):
        return              # (MLT hours are an argument of the asynchronous entry point alone)
    for dtype, mode in ((np.uint8, 'threshold'), (np.uint16, 'nomask'), (np.uint16, 'nothreshold')):
        if coord != 'plain' and mode != 'threshold':
            continue
        case = K.membership(dtype, axis, mode, coord)
        for q in FAMILY_QS:
            check(case, (q,), run(case, entry, (q,)), entry)


@pytest.mark.parametrize('entry', ENTRIES)
def test_wide_sparse_grid(entry):
    case = K.sparse(np.uint16)
    assert (case.shape[0] * case.shape[1] + K.K_BLOCK * 8 - 1) // (K.K_BLOCK * 8) > 256
    for q in FAMILY_QS:
        check(case, (q,), run(case, entry, (q,)), entry)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_one_large_cell(dtype, entry):
    case = K.one_large_cell(dtype)
    for q in FAMILY_QS:
        check(case, (q,), run(case, entry, (q,)), entry)


# ---- channel layouts ---------------------------------------------------------------------------------------------------
LAYOUTS = [(np.uint8, 0, True), (np.uint8, 0, False), (np.uint8, 1, False), (np.uint16, 1, True), (np.uint8, 4, False),
           (np.uint16, 4, True)]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('planes', LAYOUTS, ids=['%s-%d-%s' % (np.dtype(d).name, n, 'elev' if e else 'noelev') for d, n, e in LAYOUTS])
def test_channel_layouts(planes, entry):
    case = K.tier_table(*planes, order='shuffled')
    qs = (0.75, 1.0 / 3.0, 1.0)
    check(case, qs, run(case, entry, qs), entry)


# ---- the quantiles of one call do not see each other -------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
def test_eight_quantiles_equal_eight_calls_of_one(entry):
    case = K.tier_table(np.uint16, 3, True, 'shuffled')
    together = table_outputs(np.uint16, 'shuffled', entry)
    for j, q in enumerate(TABLE_QS):
        one = run(case, entry, (q,))
        assert one['quantile'].tobytes() == together['quantile'][j].tobytes(), q
        assert one['img'].tobytes() == together['img'][j].tobytes(), q
        assert one['mask'].tobytes() == together['mask'].tobytes() and one['count'].tobytes() == together['count'].tobytes()
    # and the order of the quantiles is the order of the results
    back = run(case, entry, TABLE_QS[::-1])
    assert back['quantile'].tobytes() == together['quantile'][::-1].tobytes()
    assert back['img'].tobytes() == together['img'][::-1].tobytes()


# ---- q = 0.5 and the median entry points -------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_half_agrees_with_the_median_entry_points(dtype):
    """Count, mask, image and the integer planes are equal; the elevation is np.quantile's lerp here and np.median's mean
    there (each checked against its own oracle elsewhere), with NaN in the same cells."""
    case = K.tier_table(dtype, 3, True, 'shuffled')
    for entry, med_entry in zip(ENTRIES, ('amt_median_frame', 'amt_median_frame_async')):
        half = run(case, entry, (0.5,))
        med = run(case, med_entry)
        assert half['count'].tobytes() == med['count'].tobytes() and half['mask'].tobytes() == med['mask'].tobytes()
        assert half['img'][0].tobytes() == med['img'].tobytes()
        assert np.array_equal(half['quantile'][0, ..., :3], med['quantile'][..., :3], equal_nan=True)
        assert np.array_equal(np.isnan(half['quantile'][0, ..., 3]), np.isnan(med['quantile'][..., 3]))


# ---- one workspace, both statistics ------------------------------------------------------------------------------------
def test_workspace_shared_by_median_and_quantile_calls():
    import test_gpu_median_cells as MC
    from auromat_amd._native import Context
    ctx = Context.current()
    big = K.tier_table(np.uint16, 4, True, 'shuffled')
    steps = [('amt_median_frame_async', K.tier_table(np.uint8, 1, False, 'sorted'), None),
             ('amt_quantile_frame_async', big, TABLE_QS),
             ('amt_median_frame', K.tails(np.uint16, 1, 3, 2), None),
             ('amt_quantile_frame', K.one_large_cell(np.uint8), (0.9,)),
             ('amt_median_frame', big, None),
             ('amt_quantile_frame', big, TABLE_QS),
             ('amt_median_frame_async', big, None),
             ('amt_quantile_frame_async', K.tails(np.uint8, 5, 13, 5), (0.25,))]
    outs = []
    for k, (entry, case, qs) in enumerate(steps):
        assert Context.current() is ctx
        got = run(case, entry, qs)
        outs.append(got)
        if qs is None:
            got = dict(got, median=got['quantile'])
            MC.check(case, got, 'step %d %s' % (k, entry))
        else:
            check(case, qs, got, 'step %d %s' % (k, entry))
    same_bytes(outs[1], outs[5], 'second and sixth call')
    same_bytes(outs[4], outs[6], 'fifth and seventh call')


# ---- refused quantiles, with a context to carry the message --------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
def test_refused_quantiles_raise(entry):
    from auromat_amd._native import NativeError
    case = K.tails(np.uint8, 5, 13, 5)
    for raw, nq in (([0.5], 0), ([0.5] * 9, 9), ([-0.1], 1), ([1.1], 1), ([float('nan')], 1), ([0.5, 2.0], 2)):
        with pytest.raises(NativeError):
            run(case, entry, (0.5,) * max(nq, 1), raw_q=(raw, nq))
    check(case, (0.25,), run(case, entry, (0.25,)), entry)
