"""
The median kernels (auromat_amd/csrc/amt_median.hip) on constructed cells: the cases of tests/_median_cases.py go to
``amt_median_frame`` and ``amt_median_frame_async`` as plain device arrays, with coordinates that are the device's own bits,
and every cell of every output is compared with the oracle (np.median per cell), no cell left out.  What the cases aim at:
cell sizes at and around the tier boundaries (kSmallMax, kLargeMin, kChunk, kBlock), key patterns that decide the rank rule
(all equal, an equal or differing middle pair, a pair across a digit carry, negative elevations), 0..4 channels with and
without an elevation plane, three pixel orders of one frame, frames whose pixel count is no multiple of a lane's quad, the
membership rules on and next to every edge, a grid of more than 256 scan tiles, one cell of more than a million keys, and
one workspace reused by both entry points.  tests/test_median_cpu.py checks without a GPU that the cases hold these patterns.
"""
import ctypes as C

import numpy as np
import pytest

import _median_cases as K

pytestmark = pytest.mark.gpu

ENTRIES = ('amt_median_frame', 'amt_median_frame_async')
KEYS = ('median', 'img', 'mask', 'count')
POISON = 0xA5

_expected = {}


def expected(case):
    """The oracle's outputs of a case, computed once per module (the table: once per dtype, whatever the order)."""
    key = case.oracle_key
    if key not in _expected:
        _expected[key] = K.table_expected(*key[1:]) if key[0] == 'table' else K.expected(case)
    return _expected[key]


def run(case, entry):
    """Uploads a case, calls one entry point on outputs pre-filled with a poison byte, returns the outputs as host arrays."""
    import torch
    from auromat_amd._native import Context, ptr
    from auromat_amd.util.histogram import make_axis
    ctx = Context.current()
    ny, nx = case.shape
    nch = case.img.shape[1]
    u16 = case.img.dtype == np.uint16
    assert case.img.dtype in (np.uint8, np.uint16)
    xaxis, xkeep = make_axis(ctx, case.xedges, uniform=case.uniform)
    yaxis, ykeep = make_axis(ctx, case.yedges, uniform=case.uniform)
    assert xaxis.uniform == yaxis.uniform == int(case.uniform)
    lat, lon = ctx.to_device(case.lat), ctx.to_device(case.lon)
    elev = None if case.elev is None else ctx.to_device(case.elev)
    img = ctx.to_device(case.img, case.img.dtype) if nch else None
    mask = None if case.mask is None else ctx.to_device(case.mask, np.uint8)
    med = ctx.empty((ny, nx, nch + 1))
    out_img = ctx.empty((ny, nx, nch), torch.int16 if u16 else torch.uint8) if nch else None
    out_mask = ctx.empty((ny, nx), torch.uint8)
    count = ctx.empty((ny, nx))
    for t in (med, out_img, out_mask, count):
        if t is not None:
            t.view(torch.uint8).fill_(POISON)
    args = [ptr(lat), ptr(lon), ptr(elev), ptr(img), 2 if u16 else 1, nch, ptr(mask), case.height, case.width,
            float(case.min_elevation), C.byref(xaxis), C.byref(yaxis), case.lon_wrap]
    if entry == 'amt_median_frame_async':
        args.append(case.lon_from_mlt)
    else:
        assert entry == 'amt_median_frame' and not case.lon_from_mlt
    ctx.call(entry, *(args + [ptr(med), ptr(out_img), ptr(out_mask), ptr(count)]))
    torch.cuda.synchronize()
    got_img = np.zeros((ny, nx, 0), dtype=case.img.dtype)
    if nch:
        got_img = out_img.cpu().numpy().view(case.img.dtype)
    return dict(median=med.cpu().numpy(), img=got_img, mask=out_mask.cpu().numpy(), count=count.cpu().numpy())


def _first_difference(got, want, count, what, key, plane_names):
    """Fails with the first cell (output row, column), its count and tier, and the plane."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, key, got.shape, want.shape)
    if got.size == 0:
        return
    g = got.reshape(count.shape + (-1,))
    w = want.reshape(count.shape + (-1,))
    with np.errstate(invalid='ignore'):
        bad = ~((g == w) | ((g != g) & (w != w)))
    if not bad.any():
        return
    row, col, plane = [int(v[0]) for v in np.nonzero(bad)]
    n = int(count[row, col])
    raise AssertionError('%s: %s differs in %d cell-planes; first: output cell (%d, %d), plane %s, count %d (%s tier): '
                         'got %r, want %r' % (what, key, int(bad.sum()), row, col, plane_names[plane % len(plane_names)], n,
                                              K.TIERS[int(K.tier_of(n))] if n else 'empty', g[row, col, plane],
                                              w[row, col, plane]))


def check(case, got, what=''):
    """Every cell of every output against the oracle."""
    want = expected(case)
    what = '%s %s' % (case.name, what)
    nch = case.img.shape[1]
    planes = ['channel %d' % ch for ch in range(nch)] + ['elevation']
    count = want['count']
    _first_difference(got['count'], count, count, what, 'count', ['count'])
    _first_difference(got['mask'], (count == 0).astype(np.uint8), count, what, 'mask', ['mask'])
    _first_difference(got['median'], want['median'], count, what, 'median', planes)
    _first_difference(got['img'], want['img'], count, what, 'img', planes[:nch] or ['-'])
    assert np.array_equal(got['count'], count) and np.array_equal(got['mask'], count == 0), what
    assert np.array_equal(got['median'][..., :nch], want['median'][..., :nch], equal_nan=True), what
    assert np.array_equal(got['median'][..., nch], want['median'][..., nch], equal_nan=True), what
    assert np.isnan(got['median'][count == 0]).all() and (got['img'][count == 0] == 0).all(), what
    if case.elev is None:
        assert np.isnan(got['median'][..., nch]).all(), what
    assert got['img'].dtype == want['img'].dtype and np.array_equal(got['img'], want['img']), what


def same_bytes(a, b, what):
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


# ---- (a) the tier table ------------------------------------------------------------------------------------------------
TABLE_PLANES = [(np.uint8, 3, True), (np.uint16, 3, True), (np.uint8, 1, False), (np.uint16, 4, True), (np.uint8, 0, True),
                (np.uint16, 2, False), (np.uint8, 0, False)]
_table_ids = ['%s-%d-%s' % (np.dtype(d).name, n, 'elev' if e else 'noelev') for d, n, e in TABLE_PLANES]
_table_outputs = {}


def table_outputs(planes, order, entry):
    key = (np.dtype(planes[0]).name, planes[1], planes[2], order, entry)
    if key not in _table_outputs:
        _table_outputs[key] = run(K.tier_table(*planes, order=order), entry)
    return _table_outputs[key]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('order', K.ORDERS)
@pytest.mark.parametrize('planes', TABLE_PLANES, ids=_table_ids)
def test_tier_table(planes, order, entry):
    case = K.tier_table(*planes, order=order)
    assert case.height * case.width % 4 != 0
    check(case, table_outputs(planes, order, entry), entry)


@pytest.mark.parametrize('planes', TABLE_PLANES, ids=_table_ids)
def test_tier_table_same_bytes_in_every_order_from_both_entry_points(planes):
    first = table_outputs(planes, K.ORDERS[0], ENTRIES[0])
    for order in K.ORDERS:
        for entry in ENTRIES:
            same_bytes(table_outputs(planes, order, entry), first, (order, entry))


# ---- (b) membership ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('mode', ['nothreshold', 'threshold', 'nomask'])
@pytest.mark.parametrize('axis', ['uniform', 'nonuniform'])
def test_membership(axis, mode, dtype, entry):
    case = K.membership(dtype, axis, mode, 'plain')
    check(case, run(case, entry), entry)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('axis', ['uniform', 'nonuniform'])
def test_membership_lon_wrap(axis, dtype, entry):
    case = K.membership(dtype, axis, 'threshold', 'wrap')
    check(case, run(case, entry), entry)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('axis', ['uniform', 'nonuniform'])
def test_membership_lon_from_mlt(axis, dtype):
    case = K.membership(dtype, axis, 'threshold', 'mlt')
    check(case, run(case, 'amt_median_frame_async'), 'async')


# ---- (c) tails and tiny frames -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('size', K.TAIL_SIZES, ids=['%dx%d' % s for s in K.TAIL_SIZES])
def test_tails_and_tiny_frames(size, entry):
    for dtype in (np.uint8, np.uint16):
        for ncell in K.TAIL_CELLS:
            case = K.tails(dtype, size[0], size[1], ncell)
            check(case, run(case, entry), entry)


# ---- (d) a wide sparse grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_wide_sparse_grid(dtype, entry):
    case = K.sparse(dtype)
    check(case, run(case, entry), entry)


# ---- (e) one cell of more chunks than the large tier's grid has workgroups ----------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_one_large_cell(dtype, entry):
    case = K.one_large_cell(dtype)
    check(case, run(case, entry), entry)


# ---- one workspace, both entry points, frames that differ in large cells, planes and pixels ----------------------------
def test_workspace_reuse_across_entry_points():
    from auromat_amd._native import Context
    ctx = Context.current()
    steps = [('amt_median_frame_async', K.tier_table(np.uint16, 4, True, 'shuffled')),
             ('amt_median_frame', K.tails(np.uint16, 1, 3, 2)),
             ('amt_median_frame_async', K.sparse(np.uint8)),
             ('amt_median_frame', K.tier_table(np.uint8, 0, True, 'runs')),
             ('amt_median_frame_async', K.tier_table(np.uint16, 4, True, 'shuffled')),
             ('amt_median_frame', K.tier_table(np.uint16, 4, True, 'shuffled'))]
    outs = []
    for k, (entry, case) in enumerate(steps):
        assert Context.current() is ctx
        outs.append(run(case, entry))
        check(case, outs[-1], 'step %d %s' % (k, entry))
    same_bytes(outs[0], outs[4], 'first and fifth call')
    same_bytes(outs[0], outs[5], 'first and sixth call')
