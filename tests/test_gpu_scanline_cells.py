"""
The scan-line kernels (auromat_amd/csrc/amt_scanline.hip) on constructed inputs, through the C entry points: every output is
pre-filled with poison and EVERY element is compared with tests/_scanline_oracle.py (matplotlib's contains_points plus the
four-corner rule; a NumPy gather; later-frame-wins), bit for bit.  tests/test_scanline_cpu.py checks the oracle and the cases
without a GPU.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import _scanline_cases as K
import _scanline_oracle as O

pytestmark = pytest.mark.gpu

POISON = 0xA5
EINVAL, EDOMAIN = -1, -5
SELECT_CASES = K.select_cases()


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).to(_ctx().device)


def _poison(shape, dtype):
    """a device tensor whose every byte is POISON, and the same on the host"""
    import torch
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, POISON, dtype=np.uint8).view(dtype).reshape(shape)
    return _dev(host), host


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _select(case, polygon=None, window=None, rc_only=False, **override):
    ctx = _ctx()
    window = case.window if window is None else window
    polygon = case.polygon if polygon is None else polygon
    ny, nx = case.mask.shape
    rows, cols = window[2], window[3]
    keep, keep_poison = _poison((max(rows, 0), max(cols, 0)), np.uint8)
    stats, stats_poison = _poison((5,), np.int64)
    args = dict(lat=_dev(case.lat_axis), lon=_dev(case.lon_axis), ny=ny, nx=nx, poly=_dev(polygon) if len(polygon) else None,
                m=len(polygon), mask=_dev(case.mask), keep=keep, stats=stats)
    args.update(override)
    rc = ctx._lib.amt_scanline_select(ctx.handle, _p(args['lat']), _p(args['lon']), args['ny'], args['nx'], _p(args['poly']),
                                      args['m'], _p(args['mask']), window[0], window[1], rows, cols, _p(args['keep']),
                                      _p(args['stats']))
    ctx.synchronize()
    if rc_only:
        return rc, np.array_equal(_host(keep), keep_poison) and np.array_equal(_host(stats), stats_poison)
    assert rc == 0, rc
    return _host(keep), _host(stats)


@pytest.mark.parametrize('case', SELECT_CASES, ids=[c.name for c in SELECT_CASES])
def test_select_equals_contains_points_and_the_four_corner_rule(case):
    want_keep, want_stats = O.select(case.lat_axis, case.lon_axis, case.polygon, case.mask, case.window)
    keep, stats = _select(case)
    assert np.array_equal(keep, want_keep), np.argwhere(keep != want_keep)[:8]
    assert stats.tolist() == want_stats.tolist()
    if case.name in ('outside-window', 'outside-grid', 'two-vertices', 'no-vertices', 'one-cell-masked', 'empty-window'):
        assert stats[0] == 0
    elif case.name.endswith('masked') or case.name in ('odd-sizes', 'halves'):
        # the frame mask removes cells the polygon alone would keep
        free = O.select(case.lat_axis, case.lon_axis, case.polygon, np.zeros_like(case.mask), case.window)[1]
        assert 0 < stats[0] < free[0]
    else:
        assert stats[0] > 0


def test_select_refuses_bad_arguments_and_leaves_the_outputs():
    case = next(c for c in SELECT_CASES if c.name == 'odd-sizes')
    ny, nx = case.mask.shape
    for what, kw in (('lat', dict(lat=None)), ('lon', dict(lon=None)), ('mask', dict(mask=None)), ('keep', dict(keep=None)),
                     ('stats', dict(stats=None)), ('polygon', dict(poly=None)), ('ny', dict(ny=0)), ('nx', dict(nx=-3))):
        rc, untouched = _select(case, rc_only=True, **kw)
        assert rc == EINVAL and untouched, what
    for window in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, ny + 1, 4), (0, 0, 4, nx + 1), (ny - 2, 0, 3, 4), (0, nx - 2, 4, 3),
                   (0, 0, -1, 4)):
        rc, untouched = _select(case, window=window, rc_only=True)
        assert rc == EINVAL and untouched, window


def test_select_shares_the_arithmetic_of_points_in_polygon():
    """A strip polygon of scanline_strips (thousands of vertices with real coordinates) over a lattice of 1/36 degree: the
    corner test equals amt_points_in_polygon on the same lattice bit for bit, so the keep bytes equal the four-corner rule on
    ITS answers."""
    import torch
    import auromat_amd.resample as R
    ctx = _ctx()
    s = R.scanline_strips(K.props_along('equator', 4, step_deg=0.2), 1000.0)
    polygon = s['polygons'][1]                       # around lon 2.2: sides near lon 2.1 / 2.3, top edge near lat 10.6
    assert len(polygon) > 4000
    step = 1.0 / 36                                  # 0.0277... degrees
    lat_axis = 11.3 - step * np.arange(61)           # across the top edge
    lon_axis = 1.7 + step * np.arange(41)            # across both sides
    la, lo = np.meshgrid(lat_axis, lon_axis, indexing='ij')
    inside = torch.empty(la.shape, dtype=torch.uint8, device=ctx.device)
    d_la, d_lo, d_poly = _dev(la), _dev(lo), _dev(polygon)
    ctx.call('amt_points_in_polygon', _p(d_la), _p(d_lo), la.size, _p(d_poly), len(polygon), _p(inside))
    inside = _host(inside).astype(bool)
    assert 0.1 < inside.mean() < 0.9 and inside[:, 0].sum() == 0 and inside[0].sum() == 0
    mask = K._mask(60, 40, seed=2, density=0.1)
    case = K.SelectCase('strip', lat_axis, lon_axis, polygon, mask, (0, 0, 60, 40))
    want_keep, want_stats = O.select(lat_axis, lon_axis, polygon, mask, case.window, inside=inside)
    keep, stats = _select(case)
    assert np.array_equal(keep, want_keep) and stats.tolist() == want_stats.tolist() and stats[0] > 100
    # (matplotlib agrees on this lattice as well; it is not what pins the bits)
    assert np.array_equal(O.corners_inside(lat_axis, lon_axis, polygon), inside)


# ---- amt_scanline_pack -----------------------------------------------------------------------------------------------------------

def _pack(keep, window, planes, img, ny, nx, row_offset, col_offset, count, rc_only=False):
    ctx = _ctx()
    nplane, nchan = planes.shape[2], img.shape[2]
    dtype = img.dtype
    row, _ = _poison((count,), np.int32)
    col, _ = _poison((count,), np.int32)
    out_planes, _ = _poison((nplane, count), np.float64)
    out_img, _ = _poison((nchan, count), dtype)
    d_keep, d_planes, d_img = _dev(keep), _dev(planes), _dev(img)
    rc = ctx._lib.amt_scanline_pack(ctx.handle, _p(d_keep), window[0], window[1], window[2], window[3],
                                    _p(d_planes) if nplane else None, nplane, _p(d_img) if nchan else None,
                                    2 if dtype == np.uint16 else 1, nchan, ny, nx, row_offset, col_offset, count, _p(row), _p(col),
                                    _p(out_planes) if nplane else None, _p(out_img) if nchan else None)
    if rc_only:
        return rc
    assert rc == 0, rc
    return dict(row=_host(row), col=_host(col), planes=_host(out_planes), img=_host(out_img, dtype))


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('with_elev', [True, False], ids=['elev', 'noelev'])
@pytest.mark.parametrize('nchan', [0, 1, 3, 4])
def test_pack_equals_the_numpy_gather(nchan, with_elev, dtype):
    ny, nx = 37, 23
    planes, img = K.frame_data(ny, nx, nchan, with_elev, dtype, seed=nchan)
    for window, offsets, density in (((0, 0, ny, nx), (0, 0), 0.3), ((5, 3, 29, 17), (1000, -40), 0.5), ((36, 22, 1, 1), (7, 7), 1.1),
                                     ((2, 2, 20, 20), (0, 0), 0.0)):
        keep = (np.random.RandomState(5).random_sample((window[2], window[3])) < density).astype(np.uint8)
        count = int(keep.sum())
        assert (count == 0) == (density == 0.0)
        want = O.pack(keep, window, planes, img, *offsets)
        got = O.sort_records(_pack(keep, window, planes, img, ny, nx, offsets[0], offsets[1], count))
        for key in ('row', 'col', 'planes', 'img'):
            assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (key, window)
        pairs = set(zip(got['row'].tolist(), got['col'].tolist()))
        assert len(pairs) == count                                   # unique records


def test_pack_checks_the_count_and_its_arguments():
    ny, nx = 9, 9
    planes, img = K.frame_data(ny, nx, 3, True, np.uint8, 0)
    keep = np.ones((4, 4), np.uint8)
    assert _pack(keep, (1, 1, 4, 4), planes, img, ny, nx, 0, 0, 16, rc_only=True) == 0
    assert _pack(keep, (1, 1, 4, 4), planes, img, ny, nx, 0, 0, 15, rc_only=True) == EINVAL     # one record too many
    assert _pack(keep, (1, 1, 4, 4), planes, img, ny, nx, 0, 0, 17, rc_only=True) == EINVAL     # beyond the window's size
    assert _pack(keep, (6, 6, 4, 4), planes, img, ny, nx, 0, 0, 16, rc_only=True) == EINVAL     # window outside the grid
    five = np.zeros((ny, nx, 5), np.uint8)
    assert _pack(keep, (1, 1, 4, 4), planes, five, ny, nx, 0, 0, 16, rc_only=True) == EINVAL    # nchan 0..4


# ---- amt_scanline_compose --------------------------------------------------------------------------------------------------------

def _compose(strips, frames, row_base, col_base, NY, NX, nplane, nchan, dtype=np.uint8, want_rc=0):
    from auromat_amd._native import ScanLineStrip
    ctx = _ctx()
    table = (ScanLineStrip * max(len(strips), 1))()
    keep = []
    for t, s, k in zip(table, strips, frames):
        n = len(s['row'])
        dev = [_dev(s['row']), _dev(s['col']), _dev(s['planes']), _dev(s['img'])]
        keep.append(dev)
        if n:
            t.row, t.col = dev[0].data_ptr(), dev[1].data_ptr()
            t.planes = dev[2].data_ptr() if nplane else None
            t.img = dev[3].data_ptr() if nchan else None
        t.count, t.frame = n, k
    planes, _ = _poison((NY, NX, nplane), np.float64)
    img, _ = _poison((NY, NX, nchan), dtype)
    mask, _ = _poison((NY, NX), np.uint8)
    index, _ = _poison((NY, NX), np.int32)
    rc = ctx._lib.amt_scanline_compose(ctx.handle, table, len(strips), 2 if dtype == np.uint16 else 1, nchan, nplane, row_base,
                                       col_base, NY, NX, _p(planes) if nplane else None, _p(img) if nchan else None, _p(mask),
                                       _p(index))
    assert rc == want_rc, rc
    return _host(planes), _host(img, dtype), _host(mask), _host(index)


def _assert_composed(got, want):
    for name, g, w in zip(('planes', 'img', 'mask', 'frameIndex'), got, want[:4]):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=(name == 'planes')), name


@pytest.mark.parametrize('nchan', [0, 1, 2, 3, 4])
def test_compose_later_frame_wins_whatever_the_table_order(nchan):
    """Three overlapping strips, two identical strips, an empty strip, records on all four border cells: every assignment of
    frame indices to the strips (the table itself ascends, as the contract asks) against the NumPy oracle."""
    dtype = np.uint16 if nchan % 2 else np.uint8
    nplane = nchan + 1
    NY, NX, rb, cb = 21, 33, 500, -12
    cells = [K.block(rb, rb + 12, cb, cb + 20), K.block(rb + 6, rb + 21, cb + 10, cb + 33), K.block(rb + 3, rb + 15, cb + 5, cb + 25),
             K.block(rb + 3, rb + 15, cb + 5, cb + 25),                                  # identical to the one before
             (np.array([], int), np.array([], int)),                                     # no records
             (np.array([rb, rb, rb + 20, rb + 20, rb + 9]), np.array([cb, cb + 32, cb, cb + 32, cb + 3]))]     # the corners
    strips = [K.strip_records(r, c, nplane, nchan, dtype, seed=i) for i, (r, c) in enumerate(cells)]
    frames_sets = list(itertools.permutations(range(len(strips))))
    for frames in frames_sets[::37] + [tuple(range(len(strips)))[::-1]]:
        order = np.argsort(frames)
        table, ks = [strips[i] for i in order], [int(frames[i]) * 3 + 1 for i in order]           # (ascending, with gaps)
        want = O.compose(table, ks, rb, cb, NY, NX, nplane, nchan, dtype)
        assert not want[4] and (want[3] >= 0).sum() > 400 and (want[3] < 0).sum() > 20
        _assert_composed(_compose(table, ks, rb, cb, NY, NX, nplane, nchan, dtype), want)


def test_compose_one_strip_none_and_records_outside():
    r, c = K.block(3, 8, 2, 9)
    s = K.strip_records(r, c, 4, 3, np.uint8, seed=1)
    want = O.compose([s], [7], 3, 2, 5, 7, 4, 3)
    assert (want[3] == 7).all()
    _assert_composed(_compose([s], [7], 3, 2, 5, 7, 4, 3), want)                   # one strip that fills the raster
    _assert_composed(_compose([], [], 0, 0, 6, 5, 4, 3), O.compose([], [], 0, 0, 6, 5, 4, 3))       # none: all empty
    for row_base, col_base, NY, NX in ((4, 2, 5, 7), (3, 3, 5, 7), (3, 2, 4, 7), (3, 2, 5, 6)):      # one side short each
        want = O.compose([s], [0], row_base, col_base, NY, NX, 4, 3)
        assert want[4]
        # the error code; nothing is dropped silently, and the records inside are composed
        _assert_composed(_compose([s], [0], row_base, col_base, NY, NX, 4, 3, want_rc=EDOMAIN), want)
    # frame indices must ascend strictly and be >= 0
    for frames in ((1, 1), (2, 1), (-1, 0)):
        _compose([s, s], list(frames), 3, 2, 5, 7, 4, 3, want_rc=EINVAL)
