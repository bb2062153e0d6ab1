"""
The mean-binning kernels on constructed cells: k_bin_frame (auromat_amd/csrc/amt_bin_tile.h; alone and, windowed, as the
binning of a mosaic), k_bin_finalize, k_mosaic_select and k_hist2d.  The cases of tests/_bin_cases.py (and the membership,
tier-table, tail and large-cell cases of tests/_median_cases.py) go to ``amt_bin_frame`` + ``amt_bin_frame_finalize[_window]``,
``amt_mosaic_frames`` and ``amt_hist2d_accumulate`` + ``amt_hist2d_finalize_mean`` as plain device arrays; every cell of every
output is compared with tests/_bin_oracle.py, bit for bit.  The integer accumulators of ``amt_bin_frame`` are read back and
compared first, so a binning error and a finalise error are told apart.  Two tolerances exist, both derived in the oracle: the
device's mean elevation against the exact (Fraction) mean, 2**-33 + 2 spacing(|mean|), and the float histogram's sums of
real-valued weights, (n - 1) 2**-53 sum(|w|).  tests/test_bin_cases_cpu.py checks without a GPU that the cases aim where they
claim to: the global path of flush(), the borders of the LDS window, the anchor election, axes past 32 767 bins, the packed
image decode, misaligned arrays, tile tails, heavy cells, exact halves, select-tile borders, empty and many mosaic members.
"""
import ctypes as C

import numpy as np
import pytest

import _bin_cases as K
import _bin_oracle as B
import _median_cases as MC

pytestmark = pytest.mark.gpu

POISON = 0xA5
OUT_KEYS = ('mean', 'img', 'mask', 'count')
U8_U16 = pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])


# ---- device side -------------------------------------------------------------------------------------------------------------
def _device_array(a, offset=0):
    """A host array as a flat device tensor that starts `offset` elements into its allocation."""
    import torch
    from auromat_amd._native import Context
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    whole = torch.empty(a.size + 2 * offset + 2, dtype=torch.from_numpy(a[:0].copy()).dtype, device=Context.current().device)
    part = whole[offset:offset + a.size]
    part.copy_(torch.from_numpy(a.copy()))
    assert whole.data_ptr() % 16 == 0 and part.is_contiguous()
    return part


class Frame(object):
    """A case in device memory, laid out as the case asks (coord_offset, img_offset)."""

    def __init__(self, case):
        from auromat_amd._native import Context
        from auromat_amd.util.histogram import make_axis
        self.case, self.ctx = case, Context.current()
        self.nch = case.img.shape[1]
        assert case.img.dtype in (np.uint8, np.uint16) and not case.lon_from_mlt
        self.code = 2 if case.img.dtype == np.uint16 else 1
        co, io = getattr(case, 'coord_offset', 0), getattr(case, 'img_offset', 0)
        self.lat, self.lon = _device_array(case.lat, co), _device_array(case.lon, co)
        self.elev = None if case.elev is None else _device_array(case.elev, co)
        self.img = _device_array(case.img, io) if self.nch else None
        self.mask = None if case.mask is None else _device_array(case.mask.astype(np.uint8))
        assert self.lat.data_ptr() % 16 == 8 * co
        if self.nch:
            assert self.img.data_ptr() % 16 == io * case.img.dtype.itemsize
        self.xaxis, self._xkeep = make_axis(self.ctx, case.xedges, uniform=case.uniform)
        self.yaxis, self._ykeep = make_axis(self.ctx, case.yedges, uniform=case.uniform)
        assert self.xaxis.uniform == self.yaxis.uniform == int(case.uniform)

    def bin(self, acc=None):
        """amt_bin_frame into `acc` (a new zeroed accumulator unless given).  Returns the accumulator tensor."""
        import torch
        from auromat_amd._native import ptr
        case = self.case
        ny, nx = case.shape
        if acc is None:
            acc = torch.zeros((self.nch + 2) * nx * ny, dtype=torch.int64, device=self.ctx.device)
        self.ctx.call('amt_bin_frame', ptr(self.lat), ptr(self.lon), ptr(self.elev), ptr(self.img), self.code, self.nch,
                      ptr(self.mask), case.height, case.width, float(case.min_elevation), C.byref(self.xaxis),
                      C.byref(self.yaxis), case.lon_wrap, ptr(acc))
        return acc

    def member(self, window):
        from auromat_amd._native import MosaicMember
        m = MosaicMember()
        m.lat_c, m.lon_c = self.lat.data_ptr(), self.lon.data_ptr()
        m.elev = None if self.elev is None else self.elev.data_ptr()
        m.img = None if self.img is None else self.img.data_ptr()
        m.center_mask = None if self.mask is None else self.mask.data_ptr()
        m.height, m.width = self.case.height, self.case.width
        m.win_x0, m.win_y0, m.win_nx, m.win_ny = window
        return m


def _outputs(ctx, ny, nx, nch, dtype, source=False):
    import torch
    out = dict(mean=ctx.empty((ny, nx, nch + 1)), img=ctx.empty((ny, nx, nch), torch.int16 if dtype == np.uint16 else torch.uint8),
               mask=ctx.empty((ny, nx), torch.uint8), count=ctx.empty((ny, nx)))
    if source:
        out['source'] = ctx.empty((ny, nx), torch.int32)
    for t in out.values():
        t.view(torch.uint8).fill_(POISON)
    return out


def _host(out, dtype):
    import torch
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got['img'] = got['img'].view(dtype)
    return got


def finalize(ctx, acc, acc_nx, acc_ny, nch, dtype, window=None):
    """amt_bin_frame_finalize (window None) or amt_bin_frame_finalize_window on poisoned outputs -> host arrays."""
    from auromat_amd._native import ptr
    dtype = np.dtype(dtype)
    code = 2 if dtype == np.uint16 else 1
    x0, y0, nx, ny = window or (0, 0, acc_nx, acc_ny)
    out = _outputs(ctx, ny, nx, nch, dtype)
    tail = [nch, code, ptr(out['mean']), ptr(out['img']) if nch else None, ptr(out['mask']), ptr(out['count'])]
    if window is None:
        ctx.call('amt_bin_frame_finalize', ptr(acc), nx, ny, *tail)
    else:
        ctx.call('amt_bin_frame_finalize_window', ptr(acc), acc_nx, acc_ny, x0, y0, nx, ny, *tail)
    return _host(out, dtype)


def acc_planes(acc, nx, ny, nch):
    """The accumulator (count, channel sums, fixed-point elevation; cell ix * ny + iy) as integer planes in the output layout."""
    import torch
    torch.cuda.synchronize()
    a = acc.cpu().numpy().reshape(nch + 2, nx, ny)
    lay = lambda p: np.flipud(p.T)
    return dict(count=lay(a[0]), sums=np.stack([lay(a[1 + k]) for k in range(nch)], axis=2) if nch else
                np.zeros((ny, nx, 0), dtype=np.int64), fx=lay(a[nch + 1]))


def run_mosaic(mosaic, rule, frames=None):
    from auromat_amd._native import Context, MosaicMember, ptr
    ctx = Context.current()
    frames = frames or [Frame(c) for c in mosaic.members]
    first = mosaic.members[0]
    ny, nx = mosaic.shape
    nch, dtype = first.img.shape[1], first.img.dtype
    table = (MosaicMember * len(frames))(*[f.member(w) for f, w in zip(frames, mosaic.windows)])
    out = _outputs(ctx, ny, nx, nch, dtype, source=True)
    ctx.call('amt_mosaic_frames', table, len(frames), frames[0].code, nch, float(first.min_elevation), C.byref(frames[0].xaxis),
             C.byref(frames[0].yaxis), first.lon_wrap, rule, ptr(out['mean']), ptr(out['img']) if nch else None,
             ptr(out['mask']), ptr(out['count']), ptr(out['source']))
    return _host(out, dtype)


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def _where(cases, windows, row, col):
    """From the CPU model: how the pixels of output cell (row, col) reach the accumulators."""
    parts = []
    for m, (case, window) in enumerate(zip(cases, windows)):
        ny, nx = case.shape
        here = B.cells(case, window) == row * nx + col
        path = K.paths(case, window)['path'][here]
        parts.append('%s%d pixels: %d through LDS, %d by the global path' % (
            'member %d ' % m if len(cases) > 1 else '', int(here.sum()), int((path == 1).sum()), int((path == 2).sum())))
    return '; '.join(parts)


def _same(got, want, count, what, key, plane_names, cases, windows, offset=(0, 0)):
    """Fails with the case, the first differing output cell, its count, the plane and the cell's paths."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, key, got.shape, want.shape, got.dtype, want.dtype)
    if got.size == 0:
        return
    g, w = got.reshape(count.shape + (-1,)), want.reshape(count.shape + (-1,))
    with np.errstate(invalid='ignore'):
        bad = ~((g == w) | ((g != g) & (w != w)))
    if bad.any():
        row, col, plane = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError('%s: %s differs in %d cell-planes; first: output cell (%d, %d), plane %s, count %d: got %r, want %r '
                             '[%s]' % (what, key, int(bad.sum()), row, col, plane_names[plane % len(plane_names)],
                                       int(count[row, col]), g[row, col, plane], w[row, col, plane],
                                       _where(cases, windows, row + offset[0], col + offset[1])))
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'), (what, key)


def check_outputs(got, want, what, cases, windows, offset=(0, 0)):
    """mean, img, mask, count (and source) of every cell against the oracle's finalised dict."""
    nch = want['sums'].shape[2]
    planes = ['channel %d' % ch for ch in range(nch)] + ['elevation']
    count = want['count']
    args = (cases, windows, offset)
    _same(got['count'], want['count_f'], count, what, 'count', ['count'], *args)
    _same(got['mask'], want['mask'], count, what, 'mask', ['mask'], *args)
    _same(got['mean'], want['mean'], count, what, 'mean', planes, *args)
    _same(got['img'], want['img'], count, what, 'img', planes[:nch] or ['-'], *args)
    if 'source' in want:
        _same(got['source'], want['source'], count, what, 'source', ['source'], *args)
    assert np.isnan(got['mean'][count == 0]).all() and (got['img'][count == 0] == 0).all(), what


def check_integers(got, want, what, cases, windows):
    count = want['count']
    nch = want['sums'].shape[2]
    _same(got['count'], want['count'], count, what, 'accumulated count', ['count'], cases, windows)
    _same(got['sums'], want['sums'], count, what, 'accumulated channel sum', ['channel %d' % ch for ch in range(nch)] or ['-'],
          cases, windows)
    _same(got['fx'], want['fx'], count, what, 'accumulated fixed-point elevation', ['elevation'], cases, windows)


_exact = {}


def check_exact_mean(key, flat, elev, got_elevation, what):
    """The second reference: the device's mean elevation within the derived bound of the exact (Fraction) mean."""
    if key not in _exact:
        _exact[key] = B.exact_means(flat, elev)
    worst, cell = B.worst_exact_error(_exact[key], got_elevation)
    assert worst <= 1.0, '%s: mean elevation of output cell %d is %.3f of the derived bound from the exact mean' % (what, cell, worst)


def same_bytes(a, b, what, keys=OUT_KEYS):
    for key in keys:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


_oracle = {}


def oracle(case):
    if case.oracle_key not in _oracle:
        _oracle[case.oracle_key] = B.frame(case)
    return _oracle[case.oracle_key]


def run_frame(case, exact_key=None):
    """Bins and finalises a case twice on one upload: accumulators, then outputs, against the oracle; same bytes both times.
    Returns (Frame, outputs)."""
    frame = Frame(case)
    ny, nx = case.shape
    want = oracle(case)
    outs = []
    for k in range(2):
        acc = frame.bin()
        check_integers(acc_planes(acc, nx, ny, frame.nch), want, '%s run %d' % (case.name, k), [case], [None])
        outs.append(finalize(frame.ctx, acc, nx, ny, frame.nch, case.img.dtype))
        check_outputs(outs[-1], want, '%s run %d' % (case.name, k), [case], [None])
    same_bytes(outs[0], outs[1], case.name + ': two runs')
    if case.elev is not None:
        check_exact_mean(exact_key or case.oracle_key, case.flat(), case.elev, outs[0]['mean'][..., -1], case.name)
    else:
        assert (outs[0]['mean'][..., -1][want['count'] > 0] == 0.0).all()
    return frame, outs[0]


def check_alone_equals_mosaic_member(case, frame, alone):
    """The frame as the only member of a mosaic with a full window: the same bytes as binned alone (both rules)."""
    ny, nx = case.shape
    m = K.Mosaic(case.name + '-as-mosaic', [case], [(0, 0, nx, ny)])
    for rule in ((0, 1) if case.elev is not None else (0,)):
        got = run_mosaic(m, rule, frames=[frame])
        same_bytes(alone, got, '%s alone and as a mosaic member, rule %d' % (case.name, rule))
        assert np.array_equal(got['source'], np.where(oracle(case)['count'] > 0, 0, -1))


# ---- the median cases, with the mean as the expected statistic -------------------------------------------------------------------
@U8_U16
@pytest.mark.parametrize('mode', ['nothreshold', 'threshold', 'nomask'])
@pytest.mark.parametrize('axis', ['uniform', 'nonuniform'])
def test_membership(axis, mode, dtype):
    run_frame(K.as_bin_case(MC.membership(dtype, axis, mode, 'plain')))


@U8_U16
@pytest.mark.parametrize('axis', ['uniform', 'nonuniform'])
def test_membership_lon_wrap(axis, dtype):
    run_frame(K.as_bin_case(MC.membership(dtype, axis, 'threshold', 'wrap')))


TABLE_PLANES = [(np.uint8, 3, True), (np.uint16, 3, True), (np.uint8, 1, False), (np.uint16, 4, True), (np.uint8, 0, True),
                (np.uint16, 2, False), (np.uint8, 0, False)]


@pytest.mark.parametrize('order', MC.ORDERS)
@pytest.mark.parametrize('planes', TABLE_PLANES, ids=['%s-%d-%s' % (np.dtype(d).name, n, 'elev' if e else 'noelev')
                                                      for d, n, e in TABLE_PLANES])
def test_tier_table(planes, order):
    case = K.as_bin_case(MC.tier_table(*planes, order=order))
    # (one oracle per planes and the exact means once per type, whatever the order: a cell's pixels are the same set)
    run_frame(case, exact_key=('table-exact', np.dtype(planes[0]).name))


@pytest.mark.parametrize('size', MC.TAIL_SIZES, ids=['%dx%d' % s for s in MC.TAIL_SIZES])
def test_tails_and_tiny_frames(size):
    for dtype in (np.uint8, np.uint16):
        for ncell in MC.TAIL_CELLS:
            run_frame(K.as_bin_case(MC.tails(dtype, size[0], size[1], ncell)))


@U8_U16
def test_one_large_cell(dtype):
    run_frame(K.as_bin_case(MC.one_large_cell(dtype)))


# ---- the global path, the window's borders, the election, long axes ---------------------------------------------------------------
@U8_U16
@pytest.mark.parametrize('variant', K.SCATTER_VARIANTS)
def test_scatter(variant, dtype):
    case = K.scatter(dtype, variant)
    frame, out = run_frame(case)
    check_alone_equals_mosaic_member(case, frame, out)


@pytest.mark.parametrize('nch', [0, 1, 2, 4])
def test_scatter_channel_counts(nch):
    run_frame(K.scatter(np.uint16 if nch % 2 else np.uint8, 'plain', nch))


@pytest.mark.parametrize('kind', sorted(K.WINDOW_BORDER))
def test_window_border(kind):
    run_frame(K.window_border(kind, np.uint8, 1))
    case = K.window_border(kind, np.uint16, 3)
    frame, out = run_frame(case)
    check_alone_equals_mosaic_member(case, frame, out)      # the same offsets through the windowed kernel's two flushes


@pytest.mark.parametrize('nx,ny', K.WIDE_AXES)
def test_wide_axis(nx, ny):
    run_frame(K.wide_axis(nx, ny))


def test_wide_axis_as_mosaic_member():
    case = K.wide_axis(65534, 3, np.uint16, 1)
    frame, out = run_frame(case)
    check_alone_equals_mosaic_member(case, frame, out)


@U8_U16
def test_late_anchor(dtype):
    case = K.late_anchor(dtype, 2)
    frame, out = run_frame(case)
    check_alone_equals_mosaic_member(case, frame, out)


# ---- tile tails, array alignment, the packed decode --------------------------------------------------------------------------------
# (an odd width takes the scalar path whatever the addresses: the other layouts go with the even widths)
@pytest.mark.parametrize('width,layout', [(w, l) for w in K.SIZE_WIDTHS for l in K.SIZE_LAYOUTS if l == 'aligned' or w % 2 == 0],
                         ids=lambda v: str(v))
def test_sizes(width, layout):
    for height in K.SIZE_HEIGHTS:
        case = K.sizes(height, width, layout)
        frame, out = run_frame(case)
        if layout == 'img1':
            check_alone_equals_mosaic_member(case, frame, out)      # amt_mosaic_frames decides by the image base as well


@U8_U16
@pytest.mark.parametrize('nch', range(5))
def test_channels(dtype, nch):
    for width in K.CHANNEL_WIDTHS:
        case = K.channels(dtype, nch, width)
        frame, out = run_frame(case)
        check_alone_equals_mosaic_member(case, frame, out)


# ---- heavy cells, halves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('split', [False, True], ids=['one-cell', 'two-cells'])
@pytest.mark.parametrize('kind', K.HEAVY_KINDS)
def test_heavy_cell(kind, split):
    case = K.heavy_cell(kind, split)
    frame, out = run_frame(case)
    check_alone_equals_mosaic_member(case, frame, out)
    if kind == 'elev-low':
        assert (oracle(case)['fx'] < -2 ** 59).all()          # far past 2**32, negative


@U8_U16
def test_half_means(dtype):
    case = K.half_means(dtype)
    _, out = run_frame(case)
    ks = case.promises()['ks']
    # half to even, spelled out: 0.5 -> 0, 1.5 -> 2, 254.5 -> 254, 65 534.5 -> 65 534 (cells of two pixels come first, then four)
    assert out['img'][0, 0:2 * len(ks):2, 0].tolist() == [k + k % 2 for k in ks]
    assert out['img'][0, 1:2 * len(ks):2, 0].tolist() == [k + k % 2 for k in ks]
    hi = int(np.iinfo(dtype).max)
    assert out['img'][0, 0, 1] == hi - 1 and out['mean'][0, 0, 1] == hi - 0.5          # 254.5 -> 254, 65 534.5 -> 65 534
    assert out['img'][0, 2 * len(ks), 0] == hi and out['mean'][0, 2 * len(ks), 0] == float(hi)


# ---- amt_bin_frame_finalize_window; amt_bin_frame adds ---------------------------------------------------------------------------------
@U8_U16
def test_finalize_window_and_accumulation(dtype):
    case = K.finalize_window(dtype)
    frame, whole = run_frame(case)
    acc_nx, acc_ny = K.FINALIZE_ACC
    x0, y0, nx, ny = window = K.FINALIZE_WINDOW
    want = oracle(case)
    cropped = {k: K.crop(v, window, acc_ny) for k, v in want.items()}
    offset = (acc_ny - y0 - ny, x0)
    acc = frame.bin()
    got = finalize(frame.ctx, acc, acc_nx, acc_ny, frame.nch, dtype, window)
    assert got['count'].shape == (ny, nx)
    check_outputs(got, cropped, case.name + ' through the window', [case], [None], offset)
    same_bytes(got, {k: np.ascontiguousarray(K.crop(whole[k], window, acc_ny)) for k in OUT_KEYS}, 'window and crop')
    # the finalise step only reads: the accumulators are as they were; a second frame adds to them
    check_integers(acc_planes(acc, acc_nx, acc_ny, frame.nch), want, case.name + ' after the finalise', [case], [None])
    assert frame.bin(acc) is acc
    twice = {k: 2 * want[k] for k in ('count', 'sums', 'fx')}
    check_integers(acc_planes(acc, acc_nx, acc_ny, frame.nch), twice, case.name + ' binned twice', [case], [None])
    doubled = finalize(frame.ctx, acc, acc_nx, acc_ny, frame.nch, dtype)
    assert np.array_equal(doubled['count'], 2 * whole['count'])
    same_bytes(doubled, whole, 'binned twice: no mean moves', ('mean', 'img', 'mask'))
    check_outputs(finalize(frame.ctx, acc, acc_nx, acc_ny, frame.nch, dtype, window), B.finalize(
        {k: K.crop(v, window, acc_ny) for k, v in twice.items()}, dtype), case.name + ' twice, window', [case], [None], offset)


# ---- mosaics -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_elevation', [-np.inf, 'threshold'], ids=['nothreshold', 'threshold'])
@pytest.mark.parametrize('nch', [0, 3])
@U8_U16
@pytest.mark.parametrize('rule', [0, 1])
@pytest.mark.parametrize('name', sorted(K.MOSAIC_CASES))
def test_mosaic(name, rule, dtype, nch, min_elevation):
    if min_elevation == 'threshold':
        min_elevation = K.TIES_THRESHOLD if name == 'ties' else 0.0
    m = K.MOSAIC_CASES[name](dtype, nch, min_elevation)
    want = B.mosaic(m.members, m.windows, rule)
    what = '%s rule %d min_elevation %s' % (m.name, rule, min_elevation)
    frames = [Frame(c) for c in m.members]
    got = run_mosaic(m, rule, frames)
    check_outputs(got, want, what, m.members, m.windows)
    same_bytes(got, run_mosaic(m, rule, frames), what + ': two runs', OUT_KEYS + ('source',))
    if name == 'ties' and rule == 1:
        assert got['source'].tolist() == [list(K.TIES_WINNERS)]
    # the exact mean of what the rule selects: the union's pixels, or the winner's
    n = len(m.members)
    flats = [B.cells(c, w) for c, w in zip(m.members, m.windows)]
    if rule == 1:
        flats = [np.where(want['source'].ravel()[np.maximum(f, 0)] == k, f, -1) for k, f in enumerate(flats)]
    means = B.exact_means(np.concatenate(flats), np.concatenate([c.elev for c in m.members]))
    worst, cell = B.worst_exact_error(means, got['mean'][..., -1])
    assert worst <= 1.0, (what, cell, worst)
    # the members in reverse order
    r = m.reversed()
    back = run_mosaic(r, rule, frames[::-1])
    check_outputs(back, B.mosaic(r.members, r.windows, rule), what + ' reversed', r.members, r.windows)
    if rule == 0:
        same_bytes(got, back, what + ': reversed members')
    elif name != 'ties':
        same_bytes(got, back, what + ': reversed members')
        assert np.array_equal(back['source'], np.where(got['source'] >= 0, n - 1 - got['source'], -1))


# ---- the float histogram -------------------------------------------------------------------------------------------------------------------
def _hist(h):
    import torch
    from auromat_amd._native import Context, ptr
    from auromat_amd.util.histogram import make_axis
    ctx = Context.current()
    nx, ny = len(h['xedges']) - 1, len(h['yedges']) - 1
    k = len(h['weights'])
    xaxis, _xk = make_axis(ctx, h['xedges'])
    yaxis, _yk = make_axis(ctx, h['yedges'])
    x, y = ctx.to_device(h['x']), ctx.to_device(h['y'])
    wdev = [ctx.to_device(w) for w in h['weights']]
    count, sums = ctx.zeros((nx * ny,)), [ctx.zeros((nx * ny,)) for _ in wdev]
    wptr = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in wdev])
    sptr = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in sums])
    ctx.call('amt_hist2d_accumulate', ptr(x) if len(h['x']) else None, ptr(y) if len(h['x']) else None, len(h['x']), wptr, k,
             C.byref(xaxis), C.byref(yaxis), 0, ptr(count), sptr)
    mean = ctx.empty((ny * nx * max(k, 1),))                # (never an empty allocation: the entry point refuses NULL)
    mean.view(torch.uint8).fill_(POISON)
    ctx.call('amt_hist2d_finalize_mean', ptr(count), sptr, k, nx, ny, ptr(mean))
    torch.cuda.synchronize()
    return count.cpu().numpy(), [s.cpu().numpy() for s in sums], mean.cpu().numpy()[:ny * nx * k].reshape(ny, nx, k)


@pytest.mark.parametrize('kind', ['integer', 'real'])
@pytest.mark.parametrize('nweights', [0, 1, 8])
def test_hist_points(nweights, kind):
    h = K.hist_points(nweights, kind)
    nx, ny = K.HIST_GRID
    want_count, want = B.hist2d(h['x'], h['y'], h['weights'], h['xedges'], h['yedges'])
    count, sums, mean = _hist(h)
    assert np.array_equal(count, want_count) and count.sum() > 256 * 16 * 256
    assert mean.shape == (ny, nx, nweights)
    for k, (s, bound) in enumerate(want):
        err = np.abs(sums[k] - s)
        assert (err <= bound).all(), (kind, k, int(np.argmax(err - bound)), float((err - bound).max()))
        if kind == 'integer':
            assert np.array_equal(sums[k], s)
        # the mean is one division of the device's own sum by its count, in the output layout
        with np.errstate(invalid='ignore', divide='ignore'):
            assert np.array_equal(mean[..., k], B.hist_layout(np.where(count > 0, sums[k] / count, np.nan), nx, ny), equal_nan=True)


def test_hist_no_points():
    h = K.hist_points(2, 'real', n=0)
    count, sums, mean = _hist(h)
    assert not count.any() and not any(s.any() for s in sums) and np.isnan(mean).all()
