"""
The plane form of the area-weighted binning (k_area_frame<..., PLANE = true> of auromat_amd/csrc/amt_area.hip behind
``amt_area_plane_frame``) on constructed frames of at most 20 x 20 pixels and grids of at most 64 x 64 cells, as plain device arrays.
The corner arrays are x and y of a plane.  The integer accumulators are compared with NumPy bit for bit first, then every output of
``amt_area_frame_finalize``: the weights are tests/_area_oracle.py's ``cell_weights`` (the twin of the kernel's cell_weight), the
candidate cells its ``candidate_ranges``, and the admission rule is stated in tests/_area_plane_oracle.py (``admitted``): a pixel takes part when its centre
value is finite, the elevation threshold holds, the mask is 0 and all eight corner values are finite — and, unlike
``amt_area_frame``, whatever its extent in x.  The one rule that differs is asserted both ways on a pixel 400 units wide.
"""
import ctypes as C

import numpy as np
import pytest

import _area_cases as K
import _area_oracle as O
from _area_plane_oracle import accumulate, admitted

pytestmark = pytest.mark.gpu

POISON = 0xA5
OUT_KEYS = ('area', 'img', 'mask', 'coverage')
EDOMAIN = -5


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def rect(xa, ya, xb, yb):
    return [(xa, ya), (xb, ya), (xb, yb), (xa, yb)]


def wide_case():
    """a pixel 400 units wide and two ordinary ones, on 64 x 8 cells of 10 units around 0"""
    return K.quads_frame('wide_400', [[(-203.0, 3.0), (197.0, 1.0), (199.0, 33.0), (-201.0, 31.0)], rect(-310.0, -30.0, -302.0, -21.0),
                                      rect(250.5, 10.5, 262.0, 22.0)], K.unit_edges(64, 10.0, -320.0), K.unit_edges(8, 10.0, -40.0))


def skip_case():
    """every admission rule once on a 6 x 8 lattice, and a pixel wider than 180 that stays"""
    h, w = 6, 8
    base = K.lattice('plane_rules', h, w, K.unit_edges(10, 0.5), K.unit_edges(8, 0.5), 0.1, 0.2, 0.55, 0.6, jitter=0.2, seed=51)
    y, x, c, elev = base.lat.copy(), base.lon.copy(), base.lat_c.copy(), np.full((h, w), 45.0)
    mask = np.zeros((h, w), dtype=np.uint8)
    c[0, 1], c[0, 3] = np.nan, np.inf
    elev[1, 2], elev[1, 4] = 9.999, np.nan
    mask[2, 5] = 1
    y[4, 1] = np.nan                # one NaN corner: its four pixels are dropped
    x[4, 6] = np.inf
    x[0, 8] = -179.0                # pixel (0, 7) becomes wider than 180: binned all the same
    return K.AreaCase('plane_rules', y, x, base.xedges, base.yedges, lat_c=c, elev=elev, mask=mask, min_elevation=10.0, seed=52)


def cases():
    e64 = K.unit_edges(64)
    out = [
        # one cell per pixel: 12 x 12 pixels of 2 units inside cells of 100
        K.lattice('one_cell', 12, 12, K.unit_edges(3, 100.0), K.unit_edges(3, 100.0), 110.0, 120.0, 2.0, 2.0, jitter=0.3, seed=71),
        # a few cells per pixel: pixels of 1.3 x 1.1 cells
        K.lattice('few_cells', 9, 11, K.unit_edges(16, 0.5, -1.0), K.unit_edges(14, 0.5, 2.0), -0.8, 2.3, 0.65, 0.55, jitter=0.3, seed=72),
        # more than 16 candidate cells (5 x 5) and more than 64 (9 x 9 and 60 x 60): the wave path; and both paths in one wave
        K.quads_frame('wave_path', [[(2.3, 2.6), (6.9, 2.2), (6.7, 6.8), (2.1, 6.4)], [(10.2, 10.6), (18.9, 10.1), (18.7, 18.8), (10.1, 18.4)],
                                    rect(30.25, 30.5, 30.75, 30.875), [(1.3, 1.6), (60.1, 2.2), (60.7, 61.4), (2.1, 60.8)]], e64, e64),
        wide_case(), skip_case(),
        # pixels over every border of the grid, and pixels wholly outside it
        K.lattice('borders', 12, 14, K.unit_edges(6, 0.5, 2.0), K.unit_edges(5, 0.5, 1.0), 0.3, -0.4, 0.45, 0.42, jitter=0.3, seed=61),
        # 20 x 20 pixels (two workgroups) with the coordinates 8 bytes off a 16-byte boundary, and the same aligned
        K.lattice('20x20_off1', 20, 20, K.unit_edges(24, 0.5, -1.0), K.unit_edges(20, 0.5, 2.0), -0.8, 2.3, 0.55, 0.45, jitter=0.3, seed=73,
                  coord_offset=1),
        K.lattice('20x20_off0', 20, 20, K.unit_edges(24, 0.5, -1.0), K.unit_edges(20, 0.5, 2.0), -0.8, 2.3, 0.55, 0.45, jitter=0.3, seed=73),
        K.lattice('1x19_off1', 1, 19, K.unit_edges(24, 0.5, -1.0), K.unit_edges(20, 0.5, 2.0), -0.8, 2.3, 0.55, 7.0, jitter=0.3, seed=74,
                  coord_offset=1),
    ]
    return out + K.format_cases()             # uint8 and uint16; 0, 1, 3 and 4 channels; no elevation; a mask


CASES = cases()


def test_the_cases_aim_where_they_claim():
    by = {c.name: c for c in CASES}
    for c in CASES:
        assert c.height <= 20 and c.width <= 20 and c.shape[0] <= 64 and c.shape[1] <= 64 and c.uniform, c.name
    count = lambda name: accumulate(by[name])[1]
    assert np.all(count('one_cell') == 1) and len(count('one_cell')) == 144
    few = count('few_cells')
    assert np.all(few >= 2) and np.all(few <= K.LANE_CELLS) and few.max() >= 6
    assert sorted(count('wave_path').tolist()) == [1, 25, 81, 61 * 60]
    assert count('wide_400').tolist() == [41 * 4, 1, 4]
    idx, X, _ = admitted(by['wide_400'])
    assert X[0].max() - X[0].min() > 400
    # the rules: 6 x 8 = 48 pixels; 2 centres, 2 elevations, 1 mask, 4 + 4 pixels around the two bad corners
    idx, X, _ = admitted(by['plane_rules'])
    assert len(idx) == 48 - 2 - 2 - 1 - 8 and 7 in idx.tolist() and (X[idx.tolist().index(7)].max() - X[idx.tolist().index(7)].min()) > 180
    # amt_area_frame's rules drop that pixel as well
    assert len(O.admitted(by['plane_rules'])[0]) == len(idx) - 1
    b = count('borders')
    assert (b == 0).sum() > 20 and (b > 0).sum() > 20
    formats = set((c.img.dtype.name, c.img.shape[1]) for c in CASES)
    assert formats == set((d, n) for d in ('uint8', 'uint16') for n in (0, 1, 3, 4))
    assert any(c.elev is None for c in CASES) and any(c.mask is not None for c in CASES)
    assert set(c.coord_offset for c in CASES) == {0, 1}


# ---- the device side -------------------------------------------------------------------------------------------------------------
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
    """A case in device memory, its coordinate arrays `coord_offset` doubles into their allocations."""

    def __init__(self, case):
        from auromat_amd._native import Context
        from auromat_amd.util.histogram import make_axis
        self.case, self.ctx = case, Context.current()
        self.nch = case.img.shape[1]
        self.code = 2 if case.img.dtype == np.uint16 else 1
        co = case.coord_offset
        self.y, self.x, self.c = (_device_array(v, co) for v in (case.lat, case.lon, case.lat_c))
        self.elev = None if case.elev is None else _device_array(case.elev, co)
        self.img = _device_array(case.img) if self.nch else None
        self.mask = None if case.mask is None else _device_array(case.mask.astype(np.uint8))
        assert self.x.data_ptr() % 16 == 8 * co and self.c.data_ptr() % 16 == 8 * co
        self.xaxis, self._xkeep = make_axis(self.ctx, case.xedges, uniform=True)
        self.yaxis, self._ykeep = make_axis(self.ctx, case.yedges, uniform=True)
        assert self.xaxis.uniform == self.yaxis.uniform == 1

    def new_acc(self):
        import torch
        ny, nx = self.case.shape
        return torch.zeros((self.nch + 2) * nx * ny, dtype=torch.int64, device=self.ctx.device)

    def add_to(self, acc, entry='amt_area_plane_frame'):
        """one call adding to `acc` -> its host planes (nch + 2, nx, ny)"""
        import torch
        from auromat_amd._native import ptr
        case = self.case
        ny, nx = case.shape
        args = [ptr(self.x), ptr(self.y)] if entry == 'amt_area_plane_frame' else [ptr(self.y), ptr(self.x)]
        args += [ptr(self.c), ptr(self.elev), ptr(self.img), self.code, self.nch, ptr(self.mask), case.height, case.width,
                 float(case.min_elevation), C.byref(self.xaxis), C.byref(self.yaxis)]
        if entry == 'amt_area_frame':
            args.append(0)                      # lon_wrap
        self.ctx.call(entry, *(args + [ptr(acc)]))
        torch.cuda.synchronize()
        return acc.cpu().numpy().reshape(self.nch + 2, nx, ny)


def finalize(ctx, acc, nx, ny, nch, dtype, least):
    """amt_area_frame_finalize on poisoned outputs -> (status, host arrays)"""
    import torch
    from auromat_amd._native import lib, ptr
    dtype = np.dtype(dtype)
    out = dict(area=ctx.empty((ny, nx, nch + 1)), img=ctx.empty((ny, nx, nch), torch.int16 if dtype == np.uint16 else torch.uint8),
               mask=ctx.empty((ny, nx), torch.uint8), coverage=ctx.empty((ny, nx)))
    for t in out.values():
        t.view(torch.uint8).fill_(POISON)
    rc = lib().amt_area_frame_finalize(ctx.handle, ptr(acc), nx, ny, nch, 2 if dtype == np.uint16 else 1, least, ptr(out['area']),
                                       ptr(out['img']) if nch else None, ptr(out['mask']), ptr(out['coverage']))
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got['img'] = got['img'].view(dtype)
    return rc, got


def same_planes(planes, want, what):
    for p in range(planes.shape[0]):
        bad = np.argwhere(planes[p] != want[p])
        assert len(bad) == 0, '%s: accumulator plane %d differs in %d cells, first (ix, iy) = %s: %d != %d' % (
            what, p, len(bad), tuple(bad[0]), planes[p][tuple(bad[0])], want[p][tuple(bad[0])])


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_case_equals_oracle(case):
    frame = Frame(case)
    acc = frame.new_acc()
    planes = frame.add_to(acc)
    want_acc, _ = accumulate(case)
    same_planes(planes, want_acc, case.name)
    ny, nx = case.shape
    for coverage in (0.5, 0.0):
        rc, got = finalize(frame.ctx, acc, nx, ny, frame.nch, case.img.dtype, O.min_weight(coverage))
        assert rc == 0
        want = O.finalize(want_acc, case.img.dtype, coverage)
        for key in OUT_KEYS:
            assert O.same_bits(got[key], want[key]), '%s, minCoverage %s: %s differs' % (case.name, coverage, key)


def test_wide_pixel_is_binned_here_and_dropped_by_the_frame_form():
    """The one rule that differs: on the same arrays ``amt_area_plane_frame`` bins the pixel 400 units wide and ``amt_area_frame``
    drops it (x extent >= 180); the two ordinary pixels are binned by both."""
    case = wide_case()
    frame = Frame(case)
    plane, sphere = frame.add_to(frame.new_acc()), frame.add_to(frame.new_acc(), 'amt_area_frame')
    want_plane, _ = accumulate(case)
    want_sphere, _ = O.accumulate(case)
    same_planes(plane, want_plane, 'plane form')
    same_planes(sphere, want_sphere, 'frame form')
    assert O.admitted(case)[3]['extent'] == 1
    # cells only the wide pixel reaches: columns 12 .. 51 (x in [-200, 200)) of rows 4 .. 6 (y in [0, 30))
    assert np.all(plane[0][13:51, 5] == 1 << 32) and np.all(sphere[0][12:52, 4:7] == 0)
    assert plane[0].sum() > sphere[0].sum() > 0


def test_two_calls_share_one_accumulator():
    a, b = Frame(CASES[5]), Frame(K.lattice('borders_2', 5, 9, K.unit_edges(6, 0.5, 2.0), K.unit_edges(5, 0.5, 1.0), 1.8, 0.9, 0.4, 0.5,
                                            jitter=0.2, seed=62))
    assert a.case.name == 'borders'
    acc = a.new_acc()
    first = a.add_to(acc).copy()
    both = b.add_to(acc)
    assert np.array_equal(both, first + accumulate(b.case)[0]) and not np.array_equal(both, first)
    assert np.array_equal(a.add_to(a.new_acc()), first)               # and two runs give the same bits


def ones_case(h, w, seed):
    """h x w pixels that are all the unit square of cell (0, 0): corner x alternates 0, 1 along a row, corner y down a column"""
    x = np.tile((np.arange(w + 1) % 2).astype(np.float64), (h + 1, 1))
    y = np.tile((np.arange(h + 1) % 2).astype(np.float64)[:, None], (1, w + 1))
    return K.AreaCase('ones_%dx%d' % (h, w), y, x, K.unit_edges(2), K.unit_edges(2), nch=1, seed=seed)


def test_coverage_limit():
    """16 x 16 unit squares over one cell: sum(W) = 2^40 passes; one pixel more, added by a second call, is AMT_EDOMAIN"""
    from auromat_amd._native import lib
    full, one = Frame(ones_case(16, 16, 1)), Frame(ones_case(1, 1, 2))
    acc = full.new_acc()
    planes = full.add_to(acc)
    want, _ = accumulate(full.case)
    same_planes(planes, want, 'limit')
    assert planes[0][0, 0] == 1 << 40 and planes[0].sum() == 1 << 40
    rc, got = finalize(full.ctx, acc, 2, 2, 1, np.uint8, O.min_weight(0.5))
    assert rc == 0
    ref = O.finalize(want, np.uint8, 0.5)
    for key in OUT_KEYS:
        assert O.same_bits(got[key], ref[key]), key
    planes = one.add_to(acc)
    assert planes[0][0, 0] == 257 << 32
    rc, _ = finalize(full.ctx, acc, 2, 2, 1, np.uint8, O.min_weight(0.5))
    assert rc == EDOMAIN and b'2^40' in lib().amt_last_error(full.ctx.handle)


def test_bad_arguments_are_refused():
    from auromat_amd._native import NativeError, ptr
    from auromat_amd.util.histogram import make_axis
    f = Frame(CASES[5])
    acc = f.new_acc()
    good = [ptr(f.x), ptr(f.y), ptr(f.c), None, ptr(f.img), 1, 3, None, 12, 14, float('-inf'), C.byref(f.xaxis), C.byref(f.yaxis), ptr(acc)]
    f.ctx.call('amt_area_plane_frame', *good)
    table, keep = make_axis(f.ctx, np.array([0.0, 1.0, 3.0, 4.0]), uniform=False)
    for i, v in ((0, None), (1, None), (2, None), (6, 5), (8, 0), (9, 0), (13, None), (4, None), (11, C.byref(table))):
        args = list(good)
        args[i] = v
        with pytest.raises(NativeError):
            f.ctx.call('amt_area_plane_frame', *args)
