"""
The area-weighted binning kernels (k_area_frame, k_area_finalize of auromat_amd/csrc/amt_area.hip) on constructed cells: the
cases of tests/_area_cases.py go to ``amt_area_frame`` + ``amt_area_frame_finalize`` as plain device arrays.  The integer
accumulators are read back and compared with tests/_area_oracle.py bit for bit first, then every finalised output (area, img,
mask, coverage), so a geometry error and a finalise error are told apart.  There is no tolerance anywhere: the oracle restates
the kernel's arithmetic operation for operation.  tests/test_area_cpu.py checks without a GPU that the oracle gives the exact
answers on dyadic coordinates and that the cases aim where they claim to (one cell, a few cells, the wave-cooperative path, the
skip rules, the borders of the grid, the coverage limit).
"""
import ctypes as C

import numpy as np
import pytest

import _area_cases as K
import _area_oracle as O

pytestmark = pytest.mark.gpu

POISON = 0xA5
OUT_KEYS = ('area', 'img', 'mask', 'coverage')
EDOMAIN = -5


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
        self.lat, self.lon, self.lat_c = (_device_array(v, co) for v in (case.lat, case.lon, case.lat_c))
        self.elev = None if case.elev is None else _device_array(case.elev, co)
        self.img = _device_array(case.img) if self.nch else None
        self.mask = None if case.mask is None else _device_array(case.mask.astype(np.uint8))
        assert self.lat.data_ptr() % 16 == 8 * co and self.lat_c.data_ptr() % 16 == 8 * co
        self.xaxis, self._xkeep = make_axis(self.ctx, case.xedges, uniform=case.uniform)
        self.yaxis, self._ykeep = make_axis(self.ctx, case.yedges, uniform=case.uniform)
        assert self.xaxis.uniform == self.yaxis.uniform == int(case.uniform)

    def accumulate(self):
        """amt_area_frame into a new zeroed accumulator -> (device tensor, host planes (nch + 2, nx, ny))."""
        import torch
        from auromat_amd._native import ptr
        case = self.case
        ny, nx = case.shape
        acc = torch.zeros((self.nch + 2) * nx * ny, dtype=torch.int64, device=self.ctx.device)
        self.ctx.call('amt_area_frame', ptr(self.lat), ptr(self.lon), ptr(self.lat_c), ptr(self.elev), ptr(self.img),
                      self.code, self.nch, ptr(self.mask), case.height, case.width, float(case.min_elevation),
                      C.byref(self.xaxis), C.byref(self.yaxis), case.lon_wrap, ptr(acc))
        torch.cuda.synchronize()
        return acc, acc.cpu().numpy().reshape(self.nch + 2, nx, ny)


def finalize(ctx, acc, nx, ny, nch, dtype, least):
    """amt_area_frame_finalize on poisoned outputs -> (status, host arrays)."""
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


def check_outputs(got, want, what):
    for key in OUT_KEYS:
        assert O.same_bits(got[key], want[key]), '%s: %s differs' % (what, key)


@pytest.mark.parametrize('case', K.device_cases(), ids=repr)
def test_case_equals_oracle(case):
    frame = Frame(case)
    acc, planes = frame.accumulate()
    want_acc, _ = O.accumulate(case)
    for p in range(planes.shape[0]):
        bad = np.argwhere(planes[p] != want_acc[p])
        assert len(bad) == 0, '%s: accumulator plane %d differs in %d cells, first (ix, iy) = %s: %d != %d' % (
            case.name, p, len(bad), tuple(bad[0]), planes[p][tuple(bad[0])], want_acc[p][tuple(bad[0])])
    ny, nx = case.shape
    for coverage in (0.5, 0.0):
        rc, got = finalize(frame.ctx, acc, nx, ny, frame.nch, case.img.dtype, O.min_weight(coverage))
        assert rc == 0
        check_outputs(got, O.finalize(want_acc, case.img.dtype, coverage), '%s, minCoverage %s' % (case.name, coverage))


def test_two_runs_give_the_same_bits():
    frame = Frame(K.alternating_case())
    assert np.array_equal(frame.accumulate()[1], frame.accumulate()[1])


def test_accumulators_are_added_to():
    """The call adds to what the accumulator holds: two frames binned into one equal the sum of their own."""
    a, b = Frame(K.outside_case()), Frame(K.lattice('outside_2', 5, 9, K.unit_edges(6, 0.5, 2.0), K.unit_edges(5, 0.5, 1.0), 1.8, 0.9,
                                                      0.4, 0.5, jitter=0.2, seed=62))
    import torch
    from auromat_amd._native import ptr
    acc, first = a.accumulate()
    first = first.copy()
    b.ctx.call('amt_area_frame', ptr(b.lat), ptr(b.lon), ptr(b.lat_c), ptr(b.elev), ptr(b.img), b.code, b.nch, None,
               b.case.height, b.case.width, float('-inf'), C.byref(b.xaxis), C.byref(b.yaxis), 0, ptr(acc))
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy().reshape(first.shape), first + O.accumulate(b.case)[0])


@pytest.mark.parametrize('coverage', [0.0, 0.5, 1.0])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_threshold_cells(coverage, dtype):
    """Cells with a total weight exactly at, one below and one above the threshold, on hand-made accumulators (with channel sums
    whose means are exact halves: the image rounds half to even)."""
    import torch
    from auromat_amd._native import Context
    ctx = Context.current()
    least = O.min_weight(coverage)
    assert least == {0.0: 1, 0.5: 1 << 31, 1.0: 1 << 32}[coverage]
    nx, ny, nch = 3, 2, 2
    acc = np.zeros((nch + 2, nx, ny), dtype=np.int64)
    acc[0, :, 0] = (least - 1, least, least + 1)
    acc[0, :, 1] = (0, 2, 1 << 33)
    top = int(np.iinfo(dtype).max)
    acc[1] = acc[0] * top                           # the largest value: the mean is exactly `top`
    acc[2] = acc[0] // 2 * 5                        # 2.5 where the weight is even: rounds to 2
    acc[3] = -acc[0] * 3 * 65536 // 2               # elevation -1.5 deg
    dev = torch.from_numpy(acc.reshape(-1).copy()).to(ctx.device)
    rc, got = finalize(ctx, dev, nx, ny, nch, dtype, least)
    assert rc == 0
    want = O.finalize(acc, dtype, least=least)
    assert want['mask'][1].tolist() == [1, 0, 0]    # row 1 = iy 0: below, at, above
    check_outputs(got, want, 'threshold %s' % coverage)
    # a minimum weight of 0 is the rule's floor of 1: an empty cell is never valid
    rc, got = finalize(ctx, dev, nx, ny, nch, dtype, 0)
    assert rc == 0
    check_outputs(got, O.finalize(acc, dtype, least=1), 'least 0')


@pytest.mark.parametrize('n,status', [(256, 0), (257, EDOMAIN)])
def test_coverage_limit(n, status):
    """n unit squares over one cell: sum(W) = n 2^32.  2^40 passes, one pixel more is AMT_EDOMAIN."""
    case = K.coverage_limit_case(n)
    frame = Frame(case)
    acc, planes = frame.accumulate()
    want_acc, _ = O.accumulate(case)
    assert np.array_equal(planes, want_acc) and planes[0][0, 0] == n << 32
    rc, got = finalize(frame.ctx, acc, 2, 2, 1, np.uint8, O.min_weight(0.5))
    assert rc == status
    if status == 0:
        check_outputs(got, O.finalize(want_acc, np.uint8, 0.5), case.name)
    else:
        from auromat_amd._native import lib
        assert b'2^40' in lib().amt_last_error(frame.ctx.handle)


def test_bad_arguments_are_refused():
    from auromat_amd._native import NativeError, ptr
    frame = Frame(K.outside_case())
    acc, _ = frame.accumulate()
    for nch, height in ((5, 12), (3, 0)):
        with pytest.raises(NativeError):
            frame.ctx.call('amt_area_frame', ptr(frame.lat), ptr(frame.lon), ptr(frame.lat_c), None, ptr(frame.img), 1, nch, None,
                           height, 14, float('-inf'), C.byref(frame.xaxis), C.byref(frame.yaxis), 0, ptr(acc))
    with pytest.raises(NativeError):
        frame.ctx.call('amt_area_frame', None, ptr(frame.lon), ptr(frame.lat_c), None, ptr(frame.img), 1, 3, None, 12, 14,
                       float('-inf'), C.byref(frame.xaxis), C.byref(frame.yaxis), 0, ptr(acc))
