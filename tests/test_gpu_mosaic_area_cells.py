"""
The area-weighted mosaic kernels (k_area_frame<..., WIN = true> and k_area_select of auromat_amd/csrc/amt_area.hip) on
constructed collections: the cases of tests/_mosaic_area_cases.py go to ``amt_area_mosaic_frames`` as plain device arrays, under
both overlap rules, and every output (area, img, mask, coverage, source) is compared with tests/_mosaic_area_oracle.py bit for
bit.  There is no tolerance anywhere.  tests/test_mosaic_area_cpu.py checks without a GPU that the oracle gives the exact answers
on dyadic coordinates and that the collections aim where they claim to (the lane path and the wave path on clipped ranges, the
switch between them, windows and select tiles, the kinds of rule 1 cells, the coverage limit).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _area_cases as K
import _area_oracle as O
import _mosaic_area_cases as MK
import _mosaic_area_oracle as MA

pytestmark = pytest.mark.gpu

POISON = 0xA5
OUT_KEYS = ('area', 'img', 'mask', 'coverage', 'source')
CASES = MK.device_cases()
CASE_RULES = [(c, r) for c in CASES for r in c.rules]
IDS = ['%s-rule%d' % (c.name, r) for c, r in CASE_RULES]


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


class Member(object):
    """A member in device memory, its coordinate arrays `coord_offset` doubles into their allocations."""

    def __init__(self, case):
        self.case = case
        self.nch = case.img.shape[1]
        co = case.coord_offset
        self.lat, self.lon, self.lat_c = (_device_array(v, co) for v in (case.lat, case.lon, case.lat_c))
        self.elev = None if case.elev is None else _device_array(case.elev, co)
        self.img = _device_array(case.img) if self.nch else None
        self.mask = None if case.mask is None else _device_array(case.mask.astype(np.uint8))
        assert self.lat.data_ptr() % 16 == 8 * co


class Device(object):
    """A collection in device memory with its member table and axes."""

    def __init__(self, coll):
        from auromat_amd._native import AreaMosaicMember, Context, ptr
        from auromat_amd.util.histogram import make_axis
        self.coll, self.ctx = coll, Context.current()
        self.code = 2 if coll.dtype == np.uint16 else 1
        self.members = [Member(m) for m in coll.members]
        self.table = (AreaMosaicMember * len(self.members))()
        for t, m, (x0, y0, wnx, wny) in zip(self.table, self.members, coll.windows):
            t.lat, t.lon, t.lat_c, t.elev, t.img, t.center_mask = [None if a is None else ptr(a).value for a in
                                                                   (m.lat, m.lon, m.lat_c, m.elev, m.img, m.mask)]
            t.height, t.width = m.case.height, m.case.width
            t.win_x0, t.win_y0, t.win_nx, t.win_ny = x0, y0, wnx, wny
        self.xaxis, self._xkeep = make_axis(self.ctx, coll.xedges, uniform=coll.uniform)
        self.yaxis, self._ykeep = make_axis(self.ctx, coll.yedges, uniform=coll.uniform)
        assert self.xaxis.uniform == self.yaxis.uniform == int(coll.uniform)

    def run(self, rule, least, omit=(), table=None, n=None):
        """amt_area_mosaic_frames on poisoned outputs -> (status, host arrays of the outputs that were asked for)."""
        import torch
        from auromat_amd._native import lib, ptr
        coll, ctx = self.coll, self.ctx
        ny, nx = coll.shape
        nch = coll.nch
        out = dict(area=ctx.empty((ny, nx, nch + 1)), img=ctx.empty((ny, nx, nch), torch.int16 if self.code == 2 else torch.uint8),
                   mask=ctx.empty((ny, nx), torch.uint8), coverage=ctx.empty((ny, nx)), source=ctx.empty((ny, nx), torch.int32))
        for t in out.values():
            t.view(torch.uint8).fill_(POISON)
        arg = lambda k: None if k in omit or (k == 'img' and not nch) else ptr(out[k])
        rc = lib().amt_area_mosaic_frames(ctx.handle, self.table if table is None else table, len(self.members) if n is None else n,
                                          self.code, nch, float('-inf'), C.byref(self.xaxis), C.byref(self.yaxis), coll.lon_wrap,
                                          rule, least, arg('area'), arg('img'), arg('mask'), arg('coverage'), arg('source'))
        torch.cuda.synchronize()
        got = {k: t.cpu().numpy() for k, t in out.items()}
        got['img'] = got['img'].view(coll.dtype)
        for k in omit:
            assert (got[k].view(np.uint8) == POISON).all(), 'the omitted output %s was written' % k
            del got[k]
        return rc, got


@functools.lru_cache(maxsize=None)
def device(name):
    return Device(next(c for c in CASES if c.name == name))


@functools.lru_cache(maxsize=None)
def expected(name, rule):
    coll = next(c for c in CASES if c.name == name)
    return MA.mosaic(coll.members, coll.windows, rule, coll.min_coverage)


def check_outputs(got, want, what, keys=OUT_KEYS):
    for key in keys:
        if key in got:
            assert O.same_bits(got[key], want[key]), '%s: %s differs' % (what, key)


def frame_outputs(ctx, case, least):
    """amt_area_frame + amt_area_frame_finalize of one frame on the device -> host arrays."""
    import torch
    from auromat_amd._native import lib, ptr
    from auromat_amd.util.histogram import make_axis
    m = Member(case)
    xaxis, _xk = make_axis(ctx, case.xedges, uniform=case.uniform)
    yaxis, _yk = make_axis(ctx, case.yedges, uniform=case.uniform)
    ny, nx = case.shape
    nch = m.nch
    code = 2 if case.img.dtype == np.uint16 else 1
    acc = torch.zeros((nch + 2) * nx * ny, dtype=torch.int64, device=ctx.device)
    ctx.call('amt_area_frame', ptr(m.lat), ptr(m.lon), ptr(m.lat_c), ptr(m.elev), ptr(m.img), code, nch, ptr(m.mask), case.height,
             case.width, float(case.min_elevation), C.byref(xaxis), C.byref(yaxis), case.lon_wrap, ptr(acc))
    out = dict(area=ctx.empty((ny, nx, nch + 1)), img=ctx.empty((ny, nx, nch), torch.int16 if code == 2 else torch.uint8),
               mask=ctx.empty((ny, nx), torch.uint8), coverage=ctx.empty((ny, nx)))
    rc = lib().amt_area_frame_finalize(ctx.handle, ptr(acc), nx, ny, nch, code, least, ptr(out['area']),
                                       ptr(out['img']) if nch else None, ptr(out['mask']), ptr(out['coverage']))
    assert rc == 0
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got['img'] = got['img'].view(case.img.dtype)
    return got


@pytest.mark.parametrize('coll,rule', CASE_RULES, ids=IDS)
def test_case_equals_oracle(coll, rule):
    dev = device(coll.name)
    want = expected(coll.name, rule)
    least = O.min_weight(coll.min_coverage)
    rc, got = dev.run(rule, least)
    assert rc == coll.status[rule] and want['over'] == (rc == MK.EDOMAIN)
    if rc:
        from auromat_amd._native import lib
        assert b'2^40' in lib().amt_last_error(dev.ctx.handle)
        return
    check_outputs(got, want, '%s, rule %d' % (coll.name, rule))
    assert np.array_equal(got['source'] >= 0, got['mask'] == 0)
    # a second run gives the same bits
    rc, again = dev.run(rule, least)
    assert rc == 0
    check_outputs(again, got, '%s, rule %d, second run' % (coll.name, rule))


@pytest.mark.parametrize('coverage', [0.0, 1.0])
@pytest.mark.parametrize('name', ['three_with_empty', 'sliver', 'clip_wave'])
def test_other_minimum_coverages(name, coverage):
    dev = device(name)
    for rule in (0, 1):
        rc, got = dev.run(rule, O.min_weight(coverage))
        assert rc == 0
        check_outputs(got, MA.mosaic(dev.coll.members, dev.coll.windows, rule, coverage), '%s, rule %d, %s' % (name, rule, coverage))
    # a minimum weight of 0 is the rule's floor of 1
    rc, zero = dev.run(1, 0)
    check_outputs(zero, MA.mosaic(dev.coll.members, dev.coll.windows, 1, least=1), name + ', least 0')


@pytest.mark.parametrize('coll,rule', [(c, r) for c, r in CASE_RULES if c.status[r] == 0],
                         ids=[i for i, (c, r) in zip(IDS, CASE_RULES) if c.status[r] == 0])
def test_omitted_outputs_leave_the_others_alone(coll, rule):
    dev = device(coll.name)
    least = O.min_weight(coll.min_coverage)
    rc, full = dev.run(rule, least)
    assert rc == 0
    for key in OUT_KEYS:
        rc, got = dev.run(rule, least, omit=(key,))
        assert rc == 0 and key not in got
        check_outputs(got, full, '%s, rule %d, without %s' % (coll.name, rule, key))
    rc, got = dev.run(rule, least, omit=OUT_KEYS)
    assert rc == 0 and not got


@pytest.mark.parametrize('whole,coll', MK.partition_cases(), ids=lambda v: repr(v))
def test_partition_equals_the_uncut_frame_on_the_device(whole, coll):
    """The parts of a frame as members on the full grid, rule 0: amt_area_frame + amt_area_frame_finalize of the uncut frame."""
    dev = device(coll.name)
    for coverage in (0.5, 0.0):
        least = O.min_weight(coverage)
        want = frame_outputs(dev.ctx, whole, least)
        rc, got = dev.run(0, least)
        assert rc == 0
        check_outputs(got, want, coll.name, keys=('area', 'img', 'mask', 'coverage'))
        assert np.array_equal(got['source'] >= 0, want['mask'] == 0)


def test_one_member_equals_the_frame_entry_points():
    dev = device('one_member')
    least = O.min_weight(0.5)
    want = frame_outputs(dev.ctx, dev.coll.members[0], least)
    for rule in (0, 1):
        rc, got = dev.run(rule, least)
        assert rc == 0
        check_outputs(got, want, 'one member, rule %d' % rule, keys=('area', 'img', 'mask', 'coverage'))
        assert np.array_equal(got['source'], np.where(want['mask'] == 0, 0, -1))


def test_all_windows_empty():
    """No binning launch: an all-masked grid, source -1, coverage 0."""
    from auromat_amd._native import AreaMosaicMember
    dev = device('two_in_one_tile')
    table = (AreaMosaicMember * 2)()
    for t, s in zip(table, dev.table):
        C.memmove(C.byref(t), C.byref(s), C.sizeof(AreaMosaicMember))
        t.win_x0 = t.win_y0 = t.win_nx = t.win_ny = 0
    for rule in (0, 1):
        rc, got = dev.run(rule, O.min_weight(0.5), table=table)
        assert rc == 0
        assert np.isnan(got['area']).all() and not got['img'].any() and (got['mask'] == 1).all()
        assert (got['coverage'] == 0).all() and (got['source'] == -1).all()


def test_bad_arguments_are_refused():
    from auromat_amd._native import AreaMosaicMember
    dev = device('two_in_one_tile')
    least = O.min_weight(0.5)
    EINVAL = -1

    def changed(**kw):
        table = (AreaMosaicMember * 2)()
        for t, s in zip(table, dev.table):
            C.memmove(C.byref(t), C.byref(s), C.sizeof(AreaMosaicMember))
        for k, v in kw.items():
            setattr(table[1], k, v)
        return table
    rc, _ = dev.run(1, least, omit=OUT_KEYS, table=changed(elev=None))
    assert rc == EINVAL                                     # rule 1 needs every member's elevation
    assert dev.run(0, least, omit=OUT_KEYS, table=changed(elev=None))[0] == 0
    for kw in (dict(lat=None), dict(lon=None), dict(lat_c=None), dict(img=None), dict(height=0), dict(win_nx=-1),
               dict(win_x0=47, win_nx=2), dict(win_y0=-1)):
        assert dev.run(0, least, omit=OUT_KEYS, table=changed(**kw))[0] == EINVAL, kw
    assert dev.run(2, least, omit=OUT_KEYS)[0] == EINVAL
    assert dev.run(0, least, omit=OUT_KEYS, n=0)[0] == EINVAL
    # fmt_no_elev: rule 1 is refused for the collection that the rule 0 cases run
    assert device('fmt_no_elev').run(1, least, omit=OUT_KEYS)[0] == EINVAL
