"""
``amt_area_frame_async`` (auromat_amd/csrc/amt_area.hip): the enqueue-only form of ``amt_area_frame`` +
``amt_area_frame_finalize`` on the constructed cases of tests/_area_cases.py, against tests/_area_oracle.py and against the
synchronous pair, bit for bit; the MLT switch, the row band, the caller's overflow word, the shared workspace and that the call
does not wait for its stream.  No tolerance anywhere: the oracle restates the kernel's arithmetic operation for operation.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import _area_cases as K
import _area_oracle as O
from test_gpu_area_cells import POISON, Frame, check_outputs, finalize

pytestmark = pytest.mark.gpu

EINVAL = -1


def run_async(frame, least, band=None, lon_from_mlt=0, over=None, lon=None, outputs=True):
    """amt_area_frame_async on poisoned outputs -> (status, host arrays); `lon`: a device array in place of the frame's."""
    import torch
    from auromat_amd._native import lib, ptr
    case, ctx = frame.case, frame.ctx
    ny, nx = case.shape
    nch = frame.nch
    dtype = np.dtype(case.img.dtype)
    out = dict(area=ctx.empty((ny, nx, nch + 1)), img=ctx.empty((ny, nx, nch), torch.int16 if dtype == np.uint16 else torch.uint8),
               mask=ctx.empty((ny, nx), torch.uint8), coverage=ctx.empty((ny, nx)))
    for t in out.values():
        t.view(torch.uint8).fill_(POISON)
    r0, r1 = (0, case.height) if band is None else band
    rc = lib().amt_area_frame_async(
        ctx.handle, ptr(frame.lat), ptr(frame.lon if lon is None else lon), ptr(frame.lat_c), ptr(frame.elev), ptr(frame.img),
        frame.code, nch, ptr(frame.mask), case.height, case.width, float(case.min_elevation), C.byref(frame.xaxis),
        C.byref(frame.yaxis), case.lon_wrap, lon_from_mlt, r0, r1, least, ptr(out['area']) if outputs else None,
        ptr(out['img']) if nch and outputs else None, ptr(out['mask']) if outputs else None,
        ptr(out['coverage']) if outputs else None, ptr(over))
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got['img'] = got['img'].view(dtype)
    return rc, got


def oracle(case, coverage):
    return O.finalize(O.accumulate(case)[0], case.img.dtype, coverage)


def check_against_both(case, coverages=(0.5,)):
    """The async call equals the oracle and the synchronous pair, output for output."""
    frame = Frame(case)
    acc, _ = frame.accumulate()
    want_acc, _ = O.accumulate(case)
    ny, nx = case.shape
    for coverage in coverages:
        least = O.min_weight(coverage)
        rc, got = run_async(frame, least)
        assert rc == 0
        check_outputs(got, O.finalize(want_acc, case.img.dtype, coverage), '%s, minCoverage %s, oracle' % (case.name, coverage))
        rc2, sync = finalize(frame.ctx, acc, nx, ny, frame.nch, case.img.dtype, least)
        assert rc2 == 0
        if not frame.nch:
            sync['img'] = got['img']            # (no kernel writes an image without channels: both hold the poison)
        check_outputs(got, sync, '%s, minCoverage %s, synchronous pair' % (case.name, coverage))


@pytest.mark.parametrize('case', K.device_cases(), ids=repr)
def test_case_equals_oracle_and_the_synchronous_pair(case):
    check_against_both(case)


def threshold_case(dtype):
    """Unit cells whose total weight lies exactly at, one below and one above the thresholds of minCoverage 0, 0.5 and 1: one
    rectangle of full height per cell, its width the fraction (dyadic, so W = fraction * 2^32 exactly); the last cell takes two."""
    u = 2.0 ** -32
    widths = [u, 2 * u, 0.5 - u, 0.5, 0.5 + u, 1.0 - u, 1.0, 0.25]
    rect = lambda x, f: [(x, 0.0), (x + f, 0.0), (x + f, 1.0), (x, 1.0)]
    quads = [rect(float(i), f) for i, f in enumerate(widths)]
    quads += [rect(8.0, 1.0), rect(8.0, u)]                     # 2^32 + 1 in cell 8; cell 9 stays empty
    return K.quads_frame('threshold_%s' % np.dtype(dtype).name, quads, K.unit_edges(10), K.unit_edges(1), dtype=dtype, seed=81)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_threshold_case(dtype):
    case = threshold_case(dtype)
    w = O.accumulate(case)[0][0][:, 0]
    assert w.tolist() == [1, 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, 1 << 30, (1 << 32) + 1, 0]
    masks = {c: oracle(case, c)['mask'][0].tolist() for c in (0.0, 0.5, 1.0)}
    assert masks[0.0] == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert masks[0.5] == [1, 1, 1, 0, 0, 0, 0, 1, 0, 1]
    assert masks[1.0] == [1, 1, 1, 1, 1, 1, 0, 1, 0, 1]
    check_against_both(case, (0.0, 0.5, 1.0))


def test_workspace_is_zeroed_by_every_call():
    """Two different cases back to back on one context: the second finds the first one's sums in the workspace."""
    first, second = Frame(K.heavy_cell_case()), Frame(K.outside_case())
    assert first.ctx is second.ctx
    least = O.min_weight(0.5)
    assert run_async(first, least)[0] == 0
    rc, got = run_async(second, least)
    assert rc == 0
    check_outputs(got, oracle(second.case, 0.5), 'second call')
    rc, got = run_async(first, least)
    assert rc == 0
    check_outputs(got, oracle(first.case, 0.5), 'third call')


def mlt_pair(case):
    """(hours for the device, the case the oracle takes): the oracle is fed (h - 12.0) / (24.0 / 360.0) computed in NumPy."""
    hours = case.lon * (24.0 / 360.0) + 12.0
    fed = copy.copy(case)
    fed.lon = (hours - 12.0) / (24.0 / 360.0)
    return hours, fed


@pytest.mark.parametrize('name', ['outside', 'axis_lon_wrap', 'shape_2x257_off1'])
def test_lon_from_mlt(name):
    from test_gpu_area_cells import _device_array
    case = [c for c in K.device_cases() if c.name == name][0]
    assert case.lon_wrap == (1 if name == 'axis_lon_wrap' else 0)
    hours, fed = mlt_pair(case)
    assert not np.array_equal(fed.lon, case.lon)                # (the round trip is not the identity: the expression matters)
    frame = Frame(case)
    rc, got = run_async(frame, O.min_weight(0.5), lon_from_mlt=1, lon=_device_array(hours, case.coord_offset))
    assert rc == 0
    want = oracle(fed, 0.5)
    assert (want['mask'] == 0).any()
    check_outputs(got, want, name)


def banded(case, r0, r1):
    """The case with lat_c NaN outside the rows [r0, r1)."""
    out = copy.copy(case)
    out.lat_c = case.lat_c.copy()
    out.lat_c[:r0] = np.nan
    out.lat_c[r1:] = np.nan
    return out


BAND_CASES = {
    # width 5, r0 = 3: the band starts 15 pixels into the frame, inside a wave of the full sweep
    'w5': (lambda: K.lattice('band_w5', 9, 5, K.unit_edges(8, 0.5), K.unit_edges(12, 0.5), 0.2, 0.3, 0.7, 0.6, jitter=0.2, seed=91), 3, 7),
    # 28 rows of 37 pixels: five workgroups, the last one partly filled, first pixel 185
    'blocks': (lambda: K.lattice('band_blocks', 40, 37, K.unit_edges(30, 0.5), K.unit_edges(30, 0.5), 0.1, 0.2, 0.4, 0.36,
                                 jitter=0.3, seed=92, dtype=np.uint16), 5, 33),
    # pixels wider than 16 cells inside the band: the wave path
    'wide': (lambda: K.lattice('band_wide', 6, 3, K.unit_edges(40, 0.25), K.unit_edges(40, 0.25), 0.3, 0.2, 3.1, 1.6, jitter=0.2,
                               seed=93), 1, 4),
}


@pytest.mark.parametrize('name', sorted(BAND_CASES))
def test_row_band(name):
    make, r0, r1 = BAND_CASES[name]
    case = make()
    assert np.isfinite(case.lat_c).all() and 0 < r0 < r1 < case.height
    if name == 'wide':
        assert (K.candidate_counts(banded(case, r0, r1)) > K.LANE_CELLS).any()
    frame = Frame(case)
    least = O.min_weight(0.5)
    want = oracle(banded(case, r0, r1), 0.5)
    whole = oracle(case, 0.5)
    assert not O.same_bits(want['coverage'], whole['coverage'])         # (the rows outside would have contributed)
    rc, got = run_async(frame, least, band=(r0, r1))
    assert rc == 0
    check_outputs(got, want, '%s [%d, %d)' % (name, r0, r1))
    for r in (0, r0, case.height):
        rc, got = run_async(frame, least, band=(r, r))
        assert rc == 0
        assert (got['mask'] == 1).all() and (got['coverage'] == 0).all() and np.isnan(got['area']).all() and (got['img'] == 0).all()
    rc, got = run_async(frame, least, band=(0, case.height))
    assert rc == 0
    check_outputs(got, whole, name + ' whole')


def test_the_call_does_not_wait_for_the_stream():
    import torch
    frame = Frame(K.outside_case())
    least = O.min_weight(0.5)
    # (once to size the workspace: growing it synchronises the stream, as for every user of the workspace)
    assert run_async(frame, least)[0] == 0
    from auromat_amd._native import lib, ptr
    case, ctx = frame.case, frame.ctx
    ny, nx = case.shape
    area, img = ctx.empty((ny, nx, 4)), ctx.empty((ny, nx, 3), torch.uint8)
    mask, coverage = ctx.empty((ny, nx), torch.uint8), ctx.empty((ny, nx))
    over = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    torch.cuda.synchronize()
    torch.cuda._sleep(200000000)                # tens of ms of GPU time ahead of the pass on the same stream
    slept = torch.cuda.Event()
    slept.record()
    rc = lib().amt_area_frame_async(ctx.handle, ptr(frame.lat), ptr(frame.lon), ptr(frame.lat_c), ptr(frame.elev), ptr(frame.img),
                                    frame.code, 3, None, case.height, case.width, float('-inf'), C.byref(frame.xaxis),
                                    C.byref(frame.yaxis), 0, 0, 0, case.height, least, ptr(area), ptr(img), ptr(mask),
                                    ptr(coverage), ptr(over))
    assert rc == 0
    assert not slept.query(), 'amt_area_frame_async waited for the stream'
    torch.cuda.synchronize()
    want = oracle(case, 0.5)
    got = dict(area=area.cpu().numpy(), img=img.cpu().numpy(), mask=mask.cpu().numpy(), coverage=coverage.cpu().numpy())
    check_outputs(got, want, 'behind the sleep')
    assert int(over.item()) == 0


def test_overflow_word():
    """256 unit squares over one cell leave the caller's word alone, 257 set it, and nothing clears it but the caller."""
    import torch
    from auromat_amd._native import Context
    ctx = Context.current()
    least = O.min_weight(0.5)
    fits, too_much = Frame(K.coverage_limit_case(256)), Frame(K.coverage_limit_case(257))
    over = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    rc, got = run_async(fits, least, over=over)
    assert rc == 0 and int(over.item()) == 0
    check_outputs(got, oracle(fits.case, 0.5), 'coverage_limit_256')
    rc, _ = run_async(too_much, least, over=over)
    assert rc == 0 and int(over.item()) == 1
    rc, got = run_async(fits, least, over=over)
    assert rc == 0 and int(over.item()) == 1
    check_outputs(got, oracle(fits.case, 0.5), 'coverage_limit_256 after 257')
    for frame in (fits, too_much):
        assert run_async(frame, least, over=None)[0] == 0
    rc, got = run_async(fits, least, over=None)
    check_outputs(got, oracle(fits.case, 0.5), 'coverage_limit_256 without a word')


def test_null_outputs_are_accepted():
    frame = Frame(K.outside_case())
    rc, got = run_async(frame, O.min_weight(0.5), outputs=False)
    assert rc == 0
    assert all((v.view(np.uint8) == POISON).all() for v in got.values())


def test_bad_arguments_are_refused():
    from auromat_amd._native import lib, ptr
    frame = Frame(K.outside_case())
    case, ctx = frame.case, frame.ctx
    h, w = case.height, case.width
    least = O.min_weight(0.5)
    for band in ((-1, h), (0, h + 1), (5, 4), (h + 1, h + 1)):
        assert run_async(frame, least, band=band)[0] == EINVAL, band
    assert b'row_begin' in lib().amt_last_error(ctx.handle)

    def call(lat=frame.lat, img=frame.img, code=1, nch=3, height=h, width=w, out_img=None, out_code=None):
        return lib().amt_area_frame_async(ctx.handle, ptr(lat), ptr(frame.lon), ptr(frame.lat_c), None, ptr(img),
                                          code if out_code is None else out_code, nch, None, height, width, float('-inf'),
                                          C.byref(frame.xaxis), C.byref(frame.yaxis), 0, 0, 0, max(height, 0), least, None,
                                          ptr(out_img), None, None, None)

    assert call() == 0
    # the refusals of amt_area_frame ...
    assert call(nch=5) == EINVAL
    assert call(height=0) == EINVAL
    assert call(width=0) == EINVAL
    assert call(lat=None) == EINVAL
    assert call(img=None) == EINVAL
    assert call(code=3) == EINVAL
    # ... and of amt_area_frame_finalize: an image output of an unknown type
    assert call(nch=0, img=None, out_img=frame.img, out_code=3) == EINVAL
