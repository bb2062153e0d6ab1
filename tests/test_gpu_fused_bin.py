"""
The binning that is fused into the row kernel (k_georef_rows<..., BIN> of auromat_amd/csrc/amt_georef.hip) and the two kernels
that resolve its on-edge pixels (k_apply_bin_events, k_pipe_finish of amt_binning.hip), on the constructed grids of
tests/_fused_cases.py.  Every case runs in two launches: the plain entry point first, for the device's own centre arrays, then
the same frame with bin_acc and axes built around single pixels of those arrays.  What must come out is stated by
tests/_bin_oracle.py and tests/_median_oracle.py (the reference's histogram rule) on exactly those arrays; count, the three
channel sums and the 31.32 fixed-point elevation sums are integers and must be equal in every cell.  There is no tolerance
anywhere in this module.  tests/test_fused_cases_cpu.py checks without a GPU that the cases hold what they claim.

What each family aims at
  class grids    one kept pixel ON edge k of an axis (bit for bit), one ulp below and above it, above it inside the rounding
                 zone of the right-most-edge rule, above it outside that zone but inside bin_fast's margin, and well inside a
                 cell — at the first, an interior and the last edge, on x and y around the same pixel (flags 3) and in mixed
                 pairs, at steps 1/8 and 0.1: bin_fast and its margin, bin_slow, bin_index<true>, on_lower_edge_bits and the flags,
                 the right-most-edge rule at the last edge, pixels below and beyond the axes on all four sides
  long axes      the same relations 144 to 3000 edges up an axis of 60000 bins of 0.1: the first guess of bin_index and the bits
                 of linspace_edge
  one cell       every pixel of the frame in one cell, once with every channel at its maximum: the per-lane run sums over 16
                 rows and the 32-bit window sums at their largest
  fine grids     1/128 deg cells in x, in y, in both: most pixels lie outside their wave's 8 x 8 window and take the global
                 atomics of bin_flush
  anchors        the first binned pixel of the last wave in cell 1 / cell nbin of either axis: window anchors below 1 and
                 windows that reach past the axis
  frames         63 columns x 16 rows and one more / fewer of each, 3 x 1 and 2 x 40, both image types (rows of a uint8 image
                 of odd width are not 8-byte aligned), a field with NaN corners, a camera inside the shell with -inf as the
                 threshold (every elevation is negative: to_fix32 on negative values), two date-line fields with bin_lon_wrap,
                 and every field once more on the (SM longitude, MLat) grid (bin_magnetic, SECOND = 1)
  with events    the records must be exactly the pixels on_lower_edge_bits's definition flags, with their bins, flags, channels and
                 fixed-point elevation; the accumulators hold everything else; and a Python statement of k_apply_bin_events
                 applied to both equals the oracle on every window whose last edge carries such a pixel, and on one whose last
                 edges do not.  The sub-axes of a window ARE edges of the grid given, so they share its bits, and only windows
                 whose `decimal` equals the grid's are taken: they share its scale too, by construction.  (A final grid whose
                 scale differs from its superset's is the subject of test_event_resolution_through_the_pipeline[aimed-scale].)
  pipeline       aimed fields (single interior pixels 2e-7 deg above, 8e-7 deg above and 2e-7 deg below the last x, last y,
                 first x and interior edges of the frame's own final grid at 8 px/deg, one pixel on the last x and y edge at
                 once, and the last MLat edge of a magnetic grid) through run(fuse=True) — amt_pipe_finalize with
                 k_apply_bin_events —, run(fuse=False) and the oracle on the final grid; three such frames in one launch
                 (k_pipe_finish, per-frame constant blocks with events) against single launches and the oracle.

Measured on the MI355X (printed with -s)
  per field and grid family (geodetic and magnetic, both image types): 69 grids (127 x 33: 65; the date-line fields on the
  magnetic grid: 66, without the fine grids), every relation at every position on both axes — one pixel each per grid —; 28
  on-edge pixels (7 with flags 1, 7 with flags 2, 14 with flags 3) and 28 records; 224 to 241 windows resolved; pixels outside
  their wave's window: 3x1 3, 62x15 4804, 63x16 5035, 64x17 5126, 127x33 13116, 2x40 272, broken 949, inside 783, date line
  128 / 201; the one-cell grids hold 3 / 930 / 1008 / 1088 / 4191 / 80 / 134 / 256 / 40 / 40 pixels; anchors in cell 1 and in
  cell nbin of both axes and outliers on all four sides in every field.
  camera variants: 36 class grids and 12 records each (pole: 34 and 10).
  aimed fields, records of the fused launch (edge_pixels; the superset flags interior edges too, and inside the band the
  neighbouring roundings) / pixels flagged on the final
  grid: aimed-64x17 13 / 5, aimed-127x33 13 / 7, aimed-64x17-b 6 / 3, aimed-64x17-c 7 / 3, aimed-mag-64x17 4 / 1, aimed-scale 3 / 1,
  aimed-scale-y 4 / 1, aimed-scale-xy 8 / 2, aimed-finer 3 / 0; three frames in one launch 13, 6, 7 / 3, 8, 4 / 3, 3, 3.
  Every device centre within 1e-9 deg of its place.

Expected difference 1 (the on-edge zone): CONFIRMED.  aimed-scale is a 16 x 9 field at 10 px/deg whose final x axis (7 cells) has
no edge difference below 0.1 and so rounds at 1e-6 deg, its superset at 1e-7.  A kernel that flags with the superset's rounding
alone loses the pixel 2e-7 deg beyond the final grid's last x edge: 7 pixels in the last cell of the bottom row where
run(fuse=False) and the oracle count 8.  The benchmark's sequence has both directions: of its 2605 frames 83 final grids round
coarser than their superset and 27 finer (next to the prime meridian, where a superset of 30 cells can have no difference below
0.1).  Those frames must stay with the single-pass plan, so inside a band at the end of each superset axis the kernel records
on-edge pixels under all three roundings, one flag bit per reading (bin_event), and the finalise kernels take the bit of the final
grid's rounding.  Cases: aimed-scale, aimed-scale-y, aimed-scale-xy (final coarser on x, on y, on both) and aimed-finer (final
finer on x), each with a pixel 2e-7 deg beyond the last edge (on-edge under the coarser rounding alone), one 2e-8 deg beyond it
(under both) and one 2e-7 deg above the lower edge of the last cell (inside the band, stays in its cell); through
amt_pipe_finalize and, three in a launch, through k_pipe_finish.  They assert 'single-pass' and grids equal to run(fuse=False) and
to the oracle.  test_a_poor_estimate_is_handed_back_once_and_then_fused covers the one hand-back that remains (a final grid that
rounds differently and ends below the band) and the single retry.  The flag bits 4 to 32 are not compared with an oracle record
by record (the C ABI has no band); every cell count of those cases depends on them, and the mutations below show it.
Expected difference 2 (edge bits) is counted in DESIGN.md and not fixed.  At 8 px/deg every edge used here has the same bits in
both grids (tests/test_fused_cases_cpu.py asserts it); at 10 px/deg the two versions of an edge are less than 1e-13 deg apart
(asserted there too) and every aimed pixel is at least 2e-8 deg from its edge, so it has the same relation to both.

Mutation check (scratch copies of the tree, never committed; failing tests of this module, which had 111 tests when the rows
above the line were counted and has 113 now)
  bin_fast with margin = 0                                   56   (records and pipeline: the flags are lost, the bins stay right)
  on_lower_edge_bits comparing with edge b, not b - 1        56
  window test dx < kBinW turned into dx <= kBinW             66
  to_fix32 replaced by truncation                            97
  koff forced to 0                                            2   (test_three_frames_in_one_launch: the only route to frames 2, 3)
  cx == off_x + nx turned into cx >= off_x + nx               0   an equivalent mutant: a flagged record with cx > off_x + nx moves
                                                                  to cx - 1 >= off_x + nx, still outside the window, and the window
                                                                  is all that k_apply_bin_events and k_pipe_finish hand on
  cx == off_x + nx turned into cx + 1 == off_x + nx           9   (its neighbour that can be told apart)
  band test b - 1 >= ax.band disabled                         5   (the three scale cases, the poor estimate, three frames[scale])
  margin 15.0 of an axis with a band back to 1.5              5   (the same five)
  x shift of the coarser bit, (f & 2u) << 1 to << 2           4   (scale, scale-xy, poor estimate, three frames[scale])
  y shift of the coarser bit, (f & 2u) << 2 to << 1           3   (scale-y, scale-xy, three frames[scale])
  xmask of the coarser reading 4u to 1u                       4
  ymask of the coarser reading 8u to 2u                       3
  F.masks >> 8 in k_pipe_finish to >> 9                       2   (three frames[eighth] and [scale])
  hand-back below the band disabled                           1   (test_a_poor_estimate_is_handed_back_once_and_then_fused)
  ---------------------------------------------------------------
  xmask of the finer reading 16u to 1u                        2   (aimed-finer, three frames[finer])
  x shift of the finer bit, (f & 4u) << 2 to << 1             2   (the same two)
"""
import ctypes as C

import numpy as np
import pytest

import _bin_oracle as B
import _camera_cases as CK
import _fused_cases as F
import _rowfield_cases as K
import _rowfield_oracle as R
from test_gpu_rowfield import POISON, POISON_F64, frame_params, same_bits

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16)
SPARE = 64                                            # poisoned words behind the accumulators
EVENT_ROOM = 64


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


def case_of(name):
    return F.aimed_case(name) if name.startswith('aimed') else K.by_name(name)


_FIRST, _DIRS = {}, {}


def dirs_of(name):
    if name not in _DIRS:
        _DIRS[name] = _ctx().to_device(np.array(case_of(name)['dirs']))
    return _DIRS[name]


def first_launch(name):
    """the plain entry point on poisoned buffers -> the nine host arrays (test_gpu_rowfield.kernel_arrays for any case dict)"""
    if name not in _FIRST:
        import torch
        from auromat_amd._native import GeorefOut
        c, ctx = case_of(name), _ctx()
        h, w = c['height'], c['width']
        out, bufs = GeorefOut(), {}
        for k in R.ARRAYS:
            t = ctx.empty((h + 1, w + 1) if k in R.CORNER_ARRAYS else (h, w))
            t.view(torch.uint8).fill_(POISON)
            bufs[k] = t
            setattr(out, k, t.data_ptr())
        p = frame_params(c)
        ctx.call('amt_georef_frame_dirs', C.byref(p), C.c_void_p(dirs_of(name).data_ptr()), C.byref(out))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in bufs.items()}
        for k, v in got.items():
            assert not (v.view(np.uint64) == POISON_F64).any(), (name, k)
            v.setflags(write=False)
        _FIRST[name] = got
    return _FIRST[name]


def device_image(img):
    import torch
    a = np.ascontiguousarray(img)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(_ctx().device)


def fused_launch(name, xedges, yedges, img, min_elevation, magnetic=False, lon_wrap=False, events=0, outputs=None, camera=None):
    """The second launch: amt_georef_frame_dirs with bin_acc on zeroed planes with poisoned words behind them.  events: room
    for that many records (0: no event list).  outputs: None (every per-pixel pointer NULL), 'contiguous' or 'padded'.
    -> dict(acc (5, nx, ny) int64, count, records, arrays)"""
    import torch
    from auromat_amd._native import GeorefOut
    from auromat_amd.util.histogram import make_axis
    ctx = _ctx()
    c = case_of(name) if camera is None else CK.by_name(name)
    h, w = c['height'], c['width']
    xa, _ = make_axis(ctx, xedges, uniform=True)
    ya, _ = make_axis(ctx, yedges, uniform=True)
    assert xa.uniform == 1 and ya.uniform == 1
    nx, ny = xa.nbin, ya.nbin
    words = 5 * nx * ny
    acc = torch.zeros(words + SPARE, dtype=torch.int64, device=ctx.device)
    acc.view(torch.uint8)[8 * words:] = POISON
    dimg = device_image(img)
    out = GeorefOut()
    out.bin_acc, out.bin_img, out.bin_img_dtype = acc.data_ptr(), dimg.data_ptr(), 1 if img.dtype == np.uint8 else 2
    out.bin_xaxis, out.bin_yaxis = C.addressof(xa), C.addressof(ya)
    out.bbox_min_elevation = float(min_elevation)
    out.bin_lon_wrap, out.bin_magnetic = int(lon_wrap), int(magnetic)
    ev = counter = None
    if events:
        ev = torch.full((32 * events + 8 * SPARE,), POISON, dtype=torch.uint8, device=ctx.device)
        counter = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        out.bin_events, out.bin_event_count, out.bin_event_capacity = ev.data_ptr(), counter.data_ptr(), events
    bufs = {}
    if outputs is not None:
        pitch = int(ctx._lib.amt_padded_pitch(w)) if outputs == 'padded' else None
        out.row_layout = 1 if outputs == 'padded' else 0
        for k in R.ARRAYS:
            rows, cols = (h + 1, w + 1) if k in R.CORNER_ARRAYS else (h, w)
            t = ctx.empty((rows, pitch if pitch else cols))
            t.view(torch.uint8).fill_(POISON)
            bufs[k] = t
            setattr(out, k, t.data_ptr())
    if camera is None:
        p = frame_params(c)
        ctx.call('amt_georef_frame_dirs', C.byref(p), C.c_void_p(dirs_of(name).data_ptr()), C.byref(out))
    else:
        # the camera model: MLat / MLT-only mode (no geodetic output, bin_magnetic), exact centres, the two pole plans
        out.bin_pole, out.altitude = int(camera.get('pole', 0)), float(c['altitude'])
        p = CK.native_params(c)
        ctx.call('amt_georef_frame', C.byref(p), C.byref(out))
    torch.cuda.synchronize()
    res_variant = ctx.last_variant()
    flat = acc.cpu().numpy()
    assert (flat[words:].view(np.uint64) == POISON_F64).all(), (name, 'written behind the accumulators')
    res = dict(acc=flat[:words].reshape(5, nx, ny).copy(), count=None, records=None, variant=res_variant)
    if events:
        raw = ev.cpu().numpy()
        res['count'] = int(counter.cpu().numpy().view(np.uint32)[0])
        written = min(res['count'], events)
        assert (raw[32 * written:] == POISON).all(), (name, 'written behind the records')
        res['records'] = raw[:32 * written].view(F.EVENT_DTYPE).copy()
    if outputs == 'contiguous':
        res['arrays'] = {k: v.cpu().numpy() for k, v in bufs.items()}
    return res


def grids_of(name, magnetic=False):
    return F.grids(name, first_launch(name), magnetic=magnetic)


def case_for(name, g, dtype):
    s, arrays = F.settings_of(name), first_launch(name)
    x, y = F.binned_xy(arrays, g['magnetic'], g['lon_wrap'])
    return F.as_case(g['tag'], x, y, arrays['elev'], F.grid_image(name, s, g, dtype), g['xedges'], g['yedges'], g['min_elevation'])


def launch_grid(name, g, case, **kw):
    h, w = case.height, case.width
    return fused_launch(name, g['xedges'], g['yedges'], case.img.reshape(h, w, 3), g['min_elevation'], magnetic=g['magnetic'],
                        lon_wrap=g['lon_wrap'], **kw)


def assert_planes(tag, got, want):
    for k, plane in enumerate(('count', 'sum 0', 'sum 1', 'sum 2', 'fx')):
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, '%s: plane %s differs in %d cells, first (cx, cy) %s: got %d, want %d' % (
            tag, plane, len(bad), bad[0].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def check_claims(name, g):
    """the relation a grid claims holds on the DEVICE's arrays"""
    x, y = F.binned_xy(first_launch(name), g['magnetic'], g['lon_wrap'])
    assert F.relation(float(x[g['pixel']]), g['xedges'], g['k_x']) == g['rel_x'], (name, g['tag'], 'x')
    assert F.relation(float(y[g['pixel']]), g['yedges'], g['k_y']) == g['rel_y'], (name, g['tag'], 'y')


# ---- 1. accumulators through the C ABI, directions-in form ----------------------------------------------------------------------
@pytest.mark.parametrize('magnetic', [False, True], ids=['geodetic', 'magnetic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['uint8', 'uint16'])
@pytest.mark.parametrize('name', F.FIELDS)
def test_accumulators_without_an_event_list(name, dtype, magnetic):
    """The header's promise: without bin_events the grid given is the final one — _bin_oracle on the axes as given, the
    right-most-edge rule included."""
    gl = grids_of(name, magnetic)
    assert len(gl) >= 60
    total = 0
    for g in gl:
        check_claims(name, g)
        case = case_for(name, g, dtype)
        want = F.expected_planes(case)
        got = launch_grid(name, g, case)
        assert_planes('%s %s' % (name, g['tag']), got['acc'], want)
        total += int(want[0].sum())
    assert total > 0
    print(name, dtype.__name__, 'magnetic' if magnetic else 'geodetic', len(gl), 'grids,', total, 'binned pixels')


@pytest.mark.parametrize('magnetic', [False, True], ids=['geodetic', 'magnetic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['uint8', 'uint16'])
@pytest.mark.parametrize('name', F.FIELDS)
def test_accumulators_and_records_with_an_event_list(name, dtype, magnetic):
    """With bin_events the records, sorted, are exactly the pixels the reference's rule calls on-edge (bx, by, flags, channels,
    fixed-point elevation), the counter counts them and the accumulators hold everything else; and the Python statement of
    k_apply_bin_events on accumulators plus records equals the oracle on every window (see the module docstring)."""
    gl = grids_of(name, magnetic)
    n_records = n_windows = 0
    kinds = set()
    for g in gl:
        case = case_for(name, g, dtype)
        want_acc, want_ev = F.expected_with_events(case)
        got = launch_grid(name, g, case, events=EVENT_ROOM)
        tag = '%s %s' % (name, g['tag'])
        assert got['count'] == len(want_ev), (tag, got['count'], len(want_ev))
        got_ev = F.sorted_events(got['records'])
        assert np.array_equal(got_ev, want_ev), (tag, got_ev.tolist(), want_ev.tolist())
        assert_planes(tag, got['acc'], want_acc)
        n_records += len(want_ev)
        if g['kind'] != 'class':
            continue
        for window, kind in F.windows_of(case):
            sub = F.sub_case(case, window)
            assert F.decimal_of(sub.xedges) == F.decimal_of(case.xedges) and F.decimal_of(sub.yedges) == F.decimal_of(case.yedges)
            resolved = F.apply_events(got['acc'], got['records'], window)
            assert_planes('%s window %s' % (tag, window), resolved, F.expected_planes(sub))
            n_windows += 1
            kinds.add(kind)
    assert n_records >= 8 and n_windows >= 20 and kinds == {'x', 'y', 'xy', 'free'}, (n_records, n_windows, kinds)
    print(name, dtype.__name__, 'magnetic' if magnetic else 'geodetic', n_records, 'records,', n_windows, 'windows')


@pytest.mark.parametrize('name', F.FIELDS)
def test_census_on_the_device_arrays(name):
    """every class of tests/_fused_cases.py is populated on the device's own arrays (test_fused_cases_cpu.py: on the oracle's)"""
    c = F.census(name, first_launch(name), grids_of(name))
    print(name, {k: c[k] for k in ('flags', 'outside', 'full_cell', 'largest_k')}, sorted(c['anchor']), sorted(c['sides']))
    F.assert_census(name, c)


def test_too_many_bins_are_refused():
    from auromat_amd._native import NativeError
    name = 'ownership-3x1'
    img = F.image_of(name, 3, 1, np.uint16)
    ok, bad = np.linspace(0.0, 1.0, 3), np.linspace(0.0, 655.35, 65536)
    for xe, ye in ((bad, ok), (ok, bad)):
        with pytest.raises(NativeError, match='65534'):
            fused_launch(name, xe, ye, img, 0.0)
    assert fused_launch(name, np.linspace(0.0, 655.34, 65535), ok, img, 0.0)['acc'].shape == (5, 65534, 2)


def edge_grid(name):
    """an aimed field on its own final grid: several on-edge pixels in one launch"""
    c, arrays = F.aimed_case(name), first_launch(name)
    g = F.final_grid(F.box_of(arrays, c['magnetic']), c['ppd'])
    xe, ye = F.axis_edges(g.xaxis), F.axis_edges(g.yaxis)
    assert np.array_equal(xe, c['xedges']) and np.array_equal(ye, c['yedges'])
    x, y = F.binned_xy(arrays, c['magnetic'])
    img = F.image_of(name, c['width'], c['height'], np.uint16)
    return F.as_case(name, x, y, arrays['elev'], img, xe, ye, float('-inf')), img


def test_more_on_edge_pixels_than_records():
    """capacity 2 with at least 5 on-edge pixels: the counter reports all of them, two records are written — two of the
    expected ones —, the bytes behind them keep their poison, and the accumulators hold everything that is not on an edge"""
    name = 'aimed-127x33'
    case, img = edge_grid(name)
    want_acc, want_ev = F.expected_with_events(case)
    assert len(want_ev) >= 5
    got = fused_launch(name, case.xedges, case.yedges, img, float('-inf'), events=2)
    assert got['count'] == len(want_ev)
    assert len(got['records']) == 2
    pool = [tuple(r) for r in want_ev.tolist()]
    a, b = (tuple(r) for r in got['records'].tolist())
    assert a in pool and b in pool and a != b
    assert_planes(name, got['acc'], want_acc)
    full = fused_launch(name, case.xedges, case.yedges, img, float('-inf'), events=EVENT_ROOM)
    assert np.array_equal(F.sorted_events(full['records']), want_ev)


def test_the_elevation_threshold_is_inclusive():
    """bbox_min_elevation at one pixel's elevation bits keeps the pixel, the next double above drops it"""
    name = 'ownership-64x17'
    arrays = first_launch(name)
    g = next(g for g in grids_of(name) if g['tag'] == 'inside-interior-0.125')
    e = float(np.ravel(arrays['elev'])[g['pixel']])
    counts = []
    for threshold in (e, float(np.nextafter(e, np.inf))):
        gg = dict(g, min_elevation=threshold)
        case = case_for(name, gg, np.uint16)
        assert bool(case.keep()[g['pixel']]) == (threshold == e)
        want = F.expected_planes(case)
        assert_planes('threshold %r' % threshold, launch_grid(name, gg, case)['acc'], want)
        counts.append(int(want[0].sum()))
    assert counts[0] == counts[1] + 1


@pytest.mark.parametrize('name', ['ownership-64x17', 'ownership-127x33', 'ownership-3x1'])
def test_output_pointers_and_row_layout_leave_the_planes_alone(name):
    """per-pixel output pointers NULL or given, rows contiguous or strip-padded: the same planes and records, bit for bit"""
    first = first_launch(name)
    for g in [g for g in grids_of(name) if g['kind'] in ('shape', 'anchor') or g['tag'].startswith(('zone', 'eq'))]:
        case = case_for(name, g, np.uint8)
        base = launch_grid(name, g, case, events=EVENT_ROOM)
        for outputs in ('contiguous', 'padded'):
            got = launch_grid(name, g, case, events=EVENT_ROOM, outputs=outputs)
            assert np.array_equal(got['acc'], base['acc']), (name, g['tag'], outputs)
            assert np.array_equal(F.sorted_events(got['records']), F.sorted_events(base['records'])), (name, g['tag'], outputs)
            if outputs == 'contiguous':
                want = ('lat', 'lon', 'lat_c', 'lon_c', 'elev')
                for k in want:
                    assert same_bits(got['arrays'][k], first[k]), (name, g['tag'], k)


# ---- 2. camera-model variants ------------------------------------------------------------------------------------------------
CAMERA_VARIANTS = {
    # name: (camera of tests/_camera_cases.py, bin_magnetic, bin_pole, SECOND of the kernel variant)
    'mlat-mlt-only': ('cd-64x17', True, False, 4),
    'exact-centres': ('exact-diagonal+37', False, False, 0),
    'pole': ('pole', False, True, 2),
    'pole-magnetic': ('pole', True, True, 3),
}


def camera_coordinates(variant):
    """(x, y, elev, keep) as the variant bins them, from the arrays of the plain entry point: (SM longitude, MLat), (lon_c, lat_c)
    of pixels whose four corners hit (exact centres: corners_ok), or either pair through amt_rotate_pole_deg (the pole plans)"""
    from test_gpu_camera_rows import launch
    from auromat_amd.resample import _rotate_pole_dev
    name, magnetic, pole, _ = CAMERA_VARIANTS[variant]
    c, arrays = CK.by_name(name), launch(name)['arrays']
    x, y = F.binned_xy(arrays, magnetic)
    if pole:
        ctx = _ctx()
        la, lo = _rotate_pole_dev(ctx, ctx.to_device(y), ctx.to_device(x), c['altitude'], 90)
        x, y = lo.cpu().numpy(), la.cpu().numpy()
    hit = ~np.isnan(arrays['lat'])
    keep = (hit[:-1, :-1] & hit[:-1, 1:] & hit[1:, 1:] & hit[1:, :-1]).ravel() if not c['fast_center'] else None
    return x, y, arrays['elev'], keep


@pytest.mark.parametrize('variant', sorted(CAMERA_VARIANTS))
def test_camera_model_variants(variant):
    """amt_georef_frame with bin_acc: the MLat / MLT-only mode (SECOND = 4), exact centres (fast_center = 0: a pixel is binned
    only when its four corners hit), and the two pole plans, whose binned coordinates are amt_rotate_pole_deg of the first
    launch's centre arrays (the kernel promises to recompute exactly these next to an edge: the relations eq, below1 and
    above1 hold it to that) — without and with an event list, on every class grid"""
    name, magnetic, pole, second = CAMERA_VARIANTS[variant]
    c = CK.by_name(name)
    h, w = c['height'], c['width']
    x, y, elev, keep = camera_coordinates(variant)
    min_elevation = float(np.round(np.nanpercentile(elev, 25), 3))
    gl = F.class_grids(x, y, elev, h, w, min_elevation, keep)
    # (the rotated coordinates of the pole plans lie next to 0: an edge k steps up an axis cannot take every double next to
    # them, so a few of the exact relations exist at the first edge only)
    assert len(gl) >= 30 and {g['rel'] for g in gl} == set(F.RELATIONS), [g['tag'] for g in gl]
    assert {g['tag'].split('-')[1] for g in gl} == set(F.POSITIONS)
    if keep is not None:
        assert int((~keep & ~np.isnan(np.ravel(elev))).sum()) >= 20          # centres that hit while a corner misses
    n_records = 0
    for i, g in enumerate(gl):
        assert F.relation(float(x[g['pixel']]), g['xedges'], g['k_x']) == g['rel']
        assert F.relation(float(y[g['pixel']]), g['yedges'], g['k_y']) == g['rel']
        dtype = DTYPES[i % 2]
        case = F.as_case(g['tag'], x, y, elev, F.image_of(name, w, h, dtype), g['xedges'], g['yedges'], min_elevation, keep)
        kw = dict(magnetic=magnetic, camera=dict(pole=pole))
        got = fused_launch(name, g['xedges'], g['yedges'], case.img.reshape(h, w, 3), min_elevation, **kw)
        assert tuple(got['variant'][:2]) == (second, 1 + i % 2), got['variant']
        assert_planes('%s %s' % (variant, g['tag']), got['acc'], F.expected_planes(case))
        want_acc, want_ev = F.expected_with_events(case)
        got = fused_launch(name, g['xedges'], g['yedges'], case.img.reshape(h, w, 3), min_elevation, events=EVENT_ROOM, **kw)
        assert got['count'] == len(want_ev)
        assert np.array_equal(F.sorted_events(got['records']), want_ev), (variant, g['tag'])
        assert_planes('%s %s with events' % (variant, g['tag']), got['acc'], want_acc)
        n_records += len(want_ev)
    assert n_records >= 8
    print(variant, len(gl), 'grids,', n_records, 'records')


# ---- 3. / 4. event resolution through the pipeline, on aimed fields ----------------------------------------------------------
def oracle_frame(name):
    """_bin_oracle.frame on the final grid of an aimed field, from the device's arrays"""
    case, img = edge_grid(name)
    return B.frame(case), case, img


def assert_grid(tag, res, want):
    ny, nx = want['count'].shape
    assert res['mean'].shape == (ny, nx, 4), (tag, res['mean'].shape, (ny, nx))
    assert np.array_equal(np.asarray(res['count']), want['count_f']), (tag, 'count')
    assert np.array_equal(np.asarray(res['img']), want['img']), (tag, 'img')
    assert np.array_equal(np.asarray(res['mask']).astype(np.uint8), want['mask']), (tag, 'mask')
    assert same_bits(np.asarray(res['mean']), want['mean']), (tag, 'mean')


def check_aims(name):
    """every aimed centre of the DEVICE lies where the case says (within 1e-9 deg: the class cannot change)"""
    c, arrays = F.aimed_case(name), first_launch(name)
    x, y = F.binned_xy(arrays, c['magnetic'])
    w, on_edge = c['width'], 0
    for a in c['aims']:
        i = a['pixel'][0] * w + a['pixel'][1]
        for v, edges, k in ((x[i], c['xedges'], a['ix']), (y[i], c['yedges'], a['iy'])):
            if k is not None:
                assert abs((v - edges[k]) - a['offset']) < 1e-9, (name, a, v - edges[k])
        on_edge += int(a['offset'] in (F.AIM_ON_EDGE, F.AIM_BOTH))
    return on_edge


@pytest.mark.parametrize('name', F.aimed_names())
def test_event_resolution_through_the_pipeline(name):
    """run(fuse=True) (amt_pipe_finalize with k_apply_bin_events), run(fuse=False) and _bin_oracle.frame on the final grid:
    count, img and mask equal in every cell, mean bit for bit.  aimed-scale*, aimed-finer: the final grid rounds one decimal
    coarser / finer than its superset; the kernel records the pixels under every reading (inside the band at the superset's
    end) and k_apply_bin_events takes the final grid's: the frame stays with the single-pass plan and every cell agrees."""
    from auromat_amd.pipeline import FramePipeline
    c = F.aimed_case(name)
    on_edge = check_aims(name)
    want, case, img = oracle_frame(name)
    _, _, flags = F.bins_and_flags(case)
    pipe = FramePipeline(c['width'], c['height'], with_mag=True)
    p = frame_params(c)
    res, plans, edge_pixels = [], [], None
    for fuse in (True, False):
        r = pipe.run(None, c['altitude'], None, None, img=img, fast=True, min_elevation=None, pxPerDeg=c['ppd'], params=p,
                     fuse=fuse, dirs=dirs_of(name), magnetic=c['magnetic'])
        plans.append(pipe.last_plan)
        if fuse:
            edge_pixels = int(pipe._fused['result'].edge_pixels)
        res.append({k: np.array(r[k]) for k in ('mean', 'count', 'img', 'mask')})
    print(name, plans, res[0]['mean'].shape, 'edge_pixels', edge_pixels, 'flagged on the final grid', int((flags > 0).sum()))
    assert_grid(name + ' two-pass', res[1], want)
    assert_grid(name + ' fused', res[0], want)
    for k in res[0]:
        assert same_bits(res[0][k], res[1][k]), (name, k)
    assert plans == ['single-pass', 'two-pass'], (name, plans)
    assert edge_pixels >= on_edge


def test_a_poor_estimate_is_handed_back_once_and_then_fused():
    """The hand-back of amt_pipe_wait for a final grid that rounds coarser than its superset AND ends below the band: the
    aimed-scale field launched with an estimate three degrees too large to the north and east.  FramePipeline.resample launches
    it once more with the exact box as the estimate; the final grid then ends inside the band, the frame is finalised by the
    single-pass plan and equals the oracle.  The same estimate on a field whose scales agree is not handed back."""
    from auromat_amd.pipeline import FramePipeline
    for name, handed_back in (('aimed-scale', True), ('aimed-64x17', False)):
        c = F.aimed_case(name)
        want, case, img = oracle_frame(name)
        pipe = FramePipeline(c['width'], c['height'])
        pipe.set_image(img)
        p, ppd = frame_params(c), (c['ppd'], c['ppd'])
        b = F.box_of(first_launch(name))
        pipe.start_coarse(p, None, False, hint=[b[0], b[1] + 3.0, b[2], b[3] + 3.0, b[2], b[3] + 3.0, float(case.lat.size), 0.0])
        pipe.georef(None, c['altitude'], None, None, True, None, params=p, fuse_pxPerDeg=ppd, coarse_started=True,
                    dirs=dirs_of(name), pole_in_view=0)
        first = pipe._wait_fused()
        assert first.fused == 1 and first.status == (1 if handed_back else 0), (name, first.status)
        r = pipe.resample(ppd)
        assert pipe.last_plan == 'single-pass' and bool(pipe._fused.get('retried')) == handed_back
        assert pipe._wait_fused().status == 0
        assert_grid(name, {k: np.array(r[k]) for k in ('mean', 'count', 'img', 'mask')}, want)


@pytest.mark.parametrize('names', [F.THREE_FRAMES, tuple(sorted(F.SCALE_CASES)), (F.FINER_CASE,) * 3],
                         ids=['eighth', 'scale', 'finer'])
def test_three_frames_in_one_launch(names):
    """FramePipeline.georef_many(dirs=...) + fused_ready + finalize_many (k_pipe_finish; the per-frame constant blocks of
    k_georef_rows with events): three different aimed fields, each with its own on-edge pixels, against single run(fuse=True)
    calls and the oracle on the final grids; and the three aimed-scale fields, whose final grids round coarser on x, on y and
    on both (k_pipe_finish with the coarser reading's masks), and the field whose final grid rounds finer, three times"""
    from auromat_amd.pipeline import FramePipeline
    cs = [F.aimed_case(n) for n in names]
    ppd = cs[0]['ppd']
    w, h = cs[0]['width'], cs[0]['height']
    oracles = [oracle_frame(n) for n in names]
    single = []
    one = FramePipeline(w, h)
    for n, c, (want, case, img) in zip(names, cs, oracles):
        r = one.run(None, c['altitude'], None, None, img=img, fast=True, min_elevation=None, pxPerDeg=ppd, params=frame_params(c),
                    fuse=True, dirs=dirs_of(n))
        assert one.last_plan == 'single-pass'
        single.append({k: np.array(r[k]) for k in ('mean', 'count', 'img', 'mask')})
    pipes = [FramePipeline(w, h) for _ in names]
    ps = [frame_params(c) for c in cs]
    ds = [dirs_of(n) for n in names]
    for q, p, d, (want, case, img) in zip(pipes, ps, ds, oracles):
        q.use_image(device_image(img))
        q.start_coarse(p, None, False, dirs=d)
    FramePipeline.georef_many(pipes, ps, 110.0, None, (ppd, ppd), False, dirs=ds, pole_in_view=0)
    ready = [q.fused_ready((ppd, ppd), False) for q in pipes]
    assert all(r is not None for r in ready)
    events = [int(r.edge_pixels) for r in ready]
    out = FramePipeline.finalize_many(pipes, ready, (ppd, ppd), False)
    print('edge_pixels per frame', events)
    for n, q, a, b, (want, case, img), ne in zip(names, pipes, out, single, oracles, events):
        assert q.last_plan == 'single-pass'
        assert ne >= check_aims(n)
        for k in b:
            assert same_bits(np.array(a[k]), b[k]), (n, k)
        assert_grid(n, a, want)
