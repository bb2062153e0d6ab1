"""
The core role of k_georef_rows' work items (kRoleCore; amt_prm::core_frame_ok) leaves every bit: a launch whose
roles go up to core, the same launch stopped at inner (amt_georef_set_roles(ctx, 2)) and the forced-generic one
(amt_georef_set_roles(ctx, 0)) give the same five or nine arrays, the same eight doubles of the box (its count among them), the
same accumulators and the same on-edge records — for every variant <fast | exact, SECOND 0 | 1 | 4, BIN 0 | 1 | 2> and both row
layouts —, and the sequence runner the same grids.

The frame is the smallest with a core item: 200 x 96 pixels (4 strips, 6 bands), a camera 400 km up looking at the nadir, 0.01 deg
per pixel (tests/test_core_role_cpu.py holds the rule to the oracle on this camera): every band is inner, bands 1 - 4 are core,
their two middle strips take the core loop.  The MLat / MLT-only variants (SECOND = 4) reduce the box over (MLat, SM longitude),
which the rule does not bound: they have no core item, and the test says so.  The rule must also decline with the prime meridian
or the date line through the middle of the frame, with a NaN threshold and for caller-supplied directions.
"""
import ctypes as C

import numpy as np
import pytest

import _band_role_cases as R
import _camera_cases as K
from test_core_role_cpu import H, W, aimed, core_bands, core_strips

pytestmark = pytest.mark.gpu

MIN_ELEV = 10.0
BIN_ID = {None: 0, np.uint8: 1, np.uint16: 2}
MODES = (('core', 1), ('inner', 2), ('generic', 0))
_EDGES = {}


def last_core(ctx):
    v = C.c_int64(-7)
    ctx.call('amt_georef_last_core', C.byref(v))
    return v.value


def launch(mode, p, second, bin_dtype, padded, edges=None, min_elev=MIN_ELEV):
    """_band_role_cases.launch_frame with amt_georef_set_roles(ctx, mode): launch_frame passes its `roles` through set_roles of
    its module, which maps it to 0 / 1; for the length of the call it passes the number on instead"""
    orig = R.set_roles
    R.set_roles = lambda ctx, on: ctx.call('amt_georef_set_roles', int(on))
    try:
        res = R.launch_frame(W, H, p, second, bin_dtype, padded, mode, edges, min_elev)
    finally:
        R.set_roles = orig
    res['core'] = last_core(R._ctx())
    return res


def edges_of(tag, p, second, step):
    """uniform edges around the frame's centre coordinates, `step` degrees on round numbers"""
    key = (tag, second, step)
    if key not in _EDGES:
        a = launch(0, p, second, None, False)['arrays']
        if second == 4:
            x, y = (a['mlt_c'].view(np.float64) - 12.0) / (24.0 / 360.0), a['mlat_c'].view(np.float64)
        else:
            x, y = a['lon_c'].view(np.float64), a['lat_c'].view(np.float64)

        def edges(v):
            lo, hi = np.floor(np.nanmin(v) / step - 1.0), np.ceil(np.nanmax(v) / step + 1.0)
            return np.linspace(lo * step, hi * step, int(hi - lo) + 1)      # (step is a power of two: the edges are exact)
        _EDGES[key] = (edges(x), edges(y))
    return _EDGES[key]


def three(tag, p, second, bin_dtype, padded, step=2.0 ** -7, min_elev=MIN_ELEV):
    edges = edges_of(tag, p, second, step) if bin_dtype is not None else None
    got = {name: launch(mode, p, second, bin_dtype, padded, edges, min_elev) for name, mode in MODES}
    for name in ('core', 'inner'):
        assert got[name]['variant'][:2] == (second, BIN_ID[bin_dtype]), (tag, name)
        R.assert_same((tag, name, 'against generic'), got[name], got['generic'])
    assert got['inner']['core'] == 0 and got['generic']['core'] == 0, (tag, got['inner']['core'], got['generic']['core'])
    assert got['core']['roles'] == got['inner']['roles'], (tag, 'core items count as inner ones')
    assert got['generic']['roles'][1:] == (0, 0)
    return got


VARIANTS = [(fast, second, b) for fast in (True, False) for second in (0, 1, 4) for b in (None, np.uint8, np.uint16)]


@pytest.mark.parametrize('padded', [False, True], ids=['contiguous', 'padded'])
@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: '%s-second%d-bin%d' % ('fast' if v[0] else 'exact', v[1], BIN_ID[v[2]]))
def test_core_items_leave_every_bit(variant, padded):
    fast, second, bin_dtype = variant
    c, _ = aimed('49', 0.0, 0.0)
    p = K.native_params(c, fast)
    cb, ce = core_bands(p, MIN_ELEV)
    assert (cb, ce) == (1, 5) and len(core_strips(W)) == 2
    got = three(('nadir', variant, padded), p, second, bin_dtype, padded)
    on = got['core']
    assert on['roles'][1] == 6 * 4, on['roles']                     # every item of the frame is inner
    if second == 4:
        assert on['core'] == 0                                      # the box in (MLat, SM longitude): no core item
    else:
        assert on['core'] == (ce - cb) * len(core_strips(W)) > 0, on['core']
    assert on['bbox'].view(np.float64)[6] == W * H                  # the count of valid pixels
    if bin_dtype is not None:
        n = on['acc'].size // 5
        assert int(on['acc'][:n].sum()) + on['count'] == W * H and int(on['acc'][:n].max()) < W * H
    print(variant, padded, 'core items', on['core'], 'of', on['roles'][1], 'inner; on-edge records', on.get('count'))


@pytest.mark.parametrize('kind', ['meridian', 'dateline', 'nan-threshold'])
def test_rule_declines(kind):
    c, _ = aimed('49' if kind == 'nan-threshold' else kind, 0.0, 0.0)
    thr = float('nan') if kind == 'nan-threshold' else MIN_ELEV
    for fast, second, bin_dtype, padded in ((True, 0, None, False), (True, 0, np.uint16, True), (False, 1, np.uint8, False)):
        p = K.native_params(c, fast)
        assert core_bands(p, thr) == (0, 0)
        got = three((kind, fast, second), p, second, bin_dtype, padded, step=0.25, min_elev=thr)
        assert got['core']['core'] == 0, (kind, got['core']['core'])
        if kind != 'nan-threshold':
            assert got['core']['roles'][1] == 6 * 4                 # inner all the same
            lon = got['core']['arrays']['lon'].view(np.float64)
            assert (lon > 0).any() and (lon < 0).any()              # the line runs through the frame
            box = got['core']['bbox'].view(np.float64)
            # (the box also holds the last corner row of every item as its own chain of small angles gives it, a few ulps from
            # the value the next item stores for the same corner: equal to rounding, not to the bit)
            assert box[4] > 0 >= box[5] and abs(box[4] - lon[lon > 0].min()) < 1e-9 and abs(box[5] - lon[lon <= 0].max()) < 1e-9


def test_direction_arrays_have_no_core_items():
    import torch
    from auromat_amd._native import GeorefOut
    ctx = R._ctx()
    c, _ = aimed('49', 0.0, 0.0)
    p = K.native_params(c, True)
    assert core_bands(p, MIN_ELEV) != (0, 0)
    dirs = ctx.empty((H + 1, W + 1, 3))
    ctx.call('amt_directions_tan', C.byref(p), 1, C.c_void_p(dirs.data_ptr()))
    bits = {}
    for name, mode in MODES:
        out = GeorefOut()
        lat, lon = ctx.empty((H + 1, W + 1)), ctx.empty((H + 1, W + 1))
        elev = ctx.empty((H, W))
        bbox = torch.full((8,), -1.0, dtype=torch.float64, device=ctx.device)
        out.lat, out.lon, out.elev, out.bbox, out.bbox_min_elevation = lat.data_ptr(), lon.data_ptr(), elev.data_ptr(), bbox.data_ptr(), MIN_ELEV
        ctx.call('amt_georef_set_roles', mode)
        try:
            ctx.call('amt_georef_frame_dirs', C.byref(p), C.c_void_p(dirs.data_ptr()), C.byref(out))
            torch.cuda.synchronize()
        finally:
            ctx.call('amt_georef_set_roles', 1)
        assert last_core(ctx) == 0 and R.last_roles(ctx)[1:] == (0, 0)
        bits[name] = [a.cpu().numpy().view(np.uint64) for a in (lat, lon, elev, bbox)]
    for name in ('core', 'inner'):
        for a, b in zip(bits[name], bits['generic']):
            assert np.array_equal(a, b), name


# ---- the sequence runner ------------------------------------------------------------------------------------------------------------
def test_runner_sequence_of_eight_frames():
    """eight frames of a nadir camera moving north-east, 300 x 200 pixels (5 strips, 13 bands; the runner of
    tests/test_gpu_sky_fill_reuse.py): the slots' arrays, the grids and the images are those of fresh forced-generic single-frame
    runs whether the roles go up to core or stop at inner, and the runner counts the core items"""
    import test_gpu_sky_fill_reuse as F
    ctx = R._ctx()
    frames = []
    for k in range(8):
        c = K.finish(K.camera('core-runner-%d' % k, 'core', F.W, F.H, lat=49.0 + 0.002 * k, lon=60.0 + 0.003 * k, height=400.0,
                              nadir_angle=0.0, scale=0.01, roll=2.0 * k))
        assert core_bands(K.native_params(c, True), F.MIN_ELEV) == (1, 12), c['name']
        frames.append((c['header'], np.array(c['cam']), c['time']))
    frames = F.with_images(frames)
    case = 'core-runner'
    ctx.call('amt_georef_set_roles', 0)
    try:
        cells = F.arena_cells(case, frames)             # (runs and keeps the fresh frames: forced generic)
    finally:
        ctx.call('amt_georef_set_roles', 1)
    items_per_frame = 11 * len(core_strips(F.W))
    assert items_per_frame == 33
    for name, mode in MODES[:2]:
        runner = F.Runner(batch=3)
        runner.ctx.call('amt_georef_set_roles', mode)
        try:
            runner.overwrite_slots()
            table, grids, images, _, _ = runner.call(frames, cells + 64)
            core = C.c_int64(-7)
            assert runner.lib.amt_run_core_stats(runner.run, C.byref(core)) == 0
            stats = [C.c_int64(-1) for _ in range(3)]
            assert runner.lib.amt_run_role_stats(runner.run, *[C.byref(s) for s in stats]) == 0
            # every band of these frames is inner: the inner count says how many frames were launched (a retried one twice)
            launched, rest = divmod(stats[1].value, 13 * 5)
            assert rest == 0 and launched >= len(frames) and stats[0].value == 0, (name, [s.value for s in stats])
            assert core.value == (items_per_frame * launched if name == 'core' else 0), (name, core.value, launched)
            F.check_call(runner, case, frames, table, grids, images)
        finally:
            runner.ctx.call('amt_georef_set_roles', 1)
            runner.close()
