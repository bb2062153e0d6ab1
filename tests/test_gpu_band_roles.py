"""
Roles of the frame kernel's work items (amt_prm::band_roles): with the roles the host rule names — inner rows
without the hit, threshold and keep tests, low rows without image, runs and box — every launch gives, BIT FOR BIT, what the
same launch gives with every row generic (amt_georef_set_roles(ctx, 0)): all arrays with their NaN pattern, the box and the
count of valid pixels, the accumulator planes, the on-edge records and, through the sequence runner, the final grids.

Frames: the cameras of tests/_band_role_cases.py at 200 x 120 and 130 x 50 (a last strip narrower than 63 columns, a last band
shorter than 16 rows), uint8 and uint16 images, contiguous and strip-padded rows, the kernel variants <fast | exact, SECOND 0 |
1 | 4, BIN 0 | 1 | 2> through amt_georef_frame, and 7-frame sequences through the runner (two slots, each revisited, one frame
launched twice).  amt_georef_last_roles / amt_run_role_stats say how many work items took each role: every variant must have
taken inner rows, every binning variant low rows, and a forced-generic launch none — so no comparison is vacuous.
"""
import ctypes as C

import numpy as np
import pytest

from _band_role_cases import (GEO, MAG, NINE, _ctx, assert_same, band_roles, cases, image, last_roles, launch_frame, role_of_bands,
                              set_roles)

pytestmark = pytest.mark.gpu

MIN_ELEV = 10.0
_GRIDS = {}


def params(case, fast, altitude=110.0):
    from auromat_amd.mapping.astrometry import frame_params
    _, w, h, hdr, cam, t = case
    return frame_params(hdr, altitude, cam, t, fast)


def launch(case, fast, second, bin_dtype, padded, roles, edges=None):
    """_band_role_cases.launch_frame on a case of this module at MIN_ELEV"""
    return launch_frame(case[1], case[2], params(case, fast), second, bin_dtype, padded, roles, edges, MIN_ELEV)


def grid_edges(case, fast, second):
    """Uniform edges around the frame's centre coordinates, quarter degrees on round numbers (pixels on an edge do occur)."""
    key = (case[0], fast, second)
    if key not in _GRIDS:
        a = launch(case, fast, second, None, False, False)['arrays']
        if second == 4:
            x, y = (a['mlt_c'].view(np.float64) - 12.0) / (24.0 / 360.0), a['mlat_c'].view(np.float64)
        else:
            x, y = a['lon_c'].view(np.float64), a['lat_c'].view(np.float64)
        if np.isnan(x).all():
            _GRIDS[key] = (np.linspace(-10.0, 10.0, 41), np.linspace(-10.0, 10.0, 41))
        else:
            def edges(v):
                lo, hi = np.floor(np.nanmin(v)) - 1.0, np.ceil(np.nanmax(v)) + 1.0
                return np.linspace(lo, hi, int(round((hi - lo) * 4)) + 1)
            _GRIDS[key] = (edges(x), edges(y))
    return _GRIDS[key]


def expected_items(case, fast, binning):
    """(generic, inner, low) work items by the host rule (low rows exist with fused binning only)"""
    _, w, h, hdr, cam, t = case
    r = band_roles(hdr, cam, t, MIN_ELEV, 110, fast)
    kinds = role_of_bands(r)
    inner, low = kinds.count('i'), kinds.count('l') if binning else 0
    earth = r['n'] - kinds.count('s')
    return tuple(int(v) * r['strips'] for v in (earth - inner - low, inner, low))


VARIANTS = [(fast, second, b) for fast in (True, False) for second in (0, 1, 4) for b in (None, np.uint8, np.uint16)]


@pytest.mark.parametrize('padded', [False, True], ids=['contiguous', 'padded'])
@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: '%s-second%d-bin%d' % ('fast' if v[0] else 'exact', v[1], {None: 0, np.uint8: 1, np.uint16: 2}[v[2]]))
def test_roles_leave_every_bit_of_a_frame(variant, padded):
    fast, second, bin_dtype = variant
    took = np.zeros(3, np.int64)
    binned = records = 0
    for case in cases():
        edges = grid_edges(case, fast, second) if bin_dtype is not None else None
        off = launch(case, fast, second, bin_dtype, padded, False, edges)
        on = launch(case, fast, second, bin_dtype, padded, True, edges)
        tag = (case[0], variant, padded)
        assert on['variant'][:2] == (second, {None: 0, np.uint8: 1, np.uint16: 2}[bin_dtype]), tag
        assert off['roles'][1:] == (0, 0), (tag, off['roles'])
        assert on['roles'] == expected_items(case, fast, bin_dtype is not None), (tag, on['roles'])
        assert sum(on['roles']) == sum(off['roles'])
        assert_same(tag, on, off)
        took += on['roles']
        if bin_dtype is not None:
            binned += int(on['acc'][:on['acc'].size // 5].sum())
            records += on['count']
    print(variant, padded, 'work items generic / inner / low:', took.tolist(), 'pixels binned', binned, 'on-edge records', records)
    assert took[1] > 0 and took[0] > 0
    if bin_dtype is not None:
        assert took[2] > 0 and binned > 0


def test_direction_arrays_and_pole_plans_have_no_roles():
    import torch
    from auromat_amd._native import GeorefOut
    from auromat_amd.synthetic import pole_frame
    from auromat_amd.util.histogram import make_axis
    ctx = _ctx()
    case = [c for c in cases() if c[0] == 'nadir 200x120'][0]
    _, w, h = case[:3]
    assert expected_items(case, True, False)[1] > 0                 # as a camera frame every row of it is inner
    p = params(case, True)
    dirs = ctx.empty((h + 1, w + 1, 3))
    ctx.call('amt_directions_tan', C.byref(p), 1, C.c_void_p(dirs.data_ptr()))
    out = GeorefOut()
    lat, lon = ctx.empty((h + 1, w + 1)), ctx.empty((h + 1, w + 1))
    out.lat, out.lon, out.bbox_min_elevation = lat.data_ptr(), lon.data_ptr(), MIN_ELEV
    ctx.call('amt_georef_frame_dirs', C.byref(p), C.c_void_p(dirs.data_ptr()), C.byref(out))
    torch.cuda.synchronize()
    g, i, l = last_roles(ctx)
    assert (i, l) == (0, 0) and g > 0, (g, i, l)
    # the pole plan (SECOND = 2)
    hdr, cam, t = pole_frame(w, h)
    pcase = ('pole', w, h, hdr, cam, t)
    pp = params(pcase, True)
    xa, kx = make_axis(ctx, np.linspace(-40.0, 40.0, 161), uniform=True)
    ya, ky = make_axis(ctx, np.linspace(-40.0, 40.0, 161), uniform=True)
    acc = torch.zeros(5 * xa.nbin * ya.nbin, dtype=torch.int64, device=ctx.device)
    out = GeorefOut()
    out.bbox_min_elevation = MIN_ELEV
    out.bin_acc, out.bin_img, out.bin_img_dtype = acc.data_ptr(), image(w, h, np.uint16).data_ptr(), 2
    out.bin_xaxis, out.bin_yaxis = C.addressof(xa), C.addressof(ya)
    out.bin_pole, out.altitude = 1, 110.0
    ctx.call('amt_georef_frame', C.byref(pp), C.byref(out))
    torch.cuda.synchronize()
    assert ctx.last_variant()[:2] == (2, 2)
    g, i, l = last_roles(ctx)
    assert (i, l) == (0, 0) and g > 0, (g, i, l)
    del kx, ky


# ---- the sequence runner -----------------------------------------------------------------------------------------------------------

def retried_sequence():
    """The seven frames of tests/test_gpu_sky_fill_reuse.py's retry case: one frame per launch, two slots, frame 2 launched twice."""
    from test_gpu_sky_fill_reuse import H, W, with_images
    from auromat_amd.synthetic import sequence_frame
    hdr, cam, t, _ = sequence_frame(0, W, H)
    v = np.cross([0.0, 0.0, 1.0], cam / np.linalg.norm(cam))
    far = (hdr, cam + 95.0 * np.sign(v + 1e-9), t)
    near = (hdr, cam, t)
    return with_images([near, near, far, near, far, near, near], altitudes=[110.0, 110.0, 100.0, 110.0, 100.0, 110.0, 110.0])


@pytest.mark.parametrize('setup', [(GEO, False, False), (GEO, False, True), (MAG, True, False), (NINE, True, False)],
                         ids=['geodetic', 'geodetic-padded', 'mlat-mlt-only', 'nine-arrays-magnetic'])
def test_roles_leave_every_bit_of_a_sequence(setup):
    from test_gpu_sky_fill_reuse import Runner
    names, magnetic, padded = setup
    frames = retried_sequence()
    got = {}
    for roles in (False, True):
        runner = Runner(batch=1, names=names, magnetic=magnetic, padded=padded)
        set_roles(runner.ctx, roles)
        try:
            runner.overwrite_slots()
            table, grids, images, _, _ = runner.call(frames, 400000)
            stats = [C.c_int64(-1) for _ in range(3)]
            assert runner.lib.amt_run_role_stats(runner.run, *[C.byref(s) for s in stats]) == 0
            got[roles] = dict(table=table, grids=grids.view(np.uint64), images=images, stats=tuple(s.value for s in stats),
                              slots=[runner.slot_bits(s) for s in range(runner.n_slots)])
        finally:
            set_roles(runner.ctx, True)
            runner.close()
    on, off = got[True], got[False]
    print(setup[1:], 'work items generic / inner / low: roles', on['stats'], 'forced generic', off['stats'])
    assert off['stats'][1:] == (0, 0) and on['stats'][1] > 0 and on['stats'][2] > 0 and sum(on['stats']) == sum(off['stats'])
    assert on['table']['retried'].tolist() == off['table']['retried'].tolist() and on['table']['retried'][2] == 1
    assert (on['table']['status'] == 0).all() and (off['table']['status'] == 0).all()
    for field in ('status', 'ny', 'nx', 'edge_pixels', 'grid_offset', 'image_offset', 'lon_wrapped', 'contains_pole'):
        assert on['table'][field].tolist() == off['table'][field].tolist(), field
    assert np.array_equal(on['table']['bbox'].view(np.uint64), off['table']['bbox'].view(np.uint64))
    last = on['table'][-1]
    used = int(last['grid_offset']) + 5 * int(last['ny']) * int(last['nx'])
    assert np.array_equal(on['grids'][:used], off['grids'][:used])
    used = int(last['image_offset']) + 7 * int(last['ny']) * int(last['nx'])
    assert np.array_equal(on['images'][:used], off['images'][:used])
    for s in range(len(on['slots'])):
        for name in names:
            assert np.array_equal(on['slots'][s][name], off['slots'][s][name]), (s, name)
