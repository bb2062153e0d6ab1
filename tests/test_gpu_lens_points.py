"""
amt_world_to_pixel_lens and amt_grid_to_pixel_lens (auromat_amd/csrc/amt_inverse.hip; step 9 in amt_w2p.h) on the point cases of
tests/_lens_gather_cases.py — five cameras x eight lens models x (no crop, crop) x the cameras' own points in the three frames —
against the mpmath composition of tests/_inverse_oracle.py (steps 1-8) and the lens forward in mpmath (step 9).
tests/test_lens_gather_cpu.py checks the statement and that at most 1 % of the points are ambiguous without a GPU.

Bounds.  The flags must be equal on every point that is not ambiguous.  The xy bound is 4 x the largest distance measured on the
MI355X against the mpmath composition of the same float64 inputs, the convention of tests/test_gpu_inverse_points.py:
  pixels      measured 1.130e-10 px (model 'magnify', whose slope d(r g)/dr reaches 20 at the frames' corners and stretches
              what steps 1-8 leave; every other model stays below 1.1e-11 px), bound 4.52e-10 px
The test prints what it measured (-s).
"""
import ctypes as C

import numpy as np
import pytest

import _inverse_cases as IC
import _inverse_oracle as O
import _lens_gather_cases as G

pytestmark = pytest.mark.gpu

MEASURED_PX = 1.130e-10    # largest distance measured on the MI355X [px] (camera 'dateline', model 'magnify', geodetic)
ACCURACY_PX = 4 * MEASURED_PX
POISON, SPARE, EINVAL = -1234.5, 64, -1


@pytest.fixture(scope='module')
def ctx():
    from auromat_amd._native import Context
    return Context.current()


def ref(x):
    return None if x is None else C.byref(x)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def run_points(ctx, native, frame, c0, c1, lens='old'):
    """amt_world_to_pixel_lens (lens='old': amt_world_to_pixel) into poisoned buffers -> (xy (n, 2), elev (n), flags (n))"""
    import torch
    from auromat_amd._native import ptr, to_host
    p, z = native
    n = len(c0)
    a, b = ctx.to_device(np.ascontiguousarray(c0, dtype=np.float64)), ctx.to_device(np.ascontiguousarray(c1, dtype=np.float64))
    xy = torch.full((2 * n + SPARE,), POISON, dtype=torch.float64, device=ctx.device)
    el = torch.full((n + SPARE,), POISON, dtype=torch.float64, device=ctx.device)
    fl = torch.full((n + SPARE,), 0xA5, dtype=torch.uint8, device=ctx.device)
    args = (C.byref(p), ref(z), frame, ptr(a), ptr(b), n, ptr(xy), ptr(el), ptr(fl))
    if isinstance(lens, str):
        ctx.call('amt_world_to_pixel', *args)
    else:
        ctx.call('amt_world_to_pixel_lens', *(args + (ref(lens),)))
    xy_h, el_h, fl_h = to_host(xy), to_host(el), to_host(fl)
    assert (xy_h[2 * n:] == POISON).all() and (el_h[n:] == POISON).all() and (fl_h[n:] == 0xA5).all()
    return xy_h[:2 * n].reshape(n, 2), el_h[:n], fl_h[:n]


def run_grid(ctx, native, frame, lat, lon, lens='old'):
    """amt_grid_to_pixel_lens (lens='old': amt_grid_to_pixel) -> (xy32, xy, elev, flags) host arrays (ny, nx[, 2])"""
    import torch
    from auromat_amd._native import ptr, to_host
    p, z = native
    ny, nx = len(lat), len(lon)
    a, b = ctx.to_device(np.ascontiguousarray(lat, dtype=np.float64)), ctx.to_device(np.ascontiguousarray(lon, dtype=np.float64))
    xy32 = torch.full((ny, nx, 2), POISON, dtype=torch.float32, device=ctx.device)
    xy = torch.full((ny, nx, 2), POISON, dtype=torch.float64, device=ctx.device)
    el = torch.full((ny, nx), POISON, dtype=torch.float64, device=ctx.device)
    fl = torch.full((ny, nx), 0xA5, dtype=torch.uint8, device=ctx.device)
    args = (C.byref(p), ref(z), frame, ptr(a), ny, ptr(b), nx, ptr(xy32), ptr(xy), ptr(el), ptr(fl))
    if isinstance(lens, str):
        ctx.call('amt_grid_to_pixel', *args)
    else:
        ctx.call('amt_grid_to_pixel_lens', *(args + (ref(lens),)))
    return to_host(xy32), to_host(xy), to_host(el), to_host(fl)


# ---- accuracy and flags -----------------------------------------------------------------------------------------------------------
def test_against_mpmath(ctx):
    worst, where, n_points, n_unsure = 0.0, None, 0, 0
    per_model = {}
    for camera, model, crop, frame in G.point_cases():
        r = G.points(camera, model, crop, frame)
        cam, lens = IC.by_name(camera), r['lens']
        p, z, ln = G.native(cam, lens)
        xy, elev, flags = run_points(ctx, (p, z), dict(IC.FRAMES)[frame], r['c0'], r['c1'], ln)
        what = (camera, model, crop, frame)
        sure = r['sure']
        assert np.array_equal(flags[sure], r['flags'][sure]), (what, flags, r['flags'])
        no_pixel = (flags & G.NO_PIXEL) != 0
        assert np.array_equal(np.isnan(xy[:, 0]), no_pixel) and np.array_equal(np.isnan(xy[:, 1]), no_pixel), what
        both = sure & ~no_pixel
        d = np.where(both, np.hypot(xy[:, 0] - r['x'], xy[:, 1] - r['y']), 0.0)
        per_model[model] = max(per_model.get(model, 0.0), float(d.max()))
        if d.max() > worst:
            worst, where = float(d.max()), what
        # the elevation is that of steps 1-8: the bits of the call without a lens
        plain = run_points(ctx, IC.native(cam), dict(IC.FRAMES)[frame], r['c0'], r['c1'])
        assert same_bits(elev, plain[1]), what
        n_points += len(d)
        n_unsure += int((~sure).sum())
    print('%d points (%d ambiguous, left out of the flags); largest distance from mpmath %.3e px %r; per model: %s'
          % (n_points, n_unsure, worst, where, ', '.join('%s %.2e' % kv for kv in sorted(per_model.items()))))
    assert worst <= ACCURACY_PX


# ---- the same bits as without a lens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('camera', G.CAMERAS)
def test_no_lens_gives_the_bits_of_the_old_entry_points(ctx, camera):
    from auromat_amd._native import LensModel
    cam = IC.by_name(camera)
    none = LensModel()                                      # kind AMT_LENS_NONE; its other fields are not read
    none.width, none.height, none.crop_x = -3, 0, 99
    identity = G.native_lens(G.lens_of(cam, 'identity', False))
    for frame, code in IC.FRAMES:
        r = IC.points(camera)[frame]
        want = run_points(ctx, IC.native(cam), code, r['c0'], r['c1'])
        assert frame == 'j2000' or (want[2] == 0).any()
        for lens in (None, none, identity):
            got = run_points(ctx, IC.native(cam), code, r['c0'], r['c1'], lens)
            for a, b in zip(got, want):
                assert same_bits(a, b), (camera, frame, lens and lens.kind)
        lat, lon = np.sort(r['c0'][:7]), r['c1'][:9]
        want = run_grid(ctx, IC.native(cam), code, lat, lon)
        for lens in (None, none, identity):
            got = run_grid(ctx, IC.native(cam), code, lat, lon, lens)
            for a, b in zip(got, want):
                assert same_bits(a, b), (camera, frame, lens and lens.kind)


# ---- grid form and point form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', G.MODELS)
def test_grid_form_is_the_point_form(ctx, model):
    """a 19 x 1031 outer product (more than one work item of the grid kernel each way, with tails): the bits of the point form,
    and out_xy32 the float64 rounded once"""
    cam = IC.by_name('sip-2')
    for crop in (False, True):
        lens = G.lens_of(cam, model, crop)
        p, z, ln = G.native(cam, lens)
        pts = IC.points('sip-2')['geodetic']
        lat = np.linspace(pts['c0'].min() - 0.3, pts['c0'].max() + 0.3, 19)
        lon = np.linspace(pts['c1'].min() - 0.3, pts['c1'].max() + 0.3, 1031)
        xy32, xy, el, fl = run_grid(ctx, (p, z), O.GEODETIC, lat, lon, ln)
        la, lo = np.meshgrid(lat, lon, indexing='ij')
        pxy, pel, pfl = run_points(ctx, (p, z), O.GEODETIC, la.ravel(), lo.ravel(), ln)
        assert same_bits(xy.reshape(-1, 2), pxy) and same_bits(el.ravel(), pel) and same_bits(fl.ravel(), pfl), (model, crop)
        assert same_bits(xy32, xy.astype(np.float32)), (model, crop)
        if model == 'nan':
            assert ((fl & G.LENS_FOLD) != 0)[(fl & O.NO_PIXEL) == 0].all()
        elif model == 'fold':
            assert (fl & G.LENS_FOLD).any() and (fl == 0).any()
        else:
            assert not (fl & G.LENS_FOLD).any() and (fl == 0).any()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_lens_argument_errors_write_nothing(ctx):
    import torch
    from auromat_amd._native import ptr
    cam = IC.by_name('sip-2')                               # with a zenithal block: the corrected size can be checked
    good = G.lens_of(cam, 'poly3', True)
    pts = IC.points('sip-2')['geodetic']
    n = len(pts['c0'])
    a, b = ctx.to_device(pts['c0'].copy()), ctx.to_device(pts['c1'].copy())
    xy = torch.full((n, 2), POISON, dtype=torch.float64, device=ctx.device)
    fl = torch.full((n,), 0xA5, dtype=torch.uint8, device=ctx.device)
    xy32 = torch.full((n, n, 2), POISON, dtype=torch.float32, device=ctx.device)
    gfl = torch.full((n, n), 0xA5, dtype=torch.uint8, device=ctx.device)

    def calls(p, z, ln):
        last = lambda: (ctx._lib.amt_last_error(ctx.handle) or b'').decode()            # noqa: E731
        rc1 = ctx._lib.amt_world_to_pixel_lens(ctx.handle, C.byref(p), ref(z), O.GEODETIC, ptr(a), ptr(b), n, ptr(xy), None, ptr(fl),
                                               C.byref(ln))
        e1 = last()
        rc2 = ctx._lib.amt_grid_to_pixel_lens(ctx.handle, C.byref(p), ref(z), O.GEODETIC, ptr(a), n, ptr(b), n, ptr(xy32), None, None,
                                              ptr(gfl), C.byref(ln))
        return (rc1, e1), (rc2, last())

    def variant(**kw):
        p, z, ln = G.native(cam, good)
        for k, v in kw.items():
            if k in ('pw', 'ph'):
                setattr(p, 'width' if k == 'pw' else 'height', v)
            elif k in ('zw', 'zh'):
                setattr(z, 'width' if k == 'zw' else 'height', v)
            else:
                setattr(ln, k, v)
        return p, z, ln
    W, H = good['width'], good['height']
    cases = [(dict(kind=4), 'unknown lens kind'), (dict(kind=-1), 'unknown lens kind'), (dict(width=0, pw=0), 'empty'),
             (dict(height=-2), 'empty raw frame'), (dict(crop_x=W - 10), 'crop window'), (dict(crop_y=-1), 'crop window'),
             (dict(crop_width=0), 'crop window'), (dict(crop_height=H + 1), 'crop window'),
             (dict(pw=W + 1), "params' width x height"), (dict(ph=H - 1), "params' width x height"),
             (dict(zw=cam['width'] + 1), "camera model's"), (dict(crop_height=cam['height'] - 1), "camera model's")]
    for kw, word in cases:
        for (rc, err), name in zip(calls(*variant(**kw)), ('amt_world_to_pixel_lens', 'amt_grid_to_pixel_lens')):
            assert rc == EINVAL and word in err and err.startswith(name + ': '), (kw, err)
    ctx.synchronize()
    assert (xy == POISON).all() and (fl == 0xA5).all() and (xy32 == POISON).all() and (gfl == 0xA5).all()
    for rc, err in calls(*variant()):
        assert rc == 0, err
    ctx.synchronize()
    assert not (fl == 0xA5).all() and not (gfl == 0xA5).all()
