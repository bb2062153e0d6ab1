"""
amt_world_to_pixel and amt_grid_to_pixel (auromat_amd/csrc/amt_inverse.hip) on the cameras and points of tests/_inverse_cases.py,
against the mpmath statement of tests/_inverse_oracle.py; tests/test_inverse_cpu.py shows without a GPU that the statement inverts
the forward direction and that no point's flags are ambiguous.

Bounds.  The accuracy bounds are 4 x the largest distance measured on the MI355X against the mpmath inverse of the same float64
inputs (the margin covers the spread between compilers and libm versions); every point of every camera and frame is compared,
none is left out, and the flags must be equal on all of them:
  pixels      measured 2.16e-11 px (geodetic 1.75e-11, MLat / SM longitude 2.16e-11, both on the camera 2.5 km above the shell;
              right ascension / declination 4.9e-13), bound 8.64e-11 px
  elevation   measured 1.07e-12 deg (geodetic 3.7e-13), bound 4.28e-12 deg
The round trip through the forward kernel (exact centres of amt_georef_frame, inverted, against the pixel indices) is held to the
Bowring residual that tests/test_inverse_cpu.py measures (the forward takes one Bowring step, the inverse inverts the exact
latitude: 9.302e-9 px) plus ACCURACY_PX, 9.39e-9 px; measured over the 208 683 hit pixels of the plain TAN cameras: geodetic
9.22e-9 px (the Bowring residual itself, on the camera 2.5 km above the shell), MLat / MLT 5.6e-10 px.  Every test prints what it
measured (-s).
"""
import ctypes as C

import numpy as np
import pytest

import _inverse_cases as IC
import _inverse_oracle as O

pytestmark = pytest.mark.gpu

MEASURED_PX, MEASURED_DEG = 2.160e-11, 1.071e-12      # largest distances measured on the MI355X (SM frame, low-horizon)
ACCURACY_PX, ACCURACY_DEG = 4 * MEASURED_PX, 4 * MEASURED_DEG
SPARE = 64
POISON = -1234.5
EINVAL = -1


@pytest.fixture(scope='module')
def ctx():
    from auromat_amd._native import Context
    return Context.current()


def zen_ref(z):
    return None if z is None else C.byref(z)


def run_points(ctx, cam, frame, c0, c1, elev=True, native=None, xy_offset=0):
    """amt_world_to_pixel into poisoned buffers with a spare tail -> (xy (n, 2), elev (n) or None, flags (n)); asserts that
    nothing beyond n was written.  xy_offset: doubles by which the xy buffer is shifted (1: an address that is no multiple of 16)"""
    import torch
    from auromat_amd._native import ptr, to_host
    p, z = native or IC.native(cam)
    n = len(c0)
    a = ctx.to_device(np.ascontiguousarray(c0, dtype=np.float64)) if n else None
    b = ctx.to_device(np.ascontiguousarray(c1, dtype=np.float64)) if n else None
    xy = torch.full((2 * n + SPARE + xy_offset,), POISON, dtype=torch.float64, device=ctx.device)
    el = torch.full((n + SPARE,), POISON, dtype=torch.float64, device=ctx.device) if elev else None
    fl = torch.full((n + SPARE,), 0xA5, dtype=torch.uint8, device=ctx.device)
    ctx.call('amt_world_to_pixel', C.byref(p), zen_ref(z), frame, ptr(a), ptr(b), n, C.c_void_p(xy.data_ptr() + 8 * xy_offset),
             ptr(el), ptr(fl))
    xy_h, fl_h = to_host(xy), to_host(fl)
    assert (xy_h[:xy_offset] == POISON).all() and (xy_h[xy_offset + 2 * n:] == POISON).all() and (fl_h[n:] == 0xA5).all()
    el_h = None
    if elev:
        el_h = to_host(el)
        assert (el_h[n:] == POISON).all()
        el_h = el_h[:n]
    return xy_h[xy_offset:xy_offset + 2 * n].reshape(n, 2), el_h, fl_h[:n]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- accuracy, flags, elevation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frame', ['geodetic', 'sm', 'j2000'])
def test_against_mpmath(ctx, frame):
    code = dict(IC.FRAMES)[frame]
    worst_px, worst_deg, where, n_points = 0.0, 0.0, None, 0
    for name in IC.names():
        r = IC.points(name)[frame]
        if not len(r['c0']):
            continue
        xy, elev, flags = run_points(ctx, IC.by_name(name), code, r['c0'], r['c1'])
        ref = r['ref']
        assert ref['margin'].min() >= IC.AMBIGUOUS                      # (nothing is left out of the flag comparison)
        assert np.array_equal(flags, ref['flags']), (name, flags, ref['flags'])
        no_pixel = (ref['flags'] & O.NO_PIXEL) != 0
        assert np.array_equal(np.isnan(xy[:, 0]), no_pixel) and np.array_equal(np.isnan(xy[:, 1]), no_pixel), name
        d = np.where(no_pixel, 0.0, np.hypot(xy[:, 0] - ref['x'], xy[:, 1] - ref['y']))
        if d.max() > worst_px:
            worst_px, where = float(d.max()), name
        if code == O.J2000:
            assert np.isnan(elev).all(), name
        else:
            assert not np.isnan(elev).any(), name
            worst_deg = max(worst_deg, float(np.abs(elev - ref['elev']).max()))
        n_points += len(d)
    print('%s: %d points; largest distance from mpmath %.3e px (%s), elevation %.3e deg' % (frame, n_points, worst_px, where, worst_deg))
    assert worst_px <= ACCURACY_PX and worst_deg <= ACCURACY_DEG


# ---- round trip through the forward kernel ---------------------------------------------------------------------------------------
def test_round_trip_through_the_forward_kernel(ctx):
    from auromat_amd._native import to_host
    from auromat_amd.frame import FrameData
    from auromat_amd.mapping.astrometry import georef_into
    bound = IC.bowring_residual() + ACCURACY_PX
    worst = dict(geodetic=(0.0, None), sm=(0.0, None))
    n_points = 0
    for cam in IC.cameras():
        if not O.is_plain_tan(cam):
            continue                                    # (the frame kernel's camera model is the plain TAN one)
        p, _ = IC.native(cam)
        p.fast_center = 0                               # exact centres: every pixel's own ray
        fd = georef_into(FrameData(ctx, cam['height'], cam['width']), p, geo=True, mag=True)
        lat, lon, mlat, mlt = (to_host(t).ravel() for t in (fd.lat_c, fd.lon_c, fd.mlat_c, fd.mlt_c))
        rows, cols = np.mgrid[0:cam['height'], 0:cam['width']]
        hit = ~np.isnan(lat)
        assert np.array_equal(hit, ~np.isnan(mlat))
        if not hit.any():
            continue
        px, py = cols.ravel()[hit].astype(np.float64), rows.ravel()[hit].astype(np.float64)
        for key, code, c0, c1 in (('geodetic', O.GEODETIC, lat[hit], lon[hit]), ('sm', O.SM, mlat[hit], (mlt[hit] - 12.0) / (24.0 / 360.0))):
            xy, _, flags = run_points(ctx, cam, code, c0, c1, elev=False, native=(p, None))
            assert not (flags & O.NO_PIXEL).any(), cam['name']
            d = float(np.hypot(xy[:, 0] - px, xy[:, 1] - py).max())
            if d > worst[key][0]:
                worst[key] = (d, cam['name'])
        n_points += int(hit.sum())
    print('round trip through amt_georef_frame, %d pixels: geodetic %.3e px (%s), MLat / MLT %.3e px (%s); bound %.3e px'
          % ((n_points,) + worst['geodetic'] + worst['sm'] + (bound,)))
    assert worst['geodetic'][0] <= bound and worst['sm'][0] <= bound


# ---- edge inputs -----------------------------------------------------------------------------------------------------------------
def test_block_tails_and_empty_call(ctx):
    cam = IC.by_name('cd-rotation-37')
    base = IC.points('cd-rotation-37')['geodetic']
    rng = np.random.RandomState(11)
    c0 = base['c0'][rng.randint(0, len(base['c0']), 1025)] + rng.uniform(-0.2, 0.2, 1025)
    c1 = base['c1'][rng.randint(0, len(base['c1']), 1025)] + rng.uniform(-0.2, 0.2, 1025)
    full = run_points(ctx, cam, O.GEODETIC, c0, c1)
    assert (full[2] == 0).any() and (full[2] & O.OUTSIDE).any()
    for n in (0, 1, 257):
        part = run_points(ctx, cam, O.GEODETIC, c0[:n], c1[:n])
        for got, want in zip(part, full):
            assert same_bits(got, want[:n]), n
    shifted = run_points(ctx, cam, O.GEODETIC, c0, c1, xy_offset=1)         # an xy pointer that is no multiple of 16 bytes
    assert all(same_bits(a, b) for a, b in zip(shifted, full))
    without = run_points(ctx, cam, O.GEODETIC, c0, c1, elev=False)
    assert same_bits(without[0], full[0]) and same_bits(without[2], full[2])


@pytest.mark.parametrize('frame', [O.GEODETIC, O.SM, O.J2000])
def test_invalid_inputs_poles_and_the_meridian_of_180(ctx, frame):
    cam = IC.by_name('pole' if frame != O.J2000 else 'cd-rotation-37')
    nan, inf = np.nan, np.inf
    c0 = np.array([nan, 10.0, inf, 10.0, -inf, 90.0000001, -91.0, 90.0, -90.0, 30.0, 30.0, 30.0, 30.0])
    c1 = np.array([5.0, nan, 5.0, inf, 5.0, 5.0, 5.0, 77.0, 77.0, 180.0, -180.0, 540.0, -540.0])
    xy, elev, flags = run_points(ctx, cam, frame, c0, c1)
    assert (flags[:7] == O.INVALID).all() and np.isnan(xy[:7]).all() and np.isnan(elev[:7]).all()
    assert not (flags[7:] & O.INVALID).any()
    want = [O.inverse(O.F64, cam, frame, a, b) for a, b in zip(c0, c1)]
    assert [w['flags'] for w in want] == list(flags)
    for i in (7, 8):
        if not flags[i] & O.NO_PIXEL:
            assert np.hypot(xy[i, 0] - want[i]['x'], xy[i, 1] - want[i]['y']) <= 1e-6
    assert same_bits(xy[9], xy[10]) and same_bits(xy[9], xy[11]) and same_bits(xy[9], xy[12])
    assert same_bits(elev[9:10], elev[10:11]) and same_bits(elev[9:10], elev[11:12]) and len(set(flags[9:])) == 1


def _axis_camera(projection):
    """a camera whose boresight is the J2000 x axis exactly: (dec, ra) = (0, 0) gives rho = 0 without rounding"""
    cam = dict(IC.by_name('cd-crpix-fraction'), projection=projection, sip_a=None, sip_b=None,
               rot=np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), cam=np.array([0.0, 7000.0, 0.0]))
    return cam


@pytest.mark.parametrize('projection', range(5))
def test_boresight_and_domain_limits(ctx, projection):
    cam = _axis_camera(projection)
    native = (IC.K.native_params(cam), O.zen_struct(cam))
    dec = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 60.0])
    ra = np.array([0.0, 180.0, 90.0, 90.0001, 179.99, 89.9999, 0.0])
    xy, elev, flags = run_points(ctx, cam, O.J2000, dec, ra, native=native)
    # rho = 0: CRPIX - 1 exactly
    assert xy[0, 0] == cam['crpix'][0] - 1 and xy[0, 1] == cam['crpix'][1] - 1 and not flags[0] & O.NO_PIXEL
    name = O.ZENITHAL[projection]
    unprojectable = (flags & O.UNPROJECTABLE) != 0
    assert np.array_equal(np.isnan(xy[:, 0]), unprojectable)
    # the antipode (n = -1 exactly) is outside every domain but ARC's, where rho is 1.2e-16, not 0
    assert unprojectable[1] == (name != 'ARC')
    # 90 deg off the axis: cos(pi / 2) = 6e-17 >= 0, so SIN's closed limit holds the point; TAN's open one too (n > 0)
    assert not unprojectable[2] and not unprojectable[5] and not unprojectable[6]
    assert unprojectable[3] == (name in ('TAN', 'SIN'))              # behind a TAN camera, beyond SIN's limit
    assert unprojectable[4] == (name in ('TAN', 'SIN'))              # STG, ARC, ZEA reach to just before the antipode
    want = [O.inverse(O.F64, cam, O.J2000, a, b)['flags'] for a, b in zip(dec, ra)]
    assert want == list(flags)


def test_sip_fold_over(ctx):
    cam = IC.by_name('sip-fold')
    plain = dict(cam, sip_a=None, sip_b=None)
    rows = np.array([5.0, 20.0, 40.0])
    d = [O.forward_mp(plain, cam['crpix'][0] - 1 - 14.0, y) for y in rows]       # U = -14: no preimage under u + 0.02 u^2
    near = [O.forward_mp(cam, 30.0, y) for y in rows]
    dec, ra = np.array([f['dec'] for f in d + near]), np.array([f['ra'] for f in d + near])
    xy, _, flags = run_points(ctx, cam, O.J2000, dec, ra)
    assert ((flags[:3] & O.NOT_CONVERGED) != 0).all() and np.isnan(xy[:3]).all() and not (flags[:3] & O.OUTSIDE).any()
    assert not (flags[3:] & O.NO_PIXEL).any()
    assert np.abs(xy[3:, 0] - 30.0).max() <= ACCURACY_PX and np.abs(xy[3:, 1] - rows).max() <= ACCURACY_PX


def test_bad_arguments_are_refused_and_write_nothing(ctx):
    import torch
    from auromat_amd._native import ptr, to_host
    lib = ctx._lib
    cam = IC.by_name('sip-2')
    p, z = IC.native(cam)
    n = 8
    a, b = ctx.to_device(np.zeros(n)), ctx.to_device(np.zeros(n))
    xy = torch.full((n, 2), POISON, dtype=torch.float64, device=ctx.device)
    xy32 = torch.full((n, 2), POISON, dtype=torch.float32, device=ctx.device)
    fl = torch.full((n,), 0xA5, dtype=torch.uint8, device=ctx.device)

    def points(params=p, zen=z, frame=O.GEODETIC, c0=a, c1=b, count=n, out=xy, flags=fl):
        return lib.amt_world_to_pixel(ctx.handle, None if params is None else C.byref(params), zen_ref(zen), frame, ptr(c0), ptr(c1),
                                      count, ptr(out), None, ptr(flags))

    def grid(params=p, zen=z, frame=O.GEODETIC, la=a, ny=2, lo=b, nx=4, out32=xy32, out=xy, flags=fl):
        return lib.amt_grid_to_pixel(ctx.handle, None if params is None else C.byref(params), zen_ref(zen), frame, ptr(la), ny,
                                     ptr(lo), nx, ptr(out32), ptr(out), None, ptr(flags))
    bad_proj, bad_sip, empty = O.zen_struct(cam), O.zen_struct(cam), IC.K.native_params(cam)
    bad_proj.projection, bad_sip.sip_order_b, empty.width = 5, 10, 0
    singular = IC.K.native_params(cam)
    singular.cd[:] = [1.0, 2.0, 2.0, 4.0]
    for rc in (points(params=None), points(c0=None), points(c1=None), points(out=None), points(flags=None), points(count=-1),
               points(frame=3), points(frame=-1), points(zen=bad_proj), points(zen=bad_sip), points(params=empty),
               points(params=singular, zen=None), lib.amt_world_to_pixel(None, C.byref(p), None, 0, ptr(a), ptr(b), n, ptr(xy), None, ptr(fl)),
               grid(params=None), grid(la=None), grid(lo=None), grid(flags=None), grid(out32=None, out=None), grid(ny=0), grid(nx=0),
               grid(nx=-3), grid(frame=7), grid(zen=bad_proj), grid(zen=bad_sip)):
        assert rc == EINVAL
    assert points(count=0, c0=None, c1=None, out=None, flags=None) == 0          # n = 0: fine, nothing to write
    ctx.synchronize()
    assert (to_host(xy) == POISON).all() and (to_host(xy32) == np.float32(POISON)).all() and (to_host(fl) == 0xA5).all()
    assert points() == 0 and grid() == 0
    ctx.synchronize()
    assert not (to_host(fl) == 0xA5).any()


# ---- the grid form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cd-sheared', 'dateline', 'sip-3'])
@pytest.mark.parametrize('shape', [(1, 1), (37, 53), (3, 1100)])
def test_grid_form_equals_point_form(ctx, name, shape):
    import torch
    from auromat_amd._native import ptr, to_host
    cam = IC.by_name(name)
    p, z = IC.native(cam)
    ny, nx = shape
    for key, code in IC.FRAMES:
        r = IC.points(name)[key]
        sel = (r['ref']['flags'] & (O.NO_PIXEL | O.OUTSIDE | (0 if key == 'j2000' else O.HIDDEN))) == 0    # (stars: also behind the Earth)
        lo0, hi0 = r['c0'][sel].min(), r['c0'][sel].max()
        c1s = np.where(r['c1'][sel] < 0, r['c1'][sel] + 360.0, r['c1'][sel]) if name == 'dateline' and key != 'j2000' else r['c1'][sel]
        lo1, hi1 = c1s.min(), c1s.max()
        # beyond the frame on every side, the latitude axis descending as in a resampling grid
        lat = np.linspace(hi0 + 0.3 * (hi0 - lo0), lo0 - 0.3 * (hi0 - lo0), ny) if ny > 1 else np.array([0.5 * (lo0 + hi0)])
        lon = np.linspace(lo1 - 0.3 * (hi1 - lo1), hi1 + 0.3 * (hi1 - lo1), nx) if nx > 1 else np.array([0.5 * (lo1 + hi1)])
        n = ny * nx
        xy32 = torch.full((n * 2 + SPARE,), POISON, dtype=torch.float32, device=ctx.device)
        xy = torch.full((n * 2 + SPARE,), POISON, dtype=torch.float64, device=ctx.device)
        el = torch.full((n + SPARE,), POISON, dtype=torch.float64, device=ctx.device)
        fl = torch.full((n + SPARE,), 0xA5, dtype=torch.uint8, device=ctx.device)
        lat_d, lon_d = ctx.to_device(lat), ctx.to_device(lon)
        ctx.call('amt_grid_to_pixel', C.byref(p), zen_ref(z), code, ptr(lat_d), ny, ptr(lon_d), nx, ptr(xy32), ptr(xy), ptr(el), ptr(fl))
        g32, g, ge, gf = to_host(xy32), to_host(xy), to_host(el), to_host(fl)
        assert (g32[2 * n:] == np.float32(POISON)).all() and (g[2 * n:] == POISON).all() and (ge[n:] == POISON).all() and (gf[n:] == 0xA5).all()
        la2, lo2 = np.meshgrid(lat, lon, indexing='ij')
        pxy, pe, pf = run_points(ctx, cam, code, la2.ravel(), lo2.ravel())
        assert same_bits(g[:2 * n].reshape(n, 2), pxy) and same_bits(ge[:n], pe) and same_bits(gf[:n], pf), (name, key)
        assert same_bits(g32[:2 * n], g[:2 * n].astype(np.float32)), (name, key)
        if n > 1:
            assert ((gf[:n] & (O.NO_PIXEL | O.OUTSIDE)) == 0).any() and (gf[:n] & O.OUTSIDE).any(), (name, key)
        # each output array is optional but one of the two coordinate arrays
        only32 = torch.full((n * 2,), POISON, dtype=torch.float32, device=ctx.device)
        fl2 = torch.empty((n,), dtype=torch.uint8, device=ctx.device)
        ctx.call('amt_grid_to_pixel', C.byref(p), zen_ref(z), code, ptr(lat_d), ny, ptr(lon_d), nx, ptr(only32), None, None, ptr(fl2))
        assert same_bits(to_host(only32), g32[:2 * n]) and same_bits(to_host(fl2), gf[:n])


# ---- the Python functions ------------------------------------------------------------------------------------------------------------
_header = IC.header_of


@pytest.mark.parametrize('name', ['cd-rotation-37', 'zen-SIN', 'zen-ARC', 'zen-STG', 'zen-ZEA', 'sip-2', 'sip-3'])
def test_world2pix_inverts_pix2world(ctx, name):
    from auromat_amd._native import to_host
    from auromat_amd.coordinates import wcs
    cam = IC.by_name(name)
    h = _header(cam)
    w, hh = cam['width'], cam['height']
    dirs = to_host(wcs.zenithal_directions_device(h, w, hh, corner=False))
    ra = np.degrees(np.arctan2(dirs[..., 1], dirs[..., 0])) % 360.0
    dec = np.degrees(np.arctan2(dirs[..., 2], np.hypot(dirs[..., 0], dirs[..., 1])))
    rows, cols = np.mgrid[0:hh, 0:w]
    for origin in (0, 1):
        x, y = wcs.world2pix(h, ra, dec, origin)
        assert x.shape == ra.shape and y.shape == ra.shape
        d = float(np.hypot(x - origin - cols, y - origin - rows).max())
        # (ra, dec) in float64 degrees carry half a unit in the last place of 360 deg, 2.8e-14 deg, at 0.05 - 0.4 deg / px
        assert d <= ACCURACY_PX + 2e-12, (name, d)
    print('%s: world2pix(pix2world) largest distance %.3e px' % (name, d))
    if name == 'cd-rotation-37':
        tx, ty = wcs.tan_world2pix(h, ra, dec, 0)
        assert same_bits(tx, x - 1) or np.abs(tx - (x - 1)).max() <= 1e-12
        pra, pdec = wcs.tan_pix2world(h, cols.astype(np.float64), rows.astype(np.float64), 0)
        bx, by = wcs.tan_world2pix(h, pra, pdec, 0)
        assert np.hypot(bx - cols, by - rows).max() <= ACCURACY_PX + 2e-12
        far = wcs.tan_world2pix(h, np.array([(h['CRVAL1'] + 180.0) % 360.0]), np.array([-h['CRVAL2']]), 0)
        assert np.isnan(far[0]).all() and np.isnan(far[1]).all()


def test_mapping_methods_equal_the_c_call(ctx):
    import numpy.ma as ma
    from auromat_amd.coordinates import wcs
    from auromat_amd.mapping.astrometry import DirectionArrayMapping
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    for name in ('limb-below+0.5', 'sip-3'):
        cam = IC.by_name(name)
        h = _header(cam)
        img = np.zeros((cam['height'], cam['width'], 3), dtype=np.uint8)
        if O.is_plain_tan(cam):
            m = ArraySpacecraftMapping(h, cam['altitude'], img, cam['cam'], cam['time'], name)
        else:
            dirs = wcs.zenithal_directions_device(h, cam['width'], cam['height'], corner=True)
            m = DirectionArrayMapping(dirs, cam['altitude'], img, cam['cam'], cam['time'], name, cameraHeader=h)
        native = m._inverse_model()
        pts = IC.points(name)
        for key, code, call in (('geodetic', O.GEODETIC, lambda a, b: m.latLonToPixel(a, b, returnFlags=True)),
                                ('sm', O.SM, lambda a, b: m.mLatMltToPixel(a, b / 15.0 + 12.0, returnFlags=True)),
                                ('j2000', O.J2000, lambda a, b: m.raDecToPixel(b, a, returnFlags=True))):
            c0, c1 = pts[key]['c0'].reshape(2, -1), pts[key]['c1'].reshape(2, -1)       # (a shape of its own)
            x, y, flags = call(c0, c1)
            if key == 'sm':
                c1 = (c1 / 15.0 + 12.0 - 12.0) / (24.0 / 360.0)                         # the SM longitude the method passes on
            xy, _, fl = run_points(ctx, cam, code, c0.ravel(), c1.ravel(), native=native)
            assert x.shape == c0.shape and flags.shape == c0.shape and np.array_equal(flags.ravel(), fl)
            mask = (fl & (O.NO_PIXEL | O.HIDDEN)) != 0
            assert np.array_equal(ma.getmaskarray(x).ravel(), mask) and np.array_equal(ma.getmaskarray(y).ravel(), mask)
            assert same_bits(x.data.ravel(), xy[:, 0]) and same_bits(y.data.ravel(), xy[:, 1])
            assert mask.any() and not mask.all() and (key != 'j2000' or (fl & O.OUTSIDE).any())
            # the model of the mapping is the case's: the numbers are those of the mpmath reference as well
            ok = ~mask
            assert np.hypot(x.data.ravel()[ok] - pts[key]['ref']['x'][ok], y.data.ravel()[ok] - pts[key]['ref']['y'][ok]).max() <= 1e-6
        # another altitude: the ground below is seen elsewhere
        x0, y0 = m.latLonToPixel(pts['geodetic']['c0'], pts['geodetic']['c1'], altitude=0.0)
        x1, y1 = m.latLonToPixel(pts['geodetic']['c0'], pts['geodetic']['c1'])
        assert np.hypot(x0.filled(0) - x1.filled(0), y0.filled(0) - y1.filled(0)).max() > 1.0
