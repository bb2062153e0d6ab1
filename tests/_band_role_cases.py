"""
Cameras for the tests of the band roles (amt_prm::band_roles, csrc/amt_params.h; tests/test_band_roles_cpu.py and
tests/test_gpu_band_roles.py): small frames in which the rows of work items ("bands", 16 pixel rows each) still differ — the
limb, the line of the elevation threshold, a last strip narrower than 63 columns and a last band shorter than 16 rows.
"""
import ctypes as C

import numpy as np

SIZES = ((200, 120), (130, 50))
ROWS = 16


def _look(hdr, v):
    return dict(hdr, CRVAL1=float(np.rad2deg(np.arctan2(v[1], v[0])) % 360), CRVAL2=float(np.rad2deg(np.arcsin(v[2]))))


def _rolled(hdr, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    cd = np.array([[hdr['CD1_1'], hdr['CD1_2']], [hdr['CD2_1'], hdr['CD2_2']]]).dot(np.array([[c, -s], [s, c]]))
    return dict(hdr, CD1_1=cd[0, 0], CD1_2=cd[0, 1], CD2_1=cd[1, 0], CD2_2=cd[1, 1])


def _zoomed(hdr, f):
    return dict(hdr, **{k: hdr[k] * f for k in ('CD1_1', 'CD1_2', 'CD2_1', 'CD2_2')})


def _off_nadir(cam, eta_deg):
    """Unit vector at the angle eta from the nadir, in the plane of the nadir and the J2000 pole."""
    up = cam / np.linalg.norm(cam)
    e = np.cross(up, [0.0, 0.0, 1.0])
    e /= np.linalg.norm(e)
    eta = np.deg2rad(eta_deg)
    return -np.cos(eta) * up + np.sin(eta) * e


def cameras(w, h):
    """(name, header, camera, time) — the six views of the issue at one frame size."""
    from auromat_amd.synthetic import frame_header
    hdr, cam, t = frame_header(w, h, 'iss030')
    up = cam / np.linalg.norm(cam)
    # degrees per pixel that make the frame 6 deg tall: the 2.7 deg between the limb and the line of 10 deg of elevation
    # (nadir angles 73.2 and 70.5 deg from 400 km) then span several bands
    zoom = 6.0 / (h * np.hypot(hdr['CD1_1'], hdr['CD1_2']))
    return [
        ('nadir', _look(hdr, -up), cam, t),                                       # every band inner
        ('limb across', hdr, cam, t),                                             # the pointing of the bench frame
        ('limb vertical', _rolled(hdr, 90), cam, t),                              # Earth to one side: every band mixed
        ('threshold line', _zoomed(_look(hdr, _off_nadir(cam, 70.5)), zoom), cam, t),   # the 10 deg line inside the frame
        ('below threshold', _zoomed(_look(hdr, _off_nadir(cam, 72.3)), zoom / 6), cam, t),  # 1 deg tall, between the two lines
        ('sky', _look(hdr, up), cam, t),                                          # nothing but sky
    ]


def cases():
    return [('%s %dx%d' % (c[0], w, h), w, h) + c[1:] for (w, h) in SIZES for c in cameras(w, h)]


def band_roles(hdr, cam, t, min_elev, altitude=110, fast=True):
    """amt_georef_band_roles as a dict: n bands, strips, sky (t, b), low (top_end, bottom_begin), inner (begin, end)."""
    from auromat_amd import _native
    from auromat_amd.mapping.astrometry import frame_params
    p = frame_params(hdr, altitude, cam, t, fast)
    rows = C.c_int32(0)
    r = (C.c_int32 * 8)()
    assert _native.lib().amt_georef_band_roles(C.byref(p), float(min_elev), C.byref(rows), r) == 0
    assert rows.value == ROWS
    v = list(r)
    return dict(n=v[0], strips=v[1], sky=(v[2], v[3]), low=(v[4], v[5]), inner=(v[6], v[7]))


def role_of_bands(roles):
    """Per band: 's' sky, 'i' inner, 'l' low, 'g' generic."""
    n, (t, b), (lt, lb), (i0, i1) = roles['n'], roles['sky'], roles['low'], roles['inner']
    out = []
    for c in range(n):
        if c < t or c >= b:
            out.append('s')
        elif i0 <= c < i1:
            out.append('i')
        elif c < lt or c >= lb:
            out.append('l')
        else:
            out.append('g')
    return ''.join(out)


def oracle_bands(hdr, cam, t, min_elev, altitude=110, fast=True):
    """What the oracle allows per band: (may_be_inner, may_be_low, has_hit) boolean arrays over the bands."""
    from oracle import ref_numpy as O
    from auromat_amd.coordinates import transform as T
    g = O.georef_frame(hdr, altitude, cam, O.mat_j2000_to_geo(T.date2es(t)), None, fast=fast)
    h = hdr['IMAGEH']
    n = (h + ROWS - 1) // ROWS
    miss_corner = np.isnan(g['lat'])
    miss_centre = np.isnan(g['lat_c'])
    with np.errstate(invalid='ignore'):
        passes = ~miss_centre & (g['elev'] >= min_elev)
    inner = np.zeros(n, bool)
    low = np.zeros(n, bool)
    hit = np.zeros(n, bool)
    for c in range(n):
        r0, r1 = c * ROWS, min((c + 1) * ROWS, h)
        inner[c] = not miss_corner[r0:r1 + 1].any() and not miss_centre[r0:r1].any() and passes[r0:r1].all()
        low[c] = not passes[r0:r1].any()
        hit[c] = (~miss_corner[r0:r1 + 1]).any()
    return inner, low, hit


# ---- launches of the frame kernel with and without roles (tests/test_gpu_band_roles.py, tests/test_gpu_band_role_sweep.py) ---------
EVENT_ROOM = 256
GEO = ('lat', 'lon', 'lat_c', 'lon_c', 'elev')
MAG = ('elev', 'mlat', 'mlt', 'mlat_c', 'mlt_c')
NINE = GEO + MAG[1:]
CORNERS = ('lat', 'lon', 'mlat', 'mlt')
OUTPUTS = {0: GEO, 1: NINE, 4: MAG}
EVENT_DTYPE = np.dtype([('w%d' % i, np.uint32) for i in range(8)])      # 32-byte records, compared as sorted words


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


def set_roles(ctx, on):
    ctx.call('amt_georef_set_roles', 1 if on else 0)


def last_roles(ctx):
    g, i, l = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ctx.call('amt_georef_last_roles', C.byref(g), C.byref(i), C.byref(l))
    return g.value, i.value, l.value


_IMAGES = {}


def image(w, h, dtype):
    if (w, h, dtype) not in _IMAGES:
        from auromat_amd.synthetic import frame_image
        a = np.ascontiguousarray(frame_image(w, h, seed=7, dtype=dtype))
        import torch
        _IMAGES[(w, h, dtype)] = torch.from_numpy(a.view(np.int16) if dtype == np.uint16 else a).cuda()
    return _IMAGES[(w, h, dtype)]


def launch_frame(w, h, p, second, bin_dtype, padded, roles, edges=None, min_elev=10.0):
    """amt_georef_frame of one variant on the amt_frame_params block p of a w x h frame -> dict(arrays as uint64 bits with the
    pad columns removed, bbox bits, acc, records, count, variant, items per role)"""
    import torch
    from auromat_amd._native import GeorefOut
    from auromat_amd.util.histogram import make_axis
    ctx = _ctx()
    out, bufs = GeorefOut(), {}
    pitch = int(ctx._lib.amt_padded_pitch(w))
    out.row_layout = 1 if padded else 0
    for k in OUTPUTS[second]:
        rows, cols = (h + 1, w + 1) if k in CORNERS else (h, w)
        bufs[k] = torch.full((rows, pitch if padded else cols), -777.25, dtype=torch.float64, device=ctx.device)
        setattr(out, k, bufs[k].data_ptr())
    bbox = torch.full((8,), -1.0, dtype=torch.float64, device=ctx.device)
    out.bbox, out.bbox_min_elevation = bbox.data_ptr(), float(min_elev)
    out.bin_magnetic = 1 if second == 4 else 0
    acc = ev = counter = keep = None
    if bin_dtype is not None:
        xa, kx = make_axis(ctx, edges[0], uniform=True)
        ya, ky = make_axis(ctx, edges[1], uniform=True)
        assert xa.uniform == 1 and ya.uniform == 1
        keep = (xa, ya, kx, ky)
        acc = torch.zeros(5 * xa.nbin * ya.nbin, dtype=torch.int64, device=ctx.device)
        ev = torch.zeros(32 * EVENT_ROOM, dtype=torch.uint8, device=ctx.device)
        counter = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        out.bin_acc, out.bin_img = acc.data_ptr(), image(w, h, bin_dtype).data_ptr()
        out.bin_img_dtype = 1 if bin_dtype == np.uint8 else 2
        out.bin_xaxis, out.bin_yaxis = C.addressof(xa), C.addressof(ya)
        out.bin_events, out.bin_event_count, out.bin_event_capacity = ev.data_ptr(), counter.data_ptr(), EVENT_ROOM
    set_roles(ctx, roles)
    try:
        ctx.call('amt_georef_frame', C.byref(p), C.byref(out))
        torch.cuda.synchronize()
    finally:
        set_roles(ctx, True)
    res = dict(variant=ctx.last_variant(), roles=last_roles(ctx), bbox=bbox.cpu().numpy().view(np.uint64), arrays={})
    for k, v in bufs.items():
        x = np.arange(w + 1 if k in CORNERS else w)
        if padded:
            x = 64 * (x // 63) + x % 63
        res['arrays'][k] = np.ascontiguousarray(v.cpu().numpy()[:, x]).view(np.uint64)
    if acc is not None:
        res['acc'] = acc.cpu().numpy()
        res['count'] = int(counter.cpu().numpy().view(np.uint32)[0])
        assert res['count'] <= EVENT_ROOM
        res['records'] = np.sort(ev.cpu().numpy()[:32 * res['count']].view(EVENT_DTYPE), order=list(EVENT_DTYPE.names))
    del keep
    return res


def assert_same(tag, on, off):
    assert on['variant'] == off['variant'], tag
    for k in off['arrays']:
        same = on['arrays'][k] == off['arrays'][k]
        assert same.all(), (tag, k, 'first rows that differ', np.unique(np.argwhere(~same)[:, 0])[:8])
    assert np.array_equal(on['bbox'], off['bbox']), (tag, on['bbox'].view(np.float64), off['bbox'].view(np.float64))
    if 'acc' in off:
        assert np.array_equal(on['acc'], off['acc']), (tag, 'accumulators')
        assert on['count'] == off['count'] and np.array_equal(on['records'], off['records']), (tag, 'on-edge records')
