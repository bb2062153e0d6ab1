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
