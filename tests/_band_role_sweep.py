"""
TEST INFRASTRUCTURE — cameras at the margins of the band roles (amt_prm::band_roles with inner_bands / elevation_bands(tight) /
sky_bands of auromat_amd/csrc/amt_georef.hip) for tests/test_band_role_sweep_cpu.py and tests/test_gpu_band_role_sweep.py.

The cases are built with tests/_camera_cases.py (camera, move, finish, exact, native_params), so tests/_camera_oracle.py is
their reference as it stands.  A band is 16 pixel rows, a strip 63 columns; frames are 62 to 200 wide and 1 to 120 high.

Aiming.  `aimed()` moves CRPIX so that a line of the image — elevation = threshold, or the limb — crosses a probe line at a given
coordinate.  The line is found on the elevation of a pixel's own ray at its own hit (the exact centre of _camera_oracle, in
float64 here: it only chooses the numbers of a case; the CPU test measures the result on the reference), by bisection along the
probe.  Coordinates are corner coordinates: corner row i is at i, pixel row r covers [r, r + 1].  For rolls 0, 180 and 45 deg the
probe is the frame's centre column (pixel column width // 2) and the target lies delta rows from an interior band boundary; for
roll 90 deg, where the line runs along the columns and crosses every band, the probe is the centre row and the target lies
delta columns from the frame's last corner column — the rule's margins in x.

Families
  aimed-threshold   thresholds 4.99, 5, 10, 30, 60 deg x delta -3.5 ... +3.5 x rolls 0, 180, 45, 90; 70 x 120 from 400 km at 0.05 deg / px
  aimed-limb        the limb at the same offsets and rolls (tested at thresholds none, 0 and -0.0)
  orbits            camera heights shell + 5, shell + 50, 250, 400, 1000, 5000, 42000 km over shells at 0, 110 and 1000 km (a camera
                    below its shell is left out), the 10 deg line 1.5 rows inside a boundary; a shell with the flattening 1 / 10
                    (b = 0.9 a) seen from over the equator and from over a pole, the 10 deg line on either side of a boundary
  scales            0.01, 0.05, 0.2 and 0.45 deg / px; a pair just inside and just outside the gate of elevation_bands at 30 deg and
                    a pair around the gate of sky_bands; 1 deg / px for the inner rule, which has no gate
  model             CD mirrored, anisotropic and sheared, and the reference pixel 1000 px outside the frame (the cd family's)
  sizes             heights 1, 15, 16, 17, 48, 50 and widths 62, 63, 64, 126, 127
  nothing           a nadir frame, a limb frame, a camera inside the shell and one that looks away from the Earth at 0.6 deg / px, for
                    the thresholds that decide nothing or everything
Every case exists with fast centres and, as 'exact-' + name, with exact centres.

Conditions on every case (asserted on the reference by the CPU test): no ray with |relative discriminant| below
_camera_cases.r_min(), and no pixel whose elevation lies within 1e-9 deg of a threshold it is tested at; CRPIX is nudged by
multiples of 2^-10 px until both hold in float64 with a factor 2 to spare.
"""
import numpy as np

import _camera_cases as K
import _camera_oracle as Q
import _coord_oracle as C
import _rowfield_cases as RK
import _rowfield_oracle as R

ROWS = 16
DELTAS = (-3.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5)
AIMED_THRESHOLDS = (4.99, 5.0, 10.0, 30.0, 60.0)
ROLLS = (0.0, 180.0, 45.0, 90.0)
NONE = float('-inf')
# every case is tested at these (GPU: all but 60); a family adds its own through c['thresholds']
THRESHOLDS = (NONE, 0.0, 4.99, 5.0, 10.0, 30.0, 60.0)
GPU_THRESHOLDS = (0.0, 4.99, 5.0, 10.0, 30.0, NONE)
LIMB_THRESHOLDS = (NONE, 0.0, -0.0)
NOTHING_THRESHOLDS = (float('nan'), float('inf'), 90.0, 89.99, 89.0, -5.0)
THRESHOLD_GAP = 1e-9                        # degrees between any pixel's elevation and a threshold it is tested at
ISS = K.ISS
FAMILIES = ('aimed-threshold', 'aimed-limb', 'orbits', 'scales', 'model', 'sizes', 'nothing')


# ---- the frame in any arithmetic ----------------------------------------------------------------------------------------------------
def frame_in(xp, c):
    """_camera_oracle.reference(substitute=False) of a case in the arithmetic xp (float64: the restatement that stands in for
    oracle/ref_numpy.py on a shell that is not WGS84 + altitude) -> the nine arrays and 'rel'"""
    P = Q.params_of(c)
    h, w = c['height'], c['width']
    i, j = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        k = Q.corner(xp, Q.direction(xp, P, j - 0.5, i - 0.5), P)
        out = {n: np.array(k[n]) for n in Q.CORNER_ARRAYS}
        out['rel'] = np.array(k['rel'])
        if c['fast_center']:
            def part(sl):
                return dict(p=tuple(v[sl] for v in k['p']), d=tuple(v[sl] for v in k['d']))
            s00, s01 = (slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None))
            s11, s10 = (slice(1, None), slice(1, None)), (slice(1, None), slice(None, -1))
            m = R.centre(xp, part(s00), part(s01), part(s11), part(s10), P)
        else:
            m = Q.exact_centre(xp, Q.direction(xp, P, j[:-1, :-1], i[:-1, :-1]), P)
    out.update({n: np.array(v) for n, v in m.items()})
    return out


def is_wgs84_shell(c):
    return c['a'] == K.A0 + c['altitude'] and c['b'] == K.B0 + c['altitude']


def float64_oracle(c):
    """oracle/ref_numpy.py::georef_frame where it can state the case (a shell of WGS84 + altitude), else the float64 restatement"""
    if is_wgs84_shell(c):
        return Q.float64_oracle(c)
    f = frame_in(C._F64, c)
    return {k: np.asarray(f[k], dtype=np.float64) for k in Q.ARRAYS}


def ray_elevation(xp, c, x, y):
    """elevation (deg) of the ray through pixel coordinates (x, y) at its own hit, NaN where it misses"""
    P = Q.params_of(c)
    with np.errstate(invalid='ignore', divide='ignore'):
        d = Q.direction(xp, P, xp.num(x), xp.num(y))
        p, _ = R.shell_hit(xp, d, P)
        return Q.ray_elevation(xp, d, p)


def above(xp, c, x, y, threshold):
    """does the ray through (x, y) hit at an elevation >= threshold?  threshold None: does it hit?"""
    e = np.asarray(ray_elevation(xp, c, x, y))
    with np.errstate(invalid='ignore'):
        return ~np.isnan(e) if threshold is None else (e >= threshold)


# ---- aiming -------------------------------------------------------------------------------------------------------------------------
def probe_of(c):
    """('column' | 'row', the probe's fixed pixel coordinate)"""
    return ('row', c['height'] // 2) if c['claims']['probe'] == 'row' else ('column', c['width'] // 2)


def line_position(xp, c, threshold, reach=1600.0):
    """corner coordinate along the probe at which the line (threshold None: the limb) crosses it, by bisection between the two
    neighbouring probe points, one pixel apart, at which `above` changes — the change nearest to the frame's middle"""
    kind, fixed = probe_of(c)
    mid = (c['height'] if kind == 'column' else c['width']) / 2.0
    t = np.arange(-reach, reach + 1.0) + np.floor(mid)

    def at(s):
        s = np.asarray(s, dtype=np.float64)
        f = np.full(s.shape, float(fixed))
        return above(xp, c, f, s, threshold) if kind == 'column' else above(xp, c, s, f, threshold)
    flags = at(t)
    change = np.flatnonzero(flags[1:] != flags[:-1])
    assert change.size, (c['name'], 'no line on the probe')
    n = change[np.argmin(np.abs(t[change] + 0.5 - mid))]
    lo, hi, up = float(t[n]), float(t[n + 1]), bool(flags[n + 1])
    for _ in range(60):
        m = 0.5 * (lo + hi)
        if bool(at(np.array([m]))[0]) == up:
            hi = m
        else:
            lo = m
    return 0.5 * (lo + hi) + 0.5, up                  # pixel coordinate -> corner coordinate; `up`: above towards growing coordinates


def aimed(name, family, threshold, delta, boundary, w=70, h=120, roll=0.0, probe='column', **kw):
    """A camera whose line (threshold None: the limb) crosses the probe at corner coordinate boundary + delta"""
    c = K.camera(name, family, w, h, roll=roll, line=threshold, delta=delta, boundary=boundary, probe=probe,
                 target=boundary + delta, **kw)
    return c


def place(c):
    """moves the aimed line of a case to its target (after a, b and cam of the case are final)"""
    if 'target' not in c['claims']:
        return c
    pos, up = line_position(C._F64, c, c['claims']['line'])
    d = c['claims']['target'] - pos
    K.move(c, dx=d, dy=0.0) if c['claims']['probe'] == 'row' else K.move(c, dx=0.0, dy=d)
    c['claims']['above_grows'] = bool(up)
    return c


def line_nadir_angle(height, altitude, threshold, lat=ISS['lat'], lon=ISS['lon']):
    """nadir angle (deg) of the rays at the elevation `threshold` (None: the limb) on a sphere through the shell below the camera"""
    r_cam = float(np.linalg.norm(RK.ecef(lat, lon, height)))
    r_shell = float(np.linalg.norm(RK.ecef(lat, lon, altitude)))
    k = r_shell / r_cam * (1.0 if threshold is None else np.cos(np.deg2rad(threshold)))
    return float(np.degrees(np.arcsin(min(1.0, k))))


def tested_thresholds(c):
    return tuple(THRESHOLDS) + tuple(c.get('thresholds', ()))


def conditions_hold(c):
    """in float64, with a factor 2 to spare: no corner or centre ray grazes, no fast or exact centre's elevation lies at a threshold"""
    rel, _ = K.all_rays(dict(c, fast_center=0))
    with np.errstate(invalid='ignore'):
        if (np.abs(rel) < 2.0 * K.r_min()).any():
            return False
    finite = [t for t in tested_thresholds(c) if np.isfinite(t)]
    for mode in (1, 0):
        elev = np.asarray(frame_in(C._F64, dict(c, fast_center=mode))['elev'], dtype=np.float64)
        elev = elev[~np.isnan(elev)]
        if elev.size and min(float(np.abs(elev - t).min()) for t in finite) < 2.0 * THRESHOLD_GAP:
            return False
    return True


def finish(c):
    """place(), then _camera_cases.finish with the threshold condition added to its grazing condition, for both centre modes"""
    place(c)
    for k in range(400):
        if conditions_hold(c):
            break
        K.move(c, K.NUDGE * (1 + k % 3), K.NUDGE * (1 + k % 5))
    else:
        raise AssertionError('%s: no nudge satisfies the conditions' % c['name'])
    c = K.finish(c)
    assert c['nudges'] == 0
    c['nudges'] = k
    return c


# ---- the families -------------------------------------------------------------------------------------------------------------------
def _tag(v):
    return 'none' if v is None else ('%g' % v)


def _aimed_threshold():
    out = []
    for thr in AIMED_THRESHOLDS:
        na = line_nadir_angle(ISS['height'], 110.0, thr)
        for roll in ROLLS:
            for d in DELTAS:
                row = roll == 90.0
                out.append(aimed('thr%s-roll%d%+g' % (_tag(thr), roll, d), 'aimed-threshold', thr, d, 70 if row else 64, roll=roll,
                                 probe='row' if row else 'column', nadir_angle=na, azimuth=-20.0, **ISS))
    return out


def _aimed_limb():
    out = []
    na = line_nadir_angle(ISS['height'], 110.0, None)
    for roll in ROLLS:
        for d in DELTAS:
            row = roll == 90.0
            c = aimed('limb-roll%d%+g' % (roll, d), 'aimed-limb', None, d, 70 if row else 64, roll=roll,
                      probe='row' if row else 'column', nadir_angle=na, azimuth=-20.0, **ISS)
            c['thresholds'] = LIMB_THRESHOLDS
            out.append(c)
    return out


def gate_scale(height, altitude, threshold, lat=ISS['lat'], lon=ISS['lon']):
    """deg / px at which the gate asin(k) > 8 (rows + 2) pixel angle of elevation_bands (threshold None: sky_bands) turns, for a
    camera with square pixels: k = (a + altitude) / |camera| * cos(threshold)"""
    r_cam = float(np.linalg.norm(RK.ecef(lat, lon, height)))
    k = (K.A0 + altitude) / r_cam * (1.0 if threshold is None else np.cos(np.deg2rad(threshold)))
    return float(np.degrees(np.arcsin(k))) / K.GATE


def _orbits():
    out = []
    for altitude in (0.0, 110.0, 1000.0):
        for tag, height in (('+5', altitude + 5.0), ('+50', altitude + 50.0), ('250', 250.0), ('400', 400.0), ('1000', 1000.0),
                            ('5000', 5000.0), ('42000', 42000.0)):
            if height < altitude + 5.0:
                continue                                        # (a camera inside its shell: the family `nothing` has one)
            if tag in ('250', '400', '1000') and height in (altitude + 5.0, altitude + 50.0):
                continue
            where = dict(ISS, height=height)
            scale = min(0.05, 0.5 * gate_scale(height, altitude, 10.0))
            out.append(aimed('orbit-%s-shell%d' % (tag, altitude), 'orbits', 10.0, -1.5, 32, h=80, scale=scale, altitude=altitude,
                             nadir_angle=line_nadir_angle(height, altitude, 10.0), azimuth=35.0, **where))
    # a shell of flattening 1 / 10 at 110 km: r_min and r_max differ by 10 %, the two cones of the rules by degrees
    for tag, lat in (('equator', 0.0), ('pole', 90.0)):
        for d in (-1.5, 2.5):
            c = aimed('flat-%s%+g' % (tag, d), 'orbits', 10.0, d, 32, h=80, altitude=110.0, nadir_angle=60.0, azimuth=35.0,
                      lat=lat, lon=14.0, height=400.0)
            c['a'], c['b'] = K.A0 + 110.0, 0.9 * (K.A0 + 110.0)
            up = RK.unit(c['cam'])
            c['cam'] = up * ((c['a'] if lat == 0.0 else c['b']) + 400.0)       # 400 km above the shell's equator / pole
            c['claims']['flattened'] = True
            out.append(c)
    return out


def _scales():
    out = []
    for s in (0.01, 0.05, 0.2, 0.45):
        for d in (-1.5, 2.5):
            out.append(aimed('scale-%g%+g' % (s, d), 'scales', 10.0, d, 32, h=80, scale=s, nadir_angle=line_nadir_angle(400.0, 110.0, 10.0),
                             azimuth=35.0, **ISS))
    # the gates: the 30 deg line 2.5 rows before a boundary with low bands above it (the limb is 44 rows further up), and the limb
    # with sky bands above it
    for which, thr in (('elevation', 30.0), ('sky', None)):
        g = gate_scale(400.0, 110.0, thr)
        for side, f in (('inside', 0.99), ('outside', 1.01)):
            c = aimed('gate-%s-%s' % (which, side), 'scales', thr, -2.5, 48, w=62, h=80, scale=f * g,
                      nadir_angle=line_nadir_angle(400.0, 110.0, thr), azimuth=35.0, gate=which, gate_passes=side == 'inside', **ISS)
            out.append(c)
    # 1 deg / px, where only the inner rule still speaks: the nadir, and the 30 and 60 deg lines inside the frame
    out.append(K.camera('scale-1-nadir', 'scales', 70, 80, nadir_angle=0.0, scale=1.0, crpix=(35.7, 40.4), ungated=True, **ISS))
    for thr in (30.0, 60.0):
        for d in (-1.5, 2.5):
            out.append(aimed('scale-1-thr%g%+g' % (thr, d), 'scales', thr, d, 32, h=80, scale=1.0, ungated=True,
                             nadir_angle=line_nadir_angle(400.0, 110.0, thr), azimuth=35.0, **ISS))
    return out


def _model():
    s, out = 0.05, []
    na = line_nadir_angle(400.0, 110.0, 10.0)
    for tag, cd, claims in (('flipped', [[-s, 0.0], [0.0, s]], dict(negative_det=True)), ('anisotropic', [[s, 0.0], [0.0, 1.6 * s]], {}),
                            ('sheared', [[s, 0.4 * s], [0.0, s]], {})):
        for d in (-1.5, 2.5):
            out.append(aimed('model-%s%+g' % (tag, d), 'model', 10.0, d, 32, h=80, cd=cd, roll=11.0, nadir_angle=na, azimuth=20.0,
                             **dict(ISS, **claims)))
    # the frame 1000 px (41 deg in the tangent plane) from the reference pixel, on the nadir's side of the boresight
    for d in (-1.5, 2.5):
        out.append(aimed('model-crpix-outside%+g' % d, 'model', 10.0, d, 32, h=80, crpix=(35.5, -1000.0), nadir_angle=na + 41.0,
                         azimuth=20.0, **ISS))
    return out


def _sizes():
    out = []
    na = line_nadir_angle(400.0, 110.0, 10.0)
    pairs = ((1, 62), (15, 63), (16, 64), (17, 126), (48, 127), (50, 62), (1, 127), (16, 126), (17, 63), (50, 64), (48, 126), (15, 127),
             (17, 62), (50, 127))
    for h, w in pairs:
        boundary = 16 * ((h - 1) // 16) if h > 16 else h     # an interior boundary, else the frame's last corner row
        for d in (-2.5, 2.5):
            out.append(aimed('size-%dx%d%+g' % (w, h, d), 'sizes', 10.0, d, boundary, w=w, h=h, nadir_angle=na, azimuth=-50.0, **ISS))
    return out


def _nothing():
    out = [K.camera('nothing-nadir', 'nothing', 70, 50, nadir_angle=0.0, crpix=(35.7, 25.4), **ISS),
           aimed('nothing-limb', 'nothing', None, 0.5, 32, w=70, h=50, nadir_angle=line_nadir_angle(400.0, 110.0, None), azimuth=-20.0, **ISS),
           K.camera('nothing-inside', 'nothing', 70, 40, lat=65.0, lon=25.0, height=50.0, nadir_angle=95.0, azimuth=10.0, scale=0.3,
                    inside=True),
           # away from the Earth, too coarse for sky_bands to name its bands: the mirror image of the cone, which only the test
           # `uo < 0` of inner_bands tells from the cone
           K.camera('nothing-zenith', 'nothing', 70, 50, nadir_angle=180.0, scale=0.6, pure='sky', **ISS)]
    for c in out:
        c['thresholds'] = NOTHING_THRESHOLDS
    return out


_CASES = []


def cases():
    if not _CASES:
        made = []
        for make in (_aimed_threshold, _aimed_limb, _orbits, _scales, _model, _sizes, _nothing):
            made.extend(make())
        done = []
        for c in made:
            c = finish(c)
            done.append(c)
            twin = dict(K.exact(c), family=c['family'])          # the same camera with exact centres (finish() looked at both)
            done.append(twin)
        _CASES.extend(done)
        assert {c['family'] for c in _CASES} == set(FAMILIES) and len({c['name'] for c in _CASES}) == len(_CASES)
    return _CASES


def names(fam=None, fast=None):
    return [c['name'] for c in cases() if (fam is None or c['family'] == fam) and (fast is None or bool(c['fast_center']) == fast)]


def by_name(name):
    return next(c for c in cases() if c['name'] == name)


def family(fam):
    return [c for c in cases() if c['family'] == fam]


# ---- references, once per process -------------------------------------------------------------------------------------------------
_REF, _F64 = {}, {}


def reference(name):
    if name not in _REF:
        r = Q.reference(by_name(name))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def f64(name):
    if name not in _F64:
        _F64[name] = float64_oracle(by_name(name))
    return _F64[name]


_BOUNDS = {}


def bounds(name):
    """per array 8 max(E_ref, eps scale) with its floor (_rowfield_oracle.bound), E_ref the distance of the float64 oracle from
    the reference on this very case"""
    if name not in _BOUNDS:
        _BOUNDS[name] = {k: Q.bound(k, float(Q.distance(k, f64(name), reference(name)).max())) for k in Q.ARRAYS}
    return _BOUNDS[name]


def forget(names_):
    """drops the references of these cameras (both centre modes); their bounds stay"""
    for n in names_:
        for key in (n, 'exact-' + n):
            _REF.pop(key, None)
            _F64.pop(key, None)


# ---- the roles ----------------------------------------------------------------------------------------------------------------------
def band_roles(c, min_elev, fast=None):
    """amt_georef_band_roles on the numbers of a case, as _band_role_cases.band_roles gives it"""
    import ctypes
    from auromat_amd import _native
    p = K.native_params(c, fast)
    rows = ctypes.c_int32(0)
    r = (ctypes.c_int32 * 8)()
    assert _native.lib().amt_georef_band_roles(ctypes.byref(p), float(min_elev), ctypes.byref(rows), r) == 0
    assert rows.value == ROWS
    v = list(r)
    return dict(n=v[0], strips=v[1], sky=(v[2], v[3]), low=(v[4], v[5]), inner=(v[6], v[7]))


def allowed(c, arrays, min_elev):
    """What a frame's arrays allow per band: (may be inner, may be low, has a corner that hits, smallest elevation - threshold of
    the band's pixels (NaN: a miss among them), largest elevation of the band's pixels (-inf: none hits))"""
    h = c['height']
    n = (h + ROWS - 1) // ROWS
    miss_corner = np.isnan(np.asarray(arrays['lat'], dtype=np.float64))
    elev = np.asarray(arrays['elev'], dtype=np.float64)
    miss_centre = np.isnan(np.asarray(arrays['lat_c'], dtype=np.float64)) | np.isnan(elev)
    with np.errstate(invalid='ignore'):
        passes = ~miss_centre & (elev >= min_elev)
    inner, low, hit = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    least, most = np.full(n, np.nan), np.full(n, -np.inf)
    for k in range(n):
        r0, r1 = k * ROWS, min((k + 1) * ROWS, h)
        inner[k] = not miss_corner[r0:r1 + 1].any() and not miss_centre[r0:r1].any() and passes[r0:r1].all()
        low[k] = not passes[r0:r1].any()
        hit[k] = (~miss_corner[r0:r1 + 1]).any()
        if not miss_centre[r0:r1].any() and not miss_corner[r0:r1 + 1].any():
            least[k] = float(elev[r0:r1].min()) - max(min_elev, 0.0) if min_elev == min_elev else np.nan
        if not miss_centre[r0:r1].all():
            most[k] = float(np.nanmax(elev[r0:r1]))
    return inner, low, hit, least, most
