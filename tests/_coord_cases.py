"""
TEST INFRASTRUCTURE — small constructed inputs for the 19 operator kernels of auromat_amd/csrc/amt_coords.hip.

A case is a dict: name, family, op (the entry point without amt_) and args, the float64 numbers the entry point receives (the
arguments of tests/_coord_oracle.py's functions) plus what the float64 oracle needs to be called on the same numbers (a WCS
header, an all-sky calibration).  Every case has at most a few thousand points but the three of the stride family.
tests/test_coord_cases_cpu.py checks what the families claim.

Families:
  lengths     every entry point at n = 0, 1, 63, 64, 65, 255, 256, 257 points (a wave, a block, and one beside them).  The frame
              generators take no empty frame: amt_directions_tan / _zenithal run at n x 1 pixels for n >= 1, and the all-sky
              generator, whose point count is a square, at sizes 1, 7, 8, 15, 16 with both point families (1 to 289 points)
  stride      4096 * 256 + 257 points, one more block than grid_for() launches: amt_rotate_vectors, amt_ecef_to_geodetic,
              amt_intersects_ellipsoid
  geodetic    latitudes +-90, +-(90 - 1e-k) for k = 3, 6, 9, 12, 0 and -0, longitudes +-180, +-(180 - 1e-9), 0, heights 0, 110,
              1000 km, WGS84 and an ellipsoid with b / a = 0.9; ECEF points with y = +-0 at x < 0, on the axis, 1e-3 to 1e-9 km
              beside it.  DOMAIN: every point lies outside the evolute of its ellipsoid, p > e^2 a cos^3 u — only inside it do
              the kernel's atan2(num, den) and the reference's arctan(num / den) differ; points on the axis give NaN in both.
  rotate_pole rotations by +-90 deg about x (cos(pi / 2) = 6.1e-17, as the pole plans build them), about an arbitrary axis, and
              the identity; points at the poles, at the points a rotation takes to the poles, on the date line; 0, 110, 1000 km
  rays        ellipsoid and sphere, directed and undirected; origin outside, inside and at the centre (|t1| == |t2|); rays
              towards the body, away from it, 1e-6 rad inside and outside the tangent cone; lengths 1e-3 and 1e3 (ellipsoid); a
              NaN direction.  The sphere kernel and its reference evaluate the same formula (intersection.py:26-48: t = -d.o -+
              sqrt((d.o)^2 - o.o + r^2), o + t d), which nothing in either normalises: the sphere gets unit vectors, and one case
              with directions 1 + 2^-10 long, compared on that formula.  No case is closer to a decision than a relative
              discriminant of 1e-9, a directed t of 1e-9 |origin|, or (undirected) |d.o| = 1e-9 of the root.
  magnetic    SM vectors with y = +-0 at x < 0 (MLT 24 and 0) and on the SM axis, the matrices of two dates; amt_sm_to_latlon at
              SM latitudes beyond 30 deg (it works on the unit sphere: lower ones fall inside the evolute, see sm_lats)
  wcs         TAN grids and points (corner / origin 0 and 1; 1x1, 1x65, 65x3); the five zenithal projections at 1x1, 7x5, 65x3
              with SIP of orders (3, 2), (0, 4), (9, 9), a start offset, the reference pixel itself, SIN and ZEA within 0.9 of
              their rim
  allsky      sizes 1, 2, 33, a pixel on the zenith, rotations that put azimuths on both sides of 0 / 360 and more than one turn
              away from it, both point families
  themis      a station at 45 and at 78 deg, the new height below, at and above the reference height, reference points at the
              station's zenith and 8 deg away

E_ref (the distance of the float64 oracle from the reference, the largest of a family) and the bounds are computed here, from
the references alone.
"""
from datetime import datetime

import numpy as np

import _coord_oracle as Q
from oracle import ref_numpy as O

A0, B0 = O.WGS84_A, O.WGS84_B
FLAT_A, FLAT_B = 6378.137, 6378.137 * 0.9
ET = (O.date2es(datetime(2012, 3, 4, 17, 19, 0)), O.date2es(datetime(2001, 12, 21, 3, 0, 30)))
M_GEO = [np.ascontiguousarray(O.mat_j2000_to_geo(et)) for et in ET]
M_SM = [np.ascontiguousarray(O.mat_j2000_to_sm(et)) for et in ET]
M_GEO_SM = [np.ascontiguousarray(O.mat_geo_to_sm(et)) for et in ET]
EYE = np.eye(3)
K_DEG2RAD, K_RAD2DEG = 0.017453292519943295, 57.29577951308232          # kDeg2Rad, kRad2Deg of amt_common.h

LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)
STRIDE_N = 4096 * 256 + 257
FAMILIES = ('lengths', 'stride', 'geodetic', 'rotate_pole', 'rays', 'magnetic', 'wcs', 'allsky', 'themis')


def ecef(lat, lon, height, a=A0, b=B0):
    x, y, z = O.geodetic_to_ecef(np.deg2rad(lat), np.deg2rad(lon), height, a, b)
    return np.stack(np.broadcast_arrays(x, y, z), axis=-1)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def case(name, family, op, **args):
    for v in args.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(name=name, family=family, op=op, args=args)


# ---- generic inputs of n points (lengths, stride) --------------------------------------------------------------------------------
ORIGIN_OUT = ecef(45.0, -70.0, 400.0)
ORIGIN_IN = ecef(65.0, 25.0, 0.0)


def _spread(n, seed):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0, 1, n)


def aimed_dirs(n, seed):
    """unit directions from ORIGIN_OUT at points of the 110 km shell within 8 deg of the point below it; every fifth turned away"""
    u, v, _ = _spread(n, seed)
    d = unit(ecef(45.0 + 8 * u, -70.0 + 8 * v, 110.0) - ORIGIN_OUT)
    d[4::5] = -d[4::5]
    return np.ascontiguousarray(d)


def points_xyz(n, seed):
    u, v, w = _spread(n, seed)
    return np.ascontiguousarray(ecef(89 * u, 180 * v, 1000 * w))


def sm_lats(u):
    """SM latitudes of 30 to 89 deg, both signs: smToLatLon applies Bowring's formula to points of the UNIT sphere
    (transform.py:472-480), which lie inside the evolute of the WGS84 ellipsoid unless their geographic latitude is beyond some
    4 deg — the dipole axis is 10 deg from the rotation axis, so these stay outside it"""
    return np.where(u < 0, -1.0, 1.0) * (30.0 + 59.0 * np.abs(u))


def tan_header(width, height, crpix=None):
    return {'CTYPE1': 'RA---TAN', 'CTYPE2': 'DEC--TAN', 'LATPOLE': 0.0, 'LONPOLE': 180.0, 'CRVAL1': 203.7, 'CRVAL2': -31.2,
            'CRPIX1': (width / 2 + 0.5) if crpix is None else crpix[0], 'CRPIX2': (height / 2 + 0.5) if crpix is None else crpix[1],
            'CD1_1': -0.021, 'CD1_2': 0.0043, 'CD2_1': 0.0039, 'CD2_2': 0.0207, 'IMAGEW': width, 'IMAGEH': height}


def tan_args(header, corner=None):
    """the amt_frame_params numbers of a TAN header (coordinates.wcs.fill_wcs_params) and the grid indices"""
    w, h = header['IMAGEW'], header['IMAGEH']
    out = dict(header=header, width=w, height=h, cd=[header['CD1_1'], header['CD1_2'], header['CD2_1'], header['CD2_2']],
               crpix=[header['CRPIX1'], header['CRPIX2']], rot=np.ascontiguousarray(O.wcs_rotation(header)))
    if corner is not None:
        r, c = np.mgrid[0:h + corner, 0:w + corner]
        out.update(corner=corner, row=r.ravel().astype(np.float64), col=c.ravel().astype(np.float64))
    return out


def zenithal_header(proj, width, height, orders=None, scale=0.5, crpix=None, seed=0):
    """a zenithal header, with SIP polynomials of the orders (A, B) whose terms stay below a few pixels over the frame"""
    sip = orders is not None
    h = {'CTYPE1': 'RA---%s%s' % (proj, '-SIP' if sip else ''), 'CTYPE2': 'DEC--%s%s' % (proj, '-SIP' if sip else ''),
         'LONPOLE': 180.0, 'CRVAL1': 41.3, 'CRVAL2': 62.9, 'CRPIX1': (width / 2 + 0.75) if crpix is None else crpix[0],
         'CRPIX2': (height / 2 + 0.25) if crpix is None else crpix[1],
         'CD1_1': -scale, 'CD1_2': 0.07 * scale, 'CD2_1': 0.06 * scale, 'CD2_2': 0.98 * scale}
    if sip:
        rng = np.random.RandomState(100 + seed)
        for prefix, order in zip('AB', orders):
            h[prefix + '_ORDER'] = order
            if order:
                for p in range(order + 1):
                    for q in range(order + 1 - p):
                        if p + q >= 2:
                            h['%s_%d_%d' % (prefix, p, q)] = float(rng.uniform(-1, 1) * 0.5 / 40.0 ** (p + q))
    return h


def zenithal_args(header, width, height, startX=0, startY=0, corner=1):
    from auromat_amd.coordinates.wcs import projection_of, zenithal_params
    w = zenithal_params(header, width, height, startX, startY, bool(corner))
    r, c = np.mgrid[0:height + corner, 0:width + corner]
    return dict(header=header, w=w, startX=startX, startY=startY, sip=projection_of(header)[1],
                row=r.ravel().astype(np.float64), col=c.ravel().astype(np.float64))


def allsky_args(size, cal, corner, altitude=110.0, center_offset=0.5):
    """the amt_allsky_params numbers of a calibration (mapping.miracle.allsky_params) and the grid indices"""
    scale = size / 512
    n = size + (1 if corner else 0)
    r, c = np.mgrid[0:n, 0:n]
    mat_lat = O.rotation_matrix3(np.deg2rad(90 - cal['lat']), [0, 1, 0])
    mat_lon = O.rotation_matrix3(np.deg2rad(-cal['lon']), [0, 0, -1])
    station = np.array(O.geodetic_to_ecef_zero(np.deg2rad(cal['lat']), np.deg2rad(cal['lon'])), dtype=np.float64)
    return dict(cal=cal, size=size, corner=corner, center_offset=center_offset, xc=cal['xc'] * scale, yc=cal['yc'] * scale,
                k=cal['k'] * scale, rotation=float(cal['rotation']), to_geo=np.ascontiguousarray(np.dot(mat_lon, mat_lat)),
                station=station, a=A0 + altitude, b=B0 + altitude, a0=A0, b0=B0,
                row=r.ravel().astype(np.float64), col=c.ravel().astype(np.float64))


CAL = dict(lat=69.02, lon=20.87, xc=251.3, yc=259.8, k=166.0, rotation=0.3)
ALLSKY_LENGTH_SIZES = (1, 7, 8, 15, 16)


def generic(op, n, seed=0):
    """args of `op` on n well-conditioned points"""
    u, v, w = _spread(n, seed + 1)
    if op in ('intersect_ellipsoid', 'intersects_ellipsoid'):
        return dict(a=A0 + 110.0, b=B0 + 110.0, origin=ORIGIN_OUT, dirs=aimed_dirs(n, seed), directed=1)
    if op == 'intersect_sphere':
        return dict(radius=6481.0, origin=ORIGIN_OUT, dirs=aimed_dirs(n, seed), directed=1)
    if op in ('ecef_to_geodetic', 'cartesian_to_spherical'):
        p = points_xyz(n, seed)
        out = dict(x=p[:, 0].copy(), y=p[:, 1].copy(), z=p[:, 2].copy())
        out.update(dict(a=A0, b=B0) if op == 'ecef_to_geodetic' else dict(with_r=True))
        return out
    if op == 'geodetic_to_ecef':
        return dict(lat=np.deg2rad(89 * u), lon=np.deg2rad(180 * v), h=110.0, a=A0, b=B0)
    if op == 'rotate_to_latlon':
        return dict(m=M_GEO[0], xyz=points_xyz(n, seed), a=A0, b=B0)
    if op == 'rotate_to_mlat_mlt':
        return dict(m=M_SM[0], xyz=points_xyz(n, seed))
    if op == 'rotate_vectors':
        return dict(m=M_GEO[0], xyz=points_xyz(n, seed))
    if op == 'latlon_to_mlat_mlt':
        return dict(m=M_GEO_SM[0], lat=89 * u, lon=180 * v, h=110.0, a=A0, b=B0)
    if op == 'sm_to_latlon':
        return dict(m=np.ascontiguousarray(M_GEO_SM[0].T), smlat=sm_lats(u), smlon=180 * v, a=A0, b=B0)
    if op == 'spherical_to_cartesian':
        return dict(r=6400.0 + 1000 * w, lat=np.deg2rad(89 * u), lon=np.deg2rad(180 * v))
    if op == 'rotate_pole':
        return dict(rot=O.rotation_matrix3(np.deg2rad(90), [1, 0, 0]), lat=(89 * u) * K_DEG2RAD, lon=(180 * v) * K_DEG2RAD,
                    altitude=110.0, a=A0, b=B0)
    if op == 'rotate_pole_deg':
        return dict(rot=O.rotation_matrix3(np.deg2rad(90), [1, 0, 0]), lat=89 * u, lon=180 * v, altitude=110.0, a=A0, b=B0)
    if op == 'directions_tan':
        return tan_args(tan_header(n, 1), corner=0)
    if op == 'directions_tan_points':
        return dict(tan_args(tan_header(64, 48)), px=32 + 30 * u, py=24 + 22 * v, origin=0)
    if op == 'directions_zenithal':
        return zenithal_args(zenithal_header('ARC', n, 1, orders=(2, 3)), n, 1, corner=0)
    if op == 'reproject_altitude':
        return dict(station_lat=62.4, station_lon=-114.5, lat=62.4 + 4 * u, lon=-114.5 + 8 * v, height_ref=110.0,
                    height_new=150.0, a=A0, b=B0)
    raise KeyError(op)


GRID_OPS = ('directions_tan', 'directions_zenithal', 'georef_allsky')


def _lengths():
    out = []
    for op in Q.OPS:
        if op == 'georef_allsky':
            for size in ALLSKY_LENGTH_SIZES:
                for corner in (0, 1):
                    out.append(case('lengths-georef_allsky-%d-%d' % (size, corner), 'lengths', op,
                                    **allsky_args(size, CAL, corner)))
            continue
        for n in LENGTHS:
            if n == 0 and op in GRID_OPS:
                continue                                      # "empty frame": refused, see the GPU test
            out.append(case('lengths-%s-%d' % (op, n), 'lengths', op, **generic(op, n, seed=n)))
    # the variants without a radius (NULL r)
    out.append(case('lengths-cartesian_to_spherical-65-no-r', 'lengths', 'cartesian_to_spherical',
                    **dict(generic('cartesian_to_spherical', 65, 3), with_r=False)))
    out.append(case('lengths-spherical_to_cartesian-65-no-r', 'lengths', 'spherical_to_cartesian',
                    **dict(generic('spherical_to_cartesian', 65, 3), r=None)))
    return out


def _stride():
    return [case('stride-%s' % op, 'stride', op, **generic(op, STRIDE_N, seed=11))
            for op in ('rotate_vectors', 'ecef_to_geodetic', 'intersects_ellipsoid')]


# ---- geodetic -------------------------------------------------------------------------------------------------------------------
GEODETIC_LATS = [90.0, -90.0, 0.0, -0.0] + [s * (90.0 - 10.0 ** -k) for k in (3, 6, 9, 12) for s in (1, -1)] + [37.0, -61.5]
GEODETIC_LONS = [180.0, -180.0, 180.0 - 1e-9, -(180.0 - 1e-9), 0.0, 73.0]
HEIGHTS = (0.0, 110.0, 1000.0)
ELLIPSOIDS = (('wgs84', A0, B0), ('flat', FLAT_A, FLAT_B))
AXIS_DISTANCES = (1e-3, 1e-5, 1e-7, 1e-9)


def _geodetic():
    out = []
    lat, lon = (g.ravel() for g in np.meshgrid(np.array(GEODETIC_LATS), np.array(GEODETIC_LONS), indexing='ij'))
    for tag, a, b in ELLIPSOIDS:
        for h in HEIGHTS:
            out.append(case('geodetic-to-ecef-%s-%g' % (tag, h), 'geodetic', 'geodetic_to_ecef', lat=np.deg2rad(lat),
                            lon=np.deg2rad(lon), h=h, a=a, b=b))
            x, y, z = O.geodetic_to_ecef(np.deg2rad(lat), np.deg2rad(lon), h, a, b)
            out.append(case('geodetic-from-ecef-%s-%g' % (tag, h), 'geodetic', 'ecef_to_geodetic', x=x, y=y, z=z, a=a, b=b))
        # y = +-0 at x < 0; on the axis (NaN latitude); 1e-3 .. 1e-9 km beside it, above both poles
        zs = (b + 110.0, -(b + 110.0))
        pts = [(-(a + 110.0), 0.0, 0.0), (-(a + 110.0), -0.0, 0.0), (-4000.0, 0.0, 5200.0), (-4000.0, -0.0, -5200.0)]
        pts += [(x0, y0, z0) for z0 in zs for x0, y0 in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0))]
        pts += [(s * e * 0.6, e * 0.8, z0) for z0 in zs for e in AXIS_DISTANCES for s in (1, -1)]
        p = np.array(pts, dtype=np.float64)
        out.append(dict(case('geodetic-from-ecef-%s-special' % tag, 'geodetic', 'ecef_to_geodetic', x=p[:, 0].copy(),
                             y=p[:, 1].copy(), z=p[:, 2].copy(), a=a, b=b), on_axis=np.arange(4, 12), half_turn=np.arange(0, 4)))
    return out


# ---- rotate_pole ----------------------------------------------------------------------------------------------------------------
ROTATIONS = (('plus90x', O.rotation_matrix3(np.deg2rad(90), [1, 0, 0])), ('minus90x', O.rotation_matrix3(np.deg2rad(-90), [1, 0, 0])),
             ('arbitrary', O.rotation_matrix3(0.651, [0.3, -0.5, 0.8])), ('identity', EYE))


def _rotate_pole():
    out = []
    for tag, rot in ROTATIONS:
        rot = np.ascontiguousarray(rot)
        for alt in HEIGHTS:
            lat = [90.0, -90.0, 90.0, -90.0, 0.0, 0.0, 12.0, -47.0, 33.0, -5.0, 89.999999, -89.999999, 60.0, 60.0]
            lon = [0.0, 0.0, 135.0, -60.0, 180.0, -180.0, 180.0 - 1e-9, -(180.0 - 1e-9), 77.0, -120.0, 10.0, -10.0, 90.0, -90.0]
            # the points that the rotation takes to the poles, and their neighbours 1e-6 deg away
            for z in (1.0, -1.0):
                v = rot.T @ np.array([0.0, 0.0, z])               # the direction that becomes the axis
                lo = float(np.rad2deg(np.arctan2(v[1], v[0]))) if abs(v[2]) < 1 else 0.0
                la = want = float(np.rad2deg(np.arcsin(np.clip(v[2], -1, 1))))
                for _ in range(8):                                # the geodetic latitude whose point at `alt` lies on that line
                    g = ecef(la, lo, alt)
                    la += want - float(np.rad2deg(np.arctan2(g[2], np.hypot(g[0], g[1]))))
                la = float(np.clip(la, -90.0, 90.0))
                lat += [la, la - z * 1e-6 if abs(la) == 90 else la + 1e-6]
                lon += [lo, lo + 1e-6]
            lat, lon = np.array(lat), np.array(lon)
            out.append(case('rotate_pole-%s-%g-deg' % (tag, alt), 'rotate_pole', 'rotate_pole_deg', rot=rot, lat=lat, lon=lon,
                            altitude=alt, a=A0, b=B0))
            out.append(case('rotate_pole-%s-%g-rad' % (tag, alt), 'rotate_pole', 'rotate_pole', rot=rot, lat=lat * K_DEG2RAD,
                            lon=lon * K_DEG2RAD, altitude=alt, a=A0, b=B0))
    return out


# ---- rays -----------------------------------------------------------------------------------------------------------------------
TANGENT_OFFSET = 1e-6


def _cone(origin, rad, offsets):
    """unit directions (in real space) whose angle from the tangent cone of the body rad, seen from origin, is `offsets` in the
    space where the body is the unit sphere (negative: inside the cone)"""
    os_ = origin / rad
    dist = np.sqrt(os_ @ os_)
    axis = -os_ / dist
    f = unit(np.cross(axis, [0.0, 0.0, 1.0]))
    g = np.cross(axis, f)
    theta = np.arcsin(1.0 / dist) + np.asarray(offsets)
    phi = 0.4 + 0.7 * np.arange(len(theta))
    ds = np.cos(theta)[:, None] * axis + np.sin(theta)[:, None] * (np.cos(phi)[:, None] * f + np.sin(phi)[:, None] * g)
    return unit(ds * rad)


def ray_dirs(origin, rad, scale_lengths):
    """(directions, tags): towards the body, away from it, beside the tangent cone, scaled, NaN"""
    centre = not np.any(origin)
    rng = np.random.RandomState(5)
    if centre:
        towards = unit(rng.normal(size=(12, 3)))
    else:
        towards = unit(unit(-origin) + 0.05 * rng.normal(size=(12, 3)))
    d, tags = [towards, -towards], ['towards'] * 12 + ['away'] * 12
    if not centre and (origin / rad) @ (origin / rad) > 1:
        off = np.array([-TANGENT_OFFSET, TANGENT_OFFSET] * 4)
        cone = _cone(origin, rad, off)
        d += [cone, -cone]
        tags += ['inside-cone', 'outside-cone'] * 4 + ['away-inside-cone', 'away-outside-cone'] * 4
    if scale_lengths:
        d += [towards[:4] * 1e-3, towards[4:8] * 1e3, -towards[:2] * 1e3]
        tags += ['short'] * 4 + ['long'] * 4 + ['long-away'] * 2
    d.append(np.array([[np.nan, 0.3, 0.5], [0.1, np.nan, np.nan]]))
    tags += ['nan', 'nan']
    return np.ascontiguousarray(np.concatenate(d)), tags


RAY_ORIGINS = (('outside', ORIGIN_OUT), ('inside', ORIGIN_IN), ('centre', np.zeros(3)))
SPHERE_RADIUS = 6481.0


def _rays():
    out = []
    a, b = A0 + 110.0, B0 + 110.0
    for tag, origin in RAY_ORIGINS:
        for directed in (1, 0):
            kind = 'directed' if directed else 'undirected'
            d, tags = ray_dirs(origin, np.array([a, a, b]), True)
            for op in ('intersect_ellipsoid', 'intersects_ellipsoid'):
                out.append(dict(case('rays-%s-%s-%s' % (op, tag, kind), 'rays', op, a=a, b=b, origin=origin, dirs=d,
                                     directed=directed), tags=tags))
            d, tags = ray_dirs(origin, np.full(3, SPHERE_RADIUS), False)
            out.append(dict(case('rays-intersect_sphere-%s-%s' % (tag, kind), 'rays', 'intersect_sphere', radius=SPHERE_RADIUS,
                                 origin=origin, dirs=d, directed=directed), tags=tags))
    d, tags = ray_dirs(ORIGIN_OUT, np.full(3, SPHERE_RADIUS), False)
    keep = [i for i, t in enumerate(tags) if t in ('towards', 'away')]
    for directed in (1, 0):
        out.append(dict(case('rays-intersect_sphere-nonunit-%d' % directed, 'rays', 'intersect_sphere', radius=SPHERE_RADIUS,
                             origin=ORIGIN_OUT, dirs=np.ascontiguousarray(d[keep] * (1.0 + 2.0 ** -10)), directed=directed),
                        tags=[tags[i] for i in keep]))
    return out


# ---- magnetic -------------------------------------------------------------------------------------------------------------------
def _magnetic():
    out = []
    # the identity takes the vectors to SM as they are: y = +0 (MLT 24) and, with x < 0 and z < 0 so that no product of the
    # rotation is a +0, y = -0 (MLT 0); the SM axis
    sm = np.array([[-5000.0, 0.0, 3000.0], [-5000.0, -0.0, -3000.0], [-6500.0, 0.0, 0.0], [-6500.0, -0.0, -0.0],
                   [0.0, 0.0, 6500.0], [0.0, 0.0, -6500.0], [3000.0, 1e-9, 100.0], [-3000.0, 1e-9, 100.0], [-3000.0, -1e-9, 100.0]])
    out.append(dict(case('magnetic-mlt-zero', 'magnetic', 'rotate_to_mlat_mlt', m=EYE, xyz=sm), midnight=np.arange(0, 4),
                    axis=np.arange(4, 6)))
    for i in (0, 1):
        p = points_xyz(200, 20 + i)
        out.append(case('magnetic-j2000-to-mlat-mlt-%d' % i, 'magnetic', 'rotate_to_mlat_mlt', m=M_SM[i], xyz=p))
        out.append(case('magnetic-geo-to-mlat-mlt-%d' % i, 'magnetic', 'rotate_to_mlat_mlt', m=M_GEO_SM[i], xyz=p))
        out.append(case('magnetic-j2000-to-latlon-%d' % i, 'magnetic', 'rotate_to_latlon', m=M_GEO[i], xyz=p, a=A0, b=B0))
        out.append(case('magnetic-rotate-vectors-%d' % i, 'magnetic', 'rotate_vectors', m=M_SM[i], xyz=p))
        u, v, _ = _spread(200, 30 + i)
        lat = np.concatenate((89 * u, [90.0, -90.0, 0.0]))
        lon = np.concatenate((180 * v, [0.0, 180.0, -180.0]))
        for h in (0.0, 110.0):
            out.append(case('magnetic-latlon-to-mlat-mlt-%d-%g' % (i, h), 'magnetic', 'latlon_to_mlat_mlt', m=M_GEO_SM[i], lat=lat,
                            lon=lon, h=h, a=A0, b=B0))
        smlat = np.concatenate((sm_lats(u), [90.0, -90.0, -35.0, -35.0, 45.0, 45.0]))
        smlon = np.concatenate((180 * v, [0.0, 0.0, 180.0, -180.0, 180.0, -180.0]))
        out.append(case('magnetic-sm-to-latlon-%d' % i, 'magnetic', 'sm_to_latlon', m=np.ascontiguousarray(M_GEO_SM[i].T),
                        smlat=smlat, smlon=smlon, a=A0, b=B0))
    return out


# ---- wcs ------------------------------------------------------------------------------------------------------------------------
WCS_TAN_SIZES = ((1, 1), (1, 65), (65, 3))                  # width x height
WCS_ZEN_SIZES = ((1, 1), (7, 5), (65, 3))
SIP_ORDERS = (None, (3, 2), (0, 4), (9, 9), (2, 0))


def _wcs():
    out = []
    for w, h in WCS_TAN_SIZES:
        for corner in (0, 1):
            # (an integer CRPIX puts the reference pixel itself into the centre grid: r = 0)
            hdr = tan_header(w, h, crpix=((w + 1) // 2, (h + 1) // 2) if not corner else None)
            out.append(case('wcs-tan-grid-%dx%d-corner%d' % (w, h, corner), 'wcs', 'directions_tan', **tan_args(hdr, corner)))
        for origin in (0, 1):
            hdr = tan_header(64, 48, crpix=(31.0, 22.0))
            r, c = np.mgrid[0:h, 0:w].astype(np.float64)
            px = (20.0 + 0.37 * c + 0.11 * r).ravel()
            py = (15.0 + 0.53 * r - 0.07 * c).ravel()
            px[0], py[0] = 31.0 - 1 + origin, 22.0 - 1 + origin          # the reference pixel in this origin's counting
            out.append(case('wcs-tan-points-%dx%d-origin%d' % (w, h, origin), 'wcs', 'directions_tan_points',
                            **dict(tan_args(hdr), px=px, py=py, origin=origin)))
    k = 0
    for proj in Q.ZENITHAL:
        for w, h in WCS_ZEN_SIZES:
            orders = SIP_ORDERS[k % len(SIP_ORDERS)]
            corner = k % 2
            start = ((0, 0), (3, 5), (-2, 7))[k % 3]
            # corner 0: CRPIX on a pixel of the rectangle (r = 0 there, and the SIP offsets vanish)
            crpix = None if corner else (start[0] + (w + 1) // 2, start[1] + (h + 1) // 2)
            hdr = zenithal_header(proj, w, h, orders, scale=0.5 if w < 65 else 0.7, crpix=crpix, seed=k)
            out.append(dict(case('wcs-zenithal-%s-%dx%d' % (proj, w, h), 'wcs', 'directions_zenithal',
                                 **zenithal_args(hdr, w, h, start[0], start[1], corner)), orders=orders, crpix_on_pixel=not corner))
            k += 1
    # every SIP variant on the frame where the polynomials matter most, for TAN and ZEA
    for proj in ('TAN', 'ZEA'):
        for orders in SIP_ORDERS[1:]:
            hdr = zenithal_header(proj, 65, 3, orders, scale=0.7, seed=50 + orders[0])
            out.append(dict(case('wcs-zenithal-%s-sip-%d-%d' % ((proj,) + orders), 'wcs', 'directions_zenithal',
                                 **zenithal_args(hdr, 65, 3, 1, 2, 1)), orders=orders, crpix_on_pixel=False))
    return out


# ---- allsky ---------------------------------------------------------------------------------------------------------------------
# radians; azimuths before the wrap reach from -180 deg - rotation to 180 deg - rotation: beyond +-pi more than one turn is taken off
ALLSKY_ROTATIONS = (0.0, 0.3, -3.0, 3.0, -1e-3, 7.0, -7.0)
ALLSKY_SUBSETS = (('az',), ('el',), ('dirs',), ('lat',), ('lon',), ('az', 'el', 'dirs', 'lat', 'lon'))


def _exact_cal(target, scale):
    """a calibration value (512 px image) whose product with `scale` is exactly `target`"""
    x = np.float64(target) / np.float64(scale)
    for c in (x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)):
        if c * scale == target:
            return float(c)
    raise ValueError((target, scale))


def _allsky():
    out = []
    for size in (1, 2, 33):
        scale = size / 512
        for corner in (0, 1):
            for rotation in ALLSKY_ROTATIONS:
                if size == 33 and rotation not in (0.0, 0.3, -3.0, 7.0):
                    continue
                # the zenith on a point of this family: a corner index, or a pixel centre (index + 0.5)
                zen = (1.0, 1.0) if size <= 2 else (16.0, 17.0)
                if not corner:
                    zen = (0.5, 0.5) if size == 1 else (zen[0] + 0.5 - (size == 2), zen[1] + 0.5 - (size == 2))
                cal = dict(CAL, xc=_exact_cal(zen[0], scale), yc=_exact_cal(zen[1], scale), rotation=rotation)
                out.append(dict(case('allsky-%d-corner%d-rot%g' % (size, corner, rotation), 'allsky', 'georef_allsky',
                                     **allsky_args(size, cal, corner)), zenith=zen))
    for corner in (0, 1):                                   # the zenith between the points
        out.append(dict(case('allsky-33-corner%d-offcentre' % corner, 'allsky', 'georef_allsky',
                             **allsky_args(33, dict(CAL, rotation=-0.2), corner)), zenith=None))
    return out


# ---- themis ---------------------------------------------------------------------------------------------------------------------
def _themis():
    out = []
    for tag, slat, slon in (('mid', 45.3, -100.2), ('high', 78.1, 16.0)):
        az = np.deg2rad(np.arange(0.0, 360.0, 45.0))

        def away(delta, az):                                # the point `delta` degrees along the great circle of azimuth az
            p, d = np.deg2rad(slat), np.deg2rad(delta)
            la = np.arcsin(np.sin(p) * np.cos(d) + np.cos(p) * np.sin(d) * np.cos(az))
            lo = np.deg2rad(slon) + np.arctan2(np.sin(az) * np.sin(d) * np.cos(p), np.cos(d) - np.sin(p) * np.sin(la))
            return np.rad2deg(la), (np.rad2deg(lo) + 180.0) % 360.0 - 180.0
        far, near = away(8.0, az), away(3.0, az + 0.3)
        lat = np.concatenate(([slat], far[0], near[0]))
        lon = np.concatenate(([slon], far[1], near[1]))
        for h_new in (90.0, 110.0, 150.0):
            out.append(case('themis-%s-%g' % (tag, h_new), 'themis', 'reproject_altitude', station_lat=slat, station_lon=slon,
                            lat=lat, lon=lon, height_ref=110.0, height_new=h_new, a=A0, b=B0))
    return out


_CASES = []


def cases():
    if not _CASES:
        for make in (_lengths, _stride, _geodetic, _rotate_pole, _rays, _magnetic, _wcs, _allsky, _themis):
            _CASES.extend(make())
        assert {c['family'] for c in _CASES} == set(FAMILIES)
        assert len({c['name'] for c in _CASES}) == len(_CASES)
    return _CASES


def names(families=FAMILIES):
    return [c['name'] for c in cases() if c['family'] in families]


def by_name(name):
    return next(c for c in cases() if c['name'] == name)


def family(name):
    return [c for c in cases() if c['family'] == name]


# ---- references, computed once per process ----------------------------------------------------------------------------------
_REF, _F64, _RAW = {}, {}, {}


def reference(name):
    """the longdouble arrays of tests/_coord_oracle.reference (read-only), angles in degrees"""
    if name not in _REF:
        c = by_name(name)
        r = Q.reference(c['op'], c['args'])
        for v in r.values():
            v.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def reference_longdouble(name):
    if name not in _RAW:
        c = by_name(name)
        _RAW[name] = Q.reference(c['op'], c['args'], substitute=False)
    return _RAW[name]


def float64_oracle(name):
    """the float64 oracle's outputs, in the entry point's own units"""
    if name not in _F64:
        c = by_name(name)
        _F64[name] = Q.float64_oracle(c['op'], c['args'])
    return _F64[name]


def outputs(c):
    """the outputs a case has (no radius without with_r)"""
    return [(n, k) for n, k in Q.OUT[c['op']] if not (n == 'r' and not c['args'].get('with_r', True))]


def keys(fam):
    """the (op, output) pairs of a family that carry numbers"""
    seen = []
    for c in family(fam):
        for n, k in outputs(c):
            if k != 'hit' and (c['op'], n) not in seen:
                seen.append((c['op'], n))
    return seen


_E, _S = {}, {}


def e_ref(fam, op, out):
    """distance of the float64 oracle from the reference, the largest over the family's cases of that entry point"""
    if (fam, op, out) not in _E:
        worst = 0.0
        for c in family(fam):
            if c['op'] == op and out in dict(outputs(c)):
                d = Q.distance(op, out, Q.comparable(op, float64_oracle(c['name'])), reference(c['name']))
                worst = max(worst, float(d.max()) if d.size else 0.0)
        _E[fam, op, out] = worst
    return _E[fam, op, out]


def scale(fam, op, out):
    if (fam, op, out) not in _S:
        _S[fam, op, out] = Q.scale(op, out, [reference(c['name'])[out] for c in family(fam)
                                             if c['op'] == op and out in dict(outputs(c))])
    return _S[fam, op, out]


def bound(fam, op, out):
    return Q.bound(op, out, e_ref(fam, op, out), scale(fam, op, out))
