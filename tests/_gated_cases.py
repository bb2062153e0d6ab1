"""
TEST INFRASTRUCTURE — the cases of the gated side stream (tests/_gated_stream.py): one per family of entry points, every device
input as a TRUE array and a DECOY.  Host arrays only; the `call` of a case touches the GPU, nothing else here does
(tests/test_gated_cases_cpu.py checks the decoys without one, tests/test_gpu_gated_stream.py runs the cases).

Shapes are the smallest that still run every kernel of a call: frames of 127 x 33 pixels (three strips of 63 columns and one
column, two bands of 16 rows and one row) and, for a direction array, 64 x 17 (one strip plus one column, one band plus one
row), 64 x 48 frames in the sequence runner, grids of 240 to 300 cells (43 x 27 under amt_georef_frame), 257 points, 49 points under the cubic
interpolation.

Harmlessness, the rule every decoy follows: a decoy is another VALID input.  Coordinates are another finite field in range,
images other pixel values, masks other bytes of 0 / 1, and whatever a kernel uses as an index or a count is in range in the
decoy as in the true array (`index_ranges`, checked on the CPU).  A buffer that one call of a case writes and the next reads
as an index (the nearest-neighbour indices) holds zeros, not poison, before the gate (`out_fill`).  Each case says in
`harmless` why a library that ignored the gate could compute wrong values only.

Oracles of the frame driver and the sequence runner: oracle.ref_numpy's coordinates of the frame (from its camera model or from
the direction array), the box of the corners mask_by_elevation keeps, the library's host rule for the grid of that box
(amt_grid_layout, pinned to the reference's by tests/test_host_cpu.py) and tests/_bin_oracle.py's means on it.  The oracle's
coordinates differ from the device's in the last bits, so these grids are compared with the decoy's on the CPU only, never with
the device's.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

from _gated_stream import Case

W, H = 127, 33
MIN_ELEV = 10.0
ALTITUDE = 110.0
PX_PER_DEG = 2.0
XEDGES = np.linspace(9.0, 29.0, 21)              # 20 x 12 cells of one degree: exactly np.linspace's edges
YEDGES = np.linspace(39.0, 51.0, 13)
NX, NY = len(XEDGES) - 1, len(YEDGES) - 1
FIN_HOLD_MS = 20.0                               # how long the cases of the frame driver hold the finalise stream


def _q(a, unit):
    return np.rint(np.asarray(a) / unit) * unit


# ---- a frame of plain arrays -------------------------------------------------------------------------------------------------

def scene(seed, lat0, lon0):
    """Corner arrays (H + 1, W + 1) of a gently jittered lattice (multiples of 1/64 deg), centres (multiples of 1/64 deg),
    elevations 0 .. 80 deg in steps of 1/64, a uint16 RGB image, an image mask with a fifth of the pixels set."""
    rng = np.random.RandomState(seed)
    i, j = np.mgrid[0:H + 1, 0:W + 1].astype(np.float64)
    lat = _q(lat0 + 0.25 * i + rng.uniform(-0.05, 0.05, i.shape), 1 / 64.0)
    lon = _q(lon0 + 0.125 * j + rng.uniform(-0.03, 0.03, i.shape), 1 / 64.0)
    mean4 = lambda v: 0.25 * (v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:])
    return dict(lat=lat, lon=lon, lat_c=_q(mean4(lat), 1 / 64.0), lon_c=_q(mean4(lon), 1 / 64.0),
                elev=_q(rng.uniform(0.0, 80.0, (H, W)), 1 / 64.0),
                img=rng.randint(0, 65535, (H, W, 3)).astype(np.uint16),
                img_mask=(rng.uniform(size=(H, W)) < 0.2).astype(np.uint8))


TRUE, DECOY = scene(1, 40.0, 10.0), scene(2, 41.25, 11.75)
_kept = {}                                       # device constants and host tables that live as long as the session


def _key(name, ctx):
    """what a case keeps per context — a host thread has a context of its own (Context.current), hence kept objects of its own"""
    return (name, ctx.handle.value)


def pair(*names):
    return OrderedDict((k, (TRUE[k], DECOY[k])) for k in names)


def _axes(ctx):
    from auromat_amd.util.histogram import make_axis
    xa, _ = make_axis(ctx, XEDGES, uniform=True)
    ya, _ = make_axis(ctx, YEDGES, uniform=True)
    assert xa.uniform == 1 and ya.uniform == 1
    return xa, ya


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _median_case(a, with_mask=False):
    import _median_cases as MC
    return MC.Case('gated', None, a['lat_c'].ravel(), a['lon_c'].ravel(), a['elev'].ravel(), a['img'].reshape(-1, 3),
                   a['img_mask'].ravel() if with_mask else None, XEDGES, YEDGES, H, W, min_elevation=MIN_ELEV, uniform=True)


GRID_OUT = OrderedDict([('mean', ((NY, NX, 4), np.float64)), ('img', ((NY, NX, 3), np.uint16)), ('mask', ((NY, NX), np.uint8)),
                        ('count', ((NY, NX), np.float64))])
FIELD = 'every input is a coordinate, elevation or pixel value: cells are found by a bounded search of the axis, values outside ' \
        'the grid are outliers; nothing read from an input is used as an address'


# ---- A. context-stream calls ---------------------------------------------------------------------------------------------------

def _call_masks(env):
    i, o = env.inp, env.out
    env.ctx.call('amt_mask_by_elevation', _ptr(i['elev']), _ptr(i['lat']), H, W, MIN_ELEV, _ptr(o['centre']), _ptr(o['corner']),
                 _ptr(o['n_valid']))
    env.closed('amt_mask_by_elevation')
    env.ctx.call('amt_sanitize_masks', _ptr(o['corner']), _ptr(o['centre']), _ptr(i['img_mask']), H, W, 1)
    env.closed('amt_sanitize_masks')
    env.ctx.call('amt_bbox_corners', _ptr(i['lat']), _ptr(i['lon']), _ptr(o['corner']), _ptr(o['centre']), H, W, _ptr(o['red']))
    env.closed('amt_bbox_corners')


def _oracle_masks(a):
    from oracle import ref_numpy as O
    corner, centre = O.mask_by_elevation(a['elev'], np.isnan(a['lat']), MIN_ELEV)
    corner, centre = O.sanitize_masks(corner, centre, a['img_mask'].astype(bool), True)
    box, _ = O.bbox_of_corners(a['lat'], a['lon'], corner)
    return dict(centre=centre, corner=corner, n_valid=np.array([(a['elev'] >= MIN_ELEV).sum()]), red=np.array(box))


def _call_outline(env):
    i, o = env.inp, env.out
    env.ctx.call('amt_mask_outline_links', _ptr(i['img_mask']), H, W, _ptr(o['links']), H * W * 4, _ptr(o['count']))
    env.closed('amt_mask_outline_links')


def outline_link_keys(mask):
    """The keys 4 * pixel + direction of the contour links of a mask: unmasked pixels whose neighbour in direction 0 up, 1 right,
    2 down, 3 left is masked or outside (the first word of every record, include/auromat_hip.h)."""
    m = np.pad(np.asarray(mask) != 0, 1, constant_values=True)
    inner = ~m[1:-1, 1:-1]
    nb = [m[:-2, 1:-1], m[1:-1, 2:], m[2:, 1:-1], m[1:-1, :-2]]
    flat = np.arange(inner.size).reshape(inner.shape)
    return np.sort(np.concatenate([4 * flat[inner & n] + d for d, n in enumerate(nb)]))


def _oracle_outline(a):
    keys = outline_link_keys(a['img_mask'])
    return dict(links=keys, count=np.array([len(keys)]))


def _sorted_links(b):
    """records (key, next) in the order of their keys; the poisoned tail stays where it is"""
    rec = b.view(np.int64).reshape(-1, 2)
    poison = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]
    used = ~((rec[:, 0] == poison) & (rec[:, 1] == poison))
    out = rec.copy()
    out[:used.sum()] = rec[used][np.argsort(rec[used][:, 0], kind='stable')]
    out[used.sum():] = poison
    return out


N_POLY = 257
_rs = np.random.RandomState(11)
POLY_INDEX = (np.sort(_rs.choice(H * W, N_POLY, replace=False)).astype(np.int64), _rs.permutation(H * W)[:N_POLY].astype(np.int64))


def _call_polygons(env):
    i, o = env.inp, env.out
    env.ctx.call('amt_pixel_polygons', _ptr(i['lat']), _ptr(i['lon']), _ptr(i['img']), 2, 3, H, W, _ptr(i['index']), N_POLY,
                 _ptr(o['verts']), _ptr(o['u8']), _ptr(o['f64']))
    env.closed('amt_pixel_polygons')


def _oracle_polygons(a):
    r, c = np.divmod(a['index'], W)
    corners = [(r, c), (r, c + 1), (r + 1, c + 1), (r + 1, c)]
    verts = np.stack([np.stack([a['lat'][p], a['lon'][p]], axis=1) for p in corners], axis=1)
    u8 = (a['img'].reshape(-1, 3)[a['index']] * (255.0 / 65535.0)).astype(np.uint8)
    return dict(verts=verts, u8=u8, f64=u8 / 255.0)


N_PTS = 257
_rs = np.random.RandomState(12)
_unit = lambda v: v / np.linalg.norm(v, axis=1)[:, None]
XYZ = tuple(_unit(_rs.normal(size=(N_PTS, 3))) * 6480.0 for _ in range(2))


def _m_geo():
    from datetime import datetime
    from oracle import ref_numpy as O
    return O.mat_j2000_to_geo(O.date2es(datetime(2012, 1, 25, 9, 26, 55)))


def _call_rotate(env):
    from auromat_amd._native import host9
    from oracle import ref_numpy as O
    env.ctx.call('amt_rotate_to_latlon', host9(_m_geo()), _ptr(env.inp['xyz']), N_PTS, O.WGS84_A, O.WGS84_B, _ptr(env.out['lat']),
                 _ptr(env.out['lon']))
    env.closed('amt_rotate_to_latlon')


def _oracle_rotate(a):
    from oracle import ref_numpy as O
    lat, lon = O.j2000_to_latlon(a['xyz'], _m_geo())
    return dict(lat=lat, lon=lon)


_rs = np.random.RandomState(13)
LATLON = tuple((_rs.uniform(20.0, 80.0, N_PTS), _rs.uniform(-60.0, 40.0, N_PTS)) for _ in range(2))
PLANE = tuple((_rs.uniform(-3000.0, 3000.0, N_PTS), _rs.uniform(-3000.0, 3000.0, N_PTS)) for _ in range(2))
STERE = (60.0, -10.0)


def _call_project(env):
    from auromat_amd.coordinates.projection import Stereographic
    i, o = env.inp, env.out
    P = Stereographic(*STERE)
    env.ctx.call('amt_project_forward', C.byref(P.params), _ptr(i['lat']), _ptr(i['lon']), N_PTS, _ptr(o['x']), _ptr(o['y']))
    env.closed('amt_project_forward')
    env.ctx.call('amt_project_inverse', C.byref(P.params), _ptr(i['px']), _ptr(i['py']), N_PTS, _ptr(o['ilat']), _ptr(o['ilon']))
    env.closed('amt_project_inverse')


def _oracle_project(a):
    import _projection_oracle as PO
    xp, P = PO.Float64(), PO.stere(*STERE)
    x, y = PO.forward(xp, P, a['lat'], a['lon'])
    ilat, ilon = PO.inverse(xp, P, a['px'], a['py'])
    return dict(x=x, y=y, ilat=ilat, ilon=ilon)


_rs = np.random.RandomState(14)
POLYGON = tuple(np.stack([c[0] + r * np.cos(np.linspace(0, 2 * np.pi, 9)[:-1]), c[1] + r * np.sin(np.linspace(0, 2 * np.pi, 9)[:-1])],
                         axis=1) for c, r in (((45.0, 18.0), 5.0), ((42.0, 24.0), 3.0)))
POLY_PTS = tuple((_rs.uniform(38.0, 52.0, N_PTS), _rs.uniform(8.0, 30.0, N_PTS)) for _ in range(2))


def _call_in_polygon(env):
    i = env.inp
    env.ctx.call('amt_points_in_polygon', _ptr(i['px']), _ptr(i['py']), N_PTS, _ptr(i['polygon']), 8, _ptr(env.out['inside']))
    env.closed('amt_points_in_polygon')


def _oracle_in_polygon(a):
    from oracle import ref_numpy as O
    return dict(inside=O.points_inside_polygon(np.stack([a['px'], a['py']], axis=1), a['polygon']))


_rs = np.random.RandomState(15)
HIST = tuple(dict(x=_rs.uniform(8.0, 30.0, N_PTS), y=_rs.uniform(38.0, 52.0, N_PTS),
                  w=_rs.randint(-9, 10, N_PTS).astype(np.float64)) for _ in range(2))


def _call_hist(env):
    import torch
    i, o = env.inp, env.out
    xa, ya = _axes(env.ctx)
    count = torch.zeros(NX * NY, dtype=torch.float64, device='cuda')            # (on the current stream: ordered)
    sums = torch.zeros(NX * NY, dtype=torch.float64, device='cuda')
    wp, sp = (C.c_void_p * 1)(i['w'].data_ptr()), (C.c_void_p * 1)(sums.data_ptr())
    env.ctx.call('amt_hist2d_accumulate', _ptr(i['x']), _ptr(i['y']), N_PTS, wp, 1, C.byref(xa), C.byref(ya), 0, _ptr(count), sp)
    env.closed('amt_hist2d_accumulate')
    env.ctx.call('amt_hist2d_finalize_mean', _ptr(count), sp, 1, NX, NY, _ptr(o['mean']))
    env.closed('amt_hist2d_finalize_mean')
    o['count'].copy_(count)


def _oracle_hist(a):
    import _bin_oracle as B
    count, ((s, bound),) = B.hist2d(a['x'], a['y'], [a['w']], XEDGES, YEDGES)
    assert not bound.any()                                                      # integer weights: the sums are exact
    with np.errstate(invalid='ignore', divide='ignore'):
        return dict(count=count, mean=B.hist_layout(s / count, NX, NY))


W2P_CAMERA, ZEN_CAMERA = 'cd-rotation-37', 'sip-2'         # cameras of tests/_inverse_cases.py: plain TAN; TAN with SIP terms
G_NY, G_NX = 13, 21


def _w2p_points():
    """(true, decoy) dicts of points in the geodetic frame: 257 scattered points and the axes of a 13 x 21 grid, inside the
    box of the points tests/_inverse_cases.py makes for the camera (on and around its footprint)"""
    if 'w2p' not in _kept:
        import _inverse_cases as IC
        r = IC.points(W2P_CAMERA)['geodetic']
        lat0, lat1, lon0, lon1 = r['c0'].min(), r['c0'].max(), r['c1'].min(), r['c1'].max()
        out = []
        for seed in (17, 18):
            rng = np.random.RandomState(seed)
            out.append(dict(c0=rng.uniform(lat0, lat1, N_PTS), c1=rng.uniform(lon0, lon1, N_PTS),
                            glat=np.sort(rng.uniform(lat0, lat1, G_NY)), glon=np.sort(rng.uniform(lon0, lon1, G_NX))))
        _kept['w2p'] = tuple(out)
    return _kept['w2p']


def _call_w2p(env):
    import _inverse_cases as IC
    i, o = env.inp, env.out
    p, z = IC.native(IC.by_name(W2P_CAMERA))
    assert z is None
    env.ctx.call('amt_world_to_pixel', C.byref(p), None, 0, _ptr(i['c0']), _ptr(i['c1']), N_PTS, _ptr(o['xy']), _ptr(o['elev']),
                 _ptr(o['flags']))
    env.closed('amt_world_to_pixel')
    env.ctx.call('amt_grid_to_pixel', C.byref(p), None, 0, _ptr(i['glat']), G_NY, _ptr(i['glon']), G_NX, _ptr(o['gxy32']),
                 _ptr(o['gxy']), _ptr(o['gelev']), _ptr(o['gflags']))
    env.closed('amt_grid_to_pixel')


def _oracle_w2p(a):
    import _inverse_cases as IC
    import _inverse_oracle as IO
    cam = IC.by_name(W2P_CAMERA)
    r = IO.inverse_arrays(IO.Float(), cam, IO.GEODETIC, a['c0'], a['c1'])
    la, lo = np.meshgrid(a['glat'], a['glon'], indexing='ij')
    g = IO.inverse_arrays(IO.Float(), cam, IO.GEODETIC, la, lo)
    gxy = np.stack([g['x'], g['y']], axis=-1)
    return dict(xy=np.stack([r['x'], r['y']], axis=-1), elev=r['elev'], flags=r['flags'], gxy=gxy, gxy32=gxy.astype(np.float32),
                gelev=g['elev'], gflags=g['flags'])


def _zen():
    import _inverse_cases as IC
    import _inverse_oracle as IO
    cam = IC.by_name(ZEN_CAMERA)
    return cam, IO.zen_struct(cam, corner=1)


def _call_zenithal(env):
    _, z = _zen()
    assert env.out['dirs'].shape == (z.height + 1, z.width + 1, 3)
    env.ctx.call('amt_directions_zenithal', C.byref(z), _ptr(env.out['dirs']))
    env.closed('amt_directions_zenithal')


def _zen_shape():
    cam, _ = _zen()
    return (cam['height'] + 1, cam['width'] + 1, 3)


LENS_K = (-0.01237, 0.0173)                                  # poly3: the true model and the decoy's


def _lens_coords(k):
    import _lens_oracle as LO
    return LO.forward_grid('poly3', [k], W, H)


def _call_lens(env):
    from auromat_amd._native import LensDebug, LensModel
    i, o = env.inp, env.out
    m = LensModel()
    m.kind, m.width, m.height = 1, W, H                      # AMT_LENS_POLY3
    m.k[:] = [LENS_K[0], 0.0, 0.0]
    for path, name in ((1, 'staged'), (2, 'gathered')):      # AMT_LENS_PATH_STAGED, AMT_LENS_PATH_GATHER
        dbg = LensDebug()
        dbg.force_path = path
        env.ctx.call('amt_lens_remap', C.byref(m), _ptr(i['img']), 2, 3, 1, _ptr(o[name]), _ptr(o['support']), C.byref(dbg))
        env.closed('amt_lens_remap')
        env.ctx.call('amt_remap_coords', _ptr(i['img']), W, H, 2, 3, _ptr(i['coords']), W, H, 1, _ptr(o['c_' + name]),
                     _ptr(o['c_support']), C.byref(dbg))
        env.closed('amt_remap_coords')


def _oracle_lens(a):
    import _lens_oracle as LO
    xy = _lens_coords(LENS_K[0])
    img, support = LO.remap(a['img'], xy[..., 0], xy[..., 1], 'lanczos4')
    c = a['coords'].astype(np.float64)
    c_img, c_support = LO.remap(a['img'], c[..., 0], c[..., 1], 'lanczos4')
    return dict(staged=img, gathered=img, c_staged=c_img, c_gathered=c_img, c_support=c_support)


# ---- C. per-frame statistics ---------------------------------------------------------------------------------------------------

def _frame_args(env, xa, ya):
    i = env.inp
    return [_ptr(i['lat_c']), _ptr(i['lon_c']), _ptr(i['elev']), _ptr(i['img']), 2, 3, None, H, W, MIN_ELEV, C.byref(xa),
            C.byref(ya), 0]


def _grid_ptrs(o, first='mean'):
    return [_ptr(o[first]), _ptr(o['img']), _ptr(o['mask']), _ptr(o['count'])]


def _call_bin(env):
    import torch
    xa, ya = _axes(env.ctx)
    acc = torch.zeros(5 * NX * NY, dtype=torch.int64, device='cuda')
    env.ctx.call('amt_bin_frame', *(_frame_args(env, xa, ya) + [_ptr(acc)]))
    env.closed('amt_bin_frame')
    env.ctx.call('amt_bin_frame_finalize', _ptr(acc), NX, NY, 3, 2, *_grid_ptrs(env.out))
    env.closed('amt_bin_frame_finalize')


def _oracle_bin(a):
    import _bin_oracle as B
    r = B.frame(_median_case(a))
    return dict(mean=r['mean'], img=r['img'], mask=r['mask'], count=r['count_f'])


def _call_median(env):
    xa, ya = _axes(env.ctx)
    env.ctx.call('amt_median_frame', *(_frame_args(env, xa, ya) + _grid_ptrs(env.out)))


def _call_median_async(env):
    xa, ya = _axes(env.ctx)
    env.ctx.call('amt_median_frame_async', *(_frame_args(env, xa, ya) + [0] + _grid_ptrs(env.out)))
    env.closed('amt_median_frame_async')


def _oracle_median(a):
    import _median_cases as MC
    r = MC.expected(_median_case(a))
    return dict(mean=r['median'], img=r['img'], mask=r['mask'], count=r['count'])


QS = (0.25, 0.9)


def _call_quantile_async(env):
    xa, ya = _axes(env.ctx)
    q = (C.c_double * 2)(*QS)
    env.ctx.call('amt_quantile_frame_async', *(_frame_args(env, xa, ya) + [0, q, 2] + _grid_ptrs(env.out)))
    env.closed('amt_quantile_frame_async')


def _oracle_quantile(a):
    import _quantile_oracle as Q
    from oracle import ref_numpy as O
    c = _median_case(a)
    planes = np.concatenate([c.img.astype(np.float64), c.elev[:, None]], axis=1)
    quant = Q.quantile_loop(c.lon, c.lat, planes, XEDGES, YEDGES, QS, keep=c.keep())
    img, _ = O.finalize_image(quant[..., :3], np.uint16)
    count = np.bincount(c.flat()[c.flat() >= 0], minlength=NX * NY).reshape(NY, NX)
    return dict(mean=quant, img=img, mask=count == 0, count=count)


QUANT_OUT = OrderedDict(GRID_OUT, mean=((2, NY, NX, 4), np.float64), img=((2, NY, NX, 3), np.uint16))
AREA_OUT = OrderedDict([('mean', ((NY, NX, 4), np.float64)), ('img', ((NY, NX, 3), np.uint16)), ('mask', ((NY, NX), np.uint8)),
                        ('count', ((NY, NX), np.float64))])             # (count: the coverage)
HALF = 1 << 31                                                           # minimum coverage 0.5 in units of 2^-32


def _area_args(env, xa, ya):
    i = env.inp
    return [_ptr(i['lat']), _ptr(i['lon']), _ptr(i['lat_c']), _ptr(i['elev']), _ptr(i['img']), 2, 3, None, H, W, MIN_ELEV,
            C.byref(xa), C.byref(ya), 0]


def _call_area(env):
    import torch
    xa, ya = _axes(env.ctx)
    acc = torch.zeros(5 * NX * NY, dtype=torch.int64, device='cuda')
    env.ctx.call('amt_area_frame', *(_area_args(env, xa, ya) + [_ptr(acc)]))
    env.closed('amt_area_frame')
    env.ctx.call('amt_area_frame_finalize', _ptr(acc), NX, NY, 3, 2, C.c_uint64(HALF), *_grid_ptrs(env.out))       # synchronises


def _call_area_async(env):
    xa, ya = _axes(env.ctx)
    env.ctx.call('amt_area_frame_async', *(_area_args(env, xa, ya) + [0, 0, H, C.c_uint64(HALF)] + _grid_ptrs(env.out) + [None]))
    env.closed('amt_area_frame_async')


class _AreaCase(object):
    def __init__(self, a):
        self.height, self.width = H, W
        self.lat, self.lon, self.lat_c, self.elev, self.img, self.mask = a['lat'], a['lon'], a['lat_c'], a['elev'], a['img'], None
        self.min_elevation, self.lon_wrap, self.xedges, self.yedges = MIN_ELEV, 0, XEDGES, YEDGES


def _oracle_area(a):
    import _area_oracle as A
    acc, _ = A.accumulate(_AreaCase(a))
    r = A.finalize(acc, np.uint16, 0.5)
    assert not r['over']
    return dict(mean=r['area'], img=r['img'], mask=r['mask'], count=r['coverage'])


TARGET_LAT = (YEDGES[:-1] + 0.5)[::-1].copy()                            # the grid centres, north to south
TARGET_LON = XEDGES[:-1] + 0.5
_rs = np.random.RandomState(16)
TARGET_MASK = tuple((_rs.uniform(size=(NY, NX)) < 0.25).astype(np.uint8) for _ in range(2))     # targets that are not searched
NEAREST_OUT = OrderedDict([('index', ((NY, NX), np.int64)), ('mean', ((NY * NX, 4), np.float64)), ('img', ((NY * NX, 3), np.uint16)),
                           ('mask', ((NY * NX,), np.uint8))])


def _call_nearest(env):
    from _gated_stream import dev
    i, o = env.inp, env.out
    xa, ya = _axes(env.ctx)
    key = _key('targets', env.ctx)
    if key not in _kept:                                                 # (constants of the case: uploaded once per context)
        _kept[key] = (dev(TARGET_LAT), dev(TARGET_LON))
    tlat, tlon = _kept[key]
    env.ctx.call('amt_nearest_frame', _ptr(i['lat_c']), _ptr(i['lon_c']), _ptr(i['elev']), None, H, W, MIN_ELEV, C.byref(xa),
                 C.byref(ya), 0, _ptr(tlat), _ptr(tlon), _ptr(i['target_mask']), _ptr(o['index']))
    env.closed('amt_nearest_frame')
    env.ctx.call('amt_nearest_gather', _ptr(o['index']), NY * NX, _ptr(i['img']), 2, 3, _ptr(i['elev']), _ptr(o['mean']),
                 _ptr(o['img']), _ptr(o['mask']))
    env.closed('amt_nearest_gather')


def _oracle_nearest(a):
    import _interp_oracle as I
    valid = I.valid_sources(a['lat_c'], a['lon_c'], a['elev'], None, MIN_ELEV)
    index = I.nearest_exact(a['lat_c'], a['lon_c'], valid, 0, TARGET_LAT, TARGET_LON, a['target_mask'])
    mean, img, mask = I.gather(index, a['img'].reshape(-1, 3), a['elev'])
    return dict(index=index, mean=mean, img=img, mask=mask)


# ---- B. tables uploaded from host vectors -----------------------------------------------------------------------------------------

WINDOWS = ((0, 0, 14, NY), (6, 0, 14, NY))                               # two members whose windows overlap in 8 columns
MEMBER_B = (scene(3, 40.5, 13.0), scene(4, 39.75, 12.25))
MOSAIC_OUT = OrderedDict(GRID_OUT, source=((NY, NX), np.int32))


def _mosaic_inputs():
    d = OrderedDict()
    for k in ('lat', 'lon', 'lat_c', 'lon_c', 'elev', 'img'):
        d['a_' + k] = (TRUE[k], DECOY[k])
        d['b_' + k] = (MEMBER_B[0][k], MEMBER_B[1][k])
    return d


def _members(env, struct, corners):
    table = (struct * 2)()
    for m, (pre, win) in enumerate(zip('ab', WINDOWS)):
        i = lambda k: env.inp[pre + '_' + k].data_ptr()
        if corners:
            table[m].lat, table[m].lon = i('lat'), i('lon')
        else:
            table[m].lon_c = i('lon_c')
        table[m].lat_c, table[m].elev, table[m].img, table[m].center_mask = i('lat_c'), i('elev'), i('img'), None
        table[m].height, table[m].width = H, W
        table[m].win_x0, table[m].win_y0, table[m].win_nx, table[m].win_ny = win
    return table


def _call_mosaic(name, synchronises):
    def call(env):
        from auromat_amd._native import AreaMosaicMember, MosaicMember
        o = env.out
        xa, ya = _axes(env.ctx)
        area = name == 'amt_area_mosaic_frames'
        table = _members(env, AreaMosaicMember if area else MosaicMember, area)
        env.ctx.call(name, table, 2, 2, 3, MIN_ELEV, C.byref(xa), C.byref(ya), 0, 1, *(([C.c_uint64(HALF)] if area else []) +
                                                                                    _grid_ptrs(o) + [_ptr(o['source'])]))
        # (never freed in a session: a late reader would find valid pointers)
        _kept.setdefault(_key('tables', env.ctx), []).append(table)
        if not synchronises:
            env.closed(name)
    return call


def _member_cases(a, corners=False):
    out = []
    for pre in 'ab':
        sub = dict((k, a[pre + '_' + k]) for k in ('lat', 'lon', 'lat_c', 'lon_c', 'elev', 'img'))
        sub['img_mask'] = None
        out.append(_AreaCase(sub) if corners else _median_case(sub))
    return out


def _oracle_mosaic(a):
    import _bin_oracle as B
    r = B.mosaic(_member_cases(a), WINDOWS, 1)
    return dict(mean=r['mean'], img=r['img'], mask=r['mask'], count=r['count_f'], source=r['source'])


def _oracle_mosaic_area(a):
    import _mosaic_area_oracle as MA
    r = MA.mosaic(_member_cases(a, corners=True), WINDOWS, 1, 0.5)
    return dict(mean=r['area'], img=r['img'], mask=r['mask'], count=r['coverage'], source=r['source'])


CUBIC_ROWS, CUBIC_M = 7, 40                                   # 49 points in 7 pixel rows, 40 targets


def cubic_inputs():
    """(true, decoy) dicts of the arrays amt_cubic_gradients_csr and amt_cubic_eval read.  True: a jittered 7 x 7 lattice, its
    Delaunay triangulation (amt_delaunay_create, host code of the library), the neighbour lists and the located targets.
    Decoy: another lattice, a graph of the same sizes in which vertex i has the neighbours i + 1, i + 2, ... (mod n), triangles
    (t, t + 1, t + 8) (mod n), rows of other lengths: every index is a vertex, no list holds its own vertex, and the rows are a
    partition of the points (the relaxation visits every point: one that no row holds would never hand on its gradient)."""
    if 'cubic' in _kept:
        return _kept['cubic']
    from auromat_amd import _native
    L = _native.lib()
    n = CUBIC_ROWS * CUBIC_ROWS
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def lattice(seed):
        rng = np.random.RandomState(seed)
        r, c = np.divmod(np.arange(n), CUBIC_ROWS)
        return np.ascontiguousarray(np.stack([c + rng.uniform(-0.3, 0.3, n), r + rng.uniform(-0.3, 0.3, n)], axis=1))

    xy = lattice(21)
    handle = C.c_void_p()
    assert L.amt_delaunay_create(p(xy), n, C.byref(handle)) == 0
    nt, nn, nd = C.c_int64(), C.c_int64(), C.c_int64()
    assert L.amt_delaunay_sizes(handle, C.byref(nt), C.byref(nn), C.byref(nd)) == 0 and nd.value == 0
    indptr, indices = np.empty(n + 1, dtype=np.int64), np.empty(nn.value, dtype=np.int32)
    assert L.amt_delaunay_vertex_neighbours(handle, p(indptr), p(indices)) == 0
    rng = np.random.RandomState(22)
    targets = np.ascontiguousarray(rng.uniform(-0.6, CUBIC_ROWS - 0.4, (CUBIC_M, 2)))
    vertices, centroids = np.empty((CUBIC_M, 3), dtype=np.int32), np.empty((CUBIC_M, 3, 2))
    has_nb = np.empty((CUBIC_M, 3), dtype=np.uint8)
    assert L.amt_delaunay_locate(handle, p(targets), CUBIC_M, p(vertices), p(centroids), p(has_nb)) == 0
    L.amt_delaunay_destroy(handle)
    assert (vertices[:, 0] < 0).any() and (vertices[:, 0] >= 0).sum() > 20          # targets outside the hull, and inside
    centroids = np.where(has_nb[..., None] != 0, centroids, 0.0)                  # (what locate leaves without a neighbour is not read)
    row_start = np.arange(0, n + 1, CUBIC_ROWS, dtype=np.int64)
    true = dict(xy=xy, indptr=indptr, indices=indices, row_start=row_start, values=_q(rng.uniform(0.0, 100.0, (n, 2)), 1 / 64.0),
                targets=targets, vertices=vertices, centroids=centroids, has_nb=has_nb)
    k = len(indices) // n
    d_indptr = np.concatenate([np.arange(n) * k, [len(indices)]]).astype(np.int64)
    d_indices = np.concatenate([(i + 1 + np.arange(d_indptr[i + 1] - d_indptr[i])) % n for i in range(n)]).astype(np.int32)
    t = np.arange(CUBIC_M)
    decoy = dict(xy=lattice(23), indptr=d_indptr, indices=d_indices, row_start=np.array([0, 6, 14, 21, 27, 35, 42, 49], dtype=np.int64),
                 values=_q(rng.uniform(0.0, 100.0, (n, 2)), 1 / 64.0), targets=np.ascontiguousarray(rng.uniform(0.5, 5.5, (CUBIC_M, 2))),
                 vertices=np.stack([t % n, (t + 1) % n, (t + 8) % n], axis=1).astype(np.int32),
                 centroids=np.ascontiguousarray(rng.uniform(0.0, 6.0, (CUBIC_M, 3, 2))), has_nb=(1 - np.minimum(has_nb, 1)).astype(np.uint8))
    _kept['cubic'] = (true, decoy)
    return _kept['cubic']


def _call_cubic(env):
    i, o = env.inp, env.out
    n = CUBIC_ROWS * CUBIC_ROWS
    sweeps = (C.c_int32 * 2)()
    # (reports the sweeps of every channel to the host: waits for the stream)
    env.ctx.call('amt_cubic_gradients_csr', _ptr(i['xy']), n, _ptr(i['indptr']), _ptr(i['indices']), _ptr(i['row_start']), CUBIC_ROWS,
                 _ptr(i['values']), 2, 1e-6, 400, _ptr(o['gradients']), sweeps)
    env.ctx.call('amt_cubic_eval', CUBIC_M, _ptr(i['targets']), _ptr(i['vertices']), _ptr(i['centroids']), _ptr(i['has_nb']),
                 _ptr(i['xy']), _ptr(i['values']), _ptr(o['gradients']), 2, _ptr(o['out']))
    return dict(sweeps=list(sweeps))


def _oracle_cubic(a):
    from oracle import ref_numpy as O
    n = len(a['xy'])
    grad = np.zeros((n, 2, 2))
    out = np.full((CUBIC_M, 2), np.nan)
    with np.errstate(all='ignore'):
        for ch in range(2):
            grad[:, ch, :], _ = O.clough_tocher_gradients(a['xy'], a['indptr'], a['indices'], a['values'][:, ch], maxiter=40)
        for t in range(CUBIC_M):
            v = a['vertices'][t]
            if v[0] < 0:
                continue
            tri = a['xy'][v]
            T = np.array([[tri[0, 0] - tri[2, 0], tri[1, 0] - tri[2, 0]], [tri[0, 1] - tri[2, 1], tri[1, 1] - tri[2, 1]]])
            b01 = np.linalg.solve(T, a['targets'][t] - tri[2])
            b = (b01[0], b01[1], 1.0 - b01[0] - b01[1])
            nb = [a['centroids'][t, k] if a['has_nb'][t, k] else None for k in range(3)]
            for ch in range(2):
                out[t, ch] = O.clough_tocher_value(tri, b, a['values'][v, ch], grad[v, ch, :], nb)
    return dict(gradients=grad, out=out)


S_LAT, S_LON = np.linspace(51.0, 39.0, NY + 1), np.linspace(9.0, 29.0, NX + 1)       # corner rows and columns of a strip's frame
S_OFFSET = (0, 10)                                                       # columns of the raster the two frames start at
S_NX = NX + S_OFFSET[1]
_octagon = lambda lat, lon, r: np.stack([lat + r * np.cos(np.linspace(0, 2 * np.pi, 9)[:-1]),
                                         lon + 1.6 * r * np.sin(np.linspace(0, 2 * np.pi, 9)[:-1])], axis=1)


def _strip(seed, centre):
    rng = np.random.RandomState(seed)
    return dict(polygon=_octagon(centre[0], centre[1], centre[2]), cell_mask=(rng.uniform(size=(NY, NX)) < 0.15).astype(np.uint8),
                planes=_q(rng.uniform(0.0, 500.0, (NY, NX, 4)), 1 / 64.0), img=rng.randint(0, 65535, (NY, NX, 3)).astype(np.uint16))


STRIPS = ((_strip(31, (45.0, 16.0, 4.6)), _strip(32, (44.0, 21.0, 3.7))),      # per strip: (true, decoy)
          (_strip(33, (46.0, 20.0, 4.2)), _strip(34, (45.5, 15.0, 3.9))))


def _scanline_inputs():
    return OrderedDict(('%s%d' % (k, s), (STRIPS[s][0][k], STRIPS[s][1][k])) for s in range(2)
                       for k in ('polygon', 'cell_mask', 'planes', 'img'))


def _call_scanline(env):
    import torch
    from _gated_stream import dev
    from auromat_amd._native import ScanLineStrip
    i, o, ctx = env.inp, env.out, env.ctx
    key = _key('scan_axes', ctx)
    if key not in _kept:
        _kept[key] = (dev(S_LAT), dev(S_LON))
    lat, lon = _kept[key]
    table = (ScanLineStrip * 2)()
    held = []
    for s in range(2):
        keep = torch.zeros((NY, NX), dtype=torch.uint8, device='cuda')
        stats = torch.zeros(5, dtype=torch.int64, device='cuda')
        ctx.call('amt_scanline_select', _ptr(lat), _ptr(lon), NY, NX, _ptr(i['polygon%d' % s]), 8, _ptr(i['cell_mask%d' % s]), 0, 0,
                 NY, NX, _ptr(keep), _ptr(stats))
        if s == 0:
            env.closed('amt_scanline_select')
        count = int(stats.cpu()[0])                              # the host needs the count: waits for the stream
        assert 0 < count <= NY * NX
        rec = dict(row=torch.zeros(NY * NX, dtype=torch.int32, device='cuda'), col=torch.zeros(NY * NX, dtype=torch.int32, device='cuda'),
                   planes=torch.zeros((4, NY * NX), dtype=torch.float64, device='cuda'),
                   img=torch.zeros((3, NY * NX), dtype=torch.int16, device='cuda'))
        # (record arrays of `count` elements each: plane p of the records starts at p * count)
        ctx.call('amt_scanline_pack', _ptr(keep), 0, 0, NY, NX, _ptr(i['planes%d' % s]), 4, _ptr(i['img%d' % s]), 2, 3, NY, NX, 0,
                 S_OFFSET[s], count, _ptr(rec['row']), _ptr(rec['col']), _ptr(rec['planes']), _ptr(rec['img']))
        table[s].row, table[s].col, table[s].planes, table[s].img = (rec[k].data_ptr() for k in ('row', 'col', 'planes', 'img'))
        table[s].count, table[s].frame = count, s
        held.append((keep, stats, rec))
    ctx.call('amt_scanline_compose', table, 2, 2, 3, 4, 0, 0, NY, S_NX, _ptr(o['planes']), _ptr(o['img']), _ptr(o['mask']),
             _ptr(o['frame_index']))
    _kept.setdefault(_key('tables', ctx), []).append((table, held))


def _oracle_scanline(a):
    import _scanline_oracle as SO
    window = (0, 0, NY, NX)
    strips = []
    for s in range(2):
        keep, _ = SO.select(S_LAT, S_LON, a['polygon%d' % s], a['cell_mask%d' % s], window)
        strips.append(SO.pack(keep, window, a['planes%d' % s], a['img%d' % s], 0, S_OFFSET[s]))
    planes, img, mask, index, outside = SO.compose(strips, [0, 1], 0, 0, NY, S_NX, 4, 3, np.uint16)
    assert not outside
    return dict(planes=planes, img=img, mask=mask, frame_index=index)


# ---- D. the frame driver -----------------------------------------------------------------------------------------------------------

GEOREF_BOX = (44.0, -108.0, 58.0, -86.0)                                 # south, west, north, east: holds the frame's footprint
TURN = (-60.0, -30.0)                                                    # the decoy camera: right ascension, declination [deg]
CELLS_CAP = 1024                                                         # room for the grid of a frame (13 x 21 cells at 2 px/deg)
DRIVER_OUT = OrderedDict([('mean', ((CELLS_CAP, 4), np.float64)), ('img', ((CELLS_CAP, 3), np.uint16)), ('mask', ((CELLS_CAP,), np.uint8)),
                          ('count', ((CELLS_CAP,), np.float64))])
GEO = ('lat', 'lon', 'lat_c', 'lon_c', 'elev')
SW, SH = 64, 17                                                          # one strip plus one column, one band plus one row
GEO_OUT = OrderedDict([(k, ((H + 1, W + 1) if k in ('lat', 'lon') else (H, W), np.float64)) for k in GEO])


def camera(turned=False, k=0, width=W, height=H):
    """(header, camera, time) of frame k of the synthetic sequence; `turned`: the same camera looking at TURN further on"""
    from auromat_amd.synthetic import sequence_frame
    hdr, cam, t, _ = sequence_frame(k, width, height)
    if turned:
        hdr = dict(hdr, CRVAL1=hdr['CRVAL1'] + TURN[0], CRVAL2=hdr['CRVAL2'] + TURN[1])
    return hdr, cam, t


def directions(turned=False, width=W, height=H):
    from oracle import ref_numpy as O
    return np.ascontiguousarray(O.pixel_directions(camera(turned, 0, width, height)[0], corner=True))


def frame_of_directions(dirs, k=0, width=W, height=H):
    """oracle.ref_numpy.georef_frame from a direction array (camera position and time of frame k): coordinates, elevation and
    the box of the corners that mask_by_elevation keeps"""
    from oracle import ref_numpy as O
    _, cam, t = camera(False, k, width, height)
    m_geo = O.mat_j2000_to_geo(O.date2es(t))
    p_c = O.inflated_earth_intersection(dirs.reshape(-1, 3), cam, ALTITUDE).reshape(dirs.shape)
    dir_m = O.calc_centers(dirs)
    with np.errstate(invalid='ignore'):
        p_m = O.calc_centers(p_c)
    lat, lon = (v.reshape(dirs.shape[:2]) for v in O.j2000_to_latlon(p_c.reshape(-1, 3), m_geo))
    lat_c, lon_c = (v.reshape(p_m.shape[:2]) for v in O.j2000_to_latlon(p_m.reshape(-1, 3), m_geo))
    elev = O.elevation_deg(dir_m, p_m)
    corner, centre = O.mask_by_elevation(elev, np.isnan(lat), MIN_ELEV)
    box, _ = O.bbox_of_corners(lat, lon, corner)
    return dict(lat=lat, lon=lon, lat_c=lat_c, lon_c=lon_c, elev=elev, box=np.array(box), keep=~centre)


def camera_frame(k=0, width=W, height=H):
    """the same for the camera model of frame k"""
    from oracle import ref_numpy as O
    return frame_of_directions(O.pixel_directions(camera(False, k, width, height)[0], corner=True), k, width, height)


def grid_edges(box):
    """(xedges, yedges) of the grid the library lays out at PX_PER_DEG for box = (south, west, north, east): amt_grid_layout, host
    arithmetic (tests/test_host_cpu.py pins it to the reference's)"""
    from auromat_amd import _native
    g = _native.Grid()
    south, west, north, east = (float(v) for v in box)
    assert _native.lib().amt_grid_layout(PX_PER_DEG, PX_PER_DEG, south, north, west, east, C.byref(g)) == 0
    return np.linspace(g.xaxis.first, g.xaxis.last, g.xaxis.nbin + 1), np.linspace(g.yaxis.first, g.yaxis.last, g.yaxis.nbin + 1)


def binned(f, img, box=None, integers=False):
    """tests/_bin_oracle.py on the oracle's centre coordinates of a frame `f` (frame_of_directions) and an image: the grids of
    resample(method='mean') for the frame's own box, or the integer planes on the grid of another box"""
    import _bin_oracle as B
    import _median_cases as MC
    xe, ye = grid_edges(f['box'] if box is None else box)
    h, w = f['elev'].shape
    sky = np.isnan(f['lat_c']) | np.isnan(f['elev'])
    case = MC.Case('frame', None, np.where(sky, 0.0, f['lat_c']).ravel(), np.where(sky, 0.0, f['lon_c']).ravel(),
                   np.where(sky, 0.0, f['elev']).ravel(), img.reshape(-1, 3), sky.ravel().astype(np.uint8), xe, ye, h, w,
                   min_elevation=MIN_ELEV, uniform=True)
    if integers:
        p = B.planes(case)
        return np.concatenate([p['count'].ravel(), p['sums'].ravel(), p['fx'].ravel()])
    r = B.frame(case)
    return dict(mean=r['mean'], img=r['img'], mask=r['mask'], count=r['count_f'])


def image(seed, width=W, height=H):
    from auromat_amd.synthetic import frame_image
    return frame_image(width, height, seed=seed)


def _params(k=0, width=W, height=H):
    from auromat_amd.mapping.astrometry import frame_params
    hdr, cam, t = camera(False, k, width, height)
    return frame_params(hdr, ALTITUDE, cam, t, True, magnetic=False)


def _kept_sums(img, keep):
    return img.reshape(-1, 3)[np.ravel(keep)].astype(np.int64).sum(axis=0)


def _oracle_camera(n_frames):
    """the grids of every frame: oracle.ref_numpy's coordinates, tests/_bin_oracle.py's means on the grid of the frame's box"""
    def oracle(a):
        out = {}
        for k in range(n_frames):
            r = binned(camera_frame(k), a['img%d' % k])
            # (which cells are filled and by how many pixels is the camera model's business: the image decides means and colours)
            out.update((name + (str(k) if n_frames > 1 else ''), r[name]) for name in ('mean', 'img'))
        return out
    return oracle


def _oracle_georef_frame(a):
    """the accumulator planes of the fused binning on the grid _call_georef_frame lays out"""
    return dict(acc=binned(camera_frame(), a['img0'], box=GEOREF_BOX, integers=True))


def _oracle_dirs(with_image, coordinates=True, width=W, height=H):
    def oracle(a):
        f = frame_of_directions(a['dirs'], 0, width, height)
        out = dict((k, f[k]) for k in (GEO if coordinates else ()) + ('box',))
        if with_image:
            out.update(binned(f, a['img0']))
        return out
    return oracle


def _georef_out(out, names=GEO):
    from auromat_amd._native import GeorefOut
    g = GeorefOut()
    for k in names:
        if k in out:
            setattr(g, k, out[k].data_ptr())
    g.altitude = ALTITUDE
    return g


class Driver(object):
    """amt_pipe handles per context (keyed by its handle: every host thread has a context of its own), kept for the session
    (their streams belong to the context)"""
    _pipes = {}

    @classmethod
    def get(cls, ctx, n=1):
        pipes = cls._pipes.setdefault(ctx.handle.value, [])
        while len(pipes) < n:
            h = C.c_void_p()
            ctx.call('amt_pipe_create', C.byref(h))
            pipes.append(h)
        return pipes[:n]


def release():
    """Give back what the cases keep for the session: the drivers, the sequence pipeline, device constants and host tables."""
    import torch
    torch.cuda.synchronize()
    from auromat_amd import _native
    while Driver._pipes:
        for h in Driver._pipes.popitem()[1]:
            _native.lib().amt_pipe_destroy(h)
    for key in [k for k in _kept if isinstance(k, tuple) and k[0] in ('seq', 'targets', 'scan_axes', 'host_images', 'tables')]:
        del _kept[key]


def _check(ctx, rc):
    ctx.check(rc)


def _result_values(res):
    g = res.grid
    return dict(status=res.status, fused=res.fused, lon_wrapped=res.lon_wrapped, bbox=tuple(res.bbox), ny=g.ny, nx=g.nx,
                grid=(g.lat_lo, g.lat_hi, g.lon_lo, g.lon_hi, g.lat_step, g.lon_step, g.lat_center_first, g.lon_center_first))


def _finalize_behind_a_held_stream(env, pipes, results, many):
    """amt_pipe_finalize[_many] into arrays allocated FOR the finalise stream — include/auromat_hip.h, amt_pipe_finalize_stream:
    "A host whose allocator is stream ordered (PyTorch's caching allocator, hipMallocAsync pools) must allocate the four output
    buffers FOR THIS STREAM" — while that stream is held by a short sleep, then amt_pipe_join and, on the context's stream, the
    copy into the case's outputs: a consumer on the context's stream that the join has to order behind the finalise kernel."""
    import torch
    from _gated_stream import POISON, cycles_per_ms
    ctx, lib = env.ctx, env.ctx._lib
    handle = C.c_void_p()
    _check(ctx, lib.amt_pipe_finalize_stream(pipes[0], C.byref(handle)))
    fin = torch.cuda.ExternalStream(handle.value)
    cur = torch.cuda.current_stream()
    bufs = []
    with torch.cuda.stream(fin):
        torch.cuda._sleep(int(cycles_per_ms() * FIN_HOLD_MS))
        for r in results:
            n = r.grid.ny * r.grid.nx
            b = dict(mean=torch.empty((n, 4), dtype=torch.float64, device='cuda'), img=torch.empty((n, 3), dtype=torch.int16, device='cuda'),
                     mask=torch.empty((n,), dtype=torch.uint8, device='cuda'), count=torch.empty((n,), dtype=torch.float64, device='cuda'))
            for t in b.values():
                t.view(torch.uint8).fill_(POISON)
                t.record_stream(cur)
            bufs.append(b)
    if many:
        n = len(pipes)
        arr = lambda k: (C.c_void_p * n)(*[b[k].data_ptr() for b in bufs])
        _check(ctx, lib.amt_pipe_finalize_many((C.c_void_p * n)(*[p.value for p in pipes]), n, arr('mean'), arr('img'), arr('mask'), arr('count')))
    else:
        b = bufs[0]
        _check(ctx, lib.amt_pipe_finalize(pipes[0], _ptr(b['mean']), _ptr(b['img']), _ptr(b['mask']), _ptr(b['count'])))
    # (amt_pipe_wait has synchronised: the gate is open by now, what holds the finalise kernel back is the sleep above)
    for p in pipes:
        _check(ctx, lib.amt_pipe_join(p))
    for k, b in enumerate(bufs):
        suffix = '' if len(bufs) == 1 else str(k)
        for name, t in b.items():
            env.out[name + suffix][:t.shape[0]].copy_(t)


def _call_camera_path(env):
    from auromat_amd._native import PipeResult
    ctx, lib = env.ctx, env.ctx._lib
    pipe, = Driver.get(ctx)
    p, out = _params(), _georef_out({})
    _check(ctx, lib.amt_pipe_coarse(pipe, C.byref(p), MIN_ELEV, 0))
    env.closed('amt_pipe_coarse')
    _check(ctx, lib.amt_pipe_launch(pipe, C.byref(p), C.byref(out), _ptr(env.inp['img0']), 2, MIN_ELEV, PX_PER_DEG, PX_PER_DEG, -1, 0))
    env.closed('amt_pipe_launch')
    res = PipeResult()
    _check(ctx, lib.amt_pipe_wait(pipe, C.byref(res)))                   # synchronises
    assert res.status == 0 and res.grid.ny * res.grid.nx <= CELLS_CAP, (res.status, res.grid.ny, res.grid.nx)
    _finalize_behind_a_held_stream(env, [pipe], [res], many=False)
    return _result_values(res)


N_MANY = 3


def _call_camera_many(env):
    from auromat_amd._native import PipeResult
    ctx, lib = env.ctx, env.ctx._lib
    pipes = Driver.get(ctx, N_MANY)
    params = [_params(k) for k in range(N_MANY)]
    outs = [_georef_out({}) for _ in range(N_MANY)]
    for pipe, p in zip(pipes, params):
        _check(ctx, lib.amt_pipe_coarse(pipe, C.byref(p), MIN_ELEV, 0))
    env.closed('amt_pipe_coarse')
    arr = lambda items: (C.c_void_p * N_MANY)(*items)
    _check(ctx, lib.amt_pipe_launch_many(arr(p.value for p in pipes), N_MANY, arr(C.addressof(p) for p in params),
                                         arr(C.addressof(o) for o in outs), arr(env.inp['img%d' % k].data_ptr() for k in range(N_MANY)),
                                         2, MIN_ELEV, PX_PER_DEG, PX_PER_DEG, -1, 0))
    env.closed('amt_pipe_launch_many')
    results = []
    for pipe in pipes:
        res = PipeResult()
        _check(ctx, lib.amt_pipe_wait(pipe, C.byref(res)))
        assert res.status == 0 and res.grid.ny * res.grid.nx <= CELLS_CAP, (res.status, res.grid.ny, res.grid.nx)
        results.append(res)
    _finalize_behind_a_held_stream(env, pipes, results, many=True)
    return dict(('frame%d' % k, _result_values(r)) for k, r in enumerate(results))


def _call_georef_frame(env):
    """amt_georef_frame with the binning fused in: the image decides the accumulators"""
    import torch
    from auromat_amd._native import Grid
    ctx = env.ctx
    g = Grid()
    south, west, north, east = GEOREF_BOX
    assert ctx._lib.amt_grid_layout(PX_PER_DEG, PX_PER_DEG, south, north, west, east, C.byref(g)) == 0
    assert 5 * g.nx * g.ny == env.out['acc'].numel(), (g.nx, g.ny)
    out = _georef_out(env.out)
    out.bbox, out.bbox_min_elevation = env.out['bbox'].data_ptr(), MIN_ELEV
    out.bin_xaxis, out.bin_yaxis = C.addressof(g.xaxis), C.addressof(g.yaxis)
    out.bin_img, out.bin_img_dtype, out.bin_acc = env.inp['img0'].data_ptr(), 2, env.out['acc'].data_ptr()
    env.out['acc'].zero_()                                               # on the current stream: ordered before the kernel
    p = _params()
    ctx.call('amt_georef_frame', C.byref(p), C.byref(out))
    env.closed('amt_georef_frame')


def _call_georef_frame_dirs(env):
    ctx = env.ctx
    out = _georef_out(env.out)
    out.bbox, out.bbox_min_elevation = env.out['box'].data_ptr(), MIN_ELEV
    height, width = env.out['elev'].shape                            # (127 x 33, or the frame of one strip plus one column)
    assert tuple(env.inp['dirs'].shape) == (height + 1, width + 1, 3)
    p = _params(0, width, height)
    ctx.call('amt_georef_frame_dirs', C.byref(p), _ptr(env.inp['dirs']), C.byref(out))
    env.closed('amt_georef_frame_dirs')


def _call_dirs_path(env):
    """the suspect: amt_pipe_coarse_dirs reads the caller's directions on the driver's own stream"""
    from auromat_amd._native import PipeResult
    ctx, lib = env.ctx, env.ctx._lib
    pipe, = Driver.get(ctx)
    p, out = _params(), _georef_out(env.out)
    _check(ctx, lib.amt_pipe_coarse_dirs(pipe, C.byref(p), _ptr(env.inp['dirs']), MIN_ELEV, 0))
    env.closed('amt_pipe_coarse_dirs')
    # (the launch waits on the host for the estimate, and the estimate for the directions: it returns when the gate is open)
    _check(ctx, lib.amt_pipe_launch_dirs(pipe, C.byref(p), _ptr(env.inp['dirs']), C.byref(out), _ptr(env.inp['img0']), 2, MIN_ELEV,
                                         PX_PER_DEG, PX_PER_DEG, 0, 0))
    res = PipeResult()
    _check(ctx, lib.amt_pipe_wait(pipe, C.byref(res)))
    values = _result_values(res)
    if res.status == 0 and res.grid.ny * res.grid.nx <= CELLS_CAP:
        _finalize_behind_a_held_stream(env, [pipe], [res], many=False)
    # in every run, the settled ones too: the frame is fused and finalised by the driver, not handed back
    assert (res.status, res.fused) == (0, 1), ('amt_pipe_wait handed the frame back', values)
    return values


def _call_pipeline_run(env):
    """FramePipeline.run(..., fuse=True, dirs=tensor): the single-pass plan without a second launch, as on settled inputs"""
    from auromat_amd.pipeline import FramePipeline
    pipe = FramePipeline(W, H, alloc_image=False)
    pipe.use_image(env.inp['img0'])
    res = pipe.run(None, ALTITUDE, None, None, fast=True, min_elevation=MIN_ELEV, pxPerDeg=PX_PER_DEG, params=_params(),
                   keep_on_device=True, fuse=True, dirs=env.inp['dirs'], containsPole=False)
    n = res['mean'].shape[0] * res['mean'].shape[1]
    assert n <= CELLS_CAP
    env.out['mean'][:n].copy_(res['mean'].reshape(n, 4))
    env.out['img'][:n].copy_(res['img'].reshape(n, 3))
    env.out['mask'][:n].copy_(res['mask'].reshape(n))
    env.out['count'][:n].copy_(res['count'].reshape(n))
    values = dict(plan=pipe.last_plan, retried=bool(pipe._fused.get('retried')), shape=tuple(res['mean'].shape))
    # in every run, the settled ones too: one launch of the single-pass plan
    assert values['plan'] == 'single-pass' and not values['retried'], values
    return values


# ---- E. the sequence runner ----------------------------------------------------------------------------------------------------------

RW, RH, R_FRAMES = 64, 48, 4
R_CELLS = 4096
_pad64 = lambda n: (n + 63) // 64 * 64                                   # every array of a slot starts on a 512-byte boundary
SLOT_DOUBLES = 2 * _pad64((RH + 1) * (RW + 1)) + 3 * _pad64(RH * RW)
RUN_OUT = OrderedDict([('grids', ((5 * R_CELLS + 64,), np.float64)), ('images', ((7 * R_CELLS + 256 * (R_FRAMES + 1),), np.uint8)),
                       ('slots', ((2, SLOT_DOUBLES), np.float64))])


def _slot_arrays(slots):
    """the five coordinate arrays of the runner's two slots as views of one output"""
    from auromat_amd._native import GeorefOut
    table = (GeorefOut * 2)()
    nc, nm = (RH + 1) * (RW + 1), RH * RW
    for s in range(2):
        at = 0
        for k in GEO:
            n = nc if k in ('lat', 'lon') else nm
            setattr(table[s], k, slots[s, at:at + n].data_ptr())
            at += _pad64(n)
    return table


def _run_frames(env, image_of):
    """amt_run_begin / amt_run_push / amt_run_end over the four frames: one frame per launch, two slots"""
    from auromat_amd._native import RunConfig, RunResult
    from auromat_amd.mapping.astrometry import run_frame
    ctx, lib = env.ctx, env.ctx._lib
    table = _slot_arrays(env.out['slots'])
    cfg = RunConfig(width=RW, height=RH, img_dtype=2, fast_center=1, magnetic=0, batch=1, use_hints=1, n_slots=2, two_pass=0,
                    statistic=0, altitude=ALTITUDE, min_elevation=MIN_ELEV, lat_px_per_deg=PX_PER_DEG, lon_px_per_deg=PX_PER_DEG,
                    slots=table, arcsec_per_px=0.0)
    run = C.c_void_p()
    ctx.call('amt_run_create', C.byref(cfg), C.byref(run))
    try:
        rec = (RunResult * R_FRAMES)()
        g, im = env.out['grids'], env.out['images']
        _check(ctx, lib.amt_run_begin(run, g.data_ptr(), g.numel(), im.data_ptr(), im.numel(), rec, R_FRAMES))
        env.closed('amt_run_begin')
        for k in range(R_FRAMES):
            hdr, cam, t = camera(False, k, RW, RH)
            dev_ptr, host_ptr = image_of(k)
            _check(ctx, lib.amt_run_push(run, C.byref(run_frame(hdr, cam, t, ALTITUDE, dev_ptr, img_host_ptr=host_ptr))))
            if k < 2:
                env.closed('amt_run_push %d' % k)            # (the third push finishes the first frame: it waits for its box)
        done = C.c_int32(0)
        _check(ctx, lib.amt_run_end(run, C.byref(done)))
        table_out = np.frombuffer(rec, dtype=np.dtype(RunResult)).copy()
    finally:
        lib.amt_run_destroy(run)
    assert done.value == R_FRAMES and (table_out['status'] == 0).all(), (done.value, table_out['status'].tolist())
    return dict((k, table_out[k].tolist()) for k in ('status', 'ny', 'nx', 'grid_offset', 'image_offset', 'retried', 'lon_wrapped'))


def _call_run_device(env):
    return _run_frames(env, lambda k: (env.inp['img%d' % k].data_ptr(), None))


def _call_run_host(env):
    """page-locked host images: the runner's copy stream takes them to buffers of its own"""
    import torch
    key = _key('host_images', env.ctx)
    if key not in _kept:
        _kept[key] = [torch.from_numpy(image(40 + k, RW, RH).view(np.int16)).pin_memory() for k in range(R_FRAMES)]
    return _run_frames(env, lambda k: (None, _kept[key][k].data_ptr()))


def _call_sequence_pipeline(env):
    """SequencePipeline.process with device images on whatever stream torch has current"""
    from auromat_amd.pipeline import SequencePipeline
    key = _key('seq', env.ctx)
    if key not in _kept:
        _kept[key] = SequencePipeline(RW, RH, pxPerDeg=PX_PER_DEG, min_elevation=MIN_ELEV, own_image_buffers=False)
    seq = _kept[key]
    feed = [camera(False, k, RW, RH) + (env.inp['img%d' % k],) for k in range(R_FRAMES)]
    got = seq.process(feed, keep_on_device=True)
    at, shapes = 0, []
    for k in range(R_FRAMES):
        r = got[k]
        n = r['count'].numel()
        env.out['mean'][at:at + n].copy_(r['mean'].reshape(n, 4))
        env.out['count'][at:at + n].copy_(r['count'].reshape(n))
        at += n
        shapes.append(tuple(r['count'].shape))
    return dict(shapes=shapes)


def _run_grids(a):
    return [binned(camera_frame(k, RW, RH), a['img%d' % k]) for k in range(R_FRAMES)]


def _oracle_run(a):
    """what the arenas hold, frame after frame: mean | count, and rounded image | mask (without the arenas' alignment gaps)"""
    frames = _run_grids(a)
    return dict(grids=np.concatenate([np.concatenate([r['mean'].ravel(), r['count'].ravel()]) for r in frames]),
                images=np.concatenate([np.concatenate([r['img'].ravel().view(np.uint8), r['mask'].ravel()]) for r in frames]))


def _oracle_sequence(a):
    frames = _run_grids(a)
    return dict(mean=np.concatenate([r['mean'].reshape(-1, 4) for r in frames]))


def _images(n, width=W, height=H, first=20):
    return OrderedDict(('img%d' % k, (image(first + k, width, height), image(first + 10 + k, width, height))) for k in range(n))


PIXELS = 'the image is read for its values only (sums and means of the cells the camera model puts a pixel into)'
DIRS = 'the decoy directions are the unit vectors of the same camera turned by TURN: a ray is cast, its coordinates are binned ' \
       'by a bounded search of the axes and outliers are dropped; a direction is never used as an address'


def build():
    """Every case, in the order of the families."""
    index_range = {'index': (0, H * W, 'distinct')}
    cases = [
        # A
        Case('masks', 'A', pair('elev', 'lat', 'lon', 'img_mask'),
             [('centre', ((H, W), np.uint8)), ('corner', ((H + 1, W + 1), np.uint8)), ('n_valid', ((1,), np.int64)), ('red', ((8,), np.float64))],
             _call_masks, _oracle_masks, harmless='elevations, coordinates and mask bytes are compared and reduced, never used as an address'),
        Case('outline_links', 'A', pair('img_mask'), [('links', ((H * W * 4, 2), np.int64)), ('count', ((1,), np.uint64))],
             _call_outline, _oracle_outline, canonical={'links': _sorted_links},
             harmless='a mask byte decides whether a record is written; the capacity (4 per pixel) holds the records of any mask'),
        Case('pixel_polygons', 'A', OrderedDict(pair('lat', 'lon', 'img'), index=POLY_INDEX),
             [('verts', ((N_POLY, 4, 2), np.float64)), ('u8', ((N_POLY, 3), np.uint8)), ('f64', ((N_POLY, 3), np.float64))],
             _call_polygons, _oracle_polygons, index_ranges=index_range,
             harmless='`index` is the only input used as an address: the true one and the decoy are both lists of distinct pixel '
                      'indices of this frame (checked)'),
        Case('rotate_to_latlon', 'A', OrderedDict(xyz=XYZ), [('lat', ((N_PTS,), np.float64)), ('lon', ((N_PTS,), np.float64))],
             _call_rotate, _oracle_rotate, harmless='elementwise arithmetic on finite vectors'),
        Case('project', 'A', OrderedDict(lat=(LATLON[0][0], LATLON[1][0]), lon=(LATLON[0][1], LATLON[1][1]),
                                         px=(PLANE[0][0], PLANE[1][0]), py=(PLANE[0][1], PLANE[1][1])),
             [(k, ((N_PTS,), np.float64)) for k in ('x', 'y', 'ilat', 'ilon')], _call_project, _oracle_project,
             harmless='elementwise arithmetic on finite numbers'),
        Case('points_in_polygon', 'A', OrderedDict(px=(POLY_PTS[0][0], POLY_PTS[1][0]), py=(POLY_PTS[0][1], POLY_PTS[1][1]),
                                                   polygon=POLYGON), [('inside', ((N_PTS,), np.uint8))],
             _call_in_polygon, _oracle_in_polygon,
             harmless='the vertex count is a host argument (8 for both polygons); points and vertices are compared, never used as an address'),
        Case('hist2d', 'A', OrderedDict((k, (HIST[0][k], HIST[1][k])) for k in ('x', 'y', 'w')),
             [('mean', ((NY, NX, 1), np.float64)), ('count', ((NX * NY,), np.float64))], _call_hist, _oracle_hist, harmless=FIELD),
        Case('world_to_pixel', 'A', OrderedDict((k, (_w2p_points()[0][k], _w2p_points()[1][k])) for k in ('c0', 'c1', 'glat', 'glon')),
             [('xy', ((N_PTS, 2), np.float64)), ('elev', ((N_PTS,), np.float64)), ('flags', ((N_PTS,), np.uint8)),
              ('gxy32', ((G_NY, G_NX, 2), np.float32)), ('gxy', ((G_NY, G_NX, 2), np.float64)), ('gelev', ((G_NY, G_NX), np.float64)),
              ('gflags', ((G_NY, G_NX), np.uint8))], _call_w2p, _oracle_w2p, harmless='elementwise arithmetic on finite angles'),
        Case('directions_zenithal', 'A', OrderedDict(), [('dirs', (_zen_shape(), np.float64))], _call_zenithal, None,
             harmless='no device input: the header is a host block'),
        Case('lens_remap', 'A', OrderedDict(pair('img'), coords=(_lens_coords(LENS_K[0]).astype(np.float32),
                                                                  _lens_coords(LENS_K[1]).astype(np.float32))),
             [(k, ((H, W, 3), np.uint16)) for k in ('staged', 'gathered', 'c_staged', 'c_gathered')] +
             [('support', ((H, W), np.uint8)), ('c_support', ((H, W), np.uint8))], _call_lens, _oracle_lens,
             harmless='the coordinate array decides which taps are read: both arrays are the forward coordinates of a lens model '
                      'on this frame, and a tap outside the image counts 0 by the kernel\'s own test (include/auromat_hip.h: "Taps '
                      'outside the image count 0"); pixel values are only weighted'),
        # B
        Case('mosaic', 'B', _mosaic_inputs(), MOSAIC_OUT, _call_mosaic('amt_mosaic_frames', False), _oracle_mosaic,
             harmless=FIELD + '; the member table holds pointers and sizes from the host, the same for true and decoy arrays'),
        Case('mosaic_median', 'B', _mosaic_inputs(), MOSAIC_OUT, _call_mosaic('amt_mosaic_median_frames', True), None,
             synchronises=True, harmless=FIELD + '; the member table holds pointers and sizes from the host'),
        Case('mosaic_area', 'B', _mosaic_inputs(), MOSAIC_OUT, _call_mosaic('amt_area_mosaic_frames', True), _oracle_mosaic_area,
             synchronises=True, harmless=FIELD + '; the member table holds pointers and sizes from the host'),
        Case('scanline', 'B', _scanline_inputs(),
             [('planes', ((NY, S_NX, 4), np.float64)), ('img', ((NY, S_NX, 3), np.uint16)), ('mask', ((NY, S_NX), np.uint8)),
              ('frame_index', ((NY, S_NX), np.int32))], _call_scanline, _oracle_scanline, synchronises=True,
             harmless='polygons, masks, planes and pixels are compared or copied; the window and the vertex count are host arguments; '
                      'amt_scanline_pack refuses a count that is not the number of keep bytes and writes no record beyond it, the '
                      'record buffers hold a whole frame and start as zeros (cell 0, 0), amt_scanline_compose tests every record '
                      'against the raster'),
        Case('cubic', 'B', OrderedDict((k, (cubic_inputs()[0][k], cubic_inputs()[1][k])) for k in cubic_inputs()[0]),
             [('gradients', ((CUBIC_ROWS * CUBIC_ROWS, 2, 2), np.float64)), ('out', ((CUBIC_M, 2), np.float64))], _call_cubic,
             _oracle_cubic, synchronises=True,
             index_ranges={'indptr': (0, len(cubic_inputs()[0]['indices']) + 1), 'indices': (0, CUBIC_ROWS * CUBIC_ROWS),
                           'row_start': (0, CUBIC_ROWS * CUBIC_ROWS + 1), 'vertices': (-1, CUBIC_ROWS * CUBIC_ROWS)},
             harmless='the neighbour lists, the rows\' first points and the triangles\' vertices are used as indices: in the decoy as '
                      'in the true arrays every offset lies in its list and every vertex is a point of the set (checked; -1 is the '
                      'documented "outside the hull"); coordinates and values only enter the arithmetic'),
        # C
        Case('bin_frame', 'C', pair('lat_c', 'lon_c', 'elev', 'img'), GRID_OUT, _call_bin, _oracle_bin, harmless=FIELD),
        Case('median_frame', 'C', pair('lat_c', 'lon_c', 'elev', 'img'), GRID_OUT, _call_median, _oracle_median, synchronises=True,
             harmless=FIELD + '; the sorted keys are made from the cell found that way'),
        Case('median_frame_async', 'C', pair('lat_c', 'lon_c', 'elev', 'img'), GRID_OUT, _call_median_async, _oracle_median,
             harmless=FIELD + '; the sorted keys are made from the cell found that way'),
        Case('quantile_frame_async', 'C', pair('lat_c', 'lon_c', 'elev', 'img'), QUANT_OUT, _call_quantile_async, _oracle_quantile,
             harmless=FIELD),
        Case('area_frame', 'C', pair('lat', 'lon', 'lat_c', 'elev', 'img'), AREA_OUT, _call_area, _oracle_area, harmless=FIELD),
        Case('area_frame_async', 'C', pair('lat', 'lon', 'lat_c', 'elev', 'img'), AREA_OUT, _call_area_async, _oracle_area, harmless=FIELD),
        Case('nearest', 'C', OrderedDict(pair('lat_c', 'lon_c', 'elev', 'img'), target_mask=TARGET_MASK), NEAREST_OUT, _call_nearest, _oracle_nearest,
             out_fill={'index': np.zeros((NY, NX), dtype=np.int64)},
             harmless=FIELD + '; amt_nearest_gather reads `index`, which amt_nearest_frame writes: pixel indices of this frame or -1 '
                              'whatever coordinates it read, and zeros (pixel 0) before it has run'),
    ]
    cases += [
        # D
        Case('georef_frame', 'D', _images(1), OrderedDict(GEO_OUT, bbox=((8,), np.float64), acc=((5 * GEOREF_CELLS,), np.uint64)),
             _call_georef_frame, _oracle_georef_frame, harmless=PIXELS),
        Case('georef_frame_dirs', 'D', OrderedDict(dirs=(directions(False), directions(True))), OrderedDict(GEO_OUT, box=((8,), np.float64)),
             _call_georef_frame_dirs, _oracle_dirs(False), harmless=DIRS),
        Case('georef_frame_dirs_64x17', 'D', OrderedDict(dirs=(directions(False, SW, SH), directions(True, SW, SH))),
             OrderedDict([(k, ((SH + 1, SW + 1) if k in ('lat', 'lon') else (SH, SW), np.float64)) for k in GEO] + [('box', ((8,), np.float64))]),
             _call_georef_frame_dirs, _oracle_dirs(False, width=SW, height=SH), harmless=DIRS),
        Case('camera_path', 'D', _images(1), DRIVER_OUT, _call_camera_path, _oracle_camera(1), harmless=PIXELS),
        Case('camera_path_many', 'D', _images(N_MANY),
             OrderedDict((k + str(f), v) for f in range(N_MANY) for k, v in DRIVER_OUT.items()), _call_camera_many,
             _oracle_camera(N_MANY), harmless=PIXELS),
        Case('dirs_path', 'D', OrderedDict(_images(1), dirs=(directions(False), directions(True))), OrderedDict(GEO_OUT, **DRIVER_OUT),
             _call_dirs_path, _oracle_dirs(True), harmless=DIRS + '; ' + PIXELS),
        Case('pipeline_run_dirs', 'D', OrderedDict(_images(1), dirs=(directions(False), directions(True))), DRIVER_OUT,
             _call_pipeline_run, _oracle_dirs(True, coordinates=False), synchronises=True, harmless=DIRS + '; ' + PIXELS),
        # E
        Case('run_device_images', 'E', _images(R_FRAMES, RW, RH), RUN_OUT, _call_run_device, _oracle_run, harmless=PIXELS),
        Case('run_host_images', 'E', OrderedDict(), RUN_OUT, _call_run_host, None,
             harmless='no device input: the images lie in page-locked host memory and are settled'),
        Case('sequence_pipeline', 'E', _images(R_FRAMES, RW, RH),
             [('mean', ((R_CELLS, 4), np.float64)), ('count', ((R_CELLS,), np.float64))], _call_sequence_pipeline, _oracle_sequence,
             synchronises=True, harmless=PIXELS),
    ]
    return cases


GEOREF_CELLS = 27 * 43                                                   # amt_grid_layout at 2 px/deg of 44..58 N, 108..86 W (asserted in the call)
# cases without a CPU oracle of their own (at most 3): the median mosaic has none that takes plain arrays (tests/
# _mosaic_quantile_oracle.py works on the case objects of tests/_mosaic_quantile_cases.py); the runner on host images has no
# device input, hence no decoy, and neither has amt_directions_zenithal
# outputs that no key of the case's oracle stands for, by name: they do not depend on a gated input of the case (the coordinate
# arrays and the box of a camera frame follow from the host's parameter block, the support bytes of amt_lens_remap from the lens
# model), so no decoy could change them; the GPU test still compares them with the baseline
# — nor do the counts and the mask of a camera frame's grid, which the camera model decides, whatever the image —
UNCOVERED = {'lens_remap': ('support',), 'georef_frame': ('bbox',) + GEO, 'run_device_images': ('slots',),
             'camera_path': ('mask', 'count'), 'camera_path_many': tuple(k + str(f) for f in range(3) for k in ('mask', 'count')),
             'sequence_pipeline': ('count',)}
EXEMPT = ('directions_zenithal', 'mosaic_median', 'run_host_images')
