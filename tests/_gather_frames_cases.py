"""
TEST INFRASTRUCTURE — jobs for the gathered frames (amt_gather_frames, auromat_amd.resample.gather_frames, GatherSequence).

A job is one constructed camera (tests/_gather_mosaic_cases.py, tests/_inverse_cases.py) with a grid of its own, given by the
corners of its cells: the cell centres, and with a factor n the n x n sub-samples of every cell, are `axis(corners, n)` —
corner + step * (2 s + 1) / (2 n), what gather_subsample_coordinates lays out.  Axes-form jobs hand the two axes to the kernel;
point-form jobs (a pole camera) hand it the points of a grid laid out in coordinates whose pole lies on the equator, rotated back.
Every job states what it CLAIMS to hold — cells the camera sees, cells it does not see, nobody sees any, tile tails on either
axis — and tests/test_gather_frames_cpu.py checks the claims against the float64 inverse statement of tests/_inverse_oracle.py.

`run` (GPU) is the comparison of tests/test_gpu_gather_frames_cells.py: one amt_gather_frames call whose outputs lie back to back
in one poisoned arena, against one amt_gather_mosaic / amt_gather_mosaic_supersampled call per job on a table of that one member,
all bytes.
"""
import ctypes as C

import numpy as np

import _gather_mosaic_cases as GC
import _inverse_cases as IC
import _inverse_oracle as O

TILE = 32
MAX_JOBS = 64
POISON = 0xA5
ALIGN = 256
CODES = dict(linear=0, lanczos4=1, nearest=2)
FRAMES = dict(geodetic=O.GEODETIC, sm=O.SM)
PATH_STAGED, PATH_CELL = 1, 2


def axis(corners, n=1):
    """n positions per cell of an axis given by its cells' corners"""
    c = np.asarray(corners, dtype=np.float64)
    f = (2 * np.arange(n) + 1) / (2 * n)
    return (c[:-1, None] + (c[1:, None] - c[:-1, None]) * f[None, :]).reshape(-1)


def wrap180(lon):
    return (np.asarray(lon, dtype=np.float64) + 180.0) % 360.0 - 180.0


def rotate_back(r_lat, r_lon):
    """points of a grid whose equator point (0, 90) is the north pole -> (lat, lon) [deg], on the sphere"""
    la, lo = np.deg2rad(r_lat), np.deg2rad(r_lon)
    x, y, z = np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)
    # a quarter turn about x: y -> z, z -> -y
    return np.rad2deg(np.arcsin(np.clip(y, -1.0, 1.0))), np.rad2deg(np.arctan2(-z, x))


def job(name, cam, lat0, lon0, ny, nx, step=0.1, frame='geodetic', points=False, min_elevation=None, masked_columns=None,
        claims=('seen', 'unseen')):
    """ny x nx cells of `step` degrees whose first corner is (lat0, lon0)"""
    return dict(name=name, cam=cam, frame=frame, points=points, ny=ny, nx=nx, min_elevation=min_elevation,
                masked_columns=masked_columns, claims=tuple(claims),
                lat_corners=lat0 + step * np.arange(ny + 1), lon_corners=lon0 + step * np.arange(nx + 1))


def _centred(name, cam, at, ny, nx, step=0.1, **kw):
    return job(name, cam, at[0] - step * ny / 2.0, at[1] - step * nx / 2.0, ny, nx, step, **kw)


A_CENTRE = (58.25, 27.63)            # where gm-a's (and the zenithal cameras') central pixel looks: geodetic, and SM below
_JOBS = {}


def _make():
    if _JOBS:
        return _JOBS
    made = [
        _centred('one-cell', 'gm-a', A_CENTRE, 1, 1, claims=('seen', 'all-seen')),
        _centred('g33x31', 'gm-a', A_CENTRE, 33, 31, claims=('seen', 'all-seen', 'tail-y', 'tail-x')),
        _centred('g32x64', 'gm-a', A_CENTRE, 32, 64, claims=('seen', 'all-seen')),
        job('gm-a', 'gm-a', 52.0, 18.0, 95, 155, claims=('seen', 'unseen', 'tail-y', 'tail-x', 'unseen-tile')),
        job('gm-wide', 'gm-wide', 51.0, 16.5, 105, 195, min_elevation=5.0, claims=('seen', 'unseen', 'tail-y', 'tail-x')),
        job('unseen', 'gm-a', 10.0, -60.0, 21, 40, claims=('nobody', 'tail-y', 'tail-x')),
        job('gm-a-masked', 'gm-a', 52.0, 18.0, 95, 155, min_elevation=10.0, masked_columns=(12, 52),
            claims=('seen', 'unseen', 'tail-y', 'tail-x')),
        # the pole camera looks at 89.97 N: a grid of 0.005 deg cells around the rotated frame's (0, 90)
        job('pole-points', 'pole', -0.12, 89.85, 50, 60, step=0.005, points=True, claims=('seen', 'unseen', 'tail-y', 'tail-x')),
        # the date line runs through the frame: longitudes 179.88 ... 180.08 wrap to -179.92
        job('dateline', 'dateline', 19.93, 179.88, 28, 40, step=0.005, claims=('seen', 'unseen', 'tail-x', 'wraps')),
        job('sip-3', 'sip-3', 55.0, 22.0, 50, 90, claims=('seen', 'unseen', 'tail-y', 'tail-x')),
        job('zen-ARC', 'zen-ARC', 56.0, 24.0, 40, 70, claims=('seen', 'tail-y', 'tail-x')),
    ]
    for j in made:
        _JOBS[j['name']] = j
    # the SM frame: where the central pixels of gm-a and gm-b look in (MLat, SM longitude)
    for name, cam in (('sm-a', 'gm-a'), ('sm-b', 'gm-b')):
        c = GC.by_name(cam)
        f = O.forward_mp(c, (c['width'] - 1) / 2.0, (c['height'] - 1) / 2.0)
        at = (round(f['mlat'], 1), round(f['smlon'], 1))
        _JOBS[name] = _centred(name, cam, at, 70, 110, frame='sm', claims=('seen', 'unseen', 'tail-y', 'tail-x'))
    return _JOBS


def by_name(name):
    return _make()[name]


def names():
    return list(_make())


def small(k):
    """the k-th of the 64 one-tile jobs: 1 + k % 32 rows and 32 - k % 32 columns inside gm-a's footprint (gm-b's for odd k)"""
    ny, nx = 1 + k % TILE, TILE - k % TILE
    return job('small-%d' % k, 'gm-b' if k % 2 else 'gm-a', 56.5 + 0.01 * k, 25.0 + 0.02 * k, ny, nx, claims=('seen', 'all-seen'))


# the batches of tests/test_gpu_gather_frames_cells.py
ONE = ['gm-a']
FIVE = ['one-cell', 'g33x31', 'g32x64', 'gm-a', 'gm-wide']
FIVE_OTHER_ORDER = ['gm-wide', 'g32x64', 'one-cell', 'gm-a', 'g33x31']
UNSEEN_BETWEEN = ['g33x31', 'unseen', 'g32x64']
MASKED_AND_NOT = ['gm-a-masked', 'gm-a']
FORMS = ['g33x31', 'pole-points', 'dateline', 'g32x64']
SM = ['sm-a', 'sm-b']
ZENITHAL = ['g33x31', 'sip-3', 'zen-ARC', 'gm-a']
TYPES = ['g33x31', 'gm-a', 'unseen']
SUPERSAMPLED = ['one-cell', 'g33x31', 'unseen', 'gm-a', 'pole-points']
BATCHES = dict(ONE=ONE, FIVE=FIVE, FIVE_OTHER_ORDER=FIVE_OTHER_ORDER, UNSEEN_BETWEEN=UNSEEN_BETWEEN, MASKED_AND_NOT=MASKED_AND_NOT,
               FORMS=FORMS, SM=SM, ZENITHAL=ZENITHAL, TYPES=TYPES, SUPERSAMPLED=SUPERSAMPLED)


def resolve(j):
    return by_name(j) if isinstance(j, str) else j


def camera(j):
    return GC.by_name(resolve(j)['cam'])


def coordinates(j, n=1):
    """(a, b, points): the two axes of the job's n x n sub-samples (the cell centres for n = 1), or its two point arrays"""
    j = resolve(j)
    la, lo = axis(j['lat_corners'], n), axis(j['lon_corners'], n)
    if j['points']:
        a, b = rotate_back(*np.meshgrid(la, lo, indexing='ij'))
        return np.ascontiguousarray(a), np.ascontiguousarray(b), True
    return la, wrap180(lo), False


def center_mask(j):
    """the job's centre mask (height x width uint8) or None"""
    j = resolve(j)
    if j['masked_columns'] is None:
        return None
    c = camera(j)
    cm = np.zeros((c['height'], c['width']), dtype=np.uint8)
    cm[:, j['masked_columns'][0]:j['masked_columns'][1]] = 1
    return cm


def tiles(j, n=1):
    """(tiles down, tiles across) of a job with factor n"""
    j = resolve(j)
    T = TILE // n
    return (j['ny'] + T - 1) // T, (j['nx'] + T - 1) // T


def seen_points(j, n=1):
    """which of the job's points the camera sees by resampleGather's four rules (the support rule of 'linear' and 'lanczos4'),
    in the float64 statement of tests/_inverse_oracle.py: (ny n, nx n) bool"""
    j = resolve(j)
    c = camera(j)
    a, b, points = coordinates(j, n)
    la, lo = (a, b) if points else np.meshgrid(a, b, indexing='ij')
    r = O.inverse_arrays(O.F64, c, FRAMES[j['frame']], la, lo)
    w, h = c['width'], c['height']
    with np.errstate(invalid='ignore'):
        xs, ys = r['x'].astype(np.float32).astype(np.float64), r['y'].astype(np.float32).astype(np.float64)
        seen = (r['flags'] == 0) & (xs >= 0) & (xs <= w - 1) & (ys >= 0) & (ys <= h - 1) & ~np.isnan(r['elev'])
        cm = center_mask(j)
        if cm is not None:
            ix = np.clip(np.nan_to_num(np.rint(r['x']), nan=0.0, posinf=0.0, neginf=0.0), 0, w - 1).astype(np.int64)
            iy = np.clip(np.nan_to_num(np.rint(r['y']), nan=0.0, posinf=0.0, neginf=0.0), 0, h - 1).astype(np.int64)
            seen &= cm[iy, ix] == 0
        if j['min_elevation'] is not None:
            seen &= r['elev'] >= j['min_elevation']
    return seen


def check_claims(j):
    """AssertionError unless the job holds what it claims"""
    j = resolve(j)
    seen = seen_points(j)
    ny, nx, claims = j['ny'], j['nx'], j['claims']
    assert seen.shape == (ny, nx), j['name']
    known = {'seen', 'unseen', 'all-seen', 'nobody', 'tail-y', 'tail-x', 'unseen-tile', 'wraps'}
    assert set(claims) <= known, (j['name'], set(claims) - known)
    if 'seen' in claims:
        assert seen.any(), j['name']
    if 'unseen' in claims:
        assert seen.any() and not seen.all(), j['name']
    if 'all-seen' in claims:
        assert seen.all(), j['name']
    if 'nobody' in claims:
        assert not seen.any(), j['name']
    if 'tail-y' in claims:
        assert ny % TILE, j['name']
    if 'tail-x' in claims:
        assert nx % TILE, j['name']
    if 'unseen-tile' in claims:
        assert any(not seen[i:i + TILE, k:k + TILE].any() for i in range(0, ny, TILE) for k in range(0, nx, TILE)), j['name']
    if 'wraps' in claims:
        lon = coordinates(j)[1]
        assert (np.diff(lon) < 0).sum() == 1 and seen[:, lon > 0].any() and seen[:, lon < 0].any(), j['name']
    return seen


# ---- the device side -----------------------------------------------------------------------------------------------------

def image(j, dtype=np.uint8, channels=3, seed=None):
    j = resolve(j)
    # (by the camera: two jobs of one camera sample the same image)
    return GC.image(camera(j), dtype, channels, seed=sum(map(ord, j['cam'])) % 997 if seed is None else seed)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).cuda()


class Inputs(object):
    """the device inputs of a list of jobs: per job the member (camera model, image, centre mask, threshold) and coordinates"""

    def __init__(self, jobs, dtype=np.uint8, channels=3, n=1):
        from auromat_amd._native import GatherMember
        self.jobs = [resolve(j) for j in jobs]
        self.dtype, self.channels, self.n = np.dtype(dtype), channels, n
        self.keep, self.members, self.coords = [], [], []
        for j in self.jobs:
            params, zen = IC.native(camera(j))
            img, cm = _dev(image(j, dtype, channels)), center_mask(j)
            cm = None if cm is None else _dev(cm)
            m = GatherMember()
            C.memmove(C.byref(m.params), C.byref(params), C.sizeof(params))
            if zen is not None:
                m.zenithal = C.pointer(zen)
            m.img = img.data_ptr()
            m.center_mask = None if cm is None else cm.data_ptr()
            m.min_elevation = float('nan') if j['min_elevation'] is None else float(j['min_elevation'])
            a, b, points = coordinates(j, n)
            a, b = _dev(a), _dev(b)
            self.keep.append((params, zen, img, cm, a, b))
            self.members.append(m)
            self.coords.append((a.data_ptr(), b.data_ptr(), points))


def layout(jobs, itemsize, channels, n):
    """offsets of every job's (img, mask, elev, count) in the arena, 256-byte aligned and back to back, and the arena's size
    (count only with n > 1)"""
    at, out = 0, []
    for j in jobs:
        cells = j['ny'] * j['nx']
        o = {}
        for key, size in (('img', cells * channels * itemsize), ('mask', cells), ('elev', cells * 8)) + \
                ((('count', cells),) if n > 1 else ()):
            o[key] = (at, size)
            at = (at + size + ALIGN - 1) // ALIGN * ALIGN
        out.append(o)
    return out, at + ALIGN


def frames_call(ctx, inp, arena, frame='geodetic', interpolation='linear', min_count=1, force_path=0, tile_path=None, n_jobs=None,
                edit=None):
    """amt_gather_frames on the inputs with the outputs laid out in `arena` (a uint8 tensor): (status, error text)"""
    from auromat_amd._native import GatherDebug, GatherJob
    offsets, size = layout(inp.jobs, inp.dtype.itemsize, inp.channels, inp.n)
    assert arena.numel() >= size
    table = (GatherJob * max(len(inp.jobs), 1))()
    base = arena.data_ptr()
    for t, j, m, (pa, pb, points), o in zip(table, inp.jobs, inp.members, inp.coords, offsets):
        C.memmove(C.byref(t.member), C.byref(m), C.sizeof(m))
        t.ny, t.nx = j['ny'], j['nx']
        if points:
            t.cell_lat, t.cell_lon = pa, pb
        else:
            t.lat, t.lon = pa, pb
        t.out_img, t.out_mask, t.out_elev = base + o['img'][0], base + o['mask'][0], base + o['elev'][0]
        if inp.n > 1:
            t.out_count = base + o['count'][0]
    dbg = None
    if force_path or tile_path is not None:
        dbg = GatherDebug()
        dbg.force_path = force_path
        dbg.tile_path = None if tile_path is None else tile_path.data_ptr()
    args = dict(jobs=table, n_jobs=len(inp.jobs) if n_jobs is None else n_jobs, frame=FRAMES[frame], factor=inp.n,
                min_count=min_count, bytes=inp.dtype.itemsize, channels=inp.channels, interpolation=CODES[interpolation],
                debug=None if dbg is None else C.byref(dbg))
    if edit is not None:
        edit(args, table)
    rc = ctx._lib.amt_gather_frames(ctx.handle, args['jobs'], args['n_jobs'], args['frame'], args['factor'], args['min_count'],
                                    args['bytes'], args['channels'], args['interpolation'], args['debug'])
    return rc, (ctx._lib.amt_last_error(ctx.handle) or b'').decode()


def per_job_call(ctx, inp, k, frame='geodetic', interpolation='linear', min_count=1, force_path=0, tile_path=True):
    """job k alone through amt_gather_mosaic (n = 1) or amt_gather_mosaic_supersampled on a table of its one member: the bytes
    of img, mask, elev (and count), and tile_path"""
    import torch
    from auromat_amd._native import GatherDebug
    j, n = inp.jobs[k], inp.n
    cells = j['ny'] * j['nx']
    out = dict(img=torch.full((cells * inp.channels * inp.dtype.itemsize,), POISON, dtype=torch.uint8, device='cuda'),
               mask=torch.full((cells,), POISON, dtype=torch.uint8, device='cuda'),
               elev=torch.full((cells * 8,), POISON, dtype=torch.uint8, device='cuda'),
               source=torch.full((cells * 4,), POISON, dtype=torch.uint8, device='cuda'),
               count=torch.full((cells,), POISON, dtype=torch.uint8, device='cuda'))
    ty, tx = tiles(j, n)
    dbg = GatherDebug()
    dbg.force_path = force_path
    tp = torch.full((ty * tx,), POISON, dtype=torch.uint8, device='cuda')
    if tile_path:
        dbg.tile_path = tp.data_ptr()
    pa, pb, points = inp.coords[k]
    table = (type(inp.members[k]) * 1)()
    C.memmove(C.byref(table[0]), C.byref(inp.members[k]), C.sizeof(inp.members[k]))
    axes, cell = ((None, None), (pa, pb)) if points else ((pa, pb), (None, None))
    p = {key: v.data_ptr() for key, v in out.items()}
    if n == 1:
        ctx.call('amt_gather_mosaic', table, 1, FRAMES[frame], axes[0], j['ny'], axes[1], j['nx'], cell[0], cell[1], inp.dtype.itemsize,
                 inp.channels, CODES[interpolation], 1, p['img'], p['mask'], p['elev'], p['source'], None, C.byref(dbg))
    else:
        ctx.call('amt_gather_mosaic_supersampled', table, 1, FRAMES[frame], axes[0], j['ny'], axes[1], j['nx'], cell[0], cell[1], n,
                 min_count, inp.dtype.itemsize, inp.channels, CODES[interpolation], 1, p['img'], p['mask'], p['elev'], p['source'],
                 p['count'], C.byref(dbg))
    res = {key: out[key].cpu().numpy() for key in ('img', 'mask', 'elev') + (('count',) if n > 1 else ())}
    res['tile_path'] = tp.cpu().numpy()
    return res


def run(jobs, dtype=np.uint8, channels=3, interpolation='linear', frame='geodetic', n=1, min_count=1, force_path=0, want=None):
    """One amt_gather_frames call against the per-job calls, all bytes of the arena.  Returns dict(jobs: per job the bytes and
    typed views, tile_path: per job, want: the per-job results — hand them back in as `want` to compare another run with them)"""
    import torch
    from auromat_amd._native import Context
    ctx = Context.current()
    inp = Inputs(jobs, dtype, channels, n)
    offsets, size = layout(inp.jobs, inp.dtype.itemsize, channels, n)
    arena = torch.full((size,), POISON, dtype=torch.uint8, device='cuda')
    ntiles = [int(np.prod(tiles(j, n))) for j in inp.jobs]
    tile_path = torch.full((sum(ntiles) + ALIGN,), POISON, dtype=torch.uint8, device='cuda')
    rc, err = frames_call(ctx, inp, arena, frame, interpolation, min_count, force_path, tile_path)
    assert rc == 0, err
    ctx.synchronize()
    got, tp = arena.cpu().numpy(), tile_path.cpu().numpy()
    if want is None:
        want = [per_job_call(ctx, inp, k, frame, interpolation, min_count, 0) for k in range(len(inp.jobs))]
    what = ([j['name'] for j in inp.jobs], inp.dtype, channels, interpolation, frame, n, min_count, force_path)
    untouched = np.ones(size, dtype=bool)
    results, t0 = [], 0
    for k, (j, o, w, nt) in enumerate(zip(inp.jobs, offsets, want, ntiles)):
        r = {}
        for key, (at, nbytes) in o.items():
            r[key] = got[at:at + nbytes]
            untouched[at:at + nbytes] = False
            assert np.array_equal(r[key], w[key]), (what, k, j['name'], key, int((r[key] != w[key]).sum()))
        r['tile_path'] = tp[t0:t0 + nt]
        if not force_path:
            assert np.array_equal(r['tile_path'], w['tile_path']), (what, k, j['name'], 'tile_path')
        else:
            assert not (r['tile_path'] == PATH_STAGED).any() and np.array_equal(r['tile_path'] == 0, w['tile_path'] == 0), (what, k)
        t0 += nt
        ny, nx = j['ny'], j['nx']
        r['mask2'] = r['mask'].reshape(ny, nx)
        r['elev2'] = r['elev'].view(np.float64).reshape(ny, nx)
        r['img2'] = r['img'].view(inp.dtype).reshape(ny, nx, channels)
        results.append(r)
    # the bytes between and after the outputs, and behind the last job's tiles, are the poison still
    assert (got[untouched] == POISON).all(), (what, 'bytes outside the outputs were written')
    assert (tp[t0:] == POISON).all(), (what, 'tile_path past the last job')
    del inp
    return dict(jobs=results, want=want)
