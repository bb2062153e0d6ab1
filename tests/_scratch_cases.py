"""
TEST INFRASTRUCTURE — the users of the library's scratch memory (amt_workspace, auromat_amd/csrc/amt_common.h): which call site
is reached by which case, the cases the gated side stream (tests/_gated_cases.py, tests/_gated_gather_frames_cases.py) does not
have, and for every call site that can need more than the buffer's 1 MiB minimum a second, larger shape of the same call.
Host arrays only; the `call` of a case touches the GPU, nothing else here does (tests/test_scratch_cases_cpu.py checks the
registry and the added cases without one, tests/test_gpu_scratch_state.py runs them).

The audit ("Scratch memory: who writes what before it is read", has the full table): what every call site lays out
in the buffer and the stream-ordered write that comes before the first read.  Nothing is read that the same call has not written.

  amt_bbox_corners          partials [blocks][8]                 k_bbox_corners: block_reduce8 of every block
  amt_mosaic_run            member, tile and CSR tables          one hipMemcpyAsync of the packer's staging buffer (gaps zeroed)
                            accumulators                         hipMemsetAsync; tail: the caller's (below)
  median_front              count, cursor, tier counters         one hipMemsetAsync; offset, block sums: cell_scan; medium / large
                                                                 lists: k_med_small up to the counters; cell_of: the count pass,
                                                                 every pixel; keys: the fill pass, every counted position; states:
                                                                 k_med_large_init / the first digit of k_med_large_step;
                                                                 histograms and tickets: k_med_small as it lists a large cell
  mosaic_median_front       source / first-member plane          k_mosaic_select (rule 1) / hipMemsetAsync 0x7f (rule 0, read only
                                                                 with out_source); tables: one copy; then as median_front
  amt_area_frame_finalize   overflow word                        hipMemsetAsync
  amt_area_frame_async      accumulators and the flag            one hipMemsetAsync
  amt_area_mosaic_frames    tables | flag and accumulators       one copy | one hipMemsetAsync
  amt_scanline_pack         cursor                               hipMemsetAsync
  amt_scanline_compose      strip table | outside flag           hipMemcpyAsync | hipMemsetAsync
  gather_prepare            member table                         hipMemcpyAsync
  amt_gather_frames         tile prefix and job table            one hipMemcpyAsync (the gap between them is zeroed on the host)
  prepare_georef            partials [items][8], fold [64][8]    k_georef_rows: every item, its sky items too; first fold launch
  coarse_bbox               partials [blocks][8]                 k_coarse_bbox: block_reduce8 of every block
  amt_nearest_frame         count, cursor                        hipMemsetAsync; offset, block sums: cell_scan; cell_of: k_nn_count,
                                                                 every pixel; order: k_nn_fill, every counted position
  amt_cubic_gradients_csr   second gradient buffer               k_fill_u64 before every sweep; err and tickets: hipMemsetAsync per
                                                                 sweep; active: hipMemcpyAsync; records: k_cubic_geometry, every point
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

import _gated_cases as K
from _gated_stream import Case

MIN_BYTES = 1 << 20                              # the floor of a buffer (amt_workspace)
MAX_STREAMS = 16                                 # kMaxWorkspaces
HOOK = ('amt_debug_scratch_info', 'amt_debug_scratch_fill', 'amt_debug_scratch_release')
HOOK_SITE = ('amt_context.hip', 'amt_debug_scratch_fill')        # the hook's own request for the buffer: not a user

# call site (file, enclosing function) -> the cases that reach it ON THE STREAM OF THE CALL; the first one is the case the poison
# test names as the site's minimum
SITES = OrderedDict([
    (('amt_masks.hip', 'amt_bbox_corners'), ('masks',)),
    (('amt_mosaic.hip', 'amt_mosaic_run'), ('mosaic', 'mosaic_median')),
    (('amt_median.hip', 'median_front'), ('median_frame_async', 'median_frame', 'quantile_frame_async')),
    (('amt_median.hip', 'mosaic_median_front'), ('mosaic_median_union',)),          # (rule 0; rule 1 asks through amt_mosaic_run)
    (('amt_area.hip', 'amt_area_frame_finalize'), ('area_finalize', 'area_frame')),
    (('amt_area.hip', 'amt_area_frame_async'), ('area_frame_async',)),
    (('amt_area.hip', 'amt_area_mosaic_frames'), ('mosaic_area',)),
    (('amt_scanline.hip', 'amt_scanline_pack'), ('scanline_pack', 'scanline')),
    (('amt_scanline.hip', 'amt_scanline_compose'), ('scanline_compose', 'scanline')),
    (('amt_gather.hip', 'gather_prepare'), ('gather_pair', 'gather_pair_supersampled')),
    (('amt_gather.hip', 'amt_gather_frames'), ('gather_frames_x1', 'gather_frames_x3')),
    (('amt_georef.hip', 'prepare_georef'), ('georef_frame', 'georef_frame_dirs', 'georef_frame_dirs_64x17')),
    (('amt_georef.hip', 'coarse_bbox'), ('coarse_bbox_dirs',)),
    (('amt_nearest.hip', 'amt_nearest_frame'), ('nearest',)),
    (('amt_nearest.hip', 'amt_cubic_gradients_csr'), ('cubic',)),
])
USERS = tuple(OrderedDict.fromkeys(n for names in SITES.values() for n in names))
MINIMUM = tuple(names[0] for names in SITES.values())
# The frame driver's pre-pass (amt_pipe_coarse[_dirs]) reaches coarse_bbox as well, but on the driver's OWN pre-pass stream, whose
# buffer the hook (current stream only) cannot reach: cases of the families D and E may count as users at run time without
# being listed above.  Their buffers are the pipelines' own business (out of scope, tests/test_gpu_scratch_state.py).
DRIVER_FAMILIES = ('D', 'E')
# call sites that can never ask for more than the 1 MiB floor, and why
NO_LARGE = {
    ('amt_masks.hip', 'amt_bbox_corners'): 'grid_for() stops at 4096 workgroups: 4096 x 64 bytes = 256 KiB',
    ('amt_area.hip', 'amt_area_frame_finalize'): 'one word',
    ('amt_scanline.hip', 'amt_scanline_pack'): '256 bytes',
    ('amt_gather.hip', 'amt_gather_frames'): 'AMT_GATHER_MAX_JOBS = 64 jobs of a few hundred bytes',
}

_ptr = K._ptr
GRID_OUT = lambda ny, nx: OrderedDict([('mean', ((ny, nx, 4), np.float64)), ('img', ((ny, nx, 3), np.uint16)),
                                       ('mask', ((ny, nx), np.uint8)), ('count', ((ny, nx), np.float64))])


def _axes(ctx, xedges, yedges):
    from auromat_amd.util.histogram import make_axis
    xa, _ = make_axis(ctx, xedges, uniform=True)
    ya, _ = make_axis(ctx, yedges, uniform=True)
    assert xa.uniform == 1 and ya.uniform == 1
    return xa, ya


def scene(seed, h, w, lat0=40.0, lon0=10.0, span_lat=8.25, span_lon=15.875):
    """K.scene at any size: a frame of h x w pixels whose corners span span_lat x span_lon degrees from (lat0, lon0)"""
    rng = np.random.RandomState(seed)
    dlat, dlon = span_lat / h, span_lon / w
    i, j = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    lat = K._q(lat0 + dlat * i + rng.uniform(-0.2 * dlat, 0.2 * dlat, i.shape), 1 / 1024.0)
    lon = K._q(lon0 + dlon * j + rng.uniform(-0.2 * dlon, 0.2 * dlon, i.shape), 1 / 1024.0)
    mean4 = lambda v: 0.25 * (v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:])
    return dict(lat=lat, lon=lon, lat_c=K._q(mean4(lat), 1 / 1024.0), lon_c=K._q(mean4(lon), 1 / 1024.0),
                elev=K._q(rng.uniform(0.0, 80.0, (h, w)), 1 / 64.0), img=rng.randint(0, 65535, (h, w, 3)).astype(np.uint16))


# ---- the cases the gated side stream does not have -----------------------------------------------------------------------------

def _mosaic_table(env, struct, corners, windows, h, w):
    table = (struct * 2)()
    for m, (pre, win) in enumerate(zip('ab', windows)):
        i = lambda k: env.inp[pre + '_' + k].data_ptr()
        if corners:
            table[m].lat, table[m].lon = i('lat'), i('lon')
        else:
            table[m].lon_c = i('lon_c')
        table[m].lat_c, table[m].elev, table[m].img, table[m].center_mask = i('lat_c'), i('elev'), i('img'), None
        table[m].height, table[m].width = h, w
        table[m].win_x0, table[m].win_y0, table[m].win_nx, table[m].win_ny = win
    return table


def _call_mosaic(name, rule, windows, h, w, xedges, yedges, synchronises):
    def call(env):
        from auromat_amd._native import AreaMosaicMember, MosaicMember
        o = env.out
        xa, ya = _axes(env.ctx, xedges, yedges)
        area = name == 'amt_area_mosaic_frames'
        table = _mosaic_table(env, AreaMosaicMember if area else MosaicMember, area, windows, h, w)
        env.ctx.call(name, table, 2, 2, 3, K.MIN_ELEV, C.byref(xa), C.byref(ya), 0, rule,
                     *(([C.c_uint64(K.HALF)] if area else []) + K._grid_ptrs(o) + [_ptr(o['source'])]))
        K._kept.setdefault(K._key('tables', env.ctx), []).append(table)
        if not synchronises:
            env.closed(name)
    return call


class _Mosaic(object):
    def __init__(self, members):
        self.members, self.windows, self.shape = members, K.WINDOWS, (K.NY, K.NX)


def _oracle_mosaic_median_union(a):
    import _mosaic_quantile_oracle as MQ
    r = MQ.expected(_Mosaic(K._member_cases(a)), 0)
    return dict(mean=r['stat'][0], img=r['img'][0], mask=r['mask'], count=r['count'], source=r['source'])


def _accumulators():
    """(true, decoy): what amt_area_frame leaves for the two scenes of tests/_gated_cases.py, by tests/_area_oracle.py"""
    if 'area_acc' not in K._kept:
        import _area_oracle as A
        K._kept['area_acc'] = tuple(np.ascontiguousarray(A.accumulate(K._AreaCase(s))[0].reshape(5, K.NX * K.NY)) for s in (K.TRUE, K.DECOY))
    return K._kept['area_acc']


def _call_area_finalize(env):
    env.ctx.call('amt_area_frame_finalize', _ptr(env.inp['acc']), K.NX, K.NY, 3, 2, C.c_uint64(K.HALF), *K._grid_ptrs(env.out))   # synchronises


def _oracle_area_finalize(a):
    import _area_oracle as A
    r = A.finalize(a['acc'].reshape(5, K.NX, K.NY), np.uint16, 0.5)
    assert not r['over']
    return dict(mean=r['area'], img=r['img'], mask=r['mask'], count=r['coverage'])


WINDOW = (0, 0, K.NY, K.NX)


def _keeps():
    """per strip (true, decoy) keep arrays of amt_scanline_select, by tests/_scanline_oracle.py; the decoy is the true one upside
    down: amt_scanline_pack checks its `count` argument against the keep bytes set, and that is a host argument"""
    if 'keeps' not in K._kept:
        import _scanline_oracle as SO
        out = []
        for s in range(2):
            keep, _ = SO.select(K.S_LAT, K.S_LON, K.STRIPS[s][0]['polygon'], K.STRIPS[s][0]['cell_mask'], WINDOW)
            out.append((keep, np.ascontiguousarray(np.flipud(keep))))
        K._kept['keeps'] = out
    return K._kept['keeps']


REC_BYTES = 4 + 4 + 4 * 8 + 3 * 2                # row, col, four planes, three uint16 channels


def _record_bytes(rec):
    return np.concatenate([np.ascontiguousarray(rec[k]).view(np.uint8).reshape(-1) for k in ('row', 'col', 'planes', 'img')])


def sorted_records(b):
    """the bytes of one output that holds the record arrays of amt_scanline_pack back to back (row | col | planes | img), with
    the records in the order of (row, col): the kernel hands out places in no particular order"""
    n = b.size // REC_BYTES
    row, col = b[:4 * n].view(np.int32), b[4 * n:8 * n].view(np.int32)
    planes, img = b[8 * n:40 * n].view(np.float64).reshape(4, n), b[40 * n:].view(np.uint16).reshape(3, n)
    order = np.lexsort((col, row))
    return _record_bytes(dict(row=row[order], col=col[order], planes=planes[:, order], img=img[:, order]))


def _call_scanline_pack(env):
    i, n = env.inp, int(_keeps()[0][0].sum())
    base = env.out['records'].data_ptr()
    env.ctx.call('amt_scanline_pack', _ptr(i['keep']), 0, 0, K.NY, K.NX, _ptr(i['planes']), 4, _ptr(i['img']), 2, 3, K.NY, K.NX, 0,
                 K.S_OFFSET[0], n, base, base + 4 * n, base + 8 * n, base + 40 * n)         # synchronises


def _oracle_scanline_pack(a):
    import _scanline_oracle as SO
    return dict(records=_record_bytes(SO.pack(a['keep'], WINDOW, a['planes'], a['img'], 0, K.S_OFFSET[0])))


def _strip_records():
    """per strip (true, decoy) dicts of record arrays as long as the true strip's count: tests/_scanline_oracle.py's pack of the
    true and of the decoy strip, the decoy's cut or filled up with records of cell (0, 0)"""
    if 'records' not in K._kept:
        import _scanline_oracle as SO
        out = []
        for s in range(2):
            recs = []
            for v in range(2):
                d = K.STRIPS[s][v]
                keep, _ = SO.select(K.S_LAT, K.S_LON, d['polygon'], d['cell_mask'], WINDOW)
                recs.append(SO.pack(keep, WINDOW, d['planes'], d['img'], 0, K.S_OFFSET[s]))
            n = len(recs[0]['row'])
            fit = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros(a.shape[:-1] + (n,), a.dtype)], axis=-1)[..., :n])
            out.append((recs[0], dict((k, fit(recs[1][k])) for k in recs[1])))
        K._kept['records'] = out
    return K._kept['records']


def _compose_inputs():
    return OrderedDict(('%s%d' % (k, s), (_strip_records()[s][0][k], _strip_records()[s][1][k])) for s in range(2)
                       for k in ('row', 'col', 'planes', 'img'))


def _call_scanline_compose(n_strips):
    """two strips of records; n_strips > 2: empty strips of later frames behind them (a table of more than 1 MiB)"""
    def call(env):
        from auromat_amd._native import ScanLineStrip
        i, o = env.inp, env.out
        table = (ScanLineStrip * n_strips)()
        for s in range(n_strips):
            if s < 2:
                table[s].row, table[s].col, table[s].planes, table[s].img = (i['%s%d' % (k, s)].data_ptr() for k in ('row', 'col', 'planes', 'img'))
                table[s].count = i['row%d' % s].numel()
            table[s].frame = s
        env.ctx.call('amt_scanline_compose', table, n_strips, 2, 3, 4, 0, 0, K.NY, K.S_NX, _ptr(o['planes']), _ptr(o['img']),
                     _ptr(o['mask']), _ptr(o['frame_index']))                                # synchronises
    return call


def _oracle_scanline_compose(a):
    import _scanline_oracle as SO
    strips = [dict((k, a['%s%d' % (k, s)]) for k in ('row', 'col', 'planes', 'img')) for s in range(2)]
    planes, img, mask, index, outside = SO.compose(strips, [0, 1], 0, 0, K.NY, K.S_NX, 4, 3, np.uint16)
    assert not outside
    return dict(planes=planes, img=img, mask=mask, frame_index=index)


COMPOSE_OUT = [('planes', ((K.NY, K.S_NX, 4), np.float64)), ('img', ((K.NY, K.S_NX, 3), np.uint16)), ('mask', ((K.NY, K.S_NX), np.uint8)),
               ('frame_index', ((K.NY, K.S_NX), np.int32))]

GATHER_JOB, GATHER_CAMS, GATHER_N = 'gm-a', ('gm-a', 'gm-b'), 2      # the grid (tests/_gather_frames_cases.py), the members, the factor
GATHER_HARMLESS = 'as tests/_gated_gather_frames_cases.py: the axes select the taps and every tap is tested against the image\'s ' \
                  'frame by the kernel itself; the member table comes from the host, the same for the true arrays and the decoys'


def gather_case(name, cams, n=1, supersampled=False, job=GATHER_JOB, repeat=1):
    """amt_gather_mosaic (rule 1, 'linear', uint16 RGB) of the cameras `cams` on the n x n sub-sample points of a job's grid, or
    amt_gather_mosaic_supersampled with factor n on its cells; repeat: the member table `repeat` times over"""
    import _gather_frames_cases as FC
    import _gather_mosaic_cases as GC
    import _inverse_cases as IC
    j = FC.by_name(job)
    models = [IC.native(GC.by_name(c)) for c in cams]
    a, b, points = FC.coordinates(job, n)
    assert not points
    inputs = OrderedDict([('lat', (a, a + 0.37)), ('lon', (b, FC.wrap180(b - 0.61)))])
    for k, c in enumerate(cams):
        seed = 1 + GATHER_CAMS.index(c)             # (by the camera: a member alone samples the image it has in the mosaic)
        inputs['img_%d' % k] = (GC.image(GC.by_name(c), np.uint16, 3, seed=seed), GC.image(GC.by_name(c), np.uint16, 3, seed=50 + seed))
    ny, nx = (j['ny'], j['nx']) if supersampled else (j['ny'] * n, j['nx'] * n)
    outputs = OrderedDict([('img', ((ny, nx, 3), np.uint16)), ('mask', ((ny, nx), np.uint8)), ('elev', ((ny, nx), np.float64)),
                           ('source', ((ny, nx), np.int32))] + ([('count', ((ny, nx), np.uint8))] if supersampled else []))
    min_count = max(1, (n * n + 1) // 2)

    def call(env):
        from auromat_amd._native import GatherMember
        i, o = env.inp, env.out
        table = (GatherMember * (len(cams) * repeat))()
        for k, t in enumerate(table):
            params, zen = models[k % len(cams)]
            C.memmove(C.byref(t.params), C.byref(params), C.sizeof(params))
            if zen is not None:
                t.zenithal = C.pointer(zen)
            t.img, t.min_elevation = i['img_%d' % (k % len(cams))].data_ptr(), float('nan')
        if supersampled:
            env.ctx.call('amt_gather_mosaic_supersampled', table, len(table), 0, _ptr(i['lat']), ny, _ptr(i['lon']), nx, None, None, n,
                         min_count, 2, 3, 0, 1, _ptr(o['img']), _ptr(o['mask']), _ptr(o['elev']), _ptr(o['source']), _ptr(o['count']), None)
            env.closed('amt_gather_mosaic_supersampled')
        else:
            env.ctx.call('amt_gather_mosaic', table, len(table), 0, _ptr(i['lat']), ny, _ptr(i['lon']), nx, None, None, 2, 3, 0, 1,
                         _ptr(o['img']), _ptr(o['mask']), _ptr(o['elev']), _ptr(o['source']), None, None)
            env.closed('amt_gather_mosaic')

    case = Case(name, 'B', inputs, outputs, call, harmless=GATHER_HARMLESS)
    case.min_count = min_count
    return case


COARSE_STRIDE = 4


def _call_coarse_dirs(env):
    p = K._params()
    env.ctx.call('amt_georef_coarse_bbox_dirs', C.byref(p), _ptr(env.inp['dirs']), COARSE_STRIDE, K.MIN_ELEV, 0, _ptr(env.out['bbox']))
    env.closed('amt_georef_coarse_bbox_dirs')


def _oracle_coarse_dirs(a):
    """amt_georef_coarse_bbox_dirs by oracle.ref_numpy: the corners (min(i stride, height), min(j stride, width)) whose own ray
    hits the shell at MIN_ELEV or above -> min / max latitude, min / max longitude, smallest positive and largest non-positive
    longitude, their number, and over the corners that hit the sum of the signs of (2 column - width) times 2^20 plus that of
    (2 row - height)"""
    from oracle import ref_numpy as O
    dirs = a['dirs']
    _, cam, t = K.camera(False, 0, K.W, K.H)
    p = O.inflated_earth_intersection(dirs.reshape(-1, 3), cam, K.ALTITUDE).reshape(dirs.shape)
    lat, lon = (v.reshape(dirs.shape[:2]) for v in O.j2000_to_latlon(p.reshape(-1, 3), O.mat_j2000_to_geo(O.date2es(t))))
    elev = O.elevation_deg(dirs, p)
    gy = np.minimum(np.arange((K.H + COARSE_STRIDE - 1) // COARSE_STRIDE + 1) * COARSE_STRIDE, K.H)
    gx = np.minimum(np.arange((K.W + COARSE_STRIDE - 1) // COARSE_STRIDE + 1) * COARSE_STRIDE, K.W)
    iy, ix = np.meshgrid(gy, gx, indexing='ij')
    hit = ~np.isnan(lat[iy, ix])
    with np.errstate(invalid='ignore'):
        keep = hit & (elev[iy, ix] >= K.MIN_ELEV)
    la, lo = lat[iy, ix][keep], lon[iy, ix][keep]
    inf = np.inf
    box = [la.min() if la.size else inf, la.max() if la.size else -inf, lo.min() if lo.size else inf, lo.max() if lo.size else -inf,
           lo[lo > 0].min() if (lo > 0).any() else inf, lo[lo <= 0].max() if (lo <= 0).any() else -inf, float(keep.sum()),
           float(int(np.sign(2 * ix - K.W)[hit].sum()) * (1 << 20) + int(np.sign(2 * iy - K.H)[hit].sum()))]
    return dict(bbox=np.array(box))


def added():
    """The cases of call sites that no case of the gated side stream reaches or isolates."""
    if 'added' in K._kept:
        return K._kept['added']
    import _gated_gather_frames_cases as GF
    keeps, acc = _keeps(), _accumulators()
    n_rec = int(keeps[0][0].sum())
    cases = [
        Case('mosaic_median_union', 'B', K._mosaic_inputs(), K.MOSAIC_OUT,
             _call_mosaic('amt_mosaic_median_frames', 0, K.WINDOWS, K.H, K.W, K.XEDGES, K.YEDGES, True), _oracle_mosaic_median_union,
             synchronises=True, harmless=K.FIELD + '; the member table holds pointers and sizes from the host'),
        Case('area_finalize', 'C', OrderedDict(acc=acc), K.AREA_OUT, _call_area_finalize, _oracle_area_finalize, synchronises=True,
             index_ranges={'acc': (0, 1 << 62)},
             harmless='the accumulators are sums: divided and compared, never used as an address'),
        Case('scanline_pack', 'B', OrderedDict(keep=keeps[0], planes=(K.STRIPS[0][0]['planes'], K.STRIPS[0][1]['planes']),
                                               img=(K.STRIPS[0][0]['img'], K.STRIPS[0][1]['img'])),
             [('records', ((n_rec * REC_BYTES,), np.uint8))], _call_scanline_pack, _oracle_scanline_pack, synchronises=True,
             canonical={'records': sorted_records},
             harmless='a keep byte decides whether a record is written, and none is written beyond `count`, a host argument that '
                      'both keep arrays satisfy; planes and pixels are copied'),
        Case('scanline_compose', 'B', _compose_inputs(), COMPOSE_OUT, _call_scanline_compose(2), _oracle_scanline_compose,
             synchronises=True, index_ranges=dict([('row%d' % s, (0, K.NY)) for s in range(2)] + [('col%d' % s, (0, K.S_NX)) for s in range(2)]),
             harmless='amt_scanline_compose tests every record against the raster, and the rows and columns of the true records '
                      'and of the decoys lie inside it (checked); the strip table comes from the host'),
        gather_case('gather_pair', GATHER_CAMS),
        gather_case('gather_pair_supersampled', GATHER_CAMS, GATHER_N, supersampled=True),
        Case('coarse_bbox_dirs', 'D', OrderedDict(dirs=(K.directions(False), K.directions(True))), [('bbox', ((8,), np.float64))],
             _call_coarse_dirs, _oracle_coarse_dirs, harmless=K.DIRS),
    ] + GF.build()
    K._kept['added'] = cases
    return cases


# cases without a CPU oracle: gathering has none in this suite — its exact oracles (tests/test_gpu_gather_mosaic_cells.py,
# tests/test_gpu_gather_supersample_cells.py) compose the device's own per-member and per-point results, and so does
# tests/test_gpu_scratch_state.py for the two mosaics here
EXEMPT = ('gather_pair', 'gather_pair_supersampled', 'gather_frames_x1', 'gather_frames_x3')


def build():
    """Every case: the gated side stream's, then the added ones."""
    return K.build() + added()


def by_name():
    return OrderedDict((c.name, c) for c in build())


# ---- the larger shapes: the same calls needing more than 1 MiB -------------------------------------------------------------------

LH, LW = 257, 255                                # 65535 pixels: 18 bytes each in the median's passes
FINE_X, FINE_Y = np.linspace(9.0, 29.0, 168), np.linspace(39.0, 51.0, 159)       # 167 x 158 cells: 5 planes of 8 bytes each
FINE_NX, FINE_NY = 167, 158
FINE_WINDOWS = ((0, 0, 100, FINE_NY), (60, 0, 107, FINE_NY))
NN_X, NN_Y = np.linspace(9.0, 29.0, 231), np.linspace(39.0, 51.0, 201)           # 230 x 200 cells: 12 bytes each, 8 per pixel
N_STRIPS_LARGE = 22000                           # x 48 bytes
N_MEMBERS_LARGE = 1024                           # x more than 1900 bytes (the SIP tables alone are 1600)
BIG_W, BIG_H = 2016, 8192                        # 33 strips x 512 bands of work items x 64 bytes
COARSE_W = 2100                                  # (2101 x 2101 corners / 256) blocks x 64 bytes
CUBIC_LARGE_ROWS = 65                            # 4225 points x (256 + 32) bytes


def _frame_call(entry, h, w, xedges, yedges):
    def call(env):
        i = env.inp
        xa, ya = _axes(env.ctx, xedges, yedges)
        if entry == 'amt_median_frame_async':
            env.ctx.call(entry, _ptr(i['lat_c']), _ptr(i['lon_c']), _ptr(i['elev']), _ptr(i['img']), 2, 3, None, h, w, K.MIN_ELEV,
                         C.byref(xa), C.byref(ya), 0, 0, *K._grid_ptrs(env.out))
        else:
            env.ctx.call(entry, _ptr(i['lat']), _ptr(i['lon']), _ptr(i['lat_c']), _ptr(i['elev']), _ptr(i['img']), 2, 3, None, h, w,
                         K.MIN_ELEV, C.byref(xa), C.byref(ya), 0, 0, 0, h, C.c_uint64(K.HALF), *(K._grid_ptrs(env.out) + [None]))
        env.closed(entry)
    return call


def _call_nearest_large(env):
    from _gated_stream import dev
    i, o = env.inp, env.out
    xa, ya = _axes(env.ctx, NN_X, NN_Y)
    key = K._key('targets_large', env.ctx)
    if key not in K._kept:
        K._kept[key] = (dev((NN_Y[:-1] + 0.5 * (NN_Y[1] - NN_Y[0]))[::-1].copy()), dev(NN_X[:-1] + 0.5 * (NN_X[1] - NN_X[0])))
    tlat, tlon = K._kept[key]
    env.ctx.call('amt_nearest_frame', _ptr(i['lat_c']), _ptr(i['lon_c']), _ptr(i['elev']), None, LH, LW, K.MIN_ELEV, C.byref(xa),
                 C.byref(ya), 0, _ptr(tlat), _ptr(tlon), None, _ptr(o['index']))
    env.closed('amt_nearest_frame')


def _call_georef_box_large(env):
    """the box of a frame alone, in (MLat, SM longitude): what amt_pipe_launch_box asks of the frame kernel, with the partials
    in the context's buffer"""
    from auromat_amd._native import GeorefOut
    g = GeorefOut()
    g.altitude, g.bbox, g.bbox_min_elevation, g.bin_magnetic = K.ALTITUDE, env.out['bbox'].data_ptr(), K.MIN_ELEV, 1
    p = K._params(0, BIG_W, BIG_H)
    env.ctx.call('amt_georef_frame', C.byref(p), C.byref(g))
    env.closed('amt_georef_frame')


def _call_coarse_large(env):
    p = K._params(0, COARSE_W, COARSE_W)
    env.ctx.call('amt_georef_coarse_bbox', C.byref(p), 1, K.MIN_ELEV, 0, _ptr(env.out['bbox']))
    env.closed('amt_georef_coarse_bbox')


def _cubic_large_inputs():
    """K.cubic_inputs' true arrays for a jittered lattice of CUBIC_LARGE_ROWS rows, without targets"""
    if 'cubic_large' in K._kept:
        return K._kept['cubic_large']
    from auromat_amd import _native
    L = _native.lib()
    rows = CUBIC_LARGE_ROWS
    n = rows * rows
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = np.random.RandomState(41)
    r, c = np.divmod(np.arange(n), rows)
    xy = np.ascontiguousarray(np.stack([c + rng.uniform(-0.3, 0.3, n), r + rng.uniform(-0.3, 0.3, n)], axis=1))
    handle = C.c_void_p()
    assert L.amt_delaunay_create(p(xy), n, C.byref(handle)) == 0
    nt, nn, nd = C.c_int64(), C.c_int64(), C.c_int64()
    assert L.amt_delaunay_sizes(handle, C.byref(nt), C.byref(nn), C.byref(nd)) == 0 and nd.value == 0
    indptr, indices = np.empty(n + 1, dtype=np.int64), np.empty(nn.value, dtype=np.int32)
    assert L.amt_delaunay_vertex_neighbours(handle, p(indptr), p(indices)) == 0
    L.amt_delaunay_destroy(handle)
    K._kept['cubic_large'] = dict(xy=xy, indptr=indptr, indices=indices, row_start=np.arange(0, n + 1, rows, dtype=np.int64),
                                  values=K._q(rng.uniform(0.0, 100.0, (n, 2)), 1 / 64.0))
    return K._kept['cubic_large']


def _call_cubic_large(env):
    i, n = env.inp, CUBIC_LARGE_ROWS * CUBIC_LARGE_ROWS
    sweeps = (C.c_int32 * 2)()
    env.ctx.call('amt_cubic_gradients_csr', _ptr(i['xy']), n, _ptr(i['indptr']), _ptr(i['indices']), _ptr(i['row_start']),
                 CUBIC_LARGE_ROWS, _ptr(i['values']), 2, 1e-6, 400, _ptr(env.out['gradients']), sweeps)       # synchronises
    return dict(sweeps=list(sweeps))


def _settled(d):
    """inputs of a case that only ever runs on settled inputs: the decoy is the true array"""
    return OrderedDict((k, (v, v)) for k, v in d.items())


def large():
    """call site -> the Case of the same call at a shape that needs more than 1 MiB of scratch memory (NO_LARGE: none can).
    They run on settled inputs only and are compared with their own baseline."""
    if 'large' in K._kept:
        return K._kept['large']
    a, b = scene(51, LH, LW), scene(52, LH, LW)
    ma, mb = scene(53, 129, LW), scene(54, 129, LW, 40.5, 13.0)
    sa, sb = K.TRUE, K.MEMBER_B[0]
    small_members = _settled(OrderedDict([(pre + '_' + k, s[k]) for k in ('lat', 'lon', 'lat_c', 'lon_c', 'elev', 'img')
                                          for pre, s in (('a', sa), ('b', sb))]))
    big_members = _settled(OrderedDict([(pre + '_' + k, s[k]) for k in ('lat', 'lon', 'lat_c', 'lon_c', 'elev', 'img')
                                        for pre, s in (('a', ma), ('b', mb))]))
    fine_mosaic = OrderedDict(GRID_OUT(FINE_NY, FINE_NX), source=((FINE_NY, FINE_NX), np.int32))
    cubic = _cubic_large_inputs()
    n_cubic = CUBIC_LARGE_ROWS * CUBIC_LARGE_ROWS
    why = 'settled inputs only'
    out = OrderedDict([
        (('amt_mosaic.hip', 'amt_mosaic_run'),
         Case('mosaic_large', 'B', small_members, fine_mosaic,
              _call_mosaic('amt_mosaic_frames', 1, FINE_WINDOWS, K.H, K.W, FINE_X, FINE_Y, False), harmless=why)),
        (('amt_median.hip', 'median_front'),
         Case('median_frame_async_large', 'C', _settled(dict((k, a[k]) for k in ('lat_c', 'lon_c', 'elev', 'img'))), K.GRID_OUT,
              _frame_call('amt_median_frame_async', LH, LW, K.XEDGES, K.YEDGES), harmless=why)),
        (('amt_median.hip', 'mosaic_median_front'),
         Case('mosaic_median_union_large', 'B', big_members, K.MOSAIC_OUT,
              _call_mosaic('amt_mosaic_median_frames', 0, K.WINDOWS, 129, LW, K.XEDGES, K.YEDGES, True), synchronises=True, harmless=why)),
        (('amt_area.hip', 'amt_area_frame_async'),
         Case('area_frame_async_large', 'C', _settled(dict((k, K.TRUE[k]) for k in ('lat', 'lon', 'lat_c', 'elev', 'img'))),
              GRID_OUT(FINE_NY, FINE_NX), _frame_call('amt_area_frame_async', K.H, K.W, FINE_X, FINE_Y), harmless=why)),
        (('amt_area.hip', 'amt_area_mosaic_frames'),
         Case('mosaic_area_large', 'B', small_members, fine_mosaic,
              _call_mosaic('amt_area_mosaic_frames', 1, FINE_WINDOWS, K.H, K.W, FINE_X, FINE_Y, True), synchronises=True, harmless=why)),
        (('amt_scanline.hip', 'amt_scanline_compose'),
         Case('scanline_compose_large', 'B', _settled(OrderedDict((k, v[0]) for k, v in _compose_inputs().items())), COMPOSE_OUT,
              _call_scanline_compose(N_STRIPS_LARGE), synchronises=True, harmless=why)),
        (('amt_gather.hip', 'gather_prepare'), gather_case('gather_mosaic_large', ('gm-a',), job='g33x31', repeat=N_MEMBERS_LARGE)),
        (('amt_georef.hip', 'prepare_georef'),
         Case('georef_box_large', 'D', OrderedDict(), [('bbox', ((8,), np.float64))], _call_georef_box_large, harmless=why)),
        (('amt_georef.hip', 'coarse_bbox'),
         Case('coarse_bbox_large', 'D', OrderedDict(), [('bbox', ((8,), np.float64))], _call_coarse_large, harmless=why)),
        (('amt_nearest.hip', 'amt_nearest_frame'),
         Case('nearest_large', 'C', _settled(dict((k, b[k]) for k in ('lat_c', 'lon_c', 'elev'))), [('index', ((200, 230), np.int64))],
              _call_nearest_large, harmless=why)),
        (('amt_nearest.hip', 'amt_cubic_gradients_csr'),
         Case('cubic_large', 'B', _settled(cubic), [('gradients', ((n_cubic, 2, 2), np.float64))], _call_cubic_large, synchronises=True,
              harmless=why)),
    ])
    K._kept['large'] = out
    return out


def large_bytes():
    """call site -> the bytes its larger case asks amt_workspace for, as the library's source lays the buffer out (a lower bound
    where a term is left out): every one above MIN_BYTES"""
    up = lambda v: (v + 255) // 256 * 256
    n, cells = LH * LW, K.NX * K.NY
    median = lambda n, cells: up(8 * cells) + 256 + up(4 * (cells + 1)) + 256 + 2 * up(4 * cells) + up(4 * n) + up(6 * n) + up(8 * n)
    win = sum(w[2] * w[3] for w in FINE_WINDOWS)
    return OrderedDict([
        (('amt_mosaic.hip', 'amt_mosaic_run'), 5 * 8 * win),
        (('amt_median.hip', 'median_front'), median(n, cells)),
        (('amt_median.hip', 'mosaic_median_front'), median(2 * 129 * LW, cells)),
        (('amt_area.hip', 'amt_area_frame_async'), 5 * 8 * FINE_NX * FINE_NY + 256),
        (('amt_area.hip', 'amt_area_mosaic_frames'), 5 * 8 * win),
        (('amt_scanline.hip', 'amt_scanline_compose'), N_STRIPS_LARGE * 48 + 256),
        (('amt_gather.hip', 'gather_prepare'), N_MEMBERS_LARGE * 1900),
        (('amt_georef.hip', 'prepare_georef'), ((BIG_W + 63) // 63 * ((BIG_H + 15) // 16) + 64) * 64),
        (('amt_georef.hip', 'coarse_bbox'), ((COARSE_W + 1) ** 2 + 255) // 256 * 64),
        (('amt_nearest.hip', 'amt_nearest_frame'), 4 * (3 * 230 * 200 + 1) + 8 * n),
        (('amt_nearest.hip', 'amt_cubic_gradients_csr'), CUBIC_LARGE_ROWS ** 2 * (32 + 256) + 1024),
    ])
