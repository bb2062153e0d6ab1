"""
Constructed inputs for the median kernels (auromat_amd/csrc/amt_median.hip): exactly the pixels a test wants in exactly
the cells it wants, as plain host arrays, seeded and deterministic.  A plain helper module (NumPy only) for
tests/test_gpu_median_cells.py, which runs the cases on the device, and tests/test_median_cpu.py, which checks without a
GPU that every case still holds what it promises.

The expected result of a case (``expected``) comes from tests/_median_oracle.py alone: ``median_loop`` (a literal np.median
per cell) where the non-empty cells are few, ``median_bins`` otherwise, and the image through
oracle.ref_numpy.finalize_image.  Nothing here is taken from the library.

No binned pixel has a NaN elevation: no mapping produces a finite latitude with a NaN elevation (the elevation is NaN
exactly where the line of sight misses the shell, and there the latitude is NaN too), and what np.median does with a NaN is
not the statement of the feature.  NaN elevations do appear, on pixels that every run of a case excludes (NaN latitude or
longitude, outside the edges).
"""
import functools

import numpy as np

import _median_oracle as M

# The tier boundaries of auromat_amd/csrc/amt_median.hip, by the source's names: a cell of up to kSmallMax keys is sorted
# by one wave, one of up to kLargeMin keys is selected by one workgroup in LDS, larger ones by many workgroups which take
# kChunk keys each, kBlock at a time.  test_median_cpu.py reads the four values from the source and compares.
K_SMALL_MAX = 64        # kSmallMax
K_LARGE_MIN = 16384     # kLargeMin
K_CHUNK = 4096          # kChunk
K_BLOCK = 256           # kBlock

COUNTS = (0, 1, 2, 3,
          K_SMALL_MAX - 1, K_SMALL_MAX, K_SMALL_MAX + 1, K_SMALL_MAX + 2,
          K_BLOCK - 1, K_BLOCK, K_BLOCK + 1,
          K_CHUNK - 1, K_CHUNK, K_CHUNK + 1,
          K_LARGE_MIN - 1, K_LARGE_MIN, K_LARGE_MIN + 1, K_LARGE_MIN + 2,
          5 * K_CHUNK, 5 * K_CHUNK + 1, 4 * K_LARGE_MIN + 1)
BIG = 300001            # one more cell, appended to row BIG_ROW as a column of its own
BIG_ROW = 3
ROWS = 6                # one row per value family
ORDERS = ('sorted', 'shuffled', 'runs')
RUN_LENGTHS = (1, 2, 3, 5, 7, 64, 250, 1021)
TABLE_SIZE = (1189, 1201)       # height, width: both odd, room for an excluded pixel in every 97th position
LOOP_MAX_CELLS = 512            # up to this many non-empty cells the expected medians are a literal np.median loop

TIERS = ('small', 'medium', 'large')


def tier_of(count):
    count = np.asarray(count)
    return np.where(count <= K_SMALL_MAX, 0, np.where(count <= K_LARGE_MIN, 1, 2))


class Case(object):
    """Host arrays of one frame and how to run it.  ``lon`` is what the device gets, ``lon_binned`` the x coordinate the
    oracle bins (the same array unless the device wraps or converts it); ``img`` is (n, nchan), nchan 0..4."""

    def __init__(self, name, oracle_key, lat, lon, elev, img, mask, xedges, yedges, height, width, min_elevation=-np.inf,
                 lon_wrap=0, lon_from_mlt=0, uniform=False, lon_binned=None):
        assert lat.size == lon.size == height * width == img.shape[0]
        self.name, self.oracle_key = name, oracle_key
        self.lat, self.lon, self.elev, self.img, self.mask = lat, lon, elev, img, mask
        self.xedges, self.yedges, self.height, self.width = xedges, yedges, height, width
        self.min_elevation, self.lon_wrap, self.lon_from_mlt, self.uniform = min_elevation, lon_wrap, lon_from_mlt, uniform
        self.lon_binned = lon if lon_binned is None else lon_binned

    def arrays(self):
        return (self.lat, self.lon, self.elev, self.img, self.mask, self.xedges, self.yedges, self.height, self.width)

    @property
    def shape(self):
        return len(self.yedges) - 1, len(self.xedges) - 1

    def keep(self):
        """The pixels the membership rule lets through before the edges: centre mask 0, elevation >= the threshold."""
        keep = np.ones(self.lat.size, dtype=bool)
        if self.mask is not None:
            keep &= self.mask == 0
        if self.elev is not None and not (np.isinf(self.min_elevation) and self.min_elevation < 0):
            with np.errstate(invalid='ignore'):
                keep &= self.elev >= self.min_elevation
        return keep

    def flat(self):
        """Output cell of every pixel (rows north to south), -1 for the excluded ones."""
        return np.where(self.keep(), M.cell_index(self.lon_binned, self.lat, self.xedges, self.yedges), -1)


def expected_from(lat, x, planes, xedges, yedges, keep, loop=None):
    """(median (ny, nx, k) of the columns of `planes`, count (ny, nx)) by the oracle."""
    ny, nx = len(yedges) - 1, len(xedges) - 1
    flat = np.where(keep, M.cell_index(x, lat, xedges, yedges), -1)
    count = np.bincount(flat[flat >= 0], minlength=nx * ny).reshape(ny, nx).astype(np.float64)
    if planes.shape[1] == 0:
        return np.full((ny, nx, 0), np.nan), count
    if loop is None:
        loop = (count > 0).sum() <= LOOP_MAX_CELLS
    if loop:
        med = M.median_loop(x, lat, planes, xedges, yedges, keep=keep)
    else:
        med, count_bins = M.median_bins(x, lat, planes, xedges, yedges, keep=keep)
        assert np.array_equal(count_bins, count)
    return med, count


def expected(case, loop=None):
    """dict(median (ny, nx, nchan + 1), img (ny, nx, nchan), mask, count) of a case by the oracle."""
    from oracle import ref_numpy as O
    keep = case.keep()
    med_img, count = expected_from(case.lat, case.lon_binned, case.img, case.xedges, case.yedges, keep, loop)
    if case.elev is not None:
        med_el, _ = expected_from(case.lat, case.lon_binned, case.elev[:, None], case.xedges, case.yedges, keep, loop)
    else:
        med_el = np.full(count.shape + (1,), np.nan)
    want_img, _ = O.finalize_image(med_img, case.img.dtype)
    return dict(median=np.concatenate([med_img, med_el], axis=2), img=want_img, mask=count == 0, count=count)


def middle_pairs(flat, values):
    """(cell, count, lower middle value, upper middle value) of every non-empty cell of one plane."""
    sel = flat >= 0
    f, v = flat[sel], np.asarray(values)[sel]
    count = np.bincount(f)
    start = np.concatenate(([0], np.cumsum(count)[:-1]))
    sv = v[np.lexsort((v, f))]
    full = np.flatnonzero(count > 0)
    n = count[full]
    return full, n, sv[start[full] + (n - 1) // 2], sv[start[full] + n // 2]


# ---- (a) the tier table ------------------------------------------------------------------------------------------------
def int_family(f, c, hi, rng):
    """Family f (0..5) of c values of an integer plane with maximum hi, permuted."""
    idx = np.arange(c)
    half_up = (c + 1) // 2
    if f == 0:                                  # all keys equal
        v = np.full(c, hi // 3)
    elif f == 1:                                # extremes: the middle pair of an even count is 0 | hi
        v = np.where(idx < half_up, 0, hi)
    elif f == 2:                                # the middle pair straddles a digit carry
        low = 0x0F if hi == 255 else 0x00FF
        v = np.where(idx < half_up, low, low + 1)
    elif f == 3:                                # one duplicate more than half: the upper middle key equals the lower one
        v = 8 + (idx - (c // 2 + 1)) % (hi - 8)
        v[:c // 2 + 1] = 7
    elif f == 4:                                # exactly half: the upper middle key is the smallest of many keys above
        v = hi - (idx - half_up) % (hi - 7)
        v[:half_up] = 7
    else:
        v = rng.randint(0, hi + 1, c)
    return rng.permutation(v)


def elev_family(f, c, rng):
    """The same six ideas for the elevation plane, in float64."""
    idx = np.arange(c)
    half_up = (c + 1) // 2
    if f == 0:
        v = np.full(c, -3.25)
    elif f == 1:                                # negative | smallest subnormal: opposite signs, top digit differs
        v = np.where(idx < half_up, -1e-300, 5e-324)
    elif f == 2:                                # the lowest digit differs
        v = np.where(idx < half_up, 12.5, np.nextafter(12.5, 13.0))
    elif f == 3:
        v = np.maximum(rng.normal(0, 30, c), -6.9)
        v[:c // 2 + 1] = -7.0
    elif f == 4:
        v = -np.abs(rng.normal(0, 30, c)) - 1
    else:
        v = rng.normal(0, 30, c)
    return rng.permutation(v)


def table_counts():
    """(ROWS, columns) pixels per cell: COUNTS in every row, BIG in a last column of row BIG_ROW."""
    c = np.zeros((ROWS, len(COUNTS) + 1), dtype=np.int64)
    c[:, :-1] = COUNTS
    c[BIG_ROW, -1] = BIG
    return c


@functools.lru_cache(maxsize=None)
def _table_base(dtype_name):
    """The table's pixels sorted by cell (row r, column k: latitude r + 0.5, longitude k + 0.5), then the excluded ones:
    4 channels (channel ch of row r is family (r + ch) % 6) and the elevation (family (r + 4) % 6)."""
    dtype = np.dtype(dtype_name)
    hi = int(np.iinfo(dtype).max)
    counts = table_counts()
    height, width = TABLE_SIZE
    n, n_valid = height * width, int(counts.sum())
    lat, lon = np.empty(n), np.empty(n)
    elev = np.empty(n)
    img = np.empty((n, 4), dtype=dtype)
    mask = np.zeros(n, dtype=np.uint8)
    at = 0
    for r in range(ROWS):
        for k in range(counts.shape[1]):
            c = int(counts[r, k])
            if c == 0:
                continue
            rng = np.random.RandomState(1000 * r + k + (0 if hi == 255 else 500000))
            s = slice(at, at + c)
            lat[s], lon[s] = r + 0.5, k + 0.5
            for ch in range(4):
                img[s, ch] = int_family((r + ch) % 6, c, hi, rng)
            elev[s] = elev_family((r + 4) % 6, c, rng)
            at += c
    assert at == n_valid
    # excluded pixels, four kinds in turn; those that lie inside a cell carry values that would show in its median
    j = np.arange(n - n_valid)
    kind = j % 4
    lat[at:] = np.where(kind == 0, np.nan, np.where(kind == 2, ROWS + 1.5, (j % ROWS) + 0.5))
    lon[at:] = np.where(kind == 1, -3.5, (j % counts.shape[1]) + 0.5)
    elev[at:] = np.where(kind == 0, np.nan, 1e6)
    img[at:] = hi
    mask[at:] = kind == 3
    xedges = np.arange(counts.shape[1] + 1, dtype=np.float64)
    yedges = np.arange(ROWS + 1, dtype=np.float64)
    for a in (lat, lon, elev, img, mask):
        a.setflags(write=False)
    return lat, lon, elev, img, mask, xedges, yedges, n_valid


@functools.lru_cache(maxsize=None)
def table_order(order):
    """Permutation of the table's pixels: position -> index into the sorted base."""
    counts = table_counts().ravel()
    height, width = TABLE_SIZE
    n, n_valid = height * width, int(counts.sum())
    if order == 'sorted':
        return np.arange(n)
    if order == 'shuffled':
        return np.random.RandomState(77).permutation(n)
    assert order == 'runs'
    pos = np.concatenate(([0], np.cumsum(counts)[:-1]))
    left = counts.copy()
    active = [c for c in range(len(counts)) if counts[c]]
    pieces, j = [], 0
    while active:
        still = []
        for c in active:
            run = min(RUN_LENGTHS[j % len(RUN_LENGTHS)], int(left[c]))
            j += 1
            pieces.append(np.arange(pos[c], pos[c] + run))
            pos[c] += run
            left[c] -= run
            if left[c]:
                still.append(c)
        active = still
    valid = np.concatenate(pieces)
    assert valid.size == n_valid
    # an excluded pixel in every 97th position while valid ones remain, the other excluded ones after them
    slot = np.arange(n)
    for_valid = np.flatnonzero(slot % 97 != 96)[:n_valid]
    assert for_valid.size == n_valid
    perm = np.empty(n, dtype=np.int64)
    is_valid = np.zeros(n, dtype=bool)
    is_valid[for_valid] = True
    perm[is_valid] = valid
    perm[~is_valid] = np.arange(n_valid, n)
    return perm


def tier_table(dtype, nchan, with_elev, order='sorted'):
    lat, lon, elev, img, mask, xedges, yedges, _ = _table_base(np.dtype(dtype).name)
    p = table_order(order)
    height, width = TABLE_SIZE
    return Case('table-%s-%d-%s-%s' % (np.dtype(dtype).name, nchan, 'elev' if with_elev else 'noelev', order),
                ('table', np.dtype(dtype).name, nchan, bool(with_elev)),
                lat[p], lon[p], elev[p] if with_elev else None, np.ascontiguousarray(img[p][:, :nchan]), mask[p], xedges,
                yedges, height, width)


@functools.lru_cache(maxsize=None)
def _table_expected_full(dtype_name):
    return expected(tier_table(dtype_name, 4, True, 'sorted'))


def table_expected(dtype, nchan, with_elev):
    """Expected outputs of the table whatever the order: the oracle runs once per dtype, on all planes."""
    full = _table_expected_full(np.dtype(dtype).name)
    med = np.concatenate([full['median'][..., :nchan], full['median'][..., 4:] if with_elev else
                          np.full(full['count'].shape + (1,), np.nan)], axis=2)
    return dict(median=med, img=full['img'][..., :nchan], mask=full['mask'], count=full['count'])


def table_promises(dtype):
    """What the table holds, from its arrays alone: per tier and plane kind the even-count cells whose middle pair is equal /
    differs, the (cell, channel) pairs whose mean ends in .5, and more (see the CPU test)."""
    case = tier_table(dtype, 4, True, 'sorted')
    flat = case.flat()
    out = dict(equal={}, differ={}, odd_gap={}, half_even_differs=0, opposite_signs=0)
    cell_count = np.bincount(flat[flat >= 0], minlength=case.shape[0] * case.shape[1])
    for t, tier in enumerate(TIERS):
        in_tier = (flat >= 0) & (tier_of(cell_count[np.maximum(flat, 0)]) == t)
        out['odd_gap'][tier] = M.odd_gap_pairs(case.lon, case.lat, case.img, case.xedges, case.yedges, keep=in_tier)
    for kind, planes in (('int', [case.img[:, ch] for ch in range(4)]), ('float64', [case.elev])):
        for tier in TIERS:
            out['equal'][kind, tier] = out['differ'][kind, tier] = 0
        for v in planes:
            _, n, lo, hi = middle_pairs(flat, v)
            even = n % 2 == 0
            for t, tier in enumerate(TIERS):
                here = even & (tier_of(n) == t)
                out['equal'][kind, tier] += int((here & (lo == hi)).sum())
                out['differ'][kind, tier] += int((here & (lo != hi)).sum())
            if kind == 'int':
                # a mean n.5 with n even: round-half-to-even (n) and round-half-up (n + 1) part
                s = lo.astype(np.int64) + hi.astype(np.int64)
                out['half_even_differs'] += int((even & (s % 4 == 1)).sum())
            else:
                out['opposite_signs'] += int((even & (np.signbit(lo) != np.signbit(hi))).sum())
    return out


# ---- (b) membership ----------------------------------------------------------------------------------------------------
MEMBERSHIP_SIZE = (133, 151)
MEMBERSHIP_THRESHOLD = 5.0


def _points_with_edges(rng, xedges, yedges, n=20000):
    """As tests/test_median_cpu.py makes them: inside, outside on all four sides, exactly on every edge and one ulp to either
    side of it (the last edge included)."""
    x = rng.uniform(xedges[0] - 0.5, xedges[-1] + 0.5, n)
    y = rng.uniform(yedges[0] - 0.5, yedges[-1] + 0.5, n)
    ex = np.concatenate([xedges, np.nextafter(xedges, -np.inf), np.nextafter(xedges, np.inf)])
    ey = np.concatenate([yedges, np.nextafter(yedges, -np.inf), np.nextafter(yedges, np.inf)])
    x = np.concatenate([x, ex, rng.uniform(xedges[0], xedges[-1], len(ey))])
    y = np.concatenate([y, rng.uniform(yedges[0], yedges[-1], len(ex)), ey])
    return x, y


def membership_edges(axis, coord):
    if axis == 'uniform':
        xedges = np.linspace(0.0, 4.0, 9) if coord == 'plain' else np.linspace(-100.0, 60.0, 9)
        yedges = np.linspace(-2.0, 1.0, 7)
    else:
        xedges = np.array([0.0, 0.3, 1.0, 1.2, 2.5, 2.75, 3.5, 3.9, 4.4])
        if coord != 'plain':
            xedges = -100.0 + 36.0 * xedges
        yedges = np.array([-2.0, -1.7, -1.0, -0.2, 0.1, 0.6, 1.0])
    return xedges, yedges


def membership(dtype, axis='uniform', mode='nothreshold', coord='plain'):
    """About 20 k points on a 8 x 6 grid.  axis: 'uniform' | 'nonuniform'.  mode: 'nothreshold' (min_elevation -inf, centre
    mask on), 'threshold' (both on), 'nomask' (threshold on, no centre mask).  coord: 'plain', 'wrap' (longitudes over
    -360..360, lon_wrap) or 'mlt' (MLT hours, lon_from_mlt and lon_wrap)."""
    from oracle import ref_numpy as O
    dtype = np.dtype(dtype)
    xedges, yedges = membership_edges(axis, coord)
    rng = np.random.RandomState(11)
    x, y = _points_with_edges(rng, xedges, yedges)
    height, width = MEMBERSHIP_SIZE
    n = height * width
    pad = n - x.size
    assert 0 < pad < 100
    x = np.concatenate([x, rng.uniform(xedges[0], xedges[-1], pad)])
    y = np.concatenate([y, np.full(pad, np.nan)])
    x[::997] = np.nan
    y[5::991] = np.nan
    lon_binned = None
    if coord == 'wrap':
        x = rng.uniform(-360.0, 360.0, n)
        x[::997] = np.nan
        lon_binned = O.wrap_at(x + 180, 180)
    elif coord == 'mlt':
        x = rng.uniform(0.0, 24.0, n)
        x[::997] = np.nan
        lon_binned = O.wrap_at((x - 12) * 15 + 180, 180)
    else:
        assert coord == 'plain'
    elev = rng.uniform(0.0, 50.0, n)            # ~10 % below the threshold
    # NaN elevations only where every mode excludes the pixel: NaN coordinates, and some points outside the edges
    outside = np.flatnonzero(~np.isnan(y) & (y < yedges[0]))[:7]
    elev[np.isnan(x) | np.isnan(y)] = np.nan
    elev[outside] = np.nan
    img = rng.randint(0, int(np.iinfo(dtype).max) + 1, (n, 3)).astype(dtype)
    mask = (rng.uniform(size=n) < 0.1).astype(np.uint8)
    return Case('membership-%s-%s-%s-%s' % (dtype.name, axis, mode, coord), ('membership', dtype.name, axis, mode, coord),
                y, x, elev, img, None if mode == 'nomask' else mask, xedges, yedges, height, width,
                min_elevation=-np.inf if mode == 'nothreshold' else MEMBERSHIP_THRESHOLD,
                lon_wrap=int(coord != 'plain'), lon_from_mlt=int(coord == 'mlt'), uniform=axis == 'uniform',
                lon_binned=lon_binned)


# ---- (c) tails and tiny frames -----------------------------------------------------------------------------------------
TAIL_SIZES = ((1, 1), (1, 2), (1, 3), (1, 5), (3, 21), (1, 64), (5, 13), (1, 255), (257, 1), (7, 1021))
TAIL_CELLS = (1, 2, 5)


def tails(dtype, height, width, ncell):
    """Every pixel valid, pixel i in cell i % ncell of a 1 x ncell grid; no centre mask."""
    dtype = np.dtype(dtype)
    n = height * width
    rng = np.random.RandomState(height * 10007 + width * 13 + ncell)
    lon = (np.arange(n) % ncell) + 0.5
    img = rng.randint(0, int(np.iinfo(dtype).max) + 1, (n, 3)).astype(dtype)
    return Case('tails-%s-%dx%d-%d' % (dtype.name, height, width, ncell), ('tails', dtype.name, height, width, ncell),
                np.full(n, 0.5), lon, rng.normal(0, 30, n), img, None, np.arange(ncell + 1, dtype=np.float64),
                np.array([0.0, 1.0]), height, width)


# ---- (d) a wide sparse grid --------------------------------------------------------------------------------------------
SPARSE_GRID = (1000, 1100)      # ny, nx: more than 256 tiles of the scan (kBlock * 8 cells each)
SPARSE_SIZE = (286, 287)
SPARSE_PLACED = (70, 5000, 17000)


def sparse_placed_cells():
    """(iy, ix) of the first, a middle and the very last cell in the device's cell order (iy * nx + ix)."""
    ny, nx = SPARSE_GRID
    return ((0, 0), (ny // 2, nx // 2 + 3), (ny - 1, nx - 1))


def sparse(dtype):
    """60 k pixels at seeded random cells of a 1100 x 1000 grid and three cells of 70, 5000 and 17000 pixels."""
    dtype = np.dtype(dtype)
    ny, nx = SPARSE_GRID
    height, width = SPARSE_SIZE
    n = height * width
    rng = np.random.RandomState(23)
    iy = rng.randint(0, ny, 60000)
    ix = rng.randint(0, nx, 60000)
    for (py, px), c in zip(sparse_placed_cells(), SPARSE_PLACED):
        iy = np.concatenate([iy, np.full(c, py)])
        ix = np.concatenate([ix, np.full(c, px)])
    pad = n - iy.size
    assert 0 < pad < 64
    p = rng.permutation(iy.size)
    lat = np.concatenate([iy[p] + 0.5, np.full(pad, np.nan)])
    lon = np.concatenate([ix[p] + 0.5, np.full(pad, 0.5)])
    elev = rng.normal(0, 30, n)
    elev[np.isnan(lat)] = np.nan
    img = rng.randint(0, int(np.iinfo(dtype).max) + 1, (n, 3)).astype(dtype)
    return Case('sparse-%s' % dtype.name, ('sparse', dtype.name), lat, lon, elev, img, np.zeros(n, dtype=np.uint8),
                np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), height, width)


# ---- (e) one cell larger than a whole grid of the large tier -----------------------------------------------------------
HUGE = 300 * K_CHUNK + 2        # even, and more chunks than the 256 workgroups amt_median_frame_async starts on an MI355X:
HUGE_SIZE = (1109, 1109)        # its workgroups come round to a second chunk of the cell


def one_large_cell(dtype):
    """A 1 x 1 grid whose cell holds HUGE pixels in random order: channel 0 'exactly half' (the upper middle key is the
    smallest of many above, somewhere in the segment), channel 1 'one duplicate more than half', channel 2 the digit carry,
    the elevation the pair that straddles zero."""
    dtype = np.dtype(dtype)
    hi = int(np.iinfo(dtype).max)
    height, width = HUGE_SIZE
    n = height * width
    rng = np.random.RandomState(31)
    img = np.full((n, 3), hi, dtype=dtype)
    for ch, f in enumerate((4, 3, 2)):
        img[:HUGE, ch] = int_family(f, HUGE, hi, rng)
    elev = np.full(n, np.nan)
    elev[:HUGE] = elev_family(1, HUGE, rng)
    lat = np.full(n, np.nan)
    lat[:HUGE] = 0.5
    p = rng.permutation(n)
    return Case('one-large-cell-%s' % dtype.name, ('one-large-cell', dtype.name), lat[p], np.full(n, 0.5), elev[p], img[p],
                None, np.array([0.0, 1.0]), np.array([0.0, 1.0]), height, width)
