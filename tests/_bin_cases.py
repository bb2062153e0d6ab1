"""
Constructed inputs for the mean-binning kernels (k_bin_frame of auromat_amd/csrc/amt_bin_tile.h, k_bin_finalize,
k_mosaic_select, k_hist2d): frames built for the kernels' structure — the LDS window round a tile's anchor and the global
path outside it, the anchor election, the packed image decode, tile tails, heavy cells, exact halves, mosaic windows on and
next to the select tiles — as plain host arrays, seeded and deterministic.  A plain helper module (NumPy only) for
tests/test_gpu_bin_cells.py, which runs the cases on the device, and tests/test_bin_cases_cpu.py, which checks without a GPU
that every case holds what its ``promises()`` say.  The expected results come from tests/_bin_oracle.py alone.

Most cases live on unit cells: edges 0, 1, ..., n, and a pixel meant for cell (ix, iy) (iy ascending with latitude) sits at
longitude ix + 0.5 and latitude iy + 0.5.  As in the median cases no kept pixel has a NaN elevation.

``paths`` is the CPU model of the tile body: the anchor of a K_BW x TILE_H tile is the cell of its first kept, in-grid (for a
mosaic member: in-window) pixel in row-major order; a pixel is summed in LDS iff its cell lies in
[anchor - K_WX / 2, anchor + K_WX / 2) in x and likewise in y, and goes to the accumulators by global atomics otherwise.
"""
import numpy as np

import _bin_oracle as B
from _median_cases import Case

# The tile constants of auromat_amd/csrc/amt_bin_tile.h and kSelTile of amt_mosaic_plan.h, by the sources' names;
# test_bin_cases_cpu.py reads them from the sources and compares.
K_PPT = 4
K_BW = 256
K_BH = 4
K_ROW_ITERS = 4
K_WX = 32
K_WY = 32
K_SEL_TILE = 16
TILE_H = K_BH * K_ROW_ITERS
NONE = -10 ** 6             # "no cell": the pixel gets a NaN latitude

OFFSETS = (-17, -16, -15, -1, 0, 14, 15, 16)
OFFSETS_GLOBAL = (-17, 16)


class BinCase(Case):
    """A Case with what it promises and how its arrays are to lie in device memory: `coord_offset` doubles in front of every
    coordinate array (1: the arrays start 8 bytes into a 16-byte line), `img_offset` elements in front of the image."""

    def __init__(self, *args, **kw):
        self._promise = kw.pop('promise', {})
        self.coord_offset = kw.pop('coord_offset', 0)
        self.img_offset = kw.pop('img_offset', 0)
        Case.__init__(self, *args, **kw)

    def promises(self):
        return dict(self._promise)


def as_bin_case(case, **promise):
    """A median case (tests/_median_cases.py) as it is, with the mean as the expected statistic."""
    out = BinCase(case.name, case.oracle_key, case.lat, case.lon, case.elev, case.img, case.mask, case.xedges, case.yedges,
                  case.height, case.width, min_elevation=case.min_elevation, lon_wrap=case.lon_wrap, uniform=case.uniform,
                  lon_binned=case.lon_binned, promise=promise)
    assert not case.lon_from_mlt
    return out


def paths(case, window=None):
    """The CPU model: dict(path (n) 0 not binned / 1 LDS / 2 global, tile (n), first (tiles) flat index of the tile's first
    binned pixel or -1, anchor_x / anchor_y (tiles) 0-based, dx / dy (n) cell minus anchor)."""
    ix, iy = B.cell_xy(case)
    valid = ix >= 0
    if window is not None:
        x0, y0, wnx, wny = window
        valid &= (ix >= x0) & (ix < x0 + wnx) & (iy >= y0) & (iy < y0 + wny)
    h, w = case.height, case.width
    idx = np.arange(h * w)
    row, col = idx // w, idx % w
    tiles_x = (w + K_BW - 1) // K_BW
    ntiles = tiles_x * ((h + TILE_H - 1) // TILE_H)
    tile = (row // TILE_H) * tiles_x + col // K_BW
    first = np.full(ntiles, h * w, dtype=np.int64)
    np.minimum.at(first, tile[valid], idx[valid])       # pixels of one tile: row-major order is the order of the flat index
    has = first < h * w
    at = np.minimum(first, h * w - 1)
    ax, ay = np.where(has, ix[at], NONE), np.where(has, iy[at], NONE)
    dx, dy = ix - ax[tile], iy - ay[tile]
    lds = valid & (dx >= -(K_WX // 2)) & (dx < K_WX // 2) & (dy >= -(K_WY // 2)) & (dy < K_WY // 2)
    return dict(path=np.where(valid, np.where(lds, 1, 2), 0), tile=tile, first=np.where(has, first, -1), anchor_x=ax,
                anchor_y=ay, dx=dx, dy=dy)


def path_counts(case, window=None):
    """(pixels through LDS, pixels by the global path)"""
    p = paths(case, window)['path']
    return int((p == 1).sum()), int((p == 2).sum())


def unit_edges(n):
    return np.arange(n + 1, dtype=np.float64)


def unit_frame(name, key, ix, iy, height, width, nx, ny, dtype, nch, rng, elev=None, img=None, with_elev=True, **kw):
    """Pixel i in cell (ix[i], iy[i]) of an nx x ny grid of unit cells (NONE: NaN latitude; other values outside 0..n-1 lie
    outside the edges); random elevations in -89.9 .. 89.999 and a random image unless given."""
    dtype = np.dtype(dtype)
    n = height * width
    ix, iy = np.asarray(ix).reshape(n), np.asarray(iy).reshape(n)
    none = (ix == NONE) | (iy == NONE)
    lat = np.where(none, np.nan, iy + 0.5)
    lon = ix + 0.5
    if elev is None and with_elev:
        elev = rng.uniform(-89.9, 89.999, n)
    if elev is not None:
        elev = np.where(none, np.nan, elev)
    if img is None:
        img = rng.randint(0, int(np.iinfo(dtype).max) + 1, (n, nch)).astype(dtype)
    assert img.shape == (n, nch) and img.dtype == dtype
    return BinCase(name, key, lat, lon, elev, img, None, unit_edges(nx), unit_edges(ny), height, width, **kw)


# ---- scatter: nearly every run takes the global path -------------------------------------------------------------------
SCATTER_GRID = (700, 600)       # nx, ny
SCATTER_SIZE = (96, 512)
SCATTER_VARIANTS = ('plain', 'wrap', 'alternate')


def scatter(dtype, variant='plain', nch=3):
    from oracle import ref_numpy as O
    dtype = np.dtype(dtype)
    nx, ny = SCATTER_GRID
    h, w = SCATTER_SIZE
    n = h * w
    rng = np.random.RandomState(101 + SCATTER_VARIANTS.index(variant))
    ix, iy = rng.randint(0, nx, n), rng.randint(0, ny, n)
    name, key = 'scatter-%s-%s-%d' % (dtype.name, variant, nch), ('scatter', dtype.name, variant, nch)
    promise = dict(min_global_share=0.9)
    if variant == 'alternate':
        # x-neighbours alternate between two far groups of cells: every run of a thread has length 1
        even = (np.arange(n) % w) % 2 == 0
        ix = np.where(even, 10 + rng.randint(0, 3, n), 600 + rng.randint(0, 3, n))
        iy = np.where(even, 20 + rng.randint(0, 3, n), 500 + rng.randint(0, 3, n))
        promise = dict(min_global_share=0.45, run_length=1)
    iy[::211] = NONE
    if variant != 'wrap':
        return unit_frame(name, key, ix, iy, h, w, nx, ny, dtype, nch, rng, promise=promise)
    case = unit_frame(name, key, ix, iy, h, w, nx, ny, dtype, nch, rng)
    xedges = np.linspace(-180.0, 180.0, nx + 1)
    lon = rng.uniform(-360.0, 360.0, n)
    return BinCase(name, key, case.lat, lon, case.elev, case.img, None, xedges, case.yedges, h, w, lon_wrap=1,
                   lon_binned=O.wrap_at(lon + 180, 180), promise=promise)


# ---- window_border: pixels at chosen offsets from the tile's anchor -------------------------------------------------------
WINDOW_BORDER = {           # kind: (nx, ny, anchors (0-based cells), axes the offsets go along)
    'x': (64, 64, ((30, 30), (17, 40), (40, 17), (31, 32)), 'x'),
    'y': (64, 64, ((30, 30), (17, 40), (40, 17), (31, 32)), 'y'),
    'both': (64, 64, ((30, 30), (17, 40), (40, 17), (31, 32)), 'xy'),
    'first': (64, 64, ((0, 0),), 'xy'),             # the anchor in cell 1: the window starts at a negative cell
    'last': (64, 64, ((63, 63),), 'xy'),
    '1x1': (1, 1, ((0, 0),), 'xy'),                 # a grid smaller than the window
    '3bin': (3, 64, ((1, 30), (0, 0), (2, 63)), 'xy'),
}


def window_border(kind, dtype=np.uint8, nch=1):
    """One tile per anchor: the tile's first pixel in the anchor cell, pixel k of the tile at anchor + OFFSETS[k % 8] in x
    and / or anchor + OFFSETS[(k // 8) % 8] in y.  Every combination occurs, the last LDS slot (+15, +15) included."""
    nx, ny, anchors, axes = WINDOW_BORDER[kind]
    dtype = np.dtype(dtype)
    h, w = TILE_H * len(anchors), K_BW
    k = np.arange(TILE_H * K_BW)
    off = np.array(OFFSETS)
    ox = off[k % 8] if 'x' in axes else np.zeros(k.size, dtype=np.int64)
    oy = (off[(k // 8) % 8] if 'x' in axes else off[k % 8]) if 'y' in axes else np.zeros(k.size, dtype=np.int64)
    ox[0] = oy[0] = 0
    ix = np.concatenate([a[0] + ox for a in anchors])
    iy = np.concatenate([a[1] + oy for a in anchors])
    rng = np.random.RandomState(7 + sorted(WINDOW_BORDER).index(kind))
    return unit_frame('window-border-%s-%s-%d' % (kind, dtype.name, nch), ('window-border', kind, dtype.name, nch), ix, iy, h,
                      w, nx, ny, dtype, nch, rng, promise=dict(anchors=anchors, axes=axes, lds_offsets=tuple(
                          o for o in OFFSETS if o not in OFFSETS_GLOBAL), global_offsets=OFFSETS_GLOBAL))


# ---- wide_axis: more than 32 767 bins ------------------------------------------------------------------------------------
WIDE_AXES = ((40000, 3), (65534, 3), (3, 40000), (3, 65534))        # nx, ny
WIDE_SIZE = (64, 512)           # 8 tiles


def wide_axis(nx, ny, dtype=np.uint8, nch=3):
    """Eight tiles whose anchors lie at both ends of the long axis, just below, on and above bin 32 768 (1-based; the packed
    anchor turns negative there) and in between; half of a tile's pixels within 20 cells of its anchor, half anywhere."""
    dtype = np.dtype(dtype)
    h, w = WIDE_SIZE
    long_n = max(nx, ny)
    anchors = (5, 32766, 32767, 32768, 32790, long_n - 1, 20000, long_n - 7)
    rng = np.random.RandomState(long_n + (0 if nx > ny else 1))
    idx = np.arange(h * w)
    tile = (idx // w // TILE_H) * (w // K_BW) + (idx % w) // K_BW
    a = np.array(anchors)[tile]
    near = a + rng.randint(-20, 21, h * w)
    far = rng.randint(0, long_n, h * w)
    along = np.where(rng.uniform(size=h * w) < 0.5, near, far)
    first = np.unique(tile, return_index=True)[1]
    along[first] = np.array(anchors)
    across = rng.randint(0, 3, h * w)
    ix, iy = (along, across) if nx > ny else (across, along)
    # (two of the four take the uniform axis, whose bins the kernel computes, two the edge table it bisects)
    return unit_frame('wide-axis-%dx%d' % (nx, ny), ('wide-axis', nx, ny, dtype.name, nch), ix, iy, h, w, nx, ny, dtype, nch, rng,
                      uniform=(nx, ny) in ((65534, 3), (3, 40000)), promise=dict(anchors=anchors, tiles=8))


# ---- late_anchor: the election ------------------------------------------------------------------------------------------
LATE_PATTERNS = ('row3', 'none', 'rows4-7', 'none', 'rows8-11', 'lastcol', 'none', 'rows12-15', 'none', 'none', 'lastcol',
                 'row3')
LATE_SIZE = (4 * TILE_H, 3 * K_BW)


def late_anchor(dtype=np.uint16, nch=2):
    """Twelve tiles; a tile's only valid pixels lie in row 3 (the last wave of the first row group), in a later row group,
    or in its last column; whole tiles of NaN latitude between them.  A valid pixel sits near the tile's own block of cells
    or (one in five) far from it."""
    dtype = np.dtype(dtype)
    h, w = LATE_SIZE
    nx, ny = 120, 90
    rng = np.random.RandomState(41)
    idx = np.arange(h * w)
    row, col = idx // w, idx % w
    tile = (row // TILE_H) * 3 + col // K_BW
    r, c = row % TILE_H, col % K_BW
    which = np.array(LATE_PATTERNS)[tile]
    valid = ((which == 'row3') & (r == 3)) | ((which == 'rows4-7') & (r >= 4) & (r < 8)) | \
            ((which == 'rows8-11') & (r >= 8) & (r < 12)) | ((which == 'rows12-15') & (r >= 12)) | \
            ((which == 'lastcol') & (c == K_BW - 1))
    far = rng.uniform(size=h * w) < 0.2
    ix = np.where(far, rng.randint(0, nx, h * w), 8 * tile + c // 64)
    iy = np.where(far, rng.randint(0, ny, h * w), 5 * tile + r // 4)
    ix = np.where(valid, ix, NONE)
    return unit_frame('late-anchor', ('late-anchor', dtype.name, nch), ix, iy, h, w, nx, ny, dtype, nch, rng,
                      promise=dict(patterns=LATE_PATTERNS))


# ---- sizes: tile tails ----------------------------------------------------------------------------------------------------
SIZE_WIDTHS = (1, 2, 3, 255, 256, 257, 511, 513)
SIZE_HEIGHTS = (1, 15, 16, 17)
SIZE_GRID = (40, 37)
SIZE_LAYOUTS = ('aligned', 'coords8', 'img1')


def sizes(height, width, layout='aligned'):
    """Every pixel in a random cell of a 40 x 37 grid (both paths).  Channels and type by the size; layout 'coords8': every
    coordinate array starts 8 bytes into its allocation, 'img1': the image starts one element into its allocation and has
    a channel count whose pixel pairs are whole words."""
    assert layout in SIZE_LAYOUTS
    nx, ny = SIZE_GRID
    rng = np.random.RandomState(height * 1009 + width)
    u16 = (width // 2 + height) % 2 == 1
    nch = (width + height) % 5
    if layout == 'img1':
        nch = 1 + (width // 2 + height // 2) % 4 if u16 else 2 + 2 * (height % 2)
    n = height * width
    ix, iy = rng.randint(0, nx, n), rng.randint(0, ny, n)
    if n > 4:
        iy[3::29] = NONE
    return unit_frame('sizes-%dx%d-%s' % (height, width, layout), ('sizes', height, width, layout), ix, iy, height, width, nx,
                      ny, np.uint16 if u16 else np.uint8, nch, rng, coord_offset=int(layout == 'coords8'),
                      img_offset=int(layout == 'img1'), promise=dict(vec=width % 2 == 0 and layout == 'aligned'))


# ---- channels: the packed-word decode ---------------------------------------------------------------------------------------
CHANNEL_WIDTHS = (258, 257)


def channel_image(dtype, nch, n_pixels):
    """Pixel value as a function of (pixel index, channel): byte p of pixel pair q is (16 p + 3 q + 1) mod 256, so the up to
    16 bytes of a pair are all distinct."""
    dtype = np.dtype(dtype)
    sz = dtype.itemsize
    i = np.arange(n_pixels)[:, None, None]
    ch = np.arange(nch)[None, :, None]
    b = np.arange(sz)[None, None, :]
    p = (i % 2) * nch * sz + ch * sz + b
    byte = ((16 * p + 3 * (i // 2) + 1) % 256).astype(np.uint8)
    return np.ascontiguousarray(byte).reshape(n_pixels, nch * sz).view(dtype).reshape(n_pixels, nch)


def channels(dtype, nch, width):
    """Two rows, one pixel per cell: cell (c, r) holds pixel (r, c) alone — a swapped pixel, channel or byte changes a cell."""
    dtype = np.dtype(dtype)
    h = 2
    n = h * width
    rng = np.random.RandomState(width + nch)
    idx = np.arange(n)
    return unit_frame('channels-%s-%d-%d' % (dtype.name, nch, width), ('channels', dtype.name, nch, width), idx % width,
                      idx // width, h, width, width, h, dtype, nch, rng, img=channel_image(dtype, nch, n),
                      promise=dict(pixels_per_cell=1, vec=width % 2 == 0))


# ---- heavy_cell -------------------------------------------------------------------------------------------------------------
HEAVY_SIZE = (2048, 2048)
HEAVY_KINDS = ('max', 'elev-high', 'elev-low')


def heavy_cell(kind, split):
    """2048 x 2048 pixels in one cell, or split over two (pixel pairs alternate).  'max': uint16, 3 channels, all 65 535;
    'elev-high': every elevation 89.999; 'elev-low': every elevation -89.9 (negative sums carried through unsigned atomics).

    The signed 31.32 sum holds 2**63 / (90 * 2**32) = 2.38e7 pixels of 90 deg in one cell; these cases stay below it:
    4.19e6 * 89.999 * 2**32 = 1.62e18 < 2**63 = 9.22e18.  The largest channel sum is 4.19e6 * 65 535 = 2.75e11, past 2**32 and
    below 2**53; one tile's LDS sum is at most 4096 * 65 535 = 2.7e8 < 2**32."""
    assert kind in HEAVY_KINDS
    h, w = HEAVY_SIZE
    n = h * w
    rng = np.random.RandomState(HEAVY_KINDS.index(kind) * 2 + int(split))
    ix = (np.arange(n) // 2) % 2 if split else np.zeros(n, dtype=np.int64)
    if kind == 'max':
        dtype, nch = np.dtype(np.uint16), 3
        img, elev = np.full((n, 3), 65535, dtype=np.uint16), rng.uniform(-89.9, 89.999, n)
    else:
        dtype, nch = np.dtype(np.uint8), 1
        img, elev = rng.randint(0, 256, (n, 1)).astype(np.uint8), np.full(n, 89.999 if kind == 'elev-high' else -89.9)
    assert n * 89.999 * 2.0 ** 32 < 2.0 ** 63
    return unit_frame('heavy-cell-%s-%s' % (kind, 'two' if split else 'one'), ('heavy-cell', kind, bool(split)), ix,
                      np.zeros(n, dtype=np.int64), h, w, 2 if split else 1, 1, dtype, nch, rng, elev=elev, img=img,
                      promise=dict(pixels=n, cells=2 if split else 1))


# ---- half_means ---------------------------------------------------------------------------------------------------------------
HALF_LARGE = 65536


def half_means(dtype):
    """Cells of two pixels (k, k + 1) and of four (k, k, k + 1, k + 1): mean exactly k + 0.5, for k = 0, 1, 254 and for
    uint16 also 65 534; cells of all-maximum pixels; and cells of HALF_LARGE pixels whose sum is one unit below, on and
    above HALF_LARGE * (k + 0.5) (no pixel count within reach puts a mean at the double next to a half: one unit of the sum
    is the closest a cell gets).  One cell per column of a 1-row grid; two channels: the pattern v and its mirror max - v
    (means 254.5 and 65 534.5 from k = 0)."""
    dtype = np.dtype(dtype)
    hi = int(np.iinfo(dtype).max)
    ks = [0, 1, 254] + ([65534] if hi > 255 else [])
    cells = []                                                  # per cell: values of channel 0
    for k in ks:
        cells.append([k, k + 1])
        cells.append([k + 1, k, k, k + 1])
    cells.append([hi] * 5)
    exact = len(cells) - 1
    for k in ks:
        for d in (-1, 0, 1):
            v = np.full(HALF_LARGE, k, dtype=np.int64)
            v[:HALF_LARGE // 2 + d] = k + 1
            cells.append(v)
    rng = np.random.RandomState(hi)
    vals = np.concatenate([rng.permutation(np.asarray(c, dtype=np.int64)) for c in cells])
    cell = np.concatenate([np.full(len(c), j) for j, c in enumerate(cells)])
    p = rng.permutation(vals.size)
    vals, cell = vals[p], cell[p]
    w = 1021
    h = (vals.size + w - 1) // w
    pad = h * w - vals.size
    vals = np.concatenate([vals, np.zeros(pad, dtype=np.int64)])
    cell = np.concatenate([cell, np.full(pad, NONE)])
    img = np.stack([vals, np.where(cell == NONE, 0, hi - vals)], axis=1).astype(dtype)
    return unit_frame('half-means-%s' % dtype.name, ('half-means', dtype.name), cell, np.where(cell == NONE, NONE, 0), h, w,
                      len(cells), 1, dtype, 2, rng, img=img, promise=dict(ks=tuple(ks), exact_half_cells=exact,
                                                                          large=HALF_LARGE, cells=len(cells)))


# ---- finalize_window ------------------------------------------------------------------------------------------------------------
FINALIZE_ACC = (50, 37)             # acc_nx, acc_ny
FINALIZE_WINDOW = (7, 3, 20, 11)    # off_x, off_y, nx, ny: non-zero, unequal offsets, nx != ny


def finalize_window(dtype, nch=3):
    """A frame binned on a 50 x 37 grid, to be finalised through FINALIZE_WINDOW and compared with the crop of the whole."""
    dtype = np.dtype(dtype)
    nx, ny = FINALIZE_ACC
    h, w = 33, 514
    rng = np.random.RandomState(59)
    ix, iy = rng.randint(-1, nx + 1, h * w), rng.randint(-1, ny + 1, h * w)
    return unit_frame('finalize-window-%s-%d' % (dtype.name, nch), ('finalize-window', dtype.name, nch), ix, iy, h, w, nx, ny,
                      dtype, nch, rng, promise=dict(window=FINALIZE_WINDOW))


def crop(plane, window, ny):
    """The window (off_x, off_y, nx, ny in cells, y ascending) of an output-layout plane (rows north to south)."""
    x0, y0, wnx, wny = window
    return plane[ny - y0 - wny:ny - y0, x0:x0 + wnx]


# ---- mosaics --------------------------------------------------------------------------------------------------------------------
class Mosaic(object):
    def __init__(self, name, members, windows, promise=None):
        assert len(members) == len(windows)
        self.name, self.members, self.windows, self._promise = name, members, [tuple(w) for w in windows], promise or {}

    def promises(self):
        return dict(self._promise)

    @property
    def shape(self):
        return self.members[0].shape

    def reversed(self):
        return Mosaic(self.name + '-reversed', self.members[::-1], self.windows[::-1], self._promise)


def _member(name, rng, h, w, nx, ny, dtype, nch, min_elevation, ix=None, iy=None, elev=None, img=None):
    n = h * w
    ix = rng.randint(0, nx, n) if ix is None else ix
    iy = rng.randint(0, ny, n) if iy is None else iy
    return unit_frame(name, (name,), ix, iy, h, w, nx, ny, dtype, nch, rng, elev=elev, img=img, min_elevation=min_elevation)


MOSAIC_GRID = (48, 40)
# borders at multiples of K_SEL_TILE and one before / after; members 0 and 1 overlap in the strip x = 16, one cell wide
MOSAIC_WINDOWS = ((0, 0, 17, 16), (16, 0, 16, 33), (15, 17, 33, 23))


def mosaic_windows(dtype, nch, min_elevation=-np.inf):
    nx, ny = MOSAIC_GRID
    rng = np.random.RandomState(61)
    members = [_member('mosaic-windows-m%d' % i, rng, 40 + i, 300 + 2 * i, nx, ny, dtype, nch, min_elevation) for i in range(3)]
    return Mosaic('mosaic-windows-%s-%d' % (np.dtype(dtype).name, nch), members, MOSAIC_WINDOWS,
                  dict(strip=(16, 17, 0, 16)))


def mosaic_empty_first_and_middle(dtype, nch, min_elevation=-np.inf):
    """Five members; member 0 has a 0 x 0 window and member 2 a 0-wide one: equal entries at the start and in the middle of
    the tile prefix."""
    nx, ny = MOSAIC_GRID
    rng = np.random.RandomState(67)
    members = [_member('mosaic-empty-m%d' % i, rng, 17 + 16 * i, 258 - 2 * i, nx, ny, dtype, nch, min_elevation) for i in range(5)]
    windows = ((0, 0, 0, 0), (0, 0, 30, 25), (5, 5, 0, 9), (10, 8, 38, 32), (20, 0, 20, 40))
    return Mosaic('mosaic-empty-%s-%d' % (np.dtype(dtype).name, nch), members, windows, dict(empty=(0, 2)))


MANY_GRID = (80, 70)
MANY_SCATTERED = 7


def mosaic_many(dtype, nch, min_elevation=-np.inf, all_even=False):
    """Forty small members of different sizes with random windows; member 13 has an odd width unless `all_even` (one odd
    member sends the whole launch down the scalar path); member MANY_SCATTERED has the whole grid as its window and pixels
    all over it, so its tiles take the global path of the windowed kernel."""
    nx, ny = MANY_GRID
    rng = np.random.RandomState(71)
    members, windows = [], []
    for i in range(40):
        h, w = 1 + (7 * i) % 20, 2 * (3 + i) + (1 if i == 13 and not all_even else 0)
        if i == MANY_SCATTERED:
            h, w = 40, 256
            windows.append((0, 0, nx, ny))
        else:
            x0, y0 = rng.randint(0, nx - 1), rng.randint(0, ny - 1)
            windows.append((x0, y0, rng.randint(1, min(30, nx - x0) + 1), rng.randint(1, min(30, ny - y0) + 1)))
        x0, y0, wnx, wny = windows[-1]
        n = h * w
        # pixels in and round the member's window
        ix, iy = rng.randint(x0 - 2, x0 + wnx + 2, n), rng.randint(y0 - 2, y0 + wny + 2, n)
        members.append(_member('mosaic-many-m%d' % i, rng, h, w, nx, ny, dtype, nch, min_elevation, ix=ix, iy=iy))
    return Mosaic('mosaic-many-%s-%d-%s' % (np.dtype(dtype).name, nch, 'even' if all_even else 'odd'), members, windows,
                  dict(members=40, odd_widths=0 if all_even else 1, scattered=MANY_SCATTERED))


TIES_THRESHOLD = 10.0
U = 2.0 ** -32                      # one unit of the fixed-point sum
# per cell and member the elevations of its pixels; rule 1's winner
TIES = (
    ((10.0,), (10.0,), ()),                                 # equal fx and count                      -> member 0
    ((10.0,), (10.0 + U,), ()),                             # a later member ahead by one unit of fx  -> member 1
    ((12.5,), (12.5, 12.5), ()),                            # equal mean from (fx, c) and (2 fx, 2 c) -> member 0
    ((20.0, 20.0 + U), (20.0, 20.0), (20.0 + U, 20.0 + U)),  # 2 fx + 1, 2 fx, 2 fx + 2              -> member 2
    ((), (), (33.0,)),                                      # one member alone                        -> member 2
    ((), (15.0, 15.0 + 2 * U), (15.0 + U, 15.0 + U)),       # equal fx from different samples         -> member 1
    ((40.0 + U,), (40.0,), (40.0 + U,)),                    # first and last equal, middle one below  -> member 0
)
TIES_WINNERS = (0, 1, 0, 2, 2, 1, 0)


def mosaic_ties(dtype, nch, min_elevation=-np.inf):
    """Three members on a 7 x 1 grid, whole-grid windows; every elevation is a multiple of 2**-32, so fx is the exact sum.
    min_elevation, where given, is TIES_THRESHOLD: equal to the lowest elevation, which stays in."""
    dtype = np.dtype(dtype)
    nx = len(TIES)
    rng = np.random.RandomState(73)
    members = []
    for m in range(3):
        ix = np.concatenate([np.full(len(cell[m]), c, dtype=np.int64) for c, cell in enumerate(TIES)])
        elev = np.concatenate([np.asarray(cell[m], dtype=np.float64) for cell in TIES])
        pad = (-ix.size) % 2
        ix = np.concatenate([ix, np.full(pad, NONE)])
        elev = np.concatenate([elev, np.zeros(pad)])
        img = np.full((ix.size, nch), (m + 1) * 50, dtype=dtype) + np.arange(ix.size)[:, None].astype(dtype)
        members.append(_member('mosaic-ties-m%d' % m, rng, 1, ix.size, nx, 1, dtype, nch, min_elevation, ix=ix,
                               iy=np.where(ix == NONE, NONE, 0), elev=elev, img=img))
    return Mosaic('mosaic-ties-%s-%d' % (dtype.name, nch), members, [(0, 0, nx, 1)] * 3, dict(winners=TIES_WINNERS))


MOSAIC_CASES = dict(windows=mosaic_windows, empty=mosaic_empty_first_and_middle, many=mosaic_many,
                    many_even=lambda d, n, e=-np.inf: mosaic_many(d, n, e, all_even=True), ties=mosaic_ties)


# ---- hist_points ------------------------------------------------------------------------------------------------------------------
HIST_N = 1300000                    # more than 256 * 16 * 256 points: the grid-stride loop of k_hist2d comes round
HIST_GRID = (50, 40)


def hist_points(nweights, kind, n=HIST_N):
    """dict(x, y, weights (list of nweights arrays), xedges, yedges); kind 'integer' (weights 0..1000) or 'real'."""
    nx, ny = HIST_GRID
    rng = np.random.RandomState(83 + nweights)
    x, y = rng.uniform(-1.0, nx + 1.0, n), rng.uniform(-1.0, ny + 1.0, n)
    x[::1009] = np.nan
    if kind == 'integer':
        weights = [rng.randint(0, 1001, n).astype(np.float64) for _ in range(nweights)]
    else:
        weights = [rng.normal(0, 10.0 ** k, n) for k in range(nweights)]
    return dict(x=x, y=y, weights=weights, xedges=unit_edges(nx), yedges=unit_edges(ny))
