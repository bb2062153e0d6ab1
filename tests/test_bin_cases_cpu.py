"""The constructed cases of the mean-binning tests (tests/_bin_cases.py) without a GPU: every case holds what it promises —
how many of its pixels the tile body sums in LDS and how many go by global atomics (the CPU model K.paths, with the tile
constants read from the sources), which offsets from the anchor occur, where the anchors lie — and the integer oracle
(tests/_bin_oracle.py) agrees with the histogram2d-based means of tests/_mosaic_oracle.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _bin_cases as K
import _bin_oracle as B
import _median_cases as MC
import _mosaic_oracle as MO

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'auromat_amd', 'csrc')


def test_case_constants_are_the_sources():
    tile = open(os.path.join(CSRC, 'amt_bin_tile.h')).read()
    mosaic = open(os.path.join(CSRC, 'amt_mosaic_plan.h')).read() + open(os.path.join(CSRC, 'amt_mosaic.hip')).read()
    assert re.findall(r'constexpr int kBinBlock = (\d+);', tile) == ['256']
    assert re.findall(r'constexpr int kPPT = (\d+);', tile) == [str(K.K_PPT)]
    assert re.findall(r'constexpr int kBW = 64 \* kPPT, kBH = kBinBlock / 64, kWCap = (\d+);', tile) == [str(K.K_WX * K.K_WY)]
    assert (K.K_BW, K.K_BH) == (64 * K.K_PPT, 256 // 64)
    assert re.findall(r'constexpr int kWX = (\d+), kWY = (\d+);', tile) == [(str(K.K_WX), str(K.K_WY))]
    assert re.findall(r'constexpr int kRowIters = (\d+);', tile) == [str(K.K_ROW_ITERS)]
    assert re.findall(r'constexpr int kSelTile = (\d+);', mosaic) == [str(K.K_SEL_TILE)]
    assert K.TILE_H == 16 and K.OFFSETS == (-K.K_WX // 2 - 1, -K.K_WX // 2, -K.K_WX // 2 + 1, -1, 0, K.K_WX // 2 - 2,
                                            K.K_WX // 2 - 1, K.K_WX // 2)
    # the fixed-point scale and the rounding of the elevation sum
    assert 'constexpr double kFix = 4294967296.0;' in open(os.path.join(CSRC, 'amt_common.h')).read()


def test_the_model_on_a_hand_made_tile():
    # 2 tiles of 256 x 16 side by side; tile 0: first valid pixel is (row 2, column 5) -> cell (40, 40); tile 1 has none
    h, w = 16, 512
    ix = np.full(h * w, K.NONE)
    iy = np.full(h * w, K.NONE)
    for (r, c), cell in {(2, 5): (40, 40), (2, 6): (24, 40), (2, 7): (23, 40), (9, 200): (55, 55), (9, 201): (56, 55),
                         (15, 255): (40, 56), (1, 300): (70, 0)}.items():
        ix[r * w + c], iy[r * w + c] = cell
    iy[1 * w + 300] = 99                # outside the grid: not a candidate for tile 1's anchor
    case = K.unit_frame('hand', ('hand',), ix, iy, h, w, 80, 80, np.uint8, 1, np.random.RandomState(0))
    p = K.paths(case)
    assert p['first'].tolist() == [2 * w + 5, -1] and (p['anchor_x'][0], p['anchor_y'][0]) == (40, 40)
    path = p['path'].reshape(h, w)
    assert [int(path[r, c]) for r, c in ((2, 5), (2, 6), (2, 7), (9, 200), (9, 201), (15, 255), (1, 300))] == \
        [1, 1, 2, 1, 2, 2, 0]
    assert K.path_counts(case) == (3, 3)


# ---- the reused median cases: everything in LDS, which is why they were not enough -----------------------------------------
@pytest.mark.parametrize('coord', ['plain', 'wrap'])
@pytest.mark.parametrize('axis', ['uniform', 'nonuniform'])
def test_membership_cases_never_leave_the_window(axis, coord):
    for mode in ('nothreshold', 'threshold', 'nomask'):
        case = MC.membership(np.uint8, axis, mode, coord)
        lds, glob = K.path_counts(case)
        assert lds > 5000 and glob == 0
        assert max(case.shape) <= K.K_WX // 2


def test_tails_and_the_large_cell_never_leave_the_window():
    for size in MC.TAIL_SIZES:
        for ncell in MC.TAIL_CELLS:
            case = MC.tails(np.uint8, size[0], size[1], ncell)
            assert K.path_counts(case) == (size[0] * size[1], 0)
    assert K.path_counts(MC.one_large_cell(np.uint8)) == (MC.HUGE, 0)


@pytest.mark.parametrize('order', MC.ORDERS)
def test_tier_table_paths(order):
    # 22 x 6 cells, the heavy ones in the last columns: a pixel leaves the window only when it lies 16 or more columns right
    # of its tile's anchor, and nearly every anchor is a heavy cell.  Two pixels in a thousand at most, never by the rows.
    case = MC.tier_table(np.uint8, 3, True, order)
    lds, glob = K.path_counts(case)
    assert lds + glob == int(MC.table_counts().sum())
    assert glob <= 0.002 * lds
    p = K.paths(case)
    assert (np.abs(p['dy'][p['path'] == 2]) < K.K_WY // 2).all()


# ---- the new cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', K.SCATTER_VARIANTS)
def test_scatter_takes_the_global_path(variant):
    case = K.scatter(np.uint8, variant)
    lds, glob = K.path_counts(case)
    promise = case.promises()
    assert lds > 0 and glob >= promise['min_global_share'] * (lds + glob), (lds, glob)
    assert lds + glob > 48000
    if variant == 'alternate':
        ix, iy = B.cell_xy(case)
        ix, iy = ix.reshape(case.height, case.width), iy.reshape(case.height, case.width)
        same = (ix[:, 1:] == ix[:, :-1]) & (iy[:, 1:] == iy[:, :-1]) & (ix[:, 1:] >= 0)
        assert not same.any()                                       # every run has length 1
    if variant == 'wrap':
        assert case.lon_wrap == 1 and (np.abs(case.lon) > 180).sum() > 10000


@pytest.mark.parametrize('kind', sorted(K.WINDOW_BORDER))
def test_window_border_offsets(kind):
    case = K.window_border(kind)
    nx, ny, anchors, axes = K.WINDOW_BORDER[kind]
    promise = case.promises()
    p = K.paths(case)
    assert list(zip(p['anchor_x'].tolist(), p['anchor_y'].tolist())) == [tuple(a) for a in anchors]
    binned = p['path'] > 0
    dx, dy, path = p['dx'][binned], p['dy'][binned], p['path'][binned]
    out = np.isin(dx, promise['global_offsets']) | np.isin(dy, promise['global_offsets'])
    assert np.array_equal(path == 2, out)                           # exactly the listed offsets on the stated side
    assert set(np.unique(dx)) <= set(K.OFFSETS) and set(np.unique(dy)) <= set(K.OFFSETS)
    if kind in ('x', 'y', 'both'):
        # every offset occurs in every tile, inside the grid
        for t in range(len(anchors)):
            here = binned & (p['tile'] == t)
            if 'x' in axes:
                assert set(np.unique(p['dx'][here])) == set(K.OFFSETS)
            if 'y' in axes:
                assert set(np.unique(p['dy'][here])) == set(K.OFFSETS)
        if kind == 'both':
            for a in (-16, 15):
                for b in (-16, 15):
                    assert ((dx == a) & (dy == b) & (path == 1)).any()      # the four corner slots, (+15, +15) included
            assert ((dx == 16) & (dy == 16)).any() and ((dx == -17) & (dy == 15)).any()
    if kind == 'first':
        assert dx.min() == 0 and dy.min() == 0 and (path == 2).any() and ((dx == 15) & (dy == 15)).any()
    if kind == 'last':
        assert dx.max() == 0 and dy.max() == 0 and (path == 2).any() and ((dx == -16) & (dy == -16)).any()
    if kind == '1x1':
        assert (path == 1).all() and path.size > 60
    if kind == '3bin':
        assert set(np.unique(dx)) == {-1, 0} and (path == 2).any()


@pytest.mark.parametrize('nx,ny', K.WIDE_AXES)
def test_wide_axis_straddles_bin_32768(nx, ny):
    case = K.wide_axis(nx, ny)
    assert (case.img.shape[1] + 2) * nx * ny * 8 < 10e6             # accumulator bytes
    p = K.paths(case)
    anchors = p['anchor_x'] if nx > ny else p['anchor_y']
    assert anchors.tolist() == list(case.promises()['anchors']) and (p['first'] >= 0).all()      # every tile contributes
    one_based = anchors + 1
    assert (one_based < 32768).sum() >= 2 and (one_based == 32768).sum() == 1 and (one_based > 32768).sum() >= 3
    assert max(nx, ny) in one_based                                 # the last cell
    ix, iy = B.cell_xy(case)
    along = (ix if nx > ny else iy)[p['path'] > 0] + 1
    for path in (1, 2):
        sel = along[p['path'][p['path'] > 0] == path]
        assert (sel < 32768).sum() > 1000 and (sel >= 32768).sum() > 1000
    # the packed candidate of the election is never 0 (a lost tile): only cell (65535, 65535) packs to it
    packed = (((ix + 1) & 0xffff) << 16 | ((iy + 1) & 0xffff)) + 1
    assert (packed[p['path'] > 0] & 0xffffffff != 0).all()


def test_late_anchor_row_groups():
    case = K.late_anchor()
    p = K.paths(case)
    w = case.width
    for t, pattern in enumerate(K.LATE_PATTERNS):
        first = int(p['first'][t])
        if pattern == 'none':
            assert first == -1 and not (p['path'][p['tile'] == t] > 0).any()
            continue
        r, c = (first // w) % K.TILE_H, (first % w) % K.K_BW
        assert (p['path'][p['tile'] == t] == 1).any()
        if pattern == 'row3':
            assert r == 3                                           # the last wave of the first row group
        elif pattern == 'lastcol':
            assert c == K.K_BW - 1
        else:
            lo = int(pattern[4:].split('-')[0])
            assert r == lo and lo // K.K_BH in (1, 2, 3)            # elected in a later row group
    assert (p['path'] == 2).sum() > 100
    # tiles without a valid pixel between tiles that have some
    has = p['first'] >= 0
    assert (~has[1:-1] & has[:-2] & has[2:]).any()


@pytest.mark.parametrize('height', K.SIZE_HEIGHTS)
@pytest.mark.parametrize('width', K.SIZE_WIDTHS)
def test_sizes(height, width):
    case = K.sizes(height, width)
    assert case.promises()['vec'] == (width % 2 == 0)
    lds, glob = K.path_counts(case)
    assert lds + glob >= 0.8 * height * width
    if height * width > 500:
        assert lds > 50 and glob > 50
    if width % 2 == 0:
        for layout in ('coords8', 'img1'):
            other = K.sizes(height, width, layout)
            assert (other.coord_offset, other.img_offset) == ((1, 0) if layout == 'coords8' else (0, 1))
            if layout == 'img1':
                nch, size = other.img.shape[1], other.img.dtype.itemsize
                assert (2 * nch * size) % 4 == 0 and (other.img_offset * size) % 4 != 0     # word pairs, misaligned base
    assert {K.sizes(h, 256, 'img1').img.dtype.name for h in K.SIZE_HEIGHTS} == {'uint8', 'uint16'}


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_channels_one_pixel_per_cell_and_distinct_bytes(dtype):
    for nch in range(5):
        for width in K.CHANNEL_WIDTHS:
            case = K.channels(dtype, nch, width)
            count = B.planes(case)['count']
            assert (count == 1).all()
            if nch:
                pairs = K.channel_image(dtype, nch, 64).reshape(-1).view(np.uint8).reshape(32, -1)
                assert pairs.shape[1] == 2 * nch * np.dtype(dtype).itemsize
                assert all(len(set(row)) == len(row) for row in pairs.tolist())
                assert np.array_equal(case.img[:64], K.channel_image(dtype, nch, 64))
            lds, glob = K.path_counts(case)
            assert lds > 0 and glob > 0


@pytest.mark.parametrize('kind', K.HEAVY_KINDS)
def test_heavy_cell_capacity(kind):
    n = K.HEAVY_SIZE[0] * K.HEAVY_SIZE[1]
    assert n * 90.0 * 2.0 ** 32 < 2.0 ** 63 and 2.0 ** 63 / (90 * 2.0 ** 32) > 2.38e7
    assert n * 65535 > 2 ** 32 and n * 65535 < 2 ** 53 and K.K_BW * K.TILE_H * 65535 < 2 ** 32
    if kind == 'max':                    # (the other kinds differ in their elevations only: built in the GPU test)
        case = K.heavy_cell(kind, True)
        p = B.planes(case)
        assert p['count'].tolist() == [[n // 2, n // 2]] and p['sums'].max() == n // 2 * 65535
        assert K.path_counts(case) == (n, 0)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_half_means_in_integers(dtype):
    case = K.half_means(dtype)
    promise = case.promises()
    hi = int(np.iinfo(dtype).max)
    p = B.planes(case)
    count, sums = p['count'][0], p['sums'][0]
    ks = promise['ks']
    assert ks == ((0, 1, 254) + ((65534,) if hi > 255 else ()))
    j = 0
    for k in ks:
        for n in (2, 4):
            assert count[j] == n and 2 * sums[j, 0] == (2 * k + 1) * n and 2 * sums[j, 1] == (2 * (hi - k - 1) + 1) * n
            j += 1
    assert count[j] == 5 and sums[j, 0] == 5 * hi and sums[j, 1] == 0
    j += 1
    for k in ks:
        for d in (-1, 0, 1):
            assert count[j] == promise['large'] and 2 * sums[j, 0] == (2 * k + 1) * promise['large'] + 2 * d
            j += 1
    assert j == promise['cells'] == count.size
    # half to even and half up part on the odd k + 0.5 -> k + 1 cases: both kinds occur
    f = B.finalize(p, dtype)
    exact = [c for c in range(count.size) if 2 * sums[c, 0] % count[c] == 0 and (2 * sums[c, 0] // count[c]) % 2 == 1]
    assert len(exact) == 3 * len(ks)
    assert {int(f['img'][0, c, 0]) - int(sums[c, 0] // count[c]) for c in exact} == {0, 1}


def test_finalize_window_is_a_real_window():
    x0, y0, nx, ny = K.FINALIZE_WINDOW
    acc_nx, acc_ny = K.FINALIZE_ACC
    assert 0 < x0 != y0 > 0 and nx != ny and x0 + nx < acc_nx and y0 + ny < acc_ny
    case = K.finalize_window(np.uint8)
    full = B.frame(case)
    inner = K.crop(full['count'], K.FINALIZE_WINDOW, acc_ny)
    assert inner.shape == (ny, nx) and (inner > 0).all() and full['count'].sum() > inner.sum()
    # the crop against binning through the window directly
    assert np.array_equal(inner, K.crop(B.planes(case, K.FINALIZE_WINDOW)['count'], K.FINALIZE_WINDOW, acc_ny))
    assert B.planes(case, K.FINALIZE_WINDOW)['count'].sum() == inner.sum()


# ---- mosaics ---------------------------------------------------------------------------------------------------------------
def _border_sides(mosaic):
    """Per member and border of its window: (pixels in the cells just inside, just outside) — None where the grid ends."""
    ny, nx = mosaic.shape
    out = []
    for case, (x0, y0, wnx, wny) in zip(mosaic.members, mosaic.windows):
        if wnx == 0 or wny == 0:
            continue
        ix, iy = B.cell_xy(case)
        for v, lo, hi, n in ((ix, x0, x0 + wnx, nx), (iy, y0, y0 + wny, ny)):
            out.append((int((v == lo).sum()), int((v == lo - 1).sum()) if lo > 0 else None))
            out.append((int((v == hi - 1).sum()), int((v == hi).sum()) if hi < n else None))
    return out


def test_mosaic_windows_borders():
    m = K.mosaic_windows(np.uint8, 3)
    t = K.K_SEL_TILE
    borders = sorted({b for x0, y0, nx, ny in m.windows for b in (x0, x0 + nx, y0, y0 + ny)})
    assert {t - 1, t, t + 1, 2 * t, 2 * t + 1, 3 * t} <= set(borders)
    for inside, outside in _border_sides(m):
        assert inside > 0 and (outside is None or outside > 0)
    (ax0, ay0, anx, any_), (bx0, by0, bnx, bny) = m.windows[:2]
    assert (max(ax0, bx0), min(ax0 + anx, bx0 + bnx)) == (16, 17)   # the overlap is one cell wide
    own = B.mosaic(m.members, m.windows, 0)['members']
    both = (own[0]['count'] > 0) & (own[1]['count'] > 0)
    assert both.sum() >= 10 and (np.nonzero(both)[1] == 16).all()


def test_mosaic_empty_members():
    m = K.mosaic_empty_first_and_middle(np.uint8, 3)
    assert [w[2] * w[3] == 0 for w in m.windows] == [True, False, True, False, False]
    assert m.windows[0][2:] == (0, 0) and m.windows[2][2] == 0 and m.windows[2][3] > 0
    out = B.mosaic(m.members, m.windows, 0)
    assert set(np.unique(out['source'])) == {-1, 1, 3, 4}


@pytest.mark.parametrize('all_even', [False, True])
def test_mosaic_many(all_even):
    m = K.mosaic_many(np.uint8, 3, all_even=all_even)
    assert len(m.members) == 40 and len({(c.height, c.width) for c in m.members}) == 40
    assert sum(c.width % 2 for c in m.members) == (0 if all_even else 1)
    lds, glob = K.path_counts(m.members[K.MANY_SCATTERED], m.windows[K.MANY_SCATTERED])
    assert glob > 4 * lds > 0
    for rule in (0, 1):
        assert np.unique(B.mosaic(m.members, m.windows, rule)['source']).size >= 35


def test_mosaic_ties_in_integers():
    m = K.mosaic_ties(np.uint8, 3)
    own = B.mosaic(m.members, m.windows, 1)['members']
    fx = np.array([p['fx'][0] for p in own])
    c = np.array([p['count'][0] for p in own])
    unit = 2 ** 32
    assert (fx[0, 0], c[0, 0]) == (fx[1, 0], c[1, 0]) == (10 * unit, 1) and c[2, 0] == 0
    assert fx[1, 1] - fx[0, 1] == 1 and c[0, 1] == c[1, 1] == 1
    assert (2 * fx[0, 2], 2 * c[0, 2]) == (fx[1, 2], c[1, 2])
    assert fx[:, 3].tolist() == [40 * unit + 1, 40 * unit, 40 * unit + 2] and c[:, 3].tolist() == [2, 2, 2]
    assert c[:, 4].tolist() == [0, 0, 1]
    assert fx[1, 5] == fx[2, 5] and c[1, 5] == c[2, 5] == 2 and c[0, 5] == 0
    assert fx[0, 6] == fx[2, 6] == fx[1, 6] + 1
    for elev_min in (-np.inf, K.TIES_THRESHOLD):
        m = K.mosaic_ties(np.uint8, 3, elev_min)
        assert B.mosaic(m.members, m.windows, 1)['source'].tolist() == [list(K.TIES_WINNERS)]
        assert B.mosaic(m.members, m.windows, 0)['source'].tolist() == [[0, 0, 0, 0, 2, 1, 0]]


def test_hist_points_come_round_the_grid():
    assert K.HIST_N > 256 * 16 * 256
    h = K.hist_points(2, 'integer', n=5000)
    count, sums = B.hist2d(h['x'], h['y'], h['weights'], h['xedges'], h['yedges'])
    assert count.sum() < 5000 and all((bound == 0).all() for _, bound in sums)
    h = K.hist_points(2, 'real', n=5000)
    _, sums = B.hist2d(h['x'], h['y'], h['weights'], h['xedges'], h['yedges'])
    assert all((bound[count > 1] > 0).all() for _, bound in sums)


# ---- every case's pixels on each path, in numbers ---------------------------------------------------------------------------
PATH_COUNTS = {             # case: (pixels summed in LDS, pixels by the global path) of the CPU model; seeded, so fixed
    'scatter-uint8-plain-3': (138, 48781), 'scatter-uint8-wrap-3': (110, 48809), 'scatter-uint8-alternate-3': (24458, 24461),
    'window-border-1x1-uint8-1': (65, 0), 'window-border-3bin-uint8-1': (1475, 448), 'window-border-both-uint8-1': (9220, 7164),
    'window-border-first-uint8-1': (577, 448), 'window-border-last-uint8-1': (1025, 575),
    'window-border-x-uint8-1': (12292, 4092), 'window-border-y-uint8-1': (12292, 4092),
    'wide-axis-40000x3': (10984, 19365), 'wide-axis-65534x3': (10952, 19308), 'wide-axis-3x40000': (11138, 19187),
    'wide-axis-3x65534': (11175, 19118), 'late-anchor': (2949, 667), 'sizes-17x513-aligned': (2220, 6200),
    'sizes-16x256-img1': (945, 3009), 'channels-uint16-4-258': (36, 480), 'channels-uint8-2-257': (34, 480),
    'half-means-uint8': (589847, 0), 'half-means-uint16': (786458, 3), 'finalize-window-uint8-3': (6254, 9240),
    # mosaics: over the members, each inside its window
    'mosaic-empty-uint8-3': (12639, 9351), 'mosaic-many-uint8-3-odd': (11128, 8349), 'mosaic-many-uint8-3-even': (10234, 8727),
    'mosaic-ties-uint8-3': (21, 0), 'mosaic-windows-uint8-3': (7060, 3154),
}


def test_path_counts_in_numbers():
    cases = [K.scatter(np.uint8, v) for v in K.SCATTER_VARIANTS] + [K.window_border(k) for k in sorted(K.WINDOW_BORDER)] + \
        [K.wide_axis(*a) for a in K.WIDE_AXES] + [K.late_anchor(), K.sizes(17, 513), K.sizes(16, 256, 'img1'),
                                                  K.channels(np.uint16, 4, 258), K.channels(np.uint8, 2, 257),
                                                  K.half_means(np.uint8), K.half_means(np.uint16), K.finalize_window(np.uint8)]
    got = {c.name: K.path_counts(c) for c in cases}
    for name in sorted(K.MOSAIC_CASES):
        m = K.MOSAIC_CASES[name](np.uint8, 3)
        parts = [K.path_counts(c, w) for c, w in zip(m.members, m.windows)]
        got[m.name] = (sum(a for a, _ in parts), sum(b for _, b in parts))
    assert got == PATH_COUNTS


# ---- the integer oracle against the histogram2d-based means of _mosaic_oracle.py ---------------------------------------------
def _float_sum_slack(case, window=None):
    """Per output cell the error bound of the other oracle's float64 elevation sum, divided by the count."""
    ny, nx = case.shape
    flat = B.cells(case, window)
    sel = flat >= 0
    n = np.bincount(flat[sel], minlength=nx * ny)
    a = np.bincount(flat[sel], weights=np.abs(case.elev[sel]), minlength=nx * ny)
    return (np.maximum(n - 1, 0) * 2.0 ** -53 * a / np.maximum(n, 1)).reshape(ny, nx)


def _against_histogram2d(members, windows, rule):
    nch = members[0].img.shape[1]
    want = MO.mosaic([(c.lon_binned, c.lat, c.keep(), np.column_stack([c.img.astype(np.float64), np.nan_to_num(c.elev)]), w)
                      for c, w in zip(members, windows)], members[0].xedges, members[0].yedges, rule, nch)
    got = B.mosaic(members, windows, rule)
    assert np.array_equal(got['count'], want['count']) and got['count'].sum() > 0
    assert np.array_equal(got['mean'][..., :nch], want['mean'][..., :nch], equal_nan=True)
    assert np.array_equal(got['img'], want['img'])
    full = got['count'] > 0
    slack = sum(_float_sum_slack(c, w) for c, w in zip(members, windows))
    err = np.abs(got['mean'][..., nch] - want['mean'][..., nch])[full]
    bound = (2.0 ** -33 + 2 * np.spacing(np.abs(want['mean'][..., nch])) + slack)[full]
    assert (err <= bound).all(), (err / bound).max()
    return got, want


@pytest.mark.parametrize('make', [
    lambda: MC.membership(np.uint16, 'uniform', 'threshold', 'plain'), lambda: MC.membership(np.uint8, 'nonuniform', 'nomask', 'wrap'),
    lambda: K.sizes(17, 257), lambda: K.window_border('both'), lambda: K.late_anchor(), lambda: K.finalize_window(np.uint16),
    lambda: K.scatter(np.uint8, 'wrap')], ids=['membership', 'membership-wrap', 'sizes', 'window-border', 'late-anchor',
                                               'finalize-window', 'scatter-wrap'])
def test_oracle_equals_histogram2d_means_on_frames(make):
    case = make()
    whole = (0, 0, case.shape[1], case.shape[0])
    _against_histogram2d([case], [whole], 0)


@pytest.mark.parametrize('rule', [0, 1])
def test_oracle_equals_histogram2d_means_on_mosaics(rule):
    for m in (K.mosaic_windows(np.uint8, 3), K.mosaic_empty_first_and_middle(np.uint16, 3, 0.0)):
        got, want = _against_histogram2d(m.members, m.windows, rule)
        if rule == 0:
            assert np.array_equal(got['source'], want['source'])


def test_the_fixed_point_statement_uses_a_fraction_of_the_exact_bound():
    case = MC.membership(np.uint16, 'uniform', 'threshold', 'plain')
    f = B.frame(case)
    means = B.exact_means(case.flat(), case.elev)
    assert len(means) == 48 == int((f['count'] > 0).sum())
    worst, _ = B.worst_exact_error(means, f['mean'][..., -1])
    assert worst <= 0.09
    # one-pixel cells can use all of it: a sample half a unit from its fixed-point value
    e = 12.0 + (2.0 ** -33) * (1 - 2.0 ** -10)
    assert abs(Fraction(float(B.fixed_point([e])[0])) / 2 ** 32 - Fraction(e)) > Fraction(999, 1000) * Fraction(1, 2 ** 33)
