"""
Constructed collections for the area-weighted mosaic (``amt_area_mosaic_frames``, auromat_amd/csrc/amt_area.hip) as plain
host arrays, seeded and deterministic.  A plain helper module (NumPy only) for tests/test_gpu_mosaic_area_cells.py, which runs
the collections on the device, and tests/test_mosaic_area_cpu.py, which checks without a GPU that they aim where they claim to.
Expected results come from tests/_mosaic_area_oracle.py.

A collection is a list of ``_area_cases.AreaCase`` members on ONE pair of edges (same image dtype, channel count, lon_wrap and
axis kind) and one window (x0, y0, nx, ny) of the grid per member.  Members have 1 x 1 to 33 x 17 pixels, the grids at most
48 x 40 cells (3 x 3 select tiles of 16 x 16 cells).
"""
import numpy as np

import _area_cases as K
import _area_oracle as O

SEL_TILE = 16               # kSelTile of amt_mosaic_plan.h: the election walks the members per 16 x 16 cells
EDOMAIN = -5

GX, GY = K.unit_edges(48, 0.5, 0.0), K.unit_edges(40, 0.5, 0.0)      # x in [0, 24], y in [0, 20]
FULL = (0, 0, 48, 40)
EMPTY = (0, 0, 0, 0)


class Collection(object):
    def __init__(self, name, members, windows, rules=(0, 1), status=None, min_coverage=0.5):
        self.name, self.members, self.windows = name, list(members), [tuple(int(v) for v in w) for w in windows]
        self.rules = tuple(rules)
        self.status = {0: 0, 1: 0}                                  # the expected return code per rule
        self.status.update(status or {})
        self.min_coverage = min_coverage
        first = self.members[0]
        self.xedges, self.yedges = first.xedges, first.yedges
        self.shape, self.lon_wrap, self.uniform = first.shape, first.lon_wrap, first.uniform
        self.dtype, self.nch = first.img.dtype, first.img.shape[1]
        ny, nx = self.shape
        for m, (x0, y0, wnx, wny) in zip(self.members, self.windows):
            assert np.array_equal(m.xedges, self.xedges) and np.array_equal(m.yedges, self.yedges), name
            assert (m.img.dtype, m.img.shape[1], m.lon_wrap, m.uniform) == (self.dtype, self.nch, self.lon_wrap, self.uniform)
            assert m.min_elevation == float('-inf')
            assert (wnx == 0 and wny == 0) or (0 <= x0 and 0 <= y0 and x0 + wnx <= nx and y0 + wny <= ny and wnx > 0 and wny > 0)
        assert len(self.members) == len(self.windows)

    def __repr__(self):
        return self.name


def axis_window(edges, lo, hi):
    """(first, count) of the cells [edges[c], edges[c + 1]] that meet [lo, hi], as ``resample.mosaic_axis_window``."""
    n = len(edges) - 1
    c0 = max(int(np.searchsorted(edges[1:], lo, side='left')), 0)
    c1 = min(int(np.searchsorted(edges[:-1], hi, side='right')) - 1, n - 1)
    return (c0, c1 - c0 + 1) if c1 >= c0 else (0, 0)


def box_window(case):
    """The window of the cells that meet the box of the member's finite corners (wrapped like the kernel wraps them)."""
    fin = np.isfinite(case.lat) & np.isfinite(case.lon)
    x = O.wrap180_shifted(case.lon[fin]) if case.lon_wrap else case.lon[fin]
    x0, nx = axis_window(case.xedges, x.min(), x.max())
    y0, ny = axis_window(case.yedges, case.lat[fin].min(), case.lat[fin].max())
    return (x0, y0, nx, ny) if nx and ny else EMPTY


def member(name, h, w, x0, y0, dx, dy, seed, jitter=0.25, **kw):
    return K.lattice(name, h, w, GX, GY, x0, y0, dx, dy, jitter=jitter, seed=seed, **kw)


def boxed(name, members, **kw):
    return Collection(name, members, [box_window(m) for m in members], **kw)


def clipping(case, window):
    """Per admitted pixel of `case`: candidate cells before and after the cut to `window`, and whether the cut removed cells on
    the west, east, south, north side — as the windowed kernel counts them."""
    _, X, Y, _ = O.admitted(case)
    ix0, nxr, iy0, nyr = O.candidate_ranges(X, Y, case.xedges, case.yedges)
    x0, y0, wnx, wny = window
    ix1, iy1 = ix0 + nxr - 1, iy0 + nyr - 1
    cx0, cx1 = np.maximum(ix0, x0), np.minimum(ix1, x0 + wnx - 1)
    cy0, cy1 = np.maximum(iy0, y0), np.minimum(iy1, y0 + wny - 1)
    some = (nxr > 0) & (nyr > 0)
    left = some & (cx1 >= cx0) & (cy1 >= cy0)
    after = np.where(left, (cx1 - cx0 + 1) * (cy1 - cy0 + 1), 0)
    sides = dict(west=left & (cx0 > ix0), east=left & (cx1 < ix1), south=left & (cy0 > iy0), north=left & (cy1 < iy1))
    return nxr * nyr, after, sides


# ---- member counts, sizes and windows --------------------------------------------------------------------------------------
def one_member_case():
    return Collection('one_member', [member('one', 9, 13, 3.3, 2.2, 0.55, 0.6, 11)], [FULL])


def two_in_one_tile_case():
    """Two windows that overlap inside select tile (0, 0)."""
    a, b = member('a', 6, 7, 1.2, 1.1, 0.5, 0.55, 21), member('b', 5, 5, 2.9, 2.6, 0.6, 0.5, 22)
    c = boxed('two_in_one_tile', [a, b])
    assert all(x0 + nx <= SEL_TILE and y0 + ny <= SEL_TILE for x0, y0, nx, ny in c.windows)
    return c


def three_with_empty_case():
    """Three members, the second with an empty window; the other two overlap across the borders of the select tiles."""
    a, b, c = member('a', 17, 20, 4.2, 3.1, 0.6, 0.62, 31), member('b', 6, 6, 8.0, 8.0, 0.5, 0.5, 32), \
        member('c', 15, 33, 6.5, 6.3, 0.45, 0.7, 33)
    return Collection('three_with_empty', [a, b, c], [box_window(a), EMPTY, box_window(c)])


def sizes_case():
    """1, 35, 561 (three workgroups, the last partly filled) and 512 (two full workgroups) pixels."""
    ms = [member('s1', 1, 1, 5.3, 4.2, 1.3, 1.1, 41), member('s35', 5, 7, 2.2, 9.1, 0.7, 0.6, 42),
          member('s561', 17, 33, 3.1, 1.2, 0.52, 0.9, 43), member('s512', 32, 16, 9.7, 2.3, 0.8, 0.5, 44)]
    assert [m.height * m.width for m in ms] == [1, 35, 561, 512]
    return boxed('sizes', ms)


def many_members_case():
    """65 small members (the first a single pixel) all over the grid: select tiles with long and with empty member lists."""
    ms = []
    for i in range(65):
        h, w = (1, 1) if i == 0 else (1 + i % 5, 1 + (i * 7) % 4)
        ms.append(member('m%d' % i, h, w, 1.0 + (i * 37) % 20, 1.0 + (i * 23) % 16, 0.4 + 0.1 * (i % 6), 0.45 + 0.1 * (i % 5),
                         100 + i, nch=1))
    return boxed('many_65', ms)


# ---- the three paths of the windowed kernel --------------------------------------------------------------------------------
WIDE = [(2.3, 1.6), (21.1, 2.2), (21.7, 18.4), (3.1, 17.8)]           # 40 x 34 candidate cells of the common grid
SMALL = [(6.2, 6.1), (6.9, 6.3), (7.1, 6.8), (6.3, 7.0)]


def clip_lane_case():
    """A lattice that overhangs its window on all four sides: lane-path pixels cut on each side."""
    a = member('over', 12, 12, 4.0, 4.0, 0.6, 0.6, 51)
    b = member('beside', 7, 9, 6.1, 5.2, 0.55, 0.5, 52)
    return Collection('clip_lane', [a, b], [(10, 10, 9, 9), box_window(b)])


def clip_wave_case():
    """A wide pixel whose range still has 30 x 20 cells after the cut: the wave path on a clipped range."""
    a = K.quads_frame('wide', [WIDE, SMALL], GX, GY, seed=53)
    b = member('under', 9, 9, 5.5, 5.5, 0.7, 0.7, 54)
    return Collection('clip_wave', [a, b], [(5, 5, 30, 20), box_window(b)])


def path_switch_case():
    """The same wide pixel with a window of 3 x 4 cells: wave path before the cut, lane path after."""
    a = K.quads_frame('wide', [WIDE, SMALL], GX, GY, seed=55)
    b = member('under', 9, 9, 3.5, 3.5, 0.7, 0.7, 56)
    return Collection('path_switch', [a, b], [(11, 11, 3, 4), box_window(b)])


def outside_window_case():
    """Two quadrilaterals, one inside the member's window and one inside the grid but wholly outside the window."""
    far = [(15.2, 15.1), (16.4, 15.3), (16.6, 16.2), (15.3, 16.0)]
    a = K.quads_frame('in_and_out', [SMALL, far], GX, GY, seed=57)
    b = member('other', 4, 4, 14.6, 14.4, 0.7, 0.6, 58)
    return Collection('outside_window', [a, b], [(8, 8, 10, 10), box_window(b)])


# ---- formats ---------------------------------------------------------------------------------------------------------------
FX, FY = K.unit_edges(12, 0.25, 10.0), K.unit_edges(9, 0.25, -3.0)


def _format_pair(tag, seed, **kw):
    """Two overlapping members of odd widths (13 and 7), the second 8 bytes off a 16-byte boundary."""
    a = K.lattice(tag + '_a', 9, 13, FX, FY, 9.9, -3.1, 0.26, 0.27, jitter=0.25, seed=seed, **kw)
    b = K.lattice(tag + '_b', 6, 7, FX, FY, 10.5, -2.5, 0.3, 0.28, jitter=0.25, seed=seed + 1, coord_offset=1, **kw)
    return [a, b]


def format_cases():
    out = []
    for dtype in (np.uint8, np.uint16):
        for nch in (0, 1, 3, 4):
            tag = 'fmt_%s_%d' % (np.dtype(dtype).name, nch)
            out.append(boxed(tag, _format_pair(tag, 200 + nch, dtype=dtype, nch=nch)))
    a, b = _format_pair('fmt_no_elev', 210)
    b = K.lattice('fmt_no_elev_b', 6, 7, FX, FY, 10.5, -2.5, 0.3, 0.28, jitter=0.25, seed=211, elev=None)
    out.append(boxed('fmt_no_elev', [a, b], rules=(0,)))
    a, b = _format_pair('fmt_nan_elev', 220)
    elev = a.elev.copy()
    elev[2:5, 3:9] = np.nan
    a = K.lattice('fmt_nan_elev_a', 9, 13, FX, FY, 9.9, -3.1, 0.26, 0.27, jitter=0.25, seed=220, elev=elev)
    out.append(boxed('fmt_nan_elev', [a, b]))
    mask = np.random.RandomState(5).rand(9, 13) < 0.3
    a = K.lattice('fmt_mask_a', 9, 13, FX, FY, 9.9, -3.1, 0.26, 0.27, jitter=0.25, seed=230, mask=mask)
    out.append(boxed('fmt_mask', [a, _format_pair('fmt_mask', 230)[1]]))
    return out


def lon_wrap_case():
    """Two members across +-180 binned in the shifted plane (``_area_cases.axis_cases``' frame and a copy moved north-east)."""
    ex, ey = K.unit_edges(20, 0.5, -5.0), K.unit_edges(8, 0.5, 60.0)
    ms = []
    for i, (lon0, lat0, h, w) in enumerate(((176.0, 60.0, 8, 19), (177.3, 61.1, 5, 9))):
        c, r = np.meshgrid(np.arange(w + 1, dtype=np.float64), np.arange(h + 1, dtype=np.float64))
        lon = lon0 + 0.45 * c + 0.1 * np.random.RandomState(6 + i).uniform(-1, 1, c.shape)
        lon = np.where(lon >= 180.0, lon - 360.0, lon)
        ms.append(K.AreaCase('wrap_%d' % i, lat0 + 0.4 * r, lon, ex, ey, lon_wrap=1, seed=240 + i))
    return boxed('lon_wrap', ms)


def edge_array_case():
    """Edge-array axes (unequal cells): ``_area_cases.axis_cases``' frame and a second member on the same edges."""
    a = K.axis_cases()[0]
    b = K.lattice('edges_b', 7, 5, a.xedges, a.yedges, 2.1, 0.4, 0.6, 0.5, jitter=0.3, seed=250, uniform=False)
    return boxed('edge_arrays', [a, b])


# ---- rule 1 ----------------------------------------------------------------------------------------------------------------
def tie_case():
    """The same geometry and elevation twice, different images: every cell ties, the first member wins."""
    a = member('tie_a', 8, 9, 3.3, 2.7, 0.7, 0.65, 61)
    img = np.random.RandomState(62).randint(0, 256, a.img.shape).astype(np.uint8)
    b = member('tie_b', 8, 9, 3.3, 2.7, 0.7, 0.65, 61, img=img)
    assert np.array_equal(a.elev, b.elev) and np.array_equal(a.lat, b.lat) and not np.array_equal(a.img, b.img)
    return boxed('tie', [a, b])


def sliver_case():
    """Regular lattices of unit pixels on cells of 0.5.  Member 0 looks steeply (70 deg) at [5.15, 9.15]^2, member 1 flatly
    (20 deg) at [2.15, 12.15]^2.  Member 0 covers 0.7 of the cells along its lower edges, 0.49 of the cell in its lower corner
    and 0.3 along its upper edges: there it stays below a minimum coverage of 0.5 and loses the cell to member 1, which covers
    it whole.  Along member 1's own upper edges (0.3) no member reaches the minimum."""
    a = member('steep', 4, 4, 5.15, 5.15, 1.0, 1.0, 71, jitter=0.0, elev=np.full((4, 4), 70.0))
    b = member('flat', 10, 10, 2.15, 2.15, 1.0, 1.0, 72, jitter=0.0, elev=np.full((10, 10), 20.0))
    return boxed('sliver', [a, b])


# ---- overflow --------------------------------------------------------------------------------------------------------------
def overflow_cases():
    """``coverage_limit_case``: n unit squares on one cell.  Two members of 200: each below 2^40, together above.  One member
    of 257 beside a member of 3: above on its own."""
    win = (0, 0, 2, 2)
    return [Collection('overflow_total', [K.coverage_limit_case(200), K.coverage_limit_case(200)], [win, win],
                       status={0: EDOMAIN, 1: 0}),
            Collection('overflow_member', [K.coverage_limit_case(3), K.coverage_limit_case(257)], [win, win],
                       status={0: EDOMAIN, 1: EDOMAIN}),
            Collection('overflow_at_limit', [K.coverage_limit_case(128), K.coverage_limit_case(128)], [win, win])]


# ---- partitions ------------------------------------------------------------------------------------------------------------
def cut(case, r0, r1, c0, c1, name):
    """Pixels [r0, r1) x [c0, c1) of `case` as a member of their own (with the corner rows r0..r1 and columns c0..c1)."""
    h, w = case.height, case.width
    nch = case.img.shape[1]
    img = case.img.reshape(h, w, nch)[r0:r1, c0:c1].reshape(-1, nch).copy()
    return K.AreaCase(name, case.lat[r0:r1 + 1, c0:c1 + 1].copy(), case.lon[r0:r1 + 1, c0:c1 + 1].copy(), case.xedges, case.yedges,
                      dtype=case.img.dtype, nch=nch, elev=None if case.elev is None else case.elev[r0:r1, c0:c1].copy(),
                      mask=None if case.mask is None else case.mask[r0:r1, c0:c1].copy(), lat_c=case.lat_c[r0:r1, c0:c1].copy(),
                      lon_wrap=case.lon_wrap, uniform=case.uniform, img=img)


def partition_cases():
    """(whole frame, Collection of its parts on the full grid): cut in two and in three by rows, and in two by columns."""
    out = []
    for whole, cuts, by in ((K.outside_case(), (0, 5, 12), 'rows'), (K.axis_cases()[0], (0, 3, 7, 11), 'rows'),
                            (K.skip_case(), (0, 3, 8), 'columns')):
        h, w = whole.height, whole.width
        parts = [cut(whole, a, b, 0, w, 'part') if by == 'rows' else cut(whole, 0, h, a, b, 'part') for a, b in zip(cuts, cuts[1:])]
        if whole.name == 'skip_rules':
            # (the frame's elevation threshold is not the mosaic's: min_elevation is -inf for every member)
            whole = cut(whole, 0, h, 0, w, 'skip_rules_no_threshold')
        ny, nx = whole.shape
        out.append((whole, Collection('partition_%s_%d_%s' % (whole.name, len(parts), by), parts, [(0, 0, nx, ny)] * len(parts))))
    return out


def device_cases():
    return ([one_member_case(), two_in_one_tile_case(), three_with_empty_case(), sizes_case(), many_members_case(),
             clip_lane_case(), clip_wave_case(), path_switch_case(), outside_window_case()] + format_cases() +
            [lon_wrap_case(), edge_array_case(), tie_case(), sliver_case()] + overflow_cases() +
            [c for _, c in partition_cases()])
