"""
TEST INFRASTRUCTURE — constructed grids for the binning that is fused into the row kernel (k_georef_rows<..., BIN> of
auromat_amd/csrc/amt_georef.hip with bin_fast / bin_slow / on_lower_edge_bits / to_fix32 of amt_common.h, and k_apply_bin_events /
k_pipe_finish of amt_binning.hip).  A plain helper module (NumPy only) for tests/test_gpu_fused_bin.py, which runs the cases on
the device, and tests/test_fused_cases_cpu.py, which checks without a GPU that the cases hold what they claim.

The fused kernel cannot be given centre coordinates, but it can be given axes.  So every case starts from the centre arrays a
plain launch produced (lat_c, lon_c, elev, mlat_c, mlt_c: the device's own bits; on a CPU the float64 oracle's as a stand-in)
and builds uniform axes AROUND single pixels of them:

  axis_for(v, k, nbin, step, want)   np.linspace edges whose edge k stands in the relation `want` to the double v:
        eq       v == edge k, bit for bit                    below1   v one ulp below edge k        above1   v one ulp above
        zone     v above edge k and inside its rounding zone: around(v, decimal) == around(edge, decimal)
        near     v above edge k, outside the rounding zone, but closer than 1.5 / scale to it (bin_fast's margin: the exact
                 path without a flag)
        inside   v well inside the cell above edge k
  with k = 0 (the first edge: below1 is then a pixel below the axis), k interior, and k = nbin (the last edge: zone and near
  are then pixels beyond the axis, inside and outside the rounding zone of the right-most-edge rule).  The constructor searches:
  it starts from first = target - k step, keeps last = first + nbin step, nudges both by single ulps (of the target, where
  `first` is the smaller number) and stops when np.linspace(first, last, nbin + 1)[k] has the wanted relation to v, as
  relation() — which only compares doubles — sees it.  It returns None when no nudge gets there (an edge k step away from a
  first edge in a higher binade than v cannot take every double next to v).

What the kernel must give comes from tests/_bin_oracle.py and tests/_median_oracle.py on a tests/_median_cases.Case that wraps
those arrays (see as_case), plus the three statements that exist nowhere else and are written down here in Python:
expected_with_events (which pixels on_lower_edge_bits flags: the reference's rule applied to the lower edge of the pixel's own bin),
apply_events (the rule cx == off_x + nx of k_apply_bin_events and k_pipe_finish) and anchors (which cell a wave's first binned
pixel lies in, for the census only).  tests/test_fused_cases_cpu.py pins the first two to _median_oracle.axis_index.

Aimed fields (aimed_field): smooth 0.03 x 0.04 deg / px fields of tests/_rowfield_cases.aimed in which the four corners of single
interior pixels are moved, by iteration with the float64 oracle, until the pixel's centre sits at a chosen offset from a chosen
edge of the frame's final grid (which follows from the frame's extreme corners: those stay where they are).
"""
import ctypes as C

import numpy as np

import _bin_oracle as B
import _median_cases as MC
import _median_oracle as M
import _rowfield_cases as K

RELATIONS = ('eq', 'below1', 'above1', 'zone', 'near', 'inside')
ON_EDGE = ('eq', 'above1', 'zone')                    # relations the rounding rule calls on-edge (for a pixel inside the axis)
POSITIONS = ('first', 'interior', 'last')
STEPS = (0.125, 0.1)                                  # dyadic, not dyadic
SIZES = tuple(s for s in K.OWNERSHIP_SIZES if s != (1, 1))      # the library refuses fused binning on fewer than 3 pixels
EVENT_DTYPE = np.dtype([('bx', '<i4'), ('by', '<i4'), ('flags', '<u4'), ('c0', '<u4'), ('c1', '<u4'), ('c2', '<u4'),
                        ('el', '<i8')])               # bin_event of amt_common.h
assert EVENT_DTYPE.itemsize == 32
STRIP, CHUNK = 63, 16                                 # pixel columns and rows of a work item (one wave)
WINDOW = 8                                            # kBinW: cells per axis of a wave's LDS window, anchored at bin - 4


# ---- axes ---------------------------------------------------------------------------------------------------------------------
def decimal_of(edges):
    """the `decimal` of the right-most-edge rule (histogram.py:219) of an axis"""
    return int(-np.log10(np.diff(edges).min())) + 6


def scale_of(edges):
    return 10.0 ** decimal_of(edges)


def relation(v, edges, k):
    """The relation of the double v to edge k of the axis, by comparisons of doubles alone; 'below' / 'other' when none of
    RELATIONS holds."""
    e, dec = float(edges[k]), decimal_of(edges)
    step = float(edges[-1] - edges[0]) / (len(edges) - 1)
    if v == e:
        return 'eq'
    if v == np.nextafter(e, -np.inf):
        return 'below1'
    if v == np.nextafter(e, np.inf):
        return 'above1'
    if v < e:
        return 'below'
    if np.around(v, dec) == np.around(e, dec):
        return 'zone'
    if (v - e) * 10.0 ** dec < 1.4:
        return 'near'
    if 0.05 < (v - e) / step < 0.95:
        return 'inside'
    return 'other'


def _nudged(x, j, ulp):
    return float(x + j * ulp) if j else float(x)


def axis_for(v, k, nbin, step, want):
    """np.linspace(first, last, nbin + 1) with relation(v, edges, k) == want, or None (see the module docstring)."""
    v = float(v)
    assert want in RELATIONS and 0 <= k <= nbin
    guess = int(-np.log10(step)) + 6
    order = [0] + [s * j for j in range(1, 13) for s in (1, -1)]
    for dec in (guess, guess - 1, guess + 1):
        unit = 10.0 ** -dec
        targets = dict(eq=[v], below1=[np.nextafter(v, np.inf)], above1=[np.nextafter(v, -np.inf)],
                       zone=[v - c * unit for c in (0.2, 0.1, 0.3, 0.05, 0.4, 0.02)], near=[v - 1.2 * unit],
                       inside=[v - 0.37 * step])[want]
        exact = want in ('eq', 'below1', 'above1')
        for target in targets:
            target = float(target)
            first0 = target - k * step
            ulp = max(np.spacing(abs(first0)), np.spacing(abs(target)))
            for j in order if exact else (0,):
                first = _nudged(first0, j, ulp)
                last0 = first + nbin * step
                for m in (0, 1, -1, 2, -2) if exact else (0,):
                    last = _nudged(last0, m, np.spacing(abs(last0)))
                    if exact:                                  # edge k alone, as np.linspace forms it, before the whole axis
                        e_k = last if k == nbin else np.float64(k) * np.float64((last - first) / nbin) + np.float64(first)
                        if float(e_k) != target:
                            continue
                    edges = np.linspace(first, last, nbin + 1)
                    if np.all(np.diff(edges) > 0) and relation(v, edges, k) == want:
                        edges.setflags(write=False)
                        return edges
    return None


def k_of(position, nbin):
    return dict(first=0, interior=nbin // 2, last=nbin)[position]


# ---- the arrays a case is built around -----------------------------------------------------------------------------------------
def binned_xy(arrays, magnetic=False, lon_wrap=False):
    """(x, y) as the fused kernel bins them, flat: (lon_c, lat_c), the longitude wrapped like the reference's date-line branch
    (resample.py:212-218), or (SM longitude, MLat) with the SM longitude formed as mlt_to_sm_lon forms it."""
    if magnetic:
        return (np.ravel(arrays['mlt_c']) - 12.0) / (24.0 / 360.0), np.ravel(arrays['mlat_c'])
    x = np.ravel(arrays['lon_c'])
    if lon_wrap:
        from oracle import ref_numpy as O
        x = O.wrap_at(x + 180.0, 180.0)
    return x, np.ravel(arrays['lat_c'])


def image_of(name, width, height, dtype):
    """random over the full range: every channel sum identifies its pixels"""
    rng = np.random.RandomState((sum(map(ord, name)) * 131 + width * 17 + height) % (2 ** 31))
    return rng.randint(0, np.iinfo(dtype).max + 1, size=(height, width, 3)).astype(dtype)


def as_case(tag, x, y, elev, img, xedges, yedges, min_elevation, keep=None):
    """The _median_cases.Case of one launch: its keep rule is elev >= min_elevation (and `keep`, for the pixels exact centres
    drop), its membership rule that of _median_oracle.cell_index."""
    h, w = img.shape[:2]
    mask = None if keep is None else (~np.ravel(keep)).astype(np.uint8)
    return MC.Case(tag, None, np.ravel(y), np.ravel(x), np.ravel(elev), img.reshape(h * w, 3), mask, np.asarray(xedges),
                   np.asarray(yedges), h, w, min_elevation=min_elevation, uniform=True, lon_binned=np.ravel(x))


def to_acc(p):
    """planes of _bin_oracle (rows north to south) -> the accumulator layout (5, nx, ny): [plane, cx, cy], cy ascending"""
    return np.stack([p['count'][::-1].T] + [p['sums'][::-1, :, ch].T for ch in range(3)] + [p['fx'][::-1].T]).astype(np.int64)


def expected_planes(case):
    """without an event list: the grid given is the final one"""
    return to_acc(B.planes(case))


def bins_and_flags(case):
    """1-based bins by the reference's rule (0: not binned), and the on-edge flags of every pixel: 1 / 2 when the pixel sits on
    the LOWER edge of its own x / y bin in the sense of the right-most-edge rule, around(v, decimal) == around(edge, decimal)
    (the definition of on_lower_edge_bits' first bit)."""
    nx, ny = len(case.xedges) - 1, len(case.yedges) - 1
    x, y = np.ravel(case.lon_binned), np.ravel(case.lat)
    bx, by = M.axis_index(x, case.xedges), M.axis_index(y, case.yedges)
    ok = case.keep() & (bx >= 1) & (bx <= nx) & (by >= 1) & (by <= ny)
    dx, dy = decimal_of(case.xedges), decimal_of(case.yedges)
    with np.errstate(invalid='ignore'):
        fx = np.around(x, dx) == np.around(case.xedges[np.clip(bx - 1, 0, nx)], dx)
        fy = np.around(y, dy) == np.around(case.yedges[np.clip(by - 1, 0, ny)], dy)
    flags = np.where(ok, fx * 1 + fy * 2, 0).astype(np.uint32)
    return np.where(ok, bx, 0), np.where(ok, by, 0), flags


def sorted_events(ev):
    return np.sort(np.asarray(ev, dtype=EVENT_DTYPE), order=list(EVENT_DTYPE.names))


def expected_with_events(case):
    """with an event list: (accumulators (5, nx, ny) of everything that is not on an edge, the sorted records of what is)"""
    bx, by, flags = bins_and_flags(case)
    on = flags > 0
    ev = np.zeros(int(on.sum()), dtype=EVENT_DTYPE)
    ev['bx'], ev['by'], ev['flags'] = bx[on], by[on], flags[on]
    for ch in range(3):
        ev['c%d' % ch] = case.img[on, ch]
    ev['el'] = B.fixed_point(case.elev[on])
    keep = case.keep() & ~on
    rest = MC.Case(case.name, None, case.lat, case.lon, case.elev, case.img, (~keep).astype(np.uint8), case.xedges, case.yedges,
                   case.height, case.width, uniform=True, lon_binned=case.lon_binned)
    return to_acc(B.planes(rest)), sorted_events(ev)


def apply_events(acc, events, window):
    """k_apply_bin_events / k_pipe_finish in Python: accumulators (5, acc_nx, acc_ny) plus records -> the window
    (off_x, off_y, nx, ny) of the final grid.  A record on the lower edge of the first cell beyond the window sits on the
    last edge of the final grid and goes to the last bin; every other record stays in its cell."""
    off_x, off_y, nx, ny = window
    out = np.array(acc, dtype=np.int64)
    for e in events:
        cx, cy = int(e['bx']) - 1, int(e['by']) - 1
        if (int(e['flags']) & 1) and cx == off_x + nx:
            cx -= 1
        if (int(e['flags']) & 2) and cy == off_y + ny:
            cy -= 1
        if 0 <= cx < out.shape[1] and 0 <= cy < out.shape[2]:
            out[:, cx, cy] += np.array([1, e['c0'], e['c1'], e['c2'], e['el']], dtype=np.int64)
    return out[:, off_x:off_x + nx, off_y:off_y + ny]


def sub_case(case, window):
    """the case on the sub-axes edges[off : off + n + 1], taken as the final grid"""
    off_x, off_y, nx, ny = window
    return MC.Case(case.name, None, case.lat, case.lon, case.elev, case.img, case.mask, case.xedges[off_x:off_x + nx + 1],
                   case.yedges[off_y:off_y + ny + 1], case.height, case.width, min_elevation=case.min_elevation, uniform=True,
                   lon_binned=case.lon_binned)


def windows_of(case, limit=12):
    """Windows of the case's grid whose sub-axes keep the grid's `decimal` (they share its bits by construction: they ARE its
    edges): every window whose last x or y edge is the lower edge of a flagged pixel's bin, and one whose last edges are not."""
    bx, by, flags = bins_and_flags(case)
    nx, ny = len(case.xedges) - 1, len(case.yedges) - 1
    dx, dy = decimal_of(case.xedges), decimal_of(case.yedges)
    ends_x = sorted({int(b) - 1 for b, f in zip(bx, flags) if f & 1 and b >= 2})       # last edge index = bx - 1
    ends_y = sorted({int(b) - 1 for b, f in zip(by, flags) if f & 2 and b >= 2})
    free_x = [i for i in range(nx, 0, -1) if i not in ends_x]
    free_y = [i for i in range(ny, 0, -1) if i not in ends_y]
    out = []

    def add(ex, ey, kind):
        for x0 in (0, max(0, ex - 3)):
            for y0 in (0, max(0, ey - 2)):
                w = (x0, y0, ex - x0, ey - y0)
                if w[2] < 1 or w[3] < 1 or (w, kind) in out:
                    continue
                if decimal_of(case.xedges[x0:ex + 1]) == dx and decimal_of(case.yedges[y0:ey + 1]) == dy:
                    out.append((w, kind))
    for ex in ends_x[:3]:
        add(ex, free_y[0] if free_y else ny, 'x')
    for ey in ends_y[:3]:
        add(free_x[0] if free_x else nx, ey, 'y')
    for ex in ends_x[:2]:
        for ey in ends_y[:2]:
            add(ex, ey, 'xy')
    if free_x and free_y:
        add(free_x[min(1, len(free_x) - 1)], free_y[min(1, len(free_y) - 1)], 'free')
    return out[:limit]


def anchors(case, with_events):
    """(x bin, y bin) of the first binned pixel of every wave (strip of 63 columns x chunk of 16 rows, rows top to bottom, the
    lowest column first): where the wave's LDS window is anchored.  For the census only."""
    bx, by, flags = bins_and_flags(case)
    if with_events:
        bx, by = np.where(flags > 0, 0, bx), np.where(flags > 0, 0, by)
    bx, by = bx.reshape(case.height, case.width), by.reshape(case.height, case.width)
    out = []
    for r0 in range(0, case.height, CHUNK):
        for c0 in range(0, case.width, STRIP):
            blk = bx[r0:r0 + CHUNK, c0:c0 + STRIP] > 0
            if blk.any():
                r, c = np.argwhere(blk)[0]
                out.append((int(bx[r0 + r, c0 + c]), int(by[r0 + r, c0 + c])))
    return out


def outside_window(case):
    """pixels whose cell lies outside their wave's 8 x 8 window (the global-atomic path of bin_flush), without events"""
    bx, by, _ = bins_and_flags(case)
    bx, by = bx.reshape(case.height, case.width), by.reshape(case.height, case.width)
    n = 0
    for r0 in range(0, case.height, CHUNK):
        for c0 in range(0, case.width, STRIP):
            sx, sy = bx[r0:r0 + CHUNK, c0:c0 + STRIP], by[r0:r0 + CHUNK, c0:c0 + STRIP]
            if (sx > 0).any():
                r, c = np.argwhere(sx > 0)[0]
                ax, ay = sx[r, c] - WINDOW // 2, sy[r, c] - WINDOW // 2
                inside = (sx - ax >= 0) & (sx - ax < WINDOW) & (sy - ay >= 0) & (sy - ay < WINDOW)
                n += int(((sx > 0) & ~inside).sum())
    return n


# ---- the grids of a field ------------------------------------------------------------------------------------------------------
FIELDS = tuple('ownership-%dx%d' % s for s in SIZES) + ('broken', 'inside', 'dateline-east-rows', 'dateline-west-columns')
LARGE_NBIN = 60000


def min_elevation_of(name):
    """a threshold that drops about a quarter of the field's pixels (from the float64 oracle: a fixed number per field);
    -inf on the field whose camera is inside the shell (all its elevations are negative)"""
    if name == 'inside':
        return float('-inf')
    e = K.float64_oracle(name)['elev']
    return float(np.round(np.nanpercentile(e, 25), 3))


def settings_of(name):
    c = K.by_name(name)
    return dict(width=c['width'], height=c['height'], min_elevation=min_elevation_of(name), lon_wrap=bool(c['dateline']))


def target_pixels(arrays, min_elevation, n=4):
    """kept pixels, the nearest to the frame's middle first"""
    h, w = arrays['elev'].shape
    with np.errstate(invalid='ignore'):
        kept = np.argwhere(arrays['elev'] >= min_elevation)
    d = np.abs(kept[:, 0] - (h - 1) / 2.0) / max(h, 1) + np.abs(kept[:, 1] - (w - 1) / 2.0) / max(w, 1)
    return [tuple(int(v) for v in kept[i]) for i in np.argsort(d, kind='stable')[:n]]


def _axis_pair(arrays, flat, magnetic, lon_wrap, spec_x, spec_y):
    x, y = binned_xy(arrays, magnetic, lon_wrap)
    ex = axis_for(x[flat], *spec_x)
    ey = axis_for(y[flat], *spec_y)
    return ex, ey


def grids(name, arrays, magnetic=False):
    """The grids of one field, built around single pixels of `arrays`: list of dict(tag, xedges, yedges, pixel (flat index),
    rel_x, k_x, rel_y, k_y, kind).  A relation the constructor cannot reach around the first target pixel is tried around the
    next ones; what is reached nowhere is left out (the census of the tests says what is required)."""
    s = settings_of(name)
    h, w = s['height'], s['width']
    lon_wrap = s['lon_wrap'] and not magnetic
    pixels = [r * w + c for r, c in target_pixels(arrays, s['min_elevation'])]
    out = []

    def add(tag, kind, spec_x, spec_y, pix=None, wrap=lon_wrap, **extra):
        for flat in ([pix] if pix is not None else pixels):
            ex, ey = _axis_pair(arrays, flat, magnetic, wrap, spec_x, spec_y)
            if ex is not None and ey is not None:
                out.append(dict(tag=tag, kind=kind, xedges=ex, yedges=ey, pixel=flat, rel_x=spec_x[3], k_x=spec_x[0],
                                rel_y=spec_y[3], k_y=spec_y[0], magnetic=magnetic, lon_wrap=wrap,
                                min_elevation=extra.get('min_elevation', s['min_elevation']), image=extra.get('image', 'random')))
                return
    # (a) every relation at the first, an interior and the last edge, on both axes around ONE pixel (on-edge relations: flags 3),
    # and the same relation on x paired with the next one on y; small axes: part of the frame lies outside on all four sides
    for step in STEPS:
        for i, rel in enumerate(RELATIONS):
            for pos in POSITIONS:
                nbx, nby = 5, 4
                other = RELATIONS[(i + 1) % len(RELATIONS)]
                add('%s-%s-%g' % (rel, pos, step), 'class', (k_of(pos, nbx), nbx, step, rel), (k_of(pos, nby), nby, step, rel))
                if pos == 'interior':
                    add('%s+%s-%g' % (rel, other, step), 'class', (k_of(pos, nbx), nbx, step, rel),
                        (k_of(pos, nby), nby, step, other))
    # (b) one cell for the whole frame
    # (every pixel kept: each lane has one run over all rows of its chunk; with every channel at its maximum the sums of a
    # wave's window are the largest there are, 63 * 16 * 65535)
    add('one-cell', 'shape', (0, 1, 1024.0, 'inside'), (0, 1, 1024.0, 'inside'), min_elevation=float('-inf'))
    add('one-cell-max', 'shape', (0, 1, 1024.0, 'inside'), (0, 1, 1024.0, 'inside'), min_elevation=float('-inf'), image='max')
    # (c) grids so fine that a strip spans more than 8 cells in x, in y, in both (the global-atomic path of bin_flush)
    coarse = 2.0
    x, y = binned_xy(arrays, magnetic, lon_wrap)
    with np.errstate(invalid='ignore'):
        kept = np.ravel(arrays['elev']) >= s['min_elevation']
    kept &= ~np.isnan(x) & ~np.isnan(y)
    if lon_wrap or not s['lon_wrap']:                  # (a raw longitude on both sides of the date line spans 358 deg)
        span_x, span_y = float(np.ptp(x[kept])), float(np.ptp(y[kept]))
        # (dyadic cells, 128 to 256 of them across the field on either axis: a strip spans at least 60, and the accumulators
        # of the grid that is fine on both axes stay below 3 MB)
        fine_x, fine_y = 2.0 ** np.floor(np.log2(span_x / 128)), 2.0 ** np.floor(np.log2(span_y / 128))
        nfx, nfy = int(span_x / fine_x) + 9, int(span_y / fine_y) + 9
        lowx, lowy = int(np.flatnonzero(kept)[np.argmin(x[kept])]), int(np.flatnonzero(kept)[np.argmin(y[kept])])
        # (both axes are built around ONE pixel: k places that pixel so that the axis starts 4 cells below the field's minimum)
        p0 = pixels[0]
        kfx, kfy = int((x[p0] - x[lowx]) / fine_x) + 4, int((y[p0] - y[lowy]) / fine_y) + 4
        kcx, kcy = 1, 1
        add('fine-x', 'shape', (kfx, nfx, fine_x, 'inside'), (kcy, 3, coarse, 'inside'), p0)
        add('fine-y', 'shape', (kcx, 3, coarse, 'inside'), (kfy, nfy, fine_y, 'inside'), p0)
        add('fine-xy', 'shape', (kfx, nfx, fine_x, 'inside'), (kfy, nfy, fine_y, 'inside'), p0)
    # (d) the first pixel of the LAST wave in superset cell 1 / cell nbin of either axis: the window anchor bin - 4 is below 1,
    # or the window reaches past the axis
    r0, c0 = ((h - 1) // CHUNK) * CHUNK, ((w - 1) // STRIP) * STRIP
    with np.errstate(invalid='ignore'):
        blk = arrays['elev'][r0:, c0:] >= s['min_elevation']
    if blk.any():
        r, c = np.argwhere(blk)[0]
        first = (r0 + int(r)) * w + c0 + int(c)
        for tx, kx in (('1', 0), ('n', 5)):
            for ty, ky in (('1', 0), ('n', 5)):
                add('anchor-x%s-y%s' % (tx, ty), 'anchor', (kx, 6, 0.125, 'inside'), (ky, 6, 0.125, 'inside'), first)
    # (e) step 0.1 far along a long axis: bin_index's first guess can be off by one there, and linspace_edge must give NumPy's
    # bits.  The exact relations need an edge in the binade of v: k step < 2 |v| (see axis_for)
    if s['lon_wrap']:                                  # (the raw longitude, +-179 deg: a binade in which k step is large)
        x, _ = binned_xy(arrays, magnetic, False)
    for rel in RELATIONS:
        vx, vy = abs(float(x[pixels[0]])), abs(float(y[pixels[0]]))
        kx = min(3000, int(0.9 * 2.0 ** np.ceil(np.log2(max(vx, 1.0))) / 0.1)) if rel in ('eq', 'below1', 'above1') else 3000
        ky = min(3000, int(0.9 * 2.0 ** np.ceil(np.log2(max(vy, 1.0))) / 0.1)) if rel in ('eq', 'below1', 'above1') else 3000
        add('long-x-%s' % rel, 'long', (kx, LARGE_NBIN, 0.1, rel), (1, 3, 0.125, 'inside'), wrap=False)
        add('long-y-%s' % rel, 'long', (1, 3, 0.125, 'inside'), (ky, LARGE_NBIN, 0.1, rel), wrap=False)
    return out


def class_grids(x, y, elev, h, w, min_elevation, keep=None):
    """The class grids of grids() — every relation at the first, an interior and the last edge, on both axes around one
    pixel, at both steps — around flat arrays of any origin (the camera-model variants): list of dict(tag, xedges, yedges,
    pixel, rel, k_x, k_y)."""
    e = np.where(np.ravel(keep), np.ravel(elev), np.nan) if keep is not None else np.ravel(elev)
    e = np.where(np.isnan(x) | np.isnan(y), np.nan, e)
    pixels = [r * w + c for r, c in target_pixels(dict(elev=e.reshape(h, w)), min_elevation, n=6)]
    out = []
    for step in STEPS:
        for rel in RELATIONS:
            for pos in POSITIONS:
                for flat in pixels:
                    ex, ey = axis_for(x[flat], k_of(pos, 5), 5, step, rel), axis_for(y[flat], k_of(pos, 4), 4, step, rel)
                    if ex is not None and ey is not None:
                        out.append(dict(tag='%s-%s-%g' % (rel, pos, step), xedges=ex, yedges=ey, pixel=flat, rel=rel,
                                        k_x=k_of(pos, 5), k_y=k_of(pos, 4)))
                        break
    return out


def grid_image(name, s, g, dtype):
    if g['image'] == 'max':
        return np.full((s['height'], s['width'], 3), np.iinfo(dtype).max, dtype=dtype)
    return image_of(name, s['width'], s['height'], dtype)


def census(name, arrays, grid_list, dtype=np.uint16):
    """What the grids of one field hold: pixels per relation and axis (as relation() sees the arrays given), on-edge pixels
    per flag value, pixels outside a wave's window, anchors in cell 1 / cell nbin, outliers per side."""
    s = settings_of(name)
    out = dict(rel_x={}, rel_y={}, flags={1: 0, 2: 0, 3: 0}, outside=0, anchor=set(), sides=set(), full_cell=0, largest_k=0)
    for g in grid_list:
        x, y = binned_xy(arrays, g['magnetic'], g['lon_wrap'])
        rx, ry = relation(float(x[g['pixel']]), g['xedges'], g['k_x']), relation(float(y[g['pixel']]), g['yedges'], g['k_y'])
        key = lambda rel, k, edges: (rel, 'first' if k == 0 else ('last' if k == len(edges) - 1 else 'interior'))
        out['rel_x'][key(rx, g['k_x'], g['xedges'])] = out['rel_x'].get(key(rx, g['k_x'], g['xedges']), 0) + 1
        out['rel_y'][key(ry, g['k_y'], g['yedges'])] = out['rel_y'].get(key(ry, g['k_y'], g['yedges']), 0) + 1
        case = as_case(g['tag'], x, y, arrays['elev'], grid_image(name, s, g, dtype), g['xedges'], g['yedges'], g['min_elevation'])
        bx, by, flags = bins_and_flags(case)
        for f in (1, 2, 3):
            out['flags'][f] += int((flags == f).sum())
        out['outside'] += outside_window(case)
        nx, ny = len(g['xedges']) - 1, len(g['yedges']) - 1
        for ax, ay in anchors(case, False):
            out['anchor'] |= {('x', '1' if ax == 1 else 'n') for _ in [0] if ax in (1, nx) and nx > 1}
            out['anchor'] |= {('y', '1' if ay == 1 else 'n') for _ in [0] if ay in (1, ny) and ny > 1}
        keep = case.keep()
        fx, fy = M.axis_index(x, g['xedges']), M.axis_index(y, g['yedges'])
        for side, m in (('west', fx == 0), ('east', fx == nx + 1), ('south', fy == 0), ('north', fy == ny + 1)):
            if (m & keep & ~np.isnan(x) & ~np.isnan(y)).any() and g['kind'] == 'class':
                out['sides'].add(side)
        if nx == 1 and ny == 1:
            out['full_cell'] = max(out['full_cell'], int((bx > 0).sum()))
        if g['kind'] == 'long':
            out['largest_k'] = max(out['largest_k'], g['k_x'], g['k_y'])
    return out


def assert_census(name, c):
    """Every class is populated: each relation at each position on both axes, at least 8 on-edge pixels with every flag
    value among them, pixels outside a wave's window (frames of more than 8 fine cells), anchors in cell 1 and cell nbin of
    both axes, outliers on all four sides, one cell that holds the whole frame, and a long axis used far from its start."""
    s = settings_of(name)
    for axis in ('rel_x', 'rel_y'):
        missing = [(r, p) for r in RELATIONS for p in POSITIONS if not c[axis].get((r, p))]
        assert not missing, (name, axis, missing)
    assert sum(c['flags'].values()) >= 8 and all(c['flags'].values()), (name, c['flags'])
    assert c['outside'] > 0, name
    assert c['anchor'] == {('x', '1'), ('x', 'n'), ('y', '1'), ('y', 'n')}, (name, c['anchor'])
    assert c['sides'] == {'west', 'east', 'south', 'north'}, (name, c['sides'])
    kept_all = int(np.isfinite(K.float64_oracle(name)['elev']).sum())
    assert c['full_cell'] == kept_all, (name, c['full_cell'], kept_all)
    assert c['largest_k'] >= 3000, name


# ---- aimed fields --------------------------------------------------------------------------------------------------------------
AIM_ON_EDGE, AIM_NEAR, AIM_BELOW, AIM_BOTH = 2e-7, 8e-7, -2e-7, 2e-8
CAM = K.ecef(49.0, 14.0, 400.0)


def _centre_f64(d4, c):
    """float64 oracle of one fast centre from its four corner directions (2, 2, 3) -> (lat_c, lon_c, mlat_c, mlt_c)"""
    import _rowfield_oracle as R
    f = R.float64_oracle(d4, R.params_of(c))
    return float(f['lat_c'][0, 0]), float(f['lon_c'][0, 0]), float(f['mlat_c'][0, 0]), float(f['mlt_c'][0, 0])


def final_grid(box, ppd):
    """the final grid of a box (south, north, west, east) by the library's own host layout -> Grid"""
    from auromat_amd import _native
    from auromat_amd._native import Grid
    g = Grid()
    rc = _native.lib().amt_grid_layout(float(ppd), float(ppd), box[0], box[1], box[2], box[3], C.byref(g))
    assert rc == 0, (box, ppd)
    return g


K_MARGIN_DEG = 1.0                                    # kMarginDeg of amt_pipe.hip


def superset_grid(box, ppd):
    """the superset that pipe_prepare_rest of amt_pipe.hip lays out for an estimate `box`: the box plus kMarginDeg, the
    longitude margin widened by 1 / cos(lat)"""
    lat_abs = max(abs(box[0]), abs(box[1]))
    lon_margin = min(10.0, K_MARGIN_DEG / max(0.1, np.cos(np.deg2rad(lat_abs))))
    return final_grid((max(-89.0, box[0] - K_MARGIN_DEG), min(89.0, box[1] + K_MARGIN_DEG),
                       max(-180.0, box[2] - lon_margin), min(180.0, box[3] + lon_margin)), ppd)


def axis_edges(ax):
    return np.linspace(ax.first, ax.last, ax.nbin + 1)


def box_of(arrays, magnetic=False):
    """(south, north, west, east) of all corners (no elevation threshold: every corner of these fields counts)"""
    if magnetic:
        la, lo = arrays['mlat'], (arrays['mlt'] - 12.0) / (24.0 / 360.0)
    else:
        la, lo = arrays['lat'], arrays['lon']
    return float(np.nanmin(la)), float(np.nanmax(la)), float(np.nanmin(lo)), float(np.nanmax(lo))


PITCH = (0.03, 0.04)                                  # deg per pixel of the aimed fields in latitude and longitude
MOVE_LIMIT = (0.02, 0.028)                            # deg a pixel's corners may move: no pixel folds over


def fine_smooth(w, h, lat0, lon0):
    """_rowfield_cases.smooth with smaller pixels: an edge of the final grid then has an interior pixel next to it"""
    i, j = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    # (the longitude span is 0.115 deg more than a whole number of 1/8 deg cells: with the western extreme just above a grid node
    # the eastern one is just below one, and the first and the last edge both have an interior pixel column next to them)
    pitch = (np.rint(PITCH[1] * w * 8) / 8 + 0.115 - 0.0005 * h) / w
    return lat0 - PITCH[0] * i + 0.0005 * j, lon0 + pitch * j + 0.0005 * i


def _try_aims(name, w, h, ppd, aims, lat0, lon0, magnetic, cam=None):
    """aimed_field at one placement of the field, or None when an aim has no free interior pixel within MOVE_LIMIT"""
    import _rowfield_oracle as R
    cam = CAM if cam is None else cam
    lat, lon = fine_smooth(w, h, lat0, lon0)
    base = K.aimed(name, 'fused', lat, lon, cam)
    f = R.float64_oracle(base['dirs'], R.params_of(base))
    box = box_of(f, magnetic)
    if min(abs(v * ppd - np.rint(v * ppd)) for v in box) < 1e-3:          # an extreme next to a grid node: the grid is not robust
        return None
    g = final_grid(box, ppd)
    xe, ye = axis_edges(g.xaxis), axis_edges(g.yaxis)
    cx, cy = binned_xy(f, magnetic)
    cx, cy = cx.reshape(h, w), cy.reshape(h, w)
    taken = np.zeros((h, w), bool)
    taken[0, :] = taken[-1, :] = taken[:, 0] = taken[:, -1] = True          # the outer ring keeps the frame's extremes
    done = []

    def centre(r, c, dlat, dlon):
        la, lo = lat[r:r + 2, c:c + 2] + dlat, lon[r:r + 2, c:c + 2] + dlon
        got = _centre_f64(np.ascontiguousarray(K.unit(K.ecef(la, lo, 110.0) - cam) @ K.M_GEO), base)
        return np.array(((got[3] - 12.0) / (24.0 / 360.0), got[2]) if magnetic else (got[1], got[0]))
    for axis, edge, offset in aims:
        pick = lambda e: len(e) - 1 if edge == 'last' else len(e) - 2 if edge == 'before-last' else 0 if edge == 'first' else edge
        ix, iy = pick(xe) if 'x' in axis else None, pick(ye) if 'y' in axis else None
        if (ix is not None and ix >= len(xe)) or (iy is not None and iy >= len(ye)):
            return None
        # the free interior pixel nearest to the wanted place; the axis that is not aimed keeps its coordinate, which has to
        # lie well inside a cell
        dist = np.zeros((h, w))
        for want, cc, e0 in ((None if ix is None else float(xe[ix]) + offset, cx, xe[0]),
                             (None if iy is None else float(ye[iy]) + offset, cy, ye[0])):
            if want is not None:
                dist += np.abs(cc - want)
            else:
                dist[np.abs(((cc - e0) * ppd) % 1.0 - 0.5) > 0.3] = np.inf
        dist[taken] = np.inf
        r, c = np.unravel_index(int(np.argmin(dist)), dist.shape)
        if not dist[r, c] < 2 * MOVE_LIMIT[1]:
            return None
        want = np.array([cx[r, c] if ix is None else float(xe[ix]) + offset, cy[r, c] if iy is None else float(ye[iy]) + offset])
        # Newton on the corner shift (dlat, dlon) with a finite-difference Jacobian of the float64 oracle's centre
        c0 = centre(r, c, 0.0, 0.0)
        jac = np.column_stack([(centre(r, c, 1e-3, 0.0) - c0) / 1e-3, (centre(r, c, 0.0, 1e-3) - c0) / 1e-3])
        d = np.zeros(2)
        for _ in range(40):
            res = want - centre(r, c, d[0], d[1])
            if np.all(np.abs(res) < 2e-12):
                break
            d += np.linalg.solve(jac, res)
        else:
            return None
        if not (abs(d[0]) < MOVE_LIMIT[0] and abs(d[1]) < MOVE_LIMIT[1]):
            return None
        lat[r:r + 2, c:c + 2] += d[0]
        lon[r:r + 2, c:c + 2] += d[1]
        taken[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = True        # (pixels that share a corner with it)
        done.append(dict(pixel=(int(r), int(c)), axis=axis, ix=ix, iy=iy, offset=offset))
    out = K.aimed(name, 'fused', lat, lon, cam)
    out.update(aims=done, ppd=ppd, magnetic=magnetic, xedges=xe, yedges=ye, box=box, lat0=lat0, lon0=lon0)
    return out


def aimed_field(name, w, h, ppd, aims, lat0=50.0, lon0=10.0, magnetic=False):
    """A smooth field in which pixels are aimed at edges of its own final grid.  aims: list of (axis 'x' / 'y' / 'xy', which
    edge: 'last' / 'before-last' (the lower edge of the last cell) / 'first' / an index, offset in deg).  The field is placed
    (a search over shifts of less than a cell from lat0, lon0) so that every aim has a free interior pixel within MOVE_LIMIT
    of its place; the four corners of that pixel are then moved together until the float64 oracle's centre is there.
    Returns the case dict of _rowfield_cases with `aims`: list of dict(pixel (row, col), axis, edge index per axis, offset),
    the final grid's edges and its box."""
    for n in range(400):
        shift = 8.0 / ppd
        out = _try_aims(name, w, h, ppd, aims, lat0 + 0.0113 * (n % 20) * shift, lon0 + 0.0127 * (n // 20) * shift, magnetic)
        if out is not None:
            return out
    raise AssertionError('no placement of %s lets every aim reach a pixel' % name)


def aim_zone(offset, decimal):
    """(lower end, upper end) in deg, relative to the edge, of the zone an offset belongs to: on-edge [0, half a unit of the
    rounded decimal), beyond it up to bin_fast's margin of 1.5 units, or below the edge"""
    unit = 10.0 ** -decimal
    if offset < 0:
        return -np.inf, 0.0
    if offset < 0.5 * unit:
        return 0.0, 0.5 * unit
    return 0.5 * unit, 1.5 * unit


_AIMED = {}
EIGHTH = [('x', 'last', AIM_ON_EDGE), ('y', 'last', AIM_ON_EDGE), ('xy', 'last', AIM_ON_EDGE), ('x', 'first', AIM_ON_EDGE),
          ('x', 7, AIM_ON_EDGE), ('y', 2, AIM_ON_EDGE), ('x', 'last', AIM_NEAR), ('y', 'last', AIM_NEAR), ('x', 'last', AIM_BELOW),
          ('y', 'last', AIM_BELOW), ('x', 11, AIM_NEAR), ('x', 15, AIM_BELOW), ('x', 'before-last', AIM_ON_EDGE),
          ('y', 'before-last', AIM_ON_EDGE)]
AIMED_SPECS = {
    # 8 px/deg: edges are odd multiples of 1/16, exact in the final grid and in the superset; decimal 6
    'aimed-64x17': dict(w=64, h=17, ppd=8, aims=EIGHTH),
    'aimed-127x33': dict(w=127, h=33, ppd=8, aims=EIGHTH + [('y', 5, AIM_ON_EDGE), ('xy', 4, AIM_ON_EDGE)]),
    'aimed-64x17-b': dict(w=64, h=17, ppd=8, lat0=49.1, lon0=12.3, aims=EIGHTH[:6]),
    'aimed-64x17-c': dict(w=64, h=17, ppd=8, lat0=50.6, lon0=15.1, aims=EIGHTH[2:9]),
    'aimed-mag-64x17': dict(w=64, h=17, ppd=8, magnetic=True,
                            aims=[('y', 'last', AIM_ON_EDGE), ('y', 'last', AIM_NEAR), ('y', 2, AIM_ON_EDGE), ('y', 3, AIM_BELOW)]),
}
THREE_FRAMES = ('aimed-64x17', 'aimed-64x17-b', 'aimed-64x17-c')


def aimed_names():
    return tuple(AIMED_SPECS) + tuple(SCALE_CASES) + (FINER_CASE,)


def aimed_case(name):
    if name not in _AIMED:
        if name in SCALE_CASES:
            _AIMED[name] = scale_case(name)
        elif name == FINER_CASE:
            _AIMED[name] = finer_case()
        else:
            s = dict(AIMED_SPECS[name])
            _AIMED[name] = aimed_field(name, s.pop('w'), s.pop('h'), s.pop('ppd'), s.pop('aims'), **s)
    return _AIMED[name]


# ---- expected difference 1: a final grid whose `scale` differs from its superset's ---------------------------------------------
SCALE_PPD = 10
SCALE_SIZE = (16, 9)                                  # 0.74 x 0.27 deg: a final grid of a few cells


def scales_differ(box, ppd=SCALE_PPD):
    """(final grid, superset, differs on x, differs on y) for a box"""
    g, s = final_grid(box, ppd), superset_grid(box, ppd)
    return g, s, g.xaxis.scale != s.xaxis.scale, g.yaxis.scale != s.yaxis.scale


SCALE_CASES = {'aimed-scale': 'x', 'aimed-scale-y': 'y', 'aimed-scale-xy': 'xy'}
FINER_CASE = 'aimed-finer'
CAM_WEST = K.ecef(36.0, 0.0, 400.0)


def twin_edge(final_axis, super_axis, k, step):
    """the superset's edge at the node of edge k of the final axis"""
    off = int(round((final_axis.first - super_axis.first) / step))
    return float(axis_edges(super_axis)[off + k])


def scale_case(name='aimed-scale'):
    """A 16 x 9 field at 10 px/deg whose final grid rounds at 1e-6 deg on x, on y, or on both (every edge difference of that
    axis is at least 0.1) while the superset rounds at 1e-7 on both, also when the estimate the superset is laid out for is
    off by a cell either way.  On every axis that differs: one pixel 2e-7 deg beyond the final grid's last edge (on-edge under
    the coarser rounding alone), one 2e-8 deg beyond it (on-edge under both) and one 2e-7 deg above the lower edge of the last
    cell (an interior edge inside the band: it stays in its cell).  (The final grid's edges need not have the bits of the
    superset's edges at the same nodes — where the scales differ they mostly do not —: the two versions of an edge are a few ulps
    apart, less than 1e-13 deg, and every aimed pixel is at least 2e-8 deg from its edge, so it has the same relation to both.)"""
    w, h = SCALE_SIZE
    which = SCALE_CASES[name]
    want = (1e6 if 'x' in which else 1e7, 1e6 if 'y' in which else 1e7)
    aims = []
    for axis in which:
        aims += [(axis, 'last', AIM_ON_EDGE), (axis, 'last', AIM_BOTH), (axis, 'before-last', AIM_ON_EDGE)]
    if which == 'xy':
        aims = [('xy', 'last', AIM_ON_EDGE)] + aims
    for n in range(4000):
        lat0, lon0 = 50.0 + 0.0171 * (n % 40), 9.0 + 0.0137 * (n // 40)
        lat, lon = fine_smooth(w, h, lat0, lon0)
        box = (lat0 - PITCH[0] * h, lat0 + 0.0005 * w, lon0, float(lon.max()))        # (a quick estimate of the box)
        g, s, dx, dy = scales_differ(box)
        if (g.xaxis.scale, g.yaxis.scale) != want:
            continue
        out = _try_aims(name, w, h, SCALE_PPD, aims, lat0, lon0, False)
        if out is None:
            continue
        box, ok = out['box'], True
        for shift in (0.0, -0.1, 0.1):                # the coarse estimate may differ from the exact box
            g, s, dx, dy = scales_differ((box[0] + shift, box[1] + shift, box[2] + shift, box[3] + shift))
            ok &= s.xaxis.scale == 1e7 and s.yaxis.scale == 1e7
        g, s, dx, dy = scales_differ(box)
        ok &= (g.xaxis.scale, g.yaxis.scale) == want
        if ok:
            out.update(final_scale=(g.xaxis.scale, g.yaxis.scale), superset_scale=(s.xaxis.scale, s.yaxis.scale))
            return out
    raise AssertionError('no box with differing scales found: ' + name)


def finer_case():
    """The other way round: a 16 x 9 field next to the prime meridian, where longitudes are small numbers and a superset of 33
    cells can have no edge difference below 0.1 (it rounds at 1e-6 deg) while the final grid of 7 cells has one (1e-7).  One
    pixel 2e-7 deg beyond the final grid's last x edge — on-edge under the superset's rounding, not under the final grid's:
    the reference drops it —, one 2e-8 deg beyond it (on-edge under both: the last bin) and one 2e-7 deg above the lower edge
    of the last cell."""
    w, h = SCALE_SIZE
    aims = [('x', 'last', AIM_ON_EDGE), ('x', 'last', AIM_BOTH), ('x', 'before-last', AIM_ON_EDGE)]
    for n in range(6000):
        lat0, lon0 = 34.5 + 0.0171 * (n % 60), -3.2 + 0.0137 * (n // 60)
        lon = fine_smooth(w, h, lat0, lon0)[1]
        box = (lat0 - PITCH[0] * h, lat0 + 0.0005 * w, lon0, float(lon.max()))
        ok = True
        for shift in (0.0, -0.1, 0.1):
            g, s, dx, dy = scales_differ((box[0] + shift, box[1] + shift, box[2] + shift, box[3] + shift))
            ok &= (s.xaxis.scale, s.yaxis.scale) == (1e6, 1e7)
        g, s, dx, dy = scales_differ(box)
        if not ok or (g.xaxis.scale, g.yaxis.scale) != (1e7, 1e7):
            continue
        out = _try_aims(FINER_CASE, w, h, SCALE_PPD, aims, lat0, lon0, False, cam=CAM_WEST)
        if out is None:
            continue
        g, s, dx, dy = scales_differ(out['box'])
        if (g.xaxis.scale, g.yaxis.scale, s.xaxis.scale, s.yaxis.scale) == (1e7, 1e7, 1e6, 1e7):
            out.update(final_scale=(1e7, 1e7), superset_scale=(1e6, 1e7))
            return out
    raise AssertionError('no box whose superset rounds coarser found')


def edge_bit_differences(ppd, n_boxes, seed=11):
    """Over random boxes: (final edges compared, how many differ in bits from the superset's edge at the same node,
    layouts whose scale differs on an axis, layouts)"""
    rng = np.random.RandomState(seed)
    edges = differ = scales = 0
    for _ in range(n_boxes):
        lat_c, lon_c = rng.uniform(-70, 70), rng.uniform(-150, 150)
        dlat, dlon = rng.uniform(0.3, 6), rng.uniform(0.3, 12)
        box = (lat_c - dlat, lat_c + dlat, lon_c - dlon, lon_c + dlon)
        g, s, dx, dy = scales_differ(box, ppd)
        scales += int(dx or dy)
        for ga, sa, step in ((g.xaxis, s.xaxis, s.lon_step), (g.yaxis, s.yaxis, abs(s.lat_step))):
            fe, se = axis_edges(ga), axis_edges(sa)
            off = int(round((ga.first - sa.first) / step))
            twin = se[off:off + len(fe)]
            assert len(twin) == len(fe) and np.all(np.abs(twin - fe) < 1e-9)
            edges += len(fe)
            differ += int((twin != fe).sum())
    return edges, differ, scales, n_boxes
