"""
Constructed inputs for the interpolating kernels of auromat_amd/csrc/amt_nearest.hip: graphs, row partitions and channel
layouts for the gradient relaxation (amt_cubic_gradients_csr), triangles with dyadic data for the Clough-Tocher element
(amt_cubic_eval), dyadic point sets for the nearest-neighbour search (amt_nearest_frame, amt_nearest_gather) and integer
polygons for amt_points_in_polygon.  Plain host arrays, seeded and deterministic; every builder asserts the pattern it is
there for, and tests/test_interp_cases_cpu.py checks them again without a GPU.  The expected results come from
tests/_interp_oracle.py alone.
"""
import functools
from fractions import Fraction

import numpy as np

import _interp_oracle as O

U = O.UNITS

# ============================================================================================================================
# 1. gradient relaxation
# ============================================================================================================================
BASE = ('plane', 'smooth', 'noise', 'const')
LAYOUTS = (1, 8, 9, 19, 63)
CYCLE = (1, 2, 3, 4, 5, 7, 64, 65)
WHEEL_SIZES = (8, 9, 16, 17, 41)
WHEEL_ORDERS = ('first', 'middle', 'last')
GRAPHS = ('lattice', 'crescent', 'wheels-first', 'wheels-middle', 'wheels-last', 'isolated')
FIXED_SWEEPS = 5
STOP_TOLERANCE = 1e-6
K_GS_PRE = 8            # kGsPre: neighbours held in a point's record
K_GS_CHAN = 8           # kGsChan: channels per wave


class Graph(object):
    """Points in their order, a CSR of neighbour lists (ascending), the natural rows and four base value columns."""

    def __init__(self, name, xy, indptr, indices, rows, seed, hubs=()):
        self.name = name
        self.xy = np.ascontiguousarray(xy, dtype=np.float64)
        self.n = len(self.xy)
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.rows = np.ascontiguousarray(rows, dtype=np.int64)
        self.hubs = tuple(int(h) for h in hubs)
        assert self.indptr[0] == 0 and self.indptr[-1] == len(self.indices) and len(self.indptr) == self.n + 1
        for v in range(self.n):
            lst = self.indices[self.indptr[v]:self.indptr[v + 1]]
            assert np.all(np.diff(lst) > 0) and v not in lst, (name, v)          # ascending, as build_vertex_lists makes them
            for j in lst:                                                        # symmetric
                assert v in self.indices[self.indptr[j]:self.indptr[j + 1]], (name, v, j)
        check_rows(self.rows, self.n)
        x, y = self.xy[:, 0], self.xy[:, 1]
        rng = np.random.RandomState(seed)
        self.base = np.column_stack((3 + 2 * x - 0.5 * y, 100 * np.sin(x / 1.3) * np.cos(y / 0.9), rng.uniform(size=self.n) * 50,
                                     np.full(self.n, 7.25)))
        self.degree = np.diff(self.indptr)


def check_rows(rows, n):
    assert rows[0] == 0 and rows[-1] == n and np.all(np.diff(rows) >= 0), rows


def _csr(lists):
    indptr = np.zeros(len(lists) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(l) for l in lists])
    return indptr, np.array([j for l in lists for j in sorted(l)], dtype=np.int32)


def _delaunay_csr(xy):
    import scipy.spatial
    tri = scipy.spatial.Delaunay(xy)
    p, i = tri.vertex_neighbor_vertices
    return _csr([list(i[p[v]:p[v + 1]]) for v in range(len(xy))]) + (tri,)


def _lattice_points(h, w, seed, jitter=0.012):
    ii, jj = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.RandomState(seed)
    x = 40.0 + 0.10 * ii + 0.03 * jj + rng.uniform(-jitter, jitter, ii.shape)
    y = 10.0 + 0.02 * ii + 0.10 * jj + rng.uniform(-jitter, jitter, ii.shape)
    return x, y


LATTICE_SHAPE = (12, 14)
LATTICE_SEED = 3
CRESCENT_SHAPE = (20, 24)
CRESCENT_SEED = 8


def _lattice_raw():
    h, w = LATTICE_SHAPE
    x, y = _lattice_points(h, w, LATTICE_SEED)
    xy = np.column_stack((x.ravel(), y.ravel()))
    indptr, indices, tri = _delaunay_csr(xy)
    return xy, indptr, indices, np.arange(0, h * w + 1, w), tri


@functools.lru_cache(maxsize=None)
def lattice_triangulation():
    """scipy's Delaunay object of the lattice's points (for the comparison with CloughTocher2DInterpolator)."""
    return _lattice_raw()[4]


def _crescent():
    h, w = CRESCENT_SHAPE
    x, y = _lattice_points(h, w, CRESCENT_SEED)
    ii, jj = np.mgrid[0:h, 0:w]
    valid = (ii - 12.5) ** 2 + (jj - 24.0) ** 2 > 8.2 ** 2                      # a disc bitten out of the right side
    for r in range(6):                                                          # the first rows: 0, 1, 2, 3, 4, 5 valid points
        valid[r] = False
        valid[r, 4 + r:4 + 2 * r] = True
    xy = np.column_stack((x[valid], y[valid]))
    indptr, indices, _ = _delaunay_csr(xy)
    rows = np.zeros(h + 1, dtype=np.int64)
    rows[1:] = np.cumsum(valid.sum(axis=1))
    g = Graph('crescent', xy, indptr, indices, rows, seed=21)
    lengths = np.diff(rows)
    assert list(lengths[:6]) == [0, 1, 2, 3, 4, 5], lengths
    assert {int(l) % 3 for l in lengths if l > 5} == {0, 1, 2}, lengths
    assert g.degree.max() >= 9 and g.degree.min() >= 1 and g.n <= 450, (g.degree.max(), g.n)
    return g


def _wheels(order):
    rng = np.random.RandomState(17)
    pts, lists, rows, hubs = [], [], [0], []
    for w, k in enumerate(WHEEL_SIZES):
        ang = 2 * np.pi * (np.arange(k) + rng.uniform(-0.2, 0.2, k)) / k
        rad = 1 + rng.uniform(-0.05, 0.05, k)
        rim = np.column_stack((5.0 * w + 1.0 * rad * np.cos(ang), 2.0 + 0.7 * rad * np.sin(ang)))
        hub_xy = np.array([5.0 * w + 0.03, 2.0 - 0.02])
        pos = {'first': 0, 'middle': k // 2, 'last': k}[order]               # the hub's place within its component
        start = len(pts)
        index_of_rim = [start + r + (1 if r >= pos else 0) for r in range(k)]
        hub = start + pos
        comp = [None] * (k + 1)
        comp_lists = [None] * (k + 1)
        comp[pos], comp_lists[pos] = hub_xy, list(index_of_rim)
        for r in range(k):
            comp[index_of_rim[r] - start] = rim[r]
            comp_lists[index_of_rim[r] - start] = [index_of_rim[(r - 1) % k], index_of_rim[(r + 1) % k], hub]
        pts += comp
        lists += comp_lists
        rows.append(len(pts))
        hubs.append(hub)
    indptr, indices = _csr(lists)
    g = Graph('wheels-' + order, np.array(pts), indptr, indices, rows, seed=22, hubs=hubs)
    assert [int(g.degree[h]) for h in hubs] == list(WHEEL_SIZES)
    # 8: the record full; 9: one chunk of the slow path with one neighbour; 16, 17: two and three chunks; 41
    assert K_GS_PRE in WHEEL_SIZES and K_GS_PRE + 1 in WHEEL_SIZES and 2 * K_GS_PRE in WHEEL_SIZES and 2 * K_GS_PRE + 1 in WHEEL_SIZES
    assert set(np.delete(g.degree, hubs)) == {3}
    for h, k in zip(hubs, WHEEL_SIZES):
        nb = g.indices[g.indptr[h]:g.indptr[h + 1]]
        if order == 'first':
            assert np.all(nb > h)                      # every neighbour comes from the previous sweep
        elif order == 'last':
            assert np.all(nb < h)                      # every neighbour is a hand-over
        else:
            assert np.any(nb < h) and np.any(nb > h)
    return g


def _isolated():
    xy, indptr, indices, rows, _ = _lattice_raw()
    n = len(xy)
    xy2 = np.vstack(([[39.5, 9.5]], xy, [[42.0, 12.0]]))
    indptr2 = np.concatenate(([0], indptr, [indptr[-1]]))
    rows2 = np.concatenate(([0], rows + 1, [n + 2]))
    g = Graph('isolated', xy2, indptr2, indices + 1, rows2, seed=20)
    assert g.degree[0] == 0 and g.degree[-1] == 0 and g.degree[1:-1].min() > 0
    g.base[1:-1] = graph('lattice').base                                        # the lattice's values, indices shifted
    return g


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == 'lattice':
        xy, indptr, indices, rows, _ = _lattice_raw()
        return Graph('lattice', xy, indptr, indices, rows, seed=20)
    if name == 'crescent':
        return _crescent()
    if name.startswith('wheels-'):
        return _wheels(name.split('-')[1])
    assert name == 'isolated'
    return _isolated()


def cyclic_rows(n):
    """Rows of the cyclic lengths 1, 2, 3, 4, 5, 7, 64, 65 with empty rows at the start, in the middle and at the end."""
    rows, k = [0, 0], 0
    while rows[-1] < n:
        rows.append(min(n, rows[-1] + CYCLE[k % len(CYCLE)]))
        k += 1
        if k == 4:
            rows += [rows[-1]] * 2                                               # two empty rows in the middle
    rows.append(n)
    return np.array(rows, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def partitions(name):
    """{partition name: row_start} of a graph, all over the same point order."""
    g = graph(name)
    n = g.n
    out = {'natural': g.rows, 'one-row': np.array([0, n], dtype=np.int64), 'point-rows': np.arange(n + 1, dtype=np.int64),
           'cyclic': cyclic_rows(n)}
    if g.hubs:
        alone, before = {0, n}, {0, n}
        for h in g.hubs:
            alone |= {h, h + 1}
            before |= {max(h - 2, 0), h + 1}                                    # hub with the two points just before it
        out['hub-alone'] = np.array(sorted(alone), dtype=np.int64)
        out['hub-after-two'] = np.array(sorted(before), dtype=np.int64)
    for rows in out.values():
        check_rows(rows, n)
    lengths = np.diff(out['cyclic'])
    assert lengths[0] == 0 and lengths[-1] == 0 and 0 in lengths[1:-1] and set(CYCLE[:6]) <= set(lengths), lengths
    if n > 150:
        assert {64, 65} <= set(lengths), lengths
    return out


def layout(name, nchan, nan=False):
    """(n, nchan) values: column c is base column c mod 4; nan: one NaN in the last column (the lone channel of the second
    group when nchan = 9) at a mid-graph point."""
    g = graph(name)
    v = np.ascontiguousarray(g.base[:, np.arange(nchan) % 4])
    if nan:
        assert nchan == K_GS_CHAN + 1
        v[g.n // 2, nchan - 1] = np.nan
    return v


@functools.lru_cache(maxsize=None)
def reference(name, column, sweeps, long=True, nan=False):
    """O.relax of one base column of a graph: (gradients, errors).  nan: with the NaN of layout(nan=True) (column 0)."""
    g = graph(name)
    v = g.base[:, column].copy()
    if nan:
        assert column == (K_GS_CHAN % 4)
        v[g.n // 2] = np.nan
    y, err = O.relax(g.xy, g.indptr, g.indices, v, sweeps, np.longdouble if long else np.float64)
    y.setflags(write=False)
    return y, err


EPS = float(np.finfo(np.float64).eps)


def gradient_bound(name, column, sweeps, nan=False):
    """(bound, E_ref, scale): 8 * max(E_ref, eps * scale) with E_ref the largest difference between the float64 and the
    longdouble run of the reference and scale the largest gradient component of the longdouble run."""
    yl, _ = reference(name, column, sweeps, True, nan)
    yd, _ = reference(name, column, sweeps, False, nan)
    ok = ~np.isnan(yl)
    assert np.array_equal(ok, ~np.isnan(yd))
    e_ref = float(np.max(np.abs(yd.astype(np.longdouble) - yl)[ok], initial=0.0))
    scale = float(np.max(np.abs(yl[ok]), initial=0.0))
    return 8 * max(e_ref, EPS * scale), e_ref, scale


# ============================================================================================================================
# 2. the Clough-Tocher element
# ============================================================================================================================
class ElementCase(object):
    """Rows of amt_cubic_eval: targets (m, 2), vertices (m, 3) int32 (-1: outside), centroids (m, 3, 2), has_nb (m, 3) uint8,
    over points xy (n, 2), values (n, nchan), gradients (n, nchan, 2); kind[m]: 'vertex' | 'edge' | 'inside' | 'centroid' |
    'outside'; vertex_k[m]: which vertex a 'vertex' row sits on."""
    pass


def _element_points():
    # a centre, a hexagon round it, outer points: multiples of 1 / 8, so that midpoints and quarter points are dyadic too
    pts = [(0, 0), (16, 1), (9, 14), (-7, 15), (-16, -1), (-8, -14), (8, -15),        # centre and ring
           (26, 17), (1, 30), (-25, 14), (-24, -17), (30, -12), (48, -1)]              # outer points, the last one an ear
    return np.array(pts, dtype=np.float64) / 8.0 + np.array([3.0, -2.0])


@functools.lru_cache(maxsize=None)
def element_mesh():
    """(xy, triangles (nt, 3) counter-clockwise, neighbours (nt, 3): triangle across the edge opposite vertex k or -1)."""
    import scipy.spatial
    xy = _element_points()
    assert np.array_equal(xy * U, np.rint(xy * U))
    tri = scipy.spatial.Delaunay(xy)
    return xy, tri.simplices.astype(np.int32), tri.neighbors.astype(np.int32)


def _mesh_rows(rotations=(0, 1, 2)):
    """(triangle id, vertices (3,), neighbour ids (3,)) for every triangle in the given cyclic rotations of its vertices."""
    xy, simplices, neighbours = element_mesh()
    rows = []
    for t in range(len(simplices)):
        for r in rotations:
            k = [(r + q) % 3 for q in range(3)]
            rows.append((t, simplices[t][k], neighbours[t][k]))
    return rows


def element_case(nchan=3, kind='data', flags='real'):
    """kind 'data': seeded dyadic values and gradients; 'quadratic': values and exact gradients of a quadratic with dyadic
    coefficients.  flags 'real': the mesh's neighbours; 'none': every has_neighbour flag 0."""
    xy, simplices, neighbours = element_mesh()
    n = len(xy)
    rng = np.random.RandomState(31 + nchan)
    case = ElementCase()
    case.quadratic = None
    if kind == 'quadratic':
        coef = rng.randint(-64, 65, (nchan, 6)) / 16.0                           # a + b x + c y + d xx + e xy + f yy
        x, y = xy[:, 0], xy[:, 1]
        values = np.stack([c[0] + c[1] * x + c[2] * y + c[3] * x * x + c[4] * x * y + c[5] * y * y for c in coef], axis=1)
        grads = np.stack([np.column_stack((c[1] + 2 * c[3] * x + c[4] * y, c[2] + c[4] * x + 2 * c[5] * y)) for c in coef], axis=1)
        case.quadratic = coef
    else:
        values = rng.randint(1, 64 * 50, (n, nchan)) / 64.0 * rng.choice([-1.0, 1.0], (n, nchan))       # never zero
        grads = rng.randint(-64 * 40, 64 * 40, (n, nchan, 2)) / 64.0
    centroid = xy[simplices].sum(axis=1) / 3.0                                    # (nt, 2) as float64 computes them
    targets, vertices, cents, has_nb, kinds, vertex_k, tri_id = [], [], [], [], [], [], []

    def add(t, v, nb, p, what, k=-1):
        targets.append(p)
        vertices.append(v)
        cents.append([centroid[q] if q >= 0 else (0.0, 0.0) for q in nb])
        has_nb.append([1 if (q >= 0 and flags == 'real') else 0 for q in nb])
        kinds.append(what)
        vertex_k.append(k)
        tri_id.append(t)
    for row, (t, v, nb) in enumerate(_mesh_rows()):
        a, b, c = xy[v[0]], xy[v[1]], xy[v[2]]
        for k, p in enumerate((a, b, c)):
            add(t, v, nb, p, 'vertex', k)
        for p, q in ((a, b), (b, c), (c, a)):
            add(t, v, nb, (p + q) / 2, 'edge')
            add(t, v, nb, (3 * p + q) / 4, 'edge')
        add(t, v, nb, (2 * a + b + c) / 4, 'inside')
        add(t, v, nb, (a + 2 * b + c) / 4, 'inside')
        add(t, v, nb, (a + b + 6 * c) / 8, 'inside')
        add(t, v, nb, (a + b + c) / 3, 'centroid')
        if row % 5 == 2:                                                         # a target outside the hull
            targets.append(np.array([99.0, 99.0]))
            vertices.append(np.array([-1, -1, -1], dtype=np.int32))
            cents.append([(0.0, 0.0)] * 3)
            has_nb.append([0, 0, 0])
            kinds.append('outside')
            vertex_k.append(-1)
            tri_id.append(-1)
    case.xy, case.values, case.gradients, case.nchan = xy, np.ascontiguousarray(values), np.ascontiguousarray(grads), nchan
    case.targets = np.ascontiguousarray(targets, dtype=np.float64)
    case.vertices = np.ascontiguousarray(vertices, dtype=np.int32)
    case.centroids = np.ascontiguousarray(cents, dtype=np.float64)
    case.has_nb = np.ascontiguousarray(has_nb, dtype=np.uint8)
    case.kind, case.vertex_k, case.tri_id = np.array(kinds), np.array(vertex_k), np.array(tri_id)
    case.m = len(case.targets)
    case.flags = flags
    for a in (xy, values, grads):
        assert np.array_equal(a * U * U, np.rint(a * U * U)) if kind == 'quadratic' else np.array_equal(a * U, np.rint(a * U))
    dy = case.kind != 'centroid'
    assert np.array_equal(case.targets[dy] * U, np.rint(case.targets[dy] * U))
    assert case.m % 256 != 0 and case.m > 256 and (case.kind == 'outside').sum() >= 3
    if flags == 'real':
        inside = case.vertices[:, 0] >= 0
        hull = (case.has_nb[inside] == 0)
        assert set(hull.sum(axis=1)) >= {0, 1, 2}, set(hull.sum(axis=1))          # triangles with 0, 1 and 2 hull edges
        assert hull.any(axis=0).all()                                             # a hull edge in every position k
        fan = [t for t in range(len(simplices)) if 0 in simplices[t]]
        assert len(fan) == 6 and all((neighbours[t] >= 0).all() for t in fan)
    # the same dyadic target on the common edge of two triangles, once from each side
    seen, pairs = {}, []
    for r in np.flatnonzero(case.kind == 'edge'):
        key = (float(case.targets[r, 0]), float(case.targets[r, 1]))
        for q in seen.get(key, ()):
            if case.tri_id[q] != case.tri_id[r]:
                pairs.append((q, int(r)))
        seen.setdefault(key, []).append(int(r))
    case.pairs = pairs
    assert len(pairs) > 20
    return case


def _centroid_list(case, r):
    return [tuple(case.centroids[r, k]) if case.has_nb[r, k] else None for k in range(3)]


def element_exact(case):
    """(m, nchan) object array of Fractions (None in 'outside' rows): the exact value of every row and channel."""
    out = np.empty((case.m, case.nchan), dtype=object)
    for r in range(case.m):
        v = case.vertices[r]
        if v[0] < 0:
            continue
        for c in range(case.nchan):
            out[r, c] = O.clough_tocher_exact(case.xy[v], case.targets[r], case.values[v, c], case.gradients[v, c], _centroid_list(case, r))
    return out


def element_float(case):
    """(m, nchan) float64: oracle.ref_numpy.clough_tocher_value with float64 barycentric coordinates; NaN outside."""
    from oracle import ref_numpy as R
    out = np.full((case.m, case.nchan), np.nan)
    for r in range(case.m):
        v = case.vertices[r]
        if v[0] < 0:
            continue
        b = O.barycentric_float(case.xy[v], case.targets[r])
        for c in range(case.nchan):
            out[r, c] = R.clough_tocher_value(case.xy[v], b, case.values[v, c], case.gradients[v, c], _centroid_list(case, r))
    return out


def quadratic_exact(case):
    """(m, nchan) Fractions: the quadratic's value at every target (None outside)."""
    out = np.empty((case.m, case.nchan), dtype=object)
    for r in range(case.m):
        if case.vertices[r, 0] < 0:
            continue
        x, y = Fraction(float(case.targets[r, 0])), Fraction(float(case.targets[r, 1]))
        for c in range(case.nchan):
            k = [Fraction(float(q)) for q in case.quadratic[c]]
            out[r, c] = k[0] + k[1] * x + k[2] * y + k[3] * x * x + k[4] * x * y + k[5] * y * y
    return out


def fractions_to_float(a):
    out = np.full(a.shape, np.nan)
    for idx, v in np.ndenumerate(a):
        if v is not None:
            out[idx] = float(v)
    return out


def distance_to_exact(got, exact):
    """|got - exact| per entry as float64, the difference taken in rational arithmetic (NaN where exact is None)."""
    out = np.full(exact.shape, np.nan)
    for idx, v in np.ndenumerate(exact):
        if v is not None:
            g = float(got[idx])
            out[idx] = float(abs(Fraction(g) - v)) if np.isfinite(g) else np.inf
    return out


def element_bound(case, exact, reference_float):
    """Per channel (bound, E_ref, scale): 8 * max(E_ref, eps * scale); E_ref: distance of the float64 reference from the
    exact value over the case, scale: the largest absolute exact value."""
    e_ref = np.nanmax(distance_to_exact(reference_float, exact), axis=0)
    scale = np.nanmax(np.abs(fractions_to_float(exact)), axis=0)
    return 8 * np.maximum(e_ref, EPS * scale), e_ref, scale


# ============================================================================================================================
# 3. nearest neighbour
# ============================================================================================================================
class NearestCase(object):
    def __init__(self, name, grid_args, lat, lon, elev=None, center_mask=None, min_elevation=None, lon_wrap=0,
                 target_mask=None, notes=None):
        self.name, self.grid_args = name, grid_args
        self.lat = np.ascontiguousarray(lat, dtype=np.float64)
        self.lon = np.ascontiguousarray(lon, dtype=np.float64)
        assert self.lat.ndim == 2 and self.lat.shape == self.lon.shape
        self.height, self.width = self.lat.shape
        self.elev = None if elev is None else np.ascontiguousarray(elev, dtype=np.float64)
        self.center_mask = None if center_mask is None else np.ascontiguousarray(center_mask, dtype=np.uint8)
        self.min_elevation, self.lon_wrap = min_elevation, lon_wrap
        self.grid = grid_of(*grid_args)
        self.target_mask = None if target_mask is None else np.ascontiguousarray(target_mask, dtype=np.uint8)
        self.notes = notes or {}
        self.valid = O.valid_sources(self.lat, self.lon, self.elev, self.center_mask, min_elevation)
        O.to_units(self.lat), O.to_units(self.lon)                               # dyadic, or this raises

    def expected(self):
        g = self.grid
        return O.nearest_exact(self.lat, self.lon, self.valid, self.lon_wrap, g.latCenters, g.lonCenters, self.target_mask)

    def cells(self):
        """Histogram cell (iy, ix) of every source (valid or not) as the device sorts them."""
        y, x = O.source_units(self.lat, self.lon, self.lon_wrap)
        return O.cells_of(y, x, grid_units(self.grid)[2], grid_units(self.grid)[3])

    def flat_cells(self):
        iy, ix = self.cells()
        return np.where(self.valid, iy * self.grid.nx + ix, -1)


@functools.lru_cache(maxsize=None)
def grid_of(ppd, lat_min, lat_max, lon_min, lon_max):
    """_Grid(ppd, box) with the assertion that its centres and edges are exact multiples of 1 / 64 and its steps 1 / ppd."""
    from auromat_amd.resample import _Grid
    assert ppd in ((8, 8), (4, 16), (16, 8))
    g = _Grid(ppd, lat_min, lat_max, lon_min, lon_max)
    cy, cx, ey, ex = grid_units(g)
    assert np.all(np.diff(cx) == U // ppd[1]) and np.all(np.diff(cy) == -(U // ppd[0])), (ppd, np.diff(cx), np.diff(cy))
    assert np.all(np.diff(ex) == U // ppd[1]) and np.all(np.diff(ey) == U // ppd[0])
    assert np.array_equal(ex[:-1] + U // ppd[1] // 2, cx) and np.array_equal((ey[:-1] + U // ppd[0] // 2)[::-1], cy)
    assert g.lonStep == 1.0 / ppd[1] and g.latStep == -1.0 / ppd[0], (g.lonStep, g.latStep)
    return g


def grid_units(g):
    """(lat centres (descending), lon centres, y edges (ascending), x edges) in integer units; to_units asserts exactness."""
    return O.to_units(g.latCenters), O.to_units(g.lonCenters), O.to_units(g.yedges), O.to_units(g.xedges)


def box(ppd, ny, nx, lat0=40.0, lon0=10.0):
    """Grid arguments for ny x nx cells: the box is one step wider than the cells on either side."""
    return (ppd, lat0, lat0 + (ny + 1) / float(ppd[0]), lon0, lon0 + (nx + 1) / float(ppd[1]))


def _place(case_grid, iy, ix, dy, dx):
    """Coordinates (lat, lon) of the offset (dy, dx) units from the lower edges of histogram cell (iy, ix)."""
    _, _, ey, ex = grid_units(case_grid)
    return (ey[iy] + dy) / float(U), (ex[ix] + dx) / float(U)


def run_lengths(flat_cells):
    """[(start, length, cell)] of the runs of equal cells among consecutive sources (-1: invalid)."""
    c = np.asarray(flat_cells)
    starts = np.concatenate(([0], np.flatnonzero(np.diff(c) != 0) + 1))
    ends = np.concatenate((starts[1:], [len(c)]))
    return [(int(s), int(e - s), int(c[s])) for s, e in zip(starts, ends)]


RUNS = (1, 2, 63, 64, 65, 130)


def nearest_runs(small=False):
    """Consecutive sources in the same cell in runs of 1, 2, 63, 64, 65 and 130, one run across flat index 64 (two waves), one
    across 256 (two blocks), invalid sources (NaN, masked) inside and between runs; `small`: fewer than 64 sources."""
    args = box((8, 8), 20, 24)
    g = grid_of(*args)
    rng = np.random.RandomState(41)
    plan = []                                            # (cell id or None, length, how invalid)
    cell = [0]

    def run(length):
        cell[0] += 7                                     # a new cell for every run, never the neighbour's
        plan.append((cell[0] % (g.nx * g.ny), length, None))

    def bad(how):
        plan.append((None, 1, how))
    if small:
        shape = (5, 9)
        run(1), run(2), bad('nan'), run(20), bad('mask'), run(6)
        c6 = plan[-1][0]
        bad('nan')
        plan.append((c6, 5, None))
    else:
        shape = (13, 29)
        run(1), run(2), bad('nan'), run(63), bad('mask'), run(64), run(65), bad('nan'), run(130)
        run(10)
        c10 = plan[-1][0]
        bad('nan')                                       # invalid sources inside a run of one cell
        plan.append((c10, 10, None))
        bad('mask')
        plan.append((c10, 5, None))
    total = shape[0] * shape[1]
    used = sum(p[1] for p in plan)
    assert used <= total
    for _ in range(total - used):
        run(1)
    lat, lon, mask = np.empty(total), np.empty(total), np.zeros(total, np.uint8)
    k = 0
    step = U // 8
    for c, length, how in plan:
        for _ in range(length):
            if how == 'nan':
                lat[k] = lon[k] = np.nan
            else:
                cc = c if c is not None else 5
                lat[k], lon[k] = _place(g, cc // g.nx, cc % g.nx, rng.randint(0, step), rng.randint(0, step))
                mask[k] = 1 if how == 'mask' else 0
            k += 1
    case = NearestCase('runs-small' if small else 'runs', args, lat.reshape(shape), lon.reshape(shape), center_mask=mask.reshape(shape))
    runs = run_lengths(case.flat_cells())
    lengths = [l for _, l, c in runs if c >= 0]
    if small:
        assert total < 64 and {1, 2, 20} <= set(lengths)
    else:
        assert total % 64 != 0 and set(RUNS) <= set(lengths), lengths
        assert any(s < 64 < s + l and c >= 0 for s, l, c in runs) and any(s < 256 < s + l and c >= 0 for s, l, c in runs)
    assert any(c < 0 for _, _, c in runs) and (~case.valid).sum() >= 3
    # an invalid source between two runs of the same cell
    assert any(a[2] >= 0 and b[2] < 0 and c[2] == a[2] for a, b, c in zip(runs, runs[1:], runs[2:]))
    case.notes['runs'] = runs
    return case


CROWDS = (65, 129, 200)


def nearest_crowded():
    """One cell with 65 sources, one with 129, one with 200 (the search takes 64 per step); the nearest to the cell's centre is
    the last one of the cell, the ones before it lie at the cell's rim."""
    args = box((8, 8), 9, 11)
    g = grid_of(*args)
    rng = np.random.RandomState(43)
    lat, lon, winners = [], [], {}
    rim = [(dy, dx) for dy in range(8) for dx in range(8) if max(abs(dy - 4), abs(dx - 4)) >= 3]
    for (iy, ix), count in zip(((2, 3), (5, 8), (7, 1)), CROWDS):
        for k in range(count - 3):
            dy, dx = rim[rng.randint(len(rim))]
            la, lo = _place(g, iy, ix, dy, dx)
            lat.append(la), lon.append(lo)
        for dy, dx in ((2, 2), (4, 5), (4, 4)):                                 # nearer and nearer; the last on the centre
            la, lo = _place(g, iy, ix, dy, dx)
            lat.append(la), lon.append(lo)
        winners[(iy, ix)] = len(lat) - 1
    pad = (-len(lat)) % 7
    lat += [np.nan] * pad
    lon += [np.nan] * pad
    shape = (len(lat) // 7, 7)
    case = NearestCase('crowded', args, np.reshape(lat, shape), np.reshape(lon, shape))
    counts = np.bincount(case.flat_cells()[case.valid], minlength=g.nx * g.ny)
    assert sorted(counts[counts > 0]) == list(CROWDS)
    want = case.expected()
    for (iy, ix), w in winners.items():
        assert want[g.ny - 1 - iy, ix] == w
    case.notes['winners'] = winners
    return case


RING_GRIDS = ((8, 8), (4, 16), (16, 8))
RINGS = (0, 1, 3)


def nearest_ring(ppd, r, axis):
    """A grid centre with source A exactly (r + 1/2) steps away along `axis` on the far edge of ring r — stored in ring
    r + 1 — and source B at the same distance inside ring r.  A has the lower index and must win."""
    ny, nx = 14, 16
    args = box(ppd, ny, nx)
    g = grid_of(*args)
    sy, sx = U // ppd[0], U // ppd[1]
    iy, ix = 6, 7                                                                # the centre's histogram cell
    cy, cx = _place(g, iy, ix, sy // 2, sx // 2)
    if axis == 'x':
        a = (cy, cx + (r + 0.5) / ppd[1])
        b = (cy, cx - (r + 0.5) / ppd[1])
    else:
        a = (cy + (r + 0.5) / ppd[0], cx)
        b = (cy - (r + 0.5) / ppd[0], cx)
    lat = np.array([[np.nan, a[0], b[0]]])
    lon = np.array([[np.nan, a[1], b[1]]])
    case = NearestCase('ring-%dx%d-r%d-%s' % (ppd[0], ppd[1], r, axis), args, lat, lon)
    ciy, cix = case.cells()
    ring = np.maximum(np.abs(ciy - iy), np.abs(cix - ix))
    assert ring[1] == r + 1 and ring[2] == r, ring
    y, x = O.source_units(lat, lon, 0)
    ty, tx = O.to_units(cy), O.to_units(cx)
    d = (y - ty) ** 2 + (x - tx) ** 2
    assert d[1] == d[2] == ((r * 2 + 1) * (sx if axis == 'x' else sy) // 2) ** 2
    row = g.ny - 1 - iy
    assert g.latCenters[row] == cy and g.lonCenters[ix] == cx
    case.notes.update(row=row, col=ix, winner=1, loser=2, ring=(int(ring[1]), int(ring[2])))
    assert case.expected()[row, ix] == 1
    return case


def nearest_ties():
    """Exact ties seen from one centre of a 40 x 50 grid: between two different cells of the same ring, and along a diagonal
    between ring 9 (offset (51, 68) units) and ring 11 ((85, 0) and (13, 84): 51^2 + 68^2 = 85^2 = 13^2 + 84^2)."""
    args = box((8, 8), 40, 50)
    g = grid_of(*args)
    cases = []
    for name, offsets in (('same-ring', ((0, 25), (25, 0), (-24, -7), (15, 20))), ('diagonal', ((0, 85), (68, 51), (84, 13), (51, 68)))):
        iy, ix = 20, 24
        cy, cx = _place(g, iy, ix, 4, 4)
        lat = np.array([[np.nan] + [cy + dy / float(U) for dy, dx in offsets]])
        lon = np.array([[np.nan] + [cx + dx / float(U) for dy, dx in offsets]])
        case = NearestCase('ties-' + name, args, lat, lon)
        ciy, cix = case.cells()
        ring = np.maximum(np.abs(ciy - iy), np.abs(cix - ix))[1:]
        d = [dy * dy + dx * dx for dy, dx in offsets]
        assert len(set(d)) == 1
        if name == 'same-ring':
            assert len(set(ring)) == 1 and len(set(zip(ciy[1:], cix[1:]))) == len(offsets)
        else:
            assert ring[0] == 11 and ring[1] == 9 and ring[2] == 11 and ring[3] == 9, ring      # the lowest index two rings further out
        row = g.ny - 1 - iy
        assert case.expected()[row, ix] == 1
        case.notes.update(row=row, col=ix, winner=1, ring=[int(v) for v in ring])
        cases.append(case)
    return cases


def nearest_far():
    """[a single source in a corner cell of a 40 x 50 grid; sources outside the grid on all four sides and far outside;
    no valid source at all]."""
    args = box((8, 8), 40, 50)
    g = grid_of(*args)
    la, lo = _place(g, 0, g.nx - 1, 3, 5)
    one = NearestCase('far-corner', args, [[np.nan, la], [np.nan, np.nan]], [[np.nan, lo], [np.nan, np.nan]])
    assert g.ny == 40 and g.nx == 50 and (one.expected() == 1).all()
    _, _, ey, ex = grid_units(g)
    y0, y1, x0, x1 = ey[0], ey[-1], ex[0], ex[-1]
    pts = [(y0 - 3, (x0 + x1) // 2), (y1 + 5, x0 + 40), ((y0 + y1) // 2, x0 - 9), (y0 + 70, x1 + 1),      # just outside
           (y0 - 40 * 8, x0 - 30 * 8), (y1 + 25 * 8, x1 + 60 * 8), (y1 + 2, x1),                         # far outside; on the last edge
           ((y0 + y1) // 2 + 3, (x0 + x1) // 2 + 1)]                                                       # one inside
    lat = np.array([[p[0] / float(U) for p in pts]])
    lon = np.array([[p[1] / float(U) for p in pts]])
    out = NearestCase('outside', args, lat, lon)
    want = out.expected()
    assert len(set(want.ravel())) >= 6                                           # the outside sources win somewhere
    none = NearestCase('no-valid-source', box((8, 8), 6, 5), np.full((3, 4), np.nan), np.full((3, 4), np.nan))
    assert (none.expected() == -1).all()
    return [one, out, none]


def _scatter(g, n, rng):
    iy = rng.randint(0, g.ny, size=n)
    ix = rng.randint(0, g.nx, size=n)
    _, _, ey, ex = grid_units(g)
    sy, sx = ey[1] - ey[0], ex[1] - ex[0]
    return (ey[iy] + rng.randint(0, sy, n)) / float(U), (ex[ix] + rng.randint(0, sx, n)) / float(U)


def nearest_validity():
    """center_mask; an elevation threshold with NaN elevations; a threshold of -inf with an elevation array present (NaN
    elevations are then valid); a target_mask."""
    args = box((8, 8), 12, 15)
    g = grid_of(*args)
    rng = np.random.RandomState(47)
    shape = (9, 11)
    n = shape[0] * shape[1]
    lat, lon = _scatter(g, n, rng)
    lat[::13] = np.nan
    elev = rng.randint(0, 40 * 4, n) / 4.0
    elev[::5] = np.nan
    elev[3] = 12.0                                                               # on the threshold: valid
    mask = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    tmask = (rng.uniform(size=(g.ny, g.nx)) < 0.25).astype(np.uint8)
    r = lambda a: a.reshape(shape)
    cases = [NearestCase('center-mask', args, r(lat), r(lon), center_mask=r(mask)),
             NearestCase('threshold', args, r(lat), r(lon), elev=r(elev), min_elevation=12.0),
             NearestCase('threshold-and-masks', args, r(lat), r(lon), elev=r(elev), center_mask=r(mask), min_elevation=12.0,
                         target_mask=tmask),
             NearestCase('minus-inf', args, r(lat), r(lon), elev=r(elev), min_elevation=-np.inf),
             NearestCase('target-mask', args, r(lat), r(lon), target_mask=tmask)]
    assert cases[3].valid.sum() == (~np.isnan(lat)).sum() > cases[1].valid.sum() > cases[2].valid.sum() > 10
    assert (np.isnan(elev) & cases[3].valid).any() and not (np.isnan(elev) & cases[1].valid).any()
    assert (elev == 12.0).any()
    assert len({c.expected().tobytes() for c in cases}) == len(cases)
    return cases


def nearest_lon_wrap():
    """Sources on both sides of the date line (some exactly at 180 and -180), the grid laid out in the shifted coordinates
    (longitude + 180 wrapped into [-180, 180): the date line is 0)."""
    args = (( 8, 8), 60.0, 62.0, -3.0, 3.0)
    g = grid_of(*args)
    rng = np.random.RandomState(53)
    shape = (8, 12)
    n = shape[0] * shape[1]
    lat = 60.0 + rng.randint(0, 2 * U, n) / float(U)
    off = rng.randint(-3 * U - 20, 3 * U + 20, n)                                 # shifted longitude in units, some beyond the grid
    off[:6] = 0
    lon = np.where(off >= 0, -180.0 + off / float(U), 180.0 + off / float(U))     # east of the line: -180 + d; west: 180 - d
    lon[:3] = 180.0
    lon[3:6] = -180.0
    lat[5] = np.nan
    case = NearestCase('lon-wrap', args, lat.reshape(shape), lon.reshape(shape), lon_wrap=1)
    assert (lon > 170).sum() > 20 and (lon < -170).sum() > 20 and np.all(np.abs(lon) <= 180)
    _, x = O.source_units(case.lat, case.lon, 1)
    assert np.array_equal(x[:6], np.zeros(6, np.int64)) and np.array_equal(x[6:], off[6:])
    assert len(set(case.expected().ravel())) > 40
    return case


K_SCAN_TILE = 2048      # kScanTile = kBlock * kScanItems of amt_cell_scan.h: cells per workgroup of the scan
SCAN_GRIDS = ((5, 7), (32, 32), (25, 41), (60, 97))
SCAN_TILE_GRIDS = ((32, 64), (3, 683), (33, 62))       # one tile of the scan, a tile and a cell, a tile less two cells


def scan_chunk(ny, nx):
    """The chunk of cells whose last one most sources of a scan case go to: the scan's tile for the grids at its boundaries,
    half a tile (1024 cells) for SCAN_GRIDS"""
    return K_SCAN_TILE if (ny, nx) in SCAN_TILE_GRIDS else 1024


def nearest_scan(ny, nx):
    """Grids of fewer than 64 cells, exactly 1024, 1025 and several thousand (no multiple of 1024), and of one tile of the scan
    (2048 cells), one cell more and two fewer; most sources sit in the last chunk of the scan (the top rows of the histogram;
    (60, 97) = 5820 cells spans three tiles)."""
    args = box((8, 8), ny, nx)
    g = grid_of(*args)
    assert (g.ny, g.nx) == (ny, nx)
    rng = np.random.RandomState(59 + ny)
    shape = (10, 13)
    n = shape[0] * shape[1]
    _, _, ey, ex = grid_units(g)
    chunk = scan_chunk(ny, nx)
    flat = rng.randint(chunk * ((ny * nx - 1) // chunk), ny * nx, n)             # cells of the last chunk
    lat = (ey[flat // nx] + rng.randint(0, 8, n)) / float(U)
    lon = (ex[flat % nx] + rng.randint(0, 8, n)) / float(U)
    la2, lo2 = _scatter(g, n, rng)
    few = rng.uniform(size=n) < 0.15
    lat[few], lon[few] = la2[few], lo2[few]
    case = NearestCase('scan-%dx%d' % (ny, nx), args, lat.reshape(shape), lon.reshape(shape))
    cells = case.flat_cells()
    last_chunk = (ny * nx - 1) // chunk
    assert (cells // chunk == last_chunk).mean() > 0.5
    return case


def all_nearest_cases():
    cases = [nearest_runs(), nearest_runs(small=True), nearest_crowded()]
    cases += [nearest_ring(ppd, r, axis) for ppd in RING_GRIDS for r in RINGS for axis in 'xy']
    cases += nearest_ties() + nearest_far() + nearest_validity() + [nearest_lon_wrap()]
    cases += [nearest_scan(*s) for s in SCAN_GRIDS + SCAN_TILE_GRIDS]
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.height <= 70 and c.width <= 70 and c.grid.nx * c.grid.ny <= 6000, c.name
    return cases


GATHER_CHANNELS = (0, 1, 3, 4)


def gather_case(dtype, nchan, seed=61):
    """(index (t,) int64 with -1 entries, img (n, nchan) of dtype, elev (n,))."""
    rng = np.random.RandomState(seed + nchan)
    n, t = 321, 1000 + 37
    index = rng.randint(0, n, t).astype(np.int64)
    index[rng.uniform(size=t) < 0.2] = -1
    index[0], index[-1] = -1, n - 1
    img = rng.randint(0, np.iinfo(dtype).max + 1, (n, nchan)).astype(dtype)
    elev = rng.uniform(-5, 90, n)
    return index, img, elev


# ============================================================================================================================
# 4. points in a polygon
# ============================================================================================================================
POLYGON_SIZES = (256, 257, 513)
K_BLOCK = 256


def polygon(m):
    """A simple polygon of m integer vertices: a zigzag along the bottom from left to right, a zigzag along the top back."""
    lower = (m + 1) // 2
    upper = m - lower
    bottom = [(2 * i, -(i % 3)) for i in range(lower)]
    width = bottom[-1][0]
    top = [(width - (width * i) // (upper - 1), 9 + 2 * (i % 2)) for i in range(upper)]
    poly = np.array(bottom + top, dtype=np.float64)
    assert len(poly) == m and len({tuple(p) for p in poly}) == m
    return poly


def polygon_points(poly):
    """Integer and half-integer points over the polygon's box (on vertices, on edges, on the horizontal through vertices), NaN
    and infinite points, and in front a whole block of points that share one y (a vertex's)."""
    w = int(poly[:, 0].max())
    rng = np.random.RandomState(67)
    xs = np.concatenate((np.arange(-2, 40) / 2.0, rng.randint(-4, 2 * w + 4, 150) / 2.0, [w - 1, w - 0.5, w, w + 0.5]))
    ys = np.arange(-8, 26) / 2.0
    gx, gy = np.meshgrid(xs, ys)
    block = np.column_stack((rng.randint(-4, 2 * w + 4, K_BLOCK) / 2.0, np.full(K_BLOCK, -1.0)))
    # not finite: outside, whatever the other coordinate (a y between the zigzags, where a finite x would be inside)
    nan = np.array([[np.nan, 1.0], [1.0, np.nan], [np.nan, np.nan], [np.nan, 5.0], [np.nan, -1.0], [np.nan, 100.0], [5.0, np.inf],
                    [np.inf, 5.0], [-np.inf, 5.0], [np.inf, -1.0], [-np.inf, 9.0], [np.inf, np.nan]])
    edge = (poly + np.roll(poly, -1, axis=0)) / 2.0                              # midpoints of the edges
    pts = np.vstack((block, poly, edge, nan, np.column_stack((gx.ravel(), gy.ravel()))))
    assert len(pts) % K_BLOCK != 0
    return np.ascontiguousarray(pts)
