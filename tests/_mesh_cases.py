"""
Constructed inputs for the mesh resampling (auromat_amd/csrc/amt_mesh.hip) as plain host arrays, seeded and deterministic.  A
plain helper module (NumPy only) for tests/test_gpu_mesh_cells.py, which runs the cases on the device, and
tests/test_mesh_cpu.py, which checks without a GPU that the cases aim where they claim to.  Expected results come from
tests/_mesh_oracle.py; the dyadic case also has its exact answer (``exact_membership``, rational arithmetic).

A frame is a lattice of pixel centres (x = longitude, y = latitude); a grid is two ascending edge arrays and the cell centres,
by default the middle of every cell.
"""
from fractions import Fraction

import numpy as np

LANE_CELLS = 16             # kLaneCells of amt_mesh.hip: a triangle with more candidate cells is walked by the whole wave
BLOCK = 256                 # kMeshBlock: consecutive quads (row-major) of one workgroup


class MeshCase(object):
    def __init__(self, name, x, y, xedges, yedges, dtype=np.uint8, nch=3, elev=True, mask=None, min_elevation=float('-inf'),
                 lon_wrap=0, uniform=True, coord_offset=0, seed=0, cell_lon=None, cell_lat=None, img=None):
        rng = np.random.RandomState(seed)
        self.name = name
        self.lon_c, self.lat_c = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        self.height, self.width = h, w = self.lat_c.shape
        self.elev = rng.uniform(-89.9, 89.999, (h, w)) if elev is True else (None if elev is None or elev is False else
                                                                             np.asarray(elev, dtype=np.float64).reshape(h, w))
        dtype = np.dtype(dtype)
        self.img = rng.randint(0, int(np.iinfo(dtype).max) + 1, (h * w, nch)).astype(dtype) if img is None else img
        self.mask = None if mask is None else np.asarray(mask).reshape(h, w).astype(np.uint8)
        self.min_elevation = float(min_elevation)
        self.xedges, self.yedges = np.asarray(xedges, dtype=np.float64), np.asarray(yedges, dtype=np.float64)
        self.cell_lon = (self.xedges[:-1] + self.xedges[1:]) / 2 if cell_lon is None else np.asarray(cell_lon, dtype=np.float64)
        # rows run north to south
        self.cell_lat = ((self.yedges[:-1] + self.yedges[1:]) / 2)[::-1].copy() if cell_lat is None \
            else np.asarray(cell_lat, dtype=np.float64)
        assert len(self.cell_lon) == len(self.xedges) - 1 and len(self.cell_lat) == len(self.yedges) - 1
        assert ((self.xedges[:-1] <= self.cell_lon) & (self.cell_lon < self.xedges[1:])).all()
        assert ((self.yedges[:-1] <= self.cell_lat[::-1]) & (self.cell_lat[::-1] < self.yedges[1:])).all()
        self.lon_wrap, self.uniform, self.coord_offset = lon_wrap, uniform, coord_offset
        self.shape = (len(self.yedges) - 1, len(self.xedges) - 1)

    def __repr__(self):
        return self.name


def unit_edges(n, step=1.0, first=0.0):
    return np.linspace(first, first + n * step, n + 1)


def lattice_xy(h, w, x0, y0, dx, dy, jitter=0.0, seed=1):
    """h x w centres on the lattice (x0 + c dx, y0 + r dy), every one moved by up to `jitter` of a step."""
    rng = np.random.RandomState(seed)
    c, r = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return x0 + (c + jitter * rng.uniform(-1, 1, c.shape)) * dx, y0 + (r + jitter * rng.uniform(-1, 1, r.shape)) * dy


def lattice(name, h, w, xedges, yedges, x0, y0, dx, dy, jitter=0.0, seed=1, **kw):
    x, y = lattice_xy(h, w, x0, y0, dx, dy, jitter, seed)
    return MeshCase(name, x, y, xedges, yedges, seed=seed, **kw)


def bulged_xy(h=33, w=41):
    """A smooth lattice with a bulged, strictly convex boundary: x = u (1 - 0.15 v^2), y = v (1 - 0.15 u^2) on [-1, 1]^2, scaled
    to a few degrees.  Its lattice triangulation (empty-circle diagonals) is its Delaunay triangulation."""
    v, u = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing='ij')
    return u * (1 - 0.15 * v * v) * 3 + 20, v * (1 - 0.15 * u * u) * 2 + 60


def jittered_xy(h=7, w=9, jitter=0.2, seed=1):
    """The same shape without the bulge, every point moved by up to `jitter` of the spacing."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing='ij')
    x, y = u * 3 + 20, v * 2 + 60
    return x + jitter * rng.uniform(-1, 1, x.shape) * (6.0 / (w - 1)), y + jitter * rng.uniform(-1, 1, y.shape) * (4.0 / (h - 1))


# ---- exact membership on dyadic coordinates --------------------------------------------------------------------------------
def dyadic_case():
    """A 5 x 6 lattice on quarter coordinates with one fold (vertex (2, 2) pulled across its neighbour (2, 3): the triangles
    around it overlap others) and one non-convex quad (vertex (1, 4) pulled into quad (0, 3): only one diagonal is admissible),
    on a grid whose cell centres are the multiples of 1/4: centres ON vertices, ON shared edges (lattice lines and diagonals)
    and inside triangles.  Every coordinate is a small dyadic number: the edge values are exact in float64."""
    c, r = np.meshgrid(np.arange(6, dtype=np.float64), np.arange(5, dtype=np.float64))
    x, y = c.copy(), r.copy()
    x[2, 2], y[2, 2] = 4.5, 2.5
    x[1, 4], y[1, 4] = 3.25, 0.25
    x[3, 1], y[3, 1] = 1.0, 3.5
    edges_x = np.linspace(-0.375, 5.375, 24)          # 23 cells of 1/4, centres -1/4, 0, 1/4, ..., 5 1/4: a ring outside
    edges_y = np.linspace(-0.375, 4.375, 20)
    return MeshCase('dyadic_fold', x, y, edges_x, edges_y, seed=5)


def _side(p, q, t):
    return (q[0] - p[0]) * (t[1] - p[1]) - (q[1] - p[1]) * (t[0] - p[0])


def exact_membership(case, verts_of):
    """For every cell (ix, iy) the sorted list of (id, strictly inside?) of the non-degenerate triangles whose closed area holds
    the cell's centre, in rational arithmetic.  `verts_of`: dict id -> three flat vertex indices (any order)."""
    F = Fraction
    h, w = case.lat_c.shape
    P = [(F(float(a)), F(float(b))) for a, b in zip(case.lon_c.reshape(-1), case.lat_c.reshape(-1))]
    ny, nx = case.shape
    out = {}
    for ix in range(nx):
        for iy in range(ny):
            t = (F(float(case.cell_lon[ix])), F(float(case.cell_lat[ny - 1 - iy])))
            inside = []
            for tid, (a, b, c) in verts_of.items():
                if _side(P[a], P[b], P[c]) == 0:
                    continue
                s = [_side(P[a], P[b], t), _side(P[b], P[c], t), _side(P[c], P[a], t)]
                if all(v >= 0 for v in s) or all(v <= 0 for v in s):
                    inside.append((tid, all(v != 0 for v in s)))
            out[(ix, iy)] = sorted(inside)
    return out


# ---- rules with known answers ----------------------------------------------------------------------------------------------
def one_quad(A, B, C, D, name='quad', **kw):
    """A 2 x 2 lattice: the quad A, B, C, D alone, on an 8 x 8 grid over [0, 4]^2 unless edges are given."""
    x = np.array([[A[0], B[0]], [D[0], C[0]]], dtype=np.float64)
    y = np.array([[A[1], B[1]], [D[1], C[1]]], dtype=np.float64)
    xedges, yedges = kw.pop('xedges', unit_edges(8, 0.5)), kw.pop('yedges', unit_edges(8, 0.5))
    return MeshCase(name, x, y, xedges, yedges, **kw)


def diagonal_cases():
    """name -> (case, the diagonal the rule must choose)."""
    sq = dict(A=(1, 1), B=(3, 1), D=(1, 3))
    return {
        # convex, D = (1, 3) with C moved: the circle through A, B, C
        'd_inside': (one_quad(C=(3.5, 3.5), name='d_inside', **sq), 'BD'),      # a far C makes the circle large: D inside
        'd_outside': (one_quad(C=(2.5, 2.5), name='d_outside', **sq), 'AC'),    # a near C makes it small: D outside
        'd_on_circle': (one_quad(C=(3, 3), name='d_on_circle', **sq), 'AC'),    # the square: D on the circle, not strictly inside
        'clockwise_inside': (one_quad(A=(1, 3), B=(3, 3), C=(3.5, 0.5), D=(1, 1), name='clockwise_inside'), 'BD'),
        # a dart: the reflex vertex lies inside the triangle of the other three, only the diagonal through it is admissible
        'only_ac': (one_quad(A=(3.5, 1), B=(1, 3.5), C=(1.5, 1.5), D=(1, 1), name='only_ac'), 'AC'),   # reflex at C
        'only_bd': (one_quad(A=(1, 1), B=(3.5, 1), C=(1, 3.5), D=(1.5, 1.5), name='only_bd'), 'BD'),   # reflex at D
        'bow_tie': (one_quad(A=(1, 1), B=(3, 3), C=(3, 1), D=(1, 3), name='bow_tie'), 'AC'),           # none admissible
    }


def three_vertex_cases():
    """The square with each corner missing in turn (masked): name -> (case, the slot left out)."""
    out = {}
    for m, corner in enumerate('ABCD'):
        mask = np.zeros(4, dtype=np.uint8)
        mask[(0, 1, 3, 2)[m]] = 1           # flat indices of A, B, C, D in the 2 x 2 lattice: 0, 1, 3, 2
        out['without_' + corner] = (one_quad((1, 1), (3, 1), (3, 3), (1, 3), name='without_' + corner, mask=mask.reshape(2, 2)), m)
    return out


def seam_case():
    """A lattice across +-180 without the wrap: the triangles that straddle the seam are as wide as the globe and are dropped."""
    x, y = lattice_xy(5, 8, 176.3, 60.1, 1.1, 0.7, jitter=0.15, seed=8)
    x = np.where(x >= 180.0, x - 360.0, x)
    return MeshCase('seam_dropped', x, y, unit_edges(40, 0.25, 174.0), unit_edges(16, 0.25, 59.5), seed=43)


def wrap_case():
    """The same lattice binned in the shifted plane (lon_wrap): nothing is dropped."""
    x, y = lattice_xy(5, 8, 176.3, 60.1, 1.1, 0.7, jitter=0.15, seed=8)
    x = np.where(x >= 180.0, x - 360.0, x)
    return MeshCase('lon_wrap', x, y, unit_edges(40, 0.25, -4.5), unit_edges(16, 0.25, 59.5), lon_wrap=1, seed=42)


def removal_cases():
    """A 5 x 7 lattice, and the same with vertex (2, 3) removed in each way a vertex can be: name -> case."""
    h, w = 5, 7
    ex, ey = unit_edges(30, 0.25, -0.5), unit_edges(22, 0.25, -0.5)
    x, y = lattice_xy(h, w, 0.1, 0.2, 1.0, 1.0, jitter=0.2, seed=51)
    elev = np.full((h, w), 45.0)
    out = {'whole': MeshCase('whole', x, y, ex, ey, elev=elev, min_elevation=10.0, seed=52)}
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[2, 3] = 1
    out['masked'] = MeshCase('masked', x, y, ex, ey, elev=elev, mask=mask, min_elevation=10.0, seed=52)
    for name, field, value in (('nan_lat', 'y', np.nan), ('nan_lon', 'x', np.nan), ('inf_lon', 'x', np.inf),
                               ('low_elevation', 'e', 9.999), ('nan_elevation', 'e', np.nan)):
        xx, yy, ee = x.copy(), y.copy(), elev.copy()
        dict(x=xx, y=yy, e=ee)[field][2, 3] = value
        out[name] = MeshCase(name, xx, yy, ex, ey, elev=ee, min_elevation=10.0, seed=52)
    return out


# ---- shapes, grids, formats --------------------------------------------------------------------------------------------------
def shape_cases():
    """Lattices 2 x 2 .. 33 x 41 (17 x 19: more than 256 quads, no multiple of 64) on grids of about two cells per quad; the
    coordinates 8 bytes off a 16-byte boundary for every other one."""
    out = []
    for k, (h, w) in enumerate(((2, 2), (2, 3), (3, 3), (5, 7), (17, 19), (33, 41))):
        nx, ny = 2 * w + 3, 2 * h + 1
        out.append(lattice('shape_%dx%d' % (h, w), h, w, unit_edges(nx, 0.5, -1.0), unit_edges(ny, 0.5, 2.0), -0.8, 2.3,
                           (nx * 0.5 - 0.5) / max(w - 1, 1), (ny * 0.5 - 0.5) / max(h - 1, 1), jitter=0.25,
                           seed=h * 1000 + w, coord_offset=k % 2))
    return out


def grid_cases():
    """Grids from 1 x 1 to 200 x 200 under one 5 x 7 lattice: coarser than the lattice (most triangles claim nothing), about as
    fine, and so fine that every triangle is walked by the whole wave."""
    out = []
    for n in (1, 2, 3, 16, 200):
        out.append(lattice('grid_%dx%d' % (n, n), 5, 7, unit_edges(n, 7.0 / n, -0.5), unit_edges(n, 5.0 / n, -0.5), 0.05, 0.1, 1.0,
                           1.0, jitter=0.3, seed=60 + n, nch=1))
    out.append(lattice('grid_coarse', 17, 19, unit_edges(4, 5.0, -1.0), unit_edges(3, 6.0, -1.0), 0.0, 0.0, 1.0, 1.0, jitter=0.3,
                       seed=66, nch=1))
    rng = np.random.RandomState(3)
    ex = np.concatenate(([0.0], np.cumsum(rng.uniform(0.1, 0.9, 15))))
    ey = np.concatenate(([-2.0], -2.0 + np.cumsum(rng.uniform(0.1, 0.9, 11))))
    out.append(lattice('grid_edge_tables', 11, 17, ex, ey, -0.3, -2.2, 0.5, 0.55, jitter=0.3, seed=41, uniform=False))
    return out


def candidate_case():
    """Axis-parallel rectangles on unit cells (both triangles of a rectangle have its bounding box): 4 x 4 = exactly LANE_CELLS
    candidate cells (the last triangle a lane walks itself), 17 x 1 = LANE_CELLS + 1 (the first the wave walks), 1 (a quad
    inside one cell, between the centres: a candidate, nothing to claim), 0 (a row of quads above the grid) and several
    between."""
    xs = np.array([0.25, 3.75, 3.9, 19.6, 19.8])      # columns of 4, 1, 17 and 1 cells
    ys = np.array([0.25, 3.75, 3.9, 5.5, 6.5])        # rows of 4 and 1 cells, one across the upper border, one above it
    x, y = np.meshgrid(xs, ys)
    return MeshCase('candidates', x, y, unit_edges(21), unit_edges(5), nch=1, seed=70)


def wide_case():
    """Two quads over 70 x 70 cells each, beside small ones: triangles of a few thousand candidates and of a few, in one wave."""
    xs = np.array([0.3, 69.6, 70.4, 71.1, 139.2])
    ys = np.array([0.4, 0.9, 69.7])
    x, y = np.meshgrid(xs, ys)
    x = x + np.array([[0.0], [0.2], [0.1]])
    return MeshCase('wide', x, y, unit_edges(140), unit_edges(70), nch=1, seed=71)


def format_cases():
    ex, ey = unit_edges(12, 0.25, 10.0), unit_edges(9, 0.25, -3.0)
    out = []
    for dtype in (np.uint8, np.uint16):
        for nch in (0, 1, 3, 4):
            out.append(lattice('fmt_%s_%d' % (np.dtype(dtype).name, nch), 9, 13, ex, ey, 9.9, -3.1, 0.26, 0.27, jitter=0.25,
                               seed=17 + nch, dtype=dtype, nch=nch, coord_offset=nch % 2))
    out.append(lattice('fmt_no_elev', 9, 13, ex, ey, 9.9, -3.1, 0.26, 0.27, jitter=0.25, seed=31, elev=None))
    out.append(lattice('fmt_mask', 9, 13, ex, ey, 9.9, -3.1, 0.26, 0.27, jitter=0.25, seed=32,
                       mask=np.random.RandomState(5).rand(9, 13) < 0.3))
    return out


def device_cases():
    rules = [c for c, _ in diagonal_cases().values()] + [c for c, _ in three_vertex_cases().values()]
    return ([dyadic_case()] + rules + [seam_case(), wrap_case()] + list(removal_cases().values()) + shape_cases() + grid_cases() +
            [candidate_case(), wide_case()] + format_cases())


# ---- real geometry ---------------------------------------------------------------------------------------------------------
def golden_case(z, px_per_deg, min_elevation=10.0, name='golden', field=None):
    """The centres of a georeferenced golden frame (tests/golden/georef_small_*.npz) on the grid the package lays out for the box
    of the pixels at or above `min_elevation`.  `field`: f(lon, lat) -> values for the elevation channel in place of the frame's
    (the membership keeps using the frame's elevation: it is applied as a mask)."""
    from auromat_amd.resample import _Grid
    lat, lon, elev = z['lat_c'], z['lon_c'], z['elev']
    with np.errstate(invalid='ignore'):
        keep = np.isfinite(lat) & np.isfinite(lon) & (elev >= min_elevation)
    grid = _Grid((px_per_deg, px_per_deg), lat[keep].min(), lat[keep].max(), lon[keep].min(), lon[keep].max())
    kw = dict(elev=elev, min_elevation=min_elevation)
    if field is not None:
        with np.errstate(invalid='ignore'):
            kw = dict(elev=np.where(keep, field(np.where(keep, lon, 0.0), np.where(keep, lat, 0.0)), 0.0), mask=~keep)
    return MeshCase(name, lon, lat, grid.xedges, grid.yedges, cell_lon=grid.lonCenters, cell_lat=grid.latCenters, seed=7, **kw)
