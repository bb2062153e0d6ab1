"""
The mesh resampling (auromat_amd.resample.resampleMesh, ``amt_mesh_frame``) without a GPU: is the NumPy statement
of the contract (tests/_mesh_oracle.py), which the device tests compare bit for bit against, right?

  (a) against scipy on constructed lattices: on a smooth lattice with a strictly convex boundary the lattice triangulation IS the
      Delaunay triangulation, on a jittered one it is a part of it, and the values are those of LinearNDInterpolator;
  (b) an affine field is reproduced whatever the diagonals;
  (c) exact membership in rational arithmetic on dyadic coordinates: folds, a non-convex quad, centres on edges and vertices;
  (d) every rule with a known answer: the branches of the diagonal rule, quads with three vertices, the seam, the wrap, the
      ways a vertex can be missing;
  (e) real geometry: a georeferenced frame against scipy where both triangulations have the cell's triangle;
  (f) the cases of tests/_mesh_cases.py aim where they claim to, and the Python surface that needs no device.
"""
import os
import re

import numpy as np
import pytest

import _mesh_cases as K
import _mesh_oracle as O
from conftest import ROOT, load_golden

EPS12 = 1e-12


def _triples(verts):
    return set(tuple(sorted(t)) for t in np.asarray(verts).tolist())


def _grid_over(x, y, step):
    """Edges of a grid of `step` cells that covers the points with a margin of a cell or two, off the lattice's own lines."""
    return (K.unit_edges(int(np.ceil((x.max() - x.min()) / step)) + 3, step, x.min() - 1.37 * step),
            K.unit_edges(int(np.ceil((y.max() - y.min()) / step)) + 3, step, y.min() - 1.61 * step))


def _scipy_side(case):
    """(Delaunay of the case's vertices, LinearNDInterpolator values (ny, nx, nch + 1) at the cell centres, channel spans)."""
    from scipy.interpolate import LinearNDInterpolator
    from scipy.spatial import Delaunay
    pts = np.stack([case.lon_c.reshape(-1), case.lat_c.reshape(-1)], axis=1)
    vals = np.concatenate([case.img.astype(np.float64), case.elev.reshape(-1, 1)], axis=1)
    tri = Delaunay(pts)
    gx, gy = np.meshgrid(case.cell_lon, case.cell_lat)
    return tri, LinearNDInterpolator(tri, vals)(gx, gy), vals.max(axis=0) - vals.min(axis=0)


# ---- (a) -------------------------------------------------------------------------------------------------------------------
def test_smooth_convex_lattice_is_its_delaunay_triangulation():
    x, y = K.bulged_xy(33, 41)
    case = K.MeshCase('bulged', x, y, *_grid_over(x, y, 0.1), seed=3)
    ids, verts = O.triangles(case)
    tri, want, span = _scipy_side(case)
    assert len(ids) == 2 * 32 * 40 == 2560
    assert _triples(verts) == _triples(tri.simplices)
    got = O.mesh_frame(case)
    filled = got['mask'] == 0
    assert filled.sum() > 1500 and np.array_equal(filled, ~np.isnan(want[..., 0]))
    err = np.abs(got['mesh'] - want)[filled].max(axis=0) / span
    print('bulged 33 x 41: %d cells, max |oracle - scipy| / span per channel %s' % (filled.sum(), err))
    assert (err <= EPS12).all()


def test_jittered_lattice_is_part_of_its_delaunay_triangulation():
    x, y = K.jittered_xy(7, 9, 0.2)
    case = K.MeshCase('jittered', x, y, *_grid_over(x, y, 0.1), seed=4)
    ids, verts = O.triangles(case)
    tri, want, span = _scipy_side(case)
    assert len(ids) == 2 * 6 * 8 == 96
    assert _triples(verts) <= _triples(tri.simplices) and len(tri.simplices) > 96          # (scipy adds hull triangles)
    got = O.mesh_frame(case)
    filled = got['mask'] == 0
    assert filled.sum() > 1500 and not (filled & np.isnan(want[..., 0])).any()
    # the cells scipy fills beyond the oracle's lie in its hull triangles, outside the lattice
    lattice_simplex = np.array([tuple(sorted(s)) in _triples(verts) for s in tri.simplices.tolist()])
    gx, gy = np.meshgrid(case.cell_lon, case.cell_lat)
    simplex = tri.find_simplex(np.stack([gx, gy], axis=-1))
    extra = ~filled & ~np.isnan(want[..., 0])
    assert extra.any() and not lattice_simplex[simplex[extra]].any()
    err = np.abs(got['mesh'] - want)[filled].max(axis=0) / span
    print('jittered 7 x 9: %d cells (%d more in scipy\'s hull triangles), max |oracle - scipy| / span per channel %s'
          % (filled.sum(), extra.sum(), err))
    assert (err <= EPS12).all()


# ---- (b) -------------------------------------------------------------------------------------------------------------------
def _affine_cases():
    x, y = K.jittered_xy(7, 9, 0.45, seed=9)
    return [K.dyadic_case(), K.MeshCase('jittered_45', x, y, *_grid_over(x, y, 0.1))] + K.shape_cases()[3:5] + \
        [K.diagonal_cases()[k][0] for k in ('only_ac', 'only_bd', 'bow_tie')]


@pytest.mark.parametrize('base', _affine_cases(), ids=repr)
def test_an_affine_field_is_reproduced(base):
    a, b, c = 3.25, -0.7, 1.9
    field = lambda x, y: a + b * x + c * y
    case = K.MeshCase(base.name, base.lon_c, base.lat_c, base.xedges, base.yedges, elev=field(base.lon_c, base.lat_c), nch=0)
    got = O.mesh_frame(case)
    filled = got['mask'] == 0
    gx, gy = np.meshgrid(case.cell_lon, case.cell_lat)
    span = case.elev.max() - case.elev.min()
    err = np.abs(got['mesh'][..., 0] - field(gx, gy))[filled].max() / span
    print('%s: %d cells, max error %.3g of the span' % (case.name, filled.sum(), err))
    assert filled.sum() >= 4 and err <= EPS12


# ---- (c) -------------------------------------------------------------------------------------------------------------------
def test_exact_membership_on_dyadic_coordinates():
    case = K.dyadic_case()
    h, w = case.lat_c.shape
    assert h <= 9 and w <= 9
    ok, x, y = O.vertices(case)
    at = O.quad_vertices(h, w)
    _, _, info = O.quad_split(ok[at], x[at], y[at])
    assert (info['ac'] != info['bd']).any(), 'no non-convex quad'
    ids, verts = O.triangles(case)
    exact = K.exact_membership(case, dict(zip(ids.tolist(), verts.tolist())))
    claim = O.claims(case)
    ny, nx = case.shape
    folded = on_edge = on_vertex = masked = 0
    vertex_set = set(zip(case.lon_c.reshape(-1).tolist(), case.lat_c.reshape(-1).tolist()))
    for (ix, iy), holders in exact.items():
        want = min(t for t, _ in holders) if holders else O.NOBODY
        assert claim[ix, iy] == want, ((ix, iy), holders, claim[ix, iy])
        folded += sum(strict for _, strict in holders) >= 2
        on_edge += len(holders) >= 2 and not any(strict for _, strict in holders)
        on_vertex += (case.cell_lon[ix], case.cell_lat[ny - 1 - iy]) in vertex_set
        masked += not holders
    print('dyadic: %d cells, %d in a fold, %d on shared edges only, %d on vertices, %d masked' % (nx * ny, folded, on_edge, on_vertex,
                                                                                                masked))
    assert folded >= 3 and on_edge >= 20 and on_vertex >= 20 and masked >= 1
    # ... and trying every triangle on every cell gives the same words as the candidates of the bounding boxes
    assert np.array_equal(claim, O.claims(case, every_cell=True))


# ---- (d) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(K.diagonal_cases()))
def test_diagonal_rule(name):
    case, diagonal = K.diagonal_cases()[name]
    ok, x, y = O.vertices(case)
    at = O.quad_vertices(2, 2)
    m0, m1, info = O.quad_split(ok[at], x[at], y[at])
    det = O.in_circle_det(x[at], y[at])[0]
    flags = (bool(info['ac'][0]), bool(info['bd'][0]))
    assert flags == dict(d_inside=(True, True), d_outside=(True, True), d_on_circle=(True, True), clockwise_inside=(True, True),
                         only_ac=(True, False), only_bd=(False, True), bow_tie=(False, False))[name]
    if name == 'd_on_circle':
        assert det == 0.0
    if name in ('d_inside', 'clockwise_inside'):
        assert bool(info['inside'][0]) and (det > 0) == (name == 'd_inside')      # the sign follows orient(A, B, C)
    assert (m0[0], m1[0]) == {'AC': (3, 1), 'BD': (2, 0)}[diagonal]
    ids, verts = O.triangles(case)
    A, B, C, D = 0, 1, 3, 2
    assert ids.tolist() == [0, 1]
    assert verts.tolist() == {'AC': [[A, B, C], [A, C, D]], 'BD': [[A, B, D], [B, C, D]]}[diagonal]


@pytest.mark.parametrize('name', sorted(K.three_vertex_cases()))
def test_three_valid_vertices_give_their_one_triangle(name):
    case, missing = K.three_vertex_cases()[name]
    ids, verts = O.triangles(case)
    corner = [0, 1, 3, 2]                       # flat indices of A, B, C, D
    assert ids.tolist() == [0] and verts.tolist() == [[corner[s] for s in range(4) if s != missing]]
    got = O.mesh_frame(case)
    assert (got['mask'] == 0).sum() == 10 and set(got['triangle'][got['mask'] == 0].tolist()) == {0}
    two = K.MeshCase('two', case.lon_c, case.lat_c, case.xedges, case.yedges, mask=np.array([[1, 0], [0, 1]]))
    assert len(O.triangles(two)[0]) == 0 and (O.mesh_frame(two)['mask'] == 1).all()


def test_a_triangle_as_wide_as_the_seam_is_dropped_and_the_wrap_keeps_it():
    seam, wrap = K.seam_case(), K.wrap_case()
    assert np.array_equal(seam.lon_c, wrap.lon_c) and (seam.lon_c > 175).any() and (seam.lon_c < -175).any()
    h, w = seam.lat_c.shape
    ids_s, verts_s = O.triangles(seam)
    ids_w, verts_w = O.triangles(wrap)
    assert len(ids_w) == 2 * (h - 1) * (w - 1) and 0 < len(ids_s) < len(ids_w)
    x = seam.lon_c.reshape(-1)
    crosses = lambda v: (x[v] > 0).any(axis=1) & (x[v] < 0).any(axis=1)
    assert not crosses(verts_s).any() and crosses(verts_w).sum() == len(ids_w) - len(ids_s)
    # in the shifted plane the lattice is whole: cells on both sides of the old seam are filled
    got = O.mesh_frame(wrap)
    filled_x = wrap.cell_lon[(got['mask'] == 0).any(axis=0)]
    assert (filled_x < -0.5).any() and (filled_x > 0.5).any()
    xs = O.vertices(wrap)[1]
    assert xs.min() > -5 and xs.max() < 5


def test_every_way_to_lose_a_vertex_removes_its_triangles():
    cases = K.removal_cases()
    whole = cases.pop('whole')
    h, w = whole.lat_c.shape
    v = 2 * w + 3
    ids0, verts0 = O.triangles(whole)
    assert (verts0 == v).any(axis=1).sum() >= 4
    touching = [r * (w - 1) + c for r in (1, 2) for c in (2, 3)]
    want = None
    for name, case in sorted(cases.items()):
        ids, verts = O.triangles(case)
        assert not (verts == v).any(), name
        far0, far = ~np.isin(ids0 >> 1, touching), ~np.isin(ids >> 1, touching)
        assert np.array_equal(ids0[far0], ids[far]) and np.array_equal(verts0[far0], verts[far]), name
        at = O.quad_vertices(h, w)
        for q in touching:
            mine = verts[(ids >> 1) == q]
            assert ids[(ids >> 1) == q].tolist() == [2 * q] and sorted(mine[0].tolist()) == sorted(set(at[q].tolist()) - {v}), name
        want = (ids, verts) if want is None else want
        assert np.array_equal(ids, want[0]) and np.array_equal(verts, want[1]), name


# ---- (e) -------------------------------------------------------------------------------------------------------------------
def test_real_frame_against_scipy_where_the_triangles_coincide():
    """The golden frame at min_elevation 10 on a 0.1 deg grid, a smooth field in the elevation channel.  Where the winning
    triangle is also a Delaunay simplex, scipy's LinearNDInterpolator evaluates the same linear function.  The bound per cell is
    1e-12 of the span times max(1, L^2 / |2A|) of its triangle (L its longest edge, A its area): an edge value is the difference of
    two products of size <= L^2, each rounded to 1.1e-16 of itself, and is divided by 2A — on the well-shaped triangles of (a)
    the factor is about 1 and the bound the one used there; near the limb the triangles are long and thin."""
    from scipy.interpolate import LinearNDInterpolator
    from scipy.spatial import Delaunay
    z = load_golden('georef_small_iss030_fast.npz')
    field = lambda lon, lat: 40.0 + 25.0 * np.sin(np.radians(3.0 * lon)) * np.cos(np.radians(5.0 * lat)) + 0.3 * lat
    case = K.golden_case(z, 10, 10.0, field=field)
    ok, x, y = O.vertices(case)
    assert ok.sum() == 5951
    vi = np.flatnonzero(ok)
    tri = Delaunay(np.stack([x[vi], y[vi]], axis=1))
    ids, verts = O.triangles(case)
    common = _triples(verts) & _triples(vi[tri.simplices])
    assert len(common) >= 7766              # (the quads with four vertices alone have 7766)
    got = O.mesh_frame(case)
    gx, gy = np.meshgrid(case.cell_lon, case.cell_lat)
    want = LinearNDInterpolator(tri, case.elev.reshape(-1)[vi])(gx, gy)
    filled = got['mask'] == 0
    won = O.triangle_vertices(case, got['triangle'][filled])
    is_common = np.array([tuple(sorted(t)) in common for t in won.tolist()])
    # ... and scipy must have evaluated that very simplex (it can pick a neighbour for a centre on an edge: the same value)
    r, c = np.nonzero(filled)
    r, c, won = r[is_common], c[is_common], won[is_common]
    print('real frame: %d cells filled, %d (%.1f %%) in a triangle that is also a Delaunay simplex; %d of %d lattice triangles are'
          % (filled.sum(), len(r), 100.0 * len(r) / filled.sum(), len(common), len(ids)))
    assert len(r) >= 1000
    px, py = x[won], y[won]
    L2 = np.max([(px[:, i] - px[:, j]) ** 2 + (py[:, i] - py[:, j]) ** 2 for i, j in ((0, 1), (1, 2), (2, 0))], axis=0)
    A2 = np.abs(O.orient(px[:, 0], py[:, 0], px[:, 1], py[:, 1], px[:, 2], py[:, 2]))
    kappa = np.maximum(1.0, L2 / A2)
    values = case.elev.reshape(-1)[vi]
    span = values.max() - values.min()
    err = np.abs(got['mesh'][r, c, -1] - want[r, c]) / span
    assert not np.isnan(err).any()
    print('real frame: max error %.3g of the span, max error / bound %.3g, largest L^2 / |2A| %.1f' % (err.max(), (err / (EPS12 * kappa)).max(),
                                                                                                   kappa.max()))
    assert (err <= EPS12 * kappa).all()


# ---- (f) -------------------------------------------------------------------------------------------------------------------
def test_cases_aim_where_they_claim():
    src = open(os.path.join(ROOT, 'auromat_amd', 'csrc', 'amt_mesh.hip')).read()
    assert int(re.search(r'constexpr int kLaneCells = (\d+);', src).group(1)) == K.LANE_CELLS
    assert int(re.search(r'constexpr int kMeshBlock = (\d+);', src).group(1)) == K.BLOCK
    counts = set(O.candidate_counts(K.candidate_case()).tolist())
    assert {0, 1, K.LANE_CELLS, K.LANE_CELLS + 1} <= counts, counts
    wide = O.candidate_counts(K.wide_case())
    assert wide.max() >= 4000 and wide.min() <= K.LANE_CELLS              # both paths within one wave
    assert O.candidate_counts(K.grid_cases()[4]).min() > K.LANE_CELLS     # 200 x 200: every triangle on the wave path
    coarse = K.grid_cases()[5]
    won = O.mesh_frame(coarse)['triangle']
    assert coarse.name == 'grid_coarse' and len(np.unique(won[won >= 0])) * 10 < len(O.triangles(coarse)[0])
    shapes = {c.name: c for c in K.shape_cases()}
    assert 16 * 18 > K.BLOCK and (16 * 18) % 64 != 0 and shapes['shape_17x19'].lat_c.shape == (17, 19)
    assert {c.coord_offset for c in K.shape_cases()} == {0, 1}
    names = [c.name for c in K.device_cases()]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize('case', [c for c in K.device_cases() if c.shape[0] * c.shape[1] <= 2000], ids=repr)
def test_candidate_range_does_not_matter(case):
    a, b = O.mesh_frame(case), O.mesh_frame(case, every_cell=True)
    for key in a:
        assert O.same_bits(a[key], b[key]), key


def test_uint16_samples_are_unsigned_and_the_image_rounds_half_to_even():
    # a right triangle with the cell centre in the middle of its hypotenuse: the mean of two vertices
    img = np.array([[40000], [65535], [1], [3]], dtype=np.uint16)          # flat order: A, B, D, C
    case = K.one_quad((1, 1), (3, 1), (3, 3), (1, 3), name='half', img=img, nch=1, xedges=K.unit_edges(4), yedges=K.unit_edges(4),
                      cell_lon=[0.5, 1.5, 2.0, 3.5], cell_lat=[3.5, 2.0, 1.5, 0.5])
    got = O.mesh_frame(case)
    assert got['triangle'][1, 2] == 0 and got['mesh'][1, 2, 0] == 20001.5 and got['img'][1, 2, 0] == 20002
    assert got['img'].dtype == np.uint16


def test_python_surface_without_a_device(monkeypatch):
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import BaseMapping, MappingCollection
    with pytest.raises(NotImplementedError):
        R.resample(None, method='mesh')                     # the method list stays the reference's
    for bad in (42, None, [1, 2]):
        with pytest.raises(ValueError):
            R.resampleMesh(bad)

    class Stub(BaseMapping):
        altitude, boundingBox, containsDiscontinuity, containsPole, outline = 110, 'box', False, False, 'outline'

        def __init__(self, tag):
            self.tag = tag

        def frame(self):
            return 'frame of ' + self.tag

        def createResampled(self, lats, lons, latsCenter, lonsCenter, elevation, img):
            return ('resampled', self.tag, lats, elevation is None)

    calls = []

    def fake(fd, altitude, box, ppd, disc, pole, **kw):
        calls.append((fd, ppd, pole, kw))
        z = np.zeros((2, 2))
        return dict(lat=fd, lon=z, lat_c=z, lon_c=z, mesh=np.zeros((2, 2, 2)), img=np.zeros((2, 2, 1), np.uint8),
                    mask=np.zeros((2, 2), bool), triangle=np.zeros((2, 2), np.int32), has_elev=False)

    monkeypatch.setattr(R, 'resample_frame_mesh', fake)
    one = R.resampleMesh(Stub('a'), pxPerDeg=(4, 7))
    assert one == ('resampled', 'a', 'frame of a', True) and calls == [('frame of a', (4, 7), False, dict(outline=None))]
    coll = R.resampleMesh(MappingCollection([Stub('a'), Stub('b')], 'pair', mayOverlap=False), pxPerDeg=5, containsPole=True)
    assert isinstance(coll, MappingCollection) and coll.identifier == 'pair' and coll.mayOverlap is False
    assert [m[1] for m in coll.mappings] == ['a', 'b']
    assert [c[0] for c in calls[1:]] == ['frame of a', 'frame of b'] and all(c[1:] == ((5, 5), True, dict(outline='outline'))
                                                                              for c in calls[1:])
    import inspect
    assert list(inspect.signature(R.resampleMesh).parameters) == ['mappingOrCollection', 'pxPerDeg', 'arcsecPerPx', 'containsPole']
    monkeypatch.undo()
    assert list(inspect.signature(R.resample_frame_mesh).parameters) == [
        'fd', 'altitude', 'boundingBox', 'pxPerDeg', 'containsDiscontinuity', 'containsPole', 'min_elevation', 'keep_on_device',
        'outline']
    from auromat_amd import _native
    assert 'amt_mesh_frame' in _native.exported_symbols()
    header = open(os.path.join(ROOT, 'include', 'auromat_hip.h')).read()
    assert len(_native._SIGNATURES['amt_mesh_frame'][0]) - 1 == header[header.index('int amt_mesh_frame('):].split(';')[0].count(',')
