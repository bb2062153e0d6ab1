"""
Without a GPU: the cases of tests/_interp_cases.py hold the patterns that tests/test_gpu_interp_cells.py relies on (row
lengths, degrees, run lengths, dyadic grids, ties on the ring boundary, the separation of the stopping sweep), and the plain
references of tests/_interp_oracle.py are right: the float64 relaxation against oracle.ref_numpy and against scipy's
CloughTocher2DInterpolator, the rational element against oracle.ref_numpy.clough_tocher_value, the integer brute force against
scipy's cKDTree.
"""
import os
import re

import numpy as np
import pytest

import _interp_cases as K
import _interp_oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'auromat_amd', 'csrc')
SOURCE = os.path.join(CSRC, 'amt_nearest.hip')


def test_constants_are_the_sources():
    text = open(SOURCE).read()
    common, scan = open(os.path.join(CSRC, 'amt_common.h')).read(), open(os.path.join(CSRC, 'amt_cell_scan.h')).read()
    for name, value, where in (('kGsPre', K.K_GS_PRE, text), ('kGsChan', K.K_GS_CHAN, text), ('kBlock', K.K_BLOCK, common),
                               ('kScanItems', K.K_SCAN_TILE // K.K_BLOCK, scan)):
        m = re.search(r'constexpr int %s = (\d+);' % name, where)
        assert m and int(m.group(1)) == value, name
    # the scan of the cell counts: the shared one, over tiles of kBlock * kScanItems cells
    assert 'constexpr int kScanTile = kBlock * kScanItems;' in scan and 'cell_scan(ctx, count, cells, bsum, offset);' in text
    assert 'k += 64' in text and 'nchan <= 63' in text


# ---- 1. graphs, partitions, layouts ------------------------------------------------------------------------------------------
def test_graphs_hold_their_patterns():
    lat, cre = K.graph('lattice'), K.graph('crescent')
    assert lat.n == 12 * 14 and list(np.diff(lat.rows)) == [14] * 12
    lengths = np.diff(cre.rows)
    assert set(range(6)) <= set(lengths) and {int(l) % 3 for l in lengths if l > 5} == {0, 1, 2}
    assert cre.degree.max() >= 9 and cre.degree.max() > 2 * K.K_GS_PRE // 2 and cre.n <= 450
    # the slow path inside a lattice-like graph: more neighbours than the record holds
    assert (cre.degree > K.K_GS_PRE).any() and (lat.degree > K.K_GS_PRE).any()
    for order in K.WHEEL_ORDERS:
        g = K.graph('wheels-' + order)
        assert sorted(g.degree[list(g.hubs)]) == [8, 9, 16, 17, 41] and g.n == sum(K.WHEEL_SIZES) + 5
        for h in g.hubs:
            nb = g.indices[g.indptr[h]:g.indptr[h + 1]]
            assert {'first': (nb > h).all(), 'last': (nb < h).all(), 'middle': (nb < h).any() and (nb > h).any()}[order]
    a, b = K.graph('wheels-first'), K.graph('wheels-last')
    assert np.array_equal(np.sort(a.xy, axis=0), np.sort(b.xy, axis=0))              # the same geometry
    iso = K.graph('isolated')
    assert iso.degree[0] == 0 and iso.degree[-1] == 0 and np.array_equal(iso.xy[1:-1], lat.xy)
    assert np.array_equal(iso.indices, lat.indices + 1) and np.array_equal(iso.base[1:-1], lat.base)
    for name in K.GRAPHS:
        g = K.graph(name)
        assert g.n <= 450 and (g.base[:, 3] == g.base[0, 3]).all()
        assert np.allclose(g.base[:, 0], 3 + 2 * g.xy[:, 0] - 0.5 * g.xy[:, 1])


def test_partitions_hold_their_patterns():
    for name in K.GRAPHS:
        g, parts = K.graph(name), K.partitions(name)
        assert {'natural', 'one-row', 'point-rows', 'cyclic'} <= set(parts)
        for rows in parts.values():
            assert rows[0] == 0 and rows[-1] == g.n and (np.diff(rows) >= 0).all()
        assert len(parts['one-row']) == 2 and (np.diff(parts['point-rows']) == 1).all()
        lengths = list(np.diff(parts['cyclic']))
        assert lengths[0] == 0 and lengths[-1] == 0 and 0 in lengths[2:-2]
        body = [l for l in lengths if l][:-1]                                      # (the last row is cut at n)
        assert body == [K.CYCLE[k % 8] for k in range(len(body))]
        if g.hubs:
            alone, after = parts['hub-alone'], parts['hub-after-two']
            for h in g.hubs:
                assert h in alone and h + 1 in alone
                k = np.searchsorted(after, h, side='right') - 1
                assert after[k] == max(h - 2, 0) and after[k + 1] == h + 1
        else:
            assert set(parts) == {'natural', 'one-row', 'point-rows', 'cyclic'}
    # hub last, a row of the two rim points before it and the hub: v - 1 and v - 2 from registers within the slow path (list
    # positions >= kGsPre), v - 3 a hand-over within the slow path
    g = K.graph('wheels-last')
    for h, k in zip(g.hubs, K.WHEEL_SIZES):
        nb = list(g.indices[g.indptr[h]:g.indptr[h + 1]])
        if k >= K.K_GS_PRE + 3:
            assert min(nb.index(h - 1), nb.index(h - 2), nb.index(h - 3)) >= K.K_GS_PRE


def test_layouts():
    for name in ('lattice', 'wheels-middle'):
        g = K.graph(name)
        for nchan in K.LAYOUTS:
            v = K.layout(name, nchan)
            assert v.shape == (g.n, nchan) and all(np.array_equal(v[:, c], g.base[:, c % 4]) for c in range(nchan))
        v = K.layout(name, 9, nan=True)
        assert np.isnan(v).sum() == 1 and np.isnan(v[g.n // 2, 8]) and 0 < g.n // 2 < g.n - 1
    assert K.LAYOUTS == (1, 8, 9, 19, 63)


# ---- the relaxation reference ------------------------------------------------------------------------------------------------
def test_relax_float64_equals_the_oracle_module():
    """The float64 run against oracle.ref_numpy.clough_tocher_gradients (np.hypot(..) ** 3 there, sqrt and two multiplications
    here: a few ulps of the terms), with the same stopping sweep."""
    from oracle import ref_numpy as R
    for name in ('lattice', 'crescent', 'wheels-middle'):
        g = K.graph(name)
        for b in range(3):
            want, sweeps = R.clough_tocher_gradients(g.xy, g.indptr, g.indices, g.base[:, b])
            got, err = O.relax(g.xy, g.indptr, g.indices, g.base[:, b], sweeps, np.float64)
            assert O.stopping_sweep(err, 1e-6) == sweeps, (name, b)
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (name, b)
    const, sweeps = R.clough_tocher_gradients(g.xy, g.indptr, g.indices, g.base[:, 3])
    assert sweeps == 1 and (const == 0).all()
    got, err = O.relax(g.xy, g.indptr, g.indices, g.base[:, 3], 1)
    assert (got == 0).all() and err == [0.0]


def test_relax_equals_scipy_on_the_lattice():
    """scipy.interpolate.CloughTocher2DInterpolator(tri, values).grad runs the same relaxation with its neighbours in another
    order: equal to summation order, within 8 * max(E_ref, eps * scale) with E_ref taken between scipy and the longdouble run."""
    import scipy.interpolate
    g, tri = K.graph('lattice'), K.lattice_triangulation()
    assert np.array_equal(tri.points, g.xy)
    for b in range(3):
        ip = scipy.interpolate.CloughTocher2DInterpolator(tri, g.base[:, b], tol=1e-6, maxiter=400)
        scipys = np.asarray(ip.grad).reshape(g.n, 2)
        _, err = K.reference('lattice', b, 30, True)
        sweeps = O.stopping_sweep(err, 1e-6)
        long, _ = K.reference('lattice', b, sweeps, True)
        ours, _ = K.reference('lattice', b, sweeps, False)
        e_ref = float(np.max(np.abs(scipys - long)))
        scale = float(np.max(np.abs(long)))
        bound = 8 * max(e_ref, K.EPS * scale)
        dist = float(np.max(np.abs(ours - long)))
        print(K.BASE[b], 'sweeps', sweeps, 'scipy-long %.3e ours-long %.3e scale %.3e' % (e_ref, dist, scale))
        assert dist <= bound and e_ref <= 1e-12 * scale, (b, dist, bound, e_ref)


def test_relax_longdouble_is_more_precise_and_counts_no_nan():
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps / 1000
    for name in K.GRAPHS:
        for b in range(3):
            bound, e_ref, scale = K.gradient_bound(name, b, K.FIXED_SWEEPS)
            assert 0 < e_ref < 1e-12 * scale and bound >= 8 * K.EPS * scale, (name, b, e_ref, scale)
    # isolated points: NaN gradients, errors as without them
    y, err = K.reference('isolated', 2, K.FIXED_SWEEPS, True)
    y0, err0 = K.reference('lattice', 2, K.FIXED_SWEEPS, True)
    assert np.isnan(y[0]).all() and np.isnan(y[-1]).all() and np.array_equal(y[1:-1], y0) and err == err0
    # NaN data: spreads, is not counted, leaves finite entries to compare
    for name in K.GRAPHS:
        y, err = K.reference(name, 0, K.FIXED_SWEEPS, True, True)
        yd, _ = K.reference(name, 0, K.FIXED_SWEEPS, False, True)
        assert np.isnan(y).any() and np.array_equal(np.isnan(y), np.isnan(yd)) and all(e == e for e in err), name
        # (connected graphs of a dozen rows are all NaN after 5 sweeps: a sweep carries it to every later point and one ring
        # back; the wheels the NaN is not in stay finite)
        if name.startswith('wheels'):
            assert (~np.isnan(y)).sum() >= 100, (name, int((~np.isnan(y)).sum()))


def test_stopping_sweep_is_separated_from_rounding():
    """For every non-constant base channel of the two graphs of the stopping test the reference's error at the stopping sweep is
    below 0.75 tol and the error of the sweep before above 1.5 tol; the channels do not all stop at the same sweep."""
    for name in ('lattice', 'crescent'):
        stops = []
        for b in range(3):
            _, err = K.reference(name, b, 30, True)
            k = O.stopping_sweep(err, K.STOP_TOLERANCE)
            assert k is not None and k >= 3
            assert err[k - 1] < 0.75 * K.STOP_TOLERANCE and err[k - 2] > 1.5 * K.STOP_TOLERANCE, (name, b, k, err[k - 2], err[k - 1])
            _, err64 = K.reference(name, b, k, False)
            assert O.stopping_sweep(err64, K.STOP_TOLERANCE) == k
            stops.append(k)
        assert len(set(stops)) > 1, stops
        _, err = K.reference(name, 3, 1, True)
        assert err == [0]


# ---- 2. the element ----------------------------------------------------------------------------------------------------------
_cases = {}


def element(nchan=3, kind='data', flags='real'):
    key = (nchan, kind, flags)
    if key not in _cases:
        case = K.element_case(nchan, kind, flags)
        _cases[key] = (case, K.element_exact(case), K.element_float(case))
    return _cases[key]


def test_element_cases_hold_their_patterns():
    for nchan in (3, 5):
        case = K.element_case(nchan)
        inside = case.vertices[:, 0] >= 0
        hull = case.has_nb[inside] == 0
        assert set(hull.sum(axis=1)) == {0, 1, 2} and hull.any(axis=0).all()
        assert case.m % 256 != 0 and case.m > 256 and 3 <= (~inside).sum()
        assert {'vertex', 'edge', 'inside', 'centroid', 'outside'} == set(case.kind)
        for a in (case.xy, case.values, case.gradients, case.targets[case.kind != 'centroid']):
            assert np.array_equal(a * 64, np.rint(a * 64))
        assert (case.values != 0).all() and len(case.pairs) > 20
        # the centroids are those of the triangles across the edges
        xy, simplices, neighbours = K.element_mesh()
        for r in np.flatnonzero(inside)[::7]:
            t = case.tri_id[r]
            assert set(case.vertices[r]) == set(simplices[t])
            for k in range(3):
                other = [q for q in range(len(simplices)) if q != t and len(set(simplices[q]) & set(np.delete(case.vertices[r], k))) == 2]
                assert bool(case.has_nb[r, k]) == (len(other) == 1)
                if other:
                    assert np.allclose(case.centroids[r, k], xy[simplices[other[0]]].mean(axis=0), rtol=0, atol=1e-14)
    none = K.element_case(3, 'quadratic', 'none')
    assert (none.has_nb == 0).all()


def test_exact_element_agrees_with_the_float64_element():
    case, exact, flt = element()
    bound, e_ref, scale = K.element_bound(case, exact, flt)
    print('E_ref', e_ref, 'scale', scale)
    assert (e_ref <= 1e-13 * scale).all() and (e_ref > 0).all()
    inside = case.kind != 'outside'
    assert np.isnan(flt[~inside]).all() and all(v is None for v in exact[~inside].ravel())
    # at the vertices the exact element is the vertex value
    for r in np.flatnonzero(case.kind == 'vertex'):
        want = case.values[case.vertices[r, case.vertex_k[r]]]
        assert [float(v) for v in exact[r]] == list(want)
    # C0 across an edge, exactly
    for a, b in case.pairs:
        assert list(exact[a]) == list(exact[b]), (a, b)


def test_exact_element_reproduces_quadratics():
    for flags in ('none', 'real'):
        case, exact, flt = element(3, 'quadratic', flags)
        want = K.quadratic_exact(case)
        inside = case.kind != 'outside'
        assert all(a == b for a, b in zip(exact[inside].ravel(), want[inside].ravel())), flags


# ---- 3. nearest ---------------------------------------------------------------------------------------------------------------
def test_grids_are_dyadic():
    for args in (K.box((8, 8), 20, 24), K.box((4, 16), 14, 16), K.box((16, 8), 14, 16), K.box((8, 8), 40, 50),
                 ((8, 8), 60.0, 62.0, -3.0, 3.0)):
        g = K.grid_of(*args)                                                         # asserts exactness and the steps
        for a in (g.latCenters, g.lonCenters, g.xedges, g.yedges):
            assert np.array_equal(np.asarray(a) * 64, np.rint(np.asarray(a) * 64))
    with pytest.raises(AssertionError):
        O.to_units(np.array([0.1]))


def test_nearest_cases_hold_their_patterns():
    cases = {c.name: c for c in K.all_nearest_cases()}
    runs = cases['runs'].notes['runs']
    lengths = [l for _, l, c in runs if c >= 0]
    assert set(K.RUNS) <= set(lengths)
    assert any(s < 64 < s + l for s, l, c in runs if c >= 0) and any(s < 256 < s + l for s, l, c in runs if c >= 0)
    assert cases['runs'].lat.size % 64 != 0 and cases['runs-small'].lat.size < 64
    assert (~cases['runs'].valid).sum() >= 4 and np.isnan(cases['runs'].lat).any() and cases['runs'].center_mask.any()
    counts = np.bincount(cases['crowded'].flat_cells()[cases['crowded'].valid])
    assert sorted(counts[counts > 0]) == [65, 129, 200]
    for (iy, ix), w in cases['crowded'].notes['winners'].items():
        members = np.flatnonzero(cases['crowded'].flat_cells() == iy * cases['crowded'].grid.nx + ix)
        assert w == members.max()                                                     # the nearest is the last one stored
    n_ring = 0
    for c in cases.values():
        if c.name.startswith('ring-'):
            n_ring += 1
            far, near = c.notes['ring']
            assert far == near + 1 and c.notes['winner'] < c.notes['loser']
            y, x = O.source_units(c.lat, c.lon, 0)
            ty, tx = O.to_units(c.grid.latCenters)[c.notes['row']], O.to_units(c.grid.lonCenters)[c.notes['col']]
            d = (y - ty) ** 2 + (x - tx) ** 2
            step = min(64 // c.grid_args[0][0], 64 // c.grid_args[0][1])
            assert d[1] == d[2]
            if 'x' in c.name.split('-')[-1] or c.grid_args[0][0] >= c.grid_args[0][1]:
                # exactly on the termination rule's boundary: (r + 1/2) of the smaller step
                assert 4 * d[1] == ((2 * near + 1) * step) ** 2 or c.grid_args[0] == (16, 8)
    assert n_ring == 18
    assert cases['ties-diagonal'].notes['ring'] == [11, 9, 11, 9] and len(set(cases['ties-same-ring'].notes['ring'])) == 1
    assert (cases['far-corner'].grid.ny, cases['far-corner'].grid.nx) == (40, 50) and cases['far-corner'].valid.sum() == 1
    out = cases['outside']
    _, _, ey, ex = K.grid_units(out.grid)
    y, x = O.source_units(out.lat, out.lon, 0)
    assert (y < ey[0]).any() and (y > ey[-1]).any() and (x < ex[0]).any() and (x > ex[-1]).any()
    assert (x - ex[-1]).max() > 30 * 8 and (ey[0] - y).max() > 30 * 8
    assert not cases['no-valid-source'].valid.any()
    sizes = sorted(c.grid.nx * c.grid.ny for c in cases.values() if c.name.startswith('scan-'))
    assert sizes[0] < 64 and sizes[1] == 1024 and sizes[2] == 1025 and sizes[6] > 3000 and sizes[6] % 1024 != 0
    # the boundaries of the scan's tile: a tile less two cells, exactly one tile, a tile and a cell; and more than two tiles
    assert sizes[3:6] == [K.K_SCAN_TILE - 2, K.K_SCAN_TILE, K.K_SCAN_TILE + 1] and sizes[6] > 2 * K.K_SCAN_TILE and len(sizes) == 7
    for ny, nx in K.SCAN_TILE_GRIDS:
        c = cases['scan-%dx%d' % (ny, nx)]
        assert K.scan_chunk(ny, nx) == K.K_SCAN_TILE and (c.height, c.width) == (10, 13)
        assert (c.expected() >= 0).all()                                             # every grid centre gets a nearest source
    assert all(K.scan_chunk(*s) == 1024 for s in K.SCAN_GRIDS)
    wrap = cases['lon-wrap']
    assert wrap.lon_wrap == 1 and (wrap.lon == 180).any() and (wrap.lon == -180).any()
    assert cases['minus-inf'].min_elevation == -np.inf and cases['minus-inf'].elev is not None


def test_brute_force_agrees_with_a_kd_tree_where_the_nearest_is_unique():
    import scipy.spatial
    checked = 0
    for case in K.all_nearest_cases():
        if not case.valid.any():
            continue
        y, x = O.source_units(case.lat, case.lon, case.lon_wrap)
        src = np.flatnonzero(case.valid)
        pts = np.column_stack((y[src], x[src])).astype(np.float64)
        g = case.grid
        ty, tx = O.to_units(g.latCenters), O.to_units(g.lonCenters)
        targets = np.column_stack((np.repeat(ty, g.nx), np.tile(tx, g.ny))).astype(np.float64)
        k = min(2, len(src))
        dist, idx = scipy.spatial.cKDTree(pts).query(targets, k=k)
        dist, idx = dist.reshape(len(targets), k), idx.reshape(len(targets), k)
        unique = np.ones(len(targets), bool) if k == 1 else dist[:, 0] < dist[:, 1]
        want = case.expected().ravel()
        if case.target_mask is not None:
            unique &= case.target_mask.ravel() == 0
            assert (want[case.target_mask.ravel() != 0] == -1).all()
        assert np.array_equal(want[unique], src[idx[:, 0]][unique]), case.name
        checked += int(unique.sum())
    assert checked > 10000


def test_gather_reference():
    index, img, elev = K.gather_case(np.uint16, 3)
    mean, out_img, mask = O.gather(index, img, elev)
    assert (index == -1).sum() > 50 and mean.shape == (len(index), 4)
    for t in (0, 5, len(index) - 1):
        if index[t] < 0:
            assert np.isnan(mean[t]).all() and (out_img[t] == 0).all() and mask[t] == 1
        else:
            assert list(mean[t]) == list(img[index[t]]) + [elev[index[t]]] and mask[t] == 0
    assert np.isnan(O.gather(index, img, None)[0][:, 3]).all()
    assert O.gather(index, K.gather_case(np.uint8, 0)[1], elev)[0].shape == (len(index), 1)


# ---- 4. polygons --------------------------------------------------------------------------------------------------------------
def test_polygons_hold_their_patterns():
    import matplotlib.path
    assert [m % K.K_BLOCK for m in K.POLYGON_SIZES] == [0, 1, 1] and K.POLYGON_SIZES[2] == 2 * K.K_BLOCK + 1
    for m in K.POLYGON_SIZES:
        poly = K.polygon(m)
        assert len(poly) == m and np.array_equal(poly, np.rint(poly))
        pts = K.polygon_points(poly)
        assert (pts[:K.K_BLOCK, 1] == pts[0, 1]).all() and pts[0, 1] in poly[:, 1]   # a block with one y, a vertex's
        assert np.isnan(pts).any() and len(pts) % K.K_BLOCK != 0
        on_vertex = (pts[:, None, :] == poly[None, :8, :]).all(axis=2).any(axis=0)
        assert on_vertex.all()
        finite = np.isfinite(pts).all(axis=1)
        assert not matplotlib.path.Path(poly).contains_points(pts[~finite]).any() and (~finite).sum() >= 10
        inside = matplotlib.path.Path(poly).contains_points(pts[finite])
        assert 100 < inside.sum() < finite.sum() - 100
        # simple: no two non-adjacent edges cross (integer arithmetic)
        a, b = poly.astype(np.int64), np.roll(poly, -1, axis=0).astype(np.int64)

        def orient(p, q, r):
            return np.sign((q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0]))
        i, j = np.triu_indices(m, 2)
        keep = ~((i == 0) & (j == m - 1))
        i, j = i[keep], j[keep]
        cross = (orient(a[i], b[i], a[j]) * orient(a[i], b[i], b[j]) < 0) & (orient(a[j], b[j], a[i]) * orient(a[j], b[j], b[i]) < 0)
        assert not cross.any(), m
