"""
The interpolating kernels of auromat_amd/csrc/amt_nearest.hip on constructed point sets: the cases of tests/_interp_cases.py
go to ``amt_cubic_gradients_csr``, ``amt_cubic_eval``, ``amt_nearest_frame``, ``amt_nearest_gather`` and
``amt_points_in_polygon`` as plain device arrays, outputs pre-filled with a poison byte, and every element of every output is
compared with the plain references of tests/_interp_oracle.py.  tests/test_interp_cases_cpu.py checks without a GPU that the
cases hold the patterns they claim and that the references are right.

What the cases aim at.  Relaxation (k_cubic_gs): graphs that are no lattices (degrees up to 41: the record path full, one, two,
three and six chunks of the slow path), every partition of one point order into rows (natural, one row, one point per row,
cyclic lengths with empty rows, a hub alone, a hub after two of its rim points), 1 to 63 channels (eight channel groups, partly
filled groups, channels that stop in different groups), points without neighbours, a constant channel, NaN data; compared with
a sequential Gauss-Seidel in np.longdouble after a FIXED number of sweeps (mid-relaxation), and bit for bit between all
partitions and channel layouts: the result does not depend on the schedule.  Element (k_cubic_eval): dyadic data against
rational arithmetic.  Nearest (k_nn_*): dyadic coordinates, so that squared distances are exact and ties are real, against a
brute force on integers.

Tolerances: 8 * max(E_ref, eps * scale), E_ref the distance between the float64 and the exact (longdouble / rational) run of
the REFERENCE, scale the largest exact magnitude; printed per case.  Largest values measured on the MI355X:
  relaxation, 5 sweeps (graph, channel: kernel distance / E_ref / scale = part of the bound; the largest over all partitions and
  layouts):  wheels-last plane 2.5e-15 / 1.9e-15 / 2.0 = 0.17;  lattice plane 9.5e-16 / 9.5e-16 / 2.0 = 0.13;  wheels-first smooth
  5.6e-14 / 5.5e-14 / 117 = 0.13;  crescent noise 2.3e-13 / 2.4e-13 / 661 = 0.12;  lattice noise 1.7e-13 / 1.8e-13 / 658 = 0.12;
  wheels-middle noise 2.8e-13 / 3.0e-13 / 453 = 0.12;  crescent smooth 5.6e-14 / 6.3e-14 / 93 = 0.11;  constant channel 0 / 0 / 0
  element (per call: the largest over the channels):  3 channels 2.2e-14 / 1.8e-14 / 60 = 0.16;  5 channels 1.9e-14 / 1.3e-14 / 55 =
  0.18;  quadratics, flags 0 and real alike, 4.6e-14 / 4.6e-14 / 242 = 0.11 and 1.4e-14 / 1.4e-14 / 66 = 0.12
  stopping sweeps at tolerance 1e-6, lattice and crescent alike: plane 12, smooth 12, noise 14, constant 1
"""
import ctypes as C

import numpy as np
import pytest

import _interp_cases as K
import _interp_oracle as O

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_I32 = np.frombuffer(bytes([POISON] * 4), dtype=np.int32)[0]
TINY = 1e-300


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


def poisoned(shape, dtype=None):
    import torch
    t = _ctx().empty(shape, dtype)
    t.view(torch.uint8).fill_(POISON)
    return t


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Identical bits, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ============================================================================================================================
# 1. amt_cubic_gradients_csr
# ============================================================================================================================
_device_graphs = {}
_gradient_runs = {}


def device_graph(name):
    if name not in _device_graphs:
        ctx, g = _ctx(), K.graph(name)
        _device_graphs[name] = (ctx.to_device(g.xy), ctx.to_device(g.indptr, np.int64),
                                ctx.to_device(g.indices, np.int32))
    return _device_graphs[name]


def call_gradients(name, rows, values, tolerance, max_iterations):
    """One call on poisoned outputs: (status, gradients (n, nchan, 2), iterations (nchan,))."""
    import torch
    from auromat_amd._native import ptr
    ctx, g = _ctx(), K.graph(name)
    xy, indptr, indices = device_graph(name)
    nchan = values.shape[1]
    d_rows, d_values = ctx.to_device(rows, np.int64), ctx.to_device(values)
    grad = poisoned((g.n, nchan, 2))
    sweeps = (C.c_int32 * nchan)(*([int(POISON_I32)] * nchan))
    rc = ctx._lib.amt_cubic_gradients_csr(ctx.handle, ptr(xy), g.n, ptr(indptr), ptr(indices), ptr(d_rows), len(rows) - 1,
                                          ptr(d_values), nchan, float(tolerance), int(max_iterations), ptr(grad), sweeps)
    torch.cuda.synchronize()
    return rc, grad.cpu().numpy(), np.array(list(sweeps), dtype=np.int64)


def gradients(name, part, layout, tolerance=TINY, max_iterations=K.FIXED_SWEEPS):
    """Cached run.  layout: ('single', base column) | (nchan, nan)."""
    key = (name, part, layout, tolerance, max_iterations)
    if key not in _gradient_runs:
        g = K.graph(name)
        values = np.ascontiguousarray(g.base[:, layout[1]:layout[1] + 1]) if layout[0] == 'single' else K.layout(name, *layout)
        rc, grad, sweeps = call_gradients(name, K.partitions(name)[part], values, tolerance, max_iterations)
        assert rc == 0, (key, rc)
        assert not (bits(grad) == bits(np.frombuffer(bytes([POISON] * 8), dtype=np.float64))[0]).any(), key
        _gradient_runs[key] = (grad, sweeps)
    return _gradient_runs[key]


def check_against_reference(name, grad, column, base, sweeps, what, nan=False):
    """Column `column` of a run against the longdouble reference of base column `base` after `sweeps` sweeps."""
    want, _ = K.reference(name, base, sweeps, True, nan)
    bound, e_ref, scale = K.gradient_bound(name, base, sweeps, nan)
    got = grad[:, column, :]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    ok = ~np.isnan(want)
    dist = float(np.max(np.abs(got.astype(np.longdouble) - want)[ok], initial=0.0))
    print('%s: E_ref %.3e scale %.3e bound %.3e kernel %.3e (%.2f of the bound)' % (what, e_ref, scale, bound, dist,
                                                                                    dist / bound if bound else 0.0))
    assert dist <= bound, (what, dist, bound)
    return dist / bound if bound else 0.0


@pytest.mark.parametrize('name', K.GRAPHS)
def test_gradients_after_a_fixed_number_of_sweeps(name):
    """tolerance 1e-300, max_iterations 5: every non-constant channel has run 5 sweeps, the constant one 1; the gradients are
    the longdouble reference's after 5 sweeps, for every partition, with 1 and with 19 channels."""
    const = K.BASE.index('const')
    for part in K.partitions(name):
        for b in range(4):
            grad, sweeps = gradients(name, part, ('single', b))
            assert list(sweeps) == [1 if b == const else K.FIXED_SWEEPS], (name, part, b, sweeps)
            check_against_reference(name, grad, 0, b, K.FIXED_SWEEPS, '%s %s %s' % (name, part, K.BASE[b]))
        grad, sweeps = gradients(name, part, (19, False))
        assert list(sweeps) == [1 if c % 4 == const else K.FIXED_SWEEPS for c in range(19)], (name, part, sweeps)
        for c in range(19):
            check_against_reference(name, grad, c, c % 4, K.FIXED_SWEEPS, '%s %s 19 channels, column %d' % (name, part, c))


ALL_LAYOUTS = [(n, False) for n in K.LAYOUTS if n > 1] + [(9, True)]


@pytest.mark.parametrize('name', K.GRAPHS)
def test_gradients_do_not_depend_on_the_schedule(name):
    """Bit for bit: every partition of the rows gives the same gradients, and column c of every channel layout is the
    one-channel run of its base column — also beside a channel that carries a NaN."""
    parts = list(K.partitions(name))
    single = [gradients(name, parts[0], ('single', b))[0][:, 0, :] for b in range(4)]
    for part in parts:
        for b in range(4):
            assert same_bits(gradients(name, part, ('single', b))[0][:, 0, :], single[b]), (name, part, K.BASE[b])
        for lay in ALL_LAYOUTS:
            grad, sweeps = gradients(name, part, lay)
            first = gradients(name, parts[0], lay)
            assert same_bits(grad, first[0]) and np.array_equal(sweeps, first[1]), (name, part, lay)
            for c in range(lay[0] - (1 if lay[1] else 0)):
                assert same_bits(grad[:, c, :], single[c % 4]), (name, part, lay, c)


@pytest.mark.parametrize('name', ['lattice', 'crescent'])
def test_gradients_stop_at_the_references_sweep(name):
    """tolerance 1e-6, at most 400 sweeps, 19 channels: every channel stops at the sweep the longdouble reference stops at (the
    CPU test asserts that the decision is not within rounding), the constant one after 1; the gradients are those of the run
    with exactly that many sweeps, bit for bit — a channel that stopped is carried over while its neighbours in the wave and
    in the other groups go on."""
    const = K.BASE.index('const')
    stop = []
    for b in range(4):
        _, err = K.reference(name, b, 30 if b != const else 1, True)
        stop.append(1 if b == const else O.stopping_sweep(err, K.STOP_TOLERANCE))
    assert None not in stop and len(set(stop[:3])) > 1, stop
    for part in ('natural', 'cyclic'):
        grad, sweeps = gradients(name, part, (19, False), K.STOP_TOLERANCE, 400)
        print(name, part, 'stopping sweeps', list(sweeps[:4]), 'reference', stop)
        assert list(sweeps) == [stop[c % 4] for c in range(19)], (name, part, sweeps, stop)
        for k in sorted(set(stop)):
            fixed, fixed_sweeps = gradients(name, part, (19, False), TINY, k)
            for c in range(19):
                if stop[c % 4] == k:
                    assert fixed_sweeps[c] == k
                    assert same_bits(grad[:, c, :], fixed[:, c, :]), (name, part, c, k)


def test_points_without_neighbours():
    """`isolated` is `lattice` with one more point in front and one behind, both with empty lists (as duplicates have): their
    gradients are NaN, every other point has the lattice's bits, the sweep counts are unchanged (a NaN change does not count)."""
    for lay in [('single', b) for b in range(4)] + [(19, False)]:
        for tol, maxit in ((TINY, K.FIXED_SWEEPS), (K.STOP_TOLERANCE, 400)):
            iso, iso_sweeps = gradients('isolated', 'natural', lay, tol, maxit)
            lat, lat_sweeps = gradients('lattice', 'natural', lay, tol, maxit)
            assert np.isnan(iso[0]).all() and np.isnan(iso[-1]).all(), lay
            assert not np.isnan(iso[1:-1]).any() and same_bits(iso[1:-1], lat), lay
            assert np.array_equal(iso_sweeps, lat_sweeps), (lay, iso_sweeps, lat_sweeps)


@pytest.mark.parametrize('name', K.GRAPHS)
def test_gradients_with_nan_data(name):
    """One NaN value in column 8, the lone channel of the second group: the call succeeds (no stall), the NaN set of the column
    after 5 sweeps is the reference's, the finite entries are within the tolerance."""
    want, err = K.reference(name, 0, K.FIXED_SWEEPS, True, True)
    assert np.isnan(want).any()
    # a NaN change does not count: once every gradient of a connected graph is NaN the sweep's error is 0 and the channel stops,
    # here as in the reference
    stop = O.stopping_sweep(err, TINY) or K.FIXED_SWEEPS
    assert stop == K.FIXED_SWEEPS or np.isnan(want).all()
    for part in K.partitions(name):
        grad, sweeps = gradients(name, part, (9, True))               # asserts the status
        assert sweeps[8] == stop, (name, part, sweeps, stop)
        assert np.array_equal(np.isnan(grad[:, 8, :]), np.isnan(want)), (name, part)
        check_against_reference(name, grad, 8, 0, stop, '%s %s NaN column' % (name, part), nan=True)


def test_gradients_argument_errors():
    """Rejected with a negative status and no launch (the outputs keep their poison); the context works afterwards."""
    from auromat_amd._native import ptr
    ctx, g = _ctx(), K.graph('lattice')
    rows = K.partitions('lattice')['natural']
    values = K.layout('lattice', 3)
    for what, nchan, tol, maxit in (('nchan 0', 0, 1e-6, 5), ('nchan 64', 64, 1e-6, 5), ('tolerance 0', 3, 0.0, 5),
                                    ('max_iterations 0', 3, 1e-6, 0)):
        v = np.ascontiguousarray(g.base[:, np.arange(max(nchan, 1)) % 4])
        xy, indptr, indices = device_graph('lattice')
        grad = poisoned((g.n, max(nchan, 1), 2))
        sweeps = (C.c_int32 * 64)(*([int(POISON_I32)] * 64))
        d_rows, d_v = ctx.to_device(rows, np.int64), ctx.to_device(v)
        rc = ctx._lib.amt_cubic_gradients_csr(ctx.handle, ptr(xy), g.n, ptr(indptr), ptr(indices), ptr(d_rows), len(rows) - 1, ptr(d_v),
                                              nchan, tol, maxit, ptr(grad), sweeps)
        assert rc < 0, (what, rc)
        assert (grad.cpu().numpy().view(np.uint8) == POISON).all() and all(s == POISON_I32 for s in sweeps), what
    xy, indptr, indices = device_graph('lattice')
    d_rows, d_values = ctx.to_device(rows, np.int64), ctx.to_device(values)
    grad = poisoned((g.n, 3, 2))
    sweeps = (C.c_int32 * 3)(*([int(POISON_I32)] * 3))
    good = [ptr(xy), g.n, ptr(indptr), ptr(indices), ptr(d_rows), len(rows) - 1, ptr(d_values), 3, 1e-6, 5, ptr(grad), sweeps]
    bad = list(good)
    bad[1] = 2                                                         # n = 2
    assert ctx._lib.amt_cubic_gradients_csr(ctx.handle, *bad) < 0
    for k in (0, 2, 3, 4, 6, 10, 11):                                  # a NULL array
        bad = list(good)
        bad[k] = None
        assert ctx._lib.amt_cubic_gradients_csr(ctx.handle, *bad) < 0, k
    assert (grad.cpu().numpy().view(np.uint8) == POISON).all() and all(s == POISON_I32 for s in sweeps)
    with pytest.raises(Exception):
        ctx.call('amt_cubic_gradients_csr', *bad)
    rc, after, n_sweeps = call_gradients('lattice', rows, values, TINY, K.FIXED_SWEEPS)
    assert rc == 0 and same_bits(after, gradients('lattice', 'natural', (19, False))[0][:, :3, :])


# ============================================================================================================================
# 2. amt_cubic_eval
# ============================================================================================================================
TAIL = 64
_element = {}


def run_element(case):
    """(m, nchan) values; asserts that the poison behind the buffer's used part is untouched."""
    import torch
    from auromat_amd._native import ptr
    ctx = _ctx()
    out = poisoned((case.m * case.nchan + TAIL,))
    # (the device arrays are held in names until the kernel has run: a temporary's memory is handed to the next upload)
    held = [ctx.to_device(case.targets), ctx.to_device(case.vertices, np.int32), ctx.to_device(case.centroids),
            ctx.to_device(case.has_nb, np.uint8), ctx.to_device(case.xy), ctx.to_device(case.values), ctx.to_device(case.gradients)]
    assert held[1].shape == (case.m, 3) and int(held[1].max()) < len(case.xy) and held[6].shape == (len(case.xy), case.nchan, 2)
    ctx.call('amt_cubic_eval', case.m, *([ptr(t) for t in held] + [case.nchan, ptr(out)]))
    torch.cuda.synchronize()
    del held
    host = out.cpu().numpy()
    assert (host[case.m * case.nchan:].view(np.uint8) == POISON).all(), 'written past m * nchan'
    return host[:case.m * case.nchan].reshape(case.m, case.nchan)


def element(nchan, kind='data', flags='real'):
    key = (nchan, kind, flags)
    if key not in _element:
        case = K.element_case(nchan, kind, flags)
        exact = K.element_exact(case)
        bound = K.element_bound(case, exact, K.element_float(case))
        _element[key] = (case, exact, bound, run_element(case))
    return _element[key]


def check_element(what, case, got, exact, bound):
    limit, e_ref, scale = bound
    dist = K.distance_to_exact(got, exact)
    inside = case.kind != 'outside'
    worst = np.max(dist[inside], axis=0)
    for c in range(case.nchan):
        print('%s channel %d: E_ref %.3e scale %.3e bound %.3e kernel %.3e (%.2f of the bound)' % (
            what, c, e_ref[c], scale[c], limit[c], worst[c], worst[c] / limit[c]))
    assert np.isnan(got[~inside]).all() and not np.isnan(got[inside]).any(), what
    assert (dist[inside] <= limit[None, :]).all(), (what, worst, limit)


@pytest.mark.parametrize('nchan', [3, 5])
def test_element_against_rational_arithmetic(nchan):
    """Every row and channel: vertex targets return the vertex value bit for bit, rows outside the hull are NaN, everything
    else (interior points, edge points, centroids; hull edges in every position) is the exact value within the bound."""
    case, exact, bound, got = element(nchan)
    assert case.m % 256 != 0
    for r in np.flatnonzero(case.kind == 'vertex'):
        want = case.values[case.vertices[r, case.vertex_k[r]]]
        assert bits(got[r]).tolist() == bits(want).tolist(), (r, got[r], want)
    assert np.isnan(got[case.kind == 'outside']).all() and (case.kind == 'outside').sum() >= 3
    check_element('element, %d channels' % nchan, case, got, exact, bound)


def test_element_is_continuous_across_an_edge():
    """The same target on the common edge of two triangles, evaluated from either side, within the bound of the element test."""
    case, exact, bound, got = element(3)
    for a, b in case.pairs:
        assert case.tri_id[a] != case.tri_id[b] and np.array_equal(case.targets[a], case.targets[b])
        assert (np.abs(got[a] - got[b]) <= bound[0]).all(), (a, b, got[a], got[b])


@pytest.mark.parametrize('flags', ['none', 'real'])
def test_element_reproduces_quadratics(flags):
    """Vertex values and exact gradients of quadratics with dyadic coefficients: every target returns the quadratic's value,
    with all has_neighbour flags 0 and with the real neighbours (any g reproduces quadratics)."""
    case, exact, bound, got = element(3, 'quadratic', flags)
    check_element('quadratic, flags %s' % flags, case, got, K.quadratic_exact(case), bound)


# ============================================================================================================================
# 3. amt_nearest_frame, amt_nearest_gather
# ============================================================================================================================
def run_nearest(case):
    import torch
    from auromat_amd._native import ptr
    ctx, g = _ctx(), case.grid
    xaxis, yaxis = g.axes(ctx)
    tlat, tlon = g.device_centers(ctx)
    dev = lambda a, t=np.float64: None if a is None else ctx.to_device(a, t)
    index = poisoned((g.ny, g.nx), torch.int64)
    thr = float('-inf') if case.min_elevation is None else float(case.min_elevation)
    lat, lon, elev = dev(case.lat), dev(case.lon), dev(case.elev)          # held in names until the kernels have run
    cmask, tmask = dev(case.center_mask, np.uint8), dev(case.target_mask, np.uint8)
    assert lat.numel() == lon.numel() == case.height * case.width and tlat.numel() == g.ny and tlon.numel() == g.nx
    ctx.call('amt_nearest_frame', ptr(lat), ptr(lon), ptr(elev), ptr(cmask), case.height, case.width, thr, C.byref(xaxis),
             C.byref(yaxis), case.lon_wrap, ptr(tlat), ptr(tlon), ptr(tmask), ptr(index))
    torch.cuda.synchronize()
    del lat, lon, elev, cmask, tmask
    return index.cpu().numpy()


NEAREST = K.all_nearest_cases()


@pytest.mark.parametrize('case', NEAREST, ids=[c.name for c in NEAREST])
def test_nearest_index_equals_the_exact_brute_force(case):
    """out_index of every grid centre against the brute force on integers, the lowest flat index on a tie."""
    got, want = run_nearest(case), case.expected()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (case.name, len(bad), [(tuple(b), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])
    if 'winner' in case.notes:
        assert got[case.notes['row'], case.notes['col']] == case.notes['winner']


def test_nearest_indices_wrapper_gives_the_same():
    from auromat_amd._native import to_host
    from auromat_amd.resample import nearest_indices
    ctx = _ctx()
    for case in NEAREST:
        if case.name in ('runs', 'threshold-and-masks', 'lon-wrap', 'minus-inf'):
            dev = lambda a, t=np.float64: None if a is None else ctx.to_device(a, t)
            held = [dev(case.lat), dev(case.lon), dev(case.elev), dev(case.center_mask, np.uint8), dev(case.target_mask, np.uint8)]
            idx = nearest_indices(ctx, held[0], held[1], held[2], held[3], case.height, case.width, case.min_elevation, case.grid,
                                  case.lon_wrap, held[4])
            assert np.array_equal(to_host(idx, dtype=np.int64), case.expected()), case.name


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('nchan', K.GATHER_CHANNELS)
def test_nearest_gather_equals_fancy_indexing(nchan, dtype):
    import torch
    from auromat_amd._native import ptr
    ctx = _ctx()
    index, img, elev = K.gather_case(dtype, nchan)
    t = len(index)
    code = 2 if dtype == np.uint16 else 1
    d_index, d_elev = ctx.to_device(index, np.int64), ctx.to_device(elev)
    d_img = ctx.to_device(img, dtype) if nchan else None
    for with_elev in (True, False):
        want_mean, want_img, want_mask = O.gather(index, img, elev if with_elev else None)
        for drop in (None, 'mean', 'img', 'mask'):
            mean = None if drop == 'mean' else poisoned((t, nchan + 1))
            out_img = None if (drop == 'img' or not nchan) else poisoned((t, nchan), torch.int16 if code == 2 else torch.uint8)
            out_mask = None if drop == 'mask' else poisoned((t,), torch.uint8)
            ctx.call('amt_nearest_gather', ptr(d_index), t, ptr(d_img), code if nchan else 0, nchan,
                     ptr(d_elev) if with_elev else None, ptr(mean), ptr(out_img), ptr(out_mask))
            torch.cuda.synchronize()
            what = (nchan, np.dtype(dtype).name, with_elev, drop)
            if mean is not None:
                assert np.array_equal(mean.cpu().numpy(), want_mean, equal_nan=True), what
            if out_img is not None:
                assert np.array_equal(out_img.cpu().numpy().view(dtype), want_img), what
            if out_mask is not None:
                assert np.array_equal(out_mask.cpu().numpy(), want_mask), what


# ============================================================================================================================
# 4. amt_points_in_polygon
# ============================================================================================================================
def run_polygon(points, poly, n_vertices=None):
    import torch
    from auromat_amd._native import ptr
    ctx = _ctx()
    px, py = ctx.to_device(np.ascontiguousarray(points[:, 0])), ctx.to_device(np.ascontiguousarray(points[:, 1]))
    out = poisoned((len(points),), torch.uint8)
    d_poly = ctx.to_device(poly)
    ctx.call('amt_points_in_polygon', ptr(px), ptr(py), len(points), ptr(d_poly), len(poly) if n_vertices is None else n_vertices,
             ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('m', K.POLYGON_SIZES)
def test_points_in_integer_polygons(m):
    """Polygons whose edges fill the staged chunk exactly, by one more, and twice by one more; points on vertices, on edges, on
    the horizontal through vertices, a block of points with one y, NaN points: matplotlib's contains_points."""
    import matplotlib.path
    for poly in (K.polygon(m), K.polygon(m)[::-1].copy()):
        pts = K.polygon_points(poly)
        want = matplotlib.path.Path(poly).contains_points(pts)
        assert not want[~np.isfinite(pts).all(axis=1)].any() and (~np.isfinite(pts).all(axis=1)).sum() >= 10
        got = run_polygon(pts, poly)
        assert set(np.unique(got)) <= {0, 1}
        bad = got.astype(bool) != want
        assert not bad.any(), (m, int(bad.sum()), pts[bad][:5])
        assert want.sum() > 100 and (~want).sum() > 100


def test_points_in_a_polygon_of_fewer_than_three_vertices():
    poly = K.polygon(256)
    pts = K.polygon_points(poly)
    for n_vertices in (0, 1, 2):
        assert (run_polygon(pts, poly, n_vertices) == 0).all(), n_vertices
