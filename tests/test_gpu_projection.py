"""
The projection kernels (k_project_forward, k_project_inverse of auromat_amd/csrc/amt_project.hip) on the constructed points of
tests/_projection_cases.py: ``amt_project_forward`` and ``amt_project_inverse``, both projections, every family.

Buffers: inputs and outputs lie 16 and 16 + 8 bytes into poisoned allocations with 64 doubles of padding on either side; no byte
outside [0, n) of an output changes, and the NaN pattern is that of the mpmath reference (the domain rule, the non-finite inputs).

Accuracy, per point and output:  |kernel - reference| <= 8 max(E_ref, eps scale)  — the form and the factor of
tests/test_gpu_coord_ops.py.  reference: mpmath at 50 digits on the float64 inputs; E_ref: the distance of the float64 NumPy
statement of tests/_projection_oracle.py (Snyder's text) from it at the same point; scale: max(|x|, |y|, a) forward, 90 degrees for
an inverse latitude, 180 / cos(lat) degrees for an inverse longitude (its condition number near the geographic poles); eps = 2^-52.
The bound is derived from the number format and the reference's own error and was fixed before the first run.

Largest |kernel - reference| / (eps scale) per family, as the run prints it (-s); the bound is 8 wherever E_ref is smaller:
    family     forward x    y      inverse lat  lon
    centre     0.00  0.45          0.72  0.12
    near       0.45  0.92          0.66  0.00
    limit_in   2.58  2.82          0.81  0.92
    limit_out  (NaN)               1.10  0.74
    poles      0.32  1.15          1.05  0.71
    dateline   1.99  1.75          1.11  0.39
    spread     3.38  2.23          1.13  0.68
    len_1..257 2.13  2.93          0.80  0.77
    worst overall: 3.38 (forward x, family 'spread')
"""
import ctypes as C

import numpy as np
import pytest

import _projection_cases as K
import _projection_oracle as O

pytestmark = pytest.mark.gpu

PAD = 64
POISON = 0xA5
CASES = K.cases()
F64 = O.Float64()


def _struct(P):
    from auromat_amd._native import Projection, lib
    p = Projection()
    if P['kind'] == 'paeqd':
        assert lib().amt_projection_polar_aeqd(1 if P['north'] else 0, P['lon0'], P['a'], C.byref(p)) == 0
    else:
        assert lib().amt_projection_stereographic(P['lat0'], P['lon0'], P['a'], P['b'], C.byref(p)) == 0
    return p


class Buffer(object):
    """n doubles `shift` doubles past a 16-byte boundary of a poisoned allocation, PAD doubles of padding on either side"""

    def __init__(self, n, shift, values=None):
        import torch
        from auromat_amd._native import Context
        self.n, self.first = n, PAD + 2 + shift
        self.whole = torch.empty(n + 2 * PAD + 4, dtype=torch.float64, device=Context.current().device)
        self.whole.view(torch.uint8).fill_(POISON)
        assert self.whole.data_ptr() % 16 == 0
        self.part = self.whole[self.first:self.first + n]
        if values is not None:
            self.part.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)))
        assert self.part.data_ptr() % 16 == 8 * (shift % 2)
        self.ptr = C.c_void_p(self.part.data_ptr())

    def host(self):
        """the n values; asserts that the padding is untouched"""
        raw = self.whole.cpu().numpy().view(np.uint8).reshape(-1, 8)
        outside = np.ones(len(raw), dtype=bool)
        outside[self.first:self.first + self.n] = False
        assert np.all(raw[outside] == POISON), 'bytes outside [0, n) were written'
        return raw[self.first:self.first + self.n].copy().view(np.float64).reshape(self.n)


def run(P, direction, u, v, shift):
    import torch
    from auromat_amd._native import Context
    ctx = Context.current()
    n = len(u)
    a, b = Buffer(n, shift, u), Buffer(n, shift + 1, v)
    o0, o1 = Buffer(n, shift + 1), Buffer(n, shift)
    p = _struct(P)
    ctx.call('amt_project_' + direction, C.byref(p), a.ptr, b.ptr, n, o0.ptr, o1.ptr)
    torch.cuda.synchronize()
    assert np.array_equal(a.host(), u, equal_nan=True) and np.array_equal(b.host(), v, equal_nan=True)     # inputs unchanged
    return o0.host(), o1.host()


def ratios(case, direction, got):
    """per output: |kernel - reference| / (eps scale), the bound / (eps scale) = 8 max(E_ref / (eps scale), 1), per point"""
    ref = K.reference(case, direction)
    inp = (case['lat'], case['lon']) if direction == 'forward' else K.inverse_inputs(case)
    f64 = O.points(F64, getattr(O, direction), case['projection'], *inp)
    out = []
    for g, r, (dist, eps_scale), (e_ref, _) in zip(got, ref, K.distances_and_scales(case, direction, got, ref),
                                                   K.distances_and_scales(case, direction, f64, ref)):
        assert np.array_equal(np.isnan(g), np.isnan(r)), '%s %s: NaN pattern differs at %s' % (
            case['name'], direction, np.nonzero(np.isnan(g) != np.isnan(r))[0][:6].tolist())
        ok = ~np.isnan(r)
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.where(ok, dist / eps_scale, 0.0).astype(np.float64)
            # (the float64 statement's NaN pattern is checked in tests/test_projection_cpu.py; a NaN there adds nothing here)
            lim = K.FACTOR * np.maximum(np.where(ok & ~np.isnan(e_ref), e_ref / eps_scale, 0.0).astype(np.float64), 1.0)
        rel = np.where(np.isnan(rel), 0.0, rel)         # (0 / inf at a pole itself: any longitude is right)
        out.append((rel, lim))
    return out


_MEASURED = {}


def measure(case, direction):
    """Runs a case once (both alignments) -> (inputs, outputs, [(ratio, bound) per output])"""
    key = (case['name'], direction)
    if key not in _MEASURED:
        u, v = (case['lat'], case['lon']) if direction == 'forward' else K.inverse_inputs(case)
        # the inputs 16 and 16 + 8 bytes past a 16-byte boundary, the outputs the other way round
        first, second = run(case['projection'], direction, u, v, 0), run(case['projection'], direction, u, v, 1)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, second)), 'the alignment changes the result'
        _MEASURED[key] = (u, v, first, ratios(case, direction, first))
    return _MEASURED[key]


@pytest.mark.parametrize('direction', ['forward', 'inverse'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_case_against_mpmath(case, direction):
    u, v, got, measured = measure(case, direction)
    if direction == 'inverse':
        lon = got[1][~np.isnan(got[1])]
        assert np.all((lon >= -180) & (lon < 180)), lon[(lon < -180) | (lon >= 180)]
    failed = []
    for k, (rel, lim) in enumerate(measured):
        i = int(np.argmax(rel / lim))
        print('%s %s output %d: worst %.2f eps scale (bound %.1f) at point %d' % (case['name'], direction, k, rel[i], lim[i], i))
        if not np.all(rel <= lim):
            failed.append((k, i, float(rel[i]), float(lim[i]), float(u[i]), float(v[i])))
    assert not failed, (case['name'], direction, failed)


def test_worst_ratio_per_family():
    """the table of the module docstring (-s); asserts again, per family, what the test above asserts per case"""
    overall = 0.0
    for fam in K.FAMILIES:
        row = []
        for direction in ('forward', 'inverse'):
            for k in (0, 1):
                worst = 0.0
                for case in CASES:
                    if case['family'] == fam:
                        rel, lim = measure(case, direction)[3][k]
                        assert np.all(rel <= lim), (case['name'], direction, k)
                        worst = max(worst, float(rel.max()))
                row.append(worst)
        overall = max(overall, max(row))
        print('%-10s forward x %.2f y %.2f   inverse lat %.2f lon %.2f' % ((fam,) + tuple(row)))
    print('worst overall: %.2f eps scale' % overall)


def test_centre_maps_to_centre():
    for name, P in K.projections():
        lat, lon = run(P, 'inverse', np.array([0.0, -0.0, 0.0, -0.0]), np.array([0.0, 0.0, -0.0, -0.0]), 0)
        assert np.all(np.abs(lat - P['lat0']) <= 8 * K.EPS * 90), (name, lat)
        if abs(P['lat0']) < 90:
            assert np.all(K.lon_distance(lon, P['lon0']) <= 8 * K.EPS * 180 / np.cos(np.deg2rad(P['lat0']))), (name, lon)
        else:
            assert np.all(K.lon_distance(lon, P['lon0']) == 0), (name, lon)
        x, y = run(P, 'forward', np.array([P['lat0']]), np.array([P['lon0']]), 1)
        assert np.all(np.abs(x) <= 8 * K.EPS * P['a']) and np.all(np.abs(y) <= 8 * K.EPS * P['a']), (name, x, y)


def test_empty_and_bad_arguments():
    from auromat_amd._native import Context, NativeError, Projection
    ctx = Context.current()
    p = _struct(O.stere(45.0, 10.0))
    buf = Buffer(4, 0, np.zeros(4))
    for name in ('amt_project_forward', 'amt_project_inverse'):
        ctx.call(name, C.byref(p), None, None, 0, None, None)
        ctx.call(name, C.byref(p), buf.ptr, buf.ptr, 0, buf.ptr, buf.ptr)
        with pytest.raises(NativeError):
            ctx.call(name, C.byref(p), buf.ptr, buf.ptr, -1, buf.ptr, buf.ptr)
        with pytest.raises(NativeError):
            ctx.call(name, C.byref(p), None, buf.ptr, 4, buf.ptr, buf.ptr)
        with pytest.raises(NativeError):
            ctx.call(name, None, buf.ptr, buf.ptr, 4, buf.ptr, buf.ptr)
        with pytest.raises(NativeError):
            ctx.call(name, C.byref(Projection()), buf.ptr, buf.ptr, 4, buf.ptr, buf.ptr)          # never filled
    assert np.array_equal(buf.host(), np.zeros(4))


def test_classes_keep_type_and_shape():
    import torch
    from auromat_amd._native import Context
    from auromat_amd.coordinates.projection import PolarAzimuthalEquidistant, Stereographic
    rng = np.random.RandomState(5)
    lat, lon = rng.uniform(40, 80, (3, 5, 7)), rng.uniform(-30, 50, (3, 5, 7))
    for proj, P in ((Stereographic(60.0, 10.0), O.stere(60.0, 10.0)), (PolarAzimuthalEquidistant(True), O.paeqd(True))):
        x, y = proj.forward(lat, lon)
        assert isinstance(x, np.ndarray) and x.shape == y.shape == lat.shape and x.dtype == np.float64
        wx, wy = run(P, 'forward', lat.ravel(), lon.ravel(), 0)
        assert np.array_equal(x.ravel(), wx) and np.array_equal(y.ravel(), wy)
        dev = Context.current().device
        tx, ty = proj.forward(torch.from_numpy(lat).to(dev), torch.from_numpy(lon).to(dev))
        assert isinstance(tx, torch.Tensor) and tx.is_cuda and tuple(tx.shape) == lat.shape
        assert np.array_equal(tx.cpu().numpy(), x) and np.array_equal(ty.cpu().numpy(), y)
        la, lo = proj.inverse(x, y)
        assert la.shape == lat.shape and np.max(np.abs(la - lat)) < 1e-11 and np.max(np.abs(lo - lon)) < 1e-10
        tla, tlo = proj.inverse(tx, ty)
        assert tla.is_cuda and np.array_equal(tla.cpu().numpy(), la) and np.array_equal(tlo.cpu().numpy(), lo)
        e0, e1 = proj.forward(np.zeros((0, 4)), np.zeros((0, 4)))
        assert e0.shape == e1.shape == (0, 4)
        with pytest.raises(ValueError):
            proj.forward(np.zeros(3), np.zeros(4))
