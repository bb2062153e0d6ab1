"""Quantile binning without a GPU: the NumPy statement of the feature (tests/_quantile_oracle.py: the restated arithmetic
against a literal np.quantile per cell), the library's host rank rule (amt_quantile_rank, the function the kernels call)
against that statement, the public names, the exported symbols, and the refusal of bad quantiles by the Python layer, the
C entry points and the command line."""
import ctypes as C
import inspect

import numpy as np
import pytest

import _quantile_oracle as Q

# q = 0 and 1e-9: rank 0; 1: the vi >= n-1 clamp; 0.5, 0.25, 0.75: g exactly 0 or 0.5 by n mod 4; 1/3: an inexact vi; 0.999: a
# pair among the top keys
EDGE_QS = (0.0, 1.0, 0.5, 0.25, 0.75, 1.0 / 3.0, 0.999, 1e-9)
RANK_NS = (1, 2, 3, 64, 65, 16384, 16385, 300001, 2 ** 31 - 1)


def _points(rng, xedges, yedges, n):
    x = rng.uniform(xedges[0] - 0.5, xedges[-1] + 0.5, n)
    y = rng.uniform(yedges[0] - 0.5, yedges[-1] + 0.5, n)
    x[::997] = np.nan
    return x, y


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float64])
def test_restated_arithmetic_equals_a_per_cell_np_quantile(dtype):
    rng = np.random.RandomState(5)
    xedges, yedges = np.linspace(0.0, 4.0, 9), np.linspace(-2.0, 1.0, 7)
    x, y = _points(rng, xedges, yedges, 12000)
    # cells of 1, 2 and 3 pixels beside the ~100-pixel ones: four more columns, the first takes the points beyond the old edge
    xedges = np.concatenate([xedges, [5.0, 6.0, 7.0, 8.0]])
    x = np.concatenate([x, [5.5, 6.5, 6.5, 7.5, 7.5, 7.5]])
    y = np.concatenate([y, np.full(6, 0.75)])
    if dtype == np.float64:
        v = rng.normal(0, 30, (len(x), 3))
        v[::5] = -np.abs(v[::5])
        v[-6:, 0] = [-0.0, -0.0, 0.0, -1e-300, 5e-324, 3.5]
    else:
        v = rng.randint(0, np.iinfo(dtype).max + 1, (len(x), 3)).astype(dtype)
    keep = rng.uniform(size=len(x)) > 0.1
    keep[-6:] = True
    qs = EDGE_QS + tuple(rng.uniform(0, 1, 5))
    got, count = Q.quantile_bins(x, y, v, xedges, yedges, qs, keep=keep)
    want = Q.quantile_loop(x, y, v, xedges, yedges, qs, keep=keep)
    assert got.shape == want.shape == (len(qs), 6, 12, 3)
    assert got.tobytes() == want.tobytes()                      # bit for bit, the sign of a zero included
    assert np.array_equal(np.isnan(got[0, ..., 0]), count == 0)
    assert {1, 2, 3} <= set(count.ravel().astype(int).tolist()) and count.max() > 64


def test_quantile_half_is_not_the_median_of_float_planes():
    """np.median averages the middle pair, np.quantile(0.5) lerps it: the two differ in the last bit of some float cells and
    never on integer-valued planes (which is why the median entry points keep a combine rule of their own)."""
    rng = np.random.RandomState(2)
    differ = 0
    for _ in range(4000):
        v = rng.normal(0, 30, 2 * rng.randint(1, 30))
        differ += np.quantile(v, 0.5) != np.median(v)
        u = rng.randint(0, 65536, v.size).astype(np.float64)
        assert np.quantile(u, 0.5) == np.median(u)
    assert differ > 0


def _lib_rank(n, q):
    from auromat_amd import _native
    k, k2, g = C.c_int64(-7), C.c_int64(-7), C.c_double(-7.0)
    rc = _native.lib().amt_quantile_rank(int(n), float(q), C.byref(k), C.byref(k2), C.byref(g))
    return rc, k.value, k2.value, g.value


def test_host_rank_rule_equals_the_restated_one():
    rng = np.random.RandomState(9)
    cases = [(n, q) for n in RANK_NS for q in EDGE_QS]
    ns = np.concatenate([rng.randint(1, 400001, 9000), rng.randint(1, 2 ** 31 - 1, 1000)])
    cases += list(zip(ns.tolist(), rng.uniform(0, 1, 10000).tolist()))
    for n, q in cases:
        rc, k, k2, g = _lib_rank(n, q)
        wk, wk2, wg = Q.rank_pair(n, q)
        assert rc == 0
        assert (k, k2) == (int(wk), int(wk2)), (n, q)
        assert np.float64(g).tobytes() == np.float64(wg).tobytes(), (n, q)
        assert 0 <= k <= k2 <= n - 1 and k2 - k <= 1 and (0.0 <= g < 1.0 if k2 > k else g == (n - 1) * q + 1.0)
    # what the edge values are there for
    assert _lib_rank(300001, 0.0)[1:] == (0, 1, 0.0) and _lib_rank(300001, 1e-9)[1:3] == (0, 1)
    assert _lib_rank(300001, 1.0)[1:] == (300000, 300000, 300001.0) and _lib_rank(1, 0.3)[1:] == (0, 0, 1.0)
    assert [_lib_rank(n, 0.25)[3] for n in (5, 6, 7, 8)] == [0.0, 0.25, 0.5, 0.75]
    assert [_lib_rank(n, 0.5)[3] for n in (64, 65)] == [0.5, 0.0]
    assert _lib_rank(16385, 0.999)[1:3] == (16367, 16368)


def test_host_rank_rule_refuses_bad_arguments():
    from auromat_amd import _native
    for n, q in ((0, 0.5), (-3, 0.5), (5, -0.1), (5, 1.1), (5, float('nan')), (5, float('inf'))):
        assert _lib_rank(n, q) == (-1, -7, -7, -7.0)
    k = C.c_int64()
    assert _native.lib().amt_quantile_rank(5, 0.5, None, C.byref(k), None) == -1


def test_public_names_and_signatures():
    from auromat_amd import resample as R
    from auromat_amd.pipeline import FramePipeline, SequencePipeline
    sig = inspect.signature(R.resampleQuantile)
    assert list(sig.parameters) == ['mappingOrCollection', 'q', 'pxPerDeg', 'arcsecPerPx', 'containsPole']
    assert sig.parameters['q'].default is inspect.Parameter.empty
    assert sig.parameters['pxPerDeg'].default == 25
    assert sig.parameters['arcsecPerPx'].default is None and sig.parameters['containsPole'].default is None
    assert list(inspect.signature(R.resampleQuantileMLatMLT).parameters) == ['mapping', 'q', 'kw']
    assert 'q' in inspect.signature(R.resample_frame_quantile).parameters
    assert 'q' in inspect.signature(FramePipeline.resample).parameters
    assert 'q' in inspect.signature(FramePipeline.run).parameters
    assert inspect.signature(SequencePipeline.__init__).parameters['quantile'].default is None
    # the median keeps its names and the mean its refusal of method='median'
    assert list(inspect.signature(R.resampleMedian).parameters) == ['mappingOrCollection', 'pxPerDeg', 'arcsecPerPx',
                                                                    'containsPole']
    with pytest.raises(NotImplementedError):
        R._check_method('median')


def test_symbols_and_abi_version():
    from auromat_amd import _native
    lib = _native.lib()
    for name in ('amt_quantile_frame', 'amt_quantile_frame_async', 'amt_quantile_rank', 'amt_run_set_quantile'):
        assert name in _native.exported_symbols() and hasattr(lib, name), name
    assert _native.ABI_VERSION == 10 and lib.amt_abi_version() == 10
    assert _native.QUANTILES_MAX == 8


BAD_QS = (-0.1, 1.1, float('nan'), float('inf'), (), [], (0.5, 1.5), (0.1,) * 9, 'x', None)


@pytest.mark.parametrize('q', BAD_QS, ids=[repr(q) for q in BAD_QS])
def test_bad_quantiles_raise_before_any_device_work(q):
    """ValueError from the argument alone: the mapping is an object nothing can be read from."""
    from auromat_amd import resample as R
    from auromat_amd.pipeline import SequencePipeline
    with pytest.raises(ValueError):
        R.quantile_list(q)
    with pytest.raises(ValueError):
        R.resampleQuantile(object(), q)
    with pytest.raises(ValueError):
        R.resample_frame_quantile(object(), 110, None, (10, 10), q)
    if q is not None:
        with pytest.raises(ValueError):
            SequencePipeline(64, 48, statistic='quantile', quantile=q)


def test_good_quantiles_are_taken_as_floats_in_order():
    from auromat_amd import resample as R
    assert R.quantile_list(0) == [0.0] and R.quantile_list(1) == [1.0] and R.quantile_list(np.float32(0.5)) == [0.5]
    assert R.quantile_list((0.75, 0.25, 0.75)) == [0.75, 0.25, 0.75]
    assert R.quantile_list(np.linspace(0, 1, 8)) == np.linspace(0, 1, 8).tolist()


@pytest.mark.parametrize('entry', ['amt_quantile_frame', 'amt_quantile_frame_async'])
def test_c_entry_points_refuse_bad_quantiles_first(entry):
    """The invalid-argument status for nq = 0, nq = 9, q = -0.1, q = 1.1 and NaN: the quantiles are the first thing an entry
    point looks at, before its context and its device pointers (none of which exists here)."""
    from auromat_amd import _native
    fn = getattr(_native.lib(), entry)
    extra = [0] if entry.endswith('_async') else []

    def call(qs, nq):
        arr = (C.c_double * max(len(qs), 1))(*qs)
        return fn(None, None, None, None, None, 1, 3, None, 4, 4, 0.0, None, None, 0, *(extra + [arr, nq, None, None, None, None]))

    assert call([0.5], 0) == -1
    assert call([0.5] * 9, 9) == -1
    assert call([0.5], -1) == -1
    for bad in (-0.1, 1.1, float('nan')):
        assert call([bad], 1) == -1
        assert call([0.25, bad, 0.75], 3) == -1
    assert fn(None, None, None, None, None, 1, 3, None, 4, 4, 0.0, None, None, 0, *(extra + [None, 1, None, None, None, None])) == -1


BASE = ['--data', 'in', '--format', 'netcdf', '--resample']


def test_quantile_option_parsing(capsys):
    from auromat_amd.cli.convert import parseargs
    args = parseargs(BASE + ['--statistic', 'quantile', '--quantile', '0.75'])
    assert args.statistic == 'quantile' and args.quantile == 0.75
    assert parseargs(BASE + ['--statistic', 'quantile', '--quantile', '0']).quantile == 0.0
    assert parseargs(BASE).quantile is None and parseargs(BASE + ['--statistic', 'median']).quantile is None
    for argv in (BASE + ['--statistic', 'quantile'],                            # needed with --statistic quantile
                 BASE + ['--quantile', '0.5'],                                    # refused with the mean
                 BASE + ['--statistic', 'median', '--quantile', '0.5'],          # and with the median
                 BASE + ['--statistic', 'quantile', '--quantile', '1.5'],
                 BASE + ['--statistic', 'quantile', '--quantile', 'nan'],
                 ['--data', 'in', '--format', 'netcdf', '--statistic', 'quantile', '--quantile', '0.5']):   # needs --resample
        with pytest.raises(SystemExit) as e:
            parseargs(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
