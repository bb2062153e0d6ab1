"""
Supersampled gathering on the host: where the sub-samples lie (gather_subsample_coordinates against the oracle's restatement, on
real grids), the oracle's reduction (tests/_gather_supersample_oracle.py) on hand-written 2 x 2 cells with known answers,
supersample_min_count, and the refusals, which come before any device call — this machine has no device, a device call would
raise NativeError — and in a stated order.
"""
import os

import numpy as np
import pytest

import _gather_supersample_oracle as SO

N = np.nan


def _plan(grid, dateline=False):
    return dict(grid=grid, contains_pole=False, contains_discontinuity=dateline, altitude=110.0)


@pytest.mark.parametrize('box,ppd,dateline', [((40.0, 50.0, 10.0, 20.0), (10, 10), False),
                                              ((-33.7, -31.2, 100.3, 104.9), (7, 13), False),
                                              ((-5.0, 5.0, -10.0, 5.0), (4, 4), True)])      # (a shifted box: 170 E ... 175 W)
def test_sub_sample_axes_on_real_grids(box, ppd, dateline):
    from auromat_amd.mapping.mapping import wrap_at_180
    from auromat_amd.resample import _Grid, gather_subsample_coordinates
    grid = _Grid(ppd, *box)
    for n in range(1, 9):
        sub = gather_subsample_coordinates(_plan(grid, dateline), n)
        assert sub['cell_lat'] is None and sub['cell_lon'] is None
        lat, lon = sub['lat'], sub['lon']
        assert lat.dtype == np.float64 and lon.dtype == np.float64 and lat.shape == (grid.ny * n,) and lon.shape == (grid.nx * n,)
        want_lat, want_lon = SO.sub_axis(grid.lat[:, 0], n), SO.sub_axis(grid.lon[0, :], n)
        assert np.array_equal(lat, want_lat)                                      # bit for bit
        assert np.array_equal(lon, wrap_at_180(want_lon + 180) if dateline else want_lon)
        # strictly monotonic (latitudes descend), and every sub-sample strictly inside its cell
        assert (np.diff(want_lat) < 0).all() and (np.diff(want_lon) > 0).all()
        cl, co = grid.lat[:, 0], grid.lon[0, :]
        la, lo = want_lat.reshape(grid.ny, n), want_lon.reshape(grid.nx, n)
        assert (la < cl[:-1, None]).all() and (la > cl[1:, None]).all()
        assert (lo > co[:-1, None]).all() and (lo < co[1:, None]).all()
        if dateline:
            assert (lon >= -180).all() and (lon < 180).all() and (np.diff(lon) < 0).sum() == 1      # one wrap
    # n = 1: the cells' centres, up to the rounding of the grid's own
    one = gather_subsample_coordinates(_plan(grid), 1)
    assert np.allclose(one['lat'], grid.lat_c[:, 0], rtol=0, atol=1e-12) and np.allclose(one['lon'], grid.lon_c[0, :], rtol=0, atol=1e-12)


def _fine(img, seen, elev=None, source=None):
    img = np.asarray(img)
    img = img[:, :, None] if img.ndim == 2 else img
    seen = np.asarray(seen, dtype=bool)
    elev = np.zeros(seen.shape) if elev is None else np.asarray(elev, dtype=np.float64)
    source = np.where(seen, 0, -1) if source is None else np.asarray(source)
    return dict(img=img, mask=~seen, elevation=elev, source=source.astype(np.int32))


def test_reduction_on_hand_written_cells():
    # one row of four cells, 2 x 2 sub-samples each:   sum 5 / 2       sum 7 / 2        sum 10 / 4       nobody
    img = np.array([[2, 3,   3, 4,   1, 2,   9, 9],
                    [9, 9,   9, 9,   3, 4,   9, 9]], dtype=np.uint8)
    seen = np.array([[1, 1,   1, 1,   1, 1,   0, 0],
                     [0, 0,   0, 0,   1, 1,   0, 0]])
    r = SO.reduce_cells(_fine(img, seen), 2, 1)
    assert r['count'].tolist() == [[2, 2, 4, 0]] and r['count'].dtype == np.uint8
    assert r['img'][0, :, 0].tolist() == [2, 4, 2, 0] and r['img'].dtype == np.uint8         # half to even: 2.5 -> 2, 3.5 -> 4
    assert r['mask'].tolist() == [[False, False, False, True]] and r['source'].tolist() == [[0, 0, 0, -1]]
    assert r['elevation'][0, :3].tolist() == [0.0, 0.0, 0.0] and np.isnan(r['elevation'][0, 3])
    # min_count: the cells with two seen sub-samples go, their count stays
    r = SO.reduce_cells(_fine(img, seen), 2, 3)
    assert r['mask'].tolist() == [[True, True, False, True]] and r['count'].tolist() == [[2, 2, 4, 0]]
    assert r['img'][0, :, 0].tolist() == [0, 0, 2, 0] and r['source'].tolist() == [[-1, -1, 0, -1]]
    assert np.isnan(r['elevation'][0, [0, 1, 3]]).all() and r['elevation'][0, 2] == 0.0
    # uint16 sums do not wrap: four times 65535
    r = SO.reduce_cells(_fine(np.full((2, 2), 65535, np.uint16), np.ones((2, 2))), 2, 4)
    assert r['img'].tolist() == [[[65535]]] and r['img'].dtype == np.uint16


def test_float_sums_are_ordered_and_skip_the_unseen():
    big = np.float32(2.0 ** 60)
    # ((big + 1) - big) + 1 = 1 in float64 in row-major order; any other order gives 2 or 0
    img = np.array([[big, 1.0], [-big, 1.0]], dtype=np.float32)
    elev = np.array([[2.0 ** 60, 1.0], [-2.0 ** 60, 1.0]])
    r = SO.reduce_cells(_fine(img, np.ones((2, 2)), elev), 2, 1)
    assert r['img'].dtype == np.float32 and r['img'][0, 0, 0] == np.float32(0.25) and r['elevation'][0, 0] == 0.25
    # the unseen sub-sample is skipped, NaN or not, and the division is by the count of the seen
    img = np.array([[1.5, N], [2.0, 4.0]], dtype=np.float32)
    elev = np.array([[10.0, N], [20.0, 60.0]])
    r = SO.reduce_cells(_fine(img, [[1, 0], [1, 1]], elev), 2, 1)
    assert r['count'].tolist() == [[3]] and r['img'][0, 0, 0] == np.float32(7.5 / 3.0) and r['elevation'][0, 0] == 30.0
    # the first seen value starts the sum: a lone -0.0 stays -0.0
    r = SO.reduce_cells(_fine(np.array([[9.0, 9.0], [9.0, -0.0]], np.float32), [[0, 0], [0, 1]]), 2, 1)
    assert r['img'][0, 0, 0] == 0.0 and np.signbit(r['img'][0, 0, 0])
    # the mean is rounded to float32 once, from the float64 quotient
    img = np.array([[1.0, 1.0], [1.0, 2.0]], dtype=np.float32)
    r = SO.reduce_cells(_fine(img, [[1, 1], [1, 0]]), 2, 1)
    assert r['img'][0, 0, 0] == np.float32(1.0) and SO.reduce_cells(_fine(img, np.ones((2, 2))), 2, 1)['img'][0, 0, 0] == np.float32(1.25)


def test_majority_source_its_tie_and_the_empty_cell():
    #                   3 of 4: 5      tie 2 : 2 -> 1    one seen: 7      nobody
    source = np.array([[5, 5,   4, 1,   -1, -1,   -1, -1],
                       [2, 5,   1, 4,   -1, 7,    -1, -1]])
    seen = source >= 0
    elev = np.where(seen, 10.0 * source, N)
    r = SO.reduce_cells(_fine(np.ones((2, 8), np.uint8), seen, elev, source), 2, 1)
    assert r['source'].tolist() == [[5, 1, 7, -1]] and r['source'].dtype == np.int32
    assert r['count'].tolist() == [[4, 4, 1, 0]] and r['mask'].tolist() == [[False, False, False, True]]
    assert r['elevation'][0, :3].tolist() == [42.5, 25.0, 70.0] and np.isnan(r['elevation'][0, 3])
    assert r['img'][0, :, 0].tolist() == [1, 1, 1, 0]
    # the empty cell stays empty whatever min_count, and 2-d grids of cells keep their shape
    r = SO.reduce_cells(_fine(np.ones((4, 6, 3), np.uint8), np.zeros((4, 6))), 2, 4)
    assert r['img'].shape == (2, 3, 3) and not r['img'].any() and r['mask'].all() and (r['source'] == -1).all()
    assert np.isnan(r['elevation']).all() and not r['count'].any()


def test_min_count_of_a_coverage():
    from auromat_amd.resample import supersample_min_count
    assert supersample_min_count(0.5, 3) == 5 and supersample_min_count(1.0, 8) == 64 and supersample_min_count(1e-9, 4) == 1
    assert supersample_min_count(None, 2) == 2 and supersample_min_count(None, 3) == 5 and supersample_min_count(None, 8) == 32
    for n in range(1, 9):
        assert supersample_min_count(1.0, n) == n * n and 1 <= supersample_min_count(None, n) <= n * n


class _Member(object):
    """a mapping that raises as soon as anything is asked of it beyond what a refusal needs"""
    identifier, altitude = 'm', 110.0


def test_refusals_and_their_order():
    from auromat_amd.resample import (gather_frame, gather_mosaic_frames, resampleGather, resampleGatherMLatMLT,
                                      resampleGatherMosaic, resampleGatherMosaicMLatMLT)
    m = _Member()
    calls = [lambda **kw: resampleGather(m, **kw), lambda **kw: resampleGatherMLatMLT(m, **kw),
             lambda **kw: resampleGatherMosaic([m], **kw), lambda **kw: resampleGatherMosaicMLatMLT([m], **kw),
             lambda **kw: gather_frame(dict(), None, **kw), lambda **kw: gather_mosaic_frames(dict(), **kw)]
    for call in calls:
        for bad in (0, 9, -1, 2.0, '2', None, True, False):
            with pytest.raises(ValueError, match='supersample must be an int'):
                call(supersample=bad)
        for bad in (0, 0.0, -0.5, 1.0000001, 2, N, 'half'):
            with pytest.raises(ValueError, match='minCoverage must be'):
                call(supersample=2, minCoverage=bad)
        with pytest.raises(ValueError, match='goes with supersample > 1'):
            call(minCoverage=0.5)
        with pytest.raises(ValueError, match='goes with supersample > 1'):
            call(supersample=1, minCoverage=1.0)
        # the order: the interpolation, then supersample, then minCoverage's range, then the two together
        with pytest.raises(ValueError, match='interpolation must be'):
            call(interpolation='cubic', supersample=0, minCoverage=7)
        with pytest.raises(ValueError, match='supersample must be an int'):
            call(supersample=0, minCoverage=7)
        with pytest.raises(ValueError, match='minCoverage must be'):
            call(supersample=1, minCoverage=7)


def test_symbols_and_the_unchanged_refusal_of_collections():
    from auromat_amd import _native
    from auromat_amd import resample as R
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'auromat_hip.h')).read()
    assert 'amt_gather_mosaic_supersampled' in _native._SIGNATURES and 'int amt_gather_mosaic_supersampled(amt_ctx* ctx' in header
    assert 'amt_gather_mosaic_supersampled' in _native.exported_symbols()
    assert '#define AMT_ABI_VERSION 10' in header and _native.ABI_VERSION == 10
    args, _ = _native._SIGNATURES['amt_gather_mosaic_supersampled']
    assert len(args) == len(_native._SIGNATURES['amt_gather_mosaic'][0]) + 2
    for name in ('gather_subsample_coordinates', 'supersample_min_count'):
        assert callable(getattr(R, name)), name
    mapping = _Member()
    for call in (R.resampleGather, R.resampleGatherMLatMLT):
        with pytest.raises(NotImplementedError, match='collections'):
            call([mapping, mapping], supersample=2)
        with pytest.raises(NotImplementedError, match='collections'):
            call([mapping, mapping], supersample=4, minCoverage=0.25)
