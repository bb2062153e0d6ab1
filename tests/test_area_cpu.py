"""
The contract of the area-weighted binning, without a GPU: tests/_area_oracle.py (the NumPy restatement that the device is
compared with bit for bit) against exact answers, and the cases of tests/_area_cases.py against what they claim to aim at.

(a) dyadic coordinates: every overlap is exactly representable, the expected weights come from rational arithmetic
    (Sutherland-Hodgman + shoelace in ``fractions.Fraction``), and the oracle must give exactly those integers.
(b) tiling: on a real frame the quadrilaterals of neighbouring pixels share their edges, so a cell inside the covered region
    (itself and its eight neighbours covered > 0.999) has total weight 2^32 up to rounding: every W carries half a unit, so
    |sum(W) - 2^32| <= n / 2 + 1 for a cell with n contributing pixels (1: the geometry's own rounding, ~2e-14 deg against
    cells of 0.1 and 0.5 deg, far below a unit).  Measured: 3 (n <= 13) on 3680 such cells at 10 px/deg, 7 (n <= 97) on 85
    at 2 px/deg.
(c) no cell that centre binning fills has coverage 0 (measured: 0 of 3060).
(d) the hole the feature closes: at 10 px/deg at least a quarter of the fully covered cells are empty under centre binning
    (measured: 1073 of 4014).
(e) the constructed cases aim where they claim.

The grid of (b) - (d) is laid out for the box of the corners of the admitted pixels (64 x 103 cells), which is why the measured
figures differ by a few cells from a prototype on the box of a mapping's sanitised masks (65 x 104: 1075 of 4006, 3675 inner cells).
"""
import os
import re

import numpy as np
import pytest

import _area_cases as K
import _area_oracle as O
from conftest import ROOT, load_golden

TWO32 = 1 << 32


# ---- (a) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.dyadic_cases(), ids=repr)
def test_dyadic_cases_have_their_exact_weights(case):
    if case.quads is None:
        case.quads = K.lattice_quads(case)
    want = K.exact_weights(case)
    acc, hits = O.accumulate(case)
    assert np.array_equal(acc[0], want.astype(np.int64))
    assert np.array_equal(hits > 0, want > 0)


def test_known_answers():
    by = {c.name: c for c in K.dyadic_cases()}
    acc, hits = O.accumulate(by['half_offset_lattice'])
    # a unit-square lattice offset by half a cell: four quarters of exactly 2^30 per interior cell
    assert np.all(acc[0][1:7, 1:7] == TWO32) and np.all(hits[1:7, 1:7] == 4)
    assert acc[0][0, 0] == TWO32 // 4 and acc[0][0, 3] == TWO32 // 2 and hits[0, 0] == 1 and hits[0, 3] == 2
    acc, _ = O.accumulate(by['one_pixel_40x40'])
    assert np.all(acc[0][1:39, 1:39] == TWO32) and acc[0][0, 0] == TWO32 // 4 and acc[0][0, 7] == TWO32 // 2
    acc, _ = O.accumulate(by['diamond'])
    assert acc[0].sum() == 8 * TWO32 and acc[0][1, 1] == TWO32 and acc[0][0, 0] == 0 and acc[0][0, 1] == TWO32 // 2
    acc, _ = O.accumulate(by['bow_tie'])
    assert acc[0].sum() == 8 * TWO32            # two triangles of area 4, opposite windings, no cell shared
    for name in ('all_collinear',):
        assert not O.accumulate(by[name])[0][0].any()
    acc, hits = O.accumulate(by['all_equal'])   # the point adds nothing to the cell the square fills
    assert acc[0].sum() == TWO32 and hits.sum() == 1
    assert np.array_equal(O.accumulate(by['clockwise'])[0][0], O.accumulate(by['diamond'])[0][0])


def test_weighted_sums_and_finalise_on_a_known_cell():
    case = K.dyadic_cases()[0]
    acc, _ = O.accumulate(case)
    img = case.img.reshape(7, 7, 3).astype(np.int64)
    # interior cell (ix, iy) = (3, 2) holds a quarter of pixels (r, c) = (1..2, 2..3): corners start at 0.5
    want = img[1:3, 2:4].reshape(4, 3).sum(axis=0) * (TWO32 // 4)
    assert np.array_equal(acc[1:4, 3, 2], want)
    E = np.rint(case.elev[1:3, 2:4] * 65536.0).astype(np.int64)
    assert acc[4, 3, 2] == E.sum() * (TWO32 // 4)
    out = O.finalize(acc, np.uint8, 0.5)
    r, c = 8 - 1 - 2, 3
    assert np.array_equal(out['area'][r, c, :3], want / float(TWO32)) and out['coverage'][r, c] == 1.0 and out['mask'][r, c] == 0
    assert out['coverage'][7, 0] == 0.25 and out['mask'][7, 0] == 1 and np.isnan(out['area'][7, 0]).all()
    assert not out['img'][7, 0].any()
    assert O.finalize(acc, np.uint8, 0.25)['mask'][7, 0] == 0 and O.finalize(acc, np.uint8, 0.0)['mask'].sum() == 0


def test_min_weight_rule():
    assert O.min_weight(0) == 1 and O.min_weight(0.5) == 1 << 31 and O.min_weight(1) == TWO32
    acc = np.zeros((2, 3, 1), dtype=np.int64)
    for least in (1, 1 << 31, TWO32):
        acc[0, :, 0] = (least - 1, least, least + 1)
        assert O.finalize(acc, np.uint8, least=least)['mask'][0].tolist() == [1, 0, 0]
    acc[0, :, 0] = (O.LIMIT - 1, O.LIMIT, O.LIMIT + 1)
    assert O.finalize(acc, np.uint8)['over'] and not O.finalize(acc[:, :2], np.uint8)['over']


# ---- (b) - (d) -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    z = load_golden('georef_small_iss030_fast.npz')
    out = {}
    for ppd in (10, 2):
        case = K.golden_case(z, ppd)
        acc, hits = O.accumulate(case)
        out[ppd] = (case, acc, hits, K.centre_counts(case, z['lon_c']))
    return out


def _inner(full):
    p = np.pad(full, 1, mode='constant')
    nb = np.ones_like(full)
    for dx in range(3):
        for dy in range(3):
            nb &= p[dx:dx + full.shape[0], dy:dy + full.shape[1]]
    return nb


@pytest.mark.parametrize('ppd,least_cells', [(10, 3000), (2, 50)])
def test_tiling(golden, ppd, least_cells):
    case, acc, hits, _ = golden[ppd]
    assert len(O.admitted(case)[0]) == 5951
    inner = _inner(acc[0] / float(TWO32) > 0.999)
    assert inner.sum() >= least_cells
    dev, n = np.abs(acc[0][inner] - TWO32), hits[inner]
    print('ppd %d: %d inner cells, max |sum(W) - 2^32| = %d, max n = %d' % (ppd, inner.sum(), dev.max(), n.max()))
    assert np.all(dev <= n / 2.0 + 1)


def test_every_centre_binned_cell_is_covered(golden):
    _, acc, _, centre = golden[10]
    assert (centre > 0).sum() == 3060
    assert not ((centre > 0) & (acc[0] == 0)).any()


def test_centre_binning_leaves_holes_that_area_weighting_fills(golden):
    _, acc, _, centre = golden[10]
    full = acc[0] / float(TWO32) > 0.999
    holes = full & (centre == 0)
    print('%d of %d fully covered cells are empty under centre binning' % (holes.sum(), full.sum()))
    assert full.sum() > 3500 and 4 * holes.sum() >= full.sum()
    # ... and at 2 px/deg, cells much larger than pixels, neither method leaves one
    _, acc2, _, centre2 = golden[2]
    assert not ((acc2[0] / float(TWO32) > 0.999) & (centre2 == 0)).any()


# ---- (e) -------------------------------------------------------------------------------------------------------------------
def test_cases_aim_where_they_claim():
    src = open(os.path.join(ROOT, 'auromat_amd', 'csrc', 'amt_area.hip')).read()
    assert int(re.search(r'constexpr int kLaneCells = (\d+);', src).group(1)) == K.LANE_CELLS
    assert int(re.search(r'constexpr int kAreaBlock = (\d+);', src).group(1)) == K.BLOCK
    counts = lambda c: K.candidate_counts(c)
    assert set(counts(K.heavy_cell_case())) == {1}                                    # one cell
    few = counts(K.golden_case(load_golden('georef_small_iss030_fast.npz'), 2))
    assert few.min() == 1 and 1 < few.max() <= K.LANE_CELLS                           # a few cells per lane
    assert counts(K.wide_pixel_case()).tolist() == [70 * 70]                          # >= 65 cells: past one wave's lanes
    alt = counts(K.alternating_case())
    assert alt[0::2].tolist() == [1] * 10 and alt[1::2].tolist() == [5000] * 10 and len(alt) <= 64
    # both sides of the threshold between the lane path and the wave path occur
    every = np.concatenate([counts(c) for c in K.device_cases()])
    assert (every == K.LANE_CELLS).any() and ((every > K.LANE_CELLS) & (every < 64)).any() and (every > 64).any()
    # shapes: width 1, 255, 257 and two workgroups plus one pixel; misaligned coordinates
    shapes = {(c.height, c.width) for c in K.shape_cases()}
    assert {1, 255, 257, 2 * K.BLOCK + 1} <= {w for _, w in shapes} and any(c.coord_offset == 1 for c in K.shape_cases())
    # every skip rule is hit
    skipped = O.admitted(K.skip_case())[3]
    assert skipped == dict(centre=2, elevation=2, mask=1, corner=skipped['corner'], extent=1) and skipped['corner'] >= 4
    assert O.admitted(K.axis_cases()[2])[3]['extent'] >= 8                            # the seam without the wrap
    # outside: pixels wholly outside, and pixels across each of the four borders
    out = K.outside_case()
    _, X, Y, _ = O.admitted(out)
    ex, ey = out.xedges, out.yedges
    assert (counts(out) == 0).any()
    for v, e in ((X, ex), (Y, ey)):
        assert ((v.min(axis=1) < e[0]) & (v.max(axis=1) > e[0])).any() and ((v.min(axis=1) < e[-1]) & (v.max(axis=1) > e[-1])).any()
    # the coverage limit: exactly 2^40 with 256 pixels, past it with 257
    for n, over in ((256, False), (257, True)):
        acc, _ = O.accumulate(K.coverage_limit_case(n))
        assert acc[0][0, 0] == n * TWO32 and acc[0].sum() == n * TWO32 and O.finalize(acc, np.uint8)['over'] == over
    # formats
    fmts = {(c.img.dtype.name, c.img.shape[1]) for c in K.format_cases()}
    assert fmts >= {(d, n) for d in ('uint8', 'uint16') for n in (0, 1, 3, 4)}
    assert any(c.elev is None for c in K.format_cases()) and any(c.mask is not None for c in K.format_cases())
    assert any(not c.uniform for c in K.axis_cases()) and any(c.lon_wrap for c in K.axis_cases())


def test_candidate_range_does_not_matter():
    """A cell with W = 0 receives nothing: the result on a grid equals the result on a sub-grid of the same edges."""
    case = K.outside_case()
    acc, hits = O.accumulate(case)
    big = K.lattice('outside_big', 12, 14, K.unit_edges(16, 0.5, 0.0), K.unit_edges(13, 0.5, -1.0), 0.3, -0.4, 0.45, 0.42,
                    jitter=0.3, seed=61)
    acc_big, _ = O.accumulate(big)
    assert np.array_equal(big.xedges[4:11], case.xedges) and np.array_equal(big.yedges[4:10], case.yedges)
    assert np.array_equal(acc_big[:, 4:10, 4:9], acc)
