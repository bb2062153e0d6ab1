"""
The contract of the area-weighted mosaic (``resampleMosaic(statistic='area')``, ``amt_area_mosaic_frames``) without a GPU:
tests/_mosaic_area_oracle.py (the NumPy statement that the device is compared with bit for bit) against rational arithmetic and
against the properties that follow from the contract, the keyword rules of the Python layer, the declaration of the entry point,
and the collections of tests/_mosaic_area_cases.py against what they claim to aim at.

The hole the feature closes, on the all-sky pair of tests/test_gpu_mosaic_area.py (Sodankyla and Kevo at 128 x 128 pixels,
pixels below 10 deg elevation masked, 20 px/deg, ``mayOverlap=True``, minCoverage 0.5), with the oracles alone: the mean mosaic
(tests/_mosaic_oracle.py: a pixel counts in the cell of its centre) leaves HOLES_MEASURED cells empty that the area mosaic
fills, and in WINNER_MEASURED cells that both fill the elected member differs (the mean mosaic elects by whichever centres
landed in the cell).  Measured on the 237 x 554 cells of that grid: the area mosaic fills 93435, of which the mean mosaic leaves 78136 empty (bar:
at least 100); of the 15299 cells that both fill, 2158 have another winner (bar: at least 10).
"""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _area_cases as K
import _area_oracle as O
import _mosaic_area_cases as MK
import _mosaic_area_oracle as MA
import _mosaic_oracle as MO
from conftest import ROOT, load_golden

TWO32 = 1 << 32


# ---- the oracle against rational arithmetic --------------------------------------------------------------------------------
def _dyadic_collection():
    """One-quadrilateral members on 4 x 4 unit cells, dyadic coordinates, elevations with exact fixed-point values."""
    e4 = K.unit_edges(4)
    quads = [[(2, 0), (4, 2), (2, 4), (0, 2)],                  # diamond
             [(0, 0), (4, 2), (0, 4), (2, 2)],                  # concave
             [(1.5, 1), (2.5, 2), (1.5, 3), (0.5, 2)],          # vertex on edge
             [(0.25, 0.5), (3.75, 0.5), (3.75, 3.25), (0.25, 3.25)]]
    elev = (7.5, -3.25, 12.0, 1.75)
    members = [K.quads_frame('q%d' % i, [q], e4, e4, elev=np.array([[e]]), seed=300 + i) for i, (q, e) in enumerate(zip(quads, elev))]
    return MK.Collection('dyadic', members, [(0, 0, 4, 4), (0, 0, 3, 4), (1, 1, 3, 3), (0, 1, 4, 2)])


@pytest.mark.parametrize('coverage', [0.5, 0.25, 0.0])
@pytest.mark.parametrize('rule', [0, 1])
def test_oracle_equals_rational_arithmetic(rule, coverage):
    coll = _dyadic_collection()
    least = O.min_weight(coverage)
    got = MA.mosaic(coll.members, coll.windows, rule, coverage)
    ny, nx = coll.shape
    kinds = set()
    for ix in range(nx):
        for iy in range(ny):
            own = []                                            # (member, W, [sum W v], sum W E) as Python integers
            for m, (case, (x0, y0, wnx, wny)) in enumerate(zip(coll.members, coll.windows)):
                W = int(K.exact_weights(case)[ix, iy]) if x0 <= ix < x0 + wnx and y0 <= iy < y0 + wny else 0
                E = int(Fraction(float(case.elev[0, 0])) * 65536)
                own.append((m, W, [W * int(v) for v in case.img[0]], W * E))
            if rule == 0:
                W = sum(o[1] for o in own)
                sums, se = [sum(o[2][k] for o in own) for k in range(coll.nch)], sum(o[3] for o in own)
                src = min([o[0] for o in own if o[1] > 0] or [-1]) if W >= least else -1
                cover = Fraction(W, TWO32)
            else:
                cands = [o for o in own if o[1] >= least]
                if cands:
                    top = max(Fraction(o[3], o[1]) for o in cands)
                    src, W, sums, se = next(o for o in cands if Fraction(o[3], o[1]) == top)
                    kinds.add('elected' if len(cands) > 1 else 'alone')
                else:
                    src, W, sums, se = -1, max(o[1] for o in own), None, 0
                    kinds.add('sliver' if W else 'empty')
                cover = Fraction(W, TWO32)
            r, c = ny - 1 - iy, ix
            assert got['source'][r, c] == src and got['coverage'][r, c] == float(cover), (ix, iy)
            assert got['mask'][r, c] == (0 if src >= 0 else 1)
            if src >= 0:
                # (every integer here is below 2^53: the float64 quotient is the correctly rounded fraction)
                assert [got['area'][r, c, k] for k in range(coll.nch)] == [float(Fraction(s, W)) for s in sums]
                assert got['area'][r, c, coll.nch] == float(Fraction(se, W)) / 65536.0
                assert got['img'][r, c].tolist() == [int(np.rint(float(Fraction(s, W)))) for s in sums]
            else:
                assert np.isnan(got['area'][r, c]).all() and not got['img'][r, c].any()
    assert not got['over']
    if rule == 1 and coverage == 0.5:
        assert kinds == {'elected', 'alone', 'sliver', 'empty'}


# ---- properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('whole,coll', MK.partition_cases(), ids=lambda v: repr(v))
def test_partition_property(whole, coll):
    """Under rule 0 the summed accumulators of the parts are the whole frame's, exactly: seams leave no trace."""
    want, _ = O.accumulate(whole)
    total = sum(MA.member_accumulators(m, w) for m, w in zip(coll.members, coll.windows))
    assert np.array_equal(total, want) and want[0].any()
    got = MA.mosaic(coll.members, coll.windows, 0)
    fin = O.finalize(want, whole.img.dtype, 0.5)
    for key in ('area', 'img', 'mask', 'coverage'):
        assert O.same_bits(got[key], fin[key]), key
    assert np.array_equal(got['source'] >= 0, fin['mask'] == 0)


def test_doubling_property():
    """The same member twice under rule 0: area and img are the single frame's bit for bit, the coverage is twice its value."""
    one = MK.one_member_case().members[0]
    acc, _ = O.accumulate(one)
    for coverage in (0.5, 0.0):
        least = O.min_weight(coverage)
        single = O.finalize(acc, one.img.dtype, least=least)
        twice = MA.mosaic([one, one], [MK.FULL, MK.FULL], 0, least=2 * least)
        assert O.same_bits(twice['area'], single['area']) and O.same_bits(twice['img'], single['img'])
        assert np.array_equal(twice['mask'], single['mask']) and np.array_equal(twice['coverage'], 2 * single['coverage'])
        assert np.array_equal(twice['source'], np.where(single['mask'] == 0, 0, -1))


def test_one_member_is_the_frame():
    coll = MK.one_member_case()
    acc, _ = O.accumulate(coll.members[0])
    fin = O.finalize(acc, coll.dtype, 0.5)
    for rule in (0, 1):
        got = MA.mosaic(coll.members, coll.windows, rule)
        for key in ('area', 'img', 'mask', 'coverage'):
            assert O.same_bits(got[key], fin[key]), (rule, key)
        assert np.array_equal(got['source'], np.where(fin['mask'] == 0, 0, -1))


def test_source_is_set_exactly_where_the_cell_is_valid():
    for coll in MK.device_cases():
        for rule in coll.rules:
            got = MA.mosaic(coll.members, coll.windows, rule, coll.min_coverage)
            assert np.array_equal(got['source'] >= 0, got['mask'] == 0), (coll.name, rule)
            assert got['over'] == (coll.status[rule] == MK.EDOMAIN), (coll.name, rule)


# ---- the hole the feature closes -------------------------------------------------------------------------------------------
HOLES_MEASURED, WINNER_MEASURED = 100, 10           # the bars of the issue; the measured counts stand in the docstring


def allsky_member(name, size, seed):
    """An all-sky camera's frame from its calibration (oracle.ref_numpy.allsky_georef), pixels below 10 deg masked."""
    from oracle import ref_numpy as R
    z = load_golden(name)
    cal = dict((k, float(z['cal_' + k])) for k in ('lat', 'lon', 'xc', 'yc', 'k', 'rotation'))
    g = R.allsky_georef(size, cal, 110)
    with np.errstate(invalid='ignore'):
        keep = np.isfinite(g['lat_c']) & (g['elev'] >= 10)
    img = np.random.RandomState(seed).randint(0, 255, (size * size, 1)).astype(np.uint8)
    return dict(lat=g['lat'], lon=g['lon'], lat_c=np.where(keep, g['lat_c'], np.nan), lon_c=g['lon_c'], elev=g['elev'], img=img,
                keep=keep)


def test_area_mosaic_fills_the_holes_of_the_mean_mosaic():
    from auromat_amd.resample import cached_grid
    members = [allsky_member('miracle_sod512.npz', 128, 1), allsky_member('miracle_kev96.npz', 128, 2)]
    boxes = []
    for m in members:
        corner = np.zeros(m['lat'].shape, dtype=bool)
        for dr in (0, 1):
            for dc in (0, 1):
                corner[dr:dr + 128, dc:dc + 128] |= m['keep']
        corner &= np.isfinite(m['lat']) & np.isfinite(m['lon'])
        boxes.append((m['lat'][corner].min(), m['lat'][corner].max(), m['lon'][corner].min(), m['lon'][corner].max()))
    grid = cached_grid((20, 20), min(b[0] for b in boxes), max(b[1] for b in boxes), min(b[2] for b in boxes),
                       max(b[3] for b in boxes))
    windows = []
    for b in boxes:
        (x0, wnx), (y0, wny) = MK.axis_window(grid.xedges, b[2], b[3]), MK.axis_window(grid.yedges, b[0], b[1])
        windows.append((x0, y0, wnx, wny))
    cases = [K.AreaCase('allsky%d' % i, m['lat'], m['lon'], grid.xedges, grid.yedges, nch=1, elev=m['elev'], lat_c=m['lat_c'],
                        img=m['img']) for i, m in enumerate(members)]
    area = MA.mosaic(cases, windows, 1, 0.5)
    mean = MO.mosaic([(m['lon_c'], m['lat_c'], m['keep'], np.concatenate([m['img'].astype(np.float64), m['elev'].reshape(-1, 1)], 1),
                       w) for m, w in zip(members, windows)], grid.xedges, grid.yedges, 1, 1)
    filled = area['mask'] == 0
    holes = filled & (mean['count'] == 0)
    both = filled & (mean['count'] > 0)
    other = both & (area['source'] != mean['source'])
    print('%d x %d cells: the area mosaic fills %d, of which the mean mosaic leaves %d empty; another winner in %d of %d'
          % (grid.ny, grid.nx, filled.sum(), holes.sum(), other.sum(), both.sum()))
    assert holes.sum() >= HOLES_MEASURED and other.sum() >= WINNER_MEASURED
    assert len(np.unique(area['source'][filled])) == 2 and not area['over']
    # the area mosaic leaves no cell empty that the mean mosaic fills from a pixel whose footprint covers the cell's centre
    assert (filled | (mean['count'] == 0)).mean() > 0.99


# ---- keywords --------------------------------------------------------------------------------------------------------------
class Untouchable(object):
    """A collection that must not be looked at: every attribute raises."""

    def __getattr__(self, name):
        raise AssertionError('the collection was looked at: ' + name)


@pytest.mark.parametrize('fn', ['resampleMosaic', 'resampleMosaicMLatMLT', 'mosaic_frames'])
def test_keywords_are_refused_before_the_collection_is_looked_at(fn):
    from auromat_amd import resample as R
    f = getattr(R, fn)
    for kw in (dict(statistic='mean', minCoverage=0.5), dict(statistic='median', minCoverage=0.5),
               dict(statistic='quantile', q=0.5, minCoverage=0.1), dict(minCoverage=0.5),
               dict(statistic='area', minCoverage=1.5), dict(statistic='area', minCoverage=-0.1),
               dict(statistic='area', minCoverage=float('nan')), dict(statistic='area', minCoverage='half'),
               dict(statistic='area', q=0.5), dict(statistic='area', q=[0.5], minCoverage=0.5)):
        with pytest.raises(ValueError):
            f(Untouchable(), **kw)
    # ... and what is accepted reaches the collection
    for kw in (dict(statistic='area'), dict(statistic='area', minCoverage=0), dict(statistic='area', minCoverage=1.0)):
        with pytest.raises(AssertionError, match='looked at'):
            f(Untouchable(), **kw)


def test_statistic_names_and_signatures():
    import inspect
    from auromat_amd import resample as R
    assert R.MOSAIC_STATISTICS == ('mean', 'median', 'quantile', 'area')
    assert R.mosaic_statistic('area', None) is None and R.mosaic_statistic('area', None, 0.25) is None
    assert R.mosaic_statistic('mean', None) is None and R.mosaic_statistic('quantile', 0.5) == [0.5]
    for fn in (R.resampleMosaic, R.mosaic_frames):
        spec = inspect.getfullargspec(fn)
        assert spec.args[:7] == ['collection', 'pxPerDeg', 'arcsecPerPx', 'containsPole', 'statistic', 'q', 'minCoverage']
        assert spec.defaults[-3:] == ('mean', None, None)
    with pytest.raises(NotImplementedError):
        R.resample(Untouchable(), method='area')        # resample(method=...) keeps the reference's method list


def test_entry_point_is_declared():
    from auromat_amd._native import ABI_VERSION, AreaMosaicMember, MosaicMember, _SIGNATURES
    assert ABI_VERSION == 10 and C.sizeof(AreaMosaicMember) == 6 * 8 + 6 * 4 and C.sizeof(MosaicMember) == 5 * 8 + 6 * 4
    args, ret = _SIGNATURES['amt_area_mosaic_frames']
    assert len(args) == 16 and args[1]._type_ is AreaMosaicMember and args[10] is C.c_uint64 and ret is C.c_int
    header = open(os.path.join(ROOT, 'include', 'auromat_hip.h')).read()
    assert re.search(r'#define AMT_ABI_VERSION 10\b', header)
    decl = re.search(r'int amt_area_mosaic_frames\(([^;]*)\);', header).group(1)
    assert len(decl.split(',')) == 16 and 'const amt_area_mosaic_member* members' in decl and 'uint64_t min_weight' in decl
    struct = re.search(r'typedef struct amt_area_mosaic_member \{(.*?)\} amt_area_mosaic_member;', header, re.S).group(1)
    names = re.findall(r'(\w+)\s*[;,]', re.sub(r'/\*.*?\*/', '', struct))
    assert names == [n for n, _ in AreaMosaicMember._fields_]
    # amt_mosaic_member is what it was
    old = re.search(r'typedef struct amt_mosaic_member \{(.*?)\} amt_mosaic_member;', header, re.S).group(1)
    assert re.findall(r'(\w+)\s*[;,]', re.sub(r'/\*.*?\*/', '', old)) == [n for n, _ in MosaicMember._fields_]


# ---- the collections aim where they claim ----------------------------------------------------------------------------------
def test_cases_aim_where_they_claim():
    src = open(os.path.join(ROOT, 'auromat_amd', 'csrc', 'amt_mosaic_plan.h')).read()
    assert 'kSelTile' in open(os.path.join(ROOT, 'auromat_amd', 'csrc', 'amt_area.hip')).read()
    assert int(re.search(r'constexpr int kSelTile = (\d+);', src).group(1)) == MK.SEL_TILE
    cases = {c.name: c for c in MK.device_cases()}
    assert len(cases) == len(MK.device_cases())
    # member counts 1, 2, 3 and 65; sizes below a workgroup, a single pixel, no multiple of 256, several workgroups
    assert {1, 2, 3, 65} <= {len(c.members) for c in cases.values()}
    pixels = [m.height * m.width for m in cases['sizes'].members]
    assert 1 in pixels and any(p < K.BLOCK for p in pixels) and any(p > 2 * K.BLOCK and p % K.BLOCK for p in pixels)
    assert cases['many_65'].members[0].height * cases['many_65'].members[0].width == 1
    for c in cases.values():
        assert c.shape[0] <= 40 and c.shape[1] <= 48 and all(m.height * m.width <= 33 * 17 for m in c.members)
    # more than one select tile in both directions; an empty window between two others; overlaps across tile borders
    ny, nx = cases['three_with_empty'].shape
    assert nx > 2 * MK.SEL_TILE and ny > 2 * MK.SEL_TILE
    w = cases['three_with_empty'].windows
    assert w[1] == MK.EMPTY and w[0][2] and w[2][2]
    ox = (max(w[0][0], w[2][0]), min(w[0][0] + w[0][2], w[2][0] + w[2][2]))
    oy = (max(w[0][1], w[2][1]), min(w[0][1] + w[0][3], w[2][1] + w[2][3]))
    assert ox[0] // MK.SEL_TILE < (ox[1] - 1) // MK.SEL_TILE and oy[0] // MK.SEL_TILE < (oy[1] - 1) // MK.SEL_TILE
    lists = [sum(1 for x0, y0, wnx, wny in cases['many_65'].windows
                 if wnx and x0 < (tx + 1) * 16 and x0 + wnx > tx * 16 and y0 < (ty + 1) * 16 and y0 + wny > ty * 16)
             for tx in range(3) for ty in range(3)]
    assert max(lists) > 16 and len(set(lists)) > 3
    # the lane path with a clipped range on each of the four sides
    before, after, sides = MK.clipping(cases['clip_lane'].members[0], cases['clip_lane'].windows[0])
    for side in ('west', 'east', 'south', 'north'):
        assert (sides[side] & (before <= K.LANE_CELLS)).any(), side
    assert ((after == 0) & (before > 0)).any()
    # the wave path on a clipped range, and the switch from the wave path to the lane path by the cut
    before, after, sides = MK.clipping(cases['clip_wave'].members[0], cases['clip_wave'].windows[0])
    assert before[0] == 40 * 34 and after[0] == 30 * 20 and all(sides[s][0] for s in sides)
    before, after, _ = MK.clipping(cases['path_switch'].members[0], cases['path_switch'].windows[0])
    assert before[0] > K.LANE_CELLS and after[0] == 12
    # a quadrilateral inside the grid and wholly outside its window
    before, after, _ = MK.clipping(cases['outside_window'].members[0], cases['outside_window'].windows[0])
    assert after[0] > 0 and after[1] == 0 and before[1] > 0
    # formats
    fmts = {(c.dtype.name, c.nch) for c in cases.values()}
    assert fmts >= {(d, n) for d in ('uint8', 'uint16') for n in (0, 1, 3, 4)}
    assert any(m.width % 2 for m in cases['fmt_uint8_3'].members) and any(m.coord_offset == 1 for m in cases['fmt_uint8_3'].members)
    assert cases['lon_wrap'].lon_wrap == 1 and not cases['edge_arrays'].uniform
    assert cases['fmt_no_elev'].rules == (0,) and any(m.elev is None for m in cases['fmt_no_elev'].members)
    assert np.isnan(cases['fmt_nan_elev'].members[0].elev).sum() == 18 and cases['fmt_mask'].members[0].mask.sum() > 10
    # rule 1: the tie; a steeper member below the minimum that loses to a flatter one; cells that no member reaches
    tie = cases['tie']
    got = MA.mosaic(tie.members, tie.windows, 1)
    assert (got['source'][got['mask'] == 0] == 0).all() and (got['mask'] == 0).sum() > 50
    second = MA.mosaic(tie.members[::-1], tie.windows[::-1], 1)
    assert not np.array_equal(second['img'], got['img'])
    sl = cases['sliver']
    accs = [MA.member_accumulators(m, w) for m, w in zip(sl.members, sl.windows)]
    lay = lambda p: np.flipud(p.T)
    w0, w1 = lay(accs[0][0]), lay(accs[1][0])
    got = MA.mosaic(sl.members, sl.windows, 1)
    least = O.min_weight(0.5)
    lost = (w0 > 0) & (w0 < least) & (w1 >= least)
    assert lost.sum() >= 10 and (got['source'][lost] == 1).all()                  # 0.3 and 0.49 of a cell: the sliver loses
    assert ((w0 >= least) & (w1 >= least)).sum() >= 40 and (got['source'][(w0 >= least) & (w1 >= least)] == 0).all()
    nobody = (w0 < least) & (w1 < least) & ((w0 > 0) | (w1 > 0))
    assert nobody.sum() >= 10 and (got['source'][nobody] == -1).all() and (got['coverage'][nobody] > 0).all()
    assert got['coverage'][nobody].max() < 0.5 and np.isclose(np.median(got['coverage'][nobody]), 0.3) and ((w0 == 0) & (w1 == 0)).any()
    # overflow: every member below 2^40 and the total above; one member above; exactly at the limit
    for name, single, total in (('overflow_total', False, True), ('overflow_member', True, True), ('overflow_at_limit', False, False)):
        accs = [MA.member_accumulators(m, w) for m, w in zip(cases[name].members, cases[name].windows)]
        assert any((a[0] > O.LIMIT).any() for a in accs) == single and (sum(accs)[0] > O.LIMIT).any() == total
    assert sum(MA.member_accumulators(m, w) for m, w in zip(cases['overflow_at_limit'].members,
                                                             cases['overflow_at_limit'].windows))[0].max() == O.LIMIT
    # partitions: two and three parts by rows, two by columns, the shared corner row or column in both parts
    parts = MK.partition_cases()
    assert sorted(len(c.members) for _, c in parts) == [2, 2, 3]
    for whole, c in parts:
        a, b = c.members[0], c.members[1]
        if 'rows' in c.name:
            assert np.array_equal(a.lat[-1], b.lat[0]) and np.array_equal(a.lon[-1], b.lon[0], equal_nan=True)
        else:
            assert np.array_equal(a.lat[:, -1], b.lat[:, 0], equal_nan=True) and np.array_equal(a.lon[:, -1], b.lon[:, 0], equal_nan=True)
        assert all(w == (0, 0, whole.shape[1], whole.shape[0]) for w in c.windows)
