"""
CPU-only checks of tests/_fused_cases.py, the constructed grids of tests/test_gpu_fused_bin.py: the axis constructor reaches
every relation it claims; the Python statements of on_lower_edge_bits and of k_apply_bin_events agree with the reference's histogram
rule (_median_oracle.axis_index, pinned to histogram2d) on every window of an axis; every aimed centre lies where its case
says, by the mpmath reference of tests/_rowfield_oracle.py and with 1e-8 deg to spare on both sides (the row kernel is within
1e-10 deg of that reference, tests/test_gpu_rowfield.py: a device centre cannot change class); every class of grids is
populated on the float64 oracle's arrays, the stand-in for the device's; and the two places where a final grid differs from
its superset (its `scale`, the bits of its edges) are counted with the library's own host layout, amt_grid_layout.
"""
import os
import re

import numpy as np
import pytest

import _fused_cases as F
import _median_oracle as M
import _rowfield_cases as K
import _rowfield_oracle as R
from conftest import ROOT


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from auromat_amd import _native
    return _native.lib()


def test_constants_are_those_of_the_sources():
    def source(name):
        with open(os.path.join(ROOT, 'auromat_amd', 'csrc', name)) as fp:
            return fp.read()
    georef, pipe = source('amt_georef.hip'), source('amt_pipe.hip')
    assert int(re.search(r'constexpr int kBinW = (\d+)', georef).group(1)) == F.WINDOW
    assert 'bin_ax0 = __shfl(bin_x, src) - kBinW / 2' in georef
    assert float(re.search(r'constexpr double kMarginDeg = ([0-9.]+)', pipe).group(1)) == F.K_MARGIN_DEG
    assert (F.STRIP, F.CHUNK) == (63, 16)              # (tests/_rowfield_cases.py: frame sizes around one strip and one chunk)


# ---- the axis constructor -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', F.STEPS)
def test_axis_constructor_reaches_every_relation(step):
    rng = np.random.RandomState(3)
    reached = 0
    for v in rng.uniform(-180.0, 180.0, 40):
        for rel in F.RELATIONS:
            for pos in F.POSITIONS:
                for nbin in (4, 5, 37):
                    k = F.k_of(pos, nbin)
                    e = F.axis_for(v, k, nbin, step, rel)
                    assert e is not None, (v, rel, pos, nbin, step)
                    assert len(e) == nbin + 1 and F.relation(float(v), e, k) == rel
                    assert np.array_equal(e, np.linspace(e[0], e[-1], nbin + 1))        # what make_axis(uniform=True) accepts
                    reached += 1
    assert reached == 40 * 6 * 3 * 3


def test_axis_constructor_far_along_a_long_axis():
    """k of a few thousand on 60000 bins of 0.1: the relations that tolerate a rounding error are always reached, the exact
    ones where edge k can take every double next to v — |v| >= 128 with k = 2000: then neither k step nor the first edge lies
    in a higher binade than v"""
    rng = np.random.RandomState(5)
    exact = 0
    for v in np.concatenate((rng.uniform(-180.0, 180.0, 12), rng.uniform(130.0, 180.0, 6), rng.uniform(-180.0, -130.0, 6))):
        for rel in F.RELATIONS:
            e = F.axis_for(v, 3000, F.LARGE_NBIN, 0.1, rel)
            if rel in ('zone', 'near', 'inside'):
                assert e is not None and F.relation(float(v), e, 3000) == rel, (v, rel)
                continue
            if v >= 130.0:
                e = F.axis_for(v, 2000, F.LARGE_NBIN, 0.1, rel)
                assert e is not None and F.relation(float(v), e, 2000) == rel, (v, rel)
                assert np.array_equal(e, np.linspace(e[0], e[-1], F.LARGE_NBIN + 1))
                exact += 1
    assert exact >= 18


# ---- the event rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', F.STEPS)
def test_event_rule_equals_the_histogram_rule_on_every_window(step):
    """plain searchsorted(edges, v, 'right') bins plus on-edge flags, resolved by the rule of k_apply_bin_events, against
    _median_oracle.axis_index on the sub-axis taken as the final one: every window of a 9 x 6 grid that keeps its `decimal`"""
    rng = np.random.RandomState(17)
    xe, ye = np.linspace(-3.3, -3.3 + 9 * step, 10), np.linspace(48.7, 48.7 + 6 * step, 7)
    n = 3000
    x, y = rng.uniform(xe[0] - step, xe[-1] + step, n), rng.uniform(ye[0] - step, ye[-1] + step, n)
    unit_x, unit_y = 10.0 ** -F.decimal_of(xe), 10.0 ** -F.decimal_of(ye)
    for i in range(0, 1200, 2):                        # points on edges, an ulp beside them, inside and just outside the zone
        off = (0.0, 0.2, 0.45, 0.55, 1.2, -0.2)[(i // 2) % 6]
        x[i] = xe[rng.randint(len(xe))] + off * unit_x
        y[i + 1] = ye[rng.randint(len(ye))] + off * unit_y
    x[1200:1210] = np.nextafter(xe, np.inf)
    y[1210:1217] = np.nextafter(ye, -np.inf)
    x[1220:1230], y[1220:1227] = xe, ye
    x[1230:1237] = xe[3] + 0.1 * unit_x
    y[1230:1237] = ye + 0.1 * unit_y                   # on an x edge and a y edge at once
    h, w = 50, 60
    img = rng.randint(0, 65536, size=(h, w, 3)).astype(np.uint16)
    elev = rng.uniform(-80.0, 89.0, n)
    case = F.as_case('rule', x, y, elev, img, xe, ye, 10.0)
    acc, events = F.expected_with_events(case)
    _, _, flags = F.bins_and_flags(case)
    assert len(events) == int((flags > 0).sum()) >= 100 and {1, 2, 3} <= set(events['flags'].tolist())
    # the records carry plain searchsorted bins
    bx = np.searchsorted(xe, x, 'right')
    on = flags > 0
    assert sorted(events['bx'].tolist()) == sorted(bx[on].tolist())
    checked = 0
    for x0 in range(9):
        for nx in range(1, 10 - x0):
            if F.decimal_of(xe[x0:x0 + nx + 1]) != F.decimal_of(xe):
                continue
            for y0, ny in ((0, 6), (1, 4), (2, 1), (0, 3)):
                if F.decimal_of(ye[y0:y0 + ny + 1]) != F.decimal_of(ye):
                    continue
                window = (x0, y0, nx, ny)
                got = F.apply_events(acc, events, window)
                want = F.expected_planes(F.sub_case(case, window))
                assert np.array_equal(got, want), window
                checked += 1
    assert checked >= 40
    # without an event list: the grid as given
    assert np.array_equal(F.apply_events(acc, events, (0, 0, 9, 6)), F.expected_planes(case))


def test_on_edge_flags_are_the_rounding_rule():
    """bins_and_flags against a literal loop: a kept pixel of bin b is flagged when around(v, decimal) equals around(lower edge
    of b, decimal); beyond the last edge inside its zone the pixel is in the last bin (axis_index) and not flagged by it"""
    edges = np.linspace(10.0, 10.5, 5)
    dec = F.decimal_of(edges)
    v = np.array([10.125, 10.125 + 2e-7, 10.125 + 8e-7, 10.125 - 2e-7, 10.5 + 2e-7, 10.5 + 8e-7, 10.0, 9.9999999, 10.3])
    case = F.as_case('flags', v, np.full(len(v), 0.5), np.full(len(v), 20.0), np.zeros((1, len(v), 3), np.uint8), edges,
                     np.array([0.0, 1.0]), 10.0)
    bx, by, flags = F.bins_and_flags(case)
    assert dec == 6
    assert bx.tolist() == [2, 2, 2, 1, 4, 0, 1, 0, 3]
    assert flags.tolist() == [1, 1, 0, 0, 0, 0, 1, 0, 0]
    assert np.array_equal(np.where(bx > 0, bx, 0), np.where((M.axis_index(v, edges) <= 4), M.axis_index(v, edges), 0))


# ---- aimed fields -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', F.aimed_names())
def test_aimed_centres_lie_where_the_case_says(name, lib):
    c = F.aimed_case(name)
    mp = R._mp().mp
    P = R.params_of(c)
    w, h, ppd = c['width'], c['height'], c['ppd']
    f = R.float64_oracle(c['dirs'], P)
    # the frame's extremes did not move: the final grid is that of the base field, and no extreme is next to a grid node
    assert F.box_of(f, c['magnetic']) == c['box']
    assert min(abs(v * ppd - np.rint(v * ppd)) for v in c['box']) >= 1e-3
    g = F.final_grid(c['box'], ppd)
    assert np.array_equal(F.axis_edges(g.xaxis), c['xedges']) and np.array_equal(F.axis_edges(g.yaxis), c['yedges'])
    decimals = (F.decimal_of(c['xedges']), F.decimal_of(c['yedges']))
    seen = set()
    for a in c['aims']:
        r, q = a['pixel']
        assert 1 <= r <= h - 2 and 1 <= q <= w - 2                      # interior
        ref = R.reference_mp(c['dirs'], P, r, q)
        if c['magnetic']:
            vx, vy = (ref['mlt_c'] - 12) / (mp.mpf(24) / 360), ref['mlat_c']
        else:
            vx, vy = ref['lon_c'], ref['lat_c']
        for v, edges, k, dec in ((vx, c['xedges'], a['ix'], decimals[0]), (vy, c['yedges'], a['iy'], decimals[1])):
            if k is None:
                continue
            lo, hi = F.aim_zone(a['offset'], dec)
            d = v - mp.mpf(float(edges[k]))
            if name != F.FINER_CASE:                        # (its zones are those of two roundings: the test of its own, below)
                assert d - lo >= 1e-8 and hi - d >= 1e-8, (name, a, float(d), lo, hi)
            assert abs(float(d) - a['offset']) < 1e-10
        seen.add((a['axis'], 'last' if (a['ix'] in (None, len(c['xedges']) - 1) and a['iy'] in (None, len(c['yedges']) - 1)) else
                  'first' if a['ix'] == 0 else 'interior', a['offset']))
    if name in ('aimed-64x17', 'aimed-127x33'):
        for want in (('x', 'last'), ('y', 'last'), ('xy', 'last'), ('x', 'first'), ('x', 'interior'), ('y', 'interior')):
            assert want + (F.AIM_ON_EDGE,) in seen, (name, want)
        assert {('x', 'last', F.AIM_NEAR), ('x', 'last', F.AIM_BELOW), ('y', 'last', F.AIM_NEAR), ('y', 'last', F.AIM_BELOW)} <= seen
    if name == 'aimed-mag-64x17':
        assert {('y', 'last', F.AIM_ON_EDGE), ('y', 'last', F.AIM_NEAR)} <= seen
    if ppd == 8:
        # edges at 8 px/deg are odd multiples of 1/16: the same bits in the final grid and in its superset, decimal 6 in both
        s = F.superset_grid(c['box'], ppd)
        for fa, sa in ((g.xaxis, s.xaxis), (g.yaxis, s.yaxis)):
            fe, se = F.axis_edges(fa), F.axis_edges(sa)
            assert np.array_equal(fe * 16, np.rint(fe * 16)) and np.all(np.rint(fe * 16) % 2 == 1)
            assert set(fe.tolist()) <= set(se.tolist()) and fa.scale == sa.scale == 1e6


def test_three_frames_share_a_size_and_differ():
    cs = [F.aimed_case(n) for n in F.THREE_FRAMES]
    assert len({(c['width'], c['height']) for c in cs}) == 1
    assert len({c['box'] for c in cs}) == 3 and all(sum(a['offset'] == F.AIM_ON_EDGE for a in c['aims']) >= 3 for c in cs)


# ---- the classes of grids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('magnetic', [False, True], ids=['geodetic', 'magnetic'])
@pytest.mark.parametrize('name', F.FIELDS)
def test_every_class_of_grids_is_populated(name, magnetic):
    arrays = K.float64_oracle(name)
    gl = F.grids(name, arrays, magnetic=magnetic)
    c = F.census(name, arrays, gl)
    print(name, len(gl), 'grids', {k: c[k] for k in ('flags', 'outside', 'full_cell', 'largest_k')})
    F.assert_census(name, c)
    for g in gl:
        assert g['xedges'][0] < g['xedges'][-1] and len(g['xedges']) - 1 < 65535 and len(g['yedges']) - 1 < 65535
        assert 5 * (len(g['xedges']) - 1) * (len(g['yedges']) - 1) * 8 < 8 << 20          # accumulators of a few MB at the most
    assert {F.SIZES} and set(F.SIZES) == set(K.OWNERSHIP_SIZES) - {(1, 1)}
    assert {s[0] % 2 for s in F.SIZES} == {0, 1}           # widths of both parities: uint8 rows that are not 8-byte aligned


# ---- the two places where a final grid differs from its superset ---------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(F.SCALE_CASES))
def test_a_small_final_grid_rounds_coarser_than_its_superset(name, lib):
    """expected difference 1: at 10 px/deg an axis of the field's final grid has no edge difference below 0.1 and so decimal 6,
    its superset decimal 7 — on x, on y, on both.  On such an axis one pixel sits 2e-7 deg beyond the final grid's last edge:
    inside the final grid's rounding zone (the reference counts it into the last bin), outside the superset's; one 2e-8 deg
    beyond it: inside both; and one 2e-7 deg above the lower edge of the last cell, which stays where it is.  The superset's
    version of each of those edges is less than 1e-13 deg from the final grid's: every aimed pixel has the same relation to both."""
    c = F.aimed_case(name)
    which = F.SCALE_CASES[name]
    assert c['final_scale'] == (1e6 if 'x' in which else 1e7, 1e6 if 'y' in which else 1e7) and c['superset_scale'] == (1e7, 1e7)
    g, s, dx, dy = F.scales_differ(c['box'])
    assert (bool(dx), bool(dy)) == ('x' in which, 'y' in which) and g.nx <= 9 and g.ny <= 9
    seen = set()
    for a in c['aims']:
        for axis, k, edges, fa, sa, step in (('x', a['ix'], c['xedges'], g.xaxis, s.xaxis, s.lon_step),
                                            ('y', a['iy'], c['yedges'], g.yaxis, s.yaxis, abs(s.lat_step))):
            if k is None:
                continue
            e = float(edges[k])
            assert abs(F.twin_edge(fa, sa, k, step) - e) < 1e-13 < 1e-5 * a['offset']
            v = e + a['offset']
            assert np.around(v, 6) == np.around(e, 6)
            assert (np.around(v, 7) == np.around(e, 7)) == (a['offset'] == F.AIM_BOTH)
            if k == len(edges) - 1:
                assert M.axis_index(np.array([v]), edges)[0] == len(edges) - 1            # the reference: the last bin
            seen.add((axis, 'last' if k == len(edges) - 1 else 'before-last', a['offset']))
    for axis in which:
        assert {(axis, 'last', F.AIM_ON_EDGE), (axis, 'last', F.AIM_BOTH), (axis, 'before-last', F.AIM_ON_EDGE)} <= seen
    if which == 'xy':
        assert any(a['axis'] == 'xy' for a in c['aims'])


def test_a_superset_rounds_coarser_than_its_final_grid(lib):
    """the other way round (27 of 2605 frames of the benchmark's sequence): next to the prime meridian the superset's x axis has
    no edge difference below 0.1 (decimal 6), the final grid's has one (decimal 7).  A pixel 2e-7 deg beyond the final grid's last
    edge is on-edge under the superset's rounding alone — the reference drops it —, one 2e-8 deg beyond it under both"""
    c = F.aimed_case(F.FINER_CASE)
    g, s, dx, dy = F.scales_differ(c['box'])
    assert (g.xaxis.scale, g.yaxis.scale, s.xaxis.scale, s.yaxis.scale) == (1e7, 1e7, 1e6, 1e7)
    last, nx = float(c['xedges'][-1]), g.nx
    offsets = sorted(a['offset'] for a in c['aims'] if a['ix'] == nx)
    assert offsets == [F.AIM_BOTH, F.AIM_ON_EDGE] and any(a['ix'] == nx - 1 for a in c['aims'])
    for off, kept in ((F.AIM_ON_EDGE, False), (F.AIM_BOTH, True)):
        v = last + off
        assert np.around(v, 6) == np.around(last, 6) and (np.around(v, 7) == np.around(last, 7)) == kept
        assert M.axis_index(np.array([v]), c['xedges'])[0] == (nx if kept else nx + 1)
        assert abs(F.twin_edge(g.xaxis, s.xaxis, nx, s.lon_step) - last) < 1e-13 < 1e-5 * off


def band_of(box, ppd):
    """first edge index of the band of each superset axis, as pipe_prepare_rest lays it out for an estimate `box`"""
    s = F.superset_grid(box, ppd)
    lat_abs = max(abs(box[0]), abs(box[1]))
    lon_margin = min(10.0, F.K_MARGIN_DEG / max(0.1, np.cos(np.deg2rad(lat_abs))))
    return s, max(0, s.nx - int(np.ceil(2 * lon_margin * ppd)) - 4), max(0, s.ny - int(np.ceil(2 * F.K_MARGIN_DEG * ppd)) - 4)


def test_the_band_holds_the_last_edge_of_the_final_grid(lib):
    """The band (twice the margin plus four cells from the superset's end; the formula is read from amt_pipe.hip) holds the
    final grid's last edge on both axes whenever the final grid fits its superset — for estimates off by up to 0.9 of the
    margin either way — and starts above the first half of the superset of a frame-sized box: interior edges of the final
    grid stay outside it.  An estimate three degrees too large puts the final grid's end below the band."""
    with open(os.path.join(ROOT, 'auromat_amd', 'csrc', 'amt_pipe.hip')) as fp:
        text = fp.read()
    assert 'pipe->band_x = std::max(0, pipe->super.nx - (int)std::ceil(2 * lon_margin_used * lon_px_per_deg) - 4);' in text
    assert 'pipe->band_y = std::max(0, pipe->super.ny - (int)std::ceil(2 * kMarginDeg * lat_px_per_deg) - 4);' in text
    assert 'off_x + g.nx < pipe->band_x' in text and 'off_y + g.ny < pipe->band_y' in text
    rng = np.random.RandomState(29)
    fitted = 0
    for ppd in (8, 10, 40):
        for _ in range(300):
            lat, lon = rng.uniform(-60, 60), rng.uniform(-140, 140)
            box = (lat, lat + rng.uniform(0.3, 12), lon, lon + rng.uniform(0.3, 25))
            err = rng.uniform(-0.9, 0.9, 4) * F.K_MARGIN_DEG
            est = (box[0] + err[0], box[1] + err[1], box[2] + err[2], box[3] + err[3])
            g = F.final_grid(box, ppd)
            s, band_x, band_y = band_of(est, ppd)
            off_x = int(round((g.lon_center_first - s.lon_center_first) / s.lon_step))
            off_y = int(round((g.lat_center_last - s.lat_center_last) / abs(s.lat_step)))
            if off_x < 0 or off_y < 0 or off_x + g.nx > s.nx or off_y + g.ny > s.ny:
                continue                                   # (the final grid does not fit: handed back for that reason)
            fitted += 1
            assert band_x <= off_x + g.nx <= s.nx and band_y <= off_y + g.ny <= s.ny, (ppd, box, est)
            if box[1] - box[0] > 6 and box[3] - box[2] > 8:
                assert band_x > s.nx // 2 and band_y > s.ny // 2
    assert fitted >= 700
    c = F.aimed_case('aimed-scale')
    box = c['box']
    g = F.final_grid(box, 10)
    s, band_x, band_y = band_of(poor_estimate(box), 10)
    off_x = int(round((g.lon_center_first - s.lon_center_first) / s.lon_step))
    assert 0 <= off_x and off_x + g.nx < band_x


def poor_estimate(box):
    return (box[0], box[1] + 3.0, box[2], box[3] + 3.0)


def test_count_of_differing_scales_and_edge_bits(lib):
    """expected differences 1 and 2, counted over random boxes (the figures of DESIGN.md come from 3000 boxes per resolution):
    at 8 px/deg no scale and no edge differs; at 10 px/deg scales differ only for small final grids, and a good part of the
    final edges differ in their last bit from the superset's edge at the same node"""
    edges, differ, scales, n = F.edge_bit_differences(8, 150)
    assert (differ, scales) == (0, 0) and edges > 1000
    edges, differ, scales, n = F.edge_bit_differences(10, 150)
    print('10 px/deg: %d of %d final edges differ in bits from their superset twin, %d of %d layouts differ in scale'
          % (differ, edges, scales, n))
    assert differ > 0
    small = 0
    rng = np.random.RandomState(23)
    for _ in range(300):                               # final grids of at most 9 cells per axis
        lat, lon = rng.uniform(-60, 60), rng.uniform(-150, 150)
        box = (lat, lat + rng.uniform(0.25, 0.85), lon, lon + rng.uniform(0.25, 0.85))
        g, s, dx, dy = F.scales_differ(box)
        assert g.nx <= 10 and g.ny <= 10
        small += int(dx or dy)
    print('10 px/deg: %d of 300 layouts of at most 10 cells per axis differ in scale from their superset' % small)
    assert small > 0
