"""
Roles of the frame kernel's work items (amt_prm::band_roles) on the cameras of tests/_band_role_sweep.py: the line of
the threshold and the limb within the host rule's margins of a band boundary, other orbits, shells, plate scales, camera models
and frame sizes.  tests/test_band_role_sweep_cpu.py checks without a GPU that the cases hold what they claim and that the rule
is sound on them.

For every camera, at the thresholds 0, 4.99, 5, 10, 30 and none, with fast and exact centres, the variants SECOND 0 | 1 | 4 x BIN
0 | 1 | 2 and contiguous and strip-padded rows (launch_frame / assert_same / last_roles of tests/_band_role_cases.py, which
tests/test_gpu_band_roles.py uses too):
  * the launch with roles equals the forced-generic launch (amt_georef_set_roles(ctx, 0)) BIT FOR BIT in every array, the box,
    the count of valid pixels, the accumulator planes and the on-edge records;
  * the work items per role are the host rule's (amt_georef_last_roles against amt_georef_band_roles); a forced-generic launch
    takes none; across the sweep every variant takes inner items and every binning variant low items.
Then the launches with roles against the longdouble / mpmath reference of tests/_camera_oracle.py: every element with identical
NaN patterns within 8 max(E_ref, eps scale) and its floor (_rowfield_oracle.bound), E_ref the distance of the float64 oracle from
the same reference on the same case; amt_georef_out.bbox and the valid count against
_camera_oracle.kernel_box per threshold; and the fused counts, channel sums, fixed-point elevation sums and on-edge records
against tests/_bin_oracle.py on the device's own centre arrays (tests/_fused_cases.expected_with_events), which catches a pixel
that an inner band wrongly bins or a low band wrongly drops.

Measured on the MI355X: 1196 tests in 152 s, the slowest 3.3 s; every comparison passed and no fault was found in the library.

Mutation check (scratch copies of the tree, never committed)
  `valid` of the inner loop applied in a low band (ROLE == kRoleLow ? px_ok)     6 of 6 test_low_band_pixel_on_a_grid_edge fail (a
      record for a pixel below the threshold); 144 other tests of this module, sampled (aimed-thr10-roll0, aimed-limb-roll45,
      scales, sizes-a), pass: bin_account is not reached in a low band, so only an on-edge pixel shows the mutant
The eight mutants of the host rule were run against tests/test_band_role_sweep_cpu.py alone (its docstring has the counts); a host
rule that this module would catch and that one not does not exist, since both hold the same roles to the same reference.
"""
import numpy as np
import pytest

import _band_role_sweep as S
import _camera_cases as K
import _camera_oracle as Q
import _fused_cases as F
from _band_role_cases import CORNERS, assert_same, launch_frame, role_of_bands
from test_gpu_camera_rows import check_box

pytestmark = pytest.mark.gpu

BIN_ID = {None: 0, np.uint8: 1, np.uint16: 2}
VARIANTS = [(fast, second, b) for fast in (True, False) for second in (0, 1, 4) for b in (None, np.uint8, np.uint16)]


def groups():
    """(group, family, names of its cameras — the fast cases; 'exact-' + name is the same camera with exact centres): at most
    a dozen cameras each, so that a test takes a few seconds"""
    fast = S.names(None, True)
    out = []
    for thr in S.AIMED_THRESHOLDS:
        for roll in S.ROLLS:
            head = 'thr%g-roll%d' % (thr, roll)
            out.append(('aimed-' + head, 'aimed-threshold', [n for n in fast if n[:-4] == head]))
    for roll in S.ROLLS:
        out.append(('aimed-limb-roll%d' % roll, 'aimed-limb', [n for n in fast if n[:-4] == 'limb-roll%d' % roll]))
    for tag in ('shell0', 'shell110', 'shell1000'):
        out.append(('orbits-' + tag, 'orbits', [n for n in fast if n.startswith('orbit-') and n.endswith(tag)]))
    out.append(('orbits-flat', 'orbits', [n for n in fast if n.startswith('flat-')]))
    for fam in ('scales', 'model', 'nothing'):
        out.append((fam, fam, S.names(fam, True)))
    sizes = S.names('sizes', True)
    out.append(('sizes-a', 'sizes', sizes[:14]))
    out.append(('sizes-b', 'sizes', sizes[14:]))
    assert sorted(n for g in out for n in g[2]) == sorted(fast) and all(g[2] for g in out)
    return out


GROUPS = groups()
AIMED = tuple(g[0] for g in GROUPS if g[1].startswith('aimed'))          # (every group of these bins pixels)
_GRIDS, _HOST_IMAGES, _LAST = {}, {}, []


def case_of(name, fast):
    return S.by_name(name if fast else 'exact-' + name)


def launch(name, fast, second, bin_dtype, padded, roles, thr, edges=None):
    c = case_of(name, fast)
    return launch_frame(c['width'], c['height'], K.native_params(c), second, bin_dtype, padded, roles, edges, thr)


def floats(run):
    return {k: v.view(np.float64) for k, v in run['arrays'].items()}


def grid_edges(name, fast, second):
    """Uniform edges around the frame's centre coordinates, quarter degrees on round numbers (at most 400 cells an axis)"""
    key = (name, fast, second)
    if key not in _GRIDS:
        a = floats(launch(name, fast, second, None, False, False, S.NONE))
        x, y = F.binned_xy(a, magnetic=second == 4)
        if np.isnan(x).all():
            _GRIDS[key] = (np.linspace(-10.0, 10.0, 41), np.linspace(-10.0, 10.0, 41))
        else:
            def edges(v):
                lo, hi = np.floor(np.nanmin(v)) - 1.0, np.ceil(np.nanmax(v)) + 1.0
                per_deg = 4 if hi - lo <= 100.0 else 1
                return np.linspace(lo, hi, int(round((hi - lo) * per_deg)) + 1)
            _GRIDS[key] = (edges(x), edges(y))
    return _GRIDS[key]


def host_image(w, h, dtype):
    if (w, h, dtype) not in _HOST_IMAGES:
        from auromat_amd.synthetic import frame_image
        _HOST_IMAGES[(w, h, dtype)] = np.ascontiguousarray(frame_image(w, h, seed=7, dtype=dtype))      # what _band_role_cases.image uploads
    return _HOST_IMAGES[(w, h, dtype)]


def expected_items(c, thr, binning):
    """(generic, inner, low) work items by the host rule (low rows exist with fused binning only)"""
    r = S.band_roles(c, thr)
    kinds = role_of_bands(r)
    inner, low = kinds.count('i'), kinds.count('l') if binning else 0
    earth = r['n'] - kinds.count('s')
    return tuple(int(v) * r['strips'] for v in (earth - inner - low, inner, low))


def check_arrays(c, run, second):
    """every element of a launch against the reference"""
    name = c['name']
    ref, got = S.reference(name), floats(run)
    bounds = S.bounds(name)
    failed = []
    for k in got:
        assert got[k].shape == ref[k].shape, (name, k)
        mism = np.argwhere(np.isnan(got[k]) != np.isnan(ref[k]))
        assert len(mism) == 0, '%s %s: NaN pattern differs at %s' % (name, k, mism[:6].tolist())
        d = Q.distance(k, got, ref)
        worst = float(d.max())
        if not worst <= bounds[k]:
            failed.append((k, worst, bounds[k], np.unravel_index(int(d.argmax()), d.shape)))
    assert not failed, (name, second, failed)


def check_bins(c, run, second, bin_dtype, thr, edges):
    """accumulators and on-edge records against _bin_oracle on the launch's own centre arrays"""
    a = floats(run)
    h, w = c['height'], c['width']
    x, y = F.binned_xy(a, magnetic=second == 4)
    keep = None
    if not c['fast_center']:                                     # exact centres: a pixel counts when its four corners hit
        hit = ~np.isnan(a['mlat' if second == 4 else 'lat'])
        keep = hit[:-1, :-1] & hit[:-1, 1:] & hit[1:, 1:] & hit[1:, :-1]
    case = F.as_case(c['name'], x, y, a['elev'], host_image(w, h, bin_dtype), edges[0], edges[1], thr, keep)
    want_acc, want_ev = F.expected_with_events(case)
    nx, ny = len(edges[0]) - 1, len(edges[1]) - 1
    got_ev = F.sorted_events(run['records'].view(F.EVENT_DTYPE))
    assert run['count'] == len(want_ev) and np.array_equal(got_ev, want_ev), (c['name'], thr, 'on-edge records', run['count'], len(want_ev))
    got = run['acc'].reshape(5, nx, ny)
    for k, plane in enumerate(('count', 'sum 0', 'sum 1', 'sum 2', 'fx')):
        bad = np.argwhere(got[k] != want_acc[k])
        assert len(bad) == 0, '%s thr %s: plane %s differs in %d cells, first (cx, cy) %s: got %d, want %d' % (
            c['name'], thr, plane, len(bad), bad[0].tolist(), got[k][tuple(bad[0])], want_acc[k][tuple(bad[0])])
    return int(want_acc[0].sum())


PARAMS = [(g, v, p) for g in GROUPS for v in VARIANTS for p in (False, True)]


@pytest.mark.parametrize('group,variant,padded', PARAMS,
                         ids=['%s-%s-second%d-bin%d-%s' % (g[0], 'fast' if v[0] else 'exact', v[1], BIN_ID[v[2]], 'padded' if p else 'contiguous')
                              for g, v, p in PARAMS])
def test_roles_leave_every_bit_and_match_the_reference(group, variant, padded):
    gname, fam, names = group
    fast, second, bin_dtype = variant
    if _LAST and _LAST[0][0] != gname:                           # (the references of the sweep would be a GB: those of one group are kept)
        S.forget(_LAST.pop()[1])
    if not _LAST:
        _LAST.append((gname, names))
    took = np.zeros(3, np.int64)
    binned = 0
    for name in names:
        c = case_of(name, fast)
        edges = grid_edges(name, fast, second) if bin_dtype is not None else None
        for n_thr, thr in enumerate(S.GPU_THRESHOLDS):
            off = launch(name, fast, second, bin_dtype, padded, False, thr, edges)
            on = launch(name, fast, second, bin_dtype, padded, True, thr, edges)
            tag = (c['name'], thr, variant, padded)
            assert on['variant'][:2] == (second, BIN_ID[bin_dtype]), tag
            assert off['roles'][1:] == (0, 0), (tag, off['roles'])
            assert on['roles'] == expected_items(c, thr, bin_dtype is not None), (tag, on['roles'])
            assert sum(on['roles']) == sum(off['roles'])
            assert_same(tag, on, off)
            took += on['roles']
            # ---- against the reference (the arrays do not depend on the threshold: once per camera)
            if n_thr == 0 and bin_dtype is None:
                check_arrays(c, on, second)
            if bin_dtype is None and not padded:
                slots, lats, count = Q.kernel_box(c, S.reference(c['name']), thr, magnetic=second == 4)
                box = on['bbox'].view(np.float64)
                assert box[6] == count, (tag, box[6], count)
                b = S.bounds(c['name'])
                check_box(tag, box, slots, lats, dict(lat=b['mlat'], lon=b['mlt']) if second == 4 else b)
            if bin_dtype is not None:
                binned += check_bins(c, on, second, bin_dtype, thr, edges)
    print(gname, variant, padded, 'work items generic / inner / low:', took.tolist(), 'pixels binned', binned)
    if bin_dtype is not None and gname in AIMED:
        assert binned > 0


def test_every_variant_takes_inner_and_low_items():
    """Across the sweep every variant takes inner items and every binning variant low items.  The test above holds every launch
    to the host rule's items per role, so the sums are taken on the host rule: per centre mode, with and without binning."""
    for fast in (True, False):
        for binning in (False, True):
            took = np.zeros(3, np.int64)
            for name in S.names(None, True):
                for thr in S.GPU_THRESHOLDS:
                    took += expected_items(case_of(name, fast), thr, binning)
            print('fast' if fast else 'exact', 'binning' if binning else 'plain', 'work items generic / inner / low:', took.tolist())
            assert took[0] > 0 and took[1] > 0 and (took[2] > 0) == binning, took


@pytest.mark.parametrize('fast', [True, False], ids=['fast', 'exact'])
@pytest.mark.parametrize('name', ['thr10-roll0-2.5', 'thr10-roll180-2.5', 'limb-roll0+0.5'])
def test_low_band_pixel_on_a_grid_edge(name, fast):
    """A pixel of a low band ON an x edge of the grid (bit for bit, _fused_cases.axis_for): below the threshold it leaves no
    on-edge record — the low loop's `valid` is false —, while without a threshold the same pixel is recorded."""
    thr = 10.0
    c = case_of(name, fast)
    kinds = role_of_bands(S.band_roles(c, thr))
    assert 'l' in kinds, kinds
    a = floats(launch(name, fast, 0, None, False, False, thr))
    rows = [r for r in range(c['height']) if kinds[r // S.ROWS] == 'l']
    at = [(r, q) for r in rows for q in range(c['width']) if not np.isnan(a['lat_c'][r, q]) and a['elev'][r, q] < thr]
    assert at, 'no pixel of the low band hits'
    r, q = at[len(at) // 2]
    x, y = float(a['lon_c'][r, q]), float(a['lat_c'][r, q])
    xe = F.axis_for(x, 32, 64, 0.125, 'eq')
    assert xe is not None and F.relation(x, xe, 32) == 'eq'
    edges = (xe, np.linspace(np.floor(y) - 4.0, np.floor(y) + 4.0, 65))
    for bin_dtype in (np.uint8, np.uint16):
        off = launch(name, fast, 0, bin_dtype, False, False, thr, edges)
        on = launch(name, fast, 0, bin_dtype, False, True, thr, edges)
        assert on['roles'][2] > 0 and off['roles'][2] == 0
        assert_same((c['name'], 'pixel', r, q, 'on an edge'), on, off)
        check_bins(c, on, 0, bin_dtype, thr, edges)
        free = launch(name, fast, 0, bin_dtype, False, True, S.NONE, edges)
        check_bins(c, free, 0, bin_dtype, S.NONE, edges)
        mine = [e for e in free['records'].view(F.EVENT_DTYPE) if e['el'] == np.rint(a['elev'][r, q] * 2.0 ** 32)]
        assert free['count'] > on['count'] and len(mine) >= 1, (free['count'], on['count'])


def test_corner_arrays_are_the_corner_arrays():
    """(the names this module takes corners from are those launch_frame sizes as corner arrays)"""
    assert set(CORNERS) == set(Q.CORNER_ARRAYS)
