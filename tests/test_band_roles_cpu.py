"""
The host rule behind the roles of the frame kernel's work items (amt_prm::band_roles in csrc/amt_params.h, reached through
amt_georef_band_roles; no GPU): which rows of work items ("bands") are inner — every corner ray and every centre hits the
shell and every pixel lies at or above the elevation threshold — and which are low — no pixel reaches the threshold.

Soundness has no exceptions: the oracle (oracle.ref_numpy.georef_frame, every corner and every pixel) shows no NaN corner, no
NaN centre and no elevation below the threshold in a band the rule calls inner, and no pixel at or above the threshold in a
band it calls low.  Tightness is reported per case (bands left generic that the oracle would allow) and bounded on the
benchmark's frames: at each boundary of a range the rule stays within kSlackBands bands of the oracle, the number
tests/test_sky_rows.py holds amt_georef_image_rows to ("at most three bands of 16 rows more than needed on either side").
"""
import numpy as np
import pytest

from _band_role_cases import ROWS, band_roles, cases, oracle_bands, role_of_bands

kSlackBands = 3
THRESHOLDS = (0.0, 10.0, -np.inf)          # min_elevation 0, 10 and none
SHELLS = (100, 110, 120)


def check_sound(name, roles, oracle):
    may_inner, may_low, hit = oracle
    kinds = role_of_bands(roles)
    n, (t, b), (lt, lb), (i0, i1) = roles['n'], roles['sky'], roles['low'], roles['inner']
    assert len(kinds) == n == len(may_inner)
    assert 0 <= t <= b <= n and t <= lt <= lb <= b, (name, roles)
    assert (i0, i1) == (0, 0) or lt <= i0 < i1 <= lb, (name, roles)
    for c, k in enumerate(kinds):
        if k == 'i':
            assert may_inner[c], (name, 'band %d is called inner' % c, kinds)
        elif k == 'l':
            assert may_low[c], (name, 'band %d is called low' % c, kinds)
        elif k == 's':
            assert not hit[c], (name, 'band %d is called sky' % c, kinds)
    return kinds


@pytest.mark.parametrize('case', cases(), ids=lambda c: c[0])
def test_roles_are_sound(case):
    name, w, h, hdr, cam, t = case
    report = []
    seen = set()
    for altitude in SHELLS:
        for fast in (True, False):
            for thr in THRESHOLDS:
                roles = band_roles(hdr, cam, t, thr, altitude, fast)
                assert roles['n'] == (h + ROWS - 1) // ROWS and roles['strips'] == (w + 1 + 62) // 63
                oracle = oracle_bands(hdr, cam, t, thr, altitude, fast)
                kinds = check_sound((name, altitude, fast, thr), roles, oracle)
                seen.update(kinds)
                may_inner, may_low, hit = oracle
                lost_inner = sum(1 for c, k in enumerate(kinds) if k == 'g' and may_inner[c])
                lost_low = sum(1 for c, k in enumerate(kinds) if k == 'g' and may_low[c] and hit[c])
                report.append('%s shell %d %s thr %5s: %s  generic but inner in the oracle: %d, low: %d'
                              % (name, altitude, 'fast ' if fast else 'exact', thr, kinds, lost_inner, lost_low))
    print('\n'.join(report))
    # what each view is there for
    if name.startswith('nadir'):
        assert seen == {'i'}, seen
    if name.startswith('sky'):
        # (the sky rule names no band in a frame too coarse for it: generic bands then, never a role)
        assert seen == {'s'} if h == 120 else seen <= {'s', 'g'}, seen
    if name.startswith('limb across'):
        assert {'i', 'g'} <= seen, seen         # (a frame this small may be too coarse for the sky rule to name sky bands)


def test_thresholds_that_decide_nothing():
    name, w, h, hdr, cam, t = cases()[0]
    assert role_of_bands(band_roles(hdr, cam, t, np.nan)) == 'g' * ((h + ROWS - 1) // ROWS)
    # a threshold no pixel reaches: nothing is inner; below it everything may be low
    kinds = role_of_bands(band_roles(hdr, cam, t, 89.99))
    assert 'i' not in kinds


def ranges(flags):
    """(first, last + 1) of the true entries of a boolean array, or None"""
    idx = np.flatnonzero(flags)
    return (int(idx[0]), int(idx[-1]) + 1) if idx.size else None


@pytest.mark.parametrize('k', [0, 100, 196])
def test_roles_of_the_bench_frames_are_tight(k):
    from auromat_amd.synthetic import sequence_frame
    hdr, cam, t, _ = sequence_frame(k, 4240, 2832)
    roles = band_roles(hdr, cam, t, 10.0)
    oracle = oracle_bands(hdr, cam, t, 10.0)
    kinds = check_sound(('bench', k), roles, oracle)
    may_inner, may_low, hit = oracle
    n, (st, sb), (lt, lb), (i0, i1) = roles['n'], roles['sky'], roles['low'], roles['inner']
    print('bench frame %d: %s' % (k, kinds))
    print('bench frame %d: bands sky %d, low %d, generic %d, inner %d; the oracle allows inner %d, low %d'
          % (k, kinds.count('s'), kinds.count('l'), kinds.count('g'), kinds.count('i'), int(may_inner.sum()), int((may_low & hit).sum())))
    want_inner = ranges(may_inner)
    assert want_inner is not None and i0 < i1
    assert i0 <= want_inner[0] + kSlackBands and i1 >= want_inner[1] - kSlackBands, (roles, want_inner)
    # low bands: the Earth bands above the first band with a pixel at or above the threshold (the Earth fills the bottom of these frames)
    first_pass = int(np.flatnonzero(~may_low)[0])
    assert lt >= first_pass - kSlackBands and lb == sb == n, (roles, first_pass)
