"""
The host rule of the band roles (amt_georef_band_roles: inner_bands, elevation_bands(tight), sky_bands and amt_prm::band_roles; no
GPU) on the cameras of tests/_band_role_sweep.py, which put the line of the threshold and the limb within the rule's own margins
of a band boundary, and vary orbit, shell, plate scale, camera model and frame size.

The cases hold what they claim, on the longdouble / mpmath reference of tests/_camera_oracle.py: the aimed line lies within
0.25 px of its target (the ray a quarter pixel to either side of the target is on its own side of the line, and so are the
frame's own pixel centres next to it on the probe), no ray has |relative discriminant| below _camera_cases.r_min(), no pixel's
elevation lies within 1e-9 deg of a threshold it is tested at.

Soundness, for every case x threshold and without exception: in a band the rule calls inner every corner and every centre of the
reference hits and every pixel lies at or above the threshold; in a low band no pixel reaches it; in a sky band nothing hits; and
the same against the float64 oracle (test_band_roles_cpu.check_sound).  Centres are the kernel's: the mean of four corner hits
(fast) or the pixel's own ray (exact).  Thresholds: none, 0, 4.99, 5, 10, 30, 60 for every case, -0.0 for the limb family, NaN,
+inf, 90, 89.99, 89 and -5 for the family `nothing`.

Not vacuous: each aimed family yields inner, low and generic bands, and on the safe side of an aimed line the rule's range ends
within kSlackBands = 3 bands of the reference's.  The pure rule amt_prm::band_roles / band_role_counts runs in a stand-alone C++
program (tests/csrc/band_roles_check.cpp; host compiler, sanitizers where they link, nothing loaded into this process).

Observed slack of the hand-picked margins (printed with -s by test_report_per_family; elevations in degrees):
(per family and centre mode: the smallest elevation minus threshold — minus 0 where there is none — in an inner band, the largest
elevation minus threshold in a low band, each with its case and threshold, and the bands left generic that the reference would
allow, of all band x threshold pairs)
  aimed-threshold  fast   inner +0.3082 (thr60-roll45+1.5 at 60)  low -0.2678 (thr60-roll90+3.5 at 60)  generic of 8960: 147 inner, 503 low
  aimed-threshold  exact  inner +0.3082 (the same)                low -0.2678 (the same)                generic of 8960: 147 inner, 481 low
  aimed-limb       fast   inner +1.0858 (limb-roll0-3.5 at 5)     low -1.5771 (limb-roll45-3.5 at 10)   generic of 2048: 48 inner, 138 low
  aimed-limb       exact  inner +1.0862 (the same)                low -1.5769 (the same)                generic of 2048: 48 inner, 129 low
  orbits           fast   inner +0.9135 (orbit-+5-shell1000 at 10) low -0.7686 (orbit-+5-shell1000 at 10) generic of 770: 64 inner, 13 low
  orbits           exact  inner +0.9135 (the same)                low -0.7686 (the same)                generic of 770: 64 inner, 13 low
  scales           fast   inner +0.5942 (scale-0.01+2.5 at 10)    low -1.6268 (scale-0.05-1.5 at 10)    generic of 595: 24 inner, 65 low
  scales           exact  inner +0.5942 (the same)                low -1.6266 (the same)                generic of 595: 24 inner, 65 low
  model            fast   inner +0.6813 (model-flipped+2.5 at 10) low -1.1597 (model-crpix-outside+2.5 at 10) generic of 280: 6 inner, 6 low
  model            exact  inner +0.6814 (the same)                low -1.1596 (the same)                generic of 280: 6 inner, 6 low
  sizes            fast   inner +1.4917 (size-127x48-2.5 at 5)    low -1.5051 (size-62x50-2.5 at 10)    generic of 420: 26 inner, 20 low
  sizes            exact  inner +1.4921 (the same)                low -1.5049 (the same)                generic of 420: 26 inner, 20 low
  nothing          fast   inner +5.4350 (nothing-limb at none)    low -4.3627 (nothing-limb at 10)      generic of 195: 5 inner, 63 low
  nothing          exact  inner +5.4357 (the same)                low -4.3622 (the same)                generic of 195: 5 inner, 63 low
At an aimed line the rule ends at most one band (inner) and two bands (low) short of the reference.
No fault was found in the library.

Mutation check (scratch copies of the tree, never committed; failing tests of this module, 547 tests; the host rule only)
  r_min <-> r_max in inner_bands                 224   (6 of tests/test_band_roles_cpu.py too)
  r_min <-> r_max in elevation_bands              32   (lines along the columns, the flattened shell)
  `uo < 0` dropped in inner_bands                  3   (nothing-zenith, its exact twin and the family's test)
  inner margin 2 px -> 0                           0   the band's own corner rows and columns hold every corner and every exact centre
                                                       ray; a fast centre's second-order offset is covered by the 0.05 deg of e0 (polar
                                                       cameras at 0.45 and 1 deg / px, tried on scratch cameras, stayed sound)
  e0 margin 0.05 deg -> 0                          0   with the 2 px kept every ray of a band is strictly inside the cone of r_min at the
                                                       threshold itself: the law of sines needs no margin
  tight widening 3 px -> 1 px                      0   1 px is what amt_georef_image_rows has; inside the gate (<= 0.5 deg / px) a fast
                                                       centre's offset is a few per cent of a pixel from 5 deg on
  extra band dropped below 5 deg                   0   differs at thresholds in (0, 5) only: at 4.99 and, on scratch cameras at 0.2 and
                                                       0.45 deg / px, at 0.25, 0.5, 1 and 2 deg the margin in pixels alone stayed sound
  5 deg switch ignored                             0   the same thresholds and cameras
The five survivors are margins stacked on margins; each is covered by the others on every camera tried.  The kernel mutant
(`valid` of the inner loop in a low band) is in tests/test_gpu_band_role_sweep.py.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _band_role_sweep as S
import _camera_cases as K
import _camera_oracle as Q
from _band_role_cases import role_of_bands
from test_band_roles_cpu import check_sound, kSlackBands, ranges

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'auromat_amd', 'csrc')
_LD = Q._LD
_SUMMARY = {}


def thr_tag(t):
    return 'none' if t == S.NONE else repr(float(t))


def check_aim(c, ref):
    """the line is where the case says, by the reference: rays a quarter pixel from the target, then the case's own centres"""
    cl = c['claims']
    if 'target' not in cl:
        return
    kind, fixed = S.probe_of(c)
    target, up, thr = cl['target'], cl['above_grows'], cl['line']
    for side in (-1.0, 1.0):
        s = np.array([target + 0.25 * side - 0.5])               # corner coordinate -> pixel coordinate
        f = np.array([float(fixed)])
        got = bool((S.above(_LD, c, f, s, thr) if kind == 'column' else S.above(_LD, c, s, f, thr))[0])
        assert got == (up if side > 0 else not up), (c['name'], 'the line is not within 0.25 px of', target, side)
    # the frame's own centres on the probe, up to 8 pixels to either side of the line: a pixel whose centre (corner coordinate
    # r + 1/2) lies more than 0.25 px beyond the target is on that side — an exact centre is that ray; a fast centre differs
    # from it in the second order of the pixel's size, which is why frames of 0.45 deg / px and more are left to the rays above
    if c['scale'] > 0.3:
        return
    elev = np.asarray(ref['elev'], dtype=np.float64)
    line = elev[:, fixed] if kind == 'column' else elev[fixed, :]
    with np.errstate(invalid='ignore'):
        is_above = ~np.isnan(line) if thr is None else (line >= thr)
    # (a fast centre next to the limb exists only when its four corners hit: its farthest corner lies up to 1 px nearer to an
    # oblique limb along the probe)
    nearest = 1.25 if thr is None and c['fast_center'] else 0.25
    for r in range(len(line)):
        off = r + 0.5 - target
        if nearest < abs(off) <= 8.0:
            assert bool(is_above[r]) == (up if off > 0 else not up), (c['name'], 'pixel', r, 'of the probe', float(line[r]), target)


def summarize(name):
    """every per-case check; -> {threshold tag: dict(kinds, inner margin, low margin, lost inner, lost low, reference ranges)}"""
    if name in _SUMMARY:
        return _SUMMARY[name]
    c = S.by_name(name)
    ref = Q.reference(c)
    f64 = S.float64_oracle(c)
    check_aim(c, ref)
    with np.errstate(invalid='ignore'):
        rel = [np.abs(np.asarray(ref['rel'], dtype=np.float64))] + ([] if c['fast_center'] else [np.abs(np.asarray(ref['rel_c'], dtype=np.float64))])
        assert min(float(np.nanmin(r)) for r in rel) >= K.r_min(), (name, 'a ray grazes')
    elev = np.asarray(ref['elev'])
    out = {}
    h, w = c['height'], c['width']
    for thr in S.tested_thresholds(c):
        if np.isfinite(thr) and not np.isnan(elev).all():
            gap = float(np.nanmin(np.abs(elev - np.longdouble(thr))))
            assert gap >= S.THRESHOLD_GAP, (name, thr, 'a pixel lies at the threshold', gap)
        roles = S.band_roles(c, thr)
        assert roles['n'] == (h + S.ROWS - 1) // S.ROWS and roles['strips'] == (w + 1 + 62) // 63
        may = S.allowed(c, ref, thr)
        kinds = check_sound((name, thr, 'reference'), roles, may[:3])
        check_sound((name, thr, 'float64 oracle'), roles, S.allowed(c, f64, thr)[:3])
        may_inner, may_low, hit, least, most = may
        inner_margin = min([least[k] for k, v in enumerate(kinds) if v == 'i'] or [np.inf])
        low_margin = max([most[k] - thr for k, v in enumerate(kinds) if v == 'l' and np.isfinite(most[k])] or [-np.inf])
        out[thr_tag(thr)] = dict(kinds=kinds, roles=roles, inner_margin=float(inner_margin), low_margin=float(low_margin),
                                 lost_inner=sum(1 for k, v in enumerate(kinds) if v == 'g' and may_inner[k]),
                                 lost_low=sum(1 for k, v in enumerate(kinds) if v == 'g' and may_low[k] and hit[k]),
                                 want_inner=ranges(may_inner), want_low=(may_low & hit).copy())
    _SUMMARY[name] = out
    return out


@pytest.mark.parametrize('name', S.names())
def test_case_and_soundness(name):
    s = summarize(name)
    c = S.by_name(name)
    print('%s (%d nudges): %s' % (name, c['nudges'], '  '.join('%s %s' % (t, v['kinds']) for t, v in s.items())))


def slack_of(v):
    """(bands by which the rule's inner range ends short of the reference's at either end, bands of Earth the reference allows as
    low at the top and at the bottom that the rule leaves generic)"""
    roles, kinds = v['roles'], v['kinds']
    short = 0
    if v['want_inner'] is not None:
        a, b = v['want_inner']
        i0, i1 = roles['inner']
        short = b - a if i0 == i1 else max(i0 - a, b - i1, 0)
    n = roles['n']
    top = bottom = 0
    k = roles['sky'][0]
    while k < n and v['want_low'][k]:
        top += kinds[k] == 'g'
        k += 1
    k = roles['sky'][1] - 1
    while k >= 0 and v['want_low'][k]:
        bottom += kinds[k] == 'g'
        k -= 1
    return short, max(top, bottom)


@pytest.mark.parametrize('fam', ['aimed-threshold', 'aimed-limb'])
def test_aimed_families_are_not_vacuous(fam):
    seen = set()
    worst = (0, 0)
    for c in S.family(fam):
        s = summarize(c['name'])
        for t, v in s.items():
            seen.update(v['kinds'])
        line = c['claims']['line']
        if c['claims']['probe'] != 'column':
            continue
        # at the aimed threshold (the limb: none and 0) the rule follows the reference to within kSlackBands at every end
        for t in ((S.NONE, 0.0) if line is None else (line,)):
            short, low_short = slack_of(s[thr_tag(t)])
            worst = (max(worst[0], short), max(worst[1], low_short))
            assert short <= kSlackBands and low_short <= kSlackBands, (c['name'], t, s[thr_tag(t)]['kinds'], short, low_short)
    print(fam, 'roles seen', sorted(seen), 'largest shortfall in bands: inner %d, low %d' % worst)
    assert {'i', 'l', 'g'} <= seen, seen


def test_gates_and_thresholds_that_decide_nothing():
    for mode in ('', 'exact-'):
        s = summarize(mode + 'gate-elevation-inside')
        assert 'l' in s['30.0']['kinds'], s['30.0']
        s = summarize(mode + 'gate-elevation-outside')
        assert 'l' not in s['30.0']['kinds'] and 'l' not in s['60.0']['kinds'], s
        s = summarize(mode + 'gate-sky-inside')
        assert all('s' in v['kinds'] for v in s.values()), s
        s = summarize(mode + 'gate-sky-outside')
        assert all('s' not in v['kinds'] and 'l' not in v['kinds'] for v in s.values()), s
        # the inner rule has no gate: at 1 deg / px it still names bands
        assert 'i' in summarize(mode + 'scale-1-nadir')['0.0']['kinds']
        assert any('i' in v['kinds'] for n in S.names('scales') if n.startswith(mode + 'scale-1-thr') for v in summarize(n).values())
        # thresholds that decide nothing: NaN has no order, +inf, 90, 89.99 and 89 no pixel of these frames reaches (nothing inner; the gate of
        # elevation_bands refuses a cone that narrow, so nothing is low either), and nothing is decided from inside the shell
        s = summarize(mode + 'nothing-nadir')
        n = len(s['nan']['kinds'])
        assert s['nan']['kinds'] == 'g' * n and s['none']['kinds'] == 'i' * n and s['-5.0']['kinds'] == 'i' * n
        for t in ('inf', '90.0', '89.99', '89.0'):
            assert 'i' not in s[t]['kinds'], (t, s[t])
        for t, v in summarize(mode + 'nothing-inside').items():
            assert set(v['kinds']) == {'g'}, (t, v)
        assert summarize(mode + 'nothing-limb')['nan']['kinds'].count('i') == 0
        # nothing but sky, and too coarse for the sky rule: no role at all
        for t, v in summarize(mode + 'nothing-zenith').items():
            assert set(v['kinds']) == {'g'}, (t, v)


def report_lines():
    lines = []
    for fam in S.FAMILIES:
        for fast in (True, False):
            inner, low, lost_i, lost_l, bands = np.inf, -np.inf, 0, 0, 0
            where_i = where_l = None
            for n in S.names(fam, fast):
                for t, v in summarize(n).items():
                    bands += len(v['kinds'])
                    lost_i += v['lost_inner']
                    lost_l += v['lost_low']
                    if v['inner_margin'] < inner:
                        inner, where_i = v['inner_margin'], (n, t)
                    if v['low_margin'] > low:
                        low, where_l = v['low_margin'], (n, t)
            lines.append('  %-16s %-5s inner margin %.4f (%s at %s)  low %.4f (%s at %s)  generic of %d bands: %d inner, %d low allowed'
                         % ((fam, 'fast' if fast else 'exact', inner) + (where_i or ('-', '-')) + (low,) + (where_l or ('-', '-'))
                            + (bands, lost_i, lost_l)))
    return lines


def test_report_per_family():
    """smallest elevation above the threshold (above 0 where there is none) in an inner band, largest elevation minus threshold in
    a low band, bands left generic that the reference allows: the table of the module docstring"""
    print('\n'.join(report_lines()))


# ---- the pure rule ------------------------------------------------------------------------------------------------------------------
def build(tmp_path):
    """The program, with the sanitizers when a host compiler links and runs them here, else without."""
    src = os.path.join(HERE, 'csrc', 'band_roles_check.cpp')
    compilers = [c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)]
    assert compilers, 'no host C++ compiler'
    log = []
    for flags in (['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], []):
        for cxx in compilers:
            exe = str(tmp_path / ('band_roles_check' + ('_san' if flags else '')))
            cmd = [cxx, '-std=c++17', '-O1', '-g'] + flags + ['-I', CSRC, src, '-o', exe]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
            log.append(' '.join(cmd) + '\n' + res.stdout)
            if res.returncode == 0:
                probe = subprocess.run([exe, '0'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
                if probe.returncode == 0:
                    return exe, bool(flags)
                log.append('does not run: ' + probe.stdout)
    raise AssertionError('the program does not compile:\n' + '\n'.join(log))


def test_pure_rule_over_every_small_input(tmp_path):
    exe, sanitized = build(tmp_path)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print('sanitizers: %s' % ('address, undefined' if sanitized else 'not available, built without'))
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    last = res.stdout.splitlines()[-1]
    assert last.startswith('band_roles: ') and ' inputs, 0 violations' in last, last
    # n = 0 ... 6, seven arguments each over [-1, n + 1]
    assert int(last.split()[1]) == sum((n + 3) ** 6 for n in range(7)), last
    assert role_of_bands(dict(n=3, sky=(0, 3), low=(1, 2), inner=(1, 2))) == 'lil'
