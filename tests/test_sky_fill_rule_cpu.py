"""
The host rule behind the sequence runner's sky fill (no GPU): amt_prm::sky_fill of csrc/amt_params.h — which sky bands of a
frame still have to be written when its slot's arrays hold `known` bands of NaN, and what they hold afterwards — against a
bitmask model, for every state and every sky of up to 6 bands.  Reached like amt_gl's helpers in tests/test_host_rules_cpu.py:
a probe compiled against the header.
"""
import os
import subprocess

from conftest import ROOT

PROBE = r'''
#include <climits>
#include <cstdio>
#include "amt_params.h"
int main() {
    for (int n = 0; n <= 6; ++n)
        for (int kt = 0; kt <= n; ++kt)
            for (int kb = 0; kb <= n + 1; ++kb)
                for (int t = 0; t <= n; ++t)
                    for (int b = 0; b <= n; ++b) {
                        // (kb = n + 1 stands for "nothing known", sky_known_empty(): a bottom_begin beyond every band count)
                        const amt_prm::sky_known known = {kt, kb > n ? amt_prm::sky_known_empty().bottom_begin : kb};
                        int f0 = -1, f1 = -1;
                        const amt_prm::sky_known after = amt_prm::sky_fill(known, n, t, b, &f0, &f1);
                        std::printf("%d %d %d %d %d %d %d %d %d\n", n, kt, kb, t, b, f0, f1, after.top_end, after.bottom_begin);
                    }
    const amt_prm::sky_known e = amt_prm::sky_known_empty();
    std::printf("empty %d %d\n", e.top_end, e.bottom_begin > 1000000 ? -1 : e.bottom_begin);
    return 0;
}
'''


def bands(n, top_end, bottom_begin):
    """bitmask of [0, top_end) | [bottom_begin, n)"""
    return sum(1 << c for c in range(n) if c < top_end or c >= bottom_begin)


def test_fill_and_known_cover_the_sky_for_every_state_of_up_to_six_bands(tmp_path):
    src = tmp_path / 'probe.cpp'
    src.write_text(PROBE)
    exe = str(tmp_path / 'probe')
    res = subprocess.run(['g++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'auromat_amd', 'csrc'), str(src), '-o', exe],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert res.returncode == 0, res.stdout
    lines = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split('\n')
    assert lines[-2] == 'empty 0 -1'                       # nothing known: one form for every band count
    seen = 0
    skipped_something = filled_more_than_needed = 0
    for line in lines[:-2]:
        n, kt, kb, t, b, f0, f1, at, ab = [int(v) for v in line.split()]
        known, sky = bands(n, kt, min(kb, n)), bands(n, t, b)
        # what the kernel writes: a sky item of band c fills iff f0 <= c < t or b <= c < f1
        fill = sum(1 << c for c in range(n) if (c < t or c >= b) and (f0 <= c < t or b <= c < f1))
        assert 0 <= f0 <= n and 0 <= f1 <= n, line
        assert (fill | known) & sky == sky, line               # nothing of the sky is left as it was unless it is known NaN
        assert fill & ~sky == 0, line                          # (the kernel fills sky bands only)
        assert (at, ab) == (t, b), line                        # afterwards the arrays hold the frame's own sky
        if known == 0:
            assert fill == sky and (f0, f1) == (0, n), line    # nothing known: every sky band, the range of a plain launch
        if fill != sky:
            skipped_something += 1
        if fill & known:
            filled_more_than_needed += 1                       # allowed (known bottom bands inside a growing top range, ...)
        seen += 1
    assert seen == sum((n + 1) ** 3 * (n + 2) for n in range(7))
    assert skipped_something > seen // 2 and filled_more_than_needed > 0
