"""The host plan of the mosaics (auromat_amd/csrc/amt_mosaic_plan.h: windows, unit prefix, select-tile lists, accumulator
offsets, workspace packer, member checks) against a brute-force restatement, in a stand-alone C++ program
(tests/csrc/mosaic_plan_check.cpp) built with the host compiler alone and, where its runtimes are there, under the address and
undefined-behaviour sanitizers.  The binary is run directly; nothing is loaded into this process."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'auromat_amd', 'csrc')
CASES = ('small_grid', 'tile_borders', 'middle_empty_nx', 'middle_empty_ny', 'many_65', 'all_empty', 'packer', 'refusals')


def build(tmp_path):
    """The program, with the sanitizers when a host compiler links and runs them here, else without."""
    src = os.path.join(HERE, 'csrc', 'mosaic_plan_check.cpp')
    compilers = [c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)]
    assert compilers, 'no host C++ compiler'
    log = []
    for flags in (['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], []):
        for cxx in compilers:
            exe = str(tmp_path / ('mosaic_plan_check' + ('_san' if flags else '')))
            cmd = [cxx, '-std=c++17', '-O1', '-g'] + flags + ['-I', CSRC, src, '-o', exe]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
            log.append(' '.join(cmd) + '\n' + res.stdout)
            if res.returncode == 0:
                return exe, bool(flags)
    raise AssertionError('the program does not compile:\n' + '\n'.join(log))


def test_plan_against_brute_force(tmp_path):
    exe, sanitized = build(tmp_path)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    print('sanitizers: %s' % ('address, undefined' if sanitized else 'not available, built without'))
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    lines = res.stdout.splitlines()
    assert [l.split(':')[0] for l in lines] == list(CASES)
    # the collections aim where they claim: long and empty member lists among the 65, nothing at all for the empty windows
    many = lines[CASES.index('many_65')]
    assert '65 members, 4 x 3 tiles' in many
    assert int(many.split('longest list ')[1].split(',')[0]) > 16 and int(many.split(', ')[-1].split(' ')[0]) >= 4
    assert '0 units, 0 words, longest list 0, 6 empty lists' in lines[CASES.index('all_empty')]


def test_the_header_is_the_one_definition():
    """kSelTile, the prefix search and the window rule live in the shared header only."""
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith(('.h', '.hip'))}
    assert [f for f, t in text.items() if 'constexpr int kSelTile' in t] == ['amt_mosaic_plan.h']
    assert [f for f, t in text.items() if 'window outside the grid' in t] == ['amt_mosaic_plan.h']
    assert [f for f, t in text.items() if 'start[mid] <= ' in t] == ['amt_mosaic_plan.h']
    host = text['amt_mosaic_plan.h'].split('#ifdef __HIPCC__')[0]
    assert 'hip/' not in host and '#include "' not in host
