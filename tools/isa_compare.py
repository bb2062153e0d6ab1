"""Compares the instruction streams of the kernels in two assembly files of the same source at two commits, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Iauromat_amd/csrc -c auromat_amd/csrc/amt_area.hip -save-temps -o x.o
        (in a directory of its own per commit; keeps <name>-hip-amdgcn-amd-amdhsa-gfx950.s)
    isa_compare.py BEFORE.s AFTER.s [--match TEXT] [--drop-arg N]

Per kernel the lines between its label and its .Lfunc_end are taken; comments, blank lines and assembler directives are dropped,
basic-block labels are renumbered in order of appearance and mangled symbols inside instructions are replaced by SYM, so that a
renamed or re-mangled kernel compares equal when its instructions are.  A kernel whose template gained a defaulted trailing bool
parameter is matched with its earlier name by --drop-arg N: the N-th from last `Lb0E` of the mangled name and the matching
`XT<k>_E` of its argument type are removed before names are compared.  One line per kernel: IDENTICAL / DIFFERENT with the line
counts, or the side it exists on only.  CPU only."""
import argparse, re, sys

ap = argparse.ArgumentParser()
ap.add_argument('before')
ap.add_argument('after')
ap.add_argument('--match', default='', help='only kernels whose mangled name contains this text')
ap.add_argument('--drop-arg', type=int, default=0, help='1: drop the last defaulted bool template argument (false) of the AFTER names')
a = ap.parse_args()


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is not None:
            if line.startswith('.Lfunc_end'):
                cur = None
                continue
            out[cur].append(line)
    return out


def normalised(lines):
    res, labels = [], {}
    for l in lines:
        l = l.split(';')[0].rstrip()
        if not l.strip():
            continue
        if l.lstrip().startswith('.') and not re.match(r'^\.LBB\d+_\d+:', l):
            continue
        l = re.sub(r'\.LBB\d+_\d+', lambda m: labels.setdefault(m.group(0), 'L%d' % len(labels)), l)
        res.append(re.sub(r'_Z\w+', 'SYM', l))
    return res


def earlier_name(name):
    if not a.drop_arg:
        return name
    # ...Lb0ELb0EEEv... IXT0_EXT1_EE  ->  ...Lb0EEEv... IXT0_EE
    m = re.match(r'^(.*)Lb0E(EEv.*)XT\d+_E(E.*)$', name)
    return m.group(1) + m.group(2) + m.group(3) if m else name


before = {k: normalised(v) for k, v in kernels(a.before).items()}
after = {earlier_name(k): normalised(v) for k, v in kernels(a.after).items()}
different = 0
for k in sorted(set(before) | set(after)):
    if a.match not in k:
        continue
    if k in before and k in after:
        same = before[k] == after[k]
        different += not same
        print('%s  %d / %d lines  %s' % (k, len(before[k]), len(after[k]), 'IDENTICAL' if same else 'DIFFERENT'))
    else:
        print('%s  only in %s (%d lines)' % (k, 'BEFORE' if k in before else 'AFTER', len(before.get(k) or after.get(k))))
sys.exit(1 if different else 0)
