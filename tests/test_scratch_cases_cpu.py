"""
The registry of scratch-memory users (tests/_scratch_cases.py) without a GPU: it lists exactly the call sites of amt_workspace
that the library's source has, the constants the GPU tests rely on are the source's, the debugging hook is declared where the
tests expect it, and the cases the registry adds follow the rules of tests/test_gated_cases_cpu.py — their decoys are harmless
and their CPU oracles tell the decoy from the true input in every output the GPU test compares.
"""
import os
import re

import numpy as np
import pytest

import _scratch_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'auromat_amd', 'csrc')
ADDED = S.added()
WITH_ORACLE = [c for c in ADDED if c.oracle is not None]


def call_sites():
    """[(file, enclosing function)] of every `amt_workspace(` in auromat_amd/csrc but its definition, in the order of the source"""
    sites = []
    head = re.compile(r'^(?:extern "C" )?(?:static )?(?:inline )?[A-Za-z_][\w:<>]*[ \*&]+(\w+)\(')
    for name in sorted(os.listdir(CSRC)):
        function = None
        with open(os.path.join(CSRC, name)) as fp:
            for line in fp:
                m = head.match(line)
                if m and not line.startswith(('return', 'typedef', 'using')):
                    function = m.group(1)
                if 'amt_workspace(' in line and not line.lstrip().startswith('//') and function != 'amt_workspace':
                    sites.append((name, function))
    return sites


def test_every_call_site_has_a_case():
    sites = call_sites()
    assert len(sites) == len(set(sites)) == 16, sites                    # the fifteen users and the hook
    assert set(sites) == set(S.SITES) | {S.HOOK_SITE}, set(sites) ^ (set(S.SITES) | {S.HOOK_SITE})
    assert len(S.SITES) == 15
    names = set(c.name for c in S.build())
    for site, cases in S.SITES.items():
        assert cases and set(cases) <= names, (site, cases)
    assert len(set(S.MINIMUM)) == len(S.SITES)                           # one case of its own per call site
    # every call site has a larger shape or a reason why none can exist
    large = S.large()
    assert set(large) | set(S.NO_LARGE) == set(S.SITES) and not set(large) & set(S.NO_LARGE)
    for site, need in S.large_bytes().items():
        assert site in large and need > S.MIN_BYTES, (site, need)
    assert set(S.large_bytes()) == set(large)
    assert len(set(c.name for c in large.values())) == len(large) and not set(c.name for c in large.values()) & names


def test_constants_are_the_source_s():
    common = open(os.path.join(CSRC, 'amt_common.h')).read()
    m = re.search(r'constexpr size_t kMaxWorkspaces = (\d+);', common)
    assert m and int(m.group(1)) == S.MAX_STREAMS == 16
    assert 'const size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes;' in common and S.MIN_BYTES == 1 << 20
    assert 'w->last_use = request ? ++ctx->workspace_clock : ctx->workspace_clock;' in common
    # what NO_LARGE and large_bytes() rest on
    assert 'if (blocks > 256 * 16) blocks = 256 * 16;' in common
    header = open(os.path.join(ROOT, 'include', 'auromat_hip.h')).read()
    assert re.search(r'#define AMT_GATHER_MAX_JOBS 64\b', header)
    assert re.search(r'#define AMT_SIP_MAX 10\b', header)
    assert 'amt_workspace(ctx, 256)' in open(os.path.join(CSRC, 'amt_scanline.hip')).read()
    assert 'amt_workspace(ctx, sizeof(unsigned int))' in open(os.path.join(CSRC, 'amt_area.hip')).read()


def test_the_hook_is_declared():
    from auromat_amd import _native
    header = open(os.path.join(ROOT, 'include', 'auromat_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in S.HOOK:
        assert re.search(r'\bint %s\(amt_ctx\* ctx' % name, code), name
        assert name in _native._SIGNATURES, name
    assert 'test and debugging aid' in header
    assert int(re.search(r'#define AMT_ABI_VERSION (\d+)', header).group(1)) == _native.ABI_VERSION == 10
    # the context's own 256 bytes that nothing read are gone
    assert not re.search(r'\bdouble\* scratch;', open(os.path.join(CSRC, 'amt_common.h')).read())
    assert 'ctx->scratch' not in open(os.path.join(CSRC, 'amt_context.hip')).read()


def test_added_cases_and_exemptions():
    names = [c.name for c in S.build()]
    assert len(set(names)) == len(names)
    assert tuple(c.name for c in ADDED if c.oracle is None) == S.EXEMPT
    assert set(S.USERS) <= set(names)
    # baselines are remembered by name for the whole session (tests/_gated_stream.py): no other module may make a case under a
    # name this registry adds
    here = ('_scratch_cases.py', 'test_gpu_scratch_state.py', 'test_scratch_cases_cpu.py', '_gated_gather_frames_cases.py')
    mine = [c.name for c in ADDED if not c.name.startswith('gather_frames_x')] + [c.name for c in S.large().values()] + \
        ['gather_member_0', 'gather_member_1', 'gather_points']
    for name in sorted(os.listdir(os.path.join(ROOT, 'tests'))):
        if name.endswith('.py') and name not in here:
            text = open(os.path.join(ROOT, 'tests', name)).read()
            for case in mine:
                assert "Case('%s'" % case not in text, (name, case)


@pytest.mark.parametrize('case', ADDED, ids=[c.name for c in ADDED])
def test_decoys_are_harmless(case):
    assert case.harmless, 'the case has to say why it cannot fault'
    for name, (true, decoy) in case.inputs.items():
        assert true.shape == decoy.shape and true.dtype == decoy.dtype, name
        assert not np.array_equal(true, decoy), (name, 'the decoy is the true array')
        for a in (true, decoy):
            if a.dtype.kind == 'f':
                assert np.isfinite(a).all(), (name, 'not finite')
            if name in ('lat', 'lat_c', 'elev') or name[2:] in ('lat', 'lat_c', 'elev'):
                assert (np.abs(a) <= 90.0).all(), (name, 'out of range')
            if name in ('lon', 'lon_c') or name[2:] in ('lon', 'lon_c'):
                assert (np.abs(a) <= 180.0).all(), (name, 'out of range')
            if name in ('keep', 'center_mask'):
                assert set(np.unique(a)) <= {0, 1}, name
            if name == 'dirs':
                assert np.allclose(np.linalg.norm(a, axis=-1), 1.0, rtol=0, atol=1e-12), name
        if true.dtype.kind in 'iu' and true.dtype.itemsize >= 4:
            assert name in case.index_ranges, (name, 'an integer input without a stated range')
    for name, rule in case.index_ranges.items():
        for a in case.inputs[name]:
            assert a.min() >= rule[0] and a.max() < rule[1], (name, int(a.min()), int(a.max()))
    if case.name == 'scanline_pack':                                     # `count` is a host argument: both keep arrays hold it
        assert case.inputs['keep'][0].sum() == case.inputs['keep'][1].sum() > 64


@pytest.mark.parametrize('case', WITH_ORACLE, ids=[c.name for c in WITH_ORACLE])
def test_oracles_tell_the_decoy_from_the_true_input(case):
    true = case.oracle({k: v[0] for k, v in case.inputs.items()})
    decoy = case.oracle({k: v[1] for k, v in case.inputs.items()})
    assert set(true) == set(decoy) == set(case.outputs), (set(true), set(case.outputs))
    for k in true:
        a, b = np.asarray(true[k]), np.asarray(decoy[k])
        shape, dtype = case.outputs[k]
        assert a.size == int(np.prod(shape)), (k, a.shape, shape)
        assert a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), (case.name, k, 'the decoy gives the true result')


def test_oracles_hold_what_the_cases_are_made_for():
    by = {c.name: c for c in ADDED}
    true = lambda name: by[name].oracle({k: v[0] for k, v in by[name].inputs.items()})
    # the union median: cells that both members fill, cells of one member alone, empty cells
    r = true('mosaic_median_union')
    src = r['source']
    assert set(np.unique(src)) == {-1, 0, 1} and np.array_equal(src < 0, r['mask'] != 0)
    assert (r['count'][src >= 0] > 0).all() and not np.isnan(r['mean'][src >= 0][:, :3]).any()
    # the finalise step alone: valid and invalid cells, and what amt_area_frame + finalise give for the same frame
    r = true('area_finalize')
    assert 0 < (r['mask'] != 0).sum() < r['mask'].size
    import _gated_cases as K
    whole = K._oracle_area(dict((k, K.TRUE[k]) for k in ('lat', 'lon', 'lat_c', 'elev', 'img')))
    for k in r:
        assert np.array_equal(np.asarray(r[k]), np.asarray(whole[k]), equal_nan=True), k
    # the records of a strip, and the raster of two strips that overlap
    n = int(by['scanline_pack'].inputs['keep'][0].sum())
    assert true('scanline_pack')['records'].size == n * S.REC_BYTES
    assert np.array_equal(S.sorted_records(true('scanline_pack')['records']), true('scanline_pack')['records'])
    r = true('scanline_compose')
    assert set(np.unique(r['frame_index'])) == {-1, 0, 1}
    assert np.array_equal(r['planes'], K._oracle_scanline(dict((k, v[0]) for k, v in K._scanline_inputs().items()))['planes'], equal_nan=True)
    # the coarse box: a box of corners that count, fewer than the corners that hit
    b = true('coarse_bbox_dirs')['bbox']
    assert b[0] < b[1] and b[2] < b[3] and b[6] > 20 and np.isfinite(b[:4]).all()


def test_both_gather_members_see_the_grid():
    import _gather_frames_cases as FC
    j = FC.by_name(S.GATHER_JOB)
    seen = [FC.seen_points(dict(j, cam=c)) for c in S.GATHER_CAMS]
    assert all(s.sum() > 100 for s in seen) and (seen[0] & seen[1]).sum() > 100 and (~(seen[0] | seen[1])).sum() > 100
    assert (seen[0] & ~seen[1]).any() and (seen[1] & ~seen[0]).any()
