"""
The cases of the gated side stream (tests/_gated_cases.py) without a GPU: every decoy is HARMLESS — another valid input of the
same shape and type, finite, in range, every index in range — and DISCRIMINATING: the CPU oracle of the case gives another
result for the decoy than for the true input in every output the GPU test compares, so a kernel that read the decoy cannot
reproduce the baseline by accident.  Cases without a CPU oracle are exempt from the second check, by name, three at the most.
"""
import numpy as np
import pytest

import _gated_cases as K

CASES = K.build()
IDS = [c.name for c in CASES]
RANGES = {'lat': 90.0, 'lat_c': 90.0, 'elev': 90.0, 'lon': 180.0, 'lon_c': 180.0}


def test_names_are_unique_and_exemptions_are_few():
    assert len(set(IDS)) == len(IDS)
    without = tuple(c.name for c in CASES if c.oracle is None)
    assert without == K.EXEMPT and len(K.EXEMPT) <= 3, without
    assert {c.family for c in CASES} == set('ABCDE')                 # (F, the staged copies, has no Case: tests/test_gpu_gated_stream.py)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_decoys_are_harmless(case):
    assert case.harmless, 'the case has to say why it cannot fault'
    for name, (true, decoy) in case.inputs.items():
        assert true.shape == decoy.shape and true.dtype == decoy.dtype, name
        assert not np.array_equal(true, decoy), (name, 'the decoy is the true array')
        for a in (true, decoy):
            if a.dtype.kind == 'f':
                assert np.isfinite(a).all(), (name, 'not finite')
            base = name[2:] if name[:2] in ('a_', 'b_') else name
            if base in RANGES:
                assert (np.abs(a) <= RANGES[base]).all(), (name, 'out of range')
            if base in ('img_mask', 'target_mask', 'has_nb') or base.startswith('cell_mask'):
                assert set(np.unique(a)) <= {0, 1}, name
            if base == 'dirs':
                assert np.allclose(np.linalg.norm(a, axis=-1), 1.0, rtol=0, atol=1e-12), name
        if true.dtype.kind in 'iu' and true.dtype.itemsize >= 4:
            assert name in case.index_ranges, (name, 'an integer input without a stated range')
    for name, rule in case.index_ranges.items():
        for a in case.inputs[name]:
            assert a.min() >= rule[0] and a.max() < rule[1], (name, int(a.min()), int(a.max()))
            assert 'distinct' not in rule or len(np.unique(a)) == a.size, (name, 'indices repeat')
            if name == 'indptr':
                assert a[0] == 0 and (np.diff(a) >= 0).all(), (name, 'offsets descend')
            if name == 'row_start':              # a partition of the points: the relaxation has to visit every one of them
                n = case.inputs['xy'][0].shape[0]
                assert a[0] == 0 and a[-1] == n and (np.diff(a) > 0).all(), (name, a.tolist())
    if 'indptr' in case.inputs:
        for indptr, indices in zip(case.inputs['indptr'], case.inputs['indices']):
            assert indptr[-1] == len(indices)
            own = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
            assert (indices != own).all(), 'a neighbour list holds its own vertex'
            assert (np.diff(indptr) >= 1).all() and (np.diff(indptr) < len(indptr) - 1).all()
    for name, a in case.out_fill.items():
        shape, dtype = case.outputs[name]
        assert a.shape == tuple(shape) and a.dtype == np.dtype(dtype) and not a.any(), name


@pytest.mark.parametrize('case', [c for c in CASES if c.oracle is not None], ids=[c.name for c in CASES if c.oracle is not None])
def test_decoys_are_discriminating(case):
    true = case.oracle({k: v[0] for k, v in case.inputs.items()})
    decoy = case.oracle({k: v[1] for k, v in case.inputs.items()})
    assert set(true) == set(decoy) and true
    for k in true:
        a, b = np.asarray(true[k]), np.asarray(decoy[k])
        assert a.size > 0, k
        assert a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), (case.name, k, 'the decoy gives the true result')
    # what the oracle gives is an output of the case or a proxy the case module names (sums*, box); the outputs of the case that
    # no oracle key stands for are listed by name in tests/_gated_cases.py UNCOVERED, nothing else goes unchecked
    named = set(case.outputs)
    assert set(true) <= named | {k for k in true if k.startswith('sums') or k == 'box'}, (set(true), named)
    assert named - set(true) == set(K.UNCOVERED.get(case.name, ())), (case.name, sorted(named - set(true)))


def test_the_decoy_camera_sees_another_part_of_the_earth():
    """The suspect's case: the box of the decoy directions is disjoint from the true one, so an estimate made from the decoy
    yields a superset grid the true frame does not fit into (status 1 instead of 0)."""
    t, d = K.frame_of_directions(K.directions(False)), K.frame_of_directions(K.directions(True))
    (s0, w0, n0, e0), (s1, w1, n1, e1) = t['box'], d['box']                  # (south, west, north, east)
    assert e0 < w1 or e1 < w0 or n0 < s1 or n1 < s0, (t['box'], d['box'])
    assert t['keep'].sum() > 100 and d['keep'].sum() > 100
    # beyond the margin of the superset grid (1 deg of latitude, 1 / cos(lat) deg of longitude) on the far side
    margin = 1.0 / np.cos(np.deg2rad(max(abs(s1), abs(n1))))
    assert w0 < w1 - margin - 1.0, (w0, w1, margin)
