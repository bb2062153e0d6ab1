"""
The library's host code from several host threads at once (no GPU).  include/auromat_hip.h promises that "the library keeps no
global state"; what the host side does keep is initialised on first use — the Gauss-Legendre nodes behind
amt_plate_carree_resolution (a static initialiser, csrc/amt_grid.h), the environment's thread counts of the triangulator — or
guarded by a lock (the triangulator's lazy compaction, two function-local static mutexes in csrc/amt_delaunay.hip).

  host entry points   eleven host-only entry points on fixed inputs from four threads at once behind a barrier, in a FRESH child
                      process, so that first-use initialisation is what races (tests/_threads_cpu_worker.py); every thread's
                      results must be bit-equal to those of a second child process that makes the same calls one after the
                      other.  Would catch: a table published before it is complete, a static buffer shared by two calls.
  two handles         two amt_delaunay_create_threads builds at once on different point sets with threads = 3 (pools inside
                      pools); triangles, neighbours and vertex lists equal to the same builds made one after the other.  Would
                      catch: the predicates' counters or a scratch list shared between builds.
  one handle          amt_delaunay_triangles and amt_delaunay_vertex_neighbours of ONE handle that nobody has read yet, from two
                      threads at once (both take the lazy compaction), equal to a handle compacted on one thread.  Would catch: a
                      compaction that runs twice or is read half-made.
The two triangulator scenarios also exist as a stand-alone C++ program for the thread sanitizer (tools/tsan_delaunay.cpp, its
build line in its header; the outcome is recorded in DESIGN.md): a sanitizer's runtime is never loaded into Python here.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT

WORKER = os.path.join(ROOT, 'tests', '_threads_cpu_worker.py')
LIMIT_S = 60.0


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from auromat_amd import _native
    return _native.lib()


def test_host_entry_points_from_four_threads_equal_the_sequential_answers(lib):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get('PYTHONPATH')] if p]))
    children = [subprocess.Popen([sys.executable, WORKER, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT)
                for mode in ('sequential', 'threads')]
    out = []
    for child in children:
        stdout, stderr = child.communicate(timeout=300)
        assert child.returncode == 0, stderr.decode()[-2000:]
        out.append(json.loads(stdout.decode().strip().splitlines()[-1]))
    (want,), runs = out[0]['runs'], out[1]['runs']
    assert len(runs) == 4 and len(want) == 11
    for t, got in enumerate(runs):
        assert sorted(got) == sorted(want)
        differ = [name for name in want if got[name] != want[name]]
        assert not differ, ('thread %d of 4 computed other bytes than the sequential process' % t, differ)


# ---- the triangulator ------------------------------------------------------------------------------------------------------------

THREADS, PARALLEL_MIN = 3, 300


def clouds():
    rng = np.random.RandomState(7)
    return [np.ascontiguousarray(rng.rand(6000, 2)), np.ascontiguousarray(rng.rand(4500, 2) * [30.0, 1.0])]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def build(lib, pts):
    h = C.c_void_p()
    assert lib.amt_delaunay_create_threads(_p(pts), len(pts), THREADS, PARALLEL_MIN, C.byref(h)) == 0
    info = (C.c_int64 * 2)()
    assert lib.amt_delaunay_build_info(h, info) == 0 and info[0] >= 2, ('not built in strips', list(info))
    return h


def triangles(lib, h, n):
    """(simplices, neighbours) in buffers that hold any triangulation of n points (at most 2 n triangles)"""
    tri, nbr = np.full((2 * n, 3), -7, dtype=np.int32), np.full((2 * n, 3), -7, dtype=np.int32)
    assert lib.amt_delaunay_triangles(h, _p(tri), _p(nbr)) == 0
    return tri, nbr


def vertex_neighbours(lib, h, n):
    """(indptr, indices) in buffers that hold the lists of any triangulation of n points (at most 6 n directed edges)"""
    indptr, indices = np.full(n + 1, -7, dtype=np.int64), np.full(6 * n, -7, dtype=np.int32)
    assert lib.amt_delaunay_vertex_neighbours(h, _p(indptr), _p(indices)) == 0
    return indptr, indices


def everything(lib, h, n):
    return triangles(lib, h, n) + vertex_neighbours(lib, h, n)


def run_two(fns):
    """fns on a thread each, started together -> their results; the first exception is raised again here"""
    start = threading.Barrier(len(fns), timeout=LIMIT_S)
    results, errors = [None] * len(fns), [None] * len(fns)

    def body(t):
        try:
            start.wait()
            results[t] = fns[t]()
        except BaseException as e:                      # noqa: B902
            errors[t] = e
            start.abort()

    threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(len(fns))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(LIMIT_S)
    assert not any(th.is_alive() for th in threads), 'a thread is still inside the triangulator'
    for e in errors:
        if e is not None:
            raise e
    return results


@pytest.fixture(scope='module')
def sequential(lib):
    """the lists of both point sets, each built and read alone"""
    out = []
    for pts in clouds():
        h = build(lib, pts)
        out.append(everything(lib, h, len(pts)))
        lib.amt_delaunay_destroy(h)
        assert (out[-1][0] != -7).any() and (out[-1][3] != -7).any()
    return out


def assert_lists_equal(got, want, what):
    for name, g, w in zip(('simplices', 'neighbours', 'indptr', 'indices'), got, want):
        assert np.array_equal(g, w), (what, name, int((g != w).sum()))


def test_two_triangulations_built_at_once_equal_the_sequential_builds(lib, sequential):
    sets = clouds()

    def one(pts):
        def fn():
            h = build(lib, pts)
            try:
                return everything(lib, h, len(pts))
            finally:
                lib.amt_delaunay_destroy(h)
        return fn

    got = run_two([one(pts) for pts in sets])
    for k in range(2):
        assert_lists_equal(got[k], sequential[k], 'point set %d' % k)


def test_one_triangulation_read_by_two_threads_before_it_is_compacted(lib, sequential):
    pts = clouds()[0]
    h = build(lib, pts)                                 # (nobody has asked for its sizes or lists: not compacted yet)
    try:
        tri, nb = run_two([lambda: triangles(lib, h, len(pts)), lambda: vertex_neighbours(lib, h, len(pts))])
    finally:
        lib.amt_delaunay_destroy(h)
    assert_lists_equal(tri + nb, sequential[0], 'one handle, two readers')
