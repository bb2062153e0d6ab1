"""
The Python layer from several host threads (tests/_threads.py): one context, one set of class pipelines and one stream per
thread.  Synthetic 256 x 170 frames; the 'iss030' and 'iss029' pointings have one size and one image type, hence the same keys
in the pipeline caches of the class paths.  Every result is compared, bit for bit, with the same call made alone on the main
thread beforehand.  Every test asserts object identity FIRST and only then does concurrent GPU work: on a tree in which two
threads get the same pipeline, it fails before the two of them ever drive one amt_pipe.

  test_class_pipelines_are_per_thread     fused_class_pipeline and the gather plans' box pipeline, called from two threads with
                                          one key, are different objects with different ctx.handle; a second call on the same
                                          thread gives the same object (the cache works).  Catches: a pipeline cache keyed
                                          without the thread (one amt_ctx, one amt_pipe, one set of accumulators from two
                                          threads at once, which include/auromat_hip.h forbids).
  test_concurrent_class_resampling        two threads, a barrier before each call: resample() (the fused plan), resample_frame
                                          (method='mean'), resampleMedian, resampleArea, resampleGather on their two mappings.
                                          Catches: anything of the class paths shared between threads — pipelines, cached
                                          grids, staging buffers.
  test_fused_resample_while_another_thread_is_held
                                          thread A calls the fused resample() behind a gate on its stream (the call
                                          synchronises inside: A sits in the library), thread B resamples the other mapping
                                          meanwhile; B's call must start while A is inside its own.
  test_one_grid_table_is_settled_before_it_is_kept, test_grid_tables_are_settled_before_they_are_kept
                                          THE COVER of the finding "cached device tables across streams", on one thread, behind
                                          a gate on the current stream.  One table of 1.03 MiB (the asynchronous staged upload)
                                          through _Grid._settled must come back with the gate OPEN: the uploading stream was
                                          waited for before the table was kept, and the process-wide cache hands a grid's tables
                                          to every thread.  device_corners of a fresh grid with 368 x 368 corners and
                                          device_centers of one with 135 999 rows and columns (two tables of 1.03 / 1.04 MiB
                                          each) keep their tables through that helper and hold the host arrays.  Catches: tables
                                          kept as soon as their upload is enqueued (the one-table test), an entry point that
                                          keeps tables another way.
  test_shared_grid_tables                 the equality check of one cached grid used from two streams: two threads on one
                                          bounding box and one resolution (8 x 8 deg at 46 px/deg), resample_frame with
                                          method='nearest' — the call that reads the grid's cached device tables (corners through
                                          amt_points_in_polygon, centres through amt_nearest_frame) —, method='mean' and
                                          gather_frame.  A is first, its stream gated, and puts the corner tables up under its
                                          gate; B comes second.  Both must get the single-thread results.  It does not tell
                                          settled tables from unsettled ones (the test above does): with settled tables A keeps
                                          nothing before its gate opens and B uploads its own, and B's calls leave only when
                                          A's gate opens in any case (below).
                                          Harmlessness: the tables are coordinates.  Unwritten tables are arbitrary doubles that
                                          amt_points_in_polygon only compares with the polygon's edges (a mask byte 0 / 1 per
                                          point) and that amt_nearest_frame only looks up by a bounded search of the axes: wrong
                                          cells, never an address; nothing read from a table is used as an index.
  test_handed_over_pipelines              a FramePipeline and a SequencePipeline built on the main thread, then used by ONE worker
                                          thread only, through G.run_gated on the worker's side stream (the pipeline_run_dirs
                                          and sequence_pipeline cases of tests/_gated_cases.py).  Within the header's rule (one
                                          thread at a time).  Catches: a pipeline that re-binds the calling thread's cached
                                          context instead of its own, and so keeps enqueueing on the stream its creator last
                                          had current — the gate would not hold its kernels and they would read the decoys.
  test_two_sequence_pipelines_at_once     two threads run the sequence_pipeline case at the same time, each with a
                                          SequencePipeline of its own; the main / alt / bin / copy streams are shared by every
                                          SequencePipeline of the process (pipeline._STREAMS).  Catches: results that depend on
                                          that sharing.

Measured on an MI355X with GPU_MAX_HW_QUEUES=4 (printed with -s).  Host time of the calls alone on the main thread, warm:
resample() 2.5 / 3.5 ms (iss030 / iss029), resample_frame 1.0 / 1.1, resampleMedian 1.9 / 3.7, resampleArea 1.9 / 2.2,
resampleGather 2.1 / 1.7; on the 8 x 8 deg grid nearest 2.5, mean 0.4, gather 0.5 ms; every gate is therefore 100 ms.
  held fused resample()   A's call took 101 - 103 ms; B's started 5.2 - 5.4 ms after A's and took 98 - 100 ms, both results equal
                          to the single-thread ones.  B's call returns when A's gate opens: a thread's FIRST fused resample()
                          waits for the whole device (397 ms behind a 400 ms hold of another thread, then 4.2 and 3.7 ms for the
                          second and third call beside the same hold; the cause is SUPPOSED, not shown: hipFree / hipHostFree and the
                          page-locked allocations of a new driver and copier synchronise the device).
  shared grid             A was held for 122 - 130 ms; B started 5.1 - 5.4 ms after A and took 118 - 131 ms where the three calls
                          take 3.4 ms alone: B, too, leaves when A's gate opens (the results of 4 MiB travel into page-locked
                          arrays made per call; the cause is supposed as above, not shown).
  one settled table       the call returns after 98.5 - 99.0 ms behind the 100 ms gate, the gate open; kept without the wait it
                          returns after 0.3 ms, the gate closed.
What the module catches, by mutant:
  Context.bind() re-binds the calling thread's cached context      test_handed_over_pipelines fails: pipeline_run_dirs returns the
                                                                   grid of the decoy directions, (9, 22, 4) for (14, 21, 4)
  _Grid._settled keeps the tables without waiting for the stream   test_one_grid_table_is_settled_before_it_is_kept fails (the
                                                                   gate is closed on return); test_shared_grid_tables passes
  two threads given one class pipeline                             not run on purpose (two threads would drive one amt_pipe);
                                                                   Identity.check is what fails there, before any concurrent launch
"""
import time
from collections import OrderedDict

import numpy as np
import numpy.ma as ma
import pytest

import _gated_cases as K
import _gated_stream as G
import _threads as T

pytestmark = pytest.mark.gpu

W, H = 256, 170
POINTINGS = ('iss030', 'iss029')
SEED = {'iss030': 3, 'iss029': 5}
MIN_ELEV = 10
PPD = 10
CALLS = ('resample', 'resample_frame', 'resampleMedian', 'resampleArea', 'resampleGather')
_alone = {}


@pytest.fixture(autouse=True)
def _not_hung():
    T.fail_if_hung()


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    if T._state['hung'] is None:
        K.release()


def mapping(pointing):
    """a fresh camera mapping of the pointing: nobody has asked for its arrays, the elevation mask is only remembered"""
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_header, frame_image
    hdr, cam, t = frame_header(W, H, pointing)
    m = ArraySpacecraftMapping(hdr, 110, frame_image(W, H, seed=SEED[pointing]), cam, t, pointing, fastCenterCalculation=True)
    return m.maskedByElevation(MIN_ELEV)


def of_mapping(m):
    """grid, image, mask, elevation and box of a resampled mapping"""
    bb = m.boundingBox
    return OrderedDict(lats=np.asarray(ma.getdata(m.lats)), lons=np.asarray(ma.getdata(m.lons)), img=np.asarray(ma.getdata(m.img)),
                       mask=ma.getmaskarray(m.img), elevation=ma.filled(m.elevation, np.nan),
                       box=np.array([bb.latSouth, bb.lonWest, bb.latNorth, bb.lonEast]))


def of_dict(res):
    return OrderedDict((k, np.asarray(v)) for k, v in sorted(res.items()) if isinstance(v, np.ndarray))


def call(name, pointing):
    from auromat_amd import resample as R
    m = mapping(pointing)
    if name == 'resample':
        return of_mapping(R.resample(m, pxPerDeg=PPD))
    if name == 'resample_frame':
        return of_dict(R.resample_frame(m.frame(), m.altitude, m.boundingBox, (PPD, PPD), m.containsDiscontinuity, m.containsPole,
                                        method='mean'))
    if name == 'resampleMedian':
        return of_mapping(R.resampleMedian(m, pxPerDeg=PPD))
    if name == 'resampleArea':
        return of_mapping(R.resampleArea(m, pxPerDeg=PPD))
    return of_mapping(R.resampleGather(m, pxPerDeg=PPD))


def alone(name, pointing):
    """the call made alone on the main thread (once per session), and the host time of a second, warm call"""
    key = (name, pointing)
    if key not in _alone:
        import torch
        first = call(name, pointing)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        second = call(name, pointing)
        ms = (time.perf_counter() - t0) * 1e3
        assert_same(second, first, ('two runs on the main thread', name, pointing))
        assert first['mask'].size > 500 and (~first['mask'].astype(bool)).sum() > 100, (name, pointing, 'hardly a cell is filled')
        print('%s(%s) alone on the main thread: %.1f ms of host time' % (name, pointing, ms))
        _alone[key] = (first, ms)
    return _alone[key]


def assert_same(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, k, 'other bytes than the call alone on the main thread',
                                            int((g != w).sum()) if g.dtype.kind != 'f' else int((~np.isclose(g, w, equal_nan=True)).sum()))


def class_pipelines(ctx):
    """the cached pipelines of the calling thread for the frames of this module: (fused, box pass), each asked for twice"""
    from auromat_amd import resample as R
    from auromat_amd.pipeline import fused_class_pipeline
    fused, box = fused_class_pipeline(W, H, np.uint16), R.gather_box_pipeline(ctx, W, H)
    assert fused_class_pipeline(W, H, np.uint16) is fused and R.gather_box_pipeline(ctx, W, H) is box, 'the cache does not keep them'
    return fused, box


class Identity(object):
    """what every concurrent test does first: the threads' pipelines, shown to each other before any GPU work"""

    def __init__(self, sync, n=2):
        self.pipes = [None] * n
        self.shown = sync.barrier(n)

    def check(self, t, ctx):
        self.pipes[t] = class_pipelines(ctx)
        self.shown.wait()
        for kind in (0, 1):
            objs = [p[kind] for p in self.pipes]
            assert len(set(id(o) for o in objs)) == len(objs), ('two host threads were given ONE pipeline', kind, objs)
            assert len(set(o.ctx.handle.value for o in objs)) == len(objs), ('two pipelines on one amt_ctx', kind)
            assert objs[t].ctx is ctx, 'a thread\'s pipeline is not on the thread\'s context'


def test_class_pipelines_are_per_thread():
    sync = T.Barriers()
    identity = Identity(sync)
    T.run_threads([lambda ctx, stream, t=t: identity.check(t, ctx) for t in range(2)], sync=sync)


def test_concurrent_class_resampling():
    want = dict((p, [alone(name, p)[0] for name in CALLS]) for p in POINTINGS)
    sync = T.Barriers()
    identity = Identity(sync)
    steps = [sync.barrier(2) for _ in CALLS]

    def thread(t):
        def fn(ctx, stream):
            identity.check(t, ctx)
            for step, name, w in zip(steps, CALLS, want[POINTINGS[t]]):
                step.wait()
                assert_same(call(name, POINTINGS[t]), w, ('thread %d' % t, name, POINTINGS[t]))
        return fn

    T.run_threads([thread(0), thread(1)], sync=sync)


def test_fused_resample_while_another_thread_is_held():
    (want_a, _), (want_b, ms_b) = alone('resample', POINTINGS[0]), alone('resample', POINTINGS[1])
    gate_ms = G.gate_ms_for(ms_b)
    G.cycles_per_ms()                               # (calibrated here: it synchronises the device, which no thread may)
    sync = T.Barriers()
    identity = Identity(sync)
    inside = sync.event()

    def thread_a(ctx, stream):
        identity.check(0, ctx)
        T.StreamGate(gate_ms)
        inside.set()
        t_in = time.perf_counter()
        got = call('resample', POINTINGS[0])             # uploads and launches behind the gate, then waits for its results
        t_out = time.perf_counter()
        assert_same(got, want_a, 'the held thread')
        return t_in, t_out

    def thread_b(ctx, stream):
        identity.check(1, ctx)
        T.wait_event(inside)
        time.sleep(0.005)
        t0 = time.perf_counter()
        got = call('resample', POINTINGS[1])
        t1 = time.perf_counter()
        assert_same(got, want_b, 'thread B')
        return t0, t1

    (t_in, t_out), (t0, t1) = T.run_threads([thread_a, thread_b], sync=sync)
    print('resample() of A held for %.0f ms (gate %.0f ms); B\'s resample() started %.1f ms after A\'s and took %.1f ms'
          % ((t_out - t_in) * 1e3, gate_ms, (t0 - t_in) * 1e3, (t1 - t0) * 1e3))
    assert t_in < t0 < t_out, ('thread B did not start while A was inside the library: nothing was proved',
                               (t0 - t_in) * 1e3, (t_out - t_in) * 1e3)


# ---- one cached grid, two streams --------------------------------------------------------------------------------------------------

BIG_PPD = (46, 46)
SHARED = ('nearest', 'mean', 'gather')


def shared_box():
    """8 x 8 deg around the middle of the iss030 frame's own box (whole degrees; the frame's box is 6.3 x 10.3 deg: pixels
    outside the 8 x 8 deg are outliers of the binning, cells outside the frame stay empty)"""
    from auromat_amd.mapping.mapping import BoundingBox
    bb = mapping('iss030').boundingBox
    assert not bb.containsDiscontinuity and bb.latNorth - bb.latSouth > 4 and bb.lonEast - bb.lonWest > 4, bb
    lat0, lon0 = round(0.5 * (bb.latSouth + bb.latNorth)), round(0.5 * (bb.lonWest + bb.lonEast))
    return BoundingBox(lat0 - 4.0, lon0 - 4.0, lat0 + 4.0, lon0 + 4.0)


def shared_grid(box):
    from auromat_amd import resample as R
    return R.cached_grid(BIG_PPD, box.latSouth, box.latNorth, box.lonWest, box.lonEast)


def shared_calls(m, box):
    """[(name, function)] on a mapping whose arrays exist: everything on the grid of `box` at 46 px/deg"""
    from auromat_amd import resample as R
    fd = m.frame()
    s, w, n, e = box.latSouth, box.lonWest, box.latNorth, box.lonEast
    outline = np.array([[s + 1, w + 1], [s + 1, e - 1], [n - 1, e - 1], [n - 1, w + 1]], dtype=np.float64)
    plan = dict(altitude=m.altitude, params=m._inverse_model()[0], zenithal=None, min_elevation=float(MIN_ELEV), center_mask=None,
                grid=None, contains_pole=False, contains_discontinuity=False)

    def gather():
        return R.gather_frame(dict(plan, grid=shared_grid(box)), m._img_array)

    return [('nearest', lambda: R.resample_frame(fd, m.altitude, box, BIG_PPD, False, False, method='nearest', outline=outline)),
            ('mean', lambda: R.resample_frame(fd, m.altitude, box, BIG_PPD, False, False, method='mean')),
            ('gather', gather)]


STAGED = 1 << 20                                # arrays of this size and more go up through the asynchronous staged upload


def _warmed_stream(arrays):
    """A side stream on which the arrays have gone up once already: behind the gate nothing but the upload is left to wait
    for (torch's allocator hands the same blocks out again and the context's copier has its page-locked pieces; a fresh
    hipMalloc or hipHostMalloc behind the gate could wait for the device, i.e. for the gate)."""
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        warm = [T_context().to_device(a) for a in arrays]
        side.synchronize()
        del warm
    return side


def _table_grid(tables):
    from auromat_amd import resample as R
    if tables == 'corners':
        grid = R._Grid(BIG_PPD, 47.0, 55.0, -101.0, -93.0)
        want = (np.ascontiguousarray(grid.lat.T), np.ascontiguousarray(grid.lon.T))
    else:
        grid = R._Grid((800, 400), -85.0, 85.0, -170.0, 170.0)        # 135 999 rows and columns: only the axes are ever made
        want = (np.ascontiguousarray(grid.latCenters), np.ascontiguousarray(grid.lonCenters))
    assert all(a.nbytes >= STAGED for a in want), [a.nbytes for a in want]
    return grid, want


def test_one_grid_table_is_settled_before_it_is_kept():
    """One thread, one table of 1.03 MiB through _Grid._settled (what device_corners and device_centers keep their tables
    with), behind a gate on the current stream: the call returns with the gate OPEN, because the uploading stream was waited
    for before the table was kept.  A table kept as soon as its upload is enqueued comes back at once, the gate closed."""
    import torch
    grid, want = _table_grid('corners')
    side = _warmed_stream(want[:1])
    with G.Gate(side=side) as gate:
        t0 = time.perf_counter()
        got = grid._settled(('one table', 0), T_context(), lambda: want[:1])
        ms = (time.perf_counter() - t0) * 1e3
        open_on_return = gate.opened.query()
    side.synchronize()
    host = got[0].cpu().numpy()
    torch.cuda.synchronize()
    T_context()                                     # the library follows torch back to the default stream
    print('one table: the call took %.1f ms behind a gate of %.0f ms and returned with the gate %s'
          % (ms, gate.ms, 'open' if open_on_return else 'closed'))
    assert grid._axes[('one table', 0)] is got
    assert open_on_return, 'the table was kept while its upload was still waiting behind the gate (%.0f ms)' % gate.ms
    assert host.tobytes() == want[0].tobytes()


@pytest.mark.parametrize('tables', ['corners', 'centers'])
def test_grid_tables_are_settled_before_they_are_kept(tables):
    """device_corners / device_centers of a fresh grid (two tables of 1.03 / 1.04 MiB each) behind a gate on the current
    stream: they keep their tables through _Grid._settled, one call, and come back with the gate open and the host arrays in
    the tables.  (The second table's upload waits on the host for the staging piece of the first one, so a call with two
    tables returns with the gate open whether it settles or not: the one-table test above is what tells the two apart, this
    one holds the two entry points to the helper it covers.)"""
    import torch
    grid, want = _table_grid(tables)
    key = (tables, 0)
    assert torch.cuda.current_device() == 0 and key not in grid._axes
    side = _warmed_stream(want)
    through, settled = [], grid._settled
    grid._settled = lambda k, *rest: (through.append(k), settled(k, *rest))[1]
    with G.Gate(side=side) as gate:
        ctx = T_context()
        got = grid.device_corners(ctx) if tables == 'corners' else grid.device_centers(ctx)
        open_on_return = gate.opened.query()
    side.synchronize()
    host = [t.cpu().numpy() for t in got]
    torch.cuda.synchronize()
    T_context()
    assert through == [key] and grid._axes[key] is got
    assert open_on_return, 'the tables were kept while their upload was still waiting behind the gate (%.0f ms)' % gate.ms
    for g, w in zip(host, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes()


def test_shared_grid_tables():
    import torch
    from auromat_amd import resample as R
    G.cycles_per_ms()                               # (calibrated here: it synchronises the device, which no thread may)
    box = shared_box()
    m0 = mapping('iss030')
    want = [of_dict(fn()) for _, fn in shared_calls(m0, box)]
    ms = []
    for _, fn in shared_calls(m0, box):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    print('nearest, mean, gather on the 8 x 8 deg grid alone on the main thread: %s ms of host time' % ', '.join('%.1f' % v for v in ms))
    assert (~want[0]['mask']).sum() > 100 and (~want[1]['mask']).sum() > 100 and (~want[2]['mask']).sum() > 100
    lat, _ = shared_grid(box).device_corners(T_context())
    assert lat.numel() * lat.element_size() >= 1 << 20, ('the corner tables are below the size of the staged upload', tuple(lat.shape))
    # the grid and its device tables are made again, by the threads: that is what is tested
    R._GRID_CACHE.clear()
    gate_ms = G.gate_ms_for(sum(ms))
    sync = T.Barriers()
    identity = Identity(sync)
    inside = sync.event()
    grids = [None, None]

    def thread(t):
        def fn(ctx, stream):
            identity.check(t, ctx)
            calls = shared_calls(mapping('iss030'), box)      # (the mapping's arrays exist and are settled: frame() reads its box back)
            stream.synchronize()
            if t == 0:
                T.StreamGate(gate_ms)
                inside.set()
                t0 = time.perf_counter()
                # the first thing outside_outline_mask does with the grid, ahead of its own small (blocking) upload: the corner
                # tables go up on this thread's held stream.  Kept in the cache at once, they would be what B finds.
                shared_grid(box).device_corners(ctx)
            else:
                T.wait_event(inside)
                time.sleep(0.005)
                t0 = time.perf_counter()
            for (name, call_), w in zip(calls, want):
                assert_same(of_dict(call_()), w, ('thread %d' % t, name))
            grids[t] = shared_grid(box)
            return t0, time.perf_counter()
        return fn

    (a0, a1), (b0, b1) = T.run_threads([thread(0), thread(1)], sync=sync)
    print('A held for %.0f ms (gate %.0f ms); B started %.1f ms after A and took %.1f ms' % ((a1 - a0) * 1e3, gate_ms, (b0 - a0) * 1e3,
                                                                                       (b1 - b0) * 1e3))
    assert grids[0] is grids[1], 'the two threads did not share the cached grid'
    assert a0 < b0 < a1, ('thread B did not start while A was held: nothing was proved', (b0 - a0) * 1e3, (a1 - a0) * 1e3)


def T_context():
    from auromat_amd._native import Context
    return Context.current()


# ---- pipelines that change hands ---------------------------------------------------------------------------------------------------

def test_handed_over_pipelines():
    from auromat_amd.pipeline import FramePipeline, SequencePipeline
    cases = dict((c.name, c) for c in K.build() if c.name in ('pipeline_run_dirs', 'sequence_pipeline'))
    T.baselines(cases.values())                          # (with pipelines of the cases' own, on the main thread)
    frame_pipe = FramePipeline(K.W, K.H, alloc_image=False)
    seq = SequencePipeline(K.RW, K.RH, pxPerDeg=K.PX_PER_DEG, min_elevation=K.MIN_ELEV, own_image_buffers=False)
    main_ctx = T_context()
    assert frame_pipe.ctx is main_ctx and seq.ctx is main_ctx

    def call_pipeline_run(env):
        """K._call_pipeline_run with the pipeline that was built on the main thread"""
        pipe = frame_pipe
        pipe.use_image(env.inp['img0'])
        res = pipe.run(None, K.ALTITUDE, None, None, fast=True, min_elevation=K.MIN_ELEV, pxPerDeg=K.PX_PER_DEG, params=K._params(),
                       keep_on_device=True, fuse=True, dirs=env.inp['dirs'], containsPole=False)
        n = res['mean'].shape[0] * res['mean'].shape[1]
        assert n <= K.CELLS_CAP
        for k, width in (('mean', 4), ('img', 3)):
            env.out[k][:n].copy_(res[k].reshape(n, width))
        for k in ('mask', 'count'):
            env.out[k][:n].copy_(res[k].reshape(n))
        values = dict(plan=pipe.last_plan, retried=bool(pipe._fused.get('retried')), shape=tuple(res['mean'].shape))
        assert values['plan'] == 'single-pass' and not values['retried'], values
        return values

    c = cases['pipeline_run_dirs']
    handed = G.Case(c.name, c.family, c.inputs, c.outputs, call_pipeline_run, c.oracle, synchronises=True, harmless=c.harmless)

    def worker(ctx, stream):
        assert ctx is not main_ctx and ctx.handle.value != main_ctx.handle.value
        G.run_gated(handed)
        K._kept[K._key('seq', ctx)] = seq                # what K._call_sequence_pipeline uses on this thread's context
        G.run_gated(cases['sequence_pipeline'])
        assert K._kept[K._key('seq', ctx)] is seq

    T.run_threads([worker])


def test_two_sequence_pipelines_at_once():
    case, = [c for c in K.build() if c.name == 'sequence_pipeline']
    T.baselines([case])
    sync = T.Barriers()
    start = sync.barrier(2)
    seqs = [None, None]

    def thread(t):
        def fn(ctx, stream):
            start.wait()
            got, extra, _ = T.run_case_settled(case, ctx)
            seqs[t] = K._kept[K._key('seq', ctx)]
            T.assert_baseline(case, got, extra, 'thread %d' % t)
        return fn

    T.run_threads([thread(0), thread(1)], sync=sync)
    assert seqs[0] is not seqs[1] and seqs[0].ctx.handle.value != seqs[1].ctx.handle.value
    assert seqs[0].s_main is seqs[1].s_main, 'the streams of the sequence pipelines are per process (pipeline._STREAMS)'
