"""
The C ABI from several host threads at once, one context and one stream each (tests/_threads.py): every case of
tests/_gated_cases.py — each family of entry points — while other threads are inside the library, compared as bytes with the
case's run alone on the main thread.  include/auromat_hip.h promises that "the library keeps no global state and contexts may be
used from different threads (one thread per context at a time)"; a mutable global of the library (a shared workspace, a
table filled on first use, the copier's pool), a kernel or copy on the NULL stream, or a result written through another
context's buffers shows as other bytes than the baseline, as a host value that differs, or as an error code.

  held call      thread A makes the calls of one case behind a gate on its stream (decoy inputs, the true values arrive behind
                 the gate, as in G.run_gated), sets an event and enters amt_ctx_synchronize: it sits inside the library, the
                 interpreter lock released, until its stream has run dry.  Thread B then runs the whole table once on its own
                 context and stream.  B's first call must start while A is inside amt_ctx_synchronize (time.perf_counter on
                 both sides), otherwise the test proved nothing and fails.  A case whose own calls wait for the gate
                 (amt_pipe_wait in camera_path_many, the third amt_run_push in run_device_images) returns with the gate open:
                 A then queues a second sleep of the gate's length before its snapshot, so that amt_ctx_synchronize has
                 something to wait for in those cases too.  Would catch: state shared between two contexts that a call of B
                 changes while A's kernels have not run yet (A's results then differ from the baseline), a device-wide
                 synchronisation inside a call of B (B's first call would only return when A's gate opens — B still passes, but
                 the count of B's cases inside the window drops to 1).
  free running   2 and 4 threads, a barrier before every case, one pass: (a) thread t takes the table rotated by t * len / n,
                 so that different kernels and different workspace growths (hipMalloc / hipFree) meet at each barrier; (b) all
                 threads run the same case at each barrier.  No warm-up.  Would catch: races in first-use initialisation,
                 allocation from several threads, kept objects shared by contexts.
  staged copies  amt_upload_staged / amt_download_staged from two threads at once, each context with its own copier and pool of
                 page-locked pieces: 1 byte, 4 MiB - 1, 8 MiB + 1.  Would catch: pieces handed to the wrong copier, a pool
                 shared without a lock.

The gate of the held call is G.gate_ms_for (four times, 100 ms at least, 2 s at most) of the host time of B's whole list,
measured in one settled single-thread pass on the main thread before the gate (printed with -s).

Measured on an MI355X with GPU_MAX_HW_QUEUES=4: one settled pass over the 32 cases (inputs, calls, read-back, comparison) takes
92.7 ms of host time on the main thread, so the gate is 371 ms.  A sat inside amt_ctx_synchronize for 353 ms (masks), 363 ms
(mosaic), 360 ms (median_frame_async), 383 ms (camera_path_many) and 361 ms (run_device_images; the last two with the second
sleep behind the case), and in every one of the five 29 of B's 32 cases started inside that window, every case equal to the
baseline.  The 29th, pipeline_run_dirs, is where B stops until A's gate opens: it builds a FramePipeline and its driver per
call and frees the one before; something of that waits for the whole device, other threads' held streams included (supposed,
not shown: hipFree and hipHostFree synchronise the device, and so may the page-locked allocations) — a cost of building and
freeing pipelines, seen again in tests/test_gpu_threads_classes.py, not an error in any result.  All 12 tests take 6.8 s
together, the baselines included.
"""
import ctypes as C
import time
from collections import OrderedDict

import numpy as np
import pytest

import _gated_cases as K
import _gated_stream as G
import _threads as T

pytestmark = pytest.mark.gpu

CASES = K.build()
BY_NAME = dict((c.name, c) for c in CASES)
HELD = ['masks', 'mosaic', 'median_frame_async', 'camera_path_many', 'run_device_images']      # one of each family A to E
_list_ms = {}


@pytest.fixture(scope='module', autouse=True)
def _baselines_and_release():
    T.fail_if_hung()
    T.baselines(CASES)
    yield
    if T._state['hung'] is None:
        K.release()


@pytest.fixture(autouse=True)
def _not_hung():
    T.fail_if_hung()


def whole_table(who, cases=CASES):
    """every case once on the calling thread's context and stream, each compared with the baseline -> the calls' start times"""
    starts = []
    for case in cases:
        got, extra, (t0, _) = T.run_case_settled(case)
        T.assert_baseline(case, got, extra, who)
        starts.append(t0)
    return starts


def list_host_ms():
    """host time of one settled pass over the table on the main thread (what thread B does while A is held)"""
    if 'ms' not in _list_ms:
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        whole_table('main thread')
        _list_ms['ms'] = (time.perf_counter() - t0) * 1e3
        print('one settled pass over the %d cases on the main thread: %.1f ms of host time' % (len(CASES), _list_ms['ms']))
    return _list_ms['ms']


@pytest.mark.parametrize('name', HELD)
def test_whole_table_while_another_thread_is_held_inside_the_library(name):
    import torch
    case = BY_NAME[name]
    gate_ms = G.gate_ms_for(list_host_ms())
    want, want_extra, _ = G.baseline(case)
    sync = T.Barriers()
    inside = sync.event()

    def thread_a(ctx, stream):
        inp = OrderedDict((k, G.dev(d)) for k, (_, d) in case.inputs.items())
        staging = OrderedDict((k, G.dev(t)) for k, (t, _) in case.inputs.items())
        raw, out = G._fresh_outputs(case)
        gate = T.StreamGate(gate_ms)
        for k in inp:
            inp[k].copy_(staging[k])
        extra = case.call(G.Env(ctx, inp, out))
        second = gate.opened.query()                     # the case's own calls waited for the gate: hold the stream once more
        if second:
            torch.cuda._sleep(int(G.cycles_per_ms() * gate_ms))
        snap = OrderedDict((k, v.clone()) for k, v in raw.items())
        ctx.bind()
        inside.set()
        t_in = time.perf_counter()
        ctx.synchronize()                                # amt_ctx_synchronize: inside the library until the stream has run dry
        t_out = time.perf_counter()
        got_snap = OrderedDict((k, T.bits(v, case, k)) for k, v in snap.items())
        got = OrderedDict((k, T.bits(v, case, k)) for k, v in raw.items())
        return dict(extra=extra, snap=got_snap, buf=got, window=(t_in, t_out), second=second)

    def thread_b(ctx, stream):
        T.wait_event(inside)
        time.sleep(0.005)
        return whole_table('thread B')

    a, starts = T.run_threads([thread_a, thread_b], sync=sync)
    t_in, t_out = a['window']
    n_inside = sum(t_in < t < t_out for t in starts)
    print('%s held for %.0f ms (gate %.0f ms%s): %d of B\'s %d cases started inside amt_ctx_synchronize of A'
          % (name, (t_out - t_in) * 1e3, gate_ms, ', a second one behind the case' if a['second'] else '', n_inside, len(starts)))
    assert a['extra'] == want_extra, (name, 'host values of the held call', a['extra'], want_extra)
    for k in want:
        for what in ('snap', 'buf'):
            bad = np.flatnonzero(a[what][k] != want[k])
            assert bad.size == 0, (name, k, what, 'the held thread saw other bytes than the baseline', bad.size, bad[:8])
    assert t_in < starts[0] < t_out, ('thread B did not start while A was inside the library: nothing was proved',
                                      (starts[0] - t_in) * 1e3, (t_out - t_in) * 1e3)


@pytest.mark.parametrize('schedule', ['rotated', 'same'])
@pytest.mark.parametrize('n', [2, 4])
def test_free_running_threads(n, schedule):
    sync = T.Barriers()
    steps = [sync.barrier(n) for _ in CASES]

    def thread(t):
        first = (t * len(CASES)) // n if schedule == 'rotated' else 0
        order = CASES[first:] + CASES[:first]

        def fn(ctx, stream):
            for step, case in zip(steps, order):
                step.wait()
                got, extra, _ = T.run_case_settled(case, ctx)
                T.assert_baseline(case, got, extra, 'thread %d of %d' % (t, n))
        return fn

    T.run_threads([thread(t) for t in range(n)], sync=sync)


# ---- staged copies ---------------------------------------------------------------------------------------------------------------

PIECE = 4 << 20                                 # AMT_COPY_PIECE_MB: the size of a piece of the copier
SIZES = [1, PIECE - 1, 2 * PIECE + 1]


@pytest.mark.parametrize('size', SIZES)
def test_staged_copies_from_two_threads(size):
    """each thread: its own bytes up through amt_upload_staged, a copy on its stream, and down through amt_download_staged"""
    import torch
    sync = T.Barriers()
    up, down = sync.barrier(2), sync.barrier(2)

    def thread(t):
        src = np.random.RandomState(70 + t).randint(0, 256, size).astype(np.uint8)

        def fn(ctx, stream):
            dst = torch.full((size,), G.POISON, dtype=torch.uint8, device='cuda')
            host = np.full(size, G.POISON, dtype=np.uint8)
            stream.synchronize()
            up.wait()
            ctx.call('amt_upload_staged', C.c_void_p(dst.data_ptr()), C.c_void_p(src.ctypes.data), size)
            copy = dst.clone()                          # ordered behind the upload on this thread's stream
            down.wait()
            ctx.call('amt_download_staged', C.c_void_p(host.ctypes.data), C.c_void_p(copy.data_ptr()), size)
            assert np.array_equal(host, src), ('thread', t, 'bytes changed on the way', int((host != src).sum()))
            assert np.array_equal(dst.cpu().numpy(), src), ('thread', t, 'the uploaded buffer')
        return fn

    T.run_threads([thread(0), thread(1)], sync=sync)
