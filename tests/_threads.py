"""
TEST INFRASTRUCTURE — the library from several host threads at once, one context each.

include/auromat_hip.h: "the library keeps no global state and contexts may be used from different threads (one thread per
context at a time)".  The Python layer gives every host thread a context of its own (Context.current keys its cache by process,
thread and device) and ctypes releases the interpreter lock during every call, so two Python threads really are inside the
library at the same time.

  threads   run_threads(fns) starts one daemon thread per function, four at the most, all in this process (one process has the
            GPU open).  Every thread makes a torch.cuda.Stream of its own and keeps it current for everything it does, takes
            Context.current() on it and synchronises only that stream, never the device; its last statement is one more
            synchronisation of that stream.  Before any thread does its work the contexts' handles must differ pairwise.
  results   what a thread computes is compared with the bytes and host values of G.baseline(case), the run of the case alone
            on the main thread that tests/test_gated_cases_cpu.py ties to the CPU oracles; the baselines are computed before
            the first thread starts.
  errors    a thread's exception is kept and the first one (a broken barrier last: it only follows another thread's failure)
            is raised again in the calling thread; the barriers a schedule uses are aborted when a thread fails, so that the
            others do not wait for it.
  hangs     a thread that is still alive at the limit (60 s, far above the few seconds of a pass) marks the session as hung:
            every later test of the thread modules then fails at once (fail_if_hung, an autouse fixture there) without
            touching the GPU.
"""
import threading
import time
from collections import OrderedDict

import numpy as np

import _gated_stream as G

LIMIT_S = 60.0
MAX_THREADS = 4
_state = {'hung': None}


def fail_if_hung():
    assert _state['hung'] is None, 'an earlier test left a thread hanging (%s): nothing more is started on the GPU' % _state['hung']


class Barriers(object):
    """the barriers and events of one schedule: all of them give way when a thread fails"""

    def __init__(self):
        self.items = []

    def barrier(self, n):
        b = threading.Barrier(n, timeout=LIMIT_S)
        self.items.append(b)
        return b

    def event(self):
        e = threading.Event()
        self.items.append(e)
        return e

    def abort(self):
        for b in self.items:
            b.abort() if isinstance(b, threading.Barrier) else b.set()


def wait_event(event):
    assert event.wait(LIMIT_S), 'the other thread never got there'


def run_threads(fns, limit_s=LIMIT_S, sync=None):
    """Run fns[t](ctx, stream) on a thread each -> the list of their results.  `sync`: the Barriers of the schedule."""
    import torch
    from auromat_amd._native import Context
    fail_if_hung()
    n = len(fns)
    assert 1 <= n <= MAX_THREADS
    sync = sync or Barriers()
    lined_up = sync.barrier(n)
    handles, results, errors = [None] * n, [None] * n, [None] * n

    def body(t):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                ctx = Context.current()
                handles[t] = ctx.handle.value
                lined_up.wait()
                assert len(set(handles)) == n, ('host threads share a context', handles)
                try:
                    results[t] = fns[t](ctx, stream)
                finally:
                    stream.synchronize()
        except BaseException as e:                       # noqa: B902 (kept and raised again in the calling thread)
            errors[t] = e
            sync.abort()

    threads = [threading.Thread(target=body, args=(t,), daemon=True, name='amt-test-%d' % t) for t in range(n)]
    deadline = time.monotonic() + limit_s
    for th in threads:
        th.start()
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    alive = [th.name for th in threads if th.is_alive()]
    if alive:
        _state['hung'] = ', '.join(alive)
        sync.abort()
        raise AssertionError('threads still alive after %.0f s: %s' % (limit_s, _state['hung']))
    first = sorted((isinstance(e, threading.BrokenBarrierError), t) for t, e in enumerate(errors) if e is not None)
    if first:
        raise errors[first[0][1]]
    return results


# ---- one case of tests/_gated_cases.py on the calling thread's stream ----------------------------------------------------------

def run_case_settled(case, ctx=None):
    """G.baseline's body for one run on the calling thread's current stream: true inputs, fresh poisoned outputs, that stream
    synchronised before and after -> (output bytes, host values, (start, end) of the call by time.perf_counter)."""
    import torch
    from auromat_amd._native import Context
    stream = torch.cuda.current_stream()
    inp = OrderedDict((k, G.dev(t)) for k, (t, _) in case.inputs.items())
    raw, out = G._fresh_outputs(case)
    stream.synchronize()
    env = G.Env(Context.current(), inp, out)             # (a case may have left the context on a stream of its own)
    assert ctx is None or env.ctx is ctx, 'the calling thread has another context than the one it was given'
    t0 = time.perf_counter()
    extra = case.call(env)
    t1 = time.perf_counter()
    stream.synchronize()
    return OrderedDict((k, bits(raw[k], case, k)) for k in raw), extra, (t0, t1)


def bits(t, case, k):
    return G.bits(t, case.canonical.get(k))


def assert_baseline(case, got, extra, who=''):
    """the bytes and host values of a run against G.baseline(case) (computed on the main thread before the threads start)"""
    want, want_extra, _ = G._state[('baseline', case.name)]
    assert extra == want_extra, (who, case.name, 'host values', extra, want_extra)
    for k in want:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (who, case.name, k, 'other bytes than the single-thread baseline', bad.size, bad[:8])


def baselines(cases):
    """every baseline and the gate's calibration, on the calling (main) thread: both synchronise the device"""
    G.cycles_per_ms()
    for c in cases:
        G.baseline(c)


class StreamGate(object):
    """G.Gate for a thread: a sleep of `ms` and the event `opened` on the CURRENT stream, without the device synchronisation
    of G.Gate (the other threads' streams are none of this thread's business)."""

    def __init__(self, ms):
        import torch
        # (the calibration synchronises the device: the main thread makes it, G.cycles_per_ms(), before the threads start)
        assert 'cycles_per_ms' in G._state, 'G.cycles_per_ms() has to be called on the main thread before a thread opens a gate'
        self.ms = ms
        torch.cuda.current_stream().synchronize()
        torch.cuda._sleep(int(G.cycles_per_ms() * ms))
        self.opened = torch.cuda.Event()
        self.opened.record()
