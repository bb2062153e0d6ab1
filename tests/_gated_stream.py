"""
TEST INFRASTRUCTURE — the gated side stream: calls of the library whose device inputs do not exist yet when the call is made.

Every GPU test but this family calls the library on torch's default stream with inputs that are settled, and reads results
after a host synchronisation; a kernel, memset or copy issued on another stream than the context's, a missing event wait or a
result written on the wrong stream cannot be seen that way.  Here a call is made on a side stream that is held up by a GATE, a
spinning kernel (torch.cuda._sleep) of a calibrated length:

  inputs    every device input exists twice, TRUE and DECOY (same shape and dtype).  The buffer the call reads holds the decoy,
            settled; behind the gate, on the side stream, a device-to-device copy from a settled staging tensor replaces it by
            the true values.  Work of the library that is not ordered behind the side stream reads the decoy.
  outputs   poisoned (0xA5 bytes) and settled before the gate.  Right after the call `snap = out.clone()` is enqueued on the
            side stream — an ordered consumer without host synchronisation; after side.synchronize() the snapshot, and after
            torch.cuda.synchronize() the buffer itself, must equal the BASELINE as bytes.
  baseline  the same call on the default stream with settled true inputs, fresh poisoned outputs and a full synchronisation
            before and after; made twice (the entry points are deterministic: both runs must agree), the second one timed on
            the host.
  gate      100 ms, or 4 x the host time of the call on settled inputs where that is more (calls that do host work first),
            2 s at the most: always finite, a call that synchronises inside just waits for it.
  warm-up   the library's scratch memory is kept per stream and growing it synchronises: before the gate the case runs once on
            the side stream with settled inputs (and must give the baseline's bytes there too).
  power     a case calls env.closed() after every call the header does not mark "synchronises": the gate's event must not
            have completed by then (otherwise the case proved nothing and fails).  Cases without such a call say so
            (synchronises=True).

Decoys are harmless by construction (tests/_gated_cases.py states it per case, tests/test_gated_cases_cpu.py checks it): a
kernel that reads a decoy computes wrong values, never an address out of range.
"""
import time
from collections import OrderedDict

import numpy as np

POISON = 0xA5
GATE_MS = 100.0
GATE_CAP_MS = 2000.0
_CALIBRATION_CYCLES = 2000000

_state = {}


class Case(object):
    """
    name, family   the id of the case and the letter of its family (A context-stream calls, B host tables, ...)
    inputs         OrderedDict name -> (true, decoy): host arrays of one shape and dtype
    outputs        OrderedDict name -> (shape, dtype)
    call(env)      makes the library calls with env.inp[name] / env.out[name] (device tensors), env.ctx; calls env.closed()
                   after each call that must not synchronise; may return a dict of host values (statuses, grids) that must
                   equal the baseline's too
    oracle(arrays) the CPU oracle on a dict name -> host array of the inputs -> dict of compared outputs (None: exempt)
    index_ranges   name -> (low, high): inputs a kernel uses as index, offset or count, with the half-open range every element
                   of the true array and of the decoy has to lie in
    harmless       why the case cannot fault when the library ignores the gate
    out_fill       name -> host array: what an output holds before the gate instead of poison (a buffer that a later call of
                   the case reads as an index has to be in range whenever it is read)
    canonical      name -> function of the output's bytes (uint8 array) -> the array that is compared (records the library
                   writes in no particular order are sorted first)
    """

    def __init__(self, name, family, inputs, outputs, call, oracle=None, synchronises=False, index_ranges=None, harmless='',
                 out_fill=None, canonical=None):
        self.name, self.family = name, family
        self.inputs, self.outputs = OrderedDict(inputs), OrderedDict(outputs)
        self.call, self.oracle, self.synchronises = call, oracle, synchronises
        self.index_ranges = dict(index_ranges or {})
        self.harmless = harmless
        self.out_fill, self.canonical = dict(out_fill or {}), dict(canonical or {})
        for k, (t, d) in self.inputs.items():
            assert t.shape == d.shape and t.dtype == d.dtype, (name, k)

    def __repr__(self):
        return self.name


class Env(object):
    def __init__(self, ctx, inp, out, opened=None):
        self.ctx, self.inp, self.out, self.opened = ctx, inp, out, opened
        self.checks = 0
        self.open_early = []

    def closed(self, what=''):
        """After a call that must not synchronise: the gate has to be closed still."""
        self.checks += 1
        if self.opened is not None and self.opened.query():
            self.open_early.append(what or 'call %d' % self.checks)


# ---- device arrays ---------------------------------------------------------------------------------------------------------

def dev(a):
    """host array -> settled device tensor of the same bytes (uint16 as int16, bool as uint8)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.bool_:
        a = a.view(np.uint8)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def poisoned(shape, dtype):
    import torch
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return torch.full((n,), POISON, dtype=torch.uint8, device='cuda')


def typed(t, shape, dtype):
    """a poisoned byte tensor as a tensor of `dtype` and `shape` (unsigned types as their signed twins)"""
    import torch
    twin = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8,
            np.dtype(np.int16): torch.int16, np.dtype(np.uint16): torch.int16, np.dtype(np.int32): torch.int32,
            np.dtype(np.uint32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint64): torch.int64}[np.dtype(dtype)]
    return t.view(twin).view(tuple(shape))


def bits(t, canonical=None):
    import torch
    b = t.contiguous().view(-1).view(torch.uint8).cpu().numpy()
    return b if canonical is None else np.ascontiguousarray(canonical(b)).view(np.uint8).reshape(-1)


# ---- the gate ---------------------------------------------------------------------------------------------------------------

def cycles_per_ms():
    """torch.cuda._sleep counts of one millisecond: one _sleep of a fixed count between two events on an idle stream, once per
    session (it measures the delay, not code under test)."""
    import torch
    if 'cycles_per_ms' not in _state:
        torch.cuda.synchronize()
        torch.cuda._sleep(1000)                       # loads the kernel
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(_CALIBRATION_CYCLES)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.05, ('the calibration sleep is too short to be timed', ms)
        _state['cycles_per_ms'] = _CALIBRATION_CYCLES / ms
        print('gate calibration: %d counts of torch.cuda._sleep took %.3f ms' % (_CALIBRATION_CYCLES, ms))
    return _state['cycles_per_ms']


def gate_ms_for(host_ms):
    return min(GATE_CAP_MS, max(GATE_MS, 4.0 * host_ms))


class Gate(object):
    """`with Gate(ms) as g:` — a fresh side stream, made current, that starts with a sleep of `ms` and the event g.opened."""

    def __init__(self, ms=GATE_MS, side=None):
        import torch
        self.ms = ms
        self.cycles = int(cycles_per_ms() * ms)
        self.side = torch.cuda.Stream() if side is None else side
        self.opened = torch.cuda.Event()
        self._cm = None

    def __enter__(self):
        import torch
        torch.cuda.synchronize()
        self._cm = torch.cuda.stream(self.side)
        self._cm.__enter__()
        torch.cuda._sleep(self.cycles)
        self.opened.record(self.side)
        return self

    def __exit__(self, *exc):
        return self._cm.__exit__(*exc)


# ---- one case ---------------------------------------------------------------------------------------------------------------

def _context():
    from auromat_amd._native import Context
    return Context.current()


def _fresh_outputs(case):
    import torch
    raw = OrderedDict((k, poisoned(shape, dtype)) for k, (shape, dtype) in case.outputs.items())
    for k, a in case.out_fill.items():
        raw[k].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
    return raw, OrderedDict((k, typed(raw[k], *case.outputs[k])) for k in raw)


def baseline(case):
    """(output bytes, host values, host milliseconds of the call) on the default stream with settled true inputs"""
    import torch
    key = ('baseline', case.name)
    if key in _state:
        return _state[key]
    runs = []
    for rep in range(2):
        inp = OrderedDict((k, dev(t)) for k, (t, _) in case.inputs.items())
        raw, out = _fresh_outputs(case)
        torch.cuda.synchronize()
        env = Env(_context(), inp, out)
        t0 = time.perf_counter()
        extra = case.call(env)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        runs.append((OrderedDict((k, bits(v, case.canonical.get(k))) for k, v in raw.items()), extra, host_ms))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), (case.name, k, 'two settled runs differ: the call is not deterministic')
    assert runs[0][1] == runs[1][1], (case.name, 'host values of two settled runs differ')
    for k, v in runs[1][0].items():
        assert k in case.out_fill or (v != POISON).any(), (case.name, k, 'the settled call left the output untouched')
        v.setflags(write=False)
    print('%s: host time of the call on settled inputs %.2f ms' % (case.name, runs[1][2]))
    _state[key] = runs[1]
    return _state[key]


def run_gated(case):
    """The case behind a gate: asserts what the module docstring says."""
    import torch
    want, want_extra, host_ms = baseline(case)
    # The library keeps its scratch memory per stream, and "a call that needs a larger workspace than the stream has grows it,
    # which synchronises that stream once, as for every user of the workspace" (include/auromat_hip.h): the side stream gets its
    # workspace from one call on settled inputs before the gate — which must give the baseline's bytes as well.
    side = torch.cuda.Stream()
    warm_inp = OrderedDict((k, dev(t)) for k, (t, _) in case.inputs.items())
    warm_raw, warm_out = _fresh_outputs(case)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        warm_extra = case.call(Env(_context(), warm_inp, warm_out))
    torch.cuda.synchronize()
    assert warm_extra == want_extra, (case.name, 'host values of the settled call on the side stream', warm_extra, want_extra)
    for k in want:
        assert np.array_equal(bits(warm_raw[k], case.canonical.get(k)), want[k]), (case.name, k, 'the settled call on the side stream')
    inp = OrderedDict((k, dev(d)) for k, (_, d) in case.inputs.items())
    staging = OrderedDict((k, dev(t)) for k, (t, _) in case.inputs.items())
    raw, out = _fresh_outputs(case)
    with Gate(gate_ms_for(host_ms), side) as gate:
        for k in inp:
            inp[k].copy_(staging[k])
        env = Env(_context(), inp, out, gate.opened)
        extra = case.call(env)
        snap = OrderedDict((k, v.clone()) for k, v in raw.items())
    gate.side.synchronize()
    got_snap = OrderedDict((k, bits(v, case.canonical.get(k))) for k, v in snap.items())
    torch.cuda.synchronize()
    got = OrderedDict((k, bits(v, case.canonical.get(k))) for k, v in raw.items())
    _context()                                        # the library follows torch back to the default stream
    assert case.synchronises or env.checks > 0, (case.name, 'a case that does not synchronise has to check the gate')
    assert not env.open_early, (case.name, 'the gate (%.0f ms) was open already after' % gate.ms, env.open_early)
    assert extra == want_extra, (case.name, 'host values', extra, want_extra)
    for k in want:
        bad = np.flatnonzero(got_snap[k] != want[k])
        assert bad.size == 0, (case.name, k, 'the consumer on the side stream saw other bytes than the baseline', bad.size, bad[:8])
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (case.name, k, 'the buffer holds other bytes than the baseline', bad.size, bad[:8])
