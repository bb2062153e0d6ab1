"""
The library's scratch memory (amt_workspace, auromat_amd/csrc/amt_common.h: one grow-only buffer per stream of a context, 1 MiB
at least, at most 16 streams) in the states a real sequence puts it into and the rest of the suite never does: a result must
not depend on what the context ran before.  Every user of the buffer (tests/_scratch_cases.py: one case at least per call site
of amt_workspace) is compared, as bytes, with its own baseline — the same call on settled inputs, made twice
(tests/_gated_stream.py: baseline) — while the buffer, reached through the debugging hook amt_debug_scratch_info / _fill /
_release (include/auromat_hip.h), is

  a. freshly allocated, then filled with 0xFF (counters at their maximum, doubles NaN, flags set) and with 0x5A: a region that a
     call reads before it has written it shows as other bytes.  The audit in DESIGN.md ("Scratch memory: who writes what before it
     is read") says for every region which memset, copy or kernel writes it first; it was made before the first poisoned run,
     because a poisoned cursor or table entry is an address out of range;
  b. left behind by every other user: each ordered pair (A, B) on one stream without a release in between, and A again;
  c. grown inside a call while the call before it is still pending on the stream (the old buffer is freed: the free has to
     wait), without a change to another stream's buffer;
  d. one of two buffers of one context: distinct, disjoint, and filling one leaves a call on the other alone;
  e. evicted as the least recently used of 17 streams while a call on its stream is still held behind a gate;
  f. released: the next call starts from a fresh allocation.

Whether a case is a user is decided at run time: the context's count of requests advances during its call.  The cases the
registry adds have to satisfy their CPU oracles once as well (the gather mosaics, which have none: the composition of the
device's own per-member and per-point results, as tests/test_gpu_gather_mosaic_cells.py and _supersample_cells.py do).

Out of scope: streams that their owner destroys while the context still lists them (amt_workspace comments on it; a test could
only provoke an error); the buffers the pipelines and the runner own themselves (tail->partials, slots, arenas, and the buffer
the frame driver's pre-pass gets on the driver's own stream: the sky-fill and driver-state tests); LDS; a second GPU.

No read before write was found, by the audit or by these tests.  Measured on an MI355X: the 86 tests of this file take 5 s
together, the slowest (the eviction, whose gate is 100 ms) 0.11 s.  Case names are kept apart from every other module's:
baselines are remembered by name for the session.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

import _gated_cases as K
import _gated_stream as G
import _scratch_cases as S

pytestmark = pytest.mark.gpu

ALL = S.build()
BY = OrderedDict((c.name, c) for c in ALL)
ADDED = S.added()
LARGE = S.large()
PENDING = 'area_frame_async'                     # a user that only enqueues work
SMALL = 'median_frame_async'                     # another one
HOLD_MS = 50.0                                   # how long a stream is held so that the call before a growth is still pending
_user = {}


@pytest.fixture(scope='module', autouse=True)
def _release_what_the_cases_keep():
    yield
    K.release()


# ---- the hook -----------------------------------------------------------------------------------------------------------------

def info():
    """the scratch buffer of torch's current stream: dict(bytes, ptr, streams, requests)"""
    b, p, s, r = C.c_size_t(), C.c_void_p(), C.c_int32(), C.c_uint64()
    G._context().call('amt_debug_scratch_info', C.byref(b), C.byref(p), C.byref(s), C.byref(r))
    return dict(bytes=b.value, ptr=p.value or 0, streams=s.value, requests=r.value)


def fill(byte, at_least=0):
    G._context().call('amt_debug_scratch_fill', at_least, byte)


def release():
    G._context().call('amt_debug_scratch_release')


# ---- a case on torch's current stream ---------------------------------------------------------------------------------------------

def prepare(case, n=1):
    """n sets of settled true inputs and fresh poisoned outputs (synchronises the device)"""
    import torch
    sets = []
    for _ in range(n):
        inp = OrderedDict((k, G.dev(t)) for k, (t, _d) in case.inputs.items())
        raw, out = G._fresh_outputs(case)
        sets.append((inp, raw, out))
    torch.cuda.synchronize()
    return sets if n > 1 else sets[0]


def call(case, prepared):
    """the calls of the case on torch's current stream; synchronises only where the case does"""
    inp, raw, out = prepared
    return case.call(G.Env(G._context(), inp, out))


def read(case, prepared):
    import torch
    torch.cuda.synchronize()
    return OrderedDict((k, G.bits(v, case.canonical.get(k))) for k, v in prepared[1].items())


def check(case, got, extra, what):
    want, want_extra, _ = G.baseline(case)
    assert extra == want_extra, (case.name, what, 'host values', extra, want_extra)
    for k in want:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (case.name, what, k, 'other bytes than the baseline', bad.size, bad[:8])


def run(case, what):
    p = prepare(case)
    extra = call(case, p)
    check(case, read(case, p), extra, what)


def is_user(case):
    """does the context's count of requests advance during the case's call (from a released buffer)?"""
    if case.name not in _user:
        G.baseline(case)
        release()
        before = info()['requests']
        run(case, 'a fresh allocation')
        _user[case.name] = info()['requests'] > before
    return _user[case.name]


def streams(n):
    """n distinct side streams, none of them the default stream (torch hands its pooled streams out again and again)"""
    import torch
    seen, out = {torch.cuda.default_stream().cuda_stream}, []
    for _ in range(256):
        s = torch.cuda.Stream()
        if s.cuda_stream not in seen:
            seen.add(s.cuda_stream)
            out.append(s)
        if len(out) == n:
            return out
    raise AssertionError('torch did not hand out %d distinct streams' % n)


def on(stream):
    import torch
    return torch.cuda.stream(stream)


def back_to_default():
    import torch
    torch.cuda.synchronize()
    G._context()                                     # the library follows torch back to the default stream


# ---- the added cases and their oracles --------------------------------------------------------------------------------------------

def arrays(case, got):
    return dict((k, np.ascontiguousarray(got[k]).view(np.dtype(dtype)).reshape(shape)) for k, (shape, dtype) in case.outputs.items())


def same_values(got, want, what):
    want = np.asarray(want)
    if got.dtype == np.uint8 and want.dtype != np.uint8:
        want = (want != 0).astype(np.uint8)
    assert got.shape == want.shape or got.size == want.size, (what, got.shape, want.shape)
    want = want.reshape(got.shape)
    if got.dtype.kind == 'f':
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, 'NaN in other places')
        assert np.array_equal(got[~nan].view(np.uint64), want[~nan].astype(np.float64).view(np.uint64)), (what, 'other bits')
    else:
        assert np.array_equal(got, want.astype(got.dtype)), what


@pytest.mark.parametrize('case', [c for c in ADDED if c.oracle is not None], ids=[c.name for c in ADDED if c.oracle is not None])
def test_added_case_satisfies_its_oracle(case):
    got = arrays(case, G.baseline(case)[0])
    want = case.oracle({k: v[0] for k, v in case.inputs.items()})
    assert set(want) == set(got)
    if case.name == 'coarse_bbox_dirs':
        # corner counts and the hint exactly; the box to the 1e-6 degrees the frame kernels promise (auromat_amd/csrc/amt_common.h)
        g, w = got['bbox'], want['bbox']
        print('coarse box', g.tolist(), w.tolist())
        assert g[6] == w[6] and g[7] == w[7], (g[6:], w[6:])
        empty = np.isinf(w[:6])                      # (a slot nothing entered: the same infinity)
        assert np.array_equal(g[:6][empty], w[:6][empty]) and np.abs(g[:6][~empty] - w[:6][~empty]).max() < 1e-6, (g[:6], w[:6])
        return
    for k in want:
        same_values(got[k], want[k], (case.name, k))


def test_gather_mosaics_satisfy_the_composition_of_their_members():
    """gather_mosaic: the election of tests/_gather_mosaic_oracle.py over each member's own amt_gather_mosaic; supersampled: the
    reduction of tests/_gather_supersample_oracle.py over amt_gather_mosaic on the sub-sample points.  No tolerance."""
    import _gather_mosaic_oracle as GO
    import _gather_supersample_oracle as SO

    def result(case):
        a = arrays(case, G.baseline(case)[0])
        return dict(img=a['img'], mask=a['mask'] != 0, elevation=a['elev'], source=a['source'], count=a.get('count'))

    def agree(got, want, what):
        assert np.array_equal(got['mask'], want['mask']) and np.array_equal(got['source'], want['source']), what
        assert np.array_equal(got['img'], want['img']), what
        assert np.isnan(got['elevation'][want['mask']]).all(), what
        keep = ~want['mask']
        assert np.array_equal(got['elevation'][keep].view(np.uint64), want['elevation'][keep].view(np.uint64)), what

    members = [result(S.gather_case('gather_member_%d' % k, (cam,))) for k, cam in enumerate(S.GATHER_CAMS)]
    mosaic = result(BY['gather_pair'])
    agree(mosaic, GO.compose(members, 1), 'gather_pair')
    assert {-1, 0, 1} <= set(np.unique(mosaic['source']).tolist())
    fine = result(S.gather_case('gather_points', S.GATHER_CAMS, S.GATHER_N))
    cells = result(BY['gather_pair_supersampled'])
    want = SO.reduce_cells(fine, S.GATHER_N, BY['gather_pair_supersampled'].min_count)
    agree(cells, want, 'gather_pair_supersampled')
    assert np.array_equal(cells['count'], want['count']) and 0 < want['mask'].sum() < want['mask'].size


# ---- a. poison, and f. release -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ALL, ids=list(BY))
def test_poisoned_buffer_changes_nothing(case):
    if not is_user(case):
        assert case.name not in S.USERS, 'the registry lists a case that asks for no scratch memory'
        return
    direct = case.name in S.USERS
    assert direct or case.family in S.DRIVER_FAMILIES, 'a user of scratch memory that the registry does not list'
    release()
    run(case, 'a fresh allocation, which the call sizes')            # (f: after a release the next call is right)
    sized = info()
    assert not direct or sized['bytes'] >= S.MIN_BYTES, sized
    for byte in (0xFF, 0x5A):
        p = prepare(case)
        fill(byte)
        filled = info()
        assert not direct or (filled['bytes'], filled['ptr']) == (sized['bytes'], sized['ptr']), (sized, filled)
        extra = call(case, p)
        after = info()
        check(case, read(case, p), extra, 'buffer filled with 0x%02X' % byte)
        # the whole buffer the call used was poisoned: it neither grew nor moved
        assert (after['bytes'], after['ptr']) == (filled['bytes'], filled['ptr']) and filled['bytes'] >= S.MIN_BYTES, (filled, after)


def test_every_call_site_counts_a_user():
    users = [c.name for c in ALL if is_user(c)]
    print('users of scratch memory:', users)
    for site, names in S.SITES.items():
        for name in names:
            assert name in users, (site, name, 'does not ask for scratch memory')
    assert set(S.MINIMUM) <= set(users)
    for name in users:
        assert name in S.USERS or BY[name].family in S.DRIVER_FAMILIES, name


def test_release_frees_the_buffer():
    case = BY[PENDING]
    run(case, 'before the release')
    held = info()
    assert held['bytes'] >= S.MIN_BYTES and held['ptr'] and held['streams'] >= 1
    release()
    gone = info()
    assert (gone['bytes'], gone['ptr']) == (0, 0) and gone['streams'] == held['streams'] - 1 and gone['requests'] == held['requests']
    release()                                        # nothing to free: no error
    run(case, 'after the release')
    again = info()
    assert again['bytes'] == S.MIN_BYTES and again['streams'] == held['streams'] and again['requests'] > held['requests']
    fill(0x5A, 3 * S.MIN_BYTES + 1)                  # the hook grows like a call, and does not count as one
    grown = info()
    assert grown['bytes'] == 3 * S.MIN_BYTES + 1 and grown['requests'] == again['requests'] and grown['streams'] == again['streams']
    run(case, 'after the hook has grown the buffer')
    release()


# ---- b. every ordered pair -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('first', S.USERS)
def test_every_user_after(first):
    a = BY[first]
    for name in S.USERS:
        G.baseline(BY[name])
    release()
    run(a, 'first')
    for name in S.USERS:
        run(BY[name], 'after ' + first)
        run(a, 'after ' + name)
    assert info()['bytes'] >= S.MIN_BYTES


# ---- c. growth inside a call --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('site', list(LARGE), ids=[c.name for c in LARGE.values()])
def test_growth_while_the_call_before_is_pending(site):
    import torch
    big, small = LARGE[site], BY[PENDING]
    need = S.large_bytes()[site]
    G.baseline(big)
    G.baseline(small)
    release()                                        # (the baseline's large buffer, on the default stream)
    side, other = streams(2)
    with on(other):
        release()
        run(small, 'on the other stream')
        elsewhere = info()
    with on(side):
        release()
        run(small, 'sizing the buffer')
        first = info()
        assert first['bytes'] == S.MIN_BYTES, first
        p_small, p_big = prepare(small), prepare(big)
        done = torch.cuda.Event()
        fill(0xFF)
        torch.cuda._sleep(int(G.cycles_per_ms() * HOLD_MS))
        e_small = call(small, p_small)
        done.record()
        pending = not done.query()
        e_big = call(big, p_big)                     # grows the buffer: waits for the stream, frees the old one
        grown = info()
        got_small, got_big = read(small, p_small), read(big, p_big)
        release()
    print('%s: asked for at least %d bytes, buffer %d -> %d; the call before was %s' %
          (big.name, need, first['bytes'], grown['bytes'], 'pending' if pending else 'NOT pending any more'))
    assert pending, 'the call before the growth had finished already: nothing was proved'
    check(small, got_small, e_small, 'the call before the growth')
    check(big, got_big, e_big, 'the call that grew the buffer')
    assert grown['bytes'] > S.MIN_BYTES and grown['bytes'] >= need and grown['ptr'], (first, grown, need)
    with on(other):
        assert info()['ptr'] == elsewhere['ptr'] and info()['bytes'] == elsewhere['bytes'], 'another stream\'s buffer changed'
        release()
    back_to_default()


# ---- d. two streams, one context -----------------------------------------------------------------------------------------------------------

def test_two_streams_keep_two_buffers():
    s1, s2 = streams(2)
    names = list(S.MINIMUM)
    for name in names:
        G.baseline(BY[name])
    for a, b in zip(names, names[1:] + names[:1]):
        with on(s1):
            release()
            run(BY[a], 'on the first stream')
            one = info()
        with on(s2):
            release()
            run(BY[b], 'on the second stream')
            two = info()
            p = prepare(BY[a])
            fill(0xFF)                               # enqueued on the second stream, not waited for
        assert one['ptr'] and two['ptr'] and one['bytes'] >= S.MIN_BYTES and two['bytes'] >= S.MIN_BYTES
        assert one['ptr'] + one['bytes'] <= two['ptr'] or two['ptr'] + two['bytes'] <= one['ptr'], (a, b, one, two)
        with on(s1):
            extra = call(BY[a], p)
            check(BY[a], read(BY[a], p), extra, 'while the second stream\'s buffer is filled')
            assert (info()['ptr'], info()['bytes']) == (one['ptr'], one['bytes'])
    for s in (s1, s2):
        with on(s):
            release()
    back_to_default()


# ---- e. eviction with work pending ----------------------------------------------------------------------------------------------------------

def test_eviction_of_a_stream_with_work_pending():
    """A call on S1 is held behind a gate, on decoy-then-true inputs as G.run_gated makes them; sixteen further streams then run a
    small user each, and the last of them evicts S1's buffer as the least recently used: the library has to wait for S1 before it
    frees it.  Before the gate fifteen of the further streams and then S1 get their buffers: that evicts whatever older buffers
    the context holds (freeing one waits for the device, hence for the gate), so that behind the gate the fifteen only renew
    their use and the sixteenth stream, the only new one, finds S1's buffer the oldest — the first call that has to wait."""
    import torch
    case, small = BY[PENDING], BY[SMALL]
    want, want_extra, host_ms = G.baseline(case)
    G.baseline(small)
    all_streams = streams(S.MAX_STREAMS + 1)
    assert len({s.cuda_stream for s in all_streams}) == S.MAX_STREAMS + 1
    s1, further = all_streams[0], all_streams[1:]
    with on(further[-1]):
        release()                                    # the one stream that comes new behind the gate
    for s in further[:-1]:
        with on(s):
            release()
            run(small, 'a further stream before the gate')
    with on(s1):                                     # S1 has its buffer before the gate: the gated call itself does not grow it
        release()
        run(case, 'S1 before the gate')
        full = info()
        assert full['bytes'] >= S.MIN_BYTES and full['streams'] == S.MAX_STREAMS, full
    sets = prepare(small, len(further))
    inp = OrderedDict((k, G.dev(d)) for k, (_t, d) in case.inputs.items())
    staging = OrderedDict((k, G.dev(t)) for k, (t, _d) in case.inputs.items())
    raw, out = G._fresh_outputs(case)
    closed_before, evicted_at, extras = [], None, []
    with G.Gate(G.gate_ms_for(host_ms), s1) as gate:
        for k in inp:
            inp[k].copy_(staging[k])
        env = G.Env(G._context(), inp, out, gate.opened)
        extra = case.call(env)
        snap = OrderedDict((k, v.clone()) for k, v in raw.items())
        for k, (s, p) in enumerate(zip(further, sets)):
            closed_before.append(not gate.opened.query())
            with on(s):
                extras.append(call(small, p))        # the one that evicts S1's buffer waits until the gate opens
            if evicted_at is None and info()['bytes'] == 0:
                evicted_at = k
        last = info()
    gate.side.synchronize()
    got_snap = OrderedDict((k, G.bits(v, case.canonical.get(k))) for k, v in snap.items())
    torch.cuda.synchronize()
    got = OrderedDict((k, G.bits(v, case.canonical.get(k))) for k, v in raw.items())
    print('S1\'s buffer was evicted by the call on further stream %s; the gate was closed before it: %s' %
          (evicted_at, None if evicted_at is None else closed_before[evicted_at]))
    assert not env.open_early and env.checks > 0, ('the gate was open already after', env.open_early)
    assert extra == want_extra
    assert evicted_at == len(further) - 1 and (last['bytes'], last['ptr']) == (0, 0), (evicted_at, last)
    assert closed_before[evicted_at], 'the gate was open before the call that evicted S1\'s buffer: nothing was pending'
    assert last['streams'] == S.MAX_STREAMS, last
    for k in want:
        assert np.array_equal(got_snap[k], want[k]), (k, 'the consumer on S1 saw other bytes than the baseline')
        assert np.array_equal(got[k], want[k]), (k, 'S1\'s outputs hold other bytes than the baseline')
    for p, e in zip(sets, extras):
        check(small, read(small, p), e, 'on a further stream')
    with on(s1):                                     # a new call on S1 allocates anew and is right
        run(case, 'S1 after the eviction')
        anew = info()
        assert anew['bytes'] >= S.MIN_BYTES and anew['ptr'] and anew['streams'] <= S.MAX_STREAMS, anew
    for s in all_streams:
        with on(s):
            release()
    back_to_default()
