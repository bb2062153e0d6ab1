"""
Stream ordering of every family of entry points: each case of tests/_gated_cases.py behind a gated side stream
(tests/_gated_stream.py) — the call is made while its device inputs still hold a decoy, the true values arrive behind a sleeping
kernel on the same stream, and an ordered consumer on that stream as well as the host afterwards must see the bytes of the same
call on settled inputs.  A kernel, memset or copy on another stream than the context's, a missing event wait or a result
written on the wrong stream shows as a stale result; it cannot fault (the decoys are valid inputs).

Families: A calls on the context's stream, one per translation unit; B member tables uploaded from host vectors; C per-frame
statistics; D the frame driver (its own pre-pass, tail and finalise streams; the finalise stream is held by a short sleep so
that amt_pipe_join has something to wait for); E the sequence runner (device images, page-locked host images on its copy
stream, SequencePipeline.process); F the staged copies (amt_upload_staged / amt_download_staged on the copier's streams).

Host time of the calls on settled inputs (printed with -s; the gate is 100 ms or four times this, 2 s at the most), as
measured on an MI355X — every one far below 25 ms, so every gate is 100 ms: A masks 0.04 ms, outline_links 0.01, pixel_polygons
0.01, rotate_to_latlon 0.11, project 0.03, points_in_polygon 0.01, hist2d 0.10, world_to_pixel 0.07, directions_zenithal 0.03,
lens_remap 0.03; B mosaic 0.14, mosaic_median 0.20, mosaic_area 0.15, scanline 0.26, cubic 0.76 (the triangulation of its 49
points is made once, when the cases are built); C bin_frame 0.11, median_frame 0.14, median_frame_async 0.08,
quantile_frame_async 0.08, area_frame 0.13, area_frame_async 0.06, nearest 0.10; D georef_frame 0.14, georef_frame_dirs 0.07 (both sizes),
camera_path 0.46, camera_path_many 0.62, dirs_path 0.37, pipeline_run_dirs 0.88; E run_device_images 1.62, run_host_images 2.01,
sequence_pipeline 0.59; F amt_upload_staged 0.15 - 0.17 ms for 1 byte, 4 MiB - 1 and 8 MiB + 1.

What the module caught, on an MI355X with GPU_MAX_HW_QUEUES=4 (tests of this module that fail, each mutant in a run of its own):
  the tree before the pre-pass of amt_pipe_coarse_dirs waited for the context's stream     2 of 37  dirs_path (status 1 for 0: the
                                                                                         estimate came from the decoy directions),
                                                                                         pipeline_run_dirs (a second launch)
  k_or_mask launched on stream 0                                                          1 of 37  masks
  the copier's streams do not wait for `entry`                                            5 of 37  every upload, the downloads of
                                                                                         4 MiB - 1 and 8 MiB + 1 (one byte arrives
                                                                                         behind the writer without the wait)
  amt_pipe_join enqueues no wait                                                          3 of 37  camera_path, camera_path_many, dirs_path
  the new wait of the pre-pass stream removed                                             2 of 37  dirs_path, pipeline_run_dirs
  the runner's launch does not wait for a slot's `uploaded` event                         0 of 37  SURVIVES: the gate holds the
                                                                                         consumer (the context's stream), not the
                                                                                         producer; the copy stream is the runner's
                                                                                         own and cannot be held from outside, and
                                                                                         18 KB are across the link long before the
                                                                                         launch behind the gate runs
(Counted when the module had 37 tests; georef_frame_dirs_64x17 came later and runs none of the mutated code.)
A passing run proves less than a failing one here: with four hardware queues several streams share one, and a gated stream can
hold back a stream of the library's by accident.
"""
import ctypes as C

import numpy as np
import pytest

import _gated_cases as K
import _gated_stream as G

pytestmark = pytest.mark.gpu

CASES = K.build()


@pytest.fixture(scope='module', autouse=True)
def _release_what_the_cases_keep():
    yield
    K.release()


def family(letter):
    cases = [c for c in CASES if c.family == letter]
    return pytest.mark.parametrize('case', cases, ids=[c.name for c in cases])


@family('A')
def test_context_stream_calls(case):
    G.run_gated(case)


@family('B')
def test_tables_uploaded_from_host_vectors(case):
    G.run_gated(case)


@family('C')
def test_per_frame_statistics(case):
    G.run_gated(case)


@family('D')
def test_frame_driver(case):
    G.run_gated(case)


@family('E')
def test_sequence_runner(case):
    G.run_gated(case)


# ---- F. staged copies ------------------------------------------------------------------------------------------------------------
# Bytes only: nothing that is copied is used as an address, so a copy that ignores the gate moves other bytes, no more.

PIECE = 4 << 20                                 # AMT_COPY_PIECE_MB: the size of a piece of the copier
SIZES = [1, PIECE - 1, 2 * PIECE + 1]


def _bytes(seed, n):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)


def _context():
    from auromat_amd._native import Context
    return Context.current()


def _settled_upload_ms(size):
    """host time of amt_upload_staged on settled buffers (the second of two calls: the first one builds the copier)"""
    import time
    import torch
    src, dst = _bytes(1, size), G.dev(_bytes(2, size))
    ms = 0.0
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _context().call('amt_upload_staged', C.c_void_p(dst.data_ptr()), C.c_void_p(src.ctypes.data), size)
        ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), src)
    print('amt_upload_staged of %d bytes: host time on settled buffers %.2f ms' % (size, ms))
    return ms


@pytest.mark.parametrize('size', SIZES)
def test_upload_staged_starts_behind_what_the_stream_holds(size):
    """A clone of the buffer queued behind the gate, BEFORE the upload, still has to read the old bytes: the copier's streams
    wait for the `entry` event.  A clone queued after the upload holds the new bytes: the stream continues behind them."""
    import torch
    old, new = _bytes(3, size), _bytes(4, size)
    buf = G.dev(old)
    with G.Gate(G.gate_ms_for(_settled_upload_ms(size))) as gate:
        before = buf.clone()
        _context().call('amt_upload_staged', C.c_void_p(buf.data_ptr()), C.c_void_p(new.ctypes.data), size)
        open_early = gate.opened.query()
        after = buf.clone()
    gate.side.synchronize()
    got_before, got_after = before.cpu().numpy(), after.cpu().numpy()
    torch.cuda.synchronize()
    _context()
    assert not open_early, 'the gate (%.0f ms) was open when amt_upload_staged returned' % gate.ms
    assert np.array_equal(got_before, old), ('the reader queued before the upload saw new bytes', int((got_before != old).sum()))
    assert np.array_equal(got_after, new), ('the reader queued after the upload saw old bytes', int((got_after != new).sum()))
    assert np.array_equal(buf.cpu().numpy(), new)


@pytest.mark.parametrize('size', SIZES)
def test_download_staged_waits_for_the_writer_before_it(size):
    """amt_download_staged synchronises: it returns the bytes a writer queued behind the gate leaves, not the ones before."""
    import torch
    decoy, true = _bytes(5, size), _bytes(6, size)
    buf, staging = G.dev(decoy), G.dev(true)
    host = np.full(size, G.POISON, dtype=np.uint8)
    with G.Gate() as gate:
        buf.copy_(staging)
        _context().call('amt_download_staged', C.c_void_p(host.ctypes.data), C.c_void_p(buf.data_ptr()), size)
    torch.cuda.synchronize()
    _context()
    assert np.array_equal(host, true), ('stale bytes', int((host != true).sum()), 'of them the decoy', int((host == decoy).sum()))
