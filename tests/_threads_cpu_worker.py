"""
TEST INFRASTRUCTURE — the child process of tests/test_threads_cpu.py: the library's host-only entry points on fixed inputs,
either one after the other on the main thread (`sequential`) or from four threads at once behind a barrier (`threads`), in a
fresh process so that whatever an entry point initialises on first use (the Gauss-Legendre nodes behind
amt_plate_carree_resolution, csrc/amt_grid.h) is initialised by the racing threads.  No GPU is touched: none of these entry points
takes a context.

Prints one JSON line: per run (one in `sequential`, four in `threads`) the SHA-256 of every job's result bytes.  Before the
barrier nothing of the library has been called but amt_abi_version (auromat_amd._native.lib); the inputs are Python objects.

Inputs, from the existing CPU tests: the 17 frames of tests/test_sky_rows.py (both pointings at several sizes, rolled cameras,
zenith, nadir, a pole frame; amt_frame_params_from_wcs, amt_georef_sky_rows, amt_georef_image_rows, amt_georef_band_roles,
amt_georef_core_bands, amt_pole_in_view), the boxes of tests/test_host_cpu.py (amt_plate_carree_resolution) and of
tests/_gated_cases.py (amt_grid_layout), the paced frames and boxes of tests/test_host_rules_cpu.py (amt_box_hint), every
(n, q) of a small table (amt_quantile_rank), the packed grids of tests/test_host_cpu.py (amt_seq_unpack, amt_seq_payload_size).
"""
import ctypes as C
import hashlib
import json
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

N_THREADS = 4
NEG_INF = float('-inf')
THRESHOLDS = (None, 0.0, 10.0, 45.0)
BOXES = [(40.0, -10.0, 50.0, 10.0, 100.0), (-5.0, 170.0, 5.0, -170.0, 200.0), (-5.0, -10.0, 5.0, 10.0, 200.0),
         (60.0, -180.0, 90.0, 180.0, 100.0), (-89.0, 3.0, -60.5, 47.25, 13.7), (12.5, -71.0, 12.75, -70.9, 50.0)]
LAYOUTS = [(2.0, 2.0, 44.0, 58.0, -108.0, -86.0), (10.0, 10.0, 39.0, 51.0, 9.0, 29.0), (4.0, 5.0, 40.6, 43.74, -98.0, -94.1),
           (25.0, 17.0, -12.3, 7.9, 171.0, 179.5)]
BOX_A = [40.0, 52.0, -101.0, -80.0, float('inf'), -80.0, 1000.0, 0.0]          # tests/test_host_rules_cpu.py
BOX_B = [40.5, 52.25, -100.0, -79.5, float('inf'), -79.5, 1100.0, 0.0]


def frames():
    import test_sky_rows
    return [tuple(c[1:4]) for c in test_sky_rows.cases()]


def packed_grids():
    """the buffer of tests/test_host_cpu.py::test_seq_unpack_and_payload_size_are_host_functions (Python and torch on the CPU)"""
    import torch
    from auromat_amd.resample import _Grid
    from auromat_amd.sequence import DESC_LEN, pack_results
    res = []
    for k in (2, 5, 7):
        grid = _Grid((4, 5), 40.0 + 0.3 * k, 43.0 + 0.37 * k, -100.0 + k, -96.5 + 1.2 * k)
        rs = np.random.RandomState(k)
        res.append(dict(mean=torch.from_numpy(rs.uniform(0, 9, (grid.ny, grid.nx, 4))), count=torch.from_numpy(
            rs.randint(0, 50, (grid.ny, grid.nx)).astype(np.float64)), grid=grid, contains_pole=k == 5,
            contains_discontinuity=k == 7, altitude=100.0 + k, magnetic=k == 2))
    res.insert(1, None)
    descs, payload = pack_results(res, [2, 3, 5, 7], torch.device('cpu'))
    max_frames = 6
    buf = np.zeros(max_frames * DESC_LEN + payload.numel())
    buf[:descs.numel()] = descs.numpy().ravel()
    buf[max_frames * DESC_LEN:] = payload.numpy()
    return buf, max_frames, int(payload.numel())


def make_jobs(L, FRAMES, PACKED):
    """[(name, function -> bytes)]; every function makes its own outputs, the inputs are shared and only read"""
    from auromat_amd._native import FrameParams, Grid, SeqFrame
    from auromat_amd.mapping.astrometry import run_frame

    def params(hdr, cam, t, altitude=110.0, fast=1, magnetic=1):
        p = FrameParams()
        rc = L.amt_frame_params_from_wcs(C.byref(run_frame(hdr, cam, t, altitude)), int(hdr['IMAGEW']), int(hdr['IMAGEH']), fast,
                                         float(altitude), magnetic, C.byref(p))
        assert rc == 0
        return p

    def plate_carree():
        out = []
        for box in BOXES:
            la, lo = C.c_double(-1), C.c_double(-1)
            out.append((L.amt_plate_carree_resolution(*(box + (C.byref(la), C.byref(lo)))), la.value, lo.value))
        return np.array(out).tobytes()

    def grid_layout():
        out = b''
        for args in LAYOUTS:
            g = Grid()
            assert L.amt_grid_layout(*(args + (C.byref(g),))) == 0
            out += bytes(g)
        return out

    def frame_params():
        return b''.join(bytes(params(*f, altitude=a, fast=fast, magnetic=m)) for f in FRAMES for a in (110.0, 300.0)
                        for fast in (1, 0) for m in (1, 0))

    def per_frame(fn):
        def job():
            return np.array([fn(params(*f), thr) for f in FRAMES for thr in THRESHOLDS], dtype=np.int64).tobytes()
        return job

    def band_roles(p, thr):
        rows, r = C.c_int32(0), (C.c_int32 * 8)()
        assert L.amt_georef_band_roles(C.byref(p), NEG_INF if thr is None else thr, C.byref(rows), r) == 0
        return [rows.value] + list(r)

    def core_bands(p, thr):
        c2 = (C.c_int32 * 2)()
        assert L.amt_georef_core_bands(C.byref(p), NEG_INF if thr is None else thr, c2) == 0
        return list(c2)

    def sky_rows(p, thr):
        out = [C.c_int32(0) for _ in range(4)]
        assert L.amt_georef_sky_rows(C.byref(p), *[C.byref(o) for o in out]) == 0
        return [o.value for o in out]

    def image_rows(p, thr):
        r0, r1 = C.c_int32(-1), C.c_int32(-1)
        assert L.amt_georef_image_rows(C.byref(p), NEG_INF if thr is None else thr, C.byref(r0), C.byref(r1)) == 0
        return [r0.value, r1.value]

    def pole(p, thr):
        return [L.amt_pole_in_view(C.byref(p), NEG_INF if thr is None else thr, m) for m in (0, 1)]

    def quantile_rank():
        out = []
        for n in list(range(1, 41)) + [1000, 12345678]:
            for q in (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9, 0.999, 1.0):
                k, k2, g = C.c_int64(-1), C.c_int64(-1), C.c_double(-1)
                out.append((L.amt_quantile_rank(n, q, C.byref(k), C.byref(k2), C.byref(g)), k.value, k2.value, g.value))
        return np.array(out).tobytes()

    def box_hint():
        """tests/test_host_rules_cpu.py: b 30 km after a, the new frame at the pace of a -> b, 1 ... 9 frames on"""
        import copy
        from auromat_amd.synthetic import sequence_frame
        d8 = C.c_double * 8
        a = params(*sequence_frame(0, 424, 283)[:3])
        b = copy.deepcopy(a)
        b.cam[0] += 30.0
        out = []
        for n_bc in range(1, 10):
            c = copy.deepcopy(b)
            for field in ('cam', 'rot', 'cd'):
                x, y, z = getattr(a, field), getattr(b, field), getattr(c, field)
                for i in range(len(z)):
                    z[i] = y[i] + (y[i] - x[i]) * n_bc
            est = d8()
            rc = L.amt_box_hint(d8(*BOX_B), C.byref(b), 1, d8(*BOX_A), C.byref(a), 0, 1 + n_bc, C.byref(c), est)
            out.append([float(rc)] + list(est))
            est = d8()
            rc = L.amt_box_hint(d8(*BOX_B), C.byref(b), 1, None, None, 0, 1 + n_bc, C.byref(c), est)       # no frame before the latest
            out.append([float(rc)] + list(est))
        return np.array(out).tobytes()

    def seq_unpack():
        buf, max_frames, payload = PACKED
        out = (SeqFrame * 8)()
        n = C.c_int32()
        base = buf.ctypes.data
        assert L.amt_seq_unpack(C.c_void_p(base), buf.size, 4, max_frames, out, 8, C.byref(n)) == 0 and n.value == 3
        size = C.c_int64()
        assert L.amt_seq_payload_size(out, 3, C.byref(size)) == 0 and size.value == payload
        rec = []
        for f in out[:3]:
            rec.append([f.ny, f.nx, f.nc, f.index, f.lat0, f.lon0, f.dlat, f.dlon, f.contains_pole, f.contains_discontinuity, f.magnetic,
                        f.altitude, f.mean - base, f.count - base])          # (the pointers as offsets into the buffer)
        return np.array(rec).tobytes() + np.array([size.value]).tobytes()

    return [('amt_plate_carree_resolution', plate_carree), ('amt_grid_layout', grid_layout), ('amt_frame_params_from_wcs', frame_params),
            ('amt_georef_band_roles', per_frame(band_roles)), ('amt_georef_core_bands', per_frame(core_bands)),
            ('amt_georef_sky_rows', per_frame(sky_rows)), ('amt_georef_image_rows', per_frame(image_rows)),
            ('amt_pole_in_view', per_frame(pole)), ('amt_quantile_rank', quantile_rank), ('amt_box_hint', box_hint),
            ('amt_seq_unpack', seq_unpack)]


def main(mode):
    from auromat_amd import _native
    L = _native.lib()
    jobs = make_jobs(L, frames(), packed_grids())
    digest = lambda b: hashlib.sha256(b).hexdigest()
    if mode == 'sequential':
        runs = [dict((name, digest(fn())) for name, fn in jobs)]
    else:
        runs, errors = [None] * N_THREADS, []
        start = threading.Barrier(N_THREADS, timeout=60)

        def body(t):
            try:
                start.wait()
                runs[t] = dict((name, digest(fn())) for name, fn in jobs)
            except BaseException as e:                  # noqa: B902
                errors.append(repr(e))
                start.abort()

        threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(N_THREADS)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(60)
        assert not errors and not any(th.is_alive() for th in threads), errors
    print(json.dumps(dict(mode=mode, runs=runs)))


if __name__ == '__main__':
    main(sys.argv[1])
