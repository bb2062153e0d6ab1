"""
TEST INFRASTRUCTURE — amt_gather_frames behind the gated side stream of tests/_gated_stream.py.

Three jobs of tests/_gather_frames_cases.py share a call: gm-a on a grid it sees all of, with a centre mask; the date-line camera
(another image size); gm-a again on 32 x 64 cells.  Every device input exists twice: images (random samples, other seeds), the
centre mask (other columns), and the axes (shifted by a fraction of a degree and wrapped back into range).  The call has no index
input: the job table holds pointers and sizes from the host, the same for the true arrays and the decoys.
"""
from collections import OrderedDict
import ctypes as C

import numpy as np

import _gather_frames_cases as FC

JOBS = ['g33x31', 'dateline', 'g32x64']
MASKED = 0                                  # the job that carries a centre mask
HARMLESS = ('no input is used as an index: the axes select the taps, and every tap is tested against the image\'s frame by the '
            'kernel itself (the support rule, the window\'s zero fill, the per-tap test of the global fetch); the centre mask is '
            'read at a pixel clamped to the frame; the job table and the prefix table of tile counts come from the host and are the '
            'same for the true arrays and the decoys: a kernel that ignores the gate computes other values, never another address')


def inputs(n, dtype=np.uint16, channels=3):
    out = OrderedDict()
    for k, name in enumerate(JOBS):
        cam = FC.camera(name)
        out['img_%d' % k] = (FC.image(name, dtype, channels), FC.image(name, dtype, channels, seed=900 + k))
        a, b, points = FC.coordinates(name, n)
        assert not points
        out['lat_%d' % k] = (a, a + 0.37)
        out['lon_%d' % k] = (b, FC.wrap180(b - 0.61))
        if k == MASKED:
            true, decoy = (np.zeros((cam['height'], cam['width']), dtype=np.uint8) for _ in range(2))
            true[:, 20:30] = 1
            decoy[:, 35:60] = 1
            out['center_mask'] = (true, decoy)
    return out


def outputs(n, dtype=np.uint16, channels=3):
    out = OrderedDict()
    for k, name in enumerate(JOBS):
        j = FC.by_name(name)
        out['img_%d' % k] = ((j['ny'], j['nx'], channels), dtype)
        out['mask_%d' % k] = ((j['ny'], j['nx']), np.uint8)
        out['elev_%d' % k] = ((j['ny'], j['nx']), np.float64)
        if n > 1:
            out['count_%d' % k] = ((j['ny'], j['nx']), np.uint8)
    return out


def case(n, interpolation='linear', dtype=np.uint16, channels=3):
    """the Case of one amt_gather_frames call with factor n (min_count: half of the sub-samples)"""
    import _gated_stream as GS
    import _inverse_cases as IC
    models = [IC.native(FC.camera(name)) for name in JOBS]
    min_count = max(1, (n * n + 1) // 2)

    def call(env):
        from auromat_amd._native import GatherJob
        i, o = env.inp, env.out
        table = (GatherJob * len(JOBS))()
        for k, (t, name, (params, zen)) in enumerate(zip(table, JOBS, models)):
            j = FC.by_name(name)
            C.memmove(C.byref(t.member.params), C.byref(params), C.sizeof(params))
            if zen is not None:
                t.member.zenithal = C.pointer(zen)
            t.member.img, t.member.min_elevation = i['img_%d' % k].data_ptr(), float('nan')
            if k == MASKED:
                t.member.center_mask = i['center_mask'].data_ptr()
            t.ny, t.nx = j['ny'], j['nx']
            t.lat, t.lon = i['lat_%d' % k].data_ptr(), i['lon_%d' % k].data_ptr()
            t.out_img, t.out_mask, t.out_elev = (o['%s_%d' % (key, k)].data_ptr() for key in ('img', 'mask', 'elev'))
            if n > 1:
                t.out_count = o['count_%d' % k].data_ptr()
        env.ctx.call('amt_gather_frames', table, len(JOBS), 0, n, min_count, np.dtype(dtype).itemsize, channels,
                     FC.CODES[interpolation], None)
        env.closed('amt_gather_frames')

    return GS.Case('gather_frames_x%d' % n, 'B', inputs(n, dtype, channels), outputs(n, dtype, channels), call, harmless=HARMLESS)


def build():
    return [case(1), case(3)]
