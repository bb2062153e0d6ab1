"""
Host-side rules of the gather family that need a device to be stated: the SM -> geographic conversion of a grid (one smToLatLon
call for corners and centres) against a call per array, and the texts the three gather entry points leave in amt_last_error
for a refused call, byte for byte, and which of several faults is reported: the argument checks are shared between the entry
points, and each entry point keeps its text (its own name in front, "job k: " for a job of a batch) and its order.  Every call
here is refused before anything is read through a pointer, so the tables are empty and the arrays are one tensor that nobody
writes.
"""
import datetime

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_sm_grid_to_geographic_is_a_call_per_array():
    from auromat_amd.coordinates.transform import smToLatLon
    from auromat_amd.resample import sm_grid_to_geographic
    t = datetime.datetime(2012, 1, 25, 9, 26, 57)
    # a 3 x 4 grid: (4, 5) corners, (3, 4) centres, across the SM date line and up to the pole
    lat, lon = np.meshgrid([90.0, 80.5, 71.0, 61.5], [168.0, 174.0, 180.0, -174.0, -168.0], indexing='ij')
    lat_c, lon_c = np.meshgrid([85.25, 75.75, 66.25], [171.0, 177.0, -177.0, -171.0], indexing='ij')
    got = sm_grid_to_geographic(dict(lat=lat, lon=lon, lat_c=lat_c, lon_c=lon_c), t)
    want = (smToLatLon(lat, lon, t)[0], smToLatLon(lat, lon, t)[1], smToLatLon(lat_c, lon_c, t)[0], smToLatLon(lat_c, lon_c, t)[1])
    for g, w, shape in zip(got, want, ((4, 5), (4, 5), (3, 4), (3, 4))):
        assert g.shape == shape and g.dtype == np.float64 and (g == w).all()
    assert np.isfinite(got[0]).all() and not np.array_equal(got[0], lat)


def test_refusal_texts_and_their_order():
    import torch
    from auromat_amd._native import Context, GatherJob, GatherMember
    ctx = Context.current()
    lib, last = ctx._lib, lambda: (ctx._lib.amt_last_error(ctx.handle) or b'').decode()
    mem = torch.full((64,), 0x5A, dtype=torch.uint8, device=ctx.device)
    p = mem.data_ptr()
    members, jobs = (GatherMember * 1)(), (GatherJob * 1)()

    def mosaic(channels=3, interpolation=0):
        rc = lib.amt_gather_mosaic(ctx.handle, members, 1, 0, p, 2, p, 2, None, None, 1, channels, interpolation, 1, p, p, p, p, None,
                                   None)
        return rc, last()

    def supersampled(channels=3, interpolation=0, factor=2):
        rc = lib.amt_gather_mosaic_supersampled(ctx.handle, members, 1, 0, p, 2, p, 2, None, None, factor, 1, 1, channels,
                                                interpolation, 1, p, p, p, p, p, None)
        return rc, last()

    def frames(channels=3, interpolation=0, factor=2):
        rc = lib.amt_gather_frames(ctx.handle, jobs, 1, 0, factor, 1, 1, channels, interpolation, None)
        return rc, last()

    for call, name in ((mosaic, 'amt_gather_mosaic'), (supersampled, 'amt_gather_mosaic_supersampled'), (frames, 'amt_gather_frames')):
        assert call(channels=2) == (-1, name + ': channels must be 1, 3 or 4')
        assert call(interpolation=3) == (-1, name + ': unknown interpolation')
        assert call(channels=2, interpolation=3) == (-1, name + ': unknown interpolation')
    for call, name in ((supersampled, 'amt_gather_mosaic_supersampled'), (frames, 'amt_gather_frames')):
        assert call(factor=9) == (-1, name + ': factor must be 1 ... 8')
    # the supersampled mosaic looks at its own arguments first, a batch at the shared ones
    assert supersampled(factor=9, channels=2) == (-1, 'amt_gather_mosaic_supersampled: factor must be 1 ... 8')
    assert frames(factor=9, channels=2) == (-1, 'amt_gather_frames: channels must be 1, 3 or 4')
    # a job without out_img (the table is all zero)
    assert frames() == (-1, 'amt_gather_frames: job 0: NULL argument')
    ctx.synchronize()
    assert (mem == 0x5A).all()
