"""
The fused row kernel (k_georef_rows of auromat_amd/csrc/amt_georef.hip, directions-in form) on the constructed direction fields
of tests/_rowfield_cases.py: every field goes to ``amt_georef_frame_dirs`` with the test's own output buffers, pre-filled with a
poison byte, and EVERY element of lat, lon, lat_c, lon_c, elev, mlat, mlt, mlat_c, mlt_c is compared with the longdouble /
mpmath reference of tests/_rowfield_oracle.py.  tests/test_rowfield_cases_cpu.py checks without a GPU that the fields hold what
they claim and that the reference is right.

What the fields aim at: the small-angle row marching on both sides of its limit (tan^2 <= 9e-4) and the full arctangents behind
it, the |lon| < 178 guard of the small-angle sum and its SM twin, a pole 1e-6 deg from a corner, rays 1e-7 rad inside and outside
the limb (whole miss rows inside a chunk: the wave-uniform shortcut; single missing lanes; first hits after misses), a camera
inside the shell, the asin form switch at 45 deg and the clamp at the nadir, directions that are not unit vectors or NaN, and
frame sizes around one strip of 63 corner columns and one chunk of 16 rows.

NaN patterns must be identical.  Distances (degrees): |d lat|, |d lon wrapped| cos(lat) (raw longitude is ill-conditioned at a
pole), |d elev|, |d MLT wrapped at 24 h| 15 cos(MLat).  Bound per family and array: 8 max(E_ref, eps scale) with a floor of
1e-10 deg (the level tests/test_gpu_cameras.py asserts for these arrays), E_ref the distance of the float64 oracle
(oracle/ref_numpy.py) from the same reference on the same inputs.

Then: the two plans of the pipeline (run(fuse=True) / run(fuse=False)) give bit-identical grids and arrays on every field
without a pole, and pipe.bounding_box() — amt_sanitize_masks + amt_bbox_corners behind it — equals the reference's rule on the
reference arrays at min_elevation None and 10.

Largest values measured on the MI355X, kernel distance / E_ref / bound in degrees (printed per case and per family with -s):
  ownership  lat 4.8e-14 / 2.7e-14 / 1e-10   lon 9.5e-13 / 1.8e-14 / 1e-10   elev 4.7e-12 / 4.2e-13 / 1e-10   mlt 6.5e-13 / 4.0e-14 / 1e-10
  step       lat 7.8e-13 / 1.0e-13 / 1e-10   lon 2.0e-12 / 9.5e-14 / 1e-10   elev 4.2e-13 / 2.1e-13 / 1e-10   mlt 2.1e-12 / 1.1e-13 / 1e-10
  dateline   lat 1.3e-12 / 1.5e-14 / 1e-10   lon 2.6e-13 / 5.8e-14 / 1e-10   elev 1.4e-12 / 1.0e-12 / 1e-10   mlt 2.7e-13 / 8.2e-14 / 1e-10
  pole       lat 6.8e-14 / 2.4e-14 / 1e-10   lon 5.6e-14 / 1.5e-14 / 1e-10   elev 4.7e-12 / 3.1e-14 / 1e-10   mlt 8.3e-14 / 1.8e-14 / 1e-10
  limb       lat 2.1e-11 / 2.7e-11 / 2.2e-10 lon 2.5e-11 / 3.5e-11 / 2.8e-10 elev 1.6e-11 / 2.1e-11 / 1.7e-10 mlt 2.3e-11 / 3.3e-11 / 2.6e-10
  inside     lat 2.2e-12 / 3.2e-14 / 1e-10   lon 9.0e-13 / 2.9e-14 / 1e-10   elev 2.9e-12 / 4.3e-14 / 1e-10   mlt 4.6e-13 / 5.0e-14 / 1e-10
  elevation  lat 4.6e-13 / 1.6e-13 / 1e-10   lon 1.6e-12 / 1.3e-12 / 1e-10   elev 4.6e-11 / 1.1e-10 / 8.8e-10 mlt 1.4e-12 / 1.3e-12 / 1e-10
  scaled     lat 3.9e-14 / 2.2e-14 / 1e-10   lon 1.0e-13 / 1.3e-14 / 1e-10   elev 3.2e-13 / 2.1e-14 / 1e-10   mlt 1.2e-13 / 2.8e-14 / 1e-10
  broken     lat 3.9e-14 / 2.1e-14 / 1e-10   lon 1.0e-13 / 1.2e-14 / 1e-10   elev 4.7e-12 / 2.7e-14 / 1e-10   mlt 1.2e-13 / 2.8e-14 / 1e-10
(the centre arrays and mlat come out like their corner arrays and lat: at most 2.2e-12 away from the limb.)  Only at the limb and at
89.999 deg of elevation does E_ref, not the floor, set the bound: there the kernel and the float64 oracle alike lose the digits
that the discriminant cancels and that the arc sine next to 1 magnifies.  Every case of the
plans test took the single-pass plan with fuse=True.
"""
import ctypes as C

import numpy as np
import pytest

import _rowfield_cases as K
import _rowfield_oracle as R

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_F64 = np.frombuffer(bytes([POISON] * 8), dtype=np.uint64)[0]


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


def poisoned(shape):
    import torch
    t = _ctx().empty(shape)
    t.view(torch.uint8).fill_(POISON)
    return t


def frame_params(c):
    from auromat_amd._native import FrameParams
    p = FrameParams()
    p.width, p.height, p.fast_center = c['width'], c['height'], 1
    p.cd[:] = [1.0, 0.0, 0.0, 1.0]              # the camera model is not used: the directions come from the caller
    p.crpix[:] = [0.0, 0.0]
    p.rot[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    p.cam[:] = [float(v) for v in c['cam']]
    p.a, p.b, p.a0, p.b0 = c['a'], c['b'], c['a0'], c['b0']
    p.m_geo[:] = [float(v) for v in np.asarray(c['m_geo']).ravel()]
    p.m_sm[:] = [float(v) for v in np.asarray(c['m_sm']).ravel()]
    return p


_RUNS = {}


def kernel_arrays(name):
    """One launch of the plain entry point per case, on poisoned buffers -> dict of the nine host arrays."""
    if name not in _RUNS:
        import torch
        from auromat_amd._native import GeorefOut
        c, ctx = K.by_name(name), _ctx()
        h, w = c['height'], c['width']
        dirs = ctx.to_device(np.array(c['dirs']))
        out = GeorefOut()
        bufs = {k: poisoned((h + 1, w + 1) if k in R.CORNER_ARRAYS else (h, w)) for k in R.ARRAYS}
        for k, v in bufs.items():
            setattr(out, k, v.data_ptr())
        p = frame_params(c)
        ctx.call('amt_georef_frame_dirs', C.byref(p), C.c_void_p(dirs.data_ptr()), C.byref(out))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in bufs.items()}
        for k, v in got.items():
            assert not (v.view(np.uint64) == POISON_F64).any(), (name, k, 'elements the kernel did not write')
        _RUNS[name] = got
    return _RUNS[name]


@pytest.mark.parametrize('name', K.names())
def test_every_element_against_the_reference(name):
    c, ref, got = K.by_name(name), K.reference(name), kernel_arrays(name)
    bounds = K.bounds(c['family'])
    failed = []
    for k in R.ARRAYS:
        assert got[k].shape == ref[k].shape
        mism = np.argwhere(np.isnan(got[k]) != np.isnan(ref[k]))
        assert len(mism) == 0, '%s %s: NaN pattern differs at %s' % (name, k, mism[:6].tolist())
        d = R.distance(k, got, ref)
        worst, at = float(d.max()), np.unravel_index(int(d.argmax()), d.shape)
        e_ref = K.e_ref(c['family'], k)
        print('%s %s: kernel %.3e  E_ref %.3e  bound %.3e  (%.2f of the bound, at %s)' % (name, k, worst, e_ref, bounds[k],
                                                                                         worst / bounds[k], at))
        if not worst <= bounds[k]:
            failed.append((k, worst, bounds[k], at))
    assert not failed, (name, failed)


def test_largest_distances_per_family():
    """the table of the module docstring (-s); asserts again, per family, what the test above asserts per case"""
    for fam in K.FAMILIES:
        bounds, cells = K.bounds(fam), []
        for k in R.ARRAYS:
            worst = max(float(R.distance(k, kernel_arrays(c['name']), K.reference(c['name'])).max()) for c in K.family(fam))
            cells.append('%s %.1e / %.1e / %.1e' % (k, worst, K.e_ref(fam, k), bounds[k]))
            assert worst <= bounds[k], (fam, k, worst, bounds[k])
        print('  %-10s' % fam + ';  '.join(cells))


def test_zero_on_the_date_line_is_a_half_turn():
    """y = +0 / -0 at x < 0: the longitude is 180 or -180 (compared modulo 360 above), never NaN or 0."""
    for name in ('dateline-zero-plus', 'dateline-zero-minus'):
        got = kernel_arrays(name)
        assert abs(got['lon'][1, 2]) == 180.0, (name, got['lon'][1, 2])
        assert abs(got['mlt'][1, 2] - 12.0) == 12.0, (name, got['mlt'][1, 2])


def test_longitudes_stay_in_their_range():
    """the small-angle sum never leaves [-180, 180] (MLT: [0, 24]), whatever path computed the value"""
    for name in K.names():
        got = kernel_arrays(name)
        for k in ('lon', 'lon_c'):
            v = got[k][~np.isnan(got[k])]
            assert np.all(np.abs(v) <= 180.0), (name, k, float(np.abs(v).max()))
        for k in ('mlt', 'mlt_c'):
            v = got[k][~np.isnan(got[k])]
            assert np.all((v >= 0.0) & (v <= 24.0)), (name, k, float(v.min()), float(v.max()))


# ---- the two plans ------------------------------------------------------------------------------------------------------------
PX_PER_DEG = dict(ownership=40, step=2, dateline=4, limb=10, inside=6, elevation=4, scaled=40, broken=40)
# every field without a pole but ownership-1x1: the library refuses fused binning on a frame of fewer than 3 pixels whatever
# the resolution ("fused binning needs at least 3 pixels", prepare_georef in amt_georef.hip: a lane loads a pixel as 8 bytes),
# so a one-pixel frame has one plan only; the resolutions give every other field a grid the driver can fuse
PLAN_CASES = [c['name'] for c in K.cases() if not c['pole'] and c['width'] * c['height'] >= 3]


def plan_elevation(c):
    return 10 if c['family'] in ('ownership', 'elevation') else None


def image_of(c):
    rng = np.random.RandomState(c['width'] * 131 + c['height'])
    return rng.randint(0, 65536, size=(c['height'], c['width'], 3)).astype(np.uint16)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == 'f':
        ua, ub = a.view(np.uint64), b.view(np.uint64)
        return bool(np.all((ua == ub) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


@pytest.mark.parametrize('name', PLAN_CASES)
def test_plans_are_bit_identical(name):
    from auromat_amd.pipeline import FramePipeline
    c = K.by_name(name)
    pipe = FramePipeline(c['width'], c['height'], with_mag=True)
    dirs = pipe.ctx.to_device(np.array(c['dirs']))
    p, img, ppd = frame_params(c), image_of(c), PX_PER_DEG[c['family']]
    res, arrays, plans = [], [], []
    for fuse in (True, False):
        r = pipe.run(None, c['altitude'], None, None, img=img, fast=True, min_elevation=plan_elevation(c), pxPerDeg=ppd, params=p,
                     fuse=fuse, dirs=dirs)
        plans.append(pipe.last_plan)
        res.append({k: np.array(r[k]) for k in ('mean', 'count', 'img', 'mask')})
        arrays.append({k: np.array(v) for k, v in pipe.host_arrays().items()})
    print(name, plans, res[0]['mean'].shape)
    assert plans == ['single-pass', 'two-pass'], (name, plans)
    for k in res[0]:
        assert same_bits(res[0][k], res[1][k]), (name, 'grid', k)
    assert set(arrays[0]) == set(R.ARRAYS)
    for k in arrays[0]:
        assert same_bits(arrays[0][k], arrays[1][k]), (name, 'array', k)
        assert same_bits(arrays[1][k], kernel_arrays(name)[k]), (name, 'array of the plain entry point', k)
    assert res[0]['count'].sum() > 0


# ---- the bounding box -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_elevation', [None, 10])
@pytest.mark.parametrize('name', K.names())
def test_bounding_box_follows_the_reference_rule(name, min_elevation):
    from auromat_amd.pipeline import EmptyFrame, FramePipeline
    c, ref = K.by_name(name), K.reference(name)
    want = R.reference_box(ref, min_elevation)
    pipe = FramePipeline(c['width'], c['height'], alloc_image=False)
    dirs = pipe.ctx.to_device(np.array(c['dirs']))
    pipe.georef(None, c['altitude'], None, None, min_elevation=min_elevation, params=frame_params(c), dirs=dirs)
    if want is None:
        with pytest.raises(EmptyFrame):
            pipe.bounding_box()
        return
    bb = pipe.bounding_box()
    south, west, north, east, pole, crosses = want
    b = K.bounds(c['family'])
    got = (bb.latSouth, bb.lonWest, bb.latNorth, bb.lonEast)
    print(name, min_elevation, 'box', got, 'reference', want[:4], 'pole', pole, 'date line', crosses)
    assert abs(bb.latSouth - south) <= b['lat'] and abs(bb.latNorth - north) <= b['lat'], (got, want)
    assert abs(bb.lonWest - west) <= b['lon'] and abs(bb.lonEast - east) <= b['lon'], (got, want)
    assert bool(bb.containsPole) == pole
    if not pole:                                              # (a box all around counts as crossing, by definition)
        assert bool(bb.containsDiscontinuity) == crosses
    if pole:
        assert (bb.lonWest, bb.lonEast) == (-180, 180) and (bb.latNorth == 90 if c['pole'] > 0 else bb.latSouth == -90)
        assert pole == bool(c['pole'])
    if c['dateline'] and min_elevation is None:
        assert crosses and bb.lonWest > 0 >= bb.lonEast          # west from the positive slot, east from the non-positive one
