"""
The fused row kernel (k_georef_rows of auromat_amd/csrc/amt_georef.hip) in its camera-model form, and what only that form runs —
make_affine_cam / affine_ray, sky_bands and fill_nan, exact centres with corners_ok, SECOND = 4, k_coarse_bbox<false> and the
in-kernel box — on the constructed cameras of tests/_camera_cases.py.  Every case goes to ``amt_georef_frame`` with the test's own
output buffers, pre-filled with a poison byte, and EVERY element of lat, lon, lat_c, lon_c, elev, mlat, mlt, mlat_c, mlt_c is
compared with the longdouble / mpmath reference of tests/_camera_oracle.py.  tests/test_camera_cases_cpu.py checks without a GPU
that the cases hold what they claim, that the reference is right and that the host's sky bands are sound.

NaN patterns must be identical (no ray of any case has |relative discriminant| below the margin of the row-field limb family).
Distances and bound are those of tests/_rowfield_oracle.py: |d lat|, |d lon wrapped| cos(lat), |d elev|, |d MLT wrapped at 24 h|
15 cos(MLat); per family and array 8 max(E_ref, eps scale) with a floor of 1e-10 deg, E_ref the distance of the float64 oracle
(oracle/ref_numpy.py::georef_frame on the same parameters) from the same reference.

Then: a run without the MLat / MLT pointers gives the same bits in the other five arrays; sky bands are NaN throughout with each
output base moved by one double and the element behind each array untouched; amt_georef_out.bbox and amt_georef_coarse_bbox
against the reference's boxes; the MLat / MLT-only variant bit-identical to the nine-array mode; the two plans of the pipeline
bit-identical on the header form of the cases.

Largest values measured on the MI355X, kernel distance / E_ref / bound in degrees (printed per case and per family with -s):
  cd        lat 5.2e-13 / 2.6e-14 / 1e-10    lon 2.8e-13 / 1.8e-14 / 1e-10    elev 1.5e-12 / 6.5e-14 / 1e-10    mlt 3.3e-13 / 3.5e-14 / 1e-10
  wide      lat 2.4e-12 / 1.8e-12 / 1e-10    lon 1.5e-12 / 5.9e-12 / 1e-10    elev 4.7e-12 / 1.6e-12 / 1e-10    mlt 1.7e-12 / 6.1e-12 / 1e-10
  limb      lat 2.4e-12 / 1.2e-11 / 1e-10    lon 1.1e-12 / 7.0e-12 / 1e-10    elev 1.1e-12 / 4.9e-12 / 1e-10    mlt 2.7e-13 / 1.9e-12 / 1e-10
  far       lat 7.1e-11 / 1.8e-11 / 1.5e-10  lon 1.5e-10 / 8.3e-11 / 6.7e-10  elev 3.5e-11 / 1.9e-11 / 1.5e-10  mlt 1.5e-10 / 8.4e-11 / 6.7e-10
  low       lat 3.9e-14 / 8.0e-13 / 1e-10    lon 4.5e-13 / 1.4e-12 / 1e-10    elev 1.8e-11 / 5.6e-12 / 1e-10    mlt 3.2e-13 / 1.6e-12 / 1e-10
  inside    lat 1.5e-12 / 8.6e-14 / 1e-10    lon 5.5e-13 / 3.5e-14 / 1e-10    elev 8.4e-14 / 7.1e-14 / 1e-10    mlt 1.4e-13 / 6.4e-14 / 1e-10
  exact     lat 2.3e-12 / 1.2e-11 / 1e-10    lon 1.8e-12 / 7.0e-12 / 1e-10    elev 1.6e-11 / 1.5e-11 / 1.2e-10  mlt 1.5e-12 / 2.1e-12 / 1e-10
  pole      lat 2.5e-14 / 1.7e-14 / 1e-10    lon 6.2e-15 / 3.1e-15 / 1e-10    elev 1.5e-12 / 6.0e-14 / 1e-10    mlt 1.6e-14 / 9.0e-15 / 1e-10
  dateline  lat 2.6e-13 / 9.4e-15 / 1e-10    lon 1.4e-14 / 3.2e-14 / 1e-10    elev 2.9e-13 / 2.5e-13 / 1e-10    mlt 8.8e-13 / 2.1e-14 / 1e-10
(the centre arrays and mlat come out like their corner arrays and lat; exact centres: lon_c 4.3e-12 / 2.2e-12, mlt_c 5.7e-12 / 2.5e-12.)
The worst case takes 0.49 of its bound: lat of far-disc-inside, corner (22, 143) at the top of the disc (kernel 7.1e-11, E_ref 1.8e-11,
bound 1.5e-10).  Only from 42 000 km and at 89.9 deg of elevation does E_ref, not the floor, set a bound.  Every case of the plans
test took the single-pass plan with fuse=True, in both centre modes and with both image types.  No fault was found in the library.
With `cx` of make_affine_cam off by 1e-6 171 of these tests fail, with the sign of `hcy` flipped 17, with `*top_end` of sky_bands
one band larger 125 (and 101 of tests/test_camera_cases_cpu.py), with `corners_ok` forced true 17.
"""
import ctypes as C

import numpy as np
import pytest

import _camera_cases as K
import _camera_oracle as Q

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_F64 = np.frombuffer(bytes([POISON] * 8), dtype=np.uint64)[0]
NEG_INF = float('-inf')
GEO = ('lat', 'lon', 'lat_c', 'lon_c', 'elev')
MAG = ('mlat', 'mlt', 'mlat_c', 'mlt_c')


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


def shape_of(c, k):
    return (c['height'] + 1, c['width'] + 1) if k in Q.CORNER_ARRAYS else (c['height'], c['width'])


_RUNS = {}


def launch(name, arrays=Q.ARRAYS, shift=0, box=None):
    """One amt_georef_frame of a case into poisoned buffers of the test's own, each array `shift` doubles behind the start of
    its allocation and one guard element in front of the next thing -> dict(arrays, variant, bbox).  Asserts that every element
    was written and that nothing around the arrays was."""
    key = (name, tuple(arrays), shift, box)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from auromat_amd._native import GeorefOut
    c, ctx = K.by_name(name), _ctx()
    out, bufs = GeorefOut(), {}
    for k in arrays:
        n = int(np.prod(shape_of(c, k)))
        t = ctx.empty((n + shift + 1,))
        t.view(torch.uint8).fill_(POISON)
        assert t.data_ptr() % 16 == 0
        bufs[k] = t
        setattr(out, k, t.data_ptr() + 8 * shift)
    bbox = None
    if box is not None:
        bbox = ctx.empty((8,))
        bbox.view(torch.uint8).fill_(POISON)
        out.bbox, out.bbox_min_elevation = bbox.data_ptr(), float(box)
    p = K.native_params(c)
    ctx.call('amt_georef_frame', C.byref(p), C.byref(out))
    torch.cuda.synchronize()
    got = {}
    for k, t in bufs.items():
        flat = t.cpu().numpy()
        bits = flat.view(np.uint64)
        assert (bits[:shift] == POISON_F64).all() and bits[-1] == POISON_F64, (name, k, 'written outside the array')
        assert not (bits[shift:-1] == POISON_F64).any(), (name, k, 'elements the kernel did not write')
        got[k] = flat[shift:-1].reshape(shape_of(c, k)).copy()
    res = dict(arrays=got, variant=ctx.last_variant(), bbox=None if bbox is None else bbox.cpu().numpy())
    _RUNS[key] = res
    return res


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == 'f':
        return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


# ---- the arrays -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', K.names())
def test_every_element_against_the_reference(name):
    c, ref, run = K.by_name(name), K.reference(name), launch(name)
    got, bounds = run['arrays'], K.bounds(c['family'])
    assert run['variant'] == (1, 0, 1)
    failed = []
    for k in Q.ARRAYS:
        assert got[k].shape == ref[k].shape
        mism = np.argwhere(np.isnan(got[k]) != np.isnan(ref[k]))
        assert len(mism) == 0, '%s %s: NaN pattern differs at %s' % (name, k, mism[:6].tolist())
        d = Q.distance(k, got, ref)
        worst, at = float(d.max()), np.unravel_index(int(d.argmax()), d.shape)
        print('%s %s: kernel %.3e  E_ref %.3e  bound %.3e  (%.2f of the bound, at %s)' % (
            name, k, worst, K.e_ref(c['family'], k), bounds[k], worst / bounds[k], at))
        if not worst <= bounds[k]:
            failed.append((k, worst, bounds[k], at))
    assert not failed, (name, failed)
    # without the MLat / MLT pointers: SECOND = 0, the same bits in the other five arrays
    plain = launch(name, arrays=GEO)
    assert plain['variant'] == (0, 0, 1)
    for k in GEO:
        assert same_bits(plain['arrays'][k], got[k]), (name, k)


def test_largest_distances_per_family():
    """the table of the module docstring (-s); asserts again, per family, what the test above asserts per case"""
    share = (0.0, None)
    for fam in K.FAMILIES:
        bounds, cells = K.bounds(fam), []
        for k in Q.ARRAYS:
            worst = max(float(Q.distance(k, launch(c['name'])['arrays'], K.reference(c['name'])).max()) for c in K.family(fam))
            cells.append('%s %.1e / %.1e / %.1e' % (k, worst, K.e_ref(fam, k), bounds[k]))
            share = max(share, (worst / bounds[k], (fam, k)))
            assert worst <= bounds[k], (fam, k, worst, bounds[k])
        print('  %-9s' % fam + ';  '.join(cells))
    print('  largest share of a bound: %.3f %s' % share)


def test_longitudes_stay_in_their_range():
    for name in K.names():
        got = launch(name)['arrays']
        for k in ('lon', 'lon_c'):
            v = got[k][~np.isnan(got[k])]
            assert np.all(np.abs(v) <= 180.0), (name, k)
        for k in ('mlt', 'mlt_c'):
            v = got[k][~np.isnan(got[k])]
            assert np.all((v >= 0.0) & (v <= 24.0)), (name, k)


# ---- sky bands on the device ------------------------------------------------------------------------------------------------------
def sky_rows(c):
    from auromat_amd import _native
    p = K.native_params(c)
    out = [C.c_int32(0) for _ in range(4)]
    assert _native.lib().amt_georef_sky_rows(C.byref(p), *[C.byref(o) for o in out]) == 0
    return [o.value for o in out]


def test_cases_with_sky_bands_cover_the_fill():
    """1, 2 and 3 strips (fill_nan split among as many waves), bands above and below, the last corner row inside a band, a frame
    that is all sky, and cases whose bands the gate refuses although rows of sky exist"""
    names = [c['name'] for c in K.cases() if sky_rows(c)[2] > 0 or sky_rows(c)[3] < sky_rows(c)[1]]
    assert sorted(names) == sorted(K.SKY_BAND_NAMES)
    strips = {(K.by_name(n)['width'] + 1 + 62) // 63 for n in names}
    assert {1, 2, 3} <= strips, strips
    top = [n for n in names if sky_rows(K.by_name(n))[2] > 0]
    bottom = [n for n in names if sky_rows(K.by_name(n))[3] < sky_rows(K.by_name(n))[1]]
    assert 'far-disc-inside' in top and 'far-disc-inside' in bottom and 'low-sky' in top and 'limb-above+0' in bottom
    assert len(names) >= 25
    for n in ('wide-gate-0.52', 'far-gate-refuses'):
        assert n not in names and np.isnan(K.reference(n)['lat']).all(axis=1).any()


@pytest.mark.parametrize('name', K.SKY_BAND_NAMES)
def test_sky_bands_are_nan_whatever_the_alignment(name):
    c = K.by_name(name)
    rows, n, top, bottom = sky_rows(c)
    h = c['height']
    base = launch(name)['arrays']
    for shift in (0, 1):                                         # bases at 0 and at 8 mod 16 bytes
        got = launch(name, shift=shift)['arrays']                # (asserts: every element written, the guards untouched)
        for band in list(range(top)) + list(range(bottom, n)):
            r0, r1 = band * rows, min((band + 1) * rows, h)
            for k in Q.ARRAYS:
                part = got[k][r0:r1 + (1 if r1 == h else 0)] if k in Q.CORNER_ARRAYS else got[k][r0:r1]
                assert np.isnan(part).all(), (name, shift, band, k)
        for k in Q.ARRAYS:
            assert same_bits(got[k], base[k]), (name, shift, k)
    five = launch(name, arrays=GEO, shift=1)['arrays']
    for k in GEO:
        assert same_bits(five[k], base[k]), (name, k)


# ---- the in-kernel box --------------------------------------------------------------------------------------------------------------
def check_box(tag, got, want, lats, bounds):
    for k in range(6):
        d = Q.box_distance(k, float(got[k]), want[k], lats[k])
        b = bounds['lat' if k < 2 else 'lon']
        assert d <= b, (tag, 'slot', k, float(got[k]), want[k], d, b)


@pytest.mark.parametrize('min_elevation', [NEG_INF, 10.0])
@pytest.mark.parametrize('name', K.names())
def test_kernel_box(name, min_elevation):
    c, ref = K.by_name(name), K.reference(name)
    run = launch(name, arrays=GEO, box=min_elevation)
    slots, lats, count = Q.kernel_box(c, ref, min_elevation)
    got = run['bbox']
    print(name, min_elevation, 'box', got[:7].tolist(), 'reference', slots, count)
    assert got[6] == count, (name, got[6], count)
    check_box((name, min_elevation), got, slots, lats, K.bounds(c['family']))
    for k in GEO:                                                # the box changes nothing in the arrays
        assert same_bits(run['arrays'][k], launch(name)['arrays'][k]), (name, k)


def test_exact_centres_count_only_pixels_with_four_corners():
    """the rule the test above holds the kernel to is not vacuous: the exact family has pixels whose centre is above the
    threshold while a corner misses, and the reference's count leaves them out"""
    seen = 0
    for c in K.family('exact'):
        ref = K.reference(c['name'])
        hit = ~np.isnan(ref['lat'])
        four = hit[:-1, :-1] & hit[:-1, 1:] & hit[1:, 1:] & hit[1:, :-1]
        centre = ~np.isnan(ref['elev'])
        seen += int((centre & ~four).sum())
        assert Q.kernel_box(c, ref, NEG_INF)[2] == int((centre & four).sum())
        assert launch(c['name'], arrays=GEO, box=NEG_INF)['bbox'][6] == int((centre & four).sum())
    assert seen >= 100


# ---- the coarse box -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', K.names())
def test_coarse_box(name):
    import torch
    c, ref, ctx = K.by_name(name), K.reference(name), _ctx()
    p, bounds = K.native_params(c), K.bounds(c['family'])
    for stride in (1, 7, 16, max(c['width'], c['height']) + 5):
        for magnetic in (0, 1):
            for min_elevation in (NEG_INF, 10.0):
                bbox = ctx.empty((8,))
                bbox.view(torch.uint8).fill_(POISON)
                ctx.call('amt_georef_coarse_bbox', C.byref(p), stride, min_elevation, magnetic, C.c_void_p(bbox.data_ptr()))
                got = bbox.cpu().numpy()
                slots, lats, count, hint = Q.coarse_box(c, ref, stride, min_elevation, bool(magnetic))
                tag = (name, stride, magnetic, min_elevation)
                assert got[6] == count and got[7] == hint, (tag, got[6:].tolist(), count, hint)
                mb = dict(lat=bounds['mlat'], lon=bounds['mlt']) if magnetic else bounds
                check_box(tag, got, slots, lats, mb)


# ---- MLat / MLT only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', K.names())
def test_mlat_mlt_only_is_bit_identical(name):
    """amt_georef_frame asked for the elevation and the four magnetic arrays alone (what BaseAstrometryMapping.mLatMlt asks
    for) runs SECOND = 4"""
    run, nine = launch(name, arrays=('elev',) + MAG), launch(name)
    assert run['variant'] == (4, 0, 1), run['variant']
    for k in ('elev',) + MAG:
        assert same_bits(run['arrays'][k], nine['arrays'][k]), (name, k)


# ---- the two plans ------------------------------------------------------------------------------------------------------------------
PX_PER_DEG = {'cd': 40, 'wide': 2, 'limb': 4, 'far': 1, 'low': 20, 'inside': 6, 'exact': 4, 'dateline': 40}
PLAN_PX_PER_DEG = {'exact-cd-sheared': 40, 'low-ground': 40}


def plan_settings(c):
    ppd = PLAN_PX_PER_DEG.get(c['name'], PX_PER_DEG[c['family']])
    return ppd, (10 if c['family'] in ('cd', 'far') or c['name'] in PLAN_PX_PER_DEG else None)


def image_of(c, dtype):
    rng = np.random.RandomState(c['width'] * 131 + c['height'])
    return rng.randint(0, np.iinfo(dtype).max + 1, size=(c['height'], c['width'], 3)).astype(dtype)


@pytest.mark.parametrize('name', K.PLAN_NAMES)
def test_plans_are_bit_identical(name):
    from auromat_amd.pipeline import FramePipeline
    c = K.by_name(name)
    ppd, min_elevation = plan_settings(c)
    for dtype in (np.uint8, np.uint16):
        pipe = FramePipeline(c['width'], c['height'], img_dtype=dtype, with_mag=True)
        img = image_of(c, dtype)
        for fast in (True, False):
            res, arrays, plans = [], [], []
            for fuse in (True, False):
                r = pipe.run(c['header'], c['altitude'], c['cam'], c['time'], img=img, fast=fast, min_elevation=min_elevation,
                             pxPerDeg=ppd, fuse=fuse)
                plans.append(pipe.last_plan)
                if fuse:
                    assert pipe.ctx.last_variant() == (1, 1 if dtype == np.uint8 else 2, 1)
                res.append({k: np.array(r[k]) for k in ('mean', 'count', 'img', 'mask')})
                arrays.append({k: np.array(v) for k, v in pipe.host_arrays().items()})
            print(name, np.dtype(dtype).name, 'fast' if fast else 'exact', plans, res[0]['mean'].shape, int(res[0]['count'].sum()))
            assert plans == ['single-pass', 'two-pass'], (name, dtype, fast, plans)
            for k in res[0]:
                assert same_bits(res[0][k], res[1][k]), (name, dtype, fast, 'grid', k)
            assert set(arrays[0]) == set(Q.ARRAYS)
            for k in arrays[0]:
                assert same_bits(arrays[0][k], arrays[1][k]), (name, dtype, fast, 'array', k)
                if bool(fast) == bool(c['fast_center']):
                    assert same_bits(arrays[1][k], launch(name)['arrays'][k]), (name, 'array of the plain entry point', k)
            assert res[0]['count'].sum() > 0


MAG_GRID_NAMES = ('cd-rotation-37', 'limb-below+0.5', 'wide-ellipse', 'exact-diagonal+37')


@pytest.mark.parametrize('name', MAG_GRID_NAMES)
def test_mlat_mlt_only_grid_is_bit_identical(name):
    """resampleMLatMLT's pipeline (with_geo=False: the single-pass launch on the (MLat, SM longitude) grid runs SECOND = 4)
    against the pipeline that keeps all nine arrays: the same grid and the same kept arrays"""
    from auromat_amd.pipeline import FramePipeline
    c = K.by_name(name)
    ppd, min_elevation = plan_settings(c)
    img = image_of(c, np.uint16)
    out = []
    for with_geo in (False, True):
        pipe = FramePipeline(c['width'], c['height'], with_mag=True, with_geo=with_geo)
        r = pipe.run(c['header'], c['altitude'], c['cam'], c['time'], img=img, fast=bool(c['fast_center']),
                     min_elevation=min_elevation, pxPerDeg=ppd, fuse=True, magnetic=True)
        assert pipe.last_plan == 'single-pass'
        assert pipe.ctx.last_variant() == (1 if with_geo else 4, 2, 1)
        kept = pipe.host_arrays(kept_only=True)
        out.append((dict((k, np.array(r[k])) for k in ('mean', 'count', 'img', 'mask')), {k: np.array(kept[k]) for k in ('elev',) + MAG}))
    for k in out[0][0]:
        assert same_bits(out[0][0][k], out[1][0][k]), (name, 'grid', k)
    for k in out[0][1]:
        assert same_bits(out[0][1][k], out[1][1][k]), (name, 'array', k)
        assert same_bits(out[0][1][k], launch(name)['arrays'][k]), (name, 'array of the plain entry point', k)
