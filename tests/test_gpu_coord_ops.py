"""
The 19 operator kernels of auromat_amd/csrc/amt_coords.hip on the constructed inputs of tests/_coord_cases.py: every case goes
through the C ABI (ctx.call) on device tensors, every output into a buffer of the test's own with 64 elements to spare, pre-filled
with a poison byte, and EVERY element is compared with the longdouble / mpmath reference of tests/_coord_oracle.py.
tests/test_coord_cases_cpu.py checks without a GPU that the inputs hold what they claim and that the reference is right.

Per case: every element below n is written and the spare tail is untouched; NaN patterns and the bytes of
amt_intersects_ellipsoid are identical to the reference's; distances in degrees or km — |d lat|, |d lon wrapped| cos(lat), |d MLT
wrapped at 24 h| 15 cos(MLat), azimuth wrapped at 360, absolute km, absolute components of unit vectors (radians are converted to
degrees in longdouble first) — stay within 8 max(E_ref, eps scale, S) per family, entry point and output: E_ref the distance of
the float64 oracle (oracle/ref_numpy.py) from the same reference on the same inputs, scale 90 or 180 deg, the largest coordinate
in km, or 1; S = 4.1e-15 scale for the outputs behind a hardware seed refined by one Newton step (amt_common.h), else 0.  There
is no floor.  The SIP tables of amt_directions_zenithal go to the device with every entry p + q > order set to 1e30.

Then: amt_rotate_pole_deg equals amt_rotate_pole on lat kDeg2Rad, lon kDeg2Rad times kRad2Deg bit for bit; the all-sky kernel
gives the same bits whichever subset of its outputs is asked for; empty frames are refused; and the public functions
(ecef2Geodetic, geodetic2Ecef, rotatePole, ellipsoidLineIntersection, sphereLineIntersection, tan_pix2world) keep shapes and
give the bits of the C ABI on (3, 5)-shaped, non-contiguous and empty inputs.

Largest values measured on the MI355X per family — of the angles, of the positions and of the unit vectors the output that
comes nearest to its bound — as kernel distance / E_ref / bound (degrees; km for xyz, r and x y z; printed per case and per
family, entry point and output with -s):
  lengths     georef_allsky el 2.8e-14 / 2.8e-14 / 2.3e-13;  intersect_sphere xyz 3.9e-12 / 1.4e-12 / 1.1e-11;  directions_tan_points dirs 2.1e-16 / 1.9e-16 / 1.8e-15
  stride      ecef_to_geodetic lat 1.1e-13 / 1.4e-14 / 3.0e-12;  rotate_vectors xyz 1.3e-12 / 1.3e-12 / 1.3e-11
  geodetic    ecef_to_geodetic lat 1.2e-14 / 7.5e-15 / 3.0e-12;  geodetic_to_ecef z 2.5e-12 / 7.4e-13 / 2.4e-10
  rotate_pole rotate_pole lat 3.0e-14 / 1.2e-14 / 3.0e-12
  rays        intersect_sphere xyz 7.1e-10 / 1.2e-10 / 9.6e-10
  magnetic    rotate_to_mlat_mlt mlat 1.7e-14 / 1.7e-14 / 1.6e-13;  rotate_vectors xyz 1.0e-12 / 1.0e-12 / 1.3e-11
  wcs         directions_zenithal dirs 2.4e-16 / 2.3e-16 / 1.9e-15
  allsky      georef_allsky az 1.3e-13 / 1.4e-13 / 1.1e-12;  georef_allsky dirs 1.9e-15 / 1.9e-15 / 1.5e-14
  themis      reproject_altitude lat 1.0e-13 / 5.1e-14 / 3.0e-12
The seeded outputs stay below 1.3e-13 deg (reproject_altitude; Bowring alone 1.1e-13 deg on the stride case, 1.2e-15 of 90 deg)
against bounds of 3.0e-12 and 5.9e-12 deg that S sets; everything else follows E_ref or eps scale, and only the sphere beside
the tangent cone (0.74) takes more than 0.4 of its bound.
"""
import ctypes as C

import numpy as np
import pytest

import _coord_cases as K
import _coord_oracle as Q

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_F64 = np.frombuffer(bytes([POISON] * 8), dtype=np.uint64)[0]
SPARE = 64
SIP_POISON = 1e30


# the 19 entry points of amt_coords.hip, by the operation names of tests/_coord_oracle.py
ENTRY = dict(
    intersect_ellipsoid='amt_intersect_ellipsoid', intersects_ellipsoid='amt_intersects_ellipsoid',
    intersect_sphere='amt_intersect_sphere', ecef_to_geodetic='amt_ecef_to_geodetic', geodetic_to_ecef='amt_geodetic_to_ecef',
    rotate_to_latlon='amt_rotate_to_latlon', rotate_to_mlat_mlt='amt_rotate_to_mlat_mlt', rotate_vectors='amt_rotate_vectors',
    latlon_to_mlat_mlt='amt_latlon_to_mlat_mlt', sm_to_latlon='amt_sm_to_latlon',
    cartesian_to_spherical='amt_cartesian_to_spherical', spherical_to_cartesian='amt_spherical_to_cartesian',
    rotate_pole='amt_rotate_pole', rotate_pole_deg='amt_rotate_pole_deg', directions_tan='amt_directions_tan',
    directions_tan_points='amt_directions_tan_points', directions_zenithal='amt_directions_zenithal',
    georef_allsky='amt_georef_allsky', reproject_altitude='amt_reproject_altitude')
assert set(ENTRY) == set(Q.OPS)


def _ctx():
    from auromat_amd._native import Context
    return Context.current()


class Out(object):
    """an output buffer of `n` elements and SPARE more, poisoned"""

    def __init__(self, n, width=1, byte=False):
        import torch
        self.n, self.width, self.byte = n, width, byte
        self.t = _ctx().empty((n * width + SPARE,), torch.uint8 if byte else None)
        self.t.view(torch.uint8).fill_(POISON)
        self.ptr = C.c_void_p(self.t.data_ptr())

    def host(self, what):
        """the n elements, after checking that all of them were written and nothing behind them"""
        a = self.t.cpu().numpy()
        head, tail = a[:self.n * self.width], a[self.n * self.width:]
        if self.byte:
            assert np.all(head <= 1), (what, 'bytes the kernel did not write')
            assert np.all(tail == POISON), (what, 'bytes written behind the end')
            return head.copy()
        assert not (head.view(np.uint64) == POISON_F64).any(), (what, 'elements the kernel did not write',
                                                              np.nonzero(head.view(np.uint64) == POISON_F64)[0][:4].tolist())
        assert np.all(tail.view(np.uint64) == POISON_F64), (what, 'elements written behind the end')
        return head.reshape(self.n, self.width).copy() if self.width > 1 else head.copy()


def dev(a):
    return _ctx().to_device(np.ascontiguousarray(a, dtype=np.float64))


def p_(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def frame_params(A):
    from auromat_amd._native import FrameParams
    p = FrameParams()
    p.width, p.height = int(A['width']), int(A['height'])
    p.cd[:] = [float(v) for v in A['cd']]
    p.crpix[:] = [float(v) for v in A['crpix']]
    p.rot[:] = [float(v) for v in np.asarray(A['rot']).ravel()]
    return p


def allsky_struct(A):
    from auromat_amd._native import AllSkyParams
    p = AllSkyParams()
    p.size = int(A['size'])
    p.xc, p.yc, p.k, p.rotation, p.center_offset = A['xc'], A['yc'], A['k'], A['rotation'], A['center_offset']
    p.to_geo[:] = [float(v) for v in np.asarray(A['to_geo']).ravel()]
    p.station[:] = [float(v) for v in A['station']]
    p.a, p.b, p.a0, p.b0 = A['a'], A['b'], A['a0'], A['b0']
    return p


def zenithal_struct(A):
    """the case's block with every SIP entry beyond the orders set to a large finite number: the kernel must not read them"""
    from auromat_amd._native import SIP_MAX, ZenithalWcs
    w = ZenithalWcs()
    C.memmove(C.byref(w), C.byref(A['w']), C.sizeof(ZenithalWcs))
    for table, order in ((w.sip_a, w.sip_order_a), (w.sip_b, w.sip_order_b)):
        for p in range(SIP_MAX):
            for q in range(SIP_MAX):
                if p + q > order:
                    table[p][q] = SIP_POISON
    return w


def call(op, A, want=None):
    """One launch of amt_<op> on poisoned buffers -> dict of output -> host array (float64 in the entry point's own units).
    `want`: the subset of the all-sky outputs to ask for."""
    import torch
    from auromat_amd._native import host3, host9
    ctx, name = _ctx(), ENTRY[op]
    n = Q.n_points(op, A)
    keep = []                                                  # device inputs stay alive until the call has run

    def inp(a):
        keep.append(dev(a))
        return p_(keep[-1])
    if op in ('intersect_ellipsoid', 'intersects_ellipsoid'):
        o = Out(n, 3) if op == 'intersect_ellipsoid' else Out(n, byte=True)
        ctx.call(name, float(A['a']), float(A['b']), host3(A['origin']), inp(A['dirs']), n, int(A['directed']), o.ptr)
        outs = {'xyz' if op == 'intersect_ellipsoid' else 'hit': o}
    elif op == 'intersect_sphere':
        o = Out(n, 3)
        ctx.call(name, float(A['radius']), host3(A['origin']), inp(A['dirs']), n, int(A['directed']), o.ptr)
        outs = dict(xyz=o)
    elif op == 'ecef_to_geodetic':
        outs = dict(lat=Out(n), lon=Out(n))
        ctx.call(name, inp(A['x']), inp(A['y']), inp(A['z']), n, float(A['a']), float(A['b']), outs['lat'].ptr, outs['lon'].ptr)
    elif op == 'geodetic_to_ecef':
        outs = dict(x=Out(n), y=Out(n), z=Out(n))
        ctx.call(name, inp(A['lat']), inp(A['lon']), float(A['h']), n, float(A['a']), float(A['b']), outs['x'].ptr, outs['y'].ptr,
                 outs['z'].ptr)
    elif op == 'rotate_to_latlon':
        outs = dict(lat=Out(n), lon=Out(n))
        ctx.call(name, host9(A['m']), inp(A['xyz']), n, float(A['a']), float(A['b']), outs['lat'].ptr, outs['lon'].ptr)
    elif op == 'rotate_to_mlat_mlt':
        outs = dict(mlat=Out(n), mlt=Out(n))
        ctx.call(name, host9(A['m']), inp(A['xyz']), n, outs['mlat'].ptr, outs['mlt'].ptr)
    elif op == 'rotate_vectors':
        outs = dict(xyz=Out(n, 3))
        ctx.call(name, host9(A['m']), inp(A['xyz']), n, outs['xyz'].ptr)
    elif op == 'latlon_to_mlat_mlt':
        outs = dict(mlat=Out(n), mlt=Out(n))
        ctx.call(name, host9(A['m']), inp(A['lat']), inp(A['lon']), float(A['h']), n, float(A['a']), float(A['b']),
                 outs['mlat'].ptr, outs['mlt'].ptr)
    elif op == 'sm_to_latlon':
        outs = dict(lat=Out(n), lon=Out(n))
        ctx.call(name, host9(A['m']), inp(A['smlat']), inp(A['smlon']), n, float(A['a']), float(A['b']), outs['lat'].ptr,
                 outs['lon'].ptr)
    elif op == 'cartesian_to_spherical':
        outs = dict(lat=Out(n), lon=Out(n))
        if A['with_r']:
            outs['r'] = Out(n)
        ctx.call(name, inp(A['x']), inp(A['y']), inp(A['z']), n, outs['r'].ptr if A['with_r'] else None, outs['lat'].ptr,
                 outs['lon'].ptr)
    elif op == 'spherical_to_cartesian':
        outs = dict(x=Out(n), y=Out(n), z=Out(n))
        ctx.call(name, None if A['r'] is None else inp(A['r']), inp(A['lat']), inp(A['lon']), n, outs['x'].ptr, outs['y'].ptr,
                 outs['z'].ptr)
    elif op in ('rotate_pole', 'rotate_pole_deg'):
        outs = dict(lat=Out(n), lon=Out(n))
        ctx.call(name, host9(A['rot']), inp(A['lat']), inp(A['lon']), float(A['altitude']), n, float(A['a']), float(A['b']),
                 outs['lat'].ptr, outs['lon'].ptr)
    elif op == 'directions_tan':
        outs = dict(dirs=Out(n, 3))
        p = frame_params(A)
        ctx.call(name, C.byref(p), int(A['corner']), outs['dirs'].ptr)
    elif op == 'directions_tan_points':
        outs = dict(dirs=Out(n, 3))
        p = frame_params(A)
        ctx.call(name, C.byref(p), inp(A['px']), inp(A['py']), n, int(A['origin']), outs['dirs'].ptr)
    elif op == 'directions_zenithal':
        outs = dict(dirs=Out(n, 3))
        w = zenithal_struct(A)
        ctx.call(name, C.byref(w), outs['dirs'].ptr)
    elif op == 'georef_allsky':
        want = want or ('az', 'el', 'dirs', 'lat', 'lon')
        outs = {k: Out(n, 3 if k == 'dirs' else 1) for k in want}
        p = allsky_struct(A)
        ctx.call(name, C.byref(p), int(A['corner']), *[outs[k].ptr if k in outs else None for k in ('az', 'el', 'dirs', 'lat', 'lon')])
    elif op == 'reproject_altitude':
        outs = dict(lat=Out(n), lon=Out(n))
        ctx.call(name, float(A['station_lat']), float(A['station_lon']), inp(A['lat']), inp(A['lon']), n, float(A['height_ref']),
                 float(A['height_new']), float(A['a']), float(A['b']), outs['lat'].ptr, outs['lon'].ptr)
    else:
        raise KeyError(op)
    torch.cuda.synchronize()
    return {k: o.host((op, k)) for k, o in outs.items()}


_RUNS = {}


def kernel_outputs(name):
    if name not in _RUNS:
        c = K.by_name(name)
        _RUNS[name] = call(c['op'], c['args'])
    return _RUNS[name]


def compare(c, echo=True):
    """-> list of (output, worst distance, bound, index) that miss their bound; patterns are asserted"""
    name, op = c['name'], c['op']
    got, ref = kernel_outputs(name), K.reference(name)
    cmp_, failed = Q.comparable(op, got), []
    for out, kind in K.outputs(c):
        assert got[out].shape == ref[out].shape, (name, out, got[out].shape, ref[out].shape)
        if kind == 'hit':
            mism = np.nonzero(got[out] != np.asarray(ref[out], np.uint8))[0]
            assert len(mism) == 0, '%s: bytes differ at %s' % (name, mism[:6].tolist())
            continue
        mism = np.argwhere(np.isnan(got[out]) != np.isnan(ref[out]))
        assert len(mism) == 0, '%s %s: NaN pattern differs at %s' % (name, out, mism[:6].tolist())
        if kind == 'az':                                        # (the distance below is taken modulo 360)
            assert np.all((got[out] >= 0) & (got[out] < 360)), '%s: azimuths outside [0, 360): %s' % (
                name, got[out][(got[out] < 0) | (got[out] >= 360)][:4].tolist())
        d = Q.distance(op, out, cmp_, ref)
        worst = float(d.max()) if d.size else 0.0
        at = np.unravel_index(int(d.argmax()), d.shape) if d.size else ()
        e_ref, bound = K.e_ref(c['family'], op, out), K.bound(c['family'], op, out)
        if echo:
            print('%s %s: kernel %.3e  E_ref %.3e  bound %.3e  (%.2f of the bound, at %s)' % (name, out, worst, e_ref, bound,
                                                                                             worst / bound if bound else 0, at))
        if not worst <= bound:
            failed.append((out, worst, bound, at))
    return failed


@pytest.mark.parametrize('name', K.names())
def test_every_element_against_the_reference(name):
    failed = compare(K.by_name(name))
    assert not failed, (name, failed)


def test_largest_distances_per_family():
    """the table of the module docstring (-s); asserts again, per family, what the test above asserts per case"""
    for fam in K.FAMILIES:
        for op, out in K.keys(fam):
            worst = 0.0
            for c in K.family(fam):
                if c['op'] == op and out in dict(K.outputs(c)):
                    d = Q.distance(op, out, Q.comparable(op, kernel_outputs(c['name'])), K.reference(c['name']))
                    worst = max(worst, float(d.max()) if d.size else 0.0)
            bound = K.bound(fam, op, out)
            print('  %-11s %-22s %-4s %.1e / %.1e / %.1e' % (fam, op, out, worst, K.e_ref(fam, op, out), bound))
            assert worst <= bound, (fam, op, out, worst, bound)


def test_special_values_come_out_exactly():
    """what no tolerance should have to cover: the half turn of y = +-0 at x < 0, MLT 24 and 0, the zenith pixel"""
    for tag in ('wgs84', 'flat'):
        c = K.by_name('geodetic-from-ecef-%s-special' % tag)
        got = kernel_outputs(c['name'])
        assert got['lon'][c['half_turn']].tolist() == [np.pi, -np.pi, np.pi, -np.pi]
        assert np.isnan(got['lat'][c['on_axis']]).all() and not np.isnan(got['lon']).any()
        want = np.arctan2(c['args']['y'], c['args']['x'])[c['on_axis']]           # 0 or +-pi by the signs of the zeros
        assert np.array_equal(got['lon'][c['on_axis']], want)
    c = K.by_name('magnetic-mlt-zero')
    got = kernel_outputs(c['name'])
    assert np.all(np.abs(np.abs(got['mlt'][c['midnight']] - 12.0) - 12.0) < 1e-14), got['mlt'][c['midnight']]
    assert got['mlt'][c['midnight']][0] > 12 > got['mlt'][c['midnight']][1]
    assert got['mlat'][c['axis']].tolist() == [90.0, -90.0]
    for c in K.family('allsky'):
        got, A = kernel_outputs(c['name']), c['args']
        assert np.all((got['az'] >= 0) & (got['az'] < 360)), c['name']
        if c['zenith'] is not None:
            n, off = A['size'] + A['corner'], 0.0 if A['corner'] else 0.5
            i = int(c['zenith'][0] - off) * n + int(c['zenith'][1] - off)
            assert got['el'][i] == 90.0, (c['name'], got['el'][i])


def test_rotate_pole_in_degrees_is_the_radian_kernel_bit_for_bit():
    """amt_rotate_pole_deg(lat, lon) == amt_rotate_pole(lat kDeg2Rad, lon kDeg2Rad) kRad2Deg, the products NumPy's: the two
    instances of k_rotate_pole share rotate_pole_rad, written with contraction off"""
    seen = 0
    for c in K.family('rotate_pole') + [c for c in K.family('lengths') if c['op'] == 'rotate_pole_deg']:
        if c['op'] != 'rotate_pole_deg':
            continue
        A = c['args']
        deg = kernel_outputs(c['name'])
        rad = call('rotate_pole', dict(A, lat=A['lat'] * K.K_DEG2RAD, lon=A['lon'] * K.K_DEG2RAD))
        for k in ('lat', 'lon'):
            want = rad[k] * K.K_RAD2DEG
            assert np.array_equal(deg[k].view(np.uint64), want.view(np.uint64)), (c['name'], k)
        seen += len(A['lat'])
    assert seen > 500


@pytest.mark.parametrize('name', [c['name'] for c in K.family('allsky')][::3] + ['lengths-georef_allsky-16-1'])
def test_allsky_outputs_do_not_depend_on_which_are_asked_for(name):
    c = K.by_name(name)
    full = kernel_outputs(name)
    for subset in K.ALLSKY_SUBSETS:
        got = call('georef_allsky', c['args'], want=subset)
        assert set(got) == set(subset)
        for k in subset:
            assert np.array_equal(got[k].view(np.uint64), full[k].view(np.uint64)), (name, subset, k)


def test_empty_frames_are_refused_and_empty_arrays_accepted():
    from auromat_amd._native import NativeError
    o = Out(0, 3)
    p = frame_params(dict(K.tan_args(K.tan_header(4, 4)), width=0, height=4))
    with pytest.raises(NativeError):
        _ctx().call('amt_directions_tan', C.byref(p), 0, o.ptr)
    w = zenithal_struct(K.by_name('wcs-zenithal-ARC-1x1')['args'])
    w.height = 0
    with pytest.raises(NativeError):
        _ctx().call('amt_directions_zenithal', C.byref(w), o.ptr)
    a = allsky_struct(K.by_name('allsky-1-corner0-rot0')['args'])
    a.size = 0
    with pytest.raises(NativeError):
        _ctx().call('amt_georef_allsky', C.byref(a), 0, None, None, o.ptr, None, None)
    assert o.host('refused').shape == (0, 3)                   # nothing was written
    for c in K.family('lengths'):
        if Q.n_points(c['op'], c['args']) == 0:
            assert all(v.size == 0 for v in kernel_outputs(c['name']).values())


def test_allsky_params_of_the_product_are_the_numbers_of_the_cases():
    """mapping.miracle.allsky_params (its station comes from amt_geodetic_to_ecef) against the cases' float64 numbers"""
    from collections import namedtuple
    from auromat_amd.mapping.miracle import allsky_params
    Cal = namedtuple('Cal', 'lat lon xc yc k rotation')
    A = K.by_name('allsky-33-corner0-rot0.3')['args']
    p = allsky_params(Cal(**A['cal']), A['size'], 110.0)
    assert list(p.to_geo) == list(np.asarray(A['to_geo']).ravel())
    assert (p.xc, p.yc, p.k, p.rotation, p.a, p.b, p.a0, p.b0) == (A['xc'], A['yc'], A['k'], A['rotation'], A['a'], A['b'], A['a0'],
                                                                    A['b0'])
    assert np.max(np.abs(np.array(list(p.station)) - A['station'])) <= 8 * 4.1e-15 * 6400


# ---- the public functions -------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _shapes(flat15):
    """a (3, 5) array, a non-contiguous view of the same numbers, and an empty one"""
    a = np.ascontiguousarray(flat15.reshape(3, 5))
    wide = np.zeros((3, 10))
    wide[:, ::2] = a
    return (('3x5', a), ('strided', wide[:, ::2]), ('empty', np.zeros((0, 5))))


def test_public_functions_keep_shapes_and_the_bits_of_the_c_abi():
    from auromat_amd.coordinates.intersection import ellipsoidLineIntersection, sphereLineIntersection
    from auromat_amd.coordinates.transform import ecef2Geodetic, geodetic2Ecef, rotatePole
    from auromat_amd.coordinates.wcs import tan_pix2world
    rng = np.random.RandomState(3)
    p = K.points_xyz(15, 77)
    lat, lon = np.deg2rad(rng.uniform(-89, 89, 15)), np.deg2rad(rng.uniform(-180, 180, 15))
    a, b = K.A0, K.B0
    for (tag, x), (_, y), (_, z) in zip(_shapes(p[:, 0]), _shapes(p[:, 1]), _shapes(p[:, 2])):
        assert tag == 'empty' or not (tag == 'strided' and x.flags.c_contiguous)
        la, lo = ecef2Geodetic(x, y, z)
        want = call('ecef_to_geodetic', dict(x=x.ravel(), y=y.ravel(), z=z.ravel(), a=a, b=b))
        assert la.shape == lo.shape == x.shape
        assert _same_bits(la.ravel(), want['lat']) and _same_bits(lo.ravel(), want['lon']), tag
    for (tag, la), (_, lo) in zip(_shapes(lat), _shapes(lon)):
        got = geodetic2Ecef(la, lo, 110.0)
        want = call('geodetic_to_ecef', dict(lat=la.ravel(), lon=lo.ravel(), h=110.0, a=a, b=b))
        assert all(g.shape == la.shape for g in got)
        assert all(_same_bits(g.ravel(), want[k]) for g, k in zip(got, 'xyz')), tag
    # rotatePole takes one-dimensional arrays only, as the reference does (transform.py:301-322)
    wide = np.zeros((2, 30))
    wide[:, ::2] = lat, lon
    for tag, la, lo in (('15', lat, lon), ('strided', wide[0, ::2], wide[1, ::2]), ('empty', np.zeros(0), np.zeros(0))):
        ola, olo = rotatePole(la, lo, 110.0, angle=-90)
        want = call('rotate_pole', dict(rot=K.ROTATIONS[1][1], lat=la, lon=lo, altitude=110.0, a=a, b=b))
        assert ola.shape == olo.shape == la.shape
        assert _same_bits(ola, want['lat']) and _same_bits(olo, want['lon']), tag
    # directions: (n, 3) for the ellipsoid, as the reference requires; any leading shape for the sphere, which broadcasts there
    d = K.aimed_dirs(15, 5)
    wide = np.zeros((15, 6))
    wide[:, ::2] = d
    for tag, dirs in (('15x3', d), ('strided', wide[:, ::2]), ('empty', np.zeros((0, 3)))):
        for directed in (True, False):
            got = ellipsoidLineIntersection(a + 110, b + 110, K.ORIGIN_OUT, dirs, directed=directed)
            want = call('intersect_ellipsoid', dict(a=a + 110, b=b + 110, origin=K.ORIGIN_OUT, dirs=dirs, directed=int(directed)))
            assert got.shape == dirs.shape and _same_bits(got, want['xyz'].reshape(dirs.shape)), tag
    for tag, dirs in (('3x5x3', d.reshape(3, 5, 3)), ('15x3', d), ('strided', wide[:, ::2]), ('empty', np.zeros((0, 3))),
                      ('single', d[0])):
        got = sphereLineIntersection(6481.0, K.ORIGIN_OUT, dirs)
        want = call('intersect_sphere', dict(radius=6481.0, origin=K.ORIGIN_OUT, dirs=dirs.reshape(-1, 3), directed=1))
        assert got.shape == dirs.shape, (tag, got.shape)
        assert _same_bits(got, want['xyz'].reshape(dirs.shape)), tag
    hdr = K.tan_header(64, 48, crpix=(31.0, 22.0))
    px, py = 20 + 30 * rng.uniform(size=15), 10 + 30 * rng.uniform(size=15)
    for (tag, x), (_, y) in zip(_shapes(px), _shapes(py)):
        for origin in (0, 1):
            got = tan_pix2world(hdr, x, y, origin, ascartesian=True)
            want = call('directions_tan_points', dict(K.tan_args(hdr), px=x.ravel(), py=y.ravel(), origin=origin))
            assert got.shape == x.shape + (3,) and _same_bits(got, want['dirs'].reshape(x.shape + (3,))), tag
        ra, dec = tan_pix2world(hdr, x, y, 0)
        assert ra.shape == dec.shape == x.shape
        assert np.all((ra >= 0) & (ra < 360)) and np.all(np.abs(dec) <= 90)
