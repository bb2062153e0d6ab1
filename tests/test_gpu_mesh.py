"""
Mesh resampling on the MI355X (auromat_amd.resample.resampleMesh, resampleMeshMLatMLT, resample_frame_mesh) on real geometry:
every cell of every output bit for bit against the NumPy statement of the contract (tests/_mesh_oracle.py).  The
oracle runs on the coordinates the device actually used — rotated centres are read back — so the last bits of the trigonometry
do not enter.  The kernels' paths and the rules that no frame controls are in tests/test_gpu_mesh_cells.py; that the oracle is
right is tests/test_mesh_cpu.py's matter.
"""
import os
from datetime import datetime

import numpy as np
import numpy.ma as ma
import pytest

import _mesh_cases as K
import _mesh_oracle as O
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

JPG = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.jpg')
WCS = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.wcs')
OUT_KEYS = ('mesh', 'img', 'mask', 'triangle')

# resample(method='linear') and the mesh in the cells where both interpolate in the same triangle: the largest difference
# measured on the MI355X is 5.8e-16 of a channel's span (the reference's frame at 10 px/deg: 2040 of the 4017 cells that both
# fill, 50.8 %; per channel 2.2e-16, 1.7e-16, 1.2e-16 for the colours and 5.8e-16 for the elevation); the bound is four times
# that, the project's habit for measured bounds.
LINEAR_MEASURED = 5.8e-16
LINEAR_BOUND = 4 * LINEAR_MEASURED


def _host(t):
    return None if t is None else t.cpu().numpy()


def used_case(fd, res, altitude, pole, disc, min_elevation=None):
    """The frame as the device used it, as an oracle case on the grid of the result."""
    from auromat_amd import resample as R
    lat_c, lon_c = fd.lat_c, fd.lon_c
    if pole:
        lat_c, lon_c = R._rotate_pole_dev(fd.ctx, fd.lat_c, fd.lon_c, altitude, 90)
    g = res['grid']
    img = fd.host_image()
    h, w = fd.height, fd.width
    img = np.zeros((h * w, 0), np.uint8) if img is None else np.asarray(img).reshape(h * w, -1)
    return K.MeshCase('frame', _host(lon_c).reshape(h, w), _host(lat_c).reshape(h, w), g.xedges, g.yedges, elev=_host(fd.elev),
                      mask=_host(fd.center_mask), min_elevation=float('-inf') if min_elevation is None else min_elevation,
                      lon_wrap=1 if (disc and not pole) else 0, img=img, cell_lon=g.lonCenters, cell_lat=g.latCenters)


def check_frame(fd, altitude, box, ppd, disc=False, pole=False, min_elevation=None, outline=None):
    from auromat_amd import resample as R
    res = R.resample_frame_mesh(fd, altitude, box, (ppd, ppd), disc, pole, min_elevation=min_elevation, outline=outline)
    case = used_case(fd, res, altitude, pole, disc, min_elevation)
    want = O.mesh_frame(case)
    assert res['mask'].dtype == bool and res['img'].dtype == case.img.dtype and res['triangle'].dtype == np.int32
    got = dict(res, mask=res['mask'].astype(np.uint8))
    for key in OUT_KEYS:
        assert O.same_bits(got[key], want[key]), key
    assert res['lat_c'].shape == res['mask'].shape == case.shape
    return res, want, case


def check_mapping(m, ppd):
    """resample_frame_mesh of the mapping's frame equals the oracle, and resampleMesh gives its image and elevation."""
    from auromat_amd import resample as R
    res, want, case = check_frame(m.frame(), m.altitude, m.boundingBox, ppd, m.containsDiscontinuity, m.containsPole,
                                  outline=m.outline if m.containsPole else None)
    r = R.resampleMesh(m, pxPerDeg=ppd)
    valid = want['mask'] == 0
    assert np.array_equal(~ma.getmaskarray(r.img)[..., 0], valid)
    assert np.array_equal(np.asarray(ma.getdata(r.img))[valid], want['img'][valid])
    assert np.array_equal(ma.filled(r.elevation, np.nan), want['mesh'][..., -1], equal_nan=True)
    return r, res, want, case


@pytest.fixture(scope='module')
def real_frame():
    from auromat_amd.mapping.spacecraft import getMapping
    return getMapping(JPG, WCS, altitude=110, fastCenterCalculation=True).maskedByElevation(10)


def test_reference_frame_equals_oracle(real_frame):
    r, res, want, case = check_mapping(real_frame, 10)
    filled = want['mask'] == 0
    assert case.lat_c.shape == (2832, 4256) and filled.sum() > 4000
    r.checkGuarantees()
    # every cell that centre binning fills lies inside the mesh, up to the rim (a cell whose eight neighbours are filled too is
    # not on it): a pixel at the border of the valid region is a vertex of the mesh's boundary, and a cell it falls into can
    # have its centre outside
    from auromat_amd.resample import resample
    mean = resample(real_frame, pxPerDeg=10)
    mean_filled = ~ma.getmaskarray(mean.img)[..., 0]
    assert mean_filled.shape == filled.shape
    inner = mean_filled.copy()
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            inner &= np.roll(np.roll(mean_filled, dr, 0), dc, 1)
    assert inner.sum() > 2000 and not (inner & ~filled).any()


def test_reference_frame_mlat_mlt(real_frame):
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import convertMappingToSM
    sm = convertMappingToSM(real_frame)
    r, res, want, case = check_mapping(sm, 10)
    assert (want['mask'] == 0).sum() > 4000
    geo = R.resampleMeshMLatMLT(real_frame, pxPerDeg=10)
    geo.checkGuarantees()
    assert np.array_equal(np.asarray(ma.getdata(geo.img)), np.asarray(ma.getdata(r.img)))
    assert np.array_equal(ma.getmaskarray(geo.img), ma.getmaskarray(r.img))


def test_fine_grid_on_a_window_has_no_holes(real_frame):
    """250 px/deg on a band of 24 rows and 700 columns of the frame (the oracle stays within seconds): no masked cell lies
    strictly inside a triangle of the mesh, and it fills holes of resample(method='mean'): that fills at most one cell per pixel."""
    from auromat_amd import resample as R
    from auromat_amd.frame import FrameData
    from auromat_amd.mapping.mapping import BoundingBox
    fd = real_frame.frame()
    r0, r1, c0, c1 = 1500, 1524, 1800, 2500
    cut = lambda name, extra=0: np.ascontiguousarray(
        np.asarray(fd.host(name)).reshape(fd.height + extra, fd.width + extra)[r0:r1 + extra, c0:c1 + extra])
    elev = cut('elev')
    img = np.asarray(fd.host_image()).reshape(fd.height, fd.width, -1)[r0:r1, c0:c1]
    lat, lon, lat_c, lon_c = cut('lat', 1), cut('lon', 1), cut('lat_c'), cut('lon_c')
    if fd.center_mask is not None:
        lat_c = np.where(cut('center_mask') != 0, np.nan, lat_c)
    band = FrameData.from_host(lat, lon, lat_c, lon_c, elev, np.ascontiguousarray(img))
    keep = np.isfinite(lat_c) & np.isfinite(lon_c)
    assert keep.sum() > 10000 and lon_c[keep].max() - lon_c[keep].min() < 90
    box = BoundingBox(lat_c[keep].min(), lon_c[keep].min(), lat_c[keep].max(), lon_c[keep].max())
    res, want, case = check_frame(band, real_frame.altitude, box, 250)
    masked = res['mask']
    inside = O.strictly_inside(case)
    assert inside.sum() > 10000 and not (masked & inside).any()
    mean = R.resample_frame(band, real_frame.altitude, box, (250, 250))
    holes = mean['mask'] & ~masked
    print('250 px/deg on %d x %d pixels: grid %s, mesh fills %d cells, %d of them holes of method=\'mean\' (which fills %d)'
          % (r1 - r0, c1 - c0, masked.shape, (~masked).sum(), holes.sum(), (~mean['mask']).sum()))
    assert mean['mask'].shape == masked.shape and holes.sum() >= max(1, (~masked).sum() - keep.sum())


def _miracle(name='miracle_sod64.npz', size=128, seed=1):
    from auromat_amd.mapping.mapping import BoundingBox
    from auromat_amd.mapping.miracle import CalibrationData, MIRACLEMapping
    z = load_golden(name)
    lat, lon = float(z['cal_lat']), float(z['cal_lon'])
    bb = BoundingBox(latSouth=lat + float(z['cal_lat_minus']), lonWest=lon + float(z['cal_lon_minus']),
                     latNorth=lat + float(z['cal_lat_plus']), lonEast=lon + float(z['cal_lon_plus']))
    cal = CalibrationData(station=str(z['cal_station']), validFrom=None, validTo=None, lat=lat, lon=lon, xc=float(z['cal_xc']),
                          yc=float(z['cal_yc']), k=float(z['cal_k']), rotation=float(z['cal_rotation']), boundingBoxSimple=bb)
    img = np.random.RandomState(seed).randint(0, 255, (size, size)).astype(np.uint8)
    return MIRACLEMapping(cal, img, datetime(2012, 3, 4, 17, 19, 0), 110).maskedByElevation(10)


def test_miracle_mapping_that_gather_refuses():
    from auromat_amd import resample as R
    m = _miracle()
    with pytest.raises(NotImplementedError):
        R.resampleGather(m, pxPerDeg=20)
    r, res, want, case = check_mapping(m, 20)
    filled = want['mask'] == 0
    assert filled.sum() > 500
    # an all-sky image: one connected disc, no hole inside it
    assert not (res['mask'] & O.strictly_inside(case)).any()


def test_collection_goes_member_by_member():
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import MappingCollection
    a, b = _miracle(), _miracle('miracle_kev96.npz', seed=2)
    coll = R.resampleMesh(MappingCollection([a, b], 'pair'), pxPerDeg=10)
    assert isinstance(coll, MappingCollection) and len(coll.mappings) == 2
    one = R.resampleMesh(b, pxPerDeg=10)
    assert np.array_equal(np.asarray(ma.getdata(one.img)), np.asarray(ma.getdata(coll.mappings[1].img)))
    assert (~ma.getmaskarray(one.img)).sum() > 100


def test_against_method_linear_where_the_triangles_coincide(real_frame):
    """resample(method='linear') is scipy's griddata, pinned to it by tests/test_gpu_nearest.py.  In the cells where its
    triangle (res['triangles']) has the vertices of the mesh's both evaluate the same linear function: see LINEAR_BOUND."""
    from auromat_amd import resample as R
    m = real_frame
    fd = m.frame()
    lin = R.resample_frame(fd, m.altitude, m.boundingBox, (10, 10), m.containsDiscontinuity, m.containsPole, method='linear',
                           outline=m.outline)
    res = R.resample_frame_mesh(fd, m.altitude, m.boundingBox, (10, 10), m.containsDiscontinuity, m.containsPole)
    assert np.array_equal(lin['lat_c'], res['lat_c']) and np.array_equal(lin['lon_c'], res['lon_c'])
    both = ~lin['mask'] & ~res['mask']
    case = used_case(fd, res, m.altitude, False, m.containsDiscontinuity)
    mine = np.sort(O.triangle_vertices(case, res['triangle'][both]), axis=1)
    theirs = np.sort(lin['triangles'][both], axis=1)
    same = (mine == theirs).all(axis=1)
    print('method=\'linear\' and the mesh: %d cells filled by both, %d (%.1f %%) in the same triangle'
          % (both.sum(), same.sum(), 100.0 * same.sum() / both.sum()))
    assert same.sum() >= 1000
    img = np.asarray(fd.host_image()).reshape(fd.height * fd.width, -1).astype(np.float64)
    elev = _host(fd.elev).reshape(-1)
    ok = O.vertices(case)[0]
    span = np.append(img[ok].max(axis=0) - img[ok].min(axis=0), elev[ok].max() - elev[ok].min())
    diff = np.abs(lin['mean'][both][same] - res['mesh'][both][same]).max(axis=0) / span
    print('largest difference per channel, of its span: %s (bound %.3g)' % (diff, LINEAR_BOUND))
    assert (diff <= LINEAR_BOUND).all()
