"""
The map-projected resampling on the MI355X (auromat_amd.resample.resampleStereographic, resampleStereographicMLatMLT,
resampleMLatMLTPolar) on real geometry: the golden frame georef_small_iss030_fast.npz (96 x 128 pixels) for the geographic form,
georef_small_iss029_fast.npz for the two magnetic forms, elevation >= 10 degrees.

Every output bit for bit against NumPy: tests/_area_plane_oracle.py + tests/_area_oracle.py applied to the plane coordinates that
``amt_project_forward`` returned (they are read back, so the last bits of the projection do not enter; the projection itself is
measured in tests/test_gpu_projection.py).  The coordinate arrays of the result against the mpmath inverse within the bound of that
file.  What the feature is for: the holes of centre binning — empty cells whose four edge neighbours are filled — are covered and
valid in the result.
"""
import datetime

import numpy as np
import numpy.ma as ma
import pytest

import _area_cases as AK
import _area_oracle as AO
import _area_plane_oracle as PO
import _projection_cases as K
import _projection_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUT_KEYS = ('area', 'img', 'mask', 'coverage')


def golden_mapping(name, rows=None, dtype=np.uint8, nch=3):
    """The golden frame as a GenericMapping with a seeded image, masked below 10 degrees of elevation; rows: a slice of them"""
    from auromat_amd.mapping.mapping import GenericMapping
    z = load_golden(name)
    h, w = z['lat_c'].shape
    img = np.random.RandomState(11).randint(0, int(np.iinfo(dtype).max) + 1, (h, w, nch)).astype(dtype)
    r0, r1 = rows or (0, h)
    t = datetime.datetime.strptime(str(z['time_iso'])[:19], '%Y-%m-%dT%H:%M:%S')
    m = GenericMapping(z['lat'][r0:r1 + 1], z['lon'][r0:r1 + 1], z['lat_c'][r0:r1], z['lon_c'][r0:r1], z['elev'][r0:r1],
                       float(z['altitude']), img[r0:r1], z['cam'], t, name)
    return m.maskedByElevation(10)


def plane_case(fd, x, y, xEdges, yEdges):
    """A frame as the device binned it: an oracle case on the plane grid"""
    host = lambda t: None if t is None else t.cpu().numpy()
    img = fd.host_image()
    return AK.AreaCase('frame', host(y), host(x), xEdges, yEdges, lat_c=host(fd.lat_c), elev=host(fd.elev), mask=host(fd.center_mask),
                       img=img.reshape(fd.height * fd.width, -1))


def oracle_accumulators(frames, projection, xEdges, yEdges):
    """(device accumulators as host planes (C + 2, nx, ny), the oracle's, the cases)"""
    from auromat_amd import resample as R
    acc, planes = R.project_and_bin(frames, projection, xEdges, yEdges)
    nx, ny = len(xEdges) - 1, len(yEdges) - 1
    got = acc.cpu().numpy().reshape(-1, nx, ny)
    cases = [plane_case(fd, x, y, xEdges, yEdges) for fd, (x, y) in zip(frames, planes)]
    want = sum(PO.accumulate(c)[0] for c in cases)
    return got, want, cases


def check_result(result, frames, frame_name, minCoverage=0.5):
    """A ProjectedMapping against the oracle on its own projection and edges"""
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import GenericMapping, ProjectedMapping
    assert isinstance(result, ProjectedMapping) and isinstance(result, GenericMapping)
    P, xE, yE = result.projection, result.xEdges, result.yEdges
    nx, ny = len(xE) - 1, len(yE) - 1
    got, want_acc, cases = oracle_accumulators(frames, P, xE, yE)
    assert np.array_equal(got, want_acc), 'accumulators differ in %d entries' % (got != want_acc).sum()
    dtype = cases[0].img.dtype
    want = AO.finalize(want_acc, dtype, minCoverage)
    assert not want['over']
    res = R.resample_frames_projected(frames, P, xE, yE, minCoverage)
    assert res['mask'].dtype == bool and res['img'].dtype == dtype
    for key in OUT_KEYS:
        assert AO.same_bits(res[key].astype(np.uint8) if key == 'mask' else res[key], want[key]), key
    # the mapping: shapes, types, attributes, masks
    valid = want['mask'] == 0
    assert result.img.shape == (ny, nx, want['img'].shape[2]) and result.img.dtype == dtype
    assert np.array_equal(ma.getmaskarray(result.img), np.repeat(~valid[:, :, None], result.img.shape[2], 2))
    assert np.array_equal(ma.getdata(result.img)[valid], want['img'][valid])
    assert np.array_equal(ma.getmaskarray(result.elevation), ~valid)
    assert AO.same_bits(ma.getdata(result.elevation)[valid], want['area'][:, :, -1][valid])
    assert AO.same_bits(result.coverage, want['coverage']) and result.coverage.shape == (ny, nx)
    assert result.planeFrame == frame_name
    assert result.lats.shape == result.lons.shape == (ny + 1, nx + 1) and result.latsCenter.shape == (ny, nx)
    assert valid.sum() > 500
    result.checkGuarantees()
    return want, want_acc, cases


def check_coordinates(lat, lon, P, px, py, step=7):
    """coordinate arrays of a result against the mpmath inverse of the plane points, every `step`-th point: the bound of
    tests/test_gpu_projection.py"""
    px, py = px.ravel()[::step], py.ravel()[::step]
    case = dict(name='grid', projection=P, family='grid')
    ref = O.points(K._MP, O.inverse, P, px, py)
    f64 = O.points(O.Float64(), O.inverse, P, px, py)
    got = (np.asarray(lat, dtype=np.float64).ravel()[::step], np.asarray(lon, dtype=np.float64).ravel()[::step])
    for (dist, eps_scale), (e_ref, _), name in zip(K.distances_and_scales(case, 'inverse', got, ref),
                                                   K.distances_and_scales(case, 'inverse', f64, ref), ('lat', 'lon')):
        bound = K.FACTOR * np.maximum(e_ref.astype(np.float64), eps_scale)
        worst = float(np.max(dist.astype(np.float64) / bound))
        print('%s: worst %.2f of the bound (%.2f eps scale)' % (name, worst, float(np.max(dist.astype(np.float64) / eps_scale))))
        assert worst <= 1.0, (name, worst)


def oracle_projection(result):
    p = result.projection.params
    if p.kind == 2:
        return O.paeqd(p.mode > 0, p.lon0, p.a)
    return O.stere(p.lat0, p.lon0, 6378.137, 6356.752314245179)


def corner_points(result):
    gx, gy = np.meshgrid(result.xEdges, result.yEdges[::-1])
    return gx, gy


def holes_of_centre_binning(fd, projection, xE, yE):
    """(ny, nx) bool, rows north first: cells that hold no pixel centre while their four edge neighbours do"""
    keep = (fd.center_mask.cpu().numpy() == 0) & np.isfinite(fd.lat_c.cpu().numpy())
    x, y = projection.forward(fd.lat_c.cpu().numpy()[keep], fd.lon_c.cpu().numpy()[keep])
    ix, iy = np.searchsorted(xE, x, side='right') - 1, np.searchsorted(yE, y, side='right') - 1
    nx, ny = len(xE) - 1, len(yE) - 1
    inside = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    count = np.zeros((nx, ny), dtype=np.int64)
    np.add.at(count, (ix[inside], iy[inside]), 1)
    f = count > 0
    hole = np.zeros((nx, ny), dtype=bool)
    hole[1:-1, 1:-1] = ~f[1:-1, 1:-1] & f[:-2, 1:-1] & f[2:, 1:-1] & f[1:-1, :-2] & f[1:-1, 2:]
    return np.flipud(hole.T), int(keep.sum())


def test_stereographic_closes_the_holes_of_centre_binning():
    """The 030 frame on the 747 x 728 km map around the mean position of its 5951 admitted pixels, 10 km per pixel: 75 x 73 cells;
    the 103 holes of centre binning have coverage >= 0.5 and are valid."""
    from auromat_amd import resample as R
    m = golden_mapping('georef_small_iss030_fast.npz')
    fd = m.frame()
    keep = (fd.center_mask.cpu().numpy() == 0)
    lat0, lon0 = float(fd.lat_c.cpu().numpy()[keep].mean()), float(fd.lon_c.cpu().numpy()[keep].mean())
    result = R.resampleStereographic(m, lat0=lat0, lon0=lon0, width=747.0, height=728.0, kmPerPx=10)
    assert result.img.shape == (73, 75, 3)
    assert np.array_equal(result.xEdges, np.linspace(-375.0, 375.0, 76)) and np.array_equal(result.yEdges, np.linspace(-365.0, 365.0, 74))
    want, want_acc, cases = check_result(result, [fd], 'geo')
    # the domain rule removes nothing: every finite corner is far inside the 90-degree circle
    assert np.array_equal(np.isnan(cases[0].lon), np.isnan(fd.lat.cpu().numpy()))
    holes, n = holes_of_centre_binning(fd, result.projection, result.xEdges, result.yEdges)
    assert n == 5951 and holes.sum() == 103
    assert np.all(result.coverage[holes] >= 0.5) and not ma.getmaskarray(result.img)[:, :, 0][holes].any()
    gx, gy = corner_points(result)
    check_coordinates(result.lats.data, result.lons.data, oracle_projection(result), gx, gy)
    # row 0 is the northern row, and the centre of the map is the centre of the projection
    assert result.latsCenter.data[0, 37] > result.latsCenter.data[-1, 37]
    assert abs(result.lats.data[36:38, 37:39].mean() - lat0) < 0.1


def test_stereographic_default_geometry_and_resolution():
    """Nothing given: centre and size from the bounding box by the reference's rule, 100 arcsec per pixel"""
    from auromat_amd import resample as R
    m = golden_mapping('georef_small_iss030_fast.npz', dtype=np.uint16)
    result = R.resampleStereographic(m)
    lat0, lon0, width, height = R.stereographic_geometry([m.boundingBox])
    km = R.projected_km_per_px(None, 100)
    p = result.projection.params
    assert (p.lat0, p.lon0, p.kind, p.mode) == (lat0, lon0, 1, 0)
    assert np.array_equal(result.xEdges, R.projected_edges(width, km)) and np.array_equal(result.yEdges, R.projected_edges(height, km))
    assert result.img.shape[:2] == (int(np.ceil(height / km)), int(np.ceil(width / km))) and result.img.dtype == np.uint16
    check_result(result, [m.frame()], 'geo')
    bigger = R.resampleStereographic(m, sizeFactor=1.5, kmPerPx=20, minCoverage=0.0)
    assert len(bigger.xEdges) - 1 == int(np.ceil(width * 1.5 / 20))
    check_result(bigger, [m.frame()], 'geo', minCoverage=0.0)


def test_two_halves_give_the_accumulators_of_the_whole():
    from auromat_amd import resample as R
    from auromat_amd.coordinates.projection import Stereographic
    from auromat_amd.mapping.mapping import MappingCollection
    name = 'georef_small_iss030_fast.npz'
    z = load_golden(name)
    with np.errstate(invalid='ignore'):
        rows = np.nonzero((np.isfinite(z['lat_c']) & (z['elev'] >= 10)).any(axis=1))[0]
    cut = int(rows[len(rows) // 2])             # the middle one of the rows that hold admitted pixels
    assert 0 < cut < 96
    whole, top, bottom = golden_mapping(name), golden_mapping(name, rows=(0, cut)), golden_mapping(name, rows=(cut, 96))
    P = Stereographic(51.0, -97.0)
    xE, yE = R.projected_edges(800.0, 10.0), R.projected_edges(760.0, 10.0)
    one, _ = R.project_and_bin([whole.frame()], P, xE, yE)
    two, _ = R.project_and_bin([top.frame(), bottom.frame()], P, xE, yE)
    assert np.array_equal(one.cpu().numpy(), two.cpu().numpy()) and int(one[0].sum()) > 0
    kw = dict(lat0=51.0, lon0=-97.0, width=800.0, height=760.0, kmPerPx=10)
    a = R.resampleStereographic(whole, **kw)
    for halves in ([top, bottom], MappingCollection([bottom, top], 'halves', mayOverlap=False), [MappingCollection([top], 't'), bottom]):
        b = R.resampleStereographic(halves, **kw)
        assert np.array_equal(ma.getmaskarray(a.img), ma.getmaskarray(b.img)) and np.array_equal(a.img.filled(0), b.img.filled(0))
        assert AO.same_bits(a.coverage, b.coverage) and AO.same_bits(a.elevation.filled(np.nan), b.elevation.filled(np.nan))


def test_stereographic_mlat_mlt():
    from auromat_amd import resample as R
    from auromat_amd.coordinates.transform import smToLatLon
    from auromat_amd.mapping.mapping import convertMappingToSM
    m = golden_mapping('georef_small_iss029_fast.npz')
    sm = convertMappingToSM(m)
    result = R.resampleStereographicMLatMLT(m, kmPerPx=10)
    lat0, lon0, width, height = R.stereographic_geometry([sm.boundingBox])
    p = result.projection.params
    assert (p.lat0, p.lon0, p.kind) == (lat0, lon0, 1) and abs(p.e - 0.0818191908426) < 1e-12          # WGS84, as the reference
    assert np.array_equal(result.xEdges, R.projected_edges(width, 10.0)) and np.array_equal(result.yEdges, R.projected_edges(height, 10.0))
    check_result(result, [sm.frame()], 'sm')
    # the coordinate arrays: the inverse projection (magnetic), then the arithmetic of convertSMMappingToGeo
    gx, gy = corner_points(result)
    mla, mlo = result.projection.inverse(gx, gy)
    check_coordinates(mla, mlo, oracle_projection(result), gx, gy)
    la, lo = smToLatLon(mla, mlo, m.photoTime)
    assert AO.same_bits(np.asarray(result.lats.data), la) and AO.same_bits(np.asarray(result.lons.data), lo)


def test_mlat_mlt_polar():
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import convertMappingToSM
    m = golden_mapping('georef_small_iss029_fast.npz', nch=1)
    sm = convertMappingToSM(m)
    box = sm.boundingBox
    result = R.resampleMLatMLTPolar(m, kmPerPx=25)
    north, bounding, half = R.polar_geometry(box.latSouth, box.latNorth, 6370.997)
    p = result.projection.params
    assert (p.kind, p.mode, p.lon0, p.a) == (2, 1 if north else -1, 180.0, 6370.997)
    edges = R.projected_edges(2 * half, 25.0)
    assert np.array_equal(result.xEdges, edges) and np.array_equal(result.yEdges, edges) and result.img.shape[2] == 1
    check_result(result, [sm.frame()], 'sm')
    gx, gy = corner_points(result)
    mla, mlo = result.projection.inverse(gx, gy)
    check_coordinates(mla, mlo, oracle_projection(result), gx, gy, step=101)
    # magnetic midnight (SM longitude 180) points down on a north polar map: the bottom middle corner
    mid = len(edges) // 2
    assert abs(abs(mlo[-1, mid]) - 180) < 1.0 if north else abs(mlo[-1, mid]) < 1.0


def test_export_and_image(tmp_path):
    """The netCDF exporter takes the result as any GenericMapping, and saveMapImage writes its image"""
    from PIL import Image
    from auromat_amd import resample as R
    from auromat_amd.draw import saveMapImage
    from auromat_amd.export import netcdf
    m = golden_mapping('georef_small_iss030_fast.npz')
    result = R.resampleStereographic(m, kmPerPx=20)
    path = str(tmp_path / 'map.png')
    saveMapImage(result, path)
    back = np.asarray(Image.open(path))
    assert back.shape == result.img.shape[:2] + (4,)
    assert np.array_equal(back[:, :, 3] == 0, ma.getmaskarray(result.img)[:, :, 0])
    assert np.array_equal(back[:, :, :3][back[:, :, 3] > 0], result.img.data[~ma.getmaskarray(result.img)[:, :, 0]])
    out = str(tmp_path / 'map.nc')
    netcdf.write(out, result)
    import os
    assert os.path.getsize(out) > 1000


def test_arguments():
    from auromat_amd import resample as R
    m = golden_mapping('georef_small_iss030_fast.npz')
    with pytest.raises(ValueError):
        R.resampleStereographic(m, width=0.0, height=100.0)             # an empty grid
    with pytest.raises(ValueError):
        R.resampleStereographic(m, minCoverage=2)
    # the overflow word: one cell of 100 km inside the frame's footprint, covered whole by each of 300 members
    fd = m.frame()
    keep = fd.center_mask.cpu().numpy() == 0
    lat0, lon0 = float(fd.lat_c.cpu().numpy()[keep].mean()), float(fd.lon_c.cpu().numpy()[keep].mean())
    kw = dict(lat0=lat0, lon0=lon0, width=100.0, height=100.0, kmPerPx=100)
    # (a member's weights in the cell add up to 2^32 give or take half a unit per pixel: 250 stay below 2^40, 262 do not)
    one = R.resampleStereographic([m] * 250, **kw)
    assert one.coverage.shape == (1, 1) and abs(one.coverage[0, 0] - 250.0) < 1e-3
    with pytest.raises(ValueError, match='256 times'):
        R.resampleStereographic([m] * 262, **kw)
