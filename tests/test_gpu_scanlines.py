"""
resampleScanLines / resampleScanLinesMLatMLT (auromat_amd.resample) on the ten real consecutive headers of
tests/golden/resources/seq at full size (the mapping sequence of tests/test_real_frame.py, masked by elevation 10), and on a
constructed sequence across the date line.

The oracle is put together here from pieces that other tests pin: per frame ``resample_frame`` with the sequence's longitude
frame (host arrays), the rule of ``maskedByPolygon`` restated in NumPy with matplotlib's ``contains_points`` on the frame's 2-D
corner arrays, and the NumPy compose of tests/_scanline_oracle.py.  Everything is compared bit for bit.

matplotlib tests every corner against every one of a strip's ~10^4 vertices; to keep that to seconds only the corners inside
the polygon's box are handed to it (a corner outside the box is outside the polygon), and the oracle's frames and strips are
computed once per sequence and width factor and shared by the tests.
"""
import datetime
import functools

import numpy as np
import numpy.ma as ma
import pytest

import _scanline_oracle as O
from test_real_frame import real_sequence

pytestmark = pytest.mark.gpu

ARCSEC = 100


@functools.lru_cache(maxsize=None)
def iss_mappings():
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    return tuple(ArraySpacecraftMapping(hdr, 110, img, cam, t, 'f%d' % k, fastCenterCalculation=True).maskedByElevation(10)
                 for k, (hdr, cam, t, img) in enumerate(real_sequence()))


@functools.lru_cache(maxsize=None)
def iss_mappings_sm():
    from auromat_amd.mapping.mapping import convertMappingToSM
    return tuple(convertMappingToSM(m) for m in iss_mappings())


def polygon_rule(lat, lon, cell_mask, polygon):
    """BaseMapping.maskedByPolygon on the arrays of a resampled mapping, in NumPy: (ny, nx) bool, the cells it keeps"""
    import matplotlib.path
    import auromat_amd.resample as R
    from auromat_amd.mapping.mapping import wrap_at_180
    free = ~np.asarray(cell_mask, dtype=bool)
    corner_ok = np.zeros(lat.shape, dtype=bool)                    # a corner is unmasked next to an unmasked cell
    for dy in (0, 1):
        for dx in (0, 1):
            corner_ok[dy:dy + free.shape[0], dx:dx + free.shape[1]] |= free
    own = lon[corner_ok]
    polygon = np.array(polygon, dtype=np.float64)
    if own.max() - own.min() > 180 or R.lons_contain_discontinuity(polygon[:, 1]):
        polygon[:, 1] = wrap_at_180(polygon[:, 1] + 180)
        lon = np.remainder(lon + 360.0, 360.0) - 180.0
    inside = np.zeros(lat.shape, dtype=bool)
    box = (lat >= polygon[:, 0].min()) & (lat <= polygon[:, 0].max()) & (lon >= polygon[:, 1].min()) & (lon <= polygon[:, 1].max())
    inside[box] = matplotlib.path.Path(polygon).contains_points(np.column_stack((lat[box], lon[box])))
    return O.four_corner_rule(inside, cell_mask)


def oracle(mappings, pxPerDeg=None, arcsecPerPx=100, factor=1):
    import auromat_amd.resample as R
    from auromat_amd.coordinates import geodesic
    from auromat_amd.mapping.mapping import BoundingBox
    props = [m.properties for m in mappings]
    ppd = R._px_per_deg(pxPerDeg) if pxPerDeg is not None else R.plateCarreeResolution(props[0].boundingBox, arcsecPerPx)
    shifted = R.scanline_longitude_frame(props[0].centroid)
    frames = [R.resample_frame(m.frame(), m.altitude, p.boundingBox, ppd, containsDiscontinuity=shifted) for m, p in zip(mappings, props)]
    f0 = frames[0]
    r, c = np.argwhere(~f0['mask'])[0]                              # the first unmasked cell, row-major
    diagonal = geodesic.distance(geodesic.Location(f0['lat'][r, c], f0['lon'][r, c]),
                                 geodesic.Location(f0['lat'][r + 1, c + 1], f0['lon'][r + 1, c + 1]))
    rule = R.scanline_strips(props, diagonal, factor)
    strips, kept_all, boxes, extents = [], [], [], []
    for f, polygon in zip(frames, rule['polygons']):
        kept = polygon_rule(f['lat'], f['lon'], f['mask'], polygon)
        r0, c0 = R.scanline_global_origin(f['grid'], ppd)
        strips.append(O.pack(kept, (0, 0) + kept.shape, f['mean'], f['img'], r0, c0))
        st = O.stats_of(kept)
        kept_all.append(kept)
        if st[0]:
            extents.append((r0 + st[1], r0 + st[2], c0 + st[3], c0 + st[4]))
            boxes.append(BoundingBox(f['lat'][st[2] + 1, 0], f['lon'][0, st[3]], f['lat'][st[1], 0], f['lon'][0, st[4] + 1]))
    e = np.array(extents)
    rowMin, rowMax, colMin, colMax = e[:, 0].min(), e[:, 1].max(), e[:, 2].min(), e[:, 3].max()
    union = R.scanline_union_grid(ppd, rowMin, rowMax, colMin, colMax)
    nch = f0['img'].shape[2]
    planes, img, mask, index, outside = O.compose(strips, range(len(strips)), rowMin, colMin, union.ny, union.nx, nch + 1, nch,
                                                  f0['img'].dtype)
    assert not outside
    claims = np.zeros((union.ny, union.nx), dtype=int)
    for s in strips:
        np.add.at(claims, (s['row'] - rowMin, s['col'] - colMin), 1)
    coords = R.grid_coordinates(dict(grid=union, contains_pole=False, contains_discontinuity=shifted, altitude=mappings[0].altitude))
    return dict(rule=rule, frames=frames, kept=kept_all, strips=strips, boxes=boxes, planes=planes, img=img, mask=mask.astype(bool),
                index=index, claims=claims, coords=coords, base=(int(rowMin), int(colMin)), ppd=ppd, shifted=shifted, props=props,
                maxHeight=max(geodesic.distance(b.topLeft, b.bottomRight) for b in boxes))


@functools.lru_cache(maxsize=None)
def iss_oracle(factor, sm=False):
    return oracle(iss_mappings_sm() if sm else iss_mappings(), arcsecPerPx=ARCSEC, factor=factor)


def check_against(scan, want, n):
    from auromat_amd.mapping.mapping import ScanLineMapping
    assert isinstance(scan, ScanLineMapping)
    assert all(k.sum() > 0 for k in want['kept']) and len(want['kept']) == n           # every strip is non-empty
    mask = want['mask']
    assert np.array_equal(ma.getmaskarray(scan.img), np.repeat(mask[:, :, None], scan.img.shape[2], 2))
    assert scan.img.dtype == want['img'].dtype and np.array_equal(scan.img.data, want['img'])
    assert np.array_equal(ma.getmaskarray(scan.elevation), mask)
    assert np.array_equal(scan.elevation.data, want['planes'][..., -1], equal_nan=True)
    assert scan.frameIndex.dtype == np.int32 and np.array_equal(scan.frameIndex.data, want['index'])
    assert np.array_equal(ma.getmaskarray(scan.frameIndex), mask)
    present = set(np.unique(scan.frameIndex.compressed()))
    assert present <= set(range(n)) and n - 1 in present and len(present) > 1
    for name, key in (('lats', 'lat'), ('lons', 'lon'), ('latsCenter', 'lat_c'), ('lonsCenter', 'lon_c')):
        assert np.array_equal(ma.getdata(getattr(scan, name)), want['coords'][key]), name
    assert scan.lineBoundingBoxes == want['boxes']
    assert scan.maxHeight == want['maxHeight'] and scan.width == want['rule']['width'] and scan.height == want['rule']['height']
    assert scan.azimuths == want['rule']['azimuths'] and scan.pxPerDeg == tuple(want['ppd'])
    assert all(np.array_equal(a, b) for a, b in zip(scan.polygons, want['rule']['polygons']))
    assert scan.photoTimes == [p.photoTime for p in want['props']] and scan.centroids == [p.centroid for p in want['props']]
    assert scan.identifiers == [p.identifier for p in want['props']]
    assert scan.identifier == '%s..%s' % (want['props'][0].identifier, want['props'][-1].identifier)
    assert scan.photoTime == want['props'][0].photoTime and scan.isPlateCarree


@pytest.mark.parametrize('factor', [1, 3])
def test_scan_lines_of_the_real_sequence(factor, tmp_path):
    import auromat_amd.resample as R
    from auromat_amd.draw import saveMapImage
    from auromat_amd.mapping.mapping import ProjectedMapping
    mappings = iss_mappings()
    want = iss_oracle(factor)
    pulled = []

    def once():
        for m in mappings:
            pulled.append(m.identifier)
            yield m
    scan = R.resampleScanLines(once(), arcsecPerPx=ARCSEC, lineWidthFactor=factor)
    assert pulled == [m.identifier for m in mappings]                                  # a generator, consumed once
    check_against(scan, want, 10)
    if factor == 3:
        # (factor 3 is enough for this sequence: cells claimed by two or more strips exist and go to the later one)
        shared = want['claims'] >= 2
        assert shared.sum() > 50
        later = np.full(shared.shape, -1)
        for k, s in enumerate(want['strips']):                      # (ascending: the last assignment is the largest index)
            later[s['row'] - want['base'][0], s['col'] - want['base'][1]] = k
        assert np.array_equal(scan.frameIndex.data[shared], later[shared])
        assert want['rule']['width'] == 3 * iss_oracle(1)['rule']['width']
        path = str(tmp_path / 'scan.png')
        saveMapImage(scan, path)
        from PIL import Image
        assert Image.open(path).size == (scan.img.shape[1], scan.img.shape[0])
        assert isinstance(R.resampleStereographic(scan), ProjectedMapping)


def _check_public_composition(mappings, want):
    """Where a frame's own containsDiscontinuity equals the sequence's longitude frame, its strip is
    ``resample(m, pxPerDeg=p).maskedByPolygon(polygon)`` cell for cell.  Returns the number of frames compared."""
    import auromat_amd.resample as R
    checked = 0
    for k, m in enumerate(mappings):
        if bool(m.containsDiscontinuity) != want['shifted']:
            continue
        strip = R.resample(m, pxPerDeg=want['ppd']).maskedByPolygon(want['rule']['polygons'][k])
        kept = ~ma.getmaskarray(strip.img)[..., 0]
        assert np.array_equal(kept, want['kept'][k]), k
        assert np.array_equal(strip.img.data[kept], want['frames'][k]['img'][kept]), k
        assert np.array_equal(strip.lats.data, want['frames'][k]['lat']) and np.array_equal(strip.lons.data, want['frames'][k]['lon'])
        checked += 1
    return checked


def test_strips_equal_the_public_composition():
    """The real sequence lies around longitude 155 without touching the date line: it is resampled in the shifted frame, which
    no frame of it would choose for itself, so it has no frame to compare (asserted, so that a change of that shows).  The
    constructed sequences (all frames across the date line; all frames around longitude 10) are compared frame for frame."""
    mappings, want = iss_mappings(), iss_oracle(1)
    assert want['shifted'] and not any(m.containsDiscontinuity for m in mappings)
    assert _check_public_composition(mappings, want) == 0
    across = [patch_mapping(k, 179.2 + 0.5 * k) for k in range(3)]
    assert _check_public_composition(across, oracle(across, pxPerDeg=5)) == 3
    plain = [patch_mapping(k, 10.0 + 0.5 * k) for k in range(3)]
    assert _check_public_composition(plain, oracle(plain, pxPerDeg=5)) == 3


def test_scan_lines_mlat_mlt_of_the_real_sequence():
    import auromat_amd.resample as R
    scan = R.resampleScanLinesMLatMLT(iss_mappings(), arcsecPerPx=ARCSEC)
    check_against(scan, iss_oracle(1, sm=True), 10)


def test_short_sequences_are_refused():
    import auromat_amd.resample as R
    for n in (0, 1):
        with pytest.raises(ValueError, match='mapping sequence too short, need at least 2 mappings'):
            R.resampleScanLines(iter(iss_mappings()[:n]), arcsecPerPx=ARCSEC)


# ---- a constructed sequence across the date line --------------------------------------------------------------------------------

def patch_mapping(k, lon_centre):
    """64 x 64 pixels on a regular patch of 6 x 6 degrees around (53, lon_centre), seen from a camera that moves east"""
    from auromat_amd.mapping.mapping import GenericMapping, wrap_at_180
    n = 64
    lat = np.repeat((56.0 - 6.0 * np.arange(n + 1) / n)[:, None], n + 1, 1)
    lon = wrap_at_180(np.repeat((lon_centre - 3.0 + 6.0 * np.arange(n + 1) / n)[None, :], n + 1, 0))
    lat_c = np.repeat((56.0 - 6.0 * (np.arange(n) + 0.5) / n)[:, None], n, 1)
    lon_c = wrap_at_180(np.repeat((lon_centre - 3.0 + 6.0 * (np.arange(n) + 0.5) / n)[None, :], n, 0))
    rs = np.random.RandomState(k)
    elev = 30 + 40 * rs.random_sample((n, n))
    img = rs.randint(0, 256, size=(n, n, 3)).astype(np.uint8)
    a = np.deg2rad(lon_centre + 0.3 * k)
    cam = 6778.0 * np.array([np.cos(np.deg2rad(48)) * np.cos(a), np.cos(np.deg2rad(48)) * np.sin(a), np.sin(np.deg2rad(48))])
    t = datetime.datetime(2012, 1, 25, 9, 0, 0) + datetime.timedelta(seconds=3 * k)
    return GenericMapping(lat, lon, lat_c, lon_c, elev, 110, img, cam, t, 'patch%d' % k)


def test_sequence_across_the_date_line_and_the_seam():
    import auromat_amd.resample as R
    mappings = [patch_mapping(k, 179.2 + 0.5 * k) for k in range(3)]
    assert all(m.containsDiscontinuity for m in mappings)
    want = oracle(mappings, pxPerDeg=5)
    assert want['shifted']
    scan = R.resampleScanLines(mappings, pxPerDeg=5)
    check_against(scan, want, 3)
    lons = ma.getdata(scan.lons)
    assert lons.min() >= -180 and lons.max() <= 180 and (lons > 170).any() and (lons < -170).any()       # wrapped back
    assert (want['claims'] >= 2).any()
    with pytest.raises(ValueError, match=r'frame 3 \(\'patch3\'\).*spans the seam of its longitude frame'):
        R.resampleScanLines(mappings + [patch_mapping(3, 0.5)], pxPerDeg=5)
    # the same patches around longitude 10: the unshifted frame; one across the date line does not fit it
    plain = [patch_mapping(k, 10.0 + 0.5 * k) for k in range(3)]
    want = oracle(plain, pxPerDeg=5)
    assert not want['shifted']
    check_against(R.resampleScanLines(plain, pxPerDeg=5), want, 3)
    with pytest.raises(ValueError, match='frame 3 .*spans the seam'):
        R.resampleScanLines(plain + [mappings[2]], pxPerDeg=5)
