"""
resampleGather / resampleGatherMLatMLT and graticulePixels on the GPU.

Constructed cameras (tests/_inverse_cases.py): every output is the NumPy statement of tests/_inverse_oracle.gather_statement —
coordinates from the point entry amt_world_to_pixel on the same cell centres, sampling by the remap statement of
tests/_lens_oracle.py (its comparison rule: equal, except that a sample whose exact value lies within 1e-6 counts of a rounding
boundary may differ by one count), the four masking rules, a lazily remembered maskedByElevation(10) — for uint8, uint16 and
float32 images with 1, 3 and 4 channels and the three interpolations.

The reference's frame ISS030-E-102170_dc (4256 x 2832): the grid is that of resample(); at 250 px / deg binning the pixel centres
leaves holes inside the footprint and gathering leaves none; the parallels and meridians of graticulePixels run where the
mean-resampled look-up table of the reference's drawParallelsAndMeridians puts them, to within the size of a table cell.
Measured on the MI355X: grid 1561 x 2554, 2 613 127 cells seen at 10 deg of elevation or more, all of them and no others unmasked;
binning leaves 503 287 empty cells between filled cells of a row, gathering none.  Of the 654 table cells on the drawn lines the
farthest lies 77.8 px from the exact line, 0.424 of its own diagonal in the pixel plane (the table is the approximation).
"""
import os

import numpy as np
import pytest

import _inverse_cases as IC
import _inverse_oracle as O
import _lens_oracle as L

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
JPG = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.jpg')
WCS = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.wcs')
PX_PER_DEG = 200            # the constructed frames: 0.05 deg / px from 400 km is about 300 px per degree on the ground


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


_header = IC.header_of


def _image(cam, dtype, channels, seed=3):
    rng = np.random.RandomState(seed)
    shape = (cam['height'], cam['width'], channels)
    if np.dtype(dtype) == np.float32:
        return (rng.uniform(-1.0, 1.0, shape) * 1000.0).astype(np.float32)
    return rng.randint(0, int(L.SAMPLE_MAX[np.dtype(dtype)]) + 1, size=shape).astype(dtype)


def _mapping(cam, image=None, lazy_elevation=None):
    from auromat_amd.coordinates import wcs
    from auromat_amd.mapping.astrometry import DirectionArrayMapping
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    h = _header(cam)
    img = _image(cam, np.uint8, 3) if image is None else image
    if O.is_plain_tan(cam):
        m = ArraySpacecraftMapping(h, cam['altitude'], img, cam['cam'], cam['time'], cam['name'], fastCenterCalculation=True)
    else:
        dirs = wcs.zenithal_directions_device(h, cam['width'], cam['height'], corner=True)
        m = DirectionArrayMapping(dirs, cam['altitude'], img, cam['cam'], cam['time'], cam['name'], cameraHeader=h)
    return m if lazy_elevation is None else m.maskedByElevation(lazy_elevation)


def _statement(plan, image, interpolation, magnetic):
    """the NumPy statement on the plan's cell centres, the coordinates from the point entry"""
    from auromat_amd._native import to_host
    from auromat_amd.coordinates.inverse import world_to_pixel
    from auromat_amd.resample import grid_coordinates
    coords = grid_coordinates(plan)
    frame = O.SM if magnetic else O.GEODETIC
    xy, elev, flags = world_to_pixel(plan['params'], plan['zenithal'], frame, np.ascontiguousarray(coords['lat_c']),
                                     np.ascontiguousarray(coords['lon_c']))
    cm = None if plan['center_mask'] is None else to_host(plan['center_mask']).astype(bool).reshape(image.shape[:2])
    s = O.gather_statement(None, frame, None, None, image, interpolation, min_elevation=plan['min_elevation'], center_mask=cm,
                           xy=xy, elev=elev, flags=flags)
    s['flags'] = flags
    return s, coords


def _check(res, s, image, interpolation, what):
    assert np.array_equal(res['mask'], s['mask']), what
    assert same_bits(res['elevation'], s['elevation']) and np.array_equal(res['flags'], s['flags']), what
    assert res['img'].dtype == image.dtype and res['img'].shape == s['img'].shape, what
    if interpolation == 'nearest':
        assert np.array_equal(res['img'], s['img']), what
    else:
        assert L.compare(res['img'], s['values'], image.dtype, s['magnitude']) == 0, what
    assert 0 < s['mask'].sum() < s['mask'].size, what


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize('channels', [1, 3, 4])
def test_gather_frame_is_the_statement(dtype, channels):
    from auromat_amd.resample import gather_frame, gather_plan
    cam = IC.by_name('wide-hyperbola-70')        # 130 x 100 at 0.45 deg / px: elevations from the limb's 0 deg to 50 deg and more
    image = _image(cam, dtype, channels)
    for magnetic in (False, True):
        plan = gather_plan(_mapping(cam, lazy_elevation=10), pxPerDeg=10, magnetic=magnetic)
        assert plan['min_elevation'] == 10.0 and plan['center_mask'] is None and plan['grid'].ny > 8 and plan['grid'].nx > 8
        for interpolation in ('nearest', 'linear', 'lanczos4'):
            res = gather_frame(plan, image, interpolation, magnetic)
            s, _ = _statement(plan, image, interpolation, magnetic)
            _check(res, s, image, interpolation, (dtype, channels, magnetic, interpolation))
            with np.errstate(invalid='ignore'):
                assert (s['mask'] & (s['flags'] == 0) & (s['elevation'] < 10.0)).any()         # the remembered threshold bites


@pytest.mark.parametrize('name', ['cd-flipped', 'dateline', 'pole', 'inside', 'sip-3', 'zen-ZEA'])
def test_resample_gather_on_constructed_cameras(name):
    import numpy.ma as ma
    from auromat_amd.resample import gather_plan, resample, resampleGather, resampleGatherMLatMLT, resampleMLatMLT
    cam = IC.by_name(name)
    image = _image(cam, np.uint16 if name == 'dateline' else np.uint8, 3)
    # (0.3 deg / px from 50 km below the shell; 0.4 deg / px with the limb in view: a footprint of 20 x 30 deg)
    ppd = 20 if name == 'inside' else 10 if name in ('sip-3', 'zen-ZEA') else PX_PER_DEG
    for magnetic, gather, binned in ((False, resampleGather, resample), (True, resampleGatherMLatMLT, resampleMLatMLT)):
        if magnetic and name == 'pole':
            continue
        m = _mapping(cam, image)
        if name in ('cd-flipped', 'sip-3'):
            m.frame()                                   # arrays exist: the centre mask takes part
        g = gather(m, pxPerDeg=ppd, interpolation='linear')
        plan = gather_plan(m, pxPerDeg=ppd, magnetic=magnetic)
        assert (plan['center_mask'] is not None) == (name in ('cd-flipped', 'sip-3', 'zen-ZEA', 'pole')), name
        assert plan['contains_pole'] == (name == 'pole')
        if not magnetic:
            assert plan['contains_discontinuity'] == (name == 'dateline')
        s, coords = _statement(plan, image, 'linear', magnetic)
        assert np.array_equal(ma.getmaskarray(g.img)[..., 0], s['mask']), name
        keep = ~s['mask']
        assert L.compare(np.asarray(g.img.data)[keep], s['values'][keep], image.dtype, s['magnitude'][keep]) == 0, name
        assert np.array_equal(ma.getmaskarray(g.elevation), s['mask'] | np.isnan(s['elevation'])), name
        assert same_bits(np.asarray(g.elevation.data)[keep], s['elevation'][keep]), name
        assert 0 < s['mask'].sum() < s['mask'].size, name
        # the grid is the one resample() chooses
        b = binned(_mapping(cam, image), pxPerDeg=ppd)
        for a in ('lats', 'lons', 'latsCenter', 'lonsCenter'):
            assert same_bits(np.asarray(ma.getdata(getattr(g, a))), np.asarray(ma.getdata(getattr(b, a)))), (name, a)


def test_real_frame_grid_holes_and_graticule():
    import numpy.ma as ma
    from auromat_amd.coordinates.inverse import HIDDEN, NO_PIXEL, OUTSIDE
    from auromat_amd.draw import graticulePixels
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import _resample, resample, resampleGather
    ppd = 250                 # cells of 0.44 km: about the footprint of a pixel across the line of sight at 10 deg of elevation
    lazy = getMapping(JPG, WCS, fastCenterCalculation=True).maskedByElevation(10)
    g = resampleGather(lazy, pxPerDeg=ppd, interpolation='nearest')
    assert lazy._frame is None                                              # no per-pixel array of the frame was computed
    b = resample(getMapping(JPG, WCS, fastCenterCalculation=True).maskedByElevation(10), pxPerDeg=ppd)
    for a in ('lats', 'lons', 'latsCenter', 'lonsCenter'):
        assert same_bits(np.asarray(ma.getdata(getattr(g, a))), np.asarray(ma.getdata(getattr(b, a)))), a
    gm, bm = ma.getmaskarray(g.img)[..., 0], ma.getmaskarray(b.img)[..., 0]
    # every cell whose centre projects into the frame at 10 deg of elevation or more is there, and no other
    x, y, flags = lazy.latLonToPixel(np.asarray(ma.getdata(g.latsCenter)), np.asarray(ma.getdata(g.lonsCenter)), returnFlags=True)
    elev = np.asarray(g.elevation.data)
    with np.errstate(invalid='ignore'):
        seen = (flags == 0) & (elev >= 10.0)
    assert np.array_equal(~gm, seen)
    assert not (flags[seen] & (HIDDEN | NO_PIXEL | OUTSIDE)).any()
    # binning pixel centres at this resolution leaves holes inside the footprint: cells with neighbours on both sides in their
    # row that hold pixels, but none themselves
    filled = ~bm
    left, right = np.maximum.accumulate(filled, axis=1), np.maximum.accumulate(filled[:, ::-1], axis=1)[:, ::-1]
    holes = ~filled & left & right
    print('real frame at %d px / deg: grid %s, %d cells seen, binning leaves %d holes between filled cells of a row, gathering %d'
          % (ppd, gm.shape, int(seen.sum()), int(holes.sum()), int((holes & gm & seen).sum())))
    assert holes.sum() > 100 and not (holes & seen & gm).any()
    assert (~gm & bm).sum() >= holes[seen].sum() > 0
    # ---- graticule: the reference's look-up table (mean-resampled pixel coordinates at 0.2 deg) against the exact lines ----
    m = getMapping(JPG, WCS, fastCenterCalculation=True)
    box = m.boundingBox
    par, mer = graticulePixels(m, every=2, step=0.2, boundingBox=box)
    assert len(par) >= 3 and len(mer) >= 3
    step = 8                                                                # every 8th pixel of the frame feeds the table
    la, lo = m.latsCenter.filled(np.nan)[::step, ::step], m.lonsCenter.filled(np.nan)[::step, ::step]
    rows, cols = np.mgrid[0:la.shape[0], 0:la.shape[1]] * step
    data = np.dstack((cols, rows)).astype(np.float64)
    _, _, lat_grid, lon_grid, table = _resample(la, lo, m.altitude, data, lambda: m.outline, box, (5, 5), box.containsDiscontinuity,
                                                box.containsPole, method='mean')

    def to_polyline(points, line):
        """distance of each point from the polyline (NaN vertices break it)"""
        a, c = line[:-1], line[1:]
        ok = ~(np.isnan(a).any(axis=1) | np.isnan(c).any(axis=1))
        a, c = a[ok], c[ok]
        ab = c - a
        t = np.clip(((points[:, None, :] - a[None]) * ab[None]).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300)[None], 0.0, 1.0)
        return np.sqrt((((a[None] + t[..., None] * ab[None]) - points[:, None, :]) ** 2).sum(-1)).min(axis=1)
    worst, worst_rel, n = 0.0, 0.0, 0
    for lines, values, axis in ((par, lat_grid[:, 0], 0), (mer, lon_grid[0, :], 1)):
        for deg, line in lines.items():
            idx = np.nonzero(np.abs(values - deg) < 1e-9)[0]
            if not len(idx):
                continue
            pts = table[idx[0], :, :] if axis == 0 else table[:, idx[0], :]
            cla = lat_grid[idx[0], :] if axis == 0 else lat_grid[:, idx[0]]
            clo = lon_grid[idx[0], :] if axis == 0 else lon_grid[:, idx[0]]
            have = ~np.isnan(pts).any(axis=1)
            if not have.any():
                continue
            # the size of each table cell in the pixel plane: the images of its four corners
            cx, cy = m.latLonToPixel(np.stack([cla[have] + s for s in (-0.1, -0.1, 0.1, 0.1)]),
                                     np.stack([clo[have] + s for s in (-0.1, 0.1, 0.1, -0.1)]))
            corners = np.stack((cx.filled(np.nan), cy.filled(np.nan)), axis=-1)
            diag = np.maximum(np.hypot(*(corners[0] - corners[2]).T), np.hypot(*(corners[1] - corners[3]).T))
            full = ~np.isnan(diag)
            if not full.any():
                continue
            d = to_polyline(pts[have][full], line)
            worst, worst_rel, n = max(worst, float(d.max())), max(worst_rel, float((d / diag[full]).max())), n + int(full.sum())
    print('graticule: %d table cells on the drawn lines; farthest from the exact line %.2f px, %.3f of its cell\'s diagonal'
          % (n, worst, worst_rel))
    # a table entry is the mean position of the pixels of its 0.2 x 0.2 deg cell, which the line crosses through the middle: it
    # cannot lie farther from the line than half the cell's diagonal in the pixel plane
    assert n > 50 and worst_rel <= 0.5
