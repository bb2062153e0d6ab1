"""
Resampling of mappings onto a regular latitude/longitude grid (plate carree), relative to either
geodetic or MLat/MLT coordinates — mirror of the reference's auromat/resample.py for the
``method='mean'`` binning, plus the median binning the reference names but never built (:func:`resampleMedian`).

Host side: the grid definition (global alignment, pole / discontinuity handling, bin edges —
a few hundred scalars per frame, reference resample.py:159-299).  Device side: bin assignment with
the reference's ``searchsorted(..., 'right')`` edge semantics, accumulation and mean
(``amt_bin_frame`` / ``amt_hist2d_accumulate``), reference resample.py:301-351 and
util/histogram.py:57-282.  Pixel data never leaves the GPU; only the small output grid does.
"""
from __future__ import division, print_function

import copy
import ctypes as C
import math
import threading
from functools import partial

import numpy as np
import numpy.ma as ma

from .coordinates.transform import rotation_matrix
from .coordinates.geodesic import wgs84A, wgs84B
from .mapping.mapping import (BaseMapping, BoundingBox, MappingCollection, convertMappingToSM, convertSMMappingToGeo,
                              wrap_at_180)
from .coordinates.geodesic import angularDistanceOnParallel
from .util.histogram import make_axis
from ._native import AreaMosaicMember, Context, MosaicMember, host9, ptr, to_host


def plateCarreeResolution(boundingBox, arcsecPerPx):
    """
    Approximates the latitude and longitude resolution of a plate carree projection from a
    spherical resolution for the area given by the bounding box (reference resample.py:36-61).
    The approximation is calculated for the bounding box center.  The longitude part needs
    ``geodesic.angularDistance`` between the box's mid-latitude end points, geographiclib's ``a12`` in the
    reference; :func:`auromat_amd.coordinates.geodesic.angularDistanceOnParallel` evaluates the same quantity
    from Karney's integral formulation to ~1e-14 relative, so ``round(pxPerDeg * 360 + 1)`` and with it the
    grid come out the same.

    The arithmetic runs in the library (``amt_plate_carree_resolution``, csrc/amt_grid.h: the same formulation in C++, host
    code, no GPU; microseconds where the NumPy bisection below takes a millisecond), so that the mapping classes, the
    sequence pipeline's box-first plan and the native sequence runner all derive a frame's px/deg from ONE implementation;
    :func:`plateCarreeResolution_py` is the Python restatement the tests pin it to.

    :type boundingBox: auromat_amd.mapping.mapping.BoundingBox
    :param arcsecPerPx: spherical resolution
    :rtype: tuple (latPxPerDeg, lonPxPerDeg)
    """
    from ._native import lib
    lat_ppd, lon_ppd = C.c_double(), C.c_double()
    rc = lib().amt_plate_carree_resolution(float(boundingBox.latSouth), float(boundingBox.lonWest), float(boundingBox.latNorth),
                                           float(boundingBox.lonEast), float(arcsecPerPx), C.byref(lat_ppd), C.byref(lon_ppd))
    if rc != 0 and rc != -5:
        return plateCarreeResolution_py(boundingBox, arcsecPerPx)      # (raises what the Python restatement raises)
    # (-5 = AMT_EDOMAIN: a box that goes all the way round — the reference's function returns (latPxPerDeg, 0) for it and fails
    # later, resample.py:226-227; the callers here check the longitude resolution before they lay out a grid)
    return lat_ppd.value, lon_ppd.value


def plateCarreeResolution_py(boundingBox, arcsecPerPx):
    """:func:`plateCarreeResolution` in Python (the restatement the library's C++ is checked against)."""
    degPerPx = arcsecPerPx / 3600.0
    latPxPerDeg = 1 / degPerPx
    latMiddle = (boundingBox.latNorth + boundingBox.latSouth) / 2
    lonEast = boundingBox.lonEast
    if boundingBox.lonWest > lonEast:
        lons = lonEast + 360 - boundingBox.lonWest
    else:
        lons = lonEast - boundingBox.lonWest
    # the shortest geodesic between the two end points spans min(lons, 360 - lons) of longitude
    lonMiddleDistance = angularDistanceOnParallel(latMiddle, min(lons, 360 - lons))
    px = lonMiddleDistance / degPerPx
    return latPxPerDeg, px / lons


def resampleMLatMLT(mapping, **kw):
    """Resamples a mapping such that MLat/MLT become regular grids (reference resample.py:63-71).

    See :func:`resample` for parameters.
    """
    global last_plan
    fused = getattr(mapping, '_fused_resample', None)
    if fused is not None and kw.get('method', 'mean') == 'mean' and \
            set(kw) <= {'pxPerDeg', 'containsPole', 'method', 'arcsecPerPx'}:
        # a camera mapping whose arrays nobody has asked for yet: the single-pass plan on the (MLat, SM longitude) grid
        # (arcsecPerPx: box-first, px/deg from the frame's own box in (MLat, SM longitude))
        arcsec = kw.get('arcsecPerPx')
        res = fused(None if arcsec else _px_per_deg(kw.get('pxPerDeg', 25)), kw.get('containsPole'), magnetic=True,
                    arcsecPerPx=arcsec)
        if res is not None:
            last_plan = res['plan']
            img, elevation = _masked_image_and_elevation(res['mask'], res['mean'], res['img'], True)
            from .mapping.mapping import GenericMapping
            lat, lon, lat_c, lon_c = sm_grid_to_geographic(res, mapping.photoTime)
            return GenericMapping(lat, lon, lat_c, lon_c, elevation, mapping.altitude, img, mapping.cameraPosGCRS,
                                  mapping.photoTime, mapping.identifier)
    sm = convertMappingToSM(mapping)
    smResampled = resample(sm, **kw)
    return convertSMMappingToGeo(smResampled)


def sm_grid_to_geographic(res, time):
    """(lat, lon, lat_c, lon_c) of a result whose grid is in SM coordinates, as geographic coordinates at `time`:
    convertSMMappingToGeo (reference mapping.py:1549-1559) on the grid's arrays as they are, corners and centres through ONE
    ``smToLatLon`` call — building the SM mapping first would send the grid to the device and back through its properties,
    for the same numbers."""
    from .coordinates.transform import smToLatLon
    lat, lon, lat_c, lon_c = res['lat'], res['lon'], res['lat_c'], res['lon_c']
    nc = lat.size
    la, lo = smToLatLon(np.concatenate((lat.ravel(), lat_c.ravel())), np.concatenate((lon.ravel(), lon_c.ravel())), time)
    return la[:nc].reshape(lat.shape), lo[:nc].reshape(lon.shape), la[nc:].reshape(lat_c.shape), lo[nc:].reshape(lon_c.shape)


# 'single-pass' / 'two-pass': the plan the last resample() of a camera mapping took (None: the array pipeline)
last_plan = None


def _px_per_deg(pxPerDeg):
    try:
        _, _ = pxPerDeg
    except TypeError:
        assert pxPerDeg is not None
        pxPerDeg = (pxPerDeg, pxPerDeg)
    return tuple(pxPerDeg)


def _min_elevation(min_elevation):
    """The elevation threshold as the device calls take it: -inf for none."""
    return float('-inf') if min_elevation is None else float(min_elevation)


def _members(mappingOrCollection):
    """``(mappings, rebuild)``: the mappings to work on, and what makes the result out of the list of theirs (the one result
    for a mapping; for a collection a collection with its identifier and ``mayOverlap``).  ValueError for anything else."""
    if isinstance(mappingOrCollection, BaseMapping):
        return [mappingOrCollection], lambda done: done[0]
    if isinstance(mappingOrCollection, MappingCollection):
        # (the reference forgets the identifier here and raises TypeError, resample.py:151)
        return mappingOrCollection.mappings, lambda done: MappingCollection(done, mappingOrCollection.identifier,
                                                                           mayOverlap=mappingOrCollection.mayOverlap)
    raise ValueError('First argument must be a mapping or a mapping collection, but is: {}'.
                     format(type(mappingOrCollection)))


def _masked_image_and_elevation(mask, planes, image, has_elev):
    """``(img, elevation)`` as the mapping classes take them: image (ny,nx,C) masked where `mask` (ny,nx) is set, and the
    last plane of `planes` (ny,nx,C+1) masked where it is NaN (None without an elevation)."""
    img = ma.masked_array(image, mask=np.repeat(mask[:, :, None], image.shape[2], 2))
    elevation = ma.masked_invalid(planes[:, :, -1], copy=False) if has_elev else None
    return img, elevation


def _created(mapping, res, planes, image, has_elev):
    """``mapping.createResampled`` on the grid of the frame result `res`, with its `planes` and `image` of one statistic."""
    img, elevation = _masked_image_and_elevation(res['mask'], planes, image, has_elev)
    return mapping.createResampled(res['lat'], res['lon'], res['lat_c'], res['lon_c'], elevation, img)


def _pole_and_resolution(mapping, pxPerDeg, arcsecPerPx, containsPole):
    """``(containsPole, (latPxPerDeg, lonPxPerDeg))``: the caller's word or the mapping's; `arcsecPerPx` before `pxPerDeg`."""
    pole = mapping.containsPole if containsPole is None else containsPole
    ppd = plateCarreeResolution(mapping.boundingBox, arcsecPerPx) if arcsecPerPx else _px_per_deg(pxPerDeg)
    return pole, ppd


def resample(mappingOrCollection, pxPerDeg=25, arcsecPerPx=None, containsPole=None, method='mean'):
    """
    Returns a new mapping (or collection) where the colors and elevation are resampled into a
    regular latitude/longitude grid (plate carree projection) with y=latitude and x=longitude
    (reference resample.py:73-157).

    With 'mean' binning, holes appear at low elevation angles when the resampling resolution is
    high, because binning does not interpolate empty bins; mask the mapping by elevation
    (e.g. 10deg) first.

    :param mappingOrCollection:
    :param None|number|tuple pxPerDeg: tuple (latPxPerDeg, lonPxPerDeg) or a number if both are the same
    :param None|number arcsecPerPx: spherical resolution, used to approximate pxPerDeg; has precedence
    :param None|bool containsPole: specify True|False to skip the pole check
    :param method: binning: 'mean'; interpolation: 'nearest' (value of the closest pixel centre in the lat/lon
                   plane), 'linear' and 'cubic' (scipy's griddata: the Delaunay triangulation of the pixel centres — Qhull's,
                   triangle for triangle, wherever it is unique —; 'linear': the barycentric sum in the grid centre's
                   triangle; 'cubic': scipy's gradient estimator in scipy's order with its stopping rule and the Clough-Tocher
                   element; both equal to the reference up to summation order, ~1e-13 of a channel's span (and up to the per-channel sweep count of
                   the relaxation, a yes / no decision at scipy's tolerance: see csrc/amt_nearest.hip k_cubic_gs); a cubic overshoots, and an
                   integer image wraps like numpy's cast), all masked outside the mapping's outline.
    :rtype: a subclass of BaseMapping or MappingCollection
    """
    _check_method(method)

    def doResample(mapping):
        global last_plan
        last_plan = None
        fused = getattr(mapping, '_fused_resample', None)
        if fused is not None and method == 'mean':
            # a camera mapping whose arrays nobody has asked for yet (getMapping(...).maskedByElevation(e), the user
            # guide's flow): georeferencing, mask, bounding box and binning in ONE kernel; with arcsecPerPx (the call form
            # of the reference's CLI and tests) a box pass of the same kernel comes first (box-first plan)
            res = fused(None if arcsecPerPx else _px_per_deg(pxPerDeg), containsPole, arcsecPerPx=arcsecPerPx)
            if res is not None:
                last_plan = res['plan']
                return _created(mapping, res, res['mean'], res['img'], True)
        pole, ppd = _pole_and_resolution(mapping, pxPerDeg, arcsecPerPx, containsPole)
        res = resample_frame(mapping.frame(), mapping.altitude, mapping.boundingBox, ppd,
                             mapping.containsDiscontinuity, pole, method=method,
                             outline=mapping.outline if (method != 'mean' or pole) else None)
        return _created(mapping, res, res['mean'], res['img'], res['has_elev'])

    members, rebuild = _members(mappingOrCollection)
    return rebuild([doResample(m) for m in members])


def resampleMedian(mappingOrCollection, pxPerDeg=25, arcsecPerPx=None, containsPole=None):
    """
    Like :func:`resample` with ``method='mean'``, but every channel of a cell (image channels and elevation) is the
    median of the cell's pixels instead of their mean: ``np.median`` of the same pixel set the mean bins, the mean of the
    two middle values in float64 for an even count, then the image's rounding half to even and cast (reference
    resample.py:128-136).  A star, a city light or a hot pixel among a cell's pixels moves its mean but not its median.
    Same grid, box, pole and date-line rules as :func:`resample`; empty cells are masked where the mean masks them.

    The reference names ``method='median'`` and raises NotImplementedError for it (resample.py:353-357);
    ``resample(..., method='median')`` keeps doing so, as a drop-in for the reference must, so the median has a name of
    its own.  It reads ``mapping.frame()`` like ``method='nearest'`` (any mapping with a device frame, MIRACLE and
    direction arrays included) and runs on the device (``amt_median_frame``).

    :param mappingOrCollection:
    :param None|number|tuple pxPerDeg: tuple (latPxPerDeg, lonPxPerDeg) or a number if both are the same
    :param None|number arcsecPerPx: spherical resolution, used to approximate pxPerDeg; has precedence
    :param None|bool containsPole: specify True|False to skip the pole check
    :rtype: a subclass of BaseMapping or MappingCollection
    """
    def doResample(mapping):
        global last_plan
        last_plan = None
        pole, ppd = _pole_and_resolution(mapping, pxPerDeg, arcsecPerPx, containsPole)
        res = resample_frame_median(mapping.frame(), mapping.altitude, mapping.boundingBox, ppd,
                                    mapping.containsDiscontinuity, pole, outline=mapping.outline if pole else None)
        return _created(mapping, res, res['median'], res['img'], res['has_elev'])

    members, rebuild = _members(mappingOrCollection)
    return rebuild([doResample(m) for m in members])


def resampleMedianMLatMLT(mapping, **kw):
    """:func:`resampleMedian` such that MLat/MLT become regular grids (the path of :func:`resampleMLatMLT` through the
    SM mapping: ``convertMappingToSM`` -> ``resampleMedian`` -> ``convertSMMappingToGeo``).

    See :func:`resampleMedian` for parameters.
    """
    return convertSMMappingToGeo(resampleMedian(convertMappingToSM(mapping), **kw))


def quantile_list(q):
    """The quantiles of a call as a list of floats: a number or a sequence of 1 .. 8 numbers, each in [0, 1].  ValueError for
    anything else (NaN, an empty sequence, more than ``amt_quantile_frame`` takes in one call) — before any device work."""
    from ._native import QUANTILES_MAX
    try:
        qs = [float(q)] if np.ndim(q) == 0 else [float(v) for v in q]
    except (TypeError, ValueError):
        raise ValueError('q must be a number or a sequence of numbers, but is: {!r}'.format(q))
    if not 1 <= len(qs) <= QUANTILES_MAX:
        raise ValueError('between 1 and {} quantiles per call, got {}'.format(QUANTILES_MAX, len(qs)))
    for v in qs:
        if not 0.0 <= v <= 1.0:             # (False for NaN)
            raise ValueError('quantiles must be in the range [0, 1], got {!r}'.format(v))
    return qs


def resampleQuantile(mappingOrCollection, q, pxPerDeg=25, arcsecPerPx=None, containsPole=None):
    """
    Like :func:`resampleMedian`, but every channel of a cell (image channels and elevation) is the quantile `q` of the
    cell's pixels: ``np.quantile(values.astype(float64), q)`` with NumPy's default method ``'linear'``, bit for bit, then
    the image's rounding half to even and cast.  The lower quartile of a cell is a background estimate, the 0.9 quantile a
    peak estimate that single stars and city lights do not own, the difference of the quartiles a spread.

    A number `q` gives what :func:`resampleMedian` gives (a mapping, or a collection for a collection); a sequence of up to
    8 numbers gives a list with one such result per `q`, in order, from ONE device call per mapping
    (``amt_quantile_frame``): the pixels are assigned to cells and sorted into them once.  ``q=0.5`` is the median for
    the image; for the elevation ``np.quantile`` and ``np.median`` combine the middle pair differently and may differ in
    the last bit.

    :param number|sequence q: quantile(s) in [0, 1]; ValueError otherwise
    :param mappingOrCollection, pxPerDeg, arcsecPerPx, containsPole: see :func:`resampleMedian`
    :rtype: a subclass of BaseMapping or MappingCollection, or a list of them
    """
    qs = quantile_list(q)

    def doResample(mapping):
        global last_plan
        last_plan = None
        pole, ppd = _pole_and_resolution(mapping, pxPerDeg, arcsecPerPx, containsPole)
        res = resample_frame_quantile(mapping.frame(), mapping.altitude, mapping.boundingBox, ppd, qs,
                                      mapping.containsDiscontinuity, pole, outline=mapping.outline if pole else None)
        return [_created(mapping, res, res['quantile'][j], res['img'][j], res['has_elev']) for j in range(len(qs))]

    members, rebuild = _members(mappingOrCollection)
    per_mapping = [doResample(m) for m in members]
    # one result per quantile: of a collection, one collection per quantile with every member's mapping for it
    results = [rebuild([r[j] for r in per_mapping]) for j in range(len(qs))]
    return results[0] if np.ndim(q) == 0 else results


def resampleQuantileMLatMLT(mapping, q, **kw):
    """:func:`resampleQuantile` such that MLat/MLT become regular grids (``convertMappingToSM`` -> ``resampleQuantile`` ->
    ``convertSMMappingToGeo``, as :func:`resampleMedianMLatMLT`).

    See :func:`resampleQuantile` for parameters.
    """
    res = resampleQuantile(convertMappingToSM(mapping), q, **kw)
    return [convertSMMappingToGeo(r) for r in res] if isinstance(res, list) else convertSMMappingToGeo(res)


def min_coverage_weight(minCoverage):
    """The least total weight of a valid cell of the area-weighted binning, ``max(1, rint(minCoverage * 2^32))``; ValueError for
    a `minCoverage` outside [0, 1] (or NaN) — before any device work."""
    try:
        v = float(minCoverage)
    except (TypeError, ValueError):
        raise ValueError('minCoverage must be a number in [0, 1], but is: {!r}'.format(minCoverage))
    if not 0.0 <= v <= 1.0:                 # (False for NaN)
        raise ValueError('minCoverage must be in the range [0, 1], got {!r}'.format(minCoverage))
    return max(1, int(np.rint(v * 4294967296.0)))


def area_overflow_error(frame=None, function='resampleArea', what='mapping'):
    """The ValueError for ``AMT_EDOMAIN`` / a set overflow flag of the area-weighted binning; `frame`: the index of the frame in a
    sequence; `function`, `what`: who speaks and of what (the mosaic: 'resampleMosaic', 'collection')."""
    where = '' if frame is None else ' (frame {} of the sequence)'.format(frame)
    return ValueError('{}: a cell of the grid is covered more than 256 times over by the pixels; its sums do not '
                      'fit (is the resolution far too low for this {}?)'.format(function, what) + where)


def resampleArea(mappingOrCollection, pxPerDeg=25, arcsecPerPx=None, containsPole=None, minCoverage=0.5):
    """
    Area-weighted (conservative) resampling: like :func:`resample` with ``method='mean'`` on the same grid, but a pixel is the
    quadrilateral of its four corners and every cell it overlaps receives its colours and elevation, weighted with the
    fraction of the cell that the overlap covers.  A cell's value is the weighted mean over everything that overlaps it.

    ``resample(method='mean')`` puts a pixel into the one cell that holds its centre: where cells are smaller than pixels (low
    elevation angles, high resolutions) cells between the centres stay empty.  Here every cell that the pixels cover at least
    `minCoverage` of is filled, and what the pixels saw is conserved rather than interpolated between centres; where cells are
    larger than pixels, small pixels no longer count as much as large ones.  The weights are integers (``rint(fraction *
    2^32)``) summed with integer atomics on the device (``amt_area_frame``), so the result is exact, independent of the order
    of the pixels and the same bits on every run.  No counterpart in the reference; ``resample(method=...)`` keeps the
    reference's method list.

    A pixel takes part when its centre is unmasked (as for 'mean': mask the mapping by elevation first), its four corners are
    finite and it does not straddle the seam of the longitudes (after the pole rotation or the date-line shift).

    :param mappingOrCollection, pxPerDeg, arcsecPerPx, containsPole: see :func:`resample`
    :param number minCoverage: a cell is masked unless the pixels cover at least this fraction of it, in [0, 1]
                               (0: any overlap at all); ValueError otherwise
    :rtype: a subclass of BaseMapping or MappingCollection
    """
    min_coverage_weight(minCoverage)

    def doResample(mapping):
        global last_plan
        last_plan = None
        pole, ppd = _pole_and_resolution(mapping, pxPerDeg, arcsecPerPx, containsPole)
        res = resample_frame_area(mapping.frame(), mapping.altitude, mapping.boundingBox, ppd, mapping.containsDiscontinuity,
                                  pole, outline=mapping.outline if pole else None, minCoverage=minCoverage)
        return _created(mapping, res, res['area'], res['img'], res['has_elev'])

    members, rebuild = _members(mappingOrCollection)
    return rebuild([doResample(m) for m in members])


def resampleAreaMLatMLT(mapping, **kw):
    """:func:`resampleArea` such that MLat/MLT become regular grids (``convertMappingToSM`` -> ``resampleArea`` ->
    ``convertSMMappingToGeo``, as :func:`resampleMedianMLatMLT`).

    See :func:`resampleArea` for parameters.
    """
    min_coverage_weight(kw.get('minCoverage', 0.5))
    return convertSMMappingToGeo(resampleArea(convertMappingToSM(mapping), **kw))


def resampleMesh(mappingOrCollection, pxPerDeg=25, arcsecPerPx=None, containsPole=None):
    """
    Mesh resampling: linear interpolation on the pixel lattice, on the grid of :func:`resample`.  The pixel centres form a
    smoothly deformed lattice that carries a triangulation of its own, two triangles per quad of neighbouring centres; a cell
    takes the value that is linear inside the lattice triangle holding its centre, colours and elevation alike.  On a fine
    grid it fills the holes that centre binning leaves, smoothly where :func:`resampleArea` repeats a pixel's value over many
    cells.  One device call (``amt_mesh_frame``): no global triangulation, no host pass.

    Which pixels take part: those ``resample(method='mean')`` bins (unmasked centre, finite latitude — mask the mapping by
    elevation first) with a finite longitude.  A quad with four such corners gives two triangles, one with three gives their one
    triangle, so the mesh follows masks and the limb as closely as the data allows; a triangle as wide as half the globe (across
    the seam of the longitudes, after the pole rotation or the date-line shift) is dropped.  Cells outside every triangle are
    masked: the mesh itself is the footprint, no outline is used.

    How this differs from ``resample(method='linear')``: that is scipy's griddata, the barycentric sum in the DELAUNAY triangles
    of the pixel centres in (lon, lat) degrees, which takes an exact global triangulation (a third of a second for a 12 Mpx
    frame) and, on an oblique view, joins pixels that are not neighbours in the image.  Here the triangles are the lattice's:
    they always join image neighbours, and the diagonal of a quad is chosen by the empty-circle rule, so on a smooth convex
    lattice both triangulations coincide.  The contract (triangles, diagonal rule, watertight edge values, lowest id wins) is
    DESIGN.md §4.6; results are the same bits on every run.

    How this differs from :func:`resampleGather`: that samples the image through the camera model in closed form and needs one;
    it raises NotImplementedError for MIRACLE and THEMIS mappings, direction-array mappings and mappings read back from a file.
    This needs the per-pixel centre arrays only and works for every ``BaseMapping``.

    No counterpart in the reference; ``resample(method=...)`` keeps the reference's method list.

    :param mappingOrCollection, pxPerDeg, arcsecPerPx, containsPole: see :func:`resample`
    :rtype: a subclass of BaseMapping or MappingCollection
    """
    def doResample(mapping):
        global last_plan
        last_plan = None
        pole, ppd = _pole_and_resolution(mapping, pxPerDeg, arcsecPerPx, containsPole)
        res = resample_frame_mesh(mapping.frame(), mapping.altitude, mapping.boundingBox, ppd, mapping.containsDiscontinuity,
                                  pole, outline=mapping.outline if pole else None)
        return _created(mapping, res, res['mesh'], res['img'], res['has_elev'])

    members, rebuild = _members(mappingOrCollection)
    return rebuild([doResample(m) for m in members])


def resampleMeshMLatMLT(mapping, **kw):
    """:func:`resampleMesh` such that MLat/MLT become regular grids (``convertMappingToSM`` -> ``resampleMesh`` ->
    ``convertSMMappingToGeo``, as :func:`resampleMedianMLatMLT`): the lattice's triangles in (SM longitude, MLat).

    See :func:`resampleMesh` for parameters.
    """
    return convertSMMappingToGeo(resampleMesh(convertMappingToSM(mapping), **kw))


MOSAIC_STATISTICS = ('mean', 'median', 'quantile', 'area')


def mosaic_statistic(statistic, q, minCoverage=None):
    """The quantiles of a mosaic call as a list (None for 'mean', 'median' and 'area').  ValueError for an unknown statistic, `q`
    given with 'mean', 'median' or 'area', 'quantile' without `q`, what :func:`quantile_list` refuses, `minCoverage` given with
    another statistic than 'area' or outside [0, 1] — before any member is looked at."""
    if statistic not in MOSAIC_STATISTICS:
        raise ValueError('statistic must be one of {}, but is: {!r}'.format(', '.join(MOSAIC_STATISTICS), statistic))
    if minCoverage is not None:
        if statistic != 'area':
            raise ValueError('minCoverage={!r} goes with statistic=\'area\', not with {!r}'.format(minCoverage, statistic))
        min_coverage_weight(minCoverage)
    if statistic != 'quantile':
        if q is not None:
            raise ValueError('q={!r} goes with statistic=\'quantile\', not with {!r}'.format(q, statistic))
        return None
    if q is None:
        raise ValueError('statistic=\'quantile\' needs q: a number or a sequence of up to 8 numbers in [0, 1]')
    return quantile_list(q)


def resampleMosaic(collection, pxPerDeg=25, arcsecPerPx=None, containsPole=None, statistic='mean', q=None, minCoverage=None):
    """
    Bins every member of a :class:`MappingCollection` onto ONE grid and returns ONE mapping (:class:`MosaicMapping`), where
    :func:`resample` of a collection grids each member on its own box.

    The grid is the one :func:`resample` lays out for a single mapping with the collection's box
    (``collection.boundingBox``; ``arcsecPerPx``: ``plateCarreeResolution(collection.boundingBox, arcsecPerPx)``), with the
    date-line rule for every member when that box contains the discontinuity.  When ``containsPole`` is True (or None and a
    member contains a pole) every member's centres are rotated by +90 deg about x and the box is the union of the extents of
    the members' rotated outlines.  A member's pixel counts in a cell when ``resample`` would bin it there on the common
    grid and the cell meets the member's own bounding box (in the plan's coordinates).

    Overlaps follow ``collection.mayOverlap``: False — the mean over every member's pixels in the cell; True — the member
    with the highest mean elevation in the cell wins it whole (the reference's drawing rule for overlapping mappings,
    draw_helpers.py:128-178), the earlier member on a tie.  ``source`` holds the winning member's index per cell
    (``members`` their identifiers).  Members are read through ``mapping.frame()``.

    ``statistic`` names what a cell holds: ``'mean'`` (the default), ``'median'`` (``np.median`` as :func:`resampleMedian`
    computes it) or ``'quantile'`` (``np.quantile(..., q)`` as :func:`resampleQuantile`) — over every member's pixels in the
    cell (mayOverlap False), or over the winning member's pixels alone (True; the winner is the mean mosaic's).  A cell that a
    pass of frames or a network of cameras sees many times keeps its median when one star, one city light or one saturated frame
    moves its mean.  With ``'quantile'`` a number `q` gives one mapping, a sequence of 1 to 8 a list with one mapping per `q`
    from ONE device call (:func:`resampleQuantile`'s convention).

    ``'area'`` is the area-weighted mosaic: every member's pixels are the quadrilaterals of their corners and are shared among
    the cells of the common grid they overlap, with the integer weights of :func:`resampleArea` (``amt_area_mosaic_frames``).
    The other statistics put a pixel into the one cell that holds its centre, so towards the horizon, where pixels are many
    cells wide, every member leaves holes and the overlap rule chooses between whichever centres happened to land in a cell.
    mayOverlap False: the members' weighted sums are added and a cell is valid when together they cover at least `minCoverage`
    of it.  True: of the members that cover at least `minCoverage` of the cell on their OWN, the one with the highest weighted
    mean elevation wins it whole (the earlier member on a tie); a sliver of a well-placed member does not take a cell that
    another member covers.  ``source`` is set exactly where the cell is valid.  In the pole plan the members' corners are
    rotated like their centres.

    :param str statistic: 'mean' | 'median' | 'quantile' | 'area'
    :param None|number|sequence q: the quantile(s), for statistic='quantile' only
    :param None|number minCoverage: for statistic='area' only: a cell is masked unless the pixels cover at least this
                                    fraction of it, in [0, 1] (None: 0.5)
    :raises ValueError: for an unknown statistic, `q` with 'mean', 'median' or 'area', 'quantile' without `q`, `minCoverage`
                        with another statistic than 'area' or outside [0, 1] (all before the collection is looked at); for an
                        empty collection, members of different altitudes or image dtypes / channel counts, and a member
                        without elevation when ``mayOverlap`` is True; with 'area', when a cell is covered more than 256 times
                        over
    :rtype: MosaicMapping, or a list of them
    """
    qs = mosaic_statistic(statistic, q, minCoverage)
    res = mosaic_frames(collection, pxPerDeg, arcsecPerPx, containsPole, statistic=statistic, q=qs, minCoverage=minCoverage)
    if statistic == 'mean':
        return _mosaic_mapping(collection, res)
    if statistic == 'area':
        return _mosaic_mapping(collection, res, res['area'], res['img'])
    if statistic == 'median':
        return _mosaic_mapping(collection, res, res['median'], res['img'])
    out = [_mosaic_mapping(collection, res, res['quantile'][j], res['img'][j]) for j in range(len(qs))]
    return out[0] if np.ndim(q) == 0 else out


def resampleMosaicMLatMLT(collection, **kw):
    """:func:`resampleMosaic` such that MLat/MLT become regular grids: the members converted to SM coordinates
    (``convertMappingToSM``), the mosaic, and back (``convertSMMappingToGeo``), as :func:`resampleMedianMLatMLT` does.

    See :func:`resampleMosaic` for parameters; a list result (several quantiles) is mapped element by element.
    """
    from .mapping.mapping import MosaicMapping
    mosaic_statistic(kw.get('statistic', 'mean'), kw.get('q'), kw.get('minCoverage'))
    sm = MappingCollection([convertMappingToSM(m) for m in collection.mappings], collection.identifier,
                           mayOverlap=collection.mayOverlap)

    def toGeo(mosaic):
        geo = convertSMMappingToGeo(mosaic)
        return MosaicMapping(geo.lats, geo.lons, geo.latsCenter, geo.lonsCenter, geo.elevation, geo.altitude, geo.img,
                             geo.cameraPosGCRS, geo.photoTime, geo.identifier, mosaic.source, mosaic.members)

    mosaic = resampleMosaic(sm, **kw)
    return [toGeo(m) for m in mosaic] if isinstance(mosaic, list) else toGeo(mosaic)


def _mosaic_mapping(collection, res, planes=None, image=None):
    """The MosaicMapping of a mosaic_frames result; planes (ny,nx,C+1) / image (ny,nx,C): the statistic's, default the mean's."""
    from .mapping.mapping import MosaicMapping
    members = collection.mappings
    planes = res['mean'] if planes is None else planes
    image = res['img'] if image is None else image
    img, elevation = _masked_image_and_elevation(res['mask'], planes, image, res['has_elev'])
    source = ma.masked_array(res['source'], mask=res['source'] < 0)
    photoTime = collection.photoTime
    first = next(m for m in members if m.photoTime == photoTime)
    return MosaicMapping(res['lat'], res['lon'], res['lat_c'], res['lon_c'], elevation, res['altitude'], img,
                         first.cameraPosGCRS, photoTime, collection.identifier, source, [m.identifier for m in members])


def mosaic_axis_window(edges, lo, hi):
    """(first, count) of the cells [edges[c], edges[c+1]] that meet [lo, hi]: edges[c + 1] >= lo and edges[c] <= hi (the
    edges are np.linspace's, the numbers the device's bin_index compares with)."""
    edges = np.asarray(edges, dtype=np.float64)
    n = len(edges) - 1
    if not (hi >= lo):
        return 0, 0
    c0 = int(np.searchsorted(edges[1:], lo, side='left'))        # first c with edges[c + 1] >= lo
    c1 = int(np.searchsorted(edges[:-1], hi, side='right')) - 1  # last c with edges[c] <= hi
    c0, c1 = max(c0, 0), min(c1, n - 1)
    return (c0, c1 - c0 + 1) if c1 >= c0 else (0, 0)


def mosaic_plan(collection, pxPerDeg=25, arcsecPerPx=None, containsPole=None):
    """The host side of :func:`resampleMosaic`: checks the members and lays out the common grid and every member's window
    (:func:`mosaic_layout`).  Returns mosaic_layout's dict plus altitude, rule and the members' frames."""
    members = list(collection.mappings)
    if not members:
        raise ValueError('resampleMosaic: the collection %r is empty' % (collection.identifier,))
    altitudes = [m.altitude for m in members]
    if any(a != altitudes[0] for a in altitudes):
        raise ValueError('resampleMosaic: the members differ in altitude: %s' %
                         ', '.join('%s: %s km' % (m.identifier, m.altitude) for m in members))
    frames = [m.frame() for m in members]
    kinds = [(fd.img_dtype_code or 0, fd.nchan) for fd in frames]
    if any(k != kinds[0] for k in kinds):
        raise ValueError('resampleMosaic: the members differ in image dtype or channel count: %s' %
                         ', '.join('%s: %s x %d' % (m.identifier, fd.img_dtype, fd.nchan) for m, fd in zip(members, frames)))
    rule = 1 if collection.mayOverlap else 0
    if rule:
        missing = [m.identifier for m, fd in zip(members, frames) if fd.elev is None]
        if missing:
            raise ValueError('resampleMosaic: mayOverlap=True (highest elevation wins) needs every member\'s elevation; '
                             'without: %s' % ', '.join(str(i) for i in missing))
    altitude = altitudes[0]
    pole = any(m.containsPole for m in members) if containsPole is None else bool(containsPole)
    poleBoxes = None
    if pole:
        poleBoxes = []
        for m in members:
            outline = np.asarray(m.outline, dtype=np.float64)
            ola, olo = _rotate_pole_host(outline[:, 0], outline[:, 1], altitude, 90)
            poleBoxes.append((ola.min(), ola.max(), olo.min(), olo.max()))
    plan = mosaic_layout([m.boundingBox for m in members], pxPerDeg, arcsecPerPx, poleBoxes)
    plan.update(altitude=altitude, rule=rule, frames=frames)
    return plan


def mosaic_layout(memberBoxes, pxPerDeg=25, arcsecPerPx=None, poleBoxes=None):
    """The common grid and the member windows of a mosaic, on the host alone (see :func:`resampleMosaic`).

    :param memberBoxes: every member's BoundingBox (the collection's box is their merged box)
    :param poleBoxes: the pole plan: (latMin, latMax, lonMin, lonMax) of every member's rotated outline; None: the
                      geodetic plan (with the date-line rule when the merged box contains the discontinuity)
    :return: dict(grid, pole, discontinuity, lon_wrap, boxes [per member in the plan's coordinates; lonMin = None: all
             longitudes], windows [(x0, y0, nx, ny) per member, cells of the grid; (0, 0, 0, 0) when empty])
    """
    from .mapping.mapping import BoundingBox
    merged = BoundingBox.mergedBoundingBoxes(memberBoxes)
    disc, lon_wrap = False, 0
    if poleBoxes is not None:
        boxes = [tuple(b) for b in poleBoxes]
        latMin, latMax = min(b[0] for b in boxes), max(b[1] for b in boxes)
        lonMin, lonMax = min(b[2] for b in boxes), max(b[3] for b in boxes)
    else:
        latMin, latMax, lonMin, lonMax = merged.latSouth, merged.latNorth, merged.lonWest, merged.lonEast
        disc = merged.containsDiscontinuity
        boxes = []
        for b in memberBoxes:
            west, east = b.lonWest, b.lonEast
            if disc:
                west, east = wrap_at_180(west + 180), wrap_at_180(east + 180)
            # a member box that crosses the plan's discontinuity holds both ends of the longitude axis
            boxes.append((b.latSouth, b.latNorth, west, east) if west <= east else (b.latSouth, b.latNorth, None, None))
        if disc:
            lonMin, lonMax = wrap_at_180(lonMin + 180), wrap_at_180(lonMax + 180)
            lon_wrap = 1
    ppd = plateCarreeResolution(merged, arcsecPerPx) if arcsecPerPx else _px_per_deg(pxPerDeg)
    grid = cached_grid(ppd, latMin, latMax, lonMin, lonMax)
    windows = []
    for la0, la1, lo0, lo1 in boxes:
        x0, nx = (0, grid.nx) if lo0 is None else mosaic_axis_window(grid.xedges, lo0, lo1)
        y0, ny = mosaic_axis_window(grid.yedges, la0, la1)
        windows.append((x0, y0, nx, ny) if nx and ny else (0, 0, 0, 0))
    return dict(grid=grid, pole=poleBoxes is not None, discontinuity=disc, lon_wrap=lon_wrap, boxes=boxes, windows=windows)


def mosaic_frames(collection, pxPerDeg=25, arcsecPerPx=None, containsPole=None, statistic='mean', q=None, minCoverage=None):
    """The mosaic of a collection's device frames on the common grid (``amt_mosaic_frames``; ``amt_mosaic_median_frames`` /
    ``amt_mosaic_quantile_frames`` / ``amt_area_mosaic_frames`` for the other statistics): see :func:`resampleMosaic`.

    :return: dict(lat, lon, lat_c, lon_c [grid coordinates, host], mean (ny,nx,C+1), img (ny,nx,C), mask (ny,nx),
                  count (ny,nx), source (ny,nx) int32 [-1: empty], has_elev, plan); with statistic='median' ``median`` in place
                  of ``mean``, with 'quantile' ``quantile`` (nq,ny,nx,C+1) and img (nq,ny,nx,C), as
                  :func:`resample_frame_median` / :func:`resample_frame_quantile` return them, and ``q``; with 'area' ``area``
                  (ny,nx,C+1) in place of ``mean`` and ``coverage`` (ny,nx) in place of ``count``, as
                  :func:`resample_frame_area` returns them
    """
    qs = mosaic_statistic(statistic, q, minCoverage)
    area = statistic == 'area'
    least = min_coverage_weight(0.5 if minCoverage is None else minCoverage) if area else None
    plan = mosaic_plan(collection, pxPerDeg, arcsecPerPx, containsPole)
    grid, frames, altitude = plan['grid'], plan['frames'], plan['altitude']
    ctx = frames[0].ctx
    fd0 = frames[0]
    nch = fd0.nchan
    # (with 'area' every member hands over its corner arrays as well)
    table, keep = _mosaic_members(ctx, plan, AreaMosaicMember if area else MosaicMember, nch, corners=area)
    xaxis, yaxis = grid.axes(ctx)
    planes, img, mask, count, source = _mosaic_outputs(ctx, grid, nch, fd0.img_dtype_code, (len(qs),) if qs else ())
    head = [table, len(frames), fd0.img_dtype_code or 1, nch, float('-inf'), C.byref(xaxis), C.byref(yaxis), plan['lon_wrap'],
            plan['rule']]
    tail = [ptr(planes), ptr(img) if nch else None, ptr(mask), ptr(count), ptr(source)]
    if area:
        rc = ctx._lib.amt_area_mosaic_frames(ctx.handle, *(head + [least] + tail))
        if rc == -5:                            # AMT_EDOMAIN
            raise area_overflow_error(function='resampleMosaic', what='collection')
        ctx.check(rc)
    elif statistic == 'quantile':
        ctx.call('amt_mosaic_quantile_frames', *(head + [(C.c_double * len(qs))(*qs), len(qs)] + tail))
    else:
        ctx.call('amt_mosaic_frames' if statistic == 'mean' else 'amt_mosaic_median_frames', *(head + tail))
    out = _result(grid, plan['pole'], plan['discontinuity'], altitude, all(fd.elev is not None for fd in frames),
                  {statistic: planes, 'img': img, 'mask': mask, 'coverage' if area else 'count': count, 'source': source},
                  False, fd0.img_dtype if nch else None)
    del keep                     # (after the read-back above: the kernels are done with them)
    out.update(plan=plan)
    if qs:
        out.update(q=qs)
    return out


def _mosaic_members(ctx, plan, struct, nch, corners):
    """The member table of a mosaic call from a :func:`mosaic_plan`: `struct` (``MosaicMember``, or ``AreaMosaicMember`` with
    `corners`: the corner arrays are handed over as well) per member.  In the pole plan the centres, and the corners, are rotated.
    Returns the table and `keep`: the device arrays made here that the call reads."""
    frames, altitude = plan['frames'], plan['altitude']
    keep = []
    table = (struct * len(frames))()
    for i, (fd, window) in enumerate(zip(frames, plan['windows'])):
        lat_c, lon_c, lat, lon = fd.lat_c, fd.lon_c, fd.lat, fd.lon
        if plan['pole']:
            lat_c, lon_c = _rotate_pole_dev(ctx, lat_c, lon_c, altitude, 90)
            if corners:
                lat, lon = _rotate_pole_dev(ctx, lat, lon, altitude, 90)
            keep.append((lat_c, lon_c, lat, lon))
        t = table[i]
        first = (lat, lon, lat_c) if corners else (lat_c, lon_c)      # (the structs' leading fields, in their order)
        addr = [None if a is None else ptr(a).value for a in first + (fd.elev, fd.img if nch else None, fd.center_mask)]
        if corners:
            t.lat, t.lon, t.lat_c, t.elev, t.img, t.center_mask = addr
        else:
            t.lat_c, t.lon_c, t.elev, t.img, t.center_mask = addr
        t.height, t.width = fd.height, fd.width
        t.win_x0, t.win_y0, t.win_nx, t.win_ny = window
    return table, keep


def _mosaic_outputs(ctx, grid, nch, img_dtype_code, lead=()):
    """:func:`_bin_outputs` plus ``source`` (ny,nx) int32; without channels the image is zeroed (the call does not write it)."""
    import torch
    planes, img, mask, count = _bin_outputs(ctx, grid, nch, img_dtype_code, lead)
    if not nch:
        img.zero_()
    return planes, img, mask, count, ctx.empty((grid.ny, grid.nx), torch.int32)


def _bin_outputs(ctx, grid, nch, img_dtype_code, lead=(), count=True):
    """The device outputs of a binning call on `grid`, uninitialised: planes `lead` + (ny,nx,nch+1) float64, image `lead` +
    (ny,nx,max(nch,1)) uint8 (int16 holding the bits of a uint16 image), mask (ny,nx) uint8 and count (ny,nx) float64 (None
    with ``count=False``).  `lead`: ``()`` or ``(nq,)``, one set of planes and one image per quantile."""
    import torch
    planes = ctx.empty(lead + (grid.ny, grid.nx, nch + 1))
    img = ctx.empty(lead + (grid.ny, grid.nx, max(nch, 1)), torch.uint8 if img_dtype_code != 2 else torch.int16)
    mask = ctx.empty((grid.ny, grid.nx), torch.uint8)
    return planes, img, mask, ctx.empty((grid.ny, grid.nx)) if count else None


def _result(grid, contains_pole, contains_discontinuity, altitude, has_elev, tensors, keep_on_device, img_dtype=None):
    """
    The result dict of the frame-level functions: what describes the grid, and the outputs of the device calls.

    :param tensors: dict name -> device tensor, in the order they are read back ('sweeps': a number, passed through)
    :param keep_on_device: the tensors go into the result as they are and no grid coordinates are computed (sequence mode: the
                           grid is described by `grid`, first centre + step; coordinate arrays on demand, :func:`grid_coordinates`)
    :param img_dtype: NumPy dtype of the frame's image (None: no image, 'img' is read back as uint8)
    :return: dict(has_elev, grid, contains_pole, contains_discontinuity, altitude) plus either the tensors or lat, lon, lat_c,
             lon_c [grid coordinates] and the tensors as host arrays: 'img' as `img_dtype`, 'mask' as bool, 'source' as int32,
             'index' and 'triangles' as int64, everything else as it is (float64)
    """
    out = dict(has_elev=has_elev, grid=grid, contains_pole=contains_pole, contains_discontinuity=contains_discontinuity,
               altitude=altitude)
    if keep_on_device:
        out.update(tensors)
        return out
    out.update(grid_coordinates(out))
    dtypes = dict(img=np.uint8 if img_dtype is None else img_dtype, source=np.int32, index=np.int64, triangles=np.int64)
    for name, t in tensors.items():
        if name == 'sweeps':
            out[name] = t
        elif name == 'mask':
            out[name] = to_host(t).astype(bool)
        else:
            out[name] = to_host(t, dtype=dtypes.get(name))
    return out


def _resample_frame_ordered(fd, altitude, boundingBox, pxPerDeg, qs, containsDiscontinuity, containsPole, min_elevation,
                            outline, keep_on_device):
    """Median (`qs` None: ``amt_median_frame``) or quantile binning (`qs` a list of 1 .. 8 quantiles: ``amt_quantile_frame``,
    with a leading axis over them on the planes and the image) of a device-resident frame: the body of
    :func:`resample_frame_median` and :func:`resample_frame_quantile`."""
    ctx = fd.ctx
    grid, lat_c, lon_c, lon_wrap = _frame_grid(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity, containsPole,
                                               min_elevation, outline, None)
    xaxis, yaxis = grid.axes(ctx)
    nch = fd.nchan
    planes, img, mask, count = _bin_outputs(ctx, grid, nch, fd.img_dtype_code, (len(qs),) if qs else ())
    quantiles = [(C.c_double * len(qs))(*qs), len(qs)] if qs else []
    ctx.call('amt_quantile_frame' if qs else 'amt_median_frame', ptr(lat_c), ptr(lon_c), ptr(fd.elev), ptr(fd.img),
             fd.img_dtype_code or 1, nch, ptr(fd.center_mask), fd.height, fd.width, _min_elevation(min_elevation),
             C.byref(xaxis), C.byref(yaxis), lon_wrap, *(quantiles + [ptr(planes), ptr(img) if nch else None, ptr(mask),
                                                                      ptr(count)]))
    out = _result(grid, bool(containsPole), bool(containsDiscontinuity), altitude, fd.elev is not None,
                  {'quantile' if qs else 'median': planes, 'img': img, 'mask': mask, 'count': count}, keep_on_device,
                  fd.img_dtype if nch else None)
    if qs:
        out.update(q=qs)
    return out


def resample_frame_median(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity=False, containsPole=False,
                          min_elevation=None, outline=None, keep_on_device=False):
    """
    Median binning of a device-resident frame on the grid :func:`resample_frame` lays out (``amt_median_frame``).

    :param outline: the mapping's outline, needed for the pole box as in :func:`resample_frame`
    :param keep_on_device: the arrays stay device tensors and no grid coordinates are computed (sequence mode, as
                           :func:`resample_frame`)
    :return: dict(lat, lon, lat_c, lon_c [grid coordinates, host], median (ny,nx,C+1), img (ny,nx,C), mask (ny,nx),
                  count (ny,nx), has_elev)
    """
    return _resample_frame_ordered(fd, altitude, boundingBox, pxPerDeg, None, containsDiscontinuity, containsPole,
                                   min_elevation, outline, keep_on_device)


def resample_frame_quantile(fd, altitude, boundingBox, pxPerDeg, q, containsDiscontinuity=False, containsPole=False,
                            min_elevation=None, outline=None, keep_on_device=False):
    """
    Quantile binning of a device-resident frame on the grid :func:`resample_frame` lays out: every quantile of `q` (a
    number or up to 8 numbers in [0, 1]) from one call of ``amt_quantile_frame``.

    :param outline, keep_on_device: as for :func:`resample_frame_median`
    :return: the dict of :func:`resample_frame_median` with quantile (nq,ny,nx,C+1) and img (nq,ny,nx,C) in place of
             median and img, and ``q`` (the quantiles as a list); mask and count are (ny,nx)
    """
    return _resample_frame_ordered(fd, altitude, boundingBox, pxPerDeg, quantile_list(q), containsDiscontinuity, containsPole,
                                   min_elevation, outline, keep_on_device)


def resample_frame_area(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity=False, containsPole=False,
                        min_elevation=None, keep_on_device=False, outline=None, minCoverage=0.5):
    """
    Area-weighted binning of a device-resident frame on the grid :func:`resample_frame` lays out (``amt_area_frame`` +
    ``amt_area_frame_finalize``): see :func:`resampleArea`.  The corner arrays get the treatment the centre arrays get: rotated
    with the pole, or wrapped out of the date line in the kernel.

    :param outline, keep_on_device, min_elevation: as for :func:`resample_frame`
    :param minCoverage: a cell is valid when the pixels cover at least this fraction of it
    :raises ValueError: for `minCoverage` outside [0, 1]; when a cell is covered more than 256 times over (``AMT_EDOMAIN``:
                        the integer sums could wrap)
    :return: dict(lat, lon, lat_c, lon_c [grid coordinates, host], area (ny,nx,C+1) [weighted means, NaN where masked],
                  img (ny,nx,C), mask (ny,nx), coverage (ny,nx) [fraction of the cell that the pixels cover, every cell],
                  has_elev)
    """
    import torch
    least = min_coverage_weight(minCoverage)
    ctx = fd.ctx
    # (the accumulators are zeroed by torch on its current stream and added to by the library on the context's: the same one,
    #  also after a sequence pipeline has left the context on its own stream)
    ctx.bind()
    grid, lat_c, lon_c, lon_wrap = _frame_grid(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity, containsPole,
                                               min_elevation, outline, None)
    lat, lon = fd.lat, fd.lon
    if containsPole:
        # (without an outline _frame_grid has rotated the corners once already, for the box, and keeps only the centres; the
        #  class API always has the outline)
        lat, lon = _rotate_pole_dev(ctx, fd.lat, fd.lon, altitude, 90)
    xaxis, yaxis = grid.axes(ctx)
    nch = fd.nchan
    acc = ctx.zeros((nch + 2, grid.nx * grid.ny), torch.int64)
    ctx.call('amt_area_frame', ptr(lat), ptr(lon), ptr(lat_c), ptr(fd.elev), ptr(fd.img), fd.img_dtype_code or 1, nch,
             ptr(fd.center_mask), fd.height, fd.width, _min_elevation(min_elevation), C.byref(xaxis), C.byref(yaxis), lon_wrap,
             ptr(acc))
    area, img, mask, coverage = _bin_outputs(ctx, grid, nch, fd.img_dtype_code)
    rc = ctx._lib.amt_area_frame_finalize(ctx.handle, ptr(acc), grid.nx, grid.ny, nch, fd.img_dtype_code or 1, least, ptr(area),
                                          ptr(img) if nch else None, ptr(mask), ptr(coverage))
    if rc == -5:                            # AMT_EDOMAIN
        raise area_overflow_error()
    ctx.check(rc)
    if not nch:
        img.zero_()                         # (ny,nx,1) so that the result has an image; no kernel writes it without channels
    return _result(grid, bool(containsPole), bool(containsDiscontinuity), altitude, fd.elev is not None,
                   dict(area=area, img=img, mask=mask, coverage=coverage), keep_on_device, fd.img_dtype if nch else None)


def resample_frame_mesh(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity=False, containsPole=False,
                        min_elevation=None, keep_on_device=False, outline=None):
    """
    Mesh resampling of a device-resident frame on the grid :func:`resample_frame` lays out (one ``amt_mesh_frame`` call, which
    only enqueues): see :func:`resampleMesh`.  The centre arrays are rotated with the pole, or wrapped out of the date line in
    the kernel, like those of the other frame functions.

    :param outline: the mapping's outline, needed for the pole box only (as for :func:`resample_frame_area`); no cell is
                    masked by it — the mesh is the footprint
    :param keep_on_device, min_elevation: as for :func:`resample_frame`
    :return: dict(lat, lon, lat_c, lon_c [grid coordinates, host], mesh (ny,nx,C+1) [NaN where masked], img (ny,nx,C),
                  mask (ny,nx), triangle (ny,nx) int32 [the id of the lattice triangle that holds the cell's centre: 2 q + k for
                  triangle k of the quad q = r * (width - 1) + c; -1 where masked], has_elev)
    """
    import torch
    ctx = fd.ctx
    ctx.bind()
    grid, lat_c, lon_c, lon_wrap = _frame_grid(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity, containsPole,
                                               min_elevation, outline, None)
    xaxis, yaxis = grid.axes(ctx)
    cell_lat, cell_lon = grid.device_centers(ctx)
    nch = fd.nchan
    mesh, img, mask, _ = _bin_outputs(ctx, grid, nch, fd.img_dtype_code, count=False)
    triangle = ctx.empty((grid.ny, grid.nx), torch.int32)
    claim = ctx.empty((grid.nx * grid.ny,), torch.int32)        # the call's claim words: any contents, set anew by the call
    ctx.call('amt_mesh_frame', ptr(lat_c), ptr(lon_c), ptr(fd.elev), ptr(fd.img), fd.img_dtype_code or 1, nch,
             ptr(fd.center_mask), fd.height, fd.width, _min_elevation(min_elevation), C.byref(xaxis), C.byref(yaxis), lon_wrap,
             ptr(cell_lat), ptr(cell_lon), ptr(mesh), ptr(img) if nch else None, ptr(mask), ptr(triangle), ptr(claim))
    if not nch:
        img.zero_()                         # (ny,nx,1) so that the result has an image; no kernel writes it without channels
    return _result(grid, bool(containsPole), bool(containsDiscontinuity), altitude, fd.elev is not None,
                   dict(mesh=mesh, img=img, mask=mask, triangle=triangle), keep_on_device, fd.img_dtype if nch else None)


# ---- map-projected resampling ------------------------------------------------------------------------------------------------
# The reference's three map products (auromat/draw.py: drawStereographic, drawStereographicMLatMLT, drawMLatMLTPolar) as arrays:
# the members' pixels, as the quadrilaterals of their projected corners, area-weighted onto the square cells of a map plane.

def projected_km_per_px(kmPerPx=None, arcsecPerPx=100):
    """The cell size in km: `kmPerPx`, else `arcsecPerPx` of arc on the equator (the reference's default of 100 arcsec: 3.092 km)."""
    km = float(kmPerPx) if kmPerPx else wgs84A * (float(arcsecPerPx) / 3600) * (np.pi / 180)
    if not (km > 0 and np.isfinite(km)):
        raise ValueError('the resolution must be positive, got kmPerPx={!r}, arcsecPerPx={!r}'.format(kmPerPx, arcsecPerPx))
    return km


def projected_edges(extent, kmPerPx):
    """The edges of ``ceil(extent / kmPerPx)`` cells of `kmPerPx` km centred on 0 (ascending); ValueError for an empty grid."""
    n = int(np.ceil(extent / kmPerPx)) if np.isfinite(extent) else 0
    if n < 1:
        raise ValueError('empty grid: a map of {!r} km at {!r} km per pixel'.format(extent, kmPerPx))
    return np.linspace(-n * kmPerPx / 2, n * kmPerPx / 2, n + 1)


def stereographic_geometry(boundingBoxes, lat0=None, lon0=None, width=None, height=None, boundingBox=None, sizeFactor=1):
    """(lat0, lon0, width, height) of a stereographic map as drawStereographic chooses them (reference draw.py:192-203): what is
    missing comes from `boundingBox`, else from the merged `boundingBoxes` — its centre, and 1.05 * sizeFactor times its size."""
    if lat0 is None or lon0 is None or width is None or height is None:
        if boundingBox is None:
            boundingBox = BoundingBox.mergedBoundingBoxes(boundingBoxes)
        if lat0 is None:
            lat0 = boundingBox.center.lat
        if lon0 is None:
            lon0 = boundingBox.center.lon
        if width is None:
            width = boundingBox.size.width * 1.05 * sizeFactor
        if height is None:
            height = boundingBox.size.height * 1.05 * sizeFactor
    return float(lat0), float(lon0), float(width), float(height)


def polar_geometry(latSouth, latNorth, radius):
    """(north, bounding latitude, half width in km) of a polar map as drawMLatMLTPolar chooses them (reference
    draw.py:375-385): north when the middle latitude is positive; 5 degrees beyond the far latitude; a square that holds the
    bounding parallel."""
    north = (latSouth + latNorth) / 2 > 0
    bounding = latSouth - 5 if north else latNorth + 5
    return bool(north), float(bounding), float(radius * (90 - abs(bounding)) * np.pi / 180)


def _flat_mappings(mappings):
    """A mapping, a MappingCollection or a list of either -> (the mappings, the items whose bounding boxes the reference merges)"""
    items = mappings if isinstance(mappings, (list, tuple)) else [mappings]
    flat = []
    for item in items:
        if isinstance(item, MappingCollection):
            flat.extend(item.mappings)
        elif isinstance(item, BaseMapping):
            flat.append(item)
        else:
            raise ValueError('expected mappings or mapping collections, but got: {}'.format(type(item)))
    if not flat:
        raise ValueError('no mapping to resample')
    return flat, items


def project_and_bin(frames, projection, xEdges, yEdges, min_elevation=None):
    """
    The device part of the projected resampling: for every frame, ``amt_project_forward`` on its corner arrays and
    ``amt_area_plane_frame`` into ONE accumulator on the plane grid (`xEdges`, `yEdges` ascending, km).

    :param frames: list of FrameData with the same channel count and image type
    :return: (accumulators: device tensor int64 (C + 2, nx * ny) in the layout of ``amt_area_frame``, list of the projected
             corner arrays (x, y) per frame: device tensors)
    """
    import torch
    fd0 = frames[0]
    ctx = fd0.ctx
    ctx.bind()
    nch, code = fd0.nchan, fd0.img_dtype_code
    for fd in frames:
        if fd.nchan != nch or fd.img_dtype_code != code:
            raise ValueError('the mappings differ in their channel count or image type')
    (xaxis, _), (yaxis, _) = make_axis(ctx, xEdges, uniform=True), make_axis(ctx, yEdges, uniform=True)
    nx, ny = len(xEdges) - 1, len(yEdges) - 1
    acc = ctx.zeros((nch + 2, nx * ny), torch.int64)
    planes = []
    for fd in frames:
        x, y = ctx.empty(fd.lat.shape), ctx.empty(fd.lat.shape)
        ctx.call('amt_project_forward', C.byref(projection.params), ptr(fd.lat), ptr(fd.lon), fd.lat.numel(), ptr(x), ptr(y))
        ctx.call('amt_area_plane_frame', ptr(x), ptr(y), ptr(fd.lat_c), ptr(fd.elev), ptr(fd.img) if nch else None, code or 1,
                 nch, ptr(fd.center_mask), fd.height, fd.width, _min_elevation(min_elevation), C.byref(xaxis), C.byref(yaxis),
                 ptr(acc))
        planes.append((x, y))
    return acc, planes


class _PlaneGrid(object):
    """nx, ny of a plane grid, for :func:`_bin_outputs`"""

    def __init__(self, xEdges, yEdges):
        self.nx, self.ny = len(xEdges) - 1, len(yEdges) - 1


def resample_frames_projected(frames, projection, xEdges, yEdges, minCoverage=0.5, min_elevation=None):
    """
    Area-weighted binning of device-resident frames on a map plane: :func:`project_and_bin`, ``amt_area_frame_finalize``, and
    the inverse projection of the cell corners and centres (one ``amt_project_inverse`` call for both).

    :return: dict(area (ny,nx,C+1), img (ny,nx,C), mask (ny,nx) bool, coverage (ny,nx), lat, lon (ny+1,nx+1), lat_c, lon_c
             (ny,nx) [in the projection's own coordinates], has_elev), row 0 the row of the largest y
    :raises ValueError: `minCoverage` outside [0, 1]; a cell covered more than 256 times over
    """
    least = min_coverage_weight(minCoverage)
    fd0 = frames[0]
    ctx, nch, code = fd0.ctx, fd0.nchan, fd0.img_dtype_code
    xEdges, yEdges = np.asarray(xEdges, dtype=np.float64), np.asarray(yEdges, dtype=np.float64)
    acc, _ = project_and_bin(frames, projection, xEdges, yEdges, min_elevation)
    grid = _PlaneGrid(xEdges, yEdges)
    area, img, mask, coverage = _bin_outputs(ctx, grid, nch, code)
    rc = ctx._lib.amt_area_frame_finalize(ctx.handle, ptr(acc), grid.nx, grid.ny, nch, code or 1, least, ptr(area),
                                          ptr(img) if nch else None, ptr(mask), ptr(coverage))
    if rc == -5:                            # AMT_EDOMAIN
        raise area_overflow_error()
    ctx.check(rc)
    if not nch:
        img.zero_()
    # corners (ny + 1, nx + 1) and centres (ny, nx) of the cells, north (largest y) first, through one inverse call
    xc, yc = (xEdges[:-1] + xEdges[1:]) / 2, (yEdges[:-1] + yEdges[1:]) / 2
    gx, gy = np.meshgrid(xEdges, yEdges[::-1])
    cx, cy = np.meshgrid(xc, yc[::-1])
    px, py = np.concatenate((gx.ravel(), cx.ravel())), np.concatenate((gy.ravel(), cy.ravel()))
    la, lo = projection.inverse(px, py)
    nc = gx.size
    out = dict(has_elev=all(fd.elev is not None for fd in frames), lat=la[:nc].reshape(gx.shape), lon=lo[:nc].reshape(gx.shape),
               lat_c=la[nc:].reshape(cx.shape), lon_c=lo[nc:].reshape(cx.shape), area=to_host(area),
               img=to_host(img, dtype=fd0.img_dtype if nch else np.uint8), mask=to_host(mask).astype(bool),
               coverage=to_host(coverage))
    return out


def _projected_mapping(members, res, projection, xEdges, yEdges, frame):
    """The ProjectedMapping of a resample_frames_projected result; the magnetic forms go through the arithmetic of
    convertSMMappingToGeo first, so that the coordinate arrays are geographic like every other result's."""
    from .mapping.mapping import ProjectedMapping
    times = sorted(m.photoTime for m in members)
    photoTime = times[len(times) // 2]
    first = next(m for m in members if m.photoTime == photoTime)
    lat, lon, lat_c, lon_c = res['lat'], res['lon'], res['lat_c'], res['lon_c']
    if frame == 'sm':
        lat, lon, lat_c, lon_c = sm_grid_to_geographic(res, photoTime)
    img, elevation = _masked_image_and_elevation(res['mask'], res['area'], res['img'], res['has_elev'])
    return ProjectedMapping(lat, lon, lat_c, lon_c, elevation, first.altitude, img, first.cameraPosGCRS, photoTime,
                            first.identifier, projection, xEdges, yEdges, res['coverage'], frame)


def _resample_stereographic(members, boxes, frame, lat0, lon0, width, height, boundingBox, sizeFactor, kmPerPx, arcsecPerPx,
                            minCoverage):
    from .coordinates.projection import Stereographic
    min_coverage_weight(minCoverage)
    km = projected_km_per_px(kmPerPx, arcsecPerPx)
    lat0, lon0, width, height = stereographic_geometry((b.boundingBox for b in boxes), lat0, lon0, width, height, boundingBox,
                                                       sizeFactor)
    xEdges, yEdges = projected_edges(width, km), projected_edges(height, km)
    projection = Stereographic(lat0, lon0, wgs84A, wgs84B)
    res = resample_frames_projected([m.frame() for m in members], projection, xEdges, yEdges, minCoverage)
    return _projected_mapping(members, res, projection, xEdges, yEdges, frame)


def resampleStereographic(mappings, lat0=None, lon0=None, width=None, height=None, boundingBox=None, sizeFactor=1, kmPerPx=None,
                          arcsecPerPx=100, minCoverage=0.5):
    """
    The raster of the reference's ``drawStereographic`` (auromat/draw.py:140-222, Basemap 'stere' with ellps='WGS84'): the
    mappings on the square cells of a stereographic map plane centred on (`lat0`, `lon0`), `width` x `height` km.

    Every pixel is the quadrilateral of its four projected corners and is shared among the cells it overlaps with the integer
    weights of :func:`resampleArea` (``amt_project_forward`` + ``amt_area_plane_frame``): exact, independent of the order,
    the same bits on every run.  All members are binned into ONE accumulator: a cell's value is the weighted mean over
    everything that overlaps it (the union rule); a collection's ``mayOverlap`` plays no role.  A pixel takes part when its
    centre is unmasked (mask the mappings by elevation first) and its four corners are finite and lie within 90 degrees of
    the map's centre; there is no limit on its extent in the plane.

    :param mappings: a mapping, a MappingCollection or a list of either
    :param lat0, lon0: the centre in degrees; default: the centre of the (merged) bounding box
    :param width, height: of the map in km; default: 1.05 * sizeFactor times the size of the (merged) bounding box
    :param BoundingBox boundingBox: the box the defaults are taken from, in place of the mappings' own
    :param number kmPerPx: the cell size; default: `arcsecPerPx` of arc on the equator (100 arcsec: 3.092 km)
    :param number minCoverage: a cell is masked unless the pixels cover at least this fraction of it, in [0, 1]
    :raises ValueError: `minCoverage` outside [0, 1]; an empty grid; a cell covered more than 256 times over
    :rtype: ProjectedMapping: ``nx = ceil(width / kmPerPx)`` by ``ny`` cells around the centre, row 0 the northernmost;
            coordinates by the inverse projection, ``projection``, ``xEdges``, ``yEdges`` (km), ``coverage``, ``planeFrame``
    """
    members, boxes = _flat_mappings(mappings)
    return _resample_stereographic(members, boxes, 'geo', lat0, lon0, width, height, boundingBox, sizeFactor, kmPerPx,
                                   arcsecPerPx, minCoverage)


def _to_sm(mappings):
    """The mappings, collections or list of either with every mapping converted to SM coordinates"""
    def conv(item):
        if isinstance(item, MappingCollection):
            return MappingCollection([convertMappingToSM(m) for m in item.mappings], item.identifier, mayOverlap=item.mayOverlap)
        if isinstance(item, BaseMapping):
            return convertMappingToSM(item)
        raise ValueError('expected mappings or mapping collections, but got: {}'.format(type(item)))
    return [conv(i) for i in mappings] if isinstance(mappings, (list, tuple)) else conv(mappings)


def resampleStereographicMLatMLT(mappings, **kw):
    """
    :func:`resampleStereographic` in (MLat, SM longitude): the raster of the reference's ``drawStereographicMLatMLT``
    (auromat/draw.py:224-240), which converts the mappings with ``convertMappingToSM`` and projects the magnetic coordinates
    with the same WGS84 stereographic projection.  `lat0`, `lon0` and `boundingBox` are magnetic; the coordinate arrays of the
    result are geographic (the arithmetic of ``convertSMMappingToGeo``), its ``planeFrame`` is ``'sm'``.

    See :func:`resampleStereographic` for parameters.
    """
    min_coverage_weight(kw.get('minCoverage', 0.5))
    members, boxes = _flat_mappings(_to_sm(mappings))
    args = dict(lat0=None, lon0=None, width=None, height=None, boundingBox=None, sizeFactor=1, kmPerPx=None, arcsecPerPx=100,
                minCoverage=0.5)
    unknown = set(kw) - set(args)
    if unknown:
        raise TypeError('unexpected arguments: {}'.format(sorted(unknown)))
    args.update(kw)
    return _resample_stereographic(members, boxes, 'sm', **args)


def resampleMLatMLTPolar(mappings, boundingBox=None, kmPerPx=None, arcsecPerPx=100, minCoverage=0.5):
    """
    The raster of the reference's ``drawMLatMLTPolar`` (auromat/draw.py:242-317, Basemap 'npaeqd' / 'spaeqd' with lon_0 = 180
    on Basemap's sphere of 6370.997 km): the mappings in (MLat, SM longitude) on a polar azimuthal equidistant map, magnetic
    midnight (MLT 0, SM longitude 180) at the bottom of a north polar map.

    North when the middle of the magnetic latitude range is positive; the map is the square around the bounding parallel 5
    degrees beyond the range's far end (``latSouth - 5`` / ``latNorth + 5``), half width ``R (90 - |bounding latitude|) pi / 180``.
    Binning, admission and the union rule are :func:`resampleStereographic`'s; pixels of the other hemisphere take no part.

    :param BoundingBox boundingBox: magnetic; its latitude range in place of the mappings' own
    :rtype: ProjectedMapping with ``planeFrame == 'sm'`` and geographic coordinate arrays
    """
    from .coordinates.projection import BASEMAP_SPHERE_RADIUS, PolarAzimuthalEquidistant
    min_coverage_weight(minCoverage)
    km = projected_km_per_px(kmPerPx, arcsecPerPx)
    members, boxes = _flat_mappings(_to_sm(mappings))
    if boundingBox is None:
        boundingBox = BoundingBox.mergedBoundingBoxes([b.boundingBox for b in boxes])
    north, _, half = polar_geometry(boundingBox.latSouth, boundingBox.latNorth, BASEMAP_SPHERE_RADIUS)
    xEdges = yEdges = projected_edges(2 * half, km)
    projection = PolarAzimuthalEquidistant(north, 180.0, BASEMAP_SPHERE_RADIUS)
    res = resample_frames_projected([m.frame() for m in members], projection, xEdges, yEdges, minCoverage)
    return _projected_mapping(members, res, projection, xEdges, yEdges, 'sm')


# ---- scan-line maps ----------------------------------------------------------------------------------------------------------
# The raster of the reference's drawScanLinesCo / drawScanLinesMLatMLTCo (auromat/draw.py:589-879): every frame of a sequence
# contributes the strip through its centroid, perpendicular to the direction of flight, and all strips lie on one grid.

class _ScanLineRule(object):
    """The strip rule of the reference (draw.py:635-738), one frame at a time: constants from the first step, then per frame
    the azimuth from the camera footpoints and the strip's polygon."""

    def __init__(self, firstProps, firstCellDiagonal, lineWidthFactor=1):
        from .coordinates import geodesic
        bb = firstProps.boundingBox
        # constant height of the rotated box: bigger than needed, so that it holds as much as possible
        self.height = geodesic.distance(bb.topLeft, bb.bottomRight) * 1.5
        self.firstCellDiagonal, self.lineWidthFactor = float(firstCellDiagonal), lineWidthFactor
        self.width = self.deltaAzimuth = self.deltaDistance = self.az = None

    def strip(self, cur, nxt):
        """(polygon (m, 2) [lat, lon], azimuth) of the frame with properties `cur`; `nxt`: the next frame's, None for the
        last frame (it reuses the previous azimuth)."""
        from .coordinates import geodesic
        if nxt is not None:
            azCamFoot = geodesic.course(cur.cameraFootpoint, nxt.cameraFootpoint)
        if self.width is None:
            if nxt is None:
                raise ValueError('mapping sequence too short, need at least 2 mappings')
            # wide enough for a cell to fit whatever the strip's orientation: three diagonals of the first cell
            consecutive = geodesic.distance(cur.centroid, nxt.centroid)
            self.width = max(self.firstCellDiagonal * 3, consecutive) * self.lineWidthFactor
            self.deltaDistance = geodesic.distance(cur.cameraFootpoint, cur.centroid)
            self.deltaAzimuth = azCamFoot - geodesic.course(cur.cameraFootpoint, cur.centroid)
        if nxt is not None:
            # the centroids' track from the footpoints' (smooth), assuming the camera does not move against the spacecraft
            toCentroid = azCamFoot - self.deltaAzimuth
            a = geodesic.destination(cur.cameraFootpoint, toCentroid, self.deltaDistance)
            b = geodesic.destination(nxt.cameraFootpoint, toCentroid, self.deltaDistance)
            self.az = geodesic.course(a, b)
        az, w2, h2 = self.az, self.width / 2, self.height / 2
        for pole in (90, -90):
            if geodesic.distance(cur.centroid, geodesic.Location(pole, 0.0)) <= np.hypot(w2, h2) * 1.01:
                raise ValueError('scan lines: the strip of frame {!r} reaches a pole'.format(cur.identifier))
        middleRight = geodesic.destination(cur.centroid, az, w2)
        middleLeft = geodesic.destination(cur.centroid, az + 180, w2)
        topLeft = geodesic.destination(middleLeft, az - 90, h2)
        bottomLeft = geodesic.destination(middleLeft, az + 90, h2)
        topRight = geodesic.destination(middleRight, az - 90, h2)
        bottomRight = geodesic.destination(middleRight, az + 90, h2)
        # (without the last point of each line: no point twice)
        polygon = np.concatenate((geodesic.line(topLeft, topRight)[:-1], geodesic.line(topRight, bottomRight)[:-1],
                                  geodesic.line(bottomRight, bottomLeft)[:-1], geodesic.line(bottomLeft, topLeft)[:-1]))
        return polygon, az


def scanline_strips(props, firstCellDiagonal, lineWidthFactor=1):
    """
    The strips of a sequence's scan-line map (reference draw.py:635-738), on the host.

    :param props: list of ``MappingProperties`` (boundingBox, centroid, cameraFootpoint, ...) of the unresampled frames
    :param firstCellDiagonal: metres between corners 0 and 2 of the first unmasked cell of the first resampled frame
    :param lineWidthFactor: widens the strips, for sequences with frames missing
    :return: dict(polygons [per frame (m, 2) [lat, lon]], azimuths [per frame, degrees], width, height [metres])
    :raises ValueError: fewer than two frames; a strip that reaches a pole
    """
    props = list(props)
    if len(props) < 2:
        raise ValueError('mapping sequence too short, need at least 2 mappings')
    rule = _ScanLineRule(props[0], firstCellDiagonal, lineWidthFactor)
    strips = [rule.strip(cur, nxt) for cur, nxt in zip(props, props[1:] + [None])]
    return dict(polygons=[s[0] for s in strips], azimuths=[s[1] for s in strips], width=rule.width, height=rule.height)


def scanline_longitude_frame(firstCentroid):
    """True when a sequence is resampled in longitudes shifted by 180 degrees (``containsDiscontinuity=True`` for every frame):
    the first frame's centroid lies nearer the date line than longitude 0."""
    return bool(abs(firstCentroid.lon) > 90)


def scanline_check_fits(boundingBox, shifted, frame, identifier=None):
    """ValueError when a frame's box does not fit the sequence's longitude frame: it contains +-180 (unshifted), or its
    shifted west edge lies east of its shifted east edge (shifted).  All frames of a scan-line map share one lattice, and 180
    degrees is not a whole number of its cells."""
    if shifted:
        fits = wrap_at_180(boundingBox.lonWest + 180) <= wrap_at_180(boundingBox.lonEast + 180)
    else:
        fits = not boundingBox.containsDiscontinuity
    if not fits:
        raise ValueError('scan lines: frame {} ({!r}) does not fit the longitude frame of the sequence ({}): the sequence spans '
                         'the seam of its longitude frame'.format(frame, identifier,
                                                                  'shifted by 180 degrees' if shifted else 'unshifted'))


def lons_contain_discontinuity(lons):
    """``BoundingBox.minimumBoundingBox(points).containsDiscontinuity`` for points with the longitudes `lons`, without the
    quadratic table of the general merge: the box is the complement of the widest gap between neighbouring longitudes (the
    first widest in ascending order), and it crosses +-180 unless that gap is the one across +-180."""
    cuts = np.sort(np.asarray(lons, dtype=np.float64).ravel())
    if cuts.size < 2:
        return False
    gaps = np.concatenate((cuts[1:] - cuts[:-1], [cuts[0] + 360.0 - cuts[-1]]))
    k = int(np.argmax(gaps))
    return k != cuts.size - 1 and bool(wrap_at_180(cuts[k + 1]) > wrap_at_180(cuts[k]))


def scanline_global_axes(pxPerDeg):
    """(latitude nodes ascending, longitude nodes ascending) of the global lattice every grid of `pxPerDeg` is cut from"""
    latPxPerDeg, lonPxPerDeg = pxPerDeg
    return (_global_axis(-90, 90, int(round(latPxPerDeg * 180 + 1))), _global_axis(-180, 180, int(round(lonPxPerDeg * 360 + 1))))


def _nearest_node(axis, value):
    i = int(np.clip(np.searchsorted(axis, value), 1, len(axis) - 1))
    i = i - 1 if abs(axis[i - 1] - value) <= abs(axis[i] - value) else i
    step = axis[1] - axis[0]
    assert abs(axis[i] - value) < 1e-3 * step, 'a cell centre {!r} off the global lattice (nearest node {!r})'.format(value, axis[i])
    return i


def scanline_global_origin(grid, pxPerDeg):
    """(global row of the grid's row 0, global column of its column 0).  Global rows count the latitude nodes from the north
    (row = number of nodes - 1 - node), global columns the longitude nodes from the west, in the coordinates the grid is laid
    out in; a cell's index is that of the node nearest its centre (asserted to be within 1e-3 of a step)."""
    latAll, lonAll = scanline_global_axes(pxPerDeg)
    top = _nearest_node(latAll, grid.latCenters[0])
    assert _nearest_node(latAll, grid.latCenters[-1]) == top - (grid.ny - 1)
    left = _nearest_node(lonAll, grid.lonCenters[0])
    assert _nearest_node(lonAll, grid.lonCenters[-1]) == left + (grid.nx - 1)
    return len(latAll) - 1 - top, left


def scanline_union_grid(pxPerDeg, rowMin, rowMax, colMin, colMax):
    """The :class:`_Grid` of the cells with the global rows rowMin .. rowMax and columns colMin .. colMax
    (:func:`scanline_global_origin`): laid out by ``fixedGrid`` from the nodes one beyond each end, which it returns as they
    are; its size is checked, and its centres and corners are then taken from the global axes themselves (``linspace`` between
    two nodes gives the nodes in between only up to rounding)."""
    latAll, lonAll = scanline_global_axes(pxPerDeg)
    n = len(latAll) - 1
    lo, hi = n - rowMax, n - rowMin                                     # latitude nodes of the bottom and the top row
    assert 1 <= lo <= hi <= n - 1 and 1 <= colMin <= colMax <= len(lonAll) - 2, 'the union reaches the end of the lattice'
    grid = _Grid(pxPerDeg, latAll[lo - 1], latAll[hi + 1], lonAll[colMin - 1], lonAll[colMax + 1])
    assert (grid.ny, grid.nx) == (rowMax - rowMin + 1, colMax - colMin + 1), (grid.ny, grid.nx)
    latStep, lonStep = latAll[0] - latAll[1], lonAll[1] - lonAll[0]
    grid.latCenters, grid.lonCenters = latAll[lo:hi + 1][::-1].copy(), lonAll[colMin:colMax + 1].copy()
    grid._latSpace = latAll[lo:hi + 2][::-1] + latStep / 2
    grid._lonSpace = lonAll[colMin - 1:colMax + 1] + lonStep / 2
    grid.lat0, grid.lon0 = float(grid.latCenters[0]), float(grid.lonCenters[0])
    return grid


def scanline_window(latAxis, lonAxis, polygon):
    """(row0, col0, rows, cols): the cells of a frame that can lie in `polygon` — the corners inside the polygon's box, widened
    by one cell each way and clipped to the grid; all zero when no corner lies in the box.  `latAxis` (ny + 1), `lonAxis`
    (nx + 1): the corner axes in the polygon's coordinates."""
    def span(axis, lo, hi):
        at = np.flatnonzero((axis >= lo) & (axis <= hi))
        if at.size == 0:
            return 0, 0
        first, last = max(int(at[0]) - 1, 0), min(int(at[-1]) + 1, len(axis) - 1)      # corners
        return first, last - first                                                     # cells between them
    row0, rows = span(np.asarray(latAxis), polygon[:, 0].min(), polygon[:, 0].max())
    col0, cols = span(np.asarray(lonAxis), polygon[:, 1].min(), polygon[:, 1].max())
    return (row0, col0, rows, cols) if rows and cols else (0, 0, 0, 0)


def scanline_prepare(lonAxis, polygon, containsDiscontinuity):
    """The corner axes and the polygon as ``BaseMapping.maskedByPolygon`` prepares a resampled mapping's arrays for the point
    test: when the mapping or the polygon's box contains the discontinuity, both are shifted by 180 degrees (the same
    operations, on the 1-D longitude axis).  `lonAxis`: device tensor in the mapping's own longitudes.  Returns (lonAxis
    [device], polygon [host copy])."""
    import torch
    polygon = np.array(polygon, dtype=np.float64)
    if containsDiscontinuity or lons_contain_discontinuity(polygon[:, 1]):
        polygon[:, 1] = wrap_at_180(polygon[:, 1] + 180)
        lonAxis = torch.remainder(lonAxis + 360.0, 360.0) - 180.0           # wrap_at(lon + 180, 180)
    return lonAxis, polygon


def scanline_select(ctx, latAxis, lonAxis, polygon, mask, window):
    """``amt_scanline_select``: the keep bytes (rows, cols) [device uint8] of `window` and the stats [host int64 (5)]: the
    number of cells kept and their smallest / largest row and column in the frame."""
    import torch
    ny, nx = int(mask.shape[0]), int(mask.shape[1])
    row0, col0, rows, cols = window
    keep = ctx.empty((rows, cols), torch.uint8)
    stats = ctx.empty((5,), torch.int64)
    poly = ctx.to_device(np.ascontiguousarray(polygon, dtype=np.float64))
    ctx.call('amt_scanline_select', ptr(latAxis), ptr(lonAxis), ny, nx, ptr(poly), int(poly.shape[0]), ptr(mask), row0, col0, rows,
             cols, ptr(keep) if rows * cols else None, ptr(stats))
    return keep, to_host(stats)               # (the read-back waits for the kernel: `poly` may go)


def scanline_pack(ctx, keep, window, planes, img, img_dtype_code, nch, rowOffset, colOffset, count):
    """``amt_scanline_pack``: the records of the kept cells as device tensors (row, col int32 (count), planes (P, count), img
    (C, count)); `planes` (ny, nx, P), `img` (ny, nx, C)."""
    import torch
    ny, nx, nplane = (int(v) for v in planes.shape)
    row0, col0, rows, cols = window
    row, col = ctx.empty((count,), torch.int32), ctx.empty((count,), torch.int32)
    outPlanes = ctx.empty((nplane, count))
    outImg = ctx.empty((max(nch, 1), count), torch.uint8 if img_dtype_code != 2 else torch.int16)
    ctx.call('amt_scanline_pack', ptr(keep), row0, col0, rows, cols, ptr(planes), nplane, ptr(img) if nch else None,
             img_dtype_code or 1, nch, ny, nx, int(rowOffset), int(colOffset), int(count), ptr(row), ptr(col), ptr(outPlanes),
             ptr(outImg) if nch else None)
    return dict(row=row, col=col, planes=outPlanes, img=outImg, count=int(count))


def scanline_compose(ctx, strips, frames, nch, nplane, img_dtype_code, rowBase, colBase, NY, NX):
    """``amt_scanline_compose``: the union raster of `strips` (the dicts of :func:`scanline_pack`) with the ascending frame
    indices `frames`: device tensors planes (NY, NX, nplane), img (NY, NX, max(C, 1)), mask (NY, NX), frameIndex (NY, NX)."""
    import torch
    from ._native import ScanLineStrip
    table = (ScanLineStrip * len(strips))()
    for t, s, k in zip(table, strips, frames):
        some = s['count'] > 0
        t.row, t.col = (s['row'].data_ptr(), s['col'].data_ptr()) if some else (None, None)
        t.planes = s['planes'].data_ptr() if some and nplane else None
        t.img = s['img'].data_ptr() if some and nch else None
        t.count, t.frame = s['count'], int(k)
    planes = ctx.empty((NY, NX, nplane))
    img = ctx.zeros((NY, NX, max(nch, 1)), torch.uint8 if img_dtype_code != 2 else torch.int16)
    mask = ctx.empty((NY, NX), torch.uint8)
    frameIndex = ctx.empty((NY, NX), torch.int32)
    ctx.call('amt_scanline_compose', table, len(strips), img_dtype_code or 1, nch, nplane, int(rowBase), int(colBase), NY, NX,
             ptr(planes), ptr(img) if nch else None, ptr(mask), ptr(frameIndex))
    return planes, img, mask, frameIndex


def _scanline_frame(mapping, k, props, pxPerDeg, shifted):
    """Frame `k` of a scan-line sequence resampled on the sequence's lattice (device tensors), with what the strip pass needs:
    the corner axes (latitude on the device; longitude in the mapping's own longitudes, host and device) and the global origin"""
    fd = mapping.frame()
    res = resample_frame(fd, mapping.altitude, props.boundingBox, pxPerDeg, containsDiscontinuity=shifted, containsPole=False,
                         method='mean', keep_on_device=True)
    grid, ctx = res['grid'], fd.ctx
    lonOwn = wrap_at_180(grid._lonSpace + 180) if shifted else grid._lonSpace          # (as grid_coordinates does)
    res.update(ctx=ctx, frame=k, lat_axis_host=grid._latSpace, lon_own_host=lonOwn,
               lat_axis=ctx.to_device(np.ascontiguousarray(grid._latSpace)), lon_own=ctx.to_device(np.ascontiguousarray(lonOwn)),
               origin=scanline_global_origin(grid, pxPerDeg), nchan=fd.nchan, img_dtype_code=fd.img_dtype_code,
               img_dtype=fd.img_dtype if fd.nchan else None, identifier=mapping.identifier)
    return res


def _scanline_free_columns(res):
    """(first, last) column of `res` with an unmasked cell; ValueError when every cell is masked"""
    import torch
    cols = torch.nonzero((res['mask'] == 0).any(0)).reshape(-1)
    if cols.numel() == 0:
        raise ValueError('scan lines: frame {} ({!r}) has no valid cell'.format(res['frame'], res['identifier']))
    return int(cols[0].item()), int(cols[-1].item())


def scanline_first_cell_diagonal(res):
    """Metres between corners 0 and 2 of the first unmasked cell, row-major, of a resampled frame (what the reference reads
    from the first polygon of ``generatePolygonsFromMapping``, draw.py:701-704)."""
    import torch
    from .coordinates import geodesic
    free = (res['mask'].reshape(-1) == 0)
    first = int(torch.argmax(free.to(torch.uint8)).item())
    if not bool(free[first].item()):
        raise ValueError('scan lines: frame {} ({!r}) has no valid cell'.format(res['frame'], res['identifier']))
    r, c = divmod(first, int(res['mask'].shape[1]))
    lat, lon = res['lat_axis_host'], res['lon_own_host']
    return geodesic.distance(geodesic.Location(float(lat[r]), float(lon[c])), geodesic.Location(float(lat[r + 1]), float(lon[c + 1])))


def _scanline_strip_records(res, polygon):
    """The strip of a resampled frame: select, check, pack.  Returns (records, stats, line bounding box)."""
    ctx = res['ctx']
    cmin, cmax = _scanline_free_columns(res)
    own = res['lon_own_host'][cmin:cmax + 2]
    # the resampled mapping's containsDiscontinuity: the longitudes of its unmasked corners span more than 180 degrees
    lonAxis, poly = scanline_prepare(res['lon_own'], polygon, bool(own.max() - own.min() > 180))
    window = scanline_window(res['lat_axis_host'], lonAxis.cpu().numpy(), poly)
    keep, stats = scanline_select(ctx, res['lat_axis'], lonAxis.contiguous(), poly, res['mask'], window)
    count = int(stats[0])
    if count == 0:
        raise ValueError('The given mask would mask all pixels! (scan lines: the strip of frame {} ({!r}) keeps no cell)'
                         .format(res['frame'], res['identifier']))
    rowOffset, colOffset = res['origin']
    records = scanline_pack(ctx, keep, window, res['mean'], res['img'], res['img_dtype_code'], res['nchan'], rowOffset, colOffset,
                            count)
    lat, lon = res['lat_axis_host'], res['lon_own_host']
    box = BoundingBox(float(lat[stats[2] + 1]), float(lon[stats[3]]), float(lat[stats[1]]), float(lon[stats[4] + 1]))
    return records, stats, box


def resampleScanLines(mappings, arcsecPerPx=100, pxPerDeg=None, lineWidthFactor=1):
    """
    The scan-line map of a sequence as one raster (the reference's ``drawScanLinesCo``, auromat/draw.py:589-879, without the
    drawing): every mapping contributes the strip of its resampled cells through its centroid, perpendicular to the direction
    of flight of the centroids, and the strips of all mappings lie side by side on one plate carree grid — an overview of a
    whole pass in time and space.  Where strips overlap the later mapping's cells lie on top, as the reference draws them.

    The centroid of each mapping becomes the centre of its strip, so mask the mappings by elevation first.  All mappings are
    resampled (``method='mean'``) with ONE resolution, the first mapping's ``plateCarreeResolution`` for `arcsecPerPx` unless
    `pxPerDeg` is given, so that all grids are cut from one global lattice; and in ONE longitude frame: shifted by 180 degrees
    iff the first mapping's centroid has |lon| > 90 (date-line passes stay whole).  A cell belongs to a strip when it is
    valid and its four corners lie inside the strip's polygon (the rule of ``maskedByPolygon``; ``amt_scanline_select``);
    only the strips' cells are kept on the device (``amt_scanline_pack``) until they are put together
    (``amt_scanline_compose``).

    :param mappings: iterable of unresampled mappings, consumed once; one is held at a time
    :param number arcsecPerPx: spherical resolution of the resampling
    :param None|number|tuple pxPerDeg: (latPxPerDeg, lonPxPerDeg) or a number; has precedence over `arcsecPerPx`
    :param number lineWidthFactor: widens the strips relative to the width derived from the first two mappings; useful when
                                   mappings in between are missing
    :raises ValueError: fewer than two mappings; a mapping that does not fit the sequence's longitude frame (the sequence
                        spans its seam); a strip that keeps no cell or reaches a pole; mappings of different altitudes, image
                        types or channel counts.  A mapping with a pole in view raises what its ``centroid`` raises.
    :rtype: ScanLineMapping
    """
    from .mapping.mapping import ScanLineMapping
    short = ValueError('mapping sequence too short, need at least 2 mappings')
    it = iter(mappings)
    mapping = next(it, None)
    if mapping is None:
        raise short
    # values like the centroid come from the unresampled mapping (more accurate), as in the reference
    props = mapping.properties
    ppd = _px_per_deg(pxPerDeg) if pxPerDeg is not None else plateCarreeResolution(props.boundingBox, arcsecPerPx)
    shifted = scanline_longitude_frame(props.centroid)
    scanline_check_fits(props.boundingBox, shifted, 0, props.identifier)
    altitude, cameraPosGCRS, photoTime, metadata = mapping.altitude, mapping.cameraPosGCRS, mapping.photoTime, mapping.metadata
    cur = _scanline_frame(mapping, 0, props, ppd, shifted)
    rule = _ScanLineRule(props, scanline_first_cell_diagonal(cur), lineWidthFactor)
    per = dict(photoTimes=[], identifiers=[], centroids=[], azimuths=[], polygons=[], lineBoundingBoxes=[])
    strips, extents = [], []

    def finish(res, curProps, nextProps):
        polygon, az = rule.strip(curProps, nextProps)
        records, stats, box = _scanline_strip_records(res, polygon)
        strips.append(records)
        r0, c0 = res['origin']
        extents.append((r0 + stats[1], r0 + stats[2], c0 + stats[3], c0 + stats[4]))
        for name, value in (('photoTimes', curProps.photoTime), ('identifiers', curProps.identifier), ('centroids', curProps.centroid),
                            ('azimuths', az), ('polygons', polygon), ('lineBoundingBoxes', box)):
            per[name].append(value)

    k = 0
    for mapping in it:
        k += 1
        nextProps = mapping.properties
        fd = mapping.frame()
        if (mapping.altitude, fd.nchan, fd.img_dtype_code) != (altitude, cur['nchan'], cur['img_dtype_code']):
            raise ValueError('scan lines: frame {} ({!r}) differs from the first in altitude, image type or channel count'
                             .format(k, mapping.identifier))
        scanline_check_fits(nextProps.boundingBox, shifted, k, nextProps.identifier)
        finish(cur, props, nextProps)
        cur = _scanline_frame(mapping, k, nextProps, ppd, shifted)
        props = nextProps
        del mapping, fd
    if k == 0:
        raise short
    finish(cur, props, None)

    from .coordinates import geodesic
    ctx, nch, code = cur['ctx'], cur['nchan'], cur['img_dtype_code']
    ext = np.array(extents, dtype=np.int64)
    rowMin, rowMax, colMin, colMax = int(ext[:, 0].min()), int(ext[:, 1].max()), int(ext[:, 2].min()), int(ext[:, 3].max())
    union = scanline_union_grid(ppd, rowMin, rowMax, colMin, colMax)
    planes, img, mask, frameIndex = scanline_compose(ctx, strips, range(len(strips)), nch, nch + 1, code, rowMin, colMin, union.ny,
                                                     union.nx)
    out = _result(union, False, shifted, altitude, cur['has_elev'], dict(mean=planes, img=img, mask=mask), False,
                  cur['img_dtype'])
    image, elevation = _masked_image_and_elevation(out['mask'], out['mean'], out['img'], out['has_elev'])
    index = to_host(frameIndex, dtype=np.int32)
    maxHeight = max(geodesic.distance(b.topLeft, b.bottomRight) for b in per['lineBoundingBoxes'])
    return ScanLineMapping(out['lat'], out['lon'], out['lat_c'], out['lon_c'], elevation, altitude, image, cameraPosGCRS,
                           photoTime, '{}..{}'.format(per['identifiers'][0], per['identifiers'][-1]),
                           ma.masked_array(index, mask=index < 0), per['photoTimes'], per['identifiers'], per['centroids'],
                           per['azimuths'], per['polygons'], per['lineBoundingBoxes'], rule.width, rule.height, maxHeight, ppd,
                           metadata=metadata)


def resampleScanLinesMLatMLT(mappings, **kw):
    """
    :func:`resampleScanLines` in (MLat, SM longitude), the raster of the reference's ``drawScanLinesMLatMLTCo``
    (auromat/draw.py:858-879): every mapping goes through ``convertMappingToSM`` first.  The coordinate arrays, centroids,
    polygons and boxes of the result are magnetic (MLat, SM longitude: 180 degrees is magnetic midnight).

    See :func:`resampleScanLines` for parameters.
    """
    return resampleScanLines((convertMappingToSM(m) for m in mappings), **kw)


def fixedGrid(pxPerDeg, latMin, latMax, lonMin, lonMax):
    """
    Aligns the given bounding box to a fixed plate carree grid as defined by `pxPerDeg`
    (reference resample.py:281-299).

    :param lonMin,lonMax: must NOT contain the discontinuity
    """
    latPxPerDeg, lonPxPerDeg = pxPerDeg
    latSpaceAll = _global_axis(-90, 90, int(round(latPxPerDeg * 180 + 1)))
    lonSpaceAll = _global_axis(-180, 180, int(round(lonPxPerDeg * 360 + 1)))
    # np.argmax(axis > v) / np.argmax(axis >= v) of the reference, as binary searches on the sorted axis
    # (an all-False comparison gives index 0 there, i.e. the searchsorted result n wraps to 0)
    def first_gt(axis, v):
        i = int(np.searchsorted(axis, v, side='right'))
        return i if i < len(axis) else 0

    def first_ge(axis, v):
        i = int(np.searchsorted(axis, v, side='left'))
        return i if i < len(axis) else 0

    latMinInGrid = latSpaceAll[first_gt(latSpaceAll, latMin) - 1]
    latMaxInGrid = latSpaceAll[first_ge(latSpaceAll, latMax)]
    lonMinInGrid = lonSpaceAll[first_gt(lonSpaceAll, lonMin) - 1]
    lonMaxInGrid = lonSpaceAll[first_ge(lonSpaceAll, lonMax)]
    nLat = int(round(latPxPerDeg * (latMaxInGrid - latMinInGrid) + 1))
    nLon = int(round(lonPxPerDeg * (lonMaxInGrid - lonMinInGrid) + 1))
    return nLat, nLon, latMinInGrid, latMaxInGrid, lonMinInGrid, lonMaxInGrid


_GLOBAL_AXES = {}


def _global_axis(lo, hi, n):
    key = (lo, hi, n)
    if key not in _GLOBAL_AXES:
        if len(_GLOBAL_AXES) > 64:
            _GLOBAL_AXES.clear()
        _GLOBAL_AXES[key] = np.linspace(lo, hi, n)
    return _GLOBAL_AXES[key]


_GRID_CACHE = {}


def cached_grid(pxPerDeg, latMin, latMax, lonMin, lonMax):
    """
    The :class:`_Grid` for a bounding box.  Grids only depend on the global nodes the box is rounded out
    to, and consecutive frames of a sequence mostly round to the same nodes, so the arrays (and the device
    axis descriptors attached to them) are kept and re-used.
    """
    nodes = fixedGrid(pxPerDeg, latMin, latMax, lonMin, lonMax)
    key = (tuple(pxPerDeg),) + nodes
    g = _GRID_CACHE.get(key)
    if g is None:
        if len(_GRID_CACHE) > 512:
            _GRID_CACHE.clear()
        g = _GRID_CACHE[key] = _Grid(pxPerDeg, latMin, latMax, lonMin, lonMax, _nodes=nodes)
    return g


class _Grid(object):
    """Output grid of one resampling (reference resample.py:220-241,330-334)."""

    def __init__(self, pxPerDeg, latMin, latMax, lonMin, lonMax, _nodes=None):
        latPxPerDeg, lonPxPerDeg = pxPerDeg
        assert latPxPerDeg > 0 and lonPxPerDeg > 0
        nLat, nLon, latLo, latHi, lonLo, lonHi = _nodes or fixedGrid(pxPerDeg, latMin, latMax, lonMin, lonMax)
        self._axes = {}
        assert nLat > 1, 'nlat={}, latMax={}, latMin={}, pxperdeg={}'.format(nLat, latHi, latLo, pxPerDeg)
        assert nLon > 1, 'nlon={}, lonMax={}, lonMin={}, pxperdeg={}'.format(nLon, lonHi, lonLo, pxPerDeg)
        latSpaceCenter, latStep = np.linspace(latHi, latLo, num=nLat, retstep=True)
        lonSpaceCenter, lonStep = np.linspace(lonLo, lonHi, num=nLon, retstep=True)
        # first and last centre are dropped so that no corner lies outside the determined range
        latSpace = latSpaceCenter[:-1] + latStep / 2
        lonSpace = lonSpaceCenter[:-1] + lonStep / 2
        self.latCenters = latSpaceCenter[1:-1]
        self.lonCenters = lonSpaceCenter[1:-1]
        self.latStep, self.lonStep = latStep, lonStep
        self.lat0, self.lon0 = (float(self.latCenters[0]), float(self.lonCenters[0])) if nLat > 2 and nLon > 2 \
            else (np.nan, np.nan)
        self._latSpace, self._lonSpace = latSpace, lonSpace
        self._corner_grid = self._center_grid = None
        self.nx, self.ny = len(self.lonCenters), len(self.latCenters)
        # histogram ranges; latitude edges ascend, the output is flipped afterwards
        self.xrange = [self.lonCenters[0] - lonStep / 2, self.lonCenters[-1] + lonStep / 2]
        self.yrange = [self.latCenters[-1] + latStep / 2, self.latCenters[0] - latStep / 2]
        self.xedges = np.linspace(self.xrange[0], self.xrange[1], self.nx + 1)
        self.yedges = np.linspace(self.yrange[0], self.yrange[1], self.ny + 1)

    def axes(self, ctx):
        """(amt_axis x, amt_axis y) of this grid on `ctx`'s device (built once, kept alive with the grid)."""
        key = ctx.device.index
        if key not in self._axes:
            self._axes[key] = (make_axis(ctx, self.xedges, uniform=True), make_axis(ctx, self.yedges, uniform=True))
        (xaxis, _), (yaxis, _) = self._axes[key]
        return xaxis, yaxis

    def _settled(self, key, ctx, arrays):
        """Device tables of this grid under `key`: uploaded once and SETTLED before they are kept.  Grids are cached per process
        (cached_grid) and arrays of 1 MiB and more travel asynchronously on the uploading thread's stream (Context.upload), so a
        reader on another stream — another host thread — is ordered behind nothing: the uploading stream is waited for once,
        when the tables are made, which costs a sequence that finds them in the cache nothing."""
        import torch
        tables = self._axes.get(key)
        if tables is None:
            tables = tuple(ctx.to_device(a) for a in arrays())
            torch.cuda.current_stream(ctx.device).synchronize()
            tables = self._axes.setdefault(key, tables)
        return tables

    def device_corners(self, ctx):
        """(lat, lon) of the corner grid on the device, longitude-major ((nx+1, ny+1)), kept with the grid."""
        return self._settled(('corners', ctx.device.index), ctx,
                             lambda: (np.ascontiguousarray(self.lat.T, dtype=np.float64), np.ascontiguousarray(self.lon.T, dtype=np.float64)))

    def device_centers(self, ctx):
        """(latCenters (ny), lonCenters (nx)) on the device, kept with the grid."""
        return self._settled(('centers', ctx.device.index), ctx,
                             lambda: (np.ascontiguousarray(self.latCenters), np.ascontiguousarray(self.lonCenters)))

    # 2-D coordinate arrays of the output mapping (reference resample.py:239-241), built on first use
    def _corners(self):
        if self._corner_grid is None:
            self._corner_grid = np.dstack(np.meshgrid(self._latSpace, self._lonSpace)).T
        return self._corner_grid

    def _centers(self):
        if self._center_grid is None:
            self._center_grid = np.dstack(np.meshgrid(self.latCenters, self.lonCenters)).T
        return self._center_grid

    lat = property(lambda self: self._corners()[0])
    lon = property(lambda self: self._corners()[1])
    lat_c = property(lambda self: self._centers()[0])
    lon_c = property(lambda self: self._centers()[1])


def _rot_x(angle):
    return rotation_matrix(np.deg2rad(angle), [1, 0, 0])[:3, :3]


def _rotate_pole_dev(ctx, lat_deg, lon_deg, altitude, angle):
    """rotatePole (reference transform.py:301-322) on device tensors in degrees."""
    la, lo = lat_deg.reshape(-1), lon_deg.reshape(-1)
    if not la.is_contiguous():
        la = la.contiguous()
    if not lo.is_contiguous():
        lo = lo.contiguous()
    ola, olo = ctx.empty(la.shape), ctx.empty(lo.shape)
    ctx.call('amt_rotate_pole_deg', host9(_rot_x(angle)), ptr(la), ptr(lo), float(altitude), la.numel(), wgs84A, wgs84B,
             ptr(ola), ptr(olo))
    return ola.reshape(lat_deg.shape), olo.reshape(lon_deg.shape)


def _rotate_pole_host(lat_deg, lon_deg, altitude, angle):
    ctx = Context.current()
    la, lo = _rotate_pole_dev(ctx, ctx.to_device(np.ascontiguousarray(lat_deg)),
                              ctx.to_device(np.ascontiguousarray(lon_deg)), altitude, angle)
    return to_host(la), to_host(lo)


def wrap_at_180_t(t):
    """wrap_at_180 on a torch tensor (astropy Angle.wrap_at(180 deg): into [-180, 180))."""
    import torch
    a = t - torch.floor((t + 180.0) / 360.0) * 360.0
    a = torch.where(a >= 180.0, a - 360.0, a)
    return torch.where(a < -180.0, a + 360.0, a)


def _check_method(method):
    # (reference resample.py:353-360: NotImplementedError for 'median' and for anything it does not know)
    if method not in ('mean', 'nearest', 'linear', 'cubic'):
        raise NotImplementedError("method='%s' is not implemented (use 'mean', 'nearest', 'linear' or 'cubic')" % method)


CUBIC_TOLERANCE = 1e-6      # scipy.interpolate.CloughTocher2DInterpolator(tol=1e-6, maxiter=400): griddata's defaults
CUBIC_MAX_SWEEPS = 400

def cubic_exact(ctx, lat, lon, valid, values, height, width, grid, target_mask, method='cubic', vertices_out=None):
    """
    ``scipy.interpolate.griddata((lat, lon), values, grid centres, method='cubic' | 'linear')`` as the reference calls it
    (resample.py:315-326) on its own triangulation and in its own order: the Delaunay triangulation of the valid pixel centres
    (``amt_delaunay_create``, host: equal to Qhull's wherever that is unique); for 'cubic' scipy's Gauss-Seidel gradient
    estimator over its edges in the order of the points (``amt_cubic_gradients_csr``: tolerance 1e-6, at most 400 sweeps, every
    channel with its own stopping sweep) and the Clough-Tocher element in the triangle of every grid centre
    (``amt_delaunay_locate`` + ``amt_cubic_eval``); for 'linear' the barycentric sum over that triangle's vertices.
    `vertices_out`: a list that receives the (ny * nx, 3) int64 device tensor of each grid centre's triangle as flat pixel
    indices (-1: none).

    :param lat, lon: flat float64 device tensors (height * width) in the coordinates the grid is laid out in
    :param valid: flat bool device tensor: the pixel is a data point
    :param values: (height * width, channels) float64 device tensor
    :param target_mask: (ny, nx) uint8 device tensor, non-zero = the grid centre is not wanted (outside the outline), or None
    :return: ((ny * nx, channels) float64 device tensor, NaN outside the convex hull and where masked; sweeps per channel)
    """
    import os
    import time
    import torch
    from ._native import lib
    L = lib()
    debug = bool(os.environ.get('AMT_CUBIC_DEBUG'))
    marks = []

    def mark(what):
        if debug:
            torch.cuda.synchronize()
            marks.append((what, time.perf_counter()))
    mark('start')
    idx = torch.nonzero(valid.reshape(-1)).reshape(-1)               # row-major pixel order = the reference's point order
    n, nchan = int(idx.numel()), int(values.shape[1])
    out = torch.full((grid.ny * grid.nx, nchan), float('nan'), dtype=torch.float64, device=ctx.device)
    if n < 3:
        raise ValueError("method='%s' needs at least three valid pixels" % method)
    xy = torch.stack((lat.reshape(-1)[idx], lon.reshape(-1)[idx]), dim=1).contiguous()
    xy_host = np.ascontiguousarray(to_host(xy))
    handle = C.c_void_p()
    mark('points to the host')
    rc = L.amt_delaunay_create(xy_host.ctypes.data_as(C.c_void_p), n, C.byref(handle))
    if rc == -3:                                                     # AMT_ENOMEM
        raise MemoryError("method='%s': no memory for the triangulation of %d pixel centres" % (method, n))
    if rc != 0:
        raise ValueError("method='%s': the valid pixel centres cannot be triangulated (all collinear, or a coordinate that is "
                         "not finite)" % method)
    mark('triangulation')
    try:
        if method != 'linear':
            # the vertices' neighbour lists (scipy.spatial.Delaunay.vertex_neighbor_vertices, every list in increasing order), made
            # ON THE DEVICE from the build's own triangle slots (amt_delaunay_slots: no compaction, no list building, no 190 MB of
            # lists over the link — the host spent 0.2 s on those): every finite triangle gives the directed edges v1 -> v2,
            # v2 -> v0, v0 -> v1; an inner edge comes up once in each direction (from its two triangles), a hull edge once and
            # gets its reverse here; sorted by (source, target) they are the CSR the relaxation walks
            d_indptr, d_indices = device_vertex_lists(ctx, L, handle, n)
            rows = torch.div(idx, int(width), rounding_mode='floor')
            row_start = torch.zeros(int(height) + 1, dtype=torch.int64, device=ctx.device)
            row_start[1:] = torch.cumsum(torch.bincount(rows, minlength=int(height)), 0)
            mark('neighbour lists on the device')
        # the grid centres that are wanted, in row-major order (the walk from one to the next is a step or two)
        wanted = np.ones((grid.ny, grid.nx), dtype=bool) if target_mask is None else ~to_host(target_mask).astype(bool)
        sel = np.flatnonzero(wanted.ravel())
        m = int(sel.size)
        if m:
            iy, ix = np.divmod(sel, grid.nx)
            targets = np.ascontiguousarray(np.column_stack((np.asarray(grid.latCenters)[iy], np.asarray(grid.lonCenters)[ix])))
            vertices = np.empty((m, 3), dtype=np.int32)
            centroids = np.empty((m, 3, 2), dtype=np.float64)
            has_nb = np.empty((m, 3), dtype=np.uint8)
            rc = L.amt_delaunay_locate(handle, targets.ctypes.data_as(C.c_void_p), m, vertices.ctypes.data_as(C.c_void_p),
                                       centroids.ctypes.data_as(C.c_void_p), has_nb.ctypes.data_as(C.c_void_p))
            assert rc == 0
            d_t, d_v, d_c, d_h = (ctx.to_device(a, a.dtype) for a in (targets, vertices, centroids, has_nb))
            d_sel = ctx.to_device(sel.astype(np.int64), np.int64)
        mark('point location')
        if vertices_out is not None:
            tri_px = torch.full((grid.ny * grid.nx, 3), -1, dtype=torch.int64, device=ctx.device)
            if m:
                v64 = d_v.to(torch.int64)
                tri_px[d_sel] = torch.where(v64 >= 0, idx[v64.clamp(min=0)], v64)
            vertices_out.append(tri_px)
        sweeps_all = []
        if method == 'linear':
            if m:
                # scipy's LinearNDInterpolator: the barycentric sum over the triangle's vertices
                inside = d_v[:, 0] >= 0
                v64 = d_v.to(torch.int64).clamp(min=0)
                x, y = xy[:, 0][v64], xy[:, 1][v64]                       # (m, 3)
                px, py = d_t[:, 0], d_t[:, 1]
                det = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
                w1 = ((px - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (py - y[:, 0])) / det
                w2 = ((x[:, 1] - x[:, 0]) * (py - y[:, 0]) - (px - x[:, 0]) * (y[:, 1] - y[:, 0])) / det
                wts = torch.stack((1.0 - w1 - w2, w1, w2), dim=1)
                part = (wts[:, :, None] * values[idx][v64]).sum(dim=1)
                part[~inside] = float('nan')
                out[d_sel] = part
            return out, sweeps_all
        for c0 in range(0, nchan, 32):                      # (the relaxation kernel takes up to 63 channels, one per lane)
            vals = values[idx][:, c0:c0 + 32].contiguous()
            k = int(vals.shape[1])
            grad = ctx.empty((n, k, 2))
            sweeps = (C.c_int32 * k)()
            ctx.call('amt_cubic_gradients_csr', ptr(xy), n, ptr(d_indptr), ptr(d_indices), ptr(row_start), int(height), ptr(vals),
                     k, CUBIC_TOLERANCE, CUBIC_MAX_SWEEPS, ptr(grad), sweeps)
            sweeps_all.extend(int(v) for v in sweeps)
            mark('relaxation (%d sweeps)' % max(sweeps))
            if m:
                part = ctx.empty((m, k))
                ctx.call('amt_cubic_eval', m, ptr(d_t), ptr(d_v), ptr(d_c), ptr(d_h), ptr(xy), ptr(vals), ptr(grad), k, ptr(part))
                out[d_sel, c0:c0 + k] = part
        mark('element')
    finally:
        mark('values')
        # (giving back the triangulation's ~0.6 GB of host memory takes 40 ms: on a thread of its own — the call holds no lock of
        # the interpreter —, beside whatever the caller does next)
        import threading
        threading.Thread(target=L.amt_delaunay_destroy, args=(handle,), daemon=True).start()
        mark('triangulation handed back')
        if debug:
            print('cubic_exact: ' + ', '.join('%s %.3f s' % (b[0], b[1] - a[1]) for a, b in zip(marks, marks[1:])))
    return out, sweeps_all


def device_vertex_lists(ctx, L, handle, n):
    """(indptr (n + 1) int64, indices int32) on the device: the vertex neighbour lists of a triangulation made by
    amt_delaunay_create*, equal to amt_delaunay_vertex_neighbours' (tests/test_gpu_nearest.py)."""
    import torch
    pv, pd, ns = C.c_void_p(), C.c_void_p(), C.c_int64()
    rc = L.amt_delaunay_slots(handle, C.byref(pv), C.byref(pd), C.byref(ns))
    assert rc == 0 and ns.value > 0, rc
    slots = int(ns.value)
    v_host = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_int32)), shape=(slots, 3))
    dead_host = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_uint8)), shape=(slots,))
    v = ctx.to_device(v_host, np.int32)
    dead = ctx.to_device(dead_host, np.uint8)
    tri = v[(dead == 0) & (v >= 0).all(dim=1)].to(torch.int64)            # finite triangles (a ghost carries -1)
    del v, dead
    src = torch.cat((tri[:, 1], tri[:, 2], tri[:, 0]))
    dst = torch.cat((tri[:, 2], tri[:, 0], tri[:, 1]))
    del tri
    key = torch.sort((src << 32) | dst).values
    rev = (dst << 32) | src
    del src, dst
    at = torch.searchsorted(key, rev).clamp(max=key.numel() - 1)
    hull = rev[key[at] != rev]                                             # reverses that no triangle supplies: hull edges
    del at, rev
    if hull.numel():
        key = torch.sort(torch.cat((key, hull))).values
    source = key >> 32
    indices = (key & 0xffffffff).to(torch.int32)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=ctx.device)
    indptr[1:] = torch.cumsum(torch.bincount(source, minlength=n), 0)
    return indptr, indices.contiguous()


def outside_outline_mask(ctx, grid, outline):
    """
    (ny, nx) uint8 device mask of the grid cells with a corner outside the outline polygon (reference
    resample.py:246-259: pointsInsidePolygon of the corner grid, a cell is masked if any of its 4 corners is outside).

    :param outline: (n,2) [lat,lon] polygon in the coordinates of the grid (rotated / shifted like the data)
    """
    import torch
    poly = ctx.to_device(np.ascontiguousarray(outline, dtype=np.float64))
    # points in longitude-major order: consecutive points share their y (= longitude), which lets the kernel drop
    # almost every polygon edge per block of points (it skips edges whose y-range misses the block's)
    lat, lon = grid.device_corners(ctx)
    inside = ctx.empty(tuple(lat.shape), torch.uint8)
    ctx.call('amt_points_in_polygon', ptr(lat), ptr(lon), lat.numel(), ptr(poly), int(poly.shape[0]), ptr(inside))
    out = inside.T == 0
    return (out[:-1, :-1] | out[1:, :-1] | out[:-1, 1:] | out[1:, 1:]).to(torch.uint8).contiguous()


def nearest_indices(ctx, lat_c, lon_c, elev, center_mask, height, width, min_elevation, grid, lon_wrap, target_mask):
    """(ny, nx) int64 device tensor: flat index of the pixel centre nearest to every grid centre, -1 = none / masked
    (``amt_nearest_frame``; reference resample.py:323-327, griddata(method='nearest'))."""
    import torch
    xaxis, yaxis = grid.axes(ctx)
    tlat, tlon = grid.device_centers(ctx)
    index = ctx.empty((grid.ny, grid.nx), torch.int64)
    ctx.call('amt_nearest_frame', ptr(lat_c), ptr(lon_c), ptr(elev), ptr(center_mask), height, width,
             _min_elevation(min_elevation), C.byref(xaxis), C.byref(yaxis), lon_wrap, ptr(tlat), ptr(tlon), ptr(target_mask), ptr(index))
    return index


def _frame_grid(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity, containsPole, min_elevation, outline, shard):
    """The output grid of a device-resident frame and the centre coordinates to bin (reference resample.py:159-241):
    ``(grid, lat_c, lon_c, lon_wrap)``, the pole rotated out of the data or the longitudes out of the date line."""
    import torch
    ctx = fd.ctx
    latMin, latMax = boundingBox.latSouth, boundingBox.latNorth
    lonMin, lonMax = boundingBox.lonWest, boundingBox.lonEast
    lat_c, lon_c = fd.lat_c, fd.lon_c
    lon_wrap = 0
    if containsPole:
        # rotate the pole out of the data by +90 deg about x (reference resample.py:176-201)
        if outline is not None:
            # as the reference: the extent of the rotated outline
            ola, olo = _rotate_pole_host(np.asarray(outline, dtype=np.float64)[:, 0],
                                         np.asarray(outline, dtype=np.float64)[:, 1], altitude, 90)
            latMin, latMax, lonMin, lonMax = ola.min(), ola.max(), olo.min(), olo.max()
        else:
            # (no outline at hand — the frame pipeline: all unmasked corners, the same unless the mask has islands)
            rla, rlo = _rotate_pole_dev(ctx, fd.lat, fd.lon, altitude, 90)
            corner, cmask = fd.corner_mask_tensor(), fd.center_mask_tensor()
            if min_elevation is not None and fd.elev is not None:
                # maskedByElevation(min_elevation) is fused into the binning pass below; the box is that of the corners
                # which survive it (mapping.py:845-864 + the lazy sanitisation, 1161-1213)
                cmask = (cmask.bool() | ~(fd.elev >= float(min_elevation))).to(torch.uint8)
                corner = corner.clone()
                ctx.call('amt_sanitize_masks', ptr(corner), ptr(cmask), None, fd.height, fd.width, 1)
            red = ctx.empty((8,))
            ctx.call('amt_bbox_corners', ptr(rla), ptr(rlo), ptr(corner), ptr(cmask), fd.height, fd.width, ptr(red))
            r = to_host(red)
            if shard is not None:
                r = shard.box(r)
            latMin, latMax, lonMin, lonMax = r[0], r[1], r[2], r[3]
        lat_c, lon_c = _rotate_pole_dev(ctx, fd.lat_c, fd.lon_c, altitude, 90)
    elif containsDiscontinuity:
        # rotate longitudes out of the 180 deg discontinuity (reference resample.py:203-218); the outline's
        # extremes are the box's west/east edge, and the wrap is monotonic on each side
        lonMin, lonMax = wrap_at_180(lonMin + 180), wrap_at_180(lonMax + 180)
        lon_wrap = 1

    return cached_grid(pxPerDeg, latMin, latMax, lonMin, lonMax), lat_c, lon_c, lon_wrap


def resample_frame(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity=False, containsPole=False,
                   min_elevation=None, keep_on_device=False, method='mean', outline=None, shard=None):
    """
    ``_resample`` + ``_resampleCenterData(method='mean')`` + the image finalisation of ``resample``
    (reference resample.py:119-136,159-279,301-351) on a device-resident frame.

    :param FrameData fd: centre lat/lon, elevation (optional), image and masks in HBM
    :param min_elevation: fuse ``maskedByElevation(min_elevation)`` into the binning pass (the frame's
                          own centre mask is applied in addition)
    :param method: 'mean' (binning: :func:`_bin_mean_frame`) or 'nearest', 'linear', 'cubic' (interpolation between the pixel
                   centres: :func:`_interpolate_frame`; needs `outline`)
    :param outline: (n,2) [lat,lon] polygon of the mapping (``BaseMapping.outline``) for the interpolating methods:
                    grid cells with a corner outside it are masked (reference resample.py:246-259)
    :param shard: `fd` holds a band of rows of a frame whose other bands are on other ranks (see
                  :func:`auromat_amd.sequence.resample_frame_sharded`): shard.box combines the reduction of the rotated
                  corners, shard.acc sums the integer accumulators over the ranks before the means are taken
    :param keep_on_device: the arrays stay device tensors and no grid coordinates are computed (sequence mode, :func:`_result`)
    :return: dict(lat, lon, lat_c, lon_c [grid coordinates, host], mean (ny,nx,C+1), img (ny,nx,C),
                  mask (ny,nx), count (ny,nx) ['mean' only], has_elev); 'nearest': also index (ny,nx), 'linear' and 'cubic':
                  triangles (ny,nx,3), 'cubic': sweeps
    """
    _check_method(method)
    grid, lat_c, lon_c, lon_wrap = _frame_grid(fd, altitude, boundingBox, pxPerDeg, containsDiscontinuity, containsPole,
                                               min_elevation, outline, shard)
    axes = grid.axes(fd.ctx)
    if method == 'mean':
        tensors = _bin_mean_frame(fd, grid, axes, lat_c, lon_c, lon_wrap, min_elevation, shard)
    else:
        tensors = _interpolate_frame(fd, grid, lat_c, lon_c, lon_wrap, altitude, containsDiscontinuity, containsPole,
                                     min_elevation, method, outline, shard)
    return _result(grid, bool(containsPole), bool(containsDiscontinuity), altitude, fd.elev is not None, tensors,
                   keep_on_device, fd.img_dtype if fd.nchan else None)


def _bin_mean_frame(fd, grid, axes, lat_c, lon_c, lon_wrap, min_elevation, shard):
    """method='mean' of :func:`resample_frame` on the grid and centre coordinates of :func:`_frame_grid`: integer accumulation
    (``amt_bin_frame``), the sum over the ranks of a sharded frame, means and image (``amt_bin_frame_finalize``).  Returns the
    device tensors mean, img, mask, count."""
    import torch
    ctx = fd.ctx
    xaxis, yaxis = axes
    nch = fd.nchan
    acc = ctx.zeros((nch + 2, grid.nx * grid.ny), torch.int64)
    ctx.call('amt_bin_frame', ptr(lat_c), ptr(lon_c), ptr(fd.elev), ptr(fd.img), fd.img_dtype_code, nch,
             ptr(fd.center_mask), fd.height, fd.width, _min_elevation(min_elevation), C.byref(xaxis), C.byref(yaxis), lon_wrap,
             ptr(acc))
    if shard is not None:
        shard.acc(acc)          # integer counts and sums: the order of the ranks does not matter
    mean, img, mask, count = _bin_outputs(ctx, grid, nch, fd.img_dtype_code)
    ctx.call('amt_bin_frame_finalize', ptr(acc), grid.nx, grid.ny, nch, fd.img_dtype_code or 1, ptr(mean),
             ptr(img) if nch else None, ptr(mask), ptr(count))
    return dict(mean=mean, img=img, mask=mask, count=count)


def _interpolate_frame(fd, grid, lat_c, lon_c, lon_wrap, altitude, containsDiscontinuity, containsPole, min_elevation, method,
                       outline, shard):
    """method='nearest', 'linear' and 'cubic' of :func:`resample_frame` on the grid and centre coordinates of
    :func:`_frame_grid`.  Returns the device tensors mean, img, mask and index ('nearest') or triangles ('linear', 'cubic';
    'cubic' also the number ``sweeps``)."""
    import torch
    ctx = fd.ctx
    nch = fd.nchan
    assert outline is not None, "method='%s' needs the outline of the mapping" % method
    assert shard is None, "rows of one frame over several ranks: method='mean' only"
    outline = np.array(outline, dtype=np.float64)
    if containsPole:
        outline[:, 0], outline[:, 1] = _rotate_pole_host(outline[:, 0], outline[:, 1], altitude, 90)
    elif containsDiscontinuity:
        outline[:, 1] = wrap_at_180(outline[:, 1] + 180)
    target_mask = outside_outline_mask(ctx, grid, outline)
    mean, img, mask, _ = _bin_outputs(ctx, grid, nch, fd.img_dtype_code, count=False)
    if method == 'nearest':
        index = nearest_indices(ctx, lat_c, lon_c, fd.elev, fd.center_mask, fd.height, fd.width, min_elevation, grid,
                                lon_wrap, target_mask)
        ctx.call('amt_nearest_gather', ptr(index), grid.nx * grid.ny, ptr(fd.img), fd.img_dtype_code or 1, nch,
                 ptr(fd.elev), ptr(mean), ptr(img) if nch else None, ptr(mask))
        return dict(mean=mean, img=img, mask=mask, index=index)
    tri = ctx.empty((grid.ny, grid.nx, 3), torch.int64)
    # scipy's griddata(method='linear' | 'cubic') on its own triangulation, in its own order (cubic_exact): image
    # channels and elevation as float64 channels of the valid pixels, then numpy's rounding and cast of the image
    assert fd.elev is not None, "method='%s' on a frame needs the elevation" % method
    la, lo = lat_c.reshape(-1), lon_c.reshape(-1)
    if lon_wrap:
        lo = wrap_at_180_t(lo + 180)
    valid = ~(torch.isnan(la) | torch.isnan(lo)) & (fd.elev.reshape(-1) >= _min_elevation(min_elevation))
    if fd.center_mask is not None:
        valid &= fd.center_mask.reshape(-1) == 0
    chans = [fd.elev.reshape(-1, 1)]
    if nch:
        pix = fd.img.reshape(-1, nch)
        if fd.img_dtype_code == 2:
            pix = pix.to(torch.int32) & 0xffff            # uint16 bits kept as int16
        chans.insert(0, pix.to(torch.float64))
    tri_out = []
    vals, sweeps = cubic_exact(ctx, la, lo, valid, torch.cat(chans, dim=1), fd.height, fd.width, grid, target_mask,
                               method=method, vertices_out=tri_out)
    mean.copy_(vals.reshape(grid.ny, grid.nx, nch + 1))
    empty = torch.isnan(mean[..., 0])
    mask.copy_(empty.to(torch.uint8))
    if nch:
        # np.round + astype of the interpolated floats (reference resample.py:128-136); an overshoot wraps
        rounded = torch.round(torch.nan_to_num(mean[..., :nch], nan=0.0)).to(torch.int64)
        if fd.img_dtype_code == 2:
            img.copy_((rounded & 0xffff).to(torch.int32).to(torch.int16))
        else:
            img.copy_((rounded & 0xff).to(torch.uint8))
    tri.copy_(tri_out[0].reshape(grid.ny, grid.nx, 3))
    out = dict(mean=mean, img=img, mask=mask, triangles=tri)
    if method == 'cubic':
        out['sweeps'] = max(sweeps)
    return out


def grid_coordinates(res):
    """Corner / centre coordinate arrays of a resample_frame result (reference resample.py:239-241,261-277)."""
    grid = res['grid']
    lat, lon, lat_gc, lon_gc = grid.lat, grid.lon, grid.lat_c, grid.lon_c
    if res['contains_pole']:
        lat, lon = _rotate_pole_host(lat, lon, res['altitude'], -90)            # reference resample.py:262-273
        lat_gc, lon_gc = _rotate_pole_host(lat_gc, lon_gc, res['altitude'], -90)
    elif res['contains_discontinuity']:
        lon = wrap_at_180(lon + 180)                                             # reference resample.py:274-277
        lon_gc = wrap_at_180(lon_gc + 180)
    return dict(lat=lat, lon=lon, lat_c=lat_gc, lon_c=lon_gc)


def _resample(latsCenter, lonsCenter, altitude, data, outlineLatLonFn, boundingBox, pxPerDeg,
              containsDiscontinuity=False, containsPole=False, method='mean'):
    """
    Array-level resampling with the reference's signature (resample.py:159-279): every channel of
    `data` (float, NaN = missing) is binned on its own.

    :param latsCenter, lonsCenter: (h,w), NaN = not mapped
    :param data: float data for each pixel center, (h,w,n) with n>0, or (h,w)
    :param outlineLatLonFn: callable returning (n,2) [lat,lon] points whose min/max bound the data
                            (only used in the pole / discontinuity branches)
    :param pxPerDeg: tuple (latPxPerDeg, lonPxPerDeg)
    :rtype: tuple (lat, lon, latCenter, lonCenter, data)
    """
    _check_method(method)
    ctx = Context.current()
    latMin, latMax = boundingBox.latSouth, boundingBox.latNorth
    lonMin, lonMax = boundingBox.lonWest, boundingBox.lonEast
    lat_c = ctx.to_device(np.asarray(latsCenter, dtype=np.float64))
    lon_c = ctx.to_device(np.asarray(lonsCenter, dtype=np.float64))
    lon_wrap = 0
    outline = None
    if containsPole:
        outline = np.array(outlineLatLonFn(), dtype=np.float64)
        outline[:, 0], outline[:, 1] = _rotate_pole_host(outline[:, 0], outline[:, 1], altitude, 90)
        latMin, latMax, lonMin, lonMax = np.min(outline[:, 0]), np.max(outline[:, 0]), np.min(outline[:, 1]), \
            np.max(outline[:, 1])
        lat_c, lon_c = _rotate_pole_dev(ctx, lat_c, lon_c, altitude, 90)
    elif containsDiscontinuity:
        outline = np.array(outlineLatLonFn(), dtype=np.float64)
        outline[:, 1] = wrap_at_180(outline[:, 1] + 180)
        lonMin, lonMax = np.min(outline[:, 1]), np.max(outline[:, 1])
        lon_wrap = 1
    grid = _Grid(pxPerDeg, latMin, latMax, lonMin, lonMax)
    scalar = np.ndim(data) == 2
    d = np.asarray(data, dtype=np.float64)
    if scalar:
        d = d[..., None]
    if method == 'mean':
        mean = _resampleCenterData(lat_c, lon_c, d, grid, lon_wrap)
    else:
        # nearest pixel centre for every grid centre, then everything outside the outline is masked
        # (reference resample.py:246-259,323-327; the reference rotates / shifts the outline in place, :176-218)
        import torch
        if outline is None:
            outline = np.array(outlineLatLonFn(), dtype=np.float64)
        target_mask = outside_outline_mask(ctx, grid, outline)
        h, w = d.shape[:2]
        flat = ctx.to_device(np.ascontiguousarray(d.reshape(h * w, d.shape[2])))
        if method == 'nearest':
            index = nearest_indices(ctx, lat_c.reshape(-1), lon_c.reshape(-1), None, None, h, w, None, grid, lon_wrap,
                                    target_mask)
            picked = flat[index.clamp(min=0).reshape(-1)]
            picked[index.reshape(-1) < 0] = float('nan')
        elif method == 'cubic':
            # scipy's griddata on its own triangulation, in its own order (cubic_exact); the data points are the pixels with
            # a latitude (reference resample.py:315-321)
            la, lo = lat_c.reshape(-1).contiguous(), lon_c.reshape(-1).contiguous()
            if lon_wrap:
                lo = wrap_at_180_t(lo + 180)
            picked, _ = cubic_exact(ctx, la, lo, ~(torch.isnan(la) | torch.isnan(lo)), flat, h, w, grid, target_mask)
        else:
            # scipy's griddata(method='linear') on its own triangulation (cubic_exact): Qhull's triangle of every grid centre,
            # the barycentric sum of the channels
            la, lo = lat_c.reshape(-1).contiguous(), lon_c.reshape(-1).contiguous()
            if lon_wrap:
                lo = wrap_at_180_t(lo + 180)
            picked, _ = cubic_exact(ctx, la, lo, ~(torch.isnan(la) | torch.isnan(lo)), flat, h, w, grid, target_mask, method='linear')
        mean = to_host(picked.reshape(grid.ny, grid.nx, d.shape[2]))
    coords = grid_coordinates(dict(grid=grid, contains_pole=containsPole, contains_discontinuity=containsDiscontinuity,
                                   altitude=altitude))
    if scalar:
        mean = mean.reshape(mean.shape[0], mean.shape[1])
    return coords['lat'], coords['lon'], coords['lat_c'], coords['lon_c'], mean


def _resampleCenterData(lat_c, lon_c, centerData, grid, lon_wrap):
    """Binned mean of float channels (reference resample.py:301-368, method='mean')."""
    ctx = Context.current()
    n = lat_c.numel()
    nchan = centerData.shape[2]
    assert nchan <= 8, 'at most 8 channels per call'
    chans = [ctx.to_device(np.ascontiguousarray(centerData[:, :, k])) for k in range(nchan)]
    xaxis, xkeep = make_axis(ctx, grid.xedges, uniform=True)
    yaxis, ykeep = make_axis(ctx, grid.yedges, uniform=True)
    count = ctx.zeros((grid.nx * grid.ny,))
    sums = [ctx.zeros((grid.nx * grid.ny,)) for _ in range(nchan)]
    wptr = (C.c_void_p * nchan)(*[t.data_ptr() for t in chans])
    sptr = (C.c_void_p * nchan)(*[t.data_ptr() for t in sums])
    # pixels without coordinates are outliers of the histogram (NaN latitude, resample.py:315-321)
    ctx.call('amt_hist2d_accumulate', ptr(lon_c.reshape(-1)), ptr(lat_c.reshape(-1)), n, wptr, nchan,
             C.byref(xaxis), C.byref(yaxis), lon_wrap, ptr(count), sptr)
    mean = ctx.empty((grid.ny, grid.nx, nchan))
    ctx.call('amt_hist2d_finalize_mean', ptr(count), sptr, nchan, grid.nx, grid.ny, ptr(mean))
    return to_host(mean)


def ResampleProvider(provider, **kw):
    """
    Wrap the given mapping provider by resampling every returned mapping (reference resample.py:370-394).

    See :func:`resample` for parameters.
    """
    resampleFn = partial(resample, **kw)

    class ResamplingProvider(provider.__class__):
        def get(self, *a, **k):
            return resampleFn(super(ResamplingProvider, self).get(*a, **k))

        def getById(self, *a, **k):
            return resampleFn(super(ResamplingProvider, self).getById(*a, **k))

        def getSequence(self, *a, **k):
            return map(resampleFn, super(ResamplingProvider, self).getSequence(*a, **k))

    wrapped = copy.copy(provider)
    wrapped.__class__ = ResamplingProvider
    return wrapped


# ---- gather resampling: every grid cell centre projected into the image ---------------------------------------------------------
GATHER_INTERPOLATIONS = ('nearest', 'linear', 'lanczos4')


class ThreadPipes(threading.local):
    """A cache of frame pipelines of the calling thread (`pipes`: key -> FramePipeline, at most 4).  A pipeline is one amt_ctx,
    one amt_pipe, one set of accumulators and one stored layout, and "contexts may be used from different threads (one thread
    per context at a time)" (include/auromat_hip.h): like Context._cache, the pipeline caches of the class paths are kept per
    host thread, so that two threads that resample mappings of one frame size never drive one pipeline."""

    def __init__(self):
        self.pipes = {}

    def get(self, key, make):
        pipe = self.pipes.get(key)
        if pipe is None:
            if len(self.pipes) >= 4:
                self.pipes.clear()              # (frames of many sizes: do not hoard their buffers)
            pipe = self.pipes[key] = make()
        return pipe


_GATHER_PIPES = ThreadPipes()


def _check_gather_interpolation(interpolation):
    if interpolation not in GATHER_INTERPOLATIONS:
        raise ValueError('interpolation must be one of %s, not %r' % (', '.join(GATHER_INTERPOLATIONS), interpolation))


SUPERSAMPLE_MAX = 8


def supersample_min_count(minCoverage, n):
    """The least number of seen sub-samples of a valid cell of a gathering with `n` x `n` sub-samples per cell:
    ``max(1, ceil(minCoverage * n * n))``; None means 0.5, as in :func:`resampleArea`."""
    if minCoverage is None:
        minCoverage = 0.5
    return max(1, int(math.ceil(minCoverage * n * n)))


def _check_supersample(supersample, minCoverage):
    """ValueError for a `supersample` that is not an int in 1 ... 8 (a bool is none), then for a `minCoverage` outside (0, 1],
    then for a `minCoverage` given with ``supersample == 1``; returns (n, min_count), min_count None for n = 1."""
    if isinstance(supersample, bool) or not isinstance(supersample, (int, np.integer)) or not 1 <= supersample <= SUPERSAMPLE_MAX:
        raise ValueError('supersample must be an int in 1 ... %d, but is: %r' % (SUPERSAMPLE_MAX, supersample))
    n = int(supersample)
    if minCoverage is not None:
        try:
            v = float(minCoverage)
        except (TypeError, ValueError):
            raise ValueError('minCoverage must be a number in (0, 1], but is: {!r}'.format(minCoverage))
        if not 0.0 < v <= 1.0:
            raise ValueError('minCoverage must be in the range (0, 1], got {!r}'.format(minCoverage))
        if n == 1:
            raise ValueError('minCoverage={!r} goes with supersample > 1: one point is sampled per cell'.format(minCoverage))
        minCoverage = v
    return n, (None if n == 1 else supersample_min_count(minCoverage, n))


def _subsample_axis(corners, n):
    """n sub-sample positions per cell of an axis given by its cells' corners: corner + step * (2 s + 1) / (2 n)"""
    c = np.asarray(corners, dtype=np.float64)
    f = (2 * np.arange(n) + 1) / (2 * n)
    return (c[:-1, None] + (c[1:, None] - c[:-1, None]) * f[None, :]).reshape(-1)


def gather_subsample_coordinates(plan, n):
    """
    Where a gathering with `n` x `n` sub-samples per cell samples: the sub-samples split every cell of the plan's grid
    (:func:`gather_plan` or :func:`gather_mosaic_plan`) into n x n equal parts and sit at the parts' centres — with
    ``c = grid.lat[:, 0]`` the latitude of sub-sample s of row i is ``c[i] + (c[i + 1] - c[i]) * ((2 s + 1) / (2 n))``, the
    longitudes likewise from ``grid.lon[0, :]``.  With the date line in the grid the longitudes are shifted the way
    :func:`grid_coordinates` shifts the centres; with a pole the fine mesh of the rotated grid is rotated back.

    :return: dict(lat (ny n), lon (nx n), cell_lat, cell_lon): the axes form with cell_lat = cell_lon = None, or, with a pole,
             the point form — cell_lat, cell_lon of (ny n, nx n) — with lat = lon = None; the two forms of
             ``amt_gather_mosaic_supersampled``
    """
    a, b, points = _gather_job_coordinates(plan, n, True)
    return dict(lat=None, lon=None, cell_lat=a, cell_lon=b) if points else dict(lat=a, lon=b, cell_lat=None, cell_lon=None)


def _gather_job_coordinates(plan, n, sub=None):
    """The coordinate arrays of one grid of a gather call: (a, b, points) — the two axes, or with a pole in view (`points` True)
    the two point arrays.  They hold the grid's cell centres, or (`sub`; default: n > 1) the n x n sub-samples per cell that
    :func:`gather_subsample_coordinates` describes.  The only place that decides between the two forms."""
    points = bool(plan['contains_pole'])
    if sub is None:
        sub = n > 1
    if sub:
        grid = plan['grid']
        a = _subsample_axis(grid.lat[:, 0], n)
        b = _subsample_axis(grid.lon[0, :], n)
        if points:
            a, b = _rotate_pole_host(np.repeat(a[:, None], b.size, 1), np.repeat(b[None, :], a.size, 0), plan['altitude'], -90)
        elif plan['contains_discontinuity']:
            b = wrap_at_180(b + 180)
        return a, b, points
    coords = grid_coordinates(plan)
    if points:
        return coords['lat_c'], coords['lon_c'], True
    return coords['lat_c'][:, 0], coords['lon_c'][0, :], False


def gather_box_pipeline(ctx, width, height):
    """The frame pipeline behind the box pass of the gather plans (one per host thread, device and frame size; it holds no
    image and no per-pixel array)."""
    from .pipeline import FramePipeline
    key = (str(ctx.device), int(width), int(height))
    return _GATHER_PIPES.get(key, lambda: FramePipeline(width, height, alloc_image=False, alloc_coords=False))


def _gather_box(mapping, params, zen, magnetic):
    """The box pass for a camera mapping whose arrays do not exist: (the 8-number bounding-box reduction of the frame kernel's
    box pass — no per-pixel array is written —, in (lat, lon) or (MLat, SM longitude), [7]: a pole of those coordinates is in
    view; the ``maskedByElevation`` the mapping remembers, which stays a threshold).  None, None for any other mapping."""
    if zen is None and getattr(mapping, '_frame', True) is None:
        lazy = getattr(mapping, '_lazy_elev', None)
        return gather_box_pipeline(Context.current(), params.width, params.height).box_first(params, lazy, magnetic), lazy
    return None, None


def gather_box_grid(red, pxPerDeg, arcsecPerPx):
    """The grid part of a gather plan from a box pass's reduction — :func:`resample`'s grid for that box: its resolution
    (``plateCarreeResolution`` with `arcsecPerPx`), the date-line shift, :func:`cached_grid` —, and the resolution used:
    (dict(grid, contains_pole=False, contains_discontinuity), (latPxPerDeg, lonPxPerDeg)).  `grid` is None where there is no
    longitude resolution (``plateCarreeResolution`` of a box that goes all the way round): the callers refuse that."""
    from .mapping.mapping import bounding_box_from_reduction
    bb = bounding_box_from_reduction(red)
    ppd = plateCarreeResolution(bb, arcsecPerPx) if arcsecPerPx else _px_per_deg(pxPerDeg)
    lonMin, lonMax = bb.lonWest, bb.lonEast
    if bb.containsDiscontinuity:
        lonMin, lonMax = wrap_at_180(lonMin + 180), wrap_at_180(lonMax + 180)
    grid = cached_grid(ppd, bb.latSouth, bb.latNorth, lonMin, lonMax) if ppd[1] > 0 else None
    return dict(grid=grid, contains_pole=False, contains_discontinuity=bool(bb.containsDiscontinuity)), ppd


def _mapping_lens(mapping):
    """the ``amt_lens_model`` that goes with a mapping's ``_inverse_model``, or None (also for objects that only model one)"""
    lens = getattr(mapping, '_inverse_lens', None)
    return None if lens is None else lens()


def gather_plan(mapping, pxPerDeg=25, arcsecPerPx=None, containsPole=None, magnetic=False):
    """
    What :func:`resampleGather` samples where: dict(grid, contains_pole, contains_discontinuity, altitude, params, zenithal,
    lens, min_elevation, center_mask).  `lens` is the ``amt_lens_model`` of a raw frame that still carries its lens distortion
    (``getMapping(lensRoute='raw')``; None otherwise): the cells are then projected through the camera model and the lens into
    the raw frame, whose pixels are sampled once.  The grid is the one :func:`resample` chooses for the same arguments (same bounding box,
    :func:`fixedGrid`, longitude frame).  A camera mapping whose arrays nobody has asked for yet gets its box from the box pass
    of the frame kernel and keeps a remembered ``maskedByElevation`` as a threshold (`min_elevation`); any other mapping is
    asked for its bounding box, and its centre mask (a device tensor) goes into the plan.
    """
    if not isinstance(mapping, BaseMapping):
        raise NotImplementedError('resampleGather takes one mapping; collections or lists are gathered onto one grid by '
                                  'resampleGatherMosaic')
    params, zen = mapping._inverse_model()
    plan = dict(altitude=mapping.altitude, params=params, zenithal=zen, lens=_mapping_lens(mapping), min_elevation=None,
                center_mask=None)
    red, lazy = _gather_box(mapping, params, zen, magnetic)
    if red is not None and not (bool(red[7]) if containsPole is None else bool(containsPole)):
        part, _ = gather_box_grid(red, pxPerDeg, arcsecPerPx)
        assert part['grid'] is not None         # (what _Grid asserts: a longitude resolution)
        plan.update(part, min_elevation=lazy)
        return plan
    # arrays exist (or a pole is in view, whose rotated grid is laid out from them): the two-pass plan's grid
    src = convertMappingToSM(mapping) if magnetic else mapping
    pole, ppd = _pole_and_resolution(src, pxPerDeg, arcsecPerPx, containsPole)
    fd = src.frame()
    grid, _, _, _ = _frame_grid(fd, src.altitude, src.boundingBox, ppd, src.containsDiscontinuity, pole, None,
                                src.outline if pole else None, None)
    plan.update(grid=grid, contains_pole=bool(pole), contains_discontinuity=bool(src.containsDiscontinuity) and not pole,
                center_mask=fd.center_mask_tensor())
    return plan


def gather_frame(plan, image, interpolation='linear', magnetic=False, supersample=1, minCoverage=None):
    """
    The device side of :func:`resampleGather` on a :func:`gather_plan`: cell centres through ``amt_grid_to_pixel`` (with a pole
    in view the centres of the rotated grid are rotated back and go through ``amt_world_to_pixel``), the image through
    ``amt_remap_coords`` or, for 'nearest', a gather of pixel (rint x, rint y).  Returns a :func:`resample_frame`-like dict:
    lat, lon, lat_c, lon_c, img, mask, elevation (exact line-of-sight elevation of every cell centre), flags, support.

    ``supersample`` n > 1: one call of ``amt_gather_mosaic_supersampled`` on a table of this one member — n x n sub-samples per
    cell (:func:`gather_subsample_coordinates`), each masked by the same rules, the seen ones averaged.  The dict then holds
    ``count`` (ny, nx) uint8, the seen sub-samples of every cell, in place of flags and support; a cell is masked unless
    ``count >= supersample_min_count(minCoverage, n)``, and elevation is the mean over the seen sub-samples.
    """
    import torch
    from .coordinates.inverse import W2P_GEODETIC, W2P_SM, grid_to_pixel, world_to_pixel
    from .util.lensdistortion import INTERPOLATIONS, _image_to_device
    _check_gather_interpolation(interpolation)
    n, min_count = _check_supersample(supersample, minCoverage)
    if n > 1:
        out = _gather_mosaic_call(plan, [plan], [image], interpolation, magnetic, 1, n, min_count, None)   # (the plan is the member)
        del out['source']
        return out
    ctx = Context.current()
    grid, params, zen, lens = plan['grid'], plan['params'], plan['zenithal'], plan.get('lens')
    frame = W2P_SM if magnetic else W2P_GEODETIC
    need64 = interpolation == 'nearest' or plan['center_mask'] is not None
    a, b, points = _gather_job_coordinates(plan, 1)
    a, b = ctx.to_device(np.ascontiguousarray(a)), ctx.to_device(np.ascontiguousarray(b))
    if points:
        xy, elev, flags = world_to_pixel(params, zen, frame, a, b, lens=lens)
        xy32 = xy.to(torch.float32)
    else:
        xy32, xy, elev, flags = grid_to_pixel(ctx, params, zen, frame, a, b, xy64=need64, lens=lens)
    src, np_dtype, _ = _image_to_device(ctx, image)
    h, w, nch = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    if (w, h) != (params.width, params.height):
        raise ValueError('the image is %d x %d, the camera model is for %d x %d' % (w, h, params.width, params.height))
    mask = flags != 0
    support = None
    if need64:
        # the nearest pixel (half to even, like rint), kept inside the frame for the cells that are masked anyway
        near = torch.nan_to_num(torch.round(xy), nan=0.0, posinf=0.0, neginf=0.0)
        ix = near[..., 0].clamp_(0, w - 1).to(torch.int64)
        iy = near[..., 1].clamp_(0, h - 1).to(torch.int64)
        if plan['center_mask'] is not None:
            mask |= plan['center_mask'].reshape(h, w)[iy, ix] != 0
    if interpolation == 'nearest':
        dst = src[iy, ix]
    else:
        dst = torch.empty((grid.ny, grid.nx, nch), dtype=src.dtype, device=src.device)
        support = torch.empty((grid.ny, grid.nx), dtype=torch.uint8, device=src.device)
        ctx.call('amt_remap_coords', ptr(src), w, h, src.element_size(), nch, ptr(xy32), grid.nx, grid.ny,
                 INTERPOLATIONS[interpolation], ptr(dst), ptr(support), None)
        mask |= support == 0
    if plan['min_elevation'] is not None:
        mask |= ~(elev >= float(plan['min_elevation']))
    return gather_result(plan, flags=to_host(flags), support=None if support is None else to_host(support),
                         **gather_to_host(dict(img=dst, mask=mask.to(torch.uint8), elevation=elev), np_dtype))


def _gather_image(mapping):
    img = getattr(mapping, '_img_array', None)
    return mapping.img_unmasked if img is None else img


def gather_result(plan, /, **arrays):
    """The dict every gather call returns for a plan: the grid's coordinates (:func:`grid_coordinates`), grid, contains_pole and
    contains_discontinuity, then `arrays`."""
    return dict(grid_coordinates(plan), grid=plan['grid'], contains_pole=plan['contains_pole'],
                contains_discontinuity=plan['contains_discontinuity'], **arrays)


def gather_to_host(out, np_dtype):
    """dict(img, mask, elevation[, count]) of a grid's device tensors as host arrays: img of the image's numpy dtype, from a
    contiguous tensor, mask bool, count uint8 (each read synchronises on the current stream)"""
    host = dict(img=to_host(out['img'].contiguous(), dtype=np_dtype), mask=to_host(out['mask']).astype(bool),
                elevation=to_host(out['elevation']))
    if 'count' in out:
        host['count'] = to_host(out['count'], dtype=np.uint8)
    return host


def _gather_finish(res, smTime=None):
    """What the class functions make a mapping of: (lat, lon, lat_c, lon_c, masked elevation, masked img) of a gather result; with
    `smTime` the coordinates of an (MLat, SM longitude) grid are converted back for that time."""
    img = ma.masked_array(res['img'], mask=np.repeat(res['mask'][:, :, None], res['img'].shape[2], 2))
    elevation = ma.masked_array(res['elevation'], mask=res['mask'] | np.isnan(res['elevation']))
    corners = (res['lat'], res['lon'], res['lat_c'], res['lon_c']) if smTime is None else sm_grid_to_geographic(res, smTime)
    return corners + (elevation, img)


def _with_coverage(mapping, res, n):
    """the fraction of every cell's sub-samples that were seen, as a plain attribute of a supersampled result"""
    if n > 1:
        mapping.coverage = res['count'] / float(n * n)
    return mapping


def _resample_gather(mapping, pxPerDeg, arcsecPerPx, containsPole, interpolation, magnetic, supersample=1, minCoverage=None):
    _check_gather_interpolation(interpolation)
    n, _ = _check_supersample(supersample, minCoverage)
    plan = gather_plan(mapping, pxPerDeg, arcsecPerPx, containsPole, magnetic)
    res = gather_frame(plan, _gather_image(mapping), interpolation, magnetic, supersample, minCoverage)
    if not magnetic:
        return _with_coverage(mapping.createResampled(*_gather_finish(res)), res, n)
    from .mapping.mapping import GenericMapping
    lat, lon, lat_c, lon_c, elevation, img = _gather_finish(res, mapping.photoTime)
    return _with_coverage(GenericMapping(lat, lon, lat_c, lon_c, elevation, mapping.altitude, img, mapping.cameraPosGCRS,
                                         mapping.photoTime, mapping.identifier), res, n)


def resampleGather(mapping, pxPerDeg=25, arcsecPerPx=None, containsPole=None, interpolation='linear', supersample=1,
                   minCoverage=None):
    """
    Resampling by gathering: every cell centre of the grid that :func:`resample` would choose for the same arguments is
    projected into the image through the inverse of the camera model (``amt_grid_to_pixel``) and the image is sampled there
    (``amt_remap_coords``: 'linear' or 'lanczos4'; 'nearest': the pixel at (rint x, rint y)).  The result has no holes at any
    resolution, also finer than the pixel footprint, where binning pixel centres leaves cells empty, and it needs no
    triangulation: unlike ``resample(method='linear')`` (scipy's griddata) it interpolates in the pixel plane, not in the
    lat / lon plane.  With ``supersample=1`` it samples one point per cell without averaging, which aliases where cells are
    much coarser than a pixel; ``supersample=n`` (2 ... 8) serves that case: every cell is split into n x n equal parts, the
    centre of each is gathered by the same rules, and the cell takes the mean of the seen ones, in one fused kernel
    (``amt_gather_mosaic_supersampled``; :func:`gather_subsample_coordinates` says where the sub-samples lie).  A cell is then
    masked unless at least ``supersample_min_count(minCoverage, n)`` of its n x n sub-samples are seen (`minCoverage` None: half of
    them), ``.elevation`` is the mean over the seen ones, and the result carries ``.coverage`` (ny, nx), the seen fraction.

    A cell is masked where its centre is not seen in the frame (any flag of ``amt_world_to_pixel``: invalid, hidden, outside
    the projection's domain or the frame), where the sampled point has no support (it lies outside [0, width - 1] x
    [0, height - 1]; not for 'nearest'), where the mapping's centre mask is set at the nearest pixel, and where the elevation of
    the cell's line of sight is below the mapping's elevation threshold — a ``maskedByElevation`` that a camera mapping only
    remembers is applied as that threshold, without computing the frame's arrays.  ``.elevation`` of the result is the exact
    line-of-sight elevation of each cell centre.

    For mappings with a zenithal (+ SIP) WCS camera model; ``NotImplementedError`` for collections and lists
    (:func:`resampleGatherMosaic` gathers those onto one grid), for mappings
    made from a bare direction array, and for MIRACLE / THEMIS.  A raw frame that still carries its lens distortion
    (``getMapping(lens=, lensRoute='raw')``) is gathered through its lens: the cell centres go through the camera model and
    then the lens model (``amt_grid_to_pixel_lens``) into the raw frame, whose pixels are interpolated once — no corrected
    image in between; ``supersample`` goes with it (``amt_gather_mosaic_supersampled_lens``).

    :param interpolation: 'nearest', 'linear' or 'lanczos4'
    :param int supersample: sub-samples per cell and axis, 1 ... 8
    :param None|number minCoverage: with ``supersample > 1`` only: the least seen fraction of a valid cell, in (0, 1]
    :raises ValueError: for an unknown interpolation, then for a `supersample` that is not an int in 1 ... 8, a `minCoverage`
                        outside (0, 1], and a `minCoverage` given with ``supersample=1`` — before any device work
    :rtype: GenericMapping (what ``mapping.createResampled`` returns)
    """
    return _resample_gather(mapping, pxPerDeg, arcsecPerPx, containsPole, interpolation, False, supersample, minCoverage)


def resampleGatherMLatMLT(mapping, **kw):
    """:func:`resampleGather` on the (MLat, SM longitude) grid of :func:`resampleMLatMLT`; see there for the parameters."""
    return _resample_gather(mapping, kw.pop('pxPerDeg', 25), kw.pop('arcsecPerPx', None), kw.pop('containsPole', None),
                            kw.pop('interpolation', 'linear'), True, **kw)


# ---- gather mosaics: a collection gathered onto one grid, one fused kernel ---------------------------------------------------------
_GATHER_INTERP_CODES = {'linear': 0, 'lanczos4': 1, 'nearest': 2}      # AMT_INTERP_LINEAR / _LANCZOS4 / _NEAREST
GATHER_PATH_AUTO, GATHER_PATH_STAGED, GATHER_PATH_CELL = 0, 1, 2      # AMT_GATHER_PATH_*


def _gather_collection(collection):
    """A list of mappings is a collection whose members may overlap."""
    if isinstance(collection, MappingCollection):
        return collection
    if isinstance(collection, BaseMapping):
        return MappingCollection([collection], collection.identifier, mayOverlap=True)
    members = list(collection)
    return MappingCollection(members, members[0].identifier if members else None, mayOverlap=True)


def gather_mosaic_plan(collection, pxPerDeg=25, arcsecPerPx=None, containsPole=None, magnetic=False):
    """
    The host side of :func:`resampleGatherMosaic`: checks the members the way :func:`mosaic_plan` does (not empty, equal
    altitudes, equal image dtype and channel count), asks every member for its camera model (``_inverse_model``; its
    ``NotImplementedError`` passes through with the member's identifier) and lays out the common grid: :func:`mosaic_layout`
    of the members' boxes, which is :func:`resample`'s grid for the merged box, date-line rule included.  A camera mapping
    whose arrays do not exist gets its box from the box pass of the frame kernel and keeps a remembered ``maskedByElevation``
    as its threshold, as in :func:`gather_plan`; any other member is asked for ``boundingBox`` and its centre mask goes along.
    With a pole in view (`containsPole` True, or None and a member's box pass or ``containsPole`` says so) the layout is
    :func:`mosaic_plan`'s pole layout, from the members' rotated outlines.

    :return: mosaic_layout's dict plus altitude, contains_pole, contains_discontinuity, rule, identifiers and members: a list
             of dict(params, zenithal, lens, min_elevation, center_mask, image); `lens` as in :func:`gather_plan`: members that
             are raw frames with their lens (``getMapping(lensRoute='raw')``) and members without mix freely
    """
    collection = _gather_collection(collection)
    mappings = list(collection.mappings)
    if not mappings:
        raise ValueError('resampleGatherMosaic: the collection %r is empty' % (collection.identifier,))
    altitudes = [m.altitude for m in mappings]
    if any(a != altitudes[0] for a in altitudes):
        raise ValueError('resampleGatherMosaic: the members differ in altitude: %s' %
                         ', '.join('%s: %s km' % (m.identifier, m.altitude) for m in mappings))
    images = [_gather_image(m) for m in mappings]
    kinds = [(np.dtype(im.dtype), 1 if np.ndim(im) == 2 else int(np.shape(im)[2])) for im in images]
    if any(k != kinds[0] for k in kinds):
        raise ValueError('resampleGatherMosaic: the members differ in image dtype or channel count: %s' %
                         ', '.join('%s: %s x %d' % (m.identifier, k[0], k[1]) for m, k in zip(mappings, kinds)))
    models = []
    for m in mappings:
        try:
            models.append(m._inverse_model())
        except NotImplementedError as e:
            raise NotImplementedError('resampleGatherMosaic: member %s: %s' % (m.identifier, e))
    altitude = altitudes[0]
    # the box pass for camera mappings whose arrays do not exist
    passes = [_gather_box(m, params, zen, magnetic) for m, (params, zen) in zip(mappings, models)]
    arrays = [None if red is not None else (convertMappingToSM(m) if magnetic else m) for m, (red, _) in zip(mappings, passes)]
    if containsPole is None:
        pole = any(bool(red[7]) if red is not None else bool(src.containsPole) for (red, _), src in zip(passes, arrays))
    else:
        pole = bool(containsPole)
    if pole:
        # the rotated grid is laid out from the members' outlines: every member's arrays
        passes = [(None, None)] * len(mappings)
        arrays = [convertMappingToSM(m) if magnetic else m for m in mappings]
    from .mapping.mapping import bounding_box_from_reduction
    boxes, members = [], []
    for (params, zen), lens, (red, lazy), src, image in zip(models, [_mapping_lens(m) for m in mappings], passes, arrays, images):
        member = dict(params=params, zenithal=zen, lens=lens, min_elevation=None, center_mask=None, image=image)
        if red is not None:
            boxes.append(bounding_box_from_reduction(red))
            member.update(min_elevation=lazy)
        else:
            boxes.append(src.boundingBox)
            member.update(center_mask=src.frame().center_mask_tensor())
        members.append(member)
    poleBoxes = None
    if pole:
        poleBoxes = []
        for src in arrays:
            outline = np.asarray(src.outline, dtype=np.float64)
            ola, olo = _rotate_pole_host(outline[:, 0], outline[:, 1], altitude, 90)
            poleBoxes.append((ola.min(), ola.max(), olo.min(), olo.max()))
    plan = mosaic_layout(boxes, pxPerDeg, arcsecPerPx, poleBoxes)
    plan.update(altitude=altitude, contains_pole=plan['pole'], contains_discontinuity=plan['discontinuity'],
                rule=1 if collection.mayOverlap else 0, members=members, identifiers=[m.identifier for m in mappings])
    return plan


def _gather_member_table(ctx, members, images):
    """The amt_gather_member table of a gather call: (table, keep, channels, torch dtype, numpy dtype); `keep` holds what the
    table points to and has to outlive the call's kernel."""
    from ._native import GatherMember
    from .util.lensdistortion import _image_to_device
    table = (GatherMember * len(members))()
    keep, kinds, np_dtype = [], set(), None
    for t, m, image in zip(table, members, images):
        src, np_dtype, _ = _image_to_device(ctx, image)
        h, w, nch = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
        if (w, h) != (m['params'].width, m['params'].height):
            raise ValueError('the image is %d x %d, the camera model is for %d x %d' % (w, h, m['params'].width, m['params'].height))
        kinds.add((np.dtype(np_dtype), nch, src.dtype))
        C.memmove(C.byref(t.params), C.byref(m['params']), C.sizeof(m['params']))
        if m['zenithal'] is not None:
            t.zenithal = C.pointer(m['zenithal'])
        t.img = ptr(src).value
        cm = m['center_mask']
        t.center_mask = None if cm is None else ptr(cm).value
        t.min_elevation = float('nan') if m['min_elevation'] is None else float(m['min_elevation'])
        keep.append((src, cm, m['zenithal']))
    if len(kinds) != 1:
        raise ValueError('the members\' images differ in dtype or channel count')
    _, nch, tdtype = next(iter(kinds))
    return table, keep, nch, tdtype, np_dtype


def _gather_lens_table(members):
    """The `lenses` argument of the ``_lens`` gather entry points for `members` (dicts that may hold ``lens``, an
    ``amt_lens_model``): an array of pointers, NULL where a member has no lens, or None where nobody has one — the caller then
    takes the entry point without ``_lens``.  The array refers to the members' models, which the members keep alive."""
    from ._native import LensModel
    lenses = [m.get('lens') for m in members]
    if all(lens is None for lens in lenses):
        return None
    table = (C.POINTER(LensModel) * len(members))()
    for i, lens in enumerate(lenses):
        if lens is not None:
            table[i] = C.pointer(lens)
    return table


def gather_tiles(grid, n):
    """(tiles_y, tiles_x) of a grid gathered with n x n sub-samples per cell: a tile is 32 // n cells a side"""
    T = 32 // n
    return (grid.ny + T - 1) // T, (grid.nx + T - 1) // T


def _gather_debug(ctx, debug, tiles):
    """amt_gather_debug of a `debug` dict and the tensor of its tile_path (one byte per tile, of shape `tiles`), or None, None"""
    from ._native import GatherDebug
    if debug is None:
        return None, None
    import torch
    dbg, tile_path = GatherDebug(), None
    dbg.force_path = int(debug.get('force_path', GATHER_PATH_AUTO))
    if debug.get('tile_path'):
        tile_path = ctx.zeros(tiles, torch.uint8)
        dbg.tile_path = ptr(tile_path).value
    return dbg, tile_path


def _gather_mosaic_call(plan, members, images, interpolation, magnetic, rule, n, min_count, debug, xy=False, supersampled=None):
    """ONE call of ``amt_gather_mosaic`` or, `supersampled` (default: n > 1), of ``amt_gather_mosaic_supersampled`` with n x n
    sub-samples per cell (include/auromat_hip.h states what they compute) on the plan's grid: the result dict of
    :func:`gather_mosaic_frames`, with ``count`` from the supersampled entry point and, if asked for, ``xy`` from the plain one."""
    import torch
    from .coordinates.inverse import W2P_GEODETIC, W2P_SM
    if supersampled is None:
        supersampled = n > 1
    ctx = Context.current()
    grid = plan['grid']
    ny, nx = grid.ny, grid.nx
    table, keep, nch, tdtype, np_dtype = _gather_member_table(ctx, members, images)
    a, b, points = _gather_job_coordinates(plan, n, supersampled)
    a, b = ctx.to_device(np.ascontiguousarray(a)), ctx.to_device(np.ascontiguousarray(b))
    lat, lon, cell_lat, cell_lon = (None, None, a, b) if points else (a, b, None, None)
    dev = dict(img=torch.empty((ny, nx, nch), dtype=tdtype, device=ctx.device), mask=ctx.empty((ny, nx), torch.uint8),
               elevation=ctx.empty((ny, nx)))
    source = ctx.empty((ny, nx), torch.int32)
    if supersampled:
        dev['count'] = ctx.empty((ny, nx), torch.uint8)
        fn, factor, last = 'amt_gather_mosaic_supersampled', (n, min_count), dev['count']
    else:
        fn, factor, last = 'amt_gather_mosaic', (), ctx.empty((ny, nx, 2)) if xy else None
    dbg, tile_path = _gather_debug(ctx, debug, gather_tiles(grid, n))
    lenses = _gather_lens_table(members)
    ctx.call(fn if lenses is None else fn + '_lens', table, len(members), W2P_SM if magnetic else W2P_GEODETIC, ptr(lat), ny, ptr(lon),
             nx, ptr(cell_lat), ptr(cell_lon),
             *factor + (dev['img'].element_size(), nch, _GATHER_INTERP_CODES[interpolation], int(rule), ptr(dev['img']),
                        ptr(dev['mask']), ptr(dev['elevation']), ptr(source), ptr(last), None if dbg is None else C.byref(dbg)) +
             (() if lenses is None else (lenses,)))
    out = gather_result(plan, source=to_host(source, dtype=np.int32), altitude=plan['altitude'], plan=plan,
                        **gather_to_host(dev, np_dtype))
    if xy and not supersampled:
        out['xy'] = to_host(last)
    if tile_path is not None:
        out['tile_path'] = to_host(tile_path)
    del keep                     # (after the read-back above: the kernel is done with them)
    return out


def gather_mosaic_frames(plan, images=None, interpolation='linear', magnetic=False, debug=None, xy=False, supersample=1,
                         minCoverage=None):
    """
    The device side of :func:`resampleGatherMosaic` on a :func:`gather_mosaic_plan`: ONE call of ``amt_gather_mosaic``
    (include/auromat_hip.h states what it computes), which projects every cell centre through every member's camera model,
    elects one member per cell by the plan's rule and samples that member's image alone.  With a pole in view the centres of
    the rotated grid are rotated back on the host and go in through the point form, as in :func:`gather_frame`.

    ``supersample`` n > 1: ONE call of ``amt_gather_mosaic_supersampled`` instead — the same at each of the n x n sub-samples
    of every cell (:func:`gather_subsample_coordinates`), reduced to cells in the kernel: the mean of the seen sub-samples'
    samples and elevations, ``source`` the member that won most of them, ``count`` (ny, nx) uint8 how many were seen, and a
    cell masked unless ``count >= supersample_min_count(minCoverage, n)``.  `xy` does not go with it.

    :param images: one image per member (default: the plan's)
    :param debug: dict(force_path=GATHER_PATH_*, tile_path=True): amt_gather_debug; the result then holds ``tile_path``
                  (tiles_y, tiles_x) uint8, a tile being 32 x 32 cells (32 // n x 32 // n with ``supersample`` n)
    :param xy: also return ``xy`` (ny, nx, 2) float64, the winner's pixel coordinates
    :return: dict like :func:`mosaic_frames`': lat, lon, lat_c, lon_c, img (ny, nx, C), mask (ny, nx) bool, elevation (ny, nx;
             the winner's, NaN where nobody sees the cell), source (ny, nx) int32 [-1: nobody], plan
    """
    _check_gather_interpolation(interpolation)
    n, min_count = _check_supersample(supersample, minCoverage)
    members = plan['members']
    images = [m['image'] for m in members] if images is None else list(images)
    if len(images) != len(members):
        raise ValueError('%d images for %d members' % (len(images), len(members)))
    if n > 1 and xy:
        raise ValueError('xy: a supersampled cell has no single pixel position')
    return _gather_mosaic_call(plan, members, images, interpolation, magnetic, plan['rule'], n, min_count, debug, xy)


def _resample_gather_mosaic(collection, pxPerDeg, arcsecPerPx, containsPole, interpolation, magnetic, supersample=1,
                            minCoverage=None):
    from .mapping.mapping import MosaicMapping
    _check_gather_interpolation(interpolation)
    n, _ = _check_supersample(supersample, minCoverage)
    collection = _gather_collection(collection)
    plan = gather_mosaic_plan(collection, pxPerDeg, arcsecPerPx, containsPole, magnetic)
    res = gather_mosaic_frames(plan, None, interpolation, magnetic, supersample=supersample, minCoverage=minCoverage)
    source = ma.masked_array(res['source'], mask=res['source'] < 0)
    members = collection.mappings
    photoTime = collection.photoTime
    first = next(m for m in members if m.photoTime == photoTime)
    lat, lon, lat_c, lon_c, elevation, img = _gather_finish(res, photoTime if magnetic else None)
    return _with_coverage(MosaicMapping(lat, lon, lat_c, lon_c, elevation, plan['altitude'], img, first.cameraPosGCRS, photoTime,
                                        collection.identifier, source, plan['identifiers']), res, n)


def resampleGatherMosaic(collection, pxPerDeg=25, arcsecPerPx=None, containsPole=None, interpolation='linear', supersample=1,
                         minCoverage=None):
    """
    :func:`resampleGather` for a collection: every member gathered onto ONE grid — the grid :func:`resampleMosaic` lays out
    for the same collection and arguments — in one fused kernel (``amt_gather_mosaic``).  Every cell centre is projected
    through every member's camera model; member i sees a cell by :func:`resampleGather`'s four masking rules; one member wins
    the cell and only its image is sampled there.  ``collection.mayOverlap`` True (a list of mappings counts as such a
    collection): the member whose line of sight to the cell centre has the highest elevation wins (the reference's drawing
    rule for overlapping mappings), the earlier member on a tie.  False: the first member that sees the cell.  Towards every
    member's horizon, where binning leaves holes that the overlap rule then has to choose between, gathering leaves none.

    ``.elevation`` of the result is the winner's exact line-of-sight elevation, ``.source`` the winner's index (masked where
    nobody sees the cell), ``.members`` the members' identifiers.

    ``supersample=n`` (2 ... 8), for cells much coarser than a pixel: all of the above happens at the n x n sub-samples of
    every cell (:func:`gather_subsample_coordinates`) — each has its own winner — and the cell takes the mean of the seen
    sub-samples' samples and elevations, in the same kernel launch (``amt_gather_mosaic_supersampled``).  ``.source`` is then
    the member that won most sub-samples (the earlier one on a tie), a cell is masked unless at least
    ``supersample_min_count(minCoverage, n)`` sub-samples are seen (`minCoverage` None: half of them), and the result
    carries ``.coverage`` (ny, nx), the seen fraction.

    :param interpolation: 'nearest', 'linear' or 'lanczos4'
    :param int supersample: sub-samples per cell and axis, 1 ... 8
    :param None|number minCoverage: with ``supersample > 1`` only: the least seen fraction of a valid cell, in (0, 1]
    :raises ValueError: for an unknown interpolation (before anything else), then a `supersample` that is not an int in
                        1 ... 8, a `minCoverage` outside (0, 1] or given with ``supersample=1``; an empty collection, members
                        of different altitudes or image dtypes / channel counts
    :raises NotImplementedError: for a member without a camera model in closed form (named in the message)
    :rtype: MosaicMapping
    """
    return _resample_gather_mosaic(collection, pxPerDeg, arcsecPerPx, containsPole, interpolation, False, supersample,
                                   minCoverage)


def resampleGatherMosaicMLatMLT(collection, **kw):
    """:func:`resampleGatherMosaic` on the (MLat, SM longitude) grid of :func:`resampleMosaicMLatMLT`: the cell centres go
    through the camera models as SM coordinates (``AMT_W2P_SM``) and the grid's coordinates are converted back."""
    return _resample_gather_mosaic(collection, kw.pop('pxPerDeg', 25), kw.pop('arcsecPerPx', None), kw.pop('containsPole', None),
                                   kw.pop('interpolation', 'linear'), True, **kw)


# ---- gathered frames: a batch of frames, each onto its own grid, one fused kernel ----------------------------------------------
def gather_frames_coordinates(plans, n):
    """The coordinates of a batch of ``amt_gather_frames``: (per plan (size of a, size of b, points), every plan's two arrays
    flattened one after the other into ONE float64 array — what a single copy takes to the device)."""
    host = [_gather_job_coordinates(p, n) for p in plans]
    flat = np.concatenate([np.ravel(np.asarray(v, dtype=np.float64)) for a, b, _ in host for v in (a, b)])
    return [(int(np.size(a)), int(np.size(b)), points) for a, b, points in host], flat


def _gather_frames_call(ctx, plans, images, interpolation, magnetic, n, min_count, debug=None, coords=None, arena=None):
    """ONE call of ``amt_gather_frames`` on at most GATHER_MAX_JOBS plans: (a list of dict(img, mask, elevation[, count]) of
    device tensors — views into one flat tensor per output kind —, the call's tile_path tensor or None, the images' numpy dtype).
    `coords`: (sizes, the flat device tensor) of :func:`gather_frames_coordinates` when the caller has copied them already;
    `arena`: function (cells, channels, torch dtype, n) -> dict(img, mask, elevation[, count]) of flat tensors, in place of fresh
    ones."""
    import torch
    from ._native import GATHER_MAX_JOBS, GatherJob
    from .coordinates.inverse import W2P_GEODETIC, W2P_SM
    assert 1 <= len(plans) <= GATHER_MAX_JOBS
    table, keep, nch, tdtype, np_dtype = _gather_member_table(ctx, plans, images)      # (a plan holds a member's keys)
    if coords is None:
        sizes, flat = gather_frames_coordinates(plans, n)
        coords = (sizes, ctx.to_device(flat))           # every job's coordinates in one copy
    sizes, coords = coords
    cells = [p['grid'].ny * p['grid'].nx for p in plans]
    total = sum(cells)
    if arena is None:
        made = dict(img=torch.empty((total * nch,), dtype=tdtype, device=ctx.device), mask=ctx.empty((total,), torch.uint8),
                    elevation=ctx.empty((total,)))
        if n > 1:
            made['count'] = ctx.empty((total,), torch.uint8)
    else:
        made = arena(total, nch, tdtype, n)
    jobs = (GatherJob * len(plans))()
    outs, at, cell0, tiles = [], 0, 0, 0
    for job, member, plan, (na, nb, points), ncell in zip(jobs, table, plans, sizes, cells):
        ny, nx = plan['grid'].ny, plan['grid'].nx
        C.memmove(C.byref(job.member), C.byref(member), C.sizeof(member))
        job.ny, job.nx = ny, nx
        pa = coords.data_ptr() + 8 * at
        pb = pa + 8 * na
        at += na + nb
        if points:
            job.cell_lat, job.cell_lon = pa, pb
        else:
            job.lat, job.lon = pa, pb
        out = dict(img=made['img'][cell0 * nch:(cell0 + ncell) * nch].view(ny, nx, nch),
                   mask=made['mask'][cell0:cell0 + ncell].view(ny, nx), elevation=made['elevation'][cell0:cell0 + ncell].view(ny, nx))
        if n > 1:
            out['count'] = made['count'][cell0:cell0 + ncell].view(ny, nx)
            job.out_count = out['count'].data_ptr()
        job.out_img, job.out_mask, job.out_elev = out['img'].data_ptr(), out['mask'].data_ptr(), out['elevation'].data_ptr()
        outs.append(out)
        cell0 += ncell
        ty, tx = gather_tiles(plan['grid'], n)
        tiles += ty * tx
    assert at == coords.numel()
    dbg, tile_path = _gather_debug(ctx, debug, (tiles,))
    lenses = _gather_lens_table(plans)
    ctx.call('amt_gather_frames' if lenses is None else 'amt_gather_frames_lens', jobs, len(plans), W2P_SM if magnetic else W2P_GEODETIC,
             n, 1 if n == 1 else min_count, made['img'].element_size(), nch, _GATHER_INTERP_CODES[interpolation],
             None if dbg is None else C.byref(dbg), *(() if lenses is None else (lenses,)))
    # the kernel is enqueued on the current stream: the caching allocator hands the inputs' memory to nobody who is not behind it
    del keep, coords
    return outs, tile_path, np_dtype


def gather_frames(plans, images, interpolation='linear', magnetic=False, supersample=1, minCoverage=None, keep_on_device=False,
                  debug=None):
    """
    :func:`gather_frame` for a batch: the frames of `plans` (:func:`gather_plan` results, each with a grid of its own) and their
    `images` gathered by ONE call of ``amt_gather_frames`` per at most 64 plans — one kernel launch over the tiles of all of
    them, where a loop over :func:`gather_frame` pays a member-table copy and at least one launch per frame for grids of a few
    tiles.  The images may differ in size but not in dtype or channel count.

    Every cell holds what ``amt_gather_mosaic`` (``amt_gather_mosaic_supersampled`` with ``supersample`` > 1) gives for that one
    frame: the mask is :func:`gather_frame`'s, `img` and `elevation` are its values where unmasked, and 0 / NaN where masked.

    :param debug: dict(force_path=GATHER_PATH_*, tile_path=True): amt_gather_debug; every result then holds ``tile_path``, the
                  flat bytes of its job's tiles
    :return: one dict per plan with :func:`gather_frame`'s keys lat, lon, lat_c, lon_c, grid, img, mask, elevation,
             contains_pole, contains_discontinuity and, with ``supersample`` > 1, count; no flags and no support: no coordinate
             array exists.  With `keep_on_device` img, mask (uint8), elevation and count are device tensors.
    :raises ValueError: as :func:`resampleGather`, in its order and before any device work; then for lists of different lengths
    """
    from ._native import GATHER_MAX_JOBS
    _check_gather_interpolation(interpolation)
    n, min_count = _check_supersample(supersample, minCoverage)
    plans, images = list(plans), list(images)
    if len(images) != len(plans):
        raise ValueError('%d images for %d plans' % (len(images), len(plans)))
    ctx = Context.current()
    results = []
    for k in range(0, len(plans), GATHER_MAX_JOBS):
        chunk = plans[k:k + GATHER_MAX_JOBS]
        outs, tile_path, dtype = _gather_frames_call(ctx, chunk, images[k:k + GATHER_MAX_JOBS], interpolation, magnetic, n, min_count,
                                                     debug)
        tiles = None if tile_path is None else to_host(tile_path)
        t0 = 0
        for plan, out in zip(chunk, outs):
            res = gather_result(plan, **(out if keep_on_device else gather_to_host(out, dtype)))
            if tiles is not None:
                ty, tx = gather_tiles(plan['grid'], n)
                nt = ty * tx
                res['tile_path'] = tiles[t0:t0 + nt]
                t0 += nt
            results.append(res)
    return results
