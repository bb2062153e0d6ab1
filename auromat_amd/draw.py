"""
What is needed to look at a mapping: a resampled mapping's image as a PNG, and the parallels and meridians of an unresampled
frame as pixel polylines (:func:`graticulePixels`).  Everything else the reference's auromat/draw.py does (coastlines, labels,
figures) is matplotlib's business and not built here; the map products themselves are arrays, see
auromat_amd.resample.resampleStereographic, resampleStereographicMLatMLT, resampleMLatMLTPolar and resampleScanLines.
"""
import numpy as np
import numpy.ma as ma


def mapImageRGBA(mapping):
    """``mapping.img`` as (h, w, 4) uint8: alpha 0 where masked, 255 elsewhere; a uint16 image is shifted down by 8 bits, one
    channel is replicated into R, G and B (a fourth channel of the image is dropped)."""
    img = mapping.img
    data = np.asarray(ma.getdata(img))
    mask = ma.getmaskarray(img)
    if data.ndim == 2:
        data, mask = data[:, :, None], mask[:, :, None]
    if data.dtype == np.uint16:
        data = (data >> 8).astype(np.uint8)
    elif data.dtype != np.uint8:
        raise ValueError('image must be uint8 or uint16, but is {}'.format(data.dtype))
    if data.shape[2] == 1:
        data = np.repeat(data, 3, axis=2)
    elif data.shape[2] < 3:
        raise ValueError('image must have 1, 3 or 4 channels, but has {}'.format(data.shape[2]))
    rgba = np.empty(data.shape[:2] + (4,), dtype=np.uint8)
    rgba[:, :, :3] = data[:, :, :3]
    rgba[:, :, 3] = np.where(mask.any(axis=2), 0, 255)
    rgba[:, :, :3][rgba[:, :, 3] == 0] = 0
    return rgba


def saveMapImage(mapping, path):
    """Writes ``mapping.img`` as an RGBA PNG (Pillow): row 0 on top, transparent where the mapping is masked."""
    from PIL import Image
    Image.fromarray(mapImageRGBA(mapping), 'RGBA').save(path, format='PNG')


def _multiples(lo, hi, every):
    """the multiples of `every` in [lo, hi] (a multiple within 1e-9 of an end counts)"""
    first, last = int(np.ceil(lo / every - 1e-9)), int(np.floor(hi / every + 1e-9))
    return [k * every for k in range(first, last + 1)]


def _samples(lo, hi, step):
    """lo, lo + step, ... up to hi, and hi itself at the end"""
    n = int(np.floor((hi - lo) / step + 1e-9)) + 1
    v = lo + step * np.arange(n, dtype=np.float64)
    return v if hi - v[-1] <= 1e-9 * max(1.0, abs(hi)) else np.append(v, float(hi))


def _wrap180(v):
    """into [-180, 180); values already there keep their bits"""
    v = np.asarray(v, dtype=np.float64)
    return np.where((v >= -180.0) & (v < 180.0), v, (v + 180.0) % 360.0 - 180.0)


def graticule_lines(boundingBox, every=2, step=0.2):
    """
    The parallels and meridians of :func:`graticulePixels` before they meet a camera: ``(parallels, meridians)``, two lists of
    ``(degree, lats, lons)`` with the sample points of each line.  Lines lie on the multiples of `every` inside the box and
    are sampled every `step` degrees from one side of the box to the other, both ends included; a box across the date line runs
    from its west edge eastwards through 180 deg, a box with a pole all the way around.  Longitudes are in [-180, 180).
    """
    if not (every > 0 and step > 0):
        raise ValueError('every and step must be positive')
    south, north = float(boundingBox.latSouth), float(boundingBox.latNorth)
    west, east = float(boundingBox.lonWest), float(boundingBox.lonEast)
    if boundingBox.containsPole:
        west, east = -180.0, 180.0
    elif west > east:
        east += 360.0                                     # across the date line: unwrapped, wrapped again below
    lats, lons = _samples(south, north, step), _samples(west, east, step)
    meridian_degrees = _multiples(west, east, every)
    if east - west >= 360.0 and len(meridian_degrees) > 1 and meridian_degrees[-1] - meridian_degrees[0] >= 360.0:
        meridian_degrees = meridian_degrees[:-1]          # +180 is -180
    parallels = [(deg, np.full(lons.shape, float(deg)), _wrap180(lons)) for deg in _multiples(south, north, every)]
    meridians = []
    for deg in meridian_degrees:
        w = float(_wrap180(float(deg)))
        meridians.append((int(w) if isinstance(deg, int) else float(w), lats.copy(), np.full(lats.shape, float(w))))
    return parallels, meridians


def graticulePixels(mapping, every=2, step=0.2, boundingBox=None, altitude=None):
    """
    The parallels and meridians the reference's ``drawParallelsAndMeridians`` draws on an unresampled frame (draw.py:1482-1609),
    as pixel polylines: ``(parallels, meridians)``, two dicts ``{degree: (n, 2) float64 [x, y]}``.  The reference mean-resamples
    the pixel coordinates onto a 0.2 deg grid to get a look-up table from lat / lon to pixel; here every sample point goes
    through the camera model's inverse (``mapping.latLonToPixel``), exactly.  A vertex is NaN where the point is not seen
    (invalid, hidden behind the limb, outside the projection's domain, SIP inverse not converged), so that matplotlib breaks the
    line there; vertices outside the frame keep their coordinates.  Labels and figures are matplotlib's business.

    :param every: lines on the multiples of this many degrees inside the bounding box (the reference: 2)
    :param step: sampling distance along a line in degrees (the reference's table: 0.2)
    :param boundingBox: default: the mapping's
    :param altitude: km; default: the mapping's (0 draws the graticule on the ground)
    """
    box = mapping.boundingBox if boundingBox is None else boundingBox
    parallels, meridians = graticule_lines(box, every, step)
    lines = parallels + meridians
    if not lines:
        return {}, {}
    x, y = mapping.latLonToPixel(np.concatenate([l[1] for l in lines]), np.concatenate([l[2] for l in lines]), altitude=altitude)
    xy = np.stack((x.filled(np.nan), y.filled(np.nan)), axis=-1)
    out, at = [], 0
    for deg, la, _ in lines:
        out.append((deg, xy[at:at + la.size]))
        at += la.size
    return dict(out[:len(parallels)]), dict(out[len(parallels):])
