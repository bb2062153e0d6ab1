"""
Constructed inputs of the scan-line tests (tests/test_scanline_cpu.py, tests/test_gpu_scanline_cells.py): property lists with
known strips, and frames / polygons / strips for the three kernels of auromat_amd/csrc/amt_scanline.hip.  Axes and polygons of
the select cases hold small dyadic numbers (integers, halves, eighths), so that every product of the crossing test is exact and
matplotlib and the kernel cannot differ by rounding.  The select kernel works in tiles of TILE x TILE cells and stages CHUNK
polygon edges at a time.
"""
import datetime
from collections import namedtuple

import numpy as np

TILE, CHUNK = 15, 256


# ---- property lists ------------------------------------------------------------------------------------------------------------

def props_along(track, n, step_deg, lead_deg=2.0, box_half=(5.0, 5.0), start=0.0):
    """`n` MappingProperties whose camera footpoints and centroids run along the equator heading east (track='equator':
    footpoint k at lon start + k * step_deg, its centroid lead_deg further east) or up a meridian (track='meridian':
    footpoint k at lat start + k * step_deg on lon 20, the centroid lead_deg further north)."""
    from auromat_amd.coordinates.geodesic import Location
    from auromat_amd.mapping.mapping import BoundingBox, MappingProperties
    t0 = datetime.datetime(2012, 1, 25, 9, 0, 0)
    out = []
    for k in range(n):
        at = start + k * step_deg
        foot, cen = (Location(0.0, at), Location(0.0, at + lead_deg)) if track == 'equator' else \
            (Location(at, 20.0), Location(at + lead_deg, 20.0))
        box = BoundingBox(cen.lat - box_half[0], cen.lon - box_half[1], cen.lat + box_half[0], cen.lon + box_half[1])
        out.append(MappingProperties(identifier='f%d' % k, altitude=110, cameraPosGCRS=np.zeros(3), boundingBox=box,
                                     photoTime=t0 + datetime.timedelta(seconds=3 * k), centroid=cen, cameraFootpoint=foot))
    return out


# ---- amt_scanline_select ---------------------------------------------------------------------------------------------------------

SelectCase = namedtuple('SelectCase', 'name lat_axis lon_axis polygon mask window')


def _lattice(ny, nx, lat_top=None, lon_left=0.0, step=1.0):
    """corner axes of ny x nx cells: latitudes descending from lat_top (default ny * step), longitudes ascending"""
    lat_top = ny * step if lat_top is None else lat_top
    return lat_top - step * np.arange(ny + 1), lon_left + step * np.arange(nx + 1)


def _mask(ny, nx, seed=None, density=0.3):
    if seed is None:
        return np.zeros((ny, nx), dtype=np.uint8)
    return (np.random.RandomState(seed).random_sample((ny, nx)) < density).astype(np.uint8)


def comb_polygon(length=40, step=0.125, low=0.5, high=(10.0, 9.5)):
    """a simple polygon of more than CHUNK vertices: a straight bottom at lat `low` from lon 0 to `length`, and back along a top
    that alternates between the two `high` latitudes every `step` of longitude"""
    back = np.arange(length, -step / 2, -step)
    top = [(high[i % 2], float(x)) for i, x in enumerate(back)]
    poly = np.array([(low, 0.0), (low, float(length))] + top)
    assert len(poly) > CHUNK
    return poly


def select_cases():
    cases = []

    def add(name, ny, nx, polygon, window=None, seed=None, **kw):
        lat, lon = _lattice(ny, nx, **kw)
        cases.append(SelectCase(name, lat, lon, np.asarray(polygon, dtype=np.float64).reshape(-1, 2), _mask(ny, nx, seed),
                                (0, 0, ny, nx) if window is None else window))

    # edges through corner points and along corner rows and columns: the rectangle lat 2..6, lon 3..9 on the integer lattice
    # (its south / west sides belong to it under the half-open rule, its north / east sides do not, or the other way round:
    # the oracle decides, every corner on the outline is compared), in both orientations
    rect = [(2, 3), (2, 9), (6, 9), (6, 3)]
    add('edges-on-lattice', 8, 12, rect)
    add('edges-on-lattice-reversed', 8, 12, rect[::-1])
    add('diagonal-through-corners', 8, 12, [(1, 1), (1, 9), (7, 9)])                   # hypotenuse through (k, k + 2)... corners
    add('vertex-on-lattice-longitude', 8, 12, [(1.5, 2.5), (1.5, 8.5), (6.5, 5)])      # apex on the column lon = 5
    add('concave', 12, 12, [(1, 1), (1, 11), (11, 11), (11, 8.5), (4.5, 8.5), (4.5, 3.5), (11, 3.5), (11, 1)])
    add('many-vertices', 11, 40, comb_polygon())
    add('many-vertices-masked', 11, 40, comb_polygon(), seed=3)
    add('outside-window', 20, 20, [(1.5, 1.5), (1.5, 5.5), (5.5, 5.5), (5.5, 1.5)], window=(0, 10, 8, 10))
    add('outside-grid', 6, 6, [(20, 20), (20, 30), (30, 30), (30, 20)])
    big = [(-5, -5), (-5, 50), (50, 50), (50, -5)]                                     # holds every corner of the grids below
    add('clipped-all-borders', 9, 7, big)
    add('clipped-north-west', 20, 20, [(12.5, -3), (12.5, 6.5), (33, 6.5), (33, -3)], window=(0, 0, 9, 8))
    add('clipped-south-east', 20, 20, [(-4, 12.5), (-4, 31), (6.5, 31), (6.5, 12.5)], window=(13, 12, 7, 8))
    add('one-cell', 1, 1, big)
    add('one-cell-masked', 1, 1, big, seed=1, lat_top=1.0)
    cases[-1].mask[:] = 1
    add('one-tile', TILE, TILE, big)
    add('one-tile-plus-one', TILE + 1, TILE + 1, big, seed=5)
    add('odd-sizes', 2 * TILE + 7, 3 * TILE + 2, [(3.5, 2.5), (1.5, 40.5), (35.5, 44.5), (30, 20), (33.5, 1.5)], seed=7)
    add('window-inside-polygon', 2 * TILE + 7, 3 * TILE + 2, big, window=(TILE - 1, TILE + 1, TILE + 2, 2 * TILE), seed=9)
    add('halves', 2 * TILE + 1, 2 * TILE + 3, [(1.25, 0.75), (2.75, 15.25), (14.25, 14.75), (9.5, 8), (15.25, 1.25)], seed=11,
        step=0.5)
    add('two-vertices', 5, 5, [(-5, -5), (50, 50)])
    add('no-vertices', 5, 5, np.zeros((0, 2)))
    add('empty-window', 5, 5, big, window=(2, 2, 0, 3))
    return cases


# ---- amt_scanline_pack / amt_scanline_compose ------------------------------------------------------------------------------------

def frame_data(ny, nx, nchan, with_elev, dtype, seed):
    """(planes (ny, nx, nchan + with_elev) float64, img (ny, nx, nchan) of `dtype`) with every value distinct enough to tell a
    wrong gather"""
    rs = np.random.RandomState(seed)
    planes = rs.random_sample((ny, nx, nchan + (1 if with_elev else 0))) * 1000
    top = np.iinfo(dtype).max
    img = rs.randint(0, top + 1, size=(ny, nx, nchan)).astype(dtype)
    return planes, img


def strip_records(rows, cols, nplane, nchan, dtype, seed):
    """a strip's records at the given global rows / columns with random contents"""
    rs = np.random.RandomState(seed)
    n = len(rows)
    return dict(row=np.asarray(rows, dtype=np.int32), col=np.asarray(cols, dtype=np.int32), planes=rs.random_sample((nplane, n)),
                img=rs.randint(0, np.iinfo(dtype).max + 1, size=(max(nchan, 1), n)).astype(dtype)[:nchan])


def block(r0, r1, c0, c1):
    """rows, cols of every cell of [r0, r1) x [c0, c1)"""
    r, c = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing='ij')
    return r.ravel(), c.ravel()
