"""
Map projections on the device: the plane coordinates of the reference's three map products (auromat/draw.py draws them through
Basemap: 'stere' with ellps='WGS84' for drawStereographic / drawStereographicMLatMLT, 'npaeqd' / 'spaeqd' for drawMLatMLTPolar).

Formulas: Snyder, Map Projections - A Working Manual, ch. 21 and 25 (PROJ's ``stere`` and ``aeqd``); the kernels are in
csrc/amt_project.hip, the constants of a projection come from the library's host code (csrc/amt_params.h) and need no GPU.
Angles in degrees, lengths in km, float64.  A point more than 90 degrees from the centre (for the stereographic projection:
on the conformal sphere) is outside the domain of ``forward`` and gives NaN in both outputs, as NaN and infinite inputs do.

There is no CPU fallback: ``forward`` and ``inverse`` run on the GPU, for NumPy arrays (NumPy arrays come back) and for device
tensors (device tensors come back) of any shape.
"""
import ctypes as C

import numpy as np

from .geodesic import wgs84A, wgs84B
from .._native import Context, NativeError, Projection, lib, ptr, to_host

BASEMAP_SPHERE_RADIUS = 6370.997            # km; the sphere Basemap uses when no ellipsoid is given


class _Projection(object):
    """A filled ``amt_projection`` and the two device calls."""

    def __init__(self, params):
        self.params = params

    kind = property(lambda self: self.params.kind)
    lat0 = property(lambda self: self.params.lat0)
    lon0 = property(lambda self: self.params.lon0)

    def _apply(self, name, u, v):
        import torch
        tensors = isinstance(u, torch.Tensor)
        if tensors != isinstance(v, torch.Tensor):
            raise TypeError('both arguments must be NumPy arrays or both device tensors')
        if tensors:
            ctx = Context.current(u.device)
            a, b = ctx.to_device(u), ctx.to_device(v)
        else:
            ctx = Context.current()
            a, b = ctx.to_device(np.asarray(u, dtype=np.float64)), ctx.to_device(np.asarray(v, dtype=np.float64))
        if a.shape != b.shape:
            raise ValueError('shapes differ: {} and {}'.format(tuple(a.shape), tuple(b.shape)))
        out0, out1 = ctx.empty(a.shape), ctx.empty(a.shape)
        ctx.call(name, C.byref(self.params), ptr(a), ptr(b), a.numel(), ptr(out0), ptr(out1))
        if tensors:
            return out0, out1
        return to_host(out0), to_host(out1)

    def forward(self, lat, lon):
        """(x, y) in km of (lat, lon) in degrees; NaN outside the domain"""
        return self._apply('amt_project_forward', lat, lon)

    def inverse(self, x, y):
        """(lat, lon) in degrees of (x, y) in km; lon in [-180, 180)"""
        return self._apply('amt_project_inverse', x, y)


class Stereographic(_Projection):
    """The stereographic projection of the ellipsoid (a, b) centred on (lat0, lon0) with scale 1 at the centre (Basemap / PROJ
    ``stere``); the polar form for a centre within 1e-8 degrees of a pole.  ``b == a``: a sphere."""

    def __init__(self, lat0, lon0, a=wgs84A, b=wgs84B):
        p = Projection()
        if lib().amt_projection_stereographic(float(lat0), float(lon0), float(a), float(b), C.byref(p)) != 0:
            raise ValueError('Stereographic: need |lat0| <= 90, finite arguments and 0 < b <= a; got lat0={!r}, lon0={!r}, '
                             'a={!r}, b={!r}'.format(lat0, lon0, a, b))
        _Projection.__init__(self, p)

    def __repr__(self):
        return 'Stereographic(lat0={!r}, lon0={!r}, a={!r}, e={!r})'.format(self.lat0, self.lon0, self.params.a, self.params.e)


class PolarAzimuthalEquidistant(_Projection):
    """The polar azimuthal equidistant projection of a sphere (Basemap ``npaeqd`` / ``spaeqd``): distances from the pole are
    true; the meridian `lon0` points down (north) or up (south)."""

    def __init__(self, north, lon0=180.0, radius=BASEMAP_SPHERE_RADIUS):
        p = Projection()
        if lib().amt_projection_polar_aeqd(1 if north else 0, float(lon0), float(radius), C.byref(p)) != 0:
            raise ValueError('PolarAzimuthalEquidistant: need a finite lon0 and radius > 0; got lon0={!r}, radius={!r}'.format(
                lon0, radius))
        _Projection.__init__(self, p)

    north = property(lambda self: self.params.mode > 0)

    def __repr__(self):
        return 'PolarAzimuthalEquidistant(north={!r}, lon0={!r}, radius={!r})'.format(self.north, self.lon0, self.params.a)


__all__ = ['Stereographic', 'PolarAzimuthalEquidistant', 'BASEMAP_SPHERE_RADIUS', 'NativeError']
