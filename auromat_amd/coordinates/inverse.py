"""
World -> pixel: the Python side of ``amt_world_to_pixel[_lens]`` and ``amt_grid_to_pixel[_lens]`` (include/auromat_hip.h,
"inverse georeferencing", is the statement of what they compute).

A point is ``(c0, c1)`` = (latitude-like, longitude-like) degrees in one of three frames: geodetic latitude / longitude on the
mapping shell, MLat / SM longitude on the shell, or declination / right ascension (a direction).  Every point comes back with
its pixel coordinates (0-based, a pixel's centre at (column, row)), the elevation of its line of sight and a flag byte.

``lens=`` (an ``amt_lens_model``: :class:`auromat_amd._native.LensModel`, e.g. ``LensModifier._native()``): the frame is a raw
frame that still carries its lens distortion, and the camera model belongs to the corrected (cropped) image — step 9 of the
statement.  The coordinates are then those of the raw frame, whose size is the params' ``width`` x ``height``.
"""
import ctypes as C

import numpy as np

from .._ops import Staged, ptr

W2P_GEODETIC, W2P_SM, W2P_J2000 = 0, 1, 2
INVALID, HIDDEN, UNPROJECTABLE, NOT_CONVERGED, OUTSIDE, LENS_FOLD = 1, 2, 4, 8, 16, 32
NO_PIXEL = INVALID | UNPROJECTABLE | NOT_CONVERGED | LENS_FOLD          # xy is NaN exactly where one of these is set
NOT_SEEN = NO_PIXEL | HIDDEN                                  # what the mapping methods mask


def _zen(zenithal):
    return None if zenithal is None else C.byref(zenithal)


def _lens(lens):
    return None if lens is None else C.byref(lens)


def lens_fold_radius(lens):
    """``amt_lens_fold_radius``: the radius (in units of half the frame's smaller side) at which the model of an
    ``amt_lens_model`` folds over; inf where it never does, 0 where it does at the centre, NaN with a NaN coefficient."""
    from .._native import lib
    r = C.c_double()
    if lib().amt_lens_fold_radius(C.byref(lens), C.byref(r)) != 0:
        raise ValueError('amt_lens_fold_radius: unknown lens kind %r' % (lens.kind,))
    return r.value


def world_to_pixel(params, zenithal, frame, c0, c1, elevation=True, lens=None):
    """``amt_world_to_pixel`` (with `lens`: ``amt_world_to_pixel_lens``) on arrays (or device tensors) of any one shape -> ``(xy, elev, flags)``: float64 shape + (2,),
    float64 (None without `elevation`) and uint8 of that shape.  NumPy in, NumPy out; tensors in, tensors out."""
    import torch
    st = Staged(c0, c1)
    a, b = st.inp(c0), st.inp(c1)
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError('the two coordinate arrays differ in shape: %r and %r' % (tuple(a.shape), tuple(b.shape)))
    shape, n = tuple(a.shape), a.numel()
    xy, flags = st.out((n, 2)), st.out((n,), torch.uint8)
    elev = st.out((n,)) if elevation else None
    args = (C.byref(params), _zen(zenithal), int(frame), ptr(a.reshape(-1)), ptr(b.reshape(-1)), n, ptr(xy), ptr(elev), ptr(flags))
    if lens is None:
        st.ctx.call('amt_world_to_pixel', *args)
    else:
        st.ctx.call('amt_world_to_pixel_lens', *(args + (_lens(lens),)))
    return (st.result(xy, shape + (2,)), None if elev is None else st.result(elev, shape),
            st.result(flags, shape, dtype=np.uint8))


def grid_to_pixel(ctx, params, zenithal, frame, latCentres, lonCentres, xy64=False, elevation=True, lens=None):
    """``amt_grid_to_pixel`` (with `lens`: ``amt_grid_to_pixel_lens``) on two device axes -> device tensors ``(xy32 (ny, nx, 2) float32, xy (float64 or None), elev
    (or None), flags (ny, nx) uint8)``."""
    import torch
    ny, nx = latCentres.numel(), lonCentres.numel()
    xy32 = ctx.empty((ny, nx, 2), torch.float32)
    xy = ctx.empty((ny, nx, 2)) if xy64 else None
    elev = ctx.empty((ny, nx)) if elevation else None
    flags = ctx.empty((ny, nx), torch.uint8)
    args = (C.byref(params), _zen(zenithal), int(frame), ptr(latCentres), ny, ptr(lonCentres), nx, ptr(xy32), ptr(xy), ptr(elev),
            ptr(flags))
    if lens is None:
        ctx.call('amt_grid_to_pixel', *args)
    else:
        ctx.call('amt_grid_to_pixel_lens', *(args + (_lens(lens),)))
    return xy32, xy, elev, flags


def sky_params(width=1, height=1):
    """An amt_frame_params block for questions about the sky alone (``world2pix``): a unit sphere seen from its centre, so that
    no direction is unprojectable for want of a camera; the HIDDEN flag of such a call means nothing."""
    from .._native import FrameParams
    p = FrameParams()
    p.width, p.height = int(width), int(height)
    p.cd[:] = [1.0, 0.0, 0.0, 1.0]
    identity = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    p.rot[:], p.m_geo[:], p.m_sm[:] = identity, identity, identity
    p.a = p.b = p.a0 = p.b0 = 1.0
    return p
