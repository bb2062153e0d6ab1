"""
Lens distortion correction on the GPU under the reference's names (auromat/util/lensdistortion.py, which goes through
lensfunpy and cv2; the flow of auromat/mapping/iss.py:232-243): the coordinates at which a corrected image samples the raw
frame, the corrected image itself, and — what the reference does not have — where each raw pixel lies in the corrected frame,
so that a raw frame can be georeferenced without resampling it first (``getMapping(..., lens=mod, lensRoute='raw')``).

The models are lensfun's radial ones with the radius in units of half the frame's smaller side, as the reference documents them
(draw.py:1104-1148); ``include/auromat_hip.h`` states them.  lensfun's rescaling by aspect ratio and crop factor is not part
of this: the case covered is :func:`getLensfunModifierFromParams` (crop factor 1, focal length 1).  lensfunpy is not
available to compare against, so AGREEMENT WITH LENSFUN'S OWN OUTPUT IS NOT PINNED: the kernels are tested against a NumPy /
mpmath statement of the above (tests/_lens_oracle.py).  Not built: the EXIF / lensfun database look-up, TCA, vignetting.
"""
import ctypes as C

import numpy as np

from .image import cropWindow, loadImage

MODELS = {'none': (0, 0), 'poly3': (1, 1), 'poly5': (2, 2), 'ptlens': (3, 3)}      # name: (model code, parameter count)
INTERPOLATIONS = {'linear': 0, 'lanczos4': 1}
PATH_AUTO, PATH_STAGED, PATH_GATHER = 0, 1, 2       # AMT_LENS_PATH_*
TILE = 32                                           # AMT_LENS_TILE


def _interpolation(name):
    try:
        return INTERPOLATIONS[name]
    except KeyError:
        raise ValueError('interpolation must be one of %s, not %r' % (sorted(INTERPOLATIONS), name))


def _sample_bytes(dtype):
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.int16), np.dtype(np.float32)):
        raise TypeError('image must be uint8, uint16 or float32, not %s' % dtype)
    return dtype.itemsize


def _image_to_device(ctx, im):
    """-> (contiguous device tensor (h, w, c) holding the image's bytes, numpy dtype to hand back, whether `im` had 2 dimensions)"""
    import torch
    if isinstance(im, torch.Tensor):
        assert im.is_cuda, 'a tensor image must be on the device'
        np_dtype = {torch.uint8: np.uint8, torch.int16: np.uint16, torch.float32: np.float32}.get(im.dtype)
        if np_dtype is None:
            raise TypeError('image tensor must be uint8, int16 (the bits of uint16) or float32, not %s' % im.dtype)
        t = im.contiguous()
    else:
        a = np.ascontiguousarray(im)
        _sample_bytes(a.dtype)
        if not a.flags.writeable:          # torch does not wrap read-only memory silently (np.load(mmap_mode='r') results)
            a = a.copy()
        np_dtype = a.dtype.type if a.dtype != np.int16 else np.uint16
        t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(ctx.device)
    flat = t.dim() == 2
    if flat:
        t = t.unsqueeze(2)
    if t.dim() != 3 or t.shape[2] not in (1, 3, 4):
        raise ValueError('image must be (h, w) or (h, w, c) with c in 1, 3, 4, not %s' % (tuple(t.shape),))
    return t, np_dtype, flat


def _debug(force_path, tiles):
    from .._native import LensDebug
    if force_path is None and tiles is None:
        return None
    d = LensDebug()
    d.force_path = PATH_AUTO if force_path is None else int(force_path)
    d.tile_path = tiles.data_ptr() if tiles is not None else None
    return C.byref(d)


class LensModifier(object):
    """
    What ``lensfunpy.Modifier`` is to the reference's code, for one radial distortion model and frame size.

    :param model: 'poly3', 'poly5', 'ptlens' (or 'none')
    :param params: 1, 2 or 3 coefficients
    :param width, height: size of the raw frame
    :param crop: optional (left, top, width, height) window of the corrected frame that the corrected image is (see
                 :meth:`cropped`); corrected-image coordinates then count from the window's corner
    """

    def __init__(self, model, params, width, height, crop=None):
        if model not in MODELS:
            raise ValueError('unknown distortion model %r (one of poly3, poly5, ptlens)' % (model,))
        params = [float(p) for p in params]
        if len(params) != MODELS[model][1]:
            raise ValueError('model %s takes %d parameter(s), got %d' % (model, MODELS[model][1], len(params)))
        self.model, self.params = model, params
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise ValueError('empty frame')
        if crop is not None:
            crop = tuple(int(v) for v in crop)
            left, top, cw, ch = crop
            if not (cw > 0 and ch > 0 and left >= 0 and top >= 0 and left + cw <= self.width and top + ch <= self.height):
                raise ValueError('crop window %r does not lie in the %d x %d frame' % (crop, self.width, self.height))
        self.crop = crop

    def __repr__(self):
        return 'LensModifier(%r, %r, %d, %d, crop=%r)' % (self.model, self.params, self.width, self.height, self.crop)

    def cropped(self, divisible_by=16):
        """The same lens with the corrected image cropped as :func:`auromat_amd.util.image.croppedImage` crops it."""
        top, left, h, w = cropWindow(self.height, self.width, divisible_by)
        return LensModifier(self.model, self.params, self.width, self.height, crop=(left, top, w, h))

    @property
    def corrected_size(self):
        """(width, height) of the corrected image"""
        return (self.crop[2], self.crop[3]) if self.crop else (self.width, self.height)

    def _native(self):
        from .._native import LensModel
        m = LensModel()
        m.kind, m.width, m.height = MODELS[self.model][0], self.width, self.height
        if self.crop:
            m.crop_x, m.crop_y, m.crop_width, m.crop_height = self.crop
        m.k[:] = (self.params + [0.0, 0.0, 0.0])[:3]
        return m

    # -- coordinates ---------------------------------------------------------------------------------------------
    def forward_coordinates_device(self, corner=False, float32=False):
        """Device tensor (h[+1], w[+1], 2), [x, y]: where each pixel (corner) of the corrected image samples the raw frame."""
        import torch
        from .._native import Context, ptr
        ctx = Context.current()
        w, h = self.corrected_size
        c = 1 if corner else 0
        out = ctx.empty((h + c, w + c, 2))
        out32 = ctx.empty((h + c, w + c, 2), torch.float32) if float32 else None
        ctx.call('amt_lens_coords', C.byref(self._native()), 0, 0, w, h, c, ptr(out), ptr(out32))
        return out32 if float32 else out

    def apply_geometry_distortion(self, float64=False):
        """(h, w, 2) array in [x, y] order: for every pixel of the corrected image the point of the raw frame to sample —
        float32 like lensfunpy's, or float64 as computed."""
        from .._native import to_host
        return to_host(self.forward_coordinates_device(float32=not float64))

    def undistorted_coordinates_device(self, corner=False):
        """Device tensor (height[+1], width[+1], 2): where each pixel (corner) of the RAW frame lies in the corrected image's
        coordinates; NaN where the model cannot be inverted."""
        from .._native import Context, ptr
        ctx = Context.current()
        c = 1 if corner else 0
        out = ctx.empty((self.height + c, self.width + c, 2))
        ctx.call('amt_lens_undistort', C.byref(self._native()), 0, 0, self.width, self.height, c, ptr(out))
        return out

    def undistorted_coordinates(self, corner=False):
        """:meth:`undistorted_coordinates_device` as a float64 array."""
        from .._native import to_host
        return to_host(self.undistorted_coordinates_device(corner))

    # -- images --------------------------------------------------------------------------------------------------
    def remap_device(self, im, interpolation='lanczos4', support=False, force_path=None, tile_path=False):
        """
        The corrected (and cropped) image of the raw frame `im` — an array or a device tensor (h, w[, c]), uint8, uint16
        (tensors: int16 holding the bits) or float32 — as a device tensor of the same kind: one fused kernel, coordinates
        never stored.  A (h, w, 3) uint8 / uint16 result is what ``SequencePipeline.process`` takes as a device-resident image.
        With support=True: (image, uint8 tensor (h, w), 1 where the sampled point lies inside the raw frame).
        force_path / tile_path: see ``amt_lens_debug``; tile_path=True appends the per-tile report to the result.
        """
        import torch
        from .._native import Context, ptr
        ctx = Context.current()
        src, _, flat = _image_to_device(ctx, im)
        if tuple(src.shape[:2]) != (self.height, self.width):
            raise ValueError('image is %d x %d, the lens was set up for %d x %d' % (src.shape[1], src.shape[0], self.width, self.height))
        w, h = self.corrected_size
        dst = torch.empty((h, w, src.shape[2]), dtype=src.dtype, device=src.device)
        sup = torch.empty((h, w), dtype=torch.uint8, device=src.device) if support else None
        tiles = torch.zeros((-(-h // TILE), -(-w // TILE)), dtype=torch.uint8, device=src.device) if tile_path else None
        ctx.call('amt_lens_remap', C.byref(self._native()), ptr(src), src.element_size(), src.shape[2], _interpolation(interpolation),
                 ptr(dst), ptr(sup), _debug(force_path, tiles))
        res = (dst[:, :, 0] if flat else dst,) + ((sup,) if support else ()) + ((tiles,) if tile_path else ())
        return res[0] if len(res) == 1 else res

    def remap(self, im, interpolation='lanczos4', support=False, **debug):
        """:meth:`remap_device` for arrays: array in, array of the same dtype out."""
        from .._native import to_host
        dtype = _host_dtype(im)
        res = self.remap_device(im, interpolation, support, **debug)
        if not isinstance(res, tuple):
            return to_host(res, dtype=dtype)
        return (to_host(res[0], dtype=dtype),) + tuple(to_host(r) for r in res[1:])


def _host_dtype(im):
    import torch
    if isinstance(im, torch.Tensor):
        return {torch.uint8: np.uint8, torch.int16: np.uint16, torch.float32: np.float32}[im.dtype]
    d = np.asarray(im).dtype
    return np.uint16 if d == np.int16 else d.type


def getLensfunModifierFromParams(model, params, width, height):
    """
    :param str model: 'ptlens', 'poly3', or 'poly5'
    :param list params: 1, 2 or 3 parameters, depending on the model
    :raise ValueError: for another model name or a wrong number of parameters
    """
    if model not in ('ptlens', 'poly3', 'poly5'):
        raise ValueError('unknown distortion model %r (one of poly3, poly5, ptlens)' % (model,))
    return LensModifier(model, params, width, height)


def remap(im, coords, interpolation='lanczos4', support=False, force_path=None, tile_path=False):
    """
    ``lensfunpy.util.remap(im, coords)``: `im` (h, w[, c]) sampled at `coords` (H, W, 2) in [x, y] order (float32; float64 is
    rounded to it) -> (H, W[, c]) array of im's dtype, through the sampling function of :meth:`LensModifier.remap`.
    """
    import torch
    from .._native import Context, ptr, to_host
    ctx = Context.current()
    dtype = _host_dtype(im)
    src, _, flat = _image_to_device(ctx, im)
    if isinstance(coords, torch.Tensor):
        xy = coords.to(device=src.device, dtype=torch.float32).contiguous()
    else:
        xy = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.float32)).to(src.device)
    if xy.dim() != 3 or xy.shape[2] != 2:
        raise ValueError('coords must be (H, W, 2), not %s' % (tuple(xy.shape),))
    h, w = int(xy.shape[0]), int(xy.shape[1])
    dst = torch.empty((h, w, src.shape[2]), dtype=src.dtype, device=src.device)
    sup = torch.empty((h, w), dtype=torch.uint8, device=src.device) if support else None
    tiles = torch.zeros((-(-h // TILE), -(-w // TILE)), dtype=torch.uint8, device=src.device) if tile_path else None
    ctx.call('amt_remap_coords', ptr(src), src.shape[1], src.shape[0], src.element_size(), src.shape[2], ptr(xy), w, h,
             _interpolation(interpolation), ptr(dst), ptr(sup), _debug(force_path, tiles))
    out = to_host(dst[:, :, 0].contiguous() if flat else dst, dtype=dtype)
    res = (out,) + ((to_host(sup),) if support else ()) + ((to_host(tiles),) if tile_path else ())
    return res[0] if len(res) == 1 else res


def correctLensDistortion(imagePathOrArray, undistImagePath=None, mod=None, interpolation='lanczos4', **saveImageKws):
    """
    The distortion-corrected image of a file (read by :func:`auromat_amd.util.image.loadImage`) or array; returned, and
    written through Pillow when `undistImagePath` is given (`saveImageKws` go to ``Image.save``: quality, subsampling ...).

    `mod` (a :class:`LensModifier`) is required: the reference's look-up of camera and lens in the lensfun database from the
    file's EXIF tags is not part of this package (there is no database here) -> ``NotImplementedError``.  EXIF tags are NOT
    copied to the written file (the reference does that with exiftool).
    """
    if mod is None:
        raise NotImplementedError('camera / lens look-up from EXIF tags in the lensfun database is not part of auromat_amd: pass '
                                  'mod=getLensfunModifierFromParams(model, params, width, height)')
    im = loadImage(imagePathOrArray) if isinstance(imagePathOrArray, str) else np.asarray(imagePathOrArray)
    out = mod.remap(im, interpolation)
    if undistImagePath is not None:
        from PIL import Image
        Image.fromarray(out).save(undistImagePath, **saveImageKws)
    return out


def lensDistortionPixelDistances(mod, retH=False):
    """
    For every pixel, its distance from the image centre minus that of the point it samples (reference
    util/lensdistortion.py:234-267, whose centre is (width / 2, height / 2), kept here).

    :rtype: ndarray (h, w); with retH: (difference, distance of the pixel, distance of the sampled point)
    """
    xy = np.asarray(mod.apply_geometry_distortion(), dtype=np.float64)
    h, w = xy.shape[:2]
    cx, cy = w / 2, h / 2
    y, x = np.mgrid[0:h, 0:w]
    own = np.hypot(x - cx, y - cy)
    sampled = np.hypot(xy[..., 0] - cx, xy[..., 1] - cy)
    return (own - sampled, own, sampled) if retH else own - sampled


__all__ = ['LensModifier', 'getLensfunModifierFromParams', 'correctLensDistortion', 'remap', 'lensDistortionPixelDistances']
