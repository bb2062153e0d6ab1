"""
The one thing needed to look at a resampled mapping: its image as a PNG.  Everything else the reference's auromat/draw.py does
(graticules, coastlines, labels, figures) is matplotlib's business and not built here; the map products themselves are arrays,
see auromat_amd.resample.resampleStereographic, resampleStereographicMLatMLT, resampleMLatMLTPolar and resampleScanLines.
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
