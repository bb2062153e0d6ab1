"""Image file reading under the reference's name (auromat/util/image.py:17-39, which goes through skimage.io)."""
import numpy as np


def loadImage(imagePath):
    """
    Return the RGB image in its native range ([0, 255] for uint8, [0, 65535] for uint16), shape (height, width, 3);
    grey images are repeated over the three channels, an alpha channel is ignored.  ``.npy`` arrays are returned as
    stored; everything else is read with Pillow.  Not meant for RAW files (the reference says the same: develop them
    with rawpy first).
    """
    if imagePath.lower().endswith('.npy'):
        rgb = np.load(imagePath)
    else:
        try:
            from PIL import Image
        except ImportError:
            raise NotImplementedError('Reading ' + imagePath + ' needs Pillow; pass the image as an array instead')
        with Image.open(imagePath) as im:
            if im.mode in ('I;16', 'I;16B', 'I;16L', 'I'):
                rgb = np.asarray(im).astype(np.uint16)
            else:
                if im.mode not in ('RGB', 'L'):
                    im = im.convert('RGB')
                rgb = np.asarray(im)
    if rgb.ndim == 2:
        rgb = np.repeat(rgb[:, :, None], 3, axis=2)
    rgb = np.ascontiguousarray(rgb[:, :, :3])
    assert rgb.ndim == 3 and rgb.shape[2] == 3, imagePath + '; wrong shape: ' + str(rgb.shape)
    return rgb


def cropWindow(height, width, divisible_by=16):
    """(top, left, cropped height, cropped width) of :func:`croppedImage` for an image of the given size."""
    keep_h, keep_w = (height // divisible_by) * divisible_by, (width // divisible_by) * divisible_by
    assert (height - keep_h) % 2 == 0, 'rows to crop cannot be shared between top and bottom'
    assert (width - keep_w) % 2 == 0, 'columns to crop cannot be shared between left and right'
    return (height - keep_h) // 2, (width - keep_w) // 2, keep_h, keep_w


def croppedImage(im, divisible_by=16):
    """
    The image cropped to the next smaller width and height divisible by `divisible_by`, the same amount taken from
    opposite sides (reference util/image.py:59-72; ``AssertionError`` when an amount to crop is odd, as there).  A view
    of `im`.  The distortion-corrected image of an ISS frame matches its ``.wcs`` only after this crop
    (reference mapping/iss.py:242).
    """
    top, left, h, w = cropWindow(im.shape[0], im.shape[1], divisible_by)
    return im[top:top + h, left:left + w]


__all__ = ['loadImage', 'croppedImage', 'cropWindow']
