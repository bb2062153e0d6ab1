"""
Constructed cases for the lens kernels (tests/test_lens_cpu.py checks the cases themselves, tests/test_gpu_lens_cells.py runs
them): models, frame shapes, image types and contents, each chosen for a way the kernels can go wrong.
"""
import functools

import numpy as np

import _lens_oracle as O

TILE = 32           # output tile of the remap kernel (AMT_LENS_TILE)
WINDOW = 48         # its staging window, source pixels per side

# name: (model, parameters); no round coefficients: with them linear taps give fractions such as k/200, which hit x.5 exactly.
#   |g - 1| at the corner of a 2:1 frame (r^2 = 4.9) is given for the realistic ones.
MODELS = {
    'identity': ('poly3', (0.0,)),                       # every coordinate its own pixel: the image comes back bit for bit
    'poly3': ('poly3', (-0.01237,)),                     # 0.048
    'poly5': ('poly5', (0.00613, 0.00059)),             # 0.044
    'ptlens': ('ptlens', (0.00211, -0.01013, 0.00397)),  # 0.014, not monotonic in r
    'outside': ('poly3', (0.2031,)),                     # g > 1 beyond r = 1: border pixels sample outside the frame
    'magnify': ('poly5', (3.017, 0.0)),                  # g = 1.75 at r = 0.5, 4 at r = 1: a tile's taps overflow the window
    'fold': ('poly3', (-0.4519,)),                       # d(r g)/dr = 0 at r = 1.035: no inverse beyond rd = 1.0017
    'nan': ('poly3', (float('nan'),)),
}
REALISTIC = ('poly3', 'poly5', 'ptlens')
# models whose slope d(ru g)/dru stays >= 0.1 over every frame below: the inverse is compared to 1e-9 px there
WELL_CONDITIONED = ('identity', 'poly3', 'poly5', 'ptlens', 'outside', 'magnify')

# (width, height): one pixel; smaller than the 8-tap window; exactly one tile; one tile + 1 each way; several tiles, odd, 2:1
SHAPES = ((1, 1), (7, 5), (TILE, TILE), (TILE + 1, TILE + 1), (131, 67))

DTYPES = (np.uint8, np.uint16, np.float32)
CHANNELS = (1, 3, 4)


@functools.lru_cache(maxsize=None)
def image(w, h, c, dtype, content, seed=0):
    """(h, w, c) image: 'random' seeded samples over the type's range (float32: [0, 4096)); 'step' a vertical 0 / max edge off
    the middle, so that the Lanczos overshoot clips at both ends"""
    dtype = np.dtype(dtype)
    top = O.SAMPLE_MAX.get(dtype, 4096.0)
    if content == 'random':
        rng = np.random.default_rng([seed, w, h, c, dtype.itemsize])
        im = rng.integers(0, int(top) + 1, size=(h, w, c)).astype(dtype) if dtype != np.float32 else \
            (rng.random((h, w, c)) * top).astype(np.float32)
    else:
        assert content == 'step'
        im = np.zeros((h, w, c), dtype=dtype)
        im[:, (2 * w) // 5:] = top
    im.setflags(write=False)
    return im


def remap_cases():
    """(id, model name, (w, h), channels, dtype, content, interpolation)"""
    cases = []

    def add(model, shape, c, dtype, content, interp):
        case = ('%s-%dx%d-c%d-%s-%s-%s' % (model, shape[0], shape[1], c, np.dtype(dtype).name, content, interp),
                model, shape, c, dtype, content, interp)
        if case[0] not in [k[0] for k in cases]:
            cases.append(case)

    for model in MODELS:                                  # every model on every shape
        for shape in SHAPES:
            add(model, shape, 3, np.uint16, 'random', 'lanczos4')
    for model in MODELS:                                  # the 2 x 2 taps
        for shape in ((7, 5), (TILE + 1, TILE + 1), (131, 67)):
            add(model, shape, 3, np.uint16, 'random', 'linear')
    for model in ('poly3', 'outside', 'magnify'):         # every image type
        for dtype in DTYPES:
            for c in CHANNELS:
                add(model, (131, 67), c, dtype, 'random', 'lanczos4')
    for dtype in DTYPES:                                  # overshoot at an edge, clipped at both ends
        for model in ('identity', 'poly5'):
            add(model, (131, 67), 3, dtype, 'step', 'lanczos4')
        add('poly5', (TILE + 1, TILE + 1), 1, dtype, 'step', 'linear')
    return cases


@functools.lru_cache(maxsize=None)
def remap_reference(case_id):
    """(image, exact values (h, w, c), support, magnitudes for float32 images or None) of a remap case, computed once"""
    case = {c[0]: c for c in remap_cases()}[case_id]
    _, model, (w, h), c, dtype, content, interp = case
    im = image(w, h, c, dtype, content)
    name, params = MODELS[model]
    xy = O.forward_grid(name, list(params), w, h)
    values, support = O.sample(im, xy[..., 0], xy[..., 1], interp)
    mag = O.sample(im, xy[..., 0], xy[..., 1], interp, absolute=True)[0] if im.dtype == np.float32 else None
    for a in (values, support) + ((mag,) if mag is not None else ()):
        a.setflags(write=False)
    return im, values, support, mag


def coords_cases():
    """(id, model name, (w, h), crop or None, corner)"""
    cases = []
    for model in MODELS:
        for shape in SHAPES:
            for corner in (False, True):
                cases.append(('%s-%dx%d-%s' % (model, shape[0], shape[1], 'corner' if corner else 'centre'), model, shape, None, corner))
    cases.append(('poly5-131x67-crop-corner', 'poly5', (131, 67), (2, 1, 128, 64), True))
    cases.append(('ptlens-131x67-crop-centre', 'ptlens', (131, 67), (2, 1, 128, 64), False))
    return cases


def undistort_cases():
    """as coords_cases, on the shapes whose mpmath reference stays quick (a few thousand roots in all)"""
    cases = []
    for model in MODELS:
        for shape in ((1, 1), (7, 5), (TILE + 1, TILE + 1)):
            cases.append(('%s-%dx%d-corner' % (model, shape[0], shape[1]), model, shape, None, True))
    for model in ('poly3', 'fold'):
        cases.append(('%s-131x67-centre' % model, model, (131, 67), None, False))
    cases.append(('ptlens-33x33-crop-corner', 'ptlens', (TILE + 1, TILE + 1), (0, 0, 32, 32), True))
    cases.append(('outside-7x5-crop-centre', 'outside', (7, 5), (1, 0, 5, 5), False))
    return cases


@functools.lru_cache(maxsize=None)
def undistort_reference(case_id):
    """(coordinates, slope, distance of the nearest lattice point from the fold) of an undistort case, computed once"""
    _, model, (w, h), crop, corner = {c[0]: c for c in undistort_cases()}[case_id]
    name, params = MODELS[model]
    out, slope, nearest = O.inverse_grid(name, list(params), w, h, crop, corner)
    out.setflags(write=False)
    return out, slope, nearest
