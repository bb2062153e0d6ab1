"""
TEST INFRASTRUCTURE — step 9 of world -> pixel (include/auromat_hip.h, "inverse georeferencing": the lens of a raw frame applied
after the camera model) as a statement over the arithmetic interface of tests/_inverse_oracle.py (mpmath at 50 digits, Python
floats), the point cases of the `_lens` point entry points and the hand-made plans of the `_lens` gather entry points.

The statement of one point: steps 1-8 by `_inverse_oracle.inverse` on the camera of the CORRECTED, cropped frame; its OUTSIDE
flag (and only that) is dropped; where it has a pixel (X, Y): Xf = X + crop_x, Yf = Y + crop_y, u = (Xf - cx) norm, v = (Yf - cy)
norm with the constants of the raw frame (`_lens_oracle.constants`), r = sqrt(u^2 + v^2).  The point is kept iff r < r_fold
(`fold_radius` below: `_lens_oracle.fold_radius`, 0 where the slope is not positive at the centre, NaN with a NaN coefficient: no
point is kept then); else LENS_FOLD, no pixel.  (xs, ys) = (cx + u g / norm, cy + v g / norm), (Xf, Yf) itself where g = 1; OUTSIDE iff (xs, ys) is not in
[-0.5, W - 0.5] x [-0.5, H - 0.5] of the raw frame W x H.
"""
import functools
import math

import numpy as np

import _inverse_cases as IC
import _inverse_oracle as O
import _lens_cases as LC
import _lens_oracle as LO

LENS_FOLD = 32
NO_PIXEL = O.NO_PIXEL | LENS_FOLD
AMBIGUOUS = IC.AMBIGUOUS        # relative distance from the fold radius, pixels from the raw frame's edge, and _inverse_oracle's margin

CAMERAS = ('cd-rotation-37', 'limb-below-1', 'dateline', 'zen-ARC', 'sip-2')
MODELS = ('identity', 'poly3', 'poly5', 'ptlens', 'outside', 'magnify', 'fold', 'nan')
CROP, GROW = (5, 3), (11, 7)    # crop_x, crop_y; raw frame = camera frame + GROW
KINDS = {'none': 0, 'poly3': 1, 'poly5': 2, 'ptlens': 3}

# ptlens models for the fold radius: (a, b, c) -> what the slope 4 a r^3 + 3 b r^2 + 2 c r + (1 - a - b - c) does for r > 0
PTLENS_FOLDS = {
    'two-roots': (0.2, -0.7, 0.1),          # falls through zero and comes back: two positive roots, the smaller one counts
    'no-root': (0.01, 0.02, 0.03),          # every coefficient positive: never folds
    'centre': (0.5, 0.4, 0.3),              # 1 - a - b - c < 0: folded at the centre already
    'centre-zero': (0.5, 0.25, 0.25),       # 1 - a - b - c = 0 exactly
    'cubic-down': (-0.05, 0.01, 0.02),      # leading coefficient negative: one root, on the last, unbounded piece
    'quadratic': (0.0, -0.2, 0.05),         # a = 0: the slope is a parabola
    'linear': (0.0, 0.0, -0.3),             # a = b = 0: a line
}


def lens_of(cam, model, crop):
    """dict(name, model, params, width, height [raw], crop (left, top, w, h) or None) of model `model` of _lens_cases.MODELS on
    camera `cam`: cropped, the camera's frame is the window at CROP of a corrected frame GROW larger; else that frame itself"""
    name, params = LC.MODELS[model]
    w, h = cam['width'], cam['height']
    if crop:
        return dict(name=model, model=name, params=tuple(params), width=w + GROW[0], height=h + GROW[1], crop=CROP + (w, h))
    return dict(name=model, model=name, params=tuple(params), width=w, height=h, crop=None)


def native_lens(lens):
    from auromat_amd._native import LensModel
    m = LensModel()
    m.kind, m.width, m.height = KINDS[lens['model']], lens['width'], lens['height']
    if lens['crop']:
        m.crop_x, m.crop_y, m.crop_width, m.crop_height = lens['crop']
    m.k[:] = (list(lens['params']) + [0.0, 0.0, 0.0])[:3]
    return m


def native(cam, lens):
    """(amt_frame_params with the RAW frame's size, amt_zenithal_wcs of the corrected frame or None, amt_lens_model)"""
    p, z = IC.native(cam)
    p.width, p.height = lens['width'], lens['height']
    return p, z, native_lens(lens)


def slope0(model, params):
    return LO.radial_poly(model, list(params))[1]


@functools.lru_cache(maxsize=None)
def fold_radius(model, params):
    """r_fold as an mpf; math.inf: never; 0: folded at the centre; NaN: a NaN coefficient"""
    if any(math.isnan(k) for k in params):
        return float('nan')
    if not slope0(model, params) > 0:
        return 0.0
    r = LO.fold_radius(model, list(params))
    return math.inf if r is None else r


def step9(xp, lens, X, Y):
    """step 9 for a pixel (X, Y) of the cropped corrected frame -> (xs, ys, flags [LENS_FOLD, OUTSIDE], margin)"""
    cx, cy, norm = (xp.num(v) for v in LO.constants(lens['width'], lens['height']))
    left, top = lens['crop'][:2] if lens['crop'] else (0, 0)
    rf = fold_radius(lens['model'], lens['params'])
    if isinstance(rf, float) and math.isnan(rf):
        return xp.nan, xp.nan, LENS_FOLD, float('inf')
    Xf, Yf = X + left, Y + top
    u, v = (Xf - cx) * norm, (Yf - cy) * norm
    r = xp.sqrt(u * u + v * v)
    margin = float('inf')
    if rf == 0.0:
        return xp.nan, xp.nan, LENS_FOLD, margin
    if rf != math.inf:
        rfx = float(rf) if xp is O.F64 else +rf              # (an mpf, at the precision fold_radius found it with)
        margin = abs(float((r - rfx) / rfx))
        if not r < rfx:
            return xp.nan, xp.nan, LENS_FOLD, margin
    k = [xp.num(c) for c in lens['params']]
    if lens['model'] == 'poly3':
        g = (1 - k[0]) + k[0] * r * r
    elif lens['model'] == 'poly5':
        g = 1 + k[0] * r * r + k[1] * r ** 4
    elif lens['model'] == 'ptlens':
        g = k[0] * r ** 3 + k[1] * r * r + k[2] * r + (1 - k[0] - k[1] - k[2])
    else:
        g = 1 + 0 * r
    # (a factor of exactly 1 gives the coordinate itself: in float64 (a n) / n need not round back to a)
    xs, ys = (Xf, Yf) if g == 1 else (cx + u * g / norm, cy + v * g / norm)
    W, H = lens['width'], lens['height']
    margin = min(margin, abs(float(xs + 0.5)), abs(float(xs - (W - 0.5))), abs(float(ys + 0.5)), abs(float(ys - (H - 0.5))))
    flags = 0 if (xs >= -0.5 and xs <= W - 0.5 and ys >= -0.5 and ys <= H - 0.5) else O.OUTSIDE
    return xs, ys, flags, margin


def inverse_lens(xp, cam, lens, frame, c0, c1, first=None):
    """the statement of steps 1-9 for one point -> dict(x, y, elev, flags, margin); `first`: the result of steps 1-8 if at hand"""
    r = dict(first if first is not None else O.inverse(xp, cam, frame, c0, c1))
    r['flags'] &= ~O.OUTSIDE
    if r['flags'] & O.NO_PIXEL:
        return r
    xs, ys, fl, margin = step9(xp, lens, r['x'], r['y'])
    r.update(x=xs, y=ys, flags=r['flags'] | fl, margin=min(r['margin'], margin))
    return r


@functools.lru_cache(maxsize=None)
def _steps_1_to_8(camera, frame_name):
    """the mpmath results (mpf x, y kept) of steps 1-8 for a camera's own points of one frame"""
    cam, pts = IC.by_name(camera), IC.points(camera)[frame_name]
    code = dict(IC.FRAMES)[frame_name]
    return [O.inverse(O.MP(), cam, code, a, b) for a, b in zip(pts['c0'], pts['c1'])]


@functools.lru_cache(maxsize=None)
def points(camera, model, crop, frame_name):
    """dict(c0, c1, x, y, elev, flags, margin [arrays], sure [bool: the flags are certain in float64]) of a point case"""
    cam, pts = IC.by_name(camera), IC.points(camera)[frame_name]
    lens = lens_of(cam, model, crop)
    code = dict(IC.FRAMES)[frame_name]
    res = [inverse_lens(O.MP(), cam, lens, code, a, b, first) for a, b, first in zip(pts['c0'], pts['c1'], _steps_1_to_8(camera, frame_name))]
    out = {k: np.array([float(r[k]) for r in res], dtype=np.float64) for k in ('x', 'y', 'elev', 'margin')}
    out['flags'] = np.array([r['flags'] for r in res], dtype=np.uint8)
    out['sure'] = out['margin'] >= AMBIGUOUS
    out.update(c0=pts['c0'], c1=pts['c1'], lens=lens)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def point_cases():
    return [(c, m, crop, f) for c in CAMERAS for m in MODELS for crop in (False, True) for f, _ in IC.FRAMES]


# ---- gather: hand-made plans --------------------------------------------------------------------------------------------------------
# boxes of 40 x 70 cells at 10 px / deg over the part of the footprints of gm-a and gm-b that holds the frames' centres (the only
# part that the model 'magnify' leaves inside the raw frame): latitude / longitude, and MLat / SM longitude
GRID_BOX = (54.0, 58.0, 21.0, 28.0)
GRID_BOX_SM = (52.0, 56.0, 112.0, 119.0)


def grid_40x70(sm=False):
    from auromat_amd.resample import cached_grid
    la0, la1, lo0, lo1 = GRID_BOX_SM if sm else GRID_BOX
    g = cached_grid((10.0, 10.0), la0 + 0.01, la1 + 0.09, lo0 + 0.01, lo1 + 0.09)
    assert (g.ny, g.nx) == (40, 70), (g.ny, g.nx)
    return g


def raw_image(lens, dtype=np.uint8, channels=3, seed=3):
    rng = np.random.RandomState(seed)
    shape = (lens['height'], lens['width'], channels)
    if np.dtype(dtype) == np.float32:
        return (rng.uniform(-1.0, 1.0, shape) * 1000.0).astype(np.float32)
    return rng.randint(0, int(LO.SAMPLE_MAX[np.dtype(dtype)]) + 1, size=shape).astype(dtype)


def member(camera, model=None, crop=False, dtype=np.uint8, channels=3, seed=3, min_elevation=None, center_mask=None):
    """a member dict of a gather plan (params, zenithal, lens, min_elevation, center_mask, image) for a camera of
    tests/_gather_mosaic_cases.py with the lens `model` (None: no lens, the image is the camera's own frame)"""
    import _gather_mosaic_cases as GC
    cam = GC.by_name(camera)
    lens = lens_of(cam, model or 'identity', crop and model is not None)
    p, z, ln = native(cam, lens)
    return dict(params=p, zenithal=z, lens=ln if model is not None else None, min_elevation=min_elevation, center_mask=center_mask,
                image=raw_image(lens, dtype, channels, seed), lens_case=lens, altitude=cam['altitude'])


def plan_of(members, rule=1, grid=None):
    """a gather mosaic plan (as resample.gather_mosaic_plan makes them) of hand-made members on the 40 x 70 grid"""
    return dict(grid=grid or grid_40x70(), contains_pole=False, contains_discontinuity=False, altitude=members[0]['altitude'],
                rule=rule, members=list(members), identifiers=['m%d' % i for i in range(len(members))])


def member_plan(plan, i):
    """the gather_plan of member i alone on the plan's grid"""
    m = plan['members'][i]
    return dict(grid=plan['grid'], contains_pole=plan['contains_pole'], contains_discontinuity=plan['contains_discontinuity'],
                altitude=plan['altitude'], params=m['params'], zenithal=m['zenithal'], lens=m['lens'],
                min_elevation=m['min_elevation'], center_mask=m['center_mask'])
