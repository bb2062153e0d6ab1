"""
TEST INFRASTRUCTURE — cameras, images and mappings for the gather mosaic (amt_gather_mosaic, resampleGatherMosaic).

Small constructed cameras (tests/_camera_cases.camera / finish, as tests/_inverse_cases._zenithal builds its own): 64 x 48 frames
at 0.4 deg / px from the ISS position, looking 72 deg off the nadir — the limb of the 110 km shell runs through the frame, so line-
of-sight elevations go from 0 deg to some 25 deg: gm-a, and gm-b some 450 km to the north-west of it looking at the same region, so
that the footprints overlap in part and each camera is the higher one in a part of the overlap; a 130 x 100 frame of the same kind;
and neighbours of the `dateline` and `pole` cameras aimed a little to the side from the same position (exact ties in the overlap).
At 10 px / deg the grids are a few 32 x 32 tiles on a side.
"""
import numpy as np

import _camera_cases as K
import _inverse_cases as IC
import _inverse_oracle as O
import _lens_oracle as L

_CAMS = {}


def _make():
    if _CAMS:
        return _CAMS
    view = dict(nadir_angle=72.0, scale=0.4, roll=14.0, crpix=(30.3, 25.6))
    made = [K.camera('gm-a', 'gather', 64, 48, azimuth=35.0, **dict(K.ISS, **view)),
            K.camera('gm-b', 'gather', 64, 48, lat=52.5, lon=9.0, height=400.0, azimuth=52.0, **view),
            K.camera('gm-wide', 'gather', 130, 100, azimuth=42.0, nadir_angle=70.0, scale=0.25, roll=-8.0, **K.ISS),
            K.camera('gm-dateline-b', 'gather', 40, 30, lat=20.0, lon=179.8, height=400.0, aim=(20.03, -179.96), roll=5.0),
            K.camera('gm-pole-b', 'gather', 40, 30, lat=89.2, lon=40.0, height=400.0, aim=(89.9, 130.0), scale=0.1, roll=20.0)]
    for c in made:
        _CAMS[c['name']] = K.finish(c)
    return _CAMS


def by_name(name):
    """a camera of this module, or of tests/_inverse_cases.py"""
    cams = _make()
    return cams[name] if name in cams else IC.by_name(name)


def image(cam, dtype=np.uint8, channels=3, seed=3):
    rng = np.random.RandomState(seed)
    shape = (cam['height'], cam['width'], channels)
    if np.dtype(dtype) == np.float32:
        return (rng.uniform(-1.0, 1.0, shape) * 1000.0).astype(np.float32)
    return rng.randint(0, int(L.SAMPLE_MAX[np.dtype(dtype)]) + 1, size=shape).astype(dtype)


def mapping(cam, img=None, lazy_elevation=None, identifier=None):
    """the camera as a mapping: a spacecraft mapping for a plain TAN header, else a direction-array mapping with its header"""
    from auromat_amd.coordinates import wcs
    from auromat_amd.mapping.astrometry import DirectionArrayMapping
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    h = IC.header_of(cam)
    img = image(cam) if img is None else img
    name = identifier or cam['name']
    if O.is_plain_tan(cam):
        m = ArraySpacecraftMapping(h, cam['altitude'], img, cam['cam'], cam['time'], name, fastCenterCalculation=True)
    else:
        dirs = wcs.zenithal_directions_device(h, cam['width'], cam['height'], corner=True)
        m = DirectionArrayMapping(dirs, cam['altitude'], img, cam['cam'], cam['time'], name, cameraHeader=h)
    return m if lazy_elevation is None else m.maskedByElevation(lazy_elevation)


def collection(members, mayOverlap=True, identifier='gm'):
    from auromat_amd.mapping.mapping import MappingCollection
    return MappingCollection(list(members), identifier, mayOverlap=mayOverlap)
