"""
``auromat-convert`` on the MI355X path: georeference (and optionally resample) a sequence of frames and write one
CDF or netCDF file per frame — the flag set and the flow of the reference's console script (auromat/cli/convert.py:58-219).

What differs, and why:

* ``--data`` is a directory of frames as ``<id>.wcs`` (an astrometry.net FITS header as 80-column cards, or a ``.json``
  dict of the same cards: ``CRVAL*``, ``CD*``, ``CRPIX*``, ``IMAGEW/H``, ``DATE-OBS`` [+ ``DATESHIF``], ``POS?``
  [+ ``POS?SHIF``]) next to ``<id>.npy`` (uint8 / uint16 array (h, w, 3)) or a developed image file (``<id>.jpg`` /
  ``.png`` / ``.tif`` through Pillow, as the reference's ISS provider caches them).  The reference reads provider archives
  there (ESA ISS ``api.json``, THEMIS ``thg_l1_*`` CDFs): downloads, RAW development and the CDF library are its I/O
  layer, not part of this package — ``--bps``, ``--correctgamma`` and ``--autobright`` belong to that layer and are
  accepted but have nothing to act on.
* ``--format netcdf``: netCDF-4 / HDF5 as the reference's files (:mod:`auromat_amd.export._nc4`) or, with
  ``--netcdf-container classic``, netCDF classic (:mod:`auromat_amd.export._nc3`).  ``--format cdf``: a version-3 CDF laid out
  by :mod:`auromat_amd.export._cdf3` without NASA's CDF library — read that module's header: no CDF library has opened
  these files yet.
* ``--resample`` runs the sequence through the single-pass frame pipeline (:class:`auromat_amd.pipeline.SequencePipeline`,
  grids only: no per-pixel array is ever written or copied to the host): with ``--resolution`` (arcsec / px, the
  reference's flag and default) every frame's px/deg follows from its own bounding box (``plateCarreeResolution``, the
  box-first plan); ``--px-per-deg N`` (an addition) fixes the grid instead.  With several GPUs (``torchrun --nproc-per-node N
  -m auromat_amd.cli.convert``) the frames are sharded over the ranks and every rank writes the files of its own frames.
* ``--statistic median`` (an addition; needs ``--resample``) bins every cell by the median of its pixels instead of their
  mean (:func:`auromat_amd.resample.resampleMedian` / ``resampleMedianMLatMLT``), through the same two routes; the files
  are written exactly as mean grids are.  ``--statistic quantile --quantile Q`` bins by the quantile Q in [0, 1] of a cell's
  pixels in the same way (:func:`auromat_amd.resample.resampleQuantile` / ``resampleQuantileMLatMLT``).
* ``--statistic area`` (an addition; needs ``--resample``) shares every pixel — the quadrilateral of its four corners — among
  the cells it overlaps, weighted with the covered fraction of the cell (:func:`auromat_amd.resample.resampleArea` /
  ``resampleAreaMLatMLT``), through the same two routes: no holes between the pixel centres on fine grids.  ``--min-coverage F``
  (default 0.5, in [0, 1]) masks the cells of which the pixels cover less than F.  The files hold the variables a mean grid's do.
* ``--gather {nearest,linear,lanczos4}`` (an addition; needs ``--resample``, not with a ``--statistic`` other than mean or with
  ``--lens-route raw``) gathers in place of binning: every cell centre of the frame's grid is projected into the image and the image
  is sampled there (:func:`auromat_amd.resample.resampleGather` / ``resampleGatherMLatMLT``; the pipeline route is
  :class:`auromat_amd.pipeline.GatherSequence`, a batch of frames per kernel launch).  ``--supersample N`` (1 ... 8) averages N x N
  sub-samples per cell; ``--min-coverage F`` (in (0, 1], default 0.5) then masks the cells of which fewer are seen.  The files hold
  the variables a mean grid's do.
* ``--lens-model`` / ``--lens-params`` (an addition): the images are RAW-developed frames that have not been corrected for lens
  distortion, while their ``.wcs`` files were solved on the corrected image, cropped to a multiple of ``--crop-divisible-by`` — the
  state of the ESA ISS archive, whose ``distortion_correction`` entry (reference mapping/iss.py:233-237) is honoured when it is
  found in ``metadata.json`` or a frame's ``<id>.json`` and no flag is given.  ``--lens-route resample`` (default) corrects and
  crops every image on the GPU (:meth:`auromat_amd.util.lensdistortion.LensModifier.remap_device`) and goes on as ever;
  ``--lens-route raw`` maps the uncorrected pixels themselves (``getMapping(..., lensRoute='raw')``), through the mapping classes.
  ``--lens-route fused`` (only with ``--gather``) builds the same raw-route mappings and gathers them through the lens
  (``resampleGather`` / ``resampleGatherMLatMLT``): the uncorrected image is interpolated once, no corrected image is made.
"""
from __future__ import print_function

import argparse
import os
import sys
from datetime import datetime, timedelta

import numpy as np
import numpy.ma as ma

description = 'Georeference frames on the GPU, optionally resample them, and store them as CDF or netCDF files.'

epilog = '''
Resample on the geomagnetic grid with the reference's resolution rule:
auromat-convert --data frames/ --format netcdf --resample --resolution 80

Resample a long sequence on a fixed 0.1 degree geographic grid, as fast as the GPU goes:
auromat-convert --data frames/ --format netcdf --resample --grid geo --px-per-deg 10

Gather instead of binning, 4 x 4 sub-samples per cell (no holes on fine grids, no aliasing on coarse ones):
auromat-convert --data frames/ --format netcdf --resample --gather linear --supersample 4

Don't store pixel corner coordinates:
auromat-convert --data frames/ --format netcdf --without-bounds

CDF files (version 3, laid out without NASA's CDF library), MLat/MLT coordinates only:
auromat-convert --data frames/ --format cdf --resample --without-geo
'''


class Grid(object):
    geo = 'geo'
    mag = 'mag'


class Format(object):
    cdf = 'cdf'
    netcdf = 'netcdf'


def date(s):
    return datetime.strptime(s, '%Y-%m-%dT%H:%M:%S')


def getParser():
    parser = argparse.ArgumentParser(prog='auromat-convert', epilog=epilog, description=description,
                                     formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--data', help='Data directory, by default the current directory: <id>.wcs (or <id>.json) '
                                       'header files next to <id>.npy (or .jpg / .png / .tif) images.', default=os.getcwd())
    period = parser.add_argument_group('period', 'These arguments optionally specify which data to convert.')
    period.add_argument('--start', help='UTC start date, format 2000-01-01T12:00:00', type=date)
    period.add_argument('--end', help='UTC end date (inclusive)', type=date)
    mappingArgs = parser.add_argument_group('mapping')
    mappingArgs.add_argument('--altitude', help='Altitude in km onto which to map the images, default is 110km',
                             default=110, type=int)
    mappingArgs.add_argument('--exact-centers', dest='exactCenters', action='store_true',
                             help='Cast a ray through every pixel centre (the reference\'s getMapping default) instead of '
                                  'averaging the four corner hits.')
    mappingArgs.add_argument('--min-elevation', dest='minElevation', type=float, default=-1.0,
                             help='Mask pixels seen under a smaller elevation angle before resampling (an addition: the '
                                  'reference\'s auromat-convert resamples the provider\'s mappings unmasked, cli/convert.py:'
                                  '176-185, and so does this driver by default; the user guide recommends 10 degrees); '
                                  'negative = no mask.')
    esaIssArgs = parser.add_argument_group('ESA ISS data (accepted for compatibility; RAW development is not part of this package)')
    esaIssArgs.add_argument('--bps', help='bits per sample, default is 16', choices=[8, 16], default=16, type=int)
    esaIssArgs.add_argument('--correctgamma', action='store_true')
    esaIssArgs.add_argument('--autobright', action='store_true')
    resampleArgs = parser.add_argument_group('resampling')
    resampleArgs.add_argument('--resample', help='Whether to resample or not', action='store_true')
    resampleArgs.add_argument('--resolution', metavar='RES', help='in arcsec/px, default 100', default=100, type=float)
    resampleArgs.add_argument('--px-per-deg', dest='pxPerDeg', metavar='N', type=float,
                              help='fixed grid resolution in pixels per degree instead of --resolution: the sequence then '
                                   'runs through the single-pass frame pipeline')
    resampleArgs.add_argument('--grid', help='The grid which will be regular after resampling. Default is MLat/MLT grid. '
                                             'Use geo for geographical grid.', default=Grid.mag, choices=[Grid.geo, Grid.mag])
    resampleArgs.add_argument('--statistic', choices=['mean', 'median', 'quantile', 'area'], default='mean',
                              help='How the pixels of a grid cell are combined, default mean; median is robust to stars, city '
                                   'lights and hot pixels; quantile takes --quantile; area weights every pixel with the part of '
                                   'the cell that its footprint covers and leaves no holes between pixel centres on fine grids '
                                   '(see --min-coverage); all but mean need --resample')
    resampleArgs.add_argument('--quantile', metavar='Q', type=float,
                              help='the quantile of a cell\'s pixels, in [0, 1], for --statistic quantile (numpy.quantile, '
                                   'method linear): 0.25 a background estimate, 0.9 a peak estimate')
    resampleArgs.add_argument('--min-coverage', dest='minCoverage', metavar='F', type=float,
                              help='for --statistic area: a cell is masked unless the pixels cover at least this fraction of it, '
                                   'in [0, 1], default 0.5 (0: any overlap at all)')
    resampleArgs.add_argument('--gather', choices=['nearest', 'linear', 'lanczos4'],
                              help='with --resample: gather in place of binning - every cell centre of the grid is projected into '
                                   'the image and the image is sampled there with this interpolation; no holes at any resolution')
    resampleArgs.add_argument('--supersample', metavar='N', type=int,
                              help='for --gather: N x N sub-samples per cell, averaged, 1 ... 8, default 1; for cells much coarser '
                                   'than a pixel.  --min-coverage F, in (0, 1], then masks the cells of which fewer than that '
                                   'fraction of the sub-samples is seen, default 0.5')
    lensArgs = parser.add_argument_group('lens distortion', 'For images that are not yet corrected for lens distortion (an addition; '
                                         'by default the distortion_correction entry of metadata.json or <id>.json, if any).')
    lensArgs.add_argument('--lens-model', dest='lensModel', choices=['poly3', 'poly5', 'ptlens'],
                          help='lensfun distortion model of the frames')
    lensArgs.add_argument('--lens-params', dest='lensParams', metavar='P', type=float, nargs='+',
                          help='its coefficients: k1 (poly3), k1 k2 (poly5) or a b c (ptlens)')
    lensArgs.add_argument('--lens-route', dest='lensRoute', choices=['resample', 'raw', 'fused'], default='resample',
                          help='resample: correct (Lanczos-4) and crop every image on the GPU first, default; raw: map the '
                               'uncorrected pixels themselves, nothing interpolated; fused (only with --gather): gather through '
                               'the lens - the grid\'s cell centres go through the camera model and the lens model into the '
                               'uncorrected image, which is interpolated once')
    lensArgs.add_argument('--crop-divisible-by', dest='cropDivisibleBy', metavar='N', type=int,
                          help='the .wcs files belong to the corrected image cropped to the next smaller width and height '
                               'divisible by N (16 for the ESA ISS archive); default: not cropped')
    outputArgs = parser.add_argument_group('output')
    outputArgs.add_argument('--out', help='Output directory, by default the "converted" subdirectory of --data')
    outputArgs.add_argument('--overwrite', help='Overwrites existing files.', action='store_true')
    outputArgs.add_argument('--skip', help='Skips already converted files.', action='store_true')
    outputArgs.add_argument('--format', help='Data format of converted files', choices=[Format.cdf, Format.netcdf],
                            required=True)
    outputArgs.add_argument('--netcdf-container', dest='netcdfContainer', choices=['netcdf4', 'classic'], default='netcdf4',
                            help='netCDF files: the netCDF-4 / HDF5 container the reference writes (zlib, one row per chunk; '
                                 'default) or netCDF classic with 64-bit offsets (no compression). Not an option of the '
                                 'reference.')
    outputArgs.add_argument('--without-bounds', dest='withoutBounds', action='store_true',
                            help='Do not include coordinates of pixel corners. If set, then only the pixel center '
                                 'coordinates are written, otherwise both.')
    outputArgs.add_argument('--without-mag', dest='withoutMag', help='Do not include MLat/MLT coordinates.',
                            action='store_true')
    outputArgs.add_argument('--without-geo', dest='withoutGeo', action='store_true',
                            help='Do not include geodetic coordinates. Only usable with CDF output.')
    parser.add_argument('--version', action='version', version='auromat_amd (MI355X)')
    return parser


def parseargs(argv=None):
    parser = getParser()
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        sys.exit(1)
    args = parser.parse_args(argv)
    if not args.out:
        args.out = os.path.join(args.data, 'converted')
    if args.overwrite and args.skip:
        parser.error('only one of --overwrite and --skip is allowed')
    if args.statistic != 'mean' and not args.resample:
        parser.error('--statistic %s needs --resample' % args.statistic)
    if args.statistic == 'quantile':
        if args.quantile is None:
            parser.error('--statistic quantile needs --quantile')
        if not 0.0 <= args.quantile <= 1.0:
            parser.error('--quantile must be in the range [0, 1]')
    elif args.quantile is not None:
        parser.error('--quantile is only usable with --statistic quantile')
    if args.statistic == 'area':
        if args.minCoverage is None:
            args.minCoverage = 0.5
        if not 0.0 <= args.minCoverage <= 1.0:
            parser.error('--min-coverage must be in the range [0, 1]')
    elif args.minCoverage is not None and not args.gather:
        parser.error('--min-coverage is only usable with --statistic area')
    if args.supersample is not None and not args.gather:
        parser.error('--supersample is only usable with --gather')
    if args.gather:
        if not args.resample:
            parser.error('--gather needs --resample')
        if args.statistic != 'mean':
            parser.error('--gather takes the place of binning: not with --statistic %s' % args.statistic)
        if args.lensRoute == 'raw':
            parser.error('--gather needs the inverse of the camera model, which --lens-route raw does not have '
                         '(--lens-route fused gathers through the lens)')
        if args.supersample is None:
            args.supersample = 1
        if not 1 <= args.supersample <= 8:
            parser.error('--supersample must be in the range 1 ... 8')
        if args.minCoverage is not None:
            if args.supersample == 1:
                parser.error('--min-coverage goes with --supersample above 1: one point is sampled per cell')
            if not 0.0 < args.minCoverage <= 1.0:
                parser.error('--min-coverage must be in the range (0, 1] with --gather')
    if args.lensRoute == 'fused' and not args.gather:
        parser.error('--lens-route fused needs --gather: it is the gather that goes through the lens')
    if (args.lensModel is None) != (args.lensParams is None):
        parser.error('--lens-model and --lens-params go together')
    if args.lensModel is not None:
        from ..util.lensdistortion import MODELS
        if len(args.lensParams) != MODELS[args.lensModel][1]:
            parser.error('--lens-model %s takes %d parameter(s)' % (args.lensModel, MODELS[args.lensModel][1]))
    if args.cropDivisibleBy is not None and args.cropDivisibleBy < 1:
        parser.error('--crop-divisible-by must be positive')
    if args.withoutGeo and args.format == Format.netcdf:
        parser.error('--without-geo is only usable with --format cdf')
    if args.format == Format.cdf:
        #  the version-3 container is laid out from the format description; no CDF library has opened such a file yet
        sys.stderr.write('auromat-convert: note: CDF files are written without NASA\'s CDF library and have only been read back by this '
                         'package\'s own reader; validate one with cdflib / pycdf before relying on them\n')
    return args


# ---- input: a directory of headers + arrays ---------------------------------------------------------------------
def read_header(path):
    """A FITS header stored as 80-column ASCII cards (what astrometry.net's .wcs files are) or as JSON -> dict."""
    from ..fits import readHeader
    return readHeader(path)


IMAGE_EXTENSIONS = ('.npy', '.jpg', '.jpeg', '.png', '.tif', '.tiff')


def find_image(data_dir, base):
    """-> path of the image that belongs to header `base` (<base>.npy, or a developed image file as the reference's ISS
    provider keeps next to its .wcs files: <base>.jpg / .png / .tif), None when there is none."""
    for ext in IMAGE_EXTENSIONS:
        for e in (ext, ext.upper()):
            path = os.path.join(data_dir, base + e)
            if os.path.exists(path):
                return path
    return None


def read_image(path, mmap=False):
    """(h, w, 3) uint8 / uint16 array of an image file: .npy as stored, anything else through Pillow (8-bit JPEG / PNG,
    8- or 16-bit TIFF / PNG; grey images are repeated over three channels, an alpha channel is dropped)."""
    if mmap and path.lower().endswith('.npy'):
        return np.load(path, mmap_mode='r')
    from ..util.image import loadImage
    a = loadImage(path)
    if a.dtype not in (np.uint8, np.uint16):
        raise NotImplementedError('unsupported sample type %s in %s' % (a.dtype, path))
    return a


def list_frames(data_dir, start=None, end=None):
    """-> sorted list of (identifier, header dict, image path) within [start, end] by (shifted) photo time."""
    from ..mapping.spacecraft import getPhotoTime
    frames = []
    for name in sorted(os.listdir(data_dir)):
        base, ext = os.path.splitext(name)
        if ext not in ('.wcs', '.json'):
            continue
        img = find_image(data_dir, base)
        if img is None:
            continue
        hdr = read_header(os.path.join(data_dir, name))
        t = getPhotoTime(hdr)
        if t is None:
            continue
        if 'DATESHIF' in hdr:
            t = t + timedelta(seconds=float(hdr['DATESHIF']))
        if (start and t < start) or (end and t > end):
            continue
        frames.append((t, base, hdr, img))
    frames.sort(key=lambda f: f[0])
    return [(b, h, i) for _, b, h, i in frames]


def lens_spec(args, hdr, metadata=None):
    """(model, params) of the lens distortion a frame still carries, or None: the flags, else the ``distortion_correction`` entry
    ({"model": ..., "params": [...]}, the key of the reference's ISS archive, mapping/iss.py:233-237) of the frame's own
    ``<id>.json``, else that of ``metadata.json`` (top level, or under ``sequence_metadata``)."""
    if args.lensModel is not None:
        return args.lensModel, list(args.lensParams)
    entry = hdr.get('distortion_correction')
    if not entry and metadata:
        entry = metadata.get('distortion_correction') or (metadata.get('sequence_metadata') or {}).get('distortion_correction')
    if not entry:
        return None
    return entry['model'], [float(p) for p in entry['params']]


def read_metadata(data_dir):
    """metadata.json of the data directory as a dict, or None"""
    import json
    path = os.path.join(data_dir, 'metadata.json')
    if not os.path.exists(path):
        return None
    with open(path) as fp:
        return json.load(fp)


def lens_of(args, hdr, metadata, width, height):
    """The LensModifier (crop included) for a raw frame of the given size, or None when the frame carries no distortion."""
    spec = lens_spec(args, hdr, metadata)
    if spec is None:
        return None
    from ..util.lensdistortion import getLensfunModifierFromParams
    mod = getLensfunModifierFromParams(spec[0], spec[1], width, height)
    return mod.cropped(args.cropDivisibleBy) if args.cropDivisibleBy else mod


def target_path(args, identifier):
    """-> path to write, or None when the frame is to be skipped; exits like the reference when the file exists."""
    path = os.path.join(args.out, identifier + extension(args))
    if os.path.exists(path):
        if args.skip:
            print('skipping', path)
            return None
        elif args.overwrite:
            os.remove(path)
        else:
            print('The file', path, 'already exists.\nPlease use --skip or --overwrite, or a different output folder.',
                  file=sys.stderr)
            sys.exit(1)
    return path


def extension(args):
    return '.cdf' if args.format == Format.cdf else '.nc'


# ---- the two ways through the GPU ----------------------------------------------------------------------------
def convert_with_classes(args, frames, export):
    """Frame by frame through the mapping classes: the reference's flow, its resolution rule included."""
    from ..mapping.spacecraft import getMapping
    from ..resample import (resample, resampleArea, resampleAreaMLatMLT, resampleGather, resampleGatherMLatMLT, resampleMedian,
                            resampleMedianMLatMLT, resampleMLatMLT, resampleQuantile, resampleQuantileMLatMLT)
    metadata = read_metadata(args.data)
    for identifier, hdr, img_path in frames:
        path = target_path(args, identifier)
        if path is None:
            continue
        img = read_image(img_path)
        mapping = getMapping(img, hdr, altitude=args.altitude, fastCenterCalculation=not args.exactCenters, identifier=identifier,
                             lens=lens_of(args, hdr, metadata, img.shape[1], img.shape[0]),
                             lensRoute='raw' if args.lensRoute == 'fused' else args.lensRoute)     # (fused: a raw-route mapping, gathered)
        if args.resample:
            if args.minElevation >= 0:
                mapping = mapping.maskedByElevation(args.minElevation)
            if args.gather:
                fn = resampleGather if args.grid == Grid.geo else resampleGatherMLatMLT
                mapping = fn(mapping, interpolation=args.gather, supersample=args.supersample, minCoverage=args.minCoverage,
                             **(dict(pxPerDeg=args.pxPerDeg) if args.pxPerDeg else dict(arcsecPerPx=args.resolution)))
            elif args.statistic == 'median':
                fn = resampleMedian if args.grid == Grid.geo else resampleMedianMLatMLT
                mapping = fn(mapping, **(dict(pxPerDeg=args.pxPerDeg) if args.pxPerDeg else dict(arcsecPerPx=args.resolution)))
            elif args.statistic == 'quantile':
                fn = resampleQuantile if args.grid == Grid.geo else resampleQuantileMLatMLT
                mapping = fn(mapping, args.quantile,
                             **(dict(pxPerDeg=args.pxPerDeg) if args.pxPerDeg else dict(arcsecPerPx=args.resolution)))
            elif args.statistic == 'area':
                fn = resampleArea if args.grid == Grid.geo else resampleAreaMLatMLT
                mapping = fn(mapping, minCoverage=args.minCoverage,
                             **(dict(pxPerDeg=args.pxPerDeg) if args.pxPerDeg else dict(arcsecPerPx=args.resolution)))
            else:
                fn = resample if args.grid == Grid.geo else resampleMLatMLT
                mapping = fn(mapping, arcsecPerPx=args.resolution)
        print('storing', path)
        export(path, mapping)


def grid_mapping(res, cam, t, altitude, identifier, magnetic):
    """The resampled grid of one frame (host arrays of the few hundred KB the pipeline returns) as the mapping that
    ``resample`` / ``resampleMLatMLT`` would have returned: a GenericMapping in geodetic coordinates; a grid that is
    regular in (MLat, SM longitude) goes through SM -> GEO like ``convertSMMappingToGeo`` (reference
    mapping.py:1549-1559).  The elevation comes from the 'mean' block or, for median, quantile and area-weighted grids, the
    'median' / 'quantile' / 'area' block; a gathered grid has no block and brings a plain 'elevation' (NaN where masked)."""
    from ..coordinates.transform import smToLatLon
    from ..mapping.mapping import GenericMapping
    lat, lon, lat_c, lon_c = res['lat'], res['lon'], res['lat_c'], res['lon_c']
    if magnetic:
        lat, lon = smToLatLon(lat, lon, t)
        lat_c, lon_c = smToLatLon(lat_c, lon_c, t)
    img = ma.masked_array(res['img'], mask=np.repeat(res['mask'][:, :, None], res['img'].shape[2], 2))
    block = next((res[k] for k in ('mean', 'median', 'quantile', 'area') if k in res), None)
    elevation = res['elevation'] if block is None else block[:, :, -1]
    return GenericMapping(lat, lon, lat_c, lon_c, ma.masked_invalid(elevation), altitude, img, cam, t, identifier)


def host_snapshot(mapping, with_mag):
    """What the exporters read of a mapping, evaluated HERE (the device work of a mapping — MLat/MLT of the grid, the traced
    outline behind the bounding box — stays on the thread that owns the GPU context) and held as plain host arrays: such a
    snapshot can be written by another thread while the next frames are processed."""
    from types import SimpleNamespace
    snap = SimpleNamespace(lats=mapping.lats, lons=mapping.lons, latsCenter=mapping.latsCenter, lonsCenter=mapping.lonsCenter,
                           elevation=mapping.elevation, img=mapping.img, boundingBox=mapping.boundingBox,
                           photoTime=mapping.photoTime, altitude=mapping.altitude, cameraPosGCRS=mapping.cameraPosGCRS,
                           metadata=mapping.metadata, identifier=mapping.identifier)
    if with_mag:
        snap.mLatMlt, snap.mLatMltCenter = mapping.mLatMlt, mapping.mLatMltCenter
    return snap


def convert_with_pipeline(args, frames, export):
    """The whole sequence through the single-pass frame pipeline — at a fixed px/deg (--px-per-deg) or, the reference's
    flags, at --resolution arcsec per pixel, where every frame's px/deg follows from its own bounding box (the box-first plan
    of SequencePipeline(arcsecPerPx=...)) —; this rank's share of the frames."""
    import torch
    import torch.distributed as dist
    from ..mapping.spacecraft import frame_inputs
    from ..pipeline import GatherSequence, SequencePipeline
    from ..resample import grid_coordinates
    from ..sequence import shard
    from .._native import to_host
    distributed = 'WORLD_SIZE' in os.environ and int(os.environ['WORLD_SIZE']) > 1
    rank, world = 0, 1
    if distributed:
        rank, world = int(os.environ.get('RANK', '0')), int(os.environ['WORLD_SIZE'])
        # the "file exists, neither --skip nor --overwrite" exit of the reference is decided for ALL frames on EVERY rank
        # before the process group exists: every rank leaves together and nobody waits in a collective for a rank that
        # has gone (a check per rank's own share left the others in dist.barrier() until the launcher killed them)
        if not args.skip and not args.overwrite:
            for identifier, _, _ in frames:
                path = os.path.join(args.out, identifier + extension(args))
                if os.path.exists(path):
                    print('The file', path, 'already exists.\nPlease use --skip or --overwrite, or a different output folder.',
                          file=sys.stderr)
                    sys.exit(1)
        # (AMT_CONVERT_ONE_GPU=1 AMT_CONVERT_BACKEND=gloo: several ranks on one GPU, for rehearsals — the ranks only meet in the
        # closing barrier)
        torch.cuda.set_device(0 if os.environ.get('AMT_CONVERT_ONE_GPU') else int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group(os.environ.get('AMT_CONVERT_BACKEND', 'nccl'))
        rank, world = dist.get_rank(), dist.get_world_size()
    todo = []
    for identifier, hdr, img_path in [frames[k] for k in shard(len(frames), rank, world)]:
        path = target_path(args, identifier)
        if path is not None:
            todo.append((identifier, hdr, img_path, path))
    if todo:
        first = read_image(todo[0][2], mmap=True)
        magnetic = args.grid == Grid.mag
        metadata = read_metadata(args.data)
        # frames that still carry their lens distortion are corrected and cropped on the device and handed to the pipeline as
        # device-resident images of the corrected size (the lens is not part of the native runner)
        lenses = [lens_of(args, hdr, metadata, first.shape[1], first.shape[0]) for _, hdr, _, _ in todo]
        if any(m is not None for m in lenses) and any(m is None or m.corrected_size != lenses[0].corrected_size for m in lenses):
            raise NotImplementedError('a sequence of which only some frames carry a lens distortion')
        size = lenses[0].corrected_size if lenses[0] is not None else (first.shape[1], first.shape[0])
        if args.gather:
            # gathering in place of binning: a batch of frames per launch of the gather kernel (GatherSequence)
            seq = GatherSequence(size[0], size[1], nchan=first.shape[2], img_dtype=first.dtype, altitude=args.altitude,
                                 min_elevation=args.minElevation if args.minElevation >= 0 else None, pxPerDeg=args.pxPerDeg or 25,
                                 arcsecPerPx=None if args.pxPerDeg else args.resolution, magnetic=magnetic,
                                 interpolation=args.gather, supersample=args.supersample, minCoverage=args.minCoverage)
        else:
            seq = SequencePipeline(size[0], size[1], nchan=first.shape[2], img_dtype=first.dtype,
                                   altitude=args.altitude, fast=not args.exactCenters,
                                   min_elevation=args.minElevation if args.minElevation >= 0 else None,
                                   pxPerDeg=args.pxPerDeg or 10, magnetic=magnetic, keep_coordinates=False,
                                   arcsecPerPx=None if args.pxPerDeg else args.resolution, statistic=args.statistic,
                                   quantile=args.quantile, minCoverage=args.minCoverage)

        def feed():
            # decoding a 12 Mpx JPEG takes ~100 ms of host time, the GPU 0.2 ms per frame: images are read ahead on a
            # few threads (Pillow and NumPy release the GIL while they decode / load)
            from collections import deque
            from concurrent.futures import ThreadPoolExecutor
            ahead = max(1, int(os.environ.get('AMT_CONVERT_READ_AHEAD', '8')))
            from .._native import host_threads
            with ThreadPoolExecutor(max_workers=host_threads(min(ahead, 8))) as pool:
                pending = deque()
                it = iter(todo)
                for item in it:
                    pending.append((item, pool.submit(read_image, item[2])))
                    if len(pending) >= ahead:
                        break
                while pending:
                    (identifier, hdr, img_path, path), fut = pending.popleft()
                    nxt = next(it, None)
                    if nxt is not None:
                        pending.append((nxt, pool.submit(read_image, nxt[2])))
                    cam, t = frame_inputs(hdr)
                    img = fut.result()
                    if lenses[0] is not None:
                        img = lens_of(args, hdr, metadata, img.shape[1], img.shape[0]).remap_device(img, 'lanczos4')
                        torch.cuda.current_stream().synchronize()       # (the pipeline reads it on streams of its own)
                    yield hdr, cam, t, img

        metas = [frame_inputs(hdr) for _, hdr, _, _ in todo]
        results = seq.process(feed(), keep_on_device=True)
        # the files are written by a few threads (deflate releases the interpreter lock; AMT_CONVERT_WRITERS=0: in line): a
        # resampled grid takes 6 ms to compute and 20-odd to compress and lay out
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        from .._native import host_threads
        n_writers = max(0, int(os.environ.get('AMT_CONVERT_WRITERS', '4')))
        n_writers = host_threads(n_writers) if n_writers else 0          # (several ranks on one host share its cores)
        writers = ThreadPoolExecutor(max_workers=n_writers) if n_writers else None
        written = deque()
        try:
            for k, ((identifier, hdr, img_path, path), (cam, t), res) in enumerate(zip(todo, metas, results)):
                if res is None:
                    why = 'a pole in view: --resolution yields no longitude resolution for' if \
                        seq.plans[k] == 'pole-without-resolution' else 'no valid pixel in'
                    print(why, identifier, file=sys.stderr)
                    continue
                host = dict(res)
                host.update(grid_coordinates(res))
                # the name of the block: 'mean', 'median', 'quantile' or 'area'; a gathered grid brings a plain elevation
                stat = 'elevation' if args.gather else args.statistic
                host[stat] = to_host(res[stat])
                host.update(img=to_host(res['img'], dtype=first.dtype), mask=to_host(res['mask']).astype(bool))
                print('storing', path)
                mapping = grid_mapping(host, cam, t, args.altitude, identifier, magnetic)
                if writers is None:
                    export(path, mapping)
                    continue
                written.append(writers.submit(export, path, host_snapshot(mapping, not args.withoutMag)))
                while len(written) > 2 * n_writers:
                    written.popleft().result()
            while written:
                written.popleft().result()                # (an exporter's exception surfaces here)
        finally:
            if writers is not None:
                writers.shutdown(wait=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None):
    args = parseargs(argv)
    from functools import partial
    frames = list_frames(args.data, args.start, args.end)
    if not frames:
        raise NotImplementedError('No <id>.wcs / <id>.json + <id>.npy (or .jpg / .png / .tif) frames found in ' + args.data)
    if args.format == Format.cdf:
        from ..export.cdf import write
        export = partial(write, includeBounds=not args.withoutBounds, includeMagCoords=not args.withoutMag,
                         includeGeoCoords=not args.withoutGeo)
    else:
        from ..export.netcdf import write
        export = partial(write, includeBounds=not args.withoutBounds, includeMagCoords=not args.withoutMag,
                         includeGeoCoords=not args.withoutGeo,
                         format='NETCDF4' if args.netcdfContainer == 'netcdf4' else 'NETCDF3_64BIT')
    os.makedirs(args.out, exist_ok=True)
    # --resample, with the reference's --resolution (default 100 arcsec per pixel) or with --px-per-deg: the sequence pipeline;
    # without --resample the frames are exported as they are, through the mapping classes (AMT_CONVERT_CLASSES=1 sends
    # resampling runs that way too: the reference's flow frame by frame, for A/B runs)
    # (the raw lens route maps through direction arrays, which the sequence pipeline's runner does not take)
    metadata = read_metadata(args.data)
    raw_route = args.lensRoute in ('raw', 'fused') and any(lens_spec(args, hdr, metadata) for _, hdr, _ in frames)
    if args.resample and not raw_route and not os.environ.get('AMT_CONVERT_CLASSES'):
        convert_with_pipeline(args, frames, export)
    else:
        convert_with_classes(args, frames, export)
    print('Done.')


if __name__ == '__main__':
    main()
