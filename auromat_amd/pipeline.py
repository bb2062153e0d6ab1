"""
Device-resident frame pipeline: georeference -> (mask by elevation) -> bounding box -> grid ->
binned mean, i.e. what ``resample(getMapping(...).maskedByElevation(e), pxPerDeg=...)`` does in the
reference (spacecraft.py:380-426, mapping.py:845-864, resample.py:73-157) on pre-allocated HBM buffers.

Two execution plans give identical results:

* two-pass (always available):
    1. amt_georef_frame        corner/centre lat, lon, elevation (+ MLat/MLT) and the bounding-box reduction
                               of the corners that survive the elevation mask
    2. amt_bin_frame           re-reads centre lat/lon/elevation + image, bins (elevation mask on the fly)
    3. amt_bin_frame_finalize  mean / rounding / flip into the output layout
  The host reads the 8 bounding-box doubles between 1 and 2 and lays out the grid
  (reference resample.py:220-241,281-299).

* single-pass (``fuse=True``; geodetic or MLat/MLT grids, also across the 180 deg discontinuity; not with a pole
  in view): the binning happens inside the georeferencing kernel, so nothing is read back.  Because the grid
  depends on the bounding box the kernel itself produces, an estimate of the box comes first — a cheap pre-pass
  (every 16th corner ray) or, in a sequence, the exact box of the previous frame — the kernel bins into a
  *superset* grid aligned to the same global nodes, and the exact window is cropped by the finalise kernel once
  the exact box is known.  If the exact box is not inside the superset the two-pass plan runs instead.  The
  orchestration is native code (include/auromat_hip.h: amt_pipe_*); :class:`FramePipeline` binds it.

:class:`SequencePipeline` software-pipelines a sequence of frames over several frame buffers (what bench.py times
and ``auromat_amd.sequence`` shards over GPUs); the mapping classes give the same results lazily.
"""
import ctypes as C
import os

import numpy as np

from .frame import FrameData, PaddedFrameData, has_array
from .mapping.astrometry import frame_params, pole_in_view, run_frame
from .mapping.mapping import bounding_box_from_reduction, grid_box_from_reduction, mlt_to_sm_lon
from .resample import (ThreadPipes, _px_per_deg, area_overflow_error, cached_grid, grid_coordinates, min_coverage_weight, quantile_list,
                       resample_frame, resample_frame_area, resample_frame_median, resample_frame_quantile)
from ._native import PIPE_MAX_EDGE_PIXELS, Context, GeorefOut, PipeResult, RunConfig, RunFrame, RunResult, ptr, to_host

NEG_INF = float('-inf')
_Box8 = C.c_double * 8                 # a box reduction as the library takes it


class EmptyFrame(ValueError):
    """No pixel of the frame is valid (the reference's ValueError of maskedByElevation, mapping.py:858-859)."""


class _GridView(object):
    """
    Output grid as laid out by the native driver (amt_grid): sizes, steps and first centres are available
    at once; everything else (coordinate arrays) comes from the equal :class:`auromat_amd.resample._Grid`,
    built when first asked for.
    """

    def __init__(self, g, pxPerDeg, box):
        self.nx, self.ny = g.nx, g.ny
        self.latStep, self.lonStep = g.lat_step, g.lon_step
        self.lat0, self.lon0 = g.lat_center_first, g.lon_center_first
        self._pxPerDeg, self._box, self._full = pxPerDeg, box, None

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        if self._full is None:
            self._full = cached_grid(self._pxPerDeg, *self._box)
        return getattr(self._full, name)


def _frame_block(g, pxPerDeg, bbox, wrapped, pole, altitude, grids, o8, images, ob, img16):
    """One finished frame as it lies in memory — mean | count from double `o8` of `grids`, image | mask from byte `ob` of
    `images` — and its grid `g` (amt_grid, laid out from the reduction `bbox`) -> (result dict without the arrays, packed = mean
    and count as one tensor, mean, count, img, mask, the byte behind the mask)."""
    import torch
    ny, nx = g.ny, g.nx
    n = ny * nx
    packed = grids[o8:o8 + 5 * n]
    mean = grids[o8:o8 + 4 * n].view(ny, nx, 4)
    count = grids[o8 + 4 * n:o8 + 5 * n].view(ny, nx)
    om = ob + (6 if img16 else 3) * n
    img = images[ob:om]
    img = (img.view(torch.int16) if img16 else img).view(ny, nx, 3)
    mask = images[om:om + n].view(ny, nx)
    # (a pole plan's grid is in rotated coordinates; BoundingBox.containsDiscontinuity is true for every box with a pole in
    # it, reference mapping.py:200-206)
    out = dict(has_elev=True, grid=_GridView(g, pxPerDeg, grid_box_from_reduction(bbox, wrapped)), contains_pole=pole,
               contains_discontinuity=wrapped or pole, altitude=altitude)
    return out, packed, mean, count, img, mask, om + n


def earth_rows_of(params, height, min_elevation=None):
    """(r0, r1): the pixel rows of a camera frame's image that a kernel can need (amt_georef_image_rows): outside of them no ray
    reaches the shell or — with `min_elevation` > 0 — no pixel reaches that elevation, and only pixels that survive
    maskedByElevation are ever binned (reference mapping.py:845-864, resample.py:315-321).  Conservative."""
    from . import _native
    r0, r1 = C.c_int32(0), C.c_int32(0)
    me = NEG_INF if min_elevation is None else float(min_elevation)
    _native.lib().amt_georef_image_rows(C.byref(params), me, C.byref(r0), C.byref(r1))
    return max(0, r0.value), min(int(height), r1.value)


def uploaded_rows(rows, height):
    """the rows of a host image :meth:`FramePipeline.set_image` sends for ``rows`` = (r0, r1): the band when it is worth
    it (under nine tenths of the image), else everything"""
    if rows is not None and 0 <= rows[0] < rows[1] <= height and (rows[1] - rows[0]) < 0.9 * height:
        return rows[0], rows[1]
    return 0, int(height)


class FramePipeline(object):
    def __init__(self, width, height, nchan=3, img_dtype=np.uint16, device=None, with_mag=False, alloc_image=True,
                 alloc_coords=True, with_geo=True, padded=False):
        import torch
        self.ctx = ctx = Context.current(device)
        self.width, self.height = int(width), int(height)
        h, w = self.height, self.width
        # padded=True: the per-pixel coordinate arrays are kept in strip-padded rows (amt_georef_out.row_layout: the layout the
        # row kernel writes 8-12 % faster) and compacted into the reference's contiguous arrays when somebody asks for one
        # (PaddedFrameData); for pipelines whose arrays mostly stay where they are — a sequence that bins in the same kernel
        self.padded = bool(padded)
        fd = self.fd = PaddedFrameData(ctx, h, w) if self.padded else FrameData(ctx, h, w)
        self.with_mag = with_mag
        # with_geo=False (needs with_mag): "MLat / MLT only" — the pipeline keeps mlat, mlt, mlat_c, mlt_c and the elevation,
        # which is all resampleMLatMLT consumes (reference resample.py:63-71, mapping.py:1519-1547), and the single-pass
        # launch on the (MLat, SM longitude) grid runs the kernel variant that skips the geodetic half of the arithmetic
        # and its four stores (k_georef_rows<SECOND = 4>).  The geodetic arrays are allocated, and the frame georeferenced
        # again into all nine, only when a frame takes the two-pass plan or somebody asks for them (coordinates()).
        self.with_geo = bool(with_geo) or not with_mag
        self._out = GeorefOut()
        # alloc_coords=False ("grids only"): the single-pass plan then writes no per-pixel coordinate arrays at all (its
        # kernel bins every pixel as soon as its coordinates exist; 480 MB per frame of stores fall away) and the
        # arrays are only allocated, and the frame georeferenced again into them, when a frame has to take the
        # two-pass plan (pole in view, ...) or somebody asks for them
        self._coords_valid = False
        self._kept_valid = False    # the arrays a with_geo=False pipeline keeps hold the last frame
        if alloc_coords:
            self._alloc_coords()
        fd.bbox = ctx.empty((8,))
        fd.img_dtype = np.dtype(img_dtype)
        self._img_torch_dtype = torch.uint8 if fd.img_dtype == np.uint8 else torch.int16
        self._img_shape = (h, w, nchan)
        # alloc_image=False: the caller aliases a device-resident image before the first frame (use_image)
        fd.img = ctx.empty(self._img_shape, self._img_torch_dtype) if alloc_image else None
        self._img_own = fd.img
        self._bbox_host = torch.empty(8, dtype=torch.float64, pin_memory=True)
        self._bbox_event = torch.cuda.Event()
        self._driver = None         # amt_pipe handle of the single-pass plan (created on first use)
        self._fin_stream = None     # the driver's finalise stream as torch sees it (see _finalize_fused)
        self._fused = None          # single-pass launch in flight: its px/deg, later its amt_pipe_result
        self._pole = 0
        self.last_plan = None       # 'single-pass' or 'two-pass': what the last resample() did
        # keep_on_device results of the single-pass plan are produced on the driver's own stream; by default the
        # current stream is ordered behind them at once.  A pipelined caller sets defer_join and calls join()
        # once before it consumes the results, which keeps the stream of big kernels free of wait packets.
        self.defer_join = False
        # the stream that will consume keep_on_device results when it is not the one current at finalisation (a pipelined
        # caller sets it: the outputs are then recorded for it once, at allocation, instead of array by array afterwards)
        self.consumer_stream = None
        # rows of ONE frame sharded over several ranks (auromat_amd.sequence.resample_frame_sharded): an object with
        # box(red) -> red (the 8-number bounding-box reduction combined over the ranks), acc(tensor) (the integer
        # accumulators summed over the ranks, in place) and pole (pole in view of the WHOLE frame); None = whole frames
        self.shard = None
        self.params = None
        self.altitude = None
        self.min_elevation = None
        # corner directions of the last frame when they came from the caller ((h + 1, w + 1, 3) float64 device tensor, J2000;
        # the directions-in form of the pipeline, reference astrometry.py:49-64 with any camera model) instead of the TAN model
        self._dirs = None
        self._out.bbox = fd.bbox.data_ptr()

    def _alloc_coords(self, full=False):
        """Allocate the per-pixel arrays the pipeline keeps (`full`: the geodetic ones of a with_geo=False pipeline too)."""
        fd, ctx = self.fd, self.ctx
        h, w = self.height, self.width

        def alloc(*names):
            for k in names:
                if self.padded:
                    fd.alloc_padded(k)
                else:
                    setattr(fd, k, ctx.empty((h + 1, w + 1) if k in ('lat', 'lon', 'mlat', 'mlt') else (h, w)))

        if not has_array(fd, 'elev'):
            alloc('elev')
            if self.with_mag:
                alloc('mlat', 'mlt', 'mlat_c', 'mlt_c')
        if (full or self.with_geo) and not has_array(fd, 'lat'):
            alloc('lat', 'lon', 'lat_c', 'lon_c')
        self._set_out(full)

    def _set_out(self, full=False):
        """Output pointers of the next launch: every array the pipeline holds, the geodetic ones of a with_geo=False
        pipeline only with `full` (a NULL output is not computed: amt_georef_out)."""
        fd, out = self.fd, self._out
        out.row_layout = 1 if self.padded else 0          # AMT_ROWS_STRIP_PADDED / AMT_ROWS_CONTIGUOUS
        for k in FrameData.COORDS:
            t = fd.padded(k) if self.padded else getattr(fd, k)
            if k in ('lat', 'lon', 'lat_c', 'lon_c') and not (full or self.with_geo):
                t = None
            setattr(out, k, None if t is None else t.data_ptr())

    def _has_all(self):
        return has_array(self.fd, 'elev') and has_array(self.fd, 'lat')

    def _written(self):
        """A launch is about to write the coordinate buffers: contiguous copies of padded arrays are stale."""
        if self.padded:
            self.fd.touch()

    def coordinates(self):
        """Make sure the per-pixel coordinate arrays of the last frame exist (grids-only pipelines compute them on
        demand: one more run of the georeferencing kernel) -> the FrameData."""
        if not self._coords_valid:
            self._alloc_coords(full=True)
            self.ctx.bind()
            self._out.bbox_min_elevation = NEG_INF if self.min_elevation is None else float(self.min_elevation)
            self._written()
            if self._dirs is not None:
                self.ctx.call('amt_georef_frame_dirs', C.byref(self.params), ptr(self._dirs), C.byref(self._out))
            else:
                self.ctx.call('amt_georef_frame', C.byref(self.params), C.byref(self._out))
            self._set_out()
            self.fd.corner_mask = self.fd.center_mask = None
            self._coords_valid = self._kept_valid = True
        return self.fd

    def __del__(self):
        if getattr(self, '_driver', None):
            try:
                self.ctx._lib.amt_pipe_destroy(self._driver)
            except Exception:
                pass
            self._driver = None

    # -- inputs ---------------------------------------------------------------------------------
    def set_image(self, img, rows=None):
        """Copy an (h, w, c) host image (or device tensor of the same bytes) into the frame buffer.  A pinned host
        tensor of the buffer's dtype (uint16 images as their int16 bits) is copied asynchronously on the current
        stream.  `rows` = (r0, r1), host images only: only that band of rows crosses the link — the rows a camera frame's
        kernels can need (:meth:`earth_rows`); the buffer's other rows are UNDEFINED afterwards (they keep whatever an earlier
        frame left there): the buffer is the binning kernel's input, not a copy of the image for anybody else."""
        import torch
        if self.fd.img is not self._img_own or self._img_own is None:
            # the buffer aliased a caller's device image (use_image): copy into a buffer of our own
            if self._img_own is None:
                self._img_own = self.ctx.empty(self._img_shape, self._img_torch_dtype)
            self.fd.img = self._img_own
        band = uploaded_rows(rows, self.height) != (0, self.height)
        if isinstance(img, torch.Tensor) and not img.is_cuda and img.is_pinned() and img.dtype == self.fd.img.dtype:
            src = img.reshape(self.fd.img.shape)
            if band:
                self.fd.img[rows[0]:rows[1]].copy_(src[rows[0]:rows[1]], non_blocking=True)
            else:
                self.fd.img.copy_(src, non_blocking=True)
            return
        if isinstance(img, torch.Tensor):
            t = self.ctx.to_device(img, self.fd.img_dtype)
            self.fd.img.copy_(t.reshape(self.fd.img.shape))
            return
        a = np.ascontiguousarray(img, dtype=self.fd.img_dtype)
        assert a.size == self.fd.img.numel(), 'image of the wrong size'
        self.ctx.bind()
        if band:
            a = a.reshape(self._img_shape)
            self.ctx.upload(a[rows[0]:rows[1]], self.fd.img[rows[0]:rows[1]])
            return
        self.ctx.upload(a, self.fd.img)          # through page-locked staging pieces (see Context.upload)

    def earth_rows(self, params, min_elevation=None):
        """(r0, r1): the pixel rows of a camera frame's image a kernel can need (:func:`earth_rows_of`)."""
        return earth_rows_of(params, self.height, min_elevation)

    def forget_inputs(self):
        """Drop what the pipeline holds of its caller's last frame (a 288 MB direction array of a DirectionArrayMapping, the
        parameters): a cached pipeline must not keep them alive.  The frame's arrays can then no longer be computed on demand."""
        self._dirs = None
        self._coords_valid = self._kept_valid = False

    def use_image(self, img):
        """Use a device-resident image of the buffer's layout ((h, w, c) uint8, or uint16 bits as int16) in place:
        nothing is copied; the caller keeps the tensor alive and unchanged until the frame's results exist."""
        assert img.is_cuda and img.dtype == self._img_torch_dtype and img.is_contiguous() and \
            img.numel() == int(np.prod(self._img_shape)), 'device image of the wrong layout'
        self.fd.img = img.view(self._img_shape)

    def is_resident_image(self, img):
        import torch
        return isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == self._img_torch_dtype and \
            img.is_contiguous() and img.numel() == int(np.prod(self._img_shape))

    # -- single-pass plan (native driver, include/auromat_hip.h amt_pipe_*) ----------------------
    def _pipe(self):
        if self._driver is None:
            handle = C.c_void_p()
            self.ctx.call('amt_pipe_create', C.byref(handle))
            self._driver = handle
        return self._driver

    def _pcall(self, name, *args):
        # amt_pipe_* take the driver handle (not the context) as their first argument
        self.ctx.check(getattr(self.ctx._lib, name)(self._pipe(), *args))

    def _finalize_stream(self):
        """The driver's finalise stream, wrapped for torch: tensors that the finalise kernel writes are allocated for
        it (amt_pipe_finalize_stream)."""
        import torch
        if self._fin_stream is None:
            handle = C.c_void_p()
            self._pcall('amt_pipe_finalize_stream', C.byref(handle))
            self._fin_stream = torch.cuda.ExternalStream(handle.value, device=self.ctx.device)
        return self._fin_stream

    def join(self):
        """Order the current stream behind the single-pass driver's finalise kernels (see amt_pipe_join)."""
        if self._driver is not None:
            self.ctx.bind()
            self._pcall('amt_pipe_join')

    def start_coarse(self, params, min_elevation, magnetic=False, hint=None, dirs=None):
        """
        Enqueue the coarse bounding-box pre-pass for `params` (asynchronous, on the driver's own stream), or, with
        `hint` (the 8 reduction numbers of a neighbouring frame's exact box), skip it: amt_pipe_coarse_hint.
        `dirs`: the frame's corner directions come from the caller (amt_pipe_coarse_dirs samples that array).
        """
        if hint is not None:
            self._pcall('amt_pipe_coarse_hint', hint if isinstance(hint, _Box8) else _Box8(*hint), 1 if magnetic else 0)
        elif dirs is not None:
            self._pcall('amt_pipe_coarse_dirs', C.byref(params), ptr(dirs),
                        NEG_INF if min_elevation is None else float(min_elevation), 1 if magnetic else 0)
        else:
            self._pcall('amt_pipe_coarse', C.byref(params),
                        NEG_INF if min_elevation is None else float(min_elevation), 1 if magnetic else 0)

    def box_first(self, params, min_elevation, magnetic=False):
        """
        The box pass of the box-first plan (amt_pipe_launch_box): the frame kernel without any output array, image or
        binning -> the exact 8-number bounding-box reduction of the corners that survive maskedByElevation, in (lat, lon) or,
        with `magnetic`, (MLat, SM longitude); [7] = 1 when a pole of those coordinates is in view (camera model).  One
        host synchronisation.  Raises EmptyFrame when no pixel is valid.
        """
        self.ctx.bind()
        self._pcall('amt_pipe_launch_box', C.byref(params), NEG_INF if min_elevation is None else float(min_elevation),
                    1 if magnetic else 0)
        res = PipeResult()
        self._pcall('amt_pipe_wait', C.byref(res))
        if res.status == 2 or res.bbox[6] == 0:
            self.last_plan = 'empty'
            raise EmptyFrame('minElevation=' + str(min_elevation) + ' would mask all pixels!')
        return list(res.bbox)

    def resolution_from_box(self, params, min_elevation, arcsecPerPx, magnetic=False):
        """
        `resample(mapping, arcsecPerPx=R)` derives px/deg from the mapping's own bounding box (reference resample.py:36-61,
        104-107): the box pass, plateCarreeResolution on its BoundingBox -> ((latPxPerDeg, lonPxPerDeg), reduction).  The
        reduction is what the following single-pass launch takes as its estimate (`hint`), so that launch needs no
        pre-pass and its superset grid always holds the exact one.
        """
        from .resample import plateCarreeResolution
        red = self.box_first(params, min_elevation, magnetic)
        return plateCarreeResolution(bounding_box_from_reduction(red), arcsecPerPx), red

    def _wait_fused(self):
        """amt_pipe_wait once per launch -> the amt_pipe_result."""
        f = self._fused
        if f['result'] is None:
            res = PipeResult()
            self._pcall('amt_pipe_wait', C.byref(res))
            f['result'] = res
        return f['result']

    # -- stages ---------------------------------------------------------------------------------
    def georef(self, wcsHeader, altitude, cameraPosGCRS, photoTime, fast=True, min_elevation=10.0, params=None,
               fuse_pxPerDeg=None, coarse_started=False, fuse_magnetic=False, dirs=None, pole_in_view=-1):
        """
        Stage 1.  `params` (an amt_frame_params made by :func:`frame_params`) skips the host set-up.
        `fuse_pxPerDeg` = (latPxPerDeg, lonPxPerDeg) selects the single-pass plan for that resolution, on the
        geodetic grid or, with `fuse_magnetic`, on the (MLat, SM longitude) grid of resampleMLatMLT.
        `dirs`: (h + 1, w + 1, 3) float64 device tensor of corner directions (J2000) that replaces the TAN camera model
        (`params` then carries camera position, shell and rotations only; fast centres); `pole_in_view` 0 / 1 is the caller's
        knowledge about a pole of the grid's coordinates in such a frame, -1 = unknown (amt_pipe_launch_dirs).
        """
        assert wcsHeader is None or (wcsHeader['IMAGEW'], wcsHeader['IMAGEH']) == (self.width, self.height)
        p = params if params is not None else frame_params(wcsHeader, altitude, cameraPosGCRS, photoTime, fast,
                                                           magnetic=self.with_mag)
        fd = self.fd
        self.ctx.bind()      # enqueue on whatever stream torch has current now
        out = self._out
        min_elev = NEG_INF if min_elevation is None else float(min_elevation)
        if dirs is not None:
            assert dirs.is_cuda and dirs.is_contiguous() and tuple(dirs.shape) == (self.height + 1, self.width + 1, 3), \
                'one direction per pixel corner, (h + 1, w + 1, 3) float64 on the device'
        self._written()
        if fuse_pxPerDeg is not None and fd.nchan == 3 and (self.with_mag or not fuse_magnetic):
            # coarse pre-pass (unless already enqueued), superset grid, fused kernel, bbox copy: all in the driver
            mag = 1 if fuse_magnetic else 0
            if not coarse_started:
                self.start_coarse(p, min_elevation, mag, dirs=dirs)
            out.altitude = float(altitude)
            if dirs is not None:
                self._pcall('amt_pipe_launch_dirs', C.byref(p), ptr(dirs), C.byref(out), fd.img.data_ptr(),
                            fd.img_dtype_code, min_elev, float(fuse_pxPerDeg[0]), float(fuse_pxPerDeg[1]), int(pole_in_view), mag)
            else:
                self._pcall('amt_pipe_launch', C.byref(p), C.byref(out), fd.img.data_ptr(),
                            fd.img_dtype_code, min_elev, float(fuse_pxPerDeg[0]), float(fuse_pxPerDeg[1]), -1, mag)
            self._launched(p, altitude, min_elevation, dirs, tuple(fuse_pxPerDeg), mag, pole_in_view)
            return fd
        self.params, self.altitude, self.min_elevation, self._dirs = p, altitude, min_elevation, dirs
        self._alloc_coords(full=True)
        self._coords_valid = self._kept_valid = True
        self._fused = None
        self._pole = None                                # decided lazily in bounding_box()
        out.bbox_min_elevation = min_elev
        if dirs is not None:
            self.ctx.call('amt_georef_frame_dirs', C.byref(p), ptr(dirs), C.byref(out))
        else:
            self.ctx.call('amt_georef_frame', C.byref(p), C.byref(out))
        self._set_out()
        fd.corner_mask = fd.center_mask = None
        # the 8 reduction doubles travel to pinned host memory right behind the kernel; the event lets
        # bounding_box() wait for exactly this point while later launches keep the GPU busy
        self._bbox_host.copy_(fd.bbox, non_blocking=True)
        self._bbox_event.record()
        return fd

    @staticmethod
    def georef_many(pipes, params, altitudes, min_elevation, fuse_pxPerDeg, fuse_magnetic=False, dirs=None, pole_in_view=-1):
        """
        The single-pass launch of :meth:`georef` for up to AMT_PIPE_MAX_BATCH pipelines at once (one frame each, coarse
        pre-pass already started): ONE launch of the big kernel covers all frames (amt_pipe_launch_many_res).  `dirs`: one
        (h + 1, w + 1, 3) direction tensor per frame instead of the camera model (amt_pipe_launch_dirs_many).
        """
        n = len(pipes)
        ctx = pipes[0].ctx
        ctx.bind()
        min_elev = NEG_INF if min_elevation is None else float(min_elevation)
        mag = 1 if fuse_magnetic else 0
        if not isinstance(altitudes, (list, tuple)):
            altitudes = [altitudes] * n
        for q, altitude in zip(pipes, altitudes):
            q._out.altitude = float(altitude)
            q._written()
        handles = (C.c_void_p * n)(*[q._pipe() for q in pipes])
        pp = (C.c_void_p * n)(*[C.addressof(p) for p in params])
        oo = (C.c_void_p * n)(*[C.addressof(q._out) for q in pipes])
        ii = (C.c_void_p * n)(*[q.fd.img.data_ptr() for q in pipes])
        # one resolution for all frames, or a list with one (latPxPerDeg, lonPxPerDeg) per frame (arcsecPerPx: every frame's
        # px/deg follows from its own bounding box)
        per_frame = isinstance(fuse_pxPerDeg, list)
        ppd = [tuple(v) for v in fuse_pxPerDeg] if per_frame else [tuple(fuse_pxPerDeg)] * n
        if dirs is not None:
            assert not per_frame and len(dirs) == n
            for d, q in zip(dirs, pipes):
                assert d.is_cuda and d.is_contiguous() and tuple(d.shape) == (q.height + 1, q.width + 1, 3)
            dd = (C.c_void_p * n)(*[d.data_ptr() for d in dirs])
            ctx.check(ctx._lib.amt_pipe_launch_dirs_many(handles, n, pp, dd, oo, ii, pipes[0].fd.img_dtype_code, min_elev,
                                                         float(ppd[0][0]), float(ppd[0][1]), int(pole_in_view), mag))
        else:
            la, lo = (C.c_double * n)(*[float(v[0]) for v in ppd]), (C.c_double * n)(*[float(v[1]) for v in ppd])
            ctx.check(ctx._lib.amt_pipe_launch_many_res(handles, n, pp, oo, ii, pipes[0].fd.img_dtype_code, min_elev, la, lo, -1, mag))
        for i, (q, p, altitude, v) in enumerate(zip(pipes, params, altitudes, ppd)):
            q._launched(p, altitude, min_elevation, None if dirs is None else dirs[i], v, mag, pole_in_view)

    def _launched(self, p, altitude, min_elevation, dirs, pxPerDeg, mag, pole_in_view):
        """What a single-pass launch leaves on the pipeline: the frame it holds, the launch in flight and which arrays it wrote."""
        self.params, self.altitude, self.min_elevation, self._dirs = p, altitude, min_elevation, dirs
        self._fused = dict(pxPerDeg=pxPerDeg, magnetic=bool(mag), result=None, pole_in_view=int(pole_in_view))
        self.fd.corner_mask = self.fd.center_mask = None
        self._coords_valid = has_array(self.fd, 'lat') and self.with_geo
        self._kept_valid = has_array(self.fd, 'elev')

    def bounding_box(self):
        """Waits for the fused reduction of the last georef() -> BoundingBox; ValueError if nothing is valid."""
        if self._dirs is not None:
            # caller-supplied directions: no camera model to project a pole through — the corner quads decide
            # (amt_bbox_corners counts those that wind around a pole, reference geodesic.py:183 / mapping.py:705-721)
            if self._fused is not None:
                self._wait_fused()
            self.coordinates()
            red = self._reduce_bbox(self.fd.lat, self.fd.lon)
        elif self._fused is not None and not self._fused['magnetic'] and not \
                (self._wait_fused().fused and self._wait_fused().bbox[7]):
            red = np.array(self._wait_fused().bbox[:])
        elif self._fused is not None:
            # the driver reduced the box over (MLat, SM longitude) or, pole in view, over the rotated corners; the
            # geodetic one comes from the corner arrays
            self.coordinates()
            red = self._reduce_bbox(self.fd.lat, self.fd.lon)
            red[7] = 1.0 if pole_in_view(self.params, self.min_elevation) else 0.0
        else:
            self._bbox_event.synchronize()
            red = self._bbox_host.numpy().copy()
            if self.shard is not None:
                red = self.shard.box(red)
                self._pole = bool(self.shard.pole)
            if self._pole is None:
                # pole containment from the camera model (the kernel does not count pole quads)
                self._pole = pole_in_view(self.params, self.min_elevation)
            red[7] = 1.0 if self._pole else 0.0
        if red[6] == 0:
            self.last_plan = 'empty'
            raise EmptyFrame('minElevation=' + str(self.min_elevation) + ' would mask all pixels!')
        return bounding_box_from_reduction(red)

    def _reduce_bbox(self, lat, lon):
        """8-number bounding-box reduction (see amt_bbox_corners) of corner arrays `lat`, `lon` of this frame over
        the corners that survive maskedByElevation(min_elevation); host array."""
        import torch
        fd = self.fd
        thr = NEG_INF if self.min_elevation is None else self.min_elevation
        cmask = (~(fd.elev >= thr)).to(torch.uint8)
        corner = torch.isnan(fd.lat).to(torch.uint8)
        red = self.ctx.empty((8,))
        # exact centres: a centre also needs its four corners (mapping.py:1093-1101); masking by elevation first
        # and reconciling once gives the same masks as the reference's sanitize -> mask -> sanitize order
        self.ctx.call('amt_sanitize_masks', ptr(corner), ptr(cmask), None, fd.height, fd.width,
                      1 if self.params.fast_center else 0)
        self.ctx.call('amt_bbox_corners', ptr(lat), ptr(lon), ptr(corner), ptr(cmask), fd.height, fd.width, ptr(red))
        return to_host(red)

    def fused_ready(self, pxPerDeg, magnetic):
        """The amt_pipe_result of the single-pass launch in flight when the driver can finalise it for this resolution
        (None: whatever resolution it was launched with) and grid (waits for the frame's bounding box), else None (no such
        launch, or the frame needs the general path)."""
        if self._fused is None or self._fused['magnetic'] != bool(magnetic) or \
                (pxPerDeg is not None and self._fused['pxPerDeg'] != tuple(pxPerDeg)):
            return None
        res = self._wait_fused()
        return res if res.status == 0 else None

    def _fused_nbytes(self, res):
        """Bytes of one frame's outputs (mean | count | image | mask), padded to 256."""
        n = res.grid.ny * res.grid.nx
        return (40 * n + 3 * n * (2 if self.fd.img_dtype_code == 2 else 1) + n + 255) & ~255

    def _fused_alloc(self, nbytes, cur):
        """Output memory for the finalise stream -> (bytes, the same as float64, the same as the image's type)."""
        # The finalise kernel runs on the driver's own stream and does not wait for the current one.  The caching
        # allocator hands out memory per stream: a block freed on the current stream (say the accumulators of a
        # two-pass frame before this one) may go out again at once while kernels queued there still use it — fine
        # for consumers on that stream, fatal for a kernel on another one that writes right away (found by
        # tools/fuzz_sequence.py: frames that fell back to the two-pass plan inside a single-pass sequence came out
        # wrong now and then).  So the outputs are allocated FOR the finalise stream, and the streams that read them
        # are recorded on them.
        import torch
        with torch.cuda.stream(self._finalize_stream()):
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.ctx.device)
        buf.record_stream(cur)
        if self.consumer_stream is not None and self.consumer_stream != cur:
            buf.record_stream(self.consumer_stream)
        return buf, buf.view(torch.float64), (buf.view(torch.int16) if self.fd.img_dtype_code == 2 else buf)

    def _fused_outputs(self, res, pxPerDeg, mem=None, offset=0):
        """Grid description and output arrays (one allocation for the finalise stream; `mem` = a _fused_alloc shared by
        the frames of a launch, this frame's part starting at byte `offset`) of a frame amt_pipe_wait has laid out ->
        (out dict without the arrays, packed, mean, count, img, mask)."""
        import torch
        if mem is None:
            mem = self._fused_alloc(self._fused_nbytes(res), torch.cuda.current_stream(self.ctx.device))
        buf, b64, _ = mem
        # (one allocation for the four arrays: mean | count | image | mask; bbox[7]: a pole plan)
        out, packed, mean, count, img, mask, end = _frame_block(
            res.grid, pxPerDeg, res.bbox, bool(res.lon_wrapped), bool(res.bbox[7]), self.altitude, b64, offset // 8, buf,
            offset + 40 * res.grid.ny * res.grid.nx, self.fd.img_dtype_code == 2)
        # (the frame's bytes as they lie in the allocation: one copy takes all four arrays to the host)
        out['_block'] = buf[offset:end]
        return out, packed, mean, count, img, mask

    def _fused_wrap(self, out, packed, mean, count, img, mask, keep_on_device):
        fd = self.fd
        block = out.pop('_block')
        if keep_on_device:
            # `packed`: mean and count as they lie in memory, one after the other — the payload of this frame in the
            # gather's wire format (auromat_amd.sequence.pack_results) without a copy per array
            out.update(mean=mean, img=img, mask=mask, count=count, packed=packed)
            return out
        out.update(grid_coordinates(out))
        # ONE device-to-host copy (and one synchronisation) for the four arrays, views on the host
        host = block.cpu().numpy()
        ny, nx = mean.shape[0], mean.shape[1]
        n = ny * nx
        isz = fd.img_dtype.itemsize
        out.update(mean=host[:32 * n].view(np.float64).reshape(ny, nx, 4), count=host[32 * n:40 * n].view(np.float64).reshape(ny, nx),
                   img=host[40 * n:40 * n + 3 * isz * n].view(fd.img_dtype).reshape(ny, nx, 3),
                   mask=host[40 * n + 3 * isz * n:40 * n + 3 * isz * n + n].astype(bool).reshape(ny, nx))
        return out

    def _finalize_fused(self, res, pxPerDeg, keep_on_device):
        """Crop the superset accumulators to the exact grid laid out by amt_pipe_wait."""
        out, packed, mean, count, img, mask = self._fused_outputs(res, pxPerDeg)
        self._pcall('amt_pipe_finalize', ptr(mean), ptr(img), ptr(mask), ptr(count))
        if not (keep_on_device and self.defer_join):
            self.join()
        return self._fused_wrap(out, packed, mean, count, img, mask, keep_on_device)

    @staticmethod
    def finalize_many(pipes, results, pxPerDeg, keep_on_device):
        """:meth:`_finalize_fused` for the frames of one launch with ONE call and ONE kernel (amt_pipe_finalize_many):
        `results` are their amt_pipe_results (all status 0) -> list of result dicts."""
        import torch
        n = len(pipes)
        ctx = pipes[0].ctx
        # the outputs of the launch's frames are ONE allocation when their drivers finalise on the same stream (they do:
        # the tail stream belongs to the context), each frame's part 256-byte aligned
        sizes = [q._fused_nbytes(r) for q, r in zip(pipes, results)]
        fin = pipes[0]._finalize_stream().cuda_stream
        if all(q._finalize_stream().cuda_stream == fin and q.consumer_stream == pipes[0].consumer_stream for q in pipes):
            mem = pipes[0]._fused_alloc(sum(sizes), torch.cuda.current_stream(ctx.device))
            offs = [sum(sizes[:i]) for i in range(n)]
            outs = [q._fused_outputs(r, pxPerDeg or q._fused['pxPerDeg'], mem, o) for q, r, o in zip(pipes, results, offs)]
        else:
            outs = [q._fused_outputs(r, pxPerDeg or q._fused['pxPerDeg']) for q, r in zip(pipes, results)]
        handles = (C.c_void_p * n)(*[q._pipe() for q in pipes])
        arr = lambda k: (C.c_void_p * n)(*[o[k].data_ptr() for o in outs])
        ctx.check(ctx._lib.amt_pipe_finalize_many(handles, n, arr(2), arr(4), arr(5), arr(3)))
        done = []
        for q, o in zip(pipes, outs):
            if not (keep_on_device and q.defer_join):
                q.join()
            q.last_plan = 'single-pass'
            done.append(q._fused_wrap(*o, keep_on_device=keep_on_device))
        return done

    def resample(self, pxPerDeg=10, containsPole=None, magnetic=False, keep_on_device=False, statistic='mean', q=None,
                 minCoverage=None):
        """Stages 2 + 3.  magnetic=True bins on the (MLat, SM longitude) grid (resampleMLatMLT).  statistic='median': the
        median of every cell (resampleMedian / resampleMedianMLatMLT) by the two-pass plan; the result holds 'median'
        in place of 'mean'.  statistic='quantile': the quantile(s) `q` of every cell (resampleQuantile /
        resampleQuantileMLatMLT; a number or up to 8 numbers in [0, 1]) in the same way; the result is that of
        :func:`auromat_amd.resample.resample_frame_quantile`, 'quantile' and 'img' with a leading axis over `q`.
        statistic='area': the area-weighted mean (resampleArea / resampleAreaMLatMLT; `minCoverage` in [0, 1], 0.5 when None) by
        :func:`auromat_amd.resample.resample_frame_area` on the frame's corner arrays — on a magnetic grid the SM copy whose
        corner longitudes are formed below —, never fused; the result holds 'area' and 'coverage' in place of 'mean' and
        'count'.  `minCoverage` with another statistic is a ValueError."""
        assert statistic in ('mean', 'median', 'quantile', 'area')
        assert (q is not None) == (statistic == 'quantile'), "q goes with statistic='quantile'"
        if minCoverage is not None and statistic != 'area':
            raise ValueError("minCoverage goes with statistic='area'")
        if statistic == 'area':
            minCoverage = 0.5 if minCoverage is None else minCoverage
            min_coverage_weight(minCoverage)
        if statistic == 'quantile':
            q = quantile_list(q)
        pxPerDeg = _px_per_deg(pxPerDeg)
        fd = self.fd
        self.ctx.bind()
        if statistic == 'mean' and self._fused is not None and self._fused['pxPerDeg'] == tuple(pxPerDeg) and \
                self._fused['magnetic'] == bool(magnetic):
            res = self._wait_fused()
            # (a direction-array frame whose caller left the pole open and whose box reaches within 5 deg of a pole was handed
            # back by the pole guard of amt_pipe_wait, not for a poor estimate: launching it again cannot help — the driver
            # refuses to fuse that box again —, its corner quads decide, below)
            pole_guard = self._dirs is not None and self._fused.get('pole_in_view', -1) < 0 and \
                (res.bbox[0] <= -85.0 or res.bbox[1] >= 85.0)
            if res.status == 1 and res.fused and res.bbox[6] > 0 and res.edge_pixels <= PIPE_MAX_EDGE_PIXELS and not self._fused.get('retried') \
                    and self.shard is None and not pole_guard:
                # handed back although the launch was fused (the exact box does not fit the superset grid of a poor estimate,
                # the date line judged differently by the pre-pass): once more with the exact box — in the coordinates of
                # the plan, res.bbox[7] — as the estimate, instead of five per-pixel arrays and a separate binning pass
                self.start_coarse(self.params, self.min_elevation, magnetic, hint=list(res.bbox))
                self.georef(None, self.altitude, None, None, bool(self.params.fast_center), self.min_elevation,
                            params=self.params, fuse_pxPerDeg=tuple(pxPerDeg), coarse_started=True, fuse_magnetic=bool(magnetic),
                            dirs=self._dirs, pole_in_view=self._fused.get('pole_in_view', -1))
                self._fused['retried'] = True
                res = self._wait_fused()
            # status 0: the driver could finalise the frame; a caller's containsPole must agree with its decision
            if res.status == 0 and (containsPole is None or bool(containsPole) == bool(res.bbox[7])):
                self.last_plan = 'single-pass'
                return self._finalize_fused(res, tuple(pxPerDeg), keep_on_device)
            if res.status == 2 or res.bbox[6] == 0:
                # no pixel above the threshold: known from the kernel's own reduction — a grids-only pipeline does not
                # allocate (and compute) five per-pixel arrays only to find that out again
                self.last_plan = 'empty'
                raise EmptyFrame('minElevation=' + str(self.min_elevation) + ' would mask all pixels!')
        self.coordinates()          # (grids-only pipelines: the arrays the two-pass plan reads are computed now)
        if not self.params.fast_center and fd.center_mask is None:
            # exact centres carry their own misses: a centre also needs its four corners and a corner a centre
            # (sanitize_data, reference mapping.py:1063-1125) — the separate binning pass takes the reconciled
            # centre mask; fast centres are consistent by construction (astrometry.py:35-40).  The kernel's own
            # bounding box and the single-pass plan apply the same rule per pixel.
            self.ctx.call('amt_sanitize_masks', ptr(fd.corner_mask_tensor()), ptr(fd.center_mask_tensor()), None,
                          fd.height, fd.width, 0)
        if magnetic:
            assert self.with_mag
            sm = fd.shallow_copy()
            sm.lat, sm.lat_c = fd.mlat, fd.mlat_c
            sm.lon, sm.lon_c = mlt_to_sm_lon(fd.mlt), mlt_to_sm_lon(fd.mlt_c)
            # corners of centres that pass the elevation threshold, in SM coordinates
            red = self._reduce_bbox(sm.lat, sm.lon)
            if red[6] == 0:
                self.last_plan = 'empty'
                raise EmptyFrame('minElevation=' + str(self.min_elevation) + ' would mask all pixels!')
            bb = bounding_box_from_reduction(red)
            fd = sm
        else:
            bb = self.bounding_box()
        pole = bb.containsPole if containsPole is None else containsPole
        self.last_plan = 'two-pass'
        if statistic == 'median':
            return resample_frame_median(fd, self.altitude, bb, pxPerDeg, bb.containsDiscontinuity, pole,
                                         min_elevation=self.min_elevation, keep_on_device=keep_on_device)
        if statistic == 'quantile':
            return resample_frame_quantile(fd, self.altitude, bb, pxPerDeg, q, bb.containsDiscontinuity, pole,
                                           min_elevation=self.min_elevation, keep_on_device=keep_on_device)
        if statistic == 'area':
            return resample_frame_area(fd, self.altitude, bb, pxPerDeg, bb.containsDiscontinuity, pole,
                                       min_elevation=self.min_elevation, keep_on_device=keep_on_device, minCoverage=minCoverage)
        return resample_frame(fd, self.altitude, bb, pxPerDeg, bb.containsDiscontinuity, pole,
                              min_elevation=self.min_elevation, keep_on_device=keep_on_device, shard=self.shard)

    def run(self, wcsHeader, altitude, cameraPosGCRS, photoTime, img=None, fast=True, min_elevation=10.0,
            pxPerDeg=10, containsPole=None, magnetic=False, params=None, keep_on_device=False, fuse=False,
            arcsecPerPx=None, dirs=None, statistic='mean', q=None, minCoverage=None):
        """One frame end to end; returns the dict of :func:`auromat_amd.resample.resample_frame` (statistic='median': of
        :func:`auromat_amd.resample.resample_frame_median`, statistic='quantile' with the quantile(s) `q`: of
        :func:`auromat_amd.resample.resample_frame_quantile`, statistic='area' with `minCoverage`: of
        :func:`auromat_amd.resample.resample_frame_area`; none of them is fused).  `arcsecPerPx` (has
        precedence over pxPerDeg, like the reference's resample()): the box-first plan — a box pass, px/deg from the frame's
        own bounding box, then the single-pass launch (``fuse``) or the two-pass plan; the px/deg pair used is in the
        result as 'pxPerDeg'."""
        coarse_started = False
        if img is not None:
            host_array = not hasattr(img, 'is_cuda')
            if host_array and dirs is None and (params is not None or wcsHeader is not None):
                # a host image of a camera frame: the estimate's pre-pass (or the box pass) runs while the image crosses the
                # link, and only the rows a ray can hit cross it (43 % of the bench frame are sky)
                if params is None:
                    params = frame_params(wcsHeader, altitude, cameraPosGCRS, photoTime, fast, magnetic=self.with_mag)
                if fuse and not arcsecPerPx and self.fd.nchan == 3 and (self.with_mag or not magnetic):
                    self.start_coarse(params, min_elevation, bool(magnetic))
                    coarse_started = True
                self.set_image(img, rows=self.earth_rows(params, min_elevation))
            else:
                self.set_image(img)
        assert not (arcsecPerPx and dirs is not None), 'arcsecPerPx: the box-first plan is built on the camera model'
        if arcsecPerPx:
            if params is None:
                params = frame_params(wcsHeader, altitude, cameraPosGCRS, photoTime, fast, magnetic=self.with_mag)
            pxPerDeg, red = self.resolution_from_box(params, min_elevation, arcsecPerPx, magnetic)
            # (a pole in view: the reference's plateCarreeResolution gives no longitude resolution for a box that goes all
            # around, resample.py:47-61 — nothing to bin into, there as here)
            if not pxPerDeg[1] > 0:
                # (the reference fails on its `assert nLon > 1`, resample.py:226-227; raised explicitly: python -O strips asserts)
                raise AssertionError('arcsecPerPx with a pole in view: plateCarreeResolution yields lonPxPerDeg = 0 (as the reference)')
            if fuse and not red[7]:
                self.start_coarse(params, min_elevation, magnetic, hint=red)
                coarse_started = True
        pxPerDeg = _px_per_deg(pxPerDeg)
        self.georef(wcsHeader, altitude, cameraPosGCRS, photoTime, fast, min_elevation, params=params,
                    fuse_pxPerDeg=pxPerDeg if fuse else None, fuse_magnetic=bool(magnetic), coarse_started=coarse_started,
                    dirs=dirs, pole_in_view=-1 if containsPole is None else int(bool(containsPole)))
        res = self.resample(pxPerDeg, containsPole, magnetic, keep_on_device=keep_on_device, statistic=statistic, q=q,
                            minCoverage=minCoverage)
        res['pxPerDeg'] = tuple(pxPerDeg)
        return res

    def host_arrays(self, kept_only=False):
        """Raw (NaN = missing) coordinate arrays of the last frame as NumPy arrays.  `kept_only`: only the arrays the
        pipeline's own launches write (a with_geo=False pipeline: elevation, MLat, MLT), without computing the others."""
        geo = ['lat', 'lon', 'lat_c', 'lon_c']
        names = geo + ['elev'] + (['mlat', 'mlt', 'mlat_c', 'mlt_c'] if self.with_mag else [])
        if kept_only and not self.with_geo and self._kept_valid:
            names = names[4:]
        else:
            self.coordinates()
        return {k: self.fd.host(k) for k in names}


_CLASS_PIPES = ThreadPipes()             # per host thread, like Context._cache


def fused_class_pipeline(width, height, img_dtype, magnetic=False):
    """The frame pipeline behind the mapping classes' fused resample() (one per host thread, frame size / image type / grid
    kind and device, grids only: its per-pixel arrays are only allocated when a frame has to take the two-pass plan)."""
    ctx = Context.current()
    key = (str(ctx.device), int(width), int(height), np.dtype(img_dtype).str, bool(magnetic))
    return _CLASS_PIPES.get(key, lambda: FramePipeline(width, height, img_dtype=img_dtype, with_mag=bool(magnetic),
                                                       alloc_coords=False))


_STREAMS = {}


def _shared_stream(device, role):
    """The stream of a given role (main / alt / bin / copy) on `device`, shared by every SequencePipeline of the process.
    A GPU serves a process through a handful of hardware queues and HIP maps streams onto them in turn: a pipeline that
    made streams of its own could end up with its main stream on the queue of the driver's helper streams, whose
    kernels WAIT for events — the big kernels then queue behind those waits (measured: the bench variant that came
    second paid 58 us per frame for it, whatever it computed).  With one set of streams per process the mapping is the
    same for every pipeline."""
    import torch
    key = (str(device), role)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=device)
    return _STREAMS[key]


def _runs(indices):
    """Ascending indices -> [(first, end)] of their runs of consecutive values (the frames of a batch that are launched)."""
    runs = []
    for i in indices:
        if runs and runs[-1][1] == i:
            runs[-1] = (runs[-1][0], i + 1)
        else:
            runs.append((i, i + 1))
    return runs


_RUN_RESULT_DTYPE = []


def _run_result_dtype():
    """np.dtype of amt_run_result (built once: the conversion of the nested ctypes structure takes ~60 us, which a
    20-frame call would pay twice)."""
    if not _RUN_RESULT_DTYPE:
        _RUN_RESULT_DTYPE.append(np.dtype(RunResult))
    return _RUN_RESULT_DTYPE[0]


class NativeResults(object):
    """
    The results of one :meth:`SequencePipeline.process` call through the native runner (amt_run_process): a read-only
    sequence of the usual per-frame result dicts (None for a frame without a valid pixel), built when first asked for —
    the arrays are views into two arenas the call filled (mean | count of all frames back to back, which is the payload of
    the gather's wire format as it stands; rounded image | mask per frame), so a caller that only gathers the grids
    (:func:`auromat_amd.sequence.gather_device`) touches no per-frame Python object at all.
    """

    def __init__(self, seq, records, grids, images, fallbacks, keep_on_device):
        self._seq, self._rec, self._grids, self._images = seq, records, grids, images
        self._fallbacks, self._keep = fallbacks, keep_on_device
        self._cache = {}
        self._table = np.frombuffer(records, dtype=_run_result_dtype()) if len(records) else None

    def __len__(self):
        return len(self._rec)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        if i not in self._cache:
            self._cache[i] = self._build(i)
        return self._cache[i]

    def __add__(self, other):
        return list(self) + list(other)

    def __mul__(self, n):
        return list(self) * n

    def _build(self, i):
        r = self._rec[i]
        if r.status in (2, 4):
            return None
        if r.status != 0:
            return self._fallbacks[i]
        seq = self._seq
        fd = seq.pipes[0].fd
        ppd = (r.lat_px_per_deg, r.lon_px_per_deg)
        stat = seq.statistic            # 'mean', 'median', 'quantile' or 'area': the name of the block in the result
        cnt = 'coverage' if stat == 'area' else 'count'     # (the area pass writes the coverage where the others count)
        out, packed, mean, count, img, mask, _ = _frame_block(
            r.grid, ppd, r.bbox, bool(r.lon_wrapped), bool(r.contains_pole), r.altitude, self._grids, r.grid_offset, self._images,
            r.image_offset, fd.img_dtype != np.uint8)
        out.update(magnetic=seq.magnetic, pxPerDeg=ppd)
        if self._keep:
            out.update(img=img, mask=mask, packed=packed)
            out[stat], out[cnt] = mean, count
            return out
        out.update(grid_coordinates(out))
        out.update(img=to_host(img, dtype=fd.img_dtype), mask=to_host(mask).astype(bool))
        out[stat], out[cnt] = to_host(mean), to_host(count)
        return out

    # ---- what the gather needs, without per-frame objects (auromat_amd.sequence) -----------------------------------
    def payload(self):
        """(device tensor, length): mean | count of all frames back to back, or None when a frame took another path (or the
        grids hold medians: the gather carries means)."""
        if self._table is None or not self._keep or np.any(self._table['status'] == 1) or self._seq.statistic != 'mean':
            return None
        t = self._table
        used = int((5 * t['ny'].astype(np.int64) * t['nx']).sum())
        return self._grids[:used], used

    def descriptors(self, indices):
        """The (n, 12) descriptor table of auromat_amd.sequence.describe_results."""
        t = self._table
        d = np.zeros((len(self), 12), dtype=np.float64)
        if t is None:
            return d
        ok = t['status'] == 0
        g = t['grid']
        d[:, 0], d[:, 1] = t['ny'], t['nx']
        d[:, 2] = np.where(ok, 4, 0)
        d[:, 3], d[:, 4] = g['lat_center_first'], g['lon_center_first']
        d[:, 5], d[:, 6] = g['lat_step'], g['lon_step']
        d[:, 7] = indices
        d[:, 8] = t['contains_pole']
        d[:, 9] = (t['lon_wrapped'] != 0) | (t['contains_pole'] != 0)
        d[:, 10] = t['altitude']
        d[:, 11] = 1.0 if self._seq.magnetic else 0.0
        d[~ok, :7] = 0
        d[~ok, 8:] = 0
        return d


class SequencePipeline(object):
    """
    Software-pipelined processing of a sequence of equally sized frames on one GPU — what the reference does
    with ``map`` over ``getMappingSequence`` followed by ``resample`` (spacecraft.py:326-332, cli/convert.py:185-220).

    Two frame buffers alternate.  While the GPU georeferences + bins frame k+1, the host finishes frame k
    (waits for its bounding box, lays out its grid, enqueues the crop/finalise) and prepares frame k+2 (rotation
    matrices, coarse bounding-box pre-pass).  plan='single-pass' uses the native frame driver (amt_pipe_*) and
    falls back per frame to the two-pass plan where it does not apply; plan='two-pass' bins with a separate
    kernel, optionally on a second stream beside the next frame's ray casting.
    """

    def __init__(self, width, height, nchan=3, img_dtype=np.uint16, device=None, altitude=110, fast=True,
                 min_elevation=10.0, pxPerDeg=10, plan='single-pass', bin_stream=True, shared_image=None,
                 magnetic=False, batch=3, own_image_buffers=True, keep_coordinates=True, launch_streams=1,
                 geodetic_arrays=None, arcsecPerPx=None, padded=None, statistic='mean', quantile=None, minCoverage=None):
        import torch
        assert plan in ('single-pass', 'two-pass')
        # statistic='median' (resampleMedian / resampleMedianMLatMLT): every frame through the native runner's median pass —
        # the frame kernel writes the buffer's centre and elevation arrays (contiguous rows), the median kernels bin them
        # (amt_run_config.statistic, amt_median_frame_async); the results carry 'median' in place of 'mean'
        # statistic='quantile', quantile=q (resampleQuantile / resampleQuantileMLatMLT): the same pass selecting ONE quantile
        # (amt_run_set_quantile, amt_quantile_frame_async); the results carry 'quantile'
        # statistic='area', minCoverage=f (resampleArea / resampleAreaMLatMLT; 0.5 when None): the runner's area pass on the
        # buffer's corner arrays, centre latitudes and elevation (amt_run_config.statistic = 2, amt_area_frame_async,
        # amt_run_set_min_coverage); the results carry 'area' and 'coverage' in place of 'mean' and 'count'
        assert statistic in ('mean', 'median', 'quantile', 'area')
        if statistic == 'area' and quantile is not None:
            raise ValueError("quantile goes with statistic='quantile', not with 'area'")
        assert (quantile is not None) == (statistic == 'quantile'), "quantile goes with statistic='quantile'"
        if minCoverage is not None and statistic != 'area':
            raise ValueError("minCoverage goes with statistic='area'")
        self.statistic = statistic
        self.quantile = None
        self.minCoverage = None
        if statistic == 'area':
            self.minCoverage = 0.5 if minCoverage is None else minCoverage
            self._min_weight = min_coverage_weight(self.minCoverage)
        if statistic == 'quantile':
            if np.ndim(quantile) != 0:
                raise ValueError('a sequence pipeline takes one quantile, got {!r}'.format(quantile))
            self.quantile = quantile_list(quantile)[0]
        if statistic != 'mean':
            assert plan == 'single-pass' and nchan == 3, "statistic='%s': RGB frames through the native runner" % statistic
            padded = False
            keep_coordinates = True
        # arcsecPerPx (has precedence over pxPerDeg, like the reference's resample(); what `auromat-convert --resample
        # --resolution R` passes, cli/convert.py:176-185): every frame's px/deg follows from its own bounding box
        # (plateCarreeResolution, resample.py:36-61) — the box-first plan: a box pass of the frame kernel two batches ahead of
        # the frame's single-pass launch, which takes the exact box as its estimate (process -> _process_box_first)
        self.arcsecPerPx = float(arcsecPerPx) if arcsecPerPx else None
        self.pxPerDeg = None if self.arcsecPerPx else _px_per_deg(pxPerDeg)
        if self.arcsecPerPx:
            assert plan == 'single-pass' and nchan == 3, 'arcsecPerPx: the box-first plan is a single-pass plan (RGB images)'
        self.altitude, self.fast, self.min_elevation = altitude, fast, min_elevation
        self.single_pass = plan == 'single-pass' and nchan == 3
        self.nchan = nchan
        self.magnetic = bool(magnetic)          # grids in (MLat, SM longitude): resampleMLatMLT
        # single-pass plan: `batch` frames share one launch of the big kernel (amt_pipe_launch_many; batch frames in
        # flight + batch being prepared = 2 * batch buffers).  Two-pass plan: one frame per launch and four buffers — a
        # buffer's binning pass, which runs beside the NEXT frame's big kernel, must be over before the buffer's next frame
        # starts, and with four that pass was enqueued two frames earlier.  The 14-17 us between two launches on a stream are
        # paid once per batch and the end of a launch is better filled: 0.207 -> 0.200 -> 0.198 ms per frame for
        # 1, 2, 3 frames per launch.
        self.batch = max(1, min(int(batch), 3)) if self.single_pass else 1
        # own_image_buffers=False: every frame of process() brings a device-resident image that is used in place
        # (no per-slot image buffer is allocated).  keep_coordinates=False ("grids only", what a convert run needs):
        # the single-pass plan writes no per-pixel latitude / longitude / elevation arrays, see FramePipeline.
        # geodetic_arrays (magnetic sequences): None / False = the buffers keep what resampleMLatMLT consumes — MLat, MLT
        # (corners and centres) and the elevation — and the single-pass kernel skips the geodetic half of its work
        # (FramePipeline(with_geo=False)); True = all nine per-pixel arrays, for callers that ask for both.  The grids are the
        # same bit for bit either way.
        self.geodetic_arrays = (not self.magnetic) or bool(geodetic_arrays) or not self.single_pass
        # padded (default: on for the single-pass plan, AMT_PADDED_ROWS=0 switches it off for A/B runs): the buffers' per-pixel
        # arrays in strip-padded rows, which the fused kernel writes 8-12 % faster; `pipes[i].fd.lat` & co. stay what they
        # were, contiguous arrays, compacted on request (FramePipeline(padded=True)).  The two-pass plan's binning kernel reads
        # contiguous rows: its buffers are not padded.
        if padded is None:
            padded = os.environ.get('AMT_PADDED_ROWS', '1') != '0'
        self.padded = bool(padded) and self.single_pass
        self.pipes = [FramePipeline(width, height, nchan, img_dtype, device, with_mag=self.magnetic,
                                    alloc_image=own_image_buffers and (shared_image is None or i == 0),
                                    alloc_coords=keep_coordinates or not self.single_pass, with_geo=self.geodetic_arrays,
                                    padded=self.padded)
                      for i in range((3 if self.arcsecPerPx else 2) * self.batch if self.single_pass else 4)]
        self.ctx = self.pipes[0].ctx
        if shared_image is not None:
            # every frame shows the same image (synthetic benchmarks): upload it once, both buffers alias it
            self.pipes[0].set_image(shared_image)
            for q in self.pipes[1:]:
                q.fd.img = self.pipes[0].fd.img
        for q in self.pipes:
            q.defer_join = True             # joined once per process() call
        self.s_main = _shared_stream(self.ctx.device, 'main')
        # launch_streams=2 (single-pass plan): the batches alternate between two streams.  A buffer set is used by every
        # second batch, i.e. always on the same stream, so every ordering between its users stays stream order; what
        # falls away is the order between CONSECUTIVE big kernels, which do not depend on each other: the next one
        # starts while the last waves of the previous one drain.
        self.s_alt = _shared_stream(self.ctx.device, 'alt') if (launch_streams == 2 and self.single_pass) else None
        # two-pass plan: the binning kernel is memory bound and the ray casting FP64 bound, so frame k's binning
        # runs beside frame k+1's ray casting on a second stream
        self.s_bin = _shared_stream(self.ctx.device, 'bin') if (bin_stream and not self.single_pass) else self.s_main
        self._geo_done = [torch.cuda.Event() for _ in self.pipes]
        self._bin_done = [None for _ in self.pipes]
        # per-frame images: uploaded on a copy stream of their own (created on first use: every extra stream competes
        # for the few hardware queues), so that frame k+1's 72 MB cross PCIe while frame k is being computed
        self.s_copy = None
        # events after which nothing enqueued so far reads this buffer's image any more: the single-pass launch on
        # s_main, and the separate binning kernel of a two-pass frame (plan='two-pass', or the per-frame fall-back of
        # the single-pass plan: pole in view, box misjudged, ...) wherever that runs.  An upload into the buffer waits
        # for all of them.
        self._img_busy = [[] for _ in self.pipes]
        self.plans = []                     # plan taken by each frame of the last process() call
        self.use_hints = True               # sequence coherence instead of the coarse pre-pass where possible
        self._hint = None                   # (exact bbox reduction, amt_frame_params, index) of the latest finished frame
        self._hint_prev = None              # ... and of the one finished before it (for the extrapolation, see _box_hint)
        self._frames_done = 0               # frames of earlier process() calls (hints count frames across calls)
        self.hinted = 0                     # frames of the last process() call that needed no pre-pass
        self.uploaded_bytes = 0             # image bytes the last process() call sent over the link (host images)
        # the frame loop in the library (amt_run_process) where it applies: device-resident images, no on_batch hook;
        # AMT_SEQ_NATIVE=0 keeps the Python loop (A/B runs)
        self.native = os.environ.get('AMT_SEQ_NATIVE', '1') != '0'
        self._run = None
        self._run_hints = True
        self._arena_cells = 1 << 16         # grid cells per frame the arenas of the next call are sized for

    def _stream_of(self, k):
        """The stream the batch of frame k is launched on (and its buffers are used on)."""
        if self.s_alt is None:
            return self.s_main
        return self.s_alt if (k // self.batch) % 2 else self.s_main

    def _box_hint(self, k, p):
        """
        Estimate of frame k's bounding-box reduction from frames that are already finished, or None (then the coarse
        pre-pass runs): amt_box_hint, the rule of the native runner (csrc/amt_params.h box_hint) — the latest finished
        frame's exact box when that frame is a neighbour of this one, else, in a steady sequence, the two latest boxes
        extrapolated linearly to this frame.  A poor estimate costs time (the frame falls back to the two-pass plan),
        never correctness.
        """
        last, prev = self._hint, self._hint_prev
        if last is None:
            return None
        box, q, i = prev if prev is not None else (None, None, 0)
        est = _Box8()
        ok = self.ctx._lib.amt_box_hint(last[0], C.byref(last[1]), last[2], box, None if q is None else C.byref(q), i, k,
                                        C.byref(p), est)
        return est if ok else None

    def _hint_record(self, bbox, params, k):
        """A frame the single-pass plan has finished becomes the latest record behind the box hints."""
        self._hint_prev = self._hint
        self._hint = (_Box8(*bbox), params, self._frames_done + k)

    def _altitude_of(self, f):
        """The shell of a frame tuple (header dict | amt_frame_params, camera, time, image[, altitude]): its own, or the pipeline's."""
        return f[4] if len(f) > 4 and f[4] is not None else self.altitude

    def _prepared(self, f):
        """A frame tuple -> (amt_frame_params, camera, time, image, altitude)."""
        hdr, cam, t, img = f[:4]
        alt = self._altitude_of(f)
        p = hdr if not isinstance(hdr, dict) else frame_params(hdr, alt, cam, t, self.fast, magnetic=self.magnetic)
        return p, cam, t, img, alt

    def _prepare(self, k, frame):
        prepared = self._prepared(frame)
        p = prepared[0]
        if self.single_pass:
            # the superset grid needs an estimate of the frame's bounding box: the exact box of the latest finished
            # frame when this one is its neighbour in the sequence (no kernel at all), else a coarse pre-pass (a
            # tiny kernel on the driver's own stream, which has to find room on a busy GPU)
            hint = self._box_hint(self._frames_done + k, p) if self.use_hints else None
            self.pipes[k % len(self.pipes)].start_coarse(p, self.min_elevation, self.magnetic, hint)
            self.hinted += hint is not None
        return prepared

    def _launch(self, k0, prepared, pxPerDeg=None):
        """Launch the frames k0, k0+1, ... (one batch; prepared = their _prepare results).  `pxPerDeg`: a list with one
        resolution per frame instead of the pipeline's."""
        import torch
        nb = len(self.pipes)
        qs = [self.pipes[(k0 + i) % nb] for i in range(len(prepared))]
        two_streams = self.s_bin is not self.s_main
        s_main = self._stream_of(k0)
        with torch.cuda.stream(s_main):
            for i, (q, (p, cam, t, img, alt)) in enumerate(zip(qs, prepared)):
                slot = (k0 + i) % nb
                if two_streams and self._bin_done[slot] is not None:
                    s_main.wait_event(self._bin_done[slot])     # the buffer's previous frame is still being binned
                if img is None:
                    continue
                if q.is_resident_image(img):
                    q.use_image(img)                                 # in place: nothing is overwritten
                    continue
                if self.s_copy is None:
                    self.s_copy = _shared_stream(self.ctx.device, 'copy')
                with torch.cuda.stream(self.s_copy):
                    for busy in self._img_busy[slot]:
                        self.s_copy.wait_event(busy)                 # the buffer's previous image is still being read
                    self._img_busy[slot] = []
                    # a host image: only the rows a ray of this frame can hit cross the link (no kernel reads the others)
                    on_host = not getattr(img, 'is_cuda', False)
                    rows = q.earth_rows(p, self.min_elevation) if (on_host and p is not None) else None
                    q.set_image(img, rows=rows)
                    if on_host:
                        r0, r1 = uploaded_rows(rows, q.height)
                        self.uploaded_bytes += (r1 - r0) * q.width * q.fd.nchan * q.fd.img_dtype.itemsize
                    uploaded = torch.cuda.Event()
                    uploaded.record(self.s_copy)
                s_main.wait_event(uploaded)
            if self.single_pass:
                FramePipeline.georef_many(qs, [pr[0] for pr in prepared], [pr[4] for pr in prepared],
                                          self.min_elevation, pxPerDeg if pxPerDeg is not None else self.pxPerDeg, self.magnetic)
                # a later upload into a buffer of the pipeline's own must wait until this launch has read it; frames that
                # read the caller's device-resident images need no event (each one is a packet on the stream of big
                # kernels: 5 us between two launches)
                own = [i for i, q in enumerate(qs) if q.fd.img is q._img_own]
                if own:
                    done = torch.cuda.Event()
                    done.record(s_main)
                    for i in own:
                        self._img_busy[(k0 + i) % nb].append(done)
            else:
                for i, (q, (p, cam, t, img, alt)) in enumerate(zip(qs, prepared)):
                    q.georef(None, alt, cam, t, self.fast, self.min_elevation, params=p)
                    if two_streams:
                        self._geo_done[(k0 + i) % nb].record(s_main)

    def _finish(self, k, keep_on_device):
        import torch
        slot = k % len(self.pipes)
        q = self.pipes[slot]
        two_streams = self.s_bin is not self.s_main
        s_bin = self.s_bin if two_streams else self._stream_of(k)
        with torch.cuda.stream(s_bin):
            if two_streams:
                s_bin.wait_event(self._geo_done[slot])
            try:
                res = q.resample(self.pxPerDeg if self.pxPerDeg is not None else q._fused['pxPerDeg'], magnetic=self.magnetic,
                                 keep_on_device=keep_on_device)
            except EmptyFrame:
                # no pixel of this frame is valid (looking off the limb, or min_elevation masks everything; the
                # reference raises ValueError there, mapping.py:858-859): the sequence goes on, the frame's place in
                # the results holds None
                res = None
            if res is not None:
                res['magnetic'] = self.magnetic
            if q.last_plan == 'two-pass':
                # the separate binning kernel reads the buffer's image (and coordinate arrays) on this stream
                if two_streams or q.fd.img is q._img_own:
                    ev = torch.cuda.Event()
                    ev.record(s_bin)
                    if q.fd.img is q._img_own:
                        self._img_busy[slot].append(ev)
                    if two_streams:
                        self._bin_done[slot] = ev
        self.plans.append(q.last_plan)
        if q.last_plan == 'single-pass':
            self._hint_record(q._fused['result'].bbox, q.params, k)
        else:
            self._hint = self._hint_prev = None     # the next frame gets a real pre-pass
        return res

    def _finish_batch(self, k0, n, keep_on_device):
        """The frames k0 .. k0+n-1 of one launch: those the driver can finalise get ONE finalise call and kernel
        (amt_pipe_finalize_many), the others (general path, no valid pixel) go one by one through :meth:`_finish`."""
        import torch
        nb = len(self.pipes)
        if not self.single_pass:
            return [self._finish(k0 + i, keep_on_device) for i in range(n)]
        qs = [self.pipes[(k0 + i) % nb] for i in range(n)]
        ready = [q.fused_ready(self.pxPerDeg, self.magnetic) for q in qs]
        idx = [i for i in range(n) if ready[i] is not None]
        done = {}
        if idx:
            with torch.cuda.stream(self._stream_of(k0)):
                res = FramePipeline.finalize_many([qs[i] for i in idx], [ready[i] for i in idx], self.pxPerDeg, keep_on_device)
            done = dict(zip(idx, res))
        out = []
        for i in range(n):
            if i not in done:
                out.append(self._finish(k0 + i, keep_on_device))
                continue
            r = done[i]
            r['magnetic'] = self.magnetic
            self.plans.append('single-pass')
            self._hint_record(ready[i].bbox, qs[i].params, k0 + i)
            out.append(r)
        return out

    # ---- the frame loop in the library (amt_run_*, include/auromat_hip.h "native sequence runner") --------------------
    def _native_applies(self, frames):
        """Device-resident images, header dicts, one launch stream; the single-pass plan or, for RGB frames with fast centres on
        a geodetic grid, the two-pass plan: what amt_run_process covers."""
        q = self.pipes[0]
        two_pass_ok = not self.single_pass and self.nchan == 3 and self.fast and not self.magnetic
        if not ((self.single_pass or two_pass_ok) and self.s_alt is None and frames):
            return False
        # (the checks of FramePipeline.is_resident_image, inlined: this runs for every frame of every call)
        dt, numel = q._img_torch_dtype, int(np.prod(q._img_shape))
        for f in frames:
            img = f[3]
            # a device-resident image, or one in page-locked host memory (a pinned torch tensor: amt_run_frame.img_host — the
            # runner uploads the rows of it that can be binned, one batch ahead of the frame's launch)
            if not (type(f[0]) is dict and hasattr(img, 'is_cuda') and img.dtype == dt and img.numel() == numel and
                    img.is_contiguous() and (img.is_cuda or img.is_pinned())):
                return False
        return True

    def _runner(self):
        if self._run is None:
            nb = len(self.pipes)
            slots = (GeorefOut * nb)()
            for i, q in enumerate(self.pipes):
                C.memmove(C.byref(slots[i]), C.byref(q._out), C.sizeof(GeorefOut))
            q = self.pipes[0]
            cfg = RunConfig(width=q.width, height=q.height, img_dtype=1 if q.fd.img_dtype == np.uint8 else 2, fast_center=1 if self.fast else 0,
                            magnetic=1 if self.magnetic else 0, batch=self.batch, use_hints=1 if self.use_hints else 0,
                            n_slots=nb, two_pass=0 if self.single_pass else 1,
                            statistic={'mean': 0, 'area': 2}.get(self.statistic, 1), altitude=float(self.altitude),
                            min_elevation=NEG_INF if self.min_elevation is None else float(self.min_elevation),
                            lat_px_per_deg=float(self.pxPerDeg[0]) if self.pxPerDeg else 0.0,
                            lon_px_per_deg=float(self.pxPerDeg[1]) if self.pxPerDeg else 0.0, slots=slots,
                            arcsec_per_px=self.arcsecPerPx or 0.0)
            handle = C.c_void_p()
            self.ctx.call('amt_run_create', C.byref(cfg), C.byref(handle))
            self._run = handle
            if self.statistic == 'quantile':
                self.ctx.check(self.ctx._lib.amt_run_set_quantile(handle, self.quantile))
            if self.statistic == 'area':
                self.ctx.check(self.ctx._lib.amt_run_set_min_coverage(handle, self._min_weight))
            self._run_hints = self.use_hints
        return self._run

    def _area_overflow(self, n):
        """The overflow words of the first `n` frames of the runner call that has just ended (amt_run_area_overflow: waits for
        the stream; the one wait an area sequence adds), as an int32 array."""
        flags = (C.c_int32 * n)()
        self.ctx.check(self.ctx._lib.amt_run_area_overflow(self._run, flags, n))
        return np.frombuffer(flags, dtype=np.int32)

    def _hint_native_reset(self):
        self.ctx.check(self.ctx._lib.amt_run_reset_hints(self._run))

    def __del__(self):
        if getattr(self, '_run', None):
            try:
                self.ctx._lib.amt_run_destroy(self._run)
            except Exception:
                pass
            self._run = None

    def _process_native(self, frames, keep_on_device, index_base=0):
        """`index_base`: the index of frames[0] in the process() call (a frame named in an error counts from its start)."""
        import torch
        ctx = self.ctx
        n = len(frames)
        if self._run is not None and self._run_hints != self.use_hints:
            ctx._lib.amt_run_destroy(self._run)           # (use_hints is part of the runner's configuration)
            self._run = None
        run = self._runner()
        for q in self.pipes:
            q._written()
        if self._hint is not None or self._hint_prev is not None:
            # the Python loop ran in between: its hints are not the runner's
            self._hint = self._hint_prev = None
        rec = (RunResult * n)()
        one = RunFrame()
        lib = ctx._lib
        done_total = 0
        grids = images = None
        arenas = []
        # the big kernels run on the stream all pipelines of the process share (see _shared_stream), behind whatever the
        # caller's stream has queued (its images); the caller's stream is ordered behind the call's work at the end
        caller = torch.cuda.current_stream(ctx.device)
        bpp = 3 if self.pipes[0].fd.img_dtype == np.uint8 else 6
        self.s_main.wait_stream(caller)
        with torch.cuda.stream(self.s_main):
            ctx.bind()                     # the library enqueues on torch's current stream
            while done_total < n:
                m = n - done_total
                cells = self._arena_cells * m
                g = torch.empty(5 * cells, dtype=torch.float64, device=ctx.device)
                im = torch.empty((bpp + 1) * cells + 256 * m, dtype=torch.uint8, device=ctx.device)
                out = C.cast(C.byref(rec[done_total]), C.POINTER(RunResult))
                ctx.check(lib.amt_run_begin(run, g.data_ptr(), g.numel(), im.data_ptr(), im.numel(), out, m))
                try:
                    # frame by frame: the library launches as soon as a batch is complete, the first after one frame
                    for f in frames[done_total:]:
                        alt = self._altitude_of(f)
                        im_f = f[3]
                        if im_f.is_cuda:
                            run_frame(f[0], f[1], f[2], alt, im_f.data_ptr(), out=one)
                        else:
                            run_frame(f[0], f[1], f[2], alt, None, out=one, img_host_ptr=im_f.data_ptr())
                        ctx.check(lib.amt_run_push(run, C.byref(one)))
                except Exception:
                    #  a call that failed leaves the runner in no state to go on from: the next call makes a new one
                    lib.amt_run_end(run, None)
                    lib.amt_run_destroy(run)
                    self._run = None
                    raise
                done = C.c_int32(0)
                rc_end = lib.amt_run_end(run, C.byref(done))
                try:
                    ctx.check(rc_end)
                except Exception:
                    lib.amt_run_destroy(run)
                    self._run = None
                    raise
                if self.statistic == 'area' and done.value > 0:
                    over = np.flatnonzero(self._area_overflow(done.value))
                    if len(over):
                        raise area_overflow_error(index_base + done_total + int(over[0]))
                g.record_stream(caller)
                im.record_stream(caller)
                arenas.append((done_total, done.value, g, im))
                if done.value < m:
                    self._arena_cells *= 4                    # the grids are larger than assumed: the rest again
                    if done.value == 0 and self._arena_cells > (1 << 28):
                        raise MemoryError('amt_run: a single grid does not fit the arena')
                done_total += done.value
        caller.wait_stream(self.s_main)
        if len(arenas) == 1:
            grids, images = arenas[0][2], arenas[0][3]
        else:
            # (rare: the first call met grids larger than assumed) one arena for all frames, offsets shifted
            grids = torch.cat([a[2][:int(sum(5 * rec[k].ny * rec[k].nx for k in range(a[0], a[0] + a[1])))] for a in arenas])
            sizes = [max([0] + [rec[k].image_offset + ((bpp + 1) * rec[k].ny * rec[k].nx + 255) // 256 * 256
                                for k in range(a[0], a[0] + a[1]) if rec[k].status == 0]) for a in arenas]
            images = torch.cat([a[3][:sz] for a, sz in zip(arenas, sizes)])
            goff = ioff = 0
            for a, sz in zip(arenas, sizes):
                for k in range(a[0], a[0] + a[1]):
                    rec[k].grid_offset += goff
                    rec[k].image_offset += ioff
                goff += int(sum(5 * rec[k].ny * rec[k].nx for k in range(a[0], a[0] + a[1])))
                ioff += sz
        # frames the single-pass plan does not cover (box outside its superset grid, ...): the general path, one by one
        table = np.frombuffer(rec, dtype=_run_result_dtype())
        status = table['status']
        self.hinted += int(table['hinted'].sum())
        self.uploaded_bytes += int(table['uploaded_bytes'].sum())
        fallbacks = {}
        max_cells = int((table['ny'].astype(np.int64) * table['nx']).max()) if n else 1
        names = {0: 'single-pass', 2: 'empty', 4: 'pole-without-resolution'}
        ordered = self.statistic != 'mean'          # (the runner's median / quantile pass: named after the statistic)
        if not status.any() and not table['two_pass'].any():
            self.plans.extend(['single-pass'] * n)
        else:
            for k in range(n):
                st = int(status[k])
                if st in names:
                    self.plans.append((self.statistic if ordered else 'two-pass') if st == 0 and table['two_pass'][k] else names[st])
                    continue
                f = frames[k]
                q = self.pipes[0]
                if f[3].is_cuda:
                    q.use_image(f[3])
                else:
                    q.set_image(f[3])
                alt = self._altitude_of(f)
                try:
                    ppd = (table['lat_px_per_deg'][k], table['lon_px_per_deg'][k]) if self.arcsecPerPx else self.pxPerDeg
                    # (median: the frames the runner's median pass does not cover — a pole in view, exact centres — by
                    # resample_frame_median on the frame's arrays, what resampleMedian / resampleMedianMLatMLT run; quantile:
                    # likewise by resample_frame_quantile, its one quantile without the leading axis; area: by
                    # resample_frame_area with the pipeline's minCoverage)
                    res = q.run(f[0], alt, f[1], f[2], fast=self.fast, min_elevation=self.min_elevation, pxPerDeg=ppd,
                                magnetic=self.magnetic, keep_on_device=keep_on_device, fuse=False,
                                statistic=self.statistic, q=self.quantile, minCoverage=self.minCoverage)
                    if self.statistic == 'quantile':
                        res['quantile'], res['img'] = res['quantile'][0], res['img'][0]
                    res['magnetic'] = self.magnetic
                except EmptyFrame:
                    res = None
                fallbacks[k] = res
                self.plans.append(q.last_plan)
        self._arena_cells = max(self._arena_cells // 2 if len(arenas) == 1 else self._arena_cells, int(max_cells * 1.5) + 64, 1 << 12)
        self._frames_done += n
        return NativeResults(self, rec, grids, images, fallbacks, keep_on_device)

    def _process_box_first(self, frames, keep_on_device, on_batch=None):
        """
        process() with a resolution per frame (arcsecPerPx).  Three stages per batch of frames, software-pipelined over 3 x
        batch frame buffers so that the GPU never waits for the host:

            box(j)     the box pass of the batch's frames (ONE launch of the frame kernel without outputs, image or binning:
                       amt_pipe_launch_box_many), enqueued two batches ahead
            launch(j)  wait for those boxes (long finished), plateCarreeResolution per frame, the exact box as the estimate
                       of the single-pass launch (no pre-pass; its superset grid always holds the exact grid), ONE launch of
                       the fused kernel with a resolution per frame (amt_pipe_launch_many_res)
            finish(j)  wait for the exact boxes of the fused launch, lay out the grids, one finalise kernel

        in the order box(0) box(1) | launch(j) finish(j-1) box(j+2) | ..., i.e. on the stream: box(j+1), fused(j), box(j+2),
        fused(j+1), ...  A frame with a pole of its grid in view has no longitude resolution under plateCarreeResolution
        (reference resample.py:47-61: its box goes all around; the class API and the reference fail on it): its place in
        the results holds None and its entry in `plans` reads 'pole-without-resolution'; a frame without a valid pixel
        yields None / 'empty' as always.
        """
        import torch
        from .resample import plateCarreeResolution
        if self._run is not None:
            self._hint_native_reset()
        self._hint = self._hint_prev = None
        out = []
        it = iter(frames)
        B, nb = self.batch, len(self.pipes)
        caller = torch.cuda.current_stream(self.ctx.device)
        for q in self.pipes:
            q.consumer_stream = caller
        min_elev = NEG_INF if self.min_elevation is None else float(self.min_elevation)
        mag = 1 if self.magnetic else 0
        lib, ctx = self.ctx._lib, self.ctx

        def box(k0):
            """Parameters + box pass of up to B frames starting at k0 -> list of (p, cam, t, img, alt), empty at the end."""
            prepared = []
            for i in range(B):
                f = next(it, None)
                if f is None:
                    break
                prepared.append(self._prepared(f))
            if prepared:
                n = len(prepared)
                qs = [self.pipes[(k0 + i) % nb] for i in range(n)]
                with torch.cuda.stream(self.s_main):
                    ctx.bind()
                    handles = (C.c_void_p * n)(*[q._pipe() for q in qs])
                    pp = (C.c_void_p * n)(*[C.addressof(pr[0]) for pr in prepared])
                    ctx.check(lib.amt_pipe_launch_box_many(handles, n, pp, min_elev, mag))
            return prepared

        def launch(k0, prepared):
            """-> per frame None (no valid pixel) or its (latPxPerDeg, lonPxPerDeg); the others are launched."""
            ppd, live = [], []
            for i, pr in enumerate(prepared):
                q = self.pipes[(k0 + i) % nb]
                res = PipeResult()
                q._pcall('amt_pipe_wait', C.byref(res))
                if res.status == 2 or res.bbox[6] == 0:
                    ppd.append(None)
                    continue
                red = list(res.bbox)
                v = plateCarreeResolution(bounding_box_from_reduction(red), self.arcsecPerPx)
                if red[7] or not v[1] > 0:
                    ppd.append('pole')
                    continue
                q.start_coarse(pr[0], self.min_elevation, self.magnetic, hint=red)
                ppd.append(v)
                live.append(i)
            # (a launch takes consecutive buffers)
            for i, j in _runs(live):
                self._launch(k0 + i, prepared[i:j], pxPerDeg=ppd[i:j])
            return ppd

        def finish(k0, ppd):
            res = []
            done = 0
            for i, j in _runs([m for m, v in enumerate(ppd) if isinstance(v, tuple)]) + [(len(ppd), len(ppd))]:
                for v in ppd[done:i]:
                    self.plans.append('empty' if v is None else 'pole-without-resolution')
                    res.append(None)
                part = self._finish_batch(k0 + i, j - i, keep_on_device) if j > i else []
                for r, v in zip(part, ppd[i:j]):
                    if r is not None:
                        r['pxPerDeg'] = v
                res.extend(part)
                done = j
            return res

        batches = {0: box(0)}
        batches[1] = box(len(batches[0])) if batches[0] else []
        starts = {0: 0, 1: len(batches[0])}
        launched = {}
        j = 0
        while batches.get(j):
            launched[j] = launch(starts[j], batches[j])
            if j >= 1:
                done = finish(starts[j - 1], launched.pop(j - 1))
                out.extend(done)
                if on_batch is not None:
                    on_batch(starts[j - 1], done)
                del batches[j - 1]
            starts[j + 2] = starts[j + 1] + len(batches[j + 1])
            batches[j + 2] = box(starts[j + 2]) if batches[j + 1] else []
            j += 1
        if j >= 1:
            done = finish(starts[j - 1], launched.pop(j - 1))
            out.extend(done)
            if on_batch is not None:
                on_batch(starts[j - 1], done)
        with torch.cuda.stream(self.s_main):
            for q in self.pipes:
                q.join()
        caller.wait_stream(self.s_main)
        self._hint = self._hint_prev = None
        self._frames_done += len(out)
        return out

    def _process_median(self, frames, keep_on_device, on_batch):
        """process() with statistic='median', 'quantile' or 'area': the native runner, in pieces of up to `median_chunk` frames (an iterator — the
        convert driver's generator of decoded host images — is consumed piece by piece).  Device-resident and pinned images
        go to the runner as they are; any other image is copied to the device first, on the caller's stream."""
        import torch
        q = self.pipes[0]
        dt, shape = q._img_torch_dtype, tuple(q._img_shape)
        out = []
        it = iter(frames)
        while True:
            chunk = []
            for f in it:
                img = f[3]
                if not (hasattr(img, 'is_cuda') and img.dtype == dt and img.is_contiguous() and (img.is_cuda or img.is_pinned())):
                    a = np.ascontiguousarray(img.cpu().numpy() if hasattr(img, 'is_cuda') else img)
                    if a.dtype == np.uint16:
                        a = a.view(np.int16)
                    img = torch.from_numpy(a).to(self.ctx.device)
                assert type(f[0]) is dict and tuple(img.shape) == shape, \
                    "statistic='median' / 'quantile' / 'area': frames are (header dict, cameraPosGCRS, photoTime, image[, altitude])"
                chunk.append((f[0], f[1], f[2], img) + tuple(f[4:]))
                if len(chunk) == self.median_chunk:
                    break
            if not chunk:
                break
            got = list(self._process_native(chunk, keep_on_device, index_base=len(out)))
            if on_batch is not None:
                on_batch(len(out), got)
            out.extend(got)
        return out

    # frames per call of the runner in median sequences (the arenas and, for host images, their device copies)
    median_chunk = 24

    def finalize_stream(self):
        """The stream the single-pass results are produced on (the drivers' finalise stream, shared by the pipeline's
        buffers): consumers that want to touch results before process() returns enqueue there."""
        return self.pipes[0]._finalize_stream()

    def process(self, frames, keep_on_device=True, on_batch=None):
        """
        frames: iterable of (wcsHeader | amt_frame_params, cameraPosGCRS, photoTime, image | None[, altitude]);
        a fifth element overrides the pipeline's altitude for that frame (several shells in one sequence).
        An image can be a host array, a pinned host tensor of the buffer's dtype (uploaded asynchronously on a copy
        stream) or a device tensor of the buffer's layout, which is used in place.
        Returns the list of per-frame result dicts (see :func:`auromat_amd.resample.resample_frame`) in order;
        with keep_on_device the arrays are device tensors that are valid for work on the current stream.  A frame
        without any valid pixel yields None (the reference raises ValueError for it, mapping.py:858-859).
        `on_batch(k0, results)` is called with the results of every finished launch (frames k0, k0+1, ... of this call, in
        order) while later launches run: work on them belongs on :meth:`finalize_stream` (or behind this call's return).
        """
        import torch
        del self.plans[:]
        self.hinted = 0
        self.uploaded_bytes = 0
        if self.statistic != 'mean':
            return self._process_median(frames, keep_on_device, on_batch)
        if on_batch is None and self.native and isinstance(frames, (list, tuple)):
            # (an iterator — the convert driver's read-ahead generator of decoded host images — is consumed frame by frame
            # below: its images are not device-resident anyway, and materialising it would hold every decoded image of the
            # sequence in host memory before the first launch)
            if self._native_applies(frames):
                return self._process_native(frames, keep_on_device)
        if self.arcsecPerPx:
            return self._process_box_first(frames, keep_on_device, on_batch)
        if self._run is not None:
            self._hint_native_reset()
        # (the box of the latest finished frame stays from the previous call: a sequence handed over in pieces is still
        # a sequence, and every hint is checked against the new frame's camera before it is used)
        out = []
        it = iter(frames)
        B = self.batch
        caller = torch.cuda.current_stream(self.ctx.device)
        for q in self.pipes:
            q.consumer_stream = caller

        def next_batch(k0, size=B):
            """Prepare up to `size` frames starting at index k0 -> list (empty at the end of the sequence)."""
            prepared = []
            for i in range(size):
                f = next(it, None)
                if f is None:
                    break
                prepared.append(self._prepare(k0 + i, f))
            return prepared

        k = 0                                    # first frame of the batch that is finished next
        # the first launch carries one frame only: the GPU starts after one frame's preparation instead of three
        # (not with two launch streams, where a buffer set must stay on the stream of its batch parity)
        in_flight = next_batch(0, 1 if self.s_alt is None else B)
        if not in_flight:
            return out
        self._launch(0, in_flight)
        ahead = next_batch(len(in_flight))       # prepared, not launched
        while in_flight:
            n_now = len(in_flight)
            if ahead:
                self._launch(k + n_now, ahead)
                following = next_batch(k + n_now + len(ahead))
            else:
                following = []
            finished = self._finish_batch(k, n_now, keep_on_device)
            out.extend(finished)
            if on_batch is not None:
                on_batch(k, finished)
            k += n_now
            in_flight, ahead = ahead, following
        # order the caller's stream behind everything this call enqueued
        with torch.cuda.stream(self.s_main):
            for q in self.pipes:
                q.join()
        cur = caller
        cur.wait_stream(self.s_main)
        if self.s_alt is not None:
            cur.wait_stream(self.s_alt)
        if self.s_bin is not self.s_main:
            cur.wait_stream(self.s_bin)
        if keep_on_device:
            # the result tensors were allocated on the pipeline's streams: tell the caching allocator that the caller's
            # stream uses them too, so that their memory is not handed out again while the caller still reads it.
            # (Single-pass results are ONE allocation, recorded for the caller's stream when it was made — `packed` is
            # their mark; a call per array here cost 1-2 us each after the last kernel, where nothing hides it.)
            for res in out:
                if res is None or 'packed' in res:
                    continue
                for v in res.values():
                    if isinstance(v, torch.Tensor) and v.is_cuda:
                        v.record_stream(cur)
        self._frames_done += len(out)
        return out


class GatherSequence(object):
    """
    A sequence of equally sized frames resampled by gathering (:func:`auromat_amd.resample.resampleGather` /
    ``resampleGatherMLatMLT`` of every frame's ``maskedByElevation(min_elevation)``), a batch of frames per kernel launch.

    A gathered frame needs two pieces of device work: the box pass of the frame kernel (no output array, image or binning:
    the 8-number bounding-box reduction), from which the host lays out :func:`auromat_amd.resample.resample`'s grid for that
    frame, and the gather of the image onto that grid.  At a sequence's resolutions a grid is a few 32 x 32 tiles, so a gather
    per frame is a member-table copy and a launch.  Here the frames of a batch share them:

        box(j)     the box passes of batch j (``amt_pipe_launch_box_many``, up to three frames per launch of the frame kernel),
                   enqueued before the host waits for the boxes of batch j - 1
        gather(j)  wait for those boxes, lay out every frame's grid (the date-line rule, ``plateCarreeResolution`` per frame
                   with `arcsecPerPx`), ONE copy of the whole batch's axes from a page-locked staging buffer (three rotate; one
                   is reused only after the event of its copy) and ONE ``amt_gather_frames`` call into two arenas — the
                   samples, and elevation | mask | count

    in the order box(0) | box(1) gather(0) | box(2) gather(1) | ...  No per-pixel coordinate array exists anywhere, so the
    pipes are made without frame buffers.  :class:`SequencePipeline` is not involved and does not change.

    A frame whose box pass reports a pole of the grid's coordinates in view takes, with a fixed `pxPerDeg`, the class route —
    an ``ArraySpacecraftMapping``, :func:`auromat_amd.resample.gather_plan` and ``gather_frame``: plan 'class' —; with
    `arcsecPerPx` it has no longitude resolution: None / 'pole-without-resolution', as in :class:`SequencePipeline`.  A frame
    without a valid pixel: None / 'empty'.  Camera models are the plain TAN headers of a spacecraft sequence, with fast centres.
    """

    _TORCH_OF = {np.dtype(np.uint8): 'uint8', np.dtype(np.uint16): 'int16', np.dtype(np.float32): 'float32'}

    def __init__(self, width, height, nchan=3, img_dtype=np.uint16, device=None, altitude=110, min_elevation=10.0, pxPerDeg=25,
                 arcsecPerPx=None, magnetic=False, interpolation='linear', supersample=1, minCoverage=None, batch=8):
        from ._native import GATHER_MAX_JOBS
        from .resample import _check_gather_interpolation, _check_supersample
        # (the argument checks of resampleGather, in its order, then the pipeline's own: all before any device work)
        _check_gather_interpolation(interpolation)
        self.supersample, self._min_count = _check_supersample(supersample, minCoverage)
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or not 1 <= batch <= GATHER_MAX_JOBS:
            raise ValueError('batch must be an int in 1 ... %d, but is: %r' % (GATHER_MAX_JOBS, batch))
        if nchan not in (1, 3, 4):
            raise ValueError('nchan must be 1, 3 or 4, but is: %r' % (nchan,))
        if np.dtype(img_dtype) not in self._TORCH_OF:
            raise ValueError('img_dtype must be uint8, uint16 or float32, but is: %r' % (img_dtype,))
        if not (int(width) > 0 and int(height) > 0):
            raise ValueError('width and height must be positive, but are: %r, %r' % (width, height))
        if arcsecPerPx is not None and not float(arcsecPerPx) > 0:
            raise ValueError('arcsecPerPx must be positive, but is: %r' % (arcsecPerPx,))
        self.width, self.height, self.nchan, self.img_dtype = int(width), int(height), int(nchan), np.dtype(img_dtype)
        self.interpolation, self.minCoverage = interpolation, minCoverage
        self.arcsecPerPx = float(arcsecPerPx) if arcsecPerPx else None
        self.pxPerDeg = None if self.arcsecPerPx else _px_per_deg(pxPerDeg)
        self.altitude, self.min_elevation, self.magnetic = altitude, min_elevation, bool(magnetic)
        self.batch = int(batch)
        self.plans = []                     # plan taken by each frame of the last process() call
        self.uploaded_bytes = 0             # image bytes the last process() call sent over the link (host images)
        self.gather_calls = 0               # amt_gather_frames calls of the last process() call
        import torch
        self._img_torch_dtype = getattr(torch, self._TORCH_OF[self.img_dtype])
        # two sets of `batch` drivers: the box passes of batch j + 1 are in flight while the host reads those of batch j
        self.pipes = [FramePipeline(self.width, self.height, self.nchan, self.img_dtype if self.img_dtype != np.float32 else np.uint16,
                                    device, alloc_image=False, alloc_coords=False) for _ in range(2 * self.batch)]
        self.ctx = self.pipes[0].ctx
        self.s_main = _shared_stream(self.ctx.device, 'main')
        self.s_copy = None                  # (created with the first host image)
        self._staging = [[None, None] for _ in range(3)]      # [page-locked float64 tensor, event of its latest copy]
        self._staged = 0
        self._arenas = []                   # the arenas of the last process() call: its keep_on_device results are views

    # -- inputs -------------------------------------------------------------------------------------
    def _prepared(self, f):
        """A frame tuple -> (amt_frame_params, header, camera, time, image, altitude)."""
        hdr, cam, t, img = f[:4]
        alt = f[4] if len(f) > 4 and f[4] is not None else self.altitude
        if not isinstance(hdr, dict):
            raise NotImplementedError('GatherSequence takes frames as (WCS header dict, cameraPosGCRS, photoTime, image[, altitude])')
        if not (str(hdr.get('CTYPE1', 'RA---TAN')).strip() == 'RA---TAN' and str(hdr.get('CTYPE2', 'DEC--TAN')).strip() == 'DEC--TAN') \
                or any(k in hdr for k in ('A_ORDER', 'B_ORDER')):
            raise NotImplementedError('GatherSequence takes plain TAN headers (got CTYPE1=%r, CTYPE2=%r%s); resampleGather of a '
                                      'mapping with the header gathers any zenithal (+ SIP) model, one frame per call' %
                                      (hdr.get('CTYPE1'), hdr.get('CTYPE2'), ', SIP' if 'A_ORDER' in hdr or 'B_ORDER' in hdr else ''))
        if (int(hdr['IMAGEW']), int(hdr['IMAGEH'])) != (self.width, self.height):
            raise ValueError('the header is for %d x %d, the pipeline for %d x %d' %
                             (int(hdr['IMAGEW']), int(hdr['IMAGEH']), self.width, self.height))
        # (the parameters of the class API's camera mappings: _inverse_model)
        return frame_params(hdr, alt, cam, t, True), hdr, cam, t, img, alt

    def _device_image(self, img):
        """The frame's image on the device, ordered for s_main: a device-resident tensor of the layout is used in place, a
        host image is uploaded whole on the copy stream."""
        import torch
        shape = (self.height, self.width, self.nchan)
        if isinstance(img, torch.Tensor) and img.is_cuda:
            if img.dtype != self._img_torch_dtype or img.numel() != int(np.prod(shape)):
                raise ValueError('device image of the wrong layout: %s %s, the pipeline takes %s %s' %
                                 (tuple(img.shape), img.dtype, shape, self._img_torch_dtype))
            self.s_main.wait_stream(self._caller)       # (a generator may have written it on the caller's stream just now)
            return img.contiguous().view(shape)
        if self.s_copy is None:
            self.s_copy = _shared_stream(self.ctx.device, 'copy')
        with torch.cuda.stream(self.s_copy):
            dev = torch.empty(shape, dtype=self._img_torch_dtype, device=self.ctx.device)
            if isinstance(img, torch.Tensor):
                if img.dtype != self._img_torch_dtype or img.numel() != dev.numel():
                    raise ValueError('host tensor image of the wrong layout: %s %s' % (tuple(img.shape), img.dtype))
                dev.copy_(img.reshape(shape), non_blocking=img.is_pinned())
            else:
                a = np.ascontiguousarray(img, dtype=self.img_dtype)
                if a.size != dev.numel():
                    raise ValueError('image of %s values, the pipeline takes %s' % (a.shape, shape))
                self.ctx.bind()
                self.ctx.upload(a.view(np.int16) if a.dtype == np.uint16 else a, dev)
            uploaded = torch.cuda.Event()
            uploaded.record(self.s_copy)
        self.s_main.wait_event(uploaded)
        dev.record_stream(self.s_main)
        self.uploaded_bytes += dev.numel() * dev.element_size()
        return dev

    def _stage(self, flat):
        """One copy of `flat` (float64, host) to the device on s_main (current), from the next page-locked staging buffer."""
        import torch
        slot = self._staging[self._staged % len(self._staging)]
        self._staged += 1
        if slot[1] is not None:
            slot[1].synchronize()           # the buffer's latest copy has read it
        if slot[0] is None or slot[0].numel() < flat.size:
            slot[0] = torch.empty(max(int(flat.size) * 2, 1 << 14), dtype=torch.float64, pin_memory=True)
        slot[0][:flat.size].copy_(torch.from_numpy(flat))
        dev = torch.empty(int(flat.size), dtype=torch.float64, device=self.ctx.device)
        dev.copy_(slot[0][:flat.size], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(self.s_main)
        return dev

    def _arena(self, keep):
        def make(cells, nch, tdtype, n):
            import torch
            # two arenas: the samples; elevation | mask | count
            images = torch.empty((cells * nch,), dtype=tdtype, device=self.ctx.device)
            grids = torch.empty((cells * (10 if n > 1 else 9),), dtype=torch.uint8, device=self.ctx.device)
            keep.extend((images, grids))
            made = dict(img=images, elevation=grids[:8 * cells].view(torch.float64), mask=grids[8 * cells:9 * cells])
            if n > 1:
                made['count'] = grids[9 * cells:10 * cells]
            return made
        return make

    # -- the grid of a box --------------------------------------------------------------------------
    def _plan_of(self, red, params):
        """:func:`auromat_amd.resample.gather_plan`'s plan for a box pass's reduction, or 'pole' where plateCarreeResolution
        has no longitude resolution to give."""
        from .resample import gather_box_grid
        part, ppd = gather_box_grid(red, self.pxPerDeg, self.arcsecPerPx)
        if part['grid'] is None:
            assert self.arcsecPerPx           # (a fixed resolution is positive)
            return 'pole'
        return dict(part, altitude=None, params=params, zenithal=None, min_elevation=self.min_elevation, center_mask=None,
                    bbox=list(red), pxPerDeg=ppd)

    def _class_route(self, pr, keep_on_device):
        """A frame with a pole in view, at a fixed resolution: the class API's plan and gather (a rotated grid laid out from the
        frame's arrays)."""
        import torch
        from .mapping.spacecraft import ArraySpacecraftMapping
        from .resample import gather_frame, gather_plan
        _, hdr, cam, t, img, alt = pr
        if isinstance(img, torch.Tensor):
            img = to_host(img.contiguous(), dtype=self.img_dtype, shape=(self.height, self.width, self.nchan)) \
                if img.is_cuda else img.numpy().view(self.img_dtype).reshape(self.height, self.width, self.nchan)
        img = np.asarray(img).reshape(self.height, self.width, self.nchan)
        m = ArraySpacecraftMapping(hdr, alt, img, cam, t, 'gather-sequence', fastCenterCalculation=True)
        if self.min_elevation is not None:
            m = m.maskedByElevation(self.min_elevation)
        plan = gather_plan(m, self.pxPerDeg, None, None, self.magnetic)
        res = gather_frame(plan, img, self.interpolation, self.magnetic, self.supersample, self.minCoverage)
        res.update(bbox=None, pxPerDeg=self.pxPerDeg, altitude=alt)
        if keep_on_device:
            for k in ('img', 'mask', 'elevation', 'count'):
                if k in res:
                    a = res[k].astype(np.uint8) if k == 'mask' else res[k]
                    res[k] = torch.from_numpy(np.ascontiguousarray(a.view(np.int16) if a.dtype == np.uint16 else a)).to(self.ctx.device)
                    self._arenas.append(res[k])
        return res

    # -- the loop -----------------------------------------------------------------------------------
    def process(self, frames, keep_on_device=True, on_batch=None):
        """
        frames: iterable of (WCS header dict, cameraPosGCRS, photoTime, image[, altitude]) — :class:`SequencePipeline`'s tuples,
        consumed once, a batch ahead.  An image is a device tensor of the pipeline's layout ((h, w, c) uint8, the bits of uint16
        as int16, or float32), used in place, or a host array / tensor, uploaded whole on a copy stream.

        Returns per frame a dict — lat, lon, lat_c, lon_c, grid, img, mask, elevation, with ``supersample`` > 1 also count
        (and, for host results, coverage = count / n^2), contains_pole, contains_discontinuity, altitude, bbox (the box pass's
        reduction) and pxPerDeg — or None; `plans` holds 'gather', 'empty', 'pole-without-resolution' or 'class' per frame.
        With `keep_on_device` img, mask (uint8), elevation and count are device tensors, views into this call's arenas: valid
        for work on the current stream, which is ordered behind everything enqueued, until the next process() call.
        `on_batch(k0, results)` is called with every finished batch while the next one's box passes run.
        """
        import torch
        from .resample import _gather_frames_call, gather_frames_coordinates, gather_result, gather_to_host
        del self.plans[:]
        del self._arenas[:]
        self.uploaded_bytes = self.gather_calls = 0
        out = []
        it = iter(frames)
        B, nb = self.batch, len(self.pipes)
        caller = self._caller = torch.cuda.current_stream(self.ctx.device)
        min_elev = NEG_INF if self.min_elevation is None else float(self.min_elevation)
        mag = 1 if self.magnetic else 0
        lib, ctx = self.ctx._lib, self.ctx
        n = self.supersample
        self.s_main.wait_stream(caller)         # (device-resident images may have been written on the caller's stream)

        def box(parity):
            """Parameters + box passes of up to B frames on the drivers of set `parity` -> list of prepared frames."""
            prepared = []
            for _ in range(B):
                f = next(it, None)
                if f is None:
                    break
                prepared.append(self._prepared(f))
            with torch.cuda.stream(self.s_main):
                ctx.bind()
                for i in range(0, len(prepared), 3):            # AMT_PIPE_MAX_BATCH frames per launch of the frame kernel
                    part = prepared[i:i + 3]
                    handles = (C.c_void_p * len(part))(*[self.pipes[parity * B + i + m]._pipe() for m in range(len(part))])
                    pp = (C.c_void_p * len(part))(*[C.addressof(pr[0]) for pr in part])
                    ctx.check(lib.amt_pipe_launch_box_many(handles, len(part), pp, min_elev, mag))
            return prepared

        def gather(parity, prepared):
            results, jobs = [], []
            for i, pr in enumerate(prepared):
                res = PipeResult()
                self.pipes[parity * B + i]._pcall('amt_pipe_wait', C.byref(res))
                if res.status == 2 or res.bbox[6] == 0:
                    self.plans.append('empty')
                    results.append(None)
                    continue
                red = list(res.bbox)
                if red[7]:
                    if self.arcsecPerPx:
                        self.plans.append('pole-without-resolution')
                        results.append(None)
                    else:
                        self.plans.append('class')
                        with torch.cuda.stream(self.s_main):
                            results.append(self._class_route(pr, keep_on_device))
                    continue
                plan = self._plan_of(red, pr[0])
                if plan == 'pole':
                    self.plans.append('pole-without-resolution')
                    results.append(None)
                    continue
                plan['altitude'] = pr[5]
                self.plans.append('gather')
                jobs.append((len(results), plan, pr[4]))
                results.append(None)
            if jobs:
                plans = [p for _, p, _ in jobs]
                with torch.cuda.stream(self.s_main):
                    images = [self._device_image(img) for _, _, img in jobs]
                    ctx.bind()         # (an upload has bound the context to the copy stream)
                    sizes, flat = gather_frames_coordinates(plans, n)
                    outs, _, _ = _gather_frames_call(ctx, plans, images, self.interpolation, self.magnetic, n, self._min_count,
                                                     coords=(sizes, self._stage(flat)), arena=self._arena(self._arenas))
                    self.gather_calls += 1
                for (k, plan, _), o in zip(jobs, outs):
                    results[k] = gather_result(plan, altitude=plan['altitude'], bbox=plan['bbox'], pxPerDeg=plan['pxPerDeg'], **o)
            return results

        def deliver(k0, results):
            if not keep_on_device:
                # (one wait per batch: the read-backs are ordered behind the batch's kernel on s_main)
                with torch.cuda.stream(self.s_main):
                    for r in results:
                        if r is None or not isinstance(r['img'], torch.Tensor):
                            continue
                        r.update(gather_to_host(r, self.img_dtype))
            for r in results:
                if r is not None and n > 1 and not isinstance(r['count'], torch.Tensor):
                    r['coverage'] = r['count'] / float(n * n)
            out.extend(results)
            if on_batch is not None:
                on_batch(k0, results)

        current = box(0)
        j = 0
        while current:
            following = box((j + 1) % 2)
            deliver(len(out), gather(j % 2, current))
            current = following
            j += 1
        caller.wait_stream(self.s_main)
        for a in self._arenas:
            a.record_stream(caller)
        if not keep_on_device:
            del self._arenas[:]
        return out
