/*
 * auromat_hip.h — C ABI of libauromat_hip.so
 *
 * MI355X (gfx950) implementation of the per-pixel georeferencing + resampling
 * hot path of esa/auromat.  The reference is pure Python with an import-time
 * two-backend switch (`_np` / `_ne`, e.g. auromat/coordinates/intersection.py:160-163);
 * this library is the third backend.  Each entry point names the reference
 * function(s) it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *  - every function returns 0 on success, a negative AMT_E* code otherwise and
 *    never throws; amt_last_error() gives the message of the last failure on a context;
 *  - all array arguments are DEVICE pointers (hipMalloc'ed / torch .data_ptr()),
 *    C-contiguous, float64 unless stated; small fixed-size parameter blocks
 *    (3-vectors, 3x3 matrices, amt_frame_params) are HOST pointers;
 *  - kernels are enqueued on the context's stream and the call returns without
 *    synchronising unless documented ("synchronises"): device inputs are read, and device
 *    outputs written, in the order of that stream.  The exceptions are ordered against it by
 *    the library, except where named: amt_upload_staged / amt_download_staged copy on streams
 *    of their own between two events on the context's stream; the frame driver (amt_pipe_*)
 *    runs its pre-pass, its box folds and amt_pipe_finalize[_many] on streams of the context's
 *    own — the pre-pass of amt_pipe_coarse_dirs starts behind the context's stream, the folds
 *    behind the frame kernel, and the finalise kernel's OUTPUTS are ordered for the context's
 *    stream only by amt_pipe_join (see amt_pipe_finalize_stream for their allocation); the
 *    sequence runner (amt_run_*) uploads page-locked host images on a copy stream and joins
 *    every finalise kernel in amt_run_end.  DESIGN.md 4.3 has the table;
 *  - the caller owns every buffer; the library keeps no global state and contexts
 *    may be used from different threads (one thread per context at a time);
 *  - missing data is NaN (reference convention: intersection.py:50-56), never an error.
 */
#ifndef AUROMAT_HIP_H
#define AUROMAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: amt_georef_out grew (bin_pole, altitude); amt_rotate_pole_deg, amt_pipe_finalize_stream, amt_seq_* added (round 2) */
/* 4: amt_georef_last_variant; the MLat / MLT-only mode of the fused frame kernel (see amt_georef_out); the box-first plan
 *    (amt_pipe_launch_box[_many], amt_pipe_launch_many_res, amt_plate_carree_resolution) (round 4) */
/* 5: the single-pass plan on caller-supplied corner directions (amt_georef_coarse_bbox_dirs, amt_pipe_coarse_dirs,
 *    amt_pipe_launch_dirs); griddata(method='cubic') exactly: amt_delaunay_*, amt_cubic_gradients_csr, amt_cubic_eval (round 5) */
/* 6: amt_georef_out.row_layout (strip-padded rows for buffers a pipeline owns), amt_padded_pitch, amt_unpad_rows; host images in the
 *    sequence runner (amt_run_frame.img_host, amt_run_result.uploaded_bytes, amt_georef_image_rows, amt_malloc_host / amt_free_host)
 *    amt_pipe_launch_dirs_many, amt_host_threads, AMT_EDOMAIN; retired: amt_linear_gather, amt_cubic_gradients, amt_cubic_gather
 *    (round 6) */
/* 7: amt_median_frame (median binning, auromat_amd.resample.resampleMedian) */
/* 8: amt_median_frame_async (the median pass without a read-back); amt_run_config.statistic (median sequences in the runner, in
 *    place of reserved_); amt_pipe_set_plan(pipe, 2) */
/* 9: amt_mosaic_frames, amt_mosaic_member (the members of a collection binned onto one grid, auromat_amd.resample.resampleMosaic) */
/* 10, additions only (no struct changed, the number stays): quantile binning — amt_quantile_frame, amt_quantile_frame_async,
 *    amt_quantile_rank, amt_run_set_quantile, AMT_QUANTILES_MAX (auromat_amd.resample.resampleQuantile); the median and quantile
 *    mosaics; area-weighted binning — amt_area_frame, amt_area_frame_finalize (auromat_amd.resample.resampleArea);
 *    area-weighted mosaics — amt_area_mosaic_frames, amt_area_mosaic_member; area-weighted sequences — amt_area_frame_async,
 *    amt_run_config.statistic = 2, amt_run_set_min_coverage, amt_run_area_overflow
 *    (auromat_amd.pipeline.SequencePipeline(statistic='area')); map projections — amt_projection,
 *    amt_projection_stereographic, amt_projection_polar_aeqd, amt_project_forward, amt_project_inverse
 *    (auromat_amd.coordinates.projection) — and area-weighted binning on a map plane — amt_area_plane_frame
 *    (auromat_amd.resample.resampleStereographic, resampleStereographicMLatMLT, resampleMLatMLTPolar); scan-line maps —
 *    amt_scanline_select, amt_scanline_pack, amt_scanline_compose, amt_scanline_strip (auromat_amd.resample.resampleScanLines);
 *    the core role of the frame kernel's work items — amt_georef_last_core, amt_georef_core_bands, amt_run_core_stats,
 *    amt_georef_set_roles(ctx, 2); gather mosaics — amt_gather_mosaic, amt_gather_member, amt_gather_debug, AMT_INTERP_NEAREST
 *    (auromat_amd.resample.resampleGatherMosaic); supersampled gathering — amt_gather_mosaic_supersampled
 *    (auromat_amd.resample.resampleGather / resampleGatherMosaic with supersample > 1); gathered frames — amt_gather_frames,
 *    amt_gather_job (auromat_amd.resample.gather_frames, auromat_amd.pipeline.GatherSequence); mesh resampling —
 *    amt_mesh_frame (auromat_amd.resample.resampleMesh) */
#define AMT_ABI_VERSION 10

#define AMT_OK 0
#define AMT_EINVAL (-1)   /* bad argument (NULL pointer, negative size, unsupported dtype ...) */
#define AMT_EHIP (-2)     /* a HIP runtime call failed; see amt_last_error */
#define AMT_ENOMEM (-3)
#define AMT_EEMPTY (-4)   /* operation would leave no valid pixel (mapping.py:858-859 -> ValueError) */
#define AMT_EDOMAIN (-5)  /* the result exists but nothing can be built on it (amt_plate_carree_resolution: no longitude resolution
                           * for a box that goes all the way round; ABI v6) */

typedef struct amt_ctx amt_ctx;

/* ---- context & memory --------------------------------------------------------------- */

int amt_abi_version(void);
/* stream: the hipStream_t to enqueue on, used as given — NULL is the device's default (null)
   stream, which is also what torch.cuda.current_stream().cuda_stream reports unless a side stream
   is active.  own_stream != 0: ignore `stream`, create and own a non-blocking stream instead. */
int amt_ctx_create(int device_id, void* stream, int own_stream, amt_ctx** out_ctx);
int amt_ctx_destroy(amt_ctx* ctx);
/* A context may be moved between streams (the Python host follows torch's current stream): every call enqueues on
   the stream set at that moment, and the library's internal scratch memory is kept per stream, so work enqueued
   on different streams through one context may overlap on the GPU.  The context itself is not thread-safe: one
   host thread at a time. */
int amt_ctx_set_stream(amt_ctx* ctx, void* stream);
void* amt_ctx_get_stream(amt_ctx* ctx);
int amt_ctx_synchronize(amt_ctx* ctx);                 /* synchronises */
/* A test and debugging aid for that scratch memory: it changes no result of a correct library (every entry point writes what it
   reads there, in stream order), so a test can put the memory into any state and ask for the same bytes.  An addition to ABI
   v10; nothing else in the library calls it.
   amt_debug_scratch_info: of the context's CURRENT stream the size of its scratch buffer (*bytes, 0: it has none) and its
   device address (*ptr); how many streams of this context hold a buffer (*streams, at most 16: the least recently used
   one is synchronised and freed for a 17th); how many times entry points of this context have asked for scratch memory
   (*requests: a call that uses it adds one or more, the two functions below add none).  Every pointer is optional.
   amt_debug_scratch_fill: grows the current stream's buffer to at least `at_least` bytes exactly as an entry point that needs
   as much would (a first buffer has 1 MiB at least; growing synchronises that stream once and frees the old buffer; 0: the
   buffer as it is, or a first one), then enqueues on that stream a fill of the WHOLE buffer with `byte` (its low 8 bits).
   amt_debug_scratch_release: synchronises the current stream and frees its buffer (if any): the next entry point on that
   stream starts from a fresh allocation. */
int amt_debug_scratch_info(amt_ctx* ctx, size_t* bytes, void** ptr, int32_t* streams, uint64_t* requests);
int amt_debug_scratch_fill(amt_ctx* ctx, size_t at_least, int byte);
int amt_debug_scratch_release(amt_ctx* ctx);                                       /* synchronises */
const char* amt_last_error(amt_ctx* ctx);
/* Device properties the host side prints next to roofline numbers. */
int amt_device_info(amt_ctx* ctx, char* name, size_t name_len, int* compute_units, int* clock_khz,
                    size_t* total_mem);

/* Plain device-memory helpers so that a host without torch can drive the library. */
int amt_malloc(amt_ctx* ctx, size_t bytes, void** out_dptr);
int amt_free(amt_ctx* ctx, void* dptr);
/* Host threads a pool of this process may use when it would like `wanted` (no GPU call; ABI v6): the cores the process may run on
 * (sched_getaffinity) divided by the ranks that share the node (LOCAL_WORLD_SIZE of torch.distributed.run, or AMT_LOCAL_RANKS),
 * at least 1, at most `wanted`.  The library's own pools (amt_upload_staged's copy threads, the triangulator's strips) are
 * sized by it, so that eight ranks on one host do not start 8 x (8 + 16) threads on its cores.  *cores / *local_ranks (each
 * optional) report what it saw.  The reference is single-threaded per process (mapping/spacecraft.py:326-332). */
int amt_host_threads(int wanted, int* cores, int* local_ranks);
/* Page-locked host memory (what amt_run_frame.img_host points into: the DMA engine reads it at the link's rate while the host
 * goes on); ABI v6. */
int amt_malloc_host(amt_ctx* ctx, size_t bytes, void** out_hptr);
int amt_free_host(amt_ctx* ctx, void* hptr);
int amt_memcpy_h2d(amt_ctx* ctx, void* dst, const void* src, size_t bytes);   /* async on the stream */
int amt_memcpy_d2h(amt_ctx* ctx, void* dst, const void* src, size_t bytes);   /* synchronises */
int amt_memset(amt_ctx* ctx, void* dst, int value, size_t bytes);
/* Whole arrays between PAGEABLE host memory and the device at the rate of the link: a few host threads (AMT_COPY_THREADS,
 * default 8) each copy every n-th 4 MiB piece through page-locked staging pieces of their own and hand it to the DMA engine
 * on the context's stream (what a NumPy-array API like the reference's needs at its boundary: mapping.py:318-337 takes the
 * image as an array, every property returns one).  amt_upload_staged returns when the last piece has been handed over (the
 * source may be reused; the device side is ordered on the stream); amt_download_staged returns when dst_host is complete. */
int amt_upload_staged(amt_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
int amt_download_staged(amt_ctx* ctx, void* dst_host, const void* src_device, size_t bytes);
/* HIP-event timing on the context's stream (bench.py measures kernels with these). */
int amt_event_create(amt_ctx* ctx, void** out_event);
int amt_event_destroy(amt_ctx* ctx, void* event);
int amt_event_record(amt_ctx* ctx, void* event);
int amt_event_elapsed_ms(amt_ctx* ctx, void* start, void* stop, float* out_ms);   /* synchronises on stop */
/* Per-kernel timing: while enabled, amt_georef_frame[_dirs] and amt_bin_frame bracket their main kernel
 * launch (k_georef_rows / k_bin_frame, not the small fold / finalize kernels) with HIP events on the
 * context's stream.  enable = n > 0 brackets every n-th launch of each kind (the two event packets sit between
 * consecutive kernels on the stream, so a pipelined caller samples instead of timing every launch); 0 = off.
 * amt_timing_read sums the recorded launches and returns how many frames they covered (synchronises; a launch of
 * amt_pipe_launch_many covers several frames, so total / frames is the time per frame); enabling resets. */
#define AMT_KERNEL_GEOREF 0
#define AMT_KERNEL_BIN 1
int amt_timing_enable(amt_ctx* ctx, int enable);
int amt_timing_read(amt_ctx* ctx, int kernel, double* total_ms, int* launches);
/* Which variant of the frame kernel the context's latest amt_georef_frame[_dirs] / amt_pipe_launch[_many] / amt_run_* launch
 * ran (diagnostics; tests assert on it): *second = 0 (lat, lon) only, 1 + (MLat, MLT), 2 / 3 the pole plans, 4 the
 * MLat / MLT-only mode (see amt_georef_out); *bin = 0 no fused binning, 1 uint8, 2 uint16 image; *frames = frames in that
 * launch.  -1 in all three before the first launch. */
int amt_georef_last_variant(amt_ctx* ctx, int32_t* second, int32_t* bin, int32_t* frames);
/* Roles of the frame kernel's work items (additions to ABI 10; csrc/amt_params.h amt_prm::band_roles).  For a
 * frame of the TAN camera model the host sorts the rows of work items that cast rays into inner (every ray hits the shell and every
 * pixel lies at or above bbox_min_elevation: the row step runs without its hit, threshold and keep tests), low (no pixel can
 * reach the threshold: no image read, no binning, no box; launches with fused binning only) and generic rows; results do not
 * depend on it, bit for bit.  Frames of caller-supplied directions and the pole plans have generic rows only.
 * amt_georef_set_roles(ctx, 0): every launch through this context — amt_georef_frame, the frame drivers, the sequence runner —
 * takes generic rows only (tests compare the two); != 0, the default: the rule decides.
 * amt_georef_last_roles: work items of the context's latest launch per role, summed over its frames (each pointer optional; -1
 * before the first launch).
 * amt_georef_band_roles (no context, no GPU call): the rule itself for frame p and the threshold min_elevation (-inf: none) —
 * *rows_per_item pixel rows per row of work items, and ranges8 = { rows of work items, work items per row, the rows that cast
 * rays [sky_top_end, sky_bottom_begin) as amt_georef_sky_rows gives them, low_top_end, low_bottom_begin, inner_begin,
 * inner_end }: rows [sky_top_end, low_top_end) and [low_bottom_begin, sky_bottom_begin) are low, [inner_begin, inner_end) inner. */
int amt_georef_set_roles(amt_ctx* ctx, int enable);
int amt_georef_last_roles(amt_ctx* ctx, int64_t* generic, int64_t* inner, int64_t* low);
struct amt_frame_params;
int amt_georef_band_roles(const struct amt_frame_params* p, double min_elevation, int32_t* rows_per_item, int32_t* ranges8);
/* Core items (additions to ABI 10; csrc/amt_params.h amt_prm::core_frame_ok): inner rows of work items with an inner
 * row on either side, in a frame whose inner cone stays below 75 deg of latitude, clear of longitude 0 and +-180 deg, and whose
 * pixels are small enough for latitude and longitude to have no extreme on the pixel lattice there.  Their work items, but for the
 * first and the last of each row, take the core loop of the row step: no bounding box (none of their corners can be an extreme of
 * it), no keep flags, small angles without the test for the full arctangents after an item's first row.  Camera-model launches with a
 * finite bbox_min_elevation whose box is reduced over (lat, lon) only; results do not depend on it, bit for bit.
 * amt_georef_set_roles(ctx, 2): the roles stop at inner (A/B runs, tests).  Core items count as inner in amt_georef_last_roles and
 * amt_run_role_stats; amt_georef_last_core / amt_run_core_stats give their own count (-1 before the first launch / since the
 * last amt_run_begin).  amt_georef_core_bands (no context, no GPU call): core2 = the core rows of work items [begin, end) the rule
 * names for frame p and the threshold (0, 0: none). */
int amt_georef_last_core(amt_ctx* ctx, int64_t* core);
int amt_georef_core_bands(const struct amt_frame_params* p, double min_elevation, int32_t* core2);

/* ---- per-frame parameter block --------------------------------------------------------
 * Host scalars the reference derives once per frame:
 *   cd, crpix, rot   auromat/coordinates/wcs.py:80-99,135-139 (TAN WCS; rot = euler_matrix(...,'rzxz')[:3,:3])
 *   cam              BaseMapping.cameraPosGCRS, auromat/mapping/mapping.py:318-337
 *   a, b             wgs84A/B + altitude, auromat/mapping/mapping.py:1498-1501
 *   a0, b0           wgs84A/B for ECEF->geodetic, auromat/coordinates/transform.py:338
 *   m_geo, m_sm      mat_j2000_to_geo / mat_j2000_to_sm, auromat/coordinates/transform.py:683-691
 */
typedef struct amt_frame_params {
    int32_t width;        /* IMAGEW */
    int32_t height;       /* IMAGEH */
    int32_t fast_center;  /* BaseAstrometryMapping.fastCenterCalculation, astrometry.py:23-40 */
    int32_t reserved;
    double cd[4];         /* CD1_1 CD1_2 CD2_1 CD2_2 [deg/px] */
    double crpix[2];      /* CRPIX1 CRPIX2 (1-based FITS convention) */
    double rot[9];        /* native -> celestial rotation, row major */
    double cam[3];        /* camera position, km, J2000/GCRS */
    double a, b;          /* inflated ellipsoid axes, km */
    double a0, b0;        /* geodetic reference ellipsoid axes, km */
    double m_geo[9];      /* J2000 -> GEO, row major */
    double m_sm[9];       /* J2000 -> SM, row major */
} amt_frame_params;

/* Output block of amt_georef_frame.  Any pointer may be NULL (that array is not written).
 * Corner arrays have (height+1)*(width+1) elements, centre arrays height*width.
 * bbox (optional, 8 doubles, device): [lat_min, lat_max, lon_min, lon_max, lon_min_positive,
 * lon_max_nonpositive, n_valid_centres, 0] over the corners of centres with
 * elevation >= bbox_min_elevation — the inputs of BaseMapping.boundingBox
 * (auromat/mapping/mapping.py:693-743) for a mapping that was maskedByElevation()'d
 * (mapping.py:845-864).  Slot 7 (pole containment, what geodesic.py:183 containsOrCrossesPole decides
 * from the outline) is left 0 here: with a camera model the host projects the pole into the frame
 * instead; amt_bbox_corners fills it for arbitrary grids. */
struct amt_axis;                    /* defined in the binning section below */

typedef struct amt_georef_out {
    double* lat;      /* corners, deg   (BaseAstrometryMapping.lats,  astrometry.py:118-144) */
    double* lon;      /* corners, deg */
    double* lat_c;    /* centres, deg   (latsCenter / lonsCenter, astrometry.py:128-152) */
    double* lon_c;
    double* elev;     /* centres, deg   (elevation, astrometry.py:200-212) */
    double* mlat;     /* corners, deg   (mLatMlt, astrometry.py:170-183) */
    double* mlt;      /* corners, hours */
    double* mlat_c;   /* centres        (mLatMltCenter, astrometry.py:185-198) */
    double* mlt_c;
    double* bbox;
    double bbox_min_elevation;
    /* Optional fused binning (single-pass resample(method='mean'), auromat/resample.py:301-351): when
     * bin_acc != NULL every pixel with elevation >= bbox_min_elevation is binned right where it is
     * computed — x = lon_c, y = lat_c, or (SM longitude, MLat) with bin_magnetic, or the pole-rotated
     * (lon, lat) with bin_pole — into the uint64
     * accumulator planes of amt_bin_frame (count, 3 channel sums, fixed-point elevation), so the centre
     * arrays need not be read back (and need not be written at all: lat_c/lon_c/elev may be NULL).
     * The grid must be known before the launch: callers use a superset of the final grid, aligned to the
     * same global nodes (amt_georef_coarse_bbox), and crop in amt_bin_frame_finalize_window.
     * Both axes must be uniform; bin_img is (height, width, 3) uint8 (dtype 1) or uint16 (dtype 2).
     * MLat / MLT-only mode: with bin_magnetic, no bin_pole and lat = lon = lat_c = lon_c = NULL the kernel computes what
     * resampleMLatMLT consumes and nothing else (reference resample.py:63-71, mapping.py:1519-1547: mLatMlt, mLatMltCenter,
     * elevation, image) — ray, shell, SM rotation, (MLat, SM longitude), elevation, bin; no ECEF -> geodetic step at all.
     * mlat / mlt / mlat_c / mlt_c / elev (each optional) and the grids are bit-identical to the nine-array mode. */
    const struct amt_axis* bin_xaxis;     /* host pointers */
    const struct amt_axis* bin_yaxis;
    const void* bin_img;
    uint64_t* bin_acc;
    int32_t bin_img_dtype;
    int32_t bin_lon_wrap;
    int32_t bin_magnetic;          /* != 0: x = SM longitude (mltToSmLon(mlt)), y = MLat; bbox[0..6] then refer to these too.
                                    * Without bin_acc: only that — the box in (MLat, SM longitude); lat, lon, lat_c, lon_c
                                    * must then be NULL (MLat / MLT-only mode without binning) */
    /* Scheduling hint, no effect on results: order in which the frame's work items (strips of 63 columns x 16
     * rows, row-major) are dispatched.  1 = rows top to bottom, 2 = bottom to top; 0 or any other value = automatic:
     * bottom to top when the nadir lies below the frame centre (camera model; top to bottom for caller-supplied
     * directions).  Rays that miss the shell are cheap, hits are expensive;
     * starting with the rows where the Earth is lets the cheap items fill the end of the launch (4-5 % shorter
     * kernel; when the Earth is to the left or right every row mixes both kinds anyway).  amt_georef_coarse_bbox
     * reports the side from actual hits (bbox[7]). */
    int32_t item_order;
    /* Optional, with bin_acc: pixels that sit ON a bin edge in the sense of the right-most-edge rule
     * (histogram.py:215-224) are then not binned but appended to `bin_events` (32-byte records, see
     * csrc/amt_common.h bin_event; device memory, room for bin_event_capacity records) and counted in
     * *bin_event_count (device uint32, zero before the launch; it keeps counting beyond the capacity, which tells
     * the caller that the frame must be redone).  Whether such a pixel belongs to the bin above or below its edge
     * depends on whether the edge is the last one of the FINAL grid; the frame driver resolves them in
     * amt_pipe_finalize.  NULL: they are binned above the edge, exact only when the grid given is the final one. */
    void* bin_events;
    uint32_t* bin_event_count;
    int64_t bin_event_capacity;
    /* Pole plan of the fused binning (a pole of the grid's coordinates is in view; not with bin_lon_wrap): pixels are
     * binned at (lat, lon) — with bin_magnetic at (MLat, SM longitude) taken as if they were geodetic, as
     * resampleMLatMLT does — rotated by +90 deg about x at `altitude`: amt_rotate_pole_deg of the centre coordinates,
     * reference resample.py:176-201 — and bbox[0..5] are reduced over the rotated corners (to ~1e-11 deg: good for laying out the
     * grid unless an extreme sits within that of a grid node, see amt_pipe_wait).  `altitude` [km] is the mapping
     * altitude the shell (a, b) = (a0, b0) + altitude was built from, as rotatePole takes it.  MLat / MLT outputs can be
     * combined with either grid. */
    int32_t bin_pole;
    /* Row layout of the nine per-pixel output arrays (ABI v6; 0 in earlier callers' zero-initialised structs):
     *   AMT_ROWS_CONTIGUOUS (0)    C-contiguous (height+1, width+1) / (height, width), what the reference's properties return
     *                              (astrometry.py:118-152);
     *   AMT_ROWS_STRIP_PADDED (1)  for buffers a pipeline OWNS and hands on only on request: every array has rows of
     *                              P = amt_padded_pitch(width) doubles (corner arrays height+1 rows, pixel arrays height rows) and
     *                              element (y, x) lies at y P + 64 (x / 63) + x % 63 — the kernel's work items are strips of 63
     *                              columns, and with this layout each strip's run of a row is a whole number of 128-byte lines
     *                              that no other wave writes (a measured 8-12 % of the kernel's time: DESIGN.md 4.1).  The 64th
     *                              double of a strip (and columns beyond the frame in the last strip) is padding with
     *                              unspecified content.  amt_unpad_rows compacts an array into contiguous rows, bit for bit the
     *                              array the contiguous layout gives;
     *                              the two-pass binning (amt_bin_frame) and every other consumer read contiguous rows. */
    int32_t row_layout;
    double altitude;
} amt_georef_out;
#define AMT_ROWS_CONTIGUOUS 0
#define AMT_ROWS_STRIP_PADDED 1
/* Doubles per row of a strip-padded array of a frame `width` pixels wide (64 per strip of 63 columns; 4352 for 4240). */
int64_t amt_padded_pitch(int32_t width);
/* Strip-padded rows -> contiguous rows (device to device, on the context's stream): `src` has `rows` rows of
 * amt_padded_pitch(width) doubles, `dst` becomes a C-contiguous (rows, cols) array with cols = width (pixel arrays) or
 * width + 1 (corner arrays) — what BaseAstrometryMapping.lats & co. hand out (astrometry.py:118-152). */
int amt_unpad_rows(amt_ctx* ctx, const double* src_padded, int32_t rows, int32_t cols, int32_t width, double* dst);

/* ---- building blocks (auromat.coordinates) ------------------------------------------- */

/* auromat/coordinates/wcs.py:18-64,66-144 pix2world(..., ascartesian=True) for TAN headers and
 * auromat/mapping/astrometry.py:245-269 pixelDirection: unit direction of every pixel corner
 * (corner=1: (height+1, width+1, 3)) or centre (corner=0: (height, width, 3)), AoS. */
int amt_directions_tan(amt_ctx* ctx, const amt_frame_params* p, int corner, double* out_dirs);
/* auromat/coordinates/wcs.py:54-56: headers that are not plain TAN go to astropy.wcs.WCS(header).all_pix2world in the reference.
 * The zenithal family (Calabretta & Greisen 2002, 5.1: TAN, SIN without slant, ARC, STG, ZEA) with SIP distortion polynomials
 * (CTYPE "...-SIP": A_p_q / B_p_q, Shupe et al. 2005) on the device: unit direction (J2000) of every pixel corner (corner = 1:
 * (height+1, width+1, 3)) or centre of the rectangle that starts at pixel (start_x, start_y).  rot: native -> celestial
 * rotation, euler_matrix(RA+90, 90-Dec, -(LONPOLE-90), 'rzxz') as for amt_frame_params.  sip_a[p][q] multiplies u^p v^q
 * (u, v: pixel offsets from CRPIX), zero beyond the order; order 0 = no distortion.  The result feeds amt_georef_frame_dirs. */
#define AMT_SIP_MAX 10
typedef struct amt_zenithal_wcs {
    int32_t width, height, corner, projection;      /* projection: 0 TAN, 1 SIN, 2 ARC, 3 STG, 4 ZEA */
    double cd[4], crpix[2], rot[9];
    double start_x, start_y;
    int32_t sip_order_a, sip_order_b;
    double sip_a[AMT_SIP_MAX][AMT_SIP_MAX], sip_b[AMT_SIP_MAX][AMT_SIP_MAX];
} amt_zenithal_wcs;
int amt_directions_zenithal(amt_ctx* ctx, const amt_zenithal_wcs* w, double* out_dirs);
/* auromat/coordinates/wcs.py:66-144 tan_pix2world(header, px, py, origin, ascartesian=True) for arbitrary
 * pixel coordinates (origin 0 or 1 as in FITS/astropy); out (n,3) AoS.  Uses cd, crpix, rot of p only. */
int amt_directions_tan_points(amt_ctx* ctx, const amt_frame_params* p, const double* px, const double* py,
                              int64_t n, int origin, double* out_dirs);

/* ---- lens distortion (auromat.util.lensdistortion, auromat/mapping/iss.py:232-243) ------------------------------------
 * The step the reference takes through lensfunpy (Modifier.apply_geometry_distortion) and cv2 (lensfunpy.util.remap) before an
 * image matches its .wcs.  Radial models with the radius in units of half the frame's smaller side (reference draw.py:1104-1148):
 * with cx = (width-1)/2, cy = (height-1)/2, norm = 2/(min(width,height)-1), u = (x-cx) norm, v = (y-cy) norm, r^2 = u^2+v^2,
 *   poly3 (k[0]):            g = 1 - k0 + k0 r^2
 *   poly5 (k[0], k[1]):      g = 1 + k0 r^2 + k1 r^4
 *   ptlens (k[0],k[1],k[2]): g = a r^3 + b r^2 + c r + 1 - a - b - c
 * FORWARD: pixel (x, y) of the corrected image is sampled at (cx + u g / norm, cy + v g / norm) of the raw one (a factor of exactly
 * 1 gives (x, y) itself).  INVERSE: the ru with ru g(ru) = rd, by Newton's method from ru = rd with a fixed cap of steps; NaN where
 * it does not converge or the slope d(ru g)/dru is not positive on the way (the model folds over); rd = 0 is the centre exactly.
 * lensfun's rescaling by aspect ratio and crop factor is not part of this (crop factor 1, focal length 1: the reference's
 * getLensfunModifierFromParams), and agreement with lensfun's own output is not pinned: tests/_lens_oracle.py is the statement.
 * crop_*: the corrected image is the window [crop_x, crop_x + crop_width) x [crop_y, crop_y + crop_height) of the full corrected
 * frame (the reference crops to a multiple of 16, util/image.py:59-72) and its pixel coordinates count from the window's corner;
 * crop_width = crop_height = 0: no crop.  The raw frame is always width x height.  Additions to ABI 10. */
#define AMT_LENS_NONE 0
#define AMT_LENS_POLY3 1
#define AMT_LENS_POLY5 2
#define AMT_LENS_PTLENS 3
typedef struct amt_lens_model {
    int32_t kind, width, height;
    int32_t crop_x, crop_y, crop_width, crop_height, reserved;
    double k[3];
} amt_lens_model;
/* Forward coordinates of the pixels [x0, x0 + cols) x [y0, y0 + rows) of the (cropped) corrected image: out_xy (rows, cols, 2)
 * float64 in [x, y] order; corner = 1: the (rows + 1, cols + 1) lattice of pixel corners at x - 0.5, y - 0.5.  out_xy32 (optional):
 * the same rounded to float32, the array lensfunpy hands out. */
int amt_lens_coords(amt_ctx* ctx, const amt_lens_model* model, int32_t x0, int32_t y0, int32_t cols, int32_t rows, int corner,
                    double* out_xy, float* out_xy32);
/* Inverse: where the pixels (or corners) of that rectangle of the RAW frame lie in the (cropped) corrected frame. */
int amt_lens_undistort(amt_ctx* ctx, const amt_lens_model* model, int32_t x0, int32_t y0, int32_t cols, int32_t rows, int corner,
                       double* out_xy);
/* Sampling (both remap calls): interpolation 0 = linear, taps floor(xs), floor(xs) + 1; 1 = Lanczos-4, taps floor(xs) - 3 ...
 * floor(xs) + 4 weighted L(i - fx), L(t) = sinc(t) sinc(t/4), exactly 1 at 0 and 0 at other integers, each axis' eight weights
 * normalised to sum 1 (the role of cv2.INTER_LANCZOS4).  Taps outside the image count 0 (cv2.remap's constant border) without
 * renormalising; float64 accumulation; uint8 / uint16 results are clip(rint(v)) (half to even), float32 unrounded; a non-finite
 * source coordinate gives 0.  support (optional, one byte per output pixel): 1 where the source point lies in
 * [0, width-1] x [0, height-1].  Images are interleaved (height, width, channels), channels 1, 3 or 4, sample_bytes 1 (uint8),
 * 2 (uint16) or 4 (float32); dst has the type of src.
 * debug (optional): force_path AMT_LENS_PATH_GATHER makes every tile take its taps from global memory instead of the window staged
 * in LDS (a tile whose taps do not fit the window always does; both give the same bits); tile_path (optional, one byte per 32 x 32
 * output tile, row-major) reports what each tile did: 0 no tap inside the image, else AMT_LENS_PATH_STAGED / _GATHER. */
#define AMT_INTERP_LINEAR 0
#define AMT_INTERP_LANCZOS4 1
#define AMT_LENS_PATH_AUTO 0
#define AMT_LENS_PATH_STAGED 1     /* as AUTO: staged wherever the window holds the tile's taps */
#define AMT_LENS_PATH_GATHER 2
#define AMT_LENS_TILE 32
typedef struct amt_lens_debug {
    int32_t force_path, reserved;
    uint8_t* tile_path;
} amt_lens_debug;
/* The corrected (and cropped) image of a raw frame in one kernel: coordinates in float64 in registers, never stored. */
int amt_lens_remap(amt_ctx* ctx, const amt_lens_model* model, const void* src, int32_t sample_bytes, int32_t channels,
                   int32_t interpolation, void* dst, uint8_t* support, const amt_lens_debug* debug);
/* lensfunpy.util.remap(im, coords) for a coordinate array made elsewhere: coords (dst_height, dst_width, 2) float32, [x, y]. */
int amt_remap_coords(amt_ctx* ctx, const void* src, int32_t src_width, int32_t src_height, int32_t sample_bytes, int32_t channels,
                     const float* coords, int32_t dst_width, int32_t dst_height, int32_t interpolation, void* dst, uint8_t* support,
                     const amt_lens_debug* debug);
/* Where a model folds over (host only, no device work, no context): *out_r = r_fold, the smallest r > 0 with d(r g)/dr = 0 -
 * of the polynomial the kernels evaluate, whose coefficients 3 k0, 5 k1 (poly3, poly5), 4 a, 3 b, 2 c and 1 - a - b - c (ptlens)
 * are float64 roundings -, +inf where there is none, 0 where the slope is not positive at r = 0 already, NaN where a coefficient
 * the model reads is NaN; kind AMT_LENS_NONE: +inf.  Closed form for poly3 and poly5 (linear and quadratic in r^2); ptlens: the
 * root of the cubic is bracketed between the positive roots of its derivative and bisected to the last bit.  Only kind and k are
 * read.  Beyond r_fold the forward polynomial maps far-off corrected points back into the raw frame and the inverse has no
 * value.  AMT_EINVAL: NULL argument, unknown kind. */
int amt_lens_fold_radius(const amt_lens_model* model, double* out_r);

/* ---- inverse georeferencing: world -> pixel (additions to ABI 10) -------------------------------------------------------------
 * The way back from a place to the pixel that sees it: what the reference asks astropy's wcs_world2pix for (fits.py:193-216,
 * draw.py:1379: catalogue stars, constellation lines) and approximates with a resampled look-up table for parallels and
 * meridians (draw.py:1482-1609).  For every camera model of this library the inverse exists in closed form; this is its
 * statement (tests/_inverse_oracle.py holds it in mpmath and NumPy).
 * Inputs: a frame's amt_frame_params (cam, shell a, b, WGS84 a0, b0, m_geo, m_sm, width, height, and cd, crpix, rot of a plain
 * TAN header) and, for other zenithal headers, an amt_zenithal_wcs whose cd, crpix, rot, start_x, start_y, projection and SIP
 * terms then take the place of the camera-model cards of the params (its width, height and corner are not read).  A point is
 * (c0, c1) = (latitude-like, longitude-like) degrees in one of three frames:
 *   AMT_W2P_GEODETIC  WGS84 geodetic latitude and longitude of a point ON THE SHELL: with N = a0 / sqrt(1 - e^2 sin^2 lat),
 *                     G(h) = ((N+h) cos lat cos lon, (N+h) cos lat sin lon, (N (1-e^2) + h) sin lat) in GEO, P(h) = m_geo^T G(h)
 *                     in J2000, and h the larger root of the quadratic that puts P(h) on the shell (a, b) - the ellipsoid
 *                     whose axes are J2000's, as the forward intersects it (amt_intersect_ellipsoid on J2000 rays); h varies
 *                     with latitude and, through the few arc minutes between the two polar axes, by metres with longitude: do
 *                     not substitute the mapping altitude.  This inverts the exact geodetic latitude; the forward kernels
 *                     take one Bowring step (ecef_to_geodetic); tests/test_inverse_cpu.py records what that costs in pixels.
 *   AMT_W2P_SM        (MLat, SM longitude; MLT through mltToSmLon): the unit vector of the two angles goes to J2000 with m_sm^T
 *                     and is scaled onto the shell, u / sqrt(sum (u_i / rad_i)^2), rad = (a, a, b), as amt_pole_in_view does.
 *   AMT_W2P_J2000     (declination, right ascension): a direction without a position (stars).
 * 1. line of sight d = (P - cam) / |P - cam|; J2000: the direction itself.
 * 2. visibility, with q = P / rad, c = cam / rad: a shell point is visible iff c.c < 1 (camera inside the shell: the forward
 *    takes the far root, every shell point is seen) or q.c > 1 (camera on the outer side of the tangent plane at P) - the
 *    forward's root choice (near root outside, far root inside).  A J2000 direction is hidden iff its ray hits the shell by the
 *    forward's rule (discriminant >= 0 and ray parameter >= 0): stars are visible exactly in sky pixels.
 * 3. native direction (l, m, n) = rot^T d, rho = sqrt(l^2 + m^2).
 * 4. projection plane, degrees, k = 180/pi: x = R m / rho, y = -R l / rho with TAN R = k rho / n (domain n > 0), SIN R = k rho
 *    (n >= 0), ARC R = k atan2(rho, n), STG R = 2 k rho / (1 + n) (n > -1), ZEA R = k sqrt(2 (1 - n)) evaluated as
 *    k rho sqrt(2 / (1 + n)) (n > -1; exact as rho -> 0).  rho = 0 with n > 0 gives x = y = 0 exactly; rho = 0 with n <= 0 (the
 *    antipode of the boresight has no position angle) is outside every domain.
 * 5. pixel offsets (U, V) = CD^-1 (x, y).
 * 6. SIP: u + A(u, v) = U, v + B(u, v) = V by Newton's method from (U, V), at most 20 steps; it stops after a step of at most
 *    2^-40 max(1, |u|, |v|) pixels.  Not converged: the cap is reached, an iterate is not finite, or the Jacobian's determinant
 *    is not positive at an iterate (the polynomial folds over).  This inverts the forward polynomial amt_directions_zenithal
 *    evaluates; a header's AP / BP tables are not read.  Without SIP (u, v) = (U, V).
 * 7. 0-based pixel coordinates, a pixel's centre at (column, row): X = u + CRPIX1 - 1 - start_x, Y = v + CRPIX2 - 1 - start_y.
 * 8. elevation of the line of sight at P as the forward's exact centres define it (astrometry.py:200-212),
 *    90 deg - angle(-d, P / |P|); NaN for J2000 and invalid input, a number (negative) for hidden points.
 * Flags (one byte per point):
 *   AMT_W2P_INVALID        non-finite input or |c0| > 90
 *   AMT_W2P_HIDDEN         not visible by step 2
 *   AMT_W2P_UNPROJECTABLE  outside the projection's domain (or P = cam)
 *   AMT_W2P_NOT_CONVERGED  step 6 did not converge
 *   AMT_W2P_OUTSIDE        xy is a number and not in [-0.5, width - 0.5] x [-0.5, height - 0.5]
 *   AMT_W2P_LENS_FOLD      step 9b: beyond the radius at which the lens model folds over (or a non-finite lens factor)
 * 9. the lens (the _lens entry points with a model of kind != AMT_LENS_NONE): the frame is a RAW frame that still carries its
 *    lens distortion, and the camera model (the .wcs) belongs to the corrected image, cropped to the model's window: the X, Y of
 *    step 7 are coordinates in the cropped corrected frame.
 *    9a. Xf = X + crop_x, Yf = Y + crop_y; u, v, r^2 = u^2 + v^2 as the FORWARD of "lens distortion" forms them.
 *    9b. the principal branch: the point is kept iff r^2 < r_fold^2 (amt_lens_fold_radius, squared in float64; a constant of
 *        the model, computed once on the host) and g(r) is finite.  Beyond r_fold the forward polynomial maps far-off world
 *        points back into the raw frame, and the raw route's inverse (amt_lens_undistort) is NaN there.  A point not kept gets
 *        AMT_W2P_LENS_FOLD and xy NaN; so does every point of a model with a NaN coefficient, and of one with r_fold = 0.
 *    9c. (xs, ys) = FORWARD(Xf, Yf): the operations of amt_lens_coords in their order, its "g == 1 returns the coordinate
 *        itself" rule included.  xy is (xs, ys).
 *    9d. AMT_W2P_OUTSIDE is decided on (xs, ys) against the RAW frame: with a lens params.width x params.height is the raw
 *        frame's size (= the model's width x height), and the corrected, cropped size is the model's crop size (the header's
 *        IMAGEW / IMAGEH).  Without a lens that is the frame of step 7.
 *    Elevation, HIDDEN, UNPROJECTABLE and NOT_CONVERGED are as without a lens.  Any zenithal header, SIP included, may carry a
 *    lens at this level.
 * xy is NaN exactly where INVALID, UNPROJECTABLE, NOT_CONVERGED or LENS_FOLD is set; it stays a number for points that are only hidden or
 * outside the frame (a drawn line needs its off-frame end).  c1 is taken modulo 360 into [-180, 180): 180, -180 and 540 give the
 * same bits; c0 = +-90 is a valid point.
 * amt_world_to_pixel: n points, c0 / c1 / out_elev (optional) / out_flags of n elements, out_xy (n, 2) float64 [x, y].
 * amt_grid_to_pixel: the outer product of two axes, point (i, j) = (lat_centres[i], lon_centres[j]) - the cell centres of a
 * plate carree grid, which are never materialised; outputs (ny, nx[, 2]); out_xy32 is the float32 array amt_remap_coords takes,
 * the float64 value rounded once; out_xy32 and out_xy are each optional, but one of them is required.  The two entry points share their device
 * functions and give identical bits for identical points.  AMT_EINVAL (nothing written): NULL required pointers, n < 0, an
 * empty axis or frame, an unknown `frame`, a projection index out of range, a SIP order >= AMT_SIP_MAX, a singular CD matrix.
 * n = 0 is AMT_OK.  Both only enqueue work on the context's stream.
 * amt_world_to_pixel_lens, amt_grid_to_pixel_lens: the same argument lists plus `lens` (NULL or kind AMT_LENS_NONE: no lens, and
 * the bits of the calls without; those are calls of these with NULL - one kernel family).  AMT_EINVAL as well for an unknown
 * lens kind, a non-positive raw size, a crop window outside the full corrected frame, a raw size (the model's width x height)
 * that is not params' width x height, and a corrected size (the crop size, or the raw size without crop) that is not the camera
 * model's frame where that is known: zenithal's width x height.  With zenithal absent the params hold the raw size alone and
 * the camera model's frame cannot be checked. */
#define AMT_W2P_GEODETIC 0
#define AMT_W2P_SM 1
#define AMT_W2P_J2000 2
#define AMT_W2P_INVALID 1
#define AMT_W2P_HIDDEN 2
#define AMT_W2P_UNPROJECTABLE 4
#define AMT_W2P_NOT_CONVERGED 8
#define AMT_W2P_OUTSIDE 16
#define AMT_W2P_LENS_FOLD 32
int amt_world_to_pixel(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                       const double* c0, const double* c1, int64_t n, double* out_xy, double* out_elev, uint8_t* out_flags);
int amt_grid_to_pixel(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                      const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx, float* out_xy32, double* out_xy,
                      double* out_elev, uint8_t* out_flags);
int amt_world_to_pixel_lens(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                            const double* c0, const double* c1, int64_t n, double* out_xy, double* out_elev, uint8_t* out_flags,
                            const amt_lens_model* lens);
int amt_grid_to_pixel_lens(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                           const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx, float* out_xy32,
                           double* out_xy, double* out_elev, uint8_t* out_flags, const amt_lens_model* lens);

/* ---- gather mosaic: a collection gathered onto one grid in one fused kernel (addition to ABI 10) --------------------------------
 * auromat_amd.resample.resampleGatherMosaic.  Every cell centre of one grid is projected through EVERY member's camera model
 * (the arithmetic of amt_grid_to_pixel above), the overlap rule elects one member per cell, and only that member's image is
 * sampled (the arithmetic of amt_remap_coords).  No per-member coordinate array is written anywhere.
 * A member: its amt_frame_params, an optional amt_zenithal_wcs (as amt_world_to_pixel takes them), img on the device,
 * (params.height, params.width, channels) in the call's sample type, an optional center_mask (height x width bytes, non-zero =
 * masked) and min_elevation (degrees; -inf or NaN: none).
 * The cells: either the axes form - point (i, j) = (lat_centres[i], lon_centres[j]), as amt_grid_to_pixel - or, when both axes are
 * NULL, the point form - cell_lat, cell_lon of (ny, nx) each (the centres of a rotated grid, rotated back: the pole plan).  frame:
 * AMT_W2P_GEODETIC or AMT_W2P_SM.
 * Member i SEES a cell iff
 *   1. the flag byte of its centre is 0 (steps 1-8 above),
 *   2. for AMT_INTERP_LINEAR / _LANCZOS4: the position rounded to float32 has support, 0 <= x <= width - 1 and 0 <= y <= height - 1
 *      (amt_remap_coords' support byte for the array amt_grid_to_pixel writes),
 *   3. its center_mask, if any, is clear at the nearest pixel (rint of the float64 x, y - half to even -, clamped to the frame),
 *   4. elev >= min_elevation, if one is set,
 * and its elevation is not NaN (a NaN elevation never wins).
 * rule 1 (the reference's drawing rule for mappings that may overlap): of the members that see the cell, the one with the
 * highest float64 line-of-sight elevation at the cell centre wins, the lower index on a tie.  rule 0: the lowest index that sees
 * the cell (for collections that promise no overlap: the rules differ only where that promise is broken).
 * The cell takes the winner's sample - linear / Lanczos-4 as "Sampling (both remap calls)" states it, on the float32-rounded
 * coordinates; AMT_INTERP_NEAREST: the pixel at (rint x, rint y) of the float64 coordinates, clamped -, out_elev the winner's
 * elevation, out_source its index, out_mask 0 and out_xy (optional, (ny, nx, 2) float64) the winner's coordinates.  Without a
 * seeing member: image 0, out_mask 1, out_source -1, out_elev and out_xy NaN.  Every output equals, bit for bit, what
 * amt_grid_to_pixel (amt_world_to_pixel for the point form) + amt_remap_coords give for the winning member alone.
 * One block makes a 32 x 32 tile of cells.  A tile with ONE winner whose taps fit a 48 x 48 window of that member's image samples
 * from the window staged in LDS; any other tile takes every cell's taps from its own winner's image in global memory; both give
 * the same bits.  debug (optional): force_path AMT_GATHER_PATH_CELL makes every tile do the latter; tile_path (optional, one byte
 * per tile, row-major) reports 0 nobody sees the tile, AMT_GATHER_PATH_STAGED or AMT_GATHER_PATH_CELL (nearest: always _CELL).
 * Only enqueues work on the context's stream (the member table goes to the context's workspace).  AMT_EINVAL (nothing written):
 * NULL required pointers, n_members < 1, an empty axis, both or neither coordinate form, an unknown frame (AMT_W2P_J2000
 * included), interpolation, rule or force_path, sample_bytes outside 1, 2, 4, channels outside 1, 3, 4, a member without image,
 * and whatever amt_world_to_pixel refuses in a member's model - the error names the member's index. */
#define AMT_INTERP_NEAREST 2
#define AMT_GATHER_PATH_AUTO 0
#define AMT_GATHER_PATH_STAGED 1   /* as AUTO */
#define AMT_GATHER_PATH_CELL 2
typedef struct amt_gather_member {
    amt_frame_params params;
    const amt_zenithal_wcs* zenithal;
    const void* img;
    const uint8_t* center_mask;
    double min_elevation;
} amt_gather_member;
typedef struct amt_gather_debug {
    int32_t force_path, reserved;
    uint8_t* tile_path;
} amt_gather_debug;
int amt_gather_mosaic(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame, const double* lat_centres,
                      int32_t ny, const double* lon_centres, int32_t nx, const double* cell_lat, const double* cell_lon,
                      int32_t sample_bytes, int32_t channels, int32_t interpolation, int32_t rule, void* out_img, uint8_t* out_mask,
                      double* out_elev, int32_t* out_source, double* out_xy, const amt_gather_debug* debug);

/* ---- supersampled gather mosaic: n x n sub-samples per cell, reduced in the same kernel (addition to ABI 10) ----------------------
 * auromat_amd.resample.resampleGather / resampleGatherMosaic with supersample > 1: for cells much coarser than a pixel.
 * Cell (i, j) of the ny x nx grid has n x n sub-samples (s, t), s, t = 0 ... n - 1, n = factor in 1 ... 8.  Their coordinates come
 * in the two forms of amt_gather_mosaic: the axes form - sub_lat[ny * n], sub_lon[nx * n], sub-sample (s, t) of cell (i, j) is the
 * point (sub_lat[i * n + s], sub_lon[j * n + t]) - or, when both axes are NULL, the point form - sub_cell_lat, sub_cell_lon of
 * (ny * n, nx * n) each, sub-sample (s, t) of cell (i, j) at [i * n + s][j * n + t].
 * For every sub-sample the kernel computes exactly what amt_gather_mosaic computes for a cell centre at that point: which members
 * see it (rules 1-4 above; a NaN elevation never wins), the winner by `rule`, the winner's sample in the image type (integer samples
 * are already rounded and clamped) and the winner's float64 elevation.  Then, per cell:
 *   out_count (uint8, ny x nx): the number of sub-samples with a winner, always written;
 *   the cell is valid iff count >= min_count, 1 <= min_count <= n * n; out_mask = !valid;
 *   a valid cell, integer samples: per channel S = the exact integer sum of the seen sub-samples' samples, the output
 *     rint((double)S / (double)count), half to even;
 *   a valid cell, float32 samples: per channel the float64 sum of the seen sub-samples in row-major order (s outer, t inner), which
 *     the first seen value starts, divided by (double)count and rounded to float32;
 *   out_elev: the float64 sum of the seen sub-samples' elevations in the same order, divided by (double)count;
 *   out_source: the member that won the most sub-samples, the lower index on a tie;
 *   an invalid cell: image 0, out_source -1, out_elev NaN (out_count still the real count).
 * There is no out_xy.  factor 1 with min_count 1 gives amt_gather_mosaic's outputs bit for bit.
 * One block makes T x T cells, T = 32 / factor (integer division): at most 32 x 32 sub-sample points, elected and sampled by the
 * code of amt_gather_mosaic's kernel, staged window or per-point taps alike, and reduced to cells through LDS; no array of the
 * sub-sample grid exists in device memory.  debug as above, per T x T tile: tile_path has ceil(ny / T) x ceil(nx / T) bytes, 0 nobody
 * sees any sub-sample of the tile, AMT_GATHER_PATH_STAGED all winners of the tile are one member and their taps fit the window,
 * AMT_GATHER_PATH_CELL any other tile (nearest: always); force_path AMT_GATHER_PATH_CELL gives the same bits.
 * Only enqueues work on the context's stream (the member table goes to the context's workspace).  AMT_EINVAL (nothing written):
 * everything amt_gather_mosaic refuses, factor outside 1 ... 8, min_count outside 1 ... factor * factor, NULL out_count, and a
 * sub-sample grid whose side does not fit an int32. */
int amt_gather_mosaic_supersampled(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                   const double* sub_lat, int32_t ny, const double* sub_lon, int32_t nx, const double* sub_cell_lat,
                                   const double* sub_cell_lon, int32_t factor, int32_t min_count, int32_t sample_bytes,
                                   int32_t channels, int32_t interpolation, int32_t rule, void* out_img, uint8_t* out_mask,
                                   double* out_elev, int32_t* out_source, uint8_t* out_count, const amt_gather_debug* debug);

/* ---- gathered frames: a batch of frames, each onto a grid of its own, in one launch (addition to ABI 10) --------------------------
 * auromat_amd.resample.gather_frames, auromat_amd.pipeline.GatherSequence.  n_jobs jobs, 1 ... AMT_GATHER_MAX_JOBS.  A job is one
 * amt_gather_member, its grid - ny, nx and lat / lon (the axes form) or, when both are NULL, cell_lat / cell_lon (the point form),
 * as amt_gather_mosaic takes them; with factor > 1 the sub-sample axes (ny * factor, nx * factor) or points
 * (ny * factor, nx * factor each) as amt_gather_mosaic_supersampled takes them - and its outputs: out_img (ny, nx, channels),
 * out_mask, out_elev and, required with factor > 1 and not touched with factor 1, out_count.  Per call: frame, factor 1 ... 8,
 * min_count 1 ... factor * factor, sample_bytes, channels, interpolation.  Images of different sizes and jobs of either
 * coordinate form may share a call.
 * Job k's outputs are, byte for byte and in every cell, the masked ones included, what amt_gather_mosaic (factor 1) or
 * amt_gather_mosaic_supersampled (factor > 1) writes for a table of that one member on that grid.  There is no out_source and no
 * out_xy.
 * One launch over the sum of the jobs' tiles (32 / factor cells on a side); a block finds its job in a prefix table of tile
 * counts and runs the device code of the two kernels above on that job's tile.  debug: force_path as above; tile_path holds the
 * jobs' tiles one job after the other, each job's row-major as the per-job call reports them.
 * Only enqueues work on the context's stream (the job table goes to the context's workspace).  AMT_EINVAL (nothing written):
 * everything the two calls above refuse - for what belongs to a job the error names the job's index -, n_jobs outside
 * 1 ... AMT_GATHER_MAX_JOBS, out_count NULL with factor > 1, and a total tile count beyond INT32_MAX. */
#define AMT_GATHER_MAX_JOBS 64
typedef struct amt_gather_job {
    amt_gather_member member;
    int32_t ny, nx;
    const double* lat;          /* axes form */
    const double* lon;
    const double* cell_lat;     /* point form */
    const double* cell_lon;
    void* out_img;
    uint8_t* out_mask;
    double* out_elev;
    uint8_t* out_count;
} amt_gather_job;
int amt_gather_frames(amt_ctx* ctx, const amt_gather_job* jobs, int32_t n_jobs, int32_t frame, int32_t factor, int32_t min_count,
                      int32_t sample_bytes, int32_t channels, int32_t interpolation, const amt_gather_debug* debug);

/* ---- gathering through the lens (additions to ABI 10) ---------------------------------------------------------------------------
 * The three gather entry points for members that are RAW frames still carrying their lens distortion: the existing argument
 * lists plus `lenses`, one pointer per member (per job for amt_gather_frames_lens); a NULL entry, an entry of kind AMT_LENS_NONE
 * or a NULL array means no lens, and the calls without _lens are these with a NULL array (one kernel family; members with and
 * without a lens mix freely).  A member with a lens is projected by steps 1-9 of world -> pixel (the arithmetic of
 * amt_grid_to_pixel_lens, bit for bit), and "member i sees a cell" reads the same four rules on the raw coordinates: flag byte
 * 0, support of the float32-rounded (xs, ys) in the raw frame, center_mask at the nearest raw pixel, min_elevation.  The img
 * and center_mask of such a member are the raw frame's, params.width x params.height = the model's width x height; out_xy is
 * (xs, ys).  The raw pixels are interpolated once; no corrected image and no coordinate array is made.
 * AMT_EINVAL (nothing written; the text names the member or job) as the calls without _lens, and for what
 * amt_world_to_pixel_lens refuses in a lens. */
int amt_gather_mosaic_lens(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame, const double* lat_centres,
                           int32_t ny, const double* lon_centres, int32_t nx, const double* cell_lat, const double* cell_lon,
                           int32_t sample_bytes, int32_t channels, int32_t interpolation, int32_t rule, void* out_img,
                           uint8_t* out_mask, double* out_elev, int32_t* out_source, double* out_xy, const amt_gather_debug* debug,
                           const amt_lens_model* const* lenses);
int amt_gather_mosaic_supersampled_lens(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                        const double* sub_lat, int32_t ny, const double* sub_lon, int32_t nx,
                                        const double* sub_cell_lat, const double* sub_cell_lon, int32_t factor, int32_t min_count,
                                        int32_t sample_bytes, int32_t channels, int32_t interpolation, int32_t rule, void* out_img,
                                        uint8_t* out_mask, double* out_elev, int32_t* out_source, uint8_t* out_count,
                                        const amt_gather_debug* debug, const amt_lens_model* const* lenses);
int amt_gather_frames_lens(amt_ctx* ctx, const amt_gather_job* jobs, int32_t n_jobs, int32_t frame, int32_t factor, int32_t min_count,
                           int32_t sample_bytes, int32_t channels, int32_t interpolation, const amt_gather_debug* debug,
                           const amt_lens_model* const* lenses);

/* auromat/coordinates/intersection.py:144-163 ellipsoidLineIntersection (and
 * auromat/mapping/mapping.py:1474-1510 inflatedEarthIntersection with a=wgs84A+h, b=wgs84B+h).
 * origin: host double[3]; dirs/out: (n,3) AoS.  Misses / points behind a directed ray are NaN. */
int amt_intersect_ellipsoid(amt_ctx* ctx, double a, double b, const double* origin, const double* dirs,
                            int64_t n, int directed, double* out_xyz);
/* auromat/coordinates/intersection.py:229-237 ellipsoidLineIntersects -> uint8 (0/1). */
int amt_intersects_ellipsoid(amt_ctx* ctx, double a, double b, const double* origin, const double* dirs,
                             int64_t n, int directed, uint8_t* out_hit);
/* auromat/coordinates/intersection.py:12-48 sphereLineIntersection (earthModel='sphere'). */
int amt_intersect_sphere(amt_ctx* ctx, double radius, const double* origin, const double* dirs,
                         int64_t n, int directed, double* out_xyz);

/* auromat/coordinates/transform.py:199-297 ecef2Geodetic (Bowring 1985) -> radians. */
int amt_ecef_to_geodetic(amt_ctx* ctx, const double* x, const double* y, const double* z, int64_t n,
                         double a, double b, double* out_lat, double* out_lon);
/* auromat/coordinates/transform.py:156-178 geodetic2Ecef (radians in, scalar height). */
int amt_geodetic_to_ecef(amt_ctx* ctx, const double* lat, const double* lon, double h, int64_t n,
                         double a, double b, double* out_x, double* out_y, double* out_z);
/* auromat/coordinates/transform.py:324-343 j2000ToLatLon with the 3x3 (host, row major) given:
 * rotate (n,3) AoS points, Bowring, degrees out.  Also serves x_to_y-based geo helpers. */
int amt_rotate_to_latlon(amt_ctx* ctx, const double* m, const double* xyz, int64_t n, double a0, double b0,
                         double* out_lat_deg, double* out_lon_deg);
/* auromat/coordinates/transform.py:403-459 j2000ToMLatMLT / geoToMLatMLT: rotate into SM,
 * mlat = deg(atan2(z, hypot(x,y))), mlt = deg(atan2(y,x))*24/360 + 12. */
int amt_rotate_to_mlat_mlt(amt_ctx* ctx, const double* m, const double* xyz, int64_t n,
                           double* out_mlat_deg, double* out_mlt_h);
/* auromat/coordinates/transform.py:728-738 x_to_y: out = m @ v for (n,3) AoS vectors. */
int amt_rotate_vectors(amt_ctx* ctx, const double* m, const double* xyz, int64_t n, double* out_xyz);
/* auromat/mapping/mapping.py:540-550 BaseMapping._mLatMlt: geodetic (deg) at height h -> ECEF ->
 * SM (m = mat_geo_to_sm) -> MLat/MLT.  NaN in, NaN out. */
int amt_latlon_to_mlat_mlt(amt_ctx* ctx, const double* m, const double* lat_deg, const double* lon_deg,
                           double h, int64_t n, double a0, double b0, double* out_mlat_deg, double* out_mlt_h);
/* auromat/coordinates/transform.py:461-485 smToLatLon: SM lat/lon (deg) on the unit sphere ->
 * GEO (m = transpose of mat_geo_to_sm, passed already transposed) -> geodetic deg. */
int amt_sm_to_latlon(amt_ctx* ctx, const double* m_sm_to_geo, const double* smlat_deg, const double* smlon_deg,
                     int64_t n, double a0, double b0, double* out_lat_deg, double* out_lon_deg);

/* ---- map projections (additions to ABI v10; auromat_amd.coordinates.projection) --------------------------------------
 * Two projections onto an equal-scale map plane, forward and inverse; angles in degrees, lengths in the unit of a / radius.
 * Snyder, Map Projections - A Working Manual, ch. 21 and 25 (PROJ's stere and aeqd; the reference draws on Basemap's
 * 'stere' with ellps='WGS84' and 'npaeqd' / 'spaeqd', auromat/draw.py:319-385).
 *   stereographic, ellipsoid (a, b), centre (lat0, lon0), scale 1 at the centre: with chi the conformal latitude,
 *     D = 1 + sin chi1 sin chi + cos chi1 cos chi cos dlon,  x = k cos chi sin dlon / D,
 *     y = k (cos chi1 sin chi - sin chi1 cos chi cos dlon) / D,  k = 2 a m1 / cos chi1;
 *     the polar form when 90 - |lat0| < 1e-8 deg: sin chi1 = +-1, cos chi1 = 0, k = 2 a / sqrt((1+e)^(1+e) (1-e)^(1-e)).
 *   polar azimuthal equidistant, sphere: rho = radius (pi/2 -+ lat), x = rho sin dlon, y = -rho cos dlon (north) /
 *     +rho cos dlon (south).
 * Domain of the forward direction: a point more than 90 deg from the centre (stereographic: on the conformal sphere, D < 1;
 * equidistant: the other hemisphere) gives NaN in both outputs, as does a NaN or infinite input.
 * Inverse: the centre maps to (lat0, lon0); lon in [-180, 180); a NaN or infinite input gives NaN in both outputs (and the
 * equidistant form beyond rho = pi radius, where no latitude exists).
 * amt_projection is filled by the two host functions below (no GPU call; AMT_EINVAL for |lat0| > 90, non-finite arguments,
 * b > a, a, b or radius <= 0, NULL) and passed to the device calls as a HOST pointer. */
#define AMT_PROJ_STEREOGRAPHIC 1
#define AMT_PROJ_POLAR_AEQD 2
typedef struct amt_projection {
    int32_t kind;               /* AMT_PROJ_* */
    int32_t mode;               /* 0: oblique (or equatorial), +1 / -1: the north / south polar form */
    double lat0, lon0;          /* the centre, degrees */
    double a, e;                /* semi-major axis or radius; eccentricity (0: sphere) */
    double sin_chi1, cos_chi1;  /* conformal latitude of the centre (exactly +-1 and 0 in the polar forms) */
    double m1;                  /* cos lat0 / sqrt(1 - e^2 sin^2 lat0) (0 in the polar forms) */
    double k;                   /* the length constant above (equidistant: the radius) */
    double reserved[4];
} amt_projection;
int amt_projection_stereographic(double lat0, double lon0, double a, double b, amt_projection* out);
int amt_projection_polar_aeqd(int north, double lon0, double radius, amt_projection* out);
/* n >= 0 points, elementwise; enqueue only; alignment: any. */
int amt_project_forward(amt_ctx* ctx, const amt_projection* p, const double* lat_deg, const double* lon_deg, int64_t n,
                        double* out_x, double* out_y);
int amt_project_inverse(amt_ctx* ctx, const amt_projection* p, const double* x, const double* y, int64_t n,
                        double* out_lat_deg, double* out_lon_deg);
/* auromat/coordinates/transform.py:301-322 rotatePole: geodetic (rad) at `altitude` rotated by the
 * 3x3 `rot` (host) about the origin, back to geodetic (rad). */
int amt_rotate_pole(amt_ctx* ctx, const double* rot, const double* lat, const double* lon, double altitude,
                    int64_t n, double a0, double b0, double* out_lat, double* out_lon);
/* The same with degrees in and out (lat_deg * pi/180 -> amt_rotate_pole -> * 180/pi, rounding for rounding what
 * np.deg2rad / np.rad2deg around the call give): what the pole branch of the resampling works in
 * (auromat/resample.py:176-201,262-273). */
int amt_rotate_pole_deg(amt_ctx* ctx, const double* rot, const double* lat_deg, const double* lon_deg, double altitude,
                        int64_t n, double a0, double b0, double* out_lat_deg, double* out_lon_deg);
/* auromat/coordinates/transform.py:142-154 cartesian_to_spherical -> (r, lat, lon) radians; out_r may be NULL. */
int amt_cartesian_to_spherical(amt_ctx* ctx, const double* x, const double* y, const double* z, int64_t n,
                               double* out_r, double* out_lat, double* out_lon);
/* auromat/coordinates/transform.py:89-102 spherical_to_cartesian; r may be NULL (unit sphere). */
int amt_spherical_to_cartesian(amt_ctx* ctx, const double* r, const double* lat, const double* lon, int64_t n,
                               double* out_x, double* out_y, double* out_z);

/* ---- other camera models feeding the same intersection + geodetic steps -------- */

/* Equidistant all-sky (fisheye) calibration of one ground station, auromat/mapping/miracle.py:28-35,314-347
 * (FMI MIRACLE cal.txt: zenith pixel (xc vertical, yc horizontal), d = k*z, CCW rotation in rad), already
 * scaled to the image size (miracle.py:320-326), with the station's position and local-frame rotation. */
typedef struct amt_allsky_params {
    int32_t size;             /* image is size x size pixels */
    int32_t reserved;
    double xc, yc, k;         /* pixels, pixels, pixels per radian of zenith angle */
    double rotation;          /* radians */
    double center_offset;     /* added to the integer index of a pixel CENTRE (0.5; the reference run under its
                                 pinned NumPy 1.6 adds 0: `ind += 0.5` on an integer array, miracle.py:333-334) */
    double to_geo[9];         /* row-major R_z(-lon) . R_y(90deg - lat), miracle.py:249-252 */
    double station[3];        /* geodetic2EcefZero(lat, lon) in km, miracle.py:139-140 */
    double a, b;              /* shell semi-axes in km: wgs84A + altitude, wgs84B + altitude */
    double a0, b0;            /* wgs84A, wgs84B */
} amt_allsky_params;

/* MIRACLEMapping.calculateAzEl -> _calculateCameraToPixelDirection -> intersectionInflated* -> _calculateLatsLons
 * (auromat/mapping/miracle.py:196-258,314-347) for every pixel corner (corner=1: (size+1)^2 points) or centre
 * (corner=0: size^2 points) in one launch.  Every output may be NULL: az_deg in [0,360), el_deg = 90 - deg(d/k),
 * dirs (n,3) AoS unit vectors in GEO, lat_deg / lon_deg of the shell intersection. */
int amt_georef_allsky(amt_ctx* ctx, const amt_allsky_params* p, int corner, double* az_deg, double* el_deg,
                      double* dirs, double* lat_deg, double* lon_deg);

/* auromat/mapping/themis.py:224-253 reproject: coordinates given on the shell at height_ref (km above the
 * ellipsoid) as seen from the station at (station_lat_deg, station_lon_deg, height 0) -> the same lines of sight
 * on the shell at height_new.  Degrees in and out; NaN in, NaN out. */
int amt_reproject_altitude(amt_ctx* ctx, double station_lat_deg, double station_lon_deg, const double* lat_ref_deg,
                           const double* lon_ref_deg, int64_t n, double height_ref, double height_new,
                           double a0, double b0, double* out_lat_deg, double* out_lon_deg);

/* ---- fused frame kernel ------------------------------------------------------------- */

/* All lazy arrays of a BaseAstrometryMapping in one launch
 * (auromat/mapping/astrometry.py:49-212: cameraToPixel*Direction -> intersectionInflated* ->
 * _latsLonsCorner/_latsLonsCenter -> elevation -> mLatMlt[Center]).  Directions are generated
 * in-kernel from the WCS; fast_center selects the corner-mean centres (astrometry.py:100-101,154-160)
 * or the exact per-centre ray cast (:103-105). */
int amt_georef_frame(amt_ctx* ctx, const amt_frame_params* p, const amt_georef_out* out);
/* Same with caller-supplied corner directions ((height+1, width+1, 3) AoS, e.g. from another
 * camera model; SURVEY.md §8d "directions-in" variant).  fast_center must be 1. */
int amt_georef_frame_dirs(amt_ctx* ctx, const amt_frame_params* p, const double* corner_dirs,
                          const amt_georef_out* out);
/* Cheap estimate of the same bbox[0..6] from every `stride`-th pixel corner in both directions (a
 * 1/stride^2 sample of the rays): a corner counts when the elevation of its own ray is >= min_elevation.
 * With magnetic == 1 the box is in (MLat, SM longitude) instead of (lat, lon), with magnetic == 2 in (lat, lon)
 * rotated by +90 deg about x at the altitude a - a0 (the pole plan, amt_georef_out.bin_pole), with magnetic == 3 in
 * (MLat, SM longitude) rotated likewise.  Used to lay out a superset
 * grid for the fused binning before the full kernel runs; the caller adds a safety margin and checks the
 * exact box afterwards.  bbox[7] = sx * 2^20 + sy, where sx (sy) is the number of sampled rays that hit the
 * shell right of (below) the frame centre minus those left of (above) it: the input of amt_georef_out.item_order. */
int amt_georef_coarse_bbox(amt_ctx* ctx, const amt_frame_params* p, int32_t stride, double min_elevation,
                           int magnetic, double* bbox);
/* The same estimate for caller-supplied corner directions (amt_georef_frame_dirs): every `stride`-th direction of
 * corner_dirs ((height+1, width+1, 3), J2000) is cast instead of the TAN model's.  magnetic 0 or 1 (direction arrays have
 * no pole plan). */
int amt_georef_coarse_bbox_dirs(amt_ctx* ctx, const amt_frame_params* p, const double* corner_dirs, int32_t stride,
                                double min_elevation, int magnetic, double* bbox);
/* Host function (no GPU call): which rows of amt_georef_frame's work items cannot see the shell.  With the TAN camera
 * model the limb is a conic section in the image and the set of pixel corners whose ray hits the shell is convex, so
 * whole bands of the frame are bounded exactly from a handful of evaluations; the waves of such bands write NaN and
 * cast no ray.  An item is `rows_per_item` pixel rows tall; the frame has `n_item_rows` rows of items; rows
 * [0, top_end) and [bottom_begin, n_item_rows) are free of hits (conservative: within 1e-9 of the limb a band counts
 * as seeing the Earth).  Replaces nothing in the reference — it evaluates every ray (wcs.py:18-144,
 * intersection.py:58-104) — and changes no result. */
int amt_georef_sky_rows(const amt_frame_params* p, int32_t* rows_per_item, int32_t* n_item_rows, int32_t* top_end,
                        int32_t* bottom_begin);
/* Host function (no GPU call): the pixel rows [*row_begin, *row_end) of a camera frame's IMAGE that the fused binning can need
 * — a pixel's colours are read only to bin it, and only pixels whose ray hits the shell with an elevation >= min_elevation are
 * binned (reference mapping.py:845-864 maskedByElevation, resample.py:119-120,315-321).  Bounded from the camera model alone: the
 * limb as above, and the cone about the nadir inside which the elevation can reach min_elevation (law of sines in the triangle
 * Earth's centre / camera / hit point: sin(nadir angle) = |P| / |C| cos(elevation), |P| <= the shell's larger semi-axis).
 * Conservative, at the granularity of the work items' rows; min_elevation <= 0 or -inf: the rows a ray can hit.  What a host
 * that holds the image in page-locked memory has to send (amt_run_frame.img_host does exactly that). */
int amt_georef_image_rows(const amt_frame_params* p, double min_elevation, int32_t* row_begin, int32_t* row_end);

/* ---- mask rules ---------------------------------------------------------------------- */

/* auromat/mapping/mapping.py:845-864 maskedByElevation + the lazy _doSanitize(afterMasking=True)
 * of mapping.py:1063-1125,1161-1213.  Masks are uint8, 1 = masked.
 * center_mask[h*w] = !(elev >= min_elevation) (NaN counts as masked);
 * corner_mask[(h+1)*(w+1)] = isnan(corner_lat) | all adjacent centres masked.
 * n_valid (device int64, optional) receives the number of unmasked centres; the host raises
 * ValueError when it is 0 (AMT_EEMPTY is not raised here because the call does not synchronise). */
int amt_mask_by_elevation(amt_ctx* ctx, const double* elev, const double* corner_lat, int32_t height,
                          int32_t width, double min_elevation, uint8_t* center_mask, uint8_t* corner_mask,
                          int64_t* n_valid);
/* auromat/mapping/mapping.py:1063-1125 _doSanitize on boolean masks (in place).
 * img_mask may be NULL; after_masking as in the reference. */
int amt_sanitize_masks(amt_ctx* ctx, uint8_t* corner_mask, uint8_t* center_mask, const uint8_t* img_mask,
                       int32_t height, int32_t width, int after_masking);
/* auromat/utils.py:97-151 outline (skimage.measure.find_contours(padded mask, 0.99), rounded): the contour links of
 * a (height, width) uint8 mask (1 = masked).  For every unmasked pixel p (flat index i) and every direction d
 * (0 up, 1 right, 2 down, 3 left) whose 4-neighbour is masked or outside, one record links[2k] = 4*i + d,
 * links[2k+1] = the key of the crossing that follows it on the contour (unmasked region on the right-hand side, i.e.
 * clockwise in image coordinates; unmasked pixels are joined through edges only).  Records come in no particular order;
 * *count (device uint64, zeroed by the call) receives their number, which may exceed `capacity` (then only the first
 * `capacity` were written: call again with a larger buffer).  Following the links from any key yields one closed
 * contour; the pixel of each key (key / 4), with consecutive duplicates dropped, is the polygon the reference traces. */
int amt_mask_outline_links(amt_ctx* ctx, const uint8_t* mask, int32_t height, int32_t width, int64_t* links,
                           int64_t capacity, uint64_t* count);
/* auromat/draw_helpers.py:34-94 createPolygonsAndColors + filterNanPolygons for the pixels listed in `index` (n flat
 * pixel indices, normally the unmasked ones in row-major order): verts (n,4,2) float64 = (lat, lon) of the corners
 * (r,c), (r,c+1), (r+1,c+1), (r+1,c); colours per pixel as the mapping's `rgb` gives them (mapping.py:980-1007: uint8 as
 * is, uint16 * (255/65535) truncated; one channel is repeated): colors_u8 (n,3) and / or colors_f64 (n,3) = rgb / 255
 * (ColorMode.matplotlib); either may be NULL.  lat/lon: (height+1, width+1); img: (height, width, nchan), nchan 1 or 3. */
int amt_pixel_polygons(amt_ctx* ctx, const double* lat, const double* lon, const void* img, int32_t img_dtype,
                       int32_t nchan, int32_t height, int32_t width, const int64_t* index, int64_t n, double* verts,
                       uint8_t* colors_u8, double* colors_f64);
/* Inputs of BaseMapping.boundingBox (mapping.py:693-743) for arbitrary corner grids:
 * bbox[0..5] = min/max over unmasked corners as in amt_georef_out.bbox, bbox[6] = number of unmasked
 * corners, bbox[7] = number of unmasked centres whose corner quad winds around a pole.
 * corner_mask / center_mask may be NULL (then NaN latitude = masked; a centre is unmasked when its
 * four corners are). lat/lon: (height+1, width+1) degrees. */
int amt_bbox_corners(amt_ctx* ctx, const double* lat, const double* lon, const uint8_t* corner_mask,
                     const uint8_t* center_mask, int32_t height, int32_t width, double* bbox);

/* ---- histogram binning / plate-carree resampling ------------------------------------- */

/* Bin-edge description of one axis, reference semantics of auromat/util/histogram.py:178-224:
 * index = searchsorted(edges, v, 'right') (0 and nbin+1 are outliers), and values v >= edges[nbin]
 * with rint(v*scale)/scale == last_rounded fall into the last bin.  `scale` = 10**decimal and
 * `last_rounded` = around(edges[-1], decimal) are computed by the host exactly as the reference does.
 * uniform = 0: `edges` is a DEVICE array of nbin+1 ascending doubles, searched by bisection.
 * uniform = 1: the edges are exactly what np.linspace(first, last, nbin+1) produces, i.e.
 *   edges[i] = fl(fl(i*step) + first) for i < nbin (two roundings, no FMA), edges[nbin] = last, with
 *   step = (last-first)/nbin; the kernel evaluates them in registers (O(1) guess + exact fix-up) and
 *   `edges` may be NULL.  The host must have verified that identity for its edge array. */
typedef struct amt_axis {
    const double* edges;
    int32_t nbin;
    int32_t uniform;
    double first, last;   /* edges[0] and edges[nbin] */
    double step;          /* uniform axes: (last-first)/nbin */
    double scale;
    double last_rounded;
} amt_axis;

/* auromat/util/histogram.py:284-417,57-282 histogram2d(x, y, bins, range, weights=[None, w0, ...]).
 * Accumulates into count[nx*ny] and sums[k][nx*ny] (k < nweights; device pointers in the HOST array
 * `weights` / `sums`), all float64, row major (ix*ny + iy), which must be zeroed by the caller
 * (they may be accumulated over several calls).  NaN x or y are outliers; NaN weights poison
 * their cell (np.bincount behaviour).  lon_wrap != 0 bins wrap_at(x + 180, 180) instead of x
 * (auromat/resample.py:212-218, discontinuity branch). */
int amt_hist2d_accumulate(amt_ctx* ctx, const double* x, const double* y, int64_t n,
                          const double* const* weights, int32_t nweights, const amt_axis* xaxis,
                          const amt_axis* yaxis, int lon_wrap, double* count, double* const* sums);

/* Fused binning of one frame for resample(method='mean') (auromat/resample.py:95-142,301-351):
 * pixels with finite lat_c, elev >= min_elevation (pass -inf to disable; NaN elev is dropped when a
 * finite threshold is given) and center_mask == 0 (mask may be NULL) add 1, their image channels
 * and their elevation to cell (ix, iy), x = lon_c, y = lat_c.
 * img: (n, nchan) interleaved uint8 (img_dtype=1) or uint16 (img_dtype=2), nchan <= 4.
 * acc: device uint64[(nchan+2) * nx*ny] workspace, zeroed by the caller:
 *   plane 0 = count, planes 1..nchan = exact integer channel sums,
 *   plane nchan+1 = elevation sum in signed 31.32 fixed point (|error| <= 2^-33 deg per sample;
 *   order independent, so results are bit-reproducible; 2^63 / (90 * 2^32) = 2.38e7 pixels of 90 deg fit into one cell).
 * The call ADDS to acc: several frames (or row bands of one frame) may be binned into one accumulator.
 * Alignment: any.  The fast (vector) path needs an even width, lat_c / lon_c / elev 16-byte aligned and img 4-byte aligned;
 * otherwise (e.g. img is a slice of a uint8 / uint16 array) the launch takes the scalar path.  Same results either way. */
int amt_bin_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev,
                  const void* img, int32_t img_dtype, int32_t nchan, const uint8_t* center_mask,
                  int32_t height, int32_t width, double min_elevation, const amt_axis* xaxis,
                  const amt_axis* yaxis, int lon_wrap, uint64_t* acc);
/* Mean + layout of auromat/resample.py:339-351 and :128-136: for out row r (lat descending) and
 * column c: cell (ix=c, iy=ny-1-r).  mean: (ny, nx, nchan+1) float64, NaN where count == 0;
 * out_img (optional): (ny, nx, nchan) of img_dtype, round-half-even of the mean (0 where empty);
 * out_mask (optional): (ny, nx) uint8, 1 where count == 0; out_count (optional): (ny, nx) float64. */
int amt_bin_frame_finalize(amt_ctx* ctx, const uint64_t* acc, int32_t nx, int32_t ny, int32_t nchan,
                           int32_t img_dtype, double* mean, void* out_img, uint8_t* out_mask,
                           double* out_count);
/* Same on a window of a larger accumulator: acc has acc_nx x acc_ny cells per plane (the superset grid of
 * a fused amt_georef_frame launch); the output covers its cells [off_x, off_x+nx) x [off_y, off_y+ny). */
int amt_bin_frame_finalize_window(amt_ctx* ctx, const uint64_t* acc, int32_t acc_nx, int32_t acc_ny,
                                  int32_t off_x, int32_t off_y, int32_t nx, int32_t ny, int32_t nchan,
                                  int32_t img_dtype, double* mean, void* out_img, uint8_t* out_mask,
                                  double* out_count);
/* Area-weighted (conservative) binning (auromat_amd.resample.resampleArea; no counterpart in the reference): a pixel is the
 * quadrilateral of its corners (r, c), (r, c+1), (r+1, c+1), (r+1, c) of the corner arrays lat / lon ((height+1) x (width+1),
 * x = lon, y = lat; lon_wrap as for amt_bin_frame, applied to every corner), and every cell that it overlaps receives it with
 * the integer weight W = rint(A / cell area * 2^32), A the absolute signed (winding) area of quadrilateral and cell rectangle
 * (the rectangle between the axis's own edge values); a cell with W = 0 receives nothing.  A pixel takes part when lat_c is
 * finite, elev >= min_elevation (-inf: no threshold; elev may be NULL), center_mask == 0 (may be NULL), all eight corner values
 * are finite and the quadrilateral's x extent (after the wrap) is below 180.  The cell that holds the centre plays no role.
 * acc: the layout of amt_bin_frame, zeroed by the caller, ADDED to: plane 0 = sum(W), planes 1..nchan = sum(W * channel),
 * plane nchan+1 = sum(W * E), E = rint(elev * 2^16) (0 for a NaN elevation).  64-bit integer atomics: exact, order
 * independent, bit-reproducible.  Alignment: any. */
int amt_area_frame(amt_ctx* ctx, const double* lat, const double* lon, const double* lat_c, const double* elev, const void* img,
                   int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                   double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, uint64_t* acc);
/* amt_area_frame on a map plane (addition to ABI v10): the corner arrays are the projected x and y ((height+1) x (width+1),
 * e.g. from amt_project_forward), the axes are uniform (else AMT_EINVAL) and in the plane's unit.  x is no longitude: there is
 * no lon_wrap and NO rule on the quadrilateral's x extent — a pixel takes part when lat_c is finite, the elevation threshold
 * holds, center_mask == 0 and all eight projected corner values are finite (a corner outside the projection's domain is NaN).
 * Weights, candidate cells, accumulator layout, the ADDING to acc (the members of a collection can share one accumulator)
 * and the 2^40 limit are amt_area_frame's; amt_area_frame_finalize finishes it.  Alignment: any. */
int amt_area_plane_frame(amt_ctx* ctx, const double* x, const double* y, const double* lat_c, const double* elev,
                         const void* img, int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height,
                         int32_t width, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, uint64_t* acc);
/* Weighted means in the layout of amt_bin_frame_finalize.  A cell is valid when sum(W) >= max(1, min_weight) (min_weight =
 * rint(minimum coverage * 2^32)).  area (optional): (ny, nx, nchan+1) float64, sum(W * v) / sum(W), the elevation
 * sum(W * E) / sum(W) / 65536, NaN where invalid; out_img (optional): round-half-even of the value, 0 where invalid; out_mask
 * (optional): 1 where invalid; out_coverage (optional): sum(W) / 2^32 for every cell.  Reads one device flag back
 * (synchronises): AMT_EDOMAIN when a cell's sum(W) exceeds 2^40 (covered more than 256 times over; the products could wrap) —
 * the outputs are then unspecified. */
int amt_area_frame_finalize(amt_ctx* ctx, const uint64_t* acc, int32_t nx, int32_t ny, int32_t nchan, int32_t img_dtype,
                            uint64_t min_weight, double* area, void* out_img, uint8_t* out_mask, double* out_coverage);
/* amt_area_frame and amt_area_frame_finalize in ONE call that only enqueues on the context's stream (addition to ABI v10): it
 * reads nothing back and waits for nothing — except that growing the context's workspace synchronises, as for
 * amt_median_frame_async.  The accumulators are (nchan + 2) * nx * ny uint64 of the context's workspace, zeroed by every call;
 * consecutive calls run in stream order and share them.  Same argument checks, weights, admission rules, candidate cells and
 * finalise arithmetic as the two calls: for the same inputs every output has the same bits.  Outputs in the layout of
 * amt_area_frame_finalize, each optional.
 * lon_from_mlt != 0: lon holds the corners' MLT in hours; x = (mlt - 12.0) / (24.0 / 360.0), each operation rounded on its own
 * (auromat_amd.mapping.mapping.convertMappingToSM), before lon_wrap.
 * [row_begin, row_end), 0 <= row_begin <= row_end <= height (else AMT_EINVAL): only the pixels of these rows are visited;
 * whatever the arrays hold for the pixels of other rows plays no role.  An empty band: every cell masked, coverage 0.
 * over (optional): a device word the finalise kernel ORs 1 into when a cell's sum(W) exceeds 2^40 (the outputs of that frame are
 * then unspecified, as after AMT_EDOMAIN).  Never cleared here: the caller owns and zeroes it. */
int amt_area_frame_async(amt_ctx* ctx, const double* lat, const double* lon, const double* lat_c, const double* elev,
                         const void* img, int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height,
                         int32_t width, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                         int lon_from_mlt, int32_t row_begin, int32_t row_end, uint64_t min_weight, double* area, void* out_img,
                         uint8_t* out_mask, double* out_coverage, uint32_t* over);
/* Mesh resampling (addition to ABI v10; auromat_amd.resample.resampleMesh; no counterpart in the reference): linear
 * interpolation in the triangles of the pixel lattice itself, two per quad of neighbouring pixel centres.  DESIGN.md §4.6 is the
 * contract; in short:
 *   vertices   pixel (r, c), flat index r * width + c, at x = lon_c (after lon_wrap, as for amt_bin_frame), y = lat_c.  It takes
 *              part when lat_c is finite, elev >= min_elevation (-inf: no threshold; elev may be NULL), center_mask == 0 (may be
 *              NULL) and lon_c is finite.
 *   triangles  quad q = r * (width - 1) + c has A = (r, c), B = (r, c+1), C = (r+1, c+1), D = (r+1, c).  Four valid vertices:
 *              diagonal AC gives 2q = (A, B, C), 2q+1 = (A, C, D); diagonal BD gives 2q = (A, B, D), 2q+1 = (B, C, D).  Exactly
 *              three: their one triangle, id 2q.  Fewer: none.  A triangle whose x extent reaches 180 is dropped.
 *   diagonal   orient(P, Q, R) = (Qx-Px)*(Ry-Py) - (Qy-Py)*(Rx-Px).  AC is admissible when orient(A,B,C) and orient(A,C,D) are
 *              both > 0 or both < 0, BD when orient(A,B,D) and orient(B,C,D) are.  Both: BD exactly when D lies strictly inside
 *              the circle through A, B, C (3 x 3 in-circle determinant relative to D, with the sign of orient(A,B,C)), else AC.
 *              One: that one.  None: AC.
 *   edges      e_k of vertex k's opposite edge is orient(P, Q, cell centre) with P, Q the edge's end points in ascending flat
 *              index, negated when the triangle runs from the higher index to the lower.  A triangle holds a centre when its
 *              three values are all >= 0 or all <= 0 and not all zero (all zero: on the line of a triangle without area).
 *   election   of the triangles that hold a cell's centre the lowest id wins (32-bit atomic minimum; order independent).
 *   value      the winner's e_k with one common sign: v = ((e0*v0 + e1*v1) + e2*v2) / ((e0 + e1) + e2), every operation rounded
 *              on its own, in float64, per image channel (uint16 samples unsigned) and for the elevation (NaN without elev).
 * cell_lat (ny, north to south) / cell_lon (nx): the cell centres, each inside its cell of yaxis / xaxis (the candidate cells of a
 * triangle are those its bounding box meets, by amt_area_frame's rule); the axes may be uniform or edge tables.
 * Outputs in the layout of amt_bin_frame_finalize, each optional, at least one: mesh (ny, nx, nchan+1) float64, NaN where no
 * triangle holds the centre; out_img (ny, nx, nchan) of img_dtype, round-half-even of the value, 0 where masked; out_mask 1
 * where masked; out_triangle (ny, nx) int32 the winning id, -1 where masked.
 * claim: nx * ny uint32 of device memory of the caller's for the claim words (cell ix * ny + iy), whatever they hold: every
 * call sets them to 0xFFFFFFFF first, and leaves the winning ids there.  The call uses no memory of the context's, so it only
 * enqueues on the context's stream, whatever the shape: it reads nothing back, allocates nothing and waits for nothing, and its
 * results do not depend on what the context or the buffer held before.
 * AMT_EINVAL: height or width < 2, nchan outside 0..4, height * width or 2 * (height-1) * (width-1) not below 2^31, 65535 or more
 * bins on an axis, no output at all, claim NULL.  Alignment: any (claim: 4 bytes). */
int amt_mesh_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                   int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                   double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, const double* cell_lat,
                   const double* cell_lon, double* mesh, void* out_img, uint8_t* out_mask, int32_t* out_triangle, uint32_t* claim);
/* Median binning (auromat_amd.resample.resampleMedian; the reference names method='median' and leaves it unbuilt,
 * auromat/resample.py:353-357): the pixels amt_bin_frame would bin into cell (ix, iy) — same arguments, same membership —
 * and for every cell and channel np.median of their values: the order statistic of rank (n-1)/2, or for an even count n
 * the float64 mean (a + b) / 2 of ranks n/2 - 1 and n/2.  Exact and deterministic for any cell size.  Channel c < nchan:
 * the image channel; channel nchan: the elevation (NaN when elev is NULL).
 * Outputs in the layout of amt_bin_frame_finalize (rows north to south): median (ny, nx, nchan+1) float64, NaN where
 * empty; out_img (optional): (ny, nx, nchan) of img_dtype, round-half-even of the median (0 where empty); out_mask
 * (optional): 1 where empty; out_count (optional): pixels per cell.  Uses the context's workspace (about 6 + 2*nchan
 * (+8 with elev) bytes per pixel + 16 per cell, and 1060 bytes per channel for every 16385 pixels: the size
 * amt_median_frame_async needs for the same arguments).  Synchronises once: it reads how many cells hold more than 64 pixels. */
int amt_median_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                     int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                     double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, double* median,
                     void* out_img, uint8_t* out_mask, double* out_count);
/* amt_median_frame that only enqueues work (ABI v8): the same bits, no read-back and no host wait.  Every kernel goes on the
 * context's stream; the inputs must stay valid and the outputs untouched until the stream has run them, and the result is
 * ready in stream order.  The pass uses the workspace of the context's current stream (about 18 bytes per pixel for uint16
 * RGB plus elevation): passes enqueued one after the other on ONE stream may share it; passes that can run at the same time
 * need contexts (or streams) of their own.  (A call that needs a larger workspace than the stream has grows it, which
 * synchronises that stream once, as for every user of the workspace.)  The cells above 64 pixels are selected by one launch of a fixed grid that walks
 * the device's list of them; cells above 16384 pixels by one launch per digit position of the widest key (8 with the
 * elevation, 2 for uint16, 1 for uint8) plus one, which return at once when the frame has no such cell.
 * lon_from_mlt != 0: lon_c holds MLT hours, binned at the SM longitude (lon_c - 12) / (24 / 360) in float64, which is what
 * convertMappingToSM (auromat_amd/mapping/mapping.py) computes for resampleMedianMLatMLT. */
int amt_median_frame_async(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                           int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                           double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                           int lon_from_mlt, double* median, void* out_img, uint8_t* out_mask, double* out_count);
/* Quantile binning (auromat_amd.resample.resampleQuantile): amt_median_frame's pixels, membership, workspace and output
 * layouts, and for every cell with n >= 1 pixels, every plane (channel or elevation) and every q[j]
 * np.quantile(values.astype(float64), q[j]) by NumPy's default method 'linear', bit for bit:
 *     vi = (double)(n - 1) * q;  k = floor(vi);  g = vi - k;
 *     if vi >= n - 1:  a = b = sorted[n-1], g = vi + 1 (NumPy's index -1 for the last value);  else a = sorted[k], b = sorted[k+1]
 *     d = b - a;
 *     r = g >= 0.5 ? b - d * (1 - g) : a + d * g          (every operation rounded on its own, always evaluated)
 * q: HOST array of nq values, 1 <= nq <= AMT_QUANTILES_MAX, each finite and in [0, 1]; anything else is AMT_EINVAL, returned
 * before the other arguments are looked at or the device is touched.  quantile: (nq, ny, nx, nchan+1) float64, NaN where a cell
 * is empty (and in the elevation plane when elev is NULL); out_img (optional): (nq, ny, nx, nchan), r rounded half to even;
 * out_mask, out_count (optional): (ny, nx) as for the median.  The count, scan and fill passes run once per call whatever nq is.
 * q = 0.5 is np.quantile's b - d * 0.5, not np.median's (a + b) / 2: equal on the integer planes, not always on the elevation. */
#define AMT_QUANTILES_MAX 8
int amt_quantile_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                       int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                       double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, const double* q,
                       int nq, double* quantile, void* out_img, uint8_t* out_mask, double* out_count);
/* amt_quantile_frame that only enqueues work, as amt_median_frame_async does for the median (no read-back, no host wait, the
 * same workspace for the same frame and grid, lon_from_mlt); the large tier takes its launches once per quantile. */
int amt_quantile_frame_async(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                             int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                             double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                             int lon_from_mlt, const double* q, int nq, double* quantile, void* out_img, uint8_t* out_mask,
                             double* out_count);
/* The rank rule of the quantile kernels on the host (no device needed): k, k2 (k or k + 1) and g above for a cell of n >= 1
 * pixels.  The kernels call the same function.  AMT_EINVAL for n < 1, q outside [0, 1] or NaN, NULL outputs. */
int amt_quantile_rank(int64_t n, double q, int64_t* k, int64_t* k2, double* g);
/* Mosaics (ABI v9; auromat_amd.resample.resampleMosaic): the members of a collection binned onto ONE grid.  A pixel of member i
 * counts in cell c when amt_bin_frame on the common axes would bin it into c (same bin_index, masks, NaN and right-edge rules)
 * AND c lies in the member's window [win_x0, win_x0 + win_nx) x [win_y0, win_y0 + win_ny) (cells of the common grid, x along
 * xaxis, y along the ascending yaxis; an empty window bins nothing).  Cell value by `rule`:
 *   0 (union): the mean over every member's pixels in the cell (the integer sums added, then amt_bin_frame_finalize's
 *     arithmetic); out_source: the lowest member index present;
 *   1 (highest elevation wins, the reference's rule for overlapping mappings): of the members with pixels in the cell, the one
 *     whose float64 mean elevation (computed as amt_bin_frame_finalize computes it) is largest, the lower index on a tie; the
 *     cell takes that member's mean, image, count and mask bit for bit.  Every member needs `elev`.
 * Outputs in the layout of amt_bin_frame_finalize (rows north to south): mean (ny, nx, nchan+1), out_img, out_mask, out_count
 * (each optional) and out_source (optional): int32 (ny, nx), the member index, -1 where the cell is empty.
 * A fixed number of launches whatever n_members is; the member table is uploaded from the host array and the accumulators
 * ((nchan + 2) x 8 bytes per window cell of every member) live in the context's workspace.  The call only enqueues work: no
 * read-back and no host wait; inputs and outputs as for amt_median_frame_async.
 * Alignment: any, as for amt_bin_frame; the vector path is taken when EVERY member with a window has an even width, 16-byte
 * aligned lat_c / lon_c / elev and a 4-byte aligned img, the scalar path for the whole launch otherwise. */
typedef struct amt_mosaic_member {
    const double* lat_c;
    const double* lon_c;
    const double* elev;               /* may be NULL only for rule 0 */
    const void* img;                  /* may be NULL when nchan == 0 */
    const uint8_t* center_mask;       /* optional */
    int32_t height, width;
    int32_t win_x0, win_y0, win_nx, win_ny;   /* window in cells of the common grid */
} amt_mosaic_member;
int amt_mosaic_frames(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype, int32_t nchan,
                      double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, int32_t rule,
                      double* mean, void* out_img, uint8_t* out_mask, double* out_count, int32_t* out_source);
/* Median and quantile mosaics (additions to ABI v10; auromat_amd.resample.resampleMosaic(statistic='median' | 'quantile')):
 * amt_mosaic_frames' member table, cells, windows and rules with amt_median_frame's / amt_quantile_frame's statistic in place of
 * the mean.  A pixel of member i belongs to cell c when amt_median_frame on the common axes would put it into c and c lies in
 * the member's window.
 *   rule 0: every plane (image channels, elevation) is the statistic over the union of all members' pixels in the cell;
 *     out_count: the union's count; out_source (may be NULL): the lowest member index present;
 *   rule 1: the member amt_mosaic_frames elects (highest mean elevation as amt_bin_frame_finalize computes it, the lower index
 *     on a tie) takes the cell whole: every plane is the statistic over that member's pixels alone; out_count, out_mask and
 *     out_source are bit for bit those of amt_mosaic_frames on the same arguments.  Every member needs `elev`.
 * The elevation plane is NaN unless every member has `elev`.  Outputs as for amt_median_frame / amt_quantile_frame (median
 * (ny, nx, nchan+1), or quantile (nq, ny, nx, nchan+1) and out_img (nq, ny, nx, nchan)) plus out_source int32 (ny, nx), -1 where
 * empty.  Results are order statistics: two runs, and the members in any order, give the same bits (except out_source, and
 * exact ties of rule 1).  The members' pixels together must stay below 2^31 (AMT_EINVAL otherwise).  One count and one fill
 * launch whatever n_members is; synchronises once, as amt_median_frame does.  The quantile form checks q / nq before anything
 * else, as amt_quantile_frame does.  Workspace: amt_median_frame's for the members' pixels together, 4 bytes per cell, and for
 * rule 1 amt_mosaic_frames' accumulators. */
int amt_mosaic_median_frames(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype,
                             int32_t nchan, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                             int32_t rule, double* median, void* out_img, uint8_t* out_mask, double* out_count,
                             int32_t* out_source);
int amt_mosaic_quantile_frames(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype,
                               int32_t nchan, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                               int32_t rule, const double* q, int nq, double* quantile, void* out_img, uint8_t* out_mask,
                               double* out_count, int32_t* out_source);
/* Area-weighted mosaics (addition to ABI v10; auromat_amd.resample.resampleMosaic(statistic='area')): amt_mosaic_frames' member
 * table, windows and overlap rules with amt_area_frame's weights in place of the centre binning.  Both hold for any pair of axes
 * (the geodetic grid and the (MLat, SM longitude) grid alike).
 * Per member: integer accumulators sum(W), sum(W * v_k), sum(W * E) on the member's window [win_x0, win_x0 + win_nx) x [win_y0,
 * win_y0 + win_ny) of the common grid; W, E, the admission rules, lon_wrap and the candidate cells are amt_area_frame's on the
 * common axes (lat / lon: the member's CORNER arrays, (height+1) x (width+1); lat_c: the NaN test of the centres).  For every
 * cell of the window the accumulators equal amt_area_frame's on the whole common grid; cells outside it receive nothing; an
 * empty window bins nothing.
 *   rule 0 (union): the accumulators of all members are added per cell and amt_area_frame_finalize's arithmetic is applied to
 *     the totals: a cell is valid when total sum(W) >= max(1, min_weight); out_coverage: total sum(W) / 2^32, every cell;
 *     out_source: the lowest member index with sum(W) > 0 in the cell where it is valid, -1 where it is masked;
 *   rule 1 (highest elevation wins): candidates are the members whose OWN sum(W) in the cell reaches max(1, min_weight) (a sliver
 *     of a well-placed member does not take a cell that another covers whole); of them the member with the largest float64
 *     (double)(int64)sum(W * E) / (double)sum(W) wins, the lower index on a tie, and the cell takes its values, image, mask and
 *     coverage, bit for bit those of amt_area_frame_finalize on that member's accumulators.  Without a candidate the cell is
 *     masked (NaN, image 0, source -1) and its coverage is the largest single member's sum(W) / 2^32 (0 without any).  Every
 *     member needs `elev`.
 * In both rules out_source >= 0 exactly where out_mask == 0.  Outputs in the layout of amt_area_frame_finalize, each optional:
 * area (ny, nx, nchan+1), out_img (ny, nx, nchan), out_mask, out_coverage (ny, nx), out_source int32 (ny, nx).
 * AMT_EDOMAIN (outputs unspecified) when a member's own sum(W) in a window cell exceeds 2^40, or under rule 0 a cell's total
 * does; below that no 64-bit sum can wrap.  A fixed number of launches whatever n_members is (upload, one memset, one binning
 * launch — none when every window is empty: an all-masked grid, source -1, coverage 0 —, one election launch, the flag's
 * read-back); the accumulators ((nchan + 2) x 8 bytes per window cell of every member) live in the context's workspace.
 * Synchronises, as amt_area_frame_finalize does.  Alignment: any. */
typedef struct amt_area_mosaic_member {
    const double* lat;                /* corners, (height + 1) x (width + 1) */
    const double* lon;
    const double* lat_c;              /* centres, height x width */
    const double* elev;               /* may be NULL only for rule 0 */
    const void* img;                  /* may be NULL when nchan == 0 */
    const uint8_t* center_mask;       /* optional */
    int32_t height, width;
    int32_t win_x0, win_y0, win_nx, win_ny;   /* window in cells of the common grid */
} amt_area_mosaic_member;
int amt_area_mosaic_frames(amt_ctx* ctx, const amt_area_mosaic_member* members, int32_t n_members, int32_t img_dtype,
                           int32_t nchan, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                           int32_t rule, uint64_t min_weight, double* area, void* out_img, uint8_t* out_mask,
                           double* out_coverage, int32_t* out_source);
/* Scan-line maps (additions to ABI v10; auromat_amd.resample.resampleScanLines, reference draw.py:589-879 drawScanLinesCo): a
 * narrow strip of every resampled frame of a sequence, all strips on one raster.
 *
 * amt_scanline_select: which cells of ONE plate carree frame of ny x nx cells lie in a polygon.  lat_axis [ny + 1] / lon_axis
 * [nx + 1]: the latitudes of the corner rows and the longitudes of the corner columns (corner (i, j) of the frame is (lat_axis[i],
 * lon_axis[j]); the 2-D corner arrays are never read); polygon [n_vertices][2] (lat, lon), closed implicitly; cell_mask [ny][nx],
 * non-zero = masked.  The window [row0, row0 + rows) x [col0, col0 + cols) must lie in the grid (AMT_EINVAL otherwise); cells
 * outside it are not kept by definition and have no keep byte.  out_keep [rows][cols]: 1 iff the cell is unmasked and all four
 * of its corners are inside the polygon, the rule of BaseMapping.maskedByPolygon; a corner is inside exactly when
 * amt_points_in_polygon says so for px = its latitude, py = its longitude (the same arithmetic, bit for bit; a corner that is not
 * finite is outside).  out_stats int64[5]: the number of cells kept and the smallest / largest kept row and the smallest / largest
 * kept column, as rows and columns OF THE FRAME (not of the window); with nothing kept 0, INT64_MAX, INT64_MIN, INT64_MAX,
 * INT64_MIN.  n_vertices < 3 keeps nothing; an empty window writes only out_stats.  Only enqueues work.  AMT_EINVAL (nothing
 * written): NULL pointers, ny or nx <= 0, a window outside the grid. */
int amt_scanline_select(amt_ctx* ctx, const double* lat_axis, const double* lon_axis, int32_t ny, int32_t nx,
                        const double* polygon, int32_t n_vertices, const uint8_t* cell_mask, int32_t row0, int32_t col0,
                        int32_t rows, int32_t cols, uint8_t* out_keep, int64_t* out_stats);
/* amt_scanline_pack: one record per keep byte set in the window, structure of arrays: out_row / out_col int32 [count] (the
 * cell's row / column in the frame plus row_offset / col_offset), out_planes [nplane][count] from planes [ny][nx][nplane]
 * (float64; nplane 0..5: the image channels' means and, last, the elevation when present), out_img [nchan][count] from img
 * [ny][nx][nchan] (nchan 0..4; img_dtype 1 = uint8, 2 = uint16).  `count` is amt_scanline_select's out_stats[0].  The records of
 * one call are unique; their order is unspecified.  Synchronises: AMT_EINVAL when `count` is not the number of keep bytes set
 * (no record beyond `count` is written). */
int amt_scanline_pack(amt_ctx* ctx, const uint8_t* keep, int32_t row0, int32_t col0, int32_t rows, int32_t cols,
                      const double* planes, int32_t nplane, const void* img, int32_t img_dtype, int32_t nchan, int32_t ny,
                      int32_t nx, int32_t row_offset, int32_t col_offset, int64_t count, int32_t* out_row, int32_t* out_col,
                      double* out_planes, void* out_img);
/* amt_scanline_compose: the strips (record arrays of amt_scanline_pack) on one raster of NY x NX cells whose cell (0, 0) is
 * (row_base, col_base) of the records' global indices.  `strips` is a HOST array; its frame indices are >= 0 and ascend
 * strictly (AMT_EINVAL otherwise).  Every output is written whole: planes [NY][NX][nplane] (NaN where empty), img
 * [NY][NX][nchan] (0), mask [NY][NX] (1 where empty), frame_index int32 [NY][NX] (-1).  A cell that several strips hold goes to
 * the one with the LARGEST frame index, whole (the reference draws later frames over earlier ones): an integer maximum per cell
 * first, then every record writes where its strip won, so the result does not depend on the order of anything.  Within one
 * strip the records must be unique.  Synchronises: AMT_EDOMAIN when a record lies outside the raster (none is dropped
 * silently; the outputs then hold the records inside it). */
typedef struct amt_scanline_strip {
    const int32_t* row;               /* [count] */
    const int32_t* col;               /* [count] */
    const double* planes;             /* [nplane][count] */
    const void* img;                  /* [nchan][count] */
    int64_t count;                    /* may be 0 (the pointers are then not read) */
    int32_t frame;                    /* the frame's index in the sequence */
    int32_t reserved;
} amt_scanline_strip;
int amt_scanline_compose(amt_ctx* ctx, const amt_scanline_strip* strips, int32_t n_strips, int32_t img_dtype, int32_t nchan,
                         int32_t nplane, int32_t row_base, int32_t col_base, int32_t NY, int32_t NX, double* planes, void* img,
                         uint8_t* mask, int32_t* frame_index);
/* Same for float accumulators of amt_hist2d_accumulate: mean[k] = sums[k]/count, NaN where empty,
 * transposed + flipped to (ny, nx, nweights). */
int amt_hist2d_finalize_mean(amt_ctx* ctx, const double* count, const double* const* sums, int32_t nweights,
                             int32_t nx, int32_t ny, double* mean);

/* ---- resample(method='nearest') and the outside-outline masking -------------------- */

/* auromat/resample.py:301-327: scipy.interpolate.griddata((lat_c, lon_c)[valid], values, (latSpaceCenter[:,None],
 * lonSpaceCenter[None,:]), method='nearest'), i.e. for every grid centre the valid pixel centre at the smallest
 * Euclidean distance in the (lat, lon) plane in degrees.  Valid pixels as in amt_bin_frame (finite coordinates,
 * center_mask == 0, elev >= min_elevation unless that is -inf); lon_wrap != 0 searches with wrap_at(lon + 180, 180).
 * xaxis / yaxis: the uniform histogram axes of the output grid (amt_grid.xaxis / .yaxis: one bin per grid centre);
 * target_lat (ny, north -> south) / target_lon (nx): the grid centres themselves (device arrays);
 * target_mask: (ny, nx) uint8, 1 = do not search (e.g. outside the outline), may be NULL.
 * out_index: (ny, nx) int64, the flat index of the nearest pixel, -1 where masked or when there is no valid pixel.
 * Of several pixels at exactly the same distance the one with the lowest index wins (the k-d tree of the reference
 * returns an unspecified one).  Uses the context's workspace (about 8 bytes per pixel + 12 per grid cell). */
int amt_nearest_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev,
                      const uint8_t* center_mask, int32_t height, int32_t width, double min_elevation,
                      const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, const double* target_lat,
                      const double* target_lon, const uint8_t* target_mask, int64_t* out_index);
/* Values of the pixels chosen by amt_nearest_frame, laid out like the outputs of amt_bin_frame_finalize:
 * mean (optional): (n_targets, nchan+1) float64 image channels + elevation, NaN where index < 0;
 * out_img (optional): (n_targets, nchan) of img_dtype (0 where index < 0); out_mask (optional): 1 where index < 0. */
int amt_nearest_gather(amt_ctx* ctx, const int64_t* index, int64_t n_targets, const void* img, int32_t img_dtype,
                       int32_t nchan, const double* elev, double* mean, void* out_img, uint8_t* out_mask);
/* method='linear' and 'cubic' (reference resample.py:323-326: scipy.interpolate.griddata on a Delaunay triangulation of the valid
 * pixel centres) run on the exact triangulation below (amt_delaunay_*).  The lattice approximations of rounds 3-4
 * (amt_linear_gather, amt_cubic_gradients, amt_cubic_gather: the Gauss-reduced local lattice of the pixel grid in place of
 * Qhull's triangulation) were retired with ABI v6. */
/* ---- method='cubic' on the exact triangulation (round 5) ----
 * scipy.interpolate.griddata(method='cubic'), the reference's call (resample.py:323-326), is CloughTocher2DInterpolator on
 * scipy.spatial.Delaunay(points): Qhull's Delaunay triangulation, gradients from a Gauss-Seidel relaxation over its edges in
 * the order of the points, the Clough-Tocher element per triangle.
 *   amt_delaunay_create   HOST: the Delaunay triangulation of n >= 3 points xy (n, 2) (host memory; unique unless four points
 *                         are cocircular to the last bit: then Qhull's diagonal is not reproduced).  AMT_EINVAL when all
 *                         points are collinear.  Points that coincide with an earlier one are left out (amt_delaunay_sizes).
 *   amt_delaunay_create_threads   the same with the number of threads (<= 0: AMT_DELAUNAY_THREADS, else up to 16) and the number of
 *                         points from which on the build is parallel (<= 0: AMT_DELAUNAY_PARALLEL_MIN, else 200 000): vertical
 *                         strips triangulated side by side and joined at their seams (common tangents, the gap filled, Lawson
 *                         flips) — the same triangulation, the triangles in another order.
 *   amt_delaunay_build_info   info2[2]: strips built side by side (1: the sequential build), edge flips spent on joining them
 *   amt_delaunay_stats    stats4[4]: orientation tests that left double precision, of those exact zeros (three points collinear),
 *                         in-circle tests that left double precision, of those still undecided at 113 bits (four points
 *                         cocircular).  [1] = [3] = 0: no tie was met — the triangulation is the unique Delaunay triangulation of
 *                         the points, hence Qhull's.
 *   amt_delaunay_triangles        simplices (nt, 3) counter-clockwise and neighbours (nt, 3): the triangle opposite vertex k
 *                                 or -1 (scipy.spatial.Delaunay.simplices / .neighbors, in another order of triangles)
 *   amt_delaunay_vertex_neighbours   CSR (indptr (n + 1) int64, indices int32): Delaunay.vertex_neighbor_vertices, every vertex's
 *                                 list in increasing order (made on first request: this call or amt_delaunay_sizes' n_neighbours)
 *   amt_delaunay_slots    (ABI v6) the build's own triangle slots without a copy: *vertices (n_slots, 3) int32, counter-clockwise,
 *                         -1 = the vertex at infinity of a ghost triangle (one per hull edge), and *dead (n_slots) uint8, 1 = a
 *                         slot that holds no triangle; host pointers into the handle, valid until amt_delaunay_destroy.  A caller
 *                         that wants the vertex lists ON THE DEVICE uploads these two arrays and builds the lists there (every
 *                         finite triangle gives the directed edges v1 -> v2, v2 -> v0, v0 -> v1; an edge without its reverse is a
 *                         hull edge and gets it; sorted by (source, target) they are the CSR above) instead of waiting for the
 *                         host to make and copy them: auromat_amd.resample.cubic_exact
 *   amt_delaunay_locate   for m targets (m, 2): the vertices (m, 3) of the triangle that holds each (-1: outside the hull), the
 *                         centroids (m, 3, 2) of the triangles across its three edges and has_neighbour (m, 3)
 *   amt_cubic_gradients_csr   DEVICE: interpnd._estimate_gradients_2d_global in scipy's order — every channel relaxed until the
 *                         largest relative change of a sweep is below `tolerance` (scipy: 1e-6) or max_iterations (400)
 *                         sweeps; iterations[nchan] (host) receives the sweeps per channel (nchan <= 63).  xy (n, 2), values (n, nchan),
 *                         gradients (n, nchan, 2) on the device; the points must be in row-major pixel order and
 *                         row_start (n_rows + 1, device) give the first point of every pixel row (a wave walks a row).
 *   amt_cubic_eval        DEVICE: the element at the m targets -> out (m, nchan); NaN outside the hull. */
typedef struct amt_delaunay amt_delaunay;
int amt_delaunay_create(const double* xy, int64_t n, amt_delaunay** out);
int amt_delaunay_create_threads(const double* xy, int64_t n, int32_t threads, int64_t parallel_min, amt_delaunay** out);
int amt_delaunay_build_info(const amt_delaunay* d, int64_t* info2);
int amt_delaunay_destroy(amt_delaunay* d);
int amt_delaunay_sizes(const amt_delaunay* d, int64_t* n_triangles, int64_t* n_neighbours, int64_t* n_duplicates);
int amt_delaunay_stats(const amt_delaunay* d, int64_t* stats4);
int amt_delaunay_triangles(const amt_delaunay* d, int32_t* simplices, int32_t* neighbours);
int amt_delaunay_slots(const amt_delaunay* d, const int32_t** vertices, const uint8_t** dead, int64_t* n_slots);
int amt_delaunay_vertex_neighbours(const amt_delaunay* d, int64_t* indptr, int32_t* indices);
int amt_delaunay_locate(const amt_delaunay* d, const double* targets, int64_t m, int32_t* vertices, double* centroids,
                        uint8_t* has_neighbour);
int amt_cubic_gradients_csr(amt_ctx* ctx, const double* xy, int64_t n, const int64_t* indptr, const int32_t* indices,
                            const int64_t* row_start, int32_t n_rows, const double* values, int32_t nchan, double tolerance,
                            int32_t max_iterations, double* gradients, int32_t* iterations);
int amt_cubic_eval(amt_ctx* ctx, int64_t m, const double* targets, const int32_t* vertices, const double* centroids,
                   const uint8_t* has_neighbour, const double* xy, const double* values, const double* gradients, int32_t nchan,
                   double* out);
/* auromat/utils.py:58-74 pointsInsidePolygon = matplotlib.path.Path(polygon).contains_points(points): crossing test
 * with Agg's half-open edge rule; polygon: (n_vertices, 2) device doubles (x, y), closed implicitly. */
int amt_points_in_polygon(amt_ctx* ctx, const double* px, const double* py, int64_t n, const double* polygon,
                          int32_t n_vertices, uint8_t* out_inside);

/* ---- grid layout and the single-pass frame driver ------------------------------------------ */

/* Output grid of resample(method='mean') for a bounding box: auromat/resample.py:281-299 fixedGrid (global
 * alignment to +-90/+-180 with 1/pxPerDeg spacing), :220-241 (centres; first and last dropped) and
 * :330-334 + util/histogram.py:186,215-224 (histogram ranges, edges, right-edge rounding).  Pure host
 * arithmetic, bit-identical to the NumPy expressions (np.linspace, round, argmax); no GPU needed. */
typedef struct amt_grid {
    int32_t nx, ny;                      /* output cells along longitude / latitude */
    int32_t n_lat_nodes, n_lon_nodes;    /* fixedGrid's nLat, nLon */
    double lat_lo, lat_hi, lon_lo, lon_hi;   /* global grid nodes enclosing the box */
    double lat_step, lon_step;           /* centre spacing; lat_step < 0 (rows run north -> south) */
    double lat_center_first, lat_center_last, lon_center_first, lon_center_last;
    amt_axis xaxis, yaxis;               /* uniform histogram axes (edges == NULL); y edges ascend */
} amt_grid;
/* Returns AMT_OK, or AMT_EINVAL when the box yields no output cell (the reference asserts nLat, nLon > 1). */
int amt_grid_layout(double lat_px_per_deg, double lon_px_per_deg, double lat_min, double lat_max,
                    double lon_min, double lon_max, amt_grid* out);

/* Single-pass driver: georeference + mask by elevation + bounding box + grid + binned mean of one frame with
 * the binning fused into the georeferencing kernel (see amt_georef_out.bin_*), for geodetic grids (frames that straddle
 * the 180 deg discontinuity are binned with shifted longitudes, frames with a pole in view in coordinates rotated by
 * 90 deg about x: reference resample.py:176-218) and for MLat/MLT grids (resampleMLatMLT) likewise.  Separate calls per
 * stage so that frames can be software pipelined by one host thread:
 *   amt_pipe_coarse   enqueue the coarse bounding-box pre-pass (own high-priority stream), any time earlier
 *   amt_pipe_launch   wait for it, lay out the superset grid, zero the accumulators, launch the fused kernel
 *                     on the context's stream, start the copy of the exact bounding box
 *   amt_pipe_wait     wait for the exact box (the only host synchronisation), lay out the exact grid
 *   amt_pipe_finalize crop + finalise into arrays the caller sized from the grid amt_pipe_wait returned
 * status in amt_pipe_result: 0 = ready to finalise; 1 = this frame needs the general path (exact box outside the
 * superset, an extreme of a pole frame's box within 1e-6 cells of a grid node, a geodetic pole frame whose caller also
 * wants MLat / MLT arrays, an exact grid that rounds the right-most edge (amt_axis.scale) differently from its superset
 * and ends below the last cells of the superset, where the kernel records on-edge pixels under both roundings) — the coordinate
 * arrays and bbox are valid, nothing else;
 * 2 = no pixel above the elevation threshold (mapping.py:858-859 -> ValueError). */
typedef struct amt_pipe amt_pipe;
#define AMT_PIPE_MAX_EDGE_PIXELS 16384
typedef struct amt_pipe_result {
    int32_t status;
    int32_t fused;          /* 1 when the fused kernel was launched for this frame */
    int32_t lon_wrapped;    /* 1: the frame straddles the 180 deg discontinuity; `grid` is laid out for longitudes
                             * shifted by 180 deg (wrap_at_180(lon + 180)) and the caller shifts the output
                             * coordinates back (reference resample.py:203-218,274-277) */
    int32_t edge_pixels;    /* pixels on a bin edge (right-most-edge rule) that were resolved separately; a fused frame
                             * with more than AMT_PIPE_MAX_EDGE_PIXELS of them (the driver's records) gets status 1, and
                             * launching it again with its exact box as the estimate cannot help */
    double bbox[8];         /* exact reduction of amt_georef_frame; [7] = 1 when a pole (of the grid's coordinates) is in
                             * view: [0..5] are then in the rotated coordinates the grid is laid out in (amt_georef_out.
                             * bin_pole), and the caller rotates the output coordinates back (resample.py:262-273) */
    amt_grid grid;          /* exact output grid (valid for status 0) */
} amt_pipe_result;
int amt_pipe_create(amt_ctx* ctx, amt_pipe** out_pipe);
int amt_pipe_destroy(amt_pipe* pipe);
int amt_pipe_coarse(amt_pipe* pipe, const amt_frame_params* p, double min_elevation, int magnetic);
/* Instead of the pre-pass: the caller supplies the estimate (bbox[0..6] as amt_georef_coarse_bbox reports them),
 * e.g. the exact box amt_pipe_wait returned for a neighbouring frame of the same sequence.  Consecutive frames
 * move by a fraction of the superset margin, and a frame whose exact box does not fit its superset grid takes
 * the general path anyway (status 1), so a poor estimate costs time, never correctness. */
int amt_pipe_coarse_hint(amt_pipe* pipe, const double* bbox, int magnetic);
/* out: arrays to write (lat .. mlt_c as in amt_georef_frame; bbox / bin_* fields are managed by the driver) and
 * out->altitude, the mapping altitude [km] (read when a pole is in view).
 * img: (height, width, 3) uint8 (img_dtype 1) or uint16 (2).  min_elevation: -inf disables the mask.
 * pole_in_view: 0 / 1 = the caller's decision, < 0 = decide from the camera model (is a pole of the mapping
 * shell imaged by a valid pixel; replaces geodesic.py:183 / mapping.py:705-721 for camera mappings).
 * magnetic != 0 (same value as given to amt_pipe_coarse): grid, bounding box and pole refer to (MLat, SM
 * longitude), i.e. resampleMLatMLT (resample.py:63-71, mapping.py:1519-1547); p->m_sm must be set. */
int amt_pipe_launch(amt_pipe* pipe, const amt_frame_params* p, const amt_georef_out* out, const void* img,
                    int32_t img_dtype, double min_elevation, double lat_px_per_deg, double lon_px_per_deg,
                    int pole_in_view, int magnetic);
/* The single-pass plan for caller-supplied corner directions — north_star's "(H+1) x (W+1) corner arrays" form of the
 * pipeline, reference astrometry.py:49-64,86-106 with any camera model (BaseAstrometryMapping over pixelDirection's
 * array; here DirectionArrayMapping): amt_pipe_coarse_dirs samples the direction array for the estimate (or
 * amt_pipe_coarse_hint), amt_pipe_launch_dirs runs amt_georef_frame_dirs with the binning fused in; amt_pipe_wait /
 * amt_pipe_finalize as above.  p: width, height, cam, a, b, a0, b0, m_geo, m_sm and fast_center = 1 are read (the TAN
 * block is not).  There is no camera model to project a pole through: pole_in_view 0 / 1 is the caller's decision (1: the
 * frame is not fused, amt_pipe_wait returns status 1), < 0 = unknown — then a frame whose estimated or exact box comes
 * within 5 deg of a pole of its grid's coordinates is handed back with status 1 and the caller decides from the corner
 * arrays (amt_bbox_corners counts the quads that wind around a pole).
 * Ordering: corner_dirs is the one device input a pre-pass has.  amt_pipe_coarse_dirs (and the pre-pass amt_pipe_launch_dirs
 * starts when none is pending) records an event on the context's stream and lets the pre-pass stream wait for it, so the
 * array may come from work that is still queued on the context's stream (an upload, a kernel of the caller's camera model).
 * amt_pipe_launch_dirs waits on the host for the estimate, hence for that work.  amt_pipe_coarse has no device input and
 * puts no such packet on either stream. */
int amt_pipe_coarse_dirs(amt_pipe* pipe, const amt_frame_params* p, const double* corner_dirs, double min_elevation,
                         int magnetic);
int amt_pipe_launch_dirs(amt_pipe* pipe, const amt_frame_params* p, const double* corner_dirs, const amt_georef_out* out,
                         const void* img, int32_t img_dtype, double min_elevation, double lat_px_per_deg,
                         double lon_px_per_deg, int pole_in_view, int magnetic);
/* amt_pipe_launch_dirs for n <= AMT_PIPE_MAX_BATCH frames, one per driver, each with its own direction array, in ONE launch of
 * the big kernel (ABI v6; see amt_pipe_launch_many below). */
int amt_pipe_launch_dirs_many(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p, const double* const* corner_dirs,
                              const amt_georef_out* const* out, const void* const* img, int32_t img_dtype, double min_elevation,
                              double lat_px_per_deg, double lon_px_per_deg, int pole_in_view, int magnetic);
/* The same for n <= AMT_PIPE_MAX_BATCH frames, one per driver (all on one context), with ONE launch of the big
 * kernel when the frames are equally sized and take the same kernel variant (their constants sit side by side in
 * the kernel-argument segment; otherwise one launch each): the 14-17 us between two big kernels on a stream are
 * then paid once per n frames.  amt_pipe_wait / amt_pipe_finalize stay per driver. */
#define AMT_PIPE_MAX_BATCH 3
int amt_pipe_launch_many(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p,
                         const amt_georef_out* const* out, const void* const* img, int32_t img_dtype,
                         double min_elevation, double lat_px_per_deg, double lon_px_per_deg, int pole_in_view,
                         int magnetic);
/* The same with a resolution per frame (lat_px_per_deg[n], lon_px_per_deg[n]): what `resample(arcsecPerPx=...)` needs,
 * where px/deg follows from each frame's own bounding box (amt_plate_carree_resolution). */
int amt_pipe_launch_many_res(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p,
                             const amt_georef_out* const* out, const void* const* img, int32_t img_dtype,
                             double min_elevation, const double* lat_px_per_deg, const double* lon_px_per_deg,
                             int pole_in_view, int magnetic);
/* Box-first plan — `resample(mapping, arcsecPerPx=R)`, the reference's own call form (auromat/cli/convert.py:176-185,
 * test/mapping_test.py:24-42): plateCarreeResolution (resample.py:36-61) needs the frame's EXACT bounding box before a grid
 * can be laid out.  amt_pipe_launch_box enqueues the frame kernel with no output array, no image and no binning — ray,
 * shell, coordinates, elevation mask, box reduction only — on the context's stream; the following amt_pipe_wait returns
 * status 1 (or 2: no valid pixel) with bbox[0..6] = the exact reduction in (lat, lon), or with magnetic != 0 in (MLat,
 * SM longitude), never rotated, and bbox[7] = pole in view (camera model).  The caller derives px/deg
 * (amt_plate_carree_resolution on the BoundingBox of that reduction), hands the box back as the estimate
 * (amt_pipe_coarse_hint with bbox[7] = 0; a pole frame runs amt_pipe_coarse instead: its grid lives in rotated coordinates)
 * and launches the ordinary single-pass plan, whose superset grid then always contains the exact one. */
int amt_pipe_launch_box(amt_pipe* pipe, const amt_frame_params* p, double min_elevation, int magnetic);
int amt_pipe_launch_box_many(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p, double min_elevation,
                             int magnetic);
/* auromat/resample.py:36-61 plateCarreeResolution(BoundingBox(latSouth, lonWest, latNorth, lonEast), arcsecPerPx) ->
 * (latPxPerDeg, lonPxPerDeg); geodesic.angularDistance (geographiclib's a12 in the reference) restated from Karney's
 * integral formulation for two points on one parallel.  Host arithmetic, no GPU.  A box wider than 180 deg is measured the
 * shorter way round, as the reference does (min(lons, 360 - lons)); for a box that goes all the way around (a pole in view)
 * that gives *lon_px_per_deg = 0, which no grid can be laid out for: the outputs are filled as the reference's function
 * returns them — (3600 / arcsec_per_px, 0) — and the status is AMT_EDOMAIN (ABI v6; AMT_OK before), so that a host that checks
 * the status cannot lay out a grid without columns (the reference fails downstream on `assert nLon > 1`,
 * resample.py:226-227).  AMT_EINVAL when the resolution is not positive or the box has no width. */
int amt_plate_carree_resolution(double lat_south, double lon_west, double lat_north, double lon_east, double arcsec_per_px,
                                double* lat_px_per_deg, double* lon_px_per_deg);
int amt_pipe_wait(amt_pipe* pipe, amt_pipe_result* result);
/* mean (ny,nx,4) f64, out_img (ny,nx,3) of img_dtype, out_mask (ny,nx) u8, out_count (ny,nx) f64: device
 * buffers for result->grid of the preceding amt_pipe_wait (any may be NULL).  The kernel runs on the driver's
 * own stream so that it does not sit between two frames' big kernels on the context's stream. */
int amt_pipe_finalize(amt_pipe* pipe, double* mean, void* out_img, uint8_t* out_mask, double* out_count);
/* The same for the n <= AMT_PIPE_MAX_BATCH frames of one launch (arrays of n pointers each; all four kinds of output
 * are required here): ONE kernel finalises all of them and folds the on-edge pixels in, instead of two launches per
 * frame — the host side of the frame loop is what bounds short sequences and the grids-only mode. */
int amt_pipe_finalize_many(amt_pipe* const* pipes, int32_t n, double* const* mean, void* const* out_img,
                           uint8_t* const* out_mask, double* const* out_count);
/* The stream (hipStream_t) amt_pipe_finalize enqueues on.  A host whose allocator is stream ordered (PyTorch's caching
 * allocator, hipMallocAsync pools) must allocate the four output buffers FOR THIS STREAM: memory handed out for another
 * stream may still be in use by work queued there (the driver's finalise kernel does not wait for the context's
 * stream, that is its point), and the kernel would write into it too early. */
int amt_pipe_finalize_stream(amt_pipe* pipe, void** stream);
/* Orders the context's stream behind the last amt_pipe_finalize (no-op when it already completed): call it
 * before work on the context's stream — or, after amt_ctx_synchronize, the host — reads the outputs. */
int amt_pipe_join(amt_pipe* pipe);
/* The two-pass plan on the driver's streams, for frames amt_pipe_wait hands back with status 1 and for sequences that ask for
 * it (reference resample.py:159-279 as two steps: the coordinate arrays, then `_resampleCenterData`):
 *   amt_pipe_set_plan(pipe, 1)     the big kernel never bins (it writes the coordinate arrays of amt_georef_out and the box);
 *   amt_pipe_general_layout        after amt_pipe_wait: lays out the exact grid from the frame's box — result->grid,
 *                                  lon_wrapped, status 0 — unless the frame needs what only the caller has (a pole in view,
 *                                  exact centres, an MLat / MLT grid, no coordinate arrays): then status stays 1;
 *   amt_pipe_general_finalize      zeroes the accumulators, bins the frame's arrays (amt_bin_frame) and finalises into the
 *                                  caller's arrays (sized from result->grid), on the context's stream.
 * amt_pipe_set_plan(pipe, 2) (ABI v8) is plan 1 whose box is reported in the grid's coordinates: (MLat, SM longitude) for a
 * magnetic launch, as amt_pipe_launch_box does (the median sequences of the runner). */
int amt_pipe_set_plan(amt_pipe* pipe, int two_pass);
int amt_pipe_general_layout(amt_pipe* pipe, amt_pipe_result* result);
int amt_pipe_general_finalize(amt_pipe* pipe, double* mean, void* out_img, uint8_t* out_mask, double* out_count);

/* ---- native sequence runner ---------------------------------------------------------------------------------------
 * The per-frame loop of a sequence (reference mapping/spacecraft.py:326-332 `map(getMapping, ...)` followed by
 * cli/convert.py:178-185 `resample`) as ONE call: for every frame the host scalars (ephemeris seconds, the cxform
 * matrices J2000 -> GEO / SM with the IGRF dipole, the WCS Euler matrix: reference transform.py:491-696, wcs.py:133-139),
 * the estimate of its bounding box (the boxes of the frames finished before it, where the sequence is coherent; else the
 * coarse pre-pass), the launch (up to AMT_PIPE_MAX_BATCH frames per launch of the big kernel), the wait for its exact box,
 * the grid layout and the finalise kernel — software pipelined over `n_slots` frame slots by this one host thread.
 * Results: frame k's mean (ny, nx, 4) and count (ny, nx) lie one after the other at grids + grid_offset — consecutive
 * frames back to back, which is the payload of the gather's wire format (amt_seq_pack) without a copy —, its rounded
 * image (ny, nx, 3) and mask (ny, nx) at images + image_offset (256-byte aligned).
 * status per frame: 0 done (two_pass = 1: by the two-pass plan, which frames the single-pass plan hands back take when their
 * slot has coordinate arrays); 1 the frame needs the caller's general path (a pole in view that the pole plan does not cover,
 * ...; nothing of it is in the arenas); 2 no pixel above the elevation threshold;
 * 3 the arenas are full (this and the later frames were not processed); 4 (arcsec_per_px only) a pole of the grid's
 * coordinates is in view, for which plateCarreeResolution has no longitude resolution (reference resample.py:47-61: the box
 * goes all around; the reference fails on such a frame).
 * A frame the single-pass plan hands back although its launch was fused (its exact box does not fit the superset grid of a
 * poor estimate, the date line judged differently) is launched once more with its exact box as the estimate before it
 * takes any other path.
 * arcsec_per_px > 0 — `resample(mapping, arcsecPerPx=R)`, what the reference's auromat-convert runs (cli/convert.py:176-185) —:
 * every frame's px/deg follows from its own bounding box (amt_plate_carree_resolution; lat / lon_px_per_deg of the config are
 * ignored, the frame's pair is in its result): the box-first plan (amt_pipe_launch_box), the box pass of a batch two batches
 * ahead of its single-pass launch; needs n_slots >= 3 * batch.
 * Median sequences (statistic = 1, ABI v8; auromat_amd.resample.resampleMedian / resampleMedianMLatMLT): the big kernel
 * writes the slot's centre and elevation arrays and bins nothing (the slots need lat_c / lon_c / elev, or mlat_c / mlt_c /
 * elev for magnetic grids, in contiguous rows: row_layout 0); after the wait for the frame's exact box the runner lays out
 * the same grid as for the mean and enqueues amt_median_frame_async on the context's stream, so the median passes of all
 * frames run in stream order and share the context's workspace.  The arenas hold the same blocks: (ny, nx, 4) medians
 * (elevation last, NaN where empty), count, the image rounded half to even and the mask.  status 1 for what the pass does
 * not cover: a pole of the grid in view, exact centres (fast_center = 0); the caller finishes those.  two_pass is ignored;
 * arcsec_per_px works as for the mean (box pass, then the launch that writes the arrays).
 * Area-weighted sequences (statistic = 2, addition to ABI v10; auromat_amd.resample.resampleArea / resampleAreaMLatMLT): as
 * the median sequences, with amt_area_frame_async in the place of the median pass.  The slots need the CORNER arrays too: lat,
 * lon, lat_c, elev, or mlat, mlt, mlat_c, elev for magnetic grids (the MLT hours go to the pass as they are: lon_from_mlt), in
 * contiguous rows; the pass visits the rows amt_georef_image_rows names for the frame — every pixel it admits lies inside
 * them, and of a host image only they are on the device.  The arenas hold (ny, nx, 4) weighted means (elevation last, NaN
 * where masked), the coverage in the count's place, the rounded image and the mask.  A cell is valid from the weight of
 * amt_run_set_min_coverage on.  The runner keeps one device word per result record of a call, zeroed by amt_run_begin in stream
 * order, as the `over` of that frame's pass: amt_run_area_overflow reads them. */
typedef struct amt_run amt_run;
typedef struct amt_run_config {
    int32_t width, height;
    int32_t img_dtype;            /* 1 = uint8, 2 = uint16; (height, width, 3) */
    int32_t fast_center;          /* BaseAstrometryMapping.fastCenterCalculation */
    int32_t magnetic;             /* grids in (MLat, SM longitude): resampleMLatMLT */
    int32_t batch;                /* frames per launch, 1 .. AMT_PIPE_MAX_BATCH */
    int32_t use_hints;            /* 0: coarse pre-pass for every frame */
    int32_t n_slots;              /* frame slots, >= 2 * batch */
    int32_t two_pass;             /* 1: the two-pass plan for every frame (needs the slots' lat_c / lon_c / elev arrays) */
    int32_t statistic;            /* ABI v8: 0 mean, 1 median, 2 area-weighted mean (see "median sequences", "area-weighted
                                   * sequences" above) */
    double altitude;              /* mapping shell [km] of frames that name none */
    double min_elevation;         /* maskedByElevation; -inf disables */
    double lat_px_per_deg, lon_px_per_deg;
    const amt_georef_out* slots;  /* n_slots blocks: the per-pixel arrays each slot's frames write (NULL = not written);
                                   * bbox / bin_* fields are managed by the runner */
    double arcsec_per_px;         /* > 0: a resolution per frame from its own bounding box (see above); 0: the fixed pair */
} amt_run_config;
typedef struct amt_run_frame {
    double crval[2], crpix[2], cd[4], lonpole;   /* the TAN WCS cards (LATPOLE = 0) */
    double cam[3];                /* cameraPosGCRS [km] */
    double jd;                    /* photo time, UTC Julian date as ONE double (astropy Time(...).jd, transform.py:529) */
    double altitude;              /* mapping shell [km]; <= 0: the config's */
    const void* img;              /* device, (height, width, 3) of img_dtype; read until the call returns */
    /* ABI v6: with img == NULL, the image in PAGE-LOCKED host memory (hipHostMalloc / hipHostRegister / torch pin_memory; same
     * layout; read until amt_run_end returns).  The runner sends the rows that can be binned (amt_georef_image_rows) to a device
     * buffer of its own per slot on a copy stream of its own at once — the frame's launch comes one batch later and waits for
     * them —; amt_run_result.uploaded_bytes says how many bytes that were.  What the reference's loop does with the image it
     * has just read from disk (cli/convert.py:178-216, mapping/spacecraft.py:326-332). */
    const void* img_host;
} amt_run_frame;
typedef struct amt_run_result {
    int32_t status, slot;
    int32_t ny, nx;
    int32_t contains_pole;        /* grid laid out in coordinates rotated by +90 deg about x (resample.py:176-201) */
    int32_t lon_wrapped;          /* grid laid out in longitudes shifted by 180 deg (resample.py:203-218) */
    int32_t hinted;               /* 1: no coarse pre-pass ran for this frame */
    int32_t edge_pixels;
    int32_t two_pass;             /* 1: binned by the separate pass (amt_pipe_general_*), 0: by the fused kernel */
    int32_t reserved_;
    int64_t grid_offset;          /* doubles */
    int64_t image_offset;         /* bytes */
    double bbox[8];               /* amt_pipe_result.bbox */
    double altitude;
    amt_grid grid;
    amt_frame_params params;      /* what the frame was computed with */
    double lat_px_per_deg, lon_px_per_deg;   /* the resolution the frame was binned at */
    int32_t retried, reserved2_;  /* retried = 1: launched a second time with its exact box as the estimate */
    int64_t uploaded_bytes;       /* amt_run_frame.img_host: bytes of the image that crossed the link (0 for a device image) */
} amt_run_result;
/* The host scalars of one frame (no GPU call).  AMT_EINVAL: date outside the IGRF table with want_sm. */
int amt_frame_params_from_wcs(const amt_run_frame* frame, int32_t width, int32_t height, int32_t fast_center,
                              double altitude, int32_t want_sm, amt_frame_params* out);
/* The host rules of the frame drivers and the runner on those scalars (ABI v10; no context, no GPU call) — what the library
 * itself decides with, so that a host with a frame loop of its own decides the same:
 * amt_pole_in_view: +1 / -1 when the north / south pole of the mapping shell (magnetic != 0: of the SM frame; p->m_sm must be
 * set) is imaged by a valid pixel of the camera model — inside the frame, the first hit of its ray, at or above min_elevation
 * (-inf: no threshold) —, else 0; the decision of amt_pipe_launch(pole_in_view < 0) and of amt_pipe_launch_box.
 * amt_frames_close: 1 when two frames are neighbours in a sequence (same size, camera within 100 km, pointing and Earth
 * rotation within half a degree, plate scale within 1 %, shell within 30 km), else 0.
 * amt_box_hint: the runner's estimate of the box reduction of frame k (parameters p) from the latest frame the single-pass
 * plan finished — its exact reduction (amt_pipe_result.bbox), parameters and running index — and the one finished before it
 * (prev_box = NULL: none): last_box itself when that frame and p are close; the two boxes extrapolated linearly to k when the
 * sequence is steady (the camera keeps the pace of prev -> last, at most 16 frames ahead) and neither a pole nor the date line
 * came into view between the two.  Returns 1 and fills est8 (for amt_pipe_coarse_hint), or 0: run amt_pipe_coarse. */
int amt_pole_in_view(const amt_frame_params* p, double min_elevation, int magnetic);
int amt_frames_close(const amt_frame_params* a, const amt_frame_params* b);
int amt_box_hint(const double* last_box, const amt_frame_params* last_p, int64_t last_index, const double* prev_box,
                 const amt_frame_params* prev_p, int64_t prev_index, int64_t k, const amt_frame_params* p, double* est8);
int amt_run_create(amt_ctx* ctx, const amt_run_config* config, amt_run** out_run);
int amt_run_destroy(amt_run* run);
/* Processes frames[0 .. n) on the context's stream (+ the drivers' own streams); on return the context's stream is
 * ordered behind everything the call enqueued.  grids: device, grids_capacity doubles; images: device, images_capacity
 * bytes; both must stay untouched by other streams during the call.  results: n records (host).  frames_done (optional):
 * how many leading frames were processed (< n only with status 3).  The box hints carry over from call to call. */
int amt_run_process(amt_run* run, const amt_run_frame* frames, int32_t n, double* grids, int64_t grids_capacity,
                    void* images, int64_t images_capacity, amt_run_result* results, int32_t* frames_done);
/* The same call in pieces, for a host that produces its frames one by one (reading headers, decoding images): begin
 * with the arenas and room for max_frames results, push the frames in order — a push prepares its frame and, when a batch
 * is complete, finishes the older batch in flight and launches the new one, so the GPU starts after the first push —,
 * end to finish what is in flight and order the context's stream behind it.  `frame` is copied. */
int amt_run_begin(amt_run* run, double* grids, int64_t grids_capacity, void* images, int64_t images_capacity,
                  amt_run_result* results, int32_t max_frames);
int amt_run_push(amt_run* run, const amt_run_frame* frame);
int amt_run_end(amt_run* run, int32_t* frames_done);
/* Sky rows: a frame's rows of work items that cannot see the shell (amt_georef_sky_rows) are NaN in every array of its slot.
 * A slot takes a new frame every n_slots frames; the rows of the new frame's sky that the frame before left as NaN are not
 * written again.  The runner knows what a slot holds only between amt_run_begin and amt_run_end of one call, while it is the
 * only writer of the slots' arrays; every call begins knowing nothing, so the arrays are the caller's between calls.
 * amt_run_fill_stats: sky rows of work items (per frame launched; a frame launched twice counts twice) that the launches since
 * the last amt_run_begin wrote / left alone.  Either pointer may be NULL. */
int amt_run_fill_stats(amt_run* run, int64_t* bands_filled, int64_t* bands_skipped);
/* Work items that cast rays, per role (amt_georef_last_roles), of the launches since the last amt_run_begin (a frame launched
 * twice counts twice; addition to ABI 10).  Each pointer may be NULL. */
int amt_run_role_stats(amt_run* run, int64_t* generic, int64_t* inner, int64_t* low);
/* Likewise the inner items that took the core loop (amt_georef_last_core) */
int amt_run_core_stats(amt_run* run, int64_t* core);
/* Forget the box hints (the next frame gets a coarse pre-pass). */
int amt_run_reset_hints(amt_run* run);
/* Quantile sequences: the median pass of a runner created with statistic = 1 becomes a one-quantile pass — the frames it covers
 * go through amt_quantile_frame_async with nq = 1 on the same arena blocks, (ny, nx, 4) quantiles in place of the medians.
 * Before the first push of the runner; AMT_EINVAL for another statistic, a call in progress, q outside [0, 1] or NaN.  A runner
 * on which it was never called is a median runner, as before. */
int amt_run_set_quantile(amt_run* run, double q);
/* Area-weighted sequences: the least total weight of a valid cell, rint(minimum coverage * 2^32) as for amt_area_frame_finalize
 * (default 2^31: half a cell).  Before the first push of the runner; AMT_EINVAL for another statistic or a call in progress. */
int amt_run_set_min_coverage(amt_run* run, uint64_t min_weight);
/* Area-weighted sequences, after amt_run_end: waits for the context's stream and copies the overflow words of the first n result
 * records of the last call to the host (flags[k] != 0: a cell of frame k was covered more than 256 times over, its grid is
 * unspecified).  The only wait an area-weighted sequence adds.  AMT_EINVAL for another statistic, a call in progress or n beyond
 * the records of the last call. */
int amt_run_area_overflow(amt_run* run, int32_t* flags, int32_t n);

/* ---- sequences over several GPUs: packing of per-frame grids for the gather ------------------------------------
 * Whole frames are independent (reference mapping/spacecraft.py:326-332 iterates them with a plain `map`,
 * cli/convert.py:178-185), so a sequence shards by frame, one process per GPU, and only the per-frame output grids
 * travel: each rank packs its grids into ONE device buffer, the ranks exchange (frames, payload length) and the
 * root gathers the buffers padded to the longest (ncclAllGather of 2 int64 + ncclGather / grouped send-recv over
 * xGMI; python: auromat_amd/sequence.py on torch.distributed).  These three entry points give a non-Python host
 * the same wire format:
 *   buffer = [ max_frames x AMT_SEQ_DESC_LEN doubles | payload ],  payload per frame = mean (ny, nx, nc) then
 *   count (ny, nx), float64;  descriptor = ny, nx, nc, lat of the first row's centres, lon of the first column's
 *   centres, dlat, dlon, frame index, contains_pole, contains_discontinuity, altitude [km], magnetic.
 * A frame that straddles the 180 deg discontinuity has its grid laid out in longitudes shifted by 180 deg, a pole
 * frame in coordinates rotated by +90 deg about x at `altitude` (reference resample.py:176-218,262-277); the two
 * flags tell the receiver.  ny = 0 marks a frame without any valid pixel (the reference raises ValueError there,
 * mapping.py:858-859). */
#define AMT_SEQ_DESC_LEN 12
typedef struct amt_seq_frame {
    int32_t ny, nx, nc;            /* grid rows, columns, planes of `mean` (image channels + elevation) */
    int32_t index;                 /* position of the frame in the whole sequence */
    double lat0, lon0, dlat, dlon;
    int32_t contains_pole, contains_discontinuity, magnetic, reserved;
    double altitude;
    const double* mean;            /* pack: device pointers; unpack: pointers INTO the host buffer */
    const double* count;
} amt_seq_frame;
/* Payload length in doubles of n frames (host arithmetic only). */
int amt_seq_payload_size(const amt_seq_frame* frames, int32_t n, int64_t* n_doubles);
/* Writes the descriptors of the n frames and copies their grids (device to device, on the context's stream) into
 * `buffer` (device, capacity_doubles >= max_frames * AMT_SEQ_DESC_LEN + payload size; max_frames >= n is the
 * largest frame count of any rank, so that all ranks' payloads start at the same offset).  The unused tail of
 * the descriptor table is zeroed. */
int amt_seq_pack(amt_ctx* ctx, const amt_seq_frame* frames, int32_t n, int32_t max_frames, double* buffer,
                 int64_t capacity_doubles);
/* Splits one rank's gathered buffer, already in HOST memory, into frames: n_frames descriptors are read,
 * frames with ny = 0 are skipped; returns the number of entries written to `out` (at most capacity) in *n_out. */
int amt_seq_unpack(const double* host_buffer, int64_t n_doubles, int32_t n_frames, int32_t max_frames,
                   amt_seq_frame* out, int32_t capacity, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* AUROMAT_HIP_H */
