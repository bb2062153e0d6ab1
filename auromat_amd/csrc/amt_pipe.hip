// Single-pass frame driver (see include/auromat_hip.h, "grid layout and the single-pass frame driver").
// Host orchestration only: every kernel it launches lives in amt_georef.hip / amt_binning.hip.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <new>

#include "amt_common.h"
#include "amt_grid.h"
#include "amt_params.h"

struct amt_pipe {
    amt_ctx* ctx;
    // The context's stream carries only the big kernel of each frame.  Everything small runs beside it:
    hipStream_t pre_stream;        // coarse pre-pass of a later frame (must not queue behind the running kernel)
    hipStream_t tail_stream;       // bounding-box folds of this frame, waiting for its big kernel
    hipStream_t fin_stream;        // crop/finalise kernel: waits for nothing on the GPU (the host has seen the box),
                                   // so it must not queue behind another frame's folds, which do wait
                                   // (all three owned by the context and shared with its other drivers)
    hipEvent_t coarse_done, kernel_done, bbox_done, tail_done;
    hipEvent_t dirs_ready;         // the context's stream where a caller's direction array is handed to the pre-pass
    double* host_small;            // pinned host memory: [0..7] coarse bbox, [8..15] exact bbox
    double* host_small_dev;        // the same 16 doubles as the kernels address them (the folds write them directly)
    void* events;                  // on-edge pixels of the frame in flight (bin_event records, device)
    uint32_t* event_count;         // device counter; zero between frames
    long long n_events;            // what the frame reported (host copy)
    uint64_t* acc;                 // superset accumulators (device), 5 planes
    size_t acc_cells;              // capacity per plane
    bool acc_zero;                 // the accumulators are known to be all zero
    double* partials;              // per-wave partial boxes of the big kernel (read by the folds on tail_stream)
    size_t partials_bytes;
    // state of the frame in flight
    bool coarse_pending, launched, fused, ready, tail_pending;
    bool coarse_hinted;            // the pending coarse box came from the caller (amt_pipe_coarse_hint), no kernel ran
    int coarse_magnetic;           // coordinates of the pending coarse box (0 geodetic, 1 MLat / SM longitude,
                                   // 2 / 3 the same rotated by 90 deg about x: the pole plans)
    int lon_wrap;                  // the frame straddles the 180 deg discontinuity: longitudes are binned shifted by 180
    amt_grid super, exact;
    int32_t off_x, off_y;          // window of the exact grid inside the superset
    int band_x = kNoBand, band_y = kNoBand;     // see amt_georef_tail
    uint32_t xmask = 1, ymask = 2;              // the flag bits of the exact grid's rounding (bin_event)
    double lat_ppd, lon_ppd, min_elev;
    int pole;
    bool pole_unknown;             // direction arrays without a decision of the caller: see amt_pipe_launch_dirs
    bool pole_plan;                // this frame is binned in the coordinates rotated by 90 deg about x (bin_pole)
    int img_dtype;
    // the two-pass plan on the driver's streams (amt_pipe_general_layout / _finalize): the frame's coordinate arrays, image
    // and size as the big kernel was given them
    bool two_pass;                 // amt_pipe_set_plan: never fuse the binning into the big kernel
    bool box_in_grid;              // amt_pipe_set_plan(2): the box of a magnetic launch in (MLat, SM longitude)
    bool general_ready;            // amt_pipe_general_layout has laid out the exact grid of the frame in flight
    const double* g_lat_c;
    int g_row_layout;              // amt_georef_out.row_layout of the frame in flight (strip-padded arrays: no general path here)
    const double* g_lon_c;
    const double* g_elev;
    const void* g_img;
    int g_width, g_height, g_fast, g_mode;      // g_mode: 0 geodetic grid without a pole in view (see pipe_prepare's mode)
};

namespace {

constexpr int kCoarseStride = 16;      // every 16th pixel corner at most; >= 128 lattice points on the short side
constexpr double kMarginDeg = 1.0;     // safety margin around the coarse box (> 3 lattice steps on the ground)
constexpr double kPoleGuardDeg = 85.0; // direction arrays, pole unknown: boxes that reach beyond this latitude are not fused

int ensure_acc(amt_pipe* pipe, size_t cells) {
    if (cells <= pipe->acc_cells) return AMT_OK;
    amt_ctx* ctx = pipe->ctx;
    if (pipe->acc) {
        AMT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        AMT_HIP(ctx, hipStreamSynchronize(pipe->tail_stream));
        AMT_HIP(ctx, hipFree(pipe->acc));
        pipe->acc = nullptr;
        pipe->acc_cells = 0;
    }
    const size_t cap = cells < (1u << 16) ? (1u << 16) : cells + cells / 4;
    AMT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&pipe->acc), cap * 5 * sizeof(uint64_t)));
    pipe->acc_cells = cap;
    pipe->acc_zero = false;
    return AMT_OK;
}

int ensure_partials(amt_pipe* pipe, size_t bytes) {
    if (bytes <= pipe->partials_bytes) return AMT_OK;
    amt_ctx* ctx = pipe->ctx;
    if (pipe->partials) {
        AMT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        AMT_HIP(ctx, hipStreamSynchronize(pipe->tail_stream));
        AMT_HIP(ctx, hipFree(pipe->partials));
        pipe->partials = nullptr;
        pipe->partials_bytes = 0;
    }
    AMT_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&pipe->partials), bytes));
    pipe->partials_bytes = bytes;
    return AMT_OK;
}

}  // namespace

extern "C" {

int amt_grid_layout(double lat_px_per_deg, double lon_px_per_deg, double lat_min, double lat_max, double lon_min,
                    double lon_max, amt_grid* out) {
    if (out == nullptr) return AMT_EINVAL;
    std::memset(out, 0, sizeof(*out));
    return amt_gl::layout(lat_px_per_deg, lon_px_per_deg, lat_min, lat_max, lon_min, lon_max, out) ? AMT_OK
                                                                                                       : AMT_EINVAL;
}

int amt_plate_carree_resolution(double lat_south, double lon_west, double lat_north, double lon_east, double arcsec_per_px,
                                double* lat_px_per_deg, double* lon_px_per_deg) {
    if (lat_px_per_deg == nullptr || lon_px_per_deg == nullptr) return AMT_EINVAL;
    if (!amt_gl::plate_carree_resolution(lat_south, lon_west, lat_north, lon_east, arcsec_per_px, lat_px_per_deg, lon_px_per_deg))
        return AMT_EINVAL;
    return *lon_px_per_deg > 0 ? AMT_OK : AMT_EDOMAIN;
}

int amt_pole_in_view(const amt_frame_params* p, double min_elevation, int magnetic) {
    return p == nullptr ? 0 : amt_prm::pole_in_view(p, min_elevation, magnetic ? 1 : 0);
}

int amt_pipe_create(amt_ctx* ctx, amt_pipe** out_pipe) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, out_pipe != nullptr, "out_pipe is NULL");
    *out_pipe = nullptr;
    if (amt_set_device(ctx)) return AMT_EHIP;
    amt_pipe* pipe = new (std::nothrow) amt_pipe();
    if (pipe == nullptr) return AMT_ENOMEM;
    std::memset(pipe, 0, sizeof(*pipe));
    pipe->ctx = ctx;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (ctx->aux_pre == nullptr) (void)hipStreamCreateWithPriority(&ctx->aux_pre, hipStreamNonBlocking, hi);
    if (ctx->aux_tail == nullptr) (void)hipStreamCreateWithPriority(&ctx->aux_tail, hipStreamNonBlocking, hi);
    if (ctx->aux_fin == nullptr) (void)hipStreamCreateWithPriority(&ctx->aux_fin, hipStreamNonBlocking, hi);
    pipe->pre_stream = ctx->aux_pre;
    pipe->tail_stream = ctx->aux_tail;
    pipe->fin_stream = ctx->aux_fin;
    bool ok = pipe->pre_stream != nullptr && pipe->tail_stream != nullptr && pipe->fin_stream != nullptr &&
              hipEventCreateWithFlags(&pipe->coarse_done, hipEventDisableTiming) == hipSuccess &&
              hipEventCreate(&pipe->kernel_done) == hipSuccess &&
              hipEventCreateWithFlags(&pipe->bbox_done, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&pipe->tail_done, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&pipe->dirs_ready, hipEventDisableTiming) == hipSuccess &&
              hipMalloc(&pipe->events, AMT_PIPE_MAX_EDGE_PIXELS * 32) == hipSuccess &&
              // (zeroed on the context's stream before the first fused launch, see pipe_prepare: a memset on the null stream
              // here is not ordered against the context's non-blocking stream and may run late when processes share the GPU)
              hipMalloc(reinterpret_cast<void**>(&pipe->event_count), sizeof(uint32_t)) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&pipe->host_small), 16 * sizeof(double), hipHostMallocMapped) ==
                  hipSuccess &&
              hipHostGetDevicePointer(reinterpret_cast<void**>(&pipe->host_small_dev), pipe->host_small, 0) == hipSuccess;
    if (!ok) {
        ctx->last_error = "amt_pipe_create: resource allocation failed";
        amt_pipe_destroy(pipe);
        return AMT_EHIP;
    }
    *out_pipe = pipe;
    return AMT_OK;
}

int amt_pipe_destroy(amt_pipe* pipe) {
    if (pipe == nullptr) return AMT_EINVAL;
    if (pipe->pre_stream) (void)hipStreamSynchronize(pipe->pre_stream);
    if (pipe->tail_stream) (void)hipStreamSynchronize(pipe->tail_stream);
    if (pipe->fin_stream) (void)hipStreamSynchronize(pipe->fin_stream);
    if (pipe->coarse_done) (void)hipEventDestroy(pipe->coarse_done);
    if (pipe->kernel_done) (void)hipEventDestroy(pipe->kernel_done);
    if (pipe->bbox_done) (void)hipEventDestroy(pipe->bbox_done);
    if (pipe->tail_done) (void)hipEventDestroy(pipe->tail_done);
    if (pipe->dirs_ready) (void)hipEventDestroy(pipe->dirs_ready);
    if (pipe->partials) (void)hipFree(pipe->partials);
    if (pipe->events) (void)hipFree(pipe->events);
    if (pipe->event_count) (void)hipFree(pipe->event_count);
    if (pipe->host_small) (void)hipHostFree(pipe->host_small);
    if (pipe->acc) (void)hipFree(pipe->acc);
    delete pipe;
    return AMT_OK;
}

}  // extern "C"

namespace {

// coarse box in the coordinates of `mode` (see amt_pipe.coarse_magnetic)
int pipe_coarse(amt_pipe* pipe, const amt_frame_params* p, double min_elevation, int mode, const double* dirs = nullptr) {
    amt_ctx* ctx = pipe->ctx;
    // the pre-pass runs on the driver's own stream (and with that stream's workspace, see amt_workspace): the
    // context's stream is busy with the previous frames' kernels
    hipStream_t saved = ctx->stream;
    if (dirs != nullptr) {
        // the caller made the direction array on the context's stream (an upload, a kernel of its own camera model): the
        // pre-pass reads it on another stream and starts behind what the context's stream holds now.  The camera model has no
        // device input: no packet there.
        AMT_HIP(ctx, hipEventRecord(pipe->dirs_ready, saved));
        AMT_HIP(ctx, hipStreamWaitEvent(pipe->pre_stream, pipe->dirs_ready, 0));
    }
    ctx->stream = pipe->pre_stream;
    const double thr = std::isinf(min_elevation) ? min_elevation : min_elevation - 0.5;
    const int shorter = p->width < p->height ? p->width : p->height;
    const int stride = std::max(1, std::min(kCoarseStride, shorter / 128));
    int rc = dirs ? amt_georef_coarse_bbox_dirs(ctx, p, dirs, stride, thr, mode, pipe->host_small_dev)
                  : amt_georef_coarse_bbox(ctx, p, stride, thr, mode, pipe->host_small_dev);
    ctx->stream = saved;
    if (rc != AMT_OK) return rc;
    AMT_HIP(ctx, hipEventRecord(pipe->coarse_done, pipe->pre_stream));
    pipe->coarse_pending = true;
    pipe->coarse_hinted = false;
    pipe->coarse_magnetic = mode;
    return AMT_OK;
}

}  // namespace

extern "C" {

int amt_pipe_coarse_dirs(amt_pipe* pipe, const amt_frame_params* p, const double* corner_dirs, double min_elevation,
                         int magnetic) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    AMT_REQUIRE(ctx, p != nullptr && corner_dirs != nullptr, "NULL argument");
    return pipe_coarse(pipe, p, min_elevation, magnetic ? 1 : 0, corner_dirs);
}

int amt_pipe_coarse(amt_pipe* pipe, const amt_frame_params* p, double min_elevation, int magnetic) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    AMT_REQUIRE(ctx, p != nullptr, "NULL argument");
    // a frame with a pole of its grid in view is binned in rotated coordinates (the pole plans): its box is needed in those
    const int mode = (magnetic ? 1 : 0) + (amt_prm::pole_in_view(p, min_elevation, magnetic ? 1 : 0) != 0 ? 2 : 0);
    return pipe_coarse(pipe, p, min_elevation, mode);
}

}  // extern "C"

namespace {

// One frame of a launch: camera model, the caller's corner directions in its place (direction launches), where the kernel
// writes and what it bins (not in a box pass), and the resolution of the frame's grid
struct launch_frame {
    const amt_frame_params* p;
    const double* dirs;
    const amt_georef_out* out;
    const void* img;
    double lat_ppd, lon_ppd;
};

// What the frames of a launch share.  A box pass (amt_pipe_launch_box) is a camera launch whose frames have neither outputs nor
// image nor resolution: the kernel writes nothing but each frame's bounding box.
enum class launch_kind { camera, directions, box };
struct launch_common {
    launch_kind kind;
    int32_t img_dtype;
    double min_elevation;
    int pole_in_view, magnetic;
    amt_sky_state* sky;             // optional, one per frame (amt_common.h)
};

// the folds / finalise of the previous frame on this driver still use the partials and the accumulators
int pipe_wait_tail(amt_pipe* pipe) {
    amt_ctx* ctx = pipe->ctx;
    if (pipe->tail_pending) {
        // usually long finished (the host saw the frame's bounding box): then no packet goes on the stream.  A host
        // that is quick (the native sequence runner launches the next batch microseconds after it enqueued this driver's
        // finalise kernel) waits a moment for it instead — the big kernel of the batch before is running anyway —: every
        // wait packet between two big kernels lengthens their boundary by 3-4 us (kernel trace: 27 us per boundary
        // with three of them, 15-16 us with none)
        bool done = hipEventQuery(pipe->tail_done) == hipSuccess;
        // (two-pass plan: what the buffer waits for is its previous frame's binning pass, a kernel as long as the big one —
        // the wait goes on the stream at once)
        if (!done && !pipe->two_pass) {
            const auto t0 = std::chrono::steady_clock::now();
            while (!done && std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(150))
                done = hipEventQuery(pipe->tail_done) == hipSuccess;
        }
        if (!done) AMT_HIP(ctx, hipStreamWaitEvent(ctx->stream, pipe->tail_done, 0));
        pipe->tail_pending = false;
    }
    return AMT_OK;
}

// Everything a launch does for one frame before the big kernel: wait for the coarse box, superset grid, accumulators,
// kernel outputs (`o`) and the tail description for this frame.  Box pass: no estimate, no grid — the driver keeps nothing
// of an earlier frame's plan, the kernel gets no output but the box.
int pipe_prepare(amt_pipe* pipe, const launch_frame& f, const launch_common& L, amt_georef_out* o_out, amt_georef_tail* tail_out) {
    amt_ctx* ctx = pipe->ctx;
    const amt_frame_params* p = f.p;
    const bool box_only = L.kind == launch_kind::box;
    const double* dirs = f.dirs;
    const void* img = f.img;
    const double min_elevation = L.min_elevation, lat_px_per_deg = f.lat_ppd, lon_px_per_deg = f.lon_ppd;
    const int magnetic = L.magnetic ? 1 : 0, pole_in_view = L.pole_in_view;
    // (direction arrays: there is no camera model to project the pole through — the caller decides, or nobody does)
    pipe->pole_unknown = dirs != nullptr && pole_in_view < 0;
    pipe->pole = pole_in_view < 0 ? (dirs == nullptr && amt_prm::pole_in_view(p, min_elevation, magnetic) != 0 ? 1 : 0) : (pole_in_view ? 1 : 0);
    // frames with a pole of their grid in view take a pole plan (binned in rotated coordinates; a geodetic pole frame of
    // a caller that wants the MLat / MLT arrays as well runs the kernel variant of the magnetic pole plan with the
    // rotated pair taken from (lat, lon), see prepare_georef); direction arrays have none: their pole frames are not fused
    const int mode = dirs ? magnetic : (magnetic ? (pipe->pole ? 3 : 1) : (pipe->pole ? 2 : 0));
    pipe->pole_plan = !box_only && mode >= 2;
    // (box pass: an estimate that is still pending belongs to another plan of this frame: dropped)
    if (box_only || !pipe->coarse_pending || pipe->coarse_magnetic != mode) {
        if (pipe->coarse_pending && !pipe->coarse_hinted) AMT_HIP(ctx, hipEventSynchronize(pipe->coarse_done));
        if (!box_only)
            if (int rc = pipe_coarse(pipe, p, min_elevation, mode, dirs)) return rc;
    }
    if (!box_only && !pipe->coarse_hinted) AMT_HIP(ctx, hipEventSynchronize(pipe->coarse_done));
    pipe->coarse_pending = false;
    pipe->coarse_hinted = false;
    pipe->lat_ppd = lat_px_per_deg;
    pipe->lon_ppd = lon_px_per_deg;
    pipe->min_elev = min_elevation;
    if (!box_only) pipe->img_dtype = L.img_dtype;
    pipe->fused = false;

    if (int rc = pipe_wait_tail(pipe)) return rc;
    if (int rc = ensure_partials(pipe, amt_georef_partials_bytes(p))) return rc;

    amt_georef_out& o = *o_out;
    if (box_only) std::memset(&o, 0, sizeof(o));
    else o = *f.out;
    o.bbox = pipe->host_small_dev + 8;          // the last fold writes straight into pinned host memory
    o.bbox_min_elevation = min_elevation;
    o.bin_acc = nullptr;
    o.bin_xaxis = o.bin_yaxis = nullptr;
    o.bin_img = nullptr;
    o.bin_img_dtype = o.bin_lon_wrap = o.bin_magnetic = o.bin_pole = 0;
    if (pipe->box_in_grid || box_only) o.bin_magnetic = magnetic;       // (without bin_acc: the box in the grid's coordinates)
    o.bin_events = nullptr;
    o.bin_event_count = nullptr;
    o.bin_event_capacity = 0;
    if (!box_only) {
        // start with the side of the frame where the coarse pass found the hits (see amt_georef_out.item_order)
        const long long packed = (long long)pipe->host_small[7];
        long long sy = ((packed % (1 << 20)) + (1 << 20)) % (1 << 20);
        if (sy >= (1 << 19)) sy -= (1 << 20);
        const long long sx = (packed - sy) / (1 << 20);
        const long long ax = sx < 0 ? -sx : sx, ay = sy < 0 ? -sy : sy;
        o.item_order = (ax | ay) == 0 ? 0 : ((ay >= ax && sy > 0) ? 2 : 1);
    }

    // (a box pass: no arrays, so no general path either)
    pipe->g_lat_c = o.lat_c, pipe->g_lon_c = o.lon_c, pipe->g_elev = o.elev, pipe->g_img = img;
    pipe->g_row_layout = o.row_layout;
    pipe->g_width = p->width, pipe->g_height = p->height, pipe->g_fast = p->fast_center;
    pipe->g_mode = dirs ? -1 : mode;      // (amt_pipe_general_layout: the pole of a direction-array frame is the caller's business)
    pipe->general_ready = false;
    // coarse [lat_min, lat_max, lon_min, lon_max, lon_min_positive, lon_max_nonpositive, n, hint]
    const double* c = pipe->host_small;
    bool fuse = !box_only && !pipe->two_pass && c[6] > 0 && (!pipe->pole || pipe->pole_plan);
    if (pipe->pole_unknown && !(c[0] > -kPoleGuardDeg && c[1] < kPoleGuardDeg)) fuse = false;
    pipe->lon_wrap = 0;
    amt_gl::box_range r;
    const bool ranged = amt_gl::range_of_box(c, &r);
    const double box_lo = r.lon_lo, box_hi = r.lon_hi;
    if (fuse && pipe->pole_plan && r.wrapped) fuse = false;      // (cannot happen: the rotated frame sits at the equator)
    if (fuse && r.wrapped) {
        // the box straddles the 180 deg discontinuity: longitudes are binned shifted by 180 deg
        pipe->lon_wrap = 1;
        fuse = ranged && box_hi > box_lo;
    }
    double lon_margin_used = 0.0;
    if (fuse) {
        const double lat_abs = std::fmax(std::fabs(c[0]), std::fabs(c[1]));
        const double lon_margin = lon_margin_used = std::fmin(10.0, kMarginDeg / std::fmax(0.1, std::cos(lat_abs * amt::kDeg2Rad)));
        const double lat_lo = std::fmax(-89.0, c[0] - kMarginDeg), lat_hi = std::fmin(89.0, c[1] + kMarginDeg);
        // (a box whose MARGIN reaches past +-180 deg — a footprint that ends just short of the date line — is cut there: when
        // the exact box turns out to straddle after all, amt_pipe_wait sees that the coarse pass judged it differently)
        const double lon_lo = std::fmax(-180.0, box_lo - lon_margin), lon_hi = std::fmin(180.0, box_hi + lon_margin);
        fuse = box_lo > -179.9 && box_hi < 179.9 &&
               amt_gl::layout(lat_px_per_deg, lon_px_per_deg, lat_lo, lat_hi, lon_lo, lon_hi, &pipe->super);
    }
    if (fuse) {
        const size_t cells = (size_t)pipe->super.nx * pipe->super.ny;
        if (int rc = ensure_acc(pipe, cells)) return rc;
        if (!pipe->acc_zero) {
            // first use / after a frame that was not finalised; otherwise the finalise kernel leaves zeros behind
            AMT_HIP(ctx, hipMemsetAsync(pipe->acc, 0, pipe->acc_cells * 5 * sizeof(uint64_t), ctx->stream));
            AMT_HIP(ctx, hipMemsetAsync(pipe->event_count, 0, sizeof(uint32_t), ctx->stream));
            pipe->acc_zero = true;
        }
        o.bin_xaxis = &pipe->super.xaxis;
        o.bin_yaxis = &pipe->super.yaxis;
        o.bin_img = img;
        o.bin_img_dtype = L.img_dtype;
        o.bin_acc = pipe->acc;
        o.bin_magnetic = magnetic;
        o.bin_pole = pipe->pole_plan ? 1 : 0;
        o.bin_lon_wrap = pipe->lon_wrap;
        o.bin_events = pipe->events;
        o.bin_event_count = pipe->event_count;
        o.bin_event_capacity = AMT_PIPE_MAX_EDGE_PIXELS;
        // the exact grid ends inside the margin, so within twice the margin (and a few cells) of the superset's end: from there on
        // the kernel records what is on-edge under a neighbouring decimal too (amt_pipe_wait knows which rounding the exact grid has)
        pipe->band_x = std::max(0, pipe->super.nx - (int)std::ceil(2 * lon_margin_used * lon_px_per_deg) - 4);
        pipe->band_y = std::max(0, pipe->super.ny - (int)std::ceil(2 * kMarginDeg * lat_px_per_deg) - 4);
        pipe->fused = true;
        pipe->acc_zero = false;
    }
    tail_out->stream = pipe->tail_stream;
    tail_out->kernel_done = pipe->kernel_done;
    tail_out->partials = pipe->partials;
    tail_out->partials_bytes = pipe->partials_bytes;
    tail_out->band_x = pipe->fused ? pipe->band_x : kNoBand;
    tail_out->band_y = pipe->fused ? pipe->band_y : kNoBand;
    return AMT_OK;
}

// THE launch: frame i of `f` on driver i of `pipes`, all of them in one launch of the big kernel (amt_georef_launch_many).
// f == NULL: the caller's arrays were not all there.  The whole batch is checked before any driver's state changes.
int launch_frames(amt_pipe* const* pipes, int32_t n, const launch_frame* f, const launch_common& L) {
    if (pipes == nullptr || n < 1 || pipes[0] == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipes[0]->ctx;
    AMT_REQUIRE(ctx, n <= AMT_MAX_BATCH, "at most AMT_PIPE_MAX_BATCH frames per launch");
    AMT_REQUIRE(ctx, f != nullptr, "NULL argument");
    const bool box_only = L.kind == launch_kind::box, with_dirs = L.kind == launch_kind::directions;
    for (int i = 0; i < n; ++i) {
        AMT_REQUIRE(ctx, pipes[i] != nullptr && pipes[i]->ctx == ctx, "drivers of one launch must share the context");
        for (int k = 0; k < i; ++k) AMT_REQUIRE(ctx, pipes[k] != pipes[i], "a driver can hold one frame of a launch");
        AMT_REQUIRE(ctx, f[i].p && (box_only || (f[i].out && f[i].img)) && (!with_dirs || f[i].dirs), "NULL argument");
        AMT_REQUIRE(ctx, !with_dirs || f[i].p->fast_center, "caller-supplied directions need fast_center");
    }
    AMT_REQUIRE(ctx, box_only || L.img_dtype == 1 || L.img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    amt_georef_out o[AMT_MAX_BATCH];
    amt_georef_tail tails[AMT_MAX_BATCH];
    const amt_frame_params* pp[AMT_MAX_BATCH];
    const double* dp[AMT_MAX_BATCH];
    const amt_georef_out* op[AMT_MAX_BATCH];
    const amt_georef_tail* tp[AMT_MAX_BATCH];
    for (int i = 0; i < n; ++i) {
        if (int rc = pipe_prepare(pipes[i], f[i], L, &o[i], &tails[i])) return rc;
        pp[i] = f[i].p, dp[i] = f[i].dirs, op[i] = &o[i], tp[i] = &tails[i];
    }
    if (int rc = amt_georef_launch_many(ctx, n, pp, with_dirs ? dp : nullptr, op, tp, L.sky)) return rc;
    for (int i = 0; i < n; ++i) {
        amt_pipe* pipe = pipes[i];
        AMT_HIP(ctx, hipEventRecord(pipe->bbox_done, pipe->tail_stream));
        AMT_HIP(ctx, hipEventRecord(pipe->tail_done, pipe->tail_stream));
        pipe->tail_pending = true;
        pipe->launched = true;
    }
    return AMT_OK;
}

// The arrays of an exported launch function as frames: dirs for direction launches, out / img / lat / lon for all but box passes;
// res_stride 1: a resolution per frame, 0: one for all
int launch_arrays(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p, const double* const* dirs,
                  const amt_georef_out* const* out, const void* const* img, const double* lat, const double* lon, int res_stride,
                  const launch_common& L) {
    launch_frame f[AMT_MAX_BATCH];
    const bool box_only = L.kind == launch_kind::box, with_dirs = L.kind == launch_kind::directions;
    const bool all = p && (box_only || (out && img && lat && lon)) && (!with_dirs || dirs);
    for (int i = 0; all && n <= AMT_MAX_BATCH && i < n; ++i) {      // (n out of range: launch_frames says so, nothing is read)
        if (box_only) f[i] = {p[i], nullptr, nullptr, nullptr, 0.0, 0.0};
        else f[i] = {p[i], with_dirs ? dirs[i] : nullptr, out[i], img[i], lat[i * res_stride], lon[i * res_stride]};
    }
    return launch_frames(pipes, n, all ? f : nullptr, L);
}

}  // namespace

// amt_pipe_launch_many_res with the sky state of each frame's arrays (amt_common.h); not part of the C ABI
int amt_pipe_launch_many_sky(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p, const amt_georef_out* const* out,
                             const void* const* img, int32_t img_dtype, double min_elevation, const double* lat_px_per_deg,
                             const double* lon_px_per_deg, int pole_in_view, int magnetic, amt_sky_state* sky) {
    return launch_arrays(pipes, n, p, nullptr, out, img, lat_px_per_deg, lon_px_per_deg, 1,
                         {launch_kind::camera, img_dtype, min_elevation, pole_in_view, magnetic, sky});
}

extern "C" {

int amt_pipe_coarse_hint(amt_pipe* pipe, const double* bbox, int magnetic) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    AMT_REQUIRE(ctx, bbox != nullptr, "NULL argument");
    if (pipe->coarse_pending) {
        // a pre-pass kernel may still be writing the same 8 doubles
        AMT_HIP(ctx, hipEventSynchronize(pipe->coarse_done));
    }
    for (int i = 0; i < 7; ++i) pipe->host_small[i] = bbox[i];
    pipe->host_small[7] = 0;                       // no hit statistics: item order from the camera model
    pipe->coarse_pending = true;
    // the exact box of a pole-plan frame (bbox[7] = 1 in amt_pipe_result of a fused frame) is in rotated coordinates
    pipe->coarse_magnetic = (magnetic ? 1 : 0) + (bbox[7] != 0 ? 2 : 0);
    pipe->coarse_hinted = true;
    return AMT_OK;
}

int amt_pipe_launch_many(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p,
                         const amt_georef_out* const* out, const void* const* img, int32_t img_dtype,
                         double min_elevation, double lat_px_per_deg, double lon_px_per_deg, int pole_in_view,
                         int magnetic) {
    return launch_arrays(pipes, n, p, nullptr, out, img, &lat_px_per_deg, &lon_px_per_deg, 0,
                         {launch_kind::camera, img_dtype, min_elevation, pole_in_view, magnetic, nullptr});
}

int amt_pipe_launch_many_res(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p,
                             const amt_georef_out* const* out, const void* const* img, int32_t img_dtype,
                             double min_elevation, const double* lat_px_per_deg, const double* lon_px_per_deg,
                             int pole_in_view, int magnetic) {
    // (nothing is known about what the caller's arrays hold: every sky row is written)
    return amt_pipe_launch_many_sky(pipes, n, p, out, img, img_dtype, min_elevation, lat_px_per_deg, lon_px_per_deg, pole_in_view,
                                    magnetic, nullptr);
}

int amt_pipe_launch_dirs_many(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p, const double* const* corner_dirs,
                              const amt_georef_out* const* out, const void* const* img, int32_t img_dtype, double min_elevation,
                              double lat_px_per_deg, double lon_px_per_deg, int pole_in_view, int magnetic) {
    return launch_arrays(pipes, n, p, corner_dirs, out, img, &lat_px_per_deg, &lon_px_per_deg, 0,
                         {launch_kind::directions, img_dtype, min_elevation, pole_in_view, magnetic, nullptr});
}

int amt_pipe_launch_box_many(amt_pipe* const* pipes, int32_t n, const amt_frame_params* const* p, double min_elevation,
                             int magnetic) {
    return launch_arrays(pipes, n, p, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                         {launch_kind::box, 0, min_elevation, -1, magnetic, nullptr});
}

// one frame: the same with arrays of one (a NULL driver is the first thing launch_frames looks for)
int amt_pipe_launch(amt_pipe* pipe, const amt_frame_params* p, const amt_georef_out* out, const void* img,
                    int32_t img_dtype, double min_elevation, double lat_px_per_deg, double lon_px_per_deg,
                    int pole_in_view, int magnetic) {
    return amt_pipe_launch_many(&pipe, 1, &p, &out, &img, img_dtype, min_elevation, lat_px_per_deg, lon_px_per_deg,
                                pole_in_view, magnetic);
}

int amt_pipe_launch_dirs(amt_pipe* pipe, const amt_frame_params* p, const double* corner_dirs, const amt_georef_out* out,
                         const void* img, int32_t img_dtype, double min_elevation, double lat_px_per_deg,
                         double lon_px_per_deg, int pole_in_view, int magnetic) {
    return amt_pipe_launch_dirs_many(&pipe, 1, &p, &corner_dirs, &out, &img, img_dtype, min_elevation, lat_px_per_deg,
                                     lon_px_per_deg, pole_in_view, magnetic);
}

int amt_pipe_launch_box(amt_pipe* pipe, const amt_frame_params* p, double min_elevation, int magnetic) {
    return amt_pipe_launch_box_many(&pipe, 1, &p, min_elevation, magnetic);
}

int amt_pipe_wait(amt_pipe* pipe, amt_pipe_result* result) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    AMT_REQUIRE(ctx, result != nullptr, "result is NULL");
    AMT_REQUIRE(ctx, pipe->launched, "amt_pipe_launch has not been called for this frame");
    pipe->launched = false;
    pipe->ready = false;
    AMT_HIP(ctx, hipEventSynchronize(pipe->bbox_done));
    std::memset(result, 0, sizeof(*result));
    const double* b = pipe->host_small + 8;
    for (int i = 0; i < 8; ++i) result->bbox[i] = b[i];
    result->bbox[7] = pipe->pole ? 1.0 : 0.0;      // pole containment comes from the camera model
    result->fused = pipe->fused ? 1 : 0;
    if (b[6] == 0) {
        result->status = 2;
        return AMT_OK;
    }
    result->status = 1;
    pipe->n_events = pipe->fused ? (long long)b[7] : 0;        // the last fold put the counter into slot 7
    if (!pipe->fused || (pipe->pole && !pipe->pole_plan)) return AMT_OK;
    result->edge_pixels = (int32_t)(pipe->n_events > 2000000000ll ? 2000000000ll : pipe->n_events);
    if (pipe->n_events > AMT_PIPE_MAX_EDGE_PIXELS) return AMT_OK;         // more on-edge pixels than records: general path
    // direction arrays whose caller left the pole open: a box that comes near a pole goes back to the caller (status 1)
    if (pipe->pole_unknown && !(b[0] > -kPoleGuardDeg && b[1] < kPoleGuardDeg)) return AMT_OK;
    const bool straddles = b[3] - b[2] > 180;
    if (straddles != (pipe->lon_wrap != 0)) return AMT_OK;      // the coarse pass judged the discontinuity differently
    if (pipe->pole_plan) {
        // the kernel knows the rotated corners to ~1e-11 deg, the two-pass plan to the bit: the grids are the same
        // unless an extreme of the box sits that close to a grid node (k / px-per-deg); then the general path decides
        if (straddles) return AMT_OK;
        const double v[4] = {b[0] * pipe->lat_ppd, b[1] * pipe->lat_ppd, b[2] * pipe->lon_ppd, b[3] * pipe->lon_ppd};
        for (int i = 0; i < 4; ++i)
            if (!(std::fabs(v[i] - std::nearbyint(v[i])) > 1e-6)) return AMT_OK;
    }
    amt_grid& g = result->grid;
    if (!amt_gl::layout_of_box(pipe->lat_ppd, pipe->lon_ppd, b, &g, &result->lon_wrapped)) return AMT_OK;
    const amt_grid& s = pipe->super;
    // The kernel flagged on-edge pixels with the superset's rounding (`scale`, from the smallest edge difference of the axis
    // it was given).  An exact grid can round one decimal coarser (it has no edge difference below the step, its superset
    // has) or finer (the other way round): its last edge then owns other pixels than the kernel's first flag bit says.
    // Inside the band the kernel recorded all three readings (bin_event), and the finalise kernels take the bit of the
    // exact grid's rounding.  Any other relation of the two scales: the general path.
    auto reading = [](double exact, double super, uint32_t same, uint32_t coarser, uint32_t finer) -> uint32_t {
        return exact == super ? same : (exact * 10.0 == super ? coarser : (exact == super * 10.0 ? finer : 0u));
    };
    const uint32_t xmask = reading(g.xaxis.scale, s.xaxis.scale, 1u, 4u, 16u);
    const uint32_t ymask = reading(g.yaxis.scale, s.yaxis.scale, 2u, 8u, 32u);
    if (!xmask || !ymask) return AMT_OK;
    // window of the exact grid inside the superset (same global nodes => integer offsets)
    const long off_x = std::lround((g.lon_center_first - s.lon_center_first) / s.lon_step);
    const long off_y = std::lround((g.lat_center_last - s.lat_center_last) / std::fabs(s.lat_step));
    if (off_x < 0 || off_y < 0 || off_x + g.nx > s.nx || off_y + g.ny > s.ny) return AMT_OK;
    const double lon_at = s.lon_center_first + off_x * s.lon_step;
    const double lat_at = s.lat_center_last + off_y * std::fabs(s.lat_step);
    if (std::fabs(lon_at - g.lon_center_first) > 1e-9 || std::fabs(lat_at - g.lat_center_last) > 1e-9) return AMT_OK;
    // (an exact grid that rounds differently and ends below the band — a poor estimate —: the general path)
    if ((xmask != 1u && off_x + g.nx < pipe->band_x) || (ymask != 2u && off_y + g.ny < pipe->band_y)) return AMT_OK;
    pipe->xmask = xmask, pipe->ymask = ymask;
    pipe->exact = g;
    pipe->off_x = (int32_t)off_x;
    pipe->off_y = (int32_t)off_y;
    pipe->ready = true;
    result->status = 0;
    return AMT_OK;
}

int amt_pipe_finalize(amt_pipe* pipe, double* mean, void* out_img, uint8_t* out_mask, double* out_count) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    AMT_REQUIRE(ctx, pipe->ready, "amt_pipe_wait has not returned status 0 for this frame");
    pipe->ready = false;
    const amt_grid& s = pipe->super;
    const amt_grid& g = pipe->exact;
    // on-edge pixels first (their bin depends on where the final grid ends), then the crop: on the finalise stream
    // (this frame's big kernel and folds are complete: the host has read the box), zeroing the accumulators for
    // the next frame on the way
    if (pipe->n_events > 0) {
        if (int rc = amt_bin_apply_events_on(ctx, pipe->fin_stream, pipe->events, pipe->event_count, pipe->acc, s.nx, s.ny,
                                             pipe->off_x, pipe->off_y, g.nx, g.ny, pipe->xmask, pipe->ymask))
            return rc;
    }
    if (int rc = amt_bin_finalize_on(ctx, pipe->fin_stream, pipe->acc, s.nx, s.ny, pipe->off_x, pipe->off_y, g.nx, g.ny,
                                     3, pipe->img_dtype, mean, out_img, out_mask, out_count, 1))
        return rc;
    pipe->acc_zero = true;
    AMT_HIP(ctx, hipEventRecord(pipe->tail_done, pipe->fin_stream));
    pipe->tail_pending = true;
    return AMT_OK;
}

int amt_pipe_finalize_many(amt_pipe* const* pipes, int32_t n, double* const* mean, void* const* out_img,
                           uint8_t* const* out_mask, double* const* out_count) {
    if (pipes == nullptr || n < 1 || pipes[0] == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipes[0]->ctx;
    AMT_REQUIRE(ctx, n <= AMT_MAX_BATCH, "at most AMT_PIPE_MAX_BATCH frames per call");
    AMT_REQUIRE(ctx, mean && out_img && out_mask && out_count, "NULL argument");
    finish_batch B;
    std::memset(&B, 0, sizeof(B));
    B.n = n;
    for (int i = 0; i < n; ++i) {
        amt_pipe* pipe = pipes[i];
        AMT_REQUIRE(ctx, pipe != nullptr && pipe->ctx == ctx && pipe->fin_stream == pipes[0]->fin_stream,
                    "drivers of one call must share the context");
        for (int k = 0; k < i; ++k) AMT_REQUIRE(ctx, pipes[k] != pipe, "a driver can hold one frame of a call");
        AMT_REQUIRE(ctx, pipe->ready, "amt_pipe_wait has not returned status 0 for this frame");
        AMT_REQUIRE(ctx, pipe->img_dtype == pipes[0]->img_dtype, "frames of one call must share the image type");
        AMT_REQUIRE(ctx, pipe->n_events <= AMT_PIPE_MAX_EDGE_PIXELS, "more on-edge pixels than records");
        finish_frame& F = B.f[i];
        F.events = pipe->events;
        F.count = pipe->event_count;
        F.acc = reinterpret_cast<unsigned long long*>(pipe->acc);
        F.acc_nx = pipe->super.nx, F.acc_ny = pipe->super.ny;
        F.off_x = pipe->off_x, F.off_y = pipe->off_y;
        F.nx = pipe->exact.nx, F.ny = pipe->exact.ny;
        F.n_events = (unsigned int)pipe->n_events;
        F.masks = pipe->xmask | (pipe->ymask << 8);
        F.mean = mean[i], F.img = out_img[i], F.mask = out_mask[i], F.out_count = out_count[i];
    }
    // one launch for all of them, on the finalise stream (see amt_pipe_finalize)
    if (int rc = amt_pipe_finish_on(ctx, pipes[0]->fin_stream, B, pipes[0]->img_dtype)) return rc;
    for (int i = 0; i < n; ++i) {
        amt_pipe* pipe = pipes[i];
        pipe->ready = false;
        pipe->acc_zero = true;
        AMT_HIP(ctx, hipEventRecord(pipe->tail_done, pipe->fin_stream));
        pipe->tail_pending = true;
    }
    return AMT_OK;
}

int amt_pipe_set_plan(amt_pipe* pipe, int two_pass) {
    if (pipe == nullptr) return AMT_EINVAL;
    pipe->two_pass = two_pass != 0;
    pipe->box_in_grid = two_pass == 2;
    return AMT_OK;
}

int amt_pipe_general_layout(amt_pipe* pipe, amt_pipe_result* result) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    AMT_REQUIRE(ctx, result != nullptr, "result is NULL");
    pipe->general_ready = false;
    if (result->status != 1) return AMT_OK;
    // what the kernels of this path do not cover stays with the caller: a pole in view (binned in rotated coordinates),
    // exact centres (their masks are reconciled first), MLat / MLT grids, frames whose coordinate arrays were not written or
    // lie in strip-padded rows (amt_bin_frame reads contiguous rows: the caller compacts them first, amt_unpad_rows)
    if (pipe->pole || !pipe->g_fast || pipe->g_mode != 0 || !pipe->g_lat_c || !pipe->g_lon_c || !pipe->g_elev || pipe->g_row_layout != 0) return AMT_OK;
    const double* b = result->bbox;
    if (!(b[6] > 0)) return AMT_OK;
    amt_grid g;
    int32_t wrapped = 0;
    if (!amt_gl::layout_of_box(pipe->lat_ppd, pipe->lon_ppd, b, &g, &wrapped)) return AMT_OK;
    if (g.nx >= 65535 || g.ny >= 65535) return AMT_OK;
    result->grid = g;
    result->lon_wrapped = wrapped;
    result->status = 0;
    pipe->exact = g;
    pipe->lon_wrap = wrapped;
    pipe->general_ready = true;
    return AMT_OK;
}

int amt_pipe_general_finalize(amt_pipe* pipe, double* mean, void* out_img, uint8_t* out_mask, double* out_count) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    AMT_REQUIRE(ctx, pipe->general_ready, "amt_pipe_general_layout has not laid out this frame");
    AMT_REQUIRE(ctx, mean && out_img && out_mask && out_count, "NULL argument");
    pipe->general_ready = false;
    const amt_grid& g = pipe->exact;
    const size_t cells = (size_t)g.nx * g.ny;
    if (int rc = ensure_acc(pipe, cells)) return rc;
    // The binning pass and the finalise kernel go on the context's stream, IN LINE with the big kernels (behind this frame's,
    // which has finished: the host has its box; in a sequence behind the next frame's, which is running or queued).  Beside
    // a big kernel — on the finalise stream — the two slow each other down by more than they overlap (kernel trace of a
    // two-pass sequence: binning 82 -> 190-240 us, big kernel 118 -> 140-245 us; profiles/r3/x_two_pass_timeline.txt).
    hipStream_t fs = ctx->stream;
    AMT_HIP(ctx, hipMemsetAsync(pipe->acc, 0, cells * 5 * sizeof(uint64_t), fs));
    int rc = amt_bin_frame(ctx, pipe->g_lat_c, pipe->g_lon_c, pipe->g_elev, pipe->g_img, pipe->img_dtype, 3, nullptr, pipe->g_height,
                           pipe->g_width, pipe->min_elev, &g.xaxis, &g.yaxis, pipe->lon_wrap, pipe->acc);
    if (rc != AMT_OK) return rc;
    rc = amt_bin_finalize_on(ctx, fs, pipe->acc, g.nx, g.ny, 0, 0, g.nx, g.ny, 3, pipe->img_dtype, mean, out_img, out_mask,
                             out_count, 0);
    if (rc != AMT_OK) return rc;
    pipe->acc_zero = false;
    AMT_HIP(ctx, hipEventRecord(pipe->tail_done, fs));
    pipe->tail_pending = true;
    return AMT_OK;
}

int amt_pipe_finalize_stream(amt_pipe* pipe, void** stream) {
    if (pipe == nullptr || stream == nullptr) return AMT_EINVAL;
    *stream = reinterpret_cast<void*>(pipe->fin_stream);
    return AMT_OK;
}

int amt_pipe_join(amt_pipe* pipe) {
    if (pipe == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = pipe->ctx;
    if (pipe->tail_pending && hipEventQuery(pipe->tail_done) != hipSuccess)
        AMT_HIP(ctx, hipStreamWaitEvent(ctx->stream, pipe->tail_done, 0));
    return AMT_OK;
}

}  // extern "C"
