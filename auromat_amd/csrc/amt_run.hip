// Native sequence runner (include/auromat_hip.h, "native sequence runner"): the per-frame host loop of a sequence —
// host scalars, box hints, launches, waits, grid layouts, finalise kernels — in one C call.  Host orchestration only;
// it drives the single-pass frame drivers of amt_pipe.hip through their public entry points and, for the launches, through
// amt_pipe_launch_many_sky (amt_common.h: amt_pipe_launch_many_res with the sky state of each frame's slot).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "amt_common.h"
#include "amt_grid.h"
#include "amt_params.h"

namespace {

// One frame slot: a driver, the caller's arrays, and the frame the slot holds (frame k lies in slot k % n_slots).
struct slot {
    amt_pipe* pipe = nullptr;
    amt_georef_out out{};                   // the caller's arrays (+ the altitude of the frame in the slot)
    amt_frame_params prm{};                 // the frame in flight
    double alt = 0;
    int hinted = 0;
    const void* img = nullptr;              // the image of the frame in the slot
    // box-first plan (cfg.arcsec_per_px > 0): the resolution the frame's box gave (otherwise the config's), and what became of a
    // frame that was not launched (2 no valid pixel, 4 a pole in view, 0 launched)
    double ppd_lat = 0, ppd_lon = 0;
    int pre_status = 0;
    // host images (amt_run_frame.img_host): a device image buffer of the runner's own (allocated when the slot first takes such
    // a frame; all three or none, slot_image_create), the event behind the frame's upload on the runner's copy stream (the
    // launch that reads the buffer waits for it), and the event behind a separate binning pass that still reads the buffer (the
    // next upload waits for it)
    void* own_img = nullptr;
    hipEvent_t uploaded = nullptr, img_free = nullptr;
    bool upload_pending = false, img_busy = false;
    int64_t uploaded_bytes = 0;
    // Sky rows of work items that the slot's arrays already hold as NaN (amt_prm::sky_fill): [0, top_end) and
    // [bottom_begin, n), the sky of the frame the slot held before.  The launch of the slot's next frame does not write
    // them again.  Valid only inside one call, begin ... end, while the runner is the only writer of the slots' arrays — a caller
    // may do what it likes with them between calls —, kept per slot index and nowhere else; forgotten (forget_sky) when a call
    // begins, when a push or the end of a call fails, and when the context's stream changes under the call: the big kernels of
    // all frames, retries included, go on that one stream, and its order is what makes a slot's previous writer finished.
    amt_prm::sky_known known = amt_prm::sky_known_empty();
};

// consecutive frames k0 ... k0 + count - 1 of the call, and the (at most two) batches in one stage of the loop, older first
struct batch { int k0, count; };
struct batch_queue {
    batch q[2];
    int n = 0;
    int size() const { return n; }
    const batch& front() const { return q[0]; }
    void push(batch b) { q[n++] = b; }
    void pop() { q[0] = q[1], --n; }
};

}  // namespace

struct amt_run {
    amt_ctx* ctx = nullptr;
    amt_run_config cfg{};
    std::vector<slot> slots;
    hipEvent_t entry = nullptr;             // the context's stream at the start of a call (the finalise stream waits for it)
    // box hints: the two latest frames finished by the single-pass plan (exact reduction, params, running index)
    struct hint {
        bool valid = false;
        double box[8];
        amt_frame_params p;
        long long index;
    } last, prev;
    long long frames_done = 0;
    bool has_quantile = false;              // amt_run_set_quantile: the median pass selects `quantile` instead
    double quantile = 0.5;
    // area-weighted sequences (cfg.statistic == 2): the least weight of a valid cell (amt_run_set_min_coverage), and one device
    // word per result record of the call in progress, zeroed by amt_run_begin on the context's stream: frame k's pass ORs its
    // overflow flag into word k (amt_run_area_overflow reads them)
    uint64_t min_weight = (uint64_t)1 << 31;
    uint32_t* over = nullptr;
    int over_capacity = 0;
    // the call in progress (amt_run_begin ... amt_run_end)
    bool active = false, full = false;
    double* grids = nullptr;
    char* images = nullptr;
    int64_t grids_capacity = 0, images_capacity = 0, grid_used = 0, image_used = 0;
    amt_run_result* results = nullptr;
    int max_frames = 0, n_pushed = 0;
    batch collecting = {0, 0};              // prepared frames of the batch being collected
    batch_queue launched;                   // the batches in flight
    batch_queue boxed;                      // box-first plan: the batches whose box pass is in flight
    hipStream_t copy_stream = nullptr;      // host images: the uploads' stream, created with the first of them
    hipStream_t launch_stream = nullptr;    // the stream of the latest launch (slot::known)
    int64_t bands_filled = 0, bands_skipped = 0;    // amt_run_fill_stats: since the last amt_run_begin
    int64_t role_items[3] = {0, 0, 0};              // amt_run_role_stats: likewise (generic, inner, low)
    int64_t core_items = 0;                         // amt_run_core_stats: likewise (the inner items that took the core loop)

    slot& slot_of(int k) { return slots[k % cfg.n_slots]; }
};

namespace {

// estimate of frame k's box reduction from the frames the single-pass plan has finished (amt_prm::box_hint)
bool box_hint(const amt_run* run, long long k, const amt_frame_params& p, double* est) {
    const amt_run::hint &last = run->last, &prev = run->prev;
    return last.valid && amt_prm::box_hint(last.box, last.p, last.index, prev.valid ? prev.box : nullptr, &prev.p, prev.index, k, p, est);
}

// the next frame gets a real pre-pass
void forget_hints(amt_run* run) { run->last.valid = run->prev.valid = false; }

// frame k of the call, in slot s, was finished with the exact box reduction `box`
void remember_hint(amt_run* run, const slot& s, int k, const double* box) {
    run->prev = run->last;
    run->last.valid = true;
    std::memcpy(run->last.box, box, sizeof(run->last.box));
    run->last.p = s.prm;
    run->last.index = run->frames_done + k;
}

// nothing is known about what the slots' arrays hold: the next frame of every slot writes all of its sky rows
void forget_sky(amt_run* run) { for (slot& s : run->slots) s.known = amt_prm::sky_known_empty(); }

// A slot's device image buffer and both of its events, or none of the three: on failure whatever was created is given back
// and the slot is left as it was.
int slot_image_create(amt_ctx* ctx, slot& s, size_t bytes) {
    void* buf = nullptr;
    hipEvent_t uploaded = nullptr, img_free = nullptr;
    if (hipMalloc(&buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        ctx->last_error = "amt_run_push: no device memory for a slot's image buffer";
        return AMT_ENOMEM;
    }
    hipError_t err = hipEventCreateWithFlags(&uploaded, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&img_free, hipEventDisableTiming);
    if (err != hipSuccess) {
        if (uploaded != nullptr) (void)hipEventDestroy(uploaded);
        (void)hipFree(buf);
        ctx->last_error = std::string("amt_run_push: event creation for a slot's image buffer -> ") + hipGetErrorString(err);
        return AMT_EHIP;
    }
    s.own_img = buf, s.uploaded = uploaded, s.img_free = img_free;
    return AMT_OK;
}

void slot_image_release(slot& s) {
    if (s.own_img == nullptr) return;
    (void)hipFree(s.own_img);
    (void)hipEventDestroy(s.uploaded);
    (void)hipEventDestroy(s.img_free);
    s.own_img = nullptr, s.uploaded = s.img_free = nullptr;
}

}  // namespace

extern "C" {

int amt_frame_params_from_wcs(const amt_run_frame* frame, int32_t width, int32_t height, int32_t fast_center,
                              double altitude, int32_t want_sm, amt_frame_params* out) {
    if (frame == nullptr || out == nullptr || width <= 0 || height <= 0) return AMT_EINVAL;
    return amt_prm::frame_params(frame, width, height, fast_center, altitude, want_sm, out);
}

int amt_frames_close(const amt_frame_params* a, const amt_frame_params* b) {
    return a != nullptr && b != nullptr && amt_prm::close_frames(*a, *b) ? 1 : 0;
}

int amt_box_hint(const double* last_box, const amt_frame_params* last_p, int64_t last_index, const double* prev_box,
                 const amt_frame_params* prev_p, int64_t prev_index, int64_t k, const amt_frame_params* p, double* est8) {
    if (last_box == nullptr || last_p == nullptr || p == nullptr || est8 == nullptr) return 0;
    return amt_prm::box_hint(last_box, *last_p, last_index, prev_box, prev_p, prev_index, k, *p, est8) ? 1 : 0;
}

int amt_run_create(amt_ctx* ctx, const amt_run_config* config, amt_run** out_run) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, config != nullptr && out_run != nullptr, "NULL argument");
    *out_run = nullptr;
    AMT_REQUIRE(ctx, config->width > 0 && config->height > 0, "empty frame");
    AMT_REQUIRE(ctx, config->img_dtype == 1 || config->img_dtype == 2, "img_dtype must be 1 (uint8) or 2 (uint16)");
    AMT_REQUIRE(ctx, config->batch >= 1 && config->batch <= AMT_PIPE_MAX_BATCH, "batch out of range");
    AMT_REQUIRE(ctx, config->n_slots >= 2 * config->batch && config->slots != nullptr, "n_slots must be at least 2 * batch");
    AMT_REQUIRE(ctx, config->arcsec_per_px > 0 || (config->lat_px_per_deg > 0 && config->lon_px_per_deg > 0), "px per degree must be positive");
    AMT_REQUIRE(ctx, config->statistic >= 0 && config->statistic <= 2, "statistic must be 0 (mean), 1 (median) or 2 (area-weighted)");
    AMT_REQUIRE(ctx, !(config->arcsec_per_px > 0) || ((config->statistic != 0 || !config->two_pass) && config->n_slots >= 3 * config->batch),
                "arcsec_per_px: the box-first plan is a single-pass plan and needs n_slots >= 3 * batch");
    amt_run* run = new (std::nothrow) amt_run();
    if (run == nullptr) return AMT_ENOMEM;
    run->ctx = ctx;
    run->cfg = *config;
    run->cfg.slots = nullptr;
    run->slots.resize(config->n_slots);
    if (amt_set_device(ctx)) {
        delete run;
        return AMT_EHIP;
    }
    for (int i = 0; i < config->n_slots; ++i) {
        slot& s = run->slots[i];
        s.out = config->slots[i];
        s.ppd_lat = config->lat_px_per_deg, s.ppd_lon = config->lon_px_per_deg;
        int rc = amt_pipe_create(ctx, &s.pipe);
        // (median, area: the big kernel writes the slot's arrays and bins nothing; its box in the grid's coordinates)
        if (rc == AMT_OK) rc = amt_pipe_set_plan(s.pipe, config->statistic != 0 ? 2 : config->two_pass);
        if (rc != AMT_OK) {
            amt_run_destroy(run);
            return rc;
        }
    }
    if (hipEventCreateWithFlags(&run->entry, hipEventDisableTiming) != hipSuccess) {
        ctx->last_error = "amt_run_create: event creation failed";
        amt_run_destroy(run);
        return AMT_EHIP;
    }
    *out_run = run;
    return AMT_OK;
}

int amt_run_destroy(amt_run* run) {
    if (run == nullptr) return AMT_EINVAL;
    for (slot& s : run->slots)
        if (s.pipe != nullptr) amt_pipe_destroy(s.pipe);
    if (run->entry) (void)hipEventDestroy(run->entry);
    if (run->copy_stream) (void)hipStreamSynchronize(run->copy_stream);
    for (slot& s : run->slots) slot_image_release(s);
    if (run->copy_stream) (void)hipStreamDestroy(run->copy_stream);
    if (run->over) (void)hipFree(run->over);
    delete run;
    return AMT_OK;
}

int amt_run_set_quantile(amt_run* run, double q) {
    if (run == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = run->ctx;
    AMT_REQUIRE(ctx, run->cfg.statistic == 1, "the runner was not created with statistic = 1");
    AMT_REQUIRE(ctx, !run->active && run->frames_done == 0, "to be called before the first push");
    AMT_REQUIRE(ctx, q >= 0.0 && q <= 1.0, "the quantile must lie in [0, 1]");
    run->has_quantile = true;
    run->quantile = q;
    return AMT_OK;
}

int amt_run_set_min_coverage(amt_run* run, uint64_t min_weight) {
    if (run == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = run->ctx;
    AMT_REQUIRE(ctx, run->cfg.statistic == 2, "the runner was not created with statistic = 2");
    AMT_REQUIRE(ctx, !run->active && run->frames_done == 0, "to be called before the first push");
    run->min_weight = min_weight;
    return AMT_OK;
}

int amt_run_area_overflow(amt_run* run, int32_t* flags, int32_t n) {
    if (run == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = run->ctx;
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, run->cfg.statistic == 2, "the runner was not created with statistic = 2");
    AMT_REQUIRE(ctx, !run->active, "to be called after amt_run_end");
    AMT_REQUIRE(ctx, n >= 0 && n <= run->max_frames && (n == 0 || flags != nullptr), "n beyond the records of the last call");
    if (n == 0) return AMT_OK;
    if (amt_set_device(ctx)) return AMT_EHIP;
    static_assert(sizeof(int32_t) == sizeof(uint32_t), "one word per record");
    AMT_HIP(ctx, hipMemcpyAsync(flags, run->over, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    AMT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AMT_OK;
}

int amt_run_fill_stats(amt_run* run, int64_t* bands_filled, int64_t* bands_skipped) {
    if (run == nullptr) return AMT_EINVAL;
    if (bands_filled) *bands_filled = run->bands_filled;
    if (bands_skipped) *bands_skipped = run->bands_skipped;
    return AMT_OK;
}

int amt_run_role_stats(amt_run* run, int64_t* generic, int64_t* inner, int64_t* low) {
    if (run == nullptr) return AMT_EINVAL;
    if (generic) *generic = run->role_items[0];
    if (inner) *inner = run->role_items[1];
    if (low) *low = run->role_items[2];
    return AMT_OK;
}

int amt_run_core_stats(amt_run* run, int64_t* core) {
    if (run == nullptr || core == nullptr) return AMT_EINVAL;
    *core = run->core_items;
    return AMT_OK;
}

int amt_run_reset_hints(amt_run* run) {
    if (run == nullptr) return AMT_EINVAL;
    forget_hints(run);
    return AMT_OK;
}

}  // extern "C"

// ---- the loop as a state machine: begin / push (one frame at a time) / end ------------------------------------------
// The batches in flight form a queue of at most two: when a batch of prepared frames is complete, the older launched
// batch is finished first if two are in flight (wait for the boxes, lay out the grids, one finalise kernel), then the new
// batch is launched; and a frame whose slot still belongs to a frame in flight finishes that frame's batch first
// (amt_run_push).  The frames arrive one by one, so the first launch happens after the first frame's preparation whatever
// the length of the sequence.

namespace {

// How a frame's outputs are produced: by the fused kernel's finalise, or by a second pass over the arrays the big kernel wrote
// for the slot — general (the native two-pass plan of mean sequences), ordered (median or quantile), area.
enum class pass { fused, general, ordered, area };

// The pass that produces the frame in slot s, and for a second pass its grid in *pr (status 0).
// Median and quantile sequences: the exact grid of a frame the big kernel has written the slot's arrays for (status 1 from
// amt_pipe_wait), laid out as amt_pipe_general_layout and the single-pass plan lay it out (amt_gl::layout_of_box), in (MLat, SM
// longitude) on a magnetic grid.  What the ordered pass does not cover keeps status 1: a pole of the grid in view, exact centres,
// slots without the arrays.  Area-weighted sequences: the same rule on the arrays the area pass reads — the corners and their
// centres' latitude (the NaN test) in place of the centres.
int choose_pass(const amt_run* run, const slot& s, amt_pipe_result* pr, pass* how) {
    const amt_run_config& cfg = run->cfg;
    const amt_georef_out& o = s.out;
    const double* b = pr->bbox;
    *how = pass::fused;
    if (cfg.statistic == 0) {
        // the two-pass plan, natively, when the frame's coordinate arrays exist and nothing else is needed
        if (pr->status != 1) return AMT_OK;
        if (int rc = amt_pipe_general_layout(s.pipe, pr)) return rc;
        if (pr->status == 0) *how = pass::general;
        return AMT_OK;
    }
    const pass second = cfg.statistic == 2 ? pass::area : pass::ordered;
    const bool have = second == pass::area ? (cfg.magnetic ? (o.mlat && o.mlt && o.mlat_c) : (o.lat && o.lon && o.lat_c))
                                           : (cfg.magnetic ? (o.mlat_c && o.mlt_c) : (o.lat_c && o.lon_c));
    if (pr->status == 0) *how = second;
    if (pr->status != 1 || b[7] != 0 || !cfg.fast_center || !have || !o.elev || o.row_layout != 0 || !(b[6] > 0)) return AMT_OK;
    if (!amt_gl::layout_of_box(s.ppd_lat, s.ppd_lon, b, &pr->grid, &pr->lon_wrapped)) return AMT_OK;
    pr->status = 0;
    *how = second;
    return AMT_OK;
}

// The single-pass launch of the frames in `slots` (m of them, at most a batch), in one kernel.  Each frame's launch leaves the
// sky rows alone that its slot holds as NaN already — nothing_known: writes them all — and says which the slot holds now.
int launch_slots(amt_run* run, const int* slots, int m, bool nothing_known = false) {
    amt_ctx* ctx = run->ctx;
    const amt_run_config& cfg = run->cfg;
    amt_pipe* pp[AMT_PIPE_MAX_BATCH];
    const amt_frame_params* prm[AMT_PIPE_MAX_BATCH];
    const amt_georef_out* oo[AMT_PIPE_MAX_BATCH];
    const void* ii[AMT_PIPE_MAX_BATCH];
    double la[AMT_PIPE_MAX_BATCH], lo[AMT_PIPE_MAX_BATCH];
    amt_sky_state sky[AMT_PIPE_MAX_BATCH];
    // what the slots hold is known as long as every launch goes on one stream (slot::known)
    if (ctx->stream != run->launch_stream) forget_sky(run), run->launch_stream = ctx->stream;
    for (int j = 0; j < m; ++j) {
        slot& s = run->slots[slots[j]];
        s.out.altitude = s.alt;
        pp[j] = s.pipe, prm[j] = &s.prm, oo[j] = &s.out, ii[j] = s.img;
        la[j] = s.ppd_lat, lo[j] = s.ppd_lon;
        const amt_prm::sky_known known = nothing_known ? amt_prm::sky_known_empty() : s.known;
        sky[j] = {known.top_end, known.bottom_begin, 0, 0, {0, 0, 0}};
        if (s.img == nullptr) {
            ctx->last_error = "amt_run: a frame has no image";
            return AMT_EINVAL;
        }
        if (s.upload_pending) {
            // the frame's image rows are crossing the link on the copy stream (since its push, one batch ago)
            AMT_HIP(ctx, hipStreamWaitEvent(ctx->stream, s.uploaded, 0));
            s.upload_pending = false;
        }
    }
    if (int rc = amt_pipe_launch_many_sky(pp, m, prm, oo, ii, cfg.img_dtype, cfg.min_elevation, la, lo, -1, cfg.magnetic ? 1 : 0, sky))
        return rc;
    for (int j = 0; j < m; ++j) {
        run->slots[slots[j]].known = {sky[j].known_top_end, sky[j].known_bottom_begin};
        run->bands_filled += sky[j].bands_filled, run->bands_skipped += sky[j].bands_skipped;
        for (int k = 0; k < 3; ++k) run->role_items[k] += sky[j].role_items[k];
        run->core_items += sky[j].core_items;
    }
    return AMT_OK;
}

// A frame's outputs in the arenas: four planes of mean values and one of counts, doubles, in `grids`; the image and, behind it,
// the mask in `images`, padded to a multiple of 256 bytes.
struct frame_outputs {
    int64_t grid_doubles, image_bytes;
    double *mean, *count;
    void* image;
    uint8_t* mask;
};

// the outputs of a frame of `cells` cells at the arenas' fill marks; false: no room (or none since an earlier frame)
bool next_outputs(const amt_run* run, int64_t cells, frame_outputs* f) {
    const int64_t pixel_bytes = cells * 3 * (run->cfg.img_dtype == 2 ? 2 : 1);
    f->grid_doubles = 5 * cells;
    f->image_bytes = (pixel_bytes + cells + 255) & ~(int64_t)255;
    if (run->full || run->grid_used + f->grid_doubles > run->grids_capacity || run->image_used + f->image_bytes > run->images_capacity)
        return false;
    f->mean = run->grids + run->grid_used, f->count = f->mean + 4 * cells;
    f->image = run->images + run->image_used;
    f->mask = reinterpret_cast<uint8_t*>(run->images + run->image_used + pixel_bytes);
    return true;
}

// The second pass of frame k (how != fused) into f, on the context's stream behind the frame's big kernel (and the batch
// launched after it): every such pass of the call runs in stream order, so they share the workspace of that stream.
int second_pass(amt_run* run, pass how, int k, const amt_pipe_result& pr, const frame_outputs& f) {
    amt_ctx* ctx = run->ctx;
    const amt_run_config& cfg = run->cfg;
    slot& s = run->slot_of(k);
    const amt_georef_out& o = s.out;
    const bool mag = cfg.magnetic != 0;
    int rc = AMT_OK;
    if (how == pass::ordered) {
        rc = run->has_quantile
                 ? amt_quantile_frame_async(ctx, mag ? o.mlat_c : o.lat_c, mag ? o.mlt_c : o.lon_c, o.elev, s.img, cfg.img_dtype, 3,
                                            nullptr, cfg.height, cfg.width, cfg.min_elevation, &pr.grid.xaxis, &pr.grid.yaxis,
                                            pr.lon_wrapped, mag ? 1 : 0, &run->quantile, 1, f.mean, f.image, f.mask, f.count)
                 : amt_median_frame_async(ctx, mag ? o.mlat_c : o.lat_c, mag ? o.mlt_c : o.lon_c, o.elev, s.img, cfg.img_dtype, 3,
                                          nullptr, cfg.height, cfg.width, cfg.min_elevation, &pr.grid.xaxis, &pr.grid.yaxis,
                                          pr.lon_wrapped, mag ? 1 : 0, f.mean, f.image, f.mask, f.count);
    } else if (how == pass::area) {
        // the rows that can be binned (amt_georef_image_rows is conservative for exactly the pixels this pass admits: centre on
        // the shell, elevation >= min_elevation): of a host image only those were uploaded, the others hold an older frame's bytes
        int32_t r0 = 0, r1 = cfg.height;
        if (int rc2 = amt_georef_image_rows(&s.prm, cfg.min_elevation, &r0, &r1)) return rc2;
        r0 = std::min(std::max(r0, 0), cfg.height);
        r1 = std::min(std::max(r1, r0), cfg.height);
        rc = amt_area_frame_async(ctx, mag ? o.mlat : o.lat, mag ? o.mlt : o.lon, mag ? o.mlat_c : o.lat_c, o.elev, s.img,
                                  cfg.img_dtype, 3, nullptr, cfg.height, cfg.width, cfg.min_elevation, &pr.grid.xaxis,
                                  &pr.grid.yaxis, pr.lon_wrapped, mag ? 1 : 0, r0, r1, run->min_weight, f.mean, f.image, f.mask,
                                  f.count, run->over + k);
    } else {
        rc = amt_pipe_general_finalize(s.pipe, f.mean, f.image, f.mask, f.count);
    }
    if (rc) return rc;
    if (s.img == s.own_img && s.own_img != nullptr) {
        // the pass reads the slot's image buffer on the context's stream: the slot's next upload waits for it
        AMT_HIP(ctx, hipEventRecord(s.img_free, ctx->stream));
        s.img_busy = true;
    }
    return AMT_OK;
}

int run_finish(amt_run* run, batch b) {
    const amt_run_config& cfg = run->cfg;
    // the fused frames of the batch: one finalise kernel for all of them
    amt_pipe* pp[AMT_PIPE_MAX_BATCH];
    double* mean[AMT_PIPE_MAX_BATCH];
    void* oimg[AMT_PIPE_MAX_BATCH];
    uint8_t* omask[AMT_PIPE_MAX_BATCH];
    double* ocount[AMT_PIPE_MAX_BATCH];
    int m = 0;
    for (int k = b.k0; k < b.k0 + b.count; ++k) {
        slot& s = run->slot_of(k);
        amt_run_result& r = run->results[k];
        std::memset(&r, 0, sizeof(r));
        r.slot = k % cfg.n_slots, r.hinted = s.hinted;
        r.altitude = s.alt, r.params = s.prm;
        r.lat_px_per_deg = s.ppd_lat, r.lon_px_per_deg = s.ppd_lon;
        r.uploaded_bytes = s.uploaded_bytes;
        if (s.pre_status != 0) {
            // box-first plan: the box pass found no valid pixel (2) or a pole in view (4); nothing was launched
            r.status = s.pre_status;
            forget_hints(run);
            continue;
        }
        amt_pipe_result pr;
        if (int rc = amt_pipe_wait(s.pipe, &pr)) return rc;
        if (pr.status == 1 && pr.fused && !cfg.two_pass && pr.bbox[6] > 0 && pr.edge_pixels <= AMT_PIPE_MAX_EDGE_PIXELS) {
            // handed back although the launch was fused — the exact box does not fit the superset grid of a poor estimate,
            // the date line judged differently —: once more, with the exact box (in the coordinates of the plan: bbox[7])
            // as the estimate.  On the context's stream, behind the batch launched after this one; rare.
            // (it writes every sky row again — nothing known —, and the slot then holds this frame's sky)
            const int one = r.slot;
            if (int rc = amt_pipe_coarse_hint(s.pipe, pr.bbox, cfg.magnetic ? 1 : 0)) return rc;
            if (int rc = launch_slots(run, &one, 1, true)) return rc;
            if (int rc = amt_pipe_wait(s.pipe, &pr)) return rc;
            r.retried = 1;
        }
        pass how;
        if (int rc = choose_pass(run, s, &pr, &how)) return rc;
        r.status = pr.status;
        r.two_pass = how != pass::fused ? 1 : 0;
        std::memcpy(r.bbox, pr.bbox, sizeof(r.bbox));
        r.edge_pixels = pr.edge_pixels;
        if (pr.status != 0) {
            forget_hints(run);
            continue;
        }
        frame_outputs f;
        if (!next_outputs(run, (int64_t)pr.grid.ny * pr.grid.nx, &f)) {
            // no room: this frame's accumulators are dropped with the frame (the driver zeroes them before its next
            // launch); the caller runs the rest again with larger arenas
            run->full = true;
            r.status = 3;
            continue;
        }
        r.ny = pr.grid.ny, r.nx = pr.grid.nx;
        r.contains_pole = pr.bbox[7] != 0 ? 1 : 0;
        r.lon_wrapped = pr.lon_wrapped;
        r.grid = pr.grid;
        r.grid_offset = run->grid_used, r.image_offset = run->image_used;
        if (how == pass::fused) {
            pp[m] = s.pipe;
            mean[m] = f.mean, ocount[m] = f.count, oimg[m] = f.image, omask[m] = f.mask;
            ++m;
        } else if (int rc = second_pass(run, how, k, pr, f)) {
            return rc;
        }
        run->grid_used += f.grid_doubles;
        run->image_used += f.image_bytes;
        remember_hint(run, s, k, pr.bbox);
    }
    if (m > 0)
        if (int rc = amt_pipe_finalize_many(pp, m, mean, oimg, omask, ocount)) return rc;
    return AMT_OK;
}

// the frames of the batch that are launched (box-first plan: not those without a valid pixel or with a pole in view), as runs
// of consecutive frames
int run_launch(amt_run* run, batch b) {
    int slots[AMT_PIPE_MAX_BATCH];
    for (int i = 0; i < b.count; ++i) {             // (past the frame that ended the run)
        int m = 0;
        for (; i < b.count && run->slot_of(b.k0 + i).pre_status == 0; ++i) slots[m++] = (b.k0 + i) % run->cfg.n_slots;
        if (m > 0)
            if (int rc = launch_slots(run, slots, m)) return rc;
    }
    return AMT_OK;
}

// ---- box-first plan (cfg.arcsec_per_px > 0) --------------------------------------------------------------------------
// box(b): ONE launch of the frame kernel without outputs for the batch's frames (amt_pipe_launch_box_many)
int run_box(amt_run* run, batch b) {
    amt_pipe* pp[AMT_PIPE_MAX_BATCH];
    const amt_frame_params* prm[AMT_PIPE_MAX_BATCH];
    for (int i = 0; i < b.count; ++i) {
        slot& s = run->slot_of(b.k0 + i);
        pp[i] = s.pipe, prm[i] = &s.prm;
        s.pre_status = 0;
    }
    return amt_pipe_launch_box_many(pp, b.count, prm, run->cfg.min_elevation, run->cfg.magnetic ? 1 : 0);
}

// the boxes of a boxed batch -> px/deg per frame (BaseMapping.boundingBox of the reduction, reference mapping.py:711-741, then
// plateCarreeResolution, resample.py:36-61), the exact box as the estimate of the single-pass launch
int run_resolve(amt_run* run, batch b) {
    const amt_run_config& cfg = run->cfg;
    for (int i = 0; i < b.count; ++i) {
        slot& s = run->slot_of(b.k0 + i);
        amt_pipe_result pr;
        if (int rc = amt_pipe_wait(s.pipe, &pr)) return rc;
        const double* box = pr.bbox;
        if (pr.status == 2 || !(box[6] > 0)) {
            s.pre_status = 2;
            continue;
        }
        amt_gl::box_range r;
        double la = 0, lo = 0;
        if (box[7] != 0 || !amt_gl::range_of_box(box, &r) ||
            !amt_gl::plate_carree_resolution(r.lat_lo, r.west, r.lat_hi, r.east, cfg.arcsec_per_px, &la, &lo) || !(lo > 0)) {
            s.pre_status = 4;
            continue;
        }
        s.ppd_lat = la, s.ppd_lon = lo;
        if (int rc = amt_pipe_coarse_hint(s.pipe, box, cfg.magnetic ? 1 : 0)) return rc;
        s.hinted = 1;
    }
    return AMT_OK;
}

// frames that were only prepared (the arenas ran full, the call failed) are reported as not processed
void mark_not_processed(amt_run* run, batch b) {
    for (int i = 0; i < b.count; ++i) {
        std::memset(&run->results[b.k0 + i], 0, sizeof(amt_run_result));
        run->results[b.k0 + i].status = 3;
    }
}

// box-first plan: the oldest boxed batch -> resolutions, its single-pass launch; then at most one batch stays in flight
int run_launch_boxed(amt_run* run) {
    const batch b = run->boxed.front();
    run->boxed.pop();
    if (int rc = run_resolve(run, b)) return rc;
    if (!run->full)
        if (int rc = run_launch(run, b)) return rc;
    // (arenas full: the frames were not launched, and run_finish reports them as not processed)
    if (run->full)
        for (int i = 0; i < b.count; ++i)
            if (run->slot_of(b.k0 + i).pre_status == 0) run->slot_of(b.k0 + i).pre_status = 3;
    run->launched.push(b);
    while (run->launched.size() > 1) {
        if (int rc = run_finish(run, run->launched.front())) return rc;
        run->launched.pop();
    }
    return AMT_OK;
}

// box-first plan, a complete batch b of prepared frames: launch(b - 2), finish(b - 3), box(b)
int run_batch_ready_box(amt_run* run, batch b) {
    if (run->boxed.size() == 2)
        if (int rc = run_launch_boxed(run)) return rc;
    if (run->full) {
        mark_not_processed(run, b);
        return AMT_OK;
    }
    if (int rc = run_box(run, b)) return rc;
    run->boxed.push(b);
    return AMT_OK;
}

// a complete batch of prepared frames: finish the older of two batches in flight, then launch it
int run_batch_ready(amt_run* run, batch b) {
    if (run->cfg.arcsec_per_px > 0) return run_batch_ready_box(run, b);
    if (run->launched.size() == 2) {
        if (int rc = run_finish(run, run->launched.front())) return rc;
        run->launched.pop();
    }
    if (run->full) {
        mark_not_processed(run, b);
        return AMT_OK;
    }
    if (int rc = run_launch(run, b)) return rc;
    run->launched.push(b);
    return AMT_OK;
}

// A frame whose image lies in page-locked HOST memory: the rows of it that can be binned (amt_georef_image_rows: inside the limb
// and inside the cone of elevations >= min_elevation) go to the slot's own device buffer on the runner's copy stream, now — the
// frame is launched one batch later, behind the batch that is running —, and the launch waits for the event behind them.
int run_upload(amt_run* run, slot& s, const void* host) {
    amt_ctx* ctx = run->ctx;
    const amt_run_config& cfg = run->cfg;
    const size_t row_bytes = (size_t)cfg.width * 3 * (cfg.img_dtype == 2 ? 2 : 1);
    if (run->copy_stream == nullptr) AMT_HIP(ctx, hipStreamCreateWithFlags(&run->copy_stream, hipStreamNonBlocking));
    if (s.own_img == nullptr)
        if (int rc = slot_image_create(ctx, s, row_bytes * cfg.height)) return rc;
    int32_t r0 = 0, r1 = cfg.height;
    if (int rc = amt_georef_image_rows(&s.prm, cfg.min_elevation, &r0, &r1)) return rc;
    if (s.img_busy) {
        AMT_HIP(ctx, hipStreamWaitEvent(run->copy_stream, s.img_free, 0));
        s.img_busy = false;
    }
    if (r1 > r0) {
        // (one copy: the band in two or three pieces on as many streams is slower, 13.7 / 12.9 k against 15.7 k Mpixel/s —
        // profiles/REJECTED.md)
        AMT_HIP(ctx, hipMemcpyAsync(static_cast<char*>(s.own_img) + (size_t)r0 * row_bytes,
                                    static_cast<const char*>(host) + (size_t)r0 * row_bytes, (size_t)(r1 - r0) * row_bytes,
                                    hipMemcpyHostToDevice, run->copy_stream));
        AMT_HIP(ctx, hipEventRecord(s.uploaded, run->copy_stream));
        s.upload_pending = true;
    }
    s.uploaded_bytes = (int64_t)(r1 - r0) * (int64_t)row_bytes;
    s.img = s.own_img;
    return AMT_OK;
}

int run_push_impl(amt_run* run, const amt_run_frame* f) {
    amt_ctx* ctx = run->ctx;
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, run->active, "amt_run_push without amt_run_begin");
    AMT_REQUIRE(ctx, f != nullptr, "NULL frame");
    AMT_REQUIRE(ctx, run->n_pushed < run->max_frames, "more frames than amt_run_begin announced");
    const amt_run_config& cfg = run->cfg;
    const int k = run->n_pushed++;
    mark_not_processed(run, {k, 1});                // until the frame is finished (also if this call fails)
    if (run->full) return AMT_OK;
    // the slot's previous frame (k - n_slots) may still be in flight: it is finished before its slot — parameters, shell,
    // driver — takes the new frame.  (With n_slots = 2 * batch that is the batch launched before the one now running, so
    // nothing waits that the loop `launch(B); finish(A); prepare(C)` would not wait for.)
    for (;;) {
        if (run->launched.size() > 0 && run->launched.front().k0 <= k - cfg.n_slots) {
            if (int rc = run_finish(run, run->launched.front())) return rc;
            run->launched.pop();
            if (run->full) return AMT_OK;
            continue;
        }
        if (run->boxed.size() > 0 && run->boxed.front().k0 <= k - cfg.n_slots) {
            if (int rc = run_launch_boxed(run)) return rc;      // (cannot happen with n_slots >= 3 * batch)
            continue;
        }
        break;
    }
    slot& s = run->slot_of(k);
    const int mag = cfg.magnetic ? 1 : 0;
    const double altitude = f->altitude > 0 ? f->altitude : cfg.altitude;
    // (the J2000 -> SM matrix only where somebody reads it: MLat / MLT grids or arrays)
    const int want_sm = mag || s.out.mlat != nullptr || s.out.mlat_c != nullptr;
    int rc = amt_prm::frame_params(f, cfg.width, cfg.height, cfg.fast_center, altitude, want_sm, &s.prm);
    if (rc != AMT_OK) {
        ctx->last_error = "amt_run_push: the date of a frame is outside the IGRF table";
        return rc;
    }
    s.alt = altitude;
    s.img = f->img;
    s.uploaded_bytes = 0;
    s.upload_pending = false;
    if (f->img == nullptr && f->img_host != nullptr)
        if (int rc2 = run_upload(run, s, f->img_host)) return rc2;
    s.pre_status = 0;
    if (!(cfg.arcsec_per_px > 0)) {
        double est[8];
        const bool hint = cfg.use_hints && box_hint(run, run->frames_done + k, s.prm, est);
        rc = hint ? amt_pipe_coarse_hint(s.pipe, est, mag) : amt_pipe_coarse(s.pipe, &s.prm, cfg.min_elevation, mag);
        if (rc != AMT_OK) return rc;
        s.hinted = hint ? 1 : 0;
    }
    if (run->collecting.count == 0) run->collecting.k0 = k;
    ++run->collecting.count;
    // the first launch carries one frame only: the GPU starts after one frame's preparation instead of `batch`
    // (sizing the first launch so that the LAST one of the announced frames is full — 20 frames as 2 + 6 x 3 instead of
    // 1 + 6 x 3 + 1 — was measured in round 4: 287 against 251 us of non-kernel time per 20-frame call; not kept)
    if (run->collecting.count == (k == 0 && !(cfg.arcsec_per_px > 0) ? 1 : cfg.batch)) {
        rc = run_batch_ready(run, run->collecting);
        run->collecting.count = 0;
    }
    return rc;
}

}  // namespace

extern "C" {

int amt_run_begin(amt_run* run, double* grids, int64_t grids_capacity, void* images, int64_t images_capacity,
                  amt_run_result* results, int32_t max_frames) {
    if (run == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = run->ctx;
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, !run->active, "amt_run_begin: a call is already in progress (amt_run_end it first)");
    AMT_REQUIRE(ctx, max_frames >= 0 && (max_frames == 0 || results != nullptr), "NULL argument");
    AMT_REQUIRE(ctx, max_frames == 0 || (grids != nullptr && images != nullptr), "the arenas are NULL");
    if (amt_set_device(ctx)) return AMT_EHIP;
    // the finalise kernels run on a stream of the drivers' own and write into the arenas: whatever the context's stream
    // has queued on that memory before this call must be done first
    void* fin = nullptr;
    if (int rc = amt_pipe_finalize_stream(run->slots[0].pipe, &fin)) return rc;
    AMT_HIP(ctx, hipEventRecord(run->entry, ctx->stream));
    AMT_HIP(ctx, hipStreamWaitEvent(static_cast<hipStream_t>(fin), run->entry, 0));
    if (run->cfg.statistic == 2 && max_frames > 0) {
        if (max_frames > run->over_capacity) {
            // (hipFree waits for whatever still uses the old words)
            if (run->over) (void)hipFree(run->over);
            run->over = nullptr;
            run->over_capacity = 0;
            const int cap = std::max(max_frames, 64);
            if (hipMalloc(reinterpret_cast<void**>(&run->over), (size_t)cap * sizeof(uint32_t)) != hipSuccess) {
                (void)hipGetLastError();
                run->over = nullptr;
                ctx->last_error = "amt_run_begin: no device memory for the overflow flags";
                return AMT_ENOMEM;
            }
            run->over_capacity = cap;
        }
        AMT_HIP(ctx, hipMemsetAsync(run->over, 0, (size_t)max_frames * sizeof(uint32_t), ctx->stream));
    }
    run->grids = grids, run->grids_capacity = grids_capacity;
    run->images = static_cast<char*>(images), run->images_capacity = images_capacity;
    run->results = results, run->max_frames = max_frames;
    run->grid_used = run->image_used = 0;
    run->full = false;
    run->n_pushed = 0;
    run->collecting = {0, 0}, run->launched = {}, run->boxed = {};
    forget_sky(run);                                // whatever the caller did with the slots' arrays since the last call
    run->launch_stream = ctx->stream;
    run->bands_filled = run->bands_skipped = 0;
    run->role_items[0] = run->role_items[1] = run->role_items[2] = 0;
    run->core_items = 0;
    run->active = true;
    return AMT_OK;
}

int amt_run_push(amt_run* run, const amt_run_frame* f) {
    if (run == nullptr) return AMT_EINVAL;
    const int rc = run_push_impl(run, f);
    //  a failed push leaves no hints behind whose indices refer to frames that were never counted; and a launch or
    // a wait failed somewhere in the queue: what the slots hold is anybody's guess
    if (rc != AMT_OK) forget_hints(run), forget_sky(run);
    return rc;
}

int amt_run_end(amt_run* run, int32_t* frames_done) {
    if (run == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = run->ctx;
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, run->active, "amt_run_end without amt_run_begin");
    run->active = false;
    int rc_all = AMT_OK;
    if (run->collecting.count > 0) {
        rc_all = run_batch_ready(run, run->collecting);
        run->collecting.count = 0;
    }
    while (run->boxed.size() > 0 && rc_all == AMT_OK) rc_all = run_launch_boxed(run);
    for (; run->launched.size() > 0; run->launched.pop()) {
        const int rc = run_finish(run, run->launched.front());
        if (rc_all == AMT_OK) rc_all = rc;
    }
    // host images are read "until amt_run_end returns": the upload of a frame that was pushed but never launched (arenas full, a
    // failed call) may still be in flight
    if (run->copy_stream != nullptr && hipStreamSynchronize(run->copy_stream) != hipSuccess && rc_all == AMT_OK) {
        (void)hipGetLastError();
        ctx->last_error = "amt_run_end: the copy stream failed";
        rc_all = AMT_EHIP;
    }
    // order the context's stream behind every finalise kernel of this call
    for (slot& s : run->slots) {
        s.upload_pending = false;
        const int rc = amt_pipe_join(s.pipe);
        if (rc_all == AMT_OK) rc_all = rc;
    }
    if (rc_all != AMT_OK) {
        //  a failed call leaves no half-valid state behind: no hints, nothing counted
        forget_hints(run), forget_sky(run);
        if (frames_done) *frames_done = 0;
        return rc_all;
    }
    const int n = run->n_pushed;
    int done = n;
    for (int i = 0; i < n; ++i)
        if (run->results[i].status == 3) {
            done = i;
            break;
        }
    for (int i = done; i < n; ++i) run->results[i].status = 3;
    if (frames_done) *frames_done = done;
    run->frames_done += done;
    if (done < n) forget_hints(run);
    return AMT_OK;
}

int amt_run_process(amt_run* run, const amt_run_frame* frames, int32_t n, double* grids, int64_t grids_capacity,
                    void* images, int64_t images_capacity, amt_run_result* results, int32_t* frames_done) {
    if (run == nullptr) return AMT_EINVAL;
    amt_ctx* ctx = run->ctx;
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, n >= 0 && (n == 0 || frames != nullptr), "NULL argument");
    if (frames_done) *frames_done = 0;
    if (n == 0) return AMT_OK;
    if (int rc = amt_run_begin(run, grids, grids_capacity, images, images_capacity, results, n)) return rc;
    int rc_all = AMT_OK;
    for (int i = 0; i < n && rc_all == AMT_OK; ++i) rc_all = amt_run_push(run, frames + i);
    const int rc = amt_run_end(run, frames_done);
    return rc_all != AMT_OK ? rc_all : rc;
}

}  // extern "C"
