// Mosaic binning: the members of a MappingCollection binned onto ONE grid (auromat_amd.resample.resampleMosaic).
//
// A fixed number of launches whatever the member count: the member table is uploaded, the members' window accumulators
// are zeroed, one launch of k_bin_frame<..., WIN = true> ("k_mosaic_bin", amt_bin_tile.h: the frame kernel restricted to
// each member's window of the common grid) bins every member's tiles, and k_mosaic_select gives every output cell its value
// by the overlap rule.
// Integer sums and an ordered walk over the members make the result independent of the order in which tiles run.
// The median and quantile mosaics (amt_median.hip) run the same binning and election for `source` alone (amt_mosaic_run).
#include <algorithm>

#include "amt_common.h"
#include "amt_bin_tile.h"

namespace {

using namespace amt;

struct select_args {
    const mosaic_dev* __restrict__ members;
    const int* __restrict__ list_start;     // CSR per 16 x 16 tile of cells: members whose window meets the tile,
    const int* __restrict__ list;           // ascending
    int tiles_y;                            // tiles along the (ascending) latitude bins
    int nx, ny, nch, rule;
    double* mean;
    void* img;
    uint8_t* mask;
    double* count;
    int32_t* source;
};

// One thread per output cell: the cell's tile's members, in ascending order.  rule 0: the sums of every member that has
// pixels there (source: the first); rule 1: the member with the largest mean elevation, computed as the finalise step
// computes it, the first on a tie.  Then the finalise arithmetic of k_bin_finalize (finalize_cell).
template <typename IMG_T>
__global__ __launch_bounds__(kSelTile * kSelTile) void k_mosaic_select(select_args S) {
    int cx, cy;
    const int64_t i = select_cell(S.tiles_y, S.nx, S.ny, cx, cy);
    if (i < 0) return;
    const int nch = S.nch;
    unsigned long long cnt = 0, sums[4] = {0, 0, 0, 0};
    long long fx = 0;
    int src = -1;
    double best = 0.0;
    walk_tile_members(S.members, S.list_start, S.list, cx, cy,
                      [&](int m, const unsigned long long* acc, int64_t plane, int64_t cell) {
        const unsigned long long c = acc[cell];
        if (c == 0) return;
        const long long f = (long long)acc[(int64_t)(1 + nch) * plane + cell];
        if (S.rule == 0) {
            cnt += c;
            fx += f;
            for (int ch = 0; ch < nch; ++ch) sums[ch] += acc[(int64_t)(1 + ch) * plane + cell];
            if (src < 0) src = m;
        } else {
            const double el = ((double)f / kFix) / (double)c;      // finalize_cell's elevation mean
            if (src < 0 || el > best) {
                src = m;
                best = el;
                cnt = c;
                fx = f;
                for (int ch = 0; ch < nch; ++ch) sums[ch] = acc[(int64_t)(1 + ch) * plane + cell];
            }
        }
    });
    finalize_cell(cnt, [&](int ch) { return sums[ch]; }, [&]() { return fx; }, nch, i, S.mean, static_cast<IMG_T*>(S.img),
                  S.mask, S.count, cell_wants{S.mean != nullptr, S.img != nullptr, S.mask != nullptr, S.count != nullptr});
    if (S.source) S.source[i] = src;
}

}  // namespace

// amt_mosaic_frames; `tail_bytes` more bytes of the context's workspace behind the call's own tables and accumulators are
// handed to the caller through `tail` (256-byte aligned): amt_mosaic_median_frames and amt_mosaic_quantile_frames
// (amt_median.hip) keep the median workspace there, in the same allocation, so that one call sizes the workspace once; with a
// tail and no out_source the elected member of every cell ((ny, nx) int32) is written to the tail's first bytes.
int amt_mosaic_run(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype, int32_t nchan,
                   double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, int32_t rule, double* mean,
                   void* out_img, uint8_t* out_mask, double* out_count, int32_t* out_source, size_t tail_bytes, char** tail) {
    AMT_REQUIRE(ctx, members && xaxis && yaxis, "NULL argument");
    AMT_REQUIRE(ctx, out_img == nullptr || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    const int nx = xaxis->nbin, ny = yaxis->nbin;
    const char* bad = mosaic_members_bad(members, n_members, rule, nchan, axis_ok(xaxis) && axis_ok(yaxis), nx, ny,
                                         [](const amt_mosaic_member& m) { return m.lon_c ? nullptr : "member without centres"; });
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    AMT_REQUIRE(ctx, nchan == 0 || img_dtype == 1 || img_dtype == 2, "member image missing");
    if (amt_set_device(ctx)) return AMT_EHIP;

    mosaic_plan P;
    const bool fits = plan_members(P, members, n_members, nx, ny, nchan, [](const amt_mosaic_member& m) {
        return (int64_t)((m.width + kBW - 1) / kBW) * ((m.height + kBH * kRowIters - 1) / (kBH * kRowIters));
    });
    AMT_REQUIRE(ctx, fits, "too many tiles");
    plan_select_lists(P);

    // the workspace: member descriptors | tile prefix [n + 1] | CSR of the select tiles (one upload); the accumulators; the tail
    std::vector<mosaic_dev> dev((size_t)n_members);
    workspace_packer K;
    const size_t o_dev = K.upload(dev.data(), dev.size() * sizeof(mosaic_dev));      // (filled below, copied by K.host())
    const size_t o_tstart = K.upload(P.unit_start.data(), P.unit_start.size() * sizeof(int));
    const size_t o_lstart = K.upload(P.list_start.data(), P.list_start.size() * sizeof(int));
    const size_t o_list = K.upload(P.list.data(), P.list.size() * sizeof(int));
    const size_t o_acc = K.add(std::max<size_t>(P.acc_words, 1) * sizeof(unsigned long long));
    const size_t o_tail = tail ? K.add(tail_bytes) : 0;
    char* ws = static_cast<char*>(amt_workspace(ctx, K.total()));
    if (ws == nullptr) {
        ctx->last_error = "amt_mosaic_frames: workspace allocation failed";
        return AMT_ENOMEM;
    }
    if (tail != nullptr) *tail = ws + o_tail;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws + o_acc);

    bool vec = true;
    auto aligned16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    auto aligned4 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; };
    for (int32_t i = 0; i < n_members; ++i) {
        const amt_mosaic_member& m = members[i];
        mosaic_dev& d = dev[(size_t)i];
        bad = make_frame_src(&d.A.S, m.lat_c, m.lon_c, m.elev, m.center_mask, m.height, m.width, min_elevation, xaxis, yaxis,
                             lon_wrap, 0);
        AMT_REQUIRE(ctx, bad == nullptr, bad);          // (mosaic_members_bad has looked at every member)
        d.A.img = m.img;
        d.A.acc = acc + P.acc_off[(size_t)i];
        d.W = P.win[(size_t)i];
        // (as amt_bin_frame: even width, 16-byte aligned coordinates and a 4-byte aligned image, of every member with a window)
        if (d.W.nx != 0)
            vec = vec && (m.width % 2 == 0) && aligned16(m.lat_c) && aligned16(m.lon_c) &&
                  (m.elev == nullptr || aligned16(m.elev)) && (nchan == 0 || aligned4(m.img));
    }
    // (pageable source: the copy has consumed the staging buffer when the call returns)
    const std::vector<char> host = K.host();
    AMT_HIP(ctx, hipMemcpyAsync(ws + o_dev, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    if (P.acc_words) AMT_HIP(ctx, hipMemsetAsync(acc, 0, P.acc_words * sizeof(unsigned long long), ctx->stream));

    if (P.units > 0) {
        mosaic_args M;
        M.members = reinterpret_cast<const mosaic_dev*>(ws + o_dev);
        M.tile_start = reinterpret_cast<const int*>(ws + o_tstart);
        M.n = n_members;
        const dim3 grid((unsigned)P.units), block(kBinBlock);
        const bool u8 = img_dtype != 2;
#define AMT_MOSAIC_CASE(T, N)                                                                              \
    do {                                                                                                   \
        if (vec) hipLaunchKernelGGL((k_bin_frame<T, N, true, true>), grid, block, 0, ctx->stream, M);      \
        else hipLaunchKernelGGL((k_bin_frame<T, N, false, true>), grid, block, 0, ctx->stream, M);         \
    } while (0)
        switch (nchan) {
            case 0: AMT_MOSAIC_CASE(uint8_t, 0); break;
            case 1: if (u8) AMT_MOSAIC_CASE(uint8_t, 1); else AMT_MOSAIC_CASE(uint16_t, 1); break;
            case 2: if (u8) AMT_MOSAIC_CASE(uint8_t, 2); else AMT_MOSAIC_CASE(uint16_t, 2); break;
            case 3: if (u8) AMT_MOSAIC_CASE(uint8_t, 3); else AMT_MOSAIC_CASE(uint16_t, 3); break;
            default: if (u8) AMT_MOSAIC_CASE(uint8_t, 4); else AMT_MOSAIC_CASE(uint16_t, 4); break;
        }
#undef AMT_MOSAIC_CASE
        AMT_LAUNCH_CHECK(ctx);
    }

    select_args S;
    S.members = reinterpret_cast<const mosaic_dev*>(ws + o_dev);
    S.list_start = reinterpret_cast<const int*>(ws + o_lstart);
    S.list = reinterpret_cast<const int*>(ws + o_list);
    S.tiles_y = P.sty;
    S.nx = nx;
    S.ny = ny;
    S.nch = nchan;
    S.rule = rule;
    S.mean = mean;
    S.img = out_img;
    S.mask = out_mask;
    S.count = out_count;
    S.source = out_source ? out_source : (tail ? reinterpret_cast<int32_t*>(ws + o_tail) : nullptr);
    const dim3 sgrid((unsigned)(P.stx * P.sty)), sblock(kSelTile * kSelTile);
    if (img_dtype == 2)
        hipLaunchKernelGGL(k_mosaic_select<uint16_t>, sgrid, sblock, 0, ctx->stream, S);
    else
        hipLaunchKernelGGL(k_mosaic_select<uint8_t>, sgrid, sblock, 0, ctx->stream, S);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

extern "C" int amt_mosaic_frames(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype,
                                 int32_t nchan, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis,
                                 int lon_wrap, int32_t rule, double* mean, void* out_img, uint8_t* out_mask,
                                 double* out_count, int32_t* out_source) {
    AMT_CHECK_CTX(ctx);
    return amt_mosaic_run(ctx, members, n_members, img_dtype, nchan, min_elevation, xaxis, yaxis, lon_wrap, rule, mean, out_img,
                          out_mask, out_count, out_source, 0, nullptr);
}
