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

constexpr int kSelTile = 16;        // k_mosaic_select: one workgroup per 16 x 16 cells of the common grid

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
    const int tile = (int)blockIdx.x;
    const int tx = tile / S.tiles_y, ty = tile - tx * S.tiles_y;
    const int cx = tx * kSelTile + (int)(threadIdx.x % kSelTile), cy = ty * kSelTile + (int)(threadIdx.x / kSelTile);
    if (cx >= S.nx || cy >= S.ny) return;
    const int64_t i = (int64_t)(S.ny - 1 - cy) * S.nx + cx;      // output row r = ny - 1 - cy (north to south)
    const int nch = S.nch;
    const int b = S.list_start[tile], e = S.list_start[tile + 1];
    unsigned long long cnt = 0, sums[4] = {0, 0, 0, 0};
    long long fx = 0;
    int src = -1;
    double best = 0.0;
    for (int k = b; k < e; ++k) {
        const int m = S.list[k];
        const mosaic_dev& D = S.members[m];
        const int wx = cx - D.W.x0, wy = cy - D.W.y0;
        if (wx < 0 || wx >= D.W.nx || wy < 0 || wy >= D.W.ny) continue;
        const unsigned long long* acc = D.A.acc;
        const int64_t plane = (int64_t)D.W.nx * D.W.ny, cell = (int64_t)wx * D.W.ny + wy;
        const unsigned long long c = acc[cell];
        if (c == 0) continue;
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
    }
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
    AMT_REQUIRE(ctx, n_members >= 1, "no members");
    AMT_REQUIRE(ctx, rule == 0 || rule == 1, "rule must be 0 (union) or 1 (highest elevation)");
    AMT_REQUIRE(ctx, nchan >= 0 && nchan <= 4, "nchan must be 0..4");
    AMT_REQUIRE(ctx, out_img == nullptr || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    AMT_REQUIRE(ctx, axis_ok(xaxis) && axis_ok(yaxis), "bad axis");
    AMT_REQUIRE(ctx, xaxis->nbin < 65535 && yaxis->nbin < 65535, "at most 65534 bins per axis");
    const int nx = xaxis->nbin, ny = yaxis->nbin;
    for (int32_t i = 0; i < n_members; ++i) {
        const amt_mosaic_member& m = members[i];
        AMT_REQUIRE(ctx, m.lat_c && m.lon_c && m.height > 0 && m.width > 0, "member without centres");
        AMT_REQUIRE(ctx, nchan == 0 || (m.img && (img_dtype == 1 || img_dtype == 2)), "member image missing");
        AMT_REQUIRE(ctx, rule == 0 || m.elev != nullptr, "rule 1 needs every member's elevation");
        AMT_REQUIRE(ctx, m.win_nx >= 0 && m.win_ny >= 0, "bad window");
        AMT_REQUIRE(ctx, m.win_nx == 0 || m.win_ny == 0 ||
                         (m.win_x0 >= 0 && m.win_y0 >= 0 && m.win_x0 + m.win_nx <= nx && m.win_y0 + m.win_ny <= ny),
                    "window outside the grid");
    }
    if (amt_set_device(ctx)) return AMT_EHIP;

    // host tables: member descriptors | tile prefix [n + 1] | CSR of the 16 x 16 cell tiles; then the accumulators
    axis_dev ax, ay;
    make_axis(xaxis, &ax);
    make_axis(yaxis, &ay);
    const int stx = (nx + kSelTile - 1) / kSelTile, sty = (ny + kSelTile - 1) / kSelTile;
    const int64_t n_sel = (int64_t)stx * sty;
    std::vector<mosaic_dev> dev((size_t)n_members);
    std::vector<int> tile_start((size_t)n_members + 1, 0);
    std::vector<int> list_start((size_t)n_sel + 1, 0), list;
    std::vector<size_t> acc_off((size_t)n_members, 0);
    size_t acc_words = 0;
    bool vec = true;
    auto aligned16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    auto aligned4 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; };
    int64_t tiles = 0;
    for (int32_t i = 0; i < n_members; ++i) {
        const amt_mosaic_member& m = members[i];
        mosaic_dev& d = dev[(size_t)i];
        const bool empty = m.win_nx == 0 || m.win_ny == 0;
        d.A.lat_c = m.lat_c;
        d.A.lon_c = m.lon_c;
        d.A.elev = m.elev;
        d.A.img = m.img;
        d.A.mask = m.center_mask;
        d.A.height = m.height;
        d.A.width = m.width;
        d.A.min_elev = min_elevation;
        d.A.use_elev_threshold = (m.elev != nullptr) && !(std::isinf(min_elevation) && min_elevation < 0);
        d.A.ax = ax;
        d.A.ay = ay;
        d.A.lon_wrap = lon_wrap ? 1 : 0;
        d.A.acc = nullptr;
        d.W = {m.win_x0, m.win_y0, empty ? 0 : m.win_nx, empty ? 0 : m.win_ny};
        const int64_t tiles_x = (m.width + kBW - 1) / kBW, tiles_y = (m.height + kBH * kRowIters - 1) / (kBH * kRowIters);
        tile_start[(size_t)i] = (int)tiles;
        if (!empty) {
            tiles += tiles_x * tiles_y;
            acc_off[(size_t)i] = acc_words;
            acc_words += (size_t)(nchan + 2) * (size_t)m.win_nx * (size_t)m.win_ny;
            // (as amt_bin_frame: even width, 16-byte aligned coordinates and a 4-byte aligned image, of every member)
            vec = vec && (m.width % 2 == 0) && aligned16(m.lat_c) && aligned16(m.lon_c) &&
                  (m.elev == nullptr || aligned16(m.elev)) && (nchan == 0 || aligned4(m.img));
        }
        AMT_REQUIRE(ctx, tiles < (int64_t)1 << 31, "too many tiles");
    }
    tile_start[(size_t)n_members] = (int)tiles;
    for (int tx = 0; tx < stx; ++tx)
        for (int ty = 0; ty < sty; ++ty) {
            const int64_t t = (int64_t)tx * sty + ty;
            list_start[(size_t)t] = (int)list.size();
            for (int32_t i = 0; i < n_members; ++i) {
                const bin_window& w = dev[(size_t)i].W;
                if (w.nx == 0) continue;
                if (w.x0 < (tx + 1) * kSelTile && w.x0 + w.nx > tx * kSelTile && w.y0 < (ty + 1) * kSelTile &&
                    w.y0 + w.ny > ty * kSelTile)
                    list.push_back(i);
            }
        }
    list_start[(size_t)n_sel] = (int)list.size();

    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_tstart = up(dev.size() * sizeof(mosaic_dev));
    const size_t o_lstart = o_tstart + up(tile_start.size() * sizeof(int));
    const size_t o_list = o_lstart + up(list_start.size() * sizeof(int));
    const size_t o_acc = o_list + up(std::max<size_t>(list.size(), 1) * sizeof(int));
    const size_t bytes = o_acc + std::max<size_t>(acc_words, 1) * sizeof(unsigned long long);
    const size_t o_tail = up(bytes);
    char* ws = static_cast<char*>(amt_workspace(ctx, tail_bytes ? o_tail + tail_bytes : bytes));
    if (ws == nullptr) {
        ctx->last_error = "amt_mosaic_frames: workspace allocation failed";
        return AMT_ENOMEM;
    }
    if (tail != nullptr) *tail = ws + o_tail;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws + o_acc);
    for (int32_t i = 0; i < n_members; ++i) dev[(size_t)i].A.acc = acc + acc_off[(size_t)i];
    std::vector<char> host(o_acc, 0);
    std::memcpy(host.data(), dev.data(), dev.size() * sizeof(mosaic_dev));
    std::memcpy(host.data() + o_tstart, tile_start.data(), tile_start.size() * sizeof(int));
    std::memcpy(host.data() + o_lstart, list_start.data(), list_start.size() * sizeof(int));
    if (!list.empty()) std::memcpy(host.data() + o_list, list.data(), list.size() * sizeof(int));
    // (pageable source: the copy has consumed `host` when the call returns)
    AMT_HIP(ctx, hipMemcpyAsync(ws, host.data(), o_acc, hipMemcpyHostToDevice, ctx->stream));
    if (acc_words) AMT_HIP(ctx, hipMemsetAsync(acc, 0, acc_words * sizeof(unsigned long long), ctx->stream));

    if (tiles > 0) {
        mosaic_args M;
        M.members = reinterpret_cast<const mosaic_dev*>(ws);
        M.tile_start = reinterpret_cast<const int*>(ws + o_tstart);
        M.n = n_members;
        const dim3 grid((unsigned)tiles), block(kBinBlock);
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
    S.members = reinterpret_cast<const mosaic_dev*>(ws);
    S.list_start = reinterpret_cast<const int*>(ws + o_lstart);
    S.list = reinterpret_cast<const int*>(ws + o_list);
    S.tiles_y = sty;
    S.nx = nx;
    S.ny = ny;
    S.nch = nchan;
    S.rule = rule;
    S.mean = mean;
    S.img = out_img;
    S.mask = out_mask;
    S.count = out_count;
    S.source = out_source ? out_source : (tail ? reinterpret_cast<int32_t*>(ws + o_tail) : nullptr);
    const dim3 sgrid((unsigned)n_sel), sblock(kSelTile * kSelTile);
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
