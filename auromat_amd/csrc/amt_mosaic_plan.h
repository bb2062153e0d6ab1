// What the mosaics share (amt_mosaic.hip: mean; amt_median.hip: median and quantile; amt_area.hip: area-weighted): a member's
// window of the common grid, the checks of a member table, the host plan of a call (work units per member, the members of every
// select tile, the members' accumulators) and the layout of its workspace; for the kernels, the search of a work unit's member
// and the walk over the members of a cell.  One definition each, so that a window or election rule is changed in one place.
// The host part is plain C++17 without a HIP header (tests/csrc/mosaic_plan_check.cpp compiles it alone).
#pragma once

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace amt {

constexpr int kSelTile = 16;        // the select kernels: one workgroup per 16 x 16 cells of the common grid

// Cells [x0, x0 + nx) x [y0, y0 + ny) (0-based, x = longitude bin, y = ascending latitude bin) of the common grid that a member
// keeps: pixels binned elsewhere are dropped, and the member's accumulator planes hold the window only (cell (x, y) at
// (x - x0) * ny + (y - y0), nx * ny cells per plane).  A frame binned alone has no window: {0, 0, 0, 0}.
struct cell_window {
    int x0, y0, nx, ny;
};

// The window of a member's win_* fields: without cells along either axis it is empty along both.
inline cell_window window_of(int win_x0, int win_y0, int win_nx, int win_ny) {
    const bool empty = win_nx == 0 || win_ny == 0;
    return cell_window{win_x0, win_y0, empty ? 0 : win_nx, empty ? 0 : win_ny};
}

// The checks every mosaic entry point makes of its call and its member table (amt_mosaic_member, amt_area_mosaic_member: the
// fields they share); axes_ok: axis_ok() of both axes, nx, ny: their bins; own(member): what the entry point alone asks of a
// member, asked first.  Returns what is wrong, or NULL.
template <typename MEMBER, typename OWN>
const char* mosaic_members_bad(const MEMBER* members, int32_t n_members, int32_t rule, int32_t nchan, bool axes_ok, int nx,
                               int ny, OWN own) {
    if (n_members < 1) return "no members";
    if (rule != 0 && rule != 1) return "rule must be 0 (union) or 1 (highest elevation)";
    if (nchan < 0 || nchan > 4) return "nchan must be 0..4";
    if (!axes_ok) return "bad axis";
    if (nx >= 65535 || ny >= 65535) return "at most 65534 bins per axis";
    for (int32_t i = 0; i < n_members; ++i) {
        const MEMBER& m = members[i];
        if (const char* bad = own(m)) return bad;
        if (!m.lat_c || m.height <= 0 || m.width <= 0) return "member without centres";
        if (nchan != 0 && !m.img) return "member image missing";
        if (rule != 0 && !m.elev) return "rule 1 needs every member's elevation";
        if (m.win_nx < 0 || m.win_ny < 0) return "bad window";
        if (m.win_nx != 0 && m.win_ny != 0 &&
            !(m.win_x0 >= 0 && m.win_y0 >= 0 && m.win_x0 + m.win_nx <= nx && m.win_y0 + m.win_ny <= ny))
            return "window outside the grid";
    }
    return nullptr;
}

// The host plan of a mosaic call over n members.
struct mosaic_plan {
    std::vector<cell_window> win;       // [n], by window_of
    std::vector<int> unit_start;        // [n + 1]: the first work unit (tile, workgroup) of every member; a member without a
    int64_t units = 0;                  //   window has none (equal entries); units: all of them
    std::vector<size_t> acc_off;        // [n]: the first accumulator word of a member with a window; (nchan + 2) planes of its
    size_t acc_words = 0;               //   window each; acc_words: all of them
    int stx = 0, sty = 0;               // select tiles along x and y
    std::vector<int> list_start, list;  // plan_select_lists: CSR per select tile (index tx * sty + ty) of the members whose
                                        //   window meets the tile, ascending
};

// Windows, unit prefix and accumulator offsets; units_of(member): the work units of a member that has a window.
// False when the units do not fit 31 bits (the plan is then not to be used).
template <typename MEMBER, typename UNITS>
bool plan_members(mosaic_plan& P, const MEMBER* members, int n, int nx, int ny, int nchan, UNITS units_of) {
    P = mosaic_plan{};
    P.win.resize((size_t)n);
    P.unit_start.assign((size_t)n + 1, 0);
    P.acc_off.assign((size_t)n, 0);
    P.stx = (nx + kSelTile - 1) / kSelTile;
    P.sty = (ny + kSelTile - 1) / kSelTile;
    for (int i = 0; i < n; ++i) {
        const MEMBER& m = members[i];
        const cell_window w = P.win[(size_t)i] = window_of(m.win_x0, m.win_y0, m.win_nx, m.win_ny);
        P.unit_start[(size_t)i] = (int)P.units;
        if (w.nx != 0) {
            P.units += (int64_t)units_of(m);
            P.acc_off[(size_t)i] = P.acc_words;
            P.acc_words += (size_t)(nchan + 2) * (size_t)w.nx * (size_t)w.ny;
        }
        if (P.units >= (int64_t)1 << 31) return false;
    }
    P.unit_start[(size_t)n] = (int)P.units;
    return true;
}

// The members of every select tile (the mean and the area mosaic; the ordered mosaics elect no cell of their own and skip it).
inline void plan_select_lists(mosaic_plan& P) {
    P.list_start.assign((size_t)P.stx * (size_t)P.sty + 1, 0);
    P.list.clear();
    size_t t = 0;
    for (int tx = 0; tx < P.stx; ++tx)
        for (int ty = 0; ty < P.sty; ++ty) {
            P.list_start[t++] = (int)P.list.size();
            for (size_t i = 0; i < P.win.size(); ++i) {
                const cell_window& w = P.win[i];
                if (w.nx == 0) continue;
                if (w.x0 < (tx + 1) * kSelTile && w.x0 + w.nx > tx * kSelTile && w.y0 < (ty + 1) * kSelTile &&
                    w.y0 + w.ny > ty * kSelTile)
                    P.list.push_back((int)i);
            }
        }
    P.list_start[t] = (int)P.list.size();
}

// The layout of a call's workspace: segments in the order they are added, each at a multiple of 256 bytes.  upload() adds a
// segment whose `bytes` host() copies from `src` WHEN IT IS CALLED (at least 4 bytes are reserved); the uploaded segments must
// follow one another, and host() is one staging buffer for all of them, which one copy takes to the first one's offset.
class workspace_packer {
public:
    size_t add(size_t bytes) {
        const size_t at = up(end_);
        end_ = at + bytes;
        return at;
    }
    size_t upload(const void* src, size_t bytes) {
        const size_t at = add(bytes ? bytes : 4);
        assert(parts_.empty() || at == staged_end_);
        parts_.push_back(part{at, src, bytes});
        staged_end_ = up(end_);
        return at;
    }
    std::vector<char> host() const {
        std::vector<char> h(parts_.empty() ? 0 : staged_end_ - parts_[0].at, 0);
        for (const part& p : parts_)
            if (p.bytes) std::memcpy(h.data() + (p.at - parts_[0].at), p.src, p.bytes);
        return h;
    }
    size_t total() const { return end_; }       // (the last segment's end, not rounded up)

private:
    struct part { size_t at; const void* src; size_t bytes; };
    static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
    size_t end_ = 0, staged_end_ = 0;
    std::vector<part> parts_;
};

#ifdef __HIPCC__
// The member of global work unit b: the last i with start[i] <= b (members without a window have no units: equal entries), by
// a binary search over wave-uniform loads.
__device__ __forceinline__ int member_of(const int* __restrict__ start, int n, unsigned b) {
    int lo = 0, hi = n;                     // start[lo] <= b < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)start[mid] <= b) lo = mid; else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// A select kernel's thread: cell (cx, cy) of select tile blockIdx.x (tx * tiles_y + ty).  Returns the cell's index in the
// outputs, row ny - 1 - cy (north to south), or -1 outside the grid.
__device__ __forceinline__ int64_t select_cell(int tiles_y, int nx, int ny, int& cx, int& cy) {
    const int tile = (int)blockIdx.x;
    const int tx = tile / tiles_y, ty = tile - tx * tiles_y;
    cx = tx * kSelTile + (int)(threadIdx.x % kSelTile);
    cy = ty * kSelTile + (int)(threadIdx.x / kSelTile);
    return cx >= nx || cy >= ny ? -1 : (int64_t)(ny - 1 - cy) * nx + cx;
}

// Calls f(m, acc, plane, cell) for every member m of select tile blockIdx.x whose window holds cell (cx, cy), in ascending
// order: acc the member's accumulators, plane the cells of one of its planes, cell the cell's index in a plane.
// MEMBER: {A (with .acc), W}.
template <typename MEMBER, typename F>
__device__ __forceinline__ void walk_tile_members(const MEMBER* __restrict__ members, const int* __restrict__ list_start,
                                                  const int* __restrict__ list, int cx, int cy, F f) {
    const int b = list_start[blockIdx.x], e = list_start[blockIdx.x + 1];
    for (int k = b; k < e; ++k) {
        const int m = list[k];
        const MEMBER& D = members[m];
        const int wx = cx - D.W.x0, wy = cy - D.W.y0;
        if (wx < 0 || wx >= D.W.nx || wy < 0 || wy >= D.W.ny) continue;
        f(m, D.A.acc, (int64_t)D.W.nx * D.W.ny, (int64_t)wx * D.W.ny + wy);
    }
}
#endif  // __HIPCC__

}  // namespace amt
