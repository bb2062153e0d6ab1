// The host plan of the mosaics (auromat_amd/csrc/amt_mosaic_plan.h, its host part alone) against a brute-force restatement —
// every select tile x every member — on constructed window sets, and the workspace packer's offsets.  No GPU, no HIP header.
// Prints one line per case and exits 0, or names the first failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "amt_mosaic_plan.h"

using namespace amt;

namespace {

struct member {                         // the fields of amt_mosaic_member / amt_area_mosaic_member that the plan reads
    const double* lat_c;
    const double* elev;
    const void* img;
    int32_t height, width;
    int32_t win_x0, win_y0, win_nx, win_ny;
};

const double kSome = 0.0;

member make(int x0, int y0, int nx, int ny, int h = 3, int w = 5) { return member{&kSome, &kSome, &kSome, h, w, x0, y0, nx, ny}; }

std::string g_case;

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            std::fprintf(stderr, "%s: %s (line %d)\n", g_case.c_str(), #cond, __LINE__);     \
            std::exit(1);                                                                      \
        }                                                                                      \
    } while (0)

int64_t units_of(const member& m) { return (int64_t)m.height * m.width + 1; }     // any count the caller likes

void check_plan(const char* name, const std::vector<member>& ms, int nx, int ny, int nchan) {
    g_case = name;
    const int n = (int)ms.size();
    mosaic_plan P;
    CHECK(plan_members(P, ms.data(), n, nx, ny, nchan, units_of));
    plan_select_lists(P);
    CHECK(mosaic_members_bad(ms.data(), n, 1, nchan, true, nx, ny, [](const member&) -> const char* { return nullptr; }) ==
          nullptr);

    // windows: the empty rule; the prefix: the running sum of the caller's counts over the members that have a window
    CHECK((int)P.win.size() == n && (int)P.unit_start.size() == n + 1 && (int)P.acc_off.size() == n);
    int64_t units = 0;
    size_t words = 0;
    std::vector<char> owner;
    for (int i = 0; i < n; ++i) {
        const member& m = ms[(size_t)i];
        const cell_window w = P.win[(size_t)i];
        const bool empty = m.win_nx == 0 || m.win_ny == 0;
        CHECK(w.x0 == m.win_x0 && w.y0 == m.win_y0);
        CHECK(empty ? (w.nx == 0 && w.ny == 0) : (w.nx == m.win_nx && w.ny == m.win_ny));
        CHECK(P.unit_start[(size_t)i] == units);
        if (empty) continue;
        units += units_of(m);
        // the accumulators: (nchan + 2) planes of the window, disjoint, no gaps
        const size_t len = (size_t)(nchan + 2) * (size_t)w.nx * (size_t)w.ny;
        CHECK(P.acc_off[(size_t)i] == words);
        words += len;
    }
    CHECK(P.unit_start[(size_t)n] == units && P.units == units);
    CHECK(P.acc_words == words);
    owner.assign(P.acc_words, 0);
    for (int i = 0; i < n; ++i) {
        const cell_window w = P.win[(size_t)i];
        if (w.nx == 0) continue;
        const size_t len = (size_t)(nchan + 2) * (size_t)w.nx * (size_t)w.ny;
        CHECK(P.acc_off[(size_t)i] + len <= P.acc_words);
        for (size_t k = 0; k < len; ++k) {
            CHECK(owner[P.acc_off[(size_t)i] + k] == 0);
            owner[P.acc_off[(size_t)i] + k] = 1;
        }
    }
    for (char c : owner) CHECK(c == 1);

    // the select tiles: tile tx * sty + ty holds, ascending, exactly the members with a cell inside it
    CHECK(P.stx == (nx + kSelTile - 1) / kSelTile && P.sty == (ny + kSelTile - 1) / kSelTile);
    CHECK(P.list_start.size() == (size_t)P.stx * P.sty + 1 && P.list_start[0] == 0);
    CHECK(P.list_start.back() == (int)P.list.size());
    size_t longest = 0, without = 0;
    for (int tx = 0; tx < P.stx; ++tx)
        for (int ty = 0; ty < P.sty; ++ty) {
            std::vector<int> brute;
            for (int i = 0; i < n; ++i) {
                const member& m = ms[(size_t)i];
                bool meets = false;
                for (int x = m.win_x0; x < m.win_x0 + m.win_nx && !meets; ++x)
                    for (int y = m.win_y0; y < m.win_y0 + m.win_ny && !meets; ++y)
                        meets = x / kSelTile == tx && y / kSelTile == ty;
                if (meets) brute.push_back(i);
            }
            const size_t t = (size_t)tx * P.sty + ty;
            CHECK(P.list_start[t] <= P.list_start[t + 1]);
            const std::vector<int> got(P.list.begin() + P.list_start[t], P.list.begin() + P.list_start[t + 1]);
            for (size_t k = 1; k < got.size(); ++k) CHECK(got[k - 1] < got[k]);
            CHECK(got == brute);
            longest = got.size() > longest ? got.size() : longest;
            without += got.empty();
        }
    std::printf("%s: %d members, %d x %d tiles, %lld units, %zu words, longest list %zu, %zu empty lists\n", name, n, P.stx,
                P.sty, (long long)P.units, P.acc_words, longest, without);
}

// the three workspace layouts: 256-aligned, in the stated order, no overlap, the uploaded segments one staging buffer
void check_packer() {
    g_case = "packer";
    struct seg { size_t at, bytes; bool uploaded; };
    const long sizes[][6] = {{1000, 12, 44, 4, 8, -1},              // mean: tables x 4 | acc | (no tail)
                             {1000, 12, 44, 4, 8, 77},              //                        | tail
                             {256, 512, 300, 4000, 256, 0},         // area: tables x 4 | flag (256) | acc (none)
                             {7, 1, 1, 0, 1, 1}};                   // an uploaded segment without bytes keeps 4
    for (const auto& s : sizes) {
        workspace_packer K;
        std::vector<seg> segs;
        std::vector<char> src(4096, 0);         // what the uploaded segments are copied from, written after upload()
        for (int k = 0; k < 6; ++k) {
            if (s[k] < 0) continue;
            const bool up = k < 4;
            const size_t at = up ? K.upload(src.data(), (size_t)s[k]) : K.add((size_t)s[k]);
            segs.push_back({at, up && s[k] == 0 ? 4 : (size_t)s[k], up});
        }
        size_t end = 0;
        for (const seg& g : segs) {
            CHECK(g.at % 256 == 0 && g.at >= end && g.at - end < 256);
            end = g.at + g.bytes;
        }
        CHECK(K.total() == end);
        // the staging buffer: from the first uploaded segment to the 256-aligned end of the last
        src[0] = 7;                             // (host() reads the sources when it is called)
        const std::vector<char> host = K.host();
        CHECK(segs[0].at == 0 && host.size() == segs[4].at);
        for (int k = 0; k < 4; ++k) {
            CHECK(host[segs[(size_t)k].at] == (s[k] ? 7 : 0));
            if (s[k] > 1) CHECK(host[segs[(size_t)k].at + 1] == 0);
        }
    }
    // the ordered mosaics: plane | table | prefix (uploaded from the table on) | median workspace
    workspace_packer K;
    int v = 0;
    std::vector<char> tab(3 * 56, 5);
    const size_t plane = K.add(37 * 21 * 4), table = K.upload(tab.data(), tab.size()), prefix = K.upload(&v, sizeof(v)),
                 med = K.add(12345);
    CHECK(plane == 0 && table == 3328 && prefix == 3584 && med == 3840 && K.total() == 3840 + 12345);
    v = 0x01020304;
    const std::vector<char> host = K.host();
    CHECK(host.size() == med - table && host[0] == 5 && host[tab.size() - 1] == 5 && host[tab.size()] == 0);
    int back = 0;
    std::memcpy(&back, host.data() + (prefix - table), sizeof(back));
    CHECK(back == v);
    std::printf("packer: ok\n");
}

// what the shared member check refuses, by its message
void check_refusals() {
    g_case = "refusals";
    auto none = [](const member&) -> const char* { return nullptr; };
    auto says = [&](const std::vector<member>& ms, int rule, int nchan, bool axes, int nx, int ny, const char* text) {
        const char* bad = mosaic_members_bad(ms.data(), (int32_t)ms.size(), rule, nchan, axes, nx, ny, none);
        return bad != nullptr && std::string(bad) == text;
    };
    const std::vector<member> one = {make(0, 0, 5, 3)};
    CHECK(says({}, 0, 0, true, 5, 3, "no members"));
    CHECK(says(one, 2, 0, true, 5, 3, "rule must be 0 (union) or 1 (highest elevation)"));
    CHECK(says(one, 0, 5, true, 5, 3, "nchan must be 0..4"));
    CHECK(says(one, 0, 0, false, 5, 3, "bad axis"));
    CHECK(says(one, 0, 0, true, 65535, 3, "at most 65534 bins per axis"));
    std::vector<member> ms = one;
    ms[0].lat_c = nullptr;
    CHECK(says(ms, 0, 0, true, 5, 3, "member without centres"));
    ms = one, ms[0].img = nullptr;
    CHECK(says(ms, 0, 1, true, 5, 3, "member image missing") && !says(ms, 0, 0, true, 5, 3, "member image missing"));
    ms = one, ms[0].elev = nullptr;
    CHECK(says(ms, 1, 0, true, 5, 3, "rule 1 needs every member's elevation"));
    CHECK(mosaic_members_bad(ms.data(), 1, 0, 0, true, 5, 3, none) == nullptr);
    ms = one, ms[0].win_nx = -1;
    CHECK(says(ms, 0, 0, true, 5, 3, "bad window"));
    CHECK(says({make(1, 0, 5, 3)}, 0, 0, true, 5, 3, "window outside the grid"));
    CHECK(says({make(0, -1, 5, 3)}, 0, 0, true, 5, 3, "window outside the grid"));
    // an empty window may lie anywhere
    CHECK(mosaic_members_bad(std::vector<member>{make(99, -7, 0, 3)}.data(), 1, 0, 0, true, 5, 3, none) == nullptr);
    // the entry point's own check of a member comes first
    const char* own = mosaic_members_bad(ms.data(), 1, 0, 0, true, 5, 3, [](const member&) -> const char* { return "own"; });
    CHECK(own != nullptr && std::string(own) == "own");
    std::printf("refusals: ok\n");
}

}  // namespace

int main() {
    // one member covering a grid smaller than one select tile
    check_plan("small_grid", {make(0, 0, 5, 3)}, 5, 3, 1);

    // 37 x 21 cells: windows that end exactly on a tile border (x0 + nx == 16, == 32), start exactly on one, one cell wide
    check_plan("tile_borders",
               {make(3, 2, 13, 5), make(10, 0, 22, 16), make(16, 16, 21, 5), make(32, 3, 5, 18), make(15, 15, 1, 1),
                make(16, 0, 1, 21), make(0, 16, 37, 1), make(31, 15, 2, 2)},
               37, 21, 3);

    // three members, the middle one empty: as win_nx == 0 and as win_ny == 0
    check_plan("middle_empty_nx", {make(0, 0, 20, 20), make(7, 9, 0, 4), make(12, 12, 25, 9)}, 37, 21, 0);
    check_plan("middle_empty_ny", {make(0, 0, 20, 20), make(7, 9, 4, 0), make(12, 12, 25, 9)}, 37, 21, 4);

    // 65 members of one to four cells scattered over 64 x 48 cells: long lists in some tiles, none in others
    std::vector<member> many;
    unsigned s = 12345;
    auto next = [&](unsigned mod) { s = s * 1103515245u + 12345u; return (int)((s >> 16) % mod); };
    for (int i = 0; i < 65; ++i) {
        const int nx = 1 + next(2), ny = 1 + next(2);
        // two thirds of them crowd the tiles around (16, 16), tile corners included; the rest lie in the grid's western half
        const int x0 = i % 3 ? 14 + next(4) : next(32 - nx), y0 = i % 3 ? 14 + next(4) : next(48 - ny);
        many.push_back(make(x0, y0, nx, ny, 1 + next(4), 1 + next(4)));
    }
    check_plan("many_65", many, 64, 48, 2);

    // all members empty
    {
        const std::vector<member> none = {make(0, 0, 0, 0), make(5, 5, 0, 7), make(1, 2, 3, 0)};
        check_plan("all_empty", none, 37, 21, 1);
        mosaic_plan P;
        CHECK(plan_members(P, none.data(), 3, 37, 21, 1, units_of));
        plan_select_lists(P);
        CHECK(P.units == 0 && P.acc_words == 0 && P.list.empty());
    }

    // the unit prefix is kept in 31 bits
    {
        g_case = "too_many_units";
        const std::vector<member> big = {make(0, 0, 1, 1), make(0, 0, 1, 1)};
        mosaic_plan P;
        CHECK(!plan_members(P, big.data(), 2, 5, 3, 0, [](const member&) { return (int64_t)1 << 30; }));
    }

    check_packer();
    check_refusals();
    return 0;
}
