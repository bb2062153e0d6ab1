// The pure rule of the band roles (amt_prm::band_roles and amt_prm::band_role_counts of auromat_amd/csrc/amt_params.h) on every
// input with n <= 6 bands and each of the six other arguments in [-1, n + 1], against a band-by-band restatement.  No GPU, no
// HIP header.  Prints one summary line and exits 0, or names the first input that breaks a check and exits 1.
// With an argument (any) it checks a single input: whether the program runs at all as built.
#include <cstdio>
#include <cstdlib>

#include "amt_params.h"

using namespace amt_prm;

namespace {

long g_inputs = 0;

void fail(const char* what, int n, int t, int b, int ct, int cb, int i0, int i1, const band_role_ranges& r) {
    std::fprintf(stderr, "band_roles(n %d, t %d, b %d, can %d %d, in %d %d) -> inner [%d, %d) low_top_end %d low_bottom_begin %d: %s\n", n,
                 t, b, ct, cb, i0, i1, r.inner_begin, r.inner_end, r.low_top_end, r.low_bottom_begin, what);
    std::exit(1);
}

void check(int n, int t, int b, int ct, int cb, int i0, int i1) {
    ++g_inputs;
    const band_role_ranges r = band_roles(n, t, b, ct, cb, i0, i1);
#define CHECK(cond) \
    if (!(cond)) fail(#cond, n, t, b, ct, cb, i0, i1, r)
    // the Earth bands as the rule reads them
    const int tt = std::min(std::max(t, 0), n), bb = std::min(std::max(b, tt), n);
    const bool inner = r.inner_begin != 0 || r.inner_end != 0;
    CHECK(tt <= r.low_top_end && r.low_top_end <= r.low_bottom_begin && r.low_bottom_begin <= bb);
    if (inner) {
        CHECK(r.inner_begin < r.inner_end);
        CHECK(r.low_top_end <= r.inner_begin && r.inner_end <= r.low_bottom_begin);
    }
    // band by band: a low band lies outside [can_top, can_bottom), an inner band inside [in_begin, in_end), both among the
    // Earth bands; and the rule gives up nothing it could name: an Earth band outside [can_top, can_bottom) is low, one inside
    // it and inside [in_begin, in_end) is inner
    int want[3] = {0, 0, 0};
    for (int c = 0; c < n; ++c) {
        const bool earth = c >= tt && c < bb;
        const bool is_inner = inner && c >= r.inner_begin && c < r.inner_end;
        const bool is_low = earth && !is_inner && (c < r.low_top_end || c >= r.low_bottom_begin);
        if (is_inner) CHECK(earth && c >= i0 && c < i1);
        if (is_low) CHECK(c < ct || c >= cb);
        if (earth && ct <= cb && (c < ct || c >= cb)) CHECK(is_low);
        if (earth && ct <= cb && c >= ct && c < cb && c >= i0 && c < i1) CHECK(is_inner);
        if (earth) ++want[is_inner ? 1 : is_low ? 2 : 0];
    }
    int counts[3] = {-1, -1, -1};
    band_role_counts(r, tt, bb, counts);
    CHECK(counts[0] + counts[1] + counts[2] == bb - tt);
    CHECK(counts[0] == want[0] && counts[1] == want[1] && counts[2] == want[2]);
    if (t >= 0 && t <= b && b <= n) {                     // (what a frame's sky bands are: the same without the caller's clamp)
        band_role_counts(r, t, b, counts);
        CHECK(counts[0] == want[0] && counts[1] == want[1] && counts[2] == want[2]);
    }
    // whatever t and b: the counts sum to the bands between them as band_role_counts reads them
    band_role_counts(r, t, b, counts);
    CHECK(counts[0] + counts[1] + counts[2] == std::max(b, std::max(t, 0)) - std::max(t, 0));
#undef CHECK
}

}  // namespace

int main(int argc, char**) {
    if (argc > 1) {
        check(3, 0, 3, 1, 2, 1, 2);
        return 0;
    }
    for (int n = 0; n <= 6; ++n)
        for (int t = -1; t <= n + 1; ++t)
            for (int b = -1; b <= n + 1; ++b)
                for (int ct = -1; ct <= n + 1; ++ct)
                    for (int cb = -1; cb <= n + 1; ++cb)
                        for (int i0 = -1; i0 <= n + 1; ++i0)
                            for (int i1 = -1; i1 <= n + 1; ++i1) check(n, t, b, ct, cb, i0, i1);
    // no roles: every Earth band generic
    for (int n = 0; n <= 6; ++n) {
        const band_role_ranges r = band_roles_none(n);
        int counts[3];
        band_role_counts(r, 0, n, counts);
        if (counts[0] != n || counts[1] != 0 || counts[2] != 0) {
            std::fprintf(stderr, "band_roles_none(%d): counts %d %d %d\n", n, counts[0], counts[1], counts[2]);
            return 1;
        }
    }
    std::printf("band_roles: %ld inputs, 0 violations\n", g_inputs);
    return 0;
}
