// The host triangulator (csrc/amt_delaunay.hip is plain C++ for the host) from two host threads at once, under ThreadSanitizer ON
// THE CPU: a stand-alone program with its own main, never loaded into Python and never run on a GPU machine.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -DAMT_DELAUNAY_STANDALONE -o /tmp/tsan_delaunay \
//       tools/tsan_delaunay.cpp -x c++ auromat_amd/csrc/amt_delaunay.hip
//   /tmp/tsan_delaunay            (exit 0 and "ok": no report of the sanitizer, every result equal to the sequential one)
//
// (tests/test_threads_cpu.py runs the same two scenarios through ctypes, without a sanitizer.)
//
// Scenario 1, two handles: two amt_delaunay_create_threads builds at once on different point sets with threads = 3 (pools inside
// pools; the predicates' counters are thread_local pointers), their triangles against the same builds made one after the other.
// Scenario 2, one handle: amt_delaunay_triangles and amt_delaunay_vertex_neighbours of ONE handle that nobody has read yet from
// two threads at once — both take the lazy compaction behind the function-local static mutexes of ensure_compact /
// ensure_vertex_lists — against a handle compacted on one thread.
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../include/auromat_hip.h"

namespace {

std::vector<double> cloud(uint64_t seed, int64_t n, double sx, double sy) {
    std::vector<double> xy((size_t)(2 * n));
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (auto& v : xy) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        v = (double)(s >> 11) * (1.0 / 9007199254740992.0);
    }
    for (int64_t i = 0; i < n; ++i) xy[(size_t)(2 * i)] *= sx, xy[(size_t)(2 * i + 1)] *= sy;
    return xy;
}

struct lists {
    std::vector<int32_t> tri, nbr, indices;
    std::vector<int64_t> indptr;
    bool operator==(const lists& o) const { return tri == o.tri && nbr == o.nbr && indices == o.indices && indptr == o.indptr; }
};

constexpr int kThreads = 3;
constexpr int64_t kParallelMin = 300;

amt_delaunay* build(const std::vector<double>& xy) {
    amt_delaunay* d = nullptr;
    const int rc = amt_delaunay_create_threads(xy.data(), (int64_t)(xy.size() / 2), kThreads, kParallelMin, &d);
    return rc == 0 ? d : nullptr;
}

// room for any triangulation of n points: at most 2 n triangles, 6 n directed edges
void triangles_of(const amt_delaunay* d, int64_t n, lists* out) {
    out->tri.assign((size_t)(6 * n), -7), out->nbr.assign((size_t)(6 * n), -7);
    if (amt_delaunay_triangles(d, out->tri.data(), out->nbr.data()) != 0) out->tri.clear();
}

void neighbours_of(const amt_delaunay* d, int64_t n, lists* out) {
    out->indptr.assign((size_t)(n + 1), -7), out->indices.assign((size_t)(6 * n), -7);
    if (amt_delaunay_vertex_neighbours(d, out->indptr.data(), out->indices.data()) != 0) out->indptr.clear();
}

}  // namespace

int main() {
    const int64_t n[2] = {6000, 4500};
    const std::vector<double> pts[2] = {cloud(1, n[0], 1.0, 1.0), cloud(2, n[1], 30.0, 1.0)};
    int bad = 0;

    // the sequential answers
    lists want[2];
    for (int k = 0; k < 2; ++k) {
        amt_delaunay* d = build(pts[k]);
        if (d == nullptr) return 2;
        triangles_of(d, n[k], &want[k]);
        neighbours_of(d, n[k], &want[k]);
        int64_t info[2] = {0, 0};
        amt_delaunay_build_info(d, info);
        if (info[0] < 2) {
            std::printf("set %d was not built in strips (%lld): the parallel build is not exercised\n", k, (long long)info[0]);
            ++bad;
        }
        amt_delaunay_destroy(d);
    }

    // 1. two handles built at once
    {
        amt_delaunay* d[2] = {nullptr, nullptr};
        lists got[2];
        std::thread t0([&] { d[0] = build(pts[0]); if (d[0]) triangles_of(d[0], n[0], &got[0]), neighbours_of(d[0], n[0], &got[0]); });
        std::thread t1([&] { d[1] = build(pts[1]); if (d[1]) triangles_of(d[1], n[1], &got[1]), neighbours_of(d[1], n[1], &got[1]); });
        t0.join(), t1.join();
        for (int k = 0; k < 2; ++k) {
            if (d[k] == nullptr || !(got[k] == want[k])) {
                std::printf("two handles: set %d differs from its sequential build\n", k);
                ++bad;
            }
            if (d[k]) amt_delaunay_destroy(d[k]);
        }
    }

    // 2. one handle read by two threads before anybody has compacted it
    {
        amt_delaunay* d = build(pts[0]);
        if (d == nullptr) return 2;
        lists got;
        std::thread t0([&] { triangles_of(d, n[0], &got); });
        std::thread t1([&] { neighbours_of(d, n[0], &got); });
        t0.join(), t1.join();
        if (!(got == want[0])) {
            std::printf("one handle: the lists read by two threads differ from the sequential ones\n");
            ++bad;
        }
        amt_delaunay_destroy(d);
    }
    std::printf(bad ? "FAILED (%d)\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
