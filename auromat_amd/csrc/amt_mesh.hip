// Mesh resampling: linear interpolation on the pixel lattice.  The pixel centres of a frame form a smoothly deformed lattice,
// and that lattice carries a triangulation of its own: two triangles per quad of neighbouring centres.  Every cell of the
// output grid takes the value that is linear inside the lattice triangle holding the cell's centre (DESIGN.md §4.6 states the
// contract; tests/_mesh_oracle.py restates it in NumPy operation for operation).  No global triangulation, no host pass and
// no camera model: any frame with per-pixel centre arrays will do.  No counterpart in the reference: resample(method='linear')
// interpolates in scipy's Delaunay triangles of the same points, which on an oblique view join pixels that are no image
// neighbours.
//
// k_mesh_claim: one quad per lane.  The quad's triangles (quad_split: which diagonal, or the one triangle of a quad with three
// valid vertices) claim every cell whose centre they hold with a 32-bit atomicMin of the triangle id on the cell's claim word
// (0xFFFFFFFF: nobody), so the lowest id wins whatever the order.  Candidate cells come from the triangle's bounding box through
// bin_index, as in k_area_frame, and as there in two regimes: a lane walks a triangle of at most kLaneCells candidates itself;
// larger ones (a triangle near the limb on a fine grid covers thousands of cells) are collected by ballot and broadcast one at
// a time, and the wave's 64 lanes stride over their cells.  Both go through claim_cell -> tri_edges: the same bits.
//
// k_mesh_sample: one cell per lane.  It reads the winner, rebuilds its triangle from the id through the same quad_split and
// tri_edges — the only statement of the diagonal rule and of the edge values — and writes the outputs.
//
// No LDS privatisation, for the reasons at the top of amt_area.hip: the regime this pass exists for is the fine grid, where a
// (triangle, cell) pair is nearly unique (a cell centre lies in one triangle, two on a shared edge), so a window of LDS words
// would be flushed with one global atomic per LDS atomic.  A wave's claims go to neighbouring words of one or two grid columns
// (iy runs fastest).
#include "amt_common.h"
#include "amt_frame_src.h"

namespace {

using namespace amt;

constexpr int kMeshBlock = 256;
static_assert(kMeshBlock == kBlock, "grid_for counts workgroups of kBlock threads");
constexpr int kLaneCells = 16;                   // a triangle with more candidate cells is walked by the whole wave
constexpr unsigned int kNobody = 0xFFFFFFFFu;    // a claim word nobody has claimed

struct mesh_args {
    frame_src S;
    const void* img;
    int nch;
    const double* cell_lat;      // (ny) cell-centre latitudes, rows north to south: cell iy has cell_lat[ny - 1 - iy]
    const double* cell_lon;      // (nx)
    unsigned int* claim;         // nx * ny words, cell ix * ny + iy
};

// The four vertices of quad (r, c): A = (r, c), B = (r, c + 1), C = (r + 1, c + 1), D = (r + 1, c) in slots 0..3.
struct mesh_quad {
    double x[4], y[4];
    bool ok[4];
    int at[4];                   // flat lattice indices
};

// A triangle: three vertices of a quad in slot order, which is the order the contract lists them in.
struct mesh_tri {
    double x[3], y[3];
    int at[3];
};

// A vertex takes part when the frame's membership rule keeps its pixel and its longitude is finite.
__device__ __forceinline__ void load_quad(const frame_src& S, int r, int c, mesh_quad& Q) {
    const int i = r * S.width + c;
    Q.at[0] = i;
    Q.at[1] = i + 1;
    Q.at[2] = i + S.width + 1;
    Q.at[3] = i + S.width;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = Q.at[k];
        const double la = S.lat_c[p], lo = S.lon_c[p];
        const double ev = S.use_elev_threshold ? S.elev[p] : 0.0;
        Q.ok[k] = src_keeps(S, la, ev, S.mask ? S.mask[p] : 0u) && finite(lo);
        Q.x[k] = Q.ok[k] ? src_x(S, lo) : 0.0;
        Q.y[k] = Q.ok[k] ? la : 0.0;
    }
}

__device__ __forceinline__ double orient(double px, double py, double qx, double qy, double rx, double ry) {
#pragma clang fp contract(off)
    const double a = (qx - px) * (ry - py);
    const double b = (qy - py) * (rx - px);
    return a - b;
}

__device__ __forceinline__ bool same_side(double a, double b) { return (a > 0.0 && b > 0.0) || (a < 0.0 && b < 0.0); }

// THE diagonal rule.  A triangle of a quad is named by the slot it leaves out: diagonal AC gives (A, B, C) = without D and
// (A, C, D) = without B; diagonal BD gives (A, B, D) = without C and (B, C, D) = without A; a quad with exactly three valid
// vertices gives the one triangle without the invalid one.  m0, m1: the slot that triangle 2q and 2q + 1 leave out, -1: none.
__device__ __forceinline__ void quad_split(const mesh_quad& Q, int& m0, int& m1) {
#pragma clang fp contract(off)
    m0 = m1 = -1;
    const int n = (int)Q.ok[0] + (int)Q.ok[1] + (int)Q.ok[2] + (int)Q.ok[3];
    if (n < 3) return;
    if (n == 3) {
        m0 = !Q.ok[0] ? 0 : (!Q.ok[1] ? 1 : (!Q.ok[2] ? 2 : 3));
        return;
    }
    const double oabc = orient(Q.x[0], Q.y[0], Q.x[1], Q.y[1], Q.x[2], Q.y[2]);
    const double oacd = orient(Q.x[0], Q.y[0], Q.x[2], Q.y[2], Q.x[3], Q.y[3]);
    const double oabd = orient(Q.x[0], Q.y[0], Q.x[1], Q.y[1], Q.x[3], Q.y[3]);
    const double obcd = orient(Q.x[1], Q.y[1], Q.x[2], Q.y[2], Q.x[3], Q.y[3]);
    const bool ac = same_side(oabc, oacd), bd = same_side(oabd, obcd);
    bool take_bd = bd && !ac;
    if (ac && bd) {
        // D strictly inside the circle through A, B, C: the 3 x 3 in-circle determinant relative to D, with the sign of
        // orient(A, B, C)
        const double adx = Q.x[0] - Q.x[3], ady = Q.y[0] - Q.y[3];
        const double bdx = Q.x[1] - Q.x[3], bdy = Q.y[1] - Q.y[3];
        const double cdx = Q.x[2] - Q.x[3], cdy = Q.y[2] - Q.y[3];
        const double ad2 = adx * adx + ady * ady;
        const double bd2 = bdx * bdx + bdy * bdy;
        const double cd2 = cdx * cdx + cdy * cdy;
        const double m1_ = bdy * cd2 - cdy * bd2;
        const double m2_ = bdx * cd2 - cdx * bd2;
        const double m3_ = bdx * cdy - bdy * cdx;
        const double t1 = adx * m1_;
        const double t2 = ady * m2_;
        const double t3 = ad2 * m3_;
        const double det = (t1 - t2) + t3;
        take_bd = oabc > 0.0 ? det > 0.0 : det < 0.0;
    }
    m0 = take_bd ? 2 : 3;
    m1 = take_bd ? 0 : 1;
}

__device__ __forceinline__ double pick(const double (&a)[4], int s) { return s == 0 ? a[0] : (s == 1 ? a[1] : (s == 2 ? a[2] : a[3])); }
__device__ __forceinline__ int pick(const int (&a)[4], int s) { return s == 0 ? a[0] : (s == 1 ? a[1] : (s == 2 ? a[2] : a[3])); }

// The triangle of Q without slot m.  False for a triangle as wide as half the globe: it straddles the seam of the longitudes
// (the area kernel's rule).
__device__ __forceinline__ bool make_tri(const mesh_quad& Q, int m, mesh_tri& T) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int s = k + (k >= m ? 1 : 0);
        T.x[k] = pick(Q.x, s);
        T.y[k] = pick(Q.y, s);
        T.at[k] = pick(Q.at, s);
    }
    const double xmin = fmin(fmin(T.x[0], T.x[1]), T.x[2]), xmax = fmax(fmax(T.x[0], T.x[1]), T.x[2]);
    return xmax - xmin < 180.0;
}

// The edge function of (tx, ty) against the edge from vertex a to vertex b of T: always evaluated with the end points in
// ascending lattice index and negated when the triangle runs the other way, so the two triangles on a shared edge see the same
// number with opposite signs.
template <int a, int b>
__device__ __forceinline__ double edge_value(const mesh_tri& T, double tx, double ty) {
#pragma clang fp contract(off)
    const bool up = T.at[a] < T.at[b];
    const double px = up ? T.x[a] : T.x[b], py = up ? T.y[a] : T.y[b];
    const double qx = up ? T.x[b] : T.x[a], qy = up ? T.y[b] : T.y[a];
    const double e = orient(px, py, qx, qy, tx, ty);
    return up ? e : -e;
}

// THE edge values: e[k] belongs to the edge opposite vertex k.  True when T holds (tx, ty): all three >= 0 or all three <= 0
// (edges are closed), and not all three zero — which happens only on the line of a triangle without area, so such a triangle
// claims nothing.
__device__ __forceinline__ bool tri_edges(const mesh_tri& T, double tx, double ty, double (&e)[3]) {
    e[0] = edge_value<1, 2>(T, tx, ty);
    e[1] = edge_value<2, 0>(T, tx, ty);
    e[2] = edge_value<0, 1>(T, tx, ty);
    const bool pos = e[0] >= 0.0 && e[1] >= 0.0 && e[2] >= 0.0;
    const bool neg = e[0] <= 0.0 && e[1] <= 0.0 && e[2] <= 0.0;
    return (pos || neg) && !(pos && neg);
}

__device__ __forceinline__ void claim_cell(const mesh_args& A, const mesh_tri& T, unsigned int id, int ix, int iy) {
    const int ny = A.S.ay.nbin;
    double e[3];
    if (tri_edges(T, A.cell_lon[ix], A.cell_lat[ny - 1 - iy], e)) atomicMin(&A.claim[(int64_t)ix * ny + iy], id);
}

struct mesh_job {
    mesh_tri T;
    int ix0, iy0, nxr, nyr;          // candidate cells [ix0, ix0 + nxr) x [iy0, iy0 + nyr); nxr = 0: nothing to claim
};

// The candidate cells of T: those its bounding box meets, by the rule of k_area_frame.
__device__ __forceinline__ void candidate_cells(const frame_src& S, mesh_job& J) {
    const mesh_tri& T = J.T;
    const double xmin = fmin(fmin(T.x[0], T.x[1]), T.x[2]), xmax = fmax(fmax(T.x[0], T.x[1]), T.x[2]);
    const double ymin = fmin(fmin(T.y[0], T.y[1]), T.y[2]), ymax = fmax(fmax(T.y[0], T.y[1]), T.y[2]);
    if (!(xmax > S.ax.e0 && xmin < S.ax.e_last && ymax > S.ay.e0 && ymin < S.ay.e_last)) return;
    const int nbx = S.ax.nbin, nby = S.ay.nbin;
    const int ix0 = min(max(bin_index(S.ax, xmin) - 1, 0), nbx - 1);
    const int ix1 = min(max(bin_index(S.ax, xmax) - 1, 0), nbx - 1);
    const int iy0 = min(max(bin_index(S.ay, ymin) - 1, 0), nby - 1);
    const int iy1 = min(max(bin_index(S.ay, ymax) - 1, 0), nby - 1);
    J.ix0 = ix0;
    J.iy0 = iy0;
    J.nxr = ix1 - ix0 + 1;
    J.nyr = iy1 - iy0 + 1;
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_claim(mesh_args A) {
    const frame_src& S = A.S;
    const int qw = S.width - 1;
    const int64_t nquad = (int64_t)(S.height - 1) * qw;
    const int lane = threadIdx.x & 63;
    // (whole waves run every iteration: the cooperative part below needs all 64 lanes)
    const int64_t per_sweep = (int64_t)gridDim.x * kMeshBlock;
    for (int64_t base = (int64_t)blockIdx.x * kMeshBlock + (threadIdx.x & ~63); base < nquad; base += per_sweep) {
        const int64_t q = base + lane;
        mesh_quad Q;
        int m[2] = {-1, -1};
        if (q < nquad) {
            const int r = (int)(q / qw), c = (int)(q - (int64_t)r * qw);
            load_quad(S, r, c, Q);
            quad_split(Q, m[0], m[1]);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            mesh_job J;
            J.ix0 = J.iy0 = J.nxr = J.nyr = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                J.T.x[i] = J.T.y[i] = 0.0;
                J.T.at[i] = 0;
            }
            if (m[k] >= 0 && make_tri(Q, m[k], J.T)) candidate_cells(S, J);
            const unsigned int id = (unsigned int)(2 * q + k);
            const long long ncells = (long long)J.nxr * J.nyr;
            const bool wide = ncells > kLaneCells;
            if (!wide)
                for (int jx = 0; jx < J.nxr; ++jx)
                    for (int jy = 0; jy < J.nyr; ++jy) claim_cell(A, J.T, id, J.ix0 + jx, J.iy0 + jy);
            // the wide triangles of this wave, one at a time over all 64 lanes
            unsigned long long todo = __ballot(wide);
            while (todo) {
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1;
                mesh_job W;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    W.T.x[i] = __shfl(J.T.x[i], src);
                    W.T.y[i] = __shfl(J.T.y[i], src);
                    W.T.at[i] = __shfl(J.T.at[i], src);
                }
                W.ix0 = __shfl(J.ix0, src);
                W.iy0 = __shfl(J.iy0, src);
                W.nxr = __shfl(J.nxr, src);
                W.nyr = __shfl(J.nyr, src);
                const unsigned int wid = (unsigned int)(2 * (base + src) + k);
                // lane l takes cells l, l + 64, ... of the range in the order jx * nyr + jy; the step of 64 cells is split into
                // whole columns and a rest once per triangle, so that no cell costs a division
                const int step_x = 64 / W.nyr, step_y = 64 - step_x * W.nyr;
                int jx = lane / W.nyr, jy = lane - jx * W.nyr;
                while (jx < W.nxr) {
                    claim_cell(A, W.T, wid, W.ix0 + jx, W.iy0 + jy);
                    jx += step_x;
                    jy += step_y;
                    if (jy >= W.nyr) {
                        jy -= W.nyr;
                        jx += 1;
                    }
                }
            }
        }
    }
}

// One cell per lane, in output order (row r north to south, column c: cell ix = c, iy = ny - 1 - r).
template <typename IMG_T>
__global__ __launch_bounds__(kMeshBlock) void k_mesh_sample(mesh_args A, double* __restrict__ mesh, IMG_T* __restrict__ out_img,
                                                            uint8_t* __restrict__ out_mask, int32_t* __restrict__ out_triangle) {
#pragma clang fp contract(off)
    const frame_src& S = A.S;
    const int nx = S.ax.nbin, ny = S.ay.nbin, nch = A.nch;
    const int qw = S.width - 1;
    const int64_t n = (int64_t)nx * ny;
    const IMG_T* img = static_cast<const IMG_T*>(A.img);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / nx), c = (int)(i - (int64_t)r * nx);
        const unsigned int id = A.claim[(int64_t)c * ny + (ny - 1 - r)];
        const bool won = id != kNobody;
        double e[3] = {0.0, 0.0, 0.0};
        mesh_tri T;
        if (won) {
            const int q = (int)(id >> 1);
            const int qr = q / qw, qc = q - qr * qw;
            mesh_quad Q;
            load_quad(S, qr, qc, Q);
            int m0, m1;
            quad_split(Q, m0, m1);
            make_tri(Q, (id & 1u) ? m1 : m0, T);
            tri_edges(T, A.cell_lon[c], A.cell_lat[r], e);
            // one common sign
            if (e[0] < 0.0 || e[1] < 0.0 || e[2] < 0.0) {
                e[0] = -e[0];
                e[1] = -e[1];
                e[2] = -e[2];
            }
        }
        const double den = (e[0] + e[1]) + e[2];
        for (int k = 0; k <= nch; ++k) {
            double v = NAN;
            if (won && (k < nch || S.elev != nullptr)) {
                double v0, v1, v2;
                if (k < nch) {
                    v0 = (double)img[(int64_t)T.at[0] * nch + k];
                    v1 = (double)img[(int64_t)T.at[1] * nch + k];
                    v2 = (double)img[(int64_t)T.at[2] * nch + k];
                } else {
                    v0 = S.elev[T.at[0]];
                    v1 = S.elev[T.at[1]];
                    v2 = S.elev[T.at[2]];
                }
                const double p0 = e[0] * v0, p1 = e[1] * v1, p2 = e[2] * v2;
                const double num = (p0 + p1) + p2;
                v = num / den;
            }
            if (mesh) mesh[i * (nch + 1) + k] = v;
            if (k < nch && out_img) out_img[i * nch + k] = won ? (IMG_T)rint(v) : (IMG_T)0;
        }
        if (out_mask) out_mask[i] = won ? 0 : 1;
        if (out_triangle) out_triangle[i] = won ? (int32_t)id : -1;
    }
}

}  // namespace

extern "C" {

int amt_mesh_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                   int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                   double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, const double* cell_lat,
                   const double* cell_lon, double* mesh, void* out_img, uint8_t* out_mask, int32_t* out_triangle, uint32_t* claim) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, cell_lat && cell_lon && claim, "NULL argument");
    AMT_REQUIRE(ctx, mesh || out_img || out_mask || out_triangle, "no output");
    mesh_args A;
    const char* bad = make_frame_src(&A.S, lat_c, lon_c, elev, center_mask, height, width, min_elevation, xaxis, yaxis, lon_wrap, 0);
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    AMT_REQUIRE(ctx, height >= 2 && width >= 2, "a lattice of at least 2 x 2 centres");
    AMT_REQUIRE(ctx, (int64_t)height * width < ((int64_t)1 << 31) && 2 * (int64_t)(height - 1) * (width - 1) < ((int64_t)1 << 31),
                "triangle ids below 2^31");
    AMT_REQUIRE(ctx, nchan >= 0 && nchan <= 4, "nchan must be 0..4");
    AMT_REQUIRE(ctx, (nchan == 0 && out_img == nullptr) || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    AMT_REQUIRE(ctx, nchan == 0 || img != nullptr, "NULL argument");
    AMT_REQUIRE(ctx, xaxis->nbin < 65535 && yaxis->nbin < 65535, "at most 65534 bins per axis");
    if (amt_set_device(ctx)) return AMT_EHIP;
    const int nx = xaxis->nbin, ny = yaxis->nbin;
    // the claim words: the caller's memory, set to "nobody" by every call, whatever it held
    const size_t claim_bytes = (size_t)nx * (size_t)ny * sizeof(unsigned int);
    AMT_HIP(ctx, hipMemsetAsync(claim, 0xFF, claim_bytes, ctx->stream));
    A.img = img;
    A.nch = nchan;
    A.cell_lat = cell_lat;
    A.cell_lon = cell_lon;
    A.claim = claim;
    const dim3 block(kMeshBlock);
    hipLaunchKernelGGL(k_mesh_claim, grid_for((int64_t)(height - 1) * (width - 1)), block, 0, ctx->stream, A);
    AMT_LAUNCH_CHECK(ctx);
    const dim3 sgrid = grid_for((int64_t)nx * ny);
    if (img_dtype == 2)
        hipLaunchKernelGGL(k_mesh_sample<uint16_t>, sgrid, block, 0, ctx->stream, A, mesh, static_cast<uint16_t*>(out_img), out_mask,
                           out_triangle);
    else
        hipLaunchKernelGGL(k_mesh_sample<uint8_t>, sgrid, block, 0, ctx->stream, A, mesh, static_cast<uint8_t*>(out_img), out_mask,
                           out_triangle);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

}  // extern "C"
