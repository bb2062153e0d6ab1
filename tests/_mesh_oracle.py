"""
The contract of the mesh resampling (``amt_mesh_frame``, auromat_amd/csrc/amt_mesh.hip) in NumPy.  A plain helper
module for tests/test_mesh_cpu.py, tests/test_gpu_mesh_cells.py and tests/test_gpu_mesh.py.

Every function is the twin of a device function: ``orient`` / ``orient``, ``quad_split`` / ``quad_split``, ``edge_values`` /
``tri_edges``, ``candidate_ranges`` / ``candidate_cells``; the same operations in the same order, every one rounded on its own
(NumPy never contracts a product and a sum), so the claims, the winners and the values agree bit for bit.

A case is any object with: lat_c, lon_c (h, w) float64; elev (h, w) or None; mask (h, w) uint8 or None; min_elevation; img
(h * w, nch) uint8 | uint16; xedges, yedges (ascending); cell_lat (ny, north to south), cell_lon (nx); lon_wrap.
"""
import numpy as np

from _area_oracle import same_bits, wrap180_shifted  # noqa: F401  (same_bits: for the tests that compare)

NOBODY = 0xFFFFFFFF


def orient(px, py, qx, qy, rx, ry):
    """(Qx-Px)*(Ry-Py) - (Qy-Py)*(Rx-Px): two products, one difference."""
    a = (qx - px) * (ry - py)
    b = (qy - py) * (rx - px)
    return a - b


def vertices(case):
    """(ok, x, y), flat (h * w): which pixels are vertices, and where (0 for the others, as the kernel has it)."""
    h, w = case.lat_c.shape
    la = np.asarray(case.lat_c, dtype=np.float64).reshape(h * w)
    lo = np.asarray(case.lon_c, dtype=np.float64).reshape(h * w)
    ok = np.isfinite(la)
    if case.elev is not None and not (np.isinf(case.min_elevation) and case.min_elevation < 0):
        with np.errstate(invalid='ignore'):
            ok &= np.asarray(case.elev, dtype=np.float64).reshape(h * w) >= case.min_elevation
    if case.mask is not None:
        ok &= np.asarray(case.mask).reshape(h * w) == 0
    ok &= np.isfinite(lo)
    lo = np.where(ok, lo, 0.0)
    x = wrap180_shifted(lo) if case.lon_wrap else lo
    return ok, np.where(ok, x, 0.0), np.where(ok, la, 0.0)


def quad_vertices(h, w, q=None):
    """(n, 4) flat indices of A = (r, c), B = (r, c+1), C = (r+1, c+1), D = (r+1, c) of the quads q = r * (w - 1) + c (all of
    them for None)."""
    q = np.arange((h - 1) * (w - 1)) if q is None else np.asarray(q, dtype=np.int64)
    a = q // (w - 1) * w + q % (w - 1)
    return np.stack([a, a + 1, a + w + 1, a + w], axis=1)


def quads_near_a_centre(case, ok, x, y):
    """The quads with at least three vertices whose bounding box (of all four slots) holds a cell centre: no other quad has a
    triangle that holds one.  A shortcut for frames of millions of pixels on grids much coarser than the lattice; the answer
    does not depend on it (tests/test_mesh_cpu.py)."""
    h, w = case.lat_c.shape
    def four(v):
        v = v.reshape(h, w)
        return v[:-1, :-1], v[:-1, 1:], v[1:, 1:], v[1:, :-1]
    n = sum(v.astype(np.int8) for v in four(ok))
    def any_centre(v, centres):
        lo, hi = np.minimum.reduce(four(v)), np.maximum.reduce(four(v))
        return np.searchsorted(centres, hi, side='right') > np.searchsorted(centres, lo, side='left')
    near = (n >= 3) & any_centre(x, np.asarray(case.cell_lon)) & any_centre(y, np.asarray(case.cell_lat)[::-1])
    return np.flatnonzero(near.reshape(-1))


def same_side(a, b):
    return ((a > 0) & (b > 0)) | ((a < 0) & (b < 0))


def in_circle_det(X, Y):
    """The 3 x 3 in-circle determinant of A, B, C relative to D for quads X, Y (n, 4), in the kernel's order of operations."""
    adx, ady = X[:, 0] - X[:, 3], Y[:, 0] - Y[:, 3]
    bdx, bdy = X[:, 1] - X[:, 3], Y[:, 1] - Y[:, 3]
    cdx, cdy = X[:, 2] - X[:, 3], Y[:, 2] - Y[:, 3]
    ad2 = adx * adx + ady * ady
    bd2 = bdx * bdx + bdy * bdy
    cd2 = cdx * cdx + cdy * cdy
    m1 = bdy * cd2 - cdy * bd2
    m2 = bdx * cd2 - cdx * bd2
    m3 = bdx * cdy - bdy * cdx
    t1, t2, t3 = adx * m1, ady * m2, ad2 * m3
    return (t1 - t2) + t3


def quad_split(okq, X, Y):
    """(m0, m1) per quad: the slot (0 = A .. 3 = D) that triangle 2q and 2q + 1 leave out, -1 for no triangle.  Diagonal AC:
    (3, 1) = (A, B, C), (A, C, D); diagonal BD: (2, 0) = (A, B, D), (B, C, D); three valid vertices: the invalid one, -1.
    Also returns dict(ac, bd, inside) for the quads with four vertices (False elsewhere)."""
    n = okq.sum(axis=1)
    four = n == 4
    with np.errstate(over='ignore', invalid='ignore'):
        oabc = orient(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
        oacd = orient(X[:, 0], Y[:, 0], X[:, 2], Y[:, 2], X[:, 3], Y[:, 3])
        oabd = orient(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 3], Y[:, 3])
        obcd = orient(X[:, 1], Y[:, 1], X[:, 2], Y[:, 2], X[:, 3], Y[:, 3])
        det = in_circle_det(X, Y)
    ac, bd = same_side(oabc, oacd) & four, same_side(oabd, obcd) & four
    inside = np.where(oabc > 0, det > 0, det < 0) & four
    take_bd = np.where(ac & bd, inside, bd & ~ac)
    m0 = np.where(four, np.where(take_bd, 2, 3), np.where(n == 3, np.argmin(okq, axis=1), -1))
    m1 = np.where(four, np.where(take_bd, 0, 1), -1)
    return m0, m1, dict(ac=ac, bd=bd, inside=inside)


def triangles(case, quads=None, near_centres=False):
    """(ids (nt) int64 ascending, verts (nt, 3) flat indices in the triangle's own order): every triangle of the mesh — or of
    the quads given, or of quads_near_a_centre —, those as wide as the seam dropped."""
    h, w = case.lat_c.shape
    ok, x, y = vertices(case)
    if near_centres:
        quads = quads_near_a_centre(case, ok, x, y)
    quads = np.arange((h - 1) * (w - 1)) if quads is None else np.asarray(quads, dtype=np.int64)
    at = quad_vertices(h, w, quads)
    m0, m1, _ = quad_split(ok[at], x[at], y[at])
    ids, verts = [], []
    for k, m in ((0, m0), (1, m1)):
        q = np.flatnonzero(m >= 0)
        slots = np.arange(3)[None, :] + (np.arange(3)[None, :] >= m[q][:, None])
        ids.append(2 * quads[q] + k)
        verts.append(at[q][np.arange(len(q))[:, None], slots])
    ids, verts = np.concatenate(ids), np.concatenate(verts)
    order = np.argsort(ids)
    ids, verts = ids[order], verts[order]
    tx = x[verts]
    keep = tx.max(axis=1) - tx.min(axis=1) < 180.0
    return ids[keep], verts[keep]


def edge_values(verts, x, y, tx, ty):
    """(n, 3): e[:, k] of the edge opposite vertex k of triangles verts (n, 3) at the points tx, ty (n): evaluated with the
    edge's end points in ascending flat index, negated when the triangle runs the other way."""
    out = np.empty((len(verts), 3))
    for k, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
        va, vb = verts[:, a], verts[:, b]
        up = va < vb
        p, q = np.where(up, va, vb), np.where(up, vb, va)
        e = orient(x[p], y[p], x[q], y[q], tx, ty)
        out[:, k] = np.where(up, e, -e)
    return out


def holds(e):
    """All three >= 0 or all three <= 0, and not all zero."""
    pos, neg = (e >= 0).all(axis=1), (e <= 0).all(axis=1)
    return (pos | neg) & ~(pos & neg)


def candidate_ranges(X, Y, xedges, yedges):
    """(ix0, nxr, iy0, nyr) of triangles X, Y (n, 3): the cells whose rectangles their bounding boxes can meet (0 cells for one
    wholly outside the grid) — the rule of the area binning."""
    def axis(v, edges):
        n = len(edges) - 1
        lo = np.clip(np.searchsorted(edges, v.min(axis=1), side='right') - 1, 0, n - 1)
        hi = np.clip(np.searchsorted(edges, v.max(axis=1), side='right') - 1, 0, n - 1)
        outside = (v.max(axis=1) <= edges[0]) | (v.min(axis=1) >= edges[-1])
        return lo, np.where(outside, 0, hi - lo + 1)
    ix0, nxr = axis(X, xedges)
    iy0, nyr = axis(Y, yedges)
    nxr, nyr = np.where(nyr == 0, 0, nxr), np.where(nxr == 0, 0, nyr)
    return ix0, nxr, iy0, nyr


def pairs(case, every_cell=False):
    """Yields (ids (n), cell (n) = ix * ny + iy, e (n, 3)): every (triangle, candidate cell) pair of the claim pass with the
    edge values at the cell's centre, in slices.  `every_cell`: every triangle with every cell of the grid."""
    xedges, yedges = np.asarray(case.xedges, dtype=np.float64), np.asarray(case.yedges, dtype=np.float64)
    nx, ny = len(xedges) - 1, len(yedges) - 1
    _, x, y = vertices(case)
    ids, verts = triangles(case, near_centres=not every_cell)
    if every_cell:
        z = np.zeros(len(ids), dtype=np.int64)
        ix0, nxr, iy0, nyr = z, z + nx, z, z + ny
    else:
        ix0, nxr, iy0, nyr = candidate_ranges(x[verts], y[verts], xedges, yedges)
    counts = nxr * nyr
    # (in slices of the triangles, so that a fine grid does not need all pairs in memory at once)
    total = np.cumsum(counts)
    a = b = 0
    while b < len(ids):
        a, b = b, max(b + 1, int(np.searchsorted(total, (total[b - 1] if b else 0) + (1 << 22), side='right')))
        c = counts[a:b]
        if c.sum() == 0:
            continue
        tri = a + np.repeat(np.arange(b - a), c)
        k = np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c)
        ix, iy = ix0[tri] + k // np.maximum(nyr[tri], 1), iy0[tri] + k % np.maximum(nyr[tri], 1)
        e = edge_values(verts[tri], x, y, np.asarray(case.cell_lon)[ix], np.asarray(case.cell_lat)[ny - 1 - iy])
        yield ids[tri], ix * ny + iy, e


def claims(case, every_cell=False):
    """The claim words after k_mesh_claim: uint32 (nx, ny), NOBODY where no triangle holds the centre.  `every_cell`: every
    triangle is tried on every cell of the grid instead of on its candidates (the answer must not depend on it)."""
    ny, nx = len(case.yedges) - 1, len(case.xedges) - 1
    claim = np.full(nx * ny, NOBODY, dtype=np.int64)
    for ids, cell, e in pairs(case, every_cell):
        held = holds(e)
        np.minimum.at(claim, cell[held], ids[held])
    return claim.astype(np.uint32).reshape(nx, ny)


def strictly_inside(case):
    """bool (ny, nx), output layout: the cell's centre lies strictly inside a triangle of the mesh (all three edge values > 0
    or all three < 0)."""
    ny, nx = len(case.yedges) - 1, len(case.xedges) - 1
    inside = np.zeros(nx * ny, dtype=bool)
    for _, cell, e in pairs(case):
        inside[cell[(e > 0).all(axis=1) | (e < 0).all(axis=1)]] = True
    return np.flipud(inside.reshape(nx, ny).T)


def candidate_counts(case):
    """Candidate cells per triangle, as the kernel counts them."""
    _, x, y = vertices(case)
    _, verts = triangles(case)
    _, nxr, _, nyr = candidate_ranges(x[verts], y[verts], np.asarray(case.xedges, dtype=np.float64),
                                      np.asarray(case.yedges, dtype=np.float64))
    return nxr * nyr


def triangle_vertices(case, ids):
    """(n, 3) flat indices of the triangles `ids` in the triangle's own order, rebuilt from the ids as k_mesh_sample does (-1
    rows for an id that names no triangle of the mesh)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    h, w = case.lat_c.shape
    out = np.full((len(ids), 3), -1, dtype=np.int64)
    good = (ids >= 0) & (ids < 2 * (h - 1) * (w - 1))
    quads = np.unique(ids[good] >> 1)
    all_ids, verts = triangles(case, quads=quads)
    pos = np.minimum(np.searchsorted(all_ids, ids[good]), max(len(all_ids) - 1, 0))
    found = all_ids[pos] == ids[good] if len(all_ids) else np.zeros(good.sum(), dtype=bool)
    rows = np.flatnonzero(good)[found]
    out[rows] = verts[pos[found]]
    return out


def sample(case, claim):
    """The outputs of k_mesh_sample for claim words (nx, ny): dict(mesh (ny, nx, nch + 1), img (ny, nx, nch), mask (ny, nx) uint8,
    triangle (ny, nx) int32)."""
    nx, ny = claim.shape
    img = np.asarray(case.img)
    h, w = case.lat_c.shape
    img = img.reshape(h * w, -1) if img.size else np.zeros((h * w, 0), dtype=img.dtype)
    nch = img.shape[1]
    _, x, y = vertices(case)
    word = np.flipud(claim.T)                    # cell (ix, iy) -> row ny - 1 - iy, column ix
    won = word != NOBODY
    triangle = np.where(won, word.astype(np.int64), -1).astype(np.int32)
    mesh = np.full((ny, nx, nch + 1), np.nan)
    out_img = np.zeros((ny, nx, nch), dtype=img.dtype)
    r, c = np.nonzero(won)
    if len(r):
        verts = triangle_vertices(case, triangle[r, c])
        assert (verts >= 0).all(), 'a claim word names no triangle of the mesh'
        e = edge_values(verts, x, y, np.asarray(case.cell_lon)[c], np.asarray(case.cell_lat)[r])
        e = np.where((e < 0).any(axis=1)[:, None], -e, e)
        den = (e[:, 0] + e[:, 1]) + e[:, 2]
        chans = [img[:, k].astype(np.float64) for k in range(nch)]
        if case.elev is not None:
            chans.append(np.asarray(case.elev, dtype=np.float64).reshape(h * w))
        with np.errstate(invalid='ignore', divide='ignore'):
            for k, v in enumerate(chans):
                p0, p1, p2 = e[:, 0] * v[verts[:, 0]], e[:, 1] * v[verts[:, 1]], e[:, 2] * v[verts[:, 2]]
                val = ((p0 + p1) + p2) / den
                mesh[r, c, k] = val
                if k < nch:
                    out_img[r, c, k] = np.rint(val).astype(img.dtype)
    return dict(mesh=mesh, img=out_img, mask=(~won).astype(np.uint8), triangle=triangle)


def mesh_frame(case, every_cell=False):
    """The four outputs of ``amt_mesh_frame``."""
    return sample(case, claims(case, every_cell))
