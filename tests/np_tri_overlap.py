"""The reference of tests/test_tri_overlap.py: art_overlap_triangles' semantics restated in numpy.

(a) brute_force   the semantics over every (query, triangle) pair in float32, operation by operation, on np_closest.world_triangles' fields: what the device must write.
                  tri_tri_overlap takes its precision from its operands: the same formulas on float64 arrays are the float64 evaluation the tests compare with
(b) witness       whether two triangles share a point, in float64 and by another method: an edge of either meets the other (closed Moeller-Trumbore), and for
                  coplanar pairs a test in the plane (an edge of one meets an edge of the other, or a vertex of one lies in the other).  Used with the query shrunk
                  and grown about its centroid: (a) must say 1 where the shrunk query meets the triangle and 0 where the grown one does not"""
import numpy as np

from np_closest import F, NOWHERE, world_triangles  # noqa: F401  (world_triangles: imported, not copied; re-exported for the tests)


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _min3(p0, p1, p2):
    """two selects from the first: a comparison with a NaN is false"""
    mn = np.where(p1 < p0, p1, p0)
    return np.where(p2 < mn, p2, mn)


def _max3(p0, p1, p2):
    mx = np.where(p1 > p0, p1, p0)
    return np.where(p2 > mx, p2, mx)


def _axis_separates(x, e1, e2, a0, a1, a2):
    """the scene triangle's projections 0, x.e1, x.e2 against the query's x.a0, x.a1, x.a2"""
    t1, t2, p0, p1, p2 = _dot(x, e1), _dot(x, e2), _dot(x, a0), _dot(x, a1), _dot(x, a2)
    zero = np.zeros_like(t1)
    return (_min3(zero, t1, t2) > _max3(p0, p1, p2)) | (_max3(zero, t1, t2) < _min3(p0, p1, p2))


def axes(v0, e1, e2, q0, q1, q2):
    """the 17 axes of condition 3 in their order, and the operands every projection takes: (axes, a0, a1, a2)"""
    a0, a1, a2 = _sub(q0, v0), _sub(q1, v0), _sub(q2, v0)
    f = (e1, _sub(e2, e1), [-e2[k] for k in range(3)])
    g = (_sub(a1, a0), _sub(a2, a1), _sub(a0, a2))
    n, m = _cross(e1, e2), _cross(g[0], g[1])
    return [n, m] + [_cross(f[i], g[j]) for i in range(3) for j in range(3)] + [_cross(n, f[i]) for i in range(3)] + [_cross(m, g[j]) for j in range(3)], a0, a1, a2


def tri_tri_overlap(v0, e1, e2, q0, q1, q2, skip=()):
    """condition 3 for component triples of equal shape, in the operands' precision: the device's tri_tri_overlap, operation by operation.  skip: axes left out (the
    tests' own use: what the six in-plane axes decide)"""
    ax, a0, a1, a2 = axes(v0, e1, e2, q0, q1, q2)
    sep = np.zeros(np.shape(a0[0]), bool)
    for k, x in enumerate(ax):
        if k not in skip:
            sep = sep | _axis_separates(x, e1, e2, a0, a1, a2)
    return ~sep


def live(tris):
    """[n] bool: a query with nine finite coordinates"""
    q = np.asarray(tris, F).reshape(-1, 12)
    return np.isfinite(q[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).all(axis=1)


def query_box(tris):
    """qlo, qhi [n, 3]: the componentwise minimum and maximum of the three vertices, by the selects"""
    q = np.asarray(tris, F).reshape(-1, 12)
    with np.errstate(all="ignore"):
        return _min3(q[:, 0:3], q[:, 4:7], q[:, 8:11]), _max3(q[:, 0:3], q[:, 4:7], q[:, 8:11])


def pairs(T, tris, vis=None, cull=0xFF, chunk=256, skip=()):
    """(query index, gid) of every candidate pair, sorted by query and then gid; conditions 1 and 2 by comparison over every pair, 3 over the pairs those leave"""
    q = np.ascontiguousarray(tris, F).reshape(-1, 12)
    n, nt = q.shape[0], T["v0"].shape[0]
    seen = np.ones(nt, bool) if vis is None else (np.asarray(vis)[T["prim"]] & cull) != 0
    if cull == 0:
        seen[:] = False
    ok = live(q)
    here = seen & (T["lo"][:, 0] < NOWHERE)
    qlo, qhi = query_box(q)
    qi, gi = [], []
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            lo, hi = qlo[a:a + chunk, None], qhi[a:a + chunk, None]
            meets = ((T["lo"][None] <= hi) & (lo <= T["hi"][None])).all(axis=2) & here[None] & ok[a:a + chunk, None]
            i, g = np.nonzero(meets)
            if not i.size:
                continue
            col = lambda x, at: [x[at, k] for k in range(3)]   # noqa: E731
            keep = tri_tri_overlap(col(T["v0"], g), col(T["e1"], g), col(T["e2"], g), col(q[:, 0:3], i + a), col(q[:, 4:7], i + a), col(q[:, 8:11], i + a), skip)
            qi.append(i[keep] + a); gi.append(g[keep])
    if not qi:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(qi), np.concatenate(gi)


def brute_force(T, q, K=8, vis=None, cull=0xFF):
    """T: world_triangles(); q [n, 12] float32 (q0.xyz, -, q1.xyz, -, q2.xyz, -); vis: the primitives' masks (None: all 0xFF).  -> hit [n] uint8, count [n] uint32
    (every candidate), ids [n, K, 2] int32: the K candidates of smallest gid in ascending order, (-1, -1) behind them"""
    n = np.asarray(q).reshape(-1, 12).shape[0]
    qi, gi = pairs(T, q, vis, cull)
    count = np.bincount(qi, minlength=n).astype(np.uint32)
    ids = np.full((n, K, 2), -1, np.int32)
    first = np.concatenate([[0], np.cumsum(count.astype(np.int64))[:-1]])
    rank = np.arange(qi.size) - first[qi]          # (pairs are sorted by query, then gid)
    keep = rank < K
    ids[qi[keep], rank[keep], 0], ids[qi[keep], rank[keep], 1] = T["prim"][gi[keep]], T["tri"][gi[keep]]
    return (count > 0).astype(np.uint8), count, ids


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _seg_meets_tri(p, d, a, e1, e2):
    """[P] bool: the closed segment {p + t d, 0 <= t <= 1} meets the closed triangle a, a + e1, a + e2 at a point where it crosses the plane (Moeller-Trumbore with every
    comparison closed).  A segment parallel to the plane is left to the coplanar branch"""
    h = np.cross(d, e2)
    det = np.einsum("pk,pk->p", e1, h)
    scale = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * np.linalg.norm(d, axis=1)
    ok = np.abs(det) > 1e-14 * scale
    inv = 1.0 / np.where(ok, det, 1.0)
    s = p - a
    u = np.einsum("pk,pk->p", s, h) * inv
    qv = np.cross(s, e1)
    v = np.einsum("pk,pk->p", d, qv) * inv
    t = np.einsum("pk,pk->p", e2, qv) * inv
    return ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def _orient(a, b, c):
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def _seg_meets_seg_2d(a, b, c, d):
    o1, o2, o3, o4 = _orient(a, b, c), _orient(a, b, d), _orient(c, d, a), _orient(c, d, b)
    cross = (o1 * o2 <= 0) & (o3 * o4 <= 0)
    line = (o1 == 0) & (o2 == 0) & (o3 == 0) & (o4 == 0)   # on one line: the intervals decide
    lo1, hi1, lo2, hi2 = np.minimum(a, b), np.maximum(a, b), np.minimum(c, d), np.maximum(c, d)
    return np.where(line, ((lo1 <= hi2) & (lo2 <= hi1)).all(axis=1), cross)


def _point_in_tri_2d(p, a, b, c):
    o1, o2, o3 = _orient(a, b, p), _orient(b, c, p), _orient(c, a, p)
    return ((o1 >= 0) & (o2 >= 0) & (o3 >= 0)) | ((o1 <= 0) & (o2 <= 0) & (o3 <= 0))


def witness(w, q):
    """[P] bool: does triangle w[p] ([P, 3, 3]) share a point with triangle q[p] ([P, 3, 3])?  float64.  Pairs in one plane (every vertex of q within 1e-9 of the pair's
    size of w's plane) are decided in that plane, the others by the six edge-against-face tests"""
    w, q = np.asarray(w, np.float64), np.asarray(q, np.float64)
    hit = np.zeros(w.shape[0], bool)
    for A, B in ((w, q), (q, w)):
        a, e1, e2 = A[:, 0], A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]
        for k in range(3):
            hit |= _seg_meets_tri(B[:, k], B[:, (k + 1) % 3] - B[:, k], a, e1, e2)
    n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
    nn = np.linalg.norm(n, axis=1)
    size = np.maximum(np.abs(w).max(axis=(1, 2)), np.abs(q).max(axis=(1, 2)))
    dist = np.abs(np.einsum("pvk,pk->pv", q - w[:, None, 0], n)) / np.where(nn > 0, nn, 1.0)[:, None]
    flat = np.flatnonzero((nn > 0) & (dist <= 1e-9 * size[:, None]).all(axis=1))
    if flat.size:
        drop = np.argmax(np.abs(n[flat]), axis=1)
        keep = np.array([[1, 2], [0, 2], [0, 1]])[drop]
        W, Q = np.take_along_axis(w[flat], keep[:, None, :], axis=2), np.take_along_axis(q[flat], keep[:, None, :], axis=2)
        h = np.zeros(flat.size, bool)
        for i in range(3):
            h |= _point_in_tri_2d(Q[:, i], W[:, 0], W[:, 1], W[:, 2]) | _point_in_tri_2d(W[:, i], Q[:, 0], Q[:, 1], Q[:, 2])
            for j in range(3):
                h |= _seg_meets_seg_2d(W[:, i], W[:, (i + 1) % 3], Q[:, j], Q[:, (j + 1) % 3])
        hit[flat] = h
    return hit
