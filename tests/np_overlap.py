"""The reference of tests/test_overlap.py: art_overlap_boxes' semantics restated in numpy.

(a) brute_force   the semantics over every (box, triangle) pair in float32, operation by operation, on np_closest.world_triangles' fields: what the device must write
(b) witness       whether a triangle and a box share a point, in float64 and by another method: the triangle's polygon clipped against the box's six planes
                  (Sutherland-Hodgman); non-empty is an overlap.  Used with the box shrunk and grown by eps: (a) must say 1 where the shrunk box overlaps and 0 where
                  the grown one does not"""
import numpy as np

from np_closest import F, NOWHERE, world_triangles  # noqa: F401  (world_triangles: imported, not copied; re-exported for the tests)


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _axis_separates(p0, p1, p2, rad):
    """min and max by comparisons: a NaN separates nothing"""
    mn = np.where(p1 < p0, p1, p0); mx = np.where(p1 > p0, p1, p0)
    mn = np.where(p2 < mn, p2, mn); mx = np.where(p2 > mx, p2, mx)
    return (mn > rad) | (mx < -rad)


def tri_box_overlap(v0, e1, e2, lo, hi):
    """conditions 3 and 4 for float32 component triples of equal shape: the device's tri_box_overlap, operation by operation"""
    half = F(0.5)
    c = [half * lo[k] + half * hi[k] for k in range(3)]
    h = [half * hi[k] - half * lo[k] for k in range(3)]
    a0 = [v0[k] - c[k] for k in range(3)]
    a1 = [a0[k] + e1[k] for k in range(3)]
    a2 = [a0[k] + e2[k] for k in range(3)]
    n = _cross(e1, e2)
    sep = np.abs(_dot(n, a0)) > (h[0] * np.abs(n[0]) + h[1] * np.abs(n[1])) + h[2] * np.abs(n[2])
    for f in (e1, [e2[k] - e1[k] for k in range(3)], [-e2[k] for k in range(3)]):
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            p = [a[j] * f[i] - a[i] * f[j] for a in (a0, a1, a2)]
            sep = sep | _axis_separates(p[0], p[1], p[2], h[i] * np.abs(f[j]) + h[j] * np.abs(f[i]))
    return ~sep


def live(boxes):
    """[n] bool: a box with six finite coordinates and lo <= hi on every axis"""
    b = np.asarray(boxes, F).reshape(-1, 8)
    with np.errstate(all="ignore"):
        return np.isfinite(b[:, [0, 1, 2, 4, 5, 6]]).all(axis=1) & (b[:, 0:3] <= b[:, 4:7]).all(axis=1)


def pairs(T, boxes, vis=None, cull=0xFF, chunk=256):
    """(box index, gid) of every candidate pair, sorted by box and then gid; conditions 1 and 2 by comparison over every pair, 3 and 4 over the pairs those leave"""
    b = np.ascontiguousarray(boxes, F).reshape(-1, 8)
    n, nt = b.shape[0], T["v0"].shape[0]
    seen = np.ones(nt, bool) if vis is None else (np.asarray(vis)[T["prim"]] & cull) != 0
    if cull == 0:
        seen[:] = False
    ok = live(b)
    here = seen & (T["lo"][:, 0] < NOWHERE)
    bi, gi = [], []
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            lo, hi = b[a:a + chunk, None, 0:3], b[a:a + chunk, None, 4:7]
            meets = ((T["lo"][None] <= hi) & (lo <= T["hi"][None])).all(axis=2) & here[None] & ok[a:a + chunk, None]
            i, g = np.nonzero(meets)
            if not i.size:
                continue
            col = lambda x, at: [x[at, k] for k in range(3)]   # noqa: E731
            keep = tri_box_overlap(col(T["v0"], g), col(T["e1"], g), col(T["e2"], g), col(b[:, 0:3], i + a), col(b[:, 4:7], i + a))
            bi.append(i[keep] + a); gi.append(g[keep])
    if not bi:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(bi), np.concatenate(gi)


def brute_force(T, boxes, K=8, vis=None, cull=0xFF):
    """T: world_triangles(); boxes [n, 8] float32 (lo.xyz, -, hi.xyz, -); vis: the primitives' masks (None: all 0xFF).  -> hit [n] uint8, count [n] uint32 (every
    candidate), ids [n, K, 2] int32: the K candidates of smallest gid in ascending order, (-1, -1) behind them"""
    n = np.asarray(boxes).reshape(-1, 8).shape[0]
    bi, gi = pairs(T, boxes, vis, cull)
    count = np.bincount(bi, minlength=n).astype(np.uint32)
    ids = np.full((n, K, 2), -1, np.int32)
    first = np.concatenate([[0], np.cumsum(count.astype(np.int64))[:-1]])
    rank = np.arange(bi.size) - first[bi]          # (pairs are sorted by box, then gid)
    keep = rank < K
    ids[bi[keep], rank[keep], 0], ids[bi[keep], rank[keep], 1] = T["prim"][gi[keep]], T["tri"][gi[keep]]
    return (count > 0).astype(np.uint8), count, ids


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------------------
def witness(w, lo, hi):
    """[P] bool: does triangle w[p] ([P, 3, 3]) share a point with the closed box lo[p], hi[p] ([P, 3])?  float64; the polygon (at most 9 vertices) is clipped against
    each of the six half-spaces in turn, a vertex on a plane is inside.  An inverted box (lo > hi) shares nothing"""
    w, lo, hi = np.asarray(w, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    P = w.shape[0]
    poly = np.zeros((P, 10, 3)); poly[:, :3] = w
    cnt = np.full(P, 3)
    rows = np.arange(P)
    for axis in range(3):
        for sign, bound in ((1.0, lo[:, axis]), (-1.0, hi[:, axis])):
            d = sign * (poly[:, :, axis] - bound[:, None])   # >= 0: inside
            out, m = np.zeros_like(poly), np.zeros(P, np.int64)
            for i in range(9):
                nxt = np.where(i + 1 < cnt, i + 1, 0)
                da, db = d[:, i], d[rows, nxt]
                va, vb = poly[:, i], poly[rows, nxt]
                valid = i < cnt
                emit = valid & (da >= 0)
                out[rows[emit], m[emit]] = va[emit]; m[emit] += 1
                cross = valid & ((da >= 0) != (db >= 0))
                with np.errstate(all="ignore"):
                    t = da / (da - db)
                    x = va + t[:, None] * (vb - va)
                out[rows[cross], m[cross]] = x[cross]; m[cross] += 1
            poly, cnt = out, np.minimum(m, 9)
    return (cnt > 0) & (lo <= hi).all(axis=1)
