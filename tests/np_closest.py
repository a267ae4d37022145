"""The reference of tests/test_closest_points.py: art_closest_points' semantics restated in numpy.

(a) world_triangles   the world vertices of every triangle in gid order, with xform_point's operation order in float32, and from them the DevTri fields
(b) brute_force       the semantics over every (query, triangle) pair in float32, operation by operation: what the device must write, ids and bits
(c) witness           the true distance in float64 from the same float32 inputs, written independently of (b) (Ericson's region walk, not (b)'s face-then-edges)"""
import numpy as np

F = np.float32
NOWHERE = F(3.0e38)


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------------------------
def world_triangles(primitives, disabled=()):
    """dict of float32 arrays over all triangles in gid order (the running index over the primitives in add order): w [T, 3, 3] world vertices, v0, e1, e2, lo, hi
    [T, 3] (the DevTri fields: one subtraction each, min / max of the three vertices), prim, tri [T].  A primitive in `disabled` (out of the built structure by
    residency) has the record the refit writes: a point nowhere"""
    ws, prim, tri, out = [], [], [], []
    for p, P in enumerate(primitives):
        v = np.asarray(P.verts, F)[:, 0:3]
        idx = np.asarray(P.indices).reshape(-1, 3).astype(np.int64)
        m = np.asarray(P.model, F).reshape(3, 4)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        wv = np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], 1).astype(F)
        ws.append(wv[idx])
        prim.append(np.full(idx.shape[0], p, np.int32)); tri.append(np.arange(idx.shape[0], dtype=np.int32)); out.append(np.full(idx.shape[0], p in disabled))
    w = np.concatenate(ws).astype(F)
    prim, tri, out = np.concatenate(prim), np.concatenate(tri), np.concatenate(out)
    v0, e1, e2 = w[:, 0].copy(), w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]
    lo, hi = np.minimum(np.minimum(w[:, 0], w[:, 1]), w[:, 2]), np.maximum(np.maximum(w[:, 0], w[:, 1]), w[:, 2])
    v0[out], e1[out], e2[out], lo[out], hi[out] = NOWHERE, 0, 0, NOWHERE, NOWHERE
    return dict(w=w, v0=v0, e1=e1, e2=e2, lo=lo, hi=hi, prim=prim, tri=tri)


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _uv_d2(w, e1, e2, u, v):
    d = [w[k] - (u * e1[k] + v * e2[k]) for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _seg(w, e):
    den = _dot(e, e)
    s = _dot(w, e) / np.where(den > 0, den, F(1))
    s = np.where(den > 0, s, F(0))
    s = np.where(s > 0, s, F(0))
    return np.where(s < 1, s, F(1)).astype(F)


def tri_closest(w, e1, e2):
    """d2_tri, u, v, feature (0 face, 1..3 the edges v0v1, v0v2, v1v2, -1 none) for broadcastable float32 component triples: the device's tri_closest, operation by operation"""
    n = _cross(e1, e2)
    nn = _dot(n, n)
    den = np.where(nn > 0, nn, F(1))
    fu, fv = _dot(_cross(w, e2), n) / den, _dot(_cross(e1, w), n) / den
    inside = (nn > 0) & (fu >= 0) & (fv >= 0) & (fu + fv <= 1)
    shape = np.broadcast(fu, w[0]).shape
    best, u, v, feat = np.full(shape, np.inf, F), np.zeros(shape, F), np.zeros(shape, F), np.full(shape, -1, np.int8)
    zero = np.zeros(shape, F)

    def take(ok, d, cu, cv, f):
        nonlocal best, u, v, feat
        t = ok & (d < best)
        best, u, v, feat = np.where(t, d, best), np.where(t, cu, u), np.where(t, cv, v), np.where(t, np.int8(f), feat)
    take(inside, _uv_d2(w, e1, e2, fu, fv), fu, fv, 0)
    sa = _seg(w, e1)
    take(True, _uv_d2(w, e1, e2, sa, zero), sa + zero, zero, 1)
    sb = _seg(w, e2)
    take(True, _uv_d2(w, e1, e2, zero, sb), zero, sb + zero, 2)
    sc = _seg([w[k] - e1[k] for k in range(3)], [e2[k] - e1[k] for k in range(3)])
    uc = F(1) - sc
    take(True, _uv_d2(w, e1, e2, uc, sc), uc + zero, sc + zero, 3)
    return best.astype(F), u.astype(F), v.astype(F), feat


def box_d2(p, lo, hi):
    e = [np.fmax(np.fmax(lo[k] - p[k], p[k] - hi[k]), F(0)) for k in range(3)]   # (fmax: fmaxf's rule for a NaN operand)
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def brute_force(T, queries, vis=None, cull=0xFF, chunk=256, stats=False):
    """T: world_triangles(); queries [n, 4] float32 (p.xyz, r); vis: the primitives' masks (None: all 0xFF).  -> duv [n, 4] float32, ids [n, 2] int32, point [n, 4]
    float32 as the device writes them.  stats: also a dict -- feature [n] of the winning candidate (-1: a miss), ties [n] candidates that share the minimum d2_eff, d2 [n] the winner's d2_eff (inf: a miss),
    raised: pairs where box_d2 > d2_tri among finite ones"""
    q = np.ascontiguousarray(queries, F).reshape(-1, 4)
    n, nt = q.shape[0], T["v0"].shape[0]
    duv, ids, point = np.zeros((n, 4), F), np.full((n, 2), -1, np.int32), np.zeros((n, 4), F)
    duv[:, 0] = q[:, 3]
    feature, ties, raised, best = np.full(n, -1, np.int8), np.zeros(n, np.int64), 0, np.full(n, np.inf, F)
    seen = np.ones(nt, bool) if vis is None else (np.asarray(vis)[T["prim"]] & cull) != 0
    if cull == 0:
        seen[:] = False
    col = lambda a: [a[None, :, k] for k in range(3)]   # noqa: E731
    v0, e1, e2, lo, hi = col(T["v0"]), col(T["e1"]), col(T["e2"]), col(T["lo"]), col(T["hi"])
    with np.errstate(all="ignore"):
        live = np.isfinite(q[:, 0:3]).all(axis=1) & ~np.isnan(q[:, 3]) & ~(q[:, 3] < 0)
        for a in range(0, n, chunk):
            at = np.flatnonzero(live[a:a + chunk]) + a
            if not at.size:
                continue
            p = [q[at, k][:, None] for k in range(3)]
            dt, u, v, feat = tri_closest([p[k] - v0[k] for k in range(3)], e1, e2)
            bd = box_d2(p, lo, hi).astype(F)
            fin = np.isfinite(dt) & np.isfinite(bd)
            raised += int((fin & (bd > dt)).sum())
            de = np.maximum(dt, bd)
            r2 = (q[at, 3] * q[at, 3])[:, None]
            cand = seen[None, :] & fin & (de <= r2)
            key = np.where(cand, de, F(np.inf))
            g = np.argmin(key, axis=1)          # the first of the smallest: the smallest gid
            rows = np.arange(at.size)
            hit = cand[rows, g]
            ties[at] = np.where(hit, (cand & (key == key[rows, g][:, None])).sum(axis=1), 0)
            h, gh, rh = at[hit], g[hit], rows[hit]
            bu, bv = u[rh, gh], v[rh, gh]
            duv[h, 0], duv[h, 1], duv[h, 2] = np.sqrt(de[rh, gh]), bu, bv
            ids[h, 0], ids[h, 1] = T["prim"][gh], T["tri"][gh]
            for k in range(3):
                point[h, k] = T["v0"][gh, k] + (bu * T["e1"][gh, k] + bv * T["e2"][gh, k])
            point[h, 3] = 1
            feature[h], best[h] = feat[rh, gh], de[rh, gh]
    if stats:
        return duv, ids, point, dict(feature=feature, ties=ties, raised=raised, d2=best)
    return duv, ids, point


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------------------------------
def witness(T, queries, chunk=256):
    """the true distance [n] (float64) from each query point to the nearest of the triangles T["w"], radius ignored: Ericson's Voronoi-region test (Real-Time
    Collision Detection 5.1.5) on the float32 world vertices, in float64"""
    q = np.asarray(queries, np.float64).reshape(-1, 4)[:, None, 0:3]
    A, B, Cc = (np.asarray(T["w"][:, k], np.float64)[None] for k in range(3))
    out = np.zeros(q.shape[0])
    dot = lambda a, b: (a * b).sum(-1)   # noqa: E731
    with np.errstate(all="ignore"):
        for s in range(0, q.shape[0], chunk):
            P = q[s:s + chunk]
            ab, ac, ap = B - A, Cc - A, P - A
            d1, d2 = dot(ab, ap), dot(ac, ap)
            bp = P - B
            d3, d4 = dot(ab, bp), dot(ac, bp)
            cp = P - Cc
            d5, d6 = dot(ab, cp), dot(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            den = va + vb + vc
            v, w = vb / den, vc / den                                                     # inside the face: barycentrics of B and C
            e = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            for region, rv, rw in ((((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)), 1 - e, e),      # edge BC   (the later a region, the higher its rank)
                                   (((vb <= 0) & (d2 >= 0) & (d6 <= 0)), 0.0, d2 / (d2 - d6)),     # edge AC
                                   (((d6 >= 0) & (d5 <= d6)), 0.0, 1.0),                           # vertex C
                                   (((vc <= 0) & (d1 >= 0) & (d3 <= 0)), d1 / (d1 - d3), 0.0),     # edge AB
                                   (((d3 >= 0) & (d4 <= d3)), 1.0, 0.0),                           # vertex B
                                   (((d1 <= 0) & (d2 <= 0)), 0.0, 0.0)):                           # vertex A
                v, w = np.where(region, rv, v), np.where(region, rw, w)
            pt = A + ab * v[..., None] + ac * w[..., None]
            d = np.sqrt(dot(P - pt, P - pt))
            out[s:s + chunk] = np.nanmin(d, axis=1)
    return out
