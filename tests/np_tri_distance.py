"""The reference of tests/test_tri_distance.py: art_closest_triangles' semantics restated in numpy.

(a) brute_force   the semantics in float32, operation by operation, on np_closest.world_triangles' fields: what the device must write, bit for bit.  It runs over every
                  (query, triangle) pair whose box_d2 is finite and at most r * r -- leaving the others out is exact, since d2_eff >= box_d2.  tri_closest, the
                  clamped parameter and the 17 axes are np_closest's and np_tri_overlap's functions, imported and not copied.  `mutate` names one deliberate
                  error, for the tests that tell models apart
(b) witness       the true distance between two triangles in float64 by other means: Voronoi regions for the six vertex-triangle distances (np_closest.witness's
                  method), a float64 segment-segment distance for the nine edge pairs, and np_tri_overlap.witness for "they share a point" """
import numpy as np

import np_tri_overlap as nto
from np_closest import F, NOWHERE, _dot, tri_closest, world_triangles  # noqa: F401  (world_triangles: re-exported for the tests)

MUTATIONS = ("no edge pairs", "no scene vertices", "no overlap rule", "strict r")
GROUPS = ("query vertex", "scene vertex", "edge pair")


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _add(a, b):
    return [a[k] + b[k] for k in range(3)]


def _one(x):
    return x.dtype.type(1)


def _clamp01(x):
    """two selects: a NaN becomes 0"""
    x = np.where(x > 0, x, x.dtype.type(0))
    return np.where(x < 1, x, x.dtype.type(1))


def boxes_d2(qlo, qhi, tlo, thi):
    """the squared distance between [qlo, qhi] and [tlo, thi], component lists: per axis max(max(tlo - qhi, qlo - thi), 0) by selects, summed (x^2 + y^2) + z^2"""
    e = []
    for k in range(3):
        a, b = tlo[k] - qhi[k], qlo[k] - thi[k]
        m = np.where(b > a, b, a)
        e.append(np.where(m > 0, m, m.dtype.type(0)))
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def seg_seg(p1, d1, p2, d2):
    """the clamped segment pair of DESIGN.md 3.14 (Ericson 5.1.9): -> (squared distance, s, t)"""
    r = _sub(p1, p2)
    a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
    one, zero = _one(a), a.dtype.type(0)
    den = a * e - b * b
    qa = np.where(a > 0, a, one)
    s = _clamp01((b * f - c * e) / np.where(den > 0, den, one))
    s = np.where(den > 0, s, zero)
    s = np.where(a > 0, s, zero)
    t = (b * s + f) / np.where(e > 0, e, one)
    t = np.where(e > 0, t, zero)
    s0, s1 = _clamp01(-c / qa), _clamp01((b - c) / qa)
    s = np.where(t < 0, s0, s)
    s = np.where(t > 1, s1, s)
    s = np.where(a > 0, s, zero)
    t = _clamp01(t)
    d = [(p1[k] + s * d1[k]) - (p2[k] + t * d2[k]) for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], s, t


def features(v0, e1, e2, q0, q1, q2, mutate=None):
    """the fifteen features in their order, the first of the smallest winning: -> (d2, u, v, s, t, group) -- group 0 a query vertex, 1 a scene vertex, 2 an edge pair,
    -1 none gave a number"""
    dt = np.result_type(*v0)
    shape = np.broadcast(v0[0], q0[0]).shape
    z, o = np.zeros(shape, dt), np.ones(shape, dt)
    best = np.full(shape, np.inf, dt)
    u, v, s, t, grp = z, z, z, z, np.full(shape, -1, np.int8)

    def take(d, cu, cv, cs, ct, g):
        nonlocal best, u, v, s, t, grp
        w = d < best
        best, u, v, s, t, grp = np.where(w, d, best), np.where(w, cu, u), np.where(w, cv, v), np.where(w, cs, s), np.where(w, ct, t), np.where(w, np.int8(g), grp)
    g1, g2 = _sub(q1, q0), _sub(q2, q0)
    for qm, cs, ct in ((q0, z, z), (q1, o, z), (q2, z, o)):
        d, cu, cv, _ = tri_closest(_sub(qm, v0), e1, e2)
        take(d, cu, cv, cs, ct, 0)
    v1, v2 = _add(v0, e1), _add(v0, e2)
    if mutate != "no scene vertices":
        for vk, cu, cv in ((v0, z, z), (v1, o, z), (v2, z, o)):
            d, cs, ct, _ = tri_closest(_sub(vk, q0), g1, g2)
            take(d, cu, cv, cs, ct, 1)
    if mutate != "no edge pairs":
        sp, sd = (v0, v0, v1), (e1, e2, _sub(e2, e1))
        qp, qd = (q0, q0, _add(q0, g1)), (g1, g2, _sub(g2, g1))
        for i in range(3):
            for j in range(3):
                d, x, y = seg_seg(sp[i], sd[i], qp[j], qd[j])
                cu, cv = (x, z) if i == 0 else ((z, x) if i == 1 else (dt.type(1) - x, x))
                cs, ct = (y, z) if j == 0 else ((z, y) if j == 1 else (dt.type(1) - y, y))
                take(d, cu, cv, cs, ct, 2)
    return best, u, v, s, t, grp


def pair_d2(v0, e1, e2, q0, q1, q2, mutate=None):
    """d2_tri and the witnesses of float32 component triples of equal shape: -> (d2_tri, u, v, s, t, group, cut) -- cut: the 17 axes made it 0"""
    d, u, v, s, t, grp = features(v0, e1, e2, q0, q1, q2, mutate)
    cut = (d > 0) & (d < np.inf)
    if mutate == "no overlap rule":
        cut[...] = False
    if cut.any():
        at = np.nonzero(cut)
        pick = lambda x: [c[at] for c in x]   # noqa: E731
        cut[at] = nto.tri_tri_overlap(pick(v0), pick(e1), pick(e2), pick(q0), pick(q1), pick(q2))
    return np.where(cut, d.dtype.type(0), d), u, v, s, t, grp, cut


def live(tris):
    """[n] bool: nine finite coordinates, a radius that is no NaN and not below 0 (-0.0 is not)"""
    q = np.asarray(tris, F).reshape(-1, 12)
    with np.errstate(all="ignore"):
        return nto.live(q) & ~np.isnan(q[:, 3]) & ~(q[:, 3] < 0)


def brute_force(T, tris, vis=None, cull=0xFF, chunk=64, stats=False, mutate=None):
    """T: world_triangles(); tris [n, 12] float32 (q0.xyz, r, q1.xyz, -, q2.xyz, -); vis: the primitives' masks (None: all 0xFF).  -> duv [n, 4] float32, ids [n, 2]
    int32, point [n, 4], qpoint [n, 4] float32 as the device writes them.  stats: also a dict -- group [n] of the winner (-1: a miss), cut [n] the winner's distance is
    the overlap rule's 0, ties [n] candidates that share the minimum d2_eff, pairs: the pairs evaluated"""
    q = np.ascontiguousarray(tris, F).reshape(-1, 12)
    n, nt = q.shape[0], T["v0"].shape[0]
    duv, ids, point, qpoint = np.zeros((n, 4), F), np.full((n, 2), -1, np.int32), np.zeros((n, 4), F), np.zeros((n, 4), F)
    duv[:, 0] = q[:, 3]
    group, wcut, ties, npairs = np.full(n, -1, np.int8), np.zeros(n, bool), np.zeros(n, np.int64), 0
    seen = np.ones(nt, bool) if vis is None else (np.asarray(vis)[T["prim"]] & cull) != 0
    if cull == 0:
        seen[:] = False
    here = seen & (T["lo"][:, 0] < NOWHERE)
    ok = live(q)
    qlo, qhi = nto.query_box(q)
    col = lambda x, at: [x[at, k] for k in range(3)]   # noqa: E731
    with np.errstate(all="ignore"):
        r2 = q[:, 3] * q[:, 3]
        for a in range(0, n, chunk):
            sl = slice(a, a + chunk)
            bd = boxes_d2([qlo[sl, None, k] for k in range(3)], [qhi[sl, None, k] for k in range(3)], [T["lo"][None, :, k] for k in range(3)], [T["hi"][None, :, k] for k in range(3)]).astype(F)
            near = here[None] & ok[sl, None] & np.isfinite(bd) & (bd <= r2[sl, None])
            i, g = np.nonzero(near)
            if not i.size:
                continue
            i += a
            npairs += i.size
            dt, u, v, s, t, grp, cut = pair_d2(col(T["v0"], g), col(T["e1"], g), col(T["e2"], g), col(q[:, 0:3], i), col(q[:, 4:7], i), col(q[:, 8:11], i), mutate)
            b = bd[i - a, g]
            de = np.where(b > dt, b, dt).astype(F)
            cand = np.isfinite(dt) & ((de < r2[i]) if mutate == "strict r" else (de <= r2[i]))
            i, g, de, u, v, s, t, grp, cut = (x[cand] for x in (i, g, de, u, v, s, t, grp, cut))
            if not i.size:
                continue
            order = np.lexsort((g, de, i))                       # by query, then (d2_eff, gid)
            i, g, de, u, v, s, t, grp, cut = (x[order] for x in (i, g, de, u, v, s, t, grp, cut))
            first = np.flatnonzero(np.concatenate([[True], i[1:] != i[:-1]]))
            h, gh = i[first], g[first]
            ties[h] = np.add.reduceat((de == np.repeat(de[first], np.diff(np.append(first, i.size)))).astype(np.int64), first)
            bu, bv, bs, bt = u[first].astype(F), v[first].astype(F), s[first].astype(F), t[first].astype(F)
            duv[h, 0], duv[h, 1], duv[h, 2] = np.sqrt(de[first]), bu, bv
            ids[h, 0], ids[h, 1] = T["prim"][gh], T["tri"][gh]
            for k in range(3):
                point[h, k] = T["v0"][gh, k] + (bu * T["e1"][gh, k] + bv * T["e2"][gh, k])
                g1, g2 = q[h, 4 + k] - q[h, k], q[h, 8 + k] - q[h, k]
                qpoint[h, k] = q[h, k] + (bs * g1 + bt * g2)
            point[h, 3], qpoint[h, 3] = 1, 1
            group[h], wcut[h] = grp[first], cut[first]
    if stats:
        return duv, ids, point, qpoint, dict(group=group, cut=wcut, ties=ties, pairs=npairs)
    return duv, ids, point, qpoint


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _point_tri_64(p, a, b, c):
    """[P] float64: the distance from p to the triangle a b c by Ericson's Voronoi regions (5.1.5); a zero-area triangle falls into a vertex or an edge region"""
    dot = lambda x, y: (x * y).sum(-1)   # noqa: E731
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = va + vb + vc
        v, w = vb / den, vc / den
        e = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        for region, rv, rw in ((((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)), 1 - e, e), (((vb <= 0) & (d2 >= 0) & (d6 <= 0)), 0.0, d2 / (d2 - d6)), (((d6 >= 0) & (d5 <= d6)), 0.0, 1.0),
                               (((vc <= 0) & (d1 >= 0) & (d3 <= 0)), d1 / (d1 - d3), 0.0), (((d3 >= 0) & (d4 <= d3)), 1.0, 0.0), (((d1 <= 0) & (d2 <= 0)), 0.0, 0.0)):
            v, w = np.where(region, rv, v), np.where(region, rw, w)
        v, w = np.nan_to_num(v), np.nan_to_num(w)   # (a point triangle: 0 / 0 inside no region -- vertex a)
        pt = a + ab * v[..., None] + ac * w[..., None]
        return np.sqrt(dot(p - pt, p - pt))


def _seg_seg_64(p1, q1, p2, q2):
    """[P] float64: the distance between the segments p1 q1 and p2 q2 -- the smaller of the line-line distance where both feet fall inside, and the four end points
    against the other segment (a method of its own: no clamped re-solve)"""
    dot = lambda x, y: (x * y).sum(-1)   # noqa: E731

    def point_seg(p, a, b):
        ab = b - a
        den = dot(ab, ab)
        t = np.clip(dot(p - a, ab) / np.where(den > 0, den, 1.0), 0.0, 1.0)
        d = p - (a + ab * t[..., None])
        return np.sqrt(dot(d, d))
    best = np.minimum(np.minimum(point_seg(p1, p2, q2), point_seg(q1, p2, q2)), np.minimum(point_seg(p2, p1, q1), point_seg(q2, p1, q1)))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, f = dot(d1, d1), dot(d2, d2), dot(d1, d2), dot(d1, r), dot(d2, r)
    den = a * e - b * b
    with np.errstate(all="ignore"):
        ok = den > 1e-12 * a * e
        s = (b * f - c * e) / np.where(ok, den, 1.0)
        t = (a * f - b * c) / np.where(ok, den, 1.0)
        inside = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
        d = (p1 + d1 * s[..., None]) - (p2 + d2 * t[..., None])
        return np.where(inside, np.minimum(best, np.sqrt(dot(d, d))), best)


def witness(w, q):
    """[P] float64: the distance between triangle w[p] and triangle q[p] ([P, 3, 3] each): 0 where np_tri_overlap.witness says they share a point, else the smallest of
    the six vertex-triangle and the nine edge-edge distances"""
    w, q = np.asarray(w, np.float64), np.asarray(q, np.float64)
    best = np.full(w.shape[0], np.inf)
    for k in range(3):
        best = np.minimum(best, _point_tri_64(q[:, k], w[:, 0], w[:, 1], w[:, 2]))
        best = np.minimum(best, _point_tri_64(w[:, k], q[:, 0], q[:, 1], q[:, 2]))
    for i in range(3):
        for j in range(3):
            best = np.minimum(best, _seg_seg_64(w[:, i], w[:, (i + 1) % 3], q[:, j], q[:, (j + 1) % 3]))
    return np.where(nto.witness(w, q), 0.0, best)
