"""The reference of tests/test_tri_cast.py: art_cast_triangles' semantics restated in numpy.

(a) brute_force   the semantics in float32, operation by operation, on np_closest.world_triangles' fields: what the device must write, bit for bit.  The shifted-box slab
                  is evaluated for every (query, triangle) pair and the sixteen features for the pairs that pass it, which is the semantics' own condition for a
                  candidate.  The 17 axes are np_tri_overlap's, S's witnesses np_tri_distance.features, the slab's fma np_sweep's (one rounding, by round-to-odd in
                  float64): imported, not copied.  `mutate` names one deliberate error, for the tests that tell models apart
(b) witness       the first contact time of two translating triangles in float64 by other means: Moeller-Trumbore for a vertex against a face, a 3 x 3 linear solve for
                  a pair of edges, np_tri_overlap.witness for "they share a point at tmin".  touch_distance is np_tri_distance.witness on a posed query"""
import numpy as np

import np_tri_distance as ntd
import np_tri_overlap as nto
from np_closest import F, NOWHERE, _cross, _dot, world_triangles  # noqa: F401  (world_triangles: re-exported for the tests)
from np_sweep import _fma

MUTATIONS = ("no edge pairs", "no scene vertices", "no start")
FEATURES = ("S", "QV0", "QV1", "QV2", "SV0", "SV1", "SV2", "E00", "E01", "E02", "E10", "E11", "E12", "E20", "E21", "E22")
COORDS = [0, 1, 2, 4, 5, 6, 8, 9, 10]


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _add(a, b):
    return [a[k] + b[k] for k in range(3)]


def pose(q0, q1, q2, d, t):
    """the query's vertices at time t: one product and one sum a component"""
    return tuple([qm[k] + t * d[k] for k in range(3)] for qm in (q0, q1, q2))


def _vertex_face(w0, d, e1, e2, n, nn, nd):
    """the ray (w0, d) against the face (0, e1, e2) with normal n: -> t, fu, fv, taken"""
    one = nn.dtype.type(1)
    t = -_dot(n, w0) / np.where(nd != 0, nd, one)
    w = [w0[k] + t * d[k] for k in range(3)]
    den = np.where(nn > 0, nn, one)
    fu, fv = _dot(_cross(w, e2), n) / den, _dot(_cross(e1, w), n) / den
    return t, fu, fv, (nn > 0) & (nd != 0) & (fu >= 0) & (fv >= 0) & (fu + fv <= 1)


def pair_cast(v0, e1, e2, q0, q1, q2, d, tmin, tmax, mutate=None):
    """t_tri and the witnesses for component triples of equal shape, in the operands' precision: -> (t_tri, u, v, s, t, feature) -- feature an index into FEATURES, -1 none"""
    dt = np.result_type(*v0)
    shape = np.shape(v0[0])
    z, o = np.zeros(shape, dt), np.ones(shape, dt)
    best = np.full(shape, np.inf, dt)
    u, v, s, tt, feat = z, z, z, z, np.full(shape, -1, np.int8)

    def take(ok, t, cu, cv, cs, ct, f):
        nonlocal best, u, v, s, tt, feat
        k = ok & (t >= tmin) & (t < tmax) & (t < best)
        best, u, v, s, tt, feat = np.where(k, t, best), np.where(k, cu, u), np.where(k, cv, v), np.where(k, cs, s), np.where(k, ct, tt), np.where(k, np.int8(f), feat)
    g1, g2 = _sub(q1, q0), _sub(q2, q0)
    if mutate != "no start":
        p0, p1, p2 = pose(q0, q1, q2, d, tmin)
        start = nto.tri_tri_overlap(v0, e1, e2, p0, p1, p2) & (tmin >= tmin) & (tmin < tmax)
        if start.any():
            at = np.nonzero(start)
            pick = lambda x: [c[at] for c in x]   # noqa: E731
            _, su, sv, ss, st, _ = ntd.features(pick(v0), pick(e1), pick(e2), pick(p0), pick(p1), pick(p2))
            wu, wv, ws, wt = z.copy(), z.copy(), z.copy(), z.copy()
            wu[at], wv[at], ws[at], wt[at] = su, sv, ss, st
            take(start, tmin + z, wu, wv, ws, wt, 0)
    n = _cross(e1, e2)
    nn, nd = _dot(n, n), _dot(n, d)
    for i, (qm, cs, ct) in enumerate(((q0, z, z), (q1, o, z), (q2, z, o))):
        t, fu, fv, ok = _vertex_face(_sub(qm, v0), d, e1, e2, n, nn, nd)
        take(ok, t, fu, fv, cs, ct, 1 + i)
    v1, v2 = _add(v0, e1), _add(v0, e2)
    if mutate != "no scene vertices":
        n = _cross(g1, g2)
        back = [-d[k] for k in range(3)]
        nn, nd = _dot(n, n), _dot(n, back)
        for j, (vk, cu, cv) in enumerate(((v0, z, z), (v1, o, z), (v2, z, o))):
            t, fu, fv, ok = _vertex_face(_sub(vk, q0), back, g1, g2, n, nn, nd)
            take(ok, t, cu, cv, fu, fv, 4 + j)
    if mutate != "no edge pairs":
        sp, sd = (v0, v0, v1), (e1, e2, _sub(e2, e1))
        qp, qd = (q0, q0, _add(q0, g1)), (g1, g2, _sub(g2, g1))
        one = dt.type(1)
        for i in range(3):
            for j in range(3):
                n, r0 = _cross(sd[i], qd[j]), _sub(sp[i], qp[j])
                nn, nd = _dot(n, n), _dot(n, d)
                den = np.where(nn > 0, nn, one)
                t = _dot(n, r0) / np.where(nd != 0, nd, one)
                m = [r0[k] - t * d[k] for k in range(3)]
                se, sq = -_dot(_cross(m, qd[j]), n) / den, -_dot(_cross(m, sd[i]), n) / den
                ok = (nn > 0) & (nd != 0) & (se >= 0) & (se <= 1) & (sq >= 0) & (sq <= 1)
                cu, cv = (se, z) if i == 0 else ((z, se) if i == 1 else (one - se, se))
                cs, ct = (sq, z) if j == 0 else ((z, sq) if j == 1 else (one - sq, sq))
                take(ok, t, cu, cv, cs, ct, 7 + 3 * i + j)
    return best, u, v, s, tt, feat


def live(sweeps):
    """[n] bool: nine finite coordinates, a finite d, a tmax that is no NaN"""
    q = np.asarray(sweeps, F).reshape(-1, 16)
    return np.isfinite(q[:, COORDS]).all(axis=1) & np.isfinite(q[:, 12:15]).all(axis=1) & ~np.isnan(q[:, 7])


def shifted_slab(qlo, qhi, tlo, thi, d, tmin, tlimit):
    """1.1's slab of the ray (0, d) against [tlo - qhi, thi - qlo], broadcastable [.., 3] float32 arrays: -> tn, passed"""
    safe = np.where(np.abs(d) < F(1e-20), np.copysign(F(1e-20), d), d).astype(F)
    inv = (F(1) / safe).astype(F)
    ood = (F(0) * inv).astype(F)
    lo, hi = (tlo - qhi).astype(F), (thi - qlo).astype(F)
    inv, ood = np.broadcast_to(inv, lo.shape), np.broadcast_to(ood, lo.shape)
    t0, t1 = _fma(lo, inv, -ood, F), _fma(hi, inv, -ood, F)
    tn, tf = np.fmax.reduce(np.fmin(t0, t1), axis=-1), np.fmin.reduce(np.fmax(t0, t1), axis=-1)
    return tn, np.fmax(tn, tmin) <= np.fmin(tf, tlimit)


def brute_force(T, sweeps, vis=None, cull=0xFF, chunk=64, stats=False, mutate=None):
    """T: world_triangles(); sweeps [n, 16] float32 (q0.xyz, tmin | q1.xyz, tmax | q2.xyz, - | d.xyz, -); vis: the primitives' masks (None: all 0xFF).  -> tuv [n, 4]
    float32, ids [n, 2] int32, point [n, 4], qpoint [n, 4] float32 as the device writes them.  stats: also a dict -- feature [n] of the winner (-1: a miss), ties [n]
    candidates that share the minimum t_eff, raised: candidates whose box is entered after t_tri, pairs: the pairs evaluated"""
    q = np.ascontiguousarray(sweeps, F).reshape(-1, 16)
    n, nt = q.shape[0], T["v0"].shape[0]
    tuv, ids, point, qpoint = np.zeros((n, 4), F), np.full((n, 2), -1, np.int32), np.zeros((n, 4), F), np.zeros((n, 4), F)
    tuv[:, 0] = q[:, 7]
    feature, ties, raised, npairs = np.full(n, -1, np.int8), np.zeros(n, np.int64), 0, 0
    seen = np.ones(nt, bool) if vis is None else (np.asarray(vis)[T["prim"]] & cull) != 0
    if cull == 0:
        seen[:] = False
    here = seen & (T["lo"][:, 0] < NOWHERE)
    ok = live(q)
    qlo, qhi = nto.query_box(q[:, 0:12])
    col = lambda x, at: [x[at, k] for k in range(3)]   # noqa: E731
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            sl = slice(a, a + chunk)
            tn, passed = shifted_slab(qlo[sl, None], qhi[sl, None], T["lo"][None], T["hi"][None], q[sl, None, 12:15], q[sl, None, 3], q[sl, None, 7])
            i, g = np.nonzero(passed & here[None] & ok[sl, None])
            if not i.size:
                continue
            tn = tn[i, g]
            i += a
            npairs += i.size
            tt, u, v, s, t, feat = pair_cast(col(T["v0"], g), col(T["e1"], g), col(T["e2"], g), col(q[:, 0:3], i), col(q[:, 4:7], i), col(q[:, 8:11], i), col(q[:, 12:15], i),
                                             q[i, 3], q[i, 7], mutate)
            cand = tt < np.inf
            raised += int((cand & (tn > tt)).sum())
            te = np.fmax(tt, tn).astype(F)
            i, g, te, u, v, s, t, feat = (x[cand] for x in (i, g, te, u, v, s, t, feat))
            if not i.size:
                continue
            order = np.lexsort((g, te, i))                       # by query, then (t_eff, gid)
            i, g, te, u, v, s, t, feat = (x[order] for x in (i, g, te, u, v, s, t, feat))
            first = np.flatnonzero(np.concatenate([[True], i[1:] != i[:-1]]))
            h, gh = i[first], g[first]
            ties[h] = np.add.reduceat((te == np.repeat(te[first], np.diff(np.append(first, i.size)))).astype(np.int64), first)
            bu, bv, bs, bt = u[first].astype(F), v[first].astype(F), s[first].astype(F), t[first].astype(F)
            tuv[h, 0], tuv[h, 1], tuv[h, 2] = te[first], bu, bv
            ids[h, 0], ids[h, 1] = T["prim"][gh], T["tri"][gh]
            for k in range(3):
                point[h, k] = T["v0"][gh, k] + (bu * T["e1"][gh, k] + bv * T["e2"][gh, k])
                g1, g2 = q[h, 4 + k] - q[h, k], q[h, 8 + k] - q[h, k]
                qpoint[h, k] = q[h, k] + (bs * g1 + bt * g2)
            point[h, 3], qpoint[h, 3] = 1, 1
            feature[h] = feat[first]
    if stats:
        return tuv, ids, point, qpoint, dict(feature=feature, ties=ties, raised=raised, pairs=npairs)
    return tuv, ids, point, qpoint


def sweeps_of(tris, d, tmin=0.0, tmax=1.0):
    """[n, 16] float32 queries from triangles [n, 3, 3], displacements [n, 3] (or one) and the limits"""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    q = np.zeros((tris.shape[0], 16), F)
    q[:, 0:3], q[:, 4:7], q[:, 8:11] = tris[:, 0], tris[:, 1], tris[:, 2]
    q[:, 12:15] = np.asarray(d, F)
    q[:, 3], q[:, 7] = tmin, tmax
    return q


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _ray_tri_64(p, d, a, e1, e2):
    """[P] float64: the t at which the line {p + t d} meets the closed triangle a, a + e1, a + e2 (Moeller-Trumbore, every comparison closed); inf where it does not, or
    runs in the plane"""
    h = np.cross(d, e2)
    det = np.einsum("pk,pk->p", e1, h)
    ok = det != 0
    inv = 1.0 / np.where(ok, det, 1.0)
    s = p - a
    u = np.einsum("pk,pk->p", s, h) * inv
    qv = np.cross(s, e1)
    v = np.einsum("pk,pk->p", d, qv) * inv
    t = np.einsum("pk,pk->p", e2, qv) * inv
    return np.where(ok & (u >= 0) & (v >= 0) & (u + v <= 1), t, np.inf)


def _edge_edge_64(a, e, b, g, d):
    """[P] float64: the t at which the segment {b + t d + sq g} meets the segment {a + se e}: the 3 x 3 system [d, g, -e] (t, sq, se) = a - b; inf where the matrix is
    singular or a parameter leaves [0, 1]"""
    M = np.stack([d, g, -e], axis=2)
    det = np.linalg.det(M)
    ok = det != 0
    M = np.where(ok[:, None, None], M, np.eye(3)[None])
    x = np.linalg.solve(M, (a - b)[:, :, None])[:, :, 0]
    return np.where(ok & (x[:, 1] >= 0) & (x[:, 1] <= 1) & (x[:, 2] >= 0) & (x[:, 2] <= 1), x[:, 0], np.inf)


def witness(w, q, d, tmin, tmax):
    """[P] float64: the first t in [tmin, tmax) at which the triangle q[p] + t d[p] touches the triangle w[p] ([P, 3, 3] each, d [P, 3], the limits [P]); inf: none"""
    w, q, d = np.asarray(w, np.float64), np.asarray(q, np.float64), np.asarray(d, np.float64)
    tmin, tmax = np.broadcast_to(np.asarray(tmin, np.float64), w.shape[:1]), np.broadcast_to(np.asarray(tmax, np.float64), w.shape[:1])
    best = np.full(w.shape[0], np.inf)
    with np.errstate(all="ignore"):
        def take(t):
            nonlocal best
            best = np.where((t >= tmin) & (t < tmax) & (t < best), t, best)
        take(np.where(nto.witness(w, q + (tmin[:, None] * d)[:, None, :]), tmin, np.inf))
        for k in range(3):
            take(_ray_tri_64(q[:, k], d, w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]))
            take(_ray_tri_64(w[:, k], -d, q[:, 0], q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]))
        for i in range(3):
            for j in range(3):
                take(_edge_edge_64(w[:, i], w[:, (i + 1) % 3] - w[:, i], q[:, j], q[:, (j + 1) % 3] - q[:, j], d))
    return best


def posed(q, d, t):
    """the query triangles [P, 3, 3] at time t [P] in float64"""
    return np.asarray(q, np.float64) + (np.asarray(t, np.float64)[:, None] * np.asarray(d, np.float64))[:, None, :]


def touch_distance(w, q, d, t):
    """[P] float64: the distance between triangle w[p] and the query posed at t[p] (np_tri_distance.witness)"""
    return ntd.witness(w, posed(q, d, t))


def pair_model(w, q, d, tmin, tmax, mutate=None):
    """the float32 semantics pair by pair: triangle w[p] alone as the scene of query p.  -> (t_eff [P] float32, inf a miss; feature [P])"""
    w, q = np.asarray(w, F), np.asarray(q, F)
    s = sweeps_of(q, d, tmin, tmax)
    v0, e1, e2 = w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]
    tlo, thi = np.minimum(np.minimum(w[:, 0], w[:, 1]), w[:, 2]), np.maximum(np.maximum(w[:, 0], w[:, 1]), w[:, 2])
    qlo, qhi = nto.query_box(s[:, 0:12])
    col = lambda x: [x[:, k] for k in range(3)]   # noqa: E731
    with np.errstate(all="ignore"):
        tn, passed = shifted_slab(qlo, qhi, tlo, thi, s[:, 12:15], s[:, 3], s[:, 7])
        tt, _, _, _, _, feat = pair_cast(col(v0), col(e1), col(e2), col(s[:, 0:3]), col(s[:, 4:7]), col(s[:, 8:11]), col(s[:, 12:15]), s[:, 3], s[:, 7], mutate)
        hit = passed & (tt < np.inf) & live(s)
        return np.where(hit, np.fmax(tt, tn), F(np.inf)).astype(F), np.where(hit, feat, -1)
