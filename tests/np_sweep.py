"""The reference of tests/test_sphere_cast.py: art_cast_spheres' semantics restated in numpy.

brute_force   the semantics over every (ray, triangle) pair, operation by operation, in float32 -- what the device must write, ids and bits -- or, with dtype=float64,
              the same function on the same float32 inputs (the accuracy test's yardstick).  The inflated-box slab is evaluated for every pair; the eight features only
              for the pairs that pass it, which is the semantics' own condition for a candidate.
It reuses np_closest.world_triangles and np_closest.tri_closest (feature S); the independent witness is np_closest.witness."""
import contextlib

import numpy as np

import np_closest as nc

F32 = np.float32
FEATURES = ("S", "F", "E01", "E02", "E12", "V0", "V1", "V2")


@contextlib.contextmanager
def _precision(F):
    """np_closest computes in its module-wide F: the float64 run of this file's one function borrows it for the duration"""
    old, nc.F = nc.F, F
    try:
        yield
    finally:
        nc.F = old


def _fma(a, b, c, F):
    """fmaf(a, b, c) for float32 operands, with ONE rounding: the product is exact in float64, the sum is rounded to odd there (TwoSum gives its error exactly) and then
    to float32 -- 53 >= 2 * 24 + 2 bits, so the result is the correctly rounded one.  float64: a * b + c, two roundings (nothing is compared by bits there)"""
    if F is not F32:
        return a * b + c
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) != 0
    fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ~odd
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _root(A, B, Cq, F):
    """the ENTRY root of A t^2 + 2 B t + Cq = 0 -> t, valid"""
    disc = B * B - A * Cq
    t = (-B - np.sqrt(np.where(disc >= 0, disc, F(0)))) / np.where(A > 0, A, F(1))
    return t, (A > 0) & (disc >= 0)


def _edge(m, e, d, rr, F):
    ee = nc._dot(e, e)
    q = np.where(ee > 0, ee, F(1))
    qm, qd = nc._dot(m, e) / q, nc._dot(d, e) / q
    mp, dp = [m[k] - qm * e[k] for k in range(3)], [d[k] - qd * e[k] for k in range(3)]
    t, ok = _root(nc._dot(dp, dp), nc._dot(mp, dp), nc._dot(mp, mp) - rr, F)
    s = qm + t * qd
    return t, s, (ee > 0) & ok & (s >= 0) & (s <= 1)


def tri_sweep(w0, d, e1, e2, rho, tmin, tmax, F=F32):
    """t_tri, u, v, feature (index into FEATURES, -1 none) for broadcastable component triples of dtype F: the device's tri_sweep, operation by operation"""
    rr, dd = rho * rho, nc._dot(d, d)
    shape = np.broadcast(w0[0], e1[0], tmin).shape
    best, u, v, feat = np.full(shape, np.inf, F), np.zeros(shape, F), np.zeros(shape, F), np.full(shape, -1, np.int8)
    zero, one = np.zeros(shape, F), np.ones(shape, F)

    def take(ok, t, cu, cv, f):
        nonlocal best, u, v, feat
        k = ok & (t >= tmin) & (t < tmax) & (t < best)
        best, u, v, feat = np.where(k, t, best), np.where(k, cu, u), np.where(k, cv, v), np.where(k, np.int8(f), feat)
    with _precision(F):
        d2, su, sv, _ = nc.tri_closest([w0[k] + tmin * d[k] for k in range(3)], e1, e2)
    take(d2 <= rr, tmin + zero, su, sv, 0)
    n = nc._cross(e1, e2)
    nn, h, nd = nc._dot(n, n), nc._dot(n, w0), nc._dot(n, d)
    off = rho * np.sqrt(nn)
    off = np.where(h >= 0, off, -off)
    t = (off - h) / np.where(nd != 0, nd, F(1))
    w = [w0[k] + t * d[k] for k in range(3)]
    den = np.where(nn > 0, nn, F(1))
    fu, fv = nc._dot(nc._cross(w, e2), n) / den, nc._dot(nc._cross(e1, w), n) / den
    take((nn > 0) & (nd != 0) & (fu >= 0) & (fv >= 0) & (fu + fv <= 1), t, fu, fv, 1)
    w1, w2 = [w0[k] - e1[k] for k in range(3)], [w0[k] - e2[k] for k in range(3)]
    t, s, ok = _edge(w0, e1, d, rr, F)
    take(ok, t, s, zero, 2)
    t, s, ok = _edge(w0, e2, d, rr, F)
    take(ok, t, zero, s, 3)
    t, s, ok = _edge(w1, [e2[k] - e1[k] for k in range(3)], d, rr, F)
    take(ok, t, F(1) - s, s, 4)
    for f, (m, cu, cv) in enumerate(((w0, zero, zero), (w1, one, zero), (w2, zero, one))):
        t, ok = _root(dd, nc._dot(m, d), nc._dot(m, m) - rr, F)
        take(ok, t + zero, cu, cv, 5 + f)
    return best.astype(F), u.astype(F), v.astype(F), feat


def brute_force(T, rays, rho, vis=None, cull=0xFF, chunk=128, stats=False, dtype=F32):
    """T: np_closest.world_triangles(); rays [n, 8] float32 (o.xyz, tmin, d.xyz, tmax); rho: the radius; vis: the primitives' masks (None: all 0xFF).  -> tuv [n, 4],
    ids [n, 2] int32, point [n, 4] as the device writes them (dtype float32), or computed in float64 from the same inputs.  stats: also a dict -- feature [n] of the
    winning candidate (-1: a miss), ties [n] candidates that share the minimum t_eff, raised: pairs where the box's entry lies above t_tri"""
    F = dtype
    r = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    n, nt = r.shape[0], T["v0"].shape[0]
    tuv, ids, point = np.zeros((n, 4), F), np.full((n, 2), -1, np.int32), np.zeros((n, 4), F)
    tuv[:, 0] = r[:, 7]
    feature, ties, raised = np.full(n, -1, np.int8), np.zeros(n, np.int64), 0
    seen = np.ones(nt, bool) if vis is None else (np.asarray(vis)[T["prim"]] & cull) != 0
    if cull == 0:
        seen[:] = False
    rho = F(F32(rho))
    tri = {k: T[k].astype(F) for k in ("v0", "e1", "e2")}
    lo, hi = T["lo"].astype(F) - rho, T["hi"].astype(F) + rho          # the triangle's own box, inflated: one operation a plane
    with np.errstate(all="ignore"):
        live = np.isfinite(r[:, 0:3]).all(axis=1) & np.isfinite(r[:, 4:7]).all(axis=1) & ~np.isnan(r[:, 7])
        for a in range(0, n, chunk):
            at = np.flatnonzero(live[a:a + chunk]) + a
            if not at.size:
                continue
            o, d, tmin, tmax = r[at, 0:3].astype(F), r[at, 4:7].astype(F), r[at, 3].astype(F), r[at, 7].astype(F)
            safe = np.where(np.abs(d) < F(1e-20), np.copysign(F(1e-20), d), d).astype(F)
            inv = (F(1) / safe).astype(F)
            ood = (o * inv).astype(F)
            t0 = _fma(lo[None], inv[:, None, :], -ood[:, None, :], F)
            t1 = _fma(hi[None], inv[:, None, :], -ood[:, None, :], F)
            tn, tf = np.fmax.reduce(np.fmin(t0, t1), axis=2), np.fmin.reduce(np.fmax(t0, t1), axis=2)
            passed = (np.fmax(tn, tmin[:, None]) <= np.fmin(tf, tmax[:, None])) & seen[None, :]
            ri, gi = np.nonzero(passed)                                  # row-major: ascending gid within a ray
            if not ri.size:
                continue
            col = lambda x, i: [x[i, k] for k in range(3)]   # noqa: E731
            w0 = [o[ri, k] - tri["v0"][gi, k] for k in range(3)]
            tt, u, v, feat = tri_sweep(w0, col(d, ri), col(tri["e1"], gi), col(tri["e2"], gi), rho, tmin[ri], tmax[ri], F)
            cand = tt < np.inf
            raised += int((cand & (tn[ri, gi] > tt)).sum())
            te = np.fmax(tt, tn[ri, gi])
            key = np.full(passed.shape, np.inf, F)
            key[ri[cand], gi[cand]] = te[cand]
            is_c = np.zeros(passed.shape, bool)
            is_c[ri[cand], gi[cand]] = True
            g = np.argmin(key, axis=1)                                   # the first of the smallest: the smallest gid
            rows = np.arange(at.size)
            hit = is_c.any(axis=1)
            # (a candidate's t_eff is finite or +inf; +inf among candidates: the smallest gid of them, which argmin over `key` alone would confuse with a non-candidate)
            inf_only = hit & ~np.isfinite(key[rows, g])
            if inf_only.any():
                g = np.where(inf_only, np.argmax(is_c, axis=1), g)
            ties[at] = np.where(hit, (is_c & (key == key[rows, g][:, None])).sum(axis=1), 0)
            pair = np.full(passed.shape, -1, np.int64)
            pair[ri, gi] = np.arange(ri.size)
            h, gh, ph = at[hit], g[hit], pair[rows[hit], g[hit]]
            bu, bv = u[ph], v[ph]
            tuv[h, 0], tuv[h, 1], tuv[h, 2] = key[rows[hit], gh], bu, bv
            ids[h, 0], ids[h, 1] = T["prim"][gh], T["tri"][gh]
            for k in range(3):
                point[h, k] = tri["v0"][gh, k] + (bu * tri["e1"][gh, k] + bv * tri["e2"][gh, k])
            point[h, 3] = 1
            feature[h] = feat[ph]
    if stats:
        return tuv, ids, point, dict(feature=feature, ties=ties, raised=raised)
    return tuv, ids, point


def centres(rays, t):
    """c(t) = o + t*d in float64 -> [n, 4] queries for np_closest.witness (radius unused)"""
    r = np.asarray(rays, np.float64).reshape(-1, 8)
    q = np.zeros((r.shape[0], 4))
    q[:, 0:3] = r[:, 0:3] + np.asarray(t, np.float64)[:, None] * r[:, 4:7]
    return q
