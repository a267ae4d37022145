"""The reference of tests/test_closest_multi.py: art_closest_points_multi's semantics in numpy float32 over every (query, triangle) pair.

The formulas are tests/np_closest.py's, called and not copied: world_triangles, tri_closest, box_d2.  What is added is 3.10's own part: the candidates in ascending
(d2_eff, global triangle id) and the first K of them as records.  The records for K are a prefix of those for any larger K, so the sorted candidates are computed once
to a depth of ART_CAST_MAX_HITS + 1 (table) and cut to size (records): the entry behind the K-th says whether the K-th rank was contested."""
import numpy as np

import np_closest as nc

F = np.float32
DEPTH = 9   # ART_CAST_MAX_HITS + 1


def table(T, queries, vis=None, cull=0xFF, depth=DEPTH, chunk=256):
    """T: np_closest.world_triangles(); queries [n, 4] float32 (p.xyz, r); vis: the primitives' masks (None: all 0xFF).  -> dict over the queries: gid [n, depth] int64,
    each query's first `depth` candidates in ascending (d2_eff, gid), -1 where there are no more; d2, u, v [n, depth] float32 of those (d2: inf where none); cand [n]
    how many candidates the query has in all"""
    q = np.ascontiguousarray(queries, F).reshape(-1, 4)
    n, nt = q.shape[0], T["v0"].shape[0]
    depth = min(depth, nt)
    gid, d2 = np.full((n, depth), -1, np.int64), np.full((n, depth), np.inf, F)
    bu, bv, total = np.zeros((n, depth), F), np.zeros((n, depth), F), np.zeros(n, np.int64)
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
            dt, u, v, _ = nc.tri_closest([p[k] - v0[k] for k in range(3)], e1, e2)
            bd = nc.box_d2(p, lo, hi).astype(F)
            de = np.maximum(dt, bd)
            r2 = (q[at, 3] * q[at, 3])[:, None]
            cand = seen[None, :] & np.isfinite(dt) & np.isfinite(bd) & (de <= r2)
            key = np.where(cand, de, F(np.inf))
            order = np.argsort(key, axis=1, kind="stable")[:, :depth]   # stable: equal d2_eff stay in gid order; what is no candidate sorts last (a candidate's d2_eff is finite)
            rows = np.arange(at.size)[:, None]
            ok = cand[rows, order]
            gid[at] = np.where(ok, order, -1)
            d2[at] = np.where(ok, de[rows, order], F(np.inf))
            bu[at], bv[at] = np.where(ok, u[rows, order], F(0)), np.where(ok, v[rows, order], F(0))
            total[at] = cand.sum(axis=1)
    return dict(gid=gid, d2=d2, u=bu, v=bv, cand=total)


def records(T, queries, tab, K):
    """the first K entries of table()'s candidates as the device writes them: duv [n, K, 4] float32, ids [n, K, 2] int32, point [n, K, 4] float32, count [n] uint8 --
    each answer art_closest_points' own record for that triangle, then miss records (r as given, 0, 0, 0), (-1, -1) and a point of zeros"""
    q = np.ascontiguousarray(queries, F).reshape(-1, 4)
    n = q.shape[0]
    duv, ids, point = np.zeros((n, K, 4), F), np.full((n, K, 2), -1, np.int32), np.zeros((n, K, 4), F)
    duv[:, :, 0] = q[:, 3][:, None]
    k = min(K, tab["gid"].shape[1])
    g = tab["gid"][:, :k]
    hit = g >= 0
    gh, u, v = g[hit], tab["u"][:, :k][hit], tab["v"][:, :k][hit]
    with np.errstate(all="ignore"):
        rec = np.zeros((gh.size, 4), F)
        rec[:, 0], rec[:, 1], rec[:, 2] = np.sqrt(tab["d2"][:, :k][hit]), u, v
        pt = np.zeros((gh.size, 4), F)
        for c in range(3):
            pt[:, c] = T["v0"][gh, c] + (u * T["e1"][gh, c] + v * T["e2"][gh, c])
        pt[:, 3] = 1
    duv[:, :k][hit], point[:, :k][hit] = rec, pt
    ids[:, :k][hit] = np.stack([T["prim"][gh], T["tri"][gh]], 1)
    return duv, ids, point, hit.sum(axis=1).astype(np.uint8)


def brute_force(T, queries, K, vis=None, cull=0xFF):
    """(duv, ids, point, count) of the queries at K"""
    return records(T, queries, table(T, queries, vis, cull, depth=K), K)


def contested(tab, K):
    """per query: K candidates and more exist, and the K-th and the (K+1)-th share their d2_eff -- the global id alone decided who stayed"""
    if tab["d2"].shape[1] <= K:
        return np.zeros(tab["d2"].shape[0], bool)
    return (tab["gid"][:, K] >= 0) & (tab["d2"][:, K - 1] == tab["d2"][:, K])
