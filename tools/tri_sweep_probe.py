#!/usr/bin/env python3
"""What art_cast_triangles costs.  The scene is sponza_like 1.0 (config 2); --queries (2^20) random triangles of two sizes -- the three vertices within
a cube of side 0.5 % and 5 % of the scene's extent round a centre in the scene's box -- each swept along a random direction by 10 % of the extent (tmin 0, tmax 1).  Per
size, --repeats times in turn: the swept triangles; for scale, art_cast_spheres over the same rays (the centre, d, tmin, tmax) at rho = half the cube's diagonal, the ball
that holds the query; and art_closest_triangles over the same triangles at r = |d|, the sweep's reach.  Device ms per call from events on the stream around --calls calls
after --warmup of them; medians and the spread of the repeats; Mquery/s; the share of the queries with a contact, with one at tmin (S), and of the balls that touch.  One
JSON line.
    python tools/tri_sweep_probe.py [--queries 1048576] [--calls 1] [--warmup 1] [--repeats 3]"""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from araytracingjourney_amd import renderer, scenes
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1 << 20); ap.add_argument("--calls", type=int, default=1); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    n = a.queries
    sc = scenes.sponza_like(1.0)
    pts = []
    for p in sc.primitives:
        m = np.asarray(p.model, np.float32).reshape(3, 4)
        pts.append(np.asarray(p.verts, np.float32)[:, 0:3] @ m[:, :3].T + m[:, 3])
    pts = np.concatenate(pts)
    lo, hi = pts.min(0), pts.max(0)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(13)
    c = (lo + rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.normal(0.0, 1.0, (n, 3))
    d = (d * (0.1 * ext / np.linalg.norm(d, axis=1))[:, None]).astype(np.float32)
    unit = rng.uniform(-0.5, 0.5, (n, 3, 3))
    r = renderer.renderer_for_scene(sc, (64, 64), n_lights=1)
    res = {"what": "tri_sweep_probe", "scene": "sponza_like 1.0 (config 2)", "triangles": int(sum(np.asarray(p.indices).size // 3 for p in sc.primitives)), "queries": n, "calls": a.calls,
           "repeats": a.repeats, "extent": ext, "reach": 0.1 * ext, "sizes": {}}
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    for pct in (0.5, 5.0):
        side = 0.01 * pct * ext
        rho = 0.5 * math.sqrt(3.0) * side
        q = np.zeros((n, 16), np.float32)
        tri = c[:, None, :] + (side * unit).astype(np.float32)
        q[:, 0:3], q[:, 4:7], q[:, 8:11], q[:, 12:15], q[:, 7] = tri[:, 0], tri[:, 1], tri[:, 2], d, 1.0
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3], rays[:, 4:7], rays[:, 7] = c, d, 1.0
        near = np.ascontiguousarray(q[:, 0:12]); near[:, 3] = 0.1 * ext; near[:, 7] = 0.0
        with torch.cuda.stream(s):
            d_q, d_r, d_t = torch.from_numpy(q).cuda(), torch.from_numpy(rays).cuda(), torch.from_numpy(near).cuda()
            four = lambda: (torch.empty((n, 4), device="cuda"), torch.empty((n, 2), dtype=torch.int32, device="cuda"), torch.empty((n, 4), device="cuda"), torch.empty((n, 4), device="cuda"))   # noqa: E731
            o_cast, o_dist = four(), four()
            o_ball = four()[:3]
        legs = {"cast_triangles": lambda: r.cast_triangles(d_q, out=o_cast), "cast_spheres": lambda: r.cast_spheres(d_r, rho, out=o_ball), "closest_triangles": lambda: r.closest_triangles(d_t, out=o_dist)}
        runs = {leg: [] for leg in legs}
        with torch.cuda.stream(s):
            for _ in range(a.repeats):
                for leg, call in legs.items():
                    for _ in range(a.warmup):
                        call()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(a.calls):
                        call()
                    e1.record(s)
                    s.synchronize()
                    runs[leg].append(e0.elapsed_time(e1) / a.calls)
        out = {"side": side, "rho": rho, "legs": {}}
        for leg, t in runs.items():
            med = statistics.median(t)
            out["legs"][leg] = {"device_ms": [round(x, 4) for x in t], "median": round(med, 4), "spread_pct": round(100.0 * (max(t) / min(t) - 1.0), 2), "m_per_s": round(n / med / 1e3, 2)}
        has = o_cast[1][:, 0] >= 0
        out["contact_pct"] = round(100.0 * int(has.sum()) / n, 3)
        out["at_tmin_pct"] = round(100.0 * int((has & (o_cast[0][:, 0] == 0)).sum()) / n, 3)
        out["ball_touches_pct"] = round(100.0 * int((o_ball[1][:, 0] >= 0).sum()) / n, 3)
        out["within_reach_pct"] = round(100.0 * int((o_dist[1][:, 0] >= 0).sum()) / n, 3)
        out["median_t"] = float(o_cast[0][has, 0].median()) if bool(has.any()) else None
        res["sizes"][f"{pct:g}pct"] = out
    res["counts"] = r.cast_counts()
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
