#!/usr/bin/env python3
"""What art_closest_triangles costs.  The scene is sponza_like 1.0 (config 2); the queries are the two sets of tests/test_tri_overlap.py at --queries
(2^20) each: random triangles sized 0.3 % .. 30 % of the scene's extent, and the scene's own triangles moved by 0.1 % .. 2 % of it.  Per set, --repeats times in turn:
the distance at r = 1 % of the extent, the distance at r = +inf, and -- for scale -- art_overlap_triangles LIST at K = 8 with counts on the same queries.  Device ms per
call from events on the stream around --calls calls after --warmup of them; medians and the spread of the repeats; Mquery/s; the share of the queries with an answer,
with d = 0, and the share of those d = 0 that the overlap query counts as touched (the same 17 axes: every one, where the features did not find 0 first).  One JSON line.
    python tools/tri_distance_probe.py [--queries 1048576] [--calls 1] [--warmup 1] [--repeats 3]"""
import argparse, json, os, statistics, sys
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
    world = []
    for p in sc.primitives:
        m = np.asarray(p.model, np.float32).reshape(3, 4)
        v = np.asarray(p.verts, np.float32)[:, 0:3] @ m[:, :3].T + m[:, 3]
        world.append(v[np.asarray(p.indices).reshape(-1, 3)])
    world = np.concatenate(world).astype(np.float32)   # [T, 3, 3]
    lo, hi = world.reshape(-1, 3).min(0), world.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(13)
    c = lo + rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo)
    sets = {"random": c[:, None, :] + ext * 10.0 ** rng.uniform(-2.5, -0.5, (n, 1, 1)) * rng.uniform(-1.0, 1.0, (n, 3, 3))}
    d = rng.normal(0.0, 1.0, (n, 3))
    d *= (ext * 10.0 ** rng.uniform(-3.0, -1.7, n) / np.linalg.norm(d, axis=1))[:, None]
    sets["moved"] = world[rng.integers(0, world.shape[0], n)] + d[:, None, :]
    r = renderer.renderer_for_scene(sc, (64, 64), n_lights=1)
    res = {"what": "tri_distance_probe", "scene": "sponza_like 1.0 (config 2)", "triangles": int(world.shape[0]), "queries": n, "calls": a.calls, "repeats": a.repeats,
           "r_near": 0.01 * ext, "sets": {}}
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    for name, w in sets.items():
        q = np.zeros((n, 3, 4), np.float32); q[:, :, 0:3] = w
        with torch.cuda.stream(s):
            near = torch.from_numpy(q.reshape(n, 12)).cuda()
            far = near.clone()
            near[:, 3], far[:, 3] = 0.01 * ext, float("inf")
            outs = {leg: (torch.empty((n, 4), device="cuda"), torch.empty((n, 2), dtype=torch.int32, device="cuda"), torch.empty((n, 4), device="cuda"), torch.empty((n, 4), device="cuda"))
                    for leg in ("r_1pct", "r_inf")}
            ids, count = torch.empty((n, 8, 2), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda")
        legs = {"r_1pct": lambda: r.closest_triangles(near, out=outs["r_1pct"]), "r_inf": lambda: r.closest_triangles(far, out=outs["r_inf"]),
                "overlap_list8": lambda: r.overlap_triangles(near, "list", 8, out=(ids, count))}
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
        out = {"legs": {}}
        for leg, t in runs.items():
            med = statistics.median(t)
            out["legs"][leg] = {"device_ms": [round(x, 4) for x in t], "median": round(med, 4), "spread_pct": round(100.0 * (max(t) / min(t) - 1.0), 2), "m_per_s": round(n / med / 1e3, 2)}
        for leg in ("r_1pct", "r_inf"):
            duv, rid = outs[leg][0], outs[leg][1]
            has = rid[:, 0] >= 0
            zero = has & (duv[:, 0] == 0)
            out[leg] = {"answered_pct": round(100.0 * int(has.sum()) / n, 3), "zero_pct": round(100.0 * int(zero.sum()) / n, 3),
                        "zero_and_touched_pct_of_zero": round(100.0 * int((zero & (count > 0)).sum()) / max(int(zero.sum()), 1), 3),
                        "touched_and_not_zero": int(((count > 0) & ~zero).sum()), "median_d_of_clear": float(duv[has & ~zero, 0].median()) if bool((has & ~zero).any()) else None}
        assert bool((outs["r_inf"][1][:, 0] >= 0).all())   # r = +inf: every query has an answer
        res["sets"][name] = out
    res["counts"] = r.cast_counts()
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
