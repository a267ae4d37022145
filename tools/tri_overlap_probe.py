#!/usr/bin/env python3
"""What art_overlap_triangles costs.  The scene is sponza_like 1.0 (config 2); the queries are the two sets of tests/test_tri_overlap.py at --queries
(2^20) each: random triangles sized 0.3 % .. 30 % of the scene's extent, and the scene's own triangles moved by 0.1 % .. 2 % of it.  Per set, --repeats times in turn:
ANY, LIST at K = 8 with counts, and -- what a caller had to use before -- art_overlap_boxes, ANY and LIST, on the same queries' own boxes.  Device ms per call from
events on the stream around --calls calls after --warmup of them; medians and the spread of the repeats; Mquery/s; the share of the box answers the exact test rejects
(queries the box calls touched and the triangle does not; candidates the box counts and the triangle does not).  One JSON line.
    python tools/tri_overlap_probe.py [--queries 1048576] [--calls 1] [--warmup 1] [--repeats 3]"""
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
    res = {"what": "tri_overlap_probe", "scene": "sponza_like 1.0 (config 2)", "triangles": int(world.shape[0]), "queries": n, "calls": a.calls, "repeats": a.repeats, "sets": {}}
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    for name, w in sets.items():
        q = np.zeros((n, 3, 4), np.float32); q[:, :, 0:3] = w
        with torch.cuda.stream(s):
            tris = torch.from_numpy(q.reshape(n, 12)).cuda()
            boxes = torch.zeros((n, 8), device="cuda")
            v = tris.reshape(n, 3, 4)[:, :, 0:3]
            boxes[:, 0:3], boxes[:, 4:7] = v.min(dim=1).values, v.max(dim=1).values
            hit, bhit = (torch.empty((n,), dtype=torch.uint8, device="cuda") for _ in range(2))
            ids, bids = (torch.empty((n, 8, 2), dtype=torch.int32, device="cuda") for _ in range(2))
            count, bcount = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
        legs = {"any": lambda: r.overlap_triangles(tris, "any", out=hit), "list8": lambda: r.overlap_triangles(tris, "list", 8, out=(ids, count)),
                "box_any": lambda: r.overlap_boxes(boxes, "any", out=bhit), "box_list8": lambda: r.overlap_boxes(boxes, "list", 8, out=(bids, bcount))}
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
            out["legs"][leg] = {"device_ms": [round(x, 4) for x in t], "median": round(med, 4), "spread_pct": round(100.0 * (max(t) / min(t) - 1.0), 2), "m_per_s": round(n / med / 1e3, 1)}
        assert bool((hit.bool() == (count > 0)).all()) and bool((bhit.bool() == (bcount > 0)).all())   # ANY is LIST's count > 0
        touched, btouched = int(hit.sum()), int(bhit.sum())
        cands, bcands = int(count.to(torch.int64).sum()), int(bcount.to(torch.int64).sum())
        out["touched_pct"] = {"triangle": round(100.0 * touched / n, 3), "box": round(100.0 * btouched / n, 3)}
        out["box_answers_rejected_pct"] = {"queries": round(100.0 * (btouched - touched) / max(btouched, 1), 3), "candidates": round(100.0 * (bcands - cands) / max(bcands, 1), 3)}
        out["more_by_triangle_than_by_box"] = int((count > bcount).sum())   # (a triangle that touches the query touches its box, up to the two tests' roundings)
        out["mean_count_of_touched"] = {"triangle": round(cands / max(touched, 1), 2), "box": round(bcands / max(btouched, 1), 2)}
        res["sets"][name] = out
    res["counts"] = r.cast_counts()
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
