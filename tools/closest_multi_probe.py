#!/usr/bin/env python3
"""What art_closest_points_multi costs, beside art_closest_points on the same queries in the same run: what the list costs at K = 1 against the
single-answer kernel, and how the time grows with K.  The scene and the queries are tools/closest_probe.py's: sponza_like 1.0 (config 2), --points (2^22) queries with
r = inf, "surface" -- the hit positions of the scene's camera rays in pixel order, "box" -- uniform in the scene's bounding box, "sphere" -- on a sphere outside it.
Per kind and leg (closest_points, then this call at each of --ks), --repeats times in turn: device ms per call from events on the stream around --calls calls after
--warmup of them; medians and the spread of the repeats; Mquery/s; the mean count and the mean distance of the last record that is an answer.  One JSON line.
    python tools/closest_multi_probe.py [--points 4194304] [--ks 1,4,8] [--calls 5] [--warmup 2] [--repeats 3] [--leaf-batch N] [--refill N] [--chunk N]"""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    from araytracingjourney_amd import renderer, scenes
    from resolve_probe import camera_rays
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 22); ap.add_argument("--calls", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--ks", default="1,4,8")
    ap.add_argument("--leaf-batch", type=int, default=0); ap.add_argument("--refill", type=int, default=0); ap.add_argument("--chunk", type=int, default=0)   # ArtTuning overrides, for sweeps (0: the preset)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    side = int(math.isqrt(a.points))
    n = side * side
    sc = scenes.sponza_like(1.0)
    tuning = {"trace_leaf_batch": a.leaf_batch, "trace_refill": a.refill, "trace_chunk": a.chunk}
    r = renderer.renderer_for_scene(sc, (64, 64), n_lights=1, tuning=tuning)
    rays = torch.from_numpy(camera_rays(sc.camera, side)).cuda()
    _, surf = r.cast_surface(rays, want=("pos",))
    torch.cuda.synchronize()
    pos = surf["pos"]
    hit = pos[:, 3] == 1
    lo, hi = pos[hit, :3].min(0).values, pos[hit, :3].max(0).values   # (the box of what the camera sees: the scene's, near enough for a probe)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    on = torch.where(hit[:, None], pos[:, :3], pos[hit, :3][0])   # pixel order; a ray that missed takes the first hit's point
    inf = torch.full((n, 1), math.inf, device="cuda")
    box = lo + (hi - lo) * torch.rand((n, 3), device="cuda", generator=g)
    d = torch.randn((n, 3), device="cuda", generator=g)
    sph = (lo + hi) * 0.5 + d / d.norm(dim=1, keepdim=True) * (hi - lo).norm()
    kinds = {"surface": torch.cat([on, inf], 1).contiguous(), "box": torch.cat([box, inf], 1).contiguous(), "sphere": torch.cat([sph, inf], 1).contiguous()}
    del rays, surf, pos, on, box, sph, d
    out_1 = (torch.empty((n, 4), device="cuda"), torch.empty((n, 2), dtype=torch.int32, device="cuda"), torch.empty((n, 4), device="cuda"))
    out_k = {k: (torch.empty((n, k, 4), device="cuda"), torch.empty((n, k, 2), dtype=torch.int32, device="cuda"), torch.empty((n, k, 4), device="cuda"),
                 torch.empty((n,), dtype=torch.uint8, device="cuda")) for k in ks}
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    legs = {}
    for kind, q in kinds.items():
        legs[(kind, 0)] = (lambda q=q: r.closest_points(q, out=out_1))
        for k in ks:
            legs[(kind, k)] = (lambda q=q, k=k: r.closest_points_multi(q, k, out=out_k[k]))
    runs = {leg: [] for leg in legs}
    res = {"what": "closest_multi_probe", "scene": "sponza_like 1.0 (config 2)", "queries": n, "calls": a.calls, "repeats": a.repeats, "tuning": tuning, "legs": {}}
    seen = {}
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
                kind, k = leg
                if k:   # what came back: answers a query, the distance of the farthest of them
                    duv, _, _, count = out_k[k]
                    last = duv[:, :, 0].gather(1, (count.long() - 1).clamp(min=0)[:, None])[:, 0]
                    seen[leg] = (round(float(count.float().mean().item()), 3), round(float(last[count > 0].mean().item()), 5))
                else:
                    seen[leg] = (1.0, round(float(out_1[0][:, 0].mean().item()), 5))
    for (kind, k), v in runs.items():
        med = statistics.median(v)
        single = statistics.median(runs[(kind, 0)])
        res["legs"][f"{kind}_" + (f"k{k}" if k else "single")] = {"device_ms": [round(x, 4) for x in v], "median": round(med, 4), "spread_pct": round(100.0 * (max(v) / min(v) - 1.0), 2),
                                                                  "m_per_s": round(n / med / 1e3, 1), "over_single": round(med / single, 3), "mean_count": seen[(kind, k)][0],
                                                                  "mean_last_distance": seen[(kind, k)][1]}
    res["counts"] = r.cast_counts()
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
