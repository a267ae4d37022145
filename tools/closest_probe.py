#!/usr/bin/env python3
"""What art_closest_points costs, beside the closest cast of as many rays for scale.  The scene is sponza_like 1.0 (config 2); --points (2^22) queries
with r = inf of three kinds: "surface" -- the hit positions of the scene's camera rays in pixel order (d near 0: the walk finds its answer at once and prunes everything
else), "box" -- uniform in the scene's bounding box, "sphere" -- on a sphere outside it (large d: the limit stays wide and whole subtrees tie).  Per kind, --repeats
times in turn: the queries, device ms per call from events on the stream around --calls calls after --warmup of them; medians and the spread of the repeats; Mquery/s.
The cast is the pixel-order cast of tools/resolve_probe.py.  One JSON line.
    python tools/closest_probe.py [--points 4194304] [--calls 5] [--warmup 2] [--repeats 3] [--leaf-batch N] [--refill N] [--chunk N]"""
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leaf-batch", type=int, default=0); ap.add_argument("--refill", type=int, default=0); ap.add_argument("--chunk", type=int, default=0)   # ArtTuning overrides, for sweeps (0: the preset)
    a = ap.parse_args()
    side = int(math.isqrt(a.points))
    n = side * side
    sc = scenes.sponza_like(1.0)
    tuning = {"trace_leaf_batch": a.leaf_batch, "trace_refill": a.refill, "trace_chunk": a.chunk}
    r = renderer.renderer_for_scene(sc, (64, 64), n_lights=1, tuning=tuning)
    rays = torch.from_numpy(camera_rays(sc.camera, side)).cuda()
    (tuv, ids), surf = r.cast_surface(rays, want=("pos",))
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
    out_q = (torch.empty((n, 4), device="cuda"), torch.empty((n, 2), dtype=torch.int32, device="cuda"), torch.empty((n, 4), device="cuda"))
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    legs = {"cast_closest": lambda: r.cast_rays(rays, out=(tuv, ids))}
    for k, q in kinds.items():
        legs["closest_" + k] = (lambda q=q: r.closest_points(q, out=out_q))
    runs = {leg: [] for leg in legs}
    res = {"what": "closest_probe", "scene": "sponza_like 1.0 (config 2)", "queries": n, "calls": a.calls, "repeats": a.repeats, "tuning": tuning, "legs": {}}
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
                if leg != "cast_closest":
                    res.setdefault("mean_distance", {})[leg] = round(float(out_q[0][:, 0].mean().item()), 5)
    for leg, v in runs.items():
        med = statistics.median(v)
        res["legs"][leg] = {"device_ms": [round(x, 4) for x in v], "median": round(med, 4), "spread_pct": round(100.0 * (max(v) / min(v) - 1.0), 2), "m_per_s": round(n / med / 1e3, 1)}
    res["counts"] = r.cast_counts()
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
