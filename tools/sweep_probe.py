#!/usr/bin/env python3
"""What art_cast_spheres costs, beside the closest cast of the same rays in the same run.  The scene is sponza_like 1.0 (config 2); --rays (2^22) rays of
two kinds: "random" -- the tests' random_rays (unrelated neighbours) -- and "pixels" -- the scene's camera rays in pixel order (tools/resolve_probe.py's); radii 0, 0.01
and 0.05 (--radii).  Per kind and radius, --repeats times in turn: device ms per call from events on the stream around --calls calls after --warmup of them; medians and
the spread of the repeats; Mray/s; the share of rays that touch something.  One JSON line.
    python tools/sweep_probe.py [--rays 4194304] [--radii 0,0.01,0.05] [--calls 5] [--warmup 2] [--repeats 3] [--leaf-batch N] [--refill N] [--chunk N]"""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    from araytracingjourney_amd import renderer, scenes
    from helpers import random_rays
    from resolve_probe import camera_rays
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22); ap.add_argument("--radii", default="0,0.01,0.05")
    ap.add_argument("--calls", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leaf-batch", type=int, default=0); ap.add_argument("--refill", type=int, default=0); ap.add_argument("--chunk", type=int, default=0)   # ArtTuning overrides, for sweeps (0: the preset)
    a = ap.parse_args()
    side = int(math.isqrt(a.rays))
    n = side * side
    radii = [float(x) for x in a.radii.split(",")]
    sc = scenes.sponza_like(1.0)
    tuning = {"trace_leaf_batch": a.leaf_batch, "trace_refill": a.refill, "trace_chunk": a.chunk}
    r = renderer.renderer_for_scene(sc, (64, 64), n_lights=1, tuning=tuning)
    kinds = {"random": torch.from_numpy(random_rays(n, 7)).cuda(), "pixels": torch.from_numpy(camera_rays(sc.camera, side)).cuda()}
    out_c = (torch.empty((n, 4), device="cuda"), torch.empty((n, 2), dtype=torch.int32, device="cuda"))
    out_s = out_c + (torch.empty((n, 4), device="cuda"),)
    legs = {}
    for k, rays in kinds.items():
        legs[f"cast_closest_{k}"] = (lambda rays=rays: r.cast_rays(rays, out=out_c))
        for rho in radii:
            legs[f"sweep_{k}_r{rho:g}"] = (lambda rays=rays, rho=rho: r.cast_spheres(rays, rho, out=out_s))
    runs = {leg: [] for leg in legs}
    res = {"what": "sweep_probe", "scene": "sponza_like 1.0 (config 2)", "rays": n, "calls": a.calls, "repeats": a.repeats, "tuning": tuning, "legs": {}, "hit_share": {}}
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
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
                res["hit_share"][leg] = round(float((out_c[1][:, 0] >= 0).float().mean().item()), 4)
    for leg, v in runs.items():
        med = statistics.median(v)
        res["legs"][leg] = {"device_ms": [round(x, 4) for x in v], "median": round(med, 4), "spread_pct": round(100.0 * (max(v) / min(v) - 1.0), 2), "m_per_s": round(n / med / 1e3, 1)}
    res["counts"] = r.cast_counts()
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
