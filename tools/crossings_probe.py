#!/usr/bin/env python3
"""The surfaces each ray enters and leaves on config 2 (art_cast_crossings): what the uncapped count costs beside the closest cast and the list of 8.
The scene is sponza_like 1.0; the rays are --rays (2^22) random_rays of the tests (tests/helpers.py: from a sphere around the scene and from inside it, towards points
near the origin -- incoherent, and most go through several surfaces).  Per leg: device time per cast from events on the cast's stream around --casts casts after --warmup
of them, --repeats times in turn (closest, multi 8, crossings, closest, ...), all in this one run; medians, the spread of the repeats, Mray/s.  For crossings also what it
counted: all crossings, entries, exits, the most of one ray and the rays with more than 8 -- those the list of 8 cuts.
One JSON line.
    python tools/crossings_probe.py [--rays 4194304] [--casts 10] [--warmup 3] [--repeats 3] [--legs closest,multi8,crossings]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from araytracingjourney_amd import renderer, scenes
    from helpers import random_rays
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22); ap.add_argument("--casts", type=int, default=10); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--legs", default="closest,multi8,crossings")
    a = ap.parse_args()
    legs, n = a.legs.split(","), a.rays
    r = renderer.renderer_for_scene(scenes.sponza_like(1.0), (64, 64), n_lights=1)
    d = torch.from_numpy(random_rays(n, 7)).cuda()
    kmax = max([int(leg[5:]) for leg in legs if leg.startswith("multi")] + [1])
    tuv = torch.empty((n * kmax, 4), dtype=torch.float32, device="cuda"); ids = torch.empty((n * kmax, 2), dtype=torch.int32, device="cuda")
    byte = torch.empty((n,), dtype=torch.uint8, device="cuda"); cross = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())

    def cast(leg):
        if leg == "closest":
            r.cast_rays(d, out=(tuv[:n], ids[:n]))
        elif leg == "crossings":
            r.cast_crossings(d, out=cross)
        else:
            k = int(leg[5:])
            r.cast_rays_multi(d, k, out=(tuv[:n * k].view(n, k, 4), ids[:n * k].view(n, k, 2), byte))
    runs, counted = {leg: [] for leg in legs}, {}
    with torch.cuda.stream(s):
        for _ in range(a.repeats):
            for leg in legs:
                for _ in range(a.warmup):
                    cast(leg)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(a.casts):
                    cast(leg)
                e1.record(s)
                s.synchronize()
                runs[leg].append(e0.elapsed_time(e1) / a.casts)
                if leg == "closest":
                    counted[leg] = {"hit_records": int((ids[:n, 0] >= 0).sum().item())}
                elif leg == "crossings":
                    total = cross.to(torch.int64).sum(dim=1)
                    counted[leg] = {"crossings": int(total.sum().item()), "entries": int(cross[:, 0].to(torch.int64).sum().item()), "exits": int(cross[:, 1].to(torch.int64).sum().item()),
                                    "most_of_a_ray": int(total.max().item()), "rays_above_8": int((total > 8).sum().item())}
                else:
                    counted[leg] = {"hit_records": int(byte.to(torch.int64).sum().item())}
    out = {"what": "crossings_probe", "scene": "sponza_like 1.0 (config 2)", "rays": n, "casts": a.casts, "repeats": a.repeats, "legs": {}, "counts": r.cast_counts()}
    for leg in legs:
        v = runs[leg]
        med = statistics.median(v)
        out["legs"][leg] = dict({"device_ms_per_cast": [round(x, 4) for x in v], "median": round(med, 4), "spread_pct": round(100.0 * (max(v) / min(v) - 1.0), 2),
                                 "mray_per_s": round(n / med / 1e3, 1)}, **counted[leg])
    if "crossings" in legs:
        for leg in legs:
            if leg != "crossings":
                out["crossings_over_" + leg] = round(out["legs"]["crossings"]["median"] / out["legs"][leg]["median"], 4)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
