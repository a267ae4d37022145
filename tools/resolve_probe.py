#!/usr/bin/env python3
"""What art_resolve_hits costs beside the cast that feeds it.  The scene is sponza_like 1.0 (config 2); the rays are --rays (2^22) of the scene's camera in
pixel order (a square frame: neighbouring records hit neighbouring triangles) and as many random_rays of the tests (tests/helpers.py: incoherent -- neighbouring records hit
unrelated triangles, so every lane of the gather reads another 144-byte shading record).  Per order, --repeats times in turn: the closest cast, the resolve of its records
with all six outputs, and with pos + ng only -- device ms per call from events on the stream around --calls calls after --warmup of them; medians, the spread of the repeats.
Bytes are counted from the record layout, not from counters: every record 24 B in and its outputs (88 B with all six, 32 B with pos + ng); every HIT record also 4 B of the
gid -> leaf table, the 144-byte shading record and 16 B of texels per layer sampled (three with all six outputs, none with pos + ng).  The primitive table (144 B a
primitive) is shared by all records and not counted.  gb_per_s = those bytes / device time, against the 8 TB/s HBM peak of the data sheet: what the lanes ask for.  Records
that name the same triangle share its shading record and texels through the caches (in pixel order a triangle covers many pixels), so the figure can pass the peak;
stream_gb_per_s counts only what no cache can save -- the records in and the outputs out -- and is the floor of the HBM traffic.
One JSON line.
    python tools/resolve_probe.py [--rays 4194304] [--calls 10] [--warmup 3] [--repeats 3]"""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12


def camera_rays(cam, side):
    """the primary rays of raytrace.rgen.glsl:78-88 for a side x side frame, in pixel order (numpy, float64 -> float32)"""
    import numpy as np
    import np_shading as nps
    view, view_inv, proj, proj_inv = nps.camera_matrices(cam["pos"], cam["dir"], 1.0, cam["fovy"], cam["znear"], cam["zfar"])
    y, x = np.mgrid[0:side, 0:side]
    d = (np.stack([x.reshape(-1) + 0.5, y.reshape(-1) + 0.5], 1) / side) * 2.0 - 1.0
    t = np.concatenate([d, np.ones((d.shape[0], 2))], 1) @ proj_inv.T
    t = t[:, :3] / np.linalg.norm(t[:, :3], axis=1, keepdims=True)
    rays = np.zeros((d.shape[0], 8), np.float32)
    rays[:, 0:3] = (view_inv @ np.array([0.0, 0.0, 0.0, 1.0]))[:3]
    rays[:, 3], rays[:, 4:7], rays[:, 7] = 0.001, t @ view_inv[:3, :3].T, 10000.0
    return rays


def main():
    import torch
    from araytracingjourney_amd import renderer, scenes
    from helpers import random_rays
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22); ap.add_argument("--calls", type=int, default=10); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    side = int(math.isqrt(a.rays))
    n = side * side
    sc = scenes.sponza_like(1.0)
    r = renderer.renderer_for_scene(sc, (64, 64), n_lights=1)
    orders = {"pixel_order": torch.from_numpy(camera_rays(sc.camera, side)).cuda(), "random_rays": torch.from_numpy(random_rays(n, 7)).cuda()}
    tuv = torch.empty((n, 4), dtype=torch.float32, device="cuda"); ids = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    names = ("pos", "ng", "ns", "uv", "albedo", "orm")
    bufs = {k: torch.empty((n, renderer.Renderer._RESOLVE_OUTPUTS[k]), dtype=torch.float32, device="cuda") for k in names}
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    legs = {"cast_closest": lambda d: r.cast_rays(d, out=(tuv, ids)), "resolve_all_six": lambda d: r.resolve_hits(tuv, ids, names, out=bufs),
            "resolve_pos_ng": lambda d: r.resolve_hits(tuv, ids, ("pos", "ng"), out=bufs)}
    out = {"what": "resolve_probe", "scene": "sponza_like 1.0 (config 2)", "records": n, "calls": a.calls, "repeats": a.repeats, "hbm_peak_gb_s": HBM_PEAK / 1e9, "orders": {}}
    with torch.cuda.stream(s):
        for order, d in orders.items():
            runs = {leg: [] for leg in legs}
            for _ in range(a.repeats):
                for leg, call in legs.items():   # (the cast first: the resolves read its records)
                    for _ in range(a.warmup):
                        call(d)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(a.calls):
                        call(d)
                    e1.record(s)
                    s.synchronize()
                    runs[leg].append(e0.elapsed_time(e1) / a.calls)
            hits = int((ids[:, 0] >= 0).sum().item())
            res = {"hit_records": hits}
            for leg, v in runs.items():
                med = statistics.median(v)
                res[leg] = {"device_ms": [round(x, 4) for x in v], "median": round(med, 4), "spread_pct": round(100.0 * (max(v) / min(v) - 1.0), 2)}
                if leg != "cast_closest":
                    o, layers = (88, 3) if leg == "resolve_all_six" else (32, 0)
                    per_hit = 24 + o + 4 + 144 + 16 * layers
                    total = n * (24 + o) + hits * (4 + 144 + 16 * layers)
                    res[leg].update(bytes_per_hit_record=per_hit, gb_per_s=round(total / med / 1e6, 1), of_hbm_peak=round(total / (med * 1e-3) / HBM_PEAK, 4),
                                    stream_gb_per_s=round(n * (24 + o) / med / 1e6, 1), stream_of_hbm_peak=round(n * (24 + o) / (med * 1e-3) / HBM_PEAK, 4),
                                    over_cast=round(med / statistics.median(runs["cast_closest"]), 4))
            out["orders"][order] = res
    out["counts"] = r.cast_counts()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
