#!/usr/bin/env python3
"""Rays in device buffers on config 2 (art_cast_rays): what a cast costs.  The scene is sponza_like 1.0; the rays are the 2^22 primary rays of a
2048 x 2048 frame from config 2's camera (raytrace.rgen.glsl:78-88, tmin 0.001, tmax 10000), once in pixel order (row-major) and once shuffled.
  --mode cast    per ordering and kind (closest, any): device time per cast from events on the cast's stream around --casts casts after --warmup of them; Mray/s
  --mode query   the same rays through art_query_closest / art_query_any (host buffers): runs on a build without art_cast_rays too (ART_LIB_PATH, or a checkout of an
                 earlier commit) -- the kernel's time then comes from `rocprofv3 --kernel-trace --stats -- python tools/cast_probe.py --mode query` (k_trace<2, ..> there,
                 k_cast<..> here: this build has no k_trace<2, ..> instance any more), in a run of its own; --repeats queries per ordering
  --mode frames  what a 1920 x 1080 frame costs (8 ring slots, --steps frames, fenced at both ends) alone and with casts of the shuffled rays kept in flight beside it
One JSON line.
    python tools/cast_probe.py --mode cast [--casts 20] [--warmup 5] [--leaf-batch N] [--refill N] [--chunk N]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 2048


def primary_rays(cam):
    """the rays raytrace.rgen.glsl:78-88 makes for a W x H frame, row-major: o.xyz, tmin, d.xyz, tmax (float32 arithmetic)"""
    import numpy as np
    f = np.float32
    vi = np.frombuffer(bytes(cam), np.float32, 16, 64).reshape(4, 4).T      # view_inv, column-major in the block
    pi = np.frombuffer(bytes(cam), np.float32, 16, 192).reshape(4, 4).T     # proj_inv
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    dx, dy = (x + f(0.5)) / f(W) * f(2) - f(1), (y + f(0.5)) / f(H) * f(2) - f(1)
    tgt = np.stack([pi[k, 0] * dx + pi[k, 1] * dy + pi[k, 2] + pi[k, 3] for k in range(3)], -1).astype(np.float32)
    tgt /= np.linalg.norm(tgt, axis=-1, keepdims=True)
    d = np.stack([vi[k, 0] * tgt[..., 0] + vi[k, 1] * tgt[..., 1] + vi[k, 2] * tgt[..., 2] for k in range(3)], -1).astype(np.float32)
    rays = np.zeros((H * W, 8), np.float32)
    rays[:, 0:3] = vi[:3, 3]
    rays[:, 3] = 0.001
    rays[:, 4:7] = d.reshape(-1, 3)
    rays[:, 7] = 10000.0
    return rays


def main():
    import numpy as np
    import torch
    from araytracingjourney_amd import renderer, scenes
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="cast", choices=["cast", "query", "frames"])
    ap.add_argument("--casts", type=int, default=20); ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400); ap.add_argument("--frames-in-flight", type=int, default=8)
    ap.add_argument("--leaf-batch", type=int, default=0); ap.add_argument("--refill", type=int, default=0); ap.add_argument("--chunk", type=int, default=0)
    a = ap.parse_args()
    sc = scenes.sponza_like(1.0)
    tuning = {"trace_leaf_batch": a.leaf_batch, "trace_refill": a.refill, "trace_chunk": a.chunk}
    extent = (1920, 1080) if a.mode == "frames" else (64, 64)
    r = renderer.renderer_for_scene(sc, extent, n_lights=1, frames_in_flight=a.frames_in_flight if a.mode == "frames" else 1, tuning=tuning)
    cam = renderer.Camera(sc.camera["pos"], sc.camera["dir"], W / H, sc.camera["fovy"], sc.camera["znear"], sc.camera["zfar"]).update_host_buffer()
    rays = {"pixel_order": primary_rays(cam)}
    rays["shuffled"] = rays["pixel_order"][np.random.default_rng(1).permutation(W * H)]
    n = W * H
    out = {"what": "cast_probe", "mode": a.mode, "scene": "sponza_like 1.0 (config 2)", "rays": n, "lib": os.environ.get("ART_LIB_PATH", "in-tree"), "tuning": tuning}
    if a.mode == "query":
        out["queries"] = {}
        for order, h in rays.items():
            ms = []
            for _ in range(a.repeats):
                t0 = time.perf_counter(); tuv, ids = r.query_closest(h); ms.append((time.perf_counter() - t0) * 1e3)
            hit = r.query_any(h)
            out["queries"][order] = {"host_ms_per_closest_query": [round(x, 2) for x in ms], "closest_hits": int((ids[:, 0] >= 0).sum()), "any_hits": int(hit.sum())}
    elif a.mode == "cast":
        s = torch.cuda.Stream()
        out["casts"] = {}
        for order, h in rays.items():
            d = torch.from_numpy(h).cuda()
            tuv = torch.empty((n, 4), dtype=torch.float32, device="cuda"); ids = torch.empty((n, 2), dtype=torch.int32, device="cuda"); hit = torch.empty((n,), dtype=torch.uint8, device="cuda")
            s.wait_stream(torch.cuda.current_stream())
            for kind, o in (("closest", (tuv, ids)), ("any", hit)):
                with torch.cuda.stream(s):
                    for _ in range(a.warmup):
                        r.cast_rays(d, kind=kind, out=o)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(a.casts):
                        r.cast_rays(d, kind=kind, out=o)
                    e1.record(s)
                s.synchronize()
                ms = e0.elapsed_time(e1) / a.casts
                out["casts"][f"{order}/{kind}"] = {"device_ms_per_cast": round(ms, 4), "mray_per_s": round(n / ms / 1e3, 1),
                                                  "hits": int((ids[:, 0] >= 0).sum().item()) if kind == "closest" else int(hit.sum().item())}
        out["counts"] = r.cast_counts()
    else:
        d = torch.from_numpy(rays["shuffled"]).cuda()
        tuv = torch.empty((n, 4), dtype=torch.float32, device="cuda"); ids = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        F = a.frames_in_flight

        def run(with_casts):
            for _ in range(3 * F):
                r.trace()
            r.sync(); r.cast_sync()
            casts = 0
            t0 = time.perf_counter()
            for f in range(a.steps):
                r.trace()
                if with_casts and f % 8 == 0:      # (a cast lasts several frames: a few stay in flight all the way, the pool is never lapped)
                    with torch.cuda.stream(s):
                        r.cast_rays(d, out=(tuv, ids)); casts += 1
            r.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            t1 = time.perf_counter(); r.cast_sync(); tail = (time.perf_counter() - t1) * 1e3
            return ms, casts, tail
        r.upload_state()
        alone = [run(False)[0] for _ in range(a.repeats)]
        beside = [run(True) for _ in range(a.repeats)]
        out["frames"] = {"extent": [1920, 1080], "frames_in_flight": F, "steps": a.steps, "fenced_ms_per_frame_alone": [round(x, 4) for x in alone],
                         "fenced_ms_per_frame_beside_casts": [round(x[0], 4) for x in beside], "casts_per_run": beside[0][1],
                         "ms_until_the_casts_were_done_after_the_frames": [round(x[2], 2) for x in beside], "counts": r.cast_counts()}
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
