#!/usr/bin/env python3
"""Alpha-masked primitives on config 2 (art_scene_set_alpha_cutoff): what a masked frame costs.  The twelve banners of sponza_like (primitives 12..23) get a
cut-out alpha -- a fringe along one edge and a grid of holes, about 40 % of the texels cut -- and three cases are timed on the same scene:
  masked  the banners' cutoff 0.5: the instances with the alpha test, the banners' leaves flagged
  opaque  every cutoff 0: the default instances
  forced  the banners opaque, the instances with the alpha test all the same (a one-triangle primitive far below the floor has the cutoff: every leaf flag
          the frames meet is clear -- what the test costs an opaque triangle)
Per case: ms a frame over --steps frames, 8 ring slots, fenced at both ends, and the single-frame time (trace + sync, one frame in flight, median of --single).
Then the same three cases for the AO pass of config 5 (3840 x 2160, 16 spp): ms a step (frame + art_trace_ao) minus the frame alone.  One JSON line.
    python tools/alpha_probe.py [--steps 1000] [--single 50] [--no-ao]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

BANNERS = list(range(12, 24))


def banner_alpha(tw, th):
    """alpha of a cut-out banner: a saw-tooth fringe over the last fifth of v and a grid of round holes; 0 = cut"""
    y, x = np.mgrid[0:th, 0:tw].astype(np.float64)
    u, v = (x + 0.5) / tw, (y + 0.5) / th
    fringe = v > 0.8 + 0.15 * np.abs(((u * 8.0) % 1.0) - 0.5) * 2.0
    cu, cv = (u * 4.0) % 1.0 - 0.5, (v * 5.0) % 1.0 - 0.5
    holes = (cu * cu + cv * cv) < 0.32 ** 2
    return np.where(fringe | holes, 0, 255).astype(np.uint8)


def banner_scene(sc):
    """sc with the banners' albedo alpha replaced by banner_alpha (the colours kept); the rest shared"""
    from araytracingjourney_amd import scenes
    prims = list(sc.primitives)
    for i in BANNERS:
        p = prims[i]
        tex = p.tex.copy()
        tex[0, ..., 3] = banner_alpha(tex.shape[2], tex.shape[1])
        prims[i] = type(p)(p.verts, p.indices, tex, p.model)
    return scenes.Scene(sc.name + "+cut-out banners", prims, sc.camera, sc.lights)


def far_triangle():
    """one small triangle far below the floor, alpha 255: what the forced case puts its cutoff on"""
    from araytracingjourney_amd import scenes
    mb = scenes.MeshBuilder()
    mb.add([(0, -50, 0), (0.01, -50, 0), (0, -50, 0.01)], [(0, 0), (1, 0), (0, 1)], [(0, 1, 0)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
    t = np.zeros((3, 1, 1, 4), np.uint8); t[0] = 255; t[1] = (255, 128, 0, 255); t[2] = (128, 128, 255, 255)
    return mb.finish(t)


def main():
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    from araytracingjourney_amd import renderer, scenes
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000); ap.add_argument("--single", type=int, default=50); ap.add_argument("--frames-in-flight", type=int, default=8)
    ap.add_argument("--ao-steps", type=int, default=200); ap.add_argument("--no-ao", action="store_true")
    a = ap.parse_args()
    base = banner_scene(scenes.sponza_like(1.0))
    sc = scenes.Scene(base.name, list(base.primitives) + [far_triangle()], base.camera, base.lights)
    far = len(sc.primitives) - 1
    cases = {"masked": {i: 0.5 for i in BANNERS}, "opaque": {}, "forced": {far: 0.5}}

    def make(extent, F, lights):
        r = renderer.Renderer(extent, frames_in_flight=F)
        r.add_model(sc.primitives)
        cam = r.camera_mut()
        cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
        for d in lights:
            r.lights_mut().push_dict(d)
        r.prepare_first_frame(); r.upload_state()
        return r

    out = {"what": "alpha_probe", "scene": "sponza_like 1.0 (config 2), banners 12..23 cut out", "banner_cut_fraction": round(float((banner_alpha(256, 256) == 0).mean()), 4),
           "extent": [1920, 1080], "frames_in_flight": a.frames_in_flight, "steps": a.steps, "cases": {}}
    lights = scenes.sponza_lights(1)
    for name, cut in cases.items():
        r = make((1920, 1080), a.frames_in_flight, lights)
        m = r.models_mut()[0]
        for i, c in cut.items():
            m.set_alpha_cutoff(i, c)
        for _ in range(3 * a.frames_in_flight):
            r.trace()
        r.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.trace()
        r.sync()
        fenced = (time.perf_counter() - t0) * 1e3 / a.steps
        single = []
        for _ in range(a.single):
            t0 = time.perf_counter(); r.trace(); r.sync(); single.append((time.perf_counter() - t0) * 1e3)
        st = r.stats()
        out["cases"][name] = {"fenced_ms_per_frame": round(fenced, 4), "single_frame_ms_median": round(float(np.median(single)), 4),
                              "frame_ms_device": round(float(st["frame_ms"]), 4), "hit_pixels": int(st["hit_pixels"]), "shadow_rays": int(st["shadow_rays"]),
                              "refits": int(st["refits"]), "rebuilds": int(st["rebuilds"])}
        r.close()
    c = out["cases"]
    out["masked_over_opaque"] = round(c["masked"]["fenced_ms_per_frame"] / c["opaque"]["fenced_ms_per_frame"], 4)
    out["forced_over_opaque"] = round(c["forced"]["fenced_ms_per_frame"] / c["opaque"]["fenced_ms_per_frame"], 4)
    if not a.no_ao:
        out["ao"] = {"config": "5 (3840 x 2160, 16 spp, radius 0.2914)", "steps": a.ao_steps, "cases": {}}
        for name, cut in cases.items():
            r = make((3840, 2160), a.frames_in_flight, lights)
            m = r.models_mut()[0]
            for i, cc in cut.items():
                m.set_alpha_cutoff(i, cc)
            for _ in range(2 * a.frames_in_flight):
                r.trace(); r.trace_ao(16, 0.2 * 1.457)
            r.sync()
            t0 = time.perf_counter()
            for _ in range(a.ao_steps):
                r.trace(); r.trace_ao(16, 0.2 * 1.457)
            r.sync()
            step = (time.perf_counter() - t0) * 1e3 / a.ao_steps
            t0 = time.perf_counter()
            for _ in range(a.ao_steps):
                r.trace()
            r.sync()
            frame = (time.perf_counter() - t0) * 1e3 / a.ao_steps
            out["ao"]["cases"][name] = {"ms_per_step": round(step, 4), "frame_only_ms": round(frame, 4), "ao_ms": round(step - frame, 4), "ao_rays": int(r.stats()["ao_rays"])}
            r.close()
        ac = out["ao"]["cases"]
        out["ao"]["masked_over_opaque"] = round(ac["masked"]["ao_ms"] / ac["opaque"]["ao_ms"], 4)
        out["ao"]["forced_over_opaque"] = round(ac["forced"]["ao_ms"] / ac["opaque"]["ao_ms"], 4)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    k = kernel_resources()
    pick = {"k_frame<true,true,false,false>": "_ZN3art7k_frameILb1ELb1ELb0ELb0ELb0EEEvNS_9FrameArgsE", "k_frame<true,true,false,false,ALPHA>": "_ZN3art7k_frameILb1ELb1ELb0ELb0ELb1EEEvNS_9FrameArgsE",
            "k_trace_ao": "_ZN3art10k_trace_aoILb0EEEvNS_9TraceArgsE", "k_trace_ao<ALPHA>": "_ZN3art10k_trace_aoILb1EEEvNS_9TraceArgsE"}
    out["kernels"] = {n: {f: k[m][f] for f in ("vgpr", "sgpr", "scratch", "spill_v", "spill_s", "waves_per_simd")} for n, m in pick.items() if m in k}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
