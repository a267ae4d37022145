#!/usr/bin/env python3
"""Ray visibility masks on config 2 (art_scene_set_primitive_mask, art_set_ray_masks): what they cost.  Three legs on the same scene, sponza_like 1.0
with a one-triangle primitive far below the floor, 1920 x 1080, one light:
  plain       nothing masked, no new entry point called: the default instances
  shadowless  the twelve banners (primitives 12..23) CAMERA | AO, rays CAMERA / SHADOW / AO: the banners are seen and cast no shadow (the filtered instances, the
              banners' leaves flagged and skipped by the shadow walks)
  forced      every primitive in sight visible to every ray, the filtered instances all the same: the far triangle carries the odd mask, so every leaf flag the frames
              meet is clear -- what the filter costs a scene that masks nothing it sees
Per leg: ms a frame over --steps frames, 8 ring slots, fenced at both ends, repeated --repeats times in turn (plain, shadowless, forced, plain, ...); medians and the
spread of the repeats.  One JSON line.  --legs plain runs on a build without the new entry points too (ART_LIB_PATH, or a checkout of an earlier commit): the
default path of two builds is compared leg by leg, alternating, against the spread of the earlier build's own repeats.
    python tools/mask_probe.py [--steps 1000] [--repeats 3] [--legs plain,shadowless,forced]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BANNERS = list(range(12, 24))
CAMERA, SHADOW, AO = 1, 2, 4


def far_triangle():
    """one small triangle far below the floor: what the forced leg puts its odd mask on"""
    import numpy as np
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
    ap.add_argument("--steps", type=int, default=1000); ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--frames-in-flight", type=int, default=8)
    ap.add_argument("--legs", default="plain,shadowless,forced")
    a = ap.parse_args()
    legs = a.legs.split(",")
    base = scenes.sponza_like(1.0)
    sc = scenes.Scene(base.name, list(base.primitives) + [far_triangle()], base.camera, base.lights)
    far = len(sc.primitives) - 1
    lights = scenes.sponza_lights(1)

    def make(leg):
        r = renderer.Renderer((1920, 1080), frames_in_flight=a.frames_in_flight)
        r.add_model(sc.primitives)
        cam = r.camera_mut()
        cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
        for d in lights:
            r.lights_mut().push_dict(d)
        r.prepare_first_frame()
        m = r.models_mut()[0]
        if leg == "shadowless":
            for i in BANNERS:
                m.set_mask(i, CAMERA | AO)
            r.set_ray_masks(CAMERA, SHADOW, AO)
        elif leg == "forced":
            m.set_mask(far, 0x80)
        r.upload_state()
        for _ in range(3 * a.frames_in_flight):
            r.trace()
        r.sync()
        return r
    ctx = {leg: make(leg) for leg in legs}   # (all legs' contexts live side by side: a repeat is 1 000 frames of each in turn)
    runs = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg in legs:
            r = ctx[leg]
            for _ in range(a.frames_in_flight):
                r.trace()
            r.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                r.trace()
            r.sync()
            runs[leg].append((time.perf_counter() - t0) * 1e3 / a.steps)
    out = {"what": "mask_probe", "scene": "sponza_like 1.0 (config 2) + a far triangle", "extent": [1920, 1080], "frames_in_flight": a.frames_in_flight, "steps": a.steps,
           "repeats": a.repeats, "lib": os.environ.get("ART_LIB_PATH", "in-tree"), "legs": {}}
    for leg in legs:
        st = ctx[leg].stats()
        v = runs[leg]
        out["legs"][leg] = {"fenced_ms_per_frame": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "spread_pct": round(100.0 * (max(v) / min(v) - 1.0), 2),
                            "hit_pixels": int(st["hit_pixels"]), "shadow_rays": int(st["shadow_rays"]), "refits": int(st["refits"]), "rebuilds": int(st["rebuilds"])}
        ctx[leg].close()
    if "plain" in legs:
        for leg in legs:
            if leg != "plain":
                out[leg + "_over_plain"] = round(out["legs"][leg]["median"] / out["legs"]["plain"]["median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
