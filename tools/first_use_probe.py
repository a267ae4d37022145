#!/usr/bin/env python3
"""What a fresh process pays at its first art_scene_build and its first refit (config 2, its 164 k-triangle model moved): the code objects of the builders are loaded by
art_create (build_prewarm / sah_prewarm), so neither should hold a load.  Wall clock around the calls, and the library's own figures beside them.  One JSON line; run it
several times, a process each, and alternate builds through ART_LIB_PATH.
    python tools/first_use_probe.py [--width 1920 --height 1080]"""
import argparse, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
try:
    import torch  # noqa: F401
except Exception:
    pass
from araytracingjourney_amd import renderer, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
a = ap.parse_args()
sc = scenes.sponza_like(1.0)
j = len(sc.primitives) - 1
t0 = time.perf_counter()
r = renderer.Renderer((a.width, a.height), frames_in_flight=3, tuning={"refit_rebuild_ratio": -1.0})
create_ms = (time.perf_counter() - t0) * 1e3
r.add_model([p for i, p in enumerate(sc.primitives) if i != j]); r.add_model([sc.primitives[j]])
cam = r.camera_mut()
cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
for d in scenes.sponza_lights(1):
    r.lights_mut().push_dict(d)
t0 = time.perf_counter()
r.prepare_first_frame()
first_build_wall = (time.perf_counter() - t0) * 1e3
first_build_ms = r.stats()["build_ms"]
r.upload_state()
for _ in range(6):
    r.trace()
r.sync()
model = r.models_mut()[1]
base = np.vstack([np.asarray(sc.primitives[j].model, np.float64).reshape(3, 4), [0, 0, 0, 1]])
moved = []
for i in range(1, 4):   # the first moved frame (the ring of versions, the work lists, the first refit), then two more
    t = np.eye(4); t[:3, 3] = (0.02 * i, 0.01 * math.sin(i), 0.0)
    model.set_model_matrix(np.ascontiguousarray((t @ base)[:3], np.float32))
    t0 = time.perf_counter()
    r.trace(); r.sync()
    moved.append(round((time.perf_counter() - t0) * 1e3, 3))
st = r.stats()
t0 = time.perf_counter()
r.prepare_first_frame()
second_build_wall = (time.perf_counter() - t0) * 1e3
out = {"what": "first_use_probe", "lib": os.environ.get("ART_LIB_PATH", "in-tree"), "create_ms": round(create_ms, 2), "first_build_wall_ms": round(first_build_wall, 2),
       "first_build_ms": round(first_build_ms, 3), "second_build_wall_ms": round(second_build_wall, 2), "second_build_ms": round(r.stats()["build_ms"], 3),
       "moved_frame_wall_ms": moved, "first_move_ms": round(st.get("first_move_ms", 0.0), 3), "refit_ms": round(st["refit_ms"], 4), "refits": st["refits"]}
r.close()
print(json.dumps(out))
