#!/usr/bin/env python3
"""Deformed meshes on config 2 (art_scene_set_vertices): ms per frame for four legs -- still, the 164 k-triangle model moving, the same model deforming, moving
and deforming -- as a 20-frame burst and as 1 000 frames fenced at both ends, 8 ring slots.  Also: the refit's device time (ArtStats.refit_ms, the model alone),
host time per art_scene_set_vertices call, the device memory the first deformation takes (versions' shading records + staging), and the register and spill counts
of both k_refit_sub instances and of k_ingest_verts from the code object.  --device: the deforming legs go through art_scene_set_vertices_device, the shapes being
tensors on the device (no staging: first_deformation_device_bytes is the shading records alone).  Either way two more legs deform the model from a DEVICE tensor a
kernel has just produced: "from device, through the host" (tensor -> .cpu() -> art_scene_set_vertices: what a caller had to do before the device form) and "from
device" (art_scene_set_vertices_device).  One JSON line.
    python tools/deform_probe.py [--frames-in-flight 8] [--steps 1000] [--burst 20] [--no-regs] [--device] [--priority-stream]"""
import argparse, ctypes as C, json, math, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from araytracingjourney_amd import renderer, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--frames-in-flight", type=int, default=8); ap.add_argument("--steps", type=int, default=1000); ap.add_argument("--burst", type=int, default=20)
ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080); ap.add_argument("--no-regs", action="store_true"); ap.add_argument("--device", action="store_true"); ap.add_argument("--priority-stream", action="store_true")
a = ap.parse_args()
if a.priority_stream:   # the torch work and the device form's kernel on a high-priority stream instead of the null stream
    torch.cuda.set_stream(torch.cuda.Stream(priority=-1))


def regs():
    """VGPRs / SGPR and VGPR spills / waves per SIMD of k_refit_sub<true> and <false> and of k_ingest_verts' two instances, as the compiler reports them for the code
    object of art_refit.hip"""
    src = os.path.join(ROOT, "araytracingjourney_amd", "csrc", "art_refit.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True, timeout=600).stderr
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            names = {"_ZN3art11k_refit_subILb1EEE": "fold", "_ZN3art11k_refit_subILb0EEE": "plain", "_ZN3art14k_ingest_vertsILi0EEE": "ingest_full", "_ZN3art14k_ingest_vertsILi1EEE": "ingest_positions"}
            cur = names.get(next((k for k in names if m.group(1).startswith(k)), None))
            if cur:
                res[cur] = {}
            continue
        if cur:
            for key, name in (("VGPRs:", "vgpr"), ("SGPRs Spill:", "sgpr_spill"), ("VGPRs Spill:", "vgpr_spill"), ("Occupancy [waves/SIMD]:", "waves"), ("ScratchSize [bytes/lane]:", "scratch"), ("LDS Size [bytes/block]:", "lds")):
                m = re.search(re.escape(key) + r" (\d+)", line)
                if m:
                    res[cur][name] = int(m.group(1))
    return res


hip = C.CDLL("libamdhip64.so")


def free_bytes():
    f, t = C.c_size_t(), C.c_size_t()
    hip.hipMemGetInfo(C.byref(f), C.byref(t))
    return f.value


sc = scenes.sponza_like(1.0)
lights = scenes.sponza_lights(1)
j = len(sc.primitives) - 1
F = a.frames_in_flight
r = renderer.Renderer((a.width, a.height), frames_in_flight=F, dynamic_scene=True, tuning={"refit_rebuild_ratio": -1.0})
r.add_model([p for i, p in enumerate(sc.primitives) if i != j]); r.add_model([sc.primitives[j]])
cam = r.camera_mut()
cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
for d in lights:
    r.lights_mut().push_dict(d)
r.prepare_first_frame(); r.upload_state()
model = r.models_mut()[1]
pid = model.primitive_ids[0]
p = sc.primitives[j]
base = np.vstack([np.asarray(p.model, np.float64).reshape(3, 4), [0, 0, 0, 1]])
poses, shapes = [], []
for i in range(8):   # a closed loop of poses and of shapes (positions breathing along their normals, normals turned)
    an = 2 * math.pi * i / 8
    ry = np.array([[math.cos(an), 0, math.sin(an), 0], [0, 1, 0, 0], [-math.sin(an), 0, math.cos(an), 0], [0, 0, 0, 1]])
    t = np.eye(4); t[:3, 3] = (0.05 * math.cos(an) - 0.05, 0.02 * math.sin(2 * an), 0.05 * math.sin(an))
    poses.append(np.ascontiguousarray((t @ ry @ base)[:3], np.float32))
    v = np.array(p.verts, np.float32, copy=True)
    f = (np.float32(0.01) * np.sin(np.float32(an) + np.float32(6.0) * v[:, 0] + np.float32(4.0) * v[:, 2])).astype(np.float32)
    v[:, 0:3] += f[:, None] * v[:, 5:8]
    shapes.append(np.ascontiguousarray(v))
L, ctx = r._L, r._ctx
set_ns = []
d_shapes = [torch.from_numpy(v).cuda() for v in shapes]   # the shapes where a skinning kernel would leave them
d_made = torch.empty_like(d_shapes[0])


def set_shape(k, how=None):
    """how: None = the form --device chooses, from ready-made vertices; "via host" / "device": the vertices are first made on the device (a kernel writes d_made)"""
    v, dv = shapes[k % len(shapes)], d_shapes[k % len(shapes)]
    t0 = time.perf_counter_ns()
    if how is not None:
        torch.mul(dv, 1.0, out=d_made)   # the producer
        dv = d_made
        if how == "via host":
            v = d_made.cpu().numpy()
    if how == "device" or (how is None and a.device):
        model.set_vertices_device(0, dv)
    else:
        rc = L.art_scene_set_vertices(ctx, pid, v.ctypes.data_as(C.c_void_p), v.shape[0])
        assert rc == 0, rc
    set_ns.append(time.perf_counter_ns() - t0)


def set_pose(k):
    rc = L.art_scene_set_model_matrix(ctx, pid, 1, poses[k % len(poses)].ctypes.data_as(C.c_void_p))
    assert rc == 0, rc


def frame(leg, k):
    if leg in ("moving", "moving+deforming"):
        set_pose(k)
    if leg in ("deforming", "moving+deforming"):
        set_shape(k)
    if leg.startswith("from device"):
        set_shape(k, "via host" if leg.endswith("through the host") else "device")
    r.trace()


for _ in range(3 * F):
    r.trace()
r.sync()
free0 = free_bytes()
set_shape(1); set_ns.clear()
r.sync()
first_deform_bytes = free0 - free_bytes()
out = {"what": "deform_probe", "scene": "sponza_like 1.0 (config 2)", "extent": [a.width, a.height], "frames_in_flight": F, "model_triangles": int(p.n_tris),
       "model_vertices": int(p.verts.shape[0]), "form": "device" if a.device else "host", "priority_stream": bool(a.priority_stream), "legs": {}}
k = 0
for leg in ("still", "moving", "deforming", "moving+deforming", "from device, through the host", "from device"):
    for _ in range(3 * F):   # settle
        frame(leg, k); k += 1
    r.sync()
    set_ns.clear()
    t0 = time.perf_counter()
    for _ in range(a.burst):
        frame(leg, k); k += 1
    r.sync()
    burst = (time.perf_counter() - t0) * 1e3 / a.burst
    t0 = time.perf_counter()
    for _ in range(a.steps):
        frame(leg, k); k += 1
    r.sync()
    fenced = (time.perf_counter() - t0) * 1e3 / a.steps
    row = {"burst_ms_per_frame": round(burst, 4), "fenced_ms_per_frame": round(fenced, 4)}
    if set_ns:
        s = np.sort(np.array(set_ns)) / 1e6
        row["set_vertices_host_ms"] = {"median": round(float(s[len(s) // 2]), 4), "p90": round(float(s[int(len(s) * 0.9)]), 4)}
    out["legs"][leg] = row
refit_alone = {}
for leg in ("moving", "deforming", "moving+deforming"):   # the refit with nothing else on the GPU
    ms = []
    for _ in range(16):
        frame(leg, k); k += 1
        r.sync()
        ms.append(r.stats()["refit_ms"])
    refit_alone[leg] = round(float(np.median(ms)), 4)
st = r.stats()
T = int(st["num_triangles"])
out["refit_device_ms_alone"] = refit_alone
out["first_deformation_device_bytes"] = int(first_deform_bytes)
out["shade_copies_bytes_formula"] = 144 * T * (min(max(2 * F, 4), 24) - 1)
out["refits"], out["rebuilds"] = st["refits"], st["rebuilds"]
out["vertex_update_counts"] = r.vertex_update_counts()
if not a.no_regs:
    kr = regs()
    out["k_refit_sub"] = {k: kr[k] for k in ("fold", "plain") if k in kr}
    out["k_ingest_verts"] = {k[7:]: kr[k] for k in ("ingest_full", "ingest_positions") if k in kr}
r.close()
print(json.dumps(out))
