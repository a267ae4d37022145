"""Host-side mirror of the reference's renderer API over the libart C ABI.

Names follow /root/reference/src/vk_renderer: `Renderer` ~ `VulkanTempleRayTracedRenderer` (renderer.rs:121-137:
new / add_model / prepare_first_frame / render_frame / camera_mut / lights_mut), `Camera` ~ `VkCamera`
(vk_camera.rs:128-193), `Lights`, `PointLight`, `SpotLight`, `DirectionalLight`, `AreaLight` ~ lights.rs.
All arithmetic (matrices, light records, tracing) happens inside libart; this module only marshals.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import ArtCamera, ArtConfig, ArtLight, ArtStats, check


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ------------------------------------------------------------------------------------------------ lights (lights.rs)
class PointLight:
    def __init__(self, pos, color, falloff_distance, casts_shadows):  # lights.rs:103
        self.pos, self.color, self.falloff_distance, self.casts_shadows = tuple(pos), tuple(color), float(falloff_distance), bool(casts_shadows)

    def get_light_shader_data(self) -> ArtLight:  # lights.rs:144-159
        o = ArtLight()
        check(_lib.load().art_light_point(_f3(self.pos), _f3(self.color), self.falloff_distance, int(self.casts_shadows), C.byref(o)))
        return o


class SpotLight:
    def __init__(self, pos, dir, color, falloff_distance, penumbra_umbra_angles, casts_shadows):  # lights.rs:171
        self.pos, self.dir, self.color = tuple(pos), tuple(dir), tuple(color)
        self.falloff_distance, self.penumbra_umbra_angles, self.casts_shadows = float(falloff_distance), tuple(penumbra_umbra_angles), bool(casts_shadows)

    def get_light_shader_data(self) -> ArtLight:  # lights.rs:228-243
        o = ArtLight()
        check(_lib.load().art_light_spot(_f3(self.pos), _f3(self.dir), _f3(self.color), self.falloff_distance, self.penumbra_umbra_angles[0],
                                         self.penumbra_umbra_angles[1], int(self.casts_shadows), C.byref(o)))
        return o


class DirectionalLight:
    def __init__(self, dir, color, casts_shadows):  # lights.rs:252
        self.dir, self.color, self.casts_shadows = tuple(dir), tuple(color), bool(casts_shadows)

    def get_light_shader_data(self) -> ArtLight:  # lights.rs:281-296
        o = ArtLight()
        check(_lib.load().art_light_directional(_f3(self.dir), _f3(self.color), int(self.casts_shadows), C.byref(o)))
        return o


class AreaLight:
    def __init__(self, pos, pos2, pos3, invert_normal, color, falloff_distance, penumbra_umbra_angles, casts_shadows):  # lights.rs:310
        self.pos, self.pos2, self.pos3, self.invert_normal, self.color = tuple(pos), tuple(pos2), tuple(pos3), bool(invert_normal), tuple(color)
        self.falloff_distance, self.penumbra_umbra_angles, self.casts_shadows = float(falloff_distance), tuple(penumbra_umbra_angles), bool(casts_shadows)

    def get_light_shader_data(self) -> ArtLight:  # lights.rs:383-403
        o = ArtLight()
        check(_lib.load().art_light_area(_f3(self.pos), _f3(self.pos2), _f3(self.pos3), int(self.invert_normal), _f3(self.color), self.falloff_distance,
                                         self.penumbra_umbra_angles[0], self.penumbra_umbra_angles[1], int(self.casts_shadows), C.byref(o)))
        return o


class Lights:
    """lights.rs:4-67.  Serialisation order point, spot, directional, area; unlike the reference's
    copy_lights_shader_data (lights.rs:24-47, which writes every light of a kind into one slot) each light gets
    its own slot -- identical whenever there is at most one light per kind."""

    def __init__(self):
        self.point_lights, self.spot_lights, self.directional_lights, self.area_lights = [], [], [], []

    def get_point_lights_mut(self):
        return self.point_lights

    def get_spot_lights_mut(self):
        return self.spot_lights

    def get_directional_lights_mut(self):
        return self.directional_lights

    def get_area_lights_mut(self):
        return self.area_lights

    def get_lights_count(self):
        return len(self.point_lights) + len(self.spot_lights) + len(self.directional_lights) + len(self.area_lights)

    def copy_lights_shader_data(self):
        all_ = self.point_lights + self.spot_lights + self.directional_lights + self.area_lights
        arr = (ArtLight * max(1, len(all_)))()
        for i, l in enumerate(all_):
            arr[i] = l.get_light_shader_data()
        return arr, len(all_)

    def push_dict(self, d):
        k = d["kind"]
        if k == "point":
            self.point_lights.append(PointLight(d["pos"], d["color"], d["falloff"], d["casts_shadows"]))
        elif k == "spot":
            self.spot_lights.append(SpotLight(d["pos"], d["dir"], d["color"], d["falloff"], (d["penumbra"], d["umbra"]), d["casts_shadows"]))
        elif k == "directional":
            self.directional_lights.append(DirectionalLight(d["dir"], d["color"], d["casts_shadows"]))
        elif k == "area":
            self.area_lights.append(AreaLight(d["pos"], d["pos2"], d["pos3"], d.get("invert_normal", False), d["color"], d["falloff"],
                                              (d["penumbra"], d["umbra"]), d["casts_shadows"]))
        else:
            raise ValueError(k)


# ------------------------------------------------------------------------------------------------ camera (vk_camera.rs)
class Camera:
    def __init__(self, pos, dir, aspect, fovy, znear, zfar):  # VkCamera::new, defaults renderer.rs:222-231
        self._pos, self._dir, self._aspect, self._fovy, self._znear, self._zfar = tuple(pos), tuple(dir), aspect, fovy, znear, zfar
        self.needs_update = True
        self._block = ArtCamera()

    def set_pos(self, pos):
        self._pos, self.needs_update = tuple(pos), True

    def set_dir(self, dir):
        self._dir, self.needs_update = tuple(dir), True  # normalised inside libart like vk_camera.rs:133-136

    def set_aspect(self, aspect):
        self._aspect, self.needs_update = aspect, True

    def set_fovy(self, fovy):
        self._fovy, self.needs_update = fovy, True

    def set_znear(self, znear):
        self._znear, self.needs_update = znear, True

    def set_zfar(self, zfar):
        self._zfar, self.needs_update = zfar, True

    def pos(self):
        return self._pos

    def dir(self):
        return self._dir

    def aspect(self):
        return self._aspect

    def fovy(self):
        return self._fovy

    def update_host_buffer(self) -> ArtCamera:  # vk_camera.rs:104-126
        if self.needs_update:
            check(_lib.load().art_camera_from_params(_f3(self._pos), _f3(self._dir), self._aspect, self._fovy, self._znear, self._zfar, C.byref(self._block)))
            self.needs_update = False
        return self._block

    def view_matrix(self):  # column-major 4x4 as numpy [4,4] (row, col)
        return np.array(self.update_host_buffer().view, dtype=np.float32).reshape(4, 4).T

    def perspective_matrix(self):
        return np.array(self.update_host_buffer().proj, dtype=np.float32).reshape(4, 4).T


# ------------------------------------------------------------------------------------------------ renderer (renderer.rs)
class Sphere:
    """model_reader.rs:100-146"""

    def __init__(self, center, radius):
        self.center, self.radius = np.asarray(center, np.float32), float(radius)

    def get_distance_from_point(self, point):  # model_reader.rs:124-126
        return float(np.linalg.norm(self.center - np.asarray(point, np.float32))) - self.radius

    def transform(self, m):  # model_reader.rs:128-141; m: row-major 3x4
        m = np.asarray(m, np.float32).reshape(3, 4)
        scale = max(float(np.linalg.norm(m[:, k])) for k in range(3))
        return Sphere(m[:, :3] @ self.center + m[:, 3], scale * self.radius)


def _positions_sphere(positions):
    """a model's object-space bounding sphere from its primitives' positions: the centre of their box, the farthest position from it"""
    lo = np.min([np.asarray(q)[:, :3].min(0) for q in positions], 0)
    hi = np.max([np.asarray(q)[:, :3].max(0) for q in positions], 0)
    c = 0.5 * (lo + hi)
    rad = max(float(np.linalg.norm(np.asarray(q)[:, :3] - c, axis=1).max()) for q in positions)
    return Sphere(c, rad)


STORAGE, HOST, DEVICE = "Storage", "Host", "Device"


class Model:
    """VkModel's residency state machine (vk_model.rs:280-345, states :27-275): Storage <-> Host <-> Device by the distance between the
    camera and the model's bounding sphere.  Only Device models are instanced in the acceleration structure (renderer.rs:640-651)."""

    def __init__(self, primitive_ids, sphere, reload=None, renderer=None, model_matrix=None, object_sphere=None, positions=None):
        self.primitive_ids = list(primitive_ids)
        self._positions = None if positions is None else [np.array(q, np.float32).reshape(-1, 3) for q in positions]   # object-space positions per primitive (set_vertices keeps the sphere from them)
        self.model_bounding_sphere = sphere
        self._object_sphere = object_sphere     # the reader's sphere, before any model matrix (set_model_matrix transforms THIS one)
        self._renderer = renderer               # the libart context that instances the primitives
        self.model_matrix = None if model_matrix is None else np.array(model_matrix, np.float32).reshape(3, 4)
        self.state = HOST                       # VkModel::new goes Storage -> Host (vk_model.rs:324-329)
        self.needs_cb_submit = False            # a transition to or from Device changes what the next build must contain
        self._reload = reload                   # Storage -> Host: how to read the model again (GLB path), None for in-memory models
        self._instanced = True                  # libart instances a primitive from the moment it is added

    def update_model_status(self, camera_pos):  # vk_model.rs:334-345
        d = self.model_bounding_sphere.get_distance_from_point(camera_pos)
        want = DEVICE if d <= 10.0 else (HOST if d <= 20.0 else STORAGE)
        if (want == DEVICE) != (self.state == DEVICE):
            self.needs_cb_submit = True
        self.state = want

    def set_model_matrix(self, matrix):
        """VkModel::set_model_matrix (vk_model.rs:461-466): the row-major 3x4 object -> world matrix of the model's instance, and the bounding sphere
        that goes with it.  Fixed against the reference: it transforms the sphere it HOLDS -- already transformed by the previous matrix -- by the new one
        (:463-465), so a model that is moved every frame compounds its matrices (a scale of 2 doubles the radius per call); here the reader's
        object-space sphere is transformed, which is the same for the one call the reference's main.rs makes.  The reference rebuilds its TLAS every
        frame for a moved model (renderer.rs:637-651); libart refits its structure on the device in front of the next frame (art_scene_set_model_matrix)."""
        m = np.ascontiguousarray(matrix, dtype=np.float32).reshape(3, 4)
        self.model_matrix = m.copy()
        self.model_bounding_sphere = (self._object_sphere if self._object_sphere is not None else self.model_bounding_sphere).transform(m)
        if self._renderer is not None and self.primitive_ids:
            ids = sorted(self.primitive_ids)
            runs, start = [], ids[0]                # consecutive ids travel as one call
            for a, b in zip(ids, ids[1:] + [None]):
                if b is None or b != a + 1:
                    runs.append((start, a - start + 1)); start = b
            for first, n in runs:
                check(self._renderer._L.art_scene_set_model_matrix(self._renderer._ctx, first, n, _ptr(m)))

    def set_vertices(self, primitive_index, vertices):
        """BLAS update (a BLAS built with ALLOW_UPDATE, rebuilt in MODE_UPDATE; the reference never does this: its BLAS flags are PREFER_FAST_TRACE only,
        vk_model.rs:968): primitive `primitive_ids[primitive_index]` gets new 48-byte vertices (float32 [n, 12]: position, uv, normal, tangent), its count,
        indices, texture and matrix kept.  The bounding sphere follows the new positions, made as add_model makes it (over every primitive of the model, before
        the model matrix).  On a built scene the next frame refits on the device (art_scene_set_vertices)."""
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != 12:
            raise ValueError("vertices must be float32 [n, 12] (position, uv, normal, tangent)")
        if not 0 <= primitive_index < len(self.primitive_ids):
            raise IndexError("primitive_index out of range")
        if self._positions is None:
            raise ValueError("the model's object-space positions are unknown")
        if self._renderer is not None:
            check(self._renderer._L.art_scene_set_vertices(self._renderer._ctx, self.primitive_ids[primitive_index], _ptr(v), v.shape[0]))
        self._positions[primitive_index] = v[:, :3].copy()
        self._object_sphere = _positions_sphere(self._positions)
        m = self.model_matrix if self.model_matrix is not None else np.eye(3, 4, dtype=np.float32)
        self.model_bounding_sphere = self._object_sphere.transform(m)

    def set_vertices_device(self, primitive_index, tensor, layout="full", stream=None):
        """set_vertices with the vertices in a torch tensor on the device (art_scene_set_vertices_device): no trip through the host.  layout "full": float32 [n, 12],
        contiguous and 16-byte aligned, all attributes replaced.  layout "positions": float32 [n, 3] with unit inner stride and any row stride >= 3 -- a column view of
        a wider state tensor works -- positions replaced, uv / normal / tangent kept as they currently are (shading normals go stale: recomputing them is the caller's
        business).  The library reads the tensor on `stream` (a torch stream or a raw hipStream_t; default: torch's current stream), behind whatever produced it there,
        and the call returns without waiting: work enqueued on that stream afterwards may overwrite the tensor.  The model's bounding sphere is left as it is -- the
        positions never reach the host -- so a caller that relies on the residency distances keeps it current itself."""
        import torch
        if layout not in ("full", "positions"):
            raise ValueError("layout must be 'full' or 'positions'")
        if self._renderer is None:
            raise ValueError("the model belongs to no renderer")
        dev = self._renderer._query_device()
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.device.index == dev):
            raise ValueError(f"tensor must be a torch tensor on cuda:{dev}")
        if layout == "full":
            if not (tensor.dtype == torch.float32 and tensor.dim() == 2 and tensor.shape[1] == 12 and tensor.is_contiguous() and tensor.data_ptr() % 16 == 0):
                raise ValueError("tensor must be float32 of shape (n, 12), contiguous and 16-byte aligned")
            code, stride = _lib.ART_VERTS_FULL, 0
        else:
            if not (tensor.dtype == torch.float32 and tensor.dim() == 2 and tensor.shape[1] == 3 and tensor.stride(1) == 1 and (tensor.stride(0) >= 3 or tensor.shape[0] <= 1)):
                raise ValueError("tensor must be float32 of shape (n, 3) with unit inner stride and a row stride of at least 3")
            code, stride = _lib.ART_VERTS_POSITIONS, 4 * (tensor.stride(0) if tensor.shape[0] > 1 else 3)
        if not 0 <= primitive_index < len(self.primitive_ids):
            raise IndexError("primitive_index out of range")
        u = _lib.ArtVertexUpdate(verts_dev=tensor.data_ptr() or None, hip_stream=self._renderer._stream_handle(stream, tensor.device),
                                 primitive_id=self.primitive_ids[primitive_index], n_verts=tensor.shape[0], layout=code, stride_bytes=stride, flags=0, reserved=0)
        check(self._renderer._L.art_scene_set_vertices_device(self._renderer._ctx, C.byref(u)))

    def vertices(self, primitive_index):
        """the current 48-byte vertices of primitive `primitive_ids[primitive_index]`, whichever form set them last: float32 [n, 12] (art_scene_get_vertices; waits for
        the primitive's latest set_vertices_device and reads the device copy back where that is ahead of the host's)"""
        if not 0 <= primitive_index < len(self.primitive_ids):
            raise IndexError("primitive_index out of range")
        if self._renderer is None or self._positions is None:
            raise ValueError("the model belongs to no renderer")
        out = np.empty((self._positions[primitive_index].shape[0], 12), np.float32)
        check(self._renderer._L.art_scene_get_vertices(self._renderer._ctx, self.primitive_ids[primitive_index], _ptr(out), out.shape[0]))
        return out

    def set_alpha_cutoff(self, primitive_index, cutoff):
        """Alpha-masked primitive (glTF alphaMode MASK; Vulkan: non-opaque geometry whose any-hit shader ignores the intersection when alpha < cutoff; the
        reference marks all its geometry opaque, vk_model.rs:927): a hit on primitive `primitive_ids[primitive_index]` is discarded for every ray -- primary,
        shadow, AO, queries -- where the alpha of its texture layer 0 is below `cutoff`.  0 is opaque (the default); cutoff must lie in [0, 1].  Nothing is
        built: the next frame takes it up (art_scene_set_alpha_cutoff)."""
        if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float, np.floating, np.integer)):
            raise TypeError("cutoff must be a number")
        c = float(cutoff)
        if not 0.0 <= c <= 1.0:   # (NaN too)
            raise ValueError("cutoff must lie in [0, 1]")
        if isinstance(primitive_index, bool) or not isinstance(primitive_index, (int, np.integer)):
            raise TypeError("primitive_index must be an integer")
        if not 0 <= primitive_index < len(self.primitive_ids):
            raise IndexError("primitive_index out of range")
        if self._renderer is not None:
            check(self._renderer._L.art_scene_set_alpha_cutoff(self._renderer._ctx, self.primitive_ids[primitive_index], c))

    def set_mask(self, primitive_index, mask):
        """Visibility mask (Vulkan: VkAccelerationStructureInstanceKHR.mask; the reference hard-codes 0xFF, vk_model.rs:373): a hit on primitive
        `primitive_ids[primitive_index]` is discarded for every ray whose cull mask shares no bit with `mask` (Renderer.set_ray_masks, the queries' cull_mask).
        0xFF is the default, 0 hides it from every ray; mask must lie in 0..0xFF.  Nothing is built: the next frame takes it up (art_scene_set_primitive_mask)."""
        v = _mask_value("mask", mask)
        if isinstance(primitive_index, bool) or not isinstance(primitive_index, (int, np.integer)):
            raise TypeError("primitive_index must be an integer")
        if not 0 <= primitive_index < len(self.primitive_ids):
            raise IndexError("primitive_index out of range")
        if self._renderer is not None:
            check(self._renderer._L.art_scene_set_primitive_mask(self._renderer._ctx, self.primitive_ids[primitive_index], v))

    def get_transform_model_matrix(self):           # vk_model.rs:358-363
        return None if self.model_matrix is None else self.model_matrix.copy()

    def needs_command_buffer_submission(self):
        return self.needs_cb_submit

    def reset_command_buffer_submission_status(self):
        self.needs_cb_submit = False


# the named bits of include/art.h: a convention only, the library gives bits no meaning
MASK_ALL, VIS_CAMERA, VIS_SHADOW, VIS_AO, VIS_QUERY = _lib.ART_MASK_ALL, _lib.ART_VIS_CAMERA, _lib.ART_VIS_SHADOW, _lib.ART_VIS_AO, _lib.ART_VIS_QUERY


def _mask_value(name, v):
    """an 8-bit visibility / cull mask: an integer in 0..0xFF"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer")
    if not 0 <= int(v) <= 0xFF:
        raise ValueError(f"{name} must lie in 0..0xFF")
    return int(v)


def tuning_from_dict(tuning) -> "_lib.ArtTuning":
    """an ArtTuning from a dict of its fields.  ctypes takes an unknown keyword as a plain attribute, so a misspelt or removed key would select nothing and the
    caller -- a test's form table, a sweep -- would run the default without a word: any key that is no field of ArtTuning is a ValueError that names it"""
    tuning = dict(tuning or {})
    fields = [n for n, _ in _lib.ArtTuning._fields_]
    bad = sorted(k for k in tuning if k not in fields)
    if bad:
        raise ValueError(f"tuning: unknown key{'s' if len(bad) > 1 else ''} {', '.join(repr(k) for k in bad)} (ArtTuning has {', '.join(fields)})")
    return _lib.ArtTuning(**tuning)


class Renderer:
    """VulkanTempleRayTracedRenderer (renderer.rs:121-137) on libart: same call order, no window/swapchain."""

    def __init__(self, extent, device=-1, shard=(0, 1), morton_bits=0, keep_debug=False, frames_in_flight=1, fast_build=False, packed_tiles=False, fixed_waves=False, tile_output=False, tuning=None, root_relief=0, dynamic_scene=False):
        self._L = _lib.load()
        w, h = extent
        cfg = ArtConfig(device=device, width=w, height=h, morton_bits=morton_bits, shard_rank=shard[0], shard_count=shard[1],
                        flags=(_lib.ART_FLAG_KEEP_DEBUG if keep_debug else 0) | (_lib.ART_FLAG_FAST_BUILD if fast_build else 0) | (_lib.ART_FLAG_PACKED_TILES if packed_tiles else 0) | (_lib.ART_FLAG_FIXED_WAVES if fixed_waves else 0) | (_lib.ART_FLAG_TILE_OUTPUT if tile_output else 0) | (_lib.ART_FLAG_DYNAMIC_SCENE if dynamic_scene else 0),
                        frames_in_flight=frames_in_flight, root_relief=root_relief)
        self._ctx = C.c_void_p()
        check(self._L.art_create(C.byref(cfg), C.byref(self._ctx)))
        # The host tells the library how many hardware queues it asked HIP for (libart itself reads no environment variable); `tuning` picks one of the
        # equivalent forms of the path (ArtTuning: staged / per-ray frames, host-built tree, wave-plan targets ...) -- tests and sweeps only.
        t = tuning_from_dict(tuning)
        if not t.hw_queues:
            t.hw_queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0)
        check(self._L.art_set_tuning(self._ctx, C.byref(t)))
        self.extent = (w, h)
        self._device = device
        self.shard = shard
        self.packed_tiles = packed_tiles
        # defaults of renderer.rs:222-231
        self._camera = Camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), w / h, math.pi / 2, 0.1, 1000.0)
        self._lights = Lights()
        self._models = []

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.art_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # renderer.rs:346 -- the reference takes a .glb path; here a model is the list of primitives the GLB reader yields
    def add_model(self, primitives, model_matrix=None):
        ids = []
        for p in primitives:
            verts = np.ascontiguousarray(p.verts, dtype=np.float32)
            idx = np.ascontiguousarray(p.indices)
            if idx.dtype not in (np.uint16, np.uint32):
                raise TypeError("indices must be uint16 or uint32")
            tex = np.ascontiguousarray(p.tex, dtype=np.uint8)
            m = np.ascontiguousarray(model_matrix if model_matrix is not None else p.model, dtype=np.float32)
            pid = C.c_uint32()
            check(self._L.art_scene_add_primitive(self._ctx, _ptr(verts), verts.shape[0], _ptr(idx), idx.size, idx.dtype.itemsize, _ptr(tex),
                                                  tex.shape[2], tex.shape[1], _ptr(m), C.byref(pid)))
            ids.append(pid.value)
        positions = [np.asarray(p.verts)[:, :3] for p in primitives]
        sp = _positions_sphere(positions)
        mm = model_matrix if model_matrix is not None else primitives[0].model
        self._models.append(Model(ids, sp.transform(mm), renderer=self, model_matrix=mm, object_sphere=sp, positions=positions))
        return ids

    def add_model_glb(self, reader, model_matrix, alpha_mask=False):
        """renderer.rs:346 with a GltfModelReader (opened with normalize + B8G8R8A8 coercion like vk_model.rs:498-504).
        alpha_mask=True (opt-in; the reference draws every material opaque): every primitive whose material is alphaMode MASK and whose base-colour image has
        an alpha channel gets its alphaCutoff (Model.set_alpha_cutoff).  An RGB image is coerced with alpha 0 and is never masked; BLEND is drawn opaque."""
        first, n = C.c_uint32(), C.c_uint32()
        m = np.ascontiguousarray(model_matrix, dtype=np.float32)
        r = self._L.art_scene_add_glb(self._ctx, reader._h, _ptr(m), C.byref(first), C.byref(n))
        if r != 0:
            raise _lib.ArtError(r, self._L.art_glb_last_error().decode("utf-8", "replace"))
        ids = list(range(first.value, first.value + n.value))
        c, rad = reader.get_primitives_bounding_sphere()   # vk_model.rs:501, then set_model_matrix (:461-466)
        from .model_reader import VERTICES
        data, infos = reader.copy_model_data_to_ptr(VERTICES, 0)   # the positions alone (12 B a vertex), for Model.set_vertices' sphere
        positions = [data[i.mesh_buffer_offset:i.mesh_buffer_offset + i.mesh_size].view(np.float32).reshape(-1, 3) for i in infos]
        model = Model(ids, Sphere(c, rad).transform(model_matrix), renderer=self, model_matrix=model_matrix, object_sphere=Sphere(c, rad), positions=positions)
        self._models.append(model)
        if alpha_mask:
            for i in range(len(ids)):
                mode, cutoff, has_alpha = reader.primitive_alpha(i)
                if mode == 1 and has_alpha:
                    model.set_alpha_cutoff(i, min(max(cutoff, 0.0), 1.0))
        return ids

    def models_mut(self):
        return self._models

    def camera_mut(self) -> Camera:
        return self._camera

    def lights_mut(self) -> Lights:
        return self._lights

    def prepare_first_frame(self):  # renderer.rs:356: uploads + BLAS/TLAS builds
        self.update_models_status(build=False)
        check(self._L.art_scene_build(self._ctx))

    def update_models_status(self, build=True):
        """renderer.rs:637-651: every model decides its residency from the camera position; the acceleration structure is rebuilt over the
        Device models when that set changed -- by libart's refit when the models concerned were part of the last build (no build: art_scene_set_primitive_enabled),
        by art_scene_build otherwise.  Returns True when it was built again."""
        changed = False
        for m in self._models:
            m.update_model_status(self._camera.pos())
            m.reset_command_buffer_submission_status()
            if (m.state == DEVICE) != m._instanced:      # what libart holds differs from the model's state
                m._instanced = m.state == DEVICE
                for pid in m.primitive_ids:
                    check(self._L.art_scene_set_primitive_enabled(self._ctx, pid, 1 if m._instanced else 0))
                changed = True
        rebuilt = False
        if changed and build and self.needs_build():   # (a model that was part of the last build leaves / re-enters by the next frame's refit: nothing to build)
            check(self._L.art_scene_build(self._ctx))
            rebuilt = True
        return rebuilt

    def needs_build(self) -> bool:
        nb = self._L.art_scene_needs_build(self._ctx)
        if nb < 0:
            check(nb)
        return bool(nb)

    def set_stream(self, hip_stream_ptr):
        check(self._L.art_set_stream(self._ctx, C.c_void_p(hip_stream_ptr)))

    def resize(self, extent):
        check(self._L.art_resize(self._ctx, extent[0], extent[1]))
        self.extent = tuple(extent)
        self._camera.set_aspect(extent[0] / extent[1])

    def upload_state(self):
        """camera.update_host_buffer + lights.update_host_and_device_buffer (renderer.rs:374, :677)."""
        check(self._L.art_set_camera(self._ctx, C.byref(self._camera.update_host_buffer())))
        arr, n = self._lights.copy_lights_shader_data()
        check(self._L.art_set_lights(self._ctx, arr, n))

    def trace(self):
        """record + submit of lightning_layer.trace_rays (renderer.rs:679-686); asynchronous."""
        check(self._L.art_trace(self._ctx))

    def trace_ao(self, spp=16, radius=0.2 * 1.457):
        """ao_layer.compute_ao (renderer.rs:688) replaced by ray-traced AO with XeGTAO's I/O contract"""
        check(self._L.art_trace_ao(self._ctx, spp, radius))

    def read_ao(self):
        w, h = self.extent
        a = np.empty((h, w), np.uint32)
        check(self._L.art_read_ao(self._ctx, _ptr(a), a.nbytes))
        return a

    def present(self):
        """tonemap_layer.present (renderer.rs:566-615): pack like the reference's images, then LPM tonemap to BGRA8"""
        check(self._L.art_present(self._ctx))

    def read_present(self):
        w, h = self.extent
        a = np.empty((h, w, 4), np.uint8)
        check(self._L.art_read_present(self._ctx, _ptr(a), a.nbytes))
        return a

    def read_packed(self):
        w, h = self.extent
        c, n, d = np.empty((h, w), np.uint32), np.empty((h, w), np.uint32), np.empty((h, w), np.uint16)
        check(self._L.art_read_packed(self._ctx, _ptr(c), _ptr(n), _ptr(d)))
        return c, n, d

    def render_frame(self, sync=True):  # renderer.rs:371
        self.update_models_status()
        self.upload_state()
        self.trace()
        if sync:
            self.sync()

    def sync(self):
        check(self._L.art_sync(self._ctx))

    # outputs (vk_rt_lightning_shadows.rs:161-183)
    def read_color(self):
        w, h = self.extent
        a = np.empty((h, w, 4), np.float32)
        check(self._L.art_read_color(self._ctx, _ptr(a), a.nbytes))
        return a

    def read_depth(self):
        w, h = self.extent
        a = np.empty((h, w), np.float32)
        check(self._L.art_read_depth(self._ctx, _ptr(a), a.nbytes))
        return a

    def read_normal(self):
        w, h = self.extent
        a = np.empty((h, w, 4), np.float32)
        check(self._L.art_read_normal(self._ctx, _ptr(a), a.nbytes))
        return a

    def device_color(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self._L.art_device_color(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def _dev(self, which):
        """(device pointer, bytes) of the latest frame's depth / normal output (art_device_depth / art_device_normal)"""
        p, n = C.c_void_p(), C.c_size_t()
        check(getattr(self._L, "art_device_" + which)(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def device_color_tiles(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self._L.art_device_color_tiles(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bind_color_tiles(self, slot, dev_ptr, nbytes):
        check(self._L.art_bind_color_tiles(self._ctx, slot, C.c_void_p(dev_ptr) if dev_ptr else None, nbytes))

    def bind_color_tiles_pair(self, slot, dev_even, dev_odd, nbytes):
        """two tile buffers per ring slot, written alternately: the next frame of a slot does not wait for the exchange of the previous one"""
        check(self._L.art_bind_color_tiles_pair(self._ctx, slot, C.c_void_p(dev_even), C.c_void_p(dev_odd), nbytes))

    def bind_color_tiles_ring(self, slot, dev_ptrs, nbytes):
        """len(dev_ptrs) tile buffers per ring slot, written in turn (one per trip round the frame ring)"""
        arr = (C.c_void_p * len(dev_ptrs))(*dev_ptrs)
        check(self._L.art_bind_color_tiles_ring(self._ctx, slot, arr, len(dev_ptrs), nbytes))

    def set_graph_mode(self, on):
        check(self._L.art_set_graph_mode(self._ctx, int(bool(on))))

    def set_frames_per_launch(self, n):
        """n frames per art_trace launch (fused frame); a ring slot then holds n frames"""
        check(self._L.art_set_frames_per_launch(self._ctx, n))
        self.frames_per_launch = n

    def set_camera_batch(self, cameras):
        """one Camera per frame of a launch"""
        arr = (ArtCamera * len(cameras))()
        for i, cam in enumerate(cameras):
            C.memmove(C.byref(arr[i]), C.byref(cam.update_host_buffer()), C.sizeof(ArtCamera))
        check(self._L.art_set_camera_batch(self._ctx, arr, len(cameras)))

    def set_read_frame(self, b):
        check(self._L.art_set_read_frame(self._ctx, b))

    def frames_done(self, first, count):
        """host-side, non-blocking: have frames [first, first + count) (art_trace order, from 0) all finished?"""
        d = C.c_int32()
        check(self._L.art_frames_done(self._ctx, first, count, C.byref(d), None))
        return bool(d.value)

    def frames_traced(self):
        d, n = C.c_int32(), C.c_uint64()
        check(self._L.art_frames_done(self._ctx, 0, 0, C.byref(d), C.byref(n)))
        return n.value

    def frames_in_flight(self):
        f, nxt = C.c_uint32(), C.c_uint32()
        check(self._L.art_frames_in_flight(self._ctx, C.byref(f), C.byref(nxt)))
        return f.value, nxt.value

    def stream_wait_frame(self, hip_stream_ptr):
        check(self._L.art_stream_wait_frame(self._ctx, C.c_void_p(hip_stream_ptr)))

    def trace_for_stream(self, hip_stream_ptr):
        """trace() + stream_wait_frame() in one call; returns the ring slot the frame took"""
        k = C.c_uint32()
        check(self._L.art_trace_for_stream(self._ctx, C.c_void_p(hip_stream_ptr), C.byref(k)))
        return k.value

    def wait_external_event(self, hip_event_ptr):
        check(self._L.art_wait_external_event(self._ctx, C.c_void_p(hip_event_ptr)))

    def layout(self) -> dict:
        lay = _lib.ArtLayout()
        check(self._L.art_get_layout(self._ctx, C.byref(lay)))
        return {n: getattr(lay, n) for n, _ in lay._fields_ if n != "reserved"}

    def timestamp_mark(self, which):
        """device timestamp behind the most recently traced frame (mark 0 or 1)"""
        check(self._L.art_timestamp_mark(self._ctx, which))

    def timestamp_elapsed_ms(self):
        ms = C.c_float()
        check(self._L.art_timestamp_elapsed(self._ctx, C.byref(ms)))
        return ms.value

    def collect_timings(self):
        sums = (C.c_float * 5)()
        n = C.c_uint32()
        check(self._L.art_collect_timings(self._ctx, sums, C.byref(n)))
        names = ("primary_ms", "shade_ms", "shadow_ms", "accumulate_ms", "frame_ms")
        k = max(1, n.value)
        return {nm: sums[i] / k for i, nm in enumerate(names)}, n.value

    def read_color_tiles(self):
        _, padded = self.shard_tile_count()
        a = np.empty((padded, 32, 32), np.uint32) if self.packed_tiles else np.empty((padded, 32, 32, 3), np.float32)   # RGB32F: the colour without its constant alpha
        check(self._L.art_read_color_tiles(self._ctx, _ptr(a), a.nbytes))
        return a

    def shard_tile_count(self):
        o, pd = C.c_uint32(), C.c_uint32()
        check(self._L.art_shard_tile_count(self._ctx, C.byref(o), C.byref(pd)))
        return o.value, pd.value

    def untile_gathered(self, gathered_dev_ptr, shard_count, frame_dev_ptr=None, hip_stream_ptr=None, shard_stride_tiles=None, n_frames=None):
        if n_frames is not None:   # several consecutive ring slots in one launch; frame_dev_ptr: n_frames images back to back
            check(self._L.art_untile_gathered_frames(self._ctx, C.c_void_p(gathered_dev_ptr), shard_count, shard_stride_tiles, n_frames,
                                                     C.c_void_p(frame_dev_ptr) if frame_dev_ptr else None, C.c_void_p(hip_stream_ptr) if hip_stream_ptr else None))
            return
        if shard_stride_tiles is not None:
            check(self._L.art_untile_gathered_strided(self._ctx, C.c_void_p(gathered_dev_ptr), shard_count, shard_stride_tiles,
                                                      C.c_void_p(frame_dev_ptr) if frame_dev_ptr else None, C.c_void_p(hip_stream_ptr) if hip_stream_ptr else None))
            return
        check(self._L.art_untile_gathered(self._ctx, C.c_void_p(gathered_dev_ptr), shard_count, C.c_void_p(frame_dev_ptr) if frame_dev_ptr else None,
                                          C.c_void_p(hip_stream_ptr) if hip_stream_ptr else None))

    def stats(self) -> dict:
        st = ArtStats()
        check(self._L.art_get_stats(self._ctx, C.byref(st)))
        return st.as_dict()

    # parity / debug surface
    def read_hits(self):
        w, h = self.extent
        tuv = np.empty((h, w, 4), np.float32)
        ids = np.empty((h, w, 2), np.int32)
        check(self._L.art_read_hits(self._ctx, _ptr(tuv), _ptr(ids), w * h))
        return tuv, ids

    def read_shadow_bits(self):
        w, h = self.extent
        b = np.empty((h, w), np.uint32)
        check(self._L.art_read_shadow_bits(self._ctx, _ptr(b), w * h))
        return b

    def read_shadow_hints(self):
        """the context's table of shadow-occluder hints (art_read_shadow_hints): uint32 [8x8 blocks of the local pixels, 4 light slots, 4 leaf positions], 0xFFFFFFFF = none"""
        a = np.empty((self.layout()["tiles_owned"] * 16, 4, 4), np.uint32)
        check(self._L.art_read_shadow_hints(self._ctx, _ptr(a), a.size))
        return a

    def write_shadow_hints(self, table):
        """overwrite that table (art_write_shadow_hints; tests only: any content leaves every frame what it is)"""
        a = np.ascontiguousarray(table, dtype=np.uint32)
        check(self._L.art_write_shadow_hints(self._ctx, _ptr(a), a.size))

    def math_sweep(self, which, first_bits=0, count=1 << 32, stride=1):
        """art_parity_math_sweep: the shading kernels' fast paths for 1 / sqrt(x) (which 0, 2; 3 the shorter candidate, 4 the control that must fail) and sqrt(x) (1) against the plain expressions on the bit patterns
        first_bits + i * stride, i < count -> dict(mismatches, first_bad_bits (None without a mismatch), fast_lanes, guard=(lo, hi))"""
        bad, fast, first, guard = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), (C.c_float * 2)()
        check(self._L.art_parity_math_sweep(self._ctx, which, first_bits, count, stride, C.byref(bad), C.byref(first), C.byref(fast), guard))
        return dict(mismatches=bad.value, first_bad_bits=first.value if bad.value else None, fast_lanes=fast.value, guard=(guard[0], guard[1]))

    def div_sweep(self, which, first_bits=0, count=1 << 32, stride=1, numerator_bits=0x3F800000):
        """art_parity_div_sweep: the short forms of the frame kernels' once-per-wave divisions against the divisions (which 0: rcp_core(safe_dir(x)); 1: div_core(numerator, x);
        2: the control that must fail; 3: div_core over the exponent-pair set, numerator_bits the seed; 4: over the camera ray's operands)
        -> dict(mismatches, first_bad=(a bits, b bits) (None without a mismatch), short_lanes, lanes, guard=(lo, hi) of the unary form, domain=(lo, hi) of div_core's operands)"""
        bad, short, lanes, first, guard = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), (C.c_uint32 * 2)(), (C.c_float * 4)()
        check(self._L.art_parity_div_sweep(self._ctx, which, first_bits, count, stride, numerator_bits, C.byref(bad), first, C.byref(short), C.byref(lanes), guard))
        return dict(mismatches=bad.value, first_bad=(first[0], first[1]) if bad.value else None, short_lanes=short.value, lanes=lanes.value, guard=(guard[0], guard[1]), domain=(guard[2], guard[3]))

    def radiance_sweep(self, which, first_bits=0, count=1 << 32, stride=1, numerator=1.0):
        """art_parity_radiance_sweep: the albedo's x^2.2 helper against libm's powf (which 0) or numerator * rcp(x) against numerator / x (1) on the bit patterns
        first_bits + i * stride, i < count -> dict(max_ulps, worst_bits (None at distance 0), class_mismatches, first_class_bits (None without one))"""
        ulps, worst, bad, first = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        check(self._L.art_parity_radiance_sweep(self._ctx, which, first_bits, count, stride, numerator, C.byref(ulps), C.byref(worst), C.byref(bad), C.byref(first)))
        return dict(max_ulps=ulps.value, worst_bits=worst.value if ulps.value else None, class_mismatches=bad.value, first_class_bits=first.value if bad.value else None)

    @staticmethod
    def live_resources():
        """art_parity_live_resources: what libart holds in this process right now -> dict(device, pinned, events, streams (in use by contexts and MultiGpu objects),
        pooled (streams parked for the next context)).  A context that was closed has given back everything but its pooled streams."""
        out = (C.c_uint64 * 5)()
        check(_lib.load().art_parity_live_resources(out))
        return dict(zip(("device", "pinned", "events", "streams", "pooled"), (int(v) for v in out)))

    PLAN_UNWRITTEN = 0xFFFFFFFF   # what art_parity_plan leaves in every word of items_out the kernel did not write

    def parity_plan(self, order, items_in, cost, level_in, worst_in, cap, share, min_steps, fixed_steps, result_in=None):
        """art_parity_plan: one launch of k_plan on made-up buffers -> (items_out [cap, 2] uint32, level_out [n64] uint8, worst_out [n64] uint32, result [8] uint32);
        result_in: the eight words the kernel's result starts from (zeros)"""
        order, cost, worst_in = (np.ascontiguousarray(a, np.uint32) for a in (order, cost, worst_in))
        items_in, level_in = np.ascontiguousarray(items_in, np.uint32).reshape(-1, 2), np.ascontiguousarray(level_in, np.uint8)
        n256 = order.size
        if level_in.size != 4 * n256 or worst_in.size != 4 * n256 or cost.size != items_in.shape[0]:
            raise ValueError("parity_plan: level_in and worst_in hold 4 * len(order) entries, cost one per item")
        items_out, level_out, worst_out = np.zeros((max(int(cap), 1), 2), np.uint32), np.zeros(4 * n256, np.uint8), np.zeros(4 * n256, np.uint32)
        result = np.zeros(8, np.uint32) if result_in is None else np.array(result_in, np.uint32)
        assert result.size == 8
        check(self._L.art_parity_plan(self._ctx, n256, _ptr(order), _ptr(items_in), items_in.shape[0], _ptr(cost), _ptr(level_in), _ptr(worst_in), int(cap), float(share),
                                      int(min_steps), int(fixed_steps), _ptr(items_out), _ptr(level_out), _ptr(worst_out), _ptr(result)))
        return items_out, level_out, worst_out, result

    def read_wave_plan(self):
        """art_read_wave_plan: the context's wave plan as it stands (a landed plan is adopted first) -> dict(level [n64] uint8, items [n, 2] uint32 -- the table the next
        frame runs --, result [8] uint32, cur, pending, replans, cap)"""
        n, state, result = C.c_uint32(), (C.c_uint32 * 4)(), np.zeros(8, np.uint32)
        check(self._L.art_read_wave_plan(self._ctx, None, 0, None, 0, C.byref(n), None, state))
        level, items = np.zeros(self.layout()["tiles_owned"] * 16, np.uint8), np.zeros((n.value, 2), np.uint32)
        check(self._L.art_read_wave_plan(self._ctx, _ptr(level), level.size, _ptr(items), n.value, C.byref(n), _ptr(result), state))
        assert n.value == items.shape[0]
        return dict(level=level, items=items, result=result, cur=state[0], pending=bool(state[1]), replans=state[2], cap=state[3])

    def sample_wave_steps(self):
        """art_sample_wave_steps: one frame with the step-counting instance -> (items [n, 2] uint32: the table that launch ran, steps [n] uint32: what its waves counted)"""
        cap = self.layout()["tiles_owned"] * 16 * 2 + 64
        items, steps, n = np.zeros((cap, 2), np.uint32), np.zeros(cap, np.uint32), C.c_uint32()
        check(self._L.art_sample_wave_steps(self._ctx, _ptr(items), _ptr(steps), cap, C.byref(n)))
        assert n.value <= cap
        return items[:n.value].copy(), steps[:n.value].copy()

    def set_ray_masks(self, primary=0xFF, shadow=0xFF, ao=0xFF):
        """the cull masks of the rays trace() (primary, shadow) and trace_ao() (ao) cast (Vulkan: traceRayEXT's cullMask; the reference hard-codes 0xFF,
        raytrace.rgen.glsl:92,169): a ray sees a primitive iff its mask (Model.set_mask) shares a bit with the ray's.  Per-launch state like the camera: a
        frame keeps what was current at its trace().  0 is legal: such a ray sees nothing (art_set_ray_masks)."""
        p, s, a = _mask_value("primary", primary), _mask_value("shadow", shadow), _mask_value("ao", ao)
        check(self._L.art_set_ray_masks(self._ctx, p, s, a))

    # ---- queries on device buffers: one tensor check, one output rule, one stream rule (the texts are the ones callers have always seen: hosts log them) ----
    _RECORDS = (("tuv", "float32", (4,), 16), ("ids", "int32", (2,), 8))   # an output: name, dtype, the shape behind n, alignment
    _POINT = ("point", "float32", (4,), 16)
    _RESOLVE_OUTPUTS = dict(pos=4, ng=4, ns=4, uv=2, albedo=4, orm=4)   # name -> floats a record (the order of ArtHitResolve's fields)

    def _query_device(self):
        """this context's device index; created on "the current device": the one torch calls current (the same HIP runtime state), looked up once"""
        if self._device < 0:
            import torch
            self._device = torch.cuda.current_device()
        return self._device

    def _on_device(self, t, dtype, align):
        import torch
        return isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self._query_device() and t.dtype == getattr(torch, dtype) and t.is_contiguous() and \
            t.data_ptr() % align == 0

    def _dev_tensor(self, t, name, dtype, tail_shape, align, n=None, exact=False):
        """t, or ValueError: a contiguous, aligned tensor of that dtype on this context's device, of shape (any, *tail_shape) -- an input -- or (>= n, *tail_shape) -- an
        output of at least n records -- or exactly tail_shape"""
        import torch
        dev = self._query_device()
        if self._on_device(t, dtype, align) and (tuple(t.shape) == tail_shape if exact else
                                                 t.dim() == 1 + len(tail_shape) and tuple(t.shape[1:]) == tail_shape and (n is None or t.shape[0] >= n)):
            return t
        if exact:
            raise ValueError(f"out: {name} must be a contiguous {dtype} tensor on cuda:{dev} of shape {tail_shape}, {align}-byte aligned")
        if n is not None:   # (n,) for no tail, (n, 4) for one, (n, K, 4,) for two
            shape = "".join(f", {w}" for w in tail_shape) + ("," if len(tail_shape) != 1 else "")
            raise ValueError(f"out: {name} must be a contiguous torch.{dtype} tensor on cuda:{dev} of shape (>= n{shape}), {align}-byte aligned")
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == dev):
            raise ValueError(f"{name} must be a torch tensor on cuda:{dev}")
        raise ValueError(f"{name} must be {dtype} of shape (n, {tail_shape[0]}), contiguous and {align}-byte aligned")

    def _outputs(self, out, n, device, specs):
        """the tensors a query writes, one per (name, dtype, shape behind n, alignment): the caller's, of at least n records each, or new ones"""
        import torch
        if out is None:
            return tuple(torch.empty((n,) + tail, dtype=getattr(torch, dtype), device=device) for _, dtype, tail, _ in specs)
        return tuple(self._dev_tensor(t, name, dtype, tail, align, n) for t, (name, dtype, tail, align) in zip(out, specs, strict=True))

    @staticmethod
    def _stream_handle(stream, device):
        """the hipStream_t a query is enqueued on: `stream` (a torch stream or a raw handle), default torch's current stream on `device`.  torch's default stream is HIP's
        null stream, handle 0 -- which the entry points read as "the context's cast stream": hipStreamLegacy (1) names the null stream itself"""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(device)
        return int(getattr(stream, "cuda_stream", stream)) or 1

    def cast_rays(self, rays, kind="closest", cull_mask=0xFF, out=None, stream=None):
        """Trace rays that sit on the device (art_cast_rays: the application's own traceRayEXT).  rays: a torch tensor on this context's device, float32, shape (n, 8) --
        o.xyz, tmin, d.xyz, tmax -- contiguous and 16-byte aligned.  kind "closest" returns (tuv, ids): (n, 4) float32 t,u,v,0 -- a miss is (tmax, 0, 0, 0) -- and (n, 2) int32
        (primitive, triangle in the primitive), -1,-1 for a miss; kind "any" returns hit: (n,) uint8.  out: the tensor(s) to write -- (tuv, ids) or hit, of at least n records,
        which must not overlap the rays -- instead of new ones.  The cast is enqueued on `stream` (a torch stream or a raw hipStream_t; default: torch's current stream) and
        the call returns: no host synchronisation, the results are ordered behind the cast on that stream like those of any torch operation."""
        m = _mask_value("cull_mask", cull_mask)
        if kind not in ("closest", "any"):
            raise ValueError("kind must be 'closest' or 'any'")
        n = self._dev_tensor(rays, "rays", "float32", (8,), 16).shape[0]
        d = _lib.ArtRayCast(rays_dev=rays.data_ptr() or None, n=n, cull_mask=m, flags=0)
        if kind == "closest":
            res = tuv, ids = self._outputs(out, n, rays.device, self._RECORDS)
            d.kind, d.tuv_dev, d.ids_dev = _lib.ART_CAST_CLOSEST, tuv.data_ptr() or None, ids.data_ptr() or None
        else:
            res, = self._outputs(None if out is None else (out,), n, rays.device, (("hit", "uint8", (), 1),))
            d.kind, d.hit_dev = _lib.ART_CAST_ANY, res.data_ptr() or None
        d.hip_stream = self._stream_handle(stream, rays.device)
        check(self._L.art_cast_rays(self._ctx, C.byref(d)))
        return res

    def cast_rays_multi(self, rays, max_hits, cull_mask=0xFF, out=None, stream=None):
        """The first max_hits hits along each ray, in order (art_cast_rays_multi).  rays: as cast_rays.  Returns (tuv, ids, count): (n, K, 4) float32 t,u,v,0, (n, K, 2) int32
        (primitive, triangle in the primitive) and (n,) uint8 -- record j of ray i is its j-th hit in ascending (t, global triangle id) while j < count[i], and the miss
        record (tmax, 0, 0, 0), (-1, -1) from there on.  out: (tuv, ids, count) to write instead of new ones, of at least n rays and exactly K records a ray, not overlapping
        the rays or each other.  Enqueued on `stream` (default: torch's current stream) without host synchronisation, like cast_rays."""
        m = _mask_value("cull_mask", cull_mask)
        k = int(max_hits)
        if k != max_hits or not 1 <= k <= _lib.ART_CAST_MAX_HITS:
            raise ValueError(f"max_hits must be an integer in 1..{_lib.ART_CAST_MAX_HITS}")
        n = self._dev_tensor(rays, "rays", "float32", (8,), 16).shape[0]
        tuv, ids, count = self._outputs(out, n, rays.device, (("tuv", "float32", (k, 4), 16), ("ids", "int32", (k, 2), 8), ("count", "uint8", (), 1)))
        d = _lib.ArtRayCastMulti(rays_dev=rays.data_ptr() or None, tuv_dev=tuv.data_ptr() or None, ids_dev=ids.data_ptr() or None, count_dev=count.data_ptr() or None,
                                 n=n, max_hits=k, cull_mask=m, flags=0, hip_stream=self._stream_handle(stream, rays.device))
        check(self._L.art_cast_rays_multi(self._ctx, C.byref(d)))
        return tuv, ids, count

    def resolve_hits(self, tuv, ids, want=("pos", "ng", "ns", "uv", "albedo", "orm"), out=None, stream=None):
        """What the rays hit (art_resolve_hits): the surface attributes behind hit records.  tuv, ids: the tensors cast_rays (kind "closest") or cast_rays_multi returned --
        (n, 4) float32 / (n, 2) int32, or (n, K, 4) / (n, K, 2) -- or records of the caller's own making in that layout.  Returns a dict with one float32 tensor per name in
        `want`, shaped like the records ((n, w) or (n, K, w)): pos (w 4: world position, w = 1 resolved / 0 miss), ng (4: geometric normal by winding, w 0), ns (4: the
        frame's shading normal, w 0), uv (2), albedo (4: texture layer 0, r g b a in [0, 1], no gamma; a is what the alpha cutoff tests), orm (4: layer 1; y roughness,
        z metallic).  A miss record (-1, -1) -- and any record that names nothing in the built structure, or holds a non-finite u or v -- gives zeros everywhere.  out: a
        dict name -> tensor to write instead of new ones (exactly the record shape).  Enqueued on `stream` (default: torch's current stream) without host
        synchronisation, behind the cast that wrote the records when that ran on the same stream.

        Transparency the caller composites itself, without a host copy of any scene data:
            tuv, ids, count = r.cast_rays_multi(rays, 4)
            a = r.resolve_hits(tuv, ids, want=("albedo",))["albedo"][..., 3]          # (n, 4): alpha of every surface crossed, 0 in the tail records
            through = torch.cumprod(1 - a, dim=1)[:, -1]                               # what is left of the ray behind its first four surfaces"""
        import torch
        dev = self._query_device()
        want = tuple(want)
        if not want or len(set(want)) != len(want) or any(w not in self._RESOLVE_OUTPUTS for w in want):
            raise ValueError(f"want must name one or more of {tuple(self._RESOLVE_OUTPUTS)}, each once")
        for t, (name, dtype, (width,), align) in zip((tuv, ids), self._RECORDS):   # (n, w) or (n, K, w): a check of its own
            if not (self._on_device(t, dtype, align) and t.dim() in (2, 3) and t.shape[-1] == width):
                raise ValueError(f"{name} must be a contiguous torch.{dtype} tensor on cuda:{dev} of shape (n, {width}) or (n, K, {width}), {align}-byte aligned")
        lead = tuple(tuv.shape[:-1])
        if tuple(ids.shape[:-1]) != lead:
            raise ValueError("tuv and ids must hold the same records")
        res = {}
        for name in want:
            width = self._RESOLVE_OUTPUTS[name]
            t = out[name] if out is not None and name in out else torch.empty(lead + (width,), dtype=torch.float32, device=tuv.device)
            res[name] = self._dev_tensor(t, name, "float32", lead + (width,), 4 * width, exact=True)
        d = _lib.ArtHitResolve(tuv_dev=tuv.data_ptr() or None, ids_dev=ids.data_ptr() or None, n=tuv.numel() // 4, flags=0, hip_stream=self._stream_handle(stream, tuv.device))
        for name, t in res.items():
            setattr(d, name + "_dev", t.data_ptr() or None)
        check(self._L.art_resolve_hits(self._ctx, C.byref(d)))
        return res

    def cast_surface(self, rays, cull_mask=0xFF, want=("pos", "ng", "ns", "uv", "albedo", "orm"), stream=None):
        """One closest cast and one resolve of its records on the same stream: ((tuv, ids), surface dict) -- cast_rays and resolve_hits, nothing in between."""
        tuv, ids = self.cast_rays(rays, "closest", cull_mask, stream=stream)
        return (tuv, ids), self.resolve_hits(tuv, ids, want, stream=stream)

    def closest_points(self, points, cull_mask=0xFF, out=None, stream=None):
        """The nearest surface point to each point (art_closest_points).  points: a torch tensor on this context's device, float32, shape (n, 4) -- p.xyz and the search
        radius r (inf: unbounded) -- contiguous and 16-byte aligned.  Returns (duv, ids, point): (n, 4) float32 d,u,v,0 -- the distance and the barycentrics of vertices 1
        and 2 of the nearest point -- (n, 2) int32 (primitive, triangle in the primitive) and (n, 4) float32 the point itself, w = 1.  Nothing within r (or a non-finite
        point, a NaN or negative r) is the miss record: (r, 0, 0, 0), (-1, -1) and a point of zeros.  Alpha cutoffs are not tested; primitive masks are, against cull_mask.
        out: (duv, ids, point) to write instead of new ones, of at least n records, not overlapping the points or each other.  Enqueued on `stream` (default: torch's
        current stream) without host synchronisation, like cast_rays."""
        m = _mask_value("cull_mask", cull_mask)
        n = self._dev_tensor(points, "points", "float32", (4,), 16).shape[0]
        duv, ids, point = self._outputs(out, n, points.device, (("duv", "float32", (4,), 16), self._RECORDS[1], self._POINT))
        d = _lib.ArtPointQuery(points_dev=points.data_ptr() or None, duv_dev=duv.data_ptr() or None, ids_dev=ids.data_ptr() or None, point_dev=point.data_ptr() or None,
                               n=n, cull_mask=m, flags=0, reserved=0, hip_stream=self._stream_handle(stream, points.device))
        check(self._L.art_closest_points(self._ctx, C.byref(d)))
        return duv, ids, point

    def closest_surface(self, points, cull_mask=0xFF, want=("pos", "ng", "ns", "uv", "albedo", "orm"), stream=None):
        """closest_points and one resolve of its records on the same stream: ((duv, ids, point), surface dict) -- the normal for a signed distance or a contact, the
        material under the nearest point.  Miss records resolve to zeros."""
        duv, ids, point = self.closest_points(points, cull_mask, stream=stream)
        return (duv, ids, point), self.resolve_hits(duv, ids, want, stream=stream)

    def closest_points_multi(self, points, max_hits, cull_mask=0xFF, out=None, stream=None):
        """The max_hits nearest triangles to each point (art_closest_points_multi).  points: as closest_points.  Returns (duv, ids, point, count): (n, K, 4) float32
        d,u,v,0, (n, K, 2) int32 (primitive, triangle in the primitive), (n, K, 4) float32 the nearest point of that triangle, w = 1, and (n,) uint8 -- record j of query i
        is its j-th nearest triangle in ascending (distance, global triangle id) while j < count[i], each closest_points' own record for that triangle, and the miss record
        (r, 0, 0, 0), (-1, -1) and a point of zeros from there on.  The answers are triangles, not distinct points: those that share the nearest edge or vertex all appear.
        out: (duv, ids, point, count) to write instead of new ones, of at least n queries and exactly K records a query, not overlapping the points or each other.
        Enqueued on `stream` (default: torch's current stream) without host synchronisation, like cast_rays."""
        m = _mask_value("cull_mask", cull_mask)
        k = int(max_hits)
        if k != max_hits or not 1 <= k <= _lib.ART_CAST_MAX_HITS:
            raise ValueError(f"max_hits must be an integer in 1..{_lib.ART_CAST_MAX_HITS}")
        n = self._dev_tensor(points, "points", "float32", (4,), 16).shape[0]
        duv, ids, point, count = self._outputs(out, n, points.device, (("duv", "float32", (k, 4), 16), ("ids", "int32", (k, 2), 8), ("point", "float32", (k, 4), 16),
                                                                       ("count", "uint8", (), 1)))
        d = _lib.ArtPointQueryMulti(points_dev=points.data_ptr() or None, duv_dev=duv.data_ptr() or None, ids_dev=ids.data_ptr() or None, point_dev=point.data_ptr() or None,
                                    count_dev=count.data_ptr() or None, n=n, max_hits=k, cull_mask=m, flags=0, hip_stream=self._stream_handle(stream, points.device))
        check(self._L.art_closest_points_multi(self._ctx, C.byref(d)))
        return duv, ids, point, count

    def closest_surface_multi(self, points, max_hits, cull_mask=0xFF, want=("pos", "ng", "ns", "uv", "albedo", "orm"), stream=None):
        """closest_points_multi and one resolve of its n x K records on the same stream: ((duv, ids, point, count), surface dict of (n, K, w) tensors) -- the normal of
        every face of a contact manifold.  Miss records resolve to zeros."""
        duv, ids, point, count = self.closest_points_multi(points, max_hits, cull_mask, stream=stream)
        return (duv, ids, point, count), self.resolve_hits(duv, ids, want, stream=stream)

    def overlap_boxes(self, boxes, kind="list", max_hits=8, cull_mask=0xFF, out=None, stream=None):
        """The triangles that touch each box (art_overlap_boxes).  boxes: a torch tensor on this context's device, float32, shape (n, 8) -- lo.xyz, -, hi.xyz, - (words 3
        and 7 are not read) -- contiguous and 16-byte aligned; a box is closed, and touching counts.  kind "list" returns (ids, count): (n, K, 2) int32 (primitive, triangle
        in the primitive) of the K = max_hits overlapping triangles with the smallest global ids, in ascending order, (-1, -1) behind them, and (n,) int32 the number of ALL
        overlapping triangles of the box, not capped by K (a uint32 on the device, handed out as the int32 torch has every operation for: a count never reaches 2^31).  kind "any" returns hit:
        (n,) uint8, 1 where some triangle overlaps; max_hits is not used.  A box with a non-finite coordinate or lo > hi on an axis overlaps nothing.  Alpha cutoffs are not
        tested; primitive masks are, against cull_mask.  out: (ids, count) or hit to write instead of new ones, of at least n boxes and exactly K records a box, not
        overlapping the boxes or each other.  Enqueued on `stream` (default: torch's current stream) without host synchronisation, like cast_rays."""
        return self._overlap(self._L.art_overlap_boxes, _lib.ArtBoxQuery, "boxes_dev", boxes, "boxes", 8, kind, max_hits, cull_mask, out, stream)

    def _overlap(self, entry, desc, field, queries, name, width, kind, max_hits, cull_mask, out, stream):
        """overlap_boxes and overlap_triangles behind their docstrings: the checks, the outputs and the call -- the two descriptors differ in their first field's name"""
        m = _mask_value("cull_mask", cull_mask)
        if kind not in ("list", "any"):
            raise ValueError("kind must be 'list' or 'any'")
        k = 0
        if kind == "list":
            k = int(max_hits)
            if k != max_hits or not 1 <= k <= _lib.ART_CAST_MAX_HITS:
                raise ValueError(f"max_hits must be an integer in 1..{_lib.ART_CAST_MAX_HITS}")
        n = self._dev_tensor(queries, name, "float32", (width,), 16).shape[0]
        d = desc(n=n, max_hits=k, cull_mask=m, flags=0, reserved=0)
        setattr(d, field, queries.data_ptr() or None)
        if kind == "list":
            res = ids, count = self._outputs(out, n, queries.device, (("ids", "int32", (k, 2), 8), ("count", "int32", (), 4)))
            d.kind, d.ids_dev, d.count_dev = _lib.ART_OVERLAP_LIST, ids.data_ptr() or None, count.data_ptr() or None
        else:
            res, = self._outputs(None if out is None else (out,), n, queries.device, (("hit", "uint8", (), 1),))
            d.kind, d.hit_dev = _lib.ART_OVERLAP_ANY, res.data_ptr() or None
        d.hip_stream = self._stream_handle(stream, queries.device)
        check(entry(self._ctx, C.byref(d)))
        return res

    def overlap_triangles(self, tris, kind="list", max_hits=8, cull_mask=0xFF, out=None, stream=None):
        """The scene triangles that touch each query triangle (art_overlap_triangles; DESIGN.md 3.13 is the definition).  tris: a torch tensor on this context's device,
        float32, shape (n, 12) -- q0.xyz, -, q1.xyz, -, q2.xyz, - (words 3, 7 and 11 are not read) -- contiguous and 16-byte aligned.  Every test is closed: touching
        counts, also at one vertex; coplanar triangles apart from each other are apart.  A SURFACE test: a query wholly inside a closed mesh touches nothing
        (points_inside on one vertex answers containment).  kind "list" returns (ids, count): (n, K, 2) int32 (primitive, triangle in the primitive) of the K = max_hits
        overlapping triangles with the smallest global ids, in ascending order, (-1, -1) behind them, and (n,) int32 the number of ALL overlapping triangles of the query,
        not capped by K (a uint32 on the device, handed out as int32, as overlap_boxes').  kind "any" returns hit: (n,) uint8, 1 where some triangle overlaps; max_hits is
        not used.  A query with a non-finite coordinate overlaps nothing; a segment or a point (equal vertices) goes through the same formulas.  Alpha cutoffs are not
        tested; primitive masks are, against cull_mask.  out: (ids, count) or hit to write instead of new ones, of at least n queries and exactly K records a query, not
        overlapping the queries or each other.  Every tensor is checked before anything is enqueued.  Enqueued on `stream` (default: torch's current stream) without
        host synchronisation, like cast_rays."""
        return self._overlap(self._L.art_overlap_triangles, _lib.ArtTriQuery, "tris_dev", tris, "tris", 12, kind, max_hits, cull_mask, out, stream)

    def collide_mesh(self, positions, indices, model_matrix=None, kind="any", max_hits=8, cull_mask=0xFF, stream=None):
        """Does this mesh, where it stands, cut the scene's surfaces, and which triangles does it cut?  positions: (V, 3) float32 and indices: (T, 3) int32 or int64,
        contiguous torch tensors on this context's device; model_matrix: a row-major 3x4 (12 floats, rows of x y z and the translation; None: the positions as they
        are).  The (T, 12) query buffer is gathered on the device, on `stream`: vertex k of triangle t is positions[indices[t, k]], through the matrix as
        ((p.x * m[r][0] + p.y * m[r][1]) + p.z * m[r][2]) + m[r][3] in float32 for each row r; a triangle with an index outside positions becomes a dead query (NaN
        coordinates: it touches nothing).  The answer is overlap_triangles of that buffer and nothing else: kind "any" returns hit, (T,) uint8; kind "list" returns
        (ids, count), (T, K, 2) int32 and (T,) int32 -- per triangle of the mesh, in the order of indices.  hit.any() is "the mesh collides".  No host synchronisation."""
        _mask_value("cull_mask", cull_mask)
        if kind not in ("list", "any"):
            raise ValueError("kind must be 'list' or 'any'")
        import torch
        tris, stream = self._mesh_tris(positions, indices, model_matrix, stream)
        with torch.cuda.stream(stream):   # (the outputs are torch's allocations on the stream that writes them)
            return self.overlap_triangles(tris, kind, max_hits, cull_mask, stream=stream)

    def closest_triangles(self, tris, cull_mask=0xFF, out=None, stream=None):
        """The distance from each query triangle to the scene, and where (art_closest_triangles; DESIGN.md 3.14 is the definition).  tris: a torch tensor on this context's
        device, float32, shape (n, 12) -- q0.xyz, r, q1.xyz, -, q2.xyz, - (word 3 is the query's search radius, inf: unbounded; words 7 and 11 are not read) --
        contiguous and 16-byte aligned: a buffer of overlap_triangles' queries with the radius written into column 3.  Returns (duv, ids, point, qpoint): (n, 4) float32
        d,u,v,0 -- the distance and the barycentrics of vertices 1 and 2 of the witness point on the scene triangle -- (n, 2) int32 (primitive, triangle in the
        primitive), (n, 4) float32 that point, w = 1, and (n, 4) float32 the witness point on the query triangle, w = 1.  A pair that touches or cuts has d = 0; its two
        points are the nearest features' and need not coincide (overlap_triangles says which triangles cut, this says the clearance is 0).  Nothing within r (or a
        non-finite coordinate, a NaN or negative r) is the miss record: (r, 0, 0, 0), (-1, -1) and points of zeros.  Alpha cutoffs are not tested; primitive masks are,
        against cull_mask.  out: (duv, ids, point, qpoint) to write instead of new ones, of at least n records, not overlapping the queries or each other.  Every tensor
        is checked before anything is enqueued.  Enqueued on `stream` (default: torch's current stream) without host synchronisation, like cast_rays."""
        m = _mask_value("cull_mask", cull_mask)
        n = self._dev_tensor(tris, "tris", "float32", (12,), 16).shape[0]
        duv, ids, point, qpoint = self._outputs(out, n, tris.device, (("duv", "float32", (4,), 16), self._RECORDS[1], self._POINT, ("qpoint", "float32", (4,), 16)))
        d = _lib.ArtTriDistance(tris_dev=tris.data_ptr() or None, duv_dev=duv.data_ptr() or None, ids_dev=ids.data_ptr() or None, point_dev=point.data_ptr() or None,
                                qpoint_dev=qpoint.data_ptr() or None, n=n, cull_mask=m, flags=0, reserved=0, hip_stream=self._stream_handle(stream, tris.device))
        check(self._L.art_closest_triangles(self._ctx, C.byref(d)))
        return duv, ids, point, qpoint

    def mesh_clearance(self, positions, indices, model_matrix=None, radius=float("inf"), cull_mask=0xFF, stream=None):
        """How far is this mesh, where it stands, from the scene's surfaces, and where?  positions, indices, model_matrix: collide_mesh's, gathered the same way on the
        device -- one closest_triangles query per triangle of the mesh, each with the search radius `radius` (a float >= 0, inf: unbounded; a triangle with an index outside
        positions is a dead query).  Returns (records, nearest): records = closest_triangles' (duv, ids, point, qpoint) per triangle, in the order of indices; nearest = a
        dict of tensors reduced on the device from them -- distance () float32, the smallest d of the triangles that have an answer; index () int64, the mesh triangle it
        belongs to, the lowest among equals; ids (2,) int32; point (4,) and qpoint (4,) float32, that record's.  Nothing within radius of any triangle (or no triangle):
        distance = radius, index = -1, ids (-1, -1), points of zeros.  distance == 0 is "the mesh touches or cuts the scene".  No host synchronisation."""
        import torch
        _mask_value("cull_mask", cull_mask)
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a float >= 0 (inf: unbounded)")
        tris, stream = self._mesh_tris(positions, indices, model_matrix, stream)
        with torch.cuda.stream(stream):
            tris[:, 3] = radius
            duv, ids, point, qpoint = records = self.closest_triangles(tris, cull_mask, stream=stream)
            nt, dev = tris.shape[0], tris.device
            if nt == 0:
                return records, dict(distance=torch.full((), radius, dtype=torch.float32, device=dev), index=torch.full((), -1, dtype=torch.int64, device=dev),
                                     ids=torch.full((2,), -1, dtype=torch.int32, device=dev), point=torch.zeros(4, device=dev), qpoint=torch.zeros(4, device=dev))
            has = ids[:, 0] >= 0
            key = torch.where(has, duv[:, 0], torch.full_like(duv[:, 0], float("inf")))
            at = torch.where(key == key.min(), torch.arange(nt, device=dev), nt).min()   # the lowest index among equals
            any_ = has.any()
            at = torch.where(any_, at, torch.zeros_like(at))   # (no answer at all: record 0 is a miss record, which is what is handed out)
            row = at.reshape(1)   # (index_select: a 0-dim tensor as a plain index would be read back by the host)
            pick = lambda t: t.index_select(0, row)[0]   # noqa: E731
            return records, dict(distance=pick(duv)[0], index=torch.where(any_, at, torch.full_like(at, -1)), ids=pick(ids), point=pick(point), qpoint=pick(qpoint))

    def cast_triangles(self, sweeps, cull_mask=0xFF, out=None, stream=None):
        """Where each query triangle, moved along its displacement, first touches the scene (art_cast_triangles; DESIGN.md 3.15 is the definition).  sweeps: a torch tensor
        on this context's device, float32, shape (n, 16) -- q0.xyz, tmin, q1.xyz, tmax, q2.xyz, -, d.xyz, - (words 11 and 15 are not read) -- contiguous and 16-byte
        aligned.  The triangle at time t is q_m + t*d (d need not be unit); the answer is the first t with tmin <= t < tmax at which it touches a scene triangle, tmin
        itself where it touches or cuts one as it starts.  Returns (tuv, ids, point, qpoint): (n, 4) float32 t,u,v,0 -- u, v the barycentrics of vertices 1 and 2 of the
        contact on the scene triangle, a record resolve_hits takes -- (n, 2) int32 (primitive, triangle in the primitive), (n, 4) float32 that point, w = 1, and (n, 4)
        float32 the witness point on the query triangle in its REST pose, w = 1 (add t*d for the contact).  No contact (or a non-finite coordinate or displacement, a NaN
        tmax) is the miss record: (tmax, 0, 0, 0), (-1, -1) and points of zeros.  d = 0 is legal: only a triangle that touches as it stands answers.  Two coplanar
        triangles that slide within their common plane are seen only where they touch at tmin.  Alpha cutoffs are not tested; primitive masks are, against cull_mask.
        out: (tuv, ids, point, qpoint) to write instead of new ones, of at least n records, not overlapping the queries or each other.  Every tensor is checked before
        anything is enqueued.  Enqueued on `stream` (default: torch's current stream) without host synchronisation, like cast_rays."""
        m = _mask_value("cull_mask", cull_mask)
        n = self._dev_tensor(sweeps, "sweeps", "float32", (16,), 16).shape[0]
        tuv, ids, point, qpoint = self._outputs(out, n, sweeps.device, (self._RECORDS[0], self._RECORDS[1], self._POINT, ("qpoint", "float32", (4,), 16)))
        d = _lib.ArtTriCast(sweeps_dev=sweeps.data_ptr() or None, tuv_dev=tuv.data_ptr() or None, ids_dev=ids.data_ptr() or None, point_dev=point.data_ptr() or None,
                            qpoint_dev=qpoint.data_ptr() or None, n=n, cull_mask=m, flags=0, reserved=0, hip_stream=self._stream_handle(stream, sweeps.device))
        check(self._L.art_cast_triangles(self._ctx, C.byref(d)))
        return tuv, ids, point, qpoint

    def sweep_mesh(self, positions, indices, direction, model_matrix=None, tmin=0.0, tmax=1.0, cull_mask=0xFF, stream=None):
        """How far can this mesh move along `direction` before it touches the scene's surfaces, and where?  positions, indices, model_matrix: collide_mesh's, gathered the
        same way on the device -- one cast_triangles query per triangle of the mesh, each with the displacement `direction` (3 finite floats, world space, not through
        the matrix; need not be unit) and the limits tmin, tmax (floats; tmax inf: unbounded; a triangle with an index outside positions is a dead query).  Returns
        (records, first): records = cast_triangles' (tuv, ids, point, qpoint) per triangle, in the order of indices; first = a dict of tensors reduced on the device from
        them -- t () float32, the smallest t of the triangles that have an answer: the mesh is free to move by t*direction; index () int64, the mesh triangle it belongs
        to, the lowest among equals; ids (2,) int32; point (4,) and qpoint (4,) float32, that record's.  No contact of any triangle (or no triangle): t = tmax,
        index = -1, ids (-1, -1), points of zeros.  No host synchronisation."""
        import torch
        _mask_value("cull_mask", cull_mask)
        dirn = np.asarray(direction.cpu() if isinstance(direction, torch.Tensor) else direction, np.float32).reshape(-1)
        if dirn.size != 3 or not np.isfinite(dirn).all():
            raise ValueError("direction must be 3 finite floats")
        tmin, tmax = float(tmin), float(tmax)
        if tmax != tmax:
            raise ValueError("tmax must not be NaN")
        tris, stream = self._mesh_tris(positions, indices, model_matrix, stream)
        with torch.cuda.stream(stream):
            nt, dev = tris.shape[0], tris.device
            sweeps = torch.zeros((nt, 16), dtype=torch.float32, device=dev)
            sweeps[:, 0:12] = tris
            sweeps[:, 3], sweeps[:, 7] = tmin, tmax
            sweeps[:, 12], sweeps[:, 13], sweeps[:, 14] = float(dirn[0]), float(dirn[1]), float(dirn[2])
            tuv, ids, point, qpoint = records = self.cast_triangles(sweeps, cull_mask, stream=stream)
            if nt == 0:
                return records, dict(t=torch.full((), tmax, dtype=torch.float32, device=dev), index=torch.full((), -1, dtype=torch.int64, device=dev),
                                     ids=torch.full((2,), -1, dtype=torch.int32, device=dev), point=torch.zeros(4, device=dev), qpoint=torch.zeros(4, device=dev))
            has = ids[:, 0] >= 0
            key = torch.where(has, tuv[:, 0], torch.full_like(tuv[:, 0], float("inf")))
            at = torch.where(key == key.min(), torch.arange(nt, device=dev), nt).min()   # the lowest index among equals (mesh_clearance's reduction)
            any_ = has.any()
            at = torch.where(any_, at, torch.zeros_like(at))   # (no answer at all: record 0 is a miss record, which is what is handed out)
            row = at.reshape(1)
            pick = lambda t: t.index_select(0, row)[0]   # noqa: E731
            return records, dict(t=pick(tuv)[0], index=torch.where(any_, at, torch.full_like(at, -1)), ids=pick(ids), point=pick(point), qpoint=pick(qpoint))

    def _mesh_tris(self, positions, indices, model_matrix, stream):
        """collide_mesh's, mesh_clearance's and sweep_mesh's gather behind their docstrings: the checks, then the (T, 12) query buffer made on the device on `stream` (words 3, 7 and 11
        are 0) -> (tris, the torch stream it was made on)"""
        import torch
        nv = self._dev_tensor(positions, "positions", "float32", (3,), 4).shape[0]
        dev = positions.device
        if not (isinstance(indices, torch.Tensor) and indices.device == dev and indices.dtype in (torch.int32, torch.int64) and indices.dim() == 2 and indices.shape[1] == 3
                and indices.is_contiguous()):
            raise ValueError(f"indices must be a contiguous int32 or int64 torch tensor on {dev} of shape (T, 3)")
        nt = indices.shape[0]
        if nt > _lib.ART_CAST_MAX_RAYS:
            raise ValueError("indices: more than ART_CAST_MAX_RAYS triangles")
        if nt and not nv:
            raise ValueError("positions: empty, with triangles to gather")
        mm = None
        if model_matrix is not None:
            mm = np.asarray(model_matrix.cpu() if isinstance(model_matrix, torch.Tensor) else model_matrix, np.float32).reshape(-1)
            if mm.size != 12 or not np.isfinite(mm).all():
                raise ValueError("model_matrix must be 12 finite floats, a row-major 3x4")
            mm = [float(x) for x in mm]
        stream = self._torch_stream(stream, dev)
        with torch.cuda.stream(stream):
            tris = torch.zeros((nt, 3, 4), dtype=torch.float32, device=dev)
            if nt:
                idx = indices.to(torch.int64)
                p = positions[idx.clamp(0, nv - 1)]                                    # (T, 3, 3)
                if mm is not None:
                    x, y, z = p[..., 0], p[..., 1], p[..., 2]
                    p = torch.stack([((x * mm[4 * r] + y * mm[4 * r + 1]) + z * mm[4 * r + 2]) + mm[4 * r + 3] for r in range(3)], dim=-1)
                outside = ((idx < 0) | (idx >= nv)).any(dim=1)
                tris[..., 0:3] = torch.where(outside[:, None, None], torch.full_like(p, float("nan")), p)
        return tris.reshape(nt, 12), stream

    def voxelize(self, origin, cell, dims, cull_mask=0xFF, stream=None):
        """An occupancy grid of the scene: a uint8 tensor [nx, ny, nz] on this context's device, 1 where some triangle touches the cell (overlap_boxes, kind "any").
        origin: the grid's low corner (3 floats); cell: the cells' edge (one float, or 3); dims: (nx, ny, nz).  Cell (i, j, k) is the closed box lo = origin + idx * cell,
        hi = origin + (idx + 1) * cell, made on the device in float32 -- one product, one sum -- so neighbours share their faces bit for bit and a triangle in a shared face
        belongs to both.  Enqueued on `stream` (default: torch's current stream) without host synchronisation."""
        import torch
        m = _mask_value("cull_mask", cull_mask)
        dims = tuple(int(x) for x in dims)
        if len(dims) != 3 or any(x < 0 for x in dims):
            raise ValueError("dims must be three integers >= 0")
        dev = torch.device("cuda", self._query_device())
        org = np.asarray(origin, np.float32).reshape(-1)
        cel = np.asarray(cell, np.float32).reshape(-1)
        if org.size != 3 or cel.size not in (1, 3) or not (np.isfinite(org).all() and np.isfinite(cel).all() and (cel > 0).all()):
            raise ValueError("origin must be three finite floats and cell one or three finite floats > 0")
        cel = np.broadcast_to(cel, (3,))
        n = dims[0] * dims[1] * dims[2]
        if n > _lib.ART_CAST_MAX_RAYS:
            raise ValueError("dims: more than ART_CAST_MAX_RAYS cells")
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        elif not hasattr(stream, "cuda_stream"):
            stream = torch.cuda.ExternalStream(int(stream), device=dev)
        with torch.cuda.stream(stream):
            boxes = torch.zeros(dims + (8,), dtype=torch.float32, device=dev)
            for axis in range(3):
                shape = [1, 1, 1]
                shape[axis] = dims[axis]
                idx = torch.arange(dims[axis] + 1, dtype=torch.float32, device=dev)
                plane = idx * float(cel[axis]) + float(org[axis])   # (a product and a sum in float32, two kernels: the planes both neighbours read)
                boxes[..., axis] = plane[:-1].reshape(shape)
                boxes[..., 4 + axis] = plane[1:].reshape(shape)
            hit = self.overlap_boxes(boxes.reshape(n, 8), "any", cull_mask=m, stream=stream)
        return hit.reshape(dims)

    def cast_crossings(self, rays, cull_mask=0xFF, out=None, stream=None):
        """How many surfaces each ray enters and leaves over its whole range (art_cast_crossings).  rays: as cast_rays.  Returns cross: (n, 2) int32 (entries, exits),
        neither capped (uint32 on the device, handed out as the int32 torch has every operation for: a count never reaches 2^31).  Every triangle the ray accepts between
        tmin and tmax that the masks and the alpha cutoff let through counts once: as an entry where the ray goes against the triangle's winding normal (resolve_hits'
        ng), as an exit where it goes along it.  A dead ray is (0, 0); tmax = inf is legal.  The definition is exact, not topological: a ray through an edge two
        triangles share counts both (see points_inside).  out: the tensor to write instead of a new one, of at least n records, not overlapping the rays.  Enqueued on
        `stream` (default: torch's current stream) without host synchronisation, like cast_rays."""
        m = _mask_value("cull_mask", cull_mask)
        n = self._dev_tensor(rays, "rays", "float32", (8,), 16).shape[0]
        cross, = self._outputs(None if out is None else (out,), n, rays.device, (("cross", "int32", (2,), 8),))
        d = _lib.ArtRayCrossings(rays_dev=rays.data_ptr() or None, cross_dev=cross.data_ptr() or None, n=n, cull_mask=m, flags=0, reserved=0,
                                 hip_stream=self._stream_handle(stream, rays.device))
        check(self._L.art_cast_crossings(self._ctx, C.byref(d)))
        return cross

    # the three directions points_inside casts along, float32 as written: none parallel to an axis, a face diagonal or a body diagonal of an axis-aligned box
    INSIDE_DIRECTIONS = np.array([[0.57291365, 0.31830987, 0.75487767], [-0.43016213, 0.81649658, 0.38490018], [0.26794919, -0.61803399, -0.73908513]], np.float32)
    _INSIDE_RULES = ("parity", "winding")

    def _torch_stream(self, stream, dev):
        import torch
        if stream is None:
            return torch.cuda.current_stream(dev)
        return stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=dev)

    def points_inside(self, points, rule="parity", cull_mask=0xFF, stream=None):
        """Is each point inside the mesh?  points: a torch tensor on this context's device, float32, shape (n, 3), contiguous.  Returns (n,) uint8, 1 = inside.
        Three rays leave each point (made on the device: tmin = 0, tmax = inf) along Renderer.INSIDE_DIRECTIONS, float32
            ( 0.57291365,  0.31830987,  0.75487767)   (-0.43016213,  0.81649658,  0.38490018)   ( 0.26794919, -0.61803399, -0.73908513),
        in ONE cast_crossings of 3n rays (ray 3i + j: point i, direction j), and the answer is the majority of the three rays' verdicts:
            rule "parity"   inside iff entries + exits is odd.  Assumes a CLOSED surface; ignores winding, so it serves meshes whose faces are wound either way.  A shell
                            inside a shell is a hole.
            rule "winding"  inside iff exits > entries.  Assumes CONSISTENT OUTWARD winding (a ray from inside leaves once more than it enters); tolerates nested and
                            overlapping shells, where parity does not.
        Why three: the count is exact, not topological -- a ray through an edge two triangles share is accepted by both (the edge fattening that makes closest hits
        watertight) and counts both, which flips that ray's parity; two of three fixed, unrelated directions rarely meet such an edge for the same point.  Of the
        built-in scenes, scenes.box's faces are NOT consistently wound: in a float64 restatement over 8142 points the winding rule was wrong for it at 163 to 463 points
        a direction, parity at none; on an icosphere both rules were exact at all of 7935 points.  Hence the default.  A non-finite point is outside.
        Enqueued on `stream` (default: torch's current stream) without host synchronisation."""
        import torch
        m = _mask_value("cull_mask", cull_mask)
        if rule not in self._INSIDE_RULES:
            raise ValueError("rule must be 'parity' or 'winding'")
        n = self._dev_tensor(points, "points", "float32", (3,), 4).shape[0]
        if 3 * n > _lib.ART_CAST_MAX_RAYS:
            raise ValueError("points: more than ART_CAST_MAX_RAYS / 3")
        dev = points.device
        stream = self._torch_stream(stream, dev)
        with torch.cuda.stream(stream):
            rays = torch.zeros((n, 3, 8), dtype=torch.float32, device=dev)
            rays[:, :, 0:3] = points[:, None, :]
            rays[:, :, 4:7] = torch.from_numpy(self.INSIDE_DIRECTIONS).to(dev)[None, :, :]
            rays[:, :, 7] = float("inf")
            cross = self.cast_crossings(rays.reshape(3 * n, 8), cull_mask=m, stream=stream).reshape(n, 3, 2)
            entries, exits = cross[..., 0], cross[..., 1]
            votes = ((entries + exits) & 1) == 1 if rule == "parity" else exits > entries
            return (votes.sum(dim=1) >= 2).to(torch.uint8)

    def signed_distance(self, points, rule="parity", cull_mask=0xFF, stream=None):
        """The distance to the nearest surface, negative inside: (sd, ids, point) -- closest_points with r = inf for each of the (n, 3) float32 points, and points_inside
        (which see for `rule`) on the same stream; sd is (n,) float32, closest_points' d negated where the point is inside; ids and point are closest_points' (the
        nearest triangle and the nearest point, w = 1).  A point with no surface anywhere (an empty or fully masked scene) keeps closest_points' miss: sd = inf."""
        import torch
        m = _mask_value("cull_mask", cull_mask)
        if rule not in self._INSIDE_RULES:
            raise ValueError("rule must be 'parity' or 'winding'")
        n = self._dev_tensor(points, "points", "float32", (3,), 4).shape[0]
        stream = self._torch_stream(stream, points.device)
        with torch.cuda.stream(stream):
            q = torch.full((n, 4), float("inf"), dtype=torch.float32, device=points.device)
            q[:, 0:3] = points
            duv, ids, point = self.closest_points(q, cull_mask=m, stream=stream)
            inside = self.points_inside(points, rule, m, stream=stream)
            d = duv[:, 0]
            return torch.where(inside != 0, -d, d), ids, point

    def voxelize_solid(self, origin, cell, dims, rule="parity", cull_mask=0xFF, stream=None):
        """voxelize's occupancy grid with the interior filled: a uint8 tensor [nx, ny, nz], 1 where some triangle touches the cell (voxelize, unchanged) OR the cell's
        centre is inside the mesh (points_inside, which see for `rule`).  The centres are made on the device in float32 as origin + (idx + 0.5) * cell -- one sum, one
        product, one sum.  origin, cell, dims: as voxelize.  Enqueued on `stream` (default: torch's current stream) without host synchronisation."""
        import torch
        if rule not in self._INSIDE_RULES:
            raise ValueError("rule must be 'parity' or 'winding'")
        dev = torch.device("cuda", self._query_device())
        stream = self._torch_stream(stream, dev)
        surface = self.voxelize(origin, cell, dims, cull_mask, stream=stream)   # (checks origin, cell, dims)
        dims = tuple(surface.shape)
        org = np.asarray(origin, np.float32).reshape(-1)
        cel = np.broadcast_to(np.asarray(cell, np.float32).reshape(-1), (3,))
        n = dims[0] * dims[1] * dims[2]
        if 3 * n > _lib.ART_CAST_MAX_RAYS:
            raise ValueError("dims: more than ART_CAST_MAX_RAYS / 3 cells")
        with torch.cuda.stream(stream):
            centres = torch.zeros(dims + (3,), dtype=torch.float32, device=dev)
            for axis in range(3):
                shape = [1, 1, 1]
                shape[axis] = dims[axis]
                idx = torch.arange(dims[axis], dtype=torch.float32, device=dev)
                centres[..., axis] = ((idx + 0.5) * float(cel[axis]) + float(org[axis])).reshape(shape)
            inside = self.points_inside(centres.reshape(n, 3), rule, cull_mask, stream=stream)
            return surface | inside.reshape(dims)

    def cast_spheres(self, rays, radius, cull_mask=0xFF, out=None, stream=None):
        """Where a ball of `radius` moving along each ray first touches the scene (art_cast_spheres).  rays: cast_rays' tensor, float32 of shape (n, 8) -- o.xyz, tmin,
        d.xyz, tmax; the ball's centre is o + t*d -- contiguous and 16-byte aligned; radius: one finite float >= 0 for the whole call.  Returns (tuv, ids, point): (n, 4)
        float32 t,u,v,0 -- the centre's t at first contact and the barycentrics of vertices 1 and 2 of the contact point -- (n, 2) int32 (primitive, triangle in the
        primitive) and (n, 4) float32 the contact point, w = 1; the contact normal is normalize(o + t*d - point).  A miss (or a dead ray) is (tmax, 0, 0, 0), (-1, -1) and a
        point of zeros.  Alpha cutoffs are not tested; primitive masks are, against cull_mask.  out: (tuv, ids, point) to write instead of new ones, of at least n records,
        not overlapping the rays or each other.  Enqueued on `stream` (default: torch's current stream) without host synchronisation, like cast_rays."""
        import math
        m = _mask_value("cull_mask", cull_mask)
        radius = float(radius)
        if not (radius >= 0.0 and math.isfinite(radius)):
            raise ValueError("radius must be a finite number >= 0")
        n = self._dev_tensor(rays, "rays", "float32", (8,), 16).shape[0]
        tuv, ids, point = self._outputs(out, n, rays.device, self._RECORDS + (self._POINT,))
        d = _lib.ArtSphereCast(rays_dev=rays.data_ptr() or None, tuv_dev=tuv.data_ptr() or None, ids_dev=ids.data_ptr() or None, point_dev=point.data_ptr() or None,
                               n=n, cull_mask=m, flags=0, radius=radius, hip_stream=self._stream_handle(stream, rays.device))
        check(self._L.art_cast_spheres(self._ctx, C.byref(d)))
        return tuv, ids, point

    def cast_spheres_surface(self, rays, radius, cull_mask=0xFF, want=("pos", "ng", "ns", "uv", "albedo", "orm"), stream=None):
        """cast_spheres and one resolve of its records on the same stream: ((tuv, ids, point), surface dict) -- the surface under the contact point.  Miss records
        resolve to zeros."""
        tuv, ids, point = self.cast_spheres(rays, radius, cull_mask, stream=stream)
        return (tuv, ids, point), self.resolve_hits(tuv, ids, want, stream=stream)

    def cast_sync(self):
        """every cast enqueued so far has finished, on whichever stream (art_cast_sync)"""
        check(self._L.art_cast_sync(self._ctx))

    def vertex_update_counts(self) -> dict:
        """what Model.set_vertices_device has done in this context: kernels enqueued, host synchronisations it made itself, device copies read back into host
        copies (art_vertex_update_counts)"""
        a, b, w = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._L.art_vertex_update_counts(self._ctx, C.byref(a), C.byref(b), C.byref(w)))
        return dict(ingests=a.value, host_syncs=b.value, readbacks=w.value)

    def cast_counts(self) -> dict:
        """casts enqueued, their rays, and the host waits casts caused (art_cast_counts)"""
        a, b, w = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._L.art_cast_counts(self._ctx, C.byref(a), C.byref(b), C.byref(w)))
        return dict(casts=a.value, rays=b.value, host_waits=w.value)

    def query_closest(self, rays, cull_mask=0xFF):
        m = _mask_value("cull_mask", cull_mask)
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        tuv = np.zeros((n, 4), np.float32)
        ids = np.zeros((n, 2), np.int32)
        check(self._L.art_query_closest_masked(self._ctx, _ptr(rays), n, m, _ptr(tuv), _ptr(ids)))   # (0xFF is art_query_closest)
        return tuv, ids

    def query_any(self, rays, cull_mask=0xFF):
        m = _mask_value("cull_mask", cull_mask)
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        hit = np.zeros(n, np.uint8)
        check(self._L.art_query_any_masked(self._ctx, _ptr(rays), n, m, _ptr(hit)))   # (0xFF is art_query_any)
        return hit

    def _leaf_count(self):
        """the leaves of the built structure: the leaf references of the 4-wide records.  (Not ArtStats.num_triangles: that leaves out the triangles of primitives disabled
        since the build, whose leaves stay -- nowhere -- in every array art_get_lbvh and art_get_traversal_tree fill.)"""
        c = self.get_wide_nodes()[1][:, 24:28].view(np.int32)
        return int(((c < 0) & (c != -2 ** 31)).sum())

    def get_lbvh(self):
        T = self._leaf_count()
        NI = max(T - 1, 0)
        out = dict(leaf_gid=np.zeros(T, np.uint32), keys=np.zeros(T, np.uint64), child=np.zeros((NI, 2), np.int32), node_lo=np.zeros((NI, 3), np.float32),
                   node_hi=np.zeros((NI, 3), np.float32), leaf_lo=np.zeros((T, 3), np.float32), leaf_hi=np.zeros((T, 3), np.float32))
        check(self._L.art_get_lbvh(self._ctx, *[_ptr(out[k]) for k in ("leaf_gid", "keys", "child", "node_lo", "node_hi", "leaf_lo", "leaf_hi")]))
        return out

    def get_traversal_tree(self):
        """the tree the walks use over get_lbvh()'s leaves (binned SAH by default)"""
        NI = max(self._leaf_count() - 1, 0)
        out = dict(child=np.zeros((NI, 2), np.int32), node_lo=np.zeros((NI, 3), np.float32), node_hi=np.zeros((NI, 3), np.float32))
        check(self._L.art_get_traversal_tree(self._ctx, _ptr(out["child"]), _ptr(out["node_lo"]), _ptr(out["node_hi"])))
        return out

    def get_wide_nodes(self):
        """the 4-wide collapse the walks read: (n, 16) uint32 quantised records and (n, 32) uint32 float-box records (art_get_wide_nodes)"""
        n = C.c_uint32()
        check(self._L.art_get_wide_nodes(self._ctx, None, None, 0, C.byref(n)))
        q, f = np.zeros((n.value, 16), np.uint32), np.zeros((n.value, 32), np.uint32)
        check(self._L.art_get_wide_nodes(self._ctx, _ptr(q), _ptr(f), n.value, C.byref(n)))
        return q, f


def mgpu_shard(rank, world, dedicated=False):
    """(shard_rank, shard_count) the context of `rank` is created with (art_mgpu_shard)"""
    sr, sc = C.c_uint32(), C.c_uint32()
    check(_lib.load().art_mgpu_shard(rank, world, _lib.ART_MGPU_DEDICATED if dedicated else _lib.ART_MGPU_SHARED, C.byref(sr), C.byref(sc)))
    return sr.value, sc.value


def mgpu_unique_id() -> bytes:
    """rank 0: the job's 128-byte RCCL id, to be handed to the other ranks"""
    buf = (C.c_uint8 * _lib.ART_MGPU_ID_BYTES)()
    check(_lib.load().art_mgpu_unique_id(buf))
    return bytes(buf)


class MultiGpu:
    """The sharded frame behind the C ABI (art_mgpu_*): this rank's share traced, the tiles of a group of launches gathered by RCCL -- to rank 0
    (one gather per group), or with `spread` frame f to rank f mod world (one grouped send / receive per group) -- and un-tiled by one launch.
    `exchange` (a Python function (send_ptr, nbytes, recv_ptr, root, stream_ptr) -> None: every rank's nbytes, rank order, into recv_ptr on `root`)
    replaces RCCL for rehearsals on one GPU."""

    def __init__(self, renderer: "Renderer", rank, world, unique_id: bytes = None, dedicated=False, launches_per_gather=0, tile_buffers=0, exchange=None, spread=False):
        self._L = _lib.load()
        self.renderer, self.rank, self.world = renderer, rank, world
        cfg = _lib.ArtMgpuConfig(rank=rank, world=world, compositor=_lib.ART_MGPU_DEDICATED if dedicated else _lib.ART_MGPU_SHARED,
                                 launches_per_gather=launches_per_gather, tile_buffers=tile_buffers, transport=_lib.ART_MGPU_HOST_EXCHANGE if exchange else _lib.ART_MGPU_RCCL,
                                 roots=_lib.ART_MGPU_ROOT_SPREAD if spread else _lib.ART_MGPU_ROOT_RANK0)
        self._cb = None
        if exchange:
            def _cb(user, send, nbytes, recv, root, stream):
                try:
                    exchange(send, nbytes, recv, root, stream)
                    return 0
                except Exception:   # nothing may unwind into the C caller
                    import traceback
                    traceback.print_exc()
                    return -1
            self._cb = _lib.ArtMgpuExchangeFn(_cb)   # kept alive as long as the object
            cfg.exchange = self._cb
        idbuf = (C.c_uint8 * _lib.ART_MGPU_ID_BYTES)(*unique_id) if unique_id is not None else None
        self._h = C.c_void_p()
        check(self._L.art_mgpu_create(renderer._ctx, C.byref(cfg), idbuf, C.byref(self._h)))

    def trace(self):
        check(self._L.art_mgpu_trace(self._h))

    def flush(self):
        check(self._L.art_mgpu_flush(self._h))

    def pending(self):
        """(groups of launches whose exchange has not been submitted yet, launches of the group still open): exchanges are submitted lazily, from later
        launches or the flush"""
        g, n = C.c_uint32(), C.c_uint32()
        check(self._L.art_mgpu_pending(self._h, C.byref(g), C.byref(n)))
        return g.value, n.value

    def assert_quiescent(self, what="a control-plane collective"):
        """The rule a host with a control plane of its own must keep (a hang of round 2: rank 0 sat in the data gather of a queued group while the others
        had entered a broadcast of the control plane on the same gloo group): nothing of the data path may be outstanding when the ranks meet anywhere
        else -- flush() first."""
        g, n = self.pending()
        if g or n:
            raise RuntimeError(f"{what} while {g} group(s) of launches are queued for their exchange and {n} launch(es) wait in an open group: call flush() first")

    def counts(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(self._L.art_mgpu_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(launches_traced=a.value, gathers=b.value, launches_per_gather=c.value)

    def read_frame(self):
        """a root (rank 0; every rank with spread roots), after flush(): the most recent frame it assembled -- [h, w, 4] float32, or [h, w] uint32 B10G11R11 words with packed tiles"""
        w, h = self.renderer.extent
        a = np.empty((h, w), np.uint32) if self.renderer.packed_tiles else np.empty((h, w, 4), np.float32)
        check(self._L.art_mgpu_read_frame(self._h, _ptr(a), a.nbytes))
        return a

    def close(self):
        if getattr(self, "_h", None):
            self._L.art_mgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def renderer_for_scene(scene, extent, n_lights=None, **kw) -> Renderer:
    """Convenience used by tests and bench: the main.rs:23-66 sequence for a synthetic scene."""
    r = Renderer(extent, **kw)
    r.add_model(scene.primitives)
    cam = r.camera_mut()
    cam.set_pos(scene.camera["pos"])
    cam.set_dir(scene.camera["dir"])
    cam.set_fovy(scene.camera["fovy"])
    cam.set_znear(scene.camera["znear"])
    cam.set_zfar(scene.camera["zfar"])
    for d in (scene.lights if n_lights is None else scene.lights[:n_lights]):
        r.lights_mut().push_dict(d)
    r.prepare_first_frame()
    return r
