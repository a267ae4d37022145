import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_bindings  # noqa: E402  (the parser of the headers and gcc's layout of their structs: the one the bindings are generated with)


def oracle_for(orc, scene, n_lights=None, morton_bits=30):
    S = orc.Scene(scene.primitives, morton_bits=morton_bits)
    ls = scene.lights if n_lights is None else scene.lights[:n_lights]
    return S, orc.make_lights(ls), len(ls)


def oracle_camera(orc, scene, w, h):
    c = scene.camera
    return orc.camera_from_params(c["pos"], c["dir"], w / h, c["fovy"], c["znear"], c["zfar"])


def random_rays(n, seed, radius=2.5):
    """Deterministic rays from points on a sphere around the scene towards points near the origin."""
    k = np.arange(n, dtype=np.float64)

    def h(a):
        x = np.sin(k * a + seed * 0.618) * 43758.5453
        return x - np.floor(x)
    th, ph = h(12.9898) * 2 * np.pi, np.arccos(2 * h(78.233) - 1)
    o = radius * np.stack([np.sin(ph) * np.cos(th), np.cos(ph), np.sin(ph) * np.sin(th)], 1)
    tgt = (np.stack([h(3.1), h(5.7), h(9.3)], 1) - 0.5) * 1.5
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o
    rays[:, 3] = 0.001
    rays[:, 4:7] = d
    rays[:, 7] = 100.0
    # a third of the rays start inside the scene
    inside = (np.arange(n) % 3) == 0
    rays[inside, 0:3] = (tgt[inside] * 0.6).astype(np.float32)
    return rays


def device_to_host(ptr, nbytes):
    """bytes at a raw device pointer (art_device_*) -> numpy uint8; the process's one HIP runtime (loaded by torch / libart)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    rc = hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), nbytes, 2)   # hipMemcpyDeviceToHost
    assert rc == 0, f"hipMemcpy failed: {rc}"
    return out


def host_to_device(ptr, array):
    """the bytes of a numpy array to a raw device pointer (art_device_*): the caller has made sure nothing on the device still uses the buffer (Renderer.sync)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.ascontiguousarray(array)
    rc = hip.hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1)   # hipMemcpyHostToDevice
    assert rc == 0, f"hipMemcpy failed: {rc}"


class MadeUpFrame:
    """art_present on buffers of the test's making (tests/test_present_edges.py): a renderer with one frame in flight renders the Cornell box once at (w, h) -- which
    lays the frame out and makes the context presentable -- optionally traces AO (the AO image has no device pointer: a test uses the values the frame has,
    `self.ao`, None without AO); then present(color, normal, depth) overwrites the three outputs art_present reads through art_device_color / _normal / _depth
    (arrays of [h, w, 4], [h, w, 4] and [h, w] float32, any of them None to leave what is there) and returns (packed colour, packed normal, packed depth, BGRA8)"""

    def __init__(self, R, scene, w, h, ao_spp=None):
        self.r = R.renderer_for_scene(scene, (w, h), frames_in_flight=1)
        self.w, self.h = w, h
        self.r.render_frame(sync=False)
        if ao_spp:
            self.r.trace_ao(ao_spp)
        self.r.sync()
        self.ao = self.r.read_ao() if ao_spp else None

    def present(self, color=None, normal=None, depth=None):
        r, w, h = self.r, self.w, self.h
        r.sync()
        for a, (ptr, nbytes), shape in ((color, r.device_color(), (h, w, 4)), (normal, r._dev("normal"), (h, w, 4)), (depth, r._dev("depth"), (h, w))):
            if a is not None:
                a = np.ascontiguousarray(a, np.float32)
                assert a.shape == shape and a.nbytes == nbytes, (a.shape, shape, a.nbytes, nbytes)   # never past the buffer's end
                host_to_device(ptr, a)
        r.present()
        return r.read_packed() + (r.read_present(),)

    def close(self):
        self.r.close()


def seam_scene(scenes):
    """one quad whose uv run from -1.25 to 2.25 (and -0.75 to 1.75) under a 4 x 5 texture of unrelated texels: nearly every pixel's bilinear footprint sits on a texel boundary,
    a fifth of them on the REPEAT wrap (tests/test_oracle.py: against numpy in fp64; tests/test_gpu_parity.py: the GPU against the oracle)"""
    import math
    rng = np.random.default_rng(7)
    tw, th = 4, 5
    tex = np.zeros((3, th, tw, 4), np.uint8)
    tex[0] = rng.integers(20, 256, (th, tw, 4))                                     # albedo: unrelated texels
    tex[1, ..., 0] = 255; tex[1, ..., 1] = rng.integers(80, 230, (th, tw)); tex[1, ..., 2] = rng.integers(0, 2, (th, tw)) * 255   # occlusion, roughness, metallic
    nm = rng.normal(0, 0.35, (th, tw, 3)); nm[..., 2] = 1.0; nm /= np.linalg.norm(nm, axis=-1, keepdims=True)
    tex[2, ..., :3] = np.round((nm * 0.5 + 0.5) * 255); tex[2, ..., 3] = 255
    mb = scenes.MeshBuilder()
    mb.add([(-0.8, -0.6, 0.5), (0.8, -0.6, 0.5), (0.8, 0.6, 0.7), (-0.8, 0.6, 0.7)], [(-1.25, -0.75), (2.25, -0.75), (2.25, 1.75), (-1.25, 1.75)],
           [(0, 0, -1)] * 4, [(1, 0, 0, 1)] * 4, [0, 1, 2, 0, 2, 3])
    prim = mb.finish(tex)
    return scenes.Scene("seams", [prim], dict(pos=(0.0, 0.0, -0.6), dir=(0.0, 0.0, 1.0), fovy=math.pi / 2, znear=0.1, zfar=1000.0),
                        [dict(kind="point", pos=(0.3, -0.2, -0.3), color=(6.0, 5.0, 4.0), falloff=4.0, casts_shadows=False)])


def check_tree_arrays(lb, tr, same_as_karras_allowed=False):
    """_check_traversal_tree on arrays: lb the canonical LBVH (leaf_gid, child, leaf_lo, leaf_hi), tr a traversal tree over its leaves (child, node_lo, node_hi) --
    a device's (get_lbvh, get_traversal_tree) or a model's (tests/np_sah.py)"""
    T = lb["leaf_gid"].size
    child = tr["child"]
    assert child.shape == (T - 1, 2)
    if not same_as_karras_allowed:
        assert not np.array_equal(child, lb["child"])                                    # a different topology than Karras'
    leaves = ~child[child < 0]
    assert np.array_equal(np.sort(leaves), np.arange(T))                                 # each leaf exactly once
    inner = child[child >= 0]
    assert np.array_equal(np.sort(inner), np.arange(1, T - 1))                           # each node but the root has exactly one parent
    def boxes(ref):
        lo = np.where((ref < 0)[:, None], lb["leaf_lo"][np.where(ref < 0, ~ref, 0)], tr["node_lo"][np.where(ref < 0, 0, ref)])
        hi = np.where((ref < 0)[:, None], lb["leaf_hi"][np.where(ref < 0, ~ref, 0)], tr["node_hi"][np.where(ref < 0, 0, ref)])
        return lo, hi
    l0, h0 = boxes(child[:, 0]); l1, h1 = boxes(child[:, 1])
    assert np.array_equal(np.minimum(l0, l1).view(np.uint32), tr["node_lo"].view(np.uint32))
    assert np.array_equal(np.maximum(h0, h1).view(np.uint32), tr["node_hi"].view(np.uint32))
    depth = np.zeros(T - 1, np.int32)                                                    # pre-order layout: parents come before children
    for n in range(T - 1):
        for c in child[n]:
            if c >= 0:
                assert c > n
                depth[c] = depth[n] + 1
    assert depth.max() + 1 <= 80
    return T


def _check_traversal_tree(r, same_as_karras_allowed=False):
    """every leaf of the canonical LBVH hangs in the traversal tree exactly once, every node box is the exact min/max union of its children's boxes, the root is node 0
    (pre-order: parents before children), the depth stays inside the walks' stacks"""
    return check_tree_arrays(r.get_lbvh(), r.get_traversal_tree(), same_as_karras_allowed)


# ---- hostile inputs for the walks (tests/test_walk_edges.py): one generator per hazard ---------------------------------------------------------------------------
# the similarities every scene is run at: (scale, offset).  Powers of two and offsets of a few thousand: no intermediate of the slab test, of Moeller-Trumbore or of the
# shading leaves float32's normal range (extreme scales, where the products go denormal or overflow, are left out on purpose)
SIMILARITIES = [(1.0, (0.0, 0.0, 0.0)), (2.0 ** -10, (0.0, 0.0, 0.0)), (2.0 ** 10, (0.0, 0.0, 0.0)), (1.0, (1000.0, -2000.0, 500.0)), (1.0, (1000.3, -2000.7, 500.1))]
# [tmin, tmax] pairs a caller may hand over in a device buffer: every one has a defined answer (the oracle's; a miss record's t is tmax as given)
RANGES = [(-5.0, 100.0), (0.001, np.inf), (-np.inf, 100.0), (2.0, 1.0), (0.001, 0.0), (-3.0, -0.5), (1.0, 1.0), (-np.inf, np.inf), (np.nan, 100.0), (1e-42, 100.0)]


def _flat_scene(name, mb, camera, lights, rgb=(200, 180, 160)):
    from araytracingjourney_amd import scenes
    return scenes.Scene(name, [mb.finish(scenes.constant_texture(rgb))], camera, lights)


def lattice_coords(n=6):
    """the n + 1 plane coordinates of the lattice in [-0.75, 0.75] (n = 6: multiples of 0.25, exact)"""
    return (np.arange(n + 1, dtype=np.float64) * (1.5 / n) - 0.75).astype(np.float32)


def lattice_scene(n=6):
    """axis-aligned unit quads on every second plane of an n^3 lattice in [-0.75, 0.75]^3, a third of the cells left empty: every leaf box has zero thickness, quads share
    edges and vertices, and whole planes of them are coplanar.  The camera looks along +z through the lattice line x = y = 0; the point light sits on lattice
    coordinates (shadow rays inside quad planes), the directional one runs along an axis"""
    import math
    from araytracingjourney_amd import scenes
    g = lattice_coords(n).astype(np.float64)
    mb = scenes.MeshBuilder()
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        nrm, tan = np.zeros(3), np.zeros(4)
        nrm[axis], tan[u], tan[3] = 1.0, 1.0, 1.0
        for i in range(0, n + 1, 2):
            for j in range(n):
                for k in range(n):
                    if (axis + i // 2 + j + 2 * k) % 3 == 0:
                        continue
                    p = np.zeros((4, 3))
                    p[:, axis] = g[i]
                    p[:, u] = (g[j], g[j + 1], g[j + 1], g[j])
                    p[:, v] = (g[k], g[k], g[k + 1], g[k + 1])
                    mb.add(p, [(0, 0), (1, 0), (1, 1), (0, 1)], [nrm] * 4, [tan] * 4, [0, 1, 2, 0, 2, 3])
    camera = dict(pos=(0.0, 0.0, -2.0), dir=(0.0, 0.0, 1.0), fovy=0.9, znear=0.1, zfar=1000.0)
    lights = [dict(kind="point", pos=(0.25, 0.25, -1.0), color=(6.0, 6.0, 6.0), falloff=6.0, casts_shadows=True),
              dict(kind="directional", dir=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), casts_shadows=True)]
    return _flat_scene("lattice", mb, camera, lights)


def lattice_rays(n=6):
    """axis-parallel rays in all six directions, the two other components both +0.0 and both -0.0, through every pair of lattice and half-way coordinates: from outside
    the scene (tmin 0.001), and from ON a quad plane with tmin = 0 (13 origins on the plane's diagonal).  n = 6: 12 * (169 + 13) = 2 184 rays"""
    g = lattice_coords(n).astype(np.float64)
    c = np.sort(np.concatenate([g, 0.5 * (g[:-1] + g[1:])]))
    a, b = [x.reshape(-1) for x in np.meshgrid(c, c, indexing="ij")]
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for sgn in (1.0, -1.0):
            for zero in (0.0, -0.0):
                far = np.zeros((a.size, 8), np.float32)
                far[:, axis], far[:, u], far[:, v], far[:, 3] = -1.5 * sgn, a, b, 0.001
                on = np.zeros((c.size, 8), np.float32)
                on[:, axis], on[:, u], on[:, v], on[:, 3] = g[2], c, c, 0.0
                for r in (far, on):
                    r[:, 4 + axis], r[:, 4 + u], r[:, 4 + v], r[:, 7] = sgn, zero, zero, 100.0
                    out.append(r)
    return np.concatenate(out)


def chain_scene(n=64, w=0.01):
    """n nested slivers: triangle k is (c/2, -w, 0), (c/2, w, 0), (2c, 0, w) with c = 2^-k -- each a factor of two nearer the origin than the last, so the canonical
    (Morton) tree over them is a comb 27 levels deep at n = 64.  -> (scene, rays): rays[0] runs along +x through every box from the small end (a nearer-child-first
    binary walk holds 26 pending nodes on the canonical tree), rays[1] is the same line backwards (5), the rest a bundle of 200 round rays[0]: origins inside
    the slivers' outline (|y|, |z| < w), directions jittered by w / 2.  The scene's camera sits at (-1, w/2, w/2) looking along +x with a field of view as narrow as the boxes"""
    from araytracingjourney_amd import scenes
    mb = scenes.MeshBuilder()
    for k in range(n):
        c = 2.0 ** -k
        mb.add([(c / 2, -w, 0.0), (c / 2, w, 0.0), (2 * c, 0.0, w)], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
    rays = np.zeros((202, 8), np.float32)
    rays[:, 3], rays[:, 7], rays[:, 4] = 0.001, 100.0, 1.0
    rays[:, 0:3] = (-1.0, 0.9 * w, 0.9 * w)
    rays[1, 0], rays[1, 4] = 3.0, -1.0
    rng = np.random.default_rng(64)
    rays[2:, 2] = rng.uniform(0.0, w, 200)                                # inside the slivers' common outline in y, z: 0 < z < w, |y| < w - z
    rays[2:, 1] = rng.uniform(-1.0, 1.0, 200) * (w - rays[2:, 2])
    rays[2:, 5:7] = rng.uniform(-0.5 * w, 0.5 * w, (200, 2))   # (unnormalised directions are legal: t is in units of |d|)
    camera = dict(pos=(-1.0, 0.5 * w, 0.5 * w), dir=(1.0, 0.0, 0.0), fovy=2.0 * w, znear=0.1, zfar=1000.0)
    # both lights shine from the far end, nearly along the chain (the slivers' normals are -z: a light exactly along x would light nothing): shadow rays run through
    # the boxes of the larger slivers, and most of them are occluded
    # (point lights first: the order of the renderer's light table, lights.rs)
    lights = [dict(kind="point", pos=(3.0, 0.0, -0.02), color=(6.0, 6.0, 6.0), falloff=5.0, casts_shadows=True),
              dict(kind="directional", dir=(-1.0, 0.0, 0.01), color=(1.0, 1.0, 1.0), casts_shadows=True)]
    return _flat_scene("chain", mb, camera, lights), rays


def degenerate_soup(n_tris, shape):
    """n_tris random triangles, a quarter of them copies of their neighbours (equal centroids: flat domains, ties); shape "soup", or one that starves a split heuristic:
    "flat" (every centroid in one plane), "line", "clusters" (a dozen far-apart clumps), "one point" (no plane separates anything)"""
    from araytracingjourney_amd import scenes
    rng = np.random.default_rng(n_tris)
    mb = scenes.MeshBuilder()
    c = rng.uniform(-1.0, 1.0, (n_tris, 3)).astype(np.float32) * np.array([1.0, 0.3, 0.6], np.float32)
    if shape == "flat": c[:, 2] = 0.25
    elif shape == "line": c[:, 1] = 0.1; c[:, 2] = -0.2
    elif shape == "clusters": c = (rng.uniform(-1.0, 1.0, (12, 3)).astype(np.float32)[rng.integers(0, 12, n_tris)] + rng.normal(0, 0.004, (n_tris, 3)).astype(np.float32)).astype(np.float32)
    elif shape == "one point": c[:] = np.array([0.1, 0.05, 0.3], np.float32)
    c[3::4] = c[2::4][: c[3::4].shape[0]]                                                 # duplicates
    ext = max(0.05, 0.8 / np.sqrt(n_tris))
    e = rng.uniform(-ext, ext, (n_tris, 2, 3)).astype(np.float32)
    e[3::4] = e[2::4][: e[3::4].shape[0]]
    for k in range(n_tris):
        p0 = c[k]; p1 = c[k] + e[k, 0]; p2 = c[k] + e[k, 1]
        mb.add([tuple(p0), tuple(p1), tuple(p2)], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
    return scenes.Scene("soup", [mb.finish(scenes.constant_texture((200, 180, 160)))], scenes.cornell().camera, scenes.cornell().lights)


def similarity(scene, rays, camera=None, lights=None, s=1.0, offset=(0.0, 0.0, 0.0)):
    """x -> s * x + offset, applied in float32 to the DATA: vertex positions, ray origins and tmin / tmax, the camera's position and znear / zfar, the lights' positions
    and falloff distances.  Directions, normals and colours stay.  -> (scene, rays) with the camera and the lights inside the scene.  s must be positive"""
    from araytracingjourney_amd import scenes
    s32, off = np.float32(s), np.asarray(offset, np.float32)
    prims = []
    for p in scene.primitives:
        assert np.array_equal(np.asarray(p.model, np.float32).reshape(3, 4), np.eye(3, 4, dtype=np.float32)), "similarity() moves vertices: the primitives must carry no matrix"
        v = np.array(p.verts, np.float32)
        v[:, 0:3] = v[:, 0:3] * s32 + off
        prims.append(scenes.Primitive(v, p.indices, p.tex))
    cam = dict(scene.camera if camera is None else camera)
    cam["pos"] = tuple(float(x) for x in np.asarray(cam["pos"], np.float32) * s32 + off)
    cam["znear"], cam["zfar"] = float(np.float32(cam["znear"]) * s32), float(np.float32(cam["zfar"]) * s32)
    ls = []
    for d in (scene.lights if lights is None else lights):
        d = dict(d)
        for k in ("pos", "pos2", "pos3"):
            if k in d:
                d[k] = tuple(float(x) for x in np.asarray(d[k], np.float32) * s32 + off)
        if "falloff" in d:
            d["falloff"] = float(np.float32(d["falloff"]) * s32)
        ls.append(d)
    out = None
    if rays is not None:
        out = np.array(rays, np.float32).reshape(-1, 8)
        out[:, 0:3] = out[:, 0:3] * s32 + off
        out[:, 3] *= s32
        out[:, 7] *= s32
    return scenes.Scene(scene.name, prims, cam, ls), out


def with_ranges(rays, ranges=RANGES):
    """every ray once per range, interleaved ray by ray (ray 0 with every range, then ray 1 ...): any 64 consecutive records hold every kind of range"""
    out = np.repeat(np.asarray(rays, np.float32).reshape(-1, 8), len(ranges), axis=0)
    out[:, 3] = np.tile(np.array([r[0] for r in ranges], np.float32), rays.shape[0])
    out[:, 7] = np.tile(np.array([r[1] for r in ranges], np.float32), rays.shape[0])
    return out


def _f32_fma(a, b, c):
    """float32(a * b + c) with one rounding wherever that matters here: the product of two float32 is exact in float64"""
    with np.errstate(all="ignore"):
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _slab(lo, hi, o, inv, tmin, tlimit):
    """the walks' slab test for one ray against boxes lo, hi [k, 3] -> (hit [k], entry distance [k]); inv = 1 / safe_dir(d)"""
    with np.errstate(all="ignore"):
        ood = (o * inv).astype(np.float32)
        t0, t1 = _f32_fma(lo, inv, -ood), _f32_fma(hi, inv, -ood)
        tn, tf = np.fmax.reduce(np.fmin(t0, t1), axis=1), np.fmin.reduce(np.fmax(t0, t1), axis=1)
        return np.fmax(tn, np.float32(tmin)) <= np.fmin(tf, np.float32(tlimit)), tn


def _ray_inv(ray):
    d = np.asarray(ray[4:7], np.float32)
    safe = np.where(np.abs(d) < np.float32(1e-20), np.copysign(np.float32(1e-20), d), d).astype(np.float32)
    return np.asarray(ray[0:3], np.float32), (np.float32(1.0) / safe).astype(np.float32)


def pending_on_first_descent_binary(child, node_lo, node_hi, leaf_lo, leaf_hi, ray):
    """nodes a nearer-child-first binary walk of `ray` holds on its stack when it first stands on a triangle (it continues with the nearer of two hit children and
    pushes the farther).  No triangle has been tested by then, so the limit is still tmax: a lower bound of the deepest stack of any closest-hit walk of this tree"""
    o, inv = _ray_inv(ray)
    cur, pending = 0, 0
    while cur >= 0:
        c = child[cur]
        lo = np.stack([leaf_lo[~x] if x < 0 else node_lo[x] for x in c])
        hi = np.stack([leaf_hi[~x] if x < 0 else node_hi[x] for x in c])
        h, tn = _slab(lo, hi, o, inv, ray[3], ray[7])
        if h[0] and h[1]:
            pending += 1
            cur = c[0] if tn[0] <= tn[1] else c[1]
        elif h[0] or h[1]:
            cur = c[0] if h[0] else c[1]
        else:
            return pending   # (the ray leaves the tree before any triangle)
    return pending


def pending_on_first_descent_wide(floats, ray):
    """the same for the 4-wide nodes (the (n, 32) uint32 float-box records of get_wide_nodes): the walk continues with the nearest hit child and pushes every other one"""
    o, inv = _ray_inv(ray)
    boxes, child = floats[:, :24].view(np.float32).reshape(-1, 4, 6), floats[:, 24:28].view(np.int32)
    cur, pending = 0, 0
    while cur >= 0:
        valid = child[cur] != -2 ** 31
        h, tn = _slab(boxes[cur, :, :3], boxes[cur, :, 3:], o, inv, ray[3], ray[7])
        h &= valid
        if not h.any():
            return pending
        pending += int(h.sum()) - 1
        cur = child[cur][np.argmin(np.where(h, tn, np.inf))]
    return pending


def pending_on_first_descent_point(lo, hi, valid, child, point):
    """the same for a nearest-point walk of the quantised 4-wide nodes (lo, hi, valid of dequantise(); child: words 12..15 of the records as int32) with r = inf: on
    with the nearest valid child by the distance to its box, every other valid child pushed -- nothing is beyond an infinite limit.  Equal distances (a point inside
    several boxes: 0) are ordered as the walk's five-comparator network orders them, which is not by index"""
    p = np.asarray(point[0:3], np.float32)
    cur, pending = 0, 0
    while cur >= 0:
        with np.errstate(all="ignore"):
            e = np.fmax(np.fmax(lo[cur] - p, p - hi[cur]), np.float32(0))
            d2 = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(np.float32)
        k = [d2[i] if valid[cur, i] else np.float32(np.inf) for i in range(4)]
        rf = [int(child[cur, i]) if valid[cur, i] else None for i in range(4)]
        for x, y in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
            if k[y] < k[x]:
                k[x], k[y], rf[x], rf[y] = k[y], k[x], rf[y], rf[x]
        if rf[0] is None:
            return pending
        pending += sum(r is not None for r in rf[1:])
        cur = rf[0]
    return pending


def dequantise(quantised):
    """the child boxes of the (n, 16) uint32 quantised records as the per-ray walks evaluate them: float32(q * 2^(e - 127) + origin), one rounding (q * scale is exact,
    and the float64 sum rounds to float32 like the exact one: q * scale has 8 bits) -> lo, hi [n, 4, 3] float32 and the valid mask [n, 4]"""
    org = quantised[:, 0:3].view(np.float32).astype(np.float64)
    e = np.stack([(quantised[:, 3] >> (8 * k)) & 255 for k in range(3)], 1).astype(np.int64)
    scale = np.ldexp(1.0, e - 127)
    planes = np.stack([[(quantised[:, 4 + k] >> (8 * i)) & 255 for k in range(6)] for i in range(4)], 0).astype(np.float64)   # [child, plane, node]
    planes = planes.transpose(2, 0, 1)                                                                                         # [node, child, plane]
    lo = (planes[:, :, 0:3] * scale[:, None, :] + org[:, None, :]).astype(np.float32)
    hi = (planes[:, :, 3:6] * scale[:, None, :] + org[:, None, :]).astype(np.float32)
    valid = ((quantised[:, 3][:, None] >> (24 + np.arange(4))) & 1).astype(bool)
    return lo, hi, valid, planes


# ---- what the tests of the queries on device buffers share (test_cast, test_cast_multi, test_resolve, test_closest_points, test_sphere_cast, test_query_forms) ------
@pytest.fixture(scope="module")
def R():
    from araytracingjourney_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _up(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: the shared references are read-only)


def _host(got):
    return tuple(t.cpu().numpy() for t in got)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dead_rays(base):
    """NaN direction, infinite origin, NaN tmax in turn"""
    d = base.copy()
    d[0::3, 4] = np.nan
    d[1::3, 0] = np.inf
    d[2::3, 7] = np.nan
    return d


def _outward_rays(base):
    """from the sphere around the scene, away from it: nothing to hit"""
    out = base[(np.arange(base.shape[0]) % 3) != 0].copy()   # (every third ray of random_rays starts inside the scene)
    out[:, 4:7] = out[:, 0:3] / np.linalg.norm(out[:, 0:3], axis=1, keepdims=True)
    return out


def _tex_of_alpha(alpha, rgb=(180, 150, 120)):
    """tests/test_alpha.py's three layers with an alpha per texel"""
    th, tw = alpha.shape
    t = np.zeros((3, th, tw, 4), np.uint8)
    t[0, ..., 0], t[0, ..., 1], t[0, ..., 2] = rgb
    t[0, ..., 3] = alpha
    t[1, ..., 0], t[1, ..., 1], t[1, ..., 2], t[1, ..., 3] = 255, 160, 0, 255
    t[2, ..., 0], t[2, ..., 1], t[2, ..., 2], t[2, ..., 3] = 128, 128, 255, 255
    return t


def _tex_flat(alpha_value, tw=8, th=8):
    """the same layers, alpha the same in every texel: no sampler is needed to know the alpha anywhere"""
    t = np.zeros((3, th, tw, 4), np.uint8)
    t[0, ..., 0], t[0, ..., 1], t[0, ..., 2], t[0, ..., 3] = 180, 150, 120, alpha_value
    t[1, ..., 0], t[1, ..., 1], t[1, ..., 2], t[1, ..., 3] = 255, 160, 0, 255
    t[2, ..., 0], t[2, ..., 1], t[2, ..., 2], t[2, ..., 3] = 128, 128, 255, 255
    return t


def layout_mismatches(header, namespace, only=None):
    """the structs the header at path `header` declares (all of them, or the one named `only`) against the ctypes classes of their names in `namespace`, gcc being the judge:
    one line "Name: what differs" for every struct whose field names in order, sizeof, any offsetof or packedness is not the class's; [] when the binding is the header's"""
    structs = [s for s in gen_bindings.parse(header)[2] if only in (None, s[0])]
    assert structs, (header, only)
    lay, bad = gen_bindings.c_layout(header, structs), []
    for name, packed, fields in structs:
        cls, names = getattr(namespace, name, None), [f for f, _, _ in fields]
        if cls is None:
            bad.append(f"{name}: no such class")
        elif names != [n for n, _ in cls._fields_]:
            bad.append(f"{name}: fields {[n for n, _ in cls._fields_]} are not the header's {names}")
        elif C.sizeof(cls) != lay[name]:
            bad.append(f"{name}: sizeof {C.sizeof(cls)} is not gcc's {lay[name]}")
        elif bool(getattr(cls, "_pack_", 0)) != packed:
            bad.append(f"{name}: packed in one, not in the other")
        else:
            bad += [f"{name}: offsetof {f} {getattr(cls, f).offset} is not gcc's {lay[name + '.' + f]}" for f in names if getattr(cls, f).offset != lay[name + "." + f]][:1]
    return bad


def _layout_is_the_headers(name, size, fields=None):
    """_lib's ctypes class `name` is the struct of include/art.h as gcc compiles it, field by field (layout_mismatches), `size` bytes long, and its fields are `fields`
    where given; returns the class"""
    from araytracingjourney_amd import _lib
    cls = getattr(_lib, name)
    assert layout_mismatches(os.path.join(ROOT, "include", "art.h"), _lib, only=name) == []
    assert C.sizeof(cls) == size and fields in (None, [n for n, _ in cls._fields_])
    return cls
