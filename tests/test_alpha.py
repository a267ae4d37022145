"""Alpha-masked primitives (art_scene_set_alpha_cutoff; glTF alphaMode MASK, in Vulkan terms non-opaque geometry whose any-hit shader ignores the intersection when
alpha < cutoff): a candidate that accept() takes is discarded when its primitive's cutoff c > 0 and the alpha of its texture layer 0 -- bilinear, REPEAT, LOD 0 at
the hit's texture coordinate -- is below c, for primary, shadow and AO rays and both queries, in every form of the frame.  The oracle has no alpha:
the references are equalities with features already pinned (a disabled primitive, the opaque scene) and a numpy brute force with the rule applied per candidate."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_radiance_close
from helpers import random_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the forms of the frame ArtTuning selects (fused packet walks over 4-wide / binary nodes; staged per-ray walks over binary / quantised 4-wide nodes; AO walks 2 / 4 / 6)
FORMS = {
    "fused": {},
    "fused-wide": {"packet_wide": 1},
    "fused-binary": {"packet_wide": 2, "ao_walk": 2},
    "per-ray": {"frame_form": 2},
    "per-ray-binary": {"frame_form": 2, "primary_walk": 2, "shadow_walk": 2, "ao_walk": 2},
    "per-ray-wide": {"frame_form": 2, "primary_walk": 4, "shadow_walk": 4, "ao_walk": 6},
    "per-ray-mixed": {"frame_form": 2, "primary_walk": 4, "shadow_walk": 2, "ao_walk": 4},
}


@pytest.fixture(scope="module")
def R():
    from araytracingjourney_amd import renderer
    return renderer


def _tex(alpha, rgb=(180, 150, 120)):
    """3 layers (albedo with the given alpha, ORM, flat normal) of alpha's extent"""
    th, tw = alpha.shape
    t = np.zeros((3, th, tw, 4), np.uint8)
    t[0, ..., 0], t[0, ..., 1], t[0, ..., 2] = rgb
    t[0, ..., 3] = alpha
    t[1, ..., 0], t[1, ..., 1], t[1, ..., 2], t[1, ..., 3] = 255, 160, 0, 255
    t[2, ..., 0], t[2, ..., 1], t[2, ..., 2], t[2, ..., 3] = 128, 128, 255, 255
    return t


def _quad(scenes, p0, du, dv, alpha, uv_scale=(1.0, 1.0), n=2):
    mb = scenes.MeshBuilder()
    scenes.quad(mb, p0, du, dv, n, n, uv_scale)
    return mb.finish(_tex(alpha))


def _ceiling_card(scenes, alpha):
    """a horizontal card under Cornell's light: seen by the camera, between the light and the floor"""
    return _quad(scenes, (-0.35, 0.3, -0.35), (0.7, 0.0, 0.0), (0.0, 0.0, 0.7), alpha)


def _scene(sc, extra):
    from araytracingjourney_amd import scenes
    return scenes.Scene(sc.name + "+card", list(sc.primitives) + list(extra), sc.camera, sc.lights)


def _outputs(r, rays, ao=True):
    """everything a frame and the queries give: colour, depth, normal, hits, shadow bits, AO, closest and any-hit queries"""
    r.sync()
    tuv, ids = r.read_hits()
    out = {"color": r.read_color(), "depth": r.read_depth(), "normal": r.read_normal(), "tuv": tuv, "ids": ids, "shadow_bits": r.read_shadow_bits()}
    if ao:
        r.trace_ao(4, 0.3)
        out["ao"] = r.read_ao()
    q_tuv, q_ids = r.query_closest(rays)
    out["q_tuv"], out["q_ids"], out["q_any"] = q_tuv, q_ids, r.query_any(rays)
    return out


def _assert_equal(a, b, what):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {k} differs ({int((x != y).sum())} values)"


def _render(R, sc, extent, tuning, cutoffs=None, disabled=(), before_build=False, F=1):
    r = R.Renderer(extent, keep_debug=True, tuning=tuning, frames_in_flight=F)
    r.add_model(sc.primitives)
    cam = r.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    for d in sc.lights:
        r.lights_mut().push_dict(d)
    m = r.models_mut()[0]
    if before_build:
        for i, c in (cutoffs or {}).items():
            m.set_alpha_cutoff(i, c)
    r.prepare_first_frame()
    if not before_build:
        for i, c in (cutoffs or {}).items():
            m.set_alpha_cutoff(i, c)
    for i in disabled:
        C_ok = r._L.art_scene_set_primitive_enabled(r._ctx, m.primitive_ids[i], 0)
        assert C_ok == 0
    r.upload_state()
    r.trace()
    return r


def _render_outputs(R, sc, extent, tuning, rays, **kw):
    """_outputs of a context made for them, which is closed again (a Renderer and its models refer to each other: unclosed, it keeps its context until a garbage collection)"""
    r = _render(R, sc, extent, tuning, **kw)
    try:
        return _outputs(r, rays)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_a_card_cut_everywhere_is_a_disabled_card(R, get_scene, scenes, form):
    """Cornell 64^2 and a card whose alpha is 0 everywhere, cutoff 0.5: every output -- colour, depth, normal, hits, shadow bits, AO and both queries -- equals the
    same context with the card disabled, bit for bit, in every form of the frame; and the opaque card is a different frame (the test sees the card)"""
    sc = _scene(get_scene("cornell"), [_ceiling_card(scenes, np.zeros((8, 8), np.uint8))])
    card = len(sc.primitives) - 1
    rays = random_rays(2048, 5, radius=0.9)
    t = FORMS[form]
    cut = _render_outputs(R, sc, (64, 64), t, rays, cutoffs={card: 0.5})
    off = _render_outputs(R, sc, (64, 64), t, rays, disabled=[card])
    _assert_equal(cut, off, f"{form}: cut card vs disabled card")
    cut_b = _render_outputs(R, sc, (64, 64), t, rays, cutoffs={card: 0.5}, before_build=True)
    _assert_equal(cut_b, off, f"{form}: cutoff set before the build vs disabled card")
    opaque = _render_outputs(R, sc, (64, 64), t, rays)
    assert not np.array_equal(opaque["depth"], off["depth"]) and not np.array_equal(opaque["shadow_bits"], off["shadow_bits"]), "the card is neither seen nor casting shadows"
    assert (opaque["q_ids"] != off["q_ids"]).any() and not np.array_equal(opaque["ao"], off["ao"])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "fused-binary", "per-ray", "per-ray-wide"])
def test_nothing_cut_is_the_opaque_scene(R, get_scene, scenes, form):
    """alpha 255 everywhere with cutoff 0.5 (the masked instances run, nothing is cut), and cutoff 0 on an all-zero alpha (opaque): both equal the unmasked scene"""
    t = FORMS[form]
    rays = random_rays(2048, 6, radius=0.9)
    full = _scene(get_scene("cornell"), [_ceiling_card(scenes, np.full((8, 8), 255, np.uint8))])
    zero = _scene(get_scene("cornell"), [_ceiling_card(scenes, np.zeros((8, 8), np.uint8))])
    card = len(full.primitives) - 1
    ref = _render_outputs(R, full, (64, 64), t, rays)
    _assert_equal(_render_outputs(R, full, (64, 64), t, rays, cutoffs={card: 0.5}), ref, f"{form}: alpha 255, cutoff 0.5")
    _assert_equal(_render_outputs(R, full, (64, 64), t, rays, cutoffs={card: 1.0}), ref, f"{form}: alpha 255, cutoff 1")
    ref0 = _render_outputs(R, zero, (64, 64), t, rays)
    r = _render(R, zero, (64, 64), t, cutoffs={card: 0.5})
    r.models_mut()[0].set_alpha_cutoff(card, 0.0)   # back to opaque: the next frame
    r.trace()
    got = _outputs(r, rays)
    r.close()
    _assert_equal(got, ref0, f"{form}: cutoff back to 0")


def _card_alpha(tw=16, th=16):
    """a texel-scale checker of cut texels (alpha 0), the others a gradient along x: bilinear alpha crosses 0.5 inside many texels"""
    y, x = np.mgrid[0:th, 0:tw]
    return np.where((x + y) % 2 == 0, 0, np.round(255.0 * x / (tw - 1))).astype(np.uint8)


def _np_alpha(prim, tri, u, v):
    """the alpha test's value in fp64: layer 0 byte 3 at the candidate's interpolated uv"""
    from np_shading import texture
    i = prim.indices[3 * tri:3 * tri + 3].astype(np.int64)
    uv = prim.verts[i, 3:5].astype(np.float64)
    st = uv[0] * (1.0 - u - v) + uv[1] * u + uv[2] * v
    return float(texture(prim.tex[0], st)[3])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "per-ray"])
def test_partial_cut_against_numpy(R, get_scene, scenes, form):
    """a card with a texel-scale checker and an alpha gradient in front of Cornell's back wall, lights behind it: every hit is the numpy brute force's closest
    candidate that passes the alpha rule, every shadow bit its any-hit with the same rule, radiance shade_pixel's within 1e-4 -- except pixels whose fp64 alpha
    of some deciding candidate lies within 1e-4 of the cutoff (fewer than 1 %) and pixels whose deciding candidate lies within 1e-4 of a triangle's edge (shared
    edges: the frame's diagonal runs along the back wall's)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import np_shading as nps
    base = get_scene("cornell")
    card = _quad(scenes, (-0.4, -0.3, 0.3), (0.8, 0.0, 0.0), (0.0, 0.75, 0.0), _card_alpha(), uv_scale=(1.0, 1.0), n=3)
    lights = list(base.lights) + [dict(kind="point", pos=(0.1, 0.05, -0.2), color=(3.0, 3.0, 3.0), falloff=3.0, casts_shadows=True)]
    from araytracingjourney_amd import scenes as S
    sc = S.Scene("cornell+card", list(base.primitives) + [card], base.camera, lights)
    ci, cutoff, w, h = len(sc.primitives) - 1, 0.5, 64, 64
    r = _render(R, sc, (w, h), FORMS[form], cutoffs={ci: cutoff})
    r.sync()
    color, (tuv, ids), bits = r.read_color(), r.read_hits(), r.read_shadow_bits()
    tris, pid, tid = nps.world_triangles(sc.primitives)
    cam = sc.camera
    view, view_inv, proj, proj_inv = nps.camera_matrices(cam["pos"], cam["dir"], w / h, cam["fovy"], cam["znear"], cam["zfar"])
    ls = [nps.light_from_record(x) for x in r._lights.copy_lights_shader_data()[0][:len(lights)]]
    r.close()
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]

    def candidates(o, d, tmin, tmax):
        p = np.cross(d, e2); det = np.einsum("ij,ij->i", e1, p)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det; tv = o - v0; u = np.einsum("ij,ij->i", tv, p) * inv; q = np.cross(tv, e1); v = (q @ d) * inv; t = np.einsum("ij,ij->i", e2, q) * inv
        ok = (det != 0) & (u >= -1e-6) & (v >= -1e-6) & (u + v <= 1 + 1e-6) & (t > tmin) & (t < tmax)   # (edges fattened like accept())
        k = np.nonzero(ok)[0]
        k = k[np.argsort(t[k])]
        return [(int(i), float(t[i]), float(u[i]), float(v[i]), float(min(u[i], v[i], 1 - u[i] - v[i]))) for i in k]

    def passes(i, u, v):   # -> (kept, near the cutoff)
        if pid[i] != ci:
            return True, False
        a = _np_alpha(sc.primitives[ci], int(tid[i]), u, v)
        return not (a < cutoff), abs(a - cutoff) < 1e-4

    near, edge, checked, cut_seen = 0, 0, 0, 0
    for y in range(h):
        for x in range(w):
            o, d = nps.primary_ray(x, y, w, h, view_inv, proj_inv)
            amb, on_edge, hit = False, False, None
            for (i, t, u, v, m) in candidates(o, d, 0.001, 10000.0):
                keep, close = passes(i, u, v)
                amb, on_edge = amb or close, on_edge or m < 1e-4
                if keep:
                    hit = (i, u, v); break
                cut_seen += 1
            if amb or on_edge:
                near += amb; edge += not amb; continue
            want = (-1, -1) if hit is None else (int(pid[hit[0]]), int(tid[hit[0]]))
            assert tuple(ids[y, x]) == want, f"{form}: pixel {x},{y}: hit {tuple(ids[y, x])}, numpy {want}"
            if hit is None:
                continue
            prim, tri, u, v = sc.primitives[want[0]], want[1], float(tuv[y, x, 1]), float(tuv[y, x, 2])

            def shadowed(li, org, L, tmax):
                blocked, a = False, False
                for (i, t, uu, vv, m) in candidates(org, L, 0.01, tmax):
                    keep, close = passes(i, uu, vv)
                    a = a or close or m < 1e-4 or abs(t - tmax) < 1e-4 * tmax
                    if keep:
                        blocked = True; break
                amb_sh[0] = amb_sh[0] or a
                return blocked
            amb_sh = [False]
            rho, depth, nrm, mask = nps.shade_pixel(prim, tri, u, v, view, view_inv, np.asarray(cam["pos"], np.float64), ls, shadowed)
            if amb_sh[0]:
                edge += 1; continue
            assert int(bits[y, x]) == int(mask), f"{form}: pixel {x},{y}: shadow bits {int(bits[y, x]):#x}, numpy {int(mask):#x}"
            assert_radiance_close(color[y, x, :3], rho, what=f"{form}: pixel {x},{y}")
            checked += 1
    assert near < 0.01 * w * h, f"{near} pixels whose alpha lies near the cutoff"
    assert edge < 0.04 * w * h, f"{edge} pixels on a triangle's edge"
    assert cut_seen > 100 and checked > 0.9 * w * h, (cut_seen, checked)


@pytest.mark.gpu
def test_cutoffs_change_without_a_build_with_sixteen_frames_in_flight(R, get_scene, scenes):
    """the card's cutoff changes every frame, mixed with a move of the card and a set_vertices, sixteen frames in flight: each frame equals a fresh context
    holding the state current at its launch; no rebuild, needs_build unchanged; residency out and in keeps the mask"""
    base = get_scene("cornell")
    card0 = _quad(scenes, (-0.4, -0.3, 0.3), (0.8, 0.0, 0.0), (0.0, 0.75, 0.0), _card_alpha(), n=3)
    sc = _scene(base, [card0])
    ci, w, h = len(sc.primitives) - 1, 48, 48
    r = R.Renderer((w, h), keep_debug=True, frames_in_flight=16)
    r.add_model(list(base.primitives))
    r.add_model([card0])
    cam = r.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    for d in sc.lights:
        r.lights_mut().push_dict(d)
    r.prepare_first_frame()
    r.upload_state()
    m = r.models_mut()[1]
    st0 = r.stats()
    states, grabs = [], []
    verts = card0.verts.copy()
    mm = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    for i in range(16):
        c = [0.5, 0.0, 0.25, 0.75, 1.0, 0.4][i % 6]
        m.set_alpha_cutoff(0, c)
        if i % 4 == 1:
            mm = np.array([1, 0, 0, 0.02 * i, 0, 1, 0, 0.01 * i, 0, 0, 1, 0], np.float32); m.set_model_matrix(mm)
        if i % 4 == 3:
            verts = card0.verts.copy(); verts[:, 3:5] += np.float32(0.05 * i); m.set_vertices(0, verts)
        r.trace()
        states.append((c, mm.copy(), verts.copy()))
        grabs.append((r.device_color(), r._dev("depth")))
        assert not r.needs_build()
    from helpers import device_to_host
    r.sync()
    outs = [(device_to_host(*gc).view(np.float32).reshape(h, w, 4).copy(), device_to_host(*gd).view(np.float32).reshape(h, w).copy()) for gc, gd in grabs]
    st = r.stats()
    assert st["rebuilds"] == st0["rebuilds"], "a cutoff change must not rebuild"
    from araytracingjourney_amd import scenes as S
    for k, (c, mm_i, v_i) in enumerate(states):   # (sixteen ring slots: no frame's buffers were reused)
        P = type(card0)
        fresh_sc = S.Scene("x", list(base.primitives) + [P(v_i, card0.indices, card0.tex, mm_i)], sc.camera, sc.lights)
        f = _render(R, fresh_sc, (w, h), {}, cutoffs={ci: c} if c > 0 else None)
        f.sync()
        f_depth, f_color = f.read_depth(), f.read_color()
        f.close()
        assert np.array_equal(outs[k][1].view(np.uint32), f_depth.view(np.uint32)), f"frame {k}: depth"
        assert np.array_equal(outs[k][0].view(np.uint32), f_color.view(np.uint32)), f"frame {k}: colour"
    # residency: the card out (a disabled primitive) and back in keeps its cutoff
    m.set_alpha_cutoff(0, 0.5)
    r.trace(); r.sync(); want = r.read_depth().copy()
    r._L.art_scene_set_primitive_enabled(r._ctx, m.primitive_ids[0], 0); r.trace(); r.sync()
    r._L.art_scene_set_primitive_enabled(r._ctx, m.primitive_ids[0], 1); r.trace(); r.sync()
    assert np.array_equal(r.read_depth().view(np.uint32), want.view(np.uint32)), "residency out and in lost the mask"
    assert r.stats()["rebuilds"] == st0["rebuilds"] and not r.needs_build()
    r.close()


@pytest.mark.gpu
def test_config2_banners_masked(R, get_scene):
    """config 2 at full size with the twelve banners (primitives 12..23) given a cut-out texture: every form of the frame gives the same frame bit for bit; a
    pixel whose opaque hit is not a banner keeps its hit; the frame differs from the opaque one"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from alpha_probe import banner_scene, BANNERS
    sc = banner_scene(get_scene("sponza_like", 1.0))
    w, h = 1920, 1080

    def frame(tuning, masked=True):
        r = _render(R, sc, (w, h), tuning, cutoffs={i: 0.5 for i in BANNERS} if masked else None)
        r.sync()
        out = r.read_hits()[1], r.read_depth(), r.read_color(), r.read_shadow_bits()
        r.close()
        return out
    ref = frame({})
    for name in ("fused-binary", "per-ray", "per-ray-wide"):
        got = frame(FORMS[name])
        for a, b, k in zip(got, ref, ("ids", "depth", "color", "shadow bits")):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), f"{name}: {k}"
    opaque = frame({}, masked=False)
    not_banner = ~np.isin(opaque[0][..., 0], BANNERS)
    assert np.array_equal(ref[0][not_banner], opaque[0][not_banner]), "a pixel that did not see a banner changed its hit"
    seen = np.isin(opaque[0][..., 0], BANNERS)
    moved = (ref[0] != opaque[0]).any(-1)
    assert moved[seen].mean() > 0.1, "the cut-out banners let nothing through"
    assert (ref[1][seen & moved] > opaque[1][seen & moved]).all(), "a pixel behind a cut texel must see something farther"


@pytest.mark.gpu
def test_bad_calls_change_nothing(R, get_scene, scenes):
    """NaN, -0.1, 1.5, an unknown id, a null context: ART_E_INVALID, the frame unchanged, no build asked for"""
    sc = _scene(get_scene("cornell"), [_ceiling_card(scenes, np.zeros((8, 8), np.uint8))])
    r = _render(R, sc, (32, 32), {}, cutoffs={len(sc.primitives) - 1: 0.5})
    r.sync(); want = r.read_color().copy()
    L, pid = r._L, r.models_mut()[0].primitive_ids[-1]
    for v in (float("nan"), -0.1, 1.5, float("inf")):
        assert L.art_scene_set_alpha_cutoff(r._ctx, pid, v) != 0
    assert L.art_scene_set_alpha_cutoff(r._ctx, 10_000, 0.5) != 0
    assert L.art_scene_set_alpha_cutoff(None, 0, 0.5) != 0
    assert not r.needs_build()
    r.trace(); r.sync()
    assert np.array_equal(r.read_color().view(np.uint32), want.view(np.uint32))
    assert r.stats()["rebuilds"] == 0
    r.close()


def _mask_glb(path, prims, cutoff=0.4, blend_first=False):
    """write a GLB with tests/glb_writer.py, then patch its JSON: every material alphaMode MASK with alphaCutoff (the first BLEND if asked); the RGBA base colours stay"""
    import json
    import struct
    from glb_writer import write_glb
    write_glb(str(path), prims, png_modes=("RGBA", "RGBA", "RGBA"))
    data = open(path, "rb").read()
    jl, = struct.unpack_from("<I", data, 12)
    doc = json.loads(data[20:20 + jl])
    for k, m in enumerate(doc["materials"]):
        m["alphaMode"] = "BLEND" if (blend_first and k == 0) else "MASK"
        m["alphaCutoff"] = cutoff
    js = json.dumps(doc).encode(); js += b" " * (-len(js) % 4)
    rest = data[20 + jl:]
    with open(path, "wb") as f:
        f.write(struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(js) + len(rest)))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js + rest)


def test_glb_reports_the_material_alpha(get_scene, scenes, tmp_path):
    """art_glb_primitive_alpha: mode, cutoff and whether the base colour had alpha; glTF's defaults (OPAQUE, 0.5) without the fields; an RGB base colour has none"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from glb_writer import write_glb
    from araytracingjourney_amd.model_reader import GltfModelReader
    prims = list(get_scene("cornell").primitives[:2])
    p = tmp_path / "mask.glb"
    _mask_glb(p, prims, cutoff=0.4, blend_first=True)
    rd = GltfModelReader(str(p))
    assert rd.primitive_alpha(0) == (2, pytest.approx(0.4), True)
    assert rd.primitive_alpha(1) == (1, pytest.approx(0.4), True)
    with pytest.raises(Exception):
        rd.primitive_alpha(2)
    rd.close()
    q = tmp_path / "plain.glb"
    write_glb(str(q), prims, png_modes=("RGB", "RGBA", "RGBA"))
    rd = GltfModelReader(str(q))
    assert rd.primitive_alpha(0) == (0, 0.5, False)
    rd.close()


@pytest.mark.gpu
def test_glb_alpha_mask_equals_the_cutoff_set_by_hand(R, get_scene, scenes, tmp_path):
    """add_model_glb(alpha_mask=True) equals the cutoffs set by hand; the default add_model_glb renders as today (opaque, though the material says MASK); the C++
    mirror's alpha mode agrees with itself the same way"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from araytracingjourney_amd.model_reader import GltfModelReader
    base = get_scene("cornell")
    card = _quad(scenes, (-0.4, -0.3, 0.3), (0.8, 0.0, 0.0), (0.0, 0.75, 0.0), _card_alpha(), n=3)
    prims = list(base.primitives) + [card]   # (the room's materials go back to OPAQUE below: only the card is MASK)
    path = tmp_path / "card.glb"
    _mask_glb(path, prims, cutoff=0.5)
    import json, struct
    data = open(path, "rb").read(); jl, = struct.unpack_from("<I", data, 12); doc = json.loads(data[20:20 + jl])
    for m in doc["materials"][:-1]:
        m["alphaMode"] = "OPAQUE"
    js = json.dumps(doc).encode(); js += b" " * (-len(js) % 4); rest = data[20 + jl:]
    with open(path, "wb") as f:
        f.write(struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(js) + len(rest))); f.write(struct.pack("<II", len(js), 0x4E4F534A) + js + rest)
    eye = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)

    def frame(mask, by_hand=False):
        r = R.Renderer((64, 64), keep_debug=True)
        rd = GltfModelReader(str(path))
        ids = r.add_model_glb(rd, eye, alpha_mask=mask)
        cam = r.camera_mut()
        cam.set_pos(base.camera["pos"]); cam.set_dir(base.camera["dir"]); cam.set_fovy(base.camera["fovy"])
        for d in base.lights:
            r.lights_mut().push_dict(d)
        r.prepare_first_frame()
        if by_hand:
            r.models_mut()[0].set_alpha_cutoff(len(ids) - 1, 0.5)
        r.upload_state(); r.trace(); r.sync()
        out = (r.read_color().copy(), r.read_depth().copy(), r.read_shadow_bits().copy())
        rd.close(); r.close()
        return out
    masked, hand, plain = frame(True), frame(False, by_hand=True), frame(False)
    for a, b in zip(masked, hand):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(masked[1], plain[1]), "the default add_model_glb must stay opaque"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([os.path.join(ROOT, "examples", "host_mirror_demo"), "alpha", str(path), "96", "64"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALPHA_OK" in out.stdout, out.stdout + out.stderr
    f = dict(kv.split("=") for kv in out.stdout.split("ALPHA_OK")[1].split("\n")[0].split())
    assert (int(f["masked_prims"]), int(f["masked_equals_by_hand"]), int(f["differs_from_opaque"]), int(f["rebuilds"])) == (1, 1, 1, 0), out.stdout


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------------------------------
_FRAME = "_ZN3art7k_frameILb{}ELb{}ELb{}ELb{}ELb{}EEEvNS_9FrameArgsE"
# the default instances' figures before the alpha test existed (VGPRs, scratch bytes): unchanged
_DEFAULT = {(1, 1, 0, 0): (63, 0), (1, 1, 0, 1): (62, 0), (1, 1, 1, 0): (63, 0), (1, 1, 1, 1): (62, 0), (1, 0, 0, 0): (64, 8), (1, 0, 0, 1): (64, 0),
            (1, 0, 1, 0): (64, 0), (1, 0, 1, 1): (64, 0), (0, 1, 0, 0): (63, 0), (0, 1, 0, 1): (61, 0), (0, 1, 1, 0): (63, 0), (0, 1, 1, 1): (61, 0),
            (0, 0, 0, 0): (64, 0), (0, 0, 0, 1): (63, 0), (0, 0, 1, 0): (64, 0), (0, 0, 1, 1): (64, 0)}


def test_frame_kernel_instances_in_the_code_object():
    """the AMDGPU metadata of libart.so's code objects: every default k_frame instance keeps its VGPR count (at most 64) and scratch, and every instance with
    the alpha test exists, as do the alpha instances of the per-ray tracers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    k = kernel_resources()
    for key, (vgpr, scratch) in _DEFAULT.items():
        d = k[_FRAME.format(*key, 0)]
        assert d["vgpr"] + d["agpr"] <= 64 and (d["vgpr"], d["scratch"]) == (vgpr, scratch), (key, d)
        assert _FRAME.format(*key, 1) in k, key
    for mode in (0, 1, 4):   # primary, shadow, AO (2 and 3 were the queries': they go through k_cast)
        for width in (2, 4):
            assert f"_ZN3art7k_traceILi{mode}ELi{width}ELb1EEEvNS_9TraceArgsE" in k
    assert "_ZN3art10k_trace_aoILb1EEEvNS_9TraceArgsE" in k


def test_model_set_alpha_cutoff_validates_its_arguments():
    """Model.set_alpha_cutoff without a context: a cutoff outside [0, 1], NaN or not a number, an index out of range are refused before anything is called"""
    from araytracingjourney_amd import renderer as R
    m = R.Model([3, 4], None)
    for bad in (float("nan"), -0.1, 1.5, float("inf")):
        with pytest.raises(ValueError):
            m.set_alpha_cutoff(0, bad)
    for bad in ("0.5", None, True):
        with pytest.raises(TypeError):
            m.set_alpha_cutoff(0, bad)
    with pytest.raises(IndexError):
        m.set_alpha_cutoff(2, 0.5)
    with pytest.raises(IndexError):
        m.set_alpha_cutoff(-1, 0.5)
    with pytest.raises(TypeError):
        m.set_alpha_cutoff(0.0, 0.5)
    m.set_alpha_cutoff(1, 0.0); m.set_alpha_cutoff(1, 1); m.set_alpha_cutoff(np.int64(0), np.float32(0.25))


def test_the_symbol_tables_know_the_new_entry_points():
    from araytracingjourney_amd import _lib
    assert _lib.SYMBOLS["art_scene_set_alpha_cutoff"][1][2] is C.c_float
    assert "art_glb_primitive_alpha" in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "art_scene_set_alpha_cutoff(ArtContext *ctx, uint32_t primitive_id, float cutoff)" in hdr
