"""art_closest_points (include/art.h): the nearest surface point to a point, defined exactly and checked bit for bit.

The reference is tests/np_closest.py: (a) the world vertices restated with xform_point's operation order, (b) the semantics as a numpy float32 brute force over every
(query, triangle) pair -- what the device must write, ids and bits -- and (c) an independent fp64 witness of the true distance.  The CPU tests check (a) against the
oracle's leaf boxes and (b) against (c) before the GPU tests lean on (b).

Measured (b) against (c), origins of random_rays(4096, 7), r = inf: worst |d32 - d64| 1.65e-7 on cornell 1.0 and 2.35e-7 on sponza_like 0.05; four times that is
allowed (tests/golden/closest_points.stats.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import np_closest as nc
from helpers import SIMILARITIES, chain_scene, degenerate_soup, lattice_coords, lattice_scene, oracle_camera, oracle_for, random_rays, similarity
from helpers import _bits, _layout_is_the_headers, _host, R, _tex_flat as _tex, torch, _up  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = os.path.join(ROOT, "tests", "golden", "closest_points.stats.json")
PATTERN = -0x5A5A5A5B   # tests/test_cast.py's: what oversized output buffers are filled with
N = 4096
SCENES = [("cornell", 1.0), ("sponza_like", 0.05)]


def queries(points, r=np.inf):
    q = np.zeros((np.asarray(points).reshape(-1, 3).shape[0], 4), np.float32)
    q[:, 0:3] = np.asarray(points, np.float32).reshape(-1, 3)
    q[:, 3] = r
    return q


_REF = {}


def _ref(get_scene, name, detail):
    """the scene, its triangles, the queries (origins of random_rays(4096, 7), r = inf) and (b)'s records with its statistics: computed once, shared, never written"""
    key = (name, detail)
    if key not in _REF:
        sc = get_scene(name, detail)
        T = nc.world_triangles(sc.primitives)
        q = queries(random_rays(N, 7)[:, 0:3])
        duv, ids, point, st = nc.brute_force(T, q, stats=True)
        for a in (q, duv, ids, point):
            a.setflags(write=False)
        _REF[key] = dict(scene=sc, T=T, q=q, want=(duv, ids, point), stats=st)
    return _REF[key]


def _same(got, want, what=""):
    """ids, the bits of d, u, v, a fourth word of 0, the bits of the point"""
    (duv, ids, point), (rduv, rids, rpoint) = got, want
    assert duv.shape == rduv.shape and ids.shape == rids.shape and point.shape == rpoint.shape, what
    assert np.array_equal(ids, rids), f"{what}: the ids of {int((ids != rids).any(axis=1).sum())} of {ids.shape[0]} queries differ (first: {np.flatnonzero((ids != rids).any(axis=1))[:5]})"
    bad = (_bits(duv)[:, :3] != _bits(rduv)[:, :3]).any(axis=1)
    assert not bad.any(), f"{what}: d, u, v of {int(bad.sum())} queries differ (first: {np.flatnonzero(bad)[:5]}: {duv[bad][:2]} for {rduv[bad][:2]})"
    assert not _bits(duv)[:, 3].any(), f"{what}: the fourth word is not 0"
    assert np.array_equal(_bits(point), _bits(rpoint)), f"{what}: the points differ"


def _ask(r, torch, q, **kw):
    got = r.closest_points(_up(torch, q), **kw)
    torch.cuda.synchronize()
    return _host(got)


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
def _sheared_scene(scenes, get_scene):
    """Cornell under a sheared, mirrored (negative determinant) model matrix"""
    base = get_scene("cornell")
    m = np.array([[-1.0, 0.25, 0.0, 0.1], [0.125, 0.75, -0.5, -0.2], [0.0, 0.375, 1.25, 0.3]], np.float32)
    assert np.linalg.det(m[:, :3].astype(np.float64)) < 0
    P = type(base.primitives[0])
    return scenes.Scene("cornell-sheared", [P(p.verts, p.indices, p.tex, m) for p in base.primitives], base.camera, base.lights)


@pytest.mark.parametrize("which", ["cornell", "sponza_like", "sheared"])
def test_world_vertices_give_the_oracles_leaf_boxes(orc, scenes, get_scene, which):
    """1: (a)'s world vertices give, by min / max, the oracle's leaf boxes bit for bit"""
    sc = _sheared_scene(scenes, get_scene) if which == "sheared" else get_scene(which, dict(SCENES)[which])
    T = nc.world_triangles(sc.primitives)
    lb = orc.Scene(sc.primitives, morton_bits=30).lbvh()
    gid = lb["leaf_gid"].astype(np.int64)
    assert T["lo"].shape[0] == gid.size and np.array_equal(np.sort(gid), np.arange(gid.size))
    assert np.array_equal(_bits(T["lo"][gid]), _bits(lb["leaf_lo"])) and np.array_equal(_bits(T["hi"][gid]), _bits(lb["leaf_hi"]))


@pytest.mark.parametrize("name,detail", SCENES)
def test_the_brute_force_against_the_witness(get_scene, name, detail):
    """2: (b)'s distance within the recorded bound of (c)'s, and the conditions the GPU tests lean on, counted in the reference: every kind of nearest feature is common,
    many queries hold a tie on the minimum d2_eff (the order is by gid), and box_d2 raises d2_tri somewhere.  Prototype figures: 1.7e-7 / 2.6e-7 worst error; this
    formula measured 1.65e-7 / 2.35e-7"""
    ref = _ref(get_scene, name, detail)
    duv, ids, point = ref["want"]
    st = ref["stats"]
    rec = json.load(open(STATS))[name]
    assert rec["allowed_abs_error"] == 4 * rec["measured_abs_error"]
    d64 = nc.witness(ref["T"], ref["q"])
    err = float(np.abs(duv[:, 0].astype(np.float64) - d64).max())
    print(f"\n[closest] {name}: worst |d32 - d64| {err:.3e} (allowed {rec['allowed_abs_error']:.3e}); features {[int((st['feature'] == f).sum()) for f in range(4)]}; "
          f"tied queries {int((st['ties'] >= 2).sum())}; raised pairs {st['raised']}")
    assert (ids[:, 0] >= 0).all() and err <= rec["allowed_abs_error"]
    assert (duv[:, 1] >= 0).all() and (duv[:, 2] >= 0).all() and (duv[:, 1].astype(np.float64) + duv[:, 2] <= 1 + 2.0 ** -23).all()
    for f in range(4):
        assert int((st["feature"] == f).sum()) >= 300, f"feature {f}"
    assert int((st["ties"] >= 2).sum()) >= 500
    assert st["raised"] > 0 and st["raised"] == rec["pairs_box_raises"]
    # the point is the nearest point: its own distance to p is d within the same bound
    assert np.abs(np.linalg.norm(point[:, :3].astype(np.float64) - ref["q"][:, :3], axis=1) - d64).max() <= rec["allowed_abs_error"]


def test_the_ctypes_descriptor_is_the_headers():
    """3: ArtPointQuery as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 56 bytes"""
    _layout_is_the_headers("ArtPointQuery", 56, ["points_dev", "duv_dev", "ids_dev", "point_dev", "hip_stream", "n", "cull_mask", "flags", "reserved"])


def test_presence():
    """4: art_closest_points(NULL, NULL) is ART_E_INVALID on any machine; the library exports it, the Rust bindings declare it, the header cites DESIGN.md 3.8, and
    Renderer has both methods"""
    from araytracingjourney_amd import _lib, renderer
    L = _lib.load()
    assert L.art_closest_points(None, None) == _lib.ART_E_INVALID and L.art_last_error().startswith(b"art_closest_points: ")
    assert L.art_closest_points(None, C.byref(_lib.ArtPointQuery(n=0))) == _lib.ART_E_INVALID
    so = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "art_closest_points" for line in syms.splitlines() if line.strip())
    rs = open(os.path.join(ROOT, "bindings", "art_sys.rs")).read()
    assert "pub fn art_closest_points(" in rs and "pub struct ArtPointQuery" in rs
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "DESIGN.md 3.8" in hdr and "### 3.8" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert callable(renderer.Renderer.closest_points) and callable(renderer.Renderer.closest_surface)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", SCENES)
def test_both_scenes_are_the_brute_forces(R, torch, get_scene, name, detail):
    """4096 queries with r = inf on a side stream: ids and bits; a permutation of the queries gives the permuted records; oversized out= tensors filled with a pattern
    are untouched beyond n; queries count neither as casts nor as rays"""
    ref = _ref(get_scene, name, detail)
    q, want = ref["q"], ref["want"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    d_q, d_p = _up(torch, q), _up(torch, q[perm])
    out = (torch.full((N + 70, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((N + 70, 2), PATTERN, dtype=torch.int32, device="cuda"),
           torch.full((N + 70, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, got_p, got_o = r.closest_points(d_q), r.closest_points(d_p), r.closest_points(d_q, out=out)
    s.synchronize()
    assert got[0].shape == (N, 4) and got[1].shape == (N, 2) and got[1].dtype == torch.int32 and got[2].shape == (N, 4) and got_o[0] is out[0]
    _same(_host(got), want, name)
    _same(_host(got_p), tuple(w[perm] for w in want), name + ", permuted")
    _same(tuple(t[:N].cpu().numpy() for t in out), want, name + ", out=")
    for t in out:
        assert (t[N:].view(torch.int32) == PATTERN).all(), "written beyond n"
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


def _below(d2):
    """the largest float32 r >= 0 with r*r < d2 (float32 product), elementwise; NaN where there is none (d2 == 0)"""
    d2 = np.asarray(d2, np.float32)
    r = np.sqrt(d2)
    for _ in range(4):
        r = np.where(r * r >= d2, np.nextafter(r, np.float32(-1)), r).astype(np.float32)
    up = np.nextafter(r, np.float32(np.inf))
    r = np.where(up * up < d2, up, r).astype(np.float32)
    ok = (r >= 0) & (r * r < d2)
    assert (ok | (d2 == 0)).all()
    return np.where(ok, r, np.float32(np.nan)).astype(np.float32)


@pytest.mark.gpu
def test_radii_and_dead_queries(R, torch, get_scene):
    """every query of Cornell's 4096 once per radius: inf, 0, -0.0, the exact d of the unbounded answer, the largest float whose square is below d2_eff (a miss), -1, NaN;
    then points with NaN / inf coordinates.  Miss records carry r as given, bit for bit"""
    ref = _ref(get_scene, "cornell", 1.0)
    q0, (duv0, ids0, _) = ref["q"][:1024], ref["want"]
    d = duv0[:1024, 0]
    d2 = np.maximum(ref["stats"]["d2"][:1024], 0).astype(np.float32)
    below = _below(d2)
    below = np.where(np.isnan(below), np.float32(-1.0), below).astype(np.float32)
    radii = [np.full(1024, np.inf, np.float32), np.zeros(1024, np.float32), np.full(1024, -0.0, np.float32), d, below, np.full(1024, -1.0, np.float32),
             np.full(1024, np.nan, np.float32), np.full(1024, -np.inf, np.float32)]
    q = np.repeat(q0, len(radii), axis=0)
    q[:, 3] = np.stack(radii, 1).reshape(-1)
    dead = q0[:64].copy()
    dead[:, 3] = np.inf
    for i in range(64):
        dead[i, i % 3] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
    q = np.concatenate([q, dead])
    want = nc.brute_force(ref["T"], q)
    k = len(radii)
    hit = want[1][:1024 * k, 0].reshape(1024, k) >= 0
    assert hit[:, 0].all() and hit[:, 3].sum() >= 512 and not hit[:, 4:].any() and (want[1][1024 * k:] == -1).all()   # the exact d is accepted more often than not; below it never
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    got = _ask(r, torch, q)
    _same(got, want, "radii")
    miss = got[1][:, 0] < 0
    assert np.array_equal(_bits(got[0][miss, 0]), _bits(q[miss, 3])) and not got[2][miss].any()
    r.close()


def _lattice_queries():
    g = lattice_coords(6).astype(np.float64)
    c = np.sort(np.concatenate([g, 0.5 * (g[:-1] + g[1:])]))   # lattice points, and the half-way coordinates: vertices, edge midpoints, face and cell centres
    x, y, z = [a.reshape(-1) for a in np.meshgrid(c, c, c, indexing="ij")]
    return queries(np.stack([x, y, z], 1))


def _hostile(which):
    """(scene, queries) of one hazard"""
    if which == "lattice":
        return lattice_scene(6), _lattice_queries()
    if which == "chain":
        sc, rays = chain_scene(64)
        on_axis = np.stack([2.0 ** -np.arange(0, 64, dtype=np.float64), np.zeros(64), np.zeros(64)], 1)
        far = np.array([[-1.0, 0.0, 0.0], [3.0, 0.5, 0.5], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1e-12, 1e-12, 0.0]])
        return sc, queries(np.concatenate([rays[:, 0:3], on_axis, on_axis * 0.75 + [0.0, 0.004, 0.002], far]))
    if which.startswith("soup:"):
        sc = degenerate_soup(256, which[5:])
        pts = random_rays(512, 11, radius=1.2)[:, 0:3]
        verts = nc.world_triangles(sc.primitives)["w"].reshape(-1, 3)[::5]
        return sc, queries(np.concatenate([pts, verts]))
    if which.startswith("segments:"):   # triangles of no area: segments (two equal vertices, or three in line) and points, among ordinary ones
        from araytracingjourney_amd import scenes
        rng = np.random.default_rng(5)
        mb = scenes.MeshBuilder()
        for k in range(96):
            a, b, c = rng.uniform(-0.8, 0.8, (3, 3)).astype(np.float32)
            kind = k % 6
            tri = [(a, b, c), (a, a, b), (a, b, b), (a, b, a), (a, a, a), (a, b, (a + (b - a) * np.float32(0.5)).astype(np.float32))][kind]
            mb.add([tuple(p) for p in tri], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
        sc = scenes.Scene("segments", [mb.finish(scenes.constant_texture((200, 180, 160)))], scenes.cornell().camera, scenes.cornell().lights)
        return sc, queries(np.concatenate([random_rays(512, 13, radius=1.0)[:, 0:3], nc.world_triangles(sc.primitives)["w"].reshape(-1, 3)]))
    if which == "one triangle":
        from araytracingjourney_amd import scenes
        mb = scenes.MeshBuilder()
        mb.add([(-0.5, -0.25, 0.1), (0.5, -0.25, 0.1), (0.0, 0.6, 0.3)], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
        sc = scenes.Scene("one", [mb.finish(scenes.constant_texture((200, 180, 160)))], scenes.cornell().camera, scenes.cornell().lights)
        q = queries(np.concatenate([random_rays(256, 3, radius=1.0)[:, 0:3], [(-0.5, -0.25, 0.1), (0.0, 0.6, 0.3), (0.0, -0.25, 0.1), (0.0, 0.0, 0.0)]]))
        q[::7, 3] = 0.5
        return sc, q
    raise KeyError(which)


HOSTILE = ["lattice", "chain", "soup:soup", "soup:flat", "soup:line", "soup:clusters", "soup:one point", "segments:", "one triangle"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_inputs(R, torch, which):
    """the generators of tests/helpers.py: a lattice with queries on lattice points, vertices and edge midpoints (d = 0 and many-way ties: the order is by gid), the chain
    of 64 nested slivers (stacks past their LDS part), the degenerate soups in every shape, triangles that are segments and points, a one-triangle scene"""
    sc, q = _hostile(which)
    T = nc.world_triangles(sc.primitives)
    want = nc.brute_force(T, q, stats=True)
    if which == "lattice":
        assert int((want[0][:, 0] == 0).sum()) >= 300 and int((want[3]["ties"] >= 4).sum()) >= 300
    if which == "segments:":
        assert int((want[3]["feature"] > 0).sum()) >= 300 and (want[1][:, 0] >= 0).all()
    r = R.renderer_for_scene(sc, (64, 64))
    _same(_ask(r, torch, q), want[:3], which)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s,offset", SIMILARITIES)
def test_world_scales(R, torch, get_scene, s, offset):
    """Cornell and 1024 queries under the similarities tests/test_walk_edges.py uses, applied to the data; half of the queries with a radius of the scene's scale"""
    rays = random_rays(1024, 7)
    sc, rays = similarity(get_scene("cornell"), rays, s=s, offset=offset)
    q = queries(rays[:, 0:3])
    q[::2, 3] = np.float32(0.3) * np.float32(s)
    want = nc.brute_force(nc.world_triangles(sc.primitives), q)
    assert 100 < int((want[1][:, 0] >= 0).sum()) < 1024 or s != 1.0
    r = R.renderer_for_scene(sc, (64, 64))
    _same(_ask(r, torch, q), want, f"scale {s}, offset {offset}")
    r.close()


def _card_scene(scenes, get_scene):
    """Cornell and two horizontal cards (tests/test_cast_multi.py's), the first with alpha 0 in every texel"""
    base = get_scene("cornell")
    prims = list(base.primitives)
    for y, a in ((0.3, 0), (-0.2, 255)):
        mb = scenes.MeshBuilder()
        scenes.quad(mb, (-0.35, y, -0.35), (0.7, 0.0, 0.0), (0.0, 0.0, 0.7), 2, 2, (1.0, 1.0))
        prims.append(mb.finish(_tex(a)))
    return scenes.Scene(base.name + "+cards", prims, base.camera, base.lights)


@pytest.mark.gpu
def test_masks_and_alpha(R, torch, scenes, get_scene):
    """primitive masks set after the build against cull masks 0xFF, 1, 2, 0x80 and 0 (which sees nothing); an alpha cutoff on a fully transparent card changes no record"""
    sc = _card_scene(scenes, get_scene)
    clear, solid = len(sc.primitives) - 2, len(sc.primitives) - 1
    q = queries(random_rays(2048, 5, radius=0.9)[:, 0:3])
    q[1::4, 3] = 0.25
    T = nc.world_triangles(sc.primitives)
    plain = nc.brute_force(T, q)
    assert int((plain[1][:, 0] == clear).sum()) > 50 and int((plain[1][:, 0] == solid).sum()) > 50
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    _same(_ask(r, torch, q), plain, "unmasked")
    m.set_alpha_cutoff(clear, 0.5); m.set_alpha_cutoff(solid, 0.5)
    _same(_ask(r, torch, q), plain, "with cutoffs: not tested")
    masks = {0: 0x01, 1: 0x02, solid: 0x03, clear: 0x02}
    for i, v in masks.items():
        m.set_mask(i, v)
    vis = np.array([masks.get(p, 0xFF) for p in range(len(sc.primitives))])
    seen = []
    for cull in (0xFF, 0x01, 0x02, 0x80, 0):
        want = nc.brute_force(T, q, vis=vis, cull=cull)
        got = _ask(r, torch, q, cull_mask=cull)
        _same(got, want, f"cull {cull:#x}")
        if cull == 0:
            assert (got[1] == -1).all() and np.array_equal(_bits(got[0][:, 0]), _bits(q[:, 3])) and not got[2].any()
        seen.append(got[1][:, 0].copy())
    assert not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[1])
    r.close()


@pytest.mark.gpu
def test_a_primitive_disabled_after_the_build_is_nowhere(R, torch, scenes, get_scene):
    """two primitives, one disabled after the build: its triangles are nowhere and its nodes all masked -- never returned, even with r = inf; then the other one too: nothing
    is left, every query misses; enabled again, the first answers return"""
    sc = _card_scene(scenes, get_scene)
    two = scenes.Scene("two", list(sc.primitives[-2:]), sc.camera, sc.lights)
    q = queries(random_rays(1024, 9, radius=0.8)[:, 0:3])
    r = R.Renderer((64, 64), tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(two.primitives)
    r.prepare_first_frame()
    both = nc.brute_force(nc.world_triangles(two.primitives), q)
    assert set(both[1][:, 0].tolist()) == {0, 1}
    _same(_ask(r, torch, q), both, "both")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 0) == 0 and not r.needs_build()
    want = nc.brute_force(nc.world_triangles(two.primitives, disabled=(1,)), q)
    assert (want[1][:, 0] == 0).all()
    _same(_ask(r, torch, q), want, "one disabled")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 0, 0) == 0
    got = _ask(r, torch, q)
    _same(got, nc.brute_force(nc.world_triangles(two.primitives, disabled=(0, 1)), q), "both disabled")
    assert (got[1] == -1).all() and np.isinf(got[0][:, 0]).all()
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 0, 1) == 0 and r._L.art_scene_set_primitive_enabled(r._ctx, 1, 1) == 0
    _same(_ask(r, torch, q), both, "enabled again")
    assert r.stats()["rebuilds"] == 0
    r.close()


@pytest.mark.gpu
def test_the_scene_as_of_the_call(R, torch, orc, get_scene):
    """Cornell's last primitive moved (art_scene_set_model_matrix), deformed (art_scene_set_vertices), disabled and enabled again on a built scene, a batch of queries behind
    every change on one stream with frames in flight and a single synchronisation at the end: every batch is the brute force over the world vertices as of its call, and the
    last frame is the oracle's for the final scene"""
    from conftest import assert_radiance_close
    sc = get_scene("cornell")
    q = _ref(get_scene, "cornell", 1.0)["q"][:2048]
    r = R.Renderer((64, 64), frames_in_flight=2, tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(list(sc.primitives[:-1]))
    r.add_model([sc.primitives[-1]])
    cam = r.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    for d in sc.lights:
        r.lights_mut().push_dict(d)
    r.prepare_first_frame()
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
    m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
    verts = np.array(moving.verts, np.float32)
    verts[:, 0:3] = verts[:, 0:3] * np.float32(0.75) + np.array([0.0, 0.05, 0.0], np.float32)
    states = [("built", sc.primitives, ()), ("moved", static + [P(moving.verts, moving.indices, moving.tex, m)], ()),
              ("deformed", static + [P(verts, moving.indices, moving.tex, m)], ()), ("disabled", static + [P(verts, moving.indices, moving.tex, m)], (len(static),)),
              ("enabled", static + [P(verts, moving.indices, moving.tex, m)], ())]
    model = r.models_mut()[1]
    pid = model.primitive_ids[0]
    d_q = _up(torch, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for what, _, _ in states:
        if what == "moved": model.set_model_matrix(m)
        elif what == "deformed": model.set_vertices(0, verts)
        elif what == "disabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 0) == 0
        elif what == "enabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 1) == 0
        with torch.cuda.stream(s):
            outs.append(r.closest_points(d_q))
        r.upload_state(); r.trace()
    r.sync(); s.synchronize()
    wants = [nc.brute_force(nc.world_triangles(prims, disabled=off), q) for _, prims, off in states]
    for (what, _, _), got, want in zip(states, outs, wants):
        _same(_host(got), want, what)
    assert not np.array_equal(wants[0][1], wants[3][1]) and not np.array_equal(_bits(wants[1][0]), _bits(wants[2][0]))
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 4 and r.cast_counts()["casts"] == 0
    S, lights, nl = oracle_for(orc, type(sc)(sc.name, states[-1][1], sc.camera, sc.lights))
    want = S.render(oracle_camera(orc, sc, 64, 64), lights, nl, 64, 64)
    assert_radiance_close(r.read_color()[..., :3], want["color"][..., :3], what="the frame behind the queries")
    r.close()


@pytest.mark.gpu
def test_the_ring_and_the_counts(R, torch, get_scene):
    """48 batches back to back on one side stream -- more than ART_CAST_POOL in flight -- all right; host_waits counts the lap when there was one and nothing else moves;
    hip_stream NULL runs on the context's cast stream with art_cast_sync as the fence; torch's default stream"""
    from araytracingjourney_amd import _lib
    ref = _ref(get_scene, "sponza_like", 0.05)
    q, want = ref["q"], ref["want"]
    assert 48 > _lib.ART_CAST_POOL
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_q = _up(torch, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        outs = [r.closest_points(d_q) for _ in range(48)]
        near = r.closest_points(d_q)[1][:, 0].to(torch.int64).sum()   # behind the queries on s: torch orders it
        assert int(near.item()) == int(want[1][:, 0].astype(np.int64).sum())
    s.synchronize()
    for i, got in enumerate(outs):
        _same(_host(got), want, f"batch {i}")
    cc = r.cast_counts()
    assert cc["casts"] == 0 and cc["rays"] == 0 and cc["host_waits"] <= 49 - _lib.ART_CAST_POOL
    got = r.closest_points(d_q)                                        # torch's default stream
    assert int(got[1][:, 0].to(torch.int64).sum().item()) == int(want[1][:, 0].astype(np.int64).sum())
    duv, ids, point = (torch.zeros((N, 4), device="cuda"), torch.zeros((N, 2), dtype=torch.int32, device="cuda"), torch.zeros((N, 4), device="cuda"))
    torch.cuda.synchronize()
    d = _lib.ArtPointQuery(points_dev=d_q.data_ptr(), duv_dev=duv.data_ptr(), ids_dev=ids.data_ptr(), point_dev=None, hip_stream=None, n=N, cull_mask=0xFF, flags=0, reserved=0)
    assert r._L.art_closest_points(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    assert np.array_equal(ids.cpu().numpy(), want[1]) and np.array_equal(_bits(duv.cpu().numpy()), _bits(want[0])) and not point.any()   # a null point_dev is not written
    # a cast beside them counts as ever
    r.cast_rays(_up(torch, random_rays(64, 7)))
    r.cast_sync()
    cc = r.cast_counts()
    assert cc["casts"] == 1 and cc["rays"] == 64
    r.close()


@pytest.mark.gpu
def test_closest_surface(R, torch, get_scene):
    """closest_points + resolve_hits on one side stream: resolve's pos (made from the object-space shading record and the matrix) lies within the recorded bound, scaled to
    the scene, of point_dev; a resolved record has w = 1, and miss records resolve to zeros"""
    ref = _ref(get_scene, "cornell", 1.0)
    bound = json.load(open(STATS))["cornell"]["allowed_abs_error"]
    q = np.array(ref["q"])
    q[::3, 3] = 0.05
    want = nc.brute_force(ref["T"], q)
    miss = want[1][:, 0] < 0
    assert 200 < int(miss.sum()) < N - 200
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        (duv, ids, point), surf = r.closest_surface(_up(torch, q), want=("pos", "ng"))
    s.synchronize()
    _same(_host((duv, ids, point)), want, "closest_surface")
    pos, ng, point = surf["pos"].cpu().numpy(), surf["ng"].cpu().numpy(), point.cpu().numpy()
    assert not pos[miss].any() and not ng[miss].any() and (pos[~miss, 3] == 1).all()
    assert np.abs(pos[~miss, :3].astype(np.float64) - point[~miss, :3]).max() <= bound
    assert np.abs(np.linalg.norm(ng[~miss, :3].astype(np.float64), axis=1) - 1).max() < 1e-5
    r.close()


@pytest.mark.gpu
def test_errors_change_nothing_and_enqueue_nothing(R, torch, get_scene):
    """every ART_E_INVALID case of include/art.h, and ART_E_STATE before the build and while the scene needs one: nothing is written, the counts stay, and every message
    names art_closest_points"""
    from araytracingjourney_amd import _lib
    sc = get_scene("cornell")
    r = R.Renderer((64, 64))
    r.add_model(sc.primitives)
    L, ctx = r._L, r._ctx
    n = 64
    pts = _up(torch, queries(random_rays(n + 1, 7)[:, 0:3]))
    duv = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    ids = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    point = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def desc(**kw):
        d = dict(points_dev=pts.data_ptr(), duv_dev=duv.data_ptr(), ids_dev=ids.data_ptr(), point_dev=point.data_ptr(), hip_stream=None, n=n, cull_mask=0xFF, flags=0, reserved=0)
        d.update(kw)
        return _lib.ArtPointQuery(**d)

    def code(d):
        return L.art_closest_points(ctx, C.byref(d) if d is not None else None)

    named = lambda: L.art_last_error().startswith(b"art_closest_points: ")   # noqa: E731
    assert code(desc()) == _lib.ART_E_STATE and named() and b"not built" in L.art_last_error()
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert L.art_closest_points(None, C.byref(desc())) == _lib.ART_E_INVALID and named()
    assert code(None) == _lib.ART_E_INVALID and named()
    bad = [desc(points_dev=None), desc(duv_dev=None), desc(ids_dev=None), desc(points_dev=pts.data_ptr() + 4), desc(points_dev=pts.data_ptr() + 8), desc(duv_dev=duv.data_ptr() + 8),
           desc(ids_dev=ids.data_ptr() + 4), desc(point_dev=point.data_ptr() + 8), desc(cull_mask=0x100), desc(cull_mask=0xFFFFFFFF), desc(flags=1), desc(flags=0x80000000),
           desc(reserved=1), desc(reserved=0x80000000), desc(n=_lib.ART_CAST_MAX_RAYS + 1), desc(n=0xFFFFFFFF)]
    for d in bad:
        assert code(d) == _lib.ART_E_INVALID and named(), (d.n, d.cull_mask, d.flags, d.reserved)
    r.cast_sync()
    assert r.cast_counts() == zero and not duv.any() and not ids.any() and not point.any()
    assert code(desc(n=0)) == 0 and code(desc(n=0, points_dev=None, duv_dev=None, ids_dev=None, point_dev=None)) == 0   # n = 0 is legal and enqueues nothing
    assert code(desc()) == 0
    r.cast_sync()
    assert r.cast_counts() == zero and (ids[:n, 0] >= 0).all() and not ids[n:].any() and not duv[n:].any() and not point[n:].any() and (point[:n, 3] == 1).all()
    # the wrapper's own checks
    for args, kw in (((pts.cpu(),), {}), ((pts.double(),), {}), ((pts[:, :3],), {}), ((pts,), dict(cull_mask=0x100)), ((pts,), dict(out=(duv[:8], ids, point))),
                     ((pts,), dict(out=(duv, ids.to(torch.int64), point))), ((pts,), dict(out=(duv, ids, point[:, :3])))):
        with pytest.raises((ValueError, TypeError)):
            r.closest_points(*args, **kw)
    r.add_model([sc.primitives[0]])   # a primitive added since the build: art_scene_needs_build
    assert r.needs_build() and code(desc()) == _lib.ART_E_STATE and named()
    with pytest.raises(_lib.ArtError):
        r.closest_points(pts)
    r.close()
