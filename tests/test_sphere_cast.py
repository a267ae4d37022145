"""art_cast_spheres (include/art.h): where a ball moving along a ray first touches the scene, defined exactly and checked bit for bit.

The reference is tests/np_sweep.py: the semantics as a numpy float32 brute force over every (ray, triangle) pair -- what the device must write, ids and bits.  The CPU
tests check it against the same function in float64 and against an independent fp64 witness of the distance (np_closest.witness) before the GPU tests lean on it.

Measured, random_rays(4096, 7) with a radius of 0.05: worst |t32 - t64| 7.52e-5 on cornell 1.0 and 4.44e-5 on sponza_like 0.05 (medians 4.7e-8 / 6.9e-8; no ray changes
between hit and miss); four times the worst is allowed (tests/golden/sphere_cast.stats.json).  The witness' distance at c(t_eff) lies -1.2e-5 .. +9.4e-6 round the radius
on cornell and -2.3e-5 .. +1.8e-5 on sponza_like."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import np_closest as nc
import np_sweep as ns
from helpers import RANGES, SIMILARITIES, chain_scene, degenerate_soup, lattice_rays, lattice_scene, random_rays, similarity, with_ranges
from helpers import _bits, _host, R, torch, _up  # noqa: F401  (R, torch: module fixtures)
from test_closest_points import _card_scene, _layout_is_the_headers, _hostile as _closest_hostile   # Cornell with two cards; gcc's layout of a header struct; its hostile scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = os.path.join(ROOT, "tests", "golden", "sphere_cast.stats.json")
PATTERN = -0x5A5A5A5B   # tests/test_cast.py's: what oversized output buffers are filled with
N = 4096
RHO = 0.05
SCENES = [("cornell", 1.0), ("sponza_like", 0.05)]


_REF = {}


def _ref(get_scene, name, detail):
    """the scene, its triangles, the rays (random_rays(4096, 7)) and the reference's records for a radius of 0.05 with its statistics: computed once, shared, never written"""
    key = (name, detail)
    if key not in _REF:
        sc = get_scene(name, detail)
        T = nc.world_triangles(sc.primitives)
        rays = random_rays(N, 7)
        tuv, ids, point, st = ns.brute_force(T, rays, RHO, stats=True)
        for a in (rays, tuv, ids, point):
            a.setflags(write=False)
        _REF[key] = dict(scene=sc, T=T, rays=rays, want=(tuv, ids, point), stats=st)
    return _REF[key]


def _same(got, want, what=""):
    """ids, the bits of t, u, v, a fourth word of 0, the bits of the point"""
    (tuv, ids, point), (rtuv, rids, rpoint) = got, want
    assert tuv.shape == rtuv.shape and ids.shape == rids.shape and point.shape == rpoint.shape, what
    assert np.array_equal(ids, rids), f"{what}: the ids of {int((ids != rids).any(axis=1).sum())} of {ids.shape[0]} rays differ (first: {np.flatnonzero((ids != rids).any(axis=1))[:5]})"
    bad = (_bits(tuv)[:, :3] != _bits(rtuv)[:, :3]).any(axis=1)
    assert not bad.any(), f"{what}: t, u, v of {int(bad.sum())} rays differ (first: {np.flatnonzero(bad)[:5]}: {tuv[bad][:2]} for {rtuv[bad][:2]})"
    assert not _bits(tuv)[:, 3].any(), f"{what}: the fourth word is not 0"
    assert np.array_equal(_bits(point), _bits(rpoint)), f"{what}: the points differ"


def _ask(r, torch, rays, rho, **kw):
    got = r.cast_spheres(_up(torch, rays), rho, **kw)
    torch.cuda.synchronize()
    return _host(got)


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,detail", SCENES)
def test_the_reference_against_itself_in_float64(get_scene, name, detail):
    """1: the reference's t within the recorded bound of the same function in float64 on the same float32 inputs: four times the worst |t32 - t64| measured, recorded per
    scene and measured again here.  Rays whose hit / miss status differs between the precisions are left out; at most 1 % may (measured: none)"""
    ref = _ref(get_scene, name, detail)
    tuv, ids, _ = ref["want"]
    t64, ids64, _ = ns.brute_force(ref["T"], ref["rays"], RHO, dtype=np.float64)
    rec = json.load(open(STATS))[name]
    assert rec["allowed_abs_error"] == 4 * rec["measured_abs_error"] and rec["radius"] == RHO and rec["rays"] == N
    hit, hit64 = ids[:, 0] >= 0, ids64[:, 0] >= 0
    differ = int((hit != hit64).sum())
    both = hit & hit64
    e = np.abs(tuv[both, 0].astype(np.float64) - t64[both, 0])
    print(f"\n[sweep] {name}: worst |t32 - t64| {e.max():.3e} (recorded {rec['measured_abs_error']:.3e}, allowed {rec['allowed_abs_error']:.3e}), median {np.median(e):.1e}; "
          f"{int(both.sum())} hits, {differ} rays change status")
    assert differ <= N // 100 and int(both.sum()) >= 3000
    assert float(e.max()) <= rec["allowed_abs_error"]


@pytest.mark.parametrize("name,detail", SCENES)
def test_an_independent_witness_of_the_distance(get_scene, name, detail):
    """2: np_closest.witness (Ericson's region walk in fp64: it shares nothing with the formula) at c(t_eff): within the allowance of the radius for every hit not won by S,
    at most the radius + the allowance for an S hit; and for (up to) 200 misses 65 samples along the ray each stay farther than the radius"""
    ref = _ref(get_scene, name, detail)
    (tuv, ids, _), st, rays = ref["want"], ref["stats"], ref["rays"]
    allow = json.load(open(STATS))[name]["allowed_abs_error"]   # (|d| = 1 for these rays: an error in t is one in distance)
    hit = ids[:, 0] >= 0
    d = nc.witness(ref["T"], ns.centres(rays[hit], tuv[hit, 0]))
    s = st["feature"][hit] == 0
    print(f"\n[sweep] {name}: witness - radius {float((d[~s] - RHO).min()):+.2e} .. {float((d[~s] - RHO).max()):+.2e} over {int((~s).sum())} contacts; S hits at most {float((d[s] - RHO).max()):+.2e}")
    assert np.abs(d[~s] - RHO).max() <= allow and (d[s] <= RHO + allow).all()
    miss = np.flatnonzero(~hit)[:200]
    assert miss.size >= 100
    ts = np.linspace(rays[miss, 3].astype(np.float64), rays[miss, 7].astype(np.float64), 65, axis=1).reshape(-1)
    dm = nc.witness(ref["T"], ns.centres(np.repeat(rays[miss], 65, axis=0), ts))
    print(f"[sweep] {name}: {miss.size} misses, nearest sample {float(dm.min()):.4f}")
    assert (dm > RHO).all()


def test_the_conditions_the_gpu_tests_lean_on(get_scene):
    """3: counted in the reference.  On sponza_like every feature wins -- S and each edge at least 100 rays, each vertex at least 10 -- at least 300 rays hold a tie on the
    minimum t_eff (the order is by gid) and the box raises t_tri somewhere; on Cornell S, F and each edge win at least 50 rays.  Measured: S F E01 E02 E12 V0 V1 V2 =
    298 / 2717 / 170 / 154 / 478 / 23 / 30 / 72 with 762 ties and 1197 raised pairs; Cornell 222 / 2981 / 119 / 139 / 133 / 2 / 7 / 5"""
    recs = json.load(open(STATS))
    for name, detail in SCENES:
        st = _ref(get_scene, name, detail)["stats"]
        wins = [int((st["feature"] == f).sum()) for f in range(8)]
        ties = int((st["ties"] >= 2).sum())
        print(f"\n[sweep] {name}: wins {dict(zip(ns.FEATURES, wins))}; tied rays {ties}; raised pairs {st['raised']}")
        assert wins == recs[name]["wins_S_F_E01_E02_E12_V0_V1_V2"] and ties == recs[name]["rays_with_ties"] and st["raised"] == recs[name]["pairs_box_raises"]
        if name == "sponza_like":
            assert all(w > 0 for w in wins) and wins[0] >= 100 and min(wins[2:5]) >= 100 and min(wins[5:8]) >= 10 and ties >= 300 and st["raised"] >= 1
        else:
            assert wins[0] >= 50 and wins[1] >= 50 and min(wins[2:5]) >= 50


def test_the_ctypes_descriptor_is_the_headers():
    """4: ArtSphereCast as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 56 bytes"""
    cls = _layout_is_the_headers("ArtSphereCast", 56, ["rays_dev", "tuv_dev", "ids_dev", "point_dev", "hip_stream", "n", "cull_mask", "flags", "radius"])
    assert cls._fields_[-1][1] is C.c_float


def test_presence():
    """5: art_cast_spheres(NULL, NULL) is ART_E_INVALID on any machine; the library exports it, the Rust bindings declare it, the header cites DESIGN.md 3.9, and
    Renderer has both methods"""
    from araytracingjourney_amd import _lib, renderer
    L = _lib.load()
    assert L.art_cast_spheres(None, None) == _lib.ART_E_INVALID and L.art_last_error().startswith(b"art_cast_spheres: ")
    assert L.art_cast_spheres(None, C.byref(_lib.ArtSphereCast(n=0))) == _lib.ART_E_INVALID
    so = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "art_cast_spheres" for line in syms.splitlines() if line.strip())
    rs = open(os.path.join(ROOT, "bindings", "art_sys.rs")).read()
    assert "pub fn art_cast_spheres(" in rs and "pub struct ArtSphereCast" in rs
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "DESIGN.md 3.9" in hdr and "### 3.9" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert callable(renderer.Renderer.cast_spheres) and callable(renderer.Renderer.cast_spheres_surface)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", SCENES)
def test_both_scenes_are_the_references(R, torch, get_scene, name, detail):
    """6: 4096 rays with a radius of 0.05 on a side stream: ids and bits; a permutation of the rays gives the permuted records; oversized out= tensors filled with a pattern
    are untouched beyond n; the sweeps count as casts and rays"""
    ref = _ref(get_scene, name, detail)
    rays, want = ref["rays"], ref["want"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    d_r, d_p = _up(torch, rays), _up(torch, rays[perm])
    out = (torch.full((N + 70, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((N + 70, 2), PATTERN, dtype=torch.int32, device="cuda"),
           torch.full((N + 70, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, got_p, got_o = r.cast_spheres(d_r, RHO), r.cast_spheres(d_p, RHO), r.cast_spheres(d_r, RHO, out=out)
    s.synchronize()
    assert got[0].shape == (N, 4) and got[1].shape == (N, 2) and got[1].dtype == torch.int32 and got[2].shape == (N, 4) and got_o[0] is out[0]
    _same(_host(got), want, name)
    _same(_host(got_p), tuple(w[perm] for w in want), name + ", permuted")
    _same(tuple(t[:N].cpu().numpy() for t in out), want, name + ", out=")
    for t in out:
        assert (t[N:].view(torch.int32) == PATTERN).all(), "written beyond n"
    assert r.cast_counts() == dict(casts=3, rays=3 * N, host_waits=0)
    r.close()


@pytest.mark.gpu
def test_radii_and_dead_rays(R, torch, get_scene):
    """7: Cornell's 4096 rays once each at radius 0, 1e-6, 0.05 and 3 -- larger than the scene: every live ray is an S hit at tmin, or a miss where tmin >= tmax -- with a
    block of rays behind them that are dead (NaN or inf in o or d, a NaN tmax), have an empty range, or run to tmax = +inf / -inf.  Miss records carry tmax as given"""
    ref = _ref(get_scene, "cornell", 1.0)
    extra = np.array(ref["rays"][:96])
    for i in range(48):
        extra[i, (0, 1, 2, 4, 5, 6)[i % 6]] = (np.nan, np.inf, -np.inf)[(i // 6) % 3]
    extra[48:64, 7] = np.nan
    extra[64:72, 3], extra[64:72, 7] = 2.0, 1.0
    extra[72:80, 3], extra[72:80, 7] = 1.0, 1.0
    extra[80:88, 7] = np.inf
    extra[88:96, 7] = -np.inf
    rays = np.concatenate([ref["rays"], extra])
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    for rho in (0.0, 1e-6, RHO, 3.0):
        want = ns.brute_force(ref["T"], rays, rho, stats=True)
        if rho == RHO:
            _same(tuple(w[:N] for w in want[:3]), ref["want"], "the shared reference")
        if rho == 3.0:
            assert (want[3]["feature"][:N] == 0).all() and np.array_equal(want[0][:N, 0], rays[:N, 3]) and (want[3]["feature"][N + 80:N + 88] == 0).all()
        assert (want[1][N:N + 80] == -1).all() and (want[1][N + 88:] == -1).all() and int((want[1][:N, 0] >= 0).sum()) >= 3000
        got = _ask(r, torch, rays, rho)
        _same(got, want[:3], f"radius {rho}")
        miss = got[1][:, 0] < 0
        assert np.array_equal(_bits(got[0][miss, 0]), _bits(rays[miss, 7])) and not got[2][miss].any()
    r.close()


def _flat(scenes, mb, name):
    return scenes.Scene(name, [mb.finish(scenes.constant_texture((200, 180, 160)))], scenes.cornell().camera, scenes.cornell().lights)


def _hostile(which, scenes, get_scene):
    """(scene, rays) of one hazard"""
    if which == "lattice":
        return lattice_scene(6), lattice_rays(6)
    if which == "chain":
        return chain_scene(64)
    if which.startswith("soup:"):
        return degenerate_soup(256, which[5:]), random_rays(512, 11, radius=1.2)
    if which == "segments":   # triangles of no area: segments (two equal vertices, or three in line) and points, among ordinary ones
        return _closest_hostile("segments:")[0], random_rays(1024, 13, radius=1.0)
    if which == "d = 0":      # a ball that does not move: at the reference's contact centres (the distance IS the radius, up to rounding), on vertices (distance 0) and anywhere
        ref = _ref(get_scene, "cornell", 1.0)
        hit = ref["want"][1][:, 0] >= 0
        c = ns.centres(ref["rays"][hit][:512], ref["want"][0][hit, 0][:512])[:, 0:3]
        o = np.concatenate([c, ref["T"]["w"].reshape(-1, 3), ref["rays"][:256, 0:3]]).astype(np.float32)
        rays = np.zeros((o.shape[0], 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 7] = o, 0.001, 100.0
        rays[1::2, 4:7] = -0.0
        return ref["scene"], rays
    if which == "ranges":     # tmin > tmax, tmax = inf, a negative tmin, infinite and NaN tmin ...: every [tmin, tmax] of tests/helpers.py
        assert (2.0, 1.0) in RANGES and (0.001, np.inf) in RANGES and (-5.0, 100.0) in RANGES
        return get_scene("cornell"), with_ranges(random_rays(256, 7), RANGES)
    if which == "one triangle":   # the tree's only node is scaled to a point when the triangle is one: three absent children whose byte boxes are inverted
        mb = scenes.MeshBuilder()
        mb.add([(0.25, 0.25, 0.25), (0.25, 0.25, 0.25), (0.25, 0.25, 0.25)], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
        rays = random_rays(512, 3, radius=1.0)
        aim = np.array([0.25, 0.25, 0.25], np.float32) - rays[::2, 0:3]
        rays[::2, 4:7] = aim / np.linalg.norm(aim, axis=1, keepdims=True)    # every second ray at the point itself
        return _flat(scenes, mb, "one point"), rays
    if which == "one real triangle":
        return _closest_hostile("one triangle")[0], random_rays(512, 3, radius=1.0)
    raise KeyError(which)


HOSTILE = ["soup:soup", "soup:flat", "soup:one point", "segments", "lattice", "chain", "d = 0", "ranges", "one triangle", "one real triangle"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_inputs(R, torch, scenes, get_scene, which):
    """8: at a radius of 0.05 and of 0 -- the degenerate soups, triangles that are segments and points (their edges and vertices answer; nothing divides by 0), the lattice
    with axis-parallel rays from lattice points, the chain of 64 nested slivers (stacks past their LDS part), d = 0, every range of tests/helpers.py, and one-triangle
    scenes: a point (the only node is scaled to a point, its absent children's inverted boxes inflate to ordinary ones) and an ordinary triangle"""
    sc, rays = _hostile(which, scenes, get_scene)
    T = nc.world_triangles(sc.primitives)
    r = R.renderer_for_scene(sc, (64, 64))
    for rho in (RHO, 0.0):
        want = ns.brute_force(T, rays, rho, stats=True)
        hits = int((want[1][:, 0] >= 0).sum())
        if which == "segments" and rho == RHO:
            assert int((want[3]["feature"] >= 2).sum()) >= 100
        if which == "d = 0":
            # (at radius 0 nothing answers: a point ON a box's plane is not inside 1.1's slab once d = 0 is clamped to 1e-20 -- the residue of o * 1e20 decides)
            assert set(np.unique(want[3]["feature"]).tolist()) <= {-1, 0} and (hits >= 300 or rho == 0.0)
        if which in ("lattice", "chain", "one triangle", "one real triangle", "ranges") and rho == RHO:
            assert hits >= (50 if which == "one real triangle" else 100), hits
        _same(_ask(r, torch, rays, rho), want[:3], f"{which}, radius {rho}")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s,offset", SIMILARITIES)
def test_world_scales(R, torch, get_scene, s, offset):
    """9: Cornell and 1024 rays under the similarities tests/test_walk_edges.py uses, applied to the data; the radius is scaled with the scene"""
    sc, rays = similarity(get_scene("cornell"), random_rays(1024, 7), s=s, offset=offset)
    rho = float(np.float32(RHO) * np.float32(s))
    want = ns.brute_force(nc.world_triangles(sc.primitives), rays, rho)
    assert int((want[1][:, 0] >= 0).sum()) >= 700
    r = R.renderer_for_scene(sc, (64, 64))
    _same(_ask(r, torch, rays, rho), want, f"scale {s}, offset {offset}")
    r.close()


@pytest.mark.gpu
def test_masks_and_alpha(R, torch, scenes, get_scene):
    """10: primitive masks set after the build against cull masks 0xFF, 1, 2, 0x80 and 0 (which sees nothing); an alpha cutoff on a fully transparent card changes no
    record: the card is still hit"""
    sc = _card_scene(scenes, get_scene)
    clear, solid = len(sc.primitives) - 2, len(sc.primitives) - 1
    rays = random_rays(2048, 5)
    T = nc.world_triangles(sc.primitives)
    plain = ns.brute_force(T, rays, RHO)
    assert int((plain[1][:, 0] == clear).sum()) > 50 and int((plain[1][:, 0] == solid).sum()) > 50
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    _same(_ask(r, torch, rays, RHO), plain, "unmasked")
    m.set_alpha_cutoff(clear, 0.5); m.set_alpha_cutoff(solid, 0.5)
    _same(_ask(r, torch, rays, RHO), plain, "with cutoffs: not tested")
    masks = {0: 0x01, 1: 0x02, solid: 0x03, clear: 0x02}
    for i, v in masks.items():
        m.set_mask(i, v)
    vis = np.array([masks.get(p, 0xFF) for p in range(len(sc.primitives))])
    seen = []
    for cull in (0xFF, 0x01, 0x02, 0x80, 0):
        want = ns.brute_force(T, rays, RHO, vis=vis, cull=cull)
        got = _ask(r, torch, rays, RHO, cull_mask=cull)
        _same(got, want, f"cull {cull:#x}")
        if cull == 0:
            assert (got[1] == -1).all() and np.array_equal(_bits(got[0][:, 0]), _bits(rays[:, 7])) and not got[2].any()
        seen.append(got[1][:, 0].copy())
    assert not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[1])
    r.close()


@pytest.mark.gpu
def test_a_primitive_disabled_after_the_build_is_nowhere(R, torch, scenes, get_scene):
    """10: two primitives, one disabled after the build: its triangles are nowhere and its nodes all masked -- never returned, even with tmax = inf and a large radius; then
    the other one too: every ray misses; enabled again, the first answers return"""
    sc = _card_scene(scenes, get_scene)
    two = scenes.Scene("two", list(sc.primitives[-2:]), sc.camera, sc.lights)
    rays = random_rays(1024, 9, radius=0.8)
    rays[::2, 7] = np.inf
    r = R.Renderer((64, 64), tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(two.primitives)
    r.prepare_first_frame()
    for rho in (RHO, 0.75):
        both = ns.brute_force(nc.world_triangles(two.primitives), rays, rho)
        assert set(both[1][:, 0].tolist()) >= {0, 1}
        _same(_ask(r, torch, rays, rho), both, "both")
        assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 0) == 0 and not r.needs_build()
        want = ns.brute_force(nc.world_triangles(two.primitives, disabled=(1,)), rays, rho)
        assert set(want[1][:, 0].tolist()) <= {0, -1} and (want[1][:, 0] == 0).sum() > 100
        _same(_ask(r, torch, rays, rho), want, "one disabled")
        assert r._L.art_scene_set_primitive_enabled(r._ctx, 0, 0) == 0
        got = _ask(r, torch, rays, rho)
        _same(got, ns.brute_force(nc.world_triangles(two.primitives, disabled=(0, 1)), rays, rho), "both disabled")
        assert (got[1] == -1).all() and np.array_equal(_bits(got[0][:, 0]), _bits(rays[:, 7]))
        assert r._L.art_scene_set_primitive_enabled(r._ctx, 0, 1) == 0 and r._L.art_scene_set_primitive_enabled(r._ctx, 1, 1) == 0
        _same(_ask(r, torch, rays, rho), both, "enabled again")
    assert r.stats()["rebuilds"] == 0
    r.close()


@pytest.mark.gpu
def test_the_scene_as_of_the_call(R, torch, get_scene):
    """11: Cornell's last primitive moved (art_scene_set_model_matrix) and moved again on a built scene, a sweep behind every change on one side stream with no
    synchronisation in between: every sweep is the reference over the world vertices as of its call"""
    sc = get_scene("cornell")
    rays = _ref(get_scene, "cornell", 1.0)["rays"][:2048]
    r = R.Renderer((64, 64), tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(list(sc.primitives[:-1]))
    r.add_model([sc.primitives[-1]])
    r.prepare_first_frame()
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    mats = [None]
    for step in ((0.06, 0.03, -0.06), (-0.1, 0.0, 0.08)):
        m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
        m[:, 3] += np.array(step, np.float32)
        mats.append(m)
    model = r.models_mut()[1]
    d_r = _up(torch, rays)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for m in mats:
        if m is not None:
            model.set_model_matrix(m)
        with torch.cuda.stream(s):
            outs.append(r.cast_spheres(d_r, RHO))
    s.synchronize()
    wants = [ns.brute_force(nc.world_triangles(static + [moving if m is None else P(moving.verts, moving.indices, moving.tex, m)]), rays, RHO) for m in mats]
    for i, (got, want) in enumerate(zip(outs, wants)):
        _same(_host(got), want, f"state {i}")
    assert not np.array_equal(_bits(wants[0][0]), _bits(wants[1][0])) and not np.array_equal(_bits(wants[1][0]), _bits(wants[2][0]))
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 2 and r.cast_counts()["casts"] == 3
    r.close()


@pytest.mark.gpu
def test_the_ring_and_the_counts(R, torch, get_scene):
    """11: 48 sweeps back to back on one side stream -- more than ART_CAST_POOL in flight -- all right; host_waits counts the lap when there was one; casts and rays count
    every sweep; hip_stream NULL runs on the context's cast stream with art_cast_sync as the fence and a null point_dev is not written; torch's default stream"""
    from araytracingjourney_amd import _lib
    ref = _ref(get_scene, "sponza_like", 0.05)
    rays, want = ref["rays"], ref["want"]
    assert 48 > _lib.ART_CAST_POOL
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_r = _up(torch, rays)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    total = int(want[1][:, 0].astype(np.int64).sum())
    with torch.cuda.stream(s):
        outs = [r.cast_spheres(d_r, RHO) for _ in range(48)]
        assert int(r.cast_spheres(d_r, RHO)[1][:, 0].to(torch.int64).sum().item()) == total   # behind the sweeps on s: torch orders it
    s.synchronize()
    for i, got in enumerate(outs):
        _same(_host(got), want, f"sweep {i}")
    cc = r.cast_counts()
    assert cc["casts"] == 49 and cc["rays"] == 49 * N and cc["host_waits"] <= 49 - _lib.ART_CAST_POOL
    assert int(r.cast_spheres(d_r, RHO)[1][:, 0].to(torch.int64).sum().item()) == total          # torch's default stream
    tuv, ids, point = (torch.zeros((N, 4), device="cuda"), torch.zeros((N, 2), dtype=torch.int32, device="cuda"), torch.zeros((N, 4), device="cuda"))
    torch.cuda.synchronize()
    d = _lib.ArtSphereCast(rays_dev=d_r.data_ptr(), tuv_dev=tuv.data_ptr(), ids_dev=ids.data_ptr(), point_dev=None, hip_stream=None, n=N, cull_mask=0xFF, flags=0, radius=RHO)
    assert r._L.art_cast_spheres(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    assert np.array_equal(ids.cpu().numpy(), want[1]) and np.array_equal(_bits(tuv.cpu().numpy()), _bits(want[0])) and not point.any()
    cc = r.cast_counts()
    assert cc["casts"] == 51 and cc["rays"] == 51 * N
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", SCENES)
def test_composition(R, torch, get_scene, name, detail):
    """12: closest_points at c(t_eff) of the non-S hits of test 6 returns a distance within the recorded allowance of the radius; cast_spheres_surface is the cast and one
    resolve of its records"""
    ref = _ref(get_scene, name, detail)
    (tuv, ids, _), st, rays = ref["want"], ref["stats"], ref["rays"]
    allow = json.load(open(STATS))[name]["allowed_abs_error"]
    sel = (ids[:, 0] >= 0) & (st["feature"] != 0)
    q = ns.centres(rays[sel], tuv[sel, 0]).astype(np.float32)
    q[:, 3] = np.inf
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    duv = r.closest_points(_up(torch, q))[0]
    torch.cuda.synchronize()
    d = duv.cpu().numpy()[:, 0].astype(np.float64)
    print(f"\n[sweep] {name}: closest_points at c(t_eff) - radius {float((d - RHO).min()):+.2e} .. {float((d - RHO).max()):+.2e} over {d.size} contacts (allowed {allow:.2e})")
    assert np.abs(d - RHO).max() <= allow
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    d_r = _up(torch, rays)
    with torch.cuda.stream(s):
        got, surf = r.cast_spheres_surface(d_r, RHO, want=("pos", "ng", "uv"))
        sep = r.resolve_hits(got[0], got[1], ("pos", "ng", "uv"))
    s.synchronize()
    _same(_host(got), ref["want"], "cast_spheres_surface")
    assert set(surf) == set(sep) == {"pos", "ng", "uv"}
    for k in surf:
        assert torch.equal(surf[k].view(torch.int32), sep[k].view(torch.int32)), k
    miss = ids[:, 0] < 0
    pos = surf["pos"].cpu().numpy()
    assert not pos[miss].any() and (pos[~miss, 3] == 1).all()
    r.close()


@pytest.mark.gpu
def test_errors_change_nothing_and_enqueue_nothing(R, torch, get_scene):
    """13: every ART_E_INVALID case of include/art.h, and ART_E_STATE before the build and while the scene needs one: nothing is written, the counts stay, and every message
    names art_cast_spheres"""
    from araytracingjourney_amd import _lib
    sc = get_scene("cornell")
    r = R.Renderer((64, 64))
    r.add_model(sc.primitives)
    L, ctx = r._L, r._ctx
    n = 64
    rays = _up(torch, random_rays(n + 1, 7))
    tuv = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    ids = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    point = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def desc(**kw):
        d = dict(rays_dev=rays.data_ptr(), tuv_dev=tuv.data_ptr(), ids_dev=ids.data_ptr(), point_dev=point.data_ptr(), hip_stream=None, n=n, cull_mask=0xFF, flags=0, radius=RHO)
        d.update(kw)
        return _lib.ArtSphereCast(**d)

    def code(d):
        return L.art_cast_spheres(ctx, C.byref(d) if d is not None else None)

    named = lambda: L.art_last_error().startswith(b"art_cast_spheres: ")   # noqa: E731
    assert code(desc()) == _lib.ART_E_STATE and named() and b"not built" in L.art_last_error()
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert L.art_cast_spheres(None, C.byref(desc())) == _lib.ART_E_INVALID and named()
    assert code(None) == _lib.ART_E_INVALID and named()
    bad = [desc(rays_dev=None), desc(tuv_dev=None), desc(ids_dev=None), desc(rays_dev=rays.data_ptr() + 4), desc(rays_dev=rays.data_ptr() + 8), desc(tuv_dev=tuv.data_ptr() + 8),
           desc(ids_dev=ids.data_ptr() + 4), desc(point_dev=point.data_ptr() + 8), desc(radius=float("nan")), desc(radius=-1e-30), desc(radius=-1.0), desc(radius=float("inf")),
           desc(radius=float("-inf")), desc(cull_mask=0x100), desc(cull_mask=0xFFFFFFFF), desc(flags=1), desc(flags=0x80000000), desc(n=_lib.ART_CAST_MAX_RAYS + 1), desc(n=0xFFFFFFFF)]
    for d in bad:
        assert code(d) == _lib.ART_E_INVALID and named(), (d.n, d.cull_mask, d.flags, d.radius)
    r.cast_sync()
    assert r.cast_counts() == zero and not tuv.any() and not ids.any() and not point.any()
    assert code(desc(n=0)) == 0 and code(desc(n=0, rays_dev=None, tuv_dev=None, ids_dev=None, point_dev=None)) == 0   # n = 0 is legal and enqueues nothing
    assert r.cast_counts() == zero
    assert code(desc(radius=-0.0)) == 0                                                                                # -0.0 is 0
    r.cast_sync()
    want = ns.brute_force(nc.world_triangles(sc.primitives), rays[:n].cpu().numpy(), 0.0)
    _same((tuv[:n].cpu().numpy(), ids[:n].cpu().numpy(), point[:n].cpu().numpy()), want, "radius -0.0")
    assert r.cast_counts() == dict(casts=1, rays=n, host_waits=0) and not ids[n:].any() and not tuv[n:].any() and not point[n:].any()
    # the wrapper's own checks
    for args, kw in (((rays.cpu(), RHO), {}), ((rays.double(), RHO), {}), ((rays[:, :4], RHO), {}), ((rays, -1.0), {}), ((rays, float("nan")), {}), ((rays, float("inf")), {}),
                     ((rays, RHO), dict(cull_mask=0x100)), ((rays, RHO), dict(out=(tuv[:8], ids, point))), ((rays, RHO), dict(out=(tuv, ids.to(torch.int64), point))),
                     ((rays, RHO), dict(out=(tuv, ids, point[:, :3])))):
        with pytest.raises((ValueError, TypeError)):
            r.cast_spheres(*args, **kw)
    r.add_model([sc.primitives[0]])   # a primitive added since the build: art_scene_needs_build
    assert r.needs_build() and code(desc()) == _lib.ART_E_STATE and named()
    with pytest.raises(_lib.ArtError):
        r.cast_spheres(rays, RHO)
    r.close()
