"""art_cast_crossings (include/art.h): how many surfaces each ray enters and leaves, uncapped, and Renderer.points_inside / signed_distance /
voxelize_solid over it.

Nothing on the device has a tolerance: the records are pairs of integers and every comparison is for equality.  The reference (tests/np_crossings.py) takes WHICH
triangles accept a ray from the oracle, one triangle at a time (test_cast_multi.hit_table: accept() is structure-independent), and the orientation of
each accepted pair from det = dot3(e1, cross3(d, e2)) restated in float32 with exact fmaf (np_sweep._fma) on np_closest.world_triangles' edges; a float64 witness that
shares none of that code vouches for the sign outside a band of 1e-6 * |e1| * |d x e2|.  The tables, scenes and rays are the other query modules' (their caches: nothing
is computed twice in a session), each read-only.

Mutation checks, on scratch builds of the library (GPU tests of this module that fail, of 49):
    det's comparison flipped (det < 0 counts as an entry)          47: all but the errors and the dead batch
    the leaf step's take sets tbest = teff (the closest walk's)    46: all but those two and the single triangles (one surface a ray)
    TravBase::pop skips spilled entries                            24: the chain and the clump on every form, sponza_like (the records, every knob), three soups
"""
import ctypes as C
import os

import numpy as np
import pytest

import np_closest as nc
import np_crossings as nx
import test_cast_multi as tm
import test_query_forms as tq
from helpers import RANGES, degenerate_soup, lattice_rays, lattice_scene, pending_on_first_descent_wide, random_rays, with_ranges
from helpers import _dead_rays, _layout_is_the_headers, R, _tex_flat as _tex, torch, _up  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = tm.PATTERN      # tests/test_cast.py's: what oversized output buffers are filled with
N = tm.N                  # 4096
LDS_DEPTH = tq.LDS_DEPTH  # kCastLds of art_query_rays.hip
WHO = b"art_cast_crossings: "


# ---- references: made once, shared, never written ------------------------------------------------------------------------------------------------------------------
_WANT, _SOLID = {}, {}


def _scene_ref(orc, get_scene, name):
    """cornell | sponza_like at 0.05 with test_cast_multi's 4097 rays and table: (scene, rays, tab, T, the (4097, 2) records)"""
    if name not in _WANT:
        ref = tm._ref(orc, get_scene, name, 0.05 if name == "sponza_like" else 1.0)
        T = nc.world_triangles(ref["scene"].primitives)
        want = nx.crossings(ref["tab"], T, ref["rays"])
        want.setflags(write=False)
        _WANT[name] = dict(scene=ref["scene"], rays=ref["rays"], tab=ref["tab"], T=T, want=want)
    return _WANT[name]


def _case_want(orc, get_scene, name):
    """test_query_forms' chain, clump and Cornell cases with the records of their rays"""
    c = tq._case(orc, get_scene, name)
    if "_cross" not in c:
        w = nx.crossings(c["tab"], c["T"], c["rays"], c["keep"])
        w.setflags(write=False)
        c["_cross"] = w
    return c, c["_cross"]


def _table_want(orc, prims, rays, disabled=(), keep_prims=None):
    """the records of `rays` in a scene made for one test: (want, tab, T)"""
    T = nc.world_triangles(prims, disabled=disabled)
    tab = tm.hit_table(orc, prims, rays)
    keep = ~np.isin(tab["prim"], list(disabled))
    if keep_prims is not None:
        keep &= keep_prims(tab["prim"])
    return nx.crossings(tab, T, rays, keep), tab, T


def _got(t):
    return t.cpu().numpy()


def _same(got, want, what):
    got = _got(got) if not isinstance(got, np.ndarray) else got
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = (got != want).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} records differ, the first at ray {int(np.flatnonzero(bad)[0])}: {got[bad][0]} for {want[bad][0]}"


# ---- closed meshes the helpers are tested on -------------------------------------------------------------------------------------------------------------------------
CUBE_LO, CUBE_HI = np.array([-0.6, -0.45, -0.5]), np.array([0.55, 0.65, 0.4])


def _mesh(scenes, verts, faces):
    mb = scenes.MeshBuilder()
    n = len(verts)
    mb.add(verts, [(0, 0)] * n, [(0, 0, 1)] * n, [(1, 0, 0, 1)] * n, np.asarray(faces).reshape(-1))
    return mb.finish(scenes.constant_texture((200, 180, 160)))


def _wound_cube(scenes):
    """12 triangles, every one wound counter-clockwise seen from outside: face `axis`, `side` has the corners (lo, lo), (hi, lo), (hi, hi), (lo, hi) in the two axes
    that follow it cyclically -- that order turns about +axis -- reversed on the low side"""
    verts, faces = [], []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side, at in ((1, CUBE_HI), (-1, CUBE_LO)):
            corners = []
            for cu, cv in ((CUBE_LO[u], CUBE_LO[v]), (CUBE_HI[u], CUBE_LO[v]), (CUBE_HI[u], CUBE_HI[v]), (CUBE_LO[u], CUBE_HI[v])):
                p = np.zeros(3)
                p[axis], p[u], p[v] = at[axis], cu, cv
                corners.append(p)
            if side < 0:
                corners.reverse()
            b = len(verts)
            verts += corners
            faces += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    return _mesh(scenes, np.array(verts), faces)


def _solid(orc, scenes, name):
    """a closed mesh, 8192 probe points in [-1, 1]^3, their 3 x 8192 rays, the records and votes of the reference, the analytic answer and the true distance to the
    surface (np_closest.witness, float64): made once"""
    if name not in _SOLID:
        if name == "cube":
            prim = _wound_cube(scenes)
        elif name == "icosphere":
            v, f = scenes.icosphere(2)
            prim = _mesh(scenes, v * 0.8, f)
        else:
            mb = scenes.MeshBuilder()
            scenes.box(mb, CUBE_LO, CUBE_HI)
            prim = mb.finish(scenes.constant_texture((200, 180, 160)))
        sc = scenes.Scene(name, [prim], scenes.cornell().camera, scenes.cornell().lights)
        points = np.random.default_rng(11).uniform(-1.0, 1.0, (8192, 3)).astype(np.float32)
        rays = nx.inside_rays(points)
        want, tab, T = _table_want(orc, sc.primitives, rays)
        w = T["w"].astype(np.float64)
        normal = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
        centre = w.reshape(-1, 3).mean(axis=0)
        outward = ((w.mean(axis=1) - centre) * normal).sum(axis=1)
        if name == "box":   # scenes.box: an axis-aligned box, whatever the winding of its faces
            lo, hi = T["lo"].min(axis=0).astype(np.float64), T["hi"].max(axis=0).astype(np.float64)
            inside = ((points > lo) & (points < hi)).all(axis=1)
        else:               # convex and wound outward (asserted): inside iff behind every face's plane
            assert (outward > 0).all(), f"{name}: a face is not wound counter-clockwise seen from outside"
            inside = (((points[:, None, :].astype(np.float64) - w[None, :, 0]) * normal[None]).sum(axis=2) < 0).all(axis=1)
        dist = nc.witness(T, np.concatenate([points, np.zeros((points.shape[0], 1), np.float32)], axis=1))
        _SOLID[name] = tq._freeze(dict(scene=sc, points=points, rays=rays, want=want, tab=tab, T=T, inside=inside.astype(np.uint8), dist=dist, outward=outward,
                                       votes={rule: nx.vote(want, rule) for rule in ("parity", "winding")}))
    return _SOLID[name]


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_ctypes_descriptor_is_the_headers():
    """1: ArtRayCrossings as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 40 bytes"""
    _layout_is_the_headers("ArtRayCrossings", 40, ["rays_dev", "cross_dev", "hip_stream", "n", "cull_mask", "flags", "reserved"])


def test_a_crossings_cast_without_a_context_is_invalid_on_any_machine():
    """2: art_cast_crossings(NULL, ...) needs no device to say ART_E_INVALID"""
    from araytracingjourney_amd import _lib
    L = _lib.load()
    assert L.art_cast_crossings(None, None) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    d = _lib.ArtRayCrossings(n=0)
    assert L.art_cast_crossings(None, C.byref(d)) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"


@pytest.mark.parametrize("name", ["cornell", "sponza_like"])
def test_the_reference_is_tied_down(orc, get_scene, name):
    """3: random_rays(4096, 7) on Cornell and sponza_like(0.05): entries + exits is the number of the table's rows a ray; the float32 sign is the float64 witness's on
    every row outside the witness's band |det| <= 1e-6 |e1| |d x e2|, and at most 1 % of the rows lie inside it (a cap on what the witness may leave out, not a device
    tolerance).  Both directions occur, and on sponza_like some ray crosses more than ART_CAST_MAX_HITS surfaces"""
    ref = _scene_ref(orc, get_scene, name)
    tab, rays, want = ref["tab"], ref["rays"], ref["want"]
    rows = np.flatnonzero(tab["ray"] < N)
    assert np.array_equal(want[:N].sum(axis=1), tm.hits_per_ray(tab, N + 1)[:N])
    d32 = nx.det32(ref["T"], rays, tab["gid"][rows], tab["ray"][rows])
    d64, band = nx.det64(ref["T"], rays, tab["gid"][rows], tab["ray"][rows])
    sure = np.abs(d64) > band
    share = 1.0 - sure.mean()
    print(f"\n[crossings] {name}: {rows.size} rows, {int((~sure).sum())} inside the witness's band ({100 * share:.4f} %); entries {int(want[:N, 0].sum())}, exits {int(want[:N, 1].sum())}, "
          f"most crossings of a ray {int(want[:N].sum(axis=1).max())}")
    assert share <= 0.01
    assert np.array_equal(d32[sure] > 0, d64[sure] > 0) and not (d32 == 0).any()
    assert want[:N, 0].sum() > 100 and want[:N, 1].sum() > 100
    if name == "sponza_like":
        assert int((want[:N].sum(axis=1) > 8).sum()) >= 50


@pytest.mark.parametrize("name,rules", [("cube", ("parity", "winding")), ("icosphere", ("parity", "winding")), ("box", ("parity",))])
def test_the_vote_of_the_reference_is_the_analytic_answer(orc, scenes, name, rules):
    """4: a cube of 12 triangles wound outward, icosphere(2) scaled by 0.8 and scenes.box, 8192 uniform points of numpy.random.default_rng(11) in [-1, 1]^3: the majority
    of the reference's three rays is the analytic answer at every point farther than 1e-3 from the surface (the true distance: np_closest.witness) -- under both rules
    for the two meshes wound outward, under parity for scenes.box, whose faces are not wound consistently (asserted: some face of it is wound inward)"""
    s = _solid(orc, scenes, name)
    far = s["dist"] > 1e-3
    from araytracingjourney_amd.renderer import Renderer
    assert np.array_equal(nx.DIRECTIONS, Renderer.INSIDE_DIRECTIONS) and Renderer.INSIDE_DIRECTIONS.dtype == np.float32 and (Renderer.INSIDE_DIRECTIONS != 0).all()
    assert int(s["inside"].sum()) > 500 and int((1 - s["inside"]).sum()) > 500 and int(far.sum()) > 8000
    for rule in rules:
        miss = (s["votes"][rule] != s["inside"]) & far
        single = (nx.vote(np.repeat(s["want"].reshape(-1, 3, 2)[:, :1], 3, axis=1).reshape(-1, 2), rule) != s["inside"]) & far
        print(f"\n[crossings] {name}, {rule}: {int(miss.sum())} of {int(far.sum())} points away from the surface voted wrong; the first ray alone: {int(single.sum())}")
        assert not miss.any(), (name, rule, int(miss.sum()))
    if name == "box":
        assert (s["outward"] < 0).any() and (s["outward"] > 0).any(), "scenes.box is wound consistently now: test the winding rule on it too"


# ---- on the device -----------------------------------------------------------------------------------------------------------------------------------------------------
def _one_triangle(scenes, indices=(0, 1, 2), model=None):
    mb = scenes.MeshBuilder()
    mb.add([(-0.5, -0.5, 0.25), (0.5, -0.5, 0.25), (0.0, 0.6, 0.25)], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, list(indices))
    prim = mb.finish(scenes.constant_texture((200, 180, 160)), model)
    return scenes.Scene("one triangle", [prim], scenes.cornell().camera, scenes.cornell().lights)


@pytest.mark.gpu
def test_single_triangles(R, torch, orc, scenes):
    """one triangle whose winding normal is +z: a ray along -z goes against it, (1, 0); the reversed ray is (0, 1); with the indices (0, 2, 1) the answers swap; under
    a model matrix that mirrors x (determinant -1) they swap again; a ray whose tmax ends short of the triangle, or whose tmin starts behind it, is (0, 0); a ray
    past the triangle and a dead ray are (0, 0).  The reference agrees with every line"""
    rays = np.zeros((6, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 7] = (0.05, -0.1, 1.0), 0.0, np.inf
    rays[:, 6] = -1.0
    rays[1, 2], rays[1, 6] = -1.0, 1.0                 # the reversed ray
    rays[2, 7] = 0.7                                    # ends short (the triangle is at t = 0.75)
    rays[3, 3] = 0.8                                    # starts behind it
    rays[4, 0] = 3.0                                    # passes beside it
    rays[5, 4] = np.nan                                 # dead
    mirror = np.array([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    down, up, none = (1, 0), (0, 1), (0, 0)
    for what, sc, (a, b) in (("as wound", _one_triangle(scenes), (down, up)), ("indices (0, 2, 1)", _one_triangle(scenes, (0, 2, 1)), (up, down)),
                             ("mirrored", _one_triangle(scenes, model=mirror), (up, down)), ("mirrored, indices (0, 2, 1)", _one_triangle(scenes, (0, 2, 1), mirror), (down, up))):
        want = np.array([a, b, none, none, none, none], np.int32)
        assert np.array_equal(_table_want(orc, sc.primitives, rays)[0], want), what
        r = R.renderer_for_scene(sc, (64, 64))
        got = r.cast_crossings(_up(torch, rays))
        torch.cuda.synchronize()
        _same(got, want, what)
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "sponza_like"])
def test_the_records_are_the_references(R, torch, orc, get_scene, name):
    """Cornell (where at least 50 rays hold a tie on t_eff among their first records) and sponza_like at detail 0.05 (where at least 50 rays cross more than 8
    triangles -- both asserted on the CPU by test_cast_multi), 4096 rays each: every record is the reference's; a permutation of the rays gives the permuted records;
    entries + exits is cast_rays_multi's count wherever that is below 8; some ray's count exceeds 8 in the device's own output (sponza_like)"""
    ref = _scene_ref(orc, get_scene, name)
    rays, want = ref["rays"][:N], ref["want"][:N]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    d_rays, d_perm = _up(torch, rays), _up(torch, rays[perm])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, got_p = r.cast_crossings(d_rays), r.cast_crossings(d_perm)
        count = r.cast_rays_multi(d_rays, 8)[2]
    s.synchronize()
    assert got.shape == (N, 2) and got.dtype == torch.int32
    _same(got, want, name)
    _same(got_p, want[perm], f"{name}, permuted")
    total, count = _got(got).sum(axis=1), _got(count)
    assert np.array_equal(np.minimum(total, 8), count)
    if name == "sponza_like":
        assert int((total > 8).sum()) >= 50 and int(total.max()) > 8
    assert r.cast_counts() == dict(casts=3, rays=3 * N, host_waits=0)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(tq.FORMS))
@pytest.mark.parametrize("name", ["chain", "clump", "cornell"])
def test_every_tree_form_gives_the_references(R, torch, orc, get_scene, name, form):
    """test_query_forms' six forms of the tree on its chain of 64 nested slivers, its 1000 triangles round one point and Cornell: the records are the references'.  On the
    chain and the clump the depth is proved first on the device's own 4-wide records: the first descent of a probe ray holds more pending entries than the 8 a lane
    keeps in LDS, so the walk's stack spills (with the limit never moving, everything pushed is also popped and visited)"""
    c, want = _case_want(orc, get_scene, name)
    r = R.renderer_for_scene(c["scene"], (64, 64), **tq.FORMS[form])
    if name in tq.PROBES:
        floats = r.get_wide_nodes()[1]
        depth = max(pending_on_first_descent_wide(floats, x) for x in c["rays"][tq.PROBES[name][0]])
        print(f"\n[crossings] {name}, {form}: pending entries on the first descent of a ray: {depth}")
        assert depth > LDS_DEPTH, depth
        assert int((want.sum(axis=1) > 8).sum()) >= 100
    got = r.cast_crossings(_up(torch, c["rays"]))
    torch.cuda.synchronize()
    _same(got, want, f"{name}, {form}")
    r.close()


_PRESETS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", tq.KNOBS, ids=lambda k: "-".join(f"{a}-{b}" for a, b in k.items()))
def test_knobs_change_the_schedule_never_the_records(R, torch, orc, get_scene, knobs):
    """test_query_forms' eight tracer settings (trace_chunk 64 / 65536, trace_refill 1 / 64, trace_blocks 1 / 16384, trace_leaf_batch 1 / 64) on sponza_like at 0.05:
    the reference's records, and the presets' word for word"""
    ref = _scene_ref(orc, get_scene, "sponza_like")
    rays = ref["rays"][:N]

    def run(tuning):
        r = R.renderer_for_scene(ref["scene"], (64, 64), tuning=tuning)
        got = r.cast_crossings(_up(torch, rays))
        torch.cuda.synchronize()
        r.close()
        return _got(got)
    if "got" not in _PRESETS:
        _PRESETS["got"] = run(None)
    got = run(knobs)
    _same(got, ref["want"][:N], str(knobs))
    assert np.array_equal(got, _PRESETS["got"])


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [64, 0], ids=["chunk-64", "preset-chunk"])
def test_sizes_at_which_a_refill_can_go_wrong(R, torch, orc, get_scene, chunk):
    """ArtTuning.trace_chunk = 64 and the preset: no ray, one, a wave less one, a wave, a wave and one, chunks and a ray more or less, several workgroups -- prefixes of
    Cornell's 4097 rays -- and a batch that is all dead, each written into a tensor five records too long filled with a pattern: the tail keeps it.  n = 0 enqueues
    nothing"""
    ref = _scene_ref(orc, get_scene, "cornell")
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning={"trace_chunk": chunk} if chunk else None)
    batches = [(ref["rays"][:n], ref["want"][:n], f"n = {n}") for n in tq.SIZES]
    batches.append((_dead_rays(ref["rays"][:130]), np.zeros((130, 2), np.int32), "all dead"))
    s = torch.cuda.Stream()
    pad, casts, n_rays = 5, 0, 0
    for rays, want, what in batches:
        n = rays.shape[0]
        d_rays = _up(torch, rays.reshape(n, 8))
        out = torch.full((n + pad, 2), PATTERN, dtype=torch.int32, device="cuda")
        before = r.cast_counts()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = r.cast_crossings(d_rays, out=out)
        s.synchronize()
        assert got is out
        if n == 0:
            assert r.cast_counts() == before, "n = 0 enqueued something"
        casts, n_rays = casts + (n > 0), n_rays + n
        _same(out[:n], want, what)
        assert (out[n:] == PATTERN).all(), f"{what}: written behind the n-th record"
    cc = r.cast_counts()
    assert cc["casts"] == casts and cc["rays"] == n_rays
    r.close()


def _soup(shape):
    """degenerate_soup(256, shape) and 512 rays from the sphere round it, each aimed at a triangle's centroid (the soup's triangles are small: random rays miss nearly
    all of them); a quarter of the triangles are copies of their neighbours, so many rays cross two coincident ones"""
    sc, rays = degenerate_soup(256, shape), random_rays(512, 11, radius=1.2)
    c = nc.world_triangles(sc.primitives)["w"].astype(np.float64).mean(axis=1)
    aim = c[(np.arange(512) * 7) % c.shape[0]] + np.random.default_rng(5).uniform(-0.005, 0.005, (512, 3)) - rays[:, 0:3]
    rays[:, 4:7] = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    return sc, rays


HOSTILE = ["lattice", "soup:soup", "soup:flat", "soup:line", "soup:clusters", "soup:one point", "ranges", "dead"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_inputs(R, torch, orc, get_scene, which):
    """lattice: axis-parallel rays (+0.0 and -0.0 in the other components) from lattice points through quads that share edges, vertices and planes -- rays that run
    along shared edges count every triangle that accepts them, as the float32 reference does (some ray's count is at least 4); soups of 256 triangles with copies,
    flat, in a line, in clusters and round one point; ranges: every kind of [tmin, tmax] a caller may hand over -- inf, -inf, inverted, negative, empty, NaN, denormal --
    on Cornell; dead: non-finite directions and origins and NaN tmax are (0, 0)"""
    if which == "lattice":
        sc, rays = lattice_scene(6), lattice_rays(6)
    elif which.startswith("soup:"):
        sc, rays = _soup(which[5:])
    elif which == "ranges":
        sc, rays = get_scene("cornell"), with_ranges(random_rays(256, 7))
    else:
        sc, rays = get_scene("cornell"), _dead_rays(random_rays(195, 7))
    want = _table_want(orc, sc.primitives, rays)[0]
    if which == "lattice":
        assert int((want.sum(axis=1) >= 4).sum()) >= 20 and int((want.sum(axis=1) % 2 == 1).sum()) >= 20
    elif which == "ranges":
        per = want.sum(axis=1).reshape(-1, len(RANGES))
        assert RANGES[3] == (2.0, 1.0) and np.isnan(RANGES[8][0]) and RANGES[1][1] == np.inf and RANGES[5] == (-3.0, -0.5) and RANGES[7] == (-np.inf, np.inf)
        assert (per[:, 3] == 0).all() and (per[:, 8] == 0).all() and per[:, 1].any() and per[:, 5].any() and per[:, 7].any()   # inverted and NaN ranges see nothing; tmax inf, negative and infinite ranges see something
    elif which == "dead":
        assert not want.any()
    else:
        assert int((want.sum(axis=1) > 0).sum()) >= 200 and int((want.sum(axis=1) >= 2).sum()) >= 50
    r = R.renderer_for_scene(sc, (64, 64))
    got = r.cast_crossings(_up(torch, rays))
    torch.cuda.synchronize()
    _same(got, want, which)
    r.close()


@pytest.mark.gpu
def test_masks_and_alpha(R, torch, orc, get_scene, scenes):
    """test_cast_multi.test_masks_and_alpha's set-up: Cornell and two horizontal cards, one with alpha 0 in every texel and one with alpha 255, a cutoff of 0.5 on both:
    the first is never counted, the second always -- EVERY candidate is alpha-tested, not only a nearest one.  Primitive masks and cull masks filter the table's rows by
    primitive; cull_mask = 0 counts nothing"""
    base = get_scene("cornell")
    prims = list(base.primitives)
    for y, a in ((0.3, 0), (-0.2, 255)):
        mb = scenes.MeshBuilder()
        scenes.quad(mb, (-0.35, y, -0.35), (0.7, 0.0, 0.0), (0.0, 0.0, 0.7), 2, 2, (1.0, 1.0))
        prims.append(mb.finish(_tex(a)))
    sc = scenes.Scene(base.name + "+cards", prims, base.camera, base.lights)
    clear, solid = len(prims) - 2, len(prims) - 1
    rays = random_rays(2048, 5, radius=0.9)
    T, tab = nc.world_triangles(sc.primitives), tm.hit_table(orc, sc.primitives, rays)
    assert int((tab["prim"] == clear).sum()) > 50 and int((tab["prim"] == solid).sum()) > 50
    # rays that cross the clear card BEHIND something else: a walk that tested only a nearest candidate would count it
    first = tm.expected(tab, rays, 1)[1][:, 0, 0]
    assert int(np.isin(np.flatnonzero(first != clear), tab["ray"][tab["prim"] == clear]).sum()) > 20
    masks = {0: 0x01, 1: 0x02, solid: 0x03}
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    d_rays = _up(torch, rays)
    got = r.cast_crossings(d_rays)
    torch.cuda.synchronize()
    _same(got, nx.crossings(tab, T, rays), "opaque")
    m.set_alpha_cutoff(clear, 0.5); m.set_alpha_cutoff(solid, 0.5)
    for i, v in masks.items():
        m.set_mask(i, v)
    vis = np.array([masks.get(p, 0xFF) for p in range(len(prims))])
    for cull in (0xFF, 0x01, 0x02, 0):
        keep = ((vis[tab["prim"]] & cull) != 0) & (tab["prim"] != clear)
        got = r.cast_crossings(d_rays, cull_mask=cull)
        torch.cuda.synchronize()
        _same(got, nx.crossings(tab, T, rays, keep), f"cull {cull:#x}")
        if cull == 0:
            assert not got.any()
    r.close()


@pytest.mark.gpu
def test_scene_changes(R, torch, orc, get_scene):
    """Cornell with its last primitive as a model of its own on a scene that never rebuilds: after a matrix move, after art_scene_set_vertices, after the primitive is
    disabled by residency (it is nowhere: never counted) and after it is enabled again, one cast each on a side stream with no synchronisation in between -- each is the
    reference of the scene as of its call"""
    sc = get_scene("cornell")
    rays = random_rays(1024, 7)
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
    m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
    verts = np.array(moving.verts, np.float32)
    verts[:, 0:3] = verts[:, 0:3] * np.float32(0.75) + np.array([0.0, 0.05, 0.0], np.float32)
    moved, deformed = static + [P(moving.verts, moving.indices, moving.tex, m)], static + [P(verts, moving.indices, moving.tex, m)]
    states = [("built", list(sc.primitives), ()), ("moved", moved, ()), ("deformed", deformed, ()), ("disabled", deformed, (len(static),)), ("enabled", deformed, ())]
    wants = [_table_want(orc, prims, rays, disabled=off)[0] for _, prims, off in states]
    assert all(not np.array_equal(a, b) for a, b in zip(wants[:-1], wants[1:]))
    r = R.Renderer((64, 64), dynamic_scene=True, tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(static)
    r.add_model([moving])
    r.prepare_first_frame()
    model = r.models_mut()[1]
    pid = model.primitive_ids[0]
    d_rays = _up(torch, rays)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for what, _, _ in states:
        if what == "moved": model.set_model_matrix(m)
        elif what == "deformed": model.set_vertices(0, verts)
        elif what == "disabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 0) == 0
        elif what == "enabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 1) == 0
        assert not r.needs_build()
        with torch.cuda.stream(s):
            outs.append(r.cast_crossings(d_rays))
    s.synchronize()
    for (what, _, _), got, want in zip(states, outs, wants):
        _same(got, want, what)
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 3, st
    r.close()


@pytest.mark.gpu
def test_the_ring_on_three_streams(R, torch, orc, get_scene):
    """40 casts -- crossings twice, then cast_rays -- over three torch streams with nothing synchronised before the end: more than the ART_CAST_POOL cursor blocks of the
    ring.  Every record is its reference; art_cast_counts counts all 40 in casts and rays"""
    from araytracingjourney_amd import _lib
    assert 40 > _lib.ART_CAST_POOL
    ref = _scene_ref(orc, get_scene, "cornell")
    rays, want = ref["rays"][:N], ref["want"][:N]
    closest = tm.expected(ref["tab"], rays, 1, ref["tab"]["ray"] < N)
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_rays = _up(torch, rays)
    streams = [torch.cuda.Stream() for _ in range(3)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(40):
        with torch.cuda.stream(streams[i % 3]):
            outs.append(r.cast_rays(d_rays) if i % 3 == 2 else r.cast_crossings(d_rays))
    counts = r.cast_counts()
    for s in streams:
        s.synchronize()
    for i, got in enumerate(outs):
        if i % 3 == 2:
            assert np.array_equal(_got(got[1]), closest[1][:, 0]) and np.array_equal(_got(got[0]).view(np.uint32)[:, :3], np.ascontiguousarray(closest[0][:, 0, :3]).view(np.uint32)), f"cast {i}"
        else:
            _same(got, want, f"cast {i}")
    assert counts["casts"] == 40 and counts["rays"] == 40 * N and counts["host_waits"] <= 40 - _lib.ART_CAST_POOL, counts
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("context", ["shard-1-of-4", "two-frames-per-launch", "eight-frames-in-flight"])
def test_other_contexts_answer_alike(R, torch, orc, get_scene, context):
    """a context that traces the second of four shards, one that traces two frames per launch, and -- on the context's own cast stream (hip_stream NULL, art_cast_sync
    as the fence) -- one with the 8 frames of a ring of 8 in flight: Cornell's records every time"""
    from araytracingjourney_amd import _lib
    ref = _scene_ref(orc, get_scene, "cornell")
    rays, want = ref["rays"][:N], ref["want"][:N]
    kw = {"shard-1-of-4": dict(shard=(1, 4)), "two-frames-per-launch": dict(frames_in_flight=2), "eight-frames-in-flight": dict(frames_in_flight=8)}[context]
    r = R.renderer_for_scene(ref["scene"], (64, 64), **kw)
    if context == "two-frames-per-launch":
        r.set_frames_per_launch(2)
    d_rays = _up(torch, rays)
    torch.cuda.synchronize()
    if context == "eight-frames-in-flight":
        out = torch.empty((N, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for f in range(8):
            r.upload_state(); r.trace()
            if f == 3:
                d = _lib.ArtRayCrossings(rays_dev=d_rays.data_ptr(), cross_dev=out.data_ptr(), hip_stream=None, n=N, cull_mask=0xFF, flags=0, reserved=0)
                assert r._L.art_cast_crossings(r._ctx, C.byref(d)) == 0
        assert r.frames_traced() == 8
        r.cast_sync(); r.sync()
        got = out
    else:
        r.upload_state(); r.trace()
        got = r.cast_crossings(d_rays)
        r.upload_state(); r.trace()
        r.sync(); torch.cuda.synchronize()
    _same(got, want, context)
    r.close()


@pytest.mark.gpu
def test_errors_change_nothing_and_enqueue_nothing(R, torch, get_scene):
    """every ART_E_INVALID case of include/art.h, and ART_E_STATE before the build and while the scene needs one: the output keeps its pattern, art_cast_counts stays what
    it was, and the message is the literal text"""
    from araytracingjourney_amd import _lib
    sc = get_scene("cornell")
    r = R.Renderer((64, 64))
    r.add_model(sc.primitives)
    L, ctx = r._L, r._ctx
    n = 64
    rays = _up(torch, random_rays(n + 1, 7))
    out = torch.full((n + 1, 2), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def desc(**kw):
        d = dict(rays_dev=rays.data_ptr(), cross_dev=out.data_ptr(), hip_stream=None, n=n, cull_mask=0xFF, flags=0, reserved=0)
        d.update(kw)
        return _lib.ArtRayCrossings(**d)

    def code(d):
        return L.art_cast_crossings(ctx, C.byref(d) if d is not None else None)

    state = WHO + b"scene not built, or changed since the build (art_scene_build)"
    assert code(desc()) == _lib.ART_E_STATE and L.art_last_error() == state
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert r.cast_counts() == zero
    assert L.art_cast_crossings(None, C.byref(desc())) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    assert code(None) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    bad = [(desc(rays_dev=None), b"rays_dev: null or not 16-byte aligned"), (desc(rays_dev=rays.data_ptr() + 4), b"rays_dev: null or not 16-byte aligned"),
           (desc(rays_dev=rays.data_ptr() + 8), b"rays_dev: null or not 16-byte aligned"), (desc(cross_dev=None), b"cross_dev: null or not 8-byte aligned"),
           (desc(cross_dev=out.data_ptr() + 4), b"cross_dev: null or not 8-byte aligned"), (desc(cull_mask=0x100), b"cull_mask: above 0xFF"),
           (desc(cull_mask=0xFFFFFFFF), b"cull_mask: above 0xFF"), (desc(flags=1), b"flags: must be 0"), (desc(flags=0x80000000), b"flags: must be 0"),
           (desc(reserved=1), b"reserved: must be 0"), (desc(reserved=0xFFFFFFFF), b"reserved: must be 0"), (desc(n=_lib.ART_CAST_MAX_RAYS + 1), b"n: above ART_CAST_MAX_RAYS"),
           (desc(n=0xFFFFFFFF), b"n: above ART_CAST_MAX_RAYS")]
    for d, text in bad:
        assert code(d) == _lib.ART_E_INVALID and L.art_last_error() == WHO + text, (text, L.art_last_error())
    assert r.cast_counts() == zero
    r.cast_sync()
    assert (out == PATTERN).all()
    assert code(desc(n=0)) == 0 and code(desc(n=0, rays_dev=None, cross_dev=None)) == 0 and r.cast_counts() == zero   # n = 0 is legal and enqueues nothing
    assert code(desc()) == 0
    r.cast_sync()
    assert r.cast_counts() == dict(casts=1, rays=n, host_waits=0) and (out[:n] != PATTERN).all() and (out[n:] == PATTERN).all()
    r.add_model([sc.primitives[0]])   # a primitive added since the build: art_scene_needs_build
    assert r.needs_build() and code(desc()) == _lib.ART_E_STATE and L.art_last_error() == state and r.cast_counts()["casts"] == 1
    # the wrappers' own checks come before anything is enqueued
    pts = rays[:, 0:3].contiguous()
    for fn, args, kw in ((r.cast_crossings, (rays.cpu(),), {}), (r.cast_crossings, (rays.double(),), {}), (r.cast_crossings, (rays[:, :7],), {}),
                         (r.cast_crossings, (rays,), dict(cull_mask=0x100)), (r.cast_crossings, (rays,), dict(out=out[:8])), (r.cast_crossings, (rays,), dict(out=out.to(torch.int64))),
                         (r.points_inside, (pts,), dict(rule="odd")), (r.points_inside, (pts.cpu(),), {}), (r.points_inside, (rays,), {}), (r.points_inside, (pts,), dict(cull_mask=-1)),
                         (r.signed_distance, (pts,), dict(rule="odd")), (r.signed_distance, (pts.double(),), {}),
                         (r.voxelize_solid, ((0, 0, 0), 0.1, (2, 2, 2)), dict(rule="odd")), (r.voxelize_solid, ((0, 0, 0), -0.1, (2, 2, 2)), {})):
        with pytest.raises(ValueError):
            fn(*args, **kw)
    assert r.cast_counts()["casts"] == 1
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_points_inside_and_signed_distance(R, torch, orc, scenes, name):
    """the wound cube and the icosphere, 8192 points: points_inside under both rules is the numpy vote at every point, and the analytic answer away from the surface;
    the one cast behind it holds the reference's 3 x 8192 records; signed_distance is closest_points' d (r = inf) with the sign of the numpy vote, bit for bit"""
    s = _solid(orc, scenes, name)
    r = R.renderer_for_scene(s["scene"], (64, 64))
    d_points = _up(torch, s["points"])
    n = s["points"].shape[0]
    cross = r.cast_crossings(_up(torch, s["rays"]))
    got = {rule: r.points_inside(d_points, rule) for rule in ("parity", "winding")}
    sd, ids, point = r.signed_distance(d_points)
    q = torch.full((n, 4), float("inf"), dtype=torch.float32, device="cuda")
    q[:, 0:3] = d_points
    duv, ids2, point2 = r.closest_points(q)
    torch.cuda.synchronize()
    _same(cross, s["want"], f"{name}: the rays of points_inside")
    far = s["dist"] > 1e-3
    for rule, g in got.items():
        g = _got(g)
        assert g.dtype == np.uint8 and g.shape == (n,)
        assert np.array_equal(g, s["votes"][rule]), f"{name}, {rule}: {int((g != s['votes'][rule]).sum())} points differ from the numpy vote"
        assert np.array_equal(g[far], s["inside"][far]), f"{name}, {rule}"
    d = _got(duv)[:, 0]
    want_sd = np.where(s["votes"]["parity"] != 0, -d, d).astype(np.float32)
    assert np.array_equal(_got(sd).view(np.uint32), want_sd.view(np.uint32)) and (_got(sd) < 0).sum() == s["votes"]["parity"].sum() > 500
    assert np.array_equal(_got(ids), _got(ids2)) and np.array_equal(_got(point).view(np.uint32), _got(point2).view(np.uint32))
    assert r.cast_counts()["casts"] == 4   # the rays, two points_inside, signed_distance's: one cast each; the point queries count as none
    r.close()


@pytest.mark.gpu
def test_voxelize_solid_fills_the_interior(R, torch, orc, scenes):
    """the icosphere in a 16^3 grid over [-1, 1]^3: voxelize_solid is voxelize OR the numpy vote of the cells' centres (made as origin + (idx + 0.5) * cell in float32),
    and it holds cells that voxelize leaves empty -- the interior"""
    s = _solid(orc, scenes, "icosphere")
    org, cell, dims = np.float32(-1.0), np.float32(0.125), (16, 16, 16)
    axis = (np.arange(16, dtype=np.float32) + np.float32(0.5)) * cell + org
    centres = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    want = _table_want(orc, s["scene"].primitives, nx.inside_rays(centres))[0]
    r = R.renderer_for_scene(s["scene"], (64, 64))
    surface = r.voxelize((-1.0, -1.0, -1.0), 0.125, dims)
    got = {rule: r.voxelize_solid((-1.0, -1.0, -1.0), 0.125, dims, rule=rule) for rule in ("parity", "winding")}
    torch.cuda.synchronize()
    surface, got = _got(surface), {rule: _got(g) for rule, g in got.items()}
    for rule, g in got.items():
        assert g.dtype == np.uint8 and g.shape == dims
        assert np.array_equal(g, surface | nx.vote(want, rule).reshape(dims)), rule
        assert int(((g == 1) & (surface == 0)).sum()) >= 100, "no interior cell"
    assert surface[0, 0, 0] == 0 and got["parity"][0, 0, 0] == 0 and got["parity"][8, 8, 8] == 1 and surface[8, 8, 8] == 0
    r.close()
