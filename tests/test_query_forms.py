"""art_cast_rays_multi, art_closest_points, art_cast_spheres and art_resolve_hits (DESIGN.md 3.6 .. 3.9) over every form of the tree, every tracer knob, the sizes at which
a chunk or a wave ends, trees a refit wrote, the shared ring of cast blocks with kinds mixed, and the other kinds of context.  Their own modules run one configuration
each -- the default device SAH tree, the cast preset, batches of 4096 or 1024 -- and the modules that vary configuration (tests/test_walk_edges.py, tests/test_cast.py)
were written before these kernels existed.

Nothing here has a tolerance.  The references are the existing modules': test_cast_multi.hit_table / expected (the oracle, one triangle at a time), np_closest.brute_force
and np_sweep.brute_force (numpy float32, operation by operation), each computed once, shared and read-only; every comparison is ids and bits.  The records are defined as
independent of the structure that finds them, and that is the property checked.  A resolve is compared word for word with the resolve of the same records on a renderer
of the default form.

"The three kinds" on one renderer: cast_rays_multi at K = 1, 4 and 8 (K = 1 also equals cast_rays bit for bit), closest_points with the point output, cast_spheres at a
radius of 0.05 and of 0.

Depth proofs (test_every_tree_form_gives_the_references): before anything is compared on the chain and on the clump, a numpy walk of the DEVICE'S OWN 4-wide records
shows that the first descent of a probe holds more pending entries than the 8 a lane keeps in LDS (kCastLds, kClosestLds), so the spill paths -- TravMulti's and
TravSweep's, and TravPoint's, where a spilled entry loses its distance and is visited unasked -- are reached.  Measured on the device (rays / rays inflated by 0.05 /
points; the deepest of the probes):
                           chain            clump
    default                37 / 37 / 37     18 / 19 / 21
    fast-build             36 / 36 / 36     21 / 21 / 21
    host-sah               31 / 31 / 31     18 / 18 / 18
    host-wide              37 / 37 / 37     18 / 19 / 21
    morton-30              37 / 37 / 37     18 / 19 / 21
    fast-build-host-wide   36 / 36 / 36     21 / 21 / 21
(The chain is a comb on every form: a ray through every box and a point with an infinite radius leave the same siblings behind on the way down.)

Mutation checks, on scratch builds: with TravPoint::pop skipping spilled entries, and with TravPoint::step_leaf's tie rule flipped to gid > bgid, every GPU test of this
module fails at its nearest-point comparison (every test runs the three kinds) -- on the chain, the clump and Cornell on every form, 2492 and 949 of sponza_like's 4096
queries under every knob, 5 and 29 of the 63 queries of the sizes' n = 63.
"""
import ctypes as C

import numpy as np
import pytest

import np_closest as nc
import np_sweep as ns
import test_cast_multi as tm
import test_closest_points as tcp
import test_sphere_cast as tsc
import test_walk_edges as twe
from helpers import chain_scene, degenerate_soup, dequantise, pending_on_first_descent_point, pending_on_first_descent_wide, random_rays
from helpers import _host, R, torch, _up  # noqa: F401  (R, torch: module fixtures)

PATTERN = -0x5A5A5A5B   # tests/test_cast.py's: what oversized output buffers are filled with
RHO = 0.05
RADII = (RHO, 0.0)
KS = (1, 4, 8)
LDS_DEPTH = 8           # kCastLds of art_query_rays.hip and kClosestLds of art_query_points.hip: stack entries a lane keeps in LDS; deeper ones spill
OUTPUTS = ("pos", "ng", "ns", "uv", "albedo", "orm")
SIZES = (0, 1, 63, 64, 65, 127, 511, 513, 4097)


# ---- scenes, inputs and references: made once, shared, never written ------------------------------------------------------------------------------------------------
_CASE, _SPONZA, _DEFAULT_RESOLVE = {}, {}, {}


def _inputs(get_scene, name):
    """(scene, rays, point queries) of a case"""
    if name == "chain":
        # the chain's own rays and tests/test_closest_points.py's queries; 32 rays that START within 0.05 of a sliver (feature S of a sphere cast: the chain's own rays
        # start a unit away) and 72 points just outside the slivers' long edges and base vertices (the chain's own queries lie on the axis: nearly all of them are nearest to a face)
        sc, rays = chain_scene(64)
        q = tcp._hostile("chain")[1]
        k = np.arange(16, dtype=np.float64)
        extra = np.zeros((32, 8), np.float32)
        extra[:, 3], extra[:, 7], extra[:, 4] = 0.001, 100.0, 1.0
        extra[:, 0], extra[:, 2] = np.tile(2.0 ** -k, 2), 0.03
        extra[16:, 1], extra[16:, 6] = 0.02, -0.02
        c = 2.0 ** -np.arange(24, dtype=np.float64)
        side = np.concatenate([np.stack([1.25 * c, np.full(24, sgn * 0.006), np.full(24, 0.006)], 1) for sgn in (1.0, -1.0)])   # 0.001 outside the middle of a long edge
        side = np.concatenate([side] + [np.stack([c[:12], np.full(12, sgn * 0.015), np.full(12, 0.005)], 1) for sgn in (1.0, -1.0)])           # beside a base vertex: the end of edge v0v1
        return sc, np.concatenate([rays, extra]), np.concatenate([q, tcp.queries(side)])
    if name == "clump":
        # 1000 triangles round one point; rays aimed at it as tests/test_walk_edges.py::_base("one-point") aims them (random rays: 12 sweep hits of 512); queries from the
        # rays' origins, from every 23rd vertex (d = 0) and from a cube a little larger than the clump, where the far edges v1v2 are the nearest features
        sc = degenerate_soup(1000, "one point")
        rays = random_rays(512, 1000)
        centre = np.array([0.1, 0.05, 0.3])
        aim = centre + np.random.default_rng(5).uniform(-0.03, 0.03, (512, 3)) - rays[:, 0:3]
        rays[:, 4:7] = aim / np.linalg.norm(aim, axis=1, keepdims=True)
        verts = nc.world_triangles(sc.primitives)["w"].reshape(-1, 3)[::23]
        near = centre + np.random.default_rng(7).uniform(-0.09, 0.09, (128, 3))
        return sc, rays, tcp.queries(np.concatenate([rays[:256, 0:3], verts, near]))
    if name == "cornell":
        rays = random_rays(4097, 7)   # (ray k does not depend on how many there are: a prefix of these is random_rays(n, 7))
        return get_scene("cornell"), rays, tcp.queries(rays[:, 0:3])
    raise KeyError(name)


def _freeze(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, (tuple, dict)):
            _freeze(a)
    return x


def _refs(orc, prims, rays, q, disabled=()):
    """the three kinds' references for one state of a scene: the multi-hit table, the nearest points, the sphere casts at both radii -- with the references' statistics"""
    T = nc.world_triangles(prims, disabled=disabled)
    tab = tm.hit_table(orc, prims, rays)
    closest = nc.brute_force(T, q, stats=True)
    sweep = {rho: ns.brute_force(T, rays, rho, stats=True) for rho in RADII}
    return _freeze(dict(T=T, rays=rays, q=q, tab=tab, keep=~np.isin(tab["prim"], list(disabled)), closest=closest[:3], cstats=closest[3],
                        sweep={rho: s[:3] for rho, s in sweep.items()}, sstats={rho: s[3] for rho, s in sweep.items()}))


def _case(orc, get_scene, name):
    if name not in _CASE:
        sc, rays, q = _inputs(get_scene, name)
        _CASE[name] = dict(_refs(orc, sc.primitives, rays, q), scene=sc, name=name)
    return _CASE[name]


def _sponza(orc, get_scene):
    """sponza_like at detail 0.05 with the 4096-input references of the kinds' own modules (their caches: nothing is computed twice in one session); the sphere casts at
    radius 0 are this module's, over the first 1024 rays (3.7 s; 4096 would take four times that)"""
    if not _SPONZA:
        m, p, s = tm._ref(orc, get_scene, "sponza_like", 0.05), tcp._ref(get_scene, "sponza_like", 0.05), tsc._ref(get_scene, "sponza_like", 0.05)
        n = tm.N
        assert np.array_equal(m["rays"][:n], s["rays"]) and np.array_equal(p["q"][:, 0:3], s["rays"][:, 0:3])
        zero = ns.brute_force(s["T"], s["rays"][:1024], 0.0, stats=True)
        _SPONZA.update(_freeze(dict(T=s["T"], rays=m["rays"][:n], q=p["q"], tab=m["tab"], keep=m["tab"]["ray"] < n, closest=p["want"], cstats=p["stats"],
                                    sweep={RHO: s["want"], 0.0: zero[:3]}, sstats={RHO: s["stats"], 0.0: zero[3]})), scene=m["scene"], name="sponza_like", sweep_n={RHO: n, 0.0: 1024})
    return _SPONZA


def _want_multi(c, K, n=None):
    """the table's first K records of the first n rays (cached: expected() sorts the whole table)"""
    n = c["rays"].shape[0] if n is None else n
    memo = c.setdefault("_multi", {})
    if (K, n) not in memo:
        memo[(K, n)] = _freeze(tm.expected(c["tab"], c["rays"][:n], K, c["keep"] & (c["tab"]["ray"] < n)))
    return memo[(K, n)]


def _words(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


# ---- the three kinds on one renderer ------------------------------------------------------------------------------------------------------------------------------
def _enqueue_kinds(r, torch, c, n=None, d_in=None, null_stream=False):
    """the three kinds (and the plain closest cast K = 1 is compared with) enqueued on torch's current stream -- or, null_stream, on the context's own cast stream
    (hip_stream NULL: the descriptors by hand, the wrappers cannot say it) -- with no synchronisation: {kind: device tensors}"""
    from araytracingjourney_amd import _lib
    if d_in is None:
        d_in = (_up(torch, c["rays"][:n]), _up(torch, c["q"][:n]))   # (n None: every ray and every query, which need not be as many)
    d_rays, d_q = d_in
    n, nq = d_rays.shape[0], d_q.shape[0]
    sweep_n = c.get("sweep_n", {})
    d_short = {rho: d_rays[:min(n, sweep_n.get(rho, n))] for rho in RADII}
    if not null_stream:
        got = {("multi", K): r.cast_rays_multi(d_rays, K) for K in KS}
        got["cast"] = r.cast_rays(d_rays)
        got["closest"] = r.closest_points(d_q)
        for rho in RADII:
            got[("sweep", rho)] = r.cast_spheres(d_short[rho], rho)
        return got
    f4 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")   # noqa: E731
    i4 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")     # noqa: E731
    got, L, ctx = {}, r._L, r._ctx
    for K in KS:   # (the caller has synchronised behind the uploads, which ran on torch's stream; nothing here waits for anything)
        out = (f4(n, K, 4), i4(n, K, 2), torch.empty((n,), dtype=torch.uint8, device="cuda"))
        d = _lib.ArtRayCastMulti(rays_dev=d_rays.data_ptr(), tuv_dev=out[0].data_ptr(), ids_dev=out[1].data_ptr(), count_dev=out[2].data_ptr(), hip_stream=None, n=n, max_hits=K, cull_mask=0xFF, flags=0)
        assert L.art_cast_rays_multi(ctx, C.byref(d)) == 0
        got[("multi", K)] = out
    out = (f4(n, 4), i4(n, 2))
    d = _lib.ArtRayCast(rays_dev=d_rays.data_ptr(), tuv_dev=out[0].data_ptr(), ids_dev=out[1].data_ptr(), hit_dev=None, hip_stream=None, n=n, kind=_lib.ART_CAST_CLOSEST, cull_mask=0xFF, flags=0)
    assert L.art_cast_rays(ctx, C.byref(d)) == 0
    got["cast"] = out
    out = (f4(nq, 4), i4(nq, 2), f4(nq, 4))
    d = _lib.ArtPointQuery(points_dev=d_q.data_ptr(), duv_dev=out[0].data_ptr(), ids_dev=out[1].data_ptr(), point_dev=out[2].data_ptr(), hip_stream=None, n=nq, cull_mask=0xFF, flags=0, reserved=0)
    assert L.art_closest_points(ctx, C.byref(d)) == 0
    got["closest"] = out
    for rho in RADII:
        m = d_short[rho].shape[0]
        out = (f4(m, 4), i4(m, 2), f4(m, 4))
        d = _lib.ArtSphereCast(rays_dev=d_short[rho].data_ptr(), tuv_dev=out[0].data_ptr(), ids_dev=out[1].data_ptr(), point_dev=out[2].data_ptr(), hip_stream=None, n=m, cull_mask=0xFF, flags=0, radius=rho)
        assert L.art_cast_spheres(ctx, C.byref(d)) == 0
        got[("sweep", rho)] = out
    return got


def _check_kinds(got, c, what, n=None):
    """every record of _enqueue_kinds' outputs against the references' first n: ids and bits"""
    n, nq = (c["rays"].shape[0], c["q"].shape[0]) if n is None else (n, n)
    for K in KS:
        tm._same(got[("multi", K)], _want_multi(c, K, n), f"{what}: multi, K = {K}")
    one, cast = got[("multi", 1)], got["cast"]
    assert np.array_equal(_words(one[0])[:, 0], _words(cast[0])) and np.array_equal(one[1].cpu().numpy()[:, 0], cast[1].cpu().numpy()), f"{what}: K = 1 is not cast_rays"
    tcp._same(_host(got["closest"]), tuple(w[:nq] for w in c["closest"]), f"{what}: closest")
    for rho in RADII:
        m = min(n, c.get("sweep_n", {}).get(rho, n))
        tsc._same(_host(got[("sweep", rho)]), tuple(w[:m] for w in c["sweep"][rho]), f"{what}: sweep, radius {rho}")


def _records(c, n=None):
    """{kind: (tuv, ids)}: the references' records as a resolve takes them"""
    n, nq = (c["rays"].shape[0], c["q"].shape[0]) if n is None else (n, n)
    rec = {("multi", K): _want_multi(c, K, n)[:2] for K in KS}
    rec["closest"] = tuple(w[:nq] for w in c["closest"][:2])
    for rho in RADII:
        m = min(n, c.get("sweep_n", {}).get(rho, n))
        rec[("sweep", rho)] = tuple(w[:m] for w in c["sweep"][rho][:2])
    return rec


def _resolve_kinds(r, torch, got):
    """one resolve of every kind's records (the device's own tensors) behind them on torch's current stream: {kind: {output: tensor}}"""
    return {k: r.resolve_hits(v[0], v[1], OUTPUTS) for k, v in got.items() if k != "cast"}


def _default_resolve(R, torch, c):
    """the resolve of the references' records on a renderer of the default form, as words: made once per scene"""
    if c["name"] not in _DEFAULT_RESOLVE:
        r = R.renderer_for_scene(c["scene"], (64, 64))
        out = {k: r.resolve_hits(_up(torch, tuv), _up(torch, ids), OUTPUTS) for k, (tuv, ids) in _records(c).items()}
        torch.cuda.synchronize()
        _DEFAULT_RESOLVE[c["name"]] = _freeze({k: {o: _words(t) for o, t in v.items()} for k, v in out.items()})
        r.close()
    return _DEFAULT_RESOLVE[c["name"]]


def _check_resolves(res, want, what):
    for k, outs in res.items():
        for o, t in outs.items():
            assert np.array_equal(_words(t), want[k][o]), f"{what}: resolve of {k}: {o} differs from the default form's"


# ---- 7: without a GPU -- the conditions the comparisons lean on, counted in the references ---------------------------------------------------------------------------
# per scene: rays with a hit, rays with at least 8 accepted triangles, rays with a tie on t_eff among their first 8 records; queries answered, queries whose minimum is
# shared, queries won by the face and by the edges v0v1, v0v2, v1v2; sphere casts that hit at radius 0.05 and at 0, casts won by S, F, an edge and a vertex over both
# radii, casts with a tie.  Each floor is the reference's own count (in the comment) rounded down
FLOORS = {
    #            hit  >= 8  tied | answered  tied  face / e01 / e02 / e12   | hit 0.05  hit 0    S     F    E    V  tied
    "chain":   (100,  100,  100,   400,      200,  (300, 20, 20, 20),          200,     100,   30,  100, 100,  10, 300),
    "clump":   (500,  500,  400,   500,      200,  (100, 100, 200, 10),        500,     500,    5,  300, 100, 400, 300),
    "cornell": (3000,   0,  100,  4000,     1000,  (1000, 1000, 1000, 600),   3000,    3000,  200, 6000, 300,  10, 300),
}


@pytest.mark.parametrize("name", list(FLOORS))
def test_the_comparisons_are_not_vacuous(orc, get_scene, name):
    """7: from the references alone.  Multi: hit rays, rays with at least 8 accepted triangles (on the chain and the clump every hit ray: k_cast_multi<8> fills and
    evicts), ties on t_eff among the first 8 (the order is by gid).  Points: every query answered (r = inf), ties on the minimum, each of the four nearest features.
    Sphere casts: hits at both radii; S, F, an edge and a vertex each win somewhere (counted over both radii: at 0.05 the ball is as large as the clump's triangles and no
    face is touched first, at 0 nothing starts inside), ties.  Measured:
        chain:   101 / 101 / 101 | 407, 232, 329 / 25 / 27 / 26 | 234, 110 | S 32 F 198 E 102 V 12, tied 202 + 108
        clump:   512 / 512 / 473 | 515, 244, 141 / 152 / 209 / 13 | 512, 512 | S 5 F 368 E 154 V 497, tied 194 + 194
        cornell: 3365 / 0 / 101 | 4097, 1914, 1300 / 1008 / 1101 / 688 | 3609, 3365 | S 222 F 6343 E 395 V 14, tied 318 + 63"""
    c = _case(orc, get_scene, name)
    n = c["rays"].shape[0]
    per = tm.hits_per_ray(c["tab"], n)
    multi = (int((per > 0).sum()), int((per >= 8).sum()), tm.tied_rays(c["tab"], n, 8))
    cs = c["cstats"]
    points = (int((c["closest"][1][:, 0] >= 0).sum()), int((cs["ties"] >= 2).sum()), tuple(int((cs["feature"] == f).sum()) for f in range(4)))
    hits = tuple(int((c["sweep"][rho][1][:, 0] >= 0).sum()) for rho in RADII)
    feat = np.concatenate([c["sstats"][rho]["feature"] for rho in RADII])
    wins = (int((feat == 0).sum()), int((feat == 1).sum()), int(((feat >= 2) & (feat <= 4)).sum()), int((feat >= 5).sum()))
    tied = tuple(int((c["sstats"][rho]["ties"] >= 2).sum()) for rho in RADII)
    print(f"\n[forms] {name}: multi hit / >= 8 / tied {multi}; points answered, tied, features {points}; sweeps hit {hits}, S F E V {wins}, tied {tied}")
    f = FLOORS[name]
    assert multi[0] >= f[0] and multi[1] >= f[1] and multi[2] >= f[2], multi
    assert points[0] >= f[3] and points[1] >= f[4] and all(a >= b for a, b in zip(points[2], f[5])), points
    assert hits[0] >= f[6] and hits[1] >= f[7] and all(a >= b for a, b in zip(wins, f[8:12])) and sum(tied) >= f[12], (hits, wins, tied)
    if name != "cornell":
        assert multi[1] == multi[0], "every ray that hits fills a list of 8"


def test_the_sponza_prefixes_are_not_vacuous(orc, get_scene):
    """7: the knob tests lean on the kinds' own modules' conditions for the 4096-input references (asserted there); the ring test takes the first 1024 inputs and the
    radius-0 sphere casts are over the first 1024 rays.  Measured in those: 969 rays hit and 20 have more than 8 hits; 1024 queries answered, 228 with a tie; 987 sphere
    casts hit at 0.05 and 969 at 0"""
    c = _sponza(orc, get_scene)
    per = tm.hits_per_ray(c["tab"], tm.N + 1)[:1024]
    figures = (int((per > 0).sum()), int((per > 8).sum()), int((c["closest"][1][:1024, 0] >= 0).sum()), int((c["cstats"]["ties"][:1024] >= 2).sum()),
               int((c["sweep"][RHO][1][:1024, 0] >= 0).sum()), int((c["sweep"][0.0][1][:, 0] >= 0).sum()))
    print(f"\n[forms] sponza_like, first 1024: {figures}")
    assert figures[0] >= 900 and figures[1] >= 20 and figures[2] == 1024 and figures[3] >= 200 and figures[4] >= 900 and figures[5] >= 900, figures
    assert c["sweep"][0.0][0].shape[0] == 1024


# ---- 1: tree forms, with the depth proved first ----------------------------------------------------------------------------------------------------------------------
FORMS = {"default": {}, "fast-build": dict(fast_build=True), "host-sah": dict(tuning={"tree_builder": 1}), "host-wide": dict(tuning={"wide_builder": 1}),
         "morton-30": dict(morton_bits=30), "fast-build-host-wide": dict(fast_build=True, tuning={"wide_builder": 1})}
# the probes whose first descents are walked in numpy: (rays, rays for the inflated boxes, queries)
PROBES = {"chain": (slice(0, 40), slice(0, 8), slice(0, 48)), "clump": (slice(0, 48), slice(0, 48), slice(0, 48))}


def _depths(r, c, name):
    """the deepest first descent of the probes on the device's own 4-wide records: rays on the float boxes (test_deep_stacks_in_every_walk's walk), rays on those boxes
    inflated by 0.05, points on the quantised boxes the nearest-point walk reads"""
    quantised, floats = r.get_wide_nodes()
    p_rays, p_sweep, p_points = PROBES[name]
    rays = max(pending_on_first_descent_wide(floats, x) for x in c["rays"][p_rays])
    boxes = floats[:, :24].view(np.float32).reshape(-1, 4, 6).copy()
    boxes[..., :3] -= np.float32(RHO)
    boxes[..., 3:] += np.float32(RHO)
    inflated = floats.copy()
    inflated[:, :24] = boxes.reshape(-1, 24).view(np.uint32)
    sweep = max(pending_on_first_descent_wide(inflated, x) for x in c["rays"][p_sweep])
    lo, hi, valid, _ = dequantise(quantised)
    child = np.ascontiguousarray(quantised[:, 12:16]).view(np.int32)
    points = max(pending_on_first_descent_point(lo, hi, valid, child, x) for x in c["q"][p_points])
    return rays, sweep, points


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["chain", "clump", "cornell"])
def test_every_tree_form_gives_the_references(R, torch, orc, get_scene, name, form):
    """1: the chain of 64 nested slivers, 1000 triangles round one point and Cornell on the default device SAH tree, the canonical LBVH (ART_FLAG_FAST_BUILD), the host
    SAH, the host 4-wide collapse, 30 Morton bits, and the canonical tree collapsed on the host: the three kinds are the references', and a resolve of each kind's records
    is the default form's word for word.  On the chain and the clump the depth is proved first (the module's docstring has the figures): more than 8 pending entries on
    the first descent of a ray, of a ray against boxes inflated by 0.05 and of a point with r = inf"""
    c = _case(orc, get_scene, name)
    want_res = _default_resolve(R, torch, c)
    r = R.renderer_for_scene(c["scene"], (64, 64), **FORMS[form])
    if name in PROBES:
        d = _depths(r, c, name)
        print(f"\n[forms] {name}, {form}: pending entries on the first descent: rays {d[0]}, rays with boxes inflated by {RHO} {d[1]}, points {d[2]}")
        assert min(d) > LDS_DEPTH, d
    s = torch.cuda.Stream()
    d_in = (_up(torch, c["rays"]), _up(torch, c["q"]))
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = _enqueue_kinds(r, torch, c, d_in=d_in)
        res = _resolve_kinds(r, torch, got)
    s.synchronize()
    _check_kinds(got, c, f"{name}, {form}")
    _check_resolves(res, want_res, f"{name}, {form}")
    r.close()


# ---- 2: knobs ----------------------------------------------------------------------------------------------------------------------------------------------------------
KNOBS = [k for k in twe.KNOBS if "ao_entry_off" not in k]
_PRESETS = {}


def _knob_outputs(R, torch, c, tuning):
    r = R.renderer_for_scene(c["scene"], (64, 64), tuning=tuning)
    got = _enqueue_kinds(r, torch, c)
    torch.cuda.synchronize()
    r.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a}-{b}" for a, b in k.items()))
def test_knobs_change_the_schedule_never_the_records(R, torch, orc, get_scene, knobs):
    """2: ArtTuning.trace_chunk 64 / 65536, trace_refill 1 / 64, trace_blocks 1 / 16384 and trace_leaf_batch 1 / 64 (test_walk_edges.KNOBS' eight tracer settings) on
    sponza_like at detail 0.05 with the shared 4096-input references: the three kinds give the references' bits, and the presets' bits word for word.

    Why trace_leaf_batch = 64 and trace_refill = 64 cannot hang k_closest's own loop (read against art_query_points.hip and art_walk.h): its step block is pooled_trace's.  Triangle tests run
    once leaf_batch lanes wait on one OR no active lane stands on an internal node, and a lane on an internal node always moves -- step_internal goes on with a child or
    pops -- so a wave whose waiting lanes can never number 64 still tests them as soon as nobody else can move: every iteration does a node step or a leaf step, and a
    walk has finitely many.  The refill block is entered when at least trace_refill lanes are idle; 64 idle lanes is always at least that, so a wave that has finished
    its queries either reads more (end - cur > 0 after a successful pop: a chunk is never empty), or is exhausted and leaves.  A filling of dead queries only (no lane
    active afterwards) loops back to the refill, which ends with the chunks"""
    assert len(KNOBS) == 8 and {a for k in KNOBS for a in k} == {"trace_chunk", "trace_refill", "trace_blocks", "trace_leaf_batch"}
    c = _sponza(orc, get_scene)
    if "got" not in _PRESETS:
        _PRESETS["got"] = {k: tuple(_words(t) for t in v) for k, v in _knob_outputs(R, torch, c, None).items()}
    got = _knob_outputs(R, torch, c, knobs)
    _check_kinds(got, c, str(knobs))
    for k, v in got.items():
        for t, w in zip(v, _PRESETS["got"][k]):
            assert np.array_equal(_words(t), w), f"{knobs}: {k} differs from the presets'"


# ---- 3: sizes ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _dead_queries(q):
    """non-finite coordinates, a NaN radius, a negative radius in turn"""
    d = np.array(q)
    d[0::4, 0], d[1::4, 2], d[2::4, 3], d[3::4, 3] = np.nan, np.inf, np.nan, -1.0
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [64, 0], ids=["chunk-64", "preset-chunk"])
def test_sizes_at_which_a_refill_can_go_wrong(R, torch, orc, get_scene, chunk):
    """3: ArtTuning.trace_chunk = 64 (a chunk is one filling of a wave) and the preset: closest_points and cast_spheres (radius 0.05 and 0) of no input, one, a wave less
    one, a wave, a wave and one, chunks and an input more or less, several workgroups -- prefixes of Cornell's 4097-input references -- of a batch that misses everything
    (queries with r = 0 away from any surface; outward rays) and of a batch that is all dead.  Every batch is written into tensors five records too long filled with a
    pattern: the tail keeps it.  n = 0 enqueues nothing"""
    c = _case(orc, get_scene, "cornell")
    r = R.renderer_for_scene(c["scene"], (64, 64), tuning={"trace_chunk": chunk} if chunk else None)
    batches = [(c["rays"][:n], c["q"][:n], tuple(w[:n] for w in c["closest"]), {rho: tuple(w[:n] for w in c["sweep"][rho]) for rho in RADII}, f"n = {n}") for n in SIZES]
    away = np.array(c["q"][:195])
    away[:, 3] = 0.0
    for rays, q, what in ((tm._outward_rays(c["rays"][:195]), away[:130], "all miss"), (tm._dead_rays(c["rays"][:130]), _dead_queries(c["q"][:130]), "all dead")):
        cw, sw = nc.brute_force(c["T"], q), {rho: ns.brute_force(c["T"], rays, rho) for rho in RADII}
        assert (cw[1] == -1).all() and all((w[1] == -1).all() for w in sw.values()), what
        batches.append((rays, q, cw, sw, what))
    s = torch.cuda.Stream()
    pad, casts, n_rays = 5, 0, 0
    for rays, q, cw, sw, what in batches:
        n = rays.shape[0]
        d_rays, d_q = _up(torch, rays.reshape(n, 8)), _up(torch, q.reshape(n, 4))
        outs = [tuple(torch.full((n + pad, w), PATTERN, dtype=torch.int32, device="cuda").view(dt) for w, dt in ((4, torch.float32), (2, torch.int32), (4, torch.float32))) for _ in range(3)]
        before = r.cast_counts()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = [r.closest_points(d_q, out=outs[0])] + [r.cast_spheres(d_rays, rho, out=o) for rho, o in zip(RADII, outs[1:])]
        s.synchronize()
        assert all(g[0] is o[0] for g, o in zip(got, outs))
        if n == 0:
            assert r.cast_counts() == before, "n = 0 enqueued something"
        casts, n_rays = casts + 2 * (n > 0), n_rays + 2 * n
        tcp._same(tuple(t[:n].cpu().numpy() for t in outs[0]), cw, f"{what}: closest")
        for rho, o in zip(RADII, outs[1:]):
            tsc._same(tuple(t[:n].cpu().numpy() for t in o), sw[rho], f"{what}: sweep, radius {rho}")
        for o in outs:
            for t in o:
                assert (t[n:].view(torch.int32) == PATTERN).all(), f"{what}: written behind the n-th record"
        if what in ("all miss", "all dead"):
            assert np.array_equal(_words(outs[0][0][:n])[:, 0], np.ascontiguousarray(q[:, 3]).view(np.uint32)), f"{what}: r as given"
            assert np.array_equal(_words(outs[1][0][:n])[:, 0], np.ascontiguousarray(rays[:, 7]).view(np.uint32)), f"{what}: tmax as given"
    cc = r.cast_counts()
    assert cc["casts"] == casts and cc["rays"] == n_rays   # point queries count as neither
    r.close()


# ---- 4: trees a refit wrote ----------------------------------------------------------------------------------------------------------------------------------------
REFITS = {"presets": {}, "fold-nodes": {"refit_fold_nodes": 1}, "one-version": {"as_versions": 1}, "no-refit-streams": {"refit_streams": 0xFFFFFFFF}}
_REFIT_REF = {}


def _refit_states(orc, get_scene):
    """Cornell with its last primitive moved, deformed, disabled and enabled again: (what, the references of that state over 1024 inputs)"""
    if not _REFIT_REF:
        sc = get_scene("cornell")
        rays = random_rays(1024, 7)
        q = tcp.queries(rays[:, 0:3])
        static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
        P = type(moving)
        m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
        m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
        verts = np.array(moving.verts, np.float32)
        verts[:, 0:3] = verts[:, 0:3] * np.float32(0.75) + np.array([0.0, 0.05, 0.0], np.float32)
        moved, deformed = static + [P(moving.verts, moving.indices, moving.tex, m)], static + [P(verts, moving.indices, moving.tex, m)]
        states = [("moved", moved, ()), ("deformed", deformed, ()), ("disabled", deformed, (len(static),)), ("enabled", deformed, ())]
        _REFIT_REF.update(scene=sc, matrix=m, verts=verts, states=[(what, dict(_refs(orc, prims, rays, q, disabled=off), name=what)) for what, prims, off in states])
    return _REFIT_REF


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(REFITS))
def test_trees_a_refit_wrote(R, torch, orc, get_scene, form):
    """4: Cornell with its last primitive as a model of its own on a dynamic scene that never rebuilds (refit_rebuild_ratio -1), under the refit's presets, with the
    quantised records made inside the refit's own workgroups (refit_fold_nodes 1), refitted in place (as_versions 1) and with every refit on its caller's stream
    (refit_streams 0xFFFFFFFF): after a matrix move, after art_scene_set_vertices, after the primitive is disabled and after it is enabled again the three kinds run on
    one side stream with no synchronisation in between, and each is the reference over the world vertices as of its call"""
    ref = _refit_states(orc, get_scene)
    sc = ref["scene"]
    r = R.Renderer((64, 64), dynamic_scene=True, tuning=dict({"refit_rebuild_ratio": -1.0}, **REFITS[form]))
    r.add_model(list(sc.primitives[:-1]))
    r.add_model([sc.primitives[-1]])
    r.prepare_first_frame()
    model = r.models_mut()[1]
    pid = model.primitive_ids[0]
    first = ref["states"][0][1]
    d_in = (_up(torch, first["rays"]), _up(torch, first["q"]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for what, c in ref["states"]:
        if what == "moved": model.set_model_matrix(ref["matrix"])
        elif what == "deformed": model.set_vertices(0, ref["verts"])
        elif what == "disabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 0) == 0
        elif what == "enabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 1) == 0
        assert not r.needs_build()
        with torch.cuda.stream(s):
            outs.append(_enqueue_kinds(r, torch, c, d_in=d_in))
    s.synchronize()
    for (what, c), got in zip(ref["states"], outs):
        _check_kinds(got, c, f"{form}, {what}")
    w = [c for _, c in ref["states"]]
    assert not np.array_equal(w[0]["closest"][0], w[1]["closest"][0]) and not np.array_equal(w[1]["closest"][1], w[2]["closest"][1]) and not np.array_equal(w[0]["sweep"][RHO][0], w[1]["sweep"][RHO][0])
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 3, st
    r.close()


# ---- 5: mixed kinds on the ring --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_ring_with_kinds_mixed_on_three_streams(R, torch, orc, get_scene):
    """5: 80 operations -- multi K = 4, closest_points, cast_spheres, resolve_hits, cast_rays in turn -- over three torch streams, sponza_like at 0.05 with 1024 inputs
    each, nothing synchronised before the end: the ring of ART_CAST_POOL cursor blocks is lapped with neighbours of different kinds on different streams (a block's
    cursors are zeroed on its caller's stream).  Every result is its reference; the casts and rays counted are the 48 ray casts', and the host waited at most once per
    operation beyond the pool"""
    from araytracingjourney_amd import _lib
    assert 80 > 2 * _lib.ART_CAST_POOL
    c = _sponza(orc, get_scene)
    n = 1024
    quiet = R.renderer_for_scene(c["scene"], (64, 64))
    rec = (_up(torch, c["closest"][0][:n]), _up(torch, c["closest"][1][:n]))   # the records the resolves read: the nearest points'
    want_res = {o: _words(t) for o, t in quiet.resolve_hits(rec[0], rec[1], OUTPUTS).items()}
    torch.cuda.synchronize()
    quiet.close()
    assert any(w.any() for w in want_res.values())
    r = R.renderer_for_scene(c["scene"], (64, 64))
    d_rays, d_q = _up(torch, c["rays"][:n]), _up(torch, c["q"][:n])
    streams = [torch.cuda.Stream() for _ in range(3)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(80):
        with torch.cuda.stream(streams[i % 3]):
            kind = ("multi", "closest", "sweep", "resolve", "cast")[i % 5]
            outs.append((kind, {"multi": lambda: r.cast_rays_multi(d_rays, 4), "closest": lambda: r.closest_points(d_q), "sweep": lambda: r.cast_spheres(d_rays, RHO),
                                "resolve": lambda: r.resolve_hits(rec[0], rec[1], OUTPUTS), "cast": lambda: r.cast_rays(d_rays)}[kind]()))
    counts = r.cast_counts()
    for s in streams:
        s.synchronize()
    one = _want_multi(c, 1, n)
    for i, (kind, got) in enumerate(outs):
        what = f"operation {i} ({kind})"
        if kind == "multi":
            tm._same(got, _want_multi(c, 4, n), what)
        elif kind == "closest":
            tcp._same(_host(got), tuple(w[:n] for w in c["closest"]), what)
        elif kind == "sweep":
            tsc._same(_host(got), tuple(w[:n] for w in c["sweep"][RHO]), what)
        elif kind == "resolve":
            for o, t in got.items():
                assert np.array_equal(_words(t), want_res[o]), f"{what}: {o}"
        else:
            assert np.array_equal(got[1].cpu().numpy(), one[1][:, 0]) and np.array_equal(_words(got[0])[:, :3], np.ascontiguousarray(one[0][:, 0, :3]).view(np.uint32)) and not _words(got[0])[:, 3].any(), what
    assert counts["casts"] == 48 and counts["rays"] == 48 * n and counts["host_waits"] <= 80 - _lib.ART_CAST_POOL, counts
    r.close()


# ---- 6: other contexts -----------------------------------------------------------------------------------------------------------------------------------------------
def _launches_with_queries(R, torch, c, kw, fpl, queries):
    """two launches of a 64 x 64 context with the three kinds enqueued between them on a side stream (queries) or nothing; one synchronisation at the end -> (every
    frame of the last launch: colour, depth, normal; the kinds' outputs)"""
    r = R.renderer_for_scene(c["scene"], (64, 64), **kw)
    if fpl > 1:
        r.set_frames_per_launch(fpl)
    d_in = (_up(torch, c["rays"]), _up(torch, c["q"]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    r.upload_state(); r.trace()
    got = None
    if queries:
        with torch.cuda.stream(s):
            got = _enqueue_kinds(r, torch, c, d_in=d_in)
    r.upload_state(); r.trace()
    r.sync(); s.synchronize()
    frames = []
    for b in range(fpl):
        if fpl > 1:
            r.set_read_frame(b)
        frames.append([r.read_color(), r.read_depth(), r.read_normal()] + ([r.read_color_tiles()] if "shard" in kw else []))
    r.close()
    return frames, got


def _ring_with_queries(R, torch, c, queries, frames=8):
    """8 frames through a ring of 8, the camera stepping, with the three kinds enqueued behind the fourth on the context's own cast stream (queries) or nothing, and no
    host synchronisation until all is enqueued.  Every frame's colour, depth and normal are copied out of its slot by a side stream that waits for the frame
    (art_stream_wait_frame), as tests/test_cast.py copies them"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    sc = c["scene"]
    r = R.renderer_for_scene(sc, (64, 64), frames_in_flight=frames)
    d_in = (_up(torch, c["rays"]), _up(torch, c["q"]))
    copy_s = torch.cuda.Stream()
    torch.cuda.synchronize()
    pos = np.asarray(sc.camera["pos"], np.float64)
    kept, got = [], None
    for f in range(frames):
        r.camera_mut().set_pos(tuple(pos + 0.01 * f * np.array([1.0, 0.5, -0.5])))
        r.upload_state(); r.trace()
        r.stream_wait_frame(copy_s.cuda_stream)
        bufs = []
        for ptr, nbytes in (r.device_color(), r._dev("depth"), r._dev("normal")):
            t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            assert hip.hipMemcpyAsync(t.data_ptr(), ptr, nbytes, 3, copy_s.cuda_stream) == 0   # hipMemcpyDeviceToDevice
            bufs.append(t)
        kept.append(bufs)
        if queries and f == 3:
            got = _enqueue_kinds(r, torch, c, d_in=d_in, null_stream=True)
    in_flight = r.frames_traced()
    r.cast_sync(); r.sync(); copy_s.synchronize()
    assert in_flight == frames
    out = [[b.cpu().numpy() for b in bufs] for bufs in kept]
    r.close()
    return out, got


@pytest.mark.gpu
@pytest.mark.parametrize("context", ["shard-1-of-4", "two-frames-per-launch", "eight-frames-in-flight"])
def test_other_contexts_answer_alike_and_their_frames_do_not_notice(R, torch, orc, get_scene, context):
    """6: the three kinds on a context that traces the second of four shards, on one that traces two frames per launch, and -- on the context's own cast stream
    (hip_stream NULL, art_cast_sync as the fence) -- while the 8 frames of a ring of 8 are being traced: Cornell's 4097-input references every time, and every frame's
    colour, depth and normal are those of the same run without queries, bit for bit"""
    c = _case(orc, get_scene, "cornell")
    if context == "eight-frames-in-flight":
        run = lambda queries: _ring_with_queries(R, torch, c, queries)   # noqa: E731
    else:
        kw, fpl = (dict(shard=(1, 4)), 1) if context == "shard-1-of-4" else (dict(frames_in_flight=2), 2)
        run = lambda queries: _launches_with_queries(R, torch, c, kw, fpl, queries)   # noqa: E731
    plain, _ = run(False)
    mixed, got = run(True)
    _check_kinds(got, c, context)
    assert len(plain) == len(mixed) >= 1
    for f, (a, b) in enumerate(zip(plain, mixed)):
        for what, x, y in zip(("colour", "depth", "normal", "colour tiles"), a, b):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), f"{context}, frame {f}: {what} differs beside the queries"
    assert any(np.ascontiguousarray(x).view(np.uint8).any() for x in plain[0])
    if len(plain) > 1:
        assert any(not np.array_equal(plain[0][1], plain[f][1]) for f in range(1, len(plain))) or context == "two-frames-per-launch"
