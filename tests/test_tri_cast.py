"""art_cast_triangles (include/art.h): the first contact of each of a buffer of translating query triangles with the scene -- defined exactly and checked
bit for bit.

The reference is tests/np_tri_sweep.py: the sixteen features (S and the fifteen moving ones), the shifted-box slab and the argmin of (t_eff, gid) in numpy float32,
operation by operation, on np_closest.world_triangles' fields; the 17 axes, S's witnesses and the slab's fma are np_tri_overlap's, np_tri_distance's and np_sweep's
functions, imported.  Nothing on the device has a tolerance: the words of t, u, v, the ids and both points.  A reference is computed once per set of inputs, shared and
never written.

The CPU tests tie the reference to an independent float64 witness (np_tri_sweep.witness: Moeller-Trumbore for vertex against face, a 3 x 3 solve for an edge pair,
test_tri_overlap's witness for "they share a point at tmin").  Times are compared, never ids.  The bound is on |t32 - t64| / max(1, tmax - tmin); it is four times the
worst figure measured on the set, rounded up to one digit (tests/golden/tri_cast.stats.json has the measurements and the seeds; |d| is about 3, tmin = 0, tmax = 1):
    random pairs (20 000, 5 802 contacts)                    worst 1.71e-6, p99.9 5.9e-7     bound 7e-6
    the same offset by 100 units (20 000, 5 917)             worst 1.00e-6, p99.9 4.6e-7     bound 4e-6
    nearly parallel edges (20 000, 20 000)                   worst 3.44e-5, p99.9 1.25e-7    bound 2e-4
The sets hold no pair that touches at tmin (the start distance is above START_MARGIN = 1e-3) and the witness's contacts stay LIMIT_MARGIN = 1e-4 away from tmax: within
those margins hit / miss disagreements between the model and the witness are counted, listed and asserted to be none (measured: none on any set).
What wins in the references the device is compared with (misses / S, the start / won by a query vertex, a scene vertex, an edge pair):
    Cornell 1.0 (4096 queries, 34 triangles)         1 411 / 1 331 / 1 126,    79,   149      ties on t_eff: 1 169
    sponza_like 0.05 (4096, 7 144)                   1 205 / 1 370 / 1 076,    43,   402                     1 317
    the lattice (2071, 576)                            593 / 1 327 /   134,    10,     7                     1 317
    the clump (256, 1000)                              152 /    54 /     4,    12,    34                        69
    the chain (130, 64)                                 18 /   107 /     2,     0,     3                        86
    the soup (1024, 600)                               590 /    74 /    59,    74,   227                       185
    the specials on sponza_like (811, 7 144)           144 /   421 /   183,    14,    49                       417
Mutation checks, on scratch builds of the library run over the 44 GPU tests of this module (profiles/tri_cast_mutants.txt has pytest's lines):
  * the strict `>` of the node skip made `>=` (a child whose box is entered exactly at tbest is dropped, and with it the smaller gid among ties): 43 tests fail; the
    errors pass.
  * the edge pairs dropped from the leaf: 41 tests fail; the errors and sweep_mesh (a box face down on a floor: vertices in a face) pass.
  * the gid tie rule dropped (a tie is taken only by the first candidate): 41 tests fail; the errors and sweep_mesh's box without a matrix and with one pass.
  * the absent-child byte test dropped from the node step: NO test fails.  An absent child's reference is the leaf that is nothing and a triangle out by residency is
    refused by its own record, so in this kernel the byte test saves visits and decides no record; a test of results cannot tell the builds apart.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import np_tri_distance as ntd
import np_tri_overlap as nto
import np_tri_sweep as ns
import test_closest_points as tcp
import test_query_forms as tqf
import test_tri_overlap as tto
from helpers import chain_scene, degenerate_soup, lattice_scene
from helpers import _layout_is_the_headers, _host, R, torch, _up, _bits  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = tto.PATTERN
N = tto.N
WHO = b"art_cast_triangles: "
F = np.float32
INF = F(np.inf)
STATS = os.path.join(ROOT, "tests", "golden", "tri_cast.stats.json")
START_MARGIN, LIMIT_MARGIN = 1e-3, 1e-4

_REF = {}


# ---- inputs and references ---------------------------------------------------------------------------------------------------------------------------------------
def _cycle(values, n):
    return np.resize(np.asarray(values, F), n)


def _limits(q, tmins, tmaxs):
    """tmin and tmax cycling through the given values; a tmax of None is "tmin": an empty range"""
    n = q.shape[0]
    q[:, 3] = _cycle(tmins, n)
    tm = np.resize(np.asarray([np.nan if t is None else t for t in tmaxs], F), n)
    q[:, 7] = np.where(np.isnan(tm), q[:, 3], tm)
    return q


def scene_sweeps(T, seed):
    """4096 queries of two populations.  2048 random triangles (test_tri_overlap.scene_queries' first half: a centre in the scene's box, 0.3 % .. 30 % of the extent
    wide) whose d points at a random point of the scene's box, away from it, or along a world axis (two components 0: safe_dir's branch), in turn.  2048 of the scene's own
    triangles moved off by an offset o of 0.1 % .. 2 % of the extent, whose d is -2o (towards: back onto its own triangle at t = 0.5, with every neighbour that shares an
    edge or a vertex), +2o (away), a direction across o (along the surface), an axis, 0 (only S answers) and a long random one, in turn.  tmin cycles through 0, 0, 0.25
    and -0.5; tmax through 1, 2, +inf, tmin (an empty range), 0.5 and 1e30.  Words 11 and 15, which are not read, hold a NaN and -inf"""
    lo, hi = tto.scene_bounds(T)
    rng = np.random.default_rng(seed)
    ext = float((hi - lo).max())
    h = N // 2
    c = lo + rng.uniform(0.0, 1.0, (h, 3)) * (hi - lo).astype(np.float64)
    half = ext * 10.0 ** rng.uniform(-2.5, -0.5, (h, 1, 1))
    rnd = c[:, None, :] + half * rng.uniform(-1.0, 1.0, (h, 3, 3))
    to = lo + rng.uniform(0.0, 1.0, (h, 3)) * (hi - lo).astype(np.float64) - c
    axis = np.eye(3)[rng.integers(0, 3, h)] * (ext * rng.uniform(-1.0, 1.0, (h, 1)))
    kind = np.arange(h) % 3
    d_rnd = np.where(kind[:, None] == 0, to, np.where(kind[:, None] == 1, -to, axis))
    own = T["w"][rng.integers(0, T["w"].shape[0], h)].astype(np.float64)
    o = rng.normal(0.0, 1.0, (h, 3))
    o *= (ext * 10.0 ** rng.uniform(-3.0, -1.7, h) / np.linalg.norm(o, axis=1))[:, None]
    across = np.cross(o, own[:, 1] - own[:, 0])
    across *= (ext * 0.05 / np.maximum(np.linalg.norm(across, axis=1), 1e-30))[:, None]
    kind = np.arange(h) % 6
    d_own = np.select([kind[:, None] == k for k in range(6)], [-2.0 * o, 2.0 * o, across, axis * 0.1, np.zeros((h, 3)), rng.normal(0.0, ext, (h, 3))])
    q = ns.sweeps_of(np.concatenate([rnd, own + o[:, None, :]]), np.concatenate([d_rnd, d_own]))
    q = _limits(q, [0.0, 0.0, 0.25, -0.5], [1.0, 2.0, np.inf, None, 0.5, 1e30, 1.0])
    q[:, 11], q[:, 15] = np.nan, -np.inf
    return q


def _ref(key, make):
    """{scene, T, q, want, stats} of a set of inputs: make() -> (scene, queries); computed once, shared, never written"""
    if key not in _REF:
        sc, q = make()
        T = ns.world_triangles(sc.primitives)
        q = np.ascontiguousarray(q, F)
        q.setflags(write=False)
        *want, stats = ns.brute_force(T, q, stats=True)
        _REF[key] = dict(scene=sc, T=T, q=q, want=tto._frozen(tuple(want)), stats=tto._frozen(stats))
    return _REF[key]


def _scene_ref(get_scene, name, detail):
    def make():
        sc = get_scene(name, detail)
        return sc, scene_sweeps(ns.world_triangles(sc.primitives), 13)
    return _ref((name, detail), make)


LIVE = ns.sweeps_of([[(-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5)]], (0.25, 0.5, -0.25), 0.0, 1.0)[0]


def dead_queries():
    """a NaN, +inf and -inf in each of the twelve inputs in turn (the nine coordinates, the three of d) -- 36 triangles round the origin that would otherwise touch
    anything there -- and a NaN tmax: miss records that carry tmax as given"""
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        for k in ns.COORDS + [12, 13, 14]:
            q = LIVE.copy()
            q[k] = bad
            out.append(q)
    q = LIVE.copy()
    q[7] = np.nan
    return np.stack(out + [q]).astype(F)


def special_queries(T):
    """test_tri_overlap.special_queries on sponza_like -- [0] larger than the scene, [1] reaching 3e37, [2] far away; for 64 scene triangles the triangle handed back (it
    touches as it starts: S), its first vertex as a point (starts touching at a vertex), its centroid as a point, a segment through the face (starts cutting: S), a
    segment along its first edge, and a copy turned in its own plane (coplanar, apart) -- with d cycling through: along the triangle's normal towards it, 0, along its
    first edge (in the plane: coplanar sliding, which only S sees), a world axis, a long diagonal; tmax through 1, +inf, 4; then the three big ones again with tmin = -1,
    the same 384 specials started half a normal step off the surface (contacts after tmin), and the dead queries"""
    lo, hi = tto.scene_bounds(T)
    ext = float((hi - lo).max())
    base = tto.special_queries(T)[:-27]
    tri = base[:, ns.COORDS].reshape(-1, 3, 3)
    w = T["w"][::max(1, T["w"].shape[0] // tto.N_OWN)][:tto.N_OWN]
    n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]).astype(np.float64)
    n = n / np.maximum(np.linalg.norm(n, axis=1), 1e-30)[:, None] * 0.03 * ext
    edge = (w[:, 1] - w[:, 0]).astype(np.float64)
    per = tto.PER_OWN
    d = np.zeros((tri.shape[0], 3))
    d[0], d[1], d[2] = (0.0, -0.5 * ext, 0.0), (1e37, 0.0, -1e37), lo - hi - 2.0
    choices = np.stack([-n, np.zeros_like(n), edge, np.tile([0.0, 0.1 * ext, 0.0], (n.shape[0], 1)), np.tile([ext, -ext, ext], (n.shape[0], 1))], 1)   # [64, 5, 3]
    k = np.arange(3, tri.shape[0])
    d[3:] = choices[(k - 3) // per, k % 5]
    a = _limits(ns.sweeps_of(tri, d), [0.0], [1.0, np.inf, 4.0])
    a[2, 7] = np.inf
    big = a[:3].copy()
    big[:, 3] = -1.0
    off = tri[3:] + np.repeat(0.5 * n, per, axis=0)[:, None, :]
    b = _limits(ns.sweeps_of(off, np.repeat(-n, per, axis=0)), [0.0, 0.0, 0.25], [1.0, np.inf, 0.4, 4.0])
    return np.concatenate([a, big, b, dead_queries()]).astype(F)


def lattice_sweeps():
    """test_tri_overlap.lattice_queries -- triangles and points whose vertices are lattice points, every coordinate a multiple of 0.25 like every vertex of the scene --
    as they stand (touching as they start: S, ties by the dozen) and moved off by 0.125 along an axis; d a multiple of 0.25 along an axis or a diagonal.  Every product
    and sum is exact: contacts at t = 0.5, 0.25 .. are shared by the triangles that share the vertex or the edge that is met, and the gid rule decides"""
    q3 = tto.lattice_queries()[:, ns.COORDS].reshape(-1, 3, 3).astype(np.float64)
    n = q3.shape[0]
    unit = np.eye(3)[np.arange(n) % 3]
    shift = np.where((np.arange(n) % 2 == 0)[:, None], 0.0, 0.125) * unit
    sign = np.where(np.arange(n) % 4 < 2, 1.0, -1.0)[:, None]
    d = np.where((np.arange(n) % 5 == 4)[:, None], np.array([0.25, -0.25, 0.5]), -0.25 * sign * unit)
    return _limits(ns.sweeps_of(q3 + (sign * shift)[:, None, :], d), [0.0, 0.0, 0.25], [1.0, np.inf, 4.0, None, 0.5])


HOSTILE = ["lattice", "clump", "chain", "soup", "specials"]


def _hostile(get_scene, which):
    if which == "lattice":
        return _ref(which, lambda: (lattice_scene(6), lattice_sweeps()))
    if which == "clump":     # 1000 triangles in one place: the stack past its eight LDS pairs
        def make():
            t = tto.clump_queries()[:, ns.COORDS].reshape(-1, 3, 3).astype(np.float64)
            rng = np.random.default_rng(4)
            off = rng.normal(0.0, 0.2, (t.shape[0], 3))
            d = np.where((np.arange(t.shape[0]) % 4 == 3)[:, None], rng.normal(0.0, 0.3, (t.shape[0], 3)), -2.0 * off)
            return degenerate_soup(1000, "one point"), _limits(ns.sweeps_of(t + off[:, None, :] * (np.arange(t.shape[0]) % 2)[:, None, None], d), [0.0], [1.0, np.inf, 0.25])
        return _ref(which, make)
    if which == "chain":     # 64 nested slivers: a deep stack
        def make():
            t = tto.chain_queries()[:, ns.COORDS].reshape(-1, 3, 3).astype(np.float64)
            d = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -0.02], [-0.5, 0.001, 0.0]])[np.arange(t.shape[0]) % 4]
            up = np.array([0.0, 0.0, 0.015]) * (np.arange(t.shape[0]) % 3 == 1)[:, None]
            return chain_scene(64)[0], _limits(ns.sweeps_of(t + up[:, None, :], d), [0.0], [np.inf, 1.0, 4.0])
        return _ref(which, make)
    if which == "soup":      # duplicated and zero-area triangles
        def make():
            sc = degenerate_soup(600, "soup")
            return sc, scene_sweeps(ns.world_triangles(sc.primitives), 5)[::4]
        return _ref(which, make)
    sc = get_scene("sponza_like", 0.05)
    return _ref(which, lambda: (sc, special_queries(ns.world_triangles(sc.primitives))))


CASES = ["cornell", "sponza_like"] + HOSTILE


def _case(get_scene, name):
    return _scene_ref(get_scene, name, 0.05 if name == "sponza_like" else 1.0) if name in ("cornell", "sponza_like") else _hostile(get_scene, name)


def _same(got, want, what=""):
    """ids, the bits of t, u, v, a fourth word of 0, the bits of both points"""
    (tuv, ids, point, qpoint), (rtuv, rids, rpoint, rqpoint) = got, want
    assert tuv.shape == rtuv.shape and ids.shape == rids.shape and point.shape == rpoint.shape and qpoint.shape == rqpoint.shape, what
    bad = (ids != rids).any(axis=1)
    assert not bad.any(), f"{what}: the ids of {int(bad.sum())} of {ids.shape[0]} queries differ (first: {np.flatnonzero(bad)[:5]}: {ids[bad][:2]} for {rids[bad][:2]}, t {tuv[bad][:2, 0]} for {rtuv[bad][:2, 0]})"
    bad = (_bits(tuv)[:, :3] != _bits(rtuv)[:, :3]).any(axis=1)
    assert not bad.any(), f"{what}: t, u, v of {int(bad.sum())} queries differ (first: {np.flatnonzero(bad)[:5]}: {tuv[bad][:2]} for {rtuv[bad][:2]})"
    assert not _bits(tuv)[:, 3].any(), f"{what}: the fourth word is not 0"
    assert np.array_equal(_bits(point), _bits(rpoint)), f"{what}: the scene points differ"
    bad = (_bits(qpoint) != _bits(rqpoint)).any(axis=1)
    assert not bad.any(), f"{what}: the query points of {int(bad.sum())} queries differ (first: {np.flatnonzero(bad)[:5]}: {qpoint[bad][:2]} for {rqpoint[bad][:2]})"


def _cut(want, n=None, at=None):
    return tuple(w[:n] if at is None else w[at] for w in want)


def _ask(r, torch, q, **kw):
    got = r.cast_triangles(_up(torch, q), **kw)
    torch.cuda.synchronize()
    return _host(got)


def _patterned(torch, n):
    return (torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((n, 2), PATTERN, dtype=torch.int32, device="cuda"),
            torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32))


def _untouched(outs, n):
    return all((t[n:].view(outs[1].dtype) == PATTERN).all() for t in outs)


def _ask_into(r, torch, q, extra, what, stream=None, **kw):
    """into tensors `extra` records too long and filled with a pattern: the tail keeps it"""
    n = q.shape[0]
    outs = _patterned(torch, n + extra)
    d_q = _up(torch, np.asarray(q).reshape(n, 16))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        got = r.cast_triangles(d_q, out=outs, **kw)
        assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert _untouched(outs, n), f"{what}: written beyond n"
    return _host(tuple(t[:n] for t in outs))


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_ctypes_descriptor_is_the_headers():
    """ArtTriCast as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 64 bytes"""
    _layout_is_the_headers("ArtTriCast", 64, ["sweeps_dev", "tuv_dev", "ids_dev", "point_dev", "qpoint_dev", "hip_stream", "n", "cull_mask", "flags", "reserved"])


def test_presence():
    """art_cast_triangles(NULL, NULL) is ART_E_INVALID with the prefixed message on any machine; the library exports it, the Rust binding declares the function and the
    struct, the header cites DESIGN.md 3.15 and states the limitation, the C++ mirror has the call, and Renderer has both methods"""
    from araytracingjourney_amd import _lib, renderer
    L = _lib.load()
    assert L.art_cast_triangles(None, None) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    d = _lib.ArtTriCast(flags=1)
    nowhere = C.create_string_buffer(1 << 16)
    assert L.art_cast_triangles(nowhere, C.byref(d)) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"flags: must be 0"
    so = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "art_cast_triangles" for line in syms.splitlines() if line.strip())
    rs = open(os.path.join(ROOT, "bindings", "art_sys.rs")).read()
    assert "pub fn art_cast_triangles(" in rs and "pub struct ArtTriCast" in rs
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "DESIGN.md 3.15" in hdr and "LIMITATION" in hdr and "### 3.15" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "art_cast_triangles(" in open(os.path.join(ROOT, "araytracingjourney_amd", "host", "art_renderer.hpp")).read()
    assert callable(renderer.Renderer.cast_triangles) and callable(renderer.Renderer.sweep_mesh)


def _one(tri, query, d, tmin=0.0, tmax=1.0, mutate=None):
    """one scene triangle, one query: (t, u, v, hit, point, qpoint, feature name)"""
    w = np.asarray(tri, F).reshape(1, 3, 3)
    T = dict(w=w, v0=w[:, 0].copy(), e1=w[:, 1] - w[:, 0], e2=w[:, 2] - w[:, 0], lo=w.min(axis=1), hi=w.max(axis=1), prim=np.zeros(1, np.int32), tri=np.zeros(1, np.int32))
    tuv, ids, point, qpoint, st = ns.brute_force(T, ns.sweeps_of([query], d, tmin, tmax), stats=True, mutate=mutate)
    f = int(st["feature"][0])
    return float(tuv[0, 0]), float(tuv[0, 1]), float(tuv[0, 2]), bool(ids[0, 0] == 0), point[0, :3].tolist(), qpoint[0, :3].tolist(), ns.FEATURES[f] if f >= 0 else None


def _th(x):
    return x[0], x[3]   # (t, hit)


def test_known_answers():
    """the triangle (0,0,0) (1,0,0) (0,1,0), every coordinate exact: a query vertex entering the face, a scene vertex entering a big query's face, two edges crossing
    where no vertex of either is (and neither vertex group finds it), the start (S) for a cutting pair and for one that touches at a vertex, t_eff at tmin and below
    tmax only, d = 0, points and segments as queries, a zero-area scene triangle, and coplanar sliding as specified: seen where it touches at tmin, not after"""
    t = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    down = (0, 0, -1)
    assert _one(t, [(0.25, 0.25, 0.5), (0.5, 0.25, 1), (0.25, 0.5, 1)], down) == (0.5, 0.25, 0.25, True, [0.25, 0.25, 0.0], [0.25, 0.25, 0.5], "QV0")
    tt, u, v, hit, p, qp, f = _one(t, [(-4, -4, 0.25), (8, -4, 0.25), (-4, 8, 0.25)], down)
    assert (tt, hit, f) == (0.25, True, "SV0") and p == [0.0, 0.0, 0.0] and qp == [0.0, 0.0, 0.25]
    cross = [(0.5, -1, 0.25), (0.5, 1, 0.25), (0.5, 0, 8)]                                     # its first edge comes down on the edge v0 v1 at (0.5, 0, 0)
    far = [(0, 0, 0), (1, 0, 0), (0.5, -4, -4)]
    tt, u, v, hit, p, qp, f = _one(far, cross, down)
    assert (tt, u, v, hit, p, qp, f) == (0.25, 0.5, 0.0, True, [0.5, 0.0, 0.0], [0.5, 0.0, 0.25], "E00")
    assert _one(far, cross, down, mutate="no edge pairs")[0] > 0.25                             # without the pairs a vertex finds a later contact, or none
    cut = [(0.2, 0.2, -1), (0.2, 0.2, 1), (0.3, 0.9, 1)]                                        # an edge of the query pierces the face as it starts
    assert _th(_one(t, cut, down)) == (0.0, True) and _one(t, cut, down)[6] == "S" and _one(t, cut, (0, 0, 0))[6] == "S"
    assert _one(t, cut, down, tmin=0.25, tmax=2.0)[0] == 0.25                                    # still cutting at 0.25
    assert _one(t, cut, down, mutate="no start")[6] != "S"
    touch = [(1, 0, 0), (2, 0, 1), (2, 1, -1)]                                                   # touching at one vertex as it starts
    assert _th(_one(t, touch, (1, 0, 0))) == (0.0, True) and _one(t, touch, (1, 0, 0))[6] == "S"
    par = [(0.1, 0.1, 0.5), (0.4, 0.1, 0.5), (0.1, 0.4, 0.5)]                                    # parallel planes, 0.5 apart
    assert _th(_one(t, par, down)) == (0.5, True) and _th(_one(t, par, down, tmax=0.5)) == (0.5, False) and _one(t, par, down, tmax=0.5)[4:6] == ([0.0] * 3, [0.0] * 3)
    assert _th(_one(t, par, down, tmin=0.5)) == (0.5, True) and _one(t, par, down, tmin=0.75, tmax=4.0)[3] is False   # at tmin: S; past the plane: nothing
    assert _one(t, par, (0, 0, 0))[3] is False and _one(t, par, (0, 0, 1))[3] is False and _one(t, par, (0, 0, -0.25), tmax=np.inf)[0] == 2.0
    assert _th(_one(t, [(0.25, 0.25, 2)] * 3, down, tmax=4.0)) == (2.0, True)                    # a point
    assert _one(t, [(0.25, 0.25, 2), (0.25, 0.25, 2), (0.25, 0.25, 3)], down, tmax=4.0)[0] == 2.0    # a segment
    seg = [(0, 0, 0), (1, 0, 0), (0.5, 0, 0)]                                                    # a zero-area scene triangle: a segment
    assert _th(_one(seg, [(0.5, -1, 1), (0.5, 1, 1), (0.5, 0, 4)], down, tmax=4.0)) == (1.0, True)
    slide = [(2, 0, 0), (3, 0, 0), (2, 1, 0)]                                                    # coplanar, apart, sliding in the common plane: only S sees it
    assert _one(t, slide, (-4, 0, 0))[3] is False
    met = [(1, 0, 0), (2, 0, 0), (1, 1, 0)]                                                      # the same, touching at (1, 0, 0) as it starts
    assert _th(_one(t, met, (-4, 0, 0))) == (0.0, True) and _one(t, met, (-4, 0, 0))[6] == "S" and _one(t, met, (4, 0, 0))[6] == "S"
    # posed at 0.25 `slide` touches at (1, 0, 0) too, and S would say so -- but both boxes are flat in z and d.z is 0: 1.1's slab gives that axis the single time
    # 0 * (1 / 1e-20) = 0, which [0.25, 1) does not hold: no candidate ("coplanar sliding")
    assert _th(_one(t, slide, (-4, 0, 0), tmin=0.25)) == (1.0, False) and _th(_one(t, slide, (-4, 0, 0), tmin=-0.25)) == (1.0, False)
    tilt = [(0, 0, 0), (1, 0, 0.5), (0, 1, 0)]                                                   # a plane that is no axis plane: the same slide is S's at tmin
    assert _th(_one(tilt, [(2, 0, 1), (3, 0, 1.5), (2, 1, 1)], (-4, 0, -2), tmin=0.25)) == (0.25, True) and _one(tilt, [(2, 0, 1), (3, 0, 1.5), (2, 1, 1)], (-4, 0, -2))[3] is False


def pair_sets():
    """{name: (scene triangles [P, 3, 3], query triangles [P, 3, 3], d [P, 3])} float32, 20 000 pairs each, tmin = 0, tmax = 1: random pairs about the origin, the query 3
    units off and swept back with |d| about 3; the same offset by 100 units; and nearly parallel edges -- a copy of the triangle moved off by 0.3 .. 1 and perturbed by
    1e-4, swept back along the offset, which leaves the triangle's plane.  No pair touches within START_MARGIN as it starts (asserted where the sets are used: they
    test the moving features; S is test_tri_overlap's condition, which has a witness test of its own there)"""
    out, P = {}, 20_000
    for name, seed, off in (("random", 1, 0.0), ("offset 100", 2, 100.0)):
        rng = np.random.default_rng(seed)
        w = rng.uniform(-1, 1, (P, 3, 3))
        dirn = rng.normal(size=(P, 3))
        dirn /= np.linalg.norm(dirn, axis=1)[:, None]
        q = rng.uniform(-1, 1, (P, 3, 3)) + (3.0 * dirn)[:, None, :]
        d = -(3.0 * dirn) + rng.uniform(-1, 1, (P, 3))
        out[name] = ((w + off).astype(F), (q + off).astype(F), d.astype(F))
    rng = np.random.default_rng(3)
    w = rng.uniform(-1, 1, (P, 3, 3))
    dirn = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
    dirn = dirn / np.linalg.norm(dirn, axis=1)[:, None] + rng.normal(0.0, 0.3, (P, 3))   # out of the triangle's plane: moved within it the copy would still cut it
    dirn /= np.linalg.norm(dirn, axis=1)[:, None]
    dist = rng.uniform(0.3, 1.0, (P, 1))
    q = w + (dist * dirn)[:, None, :] + rng.uniform(-1e-4, 1e-4, (P, 3, 3))
    out["nearly parallel"] = (w.astype(F), q.astype(F), (-3.0 * dirn).astype(F))
    return out


SEEDS = {"random": 1, "offset 100": 2, "nearly parallel": 3}
_PAIRS = {}


def _bounds():
    return {k: v["bound"] for k, v in json.load(open(STATS))["sets"].items()}


def _pair_times(name, mutate=None):
    """(t32 of the model, t64 of the witness, the set) over the set's pairs; inf: no contact"""
    if not _PAIRS:
        _PAIRS.update(pair_sets())
    w, q, d = _PAIRS[name]
    key = (name, "witness")
    if key not in _PAIRS:
        _PAIRS[key] = ns.witness(w, q, d, 0.0, 1.0)
        _PAIRS[(name, "start")] = ntd.witness(w, q)
    return ns.pair_model(w, q, d, 0.0, 1.0, mutate)[0].astype(np.float64), _PAIRS[key], (w, q, d)


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_model_against_the_witness(name):
    """|t32 - t64| / max(1, tmax - tmin) over every pair of the set on which both find a contact, within the set's bound; hit / miss disagreements are counted and
    listed, and outside the stated margins there is none; the recorded worst is what this run measures (the bound is four times it, one digit up)"""
    t32, t64, (w, q, d) = _pair_times(name)
    assert (_PAIRS[(name, "start")] > START_MARGIN).all(), "the set holds a pair that touches as it starts"
    h32, h64 = np.isfinite(t32), np.isfinite(t64)
    both = h32 & h64
    err = np.abs(t32[both] - t64[both])
    differ = np.flatnonzero(h32 != h64)
    inside = differ[~(np.minimum(t32[differ], t64[differ]) > 1.0 - LIMIT_MARGIN)]
    rec = json.load(open(STATS))["sets"][name]
    print(f"\n[tri cast] {name}: {t32.size} pairs, contacts {int(h32.sum())} / {int(h64.sum())}; |t32 - t64| worst {err.max():.3g}, p99.9 {np.quantile(err, 0.999):.3g}, median {np.median(err):.3g}; "
          f"hit / miss disagreements {differ.size}: {differ[:10].tolist()} (t32 {t32[differ][:10]}, t64 {t64[differ][:10]}), outside the margin {inside.size}")
    assert both.sum() > 5000 and err.max() <= rec["bound"]
    assert inside.size == 0
    assert rec["seed"] == SEEDS[name] and rec["pairs"] == t32.size and err.max() <= rec["worst"] * 1.0000001 and 4 * rec["worst"] <= rec["bound"] < 40 * rec["worst"]


@pytest.mark.parametrize("name", list(SEEDS))
def test_a_reported_time_is_a_touching_pose_and_no_earlier_pose_touches(name):
    """at every reported t the posed query is within |d| * bound of the scene triangle by np_tri_distance.witness (a pose within bound of a touching one: the triangle
    moves by |d| a unit of t), and of 16 poses sampled between tmin and t - bound none shares a point with it by np_tri_overlap.witness"""
    t32, t64, (w, q, d) = _pair_times(name)
    B = _bounds()[name]
    hit = np.flatnonzero(np.isfinite(t32))
    w, q, d, t = w[hit], q[hit], d[hit], t32[hit]
    gap = ns.touch_distance(w, q, d, t)
    speed = np.linalg.norm(d.astype(np.float64), axis=1)
    print(f"\n[tri cast] {name}: the distance at the reported pose: worst {gap.max():.3g}, worst over |d| * bound {(gap / (speed * B)).max():.3g}")
    assert (gap <= speed * B).all()
    before = np.zeros(hit.size, bool)
    for j in range(16):
        tj = (t - B) * (j / 16.0)
        before |= (tj >= 0) & nto.witness(w, ns.posed(q, d, np.maximum(tj, 0.0)))
    assert not before.any(), np.flatnonzero(before)[:10]


@pytest.mark.parametrize("mutate", ["no edge pairs", "no scene vertices"])
def test_the_witness_tells_mutated_models_apart(mutate):
    """the model with the edge pairs dropped, with the scene-vertex features dropped: contacts go missing or come a thousand bounds late"""
    t32, t64, _ = _pair_times("random", mutate)
    both = np.isfinite(t32) & np.isfinite(t64)
    late = np.abs(t32[both] - t64[both])
    lost = int((np.isfinite(t64) & ~np.isfinite(t32)).sum())
    print(f"\n[tri cast] random, {mutate}: contacts lost {lost}, worst |t32 - t64| {late.max():.3g}")
    assert lost > 100 and late.max() > 1000 * _bounds()["random"]


# what a set has to hold for its comparison to mean something: misses, S, winners among the query vertices, the scene vertices and the edge pairs, ties on t_eff
FLOORS = dict(cornell=(500, 100, 300, 20, 50, 100), sponza_like=(500, 100, 300, 20, 100, 100), lattice=(100, 300, 50, 1, 5, 300), clump=(10, 10, 1, 5, 10, 10),
              chain=(5, 10, 1, 0, 1, 10), soup=(100, 20, 20, 20, 50, 20), specials=(50, 100, 50, 5, 20, 50))


@pytest.mark.parametrize("name", CASES)
def test_the_comparisons_are_not_vacuous(get_scene, name):
    """from the reference alone: misses, contacts at the start (S), winners of each of the three moving groups -- a set on which no edge pair ever wins tests nothing of
    the new formula -- and ties on t_eff, which the gid rule decides"""
    ref = _case(get_scene, name)
    tuv, ids, point, qpoint = ref["want"]
    st, q = ref["stats"], ref["q"]
    f = st["feature"]
    miss = ids[:, 0] < 0
    counts = (int(miss.sum()), int((f == 0).sum()), int(((f >= 1) & (f <= 3)).sum()), int(((f >= 4) & (f <= 6)).sum()), int((f >= 7).sum()), int((st["ties"] > 1).sum()))
    print(f"\n[tri cast] {name}: {q.shape[0]} queries, {ref['T']['v0'].shape[0]} triangles, {st['pairs']} pairs evaluated; misses {counts[0]}, S {counts[1]}, won by a query vertex {counts[2]}, "
          f"a scene vertex {counts[3]}, an edge pair {counts[4]}; queries with a tie on t_eff {counts[5]}; box entries above t_tri {st['raised']}; tmax = inf {int(np.isinf(q[:, 7]).sum())}")
    assert all(c >= fl for c, fl in zip(counts, FLOORS[name])), (counts, FLOORS[name])
    assert (tuv[miss, 1:] == 0).all() and np.array_equal(_bits(tuv[miss, 0]), _bits(q[miss, 7])) and not point[miss].any() and not qpoint[miss].any()
    assert (point[~miss, 3] == 1).all() and (qpoint[~miss, 3] == 1).all()
    with np.errstate(invalid="ignore"):
        assert (tuv[~miss, 0] <= q[~miss, 7]).all() and (tuv[~miss, 0] >= q[~miss, 3]).all() and (q[:, 3] == q[:, 7])[miss].sum() >= (q[:, 3] == q[:, 7]).sum()
    if name in ("cornell", "sponza_like"):
        assert q.shape[0] == N
    if name == "lattice":
        assert int((st["ties"] > 4).sum()) > 100
    if name == "specials":
        assert ids[0, 0] >= 0 and ids[2, 0] >= 0 and miss[-37:].all() and np.isnan(tuv[-1, 0])


def test_coplanar_sliding_is_answered_as_specified(get_scene):
    """the specials' copies turned in their triangle's own plane and moved along its first edge: no moving feature has a denominator, so whatever they report against
    THAT triangle is S's; the model's answer is asserted, pair by pair, to be a miss or t = tmin"""
    ref = _case(get_scene, "specials")
    T, q = ref["T"], ref["q"]
    w = T["w"][::max(1, T["w"].shape[0] // tto.N_OWN)][:tto.N_OWN]
    at = 3 + np.arange(tto.N_OWN) * tto.PER_OWN + 5           # the turned copy of scene triangle k ...
    at = at[(at % 5) == 2]                                     # ... where d is that triangle's first edge
    assert at.size >= 10
    k = (at - 3) // tto.PER_OWN
    tri, d = q[at][:, ns.COORDS].reshape(-1, 3, 3), q[at, 12:15]
    t32, feat = ns.pair_model(w[k], tri, d, q[at, 3], q[at, 7])
    assert ((feat == 0) | (feat == -1)).all() and (t32[feat == 0] == q[at, 3][feat == 0]).all()


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_both_scenes_are_the_brute_forces(R, torch, get_scene, name, detail):
    """4096 queries on a side stream: t, u, v, ids and both points; a permutation of the queries gives the permuted records; oversized out= tensors filled with a
    pattern are untouched beyond n; the queries count as casts and rays"""
    ref = _scene_ref(get_scene, name, detail)
    q = ref["q"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    _same(_ask_into(r, torch, q, 70, name, stream=torch.cuda.Stream()), ref["want"], name)
    _same(_ask(r, torch, q[perm]), _cut(ref["want"], at=perm), f"{name}, permuted")
    assert r.cast_counts() == dict(casts=2, rays=2 * N, host_waits=0)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_inputs(R, torch, get_scene, which):
    """the lattice (exact times, ties by the dozen among triangles that share vertices and edges), 1000 triangles round one point (stacks past their LDS part), the chain
    of 64 nested slivers, a soup with duplicated and zero-area triangles, and on sponza_like a query larger than the scene, one at 3e37, scene triangles handed back,
    points, segments, d = 0, coplanar sliding and the dead queries of each kind"""
    ref = _hostile(get_scene, which)
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    _same(_ask_into(r, torch, ref["q"], 3, which), ref["want"], which)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(tqf.FORMS))
@pytest.mark.parametrize("name", ["clump", "chain", "cornell"])
def test_every_tree_form_gives_the_reference(R, torch, get_scene, name, form):
    """the answers are defined as independent of the structure: the clump, the chain and Cornell's 4096 queries on every tree form of tests/test_query_forms.py"""
    ref = _case(get_scene, name)
    r = R.renderer_for_scene(ref["scene"], (64, 64), **tqf.FORMS[form])
    _same(_ask(r, torch, ref["q"]), ref["want"], f"{name}, {form}")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", tqf.KNOBS, ids=lambda k: "-".join(f"{a}-{b}" for a, b in k.items()))
def test_knobs_change_the_schedule_never_the_records(R, torch, get_scene, knobs):
    """tests/test_query_forms.py's eight tracer settings (trace_chunk 64 / 65536, trace_refill 1 / 64, trace_blocks 1 / 16384, trace_leaf_batch 1 / 64) on sponza_like at
    0.05: the reference's bits.  (The loop is the point queries': why trace_leaf_batch = 64 and trace_refill = 64 cannot hang it is argued there)"""
    ref = _scene_ref(get_scene, "sponza_like", 0.05)
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning=knobs)
    _same(_ask(r, torch, ref["q"]), ref["want"], str(knobs))
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [64, 128])
def test_sizes_at_which_a_refill_can_go_wrong(R, torch, get_scene, chunk):
    """ArtTuning.trace_chunk = 64 (a chunk is one filling of a wave) and 128: prefixes of sponza_like's queries of tests/test_query_forms.py's sizes (0, 1, 63, 64, 65
    .. 4097) with a dead query at either end, then a batch that is all dead; every batch into tensors five records too long filled with a pattern.  n = 0 enqueues nothing"""
    ref = _scene_ref(get_scene, "sponza_like", 0.05)
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning={"trace_chunk": chunk})
    extra = np.concatenate([ref["q"], ref["q"][:1]])   # 4097
    want = tuple(np.concatenate([w, w[:1]]) for w in ref["want"])
    dead = dead_queries()
    dead_want = ns.brute_force(ref["T"], dead)
    assert {0, 1, 63, 64, 65, 4097} <= set(tqf.SIZES) and (dead_want[1] == -1).all()
    casts = 0
    for n in tqf.SIZES:
        before = r.cast_counts()
        q, w = extra[:n].copy(), tuple(x[:n].copy() for x in want)
        for at, k in ((0, 3), (n - 1, 36)) if n >= 2 else ():   # a dead query at either end
            q[at] = dead[k]
            for x, dx in zip(w, dead_want):
                x[at] = dx[k]
        _same(_ask_into(r, torch, q, 5, f"n = {n}"), w, f"n = {n}")
        casts += n > 0
        if n == 0:
            assert r.cast_counts() == before
    _same(_ask_into(r, torch, np.tile(dead, (4, 1))[:130], 5, "all dead"), tuple(np.tile(x, (4, 1))[:130] for x in dead_want), "all dead")
    assert r.cast_counts() == dict(casts=casts + 1, rays=sum(tqf.SIZES) + 130, host_waits=0)
    r.close()


@pytest.mark.gpu
def test_masks(R, torch, scenes, get_scene):
    """primitive masks set after the build against cull masks 0xFF, 1, 2, 0x80 and 0 (which sees nothing): with the first triangle masked out the next one answers;
    an alpha cutoff changes nothing"""
    sc = tcp._card_scene(scenes, get_scene)
    clear, solid = len(sc.primitives) - 2, len(sc.primitives) - 1
    T = ns.world_triangles(sc.primitives)
    q = scene_sweeps(T, 5)[::2]
    plain = ns.brute_force(T, q)
    assert int((plain[1][:, 0] == clear).sum()) > 10 and int((plain[1][:, 0] == solid).sum()) > 10
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    _same(_ask(r, torch, q), plain, "unmasked")
    m.set_alpha_cutoff(clear, 0.5); m.set_alpha_cutoff(solid, 0.5)
    _same(_ask(r, torch, q), plain, "with cutoffs: not tested")
    masks = {0: 0x01, 1: 0x02, solid: 0x03, clear: 0x02}
    for i, v in masks.items():
        m.set_mask(i, v)
    vis = np.array([masks.get(p, 0xFF) for p in range(len(sc.primitives))])
    for cull in (0xFF, 0x01, 0x02, 0x80, 0):
        want = ns.brute_force(T, q, vis=vis, cull=cull)
        got = _ask(r, torch, q, cull_mask=cull)
        _same(got, want, f"cull {cull:#x}")
        hidden = [p for p in range(len(sc.primitives)) if not (vis[p] & cull)]
        assert not np.isin(got[1][:, 0], hidden).any()
        if cull == 0:
            assert (got[1] == -1).all()
        if cull == 0x01:   # the clear card is masked out: where it was first, another triangle or a miss answers, and not earlier
            was = plain[1][:, 0] == clear
            later = got[1][was, 0] >= 0
            assert int(later.sum()) > 3 and (got[0][was, 0][later] >= plain[0][was, 0][later]).all()
    r.close()


@pytest.mark.gpu
def test_a_primitive_disabled_after_the_build_is_nowhere(R, torch, scenes, get_scene):
    """two primitives, one disabled after the build: it is never returned, also with tmax = +inf, by a query a million units wide and by one swept to where its
    record stands; enabled again, the first answers return"""
    sc = tcp._card_scene(scenes, get_scene)
    two = scenes.Scene("two", list(sc.primitives[-2:]), sc.camera, sc.lights)
    T = ns.world_triangles(two.primitives)
    q = scene_sweeps(T, 9)[::4].copy()
    q[::2, 7] = np.inf
    wide = ns.sweeps_of([[(-1e6, -1e6, 2.0), (1e6, -1e6, 2.0), (0.0, 1e6, 2.0)], [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]], [(0.0, -1.0, 0.0), (3.0e38, 3.0e38, 3.0e38)], 0.0, np.inf)
    q = np.concatenate([q, wide]).astype(F)
    r = R.Renderer((64, 64), tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(two.primitives)
    r.prepare_first_frame()
    both = ns.brute_force(T, q)
    assert {0, 1} <= set(np.unique(both[1][:, 0]).tolist())
    _same(_ask(r, torch, q), both, "both")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 0) == 0 and not r.needs_build()
    want = ns.brute_force(ns.world_triangles(two.primitives, disabled=(1,)), q)
    assert not (want[1][:, 0] == 1).any() and not np.array_equal(want[1], both[1])
    _same(_ask(r, torch, q), want, "one disabled")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 1) == 0
    _same(_ask(r, torch, q), both, "enabled again")
    assert r.stats()["rebuilds"] == 0
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["presets", "one-version"])
def test_trees_a_refit_wrote(R, torch, get_scene, form):
    """Cornell with its last primitive as a model of its own on a dynamic scene that never rebuilds: after a matrix move, after art_scene_set_vertices, after
    art_scene_set_vertices_device, after the primitive is disabled and after it is enabled again a batch on one side stream with no synchronisation in between: each is
    the reference over a model built from scratch of the world vertices as of its call"""
    sc = get_scene("cornell")
    q = _scene_ref(get_scene, "cornell", 1.0)["q"][1024:3072]
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
    m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
    verts = np.array(moving.verts, np.float32)
    verts[:, 0:3] = verts[:, 0:3] * np.float32(0.75) + np.array([0.0, 0.05, 0.0], np.float32)
    verts2 = np.array(verts, np.float32)
    verts2[:, 0:3] = verts2[:, 0:3] * np.float32(0.5) + np.array([0.125, 0.0, 0.0], np.float32)
    moved, deformed, again = static + [P(moving.verts, moving.indices, moving.tex, m)], static + [P(verts, moving.indices, moving.tex, m)], static + [P(verts2, moving.indices, moving.tex, m)]
    states = [("moved", moved, ()), ("deformed", deformed, ()), ("deformed on the device", again, ()), ("disabled", again, (len(static),)), ("enabled", again, ())]
    r = R.Renderer((64, 64), dynamic_scene=True, tuning=dict({"refit_rebuild_ratio": -1.0}, **tqf.REFITS[form]))
    r.add_model(static)
    r.add_model([moving])
    r.prepare_first_frame()
    model = r.models_mut()[1]
    pid = model.primitive_ids[0]
    d_q, d_v = _up(torch, q), _up(torch, verts2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for what, _, _ in states:
        if what == "moved": model.set_model_matrix(m)
        elif what == "deformed": model.set_vertices(0, verts)
        elif what == "deformed on the device": model.set_vertices_device(0, d_v, stream=s)
        elif what == "disabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 0) == 0
        elif what == "enabled": assert r._L.art_scene_set_primitive_enabled(r._ctx, pid, 1) == 0
        assert not r.needs_build()
        with torch.cuda.stream(s):
            outs.append(r.cast_triangles(d_q))
    s.synchronize()
    wants = [ns.brute_force(ns.world_triangles(prims, disabled=off), q) for _, prims, off in states]
    for (what, _, _), got, want in zip(states, outs, wants):
        _same(_host(got), want, f"{form}, {what}")
    assert not np.array_equal(wants[0][0], wants[1][0]) and not np.array_equal(wants[1][0], wants[2][0]) and not (wants[3][1][:, 0] == len(static)).any()
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 4 and r.cast_counts()["casts"] == len(states), st
    r.close()


@pytest.mark.gpu
def test_thirty_three_calls_in_flight_and_a_resolve_behind_a_cast(R, torch, get_scene):
    """33 calls on one side stream with nothing synchronised before the end -- one more than the ring of ART_CAST_POOL cursor blocks holds, so the last waits for the
    first -- each followed, with nothing in between, by art_resolve_hits of its records on the same stream: every result is the reference, every resolve that of the
    reference's records, and art_cast_counts counts 33 casts and their rays"""
    from araytracingjourney_amd import _lib
    calls = _lib.ART_CAST_POOL + 1 if _lib.ART_CAST_POOL >= 32 else 33
    assert calls >= 33
    ref, n = _scene_ref(get_scene, "cornell", 1.0), 1024
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_q = _up(torch, ref["q"][:n])
    want = _cut(ref["want"], n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(s):
        for _ in range(calls):
            got = r.cast_triangles(d_q)
            outs.append((got, r.resolve_hits(got[0], got[1], ("pos", "ng"))))
    counts = r.cast_counts()
    s.synchronize()
    res = r.resolve_hits(_up(torch, want[0]), _up(torch, want[1]), ("pos", "ng"))
    torch.cuda.synchronize()
    for i, (got, surf) in enumerate(outs):
        _same(_host(got), want, f"call {i}")
        for k in ("pos", "ng"):
            assert torch.equal(surf[k].view(torch.int32), res[k].view(torch.int32)), f"call {i}: the resolve's {k}"
    hit = want[1][:, 0] >= 0
    assert hit.sum() > 100 and (res["pos"][torch.from_numpy(hit).cuda(), 3] == 1).all()
    assert counts["casts"] == calls and counts["rays"] == calls * n, counts
    r.close()


@pytest.mark.gpu
def test_the_contexts_own_stream_and_optional_points(R, torch, get_scene):
    """hip_stream NULL -- the descriptor by hand, the wrapper cannot say it -- is the context's cast stream, and art_cast_sync is the fence; point_dev and qpoint_dev left
    out are not written: Cornell's first 1027 queries"""
    from araytracingjourney_amd import _lib
    ref, n = _scene_ref(get_scene, "cornell", 1.0), 1027
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_q = _up(torch, ref["q"][:n])
    tuv, ids, point, qpoint = outs = _patterned(torch, n + 2)
    torch.cuda.synchronize()
    d = _lib.ArtTriCast(sweeps_dev=d_q.data_ptr(), tuv_dev=tuv.data_ptr(), ids_dev=ids.data_ptr(), n=n, cull_mask=0xFF)
    assert r._L.art_cast_triangles(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    assert (point.view(torch.int32) == PATTERN).all() and (qpoint.view(torch.int32) == PATTERN).all() and _untouched(outs, n)
    d.point_dev, d.qpoint_dev = point.data_ptr(), qpoint.data_ptr()
    assert r._L.art_cast_triangles(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    assert _untouched(outs, n)
    _same(_host(tuple(t[:n] for t in outs)), _cut(ref["want"], n), "the context's stream")
    assert r.cast_counts() == dict(casts=2, rays=2 * n, host_waits=0)
    r.close()


def _box_mesh(lo, hi):
    """the twelve triangles of the box [lo, hi]: (positions [8, 3], indices [12, 3])"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    pos = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], F)
    idx = np.array([(0, 1, 2), (0, 2, 3), (4, 6, 5), (4, 7, 6), (0, 4, 5), (0, 5, 1), (3, 2, 6), (3, 6, 7), (0, 3, 7), (0, 7, 4), (1, 5, 6), (1, 6, 2)], np.int64)
    return pos, idx


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", ["none", "translation"])
def test_sweep_mesh_drops_a_box_onto_the_floor(R, torch, get_scene, matrix):
    """a box of twelve triangles over a clear corner of Cornell's floor, dropped by twice its height above the floor: it stops at t = 0.5, the analytic height over the
    displacement, within the CPU bound of the random set; the records are cast_triangles of the buffer numpy gathers with the same operations, and `first` is their
    reduction -- the smallest t, the lowest index among equals -- as it stands and through a translation whose sums are exact; a box swept away from everything has no
    answer: index -1 and the miss record"""
    ref = _scene_ref(get_scene, "cornell", 1.0)
    T = ref["T"]
    lo, hi = tto.scene_bounds(T)
    c, h = 0.5 * (lo + hi).astype(np.float64), 0.5 * (hi - lo).astype(np.float64)
    floor = float(lo[1])
    mm = None if matrix == "none" else [1, 0, 0, 0.0, 0, 1, 0, 0.125, 0, 0, 1, 0.0]
    lift = 0.0 if mm is None else 0.125
    blo = np.array([c[0] + 0.75 * h[0], floor + 0.5 * h[1] - lift, c[2] - 0.95 * h[2]]).astype(F)
    bhi = np.array([c[0] + 0.95 * h[0], floor + 0.8 * h[1] - lift, c[2] - 0.75 * h[2]]).astype(F)
    pos, idx = _box_mesh(blo, bhi)
    height = (float(blo[1]) + lift) - floor
    drop = (0.0, -2.0 * height, 0.0)
    world = pos + np.array([0.0, lift, 0.0], F)                    # (the matrix's one sum a coordinate, exact or not: the same operation)
    q = _limits(ns.sweeps_of(world[idx], drop), [0.0], [1.0])
    want = ns.brute_force(T, q)
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    records, first = r.sweep_mesh(_up(torch, pos), _up(torch, idx), drop, mm)
    torch.cuda.synchronize()
    _same(_host(records), want, f"sweep_mesh, {matrix}")
    has = want[1][:, 0] >= 0
    at = int(np.flatnonzero(has & (want[0][:, 0] == want[0][has, 0].min()))[0])
    t = float(first["t"])
    print(f"\n[tri cast] sweep_mesh, {matrix}: t {t!r} for 0.5; triangles with an answer {int(has.sum())}")
    assert abs(t - 0.5) <= _bounds()["random"] * 1.0                                                       # max(1, tmax - tmin) = 1
    assert int(first["index"]) == at and _bits(first["t"].cpu().numpy()) == _bits(want[0][at, 0]) and np.array_equal(first["ids"].cpu().numpy(), want[1][at])
    assert np.array_equal(_bits(first["point"].cpu().numpy()), _bits(want[2][at])) and np.array_equal(_bits(first["qpoint"].cpu().numpy()), _bits(want[3][at]))
    assert abs(float(first["point"][1]) - floor) <= 1e-6 and abs(float(first["qpoint"][1]) + t * drop[1] - floor) <= 1e-5
    records, first = r.sweep_mesh(_up(torch, pos), _up(torch, idx), (0.0, 0.0, -1.0), [1, 0, 0, 0.0, 0, 1, 0, 0.0, 0, 0, 1, -64.0], tmax=2.0)
    nothing = r.sweep_mesh(_up(torch, pos), _up(torch, idx[:0]), drop, mm, tmax=3.0)
    assert int(first["index"]) == -1 and float(first["t"]) == 2.0 and (first["ids"] == -1).all() and not first["point"].any() and (records[1] == -1).all()
    assert nothing[0][0].shape == (0, 4) and int(nothing[1]["index"]) == -1 and float(nothing[1]["t"]) == 3.0
    for args in ((_up(torch, pos).cpu(), _up(torch, idx), drop), (_up(torch, pos), _up(torch, idx), (0.0, 1.0)), (_up(torch, pos), _up(torch, idx), (0.0, np.nan, 0.0)),
                 (_up(torch, pos), _up(torch, idx), drop, [1.0] * 11), (_up(torch, pos), _up(torch, idx), drop, None, 0.0, float("nan")), (_up(torch, pos), _up(torch, idx), drop, None, 0.0, 1.0, 0x100)):
        with pytest.raises((ValueError, TypeError)):
            r.sweep_mesh(*args)
    r.close()


@pytest.mark.gpu
def test_errors_change_nothing_and_enqueue_nothing(R, torch, get_scene):
    """every ART_E_INVALID case of include/art.h with its literal message, and ART_E_STATE before the build and while the scene needs one: pattern-filled outputs
    untouched and the counts unchanged; the wrapper raises ValueError before the call"""
    from araytracingjourney_amd import _lib
    sc = get_scene("cornell")
    r = R.Renderer((64, 64))
    r.add_model(sc.primitives)
    L, ctx = r._L, r._ctx
    n = 64
    sweeps = _up(torch, _scene_ref(get_scene, "cornell", 1.0)["q"][:n + 1])
    tuv, ids, point, qpoint = outs = _patterned(torch, n + 1)
    torch.cuda.synchronize()

    def desc(**kw):
        d = dict(sweeps_dev=sweeps.data_ptr(), tuv_dev=tuv.data_ptr(), ids_dev=ids.data_ptr(), point_dev=point.data_ptr(), qpoint_dev=qpoint.data_ptr(), hip_stream=None, n=n,
                 cull_mask=0xFF, flags=0, reserved=0)
        d.update(kw)
        return _lib.ArtTriCast(**d)

    def said(d):
        code = L.art_cast_triangles(ctx, C.byref(d) if d is not None else None)
        return code, L.art_last_error()

    clean = lambda: _untouched(outs, 0)   # noqa: E731
    state = WHO + b"scene not built, or changed since the build (art_scene_build)"
    assert said(desc()) == (_lib.ART_E_STATE, state)
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert L.art_cast_triangles(None, C.byref(desc())) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    assert said(None) == (_lib.ART_E_INVALID, WHO + b"null argument")
    bad = [(desc(flags=1), b"flags: must be 0"), (desc(flags=0x80000000), b"flags: must be 0"), (desc(reserved=1), b"reserved: must be 0"),
           (desc(cull_mask=0x100), b"cull_mask: above 0xFF"), (desc(cull_mask=0xFFFFFFFF), b"cull_mask: above 0xFF"),
           (desc(n=_lib.ART_CAST_MAX_RAYS + 1), b"n: above ART_CAST_MAX_RAYS"), (desc(n=0xFFFFFFFF), b"n: above ART_CAST_MAX_RAYS"),
           (desc(sweeps_dev=None), b"sweeps_dev: null or not 16-byte aligned"), (desc(sweeps_dev=sweeps.data_ptr() + 8), b"sweeps_dev: null or not 16-byte aligned"),
           (desc(tuv_dev=None), b"tuv_dev: null or not 16-byte aligned"), (desc(tuv_dev=tuv.data_ptr() + 4), b"tuv_dev: null or not 16-byte aligned"),
           (desc(ids_dev=None), b"ids_dev: null or not 8-byte aligned"), (desc(ids_dev=ids.data_ptr() + 4), b"ids_dev: null or not 8-byte aligned"),
           (desc(point_dev=point.data_ptr() + 8), b"point_dev: not 16-byte aligned"), (desc(qpoint_dev=qpoint.data_ptr() + 8), b"qpoint_dev: not 16-byte aligned")]
    for d, text in bad:
        assert said(d) == (_lib.ART_E_INVALID, WHO + text), text
    r.cast_sync()
    torch.cuda.synchronize()
    assert r.cast_counts() == zero and clean()
    assert said(desc(n=0))[0] == 0 and said(desc(n=0, sweeps_dev=None, tuv_dev=None, ids_dev=None, point_dev=None, qpoint_dev=None))[0] == 0
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    # the wrapper's own checks: before anything is enqueued
    for args, kw in (((sweeps.cpu(),), {}), ((sweeps.double(),), {}), ((sweeps[:, :12],), {}), ((sweeps,), dict(cull_mask=0x100)), ((sweeps,), dict(out=(tuv[:8], ids, point, qpoint))),
                     ((sweeps,), dict(out=(tuv, ids.to(torch.int64), point, qpoint))), ((sweeps,), dict(out=(tuv, ids, point))), ((sweeps,), dict(out=(tuv, ids, point, qpoint[:, :3])))):
        with pytest.raises((ValueError, TypeError)):
            r.cast_triangles(*args, **kw)
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    assert said(desc())[0] == 0
    r.cast_sync()
    assert _untouched(outs, n) and not (ids[:n] == PATTERN).any() and r.cast_counts() == dict(casts=1, rays=n, host_waits=0)
    r.add_model([sc.primitives[0]])   # a primitive added since the build: art_scene_needs_build
    assert r.needs_build() and said(desc()) == (_lib.ART_E_STATE, state)
    with pytest.raises(_lib.ArtError):
        r.cast_triangles(sweeps)
    r.close()
