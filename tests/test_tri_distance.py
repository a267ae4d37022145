"""art_closest_triangles (include/art.h): the distance from each of a buffer of query triangles to the scene, and where -- defined exactly and checked
bit for bit.

The reference is tests/np_tri_distance.py: the fifteen features, the overlap rule, box_d2 and the argmin of (d2_eff, gid) in numpy float32, operation by operation, on
np_closest.world_triangles' fields; tri_closest and the 17 axes are np_closest's and np_tri_overlap's functions, imported.  Nothing on the device has a tolerance: the
words of d, u, v, the ids and both points.  A reference is computed once per set of inputs, shared and never written.

The CPU tests tie the reference to an independent float64 witness (np_tri_distance.witness: Voronoi regions for vertex against triangle, a float64 segment pair, and
test_tri_overlap's witness for "they share a point").  Distances are compared, never ids.  The bound is on |d32 - d64| / M, M the largest coordinate magnitude of the
set; it is four times the worst figure measured on the set, rounded up to one digit (BOUNDS below; the worst case is a tail event that another seed moves by that much):
    random pairs (200 000, M 11.7)                       worst 1.04e-7, p99.9 6.9e-8     bound 5e-7
    the same offset by 100 units (200 000, M 112)        worst 1.03e-7, p99.9 7.6e-8     bound 5e-7
    nearly parallel edges (200 000, M 1.29)              worst 1.91e-6, p99.9 1.16e-7    bound 8e-6
    Cornell's 4096 queries at r = +inf (M 0.88)          worst 4.8e-8,  p99.9 3.4e-8     bound 2e-7
(d64 - d32) / M, the undercut, is at most 1.04e-7, 1.03e-7, 1.9e-7 and 4.0e-8 on the four.  The segment formula alone, prototyped in numpy when the query was
proposed, had a worst case of 6.3e-5 on nearly parallel edges; among the fifteen features the six vertex features find the same minimum for parallel edges (it
is attained at an end point), and what is left of the tail is 1.91e-6.
The nearly parallel set's tail is the vanishing denominator a*e - b*b of the segment formula; it errs upwards only (the witnesses are always points of the two
triangles), which test_the_model_never_undercuts_the_witness asserts for every pair of every set against the random set's bound.
What wins in the references the device is compared with (misses / d = 0 by the overlap rule / won by a query vertex, a scene vertex, an edge pair):
    Cornell 1.0 (4096 queries, 34 triangles)         1 453 / 1 640 /   559,   238,   206      ties on d2_eff: 1 667
    sponza_like 0.05 (4096, 7 144)                     870 / 1 752 /   865,   101,   508                      1 827
    the lattice (2071, 576)                              1 /     0 / 2 070,     0,     0                      2 070   (every d is 0 by a vertex in a face: the axes are not asked)
    the clump (256, 1000)                               48 /    98 /    28,    39,    43                        130
    the chain (130, 64)                                  0 /    57 /     1,     0,    72                        128
    the soup (1024, 600)                               279 /    86 /   136,   112,   411                        351
    the specials on sponza_like (418, 7 144)            69 /   135 /   187,     1,    26                        298
A point query (q0 = q1 = q2) against np_closest: of Cornell's 4096, the soup's 1024 and the chain's 130, d differs in one of Cornell's (by 1.4e-7 relative) and the ids
in 28 -- the scene-vertex feature measures |v_k - p|^2 directly, which can round below tri_closest's value for the same vertex and so choose another of the triangles
that share it; wherever a query-vertex feature wins (2 115, 603 and 79 queries) d and the ids are np_closest's bit for bit.
Mutation checks, on scratch builds of the library run over the 44 GPU tests of this module (profiles/tri_distance_mutants.txt has pytest's lines):
  * the strict `>` of the node skip made `>=` (a child whose box is exactly at the limit is dropped, and with it the smaller gid among ties): 41 tests fail -- both
    scenes, all five hostile sets, every tree form, every knob, the sizes, the masks, the refits, the ring, the context's stream, mesh_clearance without a matrix.  The
    errors and mesh_clearance through the translation and the scale pass.
  * TravPoint::pop skipping spilled entries: 42 tests fail (Cornell's ids of 29 of 4 096 queries, the r = +inf ones, whose ties at 0 keep every box at distance 0 in
    play and fill the eight LDS pairs; sponza_like's of 442; the lattice's of 381 of 2 071); the errors and mesh_clearance through the translation pass.
  * the edge pairs dropped from the leaf: 42 tests fail; the lattice (where a vertex in a face finds every 0) and the errors pass.
  * the gid tie rule dropped (a tie is taken only by the first candidate): 41 tests fail; the errors and mesh_clearance through the translation and the scale pass.
"""
import ctypes as C
import os
import subprocess
import warnings

import numpy as np
import pytest

import np_closest as nc
import np_tri_distance as nd
import np_tri_overlap as nto
import test_closest_points as tcp
import test_query_forms as tqf
import test_tri_overlap as tto
from helpers import chain_scene, degenerate_soup, lattice_scene
from helpers import _layout_is_the_headers, _host, R, torch, _up, _bits  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = tto.PATTERN
N = tto.N
WHO = b"art_closest_triangles: "
F = np.float32
COORDS = tto.COORDS
INF = F(np.inf)

_REF = {}


# ---- inputs and references ---------------------------------------------------------------------------------------------------------------------------------------
def with_radii(q, ext, seed, every=16):
    """the radius into word 3: 0.3 % .. 3 % of the extent, log-uniform, and +inf for one query in `every` (the brute force over every triangle stays a matter of seconds)"""
    rng = np.random.default_rng(seed)
    q = np.array(q, F)
    q[:, 3] = (ext * 10.0 ** rng.uniform(-2.5, -1.5, q.shape[0])).astype(F)
    q[::every, 3] = np.inf
    return q


def scene_queries(T, seed):
    """test_tri_overlap.scene_queries' two populations (random triangles, the scene's own moved a little) with the radius written into word 3"""
    lo, hi = tto.scene_bounds(T)
    return with_radii(tto.scene_queries(T, seed), float((hi - lo).max()), seed + 1)


def _ref(key, make):
    """{scene, T, q, want, stats} of a set of inputs: make() -> (scene, queries); computed once, shared, never written"""
    if key not in _REF:
        sc, q = make()
        T = nd.world_triangles(sc.primitives)
        q = np.ascontiguousarray(q, F)
        q.setflags(write=False)
        *want, stats = nd.brute_force(T, q, stats=True)
        _REF[key] = dict(scene=sc, T=T, q=q, want=tto._frozen(tuple(want)), stats=tto._frozen(stats))
    return _REF[key]


def _scene_ref(get_scene, name, detail):
    def make():
        sc = get_scene(name, detail)
        return sc, scene_queries(nd.world_triangles(sc.primitives), 13)
    return _ref((name, detail), make)


def _cycle_radii(q, radii):
    q = np.array(q, F)
    q[:, 3] = np.resize(np.asarray(radii, F), q.shape[0])
    return q


def dead_queries():
    """test_tri_overlap's 27 (a NaN, +inf, -inf in each coordinate) at r = 1, then a live triangle with r NaN, -1, -inf and -1e-30: miss records that carry r as given"""
    a = tto.dead_queries()
    a[:, 3] = 1.0
    b = np.tile(tto._tri((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5)), (4, 1))
    b[:, 3] = (np.nan, -1.0, -np.inf, -1e-30)
    return np.concatenate([a, b]).astype(F)


def special_queries(T):
    """test_tri_overlap.special_queries on sponza_like -- [0] larger than the scene with r = +inf (the whole-scene query), [1] reaching 3e37, [2] far away with r = +inf;
    scene triangles handed back, points, segments, turned copies -- with r cycling through 0, -0.0, 0.5 % of the extent and +inf (one in eight); then the dead queries"""
    lo, hi = tto.scene_bounds(T)
    q = tto.special_queries(T)[:-27]
    q = _cycle_radii(q, [0.0, -0.0, 0.005 * float((hi - lo).max()), 0.0, 0.02, np.inf, 0.001, 0.05])
    q[0:3, 3] = (np.inf, 1.0, np.inf)
    return np.concatenate([q, dead_queries()]).astype(F)


def inside_box_queries():
    """triangles in the air inside Cornell's closed room: d > 0 and nothing is cut"""
    q = np.tile(tto.INSIDE_CORNELL, (3, 1))
    q[1, COORDS] += F(0.02)
    q[:, 3] = (np.inf, 1.0, 0.05)   # the nearest surface is 0.077 away: the third is a miss
    return q.astype(F)


HOSTILE = ["lattice", "clump", "chain", "soup", "specials"]


def _hostile(get_scene, which):
    if which == "lattice":   # every coordinate a multiple of 0.25: the distances are exact, and ties come by the dozen (the gid rule); coplanar faces
        return _ref(which, lambda: (lattice_scene(6), _cycle_radii(tto.lattice_queries(), [0.25, np.inf, 0.0, 0.5, 0.375, 1.0, -0.0])))
    if which == "clump":     # 1000 triangles in one place: the stack past its eight LDS pairs
        return _ref(which, lambda: (degenerate_soup(1000, "one point"), _cycle_radii(tto.clump_queries(), [np.inf, 0.01, 0.1, 0.0, 1.0])))
    if which == "chain":
        return _ref(which, lambda: (chain_scene(64)[0], _cycle_radii(tto.chain_queries(), [np.inf, 0.001, 0.25, 0.0])))
    if which == "soup":
        def make():
            sc = degenerate_soup(600, "soup")
            return sc, scene_queries(nd.world_triangles(sc.primitives), 5)[::4]
        return _ref(which, make)
    sc = get_scene("sponza_like", 0.05)
    return _ref(which, lambda: (sc, special_queries(nd.world_triangles(sc.primitives))))


CASES = ["cornell", "sponza_like"] + HOSTILE


def _case(get_scene, name):
    return _scene_ref(get_scene, name, 0.05 if name == "sponza_like" else 1.0) if name in ("cornell", "sponza_like") else _hostile(get_scene, name)


def _same(got, want, what=""):
    """ids, the bits of d, u, v, a fourth word of 0, the bits of both points"""
    (duv, ids, point, qpoint), (rduv, rids, rpoint, rqpoint) = got, want
    assert duv.shape == rduv.shape and ids.shape == rids.shape and point.shape == rpoint.shape and qpoint.shape == rqpoint.shape, what
    bad = (ids != rids).any(axis=1)
    assert not bad.any(), f"{what}: the ids of {int(bad.sum())} of {ids.shape[0]} queries differ (first: {np.flatnonzero(bad)[:5]}: {ids[bad][:2]} for {rids[bad][:2]}, d {duv[bad][:2, 0]} for {rduv[bad][:2, 0]})"
    bad = (_bits(duv)[:, :3] != _bits(rduv)[:, :3]).any(axis=1)
    assert not bad.any(), f"{what}: d, u, v of {int(bad.sum())} queries differ (first: {np.flatnonzero(bad)[:5]}: {duv[bad][:2]} for {rduv[bad][:2]})"
    assert not _bits(duv)[:, 3].any(), f"{what}: the fourth word is not 0"
    assert np.array_equal(_bits(point), _bits(rpoint)), f"{what}: the scene points differ"
    bad = (_bits(qpoint) != _bits(rqpoint)).any(axis=1)
    assert not bad.any(), f"{what}: the query points of {int(bad.sum())} queries differ (first: {np.flatnonzero(bad)[:5]}: {qpoint[bad][:2]} for {rqpoint[bad][:2]})"


def _cut(want, n=None, at=None):
    return tuple(w[:n] if at is None else w[at] for w in want)


def _ask(r, torch, q, **kw):
    got = r.closest_triangles(_up(torch, q), **kw)
    torch.cuda.synchronize()
    return _host(got)


class _no_sync:
    """torch raises inside this block where an operation makes the host wait for the device (a 0-dim tensor read back as an index, a pageable copy)"""
    def __init__(self, torch):
        self.torch = torch

    def __enter__(self):
        self.was = self.torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # (torch calls the mode a prototype that does not see every wait; it sees a read-back and a pageable copy)
            self.torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.torch.cuda.set_sync_debug_mode(self.was)
        return False


def _patterned(torch, n):
    return (torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((n, 2), PATTERN, dtype=torch.int32, device="cuda"),
            torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32))


def _untouched(outs, n):
    return all((t[n:].view(outs[1].dtype) == PATTERN).all() for t in outs)


def _ask_into(r, torch, q, extra, what, stream=None, **kw):
    """into tensors `extra` records too long and filled with a pattern: the tail keeps it"""
    n = q.shape[0]
    outs = _patterned(torch, n + extra)
    d_q = _up(torch, np.asarray(q).reshape(n, 12))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        got = r.closest_triangles(d_q, out=outs, **kw)
        assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert _untouched(outs, n), f"{what}: written beyond n"
    return _host(tuple(t[:n] for t in outs))


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_ctypes_descriptor_is_the_headers():
    """ArtTriDistance as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 64 bytes"""
    _layout_is_the_headers("ArtTriDistance", 64, ["tris_dev", "duv_dev", "ids_dev", "point_dev", "qpoint_dev", "hip_stream", "n", "cull_mask", "flags", "reserved"])


def test_presence():
    """art_closest_triangles(NULL, NULL) is ART_E_INVALID with the prefixed message on any machine; the library exports it, the Rust binding declares the function and the
    struct, the header cites DESIGN.md 3.14 and names FCL's and PhysX's calls, the C++ mirror has the call, and Renderer has both methods"""
    from araytracingjourney_amd import _lib, renderer
    L = _lib.load()
    assert L.art_closest_triangles(None, None) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    d = _lib.ArtTriDistance(flags=1)
    nowhere = C.create_string_buffer(1 << 16)
    assert L.art_closest_triangles(nowhere, C.byref(d)) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"flags: must be 0"
    so = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "art_closest_triangles" for line in syms.splitlines() if line.strip())
    rs = open(os.path.join(ROOT, "bindings", "art_sys.rs")).read()
    assert "pub fn art_closest_triangles(" in rs and "pub struct ArtTriDistance" in rs
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "DESIGN.md 3.14" in hdr and "computeDistance" in hdr and "FCL's distance" in hdr and "### 3.14" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "art_closest_triangles(" in open(os.path.join(ROOT, "araytracingjourney_amd", "host", "art_renderer.hpp")).read()
    assert callable(renderer.Renderer.closest_triangles) and callable(renderer.Renderer.mesh_clearance)


def _one(tri, query, r=np.inf, mutate=None):
    """one scene triangle, one query: (d, u, v, hit, point, qpoint, group)"""
    w = np.asarray(tri, F).reshape(1, 3, 3)
    T = dict(w=w, v0=w[:, 0].copy(), e1=w[:, 1] - w[:, 0], e2=w[:, 2] - w[:, 0], lo=w.min(axis=1), hi=w.max(axis=1), prim=np.zeros(1, np.int32), tri=np.zeros(1, np.int32))
    q = tto._tris(np.asarray(query, F).reshape(1, 3, 3))
    q[:, 3] = r
    duv, ids, point, qpoint, st = nd.brute_force(T, q, stats=True, mutate=mutate)
    return float(duv[0, 0]), float(duv[0, 1]), float(duv[0, 2]), bool(ids[0, 0] == 0), point[0, :3].tolist(), qpoint[0, :3].tolist(), int(st["group"][0])


def _dh(x):
    return x[0], x[3]   # (d, hit)


def test_known_answers():
    """the triangle (0,0,0) (1,0,0) (0,1,0), every coordinate exact: a query above the face (a query vertex wins), a big query under a scene vertex (a scene vertex
    wins), two crossing edges that are close where no vertex of either is (an edge pair wins, and neither vertex group finds it), a cutting pair (0, and the witnesses
    are not a point of the intersection), coplanar apart, the radius closed at d == r, misses, points, segments and a zero-area scene triangle"""
    t = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    d, u, v, hit, p, qp, g = _one(t, [(0.25, 0.25, 0.5), (0.5, 0.25, 1), (0.25, 0.5, 1)])
    assert (d, u, v, hit, p, qp, g) == (0.5, 0.25, 0.25, True, [0.25, 0.25, 0.0], [0.25, 0.25, 0.5], 0)
    d, u, v, hit, p, qp, g = _one(t, [(-4, -4, -0.25), (8, -4, -0.25), (-4, 8, -0.25)])
    assert (d, hit, p, qp, g) == (0.25, True, [0.0, 0.0, 0.0], [0.0, 0.0, -0.25], 1)
    cross = [(0.5, -1, 0.25), (0.5, 1, 0.25), (0.5, 0, 8)]                                     # its first edge crosses above the edge v0 v1 at (0.5, 0, 0.25)
    d, u, v, hit, p, qp, g = _one(t, cross)
    assert (d, u, v, hit, p, qp, g) == (0.25, 0.5, 0.0, True, [0.5, 0.0, 0.0], [0.5, 0.0, 0.25], 2)
    skew = [(0.25, -1, 0.125), (0.75, 1, 0.125), (0.5, 0, 8)]                                  # no vertex is near: only the edge pair finds 0.125
    d, u, v, hit, p, qp, g = _one([(0, 0, 0), (1, 0, 0), (0.5, -4, -4)], skew)
    assert g == 2 and d == 0.125 and p == [0.5, 0.0, 0.0] and qp == [0.5, 0.0, 0.125]
    assert _one([(0, 0, 0), (1, 0, 0), (0.5, -4, -4)], skew, mutate="no edge pairs")[0] > 0.125
    d, u, v, hit, p, qp, g = _one(t, [(0.2, 0.2, -1), (0.2, 0.2, 1), (0.3, 0.9, 1)])           # an edge of the query pierces the face
    assert d == 0.0 and hit and p != qp                                                          # the clearance is 0; the witnesses are the nearest features'
    assert _one(t, [(0.2, 0.2, -1), (0.2, 0.2, 1), (0.3, 0.9, 1)], mutate="no overlap rule")[0] > 0.0
    assert _one(t, [(0.75, 0.75, 0), (1.5, 0.75, 0), (0.75, 1.5, 0)])[0] == F(np.sqrt(F(0.125)))   # coplanar, beyond the hypotenuse
    assert _one(t, [(1, 0, 0), (2, 0, 1), (2, 1, -1)])[0] == 0.0                               # touching at one vertex
    par = [(0.1, 0.1, 0.5), (0.4, 0.1, 0.5), (0.1, 0.4, 0.5)]                                    # parallel planes, 0.5 apart: d2_eff == r * r is a candidate
    assert _dh(_one(t, par, r=0.5)) == (0.5, True) and _dh(_one(t, par, r=0.5, mutate="strict r")) == (0.5, False)
    assert _dh(_one(t, par, r=0.49)) == (float(F(0.49)), False) and _one(t, par, r=0.49)[4:6] == ([0.0] * 3, [0.0] * 3)
    assert _one(t, par, r=0.0)[3] is False and _dh(_one(t, [(0.25, 0.25, 0)] * 3, r=0.0)) == (0.0, True) and _one(t, [(0.25, 0.25, 0)] * 3, r=-0.0)[3]
    assert _one(t, [(0.25, 0.25, 2)] * 3)[0] == 2.0 and _one(t, [(3, 0, 0), (3, 0, 0), (5, 0, 0)])[0] == 2.0       # a point; a segment
    seg = [(0, 0, 0), (1, 0, 0), (0.5, 0, 0)]                                                    # a zero-area scene triangle: a segment
    assert _one(seg, [(0.5, 1, -1), (0.5, 2, -1), (0.5, 1, 2)])[0] == 1.0 and _one(seg, [(0.5, -1, -1), (0.5, 1, -1), (0.5, 0, 2)])[0] == 0.0
    assert _one(t, par, mutate="no scene vertices")[0] == 0.5                                    # (a query vertex finds this one too)
    assert _one(t, [(-4, -4, -0.25), (8, -4, -0.25), (-4, 8, -0.25)], mutate="no scene vertices")[6] == 2   # ... and here an edge pair steps in at the same distance


def test_a_non_finite_scene_triangle_is_never_returned():
    """DESIGN.md 3.14, step 1's last line: a scene triangle whose first vertex has a NaN, and one whose finite vertices lie 6e38 apart (e1 and e2 overflow to +inf), give no feature a
    number (one finite edge would: a segment pair reads nothing else); the 17 axes separate nothing of the first -- by the overlap rule alone its d2_tri would be 0 and the triangle the nearest of every query -- and d2_tri stays +inf:
    a miss at any radius, and beside a finite triangle that one answers"""
    query = [(0.25, 0.25, 0.5), (0.5, 0.25, 1), (0.25, 0.5, 1)]
    col = lambda x: [np.asarray([c], F) for c in x]   # noqa: E731
    with np.errstate(all="ignore"):
        for tri in ([(np.nan, 0, 0), (1, 0, 0), (0, 1, 0)], [(-3e38, 0, 0), (3e38, 0, 0), (3e38, 1, 0)]):
            w = np.asarray(tri, F)
            v0, e1, e2 = w[0], w[1] - w[0], w[2] - w[0]
            assert not np.isfinite(e1).all() and not np.isfinite(e2).all()
            d, u, v, s_, t_, grp, cut = nd.pair_d2(col(v0), col(e1), col(e2), col(query[0]), col(query[1]), col(query[2]))
            assert np.isposinf(d[0]) and grp[0] == -1 and not cut[0]
            if np.isnan(w).any():   # no axis with a NaN separates: the overlap rule alone would make it 0, the nearest of everything
                assert nto.tri_tri_overlap(col(v0), col(e1), col(e2), col(query[0]), col(query[1]), col(query[2]))[0]
            for r in (np.inf, 1.0, 0.0):
                got = _one(tri, query, r=r)
                assert not got[3] and got[4:6] == ([0.0] * 3, [0.0] * 3)
            both = np.concatenate([w[None], np.asarray([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], F)])
            T = dict(w=both, v0=both[:, 0].copy(), e1=both[:, 1] - both[:, 0], e2=both[:, 2] - both[:, 0], lo=both.min(axis=1), hi=both.max(axis=1), prim=np.zeros(2, np.int32), tri=np.arange(2, dtype=np.int32))
            q = tto._tris(np.asarray(query, F).reshape(1, 3, 3))
            q[:, 3] = np.inf
            duv, ids, point, qpoint = nd.brute_force(T, q)
            assert ids[0].tolist() == [0, 1] and duv[0, 0] == 0.5


def pair_sets():
    """{name: (scene triangles [P, 3, 3], query triangles [P, 3, 3])} float32, 200 000 pairs each: random pairs about the origin, the same offset by 100 units, and
    nearly parallel edges -- a copy of the triangle moved by 1e-3 .. 0.3 and perturbed by 1e-4"""
    out = {}
    for name, seed, offset in (("random", 1, 0.0), ("offset 100", 2, 100.0)):
        out[name] = tto.random_pairs(200_000, seed, offset)
    rng = np.random.default_rng(3)
    t = rng.uniform(-1.0, 1.0, (200_000, 3, 3))
    d = rng.normal(0.0, 1.0, (200_000, 1, 3))
    d *= (10.0 ** rng.uniform(-3.0, np.log10(0.3), (200_000, 1, 1))) / np.linalg.norm(d, axis=2, keepdims=True)
    out["nearly parallel"] = (t.astype(F), (t + d + rng.uniform(-1e-4, 1e-4, (200_000, 3, 3))).astype(F))
    return out


# |d32 - d64| / M per set: four times the worst measured, rounded up to one digit (the module's docstring has the measurements)
BOUNDS = {"random": 5e-7, "offset 100": 5e-7, "nearly parallel": 8e-6, "cornell": 2e-7}
_PAIRS = {}


def _pair_distances(name, mutate=None):
    """(d32 of the model, d64 of the witness, M) over the set's pairs"""
    if not _PAIRS:
        _PAIRS.update(pair_sets())
    t, q = _PAIRS[name]
    col = lambda x: [x[:, k] for k in range(3)]   # noqa: E731
    with np.errstate(all="ignore"):
        d2 = nd.pair_d2(col(t[:, 0]), col(t[:, 1] - t[:, 0]), col(t[:, 2] - t[:, 0]), col(q[:, 0]), col(q[:, 1]), col(q[:, 2]), mutate)[0]
    w = np.stack([t[:, 0], t[:, 0] + (t[:, 1] - t[:, 0]), t[:, 0] + (t[:, 2] - t[:, 0])], 1)   # the triangle the record describes
    key = (name, "witness")
    if key not in _PAIRS:
        _PAIRS[key] = nd.witness(w, q)
    return np.sqrt(d2.astype(np.float64)), _PAIRS[key], float(max(np.abs(t).max(), np.abs(q).max()))


def _cornell_distances(get_scene, mutate=None):
    """Cornell's 4096 queries at r = +inf: the model's distance against the smallest witness distance over all 34 triangles"""
    ref = _scene_ref(get_scene, "cornell", 1.0)
    T, q = ref["T"], np.array(ref["q"])
    q[:, 3] = np.inf
    d32 = nd.brute_force(T, q, mutate=mutate)[0][:, 0].astype(np.float64)
    key = ("cornell", "witness")
    if key not in _PAIRS:
        wq = q[:, COORDS].reshape(-1, 3, 3)
        _PAIRS[key] = np.min([nd.witness(np.broadcast_to(T["w"][g], wq.shape), wq) for g in range(T["w"].shape[0])], axis=0)
    return d32, _PAIRS[key], float(max(np.abs(T["w"]).max(), np.abs(q[:, COORDS]).max()))


def _distances(get_scene, name, mutate=None):
    return _cornell_distances(get_scene, mutate) if name == "cornell" else _pair_distances(name, mutate)


@pytest.mark.parametrize("name", list(BOUNDS))
def test_the_model_against_the_witness(get_scene, name):
    """|d32 - d64| / M over every pair of the set (no pair is left out) within the set's bound"""
    d32, d64, M = _distances(get_scene, name)
    err = np.abs(d32 - d64) / M
    print(f"\n[tri distance] {name}: {d32.size} pairs, M {M:.4g}; |d32 - d64| / M worst {err.max():.3g}, p99.9 {np.quantile(err, 0.999):.3g}; d64 = 0 on {int((d64 == 0).sum())}, d32 = 0 on {int((d32 == 0).sum())}")
    assert np.isfinite(d32).all() and err.max() <= BOUNDS[name]


@pytest.mark.parametrize("name", list(BOUNDS))
def test_the_model_never_undercuts_the_witness(get_scene, name):
    """d32 >= d64 minus the random set's bound on every pair of every set: the witnesses are points of the two triangles, so the formulas err upwards only"""
    d32, d64, M = _distances(get_scene, name)
    under = (d64 - d32) / M
    print(f"\n[tri distance] {name}: (d64 - d32) / M worst {under.max():.3g}")
    assert under.max() <= BOUNDS["random"]


@pytest.mark.parametrize("mutate,name", [("no edge pairs", "random"), ("no scene vertices", "random"), ("no overlap rule", "random"), ("no edge pairs", "cornell"), ("no overlap rule", "cornell")])
def test_the_witness_tells_mutated_models_apart(get_scene, mutate, name):
    """the model with the edge pairs dropped, with the scene-vertex features dropped, with the overlap rule dropped: each breaks the set's bound by a factor of a
    thousand and more ("strict r" has no distance to be wrong in: test_known_answers has its case, d2_eff == r * r)"""
    d32, d64, M = _distances(get_scene, name, mutate)
    err = np.abs(d32 - d64) / M
    print(f"\n[tri distance] {name}, {mutate}: worst {err.max():.3g}, beyond the bound on {int((err > BOUNDS[name]).sum())} of {err.size}")
    assert err.max() > 1000 * BOUNDS[name]


POINT_QUERY_DIFFERS = {"cornell": (1, 28), "soup": (0, 0), "chain": (0, 0)}   # queries whose d / whose ids are not np_closest's, as measured (the module's docstring)


@pytest.mark.parametrize("name", ["cornell", "soup", "chain"])
def test_a_point_query_is_closest_points(get_scene, name):
    """q0 = q1 = q2 = p, on the queries where the overlap rule does not answer (a point the 17 axes call touching has d = 0 here and the distance to the face there): hit
    and miss are np_closest's for (p, r); wherever a query-vertex feature wins, d and the ids are np_closest's record bit for bit; where a scene vertex or an edge pair
    wins -- |v_k - p|^2 measured directly, which may round below tri_closest's value for that vertex -- d is np_closest's within the random set's bound (the module's
    docstring has the counts)"""
    ref = _case(get_scene, name)
    T, q = ref["T"], np.array(ref["q"])
    q[:, 4:7], q[:, 8:11] = q[:, 0:3], q[:, 0:3]
    duv, ids, point, qpoint, st = nd.brute_force(T, q, stats=True)
    pduv, pids, ppoint = nc.brute_force(T, q[:, 0:4])
    free = ~st["cut"]
    first = free & (st["group"] == 0)
    assert free.sum() > 0.9 * q.shape[0] and first.sum() > 50
    assert np.array_equal(ids[free, 0] >= 0, pids[free, 0] >= 0)
    assert np.array_equal(_bits(duv[first, 0]), _bits(pduv[first, 0])) and np.array_equal(ids[first], pids[first])
    M = float(max(np.abs(T["w"]).max(), np.abs(q[:, 0:3]).max()))
    hit = free & (ids[:, 0] >= 0)
    print(f"\n[tri distance] {name}: a point query against np_closest: d differs on {int((_bits(duv[hit, 0]) != _bits(pduv[hit, 0])).sum())}, ids on {int((ids[hit] != pids[hit]).any(axis=1).sum())} of {int(hit.sum())}")
    assert (np.abs(duv[hit, 0].astype(np.float64) - pduv[hit, 0]) <= BOUNDS["random"] * M).all()
    d_cap, id_cap = POINT_QUERY_DIFFERS[name]   # as measured: the exception does not grow unnoticed
    assert int((_bits(duv[hit, 0]) != _bits(pduv[hit, 0])).sum()) <= d_cap and int((ids[hit] != pids[hit]).any(axis=1).sum()) <= id_cap
    assert np.array_equal(_bits(qpoint[ids[:, 0] >= 0, :3]), _bits(q[ids[:, 0] >= 0, 0:3]))   # s = t = 0, or g1 = g2 = 0: q0 itself


def test_a_scene_triangle_as_its_own_query_has_distance_zero(get_scene):
    for name in ("cornell", "soup"):
        ref = _case(get_scene, name)
        T = ref["T"]
        q = tto._tris(T["w"])
        q[:, 3] = np.resize(np.asarray([0.0, np.inf, -0.0, 1.0], F), q.shape[0])
        duv, ids, point, qpoint = nd.brute_force(T, q)
        assert (ids[:, 0] >= 0).all() and not duv[:, 0].any()


FLOORS = dict(cornell=(100, 100, 100, 20, 100), sponza_like=(100, 100, 100, 100, 100), lattice=(1, 0, 1000, 0, 0), clump=(1, 10, 10, 1, 10), chain=(0, 10, 1, 0, 10), soup=(50, 50, 50, 20, 50), specials=(50, 50, 5, 1, 1))


@pytest.mark.parametrize("name", CASES)
def test_the_comparisons_are_not_vacuous(get_scene, name):
    """from the reference alone: misses, d = 0 by the overlap rule, winners of each of the three feature groups -- a set on which no edge pair ever wins tests nothing of
    the new formula -- and ties on d2_eff, which the gid rule decides"""
    ref = _case(get_scene, name)
    duv, ids, point, qpoint = ref["want"]
    st, q = ref["stats"], ref["q"]
    miss = ids[:, 0] < 0
    won = [int(((st["group"] == g) & ~st["cut"]).sum()) for g in range(3)]
    counts = (int(miss.sum()), int(st["cut"].sum()), *won)
    print(f"\n[tri distance] {name}: {q.shape[0]} queries, {ref['T']['v0'].shape[0]} triangles, {st['pairs']} pairs evaluated; misses {counts[0]}, d = 0 by overlap {counts[1]}, "
          f"won by a query vertex {won[0]}, a scene vertex {won[1]}, an edge pair {won[2]}; queries with a tie on d2_eff {int((st['ties'] > 1).sum())}, r = inf {int(np.isinf(q[:, 3]).sum())}")
    assert all(c >= f for c, f in zip(counts, FLOORS[name])), (counts, FLOORS[name])
    assert (duv[miss, 1:] == 0).all() and np.array_equal(_bits(duv[miss, 0]), _bits(q[miss, 3])) and not point[miss].any() and not qpoint[miss].any()
    assert (point[~miss, 3] == 1).all() and (qpoint[~miss, 3] == 1).all() and (duv[st["cut"], 0] == 0).all()
    with np.errstate(invalid="ignore"):
        assert (duv[~miss, 0] <= q[~miss, 3]).all()
    if name in ("cornell", "sponza_like"):
        assert q.shape[0] == N and int(np.isinf(q[:, 3]).sum()) == N // 16
    if name == "lattice":
        assert int((st["ties"] > 4).sum()) > 100
    if name == "specials":
        assert ids[0, 0] >= 0 and duv[0, 0] == 0 and ids[2, 0] >= 0 and duv[2, 0] > 0 and miss[-31:].all() and np.isnan(duv[-4, 0]) and duv[-3, 0] == -1.0


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_both_scenes_are_the_brute_forces(R, torch, get_scene, name, detail):
    """4096 queries on a side stream: d, u, v, ids and both points; a permutation of the queries gives the permuted records; oversized out= tensors filled with a
    pattern are untouched beyond n; triangles inside Cornell's closed room have d > 0; the queries count neither as casts nor as rays"""
    ref = _scene_ref(get_scene, name, detail)
    q = ref["q"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    _same(_ask_into(r, torch, q, 70, name, stream=torch.cuda.Stream()), ref["want"], name)
    _same(_ask(r, torch, q[perm]), _cut(ref["want"], at=perm), f"{name}, permuted")
    if name == "cornell":
        inside = inside_box_queries()
        want = nd.brute_force(ref["T"], inside)
        assert (want[0][:2, 0] > 0).all() and (want[1][:2, 0] >= 0).all() and want[1][2, 0] == -1
        _same(_ask(r, torch, inside), want, "inside the room")
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_inputs(R, torch, get_scene, which):
    """the lattice (exact distances, ties by the dozen, coplanar faces), 1000 triangles round one point (stacks past their LDS part), the chain of 64 nested slivers, a
    soup with duplicated triangles, and on sponza_like the whole-scene query at r = +inf, scene triangles handed back, points, segments, r = 0, -0.0 and +inf, and
    the dead queries of each kind"""
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
    dead_want = nd.brute_force(ref["T"], dead)
    assert {0, 1, 63, 64, 65, 4097} <= set(tqf.SIZES) and (dead_want[1] == -1).all()
    for n in tqf.SIZES:
        before = r.cast_counts()
        q, w = extra[:n].copy(), tuple(x[:n].copy() for x in want)
        for at, k in ((0, 3), (n - 1, 28)) if n >= 2 else ():   # a dead query at either end
            q[at] = dead[k]
            for x, dx in zip(w, dead_want):
                x[at] = dx[k]
        _same(_ask_into(r, torch, q, 5, f"n = {n}"), w, f"n = {n}")
        if n == 0:
            assert r.cast_counts() == before
    _same(_ask_into(r, torch, np.tile(dead, (5, 1))[:130], 5, "all dead"), tuple(np.tile(x, (5, 1))[:130] for x in dead_want), "all dead")
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


@pytest.mark.gpu
def test_masks(R, torch, scenes, get_scene):
    """primitive masks set after the build against cull masks 0xFF, 1, 2, 0x80 and 0 (which sees nothing): with the nearest triangle masked out the next one answers;
    an alpha cutoff changes nothing"""
    sc = tcp._card_scene(scenes, get_scene)
    clear, solid = len(sc.primitives) - 2, len(sc.primitives) - 1
    T = nd.world_triangles(sc.primitives)
    q = scene_queries(T, 5)[1024:3072]
    q[::3, 3] = np.inf
    plain = nd.brute_force(T, q)
    assert int((plain[1][:, 0] == clear).sum()) > 20 and int((plain[1][:, 0] == solid).sum()) > 20
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
        want = nd.brute_force(T, q, vis=vis, cull=cull)
        got = _ask(r, torch, q, cull_mask=cull)
        _same(got, want, f"cull {cull:#x}")
        hidden = [p for p in range(len(sc.primitives)) if not (vis[p] & cull)]
        assert not np.isin(got[1][:, 0], hidden).any()
        if cull == 0:
            assert (got[1] == -1).all()
        if cull == 0x01:   # the clear card is masked out: where it was nearest, another triangle or a miss answers
            was = plain[1][:, 0] == clear
            assert int((got[1][was, 0] >= 0).sum()) > 5 and (got[0][was, 0] >= plain[0][was, 0]).all()
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["presets", "one-version"])
def test_trees_a_refit_wrote(R, torch, get_scene, form):
    """Cornell with its last primitive as a model of its own on a dynamic scene that never rebuilds: after a matrix move, after art_scene_set_vertices, after the
    primitive is disabled and after it is enabled again a batch on one side stream with no synchronisation in between: each is the reference over a model built from
    scratch of the world vertices as of its call"""
    sc = get_scene("cornell")
    q = _scene_ref(get_scene, "cornell", 1.0)["q"][1024:3072]
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
    m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
    verts = np.array(moving.verts, np.float32)
    verts[:, 0:3] = verts[:, 0:3] * np.float32(0.75) + np.array([0.0, 0.05, 0.0], np.float32)
    moved, deformed = static + [P(moving.verts, moving.indices, moving.tex, m)], static + [P(verts, moving.indices, moving.tex, m)]
    states = [("moved", moved, ()), ("deformed", deformed, ()), ("disabled", deformed, (len(static),)), ("enabled", deformed, ())]
    r = R.Renderer((64, 64), dynamic_scene=True, tuning=dict({"refit_rebuild_ratio": -1.0}, **tqf.REFITS[form]))
    r.add_model(static)
    r.add_model([moving])
    r.prepare_first_frame()
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
        assert not r.needs_build()
        with torch.cuda.stream(s):
            outs.append(r.closest_triangles(d_q))
    s.synchronize()
    wants = [nd.brute_force(nd.world_triangles(prims, disabled=off), q) for _, prims, off in states]
    for (what, _, _), got, want in zip(states, outs, wants):
        _same(_host(got), want, f"{form}, {what}")
    assert not np.array_equal(wants[0][0], wants[1][0]) and not np.array_equal(wants[1][1], wants[2][1]) and not (wants[2][1][:, 0] == len(static)).any()
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 3 and r.cast_counts()["casts"] == 0, st
    r.close()


@pytest.mark.gpu
def test_the_ring_with_kinds_mixed_on_three_streams(R, torch, get_scene):
    """80 operations -- closest_triangles, overlap_triangles (list), closest_points, cast_rays in turn -- over three torch streams on Cornell with 1024 queries each,
    nothing synchronised before the end: the ring of ART_CAST_POOL cursor blocks is lapped with neighbours of other kinds on other streams.  Every result of the three
    query kinds is its reference; the casts counted are the ray casts'"""
    from araytracingjourney_amd import _lib
    assert 80 > 2 * _lib.ART_CAST_POOL
    ref, n = _scene_ref(get_scene, "cornell", 1.0), 1024
    q = ref["q"][:n]
    want_overlap = nto.brute_force(ref["T"], q, 4)
    pts = np.ascontiguousarray(q[:, 0:4])
    want_points = nc.brute_force(ref["T"], pts)
    rays = np.concatenate([q[:, 0:3], np.zeros((n, 1), F), q[:, 4:7] - q[:, 0:3], np.ones((n, 1), F)], 1).astype(F)
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_q, d_p, d_r = _up(torch, q), _up(torch, pts), _up(torch, rays)
    streams = [torch.cuda.Stream() for _ in range(3)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(80):
        with torch.cuda.stream(streams[i % 3]):
            kind = ("distance", "overlap", "points", "cast")[i % 4]
            outs.append((kind, {"distance": lambda: r.closest_triangles(d_q), "overlap": lambda: r.overlap_triangles(d_q, "list", 4), "points": lambda: r.closest_points(d_p),
                                "cast": lambda: r.cast_rays(d_r)}[kind]()))
    counts = r.cast_counts()
    for s in streams:
        s.synchronize()
    for i, (kind, got) in enumerate(outs):
        what = f"operation {i} ({kind})"
        if kind == "distance":
            _same(_host(got), _cut(ref["want"], n), what)
        elif kind == "overlap":
            ids, count = _host(got)
            assert np.array_equal(ids, want_overlap[2]) and np.array_equal(count.view(np.uint32), want_overlap[1]), what
        elif kind == "points":
            tcp._same(_host(got), want_points, what)
    assert counts["casts"] == 20 and counts["rays"] == 20 * n and counts["host_waits"] <= 80 - _lib.ART_CAST_POOL, counts
    r.close()


@pytest.mark.gpu
def test_the_contexts_own_stream_and_optional_points(R, torch, get_scene):
    """hip_stream NULL -- the descriptor by hand, the wrapper cannot say it -- is the context's cast stream, and art_cast_sync is the fence; point_dev and qpoint_dev left
    out are not written: Cornell's first 1027 queries"""
    from araytracingjourney_amd import _lib
    ref, n = _scene_ref(get_scene, "cornell", 1.0), 1027
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_q = _up(torch, ref["q"][:n])
    duv, ids, point, qpoint = outs = _patterned(torch, n + 2)
    torch.cuda.synchronize()
    d = _lib.ArtTriDistance(tris_dev=d_q.data_ptr(), duv_dev=duv.data_ptr(), ids_dev=ids.data_ptr(), n=n, cull_mask=0xFF)
    assert r._L.art_closest_triangles(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    assert (point.view(torch.int32) == PATTERN).all() and (qpoint.view(torch.int32) == PATTERN).all() and _untouched(outs, n)
    d.point_dev, d.qpoint_dev = point.data_ptr(), qpoint.data_ptr()
    assert r._L.art_closest_triangles(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    assert _untouched(outs, n)
    _same(_host(tuple(t[:n] for t in outs)), _cut(ref["want"], n), "the context's stream")
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", ["none", "translation", "scale"])
def test_mesh_clearance(R, torch, get_scene, matrix):
    """test_tri_overlap's mesh of 600 triangles in Cornell, shrunk so that most of it is clear of the walls, as it is and through matrices whose products are exact:
    the records are closest_triangles of the buffer numpy gathers with the same operations and the radius, and `nearest` is their reduction -- the smallest d among
    the records with an answer, the lowest index among equals (the nearest triangle stands in the mesh three times; moved by the translation the mesh cuts a box and
    92 of its triangles tie at 0) -- at r = 0.1 and +inf; a triangle with an index outside the positions is dead; no call makes the host wait for the device (torch's sync debug mode raises where one would); a mesh far away at r = 1 has no answer: index -1 and the miss record"""
    ref = _scene_ref(get_scene, "cornell", 1.0)
    T = ref["T"]
    lo, hi = tto.scene_bounds(T)
    rng = np.random.default_rng(17)
    c = 0.5 * (lo + hi)
    pos = (c + (rng.uniform(0.0, 1.0, (400, 3)) - 0.5) * (hi - lo) * 0.2 + np.array([0.0, 0.25 * float(hi[1] - lo[1]), 0.0])).astype(F) * F(0.5 if matrix == "scale" else 1.0)
    near = np.argsort(np.linalg.norm(pos[:, None] - pos[None], axis=2), axis=1)[:, 1:30]
    a = rng.integers(0, 400, 600)
    idx = np.stack([a, near[a, rng.integers(0, 29, 600)], near[a, rng.integers(0, 29, 600)]], 1).astype(np.int64)
    idx[7] = (0, 1, 400); idx[11] = (-1, 2, 3)   # outside the positions
    mm = tto.MATRICES[matrix]

    def gathered(idx, radius):
        p = pos[np.clip(idx, 0, 399)]
        if mm is not None:
            m = np.asarray(mm, F).reshape(3, 4)
            p = np.stack([((p[..., 0] * m[k, 0] + p[..., 1] * m[k, 1]) + p[..., 2] * m[k, 2]) + m[k, 3] for k in range(3)], -1).astype(F)
        p[[7, 11]] = np.nan
        q = tto._tris(p)
        q[:, 3] = radius
        return q
    first = nd.brute_force(T, gathered(idx, np.inf))
    best = int(np.argmin(np.where(first[1][:, 0] >= 0, first[0][:, 0], np.inf)))
    assert best not in (0, 7, 11, 599)
    idx[599] = idx[best]; idx[3] = idx[best]   # the same triangle three times: ties on the smallest distance
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_pos, d_idx = _up(torch, pos), _up(torch, idx)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    for radius, stream, d_i in ((np.inf, None, d_idx), (0.1, s, d_idx.to(torch.int32))):
        s.wait_stream(torch.cuda.current_stream())
        with _no_sync(torch):
            records, nearest = r.mesh_clearance(d_pos, d_i, mm, radius, stream=stream)
        torch.cuda.synchronize()
        want = nd.brute_force(T, gathered(idx, radius))
        _same(_host(records), want, f"mesh_clearance, {matrix}, r = {radius}")
        has = want[1][:, 0] >= 0
        assert has.sum() > 3 and not has[7] and not has[11]
        at = int(np.flatnonzero(has & (want[0][:, 0] == want[0][has, 0].min()))[0])
        assert at == min(3, best) and int((want[0][has, 0] == want[0][at, 0]).sum()) >= 3
        assert int(nearest["index"]) == at and nearest["index"].dtype == torch.int64
        assert _bits(nearest["distance"].cpu().numpy()) == _bits(want[0][at, 0]) and np.array_equal(nearest["ids"].cpu().numpy(), want[1][at])
        assert np.array_equal(_bits(nearest["point"].cpu().numpy()), _bits(want[2][at])) and np.array_equal(_bits(nearest["qpoint"].cpu().numpy()), _bits(want[3][at]))
    with _no_sync(torch):
        records, nearest = r.mesh_clearance(d_pos, d_idx, [1, 0, 0, 64.0, 0, 1, 0, 0, 0, 0, 1, 0], 1.0)
        nothing = r.mesh_clearance(d_pos, d_idx[:0], mm, 2.0)
    assert int(nearest["index"]) == -1 and float(nearest["distance"]) == 1.0 and (nearest["ids"] == -1).all() and not nearest["point"].any() and not nearest["qpoint"].any() and (records[1] == -1).all()
    records, nearest = nothing
    assert records[0].shape == (0, 4) and int(nearest["index"]) == -1 and float(nearest["distance"]) == 2.0
    for args in ((d_pos.cpu(), d_idx), (d_pos, d_idx.float()), (d_pos, d_idx[:, :2]), (d_pos[:, :2], d_idx), (d_pos, d_idx, [1.0] * 11), (d_pos, d_idx, None, -1.0),
                 (d_pos, d_idx, None, float("nan")), (d_pos, d_idx, None, 1.0, 0x100), (d_pos[:0], d_idx)):
        with pytest.raises((ValueError, TypeError)):
            r.mesh_clearance(*args)
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
    tris = _up(torch, _scene_ref(get_scene, "cornell", 1.0)["q"][:n + 1])
    duv, ids, point, qpoint = outs = _patterned(torch, n + 1)
    torch.cuda.synchronize()

    def desc(**kw):
        d = dict(tris_dev=tris.data_ptr(), duv_dev=duv.data_ptr(), ids_dev=ids.data_ptr(), point_dev=point.data_ptr(), qpoint_dev=qpoint.data_ptr(), hip_stream=None, n=n,
                 cull_mask=0xFF, flags=0, reserved=0)
        d.update(kw)
        return _lib.ArtTriDistance(**d)

    def said(d):
        code = L.art_closest_triangles(ctx, C.byref(d) if d is not None else None)
        return code, L.art_last_error()

    clean = lambda: _untouched(outs, 0)   # noqa: E731
    state = WHO + b"scene not built, or changed since the build (art_scene_build)"
    assert said(desc()) == (_lib.ART_E_STATE, state)
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert L.art_closest_triangles(None, C.byref(desc())) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    assert said(None) == (_lib.ART_E_INVALID, WHO + b"null argument")
    bad = [(desc(flags=1), b"flags: must be 0"), (desc(flags=0x80000000), b"flags: must be 0"), (desc(reserved=1), b"reserved: must be 0"),
           (desc(cull_mask=0x100), b"cull_mask: above 0xFF"), (desc(cull_mask=0xFFFFFFFF), b"cull_mask: above 0xFF"),
           (desc(n=_lib.ART_CAST_MAX_RAYS + 1), b"n: above ART_CAST_MAX_RAYS"), (desc(n=0xFFFFFFFF), b"n: above ART_CAST_MAX_RAYS"),
           (desc(tris_dev=None), b"tris_dev: null or not 16-byte aligned"), (desc(tris_dev=tris.data_ptr() + 8), b"tris_dev: null or not 16-byte aligned"),
           (desc(duv_dev=None), b"duv_dev: null or not 16-byte aligned"), (desc(duv_dev=duv.data_ptr() + 4), b"duv_dev: null or not 16-byte aligned"),
           (desc(ids_dev=None), b"ids_dev: null or not 8-byte aligned"), (desc(ids_dev=ids.data_ptr() + 4), b"ids_dev: null or not 8-byte aligned"),
           (desc(point_dev=point.data_ptr() + 8), b"point_dev: not 16-byte aligned"), (desc(qpoint_dev=qpoint.data_ptr() + 8), b"qpoint_dev: not 16-byte aligned")]
    for d, text in bad:
        assert said(d) == (_lib.ART_E_INVALID, WHO + text), text
    r.cast_sync()
    torch.cuda.synchronize()
    assert r.cast_counts() == zero and clean()
    assert said(desc(n=0))[0] == 0 and said(desc(n=0, tris_dev=None, duv_dev=None, ids_dev=None, point_dev=None, qpoint_dev=None))[0] == 0
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    # the wrapper's own checks: before anything is enqueued
    for args, kw in (((tris.cpu(),), {}), ((tris.double(),), {}), ((tris[:, :8],), {}), ((tris,), dict(cull_mask=0x100)), ((tris,), dict(out=(duv[:8], ids, point, qpoint))),
                     ((tris,), dict(out=(duv, ids.to(torch.int64), point, qpoint))), ((tris,), dict(out=(duv, ids, point))), ((tris,), dict(out=(duv, ids, point, qpoint[:, :3])))):
        with pytest.raises((ValueError, TypeError)):
            r.closest_triangles(*args, **kw)
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    assert said(desc())[0] == 0
    r.cast_sync()
    assert _untouched(outs, n) and not (ids[:n] == PATTERN).any() and r.cast_counts() == zero
    r.add_model([sc.primitives[0]])   # a primitive added since the build: art_scene_needs_build
    assert r.needs_build() and said(desc()) == (_lib.ART_E_STATE, state)
    with pytest.raises(_lib.ArtError):
        r.closest_triangles(tris)
    r.close()
