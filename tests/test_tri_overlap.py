"""art_overlap_triangles (include/art.h): the scene triangles that touch each of a buffer of query triangles, defined exactly and checked bit for bit.

The reference is tests/np_tri_overlap.py: conditions 1 .. 3 over every (query, triangle) pair in numpy float32, operation by operation, on np_closest.world_triangles'
fields (imported, not copied).  Nothing on the device has a tolerance: the hit bytes, the counts (uncapped) and the ids.  A reference is computed once per set of inputs,
to a depth of 8, shared by every kind and K and never written.

The CPU tests tie the reference to an independent witness (float64: an edge of either triangle meets the other by closed Moeller-Trumbore, coplanar pairs in their
plane) with the query scaled about its centroid by 1 - e and 1 + e.  eps is test_overlap.py's length, 1e-5 times the largest coordinate magnitude of the set, and e is
eps over the mean distance of the query's vertices from its centroid (at most 0.5): every vertex moves by about eps, whatever the query's size -- a factor of 1e-5 itself
would move the vertices of a small query by less than a float32 rounding of its coordinates.  Measured shares of the overlapping pairs that fall inside the band between
the shrunk and the grown query (bound: 1 %), over all 4096 queries of each scene:
    Cornell 1.0         4 009 overlapping pairs of 7 152 whose boxes come within eps,     8 in the band (0.200 %), eps 8.8e-6
    sponza_like 0.05   10 675 overlapping pairs of 154 774,                              13 in the band (0.122 %), eps 2.7e-5
The float32 formulas against their float64 evaluation on 200 000 random pairs, half about the origin and half offset by 100 units: 0 of 200 000 disagree (33 949 overlap), and the
witness disagrees with neither on any pair.
Measured counts, queries with more than 8 candidates / with none / the largest count:
    Cornell 1.0 (4096 queries, 34 triangles)        49 / 2 456 /    14
    sponza_like 0.05 (4096, 7 144)                 308 / 2 344 /    91
    the lattice (2071, 576)                      1 469 /    28 /    26
    the clump (256, 1000)                           72 /   153 / 1 000
    the chain (130, 64)                             33 /     1 /    64
    the specials on sponza_like (414, 7 144)        96 /   119 / 6 744
Of the specials' 64 turned triangles, 13 are kept from their originals by the six in-plane axes alone (those in an axis plane), and 7 of the 64 float32 centroids touch
their own face as a point.

Mutation checks, on scratch builds of the library run over the 44 GPU tests of this module (queries that differ at each test's first failing comparison):
  * condition 2's `<=` turned into `<` in the leaf step: 16 tests fail -- the four hostile sets (hit bytes of 2 043 of the lattice's 2 071 queries and of 98 of the 414
    specials; counts of 7 of the clump's 256, 149 for 1 000 at the point, and of 64 of the chain's 130) and the clump and the chain on all six tree forms.  The scenes'
    random and moved queries share no plane coordinate with a triangle's box, so the 28 others pass.
  * the six in-plane axes dropped: 2 tests fail -- the lattice (counts of 1 083 of 2 071 queries: coplanar faces apart from each other come out as touching) and the
    specials (one turned triangle's hit byte).  Everything else has no coplanar pair whose boxes meet.
  * TravBox::pop skipping spilled entries: 28 tests fail -- sponza_like (hit bytes of 2 of 4 096 queries, the same two under all eight knobs; counts of 8 of the first
    63 at both chunk sizes), the four hostile sets (the lattice's counts of 15 queries, the clump's hit byte of one, the chain's counts of 33 of 130 with 13 for 64, the
    specials' whole-scene query 1 666 for 6 744), the clump and the chain on all six tree forms, and the masks' scene (one count).  The 16 that pass run on Cornell's
    34 triangles, which never fill a lane's eight LDS entries -- and the errors.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_tri_overlap as nt
import test_closest_points as tcp
import test_query_forms as tqf
from helpers import chain_scene, degenerate_soup, lattice_coords, lattice_scene
from helpers import _layout_is_the_headers, _host, R, torch, _up  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = -0x5A5A5A5B   # tests/test_cast.py's: what oversized output buffers are filled with
N = 4096
KS = (1, 4, 8)          # one list size on the device: no instance boundary to straddle
KREF = 8
WHO = b"art_overlap_triangles: "
F = np.float32
COORDS = [0, 1, 2, 4, 5, 6, 8, 9, 10]

_REF = {}


def _frozen(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def scene_bounds(T):
    here = T["lo"][:, 0] < nt.NOWHERE
    return T["lo"][here].min(axis=0), T["hi"][here].max(axis=0)


def _tri(q0, q1, q2):
    q = np.zeros(12, F)
    q[0:3], q[4:7], q[8:11] = q0, q1, q2
    return q


def _tris(w):
    """[n, 3, 3] vertices -> [n, 12] queries"""
    w = np.asarray(w, F).reshape(-1, 3, 3)
    q = np.zeros((w.shape[0], 12), F)
    q[:, 0:3], q[:, 4:7], q[:, 8:11] = w[:, 0], w[:, 1], w[:, 2]
    return q


def scene_queries(T, seed):
    """4096 queries: 2048 random triangles (a centre in the scene's box, the three vertices within a cube of half side 0.3 % .. 30 % of the scene's extent round it), then
    2048 of the scene's own triangles moved by a random offset of 0.1 % .. 2 % of the extent (near-touching and edge-sharing pairs).  The smallest offset is a
    hundred times the witness test's eps: what a moved triangle touches is then decided by its offset and not by a rounding (with offsets from 0.01 % on, ten eps,
    1.147 % of Cornell's overlapping pairs lay in the witness's band, over its cap).  Words 3, 7 and 11, which are not read, hold a NaN and the infinities"""
    lo, hi = scene_bounds(T)
    rng = np.random.default_rng(seed)
    ext = float((hi - lo).max())
    c = lo + rng.uniform(0.0, 1.0, (N // 2, 3)) * (hi - lo).astype(np.float64)
    half = ext * 10.0 ** rng.uniform(-2.5, -0.5, (N // 2, 1, 1))
    rnd = c[:, None, :] + half * rng.uniform(-1.0, 1.0, (N // 2, 3, 3))
    own = T["w"][rng.integers(0, T["w"].shape[0], N // 2)].astype(np.float64)
    d = rng.normal(0.0, 1.0, (N // 2, 3))
    d *= (ext * 10.0 ** rng.uniform(-3.0, -1.7, N // 2) / np.linalg.norm(d, axis=1))[:, None]
    q = _tris(np.concatenate([rnd, own + d[:, None, :]]).astype(F))
    q[:, 3], q[:, 7], q[:, 11] = np.nan, np.inf, -np.inf
    return q


def _ref(key, make):
    """{scene, T, q, want} of a set of inputs: make() -> (scene, queries); computed once at K = 8, shared, never written"""
    if key not in _REF:
        sc, q = make()
        T = nt.world_triangles(sc.primitives)
        q = np.ascontiguousarray(q, F)
        q.setflags(write=False)
        _REF[key] = dict(scene=sc, T=T, q=q, want=_frozen(nt.brute_force(T, q, KREF)))
    return _REF[key]


def _scene_ref(get_scene, name, detail):
    def make():
        sc = get_scene(name, detail)
        return sc, scene_queries(nt.world_triangles(sc.primitives), 13)
    return _ref((name, detail), make)


def _cut(want, K, n=None):
    """the reference at K <= 8, of the first n queries: (hit, count, ids)"""
    hit, count, ids = want
    return hit[:n], count[:n], ids[:n, :K]


def _same(got, want, what=""):
    """got: (hit, count, ids) of the device, count as torch's int32; want: the reference's"""
    (hit, count, ids), (rhit, rcount, rids) = got, want
    assert hit.shape == rhit.shape and hit.dtype == np.uint8 and count.shape == rcount.shape and ids.shape == rids.shape and ids.dtype == np.int32, what
    bad = hit != rhit
    assert not bad.any(), f"{what}: the hit bytes of {int(bad.sum())} of {hit.shape[0]} queries differ (first: {np.flatnonzero(bad)[:5]})"
    bad = count.view(np.uint32) != rcount
    assert not bad.any(), f"{what}: the counts of {int(bad.sum())} of {hit.shape[0]} queries differ (first: {np.flatnonzero(bad)[:5]}: {count[bad][:3]} for {rcount[bad][:3]})"
    bad = (ids != rids).any(axis=(1, 2))
    assert not bad.any(), f"{what}: the ids of {int(bad.sum())} of {hit.shape[0]} queries differ (first: {np.flatnonzero(bad)[:5]}: {ids[bad][:1]} for {rids[bad][:1]})"


def _ask(r, torch, q, K, **kw):
    """ANY and LIST at K on the same queries: (hit, count, ids) on the host"""
    d_q = _up(torch, q)
    hit = r.overlap_triangles(d_q, "any", **kw)
    ids, count = r.overlap_triangles(d_q, "list", K, **kw)
    torch.cuda.synchronize()
    return _host((hit, count, ids))


def _patterned(torch, n, K):
    return (torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((n,), PATTERN, dtype=torch.int32, device="cuda"),
            torch.full((n, K, 2), PATTERN, dtype=torch.int32, device="cuda"))


def _ask_into(r, torch, q, K, extra, what, stream=None, **kw):
    """the same into tensors `extra` records too long and filled with a pattern: the tail keeps it"""
    n = q.shape[0]
    hit, count, ids = _patterned(torch, n + extra, K)
    d_q = _up(torch, np.asarray(q).reshape(n, 12))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        assert r.overlap_triangles(d_q, "any", out=hit, **kw) is hit
        got = r.overlap_triangles(d_q, "list", K, out=(ids, count), **kw)
        assert got[0] is ids and got[1] is count
    torch.cuda.synchronize()
    assert (hit[n:] == 0xA5).all() and (count[n:] == PATTERN).all() and (ids[n:] == PATTERN).all(), f"{what}: written beyond n"
    return _host((hit[:n], count[:n], ids[:n]))


# ---- the special queries ---------------------------------------------------------------------------------------------------------------------------------------------
def dead_queries():
    """a NaN, +inf and -inf in each of the nine coordinates in turn: 27 triangles round the origin that would otherwise touch anything there"""
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        for k in COORDS:
            q = _tri((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5))
            q[k] = bad
            out.append(q)
    return np.stack(out)


N_OWN, PER_OWN = 64, 6


def special_queries(T):
    """[0] a triangle larger than the scene, through its middle; [1] one that reaches 3e37 on every side; [2] one far away; then for 64 triangles of the scene:
    the triangle handed back unchanged (it lists itself and its neighbours), its first vertex as a point, its centroid (float32) as a point on the face, a segment
    through the face along its normal (q1 == q2), a segment along its first edge, and the triangle turned about a point just beyond the middle of its longest edge --
    in its plane, apart from it, the boxes meeting: a pair only the six in-plane axes separate where the plane is an axis plane; then the dead queries.  Words 3, 7 and
    11 hold a NaN and the infinities"""
    lo, hi = scene_bounds(T)
    c, e = 0.5 * (lo + hi), hi - lo
    out = [_tri(c + e * F(4) * np.array([-1, -0.3, -1], F), c + e * F(4) * np.array([1, 0.1, -1], F), c + e * F(4) * np.array([0, 0.2, 2], F)),
           _tri((-3e37, -3e37, -3e37), (3e37, 3e37, -3e37), (0, 3e37, 3e37)), _tri(hi + F(1), hi + F(2), hi + np.array([1, 2, 1], F))]
    w = T["w"][::max(1, T["w"].shape[0] // N_OWN)][:N_OWN]
    for t in w:
        g = ((t[0] + t[1]) + t[2]) / F(3)
        n = np.cross(t[1] - t[0], t[2] - t[0])
        n = (n / max(np.linalg.norm(n), 1e-30) * 0.05 * float(e.max())).astype(F)
        k = int(np.argmax([np.linalg.norm(t[(j + 2) % 3] - t[(j + 1) % 3]) for j in range(3)]))   # the vertex opposite the longest edge
        mid = F(0.5) * t[(k + 1) % 3] + F(0.5) * t[(k + 2) % 3]
        piv = mid + F(0.125) * (mid - t[k])
        out += [_tri(*t), _tri(t[0], t[0], t[0]), _tri(g, g, g), _tri(g - n, g + n, g + n), _tri(t[0], t[1], t[1]), _tri(*[F(2) * piv - v for v in t])]
    q = np.concatenate([np.stack(out), dead_queries()]).astype(F)
    q[:, 3], q[:, 7], q[:, 11] = np.nan, -np.inf, np.inf
    return q


def lattice_queries():
    """triangles whose vertices are lattice points: both halves of the 3 x 7 x 36 faces of the lattice's cells, the 343 lattice points as points, and 216 triangles across
    the cells' body diagonals.  Every coordinate is a multiple of 0.25 and so is every vertex of the scene: products and sums are exact, and every answer turns on <= """
    g = lattice_coords(6)
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        i, j, k = [a.reshape(-1) for a in np.meshgrid(np.arange(7), np.arange(6), np.arange(6), indexing="ij")]
        for corners in (((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (0, 1))):
            w = np.zeros((i.size, 3, 3), F)
            for m, (du, dv) in enumerate(corners):
                w[:, m, axis], w[:, m, u], w[:, m, v] = g[i], g[j + du], g[k + dv]
            out.append(_tris(w))
    i, j, k = [a.reshape(-1) for a in np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij")]
    p = np.stack([g[i], g[j], g[k]], 1)
    out.append(_tris(np.stack([p, p, p], 1)))
    i, j, k = [a.reshape(-1) for a in np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")]
    out.append(_tris(np.stack([np.stack([g[i], g[j], g[k]], 1), np.stack([g[i + 1], g[j + 1], g[k]], 1), np.stack([g[i + 1], g[j + 1], g[k + 1]], 1)], 1)))
    return np.concatenate(out)


def clump_queries():
    """1000 triangles share the vertex (0.1, 0.05, 0.3): that point as a point, triangles round it from 1e-6 to 0.5, random triangles beside it"""
    p = np.array([0.1, 0.05, 0.3], F)
    out = [_tri(p, p, p)] + [_tri(p + F(s) * np.array([-1, -1, 0], F), p + F(s) * np.array([1, -1, 0], F), p + F(s) * np.array([0, 2, 0], F)) for s in (1e-6, 1e-3, 0.01, 0.03, 0.1, 0.5)]
    rng = np.random.default_rng(3)
    for _ in range(249):
        c = p + rng.uniform(-0.08, 0.08, 3)
        out.append(_tri(*(c + rng.uniform(-0.04, 0.04, (3, 3)))))
    return np.stack(out).astype(F)


def chain_queries():
    """triangles across the chain of 64 nested slivers at x = 2^-k and x = 1.5 * 2^-k, long ones from the origin to 2^-k through all the slivers from k on, the whole"""
    w = 0.01
    out = [_tri((2.0 ** -k, -w, -w), (2.0 ** -k, w, -w), (2.0 ** -k, 0.0, 2 * w)) for k in range(64)]
    out += [_tri((1.5 * 2.0 ** -k, -w, 0.0), (1.5 * 2.0 ** -k, w, 0.0), (1.5 * 2.0 ** -k, 0.0, w)) for k in range(32)]
    out += [_tri((0.0, -w / 2, w / 4), (0.0, w / 2, w / 4), (2.0 ** -k, 0.0, w / 4)) for k in range(32)]
    out += [_tri((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), _tri((-1.0, -1.0, 0.005), (3.0, -1.0, 0.005), (1.0, 3.0, 0.005))]
    return np.stack(out).astype(F)


HOSTILE = ["lattice", "clump", "chain", "specials"]


def _hostile(get_scene, which):
    if which == "lattice":
        return _ref(which, lambda: (lattice_scene(6), lattice_queries()))
    if which == "clump":
        return _ref(which, lambda: (degenerate_soup(1000, "one point"), clump_queries()))
    if which == "chain":
        return _ref(which, lambda: (chain_scene(64)[0], chain_queries()))
    sc = get_scene("sponza_like", 0.05)
    return _ref(which, lambda: (sc, special_queries(nt.world_triangles(sc.primitives))))


INSIDE_CORNELL = _tri((-0.5, 0.2, -0.1), (-0.3, 0.2, 0.1), (-0.4, 0.4, -0.1))   # in the air beside the boxes: 0.2 wide, wholly inside the closed room


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_ctypes_descriptor_is_the_headers():
    """ArtTriQuery as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 64 bytes"""
    _layout_is_the_headers("ArtTriQuery", 64, ["tris_dev", "hit_dev", "ids_dev", "count_dev", "hip_stream", "n", "kind", "max_hits", "cull_mask", "flags", "reserved"])


def test_presence():
    """art_overlap_triangles(NULL, NULL) is ART_E_INVALID with the prefixed message on any machine; the library exports it, the Rust binding declares the function and the
    struct, the header cites DESIGN.md 3.13, the C++ mirror has the call, and Renderer has both methods"""
    from araytracingjourney_amd import _lib, renderer
    L = _lib.load()
    assert L.art_overlap_triangles(None, None) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    d = _lib.ArtTriQuery(flags=1)
    nowhere = C.create_string_buffer(1 << 16)
    assert L.art_overlap_triangles(nowhere, C.byref(d)) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"flags: must be 0"
    so = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "art_overlap_triangles" for line in syms.splitlines() if line.strip())
    rs = open(os.path.join(ROOT, "bindings", "art_sys.rs")).read()
    assert "pub fn art_overlap_triangles(" in rs and "pub struct ArtTriQuery" in rs
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "DESIGN.md 3.13" in hdr and "### 3.13" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "art_overlap_triangles(" in open(os.path.join(ROOT, "araytracingjourney_amd", "host", "art_renderer.hpp")).read()
    assert callable(renderer.Renderer.overlap_triangles) and callable(renderer.Renderer.collide_mesh)


def _one(tri, query, skip=()):
    w = np.asarray(tri, F).reshape(1, 3, 3)
    T = dict(w=w, v0=w[:, 0].copy(), e1=w[:, 1] - w[:, 0], e2=w[:, 2] - w[:, 0], lo=w.min(axis=1), hi=w.max(axis=1), prim=np.zeros(1, np.int32), tri=np.zeros(1, np.int32))
    q = _tris(np.asarray(query, F).reshape(1, 3, 3))
    if skip:
        return int(nt.pairs(T, q, skip=skip)[0].size)
    hit, count, ids = nt.brute_force(T, q, 1)
    assert count[0] == hit[0] and (ids[0, 0, 0] == 0) == bool(hit[0])
    return int(hit[0])


IN_PLANE = tuple(range(11, 17))


def test_known_answers():
    """the triangle (0,0,0) (1,0,0) (0,1,0): queries that pierce it, pass it by, touch it at a vertex, along an edge and in a point of its face; a query edge through the
    face whose three edge rays would say nothing of a scene edge piercing the QUERY's face; coplanar queries -- overlapping, touching, apart (which only the six
    in-plane axes separate); parallel planes; segments and points; a zero-area scene triangle"""
    t = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    assert _one(t, [(0.2, 0.2, -1), (0.2, 0.2, 1), (0.3, 0.9, 1)]) == 1                # an edge of the query pierces the face
    assert _one(t, [(2, 2, -1), (2, 2, 1), (3, 2, 0)]) == 0                            # the boxes apart
    assert _one(t, [(0.8, 0.8, -1), (0.8, 0.8, 1), (1.5, 1.5, 0)]) == 0                # boxes meet; the query passes the hypotenuse by
    assert _one(t, [(-1, -1, 0.5), (3, -1, -0.5), (-1, 3, -0.5)]) == 1                 # a big query through it: the triangle's edges pierce the query's face, no query edge comes near
    assert _one(t, [(1, 0, 0), (2, 0, 1), (2, 1, -1)]) == 1                            # touching at one vertex
    assert _one(t, [(1, 0, 0), (2, 0, 0), (2, 0, 1)]) == 1                             # ... and with a whole edge on the line of an edge, meeting in a point
    assert _one(t, [(0, 0, 0), (1, 0, 0), (0.5, 0, 1)]) == 1                           # sharing an edge, planes at right angles
    assert _one(t, [(0.25, 0.25, 0), (0.5, 0.25, 1), (0.25, 0.5, 1)]) == 1             # a vertex of the query in the face
    assert _one(t, [(0.25, 0.25, 1e-3), (0.5, 0.25, 1), (0.25, 0.5, 1)]) == 0          # ... and just above it
    assert _one(t, [(0.1, 0.1, 0), (0.4, 0.1, 0), (0.1, 0.4, 0)]) == 1                 # coplanar, inside
    assert _one(t, [(-1, -1, 0), (3, -1, 0), (-1, 3, 0)]) == 1                         # coplanar, round it
    assert _one(t, [(0.5, 0.5, 0), (1, 1, 0), (0.25, 1.5, 0)]) == 1                    # coplanar, a vertex on the hypotenuse
    assert _one(t, [(1, 0, 0), (2, 0, 0), (1.5, -1, 0)]) == 1                          # coplanar, touching at a vertex
    apart = [(0.75, 0.75, 0), (1.5, 0.75, 0), (0.75, 1.5, 0)]                            # coplanar, beyond the hypotenuse; the boxes meet
    assert _one(t, apart) == 0 and _one(t, apart, skip=IN_PLANE) == 1                    # 11 axes alone would call them overlapping
    assert _one(t, [(0.1, 0.1, 0.25), (0.4, 0.1, 0.25), (0.1, 0.4, 0.25)]) == 0        # parallel planes
    assert _one(t, [(0.25, 0.25, -1), (0.25, 0.25, 1), (0.25, 0.25, 1)]) == 1          # a segment through the face
    assert _one(t, [(0.75, 0.75, -1), (0.75, 0.75, 1), (0.75, 0.75, 1)]) == 0          # a segment past it
    assert _one(t, [(0.25, 0.25, 0)] * 3) == 1 and _one(t, [(0.25, 0.25, 0.5)] * 3) == 0 and _one(t, [(1, 0, 0)] * 3) == 1   # points: on the face, off it, a vertex
    seg = [(0, 0, 0), (1, 0, 0), (0.5, 0, 0)]                                            # a zero-area scene triangle: a segment
    assert _one(seg, [(0.5, -1, -1), (0.5, 1, -1), (0.5, 0, 2)]) == 1 and _one(seg, [(0.5, 1, -1), (0.5, 2, -1), (0.5, 1, 2)]) == 0


def _stretch(q, e):
    """[P, 3, 3] float64 queries scaled about their centroids by 1 + e ([P])"""
    g = q.mean(axis=1, keepdims=True)
    return g + (1.0 + e)[:, None, None] * (q - g)


@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_the_brute_force_against_the_witness(get_scene, name, detail):
    """over the scene's 4096 queries and every triangle: wherever the query shrunk about its centroid meets the triangle (float64 witness), the float32 reference says 1;
    wherever the grown one does not, it says 0; and the band between them holds at most 1 % of the overlapping pairs.  Every vertex moves by about eps = 1e-5 times the
    largest coordinate magnitude (the module's docstring)"""
    ref = _scene_ref(get_scene, name, detail)
    T, q = ref["T"], ref["q"]
    eps = 1e-5 * float(max(np.abs(T["w"]).max(), np.abs(q[:, COORDS]).max()))
    qi, gi = nt.pairs(T, q)
    said = np.zeros((q.shape[0], T["v0"].shape[0]), bool)
    said[qi, gi] = True
    w = q[:, COORDS].reshape(-1, 3, 3).astype(np.float64)
    g = w.mean(axis=1, keepdims=True)
    e = np.minimum(eps / np.linalg.norm(w - g, axis=2).mean(axis=1), 0.5)
    big = _stretch(w, e)
    lo, hi = big.min(axis=1), big.max(axis=1)
    near = ((T["lo"].astype(np.float64)[None] <= hi[:, None]) & (lo[:, None] <= T["hi"].astype(np.float64)[None])).all(axis=2)
    assert not (said & ~near).any()   # (the grown query's box of every other pair misses the triangle's own box: nothing shared, and the reference says nothing)
    ci, cg = np.nonzero(near)
    grown, shrunk = nt.witness(T["w"][cg], big[ci]), nt.witness(T["w"][cg], _stretch(w, -e)[ci])
    s = said[ci, cg]
    assert not (shrunk & ~grown).any()
    assert s[shrunk].all(), f"{int((shrunk & ~s).sum())} pairs overlap by more than eps and the reference says 0"
    assert not s[~grown].any(), f"{int((~grown & s).sum())} pairs are apart by more than eps and the reference says 1"
    band, total = int((grown & ~shrunk).sum()), int(said.sum())
    print(f"\n[tri overlap] {name}: {ci.size} near pairs, {total} overlapping, {band} in the band ({100.0 * band / total:.3f} %), eps {eps:.3g}")
    assert total > 1000 and band <= 0.01 * total


def random_pairs(n, seed, offset):
    """n pairs of random triangles that mostly come near each other: vertices within 1 of a common centre, which lies within 10 of `offset` on every axis"""
    rng = np.random.default_rng(seed)
    c = offset + rng.uniform(-10.0, 10.0, (n, 1, 3))
    t = (c + rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(F)
    q = (c + rng.uniform(-1.0, 1.0, (n, 1, 3)) * 0.7 + rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(F)
    return t, q


def test_float32_against_float64():
    """the 17-axis formulas evaluated in float32 and in float64 on the same 200 000 float32 pairs, half about the origin and half offset by 100 units: the answers agree
    but for pairs within rounding of touching -- at most 1 in 10 000 of the pairs may differ (float32's 2^-24 against separations that are uniform on the scale of 1) --
    and both agree with the witness wherever they agree with each other, but for as few"""
    differ = total = overlapping = against = 0
    for seed, offset in ((1, 0.0), (2, 100.0)):
        t, q = random_pairs(100_000, seed, offset)
        col = lambda x, dt: [x[:, k].astype(dt) for k in range(3)]   # noqa: E731
        got = {}
        for dt in (np.float32, np.float64):
            v0, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]   # the record's fields are float32 in both
            got[dt] = nt.tri_tri_overlap(col(v0, dt), col(e1, dt), col(e2, dt), col(q[:, 0], dt), col(q[:, 1], dt), col(q[:, 2], dt))
        wit = nt.witness(np.stack([t[:, 0], t[:, 0] + (t[:, 1] - t[:, 0]), t[:, 0] + (t[:, 2] - t[:, 0])], 1), q)
        same = got[np.float32] == got[np.float64]
        differ += int((~same).sum()); total += t.shape[0]; overlapping += int(got[np.float64].sum()); against += int((same & (wit != got[np.float64])).sum())
    print(f"\n[tri overlap] float32 against float64: {differ} of {total} pairs differ, {overlapping} overlap; the witness disagrees with both on {against}")
    assert overlapping > 20_000 and differ <= total // 10_000 and against <= total // 10_000


CASES = ["cornell", "sponza_like", "lattice", "clump", "chain", "specials"]


def _case(get_scene, name):
    return _scene_ref(get_scene, name, 0.05 if name == "sponza_like" else 1.0) if name in ("cornell", "sponza_like") else _hostile(get_scene, name)


@pytest.mark.parametrize("name", CASES)
def test_the_comparisons_are_not_vacuous(get_scene, name):
    """from the reference alone: queries with more than 8 candidates (the list evicts), queries with none, the largest count; what each special query is there for"""
    ref = _case(get_scene, name)
    hit, count, ids = ref["want"]
    T, q, n = ref["T"], ref["q"], ref["q"].shape[0]
    ntri = T["v0"].shape[0]
    nine = np.flatnonzero(count > 8)
    print(f"\n[tri overlap] {name}: {n} queries, {ntri} triangles; more than 8: {nine.size}, none: {int((count == 0).sum())}, largest count {int(count.max())}")
    assert np.array_equal(hit, (count > 0).astype(np.uint8)) and np.array_equal(ids[..., 0] >= 0, np.arange(8)[None] < count[:, None])
    assert nine.size >= (4 if name == "cornell" else 30) and (ids[nine, :, 0] >= 0).all()   # (Cornell has 34 triangles: few queries touch nine of them)
    if name in ("cornell", "sponza_like"):
        assert n == N and int((count == 0).sum()) >= 200 and int((count[N // 2:] > 0).sum()) >= 200 and int((count[:N // 2] > 0).sum()) >= 200
    if name == "cornell":
        one = nt.brute_force(T, INSIDE_CORNELL[None], 1)
        lo, hi = scene_bounds(T)
        assert one[1][0] == 0 and (lo < INSIDE_CORNELL[COORDS].reshape(3, 3)).all() and (INSIDE_CORNELL[COORDS].reshape(3, 3) < hi).all()   # a SURFACE test
    if name == "specials":
        assert count[0] > 8 and count[1] > 8 and count[2] == 0 and not count[-27:].any()
        own = count[3:3 + PER_OWN * N_OWN].reshape(N_OWN, PER_OWN)
        gids = np.arange(ntri)[::max(1, ntri // N_OWN)][:N_OWN]
        assert (own[:, 0] >= 2).all() and (own[:, 1] >= 1).all() and (own[:, 4] >= 1).all() and int((own[:, 3] >= 1).sum()) >= N_OWN - 4
        qi, gi = nt.pairs(T, q[3:3 + PER_OWN * N_OWN:PER_OWN])
        assert all(gids[k] in gi[qi == k] for k in range(N_OWN))      # handed back unchanged, a triangle lists itself
        turned = q[3 + 5:3 + PER_OWN * N_OWN:PER_OWN]
        lax = nt.pairs(T, turned, skip=IN_PLANE)
        only = int(sum(gids[k] in lax[1][lax[0] == k] for k in range(N_OWN))) - int(sum(gids[k] in nt.pairs(T, turned)[1][nt.pairs(T, turned)[0] == k] for k in range(N_OWN)))
        print(f"[tri overlap] specials: {only} of {N_OWN} turned triangles are kept from their originals by the six in-plane axes alone")
        assert only >= 8   # (most of sponza_like's triangles lie in no axis plane: there the turned copy is not exactly in the plane and the normal separates it)
        print(f"[tri overlap] specials: a centroid as a point touches its face for {int((own[:, 2] >= 1).sum())} of {N_OWN} (float32 centroids are not all on the face)")
    if name == "clump":
        assert ntri == 1000 and count[0] == 1000
    if name == "chain":
        assert count[-1] == 64 and int(count[:64].max()) >= 2
    if name == "lattice":
        assert n == 2 * 3 * 252 + 343 + 216 and int((count == 0).sum()) > 0


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_both_scenes_are_the_brute_forces(R, torch, get_scene, name, detail):
    """4096 queries on a side stream, ANY and LIST at K = 1, 4 and 8: hit bytes, counts and ids; a permutation of the queries gives the permuted answers; oversized out=
    tensors filled with a pattern are untouched beyond n; the queries count neither as casts nor as rays"""
    ref = _scene_ref(get_scene, name, detail)
    q = ref["q"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    s = torch.cuda.Stream()
    for K in KS:
        want = _cut(ref["want"], K)
        _same(_ask_into(r, torch, q, K, 70, f"{name}, K = {K}", stream=s), want, f"{name}, K = {K}")
        _same(_ask(r, torch, q[perm], K), tuple(w[perm] for w in want), f"{name}, K = {K}, permuted")
    if name == "cornell":
        got = _ask(r, torch, INSIDE_CORNELL[None], 8)
        assert got[0][0] == 0 and got[1][0] == 0 and (got[2] == -1).all()   # wholly inside the box, touching nothing
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_inputs(R, torch, get_scene, which):
    """the lattice with queries whose vertices are lattice points (every answer turns on <=); 1000 triangles round one point with queries round it (a count of 1000,
    stacks past their LDS part); the chain of 64 nested slivers; and on sponza_like a query larger than the scene, one that reaches 3e37, scene triangles handed back
    unchanged, points, segments, and the dead queries -- NaN, +-inf in every coordinate: hit 0, count 0, miss records"""
    ref = _hostile(get_scene, which)
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    for K in (8, 3):
        _same(_ask_into(r, torch, ref["q"], K, 3, which), _cut(ref["want"], K), f"{which}, K = {K}")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(tqf.FORMS))
@pytest.mark.parametrize("name", ["clump", "chain", "cornell"])
def test_every_tree_form_gives_the_reference(R, torch, get_scene, name, form):
    """the answers are defined as independent of the structure: the clump, the chain and Cornell's 4096 queries on every tree form of tests/test_query_forms.py"""
    ref = _case(get_scene, name)
    r = R.renderer_for_scene(ref["scene"], (64, 64), **tqf.FORMS[form])
    for K in (8, 4):
        _same(_ask(r, torch, ref["q"], K), _cut(ref["want"], K), f"{name}, {form}, K = {K}")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", tqf.KNOBS, ids=lambda k: "-".join(f"{a}-{b}" for a, b in k.items()))
def test_knobs_change_the_schedule_never_the_records(R, torch, get_scene, knobs):
    """tests/test_query_forms.py's eight tracer settings (trace_chunk 64 / 65536, trace_refill 1 / 64, trace_blocks 1 / 16384, trace_leaf_batch 1 / 64) on sponza_like at
    0.05: the reference's bits.  (The loop is the point queries': why trace_leaf_batch = 64 and trace_refill = 64 cannot hang it is argued there)"""
    ref = _scene_ref(get_scene, "sponza_like", 0.05)
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning=knobs)
    _same(_ask(r, torch, ref["q"], 8), ref["want"], str(knobs))
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [64, 128])
def test_sizes_at_which_a_refill_can_go_wrong(R, torch, get_scene, chunk):
    """ArtTuning.trace_chunk = 64 (a chunk is one filling of a wave) and 128: prefixes of sponza_like's queries of tests/test_query_forms.py's sizes (0, 1, 63, 64, 65
    .. 4097), then a batch that is all dead; every batch into tensors five records too long filled with a pattern.  n = 0 enqueues nothing"""
    ref, K = _scene_ref(get_scene, "sponza_like", 0.05), 8
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning={"trace_chunk": chunk})
    extra = np.concatenate([ref["q"], ref["q"][:1]])   # 4097
    want = tuple(np.concatenate([w, w[:1]]) for w in ref["want"])
    assert {0, 1, 63, 64, 65, 4097} <= set(tqf.SIZES)
    for n in tqf.SIZES:
        before = r.cast_counts()
        _same(_ask_into(r, torch, extra[:n], K, 5, f"n = {n}"), _cut(want, K, n), f"n = {n}")
        if n == 0:
            assert r.cast_counts() == before
    dead = np.tile(dead_queries(), (5, 1))[:130]
    got = _ask_into(r, torch, dead, K, 5, "all dead")
    assert not got[0].any() and not got[1].any() and (got[2] == -1).all()
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


@pytest.mark.gpu
def test_masks(R, torch, scenes, get_scene):
    """primitive masks set after the build against cull masks 0xFF, 1, 2, 0x80 and 0 (which sees nothing): a masked primitive drops out of every list and every count;
    an alpha cutoff changes nothing"""
    sc = tcp._card_scene(scenes, get_scene)
    clear, solid = len(sc.primitives) - 2, len(sc.primitives) - 1
    T, K = nt.world_triangles(sc.primitives), 8
    q = scene_queries(T, 5)[1024:3072]
    plain = nt.brute_force(T, q, K)
    assert int((plain[2][..., 0] == clear).any(axis=1).sum()) > 20 and int((plain[2][..., 0] == solid).any(axis=1).sum()) > 20
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    _same(_ask(r, torch, q, K), plain, "unmasked")
    m.set_alpha_cutoff(clear, 0.5); m.set_alpha_cutoff(solid, 0.5)
    _same(_ask(r, torch, q, K), plain, "with cutoffs: not tested")
    masks = {0: 0x01, 1: 0x02, solid: 0x03, clear: 0x02}
    for i, v in masks.items():
        m.set_mask(i, v)
    vis = np.array([masks.get(p, 0xFF) for p in range(len(sc.primitives))])
    counts = []
    for cull in (0xFF, 0x01, 0x02, 0x80, 0):
        want = nt.brute_force(T, q, K, vis=vis, cull=cull)
        got = _ask(r, torch, q, K, cull_mask=cull)
        _same(got, want, f"cull {cull:#x}")
        hidden = [p for p in range(len(sc.primitives)) if not (vis[p] & cull)]
        assert not np.isin(got[2][..., 0], hidden).any()
        if cull == 0:
            assert not got[0].any() and not got[1].any() and (got[2] == -1).all()
        counts.append(got[1].copy())
    assert not np.array_equal(counts[1], counts[2]) and not np.array_equal(counts[0], counts[1])
    r.close()


@pytest.mark.gpu
def test_a_primitive_disabled_after_the_build_is_nowhere(R, torch, scenes, get_scene):
    """two primitives, one disabled after the build: it is in no list and no count, also of a query a million units wide and of one at 3e38, where its record
    stands; enabled again, the first answers return"""
    sc = tcp._card_scene(scenes, get_scene)
    two = scenes.Scene("two", list(sc.primitives[-2:]), sc.camera, sc.lights)
    T, K = nt.world_triangles(two.primitives), 8
    q = np.concatenate([scene_queries(T, 9)[1536:2560], [_tri((-1e6, -1e6, 0.0), (1e6, -1e6, 0.0), (0.0, 1e6, 0.015625)), _tri((3.0e38,) * 3, (3.0e38,) * 3, (3.0e38,) * 3),
                                                         _tri((2.9e38,) * 3, (3.2e38, 2.9e38, 2.9e38), (2.9e38, 3.2e38, 3.2e38))]]).astype(F)
    r = R.Renderer((64, 64), tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(two.primitives)
    r.prepare_first_frame()
    both = nt.brute_force(T, q, K)
    assert both[1][-3] > 0 and both[1][-1] == 0 and {0, 1} <= set(np.unique(both[2][..., 0]).tolist())
    _same(_ask(r, torch, q, K), both, "both")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 0) == 0 and not r.needs_build()
    want = nt.brute_force(nt.world_triangles(two.primitives, disabled=(1,)), q, K)
    assert not (want[2][..., 0] == 1).any() and want[1][-2] == 0 and want[1][-1] == 0 and not np.array_equal(want[1], both[1])
    _same(_ask(r, torch, q, K), want, "one disabled")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 1) == 0
    _same(_ask(r, torch, q, K), both, "enabled again")
    assert r.stats()["rebuilds"] == 0
    r.close()


@pytest.mark.gpu
def test_the_scene_as_of_the_call(R, torch, get_scene):
    """Cornell's last primitive as a model of its own on a dynamic scene that never rebuilds: after art_scene_set_model_matrix a batch on a side stream, no
    synchronisation in between: each batch is the reference over the triangles as of its call, the refit in front of the query"""
    sc = get_scene("cornell")
    q = _scene_ref(get_scene, "cornell", 1.0)["q"][1024:3072]
    r = R.Renderer((64, 64), dynamic_scene=True, tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(list(sc.primitives[:-1]))
    r.add_model([sc.primitives[-1]])
    r.prepare_first_frame()
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
    m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
    states = [("built", list(sc.primitives)), ("moved", static + [P(moving.verts, moving.indices, moving.tex, m)])]
    d_q = _up(torch, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for what, _ in states:
        if what == "moved":
            r.models_mut()[1].set_model_matrix(m)
        assert not r.needs_build()
        with torch.cuda.stream(s):
            outs.append((r.overlap_triangles(d_q, "any"),) + r.overlap_triangles(d_q, "list", 8)[::-1])
    s.synchronize()
    wants = [nt.brute_force(nt.world_triangles(prims), q, 8) for _, prims in states]
    for (what, _), got, want in zip(states, outs, wants):
        _same(_host(got), want, what)
    assert not np.array_equal(wants[0][1], wants[1][1])
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 1 and r.cast_counts()["casts"] == 0
    r.close()


@pytest.mark.gpu
def test_the_contexts_own_stream(R, torch, get_scene):
    """hip_stream NULL -- the descriptor by hand, the wrapper cannot say it -- is the context's cast stream, and art_cast_sync is the fence: Cornell's first 1027 queries"""
    from araytracingjourney_amd import _lib
    ref, n, K = _scene_ref(get_scene, "cornell", 1.0), 1027, 4
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_q = _up(torch, ref["q"][:n])
    hit, count, ids = _patterned(torch, n + 2, K)
    torch.cuda.synchronize()
    for d in (_lib.ArtTriQuery(tris_dev=d_q.data_ptr(), hit_dev=hit.data_ptr(), n=n, kind=_lib.ART_OVERLAP_ANY, cull_mask=0xFF),
              _lib.ArtTriQuery(tris_dev=d_q.data_ptr(), ids_dev=ids.data_ptr(), count_dev=count.data_ptr(), n=n, kind=_lib.ART_OVERLAP_LIST, max_hits=K, cull_mask=0xFF)):
        assert r._L.art_overlap_triangles(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    assert (hit[n:] == 0xA5).all() and (count[n:] == PATTERN).all() and (ids[n:] == PATTERN).all()
    _same(_host((hit[:n], count[:n], ids[:n])), _cut(ref["want"], K, n), "the context's stream")
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


# a row-major 3x4 each, every product exact in float32: translations by powers of two, an axis permutation, a mirror, a scale by 2
MATRICES = {"none": None, "translation": [1, 0, 0, 0.25, 0, 1, 0, -0.125, 0, 0, 1, 0.5], "permutation": [0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0],
            "mirror": [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], "scale": [2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0.0625]}


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", list(MATRICES))
def test_collide_mesh(R, torch, get_scene, matrix):
    """a mesh of 600 triangles over 400 shared vertices in Cornell, as it is and through matrices whose products are exact: collide_mesh is overlap_triangles of the
    buffer numpy gathers with the same operations -- kind "any", and "list" at K = 3, int64 and int32 indices, on a side stream; a triangle with an index outside the
    positions is dead; a mesh far away collides with nothing"""
    ref = _scene_ref(get_scene, "cornell", 1.0)
    T = ref["T"]
    lo, hi = scene_bounds(T)
    rng = np.random.default_rng(17)
    pos = (lo + rng.uniform(0.0, 1.0, (400, 3)) * (hi - lo)).astype(F) * F(0.5 if matrix == "scale" else 1.0)
    near = np.argsort(np.linalg.norm(pos[:, None] - pos[None], axis=2), axis=1)[:, 1:30]   # triangles between nearby vertices, sharing vertices
    a = rng.integers(0, 400, 600)
    idx = np.stack([a, near[a, rng.integers(0, 29, 600)], near[a, rng.integers(0, 29, 600)]], 1).astype(np.int64)
    idx[7] = (0, 1, 400); idx[11] = (-1, 2, 3)   # outside the positions
    mm = MATRICES[matrix]
    p = pos[np.clip(idx, 0, 399)]
    if mm is not None:
        m = np.asarray(mm, F).reshape(3, 4)
        p = np.stack([((p[..., 0] * m[k, 0] + p[..., 1] * m[k, 1]) + p[..., 2] * m[k, 2]) + m[k, 3] for k in range(3)], -1).astype(F)
    p[[7, 11]] = np.nan
    q = _tris(p)
    want = nt.brute_force(T, q, 3)
    assert want[0].sum() > 20 and want[0][7] == 0 and want[0][11] == 0 and (want[1] > 3).any()
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_pos, d_idx = _up(torch, pos), _up(torch, idx)
    d_idx32 = d_idx.to(torch.int32)   # (made on the current stream, which the side stream waits for below)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    hit = r.collide_mesh(d_pos, d_idx, mm)
    ids, count = r.collide_mesh(d_pos, d_idx32, None if mm is None else np.asarray(mm, np.float32).reshape(3, 4), "list", 3, stream=s)
    away = r.collide_mesh(d_pos, d_idx, [1, 0, 0, 64.0, 0, 1, 0, 0, 0, 0, 1, 0])
    nothing = r.collide_mesh(d_pos, d_idx[:0], mm, "list", 2)
    torch.cuda.synchronize()
    _same(_host((hit, count, ids)), want, f"collide_mesh, {matrix}")
    assert hit.dtype == torch.uint8 and hit.shape == (600,) and not away.any() and nothing[0].shape == (0, 2, 2) and nothing[1].shape == (0,)
    _same(_ask(r, torch, q, 3), want, "the same buffer through overlap_triangles")
    for args in ((d_pos.cpu(), d_idx), (d_pos, d_idx.float()), (d_pos, d_idx[:, :2]), (d_pos[:, :2], d_idx), (d_pos, d_idx, [1.0] * 11), (d_pos, d_idx, [np.nan] * 12),
                 (d_pos, d_idx, None, "all"), (d_pos, d_idx, None, "list", 9), (d_pos[:0], d_idx)):
        with pytest.raises((ValueError, TypeError)):
            r.collide_mesh(*args)
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
    n, K = 64, 3
    tris = _up(torch, _scene_ref(get_scene, "cornell", 1.0)["q"][:n + 1])
    hit, count, ids = _patterned(torch, n + 1, K)
    torch.cuda.synchronize()

    def lst(**kw):
        d = dict(tris_dev=tris.data_ptr(), hit_dev=None, ids_dev=ids.data_ptr(), count_dev=count.data_ptr(), hip_stream=None, n=n, kind=_lib.ART_OVERLAP_LIST, max_hits=K,
                 cull_mask=0xFF, flags=0, reserved=0)
        d.update(kw)
        return _lib.ArtTriQuery(**d)

    def any_(**kw):
        return lst(**dict(dict(hit_dev=hit.data_ptr(), ids_dev=None, count_dev=None, kind=_lib.ART_OVERLAP_ANY, max_hits=0), **kw))

    def said(d):
        code = L.art_overlap_triangles(ctx, C.byref(d) if d is not None else None)
        return code, L.art_last_error()

    clean = lambda: (hit == 0xA5).all() and (count == PATTERN).all() and (ids == PATTERN).all()   # noqa: E731
    state = WHO + b"scene not built, or changed since the build (art_scene_build)"
    assert said(lst()) == (_lib.ART_E_STATE, state) and said(any_()) == (_lib.ART_E_STATE, state)
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert L.art_overlap_triangles(None, C.byref(lst())) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    assert said(None) == (_lib.ART_E_INVALID, WHO + b"null argument")
    bad = [(lst(flags=1), b"flags: must be 0"), (any_(flags=0x80000000), b"flags: must be 0"), (lst(reserved=1), b"reserved: must be 0"),
           (lst(kind=2), b"kind: ART_OVERLAP_ANY or ART_OVERLAP_LIST"), (lst(kind=0xFFFFFFFF), b"kind: ART_OVERLAP_ANY or ART_OVERLAP_LIST"),
           (lst(cull_mask=0x100), b"cull_mask: above 0xFF"), (any_(cull_mask=0xFFFFFFFF), b"cull_mask: above 0xFF"),
           (lst(n=_lib.ART_CAST_MAX_RAYS + 1), b"n: above ART_CAST_MAX_RAYS"), (any_(n=0xFFFFFFFF), b"n: above ART_CAST_MAX_RAYS"),
           (lst(tris_dev=None), b"tris_dev: null or not 16-byte aligned"), (any_(tris_dev=tris.data_ptr() + 8), b"tris_dev: null or not 16-byte aligned"),
           (any_(ids_dev=ids.data_ptr()), b"ids_dev / count_dev: must be NULL for ART_OVERLAP_ANY"), (any_(count_dev=count.data_ptr()), b"ids_dev / count_dev: must be NULL for ART_OVERLAP_ANY"),
           (any_(max_hits=1), b"max_hits: must be 0 for ART_OVERLAP_ANY"), (any_(hit_dev=None), b"hit_dev: null"),
           (lst(hit_dev=hit.data_ptr()), b"hit_dev: must be NULL for ART_OVERLAP_LIST"), (lst(max_hits=0), b"max_hits: 1 .. ART_CAST_MAX_HITS"),
           (lst(max_hits=_lib.ART_CAST_MAX_HITS + 1), b"max_hits: 1 .. ART_CAST_MAX_HITS"), (lst(ids_dev=None), b"ids_dev: null or not 8-byte aligned"),
           (lst(ids_dev=ids.data_ptr() + 4), b"ids_dev: null or not 8-byte aligned"), (lst(count_dev=count.data_ptr() + 2), b"count_dev: not 4-byte aligned")]
    for d, text in bad:
        assert said(d) == (_lib.ART_E_INVALID, WHO + text), text
    r.cast_sync()
    torch.cuda.synchronize()
    assert r.cast_counts() == zero and clean()
    assert said(lst(n=0))[0] == 0 and said(any_(n=0, tris_dev=None, hit_dev=None))[0] == 0 and said(lst(n=0, tris_dev=None, ids_dev=None, count_dev=None))[0] == 0
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    # the wrapper's own checks: before anything is enqueued
    for args, kw in (((tris.cpu(),), {}), ((tris.double(),), {}), ((tris[:, :8],), {}), ((tris, "all"), {}), ((tris, "list", 0), {}), ((tris, "list", 9), {}),
                     ((tris, "list", 2.5), {}), ((tris,), dict(cull_mask=0x100)), ((tris, "list", K), dict(out=(ids[:8], count))),
                     ((tris, "list", K), dict(out=(ids, count.to(torch.int64)))), ((tris, "list", K + 1), dict(out=(ids, count))), ((tris, "any"), dict(out=hit[:8]))):
        with pytest.raises((ValueError, TypeError)):
            r.overlap_triangles(*args, **kw)
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    assert said(lst(count_dev=None))[0] == 0   # the optional output left out: it is not written
    r.cast_sync()
    assert (count == PATTERN).all() and (ids[n:] == PATTERN).all() and not (ids[:n] == PATTERN).any() and (hit == 0xA5).all() and r.cast_counts() == zero
    assert said(any_())[0] == 0 and said(lst())[0] == 0
    r.cast_sync()
    assert (hit[:n] <= 1).all() and hit[n] == 0xA5 and (count[:n] >= 0).all() and count[n] == PATTERN and r.cast_counts() == zero
    r.add_model([sc.primitives[0]])   # a primitive added since the build: art_scene_needs_build
    assert r.needs_build() and said(lst()) == (_lib.ART_E_STATE, state)
    with pytest.raises(_lib.ArtError):
        r.overlap_triangles(tris)
    r.close()
