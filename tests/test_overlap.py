"""art_overlap_boxes (include/art.h): the triangles that touch each of a buffer of boxes, defined exactly and checked bit for bit.

The reference is tests/np_overlap.py: conditions 1 .. 4 over every (box, triangle) pair in numpy float32, operation by operation, on np_closest.world_triangles' fields
(imported, not copied).  Nothing on the device has a tolerance: the hit bytes, the counts (uncapped) and the ids.  A reference is computed once per set of inputs, to a
depth of 8, shared by every kind and K and never written.

The CPU tests tie the reference to an independent witness (float64, the triangle clipped against the box's six planes) with the box shrunk and grown by eps = 1e-5 times
the largest coordinate magnitude of the set, and count, in the reference alone, what the GPU tests lean on.  Measured shares of the overlapping pairs that fall inside the
band between the shrunk and the grown box (bound: 1 %; the sets are the 2048 random boxes of each scene -- the grid cells' faces lie in Cornell's walls by construction,
pairs that are exact by design and not generic):
    Cornell 1.0         1 864 overlapping pairs of 2 706 whose boxes come within eps,      0 in the band (0.000 %), eps 9.2e-6
    sponza_like 0.05   47 682 overlapping pairs of 49 982,                               14 in the band (0.029 %), eps 2.8e-5
Measured counts, boxes with more than 8 candidates / with none / whose 8th and 9th candidates sit in different primitives / the largest count:
    Cornell 1.0 (4096 boxes, 34 triangles)        13 / 2 698 /  1 /    14
    sponza_like 0.05 (4096, 7 144)               989 / 2 031 / 33 /   990
    the lattice (1440, 576)                    1 113 /    28 /  - /   120
    the clump (256, 1000)                        139 /    94 /  - / 1 000
    the chain (130, 64)                           58 /     1 /  - /    64
    the specials on sponza_like (216, 7 144)      65 /    22 /  7 / 7 144

Mutation checks, on scratch builds of the library run over the 31 GPU tests of this module (boxes that differ at each test's first failing comparison):
  * condition 2's `<=` turned into `<` in the leaf step: 30 tests fail -- all but the errors.  Hit bytes: Cornell 426 of 4096 (the grid's cells whose faces lie in the
    walls), sponza_like 75, the lattice 1 314 of 1 440, the specials 129 of 216 (every box with lo == hi), the masks' set 254 of 2 048, the two cards 64 of 1 027;
    counts: the chain 127 of 130, the clump's point box 149 for 1 000; the same figures on all six tree forms; the sizes at n = 4097; voxelize.
  * TravBox::pop skipping spilled entries: 19 tests fail -- sponza_like (counts of 289 of 4096 boxes), the four hostile sets (the lattice 98 of 1 440, the clump 110
    of 256 with 599 for 1 000 at the point box, the chain 57 of 130 with 13 for 64, the specials' two whole-scene boxes 1 751 for 7 144), the clump and the chain on all
    six tree forms (ANY alone, which ends at its first candidate, loses one box of the clump on the two canonical trees), and both chunk sizes of the sizes at n = 63.
    The twelve that pass run on Cornell's 34 triangles (or the two cards' 16), which never fill a lane's eight LDS entries: its scene test, its six tree forms, the
    masks, the two cards, the moved model, voxelize -- and the errors.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_overlap as no
import test_closest_points as tcp
import test_query_forms as tqf
from helpers import chain_scene, degenerate_soup, lattice_coords, lattice_scene
from helpers import _layout_is_the_headers, _host, R, torch, _up  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = -0x5A5A5A5B   # tests/test_cast.py's: what oversized output buffers are filled with
N = 4096
KS = (1, 4, 8)          # one list size on the device: no instance boundary to straddle
KREF = 8
WHO = b"art_overlap_boxes: "
F = np.float32

_REF = {}


def _frozen(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def scene_bounds(T):
    here = T["lo"][:, 0] < no.NOWHERE
    return T["lo"][here].min(axis=0), T["hi"][here].max(axis=0)


def grid_boxes(origin, cell, dims):
    """Renderer.voxelize's boxes in numpy: lo = origin + idx * cell, hi = origin + (idx + 1) * cell in float32, a product and a sum; [nx * ny * nz, 8], x slowest"""
    origin, cell = np.asarray(origin, F), np.broadcast_to(np.asarray(cell, F), (3,))
    planes = [(np.arange(dims[k] + 1, dtype=F) * cell[k] + origin[k]).astype(F) for k in range(3)]
    b = np.zeros(tuple(dims) + (8,), F)
    for k in range(3):
        shape = [1, 1, 1]
        shape[k] = dims[k]
        b[..., k], b[..., 4 + k] = planes[k][:-1].reshape(shape), planes[k][1:].reshape(shape)
    return b.reshape(-1, 8)


def scene_boxes(T, seed):
    """4096 boxes: every other cell of a 16^3 grid over the scene's box (2048), then 2048 random boxes of random size (half sides from 0.3 % to 30 % of the scene's
    extent, per axis) about centres in the scene's box.  Words 3 and 7, which are not read, hold a NaN and an infinity"""
    lo, hi = scene_bounds(T)
    cells = grid_boxes(lo, (hi - lo) / F(16), (16, 16, 16))
    i, j, k = np.unravel_index(np.arange(4096), (16, 16, 16))
    cells = cells[(i + j + k) % 2 == 0]
    rng = np.random.default_rng(seed)
    ext = (hi - lo).astype(np.float64)
    c = lo + rng.uniform(0.0, 1.0, (N // 2, 3)) * ext
    half = ext * 10.0 ** rng.uniform(-2.5, -0.5, (N // 2, 3))
    rnd = np.zeros((N // 2, 8), F)
    rnd[:, 0:3], rnd[:, 4:7] = c - half, c + half
    b = np.concatenate([cells, rnd]).astype(F)
    b[:, 3], b[:, 7] = np.nan, np.inf
    return b


def _ref(key, make):
    """{scene, T, b, want} of a set of inputs: make() -> (scene, boxes); computed once at K = 8, shared, never written"""
    if key not in _REF:
        sc, b = make()
        T = no.world_triangles(sc.primitives)
        b = np.ascontiguousarray(b, F)
        b.setflags(write=False)
        _REF[key] = dict(scene=sc, T=T, b=b, want=_frozen(no.brute_force(T, b, KREF)))
    return _REF[key]


def _scene_ref(get_scene, name, detail):
    def make():
        sc = get_scene(name, detail)
        return sc, scene_boxes(no.world_triangles(sc.primitives), 11)
    return _ref((name, detail), make)


def _cut(want, K, n=None):
    """the reference at K <= 8, of the first n boxes: (hit, count, ids)"""
    hit, count, ids = want
    return hit[:n], count[:n], ids[:n, :K]


def _same(got, want, what=""):
    """got: (hit, count, ids) of the device, count as torch's int32; want: the reference's"""
    (hit, count, ids), (rhit, rcount, rids) = got, want
    assert hit.shape == rhit.shape and hit.dtype == np.uint8 and count.shape == rcount.shape and ids.shape == rids.shape and ids.dtype == np.int32, what
    bad = hit != rhit
    assert not bad.any(), f"{what}: the hit bytes of {int(bad.sum())} of {hit.shape[0]} boxes differ (first: {np.flatnonzero(bad)[:5]})"
    bad = count.view(np.uint32) != rcount
    assert not bad.any(), f"{what}: the counts of {int(bad.sum())} of {hit.shape[0]} boxes differ (first: {np.flatnonzero(bad)[:5]}: {count[bad][:3]} for {rcount[bad][:3]})"
    bad = (ids != rids).any(axis=(1, 2))
    assert not bad.any(), f"{what}: the ids of {int(bad.sum())} of {hit.shape[0]} boxes differ (first: {np.flatnonzero(bad)[:5]}: {ids[bad][:1]} for {rids[bad][:1]})"


def _ask(r, torch, b, K, **kw):
    """ANY and LIST at K on the same boxes: (hit, count, ids) on the host"""
    d_b = _up(torch, b)
    hit = r.overlap_boxes(d_b, "any", **kw)
    ids, count = r.overlap_boxes(d_b, "list", K, **kw)
    torch.cuda.synchronize()
    return _host((hit, count, ids))


def _patterned(torch, n, K):
    return (torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((n,), PATTERN, dtype=torch.int32, device="cuda"),
            torch.full((n, K, 2), PATTERN, dtype=torch.int32, device="cuda"))


def _ask_into(r, torch, b, K, extra, what, stream=None, **kw):
    """the same into tensors `extra` records too long and filled with a pattern: the tail keeps it"""
    n = b.shape[0]
    hit, count, ids = _patterned(torch, n + extra, K)
    d_b = _up(torch, np.asarray(b).reshape(n, 8))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        assert r.overlap_boxes(d_b, "any", out=hit, **kw) is hit
        got = r.overlap_boxes(d_b, "list", K, out=(ids, count), **kw)
        assert got[0] is ids and got[1] is count
    torch.cuda.synchronize()
    assert (hit[n:] == 0xA5).all() and (count[n:] == PATTERN).all() and (ids[n:] == PATTERN).all(), f"{what}: written beyond n"
    return _host((hit[:n], count[:n], ids[:n]))


# ---- the special boxes -----------------------------------------------------------------------------------------------------------------------------------------------
def _box(lo, hi):
    b = np.zeros(8, F)
    b[0:3], b[4:7] = lo, hi
    return b


def dead_boxes():
    """a NaN, +inf and -inf in each of the six coordinates in turn, then lo > hi on each axis in turn: 21 boxes round the origin that would otherwise touch anything there"""
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 1, 2, 4, 5, 6):
            b = _box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
            b[k] = bad
            out.append(b)
    for k in range(3):
        b = _box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
        b[k], b[4 + k] = 0.25, -0.25
        out.append(b)
    return np.stack(out)


def special_boxes(T):
    """one box round the whole scene (and one that reaches 3.2e38 on every side), boxes with lo == hi on three, two and one axes at vertices of the scene, the dead
    boxes, a box far away"""
    lo, hi = scene_bounds(T)
    out = [_box(lo, hi), _box((-3.2e38,) * 3, (3.2e38,) * 3), _box(hi + F(1), hi + F(2))]
    for v in T["w"].reshape(-1, 3)[::37][:64]:   # (64 of sponza_like's 21 432 vertices)
        out.append(_box(v, v))                                   # a point: a vertex of the scene
        out.append(_box(v, v + np.array([0.2, 0, 0], F)))        # a segment from it
        out.append(_box(v - np.array([0, 0.1, 0.1], F), v + np.array([0, 0.1, 0.1], F)))   # a rectangle through it
    return np.concatenate([np.stack(out), dead_boxes()]).astype(F)


def lattice_boxes():
    """boxes whose faces pass through lattice points: the 216 cells of the lattice, the 125 boxes of two cells a side, the 343 lattice points as boxes with lo == hi, and
    the cells' 3 x 7 x 36 faces as rectangles.  Every coordinate is a multiple of 0.25 and so is every vertex of the scene: every answer turns on <="""
    g = lattice_coords(6)
    out = []
    for w in (1, 2, 0):
        i, j, k = [a.reshape(-1) for a in np.meshgrid(*[np.arange(7 - w)] * 3, indexing="ij")]
        b = np.zeros((i.size, 8), F)
        b[:, 0], b[:, 1], b[:, 2], b[:, 4], b[:, 5], b[:, 6] = g[i], g[j], g[k], g[i + w], g[j + w], g[k + w]
        out.append(b)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        i, j, k = [a.reshape(-1) for a in np.meshgrid(np.arange(7), np.arange(6), np.arange(6), indexing="ij")]
        b = np.zeros((i.size, 8), F)
        b[:, axis], b[:, 4 + axis], b[:, u], b[:, 4 + u], b[:, v], b[:, 4 + v] = g[i], g[i], g[j], g[j + 1], g[k], g[k + 1]
        out.append(b)
    return np.concatenate(out)


def clump_boxes():
    """1000 triangles share the vertex (0.1, 0.05, 0.3): that point as a box, boxes round it from 1e-6 to 0.5, boxes beside it"""
    p = np.array([0.1, 0.05, 0.3], F)
    out = [_box(p, p)] + [_box(p - F(s), p + F(s)) for s in (1e-6, 1e-3, 0.01, 0.03, 0.1, 0.5)]
    rng = np.random.default_rng(3)
    for _ in range(249):
        c, h = p + rng.uniform(-0.08, 0.08, 3), rng.uniform(0.001, 0.04, 3)
        out.append(_box(c - h, c + h))
    return np.stack(out).astype(F)


def chain_boxes():
    """boxes from the origin to 2^-k along the chain of 64 nested slivers (box k holds the slivers from k on), thin boxes across it, the whole"""
    w = 0.01
    out = [_box((0.0, -w, 0.0), (2.0 ** -k, w, w)) for k in range(64)]
    out += [_box((2.0 ** -k, -w, 0.0), (2.0 ** -k, w, w)) for k in range(64)]          # rectangles across the chain
    out += [_box((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), _box((-1.0, -1.0, -1.0), (3.0, 1.0, 1.0))]
    return np.stack(out).astype(F)


HOSTILE = ["lattice", "clump", "chain", "specials"]


def _hostile(get_scene, which):
    if which == "lattice":
        return _ref(which, lambda: (lattice_scene(6), lattice_boxes()))
    if which == "clump":
        return _ref(which, lambda: (degenerate_soup(1000, "one point"), clump_boxes()))
    if which == "chain":
        return _ref(which, lambda: (chain_scene(64)[0], chain_boxes()))
    sc = get_scene("sponza_like", 0.05)
    return _ref(which, lambda: (sc, special_boxes(no.world_triangles(sc.primitives))))


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_ctypes_descriptor_is_the_headers():
    """ArtBoxQuery as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 64 bytes"""
    _layout_is_the_headers("ArtBoxQuery", 64, ["boxes_dev", "hit_dev", "ids_dev", "count_dev", "hip_stream", "n", "kind", "max_hits", "cull_mask", "flags", "reserved"])


def test_presence():
    """art_overlap_boxes(NULL, NULL) is ART_E_INVALID with the prefixed message on any machine; the library exports it, the Rust binding declares the function and the
    struct, the header cites DESIGN.md 3.11, and Renderer has both methods"""
    from araytracingjourney_amd import _lib, renderer
    L = _lib.load()
    assert L.art_overlap_boxes(None, None) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    d = _lib.ArtBoxQuery(flags=1)
    nowhere = C.create_string_buffer(1 << 16)
    assert L.art_overlap_boxes(nowhere, C.byref(d)) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"flags: must be 0"
    assert (_lib.ART_OVERLAP_ANY, _lib.ART_OVERLAP_LIST) == (0, 1)
    so = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "art_overlap_boxes" for line in syms.splitlines() if line.strip())
    rs = open(os.path.join(ROOT, "bindings", "art_sys.rs")).read()
    assert "pub fn art_overlap_boxes(" in rs and "pub struct ArtBoxQuery" in rs
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "DESIGN.md 3.11" in hdr and "### 3.11" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert callable(renderer.Renderer.overlap_boxes) and callable(renderer.Renderer.voxelize)


def _one(tri, lo, hi):
    w = np.asarray(tri, F).reshape(1, 3, 3)
    T = dict(w=w, v0=w[:, 0].copy(), e1=w[:, 1] - w[:, 0], e2=w[:, 2] - w[:, 0], lo=w.min(axis=1), hi=w.max(axis=1), prim=np.zeros(1, np.int32), tri=np.zeros(1, np.int32))
    hit, count, ids = no.brute_force(T, _box(lo, hi)[None], 1)
    assert count[0] == hit[0] and (ids[0, 0, 0] == 0) == bool(hit[0])
    return int(hit[0])


def test_known_answers():
    """the unit box [0, 1]^3: a triangle inside it, one that straddles it, one outside; triangles that touch a face, an edge and a corner from outside count; a triangle
    whose own box meets the box but which an edge axis separates (it passes the corner by), and one the plane separates; a huge triangle that cuts the box with no
    vertex near it; a zero-area triangle (a segment through the box; a point on its corner)"""
    lo, hi = (0, 0, 0), (1, 1, 1)
    assert _one([(0.2, 0.2, 0.2), (0.8, 0.3, 0.4), (0.4, 0.7, 0.6)], lo, hi) == 1                 # inside
    assert _one([(0.5, 0.5, 0.5), (2.0, 0.5, 0.5), (0.5, 2.0, 0.5)], lo, hi) == 1                 # straddling
    assert _one([(2.0, 2.0, 2.0), (3.0, 2.0, 2.0), (2.0, 3.0, 2.5)], lo, hi) == 0                 # outside, the boxes apart
    assert _one([(1.0, 0.2, 0.2), (1.0, 0.8, 0.2), (1.0, 0.5, 0.8)], lo, hi) == 1                 # in the face x = 1
    assert _one([(1.0, 0.2, 0.2), (2.0, 0.8, 0.2), (2.0, 0.5, 0.8)], lo, hi) == 1                 # a vertex on the face
    assert _one([(1.0, 1.0, 0.5), (2.0, 1.0, 0.5), (1.0, 2.0, 0.5)], lo, hi) == 1                 # a vertex on the edge x = y = 1
    assert _one([(1.0, 1.0, 1.0), (2.0, 1.0, 1.5), (1.0, 2.0, 1.5)], lo, hi) == 1                 # a vertex on the corner
    assert _one([(1.0, 2.0, 0.5), (2.0, 1.0, 0.5), (2.0, 2.0, 0.5)], lo, hi) == 0                 # own box [1,2]^2 touches the corner edge x = y = 1; the edge x + y = 3 is far from it: an edge axis separates
    assert _one([(1.5, 0.0, 0.5), (0.0, 1.5, 0.5), (2.0, 2.0, 0.5)], (0, 0, 0), (0.5, 0.5, 1)) == 0   # own box [0,2]^2 holds the box; the edge x + y = 1.5 passes the edge x = y = 0.5 by
    assert _one([(1.0, 0.0, 0.5), (0.0, 1.0, 0.5), (2.0, 2.0, 0.5)], (0, 0, 0), (0.5, 0.5, 1)) == 1   # the same with the edge x + y = 1 through it: touching an edge counts
    assert _one([(-5.0, -5.0, 0.5), (5.0, -5.0, 0.5), (0.0, 9.0, 0.5)], lo, hi) == 1              # a huge triangle through the box, no vertex near it
    assert _one([(-5.0, -5.0, 1.5), (5.0, -5.0, 1.5), (0.0, 9.0, 1.5)], (0, 0, 0), (1, 1, 2)) == 1
    assert _one([(-5.0, -5.0, 3.0), (5.0, -5.0, -1.0), (0.0, 9.0, 3.0)], (0, 0, 0), (1, 1, 0.1)) == 0   # own box holds the box; the plane passes above it
    assert _one([(-1.0, 0.5, 0.5), (2.0, 0.5, 0.5), (0.5, 0.5, 0.5)], lo, hi) == 1               # three vertices in line: a segment through the box
    assert _one([(1.0, 1.0, 1.0)] * 3, lo, hi) == 1 and _one([(1.5, 1.0, 1.0)] * 3, lo, hi) == 0  # a point on the corner, a point outside
    assert _one([(0.5, 0.5, 0.5), (2.0, 0.5, 0.5), (0.5, 2.0, 0.5)], (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)) == 1   # lo == hi on a vertex
    assert _one([(0.0, 0.0, 0.5), (2.0, 0.0, 0.5), (0.0, 2.0, 0.5)], (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)) == 1   # lo == hi inside the face
    assert _one([(0.0, 0.0, 0.5), (2.0, 0.0, 0.5), (0.0, 2.0, 0.5)], (0.5, 0.5, 0.75), (0.5, 0.5, 0.75)) == 0  # ... and off it


@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_the_brute_force_against_the_witness(get_scene, name, detail):
    """over the scene's 2048 random boxes and every triangle: wherever the box shrunk by eps overlaps (float64 clipping), the float32 reference says 1; wherever the box
    grown by eps does not, it says 0; and the band between them holds at most 1 % of the overlapping pairs.  eps = 1e-5 times the largest coordinate magnitude"""
    ref = _scene_ref(get_scene, name, detail)
    T, b = ref["T"], ref["b"][N // 2:]
    eps = 1e-5 * float(max(np.abs(T["w"]).max(), np.abs(b[:, [0, 1, 2, 4, 5, 6]]).max()))
    bi, gi = no.pairs(T, b)
    said = np.zeros((b.shape[0], T["v0"].shape[0]), bool)
    said[bi, gi] = True
    lo, hi = b[:, 0:3].astype(np.float64), b[:, 4:7].astype(np.float64)
    near = ((T["lo"].astype(np.float64)[None] <= hi[:, None] + eps) & (lo[:, None] - eps <= T["hi"].astype(np.float64)[None])).all(axis=2)
    assert not (said & ~near).any()   # (the grown box of every other pair misses the triangle's own box: no overlap, and the reference says none)
    ci, cg = np.nonzero(near)
    grown, shrunk = no.witness(T["w"][cg], lo[ci] - eps, hi[ci] + eps), no.witness(T["w"][cg], lo[ci] + eps, hi[ci] - eps)
    s = said[ci, cg]
    assert not (shrunk & ~grown).any()
    assert s[shrunk].all(), f"{int((shrunk & ~s).sum())} pairs overlap by more than eps and the reference says 0"
    assert not s[~grown].any(), f"{int((~grown & s).sum())} pairs are apart by more than eps and the reference says 1"
    band, total = int((grown & ~shrunk).sum()), int(said.sum())
    print(f"\n[overlap] {name}: {ci.size} near pairs, {total} overlapping, {band} in the band ({100.0 * band / total:.3f} %), eps {eps:.3g}")
    assert total > 1000 and band <= 0.01 * total


@pytest.mark.parametrize("name", ["cornell", "sponza_like", "lattice", "clump", "chain", "specials"])
def test_the_comparisons_are_not_vacuous(get_scene, name):
    """from the reference alone: boxes with more than 8 candidates (the list evicts), boxes with none, and boxes whose 8th and 9th candidates sit in different primitives
    (an id pair, not a primitive, is what a record must get right) -- where the scene has more than one primitive"""
    ref = _scene_ref(get_scene, name, 0.05 if name == "sponza_like" else 1.0) if name in ("cornell", "sponza_like") else _hostile(get_scene, name)
    hit, count, ids = ref["want"]
    T, n = ref["T"], ref["b"].shape[0]
    nt = T["v0"].shape[0]
    bi, gi = no.pairs(T, ref["b"])
    first = np.concatenate([[0], np.cumsum(count.astype(np.int64))[:-1]])
    nine = np.flatnonzero(count > 8)
    split = int((T["prim"][gi[first[nine] + 7]] != T["prim"][gi[first[nine] + 8]]).sum())
    print(f"\n[overlap] {name}: {n} boxes, {nt} triangles; more than 8: {nine.size}, none: {int((count == 0).sum())}, 8th and 9th in different primitives: {split}, largest count {int(count.max())}")
    assert np.array_equal(hit, (count > 0).astype(np.uint8)) and np.array_equal(ids[..., 0] >= 0, np.arange(8)[None] < count[:, None])
    assert nine.size >= (10 if name == "cornell" else 50) and (ids[nine, :, 0] >= 0).all()   # (Cornell has 34 triangles: few boxes touch nine of them)
    if name in ("cornell", "sponza_like"):
        assert n == N and int((count == 0).sum()) >= 200 and split >= (1 if name == "cornell" else 10)
    if name == "specials":
        assert count[0] == nt and count[1] == nt and count[2] == 0 and not count[-21:].any() and (count[3:-21] > 0).all()
    if name == "clump":
        assert nt == 1000 and (count[:7] == 1000).all()   # the point itself, as a box, touches all thousand
    if name == "chain":
        assert (count[:64] >= 64 - np.arange(64)).all() and count[-1] == 64   # box k reaches 2^-k: sliver j starts at 2^-j / 2
    if name == "lattice":
        assert n == 216 + 125 + 343 + 3 * 252 and int((count == 0).sum()) > 0


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_both_scenes_are_the_brute_forces(R, torch, get_scene, name, detail):
    """4096 boxes on a side stream, ANY and LIST at K = 1, 4 and 8: hit bytes, counts and ids; a permutation of the boxes gives the permuted answers; oversized out=
    tensors filled with a pattern are untouched beyond n; the queries count neither as casts nor as rays"""
    ref = _scene_ref(get_scene, name, detail)
    b = ref["b"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    s = torch.cuda.Stream()
    for K in KS:
        want = _cut(ref["want"], K)
        _same(_ask_into(r, torch, b, K, 70, f"{name}, K = {K}", stream=s), want, f"{name}, K = {K}")
        _same(_ask(r, torch, b[perm], K), tuple(w[perm] for w in want), f"{name}, K = {K}, permuted")
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", HOSTILE)
def test_hostile_inputs(R, torch, get_scene, which):
    """the lattice with boxes whose faces pass through lattice points (every answer turns on <=); 1000 triangles round one point with boxes round it (a count of 1000,
    stacks past their LDS part); the chain of 64 nested slivers; and on sponza_like one box round the whole scene (its count is T), one that reaches 3.2e38, boxes with
    lo == hi, and the dead boxes -- NaN, +-inf in every coordinate, inverted on every axis: hit 0, count 0, miss records"""
    ref = _hostile(get_scene, which)
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    for K in (8, 3):
        _same(_ask_into(r, torch, ref["b"], K, 3, which), _cut(ref["want"], K), f"{which}, K = {K}")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(tqf.FORMS))
@pytest.mark.parametrize("name", ["clump", "chain", "cornell"])
def test_every_tree_form_gives_the_reference(R, torch, get_scene, name, form):
    """the answers are defined as independent of the structure: the clump, the chain and Cornell's 4096 boxes on every tree form of tests/test_query_forms.py"""
    ref = _scene_ref(get_scene, "cornell", 1.0) if name == "cornell" else _hostile(get_scene, name)
    r = R.renderer_for_scene(ref["scene"], (64, 64), **tqf.FORMS[form])
    for K in (8, 4):
        _same(_ask(r, torch, ref["b"], K), _cut(ref["want"], K), f"{name}, {form}, K = {K}")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [64, 128])
def test_sizes_at_which_a_refill_can_go_wrong(R, torch, get_scene, chunk):
    """ArtTuning.trace_chunk = 64 (a chunk is one filling of a wave) and 128: prefixes of sponza_like's boxes of tests/test_query_forms.py's sizes, then a batch that is
    all dead; every batch into tensors five records too long filled with a pattern.  n = 0 enqueues nothing"""
    ref, K = _scene_ref(get_scene, "sponza_like", 0.05), 8
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning={"trace_chunk": chunk})
    extra = np.concatenate([ref["b"], ref["b"][:1]])   # 4097
    want = tuple(np.concatenate([w, w[:1]]) for w in ref["want"])
    for n in tqf.SIZES:
        before = r.cast_counts()
        _same(_ask_into(r, torch, extra[:n], K, 5, f"n = {n}"), _cut(want, K, n), f"n = {n}")
        if n == 0:
            assert r.cast_counts() == before
    dead = np.tile(dead_boxes(), (7, 1))[:130]
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
    T, K = no.world_triangles(sc.primitives), 8
    b = scene_boxes(T, 5)[1024:3072]
    plain = no.brute_force(T, b, K)
    assert int((plain[2][..., 0] == clear).any(axis=1).sum()) > 20 and int((plain[2][..., 0] == solid).any(axis=1).sum()) > 20
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    _same(_ask(r, torch, b, K), plain, "unmasked")
    m.set_alpha_cutoff(clear, 0.5); m.set_alpha_cutoff(solid, 0.5)
    _same(_ask(r, torch, b, K), plain, "with cutoffs: not tested")
    masks = {0: 0x01, 1: 0x02, solid: 0x03, clear: 0x02}
    for i, v in masks.items():
        m.set_mask(i, v)
    vis = np.array([masks.get(p, 0xFF) for p in range(len(sc.primitives))])
    counts = []
    for cull in (0xFF, 0x01, 0x02, 0x80, 0):
        want = no.brute_force(T, b, K, vis=vis, cull=cull)
        got = _ask(r, torch, b, K, cull_mask=cull)
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
    """two primitives, one disabled after the build: it is in no list and no count, also of a box that reaches 3.2e38 on every side, where its record stands; enabled
    again, the first answers return"""
    sc = tcp._card_scene(scenes, get_scene)
    two = scenes.Scene("two", list(sc.primitives[-2:]), sc.camera, sc.lights)
    T, K = no.world_triangles(two.primitives), 8
    b = np.concatenate([scene_boxes(T, 9)[1536:2560], [_box((-3.2e38,) * 3, (3.2e38,) * 3), _box((-1, -1, -1), (3.2e38,) * 3), _box((2.9e38,) * 3, (3.2e38,) * 3)]]).astype(F)
    r = R.Renderer((64, 64), tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(two.primitives)
    r.prepare_first_frame()
    both = no.brute_force(T, b, K)
    nt = T["v0"].shape[0]
    assert both[1][-3] == nt and both[1][-1] == 0 and {0, 1} <= set(np.unique(both[2][..., 0]).tolist())
    _same(_ask(r, torch, b, K), both, "both")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 0) == 0 and not r.needs_build()
    want = no.brute_force(no.world_triangles(two.primitives, disabled=(1,)), b, K)
    assert not (want[2][..., 0] == 1).any() and want[1][-3] == nt // 2 and want[1][-1] == 0
    got = _ask(r, torch, b, K)
    _same(got, want, "one disabled")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 1) == 0
    _same(_ask(r, torch, b, K), both, "enabled again")
    assert r.stats()["rebuilds"] == 0
    r.close()


@pytest.mark.gpu
def test_the_scene_as_of_the_call(R, torch, get_scene):
    """Cornell's last primitive as a model of its own on a dynamic scene that never rebuilds: after art_scene_set_model_matrix a batch on a side stream, no
    synchronisation in between: each batch is the reference over the triangles as of its call"""
    sc = get_scene("cornell")
    b = _scene_ref(get_scene, "cornell", 1.0)["b"][1024:3072]
    r = R.Renderer((64, 64), dynamic_scene=True, tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(list(sc.primitives[:-1]))
    r.add_model([sc.primitives[-1]])
    r.prepare_first_frame()
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
    m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
    states = [("built", list(sc.primitives)), ("moved", static + [P(moving.verts, moving.indices, moving.tex, m)])]
    d_b = _up(torch, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for what, _ in states:
        if what == "moved":
            r.models_mut()[1].set_model_matrix(m)
        assert not r.needs_build()
        with torch.cuda.stream(s):
            outs.append((r.overlap_boxes(d_b, "any"),) + r.overlap_boxes(d_b, "list", 8)[::-1])
    s.synchronize()
    wants = [no.brute_force(no.world_triangles(prims), b, 8) for _, prims in states]
    for (what, _), got, want in zip(states, outs, wants):
        _same(_host(got), want, what)
    assert not np.array_equal(wants[0][1], wants[1][1])
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 1 and r.cast_counts()["casts"] == 0
    r.close()


@pytest.mark.gpu
def test_voxelize(R, torch, get_scene):
    """an 8^3 grid over Cornell against the reference on the same boxes made in numpy, and on a side stream; neighbours share their faces bit for bit"""
    ref = _scene_ref(get_scene, "cornell", 1.0)
    lo, hi = scene_bounds(ref["T"])
    cell = (hi - lo) / F(8)
    b = grid_boxes(lo, cell, (8, 8, 8))
    assert np.array_equal(b.reshape(8, 8, 8, 8)[1:, :, :, 0], b.reshape(8, 8, 8, 8)[:-1, :, :, 4])
    want = no.brute_force(ref["T"], b, 1)[0].reshape(8, 8, 8)
    assert 0 < int(want.sum()) < 512
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    got = r.voxelize(lo, cell, (8, 8, 8))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    again = r.voxelize(tuple(float(x) for x in lo), cell, (8, 8, 8), stream=s)
    torch.cuda.synchronize()
    assert got.shape == (8, 8, 8) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(again.cpu().numpy(), want)
    assert not r.voxelize(lo, cell, (8, 8, 8), cull_mask=0).any()
    for args in ((lo[:2], cell, (8, 8, 8)), (lo, 0.0, (8, 8, 8)), (lo, cell, (8, 8)), (lo, np.nan, (8, 8, 8))):
        with pytest.raises(ValueError):
            r.voxelize(*args)
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
    boxes = _up(torch, _scene_ref(get_scene, "cornell", 1.0)["b"][:n + 1])
    hit, count, ids = _patterned(torch, n + 1, K)
    torch.cuda.synchronize()

    def lst(**kw):
        d = dict(boxes_dev=boxes.data_ptr(), hit_dev=None, ids_dev=ids.data_ptr(), count_dev=count.data_ptr(), hip_stream=None, n=n, kind=_lib.ART_OVERLAP_LIST, max_hits=K,
                 cull_mask=0xFF, flags=0, reserved=0)
        d.update(kw)
        return _lib.ArtBoxQuery(**d)

    def any_(**kw):
        return lst(**dict(dict(hit_dev=hit.data_ptr(), ids_dev=None, count_dev=None, kind=_lib.ART_OVERLAP_ANY, max_hits=0), **kw))

    def said(d):
        code = L.art_overlap_boxes(ctx, C.byref(d) if d is not None else None)
        return code, L.art_last_error()

    clean = lambda: (hit == 0xA5).all() and (count == PATTERN).all() and (ids == PATTERN).all()   # noqa: E731
    state = WHO + b"scene not built, or changed since the build (art_scene_build)"
    assert said(lst()) == (_lib.ART_E_STATE, state) and said(any_()) == (_lib.ART_E_STATE, state)
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert L.art_overlap_boxes(None, C.byref(lst())) == _lib.ART_E_INVALID and L.art_last_error() == WHO + b"null argument"
    assert said(None) == (_lib.ART_E_INVALID, WHO + b"null argument")
    bad = [(lst(flags=1), b"flags: must be 0"), (any_(flags=0x80000000), b"flags: must be 0"), (lst(reserved=1), b"reserved: must be 0"),
           (lst(kind=2), b"kind: ART_OVERLAP_ANY or ART_OVERLAP_LIST"), (lst(kind=0xFFFFFFFF), b"kind: ART_OVERLAP_ANY or ART_OVERLAP_LIST"),
           (lst(cull_mask=0x100), b"cull_mask: above 0xFF"), (any_(cull_mask=0xFFFFFFFF), b"cull_mask: above 0xFF"),
           (lst(n=_lib.ART_CAST_MAX_RAYS + 1), b"n: above ART_CAST_MAX_RAYS"), (any_(n=0xFFFFFFFF), b"n: above ART_CAST_MAX_RAYS"),
           (lst(boxes_dev=None), b"boxes_dev: null or not 16-byte aligned"), (any_(boxes_dev=boxes.data_ptr() + 8), b"boxes_dev: null or not 16-byte aligned"),
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
    assert said(lst(n=0))[0] == 0 and said(any_(n=0, boxes_dev=None, hit_dev=None))[0] == 0 and said(lst(n=0, boxes_dev=None, ids_dev=None, count_dev=None))[0] == 0
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    # the wrapper's own checks: before anything is enqueued
    for args, kw in (((boxes.cpu(),), {}), ((boxes.double(),), {}), ((boxes[:, :4],), {}), ((boxes, "all"), {}), ((boxes, "list", 0), {}), ((boxes, "list", 9), {}),
                     ((boxes, "list", 2.5), {}), ((boxes,), dict(cull_mask=0x100)), ((boxes, "list", K), dict(out=(ids[:8], count))),
                     ((boxes, "list", K), dict(out=(ids, count.to(torch.int64)))), ((boxes, "list", K + 1), dict(out=(ids, count))), ((boxes, "any"), dict(out=hit[:8]))):
        with pytest.raises((ValueError, TypeError)):
            r.overlap_boxes(*args, **kw)
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
        r.overlap_boxes(boxes)
    r.close()
