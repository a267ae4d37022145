"""The 4-wide tree (art_wide.hip's collapse, art_records.h's wide_quantise, art_refit.hip's refit and cost) against tests/np_wide.py, bit for bit.  Every walk's parity
test passes for ANY tree whose boxes contain what is below them: a refit that leaves a masked primitive's extent in the boxes above it, a quantiser one step too far out,
a collapse that breaks ties the other way only move the ray rate.  The records are deterministic, so they can be restated and compared with no tolerance -- at the build,
and after every step of a sequence of moves, deformations and residency switches, where until now they were only probed by rays.

Without a device: (a) the model's records are a valid tree whose child boxes are the binary tree's; the dequantised planes are, IN VALUES, the tightest of the 256 a node
can represent (an index one step inwards may decode to the same float: index tightness is the wrong property) and the exponent the smallest allowed; refit() of the built
records over the built leaves gives them back, over moved leaves and with a primitive nowhere every box is the brute-force union of what is left below it; cost() is a
plain sum over a brute-force box list; (b) every mutated model (np_wide.MUTANTS) gives other arrays on at least one case; (c) which rules the cases reach is printed.
On the device: (d) both record arrays of the build -- SAH tree and LBVH topology, device and host collapse, first and second build -- are the model's; (e) after every
step of the sequences below, in every form of the refit, records, leaf boxes and the cost ratio are the model's; (f) the same after a rebuild by the cost rule.

What the cases do not reach, and why.  No scene of the table takes the quantiser's `e++` loop or its plane guards: 255 * s >= top - origin holds exactly for the first
exponent tried and rounding is monotone, so fma(255, s, origin) >= top follows -- unless the float64 difference top - origin itself rounded DOWN, which needs an
origin and a top whose binary places are more than 53 apart.  "exponent steps" is built to do that (an origin of -255 and a top of 2^-60 on x; a lo of -2^-60 under an
origin of -255 on y; a hi of 2^-60 over an origin of -254 on z) and reaches all three; nothing asserts that another case does.
The mutant "round for floor" is the one no case can tell apart, and the test asserts exactly that (as tests/test_sah_tree.py does for "kMid 2048"): rounding the first
guess of a lo plane up gives floor + 1, whose value is either above the float lo -- then the outward guard steps back to floor -- or at most lo: then the exact
origin + (floor + 1) * s, which is above lo, was rounded down onto lo, the largest value a plane at or under lo can have, and the inward step of the rule goes there from
floor as well (where neighbouring planes decode to the SAME float the quotient is an integer: s is then below the ulp of origin and of lo, which are multiples of it).
Before the inward step existed the mutant differed from the rule on exactly those planes -- 1 of 53 000 of "flat 6000", 16 of "chain 64" -- and was the tighter of the two:
that is the looseness this file found in wide_quantise (profiles/README.md, "The 4-wide tree against a numpy model").  "no plane guards" stands in for it.
Left out of the bit-for-bit comparison on the device: "clusters 20000" (a soup of more than 9 000 triangles: the model's seconds), on the CPU it is in."""
import collections
import math
import time

import numpy as np
import pytest

import np_sah
import np_wide
import test_sah_tree as sah
from helpers import R, SIMILARITIES, chain_scene, degenerate_soup, dequantise, lattice_scene, oracle_for, similarity  # noqa: F401  (R: a module fixture)

ABSENT = np_wide.ABSENT
NOWHERE = np_wide.NOWHERE


def _box_tri(lo, hi):
    return (tuple(lo), tuple(hi), (lo[0], hi[1], lo[2]))


def exponent_steps():
    """three triangles whose boxes make the root's quantiser take its e++ loop (x), its lo guard (y) and its hi guard (z): the module docstring"""
    t = 2.0 ** -60
    return sah._tri_scene("exponent steps", [_box_tri((-255.0, -255.0, -254.0), (-254.0, -254.0, -253.0)), _box_tri((-1.0, -t, -1.0), (t, 0.0, t)), _box_tri((-2.0, -2.0, 0.0), (-1.0, -1.0, 1.0))])


CASES = {k: v[0] for k, v in sah.CASES.items() if k not in sah.LARGE}
CASES.update({"lattice": lattice_scene, "chain 64": lambda: chain_scene(64)[0], "exponent steps": exponent_steps})
CASES.update({f"soup 1000 x {s:g} + {off}": (lambda s=s, off=off: similarity(degenerate_soup(1000, "soup"), None, s=s, offset=off)[0]) for s, off in SIMILARITIES})
CASES["soup 300 x 2^-10 + (1000.3, -2000.7, 500.1)"] = lambda: similarity(degenerate_soup(300, "soup"), None, s=2.0 ** -10, offset=SIMILARITIES[-1][1])[0]   # a scale under the coordinates' ulp: neighbouring planes decode to the same float
CASES.update({f"soup {T}": (lambda T=T: degenerate_soup(T, "soup")) for T in (1, 2, 4, 5)})
KINDS = ("sah", "lbvh")
ON_DEVICE = [k for k in CASES if k != "clusters 20000"]
HOST_COLLAPSE = ("soup 1", "soup 3", "soup 300", "cornell", "sponza_like 0.12", "lattice", "exponent steps")
_scene_cache, _built_cache = {}, {}


def _scene(key, orc):
    """the scene, the oracle's canonical LBVH over it (63-bit keys: the device's default leaf order), np_sah's tree over those leaves (None under 3 leaves) -- made once"""
    if key in sah.CASES:
        return sah._case(key, orc)
    if key not in _scene_cache:
        sc = CASES[key]()
        lb = oracle_for(orc, sc, morton_bits=63)[0].lbvh()
        _scene_cache[key] = (sc, lb, np_sah.build(lb["leaf_lo"], lb["leaf_hi"]))
    return _scene_cache[key]


def _binary(key, kind, orc):
    sc, lb, tree = _scene(key, orc)
    if kind == "sah" and tree is not None:
        return tree.child, tree.node_lo, tree.node_hi
    return lb["child"], lb["node_lo"], lb["node_hi"]       # (under 3 leaves the library builds no tree of its own either)


class Built:
    def __init__(self, binary, lb):
        t0 = time.perf_counter()
        before = collections.Counter(np_wide.COUNTS)
        self.binary = binary
        self.f, self.levels, self.axis = np_wide.collapse(*binary, lb["leaf_lo"], lb["leaf_hi"])
        self.q = np_wide.quantise(self.f)
        self.seconds = time.perf_counter() - t0
        self.reach = collections.Counter(np_wide.COUNTS)
        self.reach.subtract(before)


def _built(key, kind, orc):
    if (key, kind) not in _built_cache:
        _built_cache[(key, kind)] = Built(_binary(key, kind, orc), _scene(key, orc)[1])
    return _built_cache[(key, kind)]


def _leaves_below(child):
    """per node and child slot the leaf positions below it, by brute force (lists of arrays)"""
    n = child.shape[0]
    out = [[None] * 4 for _ in range(n)]
    for w in range(n - 1, -1, -1):
        for i in range(4):
            c = int(child[w, i])
            if c == ABSENT:
                out[w][i] = np.zeros(0, np.int64)
            elif c < 0:
                out[w][i] = np.array([~c], np.int64)
            else:
                out[w][i] = np.concatenate(out[c])
    return out


def _brute_boxes(child, leaf_lo, leaf_hi):
    """per node and child slot the exact union of the leaves below that are not nowhere; nothing left (or an absent child): the point at 3e38"""
    below = _leaves_below(child)
    n = child.shape[0]
    lo, hi = np.full((n, 4, 3), NOWHERE, np.float32), np.full((n, 4, 3), NOWHERE, np.float32)
    for w in range(n):
        for i in range(4):
            p = below[w][i]
            p = p[leaf_lo[p, 0] < NOWHERE]
            if p.size:
                lo[w, i], hi[w, i] = leaf_lo[p].min(0), leaf_hi[p].max(0)
    return lo, hi, below


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- without a device ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", list(CASES))
def test_model_records_are_a_valid_tree_of_the_binary_trees_boxes(orc, key, kind):
    """(a) validity: every leaf once, every node but the root one parent, levels contiguous, child boxes = the boxes of the binary nodes (or leaves) they stand on"""
    sc, lb, _ = _scene(key, orc)
    B = _built(key, kind, orc)
    bchild, nlo, nhi = B.binary
    lo, hi, child = np_wide.parts(B.f)
    T, n = sc.n_tris, child.shape[0]
    leaves = child[(child < 0) & (child != ABSENT)]
    assert np.array_equal(np.sort(~leaves), np.arange(T))
    assert np.array_equal(np.sort(child[child >= 0]), np.arange(1, n))
    assert np.array_equal(np_wide.level_offsets(child), B.levels) and B.levels[-1] == n
    nc = (child != ABSENT).sum(1)
    assert np.array_equal(child != ABSENT, np.arange(4)[None, :] < nc[:, None])                          # the valid children are slots 0 .. nc - 1
    assert np.array_equal(B.f[:, 28], (1 << nc) - 1) and np.array_equal(B.f[:, 29], B.axis) and not B.f[:, 30:].any() and B.axis.max() <= 2
    assert (nc == 4).all() or T < 4 or (nc[nc < 4] >= 2).all()
    # what each wide node stands on: the binary node with the same SET of leaves (a random 64-bit weight per leaf, summed with wrap-around)
    wgt = np.random.default_rng(1).integers(1, 2 ** 62, T).astype(np.uint64)
    NI = T - 1
    bsig = np.zeros(max(NI, 0), np.uint64)
    for b in (_post_order(bchild) if NI > 0 else []):
        bsig[b] = np.uint64(sum(int(wgt[~c]) if c < 0 else int(bsig[c]) for c in bchild[b].tolist()) % 2 ** 64)
    node_of = {int(s): b for b, s in enumerate(bsig.tolist())}
    assert len(node_of) == max(NI, 0)
    wsig = np.zeros(n, np.uint64)
    for w in range(n - 1, -1, -1):
        wsig[w] = np.uint64(sum(int(wgt[~c]) if c < 0 else int(wsig[c]) for c in child[w].tolist() if c != ABSENT) % 2 ** 64)
    for w in range(n):
        for i in range(4):
            c = int(child[w, i])
            if c == ABSENT:
                assert lo[w, i].view(np.uint32).tolist() == [NOWHERE.view(np.uint32)] * 3 and _same_bits(lo[w, i], hi[w, i])
            elif c < 0:
                assert _same_bits(lo[w, i], lb["leaf_lo"][~c]) and _same_bits(hi[w, i], lb["leaf_hi"][~c]), (w, i)
            else:
                b = node_of.get(int(wsig[c]))
                assert b is not None, f"wide node {c} stands on no binary node"
                assert _same_bits(lo[w, i], nlo[b]) and _same_bits(hi[w, i], nhi[b]), (w, i, b)
    if NI > 0:
        assert node_of.get(int(wsig[0])) == 0


def _post_order(bchild):
    """binary nodes, children before parents (node 0 is the root; any numbering)"""
    order, stack = [], [0]
    while stack:
        b = stack.pop()
        order.append(b)
        stack += [c for c in bchild[b].tolist() if c >= 0]
    return order[::-1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", list(CASES))
def test_quantised_planes_are_the_tightest_values_and_the_exponent_the_smallest(orc, key, kind):
    """(a) containment and tightness in VALUES: of the 256 planes origin + q * s a node can represent (as the walks' fma evaluates them) a child's lo plane is the largest
    that is at most its float lo, its hi plane the smallest that is at least its float hi; the exponent is -100 or one less no longer reaches the top"""
    B = _built(key, kind, orc)
    lo, hi, child = np_wide.parts(B.f)
    dlo, dhi, valid, planes = dequantise(B.q)
    present = child != ABSENT
    assert np.array_equal(valid, present) and np.array_equal(B.q[:, 12:16].view(np.int32), child) and not B.q[:, 10:12].any()
    live = present & (lo[:, :, 0] < NOWHERE)
    assert (planes[~live][:, :3] == 255).all() and (planes[~live][:, 3:] == 0).all()
    org = B.q[:, 0:3].view(np.float32)
    e = np.stack([(B.q[:, 3] >> (8 * k)) & 255 for k in range(3)], 1).astype(np.int64) - 127
    vals = np_wide._fma(np.arange(256.0)[None, None, :], np.ldexp(1.0, e)[:, :, None], org[:, :, None])            # [n, 3, 256], non-decreasing in the plane
    assert (np.diff(vals, axis=2) >= 0).all()
    with np.errstate(all="ignore"):
        best_lo = np.where(vals[:, None] <= lo[..., None], vals[:, None], np.float32(-np.inf)).max(3)               # [n, 4, 3]
        best_hi = np.where(vals[:, None] >= hi[..., None], vals[:, None], np.float32(np.inf)).min(3)
    assert (dlo[live] <= lo[live]).all() and (dhi[live] >= hi[live]).all()                                          # containment
    assert np.array_equal(dlo[live], best_lo[live]), f"{int((dlo[live] != best_lo[live]).sum())} lo planes are not the tightest value"
    assert np.array_equal(dhi[live], best_hi[live]), f"{int((dhi[live] != best_hi[live]).sum())} hi planes are not the tightest value"
    top = np.where(live[:, :, None], hi, np.float32(-np.inf)).max(1)
    assert (e >= np_wide.MIN_EXP).all()
    smaller_fails = np_wide._fma(255.0, np.ldexp(1.0, e - 1), org) < top
    assert ((e == np_wide.MIN_EXP) | smaller_fails | ~live.any(1)[:, None]).all()


def _moved(lb, seed):
    """other leaves over the same topology: a third of them carried away by a few offsets, some scaled about their corner"""
    rng = np.random.default_rng(seed)
    lo, hi = lb["leaf_lo"].copy(), lb["leaf_hi"].copy()
    T = lo.shape[0]
    pick = rng.random(T) < 0.34
    off = rng.uniform(-0.7, 0.7, (T, 3)).astype(np.float32)
    lo[pick] += off[pick]; hi[pick] += off[pick]
    grow = rng.random(T) < 0.1
    hi[grow] = (lo[grow] + (hi[grow] - lo[grow]) * np.float32(1.5)).astype(np.float32)
    return lo, hi


def _prim_of_leaf(sc, lb):
    return np.repeat(np.arange(len(sc.primitives)), [p.n_tris for p in sc.primitives])[lb["leaf_gid"].astype(np.int64)]


def _without(sc, lb, out):
    """the leaf boxes with the leaves chosen by the mask `out` nowhere"""
    lo, hi = lb["leaf_lo"].copy(), lb["leaf_hi"].copy()
    lo[out], hi[out] = NOWHERE, NOWHERE
    return lo, hi


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", list(CASES))
def test_refit_over_the_built_leaves_gives_the_built_records(orc, key, kind):
    """(a)"""
    lb, B = _scene(key, orc)[1], _built(key, kind, orc)
    assert np_wide.first_difference(np_wide.refit(B.f, lb["leaf_lo"], lb["leaf_hi"]), B.f, key) is None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", ["soup 5", "cornell", "soup 300", "lattice"])
def test_refit_over_moved_leaves_is_the_brute_force_union(orc, key, kind):
    """(a) every child box is the union of the new leaves below it, node by node; so is the cost a plain sum over that box list"""
    lb, B = _scene(key, orc)[1], _built(key, kind, orc)
    llo, lhi = _moved(lb, 5)
    f = np_wide.refit(B.f, llo, lhi)
    lo, hi, child = np_wide.parts(f)
    blo, bhi, _ = _brute_boxes(child, llo, lhi)
    assert _same_bits(lo, blo) and _same_bits(hi, bhi)
    assert np.array_equal(f[:, 24:], B.f[:, 24:]) and not np.array_equal(f, B.f)


def _big_primitive(sc):
    return int(np.argmax([p.n_tris for p in sc.primitives]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", ["cornell", "sponza_like 0.12"])
def test_refit_with_a_primitive_nowhere_leaves_nothing_of_it(orc, key, kind):
    """(a) the scene's largest primitive out: every box is the union of what is left below it, the quantised records carry the inverted box where nothing is, and
    (sponza_like: 2 560 of 8 048 triangles) at least one node has every child nowhere"""
    sc, lb, _ = _scene(key, orc)
    B = _built(key, kind, orc)
    out = _prim_of_leaf(sc, lb) == _big_primitive(sc)
    llo, lhi = _without(sc, lb, out)
    f = np_wide.refit(B.f, llo, lhi)
    lo, hi, child = np_wide.parts(f)
    blo, bhi, below = _brute_boxes(child, llo, lhi)
    assert _same_bits(lo, blo) and _same_bits(hi, bhi)
    present = child != ABSENT
    gone = np.array([[present[w, i] and out[below[w][i]].all() for i in range(4)] for w in range(child.shape[0])])
    assert np.array_equal(gone, present & (lo[:, :, 0] >= NOWHERE)) and gone.any()
    kept = lb["leaf_lo"][~out].min(0), lb["leaf_hi"][~out].max(0)
    live = present & ~gone
    assert (lo[live] >= kept[0]).all() and (hi[live] <= kept[1]).all()
    all_gone = (gone | ~present).all(1)
    if key != "cornell":
        assert all_gone.any(), "no node with every child nowhere"
    counts = collections.Counter()
    q = np_wide.quantise(f, counts=counts)
    assert counts["nowhere children"] == int(gone.sum()) and counts["all-nowhere nodes"] == int(all_gone.sum())
    _, _, _, planes = dequantise(q)
    assert (planes[gone][:, :3] == 255).all() and (planes[gone][:, 3:] == 0).all()
    assert not q[all_gone, 0:3].any() and (q[all_gone, 3] & 0xFFFFFF == 27 * 0x010101).all()      # origin 0, 2^-100 on every axis


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", ["soup 5", "cornell", "soup 300", "sponza_like 0.12"])
def test_cost_is_the_plain_sum_over_a_brute_force_box_list(orc, key, kind):
    """(a) as built and with the largest primitive (or a third of the leaves) nowhere.  Both sides sum the same non-negative float64 terms, one pairwise and one exactly
    (math.fsum): a pairwise sum of n <= 2^14 terms is within 14 * 2^-53 < 2e-15 of the exact one, relatively"""
    sc, lb, _ = _scene(key, orc)
    B = _built(key, kind, orc)
    out = _prim_of_leaf(sc, lb) == _big_primitive(sc) if len(sc.primitives) > 1 else np.arange(sc.n_tris) % 3 == 0
    for f, (llo, lhi) in ((B.f, (lb["leaf_lo"], lb["leaf_hi"])), (np_wide.refit(B.f, *_without(sc, lb, out)), _without(sc, lb, out))):
        _, _, child = np_wide.parts(f)
        blo, bhi, below = _brute_boxes(child, llo, lhi)
        terms, rlo, rhi = [], [], []
        for w in range(child.shape[0]):
            for i in range(4):
                if child[w, i] != ABSENT and blo[w, i, 0] < NOWHERE:
                    d = [float(bhi[w, i, k]) - float(blo[w, i, k]) for k in range(3)]
                    terms.append(d[0] * d[1] + d[1] * d[2] + d[2] * d[0])
                    if w == 0:
                        rlo.append(blo[w, i]); rhi.append(bhi[w, i])
        d = (np.max(rhi, 0).astype(np.float64) - np.min(rlo, 0).astype(np.float64)).tolist()
        total, root = np_wide.cost(f)
        want = math.fsum(terms)
        assert abs(total - want) <= 2e-15 * want and root == d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
        assert len(terms) <= 2 ** 14


def _everything(key, kind, orc, mutant):
    """every array the model makes for a case: the built records, the records with a primitive (or a third of the leaves) nowhere, the two costs"""
    sc, lb, _ = _scene(key, orc)
    f, _, _ = np_wide.collapse(*_binary(key, kind, orc), lb["leaf_lo"], lb["leaf_hi"], mutant=mutant) if mutant else (_built(key, kind, orc).f, None, None)
    out = _prim_of_leaf(sc, lb) == _big_primitive(sc) if len(sc.primitives) > 1 else np.arange(sc.n_tris) % 3 == 0
    g = np_wide.refit(f, *_without(sc, lb, out), mutant=mutant)
    return [f, np_wide.quantise(f, mutant=mutant), g, np_wide.quantise(g, mutant=mutant), np.array(np_wide.cost(f, mutant=mutant) + np_wide.cost(g, mutant=mutant))]


MUTANT_CASES = ("soup 5", "soup 16", "soup 40", "cornell", "lattice", "chain 64", "soup 300", "subnormal specks 12", "row 70", "exponent steps", "sponza_like 0.12") + tuple(k for k in CASES if k.startswith("soup 1000 x") or k.startswith("soup 300 x")) + ("line 6000",)
_right = {}


@pytest.mark.parametrize("mutant", np_wide.MUTANTS)
def test_cases_tell_a_mutated_model_apart(orc, mutant):
    """(b)"""
    told = []
    for key in MUTANT_CASES:
        for kind in KINDS:
            if (key, kind) not in _right:
                _right[(key, kind)] = _everything(key, kind, orc, None)
            other = _everything(key, kind, orc, mutant)
            if not all(np.array_equal(a, b) for a, b in zip(other, _right[(key, kind)])):
                told.append(f"{key} ({kind})")
    if mutant == "round for floor":   # (the module docstring: behind the guards the rounding of the first guess cannot show)
        assert not told, f"'{mutant}': other arrays on {told}"
        return
    assert told, f"no case tells '{mutant}' from the model"
    print(f"\n[wide mutant] '{mutant}' is told apart by {told}")


def test_which_rules_the_cases_reach(orc):
    """(c) printed, not required (the module docstring says what only "exponent steps" reaches); the refit states' nowhere children are counted with the largest primitive out"""
    total = collections.Counter()
    print("\n[wide reach] case | T | wide nodes | levels | batches | crown | model seconds | " + " | ".join(np_wide.REACH))
    for key in CASES:
        sc, lb, _ = _scene(key, orc)
        for kind in KINDS:
            B = _built(key, kind, orc)
            reach = collections.Counter(B.reach)
            if len(sc.primitives) > 1:
                np_wide.quantise(np_wide.refit(B.f, *_without(sc, lb, _prim_of_leaf(sc, lb) == _big_primitive(sc))), counts=reach)
            bt = np_wide.batches(B.f)
            total.update(reach)
            print(f"[wide reach] {key} ({kind}) | {sc.n_tris} | {B.f.shape[0]} | {len(B.levels) - 1} | {bt['n_batches']} | {bt['crown']} | {B.seconds:.2f} | " + " | ".join(str(reach[k]) for k in np_wide.REACH))
    print("[wide reach] all | | | | | | | " + " | ".join(str(total[k]) for k in np_wide.REACH))
    for k in ("area ties", "axis ties", "nodes with 1 child", "nodes with 2 children", "nodes with 3 children", "2^-100 axes", "nowhere children", "all-nowhere nodes"):
        assert total[k] > 0, k


def test_batches_of_the_mid_scene(orc):
    """the partition rule on the scene the refit tests use, as one model: at least 3 batches and a crown, every node in the crown or in one batch with its whole subtree"""
    B = _built("sponza_like 0.12", "sah", orc)
    bt = np_wide.batches(B.f)
    assert bt["n_batches"] >= 3 and bt["crown"] > 0 and bt["crown"] + bt["batch_nodes"].sum() == B.f.shape[0]
    assert (bt["batch_nodes"] <= np_wide.BATCH_NODES * 3 // 2).all() and bt["batch_of"][0] == -1
    inner = np.arange(1, B.f.shape[0])
    in_batch = bt["batch_of"][inner] >= 0
    up = bt["parent"][inner]
    assert (bt["batch_of"][up[~in_batch]] == -1).all()                                         # the crown is closed upwards
    same_or_root = (bt["batch_of"][up[in_batch]] == bt["batch_of"][inner[in_batch]]) | (bt["size"][up[in_batch]] > np_wide.BATCH_NODES)
    assert same_or_root.all() and (bt["size"][inner[in_batch]] <= np_wide.BATCH_NODES).all()
    small = np_wide.batches(_built("cornell", "sah", orc).f)
    assert small["n_batches"] == 0 and small["crown"] == _built("cornell", "sah", orc).f.shape[0]


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------------
def _model_of_device(r, key, kind, orc):
    """the model's records over the DEVICE's binary tree and leaves (art_get_traversal_tree, art_get_lbvh) -- the cached ones where those are the CPU case's, bit for bit"""
    lb, tr = r.get_lbvh(), r.get_traversal_tree()
    if key is not None:
        B, olb = _built(key, kind, orc), _scene(key, orc)[1]
        T = olb["leaf_lo"].shape[0]
        if lb["leaf_lo"].shape[0] == T and np.array_equal(tr["child"], B.binary[0][:max(T - 1, 0)]) and all(_same_bits(lb[k], olb[k]) for k in ("leaf_lo", "leaf_hi")) \
                and _same_bits(tr["node_lo"], B.binary[1][:max(T - 1, 0)]) and _same_bits(tr["node_hi"], B.binary[2][:max(T - 1, 0)]):
            return B.f, B.q, lb
    f, _, _ = np_wide.collapse(tr["child"], tr["node_lo"], tr["node_hi"], lb["leaf_lo"], lb["leaf_hi"])
    return f, np_wide.quantise(f), lb


def _assert_records(r, f, q, what):
    dq, df = r.get_wide_nodes()
    diff = np_wide.first_difference(df, f, what + ", float records") or np_wide.first_difference(dq, q, what + ", quantised records")
    assert diff is None, diff
    return dq, df


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", ON_DEVICE)
def test_device_records_of_a_build_are_the_models(R, orc, key, kind):
    """(d) the default SAH tree and the LBVH topology (fast_build), the device collapse: the first build, and a second one in the same context"""
    r = R.renderer_for_scene(_scene(key, orc)[0], (64, 48), fast_build=kind == "lbvh")
    f, q, _ = _model_of_device(r, key, kind, orc)
    _assert_records(r, f, q, f"{key} ({kind}), first build")
    r.prepare_first_frame()
    f, q, _ = _model_of_device(r, key, kind, orc)
    _assert_records(r, f, q, f"{key} ({kind}), second build in the same context")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", HOST_COLLAPSE)
def test_host_collapse_records_are_the_models(R, orc, key):
    """(d) ArtTuning.wide_builder = 1: the one-thread host loop"""
    r = R.renderer_for_scene(_scene(key, orc)[0], (64, 48), tuning={"wide_builder": 1})
    f, q, _ = _model_of_device(r, key, "sah", orc)
    _assert_records(r, f, q, f"{key}, host collapse")
    r.close()


class Driven:
    """a scene as one model per group of primitives on a renderer, and the same state in numpy: positions, matrices, who is enabled"""

    def __init__(self, R, sc, groups, tuning, lights=()):
        self.r = r = R.Renderer((64, 48), tuning=tuning)
        self.prims = []                                     # device primitive order: [positions, indices, matrix, enabled]
        for g in groups:
            r.add_model([sc.primitives[j] for j in g])
            self.prims += [[np.array(sc.primitives[j].verts, np.float32), sc.primitives[j].indices, np.array(sc.primitives[j].model, np.float32).reshape(3, 4), True] for j in g]
        self.first = np.cumsum([0] + [len(g) for g in groups])   # a model's first primitive id
        cam = r.camera_mut()
        cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
        for d in lights:
            r.lights_mut().push_dict(d)
        r.prepare_first_frame()
        self.step_no = 0

    def built(self, orc):
        self.f0, self.q0, lb = _model_of_device(self.r, None, None, orc)
        self.leaf_gid = lb["leaf_gid"]
        self.cost0 = np_wide.cost(self.f0)[0]
        self.leaf_prim = np.repeat(np.arange(len(self.prims)), [np.asarray(p[1]).size // 3 for p in self.prims])[self.leaf_gid.astype(np.int64)]
        _assert_records(self.r, self.f0, self.q0, "as built")
        llo, lhi = np_wide.leaf_boxes(self.prims, self.leaf_gid)
        assert _same_bits(llo, lb["leaf_lo"]) and _same_bits(lhi, lb["leaf_hi"]), "the numpy leaf boxes are not the build's"
        return self

    def move(self, model, m):
        self.r.models_mut()[model].set_model_matrix(m)
        for p in range(self.first[model], self.first[model + 1]):
            self.prims[p][2] = np.array(m, np.float32).reshape(3, 4)

    def set_vertices(self, model, verts):
        self.r.models_mut()[model].set_vertices(0, verts)
        self.prims[self.first[model]][0] = np.array(verts, np.float32)

    def enable(self, model, on, which=None):
        from araytracingjourney_amd._lib import check
        for p in range(self.first[model], self.first[model + 1]) if which is None else [which]:
            check(self.r._L.art_scene_set_primitive_enabled(self.r._ctx, int(p), 1 if on else 0))
            self.prims[p][3] = bool(on)
        assert not self.r.needs_build()

    def check(self, what):
        """after a step: both record arrays, the leaf boxes and the cost ratio are the model's for this state; reached through a frame on even steps, by the getter's
        own refresh on odd ones"""
        r = self.r
        if self.step_no % 2 == 0:
            r.render_frame()
        self.step_no += 1
        llo, lhi = np_wide.leaf_boxes(self.prims, self.leaf_gid)
        f = np_wide.refit(self.f0, llo, lhi)
        dq, df = _assert_records(r, f, np_wide.quantise(f), what)
        lb = r.get_lbvh()
        assert _same_bits(lb["leaf_lo"], llo) and _same_bits(lb["leaf_hi"], lhi), what + ": leaf boxes"
        r.sync()
        got, want = np.float32(r.stats()["refit_cost_ratio"]), np.float32(np_wide.cost(f)[0] / self.cost0)
        print(f"[wide refit] {what}: cost ratio {got!r}, the model's {want!r}")
        assert abs(np.float64(got) - np.float64(want)) <= np.spacing(want), f"{what}: cost ratio {got!r}, the model's {want!r}"
        return dq, df, got


def _pose(base, i):
    """the base matrix turned about y and carried along a small loop (float32 3x4, row-major)"""
    a = 0.17 * i
    t = np.array([[math.cos(a), 0, math.sin(a), 0.2 * math.sin(0.5 * i)], [0, 1, 0, 0.06 * i], [-math.sin(a), 0, math.cos(a), 0.15 * math.cos(0.4 * i) - 0.15], [0, 0, 0, 1]])
    return np.ascontiguousarray((t @ np.vstack([np.asarray(base, np.float64).reshape(3, 4), [0, 0, 0, 1]]))[:3], np.float32)


def _bent(verts, k):
    v = np.array(verts, np.float32)
    v[:, 0:3] = (v[:, 0:3] * np.float32(1.0 + 0.05 * k) + np.float32(0.03) * np.sin(v[:, [1, 2, 0]] * np.float32(3.0 + k))).astype(np.float32)
    return v


FORMS = {"presets": {}, "fold": {"refit_fold_nodes": 1}, "1 version": {"as_versions": 1}, "2 versions": {"as_versions": 2}, "3 versions": {"as_versions": 3},
         "fold, 2 versions": {"refit_fold_nodes": 1, "as_versions": 2}, "no refit streams": {"refit_streams": 0xFFFFFFFF}}
MOVER_IDS = range(12, 24)
_movers = {}


def _mid_scene_in_three(R, scenes, sc, a, b, tuning):
    rest = [j for j in range(len(sc.primitives)) if j not in (a, b)]
    return Driven(R, sc, [rest, [a], [b]], dict(tuning, refit_rebuild_ratio=-1.0), scenes.sponza_lights(1))


def _partition_ok(D):
    """the preconditions of the refit sequence on the context's own records: at least 3 batches, a crown, each mover's leaves in a strict subset of the batches, the two
    movers' batch sets disjoint"""
    bt = np_wide.batches(D.f0)
    pa, pb = D.first[1], D.first[2]
    sa, sb = set(bt["leaf_batch"][D.leaf_prim == pa].tolist()) - {-1}, set(bt["leaf_batch"][D.leaf_prim == pb].tolist()) - {-1}
    return bt["n_batches"] >= 3 and bt["crown"] > 0 and 0 < len(sa) < bt["n_batches"] and 0 < len(sb) < bt["n_batches"] and not (sa & sb), (bt, sa, sb)


def _choose_movers(R, orc, scenes, sc):
    """two of the 50-triangle primitives 12 .. 23 whose leaves lie in different batches of the tree built with them as models of their own (splitting the scene into
    models renumbers the triangles, so the partition is derived from the records of such a build, never assumed)"""
    if "ab" not in _movers:
        for a in MOVER_IDS:
            for b in MOVER_IDS:
                if a < b and "ab" not in _movers:
                    D = _mid_scene_in_three(R, scenes, sc, a, b, {}).built(orc)
                    if _partition_ok(D)[0]:
                        _movers["ab"] = (a, b)
                    D.r.close()
    assert "ab" in _movers, "no pair of the small primitives lies in disjoint batches"
    return _movers["ab"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_refit_states_are_the_models(R, orc, get_scene, scenes, form):
    """(e) sponza_like 0.12 as three models -- the rest, and two 50-triangle primitives A and B in disjoint batches -- through moves, a frame with no change, a
    deformation, B out / moved while out / back, the 2 560-triangle primitive out and back, and home again: after EVERY step both record arrays are refit + quantise of the
    built records over that state's leaf boxes, the leaf boxes are numpy's, and the cost ratio is float32(cost(now) / cost(built)) within one float32 ulp (both sides are
    float64 sums of at most about 16 000 non-negative terms in different orders: they differ by less than 1e-11 relatively, far under 2^-24, so only the last rounding can)"""
    sc = get_scene("sponza_like", 0.12)
    assert all(sc.primitives[j].n_tris == 50 for j in MOVER_IDS)
    a, b = _choose_movers(R, orc, scenes, sc)
    D = _mid_scene_in_three(R, scenes, sc, a, b, FORMS[form]).built(orc)
    ok, (bt, sa, sb) = _partition_ok(D)
    assert ok, (bt["n_batches"], bt["crown"], sa, sb)
    print(f"\n[wide refit] {form}: movers {a}, {b}; {D.f0.shape[0]} nodes, batches of {bt['batch_nodes'].tolist()} nodes, a crown of {bt['crown']}; A in {sorted(sa)}, B in {sorted(sb)}")
    A, B = 1, 2
    base_a, base_b, verts_a = D.prims[D.first[A]][2].copy(), D.prims[D.first[B]][2].copy(), D.prims[D.first[A]][0].copy()
    big = _big_primitive(sc)
    assert sc.primitives[big].n_tris == 2560 and big not in (a, b)
    big_id = [j for j in range(len(sc.primitives)) if j not in (a, b)].index(big)
    r = D.r
    r.render_frame()
    D.move(A, _pose(base_a, 1)); D.check("A moved")
    D.move(B, _pose(base_b, 2)); D.check("B moved")
    D.move(A, _pose(base_a, 3)); D.move(B, _pose(base_b, 4)); D.check("both moved")
    D.step_no = 0; _, _, ratio = D.check("a frame with no change")
    D.set_vertices(A, _bent(verts_a, 1)); D.check("A's vertices replaced")
    D.enable(B, False); D.check("B out")
    D.move(B, _pose(base_b, 6)); D.check("B moved while it is out")
    D.enable(B, True); D.check("B back")
    D.enable(0, False, which=big_id); dq, df, _ = D.check("the 2 560-triangle primitive out")
    lo, _, child = np_wide.parts(df)
    assert (((lo[:, :, 0] >= NOWHERE) | (child == ABSENT)).all(1)).any(), "no node with every child nowhere"
    D.move(A, _pose(base_a, 7)); D.check("A moved with the large primitive out")
    D.enable(0, True, which=big_id); D.check("the large primitive back")
    D.move(B, _pose(base_b, 9)); D.set_vertices(A, _bent(verts_a, 2)); D.check("B moved, A's vertices replaced again")
    D.set_vertices(A, verts_a); D.move(A, base_a); D.move(B, base_b)
    dq, df, ratio = D.check("home again")
    assert ratio == np.float32(1.0) and np.array_equal(df, D.f0) and np.array_equal(dq, D.q0)
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] == 11     # (every step but two: the frame with no change, and B moved while it is out -- nothing to show)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["presets", "fold, 2 versions"])
def test_refit_states_of_an_all_crown_tree(R, orc, scenes, form):
    """(e) the Cornell box, one model per primitive: a tree of a dozen nodes has no batch, the crown's workgroup does everything"""
    sc = scenes.cornell()
    D = Driven(R, sc, [[0], [1], [2]], dict(FORMS[form], refit_rebuild_ratio=-1.0), sc.lights).built(orc)
    bt = np_wide.batches(D.f0)
    assert bt["n_batches"] == 0 and bt["crown"] == D.f0.shape[0]
    base = [D.prims[p][2].copy() for p in range(3)]
    D.r.render_frame()
    D.move(1, _pose(base[1], 2)); D.check("red moved")
    D.move(2, _pose(base[2], 3)); D.enable(1, False); D.check("green moved, red out")
    D.enable(0, False); D.check("white out too")
    D.enable(0, True); D.enable(1, True); D.check("both back")
    D.move(1, base[1]); D.move(2, base[2])
    dq, df, ratio = D.check("home again")
    assert ratio == np.float32(1.0) and np.array_equal(df, D.f0) and np.array_equal(dq, D.q0) and D.r.stats()["rebuilds"] == 0
    D.r.close()


@pytest.mark.gpu
def test_records_after_a_rebuild_by_the_cost_rule(R, orc, get_scene, scenes):
    """(f) refit_rebuild_ratio = 1.05 and a move far away: the refit's cost passes it, so the next move builds -- the records are collapse + quantise over the NEW tree,
    the ratio is 1.0 again and one rebuild is counted"""
    sc = get_scene("sponza_like", 0.12)
    a, b = _choose_movers(R, orc, scenes, sc)
    rest = [j for j in range(len(sc.primitives)) if j not in (a, b)]
    D = Driven(R, sc, [rest, [a], [b]], {"refit_rebuild_ratio": 1.05}, scenes.sponza_lights(1)).built(orc)
    r = D.r
    r.render_frame()
    far = D.prims[D.first[1]][2].copy(); far[:, 3] += np.array([0.0, 6.0, 0.0], np.float32)   # (six units up: the crown's boxes inflate, the models stay within the camera's 10 units -- farther, and residency takes them out)
    D.move(1, far); D.move(2, far)
    _, _, ratio = D.check("A and B far away")
    assert ratio > 1.05 and r.stats()["rebuilds"] == 0
    D.move(1, _pose(far, 1)); r.render_frame(); r.sync()
    st = r.stats()
    assert st["rebuilds"] == 1 and st["refit_cost_ratio"] == 1.0
    f, q, lb = _model_of_device(r, None, None, orc)
    _assert_records(r, f, q, "after the rebuild")
    llo, lhi = np_wide.leaf_boxes(D.prims, lb["leaf_gid"])
    assert _same_bits(llo, lb["leaf_lo"]) and _same_bits(lhi, lb["leaf_hi"])
    assert not np.array_equal(f[:, 24:28], D.f0[:, 24:28]) if f.shape == D.f0.shape else True, "the same topology as before the move: the test shows nothing"
    r.close()
