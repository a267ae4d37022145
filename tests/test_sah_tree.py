"""The device SAH builder's tree (art_sahdev.hip: the tree every frame, cast and query walks by default) against tests/np_sah.py, bit for bit.  Any tree of exact boxes gives
the oracle's bits, so the walks' parity tests pass for ANY valid tree: a builder that bins on the wrong axis, breaks ties the other way or drops the half-bin
margin would only move the ray rate.  The builder is deterministic (integer atomics through order-preserving keys, costs in doubles in a fixed order, ties to the lower
(axis, bin), stable partitions, node numbers from the pre-order rule), so its tree can be restated and compared with no tolerance.

Without a device: (a) the model's tree is a valid tree (helpers.check_tree_arrays: _check_traversal_tree's assertions) and, where the table says so, cheaper by the
surface-area cost than the canonical LBVH topology over the same leaves; (b) every mutated model (np_sah.MUTANTS) gives another `child` array on at least one case, and the
cases reach every rule and structural event the model counts (np_sah.RULES, np_sah.EVENTS).  On the device: (c) per case the default build, and a second build in the same
context (the arena reused: stale bins, counters and lists), give the model's child / node_lo / node_hi over the device's own leaves; (d) the same through 30-bit Morton keys
and after a rebuild that a moved model starts, while the host builder and the LBVH topology do NOT give the model's tree (so a form table cannot silently run the default).

What the table does not reach, and why:
  * a level of more than 16 384 open ranges (k_mid's batch of 8) needs more than 280 000 leaves: the full-size oracle tests cover it; np_sah counts it, nothing here requires it.
  * chain_scene cannot reach the depth-48 guard of the level loop: its slivers' areas halve from one to the next, so the cheapest plane peels about log2(n) of them per level,
    not one (the model counts 23 plane splits and depth 35 for all 149 slivers float32 has room for).  The guard is reached by "row 70": seventy zero-area triangles on one
    line -- every plane costs 0, the tie goes to the lowest bin, which holds one or two leaves -- where the model counts 48 plane splits, one position split by the depth
    guard and 11 sweep nodes cut short by range depth + sub-depth >= 48.
  * "kMid 2048" cannot change the tree: which kernel takes a range (k_mid in LDS, or k_bin + k_choose + the partition kernels) is invisible in the result by design, and the
    model's tree does not depend on the threshold at all.  For this mutant the test asserts the opposite of the others: the same `child` on every case, with ranges between
    2049 and 4096 leaves present (its structural counts differ), which is what the cases at 4096 / 4097 / 4200 leaves hold the device to.
  * the SAH centroid 0.5f * lo + 0.5f * hi and k_soup's (lo + hi) * 0.5f round alike wherever halving is exact: they differ only on subnormal coordinates (or overflow).  The
    two "clamped from outside the domain" events and the centroid mutant are reached by the cases with subnormal coordinates alone: chain_scene(149), whose last slivers are
    subnormal, and the "subnormal specks".  (With a scale of 64 / subnormal = inf the bins there are 0 or the last one: bin_of's clamp as a float is what keeps that defined.)"""
import numpy as np
import pytest

import np_sah
from helpers import R, chain_scene, check_tree_arrays, degenerate_soup, oracle_for  # noqa: F401  (R: a module fixture)


def _tri_scene(name, tris, before=()):
    from araytracingjourney_amd import scenes
    mb = scenes.MeshBuilder()
    for t in tris:
        mb.add([tuple(p) for p in t], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
    c = scenes.cornell()
    return scenes.Scene(name, list(before) + [mb.finish(scenes.constant_texture((200, 180, 160)))], c.camera, c.lights)


def segment_row(n):
    """n zero-area triangles (three collinear points) in a row on the x axis: every box is a segment, every union has area 0, every plane costs 0"""
    return _tri_scene("row", [((k, 0, 0), (k + 0.25, 0, 0), (k + 0.5, 0, 0)) for k in range(n)])


def geometric_fan(n=16, ratio=8.0):
    """n triangles round one vertex, each `ratio` times smaller than the last: the exact sweep peels one per level (area ratio 64 > n)"""
    return _tri_scene("fan", [((0, 0, 0), (ratio ** -k, 0, 0.5 * ratio ** -k), (0, ratio ** -k, 0.5 * ratio ** -k)) for k in range(n)])


def subnormal_specks(n):
    """equal triangles in planes x = m * 2^-149, m odd: half of a subnormal rounds, so 0.5f * x + 0.5f * x is 0, 4, 4, 8, 8 ... for m = 1, 3, 5, 7, 9 ... where (x + x) * 0.5f is m
    itself.  All Morton keys but the first are equal, so the leaves keep this order: the sweep's stable sort on x leaves 5 in front of 3 where the exact centroid would not"""
    u = 2.0 ** -149
    odd = list(range(1, 2 * n, 2))
    order = [m for k in range(1, n - 1, 2) for m in (odd[k + 1], odd[k])]                  # 5, 3, 9, 7, 13, 11 ...
    return _tri_scene("specks", [((m * u, 0, 0), (m * u, 0.1, 0), (m * u, 0, 0.1)) for m in [1] + order + odd[len(order) + 1:]])


def soup_and_outlier(n):
    """a soup and one triangle 200 units away: every plane of the root that has leaves on both sides peels that one leaf from a range of more than 4096"""
    return _tri_scene("soup + outlier", [((200, 0, 0), (200.1, 0, 0), (200, 0.1, 0.1))], degenerate_soup(n, "soup").primitives)


def soup_and_copies(n_soup, n_copies):
    """a soup and n_copies > 16 copies of one triangle: a range of coincident centroids has no candidate plane"""
    return _tri_scene("soup + copies", [((0.1, 0.1, 0.1), (0.2, 0.1, 0.1), (0.1, 0.2, 0.2))] * n_copies, degenerate_soup(n_soup, "soup").primitives)


def _get(name, detail):
    from araytracingjourney_amd import scenes
    return scenes.get_scene(name, detail)


# id -> (the scene, whether the model's cost must be below the LBVH's, what the case is there for / what the model counted)
CASES = {
    "soup 3": (lambda: degenerate_soup(3, "soup"), False, "one small range of 3; exempt: two inner nodes, the sweep and Karras agree (1.608 both)"),
    "soup 16": (lambda: degenerate_soup(16, "soup"), True, "one small range at depth 0"),
    "soup 17": (lambda: degenerate_soup(17, "soup"), True, "one level, then small ranges"),
    "soup 18": (lambda: degenerate_soup(18, "soup"), True, "one level, then small ranges"),
    "soup 40": (lambda: degenerate_soup(40, "soup"), True, "one level, then small ranges"),
    "soup 300": (lambda: degenerate_soup(300, "soup"), True, ""),
    "soup 4096": (lambda: degenerate_soup(4096, "soup"), True, "one range at the LDS staging limit"),
    "soup 4097": (lambda: degenerate_soup(4097, "soup"), True, "just past it: k_bin, k_choose and the partition kernels for the root"),
    "soup 4200": (lambda: degenerate_soup(4200, "soup"), True, ""),
    "soup 9000": (lambda: degenerate_soup(9000, "soup"), True, "two large children in one k_bin window"),
    "soup 40000": (lambda: degenerate_soup(40000, "soup"), True, "more than 512 open ranges: batch 2"),
    "soup 160000": (lambda: degenerate_soup(160000, "soup"), True, "more than 4096 open ranges: batch 4"),
    "flat 6000": (lambda: degenerate_soup(6000, "flat"), True, "a flat side: bin 0, never chosen"),
    "line 6000": (lambda: degenerate_soup(6000, "line"), False, "exempt from the cost assertion: starves the heuristic"),
    "one point 5000": (lambda: degenerate_soup(5000, "one point"), False, "exempt from the cost assertion: starves the heuristic"),
    "clusters 20000": (lambda: degenerate_soup(20000, "clusters"), True, "large and mid ranges in one level"),
    "cornell": (lambda: _get("cornell", 1.0), True, ""),
    "sponza_like 0.12": (lambda: _get("sponza_like", 0.12), True, ""),
    "chain 149": (lambda: chain_scene(149)[0], False, "exempt: the LBVH's comb is the cheaper tree here (4.849 against the model's 5.918); subnormal centroids: 15 clamped into bin 0 from below the root's domain; depth 35"),
    "subnormal specks 12": (lambda: subnormal_specks(12), False, "exempt: equal boxes but for subnormal x, every tree costs the same; the sweep orders the leaves by the rounded centroids"),
    "subnormal specks 20": (lambda: subnormal_specks(20), False, "exempt likewise; the root's domain is [1, 39] * 2^-149, the centroids binned are 0, 4, 4, 8 ... 36, 40 * 2^-149: clamped from outside at both ends"),
    "row 70": (lambda: segment_row(70), False, "exempt: every area is 0; the level loop's depth-48 guard (1 node) and the sweep's (11 nodes), 47 one-leaf sides by k_mid<true>"),
    "fan 16": (lambda: geometric_fan(16), False, "exempt: the sweep's comb is Karras' (2.032 both); the sweep's depth-10 guard (3 nodes)"),
    "soup 4200 + outlier": (lambda: soup_and_outlier(4200), True, "a one-leaf side of a range of more than 4096 leaves: k_leaf_refs"),
    "soup 60 + 40 copies": (lambda: soup_and_copies(60, 40), True, "position splits for want of a candidate (3 nodes)"),
}
LARGE = ("soup 40000", "soup 160000")   # the mutants run over these only when no smaller case tells them apart
_cache = {}


def _case(key, orc):
    """the scene, the oracle's canonical LBVH over it (63-bit keys: the device's default leaf order) and the model's tree over those leaves, made once"""
    if key not in _cache:
        sc = CASES[key][0]()
        lb = oracle_for(orc, sc, morton_bits=63)[0].lbvh()
        _cache[key] = (sc, lb, np_sah.build(lb["leaf_lo"], lb["leaf_hi"]))
    return _cache[key]


def _as_dict(tree):
    return dict(child=tree.child, node_lo=tree.node_lo, node_hi=tree.node_hi)


@pytest.mark.parametrize("key", list(CASES))
def test_model_tree_is_valid_and_cheaper_than_the_lbvh(orc, key):
    """(a)"""
    sc, lb, tree = _case(key, orc)
    assert check_tree_arrays(lb, _as_dict(tree), same_as_karras_allowed=True) == sc.n_tris
    cost = np_sah.sah_cost(tree.child, tree.node_lo, tree.node_hi, lb["leaf_lo"], lb["leaf_hi"])
    lbvh = np_sah.sah_cost(lb["child"], lb["node_lo"], lb["node_hi"], lb["leaf_lo"], lb["leaf_hi"])
    print(f"\n[sah cost] {key}: T {sc.n_tris}, model {cost:.3f}, LBVH {lbvh:.3f}")
    if CASES[key][1]:
        assert cost < lbvh, (key, cost, lbvh)


def test_tiny_inputs_build_nothing():
    z = np.zeros((2, 3), np.float32)
    assert np_sah.build(z[:0], z[:0]) is None and np_sah.build(z[:1], z[:1]) is None and np_sah.build(z, z) is None


@pytest.mark.parametrize("mutant", np_sah.MUTANTS)
def test_cases_tell_a_mutated_builder_apart(orc, mutant):
    """(b)"""
    told, same, other_kernels = [], [], []
    for key in [k for k in CASES if k not in LARGE] + list(LARGE):
        if key in LARGE and told:
            break
        sc, lb, tree = _case(key, orc)
        other = np_sah.build(lb["leaf_lo"], lb["leaf_hi"], mutant=mutant)
        if mutant != "depth guards off":   # (a wrong builder still builds a valid tree: the walks' tests would pass; without the guards it may be deeper than the stacks)
            assert check_tree_arrays(lb, _as_dict(other), same_as_karras_allowed=True) == sc.n_tris
        (same if np.array_equal(other.child, tree.child) else told).append(key)
        if other.counts != tree.counts:
            other_kernels.append(key)
    if mutant == "kMid 2048":   # (the module docstring: the tree does not depend on which kernel takes a range)
        assert not told and other_kernels, f"'{mutant}': another tree on {told}, other kernels on {other_kernels}"
        return
    assert told, f"no case tells '{mutant}' from the builder: the same child array on {same}"
    print(f"\n[mutant] '{mutant}' is told apart by {told}")


def test_cases_reach_every_rule_and_event(orc):
    """(b): over the table (every case's model run, mutants not counted) each rule and each structural event np_sah counts happens at least once"""
    np_sah.COUNTS.clear()
    for key in CASES:
        sc, lb, _ = _case(key, orc)
        np_sah.build(lb["leaf_lo"], lb["leaf_hi"])
    missing = [name for name in np_sah.RULES + np_sah.EVENTS if np_sah.COUNTS[name] == 0]
    assert not missing, missing


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------------
def _model_for(dev_lb, key, orc):
    """the model's tree over the DEVICE's leaves (the cached one where they are the oracle's, bit for bit)"""
    if key is not None:
        _, lb, tree = _case(key, orc)
        if all(np.array_equal(dev_lb[k].view(np.uint32), lb[k].view(np.uint32)) for k in ("leaf_lo", "leaf_hi")):
            return tree
    return np_sah.build(dev_lb["leaf_lo"], dev_lb["leaf_hi"])


def _compare(r, key, orc, what):
    lb, tr = r.get_lbvh(), r.get_traversal_tree()
    tree = _model_for(lb, key, orc)
    diff = np_sah.first_difference(tree, tr["child"], tr["node_lo"], tr["node_hi"])
    assert diff is None, f"{key}, {what}: {diff}"
    assert np.array_equal(tr["child"], tree.child)
    assert np.array_equal(tr["node_lo"].view(np.uint32), tree.node_lo.view(np.uint32)) and np.array_equal(tr["node_hi"].view(np.uint32), tree.node_hi.view(np.uint32))
    return lb, tree


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CASES))
def test_device_tree_is_the_models(R, orc, key):
    """(c)"""
    r = R.renderer_for_scene(_case(key, orc)[0], (64, 48))
    _compare(r, key, orc, "first build")
    r.prepare_first_frame()                    # a second build in the same context: the arena is reused
    _compare(r, key, orc, "second build in the same context")
    r.close()


MID_CASE = "sponza_like 0.12"


@pytest.mark.gpu
def test_device_tree_over_30_bit_keys(R, orc):
    """(d): another leaf order, so another tree; the model gets the device's leaves"""
    sc, lb63, tree63 = _case(MID_CASE, orc)
    r = R.renderer_for_scene(sc, (64, 48), morton_bits=30)
    lb, tree = _compare(r, None, orc, "morton_bits=30")
    assert not np.array_equal(lb["leaf_gid"], lb63["leaf_gid"]) and not np.array_equal(tree.child, tree63.child), "the same leaf order as with 63 bits: the test shows nothing"
    r.close()


@pytest.mark.gpu
def test_device_tree_after_a_rebuild(R, orc):
    """(d): a model moved on a context whose cost rule rebuilds at once: the rebuilt tree is the model's tree over the new leaves"""
    sc = _case(MID_CASE, orc)[0]
    r = R.Renderer((64, 48), tuning=dict(refit_rebuild_ratio=1e-6))
    r.add_model(sc.primitives[:-1])
    r.add_model(sc.primitives[-1:])
    cam = r.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    r.prepare_first_frame()
    lb0, tree0 = _compare(r, None, orc, "before the move")
    moved = np.array(sc.primitives[-1].model, np.float32).reshape(3, 4).copy()
    moved[1, 3] += 6.0
    r.models_mut()[1].set_model_matrix(moved)
    r.render_frame()
    assert r.stats()["rebuilds"] == 1
    lb1, tree1 = _compare(r, None, orc, "after the rebuild")
    assert not np.array_equal(lb1["leaf_lo"], lb0["leaf_lo"]) and not np.array_equal(tree1.child, tree0.child), "the move changed nothing: the test shows nothing"
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host-sah", "fast-build"])
def test_other_builders_are_not_the_models(R, orc, form):
    """(d): the host builder (32 bins over exact centroid bounds) and the LBVH topology give other trees than the device builder's"""
    sc = _case(MID_CASE, orc)[0]
    r = R.renderer_for_scene(sc, (64, 48), **(dict(tuning={"tree_builder": 1}) if form == "host-sah" else dict(fast_build=True)))
    lb, tr = r.get_lbvh(), r.get_traversal_tree()
    assert not np.array_equal(tr["child"], _model_for(lb, MID_CASE, orc).child)
    r.close()
