"""The 4-wide tree every frame, AO pass, cast and point query walks -- its collapse from the binary tree, its 8-bit quantisation, its per-frame refit, its surface-area
cost and the refit's batches -- restated in numpy from the RULE (DESIGN.md "Data structures", 1.1, 3.1, 3.8 and the comments above the kernels), not from either of the
two C++ collapses: what tests/test_wide_tree.py compares art_get_wide_nodes with, bit for bit.  float32 where the kernels use float, float64 where they use double, no
fused operation but the one the rule names (the library is compiled with -ffp-contract=off).

The rule.  COLLAPSE: wide nodes are numbered breadth first, the root first; a wide node stands on a binary node and starts from that node's two children as candidates;
while there are fewer than four, the internal candidate of the largest half-area (dx * dy + dy * dz + dz * dx, float32, in that order; strictly greater, so the first of
equals) is replaced by its first child, its second child is appended; only leaves left ends it.  The children are then sorted, stably, by box centre 0.5f * lo + 0.5f * hi
along the axis on which the centres spread most (strictly greater: the lower axis of equals).  An internal child gets the next free number of the next level.  A single
triangle is a root with one leaf child.  Float record (DevNodeW, 32 words): child boxes lo.xyz hi.xyz in words 0..23, child references 24..27 (>= 0 a wide node, < 0
~leaf position, INT32_MIN absent -- with a point box at 3e38), the valid bits in word 28, the sort axis in 29, zeros behind.

QUANTISE (DevNode4, 16 words: origin.xyz | exps | lo planes x y z | hi planes x y z, byte c = child c | two zeros | the child references): the origin is the minimum corner
of the children that are not NOWHERE (lo.x >= 3e38: a masked subtree), 0 if there is none; per axis the scale is the smallest power of two s >= 2^-100 with
fma(255, s, origin) >= the maximum corner; a child's planes are floor / ceil of (coordinate - origin) / s in float64, clamped to 0..255, then stepped outwards while
fma(plane, s, origin) is still inside the float box (the guards) and inwards while the next plane's fma is a LARGER value (a smaller one for hi) that still contains the box
(floor and ceil are of the exact quotient; the fma may round the next plane exactly onto the box); a nowhere child and an absent one carry the inverted box, lo planes 255 and hi planes 0; exps holds the
three biased exponents and, in its top byte, the valid bits.

REFIT: the topology, child order, valid bits and sort axes are the build's; a leaf child's box is its triangle's (a masked triangle's: the point at 3e38), an internal
child's the exact min / max union of that node's own child boxes that are not nowhere, bottom-up; a node with nothing left below it is nowhere (lo = hi = 3e38).
COST: the float64 sum over all nodes of the half-areas (float64 differences and products) of the child boxes that are valid and not nowhere; the root's union apart.
BATCHES: subtree sizes in nodes; a node of at most 768 nodes whose parent has more roots a batch subtree, such roots in index order fill batches up to 768 + 384 nodes;
the root and every node above the batch roots is the crown.  (A tree of at most 768 nodes is all crown.)

The fma's single rounding (_fma).  Its operands here are q * s + o with q an integer 0..255, s a power of two and o a float32: q * s has at most 8 significant bits, o at
most 24, and the product is exact in float64.  Either the exact sum spans at most 53 bits -- then the float64 sum IS the exact sum and rounding it to float32 is the fma's
one rounding -- or it spans more: then the smaller operand lies wholly below the larger one's last bit, by more than 53 - 24 - 8 = 21 binary places when the smaller one is o
(|o| < 2^-21 * lsb(q s), and ulp32(q s) <= 2^-16 * lsb(q s): |o| < ulp32 / 32) and by more than 53 - 8 - 24 = 21 places when it is q * s (|q s| < 2^-21 * lsb(o) <=
2^-21 * ulp32(o)).  The exact sum is then the larger operand -- itself a float32 -- plus a perturbation below a quarter of its float32 ulp even at a binade boundary, so
its one rounding gives the larger operand back; the float64 sum lies between the larger operand and the exact sum, and rounds to float32 in the same way.  No double rounding in either case.
A subnormal float32 result is rounded from the same float64 value by the same argument (numpy's cast rounds correctly into the subnormals).

COUNTS says which rules the runs so far went through (tests/test_wide_tree.py prints them per case).  `mutant` makes a deliberately wrong model (MUTANTS): test-only."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
ABSENT = np.iinfo(np.int32).min
NOWHERE = F32(3.0e38)
MIN_EXP = -100
BATCH_NODES = 768
MUTANTS = (">= in the area tie", "the second child takes the slot", "unstable sort", "axis ties to the higher axis", "centre 0.5f * (lo + hi)", "exponent + 1",
           "round for floor", "nowhere children in the origin", "nowhere children in the cost", "nowhere children quantised as boxes", "no root union in the cost",
           "nowhere children in the refit's unions", "an emptied node keeps an empty box", "no inward step", "no plane guards")
REACH = ("area ties", "axis ties", "nodes with 1 child", "nodes with 2 children", "nodes with 3 children", "2^-100 axes", "e++ loop", "a smaller exponent than the extent's passes",
         "lo plane guard", "hi plane guard", "lo plane stepped inwards", "hi plane stepped inwards", "nowhere children", "all-nowhere nodes")
COUNTS = collections.Counter()


def _is(mutant, name):
    assert mutant is None or mutant in MUTANTS, mutant
    return mutant == name


def _fma(q, s, o):
    """float32 fma(q, s, o) for q in 0..255, s a power of two, o float32 (the module docstring: the float64 sum rounds like the exact one)"""
    with np.errstate(all="ignore"):
        return (np.asarray(q, F64) * np.asarray(s, F64) + np.asarray(o, F64)).astype(F32)


def parts(float_records):
    """(lo [n, 4, 3], hi [n, 4, 3] float32, child [n, 4] int32) of (n, 32) uint32 float records"""
    f = np.ascontiguousarray(float_records, np.uint32).reshape(-1, 32)
    b = f[:, :24].view(F32).reshape(-1, 4, 6)
    return b[:, :, :3].copy(), b[:, :, 3:].copy(), f[:, 24:28].view(np.int32).copy()


def _pack_float(lo, hi, child, axis):
    n = child.shape[0]
    f = np.zeros((n, 32), np.uint32)
    b = np.concatenate([lo, hi], axis=2).astype(F32)
    f[:, :24] = np.ascontiguousarray(b).view(np.uint32).reshape(n, 24)
    f[:, 24:28] = child.view(np.uint32)
    f[:, 28] = ((child != ABSENT) << np.arange(4)).sum(1).astype(np.uint32)
    f[:, 29] = axis
    return f


def collapse(child, node_lo, node_hi, leaf_lo, leaf_hi, mutant=None):
    """-> (float records (n, 32) uint32, level offsets [levels + 1], sort axis per node) of the binary tree child [T - 1, 2] (~leaf for a leaf), node_lo / node_hi over the leaves"""
    leaf_lo, leaf_hi = np.ascontiguousarray(leaf_lo, F32).reshape(-1, 3), np.ascontiguousarray(leaf_hi, F32).reshape(-1, 3)
    T = leaf_lo.shape[0]
    NI = T - 1
    child = np.ascontiguousarray(child, np.int32).reshape(-1, 2)[:NI]
    node_lo, node_hi = np.ascontiguousarray(node_lo, F32).reshape(-1, 3)[:NI], np.ascontiguousarray(node_hi, F32).reshape(-1, 3)[:NI]
    ge, second, unstable, high_axis = _is(mutant, ">= in the area tie"), _is(mutant, "the second child takes the slot"), _is(mutant, "unstable sort"), _is(mutant, "axis ties to the higher axis")
    counts = collections.Counter()
    with np.errstate(all="ignore"):
        d = node_hi - node_lo
        area = ((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0]).astype(F32).tolist()
        lo_all, hi_all = np.concatenate([node_lo, leaf_lo]), np.concatenate([node_hi, leaf_hi])       # a reference's row: ref for a node, NI + ~ref for a leaf
        if _is(mutant, "centre 0.5f * (lo + hi)"):
            cen = (F32(0.5) * (lo_all + hi_all)).astype(F32)
        else:
            cen = (F32(0.5) * lo_all + F32(0.5) * hi_all).astype(F32)
    row = lambda ref: ref if ref >= 0 else NI + ~ref
    kids = child.tolist()
    out_child, out_axis, levels = [], [], [0]
    level = [0] if NI > 0 else [~0]                     # what each wide node of the level stands on: a binary node, or (a single triangle) the leaf itself
    n_done = 0
    while level:
        nxt = []
        first_next = n_done + len(level)
        for on in level:
            if on < 0:
                cand = [on]
            else:
                cand = list(kids[on])
                while len(cand) < 4:
                    best, best_area = -1, -1.0
                    for i, c in enumerate(cand):
                        if c < 0:
                            continue
                        if best >= 0 and area[c] == best_area:
                            counts["area ties"] += 1
                        if area[c] > best_area or (ge and area[c] >= best_area):
                            best, best_area = i, area[c]
                    if best < 0:
                        break
                    a, b = kids[cand[best]]
                    if second:
                        a, b = b, a
                    cand[best] = a
                    cand.append(b)
            c = cen[[row(r) for r in cand]]                 # [nc, 3]
            with np.errstate(all="ignore"):
                spread = (c.max(0) - c.min(0)).astype(F32)
            axis, best_spread = 0, F32(-1.0)
            for k in range(3):
                if k and spread[k] == best_spread:
                    counts["axis ties"] += 1
                if spread[k] > best_spread or (high_axis and spread[k] >= best_spread):
                    axis, best_spread = k, spread[k]
            key = c[:, axis].tolist()
            order = sorted(range(len(cand)), key=(lambda i: (key[i], -i)) if unstable else (lambda i: key[i]))   # (sorted() is stable)
            cand = [cand[i] for i in order]
            if len(cand) < 4:
                counts[f"nodes with {len(cand)} child" + ("ren" if len(cand) > 1 else "")] += 1
            refs = []
            for r in cand:
                if r < 0:
                    refs.append(r)
                else:
                    refs.append(first_next + len(nxt))
                    nxt.append(r)
            out_child.append(((refs + [ABSENT] * 4)[:4], [row(r) for r in cand]))      # (the references, the rows of their boxes)
            out_axis.append(axis)
        n_done += len(level)
        levels.append(n_done)
        level = nxt
    n = n_done
    wchild = np.array([c for c, _ in out_child], np.int64).astype(np.int32).reshape(n, 4)
    lo, hi = np.full((n, 4, 3), NOWHERE, F32), np.full((n, 4, 3), NOWHERE, F32)
    for w, (_, rows) in enumerate(out_child):
        lo[w, :len(rows)] = lo_all[rows]
        hi[w, :len(rows)] = hi_all[rows]
    if mutant is None:
        COUNTS.update(counts)
    return _pack_float(lo, hi, wchild, np.array(out_axis, np.uint32)), np.array(levels, np.int64), np.array(out_axis, np.uint32)


def quantise(float_records, mutant=None, counts=None):
    """-> the (n, 16) uint32 quantised records of (n, 32) float records"""
    lo, hi, child = parts(float_records)
    n = child.shape[0]
    present = child != ABSENT
    nowhere = present & (lo[:, :, 0] >= NOWHERE)
    live = present & ~nowhere
    c = collections.Counter()
    c["nowhere children"] += int(nowhere.sum())
    c["all-nowhere nodes"] += int((present.any(1) & ~live.any(1)).sum())
    in_origin = present if _is(mutant, "nowhere children in the origin") else live
    boxed = present if _is(mutant, "nowhere children quantised as boxes") else live
    inward_off = _is(mutant, "no inward step")
    with np.errstate(all="ignore"):
        org = np.where(in_origin[:, :, None], lo, F32(np.inf)).min(1)
        top = np.where(in_origin[:, :, None], hi, F32(-np.inf)).max(1)
        none = ~in_origin.any(1)
        org[none], top[none] = F32(0), F32(0)
        # the smallest power of two s >= 2^-100 with fma(255, s, origin) >= top: from the exponent of the extent, one way or the other until it is the smallest
        ext = top.astype(F64) - org.astype(F64)
        m, ex = np.frexp(np.where(ext > 0, ext / 255.0, 1.0))
        e = np.where(ext > 0, np.where(m == 0.5, ex - 1, ex), MIN_EXP).astype(np.int64)
        e = np.maximum(e, MIN_EXP)
        ok = lambda e: _fma(255.0, np.ldexp(1.0, e), org) >= top
        while True:
            bad = ~ok(e) & (e < 127)                                                     # (finite boxes always get there; the bound only keeps a NaN from looping)
            if not bad.any():
                break
            c["e++ loop"] += int(bad.sum())
            e[bad] += 1
        while True:
            down = (e > MIN_EXP) & ok(np.maximum(e - 1, MIN_EXP))
            if not down.any():
                break
            c["a smaller exponent than the extent's passes"] += int(down.sum())
            e[down] -= 1
        c["2^-100 axes"] += int((e == MIN_EXP).sum())
        if _is(mutant, "exponent + 1"):
            e = e + 1
        s = np.ldexp(1.0, e)                                                             # [n, 3] float64, exact
        o64, s4, o4 = org.astype(F64)[:, None, :], s[:, None, :], org[:, None, :]
        lo_b, hi_b = np.where(boxed[:, :, None], lo, o4), np.where(boxed[:, :, None], hi, o4)
        down_to = (lambda x: np.floor(x + 0.5)) if _is(mutant, "round for floor") else np.floor
        ql = np.clip(down_to((lo_b.astype(F64) - o64) / s4), 0, 255).astype(np.int64)
        qh = np.clip(np.ceil((hi_b.astype(F64) - o64) / s4), 0, 255).astype(np.int64)
        guards_off = _is(mutant, "no plane guards")
        while not guards_off:                                                            # the guards: outwards while the plane, as the walks evaluate it, is inside the float box
            g = boxed[:, :, None] & (ql > 0) & (_fma(ql, s4, o4) > lo_b)
            if not g.any():
                break
            c["lo plane guard"] += int(g.sum())
            ql[g] -= 1
        while not guards_off:
            g = boxed[:, :, None] & (qh < 255) & (_fma(qh, s4, o4) < hi_b)
            if not g.any():
                break
            c["hi plane guard"] += int(g.sum())
            qh[g] += 1
        while True:                                                                      # ... and inwards while the next plane, as the walks evaluate it, is a tighter value that still contains
            v = _fma(np.minimum(ql + 1, 255), s4, o4)
            g = boxed[:, :, None] & (ql < 255) & (v <= lo_b) & (v > _fma(ql, s4, o4))
            if inward_off or not g.any():
                break
            c["lo plane stepped inwards"] += int(g.sum())
            ql[g] += 1
        while True:
            v = _fma(np.maximum(qh - 1, 0), s4, o4)
            g = boxed[:, :, None] & (qh > 0) & (v >= hi_b) & (v < _fma(qh, s4, o4))
            if inward_off or not g.any():
                break
            c["hi plane stepped inwards"] += int(g.sum())
            qh[g] -= 1
    ql = np.where(boxed[:, :, None], ql, 255)
    qh = np.where(boxed[:, :, None], qh, 0)
    q = np.zeros((n, 16), np.uint32)
    q[:, 0:3] = org.astype(F32).view(np.uint32)
    mask = (present << np.arange(4)).sum(1)
    eb = e + 127
    q[:, 3] = (eb[:, 0] | (eb[:, 1] << 8) | (eb[:, 2] << 16) | (mask << 24)).astype(np.uint32)
    shift = (8 * np.arange(4))[None, :, None]
    q[:, 4:7] = (ql << shift).sum(1).astype(np.uint32)
    q[:, 7:10] = (qh << shift).sum(1).astype(np.uint32)
    q[:, 12:16] = child.view(np.uint32)
    if mutant is None:
        COUNTS.update(c)
    if counts is not None:
        counts.update(c)
    return q


def level_offsets(child):
    """the level offsets of breadth-first numbered records from their child references alone (asserts that every level is contiguous and in order)"""
    offs, first, count = [0], 0, 1
    n = child.shape[0]
    while count:
        kids = child[first:first + count].reshape(-1)
        kids = kids[kids >= 0]
        assert np.array_equal(kids, first + count + np.arange(kids.size)), "not a breadth-first numbering"
        first, count = first + count, kids.size
        offs.append(first)
    assert first == n, (first, n)
    return np.array(offs, np.int64)


def refit(float_records, leaf_lo, leaf_hi, mutant=None):
    """-> the float records over other leaf boxes: the topology kept, every child box the exact union of what is below it"""
    leaf_lo, leaf_hi = np.ascontiguousarray(leaf_lo, F32).reshape(-1, 3), np.ascontiguousarray(leaf_hi, F32).reshape(-1, 3)
    lo, hi, child = parts(float_records)
    offs = level_offsets(child)
    union_all, keep_empty = _is(mutant, "nowhere children in the refit's unions"), _is(mutant, "an emptied node keeps an empty box")
    is_leaf = (child < 0) & (child != ABSENT)
    is_node = child >= 0
    for lv in range(len(offs) - 2, -1, -1):
        a, b = offs[lv], offs[lv + 1]
        ch = child[a:b]
        leaf = is_leaf[a:b]
        pos = np.where(leaf, ~ch, 0)
        lo[a:b] = np.where(leaf[:, :, None], leaf_lo[pos], lo[a:b])
        hi[a:b] = np.where(leaf[:, :, None], leaf_hi[pos], hi[a:b])
        node = is_node[a:b]
        if node.any():
            below = np.where(node, ch, 0)                                                  # [m, 4]: the node under each child (already refitted: a deeper level)
            blo, bhi, bch = lo[below], hi[below], child[below]                            # [m, 4, 4, 3]
            use = bch != ABSENT
            if not union_all:
                use = use & (blo[..., 0] < NOWHERE)
            ulo = np.where(use[..., None], blo, F32(np.inf)).min(2)
            uhi = np.where(use[..., None], bhi, F32(-np.inf)).max(2)
            empty = ~use.any(2)
            if not keep_empty:
                ulo[empty], uhi[empty] = NOWHERE, NOWHERE
            lo[a:b] = np.where(node[:, :, None], ulo, lo[a:b])
            hi[a:b] = np.where(node[:, :, None], uhi, hi[a:b])
    f = np.ascontiguousarray(float_records, np.uint32).reshape(-1, 32)
    return _pack_float(lo, hi, child, f[:, 29])


def cost(float_records, mutant=None):
    """-> (the float64 sum over all nodes of the half-areas of their valid child boxes that are not nowhere, the half-area of the root's union of such boxes)"""
    lo, hi, child = parts(float_records)
    live = child != ABSENT
    if not _is(mutant, "nowhere children in the cost"):
        live = live & (lo[:, :, 0] < NOWHERE)
    with np.errstate(all="ignore"):
        d = hi.astype(F64) - lo.astype(F64)
        a = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
        total = float(np.where(live, a, 0.0).sum())
        root = 0.0
        if live[0].any() and not _is(mutant, "no root union in the cost"):
            r = hi[0][live[0]].max(0).astype(F64) - lo[0][live[0]].min(0).astype(F64)
            root = float(r[0] * r[1] + r[1] * r[2] + r[2] * r[0])
    return total, root


def batches(float_records):
    """the refit's work partition -> dict(size [n] subtree sizes in nodes, batch_of [n] (-1: the crown), n_batches, batch_nodes [n_batches], crown (its node count),
    leaf_batch [T] (-1: a leaf that hangs on a crown node))"""
    _, _, child = parts(float_records)
    n = child.shape[0]
    parent = np.full(n, -1, np.int64)
    for i in range(4):
        k = child[:, i] >= 0
        parent[child[k, i]] = np.nonzero(k)[0]
    size = np.ones(n, np.int64)
    for w in range(n - 1, 0, -1):
        size[parent[w]] += size[w]
    batch_of = np.full(n, -1, np.int64)
    nb, fill = 0, 0
    for w in range(1, n):
        if size[w] > BATCH_NODES:
            continue
        up = parent[w]
        if size[up] > BATCH_NODES:
            if nb == 0 or fill + size[w] > BATCH_NODES + BATCH_NODES // 2:
                nb, fill = nb + 1, 0
            fill += size[w]
            batch_of[w] = nb - 1
        else:
            batch_of[w] = batch_of[up]
    leaves = (child < 0) & (child != ABSENT)
    T = int(leaves.sum())
    leaf_batch = np.full(T, -1, np.int64)
    holder = np.repeat(np.arange(n), 4).reshape(n, 4)
    leaf_batch[~child[leaves]] = batch_of[holder[leaves]]
    return dict(size=size, batch_of=batch_of, n_batches=nb, batch_nodes=np.bincount(batch_of[batch_of >= 0], minlength=nb), crown=int((batch_of < 0).sum()), leaf_batch=leaf_batch, parent=parent)


def xform(m, p):
    """((m0 * x + m1 * y) + m2 * z) + m3 per row of the row-major 3x4 matrix, in float32: p [n, 3] -> [n, 3]"""
    m = np.asarray(m, F32).reshape(3, 4)
    p = np.asarray(p, F32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    with np.errstate(all="ignore"):
        return (((m[None, :, 0] * x + m[None, :, 1] * y) + m[None, :, 2] * z) + m[None, :, 3]).astype(F32)


def leaf_boxes(prims, leaf_gid):
    """the leaf boxes of a scene state: prims a list of (positions [nv, >= 3] float32, indices, matrix (12 floats), enabled) in primitive order -- the triangles' global
    ids run through them in that order -- transformed in float32, min / max of the three vertices, a disabled primitive's at 3e38; -> (leaf_lo, leaf_hi) in the order of leaf_gid"""
    los, his = [], []
    for pos, idx, m, enabled in prims:
        ix = np.asarray(idx).astype(np.int64).reshape(-1, 3)
        if enabled:
            w = xform(m, np.asarray(pos, F32)[:, :3])
            a, b, c = w[ix[:, 0]], w[ix[:, 1]], w[ix[:, 2]]
            los.append(np.minimum(np.minimum(a, b), c))
            his.append(np.maximum(np.maximum(a, b), c))
        else:
            los.append(np.full((ix.shape[0], 3), NOWHERE, F32))
            his.append(np.full((ix.shape[0], 3), NOWHERE, F32))
    lo, hi = np.concatenate(los), np.concatenate(his)
    g = np.asarray(leaf_gid).astype(np.int64)
    return lo[g], hi[g]


def first_difference(got, want, what):
    """None, or a line that says where two record arrays first differ"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{what}: {got.shape[0]} records, the model has {want.shape[0]}"
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    w, k = bad[0]
    return f"{what}: {np.unique(bad[:, 0]).size} of {got.shape[0]} records differ, first node {w} word {k}: {int(got[w, k]):#010x}, the model has {int(want[w, k]):#010x} (words that differ anywhere: {sorted(set(bad[:, 1].tolist()))})"
