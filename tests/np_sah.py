"""The device SAH builder (sah_build_device, art_sahdev.hip) restated in numpy from the kernels' source and DESIGN.md 1.1 / "Tree build" -- what tests/test_sah_tree.py compares
the traversal tree with, bit for bit.  float32 where the kernels use float, float64 where they use double, integers elsewhere; no fused multiply-add anywhere (the library
is compiled with -ffp-contract=off).

build(leaf_lo, leaf_hi) takes the leaf boxes in canonical leaf order ([T, 3] float32 each) and returns a Tree: child [T - 1, 2] int32 (~leaf for a leaf), node_lo / node_hi
[T - 1, 3] float32, and per node the RULE that made it (RULES), its range's size and its depth; None for T < 3, where the kernel builds nothing.

The builder, as restated here.  A RANGE is an interval of leaf positions that becomes internal node k; its left subtree starts at node k + 1, its right one at k + nl (pre-order).
Ranges of more than SMALL leaves are split level by level: every leaf goes into one of BINS bins per axis over the range's DOMAIN, bin = trunc(clamp((c - lo) * (BINS / (hi - lo)),
0, BINS - 1)) with c = 0.5f * box.lo + 0.5f * box.hi; the plane behind bin i costs half_area(left) * n_left + half_area(right) * n_right in double; the cheapest plane wins, ties
to the lower (axis, bin); the leaves are partitioned stably by bin <= i.  Without a candidate plane, or at depth SAH_DEPTH, the range is halved by position.  The root's domain
is the bounds of the centroids the Morton keys were made over, (lo + hi) * 0.5f (another rounding than c above where halving is inexact, on subnormal coordinates: a centroid may then lie outside and is clamped); a child's
domain is its box clamped into the parent's domain and, on the split axis, to half a bin beyond the plane.  Ranges of at most SMALL leaves are finished by the exact sweep
(_small).  Which kernel takes a range (k_mid, or k_bin + k_choose + the partition kernels above MID leaves) does not change the tree; the model only counts it.

COUNTS says which rules and which structural events the builds so far went through (tests/test_sah_tree.py asserts that its cases reach every one).  `mutant` makes a
deliberately wrong builder (MUTANTS): test-only, to show that the cases can tell a wrong builder from a right one."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
BINS = 64          # art_sahdev.hip: ART_SAH_BINS, the bins per axis (a lane of k_choose's wave per bin)
SMALL = 16         # ART_SAH_SMALL (kSmall): a range of at most this many leaves is finished by one thread of k_small
MID = 4096         # ART_SAH_MID (kMid): above it a range's bins are made leaf by leaf in memory (k_bin), up to it by one block in LDS (k_mid)
SAH_DEPTH = 48     # kSahDepth: from this depth on ranges are halved by position
SMALL_DEPTH = 10   # kSmallDepth: the sweep of a small range chains at most this deep before it halves
WINDOW = 2048      # kWin: the positions a block of k_bin takes

RULES = ("binned plane", "position split: no candidate", "position split: depth guard", "sweep", "sweep: n == 2", "sweep: depth-10 guard", "sweep: depth-48 guard")
EVENTS = ("a range of more than 4096 leaves", "two large ranges in one k_bin window", "a level of more than 512 open ranges (batch 2)",
          "a level of more than 4096 open ranges (batch 4)", "a level where large and mid ranges coexist", "a one-leaf side written by k_leaf_refs",
          "a one-leaf side written by k_mid<true>", "a centroid clamped into bin 0 from outside the domain", "a centroid clamped into the last bin from outside the domain")
BATCH_8 = "a level of more than 16384 open ranges (batch 8)"   # (counted, not required: tests/test_sah_tree.py says why)
MUTANTS = ("32 bins", "ties to the higher bin", "ties to the higher axis", "costs compared in float32", "right_area kept in double", "no half-bin margin",
           "child domain = child box", "SAH centroid (lo + hi) * 0.5f", "unstable partition", "k_small sorts from the original order", "kSmall 8", "kMid 2048", "depth guards off")
COUNTS = collections.Counter()


class Tree:
    def __init__(self, T):
        self.child = np.full((T - 1, 2), np.iinfo(np.int32).min, np.int32)
        self.node_lo, self.node_hi = np.zeros((T - 1, 3), F32), np.zeros((T - 1, 3), F32)
        self.rule, self.size, self.depth = np.full(T - 1, -1, np.int8), np.zeros(T - 1, np.int64), np.zeros(T - 1, np.int64)
        self.counts = collections.Counter()

    def describe(self, k):
        return f"node {k}: a range of {int(self.size[k])} leaves at depth {int(self.depth[k])}, made by '{RULES[self.rule[k]]}'"


def half_area(lo, hi):
    """half the surface area of boxes [..., 3] in double: dx * dy + dy * dz + dz * dx, unfused and in that order; 0 for an empty box (dx < 0)"""
    d = hi.astype(F64) - lo.astype(F64)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return np.where(dx < 0, 0.0, dx * dy + dy * dz + dz * dx)


def sah_cost(child, node_lo, node_hi, leaf_lo, leaf_hi):
    """the surface-area cost of a tree: the sum over inner nodes of half_area(node) / half_area(root), plus the same over leaves, in float64 (the root is node 0)"""
    root = half_area(node_lo[0], node_hi[0])
    with np.errstate(all="ignore"):   # (a root of no area: nan)
        return float((half_area(node_lo, node_hi).sum() + half_area(leaf_lo, leaf_hi).sum()) / root)


def _centroid(lo, hi, P):
    if P["centroid_sum_first"]:
        return ((lo + hi) * F32(0.5)).astype(F32)
    return (F32(0.5) * lo + F32(0.5) * hi).astype(F32)


def _params(mutant):
    assert mutant is None or mutant in MUTANTS, mutant
    m = lambda name: mutant == name
    return dict(bins=32 if m("32 bins") else BINS, small=8 if m("kSmall 8") else SMALL, mid=2048 if m("kMid 2048") else MID,
                sah_depth=1 << 30 if m("depth guards off") else SAH_DEPTH, small_depth=1 << 30 if m("depth guards off") else SMALL_DEPTH,
                high_bin=m("ties to the higher bin"), high_axis=m("ties to the higher axis"), cost_f32=m("costs compared in float32"), right_double=m("right_area kept in double"),
                no_margin=m("no half-bin margin"), domain_is_box=m("child domain = child box"), centroid_sum_first=m("SAH centroid (lo + hi) * 0.5f"),
                unstable=m("unstable partition"), sort_from_original=m("k_small sorts from the original order"))


def build(leaf_lo, leaf_hi, mutant=None):
    leaf_lo, leaf_hi = np.ascontiguousarray(leaf_lo, F32).reshape(-1, 3), np.ascontiguousarray(leaf_hi, F32).reshape(-1, 3)
    T = leaf_lo.shape[0]
    if T < 3:
        return None
    P = _params(mutant)
    with np.errstate(all="ignore"):
        tree = _build(leaf_lo, leaf_hi, T, P)
    if mutant is None:
        COUNTS.update(tree.counts)
    return tree


def _build(leaf_lo, leaf_hi, T, P):
    nb, small_max, mid = P["bins"], P["small"], P["mid"]
    tree = Tree(T)
    C = tree.counts
    idx = np.arange(T, dtype=np.int64)
    small = []                                   # (b, e, k, depth)
    if T <= small_max:                           # the whole scene is one small range at depth 0
        small.append((0, T, 0, 0))
        ranges = []
    else:                                        # k_root_range: the bounds of k_soup's centroids, (lo + hi) * 0.5f
        c0 = ((leaf_lo + leaf_hi) * F32(0.5)).astype(F32)
        ranges = [(0, T, 0, 0, c0.min(0), c0.max(0))]
    host_big, level = int(T > mid), 0            # what the host believes about ranges of more than MID leaves: it looks every fourth level
    bin_ids = np.arange(nb)
    while ranges:
        sizes = np.array([r[1] - r[0] for r in ranges])
        big = sorted((r[0], r[1]) for r in ranges if r[1] - r[0] > mid)
        C[EVENTS[0]] += len(big)
        C[EVENTS[1]] += sum((big[i][1] - 1) // WINDOW == big[i + 1][0] // WINDOW for i in range(len(big) - 1))
        C[EVENTS[2]] += int(512 < len(ranges) <= 4096)
        C[EVENTS[3]] += int(4096 < len(ranges) <= 16384)
        C[BATCH_8] += int(len(ranges) > 16384)
        C[EVENTS[4]] += int(bool(big) and bool((sizes <= mid).any()))
        full = host_big == 0                     # k_mid<true> is the level's only kernel
        nxt = []
        for b, e, k, depth, dlo, dhi in ranges:
            n = e - b
            ids = idx[b:e]
            lo, hi = leaf_lo[ids], leaf_hi[ids]
            node_lo, node_hi = lo.min(0), hi.max(0)
            tree.node_lo[k], tree.node_hi[k], tree.size[k], tree.depth[k] = node_lo, node_hi, n, depth
            # bin_in: a flat side puts everything in bin 0
            c = _centroid(lo, hi, P)
            nonflat = dhi > dlo
            sc = F32(nb) / np.where(nonflat, dhi - dlo, F32(1)).astype(F32)
            x = ((c - dlo[None, :]).astype(F32) * sc[None, :]).astype(F32)
            bins = np.where(nonflat[None, :], np.fmin(np.fmax(x, F32(0)), F32(nb - 1)).astype(np.int64), 0).T        # [3, n]
            C[EVENTS[7]] += int(((c < dlo[None, :]) & nonflat[None, :]).sum())
            C[EVENTS[8]] += int(((c > dhi[None, :]) & nonflat[None, :]).sum())
            split = False
            if depth < P["sah_depth"]:           # (n > 2 holds: a range of the level loop has more than SMALL leaves)
                order = np.argsort(bins, axis=1, kind="stable")
                slo, shi = lo[order], hi[order]                                                                       # [3, n, 3], in bin order on each axis
                plo, phi = np.minimum.accumulate(slo, axis=1), np.maximum.accumulate(shi, axis=1)                     # boxes of the first i + 1 leaves in bin order
                qlo, qhi = np.minimum.accumulate(slo[:, ::-1], axis=1)[:, ::-1], np.maximum.accumulate(shi[:, ::-1], axis=1)[:, ::-1]   # of the leaves from i on
                cp = np.cumsum(np.bincount((bins + np.arange(3)[:, None] * nb).reshape(-1), minlength=3 * nb).reshape(3, nb), axis=1)   # leaves in bins 0 .. i
                ok = (cp > 0) & (cp < n) & (bin_ids[None, :] < nb - 1) & nonflat[:, None]
                li, ri = np.clip(cp - 1, 0, n - 1), np.clip(cp, 0, n - 1)
                ax = np.arange(3)[:, None]
                Llo, Lhi, Rlo, Rhi = plo[ax, li], phi[ax, li], qlo[ax, ri], qhi[ax, ri]                               # [3, nb, 3]
                cost = np.where(ok, half_area(Llo, Lhi) * cp + half_area(Rlo, Rhi) * (n - cp), np.inf)
                if P["cost_f32"]:
                    cost = cost.astype(F32)
                best = cost.min()
                if best < np.inf:
                    split = True
                    a_t, b_t = np.nonzero(cost == best)                                                               # ascending (axis, bin)
                    if P["high_axis"]:
                        a = int(a_t.max()); bn = int(b_t[a_t == a].min())
                    elif P["high_bin"]:
                        a = int(a_t.min()); bn = int(b_t[a_t == a].max())
                    else:
                        a, bn = int(a_t[0]), int(b_t[0])
            if split:
                tree.rule[k] = 0
                nl = int(cp[a, bn])
                go_left = bins[a] <= bn
                right = ids[~go_left]
                idx[b:e] = np.concatenate([ids[go_left], right[::-1] if P["unstable"] else right])
                lb_lo, lb_hi, rb_lo, rb_hi = Llo[a, bn].copy(), Lhi[a, bn].copy(), Rlo[a, bn].copy(), Rhi[a, bn].copy()
                if not P["domain_is_box"]:
                    w = F32((dhi[a] - dlo[a]) * F32(1.0 / nb))
                    plane = F32(dlo[a] + F32(w * F32(bn + 1)))
                    margin = F32(0) if P["no_margin"] else F32(F32(0.5) * w)
                    up, down = dhi.copy(), dlo.copy()
                    up[a], down[a] = np.fmin(dhi[a], F32(plane + margin)), np.fmax(dlo[a], F32(plane - margin))
                    lb_lo, lb_hi = np.fmax(lb_lo, dlo), np.fmin(lb_hi, up)
                    rb_lo, rb_hi = np.fmax(rb_lo, down), np.fmin(rb_hi, dhi)
            else:
                tree.rule[k] = 2 if depth >= P["sah_depth"] else 1
                nl = n // 2
                if P["domain_is_box"]:
                    lb_lo = rb_lo = node_lo; lb_hi = rb_hi = node_hi
                else:
                    lb_lo = rb_lo = np.fmax(node_lo, dlo); lb_hi = rb_hi = np.fmin(node_hi, dhi)
            for side, (cb, ce, ck, clo, chi) in enumerate(((b, b + nl, k + 1, lb_lo, lb_hi), (b + nl, e, k + nl, rb_lo, rb_hi))):
                cn = ce - cb
                if cn == 1:
                    tree.child[k, side] = ~int(idx[cb])
                    C[EVENTS[6 if full else 5]] += 1
                    continue
                tree.child[k, side] = ck
                if cn <= small_max:
                    small.append((cb, ce, ck, depth + 1))
                else:
                    nxt.append((cb, ce, ck, depth + 1, clo.astype(F32), chi.astype(F32)))
        if (level & 3) == 3 and host_big:
            host_big = sum(r[1] - r[0] > mid for r in nxt)
        ranges, level = nxt, level + 1
    if small:
        _small(tree, np.array(small, np.int64).reshape(-1, 4), idx, leaf_lo, leaf_hi, P)
    for r, name in enumerate(RULES):
        C[name] += int((tree.rule == r).sum())
    assert (tree.rule >= 0).all() and (tree.child != np.iinfo(np.int32).min).all()
    return tree


def _small(tree, sr, idx, leaf_lo, leaf_hi, P):
    """k_small for all the small ranges at once: arrays [ranges, SMALL].  One byte order per leaf (`ordr`: a leaf's place in its range); every sub-range computes its box, then
    -- if n > 2, the sub-depth is below SMALL_DEPTH and range depth + sub-depth below SAH_DEPTH -- is sorted (stable insertion sort: a stable sort) by centroid on x, then y,
    then z, each from the order the one before left; after each sort every position is a candidate, cost = half_area(left) * i + (double)(float)half_area(right) * (n - i),
    the best by strict < over (axis, i); one more sort on the winning axis unless that is z.  The children inherit the order that leaves."""
    W = P["small"]
    S, T = sr.shape[0], leaf_lo.shape[0]
    sb, se, sk, sd = sr.T
    n0 = se - sb
    leaf = idx[np.minimum(sb[:, None] + np.arange(W)[None, :], T - 1)]                     # [S, W] (past a range's end: unused)
    blo, bhi = leaf_lo[leaf], leaf_hi[leaf]                                                # [S, W, 3]
    cen = _centroid(blo, bhi, P)
    ordr = np.tile(np.arange(W), (S, 1))
    s, b, n, d, k = np.arange(S), np.zeros(S, np.int64), n0.copy(), np.zeros(S, np.int64), sk.copy()
    while s.size:
        nxt = []
        for nn in np.unique(n):
            nn = int(nn)
            m = n == nn
            ss, bb, dd, kk = s[m], b[m], d[m], k[m]
            cols = bb[:, None] + np.arange(nn)[None, :]
            o = ordr[ss[:, None], cols]                                                    # [M, nn]
            tree.node_lo[kk], tree.node_hi[kk] = blo[ss[:, None], o].min(1), bhi[ss[:, None], o].max(1)
            total = sd[ss] + dd
            tree.size[kk], tree.depth[kk] = nn, total
            g = (dd < P["small_depth"]) & (total < P["sah_depth"]) if nn > 2 else np.zeros(ss.size, bool)
            tree.rule[kk] = 4 if nn == 2 else np.where(g, 3, np.where(dd >= P["small_depth"], 5, 6))
            nl = np.full(ss.size, nn // 2)
            if g.any():
                sg, o_in = ss[g], o[g]
                rows = sg[:, None]
                cur = o_in
                best_cost, best_axis, best_nl = np.full(sg.size, np.inf), np.full(sg.size, -1), np.full(sg.size, nn // 2)
                i = np.arange(1, nn)
                for a in range(3):
                    src = o_in if P["sort_from_original"] else cur
                    cur = np.take_along_axis(src, np.argsort(cen[rows, src, a], axis=1, kind="stable"), 1)
                    lo_s, hi_s = blo[rows, cur], bhi[rows, cur]
                    ra = half_area(np.minimum.accumulate(lo_s[:, ::-1], axis=1)[:, ::-1], np.maximum.accumulate(hi_s[:, ::-1], axis=1)[:, ::-1])   # of the leaves from i on
                    if not P["right_double"]:
                        ra = ra.astype(F32).astype(F64)
                    la = half_area(np.minimum.accumulate(lo_s, axis=1), np.maximum.accumulate(hi_s, axis=1))                                       # of the first i + 1 leaves
                    cost = la[:, :-1] * i[None, :] + ra[:, 1:] * (nn - i)[None, :]
                    if P["cost_f32"]:
                        cost = cost.astype(F32)
                    j = np.argmin(cost, axis=1)                                                                                                    # the first of equal costs
                    cj = cost[np.arange(sg.size), j]
                    better = cj < best_cost
                    best_cost, best_axis, best_nl = np.where(better, cj, best_cost), np.where(better, a, best_axis), np.where(better, j + 1, best_nl)
                for a in (0, 1):                                                           # the sub-range is in z order now: once more on the winning axis
                    again = best_axis == a
                    if again.any():
                        src = cur[again]
                        cur[again] = np.take_along_axis(src, np.argsort(cen[sg[again][:, None], src, a], axis=1, kind="stable"), 1)
                o = o.copy()
                o[g] = cur
                ordr[ss[:, None], cols] = o
                nl[g] = best_nl
            nr = nn - nl
            one_l, one_r = nl == 1, nr == 1
            tree.child[kk, 0] = np.where(one_l, ~leaf[ss, o[:, 0]], kk + 1)
            tree.child[kk, 1] = np.where(one_r, ~leaf[ss, o[np.arange(ss.size), nl]], kk + nl)
            nxt.append((ss[~one_l], bb[~one_l], nl[~one_l], dd[~one_l] + 1, kk[~one_l] + 1))
            nxt.append((ss[~one_r], (bb + nl)[~one_r], nr[~one_r], dd[~one_r] + 1, (kk + nl)[~one_r]))
        s, b, n, d, k = (np.concatenate(x) for x in zip(*nxt))


def first_difference(tree, child, node_lo, node_hi):
    """None if the arrays are the model's tree bit for bit; else a line about the first node, in pre-order, where they are not"""
    bad = (tree.child != child).any(1) | (tree.node_lo.view(np.uint32) != np.ascontiguousarray(node_lo, F32).view(np.uint32)).any(1) | \
          (tree.node_hi.view(np.uint32) != np.ascontiguousarray(node_hi, F32).view(np.uint32)).any(1)
    if not bad.any():
        return None
    k = int(np.flatnonzero(bad)[0])
    return (f"{int(bad.sum())} of {bad.size} nodes differ; the first is {tree.describe(k)}: child {child[k].tolist()}, the model's {tree.child[k].tolist()}; "
            f"box {node_lo[k].tolist()} .. {node_hi[k].tolist()}, the model's {tree.node_lo[k].tolist()} .. {tree.node_hi[k].tolist()}")
