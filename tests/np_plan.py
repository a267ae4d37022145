"""The fused frame's wave plan restated in numpy and plain Python integers, from DESIGN.md 3 ("Wave plan") and the comments of art_plan.hip / art_internal.h (PlanArgs) --
what tests/test_wave_plan.py compares k_plan and the host's first table with, bit for bit.  Everything is an integer but the adaptive target, which is float32 in the
kernel's order of operations.

A TABLE is an array [n, 2] of uint32 wave items (8x8 block, mask over the block's sixteen 2x2 cells); workgroup j of a launch runs item j, on XCD j % 8.  A block's LEVEL
says how it is dealt: 0 one wave (mask 0xFFFF), 1 four quadrant waves, 2 sixteen cell waves.  Table layout, before the deal: the level-2 blocks' sixteen cells each (blocks
ascending), the level-1 blocks' four quadrants each (ascending), idle waves (0, 0) up to a whole group of 32, then every 256-pixel block of the launch order as its four
8x8 blocks -- mask 0 (an idle wave) where the block is split.  The deal then moves, inside every FULL group of 32 positions, position 32 g + 4 x + k to 32 g + 8 k + x: the
four waves of launch block 8 g + x run on XCD x.

COUNTS says which branches the calls so far went through (the tests assert that their inputs reach every one)."""
import collections

import numpy as np

U32 = 0xFFFFFFFF
QUADS = (0x0033, 0x00CC, 0x3300, 0xCC00)   # the four 4x4-pixel quadrants of an 8x8 block as cell masks (cell = (y / 2) * 4 + x / 2)
PAD_GROUP = 32
COUNTS = collections.Counter()


def deal(j, total):
    """where position j of a table of `total` items goes (j: an int or an array)"""
    j = np.asarray(j, np.int64)
    g = j >> 5
    dealt = 32 * g + 8 * (j & 3) + ((j & 31) >> 2)
    return np.where((g + 1) * 32 <= total, dealt, j)


def first_items(order):
    """the table of a fresh frame layout: every block one wave, in the launch order, dealt"""
    order = np.asarray(order, np.int64)
    blocks = (order[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    out = np.zeros((blocks.size, 2), np.uint32)
    out[deal(np.arange(blocks.size), blocks.size)] = np.stack([blocks, np.full(blocks.size, 0xFFFF)], 1)
    return out


def layout(level, order):
    """the table that deals every block as `level` says (the layout above, dealt)"""
    level, order = np.asarray(level, np.int64), np.asarray(order, np.int64)
    two, one = np.flatnonzero(level == 2), np.flatnonzero(level == 1)
    parts = [np.stack([np.repeat(two, 16), np.tile(1 << np.arange(16), two.size)], 1), np.stack([np.repeat(one, 4), np.tile(np.array(QUADS), one.size)], 1)]
    heavy = 16 * two.size + 4 * one.size
    pad = -heavy % PAD_GROUP
    COUNTS["padding items" if pad else "no padding"] += 1
    COUNTS[f"heavy / 4 = {heavy // 4 % 8} mod 8"] += 1
    parts.append(np.zeros((pad, 2), np.int64))
    blocks = (order[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    parts.append(np.stack([blocks, np.where(level[blocks] != 0, 0, 0xFFFF)], 1))
    flat = np.concatenate(parts).astype(np.uint32)
    total = flat.shape[0]
    COUNTS["total below 32" if total < 32 else ("a partial last group" if total % 32 else "whole groups only")] += 1
    out = np.zeros_like(flat)
    out[deal(np.arange(total), total)] = flat
    return out


def f32_of_u64(n):
    """float32(n) for an integer 0 <= n < 2^64, rounded to nearest, ties to even, in one step"""
    n = int(n)
    bits = n.bit_length()
    if bits <= 24:
        return np.float32(n)
    sh = bits - 24
    q, r, half = n >> sh, n & ((1 << sh) - 1), 1 << (sh - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return np.float32(np.ldexp(np.float64(q), sh))   # (q <= 2^24: exact)


def host_share(alpha, frames_per_launch, in_flight):
    """the share the host hands k_plan: alpha * B * launches in flight / (256 CUs * 32 waves), left to right in float32"""
    return np.float32(np.float32(np.float32(alpha) * np.float32(frames_per_launch)) * np.float32(in_flight)) / np.float32(8192.0)


def in_flight(frames_in_flight, hw_queues=0):
    """launches the plan counts as in flight: min(frames in flight, hardware queues (0: HIP's default of 4), 4), at least 1"""
    return max(1, min(frames_in_flight, hw_queues if hw_queues else 4, 4))


def target(total_steps, share, min_steps, fixed_steps):
    """the step target a wave may reach before its block is split"""
    if fixed_steps:
        COUNTS["fixed target"] += 1
        return int(fixed_steps)
    prod = np.float32(share) * f32_of_u64(total_steps)
    assert 0 <= prod < 2.0 ** 32, "the model stays where the conversion to uint32 is defined"
    t = int(prod)                                        # towards zero
    COUNTS["min_steps wins" if min_steps >= t else "the share wins"] += 1
    return max(int(min_steps), t)


def levels_for(worst, level, T):
    """every block's next level at target T, in uint32 arithmetic (4 T and 4 w wrap as they do in the kernel): up as soon as the slowest wave outlasts the target (level 0: past
    four targets straight to sixteen waves), down one level only with a clear margin -- a quarter of the block's slowest part would still be under half the target"""
    w, old = worst.astype(np.int64), level.astype(np.int64)
    w4, T4, half = (w * 4) & U32, (T * 4) & U32, T // 2
    l0 = np.where(w > T4, 2, np.where(w > T, 1, 0))
    l1 = np.where(w > T, 2, np.where(w4 < half, 0, 1))
    l2 = np.where(w4 < half, 1, 2)
    return np.where(old == 0, l0, np.where(old == 1, l1, l2))


def _count_thresholds(w, old, T):
    """which thresholds of the level rule the blocks sit on, or one beside, at the target the plan was made with"""
    edge = (T // 2 - 1) // 4                                 # the largest w with 4 w < T / 2
    for d in (-1, 0, 1):
        COUNTS[f"level 0: w = T{d:+d}"] += int(((old == 0) & (w == T + d)).any())
        COUNTS[f"level 0: w = 4T{d:+d}"] += int(((old == 0) & (w == 4 * T + d)).any())
        for o in (1, 2):
            COUNTS[f"level {o}: w = T{d:+d}"] += int(((old == o) & (w == T + d)).any())
    for o in (1, 2):
        for k, name in enumerate(("the last w under the margin", "the first w at the margin", "w past the margin")):
            COUNTS[f"level {o}: {name}"] += int(((old == o) & (w == edge + k)).any())


def plan(items_in, cost, level, n64, n256, order, cap, share, min_steps, fixed_steps):
    """one k_plan launch on a cleared `worst`: (the new table or None, the levels afterwards, result) with result[0..5] = items of the new table, 1 = a new table was written,
    blocks in four, blocks in sixteen, the target, the slowest wave; None for a word the kernel leaves alone"""
    items_in, cost, level = np.asarray(items_in, np.uint32).reshape(-1, 2), np.asarray(cost, np.uint32), np.asarray(level, np.uint8)
    assert n64 == 4 * n256 and level.size == n64 and cost.size == items_in.shape[0]
    live = items_in[:, 1] != 0
    COUNTS["mask 0 items ignored"] += int((~live).sum() > 0)
    worst = np.zeros(n64, np.uint32)
    np.maximum.at(worst, items_in[live, 0], cost[live])
    total_steps = int(cost[live].astype(np.uint64).sum(dtype=np.uint64)) if live.any() else 0   # (64 bits, as the kernel's)
    COUNTS["sum above 2^32" if total_steps > 2 ** 32 else ("sum above 2^24" if total_steps > 2 ** 24 else "sum below 2^24")] += 1
    least = np.full(n64, U32, np.uint32)
    np.minimum.at(least, items_in[live, 0], cost[live])
    COUNTS["a split block's parts differ"] += int(((np.bincount(items_in[live, 0], minlength=n64) > 1) & (least != worst)).any())
    T = target(total_steps, share, min_steps, fixed_steps)
    old = level.astype(np.int64)
    for attempt in range(8):
        lv = levels_for(worst, level, T)
        N1, N2, ups, downs, split = int((lv == 1).sum()), int((lv == 2).sum()), int((lv > old).sum()), int((lv < old).sum()), int((old != 0).sum())
        if (n64 + (n64 & 3) + 4 * N1 + 16 * N2 + PAD_GROUP) & U32 <= cap:   # the table fits, padding included
            COUNTS[f"fits at attempt {attempt}"] += 1
            _count_thresholds(worst.astype(np.int64), old, T)
            break
        if attempt == 7:                                                    # no target fits: the plan stays
            COUNTS["fallback"] += 1
            lv, N1, N2, ups, downs = old, 0, 0, 0, 0
        T = (T + T // 2) & U32                                              # (also behind the eighth attempt: the reported target has grown eight times)
    for o in range(3):
        for n in range(3):
            if ((old == o) & (lv == n)).any():
                COUNTS[f"level {o} -> {n}"] += 1
    wmax = int(worst.max()) if n64 else 0
    if fixed_steps:
        changed = ups + downs != 0
        COUNTS["fixed: changed" if changed else "fixed: unchanged"] += 1
    else:
        margin = max(16, split // 4)
        changed = ups != 0 or downs > margin
        if ups == 0:
            COUNTS["adaptive, no ups: downs " + ("above" if downs > margin else ("at" if downs == margin else "below")) + f" the margin ({'16' if margin == 16 else 'split / 4'})"] += 1
        else:
            COUNTS["adaptive: ups"] += 1
    if not changed:
        return None, level.copy(), [None, 0, None, None, T, wmax]
    table = layout(lv, order)
    return table, lv.astype(np.uint8), [table.shape[0], 1, N1, N2, T, wmax]


# ---- what every table must satisfy, whoever made it ----------------------------------------------------------------------------------------------------------------------
def check_table(items, level, order):
    """`items` deals the blocks as `level` says: every block's sixteen cells exactly once, a split block as its four quadrants or its sixteen cells, an idle wave where
    the launch order meets a split block; and the XCD property: in every full group of 32 positions behind the split blocks' parts, the item at position j belongs to the
    launch block that the order put at a launch position of the same residue mod 8 -- in fact to launch block 8 g + j % 8 of that group, as its 8x8 block (j % 32) / 8"""
    items, level, order = np.asarray(items, np.int64).reshape(-1, 2), np.asarray(level, np.int64), np.asarray(order, np.int64)
    n256, n64, total = order.size, level.size, items.shape[0]
    assert n64 == 4 * n256 and np.array_equal(np.sort(order), np.arange(n256))
    blocks, masks = items[:, 0], items[:, 1]
    assert (blocks < n64).all() and (masks <= 0xFFFF).all()
    live = masks != 0
    cells = (masks[live][:, None] >> np.arange(16)[None, :]) & 1                                    # [live item, cell]
    cover = np.zeros((n64, 16), np.int64)
    np.add.at(cover, blocks[live], cells)
    assert (cover == 1).all(), "a cell of some block is traced twice or not at all"
    waves = np.bincount(blocks[live], minlength=n64)
    assert np.array_equal(waves, np.array([1, 4, 16])[level]), "a block's waves are not what its level says"
    assert np.isin(masks[(level[blocks] == 1) & live], QUADS).all()                                 # (sixteen waves over sixteen cells, each once, are single cells)
    start = total - 4 * n256                                                                        # the launch order's part
    assert start >= 0 and start % PAD_GROUP == 0 and start - (16 * (level == 2).sum() + 4 * (level == 1).sum()) in range(PAD_GROUP)
    where = np.empty(n256, np.int64)
    where[order] = np.arange(n256)                                                                  # 256-pixel block -> launch position
    j = np.arange(start, total)
    full = (j // 32 + 1) * 32 <= total
    L = where[blocks[j] >> 2]
    assert (L[full] % 8 == j[full] % 8).all(), "XCD property: a launch block's wave is not on the XCD the order gave the block"
    assert (L[full] == 8 * ((j[full] - start) // 32) + j[full] % 8).all() and ((blocks[j] & 3)[full] == (j[full] % 32) // 8).all()
    assert (L[~full] == (j[~full] - start) // 4).all() and ((blocks[j] & 3)[~full] == j[~full] % 4).all()   # the partial last group stays in launch order
    assert np.array_equal(masks[j], np.where(level[blocks[j]] != 0, 0, 0xFFFF))
    assert (masks[:start][~live[:start]] == 0).all() and (blocks[:start][~live[:start]] == 0).all()  # padding: (0, 0)
    return int((level == 1).sum()), int((level == 2).sum())


def levels_of_table(items, n64):
    """the level every block has in a table, from the table alone: 0 one wave, 1 four, 2 sixteen"""
    items = np.asarray(items, np.int64).reshape(-1, 2)
    waves = np.bincount(items[items[:, 1] != 0, 0], minlength=n64)
    assert np.isin(waves, (1, 4, 16)).all()
    return np.searchsorted(np.array([1, 4, 16]), waves).astype(np.uint8)
