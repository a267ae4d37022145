"""The fused frame's wave plan -- k_plan (art_frame.hip) and its host side (art_plan.hip) -- against tests/np_plan.py, bit for bit: all of it is integers but the adaptive
target, which the model computes in float32 in the kernel's order, so nothing here has a tolerance.

(a) without a device: the model's own tables deal every block's sixteen cells exactly once and keep the XCD property, and the inputs of (b) reach every branch the plan has
    (the model counts them: np_plan.COUNTS);
(b) art_parity_plan: one k_plan launch on made-up buffers for every case of (a), twice on the same state -- table, levels, the cleared scratch, the result words;
(c) real frames: a chain of sampled frames, every adopted table the model's plan of the one before from the steps its waves counted;
(d) the levels on the device and the table the host runs stay in step through everything that resets, rebuilds, moves or rewinds.

A note on the cases: the split blocks' parts are a multiple of four items as they are (16 N2 + 4 N1), so "every residue of `heavy` mod 4" is one residue; the cases reach every
residue of heavy / 4 mod 8 instead, which is what the padding to whole groups of 32 and the deal behind it see."""
import ctypes as C
import os

import numpy as np
import pytest

import np_plan
from helpers import R  # noqa: F401  (module fixture)

SIZES = [1, 2, 7, 8, 9, 255, 256, 257, 513, 8160]        # 256-pixel blocks: n64 below, at and above 1024 threads' worth; tables below 32 items, with a partial last group, a 4K frame's
HUGE = 0xFFFFFFF0                                        # what an idle wave "counted": must be ignored
UNWRITTEN = 0xFFFFFFFF
RESULT_IN = np.arange(8, dtype=np.uint32) + 0xABCD0000   # what the result words hold before a launch
SHARE_1 = np_plan.host_share(0.7, 1, 1)                  # one frame per launch, one launch in flight


def _grown(T, k):
    for _ in range(k):
        T += T // 2
    return T


def _threshold_costs(T):
    """(old level, slowest wave) pairs on every threshold of the level rule at target T and one either side"""
    half = T // 2
    edge = (half - 1) // 4                                # the largest w with 4 w < T / 2
    down = sorted({max(edge - 1, 0), edge, edge + 1, edge + 2})
    out = [(0, w) for w in (T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1)]
    for old in (1, 2):
        out += [(old, w) for w in (T - 1, T, T + 1)] + [(old, w) for w in down]
    return out


class Case:
    def __init__(self, name, n256, level_in, block_cost, cap=None, share=SHARE_1, min_steps=150, fixed_steps=0, seed=0):
        self.name, self.n256, self.n64 = name, n256, 4 * n256
        self.order = np.random.default_rng(1000 * n256 + seed).permutation(n256).astype(np.uint32)
        self.level_in, self.block_cost = np.asarray(level_in, np.uint8), np.asarray(block_cost, np.uint32)
        assert self.level_in.size == self.n64 and self.block_cost.size == self.n64
        self.block_cost2 = (self.block_cost[::-1] // 2 + np.arange(self.n64, dtype=np.uint32) % 7).astype(np.uint32)   # the second launch: other blocks are the slow ones
        self.cap = 17 * self.n64 + 64 if cap is None else (self.n64 + self.n64 // 2 + 64 if cap == "host" else cap)   # room for every block in sixteen | what the host allocates
        self.share, self.min_steps, self.fixed_steps = np.float32(share), min_steps, fixed_steps

    def __repr__(self):
        return f"{self.name} (n256 {self.n256})"


def item_costs(items, block_cost):
    """what every wave of a table counted, given the slowest wave of every block: an unsplit block's wave counts just that; of a split block's parts one (which one depends
    on the block) counts it and the others less; idle waves carry HUGE"""
    items = np.asarray(items, np.int64)
    b, m = items[:, 0], items[:, 1]
    live = m != 0
    parts = np.bincount(b[live], minlength=block_cost.size)[b]
    cell = np.zeros(items.shape[0], np.int64)
    cell[live] = np.floor(np.log2((m[live] & -m[live]).astype(np.float64))).astype(np.int64)     # lowest cell of the part: 0..15 of sixteen, 0 2 8 10 of four
    idx = np.where(parts == 16, cell, np.where(parts == 4, (cell >> 1 & 1) | (cell >> 2 & 2), 0))
    bc = block_cost.astype(np.int64)[b]
    cost = np.where(idx == b % np.maximum(parts, 1), bc, bc * ((idx * 7 + 3) % 11) // 11)
    return np.where(live, cost, HUGE).astype(np.uint32)


def cases_for(n256):
    n64 = 4 * n256
    rng = np.random.default_rng(n256)
    out = []

    def filler(T):                                        # a few blocks with small costs, the rest 0: the frame's steps stay small
        c = np.zeros(n64, np.int64)
        some = rng.permutation(n64)[:200]
        c[some] = rng.integers(0, max(T // 8, 2), some.size)
        return c

    def thresholds(name, T, **kw):                        # the pairs in chunks of as many blocks as there are
        pairs = _threshold_costs(T)
        for i in range(0, len(pairs), n64):
            chunk = pairs[i:i + n64]
            level, cost = rng.integers(0, 3, n64), filler(T)
            at = rng.permutation(n64)[:len(chunk)]
            level[at], cost[at] = [p[0] for p in chunk], [p[1] for p in chunk]
            out.append(Case(f"{name} {i // n64}", n256, level, cost, seed=i, **kw))
            yield out[-1], at

    for _ in thresholds("thresholds, fixed target", 400, fixed_steps=400):
        pass
    for _ in thresholds("thresholds, min_steps wins", 150, min_steps=150):
        pass
    if n64 >= 28:                                         # the same with the share winning: one more block carries what the frame's steps lack for the target wanted
        T = 2000
        for case, at in list(thresholds("thresholds, the share wins", T, min_steps=150)):
            ballast = int(np.setdiff1d(np.arange(n64), at)[0])
            case.level_in[ballast] = 0
            items = np_plan.layout(case.level_in, case.order)
            for extra in range(64):                      # (float32: the exact quotient may round a step short)
                case.block_cost[ballast] = 0
                rest = int(item_costs(items, case.block_cost)[items[:, 1] != 0].sum(dtype=np.uint64))
                case.block_cost[ballast] = int(np.ceil((T + 0.5) / float(SHARE_1))) - rest + extra * 64
                total = int(item_costs(items, case.block_cost)[items[:, 1] != 0].sum(dtype=np.uint64))
                if int(SHARE_1 * np_plan.f32_of_u64(total)) == T:
                    break
            else:
                raise AssertionError("no ballast gives the target")
    # T never grows from 1: the table that does not fit falls back at target 1, the one that fits is written at target 1
    for cap in (n64 + 31, None):
        out.append(Case(f"fixed target 1, cap {cap}", n256, rng.integers(0, 3, n64), rng.integers(0, 4, n64), cap=cap, fixed_steps=1))
    # the retry loop: three blocks leave level 2 when the target grows for the 1st, 3rd and 7th time, one never does; cap = what attempt a needs
    T0 = 100
    for a, fixed in ((0, True), (1, False), (3, True), (7, False), (8, True), (8, False)):
        cost, level = rng.integers(0, T0 + 1, n64), np.zeros(n64, np.int64)
        at = rng.permutation(n64)[:4]
        cost[at] = [4 * _grown(T0, 0) + 1, 4 * _grown(T0, 2) + 1, 4 * _grown(T0, 6) + 1, 4 * _grown(T0, 8) + 1]
        if a == 8:
            level, cap = rng.integers(0, 3, n64), n64 + 31              # nothing fits (a table needs n64 + 32 at least): the levels stay as they came
        else:
            Ta = _grown(T0, a)                                          # (blocks that left level 2 early are below the target itself by now)
            cap = n64 + 16 * int((cost[at] > 4 * Ta).sum()) + 4 * int(((cost[at] > Ta) & (cost[at] <= 4 * Ta)).sum()) + 32
        out.append(Case(f"fits at attempt {a}" if a < 8 else "nothing fits", n256, level, cost, cap=cap, seed=a, **(dict(fixed_steps=T0) if fixed else dict(min_steps=T0, share=2.0 ** -40))))
    # the adaptive rule with no block going up: `downs` at, below and above max(16, split / 4)
    for split, margin in ((min(40, n64 - 4), 16), (100, 25)):
        if n64 < 24 or split > n64 - 4:
            continue
        assert max(16, split // 4) == margin
        for downs in (margin - 1, margin, margin + 1):
            level, cost = np.zeros(n64, np.int64), np.full(n64, 10, np.int64)
            at = rng.permutation(n64)[:split]
            level[at], cost[at] = 1 + np.arange(split) % 2, 100             # stays: 100 <= 150 and 4 * 100 >= 75
            cost[at[:downs]] = 0                                            # goes down a level
            out.append(Case(f"adaptive, {downs} of {split} split blocks go down", n256, level, cost, min_steps=150, share=2.0 ** -40))
    # 64-bit sums; the share (three launches in flight) wins over min_steps
    for big, name in ((5_000_000, "2^24"), (0xF0000000, "2^32")):
        cost, level = rng.integers(0, 1000, n64), rng.integers(0, 3, n64)
        at = rng.permutation(n64)[:4]
        cost[at], level[at] = big, 0
        out.append(Case(f"steps above {name}", n256, level, cost, share=np_plan.host_share(0.7, 1, 3)))
    # every residue of heavy / 4 mod 8: one block to sixteen waves, r blocks to four
    if n64 >= 8:
        for r in range(8):
            cost = np.zeros(n64, np.int64)
            at = rng.permutation(n64)[:r + 1]
            cost[at[0]], cost[at[1:]] = 4 * 300 + 1, 301
            out.append(Case(f"heavy / 4 = {4 + r}", n256, np.zeros(n64, np.int64), cost, fixed_steps=300, seed=r))
    # anything goes
    for seed in range(4):
        out.append(Case(f"random {seed}", n256, rng.integers(0, 3, n64), rng.integers(0, 1500, n64), seed=seed, cap="host" if seed >= 2 else None,
                        **(dict(fixed_steps=300) if seed % 2 else dict(share=SHARE_1 * np.float32(64.0)))))
    return out


_CASES = {}


def cases(n256):
    if n256 not in _CASES:
        _CASES[n256] = cases_for(n256)
    return _CASES[n256]


def runs_of(case):
    """the two launches of a case: (sampled table, what its waves counted, the levels before, the model's plan)"""
    items, level = np_plan.layout(case.level_in, case.order), case.level_in
    for block_cost in (case.block_cost, case.block_cost2):
        cost = item_costs(items, block_cost)
        want = np_plan.plan(items, cost, level, case.n64, case.n256, case.order, case.cap, case.share, case.min_steps, case.fixed_steps)
        yield items, cost, level, want
        items, level = (items if want[0] is None else want[0]), want[1]


BRANCHES = ([f"level {o} -> {n}" for o, n in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2))]
            + [f"level 0: w = {t}{d:+d}" for t in ("T", "4T") for d in (-1, 0, 1)] + [f"level {o}: w = T{d:+d}" for o in (1, 2) for d in (-1, 0, 1)]
            + [f"level {o}: {x}" for o in (1, 2) for x in ("the last w under the margin", "the first w at the margin", "w past the margin")]
            + [f"fits at attempt {a}" for a in (0, 1, 3, 7)] + ["fallback", "fixed target", "min_steps wins", "the share wins", "sum above 2^24", "sum above 2^32", "sum below 2^24"]
            + ["mask 0 items ignored", "a split block's parts differ", "padding items", "no padding", "total below 32", "a partial last group", "whole groups only"]
            + [f"heavy / 4 = {r} mod 8" for r in range(8)] + ["fixed: changed", "fixed: unchanged", "adaptive: ups"]
            + [f"adaptive, no ups: downs {x} the margin ({m})" for x in ("above", "at", "below") for m in ("16", "split / 4")])


def test_the_models_tables_deal_every_cell_once_and_the_cases_reach_every_branch():
    """(a) every table the model makes for the cases of (b), and the first table of every size, passes np_plan.check_table (every block's sixteen cells exactly once, split
    blocks as quadrants or cells, idle waves where the order meets a split block, the XCD property); a fallback leaves the levels and writes no table; and the cases
    together go through every branch named in BRANCHES"""
    np_plan.COUNTS.clear()
    for n256 in SIZES:
        order = cases(n256)[0].order
        np_plan.check_table(np_plan.first_items(order), np.zeros(4 * n256, np.uint8), order)
        assert np.array_equal(np_plan.first_items(order), np_plan.layout(np.zeros(4 * n256, np.uint8), order))
        for case in cases(n256):
            for items, cost, level, (table, level_out, result) in runs_of(case):
                np_plan.check_table(items, level, case.order)
                assert np.array_equal(np_plan.levels_of_table(items, case.n64), level)
                if table is None:
                    assert np.array_equal(level_out, level) and result[1] == 0
                else:
                    assert np_plan.check_table(table, level_out, case.order) == (result[2], result[3]) and result[0] == table.shape[0] <= case.cap
                if case.fixed_steps == 1:
                    assert result[4] == 1, "a target of 1 never grows"
    missing = [b for b in BRANCHES if not np_plan.COUNTS[b]]
    assert not missing, missing


def test_the_model_s_target_is_float32_in_the_kernels_order():
    """the conversion of the 64-bit sum rounds to nearest even in one step, the share is built left to right in float32, the product is truncated"""
    assert np_plan.f32_of_u64(2 ** 24 + 1) == 2.0 ** 24 and np_plan.f32_of_u64(2 ** 24 + 3) == 2.0 ** 24 + 4 and np_plan.f32_of_u64(2 ** 53 + 2 ** 29 + 1) == np.float32(2.0 ** 53 + 2.0 ** 30)
    assert np_plan.f32_of_u64(2 ** 64 - 1) == np.float32(2.0 ** 64)
    for n in (3, 2 ** 24 + 1, 2 ** 33 + 12345, 2 ** 40 - 1):
        assert np_plan.f32_of_u64(n) == np.float32(np.uint64(n))
    assert np_plan.host_share(0.7, 1, 3) == np.float32(np.float32(np.float32(0.7) * np.float32(3.0)) / np.float32(8192.0)) and np_plan.host_share(0.7, 1, 3).dtype == np.float32
    assert np_plan.target(10 ** 6, np.float32(0.5), 150, 0) == 500000 and np_plan.target(299, np.float32(0.5), 150, 0) == 150 and np_plan.target(10 ** 9, np.float32(0.5), 150, 77) == 77
    assert np_plan.in_flight(3) == 3 and np_plan.in_flight(8) == 4 and np_plan.in_flight(8, 2) == 2 and np_plan.in_flight(1, 32) == 1


# ---- (b) k_plan on made-up buffers ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare(R):
    r = R.Renderer((64, 64))                              # names the device, nothing else
    yield r
    r.close()


def _compare(got, want, level_before, cap, what):
    items_out, level_out, worst_out, result = got
    table, level_want, res_want = want
    assert not worst_out.any(), f"{what}: the scratch word of {int((worst_out != 0).sum())} blocks is not cleared"
    for i, v in enumerate(res_want):
        assert int(result[i]) == (int(RESULT_IN[i]) if v is None else v), f"{what}: result[{i}] is {int(result[i])}, the model's {v}"
    assert np.array_equal(result[6:], RESULT_IN[6:]), what
    assert np.array_equal(level_out, level_want), f"{what}: {int((level_out != level_want).sum())} levels differ"
    n = 0 if table is None else table.shape[0]
    assert n <= cap and (items_out[n:] == UNWRITTEN).all(), f"{what}: items written behind the table's end"
    if table is None:
        assert np.array_equal(level_out, level_before), what
    else:
        bad = np.flatnonzero((items_out[:n] != table).any(axis=1))
        assert bad.size == 0, f"{what}: {bad.size} of {n} items differ, the first at {int(bad[0])}: {items_out[bad[0]]} for {table[bad[0]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("n256", SIZES)
def test_k_plan_on_made_up_buffers_is_the_model(R, bare, n256):
    """(b) every case of the size, launched twice: the second launch starts from the levels and the scratch the first one LEFT ON THE DEVICE (the model from a cleared
    scratch) and samples the table the first one wrote, with other blocks slow"""
    before = R.Renderer.live_resources()
    for case in cases(n256):
        level_dev, worst_dev = case.level_in, np.zeros(case.n64, np.uint32)
        for run, (items, cost, level, want) in enumerate(runs_of(case)):
            assert np.array_equal(level_dev, level)
            got = bare.parity_plan(case.order, items, cost, level_dev, worst_dev, case.cap, case.share, case.min_steps, case.fixed_steps, result_in=RESULT_IN)
            _compare(got, want, level, case.cap, f"{case}, launch {run}")
            level_dev, worst_dev = got[1], got[2]
    assert R.Renderer.live_resources() == before


@pytest.mark.gpu
def test_parity_plan_refuses_what_the_kernel_would_index_with(R, bare):
    """the contract of art_parity_plan: an order that is no permutation, a block or a level out of range, an empty table capacity"""
    from araytracingjourney_amd._lib import ArtError
    order, items, cost, level, worst = np.arange(2), np_plan.first_items(np.arange(2)), np.zeros(8), np.zeros(8), np.zeros(8)
    bad_item = items.copy(); bad_item[3, 0] = 8
    for kw in (dict(order=[0, 0]), dict(order=[0, 2]), dict(items_in=bad_item), dict(level_in=[0, 0, 3, 0, 0, 0, 0, 0]), dict(cap=0)):
        args = dict(order=order, items_in=items, cost=cost, level_in=level, worst_in=worst, cap=64, share=0.0, min_steps=150, fixed_steps=0)
        args.update(kw)
        with pytest.raises(ArtError):
            bare.parity_plan(**args)


# ---- (c), (d): real frames ------------------------------------------------------------------------------------------------------------------------------------------------
def _renderer(R, get_scene, scene, extent, n_lights=1, **kw):
    from araytracingjourney_amd import scenes
    sc = get_scene(*scene)
    r = R.renderer_for_scene(sc, extent, n_lights=0, **kw)
    for d in scenes.sponza_lights(n_lights):
        r.lights_mut().push_dict(d)
    return r


def _hw_queues():
    return int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0)   # what Renderer tells the context


_ORDERS = {}


def _order_of(R, get_scene, scene, extent, **kw):
    """the launch order of a frame layout, read off the first table (a context whose plan is switched off keeps it): undone the deal, every four items are a 256-pixel
    block's; and that table is the model's first table of that order"""
    key = (scene, extent, tuple(sorted(kw.items())))
    if key not in _ORDERS:
        r = _renderer(R, get_scene, scene, extent, fixed_waves=True, **kw)
        r.render_frame()
        table = r.read_wave_plan()["items"]
        r.close()
        flat = table[np_plan.deal(np.arange(table.shape[0]), table.shape[0])]
        order = (flat[::4, 0] >> 2).astype(np.uint32)
        assert np.array_equal(np.sort(order), np.arange(order.size)) and np.array_equal(table, np_plan.first_items(order))
        _ORDERS[key] = order
    return _ORDERS[key]


def _in_step(r, what):
    """the levels on the device are the table's; -> the plan"""
    p = r.read_wave_plan()
    assert not p["pending"]
    of_table = np_plan.levels_of_table(p["items"], p["level"].size)
    assert np.array_equal(p["level"] != 0, of_table != 0), f"{what}: d_level says split for {int((p['level'] != 0).sum())} blocks, the current table splits {int((of_table != 0).sum())}"
    assert np.array_equal(p["level"], of_table), what
    assert r.stats()["split_blocks"] == int((of_table != 0).sum()), what
    return p


SCENES = {"cornell": (("cornell",), (64, 64)), "sponza_like": (("sponza_like", 0.12), (256, 128))}


@pytest.mark.gpu
@pytest.mark.parametrize("fixed_steps", [40, 0], ids=["fixed 40", "adaptive"])
@pytest.mark.parametrize("frames_in_flight", [1, 3])
@pytest.mark.parametrize("n_lights", [1, 4])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_adopted_table_is_the_models_plan_of_the_one_before(R, get_scene, name, n_lights, frames_in_flight, fixed_steps):
    """(c) six sampled frames in a row, nothing rendered between them: table k + 1 is plan(table k, steps k, levels k) exactly -- the share rebuilt from the context's frames
    in flight, frames per launch and queue count --, ART_STATS.split_blocks is N1 + N2 after every adoption, the count stays within the table's capacity, and every table
    passes np_plan.check_table (the XCD property among the rest)"""
    scene, extent = SCENES[name]
    order = _order_of(R, get_scene, scene, extent)
    n256, n64 = order.size, 4 * order.size
    r = _renderer(R, get_scene, scene, extent, n_lights=n_lights, frames_in_flight=frames_in_flight, tuning={"split_fixed_steps": fixed_steps})
    share = np_plan.host_share(0.7, 1, np_plan.in_flight(frames_in_flight, _hw_queues()))
    r.render_frame()
    before = _in_step(r, "the first frame")
    cap, adopted = before["cap"], 0
    assert cap == n64 + n64 // 2 + 64
    for k in range(6):
        items, steps = r.sample_wave_steps()
        assert np.array_equal(items, before["items"]), "the sampled table is the current one"
        table, level, result = np_plan.plan(items, steps, before["level"], n64, n256, order, cap, share, 150, fixed_steps)
        after = _in_step(r, f"sample {k}")
        for i, v in enumerate(result):
            assert v is None or int(after["result"][i]) == v, f"sample {k}: result[{i}] is {int(after['result'][i])}, the model's {v}"
        assert np.array_equal(after["level"], level), k
        if table is None:
            assert np.array_equal(after["items"], before["items"]) and after["replans"] == before["replans"] and after["cur"] == before["cur"], k
        else:
            assert np.array_equal(after["items"], table), k
            assert after["replans"] == before["replans"] + 1 and after["cur"] == before["cur"] ^ 1 and table.shape[0] <= cap, k
            assert r.stats()["split_blocks"] == result[2] + result[3], k
            adopted += 1
        assert np_plan.check_table(after["items"], after["level"], order) == (int((level == 1).sum()), int((level == 2).sum()))
        before = after
    if fixed_steps and name == "sponza_like":
        assert before["replans"] >= 1 and before["level"].any(), "a target of 40 steps splits blocks of this scene"
    r.close()


def _split_context(R, get_scene, **kw):
    """sponza_like with a target of 40 steps: the first frame is sampled, the second runs a table that splits blocks"""
    scene, extent = SCENES["sponza_like"]
    kw.setdefault("tuning", {"split_fixed_steps": 40})
    r = _renderer(R, get_scene, scene, extent, **kw)
    return r


def _frames(r, n, what):
    for i in range(n):
        r.render_frame()
        p = _in_step(r, f"{what}, frame {i}")
    return p


@pytest.mark.gpu
def test_levels_and_table_stay_in_step_through_resize_rebuild_tuning_and_moves(R, get_scene):
    """(d) after a resize, a scene rebuild, art_set_tuning and camera moves -- and a sync -- d_level is non-zero exactly where the current table splits a block"""
    r = _split_context(R, get_scene, frames_in_flight=2)
    assert _frames(r, 3, "fresh")["level"].any()
    r.resize((192, 96))
    assert _frames(r, 3, "after the resize")["level"].any()
    r.prepare_first_frame()                                  # art_scene_build
    assert _frames(r, 3, "after the rebuild")["level"].any()
    t = R.tuning_from_dict({"split_fixed_steps": 60, "hw_queues": _hw_queues(), "plan_moving_interval": 1})   # (a moving view is looked at again at once)
    from araytracingjourney_amd import _lib
    _lib.check(r._L.art_set_tuning(r._ctx, C.byref(t)))
    r.prepare_first_frame()
    assert _frames(r, 3, "after art_set_tuning")["level"].any()
    cam, replans = r.camera_mut(), r.read_wave_plan()["replans"]
    pos = np.array(cam.pos(), np.float64)
    for i in range(6):
        cam.set_pos(tuple(pos + 0.05 * (i + 1) * np.array([1.0, 0.2, 0.5])))
        r.render_frame(sync=False)
        r.render_frame()
        p = _in_step(r, f"camera move {i}")
    assert p["replans"] > replans, "the moved frames were planned again"
    r.close()


@pytest.mark.gpu
def test_a_plan_in_flight_survives_the_ring_rewind_of_a_sharded_job(R, get_scene):
    """(d) a sampled frame, then art_mgpu_create of a one-rank job over a host exchange: the job rewinds the frame ring behind the sample; the plan that landed is adopted
    with the levels k_plan committed, not dropped"""
    r = _split_context(R, get_scene, frames_in_flight=2, tile_output=True)
    r.upload_state()
    r.trace()                                                # frame 0: sampled, k_plan behind it
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def one_rank(send, nbytes, recv, root, stream):
        if recv:
            assert hip.hipMemcpyAsync(recv, send, nbytes, 3, stream) == 0   # hipMemcpyDeviceToDevice
    mg = R.MultiGpu(r, 0, 1, launches_per_gather=2, exchange=one_rank)
    p = _in_step(r, "behind art_mgpu_create")
    assert int(p["result"][1]) == 1 and p["level"].any() and p["replans"] == 1, "the sampled frame's plan split blocks"
    for _ in range(4):
        mg.trace()
    mg.flush()
    _in_step(r, "after two groups of the job")
    mg.close()
    r.close()


@pytest.mark.gpu
def test_a_switched_off_plan_keeps_its_levels_when_it_is_sampled(R, get_scene):
    """(d) ArtTuning.fixed_waves: art_sample_wave_steps runs k_plan all the same and nobody adopts its table -- the levels stay those of the first table, so the second
    sample's plan is made from the same state as the first one's and is the model's"""
    scene, extent = SCENES["sponza_like"]
    order = _order_of(R, get_scene, scene, extent)
    r = _split_context(R, get_scene, tuning={"split_fixed_steps": 40, "fixed_waves": 1})
    r.render_frame()
    first = _in_step(r, "a frame")
    assert np.array_equal(first["items"], np_plan.first_items(order))
    for k in range(2):
        items, steps = r.sample_wave_steps()
        assert np.array_equal(items, first["items"])
        p = _in_step(r, f"sample {k}")
        n64 = 4 * order.size
        table, level, result = np_plan.plan(items, steps, np.zeros(n64, np.uint8), n64, order.size, order, p["cap"], np_plan.host_share(0.7, 1, 1), 150, 40)
        assert table is not None and [int(x) for x in p["result"][:6]] == result, f"sample {k}: k_plan wanted the model's table"
        assert p["replans"] == 0 and r.stats()["split_blocks"] == 0
    r.close()
