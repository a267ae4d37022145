"""art_closest_points_multi (include/art.h): the K nearest triangles to a point, defined exactly and checked bit for bit.

The reference is tests/np_closest_multi.py: tests/np_closest.py's formulas (imported, not copied) over every (query, triangle) pair in numpy float32, the candidates
sorted by (d2_eff, global triangle id) and cut to K.  Nothing here has a tolerance: ids, the bits of d, u, v, a fourth word of 0, the bits of the point, the count.
A reference is computed once per set of inputs, to a depth of 9, shared by every K and never written.

The CPU tests tie the reference to art_closest_points' own (K = 1 is np_closest.brute_force bit for bit) and count, in the reference alone, what the GPU tests lean on:
every query of the shared sets has 8 candidates and more, and in hundreds of them the K-th and the (K+1)-th candidate share their d2_eff, so that the global id alone
decides who stays in the list.  Measured (queries contested at K = 2 / 4 / 8): sponza_like 0.05 761 / 911 / 1471 of 4096, the lattice 977 / 1403 / 1679 of 2197, the
clump 93 / 142 / 160 of 512, the chain 201 of 202 at every K.

Mutation checks, on scratch builds of the library run over the 43 GPU tests of this module (queries whose ids differ at each test's first failing comparison):
  * the list's tie rule flipped to `gid >` (the insertion's comparison and the entry test against the limit): 40 tests fail -- all but the one-triangle scene, the
    segments (no two candidates tie there) and the errors.  Both scenes at K = 1: 1914 and 949 of 4096, the reference's own counts of tied minima; the radii 2197 of
    8256; hostile at K = 8: the lattice 2197 of 2197, the chain 229 of 335, the soups 608 .. 660 of 666; the tree forms at K = 4, the same on all six: the chain 233 of
    407, the clump 425 of 515, Cornell 2949 of 4097; every knob 2864 of 4096; the sizes at n = 1; masks 649 of 2048, residency 870 of 1024, the scene as of the call
    1794 of 2048, the ring 959 of 1024, closest_surface_multi 1301 of 2048.
  * TravPoint::pop skipping spilled entries (the walk's own pop, inherited: the list changes nothing about the spill): 40 tests fail -- all but the one-triangle
    scene, the two cards of the residency test (16 triangles: nothing spills) and the errors.  Hostile at K = 8: the lattice 2197 of 2197, the chain 315 of 335, the
    soups 569 .. 664 of 666, the segments 517 of 800; the tree forms at K = 4: the chain 349 (373 on the canonical tree) of 407, the clump 418 .. 478 of 515, Cornell
    546 (1056) of 4097; every knob 4078 of 4096; both scenes at K = 1: 306 and 2492 of 4096 -- tests/test_query_forms.py's figure for the single-answer walk, whose
    18 tree-form tests fail beside these.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import np_closest as nc
import np_closest_multi as ncm
import test_closest_points as tcp
import test_query_forms as tqf
from helpers import chain_scene, degenerate_soup, lattice_scene, random_rays
from helpers import _bits, _layout_is_the_headers, _host, R, torch, _up  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = -0x5A5A5A5B   # tests/test_cast.py's: what oversized output buffers are filled with
N = 4096
KS = (1, 3, 4, 5, 8)    # 4 and 5 straddle the two instances of the kernel (lists of 4 and of 8)
WHO = b"art_closest_points_multi: "

_REF = {}


def _frozen(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def _ref(key, make):
    """{scene, T, q, tab} of a set of inputs: make() -> (scene, queries); computed once, shared, never written"""
    if key not in _REF:
        sc, q = make()
        T = nc.world_triangles(sc.primitives)
        q = np.ascontiguousarray(q, np.float32)
        q.setflags(write=False)
        _REF[key] = dict(scene=sc, T=T, q=q, tab=_frozen(ncm.table(T, q)), want={})
    return _REF[key]


def _scene_ref(get_scene, name, detail):
    """Cornell or sponza_like with tests/test_closest_points.py's queries: the origins of random_rays(4096, 7), r = inf"""
    return _ref((name, detail), lambda: (get_scene(name, detail), tcp.queries(random_rays(N, 7)[:, 0:3])))


def _named_ref(get_scene, name):
    if name == "lattice":
        return _ref(name, lambda: (lattice_scene(6), tcp._lattice_queries()))
    if name == "clump":
        return _ref(name, lambda: (degenerate_soup(1000, "one point"), tcp.queries(random_rays(512, 1000)[:, 0:3])))
    if name == "chain":
        return _ref(name, lambda: (chain_scene(64)[0], tcp.queries(chain_scene(64)[1][:, 0:3])))
    return _scene_ref(get_scene, name, 0.05 if name == "sponza_like" else 1.0)


def _want(ref, K, n=None):
    """the reference's records at K, of the first n queries"""
    if K not in ref["want"]:
        ref["want"][K] = _frozen(ncm.records(ref["T"], ref["q"], ref["tab"], K))
    return ref["want"][K] if n is None else tuple(w[:n] for w in ref["want"][K])


def _same(got, want, what=""):
    """ids, the bits of d, u, v, a fourth word of 0, the bits of the point, the counts"""
    (duv, ids, point, count), (rduv, rids, rpoint, rcount) = got, want
    assert duv.shape == rduv.shape and ids.shape == rids.shape and point.shape == rpoint.shape and count.shape == rcount.shape and count.dtype == np.uint8, what
    bad = (ids != rids).any(axis=(1, 2))
    assert not bad.any(), f"{what}: the ids of {int(bad.sum())} of {ids.shape[0]} queries differ (first: {np.flatnonzero(bad)[:5]}: {ids[bad][:1]} for {rids[bad][:1]})"
    bad = (_bits(duv)[..., :3] != _bits(rduv)[..., :3]).any(axis=(1, 2))
    assert not bad.any(), f"{what}: d, u, v of {int(bad.sum())} queries differ (first: {np.flatnonzero(bad)[:5]}: {duv[bad][:1]} for {rduv[bad][:1]})"
    assert not _bits(duv)[..., 3].any(), f"{what}: the fourth word is not 0"
    assert np.array_equal(_bits(point), _bits(rpoint)), f"{what}: the points differ"
    assert np.array_equal(count, rcount), f"{what}: the counts of {int((count != rcount).sum())} queries differ"


def _ask(r, torch, q, K, **kw):
    got = r.closest_points_multi(_up(torch, q), K, **kw)
    torch.cuda.synchronize()
    return _host(got)


def _patterned(torch, n, K):
    return (torch.full((n, K, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((n, K, 2), PATTERN, dtype=torch.int32, device="cuda"),
            torch.full((n, K, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"))


def _untouched(torch, out, n, what):
    for t in out[:3]:
        assert (t[n:].view(torch.int32) == PATTERN).all(), f"{what}: written beyond n"
    assert (out[3][n:] == 0xA5).all(), f"{what}: counts written beyond n"


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_ctypes_descriptor_is_the_headers():
    """ArtPointQueryMulti as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field: 64 bytes"""
    _layout_is_the_headers("ArtPointQueryMulti", 64, ["points_dev", "duv_dev", "ids_dev", "point_dev", "count_dev", "hip_stream", "n", "max_hits", "cull_mask", "flags"])


def test_presence():
    """art_closest_points_multi(NULL, NULL) is ART_E_INVALID with the prefixed message on any machine; the library exports it, the Rust binding declares the function
    and the struct, the header cites DESIGN.md 3.10, and Renderer has both methods"""
    from araytracingjourney_amd import _lib, renderer
    L = _lib.load()
    assert L.art_closest_points_multi(None, None) == _lib.ART_E_INVALID and L.art_last_error().startswith(WHO)
    assert L.art_closest_points_multi(None, C.byref(_lib.ArtPointQueryMulti(n=0, max_hits=1))) == _lib.ART_E_INVALID
    so = os.path.join(ROOT, "araytracingjourney_amd", "libart.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "art_closest_points_multi" for line in syms.splitlines() if line.strip())
    rs = open(os.path.join(ROOT, "bindings", "art_sys.rs")).read()
    assert "pub fn art_closest_points_multi(" in rs and "pub struct ArtPointQueryMulti" in rs
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    assert "DESIGN.md 3.10" in hdr and "### 3.10" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert callable(renderer.Renderer.closest_points_multi) and callable(renderer.Renderer.closest_surface_multi)


def test_the_entry_point_refuses_null_arguments_and_flags_on_any_machine():
    """tests/test_query_arguments.py's check for the new entry point: a NULL context or descriptor is refused first, and nonzero flags before the context is looked at --
    the context handed over is 64 KB of zeros that the entry point does not get to read.  The texts are literals"""
    from araytracingjourney_amd import _lib
    L = _lib.load()
    d = _lib.ArtPointQueryMulti(flags=1, max_hits=1)
    nowhere = C.create_string_buffer(1 << 16)
    for ctx, dd in ((None, C.byref(d)), (nowhere, None), (None, None)):
        assert L.art_closest_points_multi(ctx, dd) == _lib.ART_E_INVALID and L.art_last_error() == b"art_closest_points_multi: null argument"
    for flags in (1, 0x80000000):
        d.flags = flags
        assert L.art_closest_points_multi(nowhere, C.byref(d)) == _lib.ART_E_INVALID and L.art_last_error() == b"art_closest_points_multi: flags: must be 0"


@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_at_one_answer_the_reference_is_closest_points_own(get_scene, name, detail):
    """K = 1: the records are np_closest.brute_force's, bit for bit (ids, d, u, v, the point), and the count says whether there is an answer -- over r = inf and over
    radii that leave a part of the queries empty"""
    ref = _scene_ref(get_scene, name, detail)
    one = tcp._ref(get_scene, name, detail)["want"]
    got = _want(ref, 1)
    assert np.array_equal(got[1][:, 0], one[1]) and np.array_equal(_bits(got[0][:, 0]), _bits(one[0])) and np.array_equal(_bits(got[2][:, 0]), _bits(one[2]))
    assert np.array_equal(got[3], (one[1][:, 0] >= 0).astype(np.uint8)) and got[3].all()
    q = np.array(ref["q"][:512])
    q[:, 3] = np.tile(np.array([0.05, 0.2, 0.5, 0.0], np.float32), 128)
    one, got = nc.brute_force(ref["T"], q), ncm.brute_force(ref["T"], q, 1)
    assert np.array_equal(got[1][:, 0], one[1]) and np.array_equal(_bits(got[0][:, 0]), _bits(one[0])) and np.array_equal(_bits(got[2][:, 0]), _bits(one[2]))
    assert np.array_equal(got[3], (one[1][:, 0] >= 0).astype(np.uint8)) and 0 < int(got[3].sum()) < 512


# the reference's own counts of queries whose K-th and (K+1)-th candidates share their d2_eff, at K = 2, 4, 8 (the issue's table; at least half of each is asserted)
CONTESTED = {"sponza_like": (4096, 7144, (761, 911, 1471)), "lattice": (2197, 576, (977, 1403, 1679)), "clump": (512, 1000, (93, 142, 160))}


@pytest.mark.parametrize("name", list(CONTESTED) + ["chain"])
def test_the_comparisons_are_not_vacuous(get_scene, name):
    """from the reference alone, at r = inf: every query of the shared sets has K answers at K = 2, 4 and 8, and in hundreds of them the rank behind the K-th ties with
    it on d2_eff -- the order by global id at the eviction boundary is what decides their last record.  On the chain every query but one is contested at every K"""
    ref = _named_ref(get_scene, name)
    tab, n = ref["tab"], ref["q"].shape[0]
    figures = {K: int(ncm.contested(tab, K).sum()) for K in range(1, 9)}
    print(f"\n[closest multi] {name}: {n} queries, {ref['T']['v0'].shape[0]} triangles; contested at K = 1..8: {list(figures.values())}")
    for K in (2, 4, 8):
        want = _want(ref, K)
        assert (want[3] == K).all() and (want[1][..., 0] >= 0).all(), f"{name}: a query with fewer than {K} answers at r = inf"
        d = want[0][..., 0]
        assert (d[:, 1:] >= d[:, :-1]).all()
    if name == "chain":
        assert n == 202 and all(f >= n - 1 for f in figures.values()), figures
    else:
        nq, nt, floors = CONTESTED[name]
        assert n == nq and ref["T"]["v0"].shape[0] == nt
        for K, floor in zip((2, 4, 8), floors):
            assert figures[K] >= (floor + 1) // 2, (K, figures[K], floor)


# ---- on the device ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,detail", tcp.SCENES)
def test_both_scenes_are_the_references(R, torch, get_scene, name, detail):
    """1: 4096 queries with r = inf on a side stream at K = 1, 3, 4, 5, 8: ids, bits and counts; K = 1 is closest_points of the same tensor bit for bit; a permutation of
    the queries gives the permuted records; oversized out= tensors filled with a pattern are untouched beyond n; the queries count neither as casts nor as rays"""
    ref = _scene_ref(get_scene, name, detail)
    q = ref["q"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    perm = np.random.default_rng(3).permutation(N)
    d_q, d_p = _up(torch, q), _up(torch, q[perm])
    outs = {K: _patterned(torch, N + 70, K) for K in KS}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = {K: (r.closest_points_multi(d_q, K), r.closest_points_multi(d_p, K), r.closest_points_multi(d_q, K, out=outs[K])) for K in KS}
        single = r.closest_points(d_q)
    s.synchronize()
    for K in KS:
        want = _want(ref, K)
        plain, permuted, given = got[K]
        assert plain[0].shape == (N, K, 4) and plain[1].shape == (N, K, 2) and plain[1].dtype == torch.int32 and plain[2].shape == (N, K, 4) and plain[3].shape == (N,)
        assert plain[3].dtype == torch.uint8 and all(a is b for a, b in zip(given, outs[K]))
        _same(_host(plain), want, f"{name}, K = {K}")
        _same(_host(permuted), tuple(w[perm] for w in want), f"{name}, K = {K}, permuted")
        _same(tuple(t[:N].cpu().numpy() for t in outs[K]), want, f"{name}, K = {K}, out=")
        _untouched(torch, outs[K], N, f"{name}, K = {K}")
    one, (duv, ids, point) = _host(got[1][0]), _host(single)
    assert np.array_equal(_bits(one[0][:, 0]), _bits(duv)) and np.array_equal(one[1][:, 0], ids) and np.array_equal(_bits(one[2][:, 0]), _bits(point)), "K = 1 is not closest_points"
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    r.close()


@pytest.mark.gpu
def test_radii_and_dead_queries(R, torch, get_scene):
    """2: 1024 Cornell queries at K = 8, each once per radius: inf, 0, -0.0, the exact float distance of its j-th nearest triangle (j = i mod 8 + 1), the largest float
    whose square is below that d2_eff, -1, NaN, -inf; then 64 points with NaN / +-inf coordinates.  Counted in the reference first: every count 0..8 occurs, and "below"
    leaves fewer than j answers wherever there is such a radius.  Miss records carry r as given, bit for bit, and their points are zeros"""
    ref = _scene_ref(get_scene, "cornell", 1.0)
    q0, K = ref["q"][:1024], 8
    j = np.arange(1024) % 8 + 1
    d2 = ref["tab"]["d2"][np.arange(1024), j - 1]
    assert np.isfinite(d2).all()
    exact = np.sqrt(d2).astype(np.float32)
    below = tcp._below(d2)
    has_below = ~np.isnan(below)
    below = np.where(has_below, below, np.float32(-1.0)).astype(np.float32)
    radii = [np.full(1024, np.inf, np.float32), np.zeros(1024, np.float32), np.full(1024, -0.0, np.float32), exact, below, np.full(1024, -1.0, np.float32),
             np.full(1024, np.nan, np.float32), np.full(1024, -np.inf, np.float32)]
    k = len(radii)
    q = np.repeat(q0, k, axis=0)
    q[:, 3] = np.stack(radii, 1).reshape(-1)
    dead = np.array(q0[:64])
    for i in range(64):
        dead[i, i % 3] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
    q = np.concatenate([q, dead])
    want = ncm.brute_force(ref["T"], q, K)
    count = want[3][:1024 * k].reshape(1024, k).astype(np.int64)
    assert (count[:, 0] == 8).all() and not count[:, 5:].any() and not want[3][1024 * k:].any()
    assert set(np.unique(want[3]).tolist()) == set(range(9)), "a count that never occurs"
    assert int(has_below.sum()) >= 512 and (count[has_below, 4] < j[has_below]).all() and int((count[:, 3] >= j).sum()) >= 512   # the exact distance reaches rank j more often than not; below it never
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    got = _ask(r, torch, q, K)
    _same(got, want, "radii")
    miss = got[1][..., 0] < 0
    assert np.array_equal(miss, np.arange(K)[None, :] >= got[3][:, None])
    assert np.array_equal(_bits(got[0][..., 0])[miss], _bits(np.repeat(q[:, 3:4], K, axis=1))[miss]) and not got[2][miss].any() and not got[0][miss][:, 1:].any()
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", tcp.HOSTILE)
def test_hostile_inputs(R, torch, which):
    """3: tests/test_closest_points.py's hazards at K = 8 (and K = 3 on the lattice and the chain): the lattice, whose many-way ties at d = 0 decide who is evicted; the
    chain of 64 nested slivers, whose stacks go past their LDS part while the list is full; the degenerate soups; triangles that are segments and points; the
    one-triangle scene, where the count is 1 and seven miss records follow"""
    sc, q = tcp._hostile(which)
    T = nc.world_triangles(sc.primitives)
    tab = ncm.table(T, q)
    if which == "lattice":
        # measured in the reference: 261 queries have more than 3 candidates at d = 0 and 35 more than 8 (eviction among equals at distance 0); 1679 / 1959 are contested
        assert int((tab["d2"][:, 3] == 0).sum()) >= 200 and int((tab["d2"][:, 8] == 0).sum()) >= 30 and int(ncm.contested(tab, 8).sum()) >= 800 and int(ncm.contested(tab, 3).sum()) >= 800
    if which == "chain":
        assert int(ncm.contested(tab, 8).sum()) >= 200 and (tab["cand"] == 64).all()
    r = R.renderer_for_scene(sc, (64, 64))
    for K in (8, 3) if which in ("lattice", "chain") else (8,):
        want = ncm.records(T, q, tab, K)
        if which == "one triangle":
            assert want[3].max() == 1 and 0 < int((want[3] == 0).sum()) < q.shape[0] and (want[1][:, 1:] == -1).all()
        _same(_ask(r, torch, q, K), want, f"{which}, K = {K}")
    r.close()


def _form_ref(get_scene, name):
    """tests/test_query_forms.py's inputs of a case (its queries; the rays are not used)"""
    return _ref(("forms", name), lambda: tqf._inputs(get_scene, name)[0::2])


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(tqf.FORMS))
@pytest.mark.parametrize("name", ["chain", "clump", "cornell"])
def test_every_tree_form_gives_the_reference(R, torch, get_scene, name, form):
    """4: the records are defined as independent of the structure: the chain, the clump and Cornell's 4097 queries of tests/test_query_forms.py on each of its tree
    forms at K = 4 and 8 (that module proves that the chain's and the clump's first descents hold more pending entries than a lane keeps in LDS on every form)"""
    ref = _form_ref(get_scene, name)
    r = R.renderer_for_scene(ref["scene"], (64, 64), **tqf.FORMS[form])
    d_q = _up(torch, ref["q"])
    got = {K: r.closest_points_multi(d_q, K) for K in (4, 8)}
    torch.cuda.synchronize()
    for K in (4, 8):
        _same(_host(got[K]), _want(ref, K), f"{name}, {form}, K = {K}")
    r.close()


KNOBS = [{"trace_chunk": 64}, {"trace_chunk": 65536}, {"trace_refill": 1}, {"trace_refill": 64}, {"trace_leaf_batch": 1}, {"trace_leaf_batch": 64}]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join(f"{a}-{b}" for a, b in k.items()))
def test_knobs_change_the_schedule_never_the_records(R, torch, get_scene, knobs):
    """4: sponza_like at 0.05 under ArtTuning.trace_chunk 64 / 65536, trace_refill 1 / 64 and trace_leaf_batch 1 / 64, K = 4 and 8.  (The loop is k_closest's: why
    trace_leaf_batch = 64 and trace_refill = 64 cannot hang it is argued in tests/test_query_forms.py; a list changes neither the step block nor the refill.)"""
    ref = _scene_ref(get_scene, "sponza_like", 0.05)
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning=knobs)
    d_q = _up(torch, ref["q"])
    got = {K: r.closest_points_multi(d_q, K) for K in (4, 8)}
    torch.cuda.synchronize()
    for K in (4, 8):
        _same(_host(got[K]), _want(ref, K), f"{knobs}, K = {K}")
    r.close()


@pytest.mark.gpu
def test_sizes_at_which_a_refill_can_go_wrong(R, torch, get_scene):
    """4: ArtTuning.trace_chunk = 64 (a chunk is one filling of a wave) at K = 8: no query, one, a wave less one, a wave, a wave and one, 4097 -- prefixes of Cornell's
    4097 queries -- then a batch that misses everything (r = 0 away from any surface) and a batch that is all dead.  Every batch is written into tensors five records
    too long filled with a pattern: the tail keeps it.  n = 0 enqueues nothing"""
    ref, K = _form_ref(get_scene, "cornell"), 8
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning={"trace_chunk": 64})
    batches = [(ref["q"][:n], _want(ref, K, n), f"n = {n}") for n in (0, 1, 63, 64, 65, 4097)]
    away = np.array(ref["q"][:130])
    away[:, 3] = 0.0
    for q, what in ((away, "all miss"), (tqf._dead_queries(ref["q"][:130]), "all dead")):
        want = ncm.brute_force(ref["T"], q, K)
        assert not want[3].any() and (want[1] == -1).all(), what
        batches.append((q, want, what))
    s = torch.cuda.Stream()
    for q, want, what in batches:
        n = q.shape[0]
        d_q, out = _up(torch, np.asarray(q).reshape(n, 4)), _patterned(torch, n + 5, K)
        before = r.cast_counts()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = r.closest_points_multi(d_q, K, out=out)
        s.synchronize()
        assert got[0] is out[0]
        if n == 0:
            assert r.cast_counts() == before, "n = 0 enqueued something"
        _same(tuple(t[:n].cpu().numpy() for t in out), want, what)
        _untouched(torch, out, n, what)
        if what in ("all miss", "all dead"):
            assert np.array_equal(_bits(out[0][:n].cpu().numpy()[..., 0]), _bits(np.repeat(np.asarray(q)[:, 3:4], K, axis=1))), f"{what}: r as given"
    assert r.cast_counts()["casts"] == 0
    r.close()


@pytest.mark.gpu
def test_masks_and_alpha(R, torch, scenes, get_scene):
    """5: primitive masks set after the build against cull masks 0xFF, 1, 2, 0x80 and 0 (which sees nothing): a masked primitive drops out of every list and the next
    candidate moves up -- the reference's `vis`; an alpha cutoff on a fully transparent card changes no record"""
    sc = tcp._card_scene(scenes, get_scene)
    clear, solid = len(sc.primitives) - 2, len(sc.primitives) - 1
    q = tcp.queries(random_rays(2048, 5, radius=0.9)[:, 0:3])
    q[1::4, 3] = 0.25
    T, K = nc.world_triangles(sc.primitives), 4
    plain = ncm.brute_force(T, q, K)
    assert int((plain[1][..., 0] == clear).any(axis=1).sum()) > 50 and int((plain[1][..., 0] == solid).any(axis=1).sum()) > 50 and 0 < int((plain[3] < K).sum()) < 2048
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    _same(_ask(r, torch, q, K), plain, "unmasked")
    m.set_alpha_cutoff(clear, 0.5); m.set_alpha_cutoff(solid, 0.5)
    _same(_ask(r, torch, q, K), plain, "with cutoffs: not tested")
    masks = {0: 0x01, 1: 0x02, solid: 0x03, clear: 0x02}
    for i, v in masks.items():
        m.set_mask(i, v)
    vis = np.array([masks.get(p, 0xFF) for p in range(len(sc.primitives))])
    seen = []
    for cull in (0xFF, 0x01, 0x02, 0x80, 0):
        want = ncm.brute_force(T, q, K, vis=vis, cull=cull)
        got = _ask(r, torch, q, K, cull_mask=cull)
        _same(got, want, f"cull {cull:#x}")
        hidden = [p for p in range(len(sc.primitives)) if not (vis[p] & cull)]
        assert not np.isin(got[1][..., 0], hidden).any()
        if cull == 0:
            assert (got[1] == -1).all() and not got[3].any() and np.array_equal(_bits(got[0][..., 0]), _bits(np.repeat(q[:, 3:4], K, axis=1))) and not got[2].any()
        seen.append(got[1][..., 0].copy())
    assert not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[1])
    moved_up = (seen[0][:, 0] != seen[1][:, 0]) & (seen[1][:, 0] >= 0)   # the nearest was masked away and another triangle took the first record
    assert int(moved_up.sum()) > 50
    r.close()


@pytest.mark.gpu
def test_a_primitive_disabled_after_the_build_is_nowhere(R, torch, scenes, get_scene):
    """5: two primitives of two triangles each, one disabled after the build: it appears in no list even at r = inf with K = 8 -- the other's two triangles and six miss
    records; enabled again, the first answers return"""
    sc = tcp._card_scene(scenes, get_scene)
    two = scenes.Scene("two", list(sc.primitives[-2:]), sc.camera, sc.lights)
    q = tcp.queries(random_rays(1024, 9, radius=0.8)[:, 0:3])
    r = R.Renderer((64, 64), tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(two.primitives)
    r.prepare_first_frame()
    K = 8
    nt = nc.world_triangles(two.primitives)["v0"].shape[0]
    both = ncm.brute_force(nc.world_triangles(two.primitives), q, K)
    assert nt >= 4 and (both[3] == min(K, nt)).all() and {0, 1} <= set(np.unique(both[1][..., 0]).tolist())
    _same(_ask(r, torch, q, K), both, "both")
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 0) == 0 and not r.needs_build()
    want = ncm.brute_force(nc.world_triangles(two.primitives, disabled=(1,)), q, K)
    assert not (want[1][..., 0] == 1).any() and (want[3] == min(K, nt // 2)).all()
    got = _ask(r, torch, q, K)
    _same(got, want, "one disabled")
    assert not (got[1][..., 0] == 1).any()
    assert r._L.art_scene_set_primitive_enabled(r._ctx, 1, 1) == 0
    _same(_ask(r, torch, q, K), both, "enabled again")
    assert r.stats()["rebuilds"] == 0
    r.close()


@pytest.mark.gpu
def test_the_scene_as_of_the_call(R, torch, get_scene):
    """6: Cornell's last primitive as a model of its own on a dynamic scene that never rebuilds: after art_scene_set_model_matrix and after art_scene_set_vertices a batch
    at K = 8 and one at K = 3 on one side stream, no synchronisation in between: each is the reference over the triangles as of its call"""
    sc = get_scene("cornell")
    q = _scene_ref(get_scene, "cornell", 1.0)["q"][:2048]
    r = R.Renderer((64, 64), dynamic_scene=True, tuning={"refit_rebuild_ratio": -1.0})
    r.add_model(list(sc.primitives[:-1]))
    r.add_model([sc.primitives[-1]])
    r.prepare_first_frame()
    static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
    P = type(moving)
    m = np.ascontiguousarray(np.asarray(moving.model, np.float32).reshape(3, 4).copy())
    m[:, 3] += np.array([0.06, 0.03, -0.06], np.float32)
    verts = np.array(moving.verts, np.float32)
    verts[:, 0:3] = verts[:, 0:3] * np.float32(0.75) + np.array([0.0, 0.05, 0.0], np.float32)
    states = [("built", list(sc.primitives)), ("moved", static + [P(moving.verts, moving.indices, moving.tex, m)]), ("deformed", static + [P(verts, moving.indices, moving.tex, m)])]
    model = r.models_mut()[1]
    d_q = _up(torch, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    for what, _ in states:
        if what == "moved": model.set_model_matrix(m)
        elif what == "deformed": model.set_vertices(0, verts)
        assert not r.needs_build()
        with torch.cuda.stream(s):
            outs.append({K: r.closest_points_multi(d_q, K) for K in (8, 3)})
    s.synchronize()
    wants = [{K: ncm.records(T, q, ncm.table(T, q), K) for K in (8, 3)} for T in (nc.world_triangles(prims) for _, prims in states)]
    for (what, _), got, want in zip(states, outs, wants):
        for K in (8, 3):
            _same(_host(got[K]), want[K], f"{what}, K = {K}")
    assert not np.array_equal(_bits(wants[0][8][0]), _bits(wants[1][8][0])) and not np.array_equal(_bits(wants[1][8][0]), _bits(wants[2][8][0]))
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 2 and r.cast_counts()["casts"] == 0
    r.close()


@pytest.mark.gpu
def test_the_ring_on_three_streams(R, torch, get_scene):
    """7: 40 calls (K = 8, 4, 1 in turn) over three torch streams, a closest_points and a cast_rays between every four of them, nothing synchronised before the end: the
    ring of ART_CAST_POOL cursor blocks is lapped.  Every result is its reference; casts and rays count the ray casts alone"""
    from araytracingjourney_amd import _lib
    assert 40 > _lib.ART_CAST_POOL
    ref, n = _scene_ref(get_scene, "sponza_like", 0.05), 1024
    single = tcp._ref(get_scene, "sponza_like", 0.05)["want"]
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_q, d_rays = _up(torch, ref["q"][:n]), _up(torch, random_rays(64, 7))
    streams = [torch.cuda.Stream() for _ in range(3)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs, n_casts = [], 0
    for i in range(40):
        with torch.cuda.stream(streams[i % 3]):
            K = (8, 4, 1)[(i // 3) % 3]
            outs.append((K, r.closest_points_multi(d_q, K)))
            if i % 4 == 3:
                outs.append((0, r.closest_points(d_q)))
                r.cast_rays(d_rays)
                n_casts += 1
    counts = r.cast_counts()
    for s in streams:
        s.synchronize()
    assert {K for K, _ in outs} == {0, 1, 4, 8}
    for i, (K, got) in enumerate(outs):
        if K:
            _same(_host(got), _want(ref, K, n), f"operation {i}, K = {K}")
        else:
            tcp._same(_host(got), tuple(w[:n] for w in single), f"operation {i}, closest_points")
    assert counts["casts"] == n_casts == 10 and counts["rays"] == 64 * n_casts and counts["host_waits"] <= 60 - _lib.ART_CAST_POOL, counts
    r.close()


@pytest.mark.gpu
def test_closest_surface_multi(R, torch, get_scene):
    """8: closest_points_multi and one resolve of the flattened records on one side stream: the records are the reference's, the resolve equals resolve_hits on the same
    records word for word (as (n, K, w) and flattened to (n * K, w)), a resolved record has w = 1 and miss records resolve to zeros"""
    ref, K = _scene_ref(get_scene, "cornell", 1.0), 5
    bound = json.load(open(tcp.STATS))["cornell"]["allowed_abs_error"]   # tests/test_closest_points.py's bound on |resolve's pos - point_dev|
    q = np.array(ref["q"][:2048])
    q[::3, 3] = 0.15
    want = ncm.brute_force(ref["T"], q, K)
    miss = want[1][..., 0] < 0
    assert 500 < int(miss.sum()) < 2048 * K - 500 and 0 < int((want[3][::3] == 0).sum()) and int(((want[3] > 0) & (want[3] < K)).sum()) > 50
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        (duv, ids, point, count), surf = r.closest_surface_multi(_up(torch, q), K, want=("pos", "ng", "uv"))
        again = r.resolve_hits(duv, ids, want=("pos", "ng", "uv"))
        flat = r.resolve_hits(duv.view(-1, 4), ids.view(-1, 2), want=("pos", "ng", "uv"))
    s.synchronize()
    _same(_host((duv, ids, point, count)), want, "closest_surface_multi")
    for o in ("pos", "ng", "uv"):
        a = surf[o].cpu().numpy()
        assert a.shape[:2] == (2048, K)
        assert np.array_equal(_bits(a), _bits(again[o].cpu().numpy())) and np.array_equal(_bits(a).reshape(2048 * K, -1), _bits(flat[o].cpu().numpy())), o
        assert not a[miss].any(), f"{o}: a miss record resolves to something"
    pos = surf["pos"].cpu().numpy()
    assert (pos[~miss][:, 3] == 1).all() and np.abs(pos[~miss][:, :3].astype(np.float64) - want[2][~miss][:, :3]).max() <= bound
    r.close()


@pytest.mark.gpu
def test_errors_change_nothing_and_enqueue_nothing(R, torch, get_scene):
    """9: every ART_E_INVALID case of include/art.h, and ART_E_STATE before the build and while the scene needs one: the code, a message that names the entry point,
    pattern-filled outputs untouched and the counts unchanged; the wrapper raises ValueError before the call"""
    from araytracingjourney_amd import _lib
    sc = get_scene("cornell")
    r = R.Renderer((64, 64))
    r.add_model(sc.primitives)
    L, ctx = r._L, r._ctx
    n, K = 64, 3
    pts = _up(torch, tcp.queries(random_rays(n + 1, 7)[:, 0:3]))
    duv, ids, point, count = _patterned(torch, n + 1, K)
    torch.cuda.synchronize()

    def desc(**kw):
        d = dict(points_dev=pts.data_ptr(), duv_dev=duv.data_ptr(), ids_dev=ids.data_ptr(), point_dev=point.data_ptr(), count_dev=count.data_ptr(), hip_stream=None, n=n,
                 max_hits=K, cull_mask=0xFF, flags=0)
        d.update(kw)
        return _lib.ArtPointQueryMulti(**d)

    def code(d):
        return L.art_closest_points_multi(ctx, C.byref(d) if d is not None else None)

    named = lambda: L.art_last_error().startswith(WHO)   # noqa: E731
    clean = lambda: all((t.view(torch.int32) == PATTERN).all() for t in (duv, ids, point)) and (count == 0xA5).all()   # noqa: E731
    assert code(desc()) == _lib.ART_E_STATE and named() and b"not built" in L.art_last_error()
    r.prepare_first_frame()
    zero = dict(casts=0, rays=0, host_waits=0)
    assert L.art_closest_points_multi(None, C.byref(desc())) == _lib.ART_E_INVALID and named()
    assert code(None) == _lib.ART_E_INVALID and named()
    bad = [desc(points_dev=None), desc(duv_dev=None), desc(ids_dev=None), desc(points_dev=pts.data_ptr() + 4), desc(points_dev=pts.data_ptr() + 8), desc(duv_dev=duv.data_ptr() + 8),
           desc(ids_dev=ids.data_ptr() + 4), desc(point_dev=point.data_ptr() + 8), desc(max_hits=0), desc(max_hits=_lib.ART_CAST_MAX_HITS + 1), desc(max_hits=0xFFFFFFFF),
           desc(cull_mask=0x100), desc(cull_mask=0xFFFFFFFF), desc(flags=1), desc(flags=0x80000000), desc(n=_lib.ART_CAST_MAX_RAYS + 1), desc(n=0xFFFFFFFF)]
    for d in bad:
        assert code(d) == _lib.ART_E_INVALID and named(), (d.n, d.max_hits, d.cull_mask, d.flags)
    r.cast_sync()
    torch.cuda.synchronize()
    assert r.cast_counts() == zero and clean()
    assert code(desc(n=0)) == 0 and code(desc(n=0, points_dev=None, duv_dev=None, ids_dev=None, point_dev=None, count_dev=None)) == 0   # n = 0 is legal and enqueues nothing
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    # the wrapper's own checks: before anything is enqueued
    for args, kw in (((pts.cpu(), K), {}), ((pts.double(), K), {}), ((pts[:, :3], K), {}), ((pts, 0), {}), ((pts, _lib.ART_CAST_MAX_HITS + 1), {}), ((pts, 2.5), {}),
                     ((pts, K), dict(cull_mask=0x100)), ((pts, K), dict(out=(duv[:8], ids, point, count))), ((pts, K), dict(out=(duv, ids.to(torch.int64), point, count))),
                     ((pts, K + 1), dict(out=(duv, ids, point, count))), ((pts, K), dict(out=(duv, ids, point[..., :3], count)))):
        with pytest.raises((ValueError, TypeError)):
            r.closest_points_multi(*args, **kw)
    r.cast_sync()
    assert r.cast_counts() == zero and clean()
    assert code(desc(point_dev=None, count_dev=None)) == 0   # the optional outputs left out: neither is written
    r.cast_sync()
    assert (ids[:n, 0, 0] >= 0).all() and (ids[n:] == PATTERN).all() and (point.view(torch.int32) == PATTERN).all() and (count == 0xA5).all() and r.cast_counts() == zero
    assert code(desc()) == 0
    r.cast_sync()
    assert (count[:n] == K).all() and (count[n:] == 0xA5).all() and (point[:n, :, 3] == 1).all() and (point[n:].view(torch.int32) == PATTERN).all() and r.cast_counts() == zero
    r.add_model([sc.primitives[0]])   # a primitive added since the build: art_scene_needs_build
    assert r.needs_build() and code(desc()) == _lib.ART_E_STATE and named()
    with pytest.raises(_lib.ArtError):
        r.closest_points_multi(pts, K)
    r.close()
