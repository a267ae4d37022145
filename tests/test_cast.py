"""art_cast_rays (include/art.h): rays in a device buffer -- torch tensors here -- traced asynchronously on a stream.  The reference is the CPU oracle
(orc.Scene.trace_closest / trace_any over a 30-bit-Morton tree of its own): ids and the bits of t, u, v are equal, any-hit bytes are equal.  Scenes and rays are those
of the query tests (tests/test_gpu_parity.py, tests/test_alpha.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import random_rays
from helpers import _dead_rays, _layout_is_the_headers, _outward_rays, R, _tex_of_alpha as _tex, torch, _up  # noqa: F401  (R, torch: module fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = -0x5A5A5A5B   # what oversized output buffers are filled with (int32; as a float a NaN with a payload no tracer writes)


_REF = {}


def _ref(orc, get_scene, name, detail, n):
    """the oracle's records for random_rays(n, 7) on a scene: computed once, shared, never written"""
    key = (name, detail, n)
    if key not in _REF:
        sc = get_scene(name, detail)
        S = orc.Scene(sc.primitives, morton_bits=30)   # another tree than the device's 63-bit one: results must not depend on it
        rays = random_rays(n, 7)
        tuv, ids = S.trace_closest(rays)[:2]
        short = rays.copy()
        short[:, 7] = 1.5
        hit = S.trace_any(short)[0]
        for a in (rays, short, tuv, ids, hit):
            a.setflags(write=False)
        _REF[key] = dict(scene=sc, S=S, rays=rays, short=short, tuv=tuv, ids=ids, hit=hit)
    return _REF[key]


def _same_closest(got, want, what=""):
    (tuv, ids), (rtuv, rids) = got, want
    tuv, ids = tuv.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(ids, rids), f"{what}: {int((ids != rids).any(-1).sum())} id pairs differ"
    assert np.array_equal(tuv.view(np.uint32)[:, :3], np.ascontiguousarray(rtuv).view(np.uint32)[:, :3]), f"{what}: t, u, v differ"
    assert not tuv.view(np.uint32)[:, 3].any(), f"{what}: the fourth word is not 0"


def _same_any(got, want, what=""):
    assert np.array_equal(got.cpu().numpy(), want), what


@pytest.mark.gpu
@pytest.mark.parametrize("name,detail,n", [("sponza_like", 0.12, 20000), ("cornell", 1.0, 4096)])
def test_casts_match_the_oracle_bitwise(R, torch, orc, get_scene, name, detail, n):
    """closest and any-hit casts of rays torch uploaded, on a torch side stream: the oracle's ids, the bits of its t, u, v, its any-hit bytes; a random permutation of the
    rays gives the permuted records"""
    ref = _ref(orc, get_scene, name, detail, n)
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    rays, short = _up(torch, ref["rays"]), _up(torch, ref["short"])
    perm = np.random.default_rng(3).permutation(n)
    rays_p, short_p = _up(torch, ref["rays"][perm]), _up(torch, ref["short"][perm])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())   # (the uploads ran on torch's default stream)
    with torch.cuda.stream(s):
        closest, hit = r.cast_rays(rays), r.cast_rays(short, kind="any")
        closest_p, hit_p = r.cast_rays(rays_p), r.cast_rays(short_p, kind="any")
    s.synchronize()
    _same_closest(closest, (ref["tuv"], ref["ids"]), name)
    _same_any(hit, ref["hit"], name)
    _same_closest(closest_p, (ref["tuv"][perm], ref["ids"][perm]), name + ", permuted")
    _same_any(hit_p, ref["hit"][perm], name + ", permuted")
    hits = int((ref["ids"][:, 0] >= 0).sum())
    assert hits >= 1000 and n - hits >= 500 and 0 < int(ref["hit"].sum()) < n
    if name == "sponza_like":
        assert set(ref["ids"][:, 0].tolist()) == set(range(len(ref["scene"].primitives))) | {-1}   # every primitive is somebody's closest hit
    assert r.cast_counts() == dict(casts=4, rays=4 * n, host_waits=0)
    r.close()


@pytest.mark.gpu
def test_sizes_at_which_the_kernel_can_go_wrong(R, torch, orc, get_scene):
    """ArtTuning.trace_chunk = 64 (a chunk is one pool filling): no rays, one, a wave less one, a wave, a wave and one, chunks and a ray more or less, several workgroups; a
    batch that misses everything and a batch of dead rays; the records behind the n-th of an oversized output buffer keep what they held"""
    ref = _ref(orc, get_scene, "sponza_like", 0.12, 20000)
    r = R.renderer_for_scene(ref["scene"], (64, 64), tuning={"trace_chunk": 64})
    s = torch.cuda.Stream()
    batches = [(ref["rays"][:n], ref["short"][:n], ref["tuv"][:n], ref["ids"][:n], ref["hit"][:n], f"n = {n}") for n in (0, 1, 63, 64, 65, 127, 511, 513, 4097)]
    for rays, what in ((_outward_rays(ref["rays"][:195]), "all miss"), (_dead_rays(ref["rays"][:130]), "all dead")):
        tuv, ids = ref["S"].trace_closest(rays)[:2]
        hit = ref["S"].trace_any(rays)[0]
        assert (ids == -1).all() and not hit.any(), what
        batches.append((rays, rays, tuv, ids, hit, what))
    pad = 5
    for rays, short, tuv, ids, hit, what in batches:
        n = rays.shape[0]
        d_rays, d_short = _up(torch, rays.reshape(n, 8)), _up(torch, short.reshape(n, 8))
        o_tuv = torch.full((n + pad, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
        o_ids = torch.full((n + pad, 2), PATTERN, dtype=torch.int32, device="cuda")
        o_hit = torch.full((n + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = r.cast_rays(d_rays, out=(o_tuv, o_ids))
            got_hit = r.cast_rays(d_short, kind="any", out=o_hit)
        s.synchronize()
        assert got[0] is o_tuv and got[1] is o_ids and got_hit is o_hit
        _same_closest((o_tuv[:n], o_ids[:n]), (tuv, ids), what)
        _same_any(o_hit[:n], hit, what)
        assert (o_tuv[n:].view(torch.int32) == PATTERN).all() and (o_ids[n:] == PATTERN).all() and (o_hit[n:] == 0xA5).all(), f"{what}: records behind the n-th were written"
    assert r.cast_counts()["casts"] == 2 * (len(batches) - 1)   # n = 0 enqueues nothing
    r.close()


_PARTLY_DEAD = {}


def _partly_dead(ref, n=193):
    """n of the reference's rays -- by the oracle's records one that hits, one that hits, one that misses, and so on -- with every third one, the first of each three, dead
    by _dead_rays' three rules in rotation, and the oracle's records for them: computed once, never written"""
    if not _PARTLY_DEAD:
        hits, misses = np.flatnonzero(ref["ids"][:, 0] >= 0), np.flatnonzero(ref["ids"][:, 0] < 0)
        pick = np.empty(n, np.int64)
        pick[0::3], pick[1::3], pick[2::3] = hits[:len(pick[0::3])], hits[n:n + len(pick[1::3])], misses[:len(pick[2::3])]
        out = {}
        for key in ("rays", "short"):
            rays = ref[key][pick]
            rays[0::3] = _dead_rays(rays[0::3])
            out[key] = rays
        out["tuv"], out["ids"] = ref["S"].trace_closest(out["rays"])[:2]
        out["hit"] = ref["S"].trace_any(out["short"])[0]
        for a in out.values():
            a.setflags(write=False)
        _PARTLY_DEAD.update(out)
    return _PARTLY_DEAD


def test_the_partly_dead_rays_are_a_mixed_lot(orc, get_scene):
    """without a GPU: of the 193 rays of the test below every third is dead -- a miss in the oracle's records -- and the live ones hold at least 50 hits and 50 misses"""
    pd = _partly_dead(_ref(orc, get_scene, "sponza_like", 0.12, 20000))
    dead = np.arange(193) % 3 == 0
    assert not np.isfinite(pd["rays"][dead]).all(axis=1).any() and np.isfinite(pd["rays"][~dead]).all()
    assert (pd["ids"][dead] == -1).all() and not pd["hit"][dead].any()
    hits = int((pd["ids"][~dead, 0] >= 0).sum())
    assert hits >= 50 and int((~dead).sum()) - hits >= 50 and 0 < int(pd["hit"][~dead].sum()) < int((~dead).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("refill", [1, 64])
def test_a_partly_dead_pool_filling_is_compacted(R, torch, orc, get_scene, refill):
    """193 rays, every third dead, ArtTuning.trace_chunk = 64: each pool filling holds 21 or 22 dead slots between live ones, so the live rays are compacted around records
    written at once; idle lanes take from the pool one at a time (trace_refill = 1) or only once the whole wave is idle (64).  Closest records and any-hit bytes are the
    oracle's, and the records behind the n-th keep what they held"""
    pd = _partly_dead(_ref(orc, get_scene, "sponza_like", 0.12, 20000))
    n, pad = pd["rays"].shape[0], 5
    r = R.renderer_for_scene(_ref(orc, get_scene, "sponza_like", 0.12, 20000)["scene"], (64, 64), tuning={"trace_chunk": 64, "trace_refill": refill})
    d_rays, d_short = _up(torch, pd["rays"]), _up(torch, pd["short"])
    o_tuv = torch.full((n + pad, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    o_ids = torch.full((n + pad, 2), PATTERN, dtype=torch.int32, device="cuda")
    o_hit = torch.full((n + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    r.cast_rays(d_rays, out=(o_tuv, o_ids))
    r.cast_rays(d_short, kind="any", out=o_hit)
    torch.cuda.synchronize()
    _same_closest((o_tuv[:n], o_ids[:n]), (pd["tuv"], pd["ids"]), f"refill {refill}")
    _same_any(o_hit[:n], pd["hit"], f"refill {refill}")
    assert (o_tuv[n:].view(torch.int32) == PATTERN).all() and (o_ids[n:] == PATTERN).all() and (o_hit[n:] == 0xA5).all(), "records behind the n-th were written"
    r.close()


# ---- the alpha card of tests/test_alpha.py (its construction, restated) ---------------------------------------------------------------------------------
def _card_scene(scenes, base, alpha):
    """Cornell and a horizontal card under its light"""
    mb = scenes.MeshBuilder()
    scenes.quad(mb, (-0.35, 0.3, -0.35), (0.7, 0.0, 0.0), (0.0, 0.0, 0.7), 2, 2, (1.0, 1.0))
    return scenes.Scene(base.name + "+card", list(base.primitives) + [mb.finish(_tex(alpha))], base.camera, base.lights)


def _card_alpha(tw=16, th=16):
    """a texel-scale checker of cut texels (alpha 0), the others a gradient along x: bilinear alpha crosses 0.5 inside many texels"""
    y, x = np.mgrid[0:th, 0:tw]
    return np.where((x + y) % 2 == 0, 0, np.round(255.0 * x / (tw - 1))).astype(np.uint8)


def _card_renderer(R, sc, cutoff=None, masks=None, disabled=()):
    r = R.renderer_for_scene(sc, (64, 64))
    m = r.models_mut()[0]
    if cutoff is not None:
        m.set_alpha_cutoff(len(sc.primitives) - 1, cutoff)
    for i, v in (masks or {}).items():
        m.set_mask(i, v)
    for i in disabled:
        assert r._L.art_scene_set_primitive_enabled(r._ctx, m.primitive_ids[i], 0) == 0
    return r


def _cast_both(r, torch, d_rays, cull=0xFF):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        (tuv, ids), hit = r.cast_rays(d_rays, cull_mask=cull), r.cast_rays(d_rays, kind="any", cull_mask=cull)
    s.synchronize()
    return tuv.cpu().numpy(), ids.cpu().numpy(), hit.cpu().numpy()


@pytest.mark.gpu
def test_casts_equal_the_pinned_features(R, torch, orc, get_scene, scenes):
    """Cornell and the alpha card with a cutoff and primitive masks set after the build (the cast takes them up: a refit in front of it), cull masks 0xFF, 1, 2 and 0:
    the cast is art_query_*_masked of a second context with the same scene.  The queries share the cast's path, so that leg is a self-check; the independent ones: a
    disabled card is the all-cut card, cull mask 0 is all-miss, and the unmasked opaque scene is the oracle's"""
    base = get_scene("cornell")
    sc = _card_scene(scenes, base, _card_alpha())
    card = len(sc.primitives) - 1
    rays = random_rays(2048, 5, radius=0.9)
    d_rays = _up(torch, rays)
    masks = {0: 0x01, 1: 0x02, card: 0x03}
    a, b = _card_renderer(R, sc, 0.5, masks), _card_renderer(R, sc, 0.5, masks)
    seen = []
    for cull in (0xFF, 0x01, 0x02, 0):
        tuv, ids, hit = _cast_both(a, torch, d_rays, cull)
        q_tuv, q_ids = b.query_closest(rays, cull_mask=cull)
        assert np.array_equal(ids, q_ids) and np.array_equal(tuv.view(np.uint32), q_tuv.view(np.uint32)) and np.array_equal(hit, b.query_any(rays, cull_mask=cull)), hex(cull)
        if cull == 0:   # sees nothing: the miss record of every ray
            assert (ids == -1).all() and not hit.any() and np.array_equal(tuv[:, 0], rays[:, 7]) and not tuv[:, 1:].any()
        else:
            prims = set(ids[:, 0].tolist()) - {-1}
            assert prims and all(masks.get(p, 0xFF) & cull for p in prims), hex(cull)
        seen.append(ids[:, 0].copy())
    assert (seen[0] == card).any() and (seen[1] != seen[2]).any()   # the card is hit where it is not cut, and the masks tell the rays apart
    a.close(); b.close()
    # a card cut everywhere is a card that is not there
    zero = _card_scene(scenes, base, np.zeros((8, 8), np.uint8))
    cut, off = _card_renderer(R, zero, 0.5), _card_renderer(R, zero, disabled=[card])
    for x, y in zip(_cast_both(cut, torch, d_rays), _cast_both(off, torch, d_rays)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    cut.close(); off.close()
    # the opaque, unmasked scene against the oracle
    S = orc.Scene(sc.primitives, morton_bits=30)
    op = _card_renderer(R, sc)
    tuv, ids, hit = _cast_both(op, torch, d_rays)
    rtuv, rids = S.trace_closest(rays)[:2]
    assert np.array_equal(ids, rids) and np.array_equal(tuv.view(np.uint32)[:, :3], rtuv.view(np.uint32)[:, :3]) and np.array_equal(hit, S.trace_any(rays)[0])
    assert (rids[:, 0] == card).sum() > 20
    op.close()


def _pose(base, i):
    """pose i of Cornell's last primitive: rotated about y and z, carried in small steps (the box stays inside the room) -- as the moving-model tests of tests/test_gpu_parity.py"""
    import math
    a, b = 0.21 * i, 0.13 * i
    ry = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]])
    rz = np.array([[math.cos(b), -math.sin(b), 0, 0], [math.sin(b), math.cos(b), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    m = ry @ rz @ np.vstack([np.asarray(base, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    m = np.ascontiguousarray(m[:3], np.float32)
    m[:, 3] = np.asarray(base, np.float32).reshape(3, 4)[:, 3] + np.float32(0.02 * i) * np.array([1.0, 0.5, -1.0], np.float32)
    return m


_MOVED = {}


def _moved_refs(orc, sc, rays, poses):
    """the oracle built from scratch at every pose of the last primitive"""
    if not _MOVED:
        static, moving = list(sc.primitives[:-1]), sc.primitives[-1]
        P = type(moving)
        for i, m in enumerate(poses):
            S = orc.Scene(static + [P(moving.verts, moving.indices, moving.tex, m)], morton_bits=30)
            _MOVED[i] = S.trace_closest(rays)[:2]
    return _MOVED


@pytest.mark.gpu
@pytest.mark.parametrize("versions", [2, 12])
def test_a_moving_scene_is_cast_without_fences(R, torch, orc, get_scene, versions):
    """Cornell with its last primitive moved to 8 poses, one cast per pose into 8 buffers on one stream and a single synchronisation at the end: every cast is the oracle's
    answer for a scene built from scratch at its pose -- it saw the scene as of its call and kept its version of the structure.  With 2 versions the ring is lapped (a refit
    waits for the cast that still reads what it would rewrite: host_waits may count it), with 12 nothing ever waits"""
    sc = get_scene("cornell")
    rays = random_rays(4096, 7)
    r = R.Renderer((64, 64), tuning={"as_versions": versions, "refit_rebuild_ratio": -1.0})
    r.add_model(list(sc.primitives[:-1]))
    r.add_model([sc.primitives[-1]])
    r.prepare_first_frame()
    model = r.models_mut()[1]
    poses = [_pose(sc.primitives[-1].model, i + 1) for i in range(8)]
    refs = _moved_refs(orc, sc, rays, poses)
    d_rays = _up(torch, rays)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(s):
        for m in poses:
            model.set_model_matrix(m)
            outs.append(r.cast_rays(d_rays))
    s.synchronize()
    for i, got in enumerate(outs):
        _same_closest(got, refs[i], f"pose {i}")
    assert any(not np.array_equal(refs[0][1], refs[i][1]) for i in range(1, 8))   # the poses differ where the rays look
    st, cc = r.stats(), r.cast_counts()
    assert st["refits"] == 8 and st["rebuilds"] == 0 and cc["casts"] == 8 and cc["rays"] == 8 * 4096
    if versions == 12:
        assert cc["host_waits"] == 0
    r.close()


def _frames_with_casts(R, torch, sc, d_rays, casts, w=96, h=96, frames=12):
    """12 frames through a ring of 4, the camera stepping, a cast behind every frame (casts) or none; no host synchronisation until all is enqueued.  Every frame's colour,
    depth and normal are copied out of its ring slot by a side stream that waits for the frame (art_stream_wait_frame); the frame that takes the slot next waits for the
    copies (art_wait_external_event: the copy stream is in order, so the latest copy's event covers the earlier ones)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    r = R.renderer_for_scene(sc, (w, h), frames_in_flight=4)
    copy_s, cast_s = torch.cuda.Stream(), torch.cuda.Stream()
    cast_s.wait_stream(torch.cuda.current_stream())
    pos = np.asarray(sc.camera["pos"], np.float64)
    kept, events, outs = [], [], []
    for f in range(frames):
        r.camera_mut().set_pos(tuple(pos + 0.01 * f * np.array([1.0, 0.5, -0.5])))
        r.upload_state(); r.trace()
        r.stream_wait_frame(copy_s.cuda_stream)
        bufs = []
        for ptr, nbytes in (r.device_color(), r._dev("depth"), r._dev("normal")):
            t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            assert hip.hipMemcpyAsync(t.data_ptr(), ptr, nbytes, 3, copy_s.cuda_stream) == 0   # hipMemcpyDeviceToDevice
            bufs.append(t)
        kept.append(bufs)
        ev = torch.cuda.Event()
        ev.record(copy_s)
        r.wait_external_event(ev.cuda_event)
        events.append(ev)
        if casts:
            with torch.cuda.stream(cast_s):
                outs.append(r.cast_rays(d_rays))
    counts = r.cast_counts()
    r.sync(); copy_s.synchronize(); cast_s.synchronize()
    frames_out = [[b.cpu().numpy() for b in bufs] for bufs in kept]
    r.close()
    return frames_out, outs, counts


@pytest.mark.gpu
def test_casts_beside_frames_change_neither(R, torch, orc, get_scene):
    """four frames in flight, 12 frames with a cast between every two and no synchronisation: every frame's colour, depth and normal are bit-equal to the same run without
    casts, every cast is the oracle's, and no cast ever waited on the host"""
    ref = _ref(orc, get_scene, "cornell", 1.0, 4096)
    d_rays = _up(torch, ref["rays"])
    plain, _, _ = _frames_with_casts(R, torch, ref["scene"], d_rays, casts=False)
    mixed, outs, counts = _frames_with_casts(R, torch, ref["scene"], d_rays, casts=True)
    for f, (a, b) in enumerate(zip(plain, mixed)):
        for what, x, y in zip(("colour", "depth", "normal"), a, b):
            assert np.array_equal(x, y), f"frame {f}: {what} differs beside casts"
    assert any(not np.array_equal(plain[0][1], plain[f][1]) for f in range(1, 12))   # the frames differ from each other (the camera moves)
    assert len(outs) == 12
    for got in outs:
        _same_closest(got, (ref["tuv"], ref["ids"]), "a cast beside frames")
    assert counts == dict(casts=12, rays=12 * 4096, host_waits=0)


@pytest.mark.gpu
def test_streams(R, torch, orc, get_scene):
    """40 casts back to back on one side stream into buffers of their own -- more than the pool of cursor blocks holds; a cast's output reduced by torch on the same stream
    with no host synchronisation in between; torch's default stream; hip_stream NULL with art_cast_sync as the fence"""
    from araytracingjourney_amd import _lib
    ref = _ref(orc, get_scene, "cornell", 1.0, 4096)
    n = 4096
    r = R.renderer_for_scene(ref["scene"], (64, 64))
    d_rays, d_short = _up(torch, ref["rays"]), _up(torch, ref["short"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    assert 40 > _lib.ART_CAST_POOL
    with torch.cuda.stream(s):
        outs = [r.cast_rays(d_rays) if i % 2 == 0 else r.cast_rays(d_short, kind="any") for i in range(40)]
        ids_sum = r.cast_rays(d_rays)[1].to(torch.int64).sum()         # behind the cast on s: torch orders it, nobody synchronises
        hit_sum = r.cast_rays(d_short, kind="any").to(torch.int64).sum()
        assert int(ids_sum.item()) == int(ref["ids"].astype(np.int64).sum()) and int(hit_sum.item()) == int(ref["hit"].sum())   # (.item() copies on the current stream: s)
    s.synchronize()
    for i, got in enumerate(outs):
        if i % 2 == 0:
            _same_closest(got, (ref["tuv"], ref["ids"]), f"cast {i}")
        else:
            _same_any(got, ref["hit"], f"cast {i}")
    cc = r.cast_counts()
    assert cc["casts"] == 42 and cc["rays"] == 42 * n
    # torch's default stream (the null stream): ordered like any torch operation on it
    got = r.cast_rays(d_rays)
    assert int(got[1].to(torch.int64).sum().item()) == int(ref["ids"].astype(np.int64).sum())
    _same_closest(got, (ref["tuv"], ref["ids"]), "default stream")
    # the context's own cast stream
    torch.cuda.synchronize()
    tuv = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    d = _lib.ArtRayCast(rays_dev=d_rays.data_ptr(), tuv_dev=tuv.data_ptr(), ids_dev=ids.data_ptr(), n=n, kind=_lib.ART_CAST_CLOSEST, cull_mask=0xFF)
    assert r._L.art_cast_rays(r._ctx, C.byref(d)) == 0
    r.cast_sync()
    _same_closest((tuv, ids), (ref["tuv"], ref["ids"]), "hip_stream NULL")
    assert r.cast_counts()["casts"] == 44
    r.close()


@pytest.mark.gpu
def test_sharded_contexts_and_several_frames_per_launch_cast_alike(R, torch, orc, get_scene):
    """a cast depends on neither the extent nor the shard"""
    ref = _ref(orc, get_scene, "cornell", 1.0, 4096)
    d_rays = _up(torch, ref["rays"])
    for kw, fpl in ((dict(shard=(1, 3)), 1), (dict(frames_in_flight=2), 2)):
        r = R.renderer_for_scene(ref["scene"], (96, 64), **kw)
        if fpl > 1:
            r.set_frames_per_launch(fpl)
        r.render_frame()
        tuv, ids, _ = _cast_both(r, torch, d_rays)
        assert np.array_equal(ids, ref["ids"]) and np.array_equal(tuv.view(np.uint32)[:, :3], ref["tuv"].view(np.uint32)[:, :3]), kw
        r.close()


@pytest.mark.gpu
def test_errors_change_nothing_and_enqueue_nothing(R, torch, get_scene):
    """every ART_E_INVALID case of include/art.h and ART_E_STATE before the build: the counts stay what they were.  No bad pointer ever reaches a launch."""
    from araytracingjourney_amd import _lib
    sc = get_scene("cornell")
    r = R.Renderer((64, 64))
    r.add_model(sc.primitives)
    L, ctx = r._L, r._ctx
    n = 64
    rays = _up(torch, random_rays(n + 1, 7))
    tuv = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    ids = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
    hit = torch.zeros((n + 1,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def closest(**kw):
        d = dict(rays_dev=rays.data_ptr(), tuv_dev=tuv.data_ptr(), ids_dev=ids.data_ptr(), hit_dev=None, hip_stream=None, n=n, kind=_lib.ART_CAST_CLOSEST, cull_mask=0xFF, flags=0)
        d.update(kw)
        return _lib.ArtRayCast(**d)

    def any_(**kw):
        return closest(**dict(dict(tuv_dev=None, ids_dev=None, hit_dev=hit.data_ptr(), kind=_lib.ART_CAST_ANY), **kw))

    def code(d):
        return L.art_cast_rays(ctx, C.byref(d) if d is not None else None)

    assert code(closest()) == _lib.ART_E_STATE and code(any_()) == _lib.ART_E_STATE and b"not built" in L.art_last_error()   # before the build
    r.prepare_first_frame()
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    assert L.art_cast_rays(None, C.byref(closest())) == _lib.ART_E_INVALID and code(None) == _lib.ART_E_INVALID
    bad = [closest(rays_dev=None), closest(tuv_dev=None), closest(ids_dev=None), closest(hit_dev=hit.data_ptr()),
           any_(hit_dev=None), any_(tuv_dev=tuv.data_ptr()), any_(ids_dev=ids.data_ptr()),
           closest(rays_dev=rays.data_ptr() + 4), closest(rays_dev=rays.data_ptr() + 8), closest(tuv_dev=tuv.data_ptr() + 8), closest(ids_dev=ids.data_ptr() + 4), any_(rays_dev=rays.data_ptr() + 4),
           closest(kind=2), any_(kind=0xFFFFFFFF), closest(cull_mask=0x100), any_(cull_mask=0xFFFFFFFF), closest(flags=1), any_(flags=0x80000000),
           closest(n=_lib.ART_CAST_MAX_RAYS + 1), any_(n=_lib.ART_CAST_MAX_RAYS + 1), closest(n=0xFFFFFFFF)]
    for d in bad:
        assert code(d) == _lib.ART_E_INVALID and L.art_last_error().startswith(b"art_cast_rays: "), (d.kind, d.n, d.cull_mask, d.flags)
    assert r.cast_counts() == dict(casts=0, rays=0, host_waits=0)
    assert L.art_cast_counts(None, None, None, None) == _lib.ART_E_INVALID and L.art_cast_sync(None) == _lib.ART_E_INVALID
    assert 2 ** 24 <= _lib.ART_CAST_MAX_RAYS < 2 ** 32
    # nothing was enqueued: the outputs are untouched, and a valid cast still works
    r.cast_sync()
    assert not tuv.any() and not ids.any() and not hit.any()
    assert code(closest(n=0)) == 0 and code(any_(n=0, rays_dev=None, hit_dev=None)) == 0 and r.cast_counts()["casts"] == 0   # n = 0 is legal and enqueues nothing
    assert code(closest()) == 0
    r.cast_sync()
    assert r.cast_counts() == dict(casts=1, rays=n, host_waits=0) and (ids[:n, 0] >= 0).any() and not ids[n:].any()
    # a primitive added since the build: art_scene_needs_build
    r.add_model([sc.primitives[0]])
    assert r.needs_build() and code(closest()) == _lib.ART_E_STATE and r.cast_counts()["casts"] == 1
    # the wrapper's own checks
    with pytest.raises(ValueError):
        r.cast_rays(rays.cpu())
    with pytest.raises(ValueError):
        r.cast_rays(rays.double())
    with pytest.raises(ValueError):
        r.cast_rays(rays[:, :7])
    with pytest.raises(ValueError):
        r.cast_rays(rays.t().contiguous().t())
    with pytest.raises(ValueError):
        r.cast_rays(rays, kind="nearest")
    with pytest.raises(ValueError):
        r.cast_rays(rays, out=(tuv[:8], ids))
    with pytest.raises(ValueError):
        r.cast_rays(rays, cull_mask=0x100)
    r.close()


def test_the_ctypes_descriptor_is_the_headers():
    """ArtRayCast as ctypes lays it out against sizeof / offsetof of include/art.h as gcc compiles it, field by field"""
    from araytracingjourney_amd import _lib
    _layout_is_the_headers("ArtRayCast", 56)
    hdr = open(os.path.join(ROOT, "include", "art.h")).read()
    for name in ("ART_CAST_CLOSEST", "ART_CAST_ANY", "ART_CAST_MAX_RAYS", "ART_CAST_POOL"):
        assert f"#define {name} {getattr(_lib, name)}u" in hdr, name


def test_a_cast_without_a_context_is_invalid_on_any_machine():
    """art_cast_rays(NULL, NULL) needs no device to say ART_E_INVALID"""
    from araytracingjourney_amd import _lib
    L = _lib.load()
    assert L.art_cast_rays(None, None) == _lib.ART_E_INVALID and b"art_cast_rays" in L.art_last_error()
    assert L.art_cast_sync(None) == _lib.ART_E_INVALID and L.art_cast_counts(None, None, None, None) == _lib.ART_E_INVALID
