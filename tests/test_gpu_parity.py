"""GPU parity tests proper: libart (HIP, through the C ABI) against the CPU oracle on the same inputs.
Bit-exact for geometry (LBVH, t/u/v/primitive/triangle, shadow bits, ray counts); 1e-4 relative for radiance."""
import numpy as np
import pytest

from conftest import assert_radiance_close, radiance_margin, record_margin
from helpers import _check_traversal_tree, degenerate_soup, oracle_camera, oracle_for, random_rays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from araytracingjourney_amd import renderer
    return renderer


@pytest.mark.parametrize("name,detail", [("cornell", 1.0), ("sponza_like", 0.12)])
@pytest.mark.parametrize("bits", [30, 63])
def test_lbvh_matches_oracle_bitwise(R, orc, get_scene, name, detail, bits):
    sc = get_scene(name, detail)
    r = R.renderer_for_scene(sc, (64, 64), morton_bits=bits)
    S = orc.Scene(sc.primitives, morton_bits=bits)
    dev, ref = r.get_lbvh(), S.lbvh()
    assert r.stats()["num_triangles"] == S.n_tris == sc.n_tris
    for k in ("keys", "leaf_gid", "child"):
        assert np.array_equal(dev[k], ref[k]), k
    for k in ("leaf_lo", "leaf_hi", "node_lo", "node_hi"):
        assert np.array_equal(dev[k].view(np.uint32), ref[k].view(np.uint32)), k
    r.close()


@pytest.mark.parametrize("name,detail", [("cornell", 1.0), ("sponza_like", 0.12)])
def test_ray_queries_match_oracle_bitwise(R, orc, get_scene, name, detail):
    sc = get_scene(name, detail)
    r = R.renderer_for_scene(sc, (64, 64))
    S = orc.Scene(sc.primitives, morton_bits=30)  # a different tree than the device's 63-bit one: results must not depend on it
    rays = random_rays(20000, 7)
    tuv, ids = r.query_closest(rays)
    rtuv, rids, _, _ = S.trace_closest(rays)
    assert np.array_equal(ids, rids)
    assert np.array_equal(tuv.view(np.uint32)[:, :3], rtuv.view(np.uint32)[:, :3])
    assert (ids[:, 0] >= 0).sum() > 1000
    short = rays.copy()
    short[:, 7] = 1.5
    hit = r.query_any(short)
    rhit, _, _ = S.trace_any(short)
    assert np.array_equal(hit, rhit)
    assert 0 < hit.sum() < hit.size
    r.close()


FORMS = {"fused": (3, {}), "fused-1": (1, {}), "per-ray": (1, {"frame_form": 2}), "per-ray-3": (3, {"frame_form": 2}), "fused-binary": (3, {"packet_wide": 2})}   # ArtTuning (art_set_tuning): the forms libart keeps (round 4
# removed the staged packet kernels, the packet's beam as node step, PLOC trees and the 6- / 7-wave instances: measured, lost, gone)


def _frame_parity(R, orc, sc, w, h, n_lights, form="fused"):
    # the forms of the frame: one fused launch (packet walks over the 4-wide or the binary nodes), four staged launches with the per-ray walks (binary for primary rays,
    # 4-wide for shadow rays)
    fif, tuning = FORMS[form]
    r = R.renderer_for_scene(sc, (w, h), n_lights=n_lights, keep_debug=True, frames_in_flight=fif, tuning=tuning)
    r.render_frame()
    S, L, nl = oracle_for(orc, sc, n_lights)
    ref = S.render(oracle_camera(orc, sc, w, h), L, nl, w, h, threads=8, debug=True)
    tuv, ids = r.read_hits()
    assert np.array_equal(ids, ref["hit_id"]), f"{int((ids != ref['hit_id']).any(-1).sum())} hit ids differ"
    assert np.array_equal(tuv.view(np.uint32)[..., :3], ref["hit_tuv"].view(np.uint32)[..., :3])
    assert np.array_equal(r.read_shadow_bits(), ref["shadow_bits"])
    st = r.stats()
    assert st["primary_rays"] == ref["stats"]["primary_rays"] == w * h
    assert st["shadow_rays"] == ref["stats"]["shadow_rays"]
    assert st["hit_pixels"] == ref["stats"]["hit_pixels"]
    assert ref["stats"]["nonfinite_pixels"] == 0
    color = r.read_color()
    assert_radiance_close(color, ref["color"])
    assert_radiance_close(r.read_depth(), ref["depth"], what="depth")
    assert_radiance_close(r.read_normal(), ref["normal"], rel=1e-4, floor=1e-5, what="normal")
    r.close()
    ref["margin"] = radiance_margin(color[..., :3], ref["color"][..., :3])   # how much of the 1e-4 the fast intrinsics (__powf, __fdividef) use
    return ref


def _golden_stats(tag):
    import json, os
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", tag + ".stats.json")))


def _check_against_golden(tag, ref, keys=("primary_rays", "shadow_rays", "hit_pixels", "n_int_primary", "n_tri_primary", "n_int_shadow", "n_tri_shadow")):
    """the oracle's counters for this frame are the committed ones (bench.py prices its roofline with them); the GPU frame's margin under
    the 1e-4 tolerance is recorded, and must not have grown past twice the committed one (same GPU libm: it is deterministic)"""
    fx = _golden_stats(tag)
    for k in keys:
        assert ref["stats"][k] == fx[k], k
    record_margin(tag, ref["margin"])
    assert ref["margin"]["worst_tolerance_fraction"] <= 1.0
    if "gpu_margin" in fx:
        assert ref["margin"]["worst_rel_err"] <= 2.0 * fx["gpu_margin"]["worst_rel_err"] + 1e-7, (ref["margin"], fx["gpu_margin"])


@pytest.mark.parametrize("form", ["fused", "fused-1", "per-ray-3", "per-ray"])
def test_cornell_frame_matches_oracle(R, orc, get_scene, form):
    ref = _frame_parity(R, orc, get_scene("cornell"), 256, 256, None, form)
    assert ref["stats"]["shadow_rays"] > 1000


@pytest.mark.parametrize("form", ["fused", "fused-binary", "per-ray-3", "per-ray"])
@pytest.mark.parametrize("n_lights", [1, 4])
def test_sponza_frame_matches_oracle(R, orc, scenes, get_scene, n_lights, form):
    sc = get_scene("sponza_like", 0.12)
    if n_lights == 4:
        sc = scenes.Scene(sc.name, sc.primitives, sc.camera, scenes.sponza_lights(4))
    ref = _frame_parity(R, orc, sc, 480, 270, None, form)
    assert ref["stats"]["shadow_rays"] > 10000


def test_config2_full_size_frame_matches_oracle(R, orc, get_scene):
    """BASELINE config 2 at its real size: 262 816 triangles, 1920x1080, one directional light"""
    import json, os
    _frame_parity(R, orc, get_scene("sponza_like", 1.0), 1920, 1080, 1, "per-ray")
    ref = _frame_parity(R, orc, get_scene("sponza_like", 1.0), 1920, 1080, 1, "fused")   # the fused frame, as bench.py runs it
    _check_against_golden("c2_sponza_like_1080p_1light", ref)


def test_config3_full_size_frame_matches_oracle(R, orc, scenes, get_scene):
    """BASELINE config 3 at its real size: 262 816 triangles, 3840x2160, point + spot + directional + area light, 17.8 M shadow rays:
    hit ids / t / u / v / shadow bits / ray counts bit-exact, radiance within 1e-4 (raytrace.rgen.glsl:139-187)"""
    sc = get_scene("sponza_like", 1.0)
    sc = scenes.Scene(sc.name, sc.primitives, sc.camera, scenes.sponza_lights(4))
    ref = _frame_parity(R, orc, sc, 3840, 2160, None, "fused")
    assert ref["stats"]["shadow_rays"] > 17_000_000
    _check_against_golden("c3_sponza_like_2160p_4lights", ref)


def test_config4_full_size_frame_matches_oracle(R, orc, get_scene):
    """BASELINE config 4's frame at its real size on one GPU: 2.8 M triangles (63-bit keys on the device, 30-bit in the oracle), 1920x1080"""
    ref = _frame_parity(R, orc, get_scene("bistro_like", 1.0), 1920, 1080, None, "fused")
    _check_against_golden("c4_bistro_like_1080p_1light", ref)


def test_config5_full_size_ao_matches_oracle(R, orc, get_scene):
    """BASELINE config 5 at its real size: 3840x2160, 16 AO rays per hit pixel (113 M rays) on the frame's own depth + normal outputs
    (vk_xe_gtao.rs:17-23): the G-buffer inputs and the 0..255 integer output are bit-exact"""
    import zlib
    sc = get_scene("sponza_like", 1.0)
    w, h, spp, radius = 3840, 2160, 16, 0.2 * 1.457
    r = R.renderer_for_scene(sc, (w, h), n_lights=1)
    r.render_frame(sync=False)
    r.trace_ao(spp, radius)
    got = r.read_ao()
    S, L, nl = oracle_for(orc, sc, 1)
    cam = oracle_camera(orc, sc, w, h)
    ref = S.render(cam, L, nl, w, h, threads=16)
    assert np.array_equal(r.read_depth().view(np.uint32), ref["depth"].view(np.uint32))
    assert np.array_equal(r.read_normal().view(np.uint32), ref["normal"].view(np.uint32))
    want, st = orc.render_ao(S, cam, ref["depth"], ref["normal"], spp, radius, threads=16)
    assert np.array_equal(got, want), f"{int((got != want).sum())} AO values differ"
    fx = _golden_stats("c5_sponza_like_2160p_16spp_ao")
    assert r.stats()["ao_rays"] == st["ao_rays"] == fx["ao_rays"] == ref["stats"]["hit_pixels"] * spp
    assert st["n_int_ao"] == fx["n_int_ao"] and st["n_tri_ao"] == fx["n_tri_ao"] and zlib.crc32(want.tobytes()) == fx["ao_crc32"]
    r.close()


def test_config4_bistro_class_scene(R, orc, get_scene):
    """BASELINE config 4's scene (2.8 M triangles, 120 primitives, 63-bit Morton keys on the device, 30-bit in the oracle):
    device LBVH invariants at full size, then frame parity at 960x540"""
    sc = get_scene("bistro_like", 1.0)
    assert abs(sc.n_tris - 2.8e6) / 2.8e6 < 0.01 and len(sc.primitives) == 120
    r = R.renderer_for_scene(sc, (64, 64))
    b = r.get_lbvh()
    T = sc.n_tris
    assert np.array_equal(np.sort(b["leaf_gid"]), np.arange(T, dtype=np.uint32))
    k = b["keys"].astype(np.uint64)
    assert np.all(k[1:] >= k[:-1]) and np.all((k[1:] > k[:-1]) | (b["leaf_gid"][1:] > b["leaf_gid"][:-1]))
    child = b["child"]
    lo = np.concatenate([b["node_lo"], b["leaf_lo"]]); hi = np.concatenate([b["node_hi"], b["leaf_hi"]])
    idx = np.where(child < 0, (T - 1) + (~child), child)
    assert np.array_equal(lo[:T - 1], np.minimum(lo[idx[:, 0]], lo[idx[:, 1]])) and np.array_equal(hi[:T - 1], np.maximum(hi[idx[:, 0]], hi[idx[:, 1]]))
    seen = np.bincount(idx.reshape(-1), minlength=2 * T - 1)
    assert seen[0] == 0 and np.all(seen[1:] == 1)                # every node and leaf has exactly one parent
    r.close()


def test_ragged_extent_and_resize(R, orc, get_scene):
    """extent not a multiple of the 32-pixel tile; then a resize (vk_rt_lightning_shadows.rs:125)"""
    sc = get_scene("cornell")
    r = R.renderer_for_scene(sc, (100, 52))
    S, L, nl = oracle_for(orc, sc)
    for (w, h) in [(100, 52), (37, 91)]:
        r.resize((w, h))
        r.render_frame()
        ref = S.render(oracle_camera(orc, sc, w, h), L, nl, w, h, threads=4)
        assert_radiance_close(r.read_color(), ref["color"])
    r.close()


def test_sharded_tiles_gather_to_the_unsharded_frame(R, get_scene):
    """screen-tile split: 3 shard contexts on one GPU, tiles concatenated as a gather would, un-tiled by shard 0"""
    import torch
    sc = get_scene("cornell")
    w, h, G = 200, 136, 3
    whole = R.renderer_for_scene(sc, (w, h))
    whole.render_frame()
    want = whole.read_color()
    shards = [R.renderer_for_scene(sc, (w, h), shard=(k, G)) for k in range(G)]
    bufs = []
    for s in shards:
        s.render_frame()
        bufs.append(s.read_color_tiles())
    gathered = torch.from_numpy(np.concatenate(bufs)).cuda()   # what dist.gather leaves on the root
    torch.cuda.synchronize()
    shards[0].untile_gathered(gathered.data_ptr(), G)
    got = shards[0].read_color()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    owned = [s.shard_tile_count()[0] for s in shards]
    assert sum(owned) == ((w + 31) // 32) * ((h + 31) // 32) and max(owned) - min(owned) <= 2
    for s in shards + [whole]:
        s.close()


def test_tile_buffer_pairs_alternate_per_trip(R, get_scene):
    """art_bind_color_tiles_pair: a ring slot writes its two caller-owned tile buffers on alternate trips round the ring, so the exchange
    that still reads one is never in the next frame's way; several frames are un-tiled by one launch (art_untile_gathered_frames)"""
    import torch
    from araytracingjourney_amd import sharding
    sc = get_scene("cornell")
    w, h, G, F = 160, 96, 2, 2
    whole = R.renderer_for_scene(sc, (w, h))
    shards = [R.renderer_for_scene(sc, (w, h), shard=(k, G), frames_in_flight=F) for k in range(G)]
    owned, padded = shards[0].shard_tile_count()
    bufs = [torch.zeros((2, F, padded, 32, 32, 3), dtype=torch.float32, device="cuda") for _ in range(G)]
    for s, b in zip(shards, bufs):
        for k in range(F):
            s.bind_color_tiles_pair(k, b[0, k].data_ptr(), b[1, k].data_ptr(), b[0, k].numel() * 4)
    want = []
    for i in range(2 * F):                                   # two trips: frame i lands in buffer [i // F % 2][i % F]
        pos = (0.02 * i, 0.01 * i, -0.95)
        for r in [whole] + shards:
            r.camera_mut().set_pos(pos)
            r.upload_state()
            r.trace()
        want.append(whole.read_color())
    for s in shards:
        s.sync()
    for i in range(2 * F):
        for k, b in enumerate(bufs):
            ref = sharding.tile_host(want[i][..., :3], G, k)   # the tiles carry RGB; alpha is the constant 1
            n = shards[k].shard_tile_count()[0]
            assert np.array_equal(b[i // F % 2, i % F, :n].cpu().numpy().view(np.uint32), ref[:n].view(np.uint32)), (i, k)
    # the second trip's two frames, gathered [shard][slot] and un-tiled by ONE launch
    gathered = torch.stack([b[1] for b in bufs]).contiguous()             # [G, F, padded, 32, 32, 3]
    frames = torch.zeros((F, h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    shards[0].untile_gathered(gathered.data_ptr(), G, frames.data_ptr(), None, shard_stride_tiles=F * padded, n_frames=F)
    shards[0].sync(); torch.cuda.synchronize()
    for j in range(F):
        assert np.array_equal(frames[j].cpu().numpy().view(np.uint32), want[F + j].view(np.uint32)), j
    for r in [whole] + shards:
        r.close()


def test_tile_buffer_ring_and_host_side_frame_completion(R, get_scene):
    """art_bind_color_tiles_ring: a slot's frames write its n caller-owned buffers in turn, one per trip round the frame ring;
    art_frames_done: non-blocking host-side "have frames [first, first + count) finished", which lets an exchange be submitted without
    device-side waits; argument errors of both"""
    import torch
    from araytracingjourney_amd import sharding
    from araytracingjourney_amd._lib import ArtError
    sc = get_scene("cornell")
    w, h, G, F, NB = 160, 96, 2, 2, 3
    whole = R.renderer_for_scene(sc, (w, h))
    s = R.renderer_for_scene(sc, (w, h), shard=(1, G), frames_in_flight=F)
    owned, padded = s.shard_tile_count()
    b = torch.zeros((NB, F, padded, 32, 32, 3), dtype=torch.float32, device="cuda")
    for k in range(F):
        s.bind_color_tiles_ring(k, [b[i, k].data_ptr() for i in range(NB)], b[0, k].numel() * 4)
    assert s.frames_traced() == 0 and s.frames_done(0, 0)
    with pytest.raises(ArtError):
        s.frames_done(0, 1)                                   # not traced yet
    want = []
    for i in range(NB * F + 1):                               # frame i lands in buffer [i // F % NB][i % F]; the last one wraps round
        pos = (0.02 * i, 0.01 * i, -0.95)
        for r in (whole, s):
            r.camera_mut().set_pos(pos)
            r.upload_state()
            r.trace()
        want.append(sharding.tile_host(whole.read_color()[..., :3], G, 1))
    assert s.frames_traced() == NB * F + 1
    s.sync()
    assert s.frames_done(0, NB * F + 1) and s.frames_done(NB * F, 1)
    for i in range(1, NB * F + 1):                            # frame 0's buffer was rewritten by the last frame
        assert np.array_equal(b[i // F % NB, i % F, :owned].cpu().numpy().view(np.uint32), want[i][:owned].view(np.uint32)), i
    with pytest.raises(ArtError):
        s.bind_color_tiles_ring(0, [b[0, 0].data_ptr()] * 9, b[0, 0].numel() * 4)   # at most 8 buffers
    with pytest.raises(ArtError):
        s.bind_color_tiles_ring(0, [b[0, 0].data_ptr(), 0], b[0, 0].numel() * 4)     # null buffer
    for r in (whole, s):
        r.close()


def test_packed_tiles_gather_to_the_packed_colour_image(R, get_scene):
    """ART_FLAG_PACKED_TILES: the gather payload is B10G11R11 (the reference's colour image format, renderer.rs:268), 4 B per pixel;
    un-tiled on shard 0 it equals the packed colour of the unsharded frame; several frames in flight and one"""
    import torch
    sc = get_scene("cornell")
    w, h, G = 200, 136, 3
    whole = R.renderer_for_scene(sc, (w, h))
    whole.render_frame()
    whole.present()
    want = whole.read_packed()[0]
    for fif in (4, 1):
        shards = [R.renderer_for_scene(sc, (w, h), shard=(k, G), packed_tiles=True, frames_in_flight=fif) for k in range(G)]
        bufs = []
        for s in shards:
            s.render_frame()
            bufs.append(s.read_color_tiles())
        assert bufs[0].dtype == np.uint32 and bufs[0].shape[1:] == (32, 32)
        gathered = torch.from_numpy(np.concatenate(bufs).view(np.int32)).cuda()
        frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        shards[0].untile_gathered(gathered.data_ptr(), G, frame.data_ptr())
        shards[0].sync()
        torch.cuda.synchronize()
        assert np.array_equal(frame.cpu().numpy().view(np.uint32), want), fif
        for s in shards:
            s.close()
    whole.close()


@pytest.mark.parametrize("name,detail,fast", [("cornell", 1.0, False), ("sponza_like", 0.12, False), ("sponza_like", 0.12, True), ("sponza_like", 1.0, False)])
def test_wide_collapse_on_the_device_equals_the_host_loop(R, get_scene, name, detail, fast):
    """the 4-wide nodes the packet and per-ray walks read (art_get_wide_nodes): the level-by-level device collapse emits, bit for bit, the arrays of the
    one-thread host loop it replaced (same greedy expansion, same child order, same breadth-first numbering, same quantisation); and they are a tree
    over all leaves with boxes that contain their children's"""
    sc = get_scene(name, detail)
    dev = R.renderer_for_scene(sc, (64, 64), fast_build=fast)
    host = R.renderer_for_scene(sc, (64, 64), fast_build=fast, tuning={"wide_builder": 1})
    qd, fd = dev.get_wide_nodes()
    qh, fh = host.get_wide_nodes()
    assert qd.shape == qh.shape and len(qd) >= 1
    assert np.array_equal(qd, qh) and np.array_equal(fd, fh)
    T = dev.stats()["num_triangles"]
    child = fd[:, 24:28].view(np.int32)
    valid = child != -2**31                                                       # an absent child refers to INT32_MIN, the walks' "pop" value
    assert np.array_equal(valid, ((fd[:, 28][:, None] >> np.arange(4)) & 1).astype(bool))  # ... and the valid bits say the same
    assert np.array_equal(child, qd[:, 12:16].view(np.int32))
    leaves = np.sort(~child[valid & (child < 0)])
    assert np.array_equal(leaves, np.arange(T))                                  # every leaf exactly once
    inner = np.sort(child[valid & (child >= 0)])
    assert np.array_equal(inner, np.arange(1, len(fd)))                          # every node but the root has exactly one parent
    boxes = fd[:, :24].view(np.float32).reshape(-1, 4, 6)
    for k in range(4):                                                           # a child's box contains its own children's boxes
        sel = valid[:, k] & (child[:, k] >= 0)
        sub = boxes[child[sel, k]]
        sub_valid = valid[child[sel, k]]
        lo = np.where(sub_valid[..., None], sub[..., :3], np.inf).min(1)
        hi = np.where(sub_valid[..., None], sub[..., 3:], -np.inf).max(1)
        assert np.all(boxes[sel, k, :3] <= lo) and np.all(boxes[sel, k, 3:] >= hi)
    dev.close(); host.close()


@pytest.mark.parametrize("walk", [0, 2, 6], ids=["default", "binary", "generic-tracer"])
@pytest.mark.parametrize("name,detail,size,spp", [("cornell", 1.0, (256, 256), 16), ("sponza_like", 0.12, (480, 270), 16), ("sponza_like", 0.12, (200, 120), 5)])
def test_ray_traced_ao_matches_oracle_exactly(R, orc, get_scene, name, detail, size, spp, walk):
    """BASELINE config 5's pass: AO rays from the frame's depth + normal outputs; the 0..255 output is an integer: bit-exact"""
    sc = get_scene(name, detail)
    w, h = size
    radius = 0.2 * 1.457
    r = R.renderer_for_scene(sc, (w, h), tuning={"ao_walk": walk} if walk else None)   # either walk the AO rays can take (ArtTuning.ao_walk) gives the same integers
    r.render_frame(sync=False)
    r.trace_ao(spp, radius)
    got = r.read_ao()
    S, L, nl = oracle_for(orc, sc)
    cam = oracle_camera(orc, sc, w, h)
    ref = S.render(cam, L, nl, w, h, threads=8)
    assert np.array_equal(r.read_depth().view(np.uint32), ref["depth"].view(np.uint32))        # the AO inputs themselves are bit-equal
    assert np.array_equal(r.read_normal().view(np.uint32), ref["normal"].view(np.uint32))
    want, st = orc.render_ao(S, cam, ref["depth"], ref["normal"], spp, radius, threads=8)
    assert np.array_equal(got, want), f"{int((got != want).sum())} AO values differ"
    assert r.stats()["ao_rays"] == st["ao_rays"] == ref["stats"]["hit_pixels"] * spp
    assert got.min() < 128 and got.max() == 255
    r.close()


def test_glb_ingest_feeds_the_same_frame(R, get_scene, tmp_path):
    """add_model through the GLB reader (renderer.rs:346 -> vk_model.rs:494-528) == handing the same primitives over directly"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from glb_writer import write_glb
    from araytracingjourney_amd import model_reader as mr
    sc = get_scene("cornell")
    path = tmp_path / "cornell.glb"
    write_glb(str(path), sc.primitives, png_modes=("RGBA", "RGBA", "RGBA"))
    direct = R.renderer_for_scene(sc, (128, 128), keep_debug=True)
    direct.render_frame()
    g = R.Renderer((128, 128), keep_debug=True)
    ids = g.add_model_glb(mr.GltfModelReader(str(path), True, mr.COERCE_B8G8R8A8), sc.primitives[0].model)
    assert ids == [0, 1, 2]
    cam = g.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"])
    for d in sc.lights:
        g.lights_mut().push_dict(d)
    g.prepare_first_frame()
    g.render_frame()
    assert np.array_equal(g.read_color().view(np.uint32), direct.read_color().view(np.uint32))
    assert np.array_equal(g.read_hits()[1], direct.read_hits()[1])
    g.close(); direct.close()


def test_cpp_host_mirror_renders_a_glb(R, get_scene, tmp_path):
    """main.rs:15-66 on the C++ mirror: add_model(.glb) + lights + prepare_first_frame + render_frame + compute_ao; then Model::set_model_matrix (vk_model.rs:461-466)
    there and back: two refits, the moved frame differs, the frame of the model back in place is the first one bit for bit"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    from glb_writer import write_glb
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    sc = get_scene("cornell")
    path = tmp_path / "cornell.glb"
    write_glb(str(path), sc.primitives, png_modes=("RGBA", "RGBA", "RGBA"))
    out = subprocess.run([os.path.join(root, "examples", "host_mirror_demo"), "render", str(path), "160", "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "RENDER_OK" in out.stdout, out.stdout + out.stderr
    f = dict(kv.split("=") for kv in out.stdout.split("RENDER_OK")[1].split("\n")[0].split())
    assert int(f["tris"]) == 34 and int(f["primary"]) == 160 * 96 and int(f["hit"]) > 1000 and int(f["ao"]) == 16 * int(f["hit"]) and float(f["colour_sum"]) > 0
    m = dict(kv.split("=") for kv in out.stdout.split("MOVED_OK")[1].split("\n")[0].split())
    assert (int(m["refits"]), int(m["rebuilds"]), int(m["moved_differs"]), int(m["back_equals_first"])) == (2, 0, 1, 1) and float(m["refit_ms"]) > 0, out.stdout
    res = dict(kv.split("=") for kv in out.stdout.split("RESIDENT_OK")[1].split())     # the model leaves (camera 30 units away) and re-enters the structure without a build
    assert {k: int(v) for k, v in res.items()} == dict(hit_when_out=0, tris_when_out=0, tris_back=34, rebuilds=0, refits=4, back_equals_first=1), out.stdout


def test_frame_ring_gives_the_same_frames(R, get_scene):
    """3 frames in flight (the reference's FrameData ring, renderer.rs:135): every frame equals the single-slot render"""
    sc = get_scene("cornell")
    one = R.renderer_for_scene(sc, (160, 96))
    ring = R.renderer_for_scene(sc, (160, 96), frames_in_flight=3)
    assert ring.frames_in_flight() == (3, 0)
    for i in range(7):
        pos = (0.02 * i, 0.0, -0.95)
        for r in (one, ring):
            r.camera_mut().set_pos(pos)
            r.upload_state()
            r.trace()
        assert ring.frames_in_flight()[1] == (i + 1) % 3
        assert np.array_equal(ring.read_color().view(np.uint32), one.read_color().view(np.uint32)), i
        assert np.array_equal(ring.read_depth().view(np.uint32), one.read_depth().view(np.uint32))
    for i in range(9):          # same camera, no host sync between frames
        ring.trace()
    assert np.array_equal(ring.read_color().view(np.uint32), one.read_color().view(np.uint32))
    ring.set_graph_mode(True)   # replayed hipGraphs: same frames; a camera change re-captures
    for i in range(7):
        ring.trace()
    assert np.array_equal(ring.read_color().view(np.uint32), one.read_color().view(np.uint32))
    for r in (one, ring):
        r.camera_mut().set_pos((0.11, 0.02, -0.9))
        r.upload_state()
        r.trace()
    assert np.array_equal(ring.read_color().view(np.uint32), one.read_color().view(np.uint32))
    assert ring.stats()["shadow_rays"] == one.stats()["shadow_rays"]
    one.close()
    ring.close()


def test_frame_forms_and_trees_give_the_same_frame(R, get_scene):
    """the fused frame kernel (4-wide and binary nodes), the per-ray kernels -- on the device's SAH tree, the host's, and on the LBVH topology
    (ART_FLAG_FAST_BUILD): one frame, bit for bit (colour, depth, normal, ray counts); 4 lights so the light loop is covered"""
    from araytracingjourney_amd import scenes
    sc = get_scene("sponza_like", 0.12)
    w, h = 320, 200
    def frame(frames_in_flight, fast_build=False, tuning=None):
        r = R.renderer_for_scene(sc, (w, h), n_lights=0, frames_in_flight=frames_in_flight, fast_build=fast_build, tuning=tuning)
        for d in scenes.sponza_lights(4):
            r.lights_mut().push_dict(d)
        r.render_frame()
        out = (r.read_color(), r.read_depth(), r.read_normal(), r.stats())
        r.close()
        return out
    ref = frame(4)                                               # fused, SAH (the default with several frames in flight)
    assert ref[3]["frame_launches"] == 1 and ref[3]["shadow_rays"] > 10000
    for name, got in (("per-ray", frame(1, tuning={"frame_form": 2})), ("per-ray, four frames in flight", frame(4, tuning={"frame_form": 2})), ("fused, one frame in flight", frame(1)),
                      ("fused on the LBVH topology", frame(4, fast_build=True)), ("per-ray on the LBVH topology", frame(1, fast_build=True, tuning={"frame_form": 2})),
                      ("fused on the host-built SAH tree", frame(4, tuning={"tree_builder": 1})), ("fused, no block reordering", frame(4, tuning={"block_order": 1})),
                      ("per-ray, 4-wide nodes for primary rays too", frame(2, tuning={"frame_form": 2, "primary_walk": 4})), ("per-ray, binary nodes for shadow rays too", frame(2, tuning={"frame_form": 2, "shadow_walk": 2})),
                      ("fused, binary packet nodes", frame(4, tuning={"packet_wide": 2})), ("fused, 4-wide collapse on the host", frame(4, tuning={"wide_builder": 1}))):
        for k in range(3):
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (name, k)
        assert got[3]["shadow_rays"] == ref[3]["shadow_rays"] and got[3]["hit_pixels"] == ref[3]["hit_pixels"], name
    assert frame(4, tuning={"frame_form": 2})[3]["frame_launches"] == 4


def test_wave_plan_changes_the_waves_never_the_image(R, get_scene):
    """the fused frame's adaptive wave plan (ART_FLAG_FIXED_WAVES off): after a sampled frame heavy 8x8 blocks are dealt to 4 / 16 waves --
    the same frame bit for bit before and after, unsharded, sharded, with one light and four, and equal to the fixed-wave frame"""
    from araytracingjourney_amd import scenes
    sc = get_scene("sponza_like", 0.12)
    w, h = 640, 360
    low = {"split_fixed_steps": 40}                      # a low step target, so that plenty of blocks split in this small scene
    for n_lights, shard in ((1, (0, 1)), (4, (0, 1)), (4, (1, 3))):
        fixed = R.renderer_for_scene(sc, (w, h), n_lights=0, frames_in_flight=1, fixed_waves=True, shard=shard)
        r = R.renderer_for_scene(sc, (w, h), n_lights=0, frames_in_flight=2, shard=shard, tuning=low)
        for x in (fixed, r):
            for d in scenes.sponza_lights(n_lights):
                x.lights_mut().push_dict(d)
        fixed.render_frame()
        ref = (fixed.read_color(), fixed.read_depth(), fixed.read_normal(), fixed.stats())
        assert ref[3]["split_blocks"] == 0
        seen = set()
        for i in range(12):                              # the first frame is sampled; a later one runs on the new plan, and is sampled in turn
            r.render_frame()
            r.sync()
            st = r.stats()
            seen.add(st["split_blocks"])
            got = (r.read_color(), r.read_depth(), r.read_normal())
            for k in range(3):
                assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (n_lights, shard, i, k)
            assert st["shadow_rays"] == ref[3]["shadow_rays"] and st["hit_pixels"] == ref[3]["hit_pixels"]
            if shard[1] > 1:
                assert np.array_equal(r.read_color_tiles().view(np.uint32), fixed.read_color_tiles().view(np.uint32))
        assert 0 in seen and max(seen) > 20, seen        # it started unsplit and did split
        fixed.close()
        r.close()


def test_several_frames_per_launch_equal_the_single_frames(R, get_scene):
    """art_set_frames_per_launch: one launch traces n frames, each with its own camera (art_set_camera_batch); every frame -- colour,
    depth, normal, ray counts, and the compact tiles of a sharded context -- equals the frame traced alone; 1 and 4 lights"""
    import torch
    from araytracingjourney_amd import scenes
    from araytracingjourney_amd._lib import ArtError
    sc = get_scene("sponza_like", 0.12)
    w, h, B = 320, 200, 3
    for n_lights, shard in ((1, (0, 1)), (4, (1, 2))):
        one = R.renderer_for_scene(sc, (w, h), n_lights=0, frames_in_flight=1, shard=shard)
        many = R.renderer_for_scene(sc, (w, h), n_lights=0, frames_in_flight=2, shard=shard)
        for x in (one, many):
            for d in scenes.sponza_lights(n_lights):
                x.lights_mut().push_dict(d)
        many.set_frames_per_launch(B)
        many.upload_state()
        cams = []
        for b in range(B):
            p0, c0 = sc.camera["pos"], many.camera_mut()
            cams.append(R.Camera((p0[0] + 0.05 * b, p0[1] + 0.02 * b, p0[2] - 0.03 * b), c0.dir(), c0.aspect(), c0.fovy(), c0._znear, c0._zfar))
        tiles = None
        if shard[1] > 1:
            owned, padded = many.shard_tile_count()
            tiles = torch.zeros((2, B, padded, 32, 32, 3), dtype=torch.float32, device="cuda")
            with pytest.raises(ArtError):
                many.bind_color_tiles(0, tiles[0, 0].data_ptr(), tiles[0, 0].numel() * 4)      # one frame's worth: too small
            for k in range(2):
                many.bind_color_tiles(k, tiles[k].data_ptr(), tiles[k].numel() * 4)
        for trip in range(3):                                 # the second and third launches run on the wave plan of the first
            many.set_camera_batch(cams)
            many.trace()
            many.sync()
            for b in range(B):
                one.camera_mut().set_pos(cams[b].pos())
                one.render_frame()
                many.set_read_frame(b)
                for name in ("read_color", "read_depth", "read_normal"):
                    assert np.array_equal(getattr(many, name)().view(np.uint32), getattr(one, name)().view(np.uint32)), (n_lights, shard, trip, b, name)
                so, sm = one.stats(), many.stats()
                assert sm["shadow_rays"] == so["shadow_rays"] and sm["hit_pixels"] == so["hit_pixels"]
                if tiles is not None:
                    assert np.array_equal(many.read_color_tiles().view(np.uint32), one.read_color_tiles().view(np.uint32))
                    assert np.array_equal(tiles[trip % 2, b].cpu().numpy().view(np.uint32), one.read_color_tiles().view(np.uint32))
        with pytest.raises(ArtError):
            many.trace_ao(4)
        with pytest.raises(ArtError):
            many.set_read_frame(B)
        with pytest.raises(ArtError):
            many.set_frames_per_launch(5)
        one.close()
        many.close()


def test_residency_only_device_models_are_traced(R, get_scene):
    """renderer.rs:637-651 + vk_model.rs:334-345: a model farther than 10 units from the camera leaves the acceleration structure
    (the frame equals the one without it), comes back when the camera approaches; with nothing in range every ray misses"""
    sc = get_scene("cornell")
    w, h = 128, 96
    far = np.array([[1, 0, 0, 30.0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)   # the same boxes, 30 units to the right
    both = R.Renderer((w, h), frames_in_flight=2)
    near_ids = both.add_model(sc.primitives)
    far_ids = both.add_model(sc.primitives, far)
    for d in sc.lights:
        both.lights_mut().push_dict(d)
    cam = both.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    both.prepare_first_frame()
    assert [m.state for m in both.models_mut()] == [R.DEVICE, R.STORAGE]
    both.render_frame()
    only = R.renderer_for_scene(sc, (w, h), frames_in_flight=2)
    only.render_frame()
    assert np.array_equal(both.read_color().view(np.uint32), only.read_color().view(np.uint32))
    assert both.stats()["num_triangles"] == only.stats()["num_triangles"] == 34
    # camera next to the far copy: that one is instanced now, the first one is 30 units away (Storage)
    p = sc.camera["pos"]
    cam.set_pos((p[0] + 30.0, p[1], p[2]))
    both.render_frame()
    assert [m.state for m in both.models_mut()] == [R.STORAGE, R.DEVICE]
    d1, d0 = both.read_depth(), only.read_depth()                 # the same boxes seen from the same relative position (x + 30 costs float precision)
    hit1, hit0 = d1 < 10000.0, d0 < 10000.0
    assert (hit1 != hit0).mean() < 1e-3 and np.allclose(d1[hit1 & hit0], d0[hit1 & hit0], rtol=1e-3)
    # half way: both copies are 14 units off -> Host, nothing is traced
    cam.set_pos((p[0] + 15.0, p[1], p[2]))
    both.render_frame()
    assert [m.state for m in both.models_mut()] == [R.HOST, R.HOST]
    st = both.stats()
    assert st["hit_pixels"] == 0 and st["shadow_rays"] == 0 and np.all(both.read_depth() == 10000.0)
    both.close(); only.close()


@pytest.mark.parametrize("builder", ["sah-device", "sah-host"])
@pytest.mark.parametrize("name,detail", [("cornell", 1.0), ("sponza_like", 0.12), ("sponza_like", 1.0)])
def test_traversal_tree_is_a_tree_of_exact_boxes(R, get_scene, name, detail, builder):
    """what makes the SAH rebuild invisible: every leaf of the canonical LBVH hangs in the traversal tree exactly once,
    every node box is the exact min/max union of its children's boxes, the root is node 0, the depth stays inside the walks' stacks"""
    r = R.renderer_for_scene(get_scene(name, detail), (64, 64), tuning={"tree_builder": 1} if builder == "sah-host" else None)   # binned SAH on the device (default) / on the host threads
    _check_traversal_tree(r)
    r.close()


@pytest.mark.parametrize("n_tris,shape", [(16, "soup"), (17, "soup"), (18, "soup"), (40, "soup"), (300, "soup"), (4096, "soup"), (4097, "soup"), (4200, "soup"), (9000, "soup"),
                                          (6000, "flat"), (6000, "line"), (20000, "clusters"), (5000, "one point"), (30000, "soup")])
def test_device_sah_at_the_sizes_where_its_kernels_change(R, orc, n_tris, shape):
    """The device builder takes each range by the kernel that fits its size (art_sahdev.hip: a thread per range of <= 16 leaves, a block per range of <= 4 096, bins in memory
    above; a level is one fused kernel once no large range is open): scenes of exactly the sizes where that changes -- the whole scene one small range, one leaf more, a
    range that just fits a block's LDS staging and one that does not, a root that is large with children that are not -- must give a valid tree of exact boxes, and ray
    queries the oracle's answers bit for bit.  Degenerate on purpose: a quarter of the triangles are copies of their neighbours (equal centroids: flat domains, ties); and
    shapes that starve the heuristic: every centroid in one plane, on one line, in a dozen far-apart clumps (ranges that stay large down one side), in ONE point (no plane
    separates anything: median splits all the way)."""
    sc = degenerate_soup(n_tris, shape)   # (tests/helpers.py: tests/test_walk_edges.py sends the same soups through every walk)
    S, L, nl = oracle_for(orc, sc)
    rays = random_rays(6000, n_tris)
    rtuv, rids, _, _ = S.trace_closest(rays)
    r = R.renderer_for_scene(sc, (64, 48))
    assert _check_traversal_tree(r, same_as_karras_allowed=True) == n_tris
    tuv, ids = r.query_closest(rays)
    assert np.array_equal(ids, rids) and np.array_equal(tuv.view(np.uint32)[:, :3], rtuv.view(np.uint32)[:, :3])
    assert (ids[:, 0] >= 0).sum() > (20 if shape == "soup" else 0)
    r.prepare_first_frame()                                                               # a second build in the same context: the arena is reused, the scene's data is not uploaded again
    assert _check_traversal_tree(r, same_as_karras_allowed=True) == n_tris
    tuv, ids = r.query_closest(rays)
    assert np.array_equal(ids, rids) and np.array_equal(tuv.view(np.uint32)[:, :3], rtuv.view(np.uint32)[:, :3])
    r.close()


def test_single_triangle_known_answers(R):
    """analytic KAT through the GPU: one triangle, hand-computed t/u/v, edge, parallel, behind, range cases"""
    from araytracingjourney_amd import scenes
    mb = scenes.MeshBuilder()
    mb.add([(0, 0, 2), (1, 0, 2), (0, 1, 2)], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
    sc = scenes.Scene("tri", [mb.finish(scenes.constant_texture((200, 200, 200)))], scenes.cornell().camera, [])
    r = R.renderer_for_scene(sc, (8, 8))
    rays = np.array([
        [0.25, 0.25, 0, 0.001, 0, 0, 1, 100],      # hit: t=2, u=.25, v=.25
        [0.25, 0.25, 0, 0.001, 0, 0, -1, 100],     # behind
        [2.0, 2.0, 0, 0.001, 0, 0, 1, 100],        # outside
        [0.25, 0.25, 0, 0.001, 1, 0, 0, 100],      # parallel
        [0.25, 0.25, 0, 0.001, 0, 0, 1, 1.5],      # tmax too short
        [0.25, 0.25, 0, 2.5, 0, 0, 1, 100],        # tmin beyond
        [0.25, 0.25, 4, 0.001, 0, 0, -1, 100],     # back face: two-sided => hit at t=2
        [0.5, 0.5, 0, 0.001, 0, 0, 1, 100],        # on the hypotenuse: u+v=1 accepted
    ], np.float32)
    tuv, ids = r.query_closest(rays)
    assert ids[:, 0].tolist() == [0, -1, -1, -1, -1, -1, 0, 0]
    assert np.allclose(tuv[0, :3], [2, .25, .25]) and np.allclose(tuv[6, :3], [2, .25, .25]) and np.allclose(tuv[7, :3], [2, .5, .5])
    assert r.query_any(rays).tolist() == [1, 0, 0, 0, 0, 0, 1, 1]
    r.close()


@pytest.mark.parametrize("n_tris", [1, 2, 3, 5])
def test_tiny_scenes_on_every_builder(R, orc, n_tris):
    """one to five triangles (the tree builders' smallest inputs: no internal node, one, two ...): frame and ray queries against the oracle on the
    default device SAH, the host SAH and the LBVH topology"""
    from araytracingjourney_amd import scenes
    mb = scenes.MeshBuilder()
    for k in range(n_tris):
        z = 1.5 + 0.4 * k
        mb.add([(-0.6 + 0.2 * k, -0.5, z), (0.7, -0.4 + 0.1 * k, z + 0.1), (0.0, 0.6, z)], [(0, 0), (1, 0), (0, 1)], [(0, 0, -1)] * 3, [(1, 0, 0, 1)] * 3, [0, 1, 2])
    sc = scenes.Scene("tiny", [mb.finish(scenes.constant_texture((200, 180, 160)))], scenes.cornell().camera, scenes.cornell().lights)
    S, L, nl = oracle_for(orc, sc)
    ref = S.render(oracle_camera(orc, sc, 96, 64), L, nl, 96, 64, threads=2, debug=True)
    rays = random_rays(4000, 11)
    rtuv, rids, _, _ = S.trace_closest(rays)
    for kw in ({}, {"tuning": {"tree_builder": 1}}, {"fast_build": True}):
        r = R.renderer_for_scene(sc, (96, 64), keep_debug=True, **kw)
        r.render_frame()
        assert np.array_equal(r.read_hits()[1], ref["hit_id"]) and np.array_equal(r.read_shadow_bits(), ref["shadow_bits"]), kw
        assert_radiance_close(r.read_color(), ref["color"])
        tuv, ids = r.query_closest(rays)
        assert np.array_equal(ids, rids) and np.array_equal(tuv.view(np.uint32)[:, :3], rtuv.view(np.uint32)[:, :3]), kw
        assert r.stats()["num_triangles"] == n_tris
        r.close()
    assert (ref["hit_id"][..., 0] >= 0).sum() > 100


def test_largest_frames_keep_the_size_independent_properties(R, get_scene):
    """8192 x 4608 (37.7 M pixels, 2 304 x the Cornell fixture; the oracle would need minutes): what must hold whatever the size -- the fused frame
    equals the staged per-ray frame bit for bit (colour, depth, normal, ray counts), a second trace of the same frame is the same frame, every pixel is
    written (alpha 1, depth either a hit or the miss value), the eight-way shard sum of ray counts is the whole frame's"""
    sc = get_scene("sponza_like", 0.12)
    w, h = 8192, 4608
    fused = R.renderer_for_scene(sc, (w, h), n_lights=1, frames_in_flight=2)
    fused.render_frame()
    c1, d1, n1, st1 = fused.read_color(), fused.read_depth(), fused.read_normal(), fused.stats()
    fused.render_frame()
    assert np.array_equal(fused.read_color().view(np.uint32), c1.view(np.uint32))
    fused.close()
    assert (c1[..., 3] == 1.0).all() and ((d1 < 10000.0) | (d1 == 10000.0)).all() and np.isfinite(c1).all()
    assert st1["primary_rays"] == w * h and st1["hit_pixels"] == int((d1 < 10000.0).sum()) and 0 < st1["shadow_rays"] <= st1["hit_pixels"]
    per_ray = R.renderer_for_scene(sc, (w, h), n_lights=1, tuning={"frame_form": 2})
    per_ray.render_frame()
    assert np.array_equal(per_ray.read_color().view(np.uint32), c1.view(np.uint32)) and np.array_equal(per_ray.read_depth().view(np.uint32), d1.view(np.uint32))
    assert np.array_equal(per_ray.read_normal().view(np.uint32), n1.view(np.uint32))
    st2 = per_ray.stats()
    assert (st2["shadow_rays"], st2["hit_pixels"]) == (st1["shadow_rays"], st1["hit_pixels"])
    per_ray.close()
    del c1, n1
    rays = 0
    for k in range(8):
        s = R.renderer_for_scene(sc, (w, h), n_lights=1, shard=(k, 8))
        s.render_frame()
        rays += s.stats()["shadow_rays"]
        s.close()
    assert rays == st1["shadow_rays"]


def test_api_state_and_argument_errors(R, get_scene):
    """the reference panics on misuse (unwrap/expect); the C ABI returns ART_E_* with a message"""
    from araytracingjourney_amd import _lib
    import ctypes as C
    sc = get_scene("cornell")
    r = R.Renderer((64, 64))
    with pytest.raises(_lib.ArtError) as e:
        r.prepare_first_frame()                       # no primitives
    assert e.value.code == _lib.ART_E_STATE
    r.add_model(sc.primitives)
    with pytest.raises(_lib.ArtError) as e:
        r.trace()                                     # scene not built
    assert e.value.code == _lib.ART_E_STATE
    r.prepare_first_frame()
    with pytest.raises(_lib.ArtError) as e:
        r.trace()                                     # no camera yet
    assert e.value.code == _lib.ART_E_STATE and "camera" in str(e.value)
    with pytest.raises(_lib.ArtError):
        r.read_color()                                # nothing traced
    with pytest.raises(_lib.ArtError):
        r.trace_ao(16)                                # AO before a frame
    r.upload_state()                                  # zero lights: every hit pixel is black, misses too
    r.trace()
    c = r.read_color()
    assert np.array_equal(c[..., :3], np.zeros_like(c[..., :3])) and (c[..., 3] == 1).all() and r.stats()["shadow_rays"] == 0
    with pytest.raises(_lib.ArtError) as e:
        r.resize((0, 10))
    assert e.value.code == _lib.ART_E_INVALID
    with pytest.raises(_lib.ArtError):
        r.trace_ao(65)                                # spp out of range
    n = C.c_uint32()
    assert r._L.art_get_wide_nodes(r._ctx, None, None, 0, None) == _lib.ART_E_INVALID                          # nowhere to put the count
    small = np.zeros((1, 16), np.uint32)
    assert r._L.art_get_wide_nodes(r._ctx, small.ctypes.data, None, 1, C.byref(n)) == _lib.ART_E_INVALID and n.value > 1   # buffer too small: the count is still reported
    p = sc.primitives[0]
    bad = p.indices.copy(); bad[0] = p.verts.shape[0]  # index out of range is rejected on the host, never reaches a kernel
    tiny = R.Renderer((8, 8))
    with pytest.raises(_lib.ArtError) as e:
        tiny.add_model([type(p)(p.verts, bad, p.tex, p.model)])
    tiny.close()
    assert "index out of range" in str(e.value)
    cfg = _lib.ArtConfig(device=99, width=8, height=8)
    ctx = C.c_void_p()
    assert _lib.load().art_create(C.byref(cfg), C.byref(ctx)) == _lib.ART_E_INVALID
    r.close()


@pytest.mark.parametrize("form", ["fused", "fused-binary", "per-ray-3", "per-ray"])
def test_non_finite_cameras_are_errors_and_non_finite_rays_are_misses(R, orc, get_scene, form):
    """A camera looking along the up axis has no side vector (look_at_rh's cross product is zero): an error, like a NaN anywhere in a raw block.
    A finite block can still make non-finite rays (a projection inverse of zeros normalises the zero vector): such a ray accepts no triangle in
    the oracle (every Moeller-Trumbore comparison with NaN is false) and passes every box (fminf / fmaxf drop a NaN operand) -- the walks switch
    its lane off and the frame is the oracle's: all misses.  (Until round 3 the 4-wide packet walk followed the reference of an absent child.)"""
    from araytracingjourney_amd import _lib
    import ctypes as C
    import math
    sc = get_scene("cornell")
    w = h = 64
    fif, tuning = FORMS[form]
    r = R.renderer_for_scene(sc, (w, h), keep_debug=True, frames_in_flight=fif, tuning=tuning)
    for d in ((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 0.0)):
        blk = _lib.ArtCamera()
        rc = r._L.art_camera_from_params((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(*d), 1.0, math.pi / 2, 0.1, 1000.0, C.byref(blk))
        assert rc == _lib.ART_E_INVALID, d
    good = r.camera_mut().update_host_buffer()
    bad = _lib.ArtCamera.from_buffer_copy(bytes(good))
    bad.view_inv[5] = float("nan")
    assert r._L.art_set_camera(r._ctx, C.byref(bad)) == _lib.ART_E_INVALID
    bad = _lib.ArtCamera.from_buffer_copy(bytes(good))
    bad.camera_pos[1] = float("inf")
    assert r._L.art_set_camera(r._ctx, C.byref(bad)) == _lib.ART_E_INVALID
    r.render_frame()
    assert r.stats()["hit_pixels"] > 1000                                        # the good camera sees the box
    zero = _lib.ArtCamera.from_buffer_copy(bytes(good))
    for i in range(16):
        zero.proj_inv[i] = 0.0                                                   # finite, and every ray direction is normalize(0) = NaN
    assert r._L.art_set_camera(r._ctx, C.byref(zero)) == 0
    arr, n = r.lights_mut().copy_lights_shader_data()
    assert r._L.art_set_lights(r._ctx, arr, n) == 0
    r.trace(); r.sync()
    S, L, nl = oracle_for(orc, sc)
    ref = S.render(orc.OrcCamera.from_buffer_copy(bytes(zero)), L, nl, w, h, threads=2, debug=True)
    assert ref["stats"]["hit_pixels"] == 0 and (ref["hit_id"] == -1).all()
    _, ids = r.read_hits()
    assert np.array_equal(ids, ref["hit_id"])
    st = r.stats()
    assert st["hit_pixels"] == 0 and st["shadow_rays"] == 0
    assert np.array_equal(r.read_color(), ref["color"]) and np.array_equal(r.read_depth(), ref["depth"]) and np.array_equal(r.read_normal(), ref["normal"])
    # ray queries: NaN / infinite origins, directions and ranges are misses, in both per-ray walks
    rays = random_rays(64, 3)
    rays[0::4, 4] = np.nan; rays[1::4, 1] = np.inf; rays[2::4, 7] = np.nan
    tuv, qids = r.query_closest(rays)
    rtuv, rids, _, _ = S.trace_closest(rays)
    assert np.array_equal(qids, rids) and (qids[0::4] == -1).all() and (qids[1::4] == -1).all() and (qids[2::4] == -1).all() and (qids[3::4, 0] >= 0).any()
    assert np.array_equal(r.query_any(rays), S.trace_any(rays)[0])
    r.close()


@pytest.mark.parametrize("form", ["fused", "per-ray"])
def test_texture_seams_match_the_oracle(R, orc, scenes, form):
    """bilinear REPEAT where the 2x2 footprint wraps (uv below 0, at 1, past 1) on a 4 x 5 texture of unrelated texels -- the scene tests/test_oracle.py holds against numpy in
    fp64: depth and normal bit for bit (the normal map goes through the sampler), radiance 1e-4"""
    from helpers import seam_scene
    sc = seam_scene(scenes)
    ref = _frame_parity(R, orc, sc, 96, 96, None, form=form)
    fif, tuning = FORMS[form]
    r = R.renderer_for_scene(sc, (96, 96), frames_in_flight=fif, tuning=tuning)
    r.render_frame()
    assert np.array_equal(r.read_depth().view(np.uint32), ref["depth"].view(np.uint32)) and np.array_equal(r.read_normal().view(np.uint32), ref["normal"].view(np.uint32))
    assert ref["stats"]["hit_pixels"] > 3000
    r.close()


def test_sixteen_lights_and_light_updates(R, orc, get_scene, scenes):
    """sixteen lights -- what the kernel arguments carry -- a light change between frames (VkLights dirty flag, vk_lights.rs:81-139), and the list's upper bound (1024)"""
    import math
    sc = get_scene("cornell")
    lights = [dict(kind="point", pos=(0.3 * math.cos(k), 0.3, 0.3 * math.sin(k)), color=(0.5 + 0.1 * k, 0.6, 0.9 - 0.05 * k), falloff=3.0, casts_shadows=(k % 3 != 0))
              for k in range(16)]
    sc16 = scenes.Scene(sc.name, sc.primitives, sc.camera, lights)
    ref = _frame_parity(R, orc, sc16, 96, 64, None)
    assert ref["stats"]["shadow_rays"] > 96 * 64 * 5
    r = R.renderer_for_scene(sc, (96, 64))
    r.render_frame()
    a = r.read_color()
    r.lights_mut().get_point_lights_mut()[0].color = (0.0, 4.0, 0.0)
    r.render_frame()
    b = r.read_color()
    assert not np.array_equal(a, b) and b[..., 0].max() == 0 and b[..., 2].max() == 0 and b[..., 1].max() > 0
    with pytest.raises(Exception):
        for k in range(1025):
            r.lights_mut().get_point_lights_mut().append(R.PointLight((0, 0.5, 0), (1, 1, 1), 3.0, False))
        r.upload_state()
    r.close()


@pytest.mark.parametrize("form", ["fused", "fused-binary", "per-ray-3", "per-ray"])
def test_degenerate_geometry_resolves_as_the_oracle_does(R, orc, get_scene, scenes, form):
    """what a driver's traversal leaves undefined and DESIGN.md 1.1 defines: two IDENTICAL triangles (the hit goes to the lower global id), coplanar overlapping
    triangles, zero-area triangles (three collinear points, three equal points: never hit), a sliver a fraction of a pixel wide, and a fan whose shared vertex and
    edges lie under pixel centres -- hit ids, t, u, v and shadow bits bit-equal to the oracle's in every form of the frame and on every tree"""
    import numpy as np
    sc = get_scene("cornell")
    mb = scenes.MeshBuilder()
    n, t = (0.0, 0.0, -1.0), (1.0, 0.0, 0.0, 1.0)
    def tri(a, b, c):
        mb.add([a, b, c], [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], [n] * 3, [t] * 3, [0, 1, 2])
    z = 0.2
    tri((-0.5, -0.3, z), (0.1, -0.3, z), (-0.5, 0.4, z)); tri((-0.5, -0.3, z), (0.1, -0.3, z), (-0.5, 0.4, z))   # the same triangle twice
    tri((-0.3, -0.2, z), (0.4, -0.2, z), (-0.3, 0.5, z))                                                        # coplanar with them, overlapping
    tri((0.2, 0.1, 0.1), (0.3, 0.2, 0.1), (0.4, 0.3, 0.1)); tri((0.2, -0.2, 0.1), (0.2, -0.2, 0.1), (0.2, -0.2, 0.1))   # zero area: a line, a point
    tri((-0.6, 0.5, 0.0), (0.6, 0.5004, 0.0), (0.6, 0.5, 0.0))                                                  # a sliver
    c = (0.0, 0.0, 0.05)                                                                                         # a fan round the view axis: its centre and spokes under pixel centres
    ring = [(0.3 * np.cos(a), 0.3 * np.sin(a), 0.05) for a in np.linspace(0.0, 2.0 * np.pi, 9)[:-1]]
    for k in range(8):
        tri(c, ring[k], ring[(k + 1) % 8])
    extra = mb.finish(scenes.constant_texture((180, 180, 60)))
    lights = [dict(kind="point", pos=(0.0, 0.3, -0.3), color=(6.0, 6.0, 6.0), falloff=3.0, casts_shadows=True),
              dict(kind="directional", dir=(0.2, -0.4, 1.0), color=(1.0, 1.0, 1.0), casts_shadows=True)]
    ref = _frame_parity(R, orc, scenes.Scene("cornell+degenerate", list(sc.primitives) + [extra], sc.camera, lights), 129, 97, None, form=form)   # odd extent: a pixel centre on the view axis
    ids = ref["hit_id"]
    on_extra = ids[..., 0] == len(sc.primitives)
    assert on_extra.sum() > 500
    tris_hit = set(np.unique(ids[on_extra][:, 1]).tolist())
    assert 0 in tris_hit and 1 not in tris_hit           # of the two identical triangles only the first is ever the hit
    assert 3 not in tris_hit and 4 not in tris_hit       # zero-area triangles are never hit
    assert tris_hit & set(range(6, 14))                  # the fan is


@pytest.mark.parametrize("form", ["fused", "fused-binary", "per-ray-3", "per-ray"])
def test_directional_lights_along_the_axes_and_unnormalised(R, orc, get_scene, scenes, form):
    """a directional light's L, |nn_L| and the shadow ray's reciprocal direction are made on the host, once (art_api.hip directional_constants), with the
    operations the oracle runs per pixel: axis-aligned directions (zero components: the reciprocal's safe_dir branch, signed zeros), an unnormalised and a
    tiny one, in every form of the frame -- hits, shadow bits and ray counts bit-equal to the oracle's, radiance within 1e-4"""
    sc = get_scene("cornell")
    lights = [dict(kind="point", pos=(0.1, 0.3, 0.2), color=(3.0, 3.0, 3.0), falloff=3.0, casts_shadows=True),   # (the light table lists point lights first: lights.rs)
              dict(kind="directional", dir=(0.0, -1.0, 0.0), color=(2.0, 2.0, 2.0), casts_shadows=True),
              dict(kind="directional", dir=(-1.0, 0.0, 0.0), color=(0.5, 1.0, 0.5), casts_shadows=True),
              dict(kind="directional", dir=(0.0, 0.0, 1.0), color=(1.0, 0.5, 0.5), casts_shadows=True),
              dict(kind="directional", dir=(-3.0, -7.0, 2.0), color=(0.7, 0.7, 1.5), casts_shadows=True),
              dict(kind="directional", dir=(1e-12, -2e-12, -1e-12), color=(0.4, 0.4, 0.4), casts_shadows=True)]
    ref = _frame_parity(R, orc, scenes.Scene(sc.name, sc.primitives, sc.camera, lights), 128, 96, None, form=form)
    assert ref["stats"]["shadow_rays"] > 128 * 96 * 2


def test_lights_change_every_frame_while_sixteen_frames_are_in_flight(R, orc, get_scene, scenes):
    """a light animated every frame with 16 frames in flight (a double-buffered device table was overwritten while launches queued
    frames ago still read it): the light records travel by value with each launch, so every frame shows ITS lights -- each one against the oracle"""
    from helpers import device_to_host
    import math
    sc = get_scene("sponza_like", 0.12)
    w, h, F = 960, 540, 16
    r = R.renderer_for_scene(sc, (w, h), n_lights=0, frames_in_flight=F)
    r.lights_mut().get_point_lights_mut().append(R.PointLight((0.0, 1.0, 0.0), (8.0, 8.0, 8.0), 3.0, True))
    r.lights_mut().get_directional_lights_mut().append(R.DirectionalLight((-0.3, -1.0, -0.2), (3.0, 3.0, 3.0), True))
    r.render_frame()                                        # buffers allocated, wave plan sampled
    ptrs, lights = [], []
    for i in range(F):                                      # F frames back to back, no host sync: the earlier ones are still queued or running
        pl = r.lights_mut().get_point_lights_mut()[0]
        pl.pos = (0.5 * math.cos(0.7 * i), 0.6 + 0.05 * i, 0.5 * math.sin(0.7 * i))
        pl.color = (2.0 + i, 9.0 - 0.5 * i, 1.0 + 0.3 * i)
        lights.append([dict(kind="point", pos=pl.pos, color=pl.color, falloff=3.0, casts_shadows=True),
                       dict(kind="directional", dir=(-0.3, -1.0, -0.2), color=(3.0, 3.0, 3.0), casts_shadows=True)])
        r.upload_state()
        r.trace()
        ptrs.append(r.device_color())
    r.sync()
    assert len({p for p, _ in ptrs}) == F                   # every frame of the trip has its own slot
    S = orc.Scene(sc.primitives, morton_bits=30)
    cam = oracle_camera(orc, sc, w, h)
    frames = [device_to_host(p, n).view(np.float32).reshape(h, w, 4) for p, n in ptrs]
    assert not np.array_equal(frames[0], frames[F - 1])
    for i in range(F):
        ref = S.render(cam, orc.make_lights(lights[i]), 2, w, h, threads=8)
        assert_radiance_close(frames[i], ref["color"], what=f"frame {i}")
    r.close()


@pytest.mark.parametrize("form", ["fused", "per-ray"])
def test_forty_lights_some_changing_every_frame(R, orc, get_scene, scenes, form):
    """The reference's light list is a Vec behind an SSBO of n x 80 bytes that the shader loops over (lights.rs:4-67, vk_lights.rs:89-91, raytrace.rgen.glsl:150); libart carries
    the first 16 records in the kernel arguments and the rest in a table of the frame's ring slot (rounds 1-3 refused more than 16).  Forty lights of all four kinds, two of them
    -- record 1 and record 29 -- changing every frame with four frames in flight: every frame shows ITS lights against the oracle (depth and normal bit-equal, radiance 1e-4),
    and the shadow rays counted are the oracle's"""
    from helpers import device_to_host
    import math
    sc = get_scene("sponza_like", 0.12)
    w, h, F = 480, 270, 4
    fif, tuning = (F, None) if form == "fused" else (1, {"frame_form": 2})
    base = []
    for i in range(40):
        a = 2.0 * math.pi * i / 40.0
        if i % 4 == 0: base.append(dict(kind="point", pos=(0.9 * math.cos(a), 0.3 + 0.02 * i, 0.5 * math.sin(a)), color=(0.6 + 0.05 * i, 0.9, 0.4 + 0.03 * i), falloff=2.5, casts_shadows=True))
        elif i % 4 == 1: base.append(dict(kind="spot", pos=(0.7 * math.cos(a), 1.0, 0.4 * math.sin(a)), dir=(-0.3 * math.cos(a), -1.0, -0.3 * math.sin(a)), color=(1.5, 1.2, 0.5 + 0.04 * i), falloff=4.0, penumbra=0.3, umbra=0.6, casts_shadows=i % 8 == 1))
        elif i % 4 == 2: base.append(dict(kind="directional", dir=(-0.3 + 0.02 * i, -1.0, -0.2), color=(0.15, 0.12 + 0.004 * i, 0.1), casts_shadows=True))
        else: base.append(dict(kind="area", pos=(0.3 * math.cos(a), 1.2, 0.3 * math.sin(a)), pos2=(0.3 * math.cos(a) + 0.2, 1.2, 0.3 * math.sin(a)), pos3=(0.3 * math.cos(a) + 0.2, 1.2, 0.3 * math.sin(a) + 0.2), invert_normal=True, color=(0.8, 0.8, 1.0), falloff=3.0, penumbra=0.5, umbra=1.2, casts_shadows=True))
    def lights_of(frame):   # in the order lights travel in: points, spots, directionals, areas (lights.rs:24-47)
        L = [dict(d) for kind in ("point", "spot", "directional", "area") for d in base if d["kind"] == kind]
        assert L[1]["kind"] == "point" and L[29]["kind"] == "directional"
        L[1]["pos"] = (0.9 * math.cos(0.5 * frame), 0.4, 0.3 * math.sin(0.5 * frame))
        L[29]["dir"] = (0.4 - 0.2 * frame, -1.0, 0.1 * frame)
        return L
    def push(r, L):
        lm = r.lights_mut()
        for lst in (lm.get_point_lights_mut(), lm.get_spot_lights_mut(), lm.get_directional_lights_mut(), lm.get_area_lights_mut()):
            del lst[:]
        for d in L:
            lm.push_dict(d)
    r = R.renderer_for_scene(sc, (w, h), n_lights=0, frames_in_flight=fif, tuning=tuning)
    push(r, lights_of(0)); r.render_frame()                 # buffers allocated (40 lights), wave plan sampled
    S = orc.Scene(sc.primitives, morton_bits=30)
    cam = oracle_camera(orc, sc, w, h)
    ptrs = []
    for f in range(F):
        push(r, lights_of(f + 1)); r.upload_state(); r.trace()
        if fif == 1:
            r.sync()
            ref = S.render(cam, orc.make_lights(lights_of(f + 1)), 40, w, h, threads=8)
            assert r.stats()["shadow_rays"] == ref["stats"]["shadow_rays"], f
            assert np.array_equal(r.read_depth().view(np.uint32), ref["depth"].view(np.uint32)), f
            assert_radiance_close(r.read_color(), ref["color"], what=f"per-ray frame {f}, 40 lights")
        else:
            ptrs.append((r.device_color(), r._dev("depth"), r._dev("normal")))   # back to back, no host sync: each slot's table travels on its own stream
    r.sync()
    if fif > 1:
        assert len({t[0][0] for t in ptrs}) == F               # every frame of the trip has its own slot
        last = None
        for f, t in enumerate(ptrs):
            col, dep, nor = (device_to_host(p, n) for p, n in t)
            ref = S.render(cam, orc.make_lights(lights_of(f + 1)), 40, w, h, threads=8)
            assert np.array_equal(dep.view(np.uint32).reshape(h, w), ref["depth"].view(np.uint32)), f
            assert np.array_equal(nor.view(np.uint32).reshape(h, w, 4)[..., :3], ref["normal"].view(np.uint32)[..., :3]), f
            assert_radiance_close(col.view(np.float32).reshape(h, w, 4), ref["color"], what=f"frame {f} of 40 lights")
            last = ref
        assert r.stats()["shadow_rays"] == last["stats"]["shadow_rays"]   # (the latest frame's)
    r.close()


def _pose(base, i, warp=False):
    """frame i's object -> world matrix of the moving model: its base matrix, rotated about y and z and carried along a small loop (float32 3x4, row-major);
    warp: also mirrored, scaled differently along each axis and sheared (a negative determinant, an inverse-transpose that is not the matrix)"""
    import math
    a, b = 0.21 * i, 0.13 * i
    ry = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]])
    rz = np.array([[math.cos(b), -math.sin(b), 0, 0], [math.sin(b), math.cos(b), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    t = np.eye(4); t[:3, 3] = (0.25 * math.sin(0.4 * i), 0.05 * i, 0.2 * math.cos(0.3 * i) - 0.2)
    w = np.array([[-0.8, 0.15, 0, 0], [0, 1.3, 0, 0], [0.1, 0, 0.6, 0], [0, 0, 0, 1]]) if warp else np.eye(4)
    m = t @ ry @ rz @ w @ np.vstack([np.asarray(base, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    return np.ascontiguousarray(m[:3], np.float32)


def _moving_scene(R, scenes, sc, movers, extent, lights, **kw):
    """the scene as two models: the primitives in `movers` (one model that will move) and the rest"""
    r = R.Renderer(extent, **kw)
    static = [p for j, p in enumerate(sc.primitives) if j not in movers]
    moving = [sc.primitives[j] for j in movers]
    r.add_model(static)
    r.add_model(moving)
    cam = r.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    for d in lights:
        r.lights_mut().push_dict(d)
    r.prepare_first_frame()
    return r, static, moving


def _oracle_of_moved(orc, scenes, static, moving, m):
    P = type(moving[0])
    return orc.Scene(static + [P(p.verts, p.indices, p.tex, m) for p in moving], morton_bits=30)   # built from scratch where the model is now


@pytest.mark.parametrize("versions", [3, 1, 8])
def test_a_model_moves_every_frame_with_sixteen_frames_in_flight(R, orc, get_scene, scenes, versions):
    """Row a3 (VkModel::set_model_matrix vk_model.rs:461-466 + the per-frame TLAS of renderer.rs:637-651): one model is moved and rotated before every
    frame, 16 frames are launched back to back without a host sync, and EVERY frame is the oracle's frame of a scene built from scratch where the model
    is in that frame -- depth and normal bit for bit (the geometry outputs), radiance within 1e-4.  libart refits (triangle records and every box above
    them, topology kept) into a ring of `versions` copies of the structure: frames in flight keep the scene they were launched with."""
    from helpers import device_to_host
    sc = get_scene("sponza_like", 0.12)
    w, h, F = 320, 180, 16
    lights = scenes.sponza_lights(4)
    movers = [len(sc.primitives) - 1, len(sc.primitives) - 2]          # two primitives of one model (displaced spheres)
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, frames_in_flight=F, tuning={"as_versions": versions, "refit_rebuild_ratio": -1.0})
    model = r.models_mut()[1]
    base = moving[0].model
    r.render_frame()                                                    # buffers allocated, wave plan sampled
    ptrs, poses = [], []
    for i in range(F):
        m = _pose(base, i + 1)
        model.set_model_matrix(m)
        poses.append(m)
        r.upload_state(); r.trace()
        ptrs.append((r.device_color(), r._dev("depth"), r._dev("normal")))
    r.sync()
    st = r.stats()
    assert st["refits"] == F and st["rebuilds"] == 0 and st["refit_ms"] > 0
    cam = oracle_camera(orc, sc, w, h)
    L = orc.make_lights(lights)
    shown = 0
    for i in range(F):
        ref = _oracle_of_moved(orc, scenes, static, moving, poses[i]).render(cam, L, len(lights), w, h, threads=8, debug=True)
        (pc, nc), (pd, nd), (pn, nn) = ptrs[i]
        color = device_to_host(pc, nc).view(np.float32).reshape(h, w, 4)
        depth = device_to_host(pd, nd).view(np.float32).reshape(h, w)
        normal = device_to_host(pn, nn).view(np.float32).reshape(h, w, 4)
        assert np.array_equal(depth.view(np.uint32), ref["depth"].view(np.uint32)), f"frame {i}: depth"
        assert np.array_equal(normal.view(np.uint32), ref["normal"].view(np.uint32)), f"frame {i}: normal"
        assert_radiance_close(color, ref["color"], what=f"frame {i}")
        shown += int((ref["hit_id"][..., 0] >= len(static)).sum())
    assert shown > 2000                                                  # the model that moves is in view
    r.close()


@pytest.mark.parametrize("dynamic", [False, True], ids=["versions-at-first-move", "versions-at-build"])
def test_a_small_tree_is_all_crown_and_moves_all_the_same(R, orc, get_scene, scenes, dynamic):
    """the Cornell box (34 triangles: a tree of a dozen nodes, smaller than one batch of the refit -- everything is the crown's one workgroup) with its last primitive moving
    before every frame, four frames in flight: every frame is the oracle's frame of a scene built from scratch; and ART_FLAG_DYNAMIC_SCENE makes the ring of versions in
    art_scene_build (first_move_ms 0, versions_ms > 0) where a scene that did not announce it pays in front of its first moved frame"""
    from helpers import device_to_host
    sc = get_scene("cornell")
    w, h, F = 160, 160, 4
    movers = [len(sc.primitives) - 1]
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), sc.lights, frames_in_flight=F, dynamic_scene=dynamic)
    model = r.models_mut()[1]
    base = moving[0].model
    r.render_frame()
    st0 = r.stats()
    assert (st0["versions_ms"] > 0) == dynamic and st0["first_move_ms"] == 0
    ptrs, poses = [], []
    for i in range(F):
        m = _pose(base, i + 1)
        m[:, 3] = np.asarray(base, np.float32).reshape(3, 4)[:, 3] + np.float32(0.02 * (i + 1)) * np.array([1.0, 0.5, -1.0], np.float32)   # (small steps: the box stays inside the room)
        model.set_model_matrix(m); poses.append(m.copy())
        r.upload_state(); r.trace()
        ptrs.append((r.device_color(), r._dev("depth"), r._dev("normal")))
    r.sync()
    st = r.stats()
    assert st["refits"] == F and (st["first_move_ms"] == 0) == dynamic and st["versions_ms"] > 0
    cam = oracle_camera(orc, sc, w, h)
    L = orc.make_lights(sc.lights)
    for i in range(F):
        ref = _oracle_of_moved(orc, scenes, static, moving, poses[i]).render(cam, L, len(sc.lights), w, h, threads=4, debug=True)
        (pc, nc), (pd, nd), (pn, nn) = ptrs[i]
        assert np.array_equal(device_to_host(pd, nd).view(np.uint32).reshape(h, w), ref["depth"].view(np.uint32)), f"frame {i}: depth"
        assert np.array_equal(device_to_host(pn, nn).view(np.uint32).reshape(h, w, 4), ref["normal"].view(np.uint32)), f"frame {i}: normal"
        assert_radiance_close(device_to_host(pc, nc).view(np.float32).reshape(h, w, 4), ref["color"], what=f"frame {i}")
    r.close()


@pytest.mark.parametrize("F,K", [(1, 4), (2, 4), (4, 4), (8, 0), (3, 24)], ids=["1-slot-4-versions", "2-slots-4-versions", "4-slots-4-versions", "8-slots-default-16-versions", "3-slots-24-versions"])
def test_moving_frames_lap_the_ring_of_versions_without_a_sync(R, orc, get_scene, scenes, F, K):
    """advisor, round 3: no test reused a ring slot or a version without a host sync in between.  F x 4 + 3 moving frames launched back to back through F ring slots and a
    ring of K versions (every version is rewritten F times or more, its staging memory with it; the refits run on streams of their own beside the frames): the LAST F frames
    -- the ones whose outputs still exist -- are the oracle's frames of scenes built from scratch, depth and normal bit for bit.  K = 0: the default, twice the ring of
    frames (round 4d); 24: the most art_set_tuning takes"""
    from helpers import device_to_host
    sc = get_scene("sponza_like", 0.12)
    w, h = 320, 180
    lights = scenes.sponza_lights(1)
    movers = [len(sc.primitives) - 1, len(sc.primitives) - 2]
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, frames_in_flight=F, tuning={"as_versions": K, "refit_rebuild_ratio": -1.0})
    K = K or max(2 * F, 4)
    model = r.models_mut()[1]
    base = moving[0].model
    r.render_frame()
    n = F * K + 3
    ptrs, poses = [], []
    for i in range(n):
        m = _pose(base, i + 1)
        model.set_model_matrix(m)
        poses.append(m)
        r.upload_state(); r.trace()
        ptrs.append((r.device_color(), r._dev("depth"), r._dev("normal")))
    r.sync()
    assert r.stats()["refits"] == n
    cam = oracle_camera(orc, sc, w, h)
    L = orc.make_lights(lights)
    for i in range(n - F, n):
        ref = _oracle_of_moved(orc, scenes, static, moving, poses[i]).render(cam, L, len(lights), w, h, threads=8, debug=True)
        (pc, nc), (pd, nd), (pn, nn) = ptrs[i]
        assert np.array_equal(device_to_host(pd, nd).view(np.uint32).reshape(h, w), ref["depth"].view(np.uint32)), f"frame {i}: depth"
        assert np.array_equal(device_to_host(pn, nn).view(np.uint32).reshape(h, w, 4), ref["normal"].view(np.uint32)), f"frame {i}: normal"
        assert_radiance_close(device_to_host(pc, nc).view(np.float32).reshape(h, w, 4), ref["color"], what=f"frame {i}")
    r.close()


def test_a_small_model_moves_among_batches_that_stay(R, orc, get_scene, scenes):
    """round 4g / 4h: a refit launches only the batches of subtrees that hold a primitive that moved, and a large tree makes its quantised records and its cost in the
    refit's own workgroups with every batch's share of the cost cached per version (ArtTuning.refit_fold_nodes = 1: that form on this small tree; 0: the launch of its
    own behind the crown).  One 3 920-triangle primitive of a 66 k-triangle scene moves through eight poses and back to where it was built, two versions, so every
    version is rewritten four times -- the first time all batches run, afterwards the few that hold the mover: every frame is the oracle's frame of a scene built
    from scratch (depth, normal bit for bit), AO walks the refitted quantised records, and the two forms report the same cost, equal to the build's once the model is back"""
    sc = get_scene("sponza_like", 0.5)
    w, h = 256, 144
    lights = scenes.sponza_lights(1)
    movers = [6]
    cam = oracle_camera(orc, sc, w, h)
    L = orc.make_lights(lights)
    poses, refs = [], []
    ratios = {}
    for fold in (1, 0):
        r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, frames_in_flight=1, tuning={"as_versions": 2, "refit_rebuild_ratio": -1.0, "refit_fold_nodes": fold})
        model = r.models_mut()[1]
        base = moving[0].model
        if not poses:
            poses = [_pose(base, i) for i in range(1, 8)] + [np.ascontiguousarray(np.asarray(base, np.float32).reshape(3, 4))]
            refs = [_oracle_of_moved(orc, scenes, static, moving, m) for m in poses]
        r.render_frame()
        ratios[fold] = []
        for m, S in zip(poses, refs):
            model.set_model_matrix(m)
            r.render_frame()
            ref = S.render(cam, L, len(lights), w, h, threads=8, debug=True)
            assert np.array_equal(r.read_depth().view(np.uint32), ref["depth"].view(np.uint32))
            assert np.array_equal(r.read_normal().view(np.uint32), ref["normal"].view(np.uint32))
            assert_radiance_close(r.read_color(), ref["color"])
            r.sync()
            ratios[fold].append(r.stats()["refit_cost_ratio"])
        r.trace_ao(8)
        want_ao, _ = orc.render_ao(refs[-1], cam, ref["depth"], ref["normal"], 8, 0.2 * 1.457, threads=8)
        assert np.array_equal(r.read_ao(), want_ao)
        st = r.stats()
        assert st["refits"] == len(poses) and st["rebuilds"] == 0
        r.close()
    # (the cost a frame reports is that of the latest refit whose result has arrived: each frame above was waited for, so it is its own)
    assert np.allclose(ratios[1], ratios[0], rtol=1e-9), (ratios[1], ratios[0])
    assert abs(ratios[1][-1] - 1.0) < 1e-6 and max(ratios[1]) > 1.0005, ratios[1]     # back where it was built: the build's cost again; in between the tree was looser


@pytest.mark.parametrize("config", ["c2", "c4"])
def test_a_moved_model_at_the_bench_scenes_full_size(R, orc, get_scene, scenes, config):
    """row a3 at the sizes BASELINE names: config 2 (262 816 triangles; the model that moves is its u32-index primitive, 164 k triangles) and config 4 (2.8 M
    triangles, 63-bit keys) at 1920x1080 -- two poses in a row, each frame against the oracle built from scratch where the model is: hit ids, t, u, v, shadow
    bits, ray counts bit for bit, radiance within 1e-4; and ray-traced AO in the refitted structure (16 samples on config 2, 4 on config 4)"""
    sc = get_scene("sponza_like" if config == "c2" else "bistro_like", 1.0)
    lights = scenes.sponza_lights(1) if config == "c2" else sc.lights
    w, h = 1920, 1080
    movers = [len(sc.primitives) - 1]
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, keep_debug=True, frames_in_flight=3, morton_bits=63 if config == "c4" else 0)
    model = r.models_mut()[1]
    cam = oracle_camera(orc, sc, w, h)
    L = orc.make_lights(lights)
    r.render_frame()
    for i in (2, 5):
        m = _pose(moving[0].model, i)
        model.set_model_matrix(m)
        r.render_frame()
        S = _oracle_of_moved(orc, scenes, static, moving, m)
        ref = S.render(cam, L, len(lights), w, h, threads=8, debug=True)
        tuv, ids = r.read_hits()
        assert np.array_equal(ids, ref["hit_id"]), f"{int((ids != ref['hit_id']).any(-1).sum())} hit ids differ"
        assert np.array_equal(tuv.view(np.uint32)[..., :3], ref["hit_tuv"].view(np.uint32)[..., :3])
        assert np.array_equal(r.read_shadow_bits(), ref["shadow_bits"])
        st = r.stats()
        assert st["shadow_rays"] == ref["stats"]["shadow_rays"] and st["hit_pixels"] == ref["stats"]["hit_pixels"] and st["rebuilds"] == 0
        assert_radiance_close(r.read_color(), ref["color"])
    assert r.stats()["refits"] == 2 and 0 < r.stats()["refit_ms"] < 2.0                    # (the review's bar: a refresh within 2 ms on config 2)
    # ray-traced AO in the refitted structure: the per-ray walk over the QUANTISED records the refit made (for config 4's 1.4 M nodes inside the refit's own workgroups since
    # round 4g, for config 2 in the launch behind them) -- and the cost that travelled to the host with them
    spp = 16 if config == "c2" else 4
    r.trace_ao(spp)
    want_ao, _ = orc.render_ao(S, cam, ref["depth"], ref["normal"], spp, 0.2 * 1.457, threads=8)
    assert np.array_equal(r.read_ao(), want_ao)
    assert 0.95 < r.stats()["refit_cost_ratio"] < 2.0
    r.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_edits_of_a_scene_with_frames_in_flight(R, orc, get_scene, scenes, seed):
    """Row a3 under a random schedule: two models move independently (sometimes far enough that the rebuild rule -- ArtTuning.refit_rebuild_ratio --
    fires by itself: it is set to 1.2 here), one of them leaves and re-enters the structure (vk_model.rs:360-372; masked and restored by the refit, built again only when a build left it out), the camera moves; frames are launched in bursts of 1..4
    without a host sync in between, three versions of the structure behind four ring slots.  Every frame of every burst is the oracle's frame of a scene
    built from scratch in the state that frame was launched in: depth and normal bit for bit, radiance within 1e-4."""
    from araytracingjourney_amd._lib import check
    from helpers import device_to_host
    sc = get_scene("sponza_like", 0.12)
    w, h, F = 192, 108, 4
    lights = scenes.sponza_lights(4)
    n = len(sc.primitives)
    groups = {"static": list(range(n - 4)), "a": [n - 1], "b": [n - 3, n - 2]}        # b last but one in id order: its absence shifts nobody's ids but a's, which no output shows
    r = R.Renderer((w, h), frames_in_flight=F, tuning={"as_versions": 3, "refit_rebuild_ratio": 1.2})
    for g in ("static", "b", "a"):
        r.add_model([sc.primitives[j] for j in groups[g]])
    model_b, model_a = r.models_mut()[1], r.models_mut()[2]
    cam = r.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    for d in lights:
        r.lights_mut().push_dict(d)
    r.prepare_first_frame()
    r.render_frame()
    rng = np.random.default_rng(seed)
    base = {"a": sc.primitives[n - 1].model, "b": sc.primitives[n - 2].model}
    state = {"a": np.array(base["a"], np.float32).reshape(3, 4), "b": np.array(base["b"], np.float32).reshape(3, 4), "b_in": True, "pos": tuple(sc.camera["pos"])}
    P = type(sc.primitives[0])
    L = orc.make_lights(lights)
    frames = 0
    for burst in range(14):
        launched = []
        for _ in range(int(rng.integers(1, F + 1))):
            op = int(rng.integers(0, 7))
            if op in (0, 2):
                state["a"] = _pose(base["a"], int(rng.integers(1, 40)), warp=bool(rng.integers(0, 4) == 0)); model_a.set_model_matrix(state["a"])
            if op in (1, 2):
                state["b"] = _pose(base["b"], int(rng.integers(1, 40))); model_b.set_model_matrix(state["b"])   # (while b is out: takes effect with the build that brings it back)
            if op == 3:                                                                                         # far away: the tree inflates, a later move builds again
                far = _pose(base["a"], int(rng.integers(1, 40))); far[:, 3] += np.array([0.0, 7.0, 3.0], np.float32)
                state["a"] = far; model_a.set_model_matrix(far)
            if op == 4:
                state["b_in"] = not state["b_in"]
                for pid in model_b.primitive_ids:
                    check(r._L.art_scene_set_primitive_enabled(r._ctx, pid, 1 if state["b_in"] else 0))
                if r.needs_build():                                                                             # (only after the cost rule built again while b was out)
                    check(r._L.art_scene_build(r._ctx))
            if op == 5:
                p0 = sc.camera["pos"]; state["pos"] = (p0[0] + float(rng.uniform(-1, 1)), p0[1] + float(rng.uniform(-0.3, 0.3)), p0[2] + float(rng.uniform(-0.5, 0.5)))
                cam.set_pos(state["pos"])
            r.upload_state(); r.trace()                                                                         # op 6: nothing changed
            launched.append(((r.device_color(), r._dev("depth"), r._dev("normal")), dict(state)))
        r.sync()
        for ptrs, st in launched:
            prims = [sc.primitives[j] for j in groups["static"]]
            if st["b_in"]:
                prims += [P(sc.primitives[j].verts, sc.primitives[j].indices, sc.primitives[j].tex, st["b"]) for j in groups["b"]]
            prims += [P(sc.primitives[j].verts, sc.primitives[j].indices, sc.primitives[j].tex, st["a"]) for j in groups["a"]]
            c = sc.camera
            ocam = orc.camera_from_params(st["pos"], c["dir"], w / h, c["fovy"], c["znear"], c["zfar"])
            ref = orc.Scene(prims, morton_bits=30).render(ocam, L, len(lights), w, h, threads=8, debug=True)
            (pc, nc), (pd, nd), (pn, nn) = ptrs
            depth = device_to_host(pd, nd).view(np.float32).reshape(h, w)
            normal = device_to_host(pn, nn).view(np.float32).reshape(h, w, 4)
            color = device_to_host(pc, nc).view(np.float32).reshape(h, w, 4)
            what = f"seed {seed}, burst {burst}, frame {frames}"
            assert np.array_equal(depth.view(np.uint32), ref["depth"].view(np.uint32)), what + ": depth"
            assert np.array_equal(normal.view(np.uint32), ref["normal"].view(np.uint32)), what + ": normal"
            assert_radiance_close(color, ref["color"], what=what)
            frames += 1
    st = r.stats()
    print("random edits, seed", seed, ":", frames, "frames,", st["refits"], "refits,", st["rebuilds"], "rebuilds by the cost rule")
    assert st["refits"] > 0 and frames >= 14
    r.close()


@pytest.mark.parametrize("form", ["fused", "fused-binary", "per-ray"])
def test_a_model_leaves_and_re_enters_the_structure_without_a_build(R, orc, get_scene, scenes, form):
    """Residency (vk_model.rs:334-345 / :360-372, renderer.rs:637-651) on a built scene: a model that was part of the build is taken out and brought back by
    art_scene_set_primitive_enabled WITHOUT art_scene_build -- the next frame's refit writes its triangles nowhere (or back) and shrinks (or grows) the boxes
    above them.  Frames, ray queries, AO and the trees read back are those of a scene built without / with the model: hit ids, t, u, v, shadow bits bit for bit.
    It moves while it is out; a model the build never saw still needs the build."""
    from araytracingjourney_amd._lib import check
    sc = get_scene("sponza_like", 0.12)
    w, h = 240, 136
    lights = scenes.sponza_lights(4)
    fif, tuning = FORMS[form]
    n = len(sc.primitives)
    movers = [n - 1, n - 8]                                              # the displaced sphere and a column
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, keep_debug=True, frames_in_flight=fif, tuning=dict(tuning, refit_rebuild_ratio=-1.0))
    model = r.models_mut()[1]
    cam = oracle_camera(orc, sc, w, h)
    L = orc.make_lights(lights)
    r.render_frame()
    P = type(moving[0])

    def enable(on):
        for pid in model.primitive_ids:
            check(r._L.art_scene_set_primitive_enabled(r._ctx, pid, 1 if on else 0))
        assert not r.needs_build()

    def compare(S, what):
        ref = S.render(cam, L, len(lights), w, h, threads=8, debug=True)
        tuv, ids = r.read_hits()
        assert np.array_equal(ids, ref["hit_id"]), f"{what}: {int((ids != ref['hit_id']).any(-1).sum())} hit ids differ"
        assert np.array_equal(tuv.view(np.uint32)[..., :3], ref["hit_tuv"].view(np.uint32)[..., :3]), what
        assert np.array_equal(r.read_shadow_bits(), ref["shadow_bits"]), what
        st = r.stats()
        assert st["shadow_rays"] == ref["stats"]["shadow_rays"] and st["hit_pixels"] == ref["stats"]["hit_pixels"] and st["num_triangles"] == S.n_tris, what
        assert_radiance_close(r.read_color(), ref["color"], what=what)
        r.trace_ao(8)
        want_ao, _ = orc.render_ao(S, cam, ref["depth"], ref["normal"], 8, 0.2 * 1.457, threads=8)
        assert np.array_equal(r.read_ao(), want_ao), what
        rays = random_rays(20000, 5)
        qt, qi = r.query_closest(rays)
        rt, ri, _, _ = S.trace_closest(rays)
        assert np.array_equal(qi, ri) and np.array_equal(qt.view(np.uint32)[:, :3], rt.view(np.uint32)[:, :3]), what   # (the static primitives come first: the same ids with and without the model)
        short = rays.copy(); short[:, 7] = 1.5
        assert np.array_equal(r.query_any(short), S.trace_any(short)[0]), what

    without = orc.Scene(static, morton_bits=30)
    enable(False); r.render_frame()
    tuv, ids = r.read_hits()
    ref = without.render(cam, L, len(lights), w, h, threads=8, debug=True)
    assert np.array_equal(ids, ref["hit_id"]) and np.array_equal(r.read_shadow_bits(), ref["shadow_bits"])      # static primitives come first: same ids
    compare(without, "model out")
    m = _pose(moving[0].model, 5)
    model.set_model_matrix(m)                                            # moved while it is out: nothing to see ...
    r.render_frame()
    assert np.array_equal(r.read_hits()[1], ref["hit_id"])
    enable(True); r.render_frame()                                       # ... until it is back, where it was moved to
    compare(_oracle_of_moved(orc, scenes, static, moving, m), "model back")
    enable(False); enable(True); r.render_frame()                        # out and in between two frames: nothing changes
    compare(_oracle_of_moved(orc, scenes, static, moving, m), "out and in")
    st = r.stats()
    assert st["rebuilds"] == 0 and st["refits"] >= 3
    # the trees read back with the model out: every node box the exact union of what is left below it, nothing of the model in any box
    enable(False); r.render_frame()
    f = r.get_wide_nodes()[1].view(np.float32).reshape(-1, 32)
    root = f[0, :24].reshape(4, 6)
    root = root[root[:, 0] < 3.0e38]
    lb = without.lbvh()
    assert np.array_equal(root[:, :3].min(0), lb["leaf_lo"].min(0)) and np.array_equal(root[:, 3:].max(0), lb["leaf_hi"].max(0))
    # a model the build has never seen needs the build
    extra = r.add_model([P(moving[0].verts, moving[0].indices, moving[0].tex, _pose(moving[0].model, 9))])
    assert r.needs_build()
    r.close()


@pytest.mark.parametrize("form", ["fused", "fused-binary", "per-ray-3", "per-ray"])
def test_a_moved_model_in_every_form_of_the_frame(R, orc, get_scene, scenes, form):
    """after art_scene_set_model_matrix every form of the frame -- the binary node records and the per-ray walks follow the refit on demand -- gives the oracle's
    frame of the moved scene: hit ids, t, u, v and shadow bits bit for bit; so do ray queries, ray-traced AO, and the trees read back through the parity
    surface are trees of exact boxes over the moved triangles"""
    sc = get_scene("sponza_like", 0.12)
    w, h = 240, 136
    lights = scenes.sponza_lights(4)
    fif, tuning = FORMS[form]
    movers = [len(sc.primitives) - 1]
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, keep_debug=True, frames_in_flight=fif, tuning=dict(tuning, refit_rebuild_ratio=-1.0))
    model = r.models_mut()[1]
    cam = oracle_camera(orc, sc, w, h)
    L = orc.make_lights(lights)
    r.render_frame()
    for i in (3, 7, 9):
        m = _pose(moving[0].model, i, warp=i == 9)                       # the last one mirrored, anisotropic and sheared: normals go by the inverse transpose
        model.set_model_matrix(m)
        r.render_frame()
        S = _oracle_of_moved(orc, scenes, static, moving, m)
        ref = S.render(cam, L, len(lights), w, h, threads=8, debug=True)
        tuv, ids = r.read_hits()
        assert np.array_equal(ids, ref["hit_id"]), f"{int((ids != ref['hit_id']).any(-1).sum())} hit ids differ"
        assert np.array_equal(tuv.view(np.uint32)[..., :3], ref["hit_tuv"].view(np.uint32)[..., :3])
        assert np.array_equal(r.read_shadow_bits(), ref["shadow_bits"])
        st = r.stats()
        assert st["shadow_rays"] == ref["stats"]["shadow_rays"] and st["hit_pixels"] == ref["stats"]["hit_pixels"]
        assert_radiance_close(r.read_color(), ref["color"])
        assert np.array_equal(r.read_depth().view(np.uint32), ref["depth"].view(np.uint32))
        r.trace_ao(8)                                                    # AO in the structure the frame was traced in
        want_ao, _ = orc.render_ao(S, cam, ref["depth"], ref["normal"], 8, 0.2 * 1.457, threads=8)
        assert np.array_equal(r.read_ao(), want_ao)
    model.set_model_matrix(_pose(moving[0].model, 11))                   # no frame in between: the queries refit first
    S = _oracle_of_moved(orc, scenes, static, moving, model.model_matrix)
    rays = random_rays(20000, 11)
    tuv, ids = r.query_closest(rays)
    rtuv, rids, _, _ = S.trace_closest(rays)
    assert np.array_equal(ids, rids) and np.array_equal(tuv.view(np.uint32)[:, :3], rtuv.view(np.uint32)[:, :3])
    short = rays.copy(); short[:, 7] = 1.5
    assert np.array_equal(r.query_any(short), S.trace_any(short)[0])
    # the parity surface after a move: leaf boxes = the moved triangles' boxes, every node box the exact union of its children's
    lb, tr = r.get_lbvh(), r.get_traversal_tree()
    ref_lb = S.lbvh()
    by_gid = np.empty_like(ref_lb["leaf_lo"]); by_gid[ref_lb["leaf_gid"]] = ref_lb["leaf_lo"]
    assert np.array_equal(lb["leaf_lo"].view(np.uint32), by_gid[lb["leaf_gid"]].view(np.uint32))   # same world-space triangles as a fresh build (leaf order: the original build's)
    for tree, child in ((lb, lb["child"]), (tr, tr["child"])):
        def box(ref, lo_or_hi):
            return np.where((ref < 0)[:, None], lb["leaf_" + lo_or_hi][np.where(ref < 0, ~ref, 0)], tree["node_" + lo_or_hi][np.where(ref >= 0, ref, 0)])
        assert np.array_equal(tree["node_lo"], np.minimum(box(child[:, 0], "lo"), box(child[:, 1], "lo")))
        assert np.array_equal(tree["node_hi"], np.maximum(box(child[:, 0], "hi"), box(child[:, 1], "hi")))
    r.close()


def test_refit_writes_the_bits_of_the_build_and_rebuilds_past_the_cost_threshold(R, orc, get_scene, scenes):
    """a model moved away and back: the refitted triangle records and 4-wide nodes are, bit for bit, the arrays of the build (the refit repeats the build's
    arithmetic); a move that inflates the tree past ArtTuning.refit_rebuild_ratio makes art_trace build again -- and the frame is still the oracle's"""
    sc = get_scene("sponza_like", 0.12)
    w, h = 160, 90
    lights = scenes.sponza_lights(1)
    movers = [len(sc.primitives) - 1]
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, tuning={"refit_rebuild_ratio": -1.0})
    model = r.models_mut()[1]
    q0, f0 = r.get_wide_nodes()
    r.render_frame()
    c0 = r.read_color()
    model.set_model_matrix(moving[0].model)                              # where it already is: nothing to do
    r.render_frame()
    assert r.stats()["refits"] == 0
    model.set_model_matrix(_pose(moving[0].model, 2)); r.render_frame()
    q1, f1 = r.get_wide_nodes()
    assert not np.array_equal(f0, f1) and np.array_equal(f0[:, 24:], f1[:, 24:])        # boxes moved, the topology did not
    model.set_model_matrix(moving[0].model); r.render_frame()
    st = r.stats()
    assert st["refits"] == 2 and st["rebuilds"] == 0 and abs(st["refit_cost_ratio"] - 1.0) < 0.2
    q2, f2 = r.get_wide_nodes()
    assert np.array_equal(q0, q2) and np.array_equal(f0, f2)
    assert np.array_equal(r.read_color().view(np.uint32), c0.view(np.uint32))
    r.close()
    r, static, moving = _moving_scene(R, scenes, sc, movers, (w, h), lights, tuning={"refit_rebuild_ratio": 1.05})
    model = r.models_mut()[1]
    r.render_frame()
    far = np.array(moving[0].model, np.float32).reshape(3, 4).copy(); far[1, 3] += 6.0   # six units up: every box above it inflates
    model.set_model_matrix(far); r.render_frame(); r.sync()
    assert r.stats()["refit_cost_ratio"] > 1.05                          # measured on that refit ...
    model.set_model_matrix(_pose(far, 1)); r.render_frame()              # ... so the next move builds instead
    st = r.stats()
    assert st["rebuilds"] == 1 and st["refit_cost_ratio"] == 1.0
    S = _oracle_of_moved(orc, scenes, static, moving, model.model_matrix)
    ref = S.render(oracle_camera(orc, sc, w, h), orc.make_lights(lights), 1, w, h, threads=8)
    assert_radiance_close(r.read_color(), ref["color"])
    assert np.array_equal(r.read_depth().view(np.uint32), ref["depth"].view(np.uint32))
    r.close()


def test_packing_and_tonemap_match_oracle(R, orc, get_scene):
    """art_present: the reference's storage formats (bit-exact integer packing) and tonemap.comp.glsl's output (BGRA8, <= 1 LSB)"""
    sc = get_scene("sponza_like", 0.12)
    w, h = 480, 270
    r = R.renderer_for_scene(sc, (w, h))
    r.render_frame(sync=False)
    r.trace_ao(16)
    r.present()
    color, normal, depth, ao = r.read_color(), r.read_normal(), r.read_depth(), r.read_ao()
    pc, pn, pd = r.read_packed()
    want_pc, want_bgra = orc.present(color, ao)
    assert np.array_equal(pc, want_pc)
    assert np.array_equal(pn, orc.present(normal)[0])
    with np.errstate(over="ignore"):
        assert np.array_equal(pd, depth.astype(np.float16).view(np.uint16))      # R16_SFLOAT; the 10000 of misses is representable
    got = r.read_present()
    diff = np.abs(got.astype(int) - want_bgra.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.01 and (got[..., 3] == 255).all()
    assert got[..., :3].max() > 100 and (got[..., :3].reshape(-1, 3).max(1) == 0).mean() > 0.01   # lit and unlit pixels both present
    r.render_frame(sync=False)                                                     # no AO for this frame: ao = 255
    r.present()
    assert np.abs(r.read_present().astype(int) - orc.present(r.read_color())[1].astype(int)).max() <= 1
    unpresented = R.renderer_for_scene(sc, (32, 32))
    with pytest.raises(Exception):
        unpresented.read_present()
    unpresented.close()
    r.close()
