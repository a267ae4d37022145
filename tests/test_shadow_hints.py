"""Shadow-occluder hints (ArtTuning.shadow_hints, art_read_shadow_hints / art_write_shadow_hints): the any-hit packet walks of the fused frame first test
the triangles that occluded their 8x8 block a frame ago.  An any-hit answer is "some triangle accepts the ray", whatever the order, so the feature may not move one bit:
every comparison here is np.array_equal on colour, depth, normal and the shadow bits."""
import os
import sys
import threading

import numpy as np
import pytest

from helpers import oracle_camera, oracle_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = {"shadow_hints": 1}
EMPTY = 0xFFFFFFFF


@pytest.fixture(scope="module")
def R():
    from araytracingjourney_amd import renderer
    return renderer


def _outputs(r):
    r.sync()
    return {"color": r.read_color(), "depth": r.read_depth(), "normal": r.read_normal(), "shadow_bits": r.read_shadow_bits()}


def _assert_equal(a, b, what):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {k} differs ({int((x != y).sum())} values)"


def _card(scenes, p0, du, dv, alpha):
    """a quad whose albedo layer carries `alpha` (an alpha-masked primitive once it has a cutoff)"""
    th, tw = alpha.shape
    t = np.zeros((3, th, tw, 4), np.uint8)
    t[0, ..., :3] = (180, 150, 120); t[0, ..., 3] = alpha
    t[1] = (255, 160, 0, 255); t[2] = (128, 128, 255, 255)
    mb = scenes.MeshBuilder()
    scenes.quad(mb, p0, du, dv, 2, 2, (1.0, 1.0))
    return mb.finish(t)


def _checker():
    a = np.zeros((8, 8), np.uint8)
    a[::2, ::2] = 255; a[1::2, 1::2] = 255
    return a


def _four_lights(sc, scenes):
    if sc.name.startswith("cornell"):
        return list(sc.lights) + [dict(kind="point", pos=p, color=(4.0, 4.0, 4.0), falloff=3.0, casts_shadows=True) for p in ((0.3, 0.2, 0.3), (-0.3, 0.1, 0.2), (0.0, -0.2, 0.4))]
    return scenes.sponza_lights(4)


def _scene(scenes, get_scene, name, n_lights, alpha):
    sc = get_scene("cornell") if name == "cornell" else get_scene("sponza_like", 0.12)
    prims = list(sc.primitives)
    if alpha:   # a checkered card high in the scene, between the lights and the floor
        prims.append(_card(scenes, (-0.35, 0.3, -0.35), (0.7, 0.0, 0.0), (0.0, 0.0, 0.7), _checker()) if name == "cornell"
                     else _card(scenes, (-0.4, 0.55, -0.3), (0.8, 0.0, 0.0), (0.0, 0.0, 0.6), _checker()))
    return scenes.Scene(sc.name + ("+card" if alpha else ""), prims, sc.camera, sc.lights if n_lights == 1 else _four_lights(sc, scenes))


def _renderer(R, sc, extent, tuning, alpha=False, **kw):
    r = R.renderer_for_scene(sc, extent, keep_debug=True, tuning=tuning, **kw)
    if alpha:
        r.models_mut()[0].set_alpha_cutoff(len(sc.primitives) - 1, 0.5)
    r.upload_state()
    return r


def _n_leaves(r):
    return r.stats()["num_triangles"]


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("n_lights", [1, 4])
@pytest.mark.parametrize("wide", [0, 2], ids=["wide", "binary"])
@pytest.mark.parametrize("name", ["sponza_like", "cornell"])
def test_hints_on_cold_and_warm_equal_hints_off_and_the_oracles_bits(R, orc, scenes, get_scene, name, wide, n_lights, alpha):
    """every form of the fused frame that walks packets (4-wide / binary nodes, one / four lights, with / without an alpha-masked primitive, then two frames per launch):
    hints off, hints on as the first frame after the build (cold) and as the fifth (warm) give the same colour, depth, normal and shadow bits, and the bits are the oracle's
    (without the card: the oracle has no alpha)"""
    sc = _scene(scenes, get_scene, name, n_lights, alpha)
    w, h = (160, 96) if name == "sponza_like" else (96, 64)
    off = _renderer(R, sc, (w, h), dict(OFF, packet_wide=wide), alpha)
    off.trace()
    want = _outputs(off)
    on = _renderer(R, sc, (w, h), dict(packet_wide=wide), alpha)
    on.trace()
    _assert_equal(_outputs(on), want, "cold")
    for _ in range(4):
        on.trace()
    _assert_equal(_outputs(on), want, "warm")
    assert (off.read_shadow_hints() == EMPTY).all()   # off: the table is never written
    if not (alpha and n_lights == 4):                 # (the plain multi-light instance with the alpha test is compiled without hints: kFrameHints, art_frame.hip)
        assert (on.read_shadow_hints() != EMPTY).any()
    if not alpha:
        S, L, nl = oracle_for(orc, sc)
        ref = S.render(oracle_camera(orc, sc, w, h), L, nl, w, h, threads=8, debug=True)
        assert np.array_equal(want["shadow_bits"], ref["shadow_bits"])
    for r, what in ((off, "off, two frames per launch"), (on, "warm, two frames per launch")):
        r.set_frames_per_launch(2)
        r.set_camera_batch([r.camera_mut(), r.camera_mut()])
        r.trace(); r.trace()
        for b in (0, 1):
            r.set_read_frame(b)
            got = _outputs(r)
            del got["shadow_bits"]   # (read-backs of frame b: colour, depth, normal)
            _assert_equal(got, {k: want[k] for k in got}, f"{what}, frame {b}")
    on.close(); off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 2], ids=["wide", "binary"])
def test_a_poisoned_table_changes_nothing(R, scenes, get_scene, wide):
    """the table filled with (a) random valid leaf positions, (b) positions >= the leaf count and 0x7FFFFFFF, (c) the leaf positions of a primitive that is then disabled:
    each time the next frame equals the hints-off frame"""
    sc = _scene(scenes, get_scene, "sponza_like", 4, False)
    w, h = 160, 96
    off = _renderer(R, sc, (w, h), dict(OFF, packet_wide=wide))
    off.trace()
    want = _outputs(off)
    on = _renderer(R, sc, (w, h), dict(packet_wide=wide))
    on.trace()
    T, shape = _n_leaves(on), on.read_shadow_hints().shape
    rng = np.random.default_rng(11)
    on.write_shadow_hints(rng.integers(0, T, shape, dtype=np.uint32))
    assert (on.read_shadow_hints() < T).all()
    on.trace()
    _assert_equal(_outputs(on), want, "(a) random valid positions")
    bad = rng.integers(T, 2 ** 32 - 1, shape, dtype=np.uint64).astype(np.uint32)
    bad[::2] = 0x7FFFFFFF
    bad[1::7, :, 1] = rng.integers(0, T, bad[1::7, :, 1].shape, dtype=np.uint32)   # (and a valid word among them here and there)
    on.write_shadow_hints(bad)
    on.trace()
    _assert_equal(_outputs(on), want, "(b) positions past the leaves")
    # (c) the biggest primitive's leaves everywhere, then the primitive disabled: its records are points nowhere in the next frame's triangles
    p = int(np.argmax([q.n_tris for q in sc.primitives]))
    first = int(sum(q.n_tris for q in sc.primitives[:p]))
    gid = on.get_lbvh()["leaf_gid"]
    pos = np.nonzero((gid >= first) & (gid < first + sc.primitives[p].n_tris))[0].astype(np.uint32)
    assert pos.size == sc.primitives[p].n_tris
    on.write_shadow_hints(rng.choice(pos, shape))
    for r in (on, off):
        assert r._L.art_scene_set_primitive_enabled(r._ctx, r.models_mut()[0].primitive_ids[p], 0) == 0
        r.trace()
    gone = _outputs(off)
    assert not np.array_equal(gone["depth"], want["depth"])
    _assert_equal(_outputs(on), gone, "(c) the leaves of a disabled primitive")
    on.close(); off.close()


def _two_model_renderer(R, sc, extent, lights, tuning, **kw):
    r = R.Renderer(extent, keep_debug=True, tuning=tuning, **kw)
    r.add_model(sc.primitives[:-1]); r.add_model(sc.primitives[-1:])
    cam = r.camera_mut()
    cam.set_pos(sc.camera["pos"]); cam.set_dir(sc.camera["dir"]); cam.set_fovy(sc.camera["fovy"]); cam.set_znear(sc.camera["znear"]); cam.set_zfar(sc.camera["zfar"])
    for d in lights:
        r.lights_mut().push_dict(d)
    r.prepare_first_frame(); r.upload_state()
    return r


@pytest.mark.gpu
def test_a_model_moves_and_a_mesh_deforms_with_eight_frames_in_flight(R, scenes, get_scene):
    """a model moved and a mesh deformed before every frame, 8 frames in flight, hints warm: every fourth frame equals the same frame of a context with hints off"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import _pose
    sc = get_scene("sponza_like", 0.12)
    w, h, F = 160, 96, 8
    lights = scenes.sponza_lights(4)
    tune = {"refit_rebuild_ratio": -1.0}
    on, off = _two_model_renderer(R, sc, (w, h), lights, tune, frames_in_flight=F), _two_model_renderer(R, sc, (w, h), lights, dict(tune, **OFF))
    base, verts0 = sc.primitives[-1].model, np.asarray(sc.primitives[-2].verts, np.float32).reshape(-1, 12)
    for _ in range(F):
        on.trace()   # warm
    for i in range(1, 25):
        m = _pose(base, i)
        v = verts0.copy()
        v[:, 1] += 0.02 * np.sin(7.0 * v[:, 0] + 0.5 * i)
        for r in ((on, off) if i % 4 == 0 else (on,)):
            r.models_mut()[1].set_model_matrix(m)
            r.models_mut()[0].set_vertices(len(sc.primitives) - 2, v)
        on.trace()
        if i % 4 == 0:
            off.trace()
            _assert_equal(_outputs(on), _outputs(off), f"frame {i}")
    assert on.stats()["refits"] == 24 and (on.read_shadow_hints() != EMPTY).any()
    on.close(); off.close()


@pytest.mark.gpu
def test_a_rebuild_empties_the_table(R, scenes, get_scene):
    """art_scene_build -- by hand, and the one art_trace starts once the refitted tree's cost passes a tiny refit_rebuild_ratio -- leaves every entry empty: after the
    call itself, and after the automatic one in the blocks that trace no shadow ray (their entries are never written, so a marker put there survives anything but the clear)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import _pose
    sc = get_scene("sponza_like", 0.12)
    w, h = 160, 96
    r = _two_model_renderer(R, sc, (w, h), sc.lights, {"refit_rebuild_ratio": 1e-6})
    for _ in range(3):
        r.trace()
    assert (r.read_shadow_hints() != EMPTY).any()
    assert r._L.art_scene_build(r._ctx) == 0
    assert (r.read_shadow_hints() == EMPTY).all()
    r.trace(); r.sync()
    bits = r.read_shadow_bits()
    blocks = _block_view(bits, w, h)
    quiet = np.nonzero((blocks >> 16).max(axis=1) == 0)[0]   # blocks that trace no shadow ray
    assert quiet.size
    t = r.read_shadow_hints()
    assert (t[quiet] == EMPTY).all()
    t[quiet] = 5
    r.write_shadow_hints(t)
    before = r.stats()["rebuilds"]
    for i in (1, 2, 3):
        r.models_mut()[1].set_model_matrix(_pose(sc.primitives[-1].model, i))
        r.trace(); r.sync()
    assert r.stats()["rebuilds"] > before
    still = np.nonzero((_block_view(r.read_shadow_bits(), w, h) >> 16).max(axis=1) == 0)[0]
    still = np.intersect1d(still, quiet)
    assert still.size and (r.read_shadow_hints()[still] == EMPTY).all()
    r.close()


def _block_view(img, w, h):
    """[h, w] per-pixel words -> [8x8 blocks of the context's local pixels, 64] in the table's block order (one context owns every 32x32 tile, row-major; a tile's sixteen
    blocks row-major inside it); pixels outside the frame read 0"""
    tx, ty = (w + 31) // 32, (h + 31) // 32
    pad = np.zeros((ty * 32, tx * 32), img.dtype)
    pad[:h, :w] = img
    return pad.reshape(ty, 4, 8, tx, 4, 8).transpose(0, 3, 1, 4, 2, 5).reshape(ty * tx * 16, 64)


@pytest.mark.gpu
def test_the_table_holds_an_occluder_of_a_fully_shadowed_block(R, scenes, get_scene):
    """after five frames of a still camera some block whose pixels are all shadowed has a valid leaf position in its entry (structural: no timing)"""
    sc = get_scene("sponza_like", 0.12)
    w, h = 640, 360   # (8x8 blocks small enough on the screen for some to lie wholly in shadow)
    r = _renderer(R, sc, (w, h), {})
    for _ in range(5):
        r.trace()
    r.sync()
    blocks = _block_view(r.read_shadow_bits(), w, h)
    dark = np.nonzero(((blocks & 1) == 1).all(axis=1))[0]   # light 0 shadowed in every pixel of the block
    assert dark.size, "no fully shadowed block in this view"
    t = r.read_shadow_hints()
    assert (t[dark, 0] < _n_leaves(r)).any(axis=1).any()
    r.close()


@pytest.mark.gpu
def test_a_two_rank_job_with_hints_assembles_the_hints_off_frame(R, scenes, get_scene):
    """two ranks (threads of this process, one shard context each) over the host-exchange hook, hints on and warm: rank 0 assembles the frame of one context with hints off"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    sc = get_scene("sponza_like", 0.12)
    w, h, world, launches = 160, 96, 2, 6
    whole = _renderer(R, sc, (w, h), OFF)
    whole.trace()
    want = whole.read_color()
    meet, parts, errors, frames = threading.Barrier(world, timeout=120), {}, [], {}

    def rank_main(rank):
        try:
            r = R.renderer_for_scene(sc, (w, h), shard=(rank, world), frames_in_flight=2)
            r.upload_state()

            def gather(send, nbytes, recv, root, stream):
                host = np.empty(nbytes, np.uint8)
                assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), send, nbytes, 2) == 0
                parts[rank] = host
                meet.wait()
                if rank == root:
                    for k in range(world):
                        assert hip.hipMemcpy(recv + k * nbytes, parts[k].ctypes.data_as(C.c_void_p), nbytes, 1) == 0
                meet.wait()
            mg = R.MultiGpu(r, rank, world, launches_per_gather=2, exchange=gather)
            for _ in range(launches):
                mg.trace()
            mg.flush()
            if rank == 0:
                frames[0] = mg.read_frame()
            assert (r.read_shadow_hints() != EMPTY).any()
            meet.wait()
            mg.close(); r.close()
        except BaseException as e:   # (a rank that fails must not leave the other one waiting)
            errors.append(e)
            meet.abort()
    threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    assert np.array_equal(frames[0].view(np.uint32), want.view(np.uint32))
    whole.close()
