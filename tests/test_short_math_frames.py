"""Frames through the k_frame instances that take the short exact forms (kFrameShort, art_frame.hip): small one-light frames on the inputs where a form could
go wrong -- a wave-wide fallback, zero direction components, axis-aligned lights, grazing angles, textures of one, two and 3 x 5 texels sampled across their edges and at
negative coordinates, an alpha-masked card.  Every frame must equal, byte for byte, the frame of ArtTuning.plain_math = 1 (the plain expressions in every wave) and the
staged frame (frame_form 2: k_shade and the per-ray walks compile none of the forms -- the signed remainder in both texture wraps, the plain divisions), and where the CPU
oracle can render the scene, its hits and shadow bits to the bit and its radiance within the 1e-4 of every parity test."""
import numpy as np
import pytest

from conftest import assert_radiance_close
from helpers import oracle_camera, oracle_for

KEYS = ("color", "depth", "normal", "shadow_bits")


@pytest.fixture(scope="module")
def R():
    from araytracingjourney_amd import renderer
    return renderer


def _frame(R, sc, extent, tuning, cutoffs=None):
    r = R.renderer_for_scene(sc, extent, keep_debug=True, tuning=tuning)
    for i, c in (cutoffs or {}).items():
        r.models_mut()[0].set_alpha_cutoff(i, c)
    r.upload_state(); r.trace(); r.sync()
    tuv, ids = r.read_hits()
    out = {"color": r.read_color().copy(), "depth": r.read_depth().copy(), "normal": r.read_normal().copy(), "shadow_bits": r.read_shadow_bits().copy(), "tuv": tuv.copy(), "ids": ids.copy()}
    r.close()
    return out


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k} differs in {int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum())} words"


def _check(R, sc, extent, orc=None, cutoffs=None):
    """the default frame against the plain one and the staged one; against the oracle where one is given; -> the default frame"""
    assert len(sc.lights) == 1, "one light: the instances with the guarded fast paths"
    fast = _frame(R, sc, extent, {}, cutoffs)
    _same(fast, _frame(R, sc, extent, {"plain_math": 1}, cutoffs), "default vs plain_math")
    _same(fast, _frame(R, sc, extent, {"frame_form": 2}, cutoffs), "fused vs staged")
    _same(fast, _frame(R, sc, extent, {"packet_wide": 2}, cutoffs), "4-wide vs binary nodes")
    if orc is not None:
        w, h = extent
        S, L, nl = oracle_for(orc, sc)
        ref = S.render(oracle_camera(orc, sc, w, h), L, nl, w, h, threads=8, debug=True)
        assert np.array_equal(fast["ids"], ref["hit_id"]) and np.array_equal(fast["tuv"].view(np.uint32)[..., :3], ref["hit_tuv"].view(np.uint32)[..., :3])
        assert np.array_equal(fast["shadow_bits"], ref["shadow_bits"])
        assert_radiance_close(fast["color"], ref["color"])
        assert_radiance_close(fast["depth"], ref["depth"], what="depth")
        assert_radiance_close(fast["normal"], ref["normal"], rel=1e-4, floor=1e-5, what="normal")
    return fast


def _with(scenes, sc, name, prims=None, camera=None, lights=None):
    return scenes.Scene(sc.name + "+" + name, list(sc.primitives if prims is None else prims), dict(sc.camera, **(camera or {})), list(sc.lights[:1] if lights is None else lights))


@pytest.mark.gpu
def test_a_zeroed_normal_sends_its_waves_through_the_fallback(R, scenes, get_scene):
    """the scene of tests/test_exact_math.py: waves on the zero normal run the surface block again with the plain expressions, NaNs and all"""
    from test_exact_math import _scene_with_a_zero_normal
    sc = _with(scenes, _scene_with_a_zero_normal(scenes, get_scene), "one_light")
    fast = _check(R, sc, (64, 64))
    nan = np.isnan(fast["normal"][..., :3]).any(axis=-1)
    assert nan.any() and (~nan).sum() > nan.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)], ids=["+z", "-z", "+x"])
def test_a_camera_looking_down_an_axis_at_an_odd_extent(R, orc, scenes, get_scene, axis):
    """63 x 63: the centre pixel's fx / W is exactly 0.5, its ray has two zero direction components (safe_dir's 1e-20) and its row and column one"""
    sc = get_scene("cornell")
    pos = (0.0, 0.0, -0.9) if axis[2] > 0 else ((0.0, 0.0, 0.9) if axis[2] < 0 else (-0.9, 0.0, 0.0))
    fast = _check(R, _with(scenes, sc, "axis", camera=dict(pos=pos, dir=axis)), (63, 63), orc)
    assert (fast["ids"][..., 0] >= 0).all(), "inside the room every ray hits"


@pytest.mark.gpu
@pytest.mark.parametrize("d", [(0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)], ids=["-y", "+x", "+z"])
def test_a_directional_light_along_an_axis(R, orc, scenes, get_scene, d):
    sc = get_scene("cornell")
    _check(R, _with(scenes, sc, "dir", lights=[dict(kind="directional", dir=d, color=(3.0, 3.0, 3.0), casts_shadows=True)]), (64, 64), orc)


@pytest.mark.gpu
@pytest.mark.parametrize("light", [
    dict(kind="point", pos=(0.0, 0.95, 0.0), color=(3.0, 3.0, 3.0), falloff=4.0, casts_shadows=True),      # just under the ceiling: grazing NdotL on it, grazing NdotV on the floor's far end
    dict(kind="point", pos=(-0.97, 0.0, 0.0), color=(3.0, 3.0, 3.0), falloff=0.0, casts_shadows=True),     # on a wall
    dict(kind="spot", pos=(0.0, 0.9, 0.0), dir=(0.0, -1.0, 0.0), color=(4.0, 4.0, 4.0), falloff=3.0, penumbra=0.5, umbra=0.8, casts_shadows=True),
], ids=["point_ceiling", "point_wall", "spot"])
def test_point_and_spot_lights_at_grazing_angles(R, orc, scenes, get_scene, light):
    """the shadow ray's direction comes from a guarded normalisation, and the BRDF's three quotients see NdotL and NdotV near 0"""
    sc = get_scene("cornell")
    fast = _check(R, _with(scenes, sc, "light", lights=[light]), (64, 64), orc)
    assert (fast["shadow_bits"] >> 16).any(), "shadow rays were traced"


def _texture(tw, th, seed, alpha=None):
    """3 layers of random texels; the normal map leans on +z so that the surface stays lit"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (3, th, tw, 4)).astype(np.uint8)
    t[0, ..., 3] = 255 if alpha is None else alpha
    t[2, ..., 2] = 255
    t[2, ..., :2] = 96 + t[2, ..., :2] // 4
    return t


def _card(scenes, tex, uv_lo, uv_hi, n=3):
    """a card in front of Cornell's back wall whose texture coordinates run from uv_lo to uv_hi"""
    mb = scenes.MeshBuilder()
    scenes.quad(mb, (-0.6, -0.6, 0.4), (1.2, 0.0, 0.0), (0.0, 1.2, 0.0), n, n, (1.0, 1.0))
    p = mb.finish(tex)
    v = p.verts.copy()
    v[:, 3:5] = np.asarray(uv_lo, np.float32) + v[:, 3:5] * (np.asarray(uv_hi, np.float32) - np.asarray(uv_lo, np.float32))
    return scenes.Primitive(v, p.indices, p.tex, p.model)


@pytest.mark.gpu
@pytest.mark.parametrize("tw,th", [(1, 1), (2, 2), (3, 5)], ids=["1x1", "2x2", "3x5"])
@pytest.mark.parametrize("uv", [((0.0, 0.0), (1.0, 1.0)), ((-1.25, -2.5), (1.75, 0.5)), ((-0.5, 0.5), (0.5, 3.0))], ids=["edges", "negative", "across"])
def test_small_textures_sampled_on_and_across_their_edges(R, orc, scenes, get_scene, tw, th, uv):
    """the second tap's wrap is where x0 + 1 == tw: a 1 x 1 texture wraps every sample, a 3 x 5 one has no power-of-two extent; coordinates on the edges (0 and 1 at
    the card's vertices), below zero and across several repeats"""
    sc = get_scene("cornell")
    card = _card(scenes, _texture(tw, th, 7 * tw + th), *uv)
    fast = _check(R, _with(scenes, sc, f"card{tw}x{th}", prims=list(sc.primitives) + [card]), (64, 64), orc)
    assert (fast["ids"][..., 0] == len(sc.primitives)).sum() > 500, "the card fills a good part of the frame"


@pytest.mark.gpu
@pytest.mark.parametrize("uv", [((0.0, 0.0), (1.0, 1.0)), ((-1.25, -2.5), (1.75, 0.5))], ids=["edges", "negative"])
def test_an_alpha_masked_card_with_a_3x5_texture(R, scenes, get_scene, uv):
    """tex_taps: the alpha test of the packet walks (fused) and of the per-ray walks (staged) and the shading see the same four taps -- the frames are equal, the card is
    cut in places and kept in others"""
    sc = get_scene("cornell")
    alpha = np.array([[0, 255, 0], [255, 0, 255], [40, 200, 90], [255, 255, 0], [0, 130, 255]], np.uint8)
    card = _card(scenes, _texture(3, 5, 11, alpha), *uv)
    full = _with(scenes, sc, "masked", prims=list(sc.primitives) + [card])
    ci = len(sc.primitives)
    fast = _check(R, full, (64, 64), cutoffs={ci: 0.5})
    opaque = _frame(R, full, (64, 64), {})
    on_card = (opaque["ids"][..., 0] == ci)
    kept = (fast["ids"][..., 0] == ci)
    assert on_card.sum() > 500 and 0.1 * on_card.sum() < kept.sum() < 0.9 * on_card.sum() and not (kept & ~on_card).any()


@pytest.mark.gpu
def test_low_detail_sponza_like_at_128x72(R, orc, scenes, get_scene):
    sc = get_scene("sponza_like", 0.12)
    _check(R, _with(scenes, sc, "one_light"), (128, 72), orc)
