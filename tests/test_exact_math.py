"""The shading kernels' fast paths for sqrtf(x) and 1.0f / sqrtf(x) (art_device.h: inv_sqrt_exact / sqrt_exact; art_shade.h: the surface block's guard): a wave
whose inputs all lie inside the guard's range runs the compiler's own core without the range handling around it, any other wave the plain expression.  Both functions are
unary, so "the same bits" is proved, not sampled: art_parity_math_sweep runs all 2^32 inputs through the helper the frame kernels call and through a non-inlined copy of
the plain expression and compares the results as integers."""
import struct

import numpy as np
import pytest

ALL = 1 << 32
FORMS = {0: "inv_sqrt_exact", 1: "sqrt_exact", 2: "surface_block"}


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def ctx():
    from araytracingjourney_amd import renderer
    r = renderer.Renderer((64, 64))
    yield r
    r.close()


def _in_range(lo, hi):
    """patterns inside lo <= x <= hi (positive floats are ordered like their bits), and those of them that lie in a 64-aligned run of patterns wholly inside"""
    lo_b, hi_b = _bits(lo), _bits(hi)
    first, last = -(-lo_b // 64), (hi_b - 63) // 64   # first / last k with 64 k .. 64 k + 63 inside
    return hi_b - lo_b + 1, max(0, last - first + 1) * 64


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(FORMS), ids=[FORMS[k] for k in sorted(FORMS)])
def test_every_input_in_order(ctx, which):
    """all 2^32 patterns, a wave taking 64 consecutive ones: no result differs from the plain expression's, and exactly the waves wholly inside the guard's range took
    the fast path (so the sweep compared the fast path, not the fallback with itself)"""
    got = ctx.math_sweep(which, 0, ALL, 1)
    lo, hi = got["guard"]
    assert 0.0 < lo < 1.0 < hi < float("inf")
    inside, whole_waves = _in_range(lo, hi)
    print(f"\n{FORMS[which]}: guard [{lo!r}, {hi!r}], {inside} patterns inside, {got}")
    assert got["mismatches"] == 0, f"first differing input: {got['first_bad_bits']:#010x}"
    assert got["fast_lanes"] == whole_waves and whole_waves >= inside - 126


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(FORMS), ids=[FORMS[k] for k in sorted(FORMS)])
def test_every_input_in_mixed_waves(ctx, which):
    """the same 2^32 patterns, lane to lane an odd stride apart (a bijection mod 2^32): 3/8 of the patterns are inside the range, so next to no wave has its 64 lanes
    all inside -- the out-of-range lanes pull the in-range lanes of their wave through the fallback, and the results are still the plain expression's"""
    got = ctx.math_sweep(which, 0, ALL, 0x9E3779B1)
    inside, _ = _in_range(*got["guard"])
    print(f"\n{FORMS[which]}, mixed waves: {got}")
    assert got["mismatches"] == 0, f"first differing input: {got['first_bad_bits']:#010x}"
    assert got["fast_lanes"] < inside // 1000


@pytest.mark.gpu
def test_a_partial_sweep_and_bad_arguments(ctx):
    """a count that is no multiple of the wave (the lanes past it sit out), a start inside the range; which above 4 is refused"""
    from araytracingjourney_amd._lib import ArtError
    got = ctx.math_sweep(0, _bits(1.0), 1000, 1)
    assert got["mismatches"] == 0 and got["fast_lanes"] == 1000 and got["first_bad_bits"] is None
    got = ctx.math_sweep(1, _bits(-1.0), 130, 1)   # negatives: NaN from both, the same NaN
    assert got["mismatches"] == 0 and got["fast_lanes"] == 0
    with pytest.raises(ArtError):
        ctx.math_sweep(5)


@pytest.mark.gpu
def test_the_sweep_finds_an_inexact_function(ctx):
    """the sweep's own control: the hardware's 1-ulp v_rsq_f32 in place of the fast path is reported -- mismatches, all of them inside the guard's range (outside it the
    control runs the plain expression too), and the first one by its bit pattern"""
    got = ctx.math_sweep(4, 0, ALL, 1)
    lo, hi = got["guard"]
    inside, _ = _in_range(lo, hi)
    print(f"\nv_rsq_f32 alone: {got}")
    assert 0 < got["mismatches"] < inside
    assert _bits(lo) <= got["first_bad_bits"] <= _bits(hi)
    assert ctx.math_sweep(4, got["first_bad_bits"], 1, 1)["mismatches"] == 1


def _scene_with_a_zero_normal(scenes, get_scene):
    """cornell with the vertex normals of the tall box (the last primitive) zeroed: its pixels normalise a zero vector (NaN normals, as before), the room's pixels unit normals"""
    sc = get_scene("cornell")
    prims = list(sc.primitives)
    last = prims[-1]
    v = last.verts.copy()
    v[:, 5:8] = 0.0
    prims[-1] = scenes.Primitive(v, last.indices, last.tex, last.model)
    return scenes.Scene("cornell+zero_normal", prims, sc.camera, sc.lights)


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [{}, {"packet_wide": 2}, {"frame_form": 2}], ids=["fused", "fused_binary", "staged"])
def test_a_frame_with_a_degenerate_normal_equals_the_plain_frame(scenes, get_scene, tuning):
    """64x64, one light (the instances with the fast paths): waves that see only unit normals take the fast path, waves that touch the zero normal the fallback; colour,
    depth, normal and shadow bits equal the frame of ArtTuning.plain_math = 1 (the plain expressions in every wave) bit for bit, NaNs included"""
    from araytracingjourney_amd import renderer as R
    sc = _scene_with_a_zero_normal(scenes, get_scene)
    frames = []
    for plain in (0, 1):
        r = R.renderer_for_scene(sc, (64, 64), keep_debug=True, tuning=dict(tuning, plain_math=plain))
        r.upload_state(); r.trace(); r.sync()
        frames.append({"color": r.read_color().copy(), "depth": r.read_depth().copy(), "normal": r.read_normal().copy(), "shadow_bits": r.read_shadow_bits().copy()})
        r.close()
    fast, plain = frames
    nan = np.isnan(plain["normal"][..., :3]).any(axis=-1)
    assert nan.any() and (~nan).sum() > nan.sum(), "the scene must show both the zero normal and unit normals"
    for k in fast:
        assert np.array_equal(fast[k].view(np.uint8), plain[k].view(np.uint8)), f"{k} differs in {int((fast[k].view(np.uint32) != plain[k].view(np.uint32)).sum())} words"
