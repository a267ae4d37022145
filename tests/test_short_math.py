"""The short exact forms of the frame kernels' once-per-wave divisions (art_device.h: rcp_core, div_core): the compiler's own chain for a / b -- v_rcp_f32, one
refinement, q = a r, two residual corrections -- without v_div_scale / v_div_fmas / v_div_fixup around it, which do nothing while the operands lie inside the form's domain.
"The same bits" is proved over whole sets, not sampled: art_parity_div_sweep runs the helper the kernels call and a non-inlined copy of the plain division and compares the
results as integers.  A lane outside the domain takes the plain expression in the sweep, so every mismatch counted is one inside the domain."""
import struct

import numpy as np
import pytest

ALL = 1 << 32
PAIR_SET = 254 * 254 * 64
CAM_COLS, CAM_MAX_W = 16384 + 32, 16384   # art_resize's limit; the lanes of a 32-pixel tile past the frame's edge divide too


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _float(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


@pytest.fixture(scope="module")
def ctx():
    from araytracingjourney_amd import renderer
    r = renderer.Renderer((64, 64))
    yield r
    r.close()


def _unary_inside(lo, hi):
    """patterns x with lo <= |safe_dir(x)| <= hi: safe_dir lifts every |x| < 1e-20 (zeros and denormals too) to 1e-20, which is inside; both signs"""
    assert lo <= 1e-20 <= hi
    return 2 * (_bits(hi) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 0x9E3779B1], ids=["in_order", "odd_stride"])
def test_reciprocal_direction_every_input(ctx, stride):
    """rcp_core(safe_dir(x)) against 1.0f / safe_dir(x) over all 2^32 patterns, in order and an odd stride apart (a bijection mod 2^32): 0 mismatches among the lanes that
    take the short form, and exactly the patterns inside the guard's range took it"""
    got = ctx.div_sweep(0, 0, ALL, stride)
    lo, hi = got["guard"]
    inside = _unary_inside(lo, hi)
    print(f"\nrcp_core(safe_dir(x)), stride {stride:#x}: guard [{lo!r}, {hi!r}], {inside} patterns inside, {got}")
    assert 0.0 < lo <= 1e-20 and 2.0 <= hi < float("inf"), "a unit vector's components and safe_dir's floor must lie inside the guard"
    assert got["mismatches"] == 0, f"first differing input: {got['first_bad'][1]:#010x}"
    assert got["lanes"] == ALL and got["short_lanes"] == inside and 0 < inside < ALL


def _numerators():
    """16 numerators: 1, 0.5, the ends of the camera ray's numerator range (x + 0.5 for the first column and for the last lane of the last tile), the ends of the domain,
    all-zeros and all-ones mantissas, seeded random ones inside the domain"""
    rng = np.random.default_rng(20240607)
    fixed = [1.0, 0.5, CAM_COLS - 0.5, 1920 - 0.5, 3840 - 0.5, -1.0]
    pats = [_bits(v) for v in fixed] + [_bits(2.0 ** -47), _bits(2.0 ** 47), 0x3F800000 | 0x7FFFFF, 0x2F000000 | 0x7FFFFF, 0x4F000000]
    while len(pats) < 16:
        pats.append(int(rng.integers(0, 2)) << 31 | int(rng.integers(127 - 46, 127 + 46)) << 23 | int(rng.integers(0, 1 << 23)))
    return pats


@pytest.mark.gpu
@pytest.mark.parametrize("numer", _numerators(), ids=lambda b: f"{b:#010x}")
def test_quotient_every_denominator(ctx, numer):
    """div_core(a, b) against a / b for all 2^32 denominators b: 0 mismatches inside the domain; the set holds denominators on each side of both of the domain's borders"""
    got = ctx.div_sweep(1, 0, ALL, 1, numer)
    lo, hi = got["domain"]
    a = abs(_float(numer))
    assert lo <= a <= hi, "the numerators are chosen inside the domain"
    inside = 2 * (_bits(hi) - _bits(lo) + 1)   # both signs of every |b| in [lo, hi]
    print(f"\ndiv_core({_float(numer)!r}, b): domain [{lo!r}, {hi!r}], {got}")
    assert got["mismatches"] == 0, f"first differing pair: a = {got['first_bad'][0]:#010x}, b = {got['first_bad'][1]:#010x}"
    assert got["lanes"] == ALL and got["short_lanes"] == inside
    assert _bits(lo) > 0x00800000 and _bits(hi) < 0x7F000000, "denominators below and above the domain are in the set"


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 0xC0FFEE], ids=["seed_1", "seed_c0ffee"])
def test_quotient_every_exponent_pair(ctx, seed):
    """every pair of normal exponents (254 x 254) with 64 mantissa pairs each, edge and seeded random: 0 mismatches inside the domain, and the set has pairs inside and
    pairs outside it (the count inside is what the domain's exponent range gives: 94 exponents a side, the upper border's own exponent with its zero mantissa only)"""
    got = ctx.div_sweep(3, 0, PAIR_SET, 1, seed)
    lo, hi = got["domain"]
    print(f"\ndiv_core over exponent pairs, seed {seed:#x}: {got}")
    assert got["mismatches"] == 0, f"first differing pair: a = {got['first_bad'][0]:#010x}, b = {got['first_bad'][1]:#010x}"
    assert got["lanes"] == PAIR_SET
    e_lo, e_hi = _bits(lo) >> 23, _bits(hi) >> 23
    whole = e_hi - e_lo               # exponents wholly inside: e_lo .. e_hi - 1
    assert (whole * whole) * 64 <= got["short_lanes"] <= ((whole + 1) * (whole + 1)) * 64
    assert 0 < got["short_lanes"] < got["lanes"]
    assert e_lo > 1 and e_hi < 254, "exponents on each side of both borders are in the set"


@pytest.mark.gpu
def test_the_sweep_finds_an_inexact_quotient(ctx):
    """the sweep's own control: a * v_rcp_f32(b) in div_core's place is reported -- mismatches, the first one by its bits, and that pair alone mismatches again"""
    got = ctx.div_sweep(2, 0, ALL, 1, _bits(CAM_COLS - 0.5))
    lo, hi = got["domain"]
    print(f"\na * v_rcp_f32(b): {got}")
    assert 0 < got["mismatches"] < got["short_lanes"]
    a, b = got["first_bad"]
    assert a == _bits(CAM_COLS - 0.5) and lo <= abs(_float(b)) <= hi
    assert ctx.div_sweep(2, b, 1, 1, a)["mismatches"] == 1
    assert ctx.div_sweep(1, b, 1, 1, a)["mismatches"] == 0


@pytest.mark.gpu
def test_the_camera_division_every_pixel_of_every_extent(ctx):
    """fx / W as k_frame computes it, for EVERY extent the API admits (1..16384) and every column of the tiles that cover it -- a superset of x in [0, W) for
    W in {1, 2, 3, 64, 1920, 3840, 16384}, which are also run one by one: all operands inside the domain (no lane falls back), 0 mismatches"""
    got = ctx.div_sweep(4, 0, CAM_COLS * CAM_MAX_W, 1)
    lo, hi = got["domain"]
    expected = sum((W + 31) // 32 * 32 for W in range(1, CAM_MAX_W + 1))
    print(f"\ncamera fx / W, every extent: {got}")
    assert lo <= 0.5 and CAM_COLS - 0.5 <= hi and lo <= 1.0 and CAM_MAX_W <= hi, "the operands' bounds lie inside the domain"
    assert got["mismatches"] == 0, f"first differing pair: a = {_float(got['first_bad'][0])!r}, b = {_float(got['first_bad'][1])!r}"
    assert got["lanes"] == expected == got["short_lanes"]
    for W in (1, 2, 3, 64, 1920, 3840, CAM_MAX_W):
        one = ctx.div_sweep(4, (W - 1) * CAM_COLS, W, 1)
        assert one["mismatches"] == 0 and one["lanes"] == W == one["short_lanes"], (W, one)


@pytest.mark.gpu
def test_bad_arguments(ctx):
    """which above 4 and a count above 2^32 are refused; art_parity_math_sweep goes on refusing which above 4"""
    from araytracingjourney_amd._lib import ArtError
    with pytest.raises(ArtError):
        ctx.div_sweep(5)
    with pytest.raises(ArtError):
        ctx.div_sweep(0, 0, ALL + 1)
    with pytest.raises(ArtError):
        ctx.math_sweep(5)
