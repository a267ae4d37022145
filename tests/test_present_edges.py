"""art_present on buffers of the test's making: the three packers of k_present at every code, rounding tie, carry and special value, and its tone mapper against the
fp64 witness (tests/np_shading.py) at every grey code, the primaries, near-greys and random words, with and without AO.  A rendered frame reaches none of this: its
colours are finite, non-negative and moderate, its depths positive.

The CPU half judges the oracle's packers by the formats' definition (tests/test_present.py ufloat_table / ufloat_encode; numpy's float16 for R16_SFLOAT) and the
oracle's tone mapper by the witness on the very colour set the GPU half uses; the GPU half judges k_present by the definition and the witness directly, and by the
oracle only where the definition leaves a choice (which NaN code) or the witness does not apply (a pixel with an Inf or NaN channel)."""
import functools
import math

import numpy as np
import pytest

import np_shading as NP
from helpers import MadeUpFrame, R  # noqa: F401  (R: module fixture)
from test_present import _values, ufloat_encode, ufloat_nan_code, ufloat_table

FLT_MAX = np.finfo(np.float32).max


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def _flip(v, every=3):
    """the sign bit of every third entry flipped (on the bits: a NaN keeps its payload)"""
    u = np.array(v, np.float32).view(np.uint32)
    u[::every] ^= np.uint32(0x80000000)
    return u.view(np.float32)


# ---- the value lists -----------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ufloat_mids(mb):
    """the midpoints of every pair of adjacent codes, the pair (largest finite code, Inf code = 2^16) last: exact in float32"""
    t = np.concatenate([ufloat_table(mb), [65536.0]])
    mid = 0.5 * (t[:-1] + t[1:])
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
    return mid.astype(np.float32)


def overflow_values(mb):
    """the largest finite code's value, its upper midpoint and that one's two float32 neighbours, 2^16, 1e6, FLT_MAX"""
    top, mid = np.float32(ufloat_table(mb)[-1]), ufloat_mids(mb)[-1]
    return np.array([top, np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, np.float32(np.inf)), 65536.0, 1e6, FLT_MAX], np.float32)


@functools.lru_cache(None)
def ufloat_values(mb):
    t, mid = ufloat_table(mb), ufloat_mids(mb)
    first_normal = np.float32(t[1 << mb])                                                      # 2^-14
    return np.concatenate([
        t.astype(np.float32),                                                                  # every finite code's value
        mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)),          # every tie and its two neighbours (mid[0]: half the smallest denormal code)
        _f32([1, 2, 0x400000, 0x7FFFFF, 0x800000]),                                            # float32 denormals and the first float32 normal
        np.array([np.nextafter(first_normal, np.float32(0))], np.float32),                     # the last float32 below the first normal code: the denormal mantissa carries
        np.array([0.0, -0.0, -1.0, -np.inf, np.inf], np.float32),
        _f32([0x7FC00000, 0x7F800001, 0xFFC00000]),                                            # NaN: quiet, signalling, sign bit set
        _values(2000, 3 + mb),                                                                 # 2e-9 .. 5e8, log-uniform
        overflow_values(mb)])


@functools.lru_cache(None)
def f16_values():
    pos = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)               # every finite code of the positive half
    mid64 = 0.5 * (pos[:-1].astype(np.float64) + pos[1:].astype(np.float64))
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64)
    trip = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))])
    extra = np.array([65504.0, np.nextafter(np.float32(65520.0), np.float32(0)), 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                      np.nextafter(np.float32(2.0 ** -25), np.float32(0)), 0.0, -0.0, np.inf, -np.inf, np.nan, 10000.0, 1e-45, FLT_MAX, -FLT_MAX], np.float32)
    return np.concatenate([pos, -pos, trip, -trip[::4], extra])


def f16_definition(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float32).astype(np.float16).view(np.uint16)


def oracle_pack(orc, r, g, b):
    """the oracle's packed words of n colours (orc_present packs with orc_pack_b10g11r11)"""
    col = np.zeros((1, len(r), 4), np.float32)
    col[0, :, 0], col[0, :, 1], col[0, :, 2] = r, g, b
    return orc.present(col)[0][0]


def _fields(w):
    return w & 0x7FF, (w >> 11) & 0x7FF, w >> 22


# ---- CPU: the definition says what it should, and the oracle's packers are the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [6, 5])
def test_definition_round_trips_every_code_and_sends_ties_to_even(mb):
    t, mid = ufloat_table(mb), ufloat_mids(mb)
    n = 31 << mb
    assert len(t) == n == (1984 if mb == 6 else 992) and t[0] == 0 and np.all(np.diff(t) > 0) and t[-1] == (65024.0 if mb == 6 else 64512.0)
    c = np.arange(n, dtype=np.uint32)
    assert np.array_equal(ufloat_encode(t, mb), c)                                             # pack(v_c) = c
    assert np.array_equal(ufloat_encode(mid, mb), c + (c & 1))                                 # a tie: the even one of c, c + 1
    assert np.array_equal(ufloat_encode(np.nextafter(mid, np.float32(0)), mb), c) and np.array_equal(ufloat_encode(np.nextafter(mid, np.float32(np.inf)), mb), c + 1)
    assert ufloat_encode(mid[0], mb) == 0 and mid[0] == t[1] / 2                               # half the smallest denormal code: the tie goes to 0
    assert np.array_equal(ufloat_encode(np.array([-0.0, -1.0, -np.inf, np.inf], np.float32), mb), [0, 0, 0, 31 << mb])
    assert ufloat_nan_code(ufloat_encode(_f32([0x7FC00000, 0x7F800001, 0xFFC00000]), mb), mb).all() and not ufloat_nan_code(np.arange(n + 1), mb).any()
    assert ufloat_encode(np.nextafter(np.float32(2.0 ** -14), np.float32(0)), mb) == 1 << mb   # the carry out of the denormal codes


@pytest.mark.parametrize("mb", [6, 5])
def test_oracle_small_float_packer_is_the_definition(orc, mb):
    v = ufloat_values(mb)
    fields = _fields(oracle_pack(orc, v, v, v))
    got = fields[0 if mb == 6 else 2]
    assert np.array_equal(fields[1], fields[0])
    nan = np.isnan(v)
    assert nan.sum() == 3 and ufloat_nan_code(got[nan], mb).all()
    assert np.array_equal(got[~nan], ufloat_encode(v, mb)[~nan])
    # pack(unpack(code)) = code on every finite code and the Inf code, through the oracle's own unpack
    n = 31 << mb
    un = np.array([orc.unpack_b10g11r11(c << (0 if mb == 6 else 22))[0 if mb == 6 else 2] for c in range(n + 1)], np.float32)
    assert np.array_equal(un[:n].astype(np.float64), ufloat_table(mb)) and np.isinf(un[n])
    assert np.array_equal(_fields(oracle_pack(orc, un, un, un))[0 if mb == 6 else 2], np.arange(n + 1))


def test_oracle_f16_packer_is_numpys(orc):
    v = f16_values()
    got = np.array([orc.pack_f16(float(x)) for x in v], np.uint16)
    assert np.array_equal(got, f16_definition(v))
    n = 0x7C00
    assert np.array_equal(got[:n], np.arange(n)) and np.array_equal(got[n:2 * n], np.arange(n) | 0x8000)   # every finite code of both signs round-trips


@pytest.mark.parametrize("mb", [6, 5])
def test_finite_overflow_becomes_the_inf_code(orc, mb):
    """The rule as the project has it today, pinned and open: a finite value past the largest finite code (65024 with 6 mantissa bits, 64512 with 5) rounds as if the
    Inf code were the next value, 2^16 -- from the midpoint (65280, 65024) up it becomes the Inf code, below it the largest finite code.  The visible consequence: the
    tone mapper reads the packed image, so an over-range channel presents as a BLACK pixel (grey 1000 presents as 255, grey 65024 as 0: its blue is past 64512).
    Whether the reference's hardware does this is unverified: the OpenGL rule for the format is recalled as "finite values above the maximum convert to the maximum",
    which would clamp instead.  The rule is not changed here; whoever changes it changes this test"""
    v = overflow_values(mb)
    top, inf = (31 << mb) - 1, 31 << mb
    want = [top, top, inf, inf, inf, inf, inf]
    assert np.array_equal(ufloat_encode(v, mb), want)
    assert np.array_equal(_fields(oracle_pack(orc, v, v, v))[0 if mb == 6 else 2], want)
    grey = np.zeros((1, 3, 4), np.float32)
    grey[0, :, :3] = np.array([1000.0, 64512.0, 65024.0], np.float32)[:, None]
    assert np.array_equal(orc.present(grey)[1][0, :, :3], [[255] * 3, [255] * 3, [0] * 3])


# ---- the tone mapper's colour set: every colour the exact value of a packed word -------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def colour_words():
    """-> (words [6 216] uint32, n_grey): (a) the 1 984 grey codes c (blue: the 10-bit code c >> 1), in code order; (b) R, G, B, RG, GB, RB alone at every 8th code;
    (c) greys with one channel one code up or down at every 16th code (kept inside the finite codes); (d) 2 000 random finite words"""
    c = np.arange(1984, dtype=np.uint32)
    word = lambda r, g, b: (np.asarray(r, np.uint32) | (np.asarray(g, np.uint32) << 11) | (np.asarray(b, np.uint32) << 22)).astype(np.uint32)
    sets = [word(c, c, c >> 1)]
    c8, z = c[::8], np.zeros(248, np.uint32)
    sets += [word(c8, z, z), word(z, c8, z), word(z, z, c8 >> 1), word(c8, c8, z), word(z, c8, c8 >> 1), word(c8, z, c8 >> 1)]
    c16 = c[::16].astype(np.int64)
    for d in (1, -1):
        sets += [word(np.clip(c16 + d, 0, 1983), c16, c16 >> 1), word(c16, np.clip(c16 + d, 0, 1983), c16 >> 1), word(c16, c16, np.clip((c16 >> 1) + d, 0, 991))]
    rng = np.random.default_rng(11)
    sets.append(word(rng.integers(0, 1984, 2000), rng.integers(0, 1984, 2000), rng.integers(0, 992, 2000)))
    words = np.concatenate(sets)
    assert len(words) == 6216
    return words, 1984


def colours_of(words):
    """[n, 4] float32: the exact values of the words' three channels, alpha 1"""
    r, g, b = _fields(np.asarray(words, np.uint32))
    col = np.ones((len(words), 4), np.float32)
    col[:, 0], col[:, 1], col[:, 2] = ufloat_table(6)[r], ufloat_table(6)[g], ufloat_table(5)[b]
    return col


def special_colours():
    """colours with an Inf or NaN channel beside channels of 0, 1 and 1000, all-Inf and all-NaN: the witness does not apply, the oracle's BGRA does"""
    out = []
    for bad in (np.inf, np.nan):
        for k in range(3):
            for other in (0.0, 1.0, 1000.0):
                c = [other, other, other, 1.0]
                c[k] = bad
                out.append(c)
        out.append([bad, bad, bad, 1.0])
    return np.array(out, np.float32)


@functools.lru_cache(None)
def _witness_ao255():
    P = NP.lpm_setup_709()
    return np.array([NP.present_pixel(int(w), 255, P) for w in colour_words()[0]])


def judge(got_bgra, want):
    """the project's criterion (test_presentation_against_numpy_in_fp64): every 8-bit channel is floor(want + 0.5), or -- where want + 0.5 lies within 0.02 of an
    integer -- its neighbour; alpha 255.  -> the share of channels that used the allowance"""
    got = got_bgra[:, :3].astype(np.float64)
    r = np.floor(want + 0.5)
    off = got != r
    ok = (np.abs(got - r) == 1) & (np.abs((want + 0.5) - np.round(want + 0.5)) < 0.02)
    bad = off & ~ok
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    assert np.all(got_bgra[:, 3] == 255)
    return float(off.mean())


def greys_never_darken(bgra_grey, ao_grey):
    """the grey codes in code order, pixel by pixel: among the pixels of one AO value no channel falls as the grey rises.  Judged over the EVEN codes, the 992 words
    that are greys exactly.  An odd code's blue (10 bits: code >> 1) is the even code's below it: from an even code to the next odd one B / max(R, G, B) falls and
    LpmMap's saturation power takes the blue output down with it, by up to 2 of 255 (598 -> 599 is the first such step), and back up at the next even code, where the
    luma ratio's rise can cost red and green 1 (1149 -> 1150).  The witness in float64 does the same (735 falling blue steps, 184 red and green ones, none over the
    even codes), so that is the operator on a set that is not monotone, not an error of either restatement; the odd codes are judged channel by channel by judge()"""
    code = np.arange(len(bgra_grey))
    for a in np.unique(ao_grey):
        even = bgra_grey[(ao_grey == a) & (code % 2 == 0), :3].astype(int)
        assert np.all(np.diff(even, axis=0) >= 0), (a, np.argwhere(np.diff(even, axis=0) < 0)[:5])


def test_oracle_tone_mapper_on_the_colour_set(orc):
    """the CPU leg of the GPU test below (AO = 255): the oracle against the witness on all 6 216 words.  Measured: no channel of the 18 648 uses the allowance"""
    words, n_grey = colour_words()
    col = colours_of(words)
    packed, bgra = orc.present(col[None])
    assert np.array_equal(packed[0], words)                                                    # every colour IS its word
    share = judge(bgra[0], _witness_ao255())
    print(f"\n[present] oracle, AO 255: allowance used by {share:.5%} of {3 * len(words)} channels")
    assert share < 0.01
    greys_never_darken(bgra[0, :n_grey], np.full(n_grey, 255))
    assert np.all(bgra[0, 0, :3] == 0) and np.all(bgra[0, n_grey - 1, :3] == 255)              # black stays black; the largest finite word is white


# ---- GPU: k_present's packers -----------------------------------------------------------------------------------------------------------------------------------------------
PACK_W = PACK_H = 512
ALPHAS = (1.0, 7.0, np.nan, -1.0)


@pytest.fixture(scope="module")
def packer_frame(R, get_scene):
    """one 512 x 512 frame holding every list: the 11-bit list through R and (shifted by one) G, the 10-bit list through B, four times over with the colour's alpha
    1, 7, NaN and -1; the same with every third sign flipped through the normal image; the f16 list through depth.  Everything else is 0"""
    v11, v10, vd = ufloat_values(6), ufloat_values(5), f16_values()
    n = len(v11)
    r, g, b = v11, np.roll(v11, 1), v10[np.arange(n) % len(v10)]
    npix = PACK_W * PACK_H
    assert 4 * n <= npix and len(vd) <= npix
    color, normal, depth = np.zeros((npix, 4), np.float32), np.zeros((npix, 4), np.float32), np.zeros(npix, np.float32)
    for k, a in enumerate(ALPHAS):
        color[k * n:(k + 1) * n, 0], color[k * n:(k + 1) * n, 1], color[k * n:(k + 1) * n, 2], color[k * n:(k + 1) * n, 3] = r, g, b, a
    nr, ng, nb = _flip(r), _flip(g, 2), _flip(b)
    normal[:n, 0], normal[:n, 1], normal[:n, 2], normal[:n, 3] = nr, ng, nb, np.nan
    depth[:len(vd)] = vd
    f = MadeUpFrame(R, get_scene("cornell"), PACK_W, PACK_H)
    pc, pn, pd, bgra = f.present(color.reshape(PACK_H, PACK_W, 4), normal.reshape(PACK_H, PACK_W, 4), depth.reshape(PACK_H, PACK_W))
    f.close()
    return dict(n=n, rgb=(r, g, b), nrgb=(nr, ng, nb), depth=vd, pc=pc.reshape(-1), pn=pn.reshape(-1), pd=pd.reshape(-1), bgra=bgra.reshape(-1, 4))


def expected_words(orc, r, g, b):
    """the definition's word; a NaN channel's field is the oracle's (the definition allows any NaN code)"""
    o = _fields(oracle_pack(orc, r, g, b))
    f = [np.where(np.isnan(x), oc, ufloat_encode(x, mb)).astype(np.uint32) for x, oc, mb in ((r, o[0], 6), (g, o[1], 6), (b, o[2], 5))]
    assert all(ufloat_nan_code(oc[np.isnan(x)], mb).all() for x, oc, mb in ((r, o[0], 6), (g, o[1], 6), (b, o[2], 5)))
    return f[0] | (f[1] << 11) | (f[2] << 22)


@pytest.mark.gpu
def test_gpu_colour_packer_is_the_definition_whatever_the_alpha(packer_frame, orc):
    F = packer_frame
    n, want = F["n"], expected_words(orc, *F["rgb"])
    for k, a in enumerate(ALPHAS):
        got = F["pc"][k * n:(k + 1) * n]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (a, bad[:5], [hex(x) for x in got[bad[:5]]], [hex(x) for x in want[bad[:5]]], [x[bad[:5]] for x in F["rgb"]])
    assert np.all(F["pc"][4 * n:] == 0) and np.all(F["bgra"][4 * n:] == [0, 0, 0, 255])       # the rest of the frame: black


@pytest.mark.gpu
def test_gpu_normal_packer_is_the_definition_on_both_signs(packer_frame, orc):
    F = packer_frame
    n, want = F["n"], expected_words(orc, *F["nrgb"])
    got = F["pn"][:n]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], [hex(x) for x in got[bad[:5]]], [hex(x) for x in want[bad[:5]]], [x[bad[:5]] for x in F["nrgb"]])
    neg = np.signbit(F["nrgb"][0]) & ~np.isnan(F["nrgb"][0])
    assert neg.sum() > n // 4 and np.all(got[neg] & 0x7FF == 0) and np.all(F["pn"][n:] == 0)


@pytest.mark.gpu
def test_gpu_depth_packer_is_numpys_float16(packer_frame):
    F = packer_frame
    vd = F["depth"]
    got, want = F["pd"][:len(vd)], f16_definition(vd)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], [hex(x) for x in got[bad[:5]]], [hex(x) for x in want[bad[:5]]], vd[bad[:5]])
    n = 0x7C00
    assert np.array_equal(got[:n], np.arange(n)) and np.array_equal(got[n:2 * n], np.arange(n) | 0x8000) and np.all(F["pd"][len(vd):] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mb", [6, 5])
def test_gpu_finite_overflow_becomes_the_inf_code(packer_frame, mb):
    """k_present's side of test_finite_overflow_becomes_the_inf_code (which see: pinned as it stands, open; an over-range channel presents as a black pixel): the
    overflow values close each list of the packer frame"""
    F = packer_frame
    n, nv = F["n"], len(overflow_values(mb))
    top, inf = (31 << mb) - 1, 31 << mb
    if mb == 6:
        assert np.array_equal(F["rgb"][0][n - nv:], overflow_values(6))
        got = F["pc"][n - nv:n] & 0x7FF
    else:
        at = len(ufloat_values(5)) - nv                                                         # (the 10-bit list is the shorter one: blue repeats it)
        assert np.array_equal(F["rgb"][2][at:at + nv], overflow_values(5))
        got = F["pc"][at:at + nv] >> 22
    assert np.array_equal(got, [top, top, inf, inf, inf, inf, inf])


# ---- GPU: k_present's tone mapper against the fp64 witness -------------------------------------------------------------------------------------------------------------------
TONE_W, TONE_H = 128, 64


def _placement(ao, n_first, n_last):
    """pixels for the set: its last n_last items (the random words) go round-robin over the distinct AO values the frame has, the first n_first take the pixels
    that are left, in order"""
    ao = ao.reshape(-1)
    values = np.unique(ao)
    pools = [list(np.flatnonzero(ao == v)[::-1]) for v in values]
    last, k = [], 0
    while len(last) < n_last:
        if pools[k % len(pools)]:
            last.append(pools[k % len(pools)].pop())
        k += 1
    free = np.setdiff1d(np.arange(ao.size), np.array(last))
    assert len(free) >= n_first
    return np.concatenate([free[:n_first], np.array(last, np.int64)])


@pytest.mark.gpu
@pytest.mark.parametrize("ao_spp", [64, None])
def test_gpu_tone_mapper_against_numpy_in_fp64(R, orc, get_scene, ao_spp):
    """k_present's LpmMap, display gamma and 8-bit rounding against tests/np_shading.py in float64 -- its only judge that no hand of the kernel's wrote -- on the 6 216
    words of colour_words(), once under the AO of a 64-sample Cornell frame (the random words dealt round-robin over the frame's distinct AO values) and once with
    none (AO = 255); device powf is not the host's, so the oracle's agreement says nothing here.  The criterion is test_presentation_against_numpy_in_fp64's, the cap on
    the share of channels that use its allowance the existing GPU test's 1 %.
    Measured on an MI355X: 0 of the 18 648 channels use the allowance, under AO and without (share 0.00000 % both times; the test prints it)"""
    words, n_grey = colour_words()
    special = special_colours()
    col = np.concatenate([colours_of(words), special])
    f = MadeUpFrame(R, get_scene("cornell"), TONE_W, TONE_H, ao_spp)
    npix = TONE_W * TONE_H
    ao = f.ao.reshape(-1) if ao_spp else np.full(npix, 255, np.uint32)
    if ao_spp:
        assert len(np.unique(ao)) >= 32 and ao.min() < 200, (len(np.unique(ao)), ao.min())    # a spread of AO values, as test_ray_traced_ao_against_numpy_in_fp64 has it for the oracle
    n_first = len(col) - 2000
    order = np.concatenate([np.arange(len(words) - 2000), len(words) + np.arange(len(special)), np.arange(len(words) - 2000, len(words))])   # the random words last
    pix = np.empty(len(col), np.int64)
    pix[order] = _placement(ao, n_first, 2000)
    if ao_spp:
        assert len(np.unique(ao[pix[len(words) - 2000:len(words)]])) == len(np.unique(ao))     # every AO value of the frame is under some random word
    image = np.zeros((npix, 4), np.float32)
    image[pix] = col
    pc, _, _, bgra = f.present(image.reshape(TONE_H, TONE_W, 4))
    f.close()
    pc, bgra = pc.reshape(-1), bgra.reshape(-1, 4)
    want_pc, want_bgra = orc.present(image.reshape(1, npix, 4), ao.reshape(1, npix))
    assert np.array_equal(pc[pix[:len(words)]], words)                                         # every colour is its word
    assert np.array_equal(pc, want_pc[0])
    P = NP.lpm_setup_709()
    wpix, wao = pix[:len(words)], ao[pix[:len(words)]]
    want = _witness_ao255() if not ao_spp else np.array([NP.present_pixel(int(w), int(a), P) for w, a in zip(words, wao)])
    share = judge(bgra[wpix], want)
    print(f"\n[present] k_present, AO {'of %d samples' % ao_spp if ao_spp else '255'}: allowance used by {share:.5%} of {3 * len(words)} channels")
    assert share < 0.01
    greys_never_darken(bgra[wpix[:n_grey]], wao[:n_grey])
    assert np.all(bgra[wpix[0], :3] == 0) and np.all(bgra[np.setdiff1d(np.arange(npix), pix)] == [0, 0, 0, 255])   # black stays black
    spix = pix[len(words):]
    assert np.array_equal(bgra[spix], want_bgra[0][spix]), (bgra[spix], want_bgra[0][spix])    # an Inf or NaN channel: the oracle's pixel exactly
    assert np.isin(bgra[spix], (0, 255)).all()
