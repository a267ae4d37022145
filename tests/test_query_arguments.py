"""What the queries on device buffers refuse, and in which words: cast_rays (both kinds), cast_rays_multi, resolve_hits, closest_points and cast_spheres check their
tensors before anything is enqueued, and the five C entry points behind them check their descriptors.  Every text below is a literal: hosts log them."""
import ctypes as C

import pytest

N = 5   # rays, records or points a call
K = 3   # cast_rays_multi's records a ray

_RAYS = ("rays must be a torch tensor on cuda:0", "rays must be float32 of shape (n, 8), contiguous and 16-byte aligned")
_POINTS = ("points must be a torch tensor on cuda:0", "points must be float32 of shape (n, 4), contiguous and 16-byte aligned")
_RECORDS = ("tuv must be a contiguous torch.float32 tensor on cuda:0 of shape (n, 4) or (n, K, 4), 16-byte aligned",) * 2
_TUV = "out: tuv must be a contiguous torch.float32 tensor on cuda:0 of shape (>= n, 4), 16-byte aligned"
_IDS = "out: ids must be a contiguous torch.int32 tensor on cuda:0 of shape (>= n, 2), 8-byte aligned"
_HIT = "out: hit must be a contiguous torch.uint8 tensor on cuda:0 of shape (>= n,), 1-byte aligned"
_POS = "out: pos must be a contiguous float32 tensor on cuda:0 of shape (5, 4), 16-byte aligned"
_F4, _I2 = ("float32", (4,)), ("int32", (2,))
# method -> the width of its input, its outputs (dtype, shape behind n) and the texts: the input on another device; the input of another dtype, width, layout or
# alignment; the first output a record short; the second output (the only one, where there is one) of another dtype
METHODS = {
    "cast_rays-closest": (8, (_F4, _I2), _RAYS + (_TUV, _IDS)),
    "cast_rays-any": (8, (("uint8", ()),), _RAYS + (_HIT, _HIT)),
    "cast_rays_multi": (8, (("float32", (K, 4)), ("int32", (K, 2)), ("uint8", ())),
                        _RAYS + ("out: tuv must be a contiguous torch.float32 tensor on cuda:0 of shape (>= n, 3, 4,), 16-byte aligned",
                                 "out: ids must be a contiguous torch.int32 tensor on cuda:0 of shape (>= n, 3, 2,), 8-byte aligned")),
    "resolve_hits": (4, (_F4,), _RECORDS + (_POS, _POS)),
    "closest_points": (4, (_F4, _I2, _F4), _POINTS + ("out: duv must be a contiguous torch.float32 tensor on cuda:0 of shape (>= n, 4), 16-byte aligned", _IDS)),
    "cast_spheres": (8, (_F4, _I2, _F4), _RAYS + (_TUV, _IDS)),
}
BAD = ("on the cpu", "float64", "wrong width", "not contiguous", "misaligned by 4 bytes", "out: a record short", "out: wrong dtype")


@pytest.fixture(scope="module")
def cornell(get_scene):
    import torch
    from araytracingjourney_amd import renderer
    r = renderer.renderer_for_scene(get_scene("cornell"), (64, 64), device=0)
    r.prepare_first_frame()
    yield r, torch
    r.close()


def _call(r, torch, method, x, out):
    if method == "cast_rays-closest":
        return r.cast_rays(x, "closest", out=out)
    if method == "cast_rays-any":
        return r.cast_rays(x, "any", out=None if out is None else out[0])
    if method == "cast_rays_multi":
        return r.cast_rays_multi(x, K, out=out)
    if method == "resolve_hits":
        return r.resolve_hits(x, torch.full((N, 2), -1, dtype=torch.int32, device="cuda:0"), want=("pos",), out=None if out is None else dict(pos=out[0]))
    if method == "closest_points":
        return r.closest_points(x, out=out)
    return r.cast_spheres(x, 0.125, out=out)


def _outputs(torch, outs, n):
    return [torch.zeros((n,) + shape, dtype=getattr(torch, dtype), device="cuda:0") for dtype, shape in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("method", list(METHODS))
def test_a_bad_tensor_is_refused_in_the_recorded_words_and_nothing_is_enqueued(cornell, method, bad):
    r, torch = cornell
    w, outs, (where, what, short, dtype) = METHODS[method]
    x, out, text = torch.zeros((N, w), dtype=torch.float32, device="cuda:0"), None, what
    if bad == "on the cpu":
        x, text = x.cpu(), where
    elif bad == "float64":
        x = x.double()
    elif bad == "wrong width":
        x = x[:, :w - 1].contiguous()
    elif bad == "not contiguous":
        x = torch.zeros((w, N), dtype=torch.float32, device="cuda:0").t()
        assert x.shape == (N, w) and not x.is_contiguous()
    elif bad == "misaligned by 4 bytes":
        x = torch.zeros((N * w + 1,), dtype=torch.float32, device="cuda:0")[1:].view(N, w)
        assert x.is_contiguous() and x.data_ptr() % 16 == 4
    elif bad == "out: a record short":
        out, text = _outputs(torch, outs, N), short
        out[0] = _outputs(torch, outs, N - 1)[0]
    else:
        out, text = _outputs(torch, outs, N), dtype
        k = min(1, len(out) - 1)
        out[k] = out[k].to(torch.float64)
    before = r.cast_counts()
    with pytest.raises(ValueError) as e:
        _call(r, torch, method, x, None if out is None else tuple(out))
    assert str(e.value) == text
    assert r.cast_counts() == before


@pytest.mark.gpu
@pytest.mark.parametrize("method", list(METHODS))
def test_the_same_tensors_without_the_fault_are_accepted(cornell, method):
    """what the cases above start from: n records in and outputs of exactly n records, given or made by the call"""
    r, torch = cornell
    w, outs, _ = METHODS[method]
    x = torch.zeros((N, w), dtype=torch.float32, device="cuda:0")
    given = _outputs(torch, outs, N)
    got = _call(r, torch, method, x, tuple(given))
    made = _call(r, torch, method, x, None)
    r.cast_sync()
    torch.cuda.synchronize()
    for res in (got, made):
        res = list(res.values()) if isinstance(res, dict) else [res] if isinstance(res, torch.Tensor) else list(res)
        assert [(t.dtype, tuple(t.shape)) for t in res] == [(t.dtype, tuple(t.shape)) for t in given]


ENTRY_POINTS = [("art_cast_rays", "ArtRayCast", {}, b"art_cast_rays: null argument", b"art_cast_rays: flags: must be 0"),
                ("art_cast_rays_multi", "ArtRayCastMulti", dict(max_hits=1), b"art_cast_rays_multi: null argument", b"art_cast_rays_multi: flags: must be 0"),
                ("art_resolve_hits", "ArtHitResolve", {}, b"art_resolve_hits: null argument", b"art_resolve_hits: flags: must be 0"),
                ("art_closest_points", "ArtPointQuery", {}, b"art_closest_points: null argument", b"art_closest_points: flags: must be 0"),
                ("art_cast_spheres", "ArtSphereCast", {}, b"art_cast_spheres: null argument", b"art_cast_spheres: flags: must be 0")]


@pytest.mark.parametrize("name,desc,fields,null_text,flags_text", ENTRY_POINTS)
def test_an_entry_point_refuses_null_arguments_and_flags_on_any_machine(name, desc, fields, null_text, flags_text):
    """no device is needed: a NULL context or descriptor is refused first, and nonzero flags before the context is looked at -- the context handed over here is 64 KB of
    zeros that no entry point gets to read"""
    from araytracingjourney_amd import _lib
    L = _lib.load()
    fn = getattr(L, name)
    d = getattr(_lib, desc)(flags=1, **fields)
    nowhere = C.create_string_buffer(1 << 16)
    for ctx, dd in ((None, C.byref(d)), (nowhere, None), (None, None)):
        assert fn(ctx, dd) == _lib.ART_E_INVALID and L.art_last_error() == null_text
    for flags in (1, 0x80000000):
        d.flags = flags
        assert fn(nowhere, C.byref(d)) == _lib.ART_E_INVALID and L.art_last_error() == flags_text
