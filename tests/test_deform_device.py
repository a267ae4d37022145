"""art_scene_set_vertices_device ("Vertices from device buffers"): art_scene_set_vertices with the data in device memory.  One kernel on the caller's
stream writes the primitive's own slot of the build's vertex array, the next refit gathers from it, and everything is ordered on the device.  The references are those of
tests/test_deform.py: the oracle's frame of a scene built from scratch with the vertices current at the launch (depth and normal bit for bit, radiance within 1e-4), the
host form (bit for bit), and numpy for the vertex records themselves."""
import ctypes as C

import numpy as np
import pytest

import np_closest as nc
from conftest import assert_radiance_close
from helpers import _bits, _host, _layout_is_the_headers, _tex_flat, _up, R, oracle_camera, random_rays, torch  # noqa: F401  (R, torch: module fixtures)
from test_deform import _check, _deformed, _grab, _pose, _setup, _State

W = H = 160
NOWHERE_BYTES = 1 << 20   # a context's worth of zeros: an empty scene that art_scene_add_primitive can fill without a device


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_descriptor_is_the_headers_and_the_symbols_are_exported():
    from araytracingjourney_amd import _lib
    _layout_is_the_headers("ArtVertexUpdate", 40, ["verts_dev", "hip_stream", "primitive_id", "n_verts", "layout", "stride_bytes", "flags", "reserved"])
    assert (_lib.ART_VERTS_FULL, _lib.ART_VERTS_POSITIONS) == (0, 1)
    L = _lib.load()
    for name in ("art_scene_set_vertices_device", "art_scene_get_vertices"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert "art_vertex_update_counts" in _lib.PARITY_SYMBOLS and L.art_vertex_update_counts is not None


def _unbuilt_scene(n_verts=5):
    """zeros where a context would be (an empty, unbuilt scene: no entry point below gets to touch a device before it refuses) with one primitive of n_verts vertices"""
    from araytracingjourney_amd import _lib
    L = _lib.load()
    ctx = C.create_string_buffer(NOWHERE_BYTES)
    v = np.arange(n_verts * 12, dtype=np.float32).reshape(n_verts, 12)
    idx = np.array([0, 1, 2], np.uint16)
    tex = np.zeros((3, 1, 1, 4), np.uint8)
    m = np.eye(3, 4, dtype=np.float32)
    pid = C.c_uint32(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.art_scene_add_primitive(ctx, p(v), n_verts, p(idx), 3, 2, p(tex), 1, 1, p(m), C.byref(pid)) == _lib.ART_OK and pid.value == 0
    return _lib, L, ctx, v


def _host_copy(L, ctx, n):
    out = np.full((n, 12), -1, np.float32)
    assert L.art_scene_get_vertices(ctx, 0, out.ctypes.data_as(C.c_void_p), n) == 0
    return out


def test_every_refusal_comes_before_a_device_is_needed_and_changes_nothing():
    lib, L, ctx, v = _unbuilt_scene()
    n = v.shape[0]
    somewhere = 0x7F0000001000   # an address that is never read: 16-byte aligned
    ok = dict(verts_dev=somewhere, hip_stream=None, primitive_id=0, n_verts=n, layout=lib.ART_VERTS_FULL, stride_bytes=0, flags=0, reserved=0)
    pos = dict(ok, layout=lib.ART_VERTS_POSITIONS)
    bad = [("null verts_dev", dict(ok, verts_dev=None)), ("unknown id", dict(ok, primitive_id=1)), ("another count", dict(ok, n_verts=n - 1)), ("another count", dict(ok, n_verts=n + 1)),
           ("unknown layout", dict(ok, layout=2)), ("unknown layout", dict(ok, layout=0xFFFFFFFF)), ("FULL stride", dict(ok, stride_bytes=12)), ("FULL stride", dict(ok, stride_bytes=64)),
           ("POSITIONS stride", dict(pos, stride_bytes=8)), ("POSITIONS stride", dict(pos, stride_bytes=4)), ("POSITIONS stride", dict(pos, stride_bytes=14)),
           ("FULL alignment", dict(ok, verts_dev=somewhere + 4)), ("FULL alignment", dict(ok, verts_dev=somewhere + 8)), ("POSITIONS alignment", dict(pos, verts_dev=somewhere + 2)),
           ("POSITIONS alignment", dict(pos, verts_dev=somewhere + 1)), ("flags", dict(ok, flags=1)), ("flags", dict(pos, flags=0x80000000)), ("reserved", dict(ok, reserved=1))]
    for what, fields in bad:
        u = lib.ArtVertexUpdate(**fields)
        assert L.art_scene_set_vertices_device(ctx, C.byref(u)) == lib.ART_E_INVALID, what
        assert L.art_last_error().startswith(b"art_scene_set_vertices_device: "), what
    u = lib.ArtVertexUpdate(**ok)
    assert L.art_scene_set_vertices_device(None, C.byref(u)) == lib.ART_E_INVALID and L.art_scene_set_vertices_device(ctx, None) == lib.ART_E_INVALID
    assert L.art_last_error() == b"art_scene_set_vertices_device: null argument"
    assert np.array_equal(_bits(_host_copy(L, ctx, n)), _bits(v))
    out = np.zeros((n, 12), np.float32)
    for args in ((None, 0, out.ctypes.data_as(C.c_void_p), n), (ctx, 0, None, n), (ctx, 1, out.ctypes.data_as(C.c_void_p), n), (ctx, 0, out.ctypes.data_as(C.c_void_p), n + 1)):
        assert L.art_scene_get_vertices(*args) == lib.ART_E_INVALID
    a, b, c = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
    assert L.art_vertex_update_counts(ctx, C.byref(a), C.byref(b), C.byref(c)) == 0 and (a.value, b.value, c.value) == (0, 0, 0)
    assert L.art_vertex_update_counts(None, None, None, None) == lib.ART_E_INVALID


def test_a_valid_call_without_a_device_says_so():
    lib, L, ctx, v = _unbuilt_scene()
    if L.art_device_count() > 0:
        return   # (a machine with a device: the calls would go through, and the GPU cases below make them)
    for layout in (lib.ART_VERTS_FULL, lib.ART_VERTS_POSITIONS):
        u = lib.ArtVertexUpdate(verts_dev=0x7F0000001000, hip_stream=None, primitive_id=0, n_verts=v.shape[0], layout=layout, stride_bytes=0, flags=0, reserved=0)
        assert L.art_scene_set_vertices_device(ctx, C.byref(u)) == lib.ART_E_NO_DEVICE
    assert np.array_equal(_bits(_host_copy(L, ctx, v.shape[0])), _bits(v))


def test_model_set_vertices_device_checks_its_arguments_first():
    from araytracingjourney_amd import renderer
    m = renderer.Model([0], None, positions=[np.zeros((4, 3), np.float32)])
    with pytest.raises(ValueError) as e:
        m.set_vertices_device(0, np.zeros((4, 12), np.float32), layout="some")
    assert str(e.value) == "layout must be 'full' or 'positions'"
    with pytest.raises(ValueError) as e:
        m.set_vertices_device(0, np.zeros((4, 12), np.float32))
    assert str(e.value) == "the model belongs to no renderer"


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------------------------
def _cornell(R, get_scene, **kw):
    sc = get_scene("cornell")
    movers = [len(sc.primitives) - 1]
    r, model = _setup(R, sc, movers, (W, H), sc.lights, **kw)
    return sc, movers, r, model, _State(sc, movers)


def _deform_dev(torch, model, state, i, buf=None, **kw):
    """test_deform's _deform through the device form.  buf: ONE tensor, filled on torch's current stream in front of the call and overwritten on it right behind"""
    for k, j in enumerate(state.movers):
        v = _deformed(state.sc.primitives[j], i, **kw)
        t = _up(torch, v) if buf is None else buf
        if buf is not None:
            buf.copy_(_up(torch, v))
        model.set_vertices_device(k, t)
        if buf is not None:
            buf.fill_(float("nan"))
        state.verts[j] = v


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", [False, True], ids=["versions-at-first-deformation", "versions-at-build"])
def test_cornell_last_primitive_deforms_from_one_reused_tensor(R, torch, orc, get_scene, dynamic):
    """1: the FULL form before each of four frames in flight, out of one tensor that is overwritten with NaN on the same stream right behind each call: the ingest read
    it in stream order.  Four kernels, at most the first deformation's synchronisation, nothing read back"""
    F = 4
    sc, movers, r, model, state = _cornell(R, get_scene, frames_in_flight=F, dynamic_scene=dynamic)
    r.trace(); r.sync()
    buf = torch.empty((sc.primitives[movers[0]].verts.shape[0], 12), dtype=torch.float32, device="cuda:0")
    got = []
    with torch.cuda.stream(torch.cuda.Stream()):
        for i in range(F):
            _deform_dev(torch, model, state, i, buf)
            r.trace()
            got.append((state.prims(), _grab(r)))
    r.sync()
    st, cnt = r.stats(), r.vertex_update_counts()
    assert st["refits"] == F and st["rebuilds"] == 0
    assert cnt["ingests"] == F and cnt["host_syncs"] <= 1 and cnt["readbacks"] == 0, cnt
    for i, (prims, ptr) in enumerate(got):
        _check(orc, sc, prims, ptr, W, H, sc.lights, f"frame {i}")
    torch.cuda.synchronize()
    r.close()


@pytest.mark.gpu
def test_the_same_bits_as_the_host_form(R, torch, get_scene):
    """2: two contexts, one schedule -- deform, move + deform in one refit, deform twice between frames, disable, deform while out, enable -- one through
    set_vertices, the other through set_vertices_device: colour, depth, normal and a closest cast's records are bit-equal after every step"""
    from araytracingjourney_amd._lib import check
    sc, movers, a, ma, sa = _cornell(R, get_scene, frames_in_flight=2)
    _, _, b, mb, sb = _cornell(R, get_scene, frames_in_flight=2)
    rays = _up(torch, random_rays(4096, 5))
    base = sc.primitives[movers[0]].model

    def both(f):
        f(a, ma, False); f(b, mb, True)

    def deform(i):
        def f(r, model, dev):
            v = _deformed(sc.primitives[movers[0]], i)
            model.set_vertices_device(0, _up(torch, v)) if dev else model.set_vertices(0, v)
        both(f)

    def enable(on):
        both(lambda r, model, dev: check(r._L.art_scene_set_primitive_enabled(r._ctx, model.primitive_ids[0], 1 if on else 0)))

    steps = [("deform", lambda: deform(0)), ("move + deform", lambda: (both(lambda r, model, dev: model.set_model_matrix(_pose(base, 2))), deform(1))),
             ("deform twice", lambda: (deform(2), deform(3))), ("disable", lambda: enable(False)), ("deform while out", lambda: deform(4)), ("enable", lambda: enable(True))]
    for what, edit in steps:
        edit()
        out = []
        for r in (a, b):
            r.upload_state(); r.trace(); r.sync()
            tuv, ids = r.cast_rays(rays)
            torch.cuda.synchronize()
            out.append((r.read_color(), r.read_depth(), r.read_normal(), tuv.cpu().numpy(), ids.cpu().numpy()))
        for name, x, y in zip(("colour", "depth", "normal", "tuv", "ids"), *out):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what}: {name}"
    assert a.stats()["refits"] == b.stats()["refits"] and a.stats()["rebuilds"] == b.stats()["rebuilds"] == 0
    assert b.vertex_update_counts()["readbacks"] == 0 and a.vertex_update_counts() == dict(ingests=0, host_syncs=0, readbacks=0)
    a.close(); b.close()


@pytest.mark.gpu
def test_positions_keep_the_current_attributes(R, torch, get_scene):
    """3: POSITIONS at strides 12 and 16 and as a 3-column view at a byte offset inside an [n, 8] tensor, on the primitive as added, after a FULL call and after a
    host-form call that changed normals and uvs: frames and Model.vertices() are those of the host form given the same positions with the attributes current then"""
    sc, movers, d, md, _ = _cornell(R, get_scene)
    _, _, h, mh, _ = _cornell(R, get_scene)
    prim = sc.primitives[movers[0]]
    n = prim.verts.shape[0]
    cur = np.array(prim.verts, np.float32)
    rng = np.random.default_rng(11)

    def carrier(kind, pos):
        if kind == "stride 12":
            return _up(torch, pos)
        if kind == "stride 16":
            t = torch.full((n, 4), float("nan"), device="cuda:0"); t[:, :3] = _up(torch, pos)
            v = t[:, :3]
            assert v.stride(0) == 4 and v.data_ptr() % 16 == 0
            return v
        t = torch.full((n, 8), float("nan"), device="cuda:0"); t[:, 2:5] = _up(torch, pos)
        v = t[:, 2:5]
        assert v.stride(0) == 8 and v.data_ptr() % 16 == 8
        return v

    def before(kind):
        nonlocal cur
        if kind == "stride 16":     # a FULL call first: its attributes are the current ones
            cur = _deformed(prim, 3)
            md.set_vertices_device(0, _up(torch, cur)); mh.set_vertices(0, cur)
        if kind == "a view":        # a host-form call first, on both: the device copy is behind the host's when POSITIONS comes
            cur = _deformed(prim, 6)
            md.set_vertices(0, cur); mh.set_vertices(0, cur)

    for i, kind in enumerate(("stride 12", "stride 16", "a view")):
        before(kind)
        pos = (cur[:, 0:3] * np.float32(0.9 - 0.1 * i) + rng.uniform(-0.02, 0.02, (n, 3)).astype(np.float32)).astype(np.float32)
        want = cur.copy(); want[:, 0:3] = pos
        md.set_vertices_device(0, carrier(kind, pos), layout="positions")
        mh.set_vertices(0, want)
        cur = want
        for r in (d, h):
            r.trace(); r.sync()
        for name in ("read_color", "read_depth", "read_normal"):
            assert np.array_equal(getattr(d, name)().view(np.uint32), getattr(h, name)().view(np.uint32)), f"{kind}: {name}"
        assert np.array_equal(_bits(md.vertices(0)), _bits(want)), kind
        assert np.array_equal(_bits(mh.vertices(0)), _bits(want)), kind
    assert d.stats()["rebuilds"] == 0 and d.vertex_update_counts()["ingests"] == 4
    d.close(); h.close()


STRIP_SIZES = (1, 63, 64, 65, 4097)


def _strips(get_scene):
    """one primitive per size: a strip of triangles over n vertices (n < 3: one degenerate triangle)"""
    P = type(get_scene("cornell").primitives[0])
    rng = np.random.default_rng(5)
    out = []
    for k, n in enumerate(STRIP_SIZES):
        v = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
        v[:, 0] = np.arange(n, dtype=np.float32) * np.float32(0.01); v[:, 2] = np.float32(k)
        idx = np.array([[i, i + 1, i + 2] for i in range(n - 2)] or [[0, 0, 0]], np.uint32).reshape(-1)
        out.append(P(v, idx, _tex_flat(255), np.eye(3, 4, dtype=np.float32)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["full", "positions 12", "positions 16", "positions in 32 at 8"])
def test_the_kernels_edges(R, torch, get_scene, form):
    """4: strips of 1, 63, 64, 65 and 4097 vertices, every form of the kernel: what art_scene_get_vertices reads back is the numpy expectation bit for bit, NaN
    payloads, infinities and -0.0 included (nothing is traced: the records only travel)"""
    prims = _strips(get_scene)
    r = R.Renderer((64, 64))
    r.add_model(prims)
    r.prepare_first_frame()
    model = r.models_mut()[0]
    rng = np.random.default_rng(17)
    want = []
    for k, p in enumerate(prims):
        n = p.verts.shape[0]
        width = 12 if form == "full" else 3
        bits = rng.integers(0, 1 << 32, (n, width), dtype=np.uint64).astype(np.uint32)
        bits[0, 0] = 0x80000000; bits[-1, 1] = 0x7FC12345; bits[n // 2, 2] = 0xFFA00001; bits[0, width - 1] = 0x7F800000   # -0.0, two NaN payloads, +inf
        new = bits.view(np.float32)
        w = np.array(p.verts, np.float32).view(np.uint32).copy()
        w[:, :width] = bits
        want.append(w)
        if form == "full":
            t = _up(torch, new)
        else:
            cols, off = {"positions 12": (3, 0), "positions 16": (4, 0), "positions in 32 at 8": (8, 2)}[form]
            wide = torch.full((n, cols), float("nan"), device="cuda:0")
            wide[:, off:off + 3] = _up(torch, new)
            t = wide[:, off:off + 3]
        model.set_vertices_device(k, t, layout="full" if form == "full" else "positions")
    for k, w in enumerate(want):
        assert np.array_equal(_bits(model.vertices(k)), w), f"{form}: {STRIP_SIZES[k]} vertices"
    cnt = r.vertex_update_counts()
    assert cnt["ingests"] == len(prims) and cnt["readbacks"] == len(prims)
    for k, w in enumerate(want):   # (the host copies are current now: nothing more is read back)
        assert np.array_equal(_bits(model.vertices(k)), w)
    assert r.vertex_update_counts()["readbacks"] == len(prims)
    torch.cuda.synchronize()
    r.close()


def _frame_is_the_oracles(orc, sc, r, prims, what):
    r.upload_state(); r.trace(); r.sync()
    _check(orc, sc, prims, _grab(r), W, H, sc.lights, what)


@pytest.mark.gpu
def test_builds_after_a_device_deformation(R, torch, orc, get_scene):
    """5: art_scene_build over the same set reads nothing back (the slot is current); a build that lays the arrays out again -- a primitive was added -- reads the
    slot back first; a primitive added after the build and one disabled at the build take the device form into their host copies and show with the next build"""
    from araytracingjourney_amd._lib import check
    sc, movers, r, model, state = _cornell(R, get_scene)
    r.trace(); r.sync()
    _deform_dev(torch, model, state, 0)
    check(r._L.art_scene_build(r._ctx))
    assert r.vertex_update_counts()["readbacks"] == 0
    _frame_is_the_oracles(orc, sc, r, state.prims(), "a build over the same set")
    _deform_dev(torch, model, state, 1)
    extra = sc.primitives[0]
    P = type(extra)
    small = P(np.array(extra.verts, np.float32) * np.array([0.3] * 3 + [1] * 9, np.float32), extra.indices, extra.tex, extra.model)   # the room's box, shrunk
    r.add_model([small])
    assert r.needs_build()
    check(r._L.art_scene_build(r._ctx))
    assert r.vertex_update_counts()["readbacks"] >= 1
    _frame_is_the_oracles(orc, sc, r, state.prims() + [small], "a build with a primitive added")
    assert np.array_equal(_bits(model.vertices(0)), _bits(state.verts[movers[0]]))
    # added after the build: the FULL form into its host copy; disabled AT a build: POSITIONS merged into its host copy.  Both show with the next build
    small2 = P(np.array(small.verts, np.float32) + np.array([0.4, 0, 0] + [0] * 9, np.float32), small.indices, small.tex, small.model)
    r.add_model([small2])
    new2 = _deformed(small2, 2, amp=0.05)
    before = r.vertex_update_counts()
    r.models_mut()[-1].set_vertices_device(0, _up(torch, new2))
    pid = model.primitive_ids[0]
    check(r._L.art_scene_set_primitive_enabled(r._ctx, pid, 0))
    check(r._L.art_scene_build(r._ctx))                      # (the mover is disabled at this build: it has no slot now)
    cur = state.verts[movers[0]]
    pos = (cur[:, 0:3] * np.float32(0.8)).astype(np.float32)
    model.set_vertices_device(0, _up(torch, pos), layout="positions")
    after = r.vertex_update_counts()
    assert after["ingests"] == before["ingests"] and after["host_syncs"] == before["host_syncs"] + 2
    merged = cur.copy(); merged[:, 0:3] = pos
    state.verts[movers[0]] = merged
    assert np.array_equal(_bits(model.vertices(0)), _bits(merged))
    check(r._L.art_scene_set_primitive_enabled(r._ctx, pid, 1))
    assert r.needs_build()
    check(r._L.art_scene_build(r._ctx))
    _frame_is_the_oracles(orc, sc, r, state.prims() + [small, P(new2, small2.indices, small2.tex, small2.model)], "a primitive added and one disabled at the build")
    r.close()


@pytest.mark.gpu
def test_the_cost_rules_own_rebuild(R, torch, orc, get_scene):
    """5: with a tiny refit_rebuild_ratio the frame behind the second device deformation builds again, over the slot as the ingest left it"""
    sc, movers, r, model, state = _cornell(R, get_scene, tuning=dict(refit_rebuild_ratio=1e-3))
    r.trace(); r.sync()
    _deform_dev(torch, model, state, 0)
    _frame_is_the_oracles(orc, sc, r, state.prims(), "refitted")
    _deform_dev(torch, model, state, 1)
    _frame_is_the_oracles(orc, sc, r, state.prims(), "rebuilt")
    assert r.stats()["rebuilds"] >= 1 and r.vertex_update_counts()["readbacks"] == 0
    _deform_dev(torch, model, state, 2)
    _frame_is_the_oracles(orc, sc, r, state.prims(), "after the rebuild")
    r.close()


@pytest.mark.gpu
def test_queries_come_first(R, torch, orc, get_scene):
    """6: after a device deformation a closest cast and a batch of closest_points come before any frame: their refit goes in front of them"""
    sc, movers, r, model, state = _cornell(R, get_scene)
    rays, q = random_rays(4096, 9), np.zeros((2048, 4), np.float32)
    q[:, 0:3] = random_rays(2048, 7)[:, 0:3]; q[:, 3] = np.inf
    d_rays, d_q = _up(torch, rays), _up(torch, q)
    for i, first in enumerate(("cast", "points")):
        _deform_dev(torch, model, state, i, amp=0.05)
        if first == "cast":
            got_c = r.cast_rays(d_rays); got_p = r.closest_points(d_q)
        else:
            got_p = r.closest_points(d_q); got_c = r.cast_rays(d_rays)
        torch.cuda.synchronize(); r.cast_sync()
        tuv, ids = _host(got_c)
        rtuv, rids = orc.Scene(state.prims(), morton_bits=30).trace_closest(rays)[:2]
        assert np.array_equal(ids, rids) and np.array_equal(_bits(tuv)[:, :3], _bits(rtuv)[:, :3]), first
        duv, pids, point = _host(got_p)
        wduv, wids, wpoint = nc.brute_force(nc.world_triangles(state.prims()), q)
        assert np.array_equal(pids, wids) and np.array_equal(_bits(duv)[:, :3], _bits(wduv)[:, :3]) and np.array_equal(_bits(point), _bits(wpoint)), first
    assert r.stats()["refits"] == 2 and r.stats()["rebuilds"] == 0
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("versions", [3, 8])
def test_versions_lag_behind_the_slot(R, torch, orc, get_scene, versions):
    """7: the model deformed from one reused tensor before each of 2 F + 3 frames launched without a host sync, 3 and 8 versions (fewer and more than the frames in
    flight): a version regathers from the slot whatever it missed, an ingest waits for the refits that still read the slot.  The last F frames -- the ones whose outputs
    still exist -- are the oracle's; the steady state makes no host sync and no read-back"""
    F = 4
    sc, movers, r, model, state = _cornell(R, get_scene, frames_in_flight=F, tuning=dict(as_versions=versions, refit_rebuild_ratio=-1.0))
    r.trace(); r.sync()
    buf = torch.empty((sc.primitives[movers[0]].verts.shape[0], 12), dtype=torch.float32, device="cuda:0")
    n, got = 2 * F + 3, []
    with torch.cuda.stream(torch.cuda.Stream()):
        _deform_dev(torch, model, state, 100, buf)   # (the first deformation's synchronisation)
        first = r.vertex_update_counts()
        for i in range(n):
            _deform_dev(torch, model, state, i, buf)
            r.trace()
            got.append((state.prims(), _grab(r)))
    r.sync()
    cnt = r.vertex_update_counts()
    assert cnt == dict(ingests=first["ingests"] + n, host_syncs=first["host_syncs"], readbacks=0) and first["host_syncs"] <= 1
    assert r.stats()["refits"] == n and r.stats()["rebuilds"] == 0
    for i in range(n - F, n):
        _check(orc, sc, got[i][0], got[i][1], W, H, sc.lights, f"frame {i}")
    torch.cuda.synchronize()
    r.close()


@pytest.mark.gpu
def test_the_calls_do_not_wait(R, torch, orc, get_scene):
    """8: on a side stream a delay of a few tens of milliseconds, then the kernel that produces the vertices, then set_vertices_device and trace: both return while the
    delay's end event has not fired, and the frame shows the producer's vertices.  The delay is timed with events: the test fails on ITSELF if it came out under 5 ms"""
    sc, movers, r, model, state = _cornell(R, get_scene, frames_in_flight=2, dynamic_scene=True)
    r.trace(); r.sync()
    _deform_dev(torch, model, state, 0)          # the first deformation (it may synchronise) and its frame are out of the way
    r.trace(); r.sync()
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):                   # how long a spin of 2 M cycles takes here: the delay below is sized from it, not guessed
        e0.record(); torch.cuda._sleep(2_000_000); e1.record()
    s.synchronize()
    cycles = int(min(max(2_000_000 * 40.0 / max(e0.elapsed_time(e1), 1e-3), 2_000_000), 2_000_000_000))
    v = _deformed(sc.primitives[movers[0]], 5)
    src = _up(torch, v)
    buf = torch.full_like(src, float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        e0.record(); torch.cuda._sleep(cycles); e1.record()
        buf.copy_(src)                           # the producer
        model.set_vertices_device(0, buf)
        pending_after_set = not e1.query()
        r.trace()
        pending_after_trace = not e1.query()
    s.synchronize(); r.sync()
    assert e0.elapsed_time(e1) >= 5.0, f"the delay took {e0.elapsed_time(e1):.2f} ms: this test proved nothing"
    assert pending_after_set, "set_vertices_device waited for the stream"
    assert pending_after_trace, "trace waited for the ingest"
    state.verts[movers[0]] = v
    _check(orc, sc, state.prims(), _grab(r), W, H, sc.lights, "the producer's vertices")
    r.close()


@pytest.mark.gpu
def test_everything_is_given_back(R, torch, get_scene):
    """9: a context that ingested on two streams (frames, casts, a read-back, a build, a host-form call in between) gives back all it took"""
    from araytracingjourney_amd._lib import check
    names = ("device", "pinned", "events", "streams")
    sc, movers, r, model, state = _cornell(R, get_scene, frames_in_flight=2)   # (the pool of streams is filled before the baseline is taken)
    r.trace(); r.sync(); r.close()
    base = R.Renderer.live_resources()
    sc, movers, r, model, state = _cornell(R, get_scene, frames_in_flight=2)
    r.trace(); r.sync()
    rays = _up(torch, random_rays(256, 3))
    _deform_dev(torch, model, state, 0); r.trace()
    with torch.cuda.stream(torch.cuda.Stream()):
        _deform_dev(torch, model, state, 1); r.cast_rays(rays); r.trace()
    model.set_vertices(0, state.verts[movers[0]])
    model.set_vertices_device(0, _up(torch, state.verts[movers[0]][:, 0:3].copy()), layout="positions"); r.trace()
    model.vertices(0)
    check(r._L.art_scene_build(r._ctx))
    _deform_dev(torch, model, state, 2); r.trace()
    _deform_dev(torch, model, state, 3)          # (an ingest nothing has waited for when the context goes)
    assert R.Renderer.live_resources()["events"] > base["events"]
    r.close()
    torch.cuda.synchronize()
    after = R.Renderer.live_resources()
    assert [after[k] for k in names] == [base[k] for k in names]
