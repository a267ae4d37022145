// art_scene.hip -- the scene behind include/art.h: the primitive table and its setters, art_scene_build, the trees the non-default walks read on demand, and the tree
// read-outs of the parity surface.  What a setter changes in a built scene it reports to the ring of versions (art_versions.hip), which refits in front of the next launch.
// Host code only; the kernels are art_build.hip's (LBVH) and art_wide.hip's (4-wide collapse).
#include "art_context.h"
#include <cmath>
#include <cstring>

static void affine_inverse(const float *m, float *o) { // row-major 3x4
    float a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    float A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    float det = a * A + b * B + c * C;
    float id = 1.0f / det;
    o[0] = A * id;  o[1] = -(b * i - c * h) * id; o[2] = (b * f - c * e) * id;
    o[4] = B * id;  o[5] = (a * i - c * g) * id;  o[6] = -(a * f - c * d) * id;
    o[8] = C * id;  o[9] = -(a * h - b * g) * id; o[10] = (a * e - b * d) * id;
    float tx = m[3], ty = m[7], tz = m[11];
    o[3] = -((o[0] * tx + o[1] * ty) + o[2] * tz);
    o[7] = -((o[4] * tx + o[5] * ty) + o[6] * tz);
    o[11] = -((o[8] * tx + o[9] * ty) + o[10] * tz);
}

// the wide collapse is host work on the finished binary tree: done lazily, the first time a walk that needs it is launched
int32_t art::ensure_wide(ArtContext *c, bool needed) {
    if (!needed || c->bvh.wide) return ART_OK;
    int32_t r = sync_all(c); if (r) return r;
    Event e0, e1; float ms = 0;
    HIPC(e0.create()); HIPC(e1.create());
    HIPC(hipEventRecord(e0, c->main_stream()));
    hipError_t e = wide_build(c->bvh, c->T, c->main_stream(), c->wide_on_host);
    if (e == hipSuccess) e = hipEventRecord(e1, c->main_stream());
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) return hipfail(e, "wide_build");
    c->stats.build_ms += ms;
    return ART_OK;
}

static void alpha_refresh_live(ArtContext *c) {
    bool any = false;
    for (const HostPrim &p : c->prims) any = any || (p.enabled && (p.cutoff > 0.0f || p.vis != 0xFFu) && p.n_indices >= 3);
    c->alpha_live = any;
}

// the binary trees and the 64-byte node records follow the versions on demand only (the non-default walks and the parity surface read them): they are
// not versioned, so this waits for everything in flight
int32_t art::ensure_binary(ArtContext *c, bool needed) {
    if (!needed || binary_is_current(c)) return ART_OK;
    int32_t r = sync_all(c); if (r) return r;
    hipError_t e = binary_refit(c->bvh, c->T, as_ptrs(c, as_current(c)).tris, c->main_stream());
    if (e != hipSuccess) return hipfail(e, "binary_refit");
    binary_mark(c, true);
    drop_graphs(c);
    return ART_OK;
}

// hit records name a triangle by its global id: the primitive is the last slot whose first triangle is <= gid (k_soup's rule)
void art::gid_to_ids(const ArtContext *c, uint32_t gid, int32_t *ids) {
    const std::vector<uint32_t> &f = c->h_first_tri;
    size_t lo = 0, hi = f.size();
    while (hi - lo > 1) { size_t mid = (lo + hi) >> 1; if (f[mid] <= gid) lo = mid; else hi = mid; }
    ids[0] = (int32_t)lo; ids[1] = (int32_t)(gid - f[lo]);
}

// A primitive whose slot of the device's vertex array is ahead of its host copy (art_scene_set_vertices_device wrote it): the slot read back, once the ingest behind it
// has finished.  Only where the library needs the host copy: a build that lays the arrays out again, art_scene_get_vertices, an update of a primitive that has left the tree
static int32_t verts_read_back(ArtContext *c, uint32_t id) {
    HostPrim &p = c->prims[id];
    if (!p.verts_behind) return ART_OK;
    int32_t r = as_ingest_wait(c, id); if (r) return r;
    HIPC(hipMemcpy(p.verts.data(), c->h_dev_prims[id].vertices, p.verts.size() * sizeof(ArtVertex), hipMemcpyDeviceToHost));
    p.verts_behind = false;
    as_ingest_counts(c, 0, 1);
    return ART_OK;
}

extern "C" {

int32_t art_scene_add_primitive(ArtContext *c, const ArtVertex *verts, uint32_t n_verts, const void *indices, uint32_t n_indices,
                                uint32_t idx_bytes, const uint8_t *rgba8, uint32_t tw, uint32_t th, const float model3x4[12], uint32_t *out_id) {
    if (!c || !verts || !indices || !rgba8 || !model3x4) return fail(ART_E_INVALID, "art_scene_add_primitive: null argument");
    if (idx_bytes != 2 && idx_bytes != 4) return fail(ART_E_INVALID, "art_scene_add_primitive: idx_bytes must be 2 or 4");
    if (n_indices == 0 || n_indices % 3 != 0) return fail(ART_E_INVALID, "art_scene_add_primitive: index count must be a positive multiple of 3");
    if (n_verts == 0 || tw == 0 || th == 0) return fail(ART_E_INVALID, "art_scene_add_primitive: empty vertices or texture");
    if (idx_bytes == 2 && n_verts > 65536) return fail(ART_E_INVALID, "art_scene_add_primitive: u16 indices cannot address the vertex count");
    for (int i = 0; i < 12; i++) if (!std::isfinite(model3x4[i])) return fail(ART_E_INVALID, "art_scene_add_primitive: non-finite model matrix");
    for (uint32_t i = 0; i < n_indices; i++) {
        uint32_t v = idx_bytes == 2 ? ((const uint16_t *)indices)[i] : ((const uint32_t *)indices)[i];
        if (v >= n_verts) return fail(ART_E_INVALID, "art_scene_add_primitive: index out of range");
    }
    HostPrim p;
    p.verts.assign(verts, verts + n_verts);
    p.indices.assign((const uint8_t *)indices, (const uint8_t *)indices + (size_t)n_indices * idx_bytes);
    p.n_indices = n_indices; p.idx_bytes = idx_bytes;
    p.tex.assign(rgba8, rgba8 + (size_t)3 * tw * th * 4);
    p.tw = tw; p.th = th;
    std::memcpy(p.o2w, model3x4, 48);
    affine_inverse(p.o2w, p.w2o);
    c->prims.push_back(std::move(p)); c->uploaded.clear();
    c->built = false;
    if (out_id) *out_id = (uint32_t)c->prims.size() - 1;
    return ART_OK;
}

int32_t art_scene_clear(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_scene_clear: null context");
    int32_t r = cast_drain(c); if (r) return r;   // outstanding casts read the scene that goes away
    if (!c->ver.ingest_open.empty()) { r = use_device(c); if (r) return r; r = as_sync_streams(c); if (r) return r; }   // (ingests on callers' streams write the slots of primitives that go away)
    c->prims.clear(); c->uploaded.clear(); c->built = false;
    return ART_OK;
}

int32_t art_scene_set_primitive_enabled(ArtContext *c, uint32_t id, int32_t enabled) {
    if (!c) return fail(ART_E_INVALID, "art_scene_set_primitive_enabled: null context");
    if (id >= c->prims.size()) return fail(ART_E_INVALID, "art_scene_set_primitive_enabled: no such primitive");
    HostPrim &p = c->prims[id];
    if (p.enabled == (enabled != 0)) return ART_OK;
    p.enabled = enabled != 0;
    alpha_refresh_live(c);
    if (!c->built) return ART_OK;                                // takes effect with the build
    if (p.n_indices < 3) return ART_OK;                          // no triangles: nothing to take out or bring back
    if (id < c->h_dev_prims.size() && c->h_dev_prims[id].n_tri > 0) {
        // Its triangles are in the built structure: they are masked (written "nowhere", every box above them shrunk) or restored by the refit in front of the
        // next frame, like a move -- a model that crosses the residency radius (vk_model.rs:334-345) costs a fraction of a millisecond, not a build; its
        // device arrays stay where they are until the next art_scene_build (288 GB of HBM: the way back is as cheap).
        DevPrim &d = c->h_dev_prims[id];
        d.masked = (d.masked & ~kPrimOut) | (p.enabled ? 0u : kPrimOut);   // (the visibility bits stay)
        as_prim_moved(c, id, true, p.enabled ? -(int64_t)d.n_tri : (int64_t)d.n_tri);   // (ArtStats.num_triangles follows)
        return ART_OK;
    }
    c->built = false;                                            // not part of the built structure: art_scene_build
    return ART_OK;
}

// An alpha cutoff: takes effect at the next art_trace or query without a build -- the value travels in the versioned primitive table, so the next frame
// refits over no batch (as for a disabled primitive) and frames in flight keep the table they were launched with.
int32_t art_scene_set_alpha_cutoff(ArtContext *c, uint32_t id, float cutoff) {
    if (!c) return fail(ART_E_INVALID, "art_scene_set_alpha_cutoff: null context");
    if (id >= c->prims.size()) return fail(ART_E_INVALID, "art_scene_set_alpha_cutoff: no such primitive");
    if (!(cutoff >= 0.0f && cutoff <= 1.0f)) return fail(ART_E_INVALID, "art_scene_set_alpha_cutoff: the cutoff must lie in [0, 1]");   // (NaN too)
    HostPrim &p = c->prims[id];
    if (cutoff == 0.0f) cutoff = 0.0f;   // (-0 is 0: opaque)
    if (p.cutoff == cutoff) return ART_OK;
    const bool was_cut = p.cutoff > 0.0f;
    p.cutoff = cutoff;
    alpha_refresh_live(c);
    if (!c->built || id >= c->h_dev_prims.size()) return ART_OK;   // takes effect with the build
    DevPrim &d = c->h_dev_prims[id];
    d.cutoff = cutoff;
    if (d.n_tri == 0) return ART_OK;                                // no triangles in the structure (a build brings them, with the cutoff)
    as_table_changed(c, cutoff > 0.0f && !was_cut);                 // the next art_trace (or query) writes the next version of the table; a new cutoff's leaves get their bits in front of the refit
    return ART_OK;
}

// A visibility mask: the same path as a cutoff -- the value travels in the versioned primitive table (the complement, in DevPrim::masked), the next
// art_trace or query refits over no batch, frames in flight keep theirs.  Nothing is built.
int32_t art_scene_set_primitive_mask(ArtContext *c, uint32_t id, uint32_t mask) {
    if (!c) return fail(ART_E_INVALID, "art_scene_set_primitive_mask: null context");
    if (id >= c->prims.size()) return fail(ART_E_INVALID, "art_scene_set_primitive_mask: primitive_id: no such primitive");
    if (mask > 0xFFu) return fail(ART_E_INVALID, "art_scene_set_primitive_mask: mask: above 0xFF");
    HostPrim &p = c->prims[id];
    if (p.vis == mask) return ART_OK;
    p.vis = mask;
    alpha_refresh_live(c);
    if (!c->built || id >= c->h_dev_prims.size()) return ART_OK;   // takes effect with the build
    DevPrim &d = c->h_dev_prims[id];
    d.masked = (d.masked & kPrimOut) | ((~mask & 0xFFu) << kPrimVisShift);
    if (d.n_tri == 0) return ART_OK;                                // no triangles in the structure (a build brings them, with the mask)
    as_table_changed(c, mask != 0xFFu);                             // the next art_trace (or query) writes the next version of the table; its leaves get their bits in front of the refit (bits that are there already stay)
    return ART_OK;
}

int32_t art_scene_needs_build(const ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_scene_needs_build: null context");
    return c->built ? 0 : 1;
}

int32_t art_scene_set_model_matrix(ArtContext *c, uint32_t first, uint32_t n, const float model3x4[12]) {
    if (!c || !model3x4) return fail(ART_E_INVALID, "art_scene_set_model_matrix: null argument");
    if (n == 0 || first >= c->prims.size() || n > c->prims.size() - first) return fail(ART_E_INVALID, "art_scene_set_model_matrix: no such primitives");
    for (int i = 0; i < 12; i++) if (!std::isfinite(model3x4[i])) return fail(ART_E_INVALID, "art_scene_set_model_matrix: non-finite matrix");
    float w2o[12];
    affine_inverse(model3x4, w2o);
    for (uint32_t id = first; id < first + n; id++) {
        HostPrim &p = c->prims[id];
        if (std::memcmp(p.o2w, model3x4, 48) == 0) continue;     // where it already is
        std::memcpy(p.o2w, model3x4, 48); std::memcpy(p.w2o, w2o, 48);
        if (!c->built || id >= c->h_dev_prims.size()) continue;  // takes effect with the build
        std::memcpy(c->h_dev_prims[id].o2w, model3x4, 48); std::memcpy(c->h_dev_prims[id].w2o, w2o, 48);
        as_prim_moved(c, id, p.enabled);                         // the next refit is the first to show it; instanced: the next art_trace (or query) refits first
    }
    return ART_OK;
}

int32_t art_scene_set_vertices(ArtContext *c, uint32_t id, const ArtVertex *verts, uint32_t n_verts) {
    if (!c || !verts) return fail(ART_E_INVALID, "art_scene_set_vertices: null argument");
    if (id >= c->prims.size()) return fail(ART_E_INVALID, "art_scene_set_vertices: no such primitive");
    HostPrim &p = c->prims[id];
    if ((size_t)n_verts != p.verts.size()) return fail(ART_E_INVALID, "art_scene_set_vertices: the vertex count differs from the primitive's");
    const bool in_tree = c->built && id < c->h_dev_prims.size() && c->h_dev_prims[id].n_tri > 0;   // its triangles are in the built structure (masked or not)
    if (in_tree) {
        int32_t r = use_device(c); if (r) return r;
        r = as_prim_deformed(c, id, p.enabled); if (r) return r;     // the versions' memory for it (a failure changes nothing); the next refit is the first to show the vertices below
    }
    std::memcpy(p.verts.data(), verts, (size_t)n_verts * sizeof(ArtVertex));
    p.verts_stale = true;                                            // the device's build copy is behind (a rebuild over the same set uploads them again)
    p.verts_behind = false;                                          // (whatever art_scene_set_vertices_device left in the slot is replaced with it)
    return ART_OK;                                                   // (not in the tree: takes effect with the build)
}

// art_scene_set_vertices with the data in device memory ("Vertices from device buffers").  On a primitive of the built structure: one kernel on the caller's
// stream into the primitive's slot of the build's vertex array, ordered on the device (as_ingest); the host copy falls behind (verts_behind) and nothing is staged.
int32_t art_scene_set_vertices_device(ArtContext *c, const ArtVertexUpdate *u) {
    if (!c || !u || !u->verts_dev) return fail(ART_E_INVALID, "art_scene_set_vertices_device: null argument");
    if (u->flags != 0) return fail(ART_E_INVALID, "art_scene_set_vertices_device: flags: must be 0");
    if (u->reserved != 0) return fail(ART_E_INVALID, "art_scene_set_vertices_device: reserved: must be 0");
    if (u->layout != ART_VERTS_FULL && u->layout != ART_VERTS_POSITIONS) return fail(ART_E_INVALID, "art_scene_set_vertices_device: layout: neither ART_VERTS_FULL nor ART_VERTS_POSITIONS");
    const bool full = u->layout == ART_VERTS_FULL;
    if (full ? (u->stride_bytes != 0 && u->stride_bytes != 48) : (u->stride_bytes != 0 && (u->stride_bytes < 12 || u->stride_bytes % 4 != 0)))
        return fail(ART_E_INVALID, full ? "art_scene_set_vertices_device: stride_bytes: 0 or 48 for ART_VERTS_FULL" : "art_scene_set_vertices_device: stride_bytes: 0, or at least 12 and a multiple of 4, for ART_VERTS_POSITIONS");
    if ((uintptr_t)u->verts_dev % (full ? 16 : 4) != 0) return fail(ART_E_INVALID, full ? "art_scene_set_vertices_device: verts_dev: not 16-byte aligned" : "art_scene_set_vertices_device: verts_dev: not 4-byte aligned");
    const uint32_t id = u->primitive_id;
    if (id >= c->prims.size()) return fail(ART_E_INVALID, "art_scene_set_vertices_device: no such primitive");
    HostPrim &p = c->prims[id];
    if ((size_t)u->n_verts != p.verts.size()) return fail(ART_E_INVALID, "art_scene_set_vertices_device: the vertex count differs from the primitive's");
    if (hipError_t e = hipSetDevice(c->device); e != hipSuccess) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { (void)hipGetLastError(); return fail(ART_E_NO_DEVICE, "art_scene_set_vertices_device: no HIP device to read verts_dev with"); }
        return hipfail(e, "art_scene_set_vertices_device: hipSetDevice");
    }
    const uint32_t stride = full ? 0u : (u->stride_bytes ? u->stride_bytes : 12u);
    hipStream_t s = u->hip_stream ? (hipStream_t)u->hip_stream : c->main_stream();
    if (s == hipStreamLegacy) s = nullptr;   // the null stream by its own handle: an event is recorded there that the refit streams wait for, and the runtime takes the stream an event was recorded on for a pointer
    const bool in_tree = c->built && id < c->h_dev_prims.size() && c->h_dev_prims[id].n_tri > 0;   // its triangles are in the built structure (masked or not): it has a slot
    if (in_tree) {
        int32_t r = as_prim_deformed(c, id, p.enabled, false); if (r) return r;   // the versions' shading records (a failure changes nothing); the next refit is the first to show the vertices
        // POSITIONS keeps the CURRENT attributes: a slot that is behind the host copy (a host-form call since the build) gets that copy first
        r = as_ingest(c, id, u->verts_dev, stride, !full && p.verts_stale ? p.verts.data() : nullptr, s); if (r) return r;
        p.verts_stale = false; p.verts_behind = true;
        return ART_OK;
    }
    // not in the tree (added since the build, disabled at the build, no built scene): no slot.  The host copy takes the vertices, synchronously; they show with the next build
    int32_t r = verts_read_back(c, id); if (r) return r;   // (a slot from before the scene fell out of date may still be ahead: POSITIONS merges into the current attributes)
    if (full) HIPC(hipMemcpyAsync(p.verts.data(), u->verts_dev, p.verts.size() * sizeof(ArtVertex), hipMemcpyDeviceToHost, s));
    std::vector<float> pos(full ? 0 : p.verts.size() * 3);
    if (!full) HIPC(hipMemcpy2DAsync(pos.data(), 12, u->verts_dev, stride, 12, p.verts.size(), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    as_ingest_counts(c, 1, 0);
    for (size_t i = 0; i < pos.size() / 3; i++) std::memcpy(&p.verts[i], &pos[3 * i], 12);
    p.verts_stale = true;
    return ART_OK;
}

int32_t art_scene_get_vertices(ArtContext *c, uint32_t id, ArtVertex *dst, uint32_t n_verts) {
    if (!c || !dst) return fail(ART_E_INVALID, "art_scene_get_vertices: null argument");
    if (id >= c->prims.size()) return fail(ART_E_INVALID, "art_scene_get_vertices: no such primitive");
    HostPrim &p = c->prims[id];
    if ((size_t)n_verts != p.verts.size()) return fail(ART_E_INVALID, "art_scene_get_vertices: the vertex count differs from the primitive's");
    if (p.verts_behind) { int32_t r = use_device(c); if (r) return r; r = verts_read_back(c, id); if (r) return r; }
    std::memcpy(dst, p.verts.data(), (size_t)n_verts * sizeof(ArtVertex));
    return ART_OK;
}

int32_t art_vertex_update_counts(ArtContext *c, uint64_t *ingests, uint64_t *host_syncs, uint64_t *readbacks) {
    if (!c) return fail(ART_E_INVALID, "art_vertex_update_counts: null context");
    if (ingests) *ingests = c->ver.ingests;
    if (host_syncs) *host_syncs = c->ver.ingest_host_syncs;
    if (readbacks) *readbacks = c->ver.ingest_readbacks;
    return ART_OK;
}

int32_t art_scene_build(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_scene_build: null context");
    if (c->prims.empty()) return fail(ART_E_STATE, "art_scene_build: no primitives");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    as_scene_reset(c); // the versions were copies of the tree that goes away
    c->bvh = Lbvh{}; c->bvh.arena = &c->arena; c->built = false; drop_graphs(c);
    // Only enabled primitives are uploaded and instanced (get_acceleration_structure_instance returns None unless the model is in
    // the Device state, vk_model.rs:360-372).  Ids keep their meaning: a disabled primitive stays in the table with zero triangles.
    // With nothing enabled the tree is one zero-area triangle that no ray can hit (an empty TLAS: every ray misses).
    static const ArtVertex kNoVertex{};
    static const uint16_t kNoIndex[3] = {0, 0, 0};
    static const uint8_t kNoTexel[12] = {0};
    bool any = false;
    for (auto &p : c->prims) any = any || (p.enabled && p.n_indices >= 3);
    size_t nv = any ? 0 : 1, ib = any ? 0 : 16, nt = any ? 0 : 3; uint32_t T = 0;
    for (auto &p : c->prims) if (p.enabled) { nv += p.verts.size(); ib += (p.indices.size() + 15) & ~(size_t)15; nt += (size_t)3 * p.tw * p.th; }
    std::vector<uint8_t> now_set(c->prims.size());
    for (size_t k = 0; k < c->prims.size(); k++) now_set[k] = c->prims[k].enabled ? 1 : 0;
    const bool resident = any && now_set == c->uploaded;   // the same primitives as the last upload, nothing added since: their data is where this build would put it
    if (!resident) {   // the arrays are laid out again from the host copies: those that art_scene_set_vertices_device left behind their slots are read back first
        for (size_t k = 0; k < c->prims.size() && k < c->h_dev_prims.size(); k++) { r = verts_read_back(c, (uint32_t)k); if (r) return r; }
        c->uploaded.clear();   // (an upload that fails half way leaves nothing to rely on)
    }
    HIPC(c->d_verts.ensure(nv * 12)); HIPC(c->d_indices.ensure(ib)); HIPC(c->d_tex.ensure(nt));
    std::vector<DevPrim> dp(c->prims.size() + (any ? 0 : 1));
    std::vector<uint32_t> first(dp.size());
    size_t ov = 0, oi = 0, ot = 0;
    for (size_t k = 0; k < c->prims.size(); k++) {
        auto &p = c->prims[k];
        DevPrim &d = dp[k];
        std::memset(&d, 0, sizeof(d));
        d.vertices = c->d_verts.p + ov * 12; d.indices = c->d_indices.p + oi; d.texture_offset = (uint32_t)ot; d.single_index_size = p.idx_bytes;
        d.tw = p.tw; d.th = p.th; d.first_tri = T; d.n_tri = p.enabled ? p.n_indices / 3 : 0; d.cutoff = p.cutoff; d.masked = (~p.vis & 0xFFu) << kPrimVisShift;
        std::memcpy(d.o2w, p.o2w, 48); std::memcpy(d.w2o, p.w2o, 48);
        first[k] = T;
        if (!p.enabled) continue;
        if (!resident || p.verts_stale) HIPC(hipMemcpy(c->d_verts.p + ov * 12, p.verts.data(), p.verts.size() * 48, hipMemcpyHostToDevice));   // (deformed since: art_scene_set_vertices)
        p.verts_stale = false;
        if (!resident) {
            HIPC(hipMemcpy(c->d_indices.p + oi, p.indices.data(), p.indices.size(), hipMemcpyHostToDevice));
            HIPC(hipMemcpy(c->d_tex.p + ot, p.tex.data(), p.tex.size(), hipMemcpyHostToDevice));
        }
        T += d.n_tri;
        ov += p.verts.size(); oi += (p.indices.size() + 15) & ~(size_t)15; ot += (size_t)3 * p.tw * p.th;
    }
    if (!any) {
        DevPrim &d = dp.back();
        std::memset(&d, 0, sizeof(d));
        HIPC(hipMemcpy(c->d_verts.p, &kNoVertex, 48, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(c->d_indices.p, kNoIndex, 6, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(c->d_tex.p, kNoTexel, 12, hipMemcpyHostToDevice));
        d.vertices = c->d_verts.p; d.indices = c->d_indices.p; d.texture_offset = 0; d.single_index_size = 2; d.tw = 1; d.th = 1; d.first_tri = T; d.n_tri = 1;
        d.o2w[0] = d.o2w[5] = d.o2w[10] = 1.0f; d.w2o[0] = d.w2o[5] = d.w2o[10] = 1.0f;
        first.back() = T;
        T += 1;
    }
    HIPC(c->d_prims.ensure(dp.size())); HIPC(c->d_first_tri.ensure(first.size()));
    HIPC(hipMemcpy(c->d_prims.p, dp.data(), dp.size() * sizeof(DevPrim), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(c->d_first_tri.p, first.data(), first.size() * 4, hipMemcpyHostToDevice));
    c->uploaded = any ? now_set : std::vector<uint8_t>();
    c->h_first_tri = first;
    c->h_dev_prims = dp;
    c->T = T;
    BuildInputs in{c->d_prims.p, (uint32_t)dp.size(), c->d_first_tri.p, T, c->cfg.morton_bits};
    Event e0, e1;
    HIPC(e0.create()); HIPC(e1.create());
    HIPC(hipEventRecord(e0, c->main_stream()));
    const bool own_tree = c->fast_trace && T >= 3;   // a PREFER_FAST_TRACE build makes its own tree over the leaves: the canonical tree's boxes are computed only when asked for (art_get_lbvh)
    hipError_t e = lbvh_build(in, c->bvh, c->main_stream(), !own_tree);
    c->bvh.log = c->tuning.log;
    if (e != hipSuccess) return hipfail(e, "lbvh_build");
    if (c->fast_trace) { // PREFER_FAST_TRACE (vk_model.rs:968): the traversal nodes get a SAH-driven topology over the same leaves
        bool done = false;
        if (c->tree_builder == 3) { // the binned SAH on the device
            e = sah_build_device(c->bvh, T, c->main_stream());
            if (e != hipSuccess) return hipfail(e, "sah_build_device");
            done = true;
        }
        if (!done) {
            e = sah_build(c->bvh, T, c->main_stream());
            if (e != hipSuccess) return hipfail(e, "sah_build");
        }
    }
    HIPC(hipEventRecord(e1, c->main_stream())); HIPC(hipEventSynchronize(e1));
    float ms = 0; HIPC(hipEventElapsedTime(&ms, e0, e1));
    c->stats.build_ms = ms; c->stats.num_triangles = T; c->stats.num_primitives = (uint32_t)dp.size(); c->stats.num_nodes = c->kind_primary == 4 ? c->bvh.n_wide : (T > 1 ? T - 1 : 1);
    {   // the leaf bits of the alpha test, from zero (on the first stream, then waited for: the frames run on every ring slot's stream)
        const size_t nw = ((size_t)T + 31) / 32;
        HIPC(c->d_alpha_bits.ensure(nw + 1));
        HIPC(hipMemsetAsync(c->d_alpha_bits.p, 0, (nw + 1) * 4, c->main_stream()));
        bool cut = false;
        for (const DevPrim &d : dp) cut = cut || (d.n_tri > 0 && (d.cutoff > 0.0f || (d.masked >> kPrimVisShift) != 0u));
        if (cut) { launch_alpha_bits(T, c->bvh.leaf_gid, c->bvh.tri_prim, c->d_prims.p, c->d_alpha_bits.p, c->main_stream()); HIPC(hipGetLastError()); }
        // the shadow-occluder hints are leaf positions of the tree that just went away: all empty (nothing is in flight -- sync_all above -- and the wait below is in front of every later frame)
        if (c->d_hints.p) HIPC(hipMemsetAsync(c->d_hints.p, 0xFF, c->d_hints.n * 4, c->main_stream()));
        HIPC(hipStreamSynchronize(c->main_stream()));
        alpha_refresh_live(c);
    }
    c->built = true;
    plan_hint_built(c);
    return as_scene_built(c);   // the ring's records of the new table; the ring itself now if the host said its models move
}

int32_t art_get_lbvh(ArtContext *c, uint32_t *leaf_gid, uint64_t *keys, int32_t *child, float *node_lo, float *node_hi, float *leaf_lo, float *leaf_hi) {
    if (!c) return fail(ART_E_INVALID, "art_get_lbvh: null context");
    if (!c->built) return fail(ART_E_STATE, "art_get_lbvh: scene not built");
    int32_t r = use_device(c); if (r) return r;
    r = refresh_now(c); if (r) return r;       // after a move: the boxes of where the models are now (the keys and the topology are the build's)
    if (!c->bvh.canon_boxes) binary_mark(c, false);     // the build left the canonical tree's boxes for now: have them made
    r = ensure_binary(c, true); if (r) return r;
    size_t T = c->T, NI = T > 1 ? T - 1 : 0;
    if (leaf_gid) HIPC(hipMemcpy(leaf_gid, c->bvh.leaf_gid, T * 4, hipMemcpyDeviceToHost));
    if (keys) HIPC(hipMemcpy(keys, c->bvh.keys, T * 8, hipMemcpyDeviceToHost));
    if (child && NI) HIPC(hipMemcpy(child, c->bvh.child, NI * 8, hipMemcpyDeviceToHost));
    if (node_lo && NI) HIPC(hipMemcpy(node_lo, c->bvh.node_lo, NI * 12, hipMemcpyDeviceToHost));
    if (node_hi && NI) HIPC(hipMemcpy(node_hi, c->bvh.node_hi, NI * 12, hipMemcpyDeviceToHost));
    if (leaf_lo) HIPC(hipMemcpy(leaf_lo, c->bvh.leaf_lo, T * 12, hipMemcpyDeviceToHost));
    if (leaf_hi) HIPC(hipMemcpy(leaf_hi, c->bvh.leaf_hi, T * 12, hipMemcpyDeviceToHost));
    return ART_OK;
}

// the tree the walks actually use: the SAH topology when it was built (default), else the canonical one; leaves are those of art_get_lbvh
int32_t art_get_traversal_tree(ArtContext *c, int32_t *child, float *node_lo, float *node_hi) {
    if (!c) return fail(ART_E_INVALID, "art_get_traversal_tree: null context");
    if (!c->built) return fail(ART_E_STATE, "art_get_traversal_tree: scene not built");
    int32_t r = use_device(c); if (r) return r;
    r = refresh_now(c); if (r) return r;
    r = ensure_binary(c, true); if (r) return r;
    size_t T = c->T, NI = T > 1 ? T - 1 : 0;
    const bool sah = c->bvh.trav_child != nullptr;
    if (child && NI) HIPC(hipMemcpy(child, sah ? c->bvh.trav_child : c->bvh.child, NI * 8, hipMemcpyDeviceToHost));
    if (node_lo && NI) HIPC(hipMemcpy(node_lo, sah ? c->bvh.trav_lo : c->bvh.node_lo, NI * 12, hipMemcpyDeviceToHost));
    if (node_hi && NI) HIPC(hipMemcpy(node_hi, sah ? c->bvh.trav_hi : c->bvh.node_hi, NI * 12, hipMemcpyDeviceToHost));
    return ART_OK;
}

// the 4-wide collapse of that tree, as the walks read it: n_nodes records of 64 B (quantised, per-ray walks) and of 128 B (float boxes, packet walks).
// Builds it if no walk has needed it yet.  Either pointer may be NULL; *n_nodes is always set.
int32_t art_get_wide_nodes(ArtContext *c, void *quantised, void *floats, size_t capacity_nodes, uint32_t *n_nodes) {
    if (!c || !n_nodes) return fail(ART_E_INVALID, "art_get_wide_nodes: null argument");
    if (!c->built) return fail(ART_E_STATE, "art_get_wide_nodes: scene not built");
    int32_t r = use_device(c); if (r) return r;
    r = refresh_now(c); if (r) return r;
    r = ensure_wide(c, true); if (r) return r;
    *n_nodes = c->bvh.n_wide;
    if ((quantised || floats) && capacity_nodes < c->bvh.n_wide) return fail(ART_E_INVALID, "art_get_wide_nodes: buffers too small");
    const AsPtrs as = as_ptrs(c, as_current(c));   // the version the next frame would read
    if (quantised) HIPC(hipMemcpy(quantised, as.wide, (size_t)c->bvh.n_wide * sizeof(DevNode4), hipMemcpyDeviceToHost));
    if (floats) HIPC(hipMemcpy(floats, as.widef, (size_t)c->bvh.n_wide * sizeof(DevNodeW), hipMemcpyDeviceToHost));
    return ART_OK;
}

} // extern "C"
