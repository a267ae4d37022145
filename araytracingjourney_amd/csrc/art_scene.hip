// art_scene.hip -- the scene behind include/art.h: the primitive table and its setters, art_scene_build, the ring of versions of the acceleration structure (refit,
// deformation), the trees the non-default walks read on demand, and the tree read-outs of the parity surface.  Host code only; the kernels are art_build.hip's (LBVH), art_wide.hip's (4-wide collapse) and art_refit.hip's (refit).
#include "art_context.h"
#include <chrono>
#include <cmath>
#include <cstdio>
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

// ---- versions of the acceleration structure (moving models) ------------------------------------------------------------------------------
AsPtrs art::as_ptrs(const ArtContext *c, uint32_t v) {
    if (c->as.empty()) return AsPtrs{c->bvh.tris, c->bvh.widef, c->bvh.wide, c->d_prims.p, c->bvh.shade_tris};
    const AsVersion &V = c->as[v];
    return AsPtrs{V.tris, V.widef, V.wide, V.prims, V.shade};
}
static uint64_t as_epoch_of(const ArtContext *c, uint32_t v) { return c->as.empty() ? 0 : c->as[v].epoch; }
// everything that reads them has finished (the caller synchronised)
void art::as_release(ArtContext *c) {
    c->as.clear(); c->as_cur = 0;   // (their events) -- then the blocks they pointed into: device arrays, staging memory, shading records, staging of replaced vertices
    c->as_block.release(); c->as_pinned.release(); c->shade_block.release(); c->stage_block.release(); c->stage_pinned.release();
    c->deform_verts = 0; std::fill(c->deform_off.begin(), c->deform_off.end(), (int64_t)-1);
}
// the first move of a built scene: the ring of versions (ArtTuning.as_versions; default 4: one more than the reference's frames in flight, renderer.rs:135 -- measured on
// config 2 with a model of 164 k triangles moving every frame, 16 ring slots: 0.70 / 0.38 / 0.28 / 0.25 / 0.26 ms per frame with 1 / 2 / 3 / 4 / 8 versions), every one a copy of
// the build's arrays -- the topology (child references, valid masks, sort axes) is never written again -- and the cost of the tree as built
static int32_t as_create(ArtContext *c) {
    int32_t r = ensure_wide(c, true); if (r) return r;
    r = sync_all(c); if (r) return r;
    const auto t_begin = std::chrono::steady_clock::now();
    // (default: twice the frames in flight, 4 at least and 24 at most.  The host may issue the refit of frame n once the frames that read that version -- frame n - K -- are
    //  over, so K sets how far it runs ahead of the GPU: with K = F + 1 a refit is issued when its ring slot's previous frame has all but finished and its latency -- 0.5 ms
    //  among eight frames in flight -- stands in front of the slot's next frame; with K = 2 F it is a ring trip ahead.  Config 2, F = 8, a model of 164 k triangles moving
    //  every frame: 0.252 / 0.229 / 0.213 / 0.210 / 0.205 / 0.205 ms a frame with 4 / 8 / 10 / 12 / 16 / 24 versions (profiles/README.md round 4d); a version is the tree's
    //  arrays once more: 42 MB for config 2, 450 MB for config 4.)
    const uint32_t K = c->tuning.as_versions ? std::min(c->tuning.as_versions, kMaxAsVersions) : std::min(std::max(2u * c->F, 4u), kMaxAsVersions);
    const size_t np = c->h_dev_prims.size(), T = c->T, NW = c->bvh.n_wide;
    c->as.clear(); c->as.resize(K);
    hipStream_t s = c->main_stream();
    double t_sec[6] = {0, 0, 0, 0, 0, 0};
    auto lap = [&, last = std::chrono::steady_clock::now()](int i) mutable { const auto n = std::chrono::steady_clock::now(); t_sec[i] += std::chrono::duration<double, std::milli>(n - last).count(); last = n; };
    auto body = [&]() -> int32_t {
        const uint32_t want = c->tuning.refit_streams == 0xFFFFFFFFu ? 0u : (c->tuning.refit_streams ? std::min(c->tuning.refit_streams, 4u) : std::min(c->F, 4u));
        while (c->n_refit_streams < want) {   // (kept for the life of the context)
            int lo = 0, hi = 0; HIPC(hipDeviceGetStreamPriorityRange(&lo, &hi));   // hi: the numerically smallest = the most urgent: a refit is a handful of small launches a whole frame waits for
            HIPC(c->refit_stream[c->n_refit_streams].create(hi)); c->n_refit_streams++;
        }
        while (c->n_refit_streams > want) c->refit_stream[--c->n_refit_streams].release();   // (waits for it first)
        lap(0);
        if (!c->bvh.sub_off) { // the parents in the 4-wide tree and the refit's work lists (a workgroup per batch of subtrees): all there or none (refit_lists_build)
            hipError_t e = refit_lists_build(c->bvh, c->T, s);
            if (e != hipSuccess) return hipfail(e, "refit_lists_build");
        }
        lap(1);
        // one device block and one pinned block, carved per version (256-byte steps)
        auto pad = [](size_t n) { return (n + 255) & ~(size_t)255; };
        const size_t nbat = c->bvh.sub_batches ? c->bvh.sub_batches : 1;
        const size_t dev_owned = pad(T * sizeof(DevTri)) + pad(NW * sizeof(DevNodeW)) + pad(NW * sizeof(DevNode4)) + pad(np * sizeof(DevPrim)), dev_every = pad(NW * 4) + pad(32) + pad(nbat * 8);
        const size_t pin_every = pad(np * sizeof(DevPrim)) + pad(np) + pad(32) + pad(nbat * 4);
        HIPC(c->as_block.ensure((K - 1) * dev_owned + K * dev_every));
        HIPC(c->as_pinned.ensure(K * pin_every));
        lap(2);
        char *dp = c->as_block.p, *hp = c->as_pinned.p, *dhp = c->as_pinned.d;
        auto carve = [&](char *&p, size_t n) { char *q = p; p += pad(n); return q; };
        for (uint32_t v = 0; v < K; v++) { // (everything on the context's first stream, asynchronously: one wait at the end)
            AsVersion &V = c->as[v];
            V.shade = c->bvh.shade_tris;   // (every version's own copy only once a built primitive is deformed: deform_prepare)
            if (v == 0) { V.tris = c->bvh.tris; V.widef = c->bvh.widef; V.wide = c->bvh.wide; V.prims = c->d_prims.p; }
            else {
                V.owned = true;
                V.tris = (DevTri *)carve(dp, T * sizeof(DevTri)); V.widef = (DevNodeW *)carve(dp, NW * sizeof(DevNodeW)); V.wide = (DevNode4 *)carve(dp, NW * sizeof(DevNode4)); V.prims = (DevPrim *)carve(dp, np * sizeof(DevPrim));
                HIPC(hipMemcpyAsync(V.tris, c->bvh.tris, T * sizeof(DevTri), hipMemcpyDeviceToDevice, s)); HIPC(hipMemcpyAsync(V.widef, c->bvh.widef, NW * sizeof(DevNodeW), hipMemcpyDeviceToDevice, s));
                HIPC(hipMemcpyAsync(V.wide, c->bvh.wide, NW * sizeof(DevNode4), hipMemcpyDeviceToDevice, s)); HIPC(hipMemcpyAsync(V.prims, c->d_prims.p, np * sizeof(DevPrim), hipMemcpyDeviceToDevice, s));
            }
            V.mark = (uint32_t *)carve(dp, NW * 4); V.acc = (double *)carve(dp, 32); V.batch_cost = (double *)carve(dp, nbat * 8);
            HIPC(hipMemsetAsync(V.mark, 0, NW * 4, s)); HIPC(hipMemsetAsync(V.acc, 0, 32, s));
            const size_t off = (size_t)(hp - c->as_pinned.p);
            V.h_prims = (DevPrim *)carve(hp, np * sizeof(DevPrim)); V.h_touched = (uint8_t *)carve(hp, np); V.h_result = (double *)carve(hp, 32);
            V.dh_prims = (DevPrim *)(dhp + off); V.dh_touched = (uint8_t *)(dhp + off + pad(np * sizeof(DevPrim))); V.dh_result = (double *)(dhp + off + pad(np * sizeof(DevPrim)) + pad(np));
            V.h_dirty = (uint32_t *)carve(hp, nbat * 4); V.dh_dirty = (uint32_t *)(dhp + off + pad(np * sizeof(DevPrim)) + pad(np) + pad(32));
            HIPC(V.ready.create(hipEventDisableTiming));
        }
        lap(3);
        AsVersion &V0 = c->as[0];
        launch_wide_cost(c->bvh.n_wide, V0.widef, nullptr, V0.acc, V0.dh_result, s);   // the cost of the tree as built
        HIPC(hipGetLastError()); HIPC(hipStreamSynchronize(s));
        c->as_cost0 = V0.h_result[0]; c->refit_cost_ratio = 1.0f;
        lap(4);
        if (c->tuning.log & 1u) std::fprintf(stderr, "[art] versions: %u of them; refit streams %.2f ms, parents + work lists %.2f, the two allocations %.2f, copies issued + events %.2f, the wait for them + the cost of the tree as built %.2f\n", K, t_sec[0], t_sec[1], t_sec[2], t_sec[3], t_sec[4]);
        return ART_OK;
    };
    r = body();
    if (r) as_release(c);
    c->versions_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return r;
}
// the surface-area cost of the latest refit travels to the host behind it; once it has arrived it is what ArtStats.refit_cost_ratio and the rebuild rule go by
void art::harvest_cost(ArtContext *c) {
    if (c->as.empty()) return;
    AsVersion &L = c->as[c->as_cur];
    if (!L.result_pending || hipEventQuery(L.ready) != hipSuccess) return;
    L.result_pending = false; L.ready_known = true;
    if (c->as_cost0 > 0.0) c->refit_cost_ratio = (float)(L.h_result[0] / c->as_cost0);
    const unsigned long long *st = reinterpret_cast<const unsigned long long *>(L.h_result);
    c->last_refit_ms = (float)((double)(st[3] - st[2]) * 1e-5);   // wall_clock64: 100 MHz
}
int32_t art::as_wait_ready(ArtContext *c, uint32_t v, hipStream_t stream, uint32_t own_slot) {
    if (c->as.empty()) return ART_OK;
    AsVersion &V = c->as[v];
    if (V.ready_known) return ART_OK;
    if (hipEventQuery(V.ready) == hipSuccess) { V.ready_known = true; return ART_OK; }
    if (own_slot == ~0u) (void)hipGetLastError();    // (no launch check of a frame follows: the not-ready answer is not left behind)
    else if (V.ready_slot == own_slot) return ART_OK;   // the refit is in front of the launch on this very stream
    HIPC(hipStreamWaitEvent(stream, V.ready, 0));      // nothing on the host
    return ART_OK;
}
// A model moved since the last launch: bring the NEXT version of the structure up to date on stream s, the stream of ring slot k whose frame is about to be
// launched -- the frame is ordered behind the refit by the stream, frames on other streams by V.ready (art_trace).  Frames still reading the version about to be
// written are waited for on the host, like the reference's per-frame fence (renderer.rs:451-466).
// What the stream sees: three launches and one event record (round 3: two uploads, a launch per tree level, a clear, the cost's read-back and four event records --
// twenty operations, 0.3 ms of issue in front of a 0.1 ms refit).
// (k = ~0u: in front of a cast, s a stream of the context that no frame runs on: every ring slot's frames are waited for, every later launch waits for V.ready)
int32_t art::scene_refresh(ArtContext *c, uint32_t k, hipStream_t s) {
    if (!c->xform_dirty) return ART_OK;
    int32_t r;
    if (c->as.empty()) { // (a host that announced its moves with ART_FLAG_DYNAMIC_SCENE paid this in art_scene_build)
        const auto t_begin = std::chrono::steady_clock::now();
        r = as_create(c); if (r) return r;
        c->first_move_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    {   // the cost of the latest refit, if it has arrived: past the threshold the tree is built again for where the models are now
        harvest_cost(c);
        const float thr = c->tuning.refit_rebuild_ratio > 0.0f ? c->tuning.refit_rebuild_ratio : (c->tuning.refit_rebuild_ratio < 0.0f ? INFINITY : 2.0f);
        if (c->refit_cost_ratio > thr) {
            if (c->tuning.log & 1u) std::fprintf(stderr, "[art] refit cost %.2f x the build's: building again\n", c->refit_cost_ratio);
            r = art_scene_build(c); // (synchronises, uploads the primitives with their current matrices, drops the versions)
            if (r == ART_OK) c->rebuilds++;
            return r;
        }
    }
    const uint32_t K = (uint32_t)c->as.size(), next = (c->as_cur + 1) % K;
    AsVersion &V = c->as[next];
    const bool beside = c->n_refit_streams != 0;   // the refit runs beside the slot's frames, on a stream of its own
    if (beside) s = c->refit_stream[k % c->n_refit_streams];
    for (uint32_t j = 0; j < c->F; j++) {
        if (j != k || beside) { // (on the frame's own stream ring slot k's earlier work is ordered before the refit by that stream)
            if (V.aux[j]) HIPC(hipStreamSynchronize(c->stream_of(j)));
            else if (V.used[j]) {
                const uint64_t f = V.used[j] - 1;
                if (c->frame_no - f <= (uint64_t)ArtContext::kRing) HIPC(hipEventSynchronize(c->ev[f % ArtContext::kRing][4])); else HIPC(hipStreamSynchronize(c->stream_of(j)));
            }
        }
        V.used[j] = 0; V.aux[j] = false;
    }
    r = cast_wait_version(c, next); if (r) return r;   // casts still reading it (art_cast_rays: a cast holds the version it was launched on): the same wait, counted
    // the staging memory below is read by the kernels of the refit that wrote this version last: that refit has to be over before the host writes it again (it is, whenever the
    // frames above were waited for -- they ran behind it -- but nothing else says so: a version no frame ever read, a ring slot that skipped its turn)
    if (!V.ready_known) { HIPC(hipEventSynchronize(V.ready)); V.ready_known = true; }
    V.result_pending = false;
    if (c->graph_mode) drop_graphs(c); // a captured frame holds the old version's pointers
    const size_t np = c->h_dev_prims.size();
    std::memcpy(V.h_prims, c->h_dev_prims.data(), np * sizeof(DevPrim));
    for (size_t p = 0; p < np; p++) V.h_touched[p] = (p < c->prim_moved.size() && c->prim_moved[p] > V.epoch) ? 1 : 0;   // what moved since THIS version was written (it may be several refits behind)
    {   // what was deformed since this version was written: its current vertices into the version's staging (pinned, then ONE copy a run of slots on the refit's stream, in
        // front of the refit that reads them from device memory), its table entry pointed there, and its shading records gathered again by the refit's leaf stage
        size_t run_lo = 0, run_hi = 0;   // the run of staging slots the next copy covers (vertices)
        auto flush = [&]() -> int32_t {
            if (run_hi > run_lo) HIPC(hipMemcpyAsync(V.d_stage + run_lo * 12, V.h_stage + run_lo, (run_hi - run_lo) * sizeof(ArtVertex), hipMemcpyHostToDevice, s));
            run_lo = run_hi = 0; return ART_OK;
        };
        for (size_t p = 0; p < np && p < c->prim_deformed.size(); p++) {
            if (c->prim_deformed[p] <= V.epoch) continue;
            const std::vector<ArtVertex> &vv = c->prims[p].verts;
            const size_t off = (size_t)c->deform_off[p];
            std::memcpy(V.h_stage + off, vv.data(), vv.size() * sizeof(ArtVertex));
            V.h_prims[p].vertices = V.d_stage + off * 12;
            V.h_touched[p] |= kTouchRegather;
            if (off != run_hi) { r = flush(); if (r) return r; run_lo = off; }
            run_hi = off + vv.size();
        }
        r = flush(); if (r) return r;
    }
    RefitArgs ra{};
    ra.T = c->T; ra.n_wide = c->bvh.n_wide; ra.n_prims = (uint32_t)np; ra.shade = V.shade; ra.prims_host = V.dh_prims; ra.prims_dev = V.prims; ra.touched = V.dh_touched;
    ra.sub_nodes = c->bvh.sub_nodes; ra.sub_leaves = c->bvh.sub_leaves; ra.sub_off = c->bvh.sub_off; ra.sub_batches = c->bvh.sub_batches; ra.sub_levels = c->bvh.sub_levels;
    ra.leaf_parent = c->bvh.leaf_parent; ra.node_parent = c->bvh.node_parent; ra.mark = V.mark; ra.tris = V.tris; ra.wide = V.wide; ra.widef = V.widef; ra.acc = V.acc; ra.result = V.dh_result;
    {   // the batches that hold a primitive that moved (since this version was written); the others keep their triangles, their boxes and -- in a large tree -- their
        // cached share of the cost, which a version's first refit makes for all of them
        const std::vector<uint32_t> &po = c->bvh.batch_prim_off, &pi = c->bvh.batch_prim_ids;
        ra.fold = c->bvh.n_wide >= (c->tuning.refit_fold_nodes ? c->tuning.refit_fold_nodes : kFoldRequantNodes);
        const bool all = po.size() != (size_t)c->bvh.sub_batches + 1 || (ra.fold && !V.cost_cached);
        uint32_t nd = 0;
        if (!all) for (uint32_t b = 0; b < c->bvh.sub_batches; b++) {
            bool hit = false;
            for (uint32_t i = po[b]; i < po[b + 1] && !hit; i++) hit = pi[i] < np && V.h_touched[pi[i]] != 0;
            if (hit) V.h_dirty[nd++] = b;
        }
        ra.dirty = all ? nullptr : V.dh_dirty; ra.n_dirty = nd; ra.batch_cost = V.batch_cost;
        if (all) V.cost_cached = true;
    }
    if (c->alpha_bits_stale) {   // a primitive got a cutoff: its leaves' bits, from this version's table, in front of the refit whose event the frames wait for
        launch_alpha_bits(c->T, c->bvh.leaf_gid, c->bvh.tri_prim, V.dh_prims, c->d_alpha_bits.p, s);
        c->alpha_bits_stale = false;
    }
    launch_refit(ra, s);
    HIPC(hipEventRecord(V.ready, s)); V.ready_known = false; V.ready_slot = beside ? ~0u : k; V.result_pending = true;   // (~0: no frame stream is behind it by itself)
    HIPC(hipGetLastError());
    c->as_cur = next; V.epoch = ++c->as_epoch; c->xform_dirty = false; c->refits++;
    return ART_OK;
}
// for the calls that read the structure outside a frame (queries, the parity surface): nothing in flight, the pending move applied
static int32_t refresh_now(ArtContext *c) {
    int32_t r = sync_all(c); if (r) return r;
    if (!c->xform_dirty) return ART_OK;
    r = scene_refresh(c, 0, c->stream_of(0)); if (r) return r;
    r = sync_all(c); if (r) return r;   // (the refit may have run on a stream of its own)
    if (!c->as.empty()) c->as[c->as_cur].ready_known = true;
    return ART_OK;
}
// the binary trees and the 64-byte node records follow the versions on demand only (the non-default walks and the parity surface read them): they are
// not versioned, so this waits for everything in flight
int32_t art::ensure_binary(ArtContext *c, bool needed) {
    if (!needed || c->binary_epoch == as_epoch_of(c, c->as_cur)) return ART_OK;
    int32_t r = sync_all(c); if (r) return r;
    hipError_t e = binary_refit(c->bvh, c->T, as_ptrs(c, c->as_cur).tris, c->main_stream());
    if (e != hipSuccess) return hipfail(e, "binary_refit");
    c->binary_epoch = as_epoch_of(c, c->as_cur);
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
        c->masked_tris += p.enabled ? -(int64_t)d.n_tri : (int64_t)d.n_tri;
        c->prim_moved[id] = c->as_epoch + 1;
        c->xform_dirty = true;
        c->stats.num_triangles = (uint32_t)((int64_t)c->T - c->masked_tris);
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
    if (cutoff > 0.0f && !was_cut) c->alpha_bits_stale = true;      // its leaves get their bits in front of the refit
    c->xform_dirty = true;                                          // the next art_trace (or query) writes the next version of the table
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
    if (mask != 0xFFu) c->alpha_bits_stale = true;                  // its leaves get their bits in front of the refit (bits that are there already stay)
    c->xform_dirty = true;                                          // the next art_trace (or query) writes the next version of the table
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
        if (id < c->prim_moved.size()) c->prim_moved[id] = c->as_epoch + 1;   // the next refit is the first to show it
        if (p.enabled) c->xform_dirty = true;                    // instanced: the next art_trace (or query) refits first
    }
    return ART_OK;
}

// The first deformation of a built primitive (art_scene_set_vertices): every version gets shading records of its own (a frame in flight must keep the normals it was
// launched with), and the primitive a slot in every version's staging.  One synchronisation, here and never in front of a frame: an allocation that fails
// comes back from the call that asked for it, with nothing changed.
static int32_t deform_prepare(ArtContext *c, uint32_t id) {
    const uint32_t K = (uint32_t)c->as.size();
    const bool need_shade = K > 1 && !c->shade_block, need_stage = c->deform_off[id] < 0;
    if (!need_shade && !need_stage) return ART_OK;   // (the steady state)
    int32_t r = sync_all(c); if (r) return r;
    auto pad = [](size_t n) { return (n + 255) & ~(size_t)255; };
    if (need_shade) {   // versions 1 .. K-1: copies of the build's records (nothing has written any version's yet); version 0 keeps aliasing them
        const size_t each = pad((size_t)c->T * sizeof(DevShadeTri));
        DevBuf<char> blk;   // (the context takes it once the copies are in it)
        hipError_t e = blk.ensure((K - 1) * each);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(ART_E_NOMEM, std::string("art_scene_set_vertices: the versions' shading records: ") + hipGetErrorString(e)); }
        hipStream_t s = c->main_stream();
        for (uint32_t v = 1; v < K && e == hipSuccess; v++) e = hipMemcpyAsync(blk.p + (v - 1) * each, c->bvh.shade_tris, (size_t)c->T * sizeof(DevShadeTri), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hipfail(e, "art_scene_set_vertices: copies of the shading records");
        c->shade_block = std::move(blk);
        for (uint32_t v = 1; v < K; v++) c->as[v].shade = (DevShadeTri *)(c->shade_block.p + (v - 1) * each);
    }
    if (need_stage) {   // a larger staging for every version; what the old one held is not needed (a refit writes a version's staging in full for what it regathers)
        const size_t nv = c->deform_verts + c->prims[id].verts.size(), each = pad(nv * sizeof(ArtVertex));
        DevBuf<char> dblk; Pinned<char> hblk;   // (both or neither: the context keeps the old ones until then)
        hipError_t e = dblk.ensure(K * each);
        if (e == hipSuccess) e = hblk.ensure(K * each);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(ART_E_NOMEM, std::string("art_scene_set_vertices: staging of the vertices: ") + hipGetErrorString(e)); }
        c->stage_block = std::move(dblk); c->stage_pinned = std::move(hblk);
        for (uint32_t v = 0; v < K; v++) { c->as[v].d_stage = (float *)(c->stage_block.p + v * each); c->as[v].h_stage = (ArtVertex *)(c->stage_pinned.p + v * each); }
        c->deform_off[id] = (int64_t)c->deform_verts; c->deform_verts = nv;
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
        if (c->as.empty()) {   // (the ring of versions: art_scene_build made it already when the host announced ART_FLAG_DYNAMIC_SCENE)
            const auto t_begin = std::chrono::steady_clock::now();
            r = as_create(c); if (r) return r;
            c->first_move_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        }
        r = deform_prepare(c, id); if (r) return r;
    }
    std::memcpy(p.verts.data(), verts, (size_t)n_verts * sizeof(ArtVertex));
    p.verts_stale = true;                                            // the device's build copy is behind (a rebuild over the same set uploads them again)
    if (!in_tree) return ART_OK;                                     // takes effect with the build
    c->prim_deformed[id] = c->as_epoch + 1;                          // the next refit is the first to show them
    if (p.enabled) c->xform_dirty = true;                            // instanced: the next art_trace (or query) refits first; a masked one is regathered when it comes back
    return ART_OK;
}

int32_t art_scene_build(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_scene_build: null context");
    if (c->prims.empty()) return fail(ART_E_STATE, "art_scene_build: no primitives");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    as_release(c); c->xform_dirty = false; c->as_epoch = 0; c->binary_epoch = 0; c->refit_cost_ratio = 1.0f; // the versions were copies of the tree that goes away
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
    if (!resident) c->uploaded.clear();   // (an upload that fails half way leaves nothing to rely on)
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
    c->h_dev_prims = dp; c->masked_tris = 0;
    c->prim_moved.assign(dp.size(), 0); c->prim_deformed.assign(dp.size(), 0); c->deform_off.assign(dp.size(), -1);
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
        c->alpha_bits_stale = false;
        alpha_refresh_live(c);
    }
    c->built = true;
    plan_hint_built(c);
    c->first_move_ms = 0.f; c->versions_ms = 0.f;
    if (c->cfg.flags & ART_FLAG_DYNAMIC_SCENE) { r = as_create(c); if (r) return r; }   // the host said its models move: the ring of versions now, not in front of the first moved frame
    return ART_OK;
}

int32_t art_get_lbvh(ArtContext *c, uint32_t *leaf_gid, uint64_t *keys, int32_t *child, float *node_lo, float *node_hi, float *leaf_lo, float *leaf_hi) {
    if (!c) return fail(ART_E_INVALID, "art_get_lbvh: null context");
    if (!c->built) return fail(ART_E_STATE, "art_get_lbvh: scene not built");
    int32_t r = use_device(c); if (r) return r;
    r = refresh_now(c); if (r) return r;       // after a move: the boxes of where the models are now (the keys and the topology are the build's)
    if (!c->bvh.canon_boxes) c->binary_epoch = ~0ull;   // the build left the canonical tree's boxes for now: have them made
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
    const AsPtrs as = as_ptrs(c, c->as_cur);   // the version the next frame would read
    if (quantised) HIPC(hipMemcpy(quantised, as.wide, (size_t)c->bvh.n_wide * sizeof(DevNode4), hipMemcpyDeviceToHost));
    if (floats) HIPC(hipMemcpy(floats, as.widef, (size_t)c->bvh.n_wide * sizeof(DevNodeW), hipMemcpyDeviceToHost));
    return ART_OK;
}

} // extern "C"
