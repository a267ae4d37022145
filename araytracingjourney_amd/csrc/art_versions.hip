// art_versions.hip -- the ring of versions of the acceleration structure behind moving, deforming, masked and alpha-cut primitives: its memory, the refit in front of a
// frame or a cast (scene_refresh), the rebuild rule, the refit streams.  Every write of a Versions field (art_context.h) is in this unit; art_scene.hip's setters tell it what
// changed, art_api.hip and art_cast.hip ask it which version to read.  Host code only; the kernels are art_refit.hip's.
// Not here yet, because each changes behaviour: a smaller ring when the device allocation fails would go into as_create, where `K` is chosen; the
// bound on the refit streams into as_create's `want`; and `built` is true before the ring exists under ART_FLAG_DYNAMIC_SCENE -- as_scene_built is
// where the two would be ordered.
#include "art_context.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

// A cursor over a block -- its host address and, for pinned memory, the device's address of the same byte -- in 256-byte steps.  Over null bases it only counts: the walk
// that sizes a block is the walk that places the pointers into it.
struct Carve {
    char *h = nullptr, *d = nullptr; size_t off = 0;
    template <class T, class U = T> T *take(size_t n, U **twin = nullptr) {
        T *p = h ? (T *)(h + off) : nullptr;
        if (twin) *twin = d ? (U *)(d + off) : nullptr;
        off += (n * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

AsPtrs art::as_ptrs(const ArtContext *c, uint32_t v) {
    if (c->ver.as.empty()) return AsPtrs{c->bvh.tris, c->bvh.widef, c->bvh.wide, c->d_prims.p, c->bvh.shade_tris};
    const AsVersion &V = c->ver.as[v];
    return AsPtrs{V.tris, V.widef, V.wide, V.prims, V.shade};
}
uint32_t art::as_current(const ArtContext *c) { return c->ver.as_cur; }
bool art::as_pending(const ArtContext *c) { return c->ver.xform_dirty; }
static uint64_t epoch_of_current(const ArtContext *c) { return c->ver.as.empty() ? 0 : c->ver.as[c->ver.as_cur].epoch; }
bool art::binary_is_current(const ArtContext *c) { return c->ver.binary_epoch == epoch_of_current(c); }
void art::binary_mark(ArtContext *c, bool current) { c->ver.binary_epoch = current ? epoch_of_current(c) : ~0ull; }
void art::as_frame_reads(ArtContext *c, uint32_t v, uint32_t k) { if (!c->ver.as.empty()) { c->ver.as[v].used[k] = c->frame_no + 1; c->ver.as[v].aux[k] = false; } }
void art::as_aux_behind(ArtContext *c, uint32_t v, uint32_t k) { if (!c->ver.as.empty()) c->ver.as[v].aux[k] = true; }
int32_t art::as_sync_streams(ArtContext *c) {
    Versions &R = c->ver;
    for (uint32_t id : R.ingest_open) if (id < R.ingest.size() && R.ingest[id].open) { HIPC(hipEventSynchronize(R.ingest[id].done)); R.ingest[id].open = false; }   // (ingests on callers' streams: a refit below may stand behind one)
    R.ingest_open.clear();
    for (uint32_t i = 0; i < R.n_refit_streams; i++) HIPC(hipStreamSynchronize(R.refit_stream[i]));
    return ART_OK;
}
void art::as_fill_stats(const ArtContext *c, ArtStats *st) {
    const Versions &R = c->ver;
    st->first_move_ms = R.first_move_ms; st->versions_ms = R.versions_ms;
    st->refit_ms = R.last_refit_ms; st->refit_cost_ratio = R.refit_cost_ratio; st->refits = R.refits; st->rebuilds = R.rebuilds;
}

// everything that reads them has finished (the caller synchronised)
void art::as_release(ArtContext *c) {
    Versions &R = c->ver;
    R.as.clear(); R.as_cur = 0;   // (their events) -- then the blocks they pointed into: device arrays, staging memory, shading records, staging of replaced vertices
    R.as_block.release(); R.as_pinned.release(); R.shade_block.release(); R.stage_block.release(); R.stage_pinned.release();
    R.deform_verts = 0; std::fill(R.deform_off.begin(), R.deform_off.end(), (int64_t)-1);
}
// The ring's two blocks as the versions lie in them: per version the device arrays (the tree's arrays once more for every version but 0, which aliases the build's; the
// refit's marks, scratch and batch costs) and the pinned ones with the device's addresses of the same.  Returns the bytes walked: {device, pinned}.
struct RingBytes { size_t dev, pin; };
static RingBytes ring_carve(ArtContext *c, char *dev, char *pin, char *pin_d) {
    const size_t np = c->h_dev_prims.size(), T = c->T, NW = c->bvh.n_wide, nbat = c->bvh.sub_batches ? c->bvh.sub_batches : 1;
    Carve D{dev, nullptr}, P{pin, pin_d};
    for (AsVersion &V : c->ver.as) {
        if (V.owned) { V.tris = D.take<DevTri>(T); V.widef = D.take<DevNodeW>(NW); V.wide = D.take<DevNode4>(NW); V.prims = D.take<DevPrim>(np); }
        V.mark = D.take<uint32_t>(NW); V.acc = D.take<double>(4); V.batch_cost = D.take<double>(nbat);
        V.h_prims = P.take<DevPrim>(np, &V.dh_prims); V.h_touched = P.take<uint8_t>(np, &V.dh_touched); V.h_result = P.take<double>(4, &V.dh_result); V.h_dirty = P.take<uint32_t>(nbat, &V.dh_dirty);
    }
    return RingBytes{D.off, P.off};
}
// as many refit streams as the tuning asks for (default: one per ring slot, up to four), kept for the life of the context
static int32_t refit_streams_fit(ArtContext *c) {
    Versions &R = c->ver;
    const uint32_t want = c->tuning.refit_streams == 0xFFFFFFFFu ? 0u : (c->tuning.refit_streams ? std::min(c->tuning.refit_streams, 4u) : std::min(c->F, 4u));
    while (R.n_refit_streams < want) {
        int lo = 0, hi = 0; HIPC(hipDeviceGetStreamPriorityRange(&lo, &hi));   // hi: the numerically smallest = the most urgent: a refit is a handful of small launches a whole frame waits for
        HIPC(R.refit_stream[R.n_refit_streams].create(hi)); R.n_refit_streams++;
    }
    while (R.n_refit_streams > want) R.refit_stream[--R.n_refit_streams].release();   // (waits for it first)
    return ART_OK;
}
// every version a copy of the build's arrays, its marks and scratch zero, its event made: everything on stream s, asynchronously (the caller waits once)
static int32_t ring_fill(ArtContext *c, hipStream_t s) {
    const size_t np = c->h_dev_prims.size(), T = c->T, NW = c->bvh.n_wide;
    for (AsVersion &V : c->ver.as) {
        V.shade = c->bvh.shade_tris;   // (every version's own copy only once a built primitive is deformed: deform_prepare)
        if (!V.owned) { V.tris = c->bvh.tris; V.widef = c->bvh.widef; V.wide = c->bvh.wide; V.prims = c->d_prims.p; }
        else {
            HIPC(hipMemcpyAsync(V.tris, c->bvh.tris, T * sizeof(DevTri), hipMemcpyDeviceToDevice, s)); HIPC(hipMemcpyAsync(V.widef, c->bvh.widef, NW * sizeof(DevNodeW), hipMemcpyDeviceToDevice, s));
            HIPC(hipMemcpyAsync(V.wide, c->bvh.wide, NW * sizeof(DevNode4), hipMemcpyDeviceToDevice, s)); HIPC(hipMemcpyAsync(V.prims, c->d_prims.p, np * sizeof(DevPrim), hipMemcpyDeviceToDevice, s));
        }
        HIPC(hipMemsetAsync(V.mark, 0, NW * 4, s)); HIPC(hipMemsetAsync(V.acc, 0, 32, s));
        HIPC(V.ready.create(hipEventDisableTiming));
    }
    return ART_OK;
}
// the first move of a built scene: the ring of versions (ArtTuning.as_versions; default 4: one more than the reference's frames in flight, renderer.rs:135 -- measured on
// config 2 with a model of 164 k triangles moving every frame, 16 ring slots: 0.70 / 0.38 / 0.28 / 0.25 / 0.26 ms per frame with 1 / 2 / 3 / 4 / 8 versions), every one a copy of
// the build's arrays -- the topology (child references, valid masks, sort axes) is never written again -- and the cost of the tree as built
static int32_t as_create(ArtContext *c) {
    Versions &R = c->ver;
    int32_t r = ensure_wide(c, true); if (r) return r;
    r = sync_all(c); if (r) return r;
    const auto t_begin = std::chrono::steady_clock::now();
    // (default: twice the frames in flight, 4 at least and 24 at most.  The host may issue the refit of frame n once the frames that read that version -- frame n - K -- are
    //  over, so K sets how far it runs ahead of the GPU: with K = F + 1 a refit is issued when its ring slot's previous frame has all but finished and its latency -- 0.5 ms
    //  among eight frames in flight -- stands in front of the slot's next frame; with K = 2 F it is a ring trip ahead.  Config 2, F = 8, a model of 164 k triangles moving
    //  every frame: 0.252 / 0.229 / 0.213 / 0.210 / 0.205 / 0.205 ms a frame with 4 / 8 / 10 / 12 / 16 / 24 versions (profiles/README.md round 4d); a version is the tree's
    //  arrays once more: 42 MB for config 2, 450 MB for config 4.)
    const uint32_t K = c->tuning.as_versions ? std::min(c->tuning.as_versions, kMaxAsVersions) : std::min(std::max(2u * c->F, 4u), kMaxAsVersions);
    R.as.clear(); R.as.resize(K);
    for (uint32_t v = 1; v < K; v++) R.as[v].owned = true;
    hipStream_t s = c->main_stream();
    double t_sec[6] = {0, 0, 0, 0, 0, 0};
    auto lap = [&, last = std::chrono::steady_clock::now()](int i) mutable { const auto n = std::chrono::steady_clock::now(); t_sec[i] += std::chrono::duration<double, std::milli>(n - last).count(); last = n; };
    auto body = [&]() -> int32_t {
        int32_t q = refit_streams_fit(c); if (q) return q;
        lap(0);
        if (!c->bvh.sub_off) { // the parents in the 4-wide tree and the refit's work lists (a workgroup per batch of subtrees): all there or none (refit_lists_build)
            hipError_t e = refit_lists_build(c->bvh, c->T, s);
            if (e != hipSuccess) return hipfail(e, "refit_lists_build");
        }
        lap(1);
        // one device block and one pinned block: the carve over nothing says how large, the carve over the blocks places every version's pointers
        const RingBytes need = ring_carve(c, nullptr, nullptr, nullptr);
        HIPC(R.as_block.ensure(need.dev));
        HIPC(R.as_pinned.ensure(need.pin));
        lap(2);
        ring_carve(c, R.as_block.p, R.as_pinned.p, R.as_pinned.d);
        q = ring_fill(c, s); if (q) return q;
        lap(3);
        AsVersion &V0 = R.as[0];
        launch_wide_cost(c->bvh.n_wide, V0.widef, nullptr, V0.acc, V0.dh_result, s);   // the cost of the tree as built
        HIPC(hipGetLastError()); HIPC(hipStreamSynchronize(s));
        R.as_cost0 = V0.h_result[0]; R.refit_cost_ratio = 1.0f;
        lap(4);
        if (c->tuning.log & 1u) std::fprintf(stderr, "[art] versions: %u of them; refit streams %.2f ms, parents + work lists %.2f, the two allocations %.2f, copies issued + events %.2f, the wait for them + the cost of the tree as built %.2f\n", K, t_sec[0], t_sec[1], t_sec[2], t_sec[3], t_sec[4]);
        return ART_OK;
    };
    r = body();
    if (r) as_release(c);
    R.versions_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return r;
}
// the ring if there is none yet, its time booked as what the first move paid (a host that announced its moves with ART_FLAG_DYNAMIC_SCENE paid it in art_scene_build)
static int32_t ring_ensure(ArtContext *c) {
    if (!c->ver.as.empty()) return ART_OK;
    const auto t_begin = std::chrono::steady_clock::now();
    int32_t r = as_create(c); if (r) return r;
    c->ver.first_move_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return ART_OK;
}

// ---- art_scene_build's two ends, and what the setters report ----------------------------------------------------------------------------
void art::as_scene_reset(ArtContext *c) {   // (the caller synchronised) the versions were copies of the tree that goes away
    Versions &R = c->ver;
    as_release(c); R.ingest.clear(); R.ingest_open.clear();   // (the ingests' events: sync_all waited for them)
    R.xform_dirty = false; R.as_epoch = 0; R.binary_epoch = 0; R.refit_cost_ratio = 1.0f;
}
int32_t art::as_scene_built(ArtContext *c) {
    Versions &R = c->ver;
    const size_t np = c->h_dev_prims.size();
    R.masked_tris = 0; R.prim_moved.assign(np, 0); R.prim_deformed.assign(np, 0); R.deform_off.assign(np, -1); R.ingest.clear(); R.ingest.resize(np);
    R.alpha_bits_stale = false;   // (the build made the bits of every cutoff and mask there is)
    R.first_move_ms = 0.f; R.versions_ms = 0.f;
    if (c->cfg.flags & ART_FLAG_DYNAMIC_SCENE) return as_create(c);   // the host said its models move: the ring of versions now, not in front of the first moved frame
    return ART_OK;
}
void art::as_prim_moved(ArtContext *c, uint32_t id, bool shows, int64_t masked_delta) {
    Versions &R = c->ver;
    if (masked_delta) { R.masked_tris += masked_delta; c->stats.num_triangles = (uint32_t)((int64_t)c->T - R.masked_tris); }
    if (id < R.prim_moved.size()) R.prim_moved[id] = R.as_epoch + 1;   // the next refit is the first to show it
    if (shows) R.xform_dirty = true;                                    // instanced: the next art_trace (or query) refits first
}
void art::as_table_changed(ArtContext *c, bool new_alpha_bits) {
    if (new_alpha_bits) c->ver.alpha_bits_stale = true;   // the primitive's leaves get their bits in front of the refit (bits that are there already stay)
    c->ver.xform_dirty = true;                            // the next art_trace (or query) writes the next version of the table
}

// K - first equal slots of n T's each, walked like the ring's blocks (the versions' shading records; their staging, device and pinned at the same offsets): place(version,
// the slot at h, the slot at d) for every slot.  Returns the bytes walked.
template <class T, class F> static size_t carve_slots(uint32_t first, uint32_t K, size_t n, char *h, char *d, F place) {
    Carve S{h, d};
    for (uint32_t v = first; v < K; v++) { char *dv = nullptr; T *hv = S.take<T>(n, &dv); place(v, hv, dv); }
    return S.off;
}
// The first deformation of a built primitive (art_scene_set_vertices): every version gets shading records of its own (a frame in flight must keep the normals it was
// launched with), and the primitive a slot in every version's staging.  One synchronisation, here and never in front of a frame: an allocation that fails
// comes back from the call that asked for it, with nothing changed.
static int32_t deform_prepare(ArtContext *c, uint32_t id, bool staged) {
    Versions &R = c->ver;
    const uint32_t K = (uint32_t)R.as.size();
    const bool need_shade = K > 1 && !R.shade_block, need_stage = staged && R.deform_off[id] < 0;   // (the device form reads the primitive's slot of the build's vertex array: no staging)
    if (!need_shade && !need_stage) return ART_OK;   // (the steady state)
    int32_t r = sync_all(c); if (r) return r;
    if (!staged) R.ingest_host_syncs++;
    auto only_count = [](uint32_t, void *, char *) {};
    if (need_shade) {   // versions 1 .. K-1: copies of the build's records (nothing has written any version's yet); version 0 keeps aliasing them
        DevBuf<char> blk;   // (the context takes it once the copies are in it)
        hipError_t e = blk.ensure(carve_slots<DevShadeTri>(1, K, c->T, nullptr, nullptr, only_count));
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(ART_E_NOMEM, std::string("art_scene_set_vertices: the versions' shading records: ") + hipGetErrorString(e)); }
        hipStream_t s = c->main_stream();
        carve_slots<DevShadeTri>(1, K, c->T, blk.p, nullptr, [&](uint32_t, DevShadeTri *to, char *) { if (e == hipSuccess) e = hipMemcpyAsync(to, c->bvh.shade_tris, (size_t)c->T * sizeof(DevShadeTri), hipMemcpyDeviceToDevice, s); });
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hipfail(e, "art_scene_set_vertices: copies of the shading records");
        R.shade_block = std::move(blk);
        carve_slots<DevShadeTri>(1, K, c->T, R.shade_block.p, nullptr, [&](uint32_t v, DevShadeTri *at, char *) { R.as[v].shade = at; });
    }
    if (need_stage) {   // a larger staging for every version; what the old one held is not needed (a refit writes a version's staging in full for what it regathers)
        const size_t nv = R.deform_verts + c->prims[id].verts.size(), bytes = carve_slots<ArtVertex>(0, K, nv, nullptr, nullptr, only_count);
        DevBuf<char> dblk; Pinned<char> hblk;   // (both or neither: the context keeps the old ones until then)
        hipError_t e = dblk.ensure(bytes);
        if (e == hipSuccess) e = hblk.ensure(bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(ART_E_NOMEM, std::string("art_scene_set_vertices: staging of the vertices: ") + hipGetErrorString(e)); }
        R.stage_block = std::move(dblk); R.stage_pinned = std::move(hblk);
        carve_slots<ArtVertex>(0, K, nv, R.stage_pinned.p, R.stage_block.p, [&](uint32_t v, ArtVertex *h, char *d) { R.as[v].h_stage = h; R.as[v].d_stage = (float *)d; });
        R.deform_off[id] = (int64_t)R.deform_verts; R.deform_verts = nv;
    }
    return ART_OK;
}
int32_t art::as_prim_deformed(ArtContext *c, uint32_t id, bool shows, bool staged) {
    const bool ring_made = !c->ver.as.empty(), shade_made = (bool)c->ver.shade_block;
    int32_t r = ring_ensure(c); if (r) return r;   // (art_scene_build made it already when the host announced ART_FLAG_DYNAMIC_SCENE)
    r = deform_prepare(c, id, staged); if (r) return r;
    if (!staged && !ring_made && shade_made == (bool)c->ver.shade_block) c->ver.ingest_host_syncs++;   // (the ring's own wait, where deform_prepare's did not follow and count: one call, one count)
    c->ver.prim_deformed[id] = c->ver.as_epoch + 1;   // the next refit is the first to show the new vertices
    if (shows) c->ver.xform_dirty = true;             // instanced: the next art_trace (or query) refits first; a masked one is regathered when it comes back
    return ART_OK;
}

// ---- art_scene_set_vertices_device: the ingest and its ordering ("Vertices from device buffers") ---------------------------------
int32_t art::as_ingest(ArtContext *c, uint32_t id, const void *src, uint32_t stride_bytes, const ArtVertex *bring_up, hipStream_t s) {
    Versions &R = c->ver;
    PrimIngest &I = R.ingest[id];
    HIPC(I.done.create(hipEventDisableTiming));   // (once a primitive and build)
    // a refit that still gathers from the slot finishes first: up to four refit streams, so there can be more than one
    for (uint32_t v = 0; I.readers && v < (uint32_t)R.as.size(); v++) {
        if (!(I.readers & (1u << v))) continue;
        AsVersion &V = R.as[v];
        if (!V.ready_known) { if (hipEventQuery(V.ready) == hipSuccess) V.ready_known = true; else { (void)hipGetLastError(); HIPC(hipStreamWaitEvent(s, V.ready, 0)); } }
    }
    I.readers = 0;
    if (I.open) HIPC(hipStreamWaitEvent(s, I.done, 0));   // two ingests of one primitive run in call order, whichever streams they came on
    float *slot = const_cast<float *>(c->h_dev_prims[id].vertices);
    const uint32_t n = (uint32_t)c->prims[id].verts.size();
    if (bring_up) {   // the transition from the host form: the slot gets the host copy's attributes first; synchronous (the copy reads pageable memory), never the steady state
        HIPC(hipMemcpyAsync(slot, bring_up, (size_t)n * sizeof(ArtVertex), hipMemcpyHostToDevice, s));
        HIPC(hipStreamSynchronize(s)); R.ingest_host_syncs++;
    }
    launch_ingest_verts(src, stride_bytes, slot, n, s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(I.done, s));
    if (!I.open) { I.open = true; R.ingest_open.push_back(id); }
    R.ingests++;
    return ART_OK;
}
int32_t art::as_ingest_wait(ArtContext *c, uint32_t id) {
    Versions &R = c->ver;
    if (id < R.ingest.size() && R.ingest[id].open) { HIPC(hipEventSynchronize(R.ingest[id].done)); R.ingest[id].open = false; R.ingest_host_syncs++; }   // (its entry in ingest_open goes with the next sync_all)
    return ART_OK;
}
void art::as_ingest_counts(ArtContext *c, uint64_t host_syncs, uint64_t readbacks) { c->ver.ingest_host_syncs += host_syncs; c->ver.ingest_readbacks += readbacks; }

// the surface-area cost of the latest refit travels to the host behind it; once it has arrived it is what ArtStats.refit_cost_ratio and the rebuild rule go by
void art::harvest_cost(ArtContext *c) {
    Versions &R = c->ver;
    if (R.as.empty()) return;
    AsVersion &L = R.as[R.as_cur];
    if (!L.result_pending || hipEventQuery(L.ready) != hipSuccess) return;
    L.result_pending = false; L.ready_known = true;
    if (R.as_cost0 > 0.0) R.refit_cost_ratio = (float)(L.h_result[0] / R.as_cost0);
    const unsigned long long *st = reinterpret_cast<const unsigned long long *>(L.h_result);
    R.last_refit_ms = (float)((double)(st[3] - st[2]) * 1e-5);   // wall_clock64: 100 MHz
}
int32_t art::as_wait_ready(ArtContext *c, uint32_t v, hipStream_t stream, uint32_t own_slot) {
    if (c->ver.as.empty()) return ART_OK;
    AsVersion &V = c->ver.as[v];
    if (V.ready_known) return ART_OK;
    if (hipEventQuery(V.ready) == hipSuccess) { V.ready_known = true; return ART_OK; }
    if (own_slot == ~0u) (void)hipGetLastError();    // (no launch check of a frame follows: the not-ready answer is not left behind)
    else if (V.ready_slot == own_slot) return ART_OK;   // the refit is in front of the launch on this very stream
    HIPC(hipStreamWaitEvent(stream, V.ready, 0));      // nothing on the host
    return ART_OK;
}

// ---- scene_refresh and its steps ------------------------------------------------------------------------------------------------------------
// 1. the cost of the latest refit, if it has arrived: past the threshold the tree is built again for where the models are now
static bool rebuild_due(ArtContext *c) {
    harvest_cost(c);
    const float thr = c->tuning.refit_rebuild_ratio > 0.0f ? c->tuning.refit_rebuild_ratio : (c->tuning.refit_rebuild_ratio < 0.0f ? INFINITY : 2.0f);
    if (!(c->ver.refit_cost_ratio > thr)) return false;
    if (c->tuning.log & 1u) std::fprintf(stderr, "[art] refit cost %.2f x the build's: building again\n", c->ver.refit_cost_ratio);
    return true;
}
// 2. whatever still reads version `next`, about to be written, is waited for on the host, like the reference's per-frame fence (renderer.rs:451-466): the frames by ring
// slot, the casts, and the refit that wrote it last
static int32_t wait_for_readers(ArtContext *c, AsVersion &V, uint32_t next, uint32_t k, bool beside) {
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
    int32_t r = cast_wait_version(c, next); if (r) return r;   // casts still reading it (art_cast_rays: a cast holds the version it was launched on): the same wait, counted
    // the staging memory is read by the kernels of the refit that wrote this version last: that refit has to be over before the host writes it again (it is, whenever the
    // frames above were waited for -- they ran behind it -- but nothing else says so: a version no frame ever read, a ring slot that skipped its turn)
    if (!V.ready_known) { HIPC(hipEventSynchronize(V.ready)); V.ready_known = true; }
    V.result_pending = false;
    return ART_OK;
}
// 3. the primitive table as of now into the version's pinned copy, and a byte per primitive: moved since THIS version was written (it may be several refits behind)
static void stage_table(ArtContext *c, AsVersion &V) {
    const Versions &R = c->ver;
    const size_t np = c->h_dev_prims.size();
    std::memcpy(V.h_prims, c->h_dev_prims.data(), np * sizeof(DevPrim));
    for (size_t p = 0; p < np; p++) V.h_touched[p] = (p < R.prim_moved.size() && R.prim_moved[p] > V.epoch) ? 1 : 0;
}
// 4. what was deformed since this version was written: its current vertices into the version's staging (pinned, then ONE copy a run of slots on the refit's stream, in
// front of the refit that reads them from device memory), its table entry pointed there, and its shading records gathered again by the refit's leaf stage.
// A primitive whose slot of the build's vertex array holds its current vertices (art_scene_set_vertices_device wrote them there: the host copy is not ahead of it) is
// gathered from the slot, where its table entry points anyway: the refit's stream waits for the ingest's event, and the next ingest for this refit's
static int32_t stage_deformed(ArtContext *c, AsVersion &V, uint32_t v, hipStream_t s) {
    Versions &R = c->ver;
    const size_t np = c->h_dev_prims.size();
    size_t run_lo = 0, run_hi = 0;   // the run of staging slots the next copy covers (vertices)
    auto flush = [&]() -> int32_t {
        if (run_hi > run_lo) HIPC(hipMemcpyAsync(V.d_stage + run_lo * 12, V.h_stage + run_lo, (run_hi - run_lo) * sizeof(ArtVertex), hipMemcpyHostToDevice, s));
        run_lo = run_hi = 0; return ART_OK;
    };
    for (size_t p = 0; p < np && p < R.prim_deformed.size(); p++) {
        if (R.prim_deformed[p] <= V.epoch) continue;
        if (!c->prims[p].verts_stale) {
            PrimIngest &I = R.ingest[p];
            if (I.open) HIPC(hipStreamWaitEvent(s, I.done, 0));   // nothing on the host
            I.readers |= 1u << v;
            V.h_touched[p] |= kTouchRegather;
            continue;
        }
        const std::vector<ArtVertex> &vv = c->prims[p].verts;
        const size_t off = (size_t)R.deform_off[p];
        std::memcpy(V.h_stage + off, vv.data(), vv.size() * sizeof(ArtVertex));
        V.h_prims[p].vertices = V.d_stage + off * 12;
        V.h_touched[p] |= kTouchRegather;
        if (off != run_hi) { int32_t r = flush(); if (r) return r; run_lo = off; }
        run_hi = off + vv.size();
    }
    return flush();
}
static RefitArgs refit_args(const ArtContext *c, const AsVersion &V) {   // what the launch reads and writes of the tree and of this version
    RefitArgs ra{};
    ra.T = c->T; ra.n_wide = c->bvh.n_wide; ra.n_prims = (uint32_t)c->h_dev_prims.size(); ra.shade = V.shade; ra.prims_host = V.dh_prims; ra.prims_dev = V.prims; ra.touched = V.dh_touched;
    ra.sub_nodes = c->bvh.sub_nodes; ra.sub_leaves = c->bvh.sub_leaves; ra.sub_off = c->bvh.sub_off; ra.sub_batches = c->bvh.sub_batches; ra.sub_levels = c->bvh.sub_levels;
    ra.leaf_parent = c->bvh.leaf_parent; ra.node_parent = c->bvh.node_parent; ra.mark = V.mark; ra.tris = V.tris; ra.wide = V.wide; ra.widef = V.widef; ra.acc = V.acc; ra.result = V.dh_result;
    return ra;
}
// 5. the batches that hold a primitive that moved (since this version was written); the others keep their triangles, their boxes and -- in a large tree -- their
// cached share of the cost, which a version's first refit makes for all of them
static void choose_batches(const ArtContext *c, AsVersion &V, RefitArgs &ra) {
    const std::vector<uint32_t> &po = c->bvh.batch_prim_off, &pi = c->bvh.batch_prim_ids;
    const size_t np = c->h_dev_prims.size();
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
// A model moved since the last launch: bring the NEXT version of the structure up to date on stream s, the stream of ring slot k whose frame is about to be
// launched -- the frame is ordered behind the refit by the stream, frames on other streams by V.ready (art_trace).
// What the stream sees: the copies of deformed vertices, the alpha bits when they are stale, the refit's launches and one event record (round 3: two uploads, a launch per
// tree level, a clear, the cost's read-back and four event records -- twenty operations, 0.3 ms of issue in front of a 0.1 ms refit).
// (k = ~0u: in front of a cast, s a stream of the context that no frame runs on: every ring slot's frames are waited for, every later launch waits for V.ready)
int32_t art::scene_refresh(ArtContext *c, uint32_t k, hipStream_t s) {
    Versions &R = c->ver;
    if (!R.xform_dirty) return ART_OK;
    int32_t r = ring_ensure(c); if (r) return r;
    if (rebuild_due(c)) {
        r = art_scene_build(c); // (synchronises, uploads the primitives with their current matrices, drops the versions)
        if (r == ART_OK) R.rebuilds++;
        return r;
    }
    const uint32_t next = (R.as_cur + 1) % (uint32_t)R.as.size();
    AsVersion &V = R.as[next];
    const bool beside = R.n_refit_streams != 0;   // the refit runs beside the slot's frames, on a stream of its own
    if (beside) s = R.refit_stream[k % R.n_refit_streams];
    r = wait_for_readers(c, V, next, k, beside); if (r) return r;
    if (c->graph_mode) drop_graphs(c); // a captured frame holds the old version's pointers
    stage_table(c, V);
    r = stage_deformed(c, V, next, s); if (r) return r;
    RefitArgs ra = refit_args(c, V);
    choose_batches(c, V, ra);
    if (R.alpha_bits_stale) {   // a primitive got a cutoff: its leaves' bits, from this version's table, in front of the refit whose event the frames wait for
        launch_alpha_bits(c->T, c->bvh.leaf_gid, c->bvh.tri_prim, V.dh_prims, c->d_alpha_bits.p, s);
        R.alpha_bits_stale = false;
    }
    launch_refit(ra, s);
    HIPC(hipEventRecord(V.ready, s)); V.ready_known = false; V.ready_slot = beside ? ~0u : k; V.result_pending = true;   // (~0: no frame stream is behind it by itself)
    HIPC(hipGetLastError());
    R.as_cur = next; V.epoch = ++R.as_epoch; R.xform_dirty = false; R.refits++;
    return ART_OK;
}
// for the calls that read the structure outside a frame (the parity surface): nothing in flight, the pending move applied
int32_t art::refresh_now(ArtContext *c) {
    int32_t r = sync_all(c); if (r) return r;
    if (!c->ver.xform_dirty) return ART_OK;
    r = scene_refresh(c, 0, c->stream_of(0)); if (r) return r;
    r = sync_all(c); if (r) return r;   // (the refit may have run on a stream of its own)
    if (!c->ver.as.empty()) c->ver.as[c->ver.as_cur].ready_known = true;
    return ART_OK;
}
