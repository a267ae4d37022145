// art_cast.hip -- rays and points in device buffers (include/art.h: art_cast_rays, art_cast_rays_multi, art_resolve_hits, art_closest_points, art_cast_spheres, art_closest_points_multi, art_overlap_boxes, art_cast_crossings, art_overlap_triangles, art_closest_triangles, art_cast_triangles; DESIGN.md 3.5 .. 3.15) and the queries of include/art_parity.h
// over them: the host side of the ring of cast blocks (CastState, art_context.h) -- one claim / commit, one query_begin and one set of descriptor checks, which every
// entry point goes through.  Every use of a CastState / CastBlock field is in this file; the kernels are art_query_rays.hip's, art_query_points.hip's and art_resolve.hip's.
#include "art_context.h"

// the first cast of a context: its stream (counted against the budget beside kMaxFrameSlots), the cursor blocks and their events
static int32_t cast_setup(ArtContext *c) {
    CastState &K = c->cast;
    if (K.stream) return ART_OK;
    hipError_t e = K.cursors.ensure((size_t)ART_CAST_POOL * kCastCursorWords);
    for (CastBlock &b : K.block) if (e == hipSuccess) e = b.ev.create(hipEventDisableTiming);
    if (e == hipSuccess) e = K.stream.acquire(c->device);   // (last: what was made before a failure is kept by its handle and found again by the next attempt)
    if (e != hipSuccess) return hipfail(e, "art_cast_rays: the cast stream, cursor blocks and events");
    return ART_OK;
}
// every cast enqueued so far has finished, on whichever stream it runs
static int32_t cast_wait_all(ArtContext *c) {
    for (CastBlock &b : c->cast.block) if (b.set) { HIPC(hipEventSynchronize(b.ev)); b.set = false; }
    return ART_OK;
}
int32_t art::cast_sync(ArtContext *c) {
    int32_t r = cast_wait_all(c); if (r) return r;
    if (c->cast.stream) HIPC(hipStreamSynchronize(c->cast.stream));   // (a refit a cast put there, the zeroing of a block)
    return ART_OK;
}
int32_t art::cast_drain(ArtContext *c) {
    if (!c->cast.stream) return ART_OK;   // nothing was ever cast
    int32_t r = use_device(c); if (r) return r;
    return cast_wait_all(c);
}
// the casts that hold `version` (scene_refresh is about to rewrite it): the host waits for those still running -- one CastState::host_waits per call that waited
int32_t art::cast_wait_version(ArtContext *c, uint32_t version) {
    bool waited = false;
    for (CastBlock &b : c->cast.block) if (b.set && b.version == version) {
        if (hipEventQuery(b.ev) != hipSuccess) { (void)hipGetLastError(); HIPC(hipEventSynchronize(b.ev)); waited = true; }
        b.set = false;
    }
    if (waited) c->cast.host_waits++;
    return ART_OK;
}
// The host side every enqueue on the ring shares -- a query's and a resolve's (art_resolve_hits traces nothing, but it reads a version of the scene and has to be waited
// for like a cast).  cast_claim: the scene as of the call, the stream, the version to read (an event wait on that stream while its refit may still run) and the next ring
// block, free.  cast_commit: the block's event behind what the caller launched, the version it holds, and its rays in the counts of casts (0: it traces none).
struct RingSlot { hipStream_t stream; uint32_t version, block; };
static int32_t cast_claim(ArtContext *c, hipStream_t user, RingSlot *q) {
    int32_t r = use_device(c); if (r) return r;
    r = cast_setup(c); if (r) return r;
    CastState &K = c->cast;
    if (as_pending(c)) { r = scene_refresh(c, ~0u, K.stream); if (r) return r; }   // the scene as of the call: the refit in front of the cast (past the cost threshold: a rebuild)
    r = ensure_wide(c, true); if (r) return r;
    hipStream_t s = user ? user : K.stream.p;
    const uint32_t ver = as_current(c);
    r = as_wait_ready(c, ver, s, ~0u); if (r) return r;   // the refit that wrote this version may still run: an event wait on the cast's stream, nothing on the host
    const uint32_t bi = K.next % ART_CAST_POOL;
    CastBlock &B = K.block[bi];
    if (B.set) {   // the ring of cursor blocks is lapped: its oldest cast has to be over
        if (hipEventQuery(B.ev) != hipSuccess) { (void)hipGetLastError(); HIPC(hipEventSynchronize(B.ev)); K.host_waits++; }
        B.set = false;
    }
    *q = RingSlot{s, ver, bi};
    return ART_OK;
}
static int32_t cast_commit(ArtContext *c, const RingSlot &q, uint32_t rays) {
    CastState &K = c->cast; CastBlock &B = K.block[q.block]; hipStream_t s = q.stream;
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(B.ev, s));
    B.set = true; B.version = q.version; K.next++;
    if (rays) { K.casts++; K.rays += rays; }
    return ART_OK;
}
// A query of n > 0 validated records on `user` (NULL: the context's cast stream): a block claimed, its cursors zeroed on the stream, and what every query reads of
// the context and of the version it holds in `a`.  The caller adds the fields of its own, launches, and ends with cast_commit.
static int32_t query_begin(ArtContext *c, hipStream_t user, uint32_t n, uint32_t cull, void *tuv, void *ids, QueryArgs &a, RingSlot *q) {
    int32_t r = cast_claim(c, user, q); if (r) return r;
    hipStream_t s = q->stream;
    uint32_t *cursors = c->cast.cursors + (size_t)q->block * kCastCursorWords;
    HIPC(hipMemsetAsync(cursors, 0, kCastCursorWords * 4, s));
    const AsPtrs as = as_ptrs(c, q->version);
    a.wide = as.wide; a.tris = as.tris; a.tri_prim = c->bvh.tri_prim; a.first_tri = c->d_first_tri.p;
    a.n = n; a.tuv = (float4 *)tuv; a.ids = (int2 *)ids; a.cursors = cursors;
    a.tune = c->trace_tune();
    a.filter = c->alpha_live || cull == 0u;   // while the scene has a mask or a cutoff (the leaf bits mark both), or the query sees nothing
    a.alpha_bits = c->d_alpha_bits.p; a.shade = as.shade; a.prims = as.prims; a.tex_pool = c->d_tex.p; a.cull = cull;
    return ART_OK;
}
// art_cast_rays' cast, which the queries of include/art_parity.h enqueue too.  *block (optional) receives the ring block whose event stands behind it.
static int32_t cast_enqueue(ArtContext *c, const void *rays, uint32_t n, bool any, uint32_t cull, void *tuv, void *ids, void *hit, hipStream_t user, uint32_t *block) {
    CastArgs a{}; RingSlot q;
    int32_t r = query_begin(c, user, n, cull, tuv, ids, a, &q); if (r) return r;
    a.rays = (const float4 *)rays; a.kind = any ? CastKind::Any : CastKind::Closest; a.hit = (uint8_t *)hit;
    launch_cast(a, q.stream);
    if (block) *block = q.block;
    return cast_commit(c, q, n);
}

// What the entry points ask of their descriptors, one text each.  A buffer of n records: null only when there are none (n = 0 touches nothing), and aligned; an optional output (null: not wanted): aligned
static bool misaligned(const void *p, size_t align) { return ((uintptr_t)p & (align - 1)) != 0; }
static int32_t invalid(const char *who, const std::string &what) { return fail(ART_E_INVALID, std::string(who) + ": " + what); }
static int32_t check_null(const char *who, const void *c, const void *d) { return !c || !d ? invalid(who, "null argument") : ART_OK; }
static int32_t check_flags(const char *who, uint32_t flags) { return flags != 0u ? invalid(who, "flags: must be 0") : ART_OK; }
static int32_t check_cull(const char *who, uint32_t cull_mask) { return cull_mask > 0xFFu ? invalid(who, "cull_mask: above 0xFF") : ART_OK; }
static int32_t check_n(const char *who, uint32_t n) { return n > ART_CAST_MAX_RAYS ? invalid(who, "n: above ART_CAST_MAX_RAYS") : ART_OK; }
static int32_t check_built(const char *who, const ArtContext *c, bool changed = true) { return c->built ? ART_OK : fail(ART_E_STATE, std::string(who) + ": scene not built" + (changed ? ", or changed since the build" : "") + " (art_scene_build)"); }
static int32_t check_buffer(const char *who, const char *name, const void *p, size_t align, uint32_t n, bool optional = false) {
    if (!misaligned(p, align) && (optional || p || !n)) return ART_OK;
    std::string what = optional ? "" : "null";
    if (align > 1) what += (optional ? "not " : " or not ") + std::to_string(align) + "-byte aligned";
    return invalid(who, std::string(name) + ": " + what);
}
// the fields the descriptors of the three casts of rays share (cast_check), and those of the two point queries (point_check)
static int32_t cast_check(const char *who, uint32_t flags, uint32_t cull_mask, uint32_t n, const void *rays_dev) {
    int32_t r = check_flags(who, flags);
    return r || (r = check_cull(who, cull_mask)) || (r = check_n(who, n)) ? r : check_buffer(who, "rays_dev", rays_dev, 16, n);
}
static int32_t check_records(const char *who, const char *tuv_name, const void *tuv_dev, const void *ids_dev, uint32_t n) {
    const int32_t r = check_buffer(who, tuv_name, tuv_dev, 16, n);
    return r ? r : check_buffer(who, "ids_dev", ids_dev, 8, n);
}
template <class D> static int32_t point_check(const char *who, const D *d) {   // D: ArtPointQuery | ArtPointQueryMulti
    int32_t r = check_cull(who, d->cull_mask);
    return r || (r = check_n(who, d->n)) || (r = check_buffer(who, "points_dev", d->points_dev, 16, d->n)) || (r = check_records(who, "duv_dev", d->duv_dev, d->ids_dev, d->n)) ? r : check_buffer(who, "point_dev", d->point_dev, 16, d->n, true);
}
// the two overlap queries' descriptors (overlap_check -- D: ArtBoxQuery | ArtTriQuery; in_name / in_dev: its buffer of queries; which outputs a kind has) and what their launches share (overlap_begin)
template <class D> static int32_t overlap_check(const char *who, ArtContext *c, const D *d, const char *in_name, const void *in_dev) {
    int32_t r;
    if ((r = check_flags(who, d->flags))) return r;
    if (d->reserved != 0u) return invalid(who, "reserved: must be 0");
    if (d->kind != ART_OVERLAP_ANY && d->kind != ART_OVERLAP_LIST) return invalid(who, "kind: ART_OVERLAP_ANY or ART_OVERLAP_LIST");
    if ((r = check_cull(who, d->cull_mask)) || (r = check_n(who, d->n)) || (r = check_buffer(who, in_name, in_dev, 16, d->n))) return r;
    if (d->kind == ART_OVERLAP_ANY) {
        if (d->ids_dev || d->count_dev) return invalid(who, "ids_dev / count_dev: must be NULL for ART_OVERLAP_ANY");
        if (d->max_hits != 0u) return invalid(who, "max_hits: must be 0 for ART_OVERLAP_ANY");
        if ((r = check_buffer(who, "hit_dev", d->hit_dev, 1, d->n))) return r;
    } else {
        if (d->hit_dev) return invalid(who, "hit_dev: must be NULL for ART_OVERLAP_LIST");
        if (d->max_hits == 0u || d->max_hits > ART_CAST_MAX_HITS) return invalid(who, "max_hits: 1 .. ART_CAST_MAX_HITS");
        if ((r = check_buffer(who, "ids_dev", d->ids_dev, 8, d->n)) || (r = check_buffer(who, "count_dev", d->count_dev, 4, d->n, true))) return r;
    }
    return check_built(who, c);
}
// a block of the ring for a checked descriptor of n > 0 queries, and the outputs both kinds of query share
template <class D> static int32_t overlap_begin(ArtContext *c, const D *d, OverlapArgs &a, RingSlot *q) {
    const int32_t r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, nullptr, d->ids_dev, a, q); if (r) return r;
    a.any = d->kind == ART_OVERLAP_ANY; a.hit = (uint8_t *)d->hit_dev; a.count = (uint32_t *)d->count_dev; a.max_hits = d->max_hits;
    return ART_OK;
}

extern "C" {

int32_t art_cast_rays(ArtContext *c, const ArtRayCast *d) {
    const char *who = "art_cast_rays"; int32_t r;
    if ((r = check_null(who, c, d))) return r;
    if (d->kind != ART_CAST_CLOSEST && d->kind != ART_CAST_ANY) return invalid(who, "kind: ART_CAST_CLOSEST or ART_CAST_ANY");
    if ((r = cast_check(who, d->flags, d->cull_mask, d->n, d->rays_dev))) return r;
    const bool any = d->kind == ART_CAST_ANY;
    if (any) {
        if (d->tuv_dev || d->ids_dev) return invalid(who, "tuv_dev / ids_dev: must be NULL for ART_CAST_ANY");
        if ((r = check_buffer(who, "hit_dev", d->hit_dev, 1, d->n))) return r;
    } else {
        if (d->hit_dev) return invalid(who, "hit_dev: must be NULL for ART_CAST_CLOSEST");
        if ((r = check_records(who, "tuv_dev", d->tuv_dev, d->ids_dev, d->n))) return r;
    }
    if ((r = check_built(who, c, false))) return r;
    if (d->n == 0u) return ART_OK;
    return cast_enqueue(c, d->rays_dev, d->n, any, d->cull_mask, d->tuv_dev, d->ids_dev, d->hit_dev, (hipStream_t)d->hip_stream, nullptr);
}

int32_t art_cast_rays_multi(ArtContext *c, const ArtRayCastMulti *d) {
    const char *who = "art_cast_rays_multi"; int32_t r;
    if ((r = check_null(who, c, d))) return r;
    if (d->max_hits == 0u || d->max_hits > ART_CAST_MAX_HITS) return invalid(who, "max_hits: 1 .. ART_CAST_MAX_HITS");
    if ((r = cast_check(who, d->flags, d->cull_mask, d->n, d->rays_dev)) || (r = check_records(who, "tuv_dev", d->tuv_dev, d->ids_dev, d->n))) return r;
    if ((r = check_built(who, c, false))) return r;
    if (d->n == 0u) return ART_OK;
    CastArgs a{}; RingSlot q;
    r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, d->tuv_dev, d->ids_dev, a, &q); if (r) return r;
    a.rays = (const float4 *)d->rays_dev; a.kind = CastKind::Multi; a.max_hits = d->max_hits; a.count = (uint8_t *)d->count_dev;
    launch_cast(a, q.stream);
    return cast_commit(c, q, d->n);
}

// ---- the surface behind hit records (include/art.h: art_resolve_hits) ---------------------------------------------------------------------------
// A resolve goes through the casts' ring: it claims a block (whose cursors it has no use for), holds the version it reads and leaves the block's event behind its
// launch, so art_cast_sync, sync_all and scene_refresh wait for it where they wait for casts.  It is not counted as a cast: it traces nothing.
int32_t art_resolve_hits(ArtContext *c, const ArtHitResolve *d) {
    const char *who = "art_resolve_hits"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = check_flags(who, d->flags)) || (r = check_n(who, d->n)) || (r = check_records(who, "tuv_dev", d->tuv_dev, d->ids_dev, d->n))) return r;
    if (misaligned(d->pos_dev, 16) || misaligned(d->ng_dev, 16) || misaligned(d->ns_dev, 16) || misaligned(d->albedo_dev, 16) || misaligned(d->orm_dev, 16))
        return invalid(who, "pos_dev / ng_dev / ns_dev / albedo_dev / orm_dev: not 16-byte aligned");
    if ((r = check_buffer(who, "uv_dev", d->uv_dev, 8, d->n, true))) return r;
    if (d->n != 0u && !d->pos_dev && !d->ng_dev && !d->ns_dev && !d->uv_dev && !d->albedo_dev && !d->orm_dev) return invalid(who, "no output buffer given");
    if ((r = check_built(who, c))) return r;
    if (d->n == 0u) return ART_OK;
    RingSlot q;
    r = cast_claim(c, (hipStream_t)d->hip_stream, &q); if (r) return r;
    const AsPtrs as = as_ptrs(c, q.version);
    ResolveArgs a{};
    a.tuv = (const float4 *)d->tuv_dev; a.ids = (const int2 *)d->ids_dev; a.n = d->n;
    a.n_prims = (uint32_t)c->h_dev_prims.size(); a.T = c->T;   // (after cast_claim: a rebuild the cost rule started made them anew, with the table)
    a.prims = as.prims; a.shade = as.shade; a.gid_leaf = c->bvh.gid_leaf; a.tex_pool = c->d_tex.p;
    a.pos = (float4 *)d->pos_dev; a.ng = (float4 *)d->ng_dev; a.ns = (float4 *)d->ns_dev; a.uv = (float2 *)d->uv_dev; a.albedo = (float4 *)d->albedo_dev; a.orm = (float4 *)d->orm_dev;
    launch_resolve(a, q.stream);
    return cast_commit(c, q, 0);
}

// ---- nearest surface points (include/art.h: art_closest_points) ---------------------------------------------------------------------------------
// A batch of queries goes through the casts' ring like a cast, and like a resolve it is not counted as one: it traces no ray.
int32_t art_closest_points(ArtContext *c, const ArtPointQuery *d) {
    const char *who = "art_closest_points"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = check_flags(who, d->flags))) return r;
    if ((r = d->reserved != 0u ? invalid(who, "reserved: must be 0") : point_check(who, d))) return r;
    if ((r = check_built(who, c))) return r;
    if (d->n == 0u) return ART_OK;
    ClosestArgs a{}; RingSlot q;
    r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, d->duv_dev, d->ids_dev, a, &q); if (r) return r;
    a.points = (const float4 *)d->points_dev; a.point = (float4 *)d->point_dev;
    launch_closest(a, q.stream);
    return cast_commit(c, q, 0);
}

// ---- the K nearest triangles (include/art.h: art_closest_points_multi) -------------------------------------------------------------------------------
// art_closest_points' path with K records a query: a block of the ring, counted as no cast.
int32_t art_closest_points_multi(ArtContext *c, const ArtPointQueryMulti *d) {
    const char *who = "art_closest_points_multi"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = check_flags(who, d->flags))) return r;
    if ((r = d->max_hits == 0u || d->max_hits > ART_CAST_MAX_HITS ? invalid(who, "max_hits: 1 .. ART_CAST_MAX_HITS") : point_check(who, d))) return r;
    if ((r = check_built(who, c))) return r;
    if (d->n == 0u) return ART_OK;
    ClosestMultiArgs a{}; RingSlot q;
    r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, d->duv_dev, d->ids_dev, a, &q); if (r) return r;
    a.points = (const float4 *)d->points_dev; a.point = (float4 *)d->point_dev; a.max_hits = d->max_hits; a.count = (uint8_t *)d->count_dev;
    a.gid_leaf = c->bvh.gid_leaf;   // (after query_begin: a rebuild the cost rule started made the table anew)
    launch_closest_multi(a, q.stream);
    return cast_commit(c, q, 0);
}

// ---- the triangles that touch a box or a triangle (include/art.h: art_overlap_boxes, art_overlap_triangles) -----------------------------------
// art_closest_points' path with boxes or triangles for points: a block of the ring, counted as no cast.  Which outputs a kind has is checked once for both
// (overlap_check above); the rest is the family's.
int32_t art_overlap_boxes(ArtContext *c, const ArtBoxQuery *d) {
    const char *who = "art_overlap_boxes"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = overlap_check(who, c, d, "boxes_dev", d->boxes_dev))) return r;
    if (d->n == 0u) return ART_OK;
    OverlapArgs a{}; RingSlot q;
    r = overlap_begin(c, d, a, &q); if (r) return r;
    a.boxes = (const float4 *)d->boxes_dev;
    launch_overlap(a, q.stream);
    return cast_commit(c, q, 0);
}
int32_t art_overlap_triangles(ArtContext *c, const ArtTriQuery *d) {
    const char *who = "art_overlap_triangles"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = overlap_check(who, c, d, "tris_dev", d->tris_dev))) return r;
    if (d->n == 0u) return ART_OK;
    TriOverlapArgs a{}; RingSlot q;
    r = overlap_begin(c, d, a, &q); if (r) return r;
    a.qtris = (const float4 *)d->tris_dev;
    launch_tri_overlap(a, q.stream);
    return cast_commit(c, q, 0);
}

// ---- the distance from a triangle to the scene (include/art.h: art_closest_triangles) -----------------------------------------------------------------
// art_closest_points' path with triangles for points and a second point a record: a block of the ring, counted as no cast.
int32_t art_closest_triangles(ArtContext *c, const ArtTriDistance *d) {
    const char *who = "art_closest_triangles"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = check_flags(who, d->flags))) return r;
    if (d->reserved != 0u) return invalid(who, "reserved: must be 0");
    if ((r = check_cull(who, d->cull_mask)) || (r = check_n(who, d->n)) || (r = check_buffer(who, "tris_dev", d->tris_dev, 16, d->n)) || (r = check_records(who, "duv_dev", d->duv_dev, d->ids_dev, d->n)) ||
        (r = check_buffer(who, "point_dev", d->point_dev, 16, d->n, true)) || (r = check_buffer(who, "qpoint_dev", d->qpoint_dev, 16, d->n, true))) return r;
    if ((r = check_built(who, c))) return r;
    if (d->n == 0u) return ART_OK;
    TriDistanceArgs a{}; RingSlot q;
    r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, d->duv_dev, d->ids_dev, a, &q); if (r) return r;
    a.qtris = (const float4 *)d->tris_dev; a.point = (float4 *)d->point_dev; a.qpoint = (float4 *)d->qpoint_dev;
    launch_tri_distance(a, q.stream);
    return cast_commit(c, q, 0);
}

// ---- a ball along each ray (include/art.h: art_cast_spheres) -----------------------------------------------------------------------------------------
// A cast like the others, counted in casts and rays, with another kernel behind it.
int32_t art_cast_spheres(ArtContext *c, const ArtSphereCast *d) {
    const char *who = "art_cast_spheres"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = cast_check(who, d->flags, d->cull_mask, d->n, d->rays_dev))) return r;
    if (!(d->radius >= 0.0f) || d->radius == INFINITY) return invalid(who, "radius: NaN, negative or infinite");
    if ((r = check_records(who, "tuv_dev", d->tuv_dev, d->ids_dev, d->n)) || (r = check_buffer(who, "point_dev", d->point_dev, 16, d->n, true))) return r;
    if ((r = check_built(who, c))) return r;
    if (d->n == 0u) return ART_OK;
    CastArgs a{}; RingSlot q;
    r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, d->tuv_dev, d->ids_dev, a, &q); if (r) return r;
    a.rays = (const float4 *)d->rays_dev; a.kind = CastKind::Sweep; a.radius = d->radius + 0.0f; a.point = (float4 *)d->point_dev;   // (-0.0 + 0.0 is +0.0)
    launch_cast(a, q.stream);
    return cast_commit(c, q, d->n);
}

// ---- a triangle along each ray (include/art.h: art_cast_triangles) ------------------------------------------------------------------------------------
// A cast like the others, counted in casts and rays, on the point queries' loop: query_begin, a launch, cast_commit.
int32_t art_cast_triangles(ArtContext *c, const ArtTriCast *d) {
    const char *who = "art_cast_triangles"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = check_flags(who, d->flags))) return r;
    if (d->reserved != 0u) return invalid(who, "reserved: must be 0");
    if ((r = check_cull(who, d->cull_mask)) || (r = check_n(who, d->n)) || (r = check_buffer(who, "sweeps_dev", d->sweeps_dev, 16, d->n)) || (r = check_records(who, "tuv_dev", d->tuv_dev, d->ids_dev, d->n)) ||
        (r = check_buffer(who, "point_dev", d->point_dev, 16, d->n, true)) || (r = check_buffer(who, "qpoint_dev", d->qpoint_dev, 16, d->n, true))) return r;
    if ((r = check_built(who, c))) return r;
    if (d->n == 0u) return ART_OK;
    TriCastArgs a{}; RingSlot q;
    r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, d->tuv_dev, d->ids_dev, a, &q); if (r) return r;
    a.sweeps = (const float4 *)d->sweeps_dev; a.point = (float4 *)d->point_dev; a.qpoint = (float4 *)d->qpoint_dev;
    launch_tri_cast(a, q.stream);
    return cast_commit(c, q, d->n);
}

// ---- the surfaces each ray enters and leaves (include/art.h: art_cast_crossings) ----------------------------------------------------------------------
// A cast like the others, counted in casts and rays; its one output is the pair of counts (no tuv / ids records).
int32_t art_cast_crossings(ArtContext *c, const ArtRayCrossings *d) {
    const char *who = "art_cast_crossings"; int32_t r;
    if ((r = check_null(who, c, d)) || (r = cast_check(who, d->flags, d->cull_mask, d->n, d->rays_dev))) return r;
    if (d->reserved != 0u) return invalid(who, "reserved: must be 0");
    if ((r = check_buffer(who, "cross_dev", d->cross_dev, 8, d->n))) return r;
    if ((r = check_built(who, c))) return r;
    if (d->n == 0u) return ART_OK;
    CastArgs a{}; RingSlot q;
    r = query_begin(c, (hipStream_t)d->hip_stream, d->n, d->cull_mask, nullptr, nullptr, a, &q); if (r) return r;
    a.rays = (const float4 *)d->rays_dev; a.kind = CastKind::Crossings; a.cross = (uint2 *)d->cross_dev;
    launch_cast(a, q.stream);
    return cast_commit(c, q, d->n);
}

int32_t art_cast_sync(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_cast_sync: null context");
    return cast_drain(c);
}

int32_t art_cast_counts(ArtContext *c, uint64_t *casts, uint64_t *rays, uint64_t *host_waits) {
    if (!c) return fail(ART_E_INVALID, "art_cast_counts: null context");
    if (casts) *casts = c->cast.casts;
    if (rays) *rays = c->cast.rays;
    if (host_waits) *host_waits = c->cast.host_waits;
    return ART_OK;
}

// The queries of include/art_parity.h: host wrappers over the cast -- the rays into a device buffer the context keeps (it only grows), one cast on the context's cast stream,
// that cast's event as the fence, the records back.  Frames in flight are not waited for.
static int32_t query_by_cast(ArtContext *c, const float *rays, uint32_t n, uint32_t cull_mask, bool any, float *tuv, int32_t *ids, uint8_t *hit, const char *who) {
    if (n > ART_CAST_MAX_RAYS) return fail(ART_E_INVALID, std::string(who) + ": more than ART_CAST_MAX_RAYS rays");
    int32_t r = use_device(c); if (r) return r;
    CastState &K = c->cast;
    const size_t out_bytes = any ? (size_t)n : (size_t)n * 24;   // t,u,v,0 of every ray, then the id pairs
    HIPC(K.q_rays.ensure((size_t)n * 2)); HIPC(K.q_out.ensure(out_bytes));   // (the cast that read them last was fenced by its query)
    HIPC(hipMemcpy(K.q_rays.p, rays, (size_t)n * 32, hipMemcpyHostToDevice));
    uint32_t bi = 0;
    r = cast_enqueue(c, K.q_rays.p, n, any, cull_mask, any ? nullptr : K.q_out.p, any ? nullptr : K.q_out.p + (size_t)n * 16, any ? K.q_out.p : nullptr, nullptr, &bi);
    if (r) return r;
    HIPC(hipEventSynchronize(K.block[bi].ev)); K.block[bi].set = false;
    if (any) HIPC(hipMemcpy(hit, K.q_out.p, n, hipMemcpyDeviceToHost));
    else { HIPC(hipMemcpy(tuv, K.q_out.p, (size_t)n * 16, hipMemcpyDeviceToHost)); HIPC(hipMemcpy(ids, K.q_out.p + (size_t)n * 16, (size_t)n * 8, hipMemcpyDeviceToHost)); }
    return ART_OK;
}
int32_t art_query_closest(ArtContext *c, const float *rays, uint32_t n, float *tuv, int32_t *ids) { return art_query_closest_masked(c, rays, n, 0xFFu, tuv, ids); }
// (the rays' cull mask, DESIGN.md 3.4: 0xFF is art_query_closest; the filtered tracer instances run while the scene needs them or the mask is 0)
int32_t art_query_closest_masked(ArtContext *c, const float *rays, uint32_t n, uint32_t cull_mask, float *tuv, int32_t *ids) {
    if (!c || (n && (!rays || !tuv || !ids))) return fail(ART_E_INVALID, "art_query_closest: null argument");
    if (cull_mask > 0xFFu) return fail(ART_E_INVALID, "art_query_closest_masked: cull_mask: above 0xFF");
    if (!c->built) return fail(ART_E_STATE, "art_query_closest: scene not built");
    if (n == 0) return ART_OK;
    return query_by_cast(c, rays, n, cull_mask, false, tuv, ids, nullptr, "art_query_closest");
}

int32_t art_query_any(ArtContext *c, const float *rays, uint32_t n, uint8_t *hit) { return art_query_any_masked(c, rays, n, 0xFFu, hit); }
int32_t art_query_any_masked(ArtContext *c, const float *rays, uint32_t n, uint32_t cull_mask, uint8_t *hit) {
    if (!c || (n && (!rays || !hit))) return fail(ART_E_INVALID, "art_query_any: null argument");
    if (cull_mask > 0xFFu) return fail(ART_E_INVALID, "art_query_any_masked: cull_mask: above 0xFF");
    if (!c->built) return fail(ART_E_STATE, "art_query_any: scene not built");
    if (n == 0) return ART_OK;
    return query_by_cast(c, rays, n, cull_mask, true, nullptr, nullptr, hit, "art_query_any");
}

} // extern "C"
