// art_query_points.hip -- the device side of the point, box and triangle queries on device buffers (gfx950): nearest surface points (k_closest), the K nearest triangles (k_closest_multi), the triangles that
// touch a box (k_overlap) and those that touch a triangle (k_overlap_tris), the distance from a triangle to the scene (k_closest_tris), a triangle along a ray (k_cast_tris).  They have no ray to pool, so they are Sinks and walks of one loop of
// their own (point_trace); the casts and the sweep run art_walk.h's pooled loop in art_query_rays.hip.  What the two units share stands once, in art_query.h.  art_cast.hip is their host side.
#include "art_query.h"

namespace art {

// ---- nearest surface points (art_closest_points) ------------------------------------------------------------------------------------------------
// A query is a point and a radius, not a ray: the pooled loop's ray fields (inv, ood, tmin / tmax, the slab of every policy) have no meaning for it, and a query is ONE
// 16-byte load -- nothing a pool would save.  So the walk has a loop of its own (point_trace below, which the K nearest and the box query run too): the idle lanes of a
// wave read the next queries of its chunk directly (pop_chunk and the cursor block are the casts').  Stack entries are pairs (reference, the child's box_d2): `limit`
// only ever falls, and an entry whose box has fallen behind it by the time it is popped is dropped without a fetch.  Eight pairs a lane in LDS (4 KB a wave: 40 waves
// fit a CU's 160 KB, more than its 32 slots); deeper entries spill to scratch as references alone.
// No fmaf in anything that decides a record: d2_tri, box_d2 of a triangle and the point are restated by numpy float32 bit for bit (tests/np_closest.py).
struct ClosestK {
    const DevNode4 *wide; const DevTri *tris; const uint32_t *tri_prim, *first_tri;
    const float4 *points; float4 *tuv; int2 *ids; float4 *point;   // tuv: d,u,v,0; point: may be null
    uint32_t total, chunk, refill, leaf_batch;
    uint32_t *cursors;        // a cast's cursor block
    const uint32_t *bits; const DevShadeTri *shade; const DevPrim *prims; uint32_t cull;   // FILTER instance only: AlphaView's leaf bits, records and table; the queries' cull mask
};
constexpr int kClosestLds = 8;                                     // stack pairs a lane in LDS
constexpr int kQueryOvf = kOvfStack4 + (kLdsStack - kClosestLds);     // the scratch stack of point_trace's walks: Trav4's bound on pending siblings holds for any walk of the tree
template <bool FILTER> struct TravPoint {
    V3 p;
    float limit, bu, bv;     // limit: r*r, then the best candidate's d2_eff
    uint32_t bpos, bgid;
    int cur, sp;
    // (a spilled entry is the reference alone, TravBase's: pairs there would double the scratch every wave slot of the device reserves; it is visited unasked)
    __device__ __forceinline__ void push(int ref, float d2, int2 *lds, int *ovf) {
        if (sp < kClosestLds) lds[sp * kTraceBlock] = make_int2(ref, __float_as_int(d2)); else if (sp < kClosestLds + kQueryOvf) *(volatile int *)&ovf[sp - kClosestLds] = ref;   // (volatile: TravBase::push)
        sp = min(sp + 1, kClosestLds + kQueryOvf);
    }
    // the next entry whose box is still within the limit; true: none left, the query is finished
    __device__ __forceinline__ bool pop(int2 *lds, int *ovf) {
        while (sp > 0) {
            sp--;
            if (sp >= kClosestLds) { cur = *(volatile int *)&ovf[sp - kClosestLds]; return false; }
            const int2 e = lds[sp * kTraceBlock];
            if (!(__int_as_float(e.y) > limit)) { cur = e.x; return false; }
        }
        return true;
    }
    // the triangle in `cur`; a candidate below (limit, bgid) that the masks let through goes to take(d2_eff, u, v, pos, gid): the best here, the list's in TravPointMulti
    template <class TAKE> __device__ __forceinline__ bool step_leaf_take(const ClosestK &a, int2 *lds, int *ovf, const TAKE &take) {
        const uint32_t pos = (uint32_t)~cur;
        if (pos == 0x7FFFFFFFu) return pop(lds, ovf);   // kAbsentChild: nothing (TravBase::step_leaf_take)
        const float4 *tq = reinterpret_cast<const float4 *>(a.tris + pos);
        const float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid
        const float bd = box_d2(p, tc.y, tc.z, tc.w, td.x, td.y, td.z);
        float u, v;
        const float dt = tri_closest(p - mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), u, v);
        if ((dt < INFINITY) & (bd < INFINITY)) {   // the parts, not the maximum: fmaxf would drop a NaN
            const float de = fmaxf(dt, bd);
            const uint32_t gid = __float_as_uint(td.w);
            if ((de < limit || (de == limit && gid < bgid)) && (!FILTER || leaf_visible(a.bits, a.shade, a.prims, a.cull, pos))) take(de, u, v, pos, gid);
        }
        return pop(lds, ovf);
    }
    __device__ __forceinline__ bool step_leaf(const ClosestK &a, int2 *lds, int *ovf) {
        return step_leaf_take(a, lds, ovf, [this](float de, float u, float v, uint32_t pos, uint32_t gid) { limit = de; bu = u; bv = v; bpos = pos; bgid = gid; });
    }
    __device__ __forceinline__ bool step_internal(const DevNode4 *__restrict__ wide, int2 *lds, int *ovf) {
        return step_internal_by(wide, lds, ovf, [this](float lx, float ly, float lz, float hx, float hy, float hz) { return box_d2(p, lx, ly, lz, hx, hy, hz); });
    }
    // the node step for any query that has a squared distance to a box (dist: the point's box_d2 here, the query box's in TravTriDist)
    // (the decode of a child's six planes stands here and in TravBox::step_internal: one copy, as a struct returned or as out-parameters, moves k_closest* and k_overlap* -- profiles/README.md, "two query units")
    template <class DIST> __device__ __forceinline__ bool step_internal_by(const DevNode4 *__restrict__ wide, int2 *lds, int *ovf, const DIST &dist) {
        const auto [b, c, ox, oy, oz, sx, sy, sz, refs] = load_node4(wide, cur);
        float d2[4]; bool h[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t lxq = (b.x >> (8 * i)) & 255u, hxq = (b.w >> (8 * i)) & 255u;
            const float lx = fmaf((float)lxq, sx, ox), hx = fmaf((float)hxq, sx, ox);
            const float ly = fmaf((float)((b.y >> (8 * i)) & 255u), sy, oy), hy = fmaf((float)((c.x >> (8 * i)) & 255u), sy, oy);
            const float lz = fmaf((float)((b.z >> (8 * i)) & 255u), sz, oz), hz = fmaf((float)((c.y >> (8 * i)) & 255u), sz, oz);
            d2[i] = dist(lx, ly, lz, hx, hy, hz);
            h[i] = (lxq <= hxq) & !(d2[i] > limit);   // an inverted box (255 / 0): an absent child or a masked subtree -- a distance to it means nothing, so it is asked
        }
        // on with the nearest child within the limit; the others wait with their distances, the farthest at the bottom: what is popped next is the nearest of them, and
        // the limit has fallen the most by the time the far ones come up.  (A five-comparator network over (box_d2, reference); a child that is out sorts as +inf with
        // the absent reference, which is pushed nowhere and, should it come first, is a leaf that is nothing.  The order is speed only: the answer does not depend on it.)
        float k[4]; int rf[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { k[i] = h[i] ? d2[i] : INFINITY; rf[i] = h[i] ? refs[i] : kAbsentChild; }
#define ART_CSWAP(x, y) { const bool sw = k[y] < k[x]; const float tk = sw ? k[x] : k[y]; k[x] = sw ? k[y] : k[x]; k[y] = tk; const int tr_ = sw ? rf[x] : rf[y]; rf[x] = sw ? rf[y] : rf[x]; rf[y] = tr_; }
        ART_CSWAP(0, 1) ART_CSWAP(2, 3) ART_CSWAP(0, 2) ART_CSWAP(1, 3) ART_CSWAP(1, 2)
#undef ART_CSWAP
#pragma unroll
        for (int i = 3; i >= 1; i--) if (rf[i] != kAbsentChild) push(rf[i], k[i], lds, ovf);
        if (rf[0] == kAbsentChild) return pop(lds, ovf);
        cur = rf[0];
        return false;
    }
};
// The wave loop of the point and box queries (k_closest, k_closest_multi, k_overlap): a wave takes a chunk from the cursor block, its idle lanes read the next queries of
// the chunk, one each, and every lane walks its own by pooled_trace's step block.  TRAV: the walk -- push, pop, step_internal(wide, lds, ovf), step_leaf(a, lds, ovf) over
// stack entries of its own kind (STACK).  stack: the kernel's __shared__ array, kTraceBlock entries a level.  What else differs between the queries is their Sink:
//   init(tr) -> K                  once per lane, before the loop: what the walk keeps for the whole launch.  K: the records a query gets (wave-uniform; 1 where it is one)
//   begin(tr, sidx, K, radius)     reads query sidx.  A live one: the walk's start state, and radius for the finish -> true.  A dead one: its complete answer, written
//                                  there and then -> false, and it takes no lane
//   finish(tr, slot, K, radius)    the finished query's records
// (The __shared__ arrays stay where each kernel declares them; the walk, K and radius are the loop's own locals, handed to the hooks.  What this form moves in the kernels'
// code -- register names, six to eight instructions a point kernel in the path that starts a query, no resource figure -- is in profiles/README.md, "one point loop")
template <class TRAV, class ARGS, class STACK, class SINK>
__device__ __forceinline__ void point_trace(const ARGS &a, STACK *stack, const SINK &sink) {
    int ovf[kQueryOvf];
    STACK *lds = &stack[threadIdx.x];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leaf_batch = a.leaf_batch;
    const uint32_t n_chunks = (a.total + a.chunk - 1) / a.chunk;   // (pooled_trace's bounds: total <= ART_CAST_MAX_RAYS)
    uint32_t shard = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u;   // HW_REG_XCC_ID: speed only
    uint32_t shards_left = 8;
    uint32_t cur = 0, end = 0;   // wave-uniform: the unread part of this wave's chunk
    bool exhausted = false, active = false;
    TRAV tr;
    tr.sp = 0; tr.cur = 0;
    const uint32_t K = sink.init(tr);
    float radius = 0.0f;
    uint32_t slot = 0;
    for (;;) {
        const uint64_t idle = ballot64(!active);
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        if (n_idle >= a.refill) {
            if (!exhausted && cur == end) {
                const uint32_t got = pop_chunk(a.cursors, n_chunks, lane, shard, shards_left);
                if (got >= n_chunks) exhausted = true;
                else { cur = got * a.chunk; end = min(cur + a.chunk, a.total); }
            }
            if (!exhausted) {   // the idle lanes read the next queries of the chunk, one each
                const uint32_t take = min(n_idle, end - cur);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (!active && rank < take) {
                    const uint32_t sidx = cur + rank;
                    if (sink.begin(tr, sidx, K, radius)) { slot = sidx; active = true; }
                }
                cur += take;
            } else if (n_idle == 64u) break;
            if (ballot64(active) == 0ull) continue;
        }
        bool done = false;   // pooled_trace's step block: node steps, then the triangle tests once enough lanes wait on one (or nobody can move without it)
#pragma unroll
        for (int rep_ = 0; rep_ < ART_NODE_REPS; rep_++)
            if (active && !done && tr.cur >= 0) done = tr.step_internal(a.wide, lds, ovf);
        const bool on_leaf = active && !done && tr.cur < 0;
        const uint64_t lm = ballot64(on_leaf);
        if (lm != 0ull && ((uint32_t)__popcll(lm) >= leaf_batch || ballot64(active && !done && tr.cur >= 0) == 0ull)) { if (on_leaf) done = tr.step_leaf(a, lds, ovf); }
        if (done) { active = false; sink.finish(tr, slot, K, radius); }
    }
}
__device__ __forceinline__ float zero3(const float4 &q) { return (0.0f * q.x + 0.0f * q.y) + 0.0f * q.z; }   // 0 for three finite coordinates, NaN otherwise: a fetch sums one a vertex, in its own association
// a point query: xyz and the radius in w.  False: a dead one (a non-finite point, a NaN or negative radius), which gets its miss records without a walk
__device__ __forceinline__ bool read_point(const float4 *points, uint32_t sidx, float4 &q) {
    q = points[sidx];
    return zero3(q) == 0.0f && q.w == q.w && !(q.w < 0.0f);
}
// the two walks that keep ONE best candidate (TravPoint, TravTriDist): the start state for radius r, and the finished query's hit record with its optional point
template <class TRAV> __device__ __forceinline__ void best_start(TRAV &tr, float r) { tr.limit = r * r; tr.bu = 0.f; tr.bv = 0.f; tr.bpos = kNoHit; tr.bgid = kNoHit; tr.cur = 0; tr.sp = 0; }
template <class K, class TRAV> __device__ __forceinline__ void best_write(const K &a, const TRAV &tr, uint32_t slot) {
    write_hit(a, slot, tr.bgid, sqrtf(tr.limit), tr.bu, tr.bv);
    if (a.point) a.point[slot] = contact_point(a.tris, tr.bpos, tr.bu, tr.bv);
}
struct ClosestSink {
    const ClosestK &a;
    template <class TRAV> __device__ __forceinline__ uint32_t init(TRAV &) const { return 1u; }
    template <class TRAV> __device__ __forceinline__ bool begin(TRAV &tr, uint32_t sidx, uint32_t, float &radius) const {
        float4 q;
        if (read_point(a.points, sidx, q)) { tr.p = mk(q.x, q.y, q.z); best_start(tr, q.w); radius = q.w; return true; }
        write_point_miss(a, sidx, q.w);
        return false;
    }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot, uint32_t, float radius) const {
        if (tr.bgid != kNoHit) best_write(a, tr, slot); else write_point_miss(a, slot, radius);
    }
};
template <bool FILTER>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_closest(ClosestK a) {
    __shared__ int2 stack[kClosestLds * kTraceBlock];
    point_trace<TravPoint<FILTER>>(a, stack, ClosestSink{a});
}

// ---- the K nearest triangles (art_closest_points_multi) ------------------------------------------------------------------------------------------
// TravPoint's walk with the list (KList, keyed by d2_eff) in place of the single best, through TravPoint::step_leaf_take's hook; limit / bgid are the walk's LIMIT: (r*r, none)
// until the list is full, the K-th entry's pair from then on.  TravPoint's push, pop and step_internal read nothing else of the candidate, so they serve as they are: a
// child is skipped iff its box_d2 > limit -- strict, ties stay in play.  d2_tri, box_d2 and the point are the one copy above.
// An entry keeps the gid (the tie rule needs it at every comparison) and not the leaf position, which only the point of a record needs: the finish finds it through the
// structure's gid -> leaf table (Lbvh::gid_leaf, art_resolve_hits' table), one more load a record where a point is wanted and none in the walk.
template <bool FILTER> struct TravPointMulti : TravPoint<FILTER>, KList {
    __device__ __forceinline__ bool step_leaf(const ClosestK &a, int2 *lds, int *ovf) {
        return this->step_leaf_take(a, lds, ovf, [this](float de, float u, float v, uint32_t, uint32_t gid) { enter(de, u, v, gid, this->limit, this->bgid); });
    }
};
struct ClosestMultiK : ClosestK { uint8_t *count; const uint32_t *gid_leaf; uint32_t max_hits; };   // tuv / ids / point: max_hits records a query, query-major; count: a byte a query, or null
// KMAX 4 | 8: the list is KMAX KB of LDS a wave on top of the stack's 4 KB, and LDS is what bounds the waves a CU holds: 20 waves with KMAX 4, 13 with
// KMAX 8 -- five and three a SIMD, whose registers are the kernel's to use.  The loop is point_trace, with K records where k_closest has one.  (The list's array is the
// kernel's and comes to the sink as a pointer: declared in KList it cost two legs of this kernel's probe 0.4 % -- profiles/README.md, "one list, one hook")
template <int KMAX> struct ClosestMultiSink {
    const ClosestMultiK &a;
    uint4 *hits;   // the kernel's __shared__ list array
    template <class TRAV> __device__ __forceinline__ uint32_t init(TRAV &tr) const { tr.bind(hits, a.max_hits, KMAX); return tr.K; }
    template <class TRAV> __device__ __forceinline__ bool begin(TRAV &tr, uint32_t sidx, uint32_t K, float &radius) const {
        float4 q;
        if (read_point(a.points, sidx, q)) {
            tr.p = mk(q.x, q.y, q.z); tr.limit = q.w * q.w; tr.bgid = kNoHit; tr.cnt = 0u; tr.cur = 0; tr.sp = 0;
            radius = q.w;
            return true;
        }
        const size_t base = (size_t)sidx * K;   // K miss records and the count
        for (uint32_t j = 0; j < K; j++) write_point_miss(a, base + j, q.w);
        if (a.count) a.count[sidx] = 0;
        return false;
    }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot, uint32_t K, float radius) const {
        const size_t base = (size_t)slot * K;
        for (uint32_t j = 0; j < K; j++) {
            if (j < tr.cnt) {
                const uint4 e = tr.list[j * kTraceBlock];
                const float u = __uint_as_float(e.y), v = __uint_as_float(e.z);
                write_hit(a, base + j, e.w, sqrtf(__uint_as_float(e.x)), u, v);
                if (a.point) a.point[base + j] = contact_point(a.tris, a.gid_leaf[e.w], u, v);
            } else write_point_miss(a, base + j, radius);
        }
        if (a.count) a.count[slot] = (uint8_t)tr.cnt;
    }
};
template <int KMAX, bool FILTER>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(KMAX > 4 ? 3 : 5, 5))) void k_closest_multi(ClosestMultiK a) {
    __shared__ int2 stack[kClosestLds * kTraceBlock];
    __shared__ uint4 hits[KMAX * kTraceBlock];
    point_trace<TravPointMulti<FILTER>>(a, stack, ClosestMultiSink<KMAX>{a, hits});
}

// ---- the triangles that touch a box (art_overlap_boxes) -----------------------------------------------------------------------------------------------
// A query is a closed world-axis box lo.xyz, - | hi.xyz, -: two 16-byte loads a lane, nothing a pool would save, so the loop is the point queries' (point_trace: the idle
// lanes of a wave read the next queries of its chunk).  Nothing orders or shrinks: a child is skipped iff its decoded box misses the query box by comparison
// or is inverted (absent, masked), and the stack holds references alone -- eight a lane in LDS, deeper ones in scratch.  ANY ends at the first candidate; LIST visits every
// leaf whose box meets the query, counts every candidate and keeps the KMAX smallest gids in ascending order in LDS, [entry][lane], 4 bytes an entry: 2 KB of stack and
// 2 KB of list a wave, so LDS bounds nothing (40 waves fit a CU's 160 KB, more than its 32 slots) and one list size serves every K.
// No fmaf in the leaf test: tests/np_overlap.py restates every operation in numpy float32.
struct OverlapK {
    const DevNode4 *wide; const DevTri *tris; const uint32_t *tri_prim, *first_tri;
    const float4 *boxes; float4 *tuv; int2 *ids; uint8_t *hit; uint32_t *count;   // tuv: not used (query_fill's); ids: max_hits records a box, box-major (LIST); hit: a byte a box (ANY); count: may be null
    uint32_t total, chunk, refill, leaf_batch;
    uint32_t *cursors;        // a cast's cursor block
    const uint32_t *bits; const DevShadeTri *shade; const DevPrim *prims; uint32_t cull;   // FILTER instance only, as ClosestK's
    uint32_t max_hits;
};
constexpr int kOverlapLds = 8;                                     // stack references a lane in LDS
static_assert(kOverlapLds == kClosestLds, "kQueryOvf: the loop's scratch stack is what is left of Trav4's bound behind either LDS part");
// one axis of condition 4: p0, p1, p2 the three vertices' projections, rad the box's; min and max by comparisons, so a NaN separates nothing
__device__ __forceinline__ bool axis_separates(float p0, float p1, float p2, float rad) {
    float mn = p0, mx = p0;
    mn = p1 < mn ? p1 : mn; mx = p1 > mx ? p1 : mx;
    mn = p2 < mn ? p2 : mn; mx = p2 > mx ? p2 : mx;
    return (mn > rad) | (mx < -rad);
}
// the three axes e_x, e_y, e_z x f for one edge f: p_m = a_m[j'] * f[i] - a_m[i] * f[j'], rad = h[i] * |f[j']| + h[j'] * |f[i]|, (i, j') = (y, z), (z, x), (x, y)
__device__ __forceinline__ bool edge_separates(V3 a0, V3 a1, V3 a2, V3 h, V3 f) {
    const float ax = fabsf(f.x), ay = fabsf(f.y), az = fabsf(f.z);
    const bool sx = axis_separates(a0.z * f.y - a0.y * f.z, a1.z * f.y - a1.y * f.z, a2.z * f.y - a2.y * f.z, h.y * az + h.z * ay);
    const bool sy = axis_separates(a0.x * f.z - a0.z * f.x, a1.x * f.z - a1.z * f.x, a2.x * f.z - a2.z * f.x, h.z * ax + h.x * az);
    const bool sz = axis_separates(a0.y * f.x - a0.x * f.y, a1.y * f.x - a1.x * f.y, a2.y * f.x - a2.x * f.y, h.x * ay + h.y * ax);
    return sx | sy | sz;
}
// conditions 3 and 4 of DESIGN.md 3.11 (Akenine-Moeller's test) for a triangle v0 e1 e2 against the box lo, hi
__device__ __forceinline__ bool tri_box_overlap(V3 v0, V3 e1, V3 e2, V3 lo, V3 hi) {
    const V3 c = mk(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z);
    const V3 h = mk(0.5f * hi.x - 0.5f * lo.x, 0.5f * hi.y - 0.5f * lo.y, 0.5f * hi.z - 0.5f * lo.z);
    const V3 a0 = v0 - c, a1 = mk(a0.x + e1.x, a0.y + e1.y, a0.z + e1.z), a2 = mk(a0.x + e2.x, a0.y + e2.y, a0.z + e2.z);
    const V3 n = crossp(e1, e2);
    if (fabsf(dotp(n, a0)) > (h.x * fabsf(n.x) + h.y * fabsf(n.y)) + h.z * fabsf(n.z)) return false;
    const V3 f1 = e2 - e1, f2 = mk(-e2.x, -e2.y, -e2.z);
    const bool s0 = edge_separates(a0, a1, a2, h, e1), s1 = edge_separates(a0, a1, a2, h, f1), s2 = edge_separates(a0, a1, a2, h, f2);
    return !(s0 | s1 | s2);
}
template <bool ANY, bool FILTER> struct TravBox {
    V3 lo, hi;
    uint32_t cnt, K;     // cnt: candidates so far, uncapped (ANY: 0 | 1); K: 1..the kernel's KMAX, wave-uniform (LIST)
    uint32_t *list;      // LIST: this lane's entry 0; entry j at list[j * kTraceBlock], the min(cnt, K) smallest gids in ascending order
    int cur, sp;
    __device__ __forceinline__ void push(int ref, int *lds, int *ovf) {
        if (sp < kOverlapLds) lds[sp * kTraceBlock] = ref; else if (sp < kOverlapLds + kQueryOvf) *(volatile int *)&ovf[sp - kOverlapLds] = ref;   // (volatile: TravBase::push)
        sp = min(sp + 1, kOverlapLds + kQueryOvf);
    }
    // the next reference; true: none left, the query is finished
    __device__ __forceinline__ bool pop(int *lds, int *ovf) {
        if (sp == 0) return true;
        sp--;
        if (sp < kOverlapLds) cur = lds[sp * kTraceBlock]; else cur = *(volatile int *)&ovf[sp - kOverlapLds];
        return false;
    }
    // a candidate's gid into the list: it enters while the list is short, or below the K-th entry, which leaves.  (A leaf is visited at most once: no gid arrives twice)
    __device__ __forceinline__ void enter(uint32_t gid) {
        if (cnt >= K && !(gid < list[(K - 1u) * kTraceBlock])) return;
        uint32_t j = min(cnt, K - 1u);
        while (j > 0u) {   // entries above the candidate move up one
            const uint32_t p = list[(j - 1u) * kTraceBlock];
            if (p < gid) break;
            list[j * kTraceBlock] = p; j--;
        }
        list[j * kTraceBlock] = gid;
    }
    // the triangle in `cur`: conditions 1 and 2 on its own box, then the separating axes -- touch(v0, e1, e2): the query's own pair test -- then the masks; ANY is finished by its first candidate
    // (the load of the leaf's record, ta tb tc td, stands in every leaf step of this unit: a helper for it moves k_overlap* and k_closest_tris -- profiles/README.md, "two query units")
    template <class TOUCH> __device__ __forceinline__ bool step_leaf_if(const OverlapK &a, int *lds, int *ovf, const TOUCH &touch) {
        const uint32_t pos = (uint32_t)~cur;
        if (pos == 0x7FFFFFFFu) return pop(lds, ovf);   // kAbsentChild: nothing (TravBase::step_leaf_take)
        const float4 *tq = reinterpret_cast<const float4 *>(a.tris + pos);
        const float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid
        const bool meets = (tc.y < 3.0e38f) & (tc.y <= hi.x) & (lo.x <= td.x) & (tc.z <= hi.y) & (lo.y <= td.y) & (tc.w <= hi.z) & (lo.z <= td.z);
        if (meets && touch(mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x)) &&
            (!FILTER || leaf_visible(a.bits, a.shade, a.prims, a.cull, pos))) {
            if (ANY) { cnt = 1u; return true; }
            enter(__float_as_uint(td.w));
            cnt++;
        }
        return pop(lds, ovf);
    }
    __device__ __forceinline__ bool step_leaf(const OverlapK &a, int *lds, int *ovf) { return step_leaf_if(a, lds, ovf, [this](V3 v0, V3 e1, V3 e2) { return tri_box_overlap(v0, e1, e2, lo, hi); }); }
    // Four box-against-box tests.  A child is skipped iff a comparison says its box misses the query's, or its box is inverted
    // (255 / 0: absent or masked); on with the first that stays, the others wait.  (The order is speed only: nothing here shrinks)
    __device__ __forceinline__ bool step_internal(const DevNode4 *__restrict__ wide, int *lds, int *ovf) {
        const auto [b, c, ox, oy, oz, sx, sy, sz, refs] = load_node4(wide, cur);
        bool h[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {   // (the decode is TravPoint::step_internal_by's, and a copy of it: see there)
            const uint32_t lxq = (b.x >> (8 * i)) & 255u, hxq = (b.w >> (8 * i)) & 255u;
            const float lx = fmaf((float)lxq, sx, ox), hx = fmaf((float)hxq, sx, ox);
            const float ly = fmaf((float)((b.y >> (8 * i)) & 255u), sy, oy), hy = fmaf((float)((c.x >> (8 * i)) & 255u), sy, oy);
            const float lz = fmaf((float)((b.z >> (8 * i)) & 255u), sz, oz), hz = fmaf((float)((c.y >> (8 * i)) & 255u), sz, oz);
            h[i] = (lxq <= hxq) & !((lx > hi.x) | (lo.x > hx) | (ly > hi.y) | (lo.y > hy) | (lz > hi.z) | (lo.z > hz));
        }
        int first = kAbsentChild;
#pragma unroll
        for (int i = 3; i >= 0; i--) {
            if (h[i]) { if (first != kAbsentChild) push(first, lds, ovf); first = refs[i]; }
        }
        if (first == kAbsentChild) return pop(lds, ovf);
        cur = first;
        return false;
    }
};
template <bool ANY, int KMAX> struct OverlapSink {
    const OverlapK &a;
    uint32_t *gids;   // the kernel's __shared__ list array
    template <class TRAV> __device__ __forceinline__ uint32_t init(TRAV &tr) const {
        tr.cnt = 0u;
        tr.K = ANY ? 1u : min(max(a.max_hits, 1u), (uint32_t)KMAX);   // (the host launches KMAX >= K: the clamp keeps every index inside the array whatever it is handed)
        tr.list = &gids[threadIdx.x];
        return tr.K;
    }
    __device__ __forceinline__ void dead(uint32_t sidx, uint32_t K) const {   // a dead query's answer, without a walk: the ANY byte, or K (-1, -1) records and the count
        if (ANY) a.hit[sidx] = 0;
        else {
            const size_t base = (size_t)sidx * K;
            for (uint32_t j = 0; j < K; j++) a.ids[base + j] = make_int2(-1, -1);
            if (a.count) a.count[sidx] = 0u;
        }
    }
    template <class TRAV> __device__ __forceinline__ bool begin(TRAV &tr, uint32_t sidx, uint32_t K, float &) const {
        const float4 q0 = a.boxes[2 * (size_t)sidx], q1 = a.boxes[2 * (size_t)sidx + 1];
        const float z = zero3(q0) + zero3(q1);   // 0 for six finite coordinates, NaN otherwise
        if (z == 0.0f && q0.x <= q1.x && q0.y <= q1.y && q0.z <= q1.z) {
            tr.lo = mk(q0.x, q0.y, q0.z); tr.hi = mk(q1.x, q1.y, q1.z); tr.cnt = 0u; tr.cur = 0; tr.sp = 0;
            return true;
        }
        dead(sidx, K);   // a non-finite coordinate, lo > hi on an axis
        return false;
    }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot, uint32_t K, float) const {
        if (ANY) a.hit[slot] = (uint8_t)tr.cnt;
        else {
            const size_t base = (size_t)slot * K;
            for (uint32_t j = 0; j < K; j++) {
                if (j < tr.cnt) {   // (write_hit's gid -> (primitive, triangle), and a copy of it: one helper for both moves instructions in sixteen instances -- profiles/README.md, "two query units")
                    const uint32_t gid = tr.list[j * kTraceBlock], prim = a.tri_prim[gid];
                    a.ids[base + j] = make_int2((int)prim, (int)(gid - a.first_tri[prim]));
                } else a.ids[base + j] = make_int2(-1, -1);
            }
            if (a.count) a.count[slot] = tr.cnt;
        }
    }
};
// (waves_per_eu 8: the leaf test holds its operands in 64 VGPRs without a spill -- DESIGN.md 3.11's table)
template <bool ANY, int KMAX, bool FILTER>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_overlap(OverlapK a) {
    __shared__ int stack[kOverlapLds * kTraceBlock];
    __shared__ uint32_t gids[(ANY ? 1 : KMAX) * kTraceBlock];
    point_trace<TravBox<ANY, FILTER>>(a, stack, OverlapSink<ANY, KMAX>{a, gids});
}

// ---- the triangles that touch a triangle (art_overlap_triangles) ---------------------------------------------------------------------------------------
// A query is a triangle q0.xyz, - | q1.xyz, - | q2.xyz, -: three 16-byte loads a lane, and the loop, the node step against the query's own box [qlo, qhi], the stack, the
// list and the finish are the box query's (TravBox, OverlapSink) as they stand; what is this query's own are the two hooks -- the fetch (TriSink::begin) and the leaf step
// (TravTri::step_leaf): the triangle's box against [qlo, qhi], then the 17 separating axes of two triangles.  The query's vertices stay in registers beside qlo / qhi
// and the a_m = q_m - v0 are formed at each leaf (DESIGN.md 3.13's table).
// No fmaf in the leaf test: tests/np_tri_overlap.py restates every operation in numpy float32.
struct TriOverlapK : OverlapK { const float4 *qtris; };   // boxes: not used
// one axis x of condition 3: the scene triangle's projections 0, x.e1, x.e2 against the query's x.a0, x.a1, x.a2; min and max by comparisons, so a NaN separates nothing
__device__ __forceinline__ bool tri_axis_separates(V3 x, V3 e1, V3 e2, V3 a0, V3 a1, V3 a2) {
    const float t1 = dotp(x, e1), t2 = dotp(x, e2), p0 = dotp(x, a0), p1 = dotp(x, a1), p2 = dotp(x, a2);
    float tmn = 0.0f, tmx = 0.0f, qmn = p0, qmx = p0;
    tmn = t1 < tmn ? t1 : tmn; tmx = t1 > tmx ? t1 : tmx;
    tmn = t2 < tmn ? t2 : tmn; tmx = t2 > tmx ? t2 : tmx;
    qmn = p1 < qmn ? p1 : qmn; qmx = p1 > qmx ? p1 : qmx;
    qmn = p2 < qmn ? p2 : qmn; qmx = p2 > qmx ? p2 : qmx;
    return (tmn > qmx) | (tmx < qmn);
}
// condition 3 of DESIGN.md 3.13 for a triangle v0 e1 e2 against the query q0 q1 q2: the two normals, the nine edge pairs, the six in-plane axes -- a conjunction, left
// at the first group that separates
__device__ __forceinline__ bool tri_tri_overlap(V3 v0, V3 e1, V3 e2, V3 q0, V3 q1, V3 q2) {
    const V3 a0 = q0 - v0, a1 = q1 - v0, a2 = q2 - v0;
    const V3 f[3] = {e1, e2 - e1, mk(-e2.x, -e2.y, -e2.z)}, g[3] = {a1 - a0, a2 - a1, a0 - a2};
    const V3 n = crossp(e1, e2), m = crossp(g[0], g[1]);
    if (tri_axis_separates(n, e1, e2, a0, a1, a2) || tri_axis_separates(m, e1, e2, a0, a1, a2)) return false;
    bool s = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) s |= tri_axis_separates(crossp(f[i], g[j]), e1, e2, a0, a1, a2);
    }
    if (s) return false;
#pragma unroll
    for (int i = 0; i < 3; i++) s |= tri_axis_separates(crossp(n, f[i]), e1, e2, a0, a1, a2);
#pragma unroll
    for (int j = 0; j < 3; j++) s |= tri_axis_separates(crossp(m, g[j]), e1, e2, a0, a1, a2);
    return !s;
}
// TravBox with the query's vertices beside its box (lo, hi: qlo, qhi) and a pair test of its own in the leaf step; push, pop, enter and step_internal are TravBox's
template <bool ANY, bool FILTER> struct TravTri : TravBox<ANY, FILTER> {
    V3 q0, q1, q2;
    __device__ __forceinline__ bool step_leaf(const TriOverlapK &a, int *lds, int *ovf) { return this->step_leaf_if(a, lds, ovf, [this](V3 v0, V3 e1, V3 e2) { return tri_tri_overlap(v0, e1, e2, q0, q1, q2); }); }
};
// a query triangle into a walk that has q0, q1, q2, lo, hi: three 16-byte loads, the vertices and their box [qlo, qhi]; w3: word 3 as given (art_closest_triangles'
// radius; the overlap query does not read it).  False: a dead query (a non-finite coordinate among the nine), whose walk state is left as it was
template <class TRAV> __device__ __forceinline__ bool read_tri(const float4 *qtris, uint32_t sidx, TRAV &tr, float &w3) {
    const float4 r0 = qtris[3 * (size_t)sidx], r1 = qtris[3 * (size_t)sidx + 1], r2 = qtris[3 * (size_t)sidx + 2];
    const float z = (zero3(r0) + zero3(r1)) + zero3(r2);   // 0 for nine finite coordinates, NaN otherwise
    w3 = r0.w;
    if (z == 0.0f) {
        V3 mn = mk(r0.x, r0.y, r0.z), mx = mn;   // qlo, qhi: two selects an axis from the first vertex
        mn.x = r1.x < mn.x ? r1.x : mn.x; mn.y = r1.y < mn.y ? r1.y : mn.y; mn.z = r1.z < mn.z ? r1.z : mn.z;
        mx.x = r1.x > mx.x ? r1.x : mx.x; mx.y = r1.y > mx.y ? r1.y : mx.y; mx.z = r1.z > mx.z ? r1.z : mx.z;
        mn.x = r2.x < mn.x ? r2.x : mn.x; mn.y = r2.y < mn.y ? r2.y : mn.y; mn.z = r2.z < mn.z ? r2.z : mn.z;
        mx.x = r2.x > mx.x ? r2.x : mx.x; mx.y = r2.y > mx.y ? r2.y : mx.y; mx.z = r2.z > mx.z ? r2.z : mx.z;
        tr.q0 = mk(r0.x, r0.y, r0.z); tr.q1 = mk(r1.x, r1.y, r1.z); tr.q2 = mk(r2.x, r2.y, r2.z);
        tr.lo = mn; tr.hi = mx;
        return true;
    }
    return false;
}
// OverlapSink with the fetch of a triangle: init, finish and a dead query's answer are the box query's
template <bool ANY, int KMAX> struct TriSink : OverlapSink<ANY, KMAX> {
    const float4 *qtris;
    template <class TRAV> __device__ __forceinline__ bool begin(TRAV &tr, uint32_t sidx, uint32_t K, float &) const {
        float w3;
        if (read_tri(qtris, sidx, tr, w3)) { tr.cnt = 0u; tr.cur = 0; tr.sp = 0; return true; }
        this->dead(sidx, K);   // a non-finite coordinate
        return false;
    }
};
// (waves_per_eu: ANY holds the 17 axes' operands in 64 VGPRs without a spill; LIST, with the list's state beside them, spills two of them at 8 waves and uses
// 75 / 76 without a spill at 6, no more at 5 or 4 -- DESIGN.md 3.13's table)
template <bool ANY, int KMAX, bool FILTER>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(ANY ? 8 : 6, ANY ? 8 : 6))) void k_overlap_tris(TriOverlapK a) {
    __shared__ int stack[kOverlapLds * kTraceBlock];
    __shared__ uint32_t gids[(ANY ? 1 : KMAX) * kTraceBlock];
    point_trace<TravTri<ANY, FILTER>>(a, stack, TriSink<ANY, KMAX>{{a, gids}, a.qtris});
}

// ---- the distance from a triangle to the scene (art_closest_triangles) ----------------------------------------------------------------------------------
// A query is art_overlap_triangles' triangle with a radius in word 3, and the answer art_closest_points' record for a triangle in place of a point: the walk is TravPoint's
// -- its stack of (reference, distance) pairs, push, pop, the five-comparator child order (step_internal_by) and the hook of its leaf step's tie rule -- with the
// squared distance between the query's box [qlo, qhi] and a box where the point's box_d2 stood.  What is this query's own: that distance (boxes_d2), the clamped
// segment pair (seg_seg) and the fifteen features of a pair of triangles (tri_tri_closest); tri_closest, tri_tri_overlap and the fetch (read_tri) are the one copy above.
// No fmaf in anything that decides a record: tests/np_tri_distance.py restates every operation in numpy float32.
// [lo, hi] against [tlo, thi]: per axis max(max(tlo - hi, lo - thi), 0) by selects, summed (x^2 + y^2) + z^2
__device__ __forceinline__ float boxes_d2(V3 lo, V3 hi, float lx, float ly, float lz, float hx, float hy, float hz) {
    const float ax = lx - hi.x, bx = lo.x - hx, ay = ly - hi.y, by = lo.y - hy, az = lz - hi.z, bz = lo.z - hz;
    float ex = bx > ax ? bx : ax, ey = by > ay ? by : ay, ez = bz > az ? bz : az;
    ex = ex > 0.0f ? ex : 0.0f; ey = ey > 0.0f ? ey : 0.0f; ez = ez > 0.0f ? ez : 0.0f;
    return (ex * ex + ey * ey) + ez * ez;
}
__device__ __forceinline__ float clamp01(float x) { x = x > 0.0f ? x : 0.0f; return x < 1.0f ? x : 1.0f; }   // (two selects: a NaN becomes 0, seg_param's rule)
// the nearest points of the segments {p1 + s d1} and {p2 + t d2}, 0 <= s, t <= 1 (Ericson 5.1.9, every divisor guarded as seg_param's): r = p1 - p2.  -> their squared distance
__device__ __forceinline__ float seg_seg(V3 p1, V3 d1, V3 p2, V3 d2, float &s, float &t) {
    const V3 r = p1 - p2;
    const float a = dotp(d1, d1), e = dotp(d2, d2), f = dotp(d2, r), c = dotp(d1, r), b = dotp(d1, d2);
    const float den = a * e - b * b, qa = a > 0.0f ? a : 1.0f;
    s = clamp01((b * f - c * e) / (den > 0.0f ? den : 1.0f));
    s = den > 0.0f ? s : 0.0f;
    s = a > 0.0f ? s : 0.0f;
    t = (b * s + f) / (e > 0.0f ? e : 1.0f);
    t = e > 0.0f ? t : 0.0f;
    const float s0 = clamp01(-c / qa), s1 = clamp01((b - c) / qa);
    s = t < 0.0f ? s0 : s; s = t > 1.0f ? s1 : s;
    s = a > 0.0f ? s : 0.0f;
    t = clamp01(t);
    const float dx = (p1.x + s * d1.x) - (p2.x + t * d2.x), dy = (p1.y + s * d1.y) - (p2.y + t * d2.y), dz = (p1.z + s * d1.z) - (p2.z + t * d2.z);
    return (dx * dx + dy * dy) + dz * dz;
}
// The features of DESIGN.md 3.14 for the scene triangle v0 e1 e2 and the query q0 q1 q2 in their order, the first of the smallest winning: the query's vertices against
// the triangle, the triangle's vertices against the query, the nine edge pairs, scene edge outermost.  u, v: the scene side's barycentrics of the winning pair of
// points; s, t: the query side's.  +inf: no feature gave a number
__device__ __forceinline__ float tri_tri_closest(V3 v0, V3 e1, V3 e2, V3 q0, V3 q1, V3 q2, float &u, float &v, float &s, float &t) {
    float best = INFINITY, cu, cv; u = 0.0f; v = 0.0f; s = 0.0f; t = 0.0f;
    const V3 g1 = q1 - q0, g2 = q2 - q0;
    float d = tri_closest(q0 - v0, e1, e2, cu, cv);
    if (d < best) { best = d; u = cu; v = cv; s = 0.0f; t = 0.0f; }
    d = tri_closest(q1 - v0, e1, e2, cu, cv);
    if (d < best) { best = d; u = cu; v = cv; s = 1.0f; t = 0.0f; }
    d = tri_closest(q2 - v0, e1, e2, cu, cv);
    if (d < best) { best = d; u = cu; v = cv; s = 0.0f; t = 1.0f; }
    const V3 v1 = mk(v0.x + e1.x, v0.y + e1.y, v0.z + e1.z), v2 = mk(v0.x + e2.x, v0.y + e2.y, v0.z + e2.z);
    d = tri_closest(v0 - q0, g1, g2, cu, cv);
    if (d < best) { best = d; u = 0.0f; v = 0.0f; s = cu; t = cv; }
    d = tri_closest(v1 - q0, g1, g2, cu, cv);
    if (d < best) { best = d; u = 1.0f; v = 0.0f; s = cu; t = cv; }
    d = tri_closest(v2 - q0, g1, g2, cu, cv);
    if (d < best) { best = d; u = 0.0f; v = 1.0f; s = cu; t = cv; }
    const V3 sp[3] = {v0, v0, v1}, sd[3] = {e1, e2, e2 - e1}, qp[3] = {q0, q0, mk(q0.x + g1.x, q0.y + g1.y, q0.z + g1.z)}, qd[3] = {g1, g2, g2 - g1};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            d = seg_seg(sp[i], sd[i], qp[j], qd[j], cu, cv);
            if (d < best) {   // the parameters as barycentrics: edge 0 is (x, 0), edge 1 (0, x), edge 2 (1 - x, x)
                best = d;
                u = i == 0 ? cu : (i == 1 ? 0.0f : 1.0f - cu); v = i == 0 ? 0.0f : cu;
                s = j == 0 ? cv : (j == 1 ? 0.0f : 1.0f - cv); t = j == 0 ? 0.0f : cv;
            }
        }
    }
    return best;
}
// d2_tri of DESIGN.md 3.14: 0 where the 17 axes say the two touch or cut (asked only while the features are above 0: the result is the same), else the winning feature's
// distance; the witnesses are the winning feature's either way.  Where no feature gave a number (a non-finite triangle, which no axis separates either) it stays +inf
__device__ __forceinline__ float tri_tri_d2(V3 v0, V3 e1, V3 e2, V3 q0, V3 q1, V3 q2, float &u, float &v, float &s, float &t) {
    const float d = tri_tri_closest(v0, e1, e2, q0, q1, q2, u, v, s, t);
    return (d > 0.0f && d < INFINITY && tri_tri_overlap(v0, e1, e2, q0, q1, q2)) ? 0.0f : d;
}
struct TriDistanceK : ClosestK { const float4 *qtris; float4 *qpoint; };   // points: not used; qpoint: may be null
// TravPoint with the query's vertices and box where its point stood: push, pop and the child order are TravPoint's; the node step asks boxes_d2, and the leaf step is its own
template <bool FILTER> struct TravTriDist : TravPoint<FILTER> {
    V3 q0, q1, q2, lo, hi;   // (TravPoint's p is not used here, and its step_internal and step_leaf are shadowed by the two below)
    float bs, bt;   // the best candidate's barycentrics on the query
    __device__ __forceinline__ bool step_internal(const DevNode4 *__restrict__ wide, int2 *lds, int *ovf) {
        return this->step_internal_by(wide, lds, ovf, [this](float lx, float ly, float lz, float hx, float hy, float hz) { return boxes_d2(lo, hi, lx, ly, lz, hx, hy, hz); });
    }
    // the triangle in `cur`: its own box first (box_d2 > limit: d2_eff is at least that, nothing to take), then the features and the 17 axes, then TravPoint's tie rule and the masks
    __device__ __forceinline__ bool step_leaf(const TriDistanceK &a, int2 *lds, int *ovf) {
        const uint32_t pos = (uint32_t)~this->cur;
        if (pos == 0x7FFFFFFFu) return this->pop(lds, ovf);   // kAbsentChild: nothing (TravBase::step_leaf_take)
        const float4 *tq = reinterpret_cast<const float4 *>(a.tris + pos);
        const float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid
        const float bd = boxes_d2(lo, hi, tc.y, tc.z, tc.w, td.x, td.y, td.z);
        if ((tc.y < 3.0e38f) & !(bd > this->limit)) {
            float u, v, s, t;
            const float dt = tri_tri_d2(mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), q0, q1, q2, u, v, s, t);
            if ((dt < INFINITY) & (bd < INFINITY)) {   // the parts, not the maximum (TravPoint::step_leaf_take)
                const float de = bd > dt ? bd : dt;
                const uint32_t gid = __float_as_uint(td.w);
                if ((de < this->limit || (de == this->limit && gid < this->bgid)) && (!FILTER || leaf_visible(a.bits, a.shade, a.prims, a.cull, pos))) {
                    this->limit = de; this->bu = u; this->bv = v; this->bpos = pos; this->bgid = gid; bs = s; bt = t;
                }
            }
        }
        return this->pop(lds, ovf);
    }
};
// The walk carries the query side's (s, t) of its best candidate (bs, bt) beside limit, u, v, pos and gid: 123 VGPRs.  A finish that evaluates the winning pair once more
// for them instead holds the fifteen features a second time and comes out at 133 (DESIGN.md 3.14's table has both figures)
struct TriDistanceSink {
    const TriDistanceK &a;
    template <class I> __device__ __forceinline__ void miss(I at, float r) const {
        write_point_miss(a, at, r);
        if (a.qpoint) a.qpoint[at] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    template <class TRAV> __device__ __forceinline__ uint32_t init(TRAV &) const { return 1u; }
    template <class TRAV> __device__ __forceinline__ bool begin(TRAV &tr, uint32_t sidx, uint32_t, float &radius) const {
        float r;
        if (read_tri(a.qtris, sidx, tr, r) && r == r && !(r < 0.0f)) { best_start(tr, r); radius = r; return true; }   // a NaN or negative radius: read_point's rule
        miss(sidx, r);
        return false;
    }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot, uint32_t, float radius) const {
        if (tr.bgid != kNoHit) {
            best_write(a, tr, slot);
            if (a.qpoint) {
                const float s = tr.bs, t = tr.bt;
                const V3 g1 = tr.q1 - tr.q0, g2 = tr.q2 - tr.q0;
                a.qpoint[slot] = make_float4(tr.q0.x + (s * g1.x + t * g2.x), tr.q0.y + (s * g1.y + t * g2.y), tr.q0.z + (s * g1.z + t * g2.z), 1.0f);
            }
        } else miss(slot, radius);
    }
};
// (waves_per_eu 4: the fifteen features and the 17 axes hold 123 VGPRs without a spill; at 5 waves (96) the compiler spills 85 of them to scratch -- DESIGN.md
// 3.14's table)
template <bool FILTER>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_closest_tris(TriDistanceK a) {
    __shared__ int2 stack[kClosestLds * kTraceBlock];
    point_trace<TravTriDist<FILTER>>(a, stack, TriDistanceSink{a});
}

// ---- a triangle along a ray (art_cast_triangles) ---------------------------------------------------------------------------------------------------------
// A query is art_overlap_triangles' triangle with a displacement: q0.xyz, tmin | q1.xyz, tmax | q2.xyz, - | d.xyz, - -- four 16-byte loads a lane and more state than
// pooled_trace's twelve pool fields hold, so the loop is point_trace and the stack TravPoint's pairs, (reference, the child's entry time): tbest (`limit`) only ever falls,
// and an entry whose box is entered behind it by the time it is popped is dropped without a fetch.  The node step is TravSweep's sign-selected slab of the ray (0, d) with
// each child's low planes moved by -qhi and its high planes by -qlo (the box of scene point minus query point); the leaf step runs that slab on the triangle's own box
// against tbest, then the fifteen moving features -- three query vertices against the scene face, three scene vertices against the query face, nine edge pairs -- and the 17
// axes at pose tmin (S).  S is first in 3.15's order and nothing is earlier than tmin: asked last, it replaces whatever the features found, which is the same answer.
// Its witnesses (3.14's tri_tri_closest at pose tmin) are made once, at the finish, for a winner flagged S (bit 31 of bpos: no leaf sits there).
// No fmaf in anything that decides a record: tests/np_tri_sweep.py restates every operation in numpy float32 (the slab's fmaf has a zero addend here: a product).
struct TriCastK : ClosestK { const float4 *sweeps; float4 *qpoint; };   // points: not used; qpoint: may be null
constexpr uint32_t kStartFlag = 0x80000000u;
__device__ __forceinline__ void cast_take(bool ok, float t, float cu, float cv, float cs, float ct, float tmin, float tmax, float &bt, float &u, float &v, float &s, float &tt) {
    if (ok & (t >= tmin) & (t < tmax) & (t < bt)) { bt = t; u = cu; v = cv; s = cs; tt = ct; }   // (a NaN never wins)
}
// a vertex against a face: the ray (w0 + face origin, d) against the triangle (0, e1, e2) with the normal n, nn = n.n; fu, fv: 3.9's face barycentrics of where it meets the plane
__device__ __forceinline__ bool cast_vertex_face(V3 w0, V3 d, V3 e1, V3 e2, V3 n, float nn, float nd, float &t, float &fu, float &fv) {
    t = -dotp(n, w0) / (nd != 0.0f ? nd : 1.0f);
    const V3 w = mk(w0.x + t * d.x, w0.y + t * d.y, w0.z + t * d.z);
    const float den = nn > 0.0f ? nn : 1.0f;
    fu = dotp(crossp(w, e2), n) / den; fv = dotp(crossp(e1, w), n) / den;
    return (nn > 0.0f) & (nd != 0.0f) & (fu >= 0.0f) & (fv >= 0.0f) & (fu + fv <= 1.0f);
}
// t_tri of DESIGN.md 3.15 without S, for the scene triangle v0 e1 e2 and the query q0 q1 q2 moving by d: the smallest t in [tmin, tmax) among QV0..2, SV0..2 and the nine
// edge pairs, scene edge outermost, the first of equals; +inf: none.  u, v: its barycentrics on the scene triangle; s, tt: on the query
__device__ __forceinline__ float tri_tri_cast(V3 v0, V3 e1, V3 e2, V3 q0, V3 q1, V3 q2, V3 d, float tmin, float tmax, float &u, float &v, float &s, float &tt) {
    float bt = INFINITY, t, fu, fv; u = 0.0f; v = 0.0f; s = 0.0f; tt = 0.0f;
    const V3 g1 = q1 - q0, g2 = q2 - q0;
    {
        const V3 n = crossp(e1, e2);
        const float nn = dotp(n, n), nd = dotp(n, d);
        bool ok = cast_vertex_face(q0 - v0, d, e1, e2, n, nn, nd, t, fu, fv); cast_take(ok, t, fu, fv, 0.0f, 0.0f, tmin, tmax, bt, u, v, s, tt);
        ok = cast_vertex_face(q1 - v0, d, e1, e2, n, nn, nd, t, fu, fv); cast_take(ok, t, fu, fv, 1.0f, 0.0f, tmin, tmax, bt, u, v, s, tt);
        ok = cast_vertex_face(q2 - v0, d, e1, e2, n, nn, nd, t, fu, fv); cast_take(ok, t, fu, fv, 0.0f, 1.0f, tmin, tmax, bt, u, v, s, tt);
    }
    const V3 v1 = mk(v0.x + e1.x, v0.y + e1.y, v0.z + e1.z), v2 = mk(v0.x + e2.x, v0.y + e2.y, v0.z + e2.z);
    {
        const V3 n = crossp(g1, g2), nd_ = mk(-d.x, -d.y, -d.z);
        const float nn = dotp(n, n), nd = dotp(n, nd_);
        bool ok = cast_vertex_face(v0 - q0, nd_, g1, g2, n, nn, nd, t, fu, fv); cast_take(ok, t, 0.0f, 0.0f, fu, fv, tmin, tmax, bt, u, v, s, tt);
        ok = cast_vertex_face(v1 - q0, nd_, g1, g2, n, nn, nd, t, fu, fv); cast_take(ok, t, 1.0f, 0.0f, fu, fv, tmin, tmax, bt, u, v, s, tt);
        ok = cast_vertex_face(v2 - q0, nd_, g1, g2, n, nn, nd, t, fu, fv); cast_take(ok, t, 0.0f, 1.0f, fu, fv, tmin, tmax, bt, u, v, s, tt);
    }
    const V3 sp[3] = {v0, v0, v1}, sd[3] = {e1, e2, e2 - e1}, qp[3] = {q0, q0, mk(q0.x + g1.x, q0.y + g1.y, q0.z + g1.z)}, qd[3] = {g1, g2, g2 - g1};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const V3 n = crossp(sd[i], qd[j]), r0 = sp[i] - qp[j];
            const float nn = dotp(n, n), nd = dotp(n, d), den = nn > 0.0f ? nn : 1.0f;
            t = dotp(n, r0) / (nd != 0.0f ? nd : 1.0f);
            const V3 m = mk(r0.x - t * d.x, r0.y - t * d.y, r0.z - t * d.z);
            const float se = -dotp(crossp(m, qd[j]), n) / den, sq = -dotp(crossp(m, sd[i]), n) / den;
            const bool ok = (nn > 0.0f) & (nd != 0.0f) & (se >= 0.0f) & (se <= 1.0f) & (sq >= 0.0f) & (sq <= 1.0f);
            // the parameters as barycentrics (tri_tri_closest): edge 0 is (x, 0), edge 1 (0, x), edge 2 (1 - x, x)
            cast_take(ok, t, i == 0 ? se : (i == 1 ? 0.0f : 1.0f - se), i == 0 ? 0.0f : se, j == 0 ? sq : (j == 1 ? 0.0f : 1.0f - sq), j == 0 ? 0.0f : sq, tmin, tmax, bt, u, v, s, tt);
        }
    }
    return bt;
}
// TravPoint's stack of pairs and its tie rule with a swept triangle where its point stood: limit is tbest, the pairs' second word a box's entry time
template <bool FILTER> struct TravTriCast : TravPoint<FILTER> {
    V3 q0, q1, q2, lo, hi, d, inv;   // (TravPoint's p is not used here, and its step_internal and step_leaf are shadowed by the two below)
    float tmin, tmax, bs, bt;        // bs, bt: the best candidate's barycentrics on the query
    // the triangle in `cur`: its own box, shifted, against tbest first -- an exact cull: a candidate's t_eff is at least its box's entry and at least tmin -- then the features
    __device__ __forceinline__ bool step_leaf(const TriCastK &a, int2 *lds, int *ovf) {
        const uint32_t pos = (uint32_t)~this->cur;
        if (pos == 0x7FFFFFFFu) return this->pop(lds, ovf);   // kAbsentChild: nothing (TravBase::step_leaf_take)
        const float4 *tq = reinterpret_cast<const float4 *>(a.tris + pos);
        const float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid
        const float t0x = (tc.y - hi.x) * inv.x, t1x = (td.x - lo.x) * inv.x, t0y = (tc.z - hi.y) * inv.y, t1y = (td.y - lo.y) * inv.y, t0z = (tc.w - hi.z) * inv.z, t1z = (td.z - lo.z) * inv.z;
        const float te = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z)), tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
        if ((tc.y < 3.0e38f) & (fmaxf(te, tmin) <= fminf(tf, this->limit))) {
            const V3 v0 = mk(ta.x, ta.y, ta.z), e1 = mk(ta.w, tb.x, tb.y), e2 = mk(tb.z, tb.w, tc.x);
            float u, v, s, t;
            float tt = tri_tri_cast(v0, e1, e2, q0, q1, q2, d, tmin, tmax, u, v, s, t);
            bool start = false;
            if ((tmin < tmax) && tri_tri_overlap(v0, e1, e2, mk(q0.x + tmin * d.x, q0.y + tmin * d.y, q0.z + tmin * d.z), mk(q1.x + tmin * d.x, q1.y + tmin * d.y, q1.z + tmin * d.z),
                                                 mk(q2.x + tmin * d.x, q2.y + tmin * d.y, q2.z + tmin * d.z))) { tt = tmin; start = true; }
            if (tt < INFINITY) {
                const float teff = fmaxf(tt, te);
                const uint32_t gid = __float_as_uint(td.w);
                if ((teff < this->limit || (teff == this->limit && gid < this->bgid)) && (!FILTER || leaf_visible(a.bits, a.shade, a.prims, a.cull, pos))) {
                    this->limit = teff; this->bu = u; this->bv = v; this->bpos = start ? pos | kStartFlag : pos; this->bgid = gid; bs = s; bt = t;
                }
            }
        }
        return this->pop(lds, ovf);
    }
    // TravSweep's sign-selected slab, o = 0, with each child's near and far planes shifted by the query's box.  An absent child or a masked subtree carries an inverted byte
    // box (255 / 0): "left before it is entered" does not hold once the planes have moved, so it is skipped by TravPoint's explicit test.  A child is skipped iff
    // max(tn, tmin) > min(tf, tbest); on with the one entered first, the others wait with their entry times, the last at the bottom (TravPoint's order; speed only)
    __device__ __forceinline__ bool step_internal(const DevNode4 *__restrict__ wide, int2 *lds, int *ovf) {
        const auto [b, c, ox, oy, oz, sx, sy, sz, refs] = load_node4(wide, this->cur);
        const bool ngx = inv.x < 0.0f, ngy = inv.y < 0.0f, ngz = inv.z < 0.0f;
        const uint32_t nxw = ngx ? b.w : b.x, fxw = ngx ? b.x : b.w, nyw = ngy ? c.x : b.y, fyw = ngy ? b.y : c.x, nzw = ngz ? c.y : b.z, fzw = ngz ? b.z : c.y;
        const float pnx = ngx ? lo.x : hi.x, pfx = ngx ? hi.x : lo.x, pny = ngy ? lo.y : hi.y, pfy = ngy ? hi.y : lo.y, pnz = ngz ? lo.z : hi.z, pfz = ngz ? hi.z : lo.z;   // what the near and the far plane move by
        const float lim = this->limit;
        float k[4]; int rf[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float tnx = (fmaf((float)((nxw >> (8 * i)) & 255u), sx, ox) - pnx) * inv.x, tfx = (fmaf((float)((fxw >> (8 * i)) & 255u), sx, ox) - pfx) * inv.x;
            const float tny = (fmaf((float)((nyw >> (8 * i)) & 255u), sy, oy) - pny) * inv.y, tfy = (fmaf((float)((fyw >> (8 * i)) & 255u), sy, oy) - pfy) * inv.y;
            const float tnz = (fmaf((float)((nzw >> (8 * i)) & 255u), sz, oz) - pnz) * inv.z, tfz = (fmaf((float)((fzw >> (8 * i)) & 255u), sz, oz) - pfz) * inv.z;
            const float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
            const bool h = (((b.x >> (8 * i)) & 255u) <= ((b.w >> (8 * i)) & 255u)) & (fmaxf(tn, tmin) <= fminf(tf, lim));
            k[i] = h ? tn : INFINITY; rf[i] = h ? refs[i] : kAbsentChild;
        }
        // (TravPoint::step_internal_by's five comparators, and a copy of them: a child that is out sorts as +inf with the absent reference, which is pushed nowhere)
#define ART_CSWAP(x, y) { const bool sw = k[y] < k[x]; const float tk = sw ? k[x] : k[y]; k[x] = sw ? k[y] : k[x]; k[y] = tk; const int tr_ = sw ? rf[x] : rf[y]; rf[x] = sw ? rf[y] : rf[x]; rf[y] = tr_; }
        ART_CSWAP(0, 1) ART_CSWAP(2, 3) ART_CSWAP(0, 2) ART_CSWAP(1, 3) ART_CSWAP(1, 2)
#undef ART_CSWAP
#pragma unroll
        for (int i = 3; i >= 1; i--) if (rf[i] != kAbsentChild) this->push(rf[i], k[i], lds, ovf);
        if (rf[0] == kAbsentChild) return this->pop(lds, ovf);   // (a child entered at +inf -- a structure nowhere -- sorts among the absent ones: it was pushed, and comes back here)
        this->cur = rf[0];
        return false;
    }
};
struct TriCastSink {
    const TriCastK &a;
    template <class I> __device__ __forceinline__ void miss(I at, float x) const {
        write_point_miss(a, at, x);
        if (a.qpoint) a.qpoint[at] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    template <class TRAV> __device__ __forceinline__ uint32_t init(TRAV &) const { return 1u; }
    // `radius`, the loop's one float for the finish, carries nothing here: the walk keeps tmax
    template <class TRAV> __device__ __forceinline__ bool begin(TRAV &tr, uint32_t sidx, uint32_t, float &) const {
        const float4 r0 = a.sweeps[4 * (size_t)sidx], r1 = a.sweeps[4 * (size_t)sidx + 1], r2 = a.sweeps[4 * (size_t)sidx + 2], r3 = a.sweeps[4 * (size_t)sidx + 3];
        const float z = ((zero3(r0) + zero3(r1)) + zero3(r2)) + zero3(r3);   // 0 for twelve finite values, NaN otherwise
        if (z == 0.0f && r1.w == r1.w) {
            V3 mn = mk(r0.x, r0.y, r0.z), mx = mn;   // qlo, qhi: read_tri's selects
            mn.x = r1.x < mn.x ? r1.x : mn.x; mn.y = r1.y < mn.y ? r1.y : mn.y; mn.z = r1.z < mn.z ? r1.z : mn.z;
            mx.x = r1.x > mx.x ? r1.x : mx.x; mx.y = r1.y > mx.y ? r1.y : mx.y; mx.z = r1.z > mx.z ? r1.z : mx.z;
            mn.x = r2.x < mn.x ? r2.x : mn.x; mn.y = r2.y < mn.y ? r2.y : mn.y; mn.z = r2.z < mn.z ? r2.z : mn.z;
            mx.x = r2.x > mx.x ? r2.x : mx.x; mx.y = r2.y > mx.y ? r2.y : mx.y; mx.z = r2.z > mx.z ? r2.z : mx.z;
            tr.q0 = mk(r0.x, r0.y, r0.z); tr.q1 = mk(r1.x, r1.y, r1.z); tr.q2 = mk(r2.x, r2.y, r2.z); tr.lo = mn; tr.hi = mx;
            tr.d = mk(r3.x, r3.y, r3.z); tr.inv = mk(1.0f / safe_dir(r3.x), 1.0f / safe_dir(r3.y), 1.0f / safe_dir(r3.z));   // ray_init's operations
            tr.tmin = r0.w; tr.tmax = r1.w;
            tr.limit = r1.w; tr.bu = 0.f; tr.bv = 0.f; tr.bpos = kNoHit; tr.bgid = kNoHit; tr.cur = 0; tr.sp = 0;
            return true;
        }
        miss(sidx, r1.w);   // a dead query: its miss record, without a walk
        return false;
    }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot, uint32_t, float) const {
        if (tr.bgid != kNoHit) {
            const uint32_t pos = tr.bpos & ~kStartFlag;
            float u = tr.bu, v = tr.bv, s = tr.bs, t = tr.bt;
            if (tr.bpos & kStartFlag) {   // S: the witnesses of the pose at tmin
                const float4 *tq = reinterpret_cast<const float4 *>(a.tris + pos);
                const float4 ta = tq[0], tb = tq[1], tc = tq[2];
                const float tm = tr.tmin;
                (void)tri_tri_closest(mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), mk(tr.q0.x + tm * tr.d.x, tr.q0.y + tm * tr.d.y, tr.q0.z + tm * tr.d.z),
                                      mk(tr.q1.x + tm * tr.d.x, tr.q1.y + tm * tr.d.y, tr.q1.z + tm * tr.d.z), mk(tr.q2.x + tm * tr.d.x, tr.q2.y + tm * tr.d.y, tr.q2.z + tm * tr.d.z), u, v, s, t);
            }
            write_hit(a, slot, tr.bgid, tr.limit, u, v);
            if (a.point) a.point[slot] = contact_point(a.tris, pos, u, v);
            if (a.qpoint) {
                const V3 g1 = tr.q1 - tr.q0, g2 = tr.q2 - tr.q0;
                a.qpoint[slot] = make_float4(tr.q0.x + (s * g1.x + t * g2.x), tr.q0.y + (s * g1.y + t * g2.y), tr.q0.z + (s * g1.z + t * g2.z), 1.0f);
            }
        } else miss(slot, tr.tmax);
    }
};
// (waves_per_eu 4: the fifteen moving features and the 17 axes hold 118 VGPRs without a spill; at 5 waves (96) the compiler spills 33 of them to scratch, at 6 (80) 56; at 3
// it uses no more than at 4 -- DESIGN.md 3.15's table)
template <bool FILTER>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_cast_tris(TriCastK a) {
    __shared__ int2 stack[kClosestLds * kTraceBlock];
    point_trace<TravTriCast<FILTER>>(a, stack, TriCastSink{a});
}

template <class K> static void mask_fill(K &a, const QueryArgs &c) { a.bits = c.alpha_bits; a.shade = c.shade; a.prims = c.prims; a.cull = c.cull; }   // the four fields of every FILTER instance
template <class K> static K closest_fill(const ClosestArgs &c) {
    K a = query_fill<K>(c);
    a.points = c.points; a.point = c.point; mask_fill(a, c);
    return a;
}
template <class K> static K overlap_fill(const OverlapArgs &c) {
    K a = query_fill<K>(c);
    a.hit = c.hit; a.count = c.count; a.max_hits = c.max_hits; mask_fill(a, c);
    return a;
}
void launch_closest(const ClosestArgs &c, hipStream_t s) {
    launch_query(c.filter ? k_closest<true> : k_closest<false>, closest_fill<ClosestK>(c), c, s);
}
void launch_closest_multi(const ClosestMultiArgs &c, hipStream_t s) {   // the instance with the smallest list that holds K
    ClosestMultiK a = closest_fill<ClosestMultiK>(c); a.count = c.count; a.gid_leaf = c.gid_leaf; a.max_hits = c.max_hits;
    launch_query(c.max_hits <= 4u ? (c.filter ? k_closest_multi<4, true> : k_closest_multi<4, false>) : (c.filter ? k_closest_multi<8, true> : k_closest_multi<8, false>), a, c, s);
}
void launch_overlap(const OverlapArgs &c, hipStream_t s) {   // one list size: ART_CAST_MAX_HITS gids a lane are 2 KB of LDS a wave, which bounds nothing
    static_assert(ART_CAST_MAX_HITS == 8u, "k_overlap's list");
    OverlapK a = overlap_fill<OverlapK>(c); a.boxes = c.boxes;
    if (c.any) launch_query(c.filter ? k_overlap<true, 0, true> : k_overlap<true, 0, false>, a, c, s);
    else launch_query(c.filter ? k_overlap<false, 8, true> : k_overlap<false, 8, false>, a, c, s);
}
void launch_tri_overlap(const TriOverlapArgs &c, hipStream_t s) {   // launch_overlap's instances and list size
    TriOverlapK a = overlap_fill<TriOverlapK>(c); a.qtris = c.qtris;
    if (c.any) launch_query(c.filter ? k_overlap_tris<true, 0, true> : k_overlap_tris<true, 0, false>, a, c, s);
    else launch_query(c.filter ? k_overlap_tris<false, 8, true> : k_overlap_tris<false, 8, false>, a, c, s);
}
void launch_tri_distance(const TriDistanceArgs &c, hipStream_t s) {
    TriDistanceK a = closest_fill<TriDistanceK>(c); a.qtris = c.qtris; a.qpoint = c.qpoint;
    launch_query(c.filter ? k_closest_tris<true> : k_closest_tris<false>, a, c, s);
}
void launch_tri_cast(const TriCastArgs &c, hipStream_t s) {
    TriCastK a = closest_fill<TriCastK>(c); a.sweeps = c.sweeps; a.qpoint = c.qpoint;
    launch_query(c.filter ? k_cast_tris<true> : k_cast_tris<false>, a, c, s);
}

} // namespace art
