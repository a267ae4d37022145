// art_query.h -- what the kernels of both wave loops of the queries on device buffers share (gfx950), once: the ray read, the hit and miss records, the contact point, the mask test and the 4-wide node's
// decode (load_node4); the sorted list of both K-walks (KList), which a walk fills through its leaf step's hook for a candidate's fate (step_leaf_take: one leaf step a walk); the unfused geometry k_sweep and
// the point walks both use; at the bottom the arguments' common fields and the launch.  Included by art_query_rays.hip (art_walk.h's pooled loop) and art_query_points.hip (point_trace).  (The list, the leaf
// steps and the loop were copies once: what folding them moved -- tools/kernel_diff.py -- is in profiles/README.md, "one list, one hook", "one point loop" and "two query units".)  art_cast.hip is their host side.
#pragma once
#include "art_walk.h"

namespace art {

// One ray of a cast's buffer: two 16-byte loads a lane (2 KB a wave in one piece), o.xyz tmin | d.xyz tmax.  False: a dead ray (non-finite origin or direction, NaN
// tmax: TravBase::start's rule), which accepts nothing -- its source writes the miss record there and then, with tmax as given, and the ray never enters the pool.
__device__ __forceinline__ bool read_ray(const float4 *rays, uint32_t sidx, V3 &o, V3 &d, float &e0, float &e1) {
    const float4 r0 = rays[2 * (size_t)sidx], r1 = rays[2 * (size_t)sidx + 1];
    o = mk(r0.x, r0.y, r0.z); d = mk(r1.x, r1.y, r1.z); e0 = r0.w; e1 = r1.w;
    return ray_finite(o, d) && r1.w == r1.w;
}
// A record, on the device: t,u,v,0 and (primitive, triangle in the primitive) -- tri_prim names the gid's primitive (k_soup's table) and first_tri that primitive's first
// gid; no triangle record, no host.  A miss: (x,0,0,0) and (-1,-1), x the range's end as the caller gave it.  K: anything with tuv, ids, tri_prim, first_tri.
// (I: the index in its caller's own type, uint32_t or size_t: with a size_t parameter the compiler assigns the registers of k_cast, k_sweep and k_closest otherwise, and
// k_cast gains an instruction)
template <class K, class I> __device__ __forceinline__ void write_hit(const K &a, I at, uint32_t gid, float t, float u, float v) {
    const uint32_t prim = a.tri_prim[gid];
    a.tuv[at] = make_float4(t, u, v, 0.f);
    a.ids[at] = make_int2((int)prim, (int)(gid - a.first_tri[prim]));
}
template <class K, class I> __device__ __forceinline__ void write_miss(const K &a, I at, float x) { a.tuv[at] = make_float4(x, 0.f, 0.f, 0.f); a.ids[at] = make_int2(-1, -1); }
// the point u, v of the triangle at leaf position pos, from its record (v0 e1 e2), w = 1: what the point queries and k_sweep report beside a hit; a miss: zeros (point: may be null)
__device__ __forceinline__ float4 contact_point(const DevTri *tris, uint32_t pos, float u, float v) {
    const float4 *tq = reinterpret_cast<const float4 *>(tris + pos);
    const float4 ta = tq[0], tb = tq[1], tc = tq[2];
    return make_float4(ta.x + (u * ta.w + v * tb.z), ta.y + (u * tb.x + v * tb.w), ta.z + (u * tb.y + v * tc.x), 1.0f);
}
template <class K, class I> __device__ __forceinline__ void write_point_miss(const K &a, I at, float x) {
    write_miss(a, at, x);
    if (a.point) a.point[at] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// does a query with this cull mask see the triangle at leaf position pos?  The masks only -- no cutoff: the test of the walks that have no alpha_cut
__device__ __forceinline__ bool leaf_visible(const uint32_t *bits, const DevShadeTri *shade, const DevPrim *prims, uint32_t cull, uint32_t pos) {
    if (cull == 0u) return false;
    if (!((bits[pos >> 5] >> (pos & 31u)) & 1u)) return true;   // a leaf without the bit: mask 0xFF
    const uint32_t prim = __float_as_uint(reinterpret_cast<const float4 *>(shade + pos)[8].z);
    return (prim_vis(prims[prim].masked) & cull) != 0u;
}
// A 4-wide node as the queries' own walks (TravPoint, TravSweep, TravBox) take it apart: four bytes a plane, child i's in bits 8i.. of b (lo.x lo.y lo.z hi.x) and c
// (hi.y hi.z); the origin and the power-of-two scales that decode them (plane = byte * s + o); the four references.  It is Trav4::step_internal's decode, which stays
// with the kernels of the frame.  What a walk makes of a child's box is its own.  (c: the two words in use, not the uint4 -- handed on whole, k_sweep loads all four)
struct Node4 { uint4 b; uint2 c; float ox, oy, oz, sx, sy, sz; int refs[4]; };
__device__ __forceinline__ Node4 load_node4(const DevNode4 *__restrict__ wide, int cur) {
    const uint4 *nq = reinterpret_cast<const uint4 *>(wide + cur);
    uint4 a = nq[0], b = nq[1], c = nq[2], d = nq[3];
    asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z), "+v"(d.w));   // the references arrive with the boxes (Trav4::step_internal)
    return {b, make_uint2(c.x, c.y), __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z),
            __uint_as_float((a.w & 255u) << 23), __uint_as_float(((a.w >> 8) & 255u) << 23), __uint_as_float(((a.w >> 16) & 255u) << 23), {(int)d.x, (int)d.y, (int)d.z, (int)d.w}};
}
// A lane's K best candidates, which both multi walks keep (TravMulti, TravPointMulti): up to K entries (key, u, v, gid) in ascending (key, gid), the key a t_eff or a
// d2_eff -- in LDS, [entry][lane] like the walk stack, 16 bytes an entry, so the insertion runs on ds_read / ds_write_b128 with the entry index in a register and nothing
// goes to scratch.  A walk's best pair (tbest | limit, bgid) is its LIMIT: (the range's end, none) until the list is full, the K-th entry's pair from then on -- boxes and
// leaves cull against it as they cull against the best candidate of a closest walk, and a candidate enters iff it is below the limit in the total order, which is that
// walk's comparison (its step_leaf_take makes it: K = 1 IS the closest walk).  Every triangle sits in one leaf and a walk visits a leaf at most once: no entry can arrive
// twice, nothing is checked.  Only a candidate that would enter is put to the mask / alpha test.
struct KList {
    uint32_t K, cnt;   // K: 1..KMAX, wave-uniform; cnt: entries held, 0..K
    uint4 *list;       // this lane's entry 0; entry j at list[j * kTraceBlock]
    // hits: the kernel's __shared__ uint4[kmax * kTraceBlock].  (It is declared where each kernel had it, not in here: with one array in here for both walks, k_closest_multi's
    // instances with a list of 4 came out five and six instructions longer and 0.4 % slower on two legs of their probe -- profiles/README.md, "one list, one hook")
    __device__ __forceinline__ void bind(uint4 *hits, uint32_t k, uint32_t kmax) {
        K = min(max(k, 1u), kmax); cnt = 0u; list = &hits[threadIdx.x];   // (the host launches KMAX >= K: the clamp keeps every index inside the array whatever it is handed)
    }
    // a candidate below the limit enters; limit / limit_gid: the walk's pair
    __device__ __forceinline__ void enter(float key, float u, float v, uint32_t gid, float &limit, uint32_t &limit_gid) {
        uint32_t j = min(cnt, K - 1u);   // the slot that is free: behind the last entry, or the K-th entry's, which leaves
        while (j > 0u) {                 // entries above the candidate move up one
            const uint4 p = list[(j - 1u) * kTraceBlock];
            const float pk = __uint_as_float(p.x);
            if (pk < key || (pk == key && p.w < gid)) break;
            list[j * kTraceBlock] = p; j--;
        }
        list[j * kTraceBlock] = make_uint4(__float_as_uint(key), __float_as_uint(u), __float_as_uint(v), gid);
        cnt = min(cnt + 1u, K);
        if (cnt == K) { const uint4 e = list[(K - 1u) * kTraceBlock]; limit = __uint_as_float(e.x); limit_gid = e.w; }   // full: the K-th entry is the limit
    }
};

// ---- the unfused geometry k_sweep and the point walks both use: no fmaf in any of it (tests/np_closest.py, tests/np_sweep.py restate it in numpy float32) ---------------
__device__ __forceinline__ float dotp(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 crossp(V3 a, V3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// |w - (u e1 + v e2)|^2: the one distance every feature is measured by, and the point art_closest_points reports
__device__ __forceinline__ float tri_uv_d2(V3 w, V3 e1, V3 e2, float u, float v) {
    const float dx = w.x - (u * e1.x + v * e2.x), dy = w.y - (u * e1.y + v * e2.y), dz = w.z - (u * e1.z + v * e2.z);
    return (dx * dx + dy * dy) + dz * dz;
}
// the parameter of the point of segment {s e, 0 <= s <= 1} nearest to w; a segment of no length is its first end point
__device__ __forceinline__ float seg_param(V3 w, V3 e) {
    const float den = dotp(e, e);
    float s = dotp(w, e) / (den > 0.0f ? den : 1.0f);
    s = den > 0.0f ? s : 0.0f;
    s = s > 0.0f ? s : 0.0f;   // (selects, not fmaxf / fminf: a NaN becomes 0 here and in numpy.where alike)
    return s < 1.0f ? s : 1.0f;
}
// d2_tri of DESIGN.md 3.8: the face where the projection falls inside it, then the edges v0v1, v0v2, v1v2 clamped; the first of the smallest wins.  +inf: no feature gave
// a number (a triangle nowhere, a non-finite one).  u, v: barycentrics of vertices 1 and 2 of the winning point.
__device__ __forceinline__ float tri_closest(V3 w, V3 e1, V3 e2, float &u, float &v) {
    float best = INFINITY; u = 0.0f; v = 0.0f;
    const V3 n = crossp(e1, e2);
    const float nn = dotp(n, n), den = nn > 0.0f ? nn : 1.0f;
    const float fu = dotp(crossp(w, e2), n) / den, fv = dotp(crossp(e1, w), n) / den;
    if ((nn > 0.0f) & (fu >= 0.0f) & (fv >= 0.0f) & (fu + fv <= 1.0f)) {
        const float d = tri_uv_d2(w, e1, e2, fu, fv);
        if (d < best) { best = d; u = fu; v = fv; }
    }
    const float sa = seg_param(w, e1), da = tri_uv_d2(w, e1, e2, sa, 0.0f);
    if (da < best) { best = da; u = sa; v = 0.0f; }
    const float sb = seg_param(w, e2), db = tri_uv_d2(w, e1, e2, 0.0f, sb);
    if (db < best) { best = db; u = 0.0f; v = sb; }
    const float sc = seg_param(w - e1, e2 - e1), uc = 1.0f - sc, dc = tri_uv_d2(w, e1, e2, uc, sc);
    if (dc < best) { best = dc; u = uc; v = sc; }
    return best;
}
__device__ __forceinline__ float box_d2(V3 p, float lx, float ly, float lz, float hx, float hy, float hz) {
    const float ex = fmaxf(fmaxf(lx - p.x, p.x - hx), 0.0f), ey = fmaxf(fmaxf(ly - p.y, p.y - hy), 0.0f), ez = fmaxf(fmaxf(lz - p.z, p.z - hz), 0.0f);
    return (ex * ex + ey * ey) + ez * ez;
}

// The launch shape of every query: {chunk, refill, blocks, leaf_batch} as for the AO launch, whose shape the kernels have -- a query is throughput-bound like it -- with
// the context's ArtTuning overrides.  query_fill: the fields every kernel's arguments share (cast_fill, closest_fill: with those of the casts, of the point queries);
// launch_query: one instance, chosen by its caller, on that shape.
static inline Tune query_tune(const QueryArgs &c) { return tune_over(Tune{256, kPoolTake, 2048, 8}, c.tune); }
template <class K> static K query_fill(const QueryArgs &c) {
    const Tune t = query_tune(c);
    K a{};
    a.wide = c.wide; a.tris = c.tris; a.tri_prim = c.tri_prim; a.first_tri = c.first_tri; a.tuv = c.tuv; a.ids = c.ids;
    a.total = c.n; a.chunk = t.chunk; a.refill = t.refill; a.leaf_batch = t.leaf_batch; a.cursors = c.cursors;
    return a;
}
template <class K> static void launch_query(void (*kernel)(K), const K &a, const QueryArgs &c, hipStream_t s) {
    if (c.n) kernel<<<persistent_blocks(c.n, query_tune(c)), kTraceBlock, 0, s>>>(a);
}

} // namespace art
