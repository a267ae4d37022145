// art_walk.h -- the per-ray walk: a lane's traversal state over the binary and the 4-wide quantised nodes (TravBase / Trav / Trav4), the per-XCD chunk cursors
// (pop_chunk) and the pooled persistent-wave loop (pooled_trace).  Included by art_trace.hip (k_trace, k_trace_ao) and, through art_query.h, art_query_rays.hip (the casts, k_sweep) and art_query_points.hip (the point queries).
// TravBase has ONE leaf step, step_leaf_take, with a hook for what becomes of a closest candidate: step_leaf keeps it as the best, art_query_rays.hip's TravMulti lists it.
#pragma once
#include "art_device.h"

namespace art {

// ---- per-ray traversal state --------------------------------------------------------------------------------------
// `cur` and the stack hold child references: >= 0 an internal node of the structure being walked, < 0 a triangle
// (~leaf position).  Internal steps and triangle tests are separate so that the wave can batch the triangle tests: the
// Moeller-Trumbore block is ~150 instructions and, run whenever any single lane reaches a leaf, it was 60 % of all
// issued instructions at ~2 % lane utilisation.
constexpr int kOvfStack4 = 288; // 16 + 288 >= 3 pending siblings per level * 95 levels + 1
template <bool ANY, int OVF, int LDSN = kLdsStack, bool ALPHA = false> struct TravBase {   // LDSN: entries of the per-lane stack that live in LDS; ALPHA: the alpha test
    Ray r;
    float tbest, bu, bv;
    uint32_t bpos, bgid;
    int cur, sp;
    __device__ __forceinline__ void start(V3 o, V3 d, float tmin, float tmax) {
        ray_init(r, o, d, tmin, tmax);
        tbest = (ray_finite(o, d) && tmax == tmax) ? tmax : -INFINITY; // a non-finite ray (or range) fails the root's box test and ends as a miss
        bu = 0.f; bv = 0.f; bpos = kNoHit; bgid = kNoHit; cur = 0; sp = 0;
    }
    __device__ __forceinline__ void push(int ref, int *lds, int *ovf) {
        // the spill accesses are volatile so that the compiler keeps them apart from the LDS ones: merged, they become flat_load
        // / flat_store on a selected pointer, which waits on vmcnt AND lgkmcnt at every pop
        if (sp < LDSN) lds[sp * kTraceBlock] = ref; else if (sp < LDSN + OVF) *(volatile int *)&ovf[sp - LDSN] = ref;
        sp = min(sp + 1, LDSN + OVF); // the tree cannot need more (see the bounds above); never index past the spill area
    }
    __device__ __forceinline__ bool pop(int *lds, int *ovf) { // true: stack empty, the ray is finished
        if (sp == 0) return true;
        sp--;
        if (sp < LDSN) cur = lds[sp * kTraceBlock]; else cur = *(volatile int *)&ovf[sp - LDSN];
        return false;
    }
    // accept() of DESIGN.md 1.1 for the triangle in `cur`: exact triangle-AABB slab, then Moeller-Trumbore (and with ALPHA the alpha test of DESIGN.md 3.2).  What becomes of a
    // closest candidate that is below (tbest, bgid) is the caller's: take(t_eff, u, v, pos, gid) -- step_leaf keeps it as the best, TravMulti (art_query_rays.hip) enters it in its list
    template <class TAKE> __device__ __forceinline__ bool step_leaf_take(const DevTri *__restrict__ tris, int *lds, int *ovf, const AlphaView &av, const TAKE &take) {
        uint32_t pos = (uint32_t)~cur;
        // the reference of an ABSENT child of a 4-wide node (kAbsentChild: no leaf sits at position 2^31 - 1).  Its inverted box is left before it is entered by every
        // ray with a sign on every axis -- but a node scaled down to a point (a one-triangle tree, a node whose children were all masked) gives near == far on all three
        // axes to a ray through that point, which passes: such a "triangle" is nothing
        if (pos == 0x7FFFFFFFu) return pop(lds, ovf);
        const float4 *tq = reinterpret_cast<const float4 *>(tris + pos);
        float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid (DevTri)
        asm volatile("" : "+v"(td.x), "+v"(td.y), "+v"(td.z), "+v"(td.w), "+v"(tc.y), "+v"(tc.z), "+v"(tc.w)); // the box arrives with the vertices (else its load sinks below the triangle test: a second round trip for the lanes that pass it)
        float te, t, u, v;
        // triangle test first: the lane is here because this very box passed in the parent, so the slab (needed for t_eff and for
        // the conjunction) would nearly always run; after the triangle test it runs for the few hits only.  Same accept().
        if (moller_trumbore(r, mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), t, u, v)) {
            if (slab(r, tc.y, tc.z, tc.w, td.x, td.y, td.z, tbest, te)) {
                if (ANY) { if (!ALPHA || !alpha_cut(av, pos, u, v)) { bpos = pos; tbest = t; return true; } }
                else {
                    float teff = fmaxf(t, te);
                    uint32_t gid = __float_as_uint(td.w);
                    // (only a candidate that would win is tested: a cut one that would lose changes nothing)
                    if ((teff < tbest || (teff == tbest && gid < bgid)) && (!ALPHA || !alpha_cut(av, pos, u, v))) take(teff, u, v, pos, gid);
                }
            }
        }
        return pop(lds, ovf);
    }
    __device__ __forceinline__ bool step_leaf(const DevTri *__restrict__ tris, int *lds, int *ovf, const AlphaView &av) {
        return step_leaf_take(tris, lds, ovf, av, [this](float teff, float u, float v, uint32_t pos, uint32_t gid) { tbest = teff; bu = u; bv = v; bpos = pos; bgid = gid; });
    }
    // two children with hit flags / entry distances: continue with the nearer, stack the farther
    __device__ __forceinline__ bool descend2(bool h0, bool h1, float te0, float te1, int c0, int c1, int *lds, int *ovf) {
        if (h0 && h1) {
            bool first0 = te0 <= te1;
            push(first0 ? c1 : c0, lds, ovf);
            cur = first0 ? c0 : c1;
            return false;
        }
        if (h0) { cur = c0; return false; }
        if (h1) { cur = c1; return false; }
        return pop(lds, ovf);
    }
};

// 64-byte binary nodes (DevNode): both child boxes in full precision
template <bool ANY, bool ALPHA = false> struct Trav : TravBase<ANY, kOvfStack, kLdsStack, ALPHA> {
    using Nodes = const DevNode *;
    __device__ __forceinline__ bool step_internal(Nodes nodes, int *lds, int *ovf) {
        const float4 *nq = reinterpret_cast<const float4 *>(nodes + this->cur);
        float4 q0 = nq[0], q1 = nq[1], q2 = nq[2], q3 = nq[3];
        float te0, te1;
        bool h0 = slab(this->r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, this->tbest, te0);
        bool h1 = slab(this->r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, this->tbest, te1);
        return this->descend2(h0, h1, te0, te1, __float_as_int(q3.x), __float_as_int(q3.y), lds, ovf);
    }
};

// 64-byte 4-wide quantised nodes (DevNode4)
template <bool ANY, int LDSN = kLdsStack, bool ALPHA = false> struct Trav4 : TravBase<ANY, kOvfStack4 + (kLdsStack - LDSN), LDSN, ALPHA> {
    using Nodes = const DevNode4 *;
    __device__ __forceinline__ bool step_internal(Nodes wide, int *lds, int *ovf) {
        const uint4 *nq = reinterpret_cast<const uint4 *>(wide + this->cur);
        uint4 a = nq[0], b = nq[1], c = nq[2], d = nq[3];
        // the child references arrive WITH the boxes: left to itself the compiler sinks their load below the box tests (it is only needed when a child is hit),
        // which makes every node step two dependent memory round trips instead of one -- and the AO launch waits on memory 44 % of the time (profiles round3):
        // config 5 16 980 -> 17 800 Mray/s
        asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z), "+v"(d.w));
        float ox = __uint_as_float(a.x), oy = __uint_as_float(a.y), oz = __uint_as_float(a.z);
        float sx = __uint_as_float((a.w & 255u) << 23), sy = __uint_as_float(((a.w >> 8) & 255u) << 23), sz = __uint_as_float(((a.w >> 16) & 255u) << 23);
        int refs[4] = {(int)d.x, (int)d.y, (int)d.z, (int)d.w};
        float te[4]; bool h[4];
        // The slab with the entry plane of each axis chosen by the lane's direction sign -- ONE select per axis picks the word that holds the four children's near
        // planes, one the far planes -- instead of min / max of both planes per child: fma is monotone in the plane coordinate, so min(t0, t1) IS the near plane's
        // t for a box with lo <= hi, bit for bit (the packet walks' octant trick, per lane).  An absent child carries an inverted box (art_records.h wide_quantise): whatever the
        // signs it is left before it is entered, so no valid-mask test.  33 -> 22 vector instructions a child; config 5 16 440 -> 16 980 Mray/s (profiles/README.md round 3).
        const Ray &r = this->r;
        const bool ngx = r.inv.x < 0.0f, ngy = r.inv.y < 0.0f, ngz = r.inv.z < 0.0f;
        const uint32_t nxw = ngx ? b.w : b.x, fxw = ngx ? b.x : b.w, nyw = ngy ? c.x : b.y, fyw = ngy ? b.y : c.x, nzw = ngz ? c.y : b.z, fzw = ngz ? b.z : c.y;
        const float lim = this->tbest;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float tnx = fmaf(fmaf((float)((nxw >> (8 * i)) & 255u), sx, ox), r.inv.x, -r.ood.x), tfx = fmaf(fmaf((float)((fxw >> (8 * i)) & 255u), sx, ox), r.inv.x, -r.ood.x);
            float tny = fmaf(fmaf((float)((nyw >> (8 * i)) & 255u), sy, oy), r.inv.y, -r.ood.y), tfy = fmaf(fmaf((float)((fyw >> (8 * i)) & 255u), sy, oy), r.inv.y, -r.ood.y);
            float tnz = fmaf(fmaf((float)((nzw >> (8 * i)) & 255u), sz, oz), r.inv.z, -r.ood.z), tfz = fmaf(fmaf((float)((fzw >> (8 * i)) & 255u), sz, oz), r.inv.z, -r.ood.z);
            float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
            te[i] = tn;
            h[i] = fmaxf(tn, r.tmin) <= fminf(tf, lim);
        }
        float tn = 3.0e38f; int ni = -1; // continue with the nearest hit child, stack the others
        if (ANY) { // an any-hit ray's answer does not depend on the order of its visits, only how soon a hit ends it: the first hit child in the node's own order (the
                   // children are sorted along an axis) instead of the nearest saves the selection chain -- config 5 15 650 -> 16 440 Mray/s (profiles/README.md round 3)
#pragma unroll
            for (int i = 3; i >= 0; i--) if (h[i]) ni = i;
        } else
#pragma unroll
        for (int i = 0; i < 4; i++) if (h[i] && te[i] < tn) { tn = te[i]; ni = i; }
        if (ni < 0) return this->pop(lds, ovf);
#pragma unroll
        for (int i = 0; i < 4; i++) if (h[i] && i != ni) this->push(refs[i], lds, ovf);
        this->cur = ni == 0 ? refs[0] : (ni == 1 ? refs[1] : (ni == 2 ? refs[2] : refs[3]));
        return false;
    }
};

// A persistent wave takes its next chunk: lane 0 pops from the eight per-XCD cursors, its own XCD's first, and everyone learns the result.  Returns the chunk's index,
// 0xFFFFFFFF when every cursor is exhausted.  (The caller keeps exhausted / cur / end: handing them through here by reference costs k_trace up to 9 VGPRs.)
__device__ __forceinline__ uint32_t pop_chunk(uint32_t *cursors, uint32_t n_chunks, uint32_t lane, uint32_t &shard, uint32_t &shards_left) {
    uint32_t got = 0xFFFFFFFFu;
    if (lane == 0) {
        while (shards_left) { // shard s owns chunks [n*s/8, n*(s+1)/8): contiguous, so an XCD keeps a screen region
            uint32_t lo = (n_chunks * shard) >> 3, hi = (n_chunks * (shard + 1u)) >> 3;
            uint32_t c = hi > lo ? atomicAdd(&cursors[shard * kCursorStride], 1u) : 0u;
            if (hi > lo && c < hi - lo) { got = lo + c; break; }
            shard = (shard + 1u) & 7u; shards_left--;
        }
    }
    got = __builtin_amdgcn_readfirstlane(got);
    shard = __builtin_amdgcn_readfirstlane(shard);
    shards_left = __builtin_amdgcn_readfirstlane(shards_left);
    return got;
}
#ifndef ART_NODE_REPS
#define ART_NODE_REPS 3   // node steps a lane may take per turn of the loop (the turn's ballots, refill test and branches are scalar work the wave pays per turn: config 5 19 000 -> 20 000 Mray/s at 3, 19 900 at 2, 19 000 at 6)
#endif

// The pooled per-ray tracer (round 4, first for the AO launch): rays enter the wave sixty-four at a time -- the WHOLE wave makes or reads the next (up to) 64 slots of its chunk
// and writes the live ones into a pool in LDS with everything ray_init makes of them -- and a lane that finishes TAKES its next ray from the top of the pool at once (a dozen
// LDS reads).  In k_trace a finished lane waits until two dozen lanes are idle, because a refill there is ~80 instructions whoever runs it: 48 of 64 lanes held a ray
// (profiles/README.md round 3).  LDS a wave: LDSN = 8 stack entries a lane, 2 KB, + the pool's 3 KB = 32 waves in a CU's 160 KB.  One walk, Trav4 over the quantised 4-wide
// nodes (hits are structure-independent).  What differs between the two launches that run this loop is their Source:
//   kFields                      pool fields a ray: o.xyz d.xyz inv.xyz, one or two of the source's own (e0, e1), slot
//   init(tr)                     once per lane, before the loop
//   fetch(sidx, o, d, e0, e1)    slot sidx's ray; returns whether there is one to walk, and has written the slot's record itself where there is none
//   begin(tr, e0, e1)            a lane takes a ray: what the source's own fields set
//   finish(tr, slot)             the finished ray's record
constexpr uint32_t kPoolTake = 8;   // idle lanes at which the wave turns to the pool (ArtTuning.trace_refill overrides)
template <int LDSN, bool ANY, bool ALPHA, class ARGS, class SOURCE, class TRAV = Trav4<ANY, LDSN, ALPHA>>   // TRAV: the candidate policy (any | closest; TravMulti: the first K)
__device__ __forceinline__ void pooled_trace(const ARGS &a, const SOURCE &src) {
    constexpr int kSlotField = SOURCE::kFields - 1;
    static_assert(kSlotField == 10 || kSlotField == 11, "nine fields of the ray, one or two of the source, the slot");
    __shared__ int stack[LDSN * kTraceBlock];
    __shared__ float pool[SOURCE::kFields][kTraceBlock];
    int ovf[kOvfStack4 + (kLdsStack - LDSN)];
    const uint32_t leaf_batch = a.leaf_batch;
    int *lds = &stack[threadIdx.x];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (a.total + a.chunk - 1) / a.chunk;   // total <= ART_CAST_MAX_RAYS = 2^31 - 65536 and 64 <= chunk <= 65536: total + chunk, chunk ends and n_chunks * 8 fit 32 bits
    uint32_t shard = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u; // HW_REG_XCC_ID: speed only
    uint32_t shards_left = 8;
    uint32_t cur = 0, end = 0;   // wave-uniform: the unread part of this wave's chunk
    uint32_t pool_n = 0;         // wave-uniform: rays in the pool
    bool exhausted = false, active = false;
    TRAV tr;
    src.init(tr);
    uint32_t slot = 0;
    for (;;) {
        const uint64_t idle = ballot64(!active);
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        if (n_idle >= a.refill) {
            if (pool_n == 0 && !exhausted) {      // the pool is empty: the WHOLE wave fetches the next (up to) 64 slots of its chunk
                if (cur == end) {
                    const uint32_t got = pop_chunk(a.cursors, n_chunks, lane, shard, shards_left);
                    if (got >= n_chunks) exhausted = true;   // (also the never-expected out-of-range pop: no record beyond total is touched)
                    else { cur = got * a.chunk; end = min(cur + a.chunk, a.total); }
                }
                if (!exhausted) {
                    const uint32_t take = min(64u, end - cur), sidx = cur + lane;
                    bool has = false;
                    V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f); float e0 = 0.f, e1 = 0.f;
                    if (lane < take) has = src.fetch(sidx, o, d, e0, e1);
                    const uint64_t hm = ballot64(has);
                    if (has) {
                        const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u));
                        const V3 inv = mk(1.0f / safe_dir(d.x), 1.0f / safe_dir(d.y), 1.0f / safe_dir(d.z));   // ray_init's operations
                        pool[0][at] = o.x; pool[1][at] = o.y; pool[2][at] = o.z; pool[3][at] = d.x; pool[4][at] = d.y; pool[5][at] = d.z;
                        pool[6][at] = inv.x; pool[7][at] = inv.y; pool[8][at] = inv.z; pool[9][at] = e0; if (kSlotField == 11) pool[10][at] = e1;
                        pool[kSlotField][at] = __uint_as_float(sidx);
                    }
                    pool_n = (uint32_t)__popcll(hm);
                    cur += take;
                }
            }
            if (pool_n) {                             // idle lanes take rays from the top of the pool
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (!active && rank < pool_n) {
                    const uint32_t at = pool_n - 1u - rank;
                    tr.r.o = mk(pool[0][at], pool[1][at], pool[2][at]); tr.r.d = mk(pool[3][at], pool[4][at], pool[5][at]); tr.r.inv = mk(pool[6][at], pool[7][at], pool[8][at]);
                    tr.r.ood = mk(tr.r.o.x * tr.r.inv.x, tr.r.o.y * tr.r.inv.y, tr.r.o.z * tr.r.inv.z);
                    src.begin(tr, pool[9][at], kSlotField == 11 ? pool[10][at] : 0.f);
                    tr.tbest = tr.r.tmax; tr.bu = 0.f; tr.bv = 0.f; tr.bpos = kNoHit; tr.bgid = kNoHit; tr.sp = 0;
                    slot = __float_as_uint(pool[kSlotField][at]);
                    active = true;
                }
                pool_n -= min(n_idle, pool_n);
            } else if (exhausted) { if (n_idle == 64u) break; }
            if (ballot64(active) == 0ull) continue;   // nothing to trace yet (a chunk of padding / misses, 64 dead rays): fetch more
        }
        bool done = false;   // k_trace's step block: node steps, then the triangle tests once enough lanes wait on one (or nobody can move without it)
#pragma unroll
        for (int rep_ = 0; rep_ < ART_NODE_REPS; rep_++)
            if (active && !done && tr.cur >= 0) done = tr.step_internal(a.wide, lds, ovf);
        const bool on_leaf = active && !done && tr.cur < 0;
        const uint64_t lm = ballot64(on_leaf);
        if (lm != 0ull && ((uint32_t)__popcll(lm) >= leaf_batch || ballot64(active && !done && tr.cur >= 0) == 0ull)) { if (on_leaf) done = tr.step_leaf(a.tris, lds, ovf, a.alpha); }
        if (done) { active = false; src.finish(tr, slot); }
    }
}

} // namespace art
