// art_query_rays.hip -- the device side of the ray queries on device buffers (gfx950): ray casts (k_cast), the first K hits (k_cast_multi), the crossings of each ray (k_cross)
// and swept spheres (k_sweep).  The casts and the sweep are Sources and candidate policies of art_walk.h's pooled loop (pooled_trace); the queries that have no ray to pool
// run a loop of their own in art_query_points.hip.  What the two units share stands once, in art_query.h.  art_cast.hip is their host side.
#include "art_query.h"

namespace art {

// Rays the CALLER made, in a device buffer (art_cast_rays, DESIGN.md 3.5: the application's own traceRayEXT), are READ.  One walk for every context, whatever ArtTuning
// says.  Closest hits leave as records of the walk's best candidate; any-hit answers are bytes.  The order of the rays in the buffer cannot matter: a ray's record
// depends on the ray alone.
struct CastK {
    const DevNode4 *wide; const DevTri *tris; const uint32_t *tri_prim, *first_tri;
    const float4 *rays; float4 *tuv; int2 *ids; uint8_t *hit;
    uint32_t total, chunk, refill, leaf_batch;
    uint32_t *cursors;        // 8 per-XCD chunk cursors, kCursorStride words apart (zeroed in front of the launch)
    AlphaView alpha;          // the instances with the mask / alpha test only
};
static_assert(kCastCursorWords == 8u * kCursorStride, "a cast's cursor block");
constexpr int kCastLds = 8;           // per-lane stack entries in LDS
template <bool ANY> struct CastSource {
    static constexpr int kFields = 12;   // o.xyz d.xyz inv.xyz tmin tmax slot
    const CastK &a;
    template <class TRAV> __device__ __forceinline__ void init(TRAV &) const {}
    __device__ __forceinline__ bool fetch(uint32_t sidx, V3 &o, V3 &d, float &e0, float &e1) const {
        const bool has = read_ray(a.rays, sidx, o, d, e0, e1);
        if (!has) { if (ANY) a.hit[sidx] = 0; else write_miss(a, sidx, e1); }   // a dead ray: its miss record, without a walk
        return has;
    }
    template <class TRAV> __device__ __forceinline__ void begin(TRAV &tr, float e0, float e1) const { tr.r.tmin = e0; tr.r.tmax = e1; tr.cur = 0; }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot) const {
        if (ANY) a.hit[slot] = tr.bpos != kNoHit ? 1 : 0;
        else if (tr.bgid != kNoHit) write_hit(a, slot, tr.bgid, tr.tbest, tr.bu, tr.bv);
        else write_miss(a, slot, tr.r.tmax);
    }
};
template <bool ANY, bool ALPHA>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_cast(CastK a) { pooled_trace<kCastLds, ANY, ALPHA>(a, CastSource<ANY>{a}); }

// The first K hits of each ray, in order (art_cast_rays_multi): the third candidate policy.  The closest walk keeps ONE best candidate; this one hands it to
// the list, through the hook TravBase::step_leaf_take has for a candidate's fate -- the leaf step, its slab cull and the box tests of Trav4 are the closest walk's own.
template <int KMAX, int LDSN, bool ALPHA> struct TravMulti : Trav4<false, LDSN, ALPHA>, KList {
    __device__ __forceinline__ void bind(uint32_t k) {
        __shared__ uint4 hits[KMAX * kTraceBlock];
        KList::bind(hits, k, KMAX);
    }
    __device__ __forceinline__ bool step_leaf(const DevTri *__restrict__ tris, int *lds, int *ovf, const AlphaView &av) {
        return this->step_leaf_take(tris, lds, ovf, av, [this](float teff, float u, float v, uint32_t, uint32_t gid) { enter(teff, u, v, gid, this->tbest, this->bgid); });
    }
};
struct CastMultiK : CastK { uint8_t *count; uint32_t max_hits; };   // tuv / ids: max_hits records a ray, ray-major; count: a byte a ray, or null
template <int KMAX> struct CastMultiSource {
    static constexpr int kFields = 12;   // CastSource's
    const CastMultiK &a;
    template <class TRAV> __device__ __forceinline__ void init(TRAV &tr) const { tr.bind(a.max_hits); }
    __device__ __forceinline__ bool fetch(uint32_t sidx, V3 &o, V3 &d, float &e0, float &e1) const {
        const bool has = read_ray(a.rays, sidx, o, d, e0, e1);
        if (!has) {                // a dead ray: K miss records, no walk
            const size_t base = (size_t)sidx * a.max_hits;
            for (uint32_t j = 0; j < a.max_hits; j++) write_miss(a, base + j, e1);
            if (a.count) a.count[sidx] = 0;
        }
        return has;
    }
    template <class TRAV> __device__ __forceinline__ void begin(TRAV &tr, float e0, float e1) const { tr.r.tmin = e0; tr.r.tmax = e1; tr.cur = 0; tr.cnt = 0u; }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot) const {
        const size_t base = (size_t)slot * tr.K;
        for (uint32_t j = 0; j < tr.K; j++) {
            if (j < tr.cnt) {
                const uint4 e = tr.list[j * kTraceBlock];
                write_hit(a, base + j, e.w, __uint_as_float(e.x), __uint_as_float(e.y), __uint_as_float(e.z));
            } else write_miss(a, base + j, tr.r.tmax);
        }
        if (a.count) a.count[slot] = (uint8_t)tr.cnt;
    }
};
// KMAX 4 | 8: the list is KMAX KB of LDS a wave on top of the 5 KB of stack and pool, and LDS is what bounds the waves a CU holds -- small K keeps more resident.
// (waves_per_eu: LDS allows four waves a SIMD with KMAX 4 and three with KMAX 8, so the registers of that many are the kernel's to use)
template <int KMAX, bool ALPHA>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(KMAX > 4 ? 3 : 4, 4))) void k_cast_multi(CastMultiK a) {
    pooled_trace<kCastLds, false, ALPHA, CastMultiK, CastMultiSource<KMAX>, TravMulti<KMAX, kCastLds, ALPHA>>(a, CastMultiSource<KMAX>{a});
}

// The surfaces each ray enters and leaves (art_cast_crossings): the fourth candidate policy.  Nothing orders or shrinks: tbest stays the range's end for
// the whole walk, so Trav4's box tests and the triangle's slab cull against [tmin, tmax] alone and every triangle accept() takes is met once.  Two counters a lane, no list:
// LDS is the walk stack and the pool, as k_cast's.  The leaf step is a sibling of TravBase::step_leaf_take -- that one's hook has no det -- around moller_trumbore_det,
// whose det is the one that accepted the candidate.  EVERY candidate is put to the mask / alpha test (each one counts; there is no "would win").
template <int LDSN, bool ALPHA> struct TravCross : Trav4<false, LDSN, ALPHA> {
    uint32_t n_in, n_out;   // det > 0: against the winding normal, an entry; det < 0: along it, an exit
    __device__ __forceinline__ bool step_leaf(const DevTri *__restrict__ tris, int *lds, int *ovf, const AlphaView &av) {
        const uint32_t pos = (uint32_t)~this->cur;
        if (pos == 0x7FFFFFFFu) return this->pop(lds, ovf);   // kAbsentChild: nothing (TravBase::step_leaf_take)
        const float4 *tq = reinterpret_cast<const float4 *>(tris + pos);
        float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid
        asm volatile("" : "+v"(td.x), "+v"(td.y), "+v"(td.z), "+v"(td.w), "+v"(tc.y), "+v"(tc.z), "+v"(tc.w));   // the box arrives with the vertices (TravBase::step_leaf_take)
        float te, t, u, v, det;
        if (moller_trumbore_det(this->r, mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), t, u, v, det)) {
            if (slab(this->r, tc.y, tc.z, tc.w, td.x, td.y, td.z, this->tbest, te)) {
                if (!ALPHA || !alpha_cut(av, pos, u, v)) { if (det > 0.0f) n_in++; else n_out++; }   // (alpha_cut: the masks first, then the cutoff)
            }
        }
        return this->pop(lds, ovf);
    }
};
struct CrossK : CastK { uint2 *cross; };   // cross: (entries, exits) a ray; tuv / ids / hit are not used
struct CrossSource {
    static constexpr int kFields = 12;   // CastSource's
    const CrossK &a;
    template <class TRAV> __device__ __forceinline__ void init(TRAV &) const {}
    __device__ __forceinline__ bool fetch(uint32_t sidx, V3 &o, V3 &d, float &e0, float &e1) const {
        const bool has = read_ray(a.rays, sidx, o, d, e0, e1);
        if (!has) a.cross[sidx] = make_uint2(0u, 0u);   // a dead ray crosses nothing: its record, without a walk
        return has;
    }
    template <class TRAV> __device__ __forceinline__ void begin(TRAV &tr, float e0, float e1) const { tr.r.tmin = e0; tr.r.tmax = e1; tr.cur = 0; tr.n_in = 0u; tr.n_out = 0u; }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot) const { a.cross[slot] = make_uint2(tr.n_in, tr.n_out); }
};
// (waves_per_eu 8: k_cast's walk with two counters for the best candidate's five fields -- DESIGN.md 3.12's table has the compiler's figures)
template <bool ALPHA>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_cross(CrossK a) {
    pooled_trace<kCastLds, false, ALPHA, CrossK, CrossSource, TravCross<kCastLds, ALPHA>>(a, CrossSource{a});
}

// ---- a ball along a ray (art_cast_spheres) --------------------------------------------------------------------------------------------------------
// The rays are the casts' -- 32 bytes a ray, everything ray_init makes of them -- so the loop is pooled_trace with a fourth candidate policy.  The ball's radius is the
// same for every ray of a launch: boxes grow by it (one subtraction / addition a plane, before the slab), and a triangle answers with the first time the ball's centre is
// within it of the triangle: at tmin already (S), or where it enters the slab round the face, a cylinder round an edge or a sphere round a vertex.
// No fmaf in anything that decides a record but the slab's: tests/np_sweep.py restates every operation in numpy float32.
struct SweepK : CastK { float4 *point; float radius; };   // point: may be null
// the ENTRY root of A t^2 + 2 B t + Cq = 0
__device__ __forceinline__ bool sweep_root(float A, float B, float Cq, float &t) {
    const float disc = B * B - A * Cq;
    t = (-B - sqrtf(disc >= 0.0f ? disc : 0.0f)) / (A > 0.0f ? A : 1.0f);
    return (A > 0.0f) & (disc >= 0.0f);
}
// the cylinder of radius sqrt(rr) round the line {m + s e}: the direction of the edge is projected out of m and d before the quadratic (second order in lengths)
__device__ __forceinline__ bool sweep_edge(V3 m, V3 e, V3 d, float rr, float &t, float &s) {
    const float ee = dotp(e, e), q = ee > 0.0f ? ee : 1.0f, qm = dotp(m, e) / q, qd = dotp(d, e) / q;
    const V3 mp = mk(m.x - qm * e.x, m.y - qm * e.y, m.z - qm * e.z), dp = mk(d.x - qd * e.x, d.y - qd * e.y, d.z - qd * e.z);
    const bool ok = sweep_root(dotp(dp, dp), dotp(mp, dp), dotp(mp, mp) - rr, t);
    s = qm + t * qd;
    return (ee > 0.0f) & ok & (s >= 0.0f) & (s <= 1.0f);
}
__device__ __forceinline__ void sweep_take(bool ok, float t, float u, float v, float tmin, float tmax, float &bt, float &bu, float &bv) {
    if (ok & (t >= tmin) & (t < tmax) & (t < bt)) { bt = t; bu = u; bv = v; }   // (a NaN never wins)
}
// t_tri of DESIGN.md 3.9 for w0 = o - v0: the smallest t in [tmin, tmax) among S, F, E01, E02, E12, V0, V1, V2, the first of equals; +inf: none.  u, v: its barycentrics
__device__ __forceinline__ float tri_sweep(V3 w0, V3 d, V3 e1, V3 e2, float rho, float tmin, float tmax, float &u, float &v) {
    float bt = INFINITY, t, s; u = 0.0f; v = 0.0f;
    const float rr = rho * rho, dd = dotp(d, d);
    {   // S: the ball touches the triangle where it starts
        float su, sv;
        const float d2 = tri_closest(mk(w0.x + tmin * d.x, w0.y + tmin * d.y, w0.z + tmin * d.z), e1, e2, su, sv);
        sweep_take(d2 <= rr, tmin, su, sv, tmin, tmax, bt, u, v);
    }
    {   // F: the centre reaches the plane at distance rho on its own side, above the face
        const V3 n = crossp(e1, e2);
        const float nn = dotp(n, n), h = dotp(n, w0), nd = dotp(n, d);
        float off = rho * sqrtf(nn); off = h >= 0.0f ? off : -off;
        t = (off - h) / (nd != 0.0f ? nd : 1.0f);
        const V3 w = mk(w0.x + t * d.x, w0.y + t * d.y, w0.z + t * d.z);
        const float den = nn > 0.0f ? nn : 1.0f, fu = dotp(crossp(w, e2), n) / den, fv = dotp(crossp(e1, w), n) / den;
        sweep_take((nn > 0.0f) & (nd != 0.0f) & (fu >= 0.0f) & (fv >= 0.0f) & (fu + fv <= 1.0f), t, fu, fv, tmin, tmax, bt, u, v);
    }
    const V3 w1 = w0 - e1, w2 = w0 - e2;
    bool ok = sweep_edge(w0, e1, d, rr, t, s); sweep_take(ok, t, s, 0.0f, tmin, tmax, bt, u, v);
    ok = sweep_edge(w0, e2, d, rr, t, s); sweep_take(ok, t, 0.0f, s, tmin, tmax, bt, u, v);
    ok = sweep_edge(w1, e2 - e1, d, rr, t, s); sweep_take(ok, t, 1.0f - s, s, tmin, tmax, bt, u, v);
    ok = sweep_root(dd, dotp(w0, d), dotp(w0, w0) - rr, t); sweep_take(ok, t, 0.0f, 0.0f, tmin, tmax, bt, u, v);
    ok = sweep_root(dd, dotp(w1, d), dotp(w1, w1) - rr, t); sweep_take(ok, t, 1.0f, 0.0f, tmin, tmax, bt, u, v);
    ok = sweep_root(dd, dotp(w2, d), dotp(w2, w2) - rr, t); sweep_take(ok, t, 0.0f, 1.0f, tmin, tmax, bt, u, v);
    return bt;
}
// The candidate policy: TravBase's state, stack and tie rule; boxes inflated by rho.  FILTER: the visibility masks (leaf_visible; alpha cutoffs are not tested)
template <int LDSN, bool FILTER> struct TravSweep : TravBase<false, kOvfStack4 + (kLdsStack - LDSN), LDSN, false> {
    using Nodes = const DevNode4 *;
    float rho;
    // the triangle's own box, inflated, against tbest first -- an exact cull: a candidate's t_eff is at least its box's entry and at least tmin -- then the eight features
    __device__ __forceinline__ bool step_leaf(const DevTri *__restrict__ tris, int *lds, int *ovf, const AlphaView &av) {
        const uint32_t pos = (uint32_t)~this->cur;
        if (pos == 0x7FFFFFFFu) return this->pop(lds, ovf);   // kAbsentChild: nothing (TravBase::step_leaf)
        const float4 *tq = reinterpret_cast<const float4 *>(tris + pos);
        const float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid
        const Ray &r = this->r;
        float te;
        if (slab(r, tc.y - rho, tc.z - rho, tc.w - rho, td.x + rho, td.y + rho, td.z + rho, this->tbest, te)) {
            float u, v;
            const float tt = tri_sweep(r.o - mk(ta.x, ta.y, ta.z), r.d, mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), rho, r.tmin, r.tmax, u, v);
            if (tt < INFINITY) {
                const float teff = fmaxf(tt, te);
                const uint32_t gid = __float_as_uint(td.w);
                if ((teff < this->tbest || (teff == this->tbest && gid < this->bgid)) && (!FILTER || leaf_visible(av.bits, av.shade, av.prims, av.cull, pos))) { this->tbest = teff; this->bu = u; this->bv = v; this->bpos = pos; this->bgid = gid; }
            }
        }
        return this->pop(lds, ovf);
    }
    // Trav4's sign-selected slab with each child's near plane moved out and its far plane moved out by rho.  An absent child or a masked subtree carries an inverted byte box
    // (255 / 0): "left before it is entered" no longer holds once the planes have moved, so it is skipped by TravPoint's explicit test
    __device__ __forceinline__ bool step_internal(Nodes wide, int *lds, int *ovf) {
        const auto [b, c, ox, oy, oz, sx, sy, sz, refs] = load_node4(wide, this->cur);
        float te[4]; bool h[4];
        const Ray &r = this->r;
        const bool ngx = r.inv.x < 0.0f, ngy = r.inv.y < 0.0f, ngz = r.inv.z < 0.0f;
        const uint32_t nxw = ngx ? b.w : b.x, fxw = ngx ? b.x : b.w, nyw = ngy ? c.x : b.y, fyw = ngy ? b.y : c.x, nzw = ngz ? c.y : b.z, fzw = ngz ? b.z : c.y;
        const float px = ngx ? rho : -rho, py = ngy ? rho : -rho, pz = ngz ? rho : -rho;   // what the near plane moves by (lo - rho is lo + (-rho), bit for bit); the far plane by the opposite
        const float lim = this->tbest;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float tnx = fmaf(fmaf((float)((nxw >> (8 * i)) & 255u), sx, ox) + px, r.inv.x, -r.ood.x), tfx = fmaf(fmaf((float)((fxw >> (8 * i)) & 255u), sx, ox) - px, r.inv.x, -r.ood.x);
            const float tny = fmaf(fmaf((float)((nyw >> (8 * i)) & 255u), sy, oy) + py, r.inv.y, -r.ood.y), tfy = fmaf(fmaf((float)((fyw >> (8 * i)) & 255u), sy, oy) - py, r.inv.y, -r.ood.y);
            const float tnz = fmaf(fmaf((float)((nzw >> (8 * i)) & 255u), sz, oz) + pz, r.inv.z, -r.ood.z), tfz = fmaf(fmaf((float)((fzw >> (8 * i)) & 255u), sz, oz) - pz, r.inv.z, -r.ood.z);
            const float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
            te[i] = tn;
            h[i] = (((b.x >> (8 * i)) & 255u) <= ((b.w >> (8 * i)) & 255u)) & (fmaxf(tn, r.tmin) <= fminf(tf, lim));
        }
        float tn = 3.0e38f; int ni = -1;   // on with the nearest child, the others wait: the order is speed only
#pragma unroll
        for (int i = 0; i < 4; i++) if (h[i] && te[i] < tn) { tn = te[i]; ni = i; }
        if (ni < 0) {   // (a child entered at 3e38 or beyond -- a structure nowhere -- is still a child: the first of them)
#pragma unroll
            for (int i = 3; i >= 0; i--) if (h[i]) ni = i;
            if (ni < 0) return this->pop(lds, ovf);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) if (h[i] && i != ni) this->push(refs[i], lds, ovf);
        this->cur = ni == 0 ? refs[0] : (ni == 1 ? refs[1] : (ni == 2 ? refs[2] : refs[3]));
        return false;
    }
};
struct SweepSource {
    static constexpr int kFields = 12;   // o.xyz d.xyz inv.xyz tmin tmax slot
    const SweepK &a;
    template <class TRAV> __device__ __forceinline__ void init(TRAV &tr) const { tr.rho = a.radius; }   // the same for every ray
    __device__ __forceinline__ bool fetch(uint32_t sidx, V3 &o, V3 &d, float &e0, float &e1) const {
        const bool has = read_ray(a.rays, sidx, o, d, e0, e1);
        if (!has) write_point_miss(a, sidx, e1);   // a dead ray: its miss record, without a walk
        return has;
    }
    template <class TRAV> __device__ __forceinline__ void begin(TRAV &tr, float e0, float e1) const { tr.r.tmin = e0; tr.r.tmax = e1; tr.cur = 0; }
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot) const {
        if (tr.bgid != kNoHit) {
            write_hit(a, slot, tr.bgid, tr.tbest, tr.bu, tr.bv);
            if (a.point) a.point[slot] = contact_point(a.tris, tr.bpos, tr.bu, tr.bv);
        } else write_point_miss(a, slot, tr.r.tmax);
    }
};
// 6 waves a SIMD: the eight-feature test holds 79 VGPRs without a spill; at 8 waves (64) the compiler spills two dozen of them to scratch, at 4 it uses no more than at 6
template <bool FILTER>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 6))) void k_sweep(SweepK a) {
    pooled_trace<kCastLds, false, FILTER, SweepK, SweepSource, TravSweep<kCastLds, FILTER>>(a, SweepSource{a});
}
template <class K> static K cast_fill(const CastArgs &c) {
    K a = query_fill<K>(c);
    a.rays = c.rays; a.alpha = AlphaView{c.alpha_bits, c.shade, c.prims, c.tex_pool, c.cull};
    return a;
}
void launch_cast(const CastArgs &c, hipStream_t s) {
    if (c.kind == CastKind::Sweep) {          // the filtered instance tests masks, never a cutoff
        SweepK a = cast_fill<SweepK>(c); a.point = c.point; a.radius = c.radius;
        launch_query(c.filter ? k_sweep<true> : k_sweep<false>, a, c, s);
    } else if (c.kind == CastKind::Crossings) {
        CrossK a = cast_fill<CrossK>(c); a.cross = c.cross;
        launch_query(c.filter ? k_cross<true> : k_cross<false>, a, c, s);
    } else if (c.kind == CastKind::Multi) {   // the instance with the smallest list that holds K
        CastMultiK a = cast_fill<CastMultiK>(c); a.count = c.count; a.max_hits = c.max_hits;
        launch_query(c.max_hits <= 4u ? (c.filter ? k_cast_multi<4, true> : k_cast_multi<4, false>) : (c.filter ? k_cast_multi<8, true> : k_cast_multi<8, false>), a, c, s);
    } else {
        CastK a = cast_fill<CastK>(c); a.hit = c.hit;
        launch_query(c.kind == CastKind::Any ? (c.filter ? k_cast<true, true> : k_cast<true, false>) : (c.filter ? k_cast<false, true> : k_cast<false, false>), a, c, s);
    }
}

} // namespace art
