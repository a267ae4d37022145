// art_device.h -- the device helpers that more than one unit of libart compiles: vectors, the exact-math cores, the sampler, the alpha test, Ray / slab / Moller-Trumbore,
// the launch constants and the tracers' presets.  Included by art_walk.h and art_shade.h (and through them by art_trace.hip, art_frame.hip, art_query_rays.hip, art_query_points.hip and art_sweeps.hip),
// by art_resolve.hip and by art_present.hip.  A device function that is not forceinline is `inline` (sample_tex; the lights and Burley's diffuse term in art_shade.h), in every header of this directory.
//
// Built with -ffp-contract=off: every fused multiply-add below is an explicit fmaf, so the geometry stages
// (ray generation, slab test, Moller-Trumbore, hit reconstruction up to the shadow ray) follow one fixed
// floating-point expression order.
//
// Geometry semantics (order- and structure-independent):
//   accept(tri, ray) := slab(AABB(tri), ray) passes AND Moller-Trumbore hits with tmin < t < tmax
//   t_eff := max(t_MT, t_entry(AABB(tri)));  closest := argmin (t_eff, gid);  any := exists accept
#pragma once
#include "art_internal.h"

namespace art {

// ------------------------------------------------------------------------------------------------ vector helpers
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 neg(V3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
    return mk(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}
// ---- sqrtf(x) and 1.0f / sqrtf(x), bit for bit, without the range handling their inputs never need ("the guarded fast path") ----
// hipcc compiles either expression correctly rounded and denormal-safe: a 2^32 pre-scale below 2^-96, a class fix-up for 0 / inf, two v_div_scale and a v_div_fixup
// around one core -- v_sqrt_f32 moved by at most one ulp after two FMA residuals; v_rcp_f32 and the division's FMA chain.  Squared lengths of shading vectors sit
// near 1, where none of that wrapping does anything.  A wave whose active lanes all hold x in [kExactLo, kExactHi] (one ballot, one scalar branch) runs the core
// alone: the same hardware instructions and the same FMAs in the same order, so the same bits (28 -> 18 vector instructions for 1 / sqrt).  Any lane outside (a zero
// or denormal normal, inf, NaN, a negative) sends the WHOLE wave through the plain expression: those keep today's bits by construction.  kExactLo is the compiler's
// own scaling threshold; below kExactHi the root stays under 2^48, far from where v_div_scale begins to act.  tests/test_exact_math.py sweeps all 2^32 inputs.
constexpr float kExactLo = 0x1p-96f, kExactHi = 0x1p96f;
__device__ __forceinline__ float sqrt_core(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    float vp = fmaf(-dn, s, x), vs = fmaf(-up, s, x);
    s = vp <= 0.0f ? dn : s;
    return vs > 0.0f ? up : s;
}
__device__ __forceinline__ float rcp_core(float d) {   // 1.0f / d: the quotient's first estimate 1.0f * r is r itself
    float r = __builtin_amdgcn_rcpf(d);
    r = fmaf(fmaf(-d, r, 1.0f), r, r);
    float q = fmaf(fmaf(-d, r, 1.0f), r, r);
    return fmaf(fmaf(-d, q, 1.0f), r, q);
}
// The shorter form of 1.0f / sqrtf(x): v_rsq_f32, a Markstein step to the root, v_rcp_f32 and one Newton step -- 10 vector instructions instead of the core's 16.  Not the
// compiler's instructions, so nothing says by construction that it rounds alike: art_parity_math_sweep (which = 3) finds 0 mismatches against the plain expression over the
// whole of [kExactLo, kExactHi], in whole and in mixed waves.  The k_frame instances that keep their pinned registers with it run it (kFrameShort, art_frame.hip).
__device__ __forceinline__ float inv_sqrt_short(float x) {
    float y = __builtin_amdgcn_rsqf(x);
    float s = x * y, h = 0.5f * y;
    s = fmaf(s, fmaf(-h, s, 0.5f), s);
    s = fmaf(fmaf(-s, s, x), h, s);
    float q = __builtin_amdgcn_rcpf(s);
    return fmaf(fmaf(-s, q, 1.0f), q, q);
}
// a / b as hipcc compiles it once v_div_scale_f32 scales nothing and v_div_fmas_f32 / v_div_fixup_f32 pass their operand on: v_rcp_f32, one refinement, q = a r, two residual
// corrections -- the same instructions in the same order, 9 instead of 12.  The scaling does nothing where a and b are normal, |a| >= 2^-103, |b| <= 2^126, the quotient is
// normal and the exponents are less than 96 apart; div_core_domain is a box well inside that, and art_parity_div_sweep proves the bits over it (tests/test_short_math.py).
// rcp_core above is div_core(1.0f, d); the sweep proves it too, against 1.0f / safe_dir(x) (a ray's reciprocal direction), over [kExactLo, kExactHi].
constexpr float kDivLo = 0x1p-47f, kDivHi = 0x1p47f;
__device__ __forceinline__ float div_core(float a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    r = fmaf(fmaf(-b, r, 1.0f), r, r);
    float q = a * r;
    q = fmaf(fmaf(-b, q, a), r, q);
    return fmaf(fmaf(-b, q, a), r, q);
}
__device__ __forceinline__ bool div_core_domain(float a, float b) { return fabsf(a) >= kDivLo && fabsf(a) <= kDivHi && fabsf(b) >= kDivLo && fabsf(b) <= kDivHi; }
// plain: wave-uniform, forces the plain expression (ArtTuning.plain_math); fast: whether this wave took the core (the sweep counts it); FAST = false: the plain expression
// and nothing else, for the k_frame instances whose register allocation the guard's branches would move (kFrameFastMath)
__device__ __forceinline__ bool exact_in_range(float x, bool plain) {
    return !plain && __builtin_amdgcn_ballot_w64(!(x >= kExactLo && x <= kExactHi)) == 0ull;
}
template <bool FAST = true, bool SHORT = false> __device__ __forceinline__ float inv_sqrt_exact(float x, bool plain, bool &fast) {   // SHORT: inv_sqrt_short for the core
    fast = FAST && exact_in_range(x, plain);
    if (fast) return SHORT ? inv_sqrt_short(x) : rcp_core(sqrt_core(x));
    return 1.0f / sqrtf(x);
}
template <bool FAST = true> __device__ __forceinline__ float sqrt_exact(float x, bool plain, bool &fast) {
    fast = FAST && exact_in_range(x, plain);
    if (fast) return sqrt_core(x);
    return sqrtf(x);
}
// the guard of a whole block of calls (shade_surface): every call notes how far above kExactLo its x lies -- as integers, where the non-negative floats are in order and a
// zero, a denormal, a negative or a NaN wraps or lands above the range's width -- and the block tests the largest note once
__device__ __forceinline__ void exact_note(float x, uint32_t &far) { far = max(far, __float_as_uint(x) - __float_as_uint(kExactLo)); }
__device__ __forceinline__ bool exact_noted_in_range(uint32_t far) { return __builtin_amdgcn_ballot_w64(far > __float_as_uint(kExactHi) - __float_as_uint(kExactLo)) == 0ull; }
template <bool FAST = true> __device__ __forceinline__ float len3(V3 a, bool plain = false) { bool f; return sqrt_exact<FAST>(dot3(a, a), plain, f); }
template <bool FAST = true, bool SHORT = false> __device__ __forceinline__ V3 nrm3(V3 a, bool plain = false) { bool f; float inv = inv_sqrt_exact<FAST, SHORT>(dot3(a, a), plain, f); return a * inv; }
template <bool SHORT = false> __device__ __forceinline__ float inv_sqrt_noting(float x, uint32_t &far) { exact_note(x, far); return SHORT ? inv_sqrt_short(x) : rcp_core(sqrt_core(x)); }   // the core, unguarded, and its note
template <bool CORE, bool SHORT = false> __device__ __forceinline__ V3 nrm3_noting(V3 a, uint32_t &far) {   // CORE: that | the plain expression
    float x = dot3(a, a);
    return a * (CORE ? inv_sqrt_noting<SHORT>(x, far) : 1.0f / sqrtf(x));
}
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
__device__ __forceinline__ V3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
// column-major mat4 times (x,y,z,w), rows 0..2: ((c0*x + c1*y) + c2*z) + c3*w
__device__ __forceinline__ V3 mat4_mul(const float *m, float x, float y, float z, float w) {
    return mk(((m[0] * x + m[4] * y) + m[8] * z) + m[12] * w, ((m[1] * x + m[5] * y) + m[9] * z) + m[13] * w,
              ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w);
}
__device__ __forceinline__ V3 xform_point(const float *m, V3 p) {
    return mk(((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3], ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7],
              ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]);
}
__device__ __forceinline__ V3 xform_vec(const float *m, V3 p) {
    return mk((m[0] * p.x + m[1] * p.y) + m[2] * p.z, (m[4] * p.x + m[5] * p.y) + m[6] * p.z, (m[8] * p.x + m[9] * p.y) + m[10] * p.z);
}

// ------------------------------------------------------------------------------------------------ textures
// sampler2DArray, linear / REPEAT, LOD 0 (no derivatives in a raygen stage): vk_rt_descriptor_set.rs:42-56
__device__ __forceinline__ int wrapi(int i, int n) { int m = i % n; return m < 0 ? m + n : m; }
// wrapi(i + 1, n) for an i that is wrapped already, 0 <= i < n: SEL = a compare and a select instead of the signed remainder -- the same value for every such i
template <bool SEL> __device__ __forceinline__ int wrap_next(int i, int n) { return SEL ? (i + 1 == n ? 0 : i + 1) : wrapi(i + 1, n); }
// the four taps of a bilinear sample and its weights (texture_offset, tw, th: the primitive's texture in the pool) -- sample_tex's first lines, restated for the alpha
// test: shared by a call, the default k_frame instances' register allocation moved (k_frame<true, true, false, false> 63 -> 64 VGPRs)
template <bool SEL = false> __device__ __forceinline__ void tex_taps(const uint32_t *__restrict__ pool, uint32_t texture_offset, uint32_t tw_, uint32_t th_, int layer, float u, float v,
                                         uint32_t &t00, uint32_t &t10, uint32_t &t01, uint32_t &t11, float &fx, float &fy) {
    int tw = (int)tw_, th = (int)th_;
    float x = u * (float)tw - 0.5f, y = v * (float)th - 0.5f;
    float x0f = floorf(x), y0f = floorf(y);
    fx = x - x0f; fy = y - y0f;
    int x0 = wrapi((int)x0f, tw), y0 = wrapi((int)y0f, th);
    int x1 = wrap_next<SEL>(x0, tw), y1 = wrap_next<SEL>(y0, th);
    const uint32_t *base = pool + texture_offset + (size_t)layer * tw * th;
    t00 = base[(size_t)y0 * tw + x0]; t10 = base[(size_t)y0 * tw + x1]; t01 = base[(size_t)y1 * tw + x0]; t11 = base[(size_t)y1 * tw + x1];
}
// channel c (byte c of the RGBA8 texels) of the bilinear sample
__device__ __forceinline__ float tex_channel(uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, float fx, float fy, int c) {
    const float k = 1.0f / 255.0f;
    float A = (float)((t00 >> (8 * c)) & 255u) * k, B = (float)((t10 >> (8 * c)) & 255u) * k;
    float Cc = (float)((t01 >> (8 * c)) & 255u) * k, D = (float)((t11 >> (8 * c)) & 255u) * k;
    float top = A * (1.0f - fx) + B * fx, bot = Cc * (1.0f - fx) + D * fx;
    return top * (1.0f - fy) + bot * fy;
}
template <bool SEL = false> __device__ inline float4 sample_tex(const uint32_t *__restrict__ pool, const DevPrim &P, int layer, float u, float v) {
    int tw = (int)P.tw, th = (int)P.th;
    float x = u * (float)tw - 0.5f, y = v * (float)th - 0.5f;
    float x0f = floorf(x), y0f = floorf(y);
    float fx = x - x0f, fy = y - y0f;
    int x0 = wrapi((int)x0f, tw), y0 = wrapi((int)y0f, th);
    int x1 = wrap_next<SEL>(x0, tw), y1 = wrap_next<SEL>(y0, th);
    const uint32_t *base = pool + P.texture_offset + (size_t)layer * tw * th;
    uint32_t t00 = base[(size_t)y0 * tw + x0], t10 = base[(size_t)y0 * tw + x1], t01 = base[(size_t)y1 * tw + x0], t11 = base[(size_t)y1 * tw + x1];
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; c++) o[c] = tex_channel(t00, t10, t01, t11, fx, fy, c);
    return make_float4(o[0], o[1], o[2], o[3]);
}


// ------------------------------------------------------------------------------------------------ alpha-masked primitives
// A candidate that accept() takes is discarded when its primitive's cutoff c > 0 and alpha < c: alpha = byte 3 of texture layer 0, bilinear / REPEAT / LOD 0 at the
// hit's texture coordinate, made with shade_surface's operations (a visible pixel's shading and its alpha test see the same uv).  Only the instances built with the
// test (template parameter ALPHA) read any of this; the host picks them while some enabled primitive has c > 0.
struct AlphaView {
    const uint32_t *bits;        // one bit per leaf position: its primitive may have c > 0 (FrameArgs::alpha_bits)
    const DevShadeTri *shade;    // the frame's version of the shading records (uv, primitive id) and of the primitive table (c)
    const DevPrim *prims;
    const uint32_t *tex;
    uint32_t cull;               // ray visibility masks: the cull mask of this launch's rays
};
// the alpha of the candidate (pos, u, v) of primitive prim_tex = {texture_offset, tw, th}; uv0..uv2 of its shading record
template <bool SEL = false> __device__ __forceinline__ float alpha_at(const uint32_t *__restrict__ pool, uint32_t texture_offset, uint32_t tw, uint32_t th, float4 s2, float4 s3, float u, float v) {
    float bx = 1.0f - u - v, by = u, bz = v;
    float tu = (s2.y * bx + s2.w * by) + s3.y * bz, tv = (s2.z * bx + s3.x * by) + s3.z * bz;   // shade_surface's tu / tv
    uint32_t t00, t10, t01, t11; float fx, fy;
    tex_taps<SEL>(pool, texture_offset, tw, th, 0, tu, tv, t00, t10, t01, t11, fx, fy);
    return tex_channel(t00, t10, t01, t11, fx, fy, 3);
}
// per-ray walks: true = the candidate at leaf position pos is cut (its lane fetches the record, the cutoff and four texels only if the leaf's bit is set)
// The visibility rule of DESIGN.md 3.4 comes first: a candidate whose primitive's mask shares no bit with the rays' cull mask is discarded before any texel is fetched
// (a cull mask of 0 sees nothing, whatever the leaf bits say: they only mark masks other than 0xFF).
__device__ __forceinline__ bool alpha_cut(const AlphaView &av, uint32_t pos, float u, float v) {
    if (av.cull == 0u) return true;
    if (!((av.bits[pos >> 5] >> (pos & 31u)) & 1u)) return false;
    const float4 *sq = reinterpret_cast<const float4 *>(av.shade + pos);
    const float4 s8 = sq[8];
    const DevPrim &P = av.prims[__float_as_uint(s8.z)];
    if ((prim_vis(P.masked) & av.cull) == 0u) return true;
    const float4 s2 = sq[2], s3 = sq[3];
    const float c = P.cutoff;
    if (!(c > 0.0f)) return false;
    return alpha_at(av.tex, P.texture_offset, P.tw, P.th, s2, s3, u, v) < c;
}

// ------------------------------------------------------------------------------------------------ traversal
struct Ray {
    V3 o, d;
    float tmin, tmax;
    V3 inv, ood;
};
__device__ __forceinline__ float safe_dir(float d) { return fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d; }
__device__ __forceinline__ void ray_init(Ray &r, V3 o, V3 d, float tmin, float tmax) {
    r.o = o; r.d = d; r.tmin = tmin; r.tmax = tmax;
    r.inv = mk(1.0f / safe_dir(d.x), 1.0f / safe_dir(d.y), 1.0f / safe_dir(d.z));
    r.ood = mk(o.x * r.inv.x, o.y * r.inv.y, o.z * r.inv.z);
}
__device__ __forceinline__ void ray_init_inv(Ray &r, V3 o, V3 d, V3 inv, float tmin, float tmax) { // inv = 1 / safe_dir(d), made elsewhere with the same operations
    r.o = o; r.d = d; r.tmin = tmin; r.tmax = tmax; r.inv = inv;
    r.ood = mk(o.x * inv.x, o.y * inv.y, o.z * inv.z);
}
// A ray with a non-finite origin or direction accepts no triangle (every Moeller-Trumbore quantity involves both, and a comparison with NaN is false),
// but it passes every box: fminf / fmaxf drop a NaN operand.  Its lane is switched off before the walk -- the same miss, without the walk of the whole tree.
// (0 * x is 0 for a finite x and NaN otherwise; nothing here is compiled with fast-math.)
__device__ __forceinline__ bool ray_finite(V3 o, V3 d) {
    float z = 0.0f * o.x; z = fmaf(0.0f, o.y, z); z = fmaf(0.0f, o.z, z); z = fmaf(0.0f, d.x, z); z = fmaf(0.0f, d.y, z); z = fmaf(0.0f, d.z, z);
    return z == 0.0f;
}
// monotone slab test against [tmin, tlimit]; tn = un-clamped entry distance
__device__ __forceinline__ bool slab(const Ray &r, float lx, float ly, float lz, float hx, float hy, float hz, float tlimit, float &tn) {
    float t0x = fmaf(lx, r.inv.x, -r.ood.x), t1x = fmaf(hx, r.inv.x, -r.ood.x);
    float t0y = fmaf(ly, r.inv.y, -r.ood.y), t1y = fmaf(hy, r.inv.y, -r.ood.y);
    float t0z = fmaf(lz, r.inv.z, -r.ood.z), t1z = fmaf(hz, r.inv.z, -r.ood.z);
    tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    return fmaxf(tn, r.tmin) <= fminf(tf, tlimit);
}
#define ART_BARY_EPS 1.0e-6f
// Moller-Trumbore, two-sided (instance flags 0, vk_model.rs:374), edges fattened by ART_BARY_EPS, tmin < t < tmax; e1 = v1 - v0, e2 = v2 - v0 (DevTri)
__device__ __forceinline__ bool moller_trumbore(const Ray &r, V3 v0, V3 e1, V3 e2, float &t, float &u, float &v) {
    V3 p = cross3(r.d, e2);
    float det = dot3(e1, p);
    if (det == 0.0f) return false;
    float inv = 1.0f / det;
    V3 tv = r.o - v0;
    float uu = dot3(tv, p) * inv;
    if (!(uu >= -ART_BARY_EPS && uu <= 1.0f + ART_BARY_EPS)) return false;
    V3 q = cross3(tv, e1);
    float vv = dot3(r.d, q) * inv;
    if (!(vv >= -ART_BARY_EPS && uu + vv <= 1.0f + ART_BARY_EPS)) return false;
    float tt = dot3(e2, q) * inv;
    if (!(tt > r.tmin && tt < r.tmax)) return false;
    t = tt; u = uu; v = vv;
    return true;
}
// moller_trumbore, expression for expression, which also hands out its det = dot3(e1, cross3(d, e2)) = -d . (e1 x e2): > 0 the ray goes against the winding normal,
// < 0 along it (art_cast_crossings, DESIGN.md 3.12: the sign of a crossing comes from the evaluation that accepts it)
__device__ __forceinline__ bool moller_trumbore_det(const Ray &r, V3 v0, V3 e1, V3 e2, float &t, float &u, float &v, float &det_out) {
    V3 p = cross3(r.d, e2);
    float det = dot3(e1, p);
    if (det == 0.0f) return false;
    float inv = 1.0f / det;
    V3 tv = r.o - v0;
    float uu = dot3(tv, p) * inv;
    if (!(uu >= -ART_BARY_EPS && uu <= 1.0f + ART_BARY_EPS)) return false;
    V3 q = cross3(tv, e1);
    float vv = dot3(r.d, q) * inv;
    if (!(vv >= -ART_BARY_EPS && uu + vv <= 1.0f + ART_BARY_EPS)) return false;
    float tt = dot3(e2, q) * inv;
    if (!(tt > r.tmin && tt < r.tmax)) return false;
    t = tt; u = uu; v = vv; det_out = det;
    return true;
}

// the same arithmetic without the early exits: in a packet some lane nearly always survives each test, so the wave pays for
// every stage anyway and the exits only add exec-mask bookkeeping (det == 0 lanes compute inf/NaN that the flag discards)
__device__ __forceinline__ bool moller_trumbore_flat(const Ray &r, V3 v0, V3 e1, V3 e2, float &t, float &u, float &v) {
    V3 p = cross3(r.d, e2);
    float det = dot3(e1, p);
    float inv = 1.0f / det;
    V3 tv = r.o - v0;
    u = dot3(tv, p) * inv;
    V3 q = cross3(tv, e1);
    v = dot3(r.d, q) * inv;
    t = dot3(e2, q) * inv;
    return (det != 0.0f) & (u >= -ART_BARY_EPS) & (u <= 1.0f + ART_BARY_EPS) & (v >= -ART_BARY_EPS) & (u + v <= 1.0f + ART_BARY_EPS) & (t > r.tmin) & (t < r.tmax);
}

// the same test for a packet: the lanes that pass, as a mask (each compare's ballot lands in a scalar register pair, the conjunction is scalar work)
__device__ __forceinline__ uint64_t moller_trumbore_mask(const Ray &r, V3 v0, V3 e1, V3 e2, float &t, float &u, float &v) {
    V3 p = cross3(r.d, e2);
    float det = dot3(e1, p);
    float inv = 1.0f / det;
    V3 tv = r.o - v0;
    u = dot3(tv, p) * inv;
    V3 q = cross3(tv, e1);
    v = dot3(r.d, q) * inv;
    t = dot3(e2, q) * inv;
    return __builtin_amdgcn_ballot_w64(det != 0.0f) & __builtin_amdgcn_ballot_w64(u >= -ART_BARY_EPS) & __builtin_amdgcn_ballot_w64(u <= 1.0f + ART_BARY_EPS) &
           __builtin_amdgcn_ballot_w64(v >= -ART_BARY_EPS) & __builtin_amdgcn_ballot_w64(u + v <= 1.0f + ART_BARY_EPS) & __builtin_amdgcn_ballot_w64(t > r.tmin) &
           __builtin_amdgcn_ballot_w64(t < r.tmax);
}

constexpr int kLdsStack = 16;   // per-lane short stack in LDS ([entry][lane], conflict-free); deeper entries spill to scratch
constexpr int kOvfStack = 80;   // 16 + 80 >= the deepest possible radix tree (63 key bits + 32 index bits)
constexpr int kBlock = 256;
constexpr int kFrameBlock = 64;  // the fused frame: one wave per workgroup
constexpr int kTraceBlock = 64;  // the persistent per-ray tracer: likewise (its waves share nothing either)
// tunables of the persistent tracer: {chunk, refill, blocks, leaf_batch}.  Measured on config 2 (profiles/README.md):
// one frame at a time is bound by the slowest wave's critical path -> small chunks, more waves; several frames in flight
// are throughput-bound -> fewer cursor atomics, fewer resident waves.  A context's ArtTuning (trace_chunk / trace_refill / trace_blocks / trace_leaf_batch)
// overrides the presets of ITS launches, for sweeps.
struct Tune { uint32_t chunk, refill, blocks, leaf_batch; };
// [0] / [1]: primary and shadow rays, one frame at a time / several in flight; [2] / [3]: AO rays likewise -- sixteen consecutive slots are one
// pixel's rays, a refill is cheap (k_ao_pixels + k_ao_table), and the kernel fits 8 waves per SIMD: larger chunks (a wave stays on 64 neighbouring
// pixels), all 8 192 wave slots (config 5: 13 700 -> 14 280 Mray/s over the presets of the other rays).  leaf_batch: lanes that must stand on a triangle
// before the wave runs the triangle test.  1 for the other rays (one frame of them at a time is bound by its slowest wave: waiting lanes lengthen it,
// round 1); AO launches are throughput-bound, and a triangle test run for every lone lane was a third of their issued instructions at a tenth of the
// lanes: 2 / 4 / 8 / 12 / 16 lanes -> 14 510 / 14 930 / 15 370 / 15 330 / 15 070 Mray/s on config 5
static const Tune kPreset[4] = {{64, 12, 1536, 1}, {128, 24, 1024, 1}, {256, 16, 2048, 8}, {1024, 24, 2048, 8}};
// the preset for a launch, with the context's overrides (they travel with the launch: nothing process-wide)
static inline Tune tune_over(Tune t, const TraceTune &o) {
    if (o.chunk >= 64 && o.chunk <= 65536) t.chunk = o.chunk;
    if (o.refill >= 1 && o.refill <= 64) t.refill = o.refill;
    if (o.blocks >= 1 && o.blocks <= 16384) t.blocks = o.blocks;
    if (o.leaf_batch >= 1 && o.leaf_batch <= 64) t.leaf_batch = o.leaf_batch;
    return t;
}
static inline Tune tune(bool pipelined, bool ao, const TraceTune &o) { return tune_over(kPreset[(ao ? 2 : 0) + (pipelined ? 1 : 0)], o); }
constexpr int kCursorStride = 32; // one 128-byte line per XCD cursor

// local pixel id -> frame coordinates.  p = tile*1024 + sub*64 + lane; a wave covers an 8x8 pixel block.
__device__ __forceinline__ bool local_to_xy(uint32_t p, const uint32_t *__restrict__ tile_list, uint32_t tiles_x, uint32_t W, uint32_t H, uint32_t &x, uint32_t &y) {
    uint32_t tile = tile_list[p >> 10];
    uint32_t q = p & 1023u, sub = q >> 6, l = q & 63u;
    x = (tile % tiles_x) * kTile + (sub & 3u) * 8u + (l & 7u);
    y = (tile / tiles_x) * kTile + (sub >> 2) * 8u + (l >> 3);
    return x < W && y < H;
}

// the same value, but the compiler cannot know it: what is computed from it is computed again instead of being kept in registers.
// (A "memory" clobber would do that too, and would turn every wave-uniform node fetch after it from a scalar into a vector load.)
__device__ __forceinline__ uint32_t launder(uint32_t v) { asm volatile("" : "+s"(v)); return v; }   // wave-uniform values
__device__ __forceinline__ uint32_t launder_v(uint32_t v) { asm volatile("" : "+v"(v)); return v; } // per-lane values
// v_cmp straight into an SGPR pair (HIP's __ballot(int) goes through v_cndmask + v_cmp_ne)
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// streaming records (hits, shadow rays, contributions, frame outputs) are written once and read once: non-temporal accesses keep
// them from pushing the BVH out of the 4 MB L2s that the walks of all the frames in flight live in
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_nt(float4 *p, float4 v) { __builtin_nontemporal_store(f4v{v.x, v.y, v.z, v.w}, reinterpret_cast<f4v *>(p)); }
__device__ __forceinline__ void st_nt(float *p, float v) { __builtin_nontemporal_store(v, p); }
// the compact tile buffer holds RGB only (12 B per pixel): the colour output's alpha is the constant 1 of imageStore(vec4(rho, 1)), so the
// gather moves three quarters of the bytes of the RGBA32F image and loses nothing
typedef float f3v __attribute__((ext_vector_type(3)));
__device__ __forceinline__ void st_nt_rgb(float4 *tiles, size_t texel, float4 v) { __builtin_nontemporal_store(f3v{v.x, v.y, v.z}, reinterpret_cast<f3v *>(reinterpret_cast<float *>(tiles) + 3 * texel)); }
__device__ __forceinline__ float4 ld_nt(const float4 *p) { f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(p)); return make_float4(v.x, v.y, v.z, v.w); }

// ------------------------------------------------------------------------------------------------ launch shapes
static inline uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }
// persistent grid: enough waves to fill the chip (8 blocks of 4 waves per CU), never more than the work needs
static inline uint32_t persistent_blocks(uint32_t total, const Tune &t) {
    uint32_t need = (total + kTraceBlock - 1) / kTraceBlock, cap = t.blocks * (kBlock / kTraceBlock);   // the presets count 256-thread blocks
    return need < cap ? (need ? need : 1u) : cap;
}

} // namespace art
