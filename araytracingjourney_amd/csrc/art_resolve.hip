// art_resolve.hip -- art_resolve_hits (include/art.h): the surface behind the hit records a cast wrote.  A gather and an interpolation, one lane per
// record: no rays, no tree, no lights.  The values are those of shade_surface_body<false> (art_shade.h) up to N, the texture coordinate and the two material layers --
// the plain expressions in the same order -- plus the geometric normal of the world triangle.  The vector helpers and the sampler's pieces are art_device.h's own; only
// the sampler's entry is restated (sample_layer: it clamps the texel coordinate of a caller's record, which sample_tex has no need to).
#include "art_device.h"

namespace art {

namespace {
__device__ __forceinline__ V3 nrm3_plain(V3 a) { return a * (1.0f / sqrtf(dot3(a, a))); }   // the plain expression: what nrm3_noting<false> computes
__device__ __forceinline__ float4 f4(V3 a, float w) { return make_float4(a.x, a.y, a.z, w); }

// sample_tex of art_device.h: sampler2DArray, linear / REPEAT, LOD 0.  One difference, for a caller's records: the texel coordinate is clamped to +-2^30 before it
// becomes an integer (the frame's uv come from hits inside a triangle; a record may extrapolate to anything finite, and the product may overflow).  Inside that range --
// every float with a fraction lies far inside it -- the operations and the bits are sample_tex's.
__device__ __forceinline__ int texel_int(float f) { return (int)fminf(fmaxf(f, -1073741824.0f), 1073741824.0f); }   // (a NaN comes out as the bound: fmaxf returns the other operand)
__device__ __forceinline__ float4 sample_layer(const uint32_t *__restrict__ pool, uint32_t texture_offset, int tw, int th, int layer, float u, float v) {
    float x = u * (float)tw - 0.5f, y = v * (float)th - 0.5f;
    float x0f = floorf(x), y0f = floorf(y);
    float fx = x - x0f, fy = y - y0f;
    int x0 = wrapi(texel_int(x0f), tw), y0 = wrapi(texel_int(y0f), th);
    int x1 = wrapi(x0 + 1, tw), y1 = wrapi(y0 + 1, th);
    const uint32_t *base = pool + texture_offset + (size_t)layer * tw * th;
    uint32_t t00 = base[(size_t)y0 * tw + x0], t10 = base[(size_t)y0 * tw + x1], t01 = base[(size_t)y1 * tw + x0], t11 = base[(size_t)y1 * tw + x1];
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; c++) o[c] = tex_channel(t00, t10, t01, t11, fx, fy, c);
    return make_float4(o[0], o[1], o[2], o[3]);
}
} // namespace

// One lane per record.  What the record says is the CALLER's: every index is checked against the structure's own bounds before an address is formed from it, and a
// record that fails any check gets the miss record -- zeros in every buffer given.  Which buffers are given is uniform over the launch: the branches on them are scalar.
__global__ __launch_bounds__(256) void k_resolve(ResolveArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const float4 h = a.tuv[i];
    const int2 id = a.ids[i];
    const float hu = h.y, hv = h.z;
    bool ok = id.x >= 0 && (uint32_t)id.x < a.n_prims && id.y >= 0 && fabsf(hu) < INFINITY && fabsf(hv) < INFINITY;   // (a NaN compares false)
    uint32_t leaf = 0;
    if (ok) {
        const DevPrim &Q = a.prims[id.x];
        const uint32_t n_tri = Q.n_tri, gid = Q.first_tri + (uint32_t)id.y;   // n_tri = 0: a primitive the built structure does not hold
        ok = (uint32_t)id.y < n_tri && gid < a.T && Q.tw > 0u && Q.th > 0u;
        if (ok) { leaf = a.gid_leaf[gid]; ok = leaf < a.T; }
    }
    float4 o_pos = make_float4(0.f, 0.f, 0.f, 0.f), o_ng = o_pos, o_ns = o_pos, o_albedo = o_pos, o_orm = o_pos;
    float2 o_uv = make_float2(0.f, 0.f);
    if (ok) {
        const float4 *sq = reinterpret_cast<const float4 *>(a.shade + leaf);
        float4 s0 = sq[0], s1 = sq[1], s2 = sq[2], s3 = sq[3], s4 = sq[4], s5 = sq[5], s6 = sq[6], s7 = sq[7], s8 = sq[8];
        const DevPrim &P = a.prims[id.x];
        float bx = 1.0f - hu - hv, by = hu, bz = hv;
        const V3 p0 = mk(s0.x, s0.y, s0.z), p1 = mk(s0.w, s1.x, s1.y), p2 = mk(s1.z, s1.w, s2.x);
        if (a.pos) o_pos = f4(xform_point(P.o2w, (p0 * bx + p1 * by) + p2 * bz), 1.0f);
        if (a.ng) {
            const V3 w0 = xform_point(P.o2w, p0), w1 = xform_point(P.o2w, p1), w2 = xform_point(P.o2w, p2);
            const V3 c = cross3(w1 - w0, w2 - w0);
            const float l2 = dot3(c, c);
            if (l2 > 0.0f && l2 < INFINITY) o_ng = f4(c * (1.0f / sqrtf(l2)), 0.0f);   // a zero cross product (or one whose squared length is no number to divide by): (0, 0, 0)
        }
        const float tu = (s2.y * bx + s2.w * by) + s3.y * bz, tv = (s2.z * bx + s3.x * by) + s3.z * bz;
        if (a.uv) o_uv = make_float2(tu, tv);
        const int tw = (int)P.tw, th = (int)P.th;
        if (a.ns) {
            V3 nrm = nrm3_plain((mk(s3.w, s4.x, s4.y) * bx + mk(s4.z, s4.w, s5.x) * by) + mk(s5.y, s5.z, s5.w) * bz);
            const float *Wm = P.w2o;
            V3 world_normal = nrm3_plain(mk(dot3(nrm, mk(Wm[0], Wm[4], Wm[8])), dot3(nrm, mk(Wm[1], Wm[5], Wm[9])), dot3(nrm, mk(Wm[2], Wm[6], Wm[10]))));
            V3 tan = nrm3_plain((mk(s6.x, s6.y, s6.z) * bx + mk(s6.w, s7.x, s7.y) * by) + mk(s7.z, s7.w, s8.x) * bz);
            V3 world_tangent = nrm3_plain(xform_vec(P.o2w, tan));
            world_tangent = nrm3_plain(world_tangent - world_normal * dot3(world_tangent, world_normal));
            V3 world_binormal = cross3(world_normal, world_tangent) * s8.y;
            float4 tx = sample_layer(a.tex_pool, P.texture_offset, tw, th, 2, tu, tv);
            V3 N = nrm3_plain(mk(tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f));
            N = nrm3_plain((world_tangent * N.x + world_binormal * N.y) + world_normal * N.z);
            o_ns = f4(N, 0.0f);
        }
        if (a.albedo) o_albedo = sample_layer(a.tex_pool, P.texture_offset, tw, th, 0, tu, tv);
        if (a.orm) o_orm = sample_layer(a.tex_pool, P.texture_offset, tw, th, 1, tu, tv);
    }
    if (a.pos) a.pos[i] = o_pos;
    if (a.ng) a.ng[i] = o_ng;
    if (a.ns) a.ns[i] = o_ns;
    if (a.uv) a.uv[i] = o_uv;
    if (a.albedo) a.albedo[i] = o_albedo;
    if (a.orm) a.orm[i] = o_orm;
}

void launch_resolve(const ResolveArgs &r, hipStream_t s) {
    if (r.n) k_resolve<<<(r.n + 255u) / 256u, 256, 0, s>>>(r);
}

} // namespace art
