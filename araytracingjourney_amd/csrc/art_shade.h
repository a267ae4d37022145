// art_shade.h -- lights (light.glsl), BRDFs (brdfs.glsl) and the surface block of raytrace.rgen.glsl:103-199: what the staged frame's k_shade (art_trace.hip) and the
// fused frame's k_frame (art_frame.hip) both compile, so that their frames are the same bits.  art_sweeps.hip includes it for pow22_texel.
#pragma once
#include "art_device.h"

namespace art {

// ------------------------------------------------------------------------------------------------ lights (light.glsl)
__device__ inline V3 compute_barycentric(V3 a, V3 b, V3 c, V3 p) { // light.glsl:50-68
    V3 v0 = b - a, v1 = c - a, v2 = p - a;
    float d00 = dot3(v0, v0), d01 = dot3(v0, v1), d11 = dot3(v1, v1), d20 = dot3(v2, v0), d21 = dot3(v2, v1);
    float denom = d00 * d11 - d01 * d01;
    V3 r;
    r.x = (d11 * d20 - d01 * d21) / denom;
    r.y = (d00 * d21 - d01 * d20) / denom;
    r.z = 1.0f - r.x - r.y;
    return r;
}
__device__ inline V3 closest_point_to_segment(V3 p0, V3 p1, V3 p) { // light.glsl:70-75
    V3 v01 = p1 - p0;
    float t = dot3(p - p0, v01) / dot3(v01, v01);
    t = clampf(t, 0.0f, 1.0f);
    return p0 + v01 * t;
}
__device__ inline V3 closest_point_to_triangle(V3 p0, V3 p1, V3 p2, V3 pt) { // light.glsl:77-91
    V3 b = compute_barycentric(p0, p1, p2, pt);
    if (b.x < 0.0f) return closest_point_to_segment(p2, p0, pt);
    else if (b.z < 0.0f) return closest_point_to_segment(p1, p2, pt);
    return pt;
}
__device__ inline V3 get_unnormalized_L_vec(const ArtLight &l, V3 pos) { // light.glsl:93-124
    if (l.type == 0u || l.type == 1u) return ld3(l.pos) - pos;
    if (l.type == 2u) return neg(ld3(l.dir)) * 10.0f;
    if (l.type == 3u) {
        V3 ldir = ld3(l.dir), lp = ld3(l.pos), p2 = ld3(l.area_pos2), p3 = ld3(l.area_pos3);
        float distance = dot3(ldir, p2) - dot3(ldir, pos);
        V3 cp = pos + ldir * distance;
        V3 b = compute_barycentric(lp, p2, p3, cp);
        V3 c;
        if (b.x < 0.0f) { V3 p4 = (lp - p2) + p3; c = closest_point_to_triangle(lp, p3, p4, cp); }
        else if (b.y < 0.0f) c = closest_point_to_segment(lp, p2, cp);
        else if (b.z < 0.0f) c = closest_point_to_segment(p2, p3, cp);
        else c = cp;
        return c - pos;
    }
    return mk(1.0f, 1.0f, 1.0f);
}
template <bool FAST> __device__ inline V3 get_light_radiance(const ArtLight &l, V3 pos, V3 L, bool plain) { // light.glsl:34-48
    V3 rad = ld3(l.color);
    if (l.type == 1u || l.type == 3u) {
        float theta_s = acosf(clampf(dot3(ld3(l.dir), neg(L)), -1.0f, 1.0f));
        float t = clampf((theta_s - l.umbra_angle) / (l.penumbra_angle - l.umbra_angle), 0.0f, 1.0f);
        rad = rad * (t * t);
    }
    if (l.falloff_distance > 0.0f) {
        float q = __fdividef(len3<FAST>(ld3(l.pos) - pos, plain), l.falloff_distance);
        float w = fmaxf(1.0f - q * q, 0.0f);
        rad = rad * (w * w);
    }
    return rad;
}

// ------------------------------------------------------------------------------------------------ BRDFs (brdfs.glsl)
#define ART_INV_PI (1.0f / 3.14159265359f)
__device__ __forceinline__ float D_GGX(float a_, float NdotH) { // brdfs.glsl:6-14
    float om = 1.0f - NdotH * NdotH;
    float a = NdotH * a_;
    float k = __fdividef(a_, om + a * a);
    return k * k * ART_INV_PI;
}
__device__ __forceinline__ float V_SmithGGXCorrelated_fast(float a_, float NdotV, float NdotL) { // brdfs.glsl:25-29
    return __fdividef(0.5f, mixf(2.0f * NdotL * NdotV, NdotL + NdotV, a_));
}
__device__ __forceinline__ float pow5(float x) { float x2 = x * x; return x2 * x2 * x; }
__device__ __forceinline__ float F_Schlick1(float F0, float F90, float x) { return F0 + (F90 - F0) * pow5(1.0f - x); } // brdfs.glsl:44-49
__device__ inline float Burley_diffuse_local_sss(float a_, float NdotV, float nc_NdotV, float nc_NdotL, float LdotH, float ratio) { // brdfs.glsl:89-99
    float F_SS90 = a_ * LdotH * LdotH;
    float F_SS = F_Schlick1(1.0f, F_SS90, nc_NdotL) * F_Schlick1(1.0f, F_SS90, nc_NdotV);
    float f_ss = (__fdividef(1.0f, nc_NdotV * nc_NdotL) - 0.5f) * F_SS + 0.5f;
    float local_sss = 1.25f * ratio * f_ss;
    float f90 = 0.5f + 2.0f * F_SS90;
    float diffuse = (1.0f - ratio) * F_Schlick1(1.0f, f90, nc_NdotL) * F_Schlick1(1.0f, f90, nc_NdotV);
    return NdotV * (diffuse + local_sss) * ART_INV_PI;
}
// x^2.2 of a texel (the albedo's gamma; radiance only) in twelve vector instructions, two of them transcendental, where hipcc's __powf is the full libm pow (~143).
// x = m 2^e with m in [0.5, 1): 2.2 e = n + f with n an integer and |f| <= 1/2 exact (e is small), so x^2.2 = 2^n 2^(2.2 log2 m + f) and the rounded product
// stays below 2.8 in magnitude -- the one-line exp2(2.2 log2 x) rounds a product of up to 18 and loses 1.5e-6 relative at dark texels.  Exactly 0 at 0 and 1 at 1,
// NaN passes through; correct on [0, 2], no sign / integer-y / infinity handling (art_parity_radiance_sweep measures it against libm's pow over that whole range).
// Underflow is libm's: its pow returns 0 for every x below 0x1d9aa2a3 (4.09e-21: x^2.2 just under 2^-149) and the smallest denormal from there on, where round-to-nearest
// would already give that denormal from 2^-150 (x = 2.99e-21) on.  Such an x counts as 0 here too -- a compare and a select -- so that the result's class is libm's on
// every input; no texel is that small (a blend of bytes / 255 is 0 or at least 2^-56).
constexpr uint32_t kPow22UnderflowBits = 0x1d9aa2a3u;
__device__ __forceinline__ float pow22_texel(float x) {
    x = x < __uint_as_float(kPow22UnderflowBits) ? 0.0f : x;
    const float fe = (float)__builtin_amdgcn_frexp_expf(x), m = __builtin_amdgcn_frexp_mantf(x);
    const float n = rintf(2.2f * fe), f = fmaf(2.2f, fe, -n);
    const float g = fmaf(2.2f, __builtin_amdgcn_logf(m), f);
    return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(g), (int)n);
}

// ---- shading (raytrace.rgen.glsl:103-199), shared by the staged frame (k_shade) and the fused frame (k_frame) ---------
struct Surface { V3 world_pos, N, Vv, albedo; float metallic, alpha, nc_NdotV, NdotV; };

// rgen:107-150: the hit triangle's attributes, normal mapping, material; also the frame's depth / view-space normal outputs
// SITES: bit k = the block's k-th normalisation in its ten-instruction form (inv_sqrt_short) where CORE; SEL: the second taps' wrap as a compare and a select (wrap_next)
template <bool CORE, bool HOLD = false, uint32_t SITES = 0u, bool SEL = false> __device__ __forceinline__ void shade_surface_body(const FrameArgs &a, const CameraArg &cam, uint32_t pos, float hu, float hv, Surface &S, float &out_depth, V3 &out_normal, uint32_t &far) {
    // one dependent fetch: the shading record holds what get_indices + three vertex reads would return (rgen:107-114)
    const float4 *sq = reinterpret_cast<const float4 *>(a.shade_tris + pos);
    float4 s0 = sq[0], s1 = sq[1], s2 = sq[2], s3 = sq[3], s4 = sq[4], s5 = sq[5], s6 = sq[6], s7 = sq[7], s8 = sq[8];
    const DevPrim &P = a.prims[__float_as_uint(s8.z)];
    float bx = 1.0f - hu - hv, by = hu, bz = hv;
    V3 posv = (mk(s0.x, s0.y, s0.z) * bx + mk(s0.w, s1.x, s1.y) * by) + mk(s1.z, s1.w, s2.x) * bz;
    V3 world_pos = xform_point(P.o2w, posv);
    float tu = (s2.y * bx + s2.w * by) + s3.y * bz, tv = (s2.z * bx + s3.x * by) + s3.z * bz;
    V3 nrm = nrm3_noting<CORE, (SITES >> 0 & 1u) != 0u>((mk(s3.w, s4.x, s4.y) * bx + mk(s4.z, s4.w, s5.x) * by) + mk(s5.y, s5.z, s5.w) * bz, far);
    const float *Wm = P.w2o;
    V3 world_normal = nrm3_noting<CORE, (SITES >> 1 & 1u) != 0u>(mk(dot3(nrm, mk(Wm[0], Wm[4], Wm[8])), dot3(nrm, mk(Wm[1], Wm[5], Wm[9])), dot3(nrm, mk(Wm[2], Wm[6], Wm[10]))), far);
    V3 tan = nrm3_noting<CORE, (SITES >> 2 & 1u) != 0u>((mk(s6.x, s6.y, s6.z) * bx + mk(s6.w, s7.x, s7.y) * by) + mk(s7.z, s7.w, s8.x) * bz, far);
    V3 world_tangent = nrm3_noting<CORE, (SITES >> 3 & 1u) != 0u>(xform_vec(P.o2w, tan), far);
    world_tangent = nrm3_noting<CORE, (SITES >> 4 & 1u) != 0u>(world_tangent - world_normal * dot3(world_tangent, world_normal), far);
    V3 world_binormal = cross3(world_normal, world_tangent) * s8.y;
    float4 tx = sample_tex<SEL>(a.tex_pool, P, 2, tu, tv);
    V3 N = nrm3_noting<CORE, (SITES >> 5 & 1u) != 0u>(mk(tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f), far);
    N = nrm3_noting<CORE, (SITES >> 6 & 1u) != 0u>((world_tangent * N.x + world_binormal * N.y) + world_normal * N.z, far);
    tx = sample_tex<SEL>(a.tex_pool, P, 0, tu, tv);
    V3 albedo = mk(pow22_texel(tx.x), pow22_texel(tx.y), pow22_texel(tx.z)); // radiance-only from here: pow22_texel is within 8 ulp of libm's pow (the BRDF's __fdividef is the IEEE division on this toolchain)
    tx = sample_tex<SEL>(a.tex_pool, P, 1, tu, tv);
    float roughness = tx.y, metallic = tx.z;
    S.world_pos = world_pos; S.N = N; S.albedo = albedo; S.metallic = metallic;
    S.Vv = nrm3_noting<CORE, (SITES >> 7 & 1u) != 0u>(ld3(cam.camera_pos) - world_pos, far); // exact: V + L cancels at grazing angles and would amplify a 1-ulp rsq
    S.alpha = roughness * roughness;
    S.nc_NdotV = dot3(N, S.Vv);
    S.NdotV = clampf(S.nc_NdotV, 1e-5f, 1.0f);
    V3 vp = mat4_mul(cam.view, world_pos.x, world_pos.y, world_pos.z, 1.0f);
    out_depth = -vp.z;
    const float *VI = cam.view_inv;
    V3 on = mk((VI[0] * N.x + VI[1] * N.y) + VI[2] * N.z, (VI[4] * N.x + VI[5] * N.y) + VI[6] * N.z, (VI[8] * N.x + VI[9] * N.y) + VI[10] * N.z);
    on.y = -on.y; on.z = -on.z;
    on = nrm3_noting<CORE, (SITES >> 8 & 1u) != 0u>(on, far);
    out_normal = mk(on.x * 0.5f + 0.5f, on.y * 0.5f + 0.5f, on.z * 0.5f + 0.5f);
    // HOLD (the four k_frame instances <*, true, *, false, true>: one light, one frame per launch, alpha test): libm's pow was what took those instances to 61 VGPRs; without
    // it they need 58, and the figure is pinned to the register (tests/test_ray_masks.py).  The block's last result passes through v60 -- a move there and back -- so they claim 61.
    if (HOLD) { asm volatile("" : "+{v60}"(out_normal.x)); }
}

// The surface block's nine normalisations under ONE guard: a branch in front of each (inv_sqrt_exact) cuts the block into ten scheduling regions and moves the register
// allocation of every k_frame instance; here the block runs the core straight through, notes the range of what it was given, and a wave in which any lane's note is out
// of range runs the block again with the plain expressions (a normal of length zero, a NaN vertex: nothing a frame has many of).  What the first pass computed from such a
// value is discarded whole: no address depends on a normalised vector, so it is arithmetic on garbage and nothing else.
template <bool FAST, bool HOLD = false, uint32_t SITES = 0u, bool SEL = false> __device__ __forceinline__ void shade_surface(const FrameArgs &a, const CameraArg &cam, uint32_t pos, float hu, float hv, Surface &S, float &out_depth, V3 &out_normal) {
    uint32_t far = 0u;
    if (FAST) { if (!a.plain_math) { shade_surface_body<true, false, SITES, SEL>(a, cam, pos, hu, hv, S, out_depth, out_normal, far); if (exact_noted_in_range(far)) return; } }
    shade_surface_body<false, HOLD, 0u, SEL>(a, cam, pos, hu, hv, S, out_depth, out_normal, far);
}
// rgen:152-185 up to the shadow ray: c = (rho_s + rho_d) * radiance, c.w = NdotL; the shadow ray (origin, tmax | direction) if one is due
// SHORT: L's and H's normalisations in their ten-instruction form behind their guards
template <bool FAST, bool SHORT = false> __device__ __forceinline__ bool shade_light(const ArtLight &l, const Surface &S, bool plain, float4 &c4, float4 &ro, float4 &rd) {
    // a directional light's L and |nn_L| do not depend on the pixel: the host made them (art_api.hip directional_constants, the same operations)
    const bool directional = l.type == 2u;
    V3 nn_L = directional ? mk(0.f, 0.f, 0.f) : get_unnormalized_L_vec(l, S.world_pos);
    V3 L = directional ? ld3(l.area_pos2) : nrm3<FAST, SHORT>(nn_L, plain);
    V3 Hh = nrm3<FAST, SHORT>(S.Vv + L, plain);
    float nc_NdotL = dot3(S.N, L);
    float NdotL = clampf(nc_NdotL, 0.0f, 1.0f);
    float NdotH = clampf(dot3(S.N, Hh), 0.0f, 1.0f);
    float LdotH = clampf(dot3(L, Hh), 0.0f, 1.0f);
    float sch = pow5(1.0f - LdotH);
    V3 F0 = mk(mixf(0.04f, S.albedo.x, S.metallic), mixf(0.04f, S.albedo.y, S.metallic), mixf(0.04f, S.albedo.z, S.metallic));
    V3 Ks = mk(F0.x + (1.0f - F0.x) * sch, F0.y + (1.0f - F0.y) * sch, F0.z + (1.0f - F0.z) * sch);
    V3 Kd = S.albedo * (1.0f - S.metallic);
    float DG = D_GGX(S.alpha, NdotH) * V_SmithGGXCorrelated_fast(S.alpha, S.NdotV, NdotL);
    V3 rho_s = Ks * DG;
    V3 rho_d = Kd * Burley_diffuse_local_sss(S.alpha, S.NdotV, S.nc_NdotV, nc_NdotL, LdotH, 0.4f);
    V3 rad = get_light_radiance<FAST>(l, S.world_pos, L, plain);
    V3 c = (rho_s + rho_d) * rad;
    c4 = make_float4(c.x, c.y, c.z, NdotL);
    if (l.casts_shadows && nc_NdotL > 0.0f) { // raytrace.rgen.glsl:165: origin world_pos, dir L, tmax length(nn_L)
        ro = make_float4(S.world_pos.x, S.world_pos.y, S.world_pos.z, directional ? l.penumbra_angle : len3<FAST>(nn_L, plain));
        rd = make_float4(L.x, L.y, L.z, 0.f);
        return true;
    }
    return false;
}

// Light i of a frame: the first kMaxLights records travel by value in the kernel arguments (FrameArgs::lights), the rest -- the reference's list is a Vec, vk_lights.rs:89-91 --
// in a table of the frame's ring slot.  Both are read through the constant address space (wave-uniform, read-only: scalar loads, also behind the frame's own stores).
// (The argument copy is addressed through the kernel-argument segment pointer: FrameArgs is the first -- by-value -- argument of k_frame and k_shade, and taking the address of
// a.lights[i] itself would make the compiler copy all 2.6 KB of it to scratch.)
__device__ __forceinline__ ArtLight frame_light(const FrameArgs &a, uint32_t i) {
    ArtLight L;
#ifdef __HIP_DEVICE_COMPILE__
    typedef __attribute__((address_space(4))) const uint32_t *Words;
    const Words args = (Words)((__attribute__((address_space(4))) const char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FrameArgs, lights));
    const Words p = i < (uint32_t)kMaxLights ? args + i * (uint32_t)(sizeof(ArtLight) / 4) : (Words)(uintptr_t)(a.lights_more + (i - (uint32_t)kMaxLights));
    uint32_t w[sizeof(ArtLight) / 4];
#pragma unroll
    for (uint32_t k = 0; k < sizeof(ArtLight) / 4; k++) w[k] = p[k];
    __builtin_memcpy(&L, w, sizeof(ArtLight));
#else
    L = a.lights[i < (uint32_t)kMaxLights ? i : 0];   // (host pass of the compiler only)
#endif
    return L;
}

} // namespace art
