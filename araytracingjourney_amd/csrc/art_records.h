// art_records.h -- what the build units (art_build.hip, art_wide.hip, art_refit.hip) share: ONE copy of each record operation.  A refit writes the bits of a build
// because both call these: the index fetch, the shading record's gather, the triangle record from three world points, a child's box, the 4-wide node's quantisation.
#pragma once
#include "art_internal.h"
#include <cmath>

namespace art {

__device__ inline float3 xform_point(const float *m, float x, float y, float z) {
    return make_float3(((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
                       ((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
}
// ceil(log2(x)) for x > 0, exactly (frexp is exact; log2 of a double is not guaranteed to be the same on the host and the device)
__host__ __device__ inline int ceil_log2(double x) { int ex; double m = frexp(x, &ex); return m == 0.5 ? ex - 1 : ex; }
// the vertex indices of triangle tl of a primitive (u16 or u32 triples: get_indices of raytrace.rgen.glsl)
__device__ __forceinline__ void fetch_indices(const DevPrim &P, uint32_t tl, uint32_t ix[3]) {
    if (P.single_index_size == 2) { const uint16_t *q = (const uint16_t *)P.indices + 3 * (size_t)tl; ix[0] = q[0]; ix[1] = q[1]; ix[2] = q[2]; }
    else { const uint32_t *q = (const uint32_t *)P.indices + 3 * (size_t)tl; ix[0] = q[0]; ix[1] = q[1]; ix[2] = q[2]; }
}
// shading record of triangle tl of primitive `prim`: get_indices + three vertex fetches of raytrace.rgen.glsl:107-114, done once
__device__ __forceinline__ DevShadeTri gather_shade_tri(const DevPrim &P, uint32_t prim, uint32_t tl) {
    uint32_t ix[3]; fetch_indices(P, tl, ix);
    DevShadeTri st;
    for (int k = 0; k < 3; k++) {
        const float *v = P.vertices + (size_t)ix[k] * 12;
        for (int j = 0; j < 3; j++) { st.f[3 * k + j] = v[j]; st.f[15 + 3 * k + j] = v[5 + j]; st.f[24 + 3 * k + j] = v[8 + j]; }
        st.f[9 + 2 * k] = v[3]; st.f[10 + 2 * k] = v[4];
        if (k == 0) st.f[33] = v[11];
    }
    st.f[34] = __uint_as_float(prim); st.f[35] = 0.f;
    return st;
}
// triangle record from three world points: v0, the two edges, the box (DevTri: the float operations the ray tests would otherwise repeat) and the gid's bits
__device__ __forceinline__ DevTri make_dev_tri(const float *a, const float *b, const float *c, float gid_bits) {
    DevTri t;
    for (int k = 0; k < 3; k++) {
        t.f[k] = a[k]; t.f[3 + k] = b[k] - a[k]; t.f[6 + k] = c[k] - a[k];
        t.f[9 + k] = fminf(fminf(a[k], b[k]), c[k]); t.f[12 + k] = fmaxf(fmaxf(a[k], b[k]), c[k]);
    }
    t.f[15] = gid_bits;
    return t;
}
// the box of a child reference of a binary tree: a leaf's (ref < 0: ~position) or a node's
__device__ __forceinline__ void child_box(int32_t ref, const float *leaf_lo, const float *leaf_hi, const float *node_lo, const float *node_hi, const float *&lo, const float *&hi) {
    lo = ref < 0 ? leaf_lo + 3 * (size_t)(~ref) : node_lo + 3 * (size_t)ref;
    hi = ref < 0 ? leaf_hi + 3 * (size_t)(~ref) : node_hi + 3 * (size_t)ref;
}
// The quantised record of a 4-wide node from its nc child boxes: origin = the boxes' common corner, one power-of-two scale per axis, 8-bit planes rounded
// outwards so that origin + q * scale -- as the walks' fma evaluates it -- contains the float box.  Shared by the collapse and by the refit.
__device__ inline void wide_quantise(const float *const lo[4], const float *const hi[4], int nc, DevNode4 &d) {
    for (int k = 0; k < 6; k++) d.q[k] = 0;
    d.spare[0] = d.spare[1] = 0;
    float org[3] = {INFINITY, INFINITY, INFINITY}, top[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < nc; i++) if (!box_nowhere(lo[i][0])) for (int k = 0; k < 3; k++) { org[k] = fminf(org[k], lo[i][k]); top[k] = fmaxf(top[k], hi[i][k]); }
    if (org[0] > top[0]) for (int k = 0; k < 3; k++) { org[k] = 0.f; top[k] = 0.f; }   // every child masked (refit): any frame of reference will do
    d.ox = org[0]; d.oy = org[1]; d.oz = org[2];
    uint32_t ebits[3]; float scale[3];
    for (int k = 0; k < 3; k++) { // smallest power of two with 255 * scale >= extent (as evaluated by the tracer's fma), at least 2^-100
        double ext = (double)top[k] - (double)org[k];
        int e = ext > 0 ? ceil_log2(ext / 255.0) : -100;
        if (e < -100) e = -100;
        for (;;) { scale[k] = ldexpf(1.0f, e); if (fmaf(255.0f, scale[k], org[k]) >= top[k]) break; e++; }
        while (e > -100 && fmaf(255.0f, ldexpf(1.0f, e - 1), org[k]) >= top[k]) { e--; scale[k] = ldexpf(1.0f, e); }   // (the fma may round half the scale's last plane UP onto the top: the smallest scale is the one the walks' own evaluation allows)
        ebits[k] = (uint32_t)(e + 127);
    }
    uint32_t mask = 0;
    for (int i = nc; i < 4; i++) for (int k = 0; k < 3; k++) d.q[k] |= 255u << (8 * i); // an absent child: an inverted box (lo planes 255, hi planes 0), which the per-ray walk's sign-selected slab never enters
    for (int i = 0; i < nc; i++) {
        mask |= 1u << i;
        if (box_nowhere(lo[i][0])) { for (int k = 0; k < 3; k++) d.q[k] |= 255u << (8 * i); continue; }   // a masked subtree: the inverted box of an absent child
        for (int k = 0; k < 3; k++) {
            int ql = (int)floor(((double)lo[i][k] - (double)org[k]) / (double)scale[k]);
            int qh = (int)ceil(((double)hi[i][k] - (double)org[k]) / (double)scale[k]);
            ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql); qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
            while (ql > 0 && fmaf((float)ql, scale[k], org[k]) > lo[i][k]) ql--;
            while (qh < 255 && fmaf((float)qh, scale[k], org[k]) < hi[i][k]) qh++;
            // floor / ceil are of the exact quotient, but the fma may round the next plane inwards exactly ONTO the box: a tighter value that still contains it, so take it
            // (only a value that differs: a flat box on a 2^-100 axis keeps lo plane <= hi plane -- an inverted pair means "absent")
            for (float v; ql < 255 && (v = fmaf((float)(ql + 1), scale[k], org[k])) <= lo[i][k] && v > fmaf((float)ql, scale[k], org[k]);) ql++;
            for (float v; qh > 0 && (v = fmaf((float)(qh - 1), scale[k], org[k])) >= hi[i][k] && v < fmaf((float)qh, scale[k], org[k]);) qh--;
            d.q[k] |= (uint32_t)ql << (8 * i);
            d.q[3 + k] |= (uint32_t)qh << (8 * i);
        }
    }
    d.exps = ebits[0] | (ebits[1] << 8) | (ebits[2] << 16) | (mask << 24);
}

} // namespace art
