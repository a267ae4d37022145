// art_build.hip -- device LBVH builder over the world-space triangle soup (gfx950).
// Replaces the closed driver work behind VkBlasBuilder::build_blas_from_geometry (vk_blas_builder.rs:88-170,
// vkCmdBuildAccelerationStructuresKHR, PREFER_FAST_TRACE) and VkTlasBuilder::recreate_tlas
// (vk_tlas_builder.rs:38-233): instances are folded into the soup (one instance per model, renderer.rs:641-650).
// Pipeline: soup (index fetch + object->world) -> centroid bounds (ordered-int atomics) -> Morton keys ->
// stable radix sort (rocPRIM) -> Karras 2012 radix tree -> bottom-up AABB refit (arrival counters) ->
// 64-byte traversal nodes + 64-byte leaf-ordered triangle records.  The 4-wide collapse of the traversal tree is art_wide.hip's, the per-frame refit
// art_refit.hip's; the record operations the three share are art_records.h's.
#include "art_records.h"
#include <rocprim/rocprim.hpp>

namespace art {

__device__ inline uint32_t f2ord(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ inline float ord2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
constexpr uint32_t kCbSlots = 64;

// one thread per triangle: fetch indices + vertices, transform, write world triangle, its AABB, reduce centroid bounds
__global__ __launch_bounds__(256) void k_soup(const DevPrim *__restrict__ prims, uint32_t n_prims, const uint32_t *__restrict__ first_tri,
                                              uint32_t T, float *__restrict__ triw /*T*9*/, float *__restrict__ tlo, float *__restrict__ thi,
                                              uint32_t *__restrict__ tri_prim, uint32_t *__restrict__ cslots /*kCbSlots x 32 words: 6 ordered ints each, a slot per 128-byte line*/) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    float cx = 0, cy = 0, cz = 0;
    bool on = g < T;
    if (on) {
        uint32_t lo = 0, hi = n_prims; // last p with first_tri[p] <= g
        while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (first_tri[mid] <= g) lo = mid; else hi = mid; }
        const DevPrim &P = prims[lo];
        uint32_t ix[3]; fetch_indices(P, g - P.first_tri, ix);
        const float *a = P.vertices + (size_t)ix[0] * 12, *b = P.vertices + (size_t)ix[1] * 12, *c = P.vertices + (size_t)ix[2] * 12;
        float3 w0 = xform_point(P.o2w, a[0], a[1], a[2]), w1 = xform_point(P.o2w, b[0], b[1], b[2]), w2 = xform_point(P.o2w, c[0], c[1], c[2]);
        float *o = triw + (size_t)g * 9;
        o[0] = w0.x; o[1] = w0.y; o[2] = w0.z; o[3] = w1.x; o[4] = w1.y; o[5] = w1.z; o[6] = w2.x; o[7] = w2.y; o[8] = w2.z;
        float lx = fminf(fminf(w0.x, w1.x), w2.x), ly = fminf(fminf(w0.y, w1.y), w2.y), lz = fminf(fminf(w0.z, w1.z), w2.z);
        float hx = fmaxf(fmaxf(w0.x, w1.x), w2.x), hy = fmaxf(fmaxf(w0.y, w1.y), w2.y), hz = fmaxf(fmaxf(w0.z, w1.z), w2.z);
        tlo[3 * (size_t)g] = lx; tlo[3 * (size_t)g + 1] = ly; tlo[3 * (size_t)g + 2] = lz;
        thi[3 * (size_t)g] = hx; thi[3 * (size_t)g + 1] = hy; thi[3 * (size_t)g + 2] = hz;
        tri_prim[g] = lo;
        cx = (lx + hx) * 0.5f; cy = (ly + hy) * 0.5f; cz = (lz + hz) * 0.5f;
    }
    // wave reduction of the ordered keys, then one atomic per wave
    uint32_t kmin[3] = {on ? f2ord(cx) : 0xFFFFFFFFu, on ? f2ord(cy) : 0xFFFFFFFFu, on ? f2ord(cz) : 0xFFFFFFFFu};
    uint32_t kmax[3] = {on ? f2ord(cx) : 0u, on ? f2ord(cy) : 0u, on ? f2ord(cz) : 0u};
    for (int off = 32; off >= 1; off >>= 1)
        for (int k = 0; k < 3; k++) {
            kmin[k] = min(kmin[k], (uint32_t)__shfl_xor((int)kmin[k], off));
            kmax[k] = max(kmax[k], (uint32_t)__shfl_xor((int)kmax[k], off));
        }
    // (every wave of the launch on the same six words was 2.7 of the 3.0 ms this kernel took for the 2.8 M triangles of config 4: the waves are dealt to 64 slots, k_cb_fold joins them)
    if ((threadIdx.x & 63) == 0) {
        uint32_t *cb = cslots + ((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) % kCbSlots) * 32;
        for (int k = 0; k < 3; k++) { atomicMin(&cb[k], kmin[k]); atomicMax(&cb[3 + k], kmax[k]); }
    }
}
__global__ __launch_bounds__(64) void k_cb_init(uint32_t *cslots) { for (int k = 0; k < 6; k++) cslots[threadIdx.x * 32 + k] = k < 3 ? 0xFFFFFFFFu : 0u; }
__global__ __launch_bounds__(64) void k_cb_fold(const uint32_t *__restrict__ cslots, uint32_t *__restrict__ cbounds) {
    uint32_t v[6];
    for (int k = 0; k < 6; k++) v[k] = cslots[threadIdx.x * 32 + k];
    for (int off = 32; off >= 1; off >>= 1) for (int k = 0; k < 6; k++) { uint32_t o = (uint32_t)__shfl_xor((int)v[k], off); v[k] = k < 3 ? min(v[k], o) : max(v[k], o); }
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) cbounds[k] = v[k];
}

__device__ inline uint32_t expand10(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ inline uint64_t expand21(uint64_t v) {
    v &= 0x1fffffull;
    v = (v | (v << 32)) & 0x1f00000000ffffull; v = (v | (v << 16)) & 0x1f0000ff0000ffull; v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull; v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

__global__ __launch_bounds__(256) void k_morton(uint32_t T, uint32_t bits, const float *__restrict__ tlo, const float *__restrict__ thi,
                                                const uint32_t *__restrict__ cbounds, uint64_t *__restrict__ keys, uint32_t *__restrict__ gids) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T) return;
    float cmin[3], cmax[3];
    for (int k = 0; k < 3; k++) { cmin[k] = ord2f(cbounds[k]); cmax[k] = ord2f(cbounds[3 + k]); }
    float cells = bits == 30 ? 1024.0f : 2097152.0f;
    float q[3];
    for (int k = 0; k < 3; k++) {
        float ext = cmax[k] - cmin[k];
        float sc = ext > 0.0f ? cells / ext : 0.0f;
        float c = (tlo[3 * (size_t)g + k] + thi[3 * (size_t)g + k]) * 0.5f;
        q[k] = fminf(fmaxf((c - cmin[k]) * sc, 0.0f), cells - 1.0f);
    }
    uint64_t key;
    if (bits == 30) key = ((uint64_t)expand10((uint32_t)q[0]) << 2) | ((uint64_t)expand10((uint32_t)q[1]) << 1) | (uint64_t)expand10((uint32_t)q[2]);
    else key = (expand21((uint64_t)q[0]) << 2) | (expand21((uint64_t)q[1]) << 1) | expand21((uint64_t)q[2]);
    keys[g] = key; gids[g] = g;
}

__device__ inline int delta_fn(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ gid, int T, int i, int j) {
    if (j < 0 || j >= T) return -1;
    uint64_t a = keys[i], b = keys[j];
    if (a != b) return __clzll((long long)(a ^ b));
    return 64 + __clz((int)(gid[i] ^ gid[j]));
}

// Karras 2012, one thread per internal node
__global__ __launch_bounds__(256) void k_karras(int T, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ gid, int32_t *__restrict__ child,
                                                int32_t *__restrict__ parent_int, int32_t *__restrict__ parent_leaf) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T - 1) return;
    if (i == 0) parent_int[0] = -1;
    int d = delta_fn(keys, gid, T, i, i + 1) - delta_fn(keys, gid, T, i, i - 1) >= 0 ? 1 : -1;
    int dmin = delta_fn(keys, gid, T, i, i - d);
    int lmax = 2;
    while (delta_fn(keys, gid, T, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (delta_fn(keys, gid, T, i, i + (l + t) * d) > dmin) l += t;
    int j = i + l * d;
    int dnode = delta_fn(keys, gid, T, i, j);
    int sp = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (delta_fn(keys, gid, T, i, i + (sp + t) * d) > dnode) sp += t;
    } while (t > 1);
    int gamma = i + sp * d + (d < 0 ? -1 : 0);
    int lo = min(i, j), hi = max(i, j);
    if (lo == gamma) { child[2 * i] = ~gamma; parent_leaf[gamma] = i; } else { child[2 * i] = gamma; parent_int[gamma] = i; }
    if (hi == gamma + 1) { child[2 * i + 1] = ~(gamma + 1); parent_leaf[gamma + 1] = i; } else { child[2 * i + 1] = gamma + 1; parent_int[gamma + 1] = i; }
}

// leaf boxes + leaf-ordered triangle records
__global__ __launch_bounds__(256) void k_leaves(uint32_t T, const uint32_t *__restrict__ leaf_gid, const float *__restrict__ triw, const float *__restrict__ tlo,
                                                const float *__restrict__ thi, const uint32_t *__restrict__ tri_prim, const uint32_t *__restrict__ first_tri,
                                                float *__restrict__ leaf_lo, float *__restrict__ leaf_hi, DevTri *__restrict__ tris,
                                                const DevPrim *__restrict__ prims, DevShadeTri *__restrict__ shade_tris) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= T) return;
    uint32_t g = leaf_gid[p];
    for (int k = 0; k < 3; k++) { leaf_lo[3 * (size_t)p + k] = tlo[3 * (size_t)g + k]; leaf_hi[3 * (size_t)p + k] = thi[3 * (size_t)g + k]; }
    const float *w = triw + (size_t)g * 9;
    uint32_t pr = tri_prim[g];
    tris[p] = make_dev_tri(w, w + 3, w + 6, __uint_as_float(g));
    shade_tris[p] = gather_shade_tri(prims[pr], pr, g - first_tri[pr]);
}

// gid -> leaf position: the inverse of the sort's permutation (Lbvh::gid_leaf).  A refit never moves a leaf, so the table lives as long as the tree
__global__ __launch_bounds__(256) void k_gid_leaf(uint32_t T, const uint32_t *__restrict__ leaf_gid, uint32_t *__restrict__ gid_leaf) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= T) return;
    uint32_t g = leaf_gid[p];
    if (g < T) gid_leaf[g] = p;
}

// bottom-up refit: the second thread to arrive at a node owns it (its sibling's box is complete and visible)
__global__ __launch_bounds__(256) void k_refit(uint32_t T, const int32_t *__restrict__ child, const int32_t *__restrict__ parent_int,
                                               const int32_t *__restrict__ parent_leaf, const float *__restrict__ leaf_lo, const float *__restrict__ leaf_hi,
                                               float *node_lo, float *node_hi, uint32_t *arrive) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= T) return;
    int n = parent_leaf[p];
    while (n >= 0) {
        __threadfence();                       // release: this thread's boxes below n are written back
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // keep the write-back ahead of the arrival (hipcc may drop the wait)
        if (atomicAdd(&arrive[n], 1u) == 0u) return;
        __threadfence();                       // acquire: see the sibling subtree's boxes
        float l[2][3], h[2][3];
        for (int c = 0; c < 2; c++) {
            const float *cl, *chh;
            child_box(child[2 * n + c], leaf_lo, leaf_hi, node_lo, node_hi, cl, chh);
            for (int k = 0; k < 3; k++) { l[c][k] = __builtin_nontemporal_load(cl + k); h[c][k] = __builtin_nontemporal_load(chh + k); }
        }
        // (a masked subtree -- a refit after art_scene_set_primitive_enabled -- is "nowhere" and leaves the union alone; a build never sees one)
        const bool n0 = box_nowhere(l[0][0]), n1 = box_nowhere(l[1][0]);
        for (int k = 0; k < 3; k++) {
            node_lo[3 * (size_t)n + k] = n0 ? l[1][k] : (n1 ? l[0][k] : fminf(l[0][k], l[1][k]));
            node_hi[3 * (size_t)n + k] = n0 ? h[1][k] : (n1 ? h[0][k] : fmaxf(h[0][k], h[1][k]));
        }
        n = parent_int[n];
    }
}

__global__ __launch_bounds__(256) void k_emit_nodes(uint32_t T, const int32_t *__restrict__ child, const float *__restrict__ node_lo, const float *__restrict__ node_hi,
                                                    const float *__restrict__ leaf_lo, const float *__restrict__ leaf_hi, DevNode *__restrict__ nodes) {
    uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (T == 1) { // single triangle: a root whose second child can never be hit
        if (n == 0) {
            DevNode d;
            d.q[0] = make_float4(leaf_lo[0], leaf_lo[1], leaf_lo[2], leaf_hi[0]);
            d.q[1] = make_float4(leaf_hi[1], leaf_hi[2], 3.0e38f, 3.0e38f); // a far-away point box: every slab test fails
            d.q[2] = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f);
            d.q[3] = make_float4(__int_as_float(~0), __int_as_float(~0), 0.f, 0.f);
            nodes[0] = d;
        }
        return;
    }
    if (n >= T - 1) return;
    int c0 = child[2 * n], c1 = child[2 * n + 1];
    const float *l0, *h0, *l1, *h1;
    child_box(c0, leaf_lo, leaf_hi, node_lo, node_hi, l0, h0); child_box(c1, leaf_lo, leaf_hi, node_lo, node_hi, l1, h1);
    DevNode d;
    d.q[0] = make_float4(l0[0], l0[1], l0[2], h0[0]);
    d.q[1] = make_float4(h0[1], h0[2], l1[0], l1[1]);
    d.q[2] = make_float4(l1[2], h1[0], h1[1], h1[2]);
    d.q[3] = make_float4(__int_as_float(c0), __int_as_float(c1), 0.f, 0.f);
    nodes[n] = d;
}
void launch_emit_nodes(Lbvh &l, uint32_t T, hipStream_t s) { // the 64-byte node records of the tree the walks use
    const WalkTree w = l.walk_tree();
    k_emit_nodes<<<((T > 1 ? T - 1 : 1) + 255) / 256, 256, 0, s>>>(T, w.child, w.lo, w.hi, l.leaf_lo, l.leaf_hi, l.nodes);
}

// the leaf bits of the alpha test (FrameArgs::alpha_bits): a thread per word of 32 leaf positions, set where the leaf's primitive has a cutoff > 0 or a visibility mask other than 0xFF in `prims`.  Bits are only ever
// added (atomicOr): a frame in flight that reads a word while it changes sees its own bits either way, and a bit of a primitive whose cutoff went back to 0 costs that
// frame a look at the cutoff, never a wrong answer.  The next build starts from zero.
__global__ __launch_bounds__(256) void k_alpha_bits(uint32_t T, const uint32_t *__restrict__ leaf_gid, const uint32_t *__restrict__ tri_prim, const DevPrim *prims, uint32_t *bits) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= (T + 31u) / 32u) return;
    uint32_t m = 0;
    for (uint32_t j = 0; j < 32u && w * 32u + j < T; j++) { const DevPrim &P = prims[tri_prim[leaf_gid[w * 32u + j]]]; if (P.cutoff > 0.0f || (P.masked >> kPrimVisShift) != 0u) m |= 1u << j; }
    if (m) atomicOr(&bits[w], m);
}
void launch_alpha_bits(uint32_t T, const uint32_t *leaf_gid, const uint32_t *tri_prim, const DevPrim *prims, uint32_t *bits, hipStream_t s) {
    const uint32_t nw = (T + 31u) / 32u;
    if (nw) k_alpha_bits<<<(nw + 255) / 256, 256, 0, s>>>(T, leaf_gid, tri_prim, prims, bits);
}

// The binary trees (the canonical LBVH of art_get_lbvh, the traversal tree of the per-ray / binary walks) after a refit: leaf boxes from the triangle records,
// node boxes bottom-up with the build's own kernel, the 64-byte node records again.  Only the non-default forms and the parity surface read them, so this runs
// on demand and under full synchronisation (art_api.hip).
__global__ __launch_bounds__(256) void k_leaf_boxes(uint32_t T, const DevTri *__restrict__ tris, float *__restrict__ leaf_lo, float *__restrict__ leaf_hi) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= T) return;
    for (int k = 0; k < 3; k++) { leaf_lo[3 * (size_t)p + k] = tris[p].f[9 + k]; leaf_hi[3 * (size_t)p + k] = tris[p].f[12 + k]; }
}
__global__ __launch_bounds__(256) void k_parents(uint32_t NI, const int32_t *__restrict__ child, int32_t *__restrict__ parent_int, int32_t *__restrict__ parent_leaf) {
    uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= NI) return;
    if (n == 0) parent_int[0] = -1;
    for (int c = 0; c < 2; c++) { int32_t ch = child[2 * (size_t)n + c]; if (ch < 0) parent_leaf[~ch] = (int32_t)n; else parent_int[ch] = (int32_t)n; }
}
hipError_t binary_refit(Lbvh &l, uint32_t T, const DevTri *tris, hipStream_t s) {
    const uint32_t NI = T > 1 ? T - 1 : 0, B = 256, GT = (T + B - 1) / B;
    k_leaf_boxes<<<GT, B, 0, s>>>(T, tris, l.leaf_lo, l.leaf_hi);
    DevBuf<int32_t> parent_int, parent_leaf; DevBuf<uint32_t> arrive;   // (freed on every way out, behind the synchronisation on the good one)
    if (NI) {
        HIPQ(parent_int.ensure(NI)); HIPQ(parent_leaf.ensure(T)); HIPQ(arrive.ensure(NI));
        for (int tree = 0; tree < 2; tree++) {
            const int32_t *child = tree == 0 ? l.child : l.trav_child;
            float *nlo = tree == 0 ? l.node_lo : l.trav_lo, *nhi = tree == 0 ? l.node_hi : l.trav_hi;
            if (!child) continue;
            HIPQ(hipMemsetAsync(arrive.p, 0, (size_t)NI * 4, s));
            k_parents<<<(NI + B - 1) / B, B, 0, s>>>(NI, child, parent_int.p, parent_leaf.p);
            k_refit<<<GT, B, 0, s>>>(T, child, parent_int.p, parent_leaf.p, l.leaf_lo, l.leaf_hi, nlo, nhi, arrive.p);
        }
    }
    launch_emit_nodes(l, T, s);
    HIPQ(hipGetLastError());
    HIPQ(hipStreamSynchronize(s));
    l.canon_boxes = true;
    return hipSuccess;
}

__global__ void k_build_noop() {}
void build_prewarm(hipStream_t s) { k_build_noop<<<1, 1, 0, s>>>(); wide_prewarm(s); refit_prewarm(s); }

hipError_t lbvh_claim_trav(Lbvh &l, uint32_t NI) {
    if (l.trav_child) return hipSuccess;
    if (l.res_trav_child) { l.trav_child = l.res_trav_child; l.trav_lo = l.res_trav_lo; l.trav_hi = l.res_trav_hi; return hipSuccess; }
    HIPQ(l.own_trav_child.ensure((size_t)NI * 2)); HIPQ(l.own_trav_lo.ensure((size_t)NI * 3)); HIPQ(l.own_trav_hi.ensure((size_t)NI * 3));
    l.trav_child = l.own_trav_child.p; l.trav_lo = l.own_trav_lo.p; l.trav_hi = l.own_trav_hi.p;   // (the views only once all three exist)
    return hipSuccess;
}

hipError_t lbvh_build(const BuildInputs &in, Lbvh &out, hipStream_t s, bool node_boxes) {
    const uint32_t T = in.T;
    const uint32_t NI = T > 1 ? T - 1 : 1;
    Arena *const ctx_arena = out.arena;
    out = Lbvh{};
    out.arena = ctx_arena;
    Arena own; Arena &A = ctx_arena ? *ctx_arena : own;
    float *triw = nullptr, *tlo = nullptr, *thi = nullptr;
    uint32_t *cslots = nullptr, *gid_in = nullptr, *arrive = nullptr;
    uint64_t *keys_in = nullptr;
    int32_t *parent_int = nullptr, *parent_leaf = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    auto body = [&]() -> hipError_t {
        // the temporaries: one reservation of the context's arena (the sort's own scratch included)
        HIPQ(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in, out.keys, gid_in, out.leaf_gid, T, 0, 64, s));
        HIPQ(A.reserve(Arena::pad((size_t)T * 36) + 2 * Arena::pad((size_t)T * 12) + Arena::pad(kCbSlots * 32 * 4) + Arena::pad((size_t)T * 4) + Arena::pad((size_t)T * 8) + 2 * Arena::pad((size_t)NI * 4) + Arena::pad((size_t)T * 4) + Arena::pad(tmp_bytes ? tmp_bytes : 16)));
        triw = A.take<float>((size_t)T * 9); tlo = A.take<float>((size_t)T * 3); thi = A.take<float>((size_t)T * 3);
        cslots = A.take<uint32_t>(kCbSlots * 32); gid_in = A.take<uint32_t>(T); keys_in = A.take<uint64_t>(T);
        arrive = A.take<uint32_t>(NI); parent_int = A.take<int32_t>(NI); parent_leaf = A.take<int32_t>(T);
        tmp = A.take<char>(tmp_bytes ? tmp_bytes : 16);
        {   // everything that outlives the build: one allocation (and room for the traversal tree some builder will make over these leaves)
            const size_t sizes[16] = {(size_t)T * 4, (size_t)T * 8, (size_t)NI * 8, (size_t)NI * 12, (size_t)NI * 12, (size_t)T * 12, (size_t)T * 12, (size_t)T * sizeof(DevTri), (size_t)NI * sizeof(DevNode),
                                      (size_t)T * 4, (size_t)T * sizeof(DevShadeTri), 32, (size_t)NI * 8, (size_t)NI * 12, (size_t)NI * 12, (size_t)T * 4};
            size_t total = 0; for (size_t b : sizes) total += Arena::pad(b);
            HIPQ(out.block.ensure(total));
            char *p = out.block.p; auto cut = [&](size_t bytes) { char *q = p; p += Arena::pad(bytes); return q; };
            out.leaf_gid = (uint32_t *)cut(sizes[0]); out.keys = (uint64_t *)cut(sizes[1]); out.child = (int32_t *)cut(sizes[2]); out.node_lo = (float *)cut(sizes[3]); out.node_hi = (float *)cut(sizes[4]);
            out.leaf_lo = (float *)cut(sizes[5]); out.leaf_hi = (float *)cut(sizes[6]); out.tris = (DevTri *)cut(sizes[7]); out.nodes = (DevNode *)cut(sizes[8]); out.tri_prim = (uint32_t *)cut(sizes[9]);
            out.shade_tris = (DevShadeTri *)cut(sizes[10]); out.cbounds = (uint32_t *)cut(sizes[11]);
            out.res_trav_child = (int32_t *)cut(sizes[12]); out.res_trav_lo = (float *)cut(sizes[13]); out.res_trav_hi = (float *)cut(sizes[14]);
            out.gid_leaf = (uint32_t *)cut(sizes[15]);
        }
        k_cb_init<<<1, kCbSlots, 0, s>>>(cslots);
        HIPQ(hipMemsetAsync(arrive, 0, (size_t)NI * 4, s));
        const uint32_t B = 256, GT = (T + B - 1) / B;
        k_soup<<<GT, B, 0, s>>>(in.prims, in.n_prims, in.prim_first_tri, T, triw, tlo, thi, out.tri_prim, cslots);
        k_cb_fold<<<1, kCbSlots, 0, s>>>(cslots, out.cbounds);
        k_morton<<<GT, B, 0, s>>>(T, in.morton_bits, tlo, thi, out.cbounds, keys_in, gid_in);
        HIPQ(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, out.keys, gid_in, out.leaf_gid, T, 0, 64, s));
        k_leaves<<<GT, B, 0, s>>>(T, out.leaf_gid, triw, tlo, thi, out.tri_prim, in.prim_first_tri, out.leaf_lo, out.leaf_hi, out.tris, in.prims, out.shade_tris);
        k_gid_leaf<<<GT, B, 0, s>>>(T, out.leaf_gid, out.gid_leaf);
        if (T > 1) {
            k_karras<<<(T - 1 + B - 1) / B, B, 0, s>>>((int)T, out.keys, out.leaf_gid, out.child, parent_int, parent_leaf);
            if (node_boxes) k_refit<<<GT, B, 0, s>>>(T, out.child, parent_int, parent_leaf, out.leaf_lo, out.leaf_hi, out.node_lo, out.node_hi, arrive); // (1.8 ms of arrival-counter waits on config 2: skipped when nothing will read the boxes)
        }
        if (node_boxes) launch_emit_nodes(out, T, s);   // (no traversal tree yet: the canonical one)
        out.canon_boxes = node_boxes;
        HIPQ(hipGetLastError());
        HIPQ(hipStreamSynchronize(s));
        return hipSuccess;
    };
    const hipError_t err = body();
    if (err != hipSuccess) out = Lbvh{};
    return err;
}

} // namespace art
