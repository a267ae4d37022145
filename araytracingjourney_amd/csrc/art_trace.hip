// art_trace.hip -- the staged per-ray frame (gfx950): primary rays + closest hit (k_trace), hit reconstruction + PBR direct light + shadow-ray emission (k_shade),
// shadow (any-hit) rays (k_trace), accumulation (k_accumulate); the ambient-occlusion launch on the same tracer (k_ao_pixels, k_trace_ao, k_ao_resolve).  Restates
// raytrace.rgen.glsl:77-200 of the reference's shaders/rt_lightning_shadows (+ light.glsl, brdfs.glsl: art_shade.h), split at its two traceRayEXT calls; the traversal
// (art_walk.h) replaces the driver/hardware behind traceRayEXT.  The fused frame, which runs the same arithmetic in one launch, is art_frame.hip.
#include "art_walk.h"
#include "art_shade.h"
#include <type_traits>

namespace art {

// ---- ray-traced ambient occlusion (BASELINE config 5): XeGTAO's I/O contract on the tracer ------------------------
// inputs: the frame's depth + view-space normal outputs (vk_xe_gtao.rs:295-333); noise: Hilbert index driving the R2
// sequence (main_pass.comp.hlsl:48-65, XeGTAO.h:120-142) with index + 288 * sample; cosine-weighted hemisphere.
__device__ __forceinline__ uint32_t hilbert_index(uint32_t x, uint32_t y) {
    uint32_t index = 0;
#pragma unroll
    for (uint32_t lvl = 32; lvl > 0; lvl /= 2) {
        uint32_t rx = (x & lvl) > 0, ry = (y & lvl) > 0;
        index += lvl * lvl * ((3u * rx) ^ ry);
        if (ry == 0) {
            if (rx == 1) { x = 63u - x; y = 63u - y; }
            uint32_t t = x; x = y; y = t;
        }
    }
    return index;
}
// cos/sin of u turns by quadrant reduction + Taylor polynomials in a fixed fmaf order (bit-reproducible, unlike sinf/cosf)
__device__ __forceinline__ void sincos_turns(float u, float &c, float &s) {
    float q = u * 4.0f;
    int k = (int)q;
    float x = (q - (float)k) * 1.57079632679489662f, x2 = x * x;
    float sp = fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, -2.50521083854417188e-8f, 2.75573192239858907e-6f), -1.98412698412698413e-4f), 8.33333333333333333e-3f), -1.66666666666666667e-1f), 1.0f) * x;
    float cp = fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, 2.08767569878680990e-9f, -2.75573192239858907e-7f), 2.48015873015873016e-5f), -1.38888888888888889e-3f), 4.16666666666666667e-2f), -0.5f), 1.0f);
    k &= 3;
    c = k == 0 ? cp : (k == 1 ? -sp : (k == 2 ? -cp : sp));
    s = k == 0 ? sp : (k == 1 ? cp : (k == 2 ? -sp : -cp));
}
// an AO ray in three parts, so that the tracer's refill pays only for what differs from ray to ray: the pixel's point and world normal (once per
// pixel: k_ao_pixels), the sample's direction in the tangent frame (a function of the pixel's position in its 64x64 noise tile and the sample
// index only: a table, k_ao_table), and the frame itself.  ao_ray() composes the three: the same operations in the same order wherever a ray is made.
__device__ __forceinline__ void ao_pixel(const CameraArg &cam, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float depth, float4 nm, V3 &o, V3 &N) {
    float px = (float)x + 0.5f, py = (float)y + 0.5f;
    float dx = (px / (float)W) * 2.0f - 1.0f, dy = (py / (float)H) * 2.0f - 1.0f;
    V3 org = mat4_mul(cam.view_inv, 0.f, 0.f, 0.f, 1.f);
    V3 tn = nrm3(mat4_mul(cam.proj_inv, dx, dy, 1.f, 1.f));
    V3 dir = mat4_mul(cam.view_inv, tn.x, tn.y, tn.z, 0.f);
    float sc = depth / -tn.z;
    o = mk(org.x + dir.x * sc, org.y + dir.y * sc, org.z + dir.z * sc); // the primary ray scaled to the stored view depth
    float nx = nm.x * 2.0f - 1.0f, ny = -(nm.y * 2.0f - 1.0f), nz = -(nm.z * 2.0f - 1.0f); // raytrace.rgen.glsl:192-194 inverted
    const float *VI = cam.view_inv;
    N = nrm3(mk((VI[0] * nx + VI[4] * ny) + VI[8] * nz, (VI[1] * nx + VI[5] * ny) + VI[9] * nz, (VI[2] * nx + VI[6] * ny) + VI[10] * nz));
}
// cosine-weighted direction of sample `smp` of the pixel whose Hilbert index in its 64x64 tile is `hil`, in the tangent frame: (r cos, r sin, sqrt(1 - u1))
__device__ __forceinline__ void ao_sample(uint32_t hil, uint32_t smp, float &tx, float &ty, float &tz) {
    float fi = (float)(hil + 288u * smp);
    float v1 = 0.5f + fi * 0.75487766624669276f, v2 = 0.5f + fi * 0.56984029099805327f;
    float u1 = v1 - floorf(v1), u2 = v2 - floorf(v2);
    float r = sqrtf(u1), cc, ss;
    tz = sqrtf(1.0f - u1);
    sincos_turns(u2, cc, ss);
    tx = r * cc; ty = r * ss;
}
__device__ __forceinline__ V3 ao_dir(V3 N, float tx, float ty, float tz) {
    float sg = copysignf(1.0f, N.z), aa = -1.0f / (sg + N.z), bb = N.x * N.y * aa; // branchless orthonormal basis (Duff et al. 2017)
    V3 T = mk(1.0f + sg * N.x * N.x * aa, sg * bb, -sg * N.x), B = mk(bb, sg + N.y * N.y * aa, -N.y);
    return (T * tx + B * ty) + N * tz;
}
__device__ __forceinline__ void ao_ray(const CameraArg &cam, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float depth, float4 nm, uint32_t smp, V3 &o, V3 &d) {
    V3 N; float tx, ty, tz;
    ao_pixel(cam, W, H, x, y, depth, nm, o, N);
    ao_sample(hilbert_index(x & 63u, y & 63u), smp, tx, ty, tz);
    d = ao_dir(N, tx, ty, tz);
}
constexpr uint32_t kAoNoiseTile = 64 * 64; // the sample table has one entry per (sample, Hilbert index in the 64x64 tile)
// tab[j * 4096 + hil] = the tangent-frame direction of the pixel's j-th sample IN AZIMUTH ORDER (the R2 sequence's second coordinate, ties by sample index): a
// pixel's occlusion count is a sum over its samples, so their order is free -- and with it the tracer can put the samples of one azimuth quadrant of
// neighbouring pixels (similar normals, similar frames) into one wave: rays that leave in similar directions make similar walks (ao_slot_decode below).
__global__ __launch_bounds__(kBlock) void k_ao_table(uint32_t spp, float4 *__restrict__ tab) {
    uint32_t hil = blockIdx.x * kBlock + threadIdx.x;
    if (hil >= kAoNoiseTile) return;
    float key[64]; uint8_t idx[64];
    for (uint32_t s = 0; s < spp; s++) {
        float fi = (float)(hil + 288u * s), v2 = 0.5f + fi * 0.56984029099805327f;   // ao_sample's u2
        float k = v2 - floorf(v2);
        uint32_t at = s;
        while (at > 0 && key[at - 1] > k) { key[at] = key[at - 1]; idx[at] = idx[at - 1]; at--; }   // insertion keeps equal keys in sample order
        key[at] = k; idx[at] = (uint8_t)s;
    }
    for (uint32_t j = 0; j < spp; j++) {
        float tx, ty, tz;
        ao_sample(hil, idx[j], tx, ty, tz);
        tab[(size_t)j * kAoNoiseTile + hil] = make_float4(tx, ty, tz, 0.f);
    }
}
// The AO launch's slots.  Sixteen pixels -- one 4x4 quadrant of an 8x8 block -- own ceil(spp / 4) * 64 consecutive slots laid out
// [group of four samples in azimuth order][pixel][sample of the group]: the 64 slots a wave takes at a time are sixteen neighbouring pixels x the four samples of
// one azimuth quadrant.  (Round 2's order, [pixel][sample], put a pixel's whole hemisphere into sixteen neighbouring lanes: 55 % of the lanes of a vector
// instruction were active; this order: 61 %, 7 % fewer instructions.)  Slots past spp (spp not a multiple of four) are padding: no ray, occlusion byte 0.
__device__ __forceinline__ uint32_t ao_slots_per16(uint32_t spp) { return ((spp + 3u) >> 2) * 64u; }
__device__ __forceinline__ bool ao_slot_decode(uint32_t slot, uint32_t spp, uint32_t &p, uint32_t &j) {
    const uint32_t per16 = ao_slots_per16(spp), b16 = slot / per16, r = slot - b16 * per16;
    const uint32_t pi = (r >> 2) & 15u, q = b16 & 3u;
    const uint32_t x = (pi & 3u) + ((q & 1u) << 2), y = (pi >> 2) + ((q >> 1) << 2);
    p = (b16 >> 2) * 64u + y * 8u + x;    // local pixel: an 8x8 block is 64 consecutive local pixels, lane = y * 8 + x
    j = (r >> 6) * 4u + (r & 3u);
    return j < spp;
}
__device__ __forceinline__ size_t ao_slot_of(uint32_t p, uint32_t j, uint32_t spp) {
    const uint32_t lane = p & 63u, x = lane & 7u, y = lane >> 3, q = (x >> 2) | ((y >> 2) << 1), pi = (x & 3u) | ((y & 3u) << 2);
    return (size_t)((p >> 6) * 4u + q) * ao_slots_per16(spp) + (j >> 2) * 64u + pi * 4u + (j & 3u);
}

// AO rays are short: the 16 rays of a pixel stay inside a ball of the AO radius around one point.  Descend the 4-wide tree while
// exactly ONE child box overlaps that ball's bounding box -- every other subtree cannot hold a triangle the rays could reach --
// and let the pixel's rays start there (or skip them when nothing overlaps).  Quantised boxes contain the float boxes, so the test
// errs on the side of overlap; the rays' answers are those of a walk from the root (accept() is per triangle).
constexpr int kAoNothingNear = (int)0x80000000; // no leaf has position 2^31 - 1
// per local pixel, once: pix[2p] = the AO rays' origin | the node they start from (or kAoNothingNear: a miss pixel, or nothing within the radius),
// pix[2p + 1] = the world normal | the pixel's Hilbert index in its noise tile.  wide == null: every pixel starts at the root (binary walk, or entry search off).
__global__ __launch_bounds__(kBlock) void k_ao_pixels(FrameArgs a, const DevNode4 *__restrict__ wide, float radius, float4 *__restrict__ pix) {
    uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n_local) return;
    uint32_t x, y;
    bool in = local_to_xy(p, a.tile_list, a.tiles_x, a.W, a.H, x, y);
    float depth = in ? a.depth[(size_t)y * a.W + x] : 10000.0f;
    if (!(depth < 10000.0f)) { pix[2 * (size_t)p] = make_float4(0.f, 0.f, 0.f, __int_as_float(kAoNothingNear)); pix[2 * (size_t)p + 1] = make_float4(0.f, 0.f, 1.f, 0.f); return; }
    V3 o, N;
    ao_pixel(a.cam, a.W, a.H, x, y, depth, a.normal[(size_t)y * a.W + x], o, N);
    int cur = 0;
    if (wide) {
        const float R = radius * 1.01f; // t runs to `radius` along a direction of length 1 +- rounding
        const float lox = o.x - R, loy = o.y - R, loz = o.z - R, hix = o.x + R, hiy = o.y + R, hiz = o.z + R;
        for (int level = 0; level < 64; level++) {
            const uint4 *nq = reinterpret_cast<const uint4 *>(wide + cur);
            uint4 qa = nq[0], qb = nq[1], qc = nq[2], qd = nq[3];
            float ox = __uint_as_float(qa.x), oy = __uint_as_float(qa.y), oz = __uint_as_float(qa.z);
            float sx = __uint_as_float((qa.w & 255u) << 23), sy = __uint_as_float(((qa.w >> 8) & 255u) << 23), sz = __uint_as_float(((qa.w >> 16) & 255u) << 23);
            uint32_t mask = qa.w >> 24;
            int refs[4] = {(int)qd.x, (int)qd.y, (int)qd.z, (int)qd.w};
            int n_over = 0, which = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float lx = fmaf((float)((qb.x >> (8 * i)) & 255u), sx, ox), ly = fmaf((float)((qb.y >> (8 * i)) & 255u), sy, oy), lz = fmaf((float)((qb.z >> (8 * i)) & 255u), sz, oz);
                float hx = fmaf((float)((qb.w >> (8 * i)) & 255u), sx, ox), hy = fmaf((float)((qc.x >> (8 * i)) & 255u), sy, oy), hz = fmaf((float)((qc.y >> (8 * i)) & 255u), sz, oz);
                bool over = ((mask >> i) & 1u) && lx <= hix && hx >= lox && ly <= hiy && hy >= loy && lz <= hiz && hz >= loz;
                if (over) { n_over++; which = refs[i]; }
            }
            if (n_over == 0) { cur = kAoNothingNear; break; }
            if (n_over > 1) break;          // the rays may go either way from here: this node is the entry
            cur = which;
            if (cur < 0) break;             // a single triangle is all there is
        }
    }
    pix[2 * (size_t)p] = make_float4(o.x, o.y, o.z, __int_as_float(cur));
    pix[2 * (size_t)p + 1] = make_float4(N.x, N.y, N.z, __uint_as_float(hilbert_index(x & 63u, y & 63u)));
}

// what a persistent tracing wave reads its rays from and writes its results to
enum { MODE_PRIMARY = 0, MODE_SHADOW = 1, MODE_AO = 4 };   // (2 and 3 were the queries': rays in device buffers have a tracer of their own, k_cast in art_query_rays.hip.  Not renumbered: tools and profiles name k_trace<4, ..>)
struct TraceArgs {
    const DevNode *nodes; const DevNode4 *wide; const DevTri *tris;
    uint32_t total;          // candidate slots
    uint32_t leaf_batch;     // lanes that must wait on a triangle before the wave runs the triangle test
    uint32_t chunk, refill;  // slots a wave takes from a cursor at a time; idle lanes that trigger a refill (Aila & Laine 2009, dynamic fetch)
    uint32_t *cursors;       // 8 per-XCD chunk cursors, kCursorStride words apart (zeroed before the launch)
    uint32_t *count;         // rays actually traced (MODE_SHADOW), may be null
    // MODE_PRIMARY
    CameraArg cam; uint32_t W, H; const uint32_t *tile_list; uint32_t tiles_x;
    float4 *hits;
    // MODE_SHADOW: rays[2*slot] = o.xyz,tmax(<=0: no ray) | rays[2*slot+1] = d.xyz,unused
    const float4 *rays;
    float4 *contrib; uint32_t n_local; uint32_t *shadow_bits;
    // MODE_AO: rays are generated from the frame's depth + view-space normal outputs (XeGTAO's inputs) by way of k_ao_pixels; slot -> (local pixel, sample): ao_slot_decode
    uint32_t spp; float ao_radius; uint8_t *occl;
    const float4 *ao_pix;     // MODE_AO: per local pixel, origin | start node and world normal | Hilbert index (k_ao_pixels)
    const float4 *ao_tab;     // MODE_AO: [sample][Hilbert index] tangent-frame direction (k_ao_table)
    AlphaView alpha;          // the instances with the alpha test only
};

#ifdef ART_TRACE_PROF
// profiling build only (make EXTRA=-DART_TRACE_PROF; tools/trace_prof.py): what the iterations of the persistent tracer's waves are made of, summed over the waves of every launch since
// the last reset: [0] loop iterations, [1] iterations with a node step, [2] lanes in them, [3] iterations with a triangle step, [4] lanes in them, [5] iterations with a refill, [6] lanes
// refilled (= rays), [7] lanes with a ray summed over all iterations
__device__ unsigned long long g_trace_prof[8];
#define TPROF(i, n) prof_[i] += (n)
#else
#define TPROF(i, n)
#endif
// Persistent-threads wavefront tracer.  Each wave keeps up to 64 rays in flight; when kRefill or more lanes have
// finished it compacts the idle lanes with __ballot / mbcnt and hands them the next candidates of its chunk; chunks
// come from eight per-XCD work cursors (one returning atomic per chunk), so neighbouring rays stay on one XCD's L2.
// Every wave exits once all cursors are exhausted and its lanes are idle.
template <int MODE, int WIDTH, bool ALPHA = false>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MODE == MODE_AO ? 8 : 4, 8))) void k_trace(TraceArgs a) {
    constexpr bool ANY = MODE == MODE_SHADOW || MODE == MODE_AO;
    __shared__ int stack[kLdsStack * kTraceBlock];
    int ovf[WIDTH == 4 ? kOvfStack4 : kOvfStack];
    const uint32_t leaf_batch = a.leaf_batch;
    int *lds = &stack[threadIdx.x];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (a.total + a.chunk - 1) / a.chunk; // <= 2^25, so n_chunks * 8 fits

    uint32_t shard = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u; // HW_REG_XCC_ID: speed only
    uint32_t shards_left = 8;
    uint32_t cur = 0, end = 0; // wave-uniform: the unread part of this wave's chunk
    bool exhausted = false, active = false;
    typename std::conditional<WIDTH == 4, Trav4<ANY, kLdsStack, ALPHA>, Trav<ANY, ALPHA>>::type tr;
    uint32_t slot = 0, traced = 0;
#ifdef ART_TRACE_PROF
    unsigned long long prof_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    for (;;) {
        uint64_t idle = __ballot(!active);
        TPROF(0, 1); TPROF(7, 64 - __popcll(idle));
        uint32_t n_idle = (uint32_t)__popcll(idle);
        if (!exhausted && n_idle >= a.refill) {
            if (cur == end) {
                const uint32_t got = pop_chunk(a.cursors, n_chunks, lane, shard, shards_left);
                if (got >= n_chunks) exhausted = true; // (also the never-expected out-of-range pop: no slot beyond total is touched)
                else { cur = got * a.chunk; end = min(cur + a.chunk, a.total); }
            }
            if (!exhausted) {
                uint32_t avail = end - cur;
                uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (!active && rank < avail) {
                    uint32_t sidx = cur + rank;
                    if (MODE == MODE_PRIMARY) {
                        uint32_t x, y;
                        if (local_to_xy(sidx, a.tile_list, a.tiles_x, a.W, a.H, x, y)) { // raytrace.rgen.glsl:78-88
                            float px = (float)x + 0.5f, py = (float)y + 0.5f;
                            float ux = px / (float)a.W, uy = py / (float)a.H;
                            float dx = ux * 2.0f - 1.0f, dy = uy * 2.0f - 1.0f;
                            V3 org = mat4_mul(a.cam.view_inv, 0.f, 0.f, 0.f, 1.f);
                            V3 tgt = nrm3<false>(mat4_mul(a.cam.proj_inv, dx, dy, 1.f, 1.f));   // (plain: with the guard the filtered binary-node instance takes a 72nd register)
                            V3 dir = mat4_mul(a.cam.view_inv, tgt.x, tgt.y, tgt.z, 0.f);
                            tr.start(org, dir, 0.001f, 10000.0f);
                            active = true;
                        } else a.hits[sidx] = make_float4(10000.0f, 0.f, 0.f, __uint_as_float(kNoHit));
                    } else if (MODE == MODE_AO) {
                        // everything but the direction was made once per pixel (k_ao_pixels), the direction's tangent-frame part once per context (k_ao_table):
                        // a refill is three 16-byte loads, a frame from the normal and ray_init -- cheap enough to refill at few idle lanes
                        uint32_t p, smp;                               // smp: the sample's rank in the pixel's azimuth order (k_ao_table)
                        const bool real = ao_slot_decode(sidx, a.spp, p, smp);
                        float4 po = real ? a.ao_pix[2 * (size_t)p] : make_float4(0.f, 0.f, 0.f, __int_as_float(kAoNothingNear));
                        float4 pn = real ? a.ao_pix[2 * (size_t)p + 1] : make_float4(0.f, 0.f, 1.f, 0.f);   // both halves of the pixel record in one round trip (the table entry needs the second)
                        asm volatile("" : "+v"(pn.x), "+v"(pn.y), "+v"(pn.z), "+v"(pn.w));
                        int entry = __float_as_int(po.w);
                        if (entry == kAoNothingNear) a.occl[sidx] = 0; // a padding slot, a miss pixel, or no box within the AO radius: unoccluded, nothing to trace
                        else {
                            float4 t = a.ao_tab[smp * kAoNoiseTile + __float_as_uint(pn.w)];
                            tr.start(mk(po.x, po.y, po.z), ao_dir(mk(pn.x, pn.y, pn.z), t.x, t.y, t.z), a.ao_radius * 0.01f, a.ao_radius);
                            tr.cur = entry;                            // the walk starts below the part of the tree that every ray of this pixel would cross alike
                            active = true;
                        }
                    } else {
                        float4 r0 = a.rays[2 * (size_t)sidx];
                        if (r0.w > 0.0f) {
                            float4 r1 = a.rays[2 * (size_t)sidx + 1];
                            tr.start(mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), 0.01f, r0.w);   // shadow rays: tmin 0.01 (raytrace.rgen.glsl:174)
                            active = true;
                        }
                    }
                    if (active) { slot = sidx; traced++; }
                }
                TPROF(5, 1); TPROF(6, __popcll(__ballot(active) & idle));
                cur += min(n_idle, avail);
            }
            if (__ballot(active) == 0ull) continue; // nothing to trace yet: fetch again (or find the cursors exhausted)
        } else if (n_idle == 64u) {
            if (exhausted) break;
            continue;
        }
        // up to ART_NODE_REPS internal steps for every lane standing on a node ...  (this block and pooled_trace's are the same steps in two texts: one helper for both gave
        // k_trace<0, 4, true> a 78th register, and the pooled loop alone lost 0.2 to 1.3 % of its rate through it -- profiles/README.md, "one pooled loop")
        bool done = false;
        { uint64_t nm_ = __ballot(active && tr.cur >= 0); if (nm_) { TPROF(1, 1); TPROF(2, __popcll(nm_)); } }
#pragma unroll
        for (int rep_ = 0; rep_ < ART_NODE_REPS; rep_++)
        if (active && !done && tr.cur >= 0) {
            if constexpr (WIDTH == 4) done = tr.step_internal(a.wide, lds, ovf);
            else done = tr.step_internal(a.nodes, lds, ovf);
        }
        // ... and the triangle tests only once enough lanes wait on one (or nobody can move without it)
        bool on_leaf = active && !done && tr.cur < 0;
        uint64_t lm = __ballot(on_leaf);
        if (lm != 0ull && ((uint32_t)__popcll(lm) >= leaf_batch || __ballot(active && !done && tr.cur >= 0) == 0ull)) {
            TPROF(3, 1); TPROF(4, __popcll(lm));
            if (on_leaf) done = tr.step_leaf(a.tris, lds, ovf, a.alpha);
        }
        if (done) {
            active = false;
            if (MODE == MODE_PRIMARY)
                a.hits[slot] = tr.bpos != kNoHit ? make_float4(tr.tbest, tr.bu, tr.bv, __uint_as_float(tr.bpos)) : make_float4(10000.0f, 0.f, 0.f, __uint_as_float(kNoHit));
            else if (MODE == MODE_AO) a.occl[slot] = tr.bpos != kNoHit ? 1 : 0;
            else if (tr.bpos != kNoHit) { // shadowed: the light keeps 0.05 of its contribution (raytrace.rgen.glsl:179-181)
                float4 c = a.contrib[slot];
                a.contrib[slot] = make_float4(c.x * 0.05f, c.y * 0.05f, c.z * 0.05f, c.w);
                if (a.shadow_bits) { uint32_t i = slot / a.n_local; if (i < 16) atomicOr(&a.shadow_bits[slot - i * a.n_local], 1u << i); }
            }
        }
    }
#ifdef ART_TRACE_PROF
    if (lane == 0) for (int i = 0; i < 8; i++) atomicAdd(&g_trace_prof[i], prof_[i]);
#endif
    if (MODE == MODE_SHADOW && a.count) { // rays this wave traced: one atomic per wave
        for (int off = 32; off >= 1; off >>= 1) traced += (uint32_t)__shfl_xor((int)traced, off);
        if (lane == 0 && traced) atomicAdd(a.count + (blockIdx.x % kSlotCount) * kSlotStride, traced);   // one wave per workgroup
    }
}

// The AO launch's rays are MADE: the pixel's point, entry node and normal (k_ao_pixels), the sample's tangent-frame direction (k_ao_table) and a frame from the normal.
// Same slots, same rays, same walks as k_trace<MODE_AO, 4> (Trav4, any hit): the occlusion bytes cannot differ.
constexpr int kAoLds = 8;           // per-lane stack entries in LDS (AO rays start deep in the tree and are short: the walk rarely holds more; the rest spills)
struct AoSource {
    static constexpr int kFields = 11;   // o.xyz d.xyz inv.xyz entry slot
    const TraceArgs &a;
    template <class TRAV> __device__ __forceinline__ void init(TRAV &tr) const { tr.r.tmin = a.ao_radius * 0.01f; tr.r.tmax = a.ao_radius; }   // the same for every ray
    __device__ __forceinline__ bool fetch(uint32_t sidx, V3 &o, V3 &d, float &e0, float &) const {
        uint32_t p, smp;
        const bool real = ao_slot_decode(sidx, a.spp, p, smp);
        float4 po = real ? a.ao_pix[2 * (size_t)p] : make_float4(0.f, 0.f, 0.f, __int_as_float(kAoNothingNear));
        float4 pn = real ? a.ao_pix[2 * (size_t)p + 1] : make_float4(0.f, 0.f, 1.f, 0.f);
        asm volatile("" : "+v"(pn.x), "+v"(pn.y), "+v"(pn.z), "+v"(pn.w));
        bool has = false;
        e0 = po.w;   // the entry node
        if (__float_as_int(po.w) != kAoNothingNear) {
            float4 t = a.ao_tab[smp * kAoNoiseTile + __float_as_uint(pn.w)];
            o = mk(po.x, po.y, po.z); d = ao_dir(mk(pn.x, pn.y, pn.z), t.x, t.y, t.z);
            has = ray_finite(o, d);   // (a non-finite ray accepts nothing: unoccluded, like tr.start's dead ray)
        }
        if (!has) a.occl[sidx] = 0;    // a padding slot, a miss pixel, no box within the AO radius, a dead ray: nothing to trace
        return has;
    }
    template <class TRAV> __device__ __forceinline__ void begin(TRAV &tr, float e0, float) const { tr.cur = __float_as_int(e0); }   // the walk starts below the part of the tree that every ray of this pixel would cross alike
    template <class TRAV> __device__ __forceinline__ void finish(const TRAV &tr, uint32_t slot) const { a.occl[slot] = tr.bpos != kNoHit ? 1 : 0; }
};
template <bool ALPHA = false>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_trace_ao(TraceArgs a) { pooled_trace<kAoLds, true, ALPHA>(a, AoSource{a}); }

// staged frame, stage 2: emits one shadow ray per (pixel, light) that needs it
__global__ __launch_bounds__(kBlock) void k_shade(FrameArgs a) {
    if (blockIdx.x * kBlock >= a.n_local) return;
    uint32_t p = a.block_order[blockIdx.x] * kBlock + threadIdx.x;
    uint32_t x, y;
    bool in = local_to_xy(p, a.tile_list, a.tiles_x, a.W, a.H, x, y);
    size_t pix = (size_t)y * a.W + x;
    float4 h = ld_nt(&a.hits[p]);
    uint32_t pos = in ? __float_as_uint(h.w) : kNoHit;
    float out_depth = 10000.0f;
    V3 out_normal = mk(0.5f, 0.5f, 0.5f);
    uint32_t sbits = 0;
    if (pos == kNoHit) {
        for (uint32_t i = 0; i < a.n_lights; i++) {
            size_t slot = (size_t)i * a.n_local + p;
            st_nt(&a.contrib[slot], make_float4(0.f, 0.f, 0.f, 0.f));
            st_nt(&a.shadow_rays[2 * slot], make_float4(0.f, 0.f, 0.f, -1.0f)); // no shadow ray in this slot
        }
    } else {
        Surface S;
        shade_surface<true>(a, a.cam, pos, h.y, h.z, S, out_depth, out_normal);
        for (uint32_t i = 0; i < a.n_lights; i++) {
            float4 c4, ro, rd;
            const ArtLight L = frame_light(a, i);
            bool want = shade_light<true>(L, S, a.plain_math, c4, ro, rd);
            size_t slot = (size_t)i * a.n_local + p;
            st_nt(&a.contrib[slot], c4);
            if (want) {
                st_nt(&a.shadow_rays[2 * slot], ro);
                st_nt(&a.shadow_rays[2 * slot + 1], rd);
                if (i < 16) sbits |= 1u << (16 + i);
            } else st_nt(&a.shadow_rays[2 * slot], make_float4(0.f, 0.f, 0.f, -1.0f));
        }
    }
    if (in) {
        st_nt(&a.depth[pix], out_depth);
        st_nt(&a.normal[pix], make_float4(out_normal.x, out_normal.y, out_normal.z, 1.0f));
    }
    if (a.shadow_bits) a.shadow_bits[p] = sbits;
    uint64_t hitmask = __ballot(pos != kNoHit); // hit-pixel count: one atomic per wave, off the critical path
    if ((threadIdx.x & 63u) == 0 && hitmask) atomicAdd(&a.counters[kHitSlots + ((blockIdx.x * 4u + (threadIdx.x >> 6)) % kSlotCount) * kSlotStride], (uint32_t)__popcll(hitmask));
}

// art_get_stats for fused frames: shadow rays = set bits 16..31 of pix_bits, hit pixels = depth < miss depth; on demand only
__global__ __launch_bounds__(kBlock) void k_frame_stats(FrameArgs a, uint32_t *out) {
    uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    uint32_t rays = 0, hits = 0;
    if (p < a.n_local) {
        uint32_t x, y;
        bool in = local_to_xy(p, a.tile_list, a.tiles_x, a.W, a.H, x, y);
        rays = (uint32_t)__popc(a.pix_bits[p] >> 16) + (a.pix_more ? a.pix_more[p] : 0u);
        hits = in && a.depth[(size_t)y * a.W + x] < 10000.0f ? 1u : 0u;
    }
    for (int off = 32; off >= 1; off >>= 1) { rays += (uint32_t)__shfl_xor((int)rays, off); hits += (uint32_t)__shfl_xor((int)hits, off); }
    if ((threadIdx.x & 63u) == 0) { if (rays) atomicAdd(&out[0], rays); if (hits) atomicAdd(&out[1], hits); }
}

// rho += (rho_s + rho_d) * radiance * shadow_attenuation * NdotL (raytrace.rgen.glsl:185), lights in order
__global__ __launch_bounds__(kBlock) void k_accumulate(FrameArgs a) {
    if (blockIdx.x * kBlock >= a.n_local) return;
    uint32_t p = a.block_order[blockIdx.x] * kBlock + threadIdx.x;
    uint32_t x, y;
    bool in = local_to_xy(p, a.tile_list, a.tiles_x, a.W, a.H, x, y);
    float rx = 0.f, ry = 0.f, rz = 0.f;
    if (in)
        for (uint32_t i = 0; i < a.n_lights; i++) {
            float4 c = ld_nt(&a.contrib[(size_t)i * a.n_local + p]);
            rx += c.x * c.w; ry += c.y * c.w; rz += c.z * c.w;
        }
    float4 o = make_float4(rx, ry, rz, 1.0f);
    if (in) st_nt(&a.color[(size_t)y * a.W + x], o);
    if (a.color_tiles) { // compact tile buffer for the gather: row-major inside each 32x32 tile
        uint32_t q = p & 1023u, sub = q >> 6, l = q & 63u;
        uint32_t lx = (sub & 3u) * 8u + (l & 7u), ly = (sub >> 2) * 8u + (l >> 3);
        size_t ti = (size_t)(p >> 10) * kTilePixels + ly * kTile + lx;
        if (a.tiles_packed) __builtin_nontemporal_store(pack_b10g11r11(o.x, o.y, o.z), reinterpret_cast<uint32_t *>(a.color_tiles) + ti);
        else st_nt_rgb(a.color_tiles, ti, o);
    }
}

// ------------------------------------------------------------------------------------------------ launchers
// alpha: the instances with the alpha test (a.alpha set up by the caller)
template <int MODE> static void launch_trace(TraceArgs &a, int kind, bool pipelined, const TraceTune &o, bool alpha, hipStream_t s) {
    const Tune t = tune(pipelined, MODE == MODE_AO, o);
    uint32_t nb = persistent_blocks(a.total, t);
    a.chunk = t.chunk; a.refill = t.refill; a.leaf_batch = t.leaf_batch;
    if (alpha) { if (kind == 4) k_trace<MODE, 4, true><<<nb, kTraceBlock, 0, s>>>(a); else k_trace<MODE, 2, true><<<nb, kTraceBlock, 0, s>>>(a); }
    else if (kind == 4) k_trace<MODE, 4><<<nb, kTraceBlock, 0, s>>>(a);
    else k_trace<MODE, 2><<<nb, kTraceBlock, 0, s>>>(a);
}
// which: 0 primary | 1 shadow | 2 AO rays (their cull mask out of FrameArgs::ray_masks)
static AlphaView alpha_view(const FrameArgs &f, int which) { return AlphaView{f.alpha_bits, f.shade_tris, f.prims, f.tex_pool, (f.ray_masks >> (8 * which)) & 0xFFu}; }
void launch_primary(const FrameArgs &f, hipStream_t s) {   // staged frames: the persistent per-ray tracer
    TraceArgs a{};
    a.nodes = f.nodes; a.wide = f.wide; a.tris = f.tris; a.total = f.n_local; a.cursors = f.counters + 64; a.cam = f.cam; a.W = f.W; a.H = f.H;
    a.tile_list = f.tile_list; a.tiles_x = f.tiles_x; a.hits = f.hits;
    a.alpha = alpha_view(f, 0);
    launch_trace<MODE_PRIMARY>(a, f.trace_kind[0], f.pipelined, f.tune, f.alpha, s);
}
void launch_shade(const FrameArgs &a, hipStream_t s) { k_shade<<<blocks_for(a.n_local), kBlock, 0, s>>>(a); }
void launch_shadow(const FrameArgs &f, hipStream_t s) {
    if (f.n_lights == 0) return;
    TraceArgs a{};
    a.nodes = f.nodes; a.wide = f.wide; a.tris = f.tris; a.total = f.n_local * f.n_lights; a.cursors = f.counters + 64 + 8 * kCursorStride; a.count = f.counters + kShadowSlots;
    a.rays = f.shadow_rays; a.contrib = f.contrib; a.n_local = f.n_local; a.shadow_bits = f.shadow_bits;
    a.alpha = alpha_view(f, 1);
    launch_trace<MODE_SHADOW>(a, f.trace_kind[1], f.pipelined, f.tune, f.alpha, s);
}
void launch_frame_stats(const FrameArgs &a, uint32_t *out, hipStream_t s) { k_frame_stats<<<blocks_for(a.n_local), kBlock, 0, s>>>(a, out); }
void launch_accumulate(const FrameArgs &a, hipStream_t s) { k_accumulate<<<blocks_for(a.n_local), kBlock, 0, s>>>(a); }
// AO resolve: occluded count -> uint(pow(visibility, 2.2) * 255 + 0.5) through a host-built table; 255 where nothing was hit
struct AoLut { uint32_t v[65]; };
__global__ __launch_bounds__(kBlock) void k_ao_resolve(FrameArgs a, const uint8_t *__restrict__ occl, uint32_t spp, AoLut lut, uint32_t *__restrict__ ao) { // occl: one byte per slot (ao_slot_of)
    uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n_local) return;
    uint32_t x, y;
    if (!local_to_xy(p, a.tile_list, a.tiles_x, a.W, a.H, x, y)) return;
    size_t pix = (size_t)y * a.W + x;
    uint32_t k = 0;
    for (uint32_t s = 0; s < spp; s++) k += occl[ao_slot_of(p, s, spp)];
    ao[pix] = a.depth[pix] < 10000.0f ? lut.v[k] : 255u;
}
void launch_ao_table(uint32_t spp, float4 *tab, hipStream_t s) { k_ao_table<<<blocks_for(kAoNoiseTile), kBlock, 0, s>>>(spp, tab); }
void launch_ao(const FrameArgs &f, uint32_t spp, float radius, uint8_t *occl, float4 *pix, const float4 *tab, bool entry_search, uint32_t *ao, const uint32_t *lut, hipStream_t s) {
    AoLut l; for (uint32_t k = 0; k < 65; k++) l.v[k] = lut[k];
    k_ao_pixels<<<blocks_for(f.n_local), kBlock, 0, s>>>(f, ((f.trace_kind[2] == 4 || f.trace_kind[2] == 6) && entry_search) ? f.wide : nullptr, radius, pix); // one point, normal and entry node per pixel for its spp rays
    const uint32_t n_slots = (f.n_local / 16u) * (((spp + 3u) >> 2) * 64u); // ao_slot_decode
    TraceArgs a{};
    a.nodes = f.nodes; a.wide = f.wide; a.tris = f.tris; a.total = n_slots; a.cursors = f.counters + 64 + 16 * kCursorStride; a.spp = spp; a.ao_radius = radius; a.occl = occl;
    a.ao_pix = pix; a.ao_tab = tab; a.alpha = alpha_view(f, 2);
    if (f.trace_kind[2] == 4) {   // the default: the AO launch's own tracer (rays made by the whole wave into a pool); 6 = the same walk through the generic tracer (round 3's form), 2 = binary nodes
        Tune t = tune(f.pipelined, true, f.tune);
        if (!(f.tune.refill >= 1 && f.tune.refill <= 64)) t.refill = kPoolTake;
        a.chunk = t.chunk; a.refill = t.refill; a.leaf_batch = t.leaf_batch;
        if (f.alpha) k_trace_ao<true><<<persistent_blocks(a.total, t), kTraceBlock, 0, s>>>(a);
        else k_trace_ao<<<persistent_blocks(a.total, t), kTraceBlock, 0, s>>>(a);
    } else launch_trace<MODE_AO>(a, f.trace_kind[2] == 6 ? 4 : f.trace_kind[2], f.pipelined, f.tune, f.alpha, s);
    k_ao_resolve<<<blocks_for(f.n_local), kBlock, 0, s>>>(f, occl, spp, l, ao);
}
#ifdef ART_TRACE_PROF
extern "C" int32_t art_debug_trace_prof(unsigned long long *out, int32_t reset) { // out[8]
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace_prof), sizeof(g_trace_prof)) != hipSuccess) return -1;
    void *dp = nullptr;
    if (reset && (hipGetSymbolAddress(&dp, HIP_SYMBOL(g_trace_prof)) != hipSuccess || hipMemset(dp, 0, sizeof(g_trace_prof)) != hipSuccess)) return -1;
    return 0;
}
#endif

} // namespace art
