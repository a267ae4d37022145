// art_frame.hip -- the fused frame (gfx950): the packet walks (packet_walk, walk_dispatch), the 32 instances of k_frame that take an 8x8 pixel block through the whole of
// raytrace.rgen.glsl in one launch, and the wave plan made on the device behind a sampled frame (k_plan; its host side is art_plan.hip).  The shading is art_shade.h's,
// the staged frame's (art_trace.hip) to the bit.  The register figures of the k_frame instances are pinned (tests/test_alpha.py, tests/test_ray_masks.py; tools/kres.sh).
#include "art_shade.h"
#include <type_traits>

namespace art {

// ---- packet traversal for primary rays -------------------------------------------------------------------------------
// The 64 rays of a wave are the pixels of one 8x8 block: almost the same path through the tree.  The wave walks ONE shared
// path (the union of its rays' paths): the node index is wave-uniform, so the node and triangle records come through the
// scalar cache instead of a 64-lane gather, there is no per-lane stack and no divergence outside the triangle test; each lane
// still tests its own ray against both child boxes with its own t_best.  A lane that would accept a triangle passes the slab
// test of every enclosing box (monotone slab), so the packet finds exactly the per-ray answer, bit for bit.
constexpr int kPacketStack = 288; // shared stack of node references per wave: >= 3 pending siblings per level * 95 levels // a shared stack of node references per wave; the radix tree is at most 95 levels deep

// ballot64 (art_device.h) is a v_cmp straight into an SGPR pair only of a bare compare, though: the ballot of any other predicate -- a conjunction, a value that met another at the end of a branch -- is re-made on the vector unit
// (v_cndmask 0, 1 and v_cmp_ne).  The packet walks therefore keep what they know about lanes as MASKS -- one ballot per compare, combined on the scalar unit -- and change
// the per-lane ray state with selects that take a mask and write the register they read: x = lane in m ? y : x.  (Written as C++ selects, the closest-hit state had two
// definitions per loop trip and five register copies behind every triangle step.)  m is always the result of a scalar operation, never a v_cmp's own destination.
__device__ __forceinline__ void sel(float &x, float y, uint64_t m) { asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(x) : "v"(y), "s"(m)); }
__device__ __forceinline__ void sel(uint32_t &x, uint32_t y, uint64_t m) { asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(x) : "v"(y), "s"(m)); }
__device__ __forceinline__ void sel_off(float &x, uint64_t m) { asm("v_cndmask_b32_e64 %0, %0, -1.0, %1" : "+v"(x) : "s"(m)); }   // x = lane in m ? -1 : x

// The walk of one packet: `cur` (node reference) and the stack are wave-uniform.  OCT 0..7: every ray of the packet has the
// direction signs (x: bit 0, y: bit 1, z: bit 2; set = negative) -- the entry plane of each axis is then known at compile time
// (fma is monotone in the plane coordinate, so min(t0, t1) IS the chosen one, bit for bit) and a box costs 6 fma + 4 min/max
// instead of 6 + 10.  OCT 8: mixed signs, the general slab.
template <int OCT> __device__ __forceinline__ bool slab_oct(const Ray &r, float lx, float ly, float lz, float hx, float hy, float hz, float tlimit, float &tn) {
    if (OCT >= 8) return slab(r, lx, ly, lz, hx, hy, hz, tlimit, tn);
    float nx = fmaf((OCT & 1) ? hx : lx, r.inv.x, -r.ood.x), fx = fmaf((OCT & 1) ? lx : hx, r.inv.x, -r.ood.x);
    float ny = fmaf((OCT & 2) ? hy : ly, r.inv.y, -r.ood.y), fy = fmaf((OCT & 2) ? ly : hy, r.inv.y, -r.ood.y);
    float nz = fmaf((OCT & 4) ? hz : lz, r.inv.z, -r.ood.z), fz = fmaf((OCT & 4) ? lz : hz, r.inv.z, -r.ood.z);
    tn = fmaxf(fmaxf(nx, ny), nz);
    float tf = fminf(fminf(fx, fy), fz);
    return fmaxf(tn, r.tmin) <= fminf(tf, tlimit);
}

// The packet walks read the tree through the CONSTANT address space: nothing writes nodes or triangles while a frame kernel runs, and only of
// constant-space loads does the compiler believe that after the frame's own stores (hits, depth, normal) -- a wave-uniform global load behind a store
// becomes a vector load of 64 equal addresses, which is what the shadow walks of k_frame were until round 2 (node data in 16 VGPRs, the vector L1's latency).
struct ConstQuads {
    typedef float Quad __attribute__((ext_vector_type(4)));
    __attribute__((address_space(4))) const Quad *p;
    __device__ __forceinline__ float4 operator[](int i) const { Quad v = p[i]; return make_float4(v.x, v.y, v.z, v.w); }
};
template <class T> __device__ __forceinline__ ConstQuads const_quads(const T *p) { ConstQuads q; q.p = (__attribute__((address_space(4))) const ConstQuads::Quad *)(uintptr_t)p; return q; }

// (Rounds 3 and 4 measured two uses of the packet's BEAM -- interval bounds of its rays against a node's four boxes on half a wave, 9 vector instructions -- and kept neither:
// as the node step itself its weaker culling bought 38 % more triangle steps (round 3b), as a FILTER in front of the per-ray box tests it left the launch's vector instructions
// where they were -- 124.98 M -> 124.86 M: what the filtered-out box tests save goes into the beam's set-up, its 9 instructions a step and the boxes it passes needlessly --
// and added 36 % scalar instructions and 13 % wave cycles: config 2 19 370 -> 17 250 Mray/s, frames bit-equal.  profiles/README.md round 4, profiles/round4_filter_*.)
#ifdef ART_PACKET_PROF
// profiling build only (make EXTRA=-DART_PACKET_PROF; tools/packet_prof.py): what the packet walks of k_frame are made of, summed over all waves since the last reset.
// [0..11] closest-hit (primary) walks, [12..23] any-hit (shadow) walks: walks, node steps, triangle steps, triangle steps that came off the stack, triangle steps in
// which some lane accepted the triangle, lanes that accepted, child boxes hit by some lane (of 4 per node step), mixed-octant walks
__device__ unsigned long long g_packet_prof[24];   // + [8] shader-clock cycles in node steps, [9] in triangle steps (each with the pop behind it), [10] triangle steps that were hints, [11] walks that ended inside their hint steps
#define PPROF(i, n) do { if ((threadIdx.x & 63u) == 0) atomicAdd(&g_packet_prof[(ANY ? 12 : 0) + (i)], (unsigned long long)(n)); } while (0)
#else
#define PPROF(i, n)
#endif
// Shadow-occluder hints of one any-hit walk (FrameArgs::hints), wave-uniform.  In: where the walk starts -- cur / sp as hints_seed left them: the block's valid
// hints are visited as ordinary triangle steps BEFORE the root, which waits below them on the stack (no hints: cur 0, sp 0, the walk as it always was).  Lanes a hint occludes
// are off for the rest of the walk; if all are, the walk ends in its triangle step like any other.  Out: n, how many triangle steps of this walk accepted a ray; the leaf
// position of accepting step j is in stk[kPacketStack + j % 4] (four words behind the stack: a ring, so the four most recent survive).  A leaf accepts in at most one step of
// a walk -- what it would accept it accepts the first time it is visited -- so the ring holds no position twice.
struct PacketHints { int cur, sp; uint32_t n; };
// The stack of the next any-hit walk, seeded from a hint entry (any four words): a word is visited only if it is a leaf position of this tree (< n_leaves); what it holds is
// then tested against this frame's triangles like any leaf the walk reaches, so a stale or a made-up word costs a step and changes nothing.  w0 is visited first.
// (Called in front of the shadow ray's set-up: the two registers of lane 0's stack writes are not to be had once the ray is live -- seeded inside the walk, the multi-light
// instances spilled up to seven registers more.)
__device__ __forceinline__ PacketHints hints_seed(int *stk, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t n_leaves) {
    PacketHints h{0, 0, 0u};
    if ((w0 & w1 & w2 & w3) == kHintEmpty) return h;   // (a fully lit block's entry: nothing but this compare)
    const bool lane0 = (threadIdx.x & 63u) == 0;
    if (w3 < n_leaves) { if (lane0) stk[h.sp] = h.cur; h.sp++; h.cur = (int)~w3; }
    if (w2 < n_leaves) { if (lane0) stk[h.sp] = h.cur; h.sp++; h.cur = (int)~w2; }
    if (w1 < n_leaves) { if (lane0) stk[h.sp] = h.cur; h.sp++; h.cur = (int)~w1; }
    if (w0 < n_leaves) { if (lane0) stk[h.sp] = h.cur; h.sp++; h.cur = (int)~w0; }
    return h;
}
// ON: what the walk knows its live lanes by -- uint64_t, their mask (the form described at sel()), or bool, a predicate per lane and C++ selects: the form every instance had
// before, kept for the instances whose register allocation the mask form moves (kFrameMoves).  The same compares on the same values either way: no bit differs.
// What a triangle step of the mask form changes in the ray state: who (m) and to what.  The predicate form has no such state (NoUpdate), and the variable lives at the
// walk's scope, not the loop's: a local of the loop's scope, even an empty one, gives the loop's exits a block of their own, and the alpha-test instances' any-hit walks
// then compile to more instructions than the parent commit's (7 224 -> 7 278 in k_frame<true, true, true, true, true>).
struct StepUpdate { uint64_t m = 0ull; float t, u, v; uint32_t pos, gid; };
struct NoUpdate {};
template <bool ANY, bool WIDE, int OCT, bool COUNT = false, bool ALPHA = false, bool HINTS = false, bool TSEL = false, class ON>   // HINTS: an any-hit walk that takes and leaves hints; TSEL: the alpha test's second taps wrap by a select (tex_taps)
__device__ __forceinline__ void packet_walk(const FrameArgs &a, const Ray &r, ON &on, int *stk, float &tbest, float &bu, float &bv, uint32_t &bpos, uint32_t &bgid, uint32_t &steps, PacketHints &h) {
    constexpr bool MASKS = std::is_same<ON, uint64_t>::value;
    int cur = HINTS ? h.cur : 0, sp = HINTS ? h.sp : 0; // wave-uniform
    constexpr int kPop = kAbsentChild;
    // ray visibility masks: the cull mask of this walk's rays, a kernel argument; rays with a cull mask of 0 see nothing
    // (read from the arguments where it is used: a value kept through the walk costs the multi-light instances a scalar register they do not have)
    const auto cull = [&]() -> uint32_t { return ANY ? (a.ray_masks >> 8) & 0xFFu : a.ray_masks & 0xFFu; };
    if (ALPHA && cull() == 0u) return;
#ifdef ART_PACKET_PROF
    unsigned long long pp_[12] = {1, 0, 0, 0, 0, 0, 0, OCT == 8, 0, 0, 0, 0}; bool from_stack_ = false; int hints_left_ = 0;
#endif // "take the next node from the stack" (no leaf has position 2^31 - 1); also what an absent child of a 4-wide node refers to
#ifdef ART_PACKET_PROF
    if (HINTS) hints_left_ = sp;   // (every seeded hint put one reference on the stack)
#endif
    typename std::conditional<MASKS, StepUpdate, NoUpdate>::type up;   // a step's changes to the ray state (set by a triangle step, read only where up.m says so)
    for (;;) {
#ifdef ART_PACKET_PROF
        const unsigned long long tk0_ = __builtin_amdgcn_s_memtime(); const bool was_node_ = cur >= 0;
#endif
        if constexpr (MASKS) up.m = 0ull;
        if (COUNT) steps++; // wave-uniform: nodes + triangles the packet visited (the fused frame's wave plan feeds on it; one s_add here costs 3.5 %, so only sampled frames count)
        if (cur >= 0 && WIDE) {
            // 4-wide node, float boxes (128 B, two scalar loads).  Its children were sorted at build time along the axis `ax` their centroids spread
            // most on, so the packet's front-to-back order is 0,1,2,3 or 3,2,1,0 by the sign of its rays' direction on that axis -- no per-lane
            // distances, no votes.  (Order only steers the culling: the answer is order-independent)  Absent children carry a
            // point box out at 3e38, which no ray passes (art_wide.hip).  Measured against the binary walk (profiles/README.md r2): scalar
            // instructions -43 %, vector instructions +9 % (all four boxes of a node are tested, also below a child the binary walk would have
            // culled), half the dependent node fetches: config 2 +1 %, config 3 +8 %, config 4 +11 % rays/s.  The default since round 2
            // (ArtTuning.packet_wide = 2 selects the binary walk).
            ConstQuads nq = const_quads(a.widef + cur);
            float4 w0 = nq[0], w1 = nq[1], w2 = nq[2], w3 = nq[3], w4 = nq[4], w5 = nq[5], w6 = nq[6], w7 = nq[7];
            const int c0 = __float_as_int(w6.x), c1 = __float_as_int(w6.y), c2 = __float_as_int(w6.z), c3 = __float_as_int(w6.w);
            float te;
            const uint64_t m0 = ballot64(slab_oct<OCT>(r, w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, tbest, te));
            const uint64_t m1 = ballot64(slab_oct<OCT>(r, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, tbest, te));
            // (Round 4 also skipped the third and fourth box where a node has no such child -- its valid mask is a scalar, and a node of the collapse has three children on
            // average, so a quarter of the 52 box-test instructions of a step test a point box at 3e38: configs 2 / 3 / 4 19 450 / 30 990 / 17 080 Mray/s against 19 270-19 530 /
            // 31 450 / 17 170 -- nothing: the launch is not short of vector issue slots the way its 0.68 suggests; a step's chain of dependent scalar loads, ballots and the LDS
            // pop is what the waves take turns waiting for.  profiles/README.md round 4.)
            const uint64_t m2 = ballot64(slab_oct<OCT>(r, w3.x, w3.y, w3.z, w3.w, w4.x, w4.y, tbest, te));
            const uint64_t m3 = ballot64(slab_oct<OCT>(r, w4.z, w4.w, w5.x, w5.y, w5.z, w5.w, tbest, te));
#ifdef ART_PACKET_PROF
            pp_[1]++; pp_[6] += (m0 != 0ull) + (m1 != 0ull) + (m2 != 0ull) + (m3 != 0ull); from_stack_ = false;
#endif
            const uint32_t ax = __float_as_uint(w7.y);                   // 0..2 (wave-uniform)
            // mixed packets (OCT 8) go by the majority sign on that axis
            bool rev = ((OCT >> ax) & 1) != 0;
            if constexpr (OCT >= 8 && MASKS) rev = 2 * (int)__popcll(on & ballot64((ax == 0 ? r.inv.x : (ax == 1 ? r.inv.y : r.inv.z)) < 0.0f)) > (int)__popcll(on);
            else if constexpr (OCT >= 8) rev = 2 * (int)__popcll(ballot64(on && (ax == 0 ? r.inv.x : (ax == 1 ? r.inv.y : r.inv.z)) < 0.0f)) > (int)__popcll(ballot64(on));
            const bool lane0 = (threadIdx.x & 63u) == 0;
            int next = kPop;
            if (!rev) { // near -> far = 0,1,2,3: stack the far ones first
                if (m3 != 0ull) next = c3;
                if (m2 != 0ull) { if (next != kPop) { if (lane0) stk[min(sp, kPacketStack - 1)] = next; sp = min(sp + 1, kPacketStack); } next = c2; }
                if (m1 != 0ull) { if (next != kPop) { if (lane0) stk[min(sp, kPacketStack - 1)] = next; sp = min(sp + 1, kPacketStack); } next = c1; }
                if (m0 != 0ull) { if (next != kPop) { if (lane0) stk[min(sp, kPacketStack - 1)] = next; sp = min(sp + 1, kPacketStack); } next = c0; }
            } else {
                if (m0 != 0ull) next = c0;
                if (m1 != 0ull) { if (next != kPop) { if (lane0) stk[min(sp, kPacketStack - 1)] = next; sp = min(sp + 1, kPacketStack); } next = c1; }
                if (m2 != 0ull) { if (next != kPop) { if (lane0) stk[min(sp, kPacketStack - 1)] = next; sp = min(sp + 1, kPacketStack); } next = c2; }
                if (m3 != 0ull) { if (next != kPop) { if (lane0) stk[min(sp, kPacketStack - 1)] = next; sp = min(sp + 1, kPacketStack); } next = c3; }
            }
            cur = next;
        } else if (cur >= 0) {
            ConstQuads nq = const_quads(a.nodes + cur);
            float4 q0 = nq[0], q1 = nq[1], q2 = nq[2], q3 = nq[3];
            int c0 = __float_as_int(q3.x), c1 = __float_as_int(q3.y);
            float te0, te1;
            // lanes that are off carry tbest = -1: their slab tests fail by themselves, so each ballot is one v_cmp into an SGPR pair
            uint64_t m0 = ballot64(slab_oct<OCT>(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tbest, te0));
            uint64_t m1 = ballot64(slab_oct<OCT>(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tbest, te1));
            if (m0 != 0ull && m1 != 0ull) { // both: go where most rays enter first, stack the other
                uint64_t fl = ballot64(te0 <= te1), both = m0 & m1;
                uint64_t f0 = (m0 & ~m1) | (both & fl), f1 = (m1 & ~m0) | (both & ~fl);
                bool first0 = (int)__popcll(f0) >= (int)__popcll(f1);
                if ((threadIdx.x & 63u) == 0) stk[min(sp, kPacketStack - 1)] = first0 ? c1 : c0;
                sp = min(sp + 1, kPacketStack);
                cur = first0 ? c0 : c1;
            } else if (m0 != 0ull) cur = c0;
            else if (m1 != 0ull) cur = c1;
            else cur = kPop;
        } else {
            uint32_t pos = (uint32_t)~cur;
            typedef __attribute__((address_space(4))) const uint32_t *Words;
            // the filtered instances: does this leaf's primitive need a look at its record (a cutoff > 0 or a visibility mask other than 0xFF)?  One scalar bit test.
            bool unseen = false;
            const auto flagged = [&]() -> bool { return ((((Words)(uintptr_t)a.alpha_bits)[pos >> 5] >> (pos & 31u)) & 1u) != 0u; };
            // the visibility rule, before anything else of the step: the triangle is wave-uniform, so its primitive id and that primitive's mask are scalar
            // loads and the decision a scalar branch -- a leaf no ray of this walk may see costs the wave no vector work.  (A hint step comes through here as well.)
            if (ALPHA && flagged()) {
                const float4 s8 = const_quads(a.shade_tris + pos)[8];
                const Words P = (Words)(uintptr_t)(a.prims + __float_as_uint(s8.z));
                unseen = (prim_vis(P[offsetof(DevPrim, masked) / 4]) & cull()) == 0u;
            }
            if (!unseen) {
                ConstQuads tq = const_quads(a.tris + pos);
                float4 ta = tq[0], tb = tq[1], tc = tq[2], td = tq[3];   // v0 e1 e2 lo hi gid: one 64-byte scalar load (DevTri)
                float te = 0.f, t = 0.f, u = 0.f, v = 0.f;
                // accept() = slab(AABB(tri)) AND Moeller-Trumbore: the conjunction is evaluated triangle test first -- the parent already
                // tested this very box for the packet, so nearly every wave would pay for the slab, while few lanes survive the triangle test
                if constexpr (MASKS) {
                    uint64_t acc = moller_trumbore_mask(r, mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), t, u, v) & on;
                    if (acc != 0ull) acc &= ballot64(slab_oct<OCT>(r, tc.y, tc.z, tc.w, td.x, td.y, td.z, tbest, te));   // (a wave-uniform branch: te is only read where acc is set)
                    // the alpha test: the triangle is wave-uniform, so its leaf bit, its shading record's uv and primitive id and that primitive's cutoff
                    // are scalar loads, made only when the bit is set and some lane took the candidate; then the lanes that did fetch their four texels
                    const auto alpha_keep = [&](uint64_t cand) -> uint64_t {
                        if (!ALPHA || cand == 0ull || !flagged()) return cand;
                        ConstQuads sq = const_quads(a.shade_tris + pos);
                        const float4 s2 = sq[2], s3 = sq[3], s8 = sq[8];
                        const Words P = (Words)(uintptr_t)(a.prims + __float_as_uint(s8.z));
                        const float c = __uint_as_float(P[offsetof(DevPrim, cutoff) / 4]);
                        if (!(c > 0.0f)) return cand;
                        const uint32_t toff = P[offsetof(DevPrim, texture_offset) / 4], tw = P[offsetof(DevPrim, tw) / 4], th = P[offsetof(DevPrim, th) / 4];
                        bool keep = __builtin_amdgcn_inverse_ballot_w64(cand);
                        if (keep) keep = !(alpha_at<TSEL>(a.tex_pool, toff, tw, th, s2, s3, u, v) < c);
                        return cand & ballot64(keep);
                    };
                    // the ray state itself changes behind the step (below): here only who changes, and to what
                    if (ANY) { // first accepted triangle: this lane is done
                        if (ALPHA) acc = alpha_keep(acc);
                        up.m = acc; up.pos = pos; on &= ~acc;
                        // a triangle that occluded some ray is next frame's hint (only accepting triangles are kept, so a hint that accepted nothing is forgotten after one frame)
                        // (the count is wave-uniform and stays in a scalar register: the ring index is scalar arithmetic)
                        if (HINTS && acc != 0ull) { const uint32_t n = launder(h.n); if ((threadIdx.x & 63u) == 0) stk[kPacketStack + (n & 3u)] = (int)pos; h.n = n + 1u; }
                    }
                    else {
                        float teff;   // = fmaxf(t, te): one v_max_f32 (fmaxf first quiets both operands, which are the results of arithmetic here: two more instructions a step)
                        asm("v_max_f32 %0, %1, %2" : "=v"(teff) : "v"(t), "v"(te));
                        uint32_t gid = __float_as_uint(td.w);
                        uint64_t better = acc & (ballot64(teff < tbest) | (ballot64(teff == tbest) & ballot64(gid < bgid))); // three compares and three mask operations
                        if (ALPHA) better = alpha_keep(better);   // (only a candidate that would win is tested: a cut one that would lose changes nothing)
                        up.m = better; up.t = teff; up.u = u; up.v = v; up.pos = pos; up.gid = gid;
                    }
#ifdef ART_PACKET_PROF
                    { uint64_t am_ = acc; pp_[2]++; pp_[3] += from_stack_; pp_[4] += am_ != 0ull; pp_[5] += __popcll(am_); }
                    if (ANY && hints_left_ > 0) { pp_[10]++; pp_[11] += on == 0ull; hints_left_--; }
#endif
                } else {   // the same step on per-lane predicates
                    bool acc = moller_trumbore_flat(r, mk(ta.x, ta.y, ta.z), mk(ta.w, tb.x, tb.y), mk(tb.z, tb.w, tc.x), t, u, v) && on;
                    if (acc) acc = slab_oct<OCT>(r, tc.y, tc.z, tc.w, td.x, td.y, td.z, tbest, te);
                    const auto alpha_keep = [&](bool cand) -> bool {
                        if (!ALPHA || ballot64(cand) == 0ull || !flagged()) return cand;
                        ConstQuads sq = const_quads(a.shade_tris + pos);
                        const float4 s2 = sq[2], s3 = sq[3], s8 = sq[8];
                        const Words P = (Words)(uintptr_t)(a.prims + __float_as_uint(s8.z));
                        const float c = __uint_as_float(P[offsetof(DevPrim, cutoff) / 4]);
                        if (!(c > 0.0f)) return cand;
                        const uint32_t toff = P[offsetof(DevPrim, texture_offset) / 4], tw = P[offsetof(DevPrim, tw) / 4], th = P[offsetof(DevPrim, th) / 4];
                        if (cand) cand = !(alpha_at<TSEL>(a.tex_pool, toff, tw, th, s2, s3, u, v) < c);
                        return cand;
                    };
                    // the ray state changes through selects, outside the divergent branches (no register copies around them)
                    if (ANY) { // first accepted triangle: this lane is done
                        if (ALPHA) acc = alpha_keep(acc);
                        bpos = acc ? pos : bpos; on = on && !acc; tbest = acc ? -1.0f : tbest;
                        if (HINTS && ballot64(acc) != 0ull) { if ((threadIdx.x & 63u) == 0) stk[kPacketStack + (h.n & 3u)] = (int)pos; h.n++; }
                    }
                    else {
                        float teff;
                        asm("v_max_f32 %0, %1, %2" : "=v"(teff) : "v"(t), "v"(te));
                        uint32_t gid = __float_as_uint(td.w);
                        bool better = acc & ((teff < tbest) | ((teff == tbest) & (gid < bgid))); // (bitwise: three compares and three mask operations, no nested exec regions)
                        if (ALPHA) better = alpha_keep(better);
                        tbest = better ? teff : tbest; bu = better ? u : bu; bv = better ? v : bv; bpos = better ? pos : bpos; bgid = better ? gid : bgid;
                    }
#ifdef ART_PACKET_PROF
                    { uint64_t am_ = ballot64(acc); pp_[2]++; pp_[3] += from_stack_; pp_[4] += am_ != 0ull; pp_[5] += __popcll(am_); }
                    if (ANY && hints_left_ > 0) { pp_[10]++; pp_[11] += ballot64(on) == 0ull; hints_left_--; }
#endif
                }
                if constexpr (!MASKS) { if (ANY && ballot64(on) == 0ull) break; } // every ray of the packet is occluded (the mask form: below, behind the change to the ray state)
            }
            cur = kPop;
        }
        // The ray state changes here, in one place on the way to the next step, through in-place selects under the step's mask: the loop-carried registers have this one
        // definition, and a step that changed no ray (a node step, most triangle steps) passes it by on a scalar branch.  (Inside the triangle step the new values met the
        // node step's unchanged ones at the end of the branch in registers of their own, and five copies brought them home.)
        if constexpr (MASKS) if (up.m != 0ull) {
            if (ANY) { sel(bpos, up.pos, up.m); sel_off(tbest, up.m); if (on == 0ull) break; }   // (every ray of the packet is occluded: the walk ends)
            else { sel(tbest, up.t, up.m); sel(bu, up.u, up.m); sel(bv, up.v, up.m); sel(bpos, up.pos, up.m); sel(bgid, up.gid, up.m); }
        }
        if (cur == kPop) {
            if (sp == 0) break;
            sp--;
            cur = __builtin_amdgcn_readfirstlane(stk[sp]); // same address in every lane: one broadcast LDS read (lane 0's write is ordered before it within the wave)
#ifdef ART_PACKET_PROF
            from_stack_ = true;
#endif
        }
#ifdef ART_PACKET_PROF
        pp_[was_node_ ? 8 : 9] += __builtin_amdgcn_s_memtime() - tk0_;
#endif
    }
#ifdef ART_PACKET_PROF
    for (int i = 0; i < 12; i++) PPROF(i, pp_[i]);
#endif
}

// one packet through the walk that fits its rays' direction signs
template <bool ANY, bool WIDE, bool COUNT = false, bool ALPHA = false, bool HINTS = false, bool MASKS = true, bool TSEL = false>   // MASKS: the walk in its mask form (packet_walk's ON)
__device__ __forceinline__ void walk_dispatch(const FrameArgs &a, const Ray &r, bool alive, int *stk, float &tbest, float &bu, float &bv, uint32_t &bpos, uint32_t &bgid, uint32_t &steps, PacketHints &h) {
    typename std::conditional<MASKS, uint64_t, bool>::type on;
    int oct;
    if constexpr (MASKS) {
        on = ballot64(alive);   // the packet's live lanes: a mask from here on (an any-hit walk takes lanes out of it)
        const uint64_t act = on;
        if (act == 0ull) return;
        // direction signs per axis: all set, none set, or mixed over the packet's rays -- three compares, the rest is scalar work
        uint64_t nx = act & ballot64(r.inv.x < 0.0f), ny = act & ballot64(r.inv.y < 0.0f), nz = act & ballot64(r.inv.z < 0.0f);
        bool uniform = (nx == 0ull || nx == act) && (ny == 0ull || ny == act) && (nz == 0ull || nz == act);
        oct = !uniform ? 8 : (int)(launder(nx ? 2u : 0u) >> 1) | (ny ? 2 : 0) | (nz ? 4 : 0);   // ("nx ? 1 : 0" widens a predicate, which is done on the vector unit)
    } else {
        on = alive;
        uint64_t act = ballot64(on);
        if (act == 0ull) return;
        uint64_t nx = ballot64(on && r.inv.x < 0.0f), ny = ballot64(on && r.inv.y < 0.0f), nz = ballot64(on && r.inv.z < 0.0f);
        bool uniform = (nx == 0ull || nx == act) && (ny == 0ull || ny == act) && (nz == 0ull || nz == act);
        oct = !uniform ? 8 : (nx ? 1 : 0) | (ny ? 2 : 0) | (nz ? 4 : 0);
    }
    switch (oct) {
    case 0: packet_walk<ANY, WIDE, 0, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    case 1: packet_walk<ANY, WIDE, 1, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    case 2: packet_walk<ANY, WIDE, 2, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    case 3: packet_walk<ANY, WIDE, 3, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    case 4: packet_walk<ANY, WIDE, 4, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    case 5: packet_walk<ANY, WIDE, 5, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    case 6: packet_walk<ANY, WIDE, 6, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    case 7: packet_walk<ANY, WIDE, 7, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    default: packet_walk<ANY, WIDE, 8, COUNT, ALPHA, HINTS, TSEL>(a, r, on, stk, tbest, bu, bv, bpos, bgid, steps, h); break;
    }
}

// The fused frame: one wave takes an 8x8 pixel block through the whole of raytrace.rgen.glsl -- primary packet, shading, one
// shadow packet per light, accumulation -- and writes only the frame's outputs.  No hit / shadow-ray / contribution records
// cross HBM, one launch per frame, and the CUs hold waves in every phase at once (node-fetch latency of the walks, texture
// latency and ALU of the shading), which is what the staged frame needed a dozen frames in flight for.  The arithmetic and its
// order are the staged kernels': the frames are bit-identical.  pix_bits[p]: bit i = light i shadowed, bit 16+i = shadow ray
// traced (art_get_stats counts rays from it on demand; art_read_shadow_bits).
// what lane `__lane_id()` of wave item `wid` traces: local pixel id, frame coordinates, whether the item's cell mask covers it; returns "traces a ray"
__device__ __forceinline__ bool frame_pixel(const FrameArgs &a, uint32_t wid, uint32_t &p, uint32_t &x, uint32_t &y, bool &mine) {
    // wave-uniform, read-only tables: constant address space, so these stay scalar loads behind the frame's stores too (no divisions either)
    typedef uint32_t U2 __attribute__((ext_vector_type(2)));
    const U2 item_ = ((__attribute__((address_space(4))) const U2 *)(uintptr_t)a.wave_items)[wid];
    const uint2 item = make_uint2(item_.x, item_.y);
    const uint32_t txy = ((__attribute__((address_space(4))) const uint32_t *)(uintptr_t)a.tile_xy)[item.x >> 4];    // the block's 32x32 tile: x | y << 16
    const uint32_t lane = __lane_id(), sub = item.x & 15u;
    p = item.x * 64u + lane;
    mine = (item.y >> (((lane >> 4) << 2) | ((lane >> 1) & 3u))) & 1u; // cell = (y/2)*4 + x/2 of the 8x8 block
    x = (txy & 0xFFFFu) * kTile + (sub & 3u) * 8u + (lane & 7u);
    y = (txy >> 16) * kTile + (sub >> 2) * 8u + (lane >> 3);
    return x < a.W && y < a.H && mine;
}
#ifdef ART_PHASE_PROF
// profiling build only (make EXTRA=-DART_PHASE_PROF; tools/phase_prof.py): shader-clock cycles a wave spends in each phase of k_frame, summed over waves
constexpr uint32_t kPhaseWaves = 1u << 18;
__device__ uint32_t g_phase[8][kPhaseWaves]; // [phase][wave item]: the last frame that ran wrote it
__device__ __forceinline__ uint64_t tick(float &dep) { uint64_t t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t), "+v"(dep)); return t; }
#define PHASE(i, dep) { uint64_t t1_ = tick(dep); if (__lane_id() == 0 && blockIdx.x < kPhaseWaves) g_phase[i][blockIdx.x] = (uint32_t)(t1_ - t0_); t0_ = t1_; }
#else
#define PHASE(i, dep)
#endif
// The instances of k_frame that take shadow-occluder hints: all but those whose register allocation the hint code moved past what the same instance had without it -- the
// binary-node walk with several frames per launch (one VGPR more in four of its instances) and the plain multi-light instance with the alpha test (two spilled registers);
// these ignore the table and walk from the root as before (tools/kres.sh; profiles/README.md, "shadow-occluder hints").  Any subset is a correct frame: hints change no bit.
// With the visibility rule in the triangle step the step-counting sibling of the latter over binary nodes went the same way (one spilled VGPR) and joined them.
template <bool WIDE, bool ONE_LIGHT, bool COUNT, bool BATCH, bool ALPHA> constexpr bool kFrameHints = !(!WIDE && BATCH) && !(ALPHA && !ONE_LIGHT && !COUNT && !BATCH) &&
                                                                                                      !(ALPHA && !WIDE && !ONE_LIGHT && COUNT && !BATCH);
// The instances of k_frame whose normalisations take the guarded fast paths (shade_surface's block guard, inv_sqrt_exact / sqrt_exact in the camera ray and shade_light): the
// one-light instances with one frame per launch and no alpha test -- the default instance, its step-counting sibling and the two over binary nodes.  These keep the register
// allocation they had with the plain expressions to the register (63 VGPRs, no scratch: tests/test_alpha.py and tests/test_ray_masks.py pin it).  Every other instance moved:
// one to three VGPRs more in the one-light ones, 2 to 10 spilled registers in the multi-light ones, which have no register to spare for the guard's note (tools/kres.sh;
// profiles/exact_math_kres_{parent,new}.txt, profiles/README.md "exact 1/sqrt").  Those compile the plain expressions, as before.  Any subset is the same frame: the fast
// paths change no bit.
template <bool WIDE, bool ONE_LIGHT, bool COUNT, bool BATCH, bool ALPHA> constexpr bool kFrameFastMath = ONE_LIGHT && !BATCH && !ALPHA;
// Which of the instruction-saving forms an instance of k_frame takes.  Bit 0: the packet walks in their mask form (sel(), packet_walk's ON).  Bits 1-5: the phases that read
// their kernel arguments again (frame_args_again) -- 1 the hit record and the depth / normal outputs, 2 the surface (with 1), 3 each light and its hints, 4 the hint entry
// behind a shadow walk, 5 the colour outputs.  Every form computes the same bits, so any subset is the same frame; an instance takes the largest subset that leaves its
// register allocation (VGPRs, scratch, spills, occupancy; no more SGPRs) exactly where it was, and none (0: the parent commit's code, instruction for instruction) where
// that subset left it with more v_readlane / v_writelane or more vector instructions than it had: eight instances with several frames per launch.  How the table was made:
// all 64 subsets compiled for all 32 instances with -DART_MOVES_FORCE=n, the largest subset whose resource line is the parent's taken, the mask form first; then every
// instance counted against the parent (profiles/moves_static_all.txt) and the eight set to 0 by hand.  tools/moves_sweep.py does the compiling and the counting and applies
// all of these conditions at once, but prefers the FEWEST vector instructions, so it may print another table that is as valid; this one is the one that was measured
// (profiles/README.md "moves").  23 of the 32 take the mask form, 15 everything; the default instance and its step-counting sibling take the mask form and phases 1 and 4 --
// with the surface or the light read again they spill seven vector registers.  Indexed by WIDE << 4 | ONE_LIGHT << 3 | COUNT << 2 | BATCH << 1 | ALPHA.
constexpr uint8_t kFrameMovesTable[32] = {55, 63, 63, 63, 55, 63, 0, 0, 49, 55, 63, 0, 49, 63, 63, 56, 31, 63, 63, 0, 63, 63, 63, 63, 19, 63, 0, 0, 19, 63, 0, 0};
#ifdef ART_MOVES_FORCE
template <bool WIDE, bool ONE_LIGHT, bool COUNT, bool BATCH, bool ALPHA> constexpr uint32_t kFrameMoves = ART_MOVES_FORCE;   // (the sweep that made the table)
#else
template <bool WIDE, bool ONE_LIGHT, bool COUNT, bool BATCH, bool ALPHA> constexpr uint32_t kFrameMoves = kFrameMovesTable[WIDE << 4 | ONE_LIGHT << 3 | COUNT << 2 | BATCH << 1 | ALPHA];
#endif
// Which of the short exact forms an instance of k_frame takes (profiles/README.md "short math").  Bits 0-8: the surface block's nine normalisations, in the
// block's order, as inv_sqrt_short; 9: the camera ray's; 10: the light's (L and H); 11: the camera ray's fx / W and fy / H as div_core; 12: the second taps of the
// surface's texture samples wrapped by a select; 13: those of the alpha test.  Bits 0-10 hang on the guards of kFrameFastMath and mean nothing in an instance without
// them; bit 13 means nothing without the alpha test.  Every form computes the same bits
// (tests/test_short_math.py, tests/test_short_math_frames.py), so any subset is the same frame; the rule is kFrameMoves': an instance takes a subset that reproduces its
// pinned resource line with no more vector instructions and no more lane accesses than the parent, the one with the fewest vector instructions, and 0 -- the parent's
// code, instruction for instruction -- where there is none.  tools/short_math_sweep.py compiles the candidates (-DART_SHORT_FORCE=n) and prints this table.
// Indexed like kFrameMovesTable.
constexpr uint16_t kFrameShortTable[32] = {0x1800, 0x3800, 0x1800, 0x1800, 0x1800, 0x3800, 0x1800, 0x3800, 0x1ffb, 0x2800, 0x0800, 0x2800, 0x1e00, 0x2800, 0x0800, 0x2800, 0x1800, 0x3800, 0x1800, 0x3800, 0x1800, 0x3800, 0x1800, 0x3800, 0x1ffb, 0x2800, 0x0800, 0x2800, 0x1ffb, 0x2800, 0x0800, 0x2800};
#ifdef ART_SHORT_FORCE
template <bool WIDE, bool ONE_LIGHT, bool COUNT, bool BATCH, bool ALPHA> constexpr uint32_t kFrameShortRaw = ART_SHORT_FORCE;   // (the sweep that made the table)
#else
template <bool WIDE, bool ONE_LIGHT, bool COUNT, bool BATCH, bool ALPHA> constexpr uint32_t kFrameShortRaw = kFrameShortTable[WIDE << 4 | ONE_LIGHT << 3 | COUNT << 2 | BATCH << 1 | ALPHA];
#endif
template <bool WIDE, bool ONE_LIGHT, bool COUNT, bool BATCH, bool ALPHA> constexpr uint32_t kFrameShort =
    kFrameShortRaw<WIDE, ONE_LIGHT, COUNT, BATCH, ALPHA> & ((kFrameFastMath<WIDE, ONE_LIGHT, COUNT, BATCH, ALPHA> ? 0x7FFu : 0u) | 0x1800u | (ALPHA ? 0x2000u : 0u));
// The kernel's arguments, looked at again: k_frame's phases -- the camera ray, the surface, every light, the outputs -- each read what they need of FrameArgs from the
// kernel-argument segment where they need it, through the constant address space (scalar loads that hit the scalar cache and stay scalar behind the frame's stores, like
// ConstQuads), instead of through `a`, whose fields the compiler loads once at the top and then parks across the walks in the lanes of a vector register (v_writelane /
// v_readlane, up to 86 of them in an instance).  The laundered pointer is what keeps a phase's loads from being merged with an earlier phase's.
__device__ __forceinline__ const FrameArgs &frame_args_again(const FrameArgs &a) {
#ifdef __HIP_DEVICE_COMPILE__
    __attribute__((address_space(4))) const char *p = (__attribute__((address_space(4))) const char *)__builtin_amdgcn_kernarg_segment_ptr();   // FrameArgs is k_frame's first argument
    asm volatile("" : "+s"(p));
    return *(const FrameArgs *)p;
#else
    return a;   // (host pass of the compiler only)
#endif
}
template <bool WIDE, bool ONE_LIGHT, bool COUNT = false, bool BATCH = false, bool ALPHA = false>   // WIDE: the 128-byte 4-wide nodes (the default) | the 64-byte binary nodes; ALPHA: the alpha test
__global__ __launch_bounds__(kFrameBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_frame(FrameArgs a_) {
    // One wave per workgroup: the waves of a frame are independent (nothing is shared, no barrier), and a workgroup of four held its LDS and its place
    // in the dispatcher's books until its slowest wave was done -- packets differ 25x in steps.  Single-wave groups: +2.5 % rays/s (profiles/README.md r2).
    __shared__ int wstack[kPacketStack + 4];   // + the ring of a shadow walk's accepting leaf positions (PacketHints)
    constexpr bool HINTS = kFrameHints<WIDE, ONE_LIGHT, COUNT, BATCH, ALPHA>;
    constexpr bool FASTM = kFrameFastMath<WIDE, ONE_LIGHT, COUNT, BATCH, ALPHA>;
    constexpr uint32_t MV = kFrameMoves<WIDE, ONE_LIGHT, COUNT, BATCH, ALPHA>;
    constexpr uint32_t SH = kFrameShort<WIDE, ONE_LIGHT, COUNT, BATCH, ALPHA>;
    int *stk = wstack;
    const uint32_t wid = blockIdx.x;
    if (wid >= a_.n_wave_items) return;
    uint32_t steps = 0; // packet steps of this wave, all walks
    const uint32_t fb = BATCH ? blockIdx.y : 0u;   // which frame of the launch (wave-uniform)
    const CameraArg &cam0 = (BATCH && fb) ? a_.cam_more[fb - 1] : a_.cam;
    const size_t frame_px = (size_t)fb * a_.W * a_.H, frame_local = (size_t)fb * a_.n_local;
    // The pixel a lane works on is looked up again wherever it is needed (here, at the depth/normal stores, at the end) instead of being
    // carried through the walks: the walks run at the 64-register edge.
    bool in;
    Ray r;
#ifdef ART_PHASE_PROF
    float dep0_ = 0.f; uint64_t t0_ = tick(dep0_);
#endif
    {
        uint32_t p, x, y; bool mine;
        in = frame_pixel(a_, wid, p, x, y, mine);
        float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
        // fx / W: 0.5 <= fx < 16384 + 32 (a block's lanes past the frame's edge compute too) and 1 <= W <= 16384 (art_resize): inside div_core's domain, and every such pair is swept
        float dx = ((SH & 0x800u) ? div_core(fx, (float)a_.W) : fx / (float)a_.W) * 2.0f - 1.0f, dy = ((SH & 0x800u) ? div_core(fy, (float)a_.H) : fy / (float)a_.H) * 2.0f - 1.0f;
        V3 org = mat4_mul(cam0.view_inv, 0.f, 0.f, 0.f, 1.f);
        V3 tgt = nrm3<FASTM, (SH & 0x200u) != 0u>(mat4_mul(cam0.proj_inv, dx, dy, 1.f, 1.f), a_.plain_math);
        V3 dir = mat4_mul(cam0.view_inv, tgt.x, tgt.y, tgt.z, 0.f);
        ray_init(r, org, dir, 0.001f, 10000.0f);
    }
    bool on = in && ray_finite(r.o, r.d);
    PHASE(0, r.inv.x)
    float tbest = on ? r.tmax : -1.0f, bu = 0.f, bv = 0.f;
    uint32_t bpos = kNoHit, bgid = kNoHit;
    { PacketHints none{0, 0, 0u}; walk_dispatch<false, WIDE, COUNT, ALPHA, false, (MV & 1u) != 0u, (SH & 0x2000u) != 0u>(a_, r, on, stk, tbest, bu, bv, bpos, bgid, steps, none); }   // (closest-hit walks take no hints)
    PHASE(1, tbest)
    const FrameArgs &a = (MV & 2u) ? frame_args_again(a_) : a_;   // the hit record, the depth and normal outputs
    const FrameArgs &as = (MV & 4u) ? a : a_;                      // the surface
    const CameraArg &cam = (BATCH && fb) ? as.cam_more[fb - 1] : as.cam;
    uint32_t p, x, y; bool mine;
    frame_pixel(a, wid, p, x, y, mine);
    if (a.keep_hits && mine) a.hits[frame_local + p] = bpos != kNoHit ? make_float4(tbest, bu, bv, __uint_as_float(bpos)) : make_float4(10000.0f, 0.f, 0.f, __uint_as_float(kNoHit));
    const bool hit = in && bpos != kNoHit;
    float out_depth = 10000.0f;
    V3 out_normal = mk(0.5f, 0.5f, 0.5f);
    Surface S;
    S.world_pos = mk(0.f, 0.f, 0.f); S.N = mk(0.f, 0.f, 1.f); S.Vv = mk(0.f, 0.f, 1.f); S.albedo = mk(0.f, 0.f, 0.f);
    S.metallic = 0.f; S.alpha = 0.f; S.nc_NdotV = 0.f; S.NdotV = 0.f;
    if (hit) shade_surface<FASTM, ONE_LIGHT && !BATCH && ALPHA, SH & 0x1FFu, (SH & 0x1000u) != 0u>(as, cam, bpos, bu, bv, S, out_depth, out_normal);
    if (in) {
        const size_t pix = frame_px + (size_t)y * a.W + x;
        st_nt(&a.depth[pix], out_depth);
        st_nt(&a.normal[pix], make_float4(out_normal.x, out_normal.y, out_normal.z, 1.0f));
    }
    PHASE(2, S.NdotV)
    float rx = 0.f, ry = 0.f, rz = 0.f;
    uint32_t sbits = 0, more = 0;
    // (until the walks fetched their nodes into SGPRs the multi-light instance parked the surface record in LDS across each shadow walk; it fits now)
    for (uint32_t i = 0; i < (ONE_LIGHT ? 1u : a_.n_lights); i++) { // uniform loop: the shadow packet needs the whole wave
        const FrameArgs &b = (MV & 8u) ? frame_args_again(a_) : a_;   // this light, its hints
        // the block's shadow-occluder hints for this light slot (FrameArgs::hints): one wave-uniform 16-byte load through the constant address space; the parts of a split
        // block share their block's entry.  Hints off (null table): the walk starts at the root with nothing in front of it, and nothing is stored.
        PacketHints hn{0, 0, 0u};
        typedef uint32_t U4 __attribute__((ext_vector_type(4)));
        if (HINTS && b.hints) {
            const uint32_t blk = ((__attribute__((address_space(4))) const uint32_t *)(uintptr_t)b.wave_items)[2u * wid];
            const U4 e = ((__attribute__((address_space(4))) const U4 *)(uintptr_t)b.hints)[blk * kHintLights + (i & (kHintLights - 1u))];
            hn = hints_seed(stk, e.x, e.y, e.z, e.w, b.hint_leaves);
        }
        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f), ro = make_float4(0.f, 0.f, 0.f, 1.0f), rd = make_float4(0.f, 0.f, 1.f, 0.f);
        bool want = false;
        const ArtLight L = ONE_LIGHT ? b.lights[0] : frame_light(b, i);
        if (hit) want = shade_light<FASTM, (SH & 0x400u) != 0u>(L, S, b.plain_math, c4, ro, rd);
        if (want) { if (i < 16u) sbits |= 1u << (16u + i); else more++; }   // (lights 16.. have no bits of their own: their shadow rays are counted)
        Ray sr;
        if (L.type == 2u) ray_init_inv(sr, mk(ro.x, ro.y, ro.z), ld3(L.area_pos2), ld3(L.area_pos3), 0.01f, L.penumbra_angle); // (wave-uniform branch)
        else ray_init(sr, mk(ro.x, ro.y, ro.z), mk(rd.x, rd.y, rd.z), 0.01f, ro.w);
        bool son = want && ray_finite(sr.o, sr.d);
        PHASE(3, sr.inv.x)
        float st = son ? sr.tmax : -1.0f, su = 0.f, sv = 0.f;
        uint32_t spos = kNoHit, sgid = kNoHit;
        const uint64_t traced = HINTS ? ballot64(son) : 0ull;
        walk_dispatch<true, WIDE, COUNT, ALPHA, HINTS, (MV & 1u) != 0u, (SH & 0x2000u) != 0u>(b, sr, son, stk, st, su, sv, spos, sgid, steps, hn);
        const FrameArgs &c = (MV & 16u) ? frame_args_again(a_) : a_;   // where the walk's hints go
        if (HINTS && c.hints && traced != 0ull) { // (no shadow ray: the entry is left alone -- the idle wave of a split block shares the entry of the block's working parts)
            // the walk's occluders, the most recent first; the entry's address and what it holds now are looked up again (launder: like the pixel, nothing of this is carried
            // through the walk in registers); lane 0 writes them with one plain vector store unless the entry already says so
            uint32_t o[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) o[k] = k < hn.n ? (uint32_t)stk[kPacketStack + ((hn.n - 1u - k) & 3u)] : kHintEmpty;
            const uint32_t blk = ((__attribute__((address_space(4))) const uint32_t *)(uintptr_t)c.wave_items)[2u * launder(wid)];
            const size_t at = blk * kHintLights + (i & (kHintLights - 1u));
            const U4 e = ((__attribute__((address_space(4))) const U4 *)(uintptr_t)c.hints)[at];
            if (((e.x ^ o[0]) | (e.y ^ o[1]) | (e.z ^ o[2]) | (e.w ^ o[3])) != 0u && __lane_id() == 0) reinterpret_cast<uint4 *>(c.hints)[at] = make_uint4(o[0], o[1], o[2], o[3]);
        }
        PHASE(4, st)
        if (want && spos != kNoHit) { // shadowed: the light keeps 0.05 of its contribution (raytrace.rgen.glsl:179-181)
            c4 = make_float4(c4.x * 0.05f, c4.y * 0.05f, c4.z * 0.05f, c4.w);
            if (i < 16u) sbits |= 1u << i;
        }
        rx += c4.x * c4.w; ry += c4.y * c4.w; rz += c4.z * c4.w; // rgen:185, lights in order
    }
    if (!in) { rx = 0.f; ry = 0.f; rz = 0.f; }
    float4 o = make_float4(rx, ry, rz, 1.0f);
    const FrameArgs &e = (MV & 32u) ? frame_args_again(a_) : a_;   // the outputs
    frame_pixel(e, wid, p, x, y, mine);
    if (in) st_nt(&e.color[frame_px + (size_t)y * e.W + x], o);
    if (e.color_tiles && mine) { // compact tile buffer for the gather: row-major inside each 32x32 tile
        uint32_t q = p & 1023u, sub = q >> 6, l = q & 63u;
        uint32_t lx = (sub & 3u) * 8u + (l & 7u), ly = (sub >> 2) * 8u + (l >> 3);
        size_t ti = (size_t)fb * e.tiles_stride + (size_t)(p >> 10) * kTilePixels + ly * kTile + lx;
        if (e.tiles_packed) __builtin_nontemporal_store(pack_b10g11r11(o.x, o.y, o.z), reinterpret_cast<uint32_t *>(e.color_tiles) + ti);
        else st_nt_rgb(e.color_tiles, ti, o);
    }
    if (mine) e.pix_bits[frame_local + p] = sbits;
    if (!ONE_LIGHT && e.pix_more && mine) e.pix_more[frame_local + p] = more;   // more than 16 lights: shadow rays of lights 16.. (art_get_stats)
    PHASE(5, rx)
#ifdef ART_PHASE_PROF
    if (__lane_id() == 0 && blockIdx.x < kPhaseWaves) { g_phase[6][blockIdx.x] = 1u; g_phase[7][blockIdx.x] = steps; }
#endif
    if (COUNT && __lane_id() == 0) e.wave_cost[wid] = steps; // feedback for the next plan (art_api.hip plan_poll)
}

// ---- the wave plan, on the device ---------------------------------------------------------------------------------------------------------------------------------
// Rounds 1-3 made it on the host: the step counts of a sampled frame travelled up, one thread went through 32 640 blocks and built the next table (0.3-0.9 ms inside an
// art_trace call every few frames once the camera moves: frames are 0.16 ms), the table travelled down.  One workgroup does the same in ~20 us behind the sampled frame on
// that frame's stream; the host only learns "a new table of n items is ready" from pinned memory once the event behind this launch has fired.
// Table layout (what plan_build_items made): the split blocks' parts first -- sixteen cells each, then four quadrants each: the long poles start first -- padded with idle
// waves to whole groups of 32, then every 256-pixel block of the launch order as four 8x8 items (mask 0: an idle wave where the block is split); finally the deal that keeps
// the four waves of launch block 8g + x on XCD x (workgroup j runs on XCD j % 8): position 32g + 4x + k goes to 32g + 8k + x.  (Whole groups of 32, not of four: the parts are
// a multiple of four as they are, and the deal's groups must be the launch order's own -- behind 4 s items, s not a multiple of 8, launch block L sat on XCD (L + s) % 8.)
__device__ __forceinline__ uint32_t plan_block_sum(uint32_t v, uint32_t *sh) {   // sum over the 1024 threads, in every thread (sh: 16 words)
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int i = 0; i < 16; i++) t += sh[i];
    return t;
}
__device__ __forceinline__ uint32_t plan_deal(uint32_t j, uint32_t total) { const uint32_t g = j >> 5; return (g + 1u) * 32u <= total ? g * 32u + 8u * (j & 3u) + ((j & 31u) >> 2) : j; }
__global__ __launch_bounds__(1024) void k_plan(PlanArgs p) {
    __shared__ uint32_t sh[16], sc2[1024], sc1[1024];
    __shared__ unsigned long long sh64[16];
    const uint32_t tid = threadIdx.x;
    // 1. the slowest wave of every block in the sampled frame, and the frame's steps
    unsigned long long sum = 0;
    for (uint32_t i = tid; i < p.n_items_in; i += 1024u) { const uint2 it = p.items_in[i]; if (it.y) { const uint32_t c = p.cost[i]; atomicMax(&p.worst[it.x], c); sum += c; } }
    for (int off = 32; off >= 1; off >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, off);
    if ((tid & 63u) == 0) sh64[tid >> 6] = sum;
    __threadfence_block();
    __syncthreads();
    sum = 0;
    for (int i = 0; i < 16; i++) sum += sh64[i];
    uint32_t T = p.fixed_steps ? p.fixed_steps : max(p.min_steps, (uint32_t)(p.share * (float)sum));
    // 2. every block's level; a block that has to be split is a wave that outlasts its launch, blocks that could be put together again only save a few steps (going down needs
    //    a clear margin: the parts of a split block share the top of their walks)
    const uint32_t per = (p.n64 + 1023u) / 1024u, b0 = min(tid * per, p.n64), b1 = min(b0 + per, p.n64);
    uint32_t n1 = 0, n2 = 0, N1 = 0, N2 = 0, ups = 0, downs = 0, split = 0, wmax = 0;
    for (int attempt = 0; attempt < 8; attempt++, T += T / 2) {
        n1 = n2 = 0; uint32_t u = 0, d = 0, sp = 0;
        for (uint32_t b = b0; b < b1; b++) {
            const uint32_t w = __hip_atomic_load(&p.worst[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (written by atomics of other waves of this workgroup)
            const uint32_t old = p.level[b];
            uint32_t lv = old;
            if (old == 0) lv = w > 4u * T ? 2u : (w > T ? 1u : 0u);
            else if (old == 1) lv = w > T ? 2u : (w * 4u < T / 2u ? 0u : 1u);
            else lv = w * 4u < T / 2u ? 1u : 2u;
            p.level_tmp[b] = (uint8_t)lv;
            n1 += lv == 1u; n2 += lv == 2u; u += lv > old; d += lv < old; sp += old != 0u; wmax = max(wmax, w);
        }
        N1 = plan_block_sum(n1, sh); N2 = plan_block_sum(n2, sh); ups = plan_block_sum(u, sh); downs = plan_block_sum(d, sh); split = plan_block_sum(sp, sh);
        if (p.n64 + (p.n64 & 3u) + 4u * N1 + 16u * N2 + 32u <= p.cap) break;   // (the padding is at most 28 items)
        if (attempt == 7) { N1 = N2 = ups = downs = 0; for (uint32_t b = b0; b < b1; b++) p.level_tmp[b] = p.level[b]; n1 = n2 = 0; }   // (never seen: no target fits -- the plan stays)
    }
    for (int off = 32; off >= 1; off >>= 1) wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, off));
    __syncthreads();
    if ((tid & 63u) == 0) sh[tid >> 6] = wmax;
    __syncthreads();
    for (int i = 0; i < 16; i++) wmax = max(wmax, sh[i]);
    for (uint32_t b = b0; b < b1; b++) p.worst[b] = 0u;   // clear for the next sample
    const bool changed = p.fixed_steps ? (ups + downs) != 0u : (ups != 0u || downs > max(16u, split / 4u));
    if (!changed) { if (tid == 0) { p.result[1] = 0u; p.result[4] = T; p.result[5] = wmax; } return; }
    // 3. where every thread's split blocks go: exclusive scans of the per-thread counts
    sc2[tid] = n2; sc1[tid] = n1;
    __syncthreads();
    uint32_t base2 = 0, base1 = 0;
    for (uint32_t i = 0; i < tid; i++) { base2 += sc2[i]; base1 += sc1[i]; }   // (1024 LDS reads a thread: a microsecond)
    const uint32_t heavy = 16u * N2 + 4u * N1, heavy_pad = (heavy + 31u) & ~31u, total = heavy_pad + p.n256 * 4u;
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t lv = p.level_tmp[b];
        p.level[b] = (uint8_t)lv;
        if (lv == 2u) { for (uint32_t cell = 0; cell < 16u; cell++) p.items_out[plan_deal(16u * base2 + cell, total)] = make_uint2(b, 1u << cell); base2++; }
        else if (lv == 1u) { const uint32_t quad[4] = {0x0033u, 0x00CCu, 0x3300u, 0xCC00u}; for (uint32_t q = 0; q < 4u; q++) p.items_out[plan_deal(16u * N2 + 4u * base1 + q, total)] = make_uint2(b, quad[q]); base1++; }
    }
    for (uint32_t j = heavy + tid; j < heavy_pad; j += 1024u) p.items_out[plan_deal(j, total)] = make_uint2(0u, 0u);
    __threadfence_block();
    __syncthreads();   // (level[] of other threads' blocks is read below)
    // 4. the blocks in launch order; a split block leaves an idle wave behind: the XCD order of the rest is untouched
    for (uint32_t r = tid; r < p.n256 * 4u; r += 1024u) {
        const uint32_t b = p.order[r >> 2] * 4u + (r & 3u);
        p.items_out[plan_deal(heavy_pad + r, total)] = make_uint2(b, p.level[b] ? 0u : 0xFFFFu);
    }
    if (tid == 0) { p.result[0] = total; p.result[1] = 1u; p.result[2] = N1; p.result[3] = N2; p.result[4] = T; p.result[5] = wmax; }
}
void launch_plan(const PlanArgs &p, hipStream_t s) { k_plan<<<1, 1024, 0, s>>>(p); }

template <bool WIDE, bool ONE_LIGHT, bool ALPHA = false> static void launch_frame_form(const FrameArgs &a, uint32_t g, bool count, hipStream_t s) {
    if (a.batch > 1) { // several frames per launch
        const dim3 gb(g, a.batch);
        if (count) k_frame<WIDE, ONE_LIGHT, true, true, ALPHA><<<gb, kFrameBlock, 0, s>>>(a); else k_frame<WIDE, ONE_LIGHT, false, true, ALPHA><<<gb, kFrameBlock, 0, s>>>(a);
    } else if (count) k_frame<WIDE, ONE_LIGHT, true, false, ALPHA><<<g, kFrameBlock, 0, s>>>(a);
    else k_frame<WIDE, ONE_LIGHT, false, false, ALPHA><<<g, kFrameBlock, 0, s>>>(a);
}
bool launch_frame(const FrameArgs &a, hipStream_t s) { // returns whether the launch wrote a.wave_cost
    const uint32_t g = a.n_wave_items;   // one workgroup per wave item
    if (g == 0) return false;
    const bool one = a.n_lights == 1;
    const bool count = a.wave_cost != nullptr && a.n_lights > 0; // a sampled frame of the wave plan: the step-counting instances
    if (a.alpha) {   // some enabled primitive has an alpha cutoff: the instances with the alpha test
        if (a.packet_wide) { if (one) launch_frame_form<true, true, true>(a, g, count, s); else launch_frame_form<true, false, true>(a, g, count, s); }
        else { if (one) launch_frame_form<false, true, true>(a, g, count, s); else launch_frame_form<false, false, true>(a, g, count, s); }
    } else if (a.packet_wide) { if (one) launch_frame_form<true, true>(a, g, count, s); else launch_frame_form<true, false>(a, g, count, s); }
    else { if (one) launch_frame_form<false, true>(a, g, count, s); else launch_frame_form<false, false>(a, g, count, s); }
    return count;
}
#ifdef ART_PACKET_PROF
extern "C" int32_t art_debug_packet_prof(unsigned long long *out, int32_t reset) { // out[24]
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_packet_prof), sizeof(g_packet_prof)) != hipSuccess) return -1;
    void *dp = nullptr;
    if (reset && (hipGetSymbolAddress(&dp, HIP_SYMBOL(g_packet_prof)) != hipSuccess || hipMemset(dp, 0, sizeof(g_packet_prof)) != hipSuccess)) return -1;
    return 0;
}
#endif
#ifdef ART_PHASE_PROF
extern "C" int32_t art_debug_phase(uint32_t *out, int32_t reset) { // out[8][2^18]
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(g_phase)) != hipSuccess) return -1;
    void *dp = nullptr;
    if (reset && (hipGetSymbolAddress(&dp, HIP_SYMBOL(g_phase)) != hipSuccess || hipMemset(dp, 0, sizeof(g_phase)) != hipSuccess)) return -1;
    return 0;
}
#endif

} // namespace art
