// art_refit.hip -- the per-frame refit of the 4-wide tree (gfx950) and its once-per-tree work lists: a model moved (VkModel::set_model_matrix, vk_model.rs:461-466; the
// reference rebuilds its TLAS every frame for this, renderer.rs:637-651) or its vertices were replaced.  The record operations are art_records.h's, the build's own.
// The topology stays, the world-space triangles of the version and every box above them are made again.  Results cannot depend on it: accept() is per
// triangle and every node box is an exact min / max union of the triangle boxes below it -- the frames are those of a fresh build.
#include "art_records.h"

namespace art {

// the version's triangle records from the object-space shading records (the vertices k_leaves gathered) and the version's object->world matrices: k_soup's
// transform (xform_point) and k_leaves' record (make_dev_tri), so a refit with unchanged matrices writes the bits that are there
// Only what moved is made again: touched[primitive] says whose triangles (the primitives moved since this VERSION was last written).  The primitive table and
// the touched bytes are read WHERE THE HOST WROTE THEM (pinned, device-visible memory: a few hundred bytes a wave touches once); the launch also leaves the table's device copy for the frames behind it.
// A rewritten triangle marks the 4-wide node that holds it (mark[w] != 0: a box below w changes in this refit); the level passes below carry the marks upwards.
// A primitive whose vertices were replaced since the version was written (art_scene_set_vertices: touched & kTouchRegather) first has the version's shading record
// gathered again, by k_leaves' own gather_shade_tri, from the vertices the version's primitive table points at (the version's staging copy in device memory);
// its positions are then transformed exactly like a moved primitive's: the bits a build over the new vertices writes.
__device__ __forceinline__ void regather_one(uint32_t p, uint32_t prim, const DevPrim *prims_host, const DevTri *tris, DevShadeTri *__restrict__ shade) {
    const DevPrim &P = prims_host[prim]; shade[p] = gather_shade_tri(P, prim, __float_as_uint(tris[p].f[15]) - P.first_tri);
}
__device__ __forceinline__ void retri_one(uint32_t p, DevShadeTri *__restrict__ shade, const DevPrim *prims_host, const uint8_t *touched, const uint32_t *__restrict__ leaf_parent, uint32_t *mark, DevTri *tris) {
    const uint32_t prim = __float_as_uint(shade[p].f[34]);
    const uint8_t how = touched[prim];
    if (!how) return;
    if (how & kTouchRegather) regather_one(p, prim, prims_host, tris, shade);   // (a masked primitive's too: it shows its new shape when it is enabled again)
    DevTri t;
    if (prims_host[prim].masked & kPrimOut) {   // out of the structure until it is enabled again: a point nowhere, no extent
        for (int k = 0; k < 3; k++) { t.f[k] = kNowhere; t.f[3 + k] = 0.f; t.f[6 + k] = 0.f; t.f[9 + k] = kNowhere; t.f[12 + k] = kNowhere; }
        t.f[15] = tris[p].f[15];
    } else {
        const float4 *sq = reinterpret_cast<const float4 *>(shade + p);
        const float4 s0 = sq[0], s1 = sq[1], s2 = sq[2];
        const float *m = prims_host[prim].o2w;
        const float3 w0 = xform_point(m, s0.x, s0.y, s0.z), w1 = xform_point(m, s0.w, s1.x, s1.y), w2 = xform_point(m, s1.z, s1.w, s2.x);
        const float a[3] = {w0.x, w0.y, w0.z}, b[3] = {w1.x, w1.y, w1.z}, c[3] = {w2.x, w2.y, w2.z};
        t = make_dev_tri(a, b, c, tris[p].f[15]); // the global triangle id never changes
    }
    tris[p] = t;
    mark[leaf_parent[p]] = 1u;
}
// which 4-wide node holds a leaf, which one a node (the root: ~0): made once per tree, when its first model moves
__global__ __launch_bounds__(256) void k_wide_parents(uint32_t n_wide, const DevNodeW *__restrict__ widef, uint32_t *__restrict__ leaf_parent, uint32_t *__restrict__ node_parent) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_wide) return;
    if (w == 0) node_parent[0] = ~0u;
    for (int i = 0; i < 4; i++) {
        const int32_t ch = widef[w].child[i];
        if (ch == kAbsentChild) continue;
        if (ch < 0) leaf_parent[(uint32_t)~ch] = w; else node_parent[ch] = w;
    }
}
// One child box of one node of the 4-wide tree: a leaf child's box is its triangle's, an internal child's the union of that node's own child boxes (float min / max
// are exact, so whatever the order the union is the box a build would find).  Four neighbouring lanes share a node; the pass is loads and min / max only -- the
// quantised records are made afterwards, for all nodes at once (k_wide_requant): their double-precision arithmetic does not belong on the bottom-up critical path.
__device__ __forceinline__ void wide_union_child(uint32_t w, uint32_t i, const DevTri *__restrict__ tris, DevNodeW *widef, const uint32_t *__restrict__ node_parent, uint32_t *mark) {
    if (!mark[w]) return;                               // nothing below this node moved
    if (i == 0) { const uint32_t up = node_parent[w]; if (up != ~0u) mark[up] = 1u; }   // its parent's box of it changes: a level further up, a launch (or a barrier) later
    const int32_t ch = widef[w].child[i];
    if (ch == kAbsentChild) return;
    float lo[3], hi[3];
    if (ch < 0) {
        const float4 *tq = reinterpret_cast<const float4 *>(tris + (uint32_t)~ch);
        const float4 c = tq[2], d = tq[3];                  // f[8..11] | f[12..15]: e2.z lo.xyz | hi.xyz gid
        lo[0] = c.y; lo[1] = c.z; lo[2] = c.w; hi[0] = d.x; hi[1] = d.y; hi[2] = d.z;
    } else {
        const float4 *q = reinterpret_cast<const float4 *>(widef + ch);
        const float4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], a5 = q[5];
        const uint32_t cv = widef[ch].valid;
        const float b[4][6] = {{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y}, {a1.z, a1.w, a2.x, a2.y, a2.z, a2.w}, {a3.x, a3.y, a3.z, a3.w, a4.x, a4.y}, {a4.z, a4.w, a5.x, a5.y, a5.z, a5.w}};
        for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
        for (int j = 0; j < 4; j++) if (((cv >> j) & 1u) && !box_nowhere(b[j][0])) for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], b[j][k]); hi[k] = fmaxf(hi[k], b[j][3 + k]); }
        if (lo[0] > hi[0]) for (int k = 0; k < 3; k++) { lo[k] = kNowhere; hi[k] = kNowhere; }   // nothing left below that node: nowhere itself
    }
    float *o = widef[w].box[i];
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
}
// one node of the pass behind the boxes: its quantised record (the per-ray walks' DevNode4) from its float one if asked, and what it adds to the tree's surface-area cost
// (the half-areas of its child boxes); the root also leaves the half-area of its union in acc[1]
__device__ __forceinline__ double wide_requant_node(uint32_t w, const DevNodeW *__restrict__ widef, DevNode4 *__restrict__ wide, bool requant, double *acc) {
    const float4 *q = reinterpret_cast<const float4 *>(widef + w);
    const float4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], a5 = q[5];
    const int4 ch = *reinterpret_cast<const int4 *>(&widef[w].child[0]);
    const float lo[4][3] = {{a0.x, a0.y, a0.z}, {a1.z, a1.w, a2.x}, {a3.x, a3.y, a3.z}, {a4.z, a4.w, a5.x}}, hi[4][3] = {{a0.w, a1.x, a1.y}, {a2.y, a2.z, a2.w}, {a3.w, a4.x, a4.y}, {a5.y, a5.z, a5.w}};
    const int nc = (ch.x != kAbsentChild) + (ch.y != kAbsentChild) + (ch.z != kAbsentChild) + (ch.w != kAbsentChild); // the valid children are slots 0 .. nc-1
    if (requant) {
        const float *plo[4] = {lo[0], lo[1], lo[2], lo[3]}, *phi[4] = {hi[0], hi[1], hi[2], hi[3]};
        DevNode4 d;
        wide_quantise(plo, phi, nc, d);
        d.child[0] = ch.x; d.child[1] = ch.y; d.child[2] = ch.z; d.child[3] = ch.w;
        wide[w] = d;
    }
    double a = 0.0;
    float rlo[3] = {INFINITY, INFINITY, INFINITY}, rhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = 0; j < nc; j++) {
        if (box_nowhere(lo[j][0])) continue;
        double dx = (double)hi[j][0] - lo[j][0], dy = (double)hi[j][1] - lo[j][1], dz = (double)hi[j][2] - lo[j][2];
        a += dx * dy + dy * dz + dz * dx;
        for (int k = 0; k < 3; k++) { rlo[k] = fminf(rlo[k], lo[j][k]); rhi[k] = fmaxf(rhi[k], hi[j][k]); }
    }
    if (w == 0) { double dx = (double)rhi[0] - rlo[0], dy = (double)rhi[1] - rlo[1], dz = (double)rhi[2] - rlo[2]; acc[1] = dx < 0 ? 0.0 : dx * dy + dy * dz + dz * dx; }
    return a;
}
// the refit's result block {cost sum, root half-area, start stamp, end stamp} from acc (see k_wide_requant), and acc cleared for the next refit
__device__ __forceinline__ void refit_result(double *out, double sum, double *acc) {
    out[0] = sum; out[1] = *(volatile double *)&acc[1];
    reinterpret_cast<unsigned long long *>(out)[2] = *(volatile unsigned long long *)&acc[2]; reinterpret_cast<unsigned long long *>(out)[3] = wall_clock64();
    acc[0] = 0.0; acc[1] = 0.0;
}
// The tree cut into BATCHES of whole subtrees of about kBatchNodes nodes (refit_lists_build) and the crown above them: ONE workgroup rewrites a batch's triangles and then refits
// its nodes level by level, deepest first, with a workgroup barrier between levels -- everything a node of the batch depends on is the batch's own, written through the one L1
// of the CU the workgroup runs on; a second launch of one large workgroup does the same for the crown (the few hundred nodes whose subtrees are larger than a batch).
// (Measured and dropped, DESIGN.md 3.1 / profiles/README.md round 4: a launch per level of the whole tree; one launch with arrival counters, whose agent-scope release and
// acquire per node write back and invalidate the XCD's L2 where a workgroup barrier costs nothing of the kind.)
// sub_off: [0, nb + 1] node offsets of batches 0 .. nb (batch nb = the crown) | [nb + 2, 2 nb + 3] leaf offsets | then nb + 1 rows of (n_levels + 1) offsets into the batch's
// node list, deepest level of the tree first.
template <bool FOLD> __global__ void k_refit_sub(uint32_t batch0, uint32_t nb1 /*batches + the crown*/, uint32_t n_levels, const uint32_t *__restrict__ sub_nodes, const uint32_t *__restrict__ sub_leaves, const uint32_t *__restrict__ sub_off,
                            DevShadeTri *__restrict__ shade, const DevPrim *prims_host, DevPrim *prims_dev, uint32_t n_prim_words, const uint8_t *touched,
                            const uint32_t *__restrict__ leaf_parent, const uint32_t *__restrict__ node_parent, uint32_t *mark, DevTri *tris, DevNodeW *widef, unsigned long long *stamp, bool first_launch,
                            DevNode4 *wide, double *acc, double *out /*null: not the refit's last launch*/, const uint32_t *__restrict__ dirty /*null: batch batch0 + blockIdx.x*/, double *batch_cost) {
    const uint32_t b = dirty ? dirty[blockIdx.x] : batch0 + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    if (first_launch) {
        if (blockIdx.x == 0 && tid == 0) stamp[0] = wall_clock64();   // the refit's start (100 MHz): its device time travels to the host with its cost, no events
        for (uint32_t i = blockIdx.x * nt + tid; i < n_prim_words; i += gridDim.x * nt) reinterpret_cast<uint32_t *>(prims_dev)[i] = reinterpret_cast<const uint32_t *>(prims_host)[i];   // the table's device copy, for the frames
    }
    for (uint32_t i = sub_off[nb1 + 1 + b] + tid; i < sub_off[nb1 + 2 + b]; i += nt) retri_one(sub_leaves[i], shade, prims_host, touched, leaf_parent, mark, tris);
    __threadfence_block();
    __syncthreads();
    const uint32_t *lv_off = sub_off + 2 * (nb1 + 1) + (size_t)b * (n_levels + 1), n0 = sub_off[b];
    for (uint32_t lv = 0; lv < n_levels; lv++) {         // (the same trips for every thread of the workgroup)
        const uint32_t lo = lv_off[lv], hi = lv_off[lv + 1];
        if (hi == lo) continue;
        for (uint32_t i = 4u * lo + tid; i < 4u * hi; i += nt) wide_union_child(sub_nodes[n0 + (i >> 2)], i & 3u, tris, widef, node_parent, mark);
        __threadfence_block();
        __syncthreads();   // the level above reads these records
    }
    // Round 4g: what k_wide_requant does in a launch of its own behind the crown each workgroup does for ITS nodes while they are warm: the quantised records of the marked
    // ones (marks cleared), its share of the tree's cost.  The crown's workgroup runs behind all the batches (stream order) and hands the result to the host.
    if (!FOLD) return;   // (a small tree: k_wide_requant does this behind the crown, a node a thread -- see launch_refit; the instance without this tail keeps 40 registers
                         //  and eight waves a SIMD -- with it 122, and a crown of 1 024 threads would need a CU all to itself)
    __shared__ double s_cost[16];
    double a = 0.0;
    for (uint32_t i = sub_off[b] + tid; i < sub_off[b + 1]; i += nt) {
        const uint32_t w = sub_nodes[i];
        const bool m = mark[w] != 0u;
        if (m) mark[w] = 0u;
        a += wide_requant_node(w, widef, wide, m && wide, acc);
    }
    if (out) for (uint32_t i = tid; i + 1u < nb1; i += nt) a += batch_cost[i];   // the crown: every batch's share, made by this refit or kept from an earlier one of this version
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    if ((tid & 63u) == 0) s_cost[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (uint32_t i = 0; i < (nt + 63u) / 64u; i++) t += s_cost[i];
        if (out) refit_result(out, t, acc); else batch_cost[b] = t;
    }
}
// after the boxes: every node's quantised record (the per-ray walks', DevNode4) from its float one, and the tree's surface-area cost while the boxes are at hand:
// cost[0] += the half-areas of all child boxes (the measure of the rays that cross each box: what a walk pays for), cost[1] = half-area of the root's union.  A refit
// can only keep or grow the sum against the same rays; a rebuild restores it (the rule compares the plain sums: DESIGN.md 3.1, "Rebuild behind a quality threshold").
// acc (device): [0] the running sum, [1] the root's half-area, [2] the refit's start stamp (k_retri), [3] exit ticket of this launch (as a 64-bit counter).  The last block
// out writes {sum, root, start, end} to `out` -- pinned host memory when a refit's result travels to the host behind its `ready` event (no copy, no event of its
// own), a device buffer otherwise -- and clears acc for the next launch.
__global__ __launch_bounds__(256) void k_wide_requant(uint32_t n_wide, const DevNodeW *__restrict__ widef, DevNode4 *__restrict__ wide, uint32_t *mark /*null: every node*/, double *acc, double *out) {
    __shared__ double s_part[4];
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    double a = 0.0;
    if (w < n_wide) {
        const bool requant = wide && (!mark || mark[w]);      // the double-precision quantisation only where a box changed; the cost sums every node
        if (mark && mark[w]) mark[w] = 0;                      // (the marks are this version's: cleared for its next refit)
        a = wide_requant_node(w, widef, wide, requant, acc);
    }
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
        if (t != 0.0) atomicAdd(&acc[0], t);
        __threadfence();
        unsigned long long *ticket = reinterpret_cast<unsigned long long *>(&acc[3]);
        if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1ull) {   // every block's sum (and block 0's root area) is in
            __threadfence();
            refit_result(out, atomicAdd(&acc[0], 0.0), acc);
            *ticket = 0ull;
        }
    }
}
void launch_wide_parents(uint32_t n_wide, const DevNodeW *widef, uint32_t *leaf_parent, uint32_t *node_parent, hipStream_t s) {
    k_wide_parents<<<(n_wide + 255) / 256, 256, 0, s>>>(n_wide, widef, leaf_parent, node_parent);
}
// a refit in two or three launches whatever the tree's depth: the batches (their triangles, their nodes' boxes), the crown (the same for the nodes above the batches), and the
// quantised records + cost either inside those (a large tree) or in a launch behind them -> result[0..3] = cost sum, root half-area, start and end stamps (wall_clock64: 100 MHz)
template <bool FOLD> static void launch_refit_sub(const RefitArgs &r, hipStream_t s, uint32_t grid, uint32_t threads, uint32_t batch0, bool first_launch, DevNode4 *wide, double *acc, double *out, const uint32_t *dirty, double *batch_cost) {
    k_refit_sub<FOLD><<<grid, threads, 0, s>>>(batch0, r.sub_batches + 1, r.sub_levels, r.sub_nodes, r.sub_leaves, r.sub_off, r.shade, r.prims_host, r.prims_dev, r.n_prims * (uint32_t)(sizeof(DevPrim) / 4), r.touched, r.leaf_parent,
                                               r.node_parent, r.mark, r.tris, r.widef, reinterpret_cast<unsigned long long *>(r.acc) + 2, first_launch, wide, acc, out, dirty, batch_cost);
}
void launch_refit(const RefitArgs &r, hipStream_t s) {
    // The quantised records and the cost: in the refit's own workgroups for a large tree (config 4's 1.4 M nodes: a refit alone 0.57 -> 0.28 ms, a frame of a moving model
    // 0.67 -> 0.44), in a launch of their own -- a node a thread -- for a small one (config 2's 131 k nodes: folded, a refit alone 0.13 -> 0.19 ms: three nodes' double-precision
    // quantisation in a row per thread of 143 workgroups against one each in 514; among frames the two forms cost the same).  profiles/README.md round 4g
    const uint32_t grid = r.dirty ? r.n_dirty : r.sub_batches;   // (a refit runs the batches that hold a primitive that moved; the crown always)
    if (r.fold) {
        if (grid) launch_refit_sub<true>(r, s, grid, 256, 0u, true, r.wide, r.acc, nullptr, r.dirty, r.batch_cost);
        launch_refit_sub<true>(r, s, 1, r.sub_batches ? 256 : 1024, r.sub_batches, grid == 0, r.wide, r.acc, r.result, nullptr, r.batch_cost);
        return;
    }
    if (grid) launch_refit_sub<false>(r, s, grid, 256, 0u, true, nullptr, nullptr, nullptr, r.dirty, nullptr);
    launch_refit_sub<false>(r, s, 1, 1024, r.sub_batches, grid == 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    k_wide_requant<<<(r.n_wide + 255) / 256, 256, 0, s>>>(r.n_wide, r.widef, r.wide, r.mark, r.acc, r.result);
}
// The refit's work lists, once per tree (host work on the parents read back: the topology never changes).  A node whose subtree has at most kBatchNodes nodes while its parent's
// has more roots a batch subtree; runs of such roots (in index order) are dealt to batches of about kBatchNodes nodes; the nodes above them -- the crown: a few hundred for the
// bench scenes -- are batch `nb`.  The numbering is breadth-first, so a larger index is never above a smaller one: a batch's nodes in descending order are deepest level first.
__global__ __launch_bounds__(256) void k_leaf_prims(uint32_t T, const uint32_t *__restrict__ leaf_gid, const uint32_t *__restrict__ tri_prim, uint32_t *__restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < T) out[p] = tri_prim[leaf_gid[p]];
}
hipError_t refit_lists_build(Lbvh &l, uint32_t T, hipStream_t s) {
    constexpr uint32_t kBatchNodes = 768;
    const std::vector<uint32_t> &levels = l.wide_levels;
    const uint32_t NW = l.n_wide, n_levels = (uint32_t)levels.size() - 1;
    // Everything is made in locals and moved into the tree at the very end: a failure on the way leaves the tree's lists as they were (complete, or absent)
    DevBuf<uint32_t> d_leaf_parent, d_node_parent, d_sub_nodes, d_sub_leaves, d_sub_off;
    HIPQ(d_leaf_parent.ensure(T)); HIPQ(d_node_parent.ensure(NW));   // who holds whom in the 4-wide tree: the marks of a refit go up along it
    launch_wide_parents(NW, l.widef, d_leaf_parent.p, d_node_parent.p, s);
    HIPQ(hipGetLastError());
    std::vector<uint32_t> node_parent(NW), leaf_parent(T);
    HIPQ(hipStreamSynchronize(s));
    HIPQ(hipMemcpy(node_parent.data(), d_node_parent.p, (size_t)NW * 4, hipMemcpyDeviceToHost)); HIPQ(hipMemcpy(leaf_parent.data(), d_leaf_parent.p, (size_t)T * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> size(NW, 1);
    for (uint32_t w = NW; w-- > 1;) size[node_parent[w]] += size[w];
    // batch_of: ~0 = the crown; roots in index order fill batches
    std::vector<uint32_t> batch_of(NW, ~0u);
    uint32_t nb = 0, fill = 0;
    for (uint32_t w = 1; w < NW; w++) {
        if (size[w] > kBatchNodes) continue;                                   // crown
        const uint32_t up = node_parent[w];
        if (size[up] > kBatchNodes) {                                          // a batch root
            if (nb == 0 || fill + size[w] > kBatchNodes + kBatchNodes / 2) { nb++; fill = 0; }
            fill += size[w]; batch_of[w] = nb - 1;
        } else batch_of[w] = batch_of[up];
    }
    const uint32_t nb1 = nb + 1;
    auto slot = [&](uint32_t w) { return batch_of[w] == ~0u ? nb : batch_of[w]; };
    std::vector<uint32_t> off(2 * (size_t)(nb1 + 1) + (size_t)nb1 * (n_levels + 1), 0), sub_nodes(NW), sub_leaves(T);
    {   // node lists: counts -> offsets -> fill from the deepest level up; level offsets within each list
        std::vector<uint32_t> cnt(nb1 + 1, 0);
        for (uint32_t w = 0; w < NW; w++) cnt[slot(w) + 1]++;
        for (uint32_t b = 0; b < nb1; b++) cnt[b + 1] += cnt[b];
        for (uint32_t b = 0; b <= nb1; b++) off[b] = cnt[b];
        std::vector<uint32_t> at(cnt.begin(), cnt.end() - 1);
        uint32_t *lv_off = off.data() + 2 * (size_t)(nb1 + 1);
        for (uint32_t lv = n_levels; lv-- > 0;) {          // deepest level first
            for (uint32_t b = 0; b < nb1; b++) lv_off[(size_t)b * (n_levels + 1) + (n_levels - 1 - lv)] = at[b] - cnt[b];
            for (uint32_t w = levels[lv + 1]; w-- > levels[lv];) sub_nodes[at[slot(w)]++] = w;
        }
        for (uint32_t b = 0; b < nb1; b++) lv_off[(size_t)b * (n_levels + 1) + n_levels] = at[b] - cnt[b];
    }
    {   // leaf lists
        std::vector<uint32_t> cnt(nb1 + 1, 0);
        for (uint32_t p = 0; p < T; p++) cnt[slot(leaf_parent[p]) + 1]++;
        for (uint32_t b = 0; b < nb1; b++) cnt[b + 1] += cnt[b];
        for (uint32_t b = 0; b <= nb1; b++) off[nb1 + 1 + b] = cnt[b];
        std::vector<uint32_t> at(cnt.begin(), cnt.end() - 1);
        for (uint32_t p = 0; p < T; p++) sub_leaves[at[slot(leaf_parent[p])]++] = p;
    }
    std::vector<uint32_t> batch_prim_off, batch_prim_ids;
    {   // which primitives have triangles in which batch (the crown always runs): the leaf's primitive is tri_prim[leaf_gid[p]], gathered on the device
        std::vector<uint32_t> tp(T);
        DevBuf<uint32_t> d_lp;
        HIPQ(d_lp.ensure(T));
        k_leaf_prims<<<(T + 255) / 256, 256, 0, s>>>(T, l.leaf_gid, l.tri_prim, d_lp.p);
        HIPQ(hipMemcpyAsync(tp.data(), d_lp.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));   // (on the kernel's own stream: the context's streams do not wait for the null stream or it for them)
        HIPQ(hipStreamSynchronize(s));
        uint32_t n_prims = 0;
        for (uint32_t g = 0; g < T; g++) n_prims = std::max(n_prims, tp[g] + 1u);
        std::vector<uint32_t> seen(n_prims, 0u);   // seen[primitive] = batch + 1 of the last batch it was listed for (the leaf lists are batch by batch: one pass)
        batch_prim_off.assign(1, 0u);
        for (uint32_t b = 0; b < nb; b++) {
            for (uint32_t i = off[nb1 + 1 + b]; i < off[nb1 + 2 + b]; i++) {
                const uint32_t pr = tp[sub_leaves[i]];
                if (seen[pr] != b + 1u) { seen[pr] = b + 1u; batch_prim_ids.push_back(pr); }
            }
            batch_prim_off.push_back((uint32_t)batch_prim_ids.size());
        }
    }
    HIPQ(d_sub_nodes.ensure(NW)); HIPQ(d_sub_leaves.ensure(T)); HIPQ(d_sub_off.ensure(off.size()));
    HIPQ(hipMemcpy(d_sub_nodes.p, sub_nodes.data(), (size_t)NW * 4, hipMemcpyHostToDevice)); HIPQ(hipMemcpy(d_sub_leaves.p, sub_leaves.data(), (size_t)T * 4, hipMemcpyHostToDevice));
    HIPQ(hipMemcpy(d_sub_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    // all of them exist: the tree takes them (and lets go of what it had)
    l.leaf_parent = std::move(d_leaf_parent); l.node_parent = std::move(d_node_parent);
    l.sub_nodes = std::move(d_sub_nodes); l.sub_leaves = std::move(d_sub_leaves); l.sub_off = std::move(d_sub_off);
    l.batch_prim_off = std::move(batch_prim_off); l.batch_prim_ids = std::move(batch_prim_ids);
    l.sub_batches = nb; l.sub_levels = n_levels;
    if (l.log & 1u) {
        uint32_t crown = 0, big = 0; for (uint32_t w = 0; w < NW; w++) crown += batch_of[w] == ~0u;
        for (uint32_t b = 0; b < nb; b++) big = std::max(big, off[b + 1] - off[b]);
        std::fprintf(stderr, "[art] refit lists: %u nodes in %u levels; %u batches (largest %u nodes), a crown of %u nodes\n", NW, n_levels, nb, big, crown);
    }
    return hipSuccess;
}
// the quantised records (wide; null: leave them) and the cost of the float records as they are: result[0..1] (acc: 4 zeroed doubles of scratch)
void launch_wide_cost(uint32_t n_wide, const DevNodeW *widef, DevNode4 *wide, double *acc, double *result, hipStream_t s) {
    k_wide_requant<<<(n_wide + 255) / 256, 256, 0, s>>>(n_wide, widef, wide, nullptr, acc, result);
}
// art_scene_set_vertices_device: a primitive's new vertices from the caller's device buffer into its own slot of the build's vertex array (48-byte records, the slot
// 16-byte aligned), on the caller's stream -- the one read of that buffer.  A streaming copy: a grid-stride loop over at most kIngestBlocks workgroups (four of 256
// threads a CU of 256), plain stores (the refit's gather reads the slot next, from whichever XCD).
//   FULL      three 16-byte loads and stores a vertex, lane after lane: fully coalesced
//   POSITIONS lane i reads three dwords at src + i * stride and writes words 0-2 of vertex i: one 12-byte load and one 12-byte store a lane (a 16-byte load for
//             strides and pointers that allow it compiles to the same 12-byte one: the fourth word is dead).  Words 3-11 (uv, normal, tangent) are not touched.
constexpr uint32_t kIngestBlocks = 1024;
enum IngestForm { kIngestFull = 0, kIngestPositions = 1 };
template <int FORM> __global__ __launch_bounds__(256) void k_ingest_verts(const float *__restrict__ src, uint32_t stride_words, float *__restrict__ dst, uint32_t n_verts) {
    if (FORM == kIngestFull) {
        const float4 *from = reinterpret_cast<const float4 *>(src); float4 *to = reinterpret_cast<float4 *>(dst);
        const uint64_t n_quads = 3ull * n_verts;
        for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n_quads; i += gridDim.x * 256u) to[i] = from[i];
        return;
    }
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_verts; i += gridDim.x * 256u) {
        const float *from = src + (size_t)i * stride_words;
        const float x = from[0], y = from[1], z = from[2];
        float *to = static_cast<float *>(__builtin_assume_aligned(dst + (size_t)i * 12, 16));
        to[0] = x; to[1] = y; to[2] = z;
    }
}
void launch_ingest_verts(const void *src, uint32_t stride_bytes /*0: whole 48-byte vertices*/, float *slot, uint32_t n_verts, hipStream_t s) {
    if (n_verts == 0) return;
    const uint64_t items = stride_bytes ? n_verts : 3ull * n_verts;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((items + 255) / 256, kIngestBlocks), sw = stride_bytes / 4;
    const float *from = static_cast<const float *>(src);
    if (!stride_bytes) k_ingest_verts<kIngestFull><<<grid, 256, 0, s>>>(from, 12u, slot, n_verts);
    else k_ingest_verts<kIngestPositions><<<grid, 256, 0, s>>>(from, sw, slot, n_verts);
}
__global__ void k_refit_noop() {}
void refit_prewarm(hipStream_t s) { k_refit_noop<<<1, 1, 0, s>>>(); }   // build_prewarm's empty launch from this unit

} // namespace art
