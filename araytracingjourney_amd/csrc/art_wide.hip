// art_wide.hip -- the 4-wide collapse + 8-bit quantisation of the binary tree the walks use (gfx950; once per scene, on first use), twice: one host thread (wide_build_host, the
// form the device one is tested against) and level by level on the device (k_wide_expand -> scan -> k_wide_emit).  Two hands wrote the two: they share ceil_log2 and nothing else.
// Greedy collapse: start from a binary node's two children and keep replacing the internal candidate with the largest
// surface area by its own two children until there are four (or only leaves are left).
#include "art_records.h"
#include <rocprim/rocprim.hpp>

namespace art {
namespace {
struct BoxRef { const float *lo, *hi; };
inline float half_area(const float *lo, const float *hi) {
    float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return dx * dy + dy * dz + dz * dx;
}
} // namespace
// the collapse on the host, one thread (ArtTuning.wide_builder = 1; what round 1 shipped): the reference the device collapse below is tested against
static hipError_t wide_build_host(Lbvh &l, uint32_t T, hipStream_t s) {
    if (l.wide) return hipSuccess; // already built for this tree
    const uint32_t NI = T > 1 ? T - 1 : 0;
    std::vector<int32_t> child(NI ? (size_t)NI * 2 : 2);
    std::vector<float> nlo(NI ? (size_t)NI * 3 : 3), nhi(NI ? (size_t)NI * 3 : 3), llo((size_t)T * 3), lhi((size_t)T * 3);
    HIPQ(hipStreamSynchronize(s));
    if (NI) {
        const WalkTree w = l.walk_tree(); // collapse the tree the binary walks use
        HIPQ(hipMemcpy(child.data(), w.child, (size_t)NI * 8, hipMemcpyDeviceToHost));
        HIPQ(hipMemcpy(nlo.data(), w.lo, (size_t)NI * 12, hipMemcpyDeviceToHost));
        HIPQ(hipMemcpy(nhi.data(), w.hi, (size_t)NI * 12, hipMemcpyDeviceToHost));
    }
    HIPQ(hipMemcpy(llo.data(), l.leaf_lo, (size_t)T * 12, hipMemcpyDeviceToHost));
    HIPQ(hipMemcpy(lhi.data(), l.leaf_hi, (size_t)T * 12, hipMemcpyDeviceToHost));
    auto box = [&](int32_t ref) -> BoxRef {
        if (ref < 0) return BoxRef{llo.data() + 3 * (size_t)(~ref), lhi.data() + 3 * (size_t)(~ref)};
        return BoxRef{nlo.data() + 3 * (size_t)ref, nhi.data() + 3 * (size_t)ref};
    };
    std::vector<DevNode4> wide;
    std::vector<DevNodeW> widef;
    std::vector<int32_t> todo; // binary node behind each wide node, in wide-index order (BFS)
    wide.reserve(NI / 2 + 2);
    if (NI == 0) todo.push_back(~0); // single triangle: a root with one leaf child
    else todo.push_back(0);
    std::vector<uint32_t> levels; size_t level_end = 0; // breadth-first: the nodes of a level are contiguous
    for (size_t w = 0; w < todo.size(); w++) {
        if (w == level_end) { levels.push_back((uint32_t)w); level_end = todo.size(); }
        int32_t cand[4]; int nc = 0;
        if (todo[w] < 0) { cand[nc++] = todo[w]; }
        else {
            cand[nc++] = child[2 * (size_t)todo[w]]; cand[nc++] = child[2 * (size_t)todo[w] + 1];
            while (nc < 4) {
                int best = -1; float ba = -1.0f;
                for (int i = 0; i < nc; i++)
                    if (cand[i] >= 0) { BoxRef b = box(cand[i]); float a = half_area(b.lo, b.hi); if (a > ba) { ba = a; best = i; } }
                if (best < 0) break;
                int32_t n = cand[best];
                cand[best] = child[2 * (size_t)n];
                cand[nc++] = child[2 * (size_t)n + 1];
            }
        }
        // the packet walk takes the children front to back along ONE axis (0,1,2,3 or 3,2,1,0 by the rays' direction sign on it): sort them by box
        // centre along the axis the centres spread most on
        uint32_t sort_axis = 0;
        {
            float best_spread = -1.0f;
            for (uint32_t k = 0; k < 3; k++) {
                float lo = INFINITY, hi = -INFINITY;
                for (int i = 0; i < nc; i++) { BoxRef b = box(cand[i]); float c = 0.5f * b.lo[k] + 0.5f * b.hi[k]; lo = std::fmin(lo, c); hi = std::fmax(hi, c); }
                if (hi - lo > best_spread) { best_spread = hi - lo; sort_axis = k; }
            }
            auto centre = [&](int32_t ref) { BoxRef b = box(ref); return 0.5f * b.lo[sort_axis] + 0.5f * b.hi[sort_axis]; };
            std::stable_sort(cand, cand + nc, [&](int32_t x, int32_t y) { return centre(x) < centre(y); });
        }
        DevNode4 d; std::memset(&d, 0, sizeof(d));
        DevNodeW dw; std::memset(&dw, 0, sizeof(dw));
        float org[3] = {INFINITY, INFINITY, INFINITY}, top[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < nc; i++) { BoxRef b = box(cand[i]); for (int k = 0; k < 3; k++) { org[k] = std::fmin(org[k], b.lo[k]); top[k] = std::fmax(top[k], b.hi[k]); } }
        d.ox = org[0]; d.oy = org[1]; d.oz = org[2];
        uint32_t ebits[3]; float scale[3];
        for (int k = 0; k < 3; k++) {
            // smallest power of two with 255 * scale >= extent (as evaluated by the device's fma), at least 2^-100
            double ext = (double)top[k] - (double)org[k];
            int e = ext > 0 ? ceil_log2(ext / 255.0) : -100;
            if (e < -100) e = -100;
            for (;;) { scale[k] = std::ldexp(1.0f, e); if (std::fmaf(255.0f, scale[k], org[k]) >= top[k]) break; e++; }
            while (e > -100 && std::fmaf(255.0f, std::ldexp(1.0f, e - 1), org[k]) >= top[k]) { e--; scale[k] = std::ldexp(1.0f, e); }   // (... or down, where the fma rounds the last plane of half the scale up onto the top)
            ebits[k] = (uint32_t)(e + 127);
        }
        uint32_t mask = 0;
        for (int i = 0; i < 4; i++) {
            if (i >= nc) { d.child[i] = kAbsentChild; dw.child[i] = kAbsentChild; for (int k = 0; k < 3; k++) { dw.box[i][k] = 3.0e38f; dw.box[i][3 + k] = 3.0e38f; d.q[k] |= 255u << (8 * i); } continue; } // an absent child: its quantised box is INVERTED (lo planes 255, hi planes 0: the per-ray walk's sign-selected slab enters it after it has left it, whatever the direction); its float box a point box out at 3e38 -- every axis' entry
            // and exit distance is +-huge with the SAME sign, so neither the octant-specialised nor the general slab test lets a finite ray in (an INVERTED box passes the general one);
            // its reference is the walks' "pop" value, so a ray that passes every box (NaN: fminf / fmaxf drop a NaN operand) still cannot leave the node array
            mask |= 1u << i;
            BoxRef b = box(cand[i]);
            for (int k = 0; k < 3; k++) {
                int ql = (int)std::floor(((double)b.lo[k] - (double)org[k]) / (double)scale[k]);
                int qh = (int)std::ceil(((double)b.hi[k] - (double)org[k]) / (double)scale[k]);
                ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql); qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
                while (ql > 0 && std::fmaf((float)ql, scale[k], org[k]) > b.lo[k]) ql--;   // taken only where the float64 difference above itself rounded (places more than 53 bits apart: tests/test_wide_tree.py, "exponent steps")
                while (qh < 255 && std::fmaf((float)qh, scale[k], org[k]) < b.hi[k]) qh++;
                // ... and inwards where the fma rounds the next plane exactly onto the box (a value that differs only: a flat box keeps lo plane <= hi plane)
                while (ql < 255 && std::fmaf((float)(ql + 1), scale[k], org[k]) <= b.lo[k] && std::fmaf((float)(ql + 1), scale[k], org[k]) > std::fmaf((float)ql, scale[k], org[k])) ql++;
                while (qh > 0 && std::fmaf((float)(qh - 1), scale[k], org[k]) >= b.hi[k] && std::fmaf((float)(qh - 1), scale[k], org[k]) < std::fmaf((float)qh, scale[k], org[k])) qh--;
                d.q[k] |= (uint32_t)ql << (8 * i);
                d.q[3 + k] |= (uint32_t)qh << (8 * i);
            }
            for (int k = 0; k < 3; k++) { dw.box[i][k] = b.lo[k]; dw.box[i][3 + k] = b.hi[k]; }
            if (cand[i] < 0) d.child[i] = cand[i];
            else { d.child[i] = (int32_t)todo.size(); todo.push_back(cand[i]); }
            dw.child[i] = d.child[i];
        }
        d.exps = ebits[0] | (ebits[1] << 8) | (ebits[2] << 16) | (mask << 24);
        dw.valid = mask; dw.pad[0] = sort_axis;
        wide.push_back(d);
        widef.push_back(dw);
    }
    l.n_wide = (uint32_t)wide.size();
    levels.push_back(l.n_wide); l.wide_levels = levels;
    DevBuf<DevNode4> d_wide; DevBuf<DevNodeW> d_widef;   // both records or neither: the tree takes them at the end
    HIPQ(d_wide.ensure(wide.size()));
    HIPQ(hipMemcpy(d_wide.p, wide.data(), wide.size() * sizeof(DevNode4), hipMemcpyHostToDevice));
    HIPQ(d_widef.ensure(widef.size()));
    HIPQ(hipMemcpy(d_widef.p, widef.data(), widef.size() * sizeof(DevNodeW), hipMemcpyHostToDevice));
    l.wide = std::move(d_wide); l.widef = std::move(d_widef);
    return hipSuccess;
}

// ---- the same collapse on the device, level by level -------------------------------------------------------------------------------------------
// A wide node is a binary node whose two children are expanded greedily (largest half-area first) to at most four.  Level L's wide nodes are the
// internal children of level L-1's, in order: the index of a child is (first index of its level) + (exclusive scan of the internal-children counts),
// which is exactly the breadth-first numbering the host loop produces -- the two builders emit the same arrays, bit for bit.
struct WideIn { const int32_t *child; const float *nlo, *nhi, *llo, *lhi; };
__device__ inline void wide_box(const WideIn &in, int32_t ref, const float *&lo, const float *&hi) { child_box(ref, in.llo, in.lhi, in.nlo, in.nhi, lo, hi); }
// pass 1: the (sorted) children of every wide node of the level, and how many of them are internal
__global__ __launch_bounds__(256) void k_wide_expand(WideIn in, const int32_t *__restrict__ front, uint32_t n, int32_t *__restrict__ cand_out /*4 per node*/,
                                                     uint32_t *__restrict__ meta /*nc | axis << 8*/, uint32_t *__restrict__ n_internal) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    int32_t cand[4] = {kAbsentChild, kAbsentChild, kAbsentChild, kAbsentChild}; int nc = 0;
    const int32_t root = front[w];
    if (root < 0) cand[nc++] = root; // single triangle: a root with one leaf child
    else {
        cand[nc++] = in.child[2 * (size_t)root]; cand[nc++] = in.child[2 * (size_t)root + 1];
        while (nc < 4) {
            int best = -1; float ba = -1.0f;
            for (int i = 0; i < nc; i++)
                if (cand[i] >= 0) { const float *lo, *hi; wide_box(in, cand[i], lo, hi); float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2]; float a = dx * dy + dy * dz + dz * dx; if (a > ba) { ba = a; best = i; } }
            if (best < 0) break;
            int32_t nn = cand[best];
            cand[best] = in.child[2 * (size_t)nn];
            cand[nc++] = in.child[2 * (size_t)nn + 1];
        }
    }
    uint32_t sort_axis = 0; float best_spread = -1.0f;
    float cen[3][4];
    for (uint32_t k = 0; k < 3; k++) {
        float lo_c = INFINITY, hi_c = -INFINITY;
        for (int i = 0; i < nc; i++) { const float *lo, *hi; wide_box(in, cand[i], lo, hi); float c = 0.5f * lo[k] + 0.5f * hi[k]; cen[k][i] = c; lo_c = fminf(lo_c, c); hi_c = fmaxf(hi_c, c); }
        if (hi_c - lo_c > best_spread) { best_spread = hi_c - lo_c; sort_axis = k; }
    }
    float key[4];
    for (int i = 0; i < nc; i++) key[i] = sort_axis == 0 ? cen[0][i] : (sort_axis == 1 ? cen[1][i] : cen[2][i]);
    for (int i = 1; i < nc; i++) // stable insertion sort by centre (std::stable_sort's order)
        for (int j = i; j > 0 && key[j] < key[j - 1]; j--) { float tk = key[j]; key[j] = key[j - 1]; key[j - 1] = tk; int32_t tc = cand[j]; cand[j] = cand[j - 1]; cand[j - 1] = tc; }
    uint32_t ni = 0;
    for (int i = 0; i < nc; i++) ni += cand[i] >= 0;
    for (int i = 0; i < 4; i++) cand_out[4 * (size_t)w + i] = cand[i];
    meta[w] = (uint32_t)nc | (sort_axis << 8);
    n_internal[w] = ni;
}
// pass 2: the two node records of every wide node of the level; its internal children become the next level's wide nodes
__global__ __launch_bounds__(256) void k_wide_emit(WideIn in, uint32_t n, uint32_t first /*wide index of this level's first node*/, const int32_t *__restrict__ cand_in,
                                                   const uint32_t *__restrict__ meta, const uint32_t *__restrict__ offs, DevNode4 *__restrict__ wide,
                                                   DevNodeW *__restrict__ widef, int32_t *__restrict__ next_front) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const int nc = (int)(meta[w] & 255u); const uint32_t sort_axis = meta[w] >> 8;
    int32_t cand[4];
    for (int i = 0; i < 4; i++) cand[i] = cand_in[4 * (size_t)w + i];
    DevNode4 d; DevNodeW dw;
    dw.pad[1] = dw.pad[2] = 0;
    const float *lo[4] = {nullptr, nullptr, nullptr, nullptr}, *hi[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < nc; i++) wide_box(in, cand[i], lo[i], hi[i]);
    wide_quantise(lo, hi, nc, d);
    uint32_t next = first + n + offs[w]; // this node's internal children follow those of the nodes before it
    for (int i = 0; i < 4; i++) {
        if (i >= nc) { d.child[i] = kAbsentChild; dw.child[i] = kAbsentChild; for (int k = 0; k < 3; k++) { dw.box[i][k] = 3.0e38f; dw.box[i][3 + k] = 3.0e38f; } continue; }
        for (int k = 0; k < 3; k++) { dw.box[i][k] = lo[i][k]; dw.box[i][3 + k] = hi[i][k]; }
        if (cand[i] < 0) d.child[i] = cand[i];
        else { d.child[i] = (int32_t)next; next_front[next - (first + n)] = cand[i]; next++; }
        dw.child[i] = d.child[i];
    }
    dw.valid = d.exps >> 24; dw.pad[0] = sort_axis;
    wide[first + w] = d;
    widef[first + w] = dw;
}

hipError_t wide_build(Lbvh &l, uint32_t T, hipStream_t s, bool on_host) {
    if (l.wide) return hipSuccess; // already built for this tree
    if (on_host) return wide_build_host(l, T, s);
    const uint32_t NI = T > 1 ? T - 1 : 0;
    const uint32_t cap = NI ? NI : 1;   // a wide node stands on a distinct binary node: at most NI of them (one for a single triangle)
    const WalkTree wt = l.walk_tree();
    WideIn in{wt.child, wt.lo, wt.hi, l.leaf_lo, l.leaf_hi};
    int32_t *front[2] = {nullptr, nullptr}, *cand = nullptr; uint32_t *meta = nullptr, *cnt = nullptr, *offs = nullptr; void *tmp = nullptr; size_t tmp_bytes = 0;
    DevNode4 *wide = nullptr; DevNodeW *widef = nullptr;
    std::vector<uint32_t> levels; // first node of every level (breadth-first numbering: a level is contiguous), then n_wide
    Arena own; Arena &A = l.arena ? *l.arena : own;
    HIPQ(rocprim::exclusive_scan(nullptr, tmp_bytes, cnt, offs, 0u, (size_t)cap + 1, rocprim::plus<uint32_t>(), s));
    HIPQ(A.reserve(3 * Arena::pad((size_t)cap * 4) + Arena::pad((size_t)cap * 16) + 2 * Arena::pad(((size_t)cap + 1) * 4) + Arena::pad((size_t)cap * sizeof(DevNode4)) + Arena::pad((size_t)cap * sizeof(DevNodeW)) + Arena::pad(tmp_bytes ? tmp_bytes : 16)));
    front[0] = A.take<int32_t>(cap); front[1] = A.take<int32_t>(cap); cand = A.take<int32_t>((size_t)cap * 4);
    meta = A.take<uint32_t>(cap); cnt = A.take<uint32_t>((size_t)cap + 1); offs = A.take<uint32_t>((size_t)cap + 1);
    wide = A.take<DevNode4>(cap); widef = A.take<DevNodeW>(cap);
    tmp = A.take<char>(tmp_bytes ? tmp_bytes : 16);
    const int32_t root = NI ? 0 : ~0;
    HIPQ(hipMemcpyAsync(front[0], &root, 4, hipMemcpyHostToDevice, s));
    uint32_t first = 0, n = 1; int cur = 0;
    while (n) {
        if (first + n > cap) return hipErrorInvalidValue; // (cannot happen: see cap)
        const uint32_t g = (n + 255) / 256;
        k_wide_expand<<<g, 256, 0, s>>>(in, front[cur], n, cand, meta, cnt);
        HIPQ(hipMemsetAsync(cnt + n, 0, 4, s));                                  // the scan's last element = the level's total
        size_t tb = tmp_bytes;
        HIPQ(rocprim::exclusive_scan(tmp, tb, cnt, offs, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), s));
        k_wide_emit<<<g, 256, 0, s>>>(in, n, first, cand, meta, offs, wide, widef, front[cur ^ 1]);
        uint32_t n_next = 0;
        HIPQ(hipMemcpyAsync(&n_next, offs + n, 4, hipMemcpyDeviceToHost, s));
        HIPQ(hipStreamSynchronize(s));
        levels.push_back(first);
        first += n; n = n_next; cur ^= 1;
    }
    HIPQ(hipGetLastError());
    levels.push_back(first);
    // the work arrays are sized for the worst case (NI nodes); a 4-wide collapse of a binary tree has about a third of that.  Both records or neither: the tree takes them at the end
    const uint32_t n_wide = levels.back();
    DevBuf<DevNode4> d_wide; DevBuf<DevNodeW> d_widef;
    HIPQ(d_wide.ensure(n_wide)); HIPQ(d_widef.ensure(n_wide));
    HIPQ(hipMemcpyAsync(d_wide.p, wide, (size_t)n_wide * sizeof(DevNode4), hipMemcpyDeviceToDevice, s));
    HIPQ(hipMemcpyAsync(d_widef.p, widef, (size_t)n_wide * sizeof(DevNodeW), hipMemcpyDeviceToDevice, s));
    HIPQ(hipStreamSynchronize(s));
    l.wide = std::move(d_wide); l.widef = std::move(d_widef); l.n_wide = n_wide; l.wide_levels = levels;
    return hipSuccess;
}
__global__ void k_wide_noop() {}
void wide_prewarm(hipStream_t s) { k_wide_noop<<<1, 1, 0, s>>>(); }   // build_prewarm's empty launch from this unit

} // namespace art
