// art_plan.hip -- the host side of the fused frame's wave plan (WavePlan, art_context.h; k_plan, art_frame.hip): which wave of a launch traces what, when a frame is
// sampled and when the table its plan wrote is adopted.  Every write of a WavePlan field is in this file.
#include "art_context.h"
#include <cstdio>
#include <cstring>

// ---- wave plan of the fused frame ----------------------------------------------------------------------------------------------------
// the first table of a frame layout: every 8x8 block one wave, in the XCD-aware launch order (k_plan writes the later ones in the same layout)
static void plan_first_items(const WavePlan &P, uint32_t n64, std::vector<uint2> &out) {
    out.clear();
    for (uint32_t blk : P.order)
        for (uint32_t w = 0; w < 4; w++) out.push_back(make_uint2(blk * 4 + w, 0xFFFFu));
    (void)n64;
    // k_frame runs one wave per workgroup, and workgroup j lands on XCD j % 8 (round-robin dispatch): deal the items so that the four waves of launch
    // block 8g + x (a 256-pixel block the XCD-aware order gave to XCD x) stay on XCD x -- positions 32g + 8k + x, k = 0..3.  A permutation whatever the
    // hardware does; only the L2 locality depends on it.
    std::vector<uint2> q(out);
    for (size_t g = 0; (g + 1) * 32 <= out.size(); g++)
        for (uint32_t x = 0; x < 8; x++) for (uint32_t k = 0; k < 4; k++) q[g * 32 + 8 * k + x] = out[g * 32 + 4 * x + k];
    out.swap(q);
}
int32_t art::plan_reset(ArtContext *c, const std::vector<uint32_t> &order) {
    WavePlan &P = c->plan;
    P.order = order;
    const ArtTuning &t = c->tuning;
    P.enabled = !t.fixed_waves && !(c->cfg.flags & ART_FLAG_FIXED_WAVES);
    P.min_steps = t.split_min_steps ? t.split_min_steps : 150;
    P.fixed_steps = t.split_fixed_steps;
    P.alpha = t.split_alpha > 0.f ? t.split_alpha : 0.7f;
    const uint32_t hwq = t.hw_queues ? t.hw_queues : 4;   // HIP's default number of hardware queues per process; a host that raises GPU_MAX_HW_QUEUES says so in ArtTuning
    // (at most 4: a ring of 8 hides a straggler while it stays full, but a run's last frames drain without neighbours -- over the driver's 20 steps a plan made for 3-4 launches
    //  in flight is worth 4 %, over 1 000 steps it costs 1 %: profiles/README.md round 4)
    P.in_flight = std::max(1u, std::min(std::min(c->F, hwq), 4u));
    const uint32_t n64 = c->n_local / 64;
    P.cap = n64 + n64 / 2 + 64;       // at most half as many waves again
    std::vector<uint2> first;
    plan_first_items(P, n64, first);
    for (int i = 0; i < 2; i++) { HIPC(P.d_items[i].ensure(P.cap)); P.n_items[i] = 0; P.retire_set[i] = false; }
    if (!first.empty()) HIPC(hipMemcpy(P.d_items[0].p, first.data(), first.size() * sizeof(uint2), hipMemcpyHostToDevice));
    P.n_items[0] = (uint32_t)first.size(); P.cur = 0; P.split1 = P.split2 = 0;
    HIPC(P.d_level.ensure(n64 ? n64 : 1)); HIPC(P.d_level_tmp.ensure(n64 ? n64 : 1)); HIPC(P.d_worst.ensure(n64 ? n64 : 1));
    HIPC(hipMemset(P.d_level.p, 0, n64 ? n64 : 1)); HIPC(hipMemset(P.d_worst.p, 0, (size_t)(n64 ? n64 : 1) * 4));
    HIPC(P.result.ensure(8));
    std::memset(P.result.p, 0, 32);
    HIPC(P.cost_ready.create(hipEventDisableTiming));
    if (!P.plan_stream) { int lo = 0, hi = 0; HIPC(hipDeviceGetStreamPriorityRange(&lo, &hi)); HIPC(P.plan_stream.create(lo)); }   // (the least urgent: nothing waits for it)
    else HIPC(hipStreamSynchronize(P.plan_stream));
    P.pending = false; P.next_sample = c->frame_no; P.interval = 1; P.replans = 0; P.last_sample = c->frame_no;
    return ART_OK;
}
// the table the current one alternates with: free once every launch that read it has finished (the events recorded on all frame streams when it was left)
static bool plan_other_free(ArtContext *c) {
    WavePlan &P = c->plan;
    const int other = P.cur ^ 1;
    if (!P.retire_set[other]) return true;
    for (uint32_t k = 0; k < c->F; k++) if (hipEventQuery(P.retire[other][k]) != hipSuccess) return false;
    return true;
}
// the frame about to be launched counts its waves' steps: the plan's cadence says so (or art_sample_wave_steps), no sample is in flight and there is a table to write
bool art::plan_want_sample(ArtContext *c, uint32_t n_wave_items) {
    const WavePlan &P = c->plan;
    return ((P.enabled && c->frame_no >= P.next_sample) || c->force_sample) && !P.pending && n_wave_items && plan_other_free(c);
}
// behind a sampled frame, on its stream: the next plan from what its waves counted (k_plan writes the other table if a level changed that matters)
int32_t art::plan_launch(ArtContext *c, const FrameArgs &a, hipEvent_t frame_done) {
    WavePlan &P = c->plan;
    hipStream_t s = P.plan_stream;
    HIPC(hipStreamWaitEvent(s, frame_done, 0));   // (a wait in the PLAN's stream: the frames' streams see nothing of it)
    PlanArgs pa{};
    pa.items_in = P.d_items[P.cur].p; pa.n_items_in = a.n_wave_items; pa.cost = a.wave_cost;
    pa.level = P.d_level.p; pa.level_tmp = P.d_level_tmp.p; pa.n64 = c->n_local / 64; pa.worst = P.d_worst.p;
    pa.order = c->d_block_order.p; pa.n256 = c->n_local / 256;
    pa.items_out = P.d_items[P.cur ^ 1].p; pa.cap = P.cap;
    constexpr float kWaveSlots = 256.0f * 32.0f; // CUs x waves per CU
    pa.share = P.alpha * (float)c->B * (float)P.in_flight / kWaveSlots;   // (the counts are one frame's; a launch traces B frames)
    pa.min_steps = P.min_steps; pa.fixed_steps = P.fixed_steps; pa.result = P.result.d;
    launch_plan(pa, s);
    HIPC(hipEventRecord(P.cost_ready, s));
    P.pending = true; P.pending_table = P.cur; P.last_sample = c->frame_no;
    return ART_OK;
}
// The view or the lights changed: the heavy blocks are elsewhere, sooner or later.  The plan in use stays (a camera that moves like the reference's -- 0.002 units per
// millisecond, main.rs:80-105 -- shifts them by a fraction of a pixel a frame) and the waves are looked at again within kMovingInterval frames of the last look: a camera
// that moves every frame is sampled at that cadence, not at every frame (round 3 reset the interval to 1 here: every frame that found no sample in flight was a counting
// frame and every other poll a new table).
constexpr uint32_t kMovingInterval = 32;
static uint32_t plan_moving_interval(const ArtContext *c) { return c->tuning.plan_moving_interval ? c->tuning.plan_moving_interval : kMovingInterval; }
void art::plan_hint_moved(ArtContext *c) {
    WavePlan &P = c->plan;
    const uint32_t mi = plan_moving_interval(c);
    P.interval = std::min(P.interval, mi);
    P.next_sample = std::min<uint64_t>(P.next_sample, P.last_sample + mi);
    P.moved_since_poll = true;
}

// A sampled frame's plan has been made: if it wrote a new table, that one becomes the current one (the table being left stays in use until every frame stream has passed this point).
int32_t art::plan_poll(ArtContext *c) {
    WavePlan &P = c->plan;
    if (!P.pending || hipEventQuery(P.cost_ready) != hipSuccess) return ART_OK;
    P.pending = false;
    const uint32_t *res = P.result.p;
    const int verbose = (c->tuning.log & 4u) ? 2 : ((c->tuning.log & 2u) ? 1 : 0);
    if (verbose > 1) std::fprintf(stderr, "[art] plan poll at frame %llu: table %d sampled, %s, slowest wave %u steps, target %u, interval %u\n", (unsigned long long)c->frame_no, P.pending_table, res[1] ? "a new table" : "the table stays", res[5], res[4], P.interval);
    if (res[1]) {
        for (uint32_t k = 0; k < c->F; k++) {
            HIPC(P.retire[P.cur][k].create(hipEventDisableTiming));
            HIPC(hipEventRecord(P.retire[P.cur][k], c->stream_of(k)));
        }
        P.retire_set[P.cur] = true;
        P.cur ^= 1; P.n_items[P.cur] = res[0]; P.split1 = res[2]; P.split2 = res[3]; P.replans++;
        if (verbose) std::fprintf(stderr, "[art] wave plan %u at frame %llu: %u blocks in 4, %u in 16, of %u; slowest sampled wave %u steps, target %u\n", P.replans, (unsigned long long)c->frame_no, res[2], res[3], c->n_local / 64, res[5], res[4]);
        P.interval = P.moved_since_poll ? plan_moving_interval(c) : c->F + 1;        // a still view: let frames of the new plan come back, then judge it; a moving one: at its cadence
    } else P.interval = P.interval < 128 ? P.interval * 2 : 256;
    P.moved_since_poll = false;
    P.next_sample = c->frame_no + P.interval;
    return ART_OK;
}
// a new scene: the heavy blocks are elsewhere
void art::plan_hint_built(ArtContext *c) { c->plan.next_sample = c->frame_no; c->plan.interval = 1; }
// a plan behind a sampled frame: the frames first (k_plan waits for the sampled one), then the plan's stream
int32_t art::plan_sync(ArtContext *c) {
    const WavePlan &P = c->plan;
    if (P.plan_stream && P.pending) { for (uint32_t k = 0; k < c->F; k++) HIPC(hipStreamSynchronize(c->stream_of(k))); HIPC(hipStreamSynchronize(P.plan_stream)); }
    return ART_OK;
}
// the ring starts again at frame 0.  Everything is synchronised, so a sample in flight has landed: its table is adopted like any other (k_plan committed the levels with
// it; dropping the result would leave them a table ahead of the host)
int32_t art::plan_rewind(ArtContext *c) {
    int32_t r = plan_poll(c); if (r) return r;
    c->plan.next_sample = 0; c->plan.pending = false; c->plan.last_sample = 0;
    return ART_OK;
}

extern "C" {

int32_t art_sample_wave_steps(ArtContext *c, uint32_t *items, uint32_t *steps, uint32_t cap, uint32_t *n) {
    if (!c || !n) return fail(ART_E_INVALID, "art_sample_wave_steps: null argument");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    if (c->frame_ready) { r = plan_poll(c); if (r) return r; }   // a plan that has landed takes effect first
    if (c->plan.pending) return fail(ART_E_STATE, "art_sample_wave_steps: a sample is still in flight");
    c->force_sample = true;
    r = art_trace(c);
    c->force_sample = false;
    if (r) return r;
    r = sync_all(c); if (r) return r;
    WavePlan &P = c->plan;
    if (!P.pending) return fail(ART_E_STATE, "art_sample_wave_steps: this context's frames are not the fused frame (no step counts)");
    *n = P.n_items[P.pending_table];
    const uint32_t m = std::min(*n, cap);
    if (items && m) HIPC(hipMemcpy(items, P.d_items[P.pending_table].p, (size_t)m * 8, hipMemcpyDeviceToHost));
    if (steps && m) HIPC(hipMemcpy(steps, c->slot[c->last].d_wave_cost.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    if (!P.enabled) {   // nobody polls a plan that is switched off (k_plan ran all the same: its table is not adopted)
        P.pending = false;
        // ... and k_plan commits the levels together with the table it writes: a switched-off plan runs the first table for as long as its layout lives, all blocks level 0
        if (P.result.p[1]) { HIPC(hipMemset(P.d_level.p, 0, P.d_level.n)); HIPC(hipDeviceSynchronize()); }
    }
    return ART_OK;
}

// k_plan on made-up buffers (include/art_parity.h): every index the kernel makes from its inputs is checked here first
int32_t art_parity_plan(ArtContext *c, uint32_t n256, const uint32_t *order, const uint32_t *items_in, uint32_t n_items_in, const uint32_t *cost, const uint8_t *level_in,
                        const uint32_t *worst_in, uint32_t cap, float share, uint32_t min_steps, uint32_t fixed_steps, uint32_t *items_out, uint8_t *level_out,
                        uint32_t *worst_out, uint32_t result[8]) {
    if (!c || !order || !level_in || !worst_in || !items_out || !level_out || !worst_out || !result || (n_items_in && (!items_in || !cost)))
        return fail(ART_E_INVALID, "art_parity_plan: null argument");
    if (n256 < 1 || n256 > (1u << 16) || n_items_in > (1u << 22) || cap < 1 || cap > (1u << 22)) return fail(ART_E_INVALID, "art_parity_plan: n256 1..2^16, at most 2^22 items, cap 1..2^22");
    const uint32_t n64 = 4 * n256;
    std::vector<uint8_t> seen(n256, 0);
    for (uint32_t i = 0; i < n256; i++) { if (order[i] >= n256 || seen[order[i]]) return fail(ART_E_INVALID, "art_parity_plan: order is not a permutation of the 256-pixel blocks"); seen[order[i]] = 1; }
    for (uint32_t i = 0; i < n_items_in; i++) if (items_in[2 * i] >= n64) return fail(ART_E_INVALID, "art_parity_plan: an item's block is not below n64");
    for (uint32_t b = 0; b < n64; b++) if (level_in[b] > 2) return fail(ART_E_INVALID, "art_parity_plan: a level above 2");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    DevBuf<uint2> d_in, d_out; DevBuf<uint32_t> d_cost, d_worst, d_order; DevBuf<uint8_t> d_level, d_tmp; Pinned<uint32_t> res;
    HIPC(d_in.ensure(n_items_in)); HIPC(d_cost.ensure(n_items_in)); HIPC(d_out.ensure(cap)); HIPC(d_worst.ensure(n64)); HIPC(d_order.ensure(n256));
    HIPC(d_level.ensure(n64)); HIPC(d_tmp.ensure(n64)); HIPC(res.ensure(8));
    if (n_items_in) { HIPC(hipMemcpy(d_in.p, items_in, (size_t)n_items_in * 8, hipMemcpyHostToDevice)); HIPC(hipMemcpy(d_cost.p, cost, (size_t)n_items_in * 4, hipMemcpyHostToDevice)); }
    HIPC(hipMemcpy(d_order.p, order, (size_t)n256 * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_level.p, level_in, n64, hipMemcpyHostToDevice)); HIPC(hipMemcpy(d_worst.p, worst_in, (size_t)n64 * 4, hipMemcpyHostToDevice));
    HIPC(hipMemset(d_out.p, 0xFF, (size_t)cap * 8)); HIPC(hipMemset(d_tmp.p, 0xFF, n64));
    std::memcpy(res.p, result, 32);
    HIPC(hipDeviceSynchronize());   // (the copies and clears above ran on the null stream)
    PlanArgs pa{};
    pa.items_in = d_in.p; pa.n_items_in = n_items_in; pa.cost = d_cost.p;
    pa.level = d_level.p; pa.level_tmp = d_tmp.p; pa.n64 = n64; pa.worst = d_worst.p;
    pa.order = d_order.p; pa.n256 = n256; pa.items_out = d_out.p; pa.cap = cap;
    pa.share = share; pa.min_steps = min_steps; pa.fixed_steps = fixed_steps; pa.result = res.d;
    launch_plan(pa, nullptr); HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(items_out, d_out.p, (size_t)cap * 8, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(level_out, d_level.p, n64, hipMemcpyDeviceToHost)); HIPC(hipMemcpy(worst_out, d_worst.p, (size_t)n64 * 4, hipMemcpyDeviceToHost));
    std::memcpy(result, res.p, 32);
    return ART_OK;
}

int32_t art_read_wave_plan(ArtContext *c, uint8_t *level, size_t n64, uint32_t *items, uint32_t cap, uint32_t *n_items, uint32_t result[8], uint32_t state[4]) {
    if (!c) return fail(ART_E_INVALID, "art_read_wave_plan: null context");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    if (!c->frame_ready) return fail(ART_E_STATE, "art_read_wave_plan: no frame layout yet (art_trace)");
    WavePlan &P = c->plan;
    if (P.enabled) { r = plan_poll(c); if (r) return r; }   // a plan that has landed takes effect first
    if (level) {
        if (n64 != c->n_local / 64) return fail(ART_E_INVALID, "art_read_wave_plan: size mismatch");
        if (n64) HIPC(hipMemcpy(level, P.d_level.p, n64, hipMemcpyDeviceToHost));
    }
    const uint32_t n = P.n_items[P.cur], m = std::min(n, cap);
    if (n_items) *n_items = n;
    if (items && m) HIPC(hipMemcpy(items, P.d_items[P.cur].p, (size_t)m * 8, hipMemcpyDeviceToHost));
    if (result) std::memcpy(result, P.result.p, 32);
    if (state) { state[0] = (uint32_t)P.cur; state[1] = P.pending ? 1u : 0u; state[2] = P.replans; state[3] = P.cap; }
    return ART_OK;
}

} // extern "C"
