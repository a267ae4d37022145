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
// the ring starts again at frame 0 (a sample in flight has landed: everything is synchronised)
void art::plan_rewind(ArtContext *c) { c->plan.next_sample = 0; c->plan.pending = false; c->plan.last_sample = 0; }

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
    if (!P.enabled) P.pending = false;   // nobody polls a plan that is switched off (k_plan ran all the same: its table is not adopted)
    return ART_OK;
}

} // extern "C"
