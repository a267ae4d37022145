/*
 * art_parity.h -- the parity, rehearsal and measurement surface of libart: NOT part of the boundary a host application binds (that is include/art.h).
 *
 * Everything here is exported by the same libart.so -- the tests, bench.py and tools/ reach it through the same C ABI as the product calls, so what they
 * compare bit for bit is the product's binary, not a test build -- and falls into three groups:
 *   1. the EQUIVALENT FORMS of the path (ArtTuning / art_set_tuning: staged and per-ray frames, host-built trees, wave-plan targets ...) and read-backs of
 *      intermediate results (hit records, shadow bits, the trees) that the parity tests compare with the oracle;
 *   2. building blocks that art_mgpu_* (include/art.h) is made of, kept callable for rehearsals of other exchange loops (tile-buffer rings, strided un-tiles,
 *      stream / event hand-offs);
 *   3. measurement aids (per-stage event sums, device timestamps, graph mode).
 * A maintainer of the reference binds include/art.h (bindings/art_sys.rs is generated from it alone).
 */
#ifndef ART_PARITY_H
#define ART_PARITY_H
#include "art.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- parity / debug surface (not part of the reference's API; used by tests through this C ABI) ---- */
/* Which of the EQUIVALENT forms of the path a context runs.  All-zero = what the product runs; the other values exist so that tests can
 * show that every form gives the same frame bit for bit (tests/test_gpu_parity.py) and so that sweeps need no rebuild.  libart reads
 * nothing from the environment: a host application's environment cannot change which kernels or trees it gets.
 * Synchronises; the scene has to be built again afterwards (art_scene_build). */
typedef struct ArtTuning {
    uint32_t frame_form;        /* 0 one fused launch per frame, packet walks (k_frame) | 2 four staged launches, every ray by itself (the persistent per-ray tracer).  (1 -- staged launches of
                                 * packet walks -- went in round 4 with the other forms that had lost: the packet's beam as node step, PLOC trees, 6- / 7-wave instances) */
    uint32_t tree_builder;      /* 0 the context's default (binned SAH on the device; ART_FLAG_FAST_BUILD: LBVH topology) | 1 binned SAH on the host threads */
    uint32_t packet_wide;       /* the fused frame's packet walks: 0 = default (the 128-byte 4-wide float nodes), 1 = 4-wide, 2 = the 64-byte binary nodes */
    uint32_t primary_walk, shadow_walk, ao_walk; /* frame_form 2 (and the AO rays of any frame): one ray type's per-ray walk: 0 default | 2 binary nodes | 4 quantised 4-wide nodes;
                                 * ao_walk alone also takes 6: the quantised 4-wide walk through the generic persistent tracer (k_trace) instead of the AO launch's own tracer (k_trace_ao, which is what 0 and 4 run) */
    uint32_t block_order;       /* launch order of the 256-pixel blocks: 0 XCD-aware macro-blocks of 2x2 tiles | 1 identity | n: macro-blocks of n x n tiles */
    uint32_t fixed_waves;       /* 1: no adaptive wave plan (like ART_FLAG_FIXED_WAVES) */
    uint32_t split_fixed_steps; /* wave plan: a fixed packet-step target instead of the adaptive one (0: adaptive) */
    uint32_t split_min_steps;   /* wave plan: lowest target (0 = 150) */
    float split_alpha;          /* wave plan: fraction of the launch's fair share a wave may take before its block is split (0 = 0.7) */
    uint32_t ao_entry_off;      /* 1: AO rays start at the root instead of their pixel's entry node */
    uint32_t trace_chunk, trace_refill, trace_blocks; /* persistent per-ray tracer of THIS context's launches: slots per cursor pop, idle lanes that trigger a refill, resident blocks; 0 = presets */
    uint32_t hw_queues;         /* hardware queues the HOST gave the process (GPU_MAX_HW_QUEUES; 0 = HIP's default of 4): the wave plan counts min(frames in flight, this) launches in flight */
    uint32_t log;               /* to stderr: 1 build phase times, 2 wave-plan decisions, 4 every wave-plan poll */
    uint32_t wide_builder;      /* the 4-wide collapse of the binary tree: 0 level by level on the device | 1 one host thread (the form the device one is tested against) */
    uint32_t as_versions;       /* moving models: versions of the acceleration structure a context cycles through, 1..24 (0 = twice the frames in flight, 4 at least): a refit may run while as_versions - 1 older frames are in flight; 1 = refit in place, nothing in flight */
    float refit_rebuild_ratio;  /* art_trace rebuilds instead of refitting once ArtStats.refit_cost_ratio exceeds this (0 = 2.0; negative: never) */
    uint32_t trace_leaf_batch;  /* persistent per-ray tracer: lanes that must be waiting for a triangle test before the wave runs one, 1..64 (0 = presets: 1, AO rays 8) */
    uint32_t plan_moving_interval; /* wave plan: frames between two looks at the waves while the camera / the lights change every frame (0 = 32) */
    uint32_t refit_streams;     /* moving models: streams of their own the refits run on, beside the frames of the ring slot they precede (0 = min(frames in flight, 4); 0xFFFFFFFF: none -- every refit on its frame's stream, in front of it) */
    uint32_t refit_fold_nodes;  /* moving models: trees of this many 4-wide nodes and more make the quantised records and the cost inside the refit's own workgroups, with a cached share of the cost per batch (0 = 400 000; 1 = every tree: the tests' way to that form on small scenes) */
    uint32_t shadow_hints;      /* the fused frame's shadow packets test the triangles that occluded their 8x8 block a frame ago before they walk the tree from the root: 0 = on (the product) | 1 = off: the frame kernel neither reads nor writes the context's hint table */
    uint32_t plain_math;        /* the frame's normalisations and lengths (ray generation and shading of the fused and the staged frame): 0 = the guarded fast path for sqrtf(x) and 1.0f / sqrtf(x) (the product;
                                 * art_parity_math_sweep) | 1 = the plain expressions in every wave: the same frame bit for bit */
} ArtTuning;
int32_t art_set_tuning(ArtContext *ctx, const ArtTuning *tuning);
/* per-pixel primary hit record, row-major: tuv[4*i] = t,u,v,0 ; ids[2*i] = primitive index (-1 miss), triangle id */
int32_t art_read_hits(ArtContext *ctx, float *tuv, int32_t *ids, size_t n_pixels);
/* per pixel: bit i = light i shadowed, bit 16+i = shadow ray for light i traced (i < 16) */
int32_t art_read_shadow_bits(ArtContext *ctx, uint32_t *bits, size_t n_pixels);
/* the context's table of shadow-occluder hints: for every 8x8 block b of the context's local pixels (local pixel id / 64) and light slot l = light % 4, four leaf positions
 * (~child of art_get_traversal_tree / art_get_wide_nodes; 0xFFFFFFFF: none) at words[16 * b + 4 * l ..]; n_words = 16 * local pixels / 64.  Both calls synchronise and need
 * the frame layout of a first art_trace.  art_write_shadow_hints overwrites the table (tests only: ANY content leaves every frame bit for bit what it is). */
int32_t art_read_shadow_hints(ArtContext *ctx, uint32_t *words, size_t n_words);
int32_t art_write_shadow_hints(ArtContext *ctx, const uint32_t *words, size_t n_words);
/* arbitrary ray queries on the built scene.  rays: n x 8 floats (o.xyz, tmin, d.xyz, tmax), host memory. */
int32_t art_query_closest(ArtContext *ctx, const float *rays, uint32_t n, float *tuv, int32_t *ids);
int32_t art_query_any(ArtContext *ctx, const float *rays, uint32_t n, uint8_t *hit);
/* the same queries with a cull mask for their rays (art.h, ray visibility masks: a candidate on a primitive whose mask shares no bit with cull_mask is discarded;
 * 0 sees nothing, above 0xFF is ART_E_INVALID); art_query_closest / art_query_any are the 0xFF case */
int32_t art_query_closest_masked(ArtContext *ctx, const float *rays, uint32_t n, uint32_t cull_mask, float *tuv, int32_t *ids);
int32_t art_query_any_masked(ArtContext *ctx, const float *rays, uint32_t n, uint32_t cull_mask, uint8_t *hit);
/* the device-built binary LBVH, in the oracle's canonical form (any pointer may be NULL):
 * leaf_gid[T], keys[T], child[2*(T-1)], node_lo/hi[(T-1)*3], leaf_lo/hi[T*3] */
int32_t art_get_lbvh(ArtContext *ctx, uint32_t *leaf_gid, uint64_t *keys, int32_t *child, float *node_lo,
                     float *node_hi, float *leaf_lo, float *leaf_hi);
/* the topology and node boxes the walks use over those leaves (child[2*(T-1)], node_lo/hi[3*(T-1)]): the binned-SAH tree by
 * default, the canonical tree with ART_FLAG_FAST_BUILD.  Node 0 is the root; child >= 0: internal node, < 0: ~leaf position. */
int32_t art_get_traversal_tree(ArtContext *ctx, int32_t *child, float *node_lo, float *node_hi);
/* the 4-wide collapse of that tree as the walks read it (new functionality: the reference's acceleration structures are opaque, vk_blas_builder.rs:88-170):
 * n_nodes records of 64 B (8-bit quantised child boxes: the per-ray walks) and of 128 B (float child boxes, children sorted along one axis: the packet
 * walks); node 0 is the root, child >= 0: node index, < 0: ~leaf position, INT32_MIN: absent (bit i of the records' valid masks clear).  Either pointer may be NULL; *n_nodes is always set. */
int32_t art_get_wide_nodes(ArtContext *ctx, void *quantised, void *floats, size_t capacity_nodes, uint32_t *n_nodes);
/* proof that the shading kernels' guarded fast paths return the plain expressions' bits: which = 0: 1.0f / sqrtf(x) behind its own guard (inv_sqrt_exact), 1: sqrtf(x)
 * likewise (sqrt_exact), 2: 1.0f / sqrtf(x) in the form of the surface block (the unguarded core and its note, the block's guard behind it).  A kernel feeds the bit
 * patterns first_bits + i * stride (mod 2^32), i < count, lane l of a wave taking i = 64 k + l, to the helper the frame kernels call and to a non-inlined copy of the plain
 * expression in the same translation unit, and compares the two results as uint32.  *mismatches = patterns that differ, *first_bad_bits = the pattern of the lowest such i
 * (untouched when there is none), *fast_lanes = patterns whose wave took the fast path (a wave takes it only when all its lanes are inside guard[0] <= x <= guard[1]).
 * which = 3: the shorter v_rsq_f32-based form of 1.0f / sqrtf(x) (inv_sqrt_short: what the k_frame instances of kFrameShort run for the core), under the same guard;
 * which = 4: v_rsq_f32 alone under that guard -- a 1-ulp approximation, the sweep's own control: it must report mismatches.  Synchronises. */
int32_t art_parity_math_sweep(ArtContext *ctx, uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, uint64_t *mismatches, uint32_t *first_bad_bits,
                              uint64_t *fast_lanes, float guard[2]);
/* proof that the short forms of the frame kernels' once-per-wave divisions return the division's bits.  which = 0: rcp_core(safe_dir(x)) against
 * 1.0f / safe_dir(x) (a ray's reciprocal direction), x = the bit patterns first_bits + i * stride (mod 2^32), i < count; 1: div_core(a, x) against a / x for the numerator
 * a = numerator_bits, x likewise; 2: a * v_rcp_f32(x) in div_core's place, the sweep's own control: it must report mismatches; 3: div_core over pair j = first_bits + i * stride of
 * a set of 254 * 254 * 64 pairs -- every pair of normal exponents with 16 mantissa pairs from the edges and 48 hashed from (j, numerator_bits as the seed); 4: div_core over the
 * camera ray's own operands, pair j = (W - 1) * 16416 + x: a = x + 0.5, b = W for W = 1..16384 and every x below W rounded up to 32.  An index past a set is skipped.
 * A lane whose operands lie inside the form's proven domain -- guard[0] <= |safe_dir(x)| <= guard[1] for which 0, guard[2] <= |a|, |b| <= guard[3] otherwise -- takes the
 * short form, any other lane the plain expression; the reference is a non-inlined copy of the plain expression in the same translation unit, compared as uint32.
 * *mismatches = lanes that differ, first_bad = the operands (a, b) of the lowest such i (untouched when there is none), *short_lanes = lanes that took the short form,
 * *lanes = lanes of the set.  Synchronises. */
int32_t art_parity_div_sweep(ArtContext *ctx, uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, uint32_t numerator_bits, uint64_t *mismatches,
                             uint32_t first_bad[2], uint64_t *short_lanes, uint64_t *lanes, float guard[4]);
/* how far the radiance-only helpers of the shading kernels are from the expressions they stand for (they are NOT bit-equal: DESIGN.md 1 keeps radiance to 1e-4 relative).
 * which = 0: the albedo's x^2.2 (pow22_texel: frexp, one hardware log2, one exp2, ldexp) against libm's powf(x, 2.2f), the frame kernels' form; which = 1: numerator * rcp(x),
 * the candidate for the BRDF's quotients, against the IEEE numerator / x (the kernels still run the division).  x = the bit patterns first_bits + i * stride (mod 2^32),
 * i < count <= 2^32; the reference is a non-inlined copy in the same translation unit.  *max_ulps = the largest distance in units of the reference's last place over the inputs
 * whose two results are both zero-or-finite and whose reference is at least 2^-100 in magnitude, *worst_bits = an input where it occurs (untouched when the distance is 0),
 * *class_mismatches = inputs whose two results are not of the same class (zero | finite | infinite | NaN), *first_class_bits = the lowest such i's pattern (untouched when there
 * is none).  Synchronises. */
int32_t art_parity_radiance_sweep(ArtContext *ctx, uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, float numerator, uint32_t *max_ulps, uint32_t *worst_bits,
                                  uint64_t *class_mismatches, uint32_t *first_class_bits);


/* ---- building blocks of art_mgpu_* (rehearsals of other exchange loops) ---- */
/* render ring slot `slot`'s compact tiles straight into a caller-owned device buffer (e.g. the tensor handed to the
 * gather); bytes must equal padded * 12 KiB (4 KiB with ART_FLAG_PACKED_TILES) * frames per launch; NULL unbinds */
int32_t art_bind_color_tiles(ArtContext *ctx, uint32_t slot, void *dev_ptr, size_t bytes);
/* two buffers per slot: the slot's frames write them alternately (even / odd trips round the ring), so a frame never waits for the
 * exchange that is still reading the slot's previous tiles -- only for the one of two trips ago.  art_device_color_tiles and
 * art_read_color_tiles refer to the buffer the latest frame wrote. */
int32_t art_bind_color_tiles_pair(ArtContext *ctx, uint32_t slot, void *dev_even, void *dev_odd, size_t bytes);
/* n (1..8) buffers per slot, written in turn: trip t round the frame ring writes bufs[t % n], so a frame waits only for the exchange of n
 * trips ago.  With two, the host was found waiting at every trip boundary (the whole trip before last must have been exchanged);
 * four leave the slack a jittery exchange needs (profiles/README.md r1n). */
int32_t art_bind_color_tiles_ring(ArtContext *ctx, uint32_t slot, void *const *bufs, uint32_t n, size_t bytes);
int32_t art_read_color_tiles(ArtContext *ctx, void *dst, size_t bytes); /* host copy of the same buffer (tests) */
/* the same with shard s's tiles at gathered + s * shard_stride_tiles tiles: several frames gathered by ONE collective leave each
 * rank's frames back to back, so consecutive shards of one frame are a whole block of frames apart */
int32_t art_untile_gathered_strided(ArtContext *ctx, const void *gathered_dev, uint32_t shard_count, uint32_t shard_stride_tiles, void *frame_dev, void *hip_stream);
/* n_frames frames in ONE launch (the exchange of several ring slots by one collective): frame z's tiles start z * padded tiles into
 * every shard's buffer, its image is written at frames_dev + z * width * height elements */
int32_t art_untile_gathered_frames(ArtContext *ctx, const void *gathered_dev, uint32_t shard_count, uint32_t shard_stride_tiles, uint32_t n_frames, void *frames_dev, void *hip_stream);

/* make an external stream wait (on the device) for the most recently traced frame */
int32_t art_stream_wait_frame(ArtContext *ctx, void *hip_stream);
/* make the NEXT art_trace wait (on the device) for an external hipEvent_t, e.g. "the gather that read this slot's tiles
 * three frames ago has finished" */
/* art_trace + art_stream_wait_frame in one call (the per-frame host path of a sharded run); *slot_used = the ring slot the frame took */
int32_t art_trace_for_stream(ArtContext *ctx, void *hip_stream, uint32_t *slot_used);
int32_t art_wait_external_event(ArtContext *ctx, void *hip_event);


/* ---- measurement aids ---- */
/* graph mode: art_trace replays one captured hipGraph per ring slot (memset + 4 launches) instead of issuing them one by
 * one -- for host-bound runs (small per-GPU frames).  The capture is redone after a camera / light / extent / scene change;
 * per-stage timings are not available in this mode (only the whole frame). */
int32_t art_set_graph_mode(ArtContext *ctx, int32_t on);
/* two device timestamps on the frame streams (a measurement aid, e.g. "how long did frames i..j take while the ring stayed full"):
 * art_timestamp_mark(ctx, 0|1) records mark 0 / 1 behind the most recently traced frame on its stream; art_timestamp_elapsed waits for mark 1
 * and returns the time between the two. */
int32_t art_timestamp_mark(ArtContext *ctx, uint32_t which);
int32_t art_timestamp_elapsed(ArtContext *ctx, float *ms);

/* device time per stage (HIP events on the context's stream) summed over the frames traced since the previous call
 * (at most the last 128): sums_ms = primary, shade, shadow, accumulate, whole frame */
int32_t art_collect_timings(ArtContext *ctx, float sums_ms[5], uint32_t *n_frames);
/* traces ONE frame with the step-counting instance of the fused frame, waits for it and returns what every wave of that launch did:
 * items[2*i] = 8x8 pixel block (local pixel id / 64), items[2*i+1] = mask over its sixteen 2x2 cells (0: an idle wave), steps[i] = packet steps
 * (nodes + triangles visited, all walks of the wave).  *n = waves of the launch; at most cap are copied.  (tools/step_hist.py) */
int32_t art_sample_wave_steps(ArtContext *ctx, uint32_t *items, uint32_t *steps, uint32_t cap, uint32_t *n);
/* the wave plan's kernel (k_plan) on buffers of the caller's making, all in host memory (tests/test_wave_plan.py compares it with tests/np_plan.py bit for bit): one launch
 * of what runs behind a sampled frame.  In: the launch order order[n256] of the 256-pixel blocks, the sampled table items_in[2 * n_items_in] (8x8 block, cell mask) with
 * what its waves counted cost[n_items_in], every 8x8 block's level level_in[n64] (0 | 1 | 2) and scratch word worst_in[n64] (zero between launches in a context),
 * n64 = 4 * n256; a table holds cap items; the target is fixed_steps, or max(min_steps, share * steps of the table) when that is 0.  Out: items_out[2 * cap], every word
 * 0xFFFFFFFF where the kernel wrote nothing; level_out[n64], worst_out[n64]; result[8] -- the words of PlanArgs::result ([0] items of the new table, [1] 1 = a new table was
 * written, [2] blocks in four, [3] blocks in sixteen, [4] the target, [5] the slowest wave) -- goes in as the caller filled it and comes back with the words the kernel
 * wrote changed.  CONTRACT (checked, ART_E_INVALID otherwise: the kernel indexes with them): 1 <= n256 <= 2^16, order is a permutation of 0 .. n256 - 1, every item's block
 * is below n64, every level is at most 2, n_items_in <= 2^22, 1 <= cap <= 2^22.  The context only names the device.  Takes its buffers for the call and gives them back
 * (art_parity_live_resources is what it was); synchronises. */
int32_t art_parity_plan(ArtContext *ctx, uint32_t n256, const uint32_t *order, const uint32_t *items_in, uint32_t n_items_in, const uint32_t *cost, const uint8_t *level_in,
                        const uint32_t *worst_in, uint32_t cap, float share, uint32_t min_steps, uint32_t fixed_steps, uint32_t *items_out, uint8_t *level_out,
                        uint32_t *worst_out, uint32_t result[8]);
/* a context's wave plan as it stands.  Synchronises, and a plan that has landed behind a sampled frame is adopted first, as the next art_trace would adopt it.  level[n64]: every
 * 8x8 block's level on the device (n64 = local pixels / 64, ART_E_INVALID otherwise); items[2 * i], i < min(*n_items, cap): the table the next frame runs, *n_items its length;
 * result[8]: the pinned words of the latest k_plan; state[4]: which of the two tables is the current one, 1 while a sample is in flight, tables adopted since the frame was
 * laid out, items a table can hold.  Any pointer but ctx may be NULL.  Needs the frame layout of a first art_trace (ART_E_STATE). */
int32_t art_read_wave_plan(ArtContext *ctx, uint8_t *level, size_t n64, uint32_t *items, uint32_t cap, uint32_t *n_items, uint32_t result[8], uint32_t state[4]);
/* what libart holds in this process right now: out[0] device allocations, [1] pinned allocations, [2] events,
 * [3] streams in use by contexts and ArtMgpu objects, [4] streams parked in the process-wide pool.  No context needed; never fails with out non-NULL. */
int32_t art_parity_live_resources(uint64_t out[5]);
/* what art_scene_set_vertices_device has done in this context so far: kernels enqueued (one per update of a primitive of the built structure), host synchronisations
 * the device form made itself (the one of a context's first deformation counts; so do the synchronous paths: a primitive outside the structure, the transition
 * from the host form, a read-back's wait), and device copies read back into host copies.  Any pointer but ctx may be NULL.  The steady state adds to the first only. */
int32_t art_vertex_update_counts(ArtContext *ctx, uint64_t *ingests, uint64_t *host_syncs, uint64_t *readbacks);


/* groups of launches of an ArtMgpu whose exchange has not been submitted yet (their frames may still run) and launches of the group that is still open.
 * Exchanges are submitted lazily -- from later launches or the flush -- so a host that also runs a control plane of its own between the ranks (barriers,
 * broadcasts) must not enter it while either is non-zero: ranks would meet in different collectives (art_mgpu_flush first). */
int32_t art_mgpu_pending(ArtMgpu *mg, uint32_t *groups_queued, uint32_t *launches_open);

#ifdef __cplusplus
}
#endif
#endif /* ART_PARITY_H */
