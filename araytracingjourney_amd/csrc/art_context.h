// art_context.h -- the host state behind include/art.h, shared by the host units (art_api.hip: context, frame ring, read-backs; art_scene.hip: scene tables, setters and the
// build; art_versions.hip: the ring of acceleration-structure versions and the refit; art_plan.hip: the wave plan; art_cast.hip: rays in device buffers).  Private to those
// five: no kernel unit includes it, and nothing here is exported from libart.so.  Each subsystem's state is written only in its own unit; the others call the functions
// declared at the end.
#pragma once
#include "art_internal.h"

using namespace art;
#pragma GCC visibility push(hidden)

namespace art {
// the thread's art_last_error() string lives in art_api.hip: these set it and hand the code back
int32_t fail(int32_t code, const std::string &msg);
int32_t hipfail(hipError_t e, const char *what);
}
#define HIPC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hipfail(e_, #x); } while (0)

struct HostPrim {
    std::vector<ArtVertex> verts;
    std::vector<uint8_t> indices; // original width
    uint32_t n_indices, idx_bytes;
    std::vector<uint8_t> tex;
    uint32_t tw, th;
    float o2w[12], w2o[12];
    bool enabled = true; // instanced in the acceleration structure (the reference's Device state, vk_model.rs:334-345); else kept on the host only
    bool verts_stale = false; // art_scene_set_vertices replaced `verts` since they were uploaded: a build over the same set uploads them again
    bool verts_behind = false; // art_scene_set_vertices_device wrote the primitive's slot of ArtContext::d_verts since: `verts` is behind it until someone needs it (verts_read_back)
    float cutoff = 0.0f;      // alpha cutoff (art_scene_set_alpha_cutoff; 0: opaque)
    uint32_t vis = 0xFFu;     // visibility mask (art_scene_set_primitive_mask; 0xFF: every ray sees it)
};

// one frame in flight: its own stream and per-frame buffers, like the reference's FrameData ring (renderer.rs:135, :300-318).  Everything it holds is a handle (art_own.h)
struct FrameSlot {
    PoolStream own;
    DevBuf<uint32_t> d_counters, d_shadow_bits;
    DevBuf<float4> d_hits, d_contrib, d_shadow_rays, d_color, d_normal, d_color_tiles;
    DevBuf<float> d_depth;
    DevBuf<uint8_t> d_occl; DevBuf<uint32_t> d_ao; bool ao_valid = false;
    DevBuf<float4> d_ao_pix;           // per local pixel: the AO rays' origin | start node, world normal | noise index (k_ao_pixels)
    DevBuf<uint32_t> d_wave_cost;      // fused frame: packet steps of each wave of the slot's last launch (feedback for the wave plan)
    // more than 16 lights: records 16.. in a table of the slot's own (frames in flight on other slots keep theirs), uploaded on the slot's stream when the list changed since the
    // slot's last upload; the pinned staging copy is rewritten only once the upload that read it has finished
    DevBuf<ArtLight> d_lights_more; Pinned<ArtLight> h_lights_more; Event lights_ev; bool lights_ev_set = false; uint64_t lights_epoch = 0;
    DevBuf<uint32_t> d_pix_more;       // fused frame, more than 16 lights: shadow rays of lights 16.. per pixel
    DevBuf<uint32_t> d_pcolor, d_pnormal, d_bgra; DevBuf<uint16_t> d_pdepth; bool presented = false; Event ao_ev[2];
    hipEvent_t done_alias = nullptr;   // the latest frame's completion is this ring event (fused frames: one record less per frame) instead of `done`
    float4 *ext_tiles = nullptr; size_t ext_tiles_bytes = 0; // caller-owned gather source (art_bind_color_tiles)
    static constexpr uint32_t kTileRing = kTileRingMax;
    float4 *ext_ring[kTileRing] = {}; uint32_t ext_ring_n = 0; // caller-owned buffers the slot's frames write in turn, one per trip round the frame ring (art_bind_color_tiles_ring)
    float4 *tiles_of_last = nullptr;   // where the slot's most recent frame wrote its tiles
    float4 *tiles_for(uint64_t frame_no, uint32_t F) { float4 *t = ext_tiles ? (ext_ring_n > 1 ? ext_ring[(frame_no / F) % ext_ring_n] : ext_tiles) : d_color_tiles.p; tiles_of_last = t; return t; }
    float4 *last_tiles() const { return tiles_of_last ? tiles_of_last : (ext_tiles ? ext_tiles : d_color_tiles.p); }
    Event done;                      // recorded after the slot's last frame
    hipGraphExec_t graph = nullptr;  // the frame's launch sequence captured once (graph mode); dropped whenever an input changes
    void *wait_event = nullptr;      // external event the slot's next frame must wait for (art_wait_external_event)
    uint32_t as_version = 0;         // which version of the acceleration structure the slot's latest frame read (art_trace_ao and the read-backs follow it)
    bool alpha = false;              // ... and whether it ran the instances with the alpha test (art_trace_ao follows it too)
    uint32_t ray_masks = kRayMasksAll; // ... and the cull masks of its rays (art_set_ray_masks; art_trace_ao casts its rays with the frame's AO mask)
};
constexpr uint32_t kMaxFrames = kMaxFrameSlots;

// Which wave of the fused frame's launch traces what.  A launch lasts as long as its slowest wave, and an 8x8 packet that crosses dense
// distant geometry walks the union of 64 unrelated paths: up to 0.5 ms where the rest of the launch is done after 0.1 ms.  Every wave
// reports its packet steps; blocks that took many are dealt to four waves (4x4 pixels each) or sixteen (2x2) from the next plan on, heaviest first.
// The image does not depend on the plan (closest / any hit are structure- and packet-independent), only the launch's tail does.
struct WavePlan {
    bool enabled = true;               // false (ART_FLAG_FIXED_WAVES, ArtTuning.fixed_waves): every 8x8 block is one wave, always
    // A block is split when its wave makes more packet steps (nodes + triangles visited, all its walks) than the launch's fair share of the
    // machine would take anyway: alpha * (steps of the whole launch) * (launches in flight) / (wave slots of the GPU), at least min_steps.
    // With 16 full frames in flight nothing is split (a straggler hides behind the other launches, and split waves cost more steps in
    // total); one frame at a time, or a 1/8 share of a frame, is where the tail is the launch.
    float alpha = 0.7f;                // ArtTuning.split_alpha (0.5 .. 1 measured alike on 1/8 shares)
    uint32_t min_steps = 150;          // ArtTuning.split_min_steps
    uint32_t fixed_steps = 0;          // ArtTuning.split_fixed_steps: a fixed target instead (tests, experiments)
    uint32_t in_flight = 1;            // min(frames in flight, hardware queues)
    std::vector<uint32_t> order;       // launch order of the 256-pixel blocks (setup_frame)
    // The plan is made ON THE DEVICE (k_plan, art_frame.hip) behind a sampled frame, on that frame's stream: every block's level lives there, the two tables alternate so that
    // frames in flight keep theirs, and the host learns "a new table of n items" from eight pinned words once the event behind the launch has fired.  (Rounds 1-3: counts up, one
    // host thread through 32 640 blocks, table down -- 0.3-0.9 ms inside an art_trace call now and then, ten frames' time; tools/camera_leg_probe.py, profiles/README.md round 4.)
    DevBuf<uint2> d_items[2]; uint32_t n_items[2] = {0, 0}; int cur = 0;
    DevBuf<uint8_t> d_level, d_level_tmp; DevBuf<uint32_t> d_worst;
    Pinned<uint32_t> result;           // pinned: PlanArgs::result
    uint32_t split1 = 0, split2 = 0;   // blocks the current table deals to four / sixteen waves
    Event retire[2][kMaxFrames]; bool retire_set[2] = {false, false}; // recorded on every frame stream when table i was left: it may be rewritten once they have all fired
    uint32_t cap = 0;                  // items a table (and the cost buffers) hold
    Event cost_ready; bool pending = false; int pending_table = 0;   // behind the sampled frame's k_plan
    Stream plan_stream;                // k_plan runs here, behind the sampled frame's completion event: one workgroup for ~0.1 ms -- on the frame's own stream the slot's next frame stood behind it (5-10 % of a 20-frame burst)
    uint64_t next_sample = 0; uint32_t interval = 1;
    uint64_t last_sample = 0;          // the frame that was sampled last
    bool moved_since_poll = false;     // the view or the lights changed since the last plan came back: a new table is no reason to look again at once (the next one would differ too)
    uint32_t replans = 0;
};

// One version of what a frame reads of the acceleration structure.  A static scene has none (the build's arrays are read directly); the first
// art_scene_set_model_matrix makes a small ring of them: a refit writes the NEXT version while frames in flight still read the older ones, like the
// reference's per-frame TLAS (one VkTlasBuilder per FrameData, renderer.rs:300-318, :637-651).  Version 0 is the build's own arrays.
// A version owns its event and nothing else: its arrays are views into the ring's blocks (Versions::as_block, as_pinned, shade_block, stage_*) or, version 0's, into the tree.
constexpr uint32_t kMaxAsVersions = 24;
struct AsVersion {
    DevTri *tris = nullptr; DevNodeW *widef = nullptr; DevNode4 *wide = nullptr; DevPrim *prims = nullptr;
    bool owned = false;                  // version 0 aliases c->bvh.* and c->d_prims
    // Pinned host memory the refit's kernels read and write IN PLACE (no copies in front of or behind the launches): the primitive table as of this refit, a byte per
    // primitive (moved since this version was written), and the refit's result (cost sum, root half-area, start / end device stamps).  d*: the device's addresses of the same.
    DevPrim *h_prims = nullptr, *dh_prims = nullptr; uint8_t *h_touched = nullptr, *dh_touched = nullptr; double *h_result = nullptr, *dh_result = nullptr;
    uint32_t *mark = nullptr;            // per 4-wide node (art_refit.hip retri_one): all zero between refits
    uint32_t *h_dirty = nullptr, *dh_dirty = nullptr;   // pinned: the batches this refit runs (those that hold a primitive that moved since the version was written)
    double *batch_cost = nullptr; bool cost_cached = false;   // device: every batch's share of this version's cost (large trees); valid once a refit has run all batches
    double *acc = nullptr;               // 4 doubles of device scratch of the refit's last launch: zero between refits
    uint64_t used[kMaxFrameSlots] = {};  // frame number + 1 of the newest launch on each ring slot that read this version (0: none)
    bool aux[kMaxFrameSlots] = {};       // art_trace_ao / art_present ran behind that frame on the slot's stream
    Event ready; bool ready_known = true; uint32_t ready_slot = 0; // the refit that wrote it: recorded on ring slot ready_slot's stream
    bool result_pending = false;         // h_result is that refit's once `ready` has fired
    uint64_t epoch = 0;                  // which refit wrote it (0: the build)
    // Deformed meshes (art_scene_set_vertices): the version's own shading records (the build's array until the context first deforms a built primitive: version 0
    // keeps aliasing it, the others get copies), and its staging of the replaced vertices -- pinned, written by the host once the version's previous refit is over,
    // and device memory, filled by one copy on the refit's stream that the regather in the refit's leaf stage reads (Versions::deform_off: where each primitive's are)
    DevShadeTri *shade = nullptr;
    ArtVertex *h_stage = nullptr; float *d_stage = nullptr;
};

// The ring of versions behind moving, deforming, masked and alpha-cut primitives (art_scene_set_model_matrix and its kin): its memory, what changed since the build, the
// epochs and the cost rule, the refit streams.  Written only in art_versions.hip.  Members go in reverse order of declaration: the blocks before the versions that point into them.
// art_scene_set_vertices_device's record of one built primitive: the event behind its latest ingest (the next refit's stream waits for it, so does the next ingest), and
// which versions' latest refits gathered from its slot of ArtContext::d_verts -- the next ingest's stream waits for those that may still run before it overwrites the slot
struct PrimIngest { Event done; bool open = false; uint32_t readers = 0; };   // open: recorded and not yet known to have fired; readers: a bit per version (kMaxAsVersions <= 32)
struct Versions {
    DevBuf<char> as_block; Pinned<char> as_pinned;    // ONE device allocation and ONE pinned one behind all the versions (six + three per version before).  versions_ms is something else: the refit streams' creation (a
                                                      // high-priority hardware queue each: 4-10 ms apiece) and the refit's work lists (host, 9 ms for config 2) -- ArtTuning.log bit 0 prints the parts
    // Refits run on streams of their own, one per ring slot (up to four): the refit in front of frame n of slot k then overlaps frame n - F, which still runs on that slot's
    // stream, instead of queueing behind it -- the slot's chain is frame, frame, frame with the refits beside it, and the frame waits for its refit's event.  (On the frame's
    // own stream a slot's cycle was refit + frame: a model moving every frame cost the ring a third of its depth, profiles/README.md round 4.)
    Stream refit_stream[4]; uint32_t n_refit_streams = 0;
    std::vector<uint64_t> prim_moved;          // per primitive: the refit (as_epoch numbering) that first shows its latest move; 0: where the build put it
    std::vector<uint64_t> prim_deformed;       // per primitive: the refit that first shows its latest vertices (art_scene_set_vertices); 0: the build's
    std::vector<PrimIngest> ingest;            // per primitive (art_scene_set_vertices_device); the events are made by a primitive's first ingest and go with the next build
    std::vector<uint32_t> ingest_open;         // the primitives whose ingest event may not have fired yet (sync_all and art_destroy wait for them: the caller's streams are not the context's)
    uint64_t ingests = 0, ingest_host_syncs = 0, ingest_readbacks = 0;   // art_vertex_update_counts
    std::vector<int64_t> deform_off;           // per primitive: first vertex of its slot in every version's staging (-1: never deformed since the build)
    size_t deform_verts = 0;                   // vertices of a version's staging (the sum of the deformed primitives' counts)
    DevBuf<char> shade_block;                  // ONE device allocation behind the shading records of versions 1 .. K-1 (made by the first deformation of a built primitive)
    DevBuf<char> stage_block; Pinned<char> stage_pinned;    // every version's staging of replaced vertices: device, pinned
    std::vector<AsVersion> as; uint32_t as_cur = 0; bool xform_dirty = false;   // (views into the five blocks above)
    int64_t masked_tris = 0;                   // triangles of primitives disabled since the build (still in the arrays, written "nowhere")
    bool alpha_bits_stale = false;             // a built primitive got a cutoff > 0 since the bits (ArtContext::d_alpha_bits) were last made
    uint64_t as_epoch = 0, binary_epoch = 0;   // refits so far; the refit the binary trees / node records reflect
    double as_cost0 = 0.0; float refit_cost_ratio = 1.0f; uint32_t refits = 0, rebuilds = 0; float last_refit_ms = 0.f, first_move_ms = 0.f, versions_ms = 0.f;
};

// Rays in device buffers (art_cast_rays).  Every cast takes the next of a ring of ART_CAST_POOL blocks: the block's work cursors (zeroed on the cast's stream in
// front of the launch), and an event recorded behind the launch on that stream.  The event is all the host ever needs of a cast, whichever stream the caller gave: the block is
// free again once it has fired (a ring that is lapped waits for it on the host: CastState::host_waits), the version of the structure the cast reads may be rewritten once it
// has fired (scene_refresh), and art_cast_sync / sync_all wait for the events of all blocks.  (One event per VERSION behind "the latest cast that reads it" would not do: casts
// on two callers' streams are not ordered, so the latest says nothing about the one before.)
struct CastBlock { Event ev; bool set = false; uint32_t version = 0; };
struct CastState {
    PoolStream stream;                         // made by the first cast (last of all: it is what says the ring is set up): casts with hip_stream NULL, the queries, and the refit a cast finds pending when the context has no refit streams
    DevBuf<uint32_t> cursors;                  // ART_CAST_POOL * kCastCursorWords words, one allocation
    CastBlock block[ART_CAST_POOL]; uint32_t next = 0;
    uint64_t casts = 0, rays = 0, host_waits = 0;
    DevBuf<float4> q_rays; DevBuf<uint8_t> q_out;   // art_query_*: the rays and the records of one query at a time on the device; they only grow
};

// Who owns what: every device buffer, pinned block, event and stream below is a handle (art_own.h) that its destructor releases; raw pointers are views or the caller's.
// art_destroy waits for every stream of the context and for the casts on callers' streams BEFORE `delete`, so no destructor frees what the GPU still uses.  Members go in reverse
// order of declaration, and a block is declared before whatever points into it: the arena before the tree that borrows it, the versions' blocks before the versions.
struct ArtContext {
    ArtConfig cfg{};
    int device = 0;
    hipStream_t ext_stream = nullptr; // art_set_stream (single frame in flight only)
    uint32_t F = 1, last = 0;         // frames in flight; slot of the most recently submitted frame
    FrameSlot slot[kMaxFrames];
    uint32_t W = 0, H = 0;
    std::vector<HostPrim> prims;
    bool built = false, have_camera = false, frame_ready = false;
    // which of the equivalent forms this context runs: the defaults are the product, the others are reachable through art_set_tuning only (nothing reads the environment)
    ArtTuning tuning{};
    bool fused = true;        // the frame is ONE launch of packet walks (k_frame); frame_form 2: four staged launches, every ray by itself
    int tree_builder = 3;     // with fast_trace: 3 = binned SAH on the device (art_sahdev.hip), 1 = the same on the host threads (art_sah.hip)
    bool fast_trace = true;   // rebuild the traversal tree with the binned SAH after the LBVH (ART_FLAG_FAST_BUILD: keep the Karras tree)
    bool packet_wide = true;  // packets walk the 128-byte 4-wide float nodes (half the dependent node fetches); false: the 64-byte binary nodes
    int kind_primary = 8, kind_shadow = 8, kind_ao = 4; // 8 = packet walk over the binary nodes (coherent rays: primary, shadow); per-ray walks (AO, queries): 2 binary, 4 wide quantised (measured: profiles/README.md)
    uint32_t macro = 2;       // XCD-aware launch order: macro-blocks of macro x macro tiles (0: identity)
    bool ao_entry = true;     // AO rays start at the per-pixel entry node (k_ao_entry)
    bool wide_on_host = false; // ArtTuning.wide_builder
    DevBuf<float4> d_ao_tab; uint32_t ao_tab_spp = 0; // art_trace_ao's sample table and the sample count it was made for
    // device scene
    DevBuf<float> d_verts; DevBuf<uint8_t> d_indices; DevBuf<uint32_t> d_tex; DevBuf<DevPrim> d_prims; DevBuf<uint32_t> d_first_tri;
    std::vector<uint32_t> h_first_tri; // first global triangle id of every primitive slot (ascending): gid -> (primitive, triangle) on the host
    Arena arena;              // the build phases' scratch, kept from build to build (art_internal.h)
    Lbvh bvh{};
    std::vector<uint8_t> uploaded;   // which primitives' vertices / indices / texels are on the device, at the offsets a build over exactly this set computes (empty: nothing): a
                              // build over the same set -- the rebuild behind the refit's cost rule, a change of tuning -- uploads only the primitive table
    uint32_t T = 0;
    Versions ver;                              // moving models: the ring of versions of the structure (art_versions.hip)
    std::vector<DevPrim> h_dev_prims;          // host copy of d_prims (build order), matrices kept current: the primitive table as the next refit will upload it
    // alpha-masked primitives: the cutoffs travel in the versioned primitive table (DevPrim::cutoff), so a change is a refit over no batch, like a
    // primitive that is disabled; alpha_bits marks the leaves whose primitive may have a cutoff (made by the build, bits added in front of the refit that first shows a
    // new cutoff, never cleared until the next build: a superset is safe, the cutoff itself decides)
    DevBuf<uint32_t> d_alpha_bits;
    bool alpha_live = false;                   // some enabled primitive has a cutoff > 0 or a visibility mask other than 0xFF: frames and queries run the instances with the alpha test
    uint32_t ray_masks = kRayMasksAll;         // art_set_ray_masks: primary | shadow << 8 | ao << 16; per-launch state like the camera
    ArtCamera camera{};
    uint32_t B = 1, read_b = 0;       // frames per launch of the fused frame (art_set_frames_per_launch); which of them the read / device-pointer calls refer to
    ArtCamera cam_more[kMaxBatch - 1] = {}; // cameras of frames 1.. of a launch (frame 0: camera)
    std::vector<ArtLight> lights; uint64_t lights_epoch = 1;   // (bumped by every art_set_lights that changes the list)
    // frame
    std::vector<uint32_t> tile_list; uint32_t tiles_x = 0, tiles_y = 0, padded_tiles = 0, n_local = 0;
    DevBuf<uint32_t> d_tile_list;
    DevBuf<uint32_t> d_tile_xy;     // owned tile -> x | y << 16 (fused frame: no division per pixel lookup)
    DevBuf<uint32_t> d_tile_slot;   // un-tile table: tile -> owner << 24 | index among the owner's tiles (every shard's layout, setup_frame)
    DevBuf<uint32_t> d_block_order; // launch block -> 256-pixel block of the frame: one L2 (XCD) per screen region (setup_frame)
    WavePlan plan;                  // fused frame: wave -> (8x8 block, cells)
    CastState cast;                 // rays in device buffers
    // Shadow-occluder hints of the fused frame's any-hit packet walks (FrameArgs::hints): ONE table for the context -- not one per ring slot: the frames in
    // flight feed each other -- of (n_local / 64) * kHintLights entries of four leaf positions.  All 0xFF (empty) after setup_frame (allocation, resize) and after every
    // art_scene_build (leaf positions change; the build the refit's cost rule starts is one); both run with nothing in flight.  Refits, moves, deformations, enable / disable,
    // cameras and lights leave it alone: leaf positions survive them and every hint is tested against the frame's own triangles.
    DevBuf<uint32_t> d_hints;
    bool shadow_hints = true;       // ArtTuning.shadow_hints = 1 turns them off: the frames get a null table
    size_t hint_words() const { return (size_t)(n_local / 64u) * kHintLights * 4u; }
    static constexpr int kRing = 128;          // per-frame stage events kept for art_collect_timings
    Event ev[kRing][5];
    bool ev_fused[kRing] = {};                 // the frame was one launch: only ev[0] and ev[4] were recorded
    uint64_t frame_no = 0, collected_upto = 0;
    Event mark[2];                             // art_timestamp_mark
    bool traced = false;
    bool force_sample = false; // art_sample_wave_steps: the next fused frame counts its waves' steps whatever the plan's cadence
    bool graph_mode = false; // replay a captured hipGraph per slot instead of 5 launches + 6 event records (host-bound multi-GPU runs)
    uint32_t ao_spp = 0;
    ArtStats stats{};
    bool tiles_packed() const { return (cfg.flags & ART_FLAG_PACKED_TILES) != 0; }
    bool tiled() const { return cfg.shard_count > 1 || (cfg.flags & ART_FLAG_TILE_OUTPUT) != 0; } // writes the compact tile buffer beside the frame
    size_t tile_px_bytes() const { return tiles_packed() ? 4 : 12; } // B10G11R11 words or RGB32F (the colour without its constant alpha) in the compact tile buffer
    size_t tiles_bytes() const { return (size_t)padded_tiles * kTilePixels * tile_px_bytes(); } // one frame's compact tile buffer
    bool fused_frame() const { return fused && kind_primary == 8 && kind_shadow == 8; } // the frame is one launch of packet walks: no staged records, no counters
    TraceTune trace_tune() const { return TraceTune{tuning.trace_chunk, tuning.trace_refill, tuning.trace_blocks, tuning.trace_leaf_batch}; } // the per-ray tracers' knobs (frames and casts)
    hipStream_t stream_of(uint32_t k) const { return (ext_stream && F == 1) ? ext_stream : slot[k].own.p; }
    hipStream_t main_stream() const { return stream_of(0); }
};

// what a launch reads of one version (as_ptrs)
struct AsPtrs { const DevTri *tris; const DevNodeW *widef; const DevNode4 *wide; const DevPrim *prims; const DevShadeTri *shade; };

namespace art {
// ---- art_api.hip ----
int32_t use_device(ArtContext *c);
void drop_graphs(ArtContext *c);
int32_t sync_all(ArtContext *c);                           // every stream of the context, the casts on callers' streams included
// ---- art_scene.hip ----
int32_t ensure_wide(ArtContext *c, bool needed);
int32_t ensure_binary(ArtContext *c, bool needed);
void gid_to_ids(const ArtContext *c, uint32_t gid, int32_t *ids);
// ---- art_versions.hip (every write of a Versions field is there) ----
AsPtrs as_ptrs(const ArtContext *c, uint32_t v);
uint32_t as_current(const ArtContext *c);                  // the version the next launch reads
bool as_pending(const ArtContext *c);                      // a primitive changed since that version was written: scene_refresh in front of the next launch
void as_release(ArtContext *c);                            // the versions go (the caller synchronised); the tree and its work lists stay
// Launches on `stream` read version v: ordered behind the refit that wrote it, by an event wait while that refit may still run.  own_slot: the ring slot whose stream
// `stream` is -- a refit recorded on that slot's stream orders the launch by itself -- or ~0u for a stream that no ring slot owns (casts; scene_refresh writes
// ready_slot the same way).
int32_t as_wait_ready(ArtContext *c, uint32_t v, hipStream_t stream, uint32_t own_slot);
void as_frame_reads(ArtContext *c, uint32_t v, uint32_t k);   // ring slot k's frame about to be launched (frame_no) reads version v
void as_aux_behind(ArtContext *c, uint32_t v, uint32_t k);    // art_trace_ao / art_present ran behind that frame on the slot's stream
void harvest_cost(ArtContext *c);
int32_t scene_refresh(ArtContext *c, uint32_t k, hipStream_t s);
int32_t refresh_now(ArtContext *c);                        // the parity surface's: nothing in flight, the pending change applied
int32_t as_sync_streams(ArtContext *c);                    // sync_all's and art_destroy's part: a refit no frame has waited for yet
void as_fill_stats(const ArtContext *c, ArtStats *st);     // first_move_ms, versions_ms, refit_ms, refit_cost_ratio, refits, rebuilds
void as_scene_reset(ArtContext *c);                        // art_scene_build's start (synchronised): the ring goes, the epochs and the cost rule start over, nothing is pending
int32_t as_scene_built(ArtContext *c);                     // ... and its end: the per-primitive records of the new table; the ring at once under ART_FLAG_DYNAMIC_SCENE
bool binary_is_current(const ArtContext *c);               // ensure_binary's: the binary trees reflect the current version
void binary_mark(ArtContext *c, bool current);             // ... they do now / they have to be made again whatever the version
// what the setters report about a primitive of the built structure.  shows: it is enabled, so the next launch has to refit first
void as_prim_moved(ArtContext *c, uint32_t id, bool shows, int64_t masked_delta = 0);   // a matrix; masked_delta: triangles that left (+) or came back (-) with a residency change
int32_t as_prim_deformed(ArtContext *c, uint32_t id, bool shows, bool staged = true);   // new vertices: the ring if there is none, the versions' shading records and -- staged: the host form -- staging (one synchronisation the first time); fails with nothing changed
// art_scene_set_vertices_device on a primitive of the built structure, after as_prim_deformed(.., false): k_ingest_verts into the primitive's slot on stream s, ordered on the
// device behind the refits that still gather from the slot and behind the primitive's previous ingest.  bring_up: the host copy the slot is behind (a host-form call since
// the build, in front of a POSITIONS update) is copied into it first, synchronously
int32_t as_ingest(ArtContext *c, uint32_t id, const void *src, uint32_t stride_bytes, const ArtVertex *bring_up, hipStream_t s);
int32_t as_ingest_wait(ArtContext *c, uint32_t id);        // the host waits for the primitive's latest ingest (a read-back of its slot follows)
void as_ingest_counts(ArtContext *c, uint64_t host_syncs, uint64_t readbacks);   // what art_scene.hip adds to art_vertex_update_counts
void as_table_changed(ArtContext *c, bool new_alpha_bits); // a cutoff or a visibility mask: a refit over no batch; new_alpha_bits: the primitive's leaves need their bits first
// ---- art_plan.hip (every write of a WavePlan field is there) ----
int32_t plan_reset(ArtContext *c, const std::vector<uint32_t> &order);   // a new frame layout: the launch order of its 256-pixel blocks, the first table
int32_t plan_poll(ArtContext *c);
bool plan_want_sample(ArtContext *c, uint32_t n_wave_items);             // the frame about to be launched counts its waves' steps
int32_t plan_launch(ArtContext *c, const FrameArgs &a, hipEvent_t frame_done);
void plan_hint_moved(ArtContext *c);
void plan_hint_built(ArtContext *c);                                     // a new scene: the heavy blocks are elsewhere
int32_t plan_sync(ArtContext *c);                                        // sync_all's part: a plan behind a sampled frame
int32_t plan_rewind(ArtContext *c);                                      // ring_rewind's part (everything is synchronised): a landed plan is adopted, not dropped
// ---- art_cast.hip (every use of CastState / CastBlock is there) ----
int32_t cast_sync(ArtContext *c);                                        // sync_all's part: every cast enqueued so far, on whichever stream, and the cast stream
int32_t cast_wait_version(ArtContext *c, uint32_t version);              // scene_refresh's part: the casts that still read the version about to be rewritten
int32_t cast_drain(ArtContext *c);                                       // art_scene_clear's part: outstanding casts read the scene that goes away
}
#pragma GCC visibility pop
