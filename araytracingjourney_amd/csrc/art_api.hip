// art_api.hip -- the C ABI of include/art.h: context, frame ring and frame orchestration, read-backs, host maths.  (The scene: art_scene.hip; the versions of the acceleration
// structure: art_versions.hip; the wave plan: art_plan.hip; rays in device buffers: art_cast.hip; the state they share: art_context.h.)
// Product code; gfx950 only; there is no CPU fallback anywhere in this file.
#include "art_context.h"
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

static thread_local std::string g_err;
int32_t art::fail(int32_t code, const std::string &msg) { g_err = msg; return code; }
int32_t art::hipfail(hipError_t e, const char *what) { return fail(ART_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
void art::set_last_error(const char *msg) { g_err = msg ? msg : ""; }

// Frame streams are kept for the life of the process and handed from a destroyed context to the next one: streams created after
// others were destroyed share hardware queues badly (a context made after another had been destroyed ran 60 % slower, profiles r1k).
static std::mutex g_stream_mutex;
static std::vector<std::pair<int, hipStream_t>> g_free_streams; // (device, stream)
hipError_t art::acquire_stream(int device, hipStream_t *out) {
    {
        std::lock_guard<std::mutex> lock(g_stream_mutex);
        for (size_t i = 0; i < g_free_streams.size(); i++)
            if (g_free_streams[i].first == device) { *out = g_free_streams[i].second; g_free_streams.erase(g_free_streams.begin() + (long)i); live_add(kLivePooled, -1); live_add(kLiveStreams, 1); return hipSuccess; }
    }
    hipError_t e = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    if (e == hipSuccess) live_add(kLiveStreams, 1); else *out = nullptr;
    return e;
}
void art::release_stream(int device, hipStream_t s) {
    (void)hipStreamSynchronize(s);
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    g_free_streams.push_back({device, s});
    live_add(kLiveStreams, -1); live_add(kLivePooled, 1);
}

int32_t art::use_device(ArtContext *c) {
    HIPC(hipSetDevice(c->device));
    return ART_OK;
}

void art::drop_graphs(ArtContext *c) {
    for (uint32_t k = 0; k < kMaxFrames; k++)
        if (c->slot[k].graph) { (void)hipStreamSynchronize(c->stream_of(k)); (void)hipGraphExecDestroy(c->slot[k].graph); c->slot[k].graph = nullptr; } // never destroy a graph in flight
}

int32_t art::sync_all(ArtContext *c) {
    { int32_t r = cast_sync(c); if (r) return r; }   // (first: a cast may stand behind a refit below, never the other way round)
    { int32_t r = as_sync_streams(c); if (r) return r; }   // (a refit no frame has waited for yet)
    { int32_t r = plan_sync(c); if (r) return r; }
    for (uint32_t k = 0; k < c->F; k++) HIPC(hipStreamSynchronize(c->stream_of(k)));
    return ART_OK;
}

namespace {

// A directional light's L vector, its length and the shadow ray's reciprocal direction are the same for every pixel (light.glsl:96: -dir * 10): the
// kernel-argument copy of such a record carries them in fields a directional light does not use (area_pos2 = L, penumbra_angle = |nn_L|, area_pos3 =
// 1 / safe(L)), made here with the operations the kernel would run per lane -- correctly rounded sqrt and division, explicit fma, nothing contracted
// (the library is built with -ffp-contract=off): the same bits.  The caller's records are untouched.
static void directional_constants(ArtLight &l) {
    if (l.type != 2u) return;
    const float nx = -l.dir[0] * 10.0f, ny = -l.dir[1] * 10.0f, nz = -l.dir[2] * 10.0f;           // neg(dir) * 10
    const float d = std::fmaf(nz, nz, std::fmaf(ny, ny, nx * nx));                               // dot3
    const float len = std::sqrt(d), inv = 1.0f / std::sqrt(d);
    const float L[3] = {nx * inv, ny * inv, nz * inv};                                           // nrm3
    for (int k = 0; k < 3; k++) {
        l.area_pos2[k] = L[k];
        const float sd = std::fabs(L[k]) < 1e-20f ? std::copysign(1e-20f, L[k]) : L[k];          // safe_dir
        l.area_pos3[k] = 1.0f / sd;
    }
    l.penumbra_angle = len;
}

int32_t setup_frame(ArtContext *c) {
    // tile ownership + per-frame buffers for the current extent / light count
    c->tiles_x = (c->W + kTile - 1) / kTile; c->tiles_y = (c->H + kTile - 1) / kTile;
    uint32_t count = c->cfg.shard_count > 1 ? c->cfg.shard_count : 1, rank = count > 1 ? c->cfg.shard_rank : 0;
    c->tile_list.clear();
    std::vector<uint32_t> per(count, 0), slot_of((size_t)c->tiles_x * c->tiles_y);
    const std::vector<uint8_t> owner_of = shard_owner_table(c->tiles_x, c->tiles_y, count, c->cfg.root_relief);
    for (uint32_t ty = 0; ty < c->tiles_y; ty++)
        for (uint32_t tx = 0; tx < c->tiles_x; tx++) {
            uint32_t o = owner_of[(size_t)ty * c->tiles_x + tx];
            slot_of[(size_t)ty * c->tiles_x + tx] = (o << 24) | per[o];
            per[o]++;
            if (o == rank) c->tile_list.push_back(ty * c->tiles_x + tx);
        }
    HIPC(c->d_tile_slot.ensure(slot_of.size()));
    HIPC(hipMemcpy(c->d_tile_slot.p, slot_of.data(), slot_of.size() * 4, hipMemcpyHostToDevice));
    c->padded_tiles = 0;
    for (uint32_t v : per) c->padded_tiles = v > c->padded_tiles ? v : c->padded_tiles;
    c->n_local = (uint32_t)c->tile_list.size() * kTilePixels;
    size_t npix = (size_t)c->W * c->H;
    size_t nl = c->lights.size() ? c->lights.size() : 1;
    HIPC(c->d_tile_list.ensure(c->tile_list.size()));
    if (!c->tile_list.empty()) HIPC(hipMemcpy(c->d_tile_list.p, c->tile_list.data(), c->tile_list.size() * 4, hipMemcpyHostToDevice));
    {
        std::vector<uint32_t> xy(c->tile_list.size());
        for (size_t i = 0; i < xy.size(); i++) xy[i] = (c->tile_list[i] % c->tiles_x) | ((c->tile_list[i] / c->tiles_x) << 16);
        HIPC(c->d_tile_xy.ensure(xy.size()));
        if (!xy.empty()) HIPC(hipMemcpy(c->d_tile_xy.p, xy.data(), xy.size() * 4, hipMemcpyHostToDevice));
    }
    {   // Workgroups are dealt round-robin to the 8 XCDs, each with its own 4 MB L2.  Group the owned tiles into macro-blocks of
        // kMacro x kMacro tiles, deal the macro-blocks round-robin to the XCDs (balance: every XCD gets pieces from all over the
        // frame) and order the launch so that XCD x works through ITS macro-blocks: its L2 then holds the BVH of a few screen
        // regions instead of the whole view, in every kernel of the frame and in every frame in flight.  A permutation of the
        // blocks whatever the hardware's dispatch order is; only the locality depends on it.  (ArtTuning.block_order 1: identity.)
        const uint32_t macro = c->macro;
        const uint32_t nb = c->n_local / 256;
        std::vector<uint32_t> order(nb);
        for (uint32_t b = 0; b < nb; b++) order[b] = b;
        if (macro > 0 && nb >= 64) {
            const uint32_t mx = (c->tiles_x + macro - 1) / macro;
            std::vector<std::vector<uint32_t>> queue(8);
            std::vector<std::pair<uint32_t, uint32_t>> keyed; // (macro-block id, block)
            for (uint32_t b = 0; b < nb; b++) { uint32_t t = c->tile_list[b >> 2]; keyed.push_back({(t / c->tiles_x / macro) * mx + (t % c->tiles_x) / macro, b}); }
            std::stable_sort(keyed.begin(), keyed.end());
            uint32_t rank = 0;
            for (size_t i = 0; i < keyed.size(); i++) { if (i && keyed[i].first != keyed[i - 1].first) rank++; queue[rank & 7u].push_back(keyed[i].second); }
            // launch position b runs on XCD b % 8: take that XCD's next block; once a queue is empty its positions take what is left
            size_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t b = 0; b < nb; b++) {
                uint32_t q = b & 7u;
                for (uint32_t tries = 0; tries < 8 && head[q] >= queue[q].size(); tries++) q = (q + 1) & 7u;
                order[b] = queue[q][head[q]++];
            }
        }
        HIPC(c->d_block_order.ensure(nb ? nb : 1));
        if (nb) HIPC(hipMemcpy(c->d_block_order.p, order.data(), (size_t)nb * 4, hipMemcpyHostToDevice));
        int32_t pr = plan_reset(c, order); if (pr) return pr;
    }
    HIPC(c->d_hints.ensure(c->hint_words())); HIPC(hipMemset(c->d_hints.p, 0xFF, c->d_hints.n * 4));   // the blocks are other pixels now: every entry empty
    for (uint32_t k = 0; k < c->F; k++) {
        FrameSlot &S = c->slot[k];
        HIPC(S.d_wave_cost.ensure(c->plan.cap ? c->plan.cap : 1));
        HIPC(S.d_counters.ensure(kCounterWords)); HIPC(hipMemset(S.d_counters.p, 0, kCounterWords * 4)); // packet frames keep them clear themselves (k_accumulate)
        const bool staged = !c->fused_frame(); // the fused frame keeps these records in registers
        const size_t B = c->B; // frames per launch: every output holds B frames back to back
        if (staged || (c->cfg.flags & ART_FLAG_KEEP_DEBUG)) HIPC(S.d_hits.ensure(c->n_local * B));
        if (staged) { HIPC(S.d_contrib.ensure(nl * c->n_local)); HIPC(S.d_shadow_rays.ensure(2 * nl * c->n_local)); }
        HIPC(S.d_color.ensure(npix * B)); HIPC(S.d_normal.ensure(npix * B)); HIPC(S.d_depth.ensure(npix * B));
        HIPC(hipMemset(S.d_color.p, 0, npix * B * 16)); HIPC(hipMemset(S.d_normal.p, 0, npix * B * 16)); HIPC(hipMemset(S.d_depth.p, 0, npix * B * 4));
        if (c->tiled()) { HIPC(S.d_color_tiles.ensure((size_t)c->padded_tiles * kTilePixels * B)); HIPC(hipMemset(S.d_color_tiles.p, 0, c->tiles_bytes() * B)); }
        if ((c->cfg.flags & ART_FLAG_KEEP_DEBUG) || c->fused) HIPC(S.d_shadow_bits.ensure(c->n_local * B)); // fused frames always write their per-pixel shadow bits (stats)
        if (c->fused && c->lights.size() > (size_t)kMaxLights) HIPC(S.d_pix_more.ensure(c->n_local * B));
        if (S.ext_tiles && S.ext_tiles_bytes != c->tiles_bytes() * B) { S.ext_tiles = nullptr; S.ext_ring_n = 0; S.tiles_of_last = nullptr; S.ext_tiles_bytes = 0; }
    }
    HIPC(hipDeviceSynchronize()); // the clears above ran on the null stream; the slots' streams are non-blocking
    drop_graphs(c);
    c->frame_ready = true;
    return ART_OK;
}

void normalize3(const float *v, float *o) {
    float l = std::sqrt(std::fmaf(v[2], v[2], std::fmaf(v[1], v[1], v[0] * v[0])));
    float inv = 1.0f / l;
    o[0] = v[0] * inv; o[1] = v[1] * inv; o[2] = v[2] * inv;
}
void cross3h(const float *a, const float *b, float *o) {
    o[0] = std::fmaf(a[1], b[2], -(a[2] * b[1])); o[1] = std::fmaf(a[2], b[0], -(a[0] * b[2])); o[2] = std::fmaf(a[0], b[1], -(a[1] * b[0]));
}
float dot3h(const float *a, const float *b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }

// general 4x4 inverse by cofactors, column-major (stands in for nalgebra's try_inverse, vk_camera.rs:111-113)
bool mat4_inverse(const float *m, float *o) {
    float inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (!(std::fabs(det) > 0.0f)) return false; // singular, or NaN somewhere in m
    det = 1.0f / det;
    bool finite = true;
    for (int i = 0; i < 16; i++) { o[i] = inv[i] * det; finite = finite && std::isfinite(o[i]); }
    return finite;
}

} // namespace

// a camera block with a NaN or an infinity in it makes rays no triangle can be tested against (the packed struct is read through a copy: its floats are unaligned)
static bool camera_finite(const ArtCamera *cam) {
    float v[sizeof(ArtCamera) / 4];
    std::memcpy(v, cam, sizeof(ArtCamera));
    for (float x : v) if (!std::isfinite(x)) return false;
    return true;
}

int32_t art::ring_rewind(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "ring_rewind: null context");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    c->frame_no = 0; c->collected_upto = 0; c->last = 0;
    return plan_rewind(c);
}

static int32_t read_back(ArtContext *c, const void *src, size_t have, void *dst, size_t bytes, const char *who) {
    if (!c || !dst) return fail(ART_E_INVALID, std::string(who) + ": null argument");
    if (!c->traced) return fail(ART_E_STATE, std::string(who) + ": nothing traced yet");
    if (bytes != have) return fail(ART_E_INVALID, std::string(who) + ": size mismatch");
    int32_t r = use_device(c); if (r) return r;
    HIPC(hipStreamSynchronize(c->stream_of(c->last)));
    HIPC(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return ART_OK;
}
// the latest frame's image `buf`, of the frame of its launch that the read / device-pointer calls refer to (art_set_read_frame): to the host, or where it is
template <class T> static int32_t read_image(ArtContext *c, DevBuf<T> FrameSlot::*buf, void *dst, size_t bytes, const char *who) {
    if (!c) return read_back(c, nullptr, 0, dst, bytes, who);   // (which says so)
    return read_back(c, (c->slot[c->last].*buf).p + (size_t)c->read_b * c->W * c->H, (size_t)c->W * c->H * sizeof(T), dst, bytes, who);
}

// lays the frame out if that has not happened yet
static int32_t ensure_layout(ArtContext *c, const char *who) {
    if (!c->frame_ready) { int32_t r = use_device(c); if (r) return r; if (c->W == 0 || c->H == 0) return fail(ART_E_STATE, std::string(who) + ": zero extent"); r = setup_frame(c); if (r) return r; }
    return ART_OK;
}
// a device-pointer call: somewhere to put the pointer, and the frame laid out
static int32_t device_ready(ArtContext *c, void **p, const char *who) {
    if (!c || !p) return fail(ART_E_INVALID, std::string(who) + ": null argument");
    return ensure_layout(c, who);
}
template <class T> static int32_t device_image(ArtContext *c, DevBuf<T> FrameSlot::*buf, void **p, size_t *b, const char *who) {
    int32_t r = device_ready(c, p, who); if (r) return r;
    *p = (c->slot[c->last].*buf).p + (size_t)c->read_b * c->W * c->H; if (b) *b = (size_t)c->W * c->H * sizeof(T);
    return ART_OK;
}

extern "C" {

const char *art_last_error(void) { return g_err.c_str(); }

int32_t art_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t art_create(const ArtConfig *cfg, ArtContext **out) {
    if (!cfg || !out) return fail(ART_E_INVALID, "art_create: null argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ART_E_NO_DEVICE, "art_create: no HIP device (libart has no CPU fallback)");
    int dev = cfg->device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) return fail(ART_E_NO_DEVICE, "art_create: hipGetDevice failed"); }
    if (dev >= n) return fail(ART_E_INVALID, "art_create: device ordinal out of range");
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ART_E_NO_DEVICE, std::string("art_create: device is ") + prop.gcnArchName + ", libart is built for gfx950 only");
    if (cfg->morton_bits != 0 && cfg->morton_bits != 30 && cfg->morton_bits != 63) return fail(ART_E_INVALID, "art_create: morton_bits must be 0, 30 or 63");
    if (cfg->shard_count > 1 && cfg->shard_rank >= cfg->shard_count) return fail(ART_E_INVALID, "art_create: shard_rank >= shard_count");
    if (cfg->shard_count > 255) return fail(ART_E_INVALID, "art_create: at most 255 shards");
    if (cfg->frames_in_flight > kMaxFrames) return fail(ART_E_INVALID, "art_create: at most 24 frames in flight");
    if (cfg->root_relief > 255) return fail(ART_E_INVALID, "art_create: root_relief 0..255");
    ArtContext *c = new (std::nothrow) ArtContext();
    if (!c) return fail(ART_E_NOMEM, "art_create: out of memory");
    c->cfg = *cfg;
    if (c->cfg.morton_bits == 0) c->cfg.morton_bits = 63;
    c->device = dev;
    c->F = cfg->frames_in_flight == 0 ? 1 : cfg->frames_in_flight;
    hipError_t e = hipSetDevice(dev);
    for (uint32_t k = 0; k < c->F && e == hipSuccess; k++) {
        e = c->slot[k].own.acquire(c->device);
        if (e == hipSuccess) e = c->slot[k].done.create(hipEventDisableTiming);
        if (e == hipSuccess) e = c->slot[k].ao_ev[0].create();
        if (e == hipSuccess) e = c->slot[k].ao_ev[1].create();
    }
    for (int f = 0; f < ArtContext::kRing && e == hipSuccess; f++)
        for (int i = 0; i < 5 && e == hipSuccess; i++) e = c->ev[f][i].create();
    if (e != hipSuccess) { (void)art_destroy(c); return hipfail(e, "art_create"); } // the handles made so far go with the context
    c->W = cfg->width; c->H = cfg->height;
    // the fused packet frame is the default at every ring depth (one frame at a time: 0.575 ms against 0.669 ms for the staged per-ray
    // kernels, profiles/README.md r1h); art_set_tuning selects the other forms
    c->fast_trace = !(cfg->flags & ART_FLAG_FAST_BUILD);
    build_prewarm(c->main_stream()); sah_prewarm(c->main_stream());   // the builders' code objects are loaded here, once a process, not inside the first art_scene_build
    (void)hipGetLastError();
    *out = c;
    return ART_OK;
}

int32_t art_destroy(ArtContext *c) {
    if (!c) return ART_OK;
    (void)hipSetDevice(c->device);
    // everything the context put on the GPU is waited for, then every member releases what it owns (art_context.h: who owns what)
    for (uint32_t k = 0; k < c->F; k++) if (c->stream_of(k)) (void)hipStreamSynchronize(c->stream_of(k));
    drop_graphs(c);
    (void)cast_sync(c);   // (the casts on callers' streams too)
    (void)as_sync_streams(c);
    if (c->plan.plan_stream) (void)hipStreamSynchronize(c->plan.plan_stream);
    delete c;
    return ART_OK;
}

int32_t art_set_tuning(ArtContext *c, const ArtTuning *t) {
    if (!c || !t) return fail(ART_E_INVALID, "art_set_tuning: null argument");
    auto walk_ok = [](uint32_t k) { return k == 0 || k == 2 || k == 4; };
    if ((t->frame_form != 0 && t->frame_form != 2) || t->tree_builder > 1 || t->packet_wide > 2 || !walk_ok(t->primary_walk) || !walk_ok(t->shadow_walk) || !(walk_ok(t->ao_walk) || t->ao_walk == 6))
        return fail(ART_E_INVALID, "art_set_tuning: frame_form 0|2, tree_builder 0..1, packet_wide 0..2, primary_walk / shadow_walk 0|2|4, ao_walk 0|2|4|6");
    if (t->frame_form == 0 && (t->primary_walk || t->shadow_walk)) return fail(ART_E_INVALID, "art_set_tuning: the fused frame's rays are packets (primary_walk / shadow_walk choose the per-ray walks of frame_form 2)");
    if (t->as_versions > kMaxAsVersions || !(t->refit_rebuild_ratio == t->refit_rebuild_ratio)) return fail(ART_E_INVALID, "art_set_tuning: as_versions 0..24, refit_rebuild_ratio a number");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    drop_graphs(c);
    c->tuning = *t;
    c->fused = t->frame_form == 0;
    c->kind_primary = t->frame_form == 2 ? 2 : 8; c->kind_shadow = t->frame_form == 2 ? 4 : 8; c->kind_ao = 4;   // per-ray frames: binary nodes for primary rays, 4-wide for shadow rays
    if (t->primary_walk) c->kind_primary = (int)t->primary_walk;
    if (t->shadow_walk) c->kind_shadow = (int)t->shadow_walk;
    if (t->ao_walk) c->kind_ao = (int)t->ao_walk;
    c->fast_trace = !(c->cfg.flags & ART_FLAG_FAST_BUILD);
    c->tree_builder = t->tree_builder == 1 ? 1 : 3;
    c->packet_wide = t->packet_wide != 2;   // 0: the default (4-wide), 1: 4-wide, 2: binary
    c->shadow_hints = t->shadow_hints == 0;
    c->macro = t->block_order == 0 ? 2u : (t->block_order == 1 ? 0u : t->block_order);
    c->ao_entry = t->ao_entry_off == 0;
    c->wide_on_host = t->wide_builder == 1;
    c->built = false; c->frame_ready = false; c->traced = false;   // the tree and the frame layout are made again with the new choices
    return ART_OK;
}

int32_t art_set_stream(ArtContext *c, void *hip_stream) {
    if (!c) return fail(ART_E_INVALID, "art_set_stream: null context");
    if (hip_stream && c->F > 1) return fail(ART_E_STATE, "art_set_stream: a context with several frames in flight owns its streams (use art_stream_wait_frame / art_wait_external_event)");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    c->ext_stream = (hipStream_t)hip_stream;
    return ART_OK;
}

// The cull masks of the rays art_trace and art_trace_ao cast: kernel arguments, so a frame in flight keeps the ones it was launched with.
int32_t art_set_ray_masks(ArtContext *c, uint32_t primary, uint32_t shadow, uint32_t ao) {
    if (!c) return fail(ART_E_INVALID, "art_set_ray_masks: null context");
    if (primary > 0xFFu) return fail(ART_E_INVALID, "art_set_ray_masks: primary: above 0xFF");
    if (shadow > 0xFFu) return fail(ART_E_INVALID, "art_set_ray_masks: shadow: above 0xFF");
    if (ao > 0xFFu) return fail(ART_E_INVALID, "art_set_ray_masks: ao: above 0xFF");
    const uint32_t m = primary | (shadow << 8) | (ao << 16);
    if (m == c->ray_masks) return ART_OK;
    int32_t r = use_device(c); if (r) return r;
    drop_graphs(c);   // a captured frame holds the old masks
    c->ray_masks = m;
    return ART_OK;
}

int32_t art_set_camera(ArtContext *c, const ArtCamera *cam) {
    if (!c || !cam) return fail(ART_E_INVALID, "art_set_camera: null argument");
    if (!camera_finite(cam)) return fail(ART_E_INVALID, "art_set_camera: non-finite value in the camera block");
    if (!c->have_camera || std::memcmp(&c->camera, cam, sizeof(ArtCamera)) != 0) drop_graphs(c); // the camera block is a kernel argument
    if (!c->have_camera || std::memcmp(&c->camera, cam, sizeof(ArtCamera)) != 0) plan_hint_moved(c); // the heavy blocks move with the view
    c->camera = *cam; c->have_camera = true;
    for (uint32_t i = 0; i + 1 < kMaxBatch; i++) c->cam_more[i] = *cam; // every frame of a launch, until art_set_camera_batch says otherwise
    return ART_OK;
}

int32_t art_set_frames_per_launch(ArtContext *c, uint32_t n) {
    if (!c || n == 0 || n > kMaxBatch) return fail(ART_E_INVALID, "art_set_frames_per_launch: 1..4");
    if (n > 1 && !c->fused_frame()) return fail(ART_E_STATE, "art_set_frames_per_launch: only the fused frame traces several frames per launch");
    if (n == c->B) return ART_OK;
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    drop_graphs(c);
    c->B = n; c->read_b = 0; c->frame_ready = false; c->traced = false; // the per-slot buffers are laid out again, n frames each
    for (uint32_t k = 0; k < c->F; k++) { c->slot[k].ext_tiles = nullptr; c->slot[k].ext_ring_n = 0; c->slot[k].tiles_of_last = nullptr; c->slot[k].ext_tiles_bytes = 0; }
    return ART_OK;
}
int32_t art_set_camera_batch(ArtContext *c, const ArtCamera *cams, uint32_t n) {
    if (!c || !cams) return fail(ART_E_INVALID, "art_set_camera_batch: null argument");
    if (n != c->B) return fail(ART_E_INVALID, "art_set_camera_batch: one camera per frame of a launch (art_set_frames_per_launch)");
    for (uint32_t i = 1; i < n; i++) if (!camera_finite(&cams[i])) return fail(ART_E_INVALID, "art_set_camera_batch: non-finite value in a camera block");
    int32_t r = art_set_camera(c, &cams[0]); if (r) return r;
    for (uint32_t i = 1; i < n; i++) c->cam_more[i - 1] = cams[i];
    return ART_OK;
}
int32_t art_set_read_frame(ArtContext *c, uint32_t b) {
    if (!c || b >= c->B) return fail(ART_E_INVALID, "art_set_read_frame: frame >= frames per launch");
    c->read_b = b;
    return ART_OK;
}
int32_t art_camera_from_params(const float pos[3], const float dir[3], float aspect, float fovy, float znear, float zfar, ArtCamera *out) {
    if (!pos || !dir || !out) return fail(ART_E_INVALID, "art_camera_from_params: null argument");
    // VkCamera::set_dir normalises (vk_camera.rs:133-136); view = look_at_rh(pos, pos + dir, up = (0,-1,0)) (:182-189)
    float dn[3], tgt[3], f[3], s[3], u[3];
    normalize3(dir, dn);
    for (int k = 0; k < 3; k++) tgt[k] = (pos[k] + dn[k]) - pos[k];
    normalize3(tgt, f);
    const float up[3] = {0.0f, -1.0f, 0.0f};
    float sx[3]; cross3h(f, up, sx); normalize3(sx, s);
    cross3h(s, f, u);
    float *V = out->view;
    V[0] = s[0]; V[4] = s[1]; V[8] = s[2]; V[12] = -dot3h(s, pos);
    V[1] = u[0]; V[5] = u[1]; V[9] = u[2]; V[13] = -dot3h(u, pos);
    V[2] = -f[0]; V[6] = -f[1]; V[10] = -f[2]; V[14] = dot3h(f, pos);
    V[3] = 0; V[7] = 0; V[11] = 0; V[15] = 1;
    // proj = Perspective3::new(aspect, fovy, znear, zfar) (:191-193): OpenGL convention, z in [-1, 1]
    float *P = out->proj;
    std::memset(P, 0, 64);
    float cc = 1.0f / std::tan(fovy * 0.5f);
    P[0] = cc / aspect; P[5] = cc; P[10] = (zfar + znear) / (znear - zfar); P[14] = 2.0f * zfar * znear / (znear - zfar); P[11] = -1.0f;
    // (a direction along the up axis (0, -1, 0) has no side vector: look_at_rh's cross product is zero and the view matrix NaN -- an error here, where the reference would render NaN)
    if (!mat4_inverse(out->view, out->view_inv) || !mat4_inverse(out->proj, out->proj_inv)) return fail(ART_E_INVALID, "art_camera_from_params: singular or non-finite view / projection matrix (direction along the up axis, zero field of view, znear == zfar ...)");
    out->camera_pos[0] = pos[0]; out->camera_pos[1] = pos[1]; out->camera_pos[2] = pos[2];
    return ART_OK;
}

int32_t art_set_lights(ArtContext *c, const ArtLight *lights, uint32_t n) {
    if (!c || (n && !lights)) return fail(ART_E_INVALID, "art_set_lights: null argument");
    if (n > kMaxLightsTotal) return fail(ART_E_INVALID, "art_set_lights: more than 1024 lights");
    for (uint32_t i = 0; i < n; i++) if (lights[i].type > 3) return fail(ART_E_INVALID, "art_set_lights: unknown light type");
    int32_t r = use_device(c); if (r) return r;
    bool resized = n != c->lights.size();
    bool same = !resized && (n == 0 || std::memcmp(c->lights.data(), lights, (size_t)n * sizeof(ArtLight)) == 0);
    if (same) return ART_OK; // like VkLights' dirty flag (vk_lights.rs:81-139)
    c->lights.assign(lights, lights + n); c->lights_epoch++;
    plan_hint_moved(c); // the shadow walks change: look at the waves again
    if (resized) { r = sync_all(c); if (r) return r; } // the per-frame buffers are resized with the light count
    drop_graphs(c); // the records are kernel arguments (FrameArgs::lights): nothing to upload, and frames in flight keep the ones they were launched with
    if (resized) c->frame_ready = false;
    return ART_OK;
}

static void zero_light(ArtLight *l) { std::memset(l, 0, sizeof(*l)); }
static void cp3(float *d, const float *s) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; }

int32_t art_light_point(const float pos[3], const float color[3], float falloff, int32_t casts, ArtLight *o) { // lights.rs:144-159
    if (!pos || !color || !o) return fail(ART_E_INVALID, "art_light_point: null argument");
    zero_light(o); cp3(o->pos, pos); o->type = 0; o->casts_shadows = casts ? 1u : 0u; cp3(o->color, color); o->falloff_distance = falloff;
    return ART_OK;
}
int32_t art_light_spot(const float pos[3], const float dir[3], const float color[3], float falloff, float penumbra, float umbra, int32_t casts, ArtLight *o) { // lights.rs:228-243
    if (!pos || !dir || !color || !o) return fail(ART_E_INVALID, "art_light_spot: null argument");
    zero_light(o); cp3(o->pos, pos); o->type = 1; cp3(o->dir, dir); o->casts_shadows = casts ? 1u : 0u; cp3(o->color, color);
    o->falloff_distance = falloff; o->penumbra_angle = penumbra; o->umbra_angle = umbra;
    return ART_OK;
}
int32_t art_light_directional(const float dir[3], const float color[3], int32_t casts, ArtLight *o) { // lights.rs:281-296
    if (!dir || !color || !o) return fail(ART_E_INVALID, "art_light_directional: null argument");
    zero_light(o); o->type = 2; cp3(o->dir, dir); o->casts_shadows = casts ? 1u : 0u; cp3(o->color, color);
    return ART_OK;
}
int32_t art_light_area(const float pos[3], const float pos2[3], const float pos3[3], int32_t invert_normal, const float color[3], float falloff,
                       float penumbra, float umbra, int32_t casts, ArtLight *o) { // lights.rs:383-403
    if (!pos || !pos2 || !pos3 || !color || !o) return fail(ART_E_INVALID, "art_light_area: null argument");
    zero_light(o);
    float a[3] = {pos[0] - pos2[0], pos[1] - pos2[1], pos[2] - pos2[2]}, b[3] = {pos3[0] - pos2[0], pos3[1] - pos2[1], pos3[2] - pos2[2]}, n[3];
    cross3h(a, b, n);
    if (invert_normal) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    normalize3(n, n);
    cp3(o->pos, pos); o->type = 3; cp3(o->dir, n); o->casts_shadows = casts ? 1u : 0u; cp3(o->color, color); o->falloff_distance = falloff;
    cp3(o->area_pos2, pos2); o->penumbra_angle = penumbra; cp3(o->area_pos3, pos3); o->umbra_angle = umbra;
    return ART_OK;
}

int32_t art_resize(ArtContext *c, uint32_t w, uint32_t h) {
    if (!c || w == 0 || h == 0 || w > 16384 || h > 16384) return fail(ART_E_INVALID, "art_resize: bad extent");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    c->W = w; c->H = h; c->frame_ready = false; c->traced = false;
    return ART_OK;
}

static FrameArgs make_frame_args(ArtContext *c, FrameSlot &S, uint32_t version) {
    FrameArgs a{};
    static_assert(sizeof(CameraArg) == sizeof(ArtCamera), "camera block layout");
    std::memcpy(&a.cam, &c->camera, sizeof(ArtCamera));
    a.W = c->W; a.H = c->H; a.tile_list = c->d_tile_list.p; a.n_tiles_owned = (uint32_t)c->tile_list.size(); a.tiles_x = c->tiles_x; a.n_local = c->n_local; a.block_order = c->d_block_order.p;
    const AsPtrs as = as_ptrs(c, version); // the version of the acceleration structure this launch reads
    a.nodes = c->bvh.nodes; a.wide = as.wide; a.widef = as.widef; a.packet_wide = c->packet_wide; a.trace_kind[0] = c->kind_primary; a.trace_kind[1] = c->kind_shadow; a.trace_kind[2] = c->kind_ao; a.tune = c->trace_tune(); a.pipelined = c->F > 1; a.tris = as.tris; a.shade_tris = as.shade; a.prims = as.prims; a.tex_pool = c->d_tex.p;
    a.n_lights = (uint32_t)c->lights.size();
    const uint32_t n_arg = std::min(a.n_lights, (uint32_t)kMaxLights);
    if (n_arg) std::memcpy(a.lights, c->lights.data(), (size_t)n_arg * sizeof(ArtLight));
    for (uint32_t i = 0; i < n_arg; i++) directional_constants(a.lights[i]);
    a.lights_more = a.n_lights > (uint32_t)kMaxLights ? S.d_lights_more.p : nullptr;   // (art_trace brings the slot's table up to date: lights_upload)
    a.pix_more = (a.n_lights > (uint32_t)kMaxLights && c->fused) ? S.d_pix_more.p : nullptr;
    a.hits = S.d_hits.p; a.contrib = S.d_contrib.p; a.shadow_rays = S.d_shadow_rays.p; a.counters = S.d_counters.p;
    a.color = S.d_color.p; a.depth = S.d_depth.p; a.normal = S.d_normal.p;
    a.color_tiles = c->tiled() ? S.last_tiles() : nullptr; a.tiles_packed = c->tiles_packed(); // art_trace picks the frame's buffer (tiles_for)
    a.shadow_bits = (c->cfg.flags & ART_FLAG_KEEP_DEBUG) ? S.d_shadow_bits.p : nullptr;
    a.pix_bits = S.d_shadow_bits.p; a.keep_hits = (c->cfg.flags & ART_FLAG_KEEP_DEBUG) != 0;
    a.batch = c->B; a.tiles_stride = c->padded_tiles * kTilePixels;
    for (uint32_t i = 0; i + 1 < kMaxBatch; i++) std::memcpy(&a.cam_more[i], &c->cam_more[i], sizeof(ArtCamera));
    a.tile_xy = c->d_tile_xy.p; a.wave_items = c->plan.d_items[c->plan.cur].p; a.n_wave_items = c->plan.n_items[c->plan.cur]; a.wave_cost = nullptr; // art_trace sets it for the frames the wave plan samples
    // the filtered instances run while the scene needs them (alpha_live) or some ray type's cull mask is 0 (such rays see nothing, and no leaf bit says so)
    const uint32_t rm = c->ray_masks;
    a.ray_masks = rm;
    a.alpha = c->alpha_live || (rm & 0xFFu) == 0u || ((rm >> 8) & 0xFFu) == 0u || ((rm >> 16) & 0xFFu) == 0u;
    a.alpha_bits = c->d_alpha_bits.p;   // (art_trace_ao: the frame's own choice, FrameSlot::alpha and ::ray_masks)
    a.hints = c->shadow_hints ? c->d_hints.p : nullptr; a.hint_leaves = c->T;
    a.plain_math = c->tuning.plain_math != 0;
    return a;
}

// more than 16 lights: ring slot S's table of records 16.. as of the current list, on the slot's stream (in front of the frame that reads it)
static int32_t lights_upload(ArtContext *c, FrameSlot &S, hipStream_t s) {
    const size_t n = c->lights.size();
    if (n <= (size_t)kMaxLights || S.lights_epoch == c->lights_epoch) return ART_OK;
    const size_t m = n - kMaxLights;
    if (S.lights_ev_set) HIPC(hipEventSynchronize(S.lights_ev));   // the upload that read the staging copy last
    HIPC(S.h_lights_more.ensure(m));
    if (S.d_lights_more.n < m) { HIPC(hipStreamSynchronize(s)); HIPC(S.d_lights_more.ensure(m)); }   // (frames of this slot still read the old table)
    std::memcpy(S.h_lights_more.p, c->lights.data() + kMaxLights, m * sizeof(ArtLight));
    for (size_t i = 0; i < m; i++) directional_constants(S.h_lights_more.p[i]);
    HIPC(hipMemcpyAsync(S.d_lights_more.p, S.h_lights_more.p, m * sizeof(ArtLight), hipMemcpyHostToDevice, s));
    HIPC(S.lights_ev.create(hipEventDisableTiming));
    HIPC(hipEventRecord(S.lights_ev, s)); S.lights_ev_set = true;
    S.lights_epoch = c->lights_epoch;
    return ART_OK;
}

int32_t art_trace(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_trace: null context");
    if (!c->built) return fail(ART_E_STATE, "art_trace: scene not built (art_scene_build)");
    if (!c->have_camera) return fail(ART_E_STATE, "art_trace: no camera (art_set_camera)");
    if (c->W == 0 || c->H == 0) return fail(ART_E_STATE, "art_trace: zero extent (art_resize)");
    int32_t r = use_device(c); if (r) return r;
    if (!c->frame_ready) { r = sync_all(c); if (r) return r; r = setup_frame(c); if (r) return r; }
    const uint32_t k = (uint32_t)(c->frame_no % c->F);
    FrameSlot &S = c->slot[k];
    hipStream_t s = c->stream_of(k);
    if (S.wait_event) { HIPC(hipStreamWaitEvent(s, (hipEvent_t)S.wait_event, 0)); S.wait_event = nullptr; }
    if (as_pending(c)) { r = scene_refresh(c, k, s); if (r) return r; } // a model moved: the refit this frame is ordered behind (past the cost threshold: a rebuild)
    r = ensure_wide(c, c->kind_primary == 4 || c->kind_shadow == 4 || c->packet_wide); if (r) return r;
    r = ensure_binary(c, !c->packet_wide || c->kind_primary == 2 || c->kind_shadow == 2); if (r) return r;
    if (c->plan.enabled) { r = plan_poll(c); if (r) return r; }
    const uint32_t ver = as_current(c);
    r = as_wait_ready(c, ver, s, k); if (r) return r;   // the refit that wrote this version may still run on another ring slot's stream
    as_frame_reads(c, ver, k);
    S.as_version = ver;
    r = lights_upload(c, S, s); if (r) return r;
    FrameArgs a = make_frame_args(c, S, ver);
    S.alpha = a.alpha; S.ray_masks = a.ray_masks;
    if (c->tiled()) a.color_tiles = S.tiles_for(c->frame_no, c->F); // alternates when a pair of buffers is bound
    const bool fused = c->fused_frame();
    if (c->B > 1 && !fused) return fail(ART_E_STATE, "art_trace: several frames per launch need the default fused frame");
    const Event *ev = c->ev[c->frame_no % ArtContext::kRing];
    c->ev_fused[c->frame_no % ArtContext::kRing] = fused;
    auto submitted = [&]() { S.ao_valid = false; S.presented = false; c->last = k; c->frame_no++; c->traced = true; return ART_OK; };   // the frame is in slot k's queue
    if (c->graph_mode && !fused && S.ext_ring_n < 2) { // a fused frame is a single launch: nothing for a graph to save; alternating tile buffers change a kernel argument
        if (!S.graph) { // capture the frame once per slot; stage events are not part of it
            hipGraph_t g = nullptr;
            HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            hipError_t e = hipMemsetAsync(S.d_counters.p, 0, kCounterWords * 4, s);
            if (e == hipSuccess && a.n_local) { launch_primary(a, s); launch_shade(a, s); launch_shadow(a, s); launch_accumulate(a, s); e = hipGetLastError(); }
            hipError_t e2 = hipStreamEndCapture(s, &g);
            if (e != hipSuccess || e2 != hipSuccess) { if (g) (void)hipGraphDestroy(g); return hipfail(e != hipSuccess ? e : e2, "art_trace: graph capture"); }
            e = hipGraphInstantiate(&S.graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) { S.graph = nullptr; return hipfail(e, "hipGraphInstantiate"); }
        }
        for (int i = 0; i < 4; i++) HIPC(hipEventRecord(ev[i], s));
        HIPC(hipGraphLaunch(S.graph, s));
        HIPC(hipEventRecord(ev[4], s));
        HIPC(hipEventRecord(S.done, s)); S.done_alias = nullptr;
        return submitted();
    }
    if (fused) { // one launch; its time is booked on the first stage
        HIPC(hipEventRecord(ev[0], s));
        if (plan_want_sample(c, a.n_wave_items)) a.wave_cost = S.d_wave_cost.p;
        const bool counted = a.n_local ? launch_frame(a, s) : false;
        HIPC(hipEventRecord(ev[4], s));
        S.done_alias = ev[4];           // also the frame's completion event (a record is a packet in the frame's queue: 1/8 share 33 -> 29 us)
        HIPC(hipGetLastError());
        if (counted) { r = plan_launch(c, a, ev[4]); if (r) return r; } // now and then a frame counts its waves' packet steps: the next plan is made from them, behind the frame, on the device
        return submitted();
    }
    S.done_alias = nullptr;
    HIPC(hipMemsetAsync(S.d_counters.p, 0, kCounterWords * 4, s));   // the staged frame's work cursors and count slots
    HIPC(hipEventRecord(ev[0], s));
    if (a.n_local) launch_primary(a, s);
    HIPC(hipEventRecord(ev[1], s));
    if (a.n_local) launch_shade(a, s);
    HIPC(hipEventRecord(ev[2], s));
    if (a.n_local) launch_shadow(a, s);
    HIPC(hipEventRecord(ev[3], s));
    if (a.n_local) launch_accumulate(a, s);
    HIPC(hipEventRecord(ev[4], s));
    HIPC(hipEventRecord(S.done, s));
    HIPC(hipGetLastError());
    return submitted();
}

int32_t art_sync(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_sync: null context");
    int32_t r = use_device(c); if (r) return r;
    return sync_all(c);
}

int32_t art_trace_ao(ArtContext *c, uint32_t spp, float radius) {
    if (!c) return fail(ART_E_INVALID, "art_trace_ao: null context");
    if (!c->traced || !c->frame_ready) return fail(ART_E_STATE, "art_trace_ao: call art_trace first (AO consumes that frame's depth + normal outputs)");
    if (spp == 0 || spp > 64 || !(radius > 0.0f)) return fail(ART_E_INVALID, "art_trace_ao: spp must be 1..64 and radius > 0");
    if (c->B > 1) return fail(ART_E_STATE, "art_trace_ao: not with several frames per launch");
    int32_t r = use_device(c); if (r) return r;
    r = ensure_wide(c, c->kind_ao == 4 || c->kind_ao == 6); if (r) return r;
    FrameSlot &S = c->slot[c->last];
    hipStream_t s = c->stream_of(c->last);
    const size_t n_occl = (size_t)c->n_local * (((spp + 3u) >> 2) * 4u); // one byte per slot of the per-ray tracer: groups of four samples (art_trace.hip ao_slot_decode)
    if (S.d_occl.n < n_occl || S.d_ao.n < (size_t)c->W * c->H || S.d_ao_pix.n < 2 * (size_t)c->n_local) {
        HIPC(hipStreamSynchronize(s));
        HIPC(S.d_occl.ensure(n_occl)); HIPC(S.d_ao.ensure((size_t)c->W * c->H)); HIPC(S.d_ao_pix.ensure(2 * (size_t)c->n_local));
        HIPC(hipMemset(S.d_ao.p, 0, (size_t)c->W * c->H * 4)); HIPC(hipDeviceSynchronize());
    }
    if (c->ao_tab_spp != spp) { // the sample directions in the tangent frame: a function of (sample, position in the 64x64 noise tile) only
        r = sync_all(c); if (r) return r;
        HIPC(c->d_ao_tab.ensure((size_t)spp * kAoTableEntriesPerSample));
        launch_ao_table(spp, c->d_ao_tab.p, c->main_stream());
        HIPC(hipGetLastError()); HIPC(hipStreamSynchronize(c->main_stream()));
        c->ao_tab_spp = spp;
    }
    uint32_t lut[65] = {0};
    for (uint32_t k = 0; k <= spp; k++) lut[k] = (uint32_t)(std::pow(1.0 - (double)k / (double)spp, 2.2) * 255.0 + 0.5); // XE_GTAO_DEFAULT_FINAL_VALUE_POWER (vk_xe_gtao.rs:22)
    r = ensure_binary(c, c->kind_ao == 2); if (r) return r;
    FrameArgs a = make_frame_args(c, S, S.as_version); // the structure the frame itself was traced in
    a.alpha = S.alpha; a.ray_masks = S.ray_masks;       // (and the cutoffs and masks of that version's table, and the cull masks that were current at the frame's art_trace)
    as_aux_behind(c, S.as_version, c->last);
    HIPC(hipMemsetAsync(S.d_counters.p + 64 + 16 * 32, 0, 8 * 32 * 4, s)); // the AO launch's work cursors
    HIPC(hipEventRecord(S.ao_ev[0], s));
    if (a.n_local) launch_ao(a, spp, radius, S.d_occl.p, S.d_ao_pix.p, c->d_ao_tab.p, c->ao_entry, S.d_ao.p, lut, s);
    HIPC(hipEventRecord(S.ao_ev[1], s));
    HIPC(hipEventRecord(S.done, s)); S.done_alias = nullptr;
    HIPC(hipGetLastError());
    c->stats.ao_rays = 0; c->ao_spp = spp; S.ao_valid = true;
    return ART_OK;
}

int32_t art_present(ArtContext *c) {
    if (!c) return fail(ART_E_INVALID, "art_present: null context");
    if (!c->traced || !c->frame_ready) return fail(ART_E_STATE, "art_present: call art_trace first");
    if (c->B > 1) return fail(ART_E_STATE, "art_present: not with several frames per launch");
    int32_t r = use_device(c); if (r) return r;
    FrameSlot &S = c->slot[c->last];
    hipStream_t s = c->stream_of(c->last);
    size_t npix = (size_t)c->W * c->H;
    if (S.d_bgra.n < npix) { HIPC(hipStreamSynchronize(s)); HIPC(S.d_pcolor.ensure(npix)); HIPC(S.d_pnormal.ensure(npix)); HIPC(S.d_bgra.ensure(npix)); HIPC(S.d_pdepth.ensure(npix)); }
    uint32_t ctl[96];
    const float sat[3] = {0.0f, 0.0f, 0.0f}, ct[3] = {1.0f, 0.5f, 1.0f / 32.0f};
    lpm_control_block(false, 0.0f, 256.0f, 8.0f, 0.25f, 1.0f, sat, ct, ctl); // the parameters of vk_tonemap.rs:417-426
    launch_present((uint32_t)npix, S.d_color.p, S.d_normal.p, S.d_depth.p, S.ao_valid ? S.d_ao.p : nullptr, ctl, S.d_pcolor.p, S.d_pnormal.p, S.d_pdepth.p, S.d_bgra.p, s);
    HIPC(hipEventRecord(S.done, s)); S.done_alias = nullptr;
    HIPC(hipGetLastError());
    S.presented = true;
    return ART_OK;
}
int32_t art_lpm_control_block(int32_t shoulder, float soft_gap, float hdr_max, float exposure, float contrast, float shoulder_contrast, const float saturation[3],
                              const float crosstalk[3], uint32_t ctl[96]) {
    if (!saturation || !crosstalk || !ctl) return fail(ART_E_INVALID, "art_lpm_control_block: null argument");
    lpm_control_block(shoulder != 0, soft_gap, hdr_max, exposure, contrast, shoulder_contrast, saturation, crosstalk, ctl);
    return ART_OK;
}

int32_t art_read_color(ArtContext *c, void *dst, size_t bytes) { return read_image(c, &FrameSlot::d_color, dst, bytes, "art_read_color"); }
int32_t art_read_depth(ArtContext *c, void *dst, size_t bytes) { return read_image(c, &FrameSlot::d_depth, dst, bytes, "art_read_depth"); }
int32_t art_read_normal(ArtContext *c, void *dst, size_t bytes) { return read_image(c, &FrameSlot::d_normal, dst, bytes, "art_read_normal"); }

int32_t art_read_ao(ArtContext *c, void *dst, size_t bytes) {
    if (c && c->ao_spp == 0) return fail(ART_E_STATE, "art_read_ao: art_trace_ao has not run");
    return read_back(c, c ? c->slot[c->last].d_ao.p : nullptr, c ? (size_t)c->W * c->H * 4 : 0, dst, bytes, "art_read_ao");
}
static int32_t need_present(ArtContext *c, const char *who) {
    if (c && !c->slot[c->last].presented) return fail(ART_E_STATE, std::string(who) + ": art_present has not run for the latest frame");
    return ART_OK;
}
int32_t art_read_present(ArtContext *c, void *dst, size_t bytes) {
    int32_t r = need_present(c, "art_read_present"); if (r) return r;
    return read_back(c, c ? c->slot[c->last].d_bgra.p : nullptr, c ? (size_t)c->W * c->H * 4 : 0, dst, bytes, "art_read_present");
}
int32_t art_read_packed(ArtContext *c, void *color_b10g11r11, void *normal_b10g11r11, void *depth_f16) {
    int32_t r = need_present(c, "art_read_packed"); if (r) return r;
    if (!c) return fail(ART_E_INVALID, "art_read_packed: null context");
    size_t npix = (size_t)c->W * c->H;
    if (color_b10g11r11) { r = read_back(c, c->slot[c->last].d_pcolor.p, npix * 4, color_b10g11r11, npix * 4, "art_read_packed"); if (r) return r; }
    if (normal_b10g11r11) { r = read_back(c, c->slot[c->last].d_pnormal.p, npix * 4, normal_b10g11r11, npix * 4, "art_read_packed"); if (r) return r; }
    if (depth_f16) { r = read_back(c, c->slot[c->last].d_pdepth.p, npix * 2, depth_f16, npix * 2, "art_read_packed"); if (r) return r; }
    return ART_OK;
}
int32_t art_device_color(ArtContext *c, void **p, size_t *b) { return device_image(c, &FrameSlot::d_color, p, b, "art_device_color"); }
int32_t art_device_depth(ArtContext *c, void **p, size_t *b) { return device_image(c, &FrameSlot::d_depth, p, b, "art_device_depth"); }
int32_t art_device_normal(ArtContext *c, void **p, size_t *b) { return device_image(c, &FrameSlot::d_normal, p, b, "art_device_normal"); }

int32_t art_shard_layout(uint32_t width, uint32_t height, uint32_t shard_count, uint32_t shard_rank, uint32_t root_relief, uint32_t *tiles, uint32_t cap, uint32_t *owned, uint32_t *padded) {
    if (width == 0 || height == 0) return fail(ART_E_INVALID, "art_shard_layout: zero extent");
    if (root_relief > 255) return fail(ART_E_INVALID, "art_shard_layout: root_relief 0..255");
    uint32_t count = shard_count > 1 ? shard_count : 1;
    if (shard_rank >= count) return fail(ART_E_INVALID, "art_shard_layout: shard_rank >= shard_count");
    uint32_t tx_n = (width + kTile - 1) / kTile, ty_n = (height + kTile - 1) / kTile, mine = 0;
    if (count > 255) return fail(ART_E_INVALID, "art_shard_layout: at most 255 shards");
    std::vector<uint32_t> per(count, 0);
    const std::vector<uint8_t> owner_of = shard_owner_table(tx_n, ty_n, count, root_relief);
    for (uint32_t ty = 0; ty < ty_n; ty++)
        for (uint32_t tx = 0; tx < tx_n; tx++) {
            uint32_t o = owner_of[(size_t)ty * tx_n + tx];
            per[o]++;
            if (o == shard_rank) { if (tiles && mine < cap) tiles[mine] = ty * tx_n + tx; mine++; }
        }
    if (tiles && mine > cap) return fail(ART_E_INVALID, "art_shard_layout: tiles buffer too small");
    uint32_t mx = 0; for (uint32_t v : per) mx = v > mx ? v : mx;
    if (owned) *owned = mine;
    if (padded) *padded = mx;
    return ART_OK;
}
int32_t art_shard_tile_count(ArtContext *c, uint32_t *owned, uint32_t *padded) {
    if (!c) return fail(ART_E_INVALID, "art_shard_tile_count: null context");
    int32_t r = ensure_layout(c, "art_shard_tile_count"); if (r) return r;
    if (owned) *owned = (uint32_t)c->tile_list.size();
    if (padded) *padded = c->padded_tiles;
    return ART_OK;
}
int32_t art_device_color_tiles(ArtContext *c, void **p, size_t *b) {
    int32_t r = device_ready(c, p, "art_device_color_tiles"); if (r) return r;
    *p = nullptr; if (b) *b = 0;
    if (!c->tiled()) return fail(ART_E_STATE, "art_device_color_tiles: context is not sharded");
    FrameSlot &S = c->slot[c->last];
    const size_t one = c->tiles_bytes();
    *p = (char *)S.last_tiles() + c->read_b * one; if (b) *b = one;
    return ART_OK;
}
int32_t art_bind_color_tiles(ArtContext *c, uint32_t slot, void *dev, size_t bytes) {
    if (!c) return fail(ART_E_INVALID, "art_bind_color_tiles: null context");
    if (!c->tiled()) return fail(ART_E_STATE, "art_bind_color_tiles: context is not sharded");
    if (slot >= c->F) return fail(ART_E_INVALID, "art_bind_color_tiles: slot >= frames in flight");
    int32_t r = ensure_layout(c, "art_bind_color_tiles"); if (r) return r;
    if (dev && bytes != c->tiles_bytes() * c->B) return fail(ART_E_INVALID, "art_bind_color_tiles: size mismatch (padded tiles x tile bytes x frames per launch)");
    HIPC(hipStreamSynchronize(c->stream_of(slot)));
    c->slot[slot].ext_tiles = (float4 *)dev; c->slot[slot].ext_ring_n = 0; c->slot[slot].tiles_of_last = nullptr; c->slot[slot].ext_tiles_bytes = dev ? bytes : 0;
    drop_graphs(c);
    return ART_OK;
}
int32_t art_bind_color_tiles_pair(ArtContext *c, uint32_t slot, void *dev_even, void *dev_odd, size_t bytes) {
    if (!dev_even || !dev_odd) return fail(ART_E_INVALID, "art_bind_color_tiles_pair: null buffer");
    void *two[2] = {dev_even, dev_odd};
    return art_bind_color_tiles_ring(c, slot, two, 2, bytes);
}
int32_t art_bind_color_tiles_ring(ArtContext *c, uint32_t slot, void *const *bufs, uint32_t n, size_t bytes) {
    if (!bufs || n == 0 || n > FrameSlot::kTileRing) return fail(ART_E_INVALID, "art_bind_color_tiles_ring: 1..8 buffers");
    for (uint32_t i = 0; i < n; i++) if (!bufs[i]) return fail(ART_E_INVALID, "art_bind_color_tiles_ring: null buffer");
    int32_t r = art_bind_color_tiles(c, slot, bufs[0], bytes); if (r) return r;
    for (uint32_t i = 0; i < n; i++) c->slot[slot].ext_ring[i] = (float4 *)bufs[i];
    c->slot[slot].ext_ring_n = n;
    return ART_OK;
}
int32_t art_set_graph_mode(ArtContext *c, int32_t on) {
    if (!c) return fail(ART_E_INVALID, "art_set_graph_mode: null context");
    if (on && c->ext_stream) return fail(ART_E_STATE, "art_set_graph_mode: not with an external stream");
    c->graph_mode = on != 0;
    if (!on) drop_graphs(c);
    return ART_OK;
}
int32_t art_frames_in_flight(ArtContext *c, uint32_t *frames, uint32_t *next_slot) {
    if (!c) return fail(ART_E_INVALID, "art_frames_in_flight: null context");
    if (frames) *frames = c->F;
    if (next_slot) *next_slot = (uint32_t)(c->frame_no % c->F);
    return ART_OK;
}
int32_t art_frames_done(ArtContext *c, uint64_t first, uint32_t count, int32_t *done, uint64_t *traced) {
    if (!c || !done) return fail(ART_E_INVALID, "art_frames_done: null argument");
    if (traced) *traced = c->frame_no;
    *done = 0;
    if (count == 0) { *done = 1; return ART_OK; }
    if (first + count > c->frame_no) return fail(ART_E_INVALID, "art_frames_done: frames not traced yet");
    if (c->frame_no - first > (uint64_t)ArtContext::kRing) return fail(ART_E_INVALID, "art_frames_done: older than the 128 frames whose events are kept");
    int32_t r = use_device(c); if (r) return r;
    for (uint64_t f = first + count; f-- > first;) { // the newest first: it is the likeliest to be still running
        hipError_t e = hipEventQuery(c->ev[f % ArtContext::kRing][4]);
        if (e == hipErrorNotReady) return ART_OK;
        if (e != hipSuccess) return hipfail(e, "art_frames_done: hipEventQuery");
    }
    *done = 1;
    return ART_OK;
}
int32_t art_stream_wait_frame(ArtContext *c, void *hip_stream) {
    if (!c) return fail(ART_E_INVALID, "art_stream_wait_frame: null context");
    if (!c->traced) return fail(ART_E_STATE, "art_stream_wait_frame: nothing traced yet");
    int32_t r = use_device(c); if (r) return r;
    { FrameSlot &S = c->slot[c->last]; HIPC(hipStreamWaitEvent((hipStream_t)hip_stream, S.done_alias ? S.done_alias : S.done, 0)); }
    return ART_OK;
}
int32_t art_trace_for_stream(ArtContext *c, void *hip_stream, uint32_t *slot_used) {
    if (!c) return fail(ART_E_INVALID, "art_trace_for_stream: null context");
    const uint32_t k = (uint32_t)(c->frame_no % c->F);
    int32_t r = art_trace(c); if (r) return r;
    if (slot_used) *slot_used = k;
    return art_stream_wait_frame(c, hip_stream);
}
int32_t art_wait_external_event(ArtContext *c, void *hip_event) {
    if (!c) return fail(ART_E_INVALID, "art_wait_external_event: null context");
    c->slot[c->frame_no % c->F].wait_event = hip_event;
    return ART_OK;
}
int32_t art_collect_timings(ArtContext *c, float sums_ms[5], uint32_t *n_frames) {
    if (!c || !sums_ms || !n_frames) return fail(ART_E_INVALID, "art_collect_timings: null argument");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    uint64_t from = c->collected_upto;
    if (c->frame_no - from > (uint64_t)ArtContext::kRing) from = c->frame_no - ArtContext::kRing;
    for (int k = 0; k < 5; k++) sums_ms[k] = 0.f;
    for (uint64_t f = from; f < c->frame_no; f++) {
        const Event *ev = c->ev[f % ArtContext::kRing];
        float ms = 0;
        if (c->ev_fused[f % ArtContext::kRing]) { HIPC(hipEventElapsedTime(&ms, ev[0], ev[4])); sums_ms[0] += ms; sums_ms[4] += ms; continue; } // one launch: booked on the first stage
        for (int k = 0; k < 4; k++) { HIPC(hipEventElapsedTime(&ms, ev[k], ev[k + 1])); sums_ms[k] += ms; }
        HIPC(hipEventElapsedTime(&ms, ev[0], ev[4])); sums_ms[4] += ms;
    }
    *n_frames = (uint32_t)(c->frame_no - from);
    c->collected_upto = c->frame_no;
    return ART_OK;
}
int32_t art_read_color_tiles(ArtContext *c, void *dst, size_t bytes) {
    if (c && !c->tiled()) return fail(ART_E_STATE, "art_read_color_tiles: context is not sharded");
    FrameSlot *S = c ? &c->slot[c->last] : nullptr;
    const size_t one = c ? c->tiles_bytes() : 0;
    return read_back(c, S ? (const char *)S->last_tiles() + c->read_b * one : nullptr, one, dst, bytes, "art_read_color_tiles");
}
int32_t art_untile_gathered_frames(ArtContext *c, const void *gathered_dev, uint32_t shard_count, uint32_t shard_stride_tiles, uint32_t n_frames, void *frames_dev, void *hip_stream) {
    if (!c || !gathered_dev) return fail(ART_E_INVALID, "art_untile_gathered: null argument");
    int32_t r = ensure_layout(c, "art_untile_gathered"); if (r) return r;   // (first: until the frame is laid out padded_tiles is 0 and the two checks below pass whatever they are given)
    if (shard_stride_tiles < c->padded_tiles) return fail(ART_E_INVALID, "art_untile_gathered: stride smaller than a shard's padded tile count");
    if (n_frames == 0 || (n_frames > 1 && (!frames_dev || (uint64_t)n_frames * c->padded_tiles > shard_stride_tiles))) return fail(ART_E_INVALID, "art_untile_gathered_frames: frames do not fit the shard stride (or no output given)");
    if (shard_count != (c->cfg.shard_count > 1 ? c->cfg.shard_count : 1)) return fail(ART_E_INVALID, "art_untile_gathered: shard_count differs from the context's");
    r = use_device(c); if (r) return r;
    hipStream_t us = hip_stream ? (hipStream_t)hip_stream : c->stream_of(c->last);
    if (c->tiles_packed()) { // the gathered tiles are B10G11R11 words: the frame is the packed colour image (art_read_packed)
        FrameSlot &S = c->slot[c->last];
        if (!frames_dev && S.d_pcolor.n < (size_t)c->W * c->H) { HIPC(hipStreamSynchronize(us)); HIPC(S.d_pcolor.ensure((size_t)c->W * c->H)); }
        launch_untile_packed((const uint32_t *)gathered_dev, c->d_tile_slot.p, shard_stride_tiles, n_frames, c->padded_tiles, c->W, c->H, frames_dev ? (uint32_t *)frames_dev : S.d_pcolor.p, us);
    } else
    launch_untile((const float4 *)gathered_dev, c->d_tile_slot.p, shard_stride_tiles, n_frames, c->padded_tiles, c->W, c->H, frames_dev ? (float4 *)frames_dev : c->slot[c->last].d_color.p, us);
    HIPC(hipGetLastError());
    c->traced = true;
    return ART_OK;
}
int32_t art_untile_gathered_strided(ArtContext *c, const void *gathered_dev, uint32_t shard_count, uint32_t shard_stride_tiles, void *frame_dev, void *hip_stream) {
    return art_untile_gathered_frames(c, gathered_dev, shard_count, shard_stride_tiles, 1, frame_dev, hip_stream);
}
int32_t art_untile_gathered(ArtContext *c, const void *gathered_dev, uint32_t shard_count, void *frame_dev, void *hip_stream) {
    if (!c) return fail(ART_E_INVALID, "art_untile_gathered: null argument");
    int32_t r = ensure_layout(c, "art_untile_gathered"); if (r) return r;   // (padded_tiles is the stride: 0 until the frame is laid out)
    return art_untile_gathered_strided(c, gathered_dev, shard_count, c->padded_tiles, frame_dev, hip_stream);
}

int32_t art_get_layout(ArtContext *c, ArtLayout *out) {
    if (!c || !out) return fail(ART_E_INVALID, "art_get_layout: null argument");
    int32_t r = ensure_layout(c, "art_get_layout"); if (r) return r;
    std::memset(out, 0, sizeof(*out));
    out->width = c->W; out->height = c->H; out->frames_in_flight = c->F; out->frames_per_launch = c->B;
    out->shard_rank = c->cfg.shard_count > 1 ? c->cfg.shard_rank : 0; out->shard_count = c->cfg.shard_count > 1 ? c->cfg.shard_count : 1;
    out->tiles_owned = (uint32_t)c->tile_list.size(); out->tiles_padded = c->padded_tiles; out->tile_bytes = c->tiled() ? (uint32_t)(kTilePixels * c->tile_px_bytes()) : 0u; // 0: no compact tile buffer
    return ART_OK;
}
int32_t art_timestamp_mark(ArtContext *c, uint32_t which) {
    if (!c || which > 1) return fail(ART_E_INVALID, "art_timestamp_mark: mark 0 or 1");
    if (!c->traced) return fail(ART_E_STATE, "art_timestamp_mark: nothing traced yet");
    int32_t r = use_device(c); if (r) return r;
    HIPC(c->mark[which].create());
    HIPC(hipEventRecord(c->mark[which], c->stream_of(c->last)));
    return ART_OK;
}
int32_t art_timestamp_elapsed(ArtContext *c, float *ms) {
    if (!c || !ms) return fail(ART_E_INVALID, "art_timestamp_elapsed: null argument");
    if (!c->mark[0] || !c->mark[1]) return fail(ART_E_STATE, "art_timestamp_elapsed: both marks must have been recorded");
    int32_t r = use_device(c); if (r) return r;
    HIPC(hipEventSynchronize(c->mark[1]));
    HIPC(hipEventElapsedTime(ms, c->mark[0], c->mark[1]));
    return ART_OK;
}

int32_t art_get_stats(ArtContext *c, ArtStats *out) {
    if (!c || !out) return fail(ART_E_INVALID, "art_get_stats: null argument");
    if (c->traced && c->frame_ready) {
        int32_t r = use_device(c); if (r) return r;
        r = sync_all(c); if (r) return r;
        std::vector<uint32_t> raw(kCounterWords);
        if (c->fused_frame()) { // fused frames keep no counters: count from the frame's per-pixel bits + depth, here
            FrameSlot &S = c->slot[c->last];
            HIPC(hipMemsetAsync(S.d_counters.p, 0, kCounterWords * 4, c->stream_of(c->last)));
            if (c->n_local) { // of the frame the read calls refer to
                FrameArgs fa = make_frame_args(c, S, S.as_version);
                fa.pix_bits += (size_t)c->read_b * c->n_local; fa.depth += (size_t)c->read_b * c->W * c->H;
                launch_frame_stats(fa, S.d_counters.p, c->stream_of(c->last)); HIPC(hipGetLastError());
            }
            HIPC(hipStreamSynchronize(c->stream_of(c->last)));
        }
        HIPC(hipMemcpy(raw.data(), c->slot[c->last].d_counters.p, kCounterWords * 4, hipMemcpyDeviceToHost));
        uint64_t cnt[2] = {raw[0], raw[1]}; // folded totals (packet frames) + the slots (per-ray frames): one of the two is zero
        for (uint32_t k = 0; k < kSlotCount; k++) { cnt[0] += raw[kShadowSlots + k * kSlotStride]; cnt[1] += raw[kHitSlots + k * kSlotStride]; }
        uint64_t owned = 0; // pixels of owned tiles that fall inside the frame
        for (uint32_t t : c->tile_list) {
            uint32_t tx = t % c->tiles_x, ty = t / c->tiles_x;
            uint32_t w = (tx + 1) * kTile <= c->W ? kTile : c->W - tx * kTile, h = (ty + 1) * kTile <= c->H ? kTile : c->H - ty * kTile;
            owned += (uint64_t)w * h;
        }
        c->stats.primary_rays = owned; c->stats.shadow_rays = cnt[0]; c->stats.hit_pixels = cnt[1];
        c->stats.frame_launches = c->fused_frame() ? 1u : 4u;
        c->stats.split_blocks = c->plan.split1 + c->plan.split2;
        harvest_cost(c);
        c->stats.ao_rays = (uint64_t)c->ao_spp * cnt[1];
        if (c->ao_spp && c->slot[c->last].ao_valid) { float ams = 0; if (hipEventElapsedTime(&ams, c->slot[c->last].ao_ev[0], c->slot[c->last].ao_ev[1]) == hipSuccess) c->stats.ao_ms = ams; } // (only a slot whose latest frame had its AO pass has recorded these events: asking others leaves an error behind for the next hipGetLastError)
        float ms = 0;
        if (c->frame_no) {
            const Event *ev = c->ev[(c->frame_no - 1) % ArtContext::kRing];
            if (hipEventElapsedTime(&ms, ev[0], ev[4]) == hipSuccess) c->stats.frame_ms = ms;
            if (c->ev_fused[(c->frame_no - 1) % ArtContext::kRing]) { c->stats.trace_primary_ms = c->stats.frame_ms; c->stats.shade_ms = c->stats.trace_shadow_ms = c->stats.accumulate_ms = 0.f; }
            else {
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) c->stats.trace_primary_ms = ms;
            if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) c->stats.shade_ms = ms;
            if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) c->stats.trace_shadow_ms = ms;
            if (hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) c->stats.accumulate_ms = ms;
            }
        }
    }
    as_fill_stats(c, &c->stats);
    *out = c->stats;
    return ART_OK;
}

// ---- parity / debug surface ------------------------------------------------------------------------------------
// local pixel p (tile, 8x8 block, lane) -> the frame's (x, y), as the kernels' local_to_xy (art_device.h); false: outside the frame (an edge tile)
static bool local_to_xy(const ArtContext *c, uint32_t p, uint32_t &x, uint32_t &y) {
    const uint32_t tile = c->tile_list[p >> 10], q = p & 1023u, sub = q >> 6, l = q & 63u;
    x = (tile % c->tiles_x) * kTile + (sub & 3u) * 8u + (l & 7u); y = (tile / c->tiles_x) * kTile + (sub >> 2) * 8u + (l >> 3);
    return x < c->W && y < c->H;
}
int32_t art_read_hits(ArtContext *c, float *tuv, int32_t *ids, size_t n_pixels) {
    if (!c || !tuv || !ids) return fail(ART_E_INVALID, "art_read_hits: null argument");
    if (!c->traced) return fail(ART_E_STATE, "art_read_hits: nothing traced yet");
    if (n_pixels != (size_t)c->W * c->H) return fail(ART_E_INVALID, "art_read_hits: size mismatch");
    if (c->fused_frame() && !(c->cfg.flags & ART_FLAG_KEEP_DEBUG)) return fail(ART_E_STATE, "art_read_hits: fused frames keep hit records only with ART_FLAG_KEEP_DEBUG");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    std::vector<float4> h(c->n_local);
    std::vector<DevTri> tris(c->T);
    HIPC(hipMemcpy(h.data(), c->slot[c->last].d_hits.p + (size_t)c->read_b * c->n_local, (size_t)c->n_local * 16, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(tris.data(), c->bvh.tris, (size_t)c->T * sizeof(DevTri), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_pixels; i++) { tuv[4 * i] = 0; tuv[4 * i + 1] = 0; tuv[4 * i + 2] = 0; tuv[4 * i + 3] = 0; ids[2 * i] = -2; ids[2 * i + 1] = -2; } // -2: not owned
    for (uint32_t p = 0; p < c->n_local; p++) {
        uint32_t x, y;
        if (!local_to_xy(c, p, x, y)) continue;
        size_t i = (size_t)y * c->W + x;
        uint32_t pos; std::memcpy(&pos, &h[p].w, 4);
        tuv[4 * i] = h[p].x; tuv[4 * i + 1] = h[p].y; tuv[4 * i + 2] = h[p].z;
        if (pos == kNoHit) { ids[2 * i] = -1; ids[2 * i + 1] = -1; }
        else { uint32_t gid; std::memcpy(&gid, &tris[pos].f[15], 4); gid_to_ids(c, gid, ids + 2 * i); }
    }
    return ART_OK;
}

int32_t art_read_shadow_bits(ArtContext *c, uint32_t *bits, size_t n_pixels) {
    if (!c || !bits) return fail(ART_E_INVALID, "art_read_shadow_bits: null argument");
    if (!(c->cfg.flags & ART_FLAG_KEEP_DEBUG)) return fail(ART_E_STATE, "art_read_shadow_bits: context created without ART_FLAG_KEEP_DEBUG");
    if (!c->traced) return fail(ART_E_STATE, "art_read_shadow_bits: nothing traced yet");
    if (n_pixels != (size_t)c->W * c->H) return fail(ART_E_INVALID, "art_read_shadow_bits: size mismatch");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    std::vector<uint32_t> sb(c->n_local);
    HIPC(hipMemcpy(sb.data(), c->slot[c->last].d_shadow_bits.p + (size_t)c->read_b * c->n_local, (size_t)c->n_local * 4, hipMemcpyDeviceToHost));
    std::memset(bits, 0, n_pixels * 4);
    for (uint32_t p = 0; p < c->n_local; p++) {
        uint32_t x, y;
        if (!local_to_xy(c, p, x, y)) continue;
        bits[(size_t)y * c->W + x] = sb[p];
    }
    return ART_OK;
}

// the context's table of shadow-occluder hints (FrameArgs::hints): words = 4 * kHintLights * (local pixels / 64), entry (block b, light slot l) at 16 * b + 4 * l
int32_t art_read_shadow_hints(ArtContext *c, uint32_t *words, size_t n_words) {
    if (!c || !words) return fail(ART_E_INVALID, "art_read_shadow_hints: null argument");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    if (!c->frame_ready) return fail(ART_E_STATE, "art_read_shadow_hints: no frame layout yet (art_trace)");
    if (n_words != c->hint_words()) return fail(ART_E_INVALID, "art_read_shadow_hints: size mismatch");
    if (n_words) HIPC(hipMemcpy(words, c->d_hints.p, n_words * 4, hipMemcpyDeviceToHost));
    return ART_OK;
}
int32_t art_write_shadow_hints(ArtContext *c, const uint32_t *words, size_t n_words) {   // tests only: any content is a legal table
    if (!c || !words) return fail(ART_E_INVALID, "art_write_shadow_hints: null argument");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    if (!c->frame_ready) return fail(ART_E_STATE, "art_write_shadow_hints: no frame layout yet (art_trace)");
    if (n_words != c->hint_words()) return fail(ART_E_INVALID, "art_write_shadow_hints: size mismatch");
    if (n_words) HIPC(hipMemcpy(c->d_hints.p, words, n_words * 4, hipMemcpyHostToDevice));
    HIPC(hipDeviceSynchronize());
    return ART_OK;
}

// the guarded fast paths of art_device.h (inv_sqrt_exact / sqrt_exact), swept by art_sweeps.hip against the plain expressions over a set of bit patterns (include/art_parity.h)
int32_t art_parity_math_sweep(ArtContext *c, uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, uint64_t *mismatches, uint32_t *first_bad_bits,
                              uint64_t *fast_lanes, float guard[2]) {
    if (!c || !mismatches || !first_bad_bits || !fast_lanes || !guard) return fail(ART_E_INVALID, "art_parity_math_sweep: null argument");
    if (which > 4 || count > (1ull << 32)) return fail(ART_E_INVALID, "art_parity_math_sweep: which 0..4, at most 2^32 patterns");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    math_sweep_guard(guard);
    unsigned long long h[3] = {0ull, ~0ull, 0ull};
    DevBuf<unsigned long long> d;
    HIPC(d.ensure(3));
    HIPC(hipMemcpy(d.p, h, sizeof h, hipMemcpyHostToDevice));
    launch_math_sweep(which, first_bits, count, stride, d.p, nullptr); HIPC(hipGetLastError());
    HIPC(hipMemcpy(h, d.p, sizeof h, hipMemcpyDeviceToHost));
    *mismatches = h[0]; *fast_lanes = h[2];
    if (h[0]) *first_bad_bits = first_bits + (uint32_t)h[1] * stride;
    return ART_OK;
}

// the short forms of the once-per-wave divisions (rcp_core, div_core: art_device.h), swept by art_sweeps.hip against the divisions themselves (include/art_parity.h)
int32_t art_parity_div_sweep(ArtContext *c, uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, uint32_t numerator_bits, uint64_t *mismatches, uint32_t first_bad[2],
                             uint64_t *short_lanes, uint64_t *lanes, float guard[4]) {
    if (!c || !mismatches || !first_bad || !short_lanes || !lanes || !guard) return fail(ART_E_INVALID, "art_parity_div_sweep: null argument");
    if (which > 4 || count > (1ull << 32)) return fail(ART_E_INVALID, "art_parity_div_sweep: which 0..4, at most 2^32 patterns");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    div_sweep_guard(guard);
    unsigned long long h[4] = {0ull, ~0ull, 0ull, 0ull};
    DevBuf<unsigned long long> d;
    HIPC(d.ensure(4));
    HIPC(hipMemcpy(d.p, h, sizeof h, hipMemcpyHostToDevice));
    launch_div_sweep(which, first_bits, count, stride, numerator_bits, d.p, nullptr); HIPC(hipGetLastError());
    HIPC(hipMemcpy(h, d.p, sizeof h, hipMemcpyDeviceToHost));
    *mismatches = h[0]; *short_lanes = h[2]; *lanes = h[3];
    if (h[0]) {
        const uint32_t j = first_bits + (uint32_t)h[1] * stride;
        first_bad[0] = numerator_bits; first_bad[1] = j;   // which 0 (the numerator is 1), 1, 2: the pattern itself
        if (which >= 3) div_sweep_pair(which, j, numerator_bits, first_bad[0], first_bad[1]);
    }
    return ART_OK;
}

// the radiance-only helpers (pow22_texel, art_shade.h; quotient_rcp, art_sweeps.hip) against the expressions they stand for: a distance in ulps and the result classes (include/art_parity.h)
int32_t art_parity_radiance_sweep(ArtContext *c, uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, float numerator, uint32_t *max_ulps, uint32_t *worst_bits,
                                  uint64_t *class_mismatches, uint32_t *first_class_bits) {
    if (!c || !max_ulps || !worst_bits || !class_mismatches || !first_class_bits) return fail(ART_E_INVALID, "art_parity_radiance_sweep: null argument");
    if (which > 1 || count > (1ull << 32)) return fail(ART_E_INVALID, "art_parity_radiance_sweep: which 0..1, at most 2^32 patterns");
    int32_t r = use_device(c); if (r) return r;
    r = sync_all(c); if (r) return r;
    unsigned long long h[3] = {0ull, 0ull, ~0ull};
    DevBuf<unsigned long long> d;
    HIPC(d.ensure(3));
    HIPC(hipMemcpy(d.p, h, sizeof h, hipMemcpyHostToDevice));
    launch_radiance_sweep(which, first_bits, count, stride, numerator, d.p, nullptr); HIPC(hipGetLastError());
    HIPC(hipMemcpy(h, d.p, sizeof h, hipMemcpyDeviceToHost));
    *max_ulps = (uint32_t)(h[0] >> 32); *class_mismatches = h[1];
    if (h[0]) *worst_bits = first_bits + (uint32_t)h[0] * stride;
    if (h[1]) *first_class_bits = first_bits + (uint32_t)h[2] * stride;
    return ART_OK;
}

// what libart holds in this process right now (include/art_parity.h): the counters the handles of art_own.h and the stream pool above keep
int32_t art_parity_live_resources(uint64_t out[5]) {
    if (!out) return fail(ART_E_INVALID, "art_parity_live_resources: null argument");
    for (int i = 0; i < 5; i++) out[i] = g_live[i].load(std::memory_order_relaxed);
    return ART_OK;
}

} // extern "C"
