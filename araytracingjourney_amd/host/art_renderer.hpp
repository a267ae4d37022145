// art_renderer.hpp -- C++ host-side mirror of the reference's renderer API over the libart C ABI (include/art.h).
//
// The reference is compiled Rust; its toolchain is absent from this image, so the host layer a Rust maintainer would write over
// the `extern "C"` block of INTEGRATION.md is provided in C++ with the same names, argument meaning and error behaviour:
//   art::Renderer          ~ VulkanTempleRayTracedRenderer (src/vk_renderer/renderer.rs:121-137: new, add_model, prepare_first_frame,
//                            render_frame, camera_mut, lights_mut)
//   art::Camera            ~ VkCamera (vk_camera.rs:128-193)
//   art::Lights, PointLight, SpotLight, DirectionalLight, AreaLight ~ lights.rs
//   art::GltfModelReader   ~ model_reader/gltf_model_reader.rs
// The reference panics on every error (unwrap/expect); here every failed C-ABI call throws art::Panic carrying art_last_error().
#pragma once
#include <array>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/art.h"

namespace art {

struct Panic : std::runtime_error { int32_t code; Panic(int32_t c, const std::string &m) : std::runtime_error(m), code(c) {} };
inline void check(int32_t r) { if (r != ART_OK) throw Panic(r, art_last_error()); }
inline void check_glb(int32_t r) { if (r != ART_OK) throw Panic(r, art_glb_last_error()); }

using Vector3 = std::array<float, 3>;
using Vector2 = std::array<float, 2>;
using Matrix3x4 = std::array<float, 12>; // row-major

// ---- lights.rs ------------------------------------------------------------------------------------------------------
struct PointLight {      // lights.rs:95-159
    Vector3 pos, color; float falloff_distance; bool casts_shadows;
    PointLight(Vector3 p, Vector3 c, float f, bool s) : pos(p), color(c), falloff_distance(f), casts_shadows(s) {}
    ArtLight get_light_shader_data() const { ArtLight l; check(art_light_point(pos.data(), color.data(), falloff_distance, casts_shadows, &l)); return l; }
};
struct SpotLight {       // lights.rs:161-243
    Vector3 pos, dir, color; float falloff_distance; Vector2 penumbra_umbra_angles; bool casts_shadows;
    SpotLight(Vector3 p, Vector3 d, Vector3 c, float f, Vector2 a, bool s) : pos(p), dir(d), color(c), falloff_distance(f), penumbra_umbra_angles(a), casts_shadows(s) {}
    ArtLight get_light_shader_data() const { ArtLight l; check(art_light_spot(pos.data(), dir.data(), color.data(), falloff_distance, penumbra_umbra_angles[0], penumbra_umbra_angles[1], casts_shadows, &l)); return l; }
};
struct DirectionalLight { // lights.rs:245-296
    Vector3 dir, color; bool casts_shadows;
    DirectionalLight(Vector3 d, Vector3 c, bool s) : dir(d), color(c), casts_shadows(s) {}
    ArtLight get_light_shader_data() const { ArtLight l; check(art_light_directional(dir.data(), color.data(), casts_shadows, &l)); return l; }
};
struct AreaLight {       // lights.rs:298-403
    Vector3 pos, pos2, pos3; bool invert_normal; Vector3 color; float falloff_distance; Vector2 penumbra_umbra_angles; bool casts_shadows;
    AreaLight(Vector3 p, Vector3 p2, Vector3 p3, bool inv, Vector3 c, float f, Vector2 a, bool s)
        : pos(p), pos2(p2), pos3(p3), invert_normal(inv), color(c), falloff_distance(f), penumbra_umbra_angles(a), casts_shadows(s) {}
    ArtLight get_light_shader_data() const { ArtLight l; check(art_light_area(pos.data(), pos2.data(), pos3.data(), invert_normal, color.data(), falloff_distance, penumbra_umbra_angles[0], penumbra_umbra_angles[1], casts_shadows, &l)); return l; }
};
class Lights {           // lights.rs:4-67
    std::vector<PointLight> point_; std::vector<SpotLight> spot_; std::vector<DirectionalLight> directional_; std::vector<AreaLight> area_;
public:
    std::vector<PointLight> &get_point_lights_mut() { return point_; }
    std::vector<SpotLight> &get_spot_lights_mut() { return spot_; }
    std::vector<DirectionalLight> &get_directional_lights_mut() { return directional_; }
    std::vector<AreaLight> &get_area_lights_mut() { return area_; }
    size_t get_lights_count() const { return point_.size() + spot_.size() + directional_.size() + area_.size(); }
    // order point, spot, directional, area; every light gets its own slot (the reference's lights.rs:29-46 reuses one slot per kind)
    std::vector<ArtLight> copy_lights_shader_data() const {
        std::vector<ArtLight> out;
        for (auto &l : point_) out.push_back(l.get_light_shader_data());
        for (auto &l : spot_) out.push_back(l.get_light_shader_data());
        for (auto &l : directional_) out.push_back(l.get_light_shader_data());
        for (auto &l : area_) out.push_back(l.get_light_shader_data());
        return out;
    }
};

// ---- vk_camera.rs ---------------------------------------------------------------------------------------------------
class Camera {
    Vector3 pos_, dir_; float aspect_, fovy_, znear_, zfar_; bool needs_update_ = true; ArtCamera block_{};
public:
    Camera(Vector3 pos, Vector3 dir, float aspect, float fovy, float znear, float zfar) : pos_(pos), dir_(dir), aspect_(aspect), fovy_(fovy), znear_(znear), zfar_(zfar) {}
    void set_pos(Vector3 p) { pos_ = p; needs_update_ = true; }
    void set_dir(Vector3 d) { dir_ = d; needs_update_ = true; }   // normalised when the block is built (vk_camera.rs:133-136)
    void set_aspect(float a) { aspect_ = a; needs_update_ = true; }
    void set_fovy(float f) { fovy_ = f; needs_update_ = true; }
    void set_znear(float z) { znear_ = z; needs_update_ = true; }
    void set_zfar(float z) { zfar_ = z; needs_update_ = true; }
    Vector3 pos() const { return pos_; }
    Vector3 dir() const { return dir_; }
    float aspect() const { return aspect_; }
    float fovy() const { return fovy_; }
    const ArtCamera &update_host_buffer() { // vk_camera.rs:104-126
        if (needs_update_) { check(art_camera_from_params(pos_.data(), dir_.data(), aspect_, fovy_, znear_, zfar_, &block_)); needs_update_ = false; }
        return block_;
    }
};

// ---- model_reader/gltf_model_reader.rs ---------------------------------------------------------------------------------
class GltfModelReader {
    ArtGlb *h_ = nullptr;
public:
    enum Coerce { NONE = 0, R8G8B8A8_UNORM = 1, B8G8R8A8_UNORM = 2, B8G8R8_UNORM = 3 };
    static GltfModelReader open(const std::string &file_path, bool normalize_vectors, Coerce coerce_image_to_format) {
        GltfModelReader r; check_glb(art_glb_open(file_path.c_str(), normalize_vectors, (int32_t)coerce_image_to_format, &r.h_)); return r;
    }
    GltfModelReader() = default;
    GltfModelReader(GltfModelReader &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    GltfModelReader(const GltfModelReader &) = delete;
    ~GltfModelReader() { if (h_) art_glb_close(h_); }
    ArtGlb *handle() const { return h_; }
    std::pair<Vector3, float> get_primitives_bounding_sphere() const { Vector3 c; float r; check_glb(art_glb_bounding_sphere(h_, c.data(), &r)); return {c, r}; }
};

// ---- renderer.rs ------------------------------------------------------------------------------------------------------
// ---- model_reader.rs:100-146 + vk_model.rs:280-345: bounding sphere and the residency state machine ----------------------
struct Sphere {
    Vector3 center{0, 0, 0}; float radius = 0;
    float get_distance_from_point(const Vector3 &p) const { // model_reader.rs:124-126
        float dx = center[0] - p[0], dy = center[1] - p[1], dz = center[2] - p[2];
        return std::sqrt(dx * dx + dy * dy + dz * dz) - radius;
    }
    Sphere transform(const Matrix3x4 &m) const {              // model_reader.rs:128-141
        float sc = 0;
        for (int k = 0; k < 3; k++) sc = std::fmax(sc, std::sqrt(m[k] * m[k] + m[4 + k] * m[4 + k] + m[8 + k] * m[8 + k]));
        Sphere o;
        for (int r = 0; r < 3; r++) o.center[r] = m[4 * r] * center[0] + m[4 * r + 1] * center[1] + m[4 * r + 2] * center[2] + m[4 * r + 3];
        o.radius = sc * radius;
        return o;
    }
};
enum class ModelState { Storage, Host, Device };
struct Model { // VkModel: only Device models are instanced in the acceleration structure (renderer.rs:640-651)
    std::vector<uint32_t> primitive_ids; Sphere model_bounding_sphere; ModelState state = ModelState::Host; bool needs_cb_submit = false, instanced = true;
    ArtContext *ctx = nullptr; Matrix3x4 model_matrix{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; Sphere object_sphere; // the reader's sphere, before any model matrix
    std::vector<std::vector<float>> positions; // object-space positions (x y z per vertex) of every primitive: set_vertices keeps the sphere from them
    // VkModel::set_model_matrix (vk_model.rs:461-466): the instance's object -> world matrix and the sphere that goes with it.  Fixed against the reference, which
    // transforms the sphere it HOLDS (already transformed) by the new matrix (:463-465) and so compounds the matrices of a model that moves every frame; the same for
    // the one call main.rs makes.  The reference rebuilds its TLAS every frame for this (renderer.rs:637-651); libart refits in front of the next frame.
    void set_model_matrix(const Matrix3x4 &m) {
        model_matrix = m;
        model_bounding_sphere = object_sphere.transform(m);
        if (ctx && !primitive_ids.empty()) check(art_scene_set_model_matrix(ctx, primitive_ids.front(), (uint32_t)primitive_ids.size(), m.data())); // a model's ids are consecutive (art_scene_add_glb)
    }
    // BLAS update (a BLAS built with ALLOW_UPDATE, rebuilt in MODE_UPDATE; the reference never does this: its BLAS flags are PREFER_FAST_TRACE only, vk_model.rs:968):
    // primitive primitive_ids[primitive_index] gets n new vertices, its count, indices, texture and matrix kept; the sphere follows the new positions (the centre of the
    // model's box, the farthest position from it, before the model matrix).  On a built scene the next frame refits on the device (art_scene_set_vertices).
    void set_vertices(size_t primitive_index, const ArtVertex *v, uint32_t n) {
        if (primitive_index >= primitive_ids.size() || primitive_index >= positions.size()) throw Panic(ART_E_INVALID, "Model::set_vertices: no such primitive");
        if (ctx) check(art_scene_set_vertices(ctx, primitive_ids[primitive_index], v, n));
        std::vector<float> &q = positions[primitive_index];
        q.resize((size_t)n * 3);
        for (uint32_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) q[3 * (size_t)i + k] = v[i].pos[k];
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (const auto &p : positions) for (size_t i = 0; i + 2 < p.size(); i += 3) for (int k = 0; k < 3; k++) { lo[k] = std::fmin(lo[k], p[i + k]); hi[k] = std::fmax(hi[k], p[i + k]); }
        Sphere sp; float r2 = 0;
        for (int k = 0; k < 3; k++) sp.center[k] = 0.5f * (lo[k] + hi[k]);
        for (const auto &p : positions) for (size_t i = 0; i + 2 < p.size(); i += 3) {
            float dx = p[i] - sp.center[0], dy = p[i + 1] - sp.center[1], dz = p[i + 2] - sp.center[2];
            r2 = std::fmax(r2, dx * dx + dy * dy + dz * dz);
        }
        sp.radius = std::sqrt(r2);
        object_sphere = sp;
        model_bounding_sphere = object_sphere.transform(model_matrix);
    }
    // Alpha-masked primitive (glTF alphaMode MASK; Vulkan: non-opaque geometry whose any-hit shader ignores the intersection when alpha < cutoff; the reference
    // marks all its geometry opaque, vk_model.rs:927): a hit on primitive primitive_ids[primitive_index] is discarded for every ray where the alpha of its texture
    // layer 0 is below `cutoff`; 0 is opaque, cutoff must lie in [0, 1].  Nothing is built: the next frame takes it up (art_scene_set_alpha_cutoff).
    void set_alpha_cutoff(size_t primitive_index, float cutoff) {
        if (primitive_index >= primitive_ids.size()) throw Panic(ART_E_INVALID, "Model::set_alpha_cutoff: no such primitive");
        if (!(cutoff >= 0.0f && cutoff <= 1.0f)) throw Panic(ART_E_INVALID, "Model::set_alpha_cutoff: the cutoff must lie in [0, 1]");
        if (ctx) check(art_scene_set_alpha_cutoff(ctx, primitive_ids[primitive_index], cutoff));
    }
    // Visibility mask (Vulkan: VkAccelerationStructureInstanceKHR.mask; the reference hard-codes 0xFF, vk_model.rs:373): a hit on primitive primitive_ids[primitive_index]
    // is discarded for every ray whose cull mask shares no bit with `mask` (Renderer::set_ray_masks).  0xFF is the default; mask must lie in 0..0xFF.  Nothing is built:
    // the next frame takes it up (art_scene_set_primitive_mask).
    void set_mask(size_t primitive_index, uint32_t mask) {
        if (primitive_index >= primitive_ids.size()) throw Panic(ART_E_INVALID, "Model::set_mask: no such primitive");
        if (mask > 0xFFu) throw Panic(ART_E_INVALID, "Model::set_mask: the mask must lie in 0..0xFF");
        if (ctx) check(art_scene_set_primitive_mask(ctx, primitive_ids[primitive_index], mask));
    }
    const Matrix3x4 &get_transform_model_matrix() const { return model_matrix; } // vk_model.rs:358-363
    void update_model_status(const Vector3 &camera_pos) { // vk_model.rs:334-345
        float d = model_bounding_sphere.get_distance_from_point(camera_pos);
        ModelState want = d <= 10.0f ? ModelState::Device : (d <= 20.0f ? ModelState::Host : ModelState::Storage);
        if ((want == ModelState::Device) != (state == ModelState::Device)) needs_cb_submit = true;
        state = want;
    }
    bool needs_command_buffer_submission() const { return needs_cb_submit; }
    void reset_command_buffer_submission_status() { needs_cb_submit = false; }
};

class Renderer {
    ArtContext *ctx_ = nullptr; uint32_t w_, h_; Camera camera_; Lights lights_; std::vector<Model> models_;
public:
    // VulkanTempleRayTracedRenderer::new (renderer.rs:140); camera defaults of renderer.rs:222-231
    Renderer(uint32_t width, uint32_t height, int device = -1, uint32_t frames_in_flight = 1, uint32_t extra_flags = 0)   // extra_flags: ART_FLAG_* besides the host's own
        : w_(width), h_(height), camera_({0, 0, 0}, {0, 0, 1}, (float)width / (float)height, 1.57079632679f, 0.1f, 1000.0f) {
        ArtConfig cfg{}; cfg.device = device; cfg.width = width; cfg.height = height; cfg.frames_in_flight = frames_in_flight;
        cfg.flags = ART_FLAG_DYNAMIC_SCENE | extra_flags;   // this host moves its models (set_model_matrix) and switches them in and out by residency: the ring of structure versions is made by the build, not by the first moved frame
        check(art_create(&cfg, &ctx_));
    }
    Renderer(const Renderer &) = delete;
    ~Renderer() { if (ctx_) art_destroy(ctx_); }
    // alpha_mask (opt-in; the reference draws every material opaque): every primitive whose material is alphaMode MASK and whose base-colour image has an alpha
    // channel gets its alphaCutoff (Model::set_alpha_cutoff).  An RGB image is coerced with alpha 0 and is never masked; BLEND is drawn opaque.
    void add_model(const std::string &file_path, const Matrix3x4 &model_matrix, bool alpha_mask = false) { // renderer.rs:346 -> vk_model.rs:494-528
        GltfModelReader r = GltfModelReader::open(file_path, true, GltfModelReader::B8G8R8A8_UNORM);
        uint32_t first = 0, n = 0;
        check_glb(art_scene_add_glb(ctx_, r.handle(), model_matrix.data(), &first, &n));
        Model m; m.ctx = ctx_; m.model_matrix = model_matrix;
        for (uint32_t i = 0; i < n; i++) m.primitive_ids.push_back(first + i);
        auto cs = r.get_primitives_bounding_sphere();                      // vk_model.rs:501, then set_model_matrix (:461-466)
        {   // the positions alone (12 B a vertex), for Model::set_vertices' sphere
            std::vector<ArtGlbCopyInfo> infos(n ? n : 1); size_t total = 0;
            check_glb(art_glb_copy_model_data(r.handle(), ART_ATTR_VERTICES, 0, nullptr, 0, infos.data(), n, &total));
            std::vector<uint8_t> data(total ? total : 1);
            check_glb(art_glb_copy_model_data(r.handle(), ART_ATTR_VERTICES, 0, data.data(), data.size(), infos.data(), n, &total));
            for (uint32_t i = 0; i < n; i++) {
                std::vector<float> q(infos[i].mesh_size / 4);
                std::memcpy(q.data(), data.data() + infos[i].mesh_buffer_offset, q.size() * 4);
                m.positions.push_back(std::move(q));
            }
        }
        Sphere sp; sp.center = cs.first; sp.radius = cs.second;
        m.object_sphere = sp;
        m.model_bounding_sphere = sp.transform(model_matrix);
        if (alpha_mask)
            for (uint32_t i = 0; i < n; i++) {
                int32_t mode = 0, has_alpha = 0; float cutoff = 0.5f;
                check_glb(art_glb_primitive_alpha(r.handle(), i, &mode, &cutoff, &has_alpha));
                if (mode == 1 && has_alpha) m.set_alpha_cutoff(i, std::fmin(std::fmax(cutoff, 0.0f), 1.0f));
            }
        models_.push_back(m);
    }
    std::vector<Model> &models_mut() { return models_; }
    // renderer.rs:637-651: residency by camera distance; rebuilds the acceleration structure over the Device models when the set changed
    bool update_models_status(bool build = true) {
        bool changed = false;
        for (Model &m : models_) {
            m.update_model_status(camera_.pos());
            m.reset_command_buffer_submission_status();
            bool dev = m.state == ModelState::Device;
            if (dev != m.instanced) { m.instanced = dev; for (uint32_t id : m.primitive_ids) check(art_scene_set_primitive_enabled(ctx_, id, dev ? 1 : 0)); changed = true; }
        }
        if (changed && build && art_scene_needs_build(ctx_) != 0) check(art_scene_build(ctx_)); // (part of the last build: in and out by the next frame's refit)
        return changed && build;
    }
    void add_primitive(const ArtVertex *v, uint32_t nv, const void *idx, uint32_t n_idx, uint32_t idx_bytes, const uint8_t *rgba8, uint32_t tw, uint32_t th, const Matrix3x4 &m) {
        check(art_scene_add_primitive(ctx_, v, nv, idx, n_idx, idx_bytes, rgba8, tw, th, m.data(), nullptr));
    }
    void prepare_first_frame() { update_models_status(false); check(art_scene_build(ctx_)); } // renderer.rs:356
    Camera &camera_mut() { return camera_; }                              // renderer.rs:515
    Lights &lights_mut() { return lights_; }                              // renderer.rs:519
    void render_frame(bool wait = true) {                                  // renderer.rs:371
        update_models_status();
        check(art_set_camera(ctx_, &camera_.update_host_buffer()));
        std::vector<ArtLight> ls = lights_.copy_lights_shader_data();
        check(art_set_lights(ctx_, ls.data(), (uint32_t)ls.size()));
        check(art_trace(ctx_));
        if (wait) check(art_sync(ctx_));
    }
    // the cull masks of the rays render_frame (primary, shadow) and compute_ao (ao) cast (Vulkan: traceRayEXT's cullMask; the reference hard-codes 0xFF,
    // raytrace.rgen.glsl:92,169): per-launch state like the camera; 0 is legal, such a ray sees nothing (art_set_ray_masks)
    void set_ray_masks(uint32_t primary = 0xFFu, uint32_t shadow = 0xFFu, uint32_t ao = 0xFFu) {
        if (primary > 0xFFu || shadow > 0xFFu || ao > 0xFFu) throw Panic(ART_E_INVALID, "Renderer::set_ray_masks: a mask must lie in 0..0xFF");
        check(art_set_ray_masks(ctx_, primary, shadow, ao));
    }
    void compute_ao(uint32_t spp = 16, float radius = 0.2f * 1.457f) { check(art_trace_ao(ctx_, spp, radius)); } // ao_layer.compute_ao, renderer.rs:688
    // Rays of the application's own (Vulkan: traceRayEXT from its own ray-generation shader, VK_KHR_ray_query; the reference has no call for it): n rays of 8 floats -- o.xyz,
    // tmin, d.xyz, tmax -- in DEVICE memory, traced asynchronously on hip_stream (nullptr: a stream the context owns, fenced by cast_sync).  Closest hits: n x 4 floats
    // t,u,v,0 and n x 2 int32 (primitive, triangle); any hit: n bytes.  The scene is the one of the call: a pending move or mask is taken up first (art_cast_rays).
    static ArtRayCast closest_cast(const void *rays_dev, uint32_t n, void *tuv_dev, void *ids_dev, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtRayCast d{}; d.rays_dev = rays_dev; d.tuv_dev = tuv_dev; d.ids_dev = ids_dev; d.hip_stream = hip_stream; d.n = n; d.kind = ART_CAST_CLOSEST; d.cull_mask = cull_mask;
        return d;
    }
    static ArtRayCast any_cast(const void *rays_dev, uint32_t n, void *hit_dev, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtRayCast d{}; d.rays_dev = rays_dev; d.hit_dev = hit_dev; d.hip_stream = hip_stream; d.n = n; d.kind = ART_CAST_ANY; d.cull_mask = cull_mask;
        return d;
    }
    // the first max_hits hits of each ray in ascending (t, global triangle id): n x max_hits records, ray-major, and (optionally) a count byte a ray (art_cast_rays_multi)
    static ArtRayCastMulti multi_cast(const void *rays_dev, uint32_t n, uint32_t max_hits, void *tuv_dev, void *ids_dev, void *count_dev = nullptr, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtRayCastMulti d{}; d.rays_dev = rays_dev; d.tuv_dev = tuv_dev; d.ids_dev = ids_dev; d.count_dev = count_dev; d.hip_stream = hip_stream; d.n = n; d.max_hits = max_hits; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtRayCastMulti) == 56, "ArtRayCastMulti is part of the ABI");
    static void cast_rays_multi(ArtContext *ctx, const ArtRayCastMulti &d) { check(art_cast_rays_multi(ctx, &d)); }
    void cast_rays_multi(const ArtRayCastMulti &d) { cast_rays_multi(ctx_, d); }
    static void cast_rays(ArtContext *ctx, const ArtRayCast &d) { check(art_cast_rays(ctx, &d)); }   // panics like every other call of the mirror
    void cast_rays(const ArtRayCast &d) { cast_rays(ctx_, d); }
    // the nearest surface point to each of n points (p.xyz, r) in device memory: n x 4 floats d,u,v,0, n x 2 int32 and (optionally) n x float4 points (art_closest_points)
    static ArtPointQuery point_query(const void *points_dev, uint32_t n, void *duv_dev, void *ids_dev, void *point_dev = nullptr, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtPointQuery d{}; d.points_dev = points_dev; d.duv_dev = duv_dev; d.ids_dev = ids_dev; d.point_dev = point_dev; d.hip_stream = hip_stream; d.n = n; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtPointQuery) == 56, "ArtPointQuery is part of the ABI");
    static void closest_points(ArtContext *ctx, const ArtPointQuery &d) { check(art_closest_points(ctx, &d)); }
    void closest_points(const ArtPointQuery &d) { closest_points(ctx_, d); }
    // the max_hits nearest triangles to each of n points: n x max_hits records of art_closest_points' kind, query-major, and (optionally) a count a query (art_closest_points_multi)
    static ArtPointQueryMulti point_query_multi(const void *points_dev, uint32_t n, uint32_t max_hits, void *duv_dev, void *ids_dev, void *point_dev = nullptr, void *count_dev = nullptr,
                                                void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtPointQueryMulti d{}; d.points_dev = points_dev; d.duv_dev = duv_dev; d.ids_dev = ids_dev; d.point_dev = point_dev; d.count_dev = count_dev; d.hip_stream = hip_stream;
        d.n = n; d.max_hits = max_hits; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtPointQueryMulti) == 64, "ArtPointQueryMulti is part of the ABI");
    static void closest_points_multi(ArtContext *ctx, const ArtPointQueryMulti &d) { check(art_closest_points_multi(ctx, &d)); }
    void closest_points_multi(const ArtPointQueryMulti &d) { closest_points_multi(ctx_, d); }
    // the triangles that touch each of n boxes (lo.xyz, -, hi.xyz, -) in device memory: a byte a box (any_overlap), or max_hits id pairs a box in ascending global id and
    // (optionally) a uint32 count of all of them (list_overlap) (art_overlap_boxes)
    static ArtBoxQuery any_overlap(const void *boxes_dev, uint32_t n, void *hit_dev, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtBoxQuery d{}; d.boxes_dev = boxes_dev; d.hit_dev = hit_dev; d.hip_stream = hip_stream; d.n = n; d.kind = ART_OVERLAP_ANY; d.cull_mask = cull_mask;
        return d;
    }
    static ArtBoxQuery list_overlap(const void *boxes_dev, uint32_t n, uint32_t max_hits, void *ids_dev, void *count_dev = nullptr, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtBoxQuery d{}; d.boxes_dev = boxes_dev; d.ids_dev = ids_dev; d.count_dev = count_dev; d.hip_stream = hip_stream; d.n = n; d.kind = ART_OVERLAP_LIST; d.max_hits = max_hits; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtBoxQuery) == 64, "ArtBoxQuery is part of the ABI");
    static void overlap_boxes(ArtContext *ctx, const ArtBoxQuery &d) { check(art_overlap_boxes(ctx, &d)); }
    void overlap_boxes(const ArtBoxQuery &d) { overlap_boxes(ctx_, d); }
    // the scene triangles that touch each of n query triangles (q0.xyz, -, q1.xyz, -, q2.xyz, -) in device memory: a byte a query (any_collision), or max_hits id pairs a
    // query in ascending global id and (optionally) a uint32 count of all of them (list_collision) (art_overlap_triangles)
    static ArtTriQuery any_collision(const void *tris_dev, uint32_t n, void *hit_dev, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtTriQuery d{}; d.tris_dev = tris_dev; d.hit_dev = hit_dev; d.hip_stream = hip_stream; d.n = n; d.kind = ART_OVERLAP_ANY; d.cull_mask = cull_mask;
        return d;
    }
    static ArtTriQuery list_collision(const void *tris_dev, uint32_t n, uint32_t max_hits, void *ids_dev, void *count_dev = nullptr, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtTriQuery d{}; d.tris_dev = tris_dev; d.ids_dev = ids_dev; d.count_dev = count_dev; d.hip_stream = hip_stream; d.n = n; d.kind = ART_OVERLAP_LIST; d.max_hits = max_hits; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtTriQuery) == 64, "ArtTriQuery is part of the ABI");
    static void overlap_triangles(ArtContext *ctx, const ArtTriQuery &d) { check(art_overlap_triangles(ctx, &d)); }
    void overlap_triangles(const ArtTriQuery &d) { overlap_triangles(ctx_, d); }
    // the distance from each of n query triangles (q0.xyz, r, q1.xyz, -, q2.xyz, -) in device memory to the scene: records of art_closest_points' kind and (optionally)
    // n x float4 witness points on the scene triangle and on the query (art_closest_triangles)
    static ArtTriDistance tri_distance(const void *tris_dev, uint32_t n, void *duv_dev, void *ids_dev, void *point_dev = nullptr, void *qpoint_dev = nullptr, void *hip_stream = nullptr,
                                       uint32_t cull_mask = 0xFFu) {
        ArtTriDistance d{}; d.tris_dev = tris_dev; d.duv_dev = duv_dev; d.ids_dev = ids_dev; d.point_dev = point_dev; d.qpoint_dev = qpoint_dev; d.hip_stream = hip_stream; d.n = n; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtTriDistance) == 64, "ArtTriDistance is part of the ABI");
    static void closest_triangles(ArtContext *ctx, const ArtTriDistance &d) { check(art_closest_triangles(ctx, &d)); }
    void closest_triangles(const ArtTriDistance &d) { closest_triangles(ctx_, d); }
    // where each of n query triangles (q0.xyz, tmin, q1.xyz, tmax, q2.xyz, -, d.xyz, -) in device memory, moved along its d, first touches the scene: records as a closest
    // cast's and (optionally) n x float4 contact points on the scene triangle and witness points on the query in its rest pose (art_cast_triangles)
    static ArtTriCast tri_cast(const void *sweeps_dev, uint32_t n, void *tuv_dev, void *ids_dev, void *point_dev = nullptr, void *qpoint_dev = nullptr, void *hip_stream = nullptr,
                               uint32_t cull_mask = 0xFFu) {
        ArtTriCast d{}; d.sweeps_dev = sweeps_dev; d.tuv_dev = tuv_dev; d.ids_dev = ids_dev; d.point_dev = point_dev; d.qpoint_dev = qpoint_dev; d.hip_stream = hip_stream; d.n = n; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtTriCast) == 64, "ArtTriCast is part of the ABI");
    static void cast_triangles(ArtContext *ctx, const ArtTriCast &d) { check(art_cast_triangles(ctx, &d)); }
    void cast_triangles(const ArtTriCast &d) { cast_triangles(ctx_, d); }
    // where a ball of `radius` along each of n rays in device memory first touches the scene: records as a closest cast's and (optionally) n x float4 contact points (art_cast_spheres)
    static ArtSphereCast sphere_cast(const void *rays_dev, uint32_t n, float radius, void *tuv_dev, void *ids_dev, void *point_dev = nullptr, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtSphereCast d{}; d.rays_dev = rays_dev; d.tuv_dev = tuv_dev; d.ids_dev = ids_dev; d.point_dev = point_dev; d.hip_stream = hip_stream; d.n = n; d.cull_mask = cull_mask; d.radius = radius;
        return d;
    }
    static_assert(sizeof(ArtSphereCast) == 56, "ArtSphereCast is part of the ABI");
    static void cast_spheres(ArtContext *ctx, const ArtSphereCast &d) { check(art_cast_spheres(ctx, &d)); }
    void cast_spheres(const ArtSphereCast &d) { cast_spheres(ctx_, d); }
    // how many surfaces each of n rays in device memory enters and leaves over its whole range: n x (entries, exits) uint32, uncapped (art_cast_crossings)
    static ArtRayCrossings crossings_cast(const void *rays_dev, uint32_t n, void *cross_dev, void *hip_stream = nullptr, uint32_t cull_mask = 0xFFu) {
        ArtRayCrossings d{}; d.rays_dev = rays_dev; d.cross_dev = cross_dev; d.hip_stream = hip_stream; d.n = n; d.cull_mask = cull_mask;
        return d;
    }
    static_assert(sizeof(ArtRayCrossings) == 40, "ArtRayCrossings is part of the ABI");
    static void cast_crossings(ArtContext *ctx, const ArtRayCrossings &d) { check(art_cast_crossings(ctx, &d)); }
    void cast_crossings(const ArtRayCrossings &d) { cast_crossings(ctx_, d); }
    void cast_sync() { check(art_cast_sync(ctx_)); }
    struct CastCounts { uint64_t casts, rays, host_waits; };
    CastCounts cast_counts() { CastCounts c{}; check(art_cast_counts(ctx_, &c.casts, &c.rays, &c.host_waits)); return c; }
    void resize(uint32_t w, uint32_t h) { check(art_resize(ctx_, w, h)); w_ = w; h_ = h; camera_.set_aspect((float)w / (float)h); } // renderer.rs:523-564
    std::vector<float> color_output() { std::vector<float> o((size_t)w_ * h_ * 4); check(art_read_color(ctx_, o.data(), o.size() * 4)); return o; }
    std::vector<float> depth_output() { std::vector<float> o((size_t)w_ * h_); check(art_read_depth(ctx_, o.data(), o.size() * 4)); return o; }
    std::vector<float> normal_output() { std::vector<float> o((size_t)w_ * h_ * 4); check(art_read_normal(ctx_, o.data(), o.size() * 4)); return o; }
    std::vector<uint32_t> ao_output() { std::vector<uint32_t> o((size_t)w_ * h_); check(art_read_ao(ctx_, o.data(), o.size() * 4)); return o; }
    ArtStats stats() { ArtStats s; check(art_get_stats(ctx_, &s)); return s; }
    ArtContext *handle() const { return ctx_; }
};

} // namespace art
