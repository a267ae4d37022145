// host_mirror_demo.cpp -- the reference's main.rs:15-66 call sequence on the C++ host mirror.
//   host_mirror_demo check            host-only checks (no GPU): light order, camera block, panic-on-error behaviour
//   host_mirror_demo render <file.glb> [W H]   add_model + lights of main.rs + one frame; prints ray counts and a colour checksum
//   host_mirror_demo deform <file.glb> [W H]   the same scene; then Model::set_vertices on its first primitive (grown from the origin) and back
//   host_mirror_demo alpha <file.glb> [W H]    the same scene with add_model(..., alpha_mask = true), with the cutoffs set by hand, and opaque
//   host_mirror_demo masks <file.glb> [W H]    the same scene with its LAST primitive (a planar one) seen but casting no shadow (Model::set_mask, Renderer::set_ray_masks)
#include <cstdio>
#include <cstring>
#include "../araytracingjourney_amd/host/art_renderer.hpp"
#include "../include/art_parity.h"

static int host_checks() {
    using namespace art;
    Lights lights;
    lights.get_area_lights_mut().push_back(AreaLight({-0.70f, 0.77f, 0.08f}, {-0.70f, 0.77f, -0.16f}, {-0.70f, 0.90f, -0.16f}, false, {5.88f, 0.18f, 1.23f}, 3.0f, {1.5708f, 1.5708f}, true)); // main.rs:55-64
    lights.get_spot_lights_mut().push_back(SpotLight({0.0f, 1.5f, 0.0f}, {0.0f, -1.0f, 0.0f}, {13.6f, 1.6f, 22.2f}, 3.0f, {0.5236f, 0.7854f}, true));                                   // main.rs:42-49
    lights.get_point_lights_mut().push_back(PointLight({0, 1, 0}, {8, 8, 8}, 3.0f, true));
    lights.get_directional_lights_mut().push_back(DirectionalLight({-0.3f, -1.0f, -0.2f}, {3, 3, 3}, true));
    std::vector<ArtLight> recs = lights.copy_lights_shader_data();
    if (recs.size() != 4 || recs[0].type != 0 || recs[1].type != 1 || recs[2].type != 2 || recs[3].type != 3) { std::puts("FAIL light order"); return 1; } // lights.rs:24-47
    if (std::fabs(recs[3].dir[0] + 1.0f) > 1e-6f) { std::puts("FAIL area normal"); return 1; }                                                                // lights.rs:385-389
    Camera cam({0, 0, 0}, {0, 0, 1}, 1.0f, 1.57079632679f, 0.1f, 1000.0f);
    const ArtCamera &b = cam.update_host_buffer();
    if (std::fabs(b.view[0] - 1) > 1e-6f || std::fabs(b.view[5] + 1) > 1e-6f || std::fabs(b.view[10] + 1) > 1e-6f) { std::puts("FAIL view matrix"); return 1; } // up = -Y, looks down +Z
    bool panicked = false;
    try { GltfModelReader::open("/nonexistent.glb", true, GltfModelReader::B8G8R8A8_UNORM); } catch (const Panic &p) { panicked = std::strstr(p.what(), "Could not read file") != nullptr; }
    if (!panicked) { std::puts("FAIL missing file must panic"); return 1; }
    // residency state machine with the camera positions of the reference's own test (vk_model.rs:1082-1152)
    Model m; m.model_bounding_sphere.radius = 1.0f;
    m.update_model_status({100, 100, 100}); if (m.state != ModelState::Storage || m.needs_command_buffer_submission()) { std::puts("FAIL residency storage"); return 1; }
    m.update_model_status({7, 7, 7});       if (m.state != ModelState::Host || m.needs_command_buffer_submission()) { std::puts("FAIL residency host"); return 1; }
    m.update_model_status({3, 3, 3});       if (m.state != ModelState::Device || !m.needs_command_buffer_submission()) { std::puts("FAIL residency device"); return 1; }
    m.reset_command_buffer_submission_status();
    m.update_model_status({7, 7, 7});       if (m.state != ModelState::Host || !m.needs_command_buffer_submission()) { std::puts("FAIL residency back to host"); return 1; }
    Sphere sp; sp.center = {1, 0, 0}; sp.radius = 2.0f;
    Sphere st = sp.transform({2, 0, 0, 5, 0, 3, 0, 0, 0, 0, 1, 0});                                              // model_reader.rs:128-141
    if (std::fabs(st.center[0] - 7.0f) > 1e-6f || std::fabs(st.radius - 6.0f) > 1e-6f) { std::puts("FAIL sphere transform"); return 1; }
    // a cast whose answer is known without a device: a descriptor that is well-formed, through no context -- ART_E_INVALID, nothing touched (art_cast_rays)
    int cast_code = 0; float fake[8] = {0};
    try { Renderer::cast_rays(nullptr, Renderer::any_cast(fake, 0, nullptr)); } catch (const Panic &p) { cast_code = p.code; }
    if (cast_code != ART_E_INVALID) { std::puts("FAIL a cast without a context must panic with ART_E_INVALID"); return 1; }
    const ArtRayCast cd = Renderer::closest_cast(fake, 1, fake, fake, nullptr, 0x0Fu);
    if (cd.kind != ART_CAST_CLOSEST || cd.hit_dev != nullptr || cd.flags != 0u || cd.cull_mask != 0x0Fu || sizeof(ArtRayCast) != 56) { std::puts("FAIL cast descriptor"); return 1; }
    std::puts("HOST_MIRROR_OK");
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "check")) return host_checks();
        if (argc >= 3 && !std::strcmp(argv[1], "render")) {
            uint32_t W = argc >= 5 ? (uint32_t)std::atoi(argv[3]) : 800, H = argc >= 5 ? (uint32_t)std::atoi(argv[4]) : 800; // main.rs:18
            art::Renderer renderer(W, H);
            renderer.add_model(argv[2], {2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0});                                              // main.rs:30-36: Similarity3::from_scaling(2.0)
            renderer.lights_mut().get_spot_lights_mut().push_back(art::SpotLight({0.0f, 1.5f, 0.0f}, {0.0f, -1.0f, 0.0f}, {13.6f, 1.6f, 22.2f}, 3.0f, {0.5236f, 0.7854f}, true));
            renderer.lights_mut().get_point_lights_mut().push_back(art::PointLight({0.0f, 0.5f, -1.5f}, {8, 8, 8}, 6.0f, true));
            renderer.camera_mut().set_pos({0.0f, 0.3f, -2.5f});
            renderer.prepare_first_frame();
            renderer.render_frame();
            renderer.compute_ao();
            ArtStats st = renderer.stats();
            std::vector<float> c = renderer.color_output();
            double sum = 0; for (float v : c) sum += v;
            std::printf("RENDER_OK tris=%u primary=%llu shadow=%llu hit=%llu ao=%llu frame_ms=%.3f colour_sum=%.6e\n", st.num_triangles, (unsigned long long)st.primary_rays,
                        (unsigned long long)st.shadow_rays, (unsigned long long)st.hit_pixels, (unsigned long long)st.ao_rays, st.frame_ms, sum);
            // VkModel::set_model_matrix (vk_model.rs:461-466): the model moves half a unit to the right and back; the reference rebuilds its TLAS every frame for this
            // (renderer.rs:637-651), libart refits in front of the next frame -- and the frame of the model back in place is the first frame again, bit for bit
            renderer.models_mut()[0].set_model_matrix({2, 0, 0, 0.5f, 0, 2, 0, 0, 0, 0, 2, 0});
            renderer.render_frame();
            std::vector<float> moved = renderer.color_output();
            renderer.models_mut()[0].set_model_matrix({2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0});
            renderer.render_frame();
            std::vector<float> back = renderer.color_output();
            ArtStats st2 = renderer.stats();
            std::printf("MOVED_OK refits=%u rebuilds=%u moved_differs=%d back_equals_first=%d refit_ms=%.3f\n", st2.refits, st2.rebuilds, (int)(moved != c),
                        (int)(std::memcmp(back.data(), c.data(), c.size() * sizeof(float)) == 0), st2.refit_ms);
            // the residency rule (vk_model.rs:334-345, renderer.rs:637-651): thirty units away the model leaves the structure, back at the first position it re-enters --
            // by the refit in front of the frame, not by a build -- and the frame is the first frame again, bit for bit
            renderer.camera_mut().set_pos({30.0f, 0.3f, -2.5f});
            renderer.render_frame();
            ArtStats far = renderer.stats();
            renderer.camera_mut().set_pos({0.0f, 0.3f, -2.5f});
            renderer.render_frame();
            std::vector<float> again = renderer.color_output();
            ArtStats st3 = renderer.stats();
            std::printf("RESIDENT_OK hit_when_out=%llu tris_when_out=%u tris_back=%u rebuilds=%u refits=%u back_equals_first=%d\n", (unsigned long long)far.hit_pixels, far.num_triangles, st3.num_triangles,
                        st3.rebuilds, st3.refits, (int)(std::memcmp(again.data(), c.data(), c.size() * sizeof(float)) == 0));
            return 0;
        }
        if (argc >= 3 && !std::strcmp(argv[1], "deform")) {
            uint32_t W = argc >= 5 ? (uint32_t)std::atoi(argv[3]) : 800, H = argc >= 5 ? (uint32_t)std::atoi(argv[4]) : 800;
            // the first primitive's own 48-byte vertices, as art_scene_add_glb takes them
            std::vector<ArtVertex> orig;
            {
                art::GltfModelReader r = art::GltfModelReader::open(argv[2], true, art::GltfModelReader::B8G8R8A8_UNORM);
                uint32_t n = 0; art::check_glb(art_glb_primitive_count(r.handle(), &n));
                const uint32_t attrs = ART_ATTR_VERTICES | ART_ATTR_TEX_COORDS | ART_ATTR_NORMALS | ART_ATTR_TANGENTS;
                std::vector<ArtGlbCopyInfo> infos(n ? n : 1); size_t total = 0;
                art::check_glb(art_glb_copy_model_data(r.handle(), attrs, 0, nullptr, 0, infos.data(), n, &total));
                std::vector<uint8_t> data(total ? total : 1);
                art::check_glb(art_glb_copy_model_data(r.handle(), attrs, 0, data.data(), data.size(), infos.data(), n, &total));
                orig.resize(infos[0].mesh_size / sizeof(ArtVertex));
                std::memcpy(orig.data(), data.data() + infos[0].mesh_buffer_offset, orig.size() * sizeof(ArtVertex));
            }
            art::Renderer renderer(W, H);
            renderer.add_model(argv[2], {2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0});
            renderer.lights_mut().get_spot_lights_mut().push_back(art::SpotLight({0.0f, 1.5f, 0.0f}, {0.0f, -1.0f, 0.0f}, {13.6f, 1.6f, 22.2f}, 3.0f, {0.5236f, 0.7854f}, true));
            renderer.lights_mut().get_point_lights_mut().push_back(art::PointLight({0.0f, 0.5f, -1.5f}, {8, 8, 8}, 6.0f, true));
            renderer.camera_mut().set_pos({0.0f, 0.3f, -2.5f});
            renderer.prepare_first_frame();
            renderer.render_frame();
            std::vector<float> c = renderer.color_output();
            art::Model &m = renderer.models_mut()[0];
            const float r0 = m.model_bounding_sphere.radius;
            // the BLAS update: the first primitive grown from the origin, its normals turned -- the next frame refits, the one after the way back is the first frame again
            std::vector<ArtVertex> def = orig;
            for (ArtVertex &v : def) { for (int k = 0; k < 3; k++) v.pos[k] *= 1.5f; v.normal[0] = -v.normal[0]; }
            m.set_vertices(0, def.data(), (uint32_t)def.size());
            const float r1 = m.model_bounding_sphere.radius;
            renderer.render_frame();
            std::vector<float> deformed = renderer.color_output();
            m.set_vertices(0, orig.data(), (uint32_t)orig.size());
            const float r2 = m.model_bounding_sphere.radius;
            renderer.render_frame();
            std::vector<float> back = renderer.color_output();
            ArtStats st = renderer.stats();
            std::printf("DEFORM_OK verts=%zu refits=%u rebuilds=%u deformed_differs=%d back_equals_first=%d radius=%.6f,%.6f,%.6f\n", orig.size(), st.refits, st.rebuilds, (int)(deformed != c),
                        (int)(std::memcmp(back.data(), c.data(), c.size() * sizeof(float)) == 0), r0, r1, r2);
            return 0;
        }
        if (argc >= 3 && !std::strcmp(argv[1], "alpha")) {
            // alpha-masked primitives: the model added with alpha_mask (MASK materials whose base colour has alpha get their alphaCutoff), the same model with the
            // cutoffs set by hand from the reader, and the model as the reference draws it (opaque): the first two frames are equal bit for bit, the third differs
            uint32_t W = argc >= 5 ? (uint32_t)std::atoi(argv[3]) : 800, H = argc >= 5 ? (uint32_t)std::atoi(argv[4]) : 800;
            std::vector<std::pair<uint32_t, float>> by_hand;
            {
                art::GltfModelReader r = art::GltfModelReader::open(argv[2], true, art::GltfModelReader::B8G8R8A8_UNORM);
                uint32_t n = 0; art::check_glb(art_glb_primitive_count(r.handle(), &n));
                for (uint32_t i = 0; i < n; i++) {
                    int32_t mode = 0, has = 0; float c = 0.f;
                    art::check_glb(art_glb_primitive_alpha(r.handle(), i, &mode, &c, &has));
                    if (mode == 1 && has) by_hand.push_back({i, c});
                }
            }
            auto frame = [&](int how, ArtStats &st) {   // 0: alpha_mask, 1: by hand, 2: opaque
                art::Renderer renderer(W, H);
                renderer.add_model(argv[2], {2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0}, how == 0);
                renderer.lights_mut().get_spot_lights_mut().push_back(art::SpotLight({0.0f, 1.5f, 0.0f}, {0.0f, -1.0f, 0.0f}, {13.6f, 1.6f, 22.2f}, 3.0f, {0.5236f, 0.7854f}, true));
                renderer.lights_mut().get_point_lights_mut().push_back(art::PointLight({0.0f, 0.5f, -1.5f}, {8, 8, 8}, 6.0f, true));
                renderer.camera_mut().set_pos({0.0f, 0.3f, -2.5f});
                renderer.prepare_first_frame();
                if (how == 1) for (auto &bh : by_hand) renderer.models_mut()[0].set_alpha_cutoff(bh.first, bh.second);
                renderer.render_frame();
                renderer.compute_ao();
                st = renderer.stats();
                std::vector<float> c = renderer.color_output(), d = renderer.depth_output();
                std::vector<uint32_t> ao = renderer.ao_output();
                std::vector<uint8_t> all(c.size() * 4 + d.size() * 4 + ao.size() * 4);
                std::memcpy(all.data(), c.data(), c.size() * 4); std::memcpy(all.data() + c.size() * 4, d.data(), d.size() * 4); std::memcpy(all.data() + c.size() * 4 + d.size() * 4, ao.data(), ao.size() * 4);
                return all;
            };
            ArtStats s0, s1, s2;
            std::vector<uint8_t> masked = frame(0, s0), hand = frame(1, s1), opaque = frame(2, s2);
            std::printf("ALPHA_OK masked_prims=%zu masked_equals_by_hand=%d differs_from_opaque=%d hit_masked=%llu hit_opaque=%llu shadow_masked=%llu shadow_opaque=%llu rebuilds=%u\n", by_hand.size(),
                        (int)(masked == hand), (int)(masked != opaque), (unsigned long long)s0.hit_pixels, (unsigned long long)s2.hit_pixels, (unsigned long long)s0.shadow_rays,
                        (unsigned long long)s2.shadow_rays, s1.rebuilds);
            return 0;
        }
        if (argc >= 3 && !std::strcmp(argv[1], "masks")) {
            // ray visibility masks: the model's last primitive (planar, so it cannot occlude rays that start on itself) gets the mask CAMERA | AO while primary / shadow / AO
            // rays carry CAMERA / SHADOW / AO: it is seen but casts no shadow.  That frame is a composite of two others, bit for bit: the plain frame where the primary hit is
            // that primitive, the frame without it (disabled) everywhere else.
            uint32_t W = argc >= 5 ? (uint32_t)std::atoi(argv[3]) : 800, H = argc >= 5 ? (uint32_t)std::atoi(argv[4]) : 800;
            std::vector<int32_t> ids((size_t)W * H * 2);
            auto frame = [&](int how, ArtStats &st, int32_t &last) {   // 0: plain, 1: the last primitive disabled, 2: seen but shadowless
                art::Renderer renderer(W, H, -1, 1, ART_FLAG_KEEP_DEBUG);
                renderer.add_model(argv[2], {2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0});
                renderer.lights_mut().get_spot_lights_mut().push_back(art::SpotLight({0.0f, 1.5f, 0.0f}, {0.0f, -1.0f, 0.0f}, {13.6f, 1.6f, 22.2f}, 3.0f, {0.5236f, 0.7854f}, true));
                renderer.lights_mut().get_point_lights_mut().push_back(art::PointLight({0.0f, 0.5f, -1.5f}, {8, 8, 8}, 6.0f, true));
                renderer.camera_mut().set_pos({0.0f, 0.3f, -2.5f});
                renderer.prepare_first_frame();
                art::Model &m = renderer.models_mut()[0];
                last = (int32_t)m.primitive_ids.back();
                if (how == 1) art::check(art_scene_set_primitive_enabled(renderer.handle(), m.primitive_ids.back(), 0));
                if (how == 2) { m.set_mask(m.primitive_ids.size() - 1, ART_VIS_CAMERA | ART_VIS_AO); renderer.set_ray_masks(ART_VIS_CAMERA, ART_VIS_SHADOW, ART_VIS_AO); }
                renderer.render_frame();
                st = renderer.stats();
                if (how == 0) { std::vector<float> tuv((size_t)W * H * 4); art::check(art_read_hits(renderer.handle(), tuv.data(), ids.data(), (size_t)W * H)); }
                return renderer.color_output();
            };
            ArtStats s0, s1, s2; int32_t last = -1;
            std::vector<float> plain = frame(0, s0, last), off = frame(1, s1, last), shadowless = frame(2, s2, last);
            bool composite = true; size_t seen = 0;
            for (size_t p = 0; p < (size_t)W * H; p++) {
                const bool on_it = ids[2 * p] == last; seen += on_it;
                composite = composite && std::memcmp(&shadowless[4 * p], on_it ? &plain[4 * p] : &off[4 * p], 16) == 0;
            }
            std::printf("MASKS_OK primitive=%d seen_pixels=%zu shadowless_equals_composite=%d differs_from_plain=%d differs_from_off=%d shadow_rays=%llu shadow_rays_plain=%llu rebuilds=%u\n", last, seen,
                        (int)composite, (int)(shadowless != plain), (int)(shadowless != off), (unsigned long long)s2.shadow_rays, (unsigned long long)s0.shadow_rays, s2.rebuilds);
            return 0;
        }
        std::puts("usage: host_mirror_demo check | render <file.glb> [W H] | deform <file.glb> [W H] | alpha <file.glb> [W H] | masks <file.glb> [W H]");
        return 2;
    } catch (const art::Panic &p) {
        std::printf("PANIC(%d): %s\n", p.code, p.what());
        return 3;
    }
}
