// loupiote.hpp — header-only C++ mirror of the reference's `loupiote-core` API over the C ABI
// (include/lpt.h).  Same type and method names as reference crates/lib/src/{device,scene,renderer,
// errors}.rs and loaders/gltf.rs; wgpu arguments are dropped.  Errors that the reference returns as
// Result<_, Error> are thrown as loupiote::Error (kind mirrors errors.rs:2-6).
#pragma once
#include <array>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "lpt.h"

namespace loupiote {

struct Error : std::runtime_error {
    enum Kind { FileNotFound = 1, TextureToBufferReadFail = 2, AccelBuild = 3, Hip = 4, Rccl = 5, InvalidArg = 6 } kind;
    Error(int status, const char *msg) : std::runtime_error(msg), kind(static_cast<Kind>(status)) {}
};
inline void check(int status) {
    if (status != LPT_OK) throw Error(status, lpt_last_error());
}

enum class BlitMode { Pahtrace = 0, DenoisedPathrace = 1, Temporal = 2, GBuffer = 3, MotionVector = 4 };  // renderer.rs:160-167
using Mat4 = std::array<float, 16>;  // column-major (glam::Mat4::to_cols_array)

class Device {  // device.rs:72-141
   public:
    explicit Device(int hip_ordinal = 0) { check(lpt_device_create(hip_ordinal, &h_)); }
    ~Device() { lpt_device_destroy(h_); }
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    lpt_device *inner() const { return h_; }
    void synchronize() { check(lpt_device_synchronize(h_)); }
    /// SPEC.md §21, the shading kernels' interface event on the GPU, once per element (see lpt_interface_sample)
    void interface_sample(uint32_t n, const float *dirs, const float *ns, const float *ngf, const uint32_t *entering, const float *base, const float *ior,
                          const uint32_t *thin, const float *r4, float *wi, float *weight, uint32_t *kind) const {
        check(lpt_interface_sample(h_, n, dirs, ns, ngf, entering, base, ior, thin, r4, wi, weight, kind));
    }
    /// SPEC.md §29, the interface event of a material whose rough bit is set, once per element: in[n][19] -> out[n][6], kind[n] (see lpt_interface_sample_rough)
    void interface_sample_rough(uint32_t n, const float *in, float *out, uint32_t *kind) const { check(lpt_interface_sample_rough(h_, n, in, out, kind)); }
    /// SPEC.md §10, the shading kernels' BSDF on the GPU, once per element: in[n][20] -> out[n][12], ok[n] (see lpt_bsdf_probe)
    void bsdf_probe(uint32_t n, const float *in, float *out, uint32_t *ok) const { check(lpt_bsdf_probe(h_, n, in, out, ok)); }

   private:
    lpt_device *h_ = nullptr;
};

// one rank of the multi-GPU frame exchange (new functionality; plain RCCL inside the library, include/lpt.h)
class Comm {
   public:
    using Id = std::array<unsigned char, LPT_COMM_ID_BYTES>;
    static Id unique_id() { Id id{}; check(lpt_comm_unique_id(id.data())); return id; }   // on ONE rank; ship the bytes to the others
    Comm(const Device &dev, const Id &id, int rank, int world) { check(lpt_comm_create(dev.inner(), id.data(), rank, world, &h_)); }
    ~Comm() { lpt_comm_destroy(h_); }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    lpt_comm *handle() const { return h_; }

   private:
    lpt_comm *h_ = nullptr;
};

class Scene {  // scene.rs:30-54
   public:
    Scene() { check(lpt_scene_create(&h_)); }
    ~Scene() { lpt_scene_destroy(h_); }
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;
    lpt_scene *handle() const { return h_; }
    // BLASArray::add_bvh / add_bvh_indexed (gltf.rs:97-105); strides in bytes
    uint32_t add_bvh(const void *positions, size_t pstride, const void *normals, size_t nstride, const void *uvs, size_t ustride,
                     uint32_t vertex_count, const uint32_t *indices = nullptr, uint32_t index_count = 0) {
        uint32_t id = 0;
        check(lpt_scene_add_mesh(h_, positions, pstride, normals, nstride, uvs, ustride, vertex_count, indices, index_count, &id));
        return id;
    }
    uint32_t add_instance(uint32_t blas, const Mat4 &model_to_world, uint32_t material) {  // gltf.rs:141-145
        uint32_t id = 0;
        check(lpt_scene_add_instance(h_, blas, model_to_world.data(), material, &id));
        return id;
    }
    void set_instance_transform(uint32_t i, const Mat4 &m) { check(lpt_scene_set_instance_transform(h_, i, m.data())); }
    uint32_t add_material(const lpt_material &m) { uint32_t id = 0; check(lpt_scene_add_material(h_, &m, &id)); return id; }
    uint32_t add_image(const uint8_t *rgba8, uint32_t w, uint32_t h) { uint32_t id = 0; check(lpt_scene_add_image(h_, rgba8, w, h, &id)); return id; }
    uint32_t add_light(const lpt_light &l) { uint32_t id = 0; check(lpt_scene_add_light(h_, &l, &id)); return id; }
    void set_light(uint32_t i, const lpt_light &l) { check(lpt_scene_set_light(h_, i, &l)); }
    // SPEC.md §20: alpha-masked (cutout) materials; mode LPT_ALPHA_OPAQUE / LPT_ALPHA_MASK, alpha_image an image index or LPT_INVALID_INDEX
    struct MaterialAlpha { uint32_t mode; float cutoff; uint32_t alpha_image; };
    void set_material_alpha(uint32_t material, uint32_t mode, float cutoff = 0.5f, uint32_t alpha_image = LPT_INVALID_INDEX) {
        check(lpt_scene_set_material_alpha(h_, material, mode, cutoff, alpha_image));
    }
    // SPEC.md §26: alpha-blended (stochastic coverage); material_alpha then reports LPT_ALPHA_BLEND, set_material_alpha with mode 0 or 1 changes it back
    void set_material_alpha_blend(uint32_t material, uint32_t alpha_image = LPT_INVALID_INDEX) { check(lpt_scene_set_material_alpha_blend(h_, material, alpha_image)); }
    MaterialAlpha material_alpha(uint32_t material) const {
        MaterialAlpha a{};
        check(lpt_scene_get_material_alpha(h_, material, &a.mode, &a.cutoff, &a.alpha_image));
        return a;
    }
    // SPEC.md §21: transmissive materials (glass); factor 0 = opaque, thin_walled: a pane without thickness, else the boundary of a closed solid
    struct MaterialTransmission { float factor; float ior; bool thin_walled; };
    void set_material_transmission(uint32_t material, float factor, float ior = 1.5f, bool thin_walled = true) {
        check(lpt_scene_set_material_transmission(h_, material, factor, ior, thin_walled ? 1u : 0u));
    }
    MaterialTransmission material_transmission(uint32_t material) const {
        MaterialTransmission t{};
        uint32_t thin = 0;
        check(lpt_scene_get_material_transmission(h_, material, &t.factor, &t.ior, &thin));
        t.thin_walled = thin != 0;
        return t;
    }
    // SPEC.md §29: rough transmission; one bit beside the transmission state, which set_material_transmission leaves alone.  It frosts the interface by the material's roughness
    void set_material_transmission_rough(uint32_t material, bool on) { check(lpt_scene_set_material_transmission_rough(h_, material, on ? 1u : 0u)); }
    bool material_transmission_rough(uint32_t material) const {
        uint32_t on = 0;
        check(lpt_scene_get_material_transmission_rough(h_, material, &on));
        return on != 0;
    }
    // SPEC.md §28: volume attenuation (glTF attenuationColor / attenuationDistance) of a solid transmissive material; colour (1, 1, 1) or distance +inf: none
    struct MaterialAttenuation { float color[3]; float distance; float sigma[3]; };
    void set_material_attenuation(uint32_t material, const float color[3], float distance = std::numeric_limits<float>::infinity()) {
        check(lpt_scene_set_material_attenuation(h_, material, color, distance));
    }
    MaterialAttenuation material_attenuation(uint32_t material) const {
        MaterialAttenuation a{};
        check(lpt_scene_get_material_attenuation(h_, material, a.color, &a.distance, a.sigma));
        return a;
    }
    // SPEC.md §22: emissive materials; Le = factor x strength per channel, times the sRGB emissive image where one is given; a product of 0: non-emissive again
    struct MaterialEmission { float le[3]; uint32_t image; };
    void set_material_emission(uint32_t material, const float factor[3], float strength = 1.0f, uint32_t image = LPT_INVALID_INDEX) {
        check(lpt_scene_set_material_emission(h_, material, factor, strength, image));
    }
    MaterialEmission material_emission(uint32_t material) const {
        MaterialEmission e{};
        check(lpt_scene_get_material_emission(h_, material, e.le, &e.image));
        return e;
    }
    // SPEC.md §23: the emissive triangles' sampling distribution, on the host; returns the number of entries (up to `cap` of them are written)
    uint32_t emitter_distribution(uint32_t cap, float *q, uint32_t *alias, uint32_t *prim_self, uint32_t *prim_alias, double *sum_w = nullptr) const {
        uint32_t n = 0;
        check(lpt_scene_emitter_distribution(h_, cap, q, alias, prim_self, prim_alias, &n, sum_w));
        return n;
    }
    // SPEC.md §24: normal maps; image = LPT_INVALID_INDEX removes the map
    struct MaterialNormalMap { uint32_t image; float scale; };
    void set_material_normal_map(uint32_t material, uint32_t image, float scale = 1.0f) { check(lpt_scene_set_material_normal_map(h_, material, image, scale)); }
    MaterialNormalMap material_normal_map(uint32_t material) const {
        MaterialNormalMap m{};
        check(lpt_scene_get_material_normal_map(h_, material, &m.image, &m.scale));
        return m;
    }
    // SPEC.md §19: point / spot / directional lights (KHR_lights_punctual); records from point_light / spot_light / directional_light below
    uint32_t add_punctual_light(const lpt_punctual_light &l) { uint32_t id = 0; check(lpt_scene_add_punctual_light(h_, &l, &id)); return id; }
    void set_punctual_light(uint32_t i, const lpt_punctual_light &l) { check(lpt_scene_set_punctual_light(h_, i, &l)); }
    std::vector<lpt_punctual_light> punctual_lights() const {
        uint32_t n = 0;
        check(lpt_scene_punctual_count(h_, &n));
        std::vector<lpt_punctual_light> out(n);
        check(lpt_scene_get_punctual_lights(h_, 0, n, out.data()));
        return out;
    }
    lpt_scene_counts counts() const { lpt_scene_counts c; check(lpt_scene_counts_get(h_, &c)); return c; }

   private:
    lpt_scene *h_ = nullptr;
};

using Vec3 = std::array<float, 3>;
inline lpt_punctual_light point_light(const Vec3 &position, const Vec3 &color = {1.f, 1.f, 1.f}, float intensity = 1.f, float range = 0.f) {
    lpt_punctual_light l;
    check(lpt_punctual_light_make(LPT_PUNCTUAL_POINT, position.data(), nullptr, color.data(), intensity, range, 0.f, 0.f, &l));
    return l;
}
inline lpt_punctual_light spot_light(const Vec3 &position, const Vec3 &direction, const Vec3 &color = {1.f, 1.f, 1.f}, float intensity = 1.f, float range = 0.f,
                                     float inner_angle = 0.f, float outer_angle = 0.78539816f) {
    lpt_punctual_light l;
    check(lpt_punctual_light_make(LPT_PUNCTUAL_SPOT, position.data(), direction.data(), color.data(), intensity, range, inner_angle, outer_angle, &l));
    return l;
}
inline lpt_punctual_light directional_light(const Vec3 &direction, const Vec3 &color = {1.f, 1.f, 1.f}, float intensity = 1.f) {
    lpt_punctual_light l;
    check(lpt_punctual_light_make(LPT_PUNCTUAL_DIRECTIONAL, nullptr, direction.data(), color.data(), intensity, 0.f, 0.f, 0.f, &l));
    return l;
}

namespace loaders {  // loaders/gltf.rs:46-161
inline void load_gltf(const uint8_t *data, size_t size, Scene &scene) { check(lpt_load_gltf(scene.handle(), data, size)); }
inline void load_gltf_path(const std::string &path, Scene &scene) { check(lpt_load_gltf_path(scene.handle(), path.c_str())); }
// flags: LPT_GLTF_READ_BLEND marks alphaMode "BLEND" materials blended (SPEC.md §26) instead of loading them as opaque; LPT_GLTF_READ_ROUGH_TRANSMISSION marks
// transmissive materials rough, so their roughnessFactor frosts them (SPEC.md §29); 0 is the loaders above
inline void load_gltf(const uint8_t *data, size_t size, Scene &scene, uint32_t flags) { check(lpt_load_gltf_ex(scene.handle(), data, size, flags)); }
inline void load_gltf_path(const std::string &path, Scene &scene, uint32_t flags) { check(lpt_load_gltf_path_ex(scene.handle(), path.c_str(), flags)); }
/// the decoding half of ApplicationContext::load_env (app.rs:138-155): Radiance .hdr bytes -> RGBE8 pixels for ProbeGPU
inline std::vector<uint8_t> load_env(const uint8_t *data, size_t size, uint32_t &width, uint32_t &height) {
    check(lpt_decode_hdr(data, size, nullptr, 0, &width, &height));
    std::vector<uint8_t> px((size_t)width * height * 4);
    check(lpt_decode_hdr(data, size, px.data(), px.size(), &width, &height));
    return px;
}
}  // namespace loaders

class SceneGPU {  // scene.rs:56-64,151-188
   public:
    static SceneGPU new_from_scene(const Scene &scene, const Device &device, bool gpu_build = false) {
        SceneGPU s;
        check(lpt_scene_upload_ex(device.inner(), scene.handle(), gpu_build ? LPT_ACCEL_BUILD_GPU_LBVH : LPT_ACCEL_BUILD_HOST_SAH, &s.h_));
        return s;
    }
    SceneGPU(SceneGPU &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~SceneGPU() { lpt_scene_gpu_destroy(h_); }
    lpt_scene_gpu *handle() const { return h_; }
    lpt_accel_stats stats() const { lpt_accel_stats s; check(lpt_scene_gpu_stats(h_, &s)); return s; }
    /// re-bake the instances whose transform changed and refit the BVH on the GPU (standalone/src/lib.rs:118-121)
    /// re-bake every instance and rebuild the BVH on the GPU (for edits too large for a refit)
    void rebuild(const Scene &scene) { check(lpt_scene_gpu_rebuild(h_, scene.handle())); }
    uint32_t update_instances(const Scene &scene) { uint32_t n = 0; check(lpt_scene_gpu_update_instances(h_, scene.handle(), &n)); return n; }
    /// SPEC.md §19: the punctual lights to the device again, nothing else (same count; recorded frames are submitted first and see the old lights)
    void update_punctual(const Scene &scene) { check(lpt_scene_gpu_update_punctual(h_, scene.handle())); }
    /// the shading kernels' punctual-light function on the GPU: points[n][3] -> wi[n][3], dist[n], E[n][3]
    void sample_punctual(const Device &device, uint32_t light, const float *points, uint32_t n, float *wi, float *dist, float *E) const {
        check(lpt_scene_gpu_sample_punctual(device.inner(), h_, light, points, n, wi, dist, E));
    }
    // SPEC.md §23: the shading kernels' emitter sample, rands[n][4] = {ra, rb, r1, r2} per point
    // SPEC.md §24: the shading normal the shading kernels use at (prim, bary) seen along dirs, for tools and tests
    void shading_normal(const Device &device, uint32_t n, const uint32_t *prim, const float *bary, const float *dirs, float *ns_out, uint32_t *mapped_out) const {
        check(lpt_scene_gpu_shading_normal(device.inner(), h_, n, prim, bary, dirs, ns_out, mapped_out));
    }
    // SPEC.md §9: what a hit (prim, bary) reads from its textures through the shading kernels' lookups, out[n][16] (lpt.h), for tools and tests
    void sample_textures(const Device &device, uint32_t n, const uint32_t *prim, const float *bary, float *out) const {
        check(lpt_scene_gpu_sample_textures(device.inner(), h_, n, prim, bary, out));
    }
    // SPEC.md §27: what a punctual light's shadow ray along dirs is answered at (prim, bary) by the traversal's own function, out[n][8] (lpt.h), for tools and tests
    void glass_shadow(const Device &device, uint32_t n, const uint32_t *prim, const float *bary, const float *dirs, float *out) const {
        check(lpt_scene_gpu_glass_shadow(device.inner(), h_, n, prim, bary, dirs, out));
    }
    // SPEC.md §28: the volume attenuation of a hit of prim along dirs at distance t by the shading kernels' own function, out[n][4] (lpt.h), for tools and tests
    void attenuation(const Device &device, uint32_t n, const uint32_t *prim, const float *dirs, const float *t, float *out) const {
        check(lpt_scene_gpu_attenuation(device.inner(), h_, n, prim, dirs, t, out));
    }
    void sample_emitter(const Device &device, uint32_t n, const float *points, const float *rands, uint32_t *prim, uint32_t *sampled, float *y, float *wi, float *dist, float *cl,
                        float *p_a, float *E) const {
        check(lpt_scene_gpu_sample_emitter(device.inner(), h_, n, points, rands, prim, sampled, y, wi, dist, cl, p_a, E));
    }

   private:
    SceneGPU() = default;
    lpt_scene_gpu *h_ = nullptr;
};

class ProbeGPU {  // scene.rs:66-121
   public:
    ProbeGPU(const Device &device, const uint8_t *rgbe8, uint32_t width, uint32_t height) { check(lpt_probe_upload(device.inner(), rgbe8, width, height, &h_)); }
    ~ProbeGPU() { lpt_probe_destroy(h_); }
    ProbeGPU(const ProbeGPU &) = delete;
    lpt_probe *handle() const { return h_; }
    /// SPEC.md §18, the renderer's sampler on the GPU: uniforms[n][6] = {r6, r7, r8, r9, r1, r2} -> dirs[n][3], pdf_s[n], radiance[n][3]
    void sample(const Device &device, const float *uniforms, uint32_t n, float *dirs, float *pdf_s, float *radiance) const {
        check(lpt_probe_sample(device.inner(), h_, uniforms, n, dirs, pdf_s, radiance));
    }
    void pdf(const Device &device, const float *dirs, uint32_t n, float *pdf_e) const { check(lpt_probe_pdf(device.inner(), h_, dirs, n, pdf_e)); }
    /// SPEC.md §9: the probe's radiance along dirs[n][3] -> radiance[n][3]
    void lookup(const Device &device, const float *dirs, uint32_t n, float *radiance) const { check(lpt_probe_lookup(device.inner(), h_, dirs, n, radiance)); }

   private:
    lpt_probe *h_ = nullptr;
};

class Renderer {  // renderer.rs:169-811
   public:
    float downsample_factor = 0.5f;  // pub field, renderer.rs:203
    bool accumulate = false;         // pub field, renderer.rs:204

    Renderer(const Device &device, uint32_t width, uint32_t height) { check(lpt_renderer_create(device.inner(), width, height, &h_)); }
    ~Renderer() { lpt_renderer_destroy(h_); }
    Renderer(const Renderer &) = delete;
    static uint32_t max_ssbo_element_in_bytes() { return lpt_max_per_pixel_bytes(); }
    void resize(const SceneGPU &scene, const ProbeGPU *probe, uint32_t width, uint32_t height) {
        check(lpt_renderer_set_downsample(h_, downsample_factor));
        check(lpt_renderer_resize(h_, scene.handle(), probe ? probe->handle() : nullptr, width, height));
    }
    void set_resources(const SceneGPU &scene, const ProbeGPU *probe = nullptr) { check(lpt_renderer_set_resources(h_, scene.handle(), probe ? probe->handle() : nullptr)); }
    void raytrace(const Mat4 &view_transform) {
        check(lpt_renderer_set_accumulate(h_, accumulate ? 1 : 0));
        check(lpt_renderer_raytrace(h_, view_transform.data()));
    }
    /// queue.submit(encoder.finish()) (app.rs:335-337): launches what raytrace() has recorded; asynchronous
    void submit() { check(lpt_renderer_submit(h_)); }
    void reset_accumulation() { accumulate = false; check(lpt_renderer_reset_accumulation(h_)); }
    void upload_noise_texture(const uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t bytes_per_row) { check(lpt_renderer_upload_noise(h_, rgba8, w, h, bytes_per_row)); }
    void use_noise_texture(bool flag) { check(lpt_renderer_use_noise(h_, flag ? 1 : 0)); }
    void set_blit_mode(BlitMode m) { check(lpt_renderer_set_blit_mode(h_, static_cast<int>(m))); }
    std::pair<uint32_t, uint32_t> get_size() const { uint32_t w = 0, h = 0; check(lpt_renderer_get_size(h_, &w, &h)); return {w, h}; }
    std::vector<uint8_t> read_pixels() {
        auto [w, h] = get_size();
        std::vector<uint8_t> out(static_cast<size_t>(w) * h * 4);
        check(lpt_renderer_read_pixels(h_, out.data()));
        return out;
    }
    void blit(uint8_t *dst, size_t row_bytes) { check(lpt_renderer_blit_rgba8(h_, dst, row_bytes)); }
    // build-only extensions
    std::vector<float> read_radiance() {
        auto [w, h] = get_size();
        std::vector<float> out(static_cast<size_t>(w) * h * 4);
        check(lpt_renderer_read_radiance(h_, out.data()));
        return out;
    }
    void set_max_bounces(uint32_t n) { check(lpt_renderer_set_max_bounces(h_, n)); }
    /// SPEC.md §18: next-event estimation samples the environment probe too (off by default; frames change with it)
    void set_env_sampling(bool on) { check(lpt_renderer_set_env_sampling(h_, on ? 1 : 0)); }
    bool env_sampling() const { int f = 0; check(lpt_renderer_get_env_sampling(h_, &f)); return f != 0; }
    // SPEC.md §23: next-event estimation samples the emissive triangles too; off by default
    void set_emissive_sampling(bool on) { check(lpt_renderer_set_emissive_sampling(h_, on ? 1 : 0)); }
    bool emissive_sampling() const { int f = 0; check(lpt_renderer_get_emissive_sampling(h_, &f)); return f != 0; }
    // SPEC.md §27: punctual lights' shadow rays pass thin-walled transmissive triangles (off by default)
    void set_glass_shadows(bool on) { check(lpt_renderer_set_glass_shadows(h_, on ? 1 : 0)); }
    bool glass_shadows() const { int f = 0; check(lpt_renderer_get_glass_shadows(h_, &f)); return f != 0; }
    /// SPEC.md §25: a thin-lens camera — lens radius in world units (0, the default: the pinhole) and the distance of the plane in focus; frames change with it, so reset_accumulation() belongs after the call
    void set_lens(float radius, float focus_distance = 1.0f) { check(lpt_renderer_set_lens(h_, radius, focus_distance)); }
    std::pair<float, float> lens() const { float r = 0.f, f = 0.f; check(lpt_renderer_get_lens(h_, &r, &f)); return {r, f}; }
    /// SPEC.md §30: the display transform of blit / read_pixels — the mean times 2^exposure_ev, then LPT_DISPLAY_CLAMP (the default), LPT_DISPLAY_PBR_NEUTRAL or LPT_DISPLAY_ACES, then sRGB; nothing is rendered or reset, the float outputs stay linear
    void set_display(float exposure_ev = 0.0f, uint32_t op = LPT_DISPLAY_CLAMP) { check(lpt_renderer_set_display(h_, exposure_ev, op)); }
    std::pair<float, uint32_t> display() const { float ev = 0.f; uint32_t op = 0; check(lpt_renderer_get_display(h_, &ev, &op)); return {ev, op}; }
    /// SPEC.md §30.3: the exposure that puts the mean log2 luminance of the presented frame at 18 % grey, without its darkest `low` and brightest `high` fraction; `hist384` (384 words) may be null.  Nothing is set: pass the result to set_display
    float meter(float low = 0.5f, float high = 0.02f, uint32_t *hist384 = nullptr, uint32_t *counted = nullptr, uint32_t *skipped = nullptr) { float ev = 0.f; check(lpt_renderer_meter(h_, low, high, &ev, hist384, counted, skipped)); return ev; }
    /// SPEC.md §25, for tests and tools: the primary rays of sample `sample` of the next raytrace(), 3 floats per pixel of the full frame each (zeros at pixels this rank does not own)
    void primary_rays(const Mat4 &view_transform, uint32_t sample, float *origins, float *dirs) { check(lpt_renderer_primary_rays(h_, view_transform.data(), sample, origins, dirs)); }
    void set_seed(uint32_t s) { check(lpt_renderer_set_seed(h_, s)); }
    void set_vfov(float radians) { check(lpt_renderer_set_vfov(h_, radians)); }
    /// `weights` (one small integer per rank, the same on every rank; nullptr = equal shares): unequal tile shares, e.g. fewer tiles for the rank that also assembles the frame
    void set_shard(uint32_t rank, uint32_t world, uint32_t tile_w = 32, uint32_t tile_h = 8, const uint32_t *weights = nullptr) { check(lpt_renderer_set_shard_weighted(h_, rank, world, tile_w, tile_h, weights)); }
    void set_comm(const Comm *comm, const uint32_t *weights = nullptr) { check(lpt_renderer_set_comm_weighted(h_, comm ? comm->handle() : nullptr, weights)); }     // = set_shard(rank, world, 32, 8, weights) + the binding
    void exchange(int mode = LPT_EXCHANGE_GATHER_TILES) { check(lpt_renderer_exchange(h_, mode)); }             // rank 0 presents the whole frame
    void set_sort_queues(int flag) { check(lpt_renderer_set_sort_queues(h_, flag)); }
    void set_option(lpt_option option, uint64_t value) { check(lpt_renderer_set_option(h_, (int)option, value)); }
    uint64_t get_option(lpt_option option) const { uint64_t v = 0; check(lpt_renderer_get_option(h_, (int)option, &v)); return v; }
    lpt_ray_counts ray_counts() { lpt_ray_counts c; check(lpt_renderer_get_ray_counts(h_, &c)); return c; }
    /// multi-GPU denoising: this rank's filter inputs (device pointers) and, on rank 0 after the exchange, the filter passes
    void denoiser_inputs(void **noisy, void **gbuffer, void **motion, size_t *n_pixels) { check(lpt_renderer_denoiser_inputs(h_, noisy, gbuffer, motion, n_pixels)); }
    void denoise_filter() { check(lpt_renderer_denoise_filter(h_)); }
    lpt_renderer *handle() const { return h_; }

   private:
    lpt_renderer *h_ = nullptr;
};

}  // namespace loupiote
