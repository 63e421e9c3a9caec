// scene.cpp — status/error plumbing and the CPU-side Scene (flat arrays).
// Mirrors reference crates/lib/src/scene.rs:30-54 (Scene::default with one dummy
// element per array) and crates/lib/src/errors.rs (Error -> String).
#include <cmath>

#include "common.h"

namespace lpt {

static thread_local char g_error[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
int fail(int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return status;
}

static void identity(float m[16]) {
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
}

static inline void normalize3(float v[3]) {
    float l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (!(l2 > 0.f)) { v[0] = v[1] = v[2] = 0.f; return; }
    float inv = 1.0f / sqrtf(l2);
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
}

}  // namespace lpt

using namespace lpt;

extern "C" {

const char *lpt_last_error(void) { return g_error; }

const char *lpt_status_string(int status) {
    switch (status) {
        case LPT_OK: return "ok";
        case LPT_ERR_FILE_NOT_FOUND: return "file not found";
        case LPT_ERR_READBACK: return "failed to read pixels from GPU to CPU";
        case LPT_ERR_ACCEL_BUILD: return "failed to build acceleration structure";
        case LPT_ERR_HIP: return "HIP runtime error";
        case LPT_ERR_RCCL: return "RCCL error";
        case LPT_ERR_INVALID_ARG: return "invalid argument";
    }
    return "unknown status";
}

uint32_t lpt_abi_version(void) { return LPT_ABI_VERSION; }

int lpt_light_default(lpt_light *out) {
    if (!out) return fail(LPT_ERR_INVALID_ARG, "lpt_light_default: null");
    const lpt_light l = {{0.f, 0.f, 1.f, 0.f}, {1.f, 0.f, 0.f, 0.5f}, {0.f, 1.f, 0.f, 0.5f}, {0.f, 0.f, 0.f, 1.f}};
    *out = l;
    return LPT_OK;
}

int lpt_scene_create(lpt_scene **out) {
    if (!out) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_create: null out");
    lpt_scene *s = new lpt_scene();
    lpt_material m = {{1.f, 1.f, 1.f, 1.f}, 1.f, 0.f, LPT_INVALID_INDEX, LPT_INVALID_INDEX};
    s->materials.push_back(m);
    s->entries.push_back(lpt_blas_entry{0, 0, 0, 0});
    s->vertices.push_back(lpt_vertex{{0, 0, 0, 0}, {0, 0, 0, 0}});
    lpt_instance inst;
    memset(&inst, 0, sizeof inst);
    identity(inst.model_to_world);
    s->instances.push_back(inst);
    lpt_light l;
    lpt_light_default(&l);
    s->lights.push_back(l);
    *out = s;
    return LPT_OK;
}

int lpt_scene_destroy(lpt_scene *scene) {
    delete scene;
    return LPT_OK;
}

int lpt_scene_counts_get(const lpt_scene *s, lpt_scene_counts *out) {
    if (!s || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_counts_get: null");
    out->materials = (uint32_t)s->materials.size();
    out->entries = (uint32_t)s->entries.size();
    out->vertices = (uint32_t)s->vertices.size();
    out->indices = (uint32_t)s->indices.size();
    out->instances = (uint32_t)s->instances.size();
    out->lights = (uint32_t)s->lights.size();
    out->images = (uint32_t)s->images.size();
    return LPT_OK;
}

int lpt_scene_add_mesh(lpt_scene *s, const void *positions, size_t position_stride, const void *normals,
                       size_t normal_stride, const void *uvs, size_t uv_stride, uint32_t vertex_count,
                       const uint32_t *indices, uint32_t index_count, uint32_t *out_blas_index) {
    if (!s || (!positions && vertex_count)) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_mesh: null");
    if (position_stride < 12 || (normals && normal_stride < 12) || (uvs && uv_stride < 8))
        return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_mesh: stride too small");
    const uint32_t n_idx = indices ? index_count : vertex_count;
    if (n_idx % 3u != 0u) return fail(LPT_ERR_ACCEL_BUILD, "index count %u is not a multiple of 3", n_idx);
    if (indices)
        for (uint32_t i = 0; i < index_count; ++i)
            if (indices[i] >= vertex_count)
                return fail(LPT_ERR_ACCEL_BUILD, "index %u out of range (%u vertices)", indices[i], vertex_count);
    // SPEC §9: the lookups' domain.  A NaN or infinite coordinate (or one so large that u x width overflows) gives NaN filter weights, and a NaN radiance never
    // leaves the accumulation buffer; checked before the scene is touched
    if (uvs)
        for (uint32_t i = 0; i < vertex_count; ++i) {
            float t[2];
            memcpy(t, (const uint8_t *)uvs + (size_t)i * uv_stride, 8);
            if (!(std::fabs(t[0]) <= LPT_UV_MAX) || !(std::fabs(t[1]) <= LPT_UV_MAX))
                return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_mesh: texture coordinate (%g, %g) of vertex %u is not finite or exceeds LPT_UV_MAX", (double)t[0], (double)t[1], i);
        }
    lpt_blas_entry e;
    e.vertex_offset = (uint32_t)s->vertices.size();
    e.vertex_count = vertex_count;
    e.index_offset = (uint32_t)s->indices.size();
    e.index_count = n_idx;
    const size_t v0 = s->vertices.size();
    s->vertices.resize(v0 + vertex_count);
    const uint8_t *pp = (const uint8_t *)positions, *pn = (const uint8_t *)normals, *pu = (const uint8_t *)uvs;
    for (uint32_t i = 0; i < vertex_count; ++i) {
        lpt_vertex &v = s->vertices[v0 + i];
        float p[3];
        memcpy(p, pp + (size_t)i * position_stride, 12);
        v.position[0] = p[0]; v.position[1] = p[1]; v.position[2] = p[2]; v.position[3] = 0.f;
        v.normal[0] = v.normal[1] = v.normal[2] = v.normal[3] = 0.f;
        if (pn) { float n[3]; memcpy(n, pn + (size_t)i * normal_stride, 12); v.normal[0] = n[0]; v.normal[1] = n[1]; v.normal[2] = n[2]; }
        if (pu) { float t[2]; memcpy(t, pu + (size_t)i * uv_stride, 8); v.position[3] = t[0]; v.normal[3] = t[1]; }
    }
    const size_t i0 = s->indices.size();
    s->indices.resize(i0 + n_idx);
    for (uint32_t i = 0; i < n_idx; ++i) s->indices[i0 + i] = indices ? indices[i] : i;
    if (!pn) {
        // vertex normal = normalize(sum, in index order, of cross(p1-p0, p2-p0)) (SPEC §2.2)
        for (uint32_t t = 0; t + 2 < n_idx; t += 3) {
            lpt_vertex *v = &s->vertices[v0];
            const uint32_t a = s->indices[i0 + t], b = s->indices[i0 + t + 1], c = s->indices[i0 + t + 2];
            const float e1[3] = {v[b].position[0] - v[a].position[0], v[b].position[1] - v[a].position[1], v[b].position[2] - v[a].position[2]};
            const float e2[3] = {v[c].position[0] - v[a].position[0], v[c].position[1] - v[a].position[1], v[c].position[2] - v[a].position[2]};
            const float fn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const uint32_t ids[3] = {a, b, c};
            for (int k = 0; k < 3; ++k)
                for (int ax = 0; ax < 3; ++ax) v[ids[k]].normal[ax] = v[ids[k]].normal[ax] + fn[ax];
        }
        for (uint32_t i = 0; i < vertex_count; ++i) normalize3(s->vertices[v0 + i].normal);
    }
    s->entries.push_back(e);
    if (out_blas_index) *out_blas_index = (uint32_t)s->entries.size() - 1u;
    return LPT_OK;
}

int lpt_scene_add_instance(lpt_scene *s, uint32_t blas_index, const float m[16], uint32_t material_index,
                           uint32_t *out_instance_index) {
    if (!s || !m) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_instance: null");
    lpt_instance inst;
    memset(&inst, 0, sizeof inst);
    memcpy(inst.model_to_world, m, sizeof(float) * 16);
    inst.blas_index = blas_index;
    inst.material_index = material_index;
    s->instances.push_back(inst);
    if (out_instance_index) *out_instance_index = (uint32_t)s->instances.size() - 1u;
    return LPT_OK;
}

int lpt_scene_set_instance_transform(lpt_scene *s, uint32_t i, const float m[16]) {
    if (!s || !m || i >= s->instances.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_instance_transform: bad index %u", i);
    memcpy(s->instances[i].model_to_world, m, sizeof(float) * 16);
    return LPT_OK;
}

int lpt_scene_add_material(lpt_scene *s, const lpt_material *m, uint32_t *out_index) {
    if (!s || !m) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_material: null");
    s->materials.push_back(*m);
    if (out_index) *out_index = (uint32_t)s->materials.size() - 1u;
    return LPT_OK;
}

// ---- alpha-masked materials (SPEC §20): a side table of `materials`, grown on the first write
int lpt_scene_set_material_alpha(lpt_scene *s, uint32_t material_index, uint32_t mode, float cutoff, uint32_t alpha_image) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha: material %u of %zu", material_index, s->materials.size());
    if (mode > LPT_ALPHA_MASK) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha: unknown mode %u", mode);
    if (!std::isfinite(cutoff) || cutoff < 0.f) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha: the cutoff must be finite and >= 0");
    if (alpha_image != LPT_INVALID_INDEX && alpha_image >= s->images.size())
        return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha: image %u of %zu", alpha_image, s->images.size());
    if (s->alpha.size() < s->materials.size()) s->alpha.resize(s->materials.size());
    MaterialAlpha &a = s->alpha[material_index];
    a.mode = mode; a.cutoff = cutoff; a.image = alpha_image;
    return LPT_OK;
}

// SPEC §26: the third state of the same table.  BLEND has no cutoff: the stored one returns to its default and is not read
int lpt_scene_set_material_alpha_blend(lpt_scene *s, uint32_t material_index, uint32_t alpha_image) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha_blend: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha_blend: material %u of %zu", material_index, s->materials.size());
    if (alpha_image != LPT_INVALID_INDEX && alpha_image >= s->images.size())
        return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_alpha_blend: image %u of %zu", alpha_image, s->images.size());
    if (s->alpha.size() < s->materials.size()) s->alpha.resize(s->materials.size());
    MaterialAlpha &a = s->alpha[material_index];
    a.mode = LPT_ALPHA_BLEND; a.cutoff = MaterialAlpha().cutoff; a.image = alpha_image;
    return LPT_OK;
}

int lpt_scene_get_material_alpha(const lpt_scene *s, uint32_t material_index, uint32_t *mode, float *cutoff, uint32_t *alpha_image) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_alpha: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_alpha: material %u of %zu", material_index, s->materials.size());
    const MaterialAlpha a = s->material_alpha(material_index);
    if (mode) *mode = a.mode;
    if (cutoff) *cutoff = a.cutoff;
    if (alpha_image) *alpha_image = a.image;
    return LPT_OK;
}

// ---- transmissive materials (SPEC §21): a second side table of `materials`, grown on the first write; factor 0 returns the material to opaque
int lpt_scene_set_material_transmission(lpt_scene *s, uint32_t material_index, float factor, float ior, uint32_t thin_walled) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_transmission: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_transmission: material %u of %zu", material_index, s->materials.size());
    if (!std::isfinite(factor) || factor < 0.f || factor > 1.f) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_transmission: the factor must lie in [0, 1]");
    if (!std::isfinite(ior) || ior < 1.f) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_transmission: the ior must be finite and >= 1");
    if (s->transmission.size() < s->materials.size()) s->transmission.resize(s->materials.size());
    MaterialTransmission &t = s->transmission[material_index];
    t.factor = factor; t.ior = ior; t.thin_walled = thin_walled ? 1u : 0u;
    return LPT_OK;
}

int lpt_scene_get_material_transmission(const lpt_scene *s, uint32_t material_index, float *factor, float *ior, uint32_t *thin_walled) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_transmission: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_transmission: material %u of %zu", material_index, s->materials.size());
    const MaterialTransmission t = s->material_transmission(material_index);
    if (factor) *factor = t.factor;
    if (ior) *ior = t.ior;
    if (thin_walled) *thin_walled = t.thin_walled;
    return LPT_OK;
}

// ---- rough transmission (SPEC §29): one bit beside the transmission state, which lpt_scene_set_material_transmission leaves alone
int lpt_scene_set_material_transmission_rough(lpt_scene *s, uint32_t material_index, uint32_t on) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_transmission_rough: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_transmission_rough: material %u of %zu", material_index, s->materials.size());
    if (on > 1u) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_transmission_rough: on must be 0 or 1");
    if (s->transmission.size() < s->materials.size()) s->transmission.resize(s->materials.size());
    s->transmission[material_index].rough_interface = on;
    return LPT_OK;
}

int lpt_scene_get_material_transmission_rough(const lpt_scene *s, uint32_t material_index, uint32_t *on) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_transmission_rough: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_transmission_rough: material %u of %zu", material_index, s->materials.size());
    if (on) *on = s->material_transmission(material_index).rough_interface;
    return LPT_OK;
}

// ---- volume attenuation (SPEC §28): beside the transmission table and independent of it, so factor 0 and back keeps it; sigma is derived here, once
int lpt_scene_set_material_attenuation(lpt_scene *s, uint32_t material_index, const float color[3], float distance) {
    if (!s || !color) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_attenuation: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_attenuation: material %u of %zu", material_index, s->materials.size());
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(color[c]) || color[c] < 0.f || color[c] > 1.f) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_attenuation: the colour must lie in [0, 1]");
    if (!(distance > 0.f)) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_attenuation: the distance must be > 0 (+inf: none)");
    if (s->attenuation.size() < s->materials.size()) s->attenuation.resize(s->materials.size());
    MaterialAttenuation &a = s->attenuation[material_index];
    a.distance = distance;
    for (int c = 0; c < 3; ++c) { a.color[c] = color[c]; a.sigma[c] = attenuation_sigma(color[c], distance); }
    return LPT_OK;
}

int lpt_scene_get_material_attenuation(const lpt_scene *s, uint32_t material_index, float color[3], float *distance, float sigma[3]) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_attenuation: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_attenuation: material %u of %zu", material_index, s->materials.size());
    const MaterialAttenuation a = s->material_attenuation(material_index);
    if (color) for (int c = 0; c < 3; ++c) color[c] = a.color[c];
    if (distance) *distance = a.distance;
    if (sigma) for (int c = 0; c < 3; ++c) sigma[c] = a.sigma[c];
    return LPT_OK;
}

// ---- emissive materials (SPEC §22): a third side table of `materials`, grown on the first write; Le = 0 in all channels drops the record
int lpt_scene_set_material_emission(lpt_scene *s, uint32_t material_index, const float factor[3], float strength, uint32_t image) {
    if (!s || !factor) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_emission: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_emission: material %u of %zu", material_index, s->materials.size());
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(factor[c]) || factor[c] < 0.f) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_emission: the factor must be finite and >= 0");
    if (!std::isfinite(strength) || strength < 0.f) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_emission: the strength must be finite and >= 0");
    if (image != LPT_INVALID_INDEX && image >= s->images.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_emission: image %u of %zu", image, s->images.size());
    MaterialEmission e;
    for (int c = 0; c < 3; ++c) {
        e.le[c] = factor[c] * strength;
        if (!std::isfinite(e.le[c])) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_emission: factor x strength is not finite");
    }
    e.image = image;
    if (!e.emissive()) {   // non-emissive again: the record is dropped, whatever the image says
        if (material_index < s->emission.size()) s->emission[material_index] = MaterialEmission();
        return LPT_OK;
    }
    if (s->emission.size() < s->materials.size()) s->emission.resize(s->materials.size());
    s->emission[material_index] = e;
    return LPT_OK;
}

int lpt_scene_get_material_emission(const lpt_scene *s, uint32_t material_index, float le[3], uint32_t *image) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_emission: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_emission: material %u of %zu", material_index, s->materials.size());
    const MaterialEmission e = s->material_emission(material_index);
    if (le) for (int c = 0; c < 3; ++c) le[c] = e.le[c];
    if (image) *image = e.image;
    return LPT_OK;
}

// ---- normal maps (SPEC §24): a fourth side table of `materials`, grown on the first write; LPT_INVALID_INDEX removes the map
int lpt_scene_set_material_normal_map(lpt_scene *s, uint32_t material_index, uint32_t image, float scale) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_normal_map: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_normal_map: material %u of %zu", material_index, s->materials.size());
    if (!std::isfinite(scale)) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_normal_map: the scale must be finite");
    if (image != LPT_INVALID_INDEX && image >= s->images.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_material_normal_map: image %u of %zu", image, s->images.size());
    if (image == LPT_INVALID_INDEX) {   // no map again: the record is dropped, whatever the scale says
        if (material_index < s->normal_map.size()) s->normal_map[material_index] = MaterialNormalMap();
        return LPT_OK;
    }
    if (s->normal_map.size() < s->materials.size()) s->normal_map.resize(s->materials.size());
    s->normal_map[material_index].image = image;
    s->normal_map[material_index].scale = scale;
    return LPT_OK;
}

int lpt_scene_get_material_normal_map(const lpt_scene *s, uint32_t material_index, uint32_t *image, float *scale) {
    if (!s) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_normal_map: null");
    if (material_index >= s->materials.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_material_normal_map: material %u of %zu", material_index, s->materials.size());
    const MaterialNormalMap m = s->material_normal_map(material_index);
    if (image) *image = m.image;
    if (scale) *scale = m.scale;
    return LPT_OK;
}

int lpt_scene_add_image(lpt_scene *s, const uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t *out_index) {
    if (!s || !rgba8 || !w || !h) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_image: null or empty");
    Image im;
    im.width = w; im.height = h;
    im.rgba8.assign(rgba8, rgba8 + (size_t)w * h * 4);
    s->images.push_back(std::move(im));
    if (out_index) *out_index = (uint32_t)s->images.size() - 1u;
    return LPT_OK;
}

int lpt_scene_add_light(lpt_scene *s, const lpt_light *l, uint32_t *out_index) {
    if (!s || !l) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_light: null");
    s->lights.push_back(*l);
    if (out_index) *out_index = (uint32_t)s->lights.size() - 1u;
    return LPT_OK;
}

int lpt_scene_set_light(lpt_scene *s, uint32_t i, const lpt_light *l) {
    if (!s || !l || i >= s->lights.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_light: bad index %u", i);
    s->lights[i] = *l;
    return LPT_OK;
}

// ---- punctual lights (SPEC §19) -------------------------------------------------
// the record as the scene keeps it: checked, direction normalised (zero for a point light's unused direction stays zero)
static int punctual_checked(const lpt_punctual_light *l, lpt_punctual_light &out, const char *fn) {
    const float *f = l->position;   // the four rows are contiguous: 16 floats
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(f[i])) return fail(LPT_ERR_INVALID_ARG, "%s: field %d is not finite", fn, i);
    const float type = l->position[3];
    if (!(type == 0.f || type == 1.f || type == 2.f)) return fail(LPT_ERR_INVALID_ARG, "%s: unknown type %g", fn, (double)type);
    if (l->direction[3] < 0.f) return fail(LPT_ERR_INVALID_ARG, "%s: negative range", fn);
    if (l->color[0] < 0.f || l->color[1] < 0.f || l->color[2] < 0.f) return fail(LPT_ERR_INVALID_ARG, "%s: negative colour", fn);
    if (type == 1.f && !(l->cone[1] > 0.f)) return fail(LPT_ERR_INVALID_ARG, "%s: a spot light's cone[1] = 1 / (cos(inner) - cos(outer)) must be positive", fn);
    out = *l;
    normalize3(out.direction);
    if (type != 0.f && out.direction[0] == 0.f && out.direction[1] == 0.f && out.direction[2] == 0.f)
        return fail(LPT_ERR_INVALID_ARG, "%s: a spot or directional light needs a direction", fn);
    // the neutral constants of the windows a type does not have (SPEC §19: the kernel evaluates both for every type): only a spot has a cone —
    // s = clamp((c + 2) * 1, 0, 1) = 1 for every cosine —, a directional light has no range
    if (type != 1.f) { out.cone[0] = -2.f; out.cone[1] = 1.f; }
    if (type == 2.f) out.direction[3] = 0.f;
    out.color[3] = 0.f; out.cone[2] = 0.f; out.cone[3] = 0.f;
    return LPT_OK;
}

int lpt_punctual_light_make(uint32_t type, const float *position, const float *direction, const float *color, float intensity,
                            float range, float inner_angle, float outer_angle, lpt_punctual_light *out) {
    if (!out) return fail(LPT_ERR_INVALID_ARG, "lpt_punctual_light_make: null");
    if (type > LPT_PUNCTUAL_DIRECTIONAL) return fail(LPT_ERR_INVALID_ARG, "lpt_punctual_light_make: unknown type %u", type);
    if (!std::isfinite(intensity) || intensity < 0.f) return fail(LPT_ERR_INVALID_ARG, "lpt_punctual_light_make: intensity must be finite and >= 0");
    lpt_punctual_light l;
    memset(&l, 0, sizeof l);
    for (int i = 0; i < 3; ++i) {
        l.position[i] = position ? position[i] : 0.f;
        l.direction[i] = direction ? direction[i] : (i == 2 ? -1.f : 0.f);
        l.color[i] = (color ? color[i] : 1.f) * intensity;
    }
    l.position[3] = (float)type;
    l.direction[3] = range;
    // a point or directional light passes the cone window untouched: s = clamp((c - (-2)) * 1, 0, 1) = 1 for every cosine
    l.cone[0] = -2.f;
    l.cone[1] = 1.f;
    if (type == LPT_PUNCTUAL_SPOT) {
        if (!(inner_angle >= 0.f) || !(outer_angle > inner_angle) || !(outer_angle <= 1.5707964f))
            return fail(LPT_ERR_INVALID_ARG, "lpt_punctual_light_make: cone angles must satisfy 0 <= inner < outer <= pi/2");
        const double co = std::cos((double)outer_angle), ci = std::cos((double)inner_angle);
        l.cone[0] = (float)co;
        l.cone[1] = (float)(1.0 / std::fmax(ci - co, 1e-6));
    }
    lpt_punctual_light checked;
    const int st = punctual_checked(&l, checked, "lpt_punctual_light_make");
    if (st != LPT_OK) return st;
    *out = checked;
    return LPT_OK;
}

int lpt_scene_add_punctual_light(lpt_scene *s, const lpt_punctual_light *l, uint32_t *out_index) {
    if (!s || !l) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_add_punctual_light: null");
    lpt_punctual_light c;
    const int st = punctual_checked(l, c, "lpt_scene_add_punctual_light");
    if (st != LPT_OK) return st;
    s->punctual.push_back(c);
    if (out_index) *out_index = (uint32_t)s->punctual.size() - 1u;
    return LPT_OK;
}

int lpt_scene_set_punctual_light(lpt_scene *s, uint32_t i, const lpt_punctual_light *l) {
    if (!s || !l || i >= s->punctual.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_set_punctual_light: bad index %u", i);
    lpt_punctual_light c;
    const int st = punctual_checked(l, c, "lpt_scene_set_punctual_light");
    if (st != LPT_OK) return st;
    s->punctual[i] = c;
    return LPT_OK;
}

int lpt_scene_punctual_count(const lpt_scene *s, uint32_t *out) {
    if (!s || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_punctual_count: null");
    *out = (uint32_t)s->punctual.size();
    return LPT_OK;
}

#define LPT_GETTER(NAME, TYPE, FIELD)                                                            \
    int NAME(const lpt_scene *s, uint32_t first, uint32_t count, TYPE *dst) {                    \
        if (!s || (!dst && count)) return fail(LPT_ERR_INVALID_ARG, #NAME ": null");             \
        if ((size_t)first + count > s->FIELD.size())                                             \
            return fail(LPT_ERR_INVALID_ARG, #NAME ": range [%u,%u) exceeds %zu", first, first + count, s->FIELD.size()); \
        if (count) memcpy(dst, s->FIELD.data() + first, sizeof(TYPE) * (size_t)count);           \
        return LPT_OK;                                                                           \
    }
LPT_GETTER(lpt_scene_get_materials, lpt_material, materials)
LPT_GETTER(lpt_scene_get_entries, lpt_blas_entry, entries)
LPT_GETTER(lpt_scene_get_vertices, lpt_vertex, vertices)
LPT_GETTER(lpt_scene_get_indices, uint32_t, indices)
LPT_GETTER(lpt_scene_get_instances, lpt_instance, instances)
LPT_GETTER(lpt_scene_get_lights, lpt_light, lights)
LPT_GETTER(lpt_scene_get_punctual_lights, lpt_punctual_light, punctual)

int lpt_scene_get_image(const lpt_scene *s, uint32_t index, uint32_t *w, uint32_t *h, uint8_t *dst) {
    if (!s || index >= s->images.size()) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_get_image: bad index %u", index);
    const Image &im = s->images[index];
    if (w) *w = im.width;
    if (h) *h = im.height;
    if (dst) memcpy(dst, im.rgba8.data(), im.rgba8.size());
    return LPT_OK;
}

}  // extern "C"
