// material_tables.h — the per-triangle material side tables (SPEC §20 alpha masks, §21 transmission, §22 emission, §24 normal maps) as ONE derivation.
// Every kind is the same pair of host vectors: one 16-byte record per material of the kind that an instance with triangles uses, and one uint32 per baked triangle
// (keyed by prim id, so a refit leaves it alone): 0 = the triangle's material is not of the kind, else 1 + its record.  Both are empty for a scene that does not use
// the kind, which then launches what it always launched.  What differs between the kinds is one row of kMaterialKinds.
// Plain C++, no HIP: device.hip uploads what is derived here, tests/tools/material_tables_check.cpp drives it on a CPU (tests/test_material_tables.py).
#pragma once
#include <algorithm>
#include <initializer_list>

#include "common.h"

namespace lpt {

struct MaterialRec { float x, y, z, w; };   // device.hip uploads these as float4
static_assert(sizeof(MaterialRec) == 16, "a material record is one float4");
// `more`: a second record per entry of `recs`, parallel to it, for a kind that has one (SPEC §28: the transmission table's sigma rows); empty where no record needs it
struct MaterialTable { std::vector<MaterialRec> recs; std::vector<uint32_t> tri; std::vector<MaterialRec> more; };

static inline float bits_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }   // an index rides in a record as its bit pattern

// One row per kind: does material `mat` (< scene.materials.size()) have the feature, and if so its record and the plain image the record names (LPT_INVALID_INDEX:
// none).  That image is looked up on its own, never through the paired copy, so it must be resident on its own (plain_image_residency, derive_material_tables).
struct MaterialKind {
    int section;   // of SPEC.md
    bool (*state)(const lpt_scene &scene, uint32_t mat, MaterialRec &rec, uint32_t &plain_image);
    const char *names;   // "material %u now <names> was uploaded only as half of a pair"
    bool (*more)(const lpt_scene &scene, uint32_t mat, MaterialRec &row) = nullptr;   // the second record of a material that has the feature; false: it needs none (a zero row stands in)
};
enum { MAT_ALPHA = 0, MAT_TRANS, MAT_EMIS, MAT_NMAP, MAT_KINDS };

static inline bool alpha_state(const lpt_scene &scene, uint32_t mat, MaterialRec &rec, uint32_t &plain_image) {
    const MaterialAlpha a = scene.material_alpha(mat);
    if (a.mode != LPT_ALPHA_MASK && a.mode != LPT_ALPHA_BLEND) return false;
    plain_image = a.image < scene.images.size() ? a.image : LPT_INVALID_INDEX;
    // the fourth float is the mode alpha_rejects branches on: 0 masked (a >= cutoff, SPEC §20), 1 blended (a > xi, SPEC §26)
    rec = MaterialRec{a.cutoff, scene.materials[mat].color[3], bits_as_float(plain_image), a.mode == LPT_ALPHA_BLEND ? 1.0f : 0.0f};
    return true;
}
// SPEC §28: the sigma row {sigma_r, sigma_g, sigma_b, 0} of a material that is transmissive, solid and has some sigma_c > 0; the record's fourth float says so
static inline bool trans_sigma(const lpt_scene &scene, uint32_t mat, MaterialRec &row) {
    const MaterialTransmission t = scene.material_transmission(mat);
    const MaterialAttenuation a = scene.material_attenuation(mat);
    row = MaterialRec{0.0f, 0.0f, 0.0f, 0.0f};
    if (!(t.factor > 0.0f) || t.thin_walled || !a.attenuates()) return false;
    row = MaterialRec{a.sigma[0], a.sigma[1], a.sigma[2], 0.0f};
    return true;
}
static inline bool trans_state(const lpt_scene &scene, uint32_t mat, MaterialRec &rec, uint32_t &plain_image) {
    const MaterialTransmission t = scene.material_transmission(mat);
    if (!(t.factor > 0.0f)) return false;
    plain_image = LPT_INVALID_INDEX;
    MaterialRec sigma;
    // SPEC §29: the rough bit is the SIGN of `thin` (-0 solid, -1 thin-walled), so a non-rough record keeps its bits and every reader that tests `thin` against
    // 0 (shade_hit, §27's glass_shadow_eval) reads what it read
    const float thin = t.thin_walled ? 1.0f : 0.0f;
    rec = MaterialRec{t.factor, t.ior, t.rough_interface ? -thin : thin, trans_sigma(scene, mat, sigma) ? 1.0f : 0.0f};
    return true;
}
static inline bool emis_state(const lpt_scene &scene, uint32_t mat, MaterialRec &rec, uint32_t &plain_image) {
    const MaterialEmission e = scene.material_emission(mat);
    if (!e.emissive()) return false;
    plain_image = e.image < scene.images.size() ? e.image : LPT_INVALID_INDEX;
    rec = MaterialRec{e.le[0], e.le[1], e.le[2], bits_as_float(plain_image)};
    return true;
}
static inline bool nmap_state(const lpt_scene &scene, uint32_t mat, MaterialRec &rec, uint32_t &plain_image) {
    const MaterialNormalMap m = scene.material_normal_map(mat);
    if (!(m.image < scene.images.size())) return false;   // no image, no normal map
    plain_image = m.image;
    rec = MaterialRec{bits_as_float(plain_image), m.scale, 0.0f, 0.0f};
    return true;
}
static const MaterialKind kMaterialKinds[MAT_KINDS] = {
    {20, alpha_state, "masks with an image that"},
    {21, trans_state, "", trans_sigma},   // names no image
    {22, emis_state, "emits with an image that"},
    {24, nmap_state, "has a normal map whose image"},
};

// The tables of the scene as it is now, from the baked instance layout (inst_first / inst_count: every instance's run of baked triangles) and the images the atlas
// holds on their own.  Returns the first error in the order of the kinds; nothing is touched on a device, so a caller can check an edit before it bakes anything.
static inline int derive_material_tables(const lpt_scene &scene, const std::vector<uint32_t> &inst_first, const std::vector<uint32_t> &inst_count, uint32_t n_tris,
                                         const std::vector<uint8_t> &image_resident, MaterialTable (&out)[MAT_KINDS]) {
    for (int k = 0; k < MAT_KINDS; ++k) {
        MaterialTable &t = out[k];
        t = MaterialTable();
        std::vector<uint32_t> rec_of(scene.materials.size(), 0u);   // 1 + record index
        bool any_more = false;
        for (size_t i = 0; i < scene.instances.size() && i < inst_count.size(); ++i) {
            const uint32_t n = inst_count[i];
            if (!n) continue;
            const uint32_t mat = scene.instances[i].material_index < scene.materials.size() ? scene.instances[i].material_index : 0u;   // SPEC §2.5
            MaterialRec rec;
            uint32_t image;
            if (!kMaterialKinds[k].state(scene, mat, rec, image)) continue;
            if (!rec_of[mat]) {
                if (image != LPT_INVALID_INDEX && !(image < image_resident.size() && image_resident[image]))
                    return fail(LPT_ERR_INVALID_ARG, "material %u now %s was uploaded only as half of an (albedo, mra) pair: upload the scene again", mat, kMaterialKinds[k].names);
                t.recs.push_back(rec);
                if (kMaterialKinds[k].more) {
                    MaterialRec row;
                    if (kMaterialKinds[k].more(scene, mat, row)) any_more = true;
                    t.more.push_back(row);
                }
                rec_of[mat] = (uint32_t)t.recs.size();
            }
            if (t.tri.empty()) t.tri.assign(std::max(n_tris, 1u), 0u);
            if ((size_t)inst_first[i] + n > t.tri.size()) return fail(LPT_ERR_INVALID_ARG, "instance %zu lies beyond the baked triangles", i);
            std::fill(t.tri.begin() + inst_first[i], t.tri.begin() + inst_first[i] + n, rec_of[mat]);
        }
        if (!any_more) t.more.clear();
    }
    return LPT_OK;
}

// SPEC §27: how many baked triangles are thin-walled transmissive panes, from the transmission table as derived above (its record's third float is `thin`)
static inline uint32_t thin_glass_triangles(const MaterialTable &trans) {
    uint32_t n = 0;
    for (uint32_t e : trans.tri)
        if (e != 0u && trans.recs[e - 1u].z != 0.0f) n++;
    return n;
}

// Which images the tiled atlas holds on their own, given which materials' (albedo, mra) textures were stored as a pair: an image that only ever appears as half of
// a pair is not stored a second time.  An image no material references is kept (a later material edit may start to sample it), and so is every image a side-table
// record names, whatever pair it is also half of: the alpha lookup of the traversal, shade_hit<.., EMIS> and normal_map read the plain tiled image.
static inline std::vector<uint8_t> plain_image_residency(const lpt_scene &scene, const std::vector<uint8_t> &material_paired) {
    const size_t n = scene.images.size();
    std::vector<uint8_t> referenced(n, 0), alone(n, 0), resident(n, 1);
    for (size_t i = 0; i < scene.materials.size(); ++i) {
        const lpt_material &m = scene.materials[i];
        for (uint32_t id : {m.albedo_texture, m.mra_texture})
            if (id < n) { referenced[id] = 1; if (!material_paired[i]) alone[id] = 1; }
        for (const MaterialKind &kind : kMaterialKinds) {
            MaterialRec rec;
            uint32_t image;
            if (kind.state(scene, (uint32_t)i, rec, image) && image != LPT_INVALID_INDEX) { referenced[image] = 1; alone[image] = 1; }
        }
    }
    for (size_t i = 0; i < n; ++i) resident[i] = (!referenced[i] || alone[i]) ? 1 : 0;
    return resident;
}

}  // namespace lpt
