// common.h — internal declarations shared by the host-side translation units of
// libloupiote_hip.so.  Nothing here is part of the ABI (include/lpt.h is).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lpt.h"

namespace lpt {

// thread-local error text behind lpt_last_error()
void set_error(const char *fmt, ...);
int fail(int status, const char *fmt, ...);

struct Image {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> rgba8;
    bool has_alpha = false;   // the file carried an alpha channel that rgba8's fourth byte holds (decode_png; SPEC §20: only then a MASK material reads it)
};

// SPEC §20, §26: a material's alpha state (the 32-byte lpt_material keeps the reference's layout, so this rides beside it)
struct MaterialAlpha {
    uint32_t mode = LPT_ALPHA_OPAQUE;   // LPT_ALPHA_OPAQUE / _MASK / _BLEND (blended: the cutoff is not read)
    float cutoff = 0.5f;
    uint32_t image = LPT_INVALID_INDEX;
};

// SPEC §21: a material's transmission state, a second side table; factor 0 = opaque (the default)
struct MaterialTransmission {
    float factor = 0.0f;
    float ior = 1.5f;
    uint32_t thin_walled = 1u;
    uint32_t rough_interface = 0u;   // SPEC §29: the interface event is the microfacet one; set and kept apart from the three above (factor 0 and back keeps it)
};

// SPEC §28: a material's volume attenuation, kept beside its transmission state and independent of it; sigma is derived once, here on the host
struct MaterialAttenuation {
    float color[3] = {1.0f, 1.0f, 1.0f};
    float distance = INFINITY;
    float sigma[3] = {0.0f, 0.0f, 0.0f};   // attenuation_sigma per channel: finite, >= +0
    bool attenuates() const { return sigma[0] > 0.0f || sigma[1] > 0.0f || sigma[2] > 0.0f; }
};
// sigma_c = 0 if c == 1 or D == +inf, else min((float)(-log((double)c) / (double)D), FLT_MAX): c = 0 and an overflowing quotient both give FLT_MAX
inline float attenuation_sigma(float c, float distance) {
    if (c == 1.0f || std::isinf(distance)) return 0.0f;
    const float s = (float)(-std::log((double)c) / (double)distance);
    return s < FLT_MAX ? s : FLT_MAX;
}

// SPEC §22: a material's emission, a third side table; Le = 0 in all channels = non-emissive (the default, and no record is kept)
struct MaterialEmission {
    float le[3] = {0.0f, 0.0f, 0.0f};       // float32(factor_c) * float32(strength), one binary32 product per channel
    uint32_t image = LPT_INVALID_INDEX;     // the emissive image (sRGB), or none
    bool emissive() const { return le[0] != 0.0f || le[1] != 0.0f || le[2] != 0.0f; }
};

// SPEC §24: a material's normal map, a fourth side table; no image = no normal map (the default)
struct MaterialNormalMap {
    uint32_t image = LPT_INVALID_INDEX;     // the normal image (linear rgb), or none
    float scale = 1.0f;                     // glTF normalTexture.scale: multiplies the texel's x and y
};

}  // namespace lpt

// The CPU-side scene: the flat arrays of the reference's Scene / BLASArray
// (reference crates/lib/src/scene.rs:30-54).
struct lpt_scene {
    std::vector<lpt_material> materials;
    std::vector<lpt_blas_entry> entries;
    std::vector<lpt_vertex> vertices;
    std::vector<uint32_t> indices;
    std::vector<lpt_instance> instances;
    std::vector<lpt_light> lights;
    std::vector<lpt::Image> images;
    std::vector<lpt_punctual_light> punctual;   // SPEC §19: point / spot / directional lights; no dummy element, a fresh scene has none
    std::vector<lpt::MaterialAlpha> alpha;      // SPEC §20: side table of `materials`; a material beyond its end is opaque (material_alpha)
    lpt::MaterialAlpha material_alpha(size_t i) const { return i < alpha.size() ? alpha[i] : lpt::MaterialAlpha(); }
    std::vector<lpt::MaterialTransmission> transmission;   // SPEC §21: side table of `materials`; a material beyond its end is opaque (material_transmission)
    lpt::MaterialTransmission material_transmission(size_t i) const { return i < transmission.size() ? transmission[i] : lpt::MaterialTransmission(); }
    std::vector<lpt::MaterialAttenuation> attenuation;   // SPEC §28: side table of `materials`; a material beyond its end does not attenuate (material_attenuation)
    lpt::MaterialAttenuation material_attenuation(size_t i) const { return i < attenuation.size() ? attenuation[i] : lpt::MaterialAttenuation(); }
    std::vector<lpt::MaterialEmission> emission;   // SPEC §22: side table of `materials`; a material beyond its end is non-emissive (material_emission)
    lpt::MaterialEmission material_emission(size_t i) const { return i < emission.size() ? emission[i] : lpt::MaterialEmission(); }
    std::vector<lpt::MaterialNormalMap> normal_map;   // SPEC §24: side table of `materials`; a material beyond its end has no normal map (material_normal_map)
    lpt::MaterialNormalMap material_normal_map(size_t i) const { return i < normal_map.size() ? normal_map[i] : lpt::MaterialNormalMap(); }
};

namespace lpt {

// ---- baked, device-ready acceleration data (host copies) -------------------
// 64 B compressed 8-wide node: FOUR 16-byte loads per visit (round 6: a load instruction of a visit is worth ~80 VALU instructions, and the fifth row of the
// 80-byte node cost 12 % of the traversal — profiles/r06_experiments_ab.txt).  What made room:
//  * the origin is a point of a 65536^3 SCENE GRID (Accel::grid_lo / grid_step, power-of-two steps): p = grid_lo + o * grid_step, at or below the node's box
//    minimum; the quantisation steps (ex, ey, ez) cover the node's box from THERE.  The grid spans 1.5 x the scene, so a node is at most 1 / 43 690 of the scene
//    looser than with an fp32 origin (conservative either way: the children are quantised against the origin the node really stores);
//  * no triangle base: the triangles of node i's leaf children have FIXED places, 16 * i + 2 * slot + k (k = 0, 1: a leaf child carries one or two triangles),
//    in woop / leaf_prim arrays of 16 entries per node (unused places are holes: zero Woop rows, LPT_INVALID_INDEX);
//  * leaf masks instead of a byte per slot: bit s of leaf1 = slot s is a leaf child, of leaf2 = ... with two triangles; in neither mask nor imask = empty (inverted box).
struct alignas(16) Node8 {
    uint16_t ox, oy, oz;         // origin on the scene grid
    uint8_t ex, ey, ez;          // biased power-of-two quantisation step per axis
    uint8_t imask, leaf1, leaf2; // bit s: slot s is an inner node / a leaf child / a leaf child with two triangles
    uint32_t child_base;         // index of the first inner child (inner children are contiguous, in slot order)
    uint8_t qlox[8], qloy[8], qloz[8], qhix[8], qhiy[8], qhiz[8];
};
static_assert(sizeof(Node8) == 64, "Node8 must be 64 bytes");
constexpr uint32_t kNodeTris = 16;   // triangle places per node

// The scene grid of the node origins: per axis a power-of-two step with 65535 steps >= 1.5 x the extent, the scene centred in it (a refit may move things by a quarter
// of the scene before the grid has to change; it is recomputed with every refit anyway).  Shared by the host builder and the device paths (device.hip).
inline void scene_grid(const float lo[3], const float hi[3], float grid_lo[3], float grid_step[3]) {
    for (int a = 0; a < 3; ++a) {
        const double m = std::fmax(std::fabs((double)lo[a]), std::fabs((double)hi[a]));
        // never narrower than 1e-4 of the largest |coordinate|: the slack around the scene (a quarter of this) must exceed the triangle padding (6e-6 of that coordinate,
        // bvh.cpp padded_box) even for a scene that is a speck far from the origin — a node's padded box must not reach below the grid
        const double ext = std::fmax((double)hi[a] - (double)lo[a], std::fmax(m * 1e-4, 1e-30));
        int k;
        std::frexp(1.5 * ext / 65535.0, &k);                    // 1.5 ext / 65535 = f * 2^k, f in [0.5, 1)  =>  2^k is above it
        k = k < -120 ? -120 : (k > 100 ? 100 : k);
        const double step = std::ldexp(1.0, k);
        const double slack = 0.5 * (65535.0 * step - ext);
        grid_step[a] = (float)step;
        grid_lo[a] = (float)(std::floor(((double)lo[a] - slack) / step) * step);
    }
}
// the grid point at or below `v` (what a node stores) and its coordinate (what every consumer of the node computes: ONE fp32 fma, kernels.h node_origin)
inline uint16_t grid_snap(float v, float grid_lo, float grid_step, float &p) {
    double u = std::floor(((double)v - (double)grid_lo) / (double)grid_step);
    u = u < 0.0 ? 0.0 : (u > 65535.0 ? 65535.0 : u);
    uint32_t ui = (uint32_t)u;
    p = std::fmaf((float)ui, grid_step, grid_lo);
    while (p > v && ui > 0u) { --ui; p = std::fmaf((float)ui, grid_step, grid_lo); }
    return (uint16_t)ui;
}

struct alignas(16) WoopTri {  // 48 B world -> unit-triangle affine map
    float r0[4], r1[4], r2[4];
};
static_assert(sizeof(WoopTri) == 48, "WoopTri must be 48 bytes");

struct Accel {
    std::vector<lpt_vertex> tri_verts;   // 3 per baked triangle (world space)
    std::vector<uint32_t> tri_material;  // per baked triangle
    std::vector<Node8> nodes;            // node 0 = root
    std::vector<WoopTri> woop;           // kNodeTris places per node (Node8); holes are zero
    std::vector<uint32_t> leaf_prim;     // triangle place -> baked triangle id (holes: LPT_INVALID_INDEX)
    float grid_lo[3] = {0.f, 0.f, 0.f}, grid_step[3] = {1.f, 1.f, 1.f};   // the scene grid of the node origins (scene_grid)
    uint32_t max_depth = 0;
    float build_ms = 0.f;
    float max_abs = 0.f;                 // the largest |coordinate| of any baked vertex: what the scene-wide part of the triangle padding follows (bvh.cpp padded_box)
    // bookkeeping for refits (lpt_scene_gpu_update_instances)
    std::vector<uint32_t> inst_first, inst_count;  // per scene instance: its run of baked triangles
    std::vector<uint32_t> level_start;             // nodes are stored breadth first: level l = [level_start[l], level_start[l+1])
};

constexpr float kScenePad = 2e-6f;   // triangle padding per unit of the scene's largest |coordinate| (host builder, LBVH and refit alike)

// bvh.cpp
int bake_and_build(const lpt_scene &scene, Accel &out);
uint32_t bake_instance(const lpt_scene &scene, size_t instance, std::vector<lpt_vertex> &verts);   // SPEC §2.5: one instance's world-space triangles appended, 3 vertices each; returns its material
bool bake_mirrored(const float model_to_world[16]);   // SPEC §2.5: the binary32 determinant of the 3x3 part is negative: the bake exchanges vertices 1 and 2 and negates cof·N
void woop_from_triangle(const float p0[3], const float p1[3], const float p2[3], WoopTri &w);

// png.cpp
bool decode_png(const uint8_t *data, size_t size, Image &out);

// jpeg.cpp
bool decode_jpeg(const uint8_t *data, size_t size, Image &out);

// hdr.cpp
bool decode_hdr(const uint8_t *data, size_t size, uint32_t &width, uint32_t &height, std::vector<uint8_t> &rgbe);

}  // namespace lpt
