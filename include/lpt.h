/*
 * lpt.h — C ABI of the MI355X-native path-tracing core that sits behind
 * Loupiote's `crates/lib` API (crate `loupiote-core`).
 *
 * The reference has no FFI layer: its public Rust API *is* the boundary
 * (reference crates/lib/src/lib.rs:1-11).  Every entry point below replaces one
 * public Rust item; the citation after "replaces:" names it (paths relative to
 * the reference root).  A Rust shim that keeps the `Renderer/Scene/SceneGPU/
 * ProbeGPU/Device/loaders` signatures and forwards to these symbols is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - every function returns an `int` status (LPT_OK == 0); nothing unwinds
 *     across the boundary.  `lpt_last_error()` gives a thread-local message.
 *   - `create/upload` return a handle the caller destroys; input pointers are
 *     borrowed for the duration of the call only (the reference's
 *     `new_storage_with_data` / `write_texture` copy semantics,
 *     crates/lib/src/scene.rs:134-146, crates/lib/src/renderer.rs:646-660).
 *   - handles are not thread-safe; one caller thread per lpt_device (the
 *     reference drives everything from the winit thread,
 *     crates/standalone/src/app.rs:259-344).
 *   - matrices are 16 floats, column-major (glam::Mat4::to_cols_array()).
 *   - plain pointers and sizes only; no torch / HIP types in any signature.
 */
#ifndef LPT_H
#define LPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPT_ABI_VERSION 6u

/* replaces: albedo_rtx::uniforms::INVALID_INDEX (crates/lib/src/loaders/gltf.rs:120,124) */
#define LPT_INVALID_INDEX 0xFFFFFFFFu

/* ---- status codes ---------------------------------------------------------
 * replaces: enum Error { FileNotFound, TextureToBufferReadFail, AccelBuild }
 * (crates/lib/src/errors.rs:2-6) plus the conditions the reference panics on. */
enum {
    LPT_OK = 0,
    LPT_ERR_FILE_NOT_FOUND = 1, /* Error::FileNotFound(String)          */
    LPT_ERR_READBACK = 2,       /* Error::TextureToBufferReadFail       */
    LPT_ERR_ACCEL_BUILD = 3,    /* Error::AccelBuild(String)            */
    LPT_ERR_HIP = 4,            /* a HIP runtime call failed / no GPU   */
    LPT_ERR_RCCL = 5,           /* an RCCL call of the frame exchange failed */
    LPT_ERR_INVALID_ARG = 6
};

const char *lpt_last_error(void);
/* String form of a status, same text as `impl From<Error> for String`
 * (crates/lib/src/errors.rs:8-20) for the three reference variants. */
const char *lpt_status_string(int status);
uint32_t lpt_abi_version(void);

/* ---- plain-data structs ---------------------------------------------------- */

/* replaces: albedo_rtx::uniforms::Material — exactly the five fields the
 * reference writes (crates/lib/src/loaders/gltf.rs:113-126,
 * crates/lib/src/loaders/binary.rs:63-69).  32 bytes. */
typedef struct lpt_material {
    float color[4];          /* baseColorFactor                        */
    float roughness;         /* roughnessFactor                        */
    float reflectivity;      /* metallicFactor                         */
    uint32_t albedo_texture; /* image index or LPT_INVALID_INDEX       */
    uint32_t mra_texture;    /* image index or LPT_INVALID_INDEX       */
} lpt_material;

/* replaces: albedo_rtx::uniforms::Vertex { position:[f32;4], normal:[f32;4] }
 * (crates/lib/src/loaders/binary.rs:20-28).  uv rides in the two .w lanes. */
typedef struct lpt_vertex {
    float position[4]; /* x y z, u */
    float normal[4];   /* x y z, v */
} lpt_vertex;

/* replaces: albedo_rtx::uniforms::Light (crates/lib/src/scene.rs:33,50).
 * One-sided rectangular emitter.  64 bytes. */
typedef struct lpt_light {
    float normal[4];    /* xyz unit normal (emitting side), w unused        */
    float tangent[4];   /* xyz unit tangent,   w = half width               */
    float bitangent[4]; /* xyz unit bitangent, w = half height              */
    float origin[4];    /* xyz centre,         w = radiance (white)         */
} lpt_light;

/* new (SPEC.md §19; no reference counterpart: the reference's Scene carries rectangle lights only, crates/lib/src/scene.rs:33):
 * a punctual (delta) light as glTF's KHR_lights_punctual describes it.  64 bytes, four float[4] rows.  Fill it with
 * lpt_punctual_light_make: `cone` is derived data. */
#define LPT_PUNCTUAL_POINT 0u
#define LPT_PUNCTUAL_SPOT 1u
#define LPT_PUNCTUAL_DIRECTIONAL 2u
typedef struct lpt_punctual_light {
    float position[4];  /* xyz world position (point, spot); w = type: 0 point, 1 spot, 2 directional, as a float   */
    float direction[4]; /* xyz unit direction the light shines ALONG (spot, directional); w = range, 0 = unlimited    */
    float color[4];     /* rgb = colour x intensity (candela for point / spot, lux for directional); w unused, 0      */
    float cone[4];      /* x = cos(outer), y = 1 / max(cos(inner) - cos(outer), 1e-6); z, w unused, 0                */
} lpt_punctual_light;

/* replaces: albedo_rtx::uniforms::Instance as built by BLASArray::add_instance
 * (crates/lib/src/loaders/gltf.rs:141-145) and edited by Instance::set_transform
 * (crates/standalone/src/lib.rs:117-121). */
typedef struct lpt_instance {
    float model_to_world[16];
    uint32_t blas_index;
    uint32_t material_index;
    uint32_t pad[2];
} lpt_instance;

/* replaces: one BLASArray.entries element (crates/lib/src/scene.rs:43-49). */
typedef struct lpt_blas_entry {
    uint32_t vertex_offset; /* first vertex in Scene.vertices          */
    uint32_t vertex_count;
    uint32_t index_offset;  /* first index in the scene index pool     */
    uint32_t index_count;   /* 3 * triangle count                      */
} lpt_blas_entry;

typedef struct lpt_scene_counts {
    uint32_t materials, entries, vertices, indices, instances, lights, images;
} lpt_scene_counts;

typedef struct lpt_accel_stats {
    uint32_t triangles;  /* baked world-space triangles                 */
    uint32_t nodes;      /* wide-BVH nodes                              */
    uint32_t node_bytes; /* bytes per node                              */
    uint32_t tri_bytes;  /* bytes per pre-transformed triangle          */
    uint32_t max_depth;
    float build_ms;
    uint32_t host_baked_triangles; /* triangles transformed to world space on the HOST by the last upload (0 for
                                      LPT_ACCEL_BUILD_GPU_LBVH: instances are baked by k_bake_instance on the device) */
    float upload_ms;               /* wall time of the whole lpt_scene_upload(_ex) call: bake + build + copies */
    /* ABI 5: texel bytes this scene keeps in device memory — the tiled atlas (every image some material samples on its own, or none
     * references) + the paired (albedo, mra) texels of the materials whose two textures have one size; an image that only ever
     * appears as half of a pair is stored once, in the pair (the reference keeps each image once: scene.rs:172-184) */
    uint32_t texture_pairs;
    uint64_t texture_bytes_resident;
} lpt_accel_stats;

/* result of a closest-hit query (the build's `Intersection`, 16 bytes) */
typedef struct lpt_hit {
    float t, u, v;
    uint32_t prim; /* baked triangle id, 0x80000000|light for an emitter, LPT_INVALID_INDEX on miss */
} lpt_hit;

typedef struct lpt_ray_counts {
    uint64_t closest; /* closest-hit rays traced since the last reset */
    uint64_t shadow;  /* shadow (any-hit) rays traced                 */
    uint64_t shaded;  /* surface hits shaded                          */
    uint64_t nodes;   /* closest-hit kernel: BVH nodes visited (stats enabled only) */
    uint64_t tris;    /* closest-hit kernel: triangles tested  (stats enabled only) */
    uint64_t shadow_nodes; /* shadow kernel: nodes visited (stats enabled only)     */
    uint64_t shadow_tris;  /* shadow kernel: triangles tested (stats enabled only)  */
    /* closest-hit kernel, stats enabled only: wave utilisation of the persistent traversal loop */
    uint64_t wave_steps;   /* loop iterations summed over waves                        */
    uint64_t live_lanes;   /* lanes carrying a ray, summed over those iterations        */
    uint64_t node_lanes;   /* lanes that entered the node test                         */
    uint64_t tri_lanes;    /* lanes that ran a triangle test                           */
    /* ABI 4: bounce 0 is traced by packet traversal (one tree walk per 64 coherent rays): these rays are part of `closest`, their
     * node / triangle fetches are NOT part of `nodes` / `tris` */
    uint64_t primary;      /* closest-hit rays traced as packets                               */
    uint64_t packet_nodes; /* nodes entered, once per PACKET (stats enabled only)              */
    uint64_t packet_tris;  /* triangles fetched, once per PACKET (stats enabled only)          */
    /* ABI 5, stats enabled only, per-bounce launches only: the shadow rays that found an occluder, and the occluder-cache PROBE — what a
     * table of the last occluding triangle per cell of a grid over the shadow rays' origins (LPT_EXP_OCC_CELL_MILLI) would have answered
     * at each ray's start: entries found, and entries whose triangle occludes the ray (a hit would end that ray after one triangle test).
     * A measurement; no kernel uses such a cache. */
    uint64_t shadow_occluded;
    uint64_t occluder_cache_found;
    uint64_t occluder_cache_hits;
    /* ABI 6: rays of the per-bounce traversal launches that a WHOLE WAVE finished: handed over by the step budget (k_trace_coop re-traces them) or finished in
     * place at the tail of a launch (LPT_OPT_TAIL_LANES).  Which rays these are depends on scheduling; the frame does not.  Lets a test see that the path ran. */
    uint64_t wave_rays;
} lpt_ray_counts;

typedef struct lpt_timing {
    char label[32]; /* "ray generation", "intersection", "shading", "shadow", "accumulation", "asvgf", "exchange", "primary intersection", "path" */
    float ms;       /* summed over every raytrace() since enable_timings(1) */
    uint32_t launches;
} lpt_timing;

/* replaces: enum BlitMode (crates/lib/src/renderer.rs:160-167; spelling of
 * `Pahtrace` is the reference's). */
enum {
    LPT_BLIT_PATHTRACE = 0,
    LPT_BLIT_DENOISED = 1,
    LPT_BLIT_TEMPORAL = 2,
    LPT_BLIT_GBUFFER = 3,
    LPT_BLIT_MOTION = 4
};

typedef struct lpt_device lpt_device;
typedef struct lpt_scene lpt_scene;
typedef struct lpt_scene_gpu lpt_scene_gpu;
typedef struct lpt_probe lpt_probe;
typedef struct lpt_renderer lpt_renderer;
typedef struct lpt_comm lpt_comm;

/* ---- Device ---------------------------------------------------------------
 * replaces: Device::new(wgpu::Device) (crates/lib/src/device.rs:80).  One
 * process drives one GPU; `hip_ordinal` picks it.  Fails with LPT_ERR_HIP when
 * no gfx950 device is visible — there is no CPU fallback. */
int lpt_device_create(int hip_ordinal, lpt_device **out);
int lpt_device_destroy(lpt_device *dev);
int lpt_device_synchronize(lpt_device *dev);
/* name, CU count and the HIP stream handle (void*: a hipStream_t) the renderer
 * enqueues on — bench.py brackets that stream with HIP events. */
int lpt_device_info(lpt_device *dev, char *name, size_t name_cap, int *compute_units);
int lpt_device_stream(lpt_device *dev, void **hip_stream);

/* ---- Scene (CPU side) -----------------------------------------------------
 * replaces: Scene::default() and its pub fields (crates/lib/src/scene.rs:30-54).
 * As in the reference, a fresh scene holds ONE dummy element in every array
 * (material 0, BLAS entry 0, vertex 0, instance 0, light 0 = Light::new()), so
 * loaded content starts at index 1 (crates/standalone/src/lib.rs:117). */
int lpt_scene_create(lpt_scene **out);
int lpt_scene_destroy(lpt_scene *scene);
int lpt_scene_counts_get(const lpt_scene *scene, lpt_scene_counts *out);

/* replaces: BLASArray::add_bvh(MeshDescriptor) / add_bvh_indexed(IndexedMeshDescriptor)
 * (crates/lib/src/loaders/gltf.rs:91-105).  Strides are in BYTES (pas::Slice);
 * positions may be vec3 or vec4 (only xyz read); normals / uvs / indices may be
 * NULL.  Without indices, vertices are consumed three at a time.  Missing
 * normals become flat face normals (crates/lib/src/loaders/binary.rs:31-49).
 * LPT_ERR_ACCEL_BUILD on an out-of-range index or a count that is not a
 * multiple of three.  Texture coordinates must be finite and at most LPT_UV_MAX
 * in magnitude (SPEC.md §9: beyond it u x width is not a binary32 number and the
 * filter weights would be NaN): LPT_ERR_INVALID_ARG otherwise, and the scene is
 * unchanged. */
#define LPT_UV_MAX 7.9228162514264338e28f /* 2^96 */
int lpt_scene_add_mesh(lpt_scene *scene, const void *positions, size_t position_stride,
                       const void *normals, size_t normal_stride, const void *uvs,
                       size_t uv_stride, uint32_t vertex_count, const uint32_t *indices,
                       uint32_t index_count, uint32_t *out_blas_index);
/* replaces: BLASArray::add_instance(blas, model_to_world, material)
 * (crates/lib/src/loaders/gltf.rs:141-145). */
int lpt_scene_add_instance(lpt_scene *scene, uint32_t blas_index, const float model_to_world[16],
                           uint32_t material_index, uint32_t *out_instance_index);
/* replaces: Instance::set_transform (crates/standalone/src/lib.rs:118-121). */
int lpt_scene_set_instance_transform(lpt_scene *scene, uint32_t instance_index,
                                     const float model_to_world[16]);
/* replaces: scene.materials.push(..) (crates/lib/src/loaders/gltf.rs:113) */
int lpt_scene_add_material(lpt_scene *scene, const lpt_material *m, uint32_t *out_index);
/* replaces: scene.images.push(ImageData::new(rgba8,w,h)) (gltf.rs:150-153) */
int lpt_scene_add_image(lpt_scene *scene, const uint8_t *rgba8, uint32_t width, uint32_t height,
                        uint32_t *out_index);
/* replaces: pub lights: Vec<Light> (crates/lib/src/scene.rs:33) */
int lpt_scene_add_light(lpt_scene *scene, const lpt_light *l, uint32_t *out_index);
int lpt_scene_set_light(lpt_scene *scene, uint32_t index, const lpt_light *l);
/* replaces: Light::new() (crates/lib/src/scene.rs:50) */
int lpt_light_default(lpt_light *out);

/* build-only extension (SPEC.md §19; the reference has no punctual lights): the scene's point / spot / directional lights.
 * Unlike every other scene array there is NO dummy element 0: a fresh scene has none, and a scene without any renders
 * exactly what it rendered before they existed.  `direction` is normalised on entry.  LPT_ERR_INVALID_ARG (and nothing
 * appended or changed) for a non-finite field, an unknown type, a zero direction of a spot or directional light, a
 * negative range or colour. */
int lpt_scene_add_punctual_light(lpt_scene *scene, const lpt_punctual_light *l, uint32_t *out_index);
int lpt_scene_set_punctual_light(lpt_scene *scene, uint32_t index, const lpt_punctual_light *l);
int lpt_scene_punctual_count(const lpt_scene *scene, uint32_t *out);
int lpt_scene_get_punctual_lights(const lpt_scene *s, uint32_t first, uint32_t count, lpt_punctual_light *dst);
/* build-only extension: the record of a light of `type` (LPT_PUNCTUAL_*) from what KHR_lights_punctual states: colour (rgb, NULL =
 * white) x intensity, range (0 = unlimited), the spot's cone angles in radians (0 <= inner < outer <= pi/2; ignored for the other
 * types), position / direction (3 floats each; NULL = the origin / -Z, glTF's default axis).  Fills the derived `cone` fields (in
 * double, rounded once).  The same checks as lpt_scene_add_punctual_light, plus the cone angles. */
int lpt_punctual_light_make(uint32_t type, const float *position, const float *direction, const float *color, float intensity,
                            float range, float inner_angle, float outer_angle, lpt_punctual_light *out);

/* build-only extension (SPEC.md §20; the reference's loader reads no alphaMode): alpha-masked (cutout) materials.  The 32-byte
 * lpt_material keeps the reference's layout; the alpha state is a side table with one entry per material, opaque by default.
 * `mode` 0 = opaque, 1 = mask: a triangle hit counts iff color.w (times the bilinear alpha of image `alpha_image`, unless that is
 * LPT_INVALID_INDEX) >= cutoff — for closest-hit and shadow rays alike.  LPT_ERR_INVALID_ARG, and nothing changed, for a material
 * or image index out of range, a negative or non-finite cutoff, a mode greater than 1.  Out-pointers of the getter may be NULL. */
#define LPT_ALPHA_OPAQUE 0u
#define LPT_ALPHA_MASK 1u
int lpt_scene_set_material_alpha(lpt_scene *scene, uint32_t material_index, uint32_t mode, float cutoff, uint32_t alpha_image);
int lpt_scene_get_material_alpha(const lpt_scene *scene, uint32_t material_index, uint32_t *mode, float *cutoff, uint32_t *alpha_image);
/* build-only extension (SPEC.md §26): alpha-blended materials as stochastic coverage.  A third state of the same side table, reported by
 * lpt_scene_get_material_alpha as mode LPT_ALPHA_BLEND: a triangle hit counts iff the same alpha `a` > xi, where xi in [0, 1) is a hash of
 * the hit's own (prim, u, v) — so a surface of alpha `a` is seen, and shadows, with probability `a` over the samples of a pixel.  BLEND has
 * no cutoff, hence a setter of its own: the stored cutoff returns to 0.5 and is not read.  LPT_ERR_INVALID_ARG, and nothing changed, for
 * a material or image index out of range.  lpt_scene_set_material_alpha with mode 0 or 1 changes a blended material back; its mode 2
 * stays LPT_ERR_INVALID_ARG. */
#define LPT_ALPHA_BLEND 2u
int lpt_scene_set_material_alpha_blend(lpt_scene *scene, uint32_t material_index, uint32_t alpha_image);

/* build-only extension (SPEC.md §21; the reference's loader reads no KHR_materials_transmission): transmissive materials.  A second
 * side table beside the 32-byte lpt_material, opaque (factor 0) by default.  With factor tr in (0, 1] a hit on the material is, with
 * probability tr * (1 - metallic), a smooth dielectric interface of index `ior`: Fresnel reflection or refraction, tinted by the base
 * colour when transmitted.  `thin_walled` != 0: a pane without thickness (the ray goes straight on); 0: the boundary of a closed
 * solid with outward winding.  factor 0 returns the material to opaque.  LPT_ERR_INVALID_ARG, and nothing changed, for a material
 * index out of range, a factor outside [0, 1], an ior below 1, a non-finite number.  Out-pointers of the getter may be NULL. */
int lpt_scene_set_material_transmission(lpt_scene *scene, uint32_t material_index, float factor, float ior, uint32_t thin_walled);
int lpt_scene_get_material_transmission(const lpt_scene *scene, uint32_t material_index, float *factor, float *ior, uint32_t *thin_walled);

/* build-only extension (SPEC.md §29): rough transmission, frosted glass.  One bit per material, 0 by default, kept beside the transmission
 * state and independent of it (lpt_scene_set_material_transmission leaves it alone; factor 0 and back keeps it).  It acts only while the
 * material is transmissive: with `on` = 1 an interface event on the material whose roughness (the material's, times the mra texture's
 * green at the hit) is at least 0.045 samples a GGX microfacet normal and reflects or refracts about it — a thin-walled pane mirrors the
 * reflected direction to the far side —; below 0.045 the event is the smooth one of §21, bit for bit.  LPT_ERR_INVALID_ARG, and nothing
 * changed, for a material index out of range or `on` > 1.  The getter's out-pointer may be NULL. */
int lpt_scene_set_material_transmission_rough(lpt_scene *scene, uint32_t material_index, uint32_t on);
int lpt_scene_get_material_transmission_rough(const lpt_scene *scene, uint32_t material_index, uint32_t *on);

/* build-only extension (SPEC.md §28; the reference's loader reads no KHR_materials_volume): volume attenuation, glTF's
 * KHR_materials_volume.attenuationColor and .attenuationDistance.  Kept beside the transmission state and independent of it (factor 0 and
 * back keeps it); default colour (1, 1, 1) and distance +inf, which is none.  It acts only while the material is transmissive and solid
 * (factor > 0, thin_walled 0): a path segment that ends on the inside of the solid's own face is scaled per channel by exp(-sigma_c t),
 * Beer-Lambert, with sigma_c = -log(color[c]) / distance derived here once (0 for a component of 1 or a distance of +inf, FLT_MAX for a
 * component of 0 or an overflowing quotient; always finite and >= 0).  LPT_ERR_INVALID_ARG, and nothing changed, for a material index out
 * of range, a colour component that is non-finite or outside [0, 1], a distance that is NaN or <= 0.  Out-pointers of the getter may be NULL. */
int lpt_scene_set_material_attenuation(lpt_scene *scene, uint32_t material_index, const float color[3], float distance);
int lpt_scene_get_material_attenuation(const lpt_scene *scene, uint32_t material_index, float color[3], float *distance, float sigma[3]);

/* build-only extension (SPEC.md §22; the reference's loader reads no emissiveFactor): emissive materials.  A third side table beside
 * the 32-byte lpt_material, non-emissive by default.  Le_c = factor[c] * strength (one float product per channel, made here); a path
 * that hits a triangle of the material, from either side and on any bounce, picks up Le — times the sRGB-decoded rgb of `image` at the
 * hit's texture coordinate when `image` is not LPT_INVALID_INDEX — with weight 1.  No light sample is drawn toward such triangles.
 * Le = 0 in all channels returns the material to non-emissive and drops the record (the getter then reports no image).
 * LPT_ERR_INVALID_ARG, and nothing changed, for a material index out of range, a negative or non-finite number or product, an image
 * index out of range.  The getter returns Le (the products), not the factor and the strength; its out-pointers may be NULL. */
int lpt_scene_set_material_emission(lpt_scene *scene, uint32_t material_index, const float factor[3], float strength, uint32_t image);
int lpt_scene_get_material_emission(const lpt_scene *scene, uint32_t material_index, float le[3], uint32_t *image);

/* build-only extension (SPEC.md §24; the reference's loader reads no normalTexture): tangent-space normal maps.  A fourth side table
 * beside the 32-byte lpt_material, no map by default.  A surface hit on a triangle of the material shades with the interpolated normal
 * perturbed by the linear rgb of `image` at the hit's texture coordinate — x and y times `scale` — in a per-triangle frame made from
 * the uv derivatives and re-orthogonalised against the interpolated normal (the TANGENT attribute is not read).
 * image == LPT_INVALID_INDEX removes the map (the getter then reports no image and scale 1).
 * LPT_ERR_INVALID_ARG, and nothing changed, for a material or image index out of range or a non-finite scale.  The getter's
 * out-pointers may be NULL. */
int lpt_scene_set_material_normal_map(lpt_scene *scene, uint32_t material_index, uint32_t image, float scale);
int lpt_scene_get_material_normal_map(const lpt_scene *scene, uint32_t material_index, uint32_t *image, float *scale);

/* Read-back of the flat arrays (the reference exposes them as pub Vec fields). */
int lpt_scene_get_materials(const lpt_scene *s, uint32_t first, uint32_t count, lpt_material *dst);
int lpt_scene_get_entries(const lpt_scene *s, uint32_t first, uint32_t count, lpt_blas_entry *dst);
int lpt_scene_get_vertices(const lpt_scene *s, uint32_t first, uint32_t count, lpt_vertex *dst);
int lpt_scene_get_indices(const lpt_scene *s, uint32_t first, uint32_t count, uint32_t *dst);
int lpt_scene_get_instances(const lpt_scene *s, uint32_t first, uint32_t count, lpt_instance *dst);
int lpt_scene_get_lights(const lpt_scene *s, uint32_t first, uint32_t count, lpt_light *dst);
int lpt_scene_get_image(const lpt_scene *s, uint32_t index, uint32_t *width, uint32_t *height,
                        uint8_t *dst_rgba8 /* may be NULL to query the size */);

/* ---- loaders --------------------------------------------------------------
 * replaces: loaders::load_gltf(&[u8], &mut Scene) -> Result<(), Error>
 * (crates/lib/src/loaders/gltf.rs:46-156).  Accepts .glb or .gltf JSON with
 * embedded (data: URI) buffers; appends to `scene` with the reference's offset
 * rules (:60,109-110).  LPT_ERR_FILE_NOT_FOUND on any parse failure (:49-53). */
int lpt_load_gltf(lpt_scene *scene, const uint8_t *data, size_t size);
/* replaces: loaders::load_gltf_path (gltf.rs:158-161) */
int lpt_load_gltf_path(lpt_scene *scene, const char *path);
/* build-only extension (SPEC.md §14 (7), §26): the two loaders with `flags`.  flags = 0 is lpt_load_gltf / lpt_load_gltf_path byte for
 * byte.  LPT_GLTF_READ_BLEND: a material with alphaMode "BLEND" is marked blended (lpt_scene_set_material_alpha_blend) instead of
 * loading as opaque; its alpha image is chosen as a MASK material's is, and its alphaCutoff is validated and ignored.
 * LPT_GLTF_READ_ROUGH_TRANSMISSION (SPEC.md §29): every material the file makes transmissive is also marked rough
 * (lpt_scene_set_material_transmission_rough), so its roughnessFactor (times the metallicRoughnessTexture's green) frosts it — glTF's
 * default roughnessFactor of 1 is then fully frosted, glTF's own rule; without the flag such glass loads clear, as before.
 * LPT_ERR_INVALID_ARG, and an untouched scene, for an unknown flag bit (2 is one); every other rejection as lpt_load_gltf. */
#define LPT_GLTF_READ_BLEND 1u
#define LPT_GLTF_READ_ROUGH_TRANSMISSION 4u
int lpt_load_gltf_ex(lpt_scene *scene, const uint8_t *data, size_t size, uint32_t flags);
int lpt_load_gltf_path_ex(lpt_scene *scene, const char *path, uint32_t flags);

/* replaces: the `image::ImageBuffer::save` half of ApplicationContext::save_screenshot
 * (crates/standalone/src/app.rs:172-187): writes RGBA8 rows (e.g. from lpt_renderer_read_pixels) as a PNG. */
int lpt_write_png(const char *path, const uint8_t *rgba8, uint32_t width, uint32_t height, size_t row_bytes);

/* replaces: the `image::codecs::hdr::HdrDecoder` step of ApplicationContext::load_env
 * (crates/standalone/src/app.rs:138-155): Radiance RGBE (.hdr) bytes -> the 4-byte RGBE pixels ProbeGPU::new takes,
 * rows top to bottom.  Call with rgbe8 == NULL to get the size, then with a buffer of width*height*4 bytes.
 * LPT_ERR_FILE_NOT_FOUND when the data is not a decodable "-Y H +X W" 32-bit_rle_rgbe image. */
int lpt_decode_hdr(const uint8_t *data, size_t size, uint8_t *rgbe8, size_t capacity, uint32_t *width, uint32_t *height);

/* replaces: the `image::io::Reader::open(path).decode()` step of ApplicationContext::load_blue_noise
 * (crates/standalone/src/app.rs:116-132): PNG or Huffman-coded JPEG bytes -> RGBA8 pixels, rows top to bottom (channels the
 * file lacks are 0, as in the glTF image path), e.g. for lpt_renderer_upload_noise.  Call with rgba8 == NULL to get the size. */
int lpt_decode_image(const uint8_t *data, size_t size, uint8_t *rgba8, size_t capacity, uint32_t *width, uint32_t *height);

/* new (the linear-radiance counterpart of lpt_write_png): RGBA float rows (e.g. lpt_renderer_read_radiance)
 * as a Radiance RGBE .hdr file (alpha dropped, negative / NaN -> 0).  row_floats = floats between row starts (>= 4*width). */
int lpt_write_hdr(const char *path, const float *rgba, uint32_t width, uint32_t height, size_t row_floats);

/* ---- SceneGPU / ProbeGPU --------------------------------------------------
 * replaces: SceneGPU::new_from_scene(&Scene,&Device,&Queue)
 * (crates/lib/src/scene.rs:151-188).  Bakes every instance into world space,
 * builds the wide BVH on the host and copies nodes / triangles / vertices /
 * materials / lights / image atlas into HBM.  The CPU scene stays with the
 * caller.  LPT_ERR_ACCEL_BUILD when the build fails. */
int lpt_scene_upload(lpt_device *dev, const lpt_scene *scene, lpt_scene_gpu **out);
/* new (the reference builds its BVH on the CPU at load time, loaders/gltf.rs:97-105): the same upload with
 * a choice of builder.  LPT_ACCEL_BUILD_HOST_SAH = binned-SAH + SAH-optimal 8-wide collapse on the host (what
 * lpt_scene_upload does); LPT_ACCEL_BUILD_GPU_LBVH = Morton-code radix tree collapsed to 8-wide nodes on the GPU
 * (a few milliseconds; lower tree quality) for scenes that are rebuilt every frame; with it the instances are also baked
 * on the device (object-space meshes + one transform per instance travel, nothing else is computed on the host).
 * Rendered results are identical. */
#define LPT_ACCEL_BUILD_HOST_SAH 0u
#define LPT_ACCEL_BUILD_GPU_LBVH 1u
/* or-ed into `flags`: do not interleave the (albedo, mra) textures of a material (experiments; the frame does not change by a bit) */
#define LPT_UPLOAD_NO_TEXTURE_PAIRS 0x100u
int lpt_scene_upload_ex(lpt_device *dev, const lpt_scene *scene, uint32_t flags, lpt_scene_gpu **out);
int lpt_scene_gpu_destroy(lpt_scene_gpu *sg);
/* replaces: Instance::set_transform + a new SceneGPU (crates/standalone/src/lib.rs:118-121, scene.rs:151):
 * after lpt_scene_set_instance_transform on the CPU scene, re-bakes only the changed instances and refits the
 * wide BVH on the GPU (topology kept).  The meshes and the instance list must be the uploaded ones
 * (LPT_ERR_INVALID_ARG otherwise: upload again).  Renderers bound to this lpt_scene_gpu keep working; call
 * lpt_renderer_reset_accumulation as after any scene change.  out_rebaked may be NULL. */
int lpt_scene_gpu_update_instances(lpt_scene_gpu *scene_gpu, const lpt_scene *scene, uint32_t *out_rebaked);
/* new: like lpt_scene_gpu_update_instances, but every instance is re-baked and the tree is REBUILT on the GPU
 * (Morton radix tree, as LPT_ACCEL_BUILD_GPU_LBVH) instead of refitted — for edits that move things far, where a refit
 * keeps a topology that no longer fits.  Renderers bound to this lpt_scene_gpu keep working. */
int lpt_scene_gpu_rebuild(lpt_scene_gpu *scene_gpu, const lpt_scene *scene);
int lpt_scene_gpu_stats(const lpt_scene_gpu *sg, lpt_accel_stats *out);
/* build-only extension (SPEC.md §19): after lpt_scene_set_punctual_light on the CPU scene, copies the punctual lights to the device
 * again and nothing else — no bake, no refit: an animated lamp costs 64 bytes per light.  The scene must hold as many punctual lights
 * as were uploaded (LPT_ERR_INVALID_ARG otherwise: lpt_scene_gpu_rebuild or a new upload takes a changed count).  Ordering, as for
 * lpt_scene_gpu_update_instances: raytrace() calls that are recorded but not yet submitted are submitted FIRST and see the lights as
 * they were when they were recorded; the call then waits for the device before it writes.  Call lpt_renderer_reset_accumulation as
 * after any scene change. */
int lpt_scene_gpu_update_punctual(lpt_scene_gpu *scene_gpu, const lpt_scene *scene);
/* build-only extension (SPEC.md §19), for tests and tools in the manner of lpt_probe_sample: the function the shading kernels run for
 * punctual light `light_index`, once per point of points[n][3] -> wi[n][3] (unit direction towards the light), dist[n] (the shadow
 * ray's length before the 0.999 factor; 1e30, the renderer's infinity, for a directional light) and E[n][3] (the incident term:
 * colour x intensity x 1/d^2 x range window x cone window); all zero where there is no sample (the point IS the light).  Blocking; host arrays. */
int lpt_scene_gpu_sample_punctual(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t light_index, const float *points, uint32_t n,
                                  float *wi, float *dist, float *E);

/* build-only extension (SPEC.md §23; no reference counterpart): the sampling distribution of the scene's emissive triangles, pure host
 * arithmetic (no GPU): the instances of emissive materials are baked on the host (SPEC.md §2.5) and every baked triangle with a non-zero
 * binary32 cross product becomes an entry, in prim-id order, with the weight area x lum(Le).  Writes min(*n_e, cap) entries of the
 * alias table — q (the probability of keeping the slot), alias (the other slot), prim_self and prim_alias (the baked triangle ids of
 * the slot and of its alias) —, *n_e (the number of entries, which may exceed cap) and *sum_w (the sum of the weights; 0 with
 * *n_e = 0: the scene has no distribution).  NULL outputs other than n_e are skipped. */
int lpt_scene_emitter_distribution(const lpt_scene *scene, uint32_t cap, float *q, uint32_t *alias, uint32_t *prim_self, uint32_t *prim_alias,
                                   uint32_t *n_e, double *sum_w);
/* build-only extension (SPEC.md §23), for tests and tools in the manner of lpt_scene_gpu_sample_punctual: the emitter sample of the
 * shading kernels (kernels.h emitter_sample), once per point of points[n][3] with the draws rands[n][4] = {ra, rb, r1, r2} ->
 * prim[n] (the picked baked triangle), sampled[n] (0: no sample, the other outputs are then zero), y[n][3] (the point on the emitter),
 * wi[n][3] (unit direction towards it), dist[n], cl[n] (the cosine at the emitter), p_a[n] (the area density lum(Le) / sum_w) and
 * E[n][3] (Le x the emissive image).  LPT_ERR_INVALID_ARG for a scene without a distribution.  Blocking; host arrays. */
int lpt_scene_gpu_sample_emitter(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const float *points, const float *rands, uint32_t *prim,
                                 uint32_t *sampled, float *y, float *wi, float *dist, float *cl, float *p_a, float *E);

/* build-only extension (SPEC.md §24), for tests and tools in the manner of lpt_scene_gpu_sample_emitter: the shading normal the
 * shading kernels use at a hit of baked triangle prim[i] at barycentrics bary[i] = (u, v), seen along the unit direction dirs[i] —
 * §12's normal, run through the kernels' own normal-map function where the triangle's material has a map.  ns_out[n][3]; mapped_out[i]
 * = 1 where the perturbed normal was taken, 0 where §12's was kept (no map, or one of §24's fallbacks).  Works for any prim below the
 * scene's baked triangle count (LPT_ERR_INVALID_ARG otherwise); a degenerate triangle gives zeros. */
int lpt_scene_gpu_shading_normal(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *bary, const float *dirs,
                                 float *ns_out, uint32_t *mapped_out);

/* build-only extension (SPEC.md §9), for tests and tools in the manner of lpt_scene_gpu_shading_normal: what a hit of baked triangle
 * prim[i] at barycentrics bary[i] = (u, v) reads from its textures, through the shading kernels' own lookups and dispatch.
 * out[n][16] = {albedo rgb (sRGB-decoded), mra g, mra b (1 where the material has no such texture), the emissive image's texel rgb
 * (1 without one), the normal map's texel xyz as stored in [0, 1] (0 without one), 1 where §20's alpha mask (§26's coverage test for a blended material) cuts the hit away else 0
 * (0 in a scene without masks), the interpolated texture coordinate (tu, tv), 0, 0}.  LPT_ERR_INVALID_ARG for a prim at or beyond the
 * scene's baked triangle count.  Blocking; host arrays. */
int lpt_scene_gpu_sample_textures(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *bary, float *out);

/* build-only extension (SPEC.md §27), for tests and tools in the manner of lpt_scene_gpu_shading_normal: what a punctual light's
 * shadow ray along the unit direction dirs[i] is answered at a hit of baked triangle prim[i] at barycentrics bary[i] = (u, v), by the
 * traversal's own function.  out[n][8] = {the channel transmittance tau rgb, the threshold xi, the pass bits as a uint32 (bit c: tau_c >
 * xi), 0, 0, 0}; zeros for a triangle that is no thin-walled transmissive pane (opaque, solid glass) and for a degenerate one (xi is
 * still the pane's there).  LPT_ERR_INVALID_ARG for a prim at or beyond the scene's baked triangle count.  Blocking; host arrays. */
int lpt_scene_gpu_glass_shadow(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *bary, const float *dirs, float *out);

/* build-only extension (SPEC.md §28), for tests and tools in the manner of lpt_scene_gpu_glass_shadow: the volume attenuation the
 * shading kernels apply to a ray along the unit direction dirs[i] that hits baked triangle prim[i] at distance t[i], by their own function.
 * out[n][4] = {A_r, A_g, A_b, applies (0 / 1)}; {1, 1, 1, 0} where the rule does not apply: an opaque, thin-walled or non-attenuating
 * triangle, a degenerate one, a hit on the front of the face.  LPT_ERR_INVALID_ARG for a prim at or beyond the scene's baked triangle count.
 * Blocking; host arrays. */
int lpt_scene_gpu_attenuation(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *dirs, const float *t, float *out);

/* build-only extension (SPEC.md §21), for tests and tools in the manner of lpt_probe_sample: the interface event of the shading kernels
 * (kernels.h interface_sample), once per element.  Inputs, n of each: dirs[n][3] the ray's unit direction d, ns[n][3] the shading
 * normal, ngf[n][3] the geometric normal flipped against d, entering[n] (non-zero: the geometric normal was not flipped), base[n][3]
 * the base colour, ior[n], thin[n] (non-zero: thin-walled), r4[n] the uniform that picks reflection against the Fresnel term.
 * Outputs: wi[n][3] the next direction, weight[n][3], kind[n] (0 = reflected, 1 = transmitted).  Blocking; host arrays. */
int lpt_interface_sample(lpt_device *dev, uint32_t n, const float *dirs, const float *ns, const float *ngf, const uint32_t *entering,
                         const float *base, const float *ior, const uint32_t *thin, const float *r4, float *wi, float *weight, uint32_t *kind);

/* build-only extension (SPEC.md §29), for tests and tools in the manner of lpt_bsdf_probe: the interface event of a material whose rough
 * bit is set, by the shading kernels' own function (kernels.h interface_sample_rough), once per element.  in[n][19] = {d[3] the ray's unit
 * direction, Ns[3] the shading normal, Ngf[3] the geometric normal flipped against d, entering (non-zero: the geometric normal was not
 * flipped), base[3], ior, thin (non-zero: thin-walled), roughness (the hit's, before any clamp), r4 (picks reflection against the Fresnel
 * term), u1 (the azimuth: the kernels pass r5), u2 (the kernels pass r1)}.  out[n][6] = {wi[3] the next direction, weight[3]}; kind[n] =
 * 0 reflected, 1 transmitted, 2 the path ended (wi and weight are zero), plus 4 where the roughness was below 0.045 and the smooth event
 * of §21 was taken (then wi, weight and the low bits are lpt_interface_sample's).  Blocking; host arrays. */
int lpt_interface_sample_rough(lpt_device *dev, uint32_t n, const float *in, float *out, uint32_t *kind);

/* build-only extension (SPEC.md §10), for tests and tools in the manner of lpt_interface_sample: the BSDF of the shading kernels
 * (device_math.h), once per element, set up as a surface hit sets it up: make_surface, NoV = max(dot(N, V), LPT_MIN_NOV),
 * spec_probability; then bsdf_eval at L and bsdf_sample with the draws (r3, r4, r5).  in[n][20] = {base[3], roughness, metallic,
 * N[3] the shading normal, Ng[3] the geometric normal, V[3] the unit direction towards the viewer, L[3] the unit direction to
 * evaluate, r3, r4, r5}.  out[n][12] = {pspec, f[3], pdf (of L), L_s[3] the sampled direction, weight[3], pdf_s (of L_s)};
 * ok[n] = 1 where the sample exists, else 0 and its five outputs are zero.  Blocking; host arrays. */
int lpt_bsdf_probe(lpt_device *dev, uint32_t n, const float *in, float *out, uint32_t *ok);

/* replaces: ProbeGPU::new(device, queue, data, width, height)
 * (crates/lib/src/scene.rs:72-121): 4 bytes/pixel RGBE8, equirectangular. */
int lpt_probe_upload(lpt_device *dev, const uint8_t *rgbe8, uint32_t width, uint32_t height,
                     lpt_probe **out);
int lpt_probe_destroy(lpt_probe *probe);
/* new (environment importance sampling, SPEC.md §18; no reference counterpart): the probe's sampling distribution, pure host
 * arithmetic (no GPU).  For a width x height RGBE8 probe: pdf_uv[height][width] (the density over the unit square of (u, v)),
 * the marginal over rows as an alias table (row_q, row_alias: height entries) and each row's conditional (col_q, col_alias:
 * height x width entries, alias = a column of the same row); *total = the sum of the weights, 0 = the probe has no distribution
 * (black).  NULL outputs are skipped. */
int lpt_env_distribution(const uint8_t *rgbe8, uint32_t width, uint32_t height, float *pdf_uv, float *row_q, uint32_t *row_alias,
                         float *col_q, uint32_t *col_alias, double *total);
/* new (SPEC.md §18): the renderer's environment sampler run on the GPU, for tests and tools.  lpt_probe_sample: n draws of
 * uniforms[n][6] = {r6, r7, r8, r9, r1, r2} -> dirs[n][3], their density pdf_s[n] (per steradian) and the probe's radiance
 * radiance[n][3] (a draw without a sample, or a probe without a distribution: all zero).  lpt_probe_pdf: the density p_e of
 * dirs[n][3] (0 without a distribution).  Blocking; host arrays.  The distribution is built on first use and kept with the probe. */
int lpt_probe_sample(lpt_device *dev, lpt_probe *probe, const float *uniforms, uint32_t n, float *dirs, float *pdf_s, float *radiance);
int lpt_probe_pdf(lpt_device *dev, lpt_probe *probe, const float *dirs, uint32_t n, float *pdf_e);
/* build-only extension (SPEC.md §9), for tests and tools: the probe's radiance radiance[n][3] along dirs[n][3], through the lookup a
 * miss and an environment sample run (any probe; no distribution is needed).  Blocking; host arrays. */
int lpt_probe_lookup(lpt_device *dev, lpt_probe *probe, const float *dirs, uint32_t n, float *radiance);

/* ---- ray queries (the IntersectorPass on its own) -------------------------
 * replaces: passes::IntersectorPass dispatch (crates/lib/src/renderer.rs:458-463)
 * applied to caller-supplied rays.  `origins`/`dirs` are n×3 floats on the
 * HOST; results come back to the host.  Used by the parity tests. */
int lpt_trace_closest(lpt_device *dev, const lpt_scene_gpu *sg, const float *origins,
                      const float *dirs, uint32_t n, lpt_hit *out_hits);
int lpt_trace_occluded(lpt_device *dev, const lpt_scene_gpu *sg, const float *origins,
                       const float *dirs, const float *tmax, uint32_t n, uint8_t *out_occluded);

/* ---- Renderer --------------------------------------------------------------
 * replaces: Renderer::new(&Device, (w,h), swapchain_format)
 * (crates/lib/src/renderer.rs:220-324).  Applies downsample_factor 0.5 like
 * the reference (:225); there is no swapchain. */
int lpt_renderer_create(lpt_device *dev, uint32_t width, uint32_t height, lpt_renderer **out);
int lpt_renderer_destroy(lpt_renderer *r);
/* replaces: pub downsample_factor (renderer.rs:203).  Takes effect at the next resize. */
int lpt_renderer_set_downsample(lpt_renderer *r, float factor);
/* replaces: Renderer::resize(&Device,&SceneGPU,Option<&ProbeGPU>,(w,h)) (renderer.rs:326-358) */
int lpt_renderer_resize(lpt_renderer *r, const lpt_scene_gpu *sg, const lpt_probe *probe_or_null,
                        uint32_t width, uint32_t height);
/* replaces: Renderer::get_size (renderer.rs:683) — the path-traced size */
int lpt_renderer_get_size(const lpt_renderer *r, uint32_t *width, uint32_t *height);
/* replaces: Renderer::max_ssbo_element_in_bytes (renderer.rs:209-218) */
uint32_t lpt_max_per_pixel_bytes(void);
/* replaces: Renderer::set_resources(&Device,&SceneGPU,Option<&ProbeGPU>)
 * (renderer.rs:687-725); resets frame_count to 1 (:724); a NULL probe is the
 * 1×1 default texture, i.e. a black environment (:693-696, device.rs:13-26). */
int lpt_renderer_set_resources(lpt_renderer *r, const lpt_scene_gpu *sg,
                               const lpt_probe *probe_or_null);
/* replaces: Renderer::raytrace(&mut encoder,&queue,&Mat4) (renderer.rs:392-549).
 * RECORDS one sample per pixel and returns: like the reference, which records the passes of a frame into a command
 * encoder that the app submits once (crates/standalone/src/app.rs:335-337), the launches happen at the next SUBMISSION
 * POINT — lpt_renderer_submit, every call that reads or waits (read_*, blit, exchange, synchronize, get_ray_counts,
 * get_timings, ...) and every setter whose value the passes read (resize, set_resources, set_blit_mode, set_shard, ...).
 * The protocol state of the reference (frame_count, seed, the frame_back toggle) moves at record time.  Consecutive
 * recorded calls with the same view that continue one accumulation are submitted as ONE wavefront of n samples per
 * pixel (bit for bit the result of n separate launches: lpt_renderer_raytrace_n's contract), which is what keeps the
 * persistent traversal waves fed when the caller issues its samples one call at a time.  `view_transform` is
 * camera-to-world (crates/standalone/src/camera.rs:101-108).  Returns LPT_OK and does nothing when resources are unset
 * (renderer.rs:403-407,419-422).  The denoising BlitModes (one temporal pass per call) submit at once.  An error of a
 * deferred launch (e.g. out of device memory) is reported by the call that submits it. */
int lpt_renderer_raytrace(lpt_renderer *r, const float view_transform[16]);
/* replaces: queue.submit(Some(encoder.finish())) (crates/standalone/src/app.rs:335-337): launches what has been recorded.
 * Asynchronous (nothing waits for the GPU); a no-op when nothing is pending. */
int lpt_renderer_submit(lpt_renderer *r);
/* new (no reference knob): how recorded calls become wavefronts.  0 = automatic: up to 64 fusable calls wait for the next
 * submission point, which launches them as wavefronts of about 4 M rays — a larger batch is cut SPATIALLY into runs of
 * whole tile rows (whole tiles on a sharded frame), every run with all the recorded samples; at 1920x1080 the 4 samples of a
 * frame leave as two wavefronts, the upper and the lower half of the image, which take the renderer's wavefront lanes in turn
 * and overlap.  n >= 1: n calls are ONE wavefront of n samples over the whole frame, launched when the n-th is recorded
 * (1 = every raytrace() launches immediately, the round-2 behaviour), up to 64.  Results never depend on the setting.
 * Ray-queue memory: 176 B per ray of a wavefront and wavefront lane. */
int lpt_renderer_set_max_fused(lpt_renderer *r, uint32_t n);
/* new: what record-then-submit has done so far — raytrace() calls recorded (with resources set), wavefronts launched for them,
 * and calls recorded but not yet submitted.  Pure host state: does not submit, does not wait. */
int lpt_renderer_get_submission_stats(const lpt_renderer *r, uint64_t *recorded_calls, uint64_t *wavefronts, uint32_t *pending_calls);
/* Build-only batching of the call above: exactly equivalent (bit for bit) to
 * n x { lpt_renderer_raytrace(r, view); accumulate = true (app.rs:318); } but traced as ONE wavefront
 * of n samples per pixel (sample-major queues), which keeps the persistent traversal waves fed.
 * Seeds advance by max_bounces per sample and samples are accumulated in call order.  1 <= n <= 64. */
int lpt_renderer_raytrace_n(lpt_renderer *r, const float view_transform[16], uint32_t n_samples);
/* replaces: Renderer::reset_accumulation (renderer.rs:609-618) */
int lpt_renderer_reset_accumulation(lpt_renderer *r);
/* replaces: pub accumulate (renderer.rs:204; set by the app at app.rs:318) */
int lpt_renderer_set_accumulate(lpt_renderer *r, int accumulate);
int lpt_renderer_get_accumulate(const lpt_renderer *r, int *accumulate);
/* replaces: global_uniforms.{frame_count,seed} (renderer.rs:286-290) — read-only view */
int lpt_renderer_get_frame_state(const lpt_renderer *r, uint32_t *frame_count, uint32_t *seed);
/* replaces: Renderer::upload_noise_texture (renderer.rs:620-664) */
int lpt_renderer_upload_noise(lpt_renderer *r, const uint8_t *rgba8, uint32_t width,
                              uint32_t height, uint32_t bytes_per_row);
/* replaces: Renderer::use_noise_texture(&queue,bool) (renderer.rs:666-673) */
int lpt_renderer_use_noise(lpt_renderer *r, int flag);
/* replaces: Renderer::set_blit_mode (renderer.rs:675-681) */
int lpt_renderer_set_blit_mode(lpt_renderer *r, int mode);
/* replaces: the ASVGF ping-pong targets the debug BlitModes expose (renderer.rs:557-589,
 * render/asvgf.rs:9-152): current G-buffer (w*h*4 u32: prim id, depth bits, oct normal, RGBA8 albedo),
 * motion (w*h*2 f32, uv units), temporally accumulated radiance+variance (w*h*4 f32), history (w*h u32).
 * Any pointer may be NULL.  Blocking.  Parity surface for the denoiser path. */
int lpt_renderer_read_denoiser(lpt_renderer *r, uint32_t *gbuffer, float *motion, float *radiance, uint32_t *history);
/* replaces: Renderer::blit(&Device,&mut encoder,&TextureView) (renderer.rs:551-607):
 * tonemapped sRGB RGBA8 of the current target into caller memory.  Like lpt_renderer_read_radiance, a frame that is still
 * recorded is submitted together with its read-back: every wavefront's pixel rows are tonemapped and copied as soon as
 * that wavefront has been accumulated (single-GPU Pathtrace frames; also lpt_renderer_read_pixels). */
int lpt_renderer_blit_rgba8(lpt_renderer *r, uint8_t *dst, size_t row_bytes);
/* replaces: async Renderer::read_pixels -> Result<Vec<u8>,Error> (renderer.rs:727-811).
 * Blocking (the reference's device.poll(Wait), :791); w*h*4 bytes, tight rows. */
int lpt_renderer_read_pixels(lpt_renderer *r, uint8_t *dst);
/* new (SPEC.md §30; no reference counterpart): the display transform between the mean radiance and the sRGB bytes of lpt_renderer_blit_rgba8 and
 * lpt_renderer_read_pixels — per pixel c = max(mean * 2^exposure_ev, 0), then the operator's curve, then the sRGB encoding as it was.  LPT_DISPLAY_CLAMP
 * (the default, with exposure 0: every byte, launch and kernel is what it was) is the identity, LPT_DISPLAY_PBR_NEUTRAL the Khronos PBR Neutral curve of the
 * glTF sample viewer, LPT_DISPLAY_ACES Hill's fitted ACES curve.  `exposure_ev` is finite with |ev| <= 64; an unknown operator or any other exposure is
 * LPT_ERR_INVALID_ARG and changes nothing.  The state is read when pixels are presented: the call submits nothing, renders nothing and does not reset the
 * accumulation, and every float output (lpt_renderer_read_radiance*, lpt_write_hdr's input, the denoiser's buffers, the exchange, the G-buffer and motion
 * views) stays linear and untouched.  The getter's out-pointers may be NULL. */
enum { LPT_DISPLAY_CLAMP = 0, LPT_DISPLAY_PBR_NEUTRAL = 1, LPT_DISPLAY_ACES = 2 };
int lpt_renderer_set_display(lpt_renderer *r, float exposure_ev, uint32_t op);
int lpt_renderer_get_display(const lpt_renderer *r, float *exposure_ev, uint32_t *op);
/* new (SPEC.md §30.3): metering.  Submits a recorded frame, builds the luminance histogram of the presented target on the GPU — 384 bins, 8 per octave over
 * [2^-24, 2^24), of the un-exposed mean's Y = 0.2126 r + 0.7152 g + 0.0722 b, so the answer does not depend on the current exposure — and evaluates it on
 * the host: the darkest floor(low * N) and the brightest floor(high * N) of the N histogram samples are left out, and *ev = log2(0.18) - (the mean log2
 * luminance of the rest, taken at the bin centres), the exposure that puts that mean at 18 % grey.  *counted = the samples the mean rests on (0: *ev = 0),
 * *skipped = the sampled pixels without a bin (NaN, infinite, below 2^-24, at or above 2^24); hist384 (384 words) may be NULL, as may every other
 * out-pointer.  low and high lie in [0, 1) with low + high < 1, else LPT_ERR_INVALID_ARG.  Nothing is set: the caller passes *ev to
 * lpt_renderer_set_display if it wants it.  Blocking. */
int lpt_renderer_meter(lpt_renderer *r, float low, float high, float *ev, uint32_t *hist384, uint32_t *counted, uint32_t *skipped);
/* the evaluation alone, pure host arithmetic (no GPU): what lpt_renderer_meter does with its histogram.  The 384 counts must sum to less than 2^32
 * (*counted is 32 bits wide; a frame has fewer pixels), else LPT_ERR_INVALID_ARG with nothing written. */
int lpt_meter_from_histogram(const uint32_t *hist384, float low, float high, float *ev, uint32_t *counted);
/* build-only extensions (SPEC.md §30), for tests and tools in the manner of lpt_bsdf_probe.  lpt_display_probe: the display kernel's own body over n
 * caller-supplied accumulators accum_rgba[n][4] (sum r, g, b and the sample count) -> rgba8[n][4]; exposure and operator as for lpt_renderer_set_display.
 * lpt_meter_probe: the metering kernel itself over such accumulators -> hist384[384] and *skipped.  n = 0 launches nothing (the meter's outputs are zero).
 * Blocking; host arrays. */
int lpt_display_probe(lpt_device *dev, uint32_t n, const float *accum_rgba, float exposure_ev, uint32_t op, uint8_t *rgba8);
int lpt_meter_probe(lpt_device *dev, uint32_t n, const float *accum_rgba, uint32_t *hist384, uint32_t *skipped);
/* Parity surface (no reference twin): mean radiance, w*h*4 floats, a = 1 where
 * this process owns the pixel and has accumulated at least one sample.  Blocking.  `dst` may be pageable memory (the
 * HIP runtime stages the copy: 27 GB/s measured) or memory from lpt_host_alloc (one DMA at link speed).  When the frame is
 * still recorded (the usual case: raytrace() x spp, then this call) the read-back is part of the submission: the pixel rows
 * of every wavefront are resolved and copied as soon as that wavefront has been accumulated, under the wavefronts that are
 * still tracing the other rows (single-GPU Pathtrace frames; 0.39 instead of 0.62 ms exposed at 1920x1080). */
int lpt_renderer_read_radiance(lpt_renderer *r, float *dst);
/* new: page-locked host memory for read-back destinations (the wgpu staging buffer the reference maps in read_pixels,
 * renderer.rs:772-800, is such memory too).  Any lpt_device must exist first.  Free with lpt_host_free. */
int lpt_host_alloc(size_t bytes, void **out);
int lpt_host_free(void *ptr);
/* new: page-lock and map caller-owned host memory for the device (hipHostRegister) — e.g. a POSIX shared-memory segment that every rank
 * of a node maps, as the destination of lpt_renderer_read_radiance_owned.  Any lpt_device must exist first. */
int lpt_host_register(void *ptr, size_t bytes);
int lpt_host_unregister(void *ptr);
/* new (multi-GPU, HOST-SIDE GATHER; no reference counterpart): this rank's OWNED pixels of the mean radiance written straight into
 * `frame_dst`, a whole-frame w*h*4 float destination in page-locked host memory (lpt_host_alloc / lpt_host_register); the other ranks'
 * pixels are not touched.  When the consumer of the frame is the host (the SURVEY 8d span ends in read_radiance) the ranks of a node can
 * all write into ONE shared-memory frame — each GPU pushes its 1/N over its own PCIe link, nothing is gathered on rank 0's GPU first,
 * and a host-side barrier completes the frame: the alternative to lpt_renderer_exchange + lpt_renderer_read_radiance on rank 0
 * (DESIGN 6).  BlitMode::Pathtrace only.  Blocking. */
int lpt_renderer_read_radiance_owned(lpt_renderer *r, float *frame_dst);
/* new (multi-GPU, HOST-SIDE GATHER behind the boundary; replaces, on N ranks, the one blocking call the reference ends a frame with:
 * async Renderer::read_pixels, renderer.rs:727-811 — copy to a staging buffer, map it, device.poll(Wait)).  ONE whole frame (w*h*4 floats)
 * in POSIX shared memory that every rank of a node maps and page-locks; every rank writes its OWN pixels into it straight from its GPU
 * (lpt_renderer_read_radiance_owned(r, frame)) and lpt_host_frame_barrier completes the frame: a line of per-rank progress words in the same
 * segment, pause-spinning for the first microseconds, then futex sleeps.  Rank 0 creates (`name` as for shm_open: "/something"; fails with
 * LPT_ERR_FILE_NOT_FOUND if it exists), the other ranks attach once rank 0 has (the name travels out of band, like the communicator id);
 * destroy unmaps, the creator also unlinks.  A device must exist first (the segment is registered with HIP) unless LPT_HOST_FRAME_HOST_ONLY is
 * passed: a participant that only reads the finished frame (a compositor or encoder process) needs no GPU.  `world` = the barrier's participants. */
typedef struct lpt_host_frame lpt_host_frame;
enum { LPT_HOST_FRAME_HOST_ONLY = 1 };
int lpt_host_frame_create(const char *name, uint32_t width, uint32_t height, uint32_t world, uint32_t flags, lpt_host_frame **out);
int lpt_host_frame_attach(const char *name, uint32_t width, uint32_t height, uint32_t world, uint32_t flags, lpt_host_frame **out);
/* the frame: width * height * 4 floats, row-major, in page-locked shared memory (valid until lpt_host_frame_destroy) */
int lpt_host_frame_ptr(lpt_host_frame *f, float **frame);
/* returns when every one of the `world` participants has called it with this frame number (1, 2, 3, ...: the caller's frame counter, the same
 * on every rank; a rank calls it after its lpt_renderer_read_radiance_owned of that frame has returned).  LPT_ERR_READBACK after timeout_ms.
 * ARRIVE-ONLY over ONE frame: once it returns, frame `frame_no` is complete — and any rank may start writing frame_no + 1 into the same segment.  A consumer that
 * still reads frame_no (rank 0 encoding it, a LPT_HOST_FRAME_HOST_ONLY participant) must hold the writers back itself: a SECOND barrier call (another frame number,
 * e.g. 2 k for "written" and 2 k + 1 for "consumed": bench.py and examples/multi_gpu.c do this) before anybody's next lpt_renderer_read_radiance_owned, or a copy. */
int lpt_host_frame_barrier(lpt_host_frame *f, uint32_t rank, uint32_t frame_no, uint32_t timeout_ms);
int lpt_host_frame_destroy(lpt_host_frame *f);
/* replaces: renderer.queries.values()/labels()
 * (crates/standalone/src/gui/windows/performance_info.rs:19-20) */
int lpt_renderer_get_timings(lpt_renderer *r, lpt_timing *out, int *inout_count);
int lpt_renderer_enable_timings(lpt_renderer *r, int flag);

/* ---- build-only extensions (no reference knob) -------- */
/* reference constant STATIC/MOVING_NUM_BOUNCES = 3 (renderer.rs:398-399) */
int lpt_renderer_set_max_bounces(lpt_renderer *r, uint32_t bounces);
/* new (SPEC.md §18): next-event estimation samples the environment probe too (multiple importance sampling against the BSDF
 * rays that miss).  Off (0) by default; off, every frame is what it was.  Frames change with it — unlike an lpt_option, so it is
 * a call of its own.  Active while the bound probe has a distribution (not black); recorded calls are submitted first. */
int lpt_renderer_set_env_sampling(lpt_renderer *r, int flag);
int lpt_renderer_get_env_sampling(const lpt_renderer *r, int *flag);
/* new (SPEC.md §23): next-event estimation samples the emissive triangles too (multiple importance sampling against the BSDF rays
 * that hit them).  Off (0) by default; off, every frame is what it was (SPEC.md §22).  On, the expectation of a frame is unchanged and
 * its variance drops; the frame's numbers change, so call lpt_renderer_reset_accumulation after a toggle.  Active while the bound
 * scene has an emitter distribution (an emissive material in use on a triangle with an area); recorded calls are submitted first. */
int lpt_renderer_set_emissive_sampling(lpt_renderer *r, int flag);
int lpt_renderer_get_emissive_sampling(const lpt_renderer *r, int *flag);
/* new (SPEC.md §27): the shadow rays of punctual lights pass thin-walled transmissive triangles, each colour channel with the pane's
 * straight-through transmittance (decided per hit from the hit's own bits: no random number is drawn), so a KHR_lights_punctual sun
 * lights a room through a KHR_materials_transmission window.  Off (0) by default; off, every frame, launch and kernel is what it was
 * (SPEC.md §21: shadow rays stop at glass).  Active while the bound scene has a punctual light and a thin-walled transmissive triangle;
 * rectangle lights, the probe and emitters keep stopping at glass (their BSDF partners carry that light), and so does
 * lpt_trace_occluded.  Frames change with the call, so lpt_renderer_reset_accumulation belongs after it; recorded calls are submitted first. */
int lpt_renderer_set_glass_shadows(lpt_renderer *r, int flag);
int lpt_renderer_get_glass_shadows(const lpt_renderer *r, int *flag);
/* new (SPEC.md §25): a thin-lens camera.  `radius` >= 0 is the lens radius in world units (0, the default: the pinhole of SPEC.md §11, and
 * every frame, launch and kernel is what it was, whatever the focus distance); `focus_distance` > 0 (default 1) is the distance of the
 * plane in focus along the view's forward column, in units of its length.  A point on that plane is seen from the pixel the pinhole sees
 * it from; a point at depth z spreads over a disc of radius R |1/F - 1/z| in §11's screen coordinates.  A renderer setting, not scene
 * data (glTF has no such field).  LPT_ERR_INVALID_ARG, with nothing changed, for a negative or non-finite radius and for a focus distance
 * that is not finite and > 0.  Frames change with the call, so lpt_renderer_reset_accumulation belongs after it; recorded calls are
 * submitted first.  The getter's out-pointers may be NULL. */
int lpt_renderer_set_lens(lpt_renderer *r, float radius, float focus_distance);
int lpt_renderer_get_lens(const lpt_renderer *r, float *radius, float *focus_distance);
/* build-only extension (SPEC.md §25), for tests and tools in the manner of lpt_scene_gpu_shading_normal: the primary rays of the
 * renderer's own ray-generation kernel for its current size, shard, seed state, noise texture, vfov and lens, as sample `sample` (< 64)
 * of the next lpt_renderer_raytrace call would start them.  origins[h][w][3], dirs[h][w][3] in full-frame pixel order, zeros at the
 * pixels this rank does not own.  Frame state and accumulation are untouched; recorded calls are submitted first.  Blocking; host arrays. */
int lpt_renderer_primary_rays(lpt_renderer *r, const float view_transform[16], uint32_t sample, float *origins, float *dirs);
int lpt_renderer_set_seed(lpt_renderer *r, uint32_t user_seed);
/* vertical field of view in radians (reference: Camera::default inside albedo) */
int lpt_renderer_set_vfov(lpt_renderer *r, float radians);
/* Pixel-tile sharding for one-process-per-GPU rendering: this process traces
 * the tiles whose index (row-major over ceil(w/tile_w) × ceil(h/tile_h)) is
 * ≡ rank (mod world_size).  Default (0,1,32,8) = everything.  The tile area must be a multiple of 64 (one wave). */
int lpt_renderer_set_shard(lpt_renderer *r, uint32_t rank, uint32_t world_size, uint32_t tile_w,
                           uint32_t tile_h);
/* new: the same with WEIGHTED ownership.  Tile t belongs to virtual rank t % V, V = the sum of the weights, and the virtual
 * ranks are dealt to the ranks in proportion to `weights[rank]` (world_size entries, each 0..8, sum 1..64, at most 32 ranks;
 * NULL = every rank 1 = the rule above).  A rank that also assembles, reads back or filters the frame (rank 0 of an exchange)
 * is given a smaller weight so that its frame takes as long as the others': e.g. {5,8,8,8,8,8,8,8}.  A weight of 0 makes a
 * rank a pure compositor.  Every rank must pass the same weights.  Results do not depend on the weights (the RNG is keyed by
 * the global pixel): tests/test_gpu_exchange.py. */
int lpt_renderer_set_shard_weighted(lpt_renderer *r, uint32_t rank, uint32_t world_size, uint32_t tile_w, uint32_t tile_h,
                                    const uint32_t *weights_or_null);
/* new (multi-GPU denoising; reference: asvgf passes run on the one GPU, renderer.rs:513-522).  With set_shard(world > 1)
 * and a denoising BlitMode, raytrace() fills only this rank's tiles of the filter inputs.  `lpt_renderer_denoiser_inputs`
 * returns the device pointers of the full-frame input buffers of the CURRENT frame (noisy radiance float4, G-buffer
 * uint4, motion float2; n_pixels each; zero outside the rank's tiles) so that the host can sum them onto rank 0 (RCCL
 * reduce; integer sum for the G-buffer).  `lpt_renderer_denoise_filter` then runs temporal accumulation, the a-trous
 * iterations and the composite over the whole frame on that rank (no-op for world == 1: raytrace() already did). */
int lpt_renderer_denoiser_inputs(lpt_renderer *r, void **noisy, void **gbuffer, void **motion, size_t *n_pixels);
int lpt_renderer_denoise_filter(lpt_renderer *r);
/* Device address + byte size of the fp32 RGBA accumulation buffer (rgb = radiance SUM, a = sample count; zero where
 * not owned) for hosts that run their own collective.  Such a host must combine into a buffer of its own: this one is
 * rewritten only on owned pixels, so an in-place reduce would count rank 0's foreign pixels again on the next frame
 * (lpt_renderer_exchange avoids that with a separate presented frame). */
int lpt_renderer_radiance_device_ptr(lpt_renderer *r, void **device_ptr, size_t *bytes);
/* ---- multi-GPU frame exchange (new functionality: the reference is single-GPU; its Device::new is
 * crates/lib/src/device.rs:79 and the only caller of Renderer::raytrace / read_pixels is the one-threaded event loop,
 * crates/standalone/src/app.rs:297-318).  North star: frames shard by pixel tile across the GPUs of a node and the
 * accumulated radiance is combined on rank 0 with RCCL over xGMI.  Everything below is plain RCCL inside the library:
 * a Rust (or any other) host needs no torch.
 *
 *   one process per GPU                          | one process, several GPUs
 *   rank 0: lpt_comm_unique_id(id); ship the     | lpt_comm_unique_id(id); lpt_comm_group_begin();
 *   128 bytes to the other ranks out of band     | for i in 0..n: lpt_comm_create(dev[i], id, i, n, &comm[i]);
 *   every rank: lpt_comm_create(dev, id, rank,   | lpt_comm_group_end();   (and the per-frame exchanges of the n
 *   world, &comm)                                | renderers inside a begin/end pair as well)
 *
 * Then per renderer: lpt_renderer_set_comm(r, comm) (= set_shard(rank, world, 32, 8) + the binding), and per frame
 * raytrace(...) [x spp]; lpt_renderer_exchange(r, mode); on rank 0 read_radiance / read_pixels / blit return the whole
 * frame.  The exchange is enqueued on the renderer's stream behind the frame's kernels (no host synchronisation), so
 * with several renderers the exchange of frame k overlaps the kernels of frame k+1. */
#define LPT_COMM_ID_BYTES 128
/* replaces: nothing (ncclGetUniqueId).  Call once, on one rank. */
int lpt_comm_unique_id(void *out_id /* LPT_COMM_ID_BYTES */);
/* ncclCommInitRank on `dev`.  Collective over the `world_size` callers; LPT_ERR_RCCL on failure. */
int lpt_comm_create(lpt_device *dev, const void *id /* LPT_COMM_ID_BYTES */, int rank, int world_size, lpt_comm **out);
/* Unbind every renderer first (lpt_renderer_set_comm(r, NULL) or destroy it). */
int lpt_comm_destroy(lpt_comm *comm);
/* rank and size as RCCL reports them for the communicator (ncclCommUserRank / ncclCommCount) */
int lpt_comm_info(const lpt_comm *comm, int *rank, int *world_size);
/* ncclGroupStart / ncclGroupEnd: needed only when ONE thread drives several communicators (right column above).
 * lpt_renderer_exchange inside such a bracket enqueues its pack + send / recv / reduce only; RCCL issues them at the
 * outermost end, and lpt_comm_group_end then enqueues what consumes the received data (unpack, filter passes). */
int lpt_comm_group_begin(void);
int lpt_comm_group_end(void);

enum {
    /* every rank sends only the pixels it owns (W*H/N * 16 B; 4 MB per rank at 1080p, N = 8) straight to rank 0 —
     * grouped ncclSend / ncclRecv, seven xGMI links in parallel — which scatters them into the frame.  Default. */
    LPT_EXCHANGE_GATHER_TILES = 0,
    /* ncclReduce(sum, root 0) of the full-frame accumulation buffers (zero outside a rank's tiles): the literal form the
     * north star names; 33 MB around a ring at 1080p.  Bit-identical result (x + 0 = x). */
    LPT_EXCHANGE_REDUCE = 1
};
/* Binds a communicator (NULL unbinds: single-GPU again).  Implies lpt_renderer_set_shard(rank, world, 32, 8) with the
 * communicator's rank / size and therefore resets the accumulation. */
int lpt_renderer_set_comm(lpt_renderer *r, lpt_comm *comm_or_null);
/* lpt_renderer_set_comm with weighted tile ownership (lpt_renderer_set_shard_weighted; `weights` has one entry per rank of the
 * communicator, the same on every rank). */
int lpt_renderer_set_comm_weighted(lpt_renderer *r, lpt_comm *comm_or_null, const uint32_t *weights_or_null);
/* Combines the ranks' accumulation buffers into rank 0's PRESENTED frame (a separate full-frame buffer: every rank's own
 * accumulation buffer stays owned-pixels-only, so progressive frames can be exchanged again and again).  Collective over
 * the communicator; asynchronous; a no-op without a communicator.  In the denoising BlitModes it exchanges the filter
 * inputs instead (lpt_renderer_denoiser_inputs: noisy radiance, G-buffer, motion — owned pixels only, 40 B each, or three
 * ncclReduce in LPT_EXCHANGE_REDUCE mode) and runs the temporal / a-trous / composite passes on rank 0. */
int lpt_renderer_exchange(lpt_renderer *r, int mode);
/* The same exchange among renderers of ONE process without RCCL (peer copies): `root` presents the frame assembled from
 * its own tiles and those of `peers` (n_peers renderers sharded with the same world size and tile shape, on the same or
 * on other devices of the process).  In the denoising BlitModes the filter inputs travel and `root` filters the frame.
 * Used by single-process hosts and by the tests that emulate N ranks on one GPU. */
int lpt_renderer_exchange_local(lpt_renderer *root, lpt_renderer *const *peers, int n_peers);

/* new (no reference knob): the number of wavefront lanes of a renderer (1..4, default 2).  Consecutive SUBMISSIONS (the fused
 * batches of recorded raytrace() calls, or lpt_renderer_raytrace_n calls) take the lanes in turn, each on its own HIP stream
 * with its own ray queues, so the shading of one wavefront overlaps the traversal of the next; accumulation stays in call
 * order on the renderer's stream, so results do not change by a bit.  Costs one set of ray buffers per lane in use. */
int lpt_renderer_set_lanes(lpt_renderer *r, int lanes);
/* new (north star: "a sorted shade / next-event stage using wavefront ballot / prefix-sum"; the reference dispatches the
 * full pixel grid unsorted, renderer.rs:484-509).  flag != 0: the shading pass writes the next-bounce and the shadow-ray
 * queue ordered by direction octant inside every 256-ray block (ballot + popcount per key, LDS prefix sum, still one
 * atomic per block), so a traversal wave's 64 rays share one or two octants.  Results are keyed by pixel slot and do
 * not change by a bit; only traversal coherence does.  flag bits: 1 = next-bounce queue, 2 = shadow queue; any other non-zero
 * value = both queues.  Default: off (each measured slower or neutral on the bench scene). */
int lpt_renderer_set_sort_queues(lpt_renderer *r, int flag);
/* new (the reference has three settings, crates/standalone/src/settings.rs:3-17, none of them about launches): what a host may sanely
 * set about HOW a frame is launched.  EVERY value gives the same frame bit for bit — only which kernels run, and the size of their
 * grids, changes.  The library reads no environment variable for any of this (a host's environment must not change which kernels run). */
typedef enum lpt_option {
    LPT_OPT_PACKET_PRIMARY = 1,     /* bounce 0 by packet traversal, one tree walk per 8x8-pixel patch: 2 (default) = where the patch is narrow (up to 1.8 mrad
                                     * per pixel: 1080p, 4K, 1024^2 at 45 degrees; not a 270p preview), 1 = always, 0 = never (per ray) */
    LPT_OPT_WAVEFRONT_RAYS = 2,     /* rays per wavefront an automatic submission aims at (default 4 194 304) */
    LPT_OPT_PATH_RAYS = 3,          /* wavefronts of at most this many rays run every bounce behind the primary hits in ONE launch (the
                                     * path kernel: no chip-wide barrier per bounce — small frames and the tile shards of a wide multi-GPU
                                     * frame); larger ones take the per-bounce launches of renderer.rs:484-509.  Default 120 000, the
                                     * measured cross-over; 0: never */
    LPT_OPT_COOP_RAYS = 4,          /* wavefronts of at most this many rays — fewer than the chip has wave slots — take the per-bounce launches with EVERY ray
                                     * traced by a whole wave (eight lanes per node): the frame of a tiny wavefront is a chain of dependent traversal steps,
                                     * and a wave per ray shortens it several times over (64x36 pixels, 4 spp: 0.72 -> 0.39 ms per frame).  Default 32 000, the measured cross-over;
                                     * 0 = never.  Not used while lpt_renderer_enable_stats is on */
    LPT_OPT_TAIL_LANES = 5,         /* the tails of the per-bounce traversal launches finished IN PLACE: a wave whose queues are dry and that is down to this
                                     * many live rays (1..8) finishes them cooperatively, all 64 lanes per ray, from where each stands — nothing is
                                     * dropped, restarted at the root or launched behind.  Default 4; 0 = off (then LPT_EXP_STEP_BUDGET applies).  For submissions that
                                     * leave as ONE wavefront; not used while lpt_renderer_enable_stats is on */
    LPT_OPT_EXPERIMENT_BASE = 256   /* LPT_OPT_EXPERIMENT(name): the tuning knobs of the A/B tools and the variant tests — NOT a stable surface */
} lpt_option;
#define LPT_OPT_EXPERIMENT(name) (LPT_OPT_EXPERIMENT_BASE + (name))
/* The experiment knobs (tools/dev, bench.py --opt, tests that compare kernel variants).  Numbers and meanings may change with any build. */
typedef enum lpt_experiment {
    LPT_EXP_PIPE_RAYS = 0,          /* wavefronts of at most this many rays trace with the one-round-trip step (default: all); 0: never */
    LPT_EXP_REFILL = 1,             /* per-bounce traversal: lanes live below which a wave refills (default 44) */
    LPT_EXP_TRACE_WAVES_PER_CU = 2, /* per-bounce traversal: persistent waves per CU; 0 (default): sized from the ray count */
    LPT_EXP_SHADE_BLOCKS_PER_CU = 3,/* shading pass: blocks per CU; 0 (default) = 4 for a wavefront alone on the chip, 3 for the pieces of a cut batch */
    LPT_EXP_PATH_WAVES_PER_CU = 4,  /* path kernel: persistent waves per CU (default 16) */
    LPT_EXP_PATH_REFILL = 5,        /* path kernel: lanes tracing below which a batch of lanes is shaded / restarted (default 32) */
    LPT_EXP_OCC_CELL_MILLI = 6,     /* stats only: grid cell of the occluder-cache probe in 1/1000 scene units (default 250; 0: probe off) */
    LPT_EXP_STEP_BUDGET = 7,        /* per-bounce traversal launches with LPT_OPT_TAIL_LANES 0: a ray not finished after this many steps is dropped by the per-lane
                                     * kernel and traced again by a whole wave (k_trace_coop); default 48, 0 = off.  Not applied while lpt_renderer_enable_stats is on */
    LPT_EXP_BUDGET_RAYS = 8,        /* the tail in place / the step budget apply to submissions that leave as ONE wavefront of at most this many rays (default 3 000 000) */
    LPT_EXP_PACKET_QUADS = 9,       /* packet traversal of bounce 0: 1 (default) = a packet is the four samples of a 4x4-pixel quarter where the frame allows it
                                     * (dense tiles, a multiple of four samples); 0 = always one sample of an 8x8-pixel patch */
    LPT_EXP_SPLIT_RAYS = 10,        /* a batch above this many rays that would still fit one wavefront leaves as two, on the renderer's lanes (default
                                     * 3 000 000; 0: never split below LPT_OPT_WAVEFRONT_RAYS) */
    LPT_EXP_BUDGET_SPLIT = 11,      /* 1: the tail in place / the step budget also apply to the pieces of a cut batch (default 0: only to submissions that leave
                                     * as one wavefront — LPT_EXP_BUDGET_RAYS alone does not turn them on for the pieces) */
    LPT_EXP_LANE_PHASE = 12         /* how the pieces of a cut batch on the renderer's lanes are ordered against each other (stream events, no host waits):
                                     * 0 = free (both lanes run the same launch sequence in step), 1 (default) = offset start (a lane's first launch waits for
                                     * the previous lane's primary traversal), 2 = alternating traversal (one piece's traversal launch at a time, the
                                     * other pieces shade beside it) */
} lpt_experiment;
int lpt_renderer_set_option(lpt_renderer *r, int option, uint64_t value);
int lpt_renderer_get_option(const lpt_renderer *r, int option, uint64_t *value);
/* The shard layout lpt_renderer_set_shard / lpt_renderer_exchange use, for hosts that run their own exchange (pure host
 * arithmetic, no GPU needed): the number of pixel slots rank `rank` owns (whole tiles, including the part of edge tiles
 * outside the image) and where its slots start in the concatenation of all ranks' slot arrays on rank 0. */
int lpt_shard_layout(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t world_size, uint32_t rank,
                     uint32_t *out_slots, uint32_t *out_slot_offset);
int lpt_shard_layout_weighted(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t world_size, uint32_t rank,
                              const uint32_t *weights_or_null, uint32_t *out_slots, uint32_t *out_slot_offset);
/* the rank that owns tile `tile` (row-major over the tile grid) under the ownership rule (weights NULL = tile % world_size) */
int lpt_shard_owner(uint32_t world_size, const uint32_t *weights_or_null, uint32_t tile, uint32_t *out_rank);
int lpt_renderer_get_ray_counts(lpt_renderer *r, lpt_ray_counts *out);
/* per-bounce queue sizes of the LAST traced frame: closest[b] = closest-hit rays of bounce b, shadow[b] = shadow rays
 * emitted by bounce b; up to `cap` entries each (either pointer may be NULL).  Blocking. */
int lpt_renderer_get_queue_counts(lpt_renderer *r, uint32_t *closest, uint32_t *shadow, uint32_t cap);
int lpt_renderer_reset_ray_counts(lpt_renderer *r);
/* new, stats enabled only: traversal steps per ray over the per-bounce traversal launches of the LAST wavefront — the maximum (the longest
 * ray of a launch sets its duration, docs/ROUNDS.md §5.5) and a histogram by power of two (hist12[k]: 2^k <= steps < 2^(k+1)).  Blocking.
 * The stats kernels run WITHOUT the step budget (LPT_EXP_STEP_BUDGET): every ray is traced to its end by the per-lane kernel, so the histogram, the
 * maximum and the nodes / triangles per ray are those of complete traversals, whatever the option says. */
int lpt_renderer_get_step_histogram(lpt_renderer *r, uint32_t *max_steps, uint32_t *hist12);
/* count BVH nodes visited / triangles tested per ray (slower kernel variant) */
int lpt_renderer_enable_stats(lpt_renderer *r, int flag);
int lpt_renderer_synchronize(lpt_renderer *r);
/* The HIP stream (void*: a hipStream_t) this renderer enqueues on.  Each renderer owns one, so two
 * renderers on one device pipeline consecutive frames; the collective layer orders its reduce on it. */
int lpt_renderer_stream(lpt_renderer *r, void **hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LPT_H */
