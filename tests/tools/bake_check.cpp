// bake_check.cpp — TEST TOOL (never linked into the product): dumps what the host bake makes of a scene.
//
// Fills a scene through the C ABI's host calls from a file, then runs lpt::bake_instance (SPEC §2.5) over every instance in order
// and lpt::woop_from_triangle (SPEC §6) over every baked triangle, and writes both out as binary for tests/test_bake_reference.py.
//
// usage: bake_check <scene.bin> <out.bin>
// scene.bin: u32 n_meshes, per mesh {u32 n_vertices, u32 n_indices, f32 position[n][3], f32 normal[n][3], f32 uv[n][2], u32 index[n_indices]},
//            u32 n_instances, per instance {u32 mesh, u32 material, f32 model_to_world[16]}
// out.bin:   u32 n_triangles, lpt_vertex[3 n] (32 bytes each), f32 woop[n][12] (r0, r1, r2), u32 material[n]
#include <cstdio>
#include <vector>

#include "../../loupiote_amd/csrc/common.h"

namespace {

template <class T> bool rd(FILE *f, T *p, size_t n) { return !n || fread(p, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: bake_check scene.bin out.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("scene"); return 2; }
    lpt_scene *scene = nullptr;
    if (lpt_scene_create(&scene) != LPT_OK) return 1;
    uint32_t n_meshes = 0, n_inst = 0;
    if (!rd(f, &n_meshes, 1)) return 2;
    std::vector<uint32_t> blas(n_meshes);
    for (uint32_t k = 0; k < n_meshes; ++k) {
        uint32_t nv = 0, ni = 0;
        if (!rd(f, &nv, 1) || !rd(f, &ni, 1)) return 2;
        std::vector<float> pos(3 * (size_t)nv), nrm(3 * (size_t)nv), uv(2 * (size_t)nv);
        std::vector<uint32_t> idx(ni);
        if (!rd(f, pos.data(), pos.size()) || !rd(f, nrm.data(), nrm.size()) || !rd(f, uv.data(), uv.size()) || !rd(f, idx.data(), idx.size())) return 2;
        if (lpt_scene_add_mesh(scene, pos.data(), 12, nrm.data(), 12, uv.data(), 8, nv, idx.data(), ni, &blas[k]) != LPT_OK) { fprintf(stderr, "add_mesh: %s\n", lpt_last_error()); return 1; }
    }
    if (!rd(f, &n_inst, 1)) return 2;
    for (uint32_t k = 0; k < n_inst; ++k) {
        uint32_t mesh = 0, mat = 0, out = 0;
        float m[16];
        if (!rd(f, &mesh, 1) || !rd(f, &mat, 1) || !rd(f, m, 16) || mesh >= n_meshes) return 2;
        if (lpt_scene_add_instance(scene, blas[mesh], m, mat, &out) != LPT_OK) { fprintf(stderr, "add_instance: %s\n", lpt_last_error()); return 1; }
    }
    fclose(f);

    std::vector<lpt_vertex> verts;
    std::vector<uint32_t> material;
    for (size_t ii = 0; ii < scene->instances.size(); ++ii) {
        const size_t before = verts.size() / 3;
        const uint32_t mi = lpt::bake_instance(*scene, ii, verts);
        material.insert(material.end(), verts.size() / 3 - before, mi);
    }
    const uint32_t n_tris = (uint32_t)(verts.size() / 3);
    std::vector<lpt::WoopTri> woop(n_tris);
    for (uint32_t t = 0; t < n_tris; ++t) lpt::woop_from_triangle(verts[3 * t].position, verts[3 * t + 1].position, verts[3 * t + 2].position, woop[t]);
    static_assert(sizeof(lpt_vertex) == 32 && sizeof(lpt::WoopTri) == 48, "dump layout");

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 2; }
    fwrite(&n_tris, 4, 1, o);
    fwrite(verts.data(), sizeof(lpt_vertex), verts.size(), o);
    fwrite(woop.data(), sizeof(lpt::WoopTri), woop.size(), o);
    fwrite(material.data(), 4, material.size(), o);
    fclose(o);
    lpt_scene_destroy(scene);
    return 0;
}
