// emit_dist.cpp — the emissive triangles' sampling distribution (SPEC §23), built on the host.
// One entry per baked triangle of an emissive material whose binary32 cross product is not zero — the test shade_hit makes, on the positions shade_hit reads —, in prim-id
// order; weight = world-space area x lum(Le) in double; one Vose alias table over the entries (env_dist.cpp alias_table).  The emissive image plays no part in the weight.
// lpt_scene_emitter_distribution hands the table out; device.hip uploads it at upload, rebuild and instance update (the areas are world-space).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "emit_dist.h"
#include "env_dist.h"

namespace lpt {

void emitter_distribution(const lpt_scene &scene, EmitDist &out) {
    out = EmitDist();
    std::vector<lpt_vertex> verts;
    size_t first = 0;   // the instance's first baked triangle (SPEC §2.5 order)
    for (size_t ii = 0; ii < scene.instances.size(); ++ii) {
        const lpt_instance &in = scene.instances[ii];
        const size_t n = in.blas_index < scene.entries.size() ? scene.entries[in.blas_index].index_count / 3u : 0u;
        const uint32_t mat = in.material_index < scene.materials.size() ? in.material_index : 0u;
        const MaterialEmission e = scene.material_emission(mat);
        if (n && e.emissive()) {
            const double lum = (0.2126 * (double)e.le[0] + 0.7152 * (double)e.le[1]) + 0.0722 * (double)e.le[2];
            verts.clear();
            bake_instance(scene, ii, verts);
            for (size_t t = 0; t < n && 3 * t + 2 < verts.size(); ++t) {
                const float *p0 = verts[3 * t].position, *p1 = verts[3 * t + 1].position, *p2 = verts[3 * t + 2].position;
                // shade_hit's Ng and l2, binary32 with its parentheses (-ffp-contract=off)
                const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
                const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
                const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
                const float l2 = (nx * nx + ny * ny) + nz * nz;
                if (!(l2 > 0.0f)) continue;
                out.prim.push_back((uint32_t)(first + t));
                out.weight.push_back((0.5 * std::sqrt((double)l2)) * lum);
            }
        }
        first += n;
    }
    for (double w : out.weight) out.sum_w += w;
    if (!(out.sum_w > 0.0) || !std::isfinite(out.sum_w)) { out = EmitDist(); return; }
    const uint32_t n_e = (uint32_t)out.prim.size();
    out.q.assign(n_e, 1.0f);
    out.alias.resize(n_e);
    alias_table(out.weight.data(), n_e, out.q.data(), out.alias.data());
}

}  // namespace lpt

int lpt_scene_emitter_distribution(const lpt_scene *scene, uint32_t cap, float *q, uint32_t *alias, uint32_t *prim_self, uint32_t *prim_alias, uint32_t *n_e, double *sum_w) {
    if (!scene || !n_e) return lpt::fail(LPT_ERR_INVALID_ARG, "lpt_scene_emitter_distribution: null");
    lpt::EmitDist d;
    lpt::emitter_distribution(*scene, d);
    const uint32_t n = (uint32_t)d.prim.size();
    *n_e = n;
    if (sum_w) *sum_w = d.sum_w;
    for (uint32_t i = 0; i < n && i < cap; ++i) {
        if (q) q[i] = d.q[i];
        if (alias) alias[i] = d.alias[i];
        if (prim_self) prim_self[i] = d.prim[i];
        if (prim_alias) prim_alias[i] = d.prim[d.alias[i]];
    }
    return LPT_OK;
}
