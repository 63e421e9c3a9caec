// emit_dist.h — the emissive triangles' sampling distribution (SPEC §23; emit_dist.cpp).  Internal, not part of the ABI.
#pragma once
#include <cstdint>
#include <vector>

struct lpt_scene;

namespace lpt {

struct EmitDist {
    std::vector<float> q;              // [n_e]: the alias table over the entries (env_dist.h alias_table)
    std::vector<uint32_t> alias;       // [n_e]: a slot
    std::vector<uint32_t> prim;        // [n_e]: the baked triangle of every entry, ascending
    std::vector<double> weight;        // [n_e]: 0.5 sqrt(l2) lum(Le)
    double sum_w = 0.0;                // 0 (and no entry) = no distribution
};

// Bakes the instances of emissive materials on the host (SPEC §2.5) and fills `out`; the prim ids are those of the scene's bake order.
void emitter_distribution(const lpt_scene &scene, EmitDist &out);

}  // namespace lpt
