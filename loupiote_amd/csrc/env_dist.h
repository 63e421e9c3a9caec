// env_dist.h — the environment probe's sampling distribution (SPEC §18; env_dist.cpp).  Internal, not part of the ABI.
#pragma once
#include <cstdint>
#include <vector>

namespace lpt {

struct EnvDist {
    uint32_t w = 0, h = 0;
    std::vector<float> pdf_uv;         // [h][w]: W H w(x, y) / sum(w), the density over the unit square of (u, v)
    std::vector<float> row_q;          // [h]: the marginal over rows as an alias table
    std::vector<uint32_t> row_alias;
    std::vector<float> col_q;          // [h][w]: each row's conditional as an alias table (alias = a column of the same row)
    std::vector<uint32_t> col_alias;
};

// Vose's alias method over the weights p[0..n) (double): q[i] = the probability of keeping column i, alias[i] = its other outcome.  sum(p) = 0: uniform.
// The one alias build of the library: the probe's rows and columns (SPEC §18) and the emissive triangles (SPEC §23, emit_dist.cpp)
void alias_table(const double *p, uint32_t n, float *q, uint32_t *alias);

// Fills `out` and returns sum(w); 0 = the probe has no distribution (the tables are then uniform and pdf_uv is 0).
double env_distribution(const uint8_t *rgbe8, uint32_t w, uint32_t h, EnvDist &out);

}  // namespace lpt
