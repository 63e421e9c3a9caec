// env_dist.cpp — the environment probe's sampling distribution (SPEC §18), built on the host in double precision.
// Weights: the luminance of the 3x3 neighbourhood's brightest texel (x wraps, y clamps; env_lookup is bilinear, so a texel's
// footprint takes light from its neighbours) times the row's sin(theta); a marginal over rows and a conditional per row, each a
// Vose alias table; pdf_uv = W H w / sum(w).  lpt_env_distribution hands the tables out; device.hip uploads them (lpt_probe).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "env_dist.h"

namespace lpt {
namespace {

// SPEC §9 rgbe_decode's luminance, in double: 2^(e - 136) per unit of mantissa, 0 below exponent 10
double texel_lum(const uint8_t *t) {
    if (t[3] < 10u) return 0.0;
    const double s = std::ldexp(1.0, (int)t[3] - 136);
    return (0.2126 * (t[0] * s) + 0.7152 * (t[1] * s)) + 0.0722 * (t[2] * s);
}

}  // namespace

// Vose's alias method over p[0..n): q[i] = the probability of keeping i, alias[i] = the other outcome of its column (env_dist.h: SPEC §23's emitters use it too)
void alias_table(const double *p, uint32_t n, float *q, uint32_t *alias) {
    double total = 0.0;
    for (uint32_t i = 0; i < n; ++i) total += p[i];
    std::vector<double> sc(n);
    std::vector<uint32_t> small, large;
    for (uint32_t i = 0; i < n; ++i) {
        sc[i] = total > 0.0 ? p[i] * (double)n / total : 1.0;   // an empty row: uniform (never picked by its marginal)
        (sc[i] < 1.0 ? small : large).push_back(i);
    }
    while (!small.empty() && !large.empty()) {
        const uint32_t s = small.back(), l = large.back();
        small.pop_back(); large.pop_back();
        q[s] = (float)sc[s]; alias[s] = l;
        sc[l] = (sc[l] + sc[s]) - 1.0;
        (sc[l] < 1.0 ? small : large).push_back(l);
    }
    for (uint32_t i : large) { q[i] = 1.0f; alias[i] = i; }
    for (uint32_t i : small) { q[i] = 1.0f; alias[i] = i; }   // rounding leftovers: their share is 1 within the double's precision
}

double env_distribution(const uint8_t *rgbe8, uint32_t W, uint32_t H, EnvDist &out) {
    const size_t n = (size_t)W * H;
    std::vector<double> lum(n), w(n);
    for (size_t i = 0; i < n; ++i) lum[i] = texel_lum(rgbe8 + 4 * i);
    std::vector<double> row_sum(H, 0.0);
    double total = 0.0;
    for (uint32_t y = 0; y < H; ++y) {
        const double st = std::sin(M_PI * ((double)y + 0.5) / (double)H);
        for (uint32_t x = 0; x < W; ++x) {
            double m = 0.0;
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = std::min(std::max((int)y + dy, 0), (int)H - 1);
                for (int dx = -1; dx <= 1; ++dx) {
                    const uint32_t xx = (uint32_t)(((int64_t)x + dx + (int64_t)W) % (int64_t)W);
                    m = std::max(m, lum[(size_t)yy * W + xx]);
                }
            }
            w[(size_t)y * W + x] = m * st;
            row_sum[y] += m * st;
        }
        total += row_sum[y];
    }
    out.w = W; out.h = H;
    out.pdf_uv.assign(n, 0.0f);
    out.row_q.assign(H, 1.0f); out.row_alias.resize(H);
    out.col_q.assign(n, 1.0f); out.col_alias.resize(n);
    for (uint32_t y = 0; y < H; ++y) out.row_alias[y] = y;
    for (size_t i = 0; i < n; ++i) out.col_alias[i] = (uint32_t)(i % W);
    if (!(total > 0.0)) return 0.0;   // no distribution: a black probe
    alias_table(row_sum.data(), H, out.row_q.data(), out.row_alias.data());
    for (uint32_t y = 0; y < H; ++y) alias_table(&w[(size_t)y * W], W, &out.col_q[(size_t)y * W], &out.col_alias[(size_t)y * W]);
    const double scale = (double)W * (double)H / total;
    for (size_t i = 0; i < n; ++i) out.pdf_uv[i] = (float)(w[i] * scale);
    return total;
}

}  // namespace lpt

int lpt_env_distribution(const uint8_t *rgbe8, uint32_t width, uint32_t height, float *pdf_uv, float *row_q, uint32_t *row_alias, float *col_q,
                         uint32_t *col_alias, double *total) {
    if (!rgbe8 || !width || !height) return lpt::fail(LPT_ERR_INVALID_ARG, "lpt_env_distribution: null or empty probe");
    lpt::EnvDist d;
    const double t = lpt::env_distribution(rgbe8, width, height, d);
    const size_t n = (size_t)width * height;
    if (pdf_uv) std::copy(d.pdf_uv.begin(), d.pdf_uv.end(), pdf_uv);
    if (row_q) std::copy(d.row_q.begin(), d.row_q.end(), row_q);
    if (row_alias) std::copy(d.row_alias.begin(), d.row_alias.end(), row_alias);
    if (col_q) std::copy(d.col_q.begin(), d.col_q.begin() + n, col_q);
    if (col_alias) std::copy(d.col_alias.begin(), d.col_alias.begin() + n, col_alias);
    if (total) *total = t;
    return LPT_OK;
}
