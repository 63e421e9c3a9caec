// display_math.h — the display transform and the meter's arithmetic (SPEC.md §30), callable on the host and on the device.
// Plain C++: nothing here comes from HIP beyond the qualifiers behind LPT_DISPLAY_FN, so one body serves k_display, the device hook
// lpt_display_probe and a CPU check program (tests/tools/display_check.cpp).  Every expression is written with the parenthesisation
// SPEC.md §30 states, in binary32, and is compiled with -ffp-contract=off: nothing is fused.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LPT_DISPLAY_FN __host__ __device__ inline
#else
#define LPT_DISPLAY_FN inline
#endif

namespace lptd {

// the operators of lpt_renderer_set_display (include/lpt.h: LPT_DISPLAY_*)
enum : uint32_t { kDisplayClamp = 0u, kDisplayPbrNeutral = 1u, kDisplayAces = 2u, kDisplayOps = 3u };

struct rgb3 { float r, g, b; };

// §3's max2 / min2: a NaN first argument gives the second
LPT_DISPLAY_FN float disp_max2(float a, float b) { return a > b ? a : b; }
LPT_DISPLAY_FN float disp_min2(float a, float b) { return a < b ? a : b; }
LPT_DISPLAY_FN uint32_t disp_bits(float x) { uint32_t u; memcpy(&u, &x, sizeof u); return u; }
LPT_DISPLAY_FN bool disp_is_inf(float x) { return (disp_bits(x) & 0x7FFFFFFFu) == 0x7F800000u; }

// §30.2: the exposed colour c = max2(m * g, 0) per channel: a NaN and a negative value give 0, +inf stays
LPT_DISPLAY_FN rgb3 display_expose(rgb3 m, float g) {
    rgb3 c;
    c.r = disp_max2(m.r * g, 0.0f); c.g = disp_max2(m.g * g, 0.0f); c.b = disp_max2(m.b * g, 0.0f);
    return c;
}

// §30.2 PBR_NEUTRAL (Khronos PBR Neutral).  p = +inf: np = 1 and the result is (1, 1, 1) by rule (c * (np / p) would be inf * 0)
LPT_DISPLAY_FN rgb3 display_pbr_neutral(rgb3 c) {
    const float x = disp_min2(disp_min2(c.r, c.g), c.b);
    const float off = x < 0.08f ? x - (6.25f * x) * x : 0.04f;
    c.r -= off; c.g -= off; c.b -= off;
    const float p = disp_max2(disp_max2(c.r, c.g), c.b);
    if (p < 0.76f) return c;
    if (disp_is_inf(p)) { c.r = 1.0f; c.g = 1.0f; c.b = 1.0f; return c; }
    const float d = 0.24f;
    const float np = 1.0f - (d * d) / ((p + d) - 0.76f);
    const float s = np / p;
    c.r = c.r * s; c.g = c.g * s; c.b = c.b * s;
    const float k = 1.0f - 1.0f / ((0.15f * (p - np)) + 1.0f);
    c.r = c.r + (np - c.r) * k; c.g = c.g + (np - c.g) * k; c.b = c.b + (np - c.b) * k;
    return c;
}

// §30.2 ACES (Hill's fitted RRT + ODT).  The inputs are clamped to 2^60 first: v * v stays finite and inf / inf never occurs
LPT_DISPLAY_FN float display_aces_fit(float v) {
    const float n = (v * (v + 0.0245786f)) - 0.000090537f;
    const float q = (v * ((0.983729f * v) + 0.4329510f)) + 0.238081f;
    return n / q;
}
LPT_DISPLAY_FN rgb3 display_aces(rgb3 c) {
    const float kMax = 1152921504606846976.0f;   // 2^60
    const float r = disp_min2(c.r, kMax), g = disp_min2(c.g, kMax), b = disp_min2(c.b, kMax);
    const float v0 = display_aces_fit(((0.59719f * r) + (0.35458f * g)) + (0.04823f * b));
    const float v1 = display_aces_fit(((0.07600f * r) + (0.90834f * g)) + (0.01566f * b));
    const float v2 = display_aces_fit(((0.02840f * r) + (0.13383f * g)) + (0.83777f * b));
    rgb3 o;
    o.r = ((1.60475f * v0) + (-0.53108f * v1)) + (-0.07367f * v2);
    o.g = ((-0.10208f * v0) + (1.10813f * v1)) + (-0.00605f * v2);
    o.b = ((-0.00327f * v0) + (-0.07276f * v1)) + (1.07602f * v2);
    return o;
}

// the whole transform of one pixel's mean m up to the value encode_srgb8 takes (which clamps to [0, 1], a NaN to 0)
template <uint32_t OP> LPT_DISPLAY_FN rgb3 display_transform(rgb3 m, float g) {
    static_assert(OP < kDisplayOps, "SPEC §30: three operators");
    const rgb3 c = display_expose(m, g);
    if (OP == kDisplayPbrNeutral) return display_pbr_neutral(c);
    if (OP == kDisplayAces) return display_aces(c);
    return c;
}

// ---- metering (§30.3)
constexpr uint32_t kMeterBins = 384u;   // 8 bins per octave over [2^-24, 2^24)
// Y = the luminance of the un-exposed mean; false: the pixel goes to `skipped` (NaN, infinite, below 2^-24 or at or above 2^24)
LPT_DISPLAY_FN float meter_luminance(rgb3 m) { return ((0.2126f * m.r) + (0.7152f * m.g)) + (0.0722f * m.b); }
LPT_DISPLAY_FN bool meter_bin(float Y, uint32_t &bin) {
    if (!(Y >= 5.9604644775390625e-8f && Y < 16777216.0f)) return false;
    bin = (disp_bits(Y) >> 20) - ((127u - 24u) << 3);
    return true;
}

// The evaluation of a histogram, host only: floor(low * N) samples leave from the bottom and floor(high * N) from the top, a boundary bin giving up only the
// count needed; over the N' that remain, ev = log2(0.18) - (sum of count * centre) / N', centre_b = (b + 0.5) / 8 - 24 (multiples of 1/16: the sum is exact in
// binary64).  N' = 0: ev = 0.  The caller has checked that the counts sum to less than 2^32 (a frame has fewer pixels; lpt_meter_from_histogram refuses more), so
// *counted holds N'.
inline void meter_evaluate(const uint32_t hist[kMeterBins], float low, float high, float *ev, uint32_t *counted) {
    uint64_t h[kMeterBins], N = 0;
    for (uint32_t b = 0; b < kMeterBins; ++b) { h[b] = hist[b]; N += h[b]; }
    uint64_t lo = (uint64_t)((double)low * (double)N), hi = (uint64_t)((double)high * (double)N);   // floor: both are >= 0
    for (uint32_t b = 0; b < kMeterBins && lo; ++b) { const uint64_t t = h[b] < lo ? h[b] : lo; h[b] -= t; lo -= t; }
    for (uint32_t b = kMeterBins; b-- > 0u && hi;) { const uint64_t t = h[b] < hi ? h[b] : hi; h[b] -= t; hi -= t; }
    uint64_t Np = 0;
    double S = 0.0;
    for (uint32_t b = 0; b < kMeterBins; ++b) { Np += h[b]; S += (double)h[b] * (((double)b + 0.5) / 8.0 - 24.0); }
    if (ev) *ev = Np ? (float)(-2.4739311883324124 - S / (double)Np) : 0.0f;
    if (counted) *counted = (uint32_t)Np;
}

}  // namespace lptd
