// The shading kernels' forms: ONE word per instantiation of k_shade / k_path (kernels.h), a bit per feature.  Plain C++17, nothing from HIP: launch_plan.h picks the
// words (plan_wavefront), kernels.h decodes them, device.hip walks them (launch_k_shade / launch_k_path), and a CPU test can say which kernel a set of facts runs.
#pragma once
#include <cstdint>

constexpr uint32_t kShadeGbuf  = 1u << 0;   // SPEC §15.1: the PrimaryRayPass form (bounce-0 shading + G-buffer + motion)
constexpr uint32_t kShadeEnv   = 1u << 1;   // SPEC §18: next-event estimation samples the probe's distribution
constexpr uint32_t kShadePunct = 1u << 2;   // SPEC §19: the scene has punctual lights
constexpr uint32_t kShadeTrans = 1u << 3;   // SPEC §21: a transmissive material is in use
constexpr uint32_t kShadeEmis  = 1u << 4;   // SPEC §22: an emissive material is in use
constexpr uint32_t kShadeEsamp = 1u << 5;   // SPEC §23: emitter sampling is on and the scene has an emitter distribution; only with EMIS
constexpr uint32_t kShadeNmap  = 1u << 6;   // SPEC §24: a normal-mapped material is in use
constexpr uint32_t kShadeForms = 1u << 7, kPathForms = 1u << 3;   // the words a launcher walks: [0, kShadeForms) / [0, kPathForms)

// the k_shade instantiations that exist: 96 of the 128 words
constexpr bool shade_form_valid(uint32_t form) { return form < kShadeForms && (!(form & kShadeEsamp) || (form & kShadeEmis)); }
// the k_path instantiations that exist (each with STATS off and on): TRANS, EMIS and NMAP keep a wavefront off the path kernel (launch_plan.h)
constexpr bool path_form_valid(uint32_t form) { return form < kPathForms; }

// Waves per SIMD (amdgpu_waves_per_eu), from the compiler's register report: the forms of every frame before the features fit 128 VGPRs and run at 4 (k_shade: DESIGN §5.2;
// k_path spills 15 dwords per lane there and is still faster); every feature's forms need more and run at 3 (168 VGPRs), where they do not spill
// (ENV §5.2a, PUNCT §5.2b, TRANS §5.2d, EMIS §5.2e, ESAMP §5.2f, NMAP §5.2g)
constexpr int shade_waves(uint32_t form) { return (form & ~kShadeGbuf) ? 3 : 4; }
constexpr int path_waves(uint32_t form) { return (form & ~kShadeGbuf) ? 3 : 4; }

// Whether the form's k_shade issues a hit's first loads together (kernels.h shade_hit_early).  All but six words do: with GBUF | TRANS | EMIS | ESAMP and
// ENV or NMAP on top (59, 63, 121, 123, 125, 127) the loop would move one or two more scalars through VGPR lanes than it does, so those keep shade_hit, every load in
// its branch, and are the kernels they were.  k_path keeps shade_hit in every form (no register to spare, and its LDS is budgeted per wave).
constexpr bool shade_early(uint32_t form) {
    constexpr uint32_t full = kShadeGbuf | kShadeTrans | kShadeEmis | kShadeEsamp;
    return !((form & full) == full && (form & (kShadeEnv | kShadeNmap)));
}
