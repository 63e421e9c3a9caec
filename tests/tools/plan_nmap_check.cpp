// Test-only driver of loupiote_amd/csrc/launch_plan.h for WavefrontFacts::nmap (SPEC §24; tests/test_normal_map.py): over a grid of facts and knobs — emis among
// them now — it plans every case with nmap = false and with nmap = true and checks, field for field, that nmap = true gives path == false (and no path grid) and
// changes nothing else of the plan, and that nmap = false gives the plan of the facts without the field.
// Prints a summary; a non-zero exit status names the first difference.
#include <cstdio>
#include <initializer_list>

#include "../../loupiote_amd/csrc/launch_plan.h"

static bool same_but_path(const LaunchPlan &a, const LaunchPlan &b) {
    return a.variant == b.variant && a.pipe == b.pipe && a.packet == b.packet && a.coop_all == b.coop_all && a.occ_probe == b.occ_probe && a.stats_lds_pad == b.stats_lds_pad &&
           a.quad_slots == b.quad_slots && a.tail == b.tail && a.budget == b.budget && a.trace_waves == b.trace_waves && a.stream_blocks == b.stream_blocks &&
           a.shade_blocks == b.shade_blocks && a.trace_blocks == b.trace_blocks && a.coop_blocks == b.coop_blocks && a.packet_blocks == b.packet_blocks &&
           a.stack_lds == b.stack_lds && a.packet_lds == b.packet_lds;
}

int main() {
    unsigned cases = 0, with_path = 0;
    for (uint32_t n_rays : {64u, 2048u, 32000u, 32001u, 115200u, 120000u, 120001u, 1000000u, 8294400u})
        for (int flags = 0; flags < 256; ++flags)
            for (uint32_t path_rays : {0u, kPathRays, 0x7FFFFFFFu})
                for (uint32_t coop_rays : {0u, kCoopRays}) {
                    LaunchTuning t;
                    t.path_rays = path_rays; t.coop_rays = coop_rays;
                    WavefrontFacts f;
                    f.n_rays = n_rays; f.n_samples = (flags & 64) ? 4u : 1u; f.n_slots = n_rays / f.n_samples; f.cus = 256u;
                    f.solo = flags & 1; f.stats = flags & 2; f.denoise = flags & 4; f.masked = flags & 8; f.trans = flags & 16; f.punct = flags & 32; f.env = flags & 64; f.emis = flags & 128;
                    f.max_depth = 12u; f.stack_entries = 13u; f.pixel_rad = (flags & 4) ? 0.001f : 0.02f; f.dense = true; f.block8 = true;
                    f.lim = KernelLimits{256u, 64u, 8u, 32u, 128u, 0.0018f};
                    const LaunchPlan off = plan_wavefront(t, f);   // nmap = false is the default: the plan of the code before the flag
                    WavefrontFacts g = f;
                    g.nmap = false;
                    const LaunchPlan off2 = plan_wavefront(t, g);
                    g.nmap = true;
                    const LaunchPlan on = plan_wavefront(t, g);
                    ++cases;
                    with_path += off.path ? 1u : 0u;
                    const bool expect_path = !f.masked && !f.trans && !f.emis && t.path_rays && n_rays <= t.path_rays && !off.coop_all;   // the rule without nmap
                    if (off.path != expect_path || off.path != off2.path || off.path_blocks != off2.path_blocks || !same_but_path(off, off2)) {
                        std::fprintf(stderr, "nmap = false does not reproduce the plan: n_rays %u flags %d path_rays %u coop_rays %u\n", n_rays, flags, path_rays, coop_rays);
                        return 1;
                    }
                    if (on.path || on.path_blocks != 0u || !same_but_path(off, on)) {
                        std::fprintf(stderr, "nmap = true: path %d, path_blocks %u, or another field moved: n_rays %u flags %d path_rays %u coop_rays %u\n", (int)on.path, on.path_blocks, n_rays,
                                     flags, path_rays, coop_rays);
                        return 1;
                    }
                }
    std::printf("{\"cases\": %u, \"with_path\": %u}\n", cases, with_path);
    return 0;
}
