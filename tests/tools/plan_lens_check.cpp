// Test-only driver of loupiote_amd/csrc/launch_plan.h for WavefrontFacts::lens (SPEC §25; tests/test_lens.py): over the grid of facts and knobs of plan_nmap_check.cpp —
// nmap and the packet knob among them now — it plans every case with lens = false and with lens = true and checks, field for field, that lens = true gives packet == false
// and path == false with zero packet_blocks, path_blocks, packet_lds and quad_slots and changes nothing else of the plan, and that lens = false gives the plan of the facts
// without the field.  Prints a summary; a non-zero exit status names the first difference.
#include <cstdio>
#include <initializer_list>

#include "../../loupiote_amd/csrc/launch_plan.h"

// every field the lens must leave alone
static bool same_rest(const LaunchPlan &a, const LaunchPlan &b) {
    return a.variant == b.variant && a.pipe == b.pipe && a.coop_all == b.coop_all && a.occ_probe == b.occ_probe && a.stats_lds_pad == b.stats_lds_pad && a.tail == b.tail &&
           a.budget == b.budget && a.trace_waves == b.trace_waves && a.stream_blocks == b.stream_blocks && a.shade_blocks == b.shade_blocks && a.trace_blocks == b.trace_blocks &&
           a.coop_blocks == b.coop_blocks && a.stack_lds == b.stack_lds;
}
static bool same_primary(const LaunchPlan &a, const LaunchPlan &b) {
    return a.packet == b.packet && a.path == b.path && a.packet_blocks == b.packet_blocks && a.path_blocks == b.path_blocks && a.packet_lds == b.packet_lds && a.quad_slots == b.quad_slots;
}

int main() {
    unsigned cases = 0, with_path = 0, with_packet = 0, with_quads = 0;
    for (uint32_t n_rays : {64u, 2048u, 32000u, 32001u, 115200u, 120000u, 120001u, 1000000u, 8294400u})
        for (int flags = 0; flags < 512; ++flags)
            for (uint32_t path_rays : {0u, kPathRays, 0x7FFFFFFFu})
                for (uint32_t coop_rays : {0u, kCoopRays})
                    for (uint32_t packet_primary : {0u, 1u, 2u}) {
                        LaunchTuning t;
                        t.path_rays = path_rays; t.coop_rays = coop_rays; t.packet_primary = packet_primary;
                        WavefrontFacts f;
                        f.n_rays = n_rays; f.n_samples = (flags & 64) ? 4u : 1u; f.n_slots = n_rays / f.n_samples; f.cus = 256u;
                        f.solo = flags & 1; f.stats = flags & 2; f.denoise = flags & 4; f.masked = flags & 8; f.trans = flags & 16; f.punct = flags & 32; f.env = flags & 64; f.emis = flags & 128;
                        f.nmap = flags & 256;
                        f.max_depth = 12u; f.stack_entries = 13u; f.pixel_rad = (flags & 4) ? 0.001f : 0.02f; f.dense = true; f.block8 = true;
                        f.lim = KernelLimits{256u, 64u, 8u, 32u, 128u, 0.0018f};
                        const LaunchPlan off = plan_wavefront(t, f);   // lens = false is the default: the plan of the code before the field
                        WavefrontFacts g = f;
                        g.lens = false;
                        const LaunchPlan off2 = plan_wavefront(t, g);
                        g.lens = true;
                        const LaunchPlan on = plan_wavefront(t, g);
                        ++cases;
                        with_path += off.path ? 1u : 0u; with_packet += off.packet ? 1u : 0u; with_quads += off.quad_slots ? 1u : 0u;
                        // the rules without the field
                        const bool expect_packet = !f.masked && (packet_primary == 1u || (packet_primary == 2u && f.pixel_rad <= f.lim.kPacketMaxPixelRad));
                        const bool expect_path = !f.masked && !f.trans && !f.emis && !f.nmap && t.path_rays && n_rays <= t.path_rays && !off.coop_all;
                        if (off.packet != expect_packet || off.path != expect_path || !same_primary(off, off2) || !same_rest(off, off2)) {
                            std::fprintf(stderr, "lens = false does not reproduce the plan: n_rays %u flags %d path_rays %u coop_rays %u packet_primary %u\n", n_rays, flags, path_rays, coop_rays, packet_primary);
                            return 1;
                        }
                        if (on.packet || on.path || on.packet_blocks != 0u || on.path_blocks != 0u || on.packet_lds != 0u || on.quad_slots != 0u || !same_rest(off, on)) {
                            std::fprintf(stderr, "lens = true: packet %d, path %d, blocks %u / %u, packet_lds %u, quad_slots %u, or another field moved: n_rays %u flags %d path_rays %u coop_rays %u packet_primary %u\n",
                                         (int)on.packet, (int)on.path, on.packet_blocks, on.path_blocks, on.packet_lds, on.quad_slots, n_rays, flags, path_rays, coop_rays, packet_primary);
                            return 1;
                        }
                    }
    std::printf("{\"cases\": %u, \"with_path\": %u, \"with_packet\": %u, \"with_quads\": %u}\n", cases, with_path, with_packet, with_quads);
    return 0;
}
