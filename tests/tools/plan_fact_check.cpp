// Test-only driver of loupiote_amd/csrc/launch_plan.h for the facts that only take launches away — `plan_fact_check emis | nmap | lens` (SPEC §22, §24, §25;
// tests/test_emissive.py, tests/test_normal_map.py, tests/test_lens.py).  Over a grid of ray counts, facts and knobs it plans every case with the fact off and with the
// fact on and checks, field for field, that the fact off gives the plan of the rules without the field, and that the fact on removes exactly what the table in
// launch_plan.h says — emis, nmap: the path kernel (path, path_blocks); lens: packets and the path kernel (packet, path, their grids, packet_lds, quad_slots) — and
// changes nothing else of the plan.  Each fact's grid holds the facts that came before it (emis: 7 flag bits; nmap: + emis; lens: + nmap and the packet knob).
// Prints a summary; a non-zero exit status names the first difference.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../loupiote_amd/csrc/launch_plan.h"

struct Fact { const char *name; bool WavefrontFacts::*field; int flag_bits; bool packet_knob, removes_packet; uint32_t bit; };   // bit: what the fact sets in the k_shade forms
static const Fact kFacts[] = {{"emis", &WavefrontFacts::emis, 7, false, false, kShadeEmis}, {"nmap", &WavefrontFacts::nmap, 8, false, false, kShadeNmap}, {"lens", &WavefrontFacts::lens, 9, true, true, 0u}};

// every field none of these facts may move; of the shading forms, `own` is the one bit the fact sets in shade_form and shade_form0 (0: none), path_form apart (same_path)
static bool same_rest(const LaunchPlan &a, const LaunchPlan &b, uint32_t own = 0u) {
    return (a.shade_form | own) == (b.shade_form | own) && (a.shade_form0 | own) == (b.shade_form0 | own) && a.variant == b.variant && a.pipe == b.pipe && a.coop_all == b.coop_all && a.occ_probe == b.occ_probe && a.stats_lds_pad == b.stats_lds_pad && a.tail == b.tail &&
           a.budget == b.budget && a.trace_waves == b.trace_waves && a.stream_blocks == b.stream_blocks && a.shade_blocks == b.shade_blocks && a.trace_blocks == b.trace_blocks &&
           a.coop_blocks == b.coop_blocks && a.stack_lds == b.stack_lds;
}
static bool same_packet(const LaunchPlan &a, const LaunchPlan &b) { return a.packet == b.packet && a.packet_blocks == b.packet_blocks && a.packet_lds == b.packet_lds && a.quad_slots == b.quad_slots; }
static bool same_path(const LaunchPlan &a, const LaunchPlan &b) { return a.path == b.path && a.path_blocks == b.path_blocks && a.path_form == b.path_form; }

int main(int argc, char **argv) {
    const Fact *fact = nullptr;
    for (const Fact &c : kFacts)
        if (argc == 2 && !std::strcmp(argv[1], c.name)) fact = &c;
    if (!fact) {
        std::fprintf(stderr, "usage: plan_fact_check emis | nmap | lens\n");
        return 2;
    }
    unsigned cases = 0, with_path = 0, with_packet = 0, with_quads = 0;
    for (uint32_t n_rays : {64u, 2048u, 32000u, 32001u, 115200u, 120000u, 120001u, 1000000u, 8294400u})
        for (int flags = 0; flags < (1 << fact->flag_bits); ++flags)
            for (uint32_t path_rays : {0u, kPathRays, 0x7FFFFFFFu})
                for (uint32_t coop_rays : {0u, kCoopRays})
                    for (uint32_t packet_primary : {0u, 1u, 2u}) {
                        if (!fact->packet_knob && packet_primary != LaunchTuning{}.packet_primary) continue;
                        LaunchTuning t;
                        t.path_rays = path_rays; t.coop_rays = coop_rays; t.packet_primary = packet_primary;
                        WavefrontFacts f;
                        f.n_rays = n_rays; f.n_samples = (flags & 64) ? 4u : 1u; f.n_slots = n_rays / f.n_samples; f.cus = 256u;
                        f.solo = flags & 1; f.stats = flags & 2; f.denoise = flags & 4; f.masked = flags & 8; f.trans = flags & 16; f.punct = flags & 32; f.env = flags & 64;
                        f.emis = flags & 128; f.nmap = flags & 256;
                        f.max_depth = 12u; f.stack_entries = 13u; f.pixel_rad = (flags & 4) ? 0.001f : 0.02f; f.dense = true; f.block8 = true;
                        f.lim = KernelLimits{256u, 64u, 8u, 32u, 128u, 0.0018f};
                        const LaunchPlan off = plan_wavefront(t, f);   // the fact is false by default: the plan of the code before the field
                        WavefrontFacts g = f;
                        g.*(fact->field) = false;
                        const LaunchPlan off2 = plan_wavefront(t, g);
                        g.*(fact->field) = true;
                        const LaunchPlan on = plan_wavefront(t, g);
                        ++cases;
                        with_path += off.path ? 1u : 0u; with_packet += off.packet ? 1u : 0u; with_quads += off.quad_slots ? 1u : 0u;
                        // the rules without the field
                        const auto other = [&](bool WavefrontFacts::*m) { return m != fact->field && f.*m; };
                        const bool expect_packet = !f.masked && !other(&WavefrontFacts::lens) && (packet_primary == 1u || (packet_primary == 2u && f.pixel_rad <= f.lim.kPacketMaxPixelRad));
                        const bool expect_path = !f.masked && !f.trans && !other(&WavefrontFacts::emis) && !other(&WavefrontFacts::nmap) && !other(&WavefrontFacts::lens) && t.path_rays &&
                                                 n_rays <= t.path_rays && !off.coop_all;
                        if (off.packet != expect_packet || off.path != expect_path || !same_packet(off, off2) || !same_path(off, off2) || !same_rest(off, off2)) {
                            std::fprintf(stderr, "%s = false does not reproduce the plan: n_rays %u flags %d path_rays %u coop_rays %u packet_primary %u\n", fact->name, n_rays, flags, path_rays, coop_rays, packet_primary);
                            return 1;
                        }
                        const bool packet_ok = fact->removes_packet ? (!on.packet && on.packet_blocks == 0u && on.packet_lds == 0u && on.quad_slots == 0u) : same_packet(off, on);
                        const bool bit_ok = (on.shade_form & ~off.shade_form) == fact->bit && (on.shade_form0 & ~off.shade_form0) == fact->bit && on.path_form == 0u;
                        if (on.path || on.path_blocks != 0u || !packet_ok || !bit_ok || !same_rest(off, on, fact->bit)) {
                            std::fprintf(stderr, "%s = true: packet %d, path %d, blocks %u / %u, packet_lds %u, quad_slots %u, or another field moved: n_rays %u flags %d path_rays %u coop_rays %u packet_primary %u\n",
                                         fact->name, (int)on.packet, (int)on.path, on.packet_blocks, on.path_blocks, on.packet_lds, on.quad_slots, n_rays, flags, path_rays, coop_rays, packet_primary);
                            return 1;
                        }
                    }
    std::printf("{\"cases\": %u, \"with_path\": %u, \"with_packet\": %u, \"with_quads\": %u}\n", cases, with_path, with_packet, with_quads);
    return 0;
}
