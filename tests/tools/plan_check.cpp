// Test-only driver of loupiote_amd/csrc/launch_plan.h (tests/test_launch_plan.py): one case per line of stdin, or one case from argv, as `name=value` words —
// the fields of LaunchTuning, WavefrontFacts and KernelLimits by their names; what is not named keeps its default.  Prints one JSON object per case: the plan, its k_trace
// form as the bit string of the eight k_trace instantiations ("none" for k_trace_glass) and by its name in TraceVariant, its shading forms as words (kernel_forms.h).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../loupiote_amd/csrc/launch_plan.h"

static bool set_field(LaunchTuning &t, WavefrontFacts &f, const std::string &k, const std::string &v) {
    const unsigned long long u = std::strtoull(v.c_str(), nullptr, 0);
#define U32(S, N) if (k == #N) { S.N = (uint32_t)u; return true; }
#define INT(S, N) if (k == #N) { S.N = (int)std::strtol(v.c_str(), nullptr, 0); return true; }
#define FLAG(S, N) if (k == #N) { S.N = u != 0; return true; }
    U32(t, packet_primary) U32(t, pipe_rays) U32(t, path_rays) U32(t, path_waves_per_cu) INT(t, path_refill) INT(t, refill)
    U32(t, shade_blocks_per_cu) U32(t, trace_waves_per_cu) U32(t, step_budget) U32(t, budget_rays) FLAG(t, budget_split)
    U32(t, tail_lanes) U32(t, coop_rays) FLAG(t, packet_quads)
    U32(f, n_rays) U32(f, n_slots) U32(f, slot0) U32(f, n_samples) U32(f, cus) FLAG(f, solo) FLAG(f, stats) FLAG(f, denoise)
    FLAG(f, masked) FLAG(f, trans) FLAG(f, punct) FLAG(f, env) FLAG(f, emis) FLAG(f, esamp) FLAG(f, nmap) FLAG(f, lens) FLAG(f, glass_shadow) U32(f, max_depth) U32(f, stack_entries) FLAG(f, dense) FLAG(f, block8)
    U32(f.lim, kBlock) U32(f.lim, kTraceBlock) U32(f.lim, kTailMax) U32(f.lim, kCoopWavesPerCu) U32(f.lim, kPacketBlocksPerCu)
#undef U32
#undef INT
#undef FLAG
    if (k == "pixel_rad") { f.pixel_rad = std::strtof(v.c_str(), nullptr); return true; }
    if (k == "kPacketMaxPixelRad") { f.lim.kPacketMaxPixelRad = std::strtof(v.c_str(), nullptr); return true; }
    return false;
}

static std::string to_json(const LaunchPlan &p) {
    static const char *const kVariant[] = {"0000", "0100", "1000", "1100", "0010", "0110", "0001", "1001"};   // (STATS, PIPE, TAIL, MASK), in TraceVariant's order: the k_trace instantiations
    static const char *const kName[] = {"Lane", "Pipe", "Stats", "StatsPipe", "Tail", "PipeTail", "Mask", "StatsMask", "Glass", "StatsGlass"};   // TraceVariant's order
    const unsigned vi = (unsigned)p.variant;
    char buf[1024];
    std::snprintf(buf, sizeof buf, "{\"variant\": \"%s\", \"variant_name\": \"%s\", \"variant_index\": %u, \"shade_form\": %u, \"shade_form0\": %u, \"path_form\": %u, \"pipe\": %d, \"packet\": %d, \"coop_all\": %d, \"path\": %d, \"occ_probe\": %d, \"stats_lds_pad\": %d, \"quad_slots\": %u, \"tail\": %u, "
                  "\"budget\": %u, \"trace_waves\": %u, \"stream_blocks\": %u, \"shade_blocks\": %u, \"trace_blocks\": %u, \"coop_blocks\": %u, \"packet_blocks\": %u, \"path_blocks\": %u, "
                  "\"stack_lds\": %u, \"packet_lds\": %u",
                  vi < 8u ? kVariant[vi] : "none", vi < 10u ? kName[vi] : "none", vi, p.shade_form, p.shade_form0, p.path_form, p.pipe, p.packet, p.coop_all, p.path, p.occ_probe, p.stats_lds_pad, p.quad_slots, p.tail,
                  p.budget, p.trace_waves, p.stream_blocks, p.shade_blocks, p.trace_blocks, p.coop_blocks, p.packet_blocks, p.path_blocks, p.stack_lds, p.packet_lds);
    return buf;
}

static int run_case(const std::string &line) {
    LaunchTuning t;
    WavefrontFacts f;
    std::istringstream in(line);
    std::string word;
    while (in >> word) {
        const size_t eq = word.find('=');
        if (eq == std::string::npos || !set_field(t, f, word.substr(0, eq), word.substr(eq + 1))) {
            std::fprintf(stderr, "plan_check: bad word '%s'\n", word.c_str());
            return 2;
        }
    }
    const std::string once = to_json(plan_wavefront(t, f)), again = to_json(plan_wavefront(t, f));   // a pure function: the same input, the same plan
    std::printf("%s, \"same_again\": %d}\n", once.c_str(), once == again ? 1 : 0);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) {
        std::string line;
        for (int i = 1; i < argc; ++i) line += std::string(argv[i]) + " ";
        return run_case(line);
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const int st = run_case(line);
        if (st) return st;
    }
    return 0;
}
