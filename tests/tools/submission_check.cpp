// Test-only driver of loupiote_amd/csrc/submission_plan.h (tests/test_submission_plan.py): one case per line of stdin, or one case from argv, as `name=value` words —
// the fields of SubmissionFacts by their names; what is not named keeps its default.  Prints one JSON object per case: the plan.
//   pieces: [slot0, n_slots, row0, row1, lane, ticket, solo]
//   steps:  ["P", k] | ["F", k] | ["S", k, t, wait_start, wait_trav, record] with a wait as [piece, stage] or null
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../loupiote_amd/csrc/submission_plan.h"

static bool set_field(SubmissionFacts &f, const std::string &k, const std::string &v) {
    const unsigned long long u = std::strtoull(v.c_str(), nullptr, 0);
#define U32(N) if (k == #N) { f.N = (uint32_t)u; return true; }
#define U64(N) if (k == #N) { f.N = (uint64_t)u; return true; }
#define FLAG(N) if (k == #N) { f.N = u != 0; return true; }
    U32(n_slots) U32(tiles_x) U32(tile_w) U32(tile_h) U32(world) U32(height) U32(n) U32(max_fused) FLAG(pathtrace)
    U64(wavefront_rays) U64(split_rays) U32(n_lanes) U32(lane_phase) U32(bounces) U32(lane_rr) FLAG(read)
#undef U32
#undef U64
#undef FLAG
    return false;
}

static std::string wait_json(const TravEvent &e) {
    return e.piece < 0 ? "null" : "[" + std::to_string(e.piece) + ", " + std::to_string(e.stage) + "]";
}

static std::string to_json(const SubmissionPlan &p) {
    std::string s = "{\"lane_rr\": " + std::to_string(p.lane_rr) + ", \"trav_events\": " + std::to_string(p.trav_events) + ", \"pieces\": [";
    for (size_t i = 0; i < p.pieces.size(); ++i) {
        const SubmissionPiece &c = p.pieces[i];
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s[%u, %u, %u, %u, %u, %u, %d]", i ? ", " : "", c.slot0, c.n_slots, c.row0, c.row1, c.lane, c.ticket, (int)c.solo);
        s += buf;
    }
    s += "], \"steps\": [";
    for (size_t i = 0; i < p.steps.size(); ++i) {
        const SubmissionStep &t = p.steps[i];
        if (i) s += ", ";
        if (t.kind == SubmissionStep::Stage)
            s += "[\"S\", " + std::to_string(t.piece) + ", " + std::to_string(t.t) + ", " + wait_json(t.wait_start) + ", " + wait_json(t.wait_trav) + ", " + (t.record ? "1" : "0") + "]";
        else
            s += std::string(t.kind == SubmissionStep::Prepare ? "[\"P\", " : "[\"F\", ") + std::to_string(t.piece) + "]";
    }
    return s + "]";
}

static int run_case(const std::string &line) {
    SubmissionFacts f;
    std::istringstream in(line);
    std::string word;
    while (in >> word) {
        const size_t eq = word.find('=');
        if (eq == std::string::npos || !set_field(f, word.substr(0, eq), word.substr(eq + 1))) {
            std::fprintf(stderr, "submission_check: bad word '%s'\n", word.c_str());
            return 2;
        }
    }
    if (!f.n) {
        std::fprintf(stderr, "submission_check: n must be at least 1\n");
        return 2;
    }
    const std::string once = to_json(plan_submission(f)), again = to_json(plan_submission(f));   // a pure function: the same input, the same plan
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
