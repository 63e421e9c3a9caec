// How one submission (the recorded raytrace() calls of a renderer) leaves for the GPU: where the batch is cut into wavefronts ("pieces"), which lane and which
// ticket every piece takes, and the order in which the pieces' halves and stages are enqueued with the events they wait for and record — one host-side decision
// (plan_submission) that device.hip's flush_pending walks step by step.  Plain C++17, nothing from HIP: tests/tools/submission_check.cpp compiles it with g++ and
// tests/test_submission_plan.py checks the rules below on a CPU.  Every plan gives the same frame bit for bit; the level below (which kernels a piece runs) is launch_plan.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

// What the decision depends on: the rank's share of the frame, the recorded batch, the renderer's knobs
struct SubmissionFacts {
    uint32_t n_slots = 0, tiles_x = 0, tile_w = 0, tile_h = 0, world = 1, height = 0;   // the rank's pixel slots (whole tiles), the tiling, the frame's height
    uint32_t n = 1;                  // recorded calls = samples per slot (at least 1)
    uint32_t max_fused = 0;          // >= 1: the caller set the batch size (lpt_renderer_set_max_fused, lpt_renderer_raytrace_n)
    bool pathtrace = true;           // the mode is Pathtrace; the denoising modes carry frame-to-frame state
    uint64_t wavefront_rays = 0, split_rays = 0;   // LPT_OPT_WAVEFRONT_RAYS, LPT_EXP_SPLIT_RAYS
    uint32_t n_lanes = 1, lane_phase = 0, bounces = 0;   // lpt_renderer_set_lanes, LPT_EXP_LANE_PHASE, the bounce count nb
    uint32_t lane_rr = 0;            // the renderer's round-robin lane counter before this submission
    bool read = false;               // a read-back came with the flush (lpt_renderer_read_radiance, lpt_renderer_blit_rgba8)
};

// One wavefront of the submission: the rank's slots [slot0, slot0 + n_slots) with all the recorded samples
struct SubmissionPiece {
    uint32_t slot0 = 0, n_slots = 0;
    uint32_t row0 = 0, row1 = 0;     // the pixel rows the piece completes: set for the early read-back alone (world == 1, Pathtrace, a read-back present), else empty
    uint32_t lane = 0, ticket = 0;   // the Wavefront (buffers, stream) it runs in / the Ticket that carries it between its two halves
    bool solo = false;               // the submission is this one wavefront (launch_plan.h WavefrontFacts::solo)
};

// The traversal event trav[stage] of `piece`'s lane; piece < 0: none
struct TravEvent { int32_t piece = -1; uint32_t stage = 0; };

struct SubmissionStep {
    enum Kind : uint8_t { Prepare, Stage, Finish } kind = Prepare;
    uint32_t piece = 0;
    // Stage alone: stage t of the piece's launches (0: counters, ray generation, the primary rays; b + 1: shade(b) and the traversal behind it); the events it waits for
    // before its first launch / before its traversal launch; whether trav[t] of its lane is recorded behind it
    uint32_t t = 0;
    TravEvent wait_start, wait_trav;
    bool record = false;
};

struct SubmissionPlan {
    std::vector<SubmissionPiece> pieces;
    std::vector<SubmissionStep> steps;
    uint32_t lane_rr = 0;        // the counter to store back
    uint32_t trav_events = 0;    // traversal events every piece's lane must own before the steps are walked (0: no stage records one)
};

// The rules (the expressions below are their only statement in code):
//
//   what                  | rule                                                                                  | why, measured
//   ----------------------+---------------------------------------------------------------------------------------+----------------------------------------------
//   granule               | world == 1: a tile row (the rank's slots are the tiles in row-major order, so a run of  | the early read-back copies whole pixel rows
//                         | granules is a run of pixel rows); else one tile                                        |
//   one piece             | an explicit batch size (max_fused >= 1), a denoising mode, a single granule, or a batch | a denoising frame is one temporal pass
//                         | of at most wavefront_rays rays that is not split (next row)                            |
//   split                 | more than one lane and more than split_rays (3 M) rays: at least two pieces although    | 1/2 shard of the headline frame (4.15 M rays)
//                         | one wavefront would hold them                                                           | 7.22 -> 6.81 ms; a 1/4 shard (2 x 1.04 M) 4.62 ->
//                         |                                                                                         | 4.75: below 3 M the halves are too small to hide
//                         |                                                                                         | each other's drains (profiles/r04_experiments_ab.txt E)
//   cut                   | fit = granules of n samples in wavefront_rays (at least 1); pieces = max(2, ceil(granules | 1920x1080, 4 samples: two wavefronts of 4.1 M rays
//                         | / fit)); then the same number of pieces evened out: ceil(granules / pieces) granules     | 13.30 ms per frame, one of 8 M 13.68, four of 2 M
//                         | each, the last one what is left                                                         | 14.1
//   nothing owned         | one empty piece: Prepare and Finish keep the bookkeeping of the call (a compositor rank) |
//   lane                  | a denoising mode or a single lane: 0.  Else the pieces take the lanes in turn, across    | the shading of one piece overlaps the traversal
//                         | submissions: (lane_rr + k) mod n_lanes                                                  | of the other
//   ahead, ticket         | ahead = n_lanes (1 for a denoising mode or a single lane); ticket = k mod ahead          |
//   Finish(k - ahead)     | comes before Prepare(k): it is the piece that used k's lane and ticket, whose buffers k   | the first halves run ahead of the second halves
//                         | overwrites — and the accumulation and read-back copy of a piece (the copy blocks the host | by the number of lanes
//                         | when the destination is pageable) are not enqueued before the next pieces' launches     |
//   phase                 | lane_phase, but 0 with one lane (or a denoising mode) or one piece                      | LPT_EXP_LANE_PHASE
//   phase 0 (free)        | Prepare(k), Stage(k, 0 .. nb) without waits or records, piece by piece                  | the bench frame 10.52-10.53 ms
//   phase 1, 2            | the pieces leave in groups of `ahead` (side by side on the lanes): Prepare of every       | an event must be recorded before it is waited
//                         | member; then stage t of every member before stage t + 1 of any.  Every stage records    | for: hipStreamWaitEvent on an event not yet
//                         | trav[t] of its lane                                                                    | recorded does not wait
//   phase 1 (offset start)| stage 0 of a member but the group's first waits, before its first launch, for trav[0] of | the bench frame 10.44-10.47 ms: the default
//                         | the member before it                                                                   | (profiles/r08_lane_phase_ab.txt)
//   phase 2 (alternating  | the traversal launch of stage t of a member but the first waits for trav[t] of the       | 11.87 ms: one traversal grid at a time holds the
//   traversal)            | member before it; the first member's, for t > 0, for trav[t - 1] of the group's last    | chip and the other pieces shade beside it — which
//                         | member                                                                                 | gives up more than the shading beside it wins
//   the end               | Finish of the last `ahead` pieces, in order                                             |
//
// f.n >= 1: a submission has at least one recorded call.
inline SubmissionPlan plan_submission(const SubmissionFacts &f) {
    const auto div_up = [](uint32_t a, uint32_t b) { return (a + b - 1u) / b; };
    using Step = SubmissionStep;
    SubmissionPlan pl;
    pl.lane_rr = f.lane_rr;
    const bool laned = f.pathtrace && f.n_lanes > 1u;
    const auto add_piece = [&](uint32_t slot0, uint32_t n_slots, uint32_t row0, uint32_t row1, uint32_t ticket, bool solo) {
        pl.pieces.push_back(SubmissionPiece{slot0, n_slots, row0, row1, laned ? pl.lane_rr++ % f.n_lanes : 0u, ticket, solo});
    };
    const auto step = [&](Step::Kind kind, uint32_t k) { Step s; s.kind = kind; s.piece = k; pl.steps.push_back(s); };

    const uint32_t area = f.tile_w * f.tile_h;
    const bool whole_rows = f.world == 1u;
    const uint32_t granule = whole_rows ? f.tiles_x * area : area;
    const uint32_t granules = granule ? f.n_slots / granule : 0u;
    if (!granules) {
        add_piece(0u, 0u, 0u, 0u, 0u, true);
        step(Step::Prepare, 0u);
        step(Step::Finish, 0u);
        return pl;
    }
    uint32_t per_piece = granules;
    const uint64_t total = (uint64_t)f.n_slots * f.n;
    if (!f.max_fused && f.pathtrace && granules > 1u && (total > f.wavefront_rays || (f.split_rays && total > f.split_rays && f.n_lanes > 1u))) {
        const uint64_t fit = f.wavefront_rays / ((uint64_t)granule * f.n);
        const uint32_t pieces = std::max(2u, div_up(granules, (uint32_t)std::max<uint64_t>(fit, 1u)));
        per_piece = div_up(granules, pieces);
    }
    const uint32_t pieces = div_up(granules, per_piece);
    const bool early = f.read && whole_rows && f.pathtrace;
    const uint32_t ahead = laned ? f.n_lanes : 1u;
    for (uint32_t k = 0; k < pieces; ++k) {
        const uint32_t g0 = k * per_piece, g1 = std::min(granules, g0 + per_piece);
        add_piece(g0 * granule, (g1 - g0) * granule, early ? std::min(f.height, g0 * f.tile_h) : 0u, early ? std::min(f.height, g1 * f.tile_h) : 0u, k % ahead, pieces == 1u);
    }

    const uint32_t phase = (ahead > 1u && pieces > 1u) ? f.lane_phase : 0u;
    const uint32_t group = phase ? ahead : 1u, stages = f.bounces + 1u;
    pl.trav_events = phase ? stages : 0u;
    for (uint32_t k0 = 0; k0 < pieces; k0 += group) {
        const uint32_t k1 = std::min(pieces, k0 + group);
        for (uint32_t k = k0; k < k1; ++k) {
            if (k >= ahead) step(Step::Finish, k - ahead);
            step(Step::Prepare, k);
        }
        for (uint32_t t = 0; t < stages; ++t)
            for (uint32_t k = k0; k < k1; ++k) {
                Step s;
                s.kind = Step::Stage; s.piece = k; s.t = t;
                if (phase) {
                    const int32_t prev = (int32_t)(k > k0 ? k - 1u : k1 - 1u);
                    s.record = true;
                    if (phase == 1u && t == 0u && k > k0) s.wait_start = TravEvent{prev, 0u};
                    if (phase == 2u && k > k0) s.wait_trav = TravEvent{prev, t};
                    if (phase == 2u && k == k0 && t > 0u) s.wait_trav = TravEvent{prev, t - 1u};
                }
                pl.steps.push_back(s);
            }
    }
    for (uint32_t k = pieces > ahead ? pieces - ahead : 0u; k < pieces; ++k) step(Step::Finish, k);
    return pl;
}
