// Which kernels a wavefront runs — the k_trace form by name (TraceVariant), the k_shade and k_path forms as words (kernel_forms.h) — and with which grids: one host-side
// decision (plan_wavefront) that device.hip's wavefront_prepare consumes.  Plain C++17, nothing from HIP: tests/tools/plan_check.cpp compiles it with g++ and
// tests/test_launch_plan.py checks the rules below on a CPU.  Every plan gives the same frame bit for bit.
#pragma once
#include <algorithm>
#include <cstdint>

#include "kernel_forms.h"

constexpr uint32_t kStepBudget = 48u, kBudgetRays = 3000000u;  // defaults of LPT_EXP_STEP_BUDGET / LPT_EXP_BUDGET_RAYS (measured: profiles/r04_experiments_ab.txt H)
constexpr uint32_t kPathRays = 120000u;           // rays of a wavefront up to which the path kernel is used: the measured cross-over against the per-bounce launches with their tails in place
                                                  // (whole frames, ms: 113 k rays 0.913 path / 0.932 per bounce, 147 k 1.07 / 0.99, 332 k 1.89 / 1.40; it was 450 000 against the budget pair)
constexpr uint32_t kCoopRays = 32000u;            // rays of a wavefront up to which EVERY ray is traced by a whole wave (k_trace_coop over the queues): the measured cross-over (28 k rays:
                                                  // 0.755 -> 0.652 ms per frame, 37 k: 0.765 -> 0.787; profiles/r05_experiments_ab.txt V)

// The launch-tuning knobs of a renderer (lpt_renderer_set_option; experiments and the variant tests switch them)
struct LaunchTuning {
    uint32_t packet_primary = 2u;  // bounce 0 by packet traversal (k_trace_packet): 2 = where an 8x8-pixel patch is narrow enough (plan_wavefront), 1 = always, 0 = never (LPT_OPT_PACKET_PRIMARY)
    uint32_t pipe_rays = 0x7FFFFFFFu;   // wavefronts of at most this many rays trace with the one-round-trip step (k_trace<.., PIPE>): all of them; LPT_EXP_PIPE_RAYS 0: none
    // wavefronts of at most this many rays run every bounce behind the primary hits in ONE launch (k_path: no chip-wide barrier per
    // bounce); larger ones take the per-bounce launches, whose drains are then a few per cent.  LPT_OPT_PATH_RAYS; 0: never
    uint32_t path_rays = kPathRays;
    uint32_t path_waves_per_cu = 16;   // k_path: 4 waves per SIMD (kernel_forms.h path_waves)
    int path_refill = 32;              // k_path: a batch of lanes is shaded (and idle lanes start new paths) when at most this many lanes are tracing
    int refill = 44;                   // k_trace: the lanes of a wave refill from the queue when at most this many are tracing (LPT_EXP_REFILL)
    // k_shade grid, blocks per CU (LPT_EXP_SHADE_BLOCKS_PER_CU); 0 = by the submission: 4 (what is resident at 4 waves / SIMD; 8: a 1/8 shard 1.89 instead of 1.80 ms) for a
    // wavefront that has the chip to itself, 3 for the pieces of a cut batch — three 128-VGPR shading waves leave a SIMD room for one 72-VGPR k_trace wave of the piece on the
    // other lane: the kernel alone is 10 % slower (2.75 -> 3.05 ms per frame), the frame 0.5 % faster (11.27-11.29 -> 11.19-11.24; profiles/r06_experiments_ab.txt O)
    uint32_t shade_blocks_per_cu = 0;
    uint32_t trace_waves_per_cu = 0;  // 0 = sized from the wavefront's ray count (plan_wavefront); LPT_EXP_TRACE_WAVES_PER_CU pins it
    // per-bounce traversal launches: a ray that is not finished after this many steps is handed to k_trace_coop (a whole wave per ray); 0 = off.
    // Applies to wavefronts of at most `budget_rays` rays: where a launch's longest ray sets its duration
    uint32_t step_budget = kStepBudget, budget_rays = kBudgetRays;
    bool budget_split = false;     // the budget also for the pieces of a cut batch (LPT_EXP_BUDGET_SPLIT)
    // the same launches' tails finished IN PLACE instead (kernels.h tail_park / tail_walk): a wave whose queues are dry and that is down to this many live rays finishes them
    // cooperatively from where they stand (default); 0: off (then the step budget + k_trace_coop pair applies).  LPT_OPT_TAIL_LANES
    uint32_t tail_lanes = 4u;      // 1/8 shard of the bench frame: 3, 4, 5 the same (2.74 ms per frame against 2.90 with the budget pair), 2 and 8 slower
    uint32_t coop_rays = kCoopRays;   // LPT_OPT_COOP_RAYS
    bool packet_quads = true;      // a packet of bounce 0 = the four samples of a 4x4-pixel quarter (where the queue order allows it) instead of one sample of an 8x8 patch (LPT_EXP_PACKET_QUADS)
};

// The kernels' constants the arithmetic needs (kernels.h and device.hip own them; this header includes neither)
struct KernelLimits { uint32_t kBlock, kTraceBlock, kTailMax, kCoopWavesPerCu, kPacketBlocksPerCu; float kPacketMaxPixelRad; };

// What a decision depends on besides the knobs: the wavefront, the renderer's modes, the bound scene, probe and tree
struct WavefrontFacts {
    uint32_t n_rays = 0, n_slots = 0, slot0 = 0, n_samples = 0;   // n_rays = n_slots * n_samples
    uint32_t cus = 0;                 // the device's compute units
    bool solo = false;                // the submission is this ONE wavefront (not a piece of a cut batch)
    bool stats = false, denoise = false;
    bool masked = false, trans = false, punct = false, env = false;   // SPEC §20, §21, §19, §18
    bool emis = false;                // SPEC §22: an emissive material is in use
    bool esamp = false;               // SPEC §23: the renderer's switch is on, `emis`, and the scene has an emitter distribution
    bool nmap = false;                // SPEC §24: a normal-mapped material is in use
    bool lens = false;                // SPEC §25: the renderer's lens is open (R > 0): every primary ray has an origin of its own
    bool glass_shadow = false;        // SPEC §27: the renderer's switch is on, the scene has punctual lights and a thin-walled transmissive triangle
    uint32_t max_depth = 0, stack_entries = 0;   // the tree's depth / per-lane stack capacity
    float pixel_rad = 0.0f;           // angle per pixel (2 tan(vfov / 2) / height)
    bool dense = false, block8 = false;   // whole tiles only / 8x8-pixel blocks inside the tiles
    KernelLimits lim{};
};

// the k_trace instantiations that exist: (STATS, PIPE, TAIL, MASK) = 0000 0100 1000 1100 0010 0110 0001 1001; behind them k_trace_glass<STATS> (SPEC §27)
enum class TraceVariant : uint8_t { Lane, Pipe, Stats, StatsPipe, Tail, PipeTail, Mask, StatsMask, Glass, StatsGlass };

struct LaunchPlan {
    TraceVariant variant = TraceVariant::Lane;
    uint32_t shade_form = 0, shade_form0 = 0;   // k_shade<FORM> of the bounces >= 1 / of bounce 0 (kernel_forms.h)
    uint32_t path_form = 0;                     // k_path<FORM, stats> where `path`, else 0
    bool pipe = false, packet = false, coop_all = false, path = false;
    bool occ_probe = false;       // the occluder-cache probe rides along (where the renderer has its table)
    bool stats_lds_pad = false;   // k_trace<STATS>: 64 bytes of LDS behind the stacks (the steps-per-ray histogram)
    uint32_t quad_slots = 0, tail = 0, budget = 0;
    uint32_t trace_waves = 0;    // k_trace's persistent waves before the cap by the ray count: whole groups of 8
    uint32_t stream_blocks = 0, shade_blocks = 0, trace_blocks = 0, coop_blocks = 0, packet_blocks = 0, path_blocks = 0;
    uint32_t stack_lds = 0, packet_lds = 0;   // bytes: a wave's per-lane stacks / k_trace_packet's 48 planes + its stack
};

// The rules (the expressions below are their only statement in code; the SPEC sections say why):
//
//   fact / knob                          | excludes                                                        | picks                          | where
//   -------------------------------------+-----------------------------------------------------------------+--------------------------------+-----------
//   masked (alpha-masked materials)      | pipe, packet, tail, budget, occluder probe, coop-all, path:     | TraceVariant::Mask / StatsMask | SPEC §20
//                                        | k_trace<STATS, false, false, MASK> alone asks the mask          |                                |
//   glass_shadow (punctual shadow rays   | what masked excludes — pipe, packet, tail, budget, occluder      | TraceVariant::Glass /          | SPEC §27
//   pass thin panes)                     | probe, coop-all, path —: k_trace_glass<STATS> alone asks the    | StatsGlass                     |
//                                        | pane (and §20's mask, where the scene has one)                  |                                |
//   stats                                | tail, budget, coop-all (a ray dropped at the budget would be    | TraceVariant::Stats*;          | DESIGN §5.5
//                                        | missing from the histogram and counted twice by the re-trace)   | k_path<.., STATS>              |
//   denoise                              | nothing                                                         | kShadeGbuf in shade_form0 and  | SPEC §15.1
//                                        |                                                                 | path_form                      |
//   env, punct                           | nothing                                                         | kShadeEnv, kShadePunct in the  | SPEC §18, §19
//                                        |                                                                 | shade forms and path_form      |
//   trans (a transmissive material used) | path (k_path's instantiations do not double)                    | kShadeTrans in the shade forms | SPEC §21
//   emis (an emissive material used)     | path (k_path's instantiations do not double)                    | kShadeEmis in the shade forms  | SPEC §22
//   esamp (emitter sampling; with emis)  | nothing (emis has excluded the path kernel)                     | kShadeEsamp in the shade forms,| SPEC §23
//                                        |                                                                 | only where emis                |
//   nmap (a normal-mapped material used) | path (k_path's instantiations do not double)                    | kShadeNmap in the shade forms  | SPEC §24
//   lens (the lens radius R > 0)         | packet, path: k_trace_packet rests on ONE origin per packet and  | k_raygen<.., LENS>, which      | SPEC §25
//                                        | k_path reads the shared origin                                  | fills q.o                      |
//   coop-all (n_rays <= coop_rays)       | path                                                            |                                | DESIGN §5.5
//   tail (solo, n_rays <= budget_rays)   | budget (nothing is dropped, so nothing to re-trace)             | TraceVariant::Tail / PipeTail  | DESIGN §5.5
//
// Without any of these facts the plan is the default launches of every frame before the feature.
inline LaunchPlan plan_wavefront(const LaunchTuning &t, const WavefrontFacts &f) {
    const auto div_up = [](uint32_t a, uint32_t b) { return (a + b - 1u) / b; };
    const KernelLimits &k = f.lim;
    const uint32_t n_rays = f.n_rays, cus = f.cus;
    LaunchPlan pl;
    const bool plain = f.masked || f.glass_shadow;   // the plain per-lane step alone: the acceptance site that asks SPEC §20 / §26 / §27
    pl.stream_blocks = std::min<uint32_t>(div_up(n_rays, k.kBlock), cus * 8u);
    pl.shade_blocks = std::min<uint32_t>(div_up(n_rays, k.kBlock), cus * (t.shade_blocks_per_cu ? t.shade_blocks_per_cu : (f.solo ? 4u : 3u)));
    // the one-round-trip step (kernels.h ray_step_pipe): 72 VGPRs (round 6; 78 before), 6 waves per SIMD used of the 7 that fit, ~3 % more nodes and ~12 % more triangles fetched per ray —
    // and still 1 % less time per frame at 8 M rays, 2 % for a 1 M-ray tile shard (profiles/r03_experiments_ab.txt); LPT_EXP_PIPE_RAYS 0 selects the two-round-trip step
    pl.pipe = !plain && n_rays <= t.pipe_rays;
    // persistent waves: about 2.5 primary rays per lane, between 8 waves per CU and all that fit (24 = 6 per SIMD with the one-round-trip step — 28 measured no faster, round 6 —, 32 with the other).  A 1/8
    // tile shard (1 M rays per launch) is best at 24 either way (round 3, span form, two-round-trip step: 8 / 12 / 16 / 24 / 32 waves per CU -> 4.41 / 3.89 / 3.62 / 3.51 / 3.54 ms per frame)
    const uint32_t waves = t.trace_waves_per_cu ? cus * t.trace_waves_per_cu : std::min(std::max(n_rays / 160u, cus * 8u), cus * (pl.pipe ? 24u : 32u));
    pl.trace_waves = std::max(8u, waves & ~7u);  // whole groups of 8: one chunk head per XCD
    pl.trace_blocks = std::min<uint32_t>(div_up(n_rays, k.kTraceBlock), pl.trace_waves);
    pl.stack_lds = f.stack_entries * k.kTraceBlock * 8u;   // uint2 entries
    pl.stats_lds_pad = f.stats;
    // Bounce 0 by packet traversal (one tree walk per 8x8-pixel patch) pays while the patch is narrow: at 1920x1080 a packet enters 17.9 nodes
    // for rays that need 14.9 each, and the walk runs at 11.5 Grays/s against 6.2 per ray; at 240x135 the same patch spans eight times the
    // angle, the walk visits several times the nodes, and the packet launch is a third of the frame (0.43 of 1.37 ms; 0.39 ms at 480x270,
    // where the per-ray launch needs 0.13).  LPT_OPT_PACKET_PRIMARY 2 (default): packets up to 1.8 mrad per pixel; 1: always; 0: never.
    pl.packet = !plain && !f.lens && (t.packet_primary == 1u || (t.packet_primary == 2u && f.pixel_rad <= k.kPacketMaxPixelRad));
    if (pl.packet) {
        pl.packet_blocks = std::min(div_up(n_rays, 64u), cus * k.kPacketBlocksPerCu);
        pl.packet_lds = (48u + 7u * f.max_depth + 8u) * (uint32_t)sizeof(uint32_t);
        // 4 samples of a 4x4-pixel quarter per packet instead of one sample of an 8x8 patch, where the queue order allows it: a dense frame
        // (queue index = sample * slots + slot), 8x8 pixel blocks inside the tiles, whole blocks, a multiple of four samples
        pl.quad_slots = (t.packet_quads && f.dense && f.block8 && f.n_slots % 64u == 0u && f.slot0 % 64u == 0u && f.n_samples % 4u == 0u) ? f.n_slots : 0u;
    }
    pl.occ_probe = !plain && f.stats;   // the occluder-cache probe rides with the stats kernels only (kernels.h OccProbe)
    // the step budget pays where nothing else fills the tail of a launch: a submission that is ONE wavefront (a tile shard, a small frame).  The
    // pieces of a cut batch overlap on the renderer's lanes and hide each other's tails: 1/2 shard as two wavefronts 6.84 ms without, 6.93 with it
    // (not with the stats kernels: a ray dropped at the budget would be missing from the steps-per-ray histogram and its partial node / triangle counts would be
    // counted again by the cooperative kernel's full re-trace — ADVICE r04)
    const bool tail_launch = !plain && !f.stats && (f.solo || t.budget_split) && n_rays <= t.budget_rays;
    // ... the tail finished in place (tail_walk) comes first where it is on: nothing is dropped then, so there is nothing to re-trace
    pl.tail = tail_launch ? std::min(std::min(t.tail_lanes, k.kTailMax), (uint32_t)std::max(t.refill, 0)) : 0u;
    pl.budget = (tail_launch && !pl.tail && t.step_budget) ? t.step_budget : 0u;
    // a TINY wavefront (fewer rays than the chip has wave slots): the per-bounce launches with EVERY ray traced by a whole wave (k_trace_coop over the queues) — a lane per
    // ray leaves the chip empty and the frame is one chain of dependent steps (64x36, 4 spp: k_path 0.72 ms per frame, the per-lane launches 0.83, this 0.39)
    pl.coop_all = !plain && !f.stats && t.coop_rays && n_rays <= t.coop_rays;
    // k_trace_coop's grid: a wave per ray of both queues, or a wave per straggler of a budgeted launch (most waves of that grid find none and leave at once)
    pl.coop_blocks = pl.coop_all ? std::min(2u * n_rays, cus * k.kCoopWavesPerCu) : (pl.budget ? cus * k.kCoopWavesPerCu : 0u);
    // A small wavefront (the tile shard of a multi-GPU frame): every bounce behind the primary hits in ONE persistent launch (k_path); the primary hits are there, whichever kernel found them
    pl.path = !plain && !f.trans && !f.emis && !f.nmap && !f.lens && t.path_rays && n_rays <= t.path_rays && !pl.coop_all;
    if (pl.path) pl.path_blocks = std::min<uint32_t>(div_up(n_rays, k.kTraceBlock), std::max(8u, (cus * t.path_waves_per_cu) & ~7u));
    pl.variant = f.glass_shadow ? (f.stats ? TraceVariant::StatsGlass : TraceVariant::Glass)
               : f.masked ? (f.stats ? TraceVariant::StatsMask : TraceVariant::Mask)
               : pl.tail  ? (pl.pipe ? TraceVariant::PipeTail : TraceVariant::Tail)
               : f.stats  ? (pl.pipe ? TraceVariant::StatsPipe : TraceVariant::Stats)
                          : (pl.pipe ? TraceVariant::Pipe : TraceVariant::Lane);
    // the shading forms: a bit per fact; bounce 0 of a denoising frame also writes the G-buffer, and k_path exists in the forms of GBUF | ENV | PUNCT alone
    const uint32_t lights = (f.env ? kShadeEnv : 0u) | (f.punct ? kShadePunct : 0u);
    pl.shade_form = lights | (f.trans ? kShadeTrans : 0u) | (f.emis ? kShadeEmis : 0u) | (f.emis && f.esamp ? kShadeEsamp : 0u) | (f.nmap ? kShadeNmap : 0u);
    pl.shade_form0 = pl.shade_form | (f.denoise ? kShadeGbuf : 0u);
    pl.path_form = pl.path ? (lights | (f.denoise ? kShadeGbuf : 0u)) : 0u;
    return pl;
}
