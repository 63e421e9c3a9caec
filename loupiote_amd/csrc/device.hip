// device.hip — Device / SceneGPU / ProbeGPU / Renderer behind the C ABI (include/lpt.h).
//
// Host orchestration of one frame follows Renderer::raytrace
// (reference crates/lib/src/renderer.rs:392-549): pass order, the seed / bounces /
// frame_count protocol and the accumulate flag.  raytrace() RECORDS (the reference records into an encoder the app submits
// once, app.rs:335-337); a submission point launches the recorded calls as wavefronts of several samples per pixel
// (record_call / flush_pending / wavefront_prepare + enqueue_stage + wavefront_finish).  A renderer enqueues on its own HIP stream (accumulation,
// filter passes, reads, the frame exchange: in call order) and on the streams of its wavefront lanes (the
// traversal / shading of consecutive wavefronts, overlapped); nothing here waits for the GPU except the
// read-back calls (the reference's only blocking point is read_pixels, :791) and scene edits.
// Also here: the multi-GPU frame exchange (plain RCCL, opened with dlopen: lpt_comm_*, lpt_renderer_exchange) and the
// tile-ownership rule (weighted shards).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <cstdlib>
#include <mutex>
#include <new>
#include <numeric>
#include <utility>

#include "common.h"
#include "env_dist.h"
#include "emit_dist.h"
#include "material_tables.h"
#include "kernels.h"
#include "probe_kernels.h"
#include "build_kernels.h"
#include "launch_plan.h"
#include "submission_plan.h"
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>

using namespace lpt;
using namespace lptd;

#define TRY(expr) do { const int st__ = (expr); if (st__ != LPT_OK) return st__; } while (0)
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) return fail(LPT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// Owning handles: a unique_ptr that also reads as the raw handle it owns, so it goes to a launch or a HIP call as that handle does.  What an owner holds is
// released when the owner goes or is assigned over; no release waits for work in flight on a stream (hipFree alone waits, for the whole device), so whoever
// drops an owner has synchronised what still uses it.
template <typename T, typename D> struct Owner : std::unique_ptr<T, D> {
    operator T *() const { return this->get(); }
};
struct HipFree { void operator()(void *p) const { hipFree(p); } };
struct HostFree { void operator()(void *p) const { hipHostFree(p); } };
struct StreamDestroy { void operator()(hipStream_t s) const { hipStreamDestroy(s); } };
struct EventDestroy { void operator()(hipEvent_t e) const { hipEventDestroy(e); } };
// device memory of n elements: alloc() takes the new memory before it lets go of the old
template <typename T> struct DevBuf : Owner<T, HipFree> {
    int alloc(size_t n) {
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, sizeof(T) * n));
        this->reset((T *)p);
        return LPT_OK;
    }
};
using DevMem = DevBuf<char>;   // untyped: alloc(bytes), read through as<T>()
template <typename T> static inline T *as(const DevMem &m) { return (T *)m.get(); }
struct Stream : Owner<std::remove_pointer_t<hipStream_t>, StreamDestroy> {
    int create() { hipStream_t s = nullptr; HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); reset(s); return LPT_OK; }
};
struct Event : Owner<std::remove_pointer_t<hipEvent_t>, EventDestroy> {
    int create(unsigned flags = hipEventDisableTiming) { hipEvent_t e = nullptr; HIP_TRY(hipEventCreateWithFlags(&e, flags)); reset(e); return LPT_OK; }
};
template <typename T> using HostWord = Owner<T, HostFree>;   // page-locked host memory
// a group of owners is released by assignment: what it held goes, member by member in declaration order, and its plain members are back at their defaults
template <typename G> static inline void release(G &g) { g = G{}; }

struct lpt_device {
    int ordinal = 0;
    Stream stream;
    int compute_units = 0;
    char name[128] = {0};
    std::vector<lpt_renderer *> renderers;   // live renderers of this device: scene / probe edits submit their recorded calls first
};

// one RCCL communicator rank (frame exchange); created by lpt_comm_create
struct lpt_comm {
    lpt_device *dev = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
};

// librccl is opened on the first lpt_comm_* call, not at load time: a single-GPU host never needs it (and never pays for
// loading it).  rccl.h supplies the types only; nothing here links against the library.
struct Rccl {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
// nullptr (and lpt_last_error set) when librccl cannot be opened
static const Rccl *rccl() {
    static Rccl table;
    static int state = 0;   // 0 = not tried, 1 = loaded, -1 = failed
    static std::string why = "missing symbol";   // dlerror() of the failed attempt (it reads once: a second call returns NULL)
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (state == 1) return &table;
    if (state == 0) {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
        std::string rocm_path;
        if (const char *rp = getenv("ROCM_PATH")) rocm_path = std::string(rp) + "/lib/librccl.so";
        void *h = nullptr;
        // LPT_RCCL_LIBRARY: another build of RCCL — or the multi-process test stand-in (tests/tools/fake_rccl.c), which lets N
        // ranks share the one GPU of a test box; when it is set nothing else is tried
        state = -1;
        if (const char *lp = getenv("LPT_RCCL_LIBRARY")) { h = dlopen(lp, RTLD_NOW | RTLD_LOCAL); rocm_path.clear(); if (!h) { if (const char *e = dlerror()) why = e; goto rccl_done; } }
        if (!rocm_path.empty()) h = dlopen(rocm_path.c_str(), RTLD_NOW | RTLD_LOCAL);
        for (size_t i = 0; !h && i < sizeof names / sizeof names[0]; ++i) h = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
        if (!h) { if (const char *e = dlerror()) why = e; }
        if (h) {
            table.handle = h;
            bool ok = true;
#define RCCL_SYM(field, sym) do { *(void **)(&table.field) = dlsym(h, sym); if (!table.field) ok = false; } while (0)
            RCCL_SYM(GetUniqueId, "ncclGetUniqueId"); RCCL_SYM(CommInitRank, "ncclCommInitRank"); RCCL_SYM(CommDestroy, "ncclCommDestroy");
            RCCL_SYM(CommCount, "ncclCommCount"); RCCL_SYM(CommUserRank, "ncclCommUserRank");
            RCCL_SYM(GroupStart, "ncclGroupStart"); RCCL_SYM(GroupEnd, "ncclGroupEnd"); RCCL_SYM(Send, "ncclSend"); RCCL_SYM(Recv, "ncclRecv");
            RCCL_SYM(Reduce, "ncclReduce"); RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RCCL_SYM
            if (ok) state = 1;
        }
    rccl_done:;
    }
    if (state == 1) return &table;
    fail(LPT_ERR_RCCL, "librccl could not be loaded (%s): the multi-GPU frame exchange needs RCCL", why.c_str());
    return nullptr;
}

#define RCCL_TRY(expr)                                                                                \
    do {                                                                                              \
        ncclResult_t r__ = (expr);                                                                    \
        if (r__ != ncclSuccess) return fail(LPT_ERR_RCCL, "%s failed: %s", #expr, rccl() ? rccl()->GetErrorString(r__) : "?"); \
    } while (0)

// The wide BVH on the device: what a build makes and a rebuild swaps in whole.  Nodes are stored breadth first: level l = [level_start[l], level_start[l+1]).
struct DevTree {
    DevMem nodes, woop, leaf_prim;
    DevMem node_lo, node_hi;   // per-node world box (refits)
    std::vector<uint32_t> level_start;
    uint32_t n_nodes = 0, max_depth = 0;
    float build_ms = 0.f;
};

// paired textures (kernels.h DScene::pair_texels): (albedo image, mra image) -> pair index, for the materials whose two textures have one size; the shading
// records of such materials carry kPairedBit | pair index instead of two image ids
struct TexturePairs {
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> map;
    std::vector<DImage> descs;   // a paired material's record carries its pair's offset and size directly
    // which images the tiled atlas holds on their own: an image that only ever appears as half of a pair is not stored a second
    // time (scene.rs:172-184 keeps each image once)
    std::vector<uint8_t> image_resident;
};

struct lpt_scene_gpu {
    lpt_device *dev = nullptr;
    DScene d{};
    float max_abs = 0.f;            // the scene's largest |coordinate|: d.pad_abs = kScenePad x this (host build: Accel::max_abs; GPU build: the bounds pass; refit: the root box)
    DevTree tree;
    DevMem tri_verts, materials, lights, texels, images, srgb_lut, pair_texels, pair_images;
    DevMem punctual;                // SPEC §19: lpt_punctual_light records (DScene::punctual)
    struct { DevMem tri, recs; } mat_tab[MAT_KINDS];   // SPEC §20, §21, §22, §24: per kind of material_tables.h the per-triangle table and the records (DScene::alpha_tri / alpha_recs, ...); empty where the scene does not use the kind
    uint32_t n_thin_glass = 0;      // SPEC §27: baked triangles whose material is transmissive and thin-walled (derived with the tables: upload, rebuild, instance update)
    DevMem emit_tab;                // SPEC §23: the emitter distribution's entries (DScene::emit_tab); empty without a distribution
    TexturePairs pairs;
    lpt_accel_stats stats{};
    // refit bookkeeping (lpt_scene_gpu_update_instances)
    DevMem obj_verts, obj_indices, bad_flag;   // object-space meshes for device-side re-baking
    DevMem arena;                              // scratch of the GPU builder, kept for rebuilds
    size_t arena_bytes = 0;
    std::vector<uint32_t> inst_first, inst_count;
    std::vector<lpt_instance> instances;       // as baked
    size_t n_entries = 0, n_vertices = 0, n_indices = 0;
};

struct lpt_probe {
    lpt_device *dev = nullptr;
    DProbe d{};
    DevMem rgbe;
    // SPEC §18: the sampling distribution, built on first use (probe_env) — a probe never sampled costs nothing for it
    int env_state = 0;         // 0: not built, 1: built (env), 2: the probe has none (black)
    DevBuf<float4> env_buf;    // rows then cols, 16-byte entries
    DEnv env{};
};

enum { ST_RAYGEN = 0, ST_INTERSECT, ST_SHADE, ST_SHADOW, ST_ACCUM, ST_ASVGF, ST_EXCHANGE, ST_PRIMARY, ST_PATH, ST_COUNT };
// "primary intersection": the IntersectorPass of bounce 0 when it runs as packet traversal (k_trace_packet), timed apart from the
// per-ray traversal launches ("intersection") because it is another kernel
// "path": every bounce behind the primary hits in ONE launch (k_path), the form small wavefronts — the tile shard of a multi-GPU frame — take
static const char *kStageLabel[ST_COUNT] = {"ray generation", "intersection", "shading", "shadow", "accumulation", "asvgf", "exchange", "primary intersection", "path"};

// One independent wavefront context ("lane") of a renderer: everything a raytrace() call owns while its rays are in flight.
// Consecutive raytrace() calls of ONE renderer take the lanes in turn (default 2), so the traversal / shading of call k+1
// overlaps the drain tails of call k — what several renderers do for several frames, for the unchanged caller that issues
// its samples one raytrace() at a time.  Accumulation stays on the renderer's stream, in call order (the fp32 sums are
// order-sensitive), so results do not depend on the number of lanes.
// Its resources are two groups (bases, so that a member reads wf.Lsum): each is made whole or not at all, and released by assignment (release()).
struct LaneSync {                   // ensure_lane; lives as long as the renderer
    Stream stream;                  // the lane's own stream; lane 0 (and a renderer with one lane) runs on the renderer's stream and has none
    Event done;                     // recorded on `stream` behind the lane's last traversal / shading launch
    Event consumed;                 // recorded on the renderer's stream behind the accumulation that read this lane's Lsum
    bool consumed_recorded = false;
    Event trav[kMaxBounces + 1];    // LPT_EXP_LANE_PHASE: trav[t] recorded on the lane's stream behind traversal launch t (0: the primary rays) of the lane's wavefront; created when a plan first asks for them
    DevBuf<FrameCounters> ctr;
};
struct RayBuffers {                 // alloc_ray_buffers: one element per ray of a wavefront
    struct { DevBuf<float4> o, d, t; } q_mem[2], sq_mem;   // Queue's o, d, T and ShadowQueue's o, d, c
    DevBuf<float4> hits, Lsum;
    DevBuf<uint32_t> strag;         // the stragglers of a traversal launch (k_trace's step budget -> k_trace_coop): ray index | shadow << 31
    size_t ray_cap = 0;             // rays (pixel slots x samples) the buffers can hold; 0 = not allocated yet
    Queue q[2]{};                   // what the kernels get of the queues, by value: bound by alloc_ray_buffers
    ShadowQueue sq{};
};
struct Wavefront : LaneSync, RayBuffers {};   // the stream and events outlive the buffers that were used on them
constexpr int kMaxLanes = 4;
constexpr float kPacketMaxPixelRad = 1.8e-3f;    // bounce 0 as packets up to this angle per pixel (measured: 1.53 mrad, 960x540: packets 4.46 against 4.51 ms; 2.05 mrad, 720x405: 3.32 against 3.20)
constexpr uint32_t kOccEntries = 1u << 18;       // occluder-cache probe: 1 MB, L2-resident
constexpr uint64_t kSplitRays = 3000000ull;       // a batch above this leaves as at least two wavefronts (LPT_EXP_SPLIT_RAYS)
constexpr uint32_t kPacketBlocksPerCu = 128u;   // k_trace_packet's grid: one-wave blocks, packets dealt by stride (32 / 64 per CU: the same, round 5)
constexpr uint32_t kCoopWavesPerCu = 32u;   // k_trace_coop's grid: a wave per straggler, most waves find none and leave (8 / 4 per CU: the same 2.90 ms per 1/8-shard frame, round 5)
constexpr uint64_t kWavefrontRays = 1ull << 22;   // rays (pixel slots x samples) per wavefront an automatic submission aims at

// A renderer's resources that come and go with its size or mode are groups, as a lane's are.  The stream and the exchange's event are the first base: they go last.
struct RendererSync {
    Stream stream;                  // every renderer enqueues on its OWN stream, so two renderers pipeline
                                    // consecutive frames (and a frame's collective overlaps the next frame)
    Event xevent;
};
struct FrameBuffers {               // alloc_frame_buffers; `frame` and `xstage` join on the first exchange (ensure_exchange_buffers)
    uint32_t n_slots = 0;
    DevBuf<float4> accum, scratch;
    // frame exchange (lpt_renderer_exchange): `frame` = the presented whole frame on rank 0 (accum stays owned-only),
    // `xstage` = packed owned tiles (this rank's; on rank 0 those of every rank, concatenated)
    DevBuf<float4> frame, xstage;
    size_t xstage_elems = 0;
    bool presented = false;         // read_radiance / read_pixels / blit resolve from `frame` (set by an exchange, cleared by raytrace)
    bool xevent_recorded = false;
};
// denoiser path (reference render/asvgf.rs ScreenResources :9-152): 2x ping-pong {radiance, gbuffer, moments,
// history} + motion + radiance_temp; allocated on first use of a denoising BlitMode (ensure_denoiser), whole or not at all
struct Denoiser {
    DevBuf<uint4> den_gbuf[2];
    DevBuf<float4> den_rad[2];
    DevBuf<float2> den_mom[2];
    DevBuf<uint32_t> den_hist[2];
    DevBuf<float2> den_motion;
    DevBuf<float4> den_temp;
    DevBuf<float4> den_noisy;       // per-pixel sample radiance of the current frame (filter input; exchanged when sharded)
    DevBuf<float4> den_nd;          // the current G-buffer's normal + depth, decoded once per frame for the a-trous passes
    bool den_inputs_ready = false;
    int den_cur = 1;                // current_frame_back starts true (asvgf.rs:233); start() flips it
    bool has_denoiser() const { return (bool)den_temp; }   // any member tells
};

struct lpt_renderer : RendererSync, FrameBuffers, Denoiser {
    lpt_device *dev = nullptr;
    Wavefront wf[kMaxLanes];
    int n_lanes = 2;                // lpt_renderer_set_lanes
    uint32_t lane_rr = 0;
    int last_lane = 0;
    uint32_t req_w = 0, req_h = 0, w = 0, h = 0;
    float downsample = 0.5f;
    const lpt_scene_gpu *sg = nullptr;
    const lpt_probe *probe = nullptr;
    bool resources_set = false;
    // global_uniforms (renderer.rs:286-290)
    uint32_t frame_count = 1, seed = 0;
    bool accumulate = false, frame_back = true;
    // Recorded, not yet submitted raytrace() calls ("record now, submit later": the reference records every pass of a frame
    // into one encoder, renderer.rs:392-549, and the app submits it once, app.rs:335-337).  Consecutive calls with the same
    // view that continue one accumulation fuse into ONE wavefront of `n` samples per pixel; the host-side protocol state
    // (frame_count, seed, frame_back) moves at record time, the snapshot below is what the launches use.
    struct Pending { float view[16]; uint32_t n = 0, frame_count0 = 1, seed0 = 0; bool acc0 = false; } pend;
    uint32_t max_fused = 0;    // 0 = auto: up to 64 calls wait for the next submission point, which cuts them into wavefronts of about 4 M rays
                               // (spatially: runs of tile rows x all the samples); n >= 1: n calls are ONE wavefront and launch when the n-th is recorded
    LaunchTuning tune;         // which kernels a wavefront runs and their grids (launch_plan.h; lpt_renderer_set_option)
    uint64_t wavefront_rays = kWavefrontRays;   // LPT_OPT_WAVEFRONT_RAYS: tests cut small frames into many wavefronts
    uint64_t n_recorded = 0, n_wavefronts = 0;   // raytrace() calls recorded / wavefronts submitted so far (lpt_renderer_get_submission_stats)
    int mode = LPT_BLIT_PATHTRACE;
    // build-only knobs
    uint32_t max_bounces = 3, user_seed = 0;
    int glass_shadows = 0;     // SPEC §27 (lpt_renderer_set_glass_shadows): punctual lights' shadow rays pass thin-walled panes, while the bound scene has both
    int emissive_sampling = 0; // SPEC §23 (lpt_renderer_set_emissive_sampling): the ESAMP kernels while the bound scene has an emitter distribution
    int env_sampling = 0;      // SPEC §18 (lpt_renderer_set_env_sampling): the ENV kernels while the bound probe has a distribution
    float vfov = 0.78539816339744830962f;
    float lens_r = 0.0f, lens_f = 1.0f;   // SPEC §25 (lpt_renderer_set_lens): the lens radius (0: the pinhole of §11) and the focus distance
    uint32_t rank = 0, world = 1, tile_w = 32, tile_h = 8;
    std::vector<uint32_t> weights;   // tile-ownership weights of the ranks (empty = every rank 1: tile id mod world)
    ShardMap map{1u, 1u, {0u}};      // this rank's part of the ownership rule
    ShardTable h_table{};            // rank 0: the whole rule ...
    std::vector<uint32_t> h_offset;  // ... the staging offsets of the ranks (world + 1 entries, any world size) ...
    DevBuf<ShardTable> d_table;      // ... and the rule's copy in device memory for the unpack kernels; refreshed by alloc_frame_buffers
    bool use_noise = false, stats = false, timings = false;
    int sort_queues = 0;       // k_shade emits both ray queues ordered by direction octant within a block (lpt_renderer_set_sort_queues)
    uint32_t lane_phase = 1;   // the pieces of a cut batch against each other (LPT_EXP_LANE_PHASE): 0 free, 1 offset start, 2 alternating traversal (submission_plan.h: the rules and what they measured)
    lpt_comm *comm = nullptr;
    // device memory that lives as long as the renderer
    DevBuf<Totals> totals;
    uint64_t split_rays = kSplitRays;   // LPT_EXP_SPLIT_RAYS
    HostWord<uint32_t> err_host;   // the device's error word: one page-locked host word the kernels write (a bounded wait that ran out), checked behind every blocking call
    DevBuf<uint32_t> occ_table;      // occluder-cache probe (stats only): kOccEntries leaf slots + 1, zero = empty; allocated by enable_stats
    float occ_cell = 0.25f;          // its grid cell (scene units); LPT_EXP_OCC_CELL_MILLI
    DevMem default_probe;
    DevBuf<float> srgb_thr;      // 256 floats: the linear value at which sRGB code i starts (k_tonemap, SPEC §13.2)
    // SPEC §30 (lpt_renderer_set_display): read where pixels are presented as sRGB bytes, by nothing else.  (0, CLAMP), the default: k_tonemap, as before
    float display_ev = 0.0f, display_gain = 1.0f;   // the gain = (float)exp2((double)ev), rounded once
    uint32_t display_op = LPT_DISPLAY_CLAMP;
    DevBuf<uint32_t> meter_hist;   // kMeterWords: k_meter's histogram and its skipped count; allocated by the first lpt_renderer_meter
    DevMem noise;
    uint32_t noise_w = 0, noise_h = 0;
    CamBasis prev_cam{};          // prev_model_to_screen (renderer.rs:201,319,542-546), identity at start
    // per-stage timing: a ring of event sets (one per raytrace() call) harvested lazily, so
    // timing a run never stalls the host on the frame it has just enqueued
    static constexpr int kRing = 8;
    static constexpr int kMaxEvents = 3 * kMaxBounces + 4;
    std::vector<Event> ev_start, ev_stop;  // kRing * kMaxEvents each, from the first enable_timings(1)
    int ev_stage[kRing][kMaxEvents]{};
    int ev_count[kRing]{};
    uint64_t ring_pos = 0;
    double stage_ms[ST_COUNT]{};
    uint32_t stage_launches[ST_COUNT]{};
};

static inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }
// submits the recorded raytrace() calls; every synchronisation point, and every setter whose value the launches read, runs it first
// what a submission copies to the host as its wavefronts complete (lpt_renderer_read_radiance / lpt_renderer_blit_rgba8)
struct ReadPlan {
    float *radiance = nullptr;      // mean radiance, w*h*4 floats, tight rows
    uint8_t *rgba8 = nullptr;       // or: tonemapped sRGB RGBA8 ...
    size_t row_bytes = 0;           // ... with this row pitch
};
static int flush_pending(lpt_renderer *r, const ReadPlan *read = nullptr);
static void forget_deferred_exchange(lpt_renderer *r);
static FrameParams shard_params(const lpt_renderer *r);
static inline uint32_t stream_grid(const lpt_renderer *r, size_t n);
#define FLUSH_OR_RETURN(r) do { int fst__ = flush_pending(r); if (fst__ != LPT_OK) return fst__; } while (0)
// Recorded raytrace() calls saw the scene / probe as it was when they were issued: an edit (or a destroy) submits them first.
static int flush_device(lpt_device *dev) {
    int st = LPT_OK;
    if (!dev) return st;
    for (lpt_renderer *r : dev->renderers) {
        const int f = flush_pending(r);
        if (st == LPT_OK) st = f;   // the first failure is what the caller reports (lpt_last_error holds its text)
    }
    return st;
}
// what read_radiance / read_pixels / blit show: the exchanged whole frame after lpt_renderer_exchange, else the local target
static inline const float4 *presented_target(const lpt_renderer *r) { return (r->presented && r->frame) ? r->frame : r->accum; }
// SPEC §13.2: the linear value at which sRGB code i starts
static void srgb_thresholds(float thr[256]) {
    thr[0] = 0.0f;
    for (int i = 1; i < 256; ++i) {   // inverse OETF at (i - 0.5) / 255 in binary64, rounded once
        const double v = ((double)i - 0.5) / 255.0;
        thr[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
    }
}
// n accumulators to sRGB bytes, on `s`: the one decision of both sites that present bytes (a recorded frame's piecewise read-back, lpt_renderer_blit_rgba8).  While
// the display state is its default, (0, CLAMP), this is the k_tonemap launch of SPEC §13.2 as it always was; any other state launches §30's k_display<op>
static_assert((uint32_t)kDisplayClamp == (uint32_t)LPT_DISPLAY_CLAMP && (uint32_t)kDisplayPbrNeutral == (uint32_t)LPT_DISPLAY_PBR_NEUTRAL &&
              (uint32_t)kDisplayAces == (uint32_t)LPT_DISPLAY_ACES && (uint32_t)kDisplayOps == 3u,
              "display_math.h's operators are the header's LPT_DISPLAY_* values");
// k_display<op> over n accumulators: the one place that turns an operator (checked by display_args) into a kernel, for the renderer and for lpt_display_probe
static void launch_display(uint32_t op, hipStream_t s, const float4 *src, uchar4 *dst, uint32_t n, const float *thr, float gain) {
    const dim3 grid(div_up(n, kBlock)), block(kBlock);
    if (op == kDisplayClamp) hipLaunchKernelGGL(k_display<kDisplayClamp>, grid, block, 0, s, src, dst, n, thr, gain);
    else if (op == kDisplayPbrNeutral) hipLaunchKernelGGL(k_display<kDisplayPbrNeutral>, grid, block, 0, s, src, dst, n, thr, gain);
    else hipLaunchKernelGGL(k_display<kDisplayAces>, grid, block, 0, s, src, dst, n, thr, gain);
}
static void launch_present(const lpt_renderer *r, hipStream_t s, const float4 *src, uchar4 *dst, uint32_t n) {
    if (r->display_op == kDisplayClamp && r->display_ev == 0.0f) hipLaunchKernelGGL(k_tonemap, dim3(div_up(n, kBlock)), dim3(kBlock), 0, s, src, dst, n, r->srgb_thr);
    else launch_display(r->display_op, s, src, dst, n, r->srgb_thr, r->display_gain);
}
// The device's error word (a page-locked host word the kernels write when a bounded wait runs out; no shipped kernel has one since k_pool left the library in round 6).  Read behind a
// blocking call, once the stream has been waited for: the frame that raised it is void.
static int check_device_error(lpt_renderer *r) {
    if (!r->err_host) return LPT_OK;
    const uint32_t code = *(volatile uint32_t *)r->err_host;
    if (!code) return LPT_OK;
    *(volatile uint32_t *)r->err_host = 0u;
    return fail(LPT_ERR_HIP, "a device-side bounded wait ran out (code 0x%x): the frame is void", code);
}
static inline size_t stack_bytes(const DScene &sc) { return (size_t)sc.stack_entries * kTraceBlock * sizeof(uint2); }

// The one path of every per-element probe (probe_kernels.h; the entry points are under "per-element probes" below): n elements up, one launch, n answers back.  Each
// input and output is a host array and its bytes per element; `launch(grid, d)` gets the grid of `block`-thread blocks that covers n and the device arrays, the inputs
// first, each list in its order.  Everything runs on dev->stream and is waited for once at the end, so nothing depends on how the null stream orders against a
// non-blocking one; the host arrays are the caller's until then.  Argument checks are the entry point's.
// An array with `whole` set is not per element: it has `whole` bytes whatever n is (a table going up, a histogram coming back), and such an output is zero at the launch.
struct ProbeIn { const void *host; size_t stride; size_t whole = 0; };
struct ProbeOut { void *host; size_t stride; size_t whole = 0; };
template <typename Launch>
static int run_probe(lpt_device *dev, uint32_t n, uint32_t block, std::initializer_list<ProbeIn> ins, std::initializer_list<ProbeOut> outs, Launch &&launch) {
    if (!n) return LPT_OK;
    HIP_TRY(hipSetDevice(dev->ordinal));
    std::vector<DevMem> d(ins.size() + outs.size());
    const auto bytes = [n](const auto &b) { return b.whole ? b.whole : b.stride * n; };
    size_t k = 0;
    for (const ProbeIn &b : ins) TRY(d[k++].alloc(bytes(b)));
    for (const ProbeOut &b : outs) TRY(d[k++].alloc(bytes(b)));
    k = 0;
    for (const ProbeIn &b : ins) HIP_TRY(hipMemcpyAsync(d[k++].get(), b.host, bytes(b), hipMemcpyHostToDevice, dev->stream));
    for (const ProbeOut &b : outs) { if (b.whole) HIP_TRY(hipMemsetAsync(d[k].get(), 0, b.whole, dev->stream)); ++k; }
    k = ins.size();
    launch(dim3(div_up(n, block)), d.data());
    HIP_TRY(hipGetLastError());
    for (const ProbeOut &b : outs) HIP_TRY(hipMemcpyAsync(b.host, d[k++].get(), bytes(b), hipMemcpyDeviceToHost, dev->stream));
    HIP_TRY(hipStreamSynchronize(dev->stream));
    return LPT_OK;
}
// the ray queries: a ray goes up as two float4, (origin, tmax — read by the occlusion query alone) and (direction, -)
static void pack_rays(const float *origins, const float *dirs, const float *tmax, uint32_t n, std::vector<float4> &o, std::vector<float4> &d) {
    o.resize(n); d.resize(n);
    for (size_t i = 0; i < n; ++i) {
        o[i] = make_float4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], tmax ? tmax[i] : 0.f);
        d[i] = make_float4(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], 0.f);
    }
}
// the (prim, ...) probes: every element names a triangle of the scene
static int check_prims(const char *who, const DScene &d, const uint32_t *prim, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (prim[i] >= d.n_tris) return fail(LPT_ERR_INVALID_ARG, "%s: element %u names triangle %u of %u", who, i, prim[i], d.n_tris);
    return LPT_OK;
}

template <typename T>
static int upload(DevMem &dst, const std::vector<T> &src, hipStream_t s) {
    TRY(dst.alloc(sizeof(T) * std::max<size_t>(src.size(), 1u)));
    if (!src.empty()) HIP_TRY(hipMemcpyAsync(dst.get(), src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, s));
    return LPT_OK;
}

// ---------------------------------------------------------------------------- GPU builder (build_kernels.h) and refit
// Scene bounds from the baked triangles on the device (blocking), and what follows from them for every kernel that pads a triangle or writes a node: the scene-wide part
// of the triangle padding (bvh.cpp padded_box; it never shrinks — a pad a little too wide costs nothing) and the scene grid of the node origins (common.h scene_grid, of the
// bounds widened by that padding).  Before a build and before every refit.
static int scene_bounds_and_grid(lpt_scene_gpu *sg, uint32_t n, hipStream_t s, float blo[3], float bhi[3], bool keep_pad) {
    int hb[6];
    const int init[6] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, (int)0x80000000, (int)0x80000000, (int)0x80000000};
    DevMem db;
    TRY(db.alloc(sizeof init));
    HIP_TRY(hipMemcpyAsync(db.get(), init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lbvh_bounds, dim3(std::min<uint32_t>(div_up(n, 256u), 1024u)), dim3(256), 0, s, sg->d, n, as<int>(db));
    HIP_TRY(hipMemcpyAsync(hb, db.get(), sizeof hb, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int a = 0; a < 6; ++a) { const int o = hb[a] >= 0 ? hb[a] : hb[a] ^ 0x7FFFFFFF; float f; memcpy(&f, &o, 4); (a < 3 ? blo[a] : bhi[a - 3]) = f; }
    float now_abs = 0.0f;
    for (int a = 0; a < 3; ++a) now_abs = std::max(now_abs, std::max(fabsf(blo[a]), fabsf(bhi[a])));
    sg->max_abs = keep_pad ? std::max(sg->max_abs, now_abs) : now_abs;
    sg->d.pad_abs = kScenePad * sg->max_abs;   // (renderers read sg->d at submission)
    // the grid must reach below every PADDED node box: the bounds above are of the bare vertices, and after a refit the kept padding (max_abs never shrinks) may belong
    // to a place farther from the origin than anything is now — widen by the most a triangle is padded by (padded_box: 4e-6 m + pad_abs + 1e-6 extent) before choosing the grid
    float glo[3], ghi[3];
    for (int a = 0; a < 3; ++a) {
        const float e = 4.0f * sg->d.pad_abs + 2e-6f * (bhi[a] - blo[a]) + 1e-30f;
        glo[a] = blo[a] - e;
        ghi[a] = bhi[a] + e;
    }
    scene_grid(glo, ghi, sg->d.grid_lo, sg->d.grid_step);
    return LPT_OK;
}

// the boxes of every node of `t`, from the bottom level up, over the triangles and grid of `d`
static void refit_levels(const DScene &d, const DevTree &t, hipStream_t s) {
    for (size_t l = t.level_start.size() - 1; l-- > 0;) {
        const uint32_t a = t.level_start[l], b = t.level_start[l + 1];
        if (b > a) hipLaunchKernelGGL(k_refit_level, dim3(div_up(b - a, 64u)), dim3(64), 0, s, d, as<uint4>(t.nodes), as<float4>(t.node_lo), as<float4>(t.node_hi), a, b);
    }
}

// the prim-ordered Woop maps of triangles [first, first + count) to their places in `t` (a split triangle has several)
static void scatter_woop(const DevTree &t, const void *woop_prim, uint32_t first, uint32_t count, hipStream_t s) {
    const uint32_t n_places = kNodeTris * t.n_nodes;
    hipLaunchKernelGGL(k_lbvh_scatter_woop, dim3(div_up(n_places, 256u)), dim3(256), 0, s, (const float4 *)woop_prim, as<float4>(t.woop), as<const uint32_t>(t.leaf_prim),
                       n_places, first, count);
}

// A new tree over the n baked triangles already on the device (sg->d.tri_verts); `woop_prim` = their Woop maps in prim order (device).  The tree goes to
// `out` only when the build succeeds.  Of sg it sets the padding and grid of the new scene (scene_bounds_and_grid, max_abs reset) and reuses the scratch arena.
static int build_lbvh(lpt_scene_gpu *sg, uint32_t n, const void *woop_prim, hipStream_t s, DevTree &out) {
    const auto t0 = std::chrono::steady_clock::now();
    float blo[3], bhi[3];
    TRY(scene_bounds_and_grid(sg, n, s, blo, bhi, false));
    float binv[3];
    for (int a = 0; a < 3; ++a) binv[a] = bhi[a] > blo[a] ? 1.0f / (bhi[a] - blo[a]) : 0.0f;

    // scratch: one arena per scene, kept for the next rebuild (about 400 B per triangle); every piece is carved from it before the first launch
    size_t sort_bytes = 0, scan_bytes = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 30, s);
    hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, s);
    const size_t cub_cap = std::max(sort_bytes, scan_bytes);
    const size_t need = (size_t)n * 400u + cub_cap + 64u * 256u;
    if (sg->arena_bytes < need) {
        sg->arena.reset();
        sg->arena_bytes = 0;
        if (sg->arena.alloc(need) != LPT_OK) return fail(LPT_ERR_HIP, "GPU BVH build: out of device memory (%zu bytes of scratch)", need);
        sg->arena_bytes = need;
    }
    size_t arena_used = 0;
    auto carve = [&](auto *&p, size_t count) {
        const size_t at = (arena_used + 255u) & ~(size_t)255u;
        p = (std::remove_reference_t<decltype(p)>)((char *)sg->arena.get() + at);
        arena_used = at + sizeof(*p) * count;
    };
    uint32_t *keys, *vals, *keys_s, *vals_s, *leaf_big, *inner_count, *tri_count, *inner_off, *tri_off;
    uint8_t *cub_tmp;
    uint4 *nodes_big;
    int *items_a, *items_b, *kid_ref;
    LbvhTree T{};
    carve(keys, n); carve(vals, n); carve(keys_s, n); carve(vals_s, n);
    carve(T.left, n); carve(T.right, n); carve(T.parent, n); carve(T.leaf_parent, n);
    carve(T.first, n); carve(T.last, n); carve(T.lo, n); carve(T.hi, n); carve(T.tri_lo, n); carve(T.tri_hi, n); carve(T.flag, n);
    carve(cub_tmp, cub_cap);
    // wide tree, level by level
    carve(nodes_big, 4u * (size_t)n);            // <= n-1 wide nodes
    carve(leaf_big, (size_t)kNodeTris * n);      // their triangle places (16 per node; the final array is cut to the nodes there are)
    carve(items_a, n); carve(items_b, n); carve(kid_ref, 8u * (size_t)n);
    carve(inner_count, n); carve(tri_count, n); carve(inner_off, n); carve(tri_off, n);
    if (arena_used > sg->arena_bytes) return fail(LPT_ERR_HIP, "GPU BVH build: out of device memory");
    T.sorted_tri = vals_s; T.keys = keys_s; T.n = n;

    const uint32_t b256 = div_up(n, 256u);
    hipLaunchKernelGGL(k_lbvh_morton, dim3(b256), dim3(256), 0, s, sg->d, n, make_float3(blo[0], blo[1], blo[2]), make_float3(binv[0], binv[1], binv[2]), keys, vals);
    size_t cub_bytes = cub_cap;
    if (hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, keys, keys_s, vals, vals_s, (int)n, 0, 30, s) != hipSuccess) return fail(LPT_ERR_HIP, "GPU BVH build: sort failed");
    hipLaunchKernelGGL(k_lbvh_leaf_boxes, dim3(b256), dim3(256), 0, s, sg->d, T);
    HIP_TRY(hipMemsetAsync(T.flag, 0, sizeof(uint32_t) * n, s));
    hipLaunchKernelGGL(k_lbvh_tree, dim3(b256), dim3(256), 0, s, T);
    hipLaunchKernelGGL(k_lbvh_fit, dim3(b256), dim3(256), 0, s, T);

    HIP_TRY(hipMemsetAsync(leaf_big, 0xFF, sizeof(uint32_t) * (size_t)kNodeTris * n, s));   // holes: LPT_INVALID_INDEX
    HIP_TRY(hipMemsetAsync(items_a, 0, sizeof(int), s));  // level 0 = the binary root
    int *items_cur = items_a, *items_next = items_b;
    uint32_t n_items = 1, level_first = 0, tri_running = 0;
    DevTree t;
    while (n_items) {
        if (t.level_start.size() > 64) return fail(LPT_ERR_ACCEL_BUILD, "GPU BVH build: tree deeper than 64 levels");
        LbvhLevel L{items_cur, n_items, kid_ref, inner_count, tri_count};
        hipLaunchKernelGGL(k_lbvh_collapse, dim3(div_up(n_items, 64u)), dim3(64), 0, s, T, L);
        cub_bytes = cub_cap;
        hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, inner_count, inner_off, (int)n_items, s);
        cub_bytes = cub_cap;
        hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, tri_count, tri_off, (int)n_items, s);
        uint32_t tail[4];
        HIP_TRY(hipMemcpyAsync(&tail[0], inner_off + (n_items - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&tail[1], inner_count + (n_items - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&tail[2], tri_off + (n_items - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&tail[3], tri_count + (n_items - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const uint32_t inner_total = tail[0] + tail[1], tri_total = tail[2] + tail[3];
        if ((size_t)level_first + n_items + inner_total > n) return fail(LPT_ERR_ACCEL_BUILD, "GPU BVH build: node budget exceeded");
        hipLaunchKernelGGL(k_lbvh_emit, dim3(div_up(n_items, 64u)), dim3(64), 0, s, T, L, inner_off, tri_off, level_first, level_first + n_items, tri_running,
                           nodes_big, leaf_big, items_next);
        t.level_start.push_back(level_first);
        level_first += n_items;
        tri_running += tri_total;
        n_items = inner_total;
        std::swap(items_cur, items_next);
    }
    t.level_start.push_back(level_first);
    if (tri_running != n) return fail(LPT_ERR_ACCEL_BUILD, "GPU BVH build: %u of %u triangles referenced", tri_running, n);
    t.n_nodes = level_first;
    t.max_depth = (uint32_t)t.level_start.size() - 1u;
    const size_t places = (size_t)kNodeTris * t.n_nodes;
    TRY(t.nodes.alloc(sizeof(Node8) * (size_t)t.n_nodes));
    HIP_TRY(hipMemcpyAsync(t.nodes.get(), nodes_big, sizeof(Node8) * (size_t)t.n_nodes, hipMemcpyDeviceToDevice, s));
    TRY(t.node_lo.alloc(sizeof(float4) * (size_t)t.n_nodes));
    TRY(t.node_hi.alloc(sizeof(float4) * (size_t)t.n_nodes));
    TRY(t.leaf_prim.alloc(sizeof(uint32_t) * places));
    HIP_TRY(hipMemcpyAsync(t.leaf_prim.get(), leaf_big, sizeof(uint32_t) * places, hipMemcpyDeviceToDevice, s));
    // Woop maps: prim order -> their places (holes stay zero)
    TRY(t.woop.alloc(sizeof(WoopTri) * places));
    HIP_TRY(hipMemsetAsync(t.woop.get(), 0, sizeof(WoopTri) * places, s));
    scatter_woop(t, woop_prim, 0u, n, s);
    DScene d = sg->d;   // the scene's triangles and grid, the new tree's leaves
    d.leaf_prim = as<const uint32_t>(t.leaf_prim);
    refit_levels(d, t, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    t.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    out = std::move(t);
    return LPT_OK;
}

// The current tree's boxes from the shading records as they are now (topology kept), after the padding and grid that follow from them: the padding's
// scene-wide part follows the scene's largest coordinate (ANY growth counts — ADVICE r05 —; it never shrinks).  Blocking.
static int refit(lpt_scene_gpu *sg) {
    hipStream_t s = sg->dev->stream;
    float blo[3], bhi[3];
    TRY(scene_bounds_and_grid(sg, sg->stats.triangles, s, blo, bhi, true));
    refit_levels(sg->d, sg->tree, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return LPT_OK;
}

// what the kernels see of the current tree, and its part of lpt_accel_stats
static void bind_view(lpt_scene_gpu *sg) {
    const DevTree &t = sg->tree;
    sg->d.nodes = as<const DNode8>(t.nodes);
    sg->d.leaf_prim = as<const uint32_t>(t.leaf_prim);
    sg->d.woop = as<const float4>(t.woop);
    // a stack entry holds the unvisited siblings below a node at depth 1..max_depth-1 (the root's own group has one
    // member and is never pushed, the deepest nodes have no inner children): max_depth-1 entries are enough
    sg->d.stack_entries = t.max_depth > 2u ? t.max_depth - 1u : 1u;
    sg->stats.nodes = t.n_nodes;
    sg->stats.max_depth = t.max_depth;
    sg->stats.build_ms = t.build_ms;
}

// The material as the shading records carry it: a material whose albedo and mra textures were paired at upload names the pair.
// Every other texture id is an index into the atlas or LPT_INVALID_INDEX: an id beyond the images means "no texture" (SPEC §9, as
// the oracle reads it) and must not reach the kernel as a value it would take for the paired encoding.  `ok` = false:
// the material samples an image on its own that the atlas does not hold (it was only known as half of a pair at upload time).
static lpt_material device_material(const TexturePairs &p, const lpt_material &m, bool *ok = nullptr) {
    lpt_material d = m;
    if (ok) *ok = true;
    const auto it = p.map.find(std::make_pair(m.albedo_texture, m.mra_texture));
    if (it != p.map.end()) {
        const DImage &di = p.descs[it->second];
        d.albedo_texture = kPairedBit | di.offset;          // in 8-byte texels, < 2^30
        d.mra_texture = di.width | (di.height << 16);       // both <= 65535 (checked when the pair is built)
        return d;
    }
    uint32_t *ids[2] = {&d.albedo_texture, &d.mra_texture};
    for (uint32_t *id : ids) {
        if (*id >= p.image_resident.size()) *id = LPT_INVALID_INDEX;
        else if (!p.image_resident[*id] && ok) *ok = false;
    }
    return d;
}

// Bakes the instances `which` on the device (fp32 transform, cofactor normals, binary64 Woop maps: bit-identical to the host bake): their shading
// records in place, their Woop maps in prim order into `woop_prim`.  Every instance is checked before the first launch.  A non-finite vertex is
// LPT_ERR_ACCEL_BUILD, found before any kernel reads the triangles; the flag is reset for the next bake.
static int bake_instances(lpt_scene_gpu *sg, const lpt_scene &scene, const std::vector<uint32_t> &which, void *woop_prim) {
    std::vector<BakeArgs> args;
    for (uint32_t i : which) {
        const lpt_instance &now = scene.instances[i];
        const uint32_t n = sg->inst_count[i];
        if (!n) continue;
        const lpt_blas_entry &e = scene.entries[now.blas_index];
        if (e.index_count / 3u != n) return fail(LPT_ERR_INVALID_ARG, "triangle count of instance %u changed since the upload", i);
        BakeArgs a;
        memcpy(a.m, now.model_to_world, sizeof a.m);
        const float *m = a.m;
        const float a00 = m[0], a10 = m[1], a20 = m[2], a01 = m[4], a11 = m[5], a21 = m[6], a02 = m[8], a12 = m[9], a22 = m[10];
        a.c[0] = a11 * a22 - a12 * a21; a.c[1] = a12 * a20 - a10 * a22; a.c[2] = a10 * a21 - a11 * a20;   // bvh.cpp bake_instance
        a.c[3] = a02 * a21 - a01 * a22; a.c[4] = a00 * a22 - a02 * a20; a.c[5] = a01 * a20 - a00 * a21;
        a.c[6] = a01 * a12 - a02 * a11; a.c[7] = a02 * a10 - a00 * a12; a.c[8] = a00 * a11 - a01 * a10;
        a.vertex_offset = e.vertex_offset; a.index_offset = e.index_offset; a.first_tri = sg->inst_first[i]; a.n_tris = n;
        a.mirrored = bake_mirrored(m) ? 1u : 0u;
        bool resident = true;
        const lpt_material dm = device_material(sg->pairs, scene.materials[now.material_index < scene.materials.size() ? now.material_index : 0u], &resident);
        if (!resident) return fail(LPT_ERR_INVALID_ARG, "instance %u now samples a texture on its own that was uploaded only as half of an (albedo, mra) pair: upload the scene again", i);
        memcpy(a.mat, &dm, 32);
        args.push_back(a);
    }
    if (args.empty()) return LPT_OK;
    hipStream_t s = sg->dev->stream;
    for (const BakeArgs &a : args)
        hipLaunchKernelGGL(k_bake_instance, dim3(div_up(a.n_tris, 256u)), dim3(256), 0, s, a, as<const float4>(sg->obj_verts), as<const uint32_t>(sg->obj_indices),
                           as<float4>(sg->tri_verts), (float4 *)woop_prim, as<uint32_t>(sg->bad_flag));
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, sg->bad_flag.get(), sizeof bad, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!bad) return LPT_OK;
    HIP_TRY(hipMemsetAsync(sg->bad_flag.get(), 0, sizeof bad, s));
    return fail(LPT_ERR_ACCEL_BUILD, "non-finite vertex in a baked instance");
}

static std::vector<uint32_t> every_instance(const lpt_scene &scene) {
    std::vector<uint32_t> all(scene.instances.size());
    std::iota(all.begin(), all.end(), 0u);
    return all;
}

// update and rebuild: the scene's meshes and instance list must be the ones that were uploaded; anything else needs lpt_scene_upload again
static int check_same_layout(const lpt_scene_gpu *sg, const lpt_scene &scene, const char *fn) {
    if (scene.instances.size() != sg->instances.size() || scene.entries.size() != sg->n_entries ||
        scene.vertices.size() != sg->n_vertices || scene.indices.size() != sg->n_indices)
        return fail(LPT_ERR_INVALID_ARG, "%s: the scene's meshes / instance list changed since the upload; upload again", fn);
    for (size_t i = 0; i < scene.instances.size(); ++i)
        if (scene.instances[i].blas_index != sg->instances[i].blas_index) return fail(LPT_ERR_INVALID_ARG, "%s: instance %zu refers to another mesh; upload again", fn, i);
    return LPT_OK;
}

// ---------------------------------------------------------------------------- upload: host steps
// the GPU build's layout: which run of baked triangles every instance owns (SPEC §2.5 order).  No vertex is touched on the host
static int instance_layout(const lpt_scene &scene, Accel &acc, uint32_t &n_tris) {
    size_t total = 0;
    for (const lpt_instance &in : scene.instances) {
        const uint32_t cnt = in.blas_index < scene.entries.size() ? scene.entries[in.blas_index].index_count / 3u : 0u;
        acc.inst_first.push_back((uint32_t)total);
        acc.inst_count.push_back(cnt);
        total += cnt;
    }
    if (total >= (1u << 29)) return fail(LPT_ERR_ACCEL_BUILD, "too many triangles (%zu)", total);
    n_tris = (uint32_t)total;
    return LPT_OK;
}

// Paired textures: a material that has both an albedo and an mra texture of one size gets the two interleaved — 8 B per texel
// (albedo RGBA8, mra RGBA8) in apron tiles of 128 B — so that ONE set of four taps, in ONE cache line, serves both lookups of a shaded hit:
// 1 line per hit instead of 2 x 1.4 (1.56 with plain 4x4 tiles) (k_shade is bound by HBM traffic, most of it texels).  Lossless: the taps and
// the filter arithmetic are those of two separate lookups.  An image that some material samples on its own (no partner, a partner
// of another size, another partner's pair over the budget) also stays in the tiled atlas; one that only ever appears as half of a
// pair does not (scene.rs:172-184: each image once) — `image_resident`.  Returns the pairs' texels.
static std::vector<uint64_t> pair_textures(const lpt_scene &scene, bool enable, TexturePairs &p) {
    std::vector<uint64_t> texels;
    const size_t budget = (size_t)1 << 30;   // bytes of paired texels per scene
    for (const lpt_material &m : scene.materials) {
        if (!enable) break;
        const uint32_t a = m.albedo_texture, r = m.mra_texture;
        if (a >= scene.images.size() || r >= scene.images.size()) continue;
        const Image &ia = scene.images[a], &ir = scene.images[r];
        if (ia.width != ir.width || ia.height != ir.height || !ia.width || !ia.height || ia.width > 65535u || ia.height > 65535u) continue;
        if (p.map.count(std::make_pair(a, r))) continue;
        // apron tiles (kernels.h texture_lookup_pair): a stored 4x4 tile covers a 3x3 block of the image + its right / lower neighbours
        const uint32_t tx = (ia.width + 2u) / 3u, ty = (ia.height + 2u) / 3u;
        if ((texels.size() + (size_t)tx * ty * 16u) * 8u > budget || texels.size() + (size_t)tx * ty * 16u > 0x3FFFFFFFull) continue;
        DImage di;
        di.offset = (uint32_t)texels.size();   // in 8-byte texels
        di.width = ia.width; di.height = ia.height; di.pad = tx;
        const size_t base = texels.size();
        texels.resize(base + (size_t)tx * ty * 16u, 0);
        for (uint32_t tyi = 0; tyi < ty; ++tyi)
            for (uint32_t txi = 0; txi < tx; ++txi)
                for (uint32_t j = 0; j < 4u; ++j)
                    for (uint32_t i = 0; i < 4u; ++i) {
                        const uint32_t x = (3u * txi + i) % ia.width, y = (3u * tyi + j) % ia.height;   // SPEC §9: repeat wrap
                        uint32_t wa, wr;
                        memcpy(&wa, &ia.rgba8[4u * ((size_t)y * ia.width + x)], 4);
                        memcpy(&wr, &ir.rgba8[4u * ((size_t)y * ir.width + x)], 4);
                        texels[base + ((size_t)tyi * tx + txi) * 16u + j * 4u + i] = (uint64_t)wa | ((uint64_t)wr << 32);
                    }
        p.map[std::make_pair(a, r)] = (uint32_t)p.descs.size();
        p.descs.push_back(di);
    }
    std::vector<uint8_t> paired(scene.materials.size(), 0);
    for (size_t i = 0; i < scene.materials.size(); ++i) paired[i] = p.map.count(std::make_pair(scene.materials[i].albedo_texture, scene.materials[i].mra_texture)) != 0;
    p.image_resident = plain_image_residency(scene, paired);   // material_tables.h: an image a side-table record names stays in the atlas
    return texels;
}

// The tiled atlas of the images the pairs do not hold: texels are stored in 8x4-texel tiles of 128 B (one cache line): the 2x2 bilinear footprint then
// touches 1.4 lines on average instead of 2 (k_shade is bound by L2-miss traffic); `pad` = tiles per row.  Returns the texels, one descriptor per image in `descs`.
static std::vector<uint8_t> tiled_atlas(const lpt_scene &scene, const std::vector<uint8_t> &image_resident, std::vector<DImage> &descs) {
    std::vector<uint8_t> texels;
    for (size_t ii = 0; ii < scene.images.size(); ++ii) {
        const Image &im = scene.images[ii];
        DImage di;
        di.offset = (uint32_t)(texels.size() / 4);
        if (!image_resident[ii]) {   // only ever half of a pair: lives in the pairs' texels, no shading record carries its id
            di.width = di.height = di.pad = 0u;
            descs.push_back(di);
            continue;
        }
        di.width = im.width; di.height = im.height;
        const uint32_t tx = (im.width + 7u) / 8u, ty = (im.height + 3u) / 4u;
        di.pad = tx;
        descs.push_back(di);
        const size_t base = texels.size();
        texels.resize(base + (size_t)tx * ty * 128u, 0);
        for (uint32_t y = 0; y < im.height; ++y)
            for (uint32_t x = 0; x < im.width; ++x)
                memcpy(&texels[base + 4u * (((size_t)(y >> 2) * tx + (x >> 3)) * 32u + (y & 3u) * 8u + (x & 7u))], &im.rgba8[4u * ((size_t)y * im.width + x)], 4);
    }
    return texels;
}

// shading records (kernels.h DScene::tri_verts) of the host-baked triangles: three vertices + the material, 128 B per triangle
struct TriRec { float4 v[kTriRec]; };
static_assert(sizeof(TriRec) == 128 && sizeof(lpt_vertex) * 3 == 96 && sizeof(lpt_material) == 32, "shading record layout");
static std::vector<TriRec> shading_records(const lpt_scene &scene, const Accel &acc, const TexturePairs &p) {
    std::vector<TriRec> recs(acc.tri_material.size());
    for (size_t t = 0; t < recs.size(); ++t) {
        memcpy(recs[t].v, &acc.tri_verts[3 * t], 96);
        const lpt_material dm = device_material(p, scene.materials[acc.tri_material[t] < scene.materials.size() ? acc.tri_material[t] : 0]);
        memcpy(&recs[t].v[6], &dm, 32);
    }
    return recs;
}

extern "C" {

// ============================================================================ Device
int lpt_device_create(int hip_ordinal, lpt_device **out) {
    if (!out) return fail(LPT_ERR_INVALID_ARG, "lpt_device_create: null out");
    // A renderer spreads its work over several HIP streams (wavefront lanes, several renderers in flight).  The ROCm runtime
    // maps streams onto a fixed number of hardware queues (the machine's setting) and streams that share a queue serialise
    // (INTEGRATION.md §8).  The library does not touch the process environment.
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(LPT_ERR_HIP, "no HIP device visible (%s); this library has no CPU fallback", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (hip_ordinal < 0 || hip_ordinal >= n) return fail(LPT_ERR_INVALID_ARG, "HIP ordinal %d out of range (%d devices)", hip_ordinal, n);
    HIP_TRY(hipSetDevice(hip_ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, hip_ordinal));
    lpt_device *d = new (std::nothrow) lpt_device();
    if (!d) return fail(LPT_ERR_INVALID_ARG, "out of host memory");
    d->ordinal = hip_ordinal;
    d->compute_units = prop.multiProcessorCount;
    snprintf(d->name, sizeof d->name, "%s (%s)", prop.name, prop.gcnArchName);
    const int st = d->stream.create();
    if (st != LPT_OK) { delete d; return st; }
    *out = d;
    return LPT_OK;
}

int lpt_device_destroy(lpt_device *dev) {
    if (!dev) return LPT_OK;
    hipSetDevice(dev->ordinal);
    hipStreamSynchronize(dev->stream);
    delete dev;   // its stream with it
    return LPT_OK;
}

int lpt_device_synchronize(lpt_device *dev) {
    if (!dev) return fail(LPT_ERR_INVALID_ARG, "lpt_device_synchronize: null");
    HIP_TRY(hipStreamSynchronize(dev->stream));
    return LPT_OK;
}

int lpt_device_info(lpt_device *dev, char *name, size_t cap, int *cus) {
    if (!dev) return fail(LPT_ERR_INVALID_ARG, "lpt_device_info: null");
    if (name && cap) snprintf(name, cap, "%s", dev->name);
    if (cus) *cus = dev->compute_units;
    return LPT_OK;
}

int lpt_device_stream(lpt_device *dev, void **stream) {
    if (!dev || !stream) return fail(LPT_ERR_INVALID_ARG, "lpt_device_stream: null");
    *stream = (void *)dev->stream;
    return LPT_OK;
}

// ============================================================================ SceneGPU
int lpt_scene_gpu_destroy(lpt_scene_gpu *sg) {
    if (!sg) return LPT_OK;
    hipSetDevice(sg->dev->ordinal);
    flush_device(sg->dev);
    hipDeviceSynchronize();   // renderers trace on their own streams: frames still in flight read what is freed here
    // a renderer still bound to this scene is detached (a host that drops the scene first must not leave the renderer with a dangling
    // pointer): its next raytrace() is the no-op of a renderer without resources (renderer.rs:403-407) until set_resources is called again
    for (lpt_renderer *r : sg->dev->renderers)
        if (r->sg == sg) { r->sg = nullptr; r->resources_set = false; }
    delete sg;   // its device memory with it
    return LPT_OK;
}

// the scene's punctual lights onto the device (SPEC §19) and into the view the kernels get; the caller has made sure nothing in flight reads the old ones
static int upload_punctual(lpt_scene_gpu *sg, const lpt_scene &scene) {
    static_assert(sizeof(lpt_punctual_light) == 4 * sizeof(float4), "a punctual light is four float4 rows");
    const uint32_t n = (uint32_t)scene.punctual.size();
    hipStream_t s = sg->dev->stream;
    if (n != sg->d.n_punctual || !sg->punctual) TRY(sg->punctual.alloc(sizeof(lpt_punctual_light) * std::max<size_t>(n, 1u)));
    if (n) HIP_TRY(hipMemcpyAsync(sg->punctual.get(), scene.punctual.data(), sizeof(lpt_punctual_light) * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // the host vector is the caller's
    sg->d.punctual = as<const float4>(sg->punctual);
    sg->d.n_punctual = n;
    return LPT_OK;
}

// SPEC §20, §21, §22, §24, §28: one material side table (material_tables.h) onto the device and into the view the kernels get; the caller has made sure nothing in flight
// reads the old tables, and waits for the stream before the host vectors go
struct DSceneTable { const uint32_t *DScene::*tri; const float4 *DScene::*recs; uint32_t DScene::*n; };
static const DSceneTable kDSceneTables[MAT_KINDS] = {
    {&DScene::alpha_tri, &DScene::alpha_recs, &DScene::n_alpha},
    {&DScene::trans_tri, &DScene::trans_recs, &DScene::n_trans},
    {&DScene::emis_tri, &DScene::emis_recs, &DScene::n_emis},
    {&DScene::nmap_tri, &DScene::nmap_recs, &DScene::n_nmap},
};
static int commit_table(lpt_scene_gpu *sg, int kind, const MaterialTable &t) {
    auto &mem = sg->mat_tab[kind];
    const DSceneTable &view = kDSceneTables[kind];
    if (t.recs.empty()) {
        mem.tri.reset(); mem.recs.reset();
        sg->d.*view.tri = nullptr; sg->d.*view.recs = nullptr; sg->d.*view.n = 0u;
        return LPT_OK;
    }
    TRY(upload(mem.tri, t.tri, sg->dev->stream));
    // SPEC §28: the second records (the transmission table's sigma rows) stand behind the first ones, record i's at [n + i] — there only while some record needs one
    TRY(mem.recs.alloc(sizeof(MaterialRec) * (t.recs.size() + t.more.size())));
    HIP_TRY(hipMemcpyAsync(mem.recs.get(), t.recs.data(), sizeof(MaterialRec) * t.recs.size(), hipMemcpyHostToDevice, sg->dev->stream));
    if (!t.more.empty())
        HIP_TRY(hipMemcpyAsync(mem.recs.get() + sizeof(MaterialRec) * t.recs.size(), t.more.data(), sizeof(MaterialRec) * t.more.size(), hipMemcpyHostToDevice, sg->dev->stream));
    sg->d.*view.tri = as<const uint32_t>(mem.tri);
    sg->d.*view.recs = as<const float4>(mem.recs);
    sg->d.*view.n = (uint32_t)t.recs.size();
    return LPT_OK;
}

// SPEC §23: the emitter distribution of the scene as it is now (emit_dist.cpp: the emissive instances baked on the host, so nothing is read back), derived and
// committed beside the emission tables — at upload, rebuild and every instance update, since the weights are world-space areas.  The cost is a host bake of every
// emissive instance (bake_instance: normals too, which the distribution does not read) on every update, also one that moves no emitter: linear in the emissive
// triangles, meant for lamps of a few thousand triangles, not for a scene that is mostly emissive.
struct EmitTable { std::vector<float4> tab; float inv_W = 0.0f; };
static int derive_emit(const lpt_scene_gpu *sg, const lpt_scene &scene, EmitTable &out) {
    EmitDist dist;
    emitter_distribution(scene, dist);
    out = EmitTable();
    for (size_t i = 0; i < dist.prim.size(); ++i) {
        if (dist.prim[i] >= sg->d.n_tris) return fail(LPT_ERR_INVALID_ARG, "emissive triangle %u lies beyond the %u baked triangles", dist.prim[i], sg->d.n_tris);
        out.tab.push_back(make_float4(dist.q[i], bits_as_float(dist.alias[i]), bits_as_float(dist.prim[i]), bits_as_float(dist.prim[dist.alias[i]])));
    }
    if (!out.tab.empty()) out.inv_W = (float)(1.0 / dist.sum_w);
    return LPT_OK;
}
static int commit_emit(lpt_scene_gpu *sg, const EmitTable &et) {
    DScene &d = sg->d;
    if (et.tab.empty() || !d.n_emis) {
        sg->emit_tab.reset();
        d.emit_tab = nullptr; d.n_emit = 0u; d.emit_inv_W = 0.0f;
        return LPT_OK;
    }
    hipStream_t s = sg->dev->stream;
    TRY(upload(sg->emit_tab, et.tab, s));
    d.emit_tab = as<const float4>(sg->emit_tab);
    d.n_emit = (uint32_t)et.tab.size();
    d.emit_inv_W = et.inv_W;
    return LPT_OK;
}

// Everything the device keeps per triangle of the scene's materials: the four side tables and the emitter distribution.  Derived on the host (an edit is checked
// before anything is baked), committed together — at upload, rebuild and every instance update.  The distribution goes last: commit_emit reads the committed n_emis.
struct SceneTables { MaterialTable mat[MAT_KINDS]; EmitTable emit; uint32_t n_thin_glass = 0; };
static int derive_tables(const lpt_scene_gpu *sg, const lpt_scene &scene, SceneTables &out) {
    TRY(derive_material_tables(scene, sg->inst_first, sg->inst_count, sg->d.n_tris, sg->pairs.image_resident, out.mat));
    out.n_thin_glass = thin_glass_triangles(out.mat[MAT_TRANS]);   // SPEC §27
    return derive_emit(sg, scene, out.emit);
}
static int commit_tables(lpt_scene_gpu *sg, const SceneTables &t) {
    int st = LPT_OK;
    for (int k = 0; k < MAT_KINDS && st == LPT_OK; ++k) st = commit_table(sg, k, t.mat[k]);
    if (st == LPT_OK) st = commit_emit(sg, t.emit);
    if (st == LPT_OK) sg->n_thin_glass = t.n_thin_glass;
    HIP_TRY(hipStreamSynchronize(sg->dev->stream));   // the host vectors are the caller's: waited for behind a failed upload too
    return st;
}

int lpt_scene_upload(lpt_device *dev, const lpt_scene *scene, lpt_scene_gpu **out) { return lpt_scene_upload_ex(dev, scene, LPT_ACCEL_BUILD_HOST_SAH, out); }

int lpt_scene_upload_ex(lpt_device *dev, const lpt_scene *scene, uint32_t flags, lpt_scene_gpu **out) {
    if (!dev || !scene || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_upload: null");
    if ((flags & ~LPT_UPLOAD_NO_TEXTURE_PAIRS) > LPT_ACCEL_BUILD_GPU_LBVH) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_upload_ex: unknown flags %u", flags);
    const bool enable_pairs = !(flags & LPT_UPLOAD_NO_TEXTURE_PAIRS);
    flags &= ~LPT_UPLOAD_NO_TEXTURE_PAIRS;
    HIP_TRY(hipSetDevice(dev->ordinal));
    const auto t_upload = std::chrono::steady_clock::now();
    // the layout; the host bake and build unless the GPU builds the tree (tiny scenes always go to the host builder: a radix tree needs >= 2 leaves)
    Accel acc;
    uint32_t n_tris = 0;
    bool gpu_build = flags == LPT_ACCEL_BUILD_GPU_LBVH;
    if (gpu_build) {
        TRY(instance_layout(*scene, acc, n_tris));
        gpu_build = n_tris >= 16u;
    }
    if (!gpu_build) {
        TRY(bake_and_build(*scene, acc));
        n_tris = (uint32_t)acc.tri_material.size();
    }
    TexturePairs pairs;
    const std::vector<uint64_t> pair_texels = pair_textures(*scene, enable_pairs, pairs);
    std::vector<DImage> descs;
    const std::vector<uint8_t> texels = tiled_atlas(*scene, pairs.image_resident, descs);
    const std::vector<TriRec> recs = gpu_build ? std::vector<TriRec>() : shading_records(*scene, acc, pairs);
    std::vector<float> lut(256);
    for (int i = 0; i < 256; ++i) {
        const double c = (double)i / 255.0;
        lut[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
    const std::vector<uint32_t> zero(1, 0u);

    // the upload (the host vectors above outlive it: a failure destroys the scene, which waits for the device)
    std::unique_ptr<lpt_scene_gpu, int (*)(lpt_scene_gpu *)> sg(new lpt_scene_gpu(), lpt_scene_gpu_destroy);
    sg->dev = dev;
    sg->pairs = std::move(pairs);
    hipStream_t s = dev->stream;
    if (gpu_build) {
        TRY(sg->tri_verts.alloc(sizeof(TriRec) * (size_t)n_tris));   // written by k_bake_instance
    } else {   // the host-built tree; its boxes are filled by the first refit
        DevTree &t = sg->tree;
        t.n_nodes = (uint32_t)acc.nodes.size();
        t.max_depth = acc.max_depth;
        t.level_start = acc.level_start;
        t.build_ms = acc.build_ms;
        TRY(upload(t.nodes, acc.nodes, s));
        TRY(upload(t.woop, acc.woop, s));
        TRY(upload(t.leaf_prim, acc.leaf_prim, s));
        const size_t box_bytes = sizeof(float4) * std::max<size_t>(t.n_nodes, 1u);
        TRY(t.node_lo.alloc(box_bytes));
        TRY(t.node_hi.alloc(box_bytes));
        HIP_TRY(hipMemsetAsync(t.node_lo.get(), 0, box_bytes, s));
        HIP_TRY(hipMemsetAsync(t.node_hi.get(), 0, box_bytes, s));
        TRY(upload(sg->tri_verts, recs, s));
    }
    TRY(upload(sg->materials, scene->materials, s));
    TRY(upload(sg->lights, scene->lights, s));
    TRY(upload(sg->images, descs, s));
    TRY(upload(sg->texels, texels, s));
    TRY(upload(sg->pair_images, sg->pairs.descs, s));
    TRY(upload(sg->pair_texels, pair_texels, s));
    TRY(upload(sg->srgb_lut, lut, s));
    TRY(upload(sg->obj_verts, scene->vertices, s));
    TRY(upload(sg->obj_indices, scene->indices, s));
    TRY(upload(sg->bad_flag, zero, s));
    HIP_TRY(hipStreamSynchronize(s));
    sg->inst_first = acc.inst_first; sg->inst_count = acc.inst_count;
    sg->instances = scene->instances;
    sg->n_entries = scene->entries.size(); sg->n_vertices = scene->vertices.size(); sg->n_indices = scene->indices.size();

    DScene &d = sg->d;
    sg->max_abs = acc.max_abs;      // 0 on the GPU-build path: build_lbvh sets it from its bounds pass
    d.pad_abs = kScenePad * acc.max_abs;
    for (int a = 0; a < 3; ++a) { d.grid_lo[a] = acc.grid_lo[a]; d.grid_step[a] = acc.grid_step[a]; }   // (the GPU-build path: build_lbvh sets its own)
    d.tri_verts = as<const float4>(sg->tri_verts);
    d.materials = as<const lpt_material>(sg->materials);
    d.lights = as<const lpt_light>(sg->lights);
    d.texels = as<const uint8_t>(sg->texels);
    d.images = as<const DImage>(sg->images);
    d.srgb_lut = as<const float>(sg->srgb_lut);
    d.pair_texels = as<const uint2>(sg->pair_texels);
    d.pair_images = as<const DImage>(sg->pair_images);
    d.n_pairs = (uint32_t)sg->pairs.descs.size();
    d.n_tris = n_tris;
    d.n_materials = (uint32_t)scene->materials.size();
    d.n_lights = (uint32_t)scene->lights.size();
    d.n_images = (uint32_t)scene->images.size();
    TRY(upload_punctual(sg.get(), *scene));
    {
        SceneTables tables;
        TRY(derive_tables(sg.get(), *scene, tables));
        TRY(commit_tables(sg.get(), tables));
    }
    sg->stats.triangles = d.n_tris;
    sg->stats.node_bytes = (uint32_t)sizeof(Node8);
    sg->stats.tri_bytes = (uint32_t)sizeof(WoopTri);
    sg->stats.host_baked_triangles = gpu_build ? 0u : n_tris;
    sg->stats.texture_bytes_resident = (uint64_t)texels.size() + 8u * (uint64_t)pair_texels.size();
    sg->stats.texture_pairs = d.n_pairs;

    if (gpu_build) {   // bake every instance on the device, then build the tree there
        DevMem woop_prim;
        TRY(woop_prim.alloc(sizeof(WoopTri) * (size_t)n_tris));
        TRY(bake_instances(sg.get(), *scene, every_instance(*scene), woop_prim.get()));
        TRY(build_lbvh(sg.get(), n_tris, woop_prim.get(), s, sg->tree));
    }
    bind_view(sg.get());
    sg->stats.upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_upload).count();
    *out = sg.release();
    return LPT_OK;
}

int lpt_scene_gpu_stats(const lpt_scene_gpu *sg, lpt_accel_stats *out) {
    if (!sg || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_stats: null");
    *out = sg->stats;
    return LPT_OK;
}

// Interactive edit (reference: Instance::set_transform, crates/standalone/src/lib.rs:118-121, followed by a new
// SceneGPU): re-bake the instances whose transform / material changed, upload their triangles and REFIT the wide
// BVH on the GPU (topology kept, all boxes recomputed level by level).  The scene's meshes and instance list
// must be the ones that were uploaded; anything else needs lpt_scene_upload again.
int lpt_scene_gpu_update_instances(lpt_scene_gpu *sg, const lpt_scene *scene, uint32_t *out_rebaked) {
    if (!sg || !scene) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_update_instances: null");
    TRY(check_same_layout(sg, *scene, "lpt_scene_gpu_update_instances"));
    HIP_TRY(hipSetDevice(sg->dev->ordinal));
    // renderers trace on their own streams and raytrace() is asynchronous: frames still in flight read the triangles and
    // nodes this call rewrites in place, so wait for every stream of the device first
    TRY(flush_device(sg->dev));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> changed;
    for (size_t i = 0; i < scene->instances.size(); ++i)
        if (memcmp(&scene->instances[i], &sg->instances[i], sizeof(lpt_instance)) != 0) changed.push_back((uint32_t)i);
    if (!changed.empty()) {
        // an instance whose material changed may have become masked, transmissive, emissive or normal-mapped, or stopped being so, and the emitter distribution
        // weighs world-space areas (SPEC §20 - §24); checked before anything is baked
        SceneTables tables;
        TRY(derive_tables(sg, *scene, tables));
        // re-bake on the device (the object-space meshes are resident, only the transforms travel); a place-driven scatter then takes the new
        // Woop maps to every place a triangle has in the tree (a split triangle has several)
        DevMem woop_prim;
        TRY(woop_prim.alloc(sizeof(WoopTri) * (size_t)std::max(sg->stats.triangles, 1u)));
        const int st = bake_instances(sg, *scene, changed, woop_prim.get());
        if (st == LPT_ERR_INVALID_ARG) return st;   // found before anything was baked
        // recorded as baked even when a vertex was not finite: the next valid edit of the instance re-bakes it
        for (uint32_t i : changed) {
            sg->instances[i] = scene->instances[i];
            if (sg->inst_count[i]) scatter_woop(sg->tree, woop_prim.get(), sg->inst_first[i], sg->inst_count[i], sg->dev->stream);
        }
        if (st != LPT_OK) return st;
        TRY(commit_tables(sg, tables));
        if (sg->stats.triangles) TRY(refit(sg));
    }
    if (out_rebaked) *out_rebaked = (uint32_t)changed.size();
    return LPT_OK;
}

// Full rebuild on the GPU for scenes whose instances moved far (a refit keeps the old topology and degrades): every
// instance is re-baked on the device and the tree is rebuilt there (build_kernels.h).  Same preconditions as
// lpt_scene_gpu_update_instances; scenes of fewer than 16 triangles are refitted instead.
int lpt_scene_gpu_rebuild(lpt_scene_gpu *sg, const lpt_scene *scene) {
    if (!sg || !scene) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_rebuild: null");
    TRY(check_same_layout(sg, *scene, "lpt_scene_gpu_rebuild"));
    const uint32_t n = sg->stats.triangles;
    if (n < 16u) {
        TRY(lpt_scene_gpu_update_instances(sg, scene, nullptr));   // (flushes and waits first)
        SceneTables tables;   // a rebuild re-derives the tables whether or not an instance changed
        TRY(derive_tables(sg, *scene, tables));
        TRY(commit_tables(sg, tables));
        return upload_punctual(sg, *scene);
    }
    HIP_TRY(hipSetDevice(sg->dev->ordinal));
    TRY(flush_device(sg->dev));
    HIP_TRY(hipDeviceSynchronize());  // frames in flight on the renderers' streams still read what is rebuilt here
    TRY(upload_punctual(sg, *scene));   // lights are scene data: a rebuild carries them too, whatever their number (SPEC §19)
    {
        SceneTables tables;   // ... and so are the materials' side tables and the emitter distribution (SPEC §20 - §24)
        TRY(derive_tables(sg, *scene, tables));
        TRY(commit_tables(sg, tables));
    }
    DevMem woop_prim;
    TRY(woop_prim.alloc(sizeof(WoopTri) * (size_t)n));
    TRY(bake_instances(sg, *scene, every_instance(*scene), woop_prim.get()));
    // the new tree replaces the old one only when its build succeeds: bound renderers and later updates never see freed memory
    DevTree t;
    const int st = build_lbvh(sg, n, woop_prim.get(), sg->dev->stream, t);
    if (st == LPT_OK) {
        sg->tree = std::move(t);
        bind_view(sg);
    } else {
        // the shading records were re-baked in place: put the old tree in step with them as an update does (new Woop maps into the old leaf
        // order, boxes refitted, topology kept); the refit also replaces the grid build_lbvh had set for the new tree
        scatter_woop(sg->tree, woop_prim.get(), 0u, n, sg->dev->stream);
        refit(sg);
    }
    sg->instances = scene->instances;  // what is baked now
    return st;
}

// SPEC §19: the punctual lights again, nothing else.  Recorded raytrace() calls are submitted first and see the lights they were recorded with
// (the rule of lpt_scene_gpu_update_instances); the records are rewritten in place, so every stream of the device is waited for.
int lpt_scene_gpu_update_punctual(lpt_scene_gpu *sg, const lpt_scene *scene) {
    if (!sg || !scene) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_update_punctual: null");
    if (scene->punctual.size() != (size_t)sg->d.n_punctual)
        return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_update_punctual: the scene has %zu punctual lights, %u were uploaded (lpt_scene_gpu_rebuild or a new upload takes a changed count)",
                    scene->punctual.size(), sg->d.n_punctual);
    HIP_TRY(hipSetDevice(sg->dev->ordinal));
    TRY(flush_device(sg->dev));
    HIP_TRY(hipDeviceSynchronize());
    return upload_punctual(sg, *scene);
}

// ============================================================================ ProbeGPU
int lpt_probe_upload(lpt_device *dev, const uint8_t *rgbe8, uint32_t w, uint32_t h, lpt_probe **out) {
    if (!dev || !rgbe8 || !w || !h || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_probe_upload: null or empty");
    HIP_TRY(hipSetDevice(dev->ordinal));
    std::unique_ptr<lpt_probe> p(new lpt_probe());
    p->dev = dev;
    TRY(p->rgbe.alloc((size_t)w * h * 4));
    HIP_TRY(hipMemcpy(p->rgbe, rgbe8, (size_t)w * h * 4, hipMemcpyHostToDevice));
    p->d.rgbe = as<const uint8_t>(p->rgbe);
    p->d.w = w; p->d.h = h;
    *out = p.release();
    return LPT_OK;
}

// The probe's distribution (SPEC §18; env_dist.cpp) on the device, built the first time it is asked for; false: the probe has none.
// The texels come back from the device, so that a probe keeps no host copy for a mode it may never be used with.
static int probe_env(lpt_probe *p, bool &has) {
    if (!p->env_state) {
        const uint32_t W = p->d.w, H = p->d.h;
        std::vector<uint8_t> rgbe((size_t)W * H * 4);
        HIP_TRY(hipSetDevice(p->dev->ordinal));
        HIP_TRY(hipMemcpy(rgbe.data(), p->rgbe, rgbe.size(), hipMemcpyDeviceToHost));
        lpt::EnvDist d;
        if (lpt::env_distribution(rgbe.data(), W, H, d) > 0.0) {
            const size_t n = (size_t)W * H;
            std::vector<float4> tab(H + n);
            for (uint32_t y = 0; y < H; ++y) tab[y] = make_float4(d.row_q[y], bits_as_float(d.row_alias[y]), 0.0f, 0.0f);
            for (size_t i = 0; i < n; ++i) {
                const size_t a = i - i % W + d.col_alias[i];   // the alias's place: same row
                tab[H + i] = make_float4(d.col_q[i], bits_as_float(d.col_alias[i]), d.pdf_uv[i], d.pdf_uv[a]);
            }
            DevBuf<float4> buf;   // the probe's only once it holds the table
            TRY(buf.alloc(tab.size()));
            HIP_TRY(hipMemcpy(buf, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice));
            p->env_buf = std::move(buf);
            const float4 *b = p->env_buf;
            p->env = DEnv{b, b + H, W, H};
            p->env_state = 1;
        } else {
            p->env_state = 2;
        }
    }
    has = p->env_state == 1;
    return LPT_OK;
}

int lpt_probe_destroy(lpt_probe *p) {
    if (!p) return LPT_OK;
    hipSetDevice(p->dev->ordinal);
    flush_device(p->dev);
    hipDeviceSynchronize();   // frames in flight on the renderers' streams may still sample the probe
    for (lpt_renderer *r : p->dev->renderers)   // a renderer still bound to it falls back to the 1x1 default probe (renderer.rs:693-696)
        if (r->probe == p) r->probe = nullptr;
    delete p;   // its device memory with it
    return LPT_OK;
}

// ============================================================================ per-element probes
// One device function of the shading or traversal kernels over n caller-supplied elements, for tests and tools.  The kernels and their rows are probe_kernels.h's and
// the upload / launch / read-back is run_probe's (n == 0 returns there, before the device is touched); what is left here is what each call checks and how the ABI's
// arrays become rows and back.
constexpr size_t kF1 = sizeof(float), kF3 = sizeof(float[3]);
static_assert(sizeof(lpt_hit) == sizeof(float4), "k_query_closest writes lpt_hit as one float4");

// SPEC §19: punctual_sample of light `light_index`, once per point
int lpt_scene_gpu_sample_punctual(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t light_index, const float *points, uint32_t n, float *wi, float *dist, float *E) {
    if (!dev || !sg || (n && (!points || !wi || !dist || !E))) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_punctual: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_punctual: the scene belongs to another device");
    if (light_index >= sg->d.n_punctual) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_punctual: light %u of %u", light_index, sg->d.n_punctual);
    return run_probe(dev, n, kBlock, {{points, kF3}}, {{wi, kF3}, {dist, kF1}, {E, kF3}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_punctual_sample, grid, dim3(kBlock), 0, dev->stream, sg->d, light_index, as<const float>(d[0]), n, as<float>(d[1]), as<float>(d[2]), as<float>(d[3]));
    });
}

// SPEC §23: emitter_sample, once per point with its (ra, rb, r1, r2)
int lpt_scene_gpu_sample_emitter(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const float *points, const float *rands, uint32_t *prim, uint32_t *sampled, float *y,
                                 float *wi, float *dist, float *cl, float *p_a, float *E) {
    if (!dev || !sg || (n && (!points || !rands || !prim || !sampled || !y || !wi || !dist || !cl || !p_a || !E))) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_emitter: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_emitter: the scene belongs to another device");
    if (!sg->d.n_emit) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_emitter: the scene has no emitter distribution");
    std::vector<EmitterRow> rows(n);
    TRY((run_probe(dev, n, kBlock, {{points, kF3}, {rands, sizeof(float[4])}}, {{rows.data(), sizeof(EmitterRow)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_emitter_sample, grid, dim3(kBlock), 0, dev->stream, sg->d, as<const float>(d[0]), as<const float>(d[1]), n, as<EmitterRow>(d[2]));
    })));
    for (size_t i = 0; i < n; ++i) {
        const EmitterRow &r = rows[i];
        prim[i] = r.prim; sampled[i] = r.sampled; dist[i] = r.dist; cl[i] = r.cl; p_a[i] = r.p_a;
        memcpy(y + 3u * i, r.y, kF3); memcpy(wi + 3u * i, r.wi, kF3); memcpy(E + 3u * i, r.E, kF3);
    }
    return LPT_OK;
}

// SPEC §24: the shading normal of a hit (§12's, through normal_map where the triangle has a map), once per (prim, bary, direction)
int lpt_scene_gpu_shading_normal(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *bary, const float *dirs, float *ns_out, uint32_t *mapped_out) {
    if (!dev || !sg || (n && (!prim || !bary || !dirs || !ns_out || !mapped_out))) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_shading_normal: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_shading_normal: the scene belongs to another device");
    TRY(check_prims("lpt_scene_gpu_shading_normal", sg->d, prim, n));
    std::vector<NormalRow> rows(n);
    TRY((run_probe(dev, n, kBlock, {{prim, sizeof(uint32_t)}, {bary, sizeof(float[2])}, {dirs, kF3}}, {{rows.data(), sizeof(NormalRow)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_shading_normal, grid, dim3(kBlock), 0, dev->stream, sg->d, as<const uint32_t>(d[0]), as<const float>(d[1]), as<const float>(d[2]), n, as<NormalRow>(d[3]));
    })));
    for (size_t i = 0; i < n; ++i) {
        memcpy(ns_out + 3u * i, rows[i].Ns, kF3);
        mapped_out[i] = rows[i].mapped;
    }
    return LPT_OK;
}

// SPEC §27: glass_shadow_eval — what a marked shadow ray along dirs[i] asks at the hit (prim, bary) —, once per element.  out[n] is the row {tau rgb, xi, pass bits, 0, 0, 0}
int lpt_scene_gpu_glass_shadow(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *bary, const float *dirs, float *out) {
    if (!dev || !sg || (n && (!prim || !bary || !dirs || !out))) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_glass_shadow: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_glass_shadow: the scene belongs to another device");
    TRY(check_prims("lpt_scene_gpu_glass_shadow", sg->d, prim, n));
    return run_probe(dev, n, kBlock, {{prim, sizeof(uint32_t)}, {bary, sizeof(float[2])}, {dirs, kF3}}, {{out, sizeof(GlassRow)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_glass_shadow, grid, dim3(kBlock), 0, dev->stream, sg->d, as<const uint32_t>(d[0]), as<const float>(d[1]), as<const float>(d[2]), n, as<GlassRow>(d[3]));
    });
}

// SPEC §28: volume_attenuate — what a hit of baked triangle prim[i] by a ray along dirs[i] at distance t[i] does to a throughput of 1 —, once per element.  out[n] is {A rgb, applies}
int lpt_scene_gpu_attenuation(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *dirs, const float *t, float *out) {
    if (!dev || !sg || (n && (!prim || !dirs || !t || !out))) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_attenuation: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_attenuation: the scene belongs to another device");
    TRY(check_prims("lpt_scene_gpu_attenuation", sg->d, prim, n));
    return run_probe(dev, n, kBlock, {{prim, sizeof(uint32_t)}, {dirs, kF3}, {t, sizeof(float)}}, {{out, sizeof(float4)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_attenuation, grid, dim3(kBlock), 0, dev->stream, sg->d, as<const uint32_t>(d[0]), as<const float>(d[1]), as<const float>(d[2]), n, as<float4>(d[3]));
    });
}

// SPEC §9: what a hit reads from its textures (shade_hit's dispatch over texture_lookup / texture_lookup_pair / alpha_rejects), once per (prim, bary).  out[n] is the row
int lpt_scene_gpu_sample_textures(lpt_device *dev, const lpt_scene_gpu *sg, uint32_t n, const uint32_t *prim, const float *bary, float *out) {
    if (!dev || !sg || (n && (!prim || !bary || !out))) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_textures: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_scene_gpu_sample_textures: the scene belongs to another device");
    TRY(check_prims("lpt_scene_gpu_sample_textures", sg->d, prim, n));
    return run_probe(dev, n, kBlock, {{prim, sizeof(uint32_t)}, {bary, sizeof(float[2])}}, {{out, sizeof(TextureRow)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_sample_textures, grid, dim3(kBlock), 0, dev->stream, sg->d, as<const uint32_t>(d[0]), as<const float>(d[1]), n, as<TextureRow>(d[2]));
    });
}

// SPEC §21: interface_sample, once per element
int lpt_interface_sample(lpt_device *dev, uint32_t n, const float *dirs, const float *ns, const float *ngf, const uint32_t *entering, const float *base, const float *ior,
                         const uint32_t *thin, const float *r4, float *wi, float *weight, uint32_t *kind) {
    if (!dev || (n && (!dirs || !ns || !ngf || !entering || !base || !ior || !thin || !r4 || !wi || !weight || !kind))) return fail(LPT_ERR_INVALID_ARG, "lpt_interface_sample: null");
    std::vector<InterfaceRowIn> in(n);
    for (size_t i = 0; i < n; ++i) {
        InterfaceRowIn &e = in[i];
        memcpy(e.d, dirs + 3u * i, kF3); memcpy(e.Ns, ns + 3u * i, kF3); memcpy(e.Ngf, ngf + 3u * i, kF3); memcpy(e.base, base + 3u * i, kF3);
        e.ior = ior[i]; e.r4 = r4[i];
        e.entering = entering[i] ? 1u : 0u; e.thin = thin[i] ? 1u : 0u;
    }
    std::vector<InterfaceRowOut> res(n);
    TRY((run_probe(dev, n, kBlock, {{in.data(), sizeof(InterfaceRowIn)}}, {{res.data(), sizeof(InterfaceRowOut)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_interface_sample, grid, dim3(kBlock), 0, dev->stream, as<const InterfaceRowIn>(d[0]), n, as<InterfaceRowOut>(d[1]));
    })));
    for (size_t i = 0; i < n; ++i) {
        memcpy(wi + 3u * i, res[i].wi, kF3); memcpy(weight + 3u * i, res[i].weight, kF3);
        kind[i] = res[i].kind;
    }
    return LPT_OK;
}

// SPEC §29: interface_sample_rough with the rough bit set, once per element.  in[n] is the row; out[n] = {wi, weight}: the row without its `kind`
int lpt_interface_sample_rough(lpt_device *dev, uint32_t n, const float *in, float *out, uint32_t *kind) {
    if (!dev || (n && (!in || !out || !kind))) return fail(LPT_ERR_INVALID_ARG, "lpt_interface_sample_rough: null");
    std::vector<RoughRowOut> res(n);
    TRY((run_probe(dev, n, kBlock, {{in, sizeof(RoughRowIn)}}, {{res.data(), sizeof(RoughRowOut)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_interface_sample_rough, grid, dim3(kBlock), 0, dev->stream, as<const RoughRowIn>(d[0]), n, as<RoughRowOut>(d[1]));
    })));
    for (size_t i = 0; i < n; ++i) {
        RoughAbiOut o;
        memcpy(o.wi, res[i].wi, kF3); memcpy(o.weight, res[i].weight, kF3);
        memcpy(out + 6u * i, &o, sizeof o);
        kind[i] = res[i].kind;
    }
    return LPT_OK;
}

// SPEC §10: the BSDF as shade_hit sets it up (device_math.h make_surface, spec_probability, bsdf_eval, bsdf_sample), once per element.  in[n] is the row;
// out[n] = {pspec, f, pdf}, then {L_s, weight, pdf_s}: the row without its `ok`
int lpt_bsdf_probe(lpt_device *dev, uint32_t n, const float *in, float *out, uint32_t *ok) {
    if (!dev || (n && (!in || !out || !ok))) return fail(LPT_ERR_INVALID_ARG, "lpt_bsdf_probe: null");
    std::vector<BsdfRowOut> res(n);
    TRY((run_probe(dev, n, kBlock, {{in, sizeof(BsdfRowIn)}}, {{res.data(), sizeof(BsdfRowOut)}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_bsdf_probe, grid, dim3(kBlock), 0, dev->stream, as<const BsdfRowIn>(d[0]), n, as<BsdfRowOut>(d[1]));
    })));
    for (size_t i = 0; i < n; ++i) {
        const BsdfAbiOut o{res[i].eval, res[i].sampled};
        memcpy(out + 12u * i, &o, sizeof o);
        ok[i] = res[i].ok;
    }
    return LPT_OK;
}

// SPEC §18: env_sample (and env_lookup along the sample), once per draw u = (r6, r7, r8, r9, r1, r2); all zero for a probe without a distribution
int lpt_probe_sample(lpt_device *dev, lpt_probe *probe, const float *u, uint32_t n, float *dirs, float *pdf_s, float *radiance) {
    if (!dev || !probe || (n && (!u || !dirs || !pdf_s || !radiance))) return fail(LPT_ERR_INVALID_ARG, "lpt_probe_sample: null");
    if (probe->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_probe_sample: the probe belongs to another device");
    if (!n) return LPT_OK;   // (before probe_env: it reads the probe back)
    bool has = false;
    TRY(probe_env(probe, has));
    if (!has) {
        std::fill(dirs, dirs + 3 * (size_t)n, 0.0f); std::fill(pdf_s, pdf_s + n, 0.0f); std::fill(radiance, radiance + 3 * (size_t)n, 0.0f);
        return LPT_OK;
    }
    return run_probe(dev, n, kBlock, {{u, sizeof(float[6])}}, {{dirs, kF3}, {pdf_s, kF1}, {radiance, kF3}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_env_sample, grid, dim3(kBlock), 0, dev->stream, probe->d, probe->env, as<const float>(d[0]), n, as<float>(d[1]), as<float>(d[2]), as<float>(d[3]));
    });
}

// SPEC §18: env_pdf, once per direction; zero for a probe without a distribution
int lpt_probe_pdf(lpt_device *dev, lpt_probe *probe, const float *dirs, uint32_t n, float *pdf_e) {
    if (!dev || !probe || (n && (!dirs || !pdf_e))) return fail(LPT_ERR_INVALID_ARG, "lpt_probe_pdf: null");
    if (probe->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_probe_pdf: the probe belongs to another device");
    if (!n) return LPT_OK;   // (before probe_env, as above)
    bool has = false;
    TRY(probe_env(probe, has));
    if (!has) { std::fill(pdf_e, pdf_e + n, 0.0f); return LPT_OK; }
    return run_probe(dev, n, kBlock, {{dirs, kF3}}, {{pdf_e, kF1}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_env_pdf, grid, dim3(kBlock), 0, dev->stream, probe->env, as<const float>(d[0]), n, as<float>(d[1]));
    });
}

// SPEC §9: env_lookup, once per direction (needs no distribution: any probe answers)
int lpt_probe_lookup(lpt_device *dev, lpt_probe *probe, const float *dirs, uint32_t n, float *radiance) {
    if (!dev || !probe || (n && (!dirs || !radiance))) return fail(LPT_ERR_INVALID_ARG, "lpt_probe_lookup: null");
    if (probe->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_probe_lookup: the probe belongs to another device");
    return run_probe(dev, n, kBlock, {{dirs, kF3}}, {{radiance, kF3}}, [&](dim3 grid, const DevMem *d) {
        hipLaunchKernelGGL(k_env_lookup, grid, dim3(kBlock), 0, dev->stream, probe->d, as<const float>(d[0]), n, as<float>(d[1]));
    });
}

// the ray queries: traverse (and intersect_lights behind a closest hit), one ray per lane of a traversal block; MASK where the scene has alpha masks (SPEC §20)
int lpt_trace_closest(lpt_device *dev, const lpt_scene_gpu *sg, const float *origins, const float *dirs, uint32_t n, lpt_hit *out) {
    if (!dev || !sg || (n && (!origins || !dirs || !out))) return fail(LPT_ERR_INVALID_ARG, "lpt_trace_closest: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_trace_closest: the scene belongs to another device");
    std::vector<float4> o, d;
    pack_rays(origins, dirs, nullptr, n, o, d);
    return run_probe(dev, n, kTraceBlock, {{o.data(), sizeof(float4)}, {d.data(), sizeof(float4)}}, {{out, sizeof(lpt_hit)}}, [&](dim3 grid, const DevMem *m) {
        const auto k = sg->d.n_alpha ? k_query_closest<true> : k_query_closest<false>;
        hipLaunchKernelGGL(k, grid, dim3(kTraceBlock), stack_bytes(sg->d), dev->stream, sg->d, as<const float4>(m[0]), as<const float4>(m[1]), as<float4>(m[2]), n);
    });
}

int lpt_trace_occluded(lpt_device *dev, const lpt_scene_gpu *sg, const float *origins, const float *dirs, const float *tmax, uint32_t n, uint8_t *out) {
    if (!dev || !sg || (n && (!origins || !dirs || !tmax || !out))) return fail(LPT_ERR_INVALID_ARG, "lpt_trace_occluded: null");
    if (sg->dev != dev) return fail(LPT_ERR_INVALID_ARG, "lpt_trace_occluded: the scene belongs to another device");
    std::vector<float4> o, d;
    pack_rays(origins, dirs, tmax, n, o, d);
    return run_probe(dev, n, kTraceBlock, {{o.data(), sizeof(float4)}, {d.data(), sizeof(float4)}}, {{out, sizeof(uint8_t)}}, [&](dim3 grid, const DevMem *m) {
        const auto k = sg->d.n_alpha ? k_query_occluded<true> : k_query_occluded<false>;
        hipLaunchKernelGGL(k, grid, dim3(kTraceBlock), stack_bytes(sg->d), dev->stream, sg->d, as<const float4>(m[0]), as<const float4>(m[1]), as<uint8_t>(m[2]), n);
    });
}

// ============================================================================ Renderer
static int ensure_denoiser(lpt_renderer *r) {
    if (r->has_denoiser()) return LPT_OK;
    const size_t n = (size_t)r->w * r->h;
    hipStream_t s = r->stream;
    Denoiser d;   // joins the renderer once it is whole: a failure half way leaves the renderer without one, and a later call starts over
    for (int k = 0; k < 2; ++k) {
        TRY(d.den_gbuf[k].alloc(n));
        TRY(d.den_rad[k].alloc(n));
        TRY(d.den_mom[k].alloc(n));
        TRY(d.den_hist[k].alloc(n));
        HIP_TRY(hipMemsetAsync(d.den_gbuf[k], 0, sizeof(uint4) * n, s));
        HIP_TRY(hipMemsetAsync(d.den_rad[k], 0, sizeof(float4) * n, s));
        HIP_TRY(hipMemsetAsync(d.den_mom[k], 0, sizeof(float2) * n, s));
        HIP_TRY(hipMemsetAsync(d.den_hist[k], 0, sizeof(uint32_t) * n, s));  // history 0 = nothing to reproject
    }
    TRY(d.den_motion.alloc(n));
    TRY(d.den_noisy.alloc(n));
    TRY(d.den_nd.alloc(n));
    TRY(d.den_temp.alloc(n));
    HIP_TRY(hipMemsetAsync(d.den_noisy, 0, sizeof(float4) * n, s));
    HIP_TRY(hipMemsetAsync(d.den_motion, 0, sizeof(float2) * n, s));
    HIP_TRY(hipStreamSynchronize(s));   // the primary pass of the first frame may run on a lane's stream
    static_cast<Denoiser &>(*r) = std::move(d);
    return LPT_OK;
}

// ---- tile ownership (kernels.h ShardMap / ShardTable).  The V = sum(weights) virtual ranks are dealt to the ranks so that every
// rank's share of any run of tiles follows its weight: virtual rank v goes to the rank that is furthest behind its share
// (ties: the lowest rank).  Unit weights give virtual rank = rank.  Pure host arithmetic, the same on every rank.
static std::vector<uint32_t> deal_virtual_ranks(const std::vector<uint32_t> &weights, uint32_t world) {
    std::vector<uint32_t> owner;
    if (weights.empty()) { owner.resize(world); for (uint32_t q = 0; q < world; ++q) owner[q] = q; return owner; }
    uint32_t V = 0;
    for (uint32_t wq : weights) V += wq;
    std::vector<uint32_t> given(world, 0u);
    for (uint32_t v = 0; v < V; ++v) {
        uint32_t best = 0;
        long long best_deficit = -(1ll << 60);
        for (uint32_t q = 0; q < world; ++q) {
            const long long deficit = (long long)weights[q] * (v + 1u) - (long long)given[q] * V;   // share due - share given, times V
            if (given[q] < weights[q] && deficit > best_deficit) { best = q; best_deficit = deficit; }
        }
        owner.push_back(best);
        given[best]++;
    }
    return owner;
}
static inline uint32_t tiles_of_virtual(uint32_t n_tiles, uint32_t V, uint32_t v) { return n_tiles / V + (v < n_tiles % V ? 1u : 0u); }
static ShardMap make_shard_map(const std::vector<uint32_t> &weights, uint32_t rank, uint32_t world) {
    ShardMap m{};
    const std::vector<uint32_t> owner = deal_virtual_ranks(weights, world);
    m.V = (uint32_t)owner.size();
    for (uint32_t v = 0; v < m.V; ++v)
        if (owner[v] == rank && m.w < kMaxWeight) m.vlist[m.w++] = v;
    return m;
}
static uint32_t owned_tiles(const ShardMap &m, uint32_t n_tiles) {
    uint32_t n = 0;
    for (uint32_t j = 0; j < m.w; ++j) n += tiles_of_virtual(n_tiles, m.V, m.vlist[j]);
    return n;
}
// `offsets` (world + 1 entries, any world size): where every rank's slots start in rank 0's staging area — the host's copy of the rule.
// The device table holds arrays only for a WEIGHTED rule (world <= kMaxWorld, sum of weights <= kMaxVirtual: checked by the callers);
// unit weights are the closed form on both sides (the fixed-size arrays were written for any world).
static ShardTable make_shard_table(const std::vector<uint32_t> &weights, uint32_t world, uint32_t n_tiles, uint32_t area, std::vector<uint32_t> &offsets) {
    ShardTable t{};
    offsets.assign((size_t)world + 1u, 0u);
    if (weights.empty()) {
        t.V = world;
        t.unit_world = world;
        for (uint32_t q = 0; q <= world; ++q) offsets[q] = shard_slot_offset(n_tiles, world, area, q);
        return t;
    }
    const std::vector<uint32_t> owner = deal_virtual_ranks(weights, world);
    t.V = (uint32_t)owner.size();
    std::vector<uint32_t> tiles(world, 0u);
    for (uint32_t v = 0; v < t.V && v < kMaxVirtual; ++v) {
        if (owner[v] >= kMaxWorld) continue;   // unreachable behind the callers' checks; never write past the arrays
        t.owner[v] = (uint8_t)owner[v];
        t.j[v] = (uint8_t)t.w[owner[v]]++;
        tiles[owner[v]] += tiles_of_virtual(n_tiles, t.V, v);
    }
    for (uint32_t q = 0; q < world; ++q) {
        offsets[q + 1] = offsets[q] + tiles[q] * area;
        if (q < kMaxWorld) t.offset[q + 1] = offsets[q + 1];
    }
    return t;
}

static void shard_geometry(const lpt_renderer *r, uint32_t &tiles_x, uint32_t &n_tiles, uint32_t &n_slots) {
    tiles_x = div_up(r->w, r->tile_w);
    const uint32_t tiles_y = div_up(r->h, r->tile_h);
    n_tiles = tiles_x * tiles_y;
    n_slots = owned_tiles(r->map, n_tiles) * r->tile_w * r->tile_h;
}

// per-ray buffers of one lane (queues, hits, shadow queue, per-sample radiance): one element per ray of a wavefront.  The lane lets go of what it has first;
// the new buffers join it, with the queue views the kernels get, once they are whole
static int alloc_ray_buffers(Wavefront &wf, size_t rays) {
    release<RayBuffers>(wf);
    const size_t n = std::max<size_t>(rays, 64);
    if (n > 0x7FFFFFFFull) return fail(LPT_ERR_INVALID_ARG, "a wavefront of %zu rays exceeds 2^31", n);
    RayBuffers b;
    for (int k = 0; k < 2; ++k) {
        TRY(b.q_mem[k].o.alloc(n));
        TRY(b.q_mem[k].d.alloc(n));
        TRY(b.q_mem[k].t.alloc(n));
        b.q[k] = Queue{b.q_mem[k].o, b.q_mem[k].d, b.q_mem[k].t};
    }
    TRY(b.sq_mem.o.alloc(n));
    TRY(b.sq_mem.d.alloc(n));
    TRY(b.sq_mem.t.alloc(n));
    b.sq = ShadowQueue{b.sq_mem.o, b.sq_mem.d, b.sq_mem.t};
    TRY(b.hits.alloc(n));
    TRY(b.Lsum.alloc(n));
    TRY(b.strag.alloc(2 * n));   // a launch carries at most n closest-hit + n shadow rays
    b.ray_cap = n;
    static_cast<RayBuffers &>(wf) = std::move(b);
    return LPT_OK;
}

// stream, events and counters of a lane (created on first use), and the `n_trav` traversal events a phased plan has its stages record.
// Lane 0 enqueues on the renderer's stream: the runtime maps
// streams onto a fixed number of hardware queues (4 by default: the null stream, the device's, the renderer's and one more), and
// streams that share a queue run back to back — with a stream of its own for every lane, the two lanes of the default renderer
// shared one queue and never overlapped (profiles/r08_lane_phase_ab.txt)
static int ensure_lane(lpt_renderer *r, int l, uint32_t n_trav = 0) {
    Wavefront &wf = r->wf[l];
    if (l > 0 && !wf.stream) TRY(wf.stream.create());
    if (!wf.done) TRY(wf.done.create());
    if (!wf.consumed) TRY(wf.consumed.create());
    if (!wf.ctr) TRY(wf.ctr.alloc(1));
    for (uint32_t t = 0; t < n_trav; ++t)
        if (!wf.trav[t]) TRY(wf.trav[t].create());
    return LPT_OK;
}

// lane `l` holds `n` rays: a lane that has to grow waits first for what still reads its buffers — everything that read them has been enqueued behind the
// waits of the renderer's stream, and the lane's own launches are on its own
static int lane_hold(lpt_renderer *r, int l, size_t n) {
    TRY(ensure_lane(r, l));
    Wavefront &wf = r->wf[l];
    if (n <= wf.ray_cap) return LPT_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (wf.stream) HIP_TRY(hipStreamSynchronize(wf.stream));
    return alloc_ray_buffers(wf, n);
}

// The frame buffers for the renderer's size and shard; what depended on the old ones (the denoiser: Renderer::resize re-creates the ASVGF resources,
// renderer.rs:347-355; every lane's ray buffers) goes with them.  A failure leaves the renderer without frame buffers: raytrace() is then the no-op of a 0 x 0
// renderer (record_call) and the reads report that there is no target.
static int alloc_frame_buffers(lpt_renderer *r) {
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipStreamSynchronize(r->stream));
    release<Denoiser>(*r);
    for (int l = 0; l < kMaxLanes; ++l) release<RayBuffers>(r->wf[l]);
    release<FrameBuffers>(*r);
    if (!r->w || !r->h) return LPT_OK;
    uint32_t tiles_x, n_tiles, n_slots;
    shard_geometry(r, tiles_x, n_tiles, n_slots);
    const size_t px = (size_t)r->w * r->h;
    if (r->rank == 0u) {   // a possible root of an exchange (also of a one-rank communicator): the whole ownership rule, for the unpack kernels
        r->h_table = make_shard_table(r->weights, r->world, n_tiles, r->tile_w * r->tile_h, r->h_offset);
        if (!r->d_table) TRY(r->d_table.alloc(1));
        HIP_TRY(hipMemcpy(r->d_table, &r->h_table, sizeof(ShardTable), hipMemcpyHostToDevice));
    }
    FrameBuffers fb;
    fb.n_slots = n_slots;   // the lanes' ray buffers are allocated by the first raytrace() that uses them
    TRY(fb.accum.alloc(px));
    TRY(fb.scratch.alloc(px));
    HIP_TRY(hipMemsetAsync(fb.accum, 0, sizeof(float4) * px, r->stream));
    static_cast<FrameBuffers &>(*r) = std::move(fb);
    return LPT_OK;
}

int lpt_renderer_create(lpt_device *dev, uint32_t width, uint32_t height, lpt_renderer **out) {
    if (!dev || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_create: null");
    HIP_TRY(hipSetDevice(dev->ordinal));
    std::unique_ptr<lpt_renderer> r(new lpt_renderer());   // a failure below drops it, and what it owns by then
    r->dev = dev;
    TRY(r->stream.create());
    r->prev_cam.origin = mk3(0.f, 0.f, 0.f); r->prev_cam.right = mk3(1.f, 0.f, 0.f); r->prev_cam.up = mk3(0.f, 1.f, 0.f);
    r->prev_cam.fwd = mk3(0.f, 0.f, 1.f); r->prev_cam.ax = r->prev_cam.ay = 1.0f;   // Mat4::IDENTITY (renderer.rs:319)
    r->req_w = width; r->req_h = height;
    // get_downsampled_size (renderer.rs:18-22)
    r->w = (uint32_t)((float)width * r->downsample);
    r->h = (uint32_t)((float)height * r->downsample);
    TRY(r->totals.alloc(1));
    HIP_TRY(hipMemset(r->totals, 0, sizeof(Totals)));
    {
        void *word = nullptr;
        HIP_TRY(hipHostMalloc(&word, sizeof(uint32_t), hipHostMallocMapped));
        r->err_host.reset((uint32_t *)word);
        *r->err_host = 0u;
    }
    TRY(r->default_probe.alloc(4));
    HIP_TRY(hipMemset(r->default_probe, 0, 4));  // 1x1 zero texel: black environment (device.rs:13-26)
    TRY(r->srgb_thr.alloc(256));
    float thr[256];
    srgb_thresholds(thr);
    HIP_TRY(hipMemcpy(r->srgb_thr, thr, sizeof thr, hipMemcpyHostToDevice));
    TRY(alloc_frame_buffers(r.get()));
    dev->renderers.push_back(r.get());
    *out = r.release();
    return LPT_OK;
}

int lpt_renderer_destroy(lpt_renderer *r) {
    if (!r) return LPT_OK;
    hipSetDevice(r->dev->ordinal);
    r->pend.n = 0;   // recorded but never submitted: nobody can read the result any more
    forget_deferred_exchange(r);   // an exchange enqueued inside a still open lpt_comm_group bracket must not outlive the renderer
    {
        auto &v = r->dev->renderers;
        v.erase(std::remove(v.begin(), v.end(), r), v.end());
    }
    hipStreamSynchronize(r->stream);
    for (int l = 0; l < kMaxLanes; ++l)   // a wavefront whose second half was never enqueued (a failed submission) is not behind r->stream
        if (r->wf[l].stream) hipStreamSynchronize(r->wf[l].stream);
    delete r;   // what it owns with it: the buffers before the streams and events they were used on
    return LPT_OK;
}

int lpt_renderer_set_downsample(lpt_renderer *r, float factor) {
    if (!r || !(factor > 0.f) || factor > 16.f) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_downsample: factor must be in (0,16]");
    FLUSH_OR_RETURN(r);
    r->downsample = factor;
    return LPT_OK;
}

int lpt_renderer_set_resources(lpt_renderer *r, const lpt_scene_gpu *sg, const lpt_probe *probe) {
    if (!r || !sg) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_resources: null");
    if (sg->dev != r->dev || (probe && probe->dev != r->dev)) return fail(LPT_ERR_INVALID_ARG, "resources belong to another device");
    FLUSH_OR_RETURN(r);
    r->sg = sg;
    r->probe = probe;
    r->resources_set = true;
    r->frame_count = 1;  // renderer.rs:724
    return LPT_OK;
}

int lpt_renderer_resize(lpt_renderer *r, const lpt_scene_gpu *sg, const lpt_probe *probe, uint32_t width, uint32_t height) {
    if (!r || !sg) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_resize: null");
    FLUSH_OR_RETURN(r);
    const uint32_t nw = (uint32_t)((float)width * r->downsample), nh = (uint32_t)((float)height * r->downsample);
    if (nw > 8192u || nh > 8192u) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_resize: the path-traced size is limited to 8192 x 8192 (got %u x %u)", nw, nh);
    r->req_w = width; r->req_h = height;
    r->w = nw;
    r->h = nh;
    int st = alloc_frame_buffers(r);
    if (st != LPT_OK) return st;
    return lpt_renderer_set_resources(r, sg, probe);
}

int lpt_renderer_get_size(const lpt_renderer *r, uint32_t *w, uint32_t *h) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_size: null");
    if (w) *w = r->w;
    if (h) *h = r->h;
    return LPT_OK;
}

// largest per-pixel record: a queued ray (origin+slot, dir+pdf, throughput) = 48 B
uint32_t lpt_max_per_pixel_bytes(void) { return 48u; }

int lpt_renderer_set_max_bounces(lpt_renderer *r, uint32_t b) {
    if (!r || b == 0 || b > (uint32_t)kMaxBounces) return fail(LPT_ERR_INVALID_ARG, "max_bounces must be in [1,%d]", kMaxBounces);
    FLUSH_OR_RETURN(r);
    r->max_bounces = b;
    return LPT_OK;
}
int lpt_renderer_set_env_sampling(lpt_renderer *r, int flag) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_env_sampling: null");
    FLUSH_OR_RETURN(r);
    r->env_sampling = flag ? 1 : 0;
    return LPT_OK;
}
int lpt_renderer_get_env_sampling(const lpt_renderer *r, int *flag) {
    if (!r || !flag) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_env_sampling: null");
    *flag = r->env_sampling;
    return LPT_OK;
}
int lpt_renderer_set_emissive_sampling(lpt_renderer *r, int flag) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_emissive_sampling: null");
    FLUSH_OR_RETURN(r);
    r->emissive_sampling = flag ? 1 : 0;
    return LPT_OK;
}
int lpt_renderer_get_emissive_sampling(const lpt_renderer *r, int *flag) {
    if (!r || !flag) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_emissive_sampling: null");
    *flag = r->emissive_sampling;
    return LPT_OK;
}
int lpt_renderer_set_glass_shadows(lpt_renderer *r, int flag) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_glass_shadows: null");
    FLUSH_OR_RETURN(r);
    r->glass_shadows = flag ? 1 : 0;
    return LPT_OK;
}
int lpt_renderer_get_glass_shadows(const lpt_renderer *r, int *flag) {
    if (!r || !flag) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_glass_shadows: null");
    *flag = r->glass_shadows;
    return LPT_OK;
}
int lpt_renderer_set_lens(lpt_renderer *r, float radius, float focus_distance) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_lens: null");
    if (!std::isfinite(radius) || radius < 0.0f) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_lens: the radius must be finite and >= 0");
    if (!std::isfinite(focus_distance) || !(focus_distance > 0.0f)) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_lens: the focus distance must be finite and > 0");
    FLUSH_OR_RETURN(r);
    r->lens_r = radius; r->lens_f = focus_distance;
    return LPT_OK;
}
int lpt_renderer_get_lens(const lpt_renderer *r, float *radius, float *focus_distance) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_lens: null");
    if (radius) *radius = r->lens_r;
    if (focus_distance) *focus_distance = r->lens_f;
    return LPT_OK;
}
int lpt_renderer_set_seed(lpt_renderer *r, uint32_t s) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_seed: null");
    FLUSH_OR_RETURN(r);
    r->user_seed = s;
    return LPT_OK;
}
int lpt_renderer_set_vfov(lpt_renderer *r, float radians) {
    if (!r || !(radians > 0.f) || !(radians < 3.14159f)) return fail(LPT_ERR_INVALID_ARG, "vfov must be in (0, pi)");
    FLUSH_OR_RETURN(r);
    r->vfov = radians;
    return LPT_OK;
}
int lpt_renderer_set_shard_weighted(lpt_renderer *r, uint32_t rank, uint32_t world, uint32_t tile_w, uint32_t tile_h, const uint32_t *weights) {
    if (!r || world == 0 || rank >= world || tile_w == 0 || tile_h == 0 || (tile_w * tile_h) % 64u != 0u)
        return fail(LPT_ERR_INVALID_ARG, "bad shard (rank %u of %u, tile %ux%u; tile area must be a multiple of 64)", rank, world, tile_w, tile_h);
    std::vector<uint32_t> wv;
    if (weights) {
        if (world > kMaxWorld) return fail(LPT_ERR_INVALID_ARG, "weighted shards: at most %u ranks", kMaxWorld);
        uint32_t sum = 0;
        bool unit = true;
        for (uint32_t q = 0; q < world; ++q) {
            if (weights[q] > kMaxWeight) return fail(LPT_ERR_INVALID_ARG, "weighted shards: weight %u of rank %u exceeds %u", weights[q], q, kMaxWeight);
            sum += weights[q];
            unit = unit && weights[q] == 1u;
        }
        if (sum == 0u || sum > kMaxVirtual) return fail(LPT_ERR_INVALID_ARG, "weighted shards: the weights must sum to 1..%u (got %u)", kMaxVirtual, sum);
        if (!unit) wv.assign(weights, weights + world);
    }
    FLUSH_OR_RETURN(r);
    r->rank = rank; r->world = world; r->tile_w = tile_w; r->tile_h = tile_h;
    r->weights = wv;
    r->map = make_shard_map(r->weights, rank, world);
    r->frame_count = 1;
    return alloc_frame_buffers(r);
}
int lpt_renderer_set_shard(lpt_renderer *r, uint32_t rank, uint32_t world, uint32_t tile_w, uint32_t tile_h) {
    return lpt_renderer_set_shard_weighted(r, rank, world, tile_w, tile_h, nullptr);
}
int lpt_renderer_reset_accumulation(lpt_renderer *r) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_reset_accumulation: null");
    r->frame_count = 1;       // renderer.rs:610
    r->accumulate = false;    // :611 ; the seed is deliberately not reset (:613-615)
    return LPT_OK;
}
int lpt_renderer_set_accumulate(lpt_renderer *r, int a) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_accumulate: null");
    r->accumulate = a != 0;
    return LPT_OK;
}
int lpt_renderer_get_accumulate(const lpt_renderer *r, int *a) {
    if (!r || !a) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_accumulate: null");
    *a = r->accumulate ? 1 : 0;
    return LPT_OK;
}
int lpt_renderer_get_frame_state(const lpt_renderer *r, uint32_t *fc, uint32_t *seed) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_frame_state: null");
    if (fc) *fc = r->frame_count;
    if (seed) *seed = r->seed;
    return LPT_OK;
}
int lpt_renderer_upload_noise(lpt_renderer *r, const uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t row_bytes) {
    if (!r || !rgba8 || !w || !h || row_bytes < w * 4u) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_upload_noise: bad arguments");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->noise.reset();
    TRY(r->noise.alloc((size_t)w * h * 4));
    HIP_TRY(hipMemcpy2D(r->noise, (size_t)w * 4, rgba8, row_bytes, (size_t)w * 4, h, hipMemcpyHostToDevice));
    r->noise_w = w; r->noise_h = h;
    return LPT_OK;
}
int lpt_renderer_use_noise(lpt_renderer *r, int flag) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_use_noise: null");
    FLUSH_OR_RETURN(r);
    r->use_noise = flag != 0;
    return LPT_OK;
}
int lpt_renderer_set_blit_mode(lpt_renderer *r, int mode) {
    if (!r || mode < LPT_BLIT_PATHTRACE || mode > LPT_BLIT_MOTION) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_blit_mode: bad mode %d", mode);
    FLUSH_OR_RETURN(r);
    r->mode = mode;
    return LPT_OK;
}
int lpt_renderer_set_lanes(lpt_renderer *r, int lanes) {
    if (!r || lanes < 1 || lanes > kMaxLanes) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_lanes: 1..%d", kMaxLanes);
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipStreamSynchronize(r->stream));   // behind its waits: every lane's work
    for (int l = 0; l < kMaxLanes; ++l) {
        if (r->wf[l].stream) HIP_TRY(hipStreamSynchronize(r->wf[l].stream));
        r->wf[l].consumed_recorded = false;
        if (l >= lanes) release<RayBuffers>(r->wf[l]);
    }
    r->n_lanes = lanes;
    r->lane_rr = 0;
    return LPT_OK;
}
int lpt_renderer_set_sort_queues(lpt_renderer *r, int flag) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_sort_queues: null");
    FLUSH_OR_RETURN(r);
    // 1: next-bounce queue, 2: shadow queue; any other non-zero value: both queues
    r->sort_queues = flag ? ((flag & 3) ? (flag & 3) : 3) : 0;
    return LPT_OK;
}
// Launch tuning that experiments and the variant tests switch (the reference has no counterpart: SURVEY §5 "Config / flags: no").
// Every value gives the same frame bit for bit; only which kernels run, and how large their grids are, changes.
// One row per option: how it is read and stored, its range, and what a value outside does — clamped to the range, or (a row with a message) rejected.
struct OptionRow { int id; uint64_t (*get)(const lpt_renderer *); void (*set)(lpt_renderer *, uint64_t); uint64_t min, max; const char *reject; };
#define OPT_FIELD(F) [](const lpt_renderer *r) -> uint64_t { return (uint64_t)r->F; }, [](lpt_renderer *r, uint64_t v) { r->F = (decltype(r->F))v; }
static const OptionRow kOptions[] = {
    {LPT_OPT_PACKET_PRIMARY, OPT_FIELD(tune.packet_primary), 0u, 2u, "LPT_OPT_PACKET_PRIMARY: 0 (never), 1 (always), 2 (by pixel footprint)"},
    {LPT_OPT_EXPERIMENT(LPT_EXP_PIPE_RAYS), OPT_FIELD(tune.pipe_rays), 0u, 0x7FFFFFFFu, nullptr},
    {LPT_OPT_WAVEFRONT_RAYS, OPT_FIELD(wavefront_rays), 64u, UINT64_MAX, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_REFILL), OPT_FIELD(tune.refill), 0u, 63u, "LPT_EXP_REFILL: 0..63"},
    {LPT_OPT_EXPERIMENT(LPT_EXP_TRACE_WAVES_PER_CU), OPT_FIELD(tune.trace_waves_per_cu), 0u, 32u, "LPT_EXP_TRACE_WAVES_PER_CU: 0 (auto) or 1..32"},
    {LPT_OPT_EXPERIMENT(LPT_EXP_SHADE_BLOCKS_PER_CU), OPT_FIELD(tune.shade_blocks_per_cu), 0u, 64u, "LPT_EXP_SHADE_BLOCKS_PER_CU: 0 (by the submission) or 1..64"},
    {LPT_OPT_PATH_RAYS, OPT_FIELD(tune.path_rays), 0u, 0x7FFFFFFFu, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_PATH_WAVES_PER_CU), OPT_FIELD(tune.path_waves_per_cu), 1u, 32u, "LPT_EXP_PATH_WAVES_PER_CU: 1..32"},
    {LPT_OPT_EXPERIMENT(LPT_EXP_PATH_REFILL), OPT_FIELD(tune.path_refill), 0u, 63u, "LPT_EXP_PATH_REFILL: 0..63"},
    {LPT_OPT_EXPERIMENT(LPT_EXP_OCC_CELL_MILLI), [](const lpt_renderer *r) { return (uint64_t)(r->occ_cell * 1000.0f + 0.5f); }, [](lpt_renderer *r, uint64_t v) { r->occ_cell = (float)v * 1.0e-3f; }, 0u, 1000000u, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_STEP_BUDGET), OPT_FIELD(tune.step_budget), 0u, 1u << 20, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_BUDGET_RAYS), OPT_FIELD(tune.budget_rays), 0u, 0x7FFFFFFFu, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_PACKET_QUADS), OPT_FIELD(tune.packet_quads), 0u, 1u, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_SPLIT_RAYS), OPT_FIELD(split_rays), 0u, UINT64_MAX, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_BUDGET_SPLIT), OPT_FIELD(tune.budget_split), 0u, 1u, nullptr},
    {LPT_OPT_EXPERIMENT(LPT_EXP_LANE_PHASE), OPT_FIELD(lane_phase), 0u, 2u, "LPT_EXP_LANE_PHASE: 0 (free), 1 (offset start), 2 (alternating traversal)"},
    {LPT_OPT_TAIL_LANES, OPT_FIELD(tune.tail_lanes), 0u, kTailMax, nullptr},
    {LPT_OPT_COOP_RAYS, OPT_FIELD(tune.coop_rays), 0u, 0x7FFFFFFFu, nullptr},
};
#undef OPT_FIELD
static const OptionRow *find_option(int option) {
    for (const OptionRow &o : kOptions) if (o.id == option) return &o;
    return nullptr;
}
int lpt_renderer_set_option(lpt_renderer *r, int option, uint64_t value) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_option: null");
    FLUSH_OR_RETURN(r);
    const OptionRow *o = find_option(option);
    if (!o) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_option: unknown option %d", option);
    if (o->reject && (value < o->min || value > o->max)) return fail(LPT_ERR_INVALID_ARG, "%s", o->reject);
    o->set(r, std::min(std::max(value, o->min), o->max));
    return LPT_OK;
}
int lpt_renderer_get_option(const lpt_renderer *r, int option, uint64_t *value) {
    if (!r || !value) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_option: null");
    const OptionRow *o = find_option(option);
    if (!o) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_option: unknown option %d", option);
    *value = o->get(r);
    return LPT_OK;
}
int lpt_renderer_enable_stats(lpt_renderer *r, int flag) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_enable_stats: null");
    FLUSH_OR_RETURN(r);
    r->stats = flag != 0;
    if (flag) {   // the occluder-cache probe's table (kernels.h OccProbe): empty at the start of every stats session
        HIP_TRY(hipSetDevice(r->dev->ordinal));
        if (!r->occ_table) TRY(r->occ_table.alloc(kOccEntries));
        HIP_TRY(hipMemsetAsync(r->occ_table, 0, sizeof(uint32_t) * kOccEntries, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));
    }
    return LPT_OK;
}
int lpt_renderer_enable_timings(lpt_renderer *r, int flag) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_enable_timings: null");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    const int total = lpt_renderer::kRing * lpt_renderer::kMaxEvents;
    if (flag) {
        r->ev_start.resize(total);   // empty owners until created: a failure half way is made up for by the next call
        r->ev_stop.resize(total);
        for (int i = 0; i < total; ++i) {
            if (!r->ev_start[i]) TRY(r->ev_start[i].create(hipEventDefault));
            if (!r->ev_stop[i]) TRY(r->ev_stop[i].create(hipEventDefault));
        }
    }
    if (flag) {  // (re)start accumulating
        HIP_TRY(hipStreamSynchronize(r->stream));
        for (int k = 0; k < lpt_renderer::kRing; ++k) r->ev_count[k] = 0;
        for (int i = 0; i < ST_COUNT; ++i) { r->stage_ms[i] = 0.0; r->stage_launches[i] = 0; }
    }
    r->timings = flag != 0;
    return LPT_OK;
}

// fold one ring slot's finished events into the per-stage totals (waits for them if needed)
static void harvest_slot(lpt_renderer *r, int slot) {
    const int n = r->ev_count[slot];
    for (int i = 0; i < n; ++i) {
        const int e = slot * lpt_renderer::kMaxEvents + i;
        float ms = 0.f;
        hipEventSynchronize(r->ev_stop[e]);
        if (hipEventElapsedTime(&ms, r->ev_start[e], r->ev_stop[e]) == hipSuccess) {
            r->stage_ms[r->ev_stage[slot][i]] += ms;
            r->stage_launches[r->ev_stage[slot][i]]++;
        }
    }
    r->ev_count[slot] = 0;
}
static inline int cur_slot(const lpt_renderer *r) { return (int)(r->ring_pos % lpt_renderer::kRing); }
// `slot`: the ring slot of the wavefront the launch belongs to (-1: the current one; a phased piece's launches are enqueued after the next piece's set-up)
static inline void stage_begin(lpt_renderer *r, int stage, hipStream_t stream, int slot = -1) {
    if (!r->timings) return;
    if (slot < 0) slot = cur_slot(r);
    if (r->ev_count[slot] >= lpt_renderer::kMaxEvents) return;
    r->ev_stage[slot][r->ev_count[slot]] = stage;
    hipEventRecord(r->ev_start[slot * lpt_renderer::kMaxEvents + r->ev_count[slot]], stream);
}
static inline void stage_end(lpt_renderer *r, hipStream_t stream, int slot = -1) {
    if (!r->timings) return;
    if (slot < 0) slot = cur_slot(r);
    if (r->ev_count[slot] >= lpt_renderer::kMaxEvents) return;
    hipEventRecord(r->ev_stop[slot * lpt_renderer::kMaxEvents + r->ev_count[slot]], stream);
    r->ev_count[slot]++;
}

}  // extern "C"

// asvgf.render (renderer.rs:513-518, asvgf.rs:250-291) / asvgf.temporal_pass (:519-522) over the whole frame, from the
// per-pixel inputs (noisy radiance, G-buffer, motion) of the current frame
static void launch_filter(lpt_renderer *r, hipStream_t s) {
    if (r->mode != LPT_BLIT_DENOISED && r->mode != LPT_BLIT_TEMPORAL) return;  // debug views read the inputs directly (:539)
    const int cur = r->den_cur, prv = 1 - r->den_cur;
    const uint32_t npx = r->w * r->h;
    const uint32_t px_blocks = div_up(npx, kBlock);
    const uint32_t stream_blocks = stream_grid(r, npx);
    hipLaunchKernelGGL(k_temporal, dim3(stream_blocks), dim3(kBlock), 0, s, (int)r->w, (int)r->h, r->den_noisy, r->den_gbuf[cur], r->den_gbuf[prv], r->den_motion,
                       r->den_rad[prv], r->den_mom[prv], r->den_hist[prv], r->den_rad[cur], r->den_mom[cur], r->den_hist[cur]);
    const float4 *result = r->den_rad[cur];
    if (r->mode == LPT_BLIT_DENOISED) {
        hipMemcpyAsync(r->den_temp, r->den_rad[cur], sizeof(float4) * npx, hipMemcpyDeviceToDevice, s);  // copy_texture_to_texture
        // even number of a-trous calls: main <-> radiance_temp, result ends in radiance_temp (asvgf.rs:286-287)
        hipLaunchKernelGGL(k_decode_gbuf, dim3(px_blocks), dim3(kBlock), 0, s, r->den_gbuf[cur], r->den_nd, npx);
        hipLaunchKernelGGL(k_atrous, dim3(px_blocks), dim3(kBlock), 0, s, r->den_nd, r->den_temp, r->accum, (int)r->w, (int)r->h, 1);
        hipLaunchKernelGGL(k_atrous, dim3(px_blocks), dim3(kBlock), 0, s, r->den_nd, r->accum, r->den_temp, (int)r->w, (int)r->h, 2);
        hipLaunchKernelGGL(k_atrous, dim3(px_blocks), dim3(kBlock), 0, s, r->den_nd, r->den_temp, r->accum, (int)r->w, (int)r->h, 4);
        hipLaunchKernelGGL(k_atrous, dim3(px_blocks), dim3(kBlock), 0, s, r->den_nd, r->accum, r->den_temp, (int)r->w, (int)r->h, 8);
        result = r->den_temp;
    }
    hipLaunchKernelGGL(k_composite, dim3(px_blocks), dim3(kBlock), 0, s, r->den_gbuf[cur], result, r->accum, npx);
}

// Runtime flags as template arguments: calls f(std::bool_constant<flag>{}...), so every combination of the flags is instantiated.  For kernels whose
// instantiations are a full cross product (k_raygen, k_trace_coop, k_trace_packet); the kernels that exist in some of their forms only have a launcher each, below.
template <class F> static void with_flags(F &&f) { f(); }
template <class F, class... Rest> static void with_flags(F &&f, bool flag, Rest... rest) {
    if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// k_trace<STATS, PIPE, TAIL, MASK>: the eight instantiations that exist, by name, and k_trace_glass<STATS> (SPEC §27) behind them (launch_plan.h picks one)
static void launch_k_trace(TraceVariant v, uint32_t blocks, size_t lds, hipStream_t s, const TraceKernargs &ka) {
    const dim3 grid(blocks), block(kTraceBlock);
    switch (v) {
    case TraceVariant::Lane:      hipLaunchKernelGGL((k_trace<false, false>), grid, block, lds, s, ka); break;
    case TraceVariant::Pipe:      hipLaunchKernelGGL((k_trace<false, true>), grid, block, lds, s, ka); break;
    case TraceVariant::Stats:     hipLaunchKernelGGL((k_trace<true, false>), grid, block, lds, s, ka); break;
    case TraceVariant::StatsPipe: hipLaunchKernelGGL((k_trace<true, true>), grid, block, lds, s, ka); break;
    case TraceVariant::Tail:      hipLaunchKernelGGL((k_trace<false, false, true>), grid, block, lds, s, ka); break;
    case TraceVariant::PipeTail:  hipLaunchKernelGGL((k_trace<false, true, true>), grid, block, lds, s, ka); break;
    case TraceVariant::Mask:      hipLaunchKernelGGL((k_trace<false, false, false, true>), grid, block, lds, s, ka); break;
    case TraceVariant::StatsMask: hipLaunchKernelGGL((k_trace<true, false, false, true>), grid, block, lds, s, ka); break;
    case TraceVariant::Glass:      hipLaunchKernelGGL((k_trace_glass<false>), grid, block, lds, s, ka); break;
    case TraceVariant::StatsGlass: hipLaunchKernelGGL((k_trace_glass<true>), grid, block, lds, s, ka); break;
    }
}

// A runtime form word as a template argument: calls f(std::integral_constant<uint32_t, W>{}) for the W of the sequence that equals `form`; false if there is none, or if f says so
template <uint32_t... W, class F> static bool with_form(std::integer_sequence<uint32_t, W...>, uint32_t form, F &&f) { return ((form == W && f(std::integral_constant<uint32_t, W>{})) || ...); }

// k_shade<FORM>: the 96 words of kernel_forms.h that exist (launch_plan.h picks one); false, and no launch, for any other word
static bool launch_k_shade(uint32_t form, uint32_t blocks, hipStream_t s, const ShadeKernargs &ka) {
    return with_form(std::make_integer_sequence<uint32_t, kShadeForms>{}, form, [&](auto w) {
        constexpr uint32_t W = decltype(w)::value;
        if constexpr (shade_form_valid(W)) hipLaunchKernelGGL((k_shade<W>), dim3(blocks), dim3(kBlock), 0, s, ka);
        return shade_form_valid(W);
    });
}

// k_path<FORM, STATS>: the 8 words x 2; an ENV form takes the probe's distribution behind its other arguments `a`, the others nothing (their argument segment ends before it)
template <class... A> static bool launch_k_path(uint32_t form, bool stats, uint32_t blocks, size_t lds, hipStream_t s, const DEnv &ev, const A &...a) {
    return with_form(std::make_integer_sequence<uint32_t, kPathForms>{}, form, [&](auto w) {
        constexpr uint32_t W = decltype(w)::value;
        if constexpr (path_form_valid(W)) with_flags([&](auto S) {
            if constexpr ((W & kShadeEnv) != 0u) hipLaunchKernelGGL((k_path<W, decltype(S)::value, DEnv>), dim3(blocks), dim3(kTraceBlock), lds, s, a..., ev);
            else hipLaunchKernelGGL((k_path<W, decltype(S)::value>), dim3(blocks), dim3(kTraceBlock), lds, s, a...);
        }, stats);
        return path_form_valid(W);
    });
}

extern "C" {

// How one stage of a wavefront's launches is ordered against the other lanes (submission_plan.h, LPT_EXP_LANE_PHASE): events it waits
// for before its first launch / before its traversal launch, and the event recorded behind its traversal launch
struct PhaseHooks { hipEvent_t wait_start = nullptr, wait_trav = nullptr, rec_trav = nullptr; };

// What the launches of one wavefront read (wavefront_prepare fills it, enqueue_stage and wavefront_finish read it): copies, so that the stages of the pieces
// of a cut batch can be enqueued in any order across the lanes; `r`'s buffers and the scene do not change before the submission is enqueued
struct WavefrontLaunch {
    lpt_renderer *r = nullptr;
    Wavefront *w = nullptr;          // the lane
    hipStream_t s = nullptr;         // the stream the lane's launches go to
    bool split = false;              // the renderer has more than one lane: the lane's `done` / `consumed` events order it against the renderer's stream
    FrameParams p{};
    GBufArgs gb{};                   // the denoising modes' targets and cameras
    // the rest only for a wavefront with slots (p.n_slots != 0):
    int slot = 0;                    // of the timing ring
    uint32_t nb = 0, seed0 = 0;
    WavefrontFacts f;
    LaunchTuning tune;
    LaunchPlan pl;
    DScene sc{};
    DProbe probe{};
    DEnv ev{};                       // read by the ENV kernels alone
    DNoise nz{};
    OccProbe occ{nullptr, 0u, 0.0f};
    size_t trace_lds = 0, coop_lds = 0;
    int sort_queues = 0;
};

// A wavefront between its two halves (flush_pending): what the second half needs to know about the first, and the first half's launches
struct Ticket {
    int lane = 0;
    bool denoise = false;
    WavefrontLaunch launch;
};

// What the launches of one wavefront read about the frame: the camera of `view`, the renderer's size, seeds, shard and lens, `n_samples` samples over the rank's
// slots [slot0, slot0 + piece_slots) (wavefront_prepare; lpt_renderer_primary_rays runs k_raygen alone from the same record)
static FrameParams frame_params(const lpt_renderer *r, const float view[16], uint32_t n_samples, uint32_t frame_count0, uint32_t seed0, bool acc0, uint32_t slot0, uint32_t piece_slots) {
    FrameParams p = shard_params(r);             // camera.dimensions / global_uniforms.dimensions (:431,436), the shard
    p.right = mk3(view[0], view[1], view[2]);    // camera.rs:101-108: cols = right, up, direction, origin
    p.up = mk3(view[4], view[5], view[6]);
    p.fwd = mk3(view[8], view[9], view[10]);
    p.origin = mk3(view[12], view[13], view[14]);
    const float th = tanf(0.5f * r->vfov);
    const float aspect = (float)r->w / (float)r->h;
    p.ax = aspect * th; p.ay = th;
    p.user_seed = r->user_seed;
    p.seed_counter = seed0;
    p.slot0 = slot0;
    p.n_slots = piece_slots;                     // the slots of THIS wavefront
    p.frame_count = frame_count0;
    p.max_bounces = r->max_bounces;
    p.n_samples = n_samples;
    p.fc_inc0 = acc0 ? 1u : 0u;
    // SPEC §25: rn = normalize(right), un = normalize(up), §3's normalize in binary32, once per frame
    const auto unit = [](f3 a) {
        const float l2 = (a.x * a.x + a.y * a.y) + a.z * a.z;
        if (!(l2 > 0.0f)) return mk3(0.0f, 0.0f, 0.0f);
        const float inv = 1.0f / sqrtf(l2);
        return mk3(a.x * inv, a.y * inv, a.z * inv);
    };
    p.lens_r = r->lens_r; p.lens_f = r->lens_f;
    p.lens_rn = unit(p.right); p.lens_un = unit(p.up);
    return p;
}

// First half of a wavefront: the launches of the `b.n` recorded raytrace() calls over the rank's pixel slots
// [piece.slot0, piece.slot0 + piece.n_slots) — ray generation, traversal, shading — on the wavefront's lane, from the protocol state the first
// of the calls saw (frame_count0, seed0, acc0 = its accumulate flag; the later ones ran with accumulate == true by construction).
// This is everything before the first launch: the lane `piece.lane` (submission_plan.h) and its buffers, the denoiser's flip and memsets, the wait for what consumed the
// lane's previous radiance, the launch plan.  The launches themselves are left in `tk` for enqueue_stage, stage by stage.
static int wavefront_prepare(lpt_renderer *r, const lpt_renderer::Pending &b, const SubmissionPiece &piece, uint32_t trav_events, Ticket &tk) {
    r->n_wavefronts++;
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    hipStream_t sm = r->stream;                  // accumulation, filter passes, bookkeeping, reads, the exchange: in call order
    const uint32_t nb = r->max_bounces;          // reference constant 3 (:398-399)
    const uint32_t n_samples = b.n, seed0 = b.seed0;

    const FrameParams p = frame_params(r, b.view, n_samples, b.frame_count0, seed0, b.acc0, piece.slot0, piece.n_slots);
    const float th = tanf(0.5f * r->vfov);
    const uint32_t n_rays = p.n_slots * n_samples;
    const bool denoise = r->mode != LPT_BLIT_PATHTRACE;
    const bool split = r->n_lanes > 1;           // the wavefront runs on the lane's own stream (a single wavefront on the renderer's own stream instead: 2.89 against 2.90 ms per 1/8-shard frame, round 5)
    const int lane = (int)piece.lane;
    TRY(ensure_lane(r, lane, trav_events));   // with the events the piece's stages record
    Wavefront &wf = r->wf[lane];
    hipStream_t s = (split && lane > 0) ? wf.stream : sm;
    r->last_lane = lane;
    if ((size_t)n_rays > wf.ray_cap && p.n_slots) {
        TRY(lane_hold(r, lane, n_rays));
        // the next wavefronts of this size take the other lanes: give them their buffers now, not in the middle of a later frame
        // (a first-use hipMalloc of gigabytes takes tens of milliseconds on some hosts)
        for (int l = 0; split && !denoise && l < r->n_lanes; ++l)
            if (l != lane) TRY(lane_hold(r, l, n_rays));
    }
    tk = Ticket{};
    tk.lane = lane; tk.denoise = denoise;
    WavefrontLaunch &L = tk.launch;
    L.r = r; L.w = &wf; L.s = s; L.split = split; L.p = p; L.nb = nb; L.seed0 = seed0;
    GBufArgs &gb = L.gb;
    if (denoise) TRY(ensure_denoiser(r));
    // the accumulation that consumed this lane's previous radiance.  A denoising frame also overwrites what the previous
    // frame's filter passes read (G-buffer ping-pong, motion) — and on a sharded frame those are enqueued by a later call
    // (lpt_renderer_exchange / denoise_filter) — so it waits for everything the renderer's stream holds so far.
    if (split && denoise) { HIP_TRY(hipEventRecord(wf.consumed, sm)); wf.consumed_recorded = true; }
    if (split && wf.consumed_recorded) HIP_TRY(hipStreamWaitEvent(s, wf.consumed, 0));
    if (denoise) {
        r->den_cur = 1 - r->den_cur;         // asvgf.start() (renderer.rs:467)
        if (r->world != 1u) {
            // sharded frame: this rank fills only its tiles; the rest must read as zero for the exchange
            const size_t npx = (size_t)r->w * r->h;
            HIP_TRY(hipMemsetAsync(r->den_gbuf[r->den_cur], 0, sizeof(uint4) * npx, s));
            HIP_TRY(hipMemsetAsync(r->den_motion, 0, sizeof(float2) * npx, s));
            HIP_TRY(hipMemsetAsync(r->den_noisy, 0, sizeof(float4) * npx, sm));
        }
        gb.gbuf = r->den_gbuf[r->den_cur];
        gb.motion = r->den_motion;
        gb.cur.origin = p.origin; gb.cur.right = p.right; gb.cur.up = p.up; gb.cur.fwd = p.fwd; gb.cur.ax = p.ax; gb.cur.ay = p.ay;
        gb.prev = r->prev_cam;
    }

    L.probe = r->probe ? r->probe->d : DProbe{as<const uint8_t>(r->default_probe), 1u, 1u};
    bool env = false;   // SPEC §18: the ENV kernels while the mode is on and the bound probe has a distribution
    if (r->env_sampling && r->probe) TRY(probe_env(const_cast<lpt_probe *>(r->probe), env));
    L.ev = env ? r->probe->env : DEnv{};
    L.nz = DNoise{as<const uint8_t>(r->noise), r->noise_w, r->noise_h, (r->use_noise && r->noise) ? 1u : 0u};
    const DScene &sc = r->sg->d;
    if (r->timings) { r->ring_pos++; harvest_slot(r, cur_slot(r)); }
    if (!p.n_slots) return LPT_OK;

    // what the launches depend on, and the decision (launch_plan.h: the rules are stated there)
    WavefrontFacts &f = L.f;
    f.n_rays = n_rays; f.n_slots = p.n_slots; f.slot0 = p.slot0; f.n_samples = n_samples; f.cus = (uint32_t)r->dev->compute_units;
    f.solo = piece.solo; f.stats = r->stats; f.denoise = denoise; f.env = env;
    f.masked = sc.n_alpha != 0u; f.trans = sc.n_trans != 0u; f.emis = sc.n_emis != 0u; f.esamp = r->emissive_sampling && f.emis && sc.n_emit != 0u; f.nmap = sc.n_nmap != 0u; f.lens = r->lens_r > 0.0f; f.punct = sc.n_punctual != 0u; f.glass_shadow = r->glass_shadows && f.punct && r->sg->n_thin_glass != 0u; f.max_depth = r->sg->stats.max_depth; f.stack_entries = sc.stack_entries;
    f.pixel_rad = 2.0f * th / (float)std::max(r->h, 1u); f.dense = (r->w % r->tile_w == 0u) && (r->h % r->tile_h == 0u); f.block8 = p.block8 != 0u;
    f.lim = KernelLimits{kBlock, kTraceBlock, kTailMax, kCoopWavesPerCu, kPacketBlocksPerCu, kPacketMaxPixelRad};
    L.tune = r->tune;
    L.sc = sc;
    const LaunchPlan &pl = L.pl = plan_wavefront(L.tune, f);
    if (pl.occ_probe && r->occ_table && r->occ_cell > 0.0f) L.occ = OccProbe{r->occ_table, kOccEntries - 1u, 1.0f / r->occ_cell};   // its table belongs to the renderer
    L.trace_lds = pl.stack_lds + (pl.tail ? sizeof(uint32_t) * tail_lds_words(f.max_depth) : 0u) + (pl.stats_lds_pad ? 64u : 0u);
    L.coop_lds = sizeof(uint32_t) * coop_stack_entries(kCoopStack, f.max_depth);
    L.sort_queues = r->sort_queues;
    L.slot = cur_slot(r);
    return LPT_OK;
}

// One traversal launch: closest-hit rays of bounce b+1 and shadow rays of bounce b, both produced by shade(b), are traced by
// ONE persistent launch (k_trace) — nb+1 traversal launches per frame instead of 2*nb.
static void launch_traversal(const WavefrontLaunch &L, int cb, int sb) {
    lpt_renderer *r = L.r;
    const Wavefront *w = L.w;
    hipStream_t s = L.s;
    const LaunchPlan &pl = L.pl;
    stage_begin(r, cb >= 0 ? ST_INTERSECT : ST_SHADOW, s, L.slot);  // :457-464, :493-498
    const Queue qin = w->q[(uint32_t)(cb < 0 ? 0 : cb) & 1u];
    const int launch_no = cb >= 0 ? cb : (int)L.nb;   // which strag_count[] this launch fills
    // every ray of both queues (coop-all), or the stragglers a budgeted launch left in w->strag: a whole wave each
    auto coop = [&](const uint32_t *strag) { with_flags([&](auto S) { hipLaunchKernelGGL(k_trace_coop<decltype(S)::value>, dim3(pl.coop_blocks), dim3(kTraceBlock), L.coop_lds, s, L.sc, qin, w->hits, w->sq, w->Lsum, w->ctr, cb, sb, strag, launch_no); }, L.f.stats); };
    if (pl.coop_all) coop(nullptr);
    else {
        launch_k_trace(pl.variant, pl.trace_blocks, L.trace_lds, s, TraceKernargs{L.sc, qin, w->hits, w->sq, w->Lsum, w->ctr, cb, sb, L.tune.refill, L.occ, pl.budget, w->strag, launch_no, pl.tail});
        if (pl.budget) coop(w->strag);
    }
    stage_end(r, s, L.slot);
}

// Stage t of a prepared wavefront's launches: stage 0 = counters, ray generation and the primary rays (with the path kernel: the whole wavefront),
// stage b + 1 = shade(b) and the traversal launch behind it.  `ph` orders the stage against the other lanes' (stream events only).
static int enqueue_stage(const WavefrontLaunch &L, uint32_t t, const PhaseHooks &ph) {
    lpt_renderer *r = L.r;
    const Wavefront *w = L.w;
    hipStream_t s = L.s;
    const int slot = L.slot;
    const uint32_t nb = L.nb;
    const LaunchPlan &pl = L.pl;
    const WavefrontFacts &f = L.f;
    const FrameParams &p = L.p;
    if (ph.wait_start) HIP_TRY(hipStreamWaitEvent(s, ph.wait_start, 0));
    if (t == 0u) {
        HIP_TRY(hipMemsetAsync(w->ctr, 0, sizeof(FrameCounters), s));
        // "ray generation" (:444-448)
        stage_begin(r, ST_RAYGEN, s, slot);
        with_flags([&](auto D, auto Ln) { hipLaunchKernelGGL((k_raygen<decltype(D)::value, decltype(Ln)::value>), dim3(pl.stream_blocks), dim3(kBlock), 0, s, p, L.nz, w->q[0], w->Lsum, w->ctr); }, f.dense, f.lens);   // LENS: SPEC §25
        stage_end(r, s, slot);
        if (ph.wait_trav) HIP_TRY(hipStreamWaitEvent(s, ph.wait_trav, 0));
        if (pl.packet) {
            // the primary rays: 64 consecutive queue entries are an 8x8-pixel patch of one sample — packet traversal (k_trace_packet)
            stage_begin(r, ST_PRIMARY, s, slot);
            with_flags([&](auto S) { hipLaunchKernelGGL(k_trace_packet<decltype(S)::value>, dim3(pl.packet_blocks), dim3(kTraceBlock), pl.packet_lds, s, L.sc, w->q[0], w->hits, w->ctr, 0, pl.quad_slots); }, f.stats);
            stage_end(r, s, slot);
        } else if (pl.coop_all || !pl.path) launch_traversal(L, 0, -1);   // a path-kernel wavefront traces its primary rays itself
        // every bounce behind the primary hits in ONE persistent launch — the passes of renderer.rs:484-509 without a chip-wide barrier between them (kernels.h k_path); same frame, same counters
        if (pl.path) {
            stage_begin(r, ST_PATH, s, slot);
            const size_t plds = pl.stack_lds + kPathLdsExtra;   // stacks + sRGB table + per-bounce counters
            const float4 *h0 = pl.packet ? w->hits : (const float4 *)nullptr;
            if (!launch_k_path(pl.path_form, f.stats, pl.path_blocks, plds, s, L.ev, L.sc, L.probe, L.nz, p, w->q[0], h0, w->Lsum, w->ctr, L.seed0, L.gb, L.tune.path_refill))
                return fail(LPT_ERR_INVALID_ARG, "the launch plan names k_path form 0x%x, which does not exist", pl.path_form);
            stage_end(r, s, slot);
        }
    } else if (!pl.path) {
        const uint32_t b = t - 1u;
        const uint32_t seed = L.seed0 + t;     // += 1 per bounce (:453, :487)
        const Queue qin = w->q[b & 1u], qout = w->q[(b + 1u) & 1u];
        stage_begin(r, ST_SHADE, s, slot);            // :471-480, :502-508
        const ShadeKernargs ska{L.sc, L.probe, L.nz, p, qin, w->hits, qout, w->sq, w->Lsum, w->ctr, (int)b, seed, L.gb, L.sort_queues, L.ev};   // ev: read by the ENV forms alone
        const uint32_t form = b == 0u ? pl.shade_form0 : pl.shade_form;   // bounce 0 of a denoising frame: the PrimaryRayPass form (bounce-0 shading + G-buffer + motion, renderer.rs:466-481)
        if (!launch_k_shade(form, pl.shade_blocks, s, ska)) return fail(LPT_ERR_INVALID_ARG, "the launch plan names k_shade form 0x%x, which does not exist", form);
        stage_end(r, s, slot);
        if (ph.wait_trav) HIP_TRY(hipStreamWaitEvent(s, ph.wait_trav, 0));
        launch_traversal(L, b + 1u < nb ? (int)(b + 1u) : -1, (int)b);
    }
    if (ph.rec_trav) HIP_TRY(hipEventRecord(ph.rec_trav, s));
    if (t == nb && L.split) HIP_TRY(hipEventRecord(w->done, s));
    HIP_TRY(hipGetLastError());
    return LPT_OK;
}

// Second half, on the renderer's stream behind every earlier call's: what reads the wavefront's radiance — accumulation (or the
// denoiser's inputs and filter) and the bookkeeping.  `read` (world == 1, Pathtrace): the pixel rows [row0, row1) this wavefront
// completes are resolved (or tonemapped) and copied to the host right behind its accumulation.
static int wavefront_finish(lpt_renderer *r, const Ticket &tk, const ReadPlan *read, uint32_t row0, uint32_t row1) {
    hipStream_t sm = r->stream;
    const FrameParams &p = tk.launch.p;
    Wavefront &wf = r->wf[tk.lane];
    const bool split = tk.launch.split;
    const uint32_t nb = p.max_bounces;
    if (p.n_slots) {
        const uint32_t stream_blocks = stream_grid(r, p.n_slots * p.n_samples);
        if (split) HIP_TRY(hipStreamWaitEvent(sm, wf.done, 0));
        if (r->mode == LPT_BLIT_PATHTRACE) {
            // AccumulationPass (:523-538)
            stage_begin(r, ST_ACCUM, sm);
            hipLaunchKernelGGL(k_accumulate, dim3(stream_blocks), dim3(kBlock), 0, sm, p, wf.Lsum, r->accum);
            stage_end(r, sm);
            if (read && row1 > row0) {
                // these pixel rows are final: their read-back overlaps the wavefronts that are still tracing the other rows
                const size_t off = (size_t)row0 * r->w, cnt = (size_t)(row1 - row0) * r->w;
                if (read->radiance) {
                    hipLaunchKernelGGL(k_resolve, dim3(div_up((uint32_t)cnt, kBlock)), dim3(kBlock), 0, sm, r->accum + off, r->scratch + off, (uint32_t)cnt);
                    HIP_TRY(hipMemcpyAsync(read->radiance + 4u * off, r->scratch + off, sizeof(float4) * cnt, hipMemcpyDeviceToHost, sm));
                } else {
                    uchar4 *px = reinterpret_cast<uchar4 *>(r->scratch.get()) + off;
                    launch_present(r, sm, r->accum + off, px, (uint32_t)cnt);
                    HIP_TRY(hipMemcpy2DAsync(read->rgba8 + (size_t)row0 * read->row_bytes, read->row_bytes, px, (size_t)r->w * 4, (size_t)r->w * 4, row1 - row0, hipMemcpyDeviceToHost, sm));
                }
            }
        } else {
            // per-pixel filter inputs; on a sharded frame (world > 1) the caller now exchanges noisy / gbuffer / motion
            // (lpt_renderer_denoiser_inputs) and rank 0 calls lpt_renderer_denoise_filter
            stage_begin(r, ST_ASVGF, sm);
            hipLaunchKernelGGL(k_den_scatter, dim3(stream_blocks), dim3(kBlock), 0, sm, p, wf.Lsum, r->den_noisy);
            r->den_inputs_ready = true;
            if (r->world == 1u) launch_filter(r, sm);
            stage_end(r, sm);
        }  // GBuffer / MotionVector: the primary pass has written the debug targets; nothing else runs (:539)
        hipLaunchKernelGGL(k_finish_frame, dim3(1), dim3(64), 0, sm, wf.ctr, r->totals, nb, tk.launch.pl.packet ? 1u : 0u);
        if (split) {
            HIP_TRY(hipEventRecord(wf.consumed, sm));
            wf.consumed_recorded = true;
        }
        HIP_TRY(hipGetLastError());
    } else if (r->mode != LPT_BLIT_PATHTRACE) {
        r->den_inputs_ready = true;   // a rank without tiles (a pure compositor / filter rank) still takes part in the frame's exchange
    }
    if (tk.denoise) r->prev_cam = tk.launch.gb.cur;       // prev_model_to_screen = P * V^-1 (:542-546)
    return LPT_OK;
}

// Submit what has been recorded (every synchronisation point and every setter that the launches read calls this first).
// Where the batch is cut into wavefronts, which lane and ticket each takes and the order of their halves and stages is plan_submission's decision
// (submission_plan.h: the rules are stated there); this walks its steps.  The piece that was launched first is complete about one stage before the last:
// `read` (lpt_renderer_read_radiance, lpt_renderer_blit_rgba8) has every piece's rows copied to the host as soon as they are final.
static int flush_pending(lpt_renderer *r, const ReadPlan *read) {
    if (!r->pend.n) return LPT_OK;
    const lpt_renderer::Pending b = r->pend;
    r->pend.n = 0;
    SubmissionFacts f;
    uint32_t n_tiles;
    shard_geometry(r, f.tiles_x, n_tiles, f.n_slots);
    f.tile_w = r->tile_w; f.tile_h = r->tile_h; f.world = r->world; f.height = r->h;
    f.n = b.n; f.max_fused = r->max_fused; f.pathtrace = r->mode == LPT_BLIT_PATHTRACE;
    f.wavefront_rays = r->wavefront_rays; f.split_rays = r->split_rays;
    f.n_lanes = (uint32_t)r->n_lanes; f.lane_phase = r->lane_phase; f.bounces = r->max_bounces;
    f.lane_rr = r->lane_rr; f.read = read != nullptr;
    const SubmissionPlan plan = plan_submission(f);
    r->lane_rr = plan.lane_rr;
    // A failure part way leaves wavefronts on the lanes' streams whose second halves (the waits that put them behind the renderer's
    // stream) were never enqueued: wait for them here, so that nothing is still running on buffers a later call frees or reuses
    auto bail = [&](int st) {
        for (int l = 0; l < kMaxLanes; ++l) {
            if (r->wf[l].stream) hipStreamSynchronize(r->wf[l].stream);
            r->wf[l].consumed_recorded = false;
        }
        hipStreamSynchronize(r->stream);
        return st;
    };
    Ticket tickets[kMaxLanes];
    const auto trav = [&](const TravEvent &e) -> hipEvent_t { return e.piece < 0 ? nullptr : r->wf[plan.pieces[(size_t)e.piece].lane].trav[e.stage]; };
    for (const SubmissionStep &step : plan.steps) {
        const SubmissionPiece &piece = plan.pieces[step.piece];
        Ticket &tk = tickets[piece.ticket];
        int st = LPT_OK;
        switch (step.kind) {
        case SubmissionStep::Prepare:
            st = wavefront_prepare(r, b, piece, plan.trav_events, tk);
            break;
        case SubmissionStep::Stage: {
            PhaseHooks ph;
            ph.wait_start = trav(step.wait_start);
            ph.wait_trav = trav(step.wait_trav);
            if (step.record) ph.rec_trav = r->wf[piece.lane].trav[step.t];
            st = enqueue_stage(tk.launch, step.t, ph);
            break;
        }
        case SubmissionStep::Finish:
            st = wavefront_finish(r, tk, read, piece.row0, piece.row1);   // the rows are empty but for the early read-back
            break;
        }
        if (st != LPT_OK) return bail(st);
    }
    return LPT_OK;
}

// recorded calls that may wait for one submission
static uint32_t fuse_cap(const lpt_renderer *r) { return r->max_fused ? r->max_fused : 64u; }

// Records ONE raytrace() call: the host-side protocol of Renderer::raytrace moves now (frame_back :401, seed :453/:487,
// frame_count :535-537), the launches wait for the next submission point.  A call fuses with the recorded ones when it
// continues the same accumulation from the same view — then the n calls are bit for bit the n samples of one wavefront
// (lpt_renderer_raytrace_n's contract; tests/test_gpu_deferred.py).
static int record_call(lpt_renderer *r, const float view[16]) {
    r->frame_back = !r->frame_back;              // renderer.rs:401
    if (!r->resources_set || !r->sg) return LPT_OK;  // :403-407, :419-422
    if (!r->accum) return LPT_OK;                // no frame buffers: a 0 x 0 renderer, or one whose allocation failed (alloc_frame_buffers)
    r->presented = false;                        // a new sample: the exchanged frame (if any) is stale
    lpt_renderer::Pending &b = r->pend;
    const bool pathtrace = r->mode == LPT_BLIT_PATHTRACE;
    if (b.n) {
        const uint32_t expect_fc = b.frame_count0 + (b.acc0 ? 1u : 0u) + (b.n - 1u);
        const bool fuses = pathtrace && r->accumulate && r->frame_count == expect_fc && b.n < fuse_cap(r) && memcmp(view, b.view, sizeof b.view) == 0;
        if (!fuses) FLUSH_OR_RETURN(r);
    }
    if (!b.n) {
        memcpy(b.view, view, sizeof b.view);
        b.frame_count0 = r->frame_count; b.seed0 = r->seed; b.acc0 = r->accumulate;
    }
    b.n++;
    r->n_recorded++;
    r->seed += r->max_bounces;                   // seed += 1 per intersect stage, never reset
    if (pathtrace && r->accumulate) r->frame_count += 1u;   // frame_count only moves in the Pathtrace arm (:523-538)
    // the denoising modes carry frame-to-frame state (one temporal pass per call): they launch at once; so does a full batch
    if (!pathtrace || b.n >= fuse_cap(r)) return flush_pending(r);
    return LPT_OK;
}

int lpt_renderer_raytrace(lpt_renderer *r, const float view[16]) {
    if (!r || !view) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_raytrace: null");
    return record_call(r, view);
}

int lpt_renderer_submit(lpt_renderer *r) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_submit: null");
    return flush_pending(r);
}

int lpt_renderer_get_submission_stats(const lpt_renderer *r, uint64_t *recorded_calls, uint64_t *wavefronts, uint32_t *pending_calls) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_submission_stats: null");
    if (recorded_calls) *recorded_calls = r->n_recorded;
    if (wavefronts) *wavefronts = r->n_wavefronts;
    if (pending_calls) *pending_calls = r->pend.n;
    return LPT_OK;
}

int lpt_renderer_set_max_fused(lpt_renderer *r, uint32_t n) {
    if (!r || n > 64u) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_max_fused: 0 (auto) or 1..64");
    FLUSH_OR_RETURN(r);
    r->max_fused = n;
    return LPT_OK;
}

int lpt_renderer_raytrace_n(lpt_renderer *r, const float view[16], uint32_t n_samples) {
    if (!r || !view) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_raytrace: null");
    if (n_samples == 0u || n_samples > 64u) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_raytrace_n: n must be in [1,64]");
    // n x { raytrace(view); accumulate = true (app.rs:318); }, submitted at once: the explicit batched form
    const uint32_t keep = r->max_fused;
    if (r->mode == LPT_BLIT_PATHTRACE) r->max_fused = std::min(64u, std::max(fuse_cap(r), n_samples + r->pend.n));   // the caller asked for this batch size
    int st = LPT_OK;
    for (uint32_t k = 0; k < n_samples && st == LPT_OK; ++k) {
        st = record_call(r, view);
        if (n_samples > 1u) r->accumulate = true;
    }
    if (st == LPT_OK) st = flush_pending(r);   // still with the explicit batch size: one wavefront, not the automatic spatial cut
    r->max_fused = keep;
    return st;
}

// SPEC §25, for tests and tools in the manner of lpt_scene_gpu_shading_normal: the renderer's own k_raygen, alone, over the rank's slots, for sample `sample` of the
// next raytrace() call; its queue comes back to the host and is laid out by pixel.  Buffers of its own: no lane, no frame state, no accumulation is touched.
int lpt_renderer_primary_rays(lpt_renderer *r, const float view[16], uint32_t sample, float *origins, float *dirs) {
    if (!r || !view || !origins || !dirs) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_primary_rays: null");
    if (sample >= 64u) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_primary_rays: sample must be below 64");
    if (!r->w || !r->h) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_primary_rays: the renderer has no size");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    uint32_t tiles_x, n_tiles, n_slots;
    shard_geometry(r, tiles_x, n_tiles, n_slots);
    const size_t npx = (size_t)r->w * r->h;
    std::fill(origins, origins + 3u * npx, 0.0f);
    std::fill(dirs, dirs + 3u * npx, 0.0f);
    if (!n_slots) return LPT_OK;
    // the sample-th of consecutive calls: its seeds are max_bounces per call further (record_call); frame_count does not reach k_raygen
    const FrameParams p = frame_params(r, view, 1u, r->frame_count, r->seed + sample * r->max_bounces, r->accumulate, 0u, n_slots);
    DevMem qo, qd, qT, lsum, ctr;
    TRY(qo.alloc(sizeof(float4) * n_slots));
    TRY(qd.alloc(sizeof(float4) * n_slots));
    TRY(qT.alloc(sizeof(float4) * n_slots));
    TRY(lsum.alloc(sizeof(float4) * n_slots));
    TRY(ctr.alloc(sizeof(FrameCounters)));
    hipStream_t s = r->stream;
    HIP_TRY(hipMemsetAsync(ctr.get(), 0, sizeof(FrameCounters), s));
    const DNoise nz{as<const uint8_t>(r->noise), r->noise_w, r->noise_h, (r->use_noise && r->noise) ? 1u : 0u};
    const Queue q{as<float4>(qo), as<float4>(qd), as<float4>(qT)};
    const bool dense = (r->w % r->tile_w == 0u) && (r->h % r->tile_h == 0u);
    const uint32_t blocks = std::min<uint32_t>(div_up(n_slots, kBlock), (uint32_t)r->dev->compute_units * 8u);   // launch_plan.h stream_blocks
    with_flags([&](auto D, auto L) { hipLaunchKernelGGL((k_raygen<decltype(D)::value, decltype(L)::value>), dim3(blocks), dim3(kBlock), 0, s, p, nz, q, as<float4>(lsum), as<FrameCounters>(ctr)); }, dense, r->lens_r > 0.0f);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    const auto hc = std::make_unique<FrameCounters>();
    HIP_TRY(hipMemcpy(hc.get(), ctr.get(), sizeof(FrameCounters), hipMemcpyDeviceToHost));
    const uint32_t n = QC(hc.get(), 0);
    if (n > n_slots) return fail(LPT_ERR_HIP, "lpt_renderer_primary_rays: k_raygen queued %u rays for %u slots", n, n_slots);
    std::vector<float4> ho(n), hd(n), hT(n);
    if (n) {
        HIP_TRY(hipMemcpy(ho.data(), qo.get(), sizeof(float4) * n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hd.data(), qd.get(), sizeof(float4) * n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hT.data(), qT.get(), sizeof(float4) * n, hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t pxy;
        memcpy(&pxy, &hT[i].w, 4);   // x | y << 13 | sample << 26
        const uint32_t x = pxy & 0x1FFFu, y = (pxy >> 13) & 0x1FFFu;
        if (x >= r->w || y >= r->h) return fail(LPT_ERR_HIP, "lpt_renderer_primary_rays: a queued ray names pixel (%u, %u)", x, y);
        const size_t at = 3u * ((size_t)y * r->w + x);
        origins[at] = ho[i].x; origins[at + 1u] = ho[i].y; origins[at + 2u] = ho[i].z;
        dirs[at] = hd[i].x; dirs[at + 1u] = hd[i].y; dirs[at + 2u] = hd[i].z;
    }
    return LPT_OK;
}

int lpt_renderer_stream(lpt_renderer *r, void **stream) {
    if (!r || !stream) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_stream: null");
    FLUSH_OR_RETURN(r);
    *stream = (void *)r->stream;
    return LPT_OK;
}

int lpt_renderer_synchronize(lpt_renderer *r) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_synchronize: null");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return check_device_error(r);
}

int lpt_renderer_radiance_device_ptr(lpt_renderer *r, void **ptr, size_t *bytes) {
    if (!r || !ptr) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_radiance_device_ptr: null");
    FLUSH_OR_RETURN(r);
    *ptr = r->accum;
    if (bytes) *bytes = sizeof(float4) * (size_t)r->w * r->h;
    return LPT_OK;
}

int lpt_renderer_read_radiance(lpt_renderer *r, float *dst) {
    if (!r || !dst) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_read_radiance: null");
    if (r->pend.n && r->accum && r->world == 1u && r->mode == LPT_BLIT_PATHTRACE) {
        // the frame is still recorded: submit it with its own read-back — every wavefront's pixel rows travel to the host as
        // soon as they are final, under the wavefronts that are still tracing (the recorded calls clear `presented`, so the
        // local target is what is shown)
        ReadPlan plan;
        plan.radiance = dst;
        const int st = flush_pending(r, &plan);
        if (st != LPT_OK) return st;
        const hipError_t se = hipStreamSynchronize(r->stream);
        if (se != hipSuccess) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: %s", hipGetErrorString(se));
        return check_device_error(r);
    }
    FLUSH_OR_RETURN(r);
    if (!r->accum) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: no render target");
    hipError_t e = hipSetDevice(r->dev->ordinal);
    const uint32_t n = r->w * r->h;
    if (e == hipSuccess) { hipLaunchKernelGGL(k_resolve, dim3(div_up(n, kBlock)), dim3(kBlock), 0, r->stream, presented_target(r), r->scratch, n); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(dst, r->scratch, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: %s", hipGetErrorString(e));
    return check_device_error(r);
}

// Host-side gather of a tile-sharded frame: this rank's OWNED pixels (mean radiance) straight into `frame_dst`, a whole-frame destination in page-locked
// host memory (lpt_host_alloc, or any memory passed to lpt_host_register — e.g. a shared-memory segment every rank of the node maps).  Pixels of other ranks
// are not touched.  Blocking.
int lpt_renderer_read_radiance_owned(lpt_renderer *r, float *frame_dst) {
    if (!r || !frame_dst) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_read_radiance_owned: null");
    FLUSH_OR_RETURN(r);
    if (!r->accum) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: no render target");
    if (r->mode != LPT_BLIT_PATHTRACE) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_read_radiance_owned: BlitMode::Pathtrace only (the denoising modes filter the whole frame on rank 0)");
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    void *mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, frame_dst, 0) != hipSuccess || !mapped) {
        (void)hipGetLastError();
        return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_read_radiance_owned: the destination must be page-locked host memory (lpt_host_alloc / lpt_host_register)");
    }
    const FrameParams p = shard_params(r);
    if (p.n_slots) hipLaunchKernelGGL(k_resolve_owned, dim3(stream_grid(r, p.n_slots)), dim3(kBlock), 0, r->stream, p, r->accum, reinterpret_cast<float4 *>(mapped));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: %s", hipGetErrorString(e));
    return check_device_error(r);
}

int lpt_host_register(void *ptr, size_t bytes) {
    if (!ptr || !bytes) return fail(LPT_ERR_INVALID_ARG, "lpt_host_register: null");
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    return LPT_OK;
}
int lpt_host_unregister(void *ptr) {
    if (!ptr) return LPT_OK;
    HIP_TRY(hipHostUnregister(ptr));
    return LPT_OK;
}

int lpt_host_alloc(size_t bytes, void **out) {
    if (!out || !bytes) return fail(LPT_ERR_INVALID_ARG, "lpt_host_alloc: null / zero size");
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return LPT_OK;
}
int lpt_host_free(void *ptr) {
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return LPT_OK;
}

int lpt_renderer_blit_rgba8(lpt_renderer *r, uint8_t *dst, size_t row_bytes) {
    if (!r || !dst || row_bytes < (size_t)r->w * 4) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_blit_rgba8: bad arguments");
    if (r->pend.n && r->accum && r->world == 1u && r->mode == LPT_BLIT_PATHTRACE) {
        // the frame is still recorded: submit it with its own read-back, piece by piece (lpt_renderer_read_radiance does the same)
        ReadPlan plan;
        plan.rgba8 = dst; plan.row_bytes = row_bytes;
        const int st = flush_pending(r, &plan);
        if (st != LPT_OK) return st;
        const hipError_t se = hipStreamSynchronize(r->stream);
        if (se != hipSuccess) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: %s", hipGetErrorString(se));
        return check_device_error(r);
    }
    FLUSH_OR_RETURN(r);
    if (!r->accum) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: no render target");
    hipError_t e = hipSetDevice(r->dev->ordinal);
    const uint32_t n = r->w * r->h;
    if (e == hipSuccess) {
        if ((r->mode == LPT_BLIT_GBUFFER || r->mode == LPT_BLIT_MOTION) && r->has_denoiser())  // debug views (renderer.rs:574-586)
            hipLaunchKernelGGL(k_debug_view, dim3(div_up(n, kBlock)), dim3(kBlock), 0, r->stream, r->den_gbuf[r->den_cur], r->den_motion,
                               (uchar4 *)r->scratch.get(), (int)r->w, (int)r->h, r->mode);
        else
            launch_present(r, r->stream, presented_target(r), (uchar4 *)r->scratch.get(), n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy2DAsync(dst, row_bytes, r->scratch, (size_t)r->w * 4, (size_t)r->w * 4, r->h, hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: %s", hipGetErrorString(e));
    return check_device_error(r);
}

int lpt_renderer_read_pixels(lpt_renderer *r, uint8_t *dst) {
    if (!r || !dst) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_read_pixels: null");
    const int mode = r->mode;  // read_pixels always reads `main` (renderer.rs:769), whatever the blit mode
    if (mode == LPT_BLIT_GBUFFER || mode == LPT_BLIT_MOTION) r->mode = LPT_BLIT_PATHTRACE;
    const int st = lpt_renderer_blit_rgba8(r, dst, (size_t)r->w * 4);
    r->mode = mode;
    return st;
}

// ------------------------------------------------------------------ display transform and metering (SPEC §30)
// what lpt_renderer_set_display and lpt_display_probe accept: a known operator and a finite |ev| <= 64; the gain is rounded once, here
static bool display_args(float ev, uint32_t op, float *gain) {
    if (op >= kDisplayOps || !std::isfinite(ev) || !(std::fabs(ev) <= 64.0f)) return false;
    *gain = (float)std::exp2((double)ev);
    return true;
}
static bool meter_args(float low, float high) {   // a NaN fails every comparison
    return low >= 0.0f && low < 1.0f && high >= 0.0f && high < 1.0f && (double)low + (double)high < 1.0;
}
// k_meter's grid: fixed by the device, whatever the frame's size.  One block per CU measured fastest of 1, 2, 4 and 16 at 1920x1080 (each block ends by
// adding its non-zero words to the same global words); an A/B build may override it
#ifndef LPT_EXP_METER_BLOCKS
#define LPT_EXP_METER_BLOCKS 1u
#endif
static inline uint32_t meter_grid(const lpt_device *dev) { return (uint32_t)std::max(1, dev->compute_units) * LPT_EXP_METER_BLOCKS; }

int lpt_renderer_set_display(lpt_renderer *r, float exposure_ev, uint32_t op) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_display: null");
    float gain;
    if (!display_args(exposure_ev, op, &gain)) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_display: the operator must be an LPT_DISPLAY_* value and the exposure finite with |ev| <= 64");
    r->display_ev = exposure_ev; r->display_gain = gain; r->display_op = op;   // read when pixels are presented: nothing is submitted or reset here
    return LPT_OK;
}
int lpt_renderer_get_display(const lpt_renderer *r, float *exposure_ev, uint32_t *op) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_display: null");
    if (exposure_ev) *exposure_ev = r->display_ev;
    if (op) *op = r->display_op;
    return LPT_OK;
}

int lpt_meter_from_histogram(const uint32_t *hist384, float low, float high, float *ev, uint32_t *counted) {
    if (!hist384) return fail(LPT_ERR_INVALID_ARG, "lpt_meter_from_histogram: null");
    if (!meter_args(low, high)) return fail(LPT_ERR_INVALID_ARG, "lpt_meter_from_histogram: low and high must lie in [0, 1) with low + high < 1");
    uint64_t total = 0;
    for (uint32_t b = 0; b < kMeterBins; ++b) total += hist384[b];
    if (total > 0xFFFFFFFFull) return fail(LPT_ERR_INVALID_ARG, "lpt_meter_from_histogram: the histogram's counts must sum to less than 2^32 (*counted is 32 bits wide)");
    meter_evaluate(hist384, low, high, ev, counted);
    return LPT_OK;
}

int lpt_renderer_meter(lpt_renderer *r, float low, float high, float *ev, uint32_t *hist384, uint32_t *counted, uint32_t *skipped) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_meter: null");
    if (!meter_args(low, high)) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_meter: low and high must lie in [0, 1) with low + high < 1");
    FLUSH_OR_RETURN(r);
    if (!r->accum) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: no render target");
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    if (!r->meter_hist) TRY(r->meter_hist.alloc(kMeterWords));
    uint32_t words[kMeterWords];
    HIP_TRY(hipMemsetAsync(r->meter_hist, 0, sizeof words, r->stream));
    hipLaunchKernelGGL(k_meter, dim3(meter_grid(r->dev)), dim3(kBlock), 0, r->stream, presented_target(r), r->w * r->h, r->meter_hist.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(words, r->meter_hist, sizeof words, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    TRY(check_device_error(r));
    if (hist384) memcpy(hist384, words, sizeof(uint32_t) * kMeterBins);
    if (skipped) *skipped = words[kMeterBins];
    meter_evaluate(words, low, high, ev, counted);
    return LPT_OK;
}

// k_display's own body over caller-supplied accumulators
int lpt_display_probe(lpt_device *dev, uint32_t n, const float *accum_rgba, float exposure_ev, uint32_t op, uint8_t *rgba8) {
    if (!dev || (n && (!accum_rgba || !rgba8))) return fail(LPT_ERR_INVALID_ARG, "lpt_display_probe: null");
    float gain;
    if (!display_args(exposure_ev, op, &gain)) return fail(LPT_ERR_INVALID_ARG, "lpt_display_probe: the operator must be an LPT_DISPLAY_* value and the exposure finite with |ev| <= 64");
    float thr[256];
    srgb_thresholds(thr);
    return run_probe(dev, n, kBlock, {{accum_rgba, sizeof(float4)}, {thr, 0, sizeof thr}}, {{rgba8, sizeof(uchar4)}}, [&](dim3, const DevMem *d) {
        launch_display(op, dev->stream, as<const float4>(d[0]), as<uchar4>(d[2]), n, as<const float>(d[1]), gain);
    });
}
// k_meter itself over caller-supplied accumulators
int lpt_meter_probe(lpt_device *dev, uint32_t n, const float *accum_rgba, uint32_t *hist384, uint32_t *skipped) {
    if (!dev || !hist384 || !skipped || (n && !accum_rgba)) return fail(LPT_ERR_INVALID_ARG, "lpt_meter_probe: null");
    uint32_t words[kMeterWords] = {};
    TRY((run_probe(dev, n, kBlock, {{accum_rgba, sizeof(float4)}}, {{words, 0, sizeof words}}, [&](dim3, const DevMem *d) {
        hipLaunchKernelGGL(k_meter, dim3(meter_grid(dev)), dim3(kBlock), 0, dev->stream, as<const float4>(d[0]), n, as<uint32_t>(d[1]));
    })));
    memcpy(hist384, words, sizeof(uint32_t) * kMeterBins);
    *skipped = words[kMeterBins];
    return LPT_OK;
}

int lpt_renderer_read_denoiser(lpt_renderer *r, uint32_t *gbuffer, float *motion, float *radiance, uint32_t *history) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_read_denoiser: null");
    FLUSH_OR_RETURN(r);
    if (!r->has_denoiser()) return fail(LPT_ERR_READBACK, "failed to read pixels from GPU to CPU: no denoising frame has been traced");
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const size_t n = (size_t)r->w * r->h;
    const int c = r->den_cur;
    if (gbuffer) HIP_TRY(hipMemcpy(gbuffer, r->den_gbuf[c], sizeof(uint4) * n, hipMemcpyDeviceToHost));
    if (motion) HIP_TRY(hipMemcpy(motion, r->den_motion, sizeof(float2) * n, hipMemcpyDeviceToHost));
    if (radiance) HIP_TRY(hipMemcpy(radiance, r->den_rad[c], sizeof(float4) * n, hipMemcpyDeviceToHost));
    if (history) HIP_TRY(hipMemcpy(history, r->den_hist[c], sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return LPT_OK;
}

// Sharded frames (set_shard, world > 1) in a denoising BlitMode: raytrace() leaves this rank's part of the filter inputs —
// noisy radiance (float4), G-buffer (uint4), motion (float2), zero outside its tiles — in full-frame buffers.  The host
// sums them over the ranks (one reduce each; the tiles are disjoint, so the sum is a gather) into rank 0's buffers and
// calls lpt_renderer_denoise_filter there, which runs the temporal / a-trous / composite passes over the whole frame.
int lpt_renderer_denoiser_inputs(lpt_renderer *r, void **noisy, void **gbuffer, void **motion, size_t *n_pixels) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_denoiser_inputs: null");
    FLUSH_OR_RETURN(r);
    if (!r->has_denoiser()) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_denoiser_inputs: no denoising frame has been traced");
    if (noisy) *noisy = r->den_noisy;
    if (gbuffer) *gbuffer = r->den_gbuf[r->den_cur];
    if (motion) *motion = r->den_motion;
    if (n_pixels) *n_pixels = (size_t)r->w * r->h;
    return LPT_OK;
}

int lpt_renderer_denoise_filter(lpt_renderer *r) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_denoise_filter: null");
    FLUSH_OR_RETURN(r);
    if (!r->has_denoiser() || !r->den_inputs_ready) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_denoise_filter: no denoising frame has been traced");
    if (r->world == 1u) return LPT_OK;  // raytrace() has already filtered the frame
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    launch_filter(r, r->stream);
    HIP_TRY(hipGetLastError());
    r->den_inputs_ready = false;
    return LPT_OK;
}

int lpt_renderer_get_ray_counts(lpt_renderer *r, lpt_ray_counts *out) {
    if (!r || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_ray_counts: null");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    Totals t;
    HIP_TRY(hipMemcpyAsync(&t, r->totals, sizeof t, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    out->closest = t.closest; out->shadow = t.shadow; out->shaded = t.shaded; out->nodes = t.nodes; out->tris = t.tris;
    out->shadow_nodes = t.shadow_nodes; out->shadow_tris = t.shadow_tris;
    out->wave_steps = t.wave_steps; out->live_lanes = t.live_lanes; out->node_lanes = t.node_lanes; out->tri_lanes = t.tri_lanes;
    out->primary = t.primary; out->packet_nodes = t.packet_nodes; out->packet_tris = t.packet_tris;
    out->shadow_occluded = t.shadow_occluded; out->occluder_cache_found = t.occ_found; out->occluder_cache_hits = t.occ_hits; out->wave_rays = t.wave_rays;
    return check_device_error(r);
}

int lpt_renderer_reset_ray_counts(lpt_renderer *r) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_reset_ray_counts: null");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipMemsetAsync(r->totals, 0, sizeof(Totals), r->stream));
    return LPT_OK;
}

int lpt_renderer_get_timings(lpt_renderer *r, lpt_timing *out, int *inout_count) {
    if (!r || !inout_count) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_timings: null");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipStreamSynchronize(r->stream));
    lpt_timing acc[ST_COUNT];
    if (!r->ev_start.empty()) for (int k = 0; k < lpt_renderer::kRing; ++k) harvest_slot(r, k);
    for (int i = 0; i < ST_COUNT; ++i) {
        memset(&acc[i], 0, sizeof acc[i]);
        snprintf(acc[i].label, sizeof acc[i].label, "%s", kStageLabel[i]);
        acc[i].ms = (float)r->stage_ms[i];
        acc[i].launches = r->stage_launches[i];
    }
    const int n = std::min(*inout_count, (int)ST_COUNT);
    if (out) for (int i = 0; i < n; ++i) out[i] = acc[i];
    *inout_count = ST_COUNT;
    return LPT_OK;
}

int lpt_renderer_get_queue_counts(lpt_renderer *r, uint32_t *closest, uint32_t *shadow, uint32_t cap) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_queue_counts: null");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    const uint32_t n = std::min<uint32_t>(cap, (uint32_t)kMaxBounces);
    HIP_TRY(hipStreamSynchronize(r->stream));
    const FrameCounters *ctr = r->wf[r->last_lane].ctr;
    if (!ctr) { if (closest) memset(closest, 0, sizeof(uint32_t) * n); if (shadow) memset(shadow, 0, sizeof(uint32_t) * n); return LPT_OK; }
    // FrameCounters keeps (shadow count of bounce b, closest-hit count of bounce b + 1) side by side: unpack
    uint32_t host[2 + 2 * kMaxBounces];
    HIP_TRY(hipMemcpy(host, &ctr->q0, sizeof host, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < n; ++b) {
        if (closest) closest[b] = b == 0u ? host[0] : host[2u + 2u * (b - 1u) + 1u];
        if (shadow) shadow[b] = host[2u + 2u * b];
    }
    return LPT_OK;
}

// stats kernels only: traversal steps per ray over the per-bounce traversal launches of the LAST wavefront (its longest ray sets a launch's duration)
int lpt_renderer_get_step_histogram(lpt_renderer *r, uint32_t *max_steps, uint32_t *hist12) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_get_step_histogram: null");
    FLUSH_OR_RETURN(r);
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const FrameCounters *ctr = r->wf[r->last_lane].ctr;
    if (max_steps) *max_steps = 0;
    if (hist12) memset(hist12, 0, sizeof(uint32_t) * 12);
    if (!ctr) return LPT_OK;
    if (max_steps) HIP_TRY(hipMemcpy(max_steps, &ctr->max_steps, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (hist12) HIP_TRY(hipMemcpy(hist12, ctr->step_hist, sizeof(uint32_t) * 12, hipMemcpyDeviceToHost));
    return LPT_OK;
}

// ============================================================================ multi-GPU frame exchange
int lpt_comm_unique_id(void *out_id) {
    if (!out_id) return fail(LPT_ERR_INVALID_ARG, "lpt_comm_unique_id: null");
    static_assert(sizeof(ncclUniqueId) == LPT_COMM_ID_BYTES, "LPT_COMM_ID_BYTES must match ncclUniqueId");
    const Rccl *nc = rccl();
    if (!nc) return LPT_ERR_RCCL;
    ncclUniqueId id;
    RCCL_TRY(nc->GetUniqueId(&id));
    memcpy(out_id, &id, sizeof id);
    return LPT_OK;
}

int lpt_comm_create(lpt_device *dev, const void *id_bytes, int rank, int world, lpt_comm **out) {
    if (!dev || !id_bytes || !out) return fail(LPT_ERR_INVALID_ARG, "lpt_comm_create: null");
    if (world < 1 || rank < 0 || rank >= world) return fail(LPT_ERR_INVALID_ARG, "lpt_comm_create: rank %d of %d", rank, world);
    const Rccl *nc = rccl();
    if (!nc) return LPT_ERR_RCCL;
    HIP_TRY(hipSetDevice(dev->ordinal));
    ncclUniqueId id;
    memcpy(&id, id_bytes, sizeof id);
    lpt_comm *c = new (std::nothrow) lpt_comm();
    if (!c) return fail(LPT_ERR_INVALID_ARG, "out of host memory");
    c->dev = dev; c->rank = rank; c->world = world;
    ncclResult_t st = nc->CommInitRank(&c->comm, world, id, rank);
    if (st != ncclSuccess) { delete c; return fail(LPT_ERR_RCCL, "ncclCommInitRank(rank %d of %d) failed: %s", rank, world, nc->GetErrorString(st)); }
    *out = c;
    return LPT_OK;
}

int lpt_comm_destroy(lpt_comm *c) {
    if (!c) return LPT_OK;
    hipSetDevice(c->dev->ordinal);
    // renderers still bound to the communicator: their recorded frames leave first, then they are unbound (they keep their shard of the frame; an
    // exchange on them is then the single-GPU no-op instead of a call into a destroyed communicator)
    flush_device(c->dev);
    for (lpt_renderer *r : c->dev->renderers)
        if (r->comm == c) { forget_deferred_exchange(r); hipStreamSynchronize(r->stream); r->comm = nullptr; }
    if (c->comm && rccl()) rccl()->CommDestroy(c->comm);
    delete c;
    return LPT_OK;
}

// rank and size as RCCL itself reports them for the communicator (ncclCommUserRank / ncclCommCount), not the values
// lpt_comm_create was called with: a host (bench.py) uses this to check that the N ranks really joined one communicator
int lpt_comm_info(const lpt_comm *c, int *rank, int *world) {
    if (!c) return fail(LPT_ERR_INVALID_ARG, "lpt_comm_info: null");
    const Rccl *nc = rccl();
    if (!nc) return LPT_ERR_RCCL;
    int rk = -1, n = -1;
    if (c->comm) {
        RCCL_TRY(nc->CommUserRank(c->comm, &rk));
        RCCL_TRY(nc->CommCount(c->comm, &n));
    }
    if (rank) *rank = rk;
    if (world) *world = n;
    return LPT_OK;
}

int lpt_shard_layout_weighted(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t world, uint32_t rank, const uint32_t *weights,
                              uint32_t *out_slots, uint32_t *out_offset) {
    if (!world || rank >= world || !tile_w || !tile_h) return fail(LPT_ERR_INVALID_ARG, "lpt_shard_layout: bad shard (rank %u of %u, tile %ux%u)", rank, world, tile_w, tile_h);
    const uint32_t n_tiles = div_up(width, tile_w) * div_up(height, tile_h), area = tile_w * tile_h;
    if (!weights) {   // unit weights: the closed form (any world size)
        const uint32_t a = shard_slot_offset(n_tiles, world, area, rank), b = shard_slot_offset(n_tiles, world, area, rank + 1u);
        if (out_slots) *out_slots = b - a;
        if (out_offset) *out_offset = a;
        return LPT_OK;
    }
    if (world > kMaxWorld) return fail(LPT_ERR_INVALID_ARG, "weighted shards: at most %u ranks", kMaxWorld);
    uint32_t sum = 0;
    for (uint32_t q = 0; q < world; ++q) { if (weights[q] > kMaxWeight) return fail(LPT_ERR_INVALID_ARG, "weighted shards: weight %u exceeds %u", weights[q], kMaxWeight); sum += weights[q]; }
    if (sum == 0u || sum > kMaxVirtual) return fail(LPT_ERR_INVALID_ARG, "weighted shards: the weights must sum to 1..%u (got %u)", kMaxVirtual, sum);
    std::vector<uint32_t> off;
    make_shard_table(std::vector<uint32_t>(weights, weights + world), world, n_tiles, area, off);
    if (out_slots) *out_slots = off[rank + 1] - off[rank];
    if (out_offset) *out_offset = off[rank];
    return LPT_OK;
}
int lpt_shard_layout(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t world, uint32_t rank, uint32_t *out_slots, uint32_t *out_offset) {
    return lpt_shard_layout_weighted(width, height, tile_w, tile_h, world, rank, nullptr, out_slots, out_offset);
}
// which rank owns tile `tile` (row-major over the tile grid) under the rule above: for hosts and tests that check the layout
int lpt_shard_owner(uint32_t world, const uint32_t *weights, uint32_t tile, uint32_t *out_rank) {
    if (!world || !out_rank || (weights && world > kMaxWorld)) return fail(LPT_ERR_INVALID_ARG, "lpt_shard_owner: bad arguments");
    std::vector<uint32_t> wv;
    if (weights) {
        uint32_t sum = 0;
        for (uint32_t q = 0; q < world; ++q) { if (weights[q] > kMaxWeight) return fail(LPT_ERR_INVALID_ARG, "weighted shards: weight %u exceeds %u", weights[q], kMaxWeight); sum += weights[q]; }
        if (sum == 0u || sum > kMaxVirtual) return fail(LPT_ERR_INVALID_ARG, "weighted shards: the weights must sum to 1..%u (got %u)", kMaxVirtual, sum);
        wv.assign(weights, weights + world);
    }
    const std::vector<uint32_t> owner = deal_virtual_ranks(wv, world);
    *out_rank = owner[tile % owner.size()];
    return LPT_OK;
}

int lpt_renderer_set_comm_weighted(lpt_renderer *r, lpt_comm *comm, const uint32_t *weights) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_comm: null");
    if (comm && comm->dev != r->dev) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_set_comm: the communicator belongs to another device");
    FLUSH_OR_RETURN(r);
    // bind only once the shard is in place: a failed set_shard must not leave a half-bound renderer
    const int st = comm ? lpt_renderer_set_shard_weighted(r, (uint32_t)comm->rank, (uint32_t)comm->world, 32u, 8u, weights) : lpt_renderer_set_shard(r, 0u, 1u, 32u, 8u);
    if (st == LPT_OK) r->comm = comm;
    return st;
}
int lpt_renderer_set_comm(lpt_renderer *r, lpt_comm *comm) { return lpt_renderer_set_comm_weighted(r, comm, nullptr); }

}  // extern "C"

// the sharding half of FrameParams (what k_pack_owned / k_unpack_frame read)
static FrameParams shard_params(const lpt_renderer *r) {
    FrameParams p{};
    p.width = r->w; p.height = r->h;
    p.rank = r->rank; p.world = r->world; p.tile_w = r->tile_w; p.tile_h = r->tile_h;
    p.map = r->map;
    p.block8 = (r->tile_w % 8u == 0u && r->tile_h % 8u == 0u) ? 1u : 0u;
    shard_geometry(r, p.tiles_x, p.n_tiles, p.n_slots);
    return p;
}

// `frame` (the presented whole frame: only where it is written — the root, or every rank of a reduce, which needs a valid
// receive buffer) and the staging area for packed tiles: this rank's slots, or every rank's on the root
static int ensure_exchange_buffers(lpt_renderer *r, bool root, bool want_frame, bool want_stage, size_t bytes_per_slot = 16) {
    const size_t npx = (size_t)r->w * r->h;
    if ((root || want_frame) && !r->frame) TRY(r->frame.alloc(std::max<size_t>(npx, 1)));
    if (!r->xevent) TRY(r->xevent.create());
    if (!want_stage) return LPT_OK;
    const FrameParams p = shard_params(r);
    const size_t slots = root ? (size_t)p.n_tiles * p.tile_w * p.tile_h : (size_t)p.n_slots;
    const size_t need = std::max<size_t>((slots * bytes_per_slot + 15) / 16, 1);   // in float4 units
    if (r->xstage_elems < need) {
        HIP_TRY(hipStreamSynchronize(r->stream));
        r->xstage.reset();
        r->xstage_elems = 0;
        TRY(r->xstage.alloc(need));
        r->xstage_elems = need;
    }
    return LPT_OK;
}
static inline uint32_t stream_grid(const lpt_renderer *r, size_t n) {
    return (uint32_t)std::max<size_t>(1, std::min<size_t>((n + kBlock - 1) / kBlock, (size_t)r->dev->compute_units * 8u));
}

// Phase 1 of an exchange: pack + the RCCL operations, enqueued on the renderer's stream.  Inside an open
// lpt_comm_group_begin / _end bracket RCCL only issues them at the outermost ncclGroupEnd, so whatever consumes the received
// data (phase 2: unpack, filter) must be enqueued after that — lpt_comm_group_end runs the deferred phase 2 of every renderer.
static int exchange_enqueue(lpt_renderer *r, int mode) {
    lpt_comm *c = r->comm;
    hipStream_t s = r->stream;
    const bool root = c->rank == 0;
    const size_t npx = (size_t)r->w * r->h;
    const Rccl &nc = *rccl();
    stage_begin(r, ST_EXCHANGE, s);
    if (r->mode != LPT_BLIT_PATHTRACE) {
        // denoising BlitModes: the per-pixel filter inputs are what is exchanged (zero outside a rank's tiles, so the sums
        // are gathers); rank 0 then filters the whole frame (SPEC §15.5)
        if (mode == LPT_EXCHANGE_REDUCE) {
            RCCL_TRY(nc.Reduce(r->den_noisy, r->den_noisy, 4 * npx, ncclFloat32, ncclSum, 0, c->comm, s));
            RCCL_TRY(nc.Reduce(r->den_gbuf[r->den_cur], r->den_gbuf[r->den_cur], 4 * npx, ncclInt32, ncclSum, 0, c->comm, s));
            RCCL_TRY(nc.Reduce(r->den_motion, r->den_motion, 2 * npx, ncclFloat32, ncclSum, 0, c->comm, s));
            return LPT_OK;
        }
        // owned tiles only: 40 B per owned pixel (41 MB per rank for a 3840x2160 frame on 8 GPUs, against 330 MB of reduces)
        int st = ensure_exchange_buffers(r, root, false, true, 40);
        if (st != LPT_OK) return st;
        const FrameParams p = shard_params(r);
        unsigned char *stage = reinterpret_cast<unsigned char *>(r->xstage.get());
        if (p.n_slots) hipLaunchKernelGGL(k_pack_den, dim3(stream_grid(r, p.n_slots)), dim3(kBlock), 0, s, p, r->den_noisy, r->den_gbuf[r->den_cur], r->den_motion, stage);
        HIP_TRY(hipGetLastError());
        if (root) {
            RCCL_TRY(nc.GroupStart());
            for (uint32_t q = 1; q < p.world; ++q) {
                const uint32_t nq = r->h_offset[q + 1] - r->h_offset[q];
                if (!nq) continue;
                ncclResult_t e = nc.Recv(stage + 40u * (size_t)r->h_offset[q], 40u * (size_t)nq, ncclUint8, (int)q, c->comm, s);
                if (e != ncclSuccess) { nc.GroupEnd(); return fail(LPT_ERR_RCCL, "ncclRecv from rank %u failed: %s", q, nc.GetErrorString(e)); }
            }
            RCCL_TRY(nc.GroupEnd());
        } else if (p.n_slots) {
            RCCL_TRY(nc.Send(stage, 40u * (size_t)p.n_slots, ncclUint8, 0, c->comm, s));
        }
        return LPT_OK;
    }
    int st = ensure_exchange_buffers(r, root, mode == LPT_EXCHANGE_REDUCE, mode == LPT_EXCHANGE_GATHER_TILES);
    if (st != LPT_OK) return st;
    const FrameParams p = shard_params(r);
    if (mode == LPT_EXCHANGE_REDUCE) {
        // every rank passes a valid receive buffer (only the root's is written)
        RCCL_TRY(nc.Reduce(r->accum, r->frame, 4 * npx, ncclFloat32, ncclSum, 0, c->comm, s));
        return LPT_OK;
    }
    if (p.n_slots) hipLaunchKernelGGL(k_pack_owned, dim3(stream_grid(r, p.n_slots)), dim3(kBlock), 0, s, p, r->accum, r->xstage);   // rank 0's offset is 0
    HIP_TRY(hipGetLastError());
    if (root) {
        RCCL_TRY(nc.GroupStart());
        for (uint32_t q = 1; q < p.world; ++q) {
            const uint32_t nq = r->h_offset[q + 1] - r->h_offset[q];
            if (!nq) continue;
            ncclResult_t e = nc.Recv(r->xstage + r->h_offset[q], 4 * (size_t)nq, ncclFloat32, (int)q, c->comm, s);
            if (e != ncclSuccess) { nc.GroupEnd(); return fail(LPT_ERR_RCCL, "ncclRecv from rank %u failed: %s", q, nc.GetErrorString(e)); }
        }
        RCCL_TRY(nc.GroupEnd());
    } else if (p.n_slots) {
        RCCL_TRY(nc.Send(r->xstage, 4 * (size_t)p.n_slots, ncclFloat32, 0, c->comm, s));
    }
    return LPT_OK;
}

// Phase 2: what reads the received data, on the same stream, behind the RCCL operations
static int exchange_finish(lpt_renderer *r, int mode) {
    hipStream_t s = r->stream;
    const bool root = r->comm->rank == 0;
    const size_t npx = (size_t)r->w * r->h;
    if (r->mode != LPT_BLIT_PATHTRACE) {
        if (root && mode == LPT_EXCHANGE_GATHER_TILES) {
            const FrameParams p = shard_params(r);
            hipLaunchKernelGGL(k_unpack_den, dim3(stream_grid(r, npx)), dim3(kBlock), 0, s, p, r->d_table, reinterpret_cast<unsigned char *>(r->xstage.get()), r->den_noisy, r->den_gbuf[r->den_cur], r->den_motion);
        }
        if (root && r->world != 1u) launch_filter(r, s);   // world == 1: raytrace() has filtered already
        stage_end(r, s);
        HIP_TRY(hipGetLastError());
        r->den_inputs_ready = false;
        return LPT_OK;   // the composite has written the local target on rank 0
    }
    if (root && mode == LPT_EXCHANGE_GATHER_TILES) {
        const FrameParams p = shard_params(r);
        hipLaunchKernelGGL(k_unpack_frame, dim3(stream_grid(r, npx)), dim3(kBlock), 0, s, p, r->d_table, r->xstage, r->frame);
    }
    stage_end(r, s);
    HIP_TRY(hipGetLastError());
    r->presented = root;
    return LPT_OK;
}

// one thread drives several communicators inside lpt_comm_group_begin / _end: the second phases wait for the outermost end
struct DeferredFinish { lpt_renderer *r; int mode; };
static thread_local int t_group_depth = 0;
static thread_local std::vector<DeferredFinish> t_deferred;
static void forget_deferred_exchange(lpt_renderer *r) {
    t_deferred.erase(std::remove_if(t_deferred.begin(), t_deferred.end(), [r](const DeferredFinish &d) { return d.r == r; }), t_deferred.end());
}

extern "C" {

int lpt_comm_group_begin(void) {
    const Rccl *nc = rccl();
    if (!nc) return LPT_ERR_RCCL;
    RCCL_TRY(nc->GroupStart());
    ++t_group_depth;
    return LPT_OK;
}
int lpt_comm_group_end(void) {
    const Rccl *nc = rccl();
    if (!nc) return LPT_ERR_RCCL;
    if (t_group_depth <= 0) return fail(LPT_ERR_INVALID_ARG, "lpt_comm_group_end without lpt_comm_group_begin");
    const ncclResult_t e = nc->GroupEnd();
    if (--t_group_depth > 0) { if (e != ncclSuccess) return fail(LPT_ERR_RCCL, "ncclGroupEnd failed: %s", nc->GetErrorString(e)); return LPT_OK; }
    std::vector<DeferredFinish> todo;
    todo.swap(t_deferred);
    if (e != ncclSuccess) return fail(LPT_ERR_RCCL, "ncclGroupEnd failed: %s", nc->GetErrorString(e));
    int st = LPT_OK;
    for (const DeferredFinish &d : todo) {   // the operations are on the streams now: enqueue their consumers
        hipSetDevice(d.r->dev->ordinal);
        const int f = exchange_finish(d.r, d.mode);
        if (st == LPT_OK) st = f;
    }
    return st;
}

int lpt_renderer_exchange(lpt_renderer *r, int mode) {
    if (!r) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange: null");
    if (mode != LPT_EXCHANGE_GATHER_TILES && mode != LPT_EXCHANGE_REDUCE) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange: unknown mode %d", mode);
    FLUSH_OR_RETURN(r);
    if (!r->comm) return LPT_OK;   // single GPU: the local target is the frame
    if (!r->w || !r->h || !r->accum) return LPT_OK;
    lpt_comm *c = r->comm;
    if ((uint32_t)c->rank != r->rank || (uint32_t)c->world != r->world)
        return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange: the renderer's shard (%u of %u) is not the communicator's (%d of %d); call lpt_renderer_set_comm again",
                    r->rank, r->world, c->rank, c->world);
    if (r->mode != LPT_BLIT_PATHTRACE && (!r->has_denoiser() || !r->den_inputs_ready)) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange: no denoising frame has been traced");
    if (!rccl()) return LPT_ERR_RCCL;
    HIP_TRY(hipSetDevice(r->dev->ordinal));
    if (r->timings) { r->ring_pos++; harvest_slot(r, cur_slot(r)); }
    int st = exchange_enqueue(r, mode);
    if (st != LPT_OK) { stage_end(r, r->stream); return st; }   // a failed exchange still closes its timing stage (get_timings after a failure)
    if (t_group_depth > 0) {   // the RCCL operations are only issued by the outermost lpt_comm_group_end: finish there
        t_deferred.push_back(DeferredFinish{r, mode});
        return LPT_OK;
    }
    return exchange_finish(r, mode);
}

int lpt_renderer_exchange_local(lpt_renderer *root, lpt_renderer *const *peers, int n_peers) {
    if (!root || n_peers < 0 || (n_peers && !peers)) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange_local: null");
    if (root->rank != 0u || root->world != (uint32_t)n_peers + 1u)
        return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange_local: root must be rank 0 of %d (is %u of %u)", n_peers + 1, root->rank, root->world);
    const bool den = root->mode != LPT_BLIT_PATHTRACE;   // denoising BlitModes: the filter inputs travel, rank 0 filters
    FLUSH_OR_RETURN(root);
    for (int i = 0; i < n_peers; ++i) if (peers[i]) FLUSH_OR_RETURN(peers[i]);
    if (!root->w || !root->h || !root->accum) return LPT_OK;
    std::vector<char> seen(root->world, 0);
    seen[0] = 1;
    for (int i = 0; i < n_peers; ++i) {
        const lpt_renderer *q = peers[i];
        if (!q || !q->accum || q->w != root->w || q->h != root->h || q->world != root->world || q->tile_w != root->tile_w || q->tile_h != root->tile_h || q->rank >= root->world || seen[q->rank] ||
            q->weights != root->weights || (q->mode != LPT_BLIT_PATHTRACE) != den)
            return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange_local: peer %d does not complete the shard set of the root", i);
        if (den && (!q->has_denoiser() || !q->den_inputs_ready)) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange_local: peer %d has not traced a denoising frame", i);
        seen[q->rank] = 1;
    }
    if (den && (!root->has_denoiser() || !root->den_inputs_ready)) return fail(LPT_ERR_INVALID_ARG, "lpt_renderer_exchange_local: no denoising frame has been traced");
    const size_t bps = den ? 40 : 16;
    HIP_TRY(hipSetDevice(root->dev->ordinal));
    int st = ensure_exchange_buffers(root, true, true, true, bps);
    if (st != LPT_OK) return st;
    const FrameParams p0 = shard_params(root);
    unsigned char *stage0 = reinterpret_cast<unsigned char *>(root->xstage.get());
    if (p0.n_slots) {
        if (den) hipLaunchKernelGGL(k_pack_den, dim3(stream_grid(root, p0.n_slots)), dim3(kBlock), 0, root->stream, p0, root->den_noisy, root->den_gbuf[root->den_cur], root->den_motion, stage0);
        else hipLaunchKernelGGL(k_pack_owned, dim3(stream_grid(root, p0.n_slots)), dim3(kBlock), 0, root->stream, p0, root->accum, root->xstage);
    }
    for (int i = 0; i < n_peers; ++i) {
        lpt_renderer *q = peers[i];
        HIP_TRY(hipSetDevice(q->dev->ordinal));
        st = ensure_exchange_buffers(q, false, false, true, bps);
        if (st != LPT_OK) return st;
        const FrameParams pq = shard_params(q);
        // the root's staging area may still be read by the unpack of its previous exchange
        if (root->xevent_recorded) HIP_TRY(hipStreamWaitEvent(q->stream, root->xevent, 0));
        if (pq.n_slots) {
            if (den) hipLaunchKernelGGL(k_pack_den, dim3(stream_grid(q, pq.n_slots)), dim3(kBlock), 0, q->stream, pq, q->den_noisy, q->den_gbuf[q->den_cur], q->den_motion, reinterpret_cast<unsigned char *>(q->xstage.get()));
            else hipLaunchKernelGGL(k_pack_owned, dim3(stream_grid(q, pq.n_slots)), dim3(kBlock), 0, q->stream, pq, q->accum, q->xstage);
            // the stand-in of ncclSend / ncclRecv inside one process: a (peer) copy into the root's staging area
            HIP_TRY(hipMemcpyPeerAsync(stage0 + bps * (size_t)root->h_offset[pq.rank], root->dev->ordinal, q->xstage, q->dev->ordinal,
                                       bps * (size_t)pq.n_slots, q->stream));
        }
        if (den) q->den_inputs_ready = false;
        HIP_TRY(hipEventRecord(q->xevent, q->stream));
        HIP_TRY(hipSetDevice(root->dev->ordinal));
        HIP_TRY(hipStreamWaitEvent(root->stream, q->xevent, 0));
    }
    if (den) {
        hipLaunchKernelGGL(k_unpack_den, dim3(stream_grid(root, (size_t)root->w * root->h)), dim3(kBlock), 0, root->stream, p0, root->d_table, stage0, root->den_noisy, root->den_gbuf[root->den_cur], root->den_motion);
        launch_filter(root, root->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(root->xevent, root->stream));
        root->xevent_recorded = true;
        root->den_inputs_ready = false;
        return LPT_OK;   // the composite has written the local target
    }
    hipLaunchKernelGGL(k_unpack_frame, dim3(stream_grid(root, (size_t)root->w * root->h)), dim3(kBlock), 0, root->stream, p0, root->d_table, root->xstage, root->frame);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(root->xevent, root->stream));
    root->xevent_recorded = true;
    root->presented = true;
    return LPT_OK;
}

}  // extern "C"
