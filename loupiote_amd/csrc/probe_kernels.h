// probe_kernels.h — the per-element probe kernels (included by device.hip after kernels.h).
//
// A probe runs ONE device function of the shading or traversal kernels (kernels.h, device_math.h) over n caller-supplied elements, one element per thread, for the
// tests and tools that hold that function to a reference: device.hip's "per-element probes" are the entry points, run_probe there the one upload / launch / read-back
// path.  Nothing here is on a frame's path, and none of the functions under test lives here.  A probe whose elements have more than a few fields moves them as rows:
// one plain struct per row, filled by the kernel and read by the host through its field names.
#pragma once
#include "kernels.h"

namespace lptd {

// ------------------------------------------------------------------ rows (device and host)
// lpt_scene_gpu_sample_emitter, one per point: a point without a sample keeps its prim and has zeros behind it
struct EmitterRow { uint32_t prim, sampled; float y[3], wi[3], dist, cl, p_a, E[3]; uint32_t pad[2]; };
// lpt_scene_gpu_shading_normal, one per element: a degenerate triangle (l2 = 0) gives zeros
struct NormalRow { float Ns[3]; uint32_t mapped; };
// lpt_scene_gpu_sample_textures, one per element, and the ABI's out[n][16] as it stands: mra g, b are 1 without the texture, the emissive texel is 1 without one, the
// normal map's raw texel 0 without one; rejected = alpha_rejects (0 in a scene without masks); uv = the interpolated texture coordinate
struct TextureRow { float albedo[3], mra_g, mra_b, emissive[3], normal[3]; uint32_t rejected; float uv[2]; uint32_t pad[2]; };
// lpt_interface_sample
struct InterfaceRowIn { float d[3], Ns[3], Ngf[3], base[3], ior, r4; uint32_t entering, thin; };
struct InterfaceRowOut { float wi[3], weight[3]; uint32_t kind; };
// lpt_interface_sample_rough: the ABI's in[n][19] and out[n][6] as they stand; entering and thin are floats (non-zero: set)
struct RoughRowIn { float d[3], Ns[3], Ngf[3], entering, base[3], ior, thin, roughness, r4, u1, u2; };
struct RoughRowOut { float wi[3], weight[3]; uint32_t kind; };
struct RoughAbiOut { float wi[3], weight[3]; };   // host only: the row without its `kind`
static_assert(sizeof(RoughRowIn) == 19 * 4 && sizeof(RoughRowOut) == 7 * 4 && sizeof(RoughAbiOut) == 6 * 4, "probe rows: the word counts of the C ABI's callers");
// lpt_bsdf_probe: the ABI's in[n][20] as it stands; out = what bsdf_eval gives for L, whether bsdf_sample gave a sample, and the sample (zeros without one)
struct BsdfRowIn { float base[3], roughness, metallic, N[3], Ng[3], V[3], L[3], r3, r4, r5; };
struct BsdfEval { float pspec, f[3], pdf; };
struct BsdfSampled { float L_s[3], weight[3], pdf_s; };
struct BsdfRowOut { BsdfEval eval; uint32_t ok; BsdfSampled sampled; };
struct BsdfAbiOut { BsdfEval eval; BsdfSampled sampled; };   // host only: the ABI's out[n][12], the row without its `ok`
// lpt_scene_gpu_glass_shadow, one per element, and the ABI's out[n][8] as it stands: glass_shadow_eval's channel transmittance, threshold and pass bits (SPEC §27)
struct GlassRow { float tau[3], xi; uint32_t bits, pad[3]; };
static_assert(sizeof(GlassRow) == 8 * 4, "probe rows: the word counts of the C ABI's callers");
static_assert(sizeof(EmitterRow) == 16 * 4 && sizeof(NormalRow) == 4 * 4 && sizeof(TextureRow) == 16 * 4, "probe rows: the word counts of the C ABI's callers");
static_assert(sizeof(InterfaceRowIn) == 16 * 4 && sizeof(InterfaceRowOut) == 7 * 4, "probe rows: the word counts of the C ABI's callers");
static_assert(sizeof(BsdfRowIn) == 20 * 4 && sizeof(BsdfRowOut) == 13 * 4 && sizeof(BsdfAbiOut) == 12 * 4, "probe rows: the word counts of the C ABI's callers");

__device__ __forceinline__ f3 get3(const float *a) { return mk3(a[0], a[1], a[2]); }
__device__ __forceinline__ void put3(float *a, const f3 v) { a[0] = v.x; a[1] = v.y; a[2] = v.z; }

// The 256-entry sRGB decode table into the block's LDS, for the probes whose function takes it as `s_lut`: every thread of a kBlock-thread block calls this before its
// bounds check.  (k_shade stages its own table beside its other LDS set-up; this one is the probes' alone.)
__device__ __forceinline__ void stage_srgb_lut(const DScene &sc, float (&s_lut)[256]) {
    static_assert(kBlock == 256, "one table entry per thread");
    s_lut[threadIdx.x] = sc.srgb_lut[threadIdx.x];
    __syncthreads();
}

// ------------------------------------------------------------------ ray queries
// lpt_trace_closest: one ray per lane, no refill
template <bool MASK = false>
__global__ __launch_bounds__(kTraceBlock) void k_query_closest(DScene sc, const float4 *o, const float4 *d, float4 *hits, uint32_t n) {
    uint2 *stack = reinterpret_cast<uint2 *>(lds_dyn) + threadIdx.x;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 o4 = o[i], d4 = d[i];
    const f3 oo = mk3(o4.x, o4.y, o4.z), dd = mk3(d4.x, d4.y, d4.z);
    Hit h;
    uint32_t a = 0, b = 0;
    traverse<false, false, MASK>(sc, oo, dd, LPT_T_INF, stack, h, a, b);
    intersect_lights(sc, oo, dd, h);
    hits[i] = make_float4(h.t, h.u, h.v, __uint_as_float(h.prim));
}
// lpt_trace_occluded: o.w = the ray's tmax
template <bool MASK = false>
__global__ __launch_bounds__(kTraceBlock) void k_query_occluded(DScene sc, const float4 *o, const float4 *d, uint8_t *out, uint32_t n) {
    uint2 *stack = reinterpret_cast<uint2 *>(lds_dyn) + threadIdx.x;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 o4 = o[i], d4 = d[i];
    Hit h;
    uint32_t a = 0, b = 0;
    out[i] = traverse<true, false, MASK>(sc, mk3(o4.x, o4.y, o4.z), mk3(d4.x, d4.y, d4.z), o4.w, stack, h, a, b) ? 1 : 0;
}

// ------------------------------------------------------------------ environment probe (SPEC §9, §18)
// lpt_probe_sample / lpt_probe_pdf: the functions shade_hit runs, one direction per thread.  u: n x {r6, r7, r8, r9, r1, r2};
// a draw without a sample gives direction 0, density 0, radiance 0
__global__ __launch_bounds__(kBlock) void k_env_sample(DProbe probe, DEnv ev, const float *u, uint32_t n, float *dirs, float *pdf_s, float *radiance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = u + 6u * (size_t)i;
    f3 d;
    float ps = 0.0f;
    f3 Le = mk3(0.f, 0.f, 0.f);
    if (env_sample(ev, r[0], r[1], r[2], r[3], r[4], r[5], d, ps)) Le = env_lookup(probe, d);
    else { d = mk3(0.f, 0.f, 0.f); ps = 0.0f; }
    put3(dirs + 3u * (size_t)i, d);
    pdf_s[i] = ps;
    put3(radiance + 3u * (size_t)i, Le);
}
__global__ __launch_bounds__(kBlock) void k_env_pdf(DEnv ev, const float *dirs, uint32_t n, float *pdf_e) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pdf_e[i] = env_pdf(ev, get3(dirs + 3u * (size_t)i));
}
// lpt_probe_lookup: SPEC §9's env_lookup, the function a miss and every environment sample run, one direction per thread
__global__ __launch_bounds__(kBlock) void k_env_lookup(DProbe probe, const float *dirs, uint32_t n, float *radiance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    put3(radiance + 3u * (size_t)i, env_lookup(probe, get3(dirs + 3u * (size_t)i)));
}

// ------------------------------------------------------------------ lights (SPEC §19, §23)
// lpt_scene_gpu_sample_punctual: punctual_sample, the function shade_hit runs, one point per thread; a point without a sample gives zeros
__global__ __launch_bounds__(kBlock) void k_punctual_sample(DScene sc, uint32_t l, const float *points, uint32_t n, float *wi_out, float *dist_out, float *E_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t j = 3u * (size_t)i;
    f3 wi, E;
    float dist;
    if (!punctual_sample(sc, l, get3(points + j), wi, dist, E)) { wi = mk3(0.f, 0.f, 0.f); E = wi; dist = 0.0f; }
    put3(wi_out + j, wi);
    dist_out[i] = dist;
    put3(E_out + j, E);
}
// lpt_scene_gpu_sample_emitter: emitter_sample, the function shade_hit runs, one point per thread.  rands: (ra, rb, r1, r2) per point
__global__ __launch_bounds__(kBlock) void k_emitter_sample(DScene sc, const float *points, const float *rands, uint32_t n, EmitterRow *out) {
    __shared__ float s_lut[256];
    stage_srgb_lut(sc, s_lut);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = rands + 4u * (size_t)i;
    EmitterSample es;
    const bool ok = emitter_sample(sc, s_lut, r[0], r[1], r[2], r[3], get3(points + 3u * (size_t)i), es);
    EmitterRow row{};
    row.prim = es.prim; row.sampled = ok ? 1u : 0u;
    if (ok) {
        put3(row.y, es.y); put3(row.wi, es.wi);
        row.dist = es.dist; row.cl = es.cl; row.p_a = es.pA;
        put3(row.E, es.E);
    }
    out[i] = row;
}

// ------------------------------------------------------------------ what a hit reads (SPEC §9, §12, §24)
// lpt_scene_gpu_shading_normal: §12's shading normal of a hit (prim, bary) seen along d, through normal_map where the triangle has a map; one element per thread
__global__ __launch_bounds__(kBlock) void k_shading_normal(DScene sc, const uint32_t *prims, const float *bary, const float *dirs, uint32_t n, NormalRow *out) {
    __shared__ float s_lut[256];
    stage_srgb_lut(sc, s_lut);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t prim = prims[i];
    const float hu = bary[2u * (size_t)i], hv = bary[2u * (size_t)i + 1u];
    const f3 d = get3(dirs + 3u * (size_t)i);
    const float4 *tv = sc.tri_verts + kTriRec * (size_t)prim;
    const float4 P0 = tv[0], N0 = tv[1], P1 = tv[2], N1 = tv[3], P2 = tv[4], N2 = tv[5];
    const uint32_t nm = sc.n_nmap ? sc.nmap_tri[prim] : 0u;
    const float bw = (1.0f - hu) - hv;
    const f3 p0 = mk3(P0.x, P0.y, P0.z), p1 = mk3(P1.x, P1.y, P1.z), p2 = mk3(P2.x, P2.y, P2.z);
    f3 Ng = cross(p1 - p0, p2 - p0);
    const float l2 = dot(Ng, Ng);
    f3 Ns = mk3(0.0f, 0.0f, 0.0f);
    bool mapped = false;
    if (l2 > 0.0f) {
        Ng = Ng * (1.0f / sqrtf(l2));
        Ns = mk3((N0.x * bw + N1.x * hu) + N2.x * hv, (N0.y * bw + N1.y * hu) + N2.y * hv, (N0.z * bw + N1.z * hu) + N2.z * hv);
        const float n2 = dot(Ns, Ns);
        Ns = n2 > 0.0f ? Ns * (1.0f / sqrtf(n2)) : Ng;
        if (dot(Ng, d) > 0.0f) Ng = neg(Ng);
        const f3 Nv = Ns;
        const bool flip = dot(Ns, Ng) < 0.0f;
        if (flip) Ns = neg(Ns);
        const float tu = (P0.w * bw + P1.w * hu) + P2.w * hv;
        const float tvv = (N0.w * bw + N1.w * hu) + N2.w * hv;
        if (nm != 0u) mapped = normal_map(sc, s_lut, nm, Nv, Ng, flip, p1 - p0, p2 - p0, P1.w - P0.w, N1.w - N0.w, P2.w - P0.w, N2.w - N0.w, tu, tvv, Ns);
    }
    NormalRow row;
    put3(row.Ns, Ns); row.mapped = mapped ? 1u : 0u;
    out[i] = row;
}

// lpt_scene_gpu_sample_textures: what a hit (prim, bary) reads from its textures (SPEC §9), through the functions and the dispatch of shade_hit (which is repeated
// here, not shared: k_shade sits at its register limit), one element per thread
__global__ __launch_bounds__(kBlock) void k_sample_textures(DScene sc, const uint32_t *prims, const float *bary, uint32_t n, TextureRow *out) {
    __shared__ float s_lut[256];
    stage_srgb_lut(sc, s_lut);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t prim = prims[i];
    const float hu = bary[2u * (size_t)i], hv = bary[2u * (size_t)i + 1u];
    const float4 *tv = sc.tri_verts + kTriRec * (size_t)prim;
    const float4 P0 = tv[0], N0 = tv[1], P1 = tv[2], N1 = tv[3], P2 = tv[4], N2 = tv[5];
    const float4 mp = tv[7];
    const uint32_t em = sc.n_emis ? sc.emis_tri[prim] : 0u;
    const uint32_t nm = sc.n_nmap ? sc.nmap_tri[prim] : 0u;
    const float bw = (1.0f - hu) - hv;
    const float tu = (P0.w * bw + P1.w * hu) + P2.w * hv;
    const float tvv = (N0.w * bw + N1.w * hu) + N2.w * hv;
    f3 alb = mk3(1.0f, 1.0f, 1.0f), emi = mk3(1.0f, 1.0f, 1.0f), nrm = mk3(0.0f, 0.0f, 0.0f);
    float mg = 1.0f, mb = 1.0f;
    const uint32_t atex = __float_as_uint(mp.z), mtex = __float_as_uint(mp.w);
    if ((atex >> 30) == 1u) {   // kPairedBit set, not LPT_INVALID_INDEX
        texture_lookup_pair(sc, s_lut, atex & ~kPairedBit, mtex, tu, tvv, alb, mg, mb);
    } else {
        if (atex < sc.n_images) {
            const float4 tex = texture_lookup(sc, s_lut, atex, tu, tvv, true);
            alb = mk3(tex.x, tex.y, tex.z);
        }
        if (mtex < sc.n_images) {
            const float4 tex = texture_lookup(sc, s_lut, mtex, tu, tvv, false);
            mg = tex.y; mb = tex.z;
        }
    }
    if (em != 0u) {
        const uint32_t etex = __float_as_uint(sc.emis_recs[em - 1u].w);
        if (etex < sc.n_images) {
            const float4 tex = texture_lookup(sc, s_lut, etex, tu, tvv, true);
            emi = mk3(tex.x, tex.y, tex.z);
        }
    }
    if (nm != 0u) {
        const float4 tex = texture_lookup(sc, s_lut, __float_as_uint(sc.nmap_recs[nm - 1u].x), tu, tvv, false);
        nrm = mk3(tex.x, tex.y, tex.z);
    }
    TextureRow row{};
    put3(row.albedo, alb); row.mra_g = mg; row.mra_b = mb;
    put3(row.emissive, emi); put3(row.normal, nrm);
    row.rejected = sc.n_alpha != 0u && alpha_rejects(sc, prim, hu, hv) ? 1u : 0u;
    row.uv[0] = tu; row.uv[1] = tvv;
    out[i] = row;
}

// lpt_scene_gpu_glass_shadow: glass_shadow_eval, the function the traversal's GLASS step runs, one (prim, bary, direction) per thread; a scene without a transmission
// table has no pane (zeros)
__global__ __launch_bounds__(kBlock) void k_glass_shadow(DScene sc, const uint32_t *prims, const float *bary, const float *dirs, uint32_t n, GlassRow *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GlassRow row{};
    if (sc.n_trans != 0u) {
        const GlassShadow g = glass_shadow_eval(sc, prims[i], bary[2u * (size_t)i], bary[2u * (size_t)i + 1u], get3(dirs + 3u * (size_t)i));
        put3(row.tau, g.tau); row.xi = g.xi; row.bits = g.bits;
    }
    out[i] = row;
}

// lpt_scene_gpu_attenuation: volume_attenuate, the function shade_hit<TRANS> runs, on T = (1, 1, 1), one (prim, direction, t) per thread.  `entering` comes from the baked
// triangle exactly as in shade_hit: the raw geometric normal, normalised, against d.  {1, 1, 1, 0} where the rule does not apply; a degenerate triangle is no surface hit
__global__ __launch_bounds__(kBlock) void k_attenuation(DScene sc, const uint32_t *prims, const float *dirs, const float *ts, uint32_t n, float4 *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f3 T = mk3(1.0f, 1.0f, 1.0f);
    bool applies = false;
    const uint32_t prim = prims[i];
    const uint32_t te = sc.n_trans != 0u ? sc.trans_tri[prim] : 0u;
    if (te != 0u) {
        const float4 *tv = sc.tri_verts + kTriRec * (size_t)prim;
        const float4 P0 = tv[0], P1 = tv[2], P2 = tv[4];
        const f3 p0 = mk3(P0.x, P0.y, P0.z), p1 = mk3(P1.x, P1.y, P1.z), p2 = mk3(P2.x, P2.y, P2.z);
        f3 Ng = cross(p1 - p0, p2 - p0);
        const float l2 = dot(Ng, Ng);
        if (l2 > 0.0f) {
            Ng = Ng * (1.0f / sqrtf(l2));
            const bool entering = !(dot(Ng, get3(dirs + 3u * (size_t)i)) > 0.0f);
            applies = volume_attenuate(sc.trans_recs[te - 1u], sc.trans_recs + (sc.n_trans + (te - 1u)), entering, ts[i], T);
        }
    }
    out[i] = make_float4(T.x, T.y, T.z, applies ? 1.0f : 0.0f);
}

// ------------------------------------------------------------------ scattering (SPEC §10, §21)
// lpt_interface_sample: interface_sample, the function shade_hit runs, one element per thread
__global__ __launch_bounds__(kBlock) void k_interface_sample(const InterfaceRowIn *in, uint32_t n, InterfaceRowOut *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const InterfaceRowIn e = in[i];
    const InterfaceOut io = interface_sample(get3(e.d), get3(e.Ns), get3(e.Ngf), e.entering != 0u, get3(e.base), e.ior, e.thin != 0u, e.r4);
    InterfaceRowOut row;
    put3(row.wi, io.wi); put3(row.weight, io.weight); row.kind = io.transmit ? 1u : 0u;
    out[i] = row;
}
// lpt_interface_sample_rough: interface_sample_rough with the rough bit set, the function shade_hit<TRANS> runs, one element per thread.
// kind: 0 reflected, 1 transmitted, 2 the path ended; + 4 where the roughness was below LPT_MIN_ROUGHNESS and the smooth event of §21 was taken
__global__ __launch_bounds__(kBlock) void k_interface_sample_rough(const RoughRowIn *in, uint32_t n, RoughRowOut *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RoughRowIn e = in[i];
    const RoughInterfaceOut ro = interface_sample_rough(get3(e.d), get3(e.Ns), get3(e.Ngf), e.entering != 0.0f, get3(e.base), e.ior, e.thin != 0.0f, true, e.roughness, e.r4, e.u1, e.u2);
    RoughRowOut row;
    put3(row.wi, ro.io.wi); put3(row.weight, ro.io.weight);
    row.kind = (ro.ended ? 2u : ro.io.transmit ? 1u : 0u) | (ro.smooth ? 4u : 0u);
    out[i] = row;
}
// lpt_bsdf_probe: §10 as shade_hit sets it up (make_surface, the clamped NoV, spec_probability), then bsdf_eval on L and bsdf_sample on (r3, r4, r5); one element per thread
__global__ __launch_bounds__(kBlock) void k_bsdf_probe(const BsdfRowIn *in, uint32_t n, BsdfRowOut *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BsdfRowIn e = in[i];
    const f3 N = get3(e.N), Ng = get3(e.Ng), V = get3(e.V);
    const Surface sf = make_surface(get3(e.base), e.roughness, e.metallic);
    const float NoV = max2(dot(N, V), LPT_MIN_NOV);
    const float pspec = spec_probability(sf, NoV);
    f3 f, Ls = mk3(0.0f, 0.0f, 0.0f), w = mk3(0.0f, 0.0f, 0.0f);
    float pdf, pdf_s = 0.0f;
    bsdf_eval(sf, N, Ng, V, NoV, pspec, get3(e.L), f, pdf);
    const bool ok = bsdf_sample(sf, N, Ng, V, NoV, pspec, e.r3, e.r4, e.r5, Ls, w, pdf_s);
    BsdfRowOut row;
    row.eval.pspec = pspec; put3(row.eval.f, f); row.eval.pdf = pdf;
    row.ok = ok ? 1u : 0u;
    put3(row.sampled.L_s, Ls); put3(row.sampled.weight, w); row.sampled.pdf_s = pdf_s;
    out[i] = row;
}

}  // namespace lptd
