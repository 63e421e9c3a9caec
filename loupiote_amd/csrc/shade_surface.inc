// The body of shade_hit / shade_hit_early (kernels.h) from the hit's barycentric weight on: the surface branch behind its shading record, the G-buffer record and the
// function's end.  Included ONCE IN EACH of the two, as text, so that the two functions share every line of the shading arithmetic and differ only in how a hit's
// first loads are issued (their heads) and in four places that say where a value comes from.  The including function defines, and undefines behind the include:
//   LPT_SHADE_EMIS_TABLES             the scene whose image table an emissive image is looked up in
//   LPT_SHADE_ADD_L(r, g, b)          the add of an emissive surface's radiance
//   LPT_SHADE_NOISE(nz, x, y, s, a, b)   the noise texture's shift of the two draws
//   LPT_SHADE_LIGHT_ROWS(cs, li, n4, t4, b4, lo4)   declares the four rows of rectangle light li
// In scope: P0 N0 P1 N1 P2 N2 mc mp (the record), em nm te (the side-table words), hu hv, and everything shade_hit declares in front of its branches.
        float bw = (1.0f - hu) - hv;
        const f3 p0 = mk3(P0.x, P0.y, P0.z), p1 = mk3(P1.x, P1.y, P1.z), p2 = mk3(P2.x, P2.y, P2.z);
        f3 P = mk3((p0.x * bw + p1.x * hu) + p2.x * hv, (p0.y * bw + p1.y * hu) + p2.y * hv, (p0.z * bw + p1.z * hu) + p2.z * hv);
        f3 Ng = cross(p1 - p0, p2 - p0);
        float l2 = dot(Ng, Ng);
        if (l2 > 0.0f) {
            out.is_surface = true;
            Ng = Ng * (1.0f / sqrtf(l2));
            f3 Ns = mk3((N0.x * bw + N1.x * hu) + N2.x * hv, (N0.y * bw + N1.y * hu) + N2.y * hv, (N0.z * bw + N1.z * hu) + N2.z * hv);
            float n2 = dot(Ns, Ns);
            Ns = n2 > 0.0f ? Ns * (1.0f / sqrtf(n2)) : Ng;
            const bool entering = !(dot(Ng, d) > 0.0f);   // (read by TRANS only)
            if (dot(Ng, d) > 0.0f) Ng = neg(Ng);
            // SPEC §28: behind the rare branch, and before the texture taps and everything at the hit that reads T
            if (TRANS && te != 0u && !entering) {
                const DScene &vs = cold().sc;
                volume_attenuate(vs.trans_recs[te - 1u], vs.trans_recs + (vs.n_trans + (te - 1u)), entering, h4.x, T);
            }
            const f3 Nv = Ns;   // (read by NMAP only: §12's normal before the flip)
            const bool flip = dot(Ns, Ng) < 0.0f;
            if (flip) Ns = neg(Ns);
            float tu = (P0.w * bw + P1.w * hu) + P2.w * hv;
            float tvv = (N0.w * bw + N1.w * hu) + N2.w * hv;
            // SPEC §24: behind the divergent branch, and before the material's own taps, so that the edges and the uv deltas are dead by then
            if (NMAP && nm != 0u) normal_map(cold().sc, s_lut, nm, Nv, Ng, flip, p1 - p0, p2 - p0, P1.w - P0.w, N1.w - N0.w, P2.w - P0.w, N2.w - N0.w, tu, tvv, Ns);
            f3 base = mk3(mc.x, mc.y, mc.z);
            float rough = mp.x, metal = mp.y;
            const uint32_t atex = __float_as_uint(mp.z), mtex = __float_as_uint(mp.w);
            const DScene &ts = cold().sc;   // the texture tables
            if ((atex >> 30) == 1u) {   // kPairedBit set, not LPT_INVALID_INDEX: both textures of the material from one set of taps
                f3 alb;
                float mg, mb;
                texture_lookup_pair(ts, s_lut, atex & ~kPairedBit, mtex, tu, tvv, alb, mg, mb);
                base.x *= alb.x; base.y *= alb.y; base.z *= alb.z;
                rough *= mg; metal *= mb;
            } else {
                if (atex < ts.n_images) {
                    const float4 tex = texture_lookup(ts, s_lut, atex, tu, tvv, true);
                    base.x *= tex.x; base.y *= tex.y; base.z *= tex.z;
                }
                if (mtex < ts.n_images) {
                    const float4 tex = texture_lookup(ts, s_lut, mtex, tu, tvv, false);
                    rough *= tex.y; metal *= tex.z;
                }
            }
            if (EMIS && em != 0u) {   // SPEC §22: weight 1 whatever the ray's pdf, both sides (the flipped Ng plays no part), the last bounce included
                const DScene &cs = cold().sc;
                const float4 er = cs.emis_recs[em - 1u];
                f3 E = mk3(er.x, er.y, er.z);
                const uint32_t etex = __float_as_uint(er.w);
                if (etex < LPT_SHADE_EMIS_TABLES.n_images) {
                    const float4 tex = texture_lookup(LPT_SHADE_EMIS_TABLES, s_lut, etex, tu, tvv, true);
                    E.x *= tex.x; E.y *= tex.y; E.z *= tex.z;
                }
                if (ESAMP) {   // SPEC §23: the BSDF strategy's weight against the emitter sample that could have found this point; a ray without a pdf keeps weight 1
                    const float pdf_prev = load_o().w;
                    if (pdf_prev >= 0.0f) {
                        const float cl = fabsf(dot(Ng, d));
                        const float pA = lum(mk3(er.x, er.y, er.z)) * cs.emit_inv_W;
                        const float p_sel = (ENV ? 0.5f : 1.0f) * ((PUNCT || cs.n_lights) ? 0.5f : 1.0f);
                        const float pl = (((h4.x * h4.x) / cl) * pA) * p_sel;
                        const float pb2 = pdf_prev * pdf_prev;
                        const float w = pb2 / (pb2 + pl * pl);
                        E = mk3(E.x * w, E.y * w, E.z * w);
                    }
                }
                LPT_SHADE_ADD_L(T.x * E.x, T.y * E.y, T.z * E.z);
            }
            g_n = Ns; g_P = P;
            g_alb = mk3(clampf(base.x, 0.0f, 1.0f), clampf(base.y, 0.0f, 1.0f), clampf(base.z, 0.0f, 1.0f));
            const Surface sf = make_surface(base, rough, metal);
            const f3 V = neg(d);
            const float NoV = max2(dot(Ns, V), LPT_MIN_NOV);
            const float pspec = spec_probability(sf, NoV);
            const uint32_t x = pxy & 0x1FFFu, y = (pxy >> 13) & 0x1FFFu, sample = pxy >> 26;
            const uint32_t pixel = y * p.width + x;
            const uint32_t seed_counter = seed_base + sample * p.max_bounces;
            Rng rg = rng_init(pixel, stage_seed(p.user_seed, seed_counter), LPT_TAG_SHADE);
            float r0 = rng_next(rg), r1 = rng_next(rg), r2 = rng_next(rg);
            float r3 = rng_next(rg), r4 = rng_next(rg), r5 = rng_next(rg);
            const ShadeCold c = cold();   // the noise texture here, the lights and the side tables in next-event estimation below
            const DScene &cs = c.sc;
            LPT_SHADE_NOISE(c.nz, x, y, seed_counter, r4, r5);
            float r6 = 0.0f, r7 = 0.0f, r8 = 0.0f, r9 = 0.0f;
            if (ENV) { r6 = rng_next(rg); r7 = rng_next(rg); r8 = rng_next(rg); r9 = rng_next(rg); }
            float ra = 0.0f, rb = 0.0f;   // ESAMP: the alias pick, behind every draw the other modes make
            if (ESAMP) { ra = rng_next(rg); rb = rng_next(rg); }
            const float p_env = (PUNCT || ESAMP || cs.n_lights) ? 0.5f : 1.0f;   // ENV: the probe's share of the light samples
            const float p_m = (PUNCT || cs.n_lights) ? 0.5f : 1.0f;   // ESAMP: the emitters' share of the non-probe light samples
            float am = max2(max2(fabsf(P.x), fabsf(P.y)), fabsf(P.z));
            float eps = 1.0e-4f * (1.0f + am);
            const f3 Po = mk3(P.x + Ng.x * eps, P.y + Ng.y * eps, P.z + Ng.z * eps);
            bool glass = false;   // TRANS: this hit is an interface event (SPEC §21)
            if (TRANS) {
                if (te != 0u) {
                    const float4 tr = cs.trans_recs[te - 1u];   // transmission, ior, thin
                    const float pt = tr.x * (1.0f - clampf(metal, 0.0f, 1.0f));
                    if (r3 < pt) {
                        glass = true;
                        if (!last_bounce) {
                            // SPEC §29: the record's `thin` carries the rough bit in its sign (-0 / -1), so its test against 0 reads as before; u1 = r5, u2 = r1 are drawn
                            // and unused at an interface event
                            const RoughInterfaceOut ro = interface_sample_rough(d, Ns, Ng, entering, base, tr.y, tr.z != 0.0f, (__float_as_uint(tr.z) >> 31) != 0u, rough, r4, r5, r1);
                            const InterfaceOut io = ro.io;
                            const f3 Tn = mk3(T.x * io.weight.x, T.y * io.weight.y, T.z * io.weight.z);
                            if (!ro.ended && (Tn.x > 0.0f || Tn.y > 0.0f || Tn.z > 0.0f)) {
                                const f3 Pn = io.transmit ? mk3(P.x - Ng.x * eps, P.y - Ng.y * eps, P.z - Ng.z * eps) : Po;
                                out.want_next = true;
                                out.no4 = make_float4(Pn.x, Pn.y, Pn.z, -1.0f);   // no pdf: what this ray finds is taken with weight 1
                                out.nd4 = make_float4(io.wi.x, io.wi.y, io.wi.z, d4.w);
                                out.nT4 = make_float4(Tn.x, Tn.y, Tn.z, T4.w);
                            }
                        }
                    } else {
                        r3 = (r3 - pt) / (1.0f - pt);
                    }
                }
            }
            // next-event estimation
            if (TRANS && glass) {   // none at an interface
            } else if (ENV && r0 < p_env) {   // the probe (SPEC §18)
                f3 wi;
                float ps;
                if (env_sample(ev, r6, r7, r8, r9, r1, r2, wi, ps)) {
                    Hit hl;
                    hl.t = LPT_T_INF; hl.u = 0.f; hl.v = 0.f; hl.prim = 0xFFFFFFFFu;
                    intersect_lights(cs, Po, wi, hl);   // a BSDF ray this way would stop at the light's front: not the probe's direction
                    if (hl.prim == 0xFFFFFFFFu) {
                        f3 f;
                        float pb;
                        bsdf_eval(sf, Ns, Ng, V, NoV, pspec, wi, f, pb);
                        if (pb > 0.0f) {
                            const f3 Le = env_lookup(c.probe, wi);
                            const float pe = p_env * env_pdf(ev, wi);
                            const float pe2 = pe * pe;
                            const float wm = last_bounce ? 1.0f : pe2 / (pe2 + pb * pb);   // the last bounce: no BSDF ray carries the other half
                            const float NoL = dot(Ns, wi);
                            const float k = (NoL * wm) / (p_env * ps);
                            f3 contrib = mk3(((T.x * f.x) * Le.x) * k, ((T.y * f.y) * Le.y) * k, ((T.z * f.z) * Le.z) * k);
                            if (contrib.x > 0.0f || contrib.y > 0.0f || contrib.z > 0.0f) {
                                out.want_shadow = true;
                                out.so4 = make_float4(Po.x, Po.y, Po.z, LPT_T_INF);
                                out.sd4 = make_float4(wi.x, wi.y, wi.z, d4.w);
                                out.sc4 = make_float4(contrib.x, contrib.y, contrib.z, 0.f);
                            }
                        }
                    }
                }
            } else if (ESAMP && light_rl<ENV, false>(r0, p_env, p_m) < p_m) {   // the emissive triangles (SPEC §23)
                // the last bounce draws none: a sample there would stand for emission one bounce deeper than §22 adds
                EmitterSample es;
                if (!last_bounce && emitter_sample(cs, s_lut, ra, rb, r1, r2, Po, es)) {
                    Hit hl;
                    hl.t = es.dist; hl.u = 0.f; hl.v = 0.f; hl.prim = 0xFFFFFFFFu;
                    intersect_lights(cs, Po, es.wi, hl);   // §19's rule: a rectangle light's front on the segment
                    if (hl.prim == 0xFFFFFFFFu) {
                        f3 f;
                        float pb;
                        bsdf_eval(sf, Ns, Ng, V, NoV, pspec, es.wi, f, pb);
                        if (pb > 0.0f) {
                            const float pl = ((es.d2 / es.cl) * es.pA) * ((ENV ? 0.5f : 1.0f) * p_m);
                            const float pl2 = pl * pl;
                            const float wm = pl2 / (pl2 + pb * pb);
                            const float NoL = dot(Ns, es.wi);
                            f3 contrib = mk3((T.x * f.x) * (((NoL * es.E.x) * wm) / pl), (T.y * f.y) * (((NoL * es.E.y) * wm) / pl), (T.z * f.z) * (((NoL * es.E.z) * wm) / pl));
                            if (contrib.x > 0.0f || contrib.y > 0.0f || contrib.z > 0.0f) {
                                out.want_shadow = true;
                                out.so4 = make_float4(Po.x, Po.y, Po.z, es.dist * 0.999f);
                                out.sd4 = make_float4(es.wi.x, es.wi.y, es.wi.z, d4.w);
                                out.sc4 = make_float4(contrib.x, contrib.y, contrib.z, 0.f);
                            }
                        }
                    }
                }
            } else if (PUNCT && light_rl<ENV, ESAMP>(r0, p_env, p_m) < pk.p_p) {   // a punctual light (SPEC §19): a delta light, so MIS weight 1 and no draw beyond r0
                const float rl = light_rl<ENV, ESAMP>(r0, p_env, p_m);
                uint32_t li = (uint32_t)((rl / pk.p_p) * (float)cs.n_punctual);
                if (li > cs.n_punctual - 1u) li = cs.n_punctual - 1u;
                f3 wi, E;
                float dist;
                if (punctual_sample(cs, li, Po, wi, dist, E)) {
                    Hit hl;
                    hl.t = dist; hl.u = 0.f; hl.v = 0.f; hl.prim = 0xFFFFFFFFu;
                    intersect_lights(cs, Po, wi, hl);   // a rectangle light's front on the segment: shadow rays test triangles only, and it would stop a BSDF ray too
                    if (hl.prim == 0xFFFFFFFFu) {
                        f3 f;
                        float pb;
                        bsdf_eval(sf, Ns, Ng, V, NoV, pspec, wi, f, pb);
                        if (pb > 0.0f) {
                            const float NoL = dot(Ns, wi);
                            f3 contrib = mk3((T.x * f.x) * ((NoL * E.x) / pk.p_pick), (T.y * f.y) * ((NoL * E.y) / pk.p_pick), (T.z * f.z) * ((NoL * E.z) / pk.p_pick));
                            if (contrib.x > 0.0f || contrib.y > 0.0f || contrib.z > 0.0f) {
                                out.want_shadow = true;
                                out.so4 = make_float4(Po.x, Po.y, Po.z, dist < LPT_T_INF ? dist * 0.999f : LPT_T_INF);
                                out.sd4 = make_float4(wi.x, wi.y, wi.z, d4.w);
                                out.sc4 = make_float4(contrib.x, contrib.y, contrib.z, 1.0f);   // SPEC §27's mark: a delta light's ray may pass thin panes (read by k_trace_glass alone)
                            }
                        }
                    }
                }
            } else if (cs.n_lights) {
                float rl = light_rl<ENV, ESAMP>(r0, p_env, p_m);
                if (PUNCT) rl = (rl - pk.p_p) / (1.0f - pk.p_p);
                uint32_t li = (uint32_t)(rl * (float)cs.n_lights);
                if (li > cs.n_lights - 1u) li = cs.n_lights - 1u;
                LPT_SHADE_LIGHT_ROWS(cs, li, n4, t4, b4, lo4);
                const float Le = lo4.w, hw = t4.w, hh = b4.w;
                float a = (2.0f * r1 - 1.0f) * hw, bq = (2.0f * r2 - 1.0f) * hh;
                f3 qp = mk3((lo4.x + t4.x * a) + b4.x * bq, (lo4.y + t4.y * a) + b4.y * bq, (lo4.z + t4.z * a) + b4.z * bq);
                f3 w = qp - Po;
                float d2 = dot(w, w);
                if (Le > 0.0f && d2 > 0.0f) {
                    float dist = sqrtf(d2);
                    f3 wi = w * (1.0f / dist);
                    float cl = -dot(mk3(n4.x, n4.y, n4.z), wi);
                    if (cl > 0.0f) {
                        f3 f;
                        float pb;
                        bsdf_eval(sf, Ns, Ng, V, NoV, pspec, wi, f, pb);
                        if (pb > 0.0f) {
                            float area = 4.0f * (hw * hh);
                            float pl = (d2 / (cl * area)) * inv_nl;
                            float pl2 = pl * pl;
                            float wm = pl2 / (pl2 + pb * pb);
                            float NoL = dot(Ns, wi);
                            float k = ((NoL * Le) * wm) / pl;
                            f3 contrib = mk3((T.x * f.x) * k, (T.y * f.y) * k, (T.z * f.z) * k);
                            if (contrib.x > 0.0f || contrib.y > 0.0f || contrib.z > 0.0f) {
                                out.want_shadow = true;
                                out.so4 = make_float4(Po.x, Po.y, Po.z, dist * 0.999f);
                                out.sd4 = make_float4(wi.x, wi.y, wi.z, d4.w);
                                out.sc4 = make_float4(contrib.x, contrib.y, contrib.z, 0.f);
                            }
                        }
                    }
                }
            }
            // BSDF sample -> next ray
            if (!last_bounce && !(TRANS && glass)) {
                f3 Ln, wgt;
                float pdf;
                if (bsdf_sample(sf, Ns, Ng, V, NoV, pspec, r3, r4, r5, Ln, wgt, pdf)) {
                    f3 Tn = mk3(T.x * wgt.x, T.y * wgt.y, T.z * wgt.z);
                    if (Tn.x > 0.0f || Tn.y > 0.0f || Tn.z > 0.0f) {
                        out.want_next = true;
                        out.no4 = make_float4(Po.x, Po.y, Po.z, pdf);
                        out.nd4 = make_float4(Ln.x, Ln.y, Ln.z, d4.w);
                        out.nT4 = make_float4(Tn.x, Tn.y, Tn.z, T4.w);
                    }
                }
            }
        }
    }
    if (GBUF && bounce == 0) {
        const GBufArgs &gb = cold().gb;
        const uint32_t gx = pxy & 0x1FFFu, gy = (pxy >> 13) & 0x1FFFu;
        const size_t px = (size_t)gy * p.width + gx;
        gb.gbuf[px] = make_uint4(prim, __float_as_uint(h4.x), oct_encode(g_n), pack_albedo(g_alb));
        float mu = 0.0f, mv = 0.0f, cu, cv, pu, pv;
        if (prim != 0xFFFFFFFFu && project(gb.cur, g_P, cu, cv) && project(gb.prev, g_P, pu, pv)) { mu = pu - cu; mv = pv - cv; }
        gb.motion[px] = make_float2(mu, mv);
    }
}
