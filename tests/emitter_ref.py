"""A restatement of SPEC.md §23 (emitter sampling), written from the SPEC text and not from the C++ (test infrastructure): §2.5's bake of an instance, the
distribution's entries and weights, the alias build, `emitter_sample`, `p_A`, the pick shares, and a binary64 quadrature of the direct light a rectangular emitter
throws on a Lambertian floor.

binary64 unless stated.  What §23 states as binary32 — the baked positions, `Ng` and `l2` behind the entry test, the slot, and every comparison that decides whether
there is a sample — is binary32 here too (`sample(..., F)` runs the whole chain in binary32; the tests take its decisions and the binary64 chain's values).
tests/emissive_ref.py supplies §9's lookup, tests/alpha_ref.py §20's mask, tests/primary_ref.py the camera rays."""
import numpy as np

import alpha_ref as AR
import emissive_ref as E
import primary_ref as P

F = np.float32


def lum(le, dt=np.float64):
    le = np.asarray(le, dt)
    return (dt(0.2126) * le[..., 0] + dt(0.7152) * le[..., 1]) + dt(0.0722) * le[..., 2]


# ------------------------------------------------------------------ §2.5 the baked positions of one instance (binary32)
def bake(pos, idx, m2w):
    """pos[n, 3] object-space, idx[3t], m2w: the 16 floats of model_to_world (column-major, as the API takes it) -> float32 [t, 3, 3]"""
    m = np.asarray(m2w, F).reshape(16)
    p = np.asarray(pos, F)[np.asarray(idx, np.int64)]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.stack([((m[0] * x + m[4] * y) + m[8] * z) + m[12], ((m[1] * x + m[5] * y) + m[9] * z) + m[13], ((m[2] * x + m[6] * y) + m[10] * z) + m[14]], 1)
    return out.astype(F).reshape(-1, 3, 3)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def ng_l2(tri, dt=F):
    """§12's `Ng = cross(p1 − p0, p2 − p0)`, `l2 = dot(Ng, Ng)` of triangles [t, 3, 3]"""
    t = np.asarray(tri, dt)
    ng = cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return ng, dot(ng, ng)


# ------------------------------------------------------------------ §23 the distribution
def alias_build(w):
    """Vose's alias method as §23 states it -> (q float32[n], alias[n])"""
    w = np.asarray(w, np.float64)
    n = len(w)
    total = 0.0
    for x in w:
        total += float(x)
    sc = [float(x) * float(n) / total for x in w]
    small, large = [i for i in range(n) if sc[i] < 1.0], [i for i in range(n) if not sc[i] < 1.0]
    q, alias = np.ones(n, F), np.arange(n, dtype=np.uint32)
    while small and large:
        s, l = small.pop(), large.pop()
        q[s], alias[s] = F(sc[s]), l
        sc[l] = (sc[l] + sc[s]) - 1.0
        (small if sc[l] < 1.0 else large).append(l)
    return q, alias


def distribution(tris, tri_le):
    """tris: float32 [T, 3, 3] — every baked triangle of the scene in prim-id order; tri_le[T]: its material's Le (float32[3]) or None.
    -> dict(prim, w, sum_w, q, alias) or None when there is no distribution"""
    _, l2 = ng_l2(tris, F)
    prim = [t for t in range(len(tris)) if tri_le[t] is not None and np.any(np.asarray(tri_le[t]) != 0) and l2[t] > 0]
    w = np.array([0.5 * np.sqrt(np.float64(l2[t])) * float(lum(tri_le[t])) for t in prim], np.float64)
    total = 0.0
    for x in w:
        total += float(x)
    if not prim or not total > 0.0:
        return None
    q, alias = alias_build(w)
    return dict(prim=np.array(prim, np.uint32), w=w, sum_w=total, q=q, alias=alias)


def pmf(q, alias):
    """the probability of every entry under (slot uniform, keep with q, else the alias), binary64"""
    n = len(q)
    p = np.zeros(n)
    for i in range(n):
        p[i] += float(q[i]) / n
        p[int(alias[i])] += (1.0 - float(q[i])) / n
    return p


def p_area(le, sum_w):
    """the area density of a point on an emissive triangle of a material with this Le: lum(Le) · inv_W"""
    return float(lum(le)) / sum_w


# ------------------------------------------------------------------ §23 the pick shares
def shares(n_rect, n_punct, env):
    """-> dict(p_env, p_m, p_sel, other): `other` = the factor (1 − p_env)(1 − p_m) that replaces (1 − p_env) in every punctual p_pick and rectangle-light pdf"""
    p_m = 0.5 if n_rect + n_punct > 0 else 1.0
    p_env = 0.5 if env else 0.0
    return dict(p_env=p_env, p_m=p_m, p_sel=(1.0 - p_env) * p_m, other=(1.0 - p_env) * (1.0 - p_m))


# ------------------------------------------------------------------ §23 the sample
def sample(dist, tris, tri_uv, tri_rec, images, rands, Po, dt=np.float64, tri_mask=None):
    """emitter_sample for every row of rands (ra, rb, r1, r2) and Po, the whole chain in `dt`.  tri_uv[T, 3, 2]; tri_rec[T] = (Le, image) or None;
    tri_mask[T] = (cutoff, color.w, alpha image[H, W, 4] or None) for a triangle of a masked material (§20), else None.  The mask's decision at the sampled
    point is binary32 whatever dt (§20 is; so are the barycentrics it is asked at).
    -> dict(prim, ok, y, wi, dist, cl, p_a, E); rows without a sample hold zeros (prim is still the pick)"""
    r = np.asarray(rands, F)
    n_e = len(dist["prim"])
    slot = np.minimum((r[:, 0] * F(n_e)).astype(np.int64), n_e - 1)          # the slot is binary32 whatever dt (§23)
    keep = r[:, 1] < dist["q"][slot]
    prim = np.where(keep, dist["prim"][slot], dist["prim"][dist["alias"][slot]]).astype(np.int64)
    t = np.asarray(tris, dt)[prim]
    r1, r2 = r[:, 2].astype(dt), r[:, 3].astype(dt)
    one = dt(1.0)
    su = np.sqrt(r1)
    u, v = su * (one - r2), su * r2
    bw = (one - u) - v
    y = (t[:, 0] * bw[:, None] + t[:, 1] * u[:, None]) + t[:, 2] * v[:, None]
    ng = cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    l2 = dot(ng, ng)
    w = y - np.asarray(Po, dt)
    d2 = dot(w, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist_ = np.sqrt(d2)
        wi = w * (one / dist_)[:, None]
        cl = np.abs(dot(ng, wi)) * (one / np.sqrt(l2))
        ok = (l2 > 0) & (d2 > 0)
        ok &= np.where(ok, cl, 0) > 0
    n = len(r)
    if tri_mask is not None:                                                 # §20 at the sampled point: a point the mask cuts away gives no sample
        su32 = np.sqrt(r[:, 2])
        u32, v32 = su32 * (F(1.0) - r[:, 3]), su32 * r[:, 3]
        for p in np.unique(prim):
            if tri_mask[p] is not None:
                m = prim == p
                cutoff, color_w, aimg = tri_mask[p]
                ok[m] &= AR.counts(AR.alpha(color_w, aimg, np.asarray(tri_uv, F)[p], u32[m], v32[m]), cutoff)
    p_a, Ev = np.zeros(n, dt), np.zeros((n, 3), dt)
    uv = np.asarray(tri_uv, dt)[prim]
    tu = (uv[:, 0, 0] * bw + uv[:, 1, 0] * u) + uv[:, 2, 0] * v
    tv = (uv[:, 0, 1] * bw + uv[:, 1, 1] * u) + uv[:, 2, 1] * v
    for p in np.unique(prim):
        m = prim == p
        le, image = tri_rec[p]
        p_a[m] = dt(p_area(le, dist["sum_w"]))
        Ev[m] = E.emitted((np.asarray(le, F), image), images, tu[m], tv[m])
    z = ~ok
    out = dict(prim=prim.astype(np.uint32), ok=ok, y=y, wi=wi, dist=dist_, cl=cl, p_a=p_a, E=Ev, tu=tu, tv=tv, bw=bw, u=u, v=v)
    for k in ("y", "wi", "dist", "cl", "p_a", "E"):
        out[k] = np.where(z.reshape((-1,) + (1,) * (out[k].ndim - 1)), 0, out[k])
    return out


# ------------------------------------------------------------------ a rectangular emitter over a Lambertian floor, binary64 quadrature
def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return x, w


def bsdf_f(normal, V, L, albedo):
    """§10's f(V, L) of a dielectric of roughness 1 and metallic 0 in binary64: (albedo/π)(1 − F) + D·vis·F with alpha = 1 (D = 1/π), k = ½, F = 0.04 + 0.96 (1 − VoH)⁵.
    The renderer has no purely Lambertian material: this is albedo/π up to the Fresnel term, which the closed form therefore carries"""
    n = np.asarray(normal, np.float64)
    H = V + L
    H = H / np.linalg.norm(H, axis=-1, keepdims=True)
    NoL, NoV, VoH = np.maximum(L @ n, 0.0), np.maximum(V @ n, 1.0e-4), np.maximum(np.sum(V * H, -1), 0.0)
    Fr = 0.04 + 0.96 * (1.0 - VoH) ** 5
    vis = 1.0 / (4.0 * ((NoL * 0.5 + 0.5) * (NoV * 0.5 + 0.5)))
    return (albedo / np.pi) * (1.0 - Fr) + (1.0 / np.pi) * vis * Fr


def floor_radiance(points, normal, albedo, center, eu, ev, hu, hv, le, order=24, eye=None):
    """∫ f Le cosθ cosθ′ / r² dA over the rectangle center ± hu·eu ± hv·ev (it emits from both sides) for every floor point [n, 3] with unit `normal`; f = albedo/π
    (Lambert) without `eye`, §10's f towards `eye` with it: a Gauss-Legendre product rule of `order`² nodes -> [n]"""
    x, wq = _gauss(order)
    c, eu, ev = (np.asarray(a, np.float64) for a in (center, eu, ev))
    nl = np.cross(eu, ev)
    nl /= np.linalg.norm(nl)
    a, b = np.meshgrid(x * hu, x * hv, indexing="ij")
    wa = np.outer(wq * hu, wq * hv).reshape(-1)
    q = c[None] + a.reshape(-1, 1) * eu[None] + b.reshape(-1, 1) * ev[None]      # [m, 3]
    d = q[None] - np.asarray(points, np.float64)[:, None]                          # [n, m, 3]
    r2 = np.sum(d * d, -1)
    r = np.sqrt(r2)
    cos_s = np.maximum(d @ np.asarray(normal, np.float64), 0.0) / r
    cos_l = np.abs(d @ nl) / r
    f = albedo / np.pi
    if eye is not None:
        V = np.asarray(eye, np.float64)[None] - np.asarray(points, np.float64)
        V /= np.linalg.norm(V, axis=1, keepdims=True)
        f = bsdf_f(normal, V[:, None, :], d / r[..., None], albedo)
    return le * np.sum(f * cos_s * cos_l / r2 * wa[None], 1)


def floor_window_mean(view, vfov, W, H, rows, cols, floor_y, albedo, emitter, le, sub=4, order=24, lambert=False):
    """the mean over the pixel window [rows, cols] of the depth-2 radiance of a white Lambertian floor y = floor_y under `emitter` (the keywords of
    floor_radiance), the camera seeing only the floor: every pixel is the mean over a sub × sub midpoint grid of its area (the jitter is uniform, §4.3).
    -> (mean, err): err = |this − the same at half the sub-pixel grid and half the order|, the stated quadrature error"""
    cam = P.basis(view, W, H, float(F(vfov)))

    def at(sub, order):
        acc = 0.0
        mask = np.zeros((H, W), bool)
        mask[rows, cols] = True
        mask = mask.reshape(-1)
        for i in range(sub):
            for j in range(sub):
                jx, jy = np.full(W * H, (i + 0.5) / sub), np.full(W * H, (j + 0.5) / sub)
                d = P.primary_rays(cam, W, H, jx, jy)[mask]
                t = (floor_y - cam.origin[1]) / d[:, 1]
                assert np.all(t > 0)
                pts = cam.origin[None] + t[:, None] * d
                acc += floor_radiance(pts, (0.0, 1.0, 0.0), albedo, le=le, order=order, eye=None if lambert else cam.origin, **emitter).mean()
        return acc / (sub * sub)

    fine, coarse = at(sub, order), at(max(sub // 2, 1), max(order // 2, 2))
    return fine, abs(fine - coarse)


# ------------------------------------------------------------------ what a weight-1 emitter sample on the LAST bounce would add (a scene of rectangles)
def rect(center, u, v, hu, hv, albedo, le=0.0):
    """the rectangle center ± hu·u ± hv·v (u ⟂ v, unit), shaded on both sides (§12 flips the normal against the ray), roughness 1, metallic 0"""
    c, u, v = (np.asarray(a, np.float64) for a in (center, u, v))
    return dict(c=c, u=u, v=v, hu=float(hu), hv=float(hv), n=np.cross(u, v), albedo=float(albedo), le=float(le))


def _closest(rects, o, d):
    """-> (t [n] (inf: a miss), index [n]) of the closest rectangle along every ray"""
    best, which = np.full(len(o), np.inf), np.full(len(o), -1)
    for k, r in enumerate(rects):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((r["c"][None] - o) @ r["n"]) / (d @ r["n"])
        q = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - r["c"][None]
        hit = np.isfinite(t) & (t > 1.0e-9) & (np.abs(q @ r["u"]) <= r["hu"]) & (np.abs(q @ r["v"]) <= r["hv"]) & (t < best)
        best, which = np.where(hit, t, best), np.where(hit, k, which)
    return best, which


def _direct(rects, lamp, x, n, V, albedo, order=8):
    """∫ f(V, L) Le cosθ cosθ′ / r² dA over the two-sided emitter `lamp` for points x [m, 3] with unit normals n [m, 3] (on V's side) and per-point albedo:
    a Gauss-Legendre product rule; every point of the scenes used lies inside a convex corner with the emitter, so nothing is in between"""
    g, wq = _gauss(order)
    a, b = np.meshgrid(g * lamp["hu"], g * lamp["hv"], indexing="ij")
    wa = np.outer(wq * lamp["hu"], wq * lamp["hv"]).reshape(-1)
    q = lamp["c"][None] + a.reshape(-1, 1) * lamp["u"][None] + b.reshape(-1, 1) * lamp["v"][None]
    d = q[None] - x[:, None]
    r2 = np.sum(d * d, -1)
    r = np.sqrt(r2)
    L = d / r[..., None]
    cos_s = np.maximum(np.sum(L * n[:, None], -1), 0.0)
    cos_l = np.abs(d @ lamp["n"]) / r
    f = _f(n[:, None], V[:, None], L, albedo[:, None])
    return lamp["le"] * np.sum(f * cos_s * cos_l / r2 * wa[None], 1)


def _f(n, V, L, albedo):
    """bsdf_f with a normal per point"""
    H = V + L
    H = H / np.linalg.norm(H, axis=-1, keepdims=True)
    NoL, NoV, VoH = np.maximum(np.sum(L * n, -1), 0.0), np.maximum(np.sum(V * n, -1), 1.0e-4), np.maximum(np.sum(V * H, -1), 0.0)
    Fr = 0.04 + 0.96 * (1.0 - VoH) ** 5
    vis = 1.0 / (4.0 * ((NoL * 0.5 + 0.5) * (NoV * 0.5 + 0.5)))
    return (albedo / np.pi) * (1.0 - Fr) + (1.0 / np.pi) * vis * Fr


def last_bounce_shift(view, vfov, W, H, rows, cols, rects, lamp, depth, spp, seed=1):
    """The window mean of the term a weight-1 emitter sample drawn at the LAST bounce (the hit of index depth − 1) would add to a frame of `depth` bounces: the
    light that goes emitter → a surface → (depth − 1 more surfaces) → camera, one segment more than §22 ever adds.  A binary64 Monte Carlo estimate over `spp`
    paths per window pixel: uniform pixel jitter (§4.3), cosine-distributed directions weighted f·π with §10's f of a dielectric of roughness 1 (bsdf_f) — any
    density gives the same expectation, so the renderer's own lobe pick is not restated —, the last vertex's direct light by quadrature (_direct).
    `rects` holds every surface, `lamp` among them (a path may touch it: its black base reflects §10's specular term).  -> (mean, standard error)"""
    import primary_ref as P
    cam = P.basis(view, W, H, float(F(vfov)))
    rs = np.random.RandomState(seed)
    mask = np.zeros((H, W), bool)
    mask[rows, cols] = True
    mask = mask.reshape(-1)
    npx = int(mask.sum())
    alb, nrm = np.array([r["albedo"] for r in rects]), np.array([r["n"] for r in rects])
    means = []
    for _ in range(spp):
        d = P.primary_rays(cam, W, H, rs.uniform(0, 1, W * H), rs.uniform(0, 1, W * H))[mask]
        o = np.broadcast_to(cam.origin[None], d.shape).copy()
        T, live = np.ones(npx), np.ones(npx, bool)
        for b in range(depth):
            t, k = _closest(rects, o, d)
            live &= np.isfinite(t)
            k = np.where(live, k, 0)
            x = o + np.where(live, t, 0.0)[:, None] * d
            n = nrm[k] * np.where(np.sum(nrm[k] * d, -1) > 0, -1.0, 1.0)[:, None]
            V = -d
            if b == depth - 1:
                break
            # a cosine-distributed direction about n: f cos / (cos / pi) = f pi
            r1, r2 = rs.uniform(0, 1, npx), rs.uniform(0, 1, npx)
            ph, sr = 2.0 * np.pi * r1, np.sqrt(r2)
            tx = np.where(np.abs(n[:, :1]) > 0.5, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
            e1 = np.cross(n, tx)
            e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
            e2 = np.cross(n, e1)
            L = e1 * (sr * np.cos(ph))[:, None] + e2 * (sr * np.sin(ph))[:, None] + n * np.sqrt(1.0 - r2)[:, None]
            T = T * _f(n, V, L, alb[k]) * np.pi
            o, d = x + 1.0e-7 * n, L
        est = np.zeros(npx)
        if live.any():
            est[live] = T[live] * _direct(rects, lamp, x[live], n[live], V[live], alb[k][live])
        means.append(est.mean())
    means = np.array(means)
    return float(means.mean()), float(means.std(ddof=1) / np.sqrt(spp))
