"""SPEC.md §29 restated in numpy, from the section alone (test infrastructure).

`interface_sample_rough` is the rough interface event in the SPEC's operation order.  With dtype float32 every operation is one binary32 rounding (numpy's
float32 add, multiply, divide and sqrt are correctly rounded; §5's `sincos2pi` is restated with an exactly rounded fused multiply-add, `fma32`), so it is
what the device hook lpt_interface_sample_rough must return bit for bit.  With dtype float64 the same code, with the exact sine and cosine, is the sampler
of the physics checks and of the scene Monte-Carlo below.

`bsdf_cos` is Walter, Marschner, Li and Torrance, "Microfacet Models for Refraction through Rough Surfaces" (EGSR 2007) in float64, written from the paper's
formulas and NOT from the sampler: the reflection term (eq. 20), the refraction term with its Jacobian (eq. 21, 17), the GGX distribution (eq. 33), Smith's
separable G = G1 G1 (eq. 34, 23) and the exact unpolarised Fresnel term.  A thin-walled pane has no formula in the paper: §29 defines its transmitted lobe as the
reflected lobe mirrored in the surface, weighted 1 - F instead of F, and that is what `bsdf_cos` writes for it.

`pane_expectation` and `scene_monte_carlo` are the float64 references of the two furnace scenes of tests/test_gpu_rough_transmission.py."""
import numpy as np

import transmission_ref as TR

F32 = np.float32
MIN_ROUGHNESS = F32(0.045)
KIND_REFLECT, KIND_TRANSMIT, KIND_ENDED, KIND_SMOOTH = 0, 1, 2, 4

_HALF_PI = F32(1.57079632679489661923)
_SIN_C = [F32(c) for c in (2.7557319223985893e-6, -1.984126984126984e-4, 8.333333333333333e-3, -1.6666666666666666e-1, 1.0)]
_COS_C = [F32(c) for c in (-2.755731922398589e-7, 2.48015873015873e-5, -1.3888888888888889e-3, 4.1666666666666664e-2, -0.5, 1.0)]


# ------------------------------------------------------------------------------------------------ binary32 building blocks
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, ONE rounding.  The product of two binary32 numbers is exact in binary64; the sum with c rounds once to 53 bits, and
    rounding that to 24 bits could round twice — only where the binary64 sum is an exact tie of binary32 while the true sum is not.  The sum's error is
    recovered exactly (Knuth's two-sum) and pushes such a tie to its side.  (No operand here is near the subnormal range.)"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64) if isinstance(c, np.ndarray) else np.float64(c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (err != 0)
    s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def sincos2pi32(u):
    """§5's sincos2pi, bit for bit: (sin, cos)(2 pi u) of a binary32 u in [0, 1)"""
    u = np.asarray(u, F32)
    q = u * F32(4)
    k = q.astype(np.int32)                       # (int)q of a non-negative q
    f = q - k.astype(F32)
    k &= 3
    x = f * _HALF_PI
    x2 = x * x
    ps = fma32(x2, np.full_like(x, _SIN_C[0]), _SIN_C[1])
    for c in _SIN_C[2:]:
        ps = fma32(x2, ps, c)
    sn = x * ps
    pc = fma32(x2, np.full_like(x, _COS_C[0]), _COS_C[1])
    for c in _COS_C[2:-1]:
        pc = fma32(x2, pc, c)
    cs = fma32(x2, pc, _COS_C[-1])
    return np.choose(k, [sn, cs, -sn, -cs]), np.choose(k, [cs, -sn, -cs, sn])


def sincos2pi(u, dtype):
    if dtype == np.float32:
        return sincos2pi32(u)
    return np.sin(2 * np.pi * u), np.cos(2 * np.pi * u)


def onb(n):
    """§10's orthonormal basis in the operation order of the kernels (the dtype of n): -> (T, B)"""
    dt = n.dtype.type
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    sign = np.copysign(dt(1), nz)
    a = dt(-1) / (sign + nz)
    bb = (nx * ny) * a
    T = np.stack([dt(1) + ((sign * nx) * nx) * a, sign * bb, (-sign) * nx], -1)
    B = np.stack([bb, sign + (ny * ny) * a, -ny], -1)
    return T, B


_dot, _normalize = TR._dot, TR._normalize


def g1(x, a2):
    """Smith's G1 for GGX as §29 writes it, x = |cos|"""
    dt = x.dtype.type
    with np.errstate(invalid="ignore", divide="ignore"):
        return (dt(2) * x) / (x + np.sqrt(a2 + (dt(1) - a2) * (x * x)))


# ------------------------------------------------------------------------------------------------ the event
def interface_sample_rough(d, Ns, Ngf, entering, base, ior, thin, rough, r4, u1, u2, dtype=np.float32):
    """§29 for a material whose rough bit is set -> wi[n, 3], weight[n, 3], kind[n] (the hook's: 0 reflected, 1 transmitted, 2 ended, + 4 smooth event)"""
    dt = dtype
    d, Ns, Ngf, base = (np.asarray(a, dt).reshape(-1, 3) for a in (d, Ns, Ngf, base))
    n = d.shape[0]
    ior, rough, r4, u1, u2 = (np.broadcast_to(np.asarray(a, dt), (n,)) for a in (ior, rough, r4, u1, u2))
    entering, thin = (np.broadcast_to(np.asarray(a).astype(bool), (n,)) for a in (entering, thin))
    one, zero = dt(1), dt(0)
    rr = np.minimum(np.maximum(rough, zero), one)
    smooth = rr < dt(MIN_ROUGHNESS)
    eta = np.where(thin | entering, one / ior, ior).astype(dt)
    V = -d
    N = np.where((_dot(V, Ns) > 0)[..., None], Ns, Ngf)
    alpha = rr * rr
    a2 = alpha * alpha
    T, B = onb(N)
    Vh = _normalize(np.stack([alpha * _dot(V, T), alpha * _dot(V, B), _dot(V, N)], -1))
    s, c = sincos2pi(u1, dt)
    s, c = s.astype(dt), c.astype(dt)
    z = (one - u2) * (one + Vh[..., 2]) - Vh[..., 2]
    st = np.sqrt(np.maximum(zero, one - z * z))
    ml = _normalize(np.stack([alpha * (st * c + Vh[..., 0]), alpha * (st * s + Vh[..., 1]), np.maximum(zero, z + Vh[..., 2])], -1))
    m = (T * ml[..., 0:1] + B * ml[..., 1:2]) + N * ml[..., 2:3]
    vm = _dot(V, m)
    cm = np.minimum(vm, one)
    Fr, ct = TR.fresnel(cm, eta)
    reflect = r4 < Fr
    wr = _normalize(m * (dt(2) * cm)[..., None] + d)
    wt = _normalize(d * eta[..., None] + m * (eta * cm - ct)[..., None])
    wt = np.where(thin[..., None], wr - N * (dt(2) * _dot(wr, N))[..., None], wt)
    wi = np.where(reflect[..., None], wr, wt)
    wn, wg = _dot(wi, N), _dot(wi, Ngf)
    valid = (vm > 0) & np.where(reflect, (wn > 0) & (wg > 0), (wn < 0) & (wg < 0))
    g = g1(np.abs(wn), a2)
    weight = np.where(reflect[..., None], np.broadcast_to(g[..., None], (n, 3)), base * g[..., None])
    kind = np.where(valid, np.where(reflect, KIND_REFLECT, KIND_TRANSMIT), KIND_ENDED)
    wi = np.where(valid[..., None], wi, zero)
    weight = np.where(valid[..., None], weight, zero)
    # below the threshold: §21's event, whatever stands above
    swi, sw, str_ = TR.interface_sample(d, Ns, Ngf, entering, base, ior, thin, r4, dtype=dt)
    wi = np.where(smooth[..., None], swi, wi)
    weight = np.where(smooth[..., None], sw, weight)
    kind = np.where(smooth, KIND_SMOOTH + str_.astype(np.int64), kind)
    return wi.astype(dt), weight.astype(dt), kind.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ Walter et al., float64
def ggx_d(nh, a2):
    """eq. 33 for n.h > 0: a2 / (pi ((n.h)^2 (a2 - 1) + 1)^2)"""
    t = nh * nh * (a2 - 1.0) + 1.0
    return np.where(nh > 0, a2 / (np.pi * t * t), 0.0)


def smith_g1(v, h, n, a2):
    """eq. 34 with eq. 23's sidedness: chi+((v.h) / (v.n)) 2 / (1 + sqrt(1 + a2 tan^2))"""
    vn, vh = v @ n, _dot(v, h)
    c2 = vn * vn
    with np.errstate(divide="ignore", invalid="ignore"):
        t2 = (1.0 - c2) / c2
        g = 2.0 / (1.0 + np.sqrt(1.0 + a2 * t2))
    return np.where((vh * vn > 0) & (c2 > 0), g, 0.0)


def bsdf_cos(V, wi, n, eta, a2, base, thin):
    """f(V, wi) |wi.n| of the rough dielectric surface with normal n, seen from V (a unit 3-vector on n's side), at the directions wi[k, 3]: the reflection
    term above the surface and the refraction term (relative index eta = eta_V / eta_far) — or, thin-walled, the mirrored reflection term — below it.
    Transmission carries `base`.  float64, scalars eta, a2, base."""
    V = np.asarray(V, np.float64)
    wi = np.asarray(wi, np.float64)
    wn = wi @ n
    vn = float(V @ n)
    up = wn > 0

    def reflection(wo, weight_of_F):
        h = V + wo
        h = h / np.maximum(np.linalg.norm(h, axis=-1, keepdims=True), 1e-300)
        vh = h @ V
        F, _ = TR.fresnel(np.minimum(np.abs(vh), 1.0), np.full(vh.shape, eta))
        G = smith_g1(np.broadcast_to(V, wo.shape), h, n, a2) * smith_g1(wo, h, n, a2)
        on = wo @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            f = weight_of_F(F) * G * ggx_d(h @ n, a2) / (4.0 * abs(vn) * np.abs(on))        # eq. 20
        return np.where(on > 0, f * np.abs(on), 0.0)

    fr = reflection(wi, lambda F: F)
    if thin:
        ft = base * reflection(wi - 2.0 * wn[:, None] * n, lambda F: 1.0 - F)
    else:
        h = eta * V + wi                                # -(eta_i i + eta_o o) up to a positive factor and the sign, which the next line fixes
        h = h / np.maximum(np.linalg.norm(h, axis=-1, keepdims=True), 1e-300)
        h = np.where((h @ n < 0)[:, None], -h, h)
        vh, oh = h @ V, _dot(wi, h)
        F, _ = TR.fresnel(np.minimum(np.abs(vh), 1.0), np.full(vh.shape, eta))
        G = smith_g1(np.broadcast_to(V, wi.shape), h, n, a2) * smith_g1(wi, h, n, a2)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = eta * vh + oh
            f = (np.abs(vh) * np.abs(oh)) / (abs(vn) * np.abs(wn)) * (1.0 - F) * G * ggx_d(h @ n, a2) / (den * den)     # eq. 21 over eta_o^2
            ft = base * np.where(np.isfinite(f), f, 0.0) * np.abs(wn)
    return np.where(up, fr, np.where(wn < 0, ft, 0.0))


def binned_bsdf(V, n, eta, a2, base, thin, n_theta=16, n_phi=32, sub=(16, 32)):
    """the integral of f |cos| over each (theta, phi) bin of the sphere about n (theta from n, phi about it in onb(n)'s frame): the midpoint rule on
    sub[1]^2 points per bin, and the STATED ERROR of that number: its distance from the same rule on sub[0]^2 points (the rule converges from both sides of a
    smooth integrand at second order, so the coarser rule's distance bounds the finer one's error wherever the integrand is resolved at all)"""
    T, B = onb(np.asarray(n, np.float64)[None])
    T, B = T[0], B[0]
    res = []
    for k in sub:
        th = (np.arange(n_theta * k) + 0.5) * (np.pi / (n_theta * k))
        ph = (np.arange(n_phi * k) + 0.5) * (2 * np.pi / (n_phi * k))
        out = np.zeros((n_theta, n_phi))
        for it in range(n_theta):                      # one band of theta at a time keeps the arrays small
            t = th[it * k:(it + 1) * k]
            tt, pp = np.meshgrid(t, ph, indexing="ij")
            w = (np.sin(tt) * np.cos(pp))[..., None] * T + (np.sin(tt) * np.sin(pp))[..., None] * B + np.cos(tt)[..., None] * n
            f = bsdf_cos(V, w.reshape(-1, 3), n, eta, a2, base, thin).reshape(tt.shape) * np.sin(tt)
            f = f * (np.pi / (n_theta * k)) * (2 * np.pi / (n_phi * k))
            out[it] = f.reshape(k, n_phi, k).sum(axis=(0, 2))
        res.append(out)
    return res[1], np.abs(res[1] - res[0])


def bin_of(wi, n, n_theta=16, n_phi=32):
    """the (theta, phi) bin of each unit direction, in binned_bsdf's frame"""
    T, B = onb(np.asarray(n, np.float64)[None])
    th = np.arccos(np.clip(wi @ n, -1.0, 1.0))
    ph = np.arctan2(wi @ B[0], wi @ T[0]) % (2 * np.pi)
    return np.minimum((th / np.pi * n_theta).astype(int), n_theta - 1), np.minimum((ph / (2 * np.pi) * n_phi).astype(int), n_phi - 1)


# ------------------------------------------------------------------------------------------------ the furnace scenes
def pane_expectation(d, n, base, ior, rough, samples, seed):
    """A thin rough pane with normal n (towards the viewer) before a constant unit probe, seen along the unit direction d, depth 2: the second ray meets nothing
    whichever side it leaves on, so the pixel's value is the event's weight.  -> (E[weight][3], its standard error [3]) from `samples` float64 draws: this is
    E_m[Fr G1(wr) + (1 - Fr) base G1(wt)] — the pick against r4 is integrated by the draw itself, whose variance the standard error carries"""
    rng = np.random.default_rng(seed)
    r4, u1, u2 = rng.random(samples), rng.random(samples), rng.random(samples)
    D = np.broadcast_to(np.asarray(d, np.float64), (samples, 3))
    _, w, _ = interface_sample_rough(D, n, n, True, base, ior, True, rough, r4, u1, u2, dtype=np.float64)
    return w.mean(0), w.std(0, ddof=1) / np.sqrt(samples)


def jittered_rays(view, vfov, w, h, pixels, samples, seed):
    """transmission_ref.camera_rays with a uniform random sub-pixel offset per sample instead of a grid: for the [k, 2] (y, x) list `pixels`, `samples` rays
    each -> origin[3], unit directions[k * samples, 3] (pixel-major)"""
    v = np.asarray(view, np.float64).reshape(4, 4)
    right, up, fwd, origin = v[0, :3], v[1, :3], v[2, :3], v[3, :3]
    th = np.tan(vfov / 2)
    rng = np.random.default_rng(seed)
    pixels = np.repeat(np.asarray(pixels), samples, 0)
    x, y = pixels[:, 1] + rng.random(len(pixels)), pixels[:, 0] + rng.random(len(pixels))
    cx, cy = (2 * x / w - 1) * (w / h * th), (1 - 2 * y / h) * th
    d = right * cx[:, None] + up * cy[:, None] + fwd
    return origin, d / np.linalg.norm(d, axis=-1, keepdims=True)


def scene_monte_carlo(rects, probe, o, d, depth, rough, seed):
    """float64 Monte-Carlo of transmission_ref's flat-rectangle scenes with every glass rectangle rough (roughness `rough`, factor 1, metallic 0): ONE path per
    ray (o[n], d[n]) of at most `depth` shaded hits under the constant probe, §29's event at each hit.  -> the path's radiance[n] (one channel: the scenes have
    grey bases)"""
    rng = np.random.default_rng(seed)
    O, Dr = np.array(np.broadcast_to(np.asarray(o, np.float64), np.shape(d))), np.array(d, np.float64)
    n = O.shape[0]
    T, L = np.ones(n), np.zeros(n)
    alive = np.ones(n, bool)
    last = np.full(n, -1)
    for b in range(depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, hit = TR._nearest(rects, O[idx], Dr[idx], last[idx])
        miss = hit < 0
        L[idx[miss]] += T[idx[miss]] * probe
        alive[idx[miss]] = False
        for i, r in enumerate(rects):
            mi = idx[hit == i]
            if mi.size == 0:
                continue
            if r["kind"] == "emitter":
                L[mi] += T[mi] * r["Le"]
                alive[mi] = False
                continue
            if r["kind"] == "black" or b + 1 >= depth:
                alive[mi] = False
                continue
            dm = Dr[mi]
            P = O[mi] + dm * t[hit == i][:, None]
            flipped = dm @ r["n"] > 0
            Ngf = np.where(flipped[:, None], -r["n"], r["n"])
            wi, w, kind = interface_sample_rough(dm, Ngf, Ngf, ~flipped, np.broadcast_to(r["base"], dm.shape), r["ior"], r["kind"] == "thin", rough,
                                                 rng.random(mi.size), rng.random(mi.size), rng.random(mi.size), dtype=np.float64)
            T[mi] *= w[:, 0]
            O[mi], Dr[mi], last[mi] = P, wi, i
            alive[mi[(kind & 3) == KIND_ENDED]] = False
    return L
