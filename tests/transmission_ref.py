"""SPEC.md §21 restated in numpy, from the section alone (no kernel source was consulted for the arithmetic).

`interface_sample` is the interface event in the SPEC's operation order; with dtype float32 every operation is one binary32 rounding (numpy's
float32 add, multiply, divide and sqrt are correctly rounded), so it is what the device hook must return bit for bit.  With dtype float64 the same
code serves the physics self-checks.

`expectation` is a float64 expectation for scenes of flat rectangles — thin panes, the faces of solids, one rectangle emitter — under a constant
probe: it follows BOTH branches of every interface event down to the depth limit (at most 2^depth leaves per ray), so a pixel's mean, its per-sample
variance and the probability of each leaf value are sums over the tree, with no sampling.  Pixel jitter is integrated on an n x n sub-pixel grid."""
import numpy as np


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]   # §3: (x + y) + z


def _normalize(a):
    l2 = _dot(a, a)
    one = l2.dtype.type(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = one / np.sqrt(l2)
    return np.where((l2 > 0)[..., None], a * inv[..., None], a.dtype.type(0))


def fresnel(c, eta):
    """-> (Fr, ct); total internal reflection (s2 >= 1): Fr = 1, ct = 0"""
    dt = c.dtype.type
    s2 = (eta * eta) * np.maximum(dt(0), dt(1) - c * c)
    tir = s2 >= dt(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ct = np.sqrt(np.where(tir, dt(0), dt(1) - s2))
        rs = (eta * c - ct) / (eta * c + ct)
        rp = (c - eta * ct) / (c + eta * ct)
        Fr = dt(0.5) * (rs * rs + rp * rp)
    return np.where(tir, dt(1), Fr), np.where(tir, dt(0), ct)


def _once(d, N, Ngf, eta, thin, r4):
    dt = d.dtype.type
    c = np.minimum(_dot(-d, N), dt(1))
    Fr, ct = fresnel(c, eta)
    reflect = r4 < Fr
    wr = _normalize(N * (dt(2) * c)[..., None] + d)
    wt = np.where(thin[..., None], d, _normalize(d * eta[..., None] + N * (eta * c - ct)[..., None]))
    wi = np.where(reflect[..., None], wr, wt)
    side = _dot(wi, Ngf)
    wrong = np.where(reflect, side <= 0, side >= 0)
    return wi, ~reflect, wrong, Fr


def interface_sample(d, Ns, Ngf, entering, base, ior, thin, r4, dtype=np.float32):
    """-> wi[n, 3], weight[n, 3], transmit[n] (bool)"""
    d, Ns, Ngf, base = (np.asarray(a, dtype).reshape(-1, 3) for a in (d, Ns, Ngf, base))
    n = d.shape[0]
    ior, r4 = (np.broadcast_to(np.asarray(a, dtype), (n,)) for a in (ior, r4))
    entering, thin = (np.broadcast_to(np.asarray(a).astype(bool), (n,)) for a in (entering, thin))
    one = dtype(1)
    eta = np.where(thin | entering, one / ior, ior).astype(dtype)
    N = np.where((_dot(-d, Ns) > 0)[..., None], Ns, Ngf)
    wi, tr, wrong, _ = _once(d, N, Ngf, eta, thin, r4)
    wi2, tr2, _, _ = _once(d, Ngf, Ngf, eta, thin, r4)
    wi = np.where(wrong[..., None], wi2, wi)
    tr = np.where(wrong, tr2, tr)
    weight = np.where(tr[..., None], base, one)
    return wi.astype(dtype), weight.astype(dtype), tr


# ------------------------------------------------------------------------------------------------ the float64 expectation
def rect(center, u, v, hu, hv, **kw):
    """a flat rectangle center +- hu u +- hv v; its normal is u x v (the OUTWARD normal of a solid's face).  kw: kind = 'thin' | 'solid' (glass: ior,
    base) | 'emitter' (Le; one-sided, emits and is hit on its normal's side only, SPEC §8) | 'black' (an opaque surface that reflects nothing)"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    r = dict(c=np.asarray(center, np.float64), u=u, v=v, hu=float(hu), hv=float(hv), n=np.cross(u, v), ior=1.5, base=(1.0, 1.0, 1.0), Le=0.0)
    r.update(kw)
    r["base"] = np.asarray(r["base"], np.float64)
    return r


def camera_rays(view, vfov, w, h, sub):
    """SPEC §11 in float64 from the column-major view matrix: origin, unit directions [h, w, len(sub)^2, 3] for sub-pixel offsets `sub` in x and y"""
    v = np.asarray(view, np.float64).reshape(4, 4)
    right, up, fwd, origin = v[0, :3], v[1, :3], v[2, :3], v[3, :3]
    th = np.tan(vfov / 2)
    jx, jy = np.meshgrid(sub, sub)
    x = np.arange(w)[None, :, None] + jx.reshape(-1)[None, None, :]
    y = np.arange(h)[:, None, None] + jy.reshape(-1)[None, None, :]
    cx = (2 * x / w - 1) * (w / h * th)
    cy = (1 - 2 * y / h) * th
    d = right * cx[..., None] + up * cy[..., None] + fwd
    return origin, d / np.linalg.norm(d, axis=-1, keepdims=True)


def _nearest(rects, o, d, last):
    n = o.shape[0]
    best_t, best_i = np.full(n, np.inf), np.full(n, -1)
    for i, r in enumerate(rects):
        dn = d @ r["n"]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((r["c"] - o) @ r["n"]) / dn
        P = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
        ok = np.isfinite(t) & (t > 1e-9) & (last != i) & (np.abs((P - r["c"]) @ r["u"]) <= r["hu"]) & (np.abs((P - r["c"]) @ r["v"]) <= r["hv"])
        if r["kind"] == "emitter":
            ok &= dn < 0
        ok &= t < best_t
        best_t, best_i = np.where(ok, t, best_t), np.where(ok, i, best_i)
    return best_t, best_i


def expectation_rays(rects, probe, o, d, depth):
    """for rays (o[n, 3], d[n, 3]) followed through both branches of every interface event, `depth` shaded hits at most:
    mean[n, 3], second moment[n, 3] of one sample's radiance, and P(the path ends without radiance: truncated at the depth limit, or absorbed)[n]"""
    n = o.shape[0]
    mean, m2 = np.zeros((n, 3)), np.zeros((n, 3))
    p_zero = np.zeros(n)
    probe = np.asarray(probe, np.float64)

    def leaf(idx, p, val):
        np.add.at(mean, idx, p[:, None] * val)
        np.add.at(m2, idx, p[:, None] * val * val)

    def go(idx, o, d, T, p, last, b):
        if idx.size == 0:
            return
        t, hit = _nearest(rects, o, d, last)
        miss = hit < 0
        if miss.any():
            leaf(idx[miss], p[miss], T[miss] * probe)
        for i, r in enumerate(rects):
            m = hit == i
            if not m.any():
                continue
            if r["kind"] == "emitter":
                leaf(idx[m], p[m], T[m] * r["Le"])
                continue
            if r["kind"] == "black" or b + 1 >= depth:   # absorbed; or an interface event on the last bounce: no next ray
                np.add.at(p_zero, idx[m], p[m])
                continue
            dm, Tm, pm, im = d[m], T[m], p[m], idx[m]
            P = o[m] + dm * t[m][:, None]
            flipped = dm @ r["n"] > 0
            Ngf = np.where(flipped[:, None], -r["n"], r["n"])
            thin = r["kind"] == "thin"
            eta = np.where(thin | ~flipped, 1.0 / r["ior"], r["ior"])
            c = np.minimum(_dot(-dm, Ngf), 1.0)
            Fr, ct = fresnel(c, eta)
            wr = dm + Ngf * (2.0 * c)[:, None]
            wt = dm if thin else dm * eta[:, None] + Ngf * (eta * c - ct)[:, None]
            wr, wt = wr / np.linalg.norm(wr, axis=1, keepdims=True), wt / np.maximum(np.linalg.norm(wt, axis=1, keepdims=True), 1e-300)
            li = np.full(im.size, i)
            a = Fr > 0
            go(im[a], P[a], wr[a], Tm[a], (pm * Fr)[a], li[a], b + 1)
            a = Fr < 1
            go(im[a], P[a], wt[a], (Tm * r["base"])[a], (pm * (1.0 - Fr))[a], li[a], b + 1)

    go(np.arange(n), np.asarray(o, np.float64), np.asarray(d, np.float64), np.ones((n, 3)), np.ones(n), np.full(n, -1), 0)
    return mean, m2, p_zero


def expectation(rects, probe, view, vfov, w, h, depth, grid, pixels=None):
    """per pixel (all, or the [k, 2] (y, x) list `pixels`), jitter integrated on a grid x grid sub-pixel grid of midpoints:
    mean[k, 3], per-sample variance[k, 3], P(sample is a truncated / absorbed path)[k]"""
    sub = (np.arange(grid) + 0.5) / grid
    origin, d = camera_rays(view, vfov, w, h, sub)
    if pixels is None:
        pixels = np.stack(np.meshgrid(np.arange(h), np.arange(w), indexing="ij"), -1).reshape(-1, 2)
    pixels = np.asarray(pixels)
    dd = d[pixels[:, 0], pixels[:, 1]].reshape(-1, 3)
    mean, m2, pz = expectation_rays(rects, probe, np.broadcast_to(origin, dd.shape), dd, depth)
    k, g2 = pixels.shape[0], grid * grid
    mean, m2, pz = mean.reshape(k, g2, 3).mean(1), m2.reshape(k, g2, 3).mean(1), pz.reshape(k, g2).mean(1)
    return mean, m2 - mean * mean, pz
