"""SPEC.md §28 restated in numpy, from the section alone (no kernel source was consulted for the arithmetic).

`sigma` is the host's derivation of the absorption coefficient (binary64, rounded once to binary32, capped at FLT_MAX).  `atten` is the factor A(sigma, t) in
§28's operation order: with float32 arrays every operation is one binary32 rounding (numpy's float32 multiply, add, subtract and floor are correctly rounded
and numpy contracts nothing), so it is what the device hook must return bit for bit.

THE ROUNDING MODEL of `atten` against binary64 exp(-sigma t), first order in u = 2^-24 (the largest relative error of one binary32 rounding), x = sigma t:
  * the argument.  x = fl(sigma t) and y = fl(x L) are two roundings, and L = 1.44269502f is log2 e off by 0.22 u relative: y is within 2.3 u relative of
    x log2 e.  An error dy of y is a relative error ln 2 dy of 2^-y, here ln 2 * y * 2.3 u = 2.3 x u: the term that grows with x, taken as 3 x u.
    f = y - k is exact (k = floor(y + 0.5) is within 0.5 of y, so the difference has no bit below y's last).
  * g = fl(f * 0.693147182f): one rounding and ln 2 off by 0.05 u, on |g| <= 0.347 only: a relative error of the result of at most 0.347 * 1.05 u < 0.4 u.
  * the Horner chain: 7 multiplications and 7 additions, 14 roundings, each of at most u times an intermediate of magnitude <= exp(0.347) = 1.42, over a result
    >= exp(-0.347) = 0.707: 2.01 u each where it enters the result whole.  The two roundings made j steps before the end enter it times |g|^j, so the chain
    gives at most 2.01 u * 2 (1 + 0.347 + 0.347^2 + ...) = 2.01 u * 3.07 < 6.2 u.  The coefficients c_0, c_1, c_2 are exact, the others add < 0.01 u.
  * the series cut behind g^7: g^8 / 8! <= 5.2e-9 absolute on a result >= 0.707: 0.12 u.
  * the last product, by an exact power of two, is exact: p is in [0.707, 1.42] and the exponent is at least 2 - 127, so the result is a normal number.
  Sum: 3 x u + (0.4 + 6.2 + 0.01 + 0.12) u < (3 x + 8) u.  `bound(x)` is that.  tests/test_volume.py prints the largest fraction of it in use (0.60 on 4 * 10^6
  log-uniform pairs when the section was written).
A = 0 from y >= 125 on (x >= 86.6): exp(-x) < 2^-124.9 there and the bound is not claimed; below, every result is 0 or a normal number.

`expectation_rays` is transmission_ref.expectation_rays with ONE addition: at a hit of a `kind == "solid"` rectangle that carries a `sigma` and is hit from
behind (`flipped`), T is first multiplied by exp(-sigma t) in binary64."""
import numpy as np

from transmission_ref import camera_rays, fresnel, rect, _dot, _nearest      # noqa: F401  (re-exported for the tests)

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
U = 2.0 ** -24
LOG2E, LN2 = F32(1.44269502), F32(0.693147182)
COEF = [F32((-1.0) ** n / float(np.prod(np.arange(1, n + 1, dtype=np.float64)))) for n in range(8)]      # (float)((-1)^n / n!)


def sigma(c, D):
    """the absorption coefficient per channel: c in [0, 1] (float32), D > 0 (float32, +inf: none) -> float32, finite, >= +0"""
    c, D = np.broadcast_arrays(np.asarray(c, F32), np.asarray(D, F32))
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        q = (-np.log(c.astype(np.float64)) / D.astype(np.float64)).astype(F32)
    q = np.where(q < FLT_MAX, q, FLT_MAX).astype(F32)
    return np.where((c == 1) | np.isinf(D), F32(0), q).astype(F32)


def atten(s, t):
    """A(sigma, t) of §28 in float32, elementwise"""
    s, t = np.broadcast_arrays(np.asarray(s, F32), np.asarray(t, F32))
    with np.errstate(all="ignore"):
        x = s * t
        y = x * LOG2E
        ok = y < F32(125.0)                      # False for +inf and NaN too
        y = np.where(ok, y, F32(0))
        k = np.floor(y + F32(0.5))
        f = y - k
        g = f * LN2
        p = np.full(g.shape, COEF[7], F32)
        for c in COEF[6::-1]:
            p = (p * g) + c
        scale = ((127 - k.astype(np.int32)) << 23).astype(np.uint32).view(F32)
        return np.where(ok, p * scale, F32(0)).astype(F32)


def bound(x):
    """the rounding model's bound on |atten - exp(-x)| / exp(-x), x = sigma t in binary64"""
    return (3.0 * np.asarray(x, np.float64) + 8.0) * U


def slab_chord(o, d, lo, hi):
    """binary64 slab method: (t_enter, t_exit) of rays o + t d against the box [lo, hi]; rays that miss have t_enter > t_exit"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (np.asarray(lo, np.float64) - o) / d, (np.asarray(hi, np.float64) - o) / d
    return np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)


def expectation_rays(rects, probe, o, d, depth):
    """transmission_ref.expectation_rays, with the volume attenuation of §28 at the hits where it applies"""
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
            if r["kind"] == "black" or b + 1 >= depth:
                np.add.at(p_zero, idx[m], p[m])
                continue
            dm, Tm, pm, im = d[m], T[m], p[m], idx[m]
            P = o[m] + dm * t[m][:, None]
            flipped = dm @ r["n"] > 0
            if r["kind"] == "solid" and r.get("sigma") is not None:      # §28: the segment that ends on the solid's own back face
                A = np.exp(-np.asarray(r["sigma"], np.float64)[None, :] * t[m][:, None])
                Tm = np.where(flipped[:, None], Tm * A, Tm)
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
    """transmission_ref.expectation over `expectation_rays` above: mean[k, 3], per-sample variance[k, 3], P(truncated / absorbed)[k]"""
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
