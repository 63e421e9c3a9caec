"""A numpy restatement of SPEC.md §24 (tangent-space normal maps), written from the SPEC text and not from the kernels (test infrastructure): §12's shading
normal up to its flip, the per-triangle frame from the uv derivatives, §9's linear lookup, the perturbed normal and the side rules.

One routine serves both precisions.  Fed binary64 arrays it is the reference; fed binary32 arrays every operation rounds to binary32 in the SPEC's order (numpy
does not contract), which is the restatement the decisions are compared with.  Every value carries a RUNNING ERROR BOUND (class R): an upper bound of
|binary32 result - reference value| built operation by operation from the standard model fl(x op y) = (x op y)(1 + e), |e| <= u = 2^-24 —
    x +- y : e_x + e_y + u |x +- y|          x y : (|x| e_y + |y| e_x + e_x e_y)(1 + u) + u |x y|
    1 / sqrt(x), two roundings (sqrt, then the reciprocal): 1 / sqrt(x - e_x) - 1 / sqrt(x) + (2 u + u^2) / sqrt(x - e_x), infinite where x - e_x <= 0
— so the bound of an output counts the roundings of its own expression, conditioning included (a nearly parallel tangent, a nearly cancelled normal).  Inputs (the
baked vertices, the barycentrics, the direction, the texel bytes, the scale) are binary32 numbers both sides read exactly: their bound is 0.  Underflow is not modelled:
the tests keep every intermediate far above 2^-126.  §9's lookup is continuous and piecewise bilinear, so a lookup position that is off by e texels moves a channel by at
most e times the steepest neighbour difference of that channel (the kernel may even sit in the neighbouring texel: the function is the same there); its own arithmetic
on non-negative terms is 2 roundings for the texel (the constant 1/255 and the product) and 9 for the taps (tests/test_gpu_emissive.py counts them): 12 u, three spare."""
import numpy as np

import emissive_ref as E
import primary_ref as P  # noqa: F401  (re-exported for the tests: camera rays, the normal word)

F = np.float32
U = 2.0 ** -24
K_LOOKUP = 12.0
INV255_F32 = F(0.003921568859368563)


class R:
    """a value (binary64: the reference; binary32: the restatement) with the running bound `e` of |binary32 result - reference value|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v)
        self.e = np.zeros(self.v.shape, np.float64) if e is None else np.asarray(e, np.float64)

    def _k(self, c):
        return c if isinstance(c, R) else R(np.asarray(c, self.v.dtype))

    def __add__(self, o):
        o = self._k(o)
        v = self.v + o.v
        return R(v, self.e + o.e + U * np.abs(v.astype(np.float64)))

    def __sub__(self, o):
        o = self._k(o)
        v = self.v - o.v
        return R(v, self.e + o.e + U * np.abs(v.astype(np.float64)))

    def __mul__(self, o):
        o = self._k(o)
        v = self.v * o.v
        a, b = np.abs(self.v.astype(np.float64)), np.abs(o.v.astype(np.float64))
        return R(v, (a * o.e + b * self.e + self.e * o.e) * (1 + U) + U * np.abs(v.astype(np.float64)))

    def __neg__(self):
        return R(-self.v, self.e)

    def rsqrt(self):
        """1 / sqrt(x) as the SPEC writes it: sqrt, then the reciprocal"""
        with np.errstate(all="ignore"):
            v = np.asarray(1, self.v.dtype) / np.sqrt(self.v)
            x = self.v.astype(np.float64)
            lo = x - self.e
            e = np.where(lo > 0, (1 + 2 * U + U * U) / np.sqrt(np.where(lo > 0, lo, 1.0)) - 1 / np.sqrt(np.where(lo > 0, x, 1.0)), np.inf)
        return R(v, e)


def sel(c, a, b):
    return R(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def vec(a, dtype):
    """(N, 3) exact inputs -> three R"""
    a = np.asarray(a, dtype)
    return tuple(R(a[..., k]) for k in range(3))


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def scale3(a, s):
    return tuple(c * s for c in a)


def sub3(a, b):
    return tuple(x - y for x, y in zip(a, b))


def add3(a, b):
    return tuple(x + y for x, y in zip(a, b))


def neg3(a):
    return tuple(-c for c in a)


def sel3(c, a, b):
    return tuple(sel(c, x, y) for x, y in zip(a, b))


def arr(a):
    return np.stack([c.v for c in a], -1)


def err(a):
    return np.stack([c.e for c in a], -1)


# ------------------------------------------------------------------ §9, linear: rgb through b·(1/255), never the sRGB table
def steepest(img):
    """per channel (3,), per axis: the largest difference between wrapped neighbours of b / 255"""
    lin = np.asarray(img, np.uint8)[..., :3].astype(np.float64) / 255.0
    return np.abs(np.roll(lin, -1, 1) - lin).reshape(-1, 3).max(0), np.abs(np.roll(lin, -1, 0) - lin).reshape(-1, 3).max(0)


def lookup_linear(img, tu, tv):
    """§9 at (tu, tv) (R, bounds included) -> three R"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    dt = tu.v.dtype
    fx, fy = tu * float(w) - 0.5, tv * float(h) - 0.5
    x0f, y0f = np.floor(fx.v), np.floor(fy.v)
    tx, ty = (fx.v - x0f)[:, None], (fy.v - y0f)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    lin = img[..., :3].astype(dt) * INV255_F32 if dt == np.float32 else img[..., :3].astype(np.float64) / 255.0
    one = np.asarray(1, dt)
    c00, c10 = lin[y0 % h, x0 % w], lin[y0 % h, (x0 + 1) % w]
    c01, c11 = lin[(y0 + 1) % h, x0 % w], lin[(y0 + 1) % h, (x0 + 1) % w]
    top, bot = c00 * (one - tx) + c10 * tx, c01 * (one - tx) + c11 * tx
    out = top * (one - ty) + bot * ty
    gx, gy = steepest(img)
    e = fx.e[:, None] * gx[None] + fy.e[:, None] * gy[None] + K_LOOKUP * U
    return tuple(R(out[:, k], e[:, k]) for k in range(3))


# ------------------------------------------------------------------ §12 up to the flip, then §24
def shading_normal(pos, nrm, uv, bary, d, image=None, scale=1.0, dtype=np.float64, e_uv=0.0):
    """N elements, each with its own baked triangle: pos (N, 3, 3), nrm (N, 3, 3), uv (N, 3, 2), bary (N, 2) = (u, v), d (N, 3) unit, all binary32 numbers;
    `image` an (h, w, 4) uint8 normal image or None (no map), `scale` a float or (N,).  e_uv: an extra bound on the interpolated (tu, tv), for a caller whose hit
    point is only known to within it.  -> a dict: Ns (N, 3) and its bound Ns_err, mapped (N,), flip (N,), Nv / Tp / Bp / Ngf, the texture coordinate, and `q`: the six
    deciding quantities {name: (value, bound)} — det, tl2, m2, bb = dot(Bp, B), side = dot(Nv, Ngf), under = dot(Ns, Ngf) — and §12's own geo = dot(Ng, d), on which
    Ngf and with it every side rule hangs.  Degenerate triangles (l2 = 0) are not
    meant: the tests have none."""
    dt = dtype
    pos, nrm, uv = np.asarray(pos, dt), np.asarray(nrm, dt), np.asarray(uv, dt)
    n = pos.shape[0]
    hu, hv = R(np.asarray(bary, dt)[:, 0]), R(np.asarray(bary, dt)[:, 1])
    dd = vec(d, dt)
    p0, p1, p2 = (vec(pos[:, k], dt) for k in range(3))
    n0, n1, n2 = (vec(nrm[:, k], dt) for k in range(3))
    with np.errstate(all="ignore"):
        bw = (R(np.ones(n, dt)) - hu) - hv
        e1, e2 = sub3(p1, p0), sub3(p2, p0)
        Ng = cross(e1, e2)
        Ng = scale3(Ng, dot(Ng, Ng).rsqrt())
        Nv = tuple((a * bw + b * hu) + c * hv for a, b, c in zip(n0, n1, n2))
        n2_ = dot(Nv, Nv)
        Nv = sel3(n2_.v > 0, scale3(Nv, n2_.rsqrt()), Ng)
        gd = dot(Ng, dd)
        Ngf = sel3(gd.v > 0, neg3(Ng), Ng)
        side = dot(Nv, Ngf)
        flip = side.v < 0
        Ns_plain = sel3(flip, neg3(Nv), Nv)
        tu = (R(uv[:, 0, 0]) * bw + R(uv[:, 1, 0]) * hu) + R(uv[:, 2, 0]) * hv
        tv = (R(uv[:, 0, 1]) * bw + R(uv[:, 1, 1]) * hu) + R(uv[:, 2, 1]) * hv
        tu, tv = R(tu.v, tu.e + e_uv), R(tv.v, tv.e + e_uv)
        out = {"Nv": arr(Nv), "Ngf": arr(Ngf), "flip": flip, "tu": tu.v, "tv": tv.v, "plain": arr(Ns_plain), "plain_err": err(Ns_plain), "q": {"geo": (gd.v, gd.e), "side": (side.v, side.e)}}
        if image is None:
            out.update(Ns=arr(Ns_plain), Ns_err=err(Ns_plain), mapped=np.zeros(n, bool))
            return out
        du1, dv1 = R(uv[:, 1, 0]) - R(uv[:, 0, 0]), R(uv[:, 1, 1]) - R(uv[:, 0, 1])
        du2, dv2 = R(uv[:, 2, 0]) - R(uv[:, 0, 0]), R(uv[:, 2, 1]) - R(uv[:, 0, 1])
        det = du1 * dv2 - du2 * dv1
        ok = (det.v != 0) & np.isfinite(det.v)
        sg = R(np.where(det.v < 0, -1, 1).astype(dt))
        T = scale3(sub3(scale3(e1, dv2), scale3(e2, dv1)), sg)
        B = scale3(sub3(scale3(e2, du1), scale3(e1, du2)), sg)
        Tp = sub3(T, scale3(Nv, dot(Nv, T)))
        tl2 = dot(Tp, Tp)
        ok_t = tl2.v > 0
        Tp = scale3(Tp, tl2.rsqrt())
        Bp = cross(Nv, Tp)
        bb = dot(Bp, B)
        Bp = sel3(bb.v < 0, neg3(Bp), Bp)
        tex = lookup_linear(image, tu, tv)
        sc = R(np.broadcast_to(np.asarray(scale, dt), (n,)))
        nx, ny, nz = (tex[0] * 2.0 - 1.0) * sc, (tex[1] * 2.0 - 1.0) * sc, tex[2] * 2.0 - 1.0
        Nm = add3(add3(scale3(Tp, nx), scale3(Bp, ny)), scale3(Nv, nz))
        m2 = dot(Nm, Nm)
        ok_m = m2.v > 0
        Nm = scale3(Nm, m2.rsqrt())
        Nm = sel3(flip, neg3(Nm), Nm)
        under = dot(Nm, Ngf)
        ok_u = under.v > 0
        mapped = ok & ok_t & ok_m & ok_u
        Ns = sel3(mapped, Nm, Ns_plain)
    out.update(Ns=arr(Ns), Ns_err=err(Ns), mapped=mapped, Tp=arr(Tp), Bp=arr(Bp), n=np.stack([nx.v, ny.v, nz.v], -1), reached={"det": np.ones(n, bool), "tl2": ok, "bb": ok & ok_t,
               "m2": ok & ok_t, "under": ok & ok_t & ok_m, "side": np.ones(n, bool), "geo": np.ones(n, bool)})
    out["q"].update(det=(det.v, det.e), tl2=(tl2.v, tl2.e), bb=(bb.v, bb.e), m2=(m2.v, m2.e), under=(under.v, under.e))
    return out


def undecided(ref):
    """(N,) the elements one of whose REACHED decisions the reference cannot call: the deciding quantity lies within its derived bound of its threshold 0.  A bound of
    exactly 0 means the binary32 value IS the reference's (all-equal uv give det = 0 in both), so that decision is certain whatever the value."""
    n = ref["flip"].shape[0]
    u = np.zeros(n, bool)
    reached = ref.get("reached", {"side": np.ones(n, bool), "geo": np.ones(n, bool)})
    for k, (v, e) in ref["q"].items():
        u |= reached[k] & (e > 0) & ~(np.abs(v.astype(np.float64)) > e)
    return u
