"""SPEC §10 in binary64, written from the SPEC's formulas: the surface, the lobe pick, f and pdf, the sampled direction for given draws and the
directional albedo; the first-order error model both implementations (the oracle's bsdf_* and the device's, through lpt_bsdf_probe) are held to;
and the set of inputs, edges first, on which they are held to it.  Nothing here is written in either implementation's operation order except
`tolerance`, whose whole point is that order.

A ROW is the hook's: {base[3], roughness, metallic, N[3], Ng[3], V[3], L[3], r3, r4, r5}, 20 binary32 numbers; an OUTPUT is {pspec, f[3], pdf,
L_s[3], weight[3], pdf_s} and `ok`.  The reference reads the same binary32 inputs (it does not re-normalise a direction: the SPEC's dots take them as
they are), with exact sin / cos and `onb`'s formulas without rounding.

THE ERROR MODEL (`tolerance`; nothing in it is tuned on an output).  Every binary32 operation of SPEC §10, in the SPEC's order and parenthesisation, is
one relative rounding u = 2^-24 of its own result; a decimal constant (0.045, 0.04, the lum weights, pi, 1/pi, 0.1, 0.9, 1e-4) is one more.  The
roundings are carried forward through the float64 partial derivatives of each operation (|a| db + |b| da for a product, (da + |q| db) / (|b| - db) for
a quotient, the exact interval for a square root, nothing for max / clamp, which are 1-Lipschitz), worst case = the sum, times 2 for the second-order
terms.  Counted along one output's chain, for one channel:
  alpha 3 (the clamp constant, r r), a2 5; diff 2; F0 5; NoV 5 (three products, two sums) of sum|N_i V_i|;
  pspec: (1 - NoV)^5 4, Fv 4 more per channel, lum 8, wd 10 more, ws / (ws + wd) 2, the clamp 1: about 45, all of well-conditioned positive sums but
    1 - NoV and 1 - ws, whose absolute errors the model carries as such;
  eval: NoL 5; V + L 1, |V + L|^2 5, sqrt 1, 1 / 1, H 1: NoH and VoH 5 + 9 each, absolute (about 14 u of a number <= 1); dd = NoH^2 (a2 - 1) + 1: 4 of
    its own, absolute, plus 2 NoH dNoH — about 30 u ABSOLUTE against dd >= a2, which is the whole of the pdf's error at small roughness
    (a2 = 4.1e-6: d dd / dd <= 0.45, D carries twice that); D 4 more; vis 9; F 5 + VoH's; f = (diff / pi)(1 - F) + (D vis) F 7 more: about 60 + D's;
    pdf = pspec D NoH / (4 VoH) + (1 - pspec) NoL / pi: 8 more and pspec's.
  sample: onb 7 per component; sincos2pi is not counted in roundings: its sine and cosine are taken as exact ones off by 5e-6 absolute, the bound
    tests/test_oracle_kat.py pins; cos^2 6 (absolute where 1 + (a2 - 1) r4 cancels), the two roots 2, H 9 per component, 2 V.H 6, L 2, normalize 9:
    L_s about 45 + the sincos term; weight and pdf_s are eval's at L_s with L_s's error carried in through NoL, NoH and VoH, and NoL / pdf 1, f w 1.
D's error is common to f and pdf, so it is carried as ONE signed term through f, pdf and weight = f NoL / pdf, where it largely cancels (a specular
sample's weight is vis F 4 VoH NoL / (pspec NoH) whatever D is); everything else is taken as independent.  A quotient whose divisor's error reaches the
divisor, and a square root or a normalisation of a number its error reaches, have no bound: the output's tolerance is infinite there and the
element is counted with the ones left out.  Branches: where float64 puts NoL, dot(Ng, L) or VoH (or, for pspec = 1, NoH of the sample) within its own
tolerance of zero the two sides may fall on different sides of the gate; where they did, the element is left out of that comparison (`check` reports the
share).  The lobe pick r3 < pspec is not left
out: `check` takes the lobe from the implementation's own binary32 pspec, which it holds to the reference by itself.  pdf_s and weight are held to the
reference AT THE DIRECTION THE IMPLEMENTATION RETURNED, which is what SPEC §10 makes them; L_s is held to the reference's direction."""
import numpy as np

U = 2.0 ** -24
SINCOS_ABS = 5e-6          # tests/test_oracle_kat.py: |sincos2pi - sin, cos| < 5e-6
ONE_M = np.float32(1.0 - U)
F32_MIN_ROUGH = float(np.float32(0.045))
OUT = ("pspec", "f", "pdf", "L_s", "weight", "pdf_s")
OUT_COLS = {"pspec": slice(0, 1), "f": slice(1, 4), "pdf": slice(4, 5), "L_s": slice(5, 8), "weight": slice(8, 11), "pdf_s": slice(11, 12)}
MUTATIONS = ("k_alpha2", "diffuse_without_1mF", "pdf_s_swapped", "cosine_r4")
LUM = np.array([0.2126, 0.7152, 0.0722])


def _dot(a, b):
    return np.sum(a * b, axis=-1)


# ------------------------------------------------------------------------------------------------ the reference
def surface(base, rough, metal):
    r = np.clip(rough, 0.045, 1.0)
    m = np.clip(metal, 0.0, 1.0)[..., None]
    alpha = r * r
    return {"diff": base * (1.0 - m), "f0": 0.04 * (1.0 - m) + base * m, "alpha": alpha, "a2": alpha * alpha}


def fresnel(f0, c):
    return f0 + (1.0 - f0) * ((1.0 - c) ** 5)[..., None]


def spec_probability(s, NoV):
    ws = fresnel(s["f0"], NoV) @ LUM
    wd = (s["diff"] @ LUM) * (1.0 - ws)
    with np.errstate(all="ignore"):
        p = np.clip(ws / (ws + wd), 0.1, 0.9)
    return np.where(wd > 0.0, p, 1.0)


def onb(N):
    sign = np.copysign(1.0, N[..., 2])
    a = -1.0 / (sign + N[..., 2])
    b = N[..., 0] * N[..., 1] * a
    T = np.stack([1.0 + sign * N[..., 0] * N[..., 0] * a, sign * b, -sign * N[..., 0]], -1)
    B = np.stack([b, sign + N[..., 1] * N[..., 1] * a, -N[..., 1]], -1)
    return T, B


def _unit(v):
    l = np.sqrt(_dot(v, v))[..., None]
    with np.errstate(all="ignore"):
        return np.where(l > 0.0, v / l, 0.0)


def evaluate(s, N, Ng, V, NoV, pspec, L, mutate=None):
    """f[..., 3] and pdf of SPEC §10 at L"""
    NoL = _dot(N, L)
    H = _unit(V + L)
    NoH, VoH = np.maximum(_dot(N, H), 0.0), np.maximum(_dot(V, H), 0.0)
    gate = (NoL > 0.0) & (_dot(Ng, L) > 0.0) & (VoH > 0.0)
    a2, alpha = s["a2"], s["alpha"]
    D = a2 / (np.pi * (NoH * NoH * (a2 - 1.0) + 1.0) ** 2)
    k = alpha * alpha / 2.0 if mutate == "k_alpha2" else alpha / 2.0
    with np.errstate(all="ignore"):
        vis = 1.0 / (4.0 * (NoL * (1.0 - k) + k) * (NoV * (1.0 - k) + k))
        F = fresnel(s["f0"], VoH)
        f = s["diff"] / np.pi * (1.0 if mutate == "diffuse_without_1mF" else (1.0 - F)) + (D * vis)[..., None] * F
        a, b = (VoH, NoH) if mutate == "pdf_s_swapped" else (NoH, VoH)
        pdf_s = np.where(b > 0.0, D * a / (4.0 * b), 0.0)
        pdf = pspec * pdf_s + (1.0 - pspec) * NoL / np.pi
    return np.where(gate[..., None], f, 0.0), np.where(gate, pdf, 0.0)


def sample_direction(s, N, V, spec, r4, r5, mutate=None):
    """the direction for the draws (r4, r5): GGX half vector and mirror where `spec`, else the cosine lobe"""
    T, B = onb(N)
    sn, cs = np.sin(2.0 * np.pi * r5), np.cos(2.0 * np.pi * r5)
    cos2 = (1.0 - r4) / (1.0 + (s["a2"] - 1.0) * r4)
    ct, st = np.sqrt(cos2), np.sqrt(np.maximum(0.0, 1.0 - cos2))
    H = T * (st * cs)[..., None] + B * (st * sn)[..., None] + N * ct[..., None]
    Ls = 2.0 * _dot(V, H)[..., None] * H - V
    r = r4 if mutate == "cosine_r4" else np.sqrt(r4)
    Ld = T * (r * cs)[..., None] + B * (r * sn)[..., None] + N * np.sqrt(np.maximum(0.0, 1.0 - r4))[..., None]
    return _unit(np.where(spec[..., None], Ls, Ld))


def split(rows):
    x = np.asarray(rows, np.float32).reshape(-1, 20).astype(np.float64)
    return {"base": x[:, 0:3], "rough": x[:, 3], "metal": x[:, 4], "N": x[:, 5:8], "Ng": x[:, 8:11], "V": x[:, 11:14], "L": x[:, 14:17],
            "r3": x[:, 17], "r4": x[:, 18], "r5": x[:, 19]}


def _setup(rows):
    """what a surface hit sets up before it evaluates or samples: the row's fields, the surface, the clamped NoV and the lobe pick's pspec"""
    q = split(rows)
    s = surface(q["base"], q["rough"], q["metal"])
    NoV = np.maximum(_dot(q["N"], q["V"]), 1e-4)
    return q, s, NoV, spec_probability(s, NoV)


def reference_at(rows, L, mutate=None):
    """f[n, 3], pdf[n] and f (N.L) / pdf [n, 3] (0 where pdf = 0) of direction L[n, 3] at the surface and view of each row, in binary64"""
    q, s, NoV, pspec = _setup(rows)
    L = np.asarray(L, np.float64)
    f, pdf = evaluate(s, q["N"], q["Ng"], q["V"], NoV, pspec, L, mutate)
    with np.errstate(all="ignore"):
        w = np.where((pdf > 0.0)[:, None], f * (_dot(q["N"], L) / pdf)[:, None], 0.0)
    return f, pdf, w


def pdf64(rows, L):
    """the float64 pdf of direction L[n, 3] at the surface and view of each row"""
    return reference_at(rows, L)[1]


def reference(rows, mutate=None, spec=None):
    """the hook in binary64 -> (out[n, 12], ok[n]); `mutate` names one of MUTATIONS, a deliberately wrong variant for the checker's own test; `spec`
    (bool[n]) overrides the lobe pick r3 < pspec — the checker passes the pick that follows from the implementation's own binary32 pspec, which it
    holds to the reference separately, so that r3 AT pspec is a tested case and not an undecidable one"""
    q, s, _, pspec = _setup(rows)
    f, pdf, _ = reference_at(rows, q["L"], mutate)
    Ls = sample_direction(s, q["N"], q["V"], q["r3"] < pspec if spec is None else spec, q["r4"], q["r5"], mutate)
    _, ps, w = reference_at(rows, Ls, mutate)
    ok = ps > 0.0
    out = np.concatenate([pspec[:, None], f, pdf[:, None], np.where(ok[:, None], Ls, 0.0), w, ps[:, None]], axis=1)
    return out, ok


# ------------------------------------------------------------------------------------------------ the directional albedo
def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def directional_albedo(base, rough, metal, N, Ng, V, n_u=1536, n_phi=1536):
    """a(V) = int f(V, L) (N.L) dL over N.L > 0, Ng.L > 0.  The specular term is integrated over the half vector in the variables of its own
    sampling, (u, phi) with cos^2 = (1 - u) / (1 + (a2 - 1) u): dL = 4 VoH dH and D NoH dH = du dphi / (2 pi), so the integrand is
    vis F NoL 4 VoH / NoH — no D, smooth however narrow the lobe.  The diffuse term is integrated in (cos^2 theta, phi) about N.  Gauss-Legendre
    in the first variable, the midpoint rule (periodic) in phi."""
    base, N, Ng, V = (np.asarray(a, np.float64) for a in (base, N, Ng, V))
    N, Ng, V = N / np.linalg.norm(N), Ng / np.linalg.norm(Ng), V / np.linalg.norm(V)
    s = surface(base[None], np.array([float(rough)]), np.array([float(metal)]))
    NoV = max(float(N @ V), 1e-4)
    T, B = onb(N[None])
    phi = (np.arange(n_phi) + 0.5) / n_phi * 2.0 * np.pi
    ring = T * np.cos(phi)[:, None] + B * np.sin(phi)[:, None]       # [n_phi, 3]
    xs, ws = _gauss(n_u)
    a2, k = s["a2"][0], s["alpha"][0] / 2.0
    total = np.zeros(3)
    for u, w in zip(xs, ws):
        # specular: one ring of half vectors
        cos2 = (1.0 - u) / (1.0 + (a2 - 1.0) * u)
        H = ring * np.sqrt(1.0 - cos2) + N * np.sqrt(cos2)
        VoH = H @ V
        L = 2.0 * VoH[:, None] * H - V
        NoL = L @ N
        g = (NoL > 0.0) & (L @ Ng > 0.0) & (VoH > 0.0)
        vis = 1.0 / (4.0 * (np.where(g, NoL, 1.0) * (1.0 - k) + k) * (NoV * (1.0 - k) + k))
        spec = np.where(g, vis * NoL * 4.0 * VoH / np.sqrt(cos2), 0.0)[:, None] * fresnel(s["f0"], np.clip(VoH, 0.0, 1.0))
        # diffuse: one ring of directions at cos^2 theta = u, dL = d(cos^2) dphi / (2 cos): (N.L) dL = du dphi / 2
        L = ring * np.sqrt(1.0 - u) + N * np.sqrt(u)
        Hd = _unit(V + L)
        dif = np.where(L @ Ng > 0.0, 0.5, 0.0)[:, None] * (s["diff"] / np.pi) * (1.0 - fresnel(s["f0"], np.maximum(Hd @ V, 0.0)))
        total += w * (spec.sum(axis=0) / n_phi + dif.sum(axis=0) * (2.0 * np.pi / n_phi))
    return total


def octant_cosine_integrals(N, Ng, n_phi=4096):
    """int (N.L) dL over N.L > 0, Ng.L > 0 and the k-th octant of the azimuth about N (onb's frame), k = 0..7; their sum is pi (1 + cos gamma) / 2.
    Exact in theta: at azimuth phi the gate cuts the polar angle at tan(theta) < -(N.Ng) / (Ng.e(phi)) where Ng.e(phi) < 0, and
    int_0^t cos sin = sin^2(t) / 2; midpoint rule in phi."""
    N, Ng = np.asarray(N, np.float64) / np.linalg.norm(N), np.asarray(Ng, np.float64) / np.linalg.norm(Ng)
    T, B = onb(N[None])
    out = np.zeros(8)
    for k in range(8):
        phi = (k + (np.arange(n_phi) + 0.5) / n_phi) * (np.pi / 4.0)
        c = (T * np.cos(phi)[:, None] + B * np.sin(phi)[:, None]) @ Ng
        cg = float(N @ Ng)
        with np.errstate(all="ignore"):
            t2 = np.where(c < 0.0, (cg / -c) ** 2, np.inf)       # tan^2 of the cut
            s2 = np.where(np.isinf(t2), 1.0, t2 / (1.0 + t2))
        out[k] = np.sum(0.5 * s2) * (np.pi / 4.0 / n_phi)
    return out


# ------------------------------------------------------------------------------------------------ the error model
class E:
    """a float64 value, a bound on its absolute binary32 error, and the signed coefficient of the one shared relative error (D's)"""
    __slots__ = ("v", "e", "g")

    def __init__(self, v, e=0.0, g=0.0):
        self.v, self.e, self.g = np.asarray(v, np.float64), e, g


def _rnd(v, e, g):
    return E(v, e + U * np.abs(v), g)


def _c(x):            # a decimal constant, rounded once to binary32
    return E(x, U * abs(x))


def _add(a, b):
    return _rnd(a.v + b.v, a.e + b.e, a.g + b.g)


def _sub(a, b):
    return _rnd(a.v - b.v, a.e + b.e, a.g - b.g)


def _mul(a, b):        # with the second-order term: (1 - VoH)^5 and its like are products of numbers smaller than their own errors
    return _rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e, a.v * b.g + b.v * a.g)


def _div(a, b):
    den = np.abs(b.v) - b.e
    q = a.v / b.v
    return _rnd(q, np.where(den > 0.0, (a.e + np.abs(q) * b.e) / np.where(den > 0.0, den, 1.0), np.inf), (a.g - q * b.g) / b.v)


def _sqrt(a):
    v = np.sqrt(a.v)
    return _rnd(v, np.maximum(np.sqrt(a.v + a.e) - v, v - np.sqrt(np.maximum(a.v - a.e, 0.0))), a.g / np.where(v > 0.0, 2.0 * v, 1.0))


def _max(a, c):       # 1-Lipschitz: the error does not grow; the constant's own rounding where it is taken
    return E(np.maximum(a.v, c), a.e + U * abs(c), np.where(a.v > c, a.g, 0.0))


def _sel(m, a, b):
    return E(np.where(m, a.v, b.v), np.where(m, a.e, b.e), np.where(m, a.g, b.g))


ONE, ZERO = E(1.0), E(0.0)


def _edot(a, b):
    return _add(_add(_mul(a[0], b[0]), _mul(a[1], b[1])), _mul(a[2], b[2]))


def _enormalize(a):
    l2 = _edot(a, a)
    inv = _div(ONE, _sqrt(l2))
    zero = l2.v == 0.0
    lost = (~zero) & (l2.v <= l2.e)          # the length is within its own error of 0: no bound
    out = []
    for c in a:
        r = _mul(c, inv)
        out.append(E(np.where(zero, 0.0, r.v), np.where(zero, 0.0, np.where(lost, np.inf, r.e)), np.where(zero, 0.0, r.g)))
    return out


def _epow5(m):
    m2 = _mul(m, m)
    return _mul(_mul(m2, m2), m)


def _efresnel(f0, fc):
    return [_add(c, _mul(_sub(ONE, c), fc)) for c in f0]


def _elum(c):
    return _add(_add(_mul(_c(0.2126), c[0]), _mul(_c(0.7152), c[1])), _mul(_c(0.0722), c[2]))


def _eeval(s, N, Ng, V, NoV, pspec, L):
    """-> f[3], pdf, weight[3] = f (N.L / pdf) with D's error moved into the shared term (E.g, against the returned eps); float64's gate; `near`: it cannot
    call the gate (NoL, dot(Ng, L) or VoH within tolerance of zero); `near_ok`: nor whether pdf > 0 (the same, and for pspec = 1 NoH)"""
    NoL, NgL = _edot(N, L), _edot(Ng, L)
    H = _enormalize([_add(V[i], L[i]) for i in range(3)])
    NoH_raw, VoH = _edot(N, H), _edot(V, H)
    NoH = _max(NoH_raw, 0.0)
    dd = _add(_mul(_mul(NoH, NoH), _sub(s["a2"], ONE)), ONE)
    D = _div(s["a2"], _mul(_c(np.pi), _mul(dd, dd)))
    eps = D.e / np.abs(D.v)
    D = E(D.v, 0.0, D.v)
    k = _mul(s["alpha"], E(0.5))
    omk = _sub(ONE, k)
    gl, gv = _add(_mul(NoL, omk), k), _add(_mul(NoV, omk), k)
    vis = _div(ONE, _mul(E(4.0), _mul(gl, gv)))
    F = _efresnel(s["f0"], _epow5(_sub(ONE, VoH)))
    dv = _mul(D, vis)
    f = [_add(_mul(_mul(s["diff"][i], _c(1.0 / np.pi)), _sub(ONE, F[i])), _mul(dv, F[i])) for i in range(3)]
    pdf_d = _mul(NoL, _c(1.0 / np.pi))
    pdf_s = _div(_mul(D, NoH), _mul(E(4.0), VoH))
    pdf = _add(_mul(pspec, pdf_s), _mul(_sub(ONE, pspec), pdf_d))
    w = _div(NoL, pdf)
    gate = (NoL.v > 0.0) & (NgL.v > 0.0) & (VoH.v > 0.0)
    shut = (NoL.v < -2.0 * NoL.e) | (NgL.v < -2.0 * NgL.e) | (VoH.v < -2.0 * VoH.e)          # clearly shut, whatever the rest
    near = ~shut & (_near(NoL) | _near(NgL) | _near(VoH) | ~np.isfinite(VoH.e))
    near_ok = near | (~shut & (pspec.v == 1.0) & _near(NoH_raw))
    return f, pdf, [_mul(c, w) for c in f], eps, gate, near, near_ok


def _bound(x, eps):
    with np.errstate(all="ignore"):
        t = 2.0 * (x.e + np.abs(x.g) * eps) + 1e-44
    return np.where(np.isnan(t), np.inf, t)


def _near(x):
    """float64 puts x within its own tolerance of zero (an exact zero with no error is not near: both sides compute it exactly)"""
    return (np.abs(x.v) <= 2.0 * x.e) & ~((x.v == 0.0) & (x.e == 0.0))


def tolerance(rows, spec=None, sample=True):
    """-> (tol, aux).  tol[name][n, k]: the absolute tolerance (inf: no bound) of pspec, f, pdf, of "w_at_L" = f (N.L) / pdf at the row's L, and (with
    `sample`) of the sampled direction "L_s", which is given whether or not the sample survives the gate.  aux: "gate"[n] float64's gate at L,
    "near_eval"[n] the elements whose gate at L float64 cannot call (NoL, dot(Ng, L) or VoH within tolerance of zero), "L_s"[n, 3] the direction,
    "ok"[n] and "near_sample"[n] the same for the sample, and "values" the outputs in SPEC order (tests/test_bsdf_reference.py holds them to
    `reference`).  `spec`: see `reference`."""
    q = split(rows)
    with np.errstate(all="ignore"):
        return _tolerance(q, spec, sample)


def _tolerance(q, spec, sample):
    ex = lambda a: [E(a[:, i]) for i in range(3)]
    base, N, Ng, V, L = (ex(q[k]) for k in ("base", "N", "Ng", "V", "L"))
    rough = q["rough"]
    r = E(np.clip(rough, 0.045, 1.0), np.where(rough <= F32_MIN_ROUGH, U * 0.045, 0.0))
    m = E(np.clip(q["metal"], 0.0, 1.0))
    alpha = _mul(r, r)
    om = _sub(ONE, m)
    s = {"alpha": alpha, "a2": _mul(alpha, alpha), "diff": [_mul(b, om) for b in base], "f0": [_add(_mul(_c(0.04), om), _mul(b, m)) for b in base]}
    NoV = _max(_edot(N, V), 1e-4)
    # the lobe pick
    ws = _elum(_efresnel(s["f0"], _epow5(_sub(ONE, NoV))))
    wd = _mul(_elum(s["diff"]), _sub(ONE, ws))
    p = _div(ws, _add(ws, wd))
    p = E(np.clip(p.v, 0.1, 0.9), p.e + U, p.g)
    pspec = _sel(wd.v > 0.0, p, ONE)
    pspec_lost = _near(wd)
    zero3 = lambda m_, t: np.where(m_[:, None], t, 0.0)
    stack = lambda xs, e_: np.stack([_bound(x, e_) for x in xs], axis=1)
    vals3 = lambda xs: np.stack([c.v for c in xs], 1)
    # eval at L
    f, pdf, w, eps, gate, near, _ = _eeval(s, N, Ng, V, NoV, pspec, L)
    tol = {"pspec": np.where(pspec_lost, np.inf, _bound(pspec, 0.0))[:, None],
           "f": zero3(gate, stack(f, eps)), "pdf": zero3(gate, stack([pdf], eps)), "w_at_L": zero3(gate, stack(w, eps))}
    aux = {"gate": gate, "near_eval": near | pspec_lost,
           "values": np.concatenate([pspec.v[:, None], zero3(gate, vals3(f)), np.where(gate, pdf.v, 0.0)[:, None], zero3(gate, vals3(w))], axis=1)}
    if not sample:
        return tol, aux
    sign = E(np.copysign(1.0, q["N"][:, 2]))
    a = _div(E(-1.0), _add(sign, N[2]))
    bb = _mul(_mul(N[0], N[1]), a)
    T = [_add(ONE, _mul(_mul(_mul(sign, N[0]), N[0]), a)), _mul(sign, bb), E(-sign.v * N[0].v)]
    B = [bb, _add(sign, _mul(_mul(N[1], N[1]), a)), E(-N[1].v)]
    sn, cs = E(np.sin(2.0 * np.pi * q["r5"]), SINCOS_ABS), E(np.cos(2.0 * np.pi * q["r5"]), SINCOS_ABS)
    r4 = E(q["r4"])
    cos2 = _div(_sub(ONE, r4), _add(ONE, _mul(_sub(s["a2"], ONE), r4)))
    ct, st = _sqrt(cos2), _sqrt(_max(_sub(ONE, cos2), 0.0))
    hx, hy = _mul(st, cs), _mul(st, sn)
    H = [_add(_add(_mul(T[i], hx), _mul(B[i], hy)), _mul(N[i], ct)) for i in range(3)]
    vh2 = _mul(E(2.0), _edot(V, H))
    Lspec = [_sub(_mul(vh2, H[i]), V[i]) for i in range(3)]
    rr = _sqrt(r4)
    lx, ly, lz = _mul(rr, cs), _mul(rr, sn), _sqrt(_max(_sub(ONE, r4), 0.0))
    Ldiff = [_add(_add(_mul(T[i], lx), _mul(B[i], ly)), _mul(N[i], lz)) for i in range(3)]
    spec = q["r3"] < pspec.v if spec is None else spec
    Ls = _enormalize([_sel(spec, Lspec[i], Ldiff[i]) for i in range(3)])
    _, ps, _, _, gate_s, _, near_s = _eeval(s, N, Ng, V, NoV, pspec, Ls)
    tol["L_s"] = stack(Ls, 0.0)
    aux.update(L_s=vals3(Ls), ok=gate_s & (ps.v > 0.0), near_sample=near_s | pspec_lost | ~np.all(np.isfinite(tol["L_s"]), axis=1))
    return tol, aux


def lobe_pick(rows, out):
    """the lobe an implementation took: r3 < its own pspec, in binary32"""
    return np.asarray(rows, np.float32).reshape(-1, 20)[:, 17] < np.asarray(out, np.float32)[:, 0]


def check(rows, out, ok, cache=None):
    """Holds an implementation's (out[n, 12], ok[n]) to the reference within `tolerance`:
      pspec, f and pdf against the reference at the row's L;
      ok against the reference's, and L_s against the reference's direction for the row's draws (the lobe taken as the implementation's own
        binary32 pspec decides it: see `reference`);
      pdf_s and weight against the reference's pdf and f (N.L) / pdf AT THE DIRECTION THE IMPLEMENTATION RETURNED — what they are by SPEC §10 —, so that
        the direction's error, already held to its own tolerance, is not carried a second time through the narrow lobe.
    -> a dict: "bad"[n] the elements that miss; "ratio"[name] the largest error / tolerance over the compared elements; "left_out_eval",
    "left_out_sample" the shares of the elements whose f and pdf / whose ok, pdf_s and weight were NOT compared, because float64 cannot call the gate
    (see the module's head) AND the two sides took different sides of it, or because the model has no bound there; "ok_mismatch" the number of
    elements whose `ok` differs where float64 can call it.  Where a gate is close but both sides are on the same side of it, the values are compared
    as everywhere.  `cache`: a dict that keeps the reference and the tolerances between calls with the same rows, lobe picks and directions."""
    rows = np.asarray(rows, np.float32).reshape(-1, 20)
    out32, ok = np.asarray(out, np.float32), np.asarray(ok).astype(bool)
    out = out32.astype(np.float64)
    n = out.shape[0]
    spec = lobe_pick(rows, out32)
    if cache is not None and "spec" in cache and np.array_equal(cache["spec"], spec):
        (want, wok), (tol, aux) = cache["ref"], cache["tol"]
    else:
        (want, wok), (tol, aux) = reference(rows, spec=spec), tolerance(rows, spec=spec)
        if cache is not None:
            cache.clear()
            cache.update(spec=spec, ref=(want, wok), tol=(tol, aux))
    # the second pass: the implementation's own direction as L
    at = np.where(ok[:, None], out32[:, 5:8], rows[:, 11:14])         # (where there is no sample: V, unused)
    if cache is not None and "at" in cache and np.array_equal(cache["at"], at):
        (f2, pdf2, w2), (tol2, aux2) = cache["ref2"], cache["tol2"]
    else:
        rows2 = rows.copy()
        rows2[:, 14:17] = at
        (f2, pdf2, w2), (tol2, aux2) = reference_at(rows, at), tolerance(rows2, sample=False)
        if cache is not None:
            cache.update(at=at, ref2=(f2, pdf2, w2), tol2=(tol2, aux2))
    took_gate = (out[:, 4] > 0.0) | np.any(out[:, 1:4] != 0.0, axis=1)
    left_eval = aux["near_eval"] & (took_gate != aux["gate"])
    left_sample = (aux["near_sample"] & (ok != wok)) | (ok & aux2["near_eval"] & ~aux2["gate"])
    mismatch = ~aux["near_sample"] & (ok != wok)
    bad = mismatch.copy()
    ratio = {}
    some = ok & ~left_sample
    pairs = {"pspec": (out[:, 0:1], want[:, 0:1], tol["pspec"], np.ones(n, bool)),
             "f": (out[:, 1:4], want[:, 1:4], tol["f"], ~left_eval), "pdf": (out[:, 4:5], want[:, 4:5], tol["pdf"], ~left_eval),
             "L_s": (out[:, 5:8], aux["L_s"], tol["L_s"], ok),
             "weight": (out[:, 8:11], w2, tol2["w_at_L"], some), "pdf_s": (out[:, 11:12], pdf2[:, None], tol2["pdf"], some)}
    for name, (got, ref_, t, cmp_) in pairs.items():
        err = np.abs(got - ref_)
        unbounded = ~np.all(np.isfinite(t), axis=1)
        if name in ("pspec", "f", "pdf"):
            left_eval = left_eval | (unbounded & cmp_)
        else:
            left_sample = left_sample | (unbounded & cmp_)
        cmp_ = cmp_ & ~unbounded
        with np.errstate(all="ignore"):
            miss = ~(err <= np.where(np.isfinite(t), t, 0.0))           # a NaN output misses
            rr = np.where((t > 1e-44) & np.isfinite(t), err / t, 0.0)
        bad |= cmp_ & np.any(miss, axis=1)
        ratio[name] = float(np.max(np.where(cmp_[:, None], rr, 0.0))) if n else 0.0
    return {"bad": bad, "ratio": ratio, "left_out_eval": float(np.mean(left_eval)), "left_out_sample": float(np.mean(left_sample)),
            "ok_mismatch": int(mismatch.sum())}


# ------------------------------------------------------------------------------------------------ the inputs
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _nrm(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tangent(N, az):
    T, B = onb(N)
    return T * np.cos(az)[..., None] + B * np.sin(az)[..., None]


ROUGHNESS = [-1.0, 0.0, 0.045, float(np.nextafter(np.float32(0.045), np.float32(1.0))), 0.1, 0.5, 1.0, 2.0]
METALLIC = [-0.5, 0.0, 0.5, 1.0, 1.5]
BASE = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.8, 0.7, 0.6), (0.8, 0.0, 0.6)]
NOV = [1.0, 0.5, 1e-2, 1e-4, 1e-5, 0.0, -0.1]
N_KINDS = ["+z", "-z", "xy+0", "xy-0", "z+1e-7", "z-1e-7", "random"]
NG_KINDS = ["same", "tilt40", "tilt89", "behind"]          # behind: N.V < 0 < Ng.V
L_KINDS = ["mirror", "V", "-V", "NoL0", "NoL1e-6", "NoL1e-20", "NoL<0", "NgL<0", "NgL0", "random"]
R3_KINDS = ["0", "below", "pspec", "1-"]
R4 = [0.0, U, 0.5, float(ONE_M)]
_q = [np.float32(0.25), np.float32(0.5), np.float32(0.75)]
R5 = [0.0, float(np.nextafter(np.float32(0), np.float32(1)))] + [float(v) for c in _q for v in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(1)))] + [float(ONE_M)]
FACTORS = (len(ROUGHNESS), len(METALLIC), len(BASE), len(N_KINDS), len(NOV), len(NG_KINDS), len(L_KINDS), len(R3_KINDS), len(R4), len(R5))


def _edge_rows(idx, rng):
    """rows for the factor indices idx[n, 10] (r3 is filled in by edge_set, which needs the oracle's pspec)"""
    n = idx.shape[0]
    rows = np.zeros((n, 20), np.float32)
    rows[:, 3] = np.array(ROUGHNESS, np.float32)[idx[:, 0]]
    rows[:, 4] = np.array(METALLIC, np.float32)[idx[:, 1]]
    rows[:, 0:3] = np.array(BASE, np.float32)[idx[:, 2]]
    az = rng.uniform(0.0, 2.0 * np.pi, (n, 4))
    rnd = _nrm(rng.standard_normal((n, 3)))
    ca, sa = np.cos(az[:, 0]), np.sin(az[:, 0])
    z0, o1 = np.zeros(n), np.ones(n)
    Ns = [np.stack([z0, z0, o1], 1), np.stack([z0, z0, -o1], 1), np.stack([ca, sa, z0], 1), np.stack([ca, sa, -z0], 1),
          _nrm(np.stack([ca, sa, z0 + 1e-7], 1)), _nrm(np.stack([ca, sa, z0 - 1e-7], 1)), rnd]
    N = np.choose(idx[:, 3][:, None], Ns)
    N = _f32(N).astype(np.float64)          # the frame below is built on the normal the implementations see
    N[(idx[:, 3] == 3), 2] = -0.0
    nov = np.array(NOV)[idx[:, 4]]
    V = N * nov[:, None] + _tangent(N, az[:, 1]) * np.sqrt(1.0 - nov * nov)[:, None]
    tilt = np.array([0.0, np.radians(40.0), np.radians(89.0), np.radians(40.0)])[idx[:, 5]]
    axis = _tangent(N, az[:, 2])
    Ng = N * np.cos(tilt)[:, None] + axis * np.sin(tilt)[:, None]
    behind = idx[:, 5] == 3
    V = np.where(behind[:, None], N * np.cos(np.radians(100.0)) + axis * np.sin(np.radians(100.0)), V)
    t2 = _tangent(N, az[:, 3])
    perp = N - _dot(N, Ng)[:, None] * Ng             # in Ng's plane, on N's side; zero where Ng = N: the tangent then
    perp = np.where((np.linalg.norm(perp, axis=1) > 1e-6)[:, None], perp, t2)
    Lrand = _nrm(rng.standard_normal((n, 3)))
    Ls = [2.0 * _dot(N, V)[:, None] * N - V, V, -V, t2, _nrm(t2 + 1e-6 * N), _nrm(t2 + 1e-20 * N), _nrm(t2 - 0.3 * N), _nrm(_nrm(perp) - 0.05 * Ng), _nrm(perp), Lrand]
    L = np.choose(idx[:, 6][:, None], Ls)
    rows[:, 5:8], rows[:, 8:11], rows[:, 11:14], rows[:, 14:17] = _f32(N), _f32(Ng), _f32(V), _f32(L)
    rows[idx[:, 3] == 3, 7] = -0.0
    rows[idx[:, 6] == 2, 14:17] = -rows[idx[:, 6] == 2, 11:14]          # L = -V and L = V exactly, in binary32
    rows[idx[:, 6] == 1, 14:17] = rows[idx[:, 6] == 1, 11:14]
    rows[:, 18] = np.array(R4, np.float32)[idx[:, 8]]
    rows[:, 19] = np.array(R5, np.float32)[idx[:, 9]]
    return rows


def _products(defaults, **axes):
    """the full product of the named factors, the others at their defaults"""
    names = list(axes)
    grids = np.meshgrid(*[np.arange(k) for k in axes.values()], indexing="ij")
    idx = np.tile(np.array(defaults), (grids[0].size, 1))
    for nm, g in zip(names, grids):
        idx[:, nm if isinstance(nm, int) else int(nm)] = g.ravel()
    return idx


def random_rows(n, seed):
    """n rows with a fixed seed: materials over and a little beyond their ranges, a quarter of the roughnesses at or below the clamp, views from
    normal to far below grazing (log-uniform), half the geometric normals tilted up to 89 degrees, any L, 24-bit uniforms"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 20), np.float32)
    rows[:, 0:3] = rng.uniform(0.0, 1.0, (n, 3))
    rows[:, 3] = np.where(rng.uniform(size=n) < 0.25, rng.uniform(0.0, 0.06, n), rng.uniform(-0.1, 1.1, n))
    rows[:, 4] = rng.uniform(-0.2, 1.2, n)
    N = _f32(_nrm(rng.standard_normal((n, 3)))).astype(np.float64)
    nov = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0.0, 1.0, n), 10.0 ** -rng.uniform(0.0, 5.0, n))
    V = N * nov[:, None] + _tangent(N, rng.uniform(0.0, 2.0 * np.pi, n)) * np.sqrt(1.0 - nov * nov)[:, None]
    tilt = np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0.0, np.radians(89.0), n))
    Ng = N * np.cos(tilt)[:, None] + _tangent(N, rng.uniform(0.0, 2.0 * np.pi, n)) * np.sin(tilt)[:, None]
    rows[:, 5:8], rows[:, 8:11], rows[:, 11:14] = _f32(N), _f32(Ng), _f32(V)
    rows[:, 14:17] = _f32(_nrm(rng.standard_normal((n, 3))))
    rows[:, 17:20] = uniforms24(rng, (n, 3))
    return rows


def uniforms24(rng, shape):
    """SPEC §4's draws: float(w >> 8) 2^-24"""
    return (rng.integers(0, 1 << 24, shape).astype(np.float64) * U).astype(np.float32)


_EDGE = {}


def edge_set(oracle_probe, n_random=1 << 18):
    """The shared inputs: every value of every factor of the issue's list against a random draw of the others (4000 rows), full products of the
    factors that interact (roughness x NoV x L; N x Ng x NoV x r5; roughness x r3 x r4 x r5; metallic x r3 x r4 x r5 at minimum roughness and NoV 0.01), and n_random random rows.
    `oracle_probe(rows) -> (out, ok)` supplies the oracle's own pspec, at and just below which r3 is placed.  Computed once per process."""
    if n_random not in _EDGE:
        rng = np.random.default_rng(20240610)
        cover = np.stack([rng.integers(0, k, 4000) for k in FACTORS], axis=1)
        d = [5, 1, 2, 6, 1, 0, 9, 3, 2, 3]               # roughness 0.5, metallic 0, base (.8, .7, .6), N random, NoV 0.5, Ng = N, L random, r3 1-, r4 .5, r5 below 1/4
        prods = [_products(d, **{"0": 8, "4": 7, "6": 10}), _products(d, **{"3": 7, "5": 4, "4": 7, "9": 12}),
                 _products(d, **{"0": 8, "7": 4, "8": 4, "9": 12}), _products([2] + d[1:4] + [2] + d[5:], **{"1": 5, "7": 4, "8": 4, "9": 12})]
        idx = np.concatenate([cover] + prods, axis=0)
        rows = _edge_rows(idx, rng)
        ps = oracle_probe(rows)[0][:, 0].astype(np.float32)
        below = np.nextafter(ps, np.float32(0.0))
        rows[:, 17] = np.choose(idx[:, 7], [np.zeros_like(ps), below, ps, np.full_like(ps, ONE_M)])
        rows = np.concatenate([rows, random_rows(n_random, 77)], axis=0)
        assert np.all(np.isfinite(rows))
        _EDGE[n_random] = (rows, idx.shape[0])
    return _EDGE[n_random]


# the five configurations of the sampling tests (+ the metal for the weight test): base, roughness, metallic, N, tilt of Ng, NoV
CONFIGS = {
    "min roughness, NoV 0.8": ((0.8, 0.7, 0.6), 0.045, 0.0, (0.0, 0.0, 1.0), 0.0, 0.8),
    "min roughness, NoV 0.02": ((0.8, 0.7, 0.6), 0.045, 0.0, (0.0, 0.0, 1.0), 0.0, 0.02),
    "roughness 0.5, NoV 1e-5": ((0.8, 0.7, 0.6), 0.5, 0.0, (0.0, 0.0, 1.0), 0.0, 1e-5),
    "roughness 0.3, Ng tilted 0.7 rad": ((0.8, 0.7, 0.6), 0.3, 0.0, (0.0, 0.0, 1.0), 0.7, 0.6),
    "N = -z, roughness 0.2, metallic 0.5": ((0.8, 0.7, 0.6), 0.2, 0.5, (0.0, 0.0, -1.0), 0.0, 0.6),
    "metallic 1": ((0.95, 0.9, 0.8), 0.25, 1.0, (0.0, 0.0, 1.0), 0.0, 0.6),
}
DENSITY_CONFIGS = list(CONFIGS)[:5]


def config_rows(config, n=1 << 20, seed=5):
    """n rows of one configuration (a name in CONFIGS, or such a tuple) with fixed-seed 24-bit uniform triples (L is unused: V) -> rows, (N, Ng, V) in float64 as the rows hold them"""
    base, rough, metal, N, tilt, nov = CONFIGS[config] if isinstance(config, str) else config
    N = np.array(N, np.float64)
    t = _tangent(N[None], np.array([0.3]))[0]
    V = _f32(N * nov + t * np.sqrt(1.0 - nov * nov))
    Ng = _f32(N * np.cos(tilt) + _tangent(N[None], np.array([2.0]))[0] * np.sin(tilt))
    rows = np.zeros((n, 20), np.float32)
    rows[:, 0:3], rows[:, 3], rows[:, 4], rows[:, 5:8], rows[:, 8:11], rows[:, 11:14], rows[:, 14:17] = base, rough, metal, _f32(N), Ng, V, V
    rows[:, 17:20] = uniforms24(np.random.default_rng(seed), (n, 3))
    return rows, (N, Ng.astype(np.float64), V.astype(np.float64))


# ------------------------------------------------------------------------------------------------ the two integral checks, for either implementation
def density_estimates(name, probe):
    """Sampling against density for configuration `name`: with X = 1[ok] (N.L_s) / pdf64(L_s) over 2^20 fixed-seed draws, E[X] = the integral of
    N.L over the gate = pi (1 + cos gamma) / 2 whatever the lobes look like, and X <= pi / (1 - pspec).  pdf64 is the FLOAT64 density at the returned
    direction, so the known rounding of the reported pdf stays out.  -> [(label, mean, expected, standard error)]: the whole, then the eight
    octants of the azimuth about N against each octant's own integral."""
    rows, (N, Ng, V) = config_rows(name)
    out, ok = probe(rows)
    ok = np.asarray(ok).astype(bool)
    L = np.asarray(out, np.float64)[:, 5:8]
    p = pdf64(rows, L)
    with np.errstate(all="ignore"):
        x = np.where(ok & (p > 0.0), (L @ N) / p, 0.0)
    pspec = float(np.asarray(out)[0, 0])
    assert np.all(x >= 0.0) and x.max() <= np.pi / (1.0 - pspec) * (1.0 + 1e-6), (name, x.max(), pspec)
    n = x.shape[0]
    T, B = onb(N[None])
    octant = np.floor(np.mod(np.arctan2(L @ B[0], L @ T[0]), 2.0 * np.pi) / (np.pi / 4.0)).astype(int).clip(0, 7)
    want = octant_cosine_integrals(N, Ng)
    res = [("all", x.mean(), np.pi * (1.0 + float(N @ Ng) / np.linalg.norm(Ng)) / 2.0, x.std(ddof=1) / np.sqrt(n))]
    for k in range(8):
        xk = np.where(octant == k, x, 0.0)
        res.append(("octant %d" % k, xk.mean(), want[k], xk.std(ddof=1) / np.sqrt(n)))
    return res


def weight_estimates(name, probe):
    """-> (mean of 1[ok] weight over 2^20 fixed-seed draws [3], the directional albedo [3], standard error [3]) for configuration `name`"""
    rows, (N, Ng, V) = config_rows(name, seed=6)
    out, ok = probe(rows)
    w = np.where(np.asarray(ok).astype(bool)[:, None], np.asarray(out, np.float64)[:, 8:11], 0.0)
    base, rough, metal = CONFIGS[name][:3]
    return w.mean(axis=0), directional_albedo(base, rough, metal, N, Ng, V), w.std(axis=0, ddof=1) / np.sqrt(w.shape[0])


def dot32(a, b):
    """SPEC §3's dot in binary32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def sample_invariants(rows, out, ok, probe):
    """What every surviving sample must satisfy, whatever its value: unit length within 4 binary32 roundings (|v|^2 3, the root, the reciprocal and
    the scaling 1/2 each: 3 u), on the open side of both normals as binary32 computes it, pdf_s the implementation's own eval pdf at L_s bit for
    bit, and weight = f (NoL / pdf) recomputed in binary32 from its own eval.  -> the number of surviving samples"""
    rows, out, ok = np.asarray(rows, np.float32), np.asarray(out, np.float32), np.asarray(ok).astype(bool)
    r, o = rows[ok].copy(), out[ok]
    Ls = o[:, 5:8]
    assert np.all(np.abs(np.linalg.norm(Ls.astype(np.float64), axis=1) - 1.0) <= 4.0 * U)
    NoL = dot32(r[:, 5:8], Ls)
    assert np.all(NoL > 0.0) and np.all(dot32(r[:, 8:11], Ls) > 0.0)
    r[:, 14:17] = Ls
    e = np.asarray(probe(r)[0], np.float32)
    f, pdf = e[:, 1:4], e[:, 4]
    assert np.array_equal(pdf.view(np.uint32), o[:, 11].view(np.uint32)) and np.all(pdf > 0.0)
    w = NoL / pdf
    assert np.array_equal((f * w[:, None]).view(np.uint32), o[:, 8:11].view(np.uint32))
    return int(ok.sum())


# ------------------------------------------------------------------------------------------------ the furnace of lights (tests/kat_scenes.py) at this module's edges
# the materials kat_scenes.directional_albedo's grid cannot resolve, and where each is seen from: a mirror-smooth metal (roughness 0 -> the clamp, pspec = 1) from
# the furnace tests' usual eye, and the minimum roughness from N.V = 0.05 through a lens narrow enough that N.V spans 0.05 +- 0.002 over the frame
FURNACE_EYE = np.array([0.9, 1.3, 2.2])
FURNACE_CASES = [((0.95, 0.9, 0.8), 0.0, 1.0), ((0.8, 0.6, 0.4), 0.045, 0.0)]
FURNACE_VIEW = {(0.045, 0.0): (np.array([1.9, 0.1, 0.6]), 0.004)}


def furnace_view(rough, metal):
    """-> (eye, vfov of the GPU test's 256 x 256 frame) for a furnace material"""
    return FURNACE_VIEW.get((rough, metal), (FURNACE_EYE, 0.02))


def furnace_albedo(base, rough, metal, eye):
    """the albedo the furnace quad (normal +y) shows towards `eye`"""
    return directional_albedo(base, rough, metal, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), eye)


# ------------------------------------------------------------------------------------------------ two pins that came out of the first run of these tests
# (1 - VoH)^5 is negative where VoH rounds above 1: |V|, |H| <= 1 + 2u and the dot's 3 roundings leave VoH - 1 <= 8u, so F and f may fall below 0 by
# (8u)^5 D vis at most, with D <= 1 / (pi a2) and vis <= 1 / (4 k (k + 1e-4 (1 - k))) at the roughness clamp: 4.4e-22.  weight = f (NoL / pdf) scales that by
# NoL / pdf <= pi / (1 - pspec) <= 10 pi; a sample of pspec = 1 cannot have VoH > 1 (there L is V's mirror about a half vector tilted off V)
_A_MIN = F32_MIN_ROUGH ** 2
NEGATIVE_F_FLOOR = -((8.0 * U) ** 5) / (np.pi * _A_MIN ** 2) / (4.0 * (_A_MIN / 2.0) * (_A_MIN / 2.0 + 1e-4 * (1.0 - _A_MIN / 2.0)))


def assert_not_negative(out):
    out = np.asarray(out, np.float64)
    assert out[:, 0].min() >= 0.1 and out[:, 4].min() >= 0.0 and out[:, 11].min() >= 0.0          # pspec, pdf, pdf_s
    assert out[:, 1:4].min() >= NEGATIVE_F_FLOOR and out[:, 8:11].min() >= 10.0 * np.pi * NEGATIVE_F_FLOOR, (out[:, 1:4].min(), out[:, 8:11].min())


GRAZING = ((0.8, 0.7, 0.6), 0.045, 0.0, (0.0, 0.0, 1.0), 0.0, 1e-4)


def grazing_weights(probe, n=1 << 18):
    """A GGX sample's weight at the roughness clamp seen from N.V = 1e-4, and what bounds it.  V and L are unit to binary32 only, so V.(V + L) =
    (|V|^2 - 1) + 2 (V.H)^2 rounds to <= 0 once V.H < 2e-4; before SPEC §10 gated f as well as pdf on VoH > 0 the pdf lost its specular term there while
    f kept D at the lobe's peak, and 0.7 % of these draws weighed more than 1e3, the largest 5e11.  weight = f NoL / pdf <= diff / (1 - pspec) +
    4 vis F NoL VoH / (pspec NoH) <= 10 + 10 / ((1 - k)(k + 1e-4 (1 - k)) NoH): for the draws whose half vector has NoH >= 1/2 -> (largest weight, bound)"""
    rows, _ = config_rows(GRAZING, n=n)
    out, ok = probe(rows)
    a2 = _A_MIN ** 2
    r4 = rows[:, 18].astype(np.float64)
    near = (1.0 - r4) / (1.0 + (a2 - 1.0) * r4) >= 0.25
    k = _A_MIN / 2.0
    w = np.asarray(out, np.float64)[:, 8:11].max(axis=1)[near & (np.asarray(ok) == 1)]
    return float(w.max()), 10.0 + 20.0 / ((1.0 - k) * (k + 1e-4 * (1.0 - k)))
