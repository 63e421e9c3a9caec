"""A binary64 restatement of the denoiser passes of SPEC §15.2-15.4 (test infrastructure), written from the SPEC text in numpy,
and the seeded edge inputs that drive it, the oracle (`oracle.orc.Denoiser.filter`) and the kernels through the same frames.

Float32 where the SPEC defines a quantity by its float32 rounding, so that a decision never flips on rounding alone:
  * the decoded normal (SPEC §15.1 decode, `v·(1/√(v·v))`) and the normal dot `(x·x' + y·y') + z·z'`;
  * the luminance `(0.2126 r + 0.7152 g) + 0.0722 b` that à-trous compares (of the float32 radiance it reads);
  * the reprojected position `(x + 0.5) + motion·W`, its in-image test and the pixel `floor` picks;
  * the reuse test (history, prim id, normal dot ≥ 0.9, `|z − z'| ≤ 0.1·max(z, z')`) and the miss test.
Every value (albedo demodulation, moments, variance, weights, sums, composite) is binary64.

Error bounds.  Next to each value the reference carries a first-order bound on how far a float32 evaluation of the same
formulas (the oracle, the kernels: one rounding of unit u = 2^-24 per operation, -ffp-contract=off) can lie from it, built from
the reference's own terms; `tolerance` doubles it to cover the second-order terms.  See `Temporal.step`, `atrous` and `composite`.

`MUTANTS` names the deliberate misreadings of the SPEC that a test must tell apart from the oracle (tests/test_denoise_reference.py).
"""
import numpy as np

INVALID = 0xFFFFFFFF
U = 2.0 ** -24
ETA = 2.0 ** -150   # the absolute error of a float32 rounding into the subnormal range
F = np.float32
LUM = np.array([0.2126, 0.7152, 0.0722])
B3 = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])
STEPS = (1, 2, 4, 8)
CAP = 64

MUTANTS = {
    "trunc": "truncation instead of floor for the reprojected pixel",
    "inside_le_w": "`m.x <= W` in the inside test",
    "cap63": "history cap 63",
    "nocap": "no history cap",
    "normal_gt": "`> 0.9` instead of `>= 0.9`",
    "depth_min": "`0.1·min(z, z')` instead of `0.1·max(z, z')`",
    "boost_h3": "variance boost while h < 3 instead of h < 4",
    "spacing_1244": "tap spacing 1, 2, 4, 4",
    "uniform_taps": "uniform 5x5 taps instead of B3",
    "var_w": "variance `Σ v w / Σ w`",
    "pow64": "`max(n·n', 0)^64` instead of ^128",
    "sigma_z_no_eps": "no `+1e-6` in σ_z",
    "tap_miss": "miss pixels are tapped",
    "clamp_taps": "out-of-image taps clamped to the border instead of skipped",
    "no_albedo_floor": "no 0.05 albedo floor",
}


# ------------------------------------------------------------------ float32 definitions (SPEC §15.1-15.3)
def f32_bits(z):
    return np.asarray(z, F).view(np.uint32)


def oct_decode32(p):
    """SPEC §15.1 decode, float32: f = u16·(2/65535) − 1, z = (1 − |x|) − |y|, folded for z < 0, then v·(1/√(v·v))"""
    p = np.asarray(p, np.uint32)
    k = F(3.0518043793392844e-05)
    fx = (p & 0xFFFF).astype(F) * k - F(1)
    fy = (p >> 16).astype(F) * k - F(1)
    fz = (F(1) - np.abs(fx)) - np.abs(fy)
    fold = fz < 0
    tx = (F(1) - np.abs(fy)) * np.where(fx >= 0, F(1), F(-1)).astype(F)
    ty = (F(1) - np.abs(fx)) * np.where(fy >= 0, F(1), F(-1)).astype(F)
    fx, fy = np.where(fold, tx, fx), np.where(fold, ty, fy)
    l2 = (fx * fx + fy * fy) + fz * fz
    with np.errstate(divide="ignore"):
        inv = F(1) / np.sqrt(l2)
    n = np.stack([fx * inv, fy * inv, fz * inv], -1)
    return np.where((l2 > 0)[..., None], n, F(0)).astype(F)


def oct_encode32(n):
    """SPEC §15.1 encode, float32 (to build inputs): p = n.xy / (|x| + |y| + |z|), folded for z < 0, u16 = uint(clamp(p·0.5+0.5)·65535+0.5)"""
    n = np.asarray(n, F)
    l1 = (np.abs(n[..., 0]) + np.abs(n[..., 1])) + np.abs(n[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        px = np.where(l1 > 0, n[..., 0] / l1, F(0)).astype(F)
        py = np.where(l1 > 0, n[..., 1] / l1, F(0)).astype(F)
    fold = n[..., 2] < 0
    tx = (F(1) - np.abs(py)) * np.where(px >= 0, F(1), F(-1)).astype(F)
    ty = (F(1) - np.abs(px)) * np.where(py >= 0, F(1), F(-1)).astype(F)
    px, py = np.where(fold, tx, px), np.where(fold, ty, py)
    ux = (np.clip(px * F(0.5) + F(0.5), F(0), F(1)) * F(65535) + F(0.5)).astype(np.uint32)
    uy = (np.clip(py * F(0.5) + F(0.5), F(0), F(1)) * F(65535) + F(0.5)).astype(np.uint32)
    return ux | (uy << 16)


def dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def lum32(c):
    c = np.asarray(c, F)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def albedo(w, mutant=None):
    """SPEC §15.2 a = max(albedo/255, 0.05) per channel of the RGBA8 word, binary64"""
    w = np.asarray(w, np.uint32)
    a = np.stack([(w >> s) & 0xFF for s in (0, 8, 16)], -1) / 255.0
    return a if mutant == "no_albedo_floor" else np.maximum(a, 0.05)


def tolerance(bound):
    """the per-value tolerance: twice the first-order bound (the second-order terms are far below it)"""
    return 2.0 * bound


def excess(got, want, bound):
    """|got − want| / tolerance per value (0 where they are equal, inf where only one of them is finite or the tolerance is 0)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = tolerance(np.asarray(bound, np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / tol
    r = np.where(got == want, 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


# ------------------------------------------------------------------ 15.2 temporal
class Temporal:
    """The reference's own history: ping-pong of G-buffer, colour, moments and history length, carried in binary64 with their
    error bounds from frame to frame.

    Bound of one frame (first order in u), for a reused pixel with α = 1/h and the previous bound e':
      il = L/a:                 e_il = 4u·|il|            (a's float32 product and the division)
      lm = lum(il):             e_lm = 8u·lum(|il|)
      c = c' + (il − c')·α:     e_c = (1−α)·e'_c + α·e_il + 3u·α·|il − c'| + u·|c|   (same for m1 with lm, m2 with lm²,
                                                                                      e_lm² = 2|lm|·e_lm + u·lm²)
      var = max(m2 − m1², 0):   e_v = e_m2 + 2|m1|·e_m1 + u·(m1² + |m2 − m1²|), and for the boost m1²·k (k = (4−h)/4)
                                      + k·(2|m1|·e_m1 + 2u·m1²) + u·|var|
    A pixel that is not reused starts again from c = il (e_c = e_il)."""

    def __init__(self, w, h, mutant=None):
        self.w, self.h, self.mutant = w, h, mutant
        n = w * h
        self.g = np.zeros((n, 4), np.uint32)
        self.c, self.ec = np.zeros((n, 3)), np.zeros((n, 3))
        self.m, self.em = np.zeros((n, 2)), np.zeros((n, 2))
        self.hist = np.zeros(n, np.uint32)

    def reproject(self, motion):
        """the previous-frame pixel index of every pixel and whether it is inside (SPEC §15.2, float32)"""
        W, H, mut = self.w, self.h, self.mutant
        n = W * H
        y, x = np.divmod(np.arange(n), W)
        mo = np.asarray(motion, F).reshape(n, 2)
        with np.errstate(invalid="ignore", over="ignore"):
            fx = (x.astype(F) + F(0.5)) + mo[:, 0] * F(W)
            fy = (y.astype(F) + F(0.5)) + mo[:, 1] * F(H)
            rnd = np.trunc if mut == "trunc" else np.floor
            mx, my = rnd(fx), rnd(fy)
            xmax = mx <= F(W) if mut == "inside_le_w" else mx < F(W)
            inside = (mx >= 0) & (my >= 0) & xmax & (my < F(H))
        j = np.where(inside, np.where(inside, my, 0).astype(np.int64) * W + np.where(inside, mx, 0).astype(np.int64), 0) % n
        return inside, j

    def step(self, noisy, gbuf, motion):
        """one frame; returns rad (n, 4: colour, variance), its bound, moments (n, 2), their bound, history (n)"""
        mut, n = self.mutant, self.w * self.h
        g = np.asarray(gbuf, np.uint32).reshape(n, 4)
        L = np.asarray(noisy, F).reshape(n, 4)[:, :3].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            il = L / albedo(g[:, 3], mut)
        lm = il @ LUM
        e_il, e_lm = 4 * U * np.abs(il), 8 * U * (np.abs(il) @ LUM)
        inside, j = self.reproject(motion)
        gp, hp = self.g[j], self.hist[j]
        zc, zp = g[:, 1].view(F), gp[:, 1].view(F)
        zref = np.where(zc < zp, zc, zp) if mut == "depth_min" else np.where(zc > zp, zc, zp)
        d = dot32(oct_decode32(g[:, 2]), oct_decode32(gp[:, 2]))
        nok = d > F(0.9) if mut == "normal_gt" else d >= F(0.9)
        with np.errstate(invalid="ignore", over="ignore"):
            zok = np.abs(zc - zp) <= F(0.1) * zref
        ok = inside & (hp > 0) & (gp[:, 0] == g[:, 0]) & nok & zok
        cap = {"cap63": 63, "nocap": 1 << 30}.get(mut, CAP)
        h = np.where(ok, np.minimum(hp.astype(np.int64) + 1, cap), 1)
        al = 1.0 / h
        x = np.concatenate([il, lm[:, None], (lm * lm)[:, None]], 1)
        ex = np.concatenate([e_il, e_lm[:, None], (2 * np.abs(lm) * e_lm + U * lm * lm)[:, None]], 1)
        prev = np.concatenate([self.c[j], self.m[j]], 1)
        eprev = np.concatenate([self.ec[j], self.em[j]], 1)
        with np.errstate(invalid="ignore", over="ignore"):
            blend = prev + (x - prev) * al[:, None]
            eb = (1 - al[:, None]) * eprev + al[:, None] * ex + 3 * U * al[:, None] * np.abs(x - prev) + U * np.abs(blend)
        new = np.where(ok[:, None], blend, x)
        enew = np.where(ok[:, None], eb, ex)
        c, m1, m2 = new[:, :3], new[:, 3], new[:, 4]
        ec, em1, em2 = enew[:, :3], enew[:, 3], enew[:, 4]
        with np.errstate(invalid="ignore", over="ignore"):
            raw = m2 - m1 * m1
            var = np.maximum(raw, 0.0)
            ev = em2 + 2 * np.abs(m1) * em1 + U * (m1 * m1 + np.abs(raw))
            k = np.maximum(4 - h, 0) * 0.25 if mut != "boost_h3" else np.where(h < 3, (4 - h) * 0.25, 0.0)
            var = var + m1 * m1 * k
            ev = ev + k * (2 * np.abs(m1) * em1 + 2 * U * m1 * m1) + U * np.abs(var) * (k > 0)
        self.g, self.c, self.ec = g.copy(), c, ec
        self.m, self.em = np.stack([m1, m2], 1), np.stack([em1, em2], 1)
        self.hist = h.astype(np.uint32)
        return (np.concatenate([c, var[:, None]], 1), np.concatenate([ec, ev[:, None]], 1), self.m.copy(), self.em.copy(), self.hist.copy())


# ------------------------------------------------------------------ 15.3 à-trous
def atrous(gbuf, rad, step, rows=None, mutant=None):
    """One pass at tap spacing `step` of the float32 radiance `rad` (h, w, 4: colour, variance) over the rows `rows` (a range,
    default all).  Returns the binary64 result and its bound, both (len(rows), w, 4).

    Bound (first order in u).  A tap's weight w = (k·wn)·(wz·wl) has, next to the float32 evaluation,
      wn = max(n·n', 0)^128:  128·(max(d, 0) + e_d)^127·e_d + 127u·wn,  e_d = 3u·Σ|n_i n'_i|
      wz, wl:                 13u each, relative (σ: 3u, the quotient 5u, the square 11u, 1/(1+r²) 2u more)
      the three products:     3u, relative, and 8η absolute (η = 2^-150: a rounding into the subnormal range)
    and then, with S = Σ w, R = Σ c w / S, V = Σ v w² / S² over the 25 taps,
      e_R = (Σ|c − R|·e_w + 25u·(Σ|c|·w + |R|·S) + Σ 2η·(|c| + 1)) / S + 2u·|R| + 2η
      e_V = (Σ 2|v|·w·e_w + 26u·Σ|v|·w² + Σ 2η·(|v| + 1)) / S² + 2|V|·(Σ e_w + 25u·S) / S + 4u·|V| + 2η
    Miss pixels pass through: exact."""
    g = np.asarray(gbuf, np.uint32)
    r32 = np.asarray(rad, F)
    H, W = g.shape[:2]
    rows = range(H) if rows is None else rows
    ys = np.arange(rows.start, rows.stop)[:, None]
    xs = np.arange(W)[None, :]
    nrm = oct_decode32(g[..., 2])
    z = g[..., 1].view(F).astype(np.float64)
    lum = lum32(r32[..., :3]).astype(np.float64)
    miss = g[..., 0] == INVALID
    c64 = r32.astype(np.float64)
    nc, zc, lc, cc = nrm[ys, xs].astype(np.float64), z[ys, xs], lum[ys, xs], c64[ys, xs]
    sig_l = 4 * np.sqrt(np.maximum(cc[..., 3], 0)) + 1e-4
    sig_z = 0.02 * zc + (0.0 if mutant == "sigma_z_no_eps" else 1e-6)
    kw = np.full(5, 0.2) if mutant == "uniform_taps" else B3
    wc = kw[2] * kw[2]
    S, Sc, Sv = np.full(zc.shape, wc), cc[..., :3] * wc, cc[..., 3] * wc * wc
    taps = []
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx == 0 and dy == 0:
                continue
            qy, qx = ys + dy * step, xs + dx * step
            valid = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            if mutant == "clamp_taps":
                valid = np.ones_like(valid)
            qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            if mutant != "tap_miss":
                valid = valid & ~miss[qy, qx]
            nq = nrm[qy, qx].astype(np.float64)
            pr = nc * nq
            d = pr.sum(-1)
            e_d = 3 * U * np.abs(pr).sum(-1)
            dp = np.maximum(d, 0)
            wn = dp ** (64 if mutant == "pow64" else 128)
            e_wn = 128 * (dp + e_d) ** 127 * e_d + 127 * U * wn
            with np.errstate(invalid="ignore", divide="ignore"):
                rz = np.abs(zc - z[qy, qx]) / sig_z
                rl = np.abs(lc - lum[qy, qx]) / sig_l
                wz, wl = 1 / (1 + rz * rz), 1 / (1 + rl * rl)
            k = kw[dx + 2] * kw[dy + 2]
            w = np.where(valid, k * wn * wz * wl, 0.0)
            ew = np.where(valid, w * (29 * U) + k * wz * wl * e_wn + 8 * ETA, 0.0)
            q = c64[qy, qx]
            S = S + w
            Sc = Sc + q[..., :3] * w[..., None]
            Sv = Sv + q[..., 3] * (w if mutant == "var_w" else w * w)
            taps.append((qy, qx, w, ew))
    with np.errstate(invalid="ignore", divide="ignore"):
        R = Sc / S[..., None]
        V = Sv / S if mutant == "var_w" else Sv / (S * S)
    aR = np.abs(cc[..., :3]) * wc
    eR, sumew = np.zeros_like(R), np.zeros_like(S)
    ev1, ev2 = np.zeros_like(S), np.abs(cc[..., 3]) * wc * wc
    eu = np.zeros_like(R)
    for qy, qx, w, ew in taps:
        q = c64[qy, qx]
        with np.errstate(invalid="ignore"):
            eR = eR + np.abs(q[..., :3] - R) * ew[..., None]
        aR = aR + np.abs(q[..., :3]) * w[..., None]
        sumew = sumew + ew
        ev1 = ev1 + 2 * np.abs(q[..., 3]) * w * ew + 2 * ETA * (np.abs(q[..., 3]) + 1)
        eu = eu + 2 * ETA * (np.abs(q[..., :3]) + 1)
        ev2 = ev2 + np.abs(q[..., 3]) * w * w
    with np.errstate(invalid="ignore", divide="ignore"):
        eR = (eR + eu + 25 * U * (aR + np.abs(R) * S[..., None])) / S[..., None] + 2 * U * np.abs(R) + 2 * ETA
        eV = (ev1 + 26 * U * ev2) / (S * S) + 2 * np.abs(V) * (sumew + 25 * U * S) / S + 4 * U * np.abs(V) + 2 * ETA
    out = np.concatenate([R, V[..., None]], -1)
    eb = np.concatenate([eR, eV[..., None]], -1)
    m = miss[ys, xs][..., None]
    return np.where(m, cc, out), np.where(m, 0.0, eb)


def composite(gbuf_w, c, e_c, mutant=None):
    """SPEC §15.4: main = (c·a, 1); bound e_c·a + 3u·|c·a| (a's float32 product, the product)"""
    a = albedo(gbuf_w, mutant)
    with np.errstate(invalid="ignore"):
        main = c[..., :3] * a
    return main, e_c[..., :3] * a + 3 * U * np.abs(main)


# ------------------------------------------------------------------ edge inputs
def _pcg(v):
    v = (np.asarray(v, np.uint64) * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    w = (((v >> ((v >> np.uint64(28)) + np.uint64(4))) ^ v) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    return ((w >> np.uint64(22)) ^ w).astype(np.uint32)


def _normalize(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def threshold_normals():
    """octahedral codes (A, B) whose decoded float32 dot is exactly 0.9f, the next float above and the next float below
    (the reuse threshold of SPEC §15.2); found by a scan of the codes around the cone of cos = 0.9 about A"""
    a = oct_encode32(_normalize([0.31, -0.22, 0.92]))
    na = oct_decode32(a)
    t1 = _normalize(np.cross(na.astype(np.float64), [1.0, 0.0, 0.0]))
    t2 = np.cross(na.astype(np.float64), t1)
    phi = np.linspace(0, 2 * np.pi, 4000, endpoint=False)[:, None]
    cand = 0.9 * na.astype(np.float64) + np.sqrt(1 - 0.81) * (np.cos(phi) * t1 + np.sin(phi) * t2)
    c = oct_encode32(cand)
    du, dv = np.meshgrid(np.arange(-3, 4), np.arange(-3, 4))
    u = ((c & 0xFFFF)[:, None].astype(np.int64) + du.reshape(-1)).clip(0, 65535)
    v = ((c >> 16)[:, None].astype(np.int64) + dv.reshape(-1)).clip(0, 65535)
    codes = np.unique((u | (v << 16)).astype(np.uint32))
    d = dot32(na, oct_decode32(codes))
    t = F(0.9)
    out = {}
    for name, want in (("eq", t), ("above", np.nextafter(t, F(1))), ("below", np.nextafter(t, F(0)))):
        hit = codes[d == want]
        assert hit.size, "no code at dot %r" % want
        out[name] = int(hit[0])
    return int(a), out


def threshold_depths(zp=2.0):
    """(z', z) pairs at the 10 % reuse threshold of SPEC §15.2, float32: the last accepted and the first rejected depth above and
    below z', and one pair that only `0.1·max` accepts (0.1·min < |z − z'| ≤ 0.1·max)"""
    zp = F(zp)
    up = np.array(sorted(set(F(zp / F(0.9)) + np.arange(-6, 7, dtype=F) * np.spacing(F(zp / F(0.9))))), F)
    dn = np.array(sorted(set(F(zp * F(0.9)) + np.arange(-6, 7, dtype=F) * np.spacing(F(zp * F(0.9))))), F)

    def acc(z):
        return np.abs(z - zp) <= F(0.1) * np.where(z > zp, z, zp)
    a_up, a_dn = acc(up), acc(dn)
    pairs = [up[a_up].max(), up[~a_up].min(), dn[a_dn].min(), dn[~a_dn].max(), F(zp * F(1.105))]
    return zp, [F(z) for z in pairs]


def _integer_landing(W, off):
    """a float32 motion mo with (x + 0.5) + mo·W landing exactly on x + 0.5 + off for an off of ±k + 0.5"""
    mo = F(off / W)
    for _ in range(64):
        p = mo * F(W)
        if p == F(off):
            return mo
        mo = np.nextafter(mo, F(np.inf) if p < F(off) else F(-np.inf))
    raise AssertionError("no integer landing for W=%d" % W)


class EdgeSequence:
    """Seeded frames of (noisy (h, w, 4) float32, gbuf (h, w, 4) uint32, motion (h, w, 2) float32): a static layout held for
    `static` frames (history reaches and holds the cap), then `events` frames of edge motion, normal, depth and id changes.

    Layout: 6x5 blocks of one primitive with jittered normals (some flipped: anti-parallel neighbours, some folded z < 0) and
    depths (some tiny, where σ_z is mostly its 1e-6); rows y ≡ 1, 2 (mod 4) are one full-width primitive of constant normal and
    depth (a NaN motion that reprojects onto column 0, or a row end read one past W, lands on a compatible pixel there); miss pixels isolated, in runs and
    on the right border (half of them with a neighbour's depth and normal); emitter ids; albedo bytes 0 and 255; radiance that is black, constant in time (zero variance) or
    drawn afresh each frame."""

    def __init__(self, w, h, static=66, events=8, seed=1):
        self.w, self.h, self.static, self.events, self.seed = w, h, static, events, seed
        n = w * h
        y, x = np.divmod(np.arange(n, dtype=np.int64), w)
        self.x, self.y = x, y
        r = lambda k: _pcg(np.arange(n, dtype=np.uint64) * np.uint64(16) + np.uint64(k) + np.uint64(seed) * np.uint64(0x9E3779B9))
        self.r = r
        uf = lambda k: r(k).astype(np.float64) / 2.0 ** 32
        block = (x // 6) + 1000 * (y // 5)
        bu = lambda k: _pcg(block.astype(np.uint64) * np.uint64(8) + np.uint64(k) + np.uint64(seed) * np.uint64(7919)).astype(np.float64) / 2.0 ** 32
        wall = (y % 4 == 1) | (y % 4 == 2)
        self.wall = wall
        prim = np.where(wall, 7, 100 + block).astype(np.uint32)
        kind = r(0) % 100
        self.miss = (~wall & (kind < 6)) | (~wall & (y % 11 == 9) & (x % 13 < 5)) | (~wall & (x == w - 1) & (y % 2 == 0) & (w > 1))
        emit = ~wall & ~self.miss & (kind >= 6) & (kind < 9)
        prim = np.where(emit, 0x80000000 | (r(1) % 4), prim)
        prim = np.where(self.miss, INVALID, prim).astype(np.uint32)
        # normals: per block a direction, per pixel a jitter; 5 % anti-parallel to their block, 10 % of the blocks facing z < 0
        base = _normalize(np.stack([bu(1) - 0.5, bu(2) - 0.5, np.where(bu(3) < 0.1, -1, 1) * (0.3 + bu(4))], -1))
        jit = 0.06 * np.stack([uf(2) - 0.5, uf(3) - 0.5, uf(4) - 0.5], -1)
        nrm = _normalize(base + jit) * np.where(kind[:, None] >= 95, -1, 1)
        nrm = np.where(wall[:, None], _normalize([0.1, 0.2, 0.95]), nrm)
        depth = (0.5 + 20 * bu(5)) * (1 + 0.06 * (uf(5) - 0.5))
        depth = np.where(bu(6) < 0.15, 1e-6 * (1 + 4 * uf(6)), depth)
        depth = np.where(wall, 3.0, depth)
        # a miss pixel's depth is the traversal's t_max, 1e30, on half of them; on the other half it and the normal are those of a
        # neighbour, so that only the miss test keeps à-trous from tapping them
        depth = np.where(self.miss & (r(17) % 2 == 0), 1e30, depth)
        nrm_code = oct_encode32(nrm)
        a = np.stack([r(7 + s) % 256 for s in range(3)], -1)
        a = np.where((r(10) % 5 == 0)[:, None], 0, a)
        a = np.where((r(11) % 5 == 0)[:, None], 255, a)
        self.alb = (a[:, 0] | (a[:, 1] << 8) | (a[:, 2] << 16) | (0xFF << 24)).astype(np.uint32)
        self.alb = np.where(self.miss | emit, 0xFFFFFFFF, self.alb).astype(np.uint32)
        self.prim, self.depth, self.nrm_code = prim, depth.astype(F), nrm_code
        self.lclass = r(12) % 4      # 0 black, 1 constant, 2-3 fresh each frame
        self.lconst = np.stack([uf(13 + s) * 2 for s in range(3)], -1)
        # event classes (after the static run), on non-wall pixels; NaN / inf / huge motions on wall pixels
        ev = r(20) % 16
        self.ev = np.where(wall, 100 + ev, ev)
        self.na, self.nb = threshold_normals()
        self.zp, self.zthr = threshold_depths()

    def __len__(self):
        return self.static + self.events

    def frame(self, k):
        w, h, n, x, y = self.w, self.h, self.w * self.h, self.x, self.y
        rk = lambda t: _pcg(np.arange(n, dtype=np.uint64) * np.uint64(64) + np.uint64(t) + np.uint64(k) * np.uint64(0x2545F491) + np.uint64(self.seed))
        fresh = np.stack([rk(s).astype(np.float64) / 2.0 ** 32 * 3 for s in range(3)], -1)
        L = np.where((self.lclass == 0)[:, None], 0.0, np.where((self.lclass == 1)[:, None], self.lconst, fresh))
        prim, depth, code = self.prim.copy(), self.depth.copy(), self.nrm_code.copy()
        mo = np.zeros((n, 2), F)
        e = k - self.static
        ev = self.ev
        # threshold pixels hold their threshold state through the static run too
        thr_n, thr_z = (ev == 1) & ~self.miss, (ev == 2) & ~self.miss
        code = np.where(thr_n, self.na, code)
        depth = np.where(thr_z, self.zp, depth)
        if e >= 0:
            kinds = ("eq", "above", "below")
            if e % 2 == 0:
                code = np.where(thr_n, self.nb[kinds[(e // 2) % 3]], code)
                depth = np.where(thr_z, self.zthr[(e // 2) % len(self.zthr)], depth)
            sub = (rk(10).astype(np.float64) / 2.0 ** 32 - 0.5) * 0.98
            sub2 = (rk(11).astype(np.float64) / 2.0 ** 32 - 0.5) * 0.98
            mo[:, 0] = np.where(ev == 3, sub / w, mo[:, 0])
            mo[:, 1] = np.where(ev == 3, sub2 / h, mo[:, 1])
            # whole-pixel shifts of 1-3 in both signs (reprojection within and across blocks)
            sh = (rk(12) % 7).astype(np.int64) - 3
            mo[:, 0] = np.where(ev == 4, F(sh) / F(w), mo[:, 0])
            mo[:, 1] = np.where(ev == 5, F(sh) / F(h), mo[:, 1])
            # landings exactly on pixel corners (x + 0.5 + mo·W an integer)
            land = np.array([_integer_landing(w, o) for o in (-1.5, -0.5, 0.5, 1.5)], F)
            mo[:, 0] = np.where(ev == 6, land[rk(13) % 4], mo[:, 0])
            mo[:, 1] = np.where(ev == 6, np.array([_integer_landing(h, o) for o in (-1.5, -0.5, 0.5, 1.5)], F)[rk(14) % 4], mo[:, 1])
            # a primitive id change (disocclusion)
            prim = np.where((ev == 7) & (e % 2 == 1) & (prim != INVALID), prim ^ 0x40, prim).astype(np.uint32)
            # every border pixel pushed out by less than a pixel (the first event frame: trunc vs floor), into its own row/column otherwise
            if e == 0 or e == 5:
                out = 0.3 + 0.6 * (rk(15).astype(np.float64) / 2.0 ** 32)
                mo[:, 0] = np.where(x == 0, F(-(0.5 + out) / w), np.where(x == w - 1, F((0.5 + out) / w), mo[:, 0]))
                mo[:, 1] = np.where(y == 0, F(-(0.5 + out) / h), np.where(y == h - 1, F((0.5 + out) / h), mo[:, 1]))
            # wall rows: NaN, ±inf and huge finite motions (|mo·W| > 2^31), a row's pixels onto its neighbours otherwise
            wk = ev - 100
            big = F(3e9)
            mo[:, 0] = np.where(wk == 0, F(np.nan), mo[:, 0])
            mo[:, 1] = np.where(wk == 1, F(np.nan), mo[:, 1])
            mo[:, 0] = np.where(wk == 2, F(np.inf), np.where(wk == 3, F(-np.inf), mo[:, 0]))
            mo[:, 1] = np.where(wk == 4, F(np.inf), np.where(wk == 5, F(-np.inf), mo[:, 1]))
            mo[:, 0] = np.where(wk == 6, big, np.where(wk == 7, -big, mo[:, 0]))
            mo[:, 1] = np.where(wk == 8, big, np.where(wk == 9, -big, mo[:, 1]))
            mo[:, 0] = np.where((wk >= 10) & (wk < 13), F(1.0) / F(w), mo[:, 0])   # (x + 1.5): row x+1, (W − 1) + 1.5: outside
        noisy = np.concatenate([L, np.ones((n, 1))], 1).astype(F).reshape(h, w, 4)
        g = np.stack([prim, f32_bits(depth), code, self.alb], -1).astype(np.uint32).reshape(h, w, 4)
        return noisy, g, mo.reshape(h, w, 2)


SIZES = [(1, 1), (1, 17), (17, 1), (19, 13), (257, 3), (160, 96)]
BIG = (3840, 2160)


def sequence(w, h):
    """the committed edge sequence of one size: 66 static frames + 8 event frames, or 2 frames at 3840x2160"""
    if (w, h) == BIG:
        return EdgeSequence(w, h, static=1, events=1, seed=5)
    return EdgeSequence(w, h, static=66, events=8, seed=1 + w * 7 + h)


def check_rows(w, h):
    """rows whose à-trous result is checked: all, or three bands of the 3840x2160 frame (top, middle, bottom)"""
    if h <= 200:
        return [range(0, h)]
    return [range(0, 24), range(h // 2 - 12, h // 2 + 12), range(h - 24, h)]


HALO = 2 * (1 + 2 + 4 + 8)   # rows beyond a band that the four passes read


def oracle_chain(atrous_pass, gbuf, rad, rows, steps=STEPS):
    """the float32 passes (an `atrous_pass(gbuf, rad, step)` callable) over the rows `rows` plus the rows they read, cropped;
    returns the input of every pass and the last output, each over `rows` only.  Cropping is exact: a pass at spacing s reads
    rows within 2s, so a result HALO rows inside the crop does not see its edge."""
    H = gbuf.shape[0]
    y0, y1 = max(rows.start - HALO, 0), min(rows.stop + HALO, H)
    g, cur = gbuf[y0:y1], np.ascontiguousarray(rad[y0:y1])
    ins = []
    for s in steps:
        ins.append(cur)
        cur = atrous_pass(g, cur, s)
    return ins, cur, range(rows.start - y0, rows.stop - y0), (y0, y1)


# ------------------------------------------------------------------ stage-by-stage comparison
class Checker:
    """Runs the reference next to a float32 implementation frame by frame and returns, per stage, the largest
    |implementation − reference| / tolerance (inf for a history that differs).  The à-trous passes are checked one at a time on
    the implementation's own input to that pass (`atrous_pass`, the oracle's), so that errors do not pile up across passes; the
    main target against the composite of the reference's last pass (mode 1) or of its temporal result (mode 2)."""

    def __init__(self, w, h, mode, mutant=None):
        self.w, self.h, self.mode, self.mutant = w, h, mode, mutant
        self.temporal = Temporal(w, h, mutant)
        self.steps = (1, 2, 4, 4) if mutant == "spacing_1244" else STEPS

    def frame(self, inputs, rad, hist, main, atrous_pass, mom=None):
        noisy, gbuf, motion = inputs
        w, h = self.w, self.h
        r_rad, e_rad, r_mom, e_mom, r_hist = self.temporal.step(noisy, gbuf, motion)
        out = {"history": 0.0 if np.array_equal(hist.reshape(-1), r_hist) else np.inf,
               "temporal colour": excess(rad.reshape(-1, 4)[:, :3], r_rad[:, :3], e_rad[:, :3]).max(),
               "variance": excess(rad.reshape(-1, 4)[:, 3], r_rad[:, 3], e_rad[:, 3]).max()}
        if mom is not None:
            out["moments"] = excess(mom.reshape(-1, 2), r_mom, e_mom).max()
        if self.mode == 2:
            m, e = composite(gbuf.reshape(-1, 4)[:, 3], r_rad, e_rad, self.mutant)
            out["main"] = excess(main.reshape(-1, 4)[:, :3], m, e).max()
            return out
        for rows in check_rows(w, h):
            ins, last, r, (y0, y1) = oracle_chain(atrous_pass, gbuf, rad.reshape(h, w, 4), rows)
            outs = ins[1:] + [last]
            for k, s in enumerate(self.steps):
                ref, eb = atrous(gbuf[y0:y1], ins[k], s, rows=r, mutant=self.mutant)
                key = "atrous %d" % STEPS[k]
                out[key] = max(out.get(key, 0.0), excess(outs[k][r.start:r.stop], ref, eb).max())
            m, e = composite(gbuf[rows.start:rows.stop, :, 3], ref, eb, self.mutant)
            out["main"] = max(out.get("main", 0.0), excess(main[rows.start:rows.stop, :, :3], m, e).max())
        return out
