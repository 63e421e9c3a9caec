"""SPEC §30 written again in numpy, from the section and not from the C++: the display transform (exposure, the CLAMP / PBR_NEUTRAL / ACES curves, §13.2's sRGB
encoding) in binary32 with every intermediate a np.float32, the same curves in binary64 together with a running bound on what binary32 may lose, and the meter's
histogram and its evaluation.

One text serves both precisions: the curves are written once over a small arithmetic context.  `F32` rounds every operation to binary32 (numpy adds, multiplies and
divides float32 arrays one correctly rounded operation at a time: nothing is fused).  `Err` carries a binary64 value v and a bound e on |binary32 result - v|, grown
term by term: an operation's inherited error by the usual first-order rules made rigorous (the products of two errors are kept), plus one rounding u = 2^-24 of the
largest magnitude the binary32 result can have, plus 2^-149 for a result that may be subnormal.  Comparisons (x < 0.08, p < 0.76, min, max) are exact in both; where
a branch is taken, `Err` replays the decisions binary32 made, so both walk the same path (the curves are continuous at both branch points: test_display checks it)."""
import math

import numpy as np

CLAMP, PBR_NEUTRAL, ACES = 0, 1, 2
OPERATORS = {"clamp": CLAMP, "pbr_neutral": PBR_NEUTRAL, "aces": ACES}
U = 2.0 ** -24
TINY = 2.0 ** -149
LOG2_018 = -2.4739311883324124   # log2(0.18), §30.3's one literal
BINS = 384

ACES_IN = ((0.59719, 0.35458, 0.04823), (0.07600, 0.90834, 0.01566), (0.02840, 0.13383, 0.83777))
ACES_OUT = ((1.60475, -0.53108, -0.07367), (-0.10208, 1.10813, -0.00605), (-0.00327, -0.07276, 1.07602))


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------- §13.2
def thresholds():
    """thr[i]: the linear value at which sRGB code i starts — the inverse OETF at (i - 0.5) / 255 in binary64, rounded once"""
    thr = np.zeros(256, np.float32)
    for i in range(1, 256):
        v = (i - 0.5) / 255.0
        thr[i] = np.float32(v / 12.92 if v <= 0.04045 else math.pow((v + 0.055) / 1.055, 2.4))
    return thr


THR = thresholds()


def encode_srgb8(c):
    """clamp to [0, 1] (a NaN to 0), then the largest code whose threshold is <= c"""
    c = f32(c)
    c = np.where(c > 0, c, np.float32(0))
    c = np.where(c < 1, c, np.float32(1))
    return (np.searchsorted(THR, c, side="right") - 1).astype(np.uint8)


# ---------------------------------------------------------------------------- the two arithmetic contexts
class F32:
    @staticmethod
    def lift(x):
        return f32(x)

    const = lift

    @staticmethod
    def add(a, b):
        return f32(a) + f32(b)

    @staticmethod
    def sub(a, b):
        return f32(a) - f32(b)

    @staticmethod
    def mul(a, b):
        return f32(a) * f32(b)

    @staticmethod
    def div(a, b):
        return f32(a) / f32(b)

    @staticmethod
    def val(a):
        return a


class Err:
    """(v, e): v in binary64, e >= |the binary32 result - v|"""

    @staticmethod
    def lift(x):   # an input: exact
        x = np.asarray(x, np.float64)
        return (x, np.zeros_like(x))

    @staticmethod
    def const(x):  # "all constants are the nearest binary32": the same number in both
        x = np.asarray(np.float32(x), np.float64)
        return (x, np.zeros_like(x))

    @staticmethod
    def _round(v, d):
        return (v, d + U * (np.abs(v) + d) + TINY)

    @staticmethod
    def add(a, b):
        return Err._round(a[0] + b[0], a[1] + b[1])

    @staticmethod
    def sub(a, b):
        return Err._round(a[0] - b[0], a[1] + b[1])

    @staticmethod
    def mul(a, b):
        return Err._round(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])

    @staticmethod
    def div(a, b):
        v = a[0] / b[0]
        room = np.abs(b[0]) - b[1]
        assert np.all(room > 0), "a divisor that may be zero"
        return Err._round(v, (a[1] + np.abs(v) * b[1]) / room)

    @staticmethod
    def val(a):
        return a[0]


def _where(mask, a, b):
    if isinstance(a, tuple):
        return (np.where(mask, a[0], b[0]), np.where(mask, a[1], b[1]))
    return np.where(mask, a, b)


def _pick(A, xs, larger):
    """min or max of a list: exact, it selects one of them (in `Err` by the values)"""
    out = xs[0]
    for x in xs[1:]:
        take = A.val(x) > A.val(out) if larger else A.val(x) < A.val(out)
        out = _where(take, x, out)
    return out


# ---------------------------------------------------------------------------- the curves, once
def pbr_neutral(A, c, replay=None):
    """c: three channels of exposed colour (>= 0, not NaN; +inf handled by rule).  Returns (channels, the branch decisions)"""
    K = A.const
    x = _pick(A, c, larger=False)
    low = A.val(x) < np.float32(0.08) if replay is None else replay["low"]
    xs = _where(np.isinf(A.val(x)), K(1.0), x)   # a harmless x where the branch is not taken
    off = _where(low, A.sub(xs, A.mul(A.mul(K(6.25), xs), xs)), K(0.04))
    c = [A.sub(ch, off) for ch in c]
    p = _pick(A, c, larger=True)
    done = A.val(p) < np.float32(0.76) if replay is None else replay["done"]
    inf = np.isinf(A.val(p))   # the rule: np = 1 and the result is (1, 1, 1)
    with np.errstate(all="ignore"):
        ps = _where(done | inf, K(1.0), p)   # a harmless p where the branch is not taken
        d = K(0.24)
        np_ = A.sub(K(1.0), A.div(A.mul(d, d), A.sub(A.add(ps, d), K(0.76))))
        s = A.div(np_, ps)
        k = A.sub(K(1.0), A.div(K(1.0), A.add(A.mul(K(0.15), A.sub(ps, np_)), K(1.0))))
        out = []
        for ch in c:
            chs = _where(done | inf, ps, ch)
            t = A.mul(chs, s)
            t = A.add(t, A.mul(A.sub(np_, t), k))
            out.append(_where(done, ch, _where(inf, K(1.0), t)))
    return out, {"low": low, "done": done}


def aces(A, c):
    K = A.const
    big = np.float32(2.0 ** 60)
    c = [_where(A.val(ch) < big, ch, A.lift(np.broadcast_to(big, np.shape(A.val(ch))))) for ch in c]

    def row(m, v):
        return A.add(A.add(A.mul(K(m[0]), v[0]), A.mul(K(m[1]), v[1])), A.mul(K(m[2]), v[2]))

    def fit(v):
        n = A.sub(A.mul(v, A.add(v, K(0.0245786))), K(0.000090537))
        q = A.add(A.mul(v, A.add(A.mul(K(0.983729), v), K(0.4329510))), K(0.238081))
        return A.div(n, q)

    v = [fit(row(m, c)) for m in ACES_IN]
    return [row(m, v) for m in ACES_OUT]


def curve(A, op, c, replay=None):
    if op == PBR_NEUTRAL:
        return pbr_neutral(A, c, replay)
    if op == ACES:
        return aces(A, c), {}
    return list(c), {}


# ---------------------------------------------------------------------------- the transform
def mean32(accum):
    """m = a.w > 0 ? a.xyz / a.w : 0"""
    a = f32(accum).reshape(-1, 4)
    with np.errstate(all="ignore"):
        w = a[:, 3:4]
        return np.where(w > 0, a[:, :3] / w, np.float32(0)).astype(np.float32)


def gain(ev):
    return np.float32(2.0 ** float(ev))   # exp2 in binary64, rounded once


def expose32(m, ev):
    """c = max2(m * g, 0): a NaN and a negative value give 0, +inf stays"""
    with np.errstate(all="ignore"):
        c = f32(m) * gain(ev)
    return np.where(c > 0, c, np.float32(0)).astype(np.float32)


def transform32(accum, ev, op):
    """[n, 3] float32: what §13.2's encoding is given"""
    c = expose32(mean32(accum), ev)
    with np.errstate(all="ignore"):
        out, _ = curve(F32, op, [c[:, 0], c[:, 1], c[:, 2]])
    return np.stack([f32(o) for o in out], axis=1)


def display_bytes(accum, ev, op):
    """[n, 4] uint8: the bytes k_display<op> presents for accumulators [n, 4]"""
    t = transform32(accum, ev, op)
    out = np.full((t.shape[0], 4), 255, np.uint8)
    out[:, :3] = encode_srgb8(t)
    return out


def curve32(op, c):
    c = f32(c).reshape(-1, 3)
    with np.errstate(all="ignore"):
        out, dec = curve(F32, op, [c[:, 0], c[:, 1], c[:, 2]])
    return np.stack([f32(o) for o in out], axis=1), dec


def curve64(op, c, replay=None):
    """([n, 3] float64 values, [n, 3] bounds on |binary32 - value|) of the curve alone on finite exposed colours c; `replay`: binary32's branch decisions"""
    c = np.asarray(c, np.float64).reshape(-1, 3)
    out, _ = curve(Err, op, [Err.lift(c[:, 0]), Err.lift(c[:, 1]), Err.lift(c[:, 2])], replay)
    return np.stack([o[0] for o in out], axis=1), np.stack([o[1] for o in out], axis=1)


# ---------------------------------------------------------------------------- the shared case set
def _ulps(x, k):
    """the float32 k ulps away from x (k of either sign; x finite and not zero)"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def edge_accumulators(n=1025):
    """[n, 4] accumulators, the special ones first: a.w = 0 (and negative, NaN, infinite); NaN, +-inf, negative and denormal channels; values up to 2^60 and FLT_MAX;
    the branch points 0.08 and 0.76 with the floats around them, as the minimum / the maximum of a pixel and as a grey that reaches p = 0.76 behind the offset; every
    threshold thr[i] with the float one ulp to either side; then random pixels, log-uniform over 2^-30 .. 2^20, with sample counts 1 .. 4"""
    fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
    rows = [(1.0, 2.0, 3.0, 0.0), (1.0, 2.0, 3.0, -1.0), (1.0, 2.0, 3.0, np.nan), (1.0, 2.0, 3.0, np.inf), (np.inf, 1.0, 1.0, np.inf), (0.0, 0.0, 0.0, 0.0)]
    specials = [0.0, -0.0, np.nan, np.inf, -np.inf, -1.0, -1e-30, tiny, 1e-40, np.finfo(np.float32).tiny, 2.0 ** 60, _ulps(2.0 ** 60, 1), _ulps(2.0 ** 60, -1), 1e30,
                fmax, 0.18, 1.0, 4.0, 1000.0]
    for v in specials:
        rows += [(v, v, v, 1.0), (v, 0.5, 0.25, 1.0), (0.25, v, 0.5, 1.0), (0.5, 0.25, v, 1.0)]
    rows += [(fmax, fmax, fmax, 0.5), (3.0, 6.0, 9.0, 3.0), (tiny, tiny, tiny, 4.0)]
    for k in range(-3, 4):
        lo, hi = (_ulps(0.08, k), _ulps(0.76, k)) if k else (np.float32(0.08), np.float32(0.76))
        g = _ulps(0.8, k) if k else np.float32(0.8)
        rows += [(lo, 0.5, 0.9, 1.0), (0.5, lo, lo, 1.0), (hi, 0.0, 0.3, 1.0), (0.0, 0.2, hi, 1.0), (g, g, g, 1.0), (lo, lo, hi, 1.0)]
    for t in THR[1:]:
        for k in (-1, 0, 1):
            v = _ulps(t, k) if k else t
            rows.append((v, v, v, 1.0))
    rows = np.array(rows, np.float32)
    assert rows.shape[0] <= n
    rng = np.random.default_rng(30)
    m = n - rows.shape[0]
    w = rng.integers(1, 5, m).astype(np.float32)
    rnd = np.concatenate([(2.0 ** rng.uniform(-30, 20, (m, 3))).astype(np.float32) * w[:, None], w[:, None]], axis=1).astype(np.float32)
    return np.concatenate([rows, rnd])


def meter_accumulators(n=1025):
    """[n, 4]: for every power of two from 2^-25 to 2^24 and the float one ulp below it, grey pixels whose luminance IS that value where a grey within a few ulps has
    it (the three weights sum to 1, so most do), and the grey of that value itself; pixels without a sample, NaN, infinite, negative and zero pixels; random ones"""
    rows = [(1.0, 1.0, 1.0, 0.0), (np.nan, 1.0, 1.0, 1.0), (np.inf, 0.0, 0.0, 1.0), (-1.0, -1.0, -1.0, 1.0), (0.0, 0.0, 0.0, 1.0), (2.0, 4.0, 6.0, 2.0), (1.0, 1.0, 1.0, -1.0)]
    exact = 0
    for e in range(-25, 25):
        for target in (np.float32(2.0 ** e), _ulps(2.0 ** e, -1)):
            rows.append((target, target, target, 1.0))
            for k in range(-4, 5):
                v = _ulps(target, k) if k else target
                if luminance32(np.array([[v, v, v]], np.float32))[0] == target:
                    rows.append((v, v, v, 1.0))
                    exact += 1
                    break
    rows = np.array(rows, np.float32)
    assert exact >= 50 and rows.shape[0] <= n, exact
    rng = np.random.default_rng(31)
    m = n - rows.shape[0]
    rnd = np.concatenate([(2.0 ** rng.uniform(-28, 26, (m, 3))).astype(np.float32), np.ones((m, 1), np.float32)], axis=1)
    return np.concatenate([rows, rnd])


# ---------------------------------------------------------------------------- §30.3: the meter
def luminance32(m):
    m = f32(m).reshape(-1, 3)
    k = [np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)]
    with np.errstate(all="ignore"):
        return ((k[0] * m[:, 0]) + (k[1] * m[:, 1])) + (k[2] * m[:, 2])


def histogram(accum):
    """(hist[384] uint32, skipped) of accumulators [n, 4]: pixels with a.w > 0 alone; Y outside [2^-24, 2^24), infinite or NaN is skipped"""
    a = f32(accum).reshape(-1, 4)
    sampled = a[:, 3] > 0
    Y = luminance32(mean32(a))[sampled]
    with np.errstate(invalid="ignore"):
        ok = (Y >= np.float32(2.0 ** -24)) & (Y < np.float32(2.0 ** 24))
    bins = (Y[ok].view(np.uint32) >> 20).astype(np.int64) - ((127 - 24) << 3)
    assert bins.size == 0 or (bins.min() >= 0 and bins.max() < BINS)
    return np.bincount(bins, minlength=BINS).astype(np.uint32), int(np.count_nonzero(~ok))


def evaluate(hist, low, high):
    """(ev float32, counted): integers throughout; the sum over bin centres in sixteenths, exact"""
    h = [int(x) for x in hist]
    assert len(h) == BINS
    N = sum(h)
    lo, hi = math.floor(float(np.float32(low)) * float(N)), math.floor(float(np.float32(high)) * float(N))
    for b in range(BINS):
        t = min(h[b], lo)
        h[b] -= t
        lo -= t
    for b in reversed(range(BINS)):
        t = min(h[b], hi)
        h[b] -= t
        hi -= t
    Np = sum(h)
    if Np == 0:
        return np.float32(0.0), 0
    S16 = sum(cnt * (2 * b + 1 - 2 * 8 * 24) for b, cnt in enumerate(h))   # centre_b = (b + 0.5) / 8 - 24 = (2 b + 1 - 384) / 16
    assert abs(S16) < 2 ** 53
    return np.float32(LOG2_018 - (S16 / 16.0) / float(Np)), Np
