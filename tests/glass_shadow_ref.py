"""SPEC.md §27 (shadows through thin glass) restated in numpy, from the SPEC: the channel transmittance tau of a thin-walled pane, the threshold xi of a
candidate hit and the pass bits.  With dtype float32 every operation is one binary32 rounding in the SPEC's order (numpy's float32 add, multiply, divide
and sqrt are correctly rounded), so `decide` is what the device hook must return bit for bit; with dtype float64 the same code is the expectation the
frames are held to, and `tau_bound` is a derived bound on what the binary32 evaluation may differ from it.  Test infrastructure only; built on
tests/alpha_ref.py (the texture coordinate), tests/blend_ref.py (§4's pcg), tests/transmission_ref.py (§21's Fresnel) and tests/texture_ref.py (the tables)."""
import numpy as np

import alpha_ref
import blend_ref
import texture_ref
import transmission_ref

F = np.float32
U32 = np.uint32
SALT = U32(0x9E3779B9)
U = 2.0 ** -24


def xi(prim, u, v):
    """h = pcg(pcg(pcg(prim ^ 0x9E3779B9) ^ bits(u)) ^ bits(v)); xi = float(h >> 8)·2^-24, in [0, 1): exact in binary32"""
    prim, u, v = np.broadcast_arrays(np.asarray(prim).astype(U32), np.asarray(u, F), np.asarray(v, F))
    h = blend_ref.pcg(blend_ref.pcg(blend_ref.pcg(prim ^ SALT) ^ blend_ref.bits(u)) ^ blend_ref.bits(v))
    return ((h >> U32(8)).astype(F) * F(2.0 ** -24)).astype(F)


def lookup32(image, tu, tv, srgb):
    """SPEC §9's bilinear, repeat lookup of image[H, W, 4] (uint8) in binary32 -> [n, 4]: rgb through the sRGB table where `srgb`, else b·(1/255)"""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[:2]
    tu, tv = np.asarray(tu, F), np.asarray(tv, F)
    fx, fy = tu * F(W) - F(0.5), tv * F(H) - F(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f).astype(F)[:, None], (fy - y0f).astype(F)[:, None]
    x0, y0 = np.mod(x0f.astype(np.int64), W), np.mod(y0f.astype(np.int64), H)
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)

    def tap(y, x):
        b = image[y, x]
        out = texture_ref.LINEAR_LUT[b]
        if srgb:
            out[:, :3] = texture_ref.SRGB_LUT[b[:, :3]]
        return out.astype(F)

    one = F(1.0)
    top = tap(y0, x0) * (one - tx) + tap(y0, x1) * tx
    bot = tap(y1, x0) * (one - tx) + tap(y1, x1) * tx
    return (top * (one - ty) + bot * ty).astype(F)


def material_at(color, metallic, uv, albedo, mra, hu, hv):
    """§21's base rgb and metallic at the hit (hu, hv), binary32: the record's colour and metallic, times the albedo image's sRGB-decoded rgb and the mra
    image's b where the material has them (None: it has not); uv[3, 2] are the triangle's texture coordinates.  A pair of equal-sized images reads the
    same texels with the same weights (SPEC §9), so one function serves both dispatches.  -> (base[n, 3], metal[n])"""
    hu, hv = np.asarray(hu, F).reshape(-1), np.asarray(hv, F).reshape(-1)
    n = hu.shape[0]
    base = np.tile(np.asarray(color, F)[:3], (n, 1))
    metal = np.full(n, F(metallic), F)
    if albedo is not None or mra is not None:
        tu, tv = alpha_ref.interp_uv(uv, hu, hv)
        if albedo is not None:
            base = (base * lookup32(albedo, tu, tv, True)[:, :3]).astype(F)
        if mra is not None:
            metal = (metal * lookup32(mra, tu, tv, False)[:, 2]).astype(F)
    return base, metal


def cosine(p, d, dtype=F):
    """c = min2(|dot(d, Ng)|·(1/sqrt(l2)), 1) on the geometric normal Ng = cross(p1 − p0, p2 − p0), l2 = dot(Ng, Ng), of the triangle p[3, 3] (binary32 data)
    for unit directions d[n, 3] -> (c[n], degenerate: l2 <= 0 or NaN)"""
    p = np.asarray(p, F).astype(dtype)
    d = np.asarray(d, F).astype(dtype).reshape(-1, 3)
    a, b = p[1] - p[0], p[2] - p[0]
    Ng = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype)
    l2 = (Ng[0] * Ng[0] + Ng[1] * Ng[1]) + Ng[2] * Ng[2]
    one = dtype(1)
    if not l2 > 0:
        return np.zeros(d.shape[0], dtype), True
    dn = (d[:, 0] * Ng[0] + d[:, 1] * Ng[1]) + d[:, 2] * Ng[2]
    return np.minimum(np.abs(dn) * (one / np.sqrt(l2)), one).astype(dtype), False


def tau(base, metal, tr, ior, c, dtype=F):
    """tau_c = (pt·(1 − Fr))·base_c, pt = tr·(1 − clamp(metal, 0, 1)), Fr = §21's Fresnel at cosine c with eta = 1/ior -> [n, 3]"""
    base = np.asarray(base).astype(dtype).reshape(-1, 3)
    n = base.shape[0]
    metal, tr, ior, c = (np.broadcast_to(np.asarray(x).astype(dtype), (n,)) for x in (metal, tr, ior, c))
    one, zero = dtype(1), dtype(0)
    pt = tr * (one - np.minimum(np.maximum(metal, zero), one))
    Fr, _ = transmission_ref.fresnel(c, (one / ior).astype(dtype))
    k = (pt * (one - Fr)).astype(dtype)
    return (k[:, None] * base).astype(dtype)


def bits(t, x):
    """bit c (0 red, 1 green, 2 blue): tau_c > xi (a NaN tau does not pass)"""
    t = np.asarray(t)
    x = np.asarray(x)[:, None]
    with np.errstate(invalid="ignore"):
        p = t > x
    return (p[:, 0].astype(U32) | (p[:, 1].astype(U32) << U32(1)) | (p[:, 2].astype(U32) << U32(2))).astype(U32)


def decide(prim, p, uv, color, metallic, albedo, mra, trans, hu, hv, d):
    """what glass_shadow_eval returns for hits (hu, hv) of directions d on baked triangle `prim` with vertices p[3, 3], texture coordinates uv[3, 2], and a
    material of base colour `color`, metallic `metallic`, images albedo / mra (or None) and transmission state trans = (factor, ior, thin_walled) or None
    (opaque) -> (tau[n, 3] float32, xi[n] float32, bits[n] uint32).  Zeros for an opaque or solid material; a degenerate thin triangle keeps its xi"""
    hu, hv = np.asarray(hu, F).reshape(-1), np.asarray(hv, F).reshape(-1)
    n = hu.shape[0]
    z3, z1, zb = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, U32)
    if trans is None or not trans[0] > 0 or not trans[2]:
        return z3, z1, zb
    x = xi(np.full(n, prim, U32), hu, hv)
    c, degenerate = cosine(p, d, F)
    if degenerate:
        return z3, x, zb
    base, metal = material_at(color, metallic, uv, albedo, mra, hu, hv)
    t = tau(base, metal, F(trans[0]), F(trans[1]), c, F)
    return t, x, bits(t, x)


def tau_bound(base, ior, c):
    """A bound on |tau32 − tau64| per channel for the same binary32 inputs (base, metal, tr, ior, c), first order in u = 2^-24 with every rounding counted at
    its largest, times 2 for the second-order terms.  The chain (all quantities in [0, 1] unless said):
      eta = fl(1/ior): u relative; e2 = fl(eta·eta): 3u relative; fl(c·c), fl(1 − ·), max2: 2u absolute; s2 = fl(e2·…): 6u absolute; w = fl(1 − s2): 7u absolute;
      ct = fl(sqrt(w)): |sqrt(w + δ) − sqrt(w)| <= min(|δ|/(2 sqrt(w)), sqrt(|δ|)), plus its own rounding: e_ct = min(7u/(2 ct), sqrt(7u)) + u — this is where
      the evaluation is ill-conditioned, at grazing incidence and where eta → 1 (there s2 → 1 and binary32 may even take the total-reflection branch, Fr = 1,
      where binary64 does not: the bound then exceeds 1 and says so);
      A = fl(eta·c): 2u·A absolute; rs = fl((A − ct)/(A + ct)): numerator and denominator each carry e_A + e_ct + u·D, |rs| <= 1, so
      e_rs = 2(e_A + e_ct)/D + 3u with D = A + ct; B = fl(eta·ct): e_ct + 2u; rp likewise with D' = c + B: e_rp = 2(e_ct + 2u)/D' + 3u;
      Fr = fl(0.5·fl(rs² + rp²)): e_Fr = e_rs + e_rp + 3u (|rs|, |rp| <= 1); k = fl(pt·fl(1 − Fr)) with pt's own three roundings: e_Fr + 5u; tau = fl(k·base): base·(e_Fr + 6u).
    Total reflection in BOTH evaluations is exact (tau = 0).  -> [n, 3] float64"""
    base = np.asarray(base, np.float64).reshape(-1, 3)
    ior, c = (np.broadcast_to(np.asarray(x, np.float64), (base.shape[0],)) for x in (ior, c))
    eta = 1.0 / ior
    ct = np.sqrt(np.maximum(0.0, 1.0 - eta * eta * np.maximum(0.0, 1.0 - c * c)))
    with np.errstate(divide="ignore", invalid="ignore"):
        e_ct = np.minimum(np.where(ct > 0, 7.0 * U / (2.0 * ct), np.inf), np.sqrt(7.0 * U)) + U
        A = eta * c
        e_rs = 2.0 * (2.0 * U * A + e_ct) / (A + ct) + 3.0 * U
        e_rp = 2.0 * (e_ct + 2.0 * U) / (c + eta * ct) + 3.0 * U
    e_fr = np.where((A + ct) > 0, e_rs + e_rp + 3.0 * U, 1.0)
    return 2.0 * base * (e_fr + 6.0 * U)[:, None]
