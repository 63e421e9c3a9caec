"""A binary64 restatement of the primary pass (test infrastructure): camera rays (SPEC §4, §11), the primary hit by brute force
(§7's rules, §8's emitters) and what bounce-0 shading writes for the denoiser, the G-buffer and the motion vectors (§15.1) — written
from the SPEC text and plain geometry in numpy, not from the kernels or the oracle.  It also holds the small scene and the camera
sequence that drive the oracle (tests/test_primary_reference.py) and the kernels (tests/test_gpu_primary_reference.py) through it.

What is exact.  The jitter: the §4 stream in uint32 (`u = float(w >> 8)·2^-24` is exact in binary32 and binary64 alike) and, with a
noise texture, §4.3's shift evaluated in binary32 left to right as the SPEC's preamble prescribes — it DEFINES the sample position, so it is restated
in the format the SPEC gives it.  Everything behind it — ray, hit, normal, albedo, projection — is binary64.

Error bounds.  Next to each value the reference carries a first-order bound on how far a binary32 evaluation of the SPEC's formulas
may lie from it (u = 2^-24 per rounding, -ffp-contract=off), built from the reference's own terms:
  * ray direction: `K_D·u` per component (derivation at K_D);
  * hit distance and barycentrics: from the terms of §7's affine test (`hit_bounds`): every product of a Woop row with the ray carries
    the rounding of the row (§6 rounds it once) and of the fma chain, the direction carries K_D·u, `t = −oz/dz` one more rounding;
  * hit point, interpolated normal, texture coordinate: the barycentric bound times the triangle's edge / normal / uv differences;
  * octahedral code: half a step of the 16-bit grid plus the binary32 error of the projected normal (`normal_code_bound`);
  * albedo byte: exact, ±1 only within the binary32 error of a `k + 0.5` boundary (`allowed_albedo`);
  * motion: from the terms of `project` (`project`), doubled by the checker as tests/denoise_ref.py does.
The depth bound is derived (`hit_bounds`), not measured: no number in this file comes from running the oracle or the kernels.

Excluded pixels: only those whose EDGE DISTANCE is below `EDGE_EPS`.  The edge distance of a pixel is the smallest barycentric margin
`|min(u, v, 1−u−v)|` (rectangles: `|min(1−|a|/hw, 1−|b|/hh)|`) over every primitive whose plane the ray crosses no farther than
`t_best·(1 + 1e-5)` — the hit itself, a neighbour across a shared edge, a nearer silhouette the ray just misses — and 0 where two
primitives are hit within that relative distance of each other.  `EDGE_EPS` is derived at its definition.

`MUTANTS` names the deliberate misreadings that the checker must tell apart from the oracle."""
import math

import numpy as np

U = 2.0 ** -24
INVALID = 0xFFFFFFFF
LIGHT_BIT = 0x80000000
T_MISS = np.float32(1e30)
F = np.float32

# Ray direction, absolute error per component of the unit vector in binary32 (§11), in units of u, for |cx|, |cy| <= 1.5:
#   sx = (x + jx)/W: 2 roundings, 2·sx − 1: 1 more, absolute <= 5u on a value in [−1, 1];  ax = aspect·tan(vfov/2) in binary32:
#   tan (2 ulp), aspect (1), product (1) -> 4u relative;  cx = (...)·ax: <= (5 + 4 + 1)u·1.5 = 15u absolute, likewise cy;
#   right·cx + up·cy + fwd per component: |right_i|·15u + |up_i|·15u + 3 roundings of values <= 2.5 -> <= (15·√2 + 7.5)u < 29u on a
#   vector of length >= 1;  normalise (dot 3, sqrt 1, 1/x 1, product 1): 6u.  Total < 35u; K_D = 40.
K_D = 40.0

# Edge threshold, in barycentric units.  §7 states the rounding of the affine test as ≈ 3e-7·(|o| + t) world units; the frames below keep
# |o| + t < 20 and every triangle edge > 0.5, so a barycentric coordinate moves by < 3e-7·20/0.5 = 1.2e-5, and the ray's own direction
# error K_D·u·t / edge < 40·6e-8·14/0.5 = 7e-5 on top.  1e-4 covers both.
EDGE_EPS = 1.0e-4

MUTANTS = {
    "pixel_centre": "pixel centre instead of the jitter",
    "cy_not_flipped": "`cy = (2sy − 1)·tan` (image upside down)",
    "aspect_on_ay": "aspect applied to ay instead of ax",
    "tan_full": "`tan(vfov)` for `tan(vfov/2)`",
    "motion_cur_minus_prev": "motion = project(cur) − project(prev)",
    "motion_pixels": "motion in pixels instead of uv units",
    "motion_no_half": "project without the 0.5 (NDC instead of uv)",
    "prev_keeps_axay": "previous basis with the current frame's ax, ay",
    "prev_is_cur": "previous basis already the current one",
    "no_identity_start": "no identity before the first frame (the first frame reprojects onto itself)",
    "geometric_normal": "geometric instead of shading normal",
    "normal_not_flipped": "shading normal not flipped to the viewer's side",
    "miss_normal_plus_d": "miss normal +d",
    "trunc_u16": "truncation instead of +0.5 in the u16 packing of the normal",
    "trunc_u8": "truncation instead of +0.5 in the u8 packing of the albedo",
    "albedo_no_texture": "albedo without the texture",
    "albedo_unclamped": "albedo not clamped before packing",
    "emitter_albedo_light": "emitter albedo = the light's radiance",
    "depth_along_fwd": "depth along fwd (z-depth) instead of along the ray",
    "motion_behind_prev": "motion computed for a point behind the previous camera",
}


# ------------------------------------------------------------------ §4 RNG, exact
def pcg(v):
    v = np.asarray(v, np.uint32)
    with np.errstate(over="ignore"):
        s = v * np.uint32(747796405) + np.uint32(2891336453)
        w = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
    return (w >> np.uint32(22)) ^ w


TAG_RAYGEN = int.from_bytes(b"RAYG", "big")


def jitter(W, H, user_seed, seed_counter, noise=None, mutant=None):
    """(jx, jy) of every pixel, (H·W,) float64 holding exact binary32 values: the first two draws of the ray-generation stream, then §4.3"""
    if mutant == "pixel_centre":
        return np.full(W * H, 0.5), np.full(W * H, 0.5)
    pixel = np.arange(W * H, dtype=np.uint32)
    with np.errstate(over="ignore"):
        stage = np.uint32(user_seed) * np.uint32(0x9E3779B9) + np.uint32(seed_counter)
        state = pcg(pixel ^ pcg(stage ^ np.uint32(TAG_RAYGEN)))
        out = []
        for _ in range(2):
            state = state * np.uint32(747796405) + np.uint32(2891336453)
            w = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
            w = (w >> np.uint32(22)) ^ w
            out.append((w >> np.uint32(8)).astype(np.float64) * U)
    if noise is not None:
        nz = np.asarray(noise, np.uint8)
        y, x = np.divmod(np.arange(W * H), W)
        tex = nz[y % nz.shape[0], x % nz.shape[1]]
        g = F(int(seed_counter) & 1023) * F(0.61803398875)
        for c in range(2):
            a = (out[c].astype(F) + (tex[:, c].astype(F) + F(0.5)) / F(256)) + g
            out[c] = (a - np.floor(a)).astype(np.float64)
    return out[0], out[1]


# ------------------------------------------------------------------ §11 camera
class Basis:
    """`(origin, right, up, fwd, ax, ay)`, the build's representation of model_to_screen (§15.1)"""

    def __init__(self, origin, right, up, fwd, ax, ay):
        self.origin, self.right, self.up, self.fwd = (np.asarray(v, np.float64) for v in (origin, right, up, fwd))
        self.ax, self.ay = float(ax), float(ay)


IDENTITY = Basis((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, 1.0)


def basis(view, W, H, vfov, mutant=None):
    v = np.asarray(view, np.float64).reshape(16)
    th = math.tan(float(F(vfov))) if mutant == "tan_full" else math.tan(0.5 * float(F(vfov)))
    ax, ay = (W / H) * th, th
    if mutant == "aspect_on_ay":
        ax, ay = th, (W / H) * th
    return Basis(v[12:15], v[0:3], v[4:7], v[8:11], ax, ay)


def primary_rays(cam, W, H, jx, jy, mutant=None):
    y, x = np.divmod(np.arange(W * H), W)
    sx, sy = (x + jx) / W, (y + jy) / H
    cx = (2.0 * sx - 1.0) * cam.ax
    cy = ((2.0 * sy - 1.0) if mutant == "cy_not_flipped" else (1.0 - 2.0 * sy)) * cam.ay
    d = cam.right[None] * cx[:, None] + cam.up[None] * cy[:, None] + cam.fwd[None]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def project(c, P, dP):
    """§15.1 `project`: (u, v), their first-order binary32 bounds and `cz`, its bound.  Terms: w = P − o (dP + u|w|); a dot product
    (Σ|basis_i|·dw_i + 3u·Σ|w_i·basis_i|); q = cx/(cz·a): dcx/|cz·a| + |q|·(dcz/|cz| + 6u) — the product, the quotient and the 4u of
    a binary32 `a` (K_D); 0.5 ± 0.5·q: 0.5·dq + u·|result|."""
    w = P - c.origin[None]
    dw = dP + U * np.abs(w)

    def dot(b):
        return w @ b, dw @ np.abs(b) + 3.0 * U * (np.abs(w) @ np.abs(b))

    cz, dcz = dot(c.fwd)
    cx, dcx = dot(c.right)
    cy, dcy = dot(c.up)
    with np.errstate(divide="ignore", invalid="ignore"):
        qx, qy = cx / (cz * c.ax), cy / (cz * c.ay)
        dqx = dcx / np.abs(cz * c.ax) + np.abs(qx) * (dcz / np.abs(cz) + 6.0 * U)
        dqy = dcy / np.abs(cz * c.ay) + np.abs(qy) * (dcz / np.abs(cz) + 6.0 * U)
    uu, vv = 0.5 + 0.5 * qx, 0.5 - 0.5 * qy
    return uu, vv, 0.5 * dqx + U * np.abs(uu), 0.5 * dqy + U * np.abs(vv), cz, dcz


# ------------------------------------------------------------------ scene data
class SceneData:
    """World-space triangles (§2.5's baked soup: 3 vertices per triangle with position|u, normal|v), one material id per triangle,
    the materials, rectangle lights and images — data only, as the loader or `add_mesh` produced it."""

    def __init__(self, tri_verts, tri_material, materials, lights, images):
        tv = np.asarray(tri_verts).reshape(-1, 3)
        self.p = tv["position"][..., :3].astype(np.float64)     # (T, 3, 3)
        self.n = tv["normal"][..., :3].astype(np.float64)
        self.uv = np.stack([tv["position"][..., 3], tv["normal"][..., 3]], -1).astype(np.float64)   # (T, 3, 2)
        self.mat = np.asarray(tri_material, np.int64)
        self.materials = materials
        self.lights = lights
        self.images = [np.asarray(i, np.uint8) for i in images]
        e1, e2 = self.p[:, 1] - self.p[:, 0], self.p[:, 2] - self.p[:, 0]
        self.e1, self.e2 = e1, e2
        self.ng = np.cross(e1, e2)
        # §6: rows of [e1 e2 n]^-1 with r.w = −r·p0
        det = np.sum(self.ng * self.ng, axis=1, keepdims=True)
        rows = [np.cross(e2, self.ng) / det, np.cross(self.ng, e1) / det, self.ng / det]
        self.rows = [np.concatenate([r, -np.sum(r * self.p[:, 0], axis=1, keepdims=True)], axis=1) for r in rows]


def srgb_to_linear(b):
    c = np.asarray(b, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def albedo_texture(img, tu, tv):
    """§9: bilinear, repeat, sRGB -> linear for rgb: the value (N, 3) and its largest change per texel step in x and in y (N, 3)"""
    h, w = img.shape[:2]
    lin = srgb_to_linear(img[..., :3])
    fx, fy = tu * w - 0.5, tv * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    c00, c10 = lin[y0 % h, x0 % w], lin[y0 % h, (x0 + 1) % w]
    c01, c11 = lin[(y0 + 1) % h, x0 % w], lin[(y0 + 1) % h, (x0 + 1) % w]
    top, bot = c00 * (1 - tx) + c10 * tx, c01 * (1 - tx) + c11 * tx
    gx = np.maximum(np.abs(c10 - c00), np.abs(c11 - c01))
    gy = np.maximum(np.abs(c01 - c00), np.abs(c11 - c10))
    return top * (1 - ty) + bot * ty, gx, gy, fx, fy


# ------------------------------------------------------------------ the primary hit, brute force
def intersect(sc, o, d):
    """closest hit of every ray `o + t·d` (§7: smaller t, equal t -> smaller prim id; §8: a rectangle must be strictly nearer):
    prim (uint32), t, u, v and the edge distance defined in the module docstring"""
    N = d.shape[0]
    # Möller-Trumbore, two-sided, all rays x all triangles
    pvec = np.cross(d[:, None, :], sc.e2[None])
    det = np.sum(sc.e1[None] * pvec, axis=2)
    tvec = (o[None] - sc.p[:, 0])[None]
    qvec = np.cross(tvec, sc.e1[None])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.sum(tvec * pvec, axis=2) / det
        v = np.sum(d[:, None, :] * qvec, axis=2) / det
        t = np.sum(sc.e2[None] * qvec, axis=2) / det
    margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
    ok = np.isfinite(t) & (t > 0)
    hit = ok & (margin >= 0)
    th = np.where(hit, t, np.inf)
    best = np.argmin(th, axis=1)            # the first of equal minima: the smaller prim id
    tb = th[np.arange(N), best]
    prim = np.where(np.isfinite(tb), best, INVALID).astype(np.uint32)
    bu, bv = u[np.arange(N), best], v[np.arange(N), best]
    # rectangles (§8)
    lm, lt, lok = [], [], []
    for k in range(sc.lights.shape[0]):
        L = sc.lights[k]
        n, tg, bt, c = (np.asarray(L[f][:3], np.float64) for f in ("normal", "tangent", "bitangent", "origin"))
        hw, hh = float(L["tangent"][3]), float(L["bitangent"][3])
        dn = d @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            tl = ((c - o) @ n) / dn
        p = o[None] + d * tl[:, None]
        a, b = (p - c[None]) @ tg, (p - c[None]) @ bt
        m = np.minimum(1.0 - np.abs(a) / hw, 1.0 - np.abs(b) / hh)
        front = (dn < 0) & np.isfinite(tl) & (tl > 0)
        take = front & (m >= 0) & (tl < tb)
        prim = np.where(take, np.uint32(LIGHT_BIT | k), prim).astype(np.uint32)
        bu, bv = np.where(take, 0.0, bu), np.where(take, 0.0, bv)
        tb = np.where(take, tl, tb)
        lm.append(m); lt.append(tl); lok.append(front)
    # edge distance
    near = tb * (1.0 + 1e-5)
    cand = ok & (t <= near[:, None])
    edge = np.min(np.where(cand, np.abs(margin), np.inf), axis=1)
    second = np.sum(hit & (t >= (tb * (1.0 - 1e-5))[:, None]) & (t <= near[:, None]), axis=1)
    for m, tl, front in zip(lm, lt, lok):
        c = front & (tl <= near)
        edge = np.minimum(edge, np.where(c, np.abs(m), np.inf))
        second = second + (c & (m >= 0) & (tl >= tb * (1.0 - 1e-5)))
    edge = np.where(second > 1, 0.0, edge)
    return prim, tb, bu, bv, edge


def hit_bounds(sc, o, d, prim, t):
    """first-order binary32 bounds (dt, du, dv) of §7's test for the triangle hits (0 elsewhere).  A row product r·o + r.w accumulates
    the rounding of the row (§6: once) and of three fma, <= 5u·(Σ|r_i·o_i| + |r.w|); r·d likewise plus Σ|r_i|·K_D·u for the direction;
    t = −oz/dz: t·(doz/|oz| + ddz/|dz| + u); u = fma(t, dx, ox): |dx|·dt + t·ddx + dox + u·(|t·dx| + |ox|)."""
    tri = (prim & LIGHT_BIT) == 0
    k = np.where(tri, prim, 0).astype(np.int64)
    ao, ad = np.abs(o)[None], np.abs(d)

    def terms(r):
        r = r[k]
        vo = r[:, :3] @ o + r[:, 3]
        vd = np.sum(r[:, :3] * d, axis=1)
        do_ = 5.0 * U * (np.sum(np.abs(r[:, :3]) * ao, axis=1) + np.abs(r[:, 3]))
        dd_ = 5.0 * U * np.sum(np.abs(r[:, :3]) * ad, axis=1) + np.sum(np.abs(r[:, :3]), axis=1) * K_D * U
        return vo, vd, do_, dd_

    oz, dz, doz, ddz = terms(sc.rows[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = np.abs(t) * (doz / np.abs(oz) + ddz / np.abs(dz) + U)
        out = [dt]
        for r in sc.rows[:2]:
            ox, dx, dox, ddx = terms(r)
            out.append(np.abs(dx) * dt + np.abs(t) * ddx + dox + U * (np.abs(t * dx) + np.abs(ox)))
    return [np.where(tri, x, 0.0) for x in out]


# ------------------------------------------------------------------ §15.1 packing
def oct_project(n):
    """p = n.xy/(|x| + |y| + |z|), folded for z < 0 (sign(0) = +1)"""
    l1 = np.sum(np.abs(n), axis=1)
    px, py = n[:, 0] / l1, n[:, 1] / l1
    fold = n[:, 2] < 0
    tx = (1.0 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0)
    ty = (1.0 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0)
    return np.where(fold, tx, px), np.where(fold, ty, py), px, py


def oct_decode(word):
    """§15.1 decode in binary64: f = u16·(2/65535) − 1, z = (1 − |x|) − |y|, folded for z < 0, normalised"""
    word = np.asarray(word, np.uint32)
    fx = (word & 0xFFFF).astype(np.float64) * (2.0 / 65535.0) - 1.0
    fy = (word >> 16).astype(np.float64) * (2.0 / 65535.0) - 1.0
    fz = (1.0 - np.abs(fx)) - np.abs(fy)
    fold = fz < 0
    tx = (1.0 - np.abs(fy)) * np.where(fx >= 0, 1.0, -1.0)
    ty = (1.0 - np.abs(fx)) * np.where(fy >= 0, 1.0, -1.0)
    v = np.stack([np.where(fold, tx, fx), np.where(fold, ty, fy), fz], -1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def normal_code_bound(en):
    """Bound of the projected normal p in binary32, given the bound `en` per component of the unit normal: l1 = |x| + |y| + |z| >= 1
    moves by <= 3·en + 2u, p = n/l1 by <= (en + |p|·dl1)/l1 + u <= 4·en + 3u; the fold one more rounding, p·0.5 + 0.5, ·65535 and + 0.5
    three more on values <= 1 -> 4·en + 10u in units of p (a code is 65535/2 of them)."""
    return 4.0 * en + 10.0 * U


# the angle between the decoded code and the encoded normal: each axis of p is off by at most d = 1/65535 (half a step) + the bound
# above; the unnormalised decode v = (x, y, 1 − |x| − |y|) then moves by <= d·√(1 + 1 + 4) = d·√6, and |v| >= 1/√3 (its L1 norm is 1),
# so the angle is <= d·√18 to first order.
def angle_bound(ep):
    return math.sqrt(18.0) * (1.0 / 65535.0 + ep)


# ------------------------------------------------------------------ one frame of the reference
class Frame:
    """what the primary pass must have written for one frame: per pixel (row-major) the expected values and their bounds"""


def reference_frame(sc, W, H, view, vfov, prev, user_seed, seed_counter, noise=None, mutant=None):
    """-> (Frame, this frame's Basis: the next frame's `prev`).  `prev` is None before the first frame."""
    cam = basis(view, W, H, vfov, mutant)
    jx, jy = jitter(W, H, user_seed, seed_counter, noise, mutant)
    d = primary_rays(cam, W, H, jx, jy, mutant)
    o = cam.origin
    N = W * H
    prim, t, u, v, edge = intersect(sc, o, d)
    miss = prim == INVALID
    emit = ~miss & ((prim & LIGHT_BIT) != 0)
    surf = ~miss & ~emit
    dt, du, dv = hit_bounds(sc, o, d, prim, t)
    DD = K_D * U
    f = Frame()
    f.mutant = mutant
    f.W, f.H, f.prim, f.edge, f.miss, f.emit, f.surf = W, H, prim, edge, miss, emit, surf
    # ---- hit point
    k = np.where(surf, prim, 0).astype(np.int64)
    bw = 1.0 - u - v
    P = sc.p[k, 0] * bw[:, None] + sc.p[k, 1] * u[:, None] + sc.p[k, 2] * v[:, None]
    dP = (np.abs(sc.e1[k]) * du[:, None] + np.abs(sc.e2[k]) * dv[:, None]
          + 4.0 * U * (np.abs(sc.p[k, 0]) * np.abs(bw)[:, None] + np.abs(sc.p[k, 1]) * np.abs(u)[:, None] + np.abs(sc.p[k, 2]) * np.abs(v)[:, None]))
    tf = np.where(miss, 0.0, t)
    Pl = o[None] + d * tf[:, None]
    # emitter (§8): t = dot(c − o, n)/dn -> 4u·Σ|(c − o)_i·n_i| / |num| + (3u·Σ|d_i·n_i| + Σ|n_i|·K_D·u)/|dn| + u, relative
    for li in range(sc.lights.shape[0]):
        m = emit & ((prim & ~np.uint32(LIGHT_BIT)) == li)
        n, c = np.asarray(sc.lights[li]["normal"][:3], np.float64), np.asarray(sc.lights[li]["origin"][:3], np.float64)
        num, dn = float((c - o) @ n), d @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = 4.0 * U * float(np.abs(c - o) @ np.abs(n)) / abs(num) + (3.0 * U * (np.abs(d) @ np.abs(n)) + np.sum(np.abs(n)) * DD) / np.abs(dn) + U
        dt = np.where(m, t * rel, dt)
    dPl = np.abs(d) * dt[:, None] + tf[:, None] * DD + U * np.abs(Pl)      # P = fma(d, t, o)
    P, dP = np.where(surf[:, None], P, Pl), np.where(surf[:, None], dP, dPl)
    f.P = P
    # ---- depth
    f.t, f.dt = t, dt
    if mutant == "depth_along_fwd":
        f.t = t * (d @ cam.fwd)
    # ---- normal
    ng = sc.ng[k] / np.linalg.norm(sc.ng[k], axis=1, keepdims=True)
    f.back = surf & (np.sum(ng * d, axis=1) > 0)                # seen from its back: the winding's normal points along the ray
    ngf = np.where(f.back[:, None], -ng, ng)
    ns_un = sc.n[k, 0] * bw[:, None] + sc.n[k, 1] * u[:, None] + sc.n[k, 2] * v[:, None]
    ln = np.linalg.norm(ns_un, axis=1)
    ns = ns_un / ln[:, None]
    flip = np.sum(ns * ngf, axis=1) < 0
    f.flip_margin = np.where(surf, np.minimum(np.abs(np.sum(ng * d, axis=1)), np.abs(np.sum(ns * ngf, axis=1))), np.inf)
    if mutant != "normal_not_flipped":
        ns = np.where(flip[:, None], -ns, ns)
    if mutant == "geometric_normal":
        ns = ngf
    dvec = np.abs(sc.n[k, 1] - sc.n[k, 0]) * du[:, None] + np.abs(sc.n[k, 2] - sc.n[k, 0]) * dv[:, None] + 4.0 * U
    en_s = 2.0 * np.linalg.norm(dvec, axis=1) / ln + 6.0 * U      # interpolation, then v·(1/√(v·v)): 6 roundings
    nrm = np.where(surf[:, None], ns, (d if mutant == "miss_normal_plus_d" else -d))
    en = np.where(surf, en_s, DD)
    for li in range(sc.lights.shape[0]):
        m = emit & ((prim & ~np.uint32(LIGHT_BIT)) == li)
        nrm = np.where(m[:, None], np.asarray(sc.lights[li]["normal"][:3], np.float64)[None], nrm)
        en = np.where(m, 0.0, en)
    f.n = nrm
    f.px, f.py, raw_x, raw_y = oct_project(nrm)
    f.ep = normal_code_bound(en)
    # where the fold's sign choice is within the bound of flipping (a component of p within ep of 0 under z < 0) the two codes may lie
    # on opposite borders of the square, both decoding to the same normal: there only the angle is compared
    f.axis_ok = ~((nrm[:, 2] < f.ep) & (((np.abs(raw_x) <= f.ep) & (raw_x != 0)) | ((np.abs(raw_y) <= f.ep) & (raw_y != 0))))
    f.code_shift = -0.5 if mutant == "trunc_u16" else 0.0
    # ---- albedo
    alb = np.ones((N, 3))
    dalb = np.zeros((N, 3))
    mats = sc.materials[sc.mat[k]]
    base = mats["color"][:, :3].astype(np.float64)
    tu = sc.uv[k, 0, 0] * bw + sc.uv[k, 1, 0] * u + sc.uv[k, 2, 0] * v
    tv = sc.uv[k, 0, 1] * bw + sc.uv[k, 1, 1] * u + sc.uv[k, 2, 1] * v
    auv = [np.abs(sc.uv[k, 0, c] * bw) + np.abs(sc.uv[k, 1, c] * u) + np.abs(sc.uv[k, 2, c] * v) for c in range(2)]
    dtu = np.abs(sc.uv[k, 1, 0] - sc.uv[k, 0, 0]) * du + np.abs(sc.uv[k, 2, 0] - sc.uv[k, 0, 0]) * dv + 4.0 * U * auv[0]
    dtv = np.abs(sc.uv[k, 1, 1] - sc.uv[k, 0, 1]) * du + np.abs(sc.uv[k, 2, 1] - sc.uv[k, 0, 1]) * dv + 4.0 * U * auv[1]
    val, dval = base.copy(), np.zeros((N, 3))
    for ti in np.unique(mats["albedo_texture"]):
        if ti >= len(sc.images) or mutant == "albedo_no_texture":
            continue
        m = mats["albedo_texture"] == ti
        img = sc.images[int(ti)]
        tex, gx, gy, fx, fy = albedo_texture(img, tu[m], tv[m])
        # fx = tu·W − 0.5 moves by W·dtu + 2u·|fx|, the weights with it: |d tex/d fx| <= gx; the three lerps add 6u·tex, the LUT entry u
        dtex = gx * (img.shape[1] * dtu[m] + 2.0 * U * np.abs(fx))[:, None] + gy * (img.shape[0] * dtv[m] + 2.0 * U * np.abs(fy))[:, None] + 7.0 * U * tex
        val[m] = base[m] * tex
        dval[m] = np.abs(base[m]) * dtex + U * np.abs(val[m])
    if mutant != "albedo_unclamped":
        val = np.clip(val, 0.0, 1.0)
    alb[surf], dalb[surf] = val[surf], dval[surf]
    if mutant == "emitter_albedo_light":
        for li in range(sc.lights.shape[0]):
            m = emit & ((prim & ~np.uint32(LIGHT_BIT)) == li)
            alb[m] = np.clip(float(sc.lights[li]["origin"][3]), 0.0, 1.0)
    f.alb, f.dalb = alb, dalb
    f.alb_half = 0.0 if mutant == "trunc_u8" else 0.5
    # ---- motion
    pc = cam
    if prev is None:
        pv = cam if mutant == "no_identity_start" else IDENTITY
    else:
        pv = prev
    if mutant == "prev_is_cur":
        pv = cam
    if mutant == "prev_keeps_axay":
        pv = Basis(pv.origin, pv.right, pv.up, pv.fwd, cam.ax, cam.ay)
    cu, cv, dcu, dcv, czc, dczc = project(pc, P, dP)
    pu, pvv, dpu, dpv, czp, dczp = project(pv, P, dP)
    if mutant == "motion_no_half":
        cu, cv, pu, pvv = 2.0 * cu - 1.0, 1.0 - 2.0 * cv, 2.0 * pu - 1.0, 1.0 - 2.0 * pvv
    mu, mv = pu - cu, pvv - cv
    if mutant == "motion_cur_minus_prev":
        mu, mv = -mu, -mv
    if mutant == "motion_pixels":
        mu, mv = mu * W, mv * H
    behind = ~miss & ~(czp > 1e-6)
    valid = ~miss & (czc > 1e-6) & ((czp > 1e-6) | (mutant == "motion_behind_prev"))
    with np.errstate(invalid="ignore"):
        f.motion = np.where(valid[:, None], np.stack([mu, mv], -1), 0.0)
        f.dmotion = np.where(valid[:, None], np.stack([dpu + dcu + U * np.abs(mu), dpv + dcv + U * np.abs(mv)], -1), 0.0)
    f.behind = behind
    # the `cz > 1e-6` decisions must not hang on rounding for a pixel that is compared
    f.cz_margin = np.where(miss, np.inf, np.minimum(np.abs(czc - 1e-6) - dczc, np.abs(czp - 1e-6) - dczp))
    # ---- self-consistency, without a tolerance: the hit point projects back into its own pixel
    if mutant is None:
        y, x = np.divmod(np.arange(N), W)
        inside = (np.floor(cu * W) == x) & (np.floor(cv * H) == y)
        assert np.all(inside | miss), "reference: project(cur, P) leaves the pixel at %s" % np.nonzero(~(inside | miss))[0][:8]
    f.compared = edge >= EDGE_EPS
    f.classes = {"surface": surf & ~f.back, "back-face": f.back, "emitter": emit, "miss": miss, "behind-previous-camera": behind}
    return f, cam


# ------------------------------------------------------------------ checking a G-buffer and a motion buffer
def allowed_albedo(f):
    """per channel the byte of the binary64 value, and whether the byte below / above is allowed: the value·255 + 0.5 lies within the
    doubled binary32 bound (255·dalb, and 2u of the product and the sum) of the integer boundary"""
    x = np.clip(f.alb, 0.0, None) * 255.0 + f.alb_half
    e = 2.0 * (255.0 * f.dalb + 2.0 * U * np.abs(x))
    kk = np.floor(x)
    return kk, (x - kk) <= e, (kk + 1.0 - x) <= e


def check(f, gbuf, motion):
    """-> {stage: the largest error / tolerance over the compared pixels} (> 1: beyond the tolerance; inf: a value that must be
    equal is not), for the kernels' or the oracle's (H, W, 4) uint32 G-buffer and (H, W, 2) float32 motion"""
    g = np.asarray(gbuf, np.uint32).reshape(-1, 4)
    m = np.asarray(motion, np.float32).reshape(-1, 2).astype(np.float64)
    c = f.compared
    if f.mutant is None:        # the scene and the cameras keep the decisions of the compared pixels away from rounding
        assert np.all(f.cz_margin[c] > 0), "reference: a compared pixel's `cz > 1e-6` hangs on rounding"
        assert np.all(f.flip_margin[c] > 1e-4), "reference: a compared pixel's normal flip hangs on rounding"
    out = {}
    out["prim"] = 0.0 if np.array_equal(g[c, 0], f.prim[c]) else np.inf
    c = c & (g[:, 0] == f.prim)             # the rest is compared where the primitive is the expected one
    # depth: a miss holds t_max exactly
    tk = g[:, 1].copy().view(np.float32).astype(np.float64)
    hitp = c & ~f.miss
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(tk - f.t) / (2.0 * f.dt)
    out["depth"] = max(float(np.max(r[hitp], initial=0.0)), 0.0 if np.all(g[c & f.miss, 1] == T_MISS.view(np.uint32)) else np.inf)
    # normal: per axis in code units, and the angle
    kx, ky = (g[:, 2] & 0xFFFF).astype(np.float64), (g[:, 2] >> 16).astype(np.float64)
    ex = np.clip(f.px * 0.5 + 0.5, 0.0, 1.0) * 65535.0 + f.code_shift
    ey = np.clip(f.py * 0.5 + 0.5, 0.0, 1.0) * 65535.0 + f.code_shift
    tol = 0.5 + 0.5 * 65535.0 * f.ep
    ca = c & f.axis_ok
    out["normal code"] = float(max(np.max((np.abs(kx - ex) / tol)[ca], initial=0.0), np.max((np.abs(ky - ey) / tol)[ca], initial=0.0)))
    dec = oct_decode(g[:, 2])
    cosang = np.clip(np.sum(dec * f.n, axis=1), -1.0, 1.0)
    sinang = np.linalg.norm(np.cross(dec, f.n), axis=1)
    ang = np.arctan2(sinang, cosang)
    out["normal angle"] = float(np.max((ang / angle_bound(f.ep))[c], initial=0.0))
    # albedo
    kk, lo, hi = allowed_albedo(f)
    got = np.stack([(g[:, 3] >> s) & 0xFF for s in (0, 8, 16)], -1).astype(np.float64)
    ok = (got == kk) | ((got == kk - 1) & lo) | ((got == kk + 1) & hi)
    out["albedo"] = 0.0 if np.all(ok[c]) else np.inf
    # motion
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(m - f.motion) / (2.0 * f.dmotion)
    r = np.where(m == f.motion, 0.0, r)
    r = np.where(np.isnan(r), np.inf, r)
    out["motion"] = float(np.max(r[c], initial=0.0))
    return out


def coverage(f):
    """the share of excluded pixels and, per class, how many pixels of it are compared"""
    return 1.0 - float(np.mean(f.compared)), {k: int(np.sum(v & f.compared)) for k, v in f.classes.items()}


# ------------------------------------------------------------------ debug views (BlitMode GBuffer / MotionVector)
def _bytes(x, e):
    kk = np.floor(x)
    return kk, (x - kk) <= e, (kk + 1.0 - x) <= e


def check_normal_view(rgba, gbuf):
    """`uint8((n·0.5 + 0.5)·255 + 0.5)` of the binary64 decode of the G-buffer's own code; ±1 only where the value lies within the
    binary32 error of the decode (9 roundings on values <= 1, then ·0.5 + 0.5, ·255, + 0.5: 4 more on values <= 256) of a boundary"""
    n = oct_decode(np.asarray(gbuf, np.uint32).reshape(-1, 4)[:, 2])
    x = (n * 0.5 + 0.5) * 255.0 + 0.5
    kk, lo, hi = _bytes(x, 2.0 * (255.0 * 9.0 * U + 4.0 * U * 256.0))
    got = np.asarray(rgba, np.uint8).reshape(-1, 4)[:, :3].astype(np.float64)
    return bool(np.all((got == kk) | ((got == kk - 1) & lo) | ((got == kk + 1) & hi)))


def check_motion_view(rgba, motion, W, H):
    """`clamp(|m|·(W, H)/8)·255`, rounded the same way, of the motion buffer's own values (3 roundings on values <= 256)"""
    m = np.abs(np.asarray(motion, np.float32).reshape(-1, 2).astype(np.float64))
    x = np.clip(m * np.array([W, H]) / 8.0, 0.0, 1.0) * 255.0 + 0.5
    kk, lo, hi = _bytes(x, 2.0 * 3.0 * U * 256.0)
    got = np.asarray(rgba, np.uint8).reshape(-1, 4)[:, :2].astype(np.float64)
    return bool(np.all((got == kk) | ((got == kk - 1) & lo) | ((got == kk + 1) & hi)))


# ------------------------------------------------------------------ the scene and the cameras
SIZES = ((61, 37), (64, 32))        # ragged (compacted ray generation) and whole 32x8 tiles (dense)
BOUNCES = 2
USER_SEED = 7
LIGHT = {"normal": (0.0, -0.6, -0.8, 0.0), "tangent": (1.0, 0.0, 0.0, 0.5), "bitangent": (0.0, 0.8, -0.6, 0.35), "origin": (1.5, 2.75, 2.5, 0.6)}


def texture():
    """8x8 sRGB albedo image: every byte range, 255 included so that base colour 1.6 clamps"""
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (8, 8, 4)).astype(np.uint8)
    img[::3, ::2, 0] = 255
    img[1, 1] = (0, 0, 0, 255)
    return img


def noise_texture():
    return np.random.RandomState(11).randint(0, 256, (16, 16, 4)).astype(np.uint8)


def build_scene(s, add_image, set_light0):
    """The scene, through `add_mesh` / `add_material` / `add_instance` of `s` (the product's Scene or the oracle loader's):
    a tilted textured quad, a coarse smooth-shaded bump, a triangle seen from its back, a strip of facets whose vertex normals sit on
    the octahedral seams, one rectangle light, open sky around.  The camera looks along +z, so that −z is a visible normal."""
    eye = np.eye(4, dtype=np.float32).T.reshape(16)
    # tilted quad, albedo texture, base colour that clamps (1.6) and darkens
    tex = add_image(texture())
    m_tex = s.add_material((1.6, 0.7, 0.25, 1.0), 0.6, 0.0, tex)
    x0, x1, y0, y1 = 0.3, 2.3, 0.0, 2.0
    pos = [(x0, y0, 0.5), (x1, y0, 1.5), (x1, y1, 1.5), (x0, y1, 0.5)]
    nq = np.array([1.0, 0.0, -2.0]) / math.sqrt(5.0)
    b = s.add_mesh(np.array(pos, np.float32), np.tile(nq, (4, 1)).astype(np.float32),
                   np.array([(0.1, 0.2), (1.3, 0.2), (1.3, 1.1), (0.1, 1.1)], np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
    s.add_instance(b, eye, m_tex)
    # bump: 3x3 vertices, the centre pulled towards the camera, vertex normals of a sphere much rounder than the facets
    m_grey = s.add_material((0.5, 0.8, 0.3, 1.0), 0.5, 0.0)
    gx, gy = np.meshgrid(np.array([-2.3, -1.3, -0.3]), np.array([0.0, 1.0, 2.0]))
    gz = np.array([[0.4, 0.2, 0.4], [0.2, -0.6, 0.2], [0.4, 0.2, 0.4]])
    pos = np.stack([gx, gy, gz], -1).reshape(9, 3)
    nb = pos - np.array([-1.3, 1.0, 1.2])
    nb /= np.linalg.norm(nb, axis=1, keepdims=True)
    idx = []
    for j in range(2):
        for i in range(2):
            a = 3 * j + i
            idx += [a, a + 3, a + 1, a + 1, a + 3, a + 4]
    b = s.add_mesh(pos.astype(np.float32), nb.astype(np.float32), None, np.array(idx, np.uint32))
    s.add_instance(b, eye, m_grey)
    # one triangle whose winding (and vertex normals) face away from the camera
    m_back = s.add_material((0.9, 0.2, 0.6, 1.0), 0.5, 0.0)
    nt = np.array([0.0, 0.6, 0.8])
    b = s.add_mesh(np.array([(-0.8, 2.2, 1.0), (0.8, 2.2, 1.0), (0.0, 3.2, 1.2)], np.float32), np.tile(nt, (3, 1)).astype(np.float32), None,
                   np.array([0, 1, 2], np.uint32))
    s.add_instance(b, eye, m_back)
    # seam strip: six facets z = 1 + a·(x − xc) + b·(y − yc), geometric normal ∝ (a, b, −1), vertex normals exactly on a seam
    m_strip = s.add_material((0.3, 0.4, 0.95, 1.0), 0.5, 0.0)
    seams = [((1, 0, 0), 0.5, 0.0), ((-1, 0, 0), -0.5, 0.0), ((0, 1, 0), 0.0, 0.5), ((0, -1, 0), 0.0, -0.5), ((0, 0, -1), 0.0, 0.0), ((0.6, 0.8, 0), 0.3, 0.4)]
    for i, (nrm, a, bb) in enumerate(seams):
        xa, xb, ya, yb = -2.4 + 0.8 * i, -1.6 + 0.8 * i, -0.9, -0.2
        xc, yc = 0.5 * (xa + xb), 0.5 * (ya + yb)
        pos = [(x, y, 1.0 + a * (x - xc) + bb * (y - yc)) for (x, y) in ((xa, ya), (xb, ya), (xb, yb), (xa, yb))]
        b = s.add_mesh(np.array(pos, np.float32), np.tile(np.array(nrm, np.float32), (4, 1)), None, np.array([0, 2, 1, 0, 3, 2], np.uint32))
        s.add_instance(b, eye, m_strip)
    set_light0(LIGHT)


def view_matrix(origin, fwd, roll=0.0):
    """16 floats, columns right, up, fwd, origin (§11), an orthonormal basis rounded to binary32"""
    fwd = np.asarray(fwd, np.float64) / np.linalg.norm(fwd)
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    right, up = math.cos(roll) * right + math.sin(roll) * up, -math.sin(roll) * right + math.cos(roll) * up
    m = np.zeros((4, 4))
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3], m[3, 3] = right, up, fwd, origin, 1.0
    return m.T.reshape(16).astype(np.float32)


ALWAYS = ("surface", "back-face", "emitter", "miss")
# (what the frame is there for, origin, fwd, roll, vfov, the classes it must compare)
SEQUENCE = [
    ("first frame: the previous basis is the identity", (0.0, 1.1, -6.0), (0.0, 0.0, 1.0), 0.0, 0.9, ALWAYS + ("behind-previous-camera",)),
    ("static", (0.0, 1.1, -6.0), (0.0, 0.0, 1.0), 0.0, 0.9, ALWAYS),
    ("translation", (0.3, 1.25, -5.7), (0.0, 0.0, 1.0), 0.0, 0.9, ALWAYS),
    ("yaw", (0.3, 1.25, -5.7), (0.12, 0.0, 1.0), 0.0, 0.9, ALWAYS),
    ("roll about fwd", (0.3, 1.25, -5.7), (0.12, 0.0, 1.0), 0.35, 0.9, ALWAYS),
    ("vfov changed", (0.3, 1.25, -5.7), (0.12, 0.0, 1.0), 0.35, 1.05, ALWAYS),
    ("forward, past the middle of the bump", (0.9, 1.7, -0.2), (0.1, 0.3, 1.0), 0.0, 1.05, ("surface", "emitter", "miss")),
    ("back again: the middle of the bump is behind the previous camera", (0.0, 1.1, -6.0), (0.0, 0.0, 1.0), 0.0, 0.9, ALWAYS + ("behind-previous-camera",)),
    ("static again", (0.0, 1.1, -6.0), (0.0, 0.0, 1.0), 0.0, 0.9, ALWAYS),
]


def frames():
    return [(what, view_matrix(o, fw, roll), float(F(vfov)), need) for what, o, fw, roll, vfov, need in SEQUENCE]


def scene_data():
    """the scene as data, baked by the oracle's loader module (§2.5; data, not arithmetic under test)"""
    from oracle import gltf_oracle as G
    s = G.Scene()
    build_scene(s, lambda img: (s.images.append(img), len(s.images) - 1)[1], lambda l: set_light(s.lights, 0, l))
    tv, tm = G.bake(s)
    return s, SceneData(tv, tm, s.materials, s.lights, s.images)


def set_light(lights, i, l):
    for k, val in l.items():
        lights[k][i] = val


def light_record(dtype):
    l = np.zeros(1, dtype)
    set_light(l, 0, LIGHT)
    return l


class Reference:
    """the reference over a frame sequence: carries the previous basis from frame to frame"""

    def __init__(self, sc, W, H, noise=None, mutant=None):
        self.sc, self.W, self.H, self.noise, self.mutant, self.prev = sc, W, H, noise, mutant, None

    def frame(self, view, vfov, seed_counter, user_seed=USER_SEED):
        f, self.prev = reference_frame(self.sc, self.W, self.H, view, vfov, self.prev, user_seed, seed_counter, self.noise, self.mutant)
        return f
