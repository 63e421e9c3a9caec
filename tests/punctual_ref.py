"""float64 numpy restatement of SPEC.md §19 (punctual lights) and of §10's BSDF for arbitrary base colour / roughness / metallic, written from
the text of the specification alone: no product code is imported.  The GPU tests compare the kernels with this; the CPU tests check it by hand
at its corners."""
import numpy as np

POINT, SPOT, DIRECTIONAL = 0, 1, 2
T_INF = 1.0e30   # the renderer's infinity (the shadow ray of a directional light)


def make(kind, position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), color=(1.0, 1.0, 1.0), intensity=1.0, range=0.0, inner=0.0, outer=np.pi / 4):
    """the record of §19 in float64: position | type, unit direction | range, colour x intensity, (cos outer, 1 / max(cos inner - cos outer, 1e-6));
    the windows a type does not have carry their neutral constants: cone (-2, 1) unless a spot, range 0 for a directional light"""
    d = np.asarray(direction, np.float64)
    n = np.linalg.norm(d)
    d = d / n if n > 0 else d
    cone = (-2.0, 1.0)
    if kind == SPOT:
        cone = (np.cos(outer), 1.0 / max(np.cos(inner) - np.cos(outer), 1e-6))
    return {"type": kind, "position": np.asarray(position, np.float64), "direction": d, "range": 0.0 if kind == DIRECTIONAL else float(range),
            "color": np.asarray(color, np.float64) * float(intensity), "cos_outer": float(cone[0]), "inv_span": float(cone[1])}


def from_record(rec):
    """an lpt_punctual_light record (numpy, PUNCTUAL_DT layout) -> the dictionary `make` returns, every number widened to float64 as stored"""
    rec = np.asarray(rec).reshape(-1)[0]
    p, d, c, k = (np.asarray(rec[n], np.float64) for n in ("position", "direction", "color", "cone"))
    return {"type": int(p[3]), "position": p[:3], "direction": d[:3], "range": float(d[3]), "color": c[:3], "cos_outer": float(k[0]), "inv_span": float(k[1])}


def range_window(d2, r):
    """clamp(1 - (d2 / r^2)^2, 0, 1); r = 0: unlimited"""
    d2 = np.asarray(d2, np.float64)
    if not r > 0:
        return np.ones_like(d2)
    q = d2 / (r * r)
    return np.clip(1.0 - q * q, 0.0, 1.0)


def cone_window(c, cos_outer, inv_span):
    """s^2, s = clamp((c - cos_outer) * inv_span, 0, 1), c = the cosine between the light's axis and the direction light -> point"""
    s = np.clip((np.asarray(c, np.float64) - cos_outer) * inv_span, 0.0, 1.0)
    return s * s


def incident(light, Po):
    """§19 incident term at points Po[n, 3] -> (ok[n], wi[n, 3], dist[n], E[n, 3]); no sample (ok false, zeros) where a point / spot light sits at Po"""
    Po = np.asarray(Po, np.float64).reshape(-1, 3)
    n = Po.shape[0]
    if light["type"] == DIRECTIONAL:
        wi = np.tile(-light["direction"], (n, 1))
        ok = np.ones(n, bool)
        dist = np.full(n, T_INF)
        g = np.ones(n)
    else:
        w = light["position"][None] - Po
        d2 = (w * w).sum(1)
        ok = d2 > 0
        d2s = np.where(ok, d2, 1.0)
        dist = np.sqrt(d2s)
        wi = w / dist[:, None]
        g = (1.0 / d2s) * range_window(d2s, light["range"])
    c = -(wi @ light["direction"])
    g = g * cone_window(c, light["cos_outer"], light["inv_span"])
    E = light["color"][None] * g[:, None]
    z = ~ok
    return ok, np.where(z[:, None], 0.0, wi), np.where(z, 0.0, dist), np.where(z[:, None], 0.0, E)


def pick(n_punctual, n_rect, env):
    """§19 pick: (p_p, the probability of ONE given punctual light, the probability of ONE given rectangle light)"""
    p_env = 0.5 if env else 0.0
    p_p = n_punctual / float(n_punctual + n_rect)
    rest = 1.0 - p_env
    return p_p, rest * p_p / n_punctual, (rest * (1.0 - p_p) / n_rect if n_rect else 0.0)


def luminance(rgb):
    rgb = np.asarray(rgb, np.float64)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def bsdf(base, roughness, metallic, N, Ng, V, L):
    """SPEC §10: f(L)[n, 3] of the metallic-roughness BSDF for unit N, Ng, V and unit directions L[n, 3]; zero unless NoL > 0 and dot(Ng, L) > 0"""
    base, N, Ng, V = (np.asarray(a, np.float64) for a in (base, N, Ng, V))
    L = np.asarray(L, np.float64).reshape(-1, 3)
    r = min(max(float(roughness), 0.045), 1.0)
    m = min(max(float(metallic), 0.0), 1.0)
    alpha = r * r
    a2 = alpha * alpha
    diff = base * (1.0 - m)
    F0 = 0.04 * (1.0 - m) + base * m
    NoV = max(float(N @ V), 1e-4)
    NoL = L @ N
    H = L + V[None]
    hn = np.linalg.norm(H, axis=1, keepdims=True)
    H = H / np.where(hn > 0, hn, 1.0)
    NoH = np.maximum(H @ N, 0.0)
    VoH = np.maximum(H @ V, 0.0)
    D = a2 / (np.pi * ((NoH * NoH) * (a2 - 1.0) + 1.0) ** 2)
    k = alpha / 2.0
    vis = 1.0 / (4.0 * (NoL * (1.0 - k) + k) * (NoV * (1.0 - k) + k))
    F = F0[None] + (1.0 - F0[None]) * ((1.0 - VoH) ** 5)[:, None]
    f = (diff[None] / np.pi) * (1.0 - F) + (D * vis)[:, None] * F
    lit = (NoL > 0) & (L @ Ng > 0)
    return np.where(lit[:, None], f, 0.0)


def radiance(light, P, N, V, base, roughness, metallic, eps_offset=True):
    """outgoing radiance f · NoL · E towards V of surface points P[n, 3] (normal N, geometric normal N) lit by `light`, unoccluded: what a depth-1
    frame's light samples average to (the pick probability cancels).  The light is seen from Po = P + N · 1e-4 (1 + max|P|), as §12 offsets it."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    N = np.asarray(N, np.float64)
    Po = P + N[None] * (1e-4 * (1.0 + np.abs(P).max(1)))[:, None] if eps_offset else P
    ok, wi, _, E = incident(light, Po)
    f = bsdf(base, roughness, metallic, N, N, V, wi)
    return np.where(ok[:, None], f * (wi @ N)[:, None] * E, 0.0)


# ---- SPEC §4: the shading stream's first draw (the light pick r0), for tests that need to know WHICH samples of a pixel picked a punctual light
def _pcg(v):
    v = np.asarray(v, np.uint64)
    s = (v * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
    return ((w >> 22) ^ w) & 0xFFFFFFFF


def r0_of(pixel, seed_counter, user_seed=0):
    """r0 of §4.2 for pixels `pixel` (y·W + x) in the shading stage with seed counter `seed_counter`"""
    stage_seed = (user_seed * 0x9E3779B9 + seed_counter) & 0xFFFFFFFF
    state = _pcg(np.asarray(pixel, np.uint64) ^ _pcg(np.uint64(stage_seed ^ 0)))
    state = (state * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    w = ((w >> 22) ^ w) & 0xFFFFFFFF
    return (w >> 8).astype(np.float64) * 2.0 ** -24
