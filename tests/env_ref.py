"""SPEC.md §18 in float64 numpy: the environment probe's sampling distribution (weights, pdf_uv) and the density p_e of a direction,
the restatement tests/test_env_distribution.py and tests/test_gpu_env_sampling.py check the library against.  The alias tables are
checked through the probabilities they imply (alias_probabilities), not entry by entry: any correct table is acceptable."""
import numpy as np

TWO_PI_SQ = 2.0 * np.pi * np.pi


def decode(rgbe):
    """§9 rgbe_decode in float64: [h, w, 4] uint8 -> [h, w, 3] linear RGB"""
    a = np.asarray(rgbe, np.uint8)
    e = a[..., 3].astype(np.int64)
    scale = np.where(e >= 10, np.ldexp(1.0, (e - 136).astype(np.int32)), 0.0)
    return a[..., :3].astype(np.float64) * scale[..., None]


def luminance(rgb):
    return (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1]) + 0.0722 * rgb[..., 2]


def weights(rgbe):
    """w(x, y): the 3x3 neighbourhood's largest luminance (x wraps, y clamps) times sin(pi (y + 0.5) / H)"""
    lum = luminance(decode(rgbe))
    H, W = lum.shape
    m = np.zeros_like(lum)
    for dy in (-1, 0, 1):
        rows = np.clip(np.arange(H) + dy, 0, H - 1)
        for dx in (-1, 0, 1):
            m = np.maximum(m, np.roll(lum[rows], -dx, axis=1))
    return m * np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None]


def distribution(rgbe):
    """(pdf_uv [h, w], total); pdf_uv is all zero when total == 0 (no distribution)"""
    w = weights(rgbe)
    total = float(w.sum())
    if not total > 0.0:
        return np.zeros_like(w), 0.0
    return w * (w.size / total), total


def alias_probabilities(q, alias):
    """what an alias table picks: P(i) = (q_i + sum over j with alias_j = i of (1 - q_j)) / N"""
    q = np.asarray(q, np.float64)
    n = q.size
    p = q.copy()
    np.add.at(p, np.asarray(alias, np.int64), 1.0 - q)
    return p / n


def uv_of(d):
    """env_lookup's (u, v) of unit directions d [n, 3] (exact functions in place of the polynomial approximations)"""
    d = np.asarray(d, np.float64)
    u = np.arctan2(d[:, 2], d[:, 0]) / (2.0 * np.pi) + 0.5
    v = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
    return u, v


def pdf_e(pdf_uv, d):
    """p_e(d) = pdf_uv(cell of d) / (2 pi^2 sin(theta)); 0 where sin(theta) = 0"""
    H, W = pdf_uv.shape
    d = np.asarray(d, np.float64)
    u, v = uv_of(d)
    cx = np.clip((u * W).astype(np.int64), 0, W - 1)
    cy = np.clip((v * H).astype(np.int64), 0, H - 1)
    s = np.sqrt(np.maximum(0.0, 1.0 - d[:, 1] ** 2))
    out = np.zeros(d.shape[0])
    ok = s > 0
    out[ok] = pdf_uv[cy[ok], cx[ok]] / (TWO_PI_SQ * s[ok])
    return out


def lookup(rgbe, d):
    """env_lookup (bilinear, x wraps, y clamps) in float64 for unit directions d [n, 3] -> [n, 3]"""
    tex = decode(rgbe)
    H, W = tex.shape[:2]
    if W == 1 and H == 1:
        return np.repeat(tex[0, 0][None], len(d), axis=0)
    u, v = uv_of(d)
    fx, fy = u * W - 0.5, v * H - 0.5
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f)[:, None], (fy - y0f)[:, None]
    x0 = np.mod(x0f.astype(np.int64), W)
    x1 = np.mod(x0 + 1, W)
    y0 = np.clip(y0f.astype(np.int64), 0, H - 1)
    y1 = np.clip(y0f.astype(np.int64) + 1, 0, H - 1)
    top = tex[y0, x0] * (1 - tx) + tex[y0, x1] * tx
    bot = tex[y1, x0] * (1 - tx) + tex[y1, x1] * tx
    return top * (1 - ty) + bot * ty


def sphere_grid(n_theta, n_phi):
    """midpoint quadrature over the sphere: (directions [n, 3], solid angle per point [n])"""
    th = (np.arange(n_theta) + 0.5) * np.pi / n_theta
    ph = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi - np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], axis=-1).reshape(-1, 3)
    dw = (np.sin(T) * (np.pi / n_theta) * (2.0 * np.pi / n_phi)).reshape(-1)
    return d, dw
