"""SPEC.md §20 (alpha mask) restated in numpy float32, from the SPEC: every operation below is one binary32 operation, in the order and with the
parentheses the SPEC writes.  Test infrastructure only."""
import numpy as np

F = np.float32
INV255 = F(1.0) / F(255.0)        # SPEC §9: texel -> float through b * (1 / 255)


def interp_uv(uv, hu, hv):
    """the texture coordinate of a hit (u, v) on a triangle whose vertices carry uv[3, 2] (SPEC §20: shade_hit's expression)"""
    uv = np.asarray(uv, F)
    hu, hv = np.asarray(hu, F), np.asarray(hv, F)
    bw = (F(1.0) - hu) - hv
    tu = (uv[0, 0] * bw + uv[1, 0] * hu) + uv[2, 0] * hv
    tv = (uv[0, 1] * bw + uv[1, 1] * hu) + uv[2, 1] * hv
    return tu.astype(F), tv.astype(F)


def tex_alpha(image, tu, tv):
    """SPEC §9's bilinear, repeat lookup of the alpha byte of image[H, W, 4] (uint8) at (tu, tv): never the sRGB table"""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[:2]
    tu, tv = np.asarray(tu, F), np.asarray(tv, F)
    fx = tu * F(W) - F(0.5)
    fy = tv * F(H) - F(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f).astype(F), (fy - y0f).astype(F)
    x0 = np.mod(x0f.astype(np.int64), W)
    y0 = np.mod(y0f.astype(np.int64), H)
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    a = image[..., 3].astype(F)
    c00, c10 = a[y0, x0] * INV255, a[y0, x1] * INV255
    c01, c11 = a[y1, x0] * INV255, a[y1, x1] * INV255
    top = c00 * (F(1.0) - tx) + c10 * tx
    bot = c01 * (F(1.0) - tx) + c11 * tx
    return (top * (F(1.0) - ty) + bot * ty).astype(F)


def alpha(color_w, image, uv, hu, hv):
    """a = color.w, times tex.w where the material has an alpha image (image None: it has none)"""
    hu = np.asarray(hu, F)
    a = np.full(hu.shape, F(color_w), F)
    if image is None:
        return a
    tu, tv = interp_uv(uv, hu, hv)
    return (a * tex_alpha(image, tu, tv)).astype(F)


def counts(a, cutoff):
    """the hit counts iff a >= c"""
    return np.asarray(a, F) >= F(cutoff)
