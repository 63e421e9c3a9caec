"""A binary64 restatement of SPEC.md §22 (emission), written from the SPEC text and not from the kernels (test infrastructure): the material record, §9's
sRGB table and bilinear repeat lookup, the emitted radiance E at a hit, and what a depth-1 frame holds per pixel given the primary hit (prim, u, v) of every pixel.

Only the record's product is binary32 (§22: `Le_c = float32(factor_c) · float32(strength)`, one binary32 product per channel); everything behind it is binary64.
tests/primary_ref.py supplies the camera rays (SPEC §4, §11)."""
import numpy as np

import primary_ref as P

F = np.float32
INVALID = 0xFFFFFFFF


# ------------------------------------------------------------------ §22 material state
def record(factor, strength=1.0, image=None):
    """-> (Le float32[3], image) or None: `Le = 0` in all channels means non-emissive, and the record is dropped whatever the image says"""
    le = np.broadcast_to(np.asarray(factor, F), (3,)) * F(strength)     # float32 x float32 -> one binary32 product per channel
    if not le.any():
        return None
    return le.astype(F), image


# ------------------------------------------------------------------ §9 the sRGB -> linear table and the lookup
def srgb_table():
    """256 entries: the sRGB decode of b / 255 in binary64, rounded to binary32 (the table holds floats)"""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(F).astype(np.float64)


def texels_of(img, tu, tv):
    """§9's taps: (x0, y0) before the wrap and the weights (tx, ty) of the lookup at (tu, tv)"""
    h, w = img.shape[:2]
    fx, fy = np.asarray(tu, np.float64) * w - 0.5, np.asarray(tv, np.float64) * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    return x0.astype(np.int64), y0.astype(np.int64), fx - x0, fy - y0


def lookup(img, tu, tv):
    """§9: bilinear, repeat, rgb through the sRGB table -> (N, 3)"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    lin = srgb_table()[img[..., :3]]
    x0, y0, tx, ty = texels_of(img, tu, tv)
    tx, ty = tx[:, None], ty[:, None]
    c00, c10 = lin[y0 % h, x0 % w], lin[y0 % h, (x0 + 1) % w]
    c01, c11 = lin[(y0 + 1) % h, x0 % w], lin[(y0 + 1) % h, (x0 + 1) % w]
    top, bot = c00 * (1 - tx) + c10 * tx, c01 * (1 - tx) + c11 * tx
    return top * (1 - ty) + bot * ty


def steepest(img):
    """the largest difference between wrapped neighbours of the decoded image, per axis (x, y): the slope of the lookup per texel step is at most this"""
    lin = srgb_table()[np.asarray(img, np.uint8)[..., :3]]
    return float(np.abs(np.roll(lin, -1, 1) - lin).max()), float(np.abs(np.roll(lin, -1, 0) - lin).max())


# ------------------------------------------------------------------ §22 at a hit
def emitted(rec, images, tu, tv):
    """E (N, 3) of an emissive material's record at the texture coordinates (tu, tv): Le, times the image's lookup where there is one"""
    n = np.asarray(tu).shape[0]
    if rec is None:
        return np.zeros((n, 3))
    le, image = rec
    E = np.broadcast_to(le.astype(np.float64), (n, 3)).copy()
    if image is not None and image != INVALID and image < len(images):
        E *= lookup(images[image], tu, tv)
    return E


def camera_rays(view, vfov, W, H, user_seed, seed_counter):
    """the primary rays of one frame in binary64: (origin (3,), directions (H·W, 3))"""
    cam = P.basis(view, W, H, float(F(vfov)))
    jx, jy = P.jitter(W, H, user_seed, seed_counter)
    return cam.origin, P.primary_rays(cam, W, H, jx, jy)


def depth1_frame(prim, u, v, tri_uv, tri_rec, images):
    """the radiance (N, 3) of a depth-1 frame with a black probe and no light: per pixel the primary hit `prim` (INVALID: a miss) with barycentrics (u, v);
    tri_uv[t] = the three vertices' (tu, tv) of triangle t; tri_rec[t] = its material's record or None.  T = 1, so L = E (§22: weight 1, both sides)."""
    prim = np.asarray(prim, np.int64)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    out = np.zeros((prim.shape[0], 3))
    uv = np.asarray(tri_uv, np.float64)
    for t, rec in enumerate(tri_rec):
        m = prim == t
        if rec is None or not m.any():
            continue
        bw = 1.0 - u[m] - v[m]
        tu = uv[t, 0, 0] * bw + uv[t, 1, 0] * u[m] + uv[t, 2, 0] * v[m]
        tv = uv[t, 0, 1] * bw + uv[t, 1, 1] * u[m] + uv[t, 2, 1] * v[m]
        out[m] = emitted(rec, images, tu, tv)
    return out


def hit_uv(prim, u, v, tri_uv):
    """the interpolated texture coordinate of every pixel that hit a triangle (NaN elsewhere)"""
    prim = np.asarray(prim, np.int64)
    uv = np.asarray(tri_uv, np.float64)
    ok = (prim >= 0) & (prim < len(uv))
    k = np.where(ok, prim, 0)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    bw = 1.0 - u - v
    tu = uv[k, 0, 0] * bw + uv[k, 1, 0] * u + uv[k, 2, 0] * v
    tv = uv[k, 0, 1] * bw + uv[k, 1, 1] * u + uv[k, 2, 1] * v
    return np.where(ok, tu, np.nan), np.where(ok, tv, np.nan)
