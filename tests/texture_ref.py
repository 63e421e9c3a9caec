"""SPEC.md §9 in binary64 numpy: the texture lookup (bilinear, repeat), the texture pair, §20's alpha value, §12's interpolation of the texture coordinate and the
environment lookup, each with a DERIVED bound on what a binary32 evaluation may differ by; the images, probes, coordinates and directions every implementation is run
over; and the named wrong variants (`MUTANTS`) the checker must reject.  Data and numpy only: nothing of the product or the oracle is imported.
tests/test_texture_reference.py holds the oracle to it, tests/test_gpu_texture_reference.py the device.

The binary32 evaluation (SPEC §9), per axis:  fx = fl(fl(u·W) − ½),  x0f = floor(fx),  tx = fl(fx − x0f),  x0 = wrap(sat(x0f)),  x1 = the texel after x0, wrapped;
per channel  top = fl(fl(c00·fl(1 − tx)) + fl(c10·tx)),  bot likewise,  out = fl(fl(top·fl(1 − ty)) + fl(bot·ty)).   u = 2⁻²⁴ below.

Bound of a lookup = value term + position term.

  Value term K·u·max|c| over the four taps.  Every rounding is relative (u times the rounded number) and every rounded number is at most max|c|(1 + O(u)): the weights lie
  in [0, 1] and sum to 1.  `top` takes four roundings: fl(1 − tx), two products, one sum.  The first is worth u·|c00| (the weight's error times the tap), the two products
  together u·(|c00|(1 − tx) + |c10|·tx) ≤ u·max|c|, the sum u·max|c|: 3 u·max|c| — we count each rounding as one, 4.  `bot` has the same error, and `out` weighs the two by
  (1 − ty) and ty, so it inherits max(top, bot) = 4, not their sum, and adds its own four: K = 8.  (Eleven roundings happen — fl(1 − tx) is shared —; 8 is the longest chain
  of them that one result sees, each counted at its largest.)  An axis whose binary32 weight is exactly 0 takes no rounding at all — 1 − 0 = 1, c·1 = c, c·0 = 0, c + 0 = c —
  so it contributes 0 instead of 4: K = Kx + Ky with Kx, Ky in {0, 4}.  Where both weights are 0 the bound is 0 and the result is the tap itself, the table entry or
  fl(b·fl(1/255)), bit for bit: the EXACT rows.  Products that underflow add at most 8·2⁻¹⁴⁹ (never the case for texels, possible for a probe's smallest exponents).

  Position term gx·δfx + gy·δfy.  The device filters at the position (x0f + tx, y0f + ty), which differs from the exact (u·W − ½, v·H − ½) by the roundings of fl(u·W),
  of the subtraction and of tx:  δfx = ½ulp(u·W) + ½ulp(fx) + u  (≤ u·(|u·W| + |fx| + 1)).  The filter is continuous and piecewise linear with slope at most the texel step, so the value moves by at
  most gx·δfx, gx = the largest step |c(x + 1, y) − c(x, y)| over the 3x3 cells around the exact cell (4x4 texels, wrapped) — which covers a binary32 position that falls
  into the neighbouring cell (δ ≤ 1 wherever the binary32 fx is not an integer, i.e. below 2²³).  In that case the device's taps are the neighbour's, whose largest is at most
  max|c| + gx + gy, hence the K·u inside the brackets of  bound = K·u·max|c| + gx·(δfx + K·u) + gy·(δfy + K·u).
  An axis whose binary32 fx is an integer is pinned: its position is that integer (saturated, wrapped), δ = 0, whatever the exact u·W is — beyond 2²⁴ the binary32 product
  moves by whole texels and "the exact coordinate" names another texel, so SPEC §9 defines the lookup on the binary32 fx there, and so does this reference.

Environment: u = atan2(d.z, d.x)/(2π) + ½, v = acos(clamp(d.y))/π with exact functions (atan2(0, 0) = 0: u = ½ at the poles); δfx carries SPEC §5's polynomial error,
3·10⁻⁴ rad = W·3e-4/(2π) texels, and five binary32 roundings worth at most W each plus tx's (φ·fl(1/2π) with the constant's own rounding, + ½, ·W, − ½): u·(5W + 1); δfy
carries 10⁻⁴ rad = H·1e-4/π texels and u·(4H + 1).  No axis is ever pinned (the binary32 fx is the polynomial's), so K = 8 throughout; x wraps, y clamps."""
import numpy as np

import env_ref

U = 2.0 ** -24
F = np.float32
TINY = 8.0 * 2.0 ** -149
INV255 = F(0.003921568859368563)
ATAN_ERR, ACOS_ERR = 3.0e-4, 1.0e-4          # SPEC §5

MUTANTS = {
    "clamp": "coordinates clamp to the image instead of repeating",
    "x1_is_x0": "the second column is the first again",
    "no_half_texel": "fx = u·W without the half-texel offset",
    "weights_swapped": "tx and ty exchanged",
    "srgb_after_filter": "the bytes are filtered first and sRGB-decoded after",
    "mra_g_b_swapped": "the pair returns mra b for g and g for b",
    "tile_stride_floor": "the atlas is read with W // 8 tiles per row instead of ceil(W / 8)",
    "apron_column": "an apron tile's columns beyond the image's right border are not wrapped: the neighbour across it reads as 0",
    "apron_row": "an apron tile's rows beyond the image's lower border are not wrapped: the neighbour across it reads as 0",
    "env_v_wraps": "the probe's v wraps instead of clamping",
    "env_u_no_half": "the probe's u without the + ½",
}
TEXTURE_MUTANTS = [m for m in MUTANTS if not m.startswith("env_")]
ENV_MUTANTS = [m for m in MUTANTS if m.startswith("env_")]


def _srgb_table():
    b = np.arange(256, dtype=np.float64) / 255.0
    return np.where(b <= 0.04045, b / 12.92, ((b + 0.055) / 1.055) ** 2.4).astype(F)


SRGB_LUT = _srgb_table()
LINEAR_LUT = (np.arange(256).astype(F) * INV255).astype(F)        # fl(float(b)·fl(1/255))


def _srgb_f64(x):
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def texel_values(b, srgb):
    """bytes [..., 4] -> the binary32 values a tap has, as float64: rgb through the table where srgb, everything else through b·(1/255)"""
    b = np.asarray(b, np.uint8)
    out = LINEAR_LUT[b].astype(np.float64)
    if srgb:
        out[..., :3] = SRGB_LUT[b[..., :3]]
    return out


# ------------------------------------------------------------------ the two storage layouts (the mutants that misread them need a model of them)
def store_atlas(img):
    """8x4-texel tiles, ceil(W / 8) per row -> (flat [tiles · 32, 4], tiles per row)"""
    H, W = img.shape[:2]
    tx, ty = (W + 7) // 8, (H + 3) // 4
    flat = np.zeros((tx * ty * 32, 4), np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    flat[((y >> 2) * tx + (x >> 3)) * 32 + (y & 3) * 8 + (x & 7)] = img
    return flat, tx


def fetch_atlas(flat, tiles_x, x, y):
    return flat[(y >> 2) * tiles_x * 32 + (y & 3) * 8 + (x >> 3) * 32 + (x & 7)]


def store_apron(img, mutant=None):
    """4x4 stored texels per 3x3 block, the right / lower neighbours wrapped in -> [ty, tx, 4, 4, 4]"""
    H, W = img.shape[:2]
    tx, ty = (W + 2) // 3, (H + 2) // 3
    tj, ti, j, i = np.mgrid[0:ty, 0:tx, 0:4, 0:4]
    x, y = 3 * ti + i, 3 * tj + j
    t = img[y % H, x % W].copy()
    if mutant == "apron_column":
        t[x >= W] = 0
    if mutant == "apron_row":
        t[y >= H] = 0
    return t


def fetch_apron(tiles, x0, y0, dx, dy):
    """the tap (x0 + dx, y0 + dy), dx, dy in {0, 1}, of the lookup whose upper-left texel is (x0, y0) (wrapped into the image)"""
    return tiles[y0 // 3, x0 // 3, y0 % 3 + dy, x0 % 3 + dx]


# ------------------------------------------------------------------ the lookup
def _axis(t, n, mutant, half=True):
    """one axis of §9 for binary32 coordinates t and size n -> (position (float64), delta, K of the axis, pinned)"""
    t32 = np.asarray(t, F)
    h32, h64 = (F(0.5), 0.5) if half else (F(0.0), 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        f32 = (t32 * F(n)) - h32                               # two binary32 roundings
        t32w = f32 - np.floor(f32)                             # one more
    pinned = t32w == 0
    tn = t32.astype(np.float64) * n
    exact = tn - h64
    with np.errstate(over="ignore"):
        e1 = np.where(tn.astype(F) == tn, 0.0, _half_ulp(tn))                                               # a representable product is not rounded
        e2 = np.where((e1 == 0) & (exact.astype(F) == exact), 0.0, _half_ulp(np.abs(exact) + e1))
    delta = np.where(pinned, 0.0, e1 + e2 + U + 2.0 ** -52 * (np.abs(tn) + 1.0))
    assert np.all(delta <= 1.0), "a binary32 fx that is not an integer lies below 2^23: half an ulp is at most 1/4"
    return np.where(pinned, f32.astype(np.float64), exact), delta, np.where(pinned, 0.0, 4.0), pinned


def _half_ulp(x):
    """half a binary32 ulp of |x| (normal range): the largest rounding error of a result whose exact value is x"""
    return np.ldexp(1.0, np.frexp(np.maximum(np.abs(x), 2.0 ** -126))[1] - 25)


def _sat(f):
    """floor(position) saturated to the int32 range"""
    return np.clip(np.floor(f), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _bilinear(tex, px, py, dx, dy, K, second):
    """tex(ix, iy, which) -> [n, C] float64 for integer texel coordinates (any integers: tex wraps or clamps them); `which` names the tap (dx, dy) or None for the
    neighbourhood.  second(i0) -> the index of the texel after i0 on x (the mutants change it).  -> (value, bound)"""
    x0, y0 = _sat(px), _sat(py)
    tx, ty = (px - np.floor(px))[:, None], (py - np.floor(py))[:, None]
    c00, c10, c01, c11 = tex(x0, y0, (0, 0)), tex(second(x0), y0, (1, 0)), tex(x0, y0 + 1, (0, 1)), tex(second(x0), y0 + 1, (1, 1))
    value = (c00 * (1 - tx) + c10 * tx) * (1 - ty) + (c01 * (1 - tx) + c11 * tx) * ty
    M = np.max(np.abs(np.stack([c00, c10, c01, c11])), axis=0)
    nb = np.stack([np.stack([tex(x0 - 1 + i, y0 - 1 + j, None) for i in range(4)]) for j in range(4)])      # [j, i, n, C]
    gx = np.max(np.abs(nb[:, 1:] - nb[:, :-1]), axis=(0, 1))
    gy = np.max(np.abs(nb[1:] - nb[:-1]), axis=(0, 1))
    Ku = (K * U)[:, None]
    bound = Ku * M + gx * (dx[:, None] + Ku) + gy * (dy[:, None] + Ku)
    return value, np.where(bound > 0, bound + TINY, 0.0)


def lookup(img, tu, tv, srgb, storage="linear", mutant=None):
    """SPEC §9's texture lookup of image [H, W, 4] uint8 at binary32 coordinates (finite, |t·size| representable) -> (rgba [n, 4] float64, bound [n, 4], exact [n]).
    exact: both binary32 weights are 0 — the bound is 0 and the value is the tap's binary32 value.  storage: "linear" reads the image, "atlas" / "apron" read a model of
    the product's two layouts (same texels unless a mutant misreads them)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    half = mutant != "no_half_texel"
    px, dx, kx, pinx = _axis(tu, W, mutant, half)
    py, dy, ky, piny = _axis(tv, H, mutant, half)
    if mutant == "weights_swapped":                 # the weights change places, the cells do not
        fx, fy = np.floor(px), np.floor(py)
        px, py = fx + (py - fy), fy + (px - fx)
    wrap = (lambda i, n: np.clip(i, 0, n - 1)) if mutant == "clamp" else (lambda i, n: np.mod(i, n))
    decode = (lambda b: LINEAR_LUT[b].astype(np.float64)) if mutant == "srgb_after_filter" else (lambda b: texel_values(b, srgb))
    flat, tiles_x = store_atlas(img)
    if mutant == "tile_stride_floor":
        tiles_x = W // 8
    apron = store_apron(img, mutant)

    def tex(ix, iy, which):
        x, y = wrap(ix, W), wrap(iy, H)
        if which is None or storage == "linear":
            return decode(img[y, x])
        if storage == "atlas":
            return decode(fetch_atlas(flat, tiles_x, x, y))
        ddx, ddy = which
        return decode(fetch_apron(apron, wrap(ix - ddx, W), wrap(iy - ddy, H), ddx, ddy))

    second = (lambda i: i) if mutant == "x1_is_x0" else (lambda i: i + 1)
    value, bound = _bilinear(tex, px, py, dx, dy, kx + ky, second)
    if mutant == "srgb_after_filter" and srgb:
        value[:, :3] = _srgb_f64(value[:, :3])
    return value, bound, pinx & piny


def pair(albedo, mra, tu, tv, storage="linear", mutant=None):
    """what the shading reads of a material's two textures: albedo rgb (sRGB) and mra g, b (linear) -> (value [n, 5], bound [n, 5], exact [n])"""
    a, ab, ex = lookup(albedo, tu, tv, True, storage, mutant)
    m, mb, _ = lookup(mra, tu, tv, False, storage, mutant)
    cols = [2, 1] if mutant == "mra_g_b_swapped" else [1, 2]
    return np.concatenate([a[:, :3], m[:, cols]], axis=1), np.concatenate([ab[:, :3], mb[:, cols]], axis=1), ex


def alpha(img, color_w, tu, tv, storage="linear", mutant=None):
    """§20's alpha a = color.w · texel alpha -> (a [n], bound [n]): the lookup's bound times |color.w| plus the product's own rounding"""
    v, b, _ = lookup(img, tu, tv, False, storage, mutant)
    cw = float(F(color_w))
    a = cw * v[:, 3]
    return a, abs(cw) * b[:, 3] + U * np.abs(a)


def mask_compared(a, bound, cutoff):
    """the rows whose §20 decision a >= cutoff the reference stands for: the others lie within the bound of the cutoff"""
    return np.abs(a - float(F(cutoff))) > bound


def interpolate(uv0, uv1, uv2, hu, hv):
    """§12's (u0·bw + u1·hu) + u2·hv, bw = (1 − hu) − hv, per column of uv [n, 2] -> (uv [n, 2] float64, bound [n, 2]).  Roundings: two in bw, worth 2u·|u0| (|1 − hu|,
    |bw| ≤ 1 + O(u) for barycentrics of a hit); three products and two sums, each at most u·S, S = |u0·bw| + |u1·hu| + |u2·hv|, the first sum less: 2u·|u0| + 5u·S with
    the second-order terms in the factor (1 + 2⁻²⁰)."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (uv0, uv1, uv2))
    hu, hv = np.asarray(hu, F).astype(np.float64)[:, None], np.asarray(hv, F).astype(np.float64)[:, None]
    bw = (1.0 - hu) - hv
    S = np.abs(a * bw) + np.abs(b * hu) + np.abs(c * hv)
    return (a * bw + b * hu) + c * hv, U * (2.0 * np.abs(a) + 5.0 * S) * (1.0 + 2.0 ** -20)


def env_uv(d):
    """the probe's (u, v) of directions [n, 3] with exact functions; atan2(0, 0) = 0 whatever the zeros' signs"""
    d = np.asarray(d, F).astype(np.float64)
    phi = np.where((d[:, 0] == 0) & (d[:, 2] == 0), 0.0, np.arctan2(d[:, 2], d[:, 0]))
    return phi / (2.0 * np.pi) + 0.5, np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi


def env(rgbe, d, mutant=None):
    """SPEC §9's environment lookup of probe [H, W, 4] uint8 along binary32 directions [n, 3] (finite, not all zero needed: a pole is u = ½) -> (rgb [n, 3], bound [n, 3])"""
    tex_all = env_ref.decode(rgbe)
    H, W = tex_all.shape[:2]
    n = len(d)
    if W == 1 and H == 1:
        return np.repeat(tex_all[0, 0][None], n, axis=0), np.zeros((n, 3))
    u, v = env_uv(d)
    if mutant == "env_u_no_half":
        u = u - 0.5
    px, py = u * W - 0.5, v * H - 0.5
    dx = np.full(n, W * ATAN_ERR / (2.0 * np.pi) + U * (5.0 * W + 1.0))
    dy = np.full(n, H * ACOS_ERR / np.pi + U * (4.0 * H + 1.0))
    ywrap = (lambda iy: np.mod(iy, H)) if mutant == "env_v_wraps" else (lambda iy: np.clip(iy, 0, H - 1))
    return _bilinear(lambda ix, iy, which: tex_all[ywrap(iy), np.mod(ix, W)], px, py, dx, dy, np.full(n, 8.0), lambda i: i + 1)


# ------------------------------------------------------------------ the checker
def ratios(value, bound, got):
    """|got − value| / bound per entry: 0 where both are 0, inf where a bound of 0 is missed or got is not finite"""
    err = np.abs(np.asarray(got, np.float64) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(np.asarray(got, np.float64)), r, np.inf)


def passes(value, bound, got):
    return bool(np.all(ratios(value, bound, got) <= 1.0))


def caught(value, bound, got):
    """the share of rows on which a (mutant) reference rejects `got`"""
    r = ratios(value, bound, got)
    return float(np.mean(np.any(r.reshape(len(r), -1) > 1.0, axis=1)))


# ------------------------------------------------------------------ the case set: images
SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (4, 4), (5, 3), (8, 4), (9, 5), (16, 16), (23, 17), (64, 64))     # W x H
NON_SQUARE = ((5, 3), (9, 5), (23, 17))


def image(W, H, k=0):
    """image k of size W x H: fixed random bytes with 0 and 255 placed in every channel (as far as the texels go round); 16x16 holds every byte value in every channel"""
    rs = np.random.RandomState(1000 * W + 10 * H + k)
    if (W, H) == (16, 16):
        return np.stack([rs.permutation(256) for _ in range(4)], axis=-1).astype(np.uint8).reshape(16, 16, 4)
    img = rs.randint(0, 256, (H, W, 4)).astype(np.uint8)
    for c in range(4):      # 0 and 255 never side by side on an axis (half a period apart, diagonally): their midpoint is exactly ½, which §20's cutoff of the tests is
        x, y = rs.randint(W), rs.randint(H)
        img[y, x, c] = 255
        if W * H > 1:
            img[(y + max(1, H // 2)) % H, (x + max(1, W // 2)) % W, c] = 0
    return img


# ------------------------------------------------------------------ the case set: coordinates
def _ulps(x):
    x = np.asarray(x, F)
    return np.concatenate([x, np.nextafter(x, F(np.inf)), np.nextafter(x, F(-np.inf))])


def axis_coords(n):
    """one axis' coordinates for size n: every texel centre and cell border and one ulp to either side, the same shifted by −3, −1, +1, +4 periods, zeros, denormals,
    ±1e-30, and magnitudes 2^10 .. 2^22 (on and off the integers)"""
    base = np.concatenate([(np.arange(n) + 0.5) / n, np.arange(n + 1) / n])
    out = [_ulps((base + s).astype(F)) for s in (0.0, -3.0, -1.0, 1.0, 4.0)]
    out.append(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-30, -1e-30], F))
    k = 2.0 ** np.arange(10, 23)
    out.append(np.concatenate([k, -k, k + 0.37, -k - 0.37, k + 0.5 / n, -k + 0.5 / n]).astype(F))
    return np.concatenate(out)


def coords(W, H):
    """the in-domain rows of a W x H image -> (tu, tv) float32: each axis' set against two fixed values of the other (a texel centre: that axis is then pinned or nearly;
    a generic one), the lattice of all texel centres and of all cell middles, 1 000 combinations of the two sets, 2 000 uniform in [−3, 4]²"""
    rs = np.random.RandomState(77 + 1000 * W + H)
    au, av = axis_coords(W), axis_coords(H)
    fu, fv = [F((W // 2 + 0.5) / W), F(0.3125)], [F((H // 2 + 0.5) / H), F(-0.4375)]
    cy, cx = np.mgrid[0:H, 0:W].reshape(2, -1)                # every texel centre (both axes pinned) and every cell's middle: each cell of the filter has its rows
    lu, lv = np.concatenate([(cx + 0.5) / W, (cx + 1.0) / W]).astype(F), np.concatenate([(cy + 0.5) / H, (cy + 1.0) / H]).astype(F)
    tu = [np.repeat(au, 2), np.tile(fu, len(av)), lu, rs.choice(au, 1000), rs.uniform(-3, 4, 2000).astype(F)]
    tv = [np.tile(fv, len(au)), np.repeat(av, 2), lv, rs.choice(av, 1000), rs.uniform(-3, 4, 2000).astype(F)]
    return np.concatenate(tu).astype(F), np.concatenate(tv).astype(F)


UV_MAX = F(2.0 ** 96)            # lpt.h LPT_UV_MAX: the largest magnitude a mesh may carry
OUTSIDE_SIZES = ((16, 16), (23, 17))


def outside(W, H):
    """coordinates whose floor(fx) is beyond the int32 range, |t·size| at and around 2^31 and 2^32 and up to the domain's end: SPEC §9's saturation rule decides the texel.
    Every binary32 fx here is an integer, so the reference pins both axes and every row is exact.  -> (tu, tv)"""
    def ax(n):
        c = np.array([2.0 ** 31 / n, 2.0 ** 32 / n, 2.0 ** 31, 2.0 ** 40, 1e20, float(UV_MAX)], np.float64).astype(F)
        c = _ulps(_ulps(c))
        c = c[c <= UV_MAX]                 # the domain ends at UV_MAX itself
        return np.concatenate([c, -c])
    au, av = ax(W), ax(H)
    small = np.array([0.3125, (W // 2 + 0.5) / W], F)
    tu = np.concatenate([np.repeat(au, 2), np.tile(small, len(av)), au])
    tv = np.concatenate([np.tile(np.array([0.3125, (H // 2 + 0.5) / H], F), len(au)), np.repeat(av, 2), av[::-1][:len(au)]])
    return tu.astype(F), tv.astype(F)


REJECTED_UV = (3e38, -3e38, np.inf, -np.inf, np.nan, 2.0 ** 97)       # what no mesh may carry (lpt_scene_add_mesh: LPT_ERR_INVALID_ARG)


# ------------------------------------------------------------------ the case set: probes and directions
PROBES = ((2, 1), (1, 2), (2, 2), (5, 3), (8, 4), (16, 8))     # W x H


def probe(W, H):
    """RGBE bytes [H, W, 4]: random mantissas, exponents around 128 with the edge values 0, 5, 9 (black), 10 (the smallest) and 255 (the largest) placed, column W // 2
    and row H // 2 black (where that leaves a texel alight)"""
    rs = np.random.RandomState(500 + 10 * W + H)
    p = rs.randint(0, 256, (H, W, 4)).astype(np.uint8)
    p[..., 3] = rs.randint(120, 137, (H, W))
    flat = p.reshape(-1, 4)
    if W * H >= 8:
        for k, e in zip(rs.permutation(W * H)[:5], (0, 5, 9, 10, 255)):
            flat[k, 3] = e
    if W >= 2:
        p[:, W // 2, :3] = 0
    if H >= 2:
        p[H // 2, :, :3] = 0
    return p


def _unit(u, v):
    phi, th = 2.0 * np.pi * (np.asarray(u, np.float64) - 0.5), np.pi * np.asarray(v, np.float64)
    return np.stack([np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)], axis=-1).astype(F)


def directions(W, H):
    """-> dict of named direction sets [n, 3] float32 for a W x H probe"""
    rs = np.random.RandomState(900 + 10 * W + H)
    uu, vv = np.meshgrid(np.arange(2 * W + 1) / (2.0 * W), np.arange(2 * H + 1) / (2.0 * H))
    tiny = [1e-7, 1e-30, 1e-45, 0.0]
    seam = [(-1.0, y, s * t) for t in tiny for s in (1.0, -1.0) for y in (0.0, 0.25)]
    e = 2.0 ** -24
    near = []
    for y in (1 - e, 1 - 2 * e, 1 - 3 * e, 1 - 16 * e):
        r = np.sqrt(1 - y * y)
        for a in np.arange(8) * (np.pi / 4) + 0.1:
            near += [(r * np.cos(a), y, r * np.sin(a)), (r * np.cos(a), -y, r * np.sin(a))]
    over = [(0.0, 1 + 2 * e, 0.0), (1e-3, 1 + 2 * e, 0.0), (0.0, -1 - 2 * e, 0.0), (0.0, 2.0, 1e-3), (1e-3, -1.5, 1e-3)]
    g = rs.normal(size=(4000, 3))
    return {
        "lattice": _unit(uu.reshape(-1), vv.reshape(-1)),
        "seam": np.array(seam, F),
        "poles": np.array([(0, 1, 0), (0, -1, 0), (0.0, 1, -0.0), (-0.0, -1, 0.0), (-0.0, 1, -0.0)], F),
        "near-poles": np.array(near, F),
        "clamped": np.array(over, F),
        "axes": np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], F),
        "sphere": (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F),
    }


def all_directions(W, H):
    return np.concatenate(list(directions(W, H).values()))
