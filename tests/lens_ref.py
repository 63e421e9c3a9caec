"""A binary64 restatement of the thin lens (SPEC §25; test infrastructure), written from the section on top of tests/primary_ref.py: the four draws of the
ray-generation stream (§4), §11's un-normalised direction, the polar map with §5's polynomial, `o'` and `d'`.  It also holds the two scenes and the cameras of the
in-focus and the out-of-focus test of tests/test_gpu_lens.py, with what the reference alone says about them (tests/test_lens.py checks that on a CPU).

What is exact.  The draws (`float(w >> 8)·2^-24` is exact in either format), §4.3's shift of the first two as primary_ref restates it, and `sincos2pi`'s quadrant
logic (`4u`, `int`, the subtraction are exact in binary32).  The polynomial is evaluated in binary64 with the binary32 coefficients the kernel holds.  Everything
else is binary64.

Tolerances.  First-order bounds on how far a binary32 evaluation of §25 may lie from this module's values, u = 2^-24 per rounding, no contraction; `derivation()`
builds them term by term and `python tests/lens_ref.py` prints the terms.  They assume what primary_ref's K_D assumes (|cx|, |cy| <= 1.5) and an orthonormal view
rounded to binary32 (|right| = |up| = |fwd| = 1 within a few u, `off` perpendicular to `fwd`, so |dir·F − off| >= F).  No number here comes from running the kernels."""
import math

import numpy as np

import primary_ref as P

U = P.U
F32 = np.float32
HALF_PI = float(F32(1.57079632679489661923))
# §5: sin to x^9 and cos to x^10, the coefficients as binary32 holds them, highest power first
SIN_C = [float(F32(c)) for c in (2.7557319223985893e-6, -1.984126984126984e-4, 8.333333333333333e-3, -1.6666666666666666e-1, 1.0)]
COS_C = [float(F32(c)) for c in (-2.755731922398589e-7, 2.48015873015873e-5, -1.3888888888888889e-3, 4.1666666666666664e-2, -0.5, 1.0)]
K_DIR = 29.0        # primary_ref's K_D derivation: the un-normalised `dir` is within 29u per component in binary32


# ------------------------------------------------------------------ §4: the stream
def draws(W, H, user_seed, seed_counter, n=4):
    """the first `n` draws of every pixel's ray-generation stream, a list of (H·W,) float64 holding exact binary32 values"""
    pixel = np.arange(W * H, dtype=np.uint32)
    out = []
    with np.errstate(over="ignore"):
        stage = np.uint32(user_seed) * np.uint32(0x9E3779B9) + np.uint32(seed_counter)
        state = P.pcg(pixel ^ P.pcg(stage ^ np.uint32(P.TAG_RAYGEN)))
        for _ in range(n):
            state = state * np.uint32(747796405) + np.uint32(2891336453)
            w = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
            w = (w >> np.uint32(22)) ^ w
            out.append((w >> np.uint32(8)).astype(np.float64) * U)
    return out


# ------------------------------------------------------------------ §5: sincos2pi
def sincos2pi(u):
    u = np.asarray(u, np.float64)
    q = u * 4.0
    k = np.floor(q).astype(np.int64)            # int(q) of a non-negative q
    x = (q - k) * HALF_PI
    k &= 3
    x2 = x * x
    ps = np.full_like(x, SIN_C[0])
    for c in SIN_C[1:]:
        ps = x2 * ps + c
    sn = x * ps
    cs = np.full_like(x, COS_C[0])
    for c in COS_C[1:]:
        cs = x2 * cs + c
    s = np.choose(k, [sn, cs, -sn, -cs])
    c = np.choose(k, [cs, -sn, -cs, sn])
    return s, c


# ------------------------------------------------------------------ §25
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def lens_offset(cam, R, lx, ly):
    """`off` (N, 3) of the lens samples (lx, ly)"""
    rr = np.sqrt(np.asarray(lx, np.float64))
    s, c = sincos2pi(ly)
    a, b = (R * rr) * c, (R * rr) * s
    return unit(cam.right)[None] * a[:, None] + unit(cam.up)[None] * b[:, None]


def raw_dirs(cam, W, H, jx, jy):
    """§11's un-normalised `dir = (right·cx + up·cy) + fwd` and (cx, cy)"""
    y, x = np.divmod(np.arange(W * H), W)
    sx, sy = (x + jx) / W, (y + jy) / H
    cx, cy = (2.0 * sx - 1.0) * cam.ax, (1.0 - 2.0 * sy) * cam.ay
    return cam.right[None] * cx[:, None] + cam.up[None] * cy[:, None] + cam.fwd[None], cx, cy


class Rays:
    """the primary rays of one sample of a frame: o (N, 3), d (N, 3), off, the un-normalised dir, the focal points origin + dir·F, and (cx, cy)"""


def primary_rays(view, W, H, vfov, R, Fd, user_seed, seed_counter, noise=None):
    cam = P.basis(view, W, H, vfov)
    jx, jy = P.jitter(W, H, user_seed, seed_counter, noise)
    r = Rays()
    r.cam, r.R, r.F = cam, float(R), float(Fd)
    r.dir, r.cx, r.cy = raw_dirs(cam, W, H, jx, jy)
    r.focus = cam.origin[None] + r.dir * r.F
    if R > 0:
        _, _, lx, ly = draws(W, H, user_seed, seed_counter, 4)
        r.lx, r.ly = lx, ly
        r.off = lens_offset(cam, r.R, lx, ly)
        v = r.dir * r.F - r.off
    else:           # §11 as it is: no draw, no F
        r.off = np.zeros_like(r.dir)
        v = r.dir
    r.o = cam.origin[None] + r.off
    r.d = v / np.linalg.norm(v, axis=1, keepdims=True)
    return r


# ------------------------------------------------------------------ tolerances
def _horner_bound(coef, x, dx2):
    """absolute binary32 error, in units of u, of the fma Horner chain p = fma(x2, p, c) at x2 = x², whose own error is dx2 (units of u): every step adds
    x2·e + |p|·dx2 + |p_new| (the fma's one rounding)"""
    x2 = x * x
    p, e = coef[0], 0.0
    for c in coef[1:]:
        pn = x2 * p + c
        e = x2 * e + abs(p) * dx2 + abs(pn)
        p = pn
    return e, p


def derivation():
    """-> (terms, K) : the named terms of the bounds, in units of u, and the constants the tolerances use"""
    t = {}
    # x = f·(π/2): one rounding on a value <= π/2;  x2 = x·x: twice x's relative error and one rounding
    xs = np.linspace(0.0, HALF_PI, 257)
    t["x = f·(pi/2), absolute"] = HALF_PI
    t["x2 = x·x, absolute (3u relative on <= 2.47)"] = 3.0 * HALF_PI ** 2
    sin_e = cos_e = 0.0
    for x in xs:
        dx, dx2 = x, 3.0 * x * x
        e, ps = _horner_bound(SIN_C, x, dx2)
        sin_e = max(sin_e, x * e + abs(ps) * dx + abs(x * ps))      # sn = x·ps: ps's error, x's error, one rounding
        e, _ = _horner_bound(COS_C, x, dx2)
        cos_e = max(cos_e, e)
    t["sin polynomial and x·ps, absolute"] = sin_e
    t["cos polynomial, absolute"] = cos_e
    k_sc = max(sin_e, cos_e)
    # rr = sqrt(lx): correctly rounded, 1u relative;  R·rr: 1 more;  (R·rr)·c: c's error on a factor <= R, 1 more rounding: per unit of R
    t["rr = sqrt(lx), relative"] = 1.0
    k_ab = 2.0 + k_sc + 1.0
    t["a = (R·rr)·c and b, absolute per unit of R"] = k_ab
    # rn = normalize(right) on the host: dot 3, sqrt 1, 1/x 1, product 1 (primary_ref's count for a unit vector)
    k_n = 6.0
    t["rn, un = normalize(right), normalize(up), absolute per component"] = k_n
    # off_i = rn_i·a + un_i·b: (|rn_i| + |un_i|)·da <= √2·da;  (|a| + |b|)-terms: a² + b² <= R², so |a|·k_n + |b|·k_n <= √2·R·k_n;  two products and the sum: 3u on
    # |rn_i·a| + |un_i·b| <= R·√2
    k_off = math.sqrt(2.0) * (k_ab + k_n + 3.0)
    t["off per component, absolute per unit of R"] = k_off
    # v = dir·F − off per component: dir within K_DIR·u, |dir_i| <= 2.5 (|cx|, |cy| <= 1.5): F·K_DIR + one rounding of dir_i·F (2.5·F) + off's error + one rounding of
    # the difference (<= 2.5·F + R)
    t["v = dir·F − off per component: per unit of F"] = K_DIR + 5.0
    t["v = dir·F − off per component: per unit of R"] = k_off + 1.0
    # d' = normalize(v): a change dv moves v/|v| by at most |dv|/|v| (its part across v), |dv| <= √3·max_i, |v| >= F; the normalisation's own 6 roundings
    t["normalize(v), absolute per component"] = 6.0
    return t, {"k_sc": k_sc, "k_off": k_off, "k_vF": K_DIR + 5.0, "k_vR": k_off + 1.0, "k_norm": 6.0}


_K = derivation()[1]


def tol_offset(R):
    """per component of `off`"""
    return _K["k_off"] * U * R


def tol_origin(R, o_abs):
    """per component of o' = origin + off: off's bound and the sum's rounding"""
    return tol_offset(R) + U * np.abs(o_abs)


def tol_direction(R, Fd):
    """per component of d' (R = 0: primary_ref's K_D)"""
    if not R > 0:
        return P.K_D * U
    return (math.sqrt(3.0) * (_K["k_vF"] * Fd + _K["k_vR"] * R) / Fd + _K["k_norm"]) * U


def tol_focus(R, Fd, o_abs_max, dir_len_max=2.5):
    """how far the binary32 ray (o', d') may pass from the binary64 focal point origin + dir·F: o's error as a length, and d's across the ray over the distance
    |dir·F − off| <= |dir|·F + R"""
    return math.sqrt(3.0) * float(np.max(tol_origin(R, o_abs_max))) + (dir_len_max * Fd + R) * math.sqrt(3.0) * tol_direction(R, Fd)


def tol_perpendicular(cam, R, o_abs_max):
    """|off·fwd| of a binary32 `off` recovered as o' − origin: the view's own departure from orthogonality, in binary64, plus o's error along fwd"""
    f = cam.fwd
    return R * (abs(unit(cam.right) @ f) + abs(unit(cam.up) @ f)) + math.sqrt(3.0) * float(np.max(tol_origin(R, o_abs_max))) * float(np.linalg.norm(f))


# ------------------------------------------------------------------ the cases of the ray test
RAY_VIEWS = [((0.0, 1.1, -6.0), (0.0, 0.0, 1.0), 0.0), ((0.3, 1.25, -5.7), (0.12, 0.0, 1.0), 0.35), ((0.9, 1.7, -0.2), (0.1, 0.3, 1.0), 0.0)]
RAY_VFOV = 1.05
RAY_LENSES = ((0.05, 4.0), (0.3, 1.5))
RAY_SAMPLES = (0, 3)
USER_SEED = 7


# ------------------------------------------------------------------ a plane in focus: the checkerboard
# The camera looks along −z from the origin; the board is the plane z = −F, cells of side CELL, two emissive materials by (i + j) parity.  It reaches beyond the
# frame's corners (|cx| <= ax, |cy| <= ay at the plane: ±ax·F by ±ay·F) by at least a cell.
BOARD_F, BOARD_R, BOARD_VFOV = 2.0, 0.08, 0.7
BOARD_CELL = 0.125
BOARD_LE = ((2.0, 0.5, 0.25), (0.125, 1.0, 3.0))
BOARD_EYE, BOARD_DIR = (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)


def board_cells(W, H):
    th = math.tan(0.5 * float(F32(BOARD_VFOV)))
    nx = int(math.ceil((W / H) * th * BOARD_F / BOARD_CELL)) + 1
    ny = int(math.ceil(th * BOARD_F / BOARD_CELL)) + 1
    return nx, ny           # cells i in [−nx, nx), j in [−ny, ny)


BOARD_DIR_LEN = 1.3         # |dir| over the board's frames: sqrt(1 + ax² + ay²) <= 1.3 at vfov 0.7 up to aspect 2 (tests/test_lens.py asserts it of the reference's own dirs)


def board_edge_eps(o_abs_max=BOARD_R):
    """The distance, in the plane, below which the pinhole's and the lens ray's hit may fall on different sides of a triangle edge.  The lens ray passes within
    tol_focus of the binary64 focal point and the pinhole ray within t·√3·K_D·u of it, t <= t_max = |dir|·F + R.  Both cross the plane at an angle whose cosine is at
    least F/t_max, so a miss distance across the ray is stretched by at most t_max/F in the plane.  §7 states the affine test's own rounding as 3e-7·(|o| + t) world
    units, once per ray."""
    t_max = BOARD_DIR_LEN * BOARD_F + BOARD_R
    stretch = t_max / BOARD_F
    lens = tol_focus(BOARD_R, BOARD_F, o_abs_max, BOARD_DIR_LEN) * stretch
    pin = t_max * math.sqrt(3.0) * P.K_D * U * stretch
    return lens + pin + 2.0 * 3.0e-7 * (o_abs_max + t_max)


def board_reference(view, W, H, user_seed, seed_counter):
    """per pixel: the cell parity (0 / 1) the binary64 focal point falls in, the triangle of the cell's quad (0: below the diagonal from the cell's low corner,
    1: above), the cell (i, j), and whether the point is compared — farther than board_edge_eps from the cell's borders and its diagonal"""
    r = primary_rays(view, W, H, BOARD_VFOV, BOARD_R, BOARD_F, user_seed, seed_counter)
    p = r.focus                                     # on z = −F up to the view's rounding
    gx, gy = p[:, 0] / BOARD_CELL, p[:, 1] / BOARD_CELL
    i, j = np.floor(gx), np.floor(gy)
    fx, fy = gx - i, gy - j
    eps = board_edge_eps() / BOARD_CELL
    margin = np.minimum(np.minimum(np.minimum(fx, 1.0 - fx), np.minimum(fy, 1.0 - fy)), np.abs(fx - fy) / math.sqrt(2.0))
    return ((i + j).astype(np.int64) & 1), (fy > fx).astype(np.int64), i.astype(np.int64), j.astype(np.int64), margin >= eps, r


# ------------------------------------------------------------------ out of focus: one small quad
SPOT_W, SPOT_H = 64, 32
SPOT_VFOV = 0.6
SPOT_R, SPOT_F, SPOT_Z = 0.2, 1.0, 4.0
SPOT_LE = (3.0, 2.0, 0.5)
SPOT_SAMPLES = 256        # four batches of 64: the expected hit count is 1024, five of its standard deviations 16 %


def spot_numbers():
    """-> the quad's half side (its pinhole footprint is 2 x 2 pixels), the disc radius in pixels, the half diagonal in pixels, the projected centre in pixels and the
    expected number of hits of SPOT_SAMPLES samples per pixel"""
    th = math.tan(0.5 * float(F32(SPOT_VFOV)))
    ax = (SPOT_W / SPOT_H) * th
    px_per_c = SPOT_W / (2.0 * ax)                  # pixels per unit of cx; the same vertically (H / (2·ay))
    half = SPOT_Z / px_per_c                        # one pixel at depth z, in world units: a 2 x 2 pixel square
    rho = SPOT_R * abs(1.0 / SPOT_F - 1.0 / SPOT_Z) * px_per_c
    area_px = (2.0 * half / SPOT_Z * px_per_c) ** 2
    return half, rho, math.sqrt(2.0) * (half / SPOT_Z) * px_per_c, (SPOT_W / 2.0, SPOT_H / 2.0), area_px * SPOT_SAMPLES


if __name__ == "__main__":
    terms, K = derivation()
    for name, val in terms.items():
        print("%-72s %8.3f u" % (name, val))
    for R, Fd in RAY_LENSES + ((BOARD_R, BOARD_F),):
        print("R = %g, F = %g: off %.3g, d' %.3g (= %.1f u) per component, focus %.3g (|o| <= 8)" % (R, Fd, tol_offset(R), tol_direction(R, Fd), tol_direction(R, Fd) / U, tol_focus(R, Fd, 8.0)))
    print("board: edge distance %.3g world units = %.3g of a cell" % (board_edge_eps(), board_edge_eps() / BOARD_CELL))
    print("spot: half side %.4g, disc radius %.3g px, half diagonal %.3g px, centre %s, expected hits %.1f" % spot_numbers())
