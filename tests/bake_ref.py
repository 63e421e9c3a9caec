"""A binary64 reference of instance baking, written from SPEC.md §2.5 (world positions, cofactor normals, the determinant and the mirrored-instance rule), §6 (Woop rows),
§7 (ray / triangle) and §12 (the interpolated, flipped shading normal; with a map §24, through normal_ref.py) — from the SPEC text, not from bvh.cpp, kernels.h or the oracle
(test infrastructure).  The three bakes of the project are held to it by tests/test_bake_reference.py (host, oracle) and tests/test_gpu_bake_reference.py (device).

Every output carries a RUNNING ERROR BOUND in the manner of normal_ref.py (its class R; u = 2^-24): each rounded binary32 operation of the SPEC's parenthesised form contributes
u·|result| and is propagated to first order through the operations that follow.
  * §2.5: a cofactor is a·b − c·d without fma, three roundings; the matrix-vector products are the two-add chains; normalize is dot, sqrt, reciprocal, product.  The inputs (the
    mesh, the matrix) are binary32 numbers that every bake reads exactly: bound 0.
  * §6: the rows are computed in binary64 and rounded ONCE: u·|row|.  Checked against rows evaluated here from the bake's own binary32 vertices, so the only other term is the
    difference of two binary64 evaluations of one formula: at most K64 = 16 roundings (the longest chain — edge, cross, cross, det, reciprocal, product, the dot with p0 — has 14)
    of 2^-53 each on the sum of the ABSOLUTE values of the formula's terms (`woop64` returns that sum).
  * §7: `tuv_chain` evaluates the fma chains with R: rows that are off by u·|row|, one rounding per fma, the division.  To this comes what the bake's own error does to the
    triangle: `tuv` is evaluated again with each of the nine vertex coordinates moved by its §2.5 bound and the changes are summed (`spread`) — first order, like everything else.
  * §12 / §24: normal_ref.shading_normal on the binary64 bake gives the roundings of the shading itself; what the bake's error does to it is again `spread` over the eighteen
    inputs (nine coordinates, nine normal components), on the normal and on every deciding quantity.
Every bound above is derived: no quantity needed the fallback of a measured constant.
A check passes when |got − ref| <= 2·bound (TOL): the factor covers the second-order terms and the rounding of the probes' own inputs.  No measured constant enters any bound.
An element whose bound says nothing is EXCLUDED, not passed: a normal whose angular bound exceeds MAX_ANGLE = 0.01 rad, or one of whose decisions lies within its bound of its
threshold; a ray whose binary64 hit lies within 2·bound of an edge, or for which another triangle of its instance group could be hit (within 2·bound) at or before it.  At most
MAX_EXCLUDED = 2 % of a case's elements may be excluded and every triangle of every case must still be compared: `census` counts, tests/test_bake_reference.py asserts."""
import functools

import numpy as np

import normal_ref as NR

R = NR.R
U = NR.U
TOL = 2.0            # |got − ref| <= TOL·bound
MAX_ANGLE = 0.01     # rad: a looser normal bound means nothing
MAX_EXCLUDED = 0.02  # share of a case's elements
K64 = 16.0           # binary64 roundings of one Woop row, see above
U64 = 2.0 ** -53
MISS = 0xFFFFFFFF


# ------------------------------------------------------------------ R helpers that normal_ref has no use for
def fma(a, b, c):
    """fma(a, b, c): one rounding"""
    v = a.v * b.v + c.v
    return R(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + c.e + U * np.abs(v))


def div(a, b):
    """a / b, correctly rounded; the denominator taken at its smallest"""
    with np.errstate(all="ignore"):
        v = a.v / b.v
        den = np.abs(b.v) - b.e
        e = np.where(den > 0, (a.e + np.abs(v) * b.e) / np.where(den > 0, den, 1.0) + U * np.abs(v), np.inf)
    return R(v, e)


def _normalize(n):
    """§3: n·(1/sqrt(dot(n, n))), zero stays zero (an exact zero: value and bound)"""
    l2 = NR.dot(n, n)
    zero = (l2.v == 0) & (l2.e == 0)
    with np.errstate(all="ignore"):
        out = NR.scale3(n, l2.rsqrt())
    return tuple(R(np.where(zero, 0.0, c.v), np.where(zero, 0.0, c.e)) for c in out)


# ------------------------------------------------------------------ §2.5
def bake64(pos, nrm, m):
    """one instance: pos (nv, 3), nrm (nv, 3) the mesh, m (16,) column-major, all binary32 numbers -> dict P, eP, N, eN (nv, 3), det, e_det, mirrored (det < 0),
    certain (|det| > e_det, or det is exact)"""
    pos, nrm = np.asarray(pos, np.float64), np.asarray(nrm, np.float64)
    mm = [R(np.float64(x)) for x in np.asarray(m, np.float32).reshape(16)]
    x, y, z = NR.vec(pos, np.float64)
    P = tuple(((mm[r] * x + mm[4 + r] * y) + mm[8 + r] * z) + mm[12 + r] for r in range(3))
    M = [[mm[4 * c + r] for c in range(3)] for r in range(3)]           # M[r][c]

    def cof(r, c):
        r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
        return M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]

    C = [[cof(r, c) for c in range(3)] for r in range(3)]
    det = (M[0][0] * C[0][0] + M[0][1] * C[0][1]) + M[0][2] * C[0][2]
    mirrored = bool(det.v < 0)
    nx, ny, nz = NR.vec(nrm, np.float64)
    N = tuple((C[r][0] * nx + C[r][1] * ny) + C[r][2] * nz for r in range(3))
    if mirrored:
        N = NR.neg3(N)
    N = _normalize(N)
    return {"P": NR.arr(P), "eP": NR.err(P), "N": NR.arr(N), "eN": NR.err(N), "det": float(det.v), "e_det": float(det.e), "mirrored": mirrored,
            "certain": bool(abs(det.v) > det.e or det.e == 0)}


def baked_triangles(mesh, m):
    """the instance's triangles in baked order: P, eP, N, eN (nt, 3, 3), uv (nt, 3, 2); vertices 1 and 2 exchanged where det < 0"""
    b = bake64(mesh["pos"], mesh["nrm"], m)
    tri = np.asarray(mesh["idx"]).reshape(-1, 3)
    if b["mirrored"]:
        tri = tri[:, [0, 2, 1]]
    out = {k: b[k][tri] for k in ("P", "eP", "N", "eN")}
    out["uv"] = np.asarray(mesh["uv"], np.float64)[tri]
    out.update(mirrored=b["mirrored"], certain=b["certain"], det=b["det"], e_det=b["e_det"])
    return out


# ------------------------------------------------------------------ §6
def woop64(P):
    """P (..., 3, 3) -> rows (..., 3, 4) in binary64, and the sum of absolute terms behind each entry (for the K64 term); det <= 0 -> zeros"""
    P = np.asarray(P, np.float64)
    p0, e1, e2 = P[..., 0, :], P[..., 1, :] - P[..., 0, :], P[..., 2, :] - P[..., 0, :]

    def cross(a, b, ab=False):
        f = (lambda s, t: np.abs(s) + np.abs(t)) if ab else (lambda s, t: s - t)
        return np.stack([f(a[..., 1] * b[..., 2], a[..., 2] * b[..., 1]), f(a[..., 2] * b[..., 0], a[..., 0] * b[..., 2]), f(a[..., 0] * b[..., 1], a[..., 1] * b[..., 0])], -1)

    n = cross(e1, e2)
    na = cross(e1, e2, True)
    det = (n * n).sum(-1)
    ok = det > 0
    with np.errstate(all="ignore"):
        inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)[..., None]
    r = np.stack([cross(e2, n) * inv, cross(n, e1) * inv, n * inv], -2)
    ra = np.stack([cross(np.abs(e2), na, True) * inv, cross(na, np.abs(e1), True) * inv, na * inv], -2)
    w = -(r * p0[..., None, :]).sum(-1)
    wa = (ra * np.abs(p0[..., None, :])).sum(-1)
    rows = np.concatenate([r, w[..., None]], -1)
    return np.where(ok[..., None, None], rows, 0.0), np.where(ok[..., None, None], np.concatenate([ra, wa[..., None]], -1), 0.0)


def woop_bound(P32):
    """reference rows for a bake's OWN binary32 vertices and the bound of its binary32 rows against them"""
    rows, absum = woop64(P32)
    return rows, U * np.abs(rows) + K64 * U64 * absum


# ------------------------------------------------------------------ §7
def tuv(P, o, d, full=False):
    """the binary64 (t, u, v) of rays o, d (..., 3) against triangles P (..., 3, 3), broadcast; NaN for a degenerate triangle.  full: (t, u, v, oz, dz), t = −oz/dz"""
    rows, _ = woop64(P)
    with np.errstate(all="ignore"):
        oc = [(rows[..., k, :3] * o).sum(-1) + rows[..., k, 3] for k in range(3)]
        dc = [(rows[..., k, :3] * d).sum(-1) for k in range(3)]
        t = -oc[2] / dc[2]
        return np.stack([t, oc[0] + t * dc[0], oc[1] + t * dc[1], oc[2], dc[2]], -1)[..., :5 if full else 3]


def tuv_chain(P, o, d):
    """§7's fma chains on rows rounded once: the bounds of (t, u, v, oz, dz) against `tuv` for a triangle the device knows exactly -> (..., 5)"""
    rows, _ = woop64(P)
    o, d = np.broadcast_arrays(np.asarray(o, np.float64), np.asarray(d, np.float64))
    shape = np.broadcast_shapes(rows.shape[:-2], o.shape[:-1])
    rows = np.broadcast_to(rows, shape + (3, 4))
    o, d = np.broadcast_to(o, shape + (3,)), np.broadcast_to(d, shape + (3,))
    oo, dd = [R(o[..., k]) for k in range(3)], [R(d[..., k]) for k in range(3)]

    def chains(k):
        r = [R(rows[..., k, j], U * np.abs(rows[..., k, j])) for j in range(4)]
        return fma(r[2], oo[2], fma(r[1], oo[1], fma(r[0], oo[0], r[3]))), fma(r[2], dd[2], fma(r[1], dd[1], r[0] * dd[0]))

    with np.errstate(all="ignore"):
        oz, dz = chains(2)
        t = -div(oz, dz)
        ox, dx = chains(0)
        oy, dy = chains(1)
        u, v = fma(t, dx, ox), fma(t, dy, oy)
    return np.stack([t.e, u.e, v.e, oz.e, dz.e], -1)


def spread(f, x, ex):
    """first-order effect of input errors: sum over the entries k of the last two axes of x of |f(x + ex_k) − f(x)|"""
    base = f(x)
    out = np.zeros_like(base)
    for i in range(x.shape[-2]):
        for j in range(x.shape[-1]):
            if not np.any(ex[..., i, j]):
                continue
            y = x.copy()
            y[..., i, j] += ex[..., i, j]
            with np.errstate(all="ignore"):
                delta = np.abs(f(y) - base)
            out += np.where(np.isfinite(delta), delta, np.inf)
    return out


def trace_reference(tris, o, d, target):
    """rays o, d (nr, 3) (binary32 numbers) against the group's triangles `tris` (P, eP: (nt, 3, 3)); target (nr,) the triangle each ray was aimed at.
    -> dict prim (nr,) (MISS where no triangle is hit for sure), tuv, bound (nr, 3), compared (nr,) bool"""
    P, eP = tris["P"], tris["eP"]
    o64, d64 = np.asarray(o, np.float64)[:, None, :], np.asarray(d, np.float64)[:, None, :]
    with np.errstate(all="ignore"):
        x = tuv(P[None], o64, d64, True)                                              # (nr, nt, 5)
        b = tuv_chain(P[None], o64, d64) + spread(lambda q: tuv(q, o64, d64, True), np.broadcast_to(P[None], (o64.shape[0],) + P.shape).copy(), np.broadcast_to(eP[None], (o64.shape[0],) + P.shape))
        b = np.where(np.isfinite(b), b, np.inf)
        # the least |t| binary32 can compute: t = −oz/dz with |oz| at its smallest and |dz| at its largest.  It speaks where the bound of t itself says nothing (a triangle
        # the ray runs nearly parallel to, dz ~ 0): such a triangle, far from the ray, is still no rival
        t_least = np.maximum(np.abs(x[..., 3]) - TOL * b[..., 3], 0.0) / (np.abs(x[..., 4]) + TOL * b[..., 4])
        t, u, v = x[..., 0], x[..., 1], x[..., 2]
        bt, bu, bv = TOL * b[..., 0], TOL * b[..., 1], TOL * b[..., 2]
        degenerate = ~np.isfinite(t) | ~np.isfinite(u) | ~np.isfinite(v)            # Woop rows all zero: never hit (t = −0/0)
        sure = ~degenerate & (t > bt) & (u > bu) & (v > bv) & (1 - u - v > bu + bv)
        out_ = degenerate | (t < -bt) | (u < -bu) | (v < -bv) | (1 - u - v < -(bu + bv))
    unsure = ~sure & ~out_
    nr = t.shape[0]
    tt = np.where(sure, t, np.inf)
    best = tt.argmin(1)
    hit = np.isfinite(tt[np.arange(nr), best])
    t_best, bt_best = t[np.arange(nr), best], bt[np.arange(nr), best]
    rival = (sure | unsure) & (t - bt <= (t_best + bt_best)[:, None]) & ~(t_least > (t_best + bt_best)[:, None])
    rival[np.arange(nr), best] = False
    compared = hit & ~rival.any(1) & (best == target)
    unsure &= np.isfinite(t_least)                                                   # t_least = inf: dz = 0 for sure, t is no number, no hit
    nothing = ~(sure | unsure).any(1)                                                # a sure miss of every triangle is a comparison too
    return {"prim": np.where(hit, best, MISS).astype(np.uint32), "tuv": x[np.arange(nr), best, :3], "bound": b[np.arange(nr), best, :3], "compared": compared | (nothing & (target == MISS)),
            "miss": nothing}


# ------------------------------------------------------------------ §12 / §24
def normal_reference(tris, prim, bary, d, image=None, scale=1.0):
    """elements (prim, bary (u, v), d): the binary64 shading normal of the binary64 bake, its bound (shading roundings + the bake's error) and whether it is compared"""
    P, N, uv = tris["P"][prim], tris["N"][prim], tris["uv"][prim]
    eP, eN = tris["eP"][prim], tris["eN"][prim]

    def run(pn):
        return NR.shading_normal(pn[:, :3], pn[:, 3:], uv, bary, d, image=image, scale=scale, dtype=np.float64)

    x = np.concatenate([P, N], 1)
    ex = np.concatenate([eP, eN], 1)
    with np.errstate(all="ignore"):
        ref = run(x)
        names = list(ref["q"])
        both = lambda r: np.concatenate([r["Ns"]] + [np.asarray(r["q"][k][0], np.float64)[:, None] for k in names], 1)
        s = spread(lambda y: both(run(y)), x, ex)
    bound = ref["Ns_err"] + s[:, :3]
    decided = ~NR.undecided(ref)
    reached = ref.get("reached", {k: np.ones(len(prim), bool) for k in names})
    for i, k in enumerate(names):
        v, e = ref["q"][k]
        tot = e + s[:, 3 + i]
        decided &= ~reached[k] | (tot == 0) | (np.abs(np.asarray(v, np.float64)) > TOL * tot)
    with np.errstate(all="ignore"):
        angle = np.sqrt((bound ** 2).sum(1))
    flat = ~(np.abs(ref["Ns"]).sum(1) > 0) | ~np.isfinite(ref["Ns"]).all(1)          # a degenerate triangle: the probe answers zeros
    compared = decided & np.isfinite(angle) & (angle <= MAX_ANGLE) & ~flat
    return {"Ns": ref["Ns"], "bound": bound, "mapped": ref["mapped"], "compared": compared, "degenerate": flat}


# ------------------------------------------------------------------ geometry (binary32 numbers throughout)
F = np.float32


def patch_mesh():
    """a bumpy 4x4 height-field patch z = f(x, y) over [-1/2, 1/2]^2, smooth analytic normals, uv that repeat; two halves of 16 triangles each (x < 0 carries the normal map)"""
    g = np.linspace(-0.5, 0.5, 5)
    X, Y = np.meshgrid(g, g, indexing="xy")
    f = 0.06 * np.sin(5.0 * X + 0.4) * np.cos(4.0 * Y - 0.3) + 0.05 * X * Y
    fx = 0.30 * np.cos(5.0 * X + 0.4) * np.cos(4.0 * Y - 0.3) + 0.05 * Y
    fy = -0.24 * np.sin(5.0 * X + 0.4) * np.sin(4.0 * Y - 0.3) + 0.05 * X
    pos = np.stack([X, Y, f], -1).reshape(-1, 3).astype(F)
    n = np.stack([-fx, -fy, np.ones_like(fx)], -1).reshape(-1, 3)
    nrm = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    uv = np.stack([(X + 0.5) * 1.7, (Y + 0.5) * 1.3], -1).reshape(-1, 2).astype(F)
    halves = []
    for cols in ((0, 1), (2, 3)):
        idx = []
        for j in range(4):
            for i in cols:
                a = j * 5 + i
                idx += [a, a + 1, a + 6, a, a + 6, a + 5] if (i + j) % 2 == 0 else [a, a + 1, a + 5, a + 1, a + 6, a + 5]
        halves.append({"pos": pos, "nrm": nrm, "uv": uv, "idx": np.asarray(idx, np.uint32)})
    return halves


def octahedron_mesh():
    """a closed octahedron subdivided once on the sphere of radius 1/2: 32 triangles, outward winding, normals = directions, spherical uv"""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.asarray(p, np.float64) for p in v]
    mid, idx = {}, []

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            p = v[a] + v[b]
            v.append(p / np.linalg.norm(p))
            mid[k] = len(v) - 1
        return mid[k]

    for a, b, c in faces:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        idx += [a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca]
    n = np.asarray(v)
    pos = (0.5 * n).astype(F)
    # normals a little off the radial direction, so that every vertex has its own and the interpolation order shows
    nn = n + 0.15 * np.stack([n[:, 1] * n[:, 2], n[:, 0] * n[:, 2], n[:, 0] * n[:, 1]], -1)
    nrm = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(F)
    uv = np.stack([0.5 + np.arctan2(n[:, 2], n[:, 0]) / (2 * np.pi), np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], -1).astype(F)
    out = {"pos": pos, "nrm": nrm, "uv": uv, "idx": np.asarray(idx, np.uint32)}
    tri = out["idx"].reshape(-1, 3)
    p = pos.astype(np.float64)
    assert np.all((np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]]) * p[tri].mean(1)).sum(1) > 0)     # outward
    return out


def mirror_mesh(mesh):
    """the mirror image in x, authored outward again: x negated, vertices 1 and 2 of every triangle exchanged, normals mirrored (every step exact)"""
    pos, nrm = mesh["pos"].copy(), mesh["nrm"].copy()
    pos[:, 0], nrm[:, 0] = -pos[:, 0], -nrm[:, 0]
    return {"pos": pos, "nrm": nrm, "uv": mesh["uv"], "idx": mesh["idx"].reshape(-1, 3)[:, [0, 2, 1]].reshape(-1).copy()}


def mirror_matrix(m):
    """M·diag(−1, 1, 1): the first column negated (exact)"""
    m = np.asarray(m, F).reshape(16).copy()
    m[:3] = -m[:3]
    return m


def normal_image():
    """5 wide, 3 high: no power of two; blue high so that the map never pushes the normal far"""
    rng = np.random.RandomState(24)
    img = rng.randint(64, 192, (3, 5, 4)).astype(np.uint8)
    img[..., 2] = 230
    return img


NORMAL_SCALE = 0.8


def dark_light(dtype):
    """the scene's one rectangle light (§2.4, §8), put where no ray of these tests can hit it: below every scene, facing down — a ray that goes down sees its back (dn > 0),
    one that goes up has it behind (t < 0)"""
    light = np.zeros(1, dtype)
    light["normal"], light["tangent"], light["bitangent"], light["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.001), (0, 0, 1, 0.001), (0, -1.0e9, 0, 0.0)
    return light


def matrix(a, t=(0.0, 0.0, 0.0)):
    """3x3 `a` (rounded to binary32) and a translation -> column-major (16,)"""
    m = np.eye(4, dtype=F)
    m[:3, :3] = np.asarray(a, np.float64).astype(F)
    m[:3, 3] = np.asarray(t, F)
    return np.ascontiguousarray(m.T).reshape(16)


def _rotation(axis, angle):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


SPACING = 64.0   # between the cases of one scene: the largest instance (rotation x scale (1, 7, 0.03)) is 7 long and its rays start 3 sizes away


def groups():
    """{scene name: [(case name, 3x3, translation, unit)]}: the cases of one scene stand SPACING apart along x.  The two uniform scales far from 1 and the far
    object have scenes of their own, so that §7's scene-wide padding term follows them alone.  `degenerate` cases (rank 1, zero) bake only degenerate triangles."""
    rot = _rotation((1.0, 2.0, 3.0), 0.9)
    main = [("identity", np.eye(3)), ("rotation", rot), ("rotation-scale", rot @ np.diag([1.0, 7.0, 0.03])),
            ("shear", np.array([[1.0, 0.7, 0.3], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])), ("mirror-x", np.diag([-1.0, 1.0, 1.0])), ("minus-identity", -np.eye(3)),
            ("rank-2", np.diag([1.0, 1.0, 0.0])), ("rank-1", np.diag([1.5, 0.0, 0.0])), ("zero", np.zeros((3, 3)))]
    out = {"main": [(n, a, (SPACING * k, 0.0, 0.0), 1.0) for k, (n, a) in enumerate(main)],
           "tiny": [("scale-2^-20", np.eye(3) * 2.0 ** -20, (0.0, 0.0, 0.0), 2.0 ** -20)],
           "huge": [("scale-2^20", np.eye(3) * 2.0 ** 20, (0.0, 0.0, 0.0), 2.0 ** 20)],
           "far": [("far-10^4", np.eye(3), (1.0e4, 0.0, 0.0), 1.0)]}
    return out


ASIDE = 40.0     # the octahedron of a case stands this far (times the case's unit) from its patch along y: rays start at most 3 x 7.1 + 3.6 from their own instance's centre


OUTSIDE = {"out-2^-60": np.eye(3) * 2.0 ** -60, "out-2^60": np.eye(3) * 2.0 ** 60}   # outside the stated domain: finite outputs and agreeing paths only


def meshes():
    a, b = patch_mesh()
    return {"patch-mapped": a, "patch-plain": b, "octahedron": octahedron_mesh()}


def case_meshes(name):
    """rank 2 flattens along the patch's height axis: the patch does not overlap itself, the closed octahedron would (its two halves coincide), so it stays out"""
    return ("patch-mapped", "patch-plain") if name == "rank-2" else ("patch-mapped", "patch-plain", "octahedron")


BARY = np.asarray([(a / 7.0, b / 7.0) for a in range(1, 6) for b in range(1, 7 - a)] + [(1.0 / 3.0, 1.0 / 3.0)], np.float64).astype(F)   # 15 lattice points inside + the centroid
assert BARY.shape == (16, 2)
MAX_TILT = np.deg2rad(75.0)


def build_group(cases, ms=None):
    """one scene: instances in order (case by case, mesh by mesh), the binary64 baked triangles of all of them, and the fixed rays.
    -> dict instances [(mesh name, m16, case index)], tris (P, eP, N, eN, uv: (nt, 3, 3)), case (nt,), mesh (nt,) names, rays o, d (nr, 3) float32, target (nr,), ray_case"""
    ms = ms or meshes()
    inst, parts, tri_case, tri_mesh = [], [], [], []
    inst_of = []
    for ci, (name, a, t, unit) in enumerate(cases):
        for mn in case_meshes(name):
            m = matrix(a, (t[0], t[1] + (ASIDE * unit if mn == "octahedron" else 0.0), t[2]))
            inst_of += [len(inst)] * (ms[mn]["idx"].size // 3)
            inst.append((mn, m, ci))
            bt = baked_triangles(ms[mn], m)
            assert bt["certain"], (name, bt["det"], bt["e_det"])
            parts.append(bt)
            tri_case += [ci] * bt["P"].shape[0]
            tri_mesh += [mn] * bt["P"].shape[0]
    tris = {k: np.concatenate([p[k] for p in parts]) for k in ("P", "eP", "N", "eN", "uv")}
    tri_case = np.asarray(tri_case)
    P = tris["P"]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = np.cross(e1, e2)
    ln = np.linalg.norm(n, axis=1)
    o, d, target, ray_case = [], [], [], []
    inst_of = np.asarray(inst_of)
    for ci, (name, a, t, unit) in enumerate(cases):
        sel = np.nonzero(tri_case == ci)[0]
        for ti in sel:
            own = P[inst_of == inst_of[ti]].reshape(-1, 3)
            size = np.linalg.norm(own.max(0) - own.min(0))                          # of the ray's own instance
            for k, (bu, bv) in enumerate(BARY.astype(np.float64)):
                x = P[ti, 0] * (1 - bu - bv) + P[ti, 1] * bu + P[ti, 2] * bv
                if ln[ti] > 0:
                    nn = n[ti] / ln[ti]
                    tx = e1[ti] / np.linalg.norm(e1[ti])
                    by = np.cross(nn, tx)
                    th, ph = MAX_TILT * k / 15.0, 2.399963229728653 * k           # the golden angle: azimuths that never repeat
                    w = nn * np.cos(th) + (tx * np.cos(ph) + by * np.sin(ph)) * np.sin(th)
                    dist = 3.0 * size
                else:                                                               # a degenerate triangle: nothing to aim at but its points; every such ray must miss
                    th, ph = np.pi * (k + 0.5) / 16.0, 2.399963229728653 * k
                    w = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
                    dist = 3.0 * max(size, unit)
                o.append(x + dist * w)
                d.append(-w)
                target.append(ti if ln[ti] > 0 else MISS)
                ray_case.append(ci)
    return {"instances": inst, "tris": tris, "tri_case": tri_case, "tri_mesh": np.asarray(tri_mesh), "o": np.asarray(o).astype(F), "d": np.asarray(d).astype(F),
            "target": np.asarray(target, np.int64), "ray_case": np.asarray(ray_case), "cases": [c[0] for c in cases], "degenerate": ~(ln > 0)}


def group_reference(g):
    """the rays' reference (each ray against the triangles of its own case: the cases stand apart, `isolated` checks that) and the normal elements' (every triangle, 16 points,
    both sides)"""
    tris = g["tris"]
    nr = g["o"].shape[0]
    tr = {"prim": np.full(nr, MISS, np.uint32), "tuv": np.zeros((nr, 3)), "bound": np.zeros((nr, 3)), "compared": np.zeros(nr, bool), "miss": np.zeros(nr, bool)}
    for ci in range(len(g["cases"])):
        rs, ts = np.nonzero(g["ray_case"] == ci)[0], np.nonzero(g["tri_case"] == ci)[0]
        tgt = g["target"][rs]
        sub = trace_reference({k: tris[k][ts] for k in ("P", "eP")}, g["o"][rs], g["d"][rs], np.where(tgt == MISS, MISS, tgt - ts[0]))
        tr["prim"][rs] = np.where(sub["prim"] == MISS, MISS, sub["prim"] + ts[0]).astype(np.uint32)
        for k in ("tuv", "bound", "compared", "miss"):
            tr[k][rs] = sub[k]
    nt = tris["P"].shape[0]
    prim = np.repeat(np.arange(nt), 32)
    bary = np.tile(np.repeat(BARY, 2, axis=0), (nt, 1))
    side = np.tile(np.asarray([1.0, -1.0]), nt * 16)
    d = (g["d"][np.repeat(np.arange(nt * 16), 2)].astype(np.float64) * side[:, None]).astype(F)     # the ray's own direction, and from behind
    nm = {"prim": prim.astype(np.uint32), "bary": bary, "d": d, "Ns": np.zeros((prim.size, 3)), "bound": np.zeros((prim.size, 3)), "mapped": np.zeros(prim.size, bool),
          "compared": np.zeros(prim.size, bool), "degenerate": np.zeros(prim.size, bool), "has_map": g["tri_mesh"][prim] == "patch-mapped"}
    for has_map in (False, True):
        s = np.nonzero(nm["has_map"] == has_map)[0]
        r = normal_reference(tris, prim[s], bary[s], d[s], image=normal_image() if has_map else None, scale=NORMAL_SCALE)
        for k in ("Ns", "bound", "mapped", "compared", "degenerate"):
            nm[k][s] = r[k]
    return tr, nm


def isolated(g, margin=0.5):
    """no ray comes near a triangle of another case: within `margin` in barycentric units, at any t"""
    P = g["tris"]["P"]
    with np.errstate(all="ignore"):
        x = tuv(P[None], g["o"].astype(np.float64)[:, None], g["d"].astype(np.float64)[:, None])
    near = (x[..., 0] > 0) & (x[..., 1] > -margin) & (x[..., 2] > -margin) & (x[..., 1] + x[..., 2] < 1 + margin)
    return not np.any(near & (g["ray_case"][:, None] != g["tri_case"][None, :]))


def census(g, tr, nm):
    """per case: the excluded share of rays and of normal elements (degenerate cases: every ray is a compared miss, every normal a compared zero), and the least number
    of comparisons any triangle gets"""
    out = {}
    nt = g["tris"]["P"].shape[0]
    for ci, name in enumerate(g["cases"]):
        rs = g["ray_case"] == ci
        ts = np.nonzero(g["tri_case"] == ci)[0]
        ne = np.isin(nm["prim"], ts)
        ok_n = nm["compared"] | nm["degenerate"]
        per_tri_r = np.bincount(g["target"][rs & tr["compared"] & (g["target"] != MISS)], minlength=nt)[ts]
        per_tri_n = np.bincount(nm["prim"][ne & ok_n], minlength=nt)[ts]
        deg = g["degenerate"][ts]
        out[name] = {"rays": int(rs.sum()), "rays_excluded": float(1 - tr["compared"][rs].mean()), "normals": int(ne.sum()), "normals_excluded": float(1 - ok_n[ne].mean()),
                     "least_rays_per_triangle": int(np.where(deg, 16, per_tri_r).min()), "least_normals_per_triangle": int(per_tri_n.min())}
    return out


# ------------------------------------------------------------------ the checker
def worst(got, ref, bound, mask):
    """the largest |got − ref| / bound over the masked elements (0/0 = 0: an exact value met exactly); > TOL fails"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    mask = np.broadcast_to(np.asarray(mask).reshape(mask.shape + (1,) * (got.ndim - np.ndim(mask))), got.shape)
    diff = np.abs(got - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(diff == 0, 0.0, diff / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(np.where(mask, ratio, 0.0).max()) if got.size else 0.0


def _cases(g, of, ratio):
    """{case name: ratio(mask of the case's elements)}; `of` (n,) the case index of every element"""
    return {name: ratio(of == ci) for ci, name in enumerate(g["cases"])}


def check_bake(g, verts):
    """a bake's binary32 vertices ((3 nt,) of the lpt_vertex layout) against the binary64 bake -> per case the worst ratios (positions, normals); uv must be the mesh's, bit
    for bit, in the reference's vertex order"""
    tris = g["tris"]
    nt = tris["P"].shape[0]
    assert verts.shape[0] == 3 * nt
    pos = verts["position"].reshape(nt, 3, 4)
    nrm = verts["normal"].reshape(nt, 3, 4)
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(nrm))
    assert np.array_equal(pos[..., 3], tris["uv"][..., 0].astype(F)) and np.array_equal(nrm[..., 3], tris["uv"][..., 1].astype(F)), "uv do not follow the vertex order"
    with np.errstate(all="ignore"):
        tight = np.sqrt((tris["eN"] ** 2).sum(-1)) <= MAX_ANGLE
    for ci, name in enumerate(g["cases"]):
        assert 1 - tight[g["tri_case"] == ci].mean() <= MAX_EXCLUDED, name
    return _cases(g, g["tri_case"], lambda c: (worst(pos[..., :3], tris["P"], tris["eP"], np.broadcast_to(c[:, None], (nt, 3))),
                                               worst(nrm[..., :3], tris["N"], tris["eN"], tight & c[:, None])))


def check_woop(g, verts, rows):
    """a bake's Woop rows (nt, 3, 4) against binary64 rows of ITS OWN vertices -> per case the worst ratio; a degenerate triangle must give zeros exactly"""
    nt = rows.shape[0]
    ref, bound = woop_bound(verts["position"].reshape(nt, 3, 4)[..., :3])
    assert np.all(np.isfinite(rows))
    assert not np.any(rows[g["degenerate"]]), "Woop rows of a degenerate triangle must be zero"
    return _cases(g, g["tri_case"], lambda c: worst(rows, ref, bound, c))


def check_trace(g, tr, hits):
    """a probe's hits (t, u, v, prim) against the rays' reference -> per case the worst ratio over (t, u, v); prims must be the reference's on every compared ray, and the
    reconstructed point P0 + u·e1 + v·e2, in the reference's vertex order, must be the ray's point at t to within what the bounds of (t, u, v) and of the vertices allow"""
    c = tr["compared"]
    assert np.array_equal(hits["prim"][c], tr["prim"][c]), np.nonzero(c & (hits["prim"] != tr["prim"]))[0][:8]
    got = np.stack([hits["t"], hits["u"], hits["v"]], -1).astype(np.float64)
    assert np.all(np.isfinite(got))
    h = c & (tr["prim"] != MISS)
    assert not np.any(got[c & (tr["prim"] == MISS), 1:]), "a miss answers no barycentrics (its t is the search's upper end, finite)"
    P, eP = g["tris"]["P"][tr["prim"][h]], g["tris"]["eP"][tr["prim"][h]]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    o, d = g["o"][h].astype(np.float64), g["d"][h].astype(np.float64)
    t, u, v = got[h, 0:1], got[h, 1:2], got[h, 2:3]
    bt, bu, bv = (tr["bound"][h, k:k + 1] for k in range(3))
    gap = np.abs((P[:, 0] + u * e1 + v * e2) - (o + t * d))
    room = TOL * (bu * np.abs(e1) + bv * np.abs(e2) + bt * np.abs(d) + eP.sum(1))
    assert np.all(gap <= room), "the hit's (u, v) do not name the ray's point in the reference's vertex order"
    return _cases(g, g["ray_case"], lambda m: worst(got, tr["tuv"], tr["bound"], h & m))


def check_normals(g, nm, ns, mapped):
    """a probe's shading normals against the reference -> per case the worst ratio; `mapped` must agree where a map is in play; degenerate triangles answer zeros"""
    assert np.all(np.isfinite(ns))
    c = nm["compared"]
    assert np.array_equal(mapped[c & nm["has_map"]], nm["mapped"][c & nm["has_map"]])
    assert not np.any(mapped[~nm["has_map"]])
    assert not np.any(ns[nm["degenerate"]]), "a degenerate triangle must answer zeros"
    return _cases(g, g["tri_case"][nm["prim"]], lambda m: worst(ns, nm["Ns"], nm["bound"], c & m))


def passes(report):
    """every ratio of a {case: ratio or tuple of ratios} report is within TOL"""
    return all(np.all(np.asarray(v) <= TOL) for v in report.values())


@functools.lru_cache(maxsize=None)
def reference(name):
    """(group, rays' reference, normals' reference) of one scene of `groups()`, computed once per process and never written to"""
    g = build_group(groups()[name])
    tr, nm = group_reference(g)
    return g, tr, nm
