"""-m gpu: alpha-blended materials, SPEC.md §26 — glTF alphaMode BLEND as stochastic coverage, down to the traversal.

The reference never sees a blended scene.  Every quad ALONE, as an opaque scene, goes through the oracle's brute-force trace_closest, which gives the candidate
(t, u, v, prim) exactly as §7 accepts it; tests/blend_ref.py (numpy, written from the SPEC) decides each candidate from (prim, u, v) — prim being the id the triangle has
in the product's scene —; the nearest accepted one, or the wall behind, wins.  The product must return that hit bit for bit.  A candidate whose reference alpha lies within
1e-6 of its threshold (xi for a blended layer, the cutoff for a masked one) may be left out, EXCLUDE_CAP = 1 % at the most, asserted from the reference alone: xi is
uniform on a 2^-24 grid, so the share is about 2e-6 and in practice nothing is left out.

Frames are compared with frames, bit for bit (the two ends a = 1 and a = 0, every launch path), and where coverage is graded the counts are held to the binomial law
with the bounds written at the assertion."""
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A, testing as T

import alpha_ref as R
import blend_ref as B
from test_gpu_alpha_mask import (BOUNCES, DIR, EXCLUDE_CAP, EYE, GLB_DIR, GLB_EYE, LAYER_IMAGE, LAYER_Z, MISS, NEAR_CUTOFF, QUAD_IDX, SIZES, SPP, VARIANTS, WALL_N, Reference,
                                 _floor_blocks, _frame, _layer_mesh, _rays, _renderer, _wall_mesh, alpha_glb, png_bytes)

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = A.INVALID_INDEX
F = np.float32
N_WALL = 2 * WALL_N * WALL_N

# alpha in 4x4-texel blocks of a 16x16 image: LEVELS[by][bx]; a Latin square, so no row or column is uniform and every level has four blocks
LEVELS = np.array([[0, 64, 128, 255], [128, 255, 0, 64], [255, 128, 64, 0], [64, 0, 255, 128]], np.uint8)


def blend_texture():
    img = np.zeros((16, 16, 4), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 200, 180, 90
    img[..., 3] = np.kron(LEVELS, np.ones((4, 4), np.uint8))
    return img


def blend_glb(**kw):
    """tests/golden/alpha-blend.glb: the mask test's floor, quad and light, the quad's material BLEND with the graded texture"""
    return alpha_glb(mode="BLEND", image=png_bytes(blend_texture()), **kw)


def solid_texture():
    img = blend_texture()
    img[..., 3] = 255
    return img


# ---------------------------------------------------------------- the layered scene of tests 2-4 and 7: the mask test's wall and quads, two layers blended, two masked
BLENDED = (True, False, False, True)        # layer 0: graded image, blended; 1, 2: the same image against the cutoff; 3: no image, color.w = 0.3, blended
CUTOFF = 0.5


def blend_scene(image=None, blended=BLENDED, color_w=None, states=True, quads=True):
    """the wall first (prims 0..31), then the four quads (prims 32..39).  color_w: one color.w for every layer (default 1, and 0.3 for the layer without an image);
    states False: the same materials, all opaque"""
    s = lp.Scene()
    img = s.add_image(blend_texture() if image is None else image)
    nrm = lambda n: np.tile(np.array([[0, 0, 1]], np.float32), (n, 1))
    wpos, widx = _wall_mesh()
    s.add_instance(s.add_mesh(wpos, nrm(len(wpos)), None, widx), np.eye(4, dtype=np.float32), s.add_material((0.7, 0.7, 0.7, 1.0), 0.8, 0.0))
    for k in range(len(LAYER_Z) if quads else 0):
        pos, uv = _layer_mesh(k)
        blas = s.add_mesh(pos, nrm(4), uv, QUAD_IDX)
        w = (1.0 if LAYER_IMAGE[k] else 0.3) if color_w is None else color_w
        mat = s.add_material((0.9, 0.8, 0.7, w), 0.7, 0.0, albedo_texture=img if LAYER_IMAGE[k] else INVALID)
        if states and blended[k]:
            s.set_material_alpha(mat, "BLEND", alpha_image=img if LAYER_IMAGE[k] else INVALID)
        elif states:
            s.set_material_alpha(mat, A.ALPHA_MASK, CUTOFF, img if LAYER_IMAGE[k] else INVALID)
        s.add_instance(blas, np.eye(4, dtype=np.float32), mat)
    light = np.zeros(1, A.LIGHT_DT)
    light["normal"], light["tangent"], light["bitangent"], light["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.8), (0, 0, 1, 0.8), (0, 2.5, 1.0, 12.0)
    s.set_light(0, light)
    return s


class BlendReference(Reference):
    """the mask test's reference — per layer ALONE through the oracle's brute force, the nearest accepted layer or the wall — with §26 deciding the blended layers"""

    def __init__(self):
        super().__init__()
        self.image = blend_texture()

    def closest(self, o, d, blended=BLENDED, cutoff=CUTOFF):
        """-> (hits as HIT_DT, near: rays with a layer's alpha within NEAR_CUTOFF of its threshold, accepted layer hits [n, layers] as t or inf, coin: candidates that
        a blended layer decided with 0 < a < 1, and how many of them counted)"""
        best = self.wall.trace_closest(o, d, brute_force=True).copy()
        near = np.zeros(len(o), bool)
        ts = np.full((len(o), len(self.layers)), np.inf)
        coin = [0, 0]
        for k, (sc, uv) in enumerate(self.layers):
            h = sc.trace_closest(o, d, brute_force=True)
            hit = h["prim"] < 2
            prim = (N_WALL + 2 * k + h["prim"]).astype(np.uint32)
            a = np.zeros(len(o), F)
            for tri in range(2):
                m = hit & (h["prim"] == tri)
                a[m] = B.alpha(1.0 if LAYER_IMAGE[k] else 0.3, self.image if LAYER_IMAGE[k] else None, uv[tri], h["u"][m], h["v"][m])
            if blended[k]:
                x = B.xi(prim, h["u"], h["v"])
                near |= hit & (np.abs(a.astype(np.float64) - x.astype(np.float64)) <= NEAR_CUTOFF)
                ok = hit & B.counts(a, prim, h["u"], h["v"])
                graded = hit & (a > 0) & (a < 1)
                coin[0] += int(graded.sum())
                coin[1] += int((graded & ok).sum())
            else:
                near |= hit & (np.abs(a.astype(np.float64) - cutoff) <= NEAR_CUTOFF)
                ok = hit & R.counts(a, cutoff)
            ts[ok, k] = h["t"][ok]
            take = ok & ((h["t"] < best["t"]) | (best["prim"] == MISS))
            best["t"][take], best["u"][take], best["v"][take] = h["t"][take], h["u"][take], h["v"][take]
            best["prim"][take] = prim[take]
        return best, near, ts, coin


@pytest.fixture(scope="module")
def reference():
    return BlendReference()


@pytest.fixture(scope="module")
def ray_reference(reference):
    o, d = _rays()
    hits, near, ts, coin = reference.closest(o, d)
    wall_t = reference.wall.trace_closest(o, d, brute_force=True)["t"]
    return o, d, hits, near, ts, wall_t, coin


pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the decision, element by element
def _decision_scene():
    """one quad per material (prims 2 m, 2 m + 1), every way a blended material's alpha image can be stored, no image with color.w 0, 0.3 and 1, and one masked
    material so that both branches of the record's mode run in one table.  -> (scene, rows of (color.w, image or None, uv[2, 3, 2], blended))"""
    rng = np.random.default_rng(5)
    s = lp.Scene()
    graded = blend_texture()
    noisy = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)          # the size of `graded`: the two pair up as (albedo, mra)
    odd = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)              # 5x3: no multiple of the 8x4 tile, no power of two
    i_graded, i_noisy, i_odd, i_copy = s.add_image(graded), s.add_image(noisy), s.add_image(odd), s.add_image(noisy)
    images = {i_graded: graded, i_noisy: noisy, i_odd: odd, i_copy: noisy}
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    rows = []
    #        color.w, albedo,   mra,      alpha image, blended
    mats = [(1.0, i_graded, INVALID, i_graded, True),       # alone in the atlas, also the albedo
            (0.8, i_graded, i_noisy, i_graded, True),       # half of an (albedo, mra) pair: the alpha lookup reads its own resident copy
            (1.0, i_copy, i_graded, i_copy, True),          # the other order of the halves
            (0.9, INVALID, INVALID, i_odd, True),           # an image nothing else samples, of an odd size
            (0.0, INVALID, INVALID, INVALID, True), (0.3, INVALID, INVALID, INVALID, True), (1.0, INVALID, INVALID, INVALID, True),
            (1.0, i_noisy, INVALID, i_noisy, False),        # masked, cutoff 0.5
            (0.5, INVALID, INVALID, i_odd, True)]
    for m, (w, alb, mra, img, blended) in enumerate(mats):
        sc = (1.0, 2.5, 0.5, 1.0)[m % 4]
        pos = np.array([[-1, -1, -float(m)], [1, -1, -float(m)], [1, 1, -float(m)], [-1, 1, -float(m)]], np.float32)
        uv = np.array([[0.1, 0.2], [0.1 + sc, 0.2], [0.1 + sc, 0.2 + sc], [0.1, 0.2 + sc]], np.float32)
        mat = s.add_material((0.9, 0.8, 0.7, w), 0.7, 0.0, albedo_texture=alb, mra_texture=mra)
        if blended:
            s.set_material_alpha(mat, "BLEND", alpha_image=img)
        else:
            s.set_material_alpha(mat, A.ALPHA_MASK, CUTOFF, img)
        s.add_instance(s.add_mesh(pos, nrm, uv, QUAD_IDX), np.eye(4, dtype=np.float32), mat)
        rows.append((w, images.get(img), uv[QUAD_IDX].reshape(2, 3, 2), blended))
    return s, rows


def _barycentrics(n, rng):
    """interior points, the three edges, the three vertices, and zeros of either sign (bits(-0) differs from bits(+0): §26 hashes the pattern)"""
    u = rng.random(n, F)
    v = (rng.random(n, F) * (F(1.0) - u)).astype(F)
    kind = rng.integers(0, 12, n)
    u[kind == 6], v[kind == 7] = F(0.0), F(0.0)                                         # the edges u = 0 and v = 0
    e = kind == 8
    v[e] = F(1.0) - u[e]                                                                # the edge u + v = 1
    for k, (cu, cv) in ((9, (0.0, 0.0)), (10, (1.0, 0.0)), (11, (0.0, 1.0))):           # the vertices
        u[kind == k], v[kind == k] = F(cu), F(cv)
    neg = rng.random(n) < 0.5
    u[(u == 0) & neg] = F(-0.0)
    neg = rng.random(n) < 0.5
    v[(v == 0) & neg] = F(-0.0)
    return u, v


@pytest.mark.parametrize("kw", [{}, {"pair_textures": False}, {"gpu_build": True}], ids=["paired", "unpaired", "gpu_build"])
def test_the_decision_element_by_element(device, kw):
    scene, rows = _decision_scene()
    rng = np.random.default_rng(26)
    n = 4096
    prim = rng.integers(0, 2 * len(rows), n).astype(np.uint32)
    u, v = _barycentrics(n, rng)
    assert (np.signbit(u) & (u == 0)).sum() > 20 and (np.signbit(v) & (v == 0)).sum() > 20 and ((u == 0) & ~np.signbit(u)).sum() > 20
    a, thr, want = np.zeros(n, F), np.zeros(n, np.float64), np.zeros(n, bool)
    for m, (w, image, uv, blended) in enumerate(rows):
        for tri in range(2):
            sel = prim == 2 * m + tri
            a[sel] = B.alpha(w, image, uv[tri], u[sel], v[sel])
            thr[sel] = B.xi(prim[sel], u[sel], v[sel]) if blended else CUTOFF
            want[sel] = ~B.counts(a[sel], prim[sel], u[sel], v[sel]) if blended else ~R.counts(a[sel], CUTOFF)
    near = np.abs(a.astype(np.float64) - thr) <= NEAR_CUTOFF
    assert near.mean() <= EXCLUDE_CAP, near.mean()
    graded = (a > 0) & (a < 1)
    assert graded.sum() > 2000 and 0.3 < want[graded].mean() < 0.7, (int(graded.sum()), want[graded].mean())    # the decision is a coin where it should be one
    sg = lp.SceneGPU.new_from_scene(scene, device, **kw)
    got = sg.sample_textures(prim, np.c_[u, v])["rejected"]
    sg.close()
    bad = ~near & (got != want)
    assert not bad.any(), (int(bad.sum()), prim[bad][:8], u[bad][:8], v[bad][:8], a[bad][:8], thr[bad][:8])


# ---------------------------------------------------------------- 2. closest hit and any hit
@pytest.mark.parametrize("gpu_build", [False, True])
def test_closest_hit_matches_the_layered_reference(device, ray_reference, gpu_build):
    o, d, want, near, ts, _, coin = ray_reference
    assert near.mean() <= EXCLUDE_CAP, near.mean()
    layer = (want["prim"] >= N_WALL) & (want["prim"] != MISS)
    assert layer.sum() > 1000 and (np.isfinite(ts).sum(1) < (ts.shape[1] - 1)).sum() > 1000     # hits on quads, and candidates that did not count in front of them
    assert coin[0] > 1000 and 0.2 < coin[1] / coin[0] < 0.8, coin                                  # graded candidates on blended layers, decided both ways
    sg = lp.SceneGPU.new_from_scene(blend_scene(), device, gpu_build=gpu_build)
    got = sg.trace_closest(o, d)
    sg.close()
    keep = ~near
    for f in ("prim", "t", "u", "v"):
        bad = keep & (got[f].view(np.uint32) != want[f].view(np.uint32))
        assert not bad.any(), (f, int(bad.sum()), got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("gpu_build", [False, True])
def test_any_hit_matches_the_layered_reference(device, ray_reference, gpu_build):
    o, d, _, near, ts, wall_t, _ = ray_reference
    tmax = np.where(wall_t < 1e29, np.float32(0.999) * wall_t, np.float32(100.0)).astype(np.float32)    # the segment ends in front of the wall
    want = (ts <= tmax[:, None].astype(np.float64)).any(1)
    assert 0.2 < want.mean() < 0.9
    sg = lp.SceneGPU.new_from_scene(blend_scene(), device, gpu_build=gpu_build)
    got = sg.trace_occluded(o, d, tmax).astype(bool)
    sg.close()
    keep = ~near
    assert np.array_equal(got[keep], want[keep]), int((got[keep] != want[keep]).sum())


# ---------------------------------------------------------------- 3. the two ends, frame for frame on every launch path
ALL = (True, True, True, True)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_alpha_one_is_the_opaque_frame(device, size):
    """image alpha 255 and color.w = 1 on every blended material: a >= 1 > xi always"""
    want = _frame(device, blend_scene(image=solid_texture(), color_w=1.0, states=False), size)
    assert want[..., :3].max() > 0.05
    for v in VARIANTS:
        got = _frame(device, blend_scene(image=solid_texture(), blended=ALL, color_w=1.0), size, v)
        assert got.tobytes() == want.tobytes(), v


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_alpha_zero_is_the_frame_without_the_blended_instances(device, size):
    """color.w = 0: a <= 0 never counts, whatever the image says"""
    want = _frame(device, blend_scene(quads=False), size)
    for v in VARIANTS:
        got = _frame(device, blend_scene(blended=ALL, color_w=0.0), size, v)
        assert got.tobytes() == want.tobytes(), v


# ---------------------------------------------------------------- 4. one frame on every launch path, and the primary prim ids
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_primary_prim_ids_and_one_frame_on_every_launch_path(device, reference, size):
    from oracle import orc
    w, h = size
    view = T.look(EYE, DIR)
    seed = BOUNCES * (SPP - 1)      # a denoised frame is one sample; the seed counter moves by the depth per frame (SPEC §1)
    o, d = np.zeros((h * w, 3), np.float32), np.zeros((h * w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            o[y * w + x], d[y * w + x] = orc.raygen(w, h, view, T.VFOV, x, y, 0, seed)
    want, near, _, coin = reference.closest(o, d)
    assert near.mean() <= EXCLUDE_CAP, near.mean()
    prims = want["prim"].reshape(h, w)
    assert ((prims >= N_WALL) & (prims != MISS)).mean() > 0.05 and (prims < N_WALL).mean() > 0.05
    assert coin[0] > 200 and 0.2 < coin[1] / coin[0] < 0.8, coin
    scene = blend_scene()
    frames = [_frame(device, scene, size, v) for v in VARIANTS]
    for v, f in zip(VARIANTS, frames):
        assert f.tobytes() == frames[0].tobytes(), v
    assert frames[0].tobytes() != _frame(device, blend_scene(states=False), size).tobytes()
    for v in VARIANTS:
        g = _frame(device, scene, size, v, gbuffer=True)
        got = g[..., 0]
        keep = ~near.reshape(h, w)
        assert np.array_equal(got[keep], prims[keep]), (v, int((got[keep] != prims[keep]).sum()))


# ---------------------------------------------------------------- 5. coverage is a
COVER_SIZE, COVER_SPP = (64, 36), 16
COVER_EYE, COVER_DIR = (0.0, 0.0, 3.0), (0.0, 0.0, -1.0)
PROBE_E = 1.0
PROBE = np.array([[[128, 128, 128, 129]]], np.uint8)        # RGBE, SPEC §9: 128 * 2^(129 - 136) = 1 in every channel, everywhere


def _on_the_quad(w, h):
    """pixels whose whole jittered footprint (jitter in [0, 1)^2, so the closed pixel square) lands inside the quad |x|, |y| < 1 at z = 0, with a hundredth of a
    unit to spare (SPEC §11 in float64)"""
    v = np.asarray(T.look(COVER_EYE, COVER_DIR), np.float64).reshape(4, 4)
    right, up, fwd, origin = v[0, :3], v[1, :3], v[2, :3], v[3, :3]
    th = np.tan(T.VFOV / 2)
    ok = np.ones((h, w), bool)
    for jx in (0.0, 1.0):
        for jy in (0.0, 1.0):
            x, y = np.meshgrid(np.arange(w) + jx, np.arange(h) + jy)
            d = right * ((2 * x / w - 1) * (w / h * th))[..., None] + up * ((1 - 2 * y / h) * th)[..., None] + fwd
            P = origin + d * (-origin[2] / d[..., 2])[..., None]
            ok &= (np.abs(P[..., 0]) < 0.99) & (np.abs(P[..., 1]) < 0.99)
    return ok


@pytest.mark.parametrize("a", [0.25, 0.75])
def test_coverage_is_alpha(device, a):
    from oracle import gltf_oracle as G, orc
    w, h = COVER_SIZE
    pos = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    s = lp.Scene()
    mat = s.add_material((0.9, 0.8, 0.7, a), 0.7, 0.0)
    s.set_material_alpha(mat, "BLEND")
    s.add_instance(s.add_mesh(pos, np.tile(np.array([[0, 0, 1]], np.float32), (4, 1)), np.zeros((4, 2), np.float32), QUAD_IDX), np.eye(4, dtype=np.float32), mat)
    dark = np.zeros(1, A.LIGHT_DT)
    dark["normal"], dark["tangent"], dark["bitangent"], dark["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)
    s.set_light(0, dark)
    # the oracle's scene: the quad alone, opaque
    omat = np.zeros(1, G.MATERIAL_DT)
    omat["color"], omat["roughness"], omat["albedo_texture"], omat["mra_texture"] = 1.0, 1.0, INVALID, INVALID
    ov = np.zeros(6, G.VERTEX_DT)
    ov["position"][:, :3] = pos[QUAD_IDX]
    ov["normal"][:, 2] = 1.0
    odark = np.zeros(1, G.LIGHT_DT)
    odark["normal"], odark["tangent"], odark["bitangent"], odark["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)
    alone = orc.OracleScene(ov, np.zeros(2, np.uint32), omat, odark)

    sg = lp.SceneGPU.new_from_scene(s, device)
    pr = lp.ProbeGPU(device, PROBE, 1, 1)
    r = lp.Renderer(device, COVER_SIZE)
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, COVER_SIZE)
    r.set_max_bounces(1)            # a hit that counts adds nothing under the dark light; a ray that passes reads the probe: one Bernoulli trial per sample
    r.set_vfov(T.VFOV)
    r.reset_accumulation()
    r.accumulate = True
    view = T.look(COVER_EYE, COVER_DIR)
    M = accepted = 0
    try:
        for sample in range(COVER_SPP):
            o, d = r.primary_rays(view, sample)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
            cand = alone.trace_closest(o, d, brute_force=True)
            on = cand["prim"] < 2
            counts = on & B.counts(F(a), cand["prim"], cand["u"], cand["v"])          # the quad's triangles are prims 0 and 1 in the product's scene too
            got = sg.trace_closest(o, d)
            assert np.array_equal(got["prim"] != MISS, counts), (sample, int(((got["prim"] != MISS) != counts).sum()))
            for f in ("prim", "t", "u", "v"):
                assert np.array_equal(got[f][counts].view(np.uint32), cand[f][counts].view(np.uint32)), (sample, f)
            M += int(on.sum())
            accepted += int(counts.sum())
        r.raytrace_n(view, COVER_SPP)
        img = r.read_radiance()
    finally:
        r.close()
        pr.close()
        sg.close()
    # from the reference alone, first: the accepted share of the candidates within 5 binomial standard deviations of a
    sigma = np.sqrt(a * (1 - a) / M)
    print("a = %.2f: %d candidates, accepted share %.5f (%.2f sigma)" % (a, M, accepted / M, abs(accepted / M - a) / sigma))
    assert M > 10000 and abs(accepted / M - a) <= 5 * sigma, (M, accepted / M)
    # the frame: over the pixels that lie on the quad with their whole footprint, the mean luminance is (1 - a) E within the same law (K trials of weight E / K)
    inside = _on_the_quad(w, h)
    lum = img[..., :3].astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
    K = int(inside.sum()) * COVER_SPP
    mean = lum[inside].mean()
    print("a = %.2f: %d pixels, mean luminance %.5f against %.5f (%.2f sigma)" % (a, inside.sum(), mean, (1 - a) * PROBE_E, abs(mean - (1 - a) * PROBE_E) / (PROBE_E * np.sqrt(a * (1 - a) / K))))
    assert inside.sum() > 300 and abs(mean - (1 - a) * PROBE_E) <= 5 * np.sqrt(a * (1 - a) / K) * PROBE_E, (int(inside.sum()), mean)
    assert np.all(np.isin(np.round(lum[inside] * COVER_SPP / PROBE_E, 4), np.arange(COVER_SPP + 1)))     # every sample is 0 or E: coverage, not a tint


# ---------------------------------------------------------------- 6. a blended card casts a graded shadow
SHADOW_SIZE, SHADOW_SPP = (96, 64), 32


def _glb_frame(device, glb, blend=False):
    s = lp.Scene()
    lp.loaders.load_gltf(glb, s, blend=blend)
    dark = np.zeros(1, A.LIGHT_DT)
    dark["normal"], dark["tangent"], dark["bitangent"], dark["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)
    s.set_light(0, dark)
    sg = lp.SceneGPU.new_from_scene(s, device)
    r = lp.Renderer(device, SHADOW_SIZE)
    r.downsample_factor = 1.0
    r.resize(device, sg, None, SHADOW_SIZE)
    r.set_max_bounces(1)            # the primary hit and its shadow ray: nothing else reaches the quad from a floor pixel
    r.set_vfov(T.VFOV)
    r.reset_accumulation()
    r.accumulate = True
    for _ in range(SHADOW_SPP):
        r.raytrace(T.look(GLB_EYE, GLB_DIR))
    img = r.read_radiance()
    r.close()
    sg.close()
    return img


def test_a_blended_card_casts_a_graded_shadow(device):
    """Per block of the card's texture, over the floor pixels whose whole footprint lies under it: alpha 0 is the frame without the card and alpha 255 the frame
    under the solid card, bit for bit; alpha l in between lets the share 1 - l / 255 of the light through.  Each shadow ray is one Bernoulli trial with p = 1 - l / 255,
    so the ratio of the block's summed radiance to the same pixels of the card-less frame lies within 5 sqrt(p (1 - p) / K) of p, K = pixels x spp — were the
    unshadowed samples all equal.  They are not quite (the floor's BSDF varies over the block, and a sample that picks the scene's dark rectangle light instead of
    the directional one carries nothing in either frame), so the tolerance is widened by exactly the relative spread (standard deviation / mean) of the per-pixel
    values of the block in the card-less frame, as a factor 1 + spread."""
    with open(os.path.join(HERE, "golden", "alpha-blend.glb"), "rb") as f:
        committed = f.read()
    assert committed == blend_glb() and len(committed) < 16384       # the committed copy is this writer's output
    w, h = SHADOW_SIZE
    blended = _glb_frame(device, committed, blend=True)
    opaque = _glb_frame(device, committed)                            # loaded plainly, BLEND is opaque (SPEC §14 (7))
    without = _glb_frame(device, blend_glb(with_quad=False))
    block = _floor_blocks(w, h)
    level = np.where(block >= 0, LEVELS.reshape(-1)[np.maximum(block, 0)].astype(int), -1)
    clear, solid = level == 0, level == 255
    assert clear.sum() >= 4 and solid.sum() >= 4, (int(clear.sum()), int(solid.sum()))
    assert np.array_equal(blended[clear], without[clear]) and blended[clear][:, :3].mean() > 0.01       # lit, exactly as if the card were not there
    assert np.array_equal(blended[solid], opaque[solid]) and blended[solid][:, :3].max() == 0           # shadowed, exactly as under the solid card: no probe, depth 1
    graded = (level == 64) | (level == 128)
    assert not np.array_equal(blended[graded], opaque[graded])                                           # the plain load casts a solid shadow there
    checked = {64: 0, 128: 0}
    for b in np.unique(block[graded]):
        sel = block == b
        l = int(LEVELS.reshape(-1)[b])
        p = 1.0 - l / 255.0
        K = int(sel.sum()) * SHADOW_SPP
        base = without[sel][:, :3].astype(np.float64).sum(1)
        spread = base.std() / base.mean()
        ratio = blended[sel][:, :3].astype(np.float64).sum() / base.sum()
        tol = 5 * np.sqrt(p * (1 - p) / K) * (1 + spread)
        print("block %2d alpha %3d: %2d pixels, ratio %.4f against %.4f, tolerance %.4f (spread %.3f)" % (b, l, sel.sum(), ratio, p, tol, spread))
        assert abs(ratio - p) <= tol, (int(b), l, int(sel.sum()), ratio, p, tol)
        checked[l] += 1
    assert checked[64] >= 2 and checked[128] >= 2, checked


# ---------------------------------------------------------------- 7. refit and rebuild
def test_refit_and_rebuild_keep_the_blend(device):
    size = (64, 36)
    moved = np.eye(4, dtype=np.float32)
    moved[:3, 3] = (0.35, -0.2, 0.4)          # column-major below: the translation goes to elements 12..14
    scene = blend_scene()
    inst = scene.counts().instances - 4       # the first quad: blended, with the graded image
    fresh_scene = blend_scene()
    fresh_scene.set_instance_transform(inst, moved.T)
    want = _frame(device, fresh_scene, size)
    assert want.tobytes() != _frame(device, scene, size).tobytes()

    sg = lp.SceneGPU.new_from_scene(scene, device)
    scene.set_instance_transform(inst, moved.T)
    view = T.look(EYE, DIR)

    def frame():
        r = _renderer(device, sg, size, "default")
        r.reset_accumulation()
        r.accumulate = True
        for _ in range(SPP):
            r.raytrace(view)
        img = r.read_radiance()
        r.close()
        return img

    sg.update_instances(scene)
    assert frame().tobytes() == want.tobytes()
    sg.rebuild(scene)
    assert frame().tobytes() == want.tobytes()
    # a blended material that becomes masked, then opaque: the rebuild re-derives the record's mode and then drops the table
    first = scene.counts().materials - 4
    scene.set_material_alpha(first, A.ALPHA_MASK, CUTOFF, 0)
    sg.rebuild(scene)
    masked = blend_scene(blended=(False, False, False, True))
    masked.set_instance_transform(inst, moved.T)
    assert frame().tobytes() == _frame(device, masked, size).tobytes()
    for m in range(scene.counts().materials):
        scene.set_material_alpha(m, "OPAQUE")
    sg.rebuild(scene)
    opaque = blend_scene(states=False)
    opaque.set_instance_transform(inst, moved.T)
    assert frame().tobytes() == _frame(device, opaque, size).tobytes()
    sg.close()
