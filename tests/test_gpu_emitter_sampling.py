"""-m gpu: emitter sampling (SPEC.md §23) on the device.  The kernels' own emitter_sample against tests/emitter_ref.py; the expectation of a frame unchanged by the
switch and its noise lower (depth 2, depth 3 in a box, with every other light kind, through a pane, an emitter that is also alpha-masked, a glTF file); depth 1 and
scenes without emitters bit-identical; a closed form that does not lean on §22; bit-identity across the forms of the frame pipeline, the G-buffer and the motion
record included; the distribution following instance edits."""
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

import emissive_ref as E
import emitter_ref as R
from emitter_scenes import Built, QUAD_IDX, dark_light, many_scene, scaled
from test_gpu_emissive import FLOOR, add_quad, emissive_glb, texture4, GLB_CAMERA
from test_gpu_transmission import Rig, add_rect, atrium_small, frame_of  # noqa: F401 (atrium_small: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 64, 36
U = 2.0 ** -24
F = np.float32
BLACK = np.zeros((1, 1, 4), np.uint8)
WINDOW = (slice(8, 28), slice(12, 52))
CAM = dict(eye=(0.0, 1.0, 0.5), direction=(0.0, -0.7, -1.0))
LAMP = dict(center=(0.0, 1.5, -3.0), u=(1, 0, 0), v=(0, 0, 1), hu=0.5, hv=0.5)
LE = 8.0


class ERig(Rig):
    def __init__(self, *a, sampling=None, sort=None, **kw):
        super().__init__(*a, **kw)
        if sampling is not None:
            self.r.set_emissive_sampling(sampling)
        if sort is not None:
            self.r.set_sort_queues(sort)


def eframe(device, scene, probe, n=4, **kw):
    rig = ERig(device, scene, probe, **kw)
    img = rig.frame(n)
    rig.close()
    return img


WALL = 0.8
BACK_WALL = dict(center=(0.0, 2.0, -4.5), u=(1, 0, 0), v=(0, 1, 0), hu=4.0, hv=2.0)      # faces +z
SIDE_WALL = dict(center=(-1.5, 2.0, -3.0), u=(0, 1, 0), v=(0, 0, 1), hu=2.0, hv=4.0)     # faces +x


def half_mask():
    """a 4 x 4 alpha image, two columns 0 and two 255: with §9's bilinear repeat lookup and the cutoff 0.5 exactly half of a quad with uv over [0, 1]^2 is cut away"""
    img = np.full((4, 4, 4), 255, np.uint8)
    img[:, :2, 3] = 0
    return img


def lamp_floor(walls=False, rect_light=False, point=False, pane=False, le=LE, masked=False):
    """the scene of test_gpu_emissive's rectangle-light test: a 1 x 1 emissive quad (black base) 1.5 above a white floor, light 0 dark"""
    s = lp.Scene()
    s.set_light(0, dark_light())
    m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(m, (1.0, 1.0, 1.0), le)
    if masked:      # the same quad with uv over [0, 1]^2 and §20's mask over half of it: a neon sign
        s.set_material_alpha(m, "MASK", 0.5, s.add_image(half_mask()))
        add_quad(s, mat=m, **LAMP)
    else:
        add_rect(s, mat=m, **LAMP)
    white = s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0)
    add_rect(s, mat=white, **FLOOR)
    if walls:       # a back wall facing +z and a side wall facing +x: with the floor a corner that keeps paths alive to the last bounce
        grey = s.add_material((WALL, WALL, WALL, 1.0), 1.0, 0.0)
        add_rect(s, mat=grey, **BACK_WALL)
        add_rect(s, mat=grey, **SIDE_WALL)
    if rect_light:
        l = np.zeros(1, lp._abi.LIGHT_DT)
        l["normal"], l["tangent"], l["bitangent"], l["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.3), (0, 0, 1, 0.3), (1.2, 1.5, -2.5, 3.0)
        s.add_light(l)
    if point:
        s.add_punctual_light(lp.point_light((-1.0, 1.0, -2.0), (1.0, 0.9, 0.8), 2.0))
    if pane:        # a thin glass pane between the camera and the floor
        g = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
        s.set_material_transmission(g, 1.0, 1.5, True)
        add_rect(s, (0.0, 0.7, 0.0), (1, 0, 0), (0, 0.82, -0.57), 1.0, 0.6, g)
    return s


def arms(device, scene, probe=BLACK, K=16, N=64, window=WINDOW, size=(W, H), **kw):
    """K batches of N spp per arm -> {arm: (mean, se)} of the window mean, the standard errors from the batch means (user seeds 300 + k off, 400 + k on)"""
    out = {}
    for on in (False, True):
        rig = ERig(device, scene, probe, size=size, sampling=on, **kw)
        batch = []
        for k in range(K):
            rig.r.set_seed((400 if on else 300) + k)
            rig.r.reset_accumulation()
            rig.r.accumulate = True
            rig.r.raytrace_n(rig.view, N)
            img = rig.r.read_radiance()[..., :3]
            assert np.all(np.isfinite(img))
            batch.append(float(img[window].mean()))
        rig.close()
        b = np.array(batch)
        out[on] = (b.mean(), b.std(ddof=1) / np.sqrt(K))
    return out


def agree(a, what, lower=True):
    (m0, s0), (m1, s1) = a[False], a[True]
    print("%s: off %.5f +- %.5f, on %.5f +- %.5f, |difference| / bound %.2f, se_off / se_on %.2f" % (what, m0, s0, m1, s1, abs(m1 - m0) / (5 * np.hypot(s0, s1)), s0 / s1))
    assert m0 > 0 and abs(m1 - m0) <= 5 * np.hypot(s0, s1), (m0, m1, s0, s1)
    if lower:
        assert s1 < s0, (s1, s0)
    return 5 * np.hypot(s0, s1)


# ---------------------------------------------------------------- 0. the switch
def test_switch_round_trips(device):
    rig = ERig(device, lamp_floor(), BLACK)
    assert rig.r.get_emissive_sampling() is False
    rig.r.set_emissive_sampling(True)
    assert rig.r.get_emissive_sampling() is True
    rig.r.set_emissive_sampling(False)
    assert rig.r.get_emissive_sampling() is False
    rig.close()


# ---------------------------------------------------------------- 1. the sampler against the reference
def _edges(b, dist, ref_tris, n_e, rs):
    """the edge rows of (rands, Po): the clamp of the slot, rb on either side of q, r1 = 0, Po in the picked triangle's plane, Po = y"""
    rows, pts = [], []
    one_m = np.nextafter(F(1.0), F(0.0))
    rows.append((one_m, 0.5, 0.3, 0.3)); pts.append((0.0, 0.0, 0.0))                     # int(ra n_e) = n_e in binary32 for n_e = 130: the clamp
    for s in range(min(n_e, 8)):
        ra, q = F((s + 0.5) / n_e), dist["q"][s]
        rows += [(ra, np.nextafter(q, F(0.0)), 0.4, 0.6), (ra, q, 0.4, 0.6), (ra, 0.0, 0.0, 0.7)]
        pts += [(0.2, 0.1, -0.5)] * 3
        t = ref_tris[dist["prim"][s]].astype(F)
        inplane = (t[0] + F(0.3) * (t[1] - t[0])) + F(2.0) * (t[2] - t[0])                # in the plane (up to binary32), outside the triangle
        rows.append((ra, 0.0, 0.25, 0.5)); pts.append(tuple(inplane))
    rands, Po = np.array(rows, F), np.array(pts, F)
    # Po = y: the reference's own binary32 point for the same draws
    k = len(rands)
    extra = rs.uniform(0, 1, (16, 4)).astype(F)
    y32 = R.sample(dist, ref_tris, np.array(b.uv, F), b.rec, b.images, extra, np.zeros((16, 3), F), F)["y"].astype(F)
    return np.concatenate([rands, extra]), np.concatenate([Po, y32]), slice(k, k + 16)


@pytest.mark.parametrize("n_e", [1, 2, 130])
def test_sampler_equals_the_reference(device, n_e):
    """THE BOUNDS, derived per sample from the operation count and the operands' magnitudes (u = 2^-24), not tuned.  M = the largest |coordinate| of the triangle.
     * barycentrics: su 1 rounding; u = su (1 - r2): 3u; v = su r2: 2u; bw = (1 - u) - v: those 5u and 2 roundings, 7u absolutely.
     * y = (p0 bw + p1 u) + p2 v: sum |p_k| db_k <= 12 u M, three products u M (bw + u + v = 1), two sums 2 u M: 15 u M; K_Y = 16.
     * w = y - Po: e_w = dy + u |w|.  dist: sqrt(3) e_w + 4 u dist (three roundings of a sum of squares, halved by the root, and the root's own).
       wi = w (1 / dist): (1 + sqrt(3)) e_w / dist + 6u.
     * Ng = cross(a, b) of the binary32 edges: 5 u |a| |b| per component (edges 1u each, two products, one difference); rel_ng = sqrt(3) that / |Ng|.
       cl = |Ng . wi| / |Ng|: numerator rel_ng + sqrt(3) dwi + 3u, denominator rel_ng + 3u on cl <= 1, two products: 2 rel_ng + sqrt(3) dwi + 8u.
     * p_A = lum(Le) inv_W: three binary32 constants, three products, two sums of non-negative terms, inv_W's rounding and the product: 10 u relative.
     * E: Le exactly without an image; with one, tests/test_gpu_emissive.py's K_ROUND = 12 roundings of §9 and the slope of the lookup times how far its position
       may move: tu by uv_max (12u) + 6 u uv_max, fx = tu W - 0.5 by W times that + 2u (W uv_max + 0.5).
    Measured on an MI355X: see DESIGN §5.2f."""
    img = texture4()
    b = many_scene(n_e, image=img)
    dist = b.reference()
    tris, uvs = np.array(b.tris, F), np.array(b.uv, F)
    sg = lp.SceneGPU.new_from_scene(b.s, device)
    rs = np.random.RandomState(7 + n_e)
    n = 4096
    rands, Po = rs.uniform(0, 1, (n, 4)).astype(F), (rs.uniform(-2, 2, (n, 3)) + (0, 0, -3)).astype(F)
    er, ep, same = _edges(b, dist, tris, n_e, rs)
    rands, Po = np.concatenate([rands, er]), np.concatenate([Po, ep])
    got = sg.sample_emitter(Po, rands)
    sg.close()
    r32 = R.sample(dist, tris, uvs, b.rec, b.images, rands, Po, F)
    r64 = R.sample(dist, tris, uvs, b.rec, b.images, rands, Po, np.float64)
    assert np.array_equal(got["prim"], r32["prim"])                                  # the pick: exact
    assert np.array_equal(got["sampled"], r32["ok"])                                 # and every "no sample" decision, as binary32 makes it
    assert not r32["ok"][n:][same].any()                                             # Po = y gives no sample
    if n_e == 130:
        assert got["prim"][n] == dist["prim"][[n_e - 1, dist["alias"][n_e - 1]][0 if 0.5 < dist["q"][n_e - 1] else 1]]
        assert len(np.unique(got["prim"])) > 100 and len({id(b.rec[p]) for p in np.unique(got["prim"])}) == 3
    ok = r32["ok"] & r64["ok"]
    assert ok.sum() > 0.9 * n and np.all(np.stack([got[k].reshape(len(ok), -1).any(1) for k in ("y", "wi", "dist", "cl", "p_a", "E")])[:, ~r32["ok"]] == 0)
    t = tris.astype(np.float64)[r64["prim"].astype(np.int64)]
    M = np.abs(t).max((1, 2))
    a, bb = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    ng = np.cross(a, bb)
    e_y = 16 * U * M
    wv = r64["y"] - Po
    e_w = e_y + U * np.abs(wv).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_dist = np.sqrt(3) * e_w + 4 * U * r64["dist"]
        e_wi = (1 + np.sqrt(3)) * e_w / r64["dist"] + 6 * U
        rel_ng = np.sqrt(3) * 5 * U * np.linalg.norm(a, axis=1) * np.linalg.norm(bb, axis=1) / np.linalg.norm(ng, axis=1)
        e_cl = 2 * rel_ng + np.sqrt(3) * e_wi + 8 * U
    e_pa = 10 * U * r64["p_a"]
    uv_max, size = 2.5, img.shape[0]
    d_f = size * (uv_max * 12 * U + 6 * U * uv_max) + 2 * U * (size * uv_max + 0.5)
    gx, gy = E.steepest(img)
    le = np.array([np.zeros(3) if b.rec[p] is None else b.rec[p][0] for p in r64["prim"]], np.float64)
    has = np.array([b.rec[p] is not None and b.rec[p][1] is not None for p in r64["prim"]])
    e_E = np.where(has[:, None], 12 * U * np.abs(r64["E"]) + (gx + gy) * d_f * le, 0.0)
    worst = {}
    for key, bound in (("y", e_y[:, None]), ("wi", e_wi[:, None]), ("dist", e_dist), ("cl", e_cl), ("p_a", e_pa), ("E", e_E)):
        err = np.abs(got[key].astype(np.float64) - r64[key])[ok]
        bd = np.broadcast_to(bound, got[key].shape)[ok]
        worst[key] = float((err / np.maximum(bd, 1e-300)).max()) if bd.max() > 0 else float(err.max())
        assert np.all(err <= bd), (key, worst[key])
    print("n_e %d: %d samples, %d without one; largest error / bound: %s" % (n_e, len(ok), (~r32["ok"]).sum(), ", ".join("%s %.3g" % kv for kv in worst.items())))


# ---------------------------------------------------------------- 2. the expectation is unchanged, the noise is lower
def test_expectation_unchanged_depth_2(device):
    """arm off = §22 (BSDF paths only), arm on = emitter sampling; depth 2, 64x36, K = 16 batches of N = 64 spp; the window means agree within 5 hypot(se_on, se_off)
    and se_on < se_off.  Measured on an MI355X: see DESIGN §5.2f."""
    agree(arms(device, lamp_floor(), depth=2, **CAM), "depth 2")


# ---------------------------------------------------------------- 3. depth 3 in a corner: the last bounce draws no emitter sample
def test_expectation_unchanged_depth_3_in_a_box(device):
    """as above at depth 3 with two diffuse walls: paths reach the last bounce on a surface, where §23 draws no emitter sample.

    THAT THIS TEST SEES A WRONG RULE.  An emitter sample drawn at the last hit with weight 1 would add the whole next term of the light transport — emitter, a surface,
    two more surfaces, camera: one segment more than §22 ever adds — to the mean of arm on.  tests/emitter_ref.py's last_bounce_shift estimates that term's window mean
    for this scene in binary64 (128 paths per window pixel, §10's BSDF, the last vertex's direct light by quadrature; the same estimator gives 0.14983 for the depth-1
    term, the quadrature of the closed-form test, and 0.0265 for the depth-2 term, the difference of the two rendered means): 0.0216 +- 0.0003.  The agreement bound
    5 hypot(se_on, se_off) measures 0.0053 on an MI355X, so the shift is 4 times the bound.  Asserted below with the shift's own 5 standard errors taken off:
    at least 3 times the bound, which leaves a frame with the wrong rule 10 standard errors of the difference outside what `agree` accepts."""
    bound = agree(arms(device, lamp_floor(walls=True), depth=3, **CAM), "depth 3, box")
    lamp = R.rect(LAMP["center"], LAMP["u"], LAMP["v"], LAMP["hu"], LAMP["hv"], 0.0, LE)
    rects = [lamp, R.rect(albedo=1.0, **FLOOR), R.rect(albedo=WALL, **BACK_WALL), R.rect(albedo=WALL, **SIDE_WALL)]
    shift, se = R.last_bounce_shift(T.look(CAM["eye"], CAM["direction"]), 0.6, W, H, WINDOW[0], WINDOW[1], rects, lamp, depth=3, spp=128)
    print("a weight-1 sample on the last bounce would shift the mean by %.5f +- %.5f = %.2f x the bound %.5f" % (shift, se, shift / bound, bound))
    assert shift - 5 * se >= 3 * bound, (shift, se, bound)


# ---------------------------------------------------------------- 4. depth 1
def test_depth_1_is_bit_identical(device):
    kw = dict(n=2, size=(W, H), depth=1, eye=(0.0, 0.4, 0.5), direction=(0.0, 0.25, -1.0))
    off, on = eframe(device, lamp_floor(), BLACK, sampling=False, **kw), eframe(device, lamp_floor(), BLACK, sampling=True, **kw)
    assert off[..., :3].max() == np.float32(LE) and on.tobytes() == off.tobytes()


# ---------------------------------------------------------------- 5. against a closed form
def test_floor_against_the_quadrature(device):
    """arm on, depth 2, the camera sees only the floor: the window mean against emitter_ref's binary64 integral of f Le cos cos' / r^2 over the emitter, averaged over
    the window's pixels, within 5 se + the quadrature's stated error.  f is §10's BSDF of the white floor (roughness 1, metallic 0): the renderer has no purely
    Lambertian material, so the closed form carries §10's Fresnel term beside albedo / pi (emitter_ref.bsdf_f); the Lambert figure is printed beside it.  This check
    does not lean on §22."""
    K, N = 16, 64
    rig = ERig(device, lamp_floor(), BLACK, size=(W, H), depth=2, sampling=True, **CAM)
    batch = []
    for k in range(K):
        rig.r.set_seed(500 + k)
        rig.r.reset_accumulation()
        rig.r.accumulate = True
        rig.r.raytrace_n(rig.view, N)
        batch.append(float(rig.r.read_radiance()[..., :3][WINDOW].mean()))
    view = rig.view
    rig.close()
    m, se = np.mean(batch), np.std(batch, ddof=1) / np.sqrt(K)
    em = dict(center=LAMP["center"], eu=LAMP["u"], ev=LAMP["v"], hu=LAMP["hu"], hv=LAMP["hv"])
    want, qerr = R.floor_window_mean(view, 0.6, W, H, WINDOW[0], WINDOW[1], 0.0, 1.0, em, LE)
    lambert, _ = R.floor_window_mean(view, 0.6, W, H, WINDOW[0], WINDOW[1], 0.0, 1.0, em, LE, lambert=True)
    print("closed form: rendered %.5f +- %.5f, integral %.5f (quadrature error %.2g; Lambert alone %.5f), |difference| / bound %.2f" % (m, se, want, qerr, lambert, abs(m - want) / (5 * se + qerr)))
    assert abs(m - want) <= 5 * se + qerr, (m, se, want, qerr)


# ---------------------------------------------------------------- 6. shares: every other light kind beside the emitters
@pytest.mark.parametrize("pane", [False, True], ids=["env_punct_emis", "env_punct_trans_emis"])
def test_shares_with_every_light_kind(device, pane):
    """a lit rectangle light, a point light and §18 over a constant probe beside the emitter: the instantiation ENV, PUNCT, EMIS (and TRANS with the pane)"""
    grey = np.zeros((2, 4, 4), np.uint8)
    grey[...] = (128, 128, 128, 127)           # RGBE: 0.25 everywhere
    s = lamp_floor(rect_light=True, point=True, pane=pane)
    agree(arms(device, s, probe=grey, depth=2, env=True, **CAM), "shares, pane %s" % pane, lower=False)


# ---------------------------------------------------------------- 6b. an emitter that is also alpha-masked (SPEC §20)
def test_a_masked_emitter_keeps_its_expectation(device):
    """the lamp with half of it cut away by its own alpha mask.  Under §22 a BSDF ray passes through the cut half and adds nothing; §23 gives no sample at a point the mask
    rejects.  A sampler that ignored the mask would light the floor with the whole quad: arm on at twice arm off (0.15 against 0.075), some 30 times the bound."""
    a = arms(device, lamp_floor(masked=True), depth=2, **CAM)
    agree(a, "masked emitter")
    whole = 0.14983      # the unmasked lamp's direct light in this window (the closed-form test); half the lamp, less than the whole and more than none
    assert 0.3 * whole < a[True][0] < 0.7 * whole, a


def test_sampler_gives_no_sample_where_the_mask_rejects(device):
    """lpt_scene_gpu_sample_emitter over a masked emissive quad: every "no sample" decision equals the reference's, which asks tests/alpha_ref.py at the sampled point"""
    b = Built()
    mask = half_mask()
    mat = b.material((2.0, 1.0, 4.0))
    b.s.set_material_alpha(mat[0], "MASK", 0.5, b.image(mask))
    pos = F([[-0.5, 1.5, -3.5], [0.5, 1.5, -3.5], [0.5, 1.5, -2.5], [-0.5, 1.5, -2.5]])
    b.mesh(pos, QUAD_IDX, mat, uv=F([[0, 0], [1.7, 0], [1.7, 1.3], [0, 1.3]]))
    dist = b.reference()
    tris, uvs = np.array(b.tris, F), np.array(b.uv, F)
    rs = np.random.RandomState(5)
    n = 4096
    rands, Po = rs.uniform(0, 1, (n, 4)).astype(F), (rs.uniform(-2, 2, (n, 3)) + (0, 0, -3)).astype(F)
    sg = lp.SceneGPU.new_from_scene(b.s, device)
    got = sg.sample_emitter(Po, rands)
    sg.close()
    tri_mask = [(0.5, 1.0, mask)] * 2
    r32 = R.sample(dist, tris, uvs, b.rec, b.images, rands, Po, F, tri_mask=tri_mask)
    plain = R.sample(dist, tris, uvs, b.rec, b.images, rands, Po, F)
    cut = plain["ok"] & ~r32["ok"]
    print("masked sampler: %d of %d samples cut away by the mask" % (cut.sum(), n))
    assert 0.3 * n < cut.sum() < 0.7 * n
    assert np.array_equal(got["prim"], r32["prim"]) and np.array_equal(got["sampled"], r32["ok"])
    assert np.all(got["y"][~r32["ok"]] == 0) and np.all(np.abs(got["y"][r32["ok"]] - r32["y"][r32["ok"]]) <= 16 * U * 3.5)      # y's bound of the sampler test, M = 3.5


# ---------------------------------------------------------------- 7. nothing else moved
def test_switch_changes_nothing_without_emitters_and_off_is_the_parent(device, atrium_small):
    desc = atrium_small
    kw = dict(n=2, size=(96, 64), depth=3, vfov=T.VFOV, eye=desc["camera"]["origin"], direction=desc["camera"]["direction"])
    plain = scenes.to_product(desc)
    assert eframe(device, plain, desc.get("probe"), sampling=True, **kw).tobytes() == eframe(device, plain, desc.get("probe"), **kw).tobytes()
    kw = dict(n=2, size=(W, H), depth=3, **CAM)
    never, off = eframe(device, lamp_floor(walls=True), BLACK, **kw), eframe(device, lamp_floor(walls=True), BLACK, sampling=False, **kw)
    assert never[..., :3].any() and never.tobytes() == off.tobytes()
    assert eframe(device, lamp_floor(walls=True), BLACK, sampling=True, **kw).tobytes() != off.tobytes()


# ---------------------------------------------------------------- 8. launch invariance with the switch on
@pytest.mark.parametrize("size,n", [((32, 18), 1), ((64, 36), 4)], ids=["coop_all", "larger"])
def test_launch_invariance(device, size, n):
    scene = lamp_floor(walls=True, point=True)
    sg = lp.SceneGPU.new_from_scene(scene, device)
    kw = dict(size=size, depth=3, sg=sg, sampling=True, **CAM)
    rig = ERig(device, scene, BLACK, **kw)
    rig.r.reset_accumulation()
    rig.r.accumulate = True
    rig.r.raytrace_n(rig.view, n)
    want = rig.r.read_radiance()
    rig.close()
    assert np.all(np.isfinite(want)) and want[..., :3].any()
    for v in (dict(options={"coop_rays": 0}), dict(sort=0), dict(sort=3), dict(options={"packet_primary": 0}), dict(options={"tail_lanes": 0}),
              dict(options={"path_rays": 0x7FFFFFFF, "coop_rays": 0})):
        assert eframe(device, scene, BLACK, n=n, **kw, **v).tobytes() == want.tobytes(), v      # n raytrace calls against one raytrace_n
    acc = np.zeros_like(want)
    for rank in range(2):
        acc += eframe(device, scene, BLACK, n=n, rank=rank, world=2, **kw)
    assert acc.tobytes() == want.tobytes()
    # a denoised mode with the switch on: two frames, one renderer against two tile shards exchanged (the G-buffer and the motion travel with the radiance)
    for mode in (lp.BlitMode.DenoisedPathrace,):
        one = ERig(device, scene, BLACK, mode=mode, **kw)
        ranks = [ERig(device, scene, BLACK, mode=mode, rank=q, world=2, **kw) for q in range(2)]
        for f in range(2):
            one.r.raytrace(one.view)
            for r in ranks:
                r.r.raytrace(one.view)
            ranks[0].r.exchange_local([r.r for r in ranks[1:]])
            got, ref = ranks[0].r.read_radiance(), one.r.read_radiance()
            assert np.all(np.isfinite(ref)) and got.tobytes() == ref.tobytes(), (mode, f)
        for r in [one] + ranks:
            r.close()
    sg.close()


def test_gbuffer_and_motion_are_those_of_the_switch_off(device):
    """a denoised mode over the emissive scene, the switch on against off: the G-buffer and the motion record of every frame equal bit for bit (SPEC §23: the G-buffer is
    §22's; the GBUF, ESAMP instantiations write it), over two frames with the camera moved between them so that the motion is not zero; the radiance differs"""
    scene = lamp_floor(walls=True, point=True)
    sg = lp.SceneGPU.new_from_scene(scene, device)
    views = [T.look(CAM["eye"], CAM["direction"]), T.look((0.1, 1.05, 0.45), (0.03, -0.7, -1.0))]
    for mode in (lp.BlitMode.DenoisedPathrace, lp.BlitMode.Temporal):
        rigs = {on: ERig(device, scene, BLACK, size=(W, H), depth=3, sg=sg, sampling=on, mode=mode, **CAM) for on in (False, True)}
        differs = False
        for f, view in enumerate(views):
            out = {}
            for on, rig in rigs.items():
                rig.r.raytrace(view)
                out[on] = rig.r.read_denoiser()
            (g0, m0, rad0, _), (g1, m1, rad1, _) = out[False], out[True]
            assert g0.any() and (f == 0 or m0.any())
            assert g1.tobytes() == g0.tobytes() and m1.tobytes() == m0.tobytes(), (mode, f)
            differs |= rad1.tobytes() != rad0.tobytes()
        assert differs, mode
        for rig in rigs.values():
            rig.close()
    sg.close()


# ---------------------------------------------------------------- 9. refit and rebuild
def test_distribution_follows_instance_edits(device):
    kw = dict(n=2, size=(W, H), depth=2, sampling=True, **CAM)

    def scene(edit):
        s = lamp_floor()
        if edit:
            s.set_instance_transform(1, scaled(1.5, (0.4, -0.6, -1.2)))       # the emitter (instance 1) moved and scaled about the origin
        return s

    fresh, fresh_edited = eframe(device, scene(False), BLACK, **kw), eframe(device, scene(True), BLACK, **kw)
    assert fresh.tobytes() != fresh_edited.tobytes()
    s = scene(False)
    sg = lp.SceneGPU.new_from_scene(s, device)
    s.set_instance_transform(1, scaled(1.5, (0.4, -0.6, -1.2)))
    assert sg.update_instances(s) == 1
    assert eframe(device, s, BLACK, sg=sg, **kw).tobytes() == fresh_edited.tobytes()
    s.set_instance_transform(1, np.eye(4, dtype=np.float32))
    sg.rebuild(s)
    assert eframe(device, s, BLACK, sg=sg, **kw).tobytes() == fresh.tobytes()
    sg.close()


# ---------------------------------------------------------------- 10. glTF
def test_gltf_panel_with_the_switch(device):
    with open(os.path.join(HERE, "golden", "emissive-panel.glb"), "rb") as f:
        s = lp.Scene()
        lp.loaders.load_gltf(f.read(), s)
    s.set_light(0, dark_light())
    a = arms(device, s, K=16, N=16, window=(slice(40, 54), slice(8, 88)), size=(96, 54), depth=3, eye=GLB_CAMERA[0], direction=GLB_CAMERA[1], vfov=T.VFOV)
    agree(a, "emissive-panel.glb")
