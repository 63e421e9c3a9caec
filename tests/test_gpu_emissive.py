"""-m gpu: emissive materials (SPEC.md §22) on the device.  A depth-1 frame of one emissive quad against the binary64 restatement in tests/emissive_ref.py; both
sides, every bounce, weight 1; agreement in the mean with a rectangle light of the same radiance; bit-identity where no emissive triangle is touched and across the
forms of the frame pipeline; the device tables following scene edits; a paired image that stays resident; and a glTF file's emitter end to end."""
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

import emissive_ref as E
import primary_ref as P
from test_gpu_env_sampling import _dark_light
from test_gpu_transmission import BASE, INTERIOR, QUAD_IDX, Rig, _is, _pane_fresnel, add_rect, atrium_small, frame_of, pane_scene  # noqa: F401 (atrium_small: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 64, 36
VFOV = 0.6
U = 2.0 ** -24
BLACK = np.zeros((1, 1, 4), np.uint8)          # RGBE 0: a black probe
USER_SEED = 11
STAGES = ("ray generation", "primary intersection", "intersection", "shadow", "shading", "path", "accumulation", "asvgf")


def texture4():
    """4x4 sRGB emissive image: bytes over the whole range, one black and one white texel"""
    img = np.random.RandomState(22).randint(0, 256, (4, 4, 4)).astype(np.uint8)
    img[0, 0], img[3, 2] = (0, 0, 0, 255), (255, 255, 255, 255)
    return img


def add_quad(s, center, u, v, hu, hv, mat, uv_max=1.0):
    """as add_rect, with texture coordinates running from (0, 0) at the first corner to (uv_max, uv_max) at the opposite one -> (instance, the two triangles' vertex uv)"""
    c, u, v = (np.asarray(a, np.float64) for a in (center, u, v))
    pos = np.array([c - hu * u - hv * v, c + hu * u - hv * v, c + hu * u + hv * v, c - hu * u + hv * v], np.float32)
    nrm = np.tile(np.cross(u, v).astype(np.float32)[None], (4, 1))
    uv = np.array([(0, 0), (uv_max, 0), (uv_max, uv_max), (0, uv_max)], np.float32)
    blas = s.add_mesh(pos, nrm, uv, QUAD_IDX)
    return s.add_instance(blas, np.eye(4, dtype=np.float32), mat), uv[QUAD_IDX].reshape(2, 3, 2), pos[QUAD_IDX].reshape(2, 3, 3)


# ---------------------------------------------------------------- 1. a depth-1 frame equals the reference
QUAD = dict(center=(0.0, 0.0, -2.0), u=(1, 0, 0), v=(0, 1, 0), hu=0.5, hv=0.3)
EYE_FRONT, DIR_FRONT = (0.11, 0.04, 0.0), (-0.03, 0.02, -1.0)
EYE_BACK, DIR_BACK = (-0.07, 0.05, -4.1), (0.02, -0.03, 1.0)
UV_MAX = 2.5
FACTOR, STRENGTH = (0.9, 0.5, 0.25), 3.0

# THE BOUND of a compared pixel, |got - want| <= K_ROUND u |want| + (gx + gy) D_F |Le|, derived and not tuned:
#  * K_ROUND, the roundings of §9 and §22 on a value all of whose terms are non-negative (so relative errors add): (1 - tx): 1; top = c00 (1 - tx) + c10 tx: 3; the same
#    for bot, in parallel; (1 - ty): 1; top (1 - ty) + bot ty: 3; E = Le tex: 1; that is 9, and T E with T = 1, 0 + x and the division by a sample count of 1 are exact.
#    The table entries are binary32 in the reference too.  K_ROUND = 12 leaves three spare.  Without an image, or with a 1 x 1 image (gx = gy = 0), this is the whole bound.
#  * D_F, how far the lookup position fx = tu W - 0.5 of the kernel may lie from the reference's, in texels.  The reference is fed the hit of the binary64 camera ray rounded to
#    binary32; the kernel hits with its own binary32 camera ray, whose direction differs by up to K_D u per component (tests/primary_ref.py, K_D = 40).  Either hit point then lies
#    within t K_D u sqrt(3) / cos + 3e-7 (|o| + t) (SPEC §7's stated rounding) of the true one; in barycentric units that is divided by the shortest edge, the two hits differ by
#    twice that, tu moves by uv_max times the sum of both barycentrics' moves, plus the 6 roundings of its interpolation; fx by W times that plus its own 2 roundings.
#    The lookup's slope per texel is at most the largest difference between neighbouring decoded texels (emissive_ref.steepest), per axis.
K_ROUND = 12.0
T_MAX, COS_MIN, EDGE_MIN, O_MAX = 2.4, 0.8, 0.6, 4.2      # asserted from the reference's own hits below
D_BARY = 2.0 * (T_MAX * P.K_D * U * np.sqrt(3.0) / COS_MIN + 3.0e-7 * (O_MAX + T_MAX)) / EDGE_MIN


def d_f(size):
    return size * (UV_MAX * 2.0 * D_BARY + 6.0 * U * UV_MAX) + 2.0 * U * (size * UV_MAX + 0.5)


def emitter_scene(image=None, uv_max=UV_MAX, pair_with=None):
    """one emissive quad (black base) before a black probe, light 0 dark.  pair_with: a second material whose albedo image is the emissive image, paired with an mra image"""
    s = lp.Scene()
    s.set_light(0, _dark_light())
    img = None if image is None else s.add_image(image)
    m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(m, FACTOR, STRENGTH, img)
    _, tri_uv, tri_pos = add_quad(s, mat=m, uv_max=uv_max, **QUAD)
    if pair_with is not None:
        mra = s.add_image(pair_with)
        pm = s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0, img, mra)
        add_rect(s, (0, -40.0, 0), (1, 0, 0), (0, 0, 1), 0.5, 0.5, pm)      # out of sight: its material makes (img, mra) a pair
    return s, tri_uv, tri_pos


def _moller(o, d, tri):
    """binary64 Moller-Trumbore of rays against one triangle -> (t, u, v), NaN where there is no hit"""
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    pv = np.cross(d, e2)
    det = pv @ e1
    tv = o - tri[0]
    u = (pv @ tv) / det
    qv = np.cross(tv, e1)
    v = (d @ qv) / det
    t = (qv @ e2) / det
    ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return np.where(ok, t, np.nan), u, v


def check_depth1(device, scene, tri_uv, tri_pos, image, eye, direction):
    """renders one depth-1 sample per pixel and compares it with the reference; returns what it measured"""
    sg = lp.SceneGPU.new_from_scene(scene, device)
    pr = lp.ProbeGPU(device, BLACK, 1, 1)
    r = lp.Renderer(device, (W, H))
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, (W, H))
    r.set_max_bounces(1)
    r.set_vfov(VFOV)
    r.set_seed(USER_SEED)
    view = T.look(eye, direction)
    seed = r.frame_state()[1]
    r.reset_accumulation()
    r.raytrace(view)
    got = r.read_radiance()[..., :3].reshape(-1, 3).astype(np.float64)
    o, d = E.camera_rays(view, VFOV, W, H, USER_SEED, seed)
    hit = sg.trace_closest(np.broadcast_to(o.astype(np.float32), d.shape), d.astype(np.float32))
    r.close()
    pr.close()
    sg.close()
    prim = hit["prim"].astype(np.int64)
    prim[hit["prim"] == E.INVALID] = -1
    on = prim >= 0
    assert 300 < on.sum() < W * H - 300                   # the quad fills part of the view
    rec = E.record(FACTOR, STRENGTH, None if image is None else 0)
    images = [] if image is None else [image]
    want = E.depth1_frame(prim, hit["u"], hit["v"], tri_uv, [rec, rec], images)
    # the reference alone: the binary64 hit of the binary64 ray, the texel it falls in, and the constants of the bound
    t64, p64 = np.full(len(d), np.nan), np.full(len(d), -1, np.int64)
    u64, v64 = np.zeros(len(d)), np.zeros(len(d))
    for k in range(2):
        t, u, v = _moller(o, d, tri_pos[k].astype(np.float64))
        m = ~np.isnan(t)
        t64[m], u64[m], v64[m], p64[m] = t[m], u[m], v[m], k
    both = on & (p64 >= 0)
    ng = np.cross(tri_pos[0][1] - tri_pos[0][0], tri_pos[0][2] - tri_pos[0][0]).astype(np.float64)
    cos = np.abs(d @ (ng / np.linalg.norm(ng)))
    assert np.nanmax(t64) <= T_MAX and cos[both].min() >= COS_MIN and np.abs(o).max() <= O_MAX
    assert min(np.linalg.norm(tri_pos[k][(i + 1) % 3] - tri_pos[k][i]) for k in range(2) for i in range(3)) >= EDGE_MIN
    left_out = on & ~both                                  # a silhouette pixel: the two rays disagree on hitting the quad at all
    tol = K_ROUND * U * np.abs(want)
    if image is not None:
        size = image.shape[0]
        tu32, tv32 = E.hit_uv(prim, hit["u"], hit["v"], tri_uv)
        tu64, tv64 = E.hit_uv(p64, u64, v64, tri_uv)
        x32, y32, _, _ = E.texels_of(image, np.nan_to_num(tu32), np.nan_to_num(tv32))
        x64, y64, fx, fy = E.texels_of(image, np.nan_to_num(tu64), np.nan_to_num(tv64))
        left_out |= both & ((x32 != x64) | (y32 != y64))   # the binary32 and the binary64 (u, v) fall in different texels
        # ... which the reference alone keeps rare: few of its own lookups sit within D_F of a texel border
        near = both & ((np.minimum(fx, 1 - fx) < d_f(size)) | (np.minimum(fy, 1 - fy) < d_f(size)))
        assert near.sum() <= 0.01 * both.sum(), (int(near.sum()), int(both.sum()))
        gx, gy = E.steepest(image)
        tol = tol + (gx + gy) * d_f(size) * np.asarray(rec[0], np.float64)[None]
    assert left_out.sum() <= 0.01 * on.sum(), (int(left_out.sum()), int(on.sum()))
    cmp = on & ~left_out
    assert np.all(got[~on & (p64 < 0)] == 0.0)             # the background is exactly 0
    err = np.abs(got - want)
    worst = float((err[cmp] / np.maximum(tol[cmp], 1e-300)).max()) if tol[cmp].min() > 0 else float(err[cmp].max())
    print("depth 1: %d emitter pixels, %d left out, largest |got - want| %.3g, largest error / bound %.3g, largest bound %.3g"
          % (on.sum(), left_out.sum(), err[cmp].max(), worst, tol[cmp].max()))
    assert want[cmp].max() > 0.5 and np.all(err[cmp] <= tol[cmp]), (float(err[cmp].max()), worst)
    return got.reshape(H, W, 3).astype(np.float32), on.reshape(H, W)


@pytest.mark.parametrize("emitter", ["untextured", "4x4", "1x1"])
def test_depth1_frame_equals_the_reference(device, emitter):
    image = {"untextured": None, "4x4": texture4(), "1x1": np.array([[[200, 90, 30, 255]]], np.uint8)}[emitter]
    scene, tri_uv, tri_pos = emitter_scene(image)
    got, on = check_depth1(device, scene, tri_uv, tri_pos, image, EYE_FRONT, DIR_FRONT)
    if image is None:      # E = Le and T = 1: the product is exact
        assert _is(got[on], np.float32(FACTOR) * np.float32(STRENGTH)).all()


# ---------------------------------------------------------------- 2. both sides, every bounce, weight 1
def test_the_back_of_the_quad_emits_the_same(device):
    image = texture4()
    scene, tri_uv, tri_pos = emitter_scene(image)
    check_depth1(device, scene, tri_uv, tri_pos, image, EYE_BACK, DIR_BACK)
    scene, tri_uv, tri_pos = emitter_scene(None)
    got, on = check_depth1(device, scene, tri_uv, tri_pos, None, EYE_BACK, DIR_BACK)
    assert _is(got[on], np.float32(FACTOR) * np.float32(STRENGTH)).all()


LAMP = dict(center=(0.0, 1.0, -3.0), u=(1, 0, 0), v=(0, 0, 1), hu=0.5, hv=0.5)        # normal u x v = -y: it faces the floor
FLOOR = dict(center=(0.0, 0.0, -3.0), u=(0, 0, 1), v=(1, 0, 0), hu=4.0, hv=4.0)       # normal +y
LAMP_EYE, LAMP_DIR = (0.0, 0.2, 0.0), (0.0, 0.0, -1.0)


def lamp_scene(le=(2.0, 1.0, 4.0), floor=True):
    s = lp.Scene()
    s.set_light(0, _dark_light())
    m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(m, le)
    add_rect(s, mat=m, **LAMP)
    if floor:
        add_rect(s, mat=s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0), **FLOOR)
    return s


def test_a_floor_under_the_quad_is_lit_and_the_quad_keeps_its_value(device):
    kw = dict(size=(W, H), eye=LAMP_EYE, direction=LAMP_DIR)
    one = frame_of(device, lamp_scene(), BLACK, n=1, depth=1, **kw)[..., :3]
    two = frame_of(device, lamp_scene(), BLACK, n=1, depth=2, **kw)[..., :3]
    quad = one.any(-1)
    assert 40 < quad.sum() < 600 and _is(one[quad], np.float32((2.0, 1.0, 4.0))).all()
    assert np.all(two[quad] >= one[quad])                   # the same primary rays: the depth-1 value plus a non-negative term
    lit = frame_of(device, lamp_scene(), BLACK, n=512, depth=2, **kw)[..., :3]
    window = (slice(22, 30), slice(16, 48))                 # floor pixels 1.2 to 3 units in front of the camera, under and before the quad
    assert not quad[window].any() and np.all(lit[window] > 0.0), int((lit[window] <= 0).sum())
    assert np.all(frame_of(device, lamp_scene(), BLACK, n=4, depth=1, **kw)[..., :3][~quad & ~np.roll(quad, 1, 0) & ~np.roll(quad, -1, 0) & ~np.roll(quad, 1, 1) & ~np.roll(quad, -1, 1)] == 0.0)


def test_an_emitter_behind_a_thin_pane_is_seen_with_the_fresnel_factor(device):
    """camera -> pane: reflected (probability Fr) into the black probe, or transmitted with weight BASE onto the emitter, which the last bounce still adds with weight 1: every
    sample is 0 or exactly BASE x Le, and the transmitted count over the pane's interior is compared with the reference's Fresnel terms within 5 sigma (derived, as in
    tests/test_gpu_transmission.py)"""
    S, le = 32, (2.0, 1.0, 4.0)
    s = pane_scene()
    m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(m, (0.5, 0.25, 1.0), 4.0)
    add_rect(s, (0, 0, -3), (1, 0, 0), (0, 1, 0), 3.0, 3.0, m)
    rig = Rig(device, s, BLACK, depth=2)
    x = rig.samples(S)
    rig.close()
    inner = x[(slice(None),) + INTERIOR]
    through, none = _is(inner, np.float32(BASE) * np.float32(le)), _is(inner, np.zeros(3, np.float32))
    assert (through ^ none).all(), int((~(through ^ none)).sum())
    Fr = _pane_fresnel()[INTERIOR]
    want, sigma = S * (1 - Fr).sum(), np.sqrt(S * (Fr * (1 - Fr)).sum())
    print("pane: transmitted samples %d, expected %.1f +- %.1f" % (through.sum(), want, sigma))
    assert abs(int(through.sum()) - want) <= 5 * sigma, (int(through.sum()), want, sigma)
    assert _is(x[:, 0, 0], np.float32(le)).all()            # beside the pane: the emitter itself


# ---------------------------------------------------------------- 3. agreement with a rectangle light
def test_agrees_with_a_rectangle_light_of_the_same_radiance(device):
    """Arm R: a floor under a downward rectangle Light of radiance 8 (next-event estimation + MIS, the code that ships).  Arm E: the same rectangle as a black emissive quad,
    light 0 dark (BSDF paths only, weight 1).  Depth 2, 64x36, the camera sees only the floor; K = 16 batches of N = 64 spp per arm (one raytrace_n each, user seeds 100 + k and
    200 + k); the floor-window means must agree within 5 sqrt(se_E^2 + se_R^2), the standard errors taken from the batch means.  N = 64 is chosen so that arm R meets its
    condition (relative standard error below 2 %) on its own.  Measured on an MI355X with N = 64: rectangle light 0.14979 +- 0.00005 (relative 0.04 %), emissive quad
    0.14934 +- 0.00093 (relative 0.62 %), |difference| = 0.10 of the bound."""
    K, N, LE = 16, 64, 8.0
    rect = dict(center=(0.0, 1.5, -3.0), hu=0.5, hv=0.5)
    means = {}
    for arm in ("R", "E"):
        s = lp.Scene()
        if arm == "R":
            l = np.zeros(1, lp._abi.LIGHT_DT)
            l["normal"], l["tangent"], l["bitangent"], l["origin"] = (0, -1, 0, 0), (1, 0, 0, rect["hu"]), (0, 0, 1, rect["hv"]), rect["center"] + (LE,)
            s.set_light(0, l)
        else:
            s.set_light(0, _dark_light())
            m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
            s.set_material_emission(m, (1.0, 1.0, 1.0), LE)
            add_rect(s, rect["center"], (1, 0, 0), (0, 0, 1), rect["hu"], rect["hv"], m)
        add_rect(s, mat=s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0), **FLOOR)
        rig = Rig(device, s, BLACK, size=(W, H), depth=2, eye=(0.0, 1.0, 0.5), direction=(0.0, -0.7, -1.0))
        batch = []
        for k in range(K):
            rig.r.set_seed((100 if arm == "R" else 200) + k)
            rig.r.reset_accumulation()
            rig.r.accumulate = True
            rig.r.raytrace_n(rig.view, N)
            img = rig.r.read_radiance()[..., :3]
            assert np.all(np.isfinite(img))
            batch.append(float(img[8:28, 12:52].mean()))
        rig.close()
        means[arm] = np.array(batch)
    mR, mE = means["R"].mean(), means["E"].mean()
    seR, seE = means["R"].std(ddof=1) / np.sqrt(K), means["E"].std(ddof=1) / np.sqrt(K)
    print("rectangle light %.5f +- %.5f (relative %.2f %%), emissive quad %.5f +- %.5f (relative %.2f %%), difference / bound %.2f"
          % (mR, seR, 100 * seR / mR, mE, seE, 100 * seE / mE, abs(mE - mR) / (5 * np.hypot(seE, seR))))
    assert mR > 0 and seR / mR < 0.02
    assert abs(mE - mR) <= 5 * np.hypot(seE, seR), (mE, mR, seE, seR)


# ---------------------------------------------------------------- 4. nothing else moved
ATRIUM = dict(size=(96, 64), depth=2, vfov=T.VFOV)


def _atrium(desc, le=None, used=True):
    """the small atrium; `le`: an emission for the material of its first instance with triangles (used) or for a material no instance uses"""
    s = scenes.to_product(desc)
    if le is not None:
        m = int(s.instances[len(s.instances) // 2]["material_index"]) if used else s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0)
        s.set_material_emission(m, le)
    return s


def _timed(device, scene, probe, size, depth, eye, direction, vfov, n=1, options=None, sg=None):
    """one raytrace_n as one wavefront with the timings on -> (radiance, {stage: launches})"""
    rig = Rig(device, scene, probe, size=size, depth=depth, eye=eye, direction=direction, vfov=vfov, options=options, sg=sg)
    rig.r.enable_timings(True)
    rig.r.reset_accumulation()
    rig.r.accumulate = True
    rig.r.raytrace_n(rig.view, n)
    img = rig.r.read_radiance()
    launches = {k: v[1] for k, v in rig.r.timings().items()}
    rig.close()
    return img, {k: launches[k] for k in STAGES}


def test_an_unused_emissive_material_changes_nothing(device, atrium_small):
    desc = atrium_small
    cam = dict(eye=desc["camera"]["origin"], direction=desc["camera"]["direction"])
    for options in (None, {"coop_rays": 0}):                # the shipped launches of this size, and the path kernel's
        a, na = _timed(device, _atrium(desc), desc.get("probe"), options=options, **ATRIUM, **cam)
        b, nb = _timed(device, _atrium(desc, (1.0, 1.0, 1.0), used=False), desc.get("probe"), options=options, **ATRIUM, **cam)
        assert np.all(np.isfinite(a)) and a[..., :3].any() and a.tobytes() == b.tobytes()
        assert na == nb and (na["path"] == 1) == (options is not None), (na, nb)


def test_pixels_that_touch_no_emissive_triangle_are_unchanged(device, atrium_small):
    desc = atrium_small
    kw = dict(n=2, eye=desc["camera"]["origin"], direction=desc["camera"]["direction"], **ATRIUM)
    plain = frame_of(device, _atrium(desc), desc.get("probe"), **kw)
    blue = frame_of(device, _atrium(desc, (0.0, 0.0, 1.0)), desc.get("probe"), **kw)
    full = frame_of(device, _atrium(desc, (1.0, 0.5, 1.0)), desc.get("probe"), **kw)
    assert blue[..., :2].tobytes() == plain[..., :2].tobytes()          # + T x 0 changes nothing, bit for bit
    mask = blue[..., 2] != plain[..., 2]                                # the pixels a path of which touched an emissive triangle
    print("pixels touched by the emitter: %d of %d" % (mask.sum(), mask.size))
    assert mask.any() and (~mask).any()
    assert full[~mask].tobytes() == plain[~mask].tobytes()
    assert np.all(full[mask][:, 0] > plain[mask][:, 0])


# ---------------------------------------------------------------- 5. launch independence
@pytest.mark.parametrize("size,n", [((64, 36), 4), ((320, 180), 2), ((512, 288), 1)], ids=["coop_all", "path_sized", "per_bounce"])
def test_launch_independence(device, atrium_small, size, n):
    """64x36 x 4 is a wavefront of the wave-per-ray range, 320x180 x 2 = 115 200 rays one of the path kernel's range (which an emissive scene leaves to the per-bounce
    launches), 512x288 lies above both"""
    desc = atrium_small
    scene, probe = _atrium(desc, (1.0, 0.5, 2.0)), desc.get("probe")
    cam = dict(eye=desc["camera"]["origin"], direction=desc["camera"]["direction"], vfov=T.VFOV)
    sg = lp.SceneGPU.new_from_scene(scene, device)
    kw = dict(size=size, depth=3, sg=sg, **cam)
    want, launches = _timed(device, scene, probe, n=n, options={"coop_rays": 0} if size[0] == 320 else None, **kw)
    assert np.all(np.isfinite(want)) and want[..., :3].any()
    if size[0] == 320:
        assert launches["path"] == 0 and launches["shading"] == 3, launches
    variants = [dict(options={"coop_rays": 0}), dict(options={"path_rays": 0}), dict(options={"packet_primary": 0}), dict(options={"packet_primary": 1}),
                dict(options={"path_rays": 0x7FFFFFFF, "coop_rays": 0}), dict(options={"tail_lanes": 0}), dict(options={"wavefront_rays": size[0] * size[1] * n // 2})]
    for v in variants:
        assert frame_of(device, scene, probe, n=n, **kw, **v).tobytes() == want.tobytes(), v      # n recorded raytrace calls against one raytrace_n
    acc = np.zeros_like(want)
    for rank in range(2):
        acc += frame_of(device, scene, probe, n=n, rank=rank, world=2, **kw)
    assert acc.tobytes() == want.tobytes()
    if size[0] != 512:
        for mode in (lp.BlitMode.DenoisedPathrace, lp.BlitMode.Temporal):
            one = Rig(device, scene, probe, mode=mode, **kw)
            ranks = [Rig(device, scene, probe, mode=mode, rank=q, world=2, **kw) for q in range(2)]
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


# ---------------------------------------------------------------- 6. the tables follow the scene
def _moved(dx):
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = dx
    return m.T


def test_tables_follow_the_scene(device):
    kw = dict(size=(W, H), depth=2, eye=LAMP_EYE, direction=LAMP_DIR, n=2)

    def lamp(dx=0.0, le=(2.0, 1.0, 4.0)):
        s = lamp_scene(le if le is not None else (1.0, 1.0, 1.0))
        if le is None:
            s.set_material_emission(1, (0.0, 0.0, 0.0))
        s.set_instance_transform(1, _moved(dx))
        return s

    fresh, fresh_moved, never = frame_of(device, lamp(), BLACK, **kw), frame_of(device, lamp(0.7), BLACK, **kw), frame_of(device, lamp(le=None), BLACK, **kw)
    assert fresh.tobytes() != fresh_moved.tobytes() and fresh[..., :3].any() and not never[..., :3].any()
    s = lamp()
    sg = lp.SceneGPU.new_from_scene(s, device)
    s.set_instance_transform(1, _moved(0.7))                # an instance update that moves the emitter
    assert sg.update_instances(s) == 1
    assert frame_of(device, s, BLACK, sg=sg, **kw).tobytes() == fresh_moved.tobytes()
    s.set_instance_transform(1, _moved(0.0))
    sg.rebuild(s)                                           # a rebuild
    assert frame_of(device, s, BLACK, sg=sg, **kw).tobytes() == fresh.tobytes()
    _, n_on = _timed(device, s, BLACK, kw["size"], 2, LAMP_EYE, LAMP_DIR, VFOV, options={"coop_rays": 0}, sg=sg)
    s.set_material_emission(1, (0.0, 0.0, 0.0))             # back to non-emissive: the tables are null again, and the path kernel is back
    assert s.material_emission(1)[1] is None and not s.material_emission(1)[0].any()
    sg.rebuild(s)
    assert frame_of(device, s, BLACK, sg=sg, **kw).tobytes() == never.tobytes()
    _, n_off = _timed(device, s, BLACK, kw["size"], 2, LAMP_EYE, LAMP_DIR, VFOV, options={"coop_rays": 0}, sg=sg)
    assert n_on["path"] == 0 and n_off["path"] == 1, (n_on, n_off)
    sg.close()


# ---------------------------------------------------------------- 7. a paired image stays resident
def test_an_emissive_image_that_is_also_half_of_a_pair_stays_resident(device):
    image = texture4()
    mra = np.random.RandomState(23).randint(0, 256, (4, 4, 4)).astype(np.uint8)
    scene, tri_uv, tri_pos = emitter_scene(image, pair_with=mra)
    check_depth1(device, scene, tri_uv, tri_pos, image, EYE_FRONT, DIR_FRONT)
    # an image uploaded ONLY as half of a pair cannot become emissive without a new upload
    s = lp.Scene()
    s.set_light(0, _dark_light())
    a, b = s.add_image(image), s.add_image(mra)
    m = s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0, a, b)
    add_rect(s, mat=m, **LAMP)
    sg = lp.SceneGPU.new_from_scene(s, device)
    s.set_material_emission(m, (1.0, 1.0, 1.0), 1.0, a)
    with pytest.raises(lp.Error) as e:
        sg.rebuild(s)
    assert "only as half of an (albedo, mra) pair" in str(e.value)
    sg.close()


# ---------------------------------------------------------------- 8. glTF end to end
GLB_FLOOR = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], "<f4")
GLB_PANEL = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], "<f4")
GLB_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], "<f4")
GLB_CAMERA = ((0.0, 1.0, 6.0), (0.0, -0.05, -1.0))
_DEFAULT = object()


def png_bytes(img):
    """an 8-bit RGBA PNG, filter 0, stored (uncompressed) deflate blocks: the same bytes whatever the zlib"""
    h, w, _ = img.shape

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    raw = b"".join(b"\0" + np.ascontiguousarray(img[y]).tobytes() for y in range(h))
    stored = b"\x78\x01" + b"\x01" + struct.pack("<HH", len(raw), len(raw) ^ 0xFFFF) + raw + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", stored) + chunk(b"IEND", b"")


def emissive_glb(panel=_DEFAULT):
    """a small .glb: an 8x8 floor and, 2 units above it, a 2x2 quad whose material has emissiveFactor (1, 0.8, 0.6), a 4x4 RGBA PNG emissive texture and
    emissiveStrength 5; no light.  `panel`: other emission-related members for the quad's material (a dict merged into it; None: none at all)"""
    blob = bytearray()
    views, accessors = [], []

    def view(raw):
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(raw)})
        blob.extend(raw)
        blob.extend(b"\0" * (-len(blob) % 4))
        return len(views) - 1

    def add(arr, ctype, atype):
        accessors.append({"bufferView": view(np.ascontiguousarray(arr).tobytes()), "componentType": ctype, "count": len(arr), "type": atype})
        return len(accessors) - 1

    up, down = np.tile(np.array([[0, 1, 0]], "<f4"), (4, 1)), np.tile(np.array([[0, -1, 0]], "<f4"), (4, 1))
    qi = add(np.array([0, 2, 1, 0, 3, 2], "<u2"), 5123, "SCALAR")
    pi = add(np.array([0, 1, 2, 0, 2, 3], "<u2"), 5123, "SCALAR")
    meshes = [{"primitives": [{"attributes": {"POSITION": add(GLB_FLOOR, 5126, "VEC3"), "NORMAL": add(up, 5126, "VEC3")}, "indices": qi, "material": 0}]},
              {"primitives": [{"attributes": {"POSITION": add(GLB_PANEL, 5126, "VEC3"), "NORMAL": add(down, 5126, "VEC3"), "TEXCOORD_0": add(GLB_UV, 5126, "VEC2")},
                               "indices": pi, "material": 1}]}]
    if panel is _DEFAULT:
        panel = {"emissiveFactor": [1.0, 0.8, 0.6], "emissiveTexture": {"index": 0}, "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 5.0}}}
    mats = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1.0], "roughnessFactor": 0.9, "metallicFactor": 0.0}},
            {"pbrMetallicRoughness": {"baseColorFactor": [0.1, 0.1, 0.1, 1.0], "roughnessFactor": 0.8, "metallicFactor": 0.0}}]
    if panel is not None:
        mats[1].update(panel)
    js = {"asset": {"version": "2.0"}, "meshes": meshes, "accessors": accessors, "bufferViews": views, "materials": mats,
          "images": [{"bufferView": view(png_bytes(texture4())), "mimeType": "image/png"}], "textures": [{"source": 0}],
          "nodes": [{"mesh": 0, "scale": [4.0, 1.0, 4.0]}, {"mesh": 1, "translation": [0.0, 2.0, 0.0]}],
          "extensionsUsed": ["KHR_materials_emissive_strength"], "buffers": [{"byteLength": len(blob)}]}
    j = json.dumps(js).encode()
    j += b" " * (-len(j) % 4)
    b = bytes(blob)
    return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + 8 + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + struct.pack("<II", len(b), 0x004E4942) + b


def test_gltf_emitter_end_to_end(device):
    with open(os.path.join(HERE, "golden", "emissive-panel.glb"), "rb") as f:
        assert f.read() == emissive_glb()                    # the committed copy is this writer's output
    a = lp.Scene()
    lp.loaders.load_gltf(emissive_glb(), a)
    le, image = a.material_emission(2)
    assert np.array_equal(le, np.float32((1.0, 0.8, 0.6)) * np.float32(5.0)) and image == 0 and a.material_emission(1)[1] is None
    c = lp.Scene()
    img = c.add_image(texture4())
    mats = [c.add_material((0.8, 0.8, 0.8, 1.0), 0.9, 0.0), c.add_material((0.1, 0.1, 0.1, 1.0), 0.8, 0.0)]
    c.set_material_emission(mats[1], (1.0, 0.8, 0.6), 5.0, img)
    up, down = np.tile(np.float32([[0, 1, 0]]), (4, 1)), np.tile(np.float32([[0, -1, 0]]), (4, 1))
    blas = [c.add_mesh(GLB_FLOOR.astype(np.float32), up, None, np.array([0, 2, 1, 0, 3, 2], np.uint32)), c.add_mesh(GLB_PANEL.astype(np.float32), down, GLB_UV.astype(np.float32), QUAD_IDX)]

    def trs(t=(0, 0, 0), s=(1, 1, 1)):
        m = np.diag(list(s) + [1.0]).astype(np.float32)
        m[:3, 3] = t
        return m.T

    c.add_instance(blas[0], trs(s=(4, 1, 4)), mats[0])
    c.add_instance(blas[1], trs(t=(0, 2, 0)), mats[1])
    frames = []
    for s in (a, c):
        s.set_light(0, _dark_light())
        frames.append(frame_of(device, s, BLACK, n=16, size=(96, 54), depth=3, eye=GLB_CAMERA[0], direction=GLB_CAMERA[1], vfov=T.VFOV))
    assert np.all(np.isfinite(frames[0])) and frames[0].tobytes() == frames[1].tobytes()
    assert frames[0][40:, :, :3].mean() > 0.0 and frames[0][..., :3].max() > 1.0      # a lit floor under a glowing panel
    b = lp.Scene()
    lp.loaders.load_gltf(emissive_glb(panel=None), b)        # the same file without the three members renders black
    b.set_light(0, _dark_light())
    assert not frame_of(device, b, BLACK, n=2, size=(96, 54), depth=3, eye=GLB_CAMERA[0], direction=GLB_CAMERA[1], vfov=T.VFOV)[..., :3].any()


def test_bench_renders_the_emissive_file():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--frames-per-step", "2", "--width", "256", "--height", "256", "--no-extras",
                        "--camera", "0,1,6,0,-0.05,-1", "--gltf", os.path.join(HERE, "golden", "emissive-panel.glb")], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert j["data"] == "real" and "emissive-panel.glb" in j["config"]["workload"] and j["config"]["frame_complete"] is True and j["value"] > 0
