"""-m gpu: tangent-space normal maps (SPEC.md §24) on the device.  The kernels' own function (lpt_scene_gpu_shading_normal) against tests/normal_ref.py over a scene
of small shapes; a depth-1 frame of a normal-mapped floor under one directional light against punctual_ref.radiance with the reference's normal; the denoiser's normal
word; bit-identity where no map is in use, across the forms of the frame pipeline, across scene edits and with a paired image; every side table at once; a glTF file."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

import emissive_ref as E
import normal_ref as N
import primary_ref as P
import punctual_ref as R
from test_gpu_emissive import _moller, _timed, png_bytes
from test_gpu_env_sampling import _dark_light
from test_gpu_transmission import QUAD_IDX, Rig, add_rect, atrium_small, frame_of  # noqa: F401 (atrium_small: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 64, 36
VFOV = 0.6
U = 2.0 ** -24
F = np.float32
BLACK = np.zeros((1, 1, 4), np.uint8)
USER_SEED = 11


def image4(seed=31):
    """4x4 normal image: random bytes in every channel, so nz runs over [-1, 1] and a scaled texel often ends under the surface"""
    return np.random.RandomState(seed).randint(0, 256, (4, 4, 4)).astype(np.uint8)


def image53():
    """5 wide, 3 high: neither a multiple of the 8x4 tile nor a power of two"""
    return np.random.RandomState(32).randint(0, 256, (3, 5, 4)).astype(np.uint8)


IMAGE1 = np.array([[[200, 90, 230, 255]]], np.uint8)


def bake_normals(nrm):
    """SPEC §2.5 under the identity transform, binary32: n (1 / sqrt((nx nx + ny ny) + nz nz))"""
    n = np.asarray(nrm, F)
    l2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    return n * (F(1) / np.sqrt(l2))[..., None]


# ---------------------------------------------------------------- 1. the hook against the reference
N_HOOK = 4100      # 64 x 64 + 4: whole blocks and a partial wave


def _tilted(ng, deg, about):
    """ng turned by `deg` degrees about the unit in-plane axis `about`"""
    a = np.radians(deg)
    ng, about = np.asarray(ng, np.float64), np.asarray(about, np.float64)
    return ng * np.cos(a) + np.cross(about, ng) * np.sin(a)


def hook_shapes():
    """name -> positions, vertex normals, uv, indices, the image and the scale of its material (image None: no map)"""
    quad = lambda c, hu, hv: np.array([[c[0] - hu, c[1] - hv, c[2]], [c[0] + hu, c[1] - hv, c[2]], [c[0] + hu, c[1] + hv, c[2]], [c[0] - hu, c[1] + hv, c[2]]], F)   # normal +z
    up = np.tile(F([[0, 0, 1]]), (4, 1))
    quv = lambda m: np.array([(0, 0), (m, 0), (m, m), (0, m)], F)
    tri = lambda x: np.array([[x, 0, -1], [x + 1.3, 0.1, -1], [x + 0.2, 0.9, -1]], F)
    tri_idx = np.array([0, 1, 2], np.uint32)
    tilt = np.array([_tilted((0, 0, 1), 40.0, ax) for ax in ((1, 0, 0), (-0.5, 0.8660254, 0), (-0.5, -0.8660254, 0))], F)
    return [
        dict(name="quad 4x4, scale 1", pos=quad((0, 0, -2), 0.5, 0.3), nrm=up, uv=quv(2.5), idx=QUAD_IDX, image=image4(), scale=1.0),
        dict(name="quad 5x3, scale 2.5", pos=quad((2, 0, -2), 0.5, 0.3), nrm=up, uv=quv(1.7), idx=QUAD_IDX, image=image53(), scale=2.5),
        dict(name="quad 1x1, scale -1", pos=quad((4, 0, -2), 0.5, 0.3), nrm=up, uv=quv(1.0), idx=QUAD_IDX, image=IMAGE1, scale=-1.0),
        dict(name="quad 4x4, scale 0", pos=quad((6, 0, -2), 0.5, 0.3), nrm=up, uv=quv(3.0), idx=QUAD_IDX, image=image4(33), scale=0.0),
        dict(name="mirrored uv", pos=tri(0.0), nrm=up[:3], uv=np.array([(1.5, 0.1), (0.2, 0.2), (1.4, 1.1)], F), idx=tri_idx, image=image4(), scale=1.0),
        dict(name="all uv equal", pos=tri(2.0), nrm=up[:3], uv=np.array([(0.3, 0.6)] * 3, F), idx=tri_idx, image=image4(), scale=1.0),
        dict(name="normals tilted 40 degrees", pos=tri(4.0), nrm=tilt, uv=np.array([(0.1, 0.2), (1.9, 0.4), (0.6, 1.7)], F), idx=tri_idx, image=image53(), scale=2.5),
        dict(name="no map", pos=tri(6.0), nrm=tilt, uv=np.array([(0.1, 0.2), (1.9, 0.4), (0.6, 1.7)], F), idx=tri_idx, image=None, scale=1.0),
    ]


def hook_scene():
    """-> (scene, shapes with `first` = the prim id of their first triangle): one instance per shape, identity transforms, so prim ids run in this order"""
    s = lp.Scene()
    s.set_light(0, _dark_light())
    shapes, first, images = hook_shapes(), 0, {}
    for sh in shapes:
        m = s.add_material((0.8, 0.8, 0.8, 1.0), 1.0, 0.0)
        if sh["image"] is not None:
            key = sh["image"].tobytes()
            if key not in images:
                images[key] = s.add_image(sh["image"])
            s.set_material_normal_map(m, images[key], sh["scale"])
        s.add_instance(s.add_mesh(sh["pos"], sh["nrm"], sh["uv"], sh["idx"]), np.eye(4, dtype=np.float32), m)
        sh["first"] = first
        first += len(sh["idx"]) // 3
    return s, shapes


def hook_cases(k, sh):
    """the committed inputs of shape number k: per element a triangle of the shape, barycentrics inside it and a unit direction — four fifths anywhere on the
    sphere (both sides), one fifth grazing: 0.003 off the triangle's plane, 3 000 times the bound of dot(Ng, d).  All binary32."""
    rng = np.random.default_rng(2400 + k)
    n_tri = len(sh["idx"]) // 3
    t = rng.integers(0, n_tri, N_HOOK)
    b = rng.uniform(0, 1, (N_HOOK, 2))
    over = b.sum(1) > 1
    b[over] = 1 - b[over]
    d = rng.normal(size=(N_HOOK, 3))
    tri = sh["pos"][sh["idx"].reshape(-1, 3)].astype(np.float64)
    e1, e2 = tri[t, 1] - tri[t, 0], tri[t, 2] - tri[t, 0]
    ng = np.cross(e1, e2)
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    graze = np.arange(N_HOOK) % 5 == 4
    a = rng.uniform(0, 2 * np.pi, N_HOOK)
    e1n = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    inplane = e1n * np.cos(a)[:, None] + np.cross(ng, e1n) * np.sin(a)[:, None]
    d[graze] = (inplane + ng * (0.003 * np.where(rng.uniform(size=N_HOOK) < 0.5, -1.0, 1.0))[:, None])[graze]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return t, b.astype(F), d.astype(F)


def hook_reference(sh, t, b, d, dtype=np.float64):
    idx = sh["idx"].reshape(-1, 3)
    return N.shading_normal(sh["pos"][idx][t], bake_normals(sh["nrm"])[idx][t], sh["uv"][idx][t], b, d, sh["image"], sh["scale"], dtype=dtype)


def test_the_kernels_function_equals_the_reference(device):
    """Measured on an MI355X: see DESIGN.md §5.2g for the largest error as a fraction of its bound per shape."""
    scene, shapes = hook_scene()
    sg = lp.SceneGPU.new_from_scene(scene, device)
    worst_all = 0.0
    for k, sh in enumerate(shapes):
        t, b, d = hook_cases(k, sh)
        ref = hook_reference(sh, t, b, d)
        ns, mapped = sg.shading_normal((sh["first"] + t).astype(np.uint32), b, d)
        skip = N.undecided(ref)
        assert skip.sum() <= 0.02 * N_HOOK, (sh["name"], int(skip.sum()))
        c = ~skip
        assert np.array_equal(mapped[c], ref["mapped"][c]), (sh["name"], int((mapped[c] != ref["mapped"][c]).sum()))
        err, bound = np.abs(ns.astype(np.float64) - ref["Ns"])[c], ref["Ns_err"][c]
        assert np.all(np.isfinite(bound)) and np.all(err <= bound), (sh["name"], float(err.max()), float((err - bound).max()))
        frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        worst_all = max(worst_all, frac)
        print("%-26s mapped %4d of %d, skipped %d, largest |Ns - ref| %.3g, largest bound %.3g, largest error / bound %.3g"
              % (sh["name"], mapped.sum(), N_HOOK, skip.sum(), err.max(), bound.max(), frac))
        if sh["image"] is None or sh["name"] == "all uv equal":
            assert not mapped.any()
        else:
            assert 0 < ref["mapped"].sum()
        assert np.abs(np.linalg.norm(ns.astype(np.float64), axis=1) - 1).max() < 1e-5
    print("largest error / bound over all shapes: %.3g" % worst_all)
    with pytest.raises(lp.Error):
        sg.shading_normal(np.array([10 ** 6], np.uint32), np.zeros((1, 2), F), np.array([[0, 0, -1]], F))      # a prim beyond the baked triangles is refused, not read
    sg.close()


# ---------------------------------------------------------------- 2. a depth-1 frame, closed form
FLOOR_POS = np.array([[-3, 0, 0], [3, 0, 0], [3, 0, -7], [-3, 0, -7]], F)     # wound so that the geometric normal is +y
FLOOR_UV = np.ascontiguousarray(FLOOR_POS[:, [0, 2]])                          # uv = (x, z)
FLOOR_BASE, FLOOR_ROUGH, FLOOR_METAL = (0.8, 0.7, 0.6), 1.0, 0.0
LIGHT = dict(direction=(-0.2, -0.7, 1.0), color=(1.0, 0.9, 0.8), intensity=3.0)
EYE, DIR = (0.1, 1.0, 0.2), (0.02, -1.0, -1.0)        # 45 degrees down: every pixel is on the floor
FLOOR_SCALE = 1.5

# THE BOUND of a compared pixel (one sample that picked the directional light), derived and not tuned:
#   |got - want| <= K_BSDF u |want| + 2 sum_i |dL/dN_i| e_i + 2 sum_i |dL/dV_i| K_D u
#  * K_BSDF counts the roundings of §10, §19 and §12.3 behind N and V on one channel: the half vector (dot 5, 1/sqrt 2, scale 1), NoH, VoH, NoV, NoL (5 each), D (8), Vis (9),
#    (1 - VoH)^5 (4), F (3), the two lobes and their sum (6), f NoL E / p (4), T f and the accumulation (2): 67.  With roughness 1 (a2 = 1) and metallic 0 every term is
#    positive except 1 - VoH, whose relative error 1 / (1 - VoH) <= 8 here (asserted) weighs on the Fresnel term, below 1/20 of f.  K_BSDF = 96 leaves a third spare.
#  * e_i is normal_ref's running bound of Ns for this pixel, built with e_uv: how far the kernel's interpolated (tu, tv) may lie from the reference's.  The reference is
#    fed the hit of the binary64 camera ray rounded to binary32; the kernel hits with its own binary32 ray, whose direction differs by up to K_D u per component
#    (tests/primary_ref.py).  As tests/test_gpu_emissive.py derives it: either hit lies within t K_D u sqrt(3) / cos + 3e-7 (|o| + t) of the true point, the two differ
#    by twice that, and uv = (x, z) moves by as much (a slope of 1 per axis).  The lookup's slope in texels and the frame's conditioning are inside the running bound.
#  * dL/dN and dL/dV are central differences of punctual_ref.radiance (step 1e-6, binary64) — the reference's own slope; the factor 2 covers the second order.
K_BSDF = 96.0
T_MAX, COS_MIN, O_MAX = 2.5, 0.4, 1.1                     # asserted from the reference's own hits below
E_UV = 2.0 * (T_MAX * P.K_D * U * np.sqrt(3.0) / COS_MIN + 3.0e-7 * (O_MAX + T_MAX))


def floor_scene(image, scale=FLOOR_SCALE, light=True, extra=None):
    s = lp.Scene()
    s.set_light(0, _dark_light())
    m = s.add_material(FLOOR_BASE + (1.0,), FLOOR_ROUGH, FLOOR_METAL)
    if image is not None:
        s.set_material_normal_map(m, s.add_image(image), scale)
    s.add_instance(s.add_mesh(FLOOR_POS, np.tile(F([[0, 1, 0]]), (4, 1)), FLOOR_UV, QUAD_IDX), np.eye(4, dtype=np.float32), m)
    if light:
        s.add_punctual_light(lp.directional_light(**LIGHT))
    if extra is not None:
        extra(s)
    return s


def _lum_radiance(light, P0, Ns, V):
    return R.radiance(light, P0[None], Ns, V, FLOOR_BASE, FLOOR_ROUGH, FLOOR_METAL)[0]


def floor_reference(sg, view, seed, image, scale=FLOOR_SCALE):
    """per pixel of the frame with seed counter `seed`: the reference's Ns at the pixel's own camera ray (and its bound), the hit, V — and which pixels compare"""
    o, d = E.camera_rays(view, VFOV, W, H, USER_SEED, seed)
    hit = sg.trace_closest(np.broadcast_to(o.astype(F), d.shape), d.astype(F))
    on = hit["prim"] != E.INVALID
    tri = FLOOR_POS[QUAD_IDX.reshape(2, 3)]
    p64 = np.full(len(d), -1, np.int64)
    t64 = np.full(len(d), np.nan)
    for k in range(2):
        t, _, _ = _moller(o, d, tri[k].astype(np.float64))
        m = ~np.isnan(t)
        p64[m], t64[m] = k, t[m]
    both = on & (p64 == hit["prim"].astype(np.int64))         # a pixel on the floor's diagonal or silhouette: the two rays disagree on the triangle
    assert both.sum() > 0.9 * on.sum() > 0.5 * W * H
    assert np.nanmax(t64) <= T_MAX and np.abs(d[both, 1]).min() >= COS_MIN and np.abs(o).max() <= O_MAX
    k = np.where(on, hit["prim"], 0).astype(np.int64)
    idx = QUAD_IDX.reshape(2, 3)
    bary = np.stack([hit["u"], hit["v"]], -1).astype(F)
    ref = N.shading_normal(FLOOR_POS[idx][k], np.tile(F([0, 1, 0]), (len(d), 3, 1)), FLOOR_UV[idx][k], bary, d.astype(F), image, scale, e_uv=E_UV)
    cmp = both & ~N.undecided(ref)
    assert cmp.sum() >= 0.98 * both.sum(), (int(cmp.sum()), int(both.sum()))
    bw = 1.0 - hit["u"].astype(np.float64) - hit["v"].astype(np.float64)
    tp = FLOOR_POS[idx][k].astype(np.float64)
    P0 = tp[:, 0] * bw[:, None] + tp[:, 1] * hit["u"].astype(np.float64)[:, None] + tp[:, 2] * hit["v"].astype(np.float64)[:, None]
    return dict(o=o, d=d, on=on, cmp=cmp, ref=ref, P=P0, V=-d, prim=hit["prim"])


def render_floor(device, image, scale=FLOOR_SCALE, reference=True):
    """one depth-1 sample per pixel with user seed USER_SEED -> (radiance (W H, 3) binary64, floor_reference's dict or None, the frame's seed counter)"""
    rig = Rig(device, floor_scene(image, scale), BLACK, size=(W, H), depth=1, eye=EYE, direction=DIR, vfov=VFOV)
    rig.r.set_seed(USER_SEED)
    rig.r.reset_accumulation()
    seed = rig.r.frame_state()[1]
    rig.r.raytrace(rig.view)
    got = rig.r.read_radiance()[..., :3].reshape(-1, 3).astype(np.float64)
    fr = floor_reference(rig.sg, rig.view, seed, image, scale) if reference else None
    rig.close()
    return got, fr, seed


def check_floor(device, image, scale=FLOOR_SCALE):
    got, fr, seed = render_floor(device, image, scale)
    light = R.from_record(lp.directional_light(**LIGHT))
    # §19's pick (SPEC §4): the shading stream of bounce 0 runs on seed counter seed + 1; one punctual and one rectangle light, so r0 < 1/2 picks the directional light (p = 1/2)
    pix = np.arange(W * H, dtype=np.uint64)
    picked = R.r0_of(pix, seed + 1, USER_SEED) < 0.5
    assert 0.4 < picked.mean() < 0.6
    assert np.all(got[fr["on"] & ~picked] == 0.0) and np.all(got[~fr["on"]] == 0.0)      # light 0 is dark, the probe black
    cmp = np.flatnonzero(fr["cmp"] & picked)
    Ns, Ne, h = fr["ref"]["Ns"], fr["ref"]["Ns_err"], 1.0e-6
    worst, tols = 0.0, np.full((W * H, 3), np.nan)
    for i in cmp:
        want = _lum_radiance(light, fr["P"][i], Ns[i], fr["V"][i]) / 0.5
        sens = np.zeros(3)
        for c in range(3):
            e = np.zeros(3)
            e[c] = h
            dn = np.abs(_lum_radiance(light, fr["P"][i], Ns[i] + e, fr["V"][i]) - _lum_radiance(light, fr["P"][i], Ns[i] - e, fr["V"][i])) / (2 * h) / 0.5
            dv = np.abs(_lum_radiance(light, fr["P"][i], Ns[i], fr["V"][i] + e) - _lum_radiance(light, fr["P"][i], Ns[i], fr["V"][i] - e)) / (2 * h) / 0.5
            sens += 2.0 * (dn * Ne[i, c] + dv * P.K_D * U)
        tol = K_BSDF * U * np.abs(want) + sens
        err = np.abs(got[i] - want)
        assert np.all(err <= tol), (int(i), got[i], want, tol)
        worst, tols[i] = max(worst, float(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0).max())), tol
    voh = np.sqrt(0.5 * (1.0 + fr["V"][cmp] @ -light["direction"]))
    assert (1.0 / (1.0 - voh)).max() <= 8.0
    print("depth 1: %d pixels compared, largest error / bound %.3g, median bound %.3g, largest bound %.3g, mapped %d"
          % (len(cmp), worst, np.nanmedian(tols), np.nanmax(tols), fr["ref"]["mapped"][cmp].sum()))
    return got, fr, tols


@pytest.mark.parametrize("image", ["4x4", "1x1"])
def test_depth1_frame_equals_the_closed_form(device, image):
    img = {"4x4": image4(), "1x1": IMAGE1}[image]
    got, fr, tols = check_floor(device, img)
    took = fr["ref"]["mapped"] & ~np.isnan(tols[:, 0])               # compared pixels that shade with the perturbed normal
    assert took.sum() > 0.25 * (~np.isnan(tols[:, 0])).sum()
    # the same scene, the same seed, without the map: it differs from the mapped frame by far more than the bound, pixel by pixel — this is what fails without the feature
    plain, _, _ = render_floor(device, None, reference=False)
    ratio = (np.abs(got - plain)[took] / np.maximum(tols[took], 1e-300)).max(-1)
    print("map against no map: |difference| / bound on the %d mapped pixels: median %.3g, smallest %.3g" % (took.sum(), np.median(ratio), ratio.min()))
    assert np.median(ratio) > 100.0


# ---------------------------------------------------------------- 3. the G-buffer's normal word
def test_the_gbuffer_normal_is_the_mapped_normal(device):
    img = image4()
    words = {}
    for name, image in (("map", img), ("plain", None)):
        rig = Rig(device, floor_scene(image), BLACK, size=(W, H), depth=2, eye=EYE, direction=DIR, vfov=VFOV, mode=lp.BlitMode.DenoisedPathrace)
        rig.r.set_seed(USER_SEED)
        rig.r.reset_accumulation()
        seed = rig.r.frame_state()[1]
        rig.r.raytrace(rig.view)
        g = rig.r.read_denoiser()[0].reshape(-1, 4)
        if image is not None:
            fr = floor_reference(rig.sg, rig.view, seed, image)
        rig.close()
        words[name] = g
    g, c = words["map"], fr["cmp"]
    assert np.array_equal(g[c, 0], fr["prim"][c])
    assert np.array_equal(g[:, 0], words["plain"][:, 0]) and np.array_equal(g[:, 3], words["plain"][:, 3]) and np.array_equal(g[:, 1], words["plain"][:, 1])
    dec = P.oct_decode(g[:, 2])
    want = fr["ref"]["Ns"]
    ang = np.arctan2(np.linalg.norm(np.cross(dec, want), axis=1), np.sum(dec * want, axis=1))
    tol = P.angle_bound(P.normal_code_bound(fr["ref"]["Ns_err"].max(1)))
    print("G-buffer: %d pixels, largest angle / bound %.3g, largest bound %.3g rad" % (c.sum(), (ang / tol)[c].max(), tol[c].max()))
    assert np.all(ang[c] <= tol[c])
    plain_dec = P.oct_decode(words["plain"][:, 2])
    took = c & fr["ref"]["mapped"]
    away = np.arccos(np.clip(np.sum(plain_dec * want, axis=1), -1, 1))[took] / tol[took]
    print("the unmapped normal against the same bound: median angle / bound %.3g" % np.median(away))
    assert np.median(away) > 1.0                             # the assertion above rejects §12's own normal on most mapped pixels: the word does carry the map


# ---------------------------------------------------------------- 4. scene data, bit for bit
ATRIUM = dict(size=(96, 64), depth=2, vfov=T.VFOV)


def _atrium(desc, used=None, image=None, scale=1.5):
    """the small atrium; used True: a normal map on the material of its middle instance, False: on a material no instance uses"""
    s = scenes.to_product(desc)
    if used is not None:
        m = int(s.instances[len(s.instances) // 2]["material_index"]) if used else s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0)
        s.set_material_normal_map(m, s.add_image(image4() if image is None else image), scale)
    return s


def test_an_unused_normal_map_changes_nothing(device, atrium_small):
    desc = atrium_small
    cam = dict(eye=desc["camera"]["origin"], direction=desc["camera"]["direction"])
    for options in (None, {"coop_rays": 0}):                # the shipped launches of this size, and the path kernel's
        a, na = _timed(device, _atrium(desc), desc.get("probe"), options=options, **ATRIUM, **cam)
        b, nb = _timed(device, _atrium(desc, used=False), desc.get("probe"), options=options, **ATRIUM, **cam)
        assert np.all(np.isfinite(a)) and a[..., :3].any() and a.tobytes() == b.tobytes()
        assert na == nb and (na["path"] == 1) == (options is not None), (na, nb)
    c = frame_of(device, _atrium(desc, used=True), desc.get("probe"), n=1, **ATRIUM, **cam)
    assert c.tobytes() != a.tobytes()                        # ... and a used one does change the frame


def check_arms(device, scene, probe, size, n, depth, cam, prepare=None, env=False, denoise=True):
    """the frame is the same bits however it is launched: per-bounce launches, coop-all, sorted queues, raytrace_n against n calls, two shards summed, both denoising modes"""
    sg = lp.SceneGPU.new_from_scene(scene, device)
    kw = dict(size=size, depth=depth, sg=sg, env=env, **cam)

    def frame(n_calls=True, sort=0, **v):
        rig = Rig(device, scene, probe, **kw, **v)
        if prepare is not None:
            prepare(rig.r)
        if sort:
            rig.r.set_sort_queues(sort)
        rig.r.reset_accumulation()
        rig.r.accumulate = True
        if n_calls:
            for _ in range(n):
                rig.r.raytrace(rig.view)
        else:
            rig.r.raytrace_n(rig.view, n)
        img = rig.r.read_radiance()
        rig.close()
        return img

    want = frame(n_calls=False)
    assert np.all(np.isfinite(want)) and want[..., :3].any()
    for v in (dict(), dict(options={"coop_rays": 0}), dict(options={"path_rays": 0}), dict(options={"path_rays": 0x7FFFFFFF, "coop_rays": 0}), dict(options={"packet_primary": 0}),
              dict(options={"tail_lanes": 0}), dict(sort=3, options={"path_rays": 0}), dict(sort=7, options={"path_rays": 0, "coop_rays": 0})):
        assert frame(**v).tobytes() == want.tobytes(), v
    acc = np.zeros_like(want)
    for rank in range(2):
        acc += frame(rank=rank, world=2)
    assert acc.tobytes() == want.tobytes()
    if denoise:
        for mode in (lp.BlitMode.DenoisedPathrace, lp.BlitMode.Temporal):
            one = Rig(device, scene, probe, mode=mode, **kw)
            ranks = [Rig(device, scene, probe, mode=mode, rank=q, world=2, **kw) for q in range(2)]
            for r in [one] + ranks:
                if prepare is not None:
                    prepare(r.r)
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
    return want


def test_launch_independence(device, atrium_small):
    desc = atrium_small
    cam = dict(eye=desc["camera"]["origin"], direction=desc["camera"]["direction"], vfov=T.VFOV)
    check_arms(device, _atrium(desc, used=True), desc.get("probe"), (W, H), 4, 3, cam)


def _moved(dx):
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = dx
    return m.T


def test_tables_follow_the_scene(device):
    kw = dict(size=(W, H), depth=2, eye=EYE, direction=DIR, vfov=VFOV, n=2)
    img = image4()

    def small_quad(s):
        m = s.add_material((0.9, 0.2, 0.2, 1.0), 1.0, 0.0)
        s.set_material_normal_map(m, s.add_image(image53()), 2.5)
        pos = np.array([[-0.5, 0.3, -2.5], [0.5, 0.3, -2.5], [0.5, 0.3, -3.5], [-0.5, 0.3, -3.5]], F)
        s.add_instance(s.add_mesh(pos, np.tile(F([[0, 1, 0]]), (4, 1)), np.ascontiguousarray(pos[:, [0, 2]]), QUAD_IDX), np.eye(4, dtype=np.float32), m)

    def build(dx=0.0, mapped=True):
        s = floor_scene(img, extra=small_quad)
        if not mapped:
            s.set_material_normal_map(1, None)
            s.set_material_normal_map(2, None)
        s.set_instance_transform(1, _moved(dx))
        return s

    fresh, fresh_moved, never = frame_of(device, build(), BLACK, **kw), frame_of(device, build(0.7), BLACK, **kw), frame_of(device, build(mapped=False), BLACK, **kw)
    assert fresh.tobytes() != fresh_moved.tobytes() and fresh.tobytes() != never.tobytes() and fresh[..., :3].any()
    s = build()
    sg = lp.SceneGPU.new_from_scene(s, device)
    s.set_instance_transform(1, _moved(0.7))                # an instance update that moves the mapped quad
    assert sg.update_instances(s) == 1
    assert frame_of(device, s, BLACK, sg=sg, **kw).tobytes() == fresh_moved.tobytes()
    s.set_instance_transform(1, _moved(0.0))
    sg.rebuild(s)                                           # a rebuild
    assert frame_of(device, s, BLACK, sg=sg, **kw).tobytes() == fresh.tobytes()
    _, n_on = _timed(device, s, BLACK, kw["size"], 2, EYE, DIR, VFOV, options={"coop_rays": 0}, sg=sg)
    s.set_material_normal_map(1, None)                      # no map again: the tables are null again, and the path kernel is back
    s.set_material_normal_map(2, None)
    assert s.material_normal_map(1) == (None, 1.0)
    sg.rebuild(s)
    assert frame_of(device, s, BLACK, sg=sg, **kw).tobytes() == never.tobytes()
    _, n_off = _timed(device, s, BLACK, kw["size"], 2, EYE, DIR, VFOV, options={"coop_rays": 0}, sg=sg)
    assert n_on["path"] == 0 and n_off["path"] == 1, (n_on, n_off)
    sg.close()


def test_a_normal_image_that_is_also_half_of_a_pair_stays_resident(device):
    img = image4()
    mra = np.random.RandomState(23).randint(0, 256, (4, 4, 4)).astype(np.uint8)

    def paired(s):      # out of sight: its material makes (image 0, mra) a pair
        add_rect(s, (0, -40.0, 0), (1, 0, 0), (0, 0, 1), 0.5, 0.5, s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0, 0, s.add_image(mra)))

    kw = dict(n=2, size=(W, H), depth=2, eye=EYE, direction=DIR, vfov=VFOV)
    alone = frame_of(device, floor_scene(img), BLACK, **kw)
    both = frame_of(device, floor_scene(img, extra=paired), BLACK, **kw)
    assert alone[..., :3].any() and alone.tobytes() == both.tobytes()
    # an image uploaded ONLY as half of a pair cannot become a normal map without a new upload
    s = lp.Scene()
    s.set_light(0, _dark_light())
    a, b = s.add_image(img), s.add_image(mra)
    m = s.add_material((1.0, 1.0, 1.0, 1.0), 1.0, 0.0, a, b)
    add_rect(s, (0, 0, -3), (0, 0, 1), (1, 0, 0), 1.0, 1.0, m)
    sg = lp.SceneGPU.new_from_scene(s, device)
    s.set_material_normal_map(m, a)
    with pytest.raises(lp.Error) as e:
        sg.rebuild(s)
    assert "only as half of an (albedo, mra) pair" in str(e.value)
    sg.close()


# ---------------------------------------------------------------- 5. together with the other tables
def test_every_side_table_at_once(device):
    """an instantiation-coverage case, not a physics check: one material is normal-mapped, alpha-masked, transmissive and emissive; emitter sampling and env sampling on"""
    probe = np.random.RandomState(5).randint(100, 140, (4, 8, 4)).astype(np.uint8)

    def everything(s):
        i1, i2 = s.add_image(image53()), s.add_image(image4(34))
        m = s.add_material((0.9, 0.8, 0.7, 1.0), 0.6, 0.0, i2)
        s.set_material_normal_map(m, i1, 2.0)
        s.set_material_alpha(m, "MASK", 0.35, i2)
        s.set_material_transmission(m, 0.5, 1.4, True)
        s.set_material_emission(m, (1.0, 0.5, 0.25), 4.0, i2)
        pos = np.array([[-0.8, 0.5, -2.0], [0.8, 0.5, -2.0], [0.8, 0.7, -3.6], [-0.8, 0.7, -3.6]], F)
        nrm = np.tile(F([[0, 1, 0]]), (4, 1))
        s.add_instance(s.add_mesh(pos, nrm, np.ascontiguousarray(pos[:, [0, 2]]), QUAD_IDX), np.eye(4, dtype=np.float32), m)

    scene = floor_scene(image4(), extra=everything)
    cam = dict(eye=EYE, direction=DIR, vfov=VFOV)
    for esamp in (True, False):
        want = check_arms(device, scene, probe, (W, H), 2, 3, cam, prepare=lambda r: r.set_emissive_sampling(esamp), env=True)
        assert want[..., :3].max() > 0.5


# ---------------------------------------------------------------- 6. glTF end to end
GLB_QUAD = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], "<f4")
GLB_UV = np.array([[0, 0], [3, 0], [3, 3], [0, 3]], "<f4")
GLB_CAMERA = ((0.0, 1.5, 5.0), (0.0, -0.35, -1.0))
_DEFAULT = object()


def normal_glb(normal=_DEFAULT):
    """a small .glb: an 8x8 floor whose material has a 4x4 RGBA PNG normalTexture of scale 2, and one directional light (KHR_lights_punctual) shining down and
    forward.  `normal`: another normalTexture member for the floor's material (None: none at all)"""
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

    up = np.tile(np.array([[0, 1, 0]], "<f4"), (4, 1))
    prim = {"attributes": {"POSITION": add(GLB_QUAD, 5126, "VEC3"), "NORMAL": add(up, 5126, "VEC3"), "TEXCOORD_0": add(GLB_UV, 5126, "VEC2")},
            "indices": add(np.array([0, 2, 1, 0, 3, 2], "<u2"), 5123, "SCALAR"), "material": 0}
    mat = {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0], "roughnessFactor": 0.7, "metallicFactor": 0.0}}
    if normal is _DEFAULT:
        normal = {"index": 0, "scale": 2.0}
    if normal is not None:
        mat["normalTexture"] = normal
    q = [float(np.sin(-np.pi / 3)), 0.0, 0.0, float(np.cos(-np.pi / 3))]     # -120 degrees about X: the light's -Z axis points down and towards +z
    js = {"asset": {"version": "2.0"}, "meshes": [{"primitives": [prim]}], "accessors": accessors, "bufferViews": views, "materials": [mat],
          "images": [{"bufferView": view(png_bytes(image4())), "mimeType": "image/png"}], "textures": [{"source": 0}],
          "nodes": [{"mesh": 0, "scale": [4.0, 1.0, 4.0]}, {"rotation": q, "extensions": {"KHR_lights_punctual": {"light": 0}}}],
          "extensionsUsed": ["KHR_lights_punctual"],
          "extensions": {"KHR_lights_punctual": {"lights": [{"type": "directional", "color": [1.0, 0.95, 0.9], "intensity": 3.0}]}},
          "buffers": [{"byteLength": len(blob)}]}
    j = json.dumps(js).encode()
    j += b" " * (-len(j) % 4)
    b = bytes(blob)
    return struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(j) + 8 + len(b)) + struct.pack("<II", len(j), 0x4E4F534A) + j + struct.pack("<II", len(b), 0x004E4942) + b


def test_gltf_normal_map_end_to_end(device):
    with open(os.path.join(HERE, "golden", "normal-map.glb"), "rb") as f:
        assert f.read() == normal_glb()                      # the committed copy is this writer's output
    a = lp.Scene()
    lp.loaders.load_gltf(normal_glb(), a)
    assert a.material_normal_map(1) == (0, 2.0) and a.material_normal_map(0) == (None, 1.0) and a.punctual_count() == 1
    c = lp.Scene()
    img = c.add_image(image4())
    m = c.add_material((0.8, 0.7, 0.6, 1.0), 0.7, 0.0)
    c.set_material_normal_map(m, img, 2.0)
    up = np.tile(F([[0, 1, 0]]), (4, 1))
    s4 = np.diag([4.0, 1.0, 4.0, 1.0]).astype(np.float32)
    c.add_instance(c.add_mesh(GLB_QUAD.astype(F), up, GLB_UV.astype(F), np.array([0, 2, 1, 0, 3, 2], np.uint32)), s4.T, m)
    c.add_punctual_light(a.punctual_lights[:1])              # the loader's record (its direction comes out of the node's rotation): the light is not what is tested
    kw = dict(n=4, size=(96, 54), depth=2, eye=GLB_CAMERA[0], direction=GLB_CAMERA[1], vfov=T.VFOV)
    frames = []
    for s in (a, c):
        s.set_light(0, _dark_light())
        frames.append(frame_of(device, s, BLACK, **kw))
    assert np.all(np.isfinite(frames[0])) and frames[0][..., :3].any() and frames[0].tobytes() == frames[1].tobytes()
    b = lp.Scene()
    lp.loaders.load_gltf(normal_glb(normal=None), b)         # the same file without the member renders a flat floor: another frame
    b.set_light(0, _dark_light())
    flat = frame_of(device, b, BLACK, **kw)
    assert flat[..., :3].any() and flat.tobytes() != frames[0].tobytes()


def test_bench_renders_the_normal_map_file():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--frames-per-step", "2", "--width", "256", "--height", "256", "--no-extras",
                        "--camera", "0,1.5,5,0,-0.35,-1", "--gltf", os.path.join(HERE, "golden", "normal-map.glb")], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert j["data"] == "real" and "normal-map.glb" in j["config"]["workload"] and j["config"]["frame_complete"] is True and j["value"] > 0
