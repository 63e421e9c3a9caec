"""-m gpu: shadows of punctual lights through thin-walled transmissive panes (SPEC.md §27, `Renderer.set_glass_shadows`).

1. the traversal's own function (`SceneGPU.glass_shadow`) against tests/glass_shadow_ref.py, bit for bit;
2./3. a floor under a horizontal pane (two stacked panes) and one directional light: over a region wholly in the pane's shadow the ratio of the frame's mean to the
   mean of the frame without the pane is the binary64 tau per channel (the product of the two);
4. frames that must not change, bit for bit, through the new kernel; 5. one frame however it is launched; 6. a cut-away masked card in front of the pane;
7. the golden glTF file end to end.

THE BOUND of 2 and 3 (the issue's): 5 sigma, sigma = sqrt(tau_c (1 - tau_c) / n), n = pixels x samples, plus 32 x 2^-24 relative for the binary32 accumulation of
16 samples and the two means.  Per sample and channel the frame with the pane is the frame without it or 0 (the same sample picks the light in both and arrives
with the same contribution; the pane decides with probability tau_c), so the ratio of the means is a mean of Bernoulli trials.  Only the samples that pick the
punctual light are trials — every scene also has its one rectangle light, dark here, which takes half of the light samples (SPEC §19) —, so the bound as
stated is about 3.5 standard deviations of the ratio; the figures are printed."""
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A, testing as T

import glass_shadow_ref as G
import transmission_ref as R
from test_gpu_env_sampling import _dark_light
from test_gpu_transmission import GLB_FLOOR, GLB_PANE, QUAD_IDX, cube_mesh, glass_glb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
INVALID = A.INVALID_INDEX
W = H = 64
SPP = 16
VFOV = 0.6
BASE = (0.5, 1.0, 0.25)
EYE_Y, EYE_Z, DIR = 1.2, 4.0, (0.0, -0.5, -1.0)        # below every pane, looking down: no camera ray meets a pane on its way to the floor
FLOOR_N, FLOOR_HALF = 4, 12.0                           # a 4x4-cell floor: 32 triangles (prims 0..31), enough for the GPU builder and a real rebuild


# ---------------------------------------------------------------- scenes
def _floor_mesh():
    g = np.linspace(-FLOOR_HALF, FLOOR_HALF, FLOOR_N + 1, dtype=np.float32)
    pos = np.array([[x, 0.0, z] for z in g for x in g], np.float32)
    idx = []
    for j in range(FLOOR_N):
        for i in range(FLOOR_N):
            a = j * (FLOOR_N + 1) + i
            idx += [a, a + FLOOR_N + 2, a + 1, a, a + FLOOR_N + 1, a + FLOOR_N + 2]      # wound so that the normal is +y
    return pos, np.array(idx, np.uint32)


def _quad(s, y, half, mat, cx=0.0, uv=None):
    """a horizontal quad at height y, |x - cx|, |z| <= half, normal +y"""
    pos = np.array([[cx - half, y, -half], [cx - half, y, half], [cx + half, y, half], [cx + half, y, -half]], np.float32)
    nrm = np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))
    blas = s.add_mesh(pos, nrm, np.zeros((4, 2), np.float32) if uv is None else uv, QUAD_IDX)
    return s.add_instance(blas, np.eye(4, dtype=np.float32), mat)


PANE1 = dict(y=2.0, half=3.0, base=BASE, metal=0.0, tr=1.0, ior=1.5, thin=True)
PANE2 = dict(y=3.0, half=4.5, base=(1.0, 0.5, 0.75), metal=0.25, tr=1.0, ior=2.4, thin=True)


def sun(angle):
    """a directional light that shines down at `angle` from the vertical, leaning towards +x -> (record, wi: the unit direction TOWARDS the light)"""
    d = np.array([np.sin(angle), -np.cos(angle), 0.0])
    return lp.directional_light(tuple(d), color=(1.0, 0.95, 0.9), intensity=3.0), -d


def sky_scene(panes=(PANE1,), angle=0.0, light=True, card=None, far_pane=False):
    """the floor, the panes above it (in order: their prims follow the floor's), one directional light.  `card` = (cutoff, half size, centre x): a masked opaque
    quad at height 1.6, under the panes, after them in prim order (no image, alpha 1: kept at a cutoff up to 1, cut away above).  `far_pane`: one more thin pane far outside the light's way (so that a scene whose own pane is solid or
    opaque still has thin glass in use)"""
    s = lp.Scene()
    s.set_light(0, _dark_light())
    fpos, fidx = _floor_mesh()
    floor = s.add_mesh(fpos, np.tile(np.array([[0, 1, 0]], np.float32), (len(fpos), 1)), None, fidx)
    s.add_instance(floor, np.eye(4, dtype=np.float32), s.add_material((0.8, 0.8, 0.8, 1.0), 1.0, 0.0))
    for p in panes:
        m = s.add_material(tuple(p["base"]) + (1.0,), 0.3, p["metal"])
        if p["tr"] is not None:
            s.set_material_transmission(m, p["tr"], p["ior"], p["thin"])
        _quad(s, p["y"], p["half"], m, cx=p.get("cx", 0.0))
    if far_pane:
        m = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
        s.set_material_transmission(m, 1.0, 1.5, True)
        _quad(s, -5.0, 0.5, m, cx=40.0)           # under the floor's level and beside it: neither a camera ray nor a shadow ray gets there
    if card is not None:
        m = s.add_material((0.8, 0.2, 0.2, 1.0), 1.0, 0.0)
        s.set_material_alpha(m, A.ALPHA_MASK, card[0])
        _quad(s, 1.6, card[1], m, cx=card[2])
    if light:
        s.add_punctual_light(sun(angle)[0])
    return s


def eye_for(angle, y=2.0):
    return (y * np.tan(angle), EYE_Y, EYE_Z)      # the camera follows the shadow of the pane's centre


class Rig:
    def __init__(self, device, scene, size=(W, H), depth=1, eye=None, glass=True, stats=False, options=None, lanes=None, rank=0, world=1, sg=None):
        self.own_sg = sg is None
        self.sg = lp.SceneGPU.new_from_scene(scene, device) if sg is None else sg
        self.r = r = lp.Renderer(device, size)
        r.downsample_factor = 1.0
        r.resize(device, self.sg, None, size)
        r.set_max_bounces(depth)
        r.set_vfov(VFOV)
        for k, v in (options or {}).items():
            r.set_option(k, v)
        if lanes is not None:
            r.set_lanes(lanes)
        if world > 1:
            r.set_shard(rank, world)
            r.set_resources(device, self.sg, None)
        if stats:
            r.enable_stats(True)
        r.set_glass_shadows(glass)
        assert r.glass_shadows is bool(glass)
        self.view = T.look(eye_for(0.0) if eye is None else eye, DIR)

    def frame(self, n=SPP, fused=False):
        self.r.reset_accumulation()
        self.r.accumulate = True
        self.r.reset_ray_counts()
        if fused:
            self.r.raytrace_n(self.view, n)
        else:
            for _ in range(n):
                self.r.raytrace(self.view)
        return self.r.read_radiance()

    def close(self):
        self.r.close()
        if self.own_sg:
            self.sg.close()


def frame_of(device, scene, n=SPP, fused=False, **kw):
    rig = Rig(device, scene, **kw)
    img = rig.frame(n, fused)
    rig.close()
    return img


# ---------------------------------------------------------------- 1. the hook against the reference, bit for bit
def _image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


HOOK_P = np.array([[-0.85, -0.45, -2.0], [0.85, -0.45, -2.0], [0.85, 0.45, -2.0], [-0.85, 0.45, -2.0]], np.float32)       # axis-aligned: Ng = (0, 0, 1.53), c exact
HOOK_T = np.array([[-0.7, -0.5, -2.3], [0.9, -0.3, -1.6], [0.6, 0.8, -1.9], [-1.0, 0.6, -2.6]], np.float32)             # tilted (planar or not: each triangle has its own Ng)
HOOK_UV = np.array([[0.0, 0.0], [2.5, 0.0], [2.5, 1.25], [0.0, 1.25]], np.float32)                                     # the textures repeat


def _hook_scene():
    """-> (scene, entries): one quad (two prims) per material; entry = (first prim, vertices[4, 3], dict of the material)"""
    s = lp.Scene()
    s.set_light(0, _dark_light())
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    meshes = [(s.add_mesh(HOOK_P, nrm, HOOK_UV, QUAD_IDX), HOOK_P), (s.add_mesh(HOOK_T, nrm, HOOK_UV, QUAD_IDX), HOOK_T)]
    tex = {"none": (None, None), "paired": (_image(4, 4, 1), _image(4, 4, 2)), "unequal": (_image(3, 5, 3), _image(4, 4, 4))}
    ids = {k: tuple(INVALID if im is None else s.add_image(im) for im in v) for k, v in tex.items()}
    entries, prim, k = [], 0, 0
    kinds = [dict(tex=t, metal=m, tr=tr, ior=ior, thin=True) for t in tex for m in (0.0, 0.5, 1.0) for tr in (0.25, 1.0) for ior in (1.0, 1.5, 2.4)]
    kinds += [dict(tex="paired", metal=0.0, tr=1.0, ior=1.5, thin=False), dict(tex="none", metal=0.0, tr=None, ior=1.5, thin=True)]      # a solid, an opaque
    for kd in kinds:
        color = (0.5 + 0.05 * (k % 7), 1.0, 0.25 + 0.1 * (k % 5), 1.0)
        m = s.add_material(color, 0.3, kd["metal"], albedo_texture=ids[kd["tex"]][0], mra_texture=ids[kd["tex"]][1])
        if kd["tr"] is not None:
            s.set_material_transmission(m, kd["tr"], kd["ior"], kd["thin"])
        blas, pos = meshes[k % 2]
        s.add_instance(blas, np.eye(4, dtype=np.float32), m)
        entries.append((prim, pos, dict(kd, color=color, albedo=tex[kd["tex"]][0], mra=tex[kd["tex"]][1])))
        prim, k = prim + 2, k + 1
    deg = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [1.0, 0.2, 0.3]], np.float32)      # a zero-area triangle of a thin pane
    m = s.add_material((1.0, 1.0, 1.0, 1.0), 0.3, 0.0)
    s.set_material_transmission(m, 1.0, 1.5, True)
    s.add_instance(s.add_mesh(deg, None, None, np.arange(3, dtype=np.uint32)), np.eye(4, dtype=np.float32), m)
    return s, entries, prim


def _hook_elements(pos, tri):
    """(hu, hv, d) for triangle `tri` (0, 1) of the quad `pos`: barycentrics at the corners, on the edges and inside x directions at c = 1, 0.5, 1e-3 and 0 from
    both sides (about the triangle's own binary32 normal) and random ones"""
    p = pos[QUAD_IDX[3 * tri:3 * tri + 3]]
    bary = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.0), (0.3, 0.3), (0.125, 0.625), (0.7, 0.05)]
    rng = np.random.default_rng(100 + tri)
    u = rng.random(22)
    bary += list(zip(u, rng.random(22) * (1 - u)))
    n = np.cross(p[1].astype(np.float64) - p[0], p[2].astype(np.float64) - p[0])
    n /= np.linalg.norm(n)
    t = np.cross(n, [0.3, 0.2, 0.9])
    t /= np.linalg.norm(t)
    dirs = []
    for c in (1.0, 0.5, 1e-3, 0.0):
        for side in (1.0, -1.0):
            dirs.append(side * c * n + np.sqrt(1 - c * c) * t)
    r = rng.normal(size=(8, 3))
    dirs += list(r / np.linalg.norm(r, axis=1, keepdims=True))
    b = np.array([bb for bb in bary for _ in dirs], np.float32)
    d = np.array([dd for _ in bary for dd in dirs], np.float32)
    return p, b[:, 0].copy(), b[:, 1].copy(), d


def test_hook_equals_the_reference_bit_for_bit(device):
    s, entries, deg_prim = _hook_scene()
    sg = lp.SceneGPU.new_from_scene(s, device)
    prims, hus, hvs, ds, want_t, want_x, want_b = [], [], [], [], [], [], []
    for first, pos, kd in entries:
        for tri in (0, 1):
            p, hu, hv, d = _hook_elements(pos, tri)
            uv = HOOK_UV[QUAD_IDX[3 * tri:3 * tri + 3]]
            trans = None if kd["tr"] is None else (kd["tr"], kd["ior"], kd["thin"])
            t, x, b = G.decide(first + tri, p, uv, kd["color"], kd["metal"], kd["albedo"], kd["mra"], trans, hu, hv, d)
            prims.append(np.full(len(hu), first + tri, np.uint32)); hus.append(hu); hvs.append(hv); ds.append(d)
            want_t.append(t); want_x.append(x); want_b.append(b)
            if trans is None or not kd["thin"]:
                assert not b.any() and not t.any()               # a solid and an opaque triangle block
    n_deg = 8
    prims.append(np.full(n_deg, deg_prim, np.uint32)); hus.append(np.linspace(0, 0.5, n_deg).astype(F)); hvs.append(np.linspace(0.4, 0, n_deg).astype(F))
    ds.append(np.tile(np.array([[0, 0, 1]], F), (n_deg, 1)))
    want_t.append(np.zeros((n_deg, 3), F)); want_x.append(G.xi(deg_prim, hus[-1], hvs[-1])); want_b.append(np.zeros(n_deg, np.uint32))
    prim, hu, hv, d = np.concatenate(prims), np.concatenate(hus), np.concatenate(hvs), np.concatenate(ds)
    want_t, want_x, want_b = np.concatenate(want_t), np.concatenate(want_x), np.concatenate(want_b)
    got = sg.glass_shadow(prim, np.stack([hu, hv], 1), d)
    with pytest.raises(lp.Error):
        sg.glass_shadow(np.array([deg_prim + 1], np.uint32), np.zeros((1, 2), F), np.array([[0, 0, 1]], F))      # beyond the baked triangles
    sg.close()
    print("hook: %d elements, bits histogram %s" % (len(prim), np.bincount(want_b, minlength=8).tolist()))
    assert len(prim) > 50000 and np.all(np.bincount(want_b, minlength=8)[[0, 7]] > 1000) and len(np.unique(want_b)) >= 4
    bad = (got["tau"].view(np.uint32) != want_t.view(np.uint32)).any(1)
    assert not bad.any(), (int(bad.sum()), prim[bad][:4], got["tau"][bad][:4], want_t[bad][:4])
    assert np.array_equal(got["xi"].view(np.uint32), want_x.view(np.uint32))
    assert np.array_equal(got["bits"], want_b)


# ---------------------------------------------------------------- 2./3. the skylight
def _shadow_region(eye, wi, panes, margin=0.1):
    """pixels whose four corners see floor points that lie under every pane along wi, `margin` inside its border (SPEC §11 in float64)"""
    view = T.look(eye, DIR)
    o, d = R.camera_rays(view, VFOV, W, H, np.array([0.0, 1.0]))
    assert (d[..., 1] < -1e-3).all()                      # every ray goes down: none meets a pane (the camera is below them)
    P = o + d * (-o[1] / d[..., 1])[..., None]            # [h, w, 4, 3] on the floor
    assert np.abs(P[..., [0, 2]]).max() < FLOOR_HALF
    ok = np.ones(P.shape[:3], bool)
    for p in panes:
        Q = P + wi * (p["y"] / wi[1])
        ok &= (np.abs(Q[..., 0] - p.get("cx", 0.0)) < p["half"] - margin) & (np.abs(Q[..., 2]) < p["half"] - margin)
    return ok.all(-1)


def _tau64(p, c):
    return G.tau([p["base"]], F(p["metal"]), F(p["tr"]), F(p["ior"]), F(c), np.float64)[0]


def _check_ratio(name, on, without, off, region, tau):
    n = int(region.sum()) * SPP
    assert region.sum() >= 300, int(region.sum())
    assert not off[region][:, :3].any()                                    # the switch off: today's frame, black under the pane
    num, den = on[region][:, :3].astype(np.float64).mean(0), without[region][:, :3].astype(np.float64).mean(0)
    assert (den > 0.01).all()
    ratio = num / den
    sigma = np.sqrt(tau * (1 - tau) / n)
    bound = 5 * sigma + 32 * 2.0 ** -24 * tau
    print("%s: %d pixels x %d samples; ratio %s, tau %s, (ratio - tau) / sigma %s" % (name, region.sum(), SPP, ratio, tau, (ratio - tau) / sigma))
    assert np.all(np.abs(ratio - tau) <= bound), (name, ratio, tau, sigma)


@pytest.mark.parametrize("angle", [0.0, np.pi / 3], ids=["straight-down", "60-degrees"])
def test_skylight_ratio_is_tau(device, angle):
    eye, wi = eye_for(angle), sun(angle)[1]
    region = _shadow_region(eye, wi, [PANE1])
    on = frame_of(device, sky_scene(angle=angle), eye=eye)
    off = frame_of(device, sky_scene(angle=angle), eye=eye, glass=False)
    without = frame_of(device, sky_scene(panes=(), angle=angle), eye=eye)
    assert np.all(np.isfinite(on))
    _check_ratio("one pane", on, without, off, region, _tau64(PANE1, np.cos(angle)))
    # per pixel and channel the frame is made of the same contributions: never more light than without the pane
    assert (on[..., :3] <= without[..., :3]).all()


def test_stacked_panes_give_the_product(device):
    angle = np.pi / 6
    eye, wi = eye_for(angle), sun(angle)[1]
    panes = (PANE1, PANE2)
    region = _shadow_region(eye, wi, panes)
    on = frame_of(device, sky_scene(panes=panes, angle=angle), eye=eye)
    off = frame_of(device, sky_scene(panes=panes, angle=angle), eye=eye, glass=False)
    without = frame_of(device, sky_scene(panes=(), angle=angle), eye=eye)
    c = np.cos(angle)
    _check_ratio("two panes", on, without, off, region, _tau64(PANE1, c) * _tau64(PANE2, c))


# ---------------------------------------------------------------- 4. what must not change, through the new kernel
# the counters that are a function of the rays and the tree.  The others — wave_steps and the lane counts, the occluder-cache probe, wave_rays (the rays the waves'
# tails finished cooperatively) — depend on which rays happen to share a wave and in which order they finish: they vary from run to run of one build
COUNTED = ("closest", "shadow", "shaded", "primary", "nodes", "tris", "shadow_nodes", "shadow_tris", "packet_nodes", "packet_tris", "shadow_occluded")
PLAN_MARKS = ("primary", "wave_rays", "occluder_cache_found")      # non-zero only under the packet kernel, the tail in place, the occluder probe: what the plain step's plan excludes


def _counts(r):
    c = r.ray_counts()
    return {f: getattr(c, f) for f in COUNTED}, {f: getattr(c, f) for f in PLAN_MARKS}


def test_a_metallic_pane_and_a_solid_one_block_as_ever(device):
    metal = dict(PANE1, metal=1.0)                          # tau = 0: the new kernel runs (thin glass in use) and every ray is stopped
    a, b = frame_of(device, sky_scene(panes=(metal,))), frame_of(device, sky_scene(panes=(metal,)), glass=False)
    assert a.tobytes() == b.tobytes() and a[..., :3].max() > 0.01
    solid = dict(PANE1, thin=False)                         # a solid in place of the thin pane; the far pane keeps thin glass in use
    a, b = frame_of(device, sky_scene(panes=(solid,), far_pane=True)), frame_of(device, sky_scene(panes=(solid,), far_pane=True), glass=False)
    assert a.tobytes() == b.tobytes()
    opaque = dict(PANE1, tr=None)
    a, b = frame_of(device, sky_scene(panes=(opaque,), far_pane=True)), frame_of(device, sky_scene(panes=(opaque,), far_pane=True), glass=False)
    assert a.tobytes() == b.tobytes()
    # ... and the thin pane itself does change the frame
    assert frame_of(device, sky_scene()).tobytes() != frame_of(device, sky_scene(), glass=False).tobytes()


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("what", ["no-punctual-light", "no-thin-glass"])
def test_without_a_light_or_without_thin_glass_the_launches_are_the_parents(device, what, stats):
    scene = (lambda: sky_scene(light=False)) if what == "no-punctual-light" else (lambda: sky_scene(panes=(dict(PANE1, thin=False),)))
    out = []
    for glass in (True, False):
        rig = Rig(device, scene(), size=(256, 144), depth=3, glass=glass, stats=stats, options={"packet_primary": 1})
        img = rig.frame(2)
        out.append((img, _counts(rig.r), rig.r.submission_stats()))
        rig.close()
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1][0] == out[1][1][0] and out[0][2] == out[1][2], (out[0][1], out[1][1])
    for _, (_, marks), _ in out:
        assert marks["primary"] > 0                         # the packet kernel ran: not the plain step's plan
        if not stats:
            assert marks["wave_rays"] > 0, marks            # ... and so did the tail in place
        elif what == "no-thin-glass":
            assert marks["occluder_cache_found"] > 0, marks # ... and the occluder probe of the stats kernels (the scene without a light casts no shadow ray)


# ---------------------------------------------------------------- 5. one frame however it is launched
BOUNCES = 3
SIZES = [(64, 36), (256, 144)]          # 2 samples: 4 608 rays (the class of coop-all) and 73 728 (the class of the path kernel)
VARIANTS = ["default", "stats", "packet", "lanes", "raytrace_n", "shards"]


def _variant_frame(device, scene, size, variant, sg=None, glass=True):
    out = None
    for rank in range(2 if variant == "shards" else 1):
        rig = Rig(device, scene, size=size, depth=BOUNCES, stats=variant == "stats", options={"packet_primary": 1} if variant == "packet" else None,
                  lanes=2 if variant == "lanes" else None, rank=rank, world=2 if variant == "shards" else 1, sg=sg, glass=glass)
        part = rig.frame(2, fused=variant == "raytrace_n")
        out = part if out is None else out + part           # the ranks' buffers are zero outside their tiles (SPEC §13)
        rig.close()
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_one_frame_on_every_launch_path(device, size):
    scene = lambda: sky_scene(panes=(PANE1, PANE2), angle=np.pi / 6, card=(0.5, 1.0, -1.5))      # a small card, kept: an occluder under a part of the panes, and the alpha table is in use
    want = _variant_frame(device, scene(), size, "default")
    assert np.all(np.isfinite(want)) and want[..., :3].max() > 0.01
    assert want.tobytes() != _variant_frame(device, scene(), size, "default", glass=False).tobytes()
    for v in VARIANTS[1:]:
        assert _variant_frame(device, scene(), size, v).tobytes() == want.tobytes(), v


def test_refit_and_rebuild_keep_the_frame(device):
    size = (64, 36)
    moved = np.eye(4, dtype=np.float32)
    moved[:3, 3] = (0.6, 0.25, -0.4)
    make = lambda: sky_scene(panes=(PANE1, PANE2), angle=np.pi / 6)
    scene = make()
    inst = 1                                                # the first pane
    fresh = make()
    fresh.set_instance_transform(inst, moved.T)
    want = _variant_frame(device, fresh, size, "default")
    assert want.tobytes() != _variant_frame(device, scene, size, "default").tobytes()
    sg = lp.SceneGPU.new_from_scene(scene, device)
    scene.set_instance_transform(inst, moved.T)
    sg.update_instances(scene)
    assert _variant_frame(device, scene, size, "default", sg=sg).tobytes() == want.tobytes()
    sg.rebuild(scene)
    assert _variant_frame(device, scene, size, "default", sg=sg).tobytes() == want.tobytes()
    # a material that stops being thin-walled: the update re-derives the count, and the frame is the switch-off frame of that scene
    thin = [m for m in range(scene.counts().materials) if scene.material_transmission(m)[0] > 0]
    assert len(thin) == 2
    for m in thin:
        scene.set_material_transmission(m, 1.0, scene.material_transmission(m)[1], False)
    sg.rebuild(scene)
    got = _variant_frame(device, scene, size, "default", sg=sg)
    sg.close()
    solid = sky_scene(panes=(dict(PANE1, thin=False), dict(PANE2, thin=False)), angle=np.pi / 6)
    solid.set_instance_transform(inst, moved.T)
    rig = Rig(device, solid, size=size, depth=BOUNCES, glass=False)
    assert got.tobytes() == rig.frame(2).tobytes()
    rig.close()


# ---------------------------------------------------------------- 6. a masked card, cut fully away, in front of the pane
def test_a_cut_away_masked_card_changes_nothing(device):
    with_card = frame_of(device, sky_scene(card=(2.0, 5.0, 0.0)))       # cutoff 2: every hit on the card is rejected (SPEC §20); it comes last, so the prim ids agree
    assert with_card.tobytes() == frame_of(device, sky_scene()).tobytes()
    kept = frame_of(device, sky_scene(card=(0.5, 5.0, 0.0)))            # the same card kept: an occluder under the pane
    region = _shadow_region(eye_for(0.0), sun(0.0)[1], [PANE1])
    assert not kept[region][:, :3].any() and with_card[region][:, :3].any()


# ---------------------------------------------------------------- 7. glTF end to end
GLB_EYE, GLB_DIR = (0.5, 1.2, 5.0), (0.0, -0.15, -1.0)


def _glb_frame(device, s, glass=True):
    s.set_light(0, _dark_light())
    sg = lp.SceneGPU.new_from_scene(s, device)
    r = lp.Renderer(device, (96, 64))
    r.downsample_factor = 1.0
    r.resize(device, sg, None, (96, 64))
    r.set_max_bounces(2)            # the floor behind the pane is seen through it: the pane, then the floor and its shadow ray
    r.set_vfov(T.VFOV)
    r.set_glass_shadows(glass)
    r.reset_accumulation()
    r.accumulate = True
    for _ in range(8):
        r.raytrace(T.look(GLB_EYE, GLB_DIR))
    img = r.read_radiance()
    r.close()
    sg.close()
    return img


def test_gltf_glass_end_to_end(device):
    with open(os.path.join(HERE, "golden", "glass-pane.glb"), "rb") as f:
        data = f.read()
    assert data == glass_glb()

    def loaded(slanted):
        a = lp.Scene()
        lp.loaders.load_gltf(data, a)
        if slanted:       # the file's sun shines straight down, along its vertical pane; the same file with the sun 45 degrees from behind the pane
            a.set_punctual_light(0, lp.directional_light((0.0, -1.0, -1.0), color=(1.0, 0.95, 0.9), intensity=3.0))
        return a

    def by_hand(a):
        c = lp.Scene()
        mats = [c.add_material((0.8, 0.7, 0.6, 1.0), 0.6, 0.1), c.add_material((0.5, 1.0, 0.25, 1.0), 0.1, 0.0), c.add_material((1.0, 1.0, 1.0, 1.0), 0.1, 0.0)]
        c.set_material_transmission(mats[1], 1.0)
        c.set_material_transmission(mats[2], 0.9, ior=1.33, thin_walled=False)
        up, front = np.tile(np.float32([[0, 1, 0]]), (4, 1)), np.tile(np.float32([[0, 0, 1]]), (4, 1))
        cp, cn, ci = cube_mesh(0.5)
        blas = [c.add_mesh(GLB_FLOOR.astype(np.float32), up, None, np.array([0, 2, 1, 0, 3, 2], np.uint32)), c.add_mesh(GLB_PANE.astype(np.float32), front, None, QUAD_IDX),
                c.add_mesh(cp, cn, None, ci)]

        def trs(t=(0, 0, 0), s=(1, 1, 1)):
            m = np.diag(list(s) + [1.0]).astype(np.float32)
            m[:3, 3] = t
            return m.T

        c.add_instance(blas[0], trs(s=(4, 1, 4)), mats[0])
        c.add_instance(blas[1], trs(t=(0, 0, 1)), mats[1])
        c.add_instance(blas[2], trs(t=(1.5, 0.5, -1.0)), mats[2])
        c.add_punctual_light(a.punctual_lights[:1].copy())
        return c

    for slanted in (False, True):
        a = loaded(slanted)
        on = _glb_frame(device, a)
        assert np.all(np.isfinite(on)) and on.tobytes() == _glb_frame(device, by_hand(loaded(slanted))).tobytes()
        off = _glb_frame(device, loaded(slanted), glass=False)
        # the floor behind the pane (-1 < z < 1), seen through it from the camera at z = 5 (SPEC §11: z = -1 is row 35.8, z = 1 row 43; the pane spans columns 19..57)
        behind = on[37:42, 30:50, :3]
        assert (behind.mean((0, 1)) > 0).all(), behind.mean((0, 1))
        if slanted:
            # there the pane's shadow falls (the light comes down at 45 degrees from the camera's side).  With the switch off all that these pixels show is the lit
            # floor in front of the pane, mirrored in it (Fresnel, a few per cent); with it on the same samples add what the pane lets through, tinted by it
            assert (on[..., :3] >= off[..., :3]).all()
            gain = (behind.astype(np.float64) - off[37:42, 30:50, :3]).mean((0, 1))
            print("glTF: behind the pane off %s, on %s" % (off[37:42, 30:50, :3].mean((0, 1)), behind.mean((0, 1))))
            assert gain[1] > gain[0] > gain[2] > 0, gain  # base (0.5, 1, 0.25) twice (the view and the light) over a floor of (0.8, 0.7, 0.6) under a light of (1, 0.95, 0.9)
            assert behind[..., 1].mean() > 2 * off[37:42, 30:50, 1].mean()
        else:
            assert on.tobytes() == off.tobytes()          # the file's own sun shines along its pane: no shadow ray meets it, and the solid cube blocks either way
