"""-m gpu: k_shade's shade_hit_early issues a hit's independent loads together, each under its lane's predicate, and waits once (kernels.h).  No arithmetic and no store
changed, so every frame is what it was, bit for bit.  What can go wrong is a WAVE WHOSE LANES ARE OF DIFFERENT KINDS — a load issued for the wrong lanes, a row read
before it has landed, a miss's radiance row taken for an emitter's — so the scene forces the mix at the smallest size:

`board`: a camera over a coarse checkerboard of small quads (three materials: plain, an albedo image, an albedo + roughness / metallic pair) with sky — a probe that is
not constant — between them and one rectangle light standing in view.  At 64 x 36 a wave's 8 x 8 pixels hold surface hits, misses and emitter hits side by side
(asserted from the primary hits), and so do the bounces behind them.

The references, all bit for bit:
 * the CPU oracle (oracle/harness.py) for everything it renders: the board, with and without the noise texture (whose texel is one of the moved loads), through the
   three pipelines, with more lights than the table in LDS holds, and the closed box that has neither a miss nor an emitter hit;
 * tests/golden/shade_load_order_frames.npz (the 64 x 36 frames themselves, float32) and .json (their ray counts and SHA-256) for the feature forms (ENV, PUNCT,
   EMIS | ESAMP, TRANS, NMAP): the oracle has no SPEC §18 - §24, so the library's own frames from BEFORE the change are the only bit-exact reference there is (written
   by tests/golden/make_shade_load_order.py on an MI355X with the parent commit's library; a frame is keyed by pixel slot and depends on neither the grid nor the order
   of the queues, so they hold on any device).  A frame that differs is reported by how many pixels differ and by how much."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T
from oracle import harness

import emissive_ref as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "shade_load_order_frames.json")
GOLDEN_FRAMES = os.path.join(HERE, "golden", "shade_load_order_frames.npz")
LIGHT_DT = [("normal", "<f4", 4), ("tangent", "<f4", 4), ("bitangent", "<f4", 4), ("origin", "<f4", 4)]
INVALID = scenes.INVALID
SMALL, MID, SPP, DEPTH = (64, 36), (160, 96), 2, 4
CAMERA = {"origin": (0.3, 2.6, 4.0), "direction": (-0.04, -0.55, -1.0)}
PROBE = np.random.RandomState(7).randint(90, 135, (4, 8, 4)).astype(np.uint8)       # RGBE, 8 x 4, no two texels alike: the four taps and their weights matter
NOISE = np.random.default_rng(5).integers(0, 256, (16, 16, 4), dtype=np.uint8)
STAGES = ("primary intersection", "intersection", "shadow", "shading", "path")
PER_BOUNCE = {"path_rays": 0, "coop_rays": 0}                  # k_shade + k_trace, one launch per bounce
K_PATH = {"coop_rays": 0}                                      # the default rule without the wave-per-ray arm: k_path at these sizes
WAVE_PER_RAY = {"coop_rays": 0x7FFFFFFF}


def rect_light(origin, tangent, bitangent, hw, hh, le):
    l = np.zeros(1, LIGHT_DT)
    l["normal"] = tuple(np.cross(tangent, bitangent)) + (0.0,)
    l["tangent"] = tuple(tangent) + (hw,)
    l["bitangent"] = tuple(bitangent) + (hh,)
    l["origin"] = tuple(origin) + (le,)
    return l


def quad(center, u, v, hu, hv):
    """the rectangle center +- hu u +- hv v: two triangles, geometric normal u x v, uv over [0, 1.5]^2 (the images repeat)"""
    c, u, v = (np.asarray(a, np.float64) for a in (center, u, v))
    pos = np.array([c - hu * u - hv * v, c + hu * u - hv * v, c + hu * u + hv * v, c - hu * u + hv * v], np.float32)
    nrm = np.tile(np.cross(u, v).astype(np.float32)[None], (4, 1))
    uv = np.array([[0, 0], [1.5, 0], [1.5, 1.5], [0, 1.5]], np.float32)
    return {"positions": pos, "normals": nrm, "uvs": uv, "indices": np.array([0, 1, 2, 0, 2, 3], np.uint32)}


def images():
    rng = np.random.RandomState(3)
    albedo = rng.randint(40, 256, (8, 8, 4)).astype(np.uint8)
    mra = rng.randint(30, 220, (8, 8, 4)).astype(np.uint8)      # the same size as the albedo: the two are stored as one paired image
    other = rng.randint(40, 256, (5, 7, 4)).astype(np.uint8)    # an image of its own, at a size that is no power of two
    return [albedo, mra, other]


MATERIALS = [((0.8, 0.8, 0.8, 1), 0.6, 0.0, INVALID, INVALID), ((1.0, 1.0, 1.0, 1), 0.5, 0.1, 0, 1), ((0.9, 0.7, 0.5, 1), 0.3, 0.0, 2, INVALID)]
IDENT = np.eye(4, dtype=np.float32)


def board(lights=1):
    """an 8 x 8 checkerboard on y = 0 with every other cell missing (0.9-wide quads in 1-wide cells: sky shows between them and through the holes), the materials taken
    in turn; light 0 stands behind the board facing the camera, the further ones (lights > 1) hang over the board facing down"""
    meshes, instances = [], []
    for iz in range(8):
        for ix in range(8):
            if (ix + iz) & 1:
                continue
            meshes.append(quad((ix - 3.5, 0.0, -iz + 1.5), (0, 0, 1), (1, 0, 0), 0.45, 0.45))       # (0, 0, 1) x (1, 0, 0) = (0, 1, 0): facing up
            instances.append((len(meshes), IDENT, 1 + (len(meshes) - 1) % 3))
    ls = [rect_light((0.0, 1.0, -5.0), (1, 0, 0), (0, 1, 0), 1.2, 0.7, 6.0)]
    for k in range(1, lights):
        ls.append(rect_light((-3.0 + 1.4 * k, 1.8 + 0.1 * k, -2.0 + 0.5 * k), (1, 0, 0), (0, 0, 1), 0.4, 0.3, 3.0 + k))   # (1, 0, 0) x (0, 0, 1) = (0, -1, 0)
    return {"name": "board(lights=%d)" % lights, "meshes": meshes, "instances": instances, "materials": MATERIALS, "images": images(), "lights": ls,
            "probe": PROBE, "camera": CAMERA}


def box():
    """a closed 4 x 3 x 6 room around the camera; the light hangs under the ceiling BEHIND the camera, facing down: no ray of a depth-1 frame leaves or finds it"""
    walls = [((0, 0, 0), (0, 0, 1), (1, 0, 0), 3.0, 2.0), ((0, 3, 0), (1, 0, 0), (0, 0, 1), 2.0, 3.0), ((-2, 1.5, 0), (0, 1, 0), (0, 0, 1), 1.5, 3.0),
             ((2, 1.5, 0), (0, 0, 1), (0, 1, 0), 3.0, 1.5), ((0, 1.5, -3), (1, 0, 0), (0, 1, 0), 2.0, 1.5), ((0, 1.5, 3), (0, 1, 0), (1, 0, 0), 1.5, 2.0)]
    meshes = [quad(*w) for w in walls]
    instances = [(k + 1, IDENT, 1 + k % 3) for k in range(6)]
    return {"name": "box", "meshes": meshes, "instances": instances, "materials": MATERIALS, "images": images(),
            "lights": [rect_light((0.0, 2.9, 2.0), (1, 0, 0), (0, 0, 1), 0.8, 0.5, 8.0)], "probe": PROBE, "camera": {"origin": (0.0, 1.4, 1.0), "direction": (0.0, -0.3, -1.0)}}


def render(device, scene, probe, camera, size, spp=SPP, depth=DEPTH, options=PER_BOUNCE, noise=None, env=False, sampling=None):
    """one raytrace_n of an lp.Scene -> (radiance, {stage: launches}, (closest, shadow, shaded))"""
    sg = lp.SceneGPU.new_from_scene(scene, device)
    pr = lp.ProbeGPU(device, probe, probe.shape[1], probe.shape[0])
    r = lp.Renderer(device, size)
    r.downsample_factor = 1.0
    if noise is not None:
        r.upload_noise_texture(noise, noise.shape[1], noise.shape[0], noise.shape[1] * 4)
        r.use_noise_texture(True)
    r.resize(device, sg, pr, size)
    r.set_max_bounces(depth)
    r.set_vfov(T.VFOV)
    for k, v in options.items():
        r.set_option(k, v)
    if env:
        r.set_env_sampling(True)
    if sampling is not None:
        r.set_emissive_sampling(sampling)
    r.enable_timings(True)
    r.reset_accumulation()
    r.accumulate = True
    r.reset_ray_counts()
    r.raytrace_n(T.look(camera["origin"], camera["direction"]), spp)
    img, c = r.read_radiance(), r.ray_counts()
    launches = {k: v[1] for k, v in r.timings().items()}
    r.close(); pr.close(); sg.close()
    return img, {k: launches[k] for k in STAGES}, (c.closest, c.shadow, c.shaded)


@functools.lru_cache(maxsize=None)
def oracle(name, size, spp=SPP, depth=DEPTH, noise=False):
    """the oracle's frame and counters of a description, rendered once per (scene, size) and shared by the tests that compare with it"""
    from oracle import orc
    desc = {"board": board, "board6": lambda: board(lights=6), "box": box}[name]()
    osc = orc.OracleScene.from_scene(harness.to_oracle(desc), probe=desc["probe"], noise=NOISE if noise else None)
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    acc, oc = osc.render(size[0], size[1], view, T.VFOV, depth, frames=spp, use_noise=noise, want_counters=True)
    return orc.resolve(acc).tobytes(), (oc.closest, oc.shadow, oc.shaded)


def test_the_primary_waves_of_the_board_hold_every_kind_of_hit(device):
    """what the other tests lean on: in the 64 x 36 frame most 8 x 8 pixel blocks — a wave of the primary hits — hold surface hits beside misses, and some an emitter hit too"""
    desc = board()
    sg = lp.SceneGPU.new_from_scene(scenes.to_product(desc), device)
    w, h = SMALL
    o, d = E.camera_rays(T.look(CAMERA["origin"], CAMERA["direction"]), T.VFOV, w, h, 0, 1)      # the first frame's primary rays (user seed 0)
    d = np.ascontiguousarray(d, np.float32)
    prim = sg.trace_closest(np.ascontiguousarray(np.broadcast_to(o.astype(np.float32), d.shape)), d)["prim"].reshape(h, w)
    sg.close()
    miss, emit = prim == 0xFFFFFFFF, (prim != 0xFFFFFFFF) & ((prim & 0x80000000) != 0)
    surf = ~miss & ~emit
    blocks = [(slice(by, by + 8), slice(bx, bx + 8)) for by in range(0, h - 7, 8) for bx in range(0, w, 8)]
    mixed = sum(1 for b in blocks if surf[b].any() and miss[b].any())
    three = sum(1 for b in blocks if surf[b].any() and miss[b].any() and emit[b].any())
    print("blocks %d: surface beside miss %d, all three kinds %d; pixels: %d surface, %d miss, %d emitter" % (len(blocks), mixed, three, surf.sum(), miss.sum(), emit.sum()))
    assert mixed >= len(blocks) // 2 and three >= 1


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
def test_the_small_board_equals_the_oracle(device, noise):
    """64 x 36, 2 spp, depth 4, the per-bounce launches: k_shade<0> on waves of mixed kinds; with the noise texture on, its texel comes with the record"""
    ref, oc = oracle("board", SMALL, noise=noise)
    img, launches, counts = render(device, scenes.to_product(board()), PROBE, CAMERA, SMALL, noise=NOISE if noise else None)
    assert launches["shading"] == DEPTH and launches["path"] == 0, launches
    print("closest %d shadow %d shaded %d" % counts)
    assert counts == oc
    assert img.tobytes() == ref


@pytest.mark.parametrize("options", [PER_BOUNCE, K_PATH, WAVE_PER_RAY], ids=["k_shade", "k_path", "wave_per_ray"])
def test_the_board_through_the_three_pipelines(device, options):
    """160 x 96: the per-bounce launches, k_path (which keeps shade_hit, every load in its branch) and a wave per ray give the oracle's bytes — so all three the same"""
    ref, oc = oracle("board", MID)
    img, launches, counts = render(device, scenes.to_product(board()), PROBE, CAMERA, MID, options=options)
    if options is PER_BOUNCE:
        assert launches["shading"] == DEPTH and launches["path"] == 0, launches
    if options is K_PATH:
        assert launches["path"] == 1 and launches["shading"] == 0, launches
    assert counts == oc
    assert img.tobytes() == ref


def test_more_lights_than_the_table_holds(device):
    """six rectangle lights, kLightTable = 4: next-event estimation that draws light 4 or 5, and an emitter hit on one of them, read the rows from memory"""
    ref, oc = oracle("board6", SMALL)
    img, launches, counts = render(device, scenes.to_product(board(lights=6)), PROBE, CAMERA, SMALL)
    assert launches["shading"] == DEPTH and launches["path"] == 0, launches
    assert counts == oc
    assert img.tobytes() == ref
    assert img.tobytes() != oracle("board", SMALL)[0]        # the further lights do light the board


def test_a_frame_without_a_miss_or_an_emitter_hit(device):
    """the closed box at depth 1: every primary ray finds a wall, the light is behind the camera, and only shadow rays follow — no wave enters a miss or an emitter branch"""
    ref, oc = oracle("box", SMALL, depth=1)
    img, launches, counts = render(device, scenes.to_product(box()), PROBE, box()["camera"], SMALL, depth=1)
    assert launches["shading"] == 1 and launches["path"] == 0, launches
    n = SMALL[0] * SMALL[1] * SPP
    assert counts[0] == n and counts[2] == n and 0 < counts[1] <= n, counts       # every ray a surface hit; no ray but the primary and the shadow rays
    assert counts == oc
    assert img.tobytes() == ref


# ---------------------------------------------------------------- the feature forms: the board, one feature at a time
def _with(extra):
    def make():
        s = scenes.to_product(board())
        extra(s)
        return s
    return make


def _punct(s):
    s.add_punctual_light(lp.point_light((-1.0, 1.2, -1.0), (1.0, 0.9, 0.8), 4.0))


def _lamp(s):
    m = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(m, (1.0, 0.8, 0.6), 5.0)
    q = quad((1.5, 0.8, -1.0), (1, 0, 0), (0, 0, 1), 0.4, 0.4)      # (1, 0, 0) x (0, 0, 1) = (0, -1, 0): facing the board
    s.add_instance(s.add_mesh(q["positions"], q["normals"], q["uvs"], q["indices"]), IDENT, m)


def _pane(s):
    m = s.add_material((0.6, 1.0, 0.4, 1.0), 0.2, 0.0)
    s.set_material_transmission(m, 0.7, 1.5, True)
    q = quad((0.0, 0.9, 0.5), (1, 0, 0), (0, 0.8, -0.6), 0.9, 0.6)
    s.add_instance(s.add_mesh(q["positions"], q["normals"], q["uvs"], q["indices"]), IDENT, m)


def _bumpy(s):
    m = s.add_material((0.7, 0.7, 0.8, 1.0), 0.4, 0.0)
    s.set_material_normal_map(m, s.add_image(np.random.RandomState(31).randint(0, 256, (4, 4, 4)).astype(np.uint8)), 1.5)
    q = quad((-1.0, 0.3, 0.2), (0, 0, 1), (1, 0, 0), 0.6, 0.6)
    s.add_instance(s.add_mesh(q["positions"], q["normals"], q["uvs"], q["indices"]), IDENT, m)


# form -> (scene, what else the renderer gets)
FEATURES = {
    "env": (_with(lambda s: None), dict(env=True)),
    "punct": (_with(_punct), {}),
    "emis_esamp": (_with(_lamp), dict(sampling=True)),
    "trans": (_with(_pane), {}),
    "nmap": (_with(_bumpy), {}),
}


def render_feature(device, case):
    scene, extra = FEATURES[case]
    return render(device, scene(), PROBE, CAMERA, SMALL, **extra)


def digest(img):
    return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()


@pytest.mark.parametrize("case", list(FEATURES))
def test_a_feature_form_gives_the_frame_it_gave_before(device, case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    img, launches, counts = render_feature(device, case)
    assert launches["shading"] == DEPTH and launches["path"] == 0, launches
    assert np.all(np.isfinite(img)) and img[..., :3].any()
    print("%s: %s closest, %s shadow, %s shaded; %s" % ((case,) + counts + (digest(img),)))
    assert list(counts) == want["counts"], (counts, want["counts"])
    with np.load(GOLDEN_FRAMES) as frames:
        ref = frames[case]
    assert digest(ref) == want["sha256"]      # the two golden files belong together
    bad = np.any(img.view(np.uint32) != ref.view(np.uint32), axis=-1)
    assert not bad.any(), "%d of %d pixels differ, first at (y, x) = %s, max |difference| %g" % (bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), np.abs(img - ref).max())
    assert digest(img) != hashlib.sha256(oracle("board", SMALL)[0]).hexdigest()      # the feature does change the board's frame
