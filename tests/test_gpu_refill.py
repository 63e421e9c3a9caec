"""-m gpu: the refill of k_trace's per-lane throughput variant (k_trace<false, true, false>: the bench's launches) — where finished rays write their hit records
(after the emitter test, whose first kLightTable records come from LDS) or deposit their light sample, and new rays start.  The variant keeps a hit's leaf place
during the traversal and looks its primitive id up only at an exact tie and at the finish (ray_step_pipe<.., PLACE>).  None of it may change a frame: every test
compares with the oracle bit for bit, over thresholds from "refill only an empty wave" to "refill whenever a lane is free"."""
import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T
from oracle import harness

pytestmark = pytest.mark.gpu

# k_trace<false, true, false>: the per-bounce launches, one-round-trip step, no cooperative tail, no step budget, no wave-per-ray rule for tiny frames
PER_BOUNCE = {"path_rays": 0, "coop_rays": 0, "tail_lanes": 0, "step_budget": 0}
REFILLS = [0, 8, 44, None, 63]   # None: the library's default threshold


def _light(origin, normal, tangent, bitangent, half_w, half_h, radiance):
    l = np.zeros(1, dtype=[("normal", "<f4", 4), ("tangent", "<f4", 4), ("bitangent", "<f4", 4), ("origin", "<f4", 4)])
    l["normal"] = tuple(normal) + (0.0,)
    l["tangent"] = tuple(tangent) + (half_w,)
    l["bitangent"] = tuple(bitangent) + (half_h,)
    l["origin"] = tuple(origin) + (radiance,)
    return l


def tie_room(n_lights=6, copies=3):
    """A closed room, a quad `copies` times in the same place as separate instances with different materials (coincident triangles, hit at identical t: the
    lowest primitive id must win, and a wrong pick shows as a different colour), and `n_lights` emitters on the back wall in the camera's view."""
    def soup(tris):
        pos = np.asarray(tris, np.float32).reshape(-1, 3)
        return scenes._mesh(pos, np.arange(pos.shape[0], dtype=np.uint32))
    def quad(o, eu, ev):
        o, eu, ev = (np.asarray(x, np.float32) for x in (o, eu, ev))
        return [[o, o + eu, o + eu + ev], [o, o + eu + ev, o + ev]]
    H = 4.0
    walls = (quad((-H, 0, -H), (0, 0, 2 * H), (2 * H, 0, 0)) + quad((-H, 0, -H), (2 * H, 0, 0), (0, 6, 0)) + quad((H, 0, H), (-2 * H, 0, 0), (0, 6, 0))
             + quad((-H, 0, H), (0, 0, -2 * H), (0, 6, 0)) + quad((H, 0, -H), (0, 0, 2 * H), (0, 6, 0)) + quad((-H, 6, -H), (2 * H, 0, 0), (0, 0, 2 * H)))
    panel = quad((-1.5, 0.6, -1.0), (3.0, 0, 0.2), (0, 1.8, -0.3))
    meshes = [soup(walls), soup(panel)]
    INV = scenes.INVALID
    materials = [((0.7, 0.7, 0.68, 1), 0.8, 0.0, INV, INV), ((0.9, 0.2, 0.15, 1), 0.3, 0.0, INV, INV), ((0.15, 0.85, 0.2, 1), 0.6, 0.0, INV, INV),
                 ((0.2, 0.3, 0.9, 1), 0.1, 1.0, INV, INV)]
    ident = scenes._translate(0, 0, 0)
    instances = [(1, ident, 0)] + [(2, ident, 1 + (k % 3)) for k in range(copies)]
    lights = [_light((-3.0 + 6.0 * k / max(n_lights - 1, 1), 3.6, -3.95), (0, 0, 1), (1, 0, 0), (0, 1, 0), 0.35, 0.25, 12.0 + k) for k in range(n_lights)]
    return {"name": "tie_room", "meshes": meshes, "instances": instances, "materials": materials, "images": [], "lights": lights,
            "probe": scenes.sky_probe(64, 32), "camera": {"origin": (0.3, 2.2, 3.6), "direction": (-0.05, 0.08, -1.0)}}


def _render(device, desc, size, depth, frames, options, stats=False):
    sg = lp.SceneGPU.new_from_scene(scenes.to_product(desc), device)
    pr = lp.ProbeGPU(device, desc["probe"], desc["probe"].shape[1], desc["probe"].shape[0])
    r = lp.Renderer(device, size)
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, size)
    r.set_max_bounces(depth)
    r.set_vfov(T.VFOV)
    for k, v in options.items():
        r.set_option(k, v)
    if stats:
        r.enable_stats(True)
    r.reset_accumulation()
    r.accumulate = True
    r.reset_ray_counts()
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    for _ in range(frames):
        r.raytrace(view)
    img, c = r.read_radiance(), r.ray_counts()
    r.close(); pr.close(); sg.close()
    return img, (c.closest, c.shadow, c.shaded)


def _options(base, refill):
    o = dict(base)
    if refill is not None:
        o["refill"] = refill
    return o


@pytest.fixture(scope="module")
def room():
    from oracle import orc
    desc = tie_room()
    return desc, orc.OracleScene.from_scene(harness.to_oracle(desc), probe=desc["probe"])


def _oracle(osc, desc, size, depth, frames):
    from oracle import orc
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    acc, oc = osc.render(size[0], size[1], view, T.VFOV, depth, frames=frames, want_counters=True)
    return orc.resolve(acc), (oc.closest, oc.shadow, oc.shaded)


@pytest.mark.parametrize("refill", REFILLS)
@pytest.mark.parametrize("base", [PER_BOUNCE, {}], ids=["per_bounce", "default"])
def test_cornell_at_every_refill_threshold_equals_the_oracle(device, cornell_glb, base, refill):
    """the Cornell box: the ceiling emitter is in the camera's view, so closest-hit rays end on it (the emitter test at the finish)"""
    size, depth, frames = (128, 96), 5, 2
    ref, oc = harness.render_oracle(cornell_glb, size[0], size[1], depth, frames)
    img, counts = T.render_hip(device, cornell_glb, size[0], size[1], depth, frames, options=_options(base, refill))
    assert (counts.closest, counts.shadow) == (oc.closest, oc.shadow)
    assert img.tobytes() == ref.tobytes()


@pytest.mark.parametrize("refill", REFILLS)
@pytest.mark.parametrize("base", [PER_BOUNCE, {}], ids=["per_bounce", "default"])
def test_coincident_triangles_and_many_emitters_equal_the_oracle(device, room, base, refill):
    """exact ties between coincident triangles of different primitive ids go to the lowest id, as in the oracle; six emitters in view"""
    desc, osc = room
    size, depth, frames = (160, 96), 6, 2
    ref, oc = _oracle(osc, desc, size, depth, frames)
    img, counts = _render(device, desc, size, depth, frames, _options(base, refill))
    assert counts == oc
    assert img.tobytes() == ref.tobytes()


@pytest.mark.parametrize("n_lights", [1, 4, 5])
def test_emitter_table_sizes_equal_the_oracle(device, n_lights):
    """emitters hit by closest-hit rays with all records in the LDS table, the table exactly full, and one record behind it"""
    from oracle import orc
    desc = tie_room(n_lights=n_lights, copies=2)
    osc = orc.OracleScene.from_scene(harness.to_oracle(desc), probe=desc["probe"])
    size, depth, frames = (96, 64), 4, 1
    ref, oc = _oracle(osc, desc, size, depth, frames)
    img, counts = _render(device, desc, size, depth, frames, PER_BOUNCE)
    assert counts == oc
    assert img.tobytes() == ref.tobytes()


def test_stats_twin_equals_the_oracle(device, room):
    """k_trace<true, true, false> (the stats kernels bench.py runs for its roofline) gives the same frame"""
    desc, osc = room
    size, depth, frames = (128, 80), 5, 1
    ref, oc = _oracle(osc, desc, size, depth, frames)
    img, counts = _render(device, desc, size, depth, frames, PER_BOUNCE, stats=True)
    assert counts == oc
    assert img.tobytes() == ref.tobytes()
