"""-m gpu: the traversal step reports a ray's end in the step that uses up its last work (ray_step_pipe / ray_step_any, kernels.h), not at the top of the step
after it.  Three things are checked: the number of steps a ray takes where it can be derived by hand; that nothing else moves — frames, ray counts and the
node / triangle counters over every launch form —; and the two call sites that could have relied on "a finished ray costs one more step": the refill and the
step budget.

A STEP is a loop iteration of the traversal kernel in which the ray visits a node or tests a triangle.  The stats kernels count them per ray (the step
histogram: bucket k holds the rays of 2^k .. 2^(k+1) - 1 steps) and in total (`live_lanes`: every step of every ray is one live lane of one wave step), so
`live_lanes` is the sum of the rays' step counts, whatever the refill schedule was.

The constants under PARENT were recorded ONCE from the commit before this change (the same functions below, run against that commit's library) and are not
to be refreshed from the code under test."""
import hashlib
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A
from loupiote_amd import scenes, testing as T
from oracle import harness

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# the per-bounce launches with a lane per ray and nothing that takes rays away from them: no path kernel, no wave per ray, no tail in place, no budget, no packets
PER_LANE = {"path_rays": 0, "coop_rays": 0, "tail_lanes": 0, "step_budget": 0, "packet_primary": 0}
TWO_TRIP = dict(PER_LANE, pipe_rays=0)      # the two-round-trip step (ray_step_any)


def _dark():
    l = np.zeros(1, A.LIGHT_DT)
    l["normal"], l["tangent"], l["bitangent"], l["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.1), (0, 0, 1, 0.1), (0, -50.0, 0, 0.0)
    return l


def _run(device, scene, size, depth, samples, options, eye, direction, probe=None, stats=False, glass=False):
    """one wavefront of `samples` samples; -> (frame, ray counts, longest ray in steps, step histogram)"""
    sg = lp.SceneGPU.new_from_scene(scene, device)
    pr = lp.ProbeGPU(device, probe, probe.shape[1], probe.shape[0]) if probe is not None else None
    r = lp.Renderer(device, size)
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, size)
    r.set_max_bounces(depth)
    r.set_vfov(T.VFOV)
    if glass:
        r.set_glass_shadows(True)
    for k, v in options.items():
        r.set_option(k, v)
    r.enable_stats(stats)
    r.reset_accumulation()
    r.accumulate = True
    r.reset_ray_counts()
    r.raytrace_n(T.look(eye, direction), samples)
    img, c = r.read_radiance(), r.ray_counts()
    mx, hist = r.step_histogram() if stats else (0, np.zeros(12, np.uint32))
    r.close()
    if pr is not None:
        pr.close()
    sg.close()
    return img, c, int(mx), hist.astype(np.int64)


# ---------------------------------------------------------------- 1. step counts that can be derived by hand
def one_triangle():
    """one triangle in the plane z = 0 that fills the view of a camera at (0, 0, 3) looking down -z (the view is 2.5 x 4.4 units there)"""
    pos = np.array([[-100, -100, 0], [100, -100, 0], [0, 100, 0]], np.float32)
    s = lp.Scene()
    s.set_light(0, _dark())
    m = scenes._mesh(pos, np.arange(3, dtype=np.uint32))
    blas = s.add_mesh(m["positions"], m["normals"], m["uvs"], m["indices"])
    s.add_instance(blas, np.eye(4, dtype=np.float32), s.add_material((0.8, 0.8, 0.8, 1.0), 0.7, 0.0))
    return s


@pytest.mark.parametrize("options", [PER_LANE, TWO_TRIP], ids=["one_trip", "two_trip"])
def test_a_ray_that_misses_the_roots_children_takes_one_step(device, options):
    """the camera turned away from the only triangle: a ray visits the root, no child box is met, nothing is left — 1 step (the parent commit: 2, the second an empty one)"""
    img, c, mx, hist = _run(device, one_triangle(), (64, 36), 1, 1, options, (0.0, 0.0, 3.0), (0.0, 0.0, 1.0), stats=True)
    print("away:", dict(closest=c.closest, shadow=c.shadow, nodes=c.nodes, tris=c.tris, live=c.live_lanes, mx=mx, hist=hist.tolist()))
    assert (c.closest, c.shadow) == (64 * 36, 0)
    assert (c.nodes, c.tris) == (64 * 36, 0)                     # the root and nothing else
    assert mx == 1
    assert hist.tolist() == [64 * 36] + [0] * 11
    assert c.live_lanes == 64 * 36


def test_root_then_triangle_is_two_steps_with_one_round_trip_per_step(device):
    """the camera on the triangle: every camera ray meets the triangle's box — the root's visit, then, a step later (ray_step_pipe tests in a step what an earlier
    step found), the triangle: 2 steps (the parent commit: 3).  A shadow ray visits the root and tests the triangle or not: 1 or 2."""
    img, c, mx, hist = _run(device, one_triangle(), (64, 36), 1, 1, PER_LANE, (0.0, 0.0, 3.0), (0.0, 0.0, -1.0), stats=True)
    print("on, one trip:", dict(closest=c.closest, shadow=c.shadow, nodes=c.nodes, tris=c.tris, snodes=c.shadow_nodes, stris=c.shadow_tris, live=c.live_lanes, mx=mx, hist=hist.tolist()))
    assert c.closest == 64 * 36 and (c.nodes, c.tris) == (64 * 36, 64 * 36)
    assert mx == 2
    assert int(hist.sum()) == c.closest + c.shadow and int(hist[2:].sum()) == 0
    assert hist[1] >= c.closest                                   # bucket 1: 2 or 3 steps, and the longest ray took 2
    assert c.live_lanes == 2 * c.closest + c.shadow_nodes + c.shadow_tris    # a shadow ray: one step per root visit, one per triangle test


def test_root_then_triangle_is_one_step_with_two_round_trips_per_step(device):
    """the same frame under pipe_rays = 0: ray_step_any tests the triangle in the step that found it — the root's visit and the triangle test are ONE step,
    for camera rays and shadow rays alike (the parent commit: 2)"""
    img, c, mx, hist = _run(device, one_triangle(), (64, 36), 1, 1, TWO_TRIP, (0.0, 0.0, 3.0), (0.0, 0.0, -1.0), stats=True)
    print("on, two trips:", dict(closest=c.closest, shadow=c.shadow, nodes=c.nodes, tris=c.tris, snodes=c.shadow_nodes, stris=c.shadow_tris, live=c.live_lanes, mx=mx, hist=hist.tolist()))
    assert c.closest == 64 * 36 and (c.nodes, c.tris) == (64 * 36, 64 * 36)
    assert mx == 1
    assert hist.tolist() == [c.closest + c.shadow] + [0] * 11
    assert c.live_lanes == c.closest + c.shadow


def occluder_scene():
    """an 8 x 8 floor at y = 0, a 2 x 2 occluder one unit above it, a rectangle light at y = 3 facing down: floor points under the occluder have occluded shadow rays"""
    def quad(o, eu, ev):
        o, eu, ev = (np.asarray(x, np.float32) for x in (o, eu, ev))
        return np.stack([o, o + eu, o + eu + ev, o, o + eu + ev, o + ev])
    s = lp.Scene()
    l = np.zeros(1, A.LIGHT_DT)
    l["normal"], l["tangent"], l["bitangent"], l["origin"] = (0, -1, 0, 0), (1, 0, 0, 0.5), (0, 0, 1, 0.5), (0.0, 3.0, 0.0, 10.0)
    s.set_light(0, l)
    for pos, color in ((quad((-4, 0, 4), (8, 0, 0), (0, 0, -8)), (0.8, 0.8, 0.8, 1.0)), (quad((-1, 1, 1), (2, 0, 0), (0, 0, -2)), (0.8, 0.3, 0.2, 1.0))):
        m = scenes._mesh(pos, np.arange(6, dtype=np.uint32))
        blas = s.add_mesh(m["positions"], m["normals"], m["uvs"], m["indices"])
        s.add_instance(blas, np.eye(4, dtype=np.float32), s.add_material(color, 0.8, 0.0))
    return s


def occluder_figures(device, options):
    img, c, mx, hist = _run(device, occluder_scene(), (64, 36), 1, 1, options, (0.0, 2.0, 5.0), (0.0, -0.4, -1.0), stats=True)
    return dict(closest=int(c.closest), shadow=int(c.shadow), occluded=int(c.shadow_occluded), live=int(c.live_lanes), mx=mx, hist=hist.tolist())


# recorded from the parent commit (occluder_figures above)
PARENT_OCCLUDER = {
    "one_trip": {'closest': 2304, 'shadow': 1556, 'occluded': 255, 'live': 13991, 'mx': 6, 'hist': [0, 908, 2952, 0, 0, 0, 0, 0, 0, 0, 0, 0]},
    "two_trip": {'closest': 2304, 'shadow': 1556, 'occluded': 255, 'live': 10875, 'mx': 5, 'hist': [0, 3713, 147, 0, 0, 0, 0, 0, 0, 0, 0, 0]},
}


@pytest.mark.parametrize("form", ["one_trip", "two_trip"])
def test_occluded_any_hit_rays_keep_their_step_count(device, form):
    """an any-hit ray that finds an occluder is reported by the step that accepts the hit, before and after: its count stays.  Every other ray — closest-hit rays,
    unoccluded shadow rays — loses exactly the one empty step.  So the sum of all step counts falls by the number of rays that are not occluded shadow rays."""
    got = occluder_figures(device, PER_LANE if form == "one_trip" else TWO_TRIP)
    was = PARENT_OCCLUDER[form]
    print("occluder", form, got)
    assert (got["closest"], got["shadow"], got["occluded"]) == (was["closest"], was["shadow"], was["occluded"])
    assert 0 < got["occluded"] < got["shadow"]
    assert got["live"] == was["live"] - (got["closest"] + got["shadow"] - got["occluded"])
    assert sum(got["hist"]) == got["closest"] + got["shadow"]


# ---------------------------------------------------------------- 2. nothing else moves
SIZE, DEPTH, SAMPLES = (160, 96), 6, 3
PER_BOUNCE = {"path_rays": 0, "coop_rays": 0, "tail_lanes": 0, "step_budget": 0}
# form -> (scene, options, do the stats kernels run the same form?  — the plan takes the tail in place away from them)
FORMS = {
    "one_trip":      ("cornell", PER_BOUNCE, True),
    "two_trip":      ("cornell", dict(PER_BOUNCE, pipe_rays=0), True),
    "tail":          ("cornell", dict(PER_BOUNCE, tail_lanes=4), False),
    "tail_two_trip": ("cornell", dict(PER_BOUNCE, tail_lanes=4, pipe_rays=0), False),
    "path":          ("cornell", {"path_rays": 0x7FFFFFFF, "coop_rays": 0}, True),
    "masked":        ("alpha-mask.glb", PER_BOUNCE, True),
    "glass":         ("glass-pane.glb", PER_BOUNCE, True),
}
CAMERAS = {"alpha-mask.glb": ((0.0, 0.9, 3.0), (0.0, -0.3, -1.0)), "glass-pane.glb": ((0.5, 1.2, 5.0), (0.0, -0.15, -1.0))}


def _form_scene(name, cornell_glb):
    s = lp.Scene()
    if name == "cornell":
        lp.loaders.load_gltf(cornell_glb, s)
        s.set_light(0, T.cornell_light())
        return s, T.CORNELL_PROBE, T.CORNELL_EYE, T.CORNELL_DIR
    with open(os.path.join(HERE, "golden", name), "rb") as f:
        lp.loaders.load_gltf(f.read(), s)
    s.set_light(0, _dark())
    return s, None, CAMERAS[name][0], CAMERAS[name][1]


def form_figures(device, cornell_glb, form):
    """-> (the shipped kernels' frame, figures): ray counts of the shipped kernels, and where the stats kernels run the same form, their frame's digest and their counters"""
    name, options, stats_too = FORMS[form]
    scene, probe, eye, direction = _form_scene(name, cornell_glb)
    glass = name == "glass-pane.glb"
    img, c, _, _ = _run(device, scene, SIZE, DEPTH, SAMPLES, options, eye, direction, probe=probe, glass=glass)
    fig = dict(sha=hashlib.sha256(img.tobytes()).hexdigest(), closest=int(c.closest), shadow=int(c.shadow), wave_rays=int(c.wave_rays))
    if stats_too:
        simg, sc, _, _ = _run(device, scene, SIZE, DEPTH, SAMPLES, options, eye, direction, probe=probe, stats=True, glass=glass)
        fig.update(stats_sha=hashlib.sha256(simg.tobytes()).hexdigest(), stats_closest=int(sc.closest), stats_shadow=int(sc.shadow),
                   nodes=int(sc.nodes), tris=int(sc.tris), shadow_nodes=int(sc.shadow_nodes), shadow_tris=int(sc.shadow_tris))
    return img, fig


# recorded from the parent commit (form_figures above; `sha`: SHA-256 of the frame's bytes)
PARENT_FORMS = {
    "one_trip": {'sha': 'f96df35ff37151a5211f69367f99dde907f772cbcdb7f40f61316ac954c2f30f',
                 'closest': 95897,
                 'shadow': 40780,
                 'nodes': 124692,
                 'tris': 257776,
                 'shadow_nodes': 54760,
                 'shadow_tris': 87575},
    "two_trip": {'sha': 'f96df35ff37151a5211f69367f99dde907f772cbcdb7f40f61316ac954c2f30f',
                 'closest': 95897,
                 'shadow': 40780,
                 'nodes': 124692,
                 'tris': 256128,
                 'shadow_nodes': 54760,
                 'shadow_tris': 87575},
    "tail": {'sha': 'f96df35ff37151a5211f69367f99dde907f772cbcdb7f40f61316ac954c2f30f', 'closest': 95897, 'shadow': 40780},
    "tail_two_trip": {'sha': 'f96df35ff37151a5211f69367f99dde907f772cbcdb7f40f61316ac954c2f30f', 'closest': 95897, 'shadow': 40780},
    "path": {'sha': 'f96df35ff37151a5211f69367f99dde907f772cbcdb7f40f61316ac954c2f30f',
             'closest': 95897,
             'shadow': 40780,
             'nodes': 124692,
             'tris': 262480,
             'shadow_nodes': 54760,
             'shadow_tris': 82871},
    "masked": {'sha': 'a9e650a3783c394bb5bb27bda10e68b7aaaab78f33c91c4642c63b5880e11927',
               'closest': 79803,
               'shadow': 17364,
               'nodes': 79803,
               'tris': 145532,
               'shadow_nodes': 17364,
               'shadow_tris': 41196},
    "glass": {'sha': 'ed06888ca31f1154b3b55e4cb3fe29f593a1c1dfead6222f0b62e4311cc19370',
              'closest': 83051,
              'shadow': 11852,
              'nodes': 83051,
              'tris': 164936,
              'shadow_nodes': 11852,
              'shadow_tris': 24548},
}


@pytest.fixture(scope="module")
def cornell_oracle(cornell_glb):
    ref, oc = harness.render_oracle(cornell_glb, SIZE[0], SIZE[1], DEPTH, SAMPLES)
    return ref, (oc.closest, oc.shadow)


@pytest.mark.parametrize("form", list(FORMS))
def test_frames_and_counters_are_the_parents_over_the_launch_forms(device, cornell_glb, cornell_oracle, form):
    """the Cornell frame over the one- and two-round-trip step, the tail in place on and off and the path kernel: byte-identical to the oracle's; a masked and a
    glass-shadow scene (the oracle knows neither: the parent's frame by its digest); closest, shadow, nodes, tris, shadow_nodes, shadow_tris as recorded"""
    img, fig = form_figures(device, cornell_glb, form)
    was = PARENT_FORMS[form]
    print("form", form, fig)
    if FORMS[form][0] == "cornell":
        ref, counts = cornell_oracle
        assert img.tobytes() == ref.tobytes()
        assert (fig["closest"], fig["shadow"]) == counts
    assert fig["sha"] == was["sha"]
    if "stats_sha" in fig:
        assert fig["stats_sha"] == was["sha"]
        assert (fig["stats_closest"], fig["stats_shadow"]) == (was["closest"], was["shadow"])
    if form == "path":
        # THE ONE PAIR THAT IS NOT THE PARENT'S.  k_path books a step's triangle test to the kind of ray its lane carries, and the parent asked that AFTER the step: an
        # occluded shadow ray's accepting test went to the path's next closest-hit ray where the path had one (4704 tests here).  The kernel now asks before the step —
        # it had to: every ray's last step is a working one now — and the split is the per-bounce launches' (the same rays through the same step); the sums are the parent's.
        assert (was["tris"], was["shadow_tris"]) == (262480, 82871) and was["tris"] + was["shadow_tris"] == fig["tris"] + fig["shadow_tris"]
        was = dict(was, tris=PARENT_FORMS["one_trip"]["tris"], shadow_tris=PARENT_FORMS["one_trip"]["shadow_tris"])
    for k in ("closest", "shadow", "nodes", "tris", "shadow_nodes", "shadow_tris"):
        if k in was:
            assert fig[k] == was[k], k
    if form.startswith("tail"):
        assert fig["wave_rays"] > 0          # waves did finish their last rays cooperatively: the form ran


# ---------------------------------------------------------------- 3. the refill
SMALL = (64, 36)
REFILLS = [0, 1, 43, 44, 63]


def refill_figures(device, cornell_glb, refill):
    scene, probe, eye, direction = _form_scene("cornell", cornell_glb)
    options = dict(PER_BOUNCE, refill=refill)
    img, c, _, _ = _run(device, scene, SMALL, DEPTH, SAMPLES, options, eye, direction, probe=probe)
    simg, sc, _, hist = _run(device, scene, SMALL, DEPTH, SAMPLES, options, eye, direction, probe=probe, stats=True)
    rays = int(sc.closest + sc.shadow - sc.primary)
    return img, simg, dict(rays=rays, live=int(sc.live_lanes), node=int(sc.node_lanes), hist_total=int(hist.sum()))


@pytest.fixture(scope="module")
def small_oracle(cornell_glb):
    ref, oc = harness.render_oracle(cornell_glb, SMALL[0], SMALL[1], DEPTH, SAMPLES)
    return ref, (oc.closest, oc.shadow)


# recorded from the parent commit (refill_figures above): live lanes that visit no node, summed over the launches' wave steps, and the rays they carried.  Both are sums
# over rays of what the ray's own steps do, so they do not depend on the threshold (the parent gives the same figures at all five)
PARENT_IDLE_LANES, PARENT_RAYS = 88804 - 25784, 19680


@pytest.mark.parametrize("refill", REFILLS)
def test_refill_thresholds_keep_the_frame_and_lose_the_empty_step(device, cornell_glb, small_oracle, refill):
    """refill only an empty wave, at one lane, just under and at the default, whenever a lane is free: the frame is the oracle's; the live lanes that visit no node, per
    ray, are fewer than before — the empty step is gone"""
    ref, counts = small_oracle
    img, simg, fig = refill_figures(device, cornell_glb, refill)
    print("refill", refill, fig, "idle lanes per ray %.4f (parent %.4f)" % ((fig["live"] - fig["node"]) / fig["rays"], PARENT_IDLE_LANES / PARENT_RAYS))
    assert img.tobytes() == ref.tobytes() and simg.tobytes() == ref.tobytes()
    assert fig["rays"] == PARENT_RAYS == counts[0] + counts[1] and fig["hist_total"] == fig["rays"]
    assert (fig["live"] - fig["node"]) / fig["rays"] < PARENT_IDLE_LANES / PARENT_RAYS


# ---------------------------------------------------------------- 4. the step budget
def test_step_budget_drops_only_unfinished_rays_and_every_ray_is_accounted_for(device, cornell_glb, small_oracle):
    """step_budget = 16: a ray still unfinished after 16 steps is dropped and traced again by a whole wave (k_trace_coop); the frame is unchanged.  A ray whose 16th
    step uses up its last work is finished by that step and is NOT dropped (the drop asks `active`, which the step has just cleared).  The launch plan keeps the
    budget away from the stats kernels (a dropped ray would be missing from their histogram), so the account is made over two runs of the same frame, a ray's step
    count being a function of the ray alone: the stats run's histogram holds every ray carried, and the stragglers of the budgeted run are the rays of more than 16
    steps — between the histogram's rays of 32 steps and more and its rays of 16 and more (bucket 4 holds 16..31)."""
    ref, counts = small_oracle
    scene, probe, eye, direction = _form_scene("cornell", cornell_glb)
    options = dict(PER_BOUNCE, step_budget=16)
    img, c, _, _ = _run(device, scene, SMALL, DEPTH, SAMPLES, options, eye, direction, probe=probe)
    simg, sc, mx, hist = _run(device, scene, SMALL, DEPTH, SAMPLES, options, eye, direction, probe=probe, stats=True)
    carried = int(c.closest + c.shadow - c.primary)
    print("budget 16:", dict(carried=carried, stragglers=int(c.wave_rays), mx=mx, hist=hist.tolist()))
    assert img.tobytes() == ref.tobytes() and simg.tobytes() == ref.tobytes()
    assert (c.closest, c.shadow) == counts == (sc.closest, sc.shadow)
    assert int(hist.sum()) == carried and sc.wave_rays == 0
    assert mx > 16 and 0 < c.wave_rays
    assert int(hist[5:].sum()) <= c.wave_rays <= int(hist[4:].sum())
    finished_in_lane = carried - int(c.wave_rays)
    assert int(hist[:4].sum()) <= finished_in_lane <= int(hist[:5].sum())     # ... and everything else was finished by its lane: the two parts make up the rays carried
