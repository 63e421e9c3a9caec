"""-m gpu: the pieces of a cut batch under every lane schedule (LPT_EXP_LANE_PHASE: free, offset start, alternating traversal) and
with one and two lanes.  The bench-shaped frame (the Sponza stand-in, 4 samples, depth 8) at a reduced size, cut into two pieces
by LPT_OPT_WAVEFRONT_RAYS: the order of the launches across the lanes must not change a single byte of the radiance.  And the Cornell box cut
into five pieces on two and three lanes: a submission that reuses its tickets, lanes and traversal events and ends in a group that is not full."""
import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import scenes, testing as T

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 480, 272, 4, 8
# slots per tile row (32x8 tiles) x samples: 17 of the 34 tile rows fit one wavefront, so the frame leaves as two pieces
CUT_RAYS = 17 * (W // 32) * 256 * SPP + 1000


@pytest.fixture(scope="module")
def atrium(device):
    desc = scenes.synthetic_atrium(texture_size=256)
    sg = lp.SceneGPU.new_from_scene(scenes.to_product(desc), device)
    probe = lp.ProbeGPU(device, desc["probe"], desc["probe"].shape[1], desc["probe"].shape[0])
    yield desc, sg, probe
    probe.close()
    sg.close()


def _frames(device, atrium, lanes, phase=None, max_fused=0):
    desc, sg, probe = atrium
    r = lp.Renderer(device, (W, H))
    r.downsample_factor = 1.0
    r.resize(device, sg, probe, (W, H))
    r.set_max_bounces(DEPTH)
    r.set_vfov(T.VFOV)
    r.set_lanes(lanes)
    r.set_max_fused(max_fused)
    r.set_option("wavefront_rays", CUT_RAYS)
    if phase is not None:
        r.set_option("lane_phase", phase)
    views = [T.look(desc["camera"]["origin"], desc["camera"]["direction"]), T.look((0.4, 1.1, 6.0), (-0.1, -0.05, -1.0))]
    out = []
    for view in views:
        r.reset_accumulation()
        r.accumulate = True
        _, wf0, _ = r.submission_stats()
        for _ in range(SPP):
            r.raytrace(view)
        img = r.read_radiance().copy()
        _, wf1, _ = r.submission_stats()
        c = r.ray_counts()
        out.append((img, wf1 - wf0, (c.closest, c.shadow, c.shaded)))
    r.close()
    return out


CW, CH, CDEPTH = 96, 72, 4
# three 32x8 tiles per row x 4 samples = 3072 rays a tile row: two fit, so the nine tile rows leave as five pieces of 2, 2, 2, 2 and 1 —
# with two or three lanes a submission reuses its tickets, lanes and traversal events, and its last group has one or two members
CORNELL_CUT_RAYS = 2 * (CW // 32) * 256 * SPP


@pytest.fixture(scope="module")
def cornell(device, cornell_glb):
    scene = lp.Scene()
    lp.loaders.load_gltf(cornell_glb, scene)
    scene.set_light(0, T.cornell_light())
    sg = lp.SceneGPU.new_from_scene(scene, device)
    probe = lp.ProbeGPU(device, T.CORNELL_PROBE, 1, 1)
    yield sg, probe
    probe.close()
    sg.close()


def _cornell_frames(device, sg, probe, lanes, phase=None, max_fused=0, options=None):
    r = lp.Renderer(device, (CW, CH))
    r.downsample_factor = 1.0
    r.resize(device, sg, probe, (CW, CH))
    r.set_max_bounces(CDEPTH)
    r.set_vfov(T.VFOV)
    r.set_lanes(lanes)
    r.set_max_fused(max_fused)
    r.set_option("wavefront_rays", CORNELL_CUT_RAYS)
    if phase is not None:
        r.set_option("lane_phase", phase)
    for name, value in (options or {}).items():
        r.set_option(name, value)
    out = []
    for view in (T.look(T.CORNELL_EYE, T.CORNELL_DIR), T.look((0.5, 0.4, 12.0), (-0.05, 0.02, -1.0))):   # five pieces each: the second submission starts from an odd lane counter
        r.reset_accumulation()
        r.accumulate = True
        _, wf0, _ = r.submission_stats()
        for _ in range(SPP):
            r.raytrace(view)
        img = r.read_radiance().copy()
        _, wf1, _ = r.submission_stats()
        c = r.ray_counts()
        out.append((img, wf1 - wf0, (c.closest, c.shadow, c.shaded)))
    r.close()
    return out


@pytest.mark.parametrize("options", [None, {"coop_rays": 0, "path_rays": 0}], ids=["defaults", "per_bounce"])
def test_five_pieces_reuse_lanes_tickets_and_events_and_give_the_same_frame(device, cornell, options):
    """per_bounce: the k_shade + k_trace stages run, so the hooks of the stages behind the primary rays order real launches"""
    sg, probe = cornell
    assert CORNELL_CUT_RAYS == 6144
    ref = _cornell_frames(device, sg, probe, lanes=1, max_fused=SPP, options=options)   # one wavefront per frame
    assert all(n == 1 for _, n, _ in ref)
    for lanes in (2, 3):
        for phase in (0, 1, 2):
            got = _cornell_frames(device, sg, probe, lanes, phase, options=options)
            for (img, n, counts), (ref_img, _, ref_counts) in zip(got, ref):
                assert n == 5, (lanes, phase, n)
                assert np.all(np.isfinite(img)) and float(img[..., :3].mean()) > 0.0
                assert img.tobytes() == ref_img.tobytes(), (lanes, phase)
                assert counts == ref_counts, (lanes, phase)


def test_lane_phase_option_round_trip(device):
    r = lp.Renderer(device, (64, 64))
    assert r.get_option("lane_phase") == 1      # offset start: the default
    for v in (0, 2, 1):
        r.set_option("lane_phase", v)
        assert r.get_option("lane_phase") == v
    with pytest.raises(lp.Error, match="LPT_EXP_LANE_PHASE"):
        r.set_option("lane_phase", 3)
    r.close()


def test_every_lane_schedule_gives_the_same_frame(device, atrium):
    ref = _frames(device, atrium, lanes=1, max_fused=SPP)   # one wavefront per frame: nothing is cut, nothing overlaps
    assert all(n == 1 for _, n, _ in ref)
    for lanes in (1, 2):
        for phase in (None, 0, 1, 2):
            got = _frames(device, atrium, lanes, phase)
            for (img, n, counts), (ref_img, _, ref_counts) in zip(got, ref):
                assert n == 2, (lanes, phase, n)           # the batch left as two pieces
                assert np.all(np.isfinite(img)) and float(img[..., :3].mean()) > 0.0
                assert img.tobytes() == ref_img.tobytes(), (lanes, phase)
                assert counts == ref_counts, (lanes, phase)
