"""-m gpu: the launch selection (loupiote_amd/csrc/launch_plan.h) as seen from outside — the per-stage launch counts of one small wavefront (Renderer.timings())
under the options and scenes that switch it, each with the frame of the scene's default configuration bit for bit — and the option table: every option of
_abi.OPTIONS round-trips, clamps or rejects as lpt.h says.  tests/test_launch_plan.py checks the same rules on the CPU over the sizes no test frame reaches."""
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A, testing as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIZE, DEPTH = (64, 32), 3          # 2048 rays: inside the wave-per-ray range (coop_rays 32 000), 25 mrad per pixel (no packets unless forced)
MAX_RAYS = 0x7FFFFFFF
STAGES = ("ray generation", "primary intersection", "intersection", "shadow", "shading", "path", "accumulation", "asvgf")
CAMERAS = {"cornell-box.glb": (T.CORNELL_EYE, T.CORNELL_DIR), "alpha-mask.glb": ((0.0, 0.9, 3.0), (0.0, -0.3, -1.0)), "glass-pane.glb": ((0.5, 1.2, 5.0), (0.0, -0.15, -1.0))}


@pytest.fixture(scope="module")
def scenes(device):
    out = {}
    for name in CAMERAS:
        with open(os.path.join(HERE, "golden", name), "rb") as f:
            s = lp.Scene()
            lp.loaders.load_gltf(f.read(), s)
        s.set_light(0, T.cornell_light())
        out[name] = lp.SceneGPU.new_from_scene(s, device)
    pr = lp.ProbeGPU(device, T.CORNELL_PROBE, 1, 1)
    yield out, pr
    pr.close()
    for sg in out.values():
        sg.close()


def render(device, scenes, name, options=None, mode=None):
    """one raytrace() as one wavefront with the timings on: (radiance, {stage: launches})"""
    sgs, pr = scenes
    r = lp.Renderer(device, SIZE)
    r.downsample_factor = 1.0
    r.resize(device, sgs[name], pr, SIZE)
    r.set_max_bounces(DEPTH)
    r.set_vfov(T.VFOV)
    r.set_max_fused(1)
    for k, v in (options or {}).items():
        r.set_option(k, v)
    if mode is not None:
        r.set_blit_mode(mode)
    r.enable_timings(True)
    r.reset_accumulation()
    r.raytrace(T.look(*CAMERAS[name]))
    img = r.read_radiance()
    launches = {k: v[1] for k, v in r.timings().items()}
    r.close()
    print(name, options, mode, {k: launches[k] for k in STAGES})
    return img, launches


def expect(launches, **want):
    names = {"raygen": "ray generation", "primary": "primary intersection"}
    got = {k: launches[names.get(k, k)] for k in want}
    assert got == want, launches


PER_BOUNCE = dict(intersection=3, shadow=1, shading=3, path=0, primary=0)


def test_cornell_stage_launches_follow_the_options(device, scenes):
    ref, n = render(device, scenes, "cornell-box.glb")
    expect(n, raygen=1, accumulation=1, asvgf=0, **PER_BOUNCE)                  # shipped: a wave per ray, a pixel too wide for packets
    assert np.all(np.isfinite(ref)) and ref[..., :3].any()
    img, n = render(device, scenes, "cornell-box.glb", {"coop_rays": 0})
    expect(n, raygen=1, path=1, intersection=0, shading=0, shadow=0, primary=0, accumulation=1)
    assert img.tobytes() == ref.tobytes()
    img, n = render(device, scenes, "cornell-box.glb", {"coop_rays": 0, "packet_primary": 1})
    expect(n, raygen=1, primary=1, path=1, intersection=0, shading=0, shadow=0, accumulation=1)
    assert img.tobytes() == ref.tobytes()
    img, n = render(device, scenes, "cornell-box.glb", {"coop_rays": 0, "path_rays": 0, "packet_primary": 1})
    expect(n, raygen=1, primary=1, intersection=2, shadow=1, shading=3, path=0, accumulation=1)
    assert img.tobytes() == ref.tobytes()


@pytest.mark.parametrize("name,want", [("alpha-mask.glb", PER_BOUNCE),                                                      # SPEC §20: the per-lane launches alone
                                       ("glass-pane.glb", dict(primary=1, path=0, intersection=2, shadow=1, shading=3))])   # SPEC §21: packets, but no path kernel
def test_masked_and_transmissive_scenes_keep_their_launches(device, scenes, name, want):
    ref, _ = render(device, scenes, name)
    img, n = render(device, scenes, name, {"packet_primary": 1, "coop_rays": 0, "path_rays": MAX_RAYS})
    expect(n, raygen=1, accumulation=1, **want)
    assert img.tobytes() == ref.tobytes()


def test_a_denoising_mode_ends_in_the_filter(device, scenes):
    """Blit mode Denoised: the frame read back is the filter's, so it is compared with the same mode's frame from the per-lane launches"""
    ref, n = render(device, scenes, "cornell-box.glb", mode=lp.BlitMode.DenoisedPathrace)
    expect(n, raygen=1, asvgf=1, accumulation=0, **PER_BOUNCE)
    img, n = render(device, scenes, "cornell-box.glb", {"coop_rays": 0, "path_rays": 0}, mode=lp.BlitMode.DenoisedPathrace)
    expect(n, raygen=1, asvgf=1, accumulation=0, **PER_BOUNCE)
    assert img.tobytes() == ref.tobytes()


# option -> (lowest, highest, rejects outside); include/lpt.h
RANGES = {"packet_primary": (0, 2, True), "wavefront_rays": (64, 2**64 - 1, False), "path_rays": (0, MAX_RAYS, False), "coop_rays": (0, MAX_RAYS, False),
          "tail_lanes": (0, 8, False), "pipe_rays": (0, MAX_RAYS, False), "refill": (0, 63, True), "trace_waves_per_cu": (0, 32, True),
          "shade_blocks_per_cu": (0, 64, True), "path_waves_per_cu": (1, 32, True), "path_refill": (0, 63, True), "occ_cell_milli": (0, 1000000, False),
          "step_budget": (0, 1 << 20, False), "budget_rays": (0, MAX_RAYS, False), "packet_quads": (0, 1, False), "split_rays": (0, 2**64 - 1, False),
          "budget_split": (0, 1, False), "lane_phase": (0, 2, True)}


def test_every_option_round_trips_clamps_or_rejects(device):
    assert set(RANGES) == set(A.OPTIONS)
    r = lp.Renderer(device, SIZE)
    for name, (lo, hi, rejects) in RANGES.items():
        for v in {lo, hi, min(lo + 1, hi), min((lo + hi) // 2, 250)} | ({250} if lo <= 250 <= hi else set()):
            r.set_option(name, v)
            assert r.get_option(name) == v, (name, v)
        kept = r.get_option(name)
        for bad in ([lo - 1] if lo > 0 else []) + ([hi + 1, 2**63] if hi < 2**63 else []):
            if rejects:
                with pytest.raises(lp.Error) as e:
                    r.set_option(name, bad)
                assert e.value.status == A.LPT_ERR_INVALID_ARG and r.get_option(name) == kept, (name, bad)
            else:
                r.set_option(name, bad)
                assert r.get_option(name) == (lo if bad < lo else hi), (name, bad)
    for unknown in (0, 6, 255, 256 + 13):
        with pytest.raises(lp.Error) as e:
            r.set_option(unknown, 1)
        assert e.value.status == A.LPT_ERR_INVALID_ARG
        with pytest.raises(lp.Error):
            r.get_option(unknown)
    r.close()
