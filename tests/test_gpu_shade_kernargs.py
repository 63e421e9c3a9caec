"""-m gpu: k_shade takes its arguments as one struct and re-reads the cold ones from the argument segment where a branch needs them (kernels.h ShadeKernargs,
DESIGN §5.2j).  No arithmetic changed, so every form of k_shade must give the frame it gave before, bit for bit.

The frames: 256 x 144 at 4 samples per pixel, 147 456 primary rays — above path_rays, so the per-bounce k_shade launches run and not k_path (asserted from the stage
counts).  shade_blocks_per_cu = 1 makes a block loop at least three times, so the park, the reservation behind a parked iteration and a last iteration that reserves
alone all run: the sites where qout / sq / ctr are re-read.  packet_primary = 1 makes k_trace_packet trace bounce 0 at this resolution, so bounce 0's k_shade reads the
hits of the kernel that feeds it in the bench frame.

The references, both bit for bit:
 * the CPU oracle (oracle/harness.py), for the forms whose scene it renders: the plain kernels on the Cornell box, dense and at a width that is not a multiple of the
   tile, and the 64 x 36 frame that k_path and the wave-per-ray kernel take;
 * tests/golden/shade_kernargs_frames.json: SHA-256 of the frames the library gave BEFORE the change (written by tests/golden/make_shade_kernargs.py on an MI355X with
   the parent commit's library), for every form: plain, GBUF, ENV, PUNCT, TRANS, EMIS, EMIS + ESAMP, NMAP.  The oracle has no §18 - §24, and k_path no TRANS / EMIS /
   NMAP form, so for those the library's own earlier output is the only bit-exact reference there is; a frame is keyed by pixel slot and does not depend on the grid
   or on the order of the queues, so the digests hold on any device.

`combined` came with the form words (kernel_forms.h): the one case whose word has several bits, ENV | PUNCT | TRANS | EMIS | ESAMP | NMAP, held to the frame of the
library before k_shade's seven bools became that word."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import testing as T
from oracle import harness

from test_gpu_emissive import STAGES
from test_gpu_emitter_sampling import BLACK, CAM, ERig, lamp_floor
from test_gpu_normal_map import DIR as FLOOR_DIR, EYE as FLOOR_EYE, VFOV as FLOOR_VFOV, floor_scene, image4
from test_gpu_transmission import DIR as PANE_DIR, EYE as PANE_EYE, VFOV as PANE_VFOV, add_rect, pane_scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "shade_kernargs_frames.json")
SIZE, SPP, DEPTH = (256, 144), 4, 5
OPTS = {"shade_blocks_per_cu": 1, "packet_primary": 1}
GREY = T.CORNELL_PROBE
PROBE_ENV = np.random.RandomState(5).randint(100, 140, (4, 8, 4)).astype(np.uint8)      # RGBE, not constant: §18's distribution has something to pick from


def _cornell():
    with open(os.path.join(HERE, "golden", "cornell-box.glb"), "rb") as f:
        glb = f.read()
    s = lp.Scene()
    lp.loaders.load_gltf(glb, s)
    s.set_light(0, T.cornell_light())
    return s


def _lamp_and_pane(s):
    """onto the floor scene: an emissive quad above the floor, facing down, and a half-transmissive thin pane 0.7 in front of FLOOR_EYE, across the middle of the view"""
    lamp = s.add_material((0.0, 0.0, 0.0, 1.0), 1.0, 0.0)
    s.set_material_emission(lamp, (1.0, 0.9, 0.7), 6.0)
    add_rect(s, (0.5, 1.2, -1.5), (1, 0, 0), (0, 0, 1), 0.3, 0.3, lamp)
    glass = s.add_material((0.5, 1.0, 0.25, 1.0), 0.3, 0.0)
    s.set_material_transmission(glass, 0.5, 1.5, True)
    add_rect(s, (0.11, 0.505, -0.295), (1, 0, 0), (0, 0.7071, -0.7071), 0.2, 0.15, glass)


CORNELL_CAM = dict(eye=T.CORNELL_EYE, direction=T.CORNELL_DIR, vfov=T.VFOV)
FLOOR_CAM = dict(eye=FLOOR_EYE, direction=FLOOR_DIR, vfov=FLOOR_VFOV)
PANE_CAM = dict(eye=PANE_EYE, direction=PANE_DIR, vfov=PANE_VFOV)
# form -> (scene, probe, camera, what else the rig gets; `size` / `spp`: instead of SIZE / SPP).  One flag of k_shade per case (GBUF: a denoising mode, whose bounce 0 is the GBUF form),
# and `combined`: every flag but GBUF
CASES = {
    "plain": (_cornell, GREY, CORNELL_CAM, {}),
    "gbuf": (_cornell, GREY, CORNELL_CAM, dict(mode=lp.BlitMode.DenoisedPathrace, size=(512, 288), spp=1)),      # a denoised frame is one sample per pixel: the same 147 456 rays
    "env": (_cornell, PROBE_ENV, CORNELL_CAM, dict(env=True)),
    "punct": (lambda: floor_scene(None), GREY, FLOOR_CAM, {}),
    "trans": (lambda: pane_scene(tr=0.5), GREY, PANE_CAM, {}),
    "emis": (lambda: lamp_floor(walls=True), BLACK, CAM, dict(sampling=False)),
    "emis_esamp": (lambda: lamp_floor(walls=True), BLACK, CAM, dict(sampling=True)),
    "nmap": (lambda: floor_scene(image4(), light=False), GREY, FLOOR_CAM, {}),
    "combined": (lambda: floor_scene(image4(), extra=_lamp_and_pane), PROBE_ENV, FLOOR_CAM, dict(env=True, sampling=True)),
}


def render(device, case, size=SIZE, spp=SPP, options=OPTS):
    """one raytrace_n of the case -> (the arrays of the frame, {stage: launches}, the ray counts)"""
    scene, probe, cam, extra = CASES[case]
    extra = dict(extra)
    size, spp = extra.pop("size", size), extra.pop("spp", spp)
    rig = ERig(device, scene(), probe, size=size, depth=DEPTH, options=options, **cam, **extra)
    rig.r.enable_timings(True)
    rig.r.reset_accumulation()
    rig.r.accumulate = True
    rig.r.reset_ray_counts()
    rig.r.raytrace_n(rig.view, spp)
    arrays = [rig.r.read_radiance()]
    if "mode" in extra:
        g, m, rad, _ = rig.r.read_denoiser()
        arrays += [g, m, rad]
    launches = {k: v[1] for k, v in rig.r.timings().items()}
    c = rig.r.ray_counts()
    rig.close()
    return arrays, {k: launches[k] for k in STAGES}, (c.closest, c.shadow, c.shaded)


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def oracle_cornell(size, spp):
    with open(os.path.join(HERE, "golden", "cornell-box.glb"), "rb") as f:
        return harness.render_oracle(f.read(), size[0], size[1], DEPTH, spp)


@pytest.mark.parametrize("case", list(CASES))
def test_every_form_gives_the_frame_it_gave_before(device, case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    arrays, launches, counts = render(device, case)
    assert np.all(np.isfinite(arrays[0])) and arrays[0][..., :3].any()
    # the changed kernels did run: one k_shade launch per bounce, no k_path, bounce 0 by packets
    assert launches["shading"] == DEPTH and launches["path"] == 0 and launches["primary intersection"] == 1, launches
    print("%s: %s closest, %s shadow, %s shaded; %s" % ((case,) + counts + (digest(arrays),)))
    assert list(counts) == want["counts"], (counts, want["counts"])
    assert digest(arrays) == want["sha256"]


def test_plain_frame_equals_the_oracle(device):
    ref, oc = oracle_cornell(SIZE, SPP)
    arrays, launches, counts = render(device, "plain")
    assert launches["shading"] == DEPTH and launches["path"] == 0 and launches["primary intersection"] == 1, launches
    assert counts == (oc.closest, oc.shadow, oc.shaded)
    assert arrays[0].tobytes() == ref.tobytes()


def test_a_width_that_is_no_multiple_of_the_tile(device):
    """250 is no multiple of 8: k_raygen's compacting form fills the queue, the packets are 64 consecutive entries (quad_slots == 0) and the last one is partial"""
    size = (250, 144)
    ref, oc = oracle_cornell(size, SPP)
    arrays, launches, counts = render(device, "plain", size=size)
    assert launches["shading"] == DEPTH and launches["path"] == 0 and launches["primary intersection"] == 1, launches
    assert counts == (oc.closest, oc.shadow, oc.shaded)
    assert arrays[0].tobytes() == ref.tobytes()


@pytest.mark.parametrize("options", [{}, {"path_rays": 0x7FFFFFFF, "coop_rays": 0}, {"path_rays": 0, "coop_rays": 0, "shade_blocks_per_cu": 1, "packet_primary": 1}],
                         ids=["wave_per_ray", "k_path", "k_shade"])
def test_the_small_frame_of_the_other_arms(device, options):
    """64 x 36: the shipped choice (a wave per ray), k_path — which shares shade_hit with k_shade — and the per-bounce launches give the oracle's frame"""
    size = (64, 36)
    ref, oc = oracle_cornell(size, SPP)
    arrays, launches, counts = render(device, "plain", size=size, options=options)
    assert (launches["path"] == 1) == ("path_rays" in options and options["path_rays"] != 0), launches
    assert counts == (oc.closest, oc.shadow, oc.shaded)
    assert arrays[0].tobytes() == ref.tobytes()
