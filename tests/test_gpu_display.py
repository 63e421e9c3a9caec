"""-m gpu: the display transform and the meter of SPEC §30 on the device.  The renderer's display state (defaults, round trip, refusals that change nothing); the
device hooks lpt_display_probe and lpt_meter_probe against tests/display_ref.py, byte for byte and count for count; a frame of tests/golden/emissive-panel.glb
under a constant probe presented through both launch sites and the denoised mode against the reference applied to the frame's own radiance; a cut frame against
the whole one; the default state against §13.2's encoding; and metering end to end."""
import os

import numpy as np
import pytest

import loupiote_amd as lp
from loupiote_amd import _abi as A, testing as T
from oracle import orc

import display_ref as D

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 63, 255, 257, 1025)
EVS = (-3.0, 0.0, 2.5)
W, H = 96, 64
PROBE4 = np.array([[[128, 128, 128, 131]]], np.uint8)   # RGBE8: 0.5 * 2^3 = radiance 4 in every direction


# ---------------------------------------------------------------------------- the state
def test_display_state_defaults_round_trip_and_refusals(device):
    r = lp.Renderer(device, (32, 16))
    try:
        assert A.lib().lpt_abi_version() == 6
        assert r.display == (0.0, "clamp")
        r.set_display(-2.0, "aces")
        assert r.display == (-2.0, "aces")
        r.set_display(2.5, "pbr_neutral")
        assert r.display == (2.5, "pbr_neutral")
        r.set_display(64.0, D.CLAMP)
        r.set_display(-64.0, "pbr_neutral")
        assert r.display == (-64.0, "pbr_neutral")
        for ev, op in ((0.0, 3), (0.0, 0xFFFFFFFF), (np.nan, 0), (np.inf, 1), (-np.inf, 2), (64.00001, 0), (-65.0, 1), (3e38, 2)):
            with pytest.raises(lp.Error) as e:
                r.set_display(ev, op)
            assert e.value.kind == "InvalidArg"
            assert r.display == (-64.0, "pbr_neutral")        # untouched
        with pytest.raises(lp.Error):
            r.set_display(0.0, "filmic")
        assert A.lib().lpt_renderer_get_display(r._h, None, None) == A.LPT_OK
        r.set_display()
        assert r.display == (0.0, "clamp")
        for low, high in ((-0.1, 0.0), (1.0, 0.0), (0.5, 0.5), (np.nan, 0.0), (0.0, 1.0)):
            with pytest.raises(lp.Error) as e:
                r.meter(low, high)
            assert e.value.kind == "InvalidArg"
    finally:
        r.close()


# ---------------------------------------------------------------------------- the hooks
@pytest.fixture(scope="module")
def edge():
    return D.edge_accumulators(max(SIZES))


@pytest.fixture(scope="module")
def edge_bytes(edge):
    """the reference, once: (op, ev) -> bytes of every case"""
    return {(op, ev): D.display_bytes(edge, ev, op) for op in D.OPERATORS.values() for ev in EVS}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", sorted(D.OPERATORS))
def test_display_probe_equals_the_binary32_reference(device, edge, edge_bytes, op, n):
    for ev in EVS:
        got = device.display_probe(edge[:n], ev, op)
        want = edge_bytes[(D.OPERATORS[op], ev)][:n]
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (ev, bad[:8], edge[bad[:4]], got[bad[:4]], want[bad[:4]])
    # the tail of the largest size alone too: every special case sits in the first cases, every threshold behind them
    if n == max(SIZES):
        assert np.array_equal(device.display_probe(edge[-n // 2:], 0.0, op), edge_bytes[(D.OPERATORS[op], 0.0)][-n // 2:])


def test_display_probe_without_elements_launches_nothing(device):
    assert device.display_probe(np.zeros((0, 4), np.float32), 0.0, "aces").shape == (0, 4)
    hist, skipped = device.meter_probe(np.zeros((0, 4), np.float32))
    assert not hist.any() and skipped == 0
    with pytest.raises(lp.Error) as e:
        device.display_probe(np.zeros((1, 4), np.float32), 65.0, "aces")
    assert e.value.kind == "InvalidArg"


@pytest.fixture(scope="module")
def meter_cases():
    return D.meter_accumulators(max(SIZES))


@pytest.mark.parametrize("n", SIZES)
def test_meter_probe_equals_the_reference_histogram(device, meter_cases, n):
    want, want_skipped = D.histogram(meter_cases[:n])
    hist, skipped = device.meter_probe(meter_cases[:n])
    assert np.array_equal(hist, want) and skipped == want_skipped
    assert int(hist.sum()) + skipped == int(np.count_nonzero(meter_cases[:n, 3] > 0))
    if n == max(SIZES):
        assert hist[0] > 0 and hist[D.BINS - 1] > 0 and skipped > 0      # both ends of the range and the skipped counter are exercised


def test_meter_probe_with_every_pixel_in_one_bin(device):
    """the contention case: every lane's LDS atomic lands on one word"""
    acc = np.tile(np.float32([[0.5, 0.5, 0.5, 1.0]]), (max(SIZES), 1))
    want, want_skipped = D.histogram(acc)
    hist, skipped = device.meter_probe(acc)
    assert np.array_equal(hist, want) and skipped == want_skipped == 0 and np.count_nonzero(hist) == 1 and hist.max() == max(SIZES)
    acc[:, 0] = np.nan                                                 # ... and on the skipped word
    hist, skipped = device.meter_probe(acc)
    assert not hist.any() and skipped == max(SIZES)


# ---------------------------------------------------------------------------- end to end
class Frame:
    """tests/golden/emissive-panel.glb at 96x64, depth 3, under a constant probe of radiance 4"""

    def __init__(self, device, mode=None, options=None, lanes=None):
        self.scene = lp.Scene()
        with open(os.path.join(HERE, "golden", "emissive-panel.glb"), "rb") as f:
            lp.loaders.load_gltf(f.read(), self.scene)
        self.sg = lp.SceneGPU.new_from_scene(self.scene, device)
        self.pr = lp.ProbeGPU(device, PROBE4, 1, 1)
        self.r = r = lp.Renderer(device, (W, H))
        r.downsample_factor = 1.0
        r.resize(device, self.sg, self.pr, (W, H))
        r.set_max_bounces(3)
        for k, v in (options or {}).items():
            r.set_option(k, v)
        if lanes is not None:
            r.set_lanes(lanes)
        if mode is not None:
            r.set_blit_mode(mode)
        self.view = T.look((0.0, 1.0, 6.0), (0.0, -0.05, -1.0))

    def record(self, frames=2):
        """2 frames, recorded and not yet submitted"""
        self.r.reset_accumulation()
        self.r.accumulate = True
        for _ in range(frames):
            self.r.raytrace(self.view)

    def close(self):
        self.r.close()
        self.pr.close()
        self.sg.close()


def ref_bytes(radiance, ev, op):
    return D.display_bytes(radiance.reshape(-1, 4), ev, D.OPERATORS[op]).reshape(radiance.shape[0], radiance.shape[1], 4)


@pytest.fixture(scope="module")
def frame(device):
    f = Frame(device)
    yield f
    f.close()


@pytest.mark.parametrize("op", ["pbr_neutral", "aces"])
def test_both_launch_sites_present_the_reference_of_the_frames_radiance(device, frame, op):
    r = frame.r
    r.set_display(-2.0, op)
    try:
        frame.record()
        assert r.submission_stats()[2] == 2                   # still recorded: read_pixels submits it with its own piecewise read-back
        px = r.read_pixels()
        rad = r.read_radiance()
        want = ref_bytes(rad, -2.0, op)
        assert rad[..., :3].max() > 4.0 and 8 < want[..., :3].mean() < 247   # the frame has radiance far above 1, and the picture is neither black nor white
        assert np.array_equal(px, want)
        assert np.array_equal(r.blit(), want)                 # the same frame again, now submitted: the other launch site
        frame.record()                                        # the next frame (its seeds have moved on), submitted before it is presented
        r.submit()
        assert r.submission_stats()[2] == 0
        got = r.blit()
        rad2 = r.read_radiance()
        want2 = ref_bytes(rad2, -2.0, op)
        assert np.array_equal(got, want2) and np.array_equal(r.read_pixels(), want2) and not np.array_equal(rad2, rad)
        r.set_display(3.0, "clamp")
        assert np.array_equal(r.read_radiance(), rad2)        # the float output is untouched by the display state
        assert np.array_equal(r.blit(), ref_bytes(rad2, 3.0, "clamp"))   # CLAMP away from exposure 0 runs the new kernel too
        assert not np.array_equal(want, ref_bytes(rad, 0.0, "clamp"))
    finally:
        r.set_display()


@pytest.mark.parametrize("op", ["pbr_neutral", "aces"])
def test_the_denoised_mode_presents_the_reference_of_its_own_radiance(device, op):
    f = Frame(device, mode=lp.BlitMode.DenoisedPathrace)
    try:
        f.r.set_display(-2.0, op)
        f.record()
        f.r.submit()
        rad = f.r.read_radiance()
        assert np.array_equal(f.r.blit(), ref_bytes(rad, -2.0, op)) and rad[..., :3].max() > 1.0
    finally:
        f.close()


def test_a_cut_frame_presents_the_bytes_of_the_whole_one(device):
    out = {}
    for lanes in (2, 1):
        f = Frame(device, options={"wavefront_rays": W * H // 2}, lanes=lanes)   # 2 samples x 6144 pixels: four pieces
        try:
            f.r.set_display(-2.0, "pbr_neutral")
            f.record()
            w0 = f.r.submission_stats()[1]
            out[lanes] = f.r.read_pixels()
            assert f.r.submission_stats()[1] - w0 > 1           # the frame did leave in pieces
            assert np.array_equal(out[lanes], ref_bytes(f.r.read_radiance(), -2.0, "pbr_neutral"))
        finally:
            f.close()
    assert np.array_equal(out[1], out[2])


def test_the_default_state_presents_the_old_bytes(device):
    """a renderer whose display was never touched, and one set to (0, CLAMP) by hand: the same bytes, and §13.2's encoding of the radiance (the oracle's tonemap)"""
    fresh = Frame(device)
    try:
        fresh.record()
        a = fresh.r.read_pixels()
        rad = fresh.r.read_radiance()
        assert np.array_equal(a, fresh.r.blit())
    finally:
        fresh.close()
    other = Frame(device)
    try:
        other.r.set_display(0.0, "clamp")
        other.record()
        b = other.r.read_pixels()
        assert np.array_equal(other.r.read_radiance(), rad)
        assert np.array_equal(b, other.r.blit())
    finally:
        other.close()
    want = orc.tonemap(rad.reshape(-1, 4)).reshape(H, W, 4)
    assert np.array_equal(a, b) and np.array_equal(a, want) and np.array_equal(a, ref_bytes(rad, 0.0, "clamp"))
    assert (a[..., :3] == 255).mean() > 0.05                  # what the issue is about: the lit parts of this frame present as flat white


def test_metering_end_to_end(device, frame):
    r = frame.r
    frame.record()
    ev, hist, counted, skipped = r.meter()                    # submits the recorded frame
    assert r.submission_stats()[2] == 0
    rad = r.read_radiance()
    want_hist, want_skipped = D.histogram(rad.reshape(-1, 4))
    want_ev, want_counted = D.evaluate(want_hist, 0.5, 0.02)
    assert np.array_equal(hist, want_hist) and skipped == want_skipped
    assert counted == want_counted > 0 and np.float32(ev).view(np.uint32) == np.float32(want_ev).view(np.uint32)
    assert r.display == (0.0, "clamp")                        # nothing is set behind the caller's back
    r.set_display(-3.0, "aces")
    assert r.meter()[0] == ev                                 # ... and the meter does not depend on the exposure
    means = []
    try:
        for e in (ev - 2.0, ev, ev + 2.0):
            r.set_display(e, "pbr_neutral")
            means.append(float(r.blit()[..., :3].mean()))
    finally:
        r.set_display()
    assert means[0] < means[1] < means[2], means
