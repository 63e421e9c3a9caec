"""-m gpu: the primary pass of the kernels — k_raygen (compacted at 61x37, dense at 64x32) and bounce-0 shading (`shade_hit` with the
G-buffer, reached from k_path, from the per-bounce k_shade and behind the packet primary kernel: the arms of the `pipeline` fixture) —
against the binary64 reference of tests/primary_ref.py, over the scene and the camera sequence of that module, in DenoisedPathrace and
Temporal, with the blue-noise texture, and sharded three ways with the ranks' buffers summed (SPEC §15.5).  Tolerances, exclusions and
class coverage are those of tests/test_primary_reference.py, which holds the oracle to the same checker.  The debug views
(k_debug_view, BlitMode GBuffer / MotionVector) are compared with their formulas over the buffers they read."""
import numpy as np
import pytest

import loupiote_amd as lp
import primary_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("pipeline")]

MODES = {1: lp.BlitMode.DenoisedPathrace, 2: lp.BlitMode.Temporal}
CASES = [(w, h, mode, "plain") for (w, h) in R.SIZES for mode in (1, 2)] + [R.SIZES[0] + (1, "noise"), R.SIZES[0] + (1, "shard3"), R.SIZES[1] + (2, "shard3")]


@pytest.fixture(scope="module")
def world(device):
    from loupiote_amd import _abi as A
    scene = lp.Scene()
    R.build_scene(scene, scene.add_image, lambda l: scene.set_light(0, R.light_record(A.LIGHT_DT)))
    sg = lp.SceneGPU.new_from_scene(scene, device)
    pr = lp.ProbeGPU(device, np.array([[[64, 64, 64, 128]]], np.uint8), 1, 1)
    yield sg, pr, R.scene_data()[1]
    pr.close()
    sg.close()


def make_renderer(device, sg, pr, w, h, mode, rank=0, world_size=1, noise=False):
    r = lp.Renderer(device, (w, h))
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, (w, h))
    r.set_max_bounces(R.BOUNCES)
    r.set_seed(R.USER_SEED)
    if noise:
        nz = R.noise_texture()
        r.upload_noise_texture(nz, nz.shape[1], nz.shape[0], nz.shape[1] * 4)
        r.use_noise_texture(True)
    if world_size > 1:
        r.set_shard(rank, world_size)
        r.set_resources(device, sg, pr)
    r.set_blit_mode(mode)
    return r


def report(k, what, need, f, worst, lines, bad):
    excluded, classes = R.coverage(f)
    lines.append("frame %d (%s): excluded %.2f %%, compared per class %s, largest error / tolerance %s"
                 % (k, what, 100.0 * excluded, classes, {s: "%.3g" % v for s, v in worst.items()}))
    if excluded > 0.01:
        bad.append("frame %d: %.2f %% of the pixels excluded" % (k, 100.0 * excluded))
    bad += ["frame %d compares no %s pixel" % (k, c) for c in need if classes[c] == 0]
    bad += ["frame %d: %s beyond the tolerance (%.3g)" % (k, s, v) for s, v in worst.items() if not v <= 1.0]


@pytest.mark.parametrize("w,h,mode,arm", CASES, ids=["%dx%d-mode%d-%s" % c for c in CASES])
def test_primary_pass_matches_float64_reference(device, world, w, h, mode, arm):
    sg, pr, sc = world
    n = 3 if arm == "shard3" else 1
    rs = [make_renderer(device, sg, pr, w, h, MODES[mode], rank, n, arm == "noise") for rank in range(n)]
    ref = R.Reference(sc, w, h, R.noise_texture() if arm == "noise" else None)
    lines, bad = [], []
    try:
        for k, (what, view, vfov, need) in enumerate(R.frames()):
            seed = rs[0].frame_state()[1]
            g, m = np.zeros((h, w, 4), np.uint32), np.zeros((h, w, 2), np.float32)
            for r in rs:
                assert r.frame_state()[1] == seed
                r.set_vfov(vfov)
                r.raytrace(view)
                gr, mr, _, _ = r.read_denoiser()
                if n > 1:       # a rank writes its own tiles and leaves zeros elsewhere: the sum is the frame (§15.5)
                    assert np.all((g == 0) | (gr == 0)) and np.all(gr.reshape(-1, 4).any(axis=1) | (mr.reshape(-1, 2) == 0).all(axis=1))
                g += gr
                m += mr
            f = ref.frame(view, vfov, seed)
            report(k, what, need, f, R.check(f, g, m), lines, bad)
    finally:
        for r in rs:
            r.close()
    print("\n".join(lines))
    assert not bad, "\n".join(bad + lines)


def test_debug_views(device, world):
    """BlitMode GBuffer / MotionVector: the frames still pass the checker in these modes, and the blitted bytes are
    `uint8((n·0.5 + 0.5)·255 + 0.5)` of the decoded normal and `clamp(|m|·(W, H)/8)·255` rounded the same way, alpha 255"""
    sg, pr, sc = world
    w, h = R.SIZES[0]
    r = make_renderer(device, sg, pr, w, h, lp.BlitMode.GBuffer)
    ref = R.Reference(sc, w, h)
    lines, bad = [], []
    moved = 0.0
    try:
        for k, (what, view, vfov, need) in enumerate(R.frames()):
            normals = k < 4
            r.set_blit_mode(lp.BlitMode.GBuffer if normals else lp.BlitMode.MotionVector)
            seed = r.frame_state()[1]
            r.set_vfov(vfov)
            r.raytrace(view)
            img = r.blit()
            g, m, _, _ = r.read_denoiser()
            f = ref.frame(view, vfov, seed)
            report(k, what, need, f, R.check(f, g, m), lines, bad)
            assert img.shape == (h, w, 4) and np.all(img[..., 3] == 255)
            if normals:
                assert R.check_normal_view(img, g), "GBuffer view, frame %d" % k
            else:
                assert R.check_motion_view(img, m, w, h) and np.all(img[..., 2] == 0), "MotionVector view, frame %d" % k
                moved = max(moved, float(img[..., :2].max()))
    finally:
        r.close()
    print("\n".join(lines))
    assert not bad, "\n".join(bad + lines)
    assert moved == 255         # the move past the bump and back shifts every surface by far more than the 8 pixels at which the view saturates
