"""-m gpu: the denoiser kernels (k_temporal, k_decode_gbuf, k_atrous, k_composite; SPEC §15.2-15.4) on the seeded edge inputs of
tests/denoise_ref.py, injected into a renderer's filter inputs: per frame, bit for bit against the oracle's passes over the same
inputs (orc.Denoiser.filter), and stage by stage within the tolerance of tests/test_denoise_reference.py against the binary64
reference.  The scene only sizes the buffers: a rank-0-of-2 shard traces its tiles without filtering, then its inputs are
overwritten and `denoise_filter` runs the passes over the whole frame (as after the exchange of a sharded frame)."""
import numpy as np
import pytest

import denoise_ref as R
import loupiote_amd as lp
from loupiote_amd import testing as T

pytestmark = pytest.mark.gpu

CASES = [(w, h, mode) for (w, h) in R.SIZES for mode in (1, 2)] + [R.BIG + (1,)]


@pytest.fixture(scope="module")
def cornell(device, cornell_glb):
    scene = lp.Scene()
    lp.loaders.load_gltf(cornell_glb, scene)
    scene.set_light(0, T.cornell_light())
    sg = lp.SceneGPU.new_from_scene(scene, device)
    pr = lp.ProbeGPU(device, T.CORNELL_PROBE, 1, 1)
    yield sg, pr
    pr.close()
    sg.close()


@pytest.mark.parametrize("w,h,mode", CASES, ids=["%dx%d-mode%d" % c for c in CASES])
def test_denoiser_kernels_on_edge_inputs(device, cornell, w, h, mode):
    import torch
    from loupiote_amd.dist import DevView
    from oracle import orc
    sg, pr = cornell
    r = lp.Renderer(device, (w, h))
    r.downsample_factor = 1.0
    r.resize(device, sg, pr, (w, h))
    r.set_max_bounces(1)
    r.set_vfov(T.VFOV)
    r.set_shard(0, 2)
    r.set_resources(device, sg, pr)
    r.set_blit_mode(lp.BlitMode.DenoisedPathrace if mode == 1 else lp.BlitMode.Temporal)
    dev = torch.device("cuda", 0)
    view = T.look(T.CORNELL_EYE, T.CORNELL_DIR)
    seq = R.sequence(w, h)
    den = orc.Denoiser(None, w, h)
    chk = R.Checker(w, h, mode)
    worst = {}
    try:
        for k in range(len(seq)):
            noisy, gbuf, motion = seq.frame(k)
            r.raytrace(view)
            r.synchronize()
            pn, pg, pm, n = r.denoiser_inputs()
            assert n == w * h
            for ptr, arr, typ in ((pn, noisy, "<f4"), (pg, gbuf.view(np.int32), "<i4"), (pm, motion, "<f4")):
                t = torch.as_tensor(DevView(ptr, arr.size, typ), device=dev)
                t.copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).to(dev))
            torch.cuda.synchronize()
            r.denoise_filter()
            g, m, rad, hist = r.read_denoiser()
            main = r.read_radiance()
            want = den.filter(noisy, gbuf, motion, mode=mode)
            og, om, orad, ohist = den.read()
            assert g.tobytes() == gbuf.tobytes() and m.tobytes() == motion.tobytes(), "inputs not injected, frame %d" % k
            assert np.array_equal(hist, ohist), "history, frame %d" % k
            assert rad.tobytes() == orad.tobytes(), "temporal radiance + variance, frame %d" % k
            assert main.tobytes() == want.tobytes(), "main target, frame %d" % k
            for key, v in chk.frame((noisy, gbuf, motion), rad, hist, main, orc.atrous_pass).items():
                worst[key] = max(worst.get(key, 0.0), v)
    finally:
        r.close()
    print("%dx%d mode %d: largest error / tolerance per stage %s" % (w, h, mode, {key: "%.3g" % v for key, v in worst.items()}))
    bad = {key: v for key, v in worst.items() if not v <= 1.0}
    assert not bad, "stages beyond the tolerance of the binary64 reference: %s" % bad
