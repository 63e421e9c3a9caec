#!/usr/bin/env python3
"""Rough transmission (SPEC.md §29): what frosting a glass costs, in time and in noise.

ms per frame of tests/golden/frosted-glass.glb (a floor, one thin pane of roughnessFactor 0.5, one solid cube of roughnessFactor 0.3, one directional light;
1920x1080, 16 spp, depth 8, a grey probe) loaded with `rough_transmission=True` against the same file loaded without the flag — clear glass, the loader's default —,
alternating; and the per-pixel standard error of the luminance of both at 16 spp, from independent frames (seeds 1..N).  Both scenes shade on the same TRANS forms of
k_shade; what differs is the event (the microfacet normal, Smith's G1) and where the scattered rays go.  Figures to report, not a bar.

usage: python tools/rough_transmission_eval.py [--frames 20] [--rounds 3] [--noise-frames 8]   (one GPU; prints one JSON line)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loupiote_amd as lp  # noqa: E402
from loupiote_amd import testing as T  # noqa: E402

SIZE, SPP, DEPTH = (1920, 1080), 16, 8
EYE, DIR = (0.5, 1.2, 5.0), (0.0, -0.15, -1.0)      # the pane and the cube both in view (tests/test_gpu_rough_transmission.py's camera)


def frame(r, view):
    r.reset_accumulation()
    r.accumulate = True
    r.raytrace_n(view, SPP)
    return r.read_radiance()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--noise-frames", type=int, default=8)
    a = ap.parse_args()
    glb = open(os.path.join(ROOT, "tests", "golden", "frosted-glass.glb"), "rb").read()
    dev = lp.Device(0)
    pr = lp.ProbeGPU(dev, T.CORNELL_PROBE, 1, 1)
    view = T.look(EYE, DIR)
    lum = np.array([0.2126, 0.7152, 0.0722])
    rs = {}
    for name in ("clear", "frosted"):
        scene = lp.Scene()
        lp.loaders.load_gltf(glb, scene, rough_transmission=name == "frosted")
        n = scene.counts().materials
        assert sum(scene.material_transmission_rough(m) for m in range(n)) == (2 if name == "frosted" else 0)
        sg = lp.SceneGPU.new_from_scene(scene, dev)
        r = lp.Renderer(dev, SIZE)
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, SIZE)
        r.set_max_bounces(DEPTH)
        r.set_vfov(T.VFOV)
        frame(r, view)   # warm-up
        rs[name] = (r, sg)
    ms = {"clear": [], "frosted": []}
    for _ in range(a.rounds):   # the two scenes alternate, so that drift of the machine lands on both
        for name, (r, _) in rs.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                frame(r, view)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    stderr, mean = {}, {}
    for name, (r, _) in rs.items():
        frames = []
        for seed in range(1, a.noise_frames + 1):
            r.set_seed(seed)
            frames.append(frame(r, view)[..., :3].astype(np.float64))
        r.set_seed(0)
        sd = np.std(np.stack(frames) @ lum, axis=0, ddof=1)
        stderr[name] = {"mean": float(sd.mean()), "p95": float(np.percentile(sd, 95)), "max": float(sd.max())}
        mean[name] = [float(c) for c in np.mean(frames, axis=(0, 1, 2))]
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": "tests/golden/frosted-glass.glb, %dx%d, %d spp, depth %d, grey probe; frosted = loaded with rough_transmission, clear = without" % (SIZE + (SPP, DEPTH)),
           "ms_per_frame_clear": ms["clear"], "ms_per_frame_frosted": ms["frosted"], "ratio_of_medians": med(ms["frosted"]) / med(ms["clear"]),
           "noise_frames": a.noise_frames, "stderr_per_pixel_at_%d_spp" % SPP: stderr, "mean_rgb": mean}
    print(json.dumps(out))
    for r, sg in rs.values():
        r.close()
        sg.close()
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
