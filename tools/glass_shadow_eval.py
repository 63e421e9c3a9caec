#!/usr/bin/env python3
"""Shadows through thin glass (SPEC.md §27): what the switch costs and how noisy its light is.

ms per frame of tests/golden/glass-pane.glb (a floor, one thin tinted pane, one solid glass cube, one directional light; 1920x1080, 16 spp, depth 4, a grey probe)
with `set_glass_shadows(True)` against the same renderer with it off, alternating; and the per-pixel standard error of both frames at 16 spp, from independent
frames (seeds 1..N).  Two arms: the file as it is — its sun shines straight down, along the vertical pane, so no shadow ray meets the pane and the difference is
the launch plan's alone (the plain per-lane step instead of packets, the one-round-trip step and the tail in place) — and the same file with the sun turned 45
degrees, so that the pane's shadow lies on the floor and the rays that cross it ask the pane.  Figures to report, not bars.

usage: python tools/glass_shadow_eval.py [--frames 20] [--rounds 3] [--noise-frames 8]   (one GPU; prints one JSON line)
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

SIZE, SPP, DEPTH = (1920, 1080), 16, 4
EYE, DIR = (0.5, 1.2, 5.0), (0.0, -0.15, -1.0)


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
    glb = open(os.path.join(ROOT, "tests", "golden", "glass-pane.glb"), "rb").read()
    dev = lp.Device(0)
    pr = lp.ProbeGPU(dev, T.CORNELL_PROBE, 1, 1)
    view = T.look(EYE, DIR)
    lum = np.array([0.2126, 0.7152, 0.0722])
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": "tests/golden/glass-pane.glb, %dx%d, %d spp, depth %d, grey probe; on / off = set_glass_shadows" % (SIZE + (SPP, DEPTH)), "noise_frames": a.noise_frames}
    for arm in ("as_loaded", "sun_45_degrees"):
        scene = lp.Scene()
        lp.loaders.load_gltf(glb, scene)
        if arm == "sun_45_degrees":
            scene.set_punctual_light(0, lp.directional_light((0.0, -1.0, -1.0), color=(1.0, 0.95, 0.9), intensity=3.0))
        sg = lp.SceneGPU.new_from_scene(scene, dev)
        r = lp.Renderer(dev, SIZE)
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, SIZE)
        r.set_max_bounces(DEPTH)
        r.set_vfov(T.VFOV)
        ms = {"off": [], "on": []}
        for name in ms:
            r.set_glass_shadows(name == "on")
            frame(r, view)   # warm-up
        for _ in range(a.rounds):   # the two settings alternate, so that drift of the machine lands on both
            for name in ms:
                r.set_glass_shadows(name == "on")
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    frame(r, view)
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
        stderr, mean = {}, {}
        for name in ms:
            r.set_glass_shadows(name == "on")
            frames = []
            for seed in range(1, a.noise_frames + 1):
                r.set_seed(seed)
                frames.append(frame(r, view)[..., :3].astype(np.float64) @ lum)
            r.set_seed(0)
            sd = np.std(np.stack(frames), axis=0, ddof=1)
            stderr[name] = {"mean": float(sd.mean()), "p95": float(np.percentile(sd, 95)), "max": float(sd.max())}
            mean[name] = float(np.mean(frames))
        out[arm] = {"ms_per_frame_off": ms["off"], "ms_per_frame_on": ms["on"], "ratio_of_medians": med(ms["on"]) / med(ms["off"]),
                    "stderr_per_pixel_at_%d_spp" % SPP: stderr, "mean_luminance": mean}
        r.close()
        sg.close()
    print(json.dumps(out))
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
