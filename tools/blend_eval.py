#!/usr/bin/env python3
"""Alpha-blended materials (SPEC.md §26): what a blended scene costs and how noisy it is.

ms per frame of tests/golden/alpha-blend.glb (a floor, one quad with alpha in blocks of 0 / 64 / 128 / 255, one directional light; 1920x1080, 16 spp, depth 4, a grey
probe) loaded with blend=True against the same file loaded plainly (BLEND as opaque: no alpha table, the kernels every scene ran before), alternating; and the per-pixel
standard error of the blended frame at 16 spp, from independent frames (seeds 1..N) — figures to report, not bars.

usage: python tools/blend_eval.py [--frames 20] [--rounds 3] [--noise-frames 8]   (one GPU; prints one JSON line)
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
EYE, DIR = (0.0, 2.2, 3.0), (0.0, -0.6, -1.0)     # above the quad: camera rays meet it, and its graded shadow on the floor is in view


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
    glb = open(os.path.join(ROOT, "tests", "golden", "alpha-blend.glb"), "rb").read()
    dev = lp.Device(0)
    pr = lp.ProbeGPU(dev, T.CORNELL_PROBE, 1, 1)
    view = T.look(EYE, DIR)
    rs = {}
    for name in ("opaque", "blended"):
        scene = lp.Scene()
        lp.loaders.load_gltf(glb, scene, blend=(name == "blended"))
        sg = lp.SceneGPU.new_from_scene(scene, dev)
        r = lp.Renderer(dev, SIZE)
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, SIZE)
        r.set_max_bounces(DEPTH)
        r.set_vfov(T.VFOV)
        frame(r, view)   # warm-up
        rs[name] = (r, sg)
    ms = {"opaque": [], "blended": []}
    for _ in range(a.rounds):   # the two scenes alternate, so that drift of the machine lands on both
        for name, (r, _) in rs.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                frame(r, view)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    # noise: the spread of independent 16-spp frames per pixel, as luminance; the opaque frame's is the floor it is read against
    lum = np.array([0.2126, 0.7152, 0.0722])
    stderr = {}
    for name, (r, _) in rs.items():
        frames = []
        for seed in range(1, a.noise_frames + 1):
            r.set_seed(seed)
            frames.append(frame(r, view)[..., :3].astype(np.float64) @ lum)
        r.set_seed(0)
        sd = np.std(np.stack(frames), axis=0, ddof=1)
        stderr[name] = {"mean": float(sd.mean()), "p95": float(np.percentile(sd, 95)), "max": float(sd.max())}
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": "tests/golden/alpha-blend.glb, %dx%d, %d spp, depth %d, grey probe; blended = load_gltf(blend=True), opaque = the plain load" % (SIZE + (SPP, DEPTH)),
           "ms_per_frame_opaque": ms["opaque"], "ms_per_frame_blended": ms["blended"], "ratio_of_medians": med(ms["blended"]) / med(ms["opaque"]),
           "stderr_per_pixel_at_%d_spp" % SPP: stderr, "noise_frames": a.noise_frames}
    print(json.dumps(out))
    for r, sg in rs.values():
        r.close()
        sg.close()
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
