#!/usr/bin/env python3
"""Volume attenuation (SPEC.md §28): what the tint of a solid glass costs.

ms per frame of tests/golden/tinted-glass.glb (a floor, one solid glass cube with attenuationColor (0.2, 0.8, 0.4) over attenuationDistance 0.5, one directional
light; 1920x1080, 16 spp, depth 8, a grey probe, the cube filling a third of the frame's height) as loaded against the same file with the attenuation removed
(`set_material_attenuation(material, (1, 1, 1))`: the record's fourth float is 0 and no sigma row is on the device), alternating.  Both scenes shade on the same
TRANS forms of k_shade and trace the same rays — the attenuation draws no random number —, so the difference is the rare branch's own: one record, one sigma row and
three evaluations of the factor per back-face hit.  A figure to report, not a bar.

usage: python tools/volume_eval.py [--frames 20] [--rounds 3]   (one GPU; prints one JSON line)
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
EYE, DIR = (1.5, 0.9, 2.0), (0.0, -0.13, -1.0)      # the cube (centre (1.5, 0.5, -1), edge 1) three units ahead


def frame(r, view):
    r.reset_accumulation()
    r.accumulate = True
    r.raytrace_n(view, SPP)
    return r.read_radiance()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    glb = open(os.path.join(ROOT, "tests", "golden", "tinted-glass.glb"), "rb").read()
    dev = lp.Device(0)
    pr = lp.ProbeGPU(dev, T.CORNELL_PROBE, 1, 1)
    view = T.look(EYE, DIR)
    rs, mean = {}, {}
    for name in ("clear", "tinted"):
        scene = lp.Scene()
        lp.loaders.load_gltf(glb, scene)
        cube = scene.counts().materials - 1
        assert scene.material_attenuation(cube)[2].max() > 0
        if name == "clear":
            scene.set_material_attenuation(cube, (1.0, 1.0, 1.0))
        sg = lp.SceneGPU.new_from_scene(scene, dev)
        r = lp.Renderer(dev, SIZE)
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, SIZE)
        r.set_max_bounces(DEPTH)
        r.set_vfov(T.VFOV)
        mean[name] = [float(c) for c in frame(r, view)[..., :3].astype(np.float64).mean((0, 1))]   # warm-up, and the frame's mean colour
        rs[name] = (r, sg)
    ms = {"clear": [], "tinted": []}
    for _ in range(a.rounds):   # the two scenes alternate, so that drift of the machine lands on both
        for name, (r, _) in rs.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                frame(r, view)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": "tests/golden/tinted-glass.glb, %dx%d, %d spp, depth %d, grey probe; tinted = as loaded, clear = its attenuation removed" % (SIZE + (SPP, DEPTH)),
           "ms_per_frame_clear": ms["clear"], "ms_per_frame_tinted": ms["tinted"], "ratio_of_medians": med(ms["tinted"]) / med(ms["clear"]), "mean_rgb": mean}
    print(json.dumps(out))
    for r, sg in rs.values():
        r.close()
        sg.close()
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
