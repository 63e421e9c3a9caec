#!/usr/bin/env python3
"""Punctual lights (SPEC.md §19) on the bench workload: what the PUNCT instantiations of k_shade / k_path cost.

ms per frame at the bench span (synthetic_atrium(seed=2), its sky probe, 1920x1080, 4 spp, depth 8) without punctual lights and with one light of
each type added — a figure to report, not a bar.

usage: python tools/punctual_eval.py [--frames 20] [--rounds 3]   (one GPU; prints one JSON line)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import loupiote_amd as lp  # noqa: E402
from loupiote_amd import scenes, testing as T  # noqa: E402


def frame(r, view, spp):
    r.reset_accumulation()
    r.accumulate = True
    for _ in range(spp):
        r.raytrace(view)
    return r.read_radiance()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = lp.Device(0)
    desc = scenes.synthetic_atrium(seed=2)
    pr = lp.ProbeGPU(dev, desc["probe"], desc["probe"].shape[1], desc["probe"].shape[0])
    view = T.look(desc["camera"]["origin"], desc["camera"]["direction"])
    rs = {}
    for name in ("without", "with"):
        scene = scenes.to_product(desc)
        if name == "with":
            scene.add_punctual_light(lp.point_light((0.0, 2.5, 0.0), color=(1.0, 0.8, 0.6), intensity=30.0, range=20.0))
            scene.add_punctual_light(lp.spot_light((2.0, 4.0, 1.0), (-0.3, -1.0, -0.2), intensity=80.0, inner_angle=0.3, outer_angle=0.6))
            scene.add_punctual_light(lp.directional_light((0.4, -1.0, 0.3), color=(1.0, 0.95, 0.9), intensity=1.5))
        sg = lp.SceneGPU.new_from_scene(scene, dev)
        r = lp.Renderer(dev, (1920, 1080))
        r.downsample_factor = 1.0
        r.resize(dev, sg, pr, (1920, 1080))
        r.set_max_bounces(8)
        r.set_vfov(T.VFOV)
        frame(r, view, 4)   # warm-up
        rs[name] = (r, sg)
    ms = {"without": [], "with": []}
    for _ in range(a.rounds):   # the two scenes alternate, so that drift of the machine lands on both
        for name, (r, _) in rs.items():
            t0 = time.perf_counter()
            for _ in range(a.frames):
                frame(r, view, 4)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    out = {"workload": "synthetic_atrium(seed=2), 1920x1080, 4 spp, depth 8; with = + one point, one spot, one directional light",
           "ms_per_frame_without": ms["without"], "ms_per_frame_with": ms["with"],
           "ratio_of_medians": sorted(ms["with"])[len(ms["with"]) // 2] / sorted(ms["without"])[len(ms["without"]) // 2]}
    print(json.dumps(out))
    for r, sg in rs.values():
        r.close()
        sg.close()
    pr.close()
    dev.close()


if __name__ == "__main__":
    main()
